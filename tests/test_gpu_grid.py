"""GPU: the sample grids -- munit_image_grid_u8 through ops.image_grid and straight through the C ABI, and
munit_amd.utils.write_2images / write_image.  Every comparison is exact, byte for byte: the kernel, the numpy oracle of
tests/grid_oracle.py and the reference's sequence of torch ops run on the device (torchvision's make_grid(normalize=True)
and save_image written out) must agree.  Where the oracle and torch disagree, torch decides (include/munit_hip.h)."""
import os
from ctypes import c_float, c_size_t

import numpy as np
import pytest
import torch

from munit_amd import _lib, ops, utils
from tests import grid_oracle as GO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ----------------------------------------------------------------------------------------------------------------------
# helpers
# ----------------------------------------------------------------------------------------------------------------------
def _device_tensor(x, layout, offset_floats=0):
    """The logical (B, C, H, W) array x as a device tensor whose memory is planar (0) or interleaved (1) and starts
    `offset_floats` floats past the (at least 16-byte aligned) start of its allocation."""
    B, C, H, W = x.shape
    buf = torch.empty(x.size + offset_floats, dtype=torch.float32, device=DEV)
    strides = (C * H * W, H * W, W, 1) if layout == GO.PLANAR else (H * W * C, 1, W * C, C)
    t = buf.as_strided((B, C, H, W), strides, offset_floats)
    t.copy_(torch.from_numpy(x))
    assert buf.data_ptr() % 16 == 0 and t.data_ptr() == buf.data_ptr() + 4 * offset_floats
    return t


def _torch_reference(tensors, nrow, pre_add=0.0, pre_mul=1.0):
    """__write_images (scripts/utils.py:768-784) as torch runs it on the device, torchvision's two calls written out."""
    if (pre_add, pre_mul) != (0.0, 1.0):
        tensors = [(t + pre_add) * pre_mul for t in tensors]
    img = torch.cat([t[:nrow].expand(-1, 3, -1, -1) for t in tensors], 0).clone()
    lo, hi = float(img.min()), float(img.max())
    img.clamp_(lo, hi)
    img.sub_(lo).div_(max(hi - lo, 1e-5))
    nmaps, _, H, W = img.shape
    xmaps, ymaps = GO.grid_shape(nmaps, nrow)
    grid = img.new_zeros((3, ymaps * H, xmaps * W))
    for m in range(nmaps):
        cy, cx = divmod(m, xmaps)
        grid[:, cy * H:(cy + 1) * H, cx * W:(cx + 1) * W].copy_(img[m])
    return grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8)


def _oracle(arrays, layouts, H, W, nrow, pre_add=0.0, pre_mul=1.0):
    return GO.grid_u8([GO.source(x[:nrow], lay) for x, lay in zip(arrays, layouts)], H, W, nrow, pre_add, pre_mul)


def _three_way(arrays, layouts, nrow, pre_add=0.0, pre_mul=1.0, offsets=None, what=""):
    """kernel == torch on the device == numpy oracle, every byte."""
    H, W = arrays[0].shape[2:]
    offsets = offsets or [0] * len(arrays)
    tensors = [_device_tensor(x, lay, off) for x, lay, off in zip(arrays, layouts, offsets)]
    got = ops.image_grid(tensors, nrow, pre_add, pre_mul)
    again = ops.image_grid(tensors, nrow, pre_add, pre_mul)
    ref = _torch_reference(tensors, nrow, pre_add, pre_mul)
    want = torch.from_numpy(_oracle(arrays, layouts, H, W, nrow, pre_add, pre_mul))
    nmaps = sum(min(x.shape[0], nrow) for x in arrays)
    xmaps, ymaps = GO.grid_shape(nmaps, nrow)
    assert got.dtype == torch.uint8 and got.device == tensors[0].device and tuple(got.shape) == (ymaps * H, xmaps * W, 3), what
    assert got.is_contiguous()
    got, again, ref = got.cpu(), again.cpu(), ref.cpu()
    print("%s: kernel != torch %d, oracle != torch %d of %d bytes"
          % (what, int((got != ref).sum()), int((want != ref).sum()), ref.numel()))
    assert torch.equal(want, ref), "%s: the oracle differs from torch in %d bytes" % (what, int((want != ref).sum()))
    assert torch.equal(got, ref), "%s: the kernel differs from torch in %d bytes" % (what, int((got != ref).sum()))
    assert torch.equal(got, again), what + ": two calls differ"
    return got


# (B, C, layout) of every tensor; n = min(B, nrow) takes the values 1, 2 and 3 in one call
SPECS = {
    1: [(3, 3, GO.PLANAR)],
    4: [(1, 3, GO.INTERLEAVED), (2, 1, GO.PLANAR), (3, 3, GO.PLANAR), (3, 1, GO.INTERLEAVED)],
    6: [(4, 3, GO.INTERLEAVED), (4, 3, GO.PLANAR), (2, 1, GO.PLANAR), (4, 3, GO.INTERLEAVED), (1, 3, GO.PLANAR),
        (4, 1, GO.PLANAR)],
}
# (nsrc, nrow): below, equal to and above nmaps; with nrow below B the images past nrow hold +-1e6 and NaN
MIXED = [(1, 3), (1, 2), (1, 5), (4, 2), (4, 9), (4, 12), (6, 3), (6, 1), (6, 19), (6, 24)]


@pytest.mark.parametrize("hw", [(5, 7), (8, 8)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("nsrc,nrow", MIXED, ids=lambda v: str(v))
def test_three_way_mixed_lists(hw, nsrc, nrow):
    """Lists of 1, 4 and 6 tensors of both layouts and both channel counts, n = 1, 2, 3 (and 4) images used per tensor,
    nrow below, equal to and above nmaps; the minimum is the first element of the first image, the maximum the last element
    of the last image used; the third tensor of a list starts 4 bytes past a 16-byte boundary.  Larger and smaller values
    and NaN sit in the images past nrow, which must not count."""
    H, W = hw
    specs = SPECS[nsrc]
    arrays = GO.mixed_batches(100 * nsrc + nrow, H, W, specs, nrow)
    nmaps = sum(min(s[0], nrow) for s in specs)
    assert {(1, 3): nmaps == nrow, (4, 9): nmaps == nrow, (6, 19): nmaps == nrow}.get((nsrc, nrow), True)
    if any(s[0] > nrow for s in specs):
        assert any(np.isnan(x).any() and x[np.isfinite(x)].max() == 1e6 for x in arrays)
    offsets = [1 if i == min(2, nsrc - 1) else 0 for i in range(nsrc)]
    got = _three_way(arrays, [s[2] for s in specs], nrow, offsets=offsets, what="mixed %s nsrc %d nrow %d" % (hw, nsrc, nrow))
    assert got[0, 0, 0] == 0 and got.max() == 255
    xmaps, ymaps = GO.grid_shape(nmaps, nrow)
    cy, cx = divmod(nmaps - 1, xmaps)
    assert got[(cy + 1) * H - 1, (cx + 1) * W - 1, 2] == 255                # the maximum: last element of the last image used
    if xmaps * ymaps > nmaps:
        assert not got[(ymaps - 1) * H:, (cx + 1) * W:].any()                # the zero cells


@pytest.mark.parametrize("shifted", [False, True], ids=["unit", "shifted"])
def test_three_way_rounding_lattice(shifted):
    """For every k in 0..254 the fp32 nearest (k + 0.5) / 255 and its two neighbours, where the byte changes: once with
    lo = 0, hi = 1, once shifted and scaled to lo = -0.9137, hi = 0.8713, where multiplying by the reciprocal and dividing
    differ in the last bit."""
    lo, hi = (-0.9137, 0.8713) if shifted else (0.0, 1.0)
    arrays = GO.lattice_batches(lo, hi)
    got = _three_way(arrays, [GO.PLANAR, GO.INTERLEAVED], 2, what="lattice lo %g hi %g" % (lo, hi))
    if not shifted:
        assert len(np.unique(got.numpy())) == 256                # t = x: both sides of every byte boundary are present


def test_three_way_pre_scale_and_constant():
    """pre_add, pre_mul = 1, 0.5 -- the (x + 1) / 2.0 of scripts/test.py:123 -- on a mixed list and on the lattice; a
    constant input gives a black grid."""
    specs = SPECS[4]
    arrays = GO.mixed_batches(7, 5, 7, specs, 2)
    _three_way(arrays, [s[2] for s in specs], 2, 1.0, 0.5, what="pre-scale mixed")
    _three_way(GO.lattice_batches(-1.0, 1.0), [GO.INTERLEAVED, GO.PLANAR], 2, 1.0, 0.5, what="pre-scale lattice")
    for c in (0.0, 0.37):
        arrays = GO.mixed_batches(8, 5, 7, specs, 3, constant=c)
        got = _three_way(arrays, [s[2] for s in specs], 3, what="constant %g" % c)
        assert not got.any()


def test_sample_shape_against_torch():
    """sample()'s own shape: six channels_last tensors of 2 x 3 x 64 x 64 -- 147456 elements, more than one sweep of the
    range pass's grid (512 x 256 threads)."""
    g = torch.Generator().manual_seed(5)
    tensors = [torch.tanh(2 * torch.randn(2, 3, 64, 64, generator=g)).to(DEV).contiguous(memory_format=torch.channels_last)
               for _ in range(6)]
    assert sum(t.numel() for t in tensors) > 512 * 256
    got = ops.image_grid(tensors, 2)
    ref = _torch_reference(tensors, 2)
    assert tuple(got.shape) == (6 * 64, 2 * 64, 3)
    assert torch.equal(got, ref), "%d bytes differ" % int((got != ref).sum())
    planar = [t.contiguous() for t in tensors]
    assert torch.equal(ops.image_grid(planar, 2), ref)


# ----------------------------------------------------------------------------------------------------------------------
# guard bands
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (4, 5, 7, 2), (6, 8, 8, 3), (3, 33, 21, 9)], ids=lambda s: "n%d_%dx%d_r%d" % s)
def test_contract_image_grid(shape):
    """Every tensor between guard bands (tests/conv_contract.Arena): guards and inputs unchanged, the output prefilled
    with two byte patterns comes out the same (every byte written, the zero cells included), the result does not depend on
    what the workspace held, a workspace one byte short and every MUNIT_ERR_ARG case leave the output untouched."""
    from tests import kernel_contract as KC
    from tests.conv_contract import ERR_WORKSPACE, GUARD_BYTE, Arena, Launches, stream
    lib = _lib.load()
    nsrc, H, W, nrow = shape
    specs = [((1, 2, 3)[i % 3], (3, 1)[i % 2], (GO.PLANAR, GO.INTERLEAVED)[(i // 2) % 2]) for i in range(nsrc)]
    arrays = GO.mixed_batches(31, H, W, specs, nrow)
    srcs = [GO.source(x[:nrow], lay) for x, (_, _, lay) in zip(arrays, specs)]
    nmaps = sum(s["n"] for s in srcs)
    xmaps, ymaps = GO.grid_shape(nmaps, nrow)
    nout = ymaps * H * xmaps * W * 3
    nws = lib.munit_image_grid_workspace_bytes(nsrc, H, W, nrow)
    sizes = {"s%d" % i: s["data"].nbytes for i, s in enumerate(srcs)}
    sizes.update(out=nout, ws=nws)
    a = Arena(sizes, torch.device(DEV))
    for i, s in enumerate(srcs):
        a.view("s%d" % i, torch.float32).copy_(torch.from_numpy(s["data"]))
    what = "image_grid %s" % (shape,)
    L = Launches(a, ["s%d" % i for i in range(nsrc)], what)
    out = a.bytes("out")

    def call(ws_fill=GUARD_BYTE, edit=None, n=None, h=H, w=W, r=nrow, o="out", ws="ws", nb=nws, null_src=False):
        a.bytes("ws").fill_(ws_fill)
        desc = [[a.ptr("s%d" % i).value, s["n"], s["channels"], s["layout"]] for i, s in enumerate(srcs)]
        if edit is not None:
            desc[edit[0]][edit[1]] = edit[2]
        arr = (_lib.GridSrc * len(desc))(*[_lib.GridSrc(*d) for d in desc])
        return lib.munit_image_grid_u8(None if null_src else arr, nsrc if n is None else n, h, w, r, c_float(0.0),
                                       c_float(1.0), a.ptr(o) if o else None, a.ptr(ws) if ws else None, c_size_t(nb), stream())

    res = []
    for fill, ws_fill in ((0x00, GUARD_BYTE), (0xA5, 0x00), (0x5A, 0x7F)):
        out.fill_(fill)
        L.after(call(ws_fill), "output prefilled with 0x%02X, workspace with 0x%02X" % (fill, ws_fill))
        res.append(out.clone())
    assert torch.equal(res[0], res[1]) and torch.equal(res[0], res[2]), what + ": the result depends on the old output or workspace"
    want = torch.from_numpy(GO.grid_u8(srcs, H, W, nrow)).reshape(-1)
    assert torch.equal(res[0].cpu(), want), "%s: %d bytes differ from the oracle" % (what, int((res[0].cpu() != want).sum()))
    last = nsrc - 1
    refusals = [("workspace one byte short", dict(nb=nws - 1), ERR_WORKSPACE), ("src = NULL", dict(null_src=True), KC.ERR_ARG),
                ("out = NULL", dict(o=None), KC.ERR_ARG), ("ws = NULL", dict(ws=None), KC.ERR_ARG),
                ("data = NULL", dict(edit=(last, 0, None)), KC.ERR_ARG), ("nsrc = 0", dict(n=0), KC.ERR_ARG),
                ("nsrc = 17", dict(n=17), KC.ERR_ARG), ("n = 0", dict(edit=(last, 1, 0)), KC.ERR_ARG),
                ("n < 0", dict(edit=(0, 1, -1)), KC.ERR_ARG), ("channels = 2", dict(edit=(last, 2, 2)), KC.ERR_ARG),
                ("channels = 4", dict(edit=(0, 2, 4)), KC.ERR_ARG), ("layout = 2", dict(edit=(last, 3, 2)), KC.ERR_ARG),
                ("layout < 0", dict(edit=(0, 3, -1)), KC.ERR_ARG), ("H = 0", dict(h=0), KC.ERR_ARG),
                ("W < 0", dict(w=-3), KC.ERR_ARG), ("nrow = 0", dict(r=0), KC.ERR_ARG),
                ("output above the limit", dict(h=1 << 15, w=1 << 15), KC.ERR_ARG)]
    for label, kw, code in refusals:
        out.fill_(0xC3)
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc == code, (what, label, rc)
        assert lib.munit_last_error(), (what, label)
        assert bool((out == 0xC3).all()), "%s: output written before the refusal (%s)" % (what, label)
        assert bool((a.bytes("ws") == GUARD_BYTE).all()), "%s: workspace written before the refusal (%s)" % (what, label)
        L.verify(label + " (refused)")


# ----------------------------------------------------------------------------------------------------------------------
# the public names
# ----------------------------------------------------------------------------------------------------------------------
def _files_from_oracle(outputs, nrow, folder):
    """The two files Pillow writes from the oracle's arrays for a write_2images list."""
    from PIL import Image
    n = len(outputs)
    raw = []
    for k, half in enumerate((outputs[:n // 2], outputs[n // 2:])):
        arrays = [t.detach().cpu().numpy() for t in half]
        H, W = arrays[0].shape[2:]
        arr = GO.grid_u8([GO.source(x[:nrow], GO.PLANAR) for x in arrays], H, W, nrow)
        path = os.path.join(folder, "oracle%d.jpg" % k)
        Image.fromarray(arr).save(path)
        raw.append((open(path, "rb").read(), arr.shape))
    return raw


def test_write_2images_on_a_sample_tuple(tmp_path):
    """write_2images on the tuple MUNIT_Trainer.sample returns at 64 x 64, display_size 2 -- as it is, and with a
    one-channel tensor spliced into each half (what the semantic maps' neighbours, the masks, look like): the two files
    hold the bytes Pillow writes from the oracle's arrays, nrow images wide and one image high per tensor."""
    import bench
    from PIL import Image
    from munit_amd.trainer import MUNIT_Trainer
    hp = bench.bench_hp(64, 1)
    hp["display_size"] = 2
    torch.manual_seed(11)
    tr = MUNIT_Trainer(hp).to(DEV)
    x_a, x_b, m_a, m_b = (t.to(DEV) for t in bench.make_batch(2, 64))
    with torch.no_grad():
        outs = tr.sample(x_a, x_b)
    assert len(outs) == 8 and all(tuple(t.shape) == (2, 3, 64, 64) for t in outs)
    spliced = list(outs[:2]) + [m_a] + list(outs[2:6]) + [m_b] + list(outs[6:])
    for tag, lst, rows in (("plain", outs, 4), ("spliced", spliced, 5)):
        folder = tmp_path / tag
        folder.mkdir()
        utils.write_2images(lst, hp["display_size"], str(folder), "test_%08d" % 4)
        want = _files_from_oracle(list(lst), 2, str(tmp_path))
        for name, (raw, shape) in zip(("gen_a2b_test_00000004.jpg", "gen_b2a_test_00000004.jpg"), want):
            path = folder / name
            assert path.is_file(), (tag, name)
            assert open(path, "rb").read() == raw, "%s %s: not the file Pillow writes from the oracle's array" % (tag, name)
            assert Image.open(path).size == (2 * 64, rows * 64) and shape == (rows * 64, 2 * 64, 3)
        assert sorted(os.listdir(folder)) == ["gen_a2b_test_00000004.jpg", "gen_b2a_test_00000004.jpg"]


def test_write_image_equals_the_former_torch_expression(tmp_path):
    """utils.write_image(x, path, 1, 0.5) writes what examples/translate_folder.py's save_image((x + 1) / 2.0, path) wrote
    with torch ops: the expression is evaluated here on the same tensor."""
    from PIL import Image
    g = torch.Generator().manual_seed(3)
    for k, shape in enumerate(((1, 3, 64, 82), (1, 3, 5, 7), (1, 1, 9, 4))):
        x = torch.tanh(torch.randn(shape, generator=g)).to(DEV)
        if k == 0:
            x = x.contiguous(memory_format=torch.channels_last)
        y = ((x + 1) / 2.0)[0].float().expand(3, -1, -1)
        lo, hi = float(y.min()), float(y.max())
        y = (y - lo) / max(hi - lo, 1e-5)
        arr = y.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()
        Image.fromarray(arr).save(tmp_path / "want.jpg")
        utils.write_image(x, str(tmp_path / "got.jpg"), 1.0, 0.5)
        got = ops.image_grid([x], 1, 1.0, 0.5).cpu().numpy()
        assert np.array_equal(got, arr), (shape, int((got != arr).sum()))
        assert open(tmp_path / "got.jpg", "rb").read() == open(tmp_path / "want.jpg", "rb").read(), shape


def test_image_grid_refuses_what_it_cannot_read():
    x = torch.zeros(4, 3, 8, 8, device=DEV)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.image_grid([x, x.cpu()], 2)
    big = torch.zeros(8, 3, 16, 9, device=DEV)
    # 8 x 8 views with a row step, a row pitch and a batch step; one channel of three; one channel repeated without memory
    for bad in (big[:4, :, ::2, :8], big[:4, :, :8, 1:], torch.zeros(8, 3, 8, 8, device=DEV)[::2], x[:, :1],
                x[:, :1].expand(-1, 3, -1, -1)):
        assert tuple(bad.shape[2:]) == (8, 8)
        with pytest.raises(RuntimeError, match="neither planar- nor interleaved-dense"):
            ops.image_grid([x, bad], 2)
    with pytest.raises(RuntimeError, match="float32"):
        ops.image_grid([x.to(torch.bfloat16)], 2)
    with pytest.raises(RuntimeError, match="tensor 1 is 8 x 4"):
        ops.image_grid([x, x[:, :, :, :4].contiguous()], 2)
    with pytest.raises(RuntimeError, match="1 \\| 3"):
        ops.image_grid([torch.zeros(2, 2, 8, 8, device=DEV)], 2)
    # dense slices are read in place
    ref = ops.image_grid([x[1:3].clone()], 2)
    assert torch.equal(ops.image_grid([x[1:3]], 2), ref) and tuple(ref.shape) == (8, 16, 3)


def test_train_loop_example_writes_the_grids(tmp_path):
    """examples/train_loop.py --output-path: two iterations at 64 x 64 with image_save_iter 2 and image_display_iter 1 and
    test folders present -- checkpoints/ and images/ in the reference's layout, the six grids of the cadence, four tensors
    high and display_size images wide; without test folders only the train grids."""
    import sys
    import yaml
    import bench
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.RandomState(9)
    for dom in ("trainA", "trainB", "testA", "testB"):
        (tmp_path / dom).mkdir()
        for k in range(4):
            Image.fromarray(rng.randint(0, 256, (80 + k, 96, 3)).astype(np.uint8)).save(tmp_path / dom / ("i%d.png" % k))
    hp = bench.bench_hp(64, 2)
    hp.update(new_size=64, data_root=str(tmp_path), num_workers=2, ratio_disc_gen=1, display_size=2, image_save_iter=2,
              image_display_iter=1)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump(hp))
    sys.path.insert(0, os.path.join(root, "examples"))
    import train_loop
    out = tmp_path / "outputs" / "cfg"
    tr = train_loop.main(["--config", str(cfg), "--iters", "2", "--output-path", str(out), "--save-every", "2"])
    assert tr.iterations == 1 and sorted(os.listdir(out)) == ["checkpoints", "images"]
    assert sorted(os.listdir(out / "checkpoints")) == ["dis_00000002.pt", "gen_00000002.pt", "optimizer.pt"]
    names = sorted(os.listdir(out / "images"))
    assert names == sorted("gen_%s_%s.jpg" % (d, p) for d in ("a2b", "b2a") for p in ("test_00000002", "train_00000002",
                                                                                    "train_current"))
    for n in names:
        im = Image.open(out / "images" / n)
        assert im.format == "JPEG" and im.size == (2 * 64, 4 * 64), n
        assert np.asarray(im).std() > 1, n                               # a picture, not a flat field
    # no test images, no save cadence: train_current alone
    for dom in ("testA", "testB"):
        for f in os.listdir(tmp_path / dom):
            os.remove(tmp_path / dom / f)
    del hp["image_save_iter"]
    cfg.write_text(yaml.safe_dump(hp))
    out2 = tmp_path / "outputs" / "second"
    train_loop.main(["--config", str(cfg), "--iters", "1", "--output-path", str(out2)])
    assert sorted(os.listdir(out2 / "images")) == ["gen_a2b_train_current.jpg", "gen_b2a_train_current.jpg"]
    assert os.listdir(out2 / "checkpoints") == []
