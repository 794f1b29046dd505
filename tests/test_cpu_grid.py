"""CPU: the sample grids (munit_image_grid_u8, munit_amd.utils.write_2images) without a device -- the numpy oracle of
tests/grid_oracle.py against results written out by hand, the new C symbols and every refusal of the entry point, the
reference's names and parameter lists in munit_amd.utils, and the cadence of examples/train_loop.write_samples."""
import inspect
import os
import re
import sys
from ctypes import c_float, c_size_t, c_void_p

import numpy as np
import pytest

from munit_amd.utils import prepare_sub_folder, write_2images, write_image
from tests import grid_oracle as GO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"munit_image_grid_workspace_bytes": 4, "munit_image_grid_u8": 11}       # name -> arguments in the header
F = np.float32


# ----------------------------------------------------------------------------------------------------------------------
# the oracle against hand-written results
# ----------------------------------------------------------------------------------------------------------------------
def test_oracle_two_by_two_by_hand():
    """One 2 x 2 three-channel image, lo = 0, hi = 1, so t = x and the byte is trunc(x * 255 + 0.5).  0.5 * 255 + 0.5 = 128
    exactly; 0.25 -> 64.25 -> 64; 0.75 -> 191.75 -> 191; 0.1 -> 25.5 + 0.5 rounds to 26.0 in fp32 (0.1f * 255 = 25.500002)."""
    x = np.array([[[[0.0, 1.0], [0.5, 0.25]], [[0.75, 0.1], [0.2, 0.9]], [[1.0, 0.0], [0.3, 0.6]]]], F)
    want = np.array([[[0, 191, 255], [255, 26, 0]], [[128, 51, 77], [64, 230, 153]]], np.uint8)
    got = GO.grid_u8([GO.source(x, GO.PLANAR)], 2, 2, 1)
    assert got.dtype == np.uint8 and got.shape == (2, 2, 3) and np.array_equal(got, want)
    # 0.2 * 255 + 0.5 = 51.5, 0.9 -> 230.0, 0.3 -> 77.0, 0.6 -> 153.5
    # pre_add, pre_mul = 1, 0.5 on 2 x - 1 gives the picture of x, and so does any shift and scale, where fp32 carries them
    # exactly (multiples of 1 / 64 here): the grid is min-max scaled
    xd = (np.round(x * 64) / 64).astype(F)
    base = GO.grid_u8([GO.source(xd, GO.PLANAR)], 2, 2, 1)
    assert np.array_equal(GO.grid_u8([GO.source(2 * xd - 1, GO.PLANAR)], 2, 2, 1, 1.0, 0.5), base)
    assert np.array_equal(GO.grid_u8([GO.source(4 * xd + 8, GO.PLANAR)], 2, 2, 1), base)
    assert np.abs(base.astype(int) - want.astype(int)).max() <= 2 and not np.array_equal(base, want)


def test_oracle_constant_image_is_black():
    """hi == lo: d = 1e-5 and t = 0 / 1e-5 = 0 everywhere."""
    for c in (0.0, 0.37, -5.0):
        got = GO.grid_u8([GO.source(np.full((2, 3, 3, 4), c, F), GO.PLANAR)], 3, 4, 2)
        assert got.shape == (3, 8, 3) and not got.any()


def test_oracle_tiling_order_and_zero_cells():
    """Five images of constant value 0..4 from three sources, nrow 3: a 2 x 3 grid, row-major in list order, the sixth cell
    0.  Image m has t = m / 4: bytes 0, 64, 128, 191, 255."""
    H, W = 2, 3
    img = lambda v: np.full((1, 3, H, W), v, F)                                              # noqa: E731
    srcs = [GO.source(np.concatenate([img(0), img(1)]), GO.PLANAR), GO.source(img(2), GO.INTERLEAVED),
            GO.source(np.concatenate([img(3), img(4)]), GO.INTERLEAVED)]
    got = GO.grid_u8(srcs, H, W, 3)
    assert got.shape == (2 * H, 3 * W, 3) and GO.grid_shape(5, 3) == (3, 2)
    cells = [[int(got[r * H, c * W, 0]) for c in range(3)] for r in range(2)]
    assert cells == [[0, 64, 128], [191, 255, 0]]
    for r in range(2):
        for c in range(3):
            assert (got[r * H:(r + 1) * H, c * W:(c + 1) * W] == cells[r][c]).all()
    # nrow above nmaps: one row of five cells; nrow 1: a column
    assert GO.grid_u8(srcs, H, W, 8).shape == (H, 5 * W, 3) and GO.grid_shape(5, 8) == (5, 1)
    col = GO.grid_u8(srcs, H, W, 1)
    assert col.shape == (5 * H, W, 3) and [int(col[m * H, 0, 0]) for m in range(5)] == [0, 64, 128, 191, 255]


def test_oracle_one_channel_expands_to_three():
    rng = np.random.RandomState(1)
    g = rng.uniform(-1, 1, (2, 1, 3, 5)).astype(F)
    rgb = rng.uniform(-1, 1, (1, 3, 3, 5)).astype(F)
    got = GO.grid_u8([GO.source(g, GO.PLANAR), GO.source(rgb, GO.PLANAR)], 3, 5, 3)
    want = GO.grid_u8([GO.source(np.repeat(g, 3, 1), GO.PLANAR), GO.source(rgb, GO.PLANAR)], 3, 5, 3)
    assert np.array_equal(got, want)
    assert np.array_equal(got[:, :10, 0], got[:, :10, 1]) and np.array_equal(got[:, :10, 0], got[:, :10, 2])
    assert not np.array_equal(got[:, 10:, 0], got[:, 10:, 1])


def test_oracle_layouts_give_the_same_bytes():
    rng = np.random.RandomState(2)
    xs = [rng.uniform(-1, 1, (n, c, 5, 7)).astype(F) for n, c in ((2, 3), (1, 1), (3, 3))]
    grids = [GO.grid_u8([GO.source(x, lay) for x, lay in zip(xs, lays)], 5, 7, 4)
             for lays in ((0, 0, 0), (1, 1, 1), (1, 0, 1), (0, 1, 0))]
    assert all(np.array_equal(g, grids[0]) for g in grids[1:]) and grids[0].any()
    s = GO.source(xs[0], GO.INTERLEAVED)
    assert s["data"][1] == xs[0][0, 1, 0, 0] and GO.source(xs[0], GO.PLANAR)["data"][1] == xs[0][0, 0, 0, 1]
    assert np.array_equal(GO.logical(s, 5, 7), xs[0])


def test_lattice_straddles_every_byte_boundary():
    """The lattice inputs do what they are for: with lo = 0, hi = 1 every byte 0..255 occurs, and the three neighbours of
    each (k + 0.5) / 255 do not all land on one byte for most k (the rounding of * 255 and + 0.5 decides)."""
    v = GO.lattice_values()
    assert v.size == 767 and v.dtype == F and v.min() == 0 and v.max() == 1
    a, b = GO.lattice_batches(0.0, 1.0)
    got = GO.grid_u8([GO.source(a, 0), GO.source(b, 1)], 8, 8, 2)
    assert set(np.unique(got).tolist()) == set(range(256))
    q = (v[:765] * F(255) + F(0.5)).astype(F).astype(np.uint8).reshape(255, 3)
    assert int((q.min(1) != q.max(1)).sum()) > 200
    a, b = GO.lattice_batches(-0.9137, 0.8713)
    assert min(a.min(), b.min()) == F(-0.9137) and max(a.max(), b.max()) == F(0.8713)
    d = F(float(F(0.8713)) - float(F(-0.9137)))
    x = np.concatenate([a.reshape(-1), b.reshape(-1)])
    t = (x - F(-0.9137)).astype(F)
    assert int(((t * F(F(1) / d)).astype(F) != (t / d).astype(F)).sum()) > 0, "reciprocal and division agree everywhere"


# ----------------------------------------------------------------------------------------------------------------------
# symbols and refusals
# ----------------------------------------------------------------------------------------------------------------------
def _lib():
    import __graft_entry__ as g
    g.build()
    from munit_amd import _lib
    return _lib, _lib.load()


def test_new_symbols_in_header_and_library():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "munit_hip.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs and hasattr(lib, name), name
    assert re.search(r"typedef struct \{[^}]*const float\* data;[^}]*int n;[^}]*int channels;[^}]*int layout;[^}]*\} munit_grid_src;",
                     header)
    assert [f[0] for f in L.GridSrc._fields_] == ["data", "n", "channels", "layout"]
    import ctypes
    assert ctypes.sizeof(L.GridSrc) == 24 and L.GridSrc.n.offset == 8 and L.GridSrc.layout.offset == 16


def test_entry_point_refuses_bad_arguments_on_the_host():
    """Every MUNIT_ERR_ARG case and the short workspace are refused before any launch: no GPU is touched (null stream, and
    the device pointers handed over are never dereferenced on the host)."""
    L, lib = _lib()
    p = 4096
    need = lib.munit_image_grid_workspace_bytes(2, 5, 7, 3)
    assert need > 0 and need % 256 == 0
    assert need == lib.munit_image_grid_workspace_bytes(16, 256, 256, 8)          # the partials of a capped grid
    for bad in ((0, 5, 7, 3), (17, 5, 7, 3), (2, 0, 7, 3), (2, 5, -1, 3), (2, 5, 7, 0)):
        assert lib.munit_image_grid_workspace_bytes(*bad) == 0

    def call(srcs=((p, 2, 3, 0), (p, 1, 1, 1)), nsrc=None, h=5, w=7, nrow=3, out=p, ws=p, nb=need, null_src=False):
        arr = (L.GridSrc * max(len(srcs), 1))(*[L.GridSrc(*s) for s in srcs])
        return lib.munit_image_grid_u8(None if null_src else arr, len(srcs) if nsrc is None else nsrc, h, w, nrow,
                                       c_float(0.0), c_float(1.0), c_void_p(out) if out else None,
                                       c_void_p(ws) if ws else None, c_size_t(nb), None)

    one = (p, 1, 3, 0)
    cases = [("src = NULL", dict(null_src=True)), ("out = NULL", dict(out=None)), ("ws = NULL", dict(ws=None)),
             ("data = NULL", dict(srcs=(one, (None, 1, 3, 0)))), ("nsrc = 0", dict(nsrc=0)), ("nsrc < 0", dict(nsrc=-1)),
             ("nsrc = 17", dict(srcs=(one,) * 17)), ("n = 0", dict(srcs=((p, 0, 3, 0),))),
             ("n < 0", dict(srcs=(one, (p, -2, 3, 0)))), ("channels = 2", dict(srcs=((p, 1, 2, 0),))),
             ("channels = 4", dict(srcs=((p, 1, 4, 1),))), ("channels = 0", dict(srcs=((p, 1, 0, 1),))),
             ("layout = 2", dict(srcs=((p, 1, 3, 2),))), ("layout < 0", dict(srcs=((p, 1, 3, -1),))),
             ("H = 0", dict(h=0)), ("W < 0", dict(w=-7)), ("nrow = 0", dict(nrow=0)), ("nrow < 0", dict(nrow=-1)),
             # outputs above 2^31 - 1 bytes: one image of 3 * 2^30; 16 M images of 8 x 8; 2 x 32768 cells of 105 x 105, of
             # which the 32769 images alone would fit
             ("one image above the limit", dict(srcs=(one,), h=1 << 15, w=1 << 15)),
             ("the sum of the sources above the limit", dict(srcs=((p, 1 << 20, 3, 0),) * 16, h=8, w=8, nrow=1 << 30)),
             ("the zero cells above the limit", dict(srcs=((p, (1 << 15) + 1, 1, 0),), h=105, w=105, nrow=1 << 15))]
    for label, kw in cases:
        assert call(**kw) == -1, label
        assert lib.munit_last_error().startswith(b"image_grid"), label
    assert call(nb=need - 1) == -2 and b"workspace" in lib.munit_last_error()
    assert call(nb=0) == -2
    # the largest output still accepted is refused only for its workspace here: 2^31 - 1 >= 3 * H * W * cells
    assert call(srcs=((p, 1, 3, 0),), h=1 << 14, w=1 << 14, nb=0) == -2


# ----------------------------------------------------------------------------------------------------------------------
# host names
# ----------------------------------------------------------------------------------------------------------------------
def test_host_names_have_the_reference_parameter_lists():
    from munit_amd import ops
    sig = inspect.signature(write_2images)
    assert list(sig.parameters) == ["image_outputs", "display_image_num", "image_directory", "postfix", "comet_exp"]
    assert {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty} == {"comet_exp": None}
    assert list(inspect.signature(prepare_sub_folder).parameters) == ["output_directory"]
    sig = inspect.signature(write_image)
    assert list(sig.parameters) == ["x", "path", "pre_add", "pre_mul"]
    assert (sig.parameters["pre_add"].default, sig.parameters["pre_mul"].default) == (0.0, 1.0)
    sig = inspect.signature(ops.image_grid)
    assert list(sig.parameters) == ["tensors", "nrow", "pre_add", "pre_mul"]
    assert (sig.parameters["pre_add"].default, sig.parameters["pre_mul"].default) == (0.0, 1.0)


def test_prepare_sub_folder_creates_both_and_is_idempotent(tmp_path, capsys):
    root = str(tmp_path / "outputs" / "run")
    ckpt, img = prepare_sub_folder(root)
    assert (ckpt, img) == (os.path.join(root, "checkpoints"), os.path.join(root, "images"))
    assert os.path.isdir(ckpt) and os.path.isdir(img) and sorted(os.listdir(root)) == ["checkpoints", "images"]
    assert capsys.readouterr().out.count("Creating directory") == 2
    open(os.path.join(img, "keep.jpg"), "w").close()
    assert prepare_sub_folder(root) == (ckpt, img)
    assert os.listdir(img) == ["keep.jpg"] and capsys.readouterr().out == ""


def test_image_grid_refuses_host_tensors_and_bad_lists():
    import torch
    from munit_amd import ops
    _lib()
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.image_grid([x], 2)
    with pytest.raises(RuntimeError, match="1..16 tensors"):
        ops.image_grid([], 2)
    with pytest.raises(RuntimeError, match="1..16 tensors"):
        ops.image_grid([x] * 17, 2)
    with pytest.raises(RuntimeError, match="nrow"):
        ops.image_grid([x], 0)
    # the layout is read from the strides alone
    assert ops._grid_layout(x) == 0 and ops._grid_layout(x.contiguous(memory_format=torch.channels_last)) == 1
    assert ops._grid_layout(x[:1]) == 0 and ops._grid_layout(x[1:]) == 0 and ops._grid_layout(x[:, :1]) is None
    assert ops._grid_layout(x[:, :, ::2]) is None and ops._grid_layout(x[:, :, :, 1:]) is None
    assert ops._grid_layout(x[::2]) == 0                                 # one image left: its batch stride does not matter
    assert ops._grid_layout(torch.zeros(3, 3, 4, 4)[::2]) is None
    assert ops._grid_layout(torch.zeros(2, 1, 4, 4).expand(-1, 3, -1, -1)) is None
    assert ops._grid_layout(torch.zeros(2, 1, 4, 4)) == 0
    assert ops._grid_layout(torch.zeros(2, 4, 4, 3).permute(0, 3, 1, 2)) == 1


# ----------------------------------------------------------------------------------------------------------------------
# cadence
# ----------------------------------------------------------------------------------------------------------------------
class _StubTrainer(object):
    def __init__(self):
        self.calls = []

    def sample(self, x_a, x_b):
        import torch
        assert not torch.is_grad_enabled()
        self.calls.append((x_a, x_b))
        return ("out", x_a, x_b)


def _cadence(config, displays, rank, iters=12):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_loop
    tr, written = _StubTrainer(), []

    def write(outputs, n, directory, postfix, comet_exp=None):
        written.append((postfix, outputs[1:], n, directory))

    for it in range(iters):
        train_loop.write_samples(tr, config, it, displays, "imgdir", rank, write)
    return tr, written


def test_cadence_of_the_sample_grids():
    config = dict(display_size=5, image_save_iter=4, image_display_iter=3)
    displays = ("train_a", "train_b", "test_a", "test_b")
    tr, written = _cadence(config, displays, 0)
    assert [w[0] for w in written] == ["train_current", "test_00000004", "train_00000004", "train_current", "test_00000008",
                                       "train_00000008", "train_current", "test_00000012", "train_00000012", "train_current"]
    assert all(w[2] == 5 and w[3] == "imgdir" for w in written)
    assert all(w[1] == (("test_a", "test_b") if w[0].startswith("test") else ("train_a", "train_b")) for w in written)
    # the test pair is sampled before the train pair, as the reference does (the styles come from one RNG stream)
    assert tr.calls == [("train_a", "train_b"), ("test_a", "test_b"), ("train_a", "train_b"), ("train_a", "train_b"),
                        ("test_a", "test_b"), ("train_a", "train_b"), ("train_a", "train_b"),
                        ("test_a", "test_b"), ("train_a", "train_b"), ("train_a", "train_b")]
    # another rank samples just as often and writes nothing
    tr1, written1 = _cadence(config, displays, 1)
    assert written1 == [] and tr1.calls == tr.calls
    # no test images: the train grids alone
    tr2, written2 = _cadence(config, ("train_a", "train_b", None, None), 0)
    assert [w[0] for w in written2] == [w[0] for w in written if not w[0].startswith("test")]
    assert tr2.calls == [c for c in tr.calls if c[0] == "train_a"]
    # a cadence key that is absent or 0 writes nothing
    for cfg in (dict(display_size=5), dict(display_size=5, image_save_iter=0, image_display_iter=0)):
        tr3, written3 = _cadence(cfg, displays, 0)
        assert written3 == [] and tr3.calls == []
    tr4, written4 = _cadence(dict(display_size=5, image_save_iter=6), displays, 0)
    assert [w[0] for w in written4] == ["test_00000006", "train_00000006", "test_00000012", "train_00000012"]


def test_write_2images_splits_the_list_and_logs_to_comet(tmp_path, monkeypatch):
    """The host side alone, with ops.image_grid stubbed: first half -> gen_a2b, second half -> gen_b2a, one grid call per
    file with nrow = display_image_num, both files logged to a comet experiment when one is given."""
    import torch
    from PIL import Image
    from munit_amd import ops, utils
    calls = []

    def grid(tensors, nrow, pre_add=0.0, pre_mul=1.0):
        calls.append((list(tensors), nrow, pre_add, pre_mul))
        return torch.full((4, 6, 3), 40 * len(calls), dtype=torch.uint8)

    monkeypatch.setattr(ops, "image_grid", grid)

    class Comet(object):
        logged = []

        def log_image(self, path):
            self.logged.append(path)

    outs = ["a0", "a1", "a2", "b0", "b1", "b2"]
    utils.write_2images(outs, 2, str(tmp_path), "test_00000004")
    assert calls == [(["a0", "a1", "a2"], 2, 0.0, 1.0), (["b0", "b1", "b2"], 2, 0.0, 1.0)]
    names = ["gen_a2b_test_00000004.jpg", "gen_b2a_test_00000004.jpg"]
    assert sorted(os.listdir(tmp_path)) == names and Comet.logged == []
    for k, n in enumerate(names):
        im = Image.open(tmp_path / n)
        assert im.format == "JPEG" and im.size == (6, 4) and abs(int(np.asarray(im)[0, 0, 0]) - 40 * (k + 1)) <= 2
    utils.write_2images(outs, 2, str(tmp_path), "train_current", Comet())
    assert Comet.logged == ["%s/gen_a2b_train_current.jpg" % tmp_path, "%s/gen_b2a_train_current.jpg" % tmp_path]
    del calls[:]
    utils.write_image(torch.zeros(1, 3, 4, 6), str(tmp_path / "one.jpg"), 1.0, 0.5)
    assert len(calls) == 1 and calls[0][1:] == (1, 1.0, 0.5) and os.path.isfile(tmp_path / "one.jpg")
    with pytest.raises(ValueError):
        utils.write_image(torch.zeros(2, 3, 4, 6), str(tmp_path / "two.jpg"))
