"""GPU: the domain-invariant perceptual loss (vgg_w > 0) -- the two vgg.hip kernel pairs, the frozen VGG16 and the training
step -- against torch on the device (the input transform, bit for bit) and the fp64 oracle of tests/vgg_oracle.py."""
import os
from ctypes import c_size_t

import pytest
import torch
import torch.nn.functional as F

from munit_amd import ops
from oracle import munit_oracle as O
from tests import vgg_oracle as V
from tests.parity import KINK_FRAC, KINK_NOISE, l2err, nerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRID_CAP = 16384 * 256           # vgg_input is a grid-stride loop capped at 16384 blocks of 256 threads


def cl(t):
    return t.float().to(DEV).contiguous(memory_format=torch.channels_last)


@pytest.fixture(scope="module")
def model():
    return V.make_model(0)


@pytest.fixture(scope="module")
def sd(model):
    return V.state(model)


@pytest.fixture(scope="module")
def vgg_dir(tmp_path_factory, model):
    root = tmp_path_factory.mktemp("vgg")
    os.makedirs(str(root / "models"))
    torch.save(model.state_dict(), str(root / "models" / "vgg16.weight"))
    return str(root)


# ------------------------------------------------------------------------------------------------------------------
# vgg_input
# ------------------------------------------------------------------------------------------------------------------
def _torch_preprocess(batch):
    """utils.vgg_preprocess's operations in its order, on the tensor's device in fp32"""
    (r, g, b) = torch.chunk(batch, 3, dim=1)
    batch = torch.cat((b, g, r), dim=1)
    batch = (batch + 1) * 255 * 0.5
    mean = torch.empty_like(batch)
    mean[:, 0, :, :] = 103.939
    mean[:, 1, :, :] = 116.779
    mean[:, 2, :, :] = 123.680
    return batch.sub(mean)


# (batch sizes of the inputs, H, W): two and four inputs, H != W; the last holds 4.4 M values in one input, past one sweep of
# the grid
@pytest.mark.parametrize("sizes,h,w", [((2, 1), 5, 7), ((1, 2, 3, 1), 16, 24), ((1, 3), 768, 640)])
@pytest.mark.parametrize("layout", ["planar", "channels_last"])
def test_vgg_input_is_torch_bit_for_bit(sizes, h, w, layout):
    g = torch.Generator().manual_seed(h + len(sizes))
    xs = [(torch.rand(n, 3, h, w, generator=g) * 2 - 1).to(DEV) for n in sizes]
    if layout == "channels_last":
        xs = [x.contiguous(memory_format=torch.channels_last) for x in xs]
    if (h, w) == (768, 640):
        assert xs[1].numel() > GRID_CAP
    needs = [i % 2 == 1 for i in range(len(xs))]           # every other input takes a gradient
    xd = [x.clone().requires_grad_(n) for x, n in zip(xs, needs)]
    xr = [x.clone().requires_grad_(n) for x, n in zip(xs, needs)]
    y = ops.vgg_input(*xd)
    ref = _torch_preprocess(torch.cat(xr))
    assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y, ref)
    # ... which is the fp64 formula to fp32 rounding: three roundings at magnitudes up to 255 and the fp32 means, against 151
    assert nerr(y, V.preprocess(torch.cat(xs).double().cpu())) < 5e-7
    dy = torch.randn(ref.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    y.backward(dy.contiguous(memory_format=torch.channels_last))
    ref.backward(dy)
    off = 0
    for x, r, n in zip(xd, xr, needs):
        if not n:
            assert x.grad is None
        else:
            assert torch.equal(x.grad, r.grad)
            want = 127.5 * dy[off:off + x.shape[0]].flip(1)           # the channels swapped back
            assert torch.equal(x.grad, want)
        off += x.shape[0]


# ------------------------------------------------------------------------------------------------------------------
# in_mse
# ------------------------------------------------------------------------------------------------------------------
IN_MSE_SHAPES = [(1, 2, 2, 512), (2, 2, 3, 512), (2, 8, 8, 512), (4, 32, 32, 512), (1, 64, 64, 512), (2, 4, 4, 8)]
# Bounds of in_mse against fp64 on the same fp32 inputs.  The statistics and the sum are fp64 in the kernel; what is fp32 is
# mean and 1 / sqrt(var + eps) as stored (one rounding each, 6e-8 relative) and the element-wise chain: three roundings to a
# normalised value, about six more to g and df.  With |n| <= ~5 on planes of up to 4096 pixels that is ~1e-6 of the largest
# gradient element and ~1e-6 relative on the loss, a mean of squares of O(1) differences: 1e-5 for both, the project's bound
# on every loss.
IN_MSE_LOSS_REL = 1e-5
IN_MSE_GRAD = 1e-5


def _in_mse_ref(f, t):
    fr = f.double().clone().requires_grad_(True)
    loss = V.in_mse(fr, t.double())
    loss.backward()
    return loss.detach(), fr.grad


def _in_mse_check(f, t, what):
    """f, t: fp32 CPU tensors (B, C, h, w) -- the fp64 reference starts from the same fp32 values"""
    fd = cl(f).requires_grad_(True)
    td = cl(t)
    loss = ops.in_mse(fd, td)
    loss.backward()
    ref, gref = _in_mse_ref(f, t)
    rel = abs(loss.item() - ref.item()) / abs(ref.item())
    e = nerr(fd.grad.cpu(), gref)
    print("in_mse %s: loss %.6g rel %.2e, grad %.2e" % (what, loss.item(), rel, e))
    assert rel <= IN_MSE_LOSS_REL, (what, loss.item(), ref.item())
    assert e <= IN_MSE_GRAD, (what, e)
    # two runs are bitwise equal
    fd2 = cl(f).requires_grad_(True)
    loss2 = ops.in_mse(fd2, td)
    loss2.backward()
    assert loss2.item() == loss.item() and torch.equal(fd2.grad, fd.grad)
    return loss, fd.grad


@pytest.mark.parametrize("shape", IN_MSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_in_mse_against_fp64(shape):
    b, h, w, c = shape
    g = torch.Generator().manual_seed(b * h * w + c)
    f = torch.randn(b, c, h, w, generator=g) * (0.5 + torch.rand(1, c, 1, 1, generator=g)) + torch.randn(1, c, 1, 1, generator=g)
    t = torch.randn(b, c, h, w, generator=g) * 2 + 0.5
    _in_mse_check(f, t, str(shape))


def test_in_mse_constant_plane_and_large_features():
    g = torch.Generator().manual_seed(5)
    f = torch.randn(2, 512, 8, 8, generator=g)
    t = torch.randn(2, 512, 8, 8, generator=g)
    f[0, 3] = 1.75                  # variance 0: eps carries the division, the normalised plane is 0
    t[1, 7] = -2.5
    f[1, 500] = 0.0
    _, grad = _in_mse_check(f, t, "constant planes")
    assert bool(torch.isfinite(grad).all())
    # features of magnitude 1e3 (relu5_3 of the real network is of order 1e2), not centred
    f = 1e3 * torch.randn(2, 512, 8, 8, generator=g) + 300
    t = 1e3 * torch.randn(2, 512, 8, 8, generator=g).abs()
    _in_mse_check(f, t, "magnitude 1e3")


@pytest.mark.parametrize("shape", [(2, 2, 3, 512), (1, 64, 64, 512)], ids=lambda s: "x".join(map(str, s)))
def test_in_mse_of_a_map_with_itself_is_exactly_zero(shape):
    b, h, w, c = shape
    f = torch.randn(b, c, h, w, generator=torch.Generator().manual_seed(9)) * 37 + 5
    for same_buffer in (True, False):
        fd = cl(f).requires_grad_(True)
        td = fd.detach() if same_buffer else cl(f)
        loss = ops.in_mse(fd, td)
        loss.backward()
        assert loss.item() == 0.0 and torch.count_nonzero(fd.grad) == 0


def test_in_mse_takes_batch_slices_and_refuses_a_target_gradient():
    g = torch.Generator().manual_seed(2)
    f, t = torch.randn(4, 512, 4, 4, generator=g), torch.randn(4, 512, 4, 4, generator=g)
    fd = cl(f).requires_grad_(True)
    parts = ops.split_batch(fd, [2, 2])
    la, lb = ops.in_mse(parts[0], cl(t)[:2]), ops.in_mse(parts[1], cl(t)[2:])
    (la + 3 * lb).backward()
    ra, ga = _in_mse_ref(f[:2], t[:2])
    rb, gb = _in_mse_ref(f[2:], t[2:])
    assert abs(la.item() - ra.item()) <= IN_MSE_LOSS_REL * ra.item() and abs(lb.item() - rb.item()) <= IN_MSE_LOSS_REL * rb.item()
    assert nerr(fd.grad.cpu(), torch.cat([ga, 3 * gb])) <= IN_MSE_GRAD
    td = cl(t).requires_grad_(True)
    with pytest.raises(RuntimeError, match="target takes no gradient"):
        ops.in_mse(cl(f).requires_grad_(True), td).backward()


# ------------------------------------------------------------------------------------------------------------------
# entry-point contract of vgg.hip, through tests/conv_contract.py's Arena: guards and inputs unchanged, outputs fully
# written (two NaN payloads give the same NaN-free bits), a workspace one byte short refused with nothing written, null
# pointers refused
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix", [1, 7 * 13, 1500000])
def test_contract_vgg_input(npix):
    from munit_amd import _lib
    from tests import conv_contract as C
    lib = _lib.load()
    assert 3 * 1500000 > GRID_CAP
    a = C.Arena(dict(x=npix * 12, y=npix * 12, dy=npix * 12, dx=npix * 12), torch.device(DEV))
    C.fill_random(a.view("x", torch.float32), 1)
    C.fill_random(a.view("dy", torch.float32), 2)
    L = C.Launches(a, ["x", "dy"], "vgg_input")
    got = {}
    for fn, src, dst in ((lib.munit_vgg_input_fwd, "x", "y"), (lib.munit_vgg_input_bwd, "dy", "dx")):
        out = a.view(dst, torch.float32)
        C.poison(out, 0)
        L.after(fn(a.ptr(src), a.ptr(dst), c_size_t(npix), C.stream()), dst)
        assert C.no_nan(out)
        first = got[dst] = out.clone()
        C.poison(out, 1)
        L.after(fn(a.ptr(src), a.ptr(dst), c_size_t(npix), C.stream()), dst + ", second payload")
        assert C.bitwise_equal(out, first)
        C.poison(out, 0)
        assert fn(None, a.ptr(dst), c_size_t(npix), C.stream()) == -1
        assert fn(a.ptr(src), None, c_size_t(npix), C.stream()) == -1
        assert fn(a.ptr(dst), a.ptr(dst), c_size_t(npix), C.stream()) == -1          # in place is refused: pixels are permuted
        L.verify("null pointers")
        assert bool((out.view(torch.int32) == C.POISON[4][0]).all())
    x = a.view("x", torch.float32).view(npix, 3)
    assert torch.equal(got["y"].view(npix, 3), (x.flip(1) + 1) * 255 * 0.5
                       - torch.tensor(V.BGR_MEAN, device=DEV, dtype=torch.float32))
    assert torch.equal(got["dx"].view(npix, 3), 127.5 * a.view("dy", torch.float32).view(npix, 3).flip(1))


@pytest.mark.parametrize("shape", [(1, 1, 4), (2, 6, 8), (3, 7, 36), (2, 16, 512), (1, 4096, 512)],
                         ids=lambda s: "x".join(map(str, s)))
def test_contract_in_mse(shape):
    from munit_amd import _lib
    from tests import conv_contract as C
    lib = _lib.load()
    b, hw, c = shape
    n = b * hw * c
    nws = lib.munit_in_mse_workspace_bytes(b, c)
    assert nws >= 8 * b * ((c + 31) // 32)
    a = C.Arena(dict(f=n * 4, t=n * 4, gout=4, out=4, stats=2 * b * c * 2 * 4, df=n * 4, ws=nws), torch.device(DEV))
    C.fill_random(a.view("f", torch.float32), 1)
    C.fill_random(a.view("t", torch.float32), 2)
    a.view("gout", torch.float32).fill_(0.75)
    out, stats, df = (a.view(k, torch.float32) for k in ("out", "stats", "df"))
    L = C.Launches(a, ["f", "t", "gout"], "in_mse %s" % (shape,))

    def fwd(k, ws_bytes=nws, f="f", t="t", o="out", s="stats", ws="ws"):
        a.bytes("ws").fill_(C.GUARD_BYTE)
        C.poison(out, k)
        C.poison(stats, k)
        p = lambda name: a.ptr(name) if name else None
        return lib.munit_in_mse_fwd(p(f), p(t), b, hw, c, p(o), p(s), p(ws), c_size_t(ws_bytes), C.stream())

    L.after(fwd(0), "fwd")
    assert C.no_nan(out) and C.no_nan(stats)
    o0, s0 = out.clone(), stats.clone()
    L.after(fwd(1), "fwd, second payload")
    assert C.bitwise_equal(out, o0) and C.bitwise_equal(stats, s0)
    fr = a.view("f", torch.float32).view(b, hw, c).double()
    st = s0.view(2, b, c, 2)
    assert nerr(st[0, :, :, 0], fr.mean(1)) < 1e-6
    assert nerr(st[0, :, :, 1], 1 / torch.sqrt(fr.var(1, unbiased=False) + 1e-5)) < 1e-6
    L.refused_short(lambda nb: fwd(0, nb), ["out", "stats"], "short workspace")
    for null in ("f", "t", "o", "s", "ws"):
        assert fwd(0, **{null: None}) == -1, null
        L.verify("fwd, null " + null)
        assert bool((out.view(torch.int32) == C.POISON[4][0]).all()) and bool((stats.view(torch.int32) == C.POISON[4][0]).all())
    for bad in ((0, hw, c), (b, 0, c), (b, hw, c + 2), (b, hw, 0)):
        assert lib.munit_in_mse_fwd(a.ptr("f"), a.ptr("t"), *bad, a.ptr("out"), a.ptr("stats"), a.ptr("ws"), c_size_t(nws),
                                    C.stream()) == -1, bad
    L.after(fwd(0), "fwd again")
    L.inputs["stats"] = a.bytes("stats").clone()

    def bwd(k, f="f", t="t", s="stats", g="gout", d="df"):
        C.poison(df, k)
        p = lambda name: a.ptr(name) if name else None
        return lib.munit_in_mse_bwd(p(f), p(t), p(s), b, hw, c, p(g), p(d), C.stream())

    L.after(bwd(0), "bwd")
    assert C.no_nan(df)
    d0 = df.clone()
    L.after(bwd(1), "bwd, second payload")
    assert C.bitwise_equal(df, d0)
    for null in ("f", "t", "s", "g", "d"):
        assert bwd(0, **{null: None}) == -1, null
        L.verify("bwd, null " + null)
        assert bool((df.view(torch.int32) == C.POISON[4][0]).all())
    assert bwd(0, d="f") == -1 and bwd(0, d="t") == -1           # df must not alias an input
    L.verify("bwd, aliased")


# ------------------------------------------------------------------------------------------------------------------
# the convolutions of the network, per kernel form
# ------------------------------------------------------------------------------------------------------------------
_WINO = "conv_wino_kernel<1, 0>"
_FWD = "conv_igemm_kernel<fwd>"
_TAPS3 = "conv_igemm_kernel<.., 5> (3 input channels as 4-channel taps)"
_PATCH = "conv_igemm_kernel<.., 2, 3> (LDS-patch fold)"
# Op cases of the frozen VGG16, (cin, cout, k, stride, pad, act, B, H, W) -> the (forward, backward-data) kernels each was
# added for (tests/test_cpu_vgg.py pins them and requires every form the network reaches, per channel class, to be run by one
# of these), each at a small shape that still has several Winograd tiles / more than one row of pixels per axis.  The first
# layer keeps its three channels: no padding to four.  On even extents (every crop that is a multiple of 8) all other layers
# run Winograd in both passes; an odd extent behind a floor pool (5 x 7 from a 20 x 28 image) takes the implicit GEMM forward
# and the LDS-patch fold backward-data.
VGG_CONV_CASES_TARGETS = {
    (3, 64, 3, 1, 1, "relu", 2, 6, 10): (_TAPS3, _PATCH),                  # conv1_1: 3 -> 64 forward, 64 -> 3 backward-data
    (3, 64, 3, 1, 1, "relu", 2, 5, 7): (_TAPS3, _PATCH),
    (64, 64, 3, 1, 1, "relu", 2, 6, 10): (_WINO, _WINO),                   # conv1_2
    (64, 128, 3, 1, 1, "relu", 2, 4, 6): (_WINO, _WINO),                   # conv2_1
    (128, 128, 3, 1, 1, "relu", 2, 4, 6): (_WINO, _WINO),                  # conv2_2
    (128, 256, 3, 1, 1, "relu", 2, 4, 6): (_WINO, _WINO),                  # conv3_1
    (256, 256, 3, 1, 1, "relu", 2, 4, 6): (_WINO, _WINO),                  # conv3_2, conv3_3
    (256, 512, 3, 1, 1, "relu", 2, 2, 4): (_WINO, _WINO),                  # conv4_1
    (512, 512, 3, 1, 1, "relu", 2, 2, 2): (_WINO, _WINO),                  # conv4_2 .. conv5_3 at a 16-pixel crop
    (512, 512, 3, 1, 1, "relu", 2, 4, 6): (_WINO, _WINO),
    (64, 128, 3, 1, 1, "relu", 2, 10, 14): (_WINO, _WINO),                 # a 20 x 28 image: even after the first pool ...
    (128, 256, 3, 1, 1, "relu", 2, 5, 7): (_FWD, _PATCH),                  # ... odd after the second
    (256, 256, 3, 1, 1, "relu", 2, 5, 7): (_FWD, _PATCH),
    (256, 512, 3, 1, 1, "relu", 2, 2, 3): (_FWD, _PATCH),                  # ... and 2 x 3 after the third
    (512, 512, 3, 1, 1, "relu", 2, 2, 3): (_FWD, _PATCH),
}
VGG_CONV_CASES = list(VGG_CONV_CASES_TARGETS)
SEG_CONV_TOL = 2e-5              # tests/test_gpu_semantic.py's bound for the same kernels


@pytest.mark.parametrize("case", VGG_CONV_CASES, ids=lambda c: "c%d-%d_b%d_%dx%d" % (c[0], c[1], c[6], c[7], c[8]))
def test_vgg_conv_fwd_dgrad(case):
    """ops.frozen_conv(act="relu", sink="vgg") -- bias and ReLU in the epilogue, backward-data through the same weight --
    against F.conv2d in fp64.  Bound: tests/test_gpu_semantic.py's for these kernels, 2e-5 normalised max error or 3 x the
    error of torch's fp32 CPU evaluation of the same case where that is larger.  The ReLU branch is the device's own
    (VGG_SINK), audited against the fp64 sign at rounding-noise margins."""
    from tests.test_gpu_semantic import SEG_CONV_TOL as tol
    assert tol == SEG_CONV_TOL
    cin, cout, k, stride, pad, act, b, h, w = case
    g = torch.Generator().manual_seed(cin + cout + b + h + w)
    wt = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) * (2.0 / (cin * k * k)) ** 0.5
    bias = 0.1 * torch.randn(cout, generator=g, dtype=torch.float64)
    x = torch.randn(b, cin, h, w, generator=g, dtype=torch.float64)
    xd = cl(x).requires_grad_(True)
    with ops.kinks(vgg=True, seg=True) as rec:
        yd = ops.frozen_conv(xd, cl(wt), bias.float().to(DEV), cl(wt), stride, pad, act, sink="vgg")
    assert len(rec.vgg) == 1 and rec.seg == []

    def ref(dtype):
        xr = x.detach().clone().to(dtype).requires_grad_(True)
        return xr, F.conv2d(xr, wt.to(dtype), bias.to(dtype), stride, pad)

    xr, pre = ref(torch.float64)
    dy = torch.randn(pre.shape, generator=g, dtype=torch.float64)
    x32, pre32 = ref(torch.float32)
    mask = rec.vgg[0].cpu()
    flips = mask != (pre.detach() > 0)
    assert not bool((flips & (pre.detach().abs() > 1e-5 * pre.detach().abs().max())).any())
    yr, y32 = pre * mask.double(), pre32 * mask.float()
    yr.backward(dy)
    y32.backward(dy.float())
    yard_f, yard_b = nerr(y32, yr), nerr(x32.grad, xr.grad)
    yd.backward(cl(dy))
    ef, eb = nerr(yd.cpu(), yr), nerr(xd.grad.cpu(), xr.grad)
    print("vgg conv %s: fwd %.2e (fp32 CPU %.2e), dgrad %.2e (fp32 CPU %.2e)" % (case, ef, yard_f, eb, yard_b))
    assert ef <= max(SEG_CONV_TOL, 3 * yard_f), (ef, yard_f)
    assert eb <= max(SEG_CONV_TOL, 3 * yard_b), (eb, yard_b)


# ------------------------------------------------------------------------------------------------------------------
# the network
# ------------------------------------------------------------------------------------------------------------------
# (images, H, W): the smallest crop (a 2 x 2 feature plane), H != W, the step tests' crop, config_256's crop, and a size that
# is no multiple of 8 (20 x 28 -> 10 x 14 -> 5 x 7 -> 2 x 3 by the pools' floor)
NETWORK_SHAPES = [(2, 16, 16), (2, 32, 48), (2, 64, 64), (1, 256, 256), (2, 20, 28)]
# tests/test_gpu_semantic.py's bound on the frozen segmentation network's output and image gradient (normalised max and relative
# L2), which runs the same kernels: kept for relu5_3 and for the image gradient of a fixed linear functional of it (the
# backward-data chain alone).  The image gradient of in_mse goes through the instance norm of planes of 2 x 2 .. 32 x 32
# pixels, which divides by a per-plane deviation that can be far below the map's largest value: a forward error is amplified
# by a factor that belongs to the data, not to the kernels.  That factor is taken from the oracle itself, evaluated in fp32
# on the CPU with the same pinned branches (tools/parity_ref32.py's method): its gradient error per unit of its relu5_3
# error.  The gradient may then be as far off as the admitted forward error makes it: NETWORK_TOL x that factor, and
# never less than NETWORK_TOL.
NETWORK_TOL = 5e-5


@pytest.mark.parametrize("b,h,w", NETWORK_SHAPES)
def test_network_features_and_image_gradient(model, sd, monkeypatch, b, h, w):
    """relu5_3 of b translated images and the gradients of sum(relu5_3 * dz) and of in_mse(vgg(x), vgg(target)) to them, against the fp64 oracle taking
    the device's branch at every ReLU and pool (audited: a disagreement with the oracle's own choice only at rounding-noise
    margins, on a small share of the elements).  The target pass runs under no_grad and asks for no backward-data; no pass
    asks for a weight gradient."""
    calls = {"dgrad": 0}
    dgrad_raw = ops.conv2d_dgrad_raw

    def rec_dgrad(*a, **kw):
        calls["dgrad"] += 1
        return dgrad_raw(*a, **kw)

    def no_wgrad(*a, **kw):
        raise AssertionError("the frozen network asked for a weight gradient")

    monkeypatch.setattr(ops, "conv2d_dgrad_raw", rec_dgrad)
    monkeypatch.setattr(ops, "conv2d_wgrad_raw", no_wgrad)
    net = model                       # stays on the host: it makes its own device copy of the weights
    x, t = V.rand_images(b, h, w, 11), V.rand_images(b, h, w, 12)
    xd = x.float().to(DEV).requires_grad_(True)                  # planar, as a caller may hand it over
    with ops.kinks(vgg=True) as k:
        with torch.no_grad():
            ft = net(cl(t))
        f = net(xd)
    assert len(k.vgg) == 2 * V.N_KINKS
    assert tuple(f.shape) == (b, 512, h // 8, w // 8) and not ft.requires_grad
    pin_t, pin_f = V.vgg_pins(k.vgg[:V.N_KINKS]), V.vgg_pins(k.vgg[V.N_KINKS:])
    # the backward-data chain on its own: the gradient of sum(relu5_3 * dz) for a fixed dz is linear in dz, well conditioned
    dz = torch.randn(f.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    f.backward(cl(dz), retain_graph=True)
    g_lin, xd.grad = xd.grad, None
    loss = ops.in_mse(f, ft)
    loss.backward()
    assert calls["dgrad"] == 26

    xr = x.clone().requires_grad_(True)
    kt, kf = [], []
    with torch.no_grad():
        ftr = V.features(sd, t, kt, pin_t)
    fr = V.features(sd, xr, kf, pin_f)
    fr.backward(dz, retain_graph=True)
    g_lin_ref, xr.grad = xr.grad, None
    e_lin = (nerr(g_lin.cpu(), g_lin_ref), l2err(g_lin, g_lin_ref))
    for kinks, pins in ((kt, pin_t), (kf, pin_f)):
        worst, frac = V.audit(kinks, pins)
        assert worst <= KINK_NOISE and frac <= KINK_FRAC, (worst, frac)
    ref = V.in_mse(fr, ftr)
    ref.backward()
    # the yardstick: the same oracle, same pins, in fp32
    sd32 = V.state(model, torch.float32)
    x32 = x.float().requires_grad_(True)
    with torch.no_grad():
        ft32 = V.features(sd32, t.float(), pins=pin_t)
    f32 = V.features(sd32, x32, pins=pin_f)
    V.in_mse(f32, ft32).backward()
    yard_f = max(nerr(f32, fr.detach()), l2err(f32, fr.detach()))
    yard_g = max(nerr(x32.grad, xr.grad), l2err(x32.grad, xr.grad))
    grad_tol = max(NETWORK_TOL, NETWORK_TOL * yard_g / yard_f)
    e_f = (nerr(f.cpu(), fr.detach()), l2err(f, fr.detach()))
    e_t = (nerr(ft.cpu(), ftr), l2err(ft, ftr))
    e_g = (nerr(xd.grad.cpu(), xr.grad), l2err(xd.grad, xr.grad))
    rel = abs(loss.item() - ref.item()) / ref.item()
    print("vgg network b=%d %dx%d: relu5_3 %.2e max %.2e L2 (target %.2e / %.2e), loss %.6g rel %.2e, image grad %.2e max %.2e L2; "
          "fp32 oracle: relu5_3 %.2e, image grad %.2e -> gradient bound %.2e"
          % (b, h, w, e_f[0], e_f[1], e_t[0], e_t[1], loss.item(), rel, e_g[0], e_g[1], yard_f, yard_g, grad_tol))
    print("vgg network b=%d %dx%d: image gradient of sum(relu5_3 * dz) %.2e max %.2e L2" % (b, h, w, e_lin[0], e_lin[1]))
    assert max(e_f) <= NETWORK_TOL and max(e_t) <= NETWORK_TOL, (e_f, e_t)
    assert max(e_lin) <= NETWORK_TOL, e_lin
    assert rel <= 1e-5, (loss.item(), ref.item())
    assert max(e_g) <= grad_tol, (e_g, grad_tol, yard_f, yard_g)


def test_network_rejects_a_crop_below_16(model):
    with pytest.raises(ValueError, match="at least 16x16"):
        model(torch.zeros(1, 3, 8, 32, device=DEV))


# ------------------------------------------------------------------------------------------------------------------
# the training step
# ------------------------------------------------------------------------------------------------------------------
def _trainer(hp, seed):
    from munit_amd.trainer import MUNIT_Trainer
    torch.manual_seed(seed)
    return MUNIT_Trainer(hp).to(DEV)


def _hp(size, batch, vgg_dir, vgg_w=1):
    hp = O.default_hp(size, batch, 1)
    hp["vgg_w"] = vgg_w
    hp["vgg_model_path"] = vgg_dir
    return hp


def _inputs(b, size, seed):
    g = torch.Generator().manual_seed(seed)
    xa = (torch.rand(b, 3, size, size, generator=g) * 2 - 1).to(DEV)
    xb = (torch.rand(b, 3, size, size, generator=g) * 2 - 1).to(DEV)
    ma = (torch.rand(b, 1, size, size, generator=g) < 0.3).float().to(DEV)
    mb = (torch.rand(b, 1, size, size, generator=g) < 0.3).float().to(DEV)
    return xa, xb, ma, mb


def _step(tr, hp, xa, xb, ma, mb):
    torch.manual_seed(11)
    tr.dis_update(xa, xb, hp)
    tr.gen_update(xa, xb, hp, ma, mb)
    torch.cuda.synchronize()


def _vgg_parity(vgg_dir, model, monkeypatch, size=64, batch=2, gen_state=1, **kw):
    from tests.parity import run_step_parity
    sink = []
    cls = V.oracle_trainer_class(model, lambda: sink)
    monkeypatch.setattr(O, "OracleTrainer", cls)
    with ops.kinks(vgg=sink):
        rep = run_step_parity(size=size, batch=batch, gen_state=gen_state, iters=1, device=DEV, check=False, ref32=True,
                              hp_overrides={"vgg_w": 1, "vgg_model_path": vgg_dir}, **kw)
    worst, frac = cls.audit_worst
    assert worst <= KINK_NOISE and frac <= KINK_FRAC, cls.audit_worst
    assert rep["loss_gen_vgg_a"] > 0 and rep["loss_gen_vgg_b"] > 0
    return rep


@pytest.mark.parametrize("mode", ["default", "gen_state0", "guided0", "extraadam"])
def test_step_parity_with_vgg_loss(vgg_dir, model, monkeypatch, mode):
    """dis_update + gen_update with vgg_w: 1 at 64^2, B = 2, against the fp64 OracleTrainer that adds the two terms through
    its own x_ba / x_ab, with the network's kinks pinned and audited as well; also with two generators (gen_state 0), sampled
    styles (guided 0) and ExtraAdam.  Every loss, the two new ones included, <= 1e-5 relative; the kink audits, Adam moments
    and the weight step keep run_step_parity's bounds.  Generator gradients: the project's 5e-5 normalised max and relative
    L2 per tensor, except where the ORACLE ITSELF evaluated in fp32 (torch CPU, same weights, inputs and pinned branches;
    tools/parity_ref32.py's method) is further than that from fp64 -- there the tensor is held to 2 x the fp32 oracle's
    error, and named when it fails.  Measured: default, gen_state 0 and ExtraAdam 3.1e-6 .. 4.7e-6
    max against the fp32 oracle's 5.5e-6 .. 6.0e-6, so those three are held to 5e-5 flat; guided 0 (sampled styles) 1.26e-4
    max / 1.01e-4 L2 where the fp32 oracle is at 6.5e-4 / 5.2e-4 -- the instance norm of the 8 x 8 relu5_3 planes divides by
    per-plane deviations far below the map's magnitude of 1e2, and that state has such planes."""
    kw = {"default": {}, "gen_state0": dict(gen_state=0), "guided0": dict(guided=0), "extraadam": dict(optimizer="extraadam")}[mode]
    rep = _vgg_parity(vgg_dir, model, monkeypatch, **kw)
    rows = rep["ref32"][0]
    assert len(rows) > 50
    med = lambda k: sorted(r[k] for r in rows)[len(rows) // 2]
    worst = lambda k: max(r[k] for r in rows)
    print("vgg step %s: HIP grad %.2e max %.2e L2, median L2 %.2e; fp32 oracle %.2e max %.2e L2, median L2 %.2e; loss rel %.2e, "
          "vgg_a %.6f vgg_b %.6f, moments %.2e" % (mode, worst(1), worst(2), med(2), worst(3), worst(4), med(4), rep["loss_rel"],
                                                 rep["loss_gen_vgg_a"], rep["loss_gen_vgg_b"], rep["moment_l2"]))
    assert rep["loss_rel"] <= 1e-5, rep["loss_rel"]
    assert rep["kink_worst_rel"] <= KINK_NOISE and rep["kink_disagree_frac"] <= KINK_FRAC
    for name, hip_max, hip_l2, r32_max, r32_l2 in rows:
        assert hip_max <= max(5e-5, 2 * r32_max) and hip_l2 <= max(5e-5, 2 * r32_l2), (name, hip_max, hip_l2, r32_max, r32_l2)
    if mode != "guided0":      # where the fp32 oracle itself meets the project's bound, the step does: no exception in play
        assert worst(3) <= 5e-5 and worst(4) <= 5e-5 and worst(1) <= 5e-5 and worst(2) <= 5e-5, (worst(1), worst(2))
    assert med(2) <= max(1e-5, 2 * med(4)), (med(2), med(4))
    # Adam moments are linear / quadratic in the gradients: twice the per-tensor bound, as run_step_parity holds them
    assert rep["moment_l2"] <= 2 * max(5e-5, 2 * worst(4)), rep["moment_l2"]
    assert rep["weight_abs"] <= 4.0 * 1e-4 and rep["weight_l2"] <= 2e-4, rep


def test_multi_stream_step_with_vgg_loss_is_bitwise_the_single_stream_step(vgg_dir):
    """gen_update joins the two branch streams before the perceptual terms and their backward feeds both decoders: the
    three-stream schedule must not change a bit of the step (tests/test_gpu_step.py's mechanism, vgg_w: 1)."""
    from munit_amd import trainer as T
    hp = _hp(64, 2, vgg_dir)
    xa, xb, ma, mb = _inputs(2, 64, 5)

    def run(streams):
        saved = (ops.SIDE_STREAM_WGRAD, T.BRANCH_STREAMS)
        ops.SIDE_STREAM_WGRAD = T.BRANCH_STREAMS = streams
        try:
            tr = _trainer(hp, 0)
            torch.manual_seed(3)
            for it in range(2):
                tr.iterations = it
                tr.update_learning_rate()
                tr.dis_update(xa, xb, hp)
                tr.gen_update(xa, xb, hp, ma, mb)
            torch.cuda.synchronize()
            return (tr.loss_gen_vgg_a.item(), tr.loss_gen_vgg_b.item(), tr.loss_gen_total.item(), tr.gen_opt.flat_g.clone(),
                    tr.gen_opt.flat_p.clone(), tr.dis_opt.flat_p.clone())
        finally:
            ops.SIDE_STREAM_WGRAD, T.BRANCH_STREAMS = saved

    ref = run(False)
    assert ref[0] > 0 and ref[1] > 0
    for _ in range(2):
        got = run(True)
        assert got[:3] == ref[:3]
        assert all(torch.equal(a, b) for a, b in zip(ref[3:], got[3:]))


def test_reuse_dis_forward_with_vgg_loss_gives_the_plain_steps_losses(vgg_dir):
    """reuse_dis_forward: 1 with vgg_w > 0: the terms take x_ba / x_ab kept from dis_update.  The first iteration's losses
    bit for bit (the two new ones included), the flat generator gradient to 1e-5 relative L2 (the kept nodes are older on
    the tape, so shared weights accumulate in another order): test_reuse_dis_forward_matches_the_plain_step's bounds."""
    from tests.parity import l2err as flat_l2
    batch = _inputs(2, 64, 5)

    def run(reuse):
        hp = _hp(64, 2, vgg_dir)
        hp["reuse_dis_forward"] = reuse
        tr = _trainer(hp, 0)
        tr.update_learning_rate()
        tr.dis_update(batch[0], batch[1], hp)
        tr.gen_update(batch[0], batch[1], hp, batch[2], batch[3])
        assert tr.fwd_reused == bool(reuse)
        torch.cuda.synchronize()
        return tr.gen_opt.flat_g.clone(), {n: float(getattr(tr, n).detach()) for n in vars(tr)
                                           if n.startswith("loss_") and torch.is_tensor(getattr(tr, n))}

    ref, got = run(0), run(1)
    assert ref[1]["loss_gen_vgg_a"] > 0 and ref[1]["loss_gen_vgg_b"] > 0
    assert ref[1] == got[1]
    assert flat_l2(got[0], ref[0]) <= 1e-5, flat_l2(got[0], ref[0])


def test_two_identical_steps_with_vgg_loss_are_bitwise_equal(vgg_dir):
    hp = _hp(64, 2, vgg_dir)
    xa, xb, ma, mb = _inputs(2, 64, 5)
    outs = []
    for _ in range(2):
        tr = _trainer(hp, 0)
        _step(tr, hp, xa, xb, ma, mb)
        outs.append((tr.loss_gen_vgg_a.item(), tr.loss_gen_vgg_b.item(), tr.gen_opt.flat_g.clone(), tr.gen_opt.flat_p.clone()))
    assert outs[0][:2] == outs[1][:2] and outs[0][0] > 0
    assert torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][3], outs[1][3])


def test_vgg_off_launches_no_vgg_kernel(vgg_dir):
    """vgg_w: 0 handed to a trainer that owns the network: nothing of the loss runs (no vgg.hip entry point, no 2x2 max-pool,
    nothing in the vgg channel) and the losses are the reference's int 0; with vgg_w: 1 the same trainer launches them."""
    from munit_amd import _lib
    hp = _hp(64, 2, vgg_dir)
    tr = _trainer(hp, 0)
    assert tr.vgg is not None
    xa, xb, ma, mb = _inputs(2, 64, 3)
    lib = _lib.load()
    names = [n for n in _lib.SIGNATURES if n.startswith(("munit_vgg_", "munit_in_mse_", "munit_maxpool2"))]
    assert len(names) == 7
    calls = []
    saved = {n: getattr(lib, n) for n in names}
    try:
        for n in names:
            setattr(lib, n, (lambda f, n: lambda *a: calls.append(n) or f(*a))(saved[n], n))
        with ops.kinks(vgg=True) as k:
            _step(tr, dict(hp, vgg_w=0), xa, xb, ma, mb)
        assert k.vgg == [] and calls == []
        assert tr.loss_gen_vgg_a == 0 and tr.loss_gen_vgg_b == 0 and not torch.is_tensor(tr.loss_gen_vgg_a)
        with ops.kinks(vgg=True) as k:
            _step(tr, hp, xa, xb, ma, mb)
        assert len(k.vgg) == 2 * V.N_KINKS
        assert calls.count("munit_vgg_input_fwd") == 4 and calls.count("munit_vgg_input_bwd") == 2
        assert calls.count("munit_in_mse_fwd") == 2 and calls.count("munit_in_mse_bwd") == 2
        assert calls.count("munit_maxpool2_fwd") == 6 and calls.count("munit_maxpool2_bwd") == 3
    finally:
        for n, f in saved.items():
            setattr(lib, n, f)
