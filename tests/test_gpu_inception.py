"""The Inception-v3 feature trunk of FID evaluation on the GPU (csrc/inception.hip through munit_amd.ops,
munit_amd/inception.py, munit_amd/inception_utils.py).

The rectangular convolution is pinned three ways, like the dense product of tests/test_gpu_fid.py: bit for bit on
integer-lattice data (taps, pads, strides, tails, channel slices -- no tolerance), elementwise under the fmaf-chain bound
(K + 2) 2^-24 (|x| * |w| + |bias|) on random data, and under the guard-band contract of tests/conv_contract.py.  The whole
trunk is held against tests/inception_oracle.py in fp64 with the allowance max(16 e32, 16 * 2^-24 max|ref|), e32 being the
error of the same oracle in fp32 on the CPU for the same case.  Every test prints the figures it asserts on."""
import functools
from ctypes import byref, c_void_p

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_contract as CC
from tests import fid_oracle as FO
from tests import inception_oracle as IO
from tests.lattice import lattice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# every filter form of the network: (KH, KW, stride, pad_h, pad_w)
FORMS = [(3, 3, 2, 0, 0), (3, 3, 1, 0, 0), (3, 3, 1, 1, 1), (1, 1, 1, 0, 0), (5, 5, 1, 2, 2),
         (1, 7, 1, 0, 3), (7, 1, 1, 3, 0), (1, 3, 1, 0, 1), (3, 1, 1, 1, 0)]
CHANNELS = [(3, 32), (16, 80), (48, 192)]
# (B, H, W, Cin, Cout, form): B = 2 with H != W, both odd; the last spans several tiles in both directions (M = 289, K = 896)
CONV_CASES = [(2, 9, 11, ci, co, f) for f in FORMS for ci, co in CHANNELS] + [(1, 17, 17, 128, 192, (1, 7, 1, 0, 3))]
TILES = (None, "128x128", "64x64", "128x64")
X_EXTRA, X_LO, Y_EXTRA, Y_LO = 16, 8, 24, 16       # the sliced run: x_ld = Cin + 16 read at 8, y_ld = Cout + 24 written at 16


def _case_id(c):
    return "b%d_%dx%d_c%d-%d_k%dx%ds%dp%d-%d" % (c[:5] + c[5])


@functools.lru_cache(maxsize=None)
def _conv_data(case, kind):
    """fp64 (x NCHW, w OIHW, bias, pre-activation reference, |x| * |w| + |bias|) of a case; kind "lattice" or "random"."""
    b, h, w, cin, cout, (kh, kw, s, ph, pw) = case
    seed = 1000 * cin + 10 * kh + kw + s
    if kind == "lattice":
        x, wt = lattice((b, cin, h, w), seed, range(-3, 4)), lattice((cout, cin, kh, kw), seed + 1, range(-3, 4))
        bias = lattice((cout,), seed + 2, range(-8, 9))
    else:
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(b, cin, h, w, generator=g).double()
        wt = torch.randn(cout, cin, kh, kw, generator=g).double()
        bias = torch.randn(cout, generator=g).double()
    pre = F.conv2d(x, wt, bias, stride=s, padding=(ph, pw))
    mag = F.conv2d(x.abs(), wt.abs(), bias.abs(), stride=s, padding=(ph, pw))
    return x, wt, bias, pre, mag


def _pixels(nchw, extra, lo, payload):
    """A poisoned (B, H, W, C + extra) device buffer holding nchw's channels at [lo, lo + C), and the slice view."""
    b, c, h, w = nchw.shape
    buf = torch.empty((b, h, w, c + extra), dtype=torch.float32, device=DEV)
    CC.poison(buf, payload)
    view = buf[..., lo:lo + c]
    view.copy_(nchw.permute(0, 2, 3, 1).float())
    return buf, view


def _run_conv(case, data, relu, sliced, tile, payload=0):
    """(result as NCHW on the host, the output buffer, its slice bounds).  sliced: False (dense), True (the sliced run above) or
    (x_extra, x_lo, y_extra, y_lo)."""
    from munit_amd import ops
    x, wt, bias = data[:3]
    b, h, w, cin, cout, (kh, kw, s, ph, pw) = case
    x_extra, x_lo, y_extra, lo = sliced if isinstance(sliced, tuple) else ((X_EXTRA, X_LO, Y_EXTRA, Y_LO) if sliced else (0,) * 4)
    _, xv = _pixels(x, x_extra, x_lo, payload)
    ho, wo = data[3].shape[2:]
    ybuf = torch.empty((b, ho, wo, cout + y_extra), dtype=torch.float32, device=DEV)
    CC.poison(ybuf, payload)
    out = ops.conv2d_rect(xv, ops.rect_weight_image(wt.float()).to(DEV), bias.float().to(DEV), kh, kw, s, ph, pw, relu=relu,
                          out=ybuf[..., lo:lo + cout], tile=tile)
    torch.cuda.synchronize()
    return out.permute(0, 3, 1, 2).cpu(), ybuf, (lo, lo + cout)


def _unwritten_intact(ybuf, bounds, payload):
    lo, hi = bounds
    raw = ybuf.view(torch.int32)
    return bool((raw[..., :lo] == CC.POISON[4][payload]).all()) and bool((raw[..., hi:] == CC.POISON[4][payload]).all())


@pytest.mark.parametrize("case", CONV_CASES, ids=_case_id)
def test_conv_rect_lattice_is_bit_exact(case):
    data = _conv_data(case, "lattice")
    pre, mag = data[3], data[4]
    assert float(mag.max()) < 2.0 ** 24          # every partial sum is an integer below 2^24: exact in any order
    for relu in (False, True):
        want = (pre.clamp_min(0) if relu else pre).float()
        for sliced in (False, True):
            for tile in TILES:
                got, ybuf, bounds = _run_conv(case, data, relu, sliced, tile)
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (relu, sliced, tile)
                assert _unwritten_intact(ybuf, bounds, 0), (relu, sliced, tile)


@pytest.mark.parametrize("case", CONV_CASES, ids=_case_id)
def test_conv_rect_random_within_the_chain_bound(case):
    data = _conv_data(case, "random")
    b, h, w, cin, cout, (kh, kw, s, ph, pw) = case
    k = kh * kw * cin
    # the operands as the kernel gets them: rounded to fp32
    x32, w32, b32 = (t.float().double() for t in data[:3])
    pre = F.conv2d(x32, w32, b32, stride=s, padding=(ph, pw))
    bound = (k + 2) * FO.U32 * F.conv2d(x32.abs(), w32.abs(), b32.abs(), stride=s, padding=(ph, pw))
    worst = 0.0
    for relu in (False, True):
        want = pre.clamp_min(0) if relu else pre           # ReLU is 1-Lipschitz: the bound carries over
        for sliced in (False, True):
            for tile in TILES:
                got, _, _ = _run_conv(case, data, relu, sliced, tile)
                worst = max(worst, float(((got.double() - want).abs() / bound).max()))
    print("conv_rect %s: K %d worst error / chain bound %.3f" % (_case_id(case), k, worst))
    assert worst <= 1.0


# Cin % 4 == 0 but no 128-bit gather: a slice that starts at channel 2 (pointer 8 bytes off), and a per-pixel stride that is
# no multiple of 4 -- the word-load path that otherwise only the 3-channel layer takes; y at an odd offset and stride as well
MISALIGNED = [(16, 2, 5, 3), (6, 4, 5, 3)]
MISALIGNED_CASES = [(2, 9, 11, 16, 80, (1, 7, 1, 0, 3)), (2, 9, 11, 48, 192, (3, 3, 2, 0, 0)), (2, 9, 11, 16, 80, (5, 5, 1, 2, 2)),
                    (1, 17, 17, 128, 192, (1, 7, 1, 0, 3))]


@pytest.mark.parametrize("case", MISALIGNED_CASES, ids=_case_id)
@pytest.mark.parametrize("layout", MISALIGNED, ids=lambda l: "x+%d@%d_y+%d@%d" % l)
def test_conv_rect_lattice_on_misaligned_slices(case, layout):
    data = _conv_data(case, "lattice")
    assert float(data[4].max()) < 2.0 ** 24
    want = data[3].clamp_min(0).float()
    for tile in TILES:
        got, ybuf, bounds = _run_conv(case, data, True, layout, tile)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), tile
        assert _unwritten_intact(ybuf, bounds, 0), tile


def test_conv_rect_tile_choice_and_override_agree_bitwise():
    """The host chooses by workgroup count: the small tile while 128 x 128 tiles would not fill the device, beyond that the
    128-row tile that pads Cout least; all give the same bits (the chain does not depend on the tile)."""
    from munit_amd import ops
    assert ops.conv2d_rect_tile(1, 17, 17, 768, 192, 1, 1) == "64x64"
    assert ops.conv2d_rect_tile(1, 8, 8, 2048, 320, 1, 1) == "64x64"
    assert ops.conv2d_rect_tile(32, 35, 35, 64, 96, 3, 3, 1, 1, 1) == "128x128"
    assert ops.conv2d_rect_tile(32, 147, 147, 32, 64, 3, 3, 1, 1, 1) == "128x64"           # pads Cout = 64 less
    assert ops.conv2d_rect_tile(32, 71, 71, 80, 192, 3, 3) == "128x64" and ops.conv2d_rect_tile(32, 73, 73, 64, 80, 1, 1) == "128x128"
    case = (1, 17, 17, 128, 192, (1, 7, 1, 0, 3))
    data = _conv_data(case, "random")
    a, b, c = (_run_conv(case, data, True, False, t)[0] for t in ("128x128", "64x64", "128x64"))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))


CONTRACT_CASES = [(2, 9, 11, 3, 32, (3, 3, 2, 0, 0)), (2, 9, 11, 16, 80, (1, 7, 1, 0, 3)), (2, 9, 11, 48, 192, (7, 1, 1, 3, 0)),
                  (2, 9, 11, 16, 80, (5, 5, 1, 2, 2)), (1, 17, 17, 128, 192, (1, 7, 1, 0, 3))]


@pytest.mark.parametrize("case", CONTRACT_CASES, ids=_case_id)
@pytest.mark.parametrize("tile", [0, 1, 2], ids=["128x128", "64x64", "128x64"])
def test_conv_rect_contract(case, tile):
    """Guard bands around every buffer, NaN in the channels of x outside the read slice and of y outside the written one."""
    from munit_amd import _lib
    lib = _lib.load()
    b, h, w, cin, cout, (kh, kw, s, ph, pw) = case
    x_ld, y_ld = cin + X_EXTRA, cout + Y_EXTRA
    ho, wo = (h + 2 * ph - kh) // s + 1, (w + 2 * pw - kw) // s + 1
    k = kh * kw * cin
    a = CC.Arena(dict(x=b * h * w * x_ld * 4, w=k * cout * 4, bias=cout * 4, y=b * ho * wo * y_ld * 4), DEV)
    xb, yb = a.view("x", torch.float32).view(b, h, w, x_ld), a.view("y", torch.float32).view(b, ho, wo, y_ld)
    CC.fill_random(a.view("w", torch.float32), 12)
    CC.fill_random(a.view("bias", torch.float32), 13)
    vals = torch.randn(b, h, w, cin, generator=torch.Generator().manual_seed(11)).to(DEV)
    d = _lib.RectDesc(b, h, w, cin, x_ld, cout, y_ld, kh, kw, s, ph, pw, 1)
    outs = []
    for payload in (0, 1):
        CC.poison(xb, payload)
        xb[..., X_LO:X_LO + cin] = vals
        CC.poison(yb, payload)
        L = CC.Launches(a, ["x", "w", "bias"], "conv_rect %s" % (case,))
        xp = c_void_p(a.ptr("x").value + 4 * X_LO)
        yp = c_void_p(a.ptr("y").value + 4 * Y_LO)
        L.after(lib.munit_conv2d_rect_fwd(byref(d), xp, a.ptr("w"), a.ptr("bias"), yp, tile, CC.stream()), "payload %d" % payload)
        assert _unwritten_intact(yb, (Y_LO, Y_LO + cout), payload)
        out = yb[..., Y_LO:Y_LO + cout].clone()
        assert CC.no_nan(out)
        outs.append(out)
    assert CC.bitwise_equal(outs[0], outs[1])


# ---- pools -------------------------------------------------------------------------------------------------------------
def _run_pool(x, mode, stride, pad, sliced, payload=0):
    from munit_amd import ops
    b, c, h, w = x.shape
    _, xv = _pixels(x, X_EXTRA if sliced else 0, X_LO if sliced else 0, payload)
    ho, wo = (h + 2 * pad - 3) // stride + 1, (w + 2 * pad - 3) // stride + 1
    ybuf = torch.empty((b, ho, wo, c + (Y_EXTRA if sliced else 0)), dtype=torch.float32, device=DEV)
    CC.poison(ybuf, payload)
    lo = Y_LO if sliced else 0
    out = ops.window3(xv, mode, stride, pad, out=ybuf[..., lo:lo + c])
    torch.cuda.synchronize()
    return out.permute(0, 3, 1, 2).cpu(), ybuf, (lo, lo + c)


@pytest.mark.parametrize("mode,stride,pad", [("max", 2, 0), ("avg", 1, 1), ("max", 1, 1), ("avg", 2, 0)])
@pytest.mark.parametrize("shape", [(2, 9, 11, 16), (1, 35, 35, 288)], ids=lambda s: "b%d_%dx%d_c%d" % s)
def test_window_contract(shape, mode, stride, pad):
    """Guard bands around both buffers, NaN in the channels of x outside the read slice and of y outside the written one,
    both payloads; the result is F.max_pool2d / F.avg_pool2d's to fp32 rounding (bit for bit for the max)."""
    from munit_amd import _lib
    lib = _lib.load()
    b, h, w, c = shape
    x_ld, y_ld = c + X_EXTRA, c + Y_EXTRA
    ho, wo = (h + 2 * pad - 3) // stride + 1, (w + 2 * pad - 3) // stride + 1
    a = CC.Arena(dict(x=b * h * w * x_ld * 4, y=b * ho * wo * y_ld * 4), DEV)
    xb, yb = a.view("x", torch.float32).view(b, h, w, x_ld), a.view("y", torch.float32).view(b, ho, wo, y_ld)
    vals = torch.randn(b, h, w, c, generator=torch.Generator().manual_seed(21))
    nchw = vals.permute(0, 3, 1, 2)
    want = F.max_pool2d(nchw, 3, stride, pad) if mode == "max" else F.avg_pool2d(nchw.double(), 3, stride, pad)
    outs = []
    for payload in (0, 1):
        CC.poison(xb, payload)
        xb[..., X_LO:X_LO + c] = vals.to(DEV)
        CC.poison(yb, payload)
        L = CC.Launches(a, ["x"], "window3 %s %s" % (shape, (mode, stride, pad)))
        xp, yp = c_void_p(a.ptr("x").value + 4 * X_LO), c_void_p(a.ptr("y").value + 4 * Y_LO)
        L.after(lib.munit_window3_fwd(xp, yp, b, h, w, c, x_ld, y_ld, _lib.WINDOW[mode], stride, pad, CC.stream()),
                "payload %d" % payload)
        assert _unwritten_intact(yb, (Y_LO, Y_LO + c), payload)
        out = yb[..., Y_LO:Y_LO + c].clone()
        assert CC.no_nan(out)
        outs.append(out)
    assert CC.bitwise_equal(outs[0], outs[1])
    got = outs[0].permute(0, 3, 1, 2).cpu()
    if mode == "max":
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    else:           # nine fp32 additions and one division: (9 + 1) 2^-24 of sum|x| / 9
        bound = 10 * FO.U32 * F.avg_pool2d(nchw.double().abs(), 3, stride, pad)
        assert bool(((got.double() - want).abs() <= bound).all())


@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "sliced"])
def test_max_window_keeps_negative_inputs(sliced):
    g = torch.Generator().manual_seed(5)
    x = -(torch.rand(2, 16, 9, 11, generator=g) + 0.25)             # all negative
    want = F.max_pool2d(x, kernel_size=3, stride=2)
    outs = []
    for payload in (0, 1):
        got, ybuf, bounds = _run_pool(x, "max", 2, 0, sliced, payload)
        assert tuple(got.shape) == (2, 16, 4, 5) and float(got.max()) < 0
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert _unwritten_intact(ybuf, bounds, payload)
        outs.append(got)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "sliced"])
def test_avg_window_divides_by_nine_at_the_corners(sliced):
    x = 9 * lattice((2, 16, 9, 11), 6, range(-5, 6)).float()
    want = F.avg_pool2d(x, kernel_size=3, stride=1, padding=1)
    got, ybuf, bounds = _run_pool(x, "avg", 1, 1, sliced)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    corner = x[:, :, :2, :2].sum((2, 3)) / 9                         # four taps, divisor 9 (not 4)
    assert torch.equal(got[:, :, 0, 0], corner) and bool((corner != x[:, :, :2, :2].sum((2, 3)) / 4).any())
    assert _unwritten_intact(ybuf, bounds, 0)


def test_window_refuses_six_channels():
    from munit_amd import ops
    x = torch.zeros(1, 9, 11, 6, device=DEV)
    with pytest.raises(RuntimeError, match=r"C % 4 == 0 is required, got 6"):
        ops.window3(x, "max", 2, 0)


# ---- input kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["planar", "channels_last"])
@pytest.mark.parametrize("shape", [(2, 3, 64, 48), (1, 3, 320, 320), (1, 3, 299, 299)], ids=lambda s: "%dx%d" % s[2:])
def test_inception_input_against_fp64(shape, layout):
    from munit_amd import ops
    g = torch.Generator().manual_seed(shape[2])
    x = (torch.rand(shape, generator=g) * 2 - 1)
    ref = IO.input_lines(x, torch.float64)
    ref32 = IO.input_lines(x, torch.float32)
    xd = x.to(DEV)
    if layout == "channels_last":
        xd = xd.contiguous(memory_format=torch.channels_last)
    got = ops.inception_input(xd).permute(0, 3, 1, 2).cpu()
    assert tuple(got.shape) == (shape[0], 3, 299, 299)
    scale = float(ref.abs().max())
    e32, ehip = float((ref32.double() - ref).abs().max()) / scale, float((got.double() - ref).abs().max()) / scale
    print("inception_input %s %s: e32 %.3e hip %.3e allowance %.3e" % (shape, layout, e32, ehip, FO.allowance(e32)))
    assert ehip <= FO.allowance(e32)
    if shape[2:] == (299, 299):          # no resize: the normalisation itself, bit for bit
        assert torch.equal(got.view(torch.int32), ref32.view(torch.int32))


def test_inception_input_refuses_other_layouts():
    from munit_amd import ops
    x = torch.zeros(2, 3, 16, 20, device=DEV)
    with pytest.raises(RuntimeError, match=r"neither planar- nor interleaved-dense"):
        ops.inception_input(x[:, :, :, ::2])
    with pytest.raises(RuntimeError, match=r"\(B >= 1, 3, H, W\)"):
        ops.inception_input(torch.zeros(2, 4, 16, 20, device=DEV))


def test_pixel_mean_is_the_references_final_mean():
    """munit_gap_fwd against torch.mean(x.view(B, C, -1), 2): divisor 64, rows independent of the batch."""
    from munit_amd import ops
    g = torch.Generator().manual_seed(9)
    x = torch.randn(3, 2048, 8, 8, generator=g)
    want = torch.mean(x.double().view(3, 2048, -1), 2)
    pix = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    got = ops.pixel_mean(pix).cpu()
    err = float((got.double() - want).abs().max() / want.abs().max())
    print("pixel_mean: error %.3e" % err)
    assert err <= FO.ALLOW_FLOOR
    assert torch.equal(ops.pixel_mean(pix[1:2].contiguous()).cpu().view(torch.int32), got[1:2].view(torch.int32))


# ---- whole trunk -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def state():
    return IO.random_state(0)


@pytest.fixture(scope="module")
def wrap(state):
    from munit_amd import inception_utils as IU
    return IU.WrapInception(state)


@pytest.fixture(scope="module")
def trunk_refs(state):
    """{case: (input fp32, fp64 features, fp32-oracle error)} -- computed once."""
    out = {}
    for name, x in IO.fixture_inputs().items():
        ref = IO.features(state, x, torch.float64)
        e32 = float((IO.features(state, x.float(), torch.float32).double() - ref).abs().max())
        out[name] = (x.float(), ref, e32)
    return out


def _trunk_allowance(e32, ref):
    return max(16 * e32, 16 * FO.U32 * float(ref.abs().max()))


@pytest.mark.parametrize("name", ["small", "full"])
def test_trunk_against_fp64(wrap, trunk_refs, name):
    x, ref, e32 = trunk_refs[name]
    assert float((ref != 0).double().mean()) >= 0.8
    got = wrap(x.to(DEV))
    assert tuple(got.shape) == (x.shape[0], 2048) and got.dtype == torch.float32 and got.is_cuda
    got = got.cpu()
    err, top = float((got.double() - ref).abs().max()), float(ref.abs().max())
    allow = _trunk_allowance(e32, ref)
    print("trunk %s: max|ref| %.4g e32 %.3e (%.3e rel) hip %.3e (%.3e rel) hip / e32 %.2f allowance %.3e"
          % (name, top, e32, e32 / top, err, err / top, err / e32, allow))
    assert err <= allow
    again = wrap(x.to(DEV)).cpu()
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))


def test_trunk_row_is_independent_of_its_batch(wrap, trunk_refs):
    x = trunk_refs["small"][0].to(DEV)
    both = wrap(x).cpu()
    alone = wrap(x[:1].contiguous()).cpu()
    assert torch.equal(both[:1].view(torch.int32), alone.view(torch.int32))


def test_trunk_batch_sizes_share_one_set_of_buffers(state):
    """The buffers are sized for the largest batch seen: a smaller batch runs in their heads, a larger one replaces them;
    the features do not depend on which."""
    from munit_amd import inception_utils as IU
    net = IU.WrapInception(state)
    x = IO.fixture_inputs()["small"].float().to(DEV)
    one = net(x[:1].contiguous()).cpu()
    flat = net.net._flat[torch.device(DEV)]
    assert flat[0] == 1
    two = net(x).cpu()                                            # grows: one set, sized for two
    assert list(net.net._flat) == [torch.device(DEV)] and net.net._flat[torch.device(DEV)][0] == 2
    ptrs = {s: t.data_ptr() for s, t in net.net._flat[torch.device(DEV)][1].items()}
    again = net(x[:1].contiguous()).cpu()                         # the short batch: in the heads of the same buffers
    assert {s: t.data_ptr() for s, t in net.net._flat[torch.device(DEV)][1].items()} == ptrs
    assert net.net.input_buffer("cuda", 1).data_ptr() == ptrs["in"]          # "cuda" and "cuda:0" are one key
    assert torch.equal(one.view(torch.int32), again.view(torch.int32)) and torch.equal(one.view(torch.int32), two[:1].view(torch.int32))


def test_trunk_accepts_channels_last_input(wrap, trunk_refs):
    x = trunk_refs["small"][0].to(DEV)
    a, b = wrap(x).cpu(), wrap(x.contiguous(memory_format=torch.channels_last)).cpu()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- through the public interface --------------------------------------------------------------------------------------
def test_load_inception_net_and_accumulate(tmp_path, monkeypatch, state):
    from oracle import munit_oracle as O
    from munit_amd import data, inception_utils as IU
    from munit_amd.trainer import MUNIT_Trainer
    from tests.test_gpu_fid import _lists, _write_images
    ckpt = str(tmp_path / "inception_v3_random.pth")
    torch.save(state, ckpt)
    monkeypatch.setenv(IU.CKPT_ENV, ckpt)
    net = IU.load_inception_net()
    assert callable(net)
    hp = O.default_hp(64, 1, 1)
    hp["gen"]["n_res"] = 1
    hp["guided"] = 1
    torch.manual_seed(11)
    trainer = MUNIT_Trainer(dict(hp))
    trainer.to(DEV)
    paths = _write_images(tmp_path, 8, 64, 64, 2)
    fa, fb = _lists(tmp_path, paths)
    loader = lambda: data.get_fid_data_loader(fa, fb, 4, False, new_size=64)
    pool = IU.accumulate_inception_activations(trainer, loader(), net)
    assert tuple(pool.shape) == (8, 2048) and pool.dtype == torch.float32 and pool.is_cuda
    fakes = torch.cat([trainer.sample_fid(x_a, x_b) for x_a, x_b in loader()]).cpu()
    ref = IO.features(state, fakes, torch.float64)
    e32 = float((IO.features(state, fakes, torch.float32).double() - ref).abs().max())
    err, allow = float((pool.cpu().double() - ref).abs().max()), _trunk_allowance(e32, ref)
    print("accumulate: max|ref| %.4g e32 %.3e hip %.3e allowance %.3e" % (float(ref.abs().max()), e32, err, allow))
    assert err <= allow
    npz = str(tmp_path / "moments.npz")
    np.savez(npz, mu=np.zeros(4), sigma=np.eye(4))          # only loaded here: the widths are compared when the metric runs
    assert callable(IU.prepare_inception_metrics(npz))
