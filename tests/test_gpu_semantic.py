"""GPU: the semantic-consistency loss (semantic_w > 0) -- the seg kernels, the frozen Resnet34_8s and the training step --
against the fp64 oracle of tests/semantic_oracle.py."""
import pytest
import torch
import torch.nn.functional as F

from munit_amd import ops
from oracle import munit_oracle as O
from tests import semantic_oracle as S
from tests.parity import nerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def cl(t):
    return t.float().to(DEV).contiguous(memory_format=torch.channels_last)


def l2err(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return ((a - ref).norm() / ref.norm().clamp_min(1e-300)).item()


@pytest.fixture(scope="module")
def model():
    return S.make_model(0).to(DEV)


@pytest.fixture(scope="module")
def sd(model):
    return S.state(model)


@pytest.mark.parametrize("n,c,h,w", [(2, 8, 4, 6), (16, 128, 32, 32), (64, 19, 8, 8)])
def test_space_to_batch_round_trip(n, c, h, w):
    x = torch.randn(n, c, h, w, dtype=torch.float64)
    y = ops.space_to_batch_raw(cl(x), 2)
    ref = x.view(n, c, h // 2, 2, w // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(n * 4, c, h // 2, w // 2)
    assert torch.equal(y.cpu().double(), ref.float().double())
    y_before = y.clone()
    back = ops.space_to_batch_raw(y, 2, inverse=True)
    assert torch.equal(y, y_before)
    assert torch.equal(back.cpu().double(), x.float().double())


@pytest.mark.parametrize("b,c,h,w", [(2, 4, 7, 9), (2, 64, 16, 16), (8, 64, 128, 128)])
def test_maxpool_first_max_rule(b, c, h, w):
    g = torch.Generator().manual_seed(b * h)
    x = torch.randint(0, 3, (b, c, h, w), generator=g).double()     # many ties
    xr = x.clone().requires_grad_(True)
    yr, idx = F.max_pool2d(xr, 3, 2, 1, return_indices=True)
    dy = torch.randn(yr.shape, generator=g, dtype=torch.float64)
    yr.backward(dy)
    xd = cl(x).requires_grad_(True)
    with ops.kinks(seg=True) as k:
        y = ops.maxpool3s2(xd)
    win = k.seg[0].cpu().long()                       # (b, ho, wo, c): window position kh*3 + kw
    assert torch.equal(y.cpu().double(), yr.detach())
    # the rule, restated: first maximal element of the window in kh-major order (torch's CPU kernel agrees)
    ho, wo = y.shape[2:]
    kh, kw = win // 3, win % 3
    row = 2 * torch.arange(ho).view(1, ho, 1, 1) - 1 + kh
    col = 2 * torch.arange(wo).view(1, 1, wo, 1) - 1 + kw
    assert torch.equal((row * w + col).permute(0, 3, 1, 2), idx)
    y.backward(cl(dy))
    assert nerr(xd.grad.cpu(), xr.grad) < 1e-6


@pytest.mark.parametrize("cin,cout,k,pad,b,h", [(3, 64, 7, 3, 2, 16), (64, 128, 3, 1, 2, 16), (64, 128, 1, 0, 2, 16),
                                               (3, 64, 7, 3, 2, 256), (64, 128, 3, 1, 2, 64)])
def test_odd_kernel_stride2_dgrad(cin, cout, k, pad, b, h):
    from munit_amd.segmentation import _even
    g = torch.Generator().manual_seed(k * h)
    w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) / (cin * k * k) ** 0.5
    x = torch.randn(b, cin, h, h, generator=g, dtype=torch.float64).requires_grad_(True)
    y = F.conv2d(x, w, None, 2, pad)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    add = torch.randn(x.shape, generator=g, dtype=torch.float64)       # the block's skip gradient (`add` operand)
    y.backward(dy)
    xd = cl(x.detach()).requires_grad_(True)
    link = ops.ResidualLink()
    link.park(cl(add))
    yd = ops.frozen_conv(xd, cl(w), None, cl(_even(w)), 2, pad, link_in=link)
    assert nerr(yd.cpu(), y.detach()) < 2e-5
    yd.backward(cl(dy))
    assert link.grad is None
    assert nerr(xd.grad.cpu(), x.grad + add) < 2e-5


_WINO = "conv_wino_kernel<1, 0>"
_WINO_S2 = "conv_wino_kernel<1, 2>"
_FWD = "conv_igemm_kernel<fwd>"
_TAPS3 = "conv_igemm_kernel<.., 5> (3 input channels as 4-channel taps)"
_DIRECT = "conv_igemm_kernel<dgrad direct>"
_PHASES = "conv_igemm_kernel<.., 1, .> phases + fold_kernel"
_PATCH = "conv_igemm_kernel<.., 2, 3> (LDS-patch fold)"
# Op cases of the frozen Resnet34_8s, (cin, cout, k, stride, pad, act, B, H, W) -> the (forward, backward-data) kernels each
# was added for (tests/test_cpu_dispatch.py pins them and requires every form the network reaches, per channel / filter /
# stride class, to be run by one of these).  Zero padding, a bias and a random `add` operand always; backward-data of the
# stride-2 layers through the zero-extended filter.  Layer4 at an odd extent (crops 96, 160, 224, ...) leaves Winograd in
# BOTH passes: forward on the implicit GEMM, backward-data on the LDS-patch fold; at 512 channels Winograd runs on even
# extents only, so the Winograd cases are 2x2 (batch 256) and 4x4.
SEG_CONV_CASES_TARGETS = {
    (3, 64, 7, 2, 3, "relu", 2, 64, 64): (_TAPS3, _PHASES),                 # conv1, 8x8 backward-data filter
    (3, 64, 7, 2, 3, "relu", 2, 96, 96): (_TAPS3, _PHASES),
    (64, 64, 3, 1, 1, "relu", 2, 24, 24): (_WINO, _WINO),                   # layer1
    (64, 128, 3, 2, 1, "relu", 2, 24, 24): (_FWD, _PHASES),                 # layer2.0.conv1, 4x4 backward-data filter
    (64, 128, 3, 2, 1, "relu", 64, 24, 24): (_FWD, _WINO_S2),
    (64, 128, 1, 2, 0, "none", 2, 24, 24): (_FWD, _DIRECT),                 # layer2.0.downsample, 2x2 backward-data filter
    (128, 128, 3, 1, 1, "none", 2, 12, 12): (_WINO, _WINO),                 # layer2
    (128, 256, 3, 1, 1, "relu", 8, 6, 6): (_WINO, _WINO),                   # layer3.0.conv1 on 2x2 phases
    (128, 256, 1, 1, 0, "none", 8, 6, 6): (_FWD, _DIRECT),                  # layer3.0.downsample
    (256, 256, 3, 1, 1, "none", 8, 6, 6): (_WINO, _WINO),                   # layer3
    (256, 256, 3, 1, 1, "relu", 16, 4, 4): (_WINO, _WINO),
    (256, 512, 3, 1, 1, "relu", 64, 2, 2): (_WINO, _WINO),                  # layer4.0.conv1, crop 64
    (256, 512, 3, 1, 1, "relu", 32, 3, 3): (_FWD, _PATCH),                  # layer4 at crop 96, 2 images
    (512, 512, 3, 1, 1, "relu", 32, 3, 3): (_FWD, _PATCH),
    (512, 512, 3, 1, 1, "none", 32, 3, 3): (_FWD, _PATCH),
    (256, 512, 3, 1, 1, "relu", 32, 5, 5): (_FWD, _PATCH),                  # crop 160
    (512, 512, 3, 1, 1, "relu", 32, 5, 5): (_FWD, _PATCH),
    (512, 512, 3, 1, 1, "none", 32, 7, 7): (_FWD, _PATCH),                  # crop 224
    (512, 512, 3, 1, 1, "relu", 256, 2, 2): (_WINO, _WINO),                 # crop 64, 16 images
    (512, 512, 3, 1, 1, "none", 128, 4, 4): (_WINO, _WINO),                 # crop 128, 8 images
    (256, 512, 1, 1, 0, "none", 32, 3, 3): (_FWD, _DIRECT),                 # layer4.0.downsample
    (256, 512, 1, 1, 0, "none", 256, 2, 2): (_FWD, _DIRECT),
    (512, 19, 1, 1, 0, "none", 32, 3, 3): (_FWD, _DIRECT),                  # fc: N = 19 forward, a reduction over 19 back
    (512, 19, 1, 1, 0, "none", 256, 2, 2): (_FWD, _DIRECT),
    (512, 19, 1, 1, 0, "none", 32, 16, 16): (_FWD, _DIRECT),
}
SEG_CONV_CASES = list(SEG_CONV_CASES_TARGETS)
SEG_CONV_TOL = 2e-5


@pytest.mark.parametrize("case", SEG_CONV_CASES, ids=lambda c: "c%d-%d_k%ds%d_%s_b%d_%dx%d" % (c[:4] + c[5:]))
def test_seg_conv_fwd_dgrad(case):
    """ops.frozen_conv (bias, optional ReLU, zero-extended backward-data filter, `add` from a ResidualLink) against
    F.conv2d in fp64.  Bound: 2e-5 normalised max error, or 3 x the error of torch's fp32 CPU evaluation of the same
    case where that is larger (these layers sum up to 4608 products).  The ReLU branch is the device's own (SEG_SINK),
    audited against the fp64 sign at rounding-noise margins."""
    from munit_amd.segmentation import _even
    cin, cout, k, stride, pad, act, b, h, w = case
    g = torch.Generator().manual_seed(cin + cout + k + b + h)
    wt = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) * (2.0 / (cin * k * k)) ** 0.5
    bias = 0.1 * torch.randn(cout, generator=g, dtype=torch.float64)
    x = torch.randn(b, cin, h, w, generator=g, dtype=torch.float64)
    add = torch.randn(b, cin, h, w, generator=g, dtype=torch.float64)

    xd = cl(x).requires_grad_(True)
    link = ops.ResidualLink()
    link.park(cl(add))
    with ops.kinks(seg=True) as k:
        yd = ops.frozen_conv(xd, cl(wt), bias.float().to(DEV), cl(_even(wt)) if stride == 2 else cl(wt), stride, pad, act,
                             link_in=link)
    sink = k.seg
    assert len(sink) == (1 if act == "relu" else 0)

    def ref(dtype):
        xr = x.detach().clone().to(dtype).requires_grad_(True)
        pre = F.conv2d(xr, wt.to(dtype), bias.to(dtype), stride, pad)
        return xr, pre

    xr, pre = ref(torch.float64)
    dy = torch.randn(pre.shape, generator=g, dtype=torch.float64)
    x32, pre32 = ref(torch.float32)
    if act == "relu":
        mask = sink[0].cpu()
        flips = (mask != (pre.detach() > 0))
        assert not bool((flips & (pre.detach().abs() > 1e-5 * pre.detach().abs().max())).any())
        yr, y32 = pre * mask.double(), pre32 * mask.float()
    else:
        yr, y32 = pre, pre32
    yr.backward(dy)
    y32.backward(dy.float())
    gx, gx32 = xr.grad + add, x32.grad + add.float()
    yard_f, yard_b = nerr(y32, yr), nerr(gx32, gx)
    yd.backward(cl(dy))
    assert link.grad is None
    ef, eb = nerr(yd.cpu(), yr), nerr(xd.grad.cpu(), gx)
    print("seg conv %s: fwd %.2e (fp32 CPU %.2e), dgrad %.2e (fp32 CPU %.2e)" % (case, ef, yard_f, eb, yard_b))
    assert ef <= max(SEG_CONV_TOL, 3 * yard_f), (ef, yard_f)
    assert eb <= max(SEG_CONV_TOL, 3 * yard_b), (eb, yard_b)


def _head_case(b, h, scale, kind, seed):
    g = torch.Generator().manual_seed(seed)
    z = 3 * torch.randn(b, 19, h, h, generator=g, dtype=torch.float64)
    H = h * scale
    labels = torch.randint(0, 19, (b, H, H), generator=g)
    mask = None
    if kind == "masked":
        mask = (torch.rand(b, 1, H, H, generator=g) < 0.4).double()
    elif kind == "all_masked":
        mask = torch.ones(b, 1, H, H, dtype=torch.float64)
    return z, labels, mask


@pytest.mark.parametrize("b,h", [(2, 4), (16, 32)])
@pytest.mark.parametrize("kind", ["plain", "masked", "all_masked"])
def test_head_loss_and_dlogits(b, h, kind):
    z, labels, mask = _head_case(b, h, 8, kind, b * h)
    zr = z.clone().requires_grad_(True)
    up = F.interpolate(zr, scale_factor=8, mode="bilinear", align_corners=False)
    ref = S.ce_loss(up, labels, mask) * 2        # norm = half the pixels: the sum of two means
    ref.backward()
    zd = cl(z).requires_grad_(True)
    md = None if mask is None else mask.float().to(DEV).contiguous()
    loss = ops.seg_cross_entropy(zd, labels.int().to(DEV).contiguous(), md, 8, norm=labels.numel() / 2)
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    if kind == "all_masked":
        assert abs(loss.item() - 2 * S.MASKED_PIXEL_LOSS) < 1e-5
    loss.backward()
    if kind == "all_masked":
        assert torch.count_nonzero(zd.grad) == 0
    else:
        assert nerr(zd.grad.cpu(), zr.grad) < 5e-5
    # deterministic: a second backward is bitwise the same
    g1 = zd.grad.clone()
    zd.grad = None
    ops.seg_cross_entropy(zd, labels.int().to(DEV).contiguous(), md, 8, norm=labels.numel() / 2).backward()
    assert torch.equal(g1, zd.grad)


@pytest.mark.parametrize("b,h", [(2, 4), (16, 32)])
def test_labels_first_max(b, h):
    z, _, _ = _head_case(b, h, 8, "plain", 7 + h)
    z[:, 5] = z[:, 3]                                   # exact ties between classes 3 and 5: 3 wins
    zd = cl(z)
    lab = ops.seg_labels(zd).cpu().long()
    up = F.interpolate(zd.cpu().double(), scale_factor=8, mode="bilinear", align_corners=False)
    ref = up.argmax(1)
    top = up.topk(2, 1).values
    tight = (top[:, 0] - top[:, 1]) < 1e-5
    assert torch.equal(lab[~tight], ref[~tight])
    assert (lab != 5).all()


@pytest.mark.parametrize("b,size", [(2, 64), (2, 256), (2, 96), (2, 160), (8, 64)])
def test_network_logits_and_input_grad(model, sd, monkeypatch, b, size):
    """Crops 96 and 160 put layer4 on 3x3 / 5x5 phase images (implicit-GEMM forward, LDS-patch fold backward-data);
    8 images at crop 64 give layer4 a batch of 128.  The convolutions the device path really plans are recorded and must
    be tests/seg_layers.py's list (what tests/test_cpu_dispatch.py reasons about), with no backward-weight call."""
    from tests import seg_layers as SL
    calls = {"fwd": [], "dgrad": [], "wgrad": 0}
    fwd_raw, dgrad_raw = ops.conv2d_fwd_raw, ops.conv2d_dgrad_raw

    def rec_fwd(x, weight, bias, stride, pad, pad_type, upsample, act, *a, **kw):
        calls["fwd"].append((tuple(x.shape), tuple(weight.shape), bias is not None, stride, pad, pad_type, bool(upsample), act))
        return fwd_raw(x, weight, bias, stride, pad, pad_type, upsample, act, *a, **kw)

    def rec_dgrad(dy, weight, x_shape, stride, pad, pad_type, upsample, add=None, **kw):
        calls["dgrad"].append((tuple(x_shape), tuple(weight.shape), stride, pad, pad_type, bool(upsample), add is not None))
        return dgrad_raw(dy, weight, x_shape, stride, pad, pad_type, upsample, add=add, **kw)

    def rec_wgrad(*a, **kw):
        calls["wgrad"] += 1
        raise AssertionError("the frozen network asked for a weight gradient")

    monkeypatch.setattr(ops, "conv2d_fwd_raw", rec_fwd)
    monkeypatch.setattr(ops, "conv2d_dgrad_raw", rec_dgrad)
    monkeypatch.setattr(ops, "conv2d_wgrad_raw", rec_wgrad)
    x = S.rand_images(b, size, size)
    xd = cl(x).requires_grad_(True)
    with ops.kinks(seg=True) as k:
        z = model(xd)
    pins = S.seg_pins(k.seg)
    # the oracle takes the device's branch at every ReLU and max-pool kink; the audit allows a disagreement with the
    # oracle's own choice only at rounding-noise margins
    xr = x.clone().requires_grad_(True)
    kinks = []
    zr = S.logits(sd, xr, up=False, kinks=kinks, pins=pins)
    assert S.audit(kinks, pins) == 0
    dz = torch.randn(zr.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    zr.backward(dz)
    assert z.shape == zr.shape
    print("network b=%d crop %d: logits %.2e max %.2e L2" % (b, size, nerr(z.cpu(), zr.detach()), l2err(z, zr.detach())))
    assert nerr(z.cpu(), zr.detach()) < 5e-5 and l2err(z, zr.detach()) < 5e-5
    z.backward(cl(dz))
    print("network b=%d crop %d: input grad %.2e max %.2e L2" % (b, size, nerr(xd.grad.cpu(), xr.grad), l2err(xd.grad, xr.grad)))
    assert nerr(xd.grad.cpu(), xr.grad) < 5e-5 and l2err(xd.grad, xr.grad) < 5e-5
    layers = SL.seg_layers(size, b)
    assert calls["fwd"] == [SL.fwd_call(l) for l in layers]
    assert sorted(calls["dgrad"]) == sorted(SL.dgrad_call(l) for l in layers) and len(calls["dgrad"]) == 37
    assert calls["wgrad"] == 0


# ------------------------------------------------------------------------------------------------------------------
# kernel edges: every seg.hip kernel is a grid-stride loop capped at 16384 blocks of 256 threads
# ------------------------------------------------------------------------------------------------------------------
GRID_CAP = 16384 * 256


def test_seg_input_three_batches_and_grid_wrap():
    """Three inputs of different batch sizes packed into one batch by offset, the first needing no gradient.  Each input
    is one launch of its own, forward and backward; the second holds 4.7 M values, past the grid cap.  Values and
    gradients against the fp64 formula; the gradient tuple has None exactly there."""
    g = torch.Generator().manual_seed(1)
    xs = [torch.rand(n, 3, 512, 512, generator=g, dtype=torch.float64) * 2 - 1 for n in (1, 6, 3)]
    assert xs[1].numel() > GRID_CAP > xs[2].numel()
    xd = [cl(x).requires_grad_(i > 0) for i, x in enumerate(xs)]
    y = ops.seg_input(*xd)
    ref = S.transform(torch.cat(xs))
    assert tuple(y.shape) == tuple(ref.shape)
    assert nerr(y.cpu(), ref) < 1e-6
    dy = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    import types
    ctx = types.SimpleNamespace(sizes=[x.shape for x in xs], needs_input_grad=(False, True, True))
    grads = ops._SegInput.backward(ctx, cl(dy))
    assert isinstance(grads, tuple) and len(grads) == 3
    assert grads[0] is None and grads[1] is not None and grads[2] is not None
    want = dy / (2 * torch.tensor(S.STD, dtype=torch.float64).view(1, 3, 1, 1))
    assert nerr(grads[1].cpu(), want[1:7]) < 1e-6 and nerr(grads[2].cpu(), want[7:]) < 1e-6
    y.backward(cl(dy))
    assert xd[0].grad is None and torch.equal(xd[1].grad, grads[1]) and torch.equal(xd[2].grad, grads[2])


def _s2b_ref(x, f):
    n, c, h, w = x.shape
    return x.view(n, c, h // f, f, w // f, f).permute(0, 3, 5, 1, 2, 4).reshape(n * f * f, c, h // f, w // f)


@pytest.mark.parametrize("n,c,h,w,f", [(2, 3, 8, 12, 1), (3, 19, 4, 12, 2), (2, 64, 8, 4, 4), (1, 3, 12, 20, 4),
                                       (2, 19, 6, 10, 2), (2, 64, 192, 192, 2), (1, 19, 512, 512, 4)])
def test_space_to_batch_factors_and_grid_wrap(n, c, h, w, f):
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(h + f), dtype=torch.float64).float()
    xd = cl(x)
    y = ops.space_to_batch_raw(xd, f)
    assert torch.equal(y.cpu(), _s2b_ref(x, f))
    back = ops.space_to_batch_raw(y, f, inverse=True)
    assert torch.equal(back.cpu(), x) and torch.equal(xd.cpu(), x)


def test_space_to_batch_twice_is_factor_four_in_phase_order():
    """f = 2 applied twice equals f = 4 with the phases reordered (py = 2 * py2 + py1, px = 2 * px2 + px1, the first
    split's phase being the slower batch index): what Resnet34_8s.forward relies on when it undoes two levels."""
    n, c, h, w = 3, 19, 8, 12
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(2), dtype=torch.float64).float()
    twice = ops.space_to_batch_raw(ops.space_to_batch_raw(cl(x), 2), 2).cpu()
    four = ops.space_to_batch_raw(cl(x), 4).cpu()
    # four: batch (n, py2, py1, px2, px1); twice: batch (n, py1, px1, py2, px2)
    want = four.view(n, 2, 2, 2, 2, c, h // 4, w // 4).permute(0, 2, 4, 1, 3, 5, 6, 7).reshape(n * 16, c, h // 4, w // 4)
    assert torch.equal(twice, want)
    undone = ops.space_to_batch_raw(ops.space_to_batch_raw(cl(twice), 2, inverse=True), 2, inverse=True)
    assert torch.equal(undone.cpu(), x)


def _maxpool_check(x, seed):
    """forward bit for bit F.max_pool2d in fp64, indices by the first-max rule, backward at 1e-6"""
    b, c, h, w = x.shape
    xr = x.clone().requires_grad_(True)
    yr, idx = F.max_pool2d(xr, 3, 2, 1, return_indices=True)
    dy = torch.randn(yr.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    yr.backward(dy)
    xd = cl(x).requires_grad_(True)
    with ops.kinks(seg=True) as k:
        y = ops.maxpool3s2(xd)
    win = k.seg[0].cpu().long()
    assert tuple(y.shape) == tuple(yr.shape)
    assert torch.equal(y.cpu().double(), yr.detach()), (b, c, h, w)
    ho, wo = y.shape[2:]
    assert int(win.min()) >= 0 and int(win.max()) <= 8
    kh, kw = win // 3, win % 3
    row = 2 * torch.arange(ho).view(1, ho, 1, 1) - 1 + kh
    col = 2 * torch.arange(wo).view(1, 1, wo, 1) - 1 + kw
    assert bool(((row >= 0) & (row < h) & (col >= 0) & (col < w)).all()), "a winner outside the image"
    # the rule restated: the first maximal element of the window in kh-major order, padding never a candidate
    cols = F.unfold(F.pad(x, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(b, c, 9, ho, wo)
    first = (cols == cols.max(2, keepdim=True).values).double().argmax(2)
    assert torch.equal(win.permute(0, 3, 1, 2), first)
    assert torch.equal((row * w + col).permute(0, 3, 1, 2), idx)
    y.backward(cl(dy))
    assert nerr(xd.grad.cpu(), xr.grad) < 1e-6


@pytest.mark.parametrize("kind", ["negative", "mixed_ties", "constant"])
def test_maxpool_borders_and_signs(kind):
    """Every (H, W) in 1..6 x 1..6 (windows that hold one real element, odd extents) with inputs that are all negative
    (the zero padding must never win), mixed sign with many ties, and one constant (negative) plane."""
    for h in range(1, 7):
        for w in range(1, 7):
            g = torch.Generator().manual_seed(10 * h + w)
            if kind == "negative":
                x = -0.5 - torch.rand(2, 5, h, w, generator=g, dtype=torch.float64)
            elif kind == "mixed_ties":
                x = torch.randint(-2, 2, (2, 5, h, w), generator=g).double()
            else:
                x = torch.full((2, 5, h, w), -3.0, dtype=torch.float64)
            _maxpool_check(x.float().double(), h * w)


def test_maxpool_forward_past_the_grid_cap():
    x = (-0.5 - torch.rand(2, 64, 384, 384, generator=torch.Generator().manual_seed(4), dtype=torch.float64)).float().double()
    assert 2 * 64 * 192 * 192 > GRID_CAP and float(x.max()) < 0
    _maxpool_check(x, 5)


def test_add_relu_zero_sums_and_grid_wrap():
    """relu(a + r) against fp64 (an fp32 sum of two fp32 values is the rounded exact sum), with sums that are exactly
    zero and negative zero; the mask handed to SEG_SINK is y > 0; 17.3 M elements (n / 4 past the grid cap)."""
    g = torch.Generator().manual_seed(6)
    shape = (2, 64, 368, 368)
    a = torch.randn(shape, generator=g).double()
    r = torch.randn(shape, generator=g).double()
    assert a.numel() // 4 > GRID_CAP
    af, rf = a.view(-1), r.view(-1)
    rf[::5] = -af[::5]                      # exact zeros
    af[1::7] = -0.0
    rf[1::7] = -0.0                         # negative zero
    rf[-3:] = 1.0 - af[-3:]                 # the last vector of four: live values
    ad, rd = cl(a).requires_grad_(True), cl(r).requires_grad_(True)
    with ops.kinks(seg=True) as k:
        y = ops.add_relu(ad, rd)
    mask = k.seg[0]
    want = (a.float().double() + r.float().double()).clamp_min(0).float()
    assert torch.equal(y.cpu(), want)
    assert torch.equal(mask, y > 0) and torch.equal(mask.cpu(), want > 0)
    assert not bool(torch.isnan(y).any())
    dy = torch.randn(shape, generator=g)
    y.backward(cl(dy))
    wg = torch.where(want > 0, dy, torch.zeros_like(dy))
    assert torch.equal(ad.grad.cpu(), wg) and torch.equal(rd.grad.cpu(), wg)


def _mask_of(kind, b, H, W, g):
    if kind == "none":
        return None
    if kind == "random":
        return (torch.rand(b, 1, H, W, generator=g) < 0.4).double()
    m = torch.zeros(b, 1, H, W, dtype=torch.float64)
    if kind == "rows":
        m[:, :, ::3] = 1.0                  # whole rows
    else:
        m[b - 1] = 1.0                      # one whole image
    return m


# (B, h, w, S, logit scale, mask, copies): copies > 1 tiles the B distinct images (the fp64 reference runs on B only)
HEAD_CASES = [
    (2, 3, 5, 8, 3.0, "none", 1), (2, 5, 3, 8, 3.0, "random", 1),          # h != w, both orders
    (2, 1, 6, 8, 3.0, "none", 1), (2, 6, 1, 8, 3.0, "random", 1), (1, 1, 1, 8, 3.0, "none", 1),
    (1, 4, 7, 8, 3.0, "rows", 1),
    (2, 4, 6, 1, 3.0, "none", 1), (2, 6, 4, 2, 3.0, "random", 1), (2, 5, 7, 4, 3.0, "image", 1),
    (2, 5, 4, 3, 3.0, "none", 1), (2, 4, 5, 3, 3.0, "random", 1),          # S not a power of two
    (2, 4, 6, 8, 20.0, "none", 1), (2, 6, 4, 8, 20.0, "random", 1), (3, 5, 5, 8, 20.0, "image", 1),   # logits ~ +-60
    (2, 96, 96, 8, 3.0, "random", 4),                                       # 4.7 M pixels: loss, gradient, labels wrap
    (2, 192, 192, 2, 3.0, "none", 4),                                       # 5.6 M dlogits: the adjoint wraps
]


@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "b%d_%dx%d_s%d_z%g_%s_x%d" % c)
def test_head_shapes_scales_and_masks(case):
    """Loss at 1e-5 relative, dlogits at 5e-5 normalised, labels equal to the fp64 argmax outside a 1e-5 tie margin (at
    most 1 % of the pixels inside it), against F.interpolate + cross-entropy in fp64."""
    b, h, w, sc, zs, kind, copies = case
    g = torch.Generator().manual_seed(1000 * h + 10 * w + sc)
    H, W = h * sc, w * sc
    z = zs * torch.randn(b, 19, h, w, generator=g, dtype=torch.float64)
    z = z.float().double()
    labels = torch.randint(0, 19, (b, H, W), generator=g)
    mask = _mask_of(kind, b, H, W, g)
    zr = z.clone().requires_grad_(True)
    up = F.interpolate(zr, size=(H, W), mode="bilinear", align_corners=False)
    ref = S.ce_loss(up, labels, mask)
    ref.backward()

    rep = lambda t: None if t is None else torch.cat([t] * copies)
    zd = cl(rep(z)).requires_grad_(True)
    ld = rep(labels).int().to(DEV).contiguous()
    md = None if mask is None else rep(mask).float().to(DEV).contiguous()
    if copies > 1:
        assert max(ld.numel(), zd.numel()) > GRID_CAP
    loss = ops.seg_cross_entropy(zd, ld, md, sc)
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item()), (loss.item(), ref.item())
    loss.backward()
    gd = zd.grad.cpu()
    for i in range(1, copies):
        assert torch.equal(gd[i * b:(i + 1) * b], gd[:b]), "copies of the same image differ"
    want = zr.grad / copies
    if float(want.abs().max()) == 0.0:
        assert torch.count_nonzero(gd) == 0
    else:
        assert nerr(gd[:b], want) < 5e-5, nerr(gd[:b], want)
    lab = ops.seg_labels(zd.detach(), sc).cpu().long()
    upd = up.detach()
    top = upd.topk(2, 1).values
    tight = (top[:, 0] - top[:, 1]) < 1e-5
    assert float(tight.double().mean()) <= 0.01
    for i in range(copies):
        li = lab[i * b:(i + 1) * b]
        assert torch.equal(li[~tight], upd.argmax(1)[~tight])
    assert int(lab.min()) >= 0 and int(lab.max()) <= 18


def _ckpt(tmp_path, model):
    p = tmp_path / "seg.pth"
    torch.save({k: v.cpu() for k, v in model.state_dict().items()}, str(p))
    return str(p)


def _trainer(hp, seed):
    from munit_amd.trainer import MUNIT_Trainer
    torch.manual_seed(seed)
    return MUNIT_Trainer(hp).to(DEV)


def _hp(size, batch, ckpt, full_adaptation=0):
    hp = O.default_hp(size, batch, 1)
    hp["semantic_w"] = 3
    hp["semantic_ckpt_path"] = ckpt
    hp["adaptation"]["full_adaptation"] = full_adaptation
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


def _semantic_parity(tmp_path, monkeypatch, size, batch, full, gen_state=1, **kw):
    from tests.parity import run_step_parity
    seg = S.make_model(0)
    sink = []
    cls = S.oracle_trainer_class(seg, lambda: sink)
    monkeypatch.setattr(O, "OracleTrainer", cls)
    with ops.kinks(seg=sink):
        rep = run_step_parity(size=size, batch=batch, gen_state=gen_state, iters=1, device=DEV,
                              hp_overrides={"semantic_w": 3, "semantic_ckpt_path": _ckpt(tmp_path, seg),
                                            "adaptation": {"full_adaptation": full}}, **kw)
    assert cls.audit_bad == 0
    assert "loss_sem_seg" in rep and rep["loss_sem_seg"] > 0
    return rep


@pytest.mark.parametrize("full", [0, 1])
def test_step_parity_with_semantic_loss(tmp_path, monkeypatch, full):
    """dis_update + gen_update with semantic_w: 3 against the fp64 OracleTrainer that adds the term through its own
    x_ab / x_ba (tests/parity.run_step_parity's bounds: every loss <= 1e-5 relative, every generator gradient <= 5e-5
    normalised max and relative L2 with the kinks pinned, median <= 1e-5, Adam moments and the weight step), at 64^2 B=2.
    The seg network's kinks and labels are pinned and audited as well."""
    rep = _semantic_parity(tmp_path, monkeypatch, 64, 2, full)
    assert rep["grad_nerr"] <= 5e-5 and rep["grad_l2"] <= 5e-5, rep


def test_step_parity_with_semantic_loss_256(tmp_path, monkeypatch):
    """The same step at 256^2 B=1.  Stated exception: here the fp32 evaluation of the reference
    itself does not meet 5e-5 / median 1e-5.  Every tensor on the x_ba path sits at ~2.8e-5 relative L2 for the oracle
    run in fp32 (torch CPU, direct convolutions, same pinned kinks and labels), median 1.05e-5.  So each generator
    gradient is held to max(5e-5, 3 x that yardstick) and the median to 3 x the yardstick's median.  Measured: HIP worst
    5.9e-5 max / 4.7e-5 L2, median 2.7e-5.  Every loss keeps 1e-5, and the kink audits, Adam moments and weight step keep
    run_step_parity's bounds."""
    from tests.parity import KINK_FRAC, KINK_NOISE
    rep = _semantic_parity(tmp_path, monkeypatch, 256, 1, 0, check=False, ref32=True)
    assert rep["loss_rel"] <= 1e-5, rep["loss_rel"]
    assert rep["kink_worst_rel"] <= KINK_NOISE and rep["kink_disagree_frac"] <= KINK_FRAC
    rows = rep["ref32"][0]
    assert len(rows) > 50
    for name, hip_max, hip_l2, r32_max, r32_l2 in rows:
        assert hip_max <= max(5e-5, 3 * r32_max) and hip_l2 <= max(5e-5, 3 * r32_l2), (name, hip_max, hip_l2, r32_max, r32_l2)
    med = lambda k: sorted(r[k] for r in rows)[len(rows) // 2]
    assert med(2) <= max(1e-5, 3 * med(4)), (med(2), med(4))
    # Adam moments are linear / quadratic in the gradients: twice the per-tensor bound, as run_step_parity holds them
    assert rep["moment_l2"] <= 2 * max(5e-5, 3 * max(r[4] for r in rows)), rep["moment_l2"]
    assert rep["weight_abs"] <= 4.0 * 1e-4 and rep["weight_l2"] <= 2e-4, rep


def test_step_parity_with_semantic_loss_96(tmp_path, monkeypatch):
    """The same step at 96^2 B=2: layer4 of the frozen network runs on 3x3 phase images (batch 64), its backward-data on the
    LDS-patch fold form.  run_step_parity's bounds unchanged."""
    rep = _semantic_parity(tmp_path, monkeypatch, 96, 2, 0)
    print("semantic step 96: grad %.2e max %.2e L2, median %.2e" % (rep["grad_nerr"], rep["grad_l2"], rep["grad_l2_median"]))
    assert rep["grad_nerr"] <= 5e-5 and rep["grad_l2"] <= 5e-5, rep


@pytest.mark.parametrize("mode", ["gen_state0", "guided0", "extraadam"])
def test_step_parity_with_semantic_loss_in_other_modes(tmp_path, monkeypatch, mode):
    """semantic_w: 3 with two generators (gen_state 0: the term's backward feeds both decoders of separate networks),
    with sampled styles (guided 0) and with the ExtraAdam optimizer, at 64^2; run_step_parity's bounds."""
    kw = {"gen_state0": dict(gen_state=0), "guided0": dict(guided=0), "extraadam": dict(optimizer="extraadam")}[mode]
    rep = _semantic_parity(tmp_path, monkeypatch, 64, 2, 0, **kw)
    print("semantic step %s: grad %.2e max %.2e L2" % (mode, rep["grad_nerr"], rep["grad_l2"]))
    assert rep["grad_nerr"] <= 5e-5 and rep["grad_l2"] <= 5e-5, rep


def test_multi_stream_step_with_semantic_loss_is_bitwise_the_single_stream_step(tmp_path, model):
    """gen_update joins the two branch streams before the semantic term and its backward feeds both decoders: the
    three-stream schedule must not change a bit of the step (tests/test_gpu_step.py's mechanism, semantic_w: 3)."""
    from munit_amd import trainer as T
    ckpt = _ckpt(tmp_path, model)
    hp = _hp(64, 2, ckpt)
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
            return (tr.loss_sem_seg.item(), tr.loss_gen_total.item(), tr.gen_opt.flat_g.clone(), tr.gen_opt.flat_p.clone(),
                    tr.dis_opt.flat_p.clone())
        finally:
            ops.SIDE_STREAM_WGRAD, T.BRANCH_STREAMS = saved

    ref = run(False)
    assert ref[0] > 0
    for _ in range(3):
        got = run(True)
        assert got[:2] == ref[:2]
        assert all(torch.equal(a, b) for a, b in zip(ref[2:], got[2:]))


def test_reuse_dis_forward_with_semantic_loss_matches_the_plain_step(tmp_path, model):
    """reuse_dis_forward: 1 with semantic_w > 0: the term takes x_ab / x_ba kept from dis_update.  Bounds of
    test_reuse_dis_forward_matches_the_plain_step: the first iteration's losses bit for bit (loss_sem_seg included), the
    flat generator gradient to 1e-5 relative L2, loss_gen_total (which carries 3 x the term) and loss_dis_total after
    further steps to 2e-3.  The term on its own is not held after several Adam steps on re-ordered sums: its labels are an
    argmax, so it is not continuous in the weights (measured after three steps: 4.100 against 4.085)."""
    from tests.parity import l2err as flat_l2
    ckpt = _ckpt(tmp_path, model)
    b0, b1 = _inputs(2, 64, 5), _inputs(2, 64, 6)

    def run(reuse):
        hp = _hp(64, 2, ckpt)
        hp["reuse_dis_forward"] = reuse
        tr = _trainer(hp, 0)
        first = None
        for it in range(3):
            b = b0 if it != 1 else b1
            tr.update_learning_rate()
            tr.dis_update(b[0], b[1], hp)
            assert (tr._fwd_cache is not None) == bool(reuse)
            tr.gen_update(b[0], b[1], hp, b[2], b[3])
            assert tr._fwd_cache is None and tr.fwd_reused == bool(reuse)
            if it == 0:
                torch.cuda.synchronize()
                first = (tr.gen_opt.flat_g.clone(), {n: float(getattr(tr, n).detach()) for n in vars(tr)
                                                     if n.startswith("loss_") and torch.is_tensor(getattr(tr, n))})
        torch.cuda.synchronize()
        return first, float(tr.loss_gen_total.detach()), float(tr.loss_dis_total.detach())

    ref, got = run(0), run(1)
    print("reuse_dis_forward with the semantic term: totals after three steps", ref[1:], got[1:])
    assert ref[0][1]["loss_sem_seg"] > 0
    assert ref[0][1] == got[0][1]
    assert flat_l2(got[0][0], ref[0][0]) <= 1e-5, flat_l2(got[0][0], ref[0][0])
    for a, b in zip(ref[1:], got[1:]):
        assert abs(a - b) <= 2e-3 * abs(a), (a, b)


def test_two_identical_steps_bitwise_equal(tmp_path, model):
    ckpt = _ckpt(tmp_path, model)
    hp = _hp(64, 2, ckpt)
    xa, xb, ma, mb = _inputs(2, 64, 5)
    outs = []
    for _ in range(2):
        tr = _trainer(hp, 0)
        _step(tr, hp, xa, xb, ma, mb)
        outs.append((tr.loss_sem_seg.item(), tr.gen_opt.flat_g.clone(), tr.gen_opt.flat_p.clone()))
    assert outs[0][0] == outs[1][0]
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])


def test_sample_returns_label_maps(tmp_path, model, sd):
    ckpt = _ckpt(tmp_path, model)
    hp = _hp(64, 2, ckpt)
    tr = _trainer(hp, 0)
    xa, xb, _, _ = _inputs(2, 64, 9)
    out = tr.sample(xa, xb)
    assert len(out) == 12
    rgb_a, x_ab1, rgb_ab = out[2], out[3], out[4]
    assert rgb_a.shape == (2, 3, 64, 64) and rgb_ab.shape == (2, 3, 64, 64)
    for img, rgb in ((xa, rgb_a), (x_ab1, rgb_ab), (xb, out[8]), (out[9], out[10])):
        up = S.logits(sd, img.cpu().double())
        top = up.topk(2, 1).values
        sure = ((top[:, 0] - top[:, 1]) > 1e-4).unsqueeze(1).expand(-1, 3, -1, -1)
        ref = S.colorize(up.argmax(1))
        assert torch.equal(rgb.cpu().double()[sure], ref.float().double()[sure])


def test_semantic_off_launches_no_seg_kernel(tmp_path, model):
    hp = O.default_hp(64, 2, 1)
    tr = _trainer(hp, 0)
    assert tr.segmentation_model is None
    xa, xb, ma, mb = _inputs(2, 64, 3)
    calls = []
    from munit_amd import _lib
    lib = _lib.load()
    names = [n for n in _lib.SIGNATURES if n.startswith(("munit_seg_", "munit_space_to_batch", "munit_maxpool",
                                                         "munit_add_relu"))]
    saved = {n: getattr(lib, n) for n in names}
    try:
        for n in names:
            f = saved[n]
            setattr(lib, n, (lambda f, n: lambda *a: calls.append(n) or f(*a))(f, n))
        with ops.kinks(seg=True) as k:
            _step(tr, hp, xa, xb, ma, mb)
        assert k.seg == [] and calls == []
    finally:
        for n, f in saved.items():
            setattr(lib, n, f)


# ------------------------------------------------------------------------------------------------------------------
# entry-point contract of seg.hip (tests/kernel_contract.py): a tiny, a ragged and a past-the-grid-cap shape each
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix", [1, 7 * 13, 1500000])
def test_contract_seg_input(npix):
    from tests import kernel_contract as K
    assert 3 * 1500000 > K.SEG_GRID_CAP
    K.check_seg_input(npix)


@pytest.mark.parametrize("shape", [(1, 2, 2, 1, 2), (3, 6, 9, 5, 3), (2, 7, 5, 19, 1), (2, 192, 192, 64, 2), (1, 8, 12, 3, 4)])
def test_contract_space_to_batch(shape):
    from tests import kernel_contract as K
    K.check_space_to_batch(*shape)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 7, 9, 5), (1, 2, 5, 3), (2, 384, 384, 64)])
def test_contract_maxpool(shape):
    from tests import kernel_contract as K
    K.check_seg_maxpool(*shape)


@pytest.mark.parametrize("n", [4, 4 * 333, 4 * (GRID_CAP + 1000)])
def test_contract_add_relu(n):
    from tests import kernel_contract as K
    K.check_add_relu(n)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 5, 3), (1, 5, 2, 8), (8, 96, 96, 8), (8, 192, 192, 2)])
@pytest.mark.parametrize("masked", [False, True])
def test_contract_seg_head(shape, masked):
    from tests import kernel_contract as K
    b, h, w, s = shape
    if (b, h) == (8, 96):
        assert b * h * s * w * s > K.SEG_GRID_CAP                      # loss, gradient and label kernels wrap
    if (b, h) == (8, 192):
        assert b * h * w * K.NCLS > K.SEG_GRID_CAP                     # the adjoint wraps
    K.check_seg_head(b, h, w, s, masked)
