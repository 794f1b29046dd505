"""GPU tests of the trainable segmentation head (adaptation.sem_seg_lambda): the two new kernel pairs of seg.hip against fp64
torch, their guard-band contract, the convolution forms the head reaches, the whole head and the trainer's update against
tests/seghead_oracle.py.

Bounds (the project's own, tests/test_gpu_featda.py and tests/parity.py): a loss within 1e-5 relative of the fp64 oracle,
gradients within 5e-5 normalised maximum error, forward tensors and running statistics 1e-5, Adam moments 1e-4 relative L2,
weights after a step 4 lr absolute and 2e-4 relative L2, a second call bitwise equal to the first.  The 7x7 average:
49 * 2^-24 * max|x|, the rounding of a 49-term fp32 sum.  The convolution op cases: 2e-5 normalised maximum error, or three
times the error of torch's own fp32 CPU evaluation where that is larger (DESIGN.md section 10's rule)."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from munit_amd import _lib, ops
from oracle import munit_oracle as O
from tests import seghead_oracle as H
from tests import semantic_oracle as S
from tests.conv_contract import Calls
from tests.parity import KINK_NOISE, l2err, nerr
from tests.test_gpu_featda import FWD_TOL, GRAD_TOL, LOSS_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEW = ("munit_avgpool7", "munit_seg_ce_direct")
POOL_EPS = 49 * 2.0 ** -24


def cl(t):
    return t.to(DEV, torch.float32).contiguous(memory_format=torch.channels_last)


# ---- the 7x7 average ---------------------------------------------------------------------------------------------------------
POOL_EXTENTS = [(h, w) for h in range(1, 10) for w in range(1, 10)] + [(16, 16), (20, 12)]


def _pool_pair(b, c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, c, h, w, generator=g) * 3 + 1
    dy = torch.randn(b, c, h, w, generator=g)
    return x, dy


def _pool_check(x, dy, ref_device="cpu"):
    xd, dyd = cl(x).requires_grad_(True), cl(dy)
    y = ops.avgpool7(xd)
    (dx,) = torch.autograd.grad(y, xd, dyd)
    yr = F.avg_pool2d(x.to(ref_device).double(), 7, 1, 3)
    dxr = F.avg_pool2d(dy.to(ref_device).double(), 7, 1, 3)             # the operator is its own adjoint
    ey = float((y.to(ref_device).double() - yr).abs().max())
    ed = float((dx.to(ref_device).double() - dxr).abs().max())
    assert ey <= POOL_EPS * float(x.abs().max()), (ey, tuple(x.shape))
    assert ed <= POOL_EPS * float(dy.abs().max()), (ed, tuple(x.shape))
    # <P x, dy> = <x, P dy> on the device's own outputs, in fp64
    xx, yy = x.to(ref_device).double(), dy.to(ref_device).double()
    lhs = float((y.to(ref_device).double() * yy).sum())
    rhs = float((xx * dx.to(ref_device).double()).sum())
    assert abs(lhs - rhs) <= POOL_EPS * float(xx.norm()) * float(yy.norm()), (lhs, rhs)
    y2 = ops.avgpool7(xd)
    assert torch.equal(y, y2)
    return ey, ed


@pytest.mark.parametrize("b,c", [(1, 4), (3, 12), (1, 512)])
def test_avgpool7_against_fp64(b, c):
    """Every extent 1..9 on both axes (below 7 everything is border), 16x16 and 20x12: values, the backward as the same
    operator, the adjoint identity, a second call bitwise the first."""
    worst = 0.0
    for i, (h, w) in enumerate(POOL_EXTENTS):
        x, dy = _pool_pair(b, c, h, w, 100 * b + i)
        worst = max(worst, *_pool_check(x, dy))
    x = torch.ones(b, c, 3, 4)          # no extent above 4: every window holds the whole map
    y = ops.avgpool7(cl(x)).cpu()
    assert torch.allclose(y, torch.full_like(y, 12 / 49), rtol=0, atol=1e-7)      # the padding is counted: always / 49
    print("avgpool7 B=%d C=%d: worst abs error %.2e" % (b, c, worst))


def test_avgpool7_past_the_grid_cap():
    from tests.seghead_contract import POOL_GRID_CAP, pool_items
    b, c, h, w = 3, 512, 128, 96
    assert pool_items(b, h, w, c) > POOL_GRID_CAP
    x, dy = _pool_pair(b, c, h, w, 7)
    _pool_check(x.to(DEV), dy.to(DEV), ref_device=DEV)


def test_avgpool7_rejects_bad_shapes():
    with pytest.raises(RuntimeError, match="C % 4"):
        ops.avgpool7(cl(torch.zeros(1, 6, 4, 4)))


# ---- the K-class head ----------------------------------------------------------------------------------------------------------
# (B, h, w, S, K, logit scale)
DIRECT_CASES = [
    (2, 3, 5, 8, 10, 3.0), (2, 5, 3, 4, 10, 3.0),                 # h != w, both orders
    (2, 1, 6, 4, 10, 3.0), (2, 6, 1, 2, 2, 3.0), (1, 1, 1, 8, 32, 3.0), (1, 4, 7, 1, 10, 3.0),
    (2, 4, 6, 1, 2, 3.0), (2, 6, 4, 2, 32, 3.0), (1, 5, 7, 4, 2, 3.0), (2, 3, 4, 8, 2, 3.0),
    (2, 4, 6, 4, 10, 20.0), (1, 6, 4, 8, 32, 20.0), (2, 5, 5, 2, 2, 20.0),       # logits ~ +-60
    (2, 16, 16, 4, 10, 3.0),                                         # the update's shape at crop 64
    (8, 96, 96, 8, 10, 3.0),                                         # 4.7 M pixels: loss and gradient wrap the grid
]


def _direct_case(b, h, w, sc, k, zs, seed):
    g = torch.Generator().manual_seed(seed)
    z = (zs * torch.randn(b, k, h, w, generator=g, dtype=torch.float64)).float().double()
    gt = torch.randint(0, k, (b, h * sc, w * sc), generator=g).double()
    gt[:, ::2] += 0.75                             # the loader's floats are truncated, not rounded
    gt[0, 0, 0], gt[-1, -1, -1] = 0.0, k - 1 + 0.5      # labels 0 and K - 1
    return z, gt


def _direct_run(z, gt, sc, norm=None):
    zd = cl(z).requires_grad_(True)
    gd = gt.float().to(DEV).contiguous()
    loss = ops.seg_cross_entropy_direct(zd, gd, sc, norm)
    loss.backward()
    g1 = zd.grad.clone()
    zd.grad = None
    loss2 = ops.seg_cross_entropy_direct(zd, gd, sc, norm)
    loss2.backward()
    bits = lambda t: t.detach().reshape(1).view(torch.int32)      # bitwise: a NaN loss equals itself
    assert torch.equal(bits(loss), bits(loss2)) and torch.equal(g1, zd.grad), "a second call differs"
    return loss, g1


@pytest.mark.parametrize("case", DIRECT_CASES, ids=lambda c: "b%d_%dx%d_s%d_k%d_z%g" % c)
def test_direct_head_loss_and_dlogits(case):
    """ops.seg_cross_entropy_direct against F.interpolate + F.cross_entropy in fp64 with test_gt_head_loss_and_dlogits'
    bounds: loss 1e-5 relative, dlogits 5e-5 normalised max, a bitwise second call."""
    b, h, w, sc, k, zs = case
    big = b * h * w * sc * sc > 1 << 20
    nb = 2 if big else b                           # the fp64 reference of the large case runs on 2 distinct images, tiled
    z, gt = _direct_case(nb, h, w, sc, k, zs, 1000 * h + 10 * w + sc + k)
    zr = z.clone().requires_grad_(True)
    up = F.interpolate(zr, size=(h * sc, w * sc), mode="bilinear", align_corners=False)
    ref = F.cross_entropy(up, gt.long())
    ref.backward()
    copies = b // nb
    loss, grad = _direct_run(torch.cat([z] * copies), torch.cat([gt] * copies), sc)
    print("direct head %s: loss %.8g ref %.8g" % (case, loss.item(), ref.item()))
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item()), (loss.item(), ref.item())
    gd = grad.cpu()
    for i in range(1, copies):
        assert torch.equal(gd[i * nb:(i + 1) * nb], gd[:nb]), "copies of the same image differ"
    assert nerr(gd[:nb], zr.grad / copies) < 5e-5, nerr(gd[:nb], zr.grad / copies)
    # norm: the sum of the pixel losses over it
    loss_h, _ = _direct_run(torch.cat([z] * copies), torch.cat([gt] * copies), sc, gt.numel() * copies / 2)
    assert abs(loss_h.item() - 2 * ref.item()) <= 1e-5 * abs(2 * ref.item())


@pytest.mark.parametrize("bad", [10.0, -1.0, float("nan"), float("inf"), 3.0e9])
def test_direct_head_invalid_label_gives_nan_loss_and_zero_gradient_there(bad):
    """include/munit_hip.h: a label outside 0..K-1 is never an index; the loss is NaN, both calls return OK, the pixel's
    gradient is 0 -- so dlogits equals that of the same map with the pixel removed from the sum."""
    b, h, w, sc, k = 2, 3, 5, 4, 10
    z, gt = _direct_case(b, h, w, sc, k, 3.0, 9)
    gt[1, 7, 11] = bad
    loss, grad = _direct_run(z, gt, sc)
    torch.cuda.synchronize()
    assert math.isnan(loss.item())
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
    zr = z.clone().requires_grad_(True)
    up = F.interpolate(zr, size=(h * sc, w * sc), mode="bilinear", align_corners=False)
    good = gt.clone()
    good[1, 7, 11] = 0
    pix = F.cross_entropy(up, good.long(), reduction="none")
    keep = torch.ones_like(pix)
    keep[1, 7, 11] = 0
    ((pix * keep).sum() / gt.numel()).backward()
    assert nerr(grad.cpu(), zr.grad) < 5e-5
    # -0.5 truncates to 0 like .type(torch.long): a valid label
    gt[1, 7, 11] = -0.5
    loss, _ = _direct_run(z, gt, sc)
    assert math.isfinite(loss.item())


def test_direct_head_rejects_wrong_tensors():
    z = cl(torch.zeros(1, 10, 2, 2))
    with pytest.raises(RuntimeError, match="float32"):
        ops.seg_cross_entropy_direct(z, torch.zeros(1, 8, 8, device=DEV, dtype=torch.int32), 4)
    with pytest.raises(RuntimeError, match="target"):
        ops.seg_cross_entropy_direct(z, torch.zeros(1, 8, 16, device=DEV), 4)
    with pytest.raises(RuntimeError, match="scale"):
        ops.seg_cross_entropy_direct(z, torch.zeros(1, 6, 6, device=DEV), 3)
    with pytest.raises(RuntimeError, match="classes"):
        ops.seg_cross_entropy_direct(cl(torch.zeros(1, 33, 2, 2)), torch.zeros(1, 8, 8, device=DEV), 4)


# ---- guard bands (tests/seghead_contract.py) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 5, 9, 12), (1, 7, 3, 512), (3, 20, 12, 8), (3, 128, 96, 512)])
def test_contract_avgpool7(shape):
    from tests import seghead_contract as K
    if shape[3] == 512 and shape[1] == 128:
        assert K.pool_items(*shape) > K.POOL_GRID_CAP
    K.check_avgpool7(*shape)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 2), (2, 3, 5, 4, 10), (1, 5, 2, 8, 32), (2, 16, 16, 4, 10), (8, 96, 96, 8, 10)])
def test_contract_direct_head(shape):
    from tests import kernel_contract as KC
    from tests import seghead_contract as K
    b, h, w, s, k = shape
    if (b, h) == (8, 96):
        assert b * h * s * w * s > KC.SEG_GRID_CAP
    K.check_direct_head(b, h, w, s, k)


# ---- the convolution forms the head dispatches to (tests/test_cpu_seghead.py names them) ----------------------------------------
_WINO, _WINO_W = "conv_wino_kernel<1, 0>", "conv_wino_wgrad_kernel<false, false, false> + wino_wgrad_reduce_kernel"
_FWD, _DIRECT, _PATCH = "conv_igemm_kernel<fwd>", "conv_igemm_kernel<dgrad direct>", "conv_igemm_kernel<.., 2, 3> (LDS-patch fold)"
_SLAB = "conv_wgrad_kernel + slab_reduce_kernel"
# (cin, cout, k, bias, images, h, w): the phase images of a 16x16 code (crop 64), of a 20x20 one (crop 80: odd 5x5 images take
# other kernels) and of a 64x64 one (crop 256), batch 1; the scoring layer on the plain 16x16 code
HEAD_CONV_CASES_TARGETS = {
    (256, 512, 3, False, 16, 4, 4): (_WINO, None, _WINO_W),
    (256, 512, 3, False, 16, 5, 5): (_FWD, None, _SLAB),
    (512, 512, 3, False, 16, 4, 4): (_WINO, _WINO, _WINO_W),
    (512, 512, 3, False, 16, 5, 5): (_FWD, _PATCH, _SLAB),
    (512, 512, 3, False, 16, 16, 16): (_WINO, _WINO, _WINO_W),
    (256, 512, 1, False, 16, 4, 4): (_FWD, None, _SLAB),
    (256, 512, 1, False, 16, 5, 5): (_FWD, None, _SLAB),
    (512, 10, 1, True, 1, 16, 16): (_FWD, _DIRECT, _SLAB),
    (512, 10, 1, True, 2, 20, 20): (_FWD, _DIRECT, _SLAB),
}
HEAD_CONV_CASES = list(HEAD_CONV_CASES_TARGETS)
HEAD_CONV_TOL = 2e-5


def head_op_case(c):
    """tests/test_cpu_dispatch.py's op-case tuple of a HEAD_CONV_CASES entry"""
    cin, cout, k, bias, n, h, w = c
    return (cin, cout, k, 1, k // 2, "zero", 0, "none", n, h, w)


@pytest.mark.parametrize("case", HEAD_CONV_CASES, ids=lambda c: "c%d-%d_k%d_b%d_n%d_%dx%d" % tuple(int(v) for v in c))
def test_head_conv_forms_against_fp64(case):
    from tests.test_cpu_dispatch import kernel_names
    cin, cout, k, bias, n, h, w = case
    names = kernel_names(_lib.load(), head_op_case(case))
    for got, want in zip(names, HEAD_CONV_CASES_TARGETS[case]):
        assert want is None or got == want, (case, names)
    g = torch.Generator().manual_seed(k * 1000 + cin + cout + h)
    x = torch.randn(n, cin, h, w, generator=g).clamp_min(0)
    wt = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * k * k))
    bs = torch.randn(cout, generator=g) * 0.1 if bias else None
    dy = torch.randn(n, cout, h, w, generator=g)

    def ref(dt):
        xr, wr = x.to(dt).requires_grad_(True), wt.to(dt).requires_grad_(True)
        br = None if bs is None else bs.to(dt).requires_grad_(True)
        yr = F.conv2d(xr, wr, br, padding=k // 2)
        gs = torch.autograd.grad(yr, [xr, wr] + ([br] if bias else []), dy.to(dt))
        return [yr.detach()] + list(gs)

    r64, r32 = ref(torch.float64), ref(torch.float32)
    yard = [nerr(a, b) for a, b in zip(r32, r64)]
    ops.set_compute("f32")
    xd, wd = cl(x).requires_grad_(True), cl(wt).requires_grad_(True)
    bd = None if bs is None else bs.to(DEV).requires_grad_(True)
    y = ops.conv2d(xd, wd, bd, 1, k // 2, "zero")
    gs = torch.autograd.grad(y, [xd, wd] + ([bd] if bias else []), cl(dy))
    ops.join_side_streams()
    errs = [nerr(a, b) for a, b in zip([y] + list(gs), r64)]
    print("head conv %s %s: fwd / dgrad / wgrad%s %s (fp32 CPU %s)"
          % (case, names, " / dbias" if bias else "", ["%.2e" % e for e in errs], ["%.2e" % e for e in yard]))
    for e, yd in zip(errs, yard):
        assert e <= max(HEAD_CONV_TOL, 3 * yd), (errs, yard)


# ---- the head alone --------------------------------------------------------------------------------------------------------------
def _module(fc_seed=5):
    from munit_amd.segmentation import SegmentationHead
    net = SegmentationHead()
    sd = H.make_state(0, fc_seed)
    H.load_into(net, sd)
    return net.to(DEV), sd


def _run_module(net, c, t, sc):
    ops.set_compute("f32")
    with ops.kinks(dann=True) as k:
        out = net(cl(c))
    sink = k.dann
    loss = ops.seg_cross_entropy_direct(out, t.reshape(t.shape[0], t.shape[2], t.shape[3]).float().to(DEV).contiguous(), sc)
    ps = list(net.parameters())
    grads = torch.autograd.grad(loss, ps)
    ops.join_side_streams()
    torch.cuda.synchronize()
    return loss, out, list(grads), sink


@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("hw", [16, 20])
def test_head_against_the_oracle(b, hw):
    """One forward + backward of the head on a seeded code (16x16: even 4x4 phase images, 20x20: odd 5x5 ones) with the ReLU
    signs pinned: loss, logits, every weight gradient, the running statistics."""
    net, sd = _module()
    c, t = H.code(b, hw, hw, 43 + b), H.labels(b, 4 * hw, 47 + b)
    before = {k: v.clone() for k, v in sd.items()}
    loss, out, dws, sink = _run_module(net, c, t, 4)
    assert len(sink) == H.PINS_PER_FORWARD
    pins = H.head_pins(sink)
    ps = H.params(sd)
    for p in ps:
        p.requires_grad_(True)
    o_ref = H.head(sd, c, pins)
    assert pins.done() and pins.worst <= KINK_NOISE, (pins.worst, pins.n_disagree)     # pinned only within rounding of a kink
    l_ref = H.ce(o_ref, t, 4 * hw)
    g_ref = torch.autograd.grad(l_ref, ps)
    rel = abs(float(loss) - float(l_ref)) / abs(float(l_ref))
    e_out = nerr(out, o_ref)
    e_w = {n: nerr(g, r) for n, g, r in zip(H.param_names(), dws, g_ref)}
    e_s = {k: nerr(v, sd[k]) for k, v in net.state_dict().items() if k.endswith(("running_mean", "running_var"))}
    print("head B=%d %dx%d: loss rel %.2e out %.2e worst weight grad %.2e (%s) worst statistic %.2e, %d pinned, worst kink %.2e"
          % (b, hw, hw, rel, e_out, max(e_w.values()), max(e_w, key=e_w.get), max(e_s.values()), pins.n_disagree, pins.worst))
    assert rel <= LOSS_TOL and e_out <= FWD_TOL
    assert max(e_w.values()) <= GRAD_TOL, e_w
    assert max(e_s.values()) <= FWD_TOL, e_s
    own = net.state_dict()
    for k in sd:
        if k.endswith(("running_mean", "running_var")):
            assert not torch.equal(sd[k], before[k])
        elif k.endswith("num_batches_tracked"):
            assert int(own[k]) == int(sd[k]) == 1


# ---- the trainer's update -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    p = tmp_path_factory.mktemp("seghead") / "seg.pth"
    torch.save(S.make_model(0).state_dict(), str(p))
    return str(p)


def _hp(ckpt, gen_state=1, size=64, **adaptation):
    hp = O.default_hp(size, 2, gen_state)
    hp["gen"]["n_res"] = 1
    hp["dis"]["num_scales"] = 1
    hp["adaptation"].update(adaptation)
    hp["semantic_ckpt_path"] = ckpt
    return hp


def _trainer(hp, seed=0):
    from munit_amd.trainer import MUNIT_Trainer
    torch.manual_seed(seed)
    return MUNIT_Trainer(dict(hp)).to(DEV)


def _codes(tr, x_a, x_b):
    with torch.no_grad():
        return (tr._content_enc(1)(ops.nhwc(x_a)).cpu().double(), tr._content_enc(2)(ops.nhwc(x_b)).cpu().double())


@pytest.mark.parametrize("gen_state", [0, 1])
def test_update_against_the_oracle(ckpt, gen_state):
    """Two consecutive segmentation_head_update calls at crop 64, batch 2, n_res 1 against tests/seghead_oracle.py run on
    the content codes the HIP encoders produced, by tests/parity.py's rules: before each call the oracle takes over the HIP
    head (its Adam moments and step count carry over); after it the weighted loss, every weight gradient with the ReLU signs
    pinned, the Adam moments, the weights after the step, the running statistics.  Generator and discriminator buffers are
    bitwise untouched."""
    lamb = 0.7
    hp = _hp(ckpt, gen_state, sem_seg_lambda=lamb)
    tr = _trainer(hp)
    lr = hp["lr"]
    x_a, x_b, _, _ = [t.to(DEV) for t in O.synthetic_batch(2, 64)]
    t_a, t_b = H.labels(2, 64, 71), H.labels(2, 64, 72)
    sd = H.state_of(tr.segmentation_head)
    opt = H.HeadOptimizer(sd, hp)
    keep = {n: t.clone() for n, t in (("gen.p", tr.gen_opt.flat_p), ("gen.g", tr.gen_opt.flat_g), ("dis.p", tr.dis_opt.flat_p),
                                      ("dis.g", tr.dis_opt.flat_g))}
    tr.gen_opt.flat_g.fill_(3.0)          # a gradient the reference would overwrite and the next gen_update zero: untouched here
    keep["gen.g"] = tr.gen_opt.flat_g.clone()
    c_a, c_b = _codes(tr, x_a, x_b)       # the generator does not move between the calls
    names = H.param_names()
    worst = dict(loss=0.0, grad_max=0.0, grad_l2=0.0, moment_l2=0.0, weight_abs=0.0, weight_l2=0.0, stat=0.0, kink=0.0)
    for call in range(2):
        if call:                           # re-synchronise, as tests/parity.run_step_parity does between iterations
            with torch.no_grad():
                for k, v in H.state_of(tr.segmentation_head).items():
                    sd[k].copy_(v)
        tr.iterations = call
        with ops.kinks(dann=True) as k:
            tr.segmentation_head_update(x_a, x_b, t_a.to(DEV), t_b.to(DEV), lamb)
        torch.cuda.synchronize()
        sink = k.dann
        assert len(sink) == 2 * H.PINS_PER_FORWARD
        pins = H.head_pins(sink)
        l_ref, g_ref = H.head_update(sd, opt, c_a, c_b, t_a, t_b, lamb, 64, pins)
        assert pins.done()
        worst["kink"] = max(worst["kink"], pins.worst)
        worst["loss"] = max(worst["loss"], abs(float(tr.loss_semantic_head) - float(l_ref)) / abs(float(l_ref)))
        own = tr.segmentation_head.state_dict()
        for (n, p), g, (mv, vv), om, ov in zip(tr.segmentation_head.named_parameters(), g_ref, tr.segmentation_opt._views,
                                               opt.m, opt.v):
            assert n in names
            worst["grad_max"] = max(worst["grad_max"], nerr(p._munit_grad, g))
            worst["grad_l2"] = max(worst["grad_l2"], l2err(p._munit_grad, g))
            worst["moment_l2"] = max(worst["moment_l2"], l2err(mv, om), l2err(vv, ov))
            a, r = p.detach().double().cpu(), sd[n].detach()
            worst["weight_abs"] = max(worst["weight_abs"], float((a - r).abs().max()))
            worst["weight_l2"] = max(worst["weight_l2"], l2err(a, r))
        for k, v in sd.items():
            if k.endswith(("running_mean", "running_var")):
                worst["stat"] = max(worst["stat"], nerr(own[k], v))
            elif k.endswith("tracked"):
                assert int(own[k]) == int(v) == 2 * (call + 1), k
        assert tr.segmentation_opt._step == opt.step_count == call + 1
    print("segmentation_head_update gen_state %d: %s" % (gen_state, {k: "%.2e" % v for k, v in worst.items()}))
    assert int(tr.segmentation_head.state_dict()["0.2.bn2.num_batches_tracked"]) == 4
    for n, t in (("gen.p", tr.gen_opt.flat_p), ("gen.g", tr.gen_opt.flat_g), ("dis.p", tr.dis_opt.flat_p),
                 ("dis.g", tr.dis_opt.flat_g)):
        assert torch.equal(t, keep[n]), n
    assert worst["kink"] <= KINK_NOISE, worst
    assert worst["loss"] <= LOSS_TOL, worst
    assert worst["grad_max"] <= GRAD_TOL and worst["grad_l2"] <= GRAD_TOL, worst
    assert worst["moment_l2"] <= 2 * GRAD_TOL, worst
    assert worst["weight_abs"] <= 4.0 * lr and worst["weight_l2"] <= 2e-4, worst
    assert worst["stat"] <= FWD_TOL, worst


def test_two_identical_updates_are_bitwise_equal(ckpt):
    hp = _hp(ckpt, sem_seg_lambda=1)
    x_a, x_b, _, _ = [t.to(DEV) for t in O.synthetic_batch(2, 64)]
    t_a, t_b = H.labels(2, 64, 71).to(DEV), H.labels(2, 64, 72).to(DEV)
    res = []
    for _ in range(2):
        tr = _trainer(hp)
        tr.segmentation_head_update(x_a, x_b, t_a, t_b.reshape(2, 64, 64), 1)       # (B, 1, H, W) and (B, H, W)
        torch.cuda.synchronize()
        res.append((tr.segmentation_opt.flat_p.clone(), tr.segmentation_opt.flat_g.clone(), tr.loss_semantic_head.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert float(res[0][1].abs().max()) > 0 and float(res[0][2]) > 0
    # a label map on the host while the images are on the device is refused before anything moves
    tr.segmentation_opt.flat_g.fill_(3.0)
    with pytest.raises(ValueError, match="target_b.*device"):
        tr.segmentation_head_update(x_a, x_b, t_a, t_b.cpu(), 1)
    assert bool((tr.segmentation_opt.flat_g == 3.0).all())
    # an invalid device label: NaN loss, finite weights (include/munit_hip.h)
    bad = t_a.clone()
    bad[0, 0, 3, 3] = 12.0
    tr.segmentation_head_update(x_a, x_b, bad, t_b, 1)
    assert math.isnan(float(tr.loss_semantic_head)) and bool(torch.isfinite(tr.segmentation_opt.flat_p).all())


def test_zero_weight_launches_none_of_the_new_kernels(ckpt):
    hp = _hp(ckpt)
    tr = _trainer(hp)
    assert not tr.train_seg and not hasattr(tr, "segmentation_head")
    x_a, x_b, m_a, m_b = [t.to(DEV) for t in O.synthetic_batch(2, 64)]
    with Calls(NEW) as calls:
        tr.dis_update(x_a, x_b, hp)
        tr.gen_update(x_a, x_b, hp, m_a, m_b)
        torch.cuda.synchronize()
    assert calls == []
    on = _hp(ckpt, sem_seg_lambda=1)
    tr = _trainer(on)
    t = H.labels(2, 64, 71).to(DEV)
    with Calls(NEW + ("munit_batchnorm", "munit_space_to_batch")) as calls:
        tr.dis_update(x_a, x_b, on)
        tr.gen_update(x_a, x_b, on, m_a, m_b)
        assert calls == []
        tr.segmentation_head_update(x_a, x_b, t, t, 1)
        torch.cuda.synchronize()
    # two forwards of the head: one pool, one loss, seven batch norms, a split and its inverse each, forward and backward
    # (the split's backward is skipped: the code carries no tape)
    assert calls.count("munit_avgpool7_fwd") == calls.count("munit_avgpool7_bwd") == 2
    assert calls.count("munit_seg_ce_direct_fwd") == calls.count("munit_seg_ce_direct_bwd") == 2
    assert calls.count("munit_batchnorm_fwd") == calls.count("munit_batchnorm_bwd") == 14
    assert calls.count("munit_space_to_batch") == 6


# ---- a whole iteration ----------------------------------------------------------------------------------------------------------
def test_featureda_iteration_with_the_head(tmp_path):
    """One run_iteration of the FeatureDA class (tests/final_configs.reduced_hp) with sem_seg_lambda: 1 added, on the iteration
    its classifier updates fall on: the head's update comes last, steps once, and the run leaves no sink or kept forward."""
    from munit_amd.trainer import MUNIT_Trainer
    from tests import final_configs as C
    from train_loop import run_iteration
    p = tmp_path / "seg.pth"
    torch.save(S.make_model(0).state_dict(), str(p))
    hp = C.reduced_hp(C.load(), "FeatureDA", str(p))
    hp["adaptation"]["sem_seg_lambda"] = 1
    real, synth = C.inputs(hp)
    dreal = tuple(t.to(DEV) for t in real)
    dsynth = tuple(t.to(DEV) for t in synth)
    torch.manual_seed(0)
    tr = MUNIT_Trainer(dict(hp)).to(DEV)
    order = []

    def pairs():
        while True:
            yield dsynth

    run_iteration(tr, hp, 1, dreal, pairs(), lambda name, args, run: order.append(name) or run())
    torch.cuda.synchronize()
    assert order[-1] == "segmentation_head_update" and order.count("segmentation_head_update") == 1
    assert order.count("domain_classifier_sr_update") == 2 and order.count("gen_update") == 2
    assert tr.segmentation_opt._step == 1 and math.isfinite(float(tr.loss_semantic_head)) and float(tr.loss_semantic_head) > 0
    for s in ("MASK_SINK", "L1_SINK", "SEG_SINK", "DANN_SINK"):
        assert getattr(ops, s) is None, s
    assert tr._fwd_cache is None
    tr.dis_opt.settle()
    assert tr.dis_opt.gate.pending is None and tr.dis_opt.gate.waited == set()
    for m in (tr.gen, tr.dis_a, tr.dis_b, tr.domain_classifier_sr_a, tr.domain_classifier_sr_b, tr.segmentation_head):
        assert all(q.requires_grad for q in m.parameters())
    for name, opt in (("gen", tr.gen_opt), ("dis", tr.dis_opt), ("feat", tr.classif_opt_sr), ("seg", tr.segmentation_opt)):
        assert bool(torch.isfinite(opt.flat_p).all()), name
