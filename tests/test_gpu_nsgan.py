"""GPU tests of the non-saturating GAN loss (dis.gan_type: nsgan): the multi-scale nsgan kernels against fp64 softplus on the
host, their extremes, alignment and guard-band contract, ops.nsgan_loss, the three losses of MsImageDis against
tests/nsgan_oracle.py, whole steps through tests/parity.py, and that neither gan_type launches the other's kernels.

Bounds (those of tests/test_gpu_outda.py): a loss within 1e-5 relative of the fp64 yardstick, forward tensors within 1e-5
normalised maximum error, gradients within 5e-5, repeated runs bitwise equal.  They are relative, so the kernel cases keep
every reference value in fp32's normal range (asserted on the reference): a mean below 1.2e-38 cannot be held to 1e-5."""
import functools

import pytest
import torch

from munit_amd import ops
from oracle import munit_oracle as O
from tests import gan_loss_contract as G
from tests import nsgan_oracle as N
from tests import outda_oracle as D
from tests.conv_contract import Calls, no_nan
from tests.parity import nerr, pinned, record, run_step_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL, GRAD_TOL, LOSS_TOL = 1e-5, 5e-5, 1e-5
FLT_MIN = 1.1754943508222875e-38
NSGAN = ("munit_nsgan_fwd", "munit_nsgan_bwd")
OTHERS = ("munit_lsgan_fwd", "munit_lsgan_bwd", "munit_mse_const")
BIG = 1024 * 256 * 2 + 5
INF, NAN = float("inf"), float("nan")


# ---- the kernels --------------------------------------------------------------------------------------------------------
_raw = functools.partial(G.raw, G.NSGAN)
_segments = G.segments


def _softplus64(x, t):
    """per-element fp64 softplus(z) and d/dx = (1 - 2 t) sigmoid(z) of fp32 data"""
    z = x.double() * (1 - 2 * t)
    return torch.clamp_min(z, 0) + torch.log1p(torch.exp(-z.abs())), (1 - 2 * t) * torch.sigmoid(z)


def _confident(sizes, seed, targets):
    """every z = (1 - 2 t) x within -12 +- 1: the right side of the label, softplus(z) ~ exp(-12) = 6e-6"""
    g = torch.Generator().manual_seed(seed)
    return [((2 * t - 1) * (12 + 2 * torch.rand(n, generator=g) - 1)).float() for n, t in zip(sizes, targets)]


SIZES = {
    "one": [1],
    "tiny": [2, 1, 1],
    "block_edge": [255, 256, 257],
    "three_scales_two_halves": [512, 512, 128, 128, 32, 32],
    "eight": [1, 3, 64, 255, 256, 257, 1000, 4097],
    "wraps": [BIG],
}
CASES = [(k, s) for k in sorted(SIZES) for s in (1.0, 8.0, 30.0)] + [("block_edge", "confident"), ("eight", "confident")]


@pytest.mark.parametrize("case,scale", CASES, ids=["%s-%s" % c for c in CASES])
def test_kernels_against_fp64_softplus(case, scale):
    """scale 30 saturates the reference's own fp32 form (100 per element, zero gradient): the yardstick is fp64 softplus"""
    sizes = SIZES[case]
    targets = [float(i % 2) for i in range(len(sizes))]
    if scale == "confident":
        host = _confident(sizes, 31 + len(sizes), targets)
        assert all(float(((1 - 2 * t) * x + 12).abs().max()) <= 1.0 for x, t in zip(host, targets))
    else:
        host = _segments(sizes, 11 + len(sizes), scale)
    xs = [x.to(DEV) for x in host]
    gout = 3.0
    out, seg, dxs = _raw(xs, targets, gout=gout)
    refs = [_softplus64(x, t) for x, t in zip(host, targets)]
    means = [float(v.mean()) for v, _ in refs]
    want_dx = [gout / x.numel() * d for x, (_, d) in zip(host, refs)]
    assert min(means) >= FLT_MIN and min(float(d.abs().max()) for d in want_dx) >= FLT_MIN      # see the module docstring
    want = sum(means)
    rel = abs(float(out) - want) / abs(want)
    e_seg = max(abs(float(s) - m) / abs(m) for s, m in zip(seg.cpu(), means))
    e_dx = max(nerr(d, w) for d, w in zip(dxs, want_dx))
    print("nsgan %s x%s: out %.8g rel %.2e, worst segment rel %.2e, worst dx %.2e" % (case, scale, float(out), rel, e_seg, e_dx))
    assert rel <= LOSS_TOL and e_seg <= LOSS_TOL and e_dx <= GRAD_TOL
    if scale == "confident":
        assert all(2.26e-6 < m < 1.68e-5 for m in means)       # exp(-13) .. exp(-11): the mean of exp(z) is ~7e-6
    assert all(bool((d != 12345.0).all()) and no_nan(d) for d in dxs)      # every element written
    out2, seg2, dxs2 = _raw(xs, targets, gout=gout)                         # a second call is bitwise the first
    assert torch.equal(out, out2) and torch.equal(seg, seg2) and all(torch.equal(a, b) for a, b in zip(dxs, dxs2))
    out3, seg3, _ = _raw(xs, targets, gout=gout, with_seg=False)
    assert torch.equal(out, out3) and bool((seg3 == 12345.0).all())         # seg_out == NULL: the same out, nothing written


def _one(x, t, gout=1.5):
    out, seg, dxs = _raw([torch.tensor(x, device=DEV)], [t], gout=gout)
    return float(out), float(seg), dxs[0].cpu().tolist()


def test_the_extremes_have_their_exact_values():
    g = 1.5
    assert _one([1e4, -1e4], 0.0, g) == (5000.0, 5000.0, [g / 2, 0.0])
    assert _one([1e4, -1e4], 1.0, g) == (5000.0, 5000.0, [0.0, -g / 2])
    assert _one([INF, -INF], 0.0, g) == (INF, INF, [g / 2, 0.0])
    assert _one([INF, -INF], 1.0, g) == (INF, INF, [0.0, -g / 2])
    assert _one([-INF, -INF], 0.0, g) == (0.0, 0.0, [0.0, 0.0])             # the right side of the label: nothing to learn
    assert _one([INF, INF, INF], 1.0, g) == (0.0, 0.0, [0.0, 0.0, 0.0])
    assert _one([0.0], 0.0, g)[2] == [g / 2] and _one([0.0], 1.0, g)[2] == [-g / 2]
    # a segment of 300 elements (two blocks) with one infinity on the wrong side, and a finite neighbour segment
    x = torch.zeros(300)
    x[299] = -INF
    out, seg, dxs = _raw([x.to(DEV), torch.zeros(4, device=DEV)], [1.0, 0.0], gout=g)
    assert float(out) == INF and seg.cpu().tolist()[0] == INF and abs(float(seg[1]) - 0.6931471805599453) <= 1e-6
    assert bool((dxs[0][:299] == dxs[0][0]).all()) and no_nan(dxs[0]) and no_nan(dxs[1])
    assert abs(float(dxs[0][299]) + g / 300) <= 1e-6 * g / 300 and abs(float(dxs[0][0]) + g / 600) <= 1e-6 * g / 600


def test_a_nan_logit_stays_in_its_own_segment_and_its_own_element():
    xs = [torch.tensor([0.5, NAN, -0.5], device=DEV), torch.tensor([2.0, -2.0], device=DEV)]
    out, seg, dxs = _raw(xs, [0.0, 1.0], gout=1.0)
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(seg[0])) and not bool(torch.isnan(seg[1]))
    assert torch.isnan(dxs[0]).cpu().tolist() == [False, True, False] and no_nan(dxs[1])
    want = _softplus64(torch.tensor([0.5, -0.5]), 0.0)[1] / 3
    assert nerr(dxs[0][[0, 2]], want) <= GRAD_TOL


def test_unaligned_segment_starts_are_bitwise_the_aligned_run():
    """Segments at float offsets 1, 2 and 3 (mod 4) of one allocation, sizes 1, 5 and 257; dx likewise."""
    G.check_unaligned_segment_starts(G.NSGAN, scale=4.0)


@pytest.mark.parametrize("sizes", [(255, 256, 257), (1, 1026)])
def test_guard_bands(sizes):
    G.check_guard_bands(G.NSGAN, sizes)


# ---- ops.nsgan_loss -------------------------------------------------------------------------------------------------------
def _outs(b, seed, sizes=(4, 2, 1), scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return [scale * torch.randn(b, 1, s, s, generator=g) for s in sizes]


def _sp(x, t):
    return N.softplus(x, t)


@pytest.mark.parametrize("half", [1, 3])
def test_nsgan_loss_function(half):
    """pair targets over batches 2 and 6 (halves of 1 and 3: the 1x1 scale's second half starts 1 and 3 floats in)"""
    b = 2 * half
    host = _outs(b, 20 + b)
    xs = [t.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True) for t in host]
    ref = [t.double().requires_grad_(True) for t in host]
    l_ref = sum(_sp(r[:half], 0) + _sp(r[half:], 1) for r in ref)
    g_ref = torch.autograd.grad(3.0 * l_ref, ref)
    with Calls(NSGAN + OTHERS) as calls:
        loss = ops.nsgan_loss(xs, [(0.0, 1.0)] * 3)
        grads = torch.autograd.grad(loss, xs, torch.tensor(3.0, device=DEV))
        torch.cuda.synchronize()
    assert calls == ["munit_nsgan_fwd", "munit_nsgan_bwd"]
    assert abs(float(loss.detach()) - float(l_ref.detach())) <= LOSS_TOL * abs(float(l_ref.detach()))
    for x, g, r in zip(xs, grads, g_ref):
        assert g.shape == x.shape and g._base is None                  # one whole tensor per input, not a view
        assert nerr(g[:half], r[:half]) <= GRAD_TOL and nerr(g[half:], r[half:]) <= GRAD_TOL
    grads2 = torch.autograd.grad(ops.nsgan_loss(xs, [(0.0, 1.0)] * 3), xs, torch.tensor(3.0, device=DEV))
    assert all(torch.equal(a, c) for a, c in zip(grads, grads2))
    # plain targets: the whole tensor is one segment; (1, 0) pairs: the halves the other way round
    for targets, want in (([1.0, 1.0, 1.0], sum(_sp(r, 1) for r in ref)), ([0, 1, 0], _sp(ref[0], 0) + _sp(ref[1], 1) + _sp(ref[2], 0)),
                          ([(1.0, 0.0)] * 3, sum(_sp(r[:half], 1) + _sp(r[half:], 0) for r in ref))):
        got = ops.nsgan_loss(xs, targets)
        w_g = torch.autograd.grad(want, ref)
        assert abs(float(got.detach()) - float(want.detach())) <= LOSS_TOL * abs(float(want.detach()))
        assert max(nerr(a, r) for a, r in zip(torch.autograd.grad(got, xs), w_g)) <= GRAD_TOL


@pytest.mark.parametrize("pair", [False, True])
def test_more_scales_than_one_call_holds_go_in_groups(pair):
    """MsImageDis's grouping: 9 plain outputs are 8 + 1 segments, 5 paired outputs 4 + 1 outputs of two segments each"""
    from munit_amd.networks import MsImageDis
    sizes = (4, 3, 2, 1, 1, 2, 3, 4, 5) if not pair else (4, 3, 2, 1, 5)
    host = _outs(2, 77, sizes)
    targets = [(0.0, 1.0)] * len(sizes) if pair else [1.0] * len(sizes)
    xs = [t.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True) for t in host]
    ref = [t.double().requires_grad_(True) for t in host]
    l_ref = sum((_sp(r[:1], 0) + _sp(r[1:], 1)) if pair else _sp(r, 1) for r in ref)
    with Calls(NSGAN + OTHERS) as calls:
        loss = MsImageDis._multi_scale(ops.nsgan_loss, xs, targets)
        grads = torch.autograd.grad(loss, xs)
        torch.cuda.synchronize()
    assert sorted(calls) == ["munit_nsgan_bwd"] * 2 + ["munit_nsgan_fwd"] * 2
    assert abs(float(loss.detach()) - float(l_ref.detach())) <= LOSS_TOL * abs(float(l_ref.detach()))
    assert max(nerr(g, r) for g, r in zip(grads, torch.autograd.grad(l_ref, ref))) <= GRAD_TOL


def test_nsgan_loss_refusals():
    x = torch.randn(3, 1, 2, 2, device=DEV)
    with pytest.raises(RuntimeError, match="float32"):
        ops.nsgan_loss([x.double()], [0.0])
    with pytest.raises(RuntimeError, match="batch"):
        ops.nsgan_loss([x], [(0.0, 1.0)])
    y = torch.randn(2, 1, 2, 2, device=DEV)
    with pytest.raises(RuntimeError, match="8 segments"):
        ops.nsgan_loss([y] * 5, [(0.0, 1.0)] * 5)
    with pytest.raises(RuntimeError, match="8 segments"):
        ops.nsgan_loss([y] * 9, [0.0] * 9)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.nsgan_loss([y.cpu()], [0.0])
    with Calls(NSGAN) as calls:
        for bad in ([0.5], [(0.0, 0.5)], [2.0], [-1.0], [float("nan")]):
            with pytest.raises(RuntimeError, match="0 or 1"):
                ops.nsgan_loss([y], bad)
    assert calls == []


# ---- MsImageDis -----------------------------------------------------------------------------------------------------------
def _dis_hp():
    hp = O.default_hp(64, 2, 1)
    hp["dis"] = dict(hp["dis"], dim=8, gan_type="nsgan")
    assert hp["dis"]["num_scales"] == 3
    return hp


def _module(hp, tag):
    from munit_amd.networks import MsImageDis
    net = MsImageDis(hp["input_dim_a"], hp["dis"])
    sd = D.make_state(hp, tag)
    D.load_into(net, sd)
    for p in sd.values():
        p.requires_grad_(True)
    return net.to(DEV), sd


@pytest.fixture(scope="module")
def dis():
    ops.set_compute("f32")
    hp = _dis_hp()
    net, sd = _module(hp, "dis_a.")
    fake, real = D.images(2, 3, 64, 61), D.images(2, 3, 64, 62)
    # the literal form of tests/nsgan_oracle.py is the yardstick: the logits must be far from where sigmoid saturates in fp64
    assert N.max_logit(sd, [fake, real], hp["dis"]) < 16
    return hp, net, sd, fake, real


LOSSES = {
    "calc_dis_loss": (lambda net, x0, x1: net.calc_dis_loss(x0, x1), lambda sd, x0, x1, hd: N.dis_loss_d(sd, "", x0, x1, hd), 2),
    "calc_gen_loss": (lambda net, x0, x1: net.calc_gen_loss(x0), lambda sd, x0, x1, hd: N.dis_loss_g(sd, "", x0, hd), 1),
    "calc_dis_loss_sr": (lambda net, x0, x1: net.calc_dis_loss_sr(x0, x1), lambda sd, x0, x1, hd: N.dis_loss_sr(sd, x0, x1, hd), 2),
}


def _hip_loss(net, which, fake, real):
    xs = [ops.nhwc(t.float().to(DEV)).requires_grad_(True) for t in (fake, real)]
    loss = LOSSES[which][0](net, xs[0], xs[1])
    return loss, torch.autograd.grad(loss, xs[:LOSSES[which][2]] + list(net.parameters()))


@pytest.mark.parametrize("which", sorted(LOSSES))
def test_losses_against_the_oracle(dis, which):
    hp, net, sd, fake, real = dis
    nin = LOSSES[which][2]
    with Calls(NSGAN + OTHERS) as calls:
        (loss, grads), km, _ = record(lambda: _hip_loss(net, which, fake, real))
    assert calls == ["munit_nsgan_fwd", "munit_nsgan_bwd"]
    rs = [fake.clone().requires_grad_(True), real.clone().requires_grad_(True)]
    with pinned(km, which):
        l_ref = LOSSES[which][1](sd, rs[0], rs[1], hp["dis"])
    g_ref = torch.autograd.grad(l_ref, rs[:nin] + list(sd.values()))
    rel = abs(float(loss.detach()) - float(l_ref.detach())) / abs(float(l_ref.detach()))
    errs = [nerr(g, r) for g, r in zip(grads, g_ref)]
    print("%s nsgan: loss %.6f rel %.2e, worst input grad %.2e, worst weight grad %.2e"
          % (which, float(l_ref.detach()), rel, max(errs[:nin]), max(errs[nin:])))
    assert rel <= LOSS_TOL and max(errs) <= GRAD_TOL, (rel, errs)


def test_gen_loss_sr_is_refused_before_the_forward(dis):
    _, net, _, fake, _ = dis
    with Calls(("munit_",)) as calls:
        with pytest.raises(NotImplementedError, match="undefined variable"):
            net.calc_gen_loss_sr(fake.float().to(DEV))
    assert calls == []


@pytest.mark.parametrize("which", ["calc_dis_loss", "calc_dis_loss_sr"])
def test_the_batched_pair_path_matches_the_two_pass_path(dis, which, monkeypatch):
    from munit_amd import networks
    _, net, _, fake, real = dis
    res = []
    for batched in (True, False):
        monkeypatch.setattr(networks, "BATCH_DIS_PAIR", batched)
        with Calls(("munit_avgpool3s2_fwd",)) as pools:
            res.append(_hip_loss(net, which, fake, real))
            torch.cuda.synchronize()
        res[-1] += (len(pools),)
    (l1, g1, n1), (l2, g2, n2) = res
    assert (n1, n2) == (2, 4)                                             # one forward over [fake; real] against two
    assert abs(float(l1.detach()) - float(l2.detach())) <= LOSS_TOL * abs(float(l2.detach()))
    assert max(nerr(a, b) for a, b in zip(g1, g2)) <= GRAD_TOL


# ---- whole steps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen_state", [1, 0])
def test_step_parity_under_nsgan(gen_state):
    with N.swapped():
        rep = run_step_parity(size=64, batch=2, gen_state=gen_state, hp_overrides={"dis": {"gan_type": "nsgan"}})
    print("nsgan step, gen_state %d: %s" % (gen_state, {k: v for k, v in rep.items() if not isinstance(v, list)}))
    assert rep["loss_dis_total"] > 0 and rep["loss_gen_adv_a"] > 0


def _hp(**over):
    hp = O.default_hp(64, 2, 1)
    hp["gen"]["n_res"] = 1
    for k, v in over.items():
        hp[k] = dict(hp[k], **v) if isinstance(v, dict) else v
    return hp


def _step(hp):
    from munit_amd.trainer import MUNIT_Trainer
    torch.manual_seed(0)
    tr = MUNIT_Trainer(dict(hp)).to(DEV)
    x_a, x_b, m_a, m_b = [t.to(DEV) for t in O.synthetic_batch(2, 64, seed=7)]
    with Calls(NSGAN + OTHERS) as calls:
        tr.dis_update(x_a, x_b, hp)
        tr.gen_update(x_a, x_b, hp, m_a, m_b)
        torch.cuda.synchronize()
    return tr, calls


def test_neither_gan_type_launches_the_other_ones_kernels():
    tr, calls = _step(_hp())
    assert calls and not [c for c in calls if c.startswith("munit_nsgan")]
    tr, calls = _step(_hp(dis=dict(gan_type="nsgan")))
    # two discriminators in dis_update, two in gen_update: one launch pair each, and nothing of the LSGAN family
    assert sorted(calls) == ["munit_nsgan_bwd"] * 4 + ["munit_nsgan_fwd"] * 4
    assert float(tr.loss_dis_total.detach()) > 0 and float(tr.loss_gen_adv_a.detach()) > 0
    assert float(tr.gen_opt.flat_g.abs().max()) > 0
