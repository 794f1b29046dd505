"""GPU tests of output-level domain adaptation (adaptation.output_classifier_lambda / output_adv_lambda): the multi-scale
LSGAN kernels against fp64 torch on the host, their alignment and guard-band contract, ops.lsgan_loss, the two losses of
MsImageDis and the trainer's updates against tests/outda_oracle.py.

Bounds (the project's own, tests/test_gpu_featda.py and tests/parity.py): a loss within 1e-5 relative of the fp64 oracle,
forward tensors within 1e-5 normalised maximum error, gradients within 5e-5, repeated runs bitwise equal; weights after an
Adam step within 4 lr and 2e-4 relative L2 per tensor, the Adam moments within 2 x 5e-5 relative L2."""
import functools

import numpy as np
import pytest
import torch

from munit_amd import ops
from oracle import munit_oracle as O
from tests import gan_loss_contract as G
from tests import outda_oracle as D
from tests.conv_contract import Calls, no_nan
from tests.parity import l2err, load_into_trainer, nerr, oracle_states, pinned, record, trainer_named_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL, GRAD_TOL, LOSS_TOL = 1e-5, 5e-5, 1e-5
NEW = ("munit_lsgan_workspace_bytes", "munit_lsgan_fwd", "munit_lsgan_bwd")
ON = dict(output_classifier_lambda=1, output_adv_lambda=1)
BIG = 1024 * 256 * 2 + 5


# ---- the kernels --------------------------------------------------------------------------------------------------------
_raw = functools.partial(G.raw, G.LSGAN)
_segments = G.segments


CASES = {
    "one": ([1], 1.0),
    "tiny": ([2, 1, 1], 1.0),
    "block_edge": ([255, 256, 257], 1.0),
    "block_edge_1e3": ([255, 256, 257], 1e3),
    "three_scales_two_halves": ([512, 512, 128, 128, 32, 32], 1.0),
    "eight": ([1, 3, 64, 255, 256, 257, 1000, 4097], 1.0),
    "wraps": ([BIG], 1.0),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_kernels_against_fp64(case):
    sizes, scale = CASES[case]
    targets = [0.0, 1.0] * 3 if case == "three_scales_two_halves" else [(0.0, 1.0, 0.5)[i % 3] for i in range(len(sizes))]
    host = _segments(sizes, 11 + len(sizes), scale)
    xs = [x.to(DEV) for x in host]
    gout = 3.0
    out, seg, dxs = _raw(xs, targets, gout=gout)
    means = [((x.double() - t) ** 2).mean() for x, t in zip(host, targets)]
    want = float(sum(means))
    rel = abs(float(out) - want) / abs(want)
    e_seg = max(abs(float(s) - float(m)) / abs(float(m)) for s, m in zip(seg.cpu(), means))
    e_dx = max(nerr(d, 2 * gout / x.numel() * (x.double() - t)) for d, x, t in zip(dxs, host, targets))
    print("lsgan %s: out %.8g rel %.2e, worst segment rel %.2e, worst dx %.2e" % (case, float(out), rel, e_seg, e_dx))
    assert rel <= LOSS_TOL and e_seg <= LOSS_TOL and e_dx <= GRAD_TOL
    assert all(no_nan(d) for d in dxs)                  # every element written
    out2, seg2, dxs2 = _raw(xs, targets, gout=gout)     # a second call is bitwise the first
    assert torch.equal(out, out2) and torch.equal(seg, seg2) and all(torch.equal(a, b) for a, b in zip(dxs, dxs2))
    out3, seg3, _ = _raw(xs, targets, gout=gout, with_seg=False)
    assert torch.equal(out, out3) and bool(torch.isnan(seg3).all())     # seg_out == NULL: the same out, nothing written


def test_lsgan_arithmetic_on_the_integer_lattice():
    """Integer logits in [-8, 8], targets 0 / 1 / 0.5: every (x - t)^2 is a multiple of 0.25 and a
    segment's sum stays below 2^24 quarter-units (4097 * 81 * 4 < 2^21), so the fp32 sum is exact in any order and the
    expected bits come from numpy alone: the mean as float64(sum) * (1 / float64(n)), out as the float64 sum of the means in
    index order, dx as g = 2 * gout / n, dx = g * (x - t) with one fp32 rounding per operation."""
    sizes, gout = [1, 3, 255, 256, 257, 4097], np.float32(3.0)
    targets = G.cycle(G.LSGAN, len(sizes))
    rng = np.random.RandomState(17)
    host = [rng.randint(-8, 9, size=n).astype(np.float32) for n in sizes]
    out, seg, dxs = _raw([torch.from_numpy(x).to(DEV) for x in host], targets, gout=float(gout))
    sums = [np.sum((x.astype(np.float64) - t) ** 2) for x, t in zip(host, targets)]
    assert all(s * 4 == int(s * 4) and s * 4 < 2 ** 24 for s in sums)
    means = [s * (1.0 / np.float64(n)) for s, n in zip(sums, sizes)]
    total = np.float64(0.0)
    for m in means:
        total += m
    assert seg.cpu().numpy().tobytes() == np.asarray(means, np.float64).astype(np.float32).tobytes()
    assert out.cpu().numpy().tobytes() == np.float32(total).tobytes()
    for x, t, n, dx in zip(host, targets, sizes, dxs):
        g = np.float32(2.0) * gout / np.float32(n)
        want = g * (x - np.float32(t))
        assert want.dtype == np.float32 and dx.cpu().numpy().tobytes() == want.tobytes(), "dx of the segment of %d" % n


def test_unaligned_segment_starts_are_bitwise_the_aligned_run():
    """Segments at float offsets 1, 2 and 3 (mod 4) of one allocation, sizes 1, 5 and 257; dx likewise."""
    G.check_unaligned_segment_starts(G.LSGAN)


@pytest.mark.parametrize("sizes", [(255, 256, 257), (1, 1026)])
def test_guard_bands(sizes):
    G.check_guard_bands(G.LSGAN, sizes)


# ---- ops.lsgan_loss -------------------------------------------------------------------------------------------------------
def _outs(b, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(b, 1, s, s, generator=g) for s in (4, 2, 1)]


@pytest.mark.parametrize("b", [2, 6])
def test_lsgan_loss_function(b):
    host = _outs(b, 20 + b)
    xs = [t.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True) for t in host]
    ref = [t.double().requires_grad_(True) for t in host]
    l_ref = sum(torch.mean(r[:b // 2] ** 2) + torch.mean((r[b // 2:] - 1) ** 2) for r in ref)
    g_ref = torch.autograd.grad(3.0 * l_ref, ref)
    with Calls(("munit_lsgan_fwd", "munit_lsgan_bwd", "munit_mse_const")) as calls:
        loss = ops.lsgan_loss(xs, [(0.0, 1.0)] * 3)
        grads = torch.autograd.grad(loss, xs, torch.tensor(3.0, device=DEV))
        torch.cuda.synchronize()
    assert calls == ["munit_lsgan_fwd", "munit_lsgan_bwd"]
    assert abs(float(loss.detach()) - float(l_ref.detach())) <= LOSS_TOL * abs(float(l_ref.detach()))
    for x, g, r in zip(xs, grads, g_ref):
        assert g.shape == x.shape and g._base is None                  # one whole tensor per input, not a view
        assert nerr(g[:b // 2], r[:b // 2]) <= GRAD_TOL and nerr(g[b // 2:], r[b // 2:]) <= GRAD_TOL
    grads2 = torch.autograd.grad(ops.lsgan_loss(xs, [(0.0, 1.0)] * 3), xs, torch.tensor(3.0, device=DEV))
    assert all(torch.equal(a, c) for a, c in zip(grads, grads2))
    # plain targets: the whole tensor is one segment
    l1 = ops.lsgan_loss(xs, [0.5, 0.5, 0.5])
    w1 = sum(torch.mean((r - 0.5) ** 2) for r in ref)
    assert abs(float(l1.detach()) - float(w1.detach())) <= LOSS_TOL * abs(float(w1.detach()))


def test_lsgan_loss_refusals():
    x = torch.randn(3, 1, 2, 2, device=DEV)
    with pytest.raises(RuntimeError, match="float32"):
        ops.lsgan_loss([x.double()], [0.0])
    with pytest.raises(RuntimeError, match="batch"):
        ops.lsgan_loss([x], [(0.0, 1.0)])
    y = torch.randn(2, 1, 2, 2, device=DEV)
    with pytest.raises(RuntimeError, match="8 segments"):
        ops.lsgan_loss([y] * 5, [(0.0, 1.0)] * 5)
    with pytest.raises(RuntimeError, match="8 segments"):
        ops.lsgan_loss([y] * 9, [0.0] * 9)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.lsgan_loss([y.cpu()], [0.0])


# ---- MsImageDis.calc_dis_loss_sr / calc_gen_loss_sr -------------------------------------------------------------------------
def _module(hp, tag):
    from munit_amd.networks import MsImageDis
    net = MsImageDis(hp["input_dim_a"], hp["dis"])
    sd = D.make_state(hp, tag)
    D.load_into(net, sd)
    for p in sd.values():
        p.requires_grad_(True)
    return net.to(DEV), sd


@pytest.mark.parametrize("batches", [(1, 1), (2, 2), (3, 3), (2, 1)])
def test_losses_against_the_oracle(batches):
    """(sim batch, real batch): equal batches take the one-forward path (batch 1: the n = 1 segment and the odd start of
    the second half at the 1x1 scale), unequal ones the two-forward path."""
    ops.set_compute("f32")
    hp = O.default_hp(64, 2, 1)
    net, sd = _module(hp, "ocls_a.")
    names = [n for n, _ in net.named_parameters()]
    assert names == list(sd)
    ps = list(net.parameters())
    bs, br = batches
    sim, real = D.images(bs, 3, 64, 61), D.images(br, 3, 64, 62)

    def hip_dis():
        xs = [ops.nhwc(t.float().to(DEV)).requires_grad_(True) for t in (sim, real)]
        loss = net.calc_dis_loss_sr(xs[0], xs[1])
        return loss, torch.autograd.grad(loss, xs + ps)

    with Calls(("munit_lsgan_fwd", "munit_lsgan_bwd", "munit_mse_const")) as calls:
        (loss, grads), km, _ = record(hip_dis)
    assert calls == ["munit_lsgan_fwd", "munit_lsgan_bwd"]
    rs = [sim.clone().requires_grad_(True), real.clone().requires_grad_(True)]
    with pinned(km, "calc_dis_loss_sr"):
        l_ref = D.dis_loss_sr(sd, rs[0], rs[1], hp["dis"])
    g_ref = torch.autograd.grad(l_ref, rs + list(sd.values()))
    rel = abs(float(loss.detach()) - float(l_ref.detach())) / abs(float(l_ref.detach()))
    errs = [nerr(g, r) for g, r in zip(grads, g_ref)]
    print("calc_dis_loss_sr %s: loss %.6f rel %.2e, d sim %.2e d real %.2e worst weight grad %.2e"
          % (batches, float(l_ref.detach()), rel, errs[0], errs[1], max(errs[2:])))
    assert rel <= LOSS_TOL and max(errs) <= GRAD_TOL, (rel, dict(zip(["sim", "real"] + names, errs)))

    def hip_gen():
        x = ops.nhwc(sim.float().to(DEV)).requires_grad_(True)
        loss = net.calc_gen_loss_sr(x)
        return loss, torch.autograd.grad(loss, [x] + ps)

    (loss, grads), km, _ = record(hip_gen)
    r = sim.clone().requires_grad_(True)
    with pinned(km, "calc_gen_loss_sr"):
        l_ref = D.gen_loss_sr(sd, r, hp["dis"])
    g_ref = torch.autograd.grad(l_ref, [r] + list(sd.values()))
    rel = abs(float(loss.detach()) - float(l_ref.detach())) / abs(float(l_ref.detach()))
    errs = [nerr(g, q) for g, q in zip(grads, g_ref)]
    print("calc_gen_loss_sr B=%d: loss %.6f rel %.2e, d image %.2e worst weight grad %.2e"
          % (bs, float(l_ref.detach()), rel, errs[0], max(errs[1:])))
    assert rel <= LOSS_TOL and max(errs) <= GRAD_TOL, (rel, dict(zip(["image"] + names, errs)))


# ---- the trainer ------------------------------------------------------------------------------------------------------------
def _hp(**over):
    hp = O.default_hp(64, 2, 1)
    hp["gen"]["n_res"] = 1
    hp["adaptation"].update(ON)
    for k, v in over.items():
        if isinstance(v, dict):
            hp[k] = dict(hp[k], **v)
        else:
            hp[k] = v
    return hp


def _trainer(hp, seed=0):
    from munit_amd.trainer import MUNIT_Trainer
    torch.manual_seed(seed)
    return MUNIT_Trainer(dict(hp)).to(DEV)


def _batch(seed=7):
    return [t.to(DEV) for t in O.synthetic_batch(2, 64, seed=seed)]


def _styles(hp, seed):
    torch.manual_seed(seed)
    return (torch.randn(2, hp["gen"]["style_dim"], 1, 1).double(), torch.randn(2, hp["gen"]["style_dim"], 1, 1).double())


def _sequence(hp, synth=False):
    """dis_update, gen_update (term on), output_domain_classifier_sr_update, twice over: every loss and every weight of the
    generator, the discriminators and the classifiers after each call against the fp64 oracle.  Before a call the oracle
    takes over the HIP trainer's weights (tests/parity.py: Adam's first steps are sign-like, so two runs otherwise drift);
    its Adam moments and step counts carry over.  Parameters whose true gradient is identically zero (a bias ahead of an
    instance norm) hold rounding noise that Adam turns into +-lr steps on both sides: not compared, as in tests/parity.py."""
    from munit_amd.trainer import MUNIT_Trainer
    from tests import synth_oracle as Y
    base = Y.oracle_trainer_class(None, lambda: [], None) if synth else None
    gen, dis_a, dis_b = oracle_states(hp, torch.float64)
    cls_a, cls_b = D.make_state(hp, "ocls_a."), D.make_state(hp, "ocls_b.")
    orc = D.oracle_trainer_class(base)(hp, gen, dis_a, dis_b).attach(cls_a, cls_b)
    tr = MUNIT_Trainer(dict(hp))
    load_into_trainer(tr, gen, dis_a, dis_b)
    D.load_into(tr.output_classifier_sr_a, cls_a)
    D.load_into(tr.output_classifier_sr_b, cls_b)
    tr.to(DEV)
    if synth:
        x_a, x_b = (t.to(DEV) for t in Y.pair_inputs(2, 64, 7, dtype=torch.float32)[:2])
        _, _, m_a, m_b = _batch()
    else:
        x_a, x_b, m_a, m_b = _batch()
    x_as, x_bs = _batch(seed=8)[:2]
    ox = {k: v.double().cpu() for k, v in dict(x_a=x_a, x_b=x_b, m_a=m_a, m_b=m_b, x_as=x_as, x_bs=x_bs).items()}
    gnames, dnames = trainer_named_params(tr)
    cnames = [("a." + k, p) for k, p in tr.output_classifier_sr_a.named_parameters()] + \
             [("b." + k, p) for k, p in tr.output_classifier_sr_b.named_parameters()]
    groups = (("gen", gnames, orc.opt["gen"]["params"]), ("dis", dnames, orc.opt["dis"]["params"]),
              ("cls", cnames, orc.cls_opt.params))
    null, lr, worst = set(), hp["lr"], dict(loss=0.0, weight_abs=0.0, weight_l2=0.0, moment_l2=0.0, kink=0.0)

    def sync():
        with torch.no_grad():
            for _, names, params in groups:
                for (n, p), q in zip(names, params):
                    q.copy_(p.detach().double().cpu())

    def compare(what, losses, new=()):
        for k in losses:
            mine, v = float(getattr(tr, k)), float(orc.losses[k])
            rel = abs(mine - v) / (abs(v) if k in new else max(1.0, abs(v)))
            worst["loss"] = max(worst["loss"], rel)
            assert rel <= LOSS_TOL, (what, k, mine, v, rel)
        for grp, names, params in groups:
            for (n, p), q in zip(names, params):
                if grp + "." + n in null:
                    continue
                a, r = p.detach().double().cpu(), q.detach()
                worst["weight_abs"] = max(worst["weight_abs"], float((a - r).abs().max()))
                worst["weight_l2"] = max(worst["weight_l2"], l2err(a, r))
                assert float((a - r).abs().max()) <= 4.0 * lr and l2err(a, r) <= 2e-4, (what, grp, n, worst)

    def run(what, seed, hip, oracle):
        km = record(hip, seed)[1]
        with pinned(km, what) as audit:
            out = oracle()
        worst["kink"] = max(worst["kink"], audit.worst_rel)
        return out

    sd_on = hp["adaptation"]["output_adv_lambda"]
    for it in (0, 1):
        tr.iterations = orc.iterations = it
        tr.update_learning_rate()
        orc.update_learning_rate()
        sync()
        sa, sb = _styles(hp, 100 + it)
        run("dis", 100 + it, lambda: tr.dis_update(x_a, x_b, hp), lambda: orc.dis_update(ox["x_a"], ox["x_b"], sa, sb))
        compare("dis_update %d" % it, ("loss_dis_a", "loss_dis_b", "loss_dis_total"))
        sync()
        sa, sb = _styles(hp, 200 + it)
        g_ref = run("gen", 200 + it, lambda: tr.gen_update(x_a, x_b, hp, m_a, m_b, synth=synth),
                    lambda: orc.gen_update(ox["x_a"], ox["x_b"], ox["m_a"], ox["m_b"], sa, sb))
        for (n, _), g in zip(gnames, g_ref):
            if g is None or float(g.abs().max()) < 1e-7:
                null.add("gen." + n)
        assert sd_on > 0 and float(tr.loss_output_classifier_sr) > 0
        names = [k for k in orc.losses if k.startswith("loss_gen") or k == "loss_output_classifier_sr"]
        assert "loss_output_classifier_sr" in names and (not synth or "loss_gen_recon_synth" in names)
        compare("gen_update %d" % it, names, new=("loss_output_classifier_sr",))
        sync()
        run("cls", 300 + it, lambda: tr.output_domain_classifier_sr_update(x_a, x_as, x_b, x_bs, hp, it),
            lambda: orc.output_domain_classifier_sr_update(ox["x_a"], ox["x_as"], ox["x_b"], ox["x_bs"]))
        compare("classifier update %d" % it, ("loss_output_classifier_sr_update",), new=("loss_output_classifier_sr_update",))
        for (mv, vv), om, ov in zip(tr.output_classif_opt_sr._views, orc.cls_opt.m, orc.cls_opt.v):
            worst["moment_l2"] = max(worst["moment_l2"], l2err(mv, om), l2err(vv, ov))
        assert worst["moment_l2"] <= 2 * GRAD_TOL, worst
    assert tr.output_classif_opt_sr._step == orc.cls_opt.step_count == 2
    assert tr.gen_opt._step == orc.opt["gen"]["step"] == 2 and tr.dis_opt._step == orc.opt["dis"]["step"] == 2
    print("sequence %s synth=%s: %s, %d parameters with a zero gradient" % (
        {k: hp[k] for k in ("gen_state", "guided")}, synth, {k: "%.2e" % v for k, v in worst.items()}, len(null)))


def test_the_sequence_of_updates_against_the_oracle():
    _sequence(_hp(adaptation=dict(output_classifier_lambda=2, output_adv_lambda=1.5)))


def test_the_sequence_with_separate_generators_and_sampled_styles():
    _sequence(_hp(gen_state=0, guided=0))


def test_the_sequence_with_the_synthetic_pair_step():
    _sequence(_hp(recon_synth_w=1), synth=True)


def test_gen_update_forms_no_discriminator_or_classifier_weight_gradient():
    hp = _hp()
    tr = _trainer(hp)
    x_a, x_b, m_a, m_b = _batch()
    tr.output_classif_opt_sr.flat_g.fill_(3.0)
    tr.dis_opt.flat_g.fill_(5.0)
    tr.gen_update(x_a, x_b, hp, m_a, m_b)
    torch.cuda.synchronize()
    assert bool((tr.output_classif_opt_sr.flat_g == 3.0).all()) and bool((tr.dis_opt.flat_g == 5.0).all())
    assert all(p.requires_grad for p in tr.output_classifier_sr_a.parameters())
    assert float(tr.loss_output_classifier_sr) > 0 and float(tr.gen_opt.flat_g.abs().max()) > 0


def test_multi_stream_updates_are_bitwise_the_single_stream_ones(monkeypatch):
    from munit_amd import trainer as T
    hp = _hp()
    x_a, x_b, m_a, m_b = _batch()
    x_as, x_bs = _batch(seed=8)[:2]
    res = []
    for streams in (True, False):
        monkeypatch.setattr(T, "BRANCH_STREAMS", streams)
        tr = _trainer(hp)
        tr.gen_update(x_a, x_b, hp, m_a, m_b)
        tr.output_domain_classifier_sr_update(x_a, x_as, x_b, x_bs, hp, 0)
        torch.cuda.synchronize()
        res.append((tr.gen_opt.flat_g.clone(), tr.loss_output_classifier_sr.clone(), tr.loss_gen_total.clone(),
                    tr.output_classif_opt_sr.flat_g.clone(), tr.output_classif_opt_sr.flat_p.clone(),
                    tr.loss_output_classifier_sr_update.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert float(res[0][0].abs().max()) > 0 and float(res[0][3].abs().max()) > 0


def test_the_term_on_the_reused_forward_matches_the_plain_step():
    """reuse_dis_forward: 1 -- the same losses as the plain step, the generator gradient within 5e-5."""
    x_a, x_b, m_a, m_b = _batch()
    res = []
    for reuse in (0, 1):
        hp = _hp(reuse_dis_forward=reuse)
        tr = _trainer(hp)
        tr.dis_update(x_a, x_b, hp)
        tr.gen_update(x_a, x_b, hp, m_a, m_b)
        torch.cuda.synchronize()
        assert tr.fwd_reused == bool(reuse)
        res.append((tr.gen_opt.flat_g.clone(), {n: float(getattr(tr, n).detach()) for n in vars(tr)
                                                if n.startswith("loss_") and torch.is_tensor(getattr(tr, n))}))
    assert "loss_output_classifier_sr" in res[0][1] and res[0][1] == res[1][1]
    assert nerr(res[1][0], res[0][0]) <= GRAD_TOL and l2err(res[1][0], res[0][0]) <= GRAD_TOL


def test_feature_off_launches_nothing_new_and_changes_nothing():
    x_a, x_b, m_a, m_b = _batch()
    off = _hp(adaptation=dict(output_classifier_lambda=0, output_adv_lambda=0))
    tr_off = _trainer(off)
    with Calls(NEW) as calls:
        tr_off.dis_update(x_a, x_b, off)
        torch.manual_seed(1)
        tr_off.gen_update(x_a, x_b, off, m_a, m_b)
        torch.cuda.synchronize()
    assert calls == [] and tr_off.loss_output_classifier_sr == 0
    # a trainer that owns the classifiers, handed output_adv_lambda 0 for the step: bitwise the trainer without them
    on = _hp()
    tr_on = _trainer(on)
    step = _hp(adaptation=dict(output_adv_lambda=0))
    tr_on.output_classif_opt_sr.flat_g.fill_(3.0)
    with Calls(NEW) as calls:
        tr_on.dis_update(x_a, x_b, step)
        torch.manual_seed(1)
        tr_on.gen_update(x_a, x_b, step, m_a, m_b)
        torch.cuda.synchronize()
    assert calls == [] and tr_on.loss_output_classifier_sr == 0
    assert torch.equal(tr_on.gen_opt.flat_g, tr_off.gen_opt.flat_g) and torch.equal(tr_on.gen_opt.flat_p, tr_off.gen_opt.flat_p)
    assert torch.equal(tr_on.loss_gen_total, tr_off.loss_gen_total) and torch.equal(tr_on.dis_opt.flat_p, tr_off.dis_opt.flat_p)
    assert bool((tr_on.output_classif_opt_sr.flat_g == 3.0).all())
    with Calls(NEW) as calls:
        tr_on.gen_update(x_a, x_b, on, m_a, m_b)
        torch.cuda.synchronize()
    assert calls.count("munit_lsgan_fwd") == calls.count("munit_lsgan_bwd") == 2      # one pair per classifier pass
