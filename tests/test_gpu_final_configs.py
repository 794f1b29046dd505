"""The configurations the reference trains (configs/Final_test/*.yaml, five classes: tests/final_configs.py) as whole
iterations in the order of scripts/train.py:182-274, driven through examples/train_loop.run_iteration.

Reductions (tests/final_configs.reduced_hp; everything else is the file's own -- weights, batch, ratio_disc_gen,
synthetic_frequency, synthetic_seg_gt):
    crop 64 x 64 for Baseline and Output_DA (the smallest multiple of 32 at which all three discriminator scales still have an
    output), 256 x 256 for FeatureDA (the smallest crop domainClassifier.check_code_hw and _check_semantic both admit at
    n_downsample 2); gen.n_res 1; dis.num_scales 3 at 64 and 1 at 256; classif_frequency and output_classif_freq 2;
    3 iterations for Baseline (the real gen_update happens once, after two skipped ones), 2 for the others (each classifier
    update happens once, on it = 1).  The segmentation network is semantic_oracle.make_model saved under tmp_path; the real pair
    is O.synthetic_batch, the synthetic one synth_oracle.pair_inputs / gt_maps with one 0 / 1 mask.

a. Against the composed fp64 oracle (final_configs.composed_oracle_class), in the scheme of test_gpu_outda._sequence: before
   each call the oracle takes over the HIP weights (its Adam moments and step counts carry over); after it every loss the call
   sets, every weight of the generator, the discriminators and the classifiers, the classifiers' Adam moments and BatchNorm
   statistics; at the first gen_update of each kind every generator gradient.  Bounds: the project's own, imported.
b. What the run leaves behind: sinks, the kept forward, a pending discriminator step, requires_grad, save / resume.
c. BRANCH_STREAMS True against False, and True twice: every optimizer's flat_p / flat_g and every loss bit for bit.

Wall time of one parametrisation of test_iterations_against_the_composed_oracle, nearly all of it the fp64 oracle on the host
(MI355X machine, 16 CPUs): Baseline 13.8 s, Output_DA 14.3 s, Output_DA+seg 13.9 s, FeatureDA 77.3 s,
FeatureDA+seg 88.9 s -- each below test_gpu_featda.py::test_step_parity_with_the_fooling_term in the same run (139.1 s), so
every iteration is compared against the oracle.  test_stream_modes_are_bitwise_equal: 1.2 .. 2.4 s each.  Worst errors
measured there: losses 7.2e-7 relative, weights 2.0 lr absolute and 8.9e-5 relative L2, classifier moments 4.6e-6, generator
gradients 1.3e-5 at 64 x 64 and 4.9e-5 max / 3.7e-5 L2 at 256 x 256, pinned kinks 2.5e-6, BatchNorm statistics 2.2e-7."""
import os
import sys
import time

import pytest
import torch

from munit_amd import ops
from tests import featda_oracle as F
from tests import final_configs as C
from tests import outda_oracle as D
from tests import semantic_oracle as S
from tests.parity import KINK_NOISE, l2err, load_into_trainer, nerr, oracle_states, pinned, record, trainer_named_params
from tests.test_gpu_featda import FWD_TOL, GRAD_TOL, LOSS_TOL

sys.path.insert(0, os.path.join(C.ROOT, "examples"))
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = sorted(C.CLASSES)
SINKS = ("MASK_SINK", "L1_SINK", "SEG_SINK", "DANN_SINK")
NEW_LOSSES = ("loss_sem_seg", "loss_gen_recon_synth", "loss_classifier_sr", "loss_output_classifier_sr",
              "loss_classifier_sr_update", "loss_output_classifier_sr_update")


@pytest.fixture(scope="module")
def fx():
    return C.load()


@pytest.fixture(scope="module")
def seg_model():
    return S.make_model(0)


def _ckpt(tmp_path, model):
    p = tmp_path / "seg.pth"
    torch.save({k: v.cpu() for k, v in model.state_dict().items()}, str(p))
    return str(p)


def _cls_state(module):
    sd = {k: v.detach().cpu().double().clone() for k, v in module.state_dict().items()}
    return {k: (v.long() if k.endswith("tracked") else v) for k, v in sd.items()}


def _pairs(synth):
    while True:
        yield synth


def _losses(tr):
    return {n: getattr(tr, n).detach().clone() for n in sorted(vars(tr)) if n.startswith("loss_") and torch.is_tensor(getattr(tr, n))}


def _optimizers(tr):
    opts = {"gen": tr.gen_opt, "dis": tr.dis_opt}
    if tr.use_classifier_sr:
        opts["feat"] = tr.classif_opt_sr
    if tr.use_output_classifier_sr:
        opts["out"] = tr.output_classif_opt_sr
    return opts


@pytest.mark.parametrize("name", NAMES)
def test_iterations_against_the_composed_oracle(fx, seg_model, tmp_path, name):
    from munit_amd.trainer import MUNIT_Trainer
    from train_loop import run_iteration
    t0 = time.perf_counter()
    hp = C.reduced_hp(fx, name, _ckpt(tmp_path, seg_model))
    ad, lr, iters = hp["adaptation"], hp["lr"], C.ITERATIONS[name]
    real, synth = C.inputs(hp)
    dreal = tuple(t.to(DEV) for t in real)
    dsynth = tuple(t.to(DEV) for t in synth[:3]) + synth[3:]          # the label maps stay on the host, as the reference's do
    oreal, osynth = tuple(t.double() for t in real), tuple(t.double() for t in synth)
    gen, dis_a, dis_b = oracle_states(hp, torch.float64)
    shared, seg_sink = {"sink": []}, [[]]
    orc = C.composed_oracle_class(hp, seg_model, lambda: seg_sink[0], (osynth[3], osynth[4]), shared)(hp, gen, dis_a, dis_b)
    tr = MUNIT_Trainer(dict(hp))
    load_into_trainer(tr, gen, dis_a, dis_b)
    gnames, dnames = trainer_named_params(tr)
    groups = [("gen", gnames, orc.opt["gen"]["params"]), ("dis", dnames, orc.opt["dis"]["params"])]
    feat = out = None
    if tr.use_output_classifier_sr:
        cls = D.make_state(hp, "ocls_a."), D.make_state(hp, "ocls_b.")
        orc.attach(*cls)
        D.load_into(tr.output_classifier_sr_a, cls[0])
        D.load_into(tr.output_classifier_sr_b, cls[1])
        out = [("a." + k, p) for k, p in tr.output_classifier_sr_a.named_parameters()] + \
              [("b." + k, p) for k, p in tr.output_classifier_sr_b.named_parameters()]
        groups.append(("out", out, orc.cls_opt.params))
    if tr.use_classifier_sr:
        sd_a, sd_b = F.make_state(31), F.make_state(32)
        F.load_into(tr.domain_classifier_sr_a, sd_a)
        F.load_into(tr.domain_classifier_sr_b, sd_b)
        shared["sd"] = (sd_a, sd_b)
        fopt = F.ClassifierOptimizer(sd_a, sd_b, hp)
        feat = [("a." + k, p) for k, p in tr.domain_classifier_sr_a.named_parameters()] + \
               [("b." + k, p) for k, p in tr.domain_classifier_sr_b.named_parameters()]
        assert [n for n, _ in feat] == ["a." + k for k in F.param_names()] + ["b." + k for k in F.param_names()]
        groups.append(("feat", feat, fopt.params))
    tr.to(DEV)
    null = set()
    worst = dict(loss=0.0, weight_abs=0.0, weight_l2=0.0, moment_l2=0.0, grad_max=0.0, grad_l2=0.0, kink=0.0, kink_frac=0.0,
                 stat=0.0)
    graded, n_calls, seed = set(), {}, [0]

    def sync():
        with torch.no_grad():
            for _, names, params in groups:
                for (n, p), q in zip(names, params):
                    q.copy_(p.detach().double().cpu())
            if feat is not None:          # the BatchNorm statistics as well
                for net, sd in ((tr.domain_classifier_sr_a, sd_a), (tr.domain_classifier_sr_b, sd_b)):
                    for k, v in _cls_state(net).items():
                        if not F.is_param(k):
                            sd[k].copy_(v)

    def compare(what, names):
        for k in names:
            mine, v = float(getattr(tr, k).detach()), float(orc.losses[k])
            rel = abs(mine - v) / (abs(v) if k in NEW_LOSSES else max(1.0, abs(v)))
            print("  %-28s %-34s %.8g  oracle %.8g  rel %.2e" % (what, k, mine, v, rel))
            worst["loss"] = max(worst["loss"], rel)
            assert rel <= LOSS_TOL, (what, k, mine, v, rel)
        for grp, pnames, params in groups:
            for (n, p), q in zip(pnames, params):
                if grp == "gen" and n in null:
                    continue
                a, r = p.detach().double().cpu(), q.detach()
                worst["weight_abs"] = max(worst["weight_abs"], float((a - r).abs().max()))
                worst["weight_l2"] = max(worst["weight_l2"], l2err(a, r))
                assert float((a - r).abs().max()) <= 4.0 * lr and l2err(a, r) <= 2e-4, (what, grp, n, worst)
        if feat is not None:
            for net, sd in ((tr.domain_classifier_sr_a, sd_a), (tr.domain_classifier_sr_b, sd_b)):
                own = net.state_dict()
                for k, v in sd.items():
                    if k.endswith("tracked"):
                        assert int(own[k]) == int(v), (what, k)
                    elif not F.is_param(k):
                        worst["stat"] = max(worst["stat"], nerr(own[k], v))
                        assert nerr(own[k], v) <= FWD_TOL, (what, k, nerr(own[k], v))

    def moments(what, opt, ms, vs):
        for (mv, vv), om, ov in zip(opt._views, ms, vs):
            worst["moment_l2"] = max(worst["moment_l2"], l2err(mv, om), l2err(vv, ov))
        assert worst["moment_l2"] <= 2 * GRAD_TOL, (what, worst)

    def styles(b):
        return (torch.randn(b, hp["gen"]["style_dim"], 1, 1).double(), torch.randn(b, hp["gen"]["style_dim"], 1, 1).double())

    def on_call(method, args, run):
        n_calls[method] = n_calls.get(method, 0) + 1
        seed[0] += 1
        is_synth = args[0] is dsynth[0]
        what = "it %d %s(%s)" % (tr.iterations, method, "synth" if is_synth else "real")
        ox = osynth if is_synth else oreal
        orc.iterations, orc.losses = tr.iterations, {}
        sync()
        for s in SINKS:
            assert getattr(ops, s) is None, s
        _, km, k = record(run, seed[0], seg=True, dann=True)
        seg_sink[0], shared["sink"] = k.seg, k.dann
        torch.manual_seed(seed[0])
        sa, sb = styles(hp["batch_size"])
        # the classifier's own update pins through `pins`: its encoders run without a tape, their codes are values, not kinks
        with pinned(None if method == "domain_classifier_sr_update" else km, what) as audit:
            if method == "dis_update":
                assert not seg_sink[0] and not shared["sink"]
                orc.dis_update(ox[0], ox[1], sa, sb)
                names = ("loss_dis_a", "loss_dis_b", "loss_dis_total")
            elif method == "gen_update":
                orc.synth_call = is_synth
                m_a, m_b = (ox[2], ox[2]) if is_synth else (ox[2], ox[3])
                type(orc).audit_bad = None
                g_ref = orc.gen_update(ox[0], ox[1], m_a, m_b, sa, sb)
                assert type(orc).audit_bad == 0, (what, type(orc).audit_bad)      # the segmentation network's kinks and labels
                if feat is not None:
                    assert shared["worst"] <= KINK_NOISE, (what, shared["worst"])
                    worst["kink"] = max(worst["kink"], shared["worst"])
                else:
                    assert not shared["sink"]
                for (n, p), g in zip(gnames, g_ref):
                    if g is None or float(g.abs().max()) < 1e-7:
                        null.add(n)
                        continue
                    if is_synth not in graded:       # the first gen_update of this kind: every generator gradient
                        e, l2 = nerr(p._munit_grad, g), l2err(p._munit_grad, g)
                        worst["grad_max"], worst["grad_l2"] = max(worst["grad_max"], e), max(worst["grad_l2"], l2)
                        assert e <= GRAD_TOL and l2 <= GRAD_TOL, (what, n, e, l2)
                graded.add(is_synth)
                names = sorted(orc.losses)
                assert "loss_sem_seg" in names and float(tr.loss_sem_seg) > 0
                assert ("loss_gen_recon_synth" in names) == (is_synth and hp["recon_synth_w"] > 0)
                assert ("loss_classifier_sr" in names) == (ad["adv_lambda"] > 0)
                assert ("loss_output_classifier_sr" in names) == (ad["output_adv_lambda"] > 0)
                for k in ("loss_gen_recon_synth", "loss_classifier_sr", "loss_output_classifier_sr"):
                    if k not in names:
                        assert float(getattr(tr, k)) == 0, (what, k)
            elif method == "domain_classifier_sr_update":
                assert not seg_sink[0] and args[2] == is_synth
                pins = F.trainer_pins(shared["sink"])
                (ga, ka), (gb, kb) = orc._views()
                with torch.no_grad():
                    c_a, c_b = ga.encode(ox[0], ka)[0], gb.encode(ox[1], kb)[0]
                orc.losses["loss_classifier_sr_update"] = F.classifier_update(sd_a, sd_b, fopt, c_a, c_b, args[2], args[3],
                                                                              tr.iterations, pins=pins)
                assert pins.done() and pins.worst <= KINK_NOISE, (what, pins.worst)
                worst["kink"] = max(worst["kink"], pins.worst)
                names = ("loss_classifier_sr_update",)
            else:
                assert method == "output_domain_classifier_sr_update" and not seg_sink[0] and not shared["sink"]
                assert args[1] is dsynth[0] and args[3] is dsynth[1]
                orc.output_domain_classifier_sr_update(oreal[0], osynth[0], oreal[1], osynth[1])
                names = ("loss_output_classifier_sr_update",)
        worst["kink"], worst["kink_frac"] = max(worst["kink"], audit.worst_rel), max(worst["kink_frac"], audit.disagree_frac)
        compare(what, names)
        if method == "domain_classifier_sr_update":
            moments(what, tr.classif_opt_sr, fopt.m, fopt.v)
        if method == "output_domain_classifier_sr_update":
            moments(what, tr.output_classif_opt_sr, orc.cls_opt.m, orc.cls_opt.v)

    pairs = _pairs(dsynth)
    for it in range(iters):
        orc.sched_steps += 1                         # update_learning_rate, which run_iteration calls on the HIP side
        run_iteration(tr, hp, it, dreal, pairs, on_call)
        assert abs(tr.gen_opt.param_groups[0]["lr"] - orc._lr()) < 1e-15
    torch.cuda.synchronize()

    # the parameters left out: a bias ahead of an instance norm / AdaIN, all of them and nothing else
    assert all(C.NULL_PATTERN.match(n) for n in null), sorted(n for n in null if not C.NULL_PATTERN.match(n))
    assert len(null) == C.null_count(hp) == len([n for n, _ in gnames if C.NULL_PATTERN.match(n)]), (len(null), C.null_count(hp))
    # optimizer steps: both sides, and the number the hand-written order of calls predicts
    want = {m: C.count_calls(name, iters, m) for m in ("dis_update", "gen_update", "domain_classifier_sr_update",
                                                        "output_domain_classifier_sr_update")}
    assert {m: n_calls.get(m, 0) for m in want} == want
    assert graded == {False, True}
    assert tr.dis_opt._step == orc.opt["dis"]["step"] == want["dis_update"]
    assert tr.gen_opt._step == orc.opt["gen"]["step"] == want["gen_update"]
    if feat is not None:
        assert tr.classif_opt_sr._step == fopt.step_count == want["domain_classifier_sr_update"] == 2
    if out is not None:
        assert tr.output_classif_opt_sr._step == orc.cls_opt.step_count == want["output_domain_classifier_sr_update"] == 1
    t_oracle = time.perf_counter() - t0
    print("final config %s (%d iterations, crop %d, batch %d): %s, %d parameters with a zero gradient, %.1f s"
          % (name, iters, hp["crop_image_height"], hp["batch_size"], {k: "%.2e" % v for k, v in worst.items()}, len(null),
             t_oracle))

    # ---- b. what the run leaves behind -----------------------------------------------------------------------------------
    for s in SINKS:
        assert getattr(ops, s) is None, s
    assert tr._fwd_cache is None
    tr.dis_opt.settle()
    assert tr.dis_opt.gate.pending is None and tr.dis_opt.gate.waited == set()
    owned = [tr.gen, tr.dis_a, tr.dis_b]
    owned += [tr.domain_classifier_sr_a, tr.domain_classifier_sr_b] if feat is not None else []
    owned += [tr.output_classifier_sr_a, tr.output_classifier_sr_b] if out is not None else []
    for m in owned:
        assert all(p.requires_grad for p in m.parameters())
    tr.save(str(tmp_path), iters - 1)
    torch.manual_seed(99)
    tr2 = MUNIT_Trainer(dict(hp)).to(DEV)
    assert tr2.resume(str(tmp_path), hp) == iters
    res = []
    for t in (tr, tr2):
        torch.manual_seed(5)
        t.dis_update(dreal[0], dreal[1], hp)
        torch.cuda.synchronize()
        res.append((t.loss_dis_a.clone(), t.loss_dis_b.clone(), t.loss_dis_total.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b), (float(a), float(b))
    assert float(res[0][2]) > 0


def _plain_run(hp, name, streams, monkeypatch):
    from munit_amd import trainer as T
    from train_loop import run_iteration
    monkeypatch.setattr(T, "BRANCH_STREAMS", streams)
    real, synth = C.inputs(hp)
    dreal = tuple(t.to(DEV) for t in real)
    dsynth = tuple(t.to(DEV) for t in synth[:3]) + synth[3:]
    torch.manual_seed(0)
    tr = T.MUNIT_Trainer(dict(hp)).to(DEV)
    pairs = _pairs(dsynth)
    for it in range(C.ITERATIONS[name]):
        run_iteration(tr, hp, it, dreal, pairs)
    torch.cuda.synchronize()
    state = {}
    for k, opt in _optimizers(tr).items():
        state[k + ".flat_p"], state[k + ".flat_g"] = opt.flat_p.clone(), opt.flat_g.clone()
    state.update(_losses(tr))
    return state


@pytest.mark.parametrize("name", NAMES)
def test_stream_modes_are_bitwise_equal(fx, seg_model, tmp_path, monkeypatch, name):
    """The same iterations without the oracle on fresh trainers with the same seeds: branch streams on, off, and on again."""
    hp = C.reduced_hp(fx, name, _ckpt(tmp_path, seg_model))
    multi, single, again = (_plain_run(hp, name, s, monkeypatch) for s in (True, False, True))
    want = {"gen.flat_p", "gen.flat_g", "dis.flat_p", "dis.flat_g", "loss_gen_total", "loss_dis_total", "loss_sem_seg"}
    if name.startswith("FeatureDA"):
        want |= {"feat.flat_p", "feat.flat_g", "loss_classifier_sr", "loss_classifier_sr_update"}
    if name.startswith("Output_DA"):
        want |= {"out.flat_p", "out.flat_g", "loss_output_classifier_sr", "loss_output_classifier_sr_update"}
    assert want <= set(multi) and sorted(multi) == sorted(single) == sorted(again)
    for k in multi:
        assert torch.equal(multi[k], single[k]), ("streams on / off", k)
        assert torch.equal(multi[k], again[k]), ("streams on, twice", k)
    assert float(multi["gen.flat_g"].abs().max()) > 0 and float(multi["dis.flat_g"].abs().max()) > 0
