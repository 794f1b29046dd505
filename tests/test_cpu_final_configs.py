"""Host-side checks of the configurations the reference trains (configs/Final_test/*.yaml): the fixture and its classes, the
trainer's acceptance of each class, the order of calls of examples/train_loop.run_iteration against a list written out by hand
from scripts/train.py:182-274, and the composition of loss_gen_total by the stacked fp64 oracles (tests/final_configs.py)."""
import os
import sys

import pytest
import torch

from oracle import munit_oracle as O
from tests import featda_oracle as F
from tests import final_configs as C
from tests import outda_oracle as D
from tests import semantic_oracle as S
from tests import synth_oracle as Y
from tests.parity import oracle_states

sys.path.insert(0, os.path.join(C.ROOT, "examples"))
NAMES = sorted(C.CLASSES)


@pytest.fixture(scope="module")
def fx():
    return C.load()


# ---- the fixture ---------------------------------------------------------------------------------------------------------
def test_fixture_falls_into_the_five_classes(fx):
    assert sorted(fx) == sorted(f for files in C.CLASSES.values() for f in files) and len(fx) == 7
    strip = lambda cfg: {k: v for k, v in cfg.items() if k not in C.IGNORED}
    for name, files in C.CLASSES.items():
        for f in files[1:]:
            assert fx[f] == fx[files[0]], (name, f)             # inside a class the settings are the same, num_workers included
    reps = [strip(fx[files[0]]) for files in C.CLASSES.values()]
    for i in range(len(reps)):
        for j in range(i):
            assert reps[i] != reps[j]                            # and no two classes are the same
    for cfg in fx.values():                                      # what every file has
        assert (cfg["semantic_w"], cfg["recon_mask"], cfg["synthetic_seg_gt"], cfg["synthetic_frequency"]) == (4, 1, 1, 1)
        assert (cfg["crop_image_height"], cfg["crop_image_width"], cfg["gen"]["n_downsample"]) == (256, 256, 2)
        assert (cfg["gen_state"], cfg["guided"], cfg["vgg_w"], cfg["domain_adv_w"]) == (1, 1, 0, 0)
        assert "optimizer" not in cfg and cfg["adaptation"]["sem_seg_lambda"] == 0
    ad = lambda n, k: fx[n]["adaptation"][k]
    feat = [n for n in fx if ad(n, "adv_lambda") > 0]
    assert sorted(feat) == ["FeatureDA", "FeatureDA+height30_seg", "FeatureDA+seg"]
    assert all((ad(n, "adv_lambda"), ad(n, "dfeat_lambda"), fx[n]["batch_size"]) == (6, 1, 1) for n in feat)
    out = [n for n in fx if ad(n, "output_adv_lambda") > 0]
    assert sorted(out) == ["Output_DA", "Output_DA+seg"]
    assert all((ad(n, "output_adv_lambda"), ad(n, "output_classifier_lambda"), fx[n]["batch_size"]) == (1, 1, 2) for n in out)
    assert sorted(n for n in fx if fx[n]["ratio_disc_gen"] == 3) == ["Baseline", "Baseline+seg"]
    assert all(fx[n]["ratio_disc_gen"] == 1 for n in feat + out)
    assert sorted(n for n in fx if fx[n]["recon_synth_w"] == 0) == ["FeatureDA+height30_seg", "FeatureDA+seg", "Output_DA+seg"]
    assert all(fx[n]["recon_synth_w"] in (0, 1) for n in fx)


def test_fixture_keeps_settings_only(fx):
    from tests.golden.make_golden_final_configs import dropped

    def leaves(v):
        if isinstance(v, dict):
            for x in v.values():
                yield from leaves(x)
        else:
            yield v

    for name, cfg in fx.items():
        assert not any(dropped(k) for k in cfg), name
        for v in leaves(cfg):
            assert isinstance(v, (int, float, str)) and not isinstance(v, (bool, list)), (name, v)
            assert not (isinstance(v, str) and ("/" in v or "." in v)), (name, v)


# ---- acceptance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_class_is_accepted(fx, name):
    """At the file's own crop of 256 with a dummy semantic_ckpt_path, the four checks of the trainer's constructor and of its
    gen_update refuse nothing."""
    from munit_amd.trainer import MUNIT_Trainer as T
    from munit_amd.utils import normalize_config
    hp = normalize_config(C.class_config(fx, name))
    hp["semantic_ckpt_path"] = "dummy.pth"
    assert hp["crop_image_height"] == 256 and hp["optimizer"] == "adam"
    ad = hp["adaptation"]
    T._check_aux(hp)
    T._check_aux(hp, construct=False)
    T._check_featda(hp, ad["dfeat_lambda"] > 0)
    T._check_outda(hp, ad["output_classifier_lambda"] > 0)
    T._check_outda(hp, ad["output_classifier_lambda"] > 0, update=ad["output_classifier_lambda"] > 0)
    T._check_semantic(hp)
    # the reductions of the GPU test are accepted as well
    red = normalize_config(C.reduced_hp(fx, name, "dummy.pth"))
    T._check_aux(red)
    T._check_featda(red, ad["dfeat_lambda"] > 0)
    T._check_outda(red, ad["output_classifier_lambda"] > 0)
    T._check_semantic(red)
    assert red["batch_size"] == hp["batch_size"] and red["ratio_disc_gen"] == hp["ratio_disc_gen"]
    assert red["synthetic_frequency"] == hp["synthetic_frequency"] == 1


# ---- the cadence -----------------------------------------------------------------------------------------------------------
class _Stub(object):
    """A trainer that records its calls: (method, batch, ...) in the form of tests/final_configs.CADENCE"""

    def __init__(self, cfg, real, synth):
        ad = cfg["adaptation"]
        self.use_classifier_sr = ad["dfeat_lambda"] > 0
        self.use_output_classifier_sr = ad["output_classifier_lambda"] > 0
        self.cfg, self.real, self.synth, self.calls, self.lr_at, self.iterations = cfg, real, synth, [], [], None

    def _which(self, x_a, x_b):
        if x_a is self.real[0] and x_b is self.real[1]:
            return "real"
        assert x_a is self.synth[0] and x_b is self.synth[1]
        return "synth"

    def update_learning_rate(self):
        assert not self.calls or self.calls[-1] != "lr"
        self.lr_at.append((self.iterations, len(self.calls)))

    def dis_update(self, x_a, x_b, hp, comet_exp=None):
        assert hp is self.cfg
        self.calls.append(("dis_update", self._which(x_a, x_b)))

    def gen_update(self, x_a, x_b, hp, mask_a=None, mask_b=None, comet_exp=None, synth=False, semantic_gt_a=None,
                   semantic_gt_b=None):
        which = self._which(x_a, x_b)
        assert hp is self.cfg and comet_exp is None
        if which == "real":
            assert mask_a is self.real[2] and mask_b is self.real[3]
        else:
            assert mask_a is self.synth[2] and mask_b is self.synth[2]       # the same mask for both images of the pair
        gt = semantic_gt_a is not None
        assert gt == (semantic_gt_b is not None)
        if gt:
            assert semantic_gt_a is self.synth[3] and semantic_gt_b is self.synth[4]
        self.calls.append(("gen_update", which, synth, gt))

    def domain_classifier_sr_update(self, x_a, x_b, domain_synth, lambda_classifier, step, comet_exp=None):
        assert lambda_classifier == self.cfg["adaptation"]["dfeat_lambda"]
        self.calls.append(("domain_classifier_sr_update", self._which(x_a, x_b), domain_synth, step))

    def output_domain_classifier_sr_update(self, x_ar, x_as, x_br, x_bs, hp, step, comet_exp=None):
        assert hp is self.cfg
        assert x_ar is self.real[0] and x_br is self.real[1] and x_as is self.synth[0] and x_bs is self.synth[1]
        self.calls.append(("output_domain_classifier_sr_update", "real+synth", step))


def _drive(cfg, iterations=6, use_hook=False):
    from train_loop import run_iteration
    real = tuple(torch.zeros(1) for _ in range(4))
    synth = tuple(torch.zeros(1) for _ in range(5))
    stub, per_it, drawn, hooked = _Stub(cfg, real, synth), [], [0], []

    def pairs():
        while True:
            drawn[0] += 1
            yield synth

    def on_call(name, args, run):
        hooked.append(name)
        return run()

    it_pairs = pairs()
    for it in range(iterations):
        n = len(stub.calls)
        run_iteration(stub, cfg, it, real, it_pairs, on_call if use_hook else None)
        per_it.append(stub.calls[n:])
        assert stub.lr_at[-1] == (it, n)              # update_learning_rate first, with trainer.iterations already `it`
    if use_hook:
        assert hooked == [c[0] for c in stub.calls]
    return per_it, drawn[0]


@pytest.mark.parametrize("name", NAMES)
def test_order_of_calls_at_the_reduced_cadence(fx, name):
    cfg = C.reduced_hp(fx, name, "dummy.pth")
    got, drawn = _drive(cfg)
    assert got == C.CADENCE[name]
    assert drawn == 6                                 # one synthetic batch per iteration, shared by the classifier update
    assert _drive(cfg, use_hook=True)[0] == got       # the hook sees every call and changes nothing
    # the synthetic gen_update is not gated by ratio_disc_gen
    assert all(C.S_GEN in calls for calls in got)
    real_gens = [it for it, calls in enumerate(got) if C.R_GEN in calls]
    assert real_gens == [it for it in range(6) if (it + 1) % cfg["ratio_disc_gen"] == 0]
    assert C.count_calls(name, C.ITERATIONS[name], "gen_update") == len([c for calls in got[:C.ITERATIONS[name]] for c in calls
                                                                           if c[0] == "gen_update"])


@pytest.mark.parametrize("name", NAMES)
def test_order_of_calls_at_the_files_own_cadence(fx, name):
    cfg = C.class_config(fx, name)
    assert (cfg["adaptation"]["classif_frequency"], cfg["adaptation"]["output_classif_freq"]) in ((15, 1), (1, 10))
    assert _drive(cfg)[0] == C.CADENCE_OWN[name]
    # the first iterations on which the classifiers are due: it + 1 = 15 for the feature ones, 10 for the output ones
    got = _drive(cfg, iterations=15)[0]
    due = [it for it, calls in enumerate(got) if any("classifier" in c[0] for c in calls)]
    want = {"Baseline": [], "FeatureDA": [14], "FeatureDA+seg": [14], "Output_DA": [9], "Output_DA+seg": [9]}[name]
    assert due == want
    if name.startswith("FeatureDA"):
        assert got[14] == [C.R_DIS, C.R_GEN, ("domain_classifier_sr_update", "real", False, 15), C.S_DIS, C.S_GEN,
                           ("domain_classifier_sr_update", "synth", True, 15)]
    if name.startswith("Output_DA"):
        assert got[9] == [C.R_DIS, C.R_GEN, ("output_domain_classifier_sr_update", "real+synth", 10), C.S_DIS, C.S_GEN]


def test_synthetic_block_is_gated_on_it_and_the_classifier_on_it_plus_one(fx):
    cfg = C.reduced_hp(fx, "FeatureDA", "dummy.pth")
    cfg["synthetic_frequency"] = 2
    got, drawn = _drive(cfg)
    assert got == C.CADENCE_FEATDA_SYNTH2 and drawn == 3
    cfg["synthetic_seg_gt"] = 0                       # scripts/train.py:237-248: the ground truth is withheld
    got, _ = _drive(cfg)
    assert got[0] == [C.R_DIS, C.R_GEN, C.S_DIS, ("gen_update", "synth", True, False)]


def test_without_synthetic_pairs_only_the_real_calls_run(fx):
    from train_loop import run_iteration
    cfg = C.reduced_hp(fx, "FeatureDA", "dummy.pth")
    real = tuple(torch.zeros(1) for _ in range(4))
    stub = _Stub(cfg, real, (None,) * 5)
    run_iteration(stub, cfg, 1, real, None)
    assert stub.calls == [C.R_DIS, C.R_GEN, ("domain_classifier_sr_update", "real", False, 2)]


# ---- the composition of loss_gen_total -------------------------------------------------------------------------------------
BASE_TERMS = ["loss_gen_adv_a", "loss_gen_adv_b", "loss_gen_recon_x_a", "loss_gen_recon_x_b", "loss_gen_recon_s_a",
              "loss_gen_recon_s_b", "loss_gen_recon_c_a", "loss_gen_recon_c_b", "loss_gen_cycrecon_x_a", "loss_gen_cycrecon_x_b"]
EXTRA_TERMS = {      # class -> (real call, synthetic call)
    "Baseline": (["loss_sem_seg"], ["loss_sem_seg", "loss_gen_recon_synth"]),
    "FeatureDA": (["loss_sem_seg", "loss_classifier_sr"], ["loss_sem_seg", "loss_gen_recon_synth", "loss_classifier_sr"]),
    "FeatureDA+seg": (["loss_sem_seg", "loss_classifier_sr"], ["loss_sem_seg", "loss_classifier_sr"]),
    "Output_DA": (["loss_sem_seg", "loss_output_classifier_sr"],
                  ["loss_sem_seg", "loss_gen_recon_synth", "loss_output_classifier_sr"]),
    "Output_DA+seg": (["loss_sem_seg", "loss_output_classifier_sr"], ["loss_sem_seg", "loss_output_classifier_sr"]),
}


@pytest.fixture(scope="module")
def seg_model():
    return S.make_model(0)


@pytest.mark.parametrize("name", NAMES)
def test_composed_total_is_the_weighted_sum_of_the_single_terms(fx, seg_model, name):
    """fp64, forward only, at the GPU test's reduced geometry.  The stacked oracle's loss_gen_total against sum(weight * term):
    the weights from the fixture, the ten base terms from a plain OracleTrainer on the same weights and every further term
    from its single-term function (semantic_oracle.semantic_loss, synth_oracle.ce_gt_loss / pair_loss, featda_oracle.sr_loss,
    outda_oracle.gen_loss_sr) on that plain run's translations and codes.  1e-12 relative."""
    hp = C.reduced_hp(fx, name, "dummy.pth")
    cfg = C.class_config(fx, name)
    dt = torch.float64
    real, synth = C.inputs(hp)
    x_a, x_b, m_a, m_b = (t.to(dt) for t in real)
    x_as, x_bs, mask_s, sem_a, sem_b = (t.to(dt) for t in synth)
    gen, dis_a, dis_b = oracle_states(hp, dt)
    shared = {"sink": None}
    orc = C.composed_oracle_class(hp, seg_model, lambda: None, (sem_a, sem_b), shared)(hp, gen, dis_a, dis_b)
    plain = O.OracleTrainer(hp, gen, dis_a, dis_b)
    ad = hp["adaptation"]
    if ad["adv_lambda"] > 0:
        fresh = lambda: (F.make_state(31), F.make_state(32))       # two copies: training-mode BatchNorm moves the statistics
        own = fresh()
    if ad["output_adv_lambda"] > 0:
        cls = (D.make_state(hp, "ocls_a.", dt), D.make_state(hp, "ocls_b.", dt))
        orc.attach(*cls)
    sd = S.state(seg_model, dt)
    for k, (xa, xb, ma, mb) in enumerate(((x_a, x_b, m_a, m_b), (x_as, x_bs, mask_s, mask_s))):
        orc.synth_call = bool(k)
        if ad["adv_lambda"] > 0:
            shared["sd"] = fresh()
        with torch.no_grad():
            L = orc.gen_losses(xa, xb, ma, mb)
            P = plain.gen_losses(xa, xb, ma, mb)
            last = plain._last
            terms = {t: P[t] for t in BASE_TERMS}
            if k == 0:
                terms["loss_sem_seg"] = (S.semantic_loss(sd, xa, last["x_ab"], ma)[0]
                                         + S.semantic_loss(sd, xb, last["x_ba"], mb)[0])
            else:
                terms["loss_sem_seg"] = (Y.ce_gt_loss(S.logits(sd, last["x_ab"]), sem_a, ma)
                                         + Y.ce_gt_loss(S.logits(sd, last["x_ba"]), sem_b, mb))
                if cfg["recon_synth_w"] > 0:
                    terms["loss_gen_recon_synth"] = Y.pair_loss(xa, xb, last["x_ab"], last["x_ba"])
            if ad["adv_lambda"] > 0:
                terms["loss_classifier_sr"] = F.sr_loss(own[0], own[1], last["c_a"], last["c_b"], fool=True)
                own = fresh()
            if ad["output_adv_lambda"] > 0:
                terms["loss_output_classifier_sr"] = (D.gen_loss_sr(cls[0], last["x_ba"], hp["dis"])
                                                      + D.gen_loss_sr(cls[1], last["x_ab"], hp["dis"]))
        assert sorted(terms) == sorted(BASE_TERMS + EXTRA_TERMS[name][k])
        assert sorted(t for t in L if t != "loss_gen_total") == sorted(terms)
        for t, v in terms.items():
            assert float(v) > 0, t                                     # every term named is non-zero ...
            assert abs(float(L[t]) - float(v)) <= 1e-12 * abs(float(v)), (t, float(L[t]), float(v))
            assert C.weight_of(cfg, t) > 0, t                          # ... and so is its weight
        total = sum(C.weight_of(cfg, t) * float(v) for t, v in terms.items())
        assert abs(float(L["loss_gen_total"]) - total) <= 1e-12 * abs(total), (k, float(L["loss_gen_total"]), total)
        for t in C.WEIGHTS:                                            # a term that is absent has weight 0 or is the other call's
            if t not in terms:
                assert C.weight_of(cfg, t) == 0 or (t == "loss_gen_recon_synth" and k == 0), t
