"""The configurations the reference trains (configs/Final_test/*.yaml, kept as tests/golden/golden_final_configs.json) for
the tests that run them as whole iterations: their classes, the reduced hyper-parameters, the order of calls of one iteration
written out by hand, and the fp64 oracle composed of the single-term oracles.

Classes (files with the same settings once paths, lists, logging and FID keys are dropped):
    Baseline        Baseline, Baseline+seg              semantic 4, pair term 1, ratio_disc_gen 3, batch 2
    FeatureDA       FeatureDA                           + adv_lambda 6 / dfeat_lambda 1, ratio_disc_gen 1, batch 1
    FeatureDA+seg   FeatureDA+seg, FeatureDA+height30_seg   the same without the pair term
    Output_DA       Output_DA                           + output_classifier_lambda 1 / output_adv_lambda 1, batch 2
    Output_DA+seg   Output_DA+seg                       the same without the pair term

Reductions of the GPU test (reduced_hp), everything else is the file's own:
    crop        64 x 64 for Baseline and Output_DA (the smallest multiple of 32 at which all three discriminator scales
                still have an output); 256 x 256 for FeatureDA (the smallest crop domainClassifier.check_code_hw and
                _check_semantic both admit at n_downsample 2)
    depth       gen.n_res 1; dis.num_scales 3 at 64 (the lsgan kernel sees its 6 segments and the 1x1 scale), 1 at 256
    cadence     classif_frequency and output_classif_freq 2 (the files' 15 and 10 never fall in a test's iterations);
                ratio_disc_gen and synthetic_frequency are the file's own
    iterations  3 for Baseline (the real gen_update happens once, after two skipped ones), 2 for the others (each
                classifier update happens once, on it = 1)"""
import json
import os
import re

import torch

from oracle import munit_oracle as O
from tests import featda_oracle as F
from tests import outda_oracle as D
from tests import semantic_oracle as S
from tests import synth_oracle as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "golden_final_configs.json")

CLASSES = {
    "Baseline": ("Baseline", "Baseline+seg"),
    "FeatureDA": ("FeatureDA",),
    "FeatureDA+seg": ("FeatureDA+seg", "FeatureDA+height30_seg"),
    "Output_DA": ("Output_DA",),
    "Output_DA+seg": ("Output_DA+seg",),
}
ITERATIONS = {"Baseline": 3, "FeatureDA": 2, "FeatureDA+seg": 2, "Output_DA": 2, "Output_DA+seg": 2}
IGNORED = ("num_workers",)          # differs inside no class but FeatureDA's own file (8 against 4): not a training setting


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def class_config(fx, name):
    """the settings of a class: its first file's (the test of the fixture asserts that its files agree)"""
    return json.loads(json.dumps(fx[CLASSES[name][0]]))


def crop_of(name):
    return 256 if name.startswith("FeatureDA") else 64


def reduced_hp(fx, name, ckpt):
    hp = class_config(fx, name)
    size = crop_of(name)
    hp["crop_image_height"] = hp["crop_image_width"] = hp["new_size"] = size
    hp["gen"]["n_res"] = 1
    hp["dis"]["num_scales"] = 3 if size == 64 else 1
    hp["adaptation"]["classif_frequency"] = hp["adaptation"]["output_classif_freq"] = 2
    hp["semantic_ckpt_path"] = ckpt
    hp["num_workers"] = 0
    hp.setdefault("optimizer", "adam")
    return hp


# ---- the order of calls, by hand from scripts/train.py:182-274 -------------------------------------------------------------
# (method, batch, ...): gen_update carries (synth, ground truth given), domain_classifier_sr_update (domain_synth, step),
# output_domain_classifier_sr_update (step).  step is it + 1.
R_DIS, S_DIS = ("dis_update", "real"), ("dis_update", "synth")
R_GEN, S_GEN = ("gen_update", "real", False, False), ("gen_update", "synth", True, True)


def _f_real(step):
    return ("domain_classifier_sr_update", "real", False, step)


def _f_synth(step):
    return ("domain_classifier_sr_update", "synth", True, step)


def _o_cls(step):
    return ("output_domain_classifier_sr_update", "real+synth", step)


_BASELINE = [
    [R_DIS, S_DIS, S_GEN],                  # it 0: (0 + 1) % 3 != 0 skips the real gen_update; the synthetic one is not gated
    [R_DIS, S_DIS, S_GEN],                  # it 1
    [R_DIS, R_GEN, S_DIS, S_GEN],           # it 2: (2 + 1) % 3 == 0
    [R_DIS, S_DIS, S_GEN],                  # it 3
    [R_DIS, S_DIS, S_GEN],                  # it 4
    [R_DIS, R_GEN, S_DIS, S_GEN],           # it 5
]
_FEATDA = [
    [R_DIS, R_GEN, S_DIS, S_GEN],                               # it 0: (0 + 1) % 2 != 0, no classifier update
    [R_DIS, R_GEN, _f_real(2), S_DIS, S_GEN, _f_synth(2)],      # it 1: (1 + 1) % 2 == 0, both, with step 2
    [R_DIS, R_GEN, S_DIS, S_GEN],
    [R_DIS, R_GEN, _f_real(4), S_DIS, S_GEN, _f_synth(4)],
    [R_DIS, R_GEN, S_DIS, S_GEN],
    [R_DIS, R_GEN, _f_real(6), S_DIS, S_GEN, _f_synth(6)],
]
_OUTDA = [
    [R_DIS, R_GEN, S_DIS, S_GEN],
    [R_DIS, R_GEN, _o_cls(2), S_DIS, S_GEN],                    # the classifier update and the synthetic step share one pair
    [R_DIS, R_GEN, S_DIS, S_GEN],
    [R_DIS, R_GEN, _o_cls(4), S_DIS, S_GEN],
    [R_DIS, R_GEN, S_DIS, S_GEN],
    [R_DIS, R_GEN, _o_cls(6), S_DIS, S_GEN],
]
# at the reduced cadence (classif_frequency 2, output_classif_freq 2), iterations 0..5
CADENCE = {"Baseline": _BASELINE, "FeatureDA": _FEATDA, "FeatureDA+seg": _FEATDA, "Output_DA": _OUTDA, "Output_DA+seg": _OUTDA}
# at the files' own cadence (classif_frequency 15, output_classif_freq 10) no classifier update falls in iterations 0..5
_PLAIN = [[R_DIS, R_GEN, S_DIS, S_GEN]] * 6
CADENCE_OWN = {"Baseline": _BASELINE, "FeatureDA": _PLAIN, "FeatureDA+seg": _PLAIN, "Output_DA": _PLAIN, "Output_DA+seg": _PLAIN}
# FeatureDA with synthetic_frequency 2 and classif_frequency 2: the synthetic block is gated on `it` (0, 2, 4), the classifier
# updates on `it + 1` (it = 1, 3, 5): the two never meet, so domain_classifier_sr_update(synthetic) never runs
CADENCE_FEATDA_SYNTH2 = [
    [R_DIS, R_GEN, S_DIS, S_GEN],
    [R_DIS, R_GEN, _f_real(2)],
    [R_DIS, R_GEN, S_DIS, S_GEN],
    [R_DIS, R_GEN, _f_real(4)],
    [R_DIS, R_GEN, S_DIS, S_GEN],
    [R_DIS, R_GEN, _f_real(6)],
]


def count_calls(name, iterations, method):
    return sum(1 for calls in CADENCE[name][:iterations] for c in calls if c[0] == method)


# ---- parameters with an identically zero gradient -----------------------------------------------------------------------
# a convolution bias ahead of an instance norm (the content encoders) or ahead of AdaIN (the decoders' residual blocks)
NULL_PATTERN = re.compile(r"^(enc[12]_content\.model\..*conv\.bias|dec[12]\.model\.0\..*conv\.bias)$")


def null_count(hp):
    g = hp["gen"]
    return 2 * (1 + g["n_downsample"] + 2 * g["n_res"]) + 2 * 2 * g["n_res"]


# ---- the composed oracle ------------------------------------------------------------------------------------------------
def composed_oracle_class(hp, seg_model, seg_sink, gts, shared):
    """One class for a whole iteration, innermost first: OracleTrainer, the output term (tests/outda_oracle.py) or the
    fooling term (tests/featda_oracle.py) as `hp` says, the pseudo-label semantic term (tests/semantic_oracle.py), then the
    pair term and the ground-truth semantic term (tests/synth_oracle.py).  The instance's `synth_call` selects which of the
    two semantic oracles acts: False for the real gen_update, True for gen_update(synth=True).  Pinned kinks are consumed in
    the order the HIP gen_update records them: MASK_SINK / L1_SINK by the base terms with the output term right behind the
    adversarial ones and the pair term's two sign patterns last; DANN_SINK (`shared["sink"]`) and SEG_SINK (`seg_sink()`)
    are lists of their own.  A sink of None leaves that oracle unpinned (the host-side composition check)."""
    ad = hp["adaptation"]
    cls = None
    if ad["output_adv_lambda"] > 0:
        cls = D.oracle_trainer_class(cls)
    if ad["adv_lambda"] > 0:
        cls = F.oracle_trainer_class(shared, cls)
    cls = S.oracle_trainer_class(seg_model, seg_sink, cls)
    return Y.oracle_trainer_class(seg_model, seg_sink, gts, cls)


WEIGHTS = {      # loss name -> where its weight stands in the configuration
    "loss_gen_adv_a": ("gan_w",), "loss_gen_adv_b": ("gan_w",),
    "loss_gen_recon_x_a": ("recon_x_w",), "loss_gen_recon_x_b": ("recon_x_w",),
    "loss_gen_recon_s_a": ("recon_s_w",), "loss_gen_recon_s_b": ("recon_s_w",),
    "loss_gen_recon_c_a": ("recon_c_w",), "loss_gen_recon_c_b": ("recon_c_w",),
    "loss_gen_cycrecon_x_a": ("recon_x_cyc_w",), "loss_gen_cycrecon_x_b": ("recon_x_cyc_w",),
    "loss_sem_seg": ("semantic_w",), "loss_gen_recon_synth": ("recon_synth_w",),
    "loss_classifier_sr": ("adaptation", "adv_lambda"), "loss_output_classifier_sr": ("adaptation", "output_adv_lambda"),
}


def weight_of(cfg, loss):
    v = cfg
    for k in WEIGHTS[loss]:
        v = v[k]
    return v


def inputs(hp):
    """The real pair (O.synthetic_batch) and the synthetic pair (Y.pair_inputs, Y.gt_maps and one 0 / 1 mask) of a test, fp32
    values on the host: (x_a, x_b, m_a, m_b), (x_as, x_bs, mask_s, sem_a, sem_b)"""
    b, size = hp["batch_size"], hp["crop_image_height"]
    real = O.synthetic_batch(b, size, seed=7)
    x_as, x_bs = Y.pair_inputs(b, size, 17, dtype=torch.float32)[:2]
    g = torch.Generator().manual_seed(18)
    mask_s = (torch.rand(b, 1, size, size, generator=g) > 0.5).float()
    sem_a, sem_b = Y.gt_maps(b, size, 19).unsqueeze(1).float(), Y.gt_maps(b, size, 20).unsqueeze(1).float()
    return real, (x_as, x_bs, mask_s, sem_a, sem_b)
