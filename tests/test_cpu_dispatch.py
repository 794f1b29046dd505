"""CPU (no GPU): every convolution kernel form a training step can dispatch to is run by an fp64 op test.

The conv library picks one of ~25 kernel forms per pass from shape thresholds and divisibility (Winograd F(2x2,3x3) and
F(3x3,2x2), sub-pixel, box-sum, LDS patch, folded gather, 3-channel taps, split-K, FAST / XCLAMP loaders).  The op tests
(tests/test_gpu_ops.py::CONV_CASES, tests/test_gpu_shapes.py::LAYERS) aim at those forms; this file checks that they reach
them.  It lists every conv layer of the step (the oracle's generator and discriminator forward on `meta` tensors, with
hooks on O.conv_block / O.upsample2 / the 1x1 heads / the MLP linears) for every geometry of tests/geometries.ALL and for
configs/config_256.yaml's networks at several crops, batches and padding modes, asks the library which kernel carries each
pass (munit_conv2d_kernel_name mirrors the dispatch of the entry points), and requires each (pass, kernel) pair to be one
that an op test runs.  It also requires every kernel name the dispatch can return to be covered, so that a new branch
cannot land without an op test, and pins the kernel names of the cases added for that purpose (CONV_CASES_TARGETS).

The frozen Resnet34_8s of the semantic loss (tests/seg_layers.py lists its 37 convolutions from the module itself) is a
second production grid: every square crop that is a multiple of 32 from 64 to 512, B and 2B images.  Its layers differ
from the generators' by zero padding, a bias, the zero-extended backward-data filter of the stride-2 layers and the `add`
operand, so a layer counts as covered only by a case of tests/test_gpu_semantic.py::SEG_CONV_CASES (run through
ops.frozen_conv) that has the layer's channels, filter and stride and takes the same (pass, kernel name)."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from oracle import munit_oracle as O
from tests import geometries as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES = ("fwd", "dgrad", "wgrad")
BATCHES = (1, 2, 3, 4, 8, 16, 32)
CROPS_256 = (64, 96, 128, 192, 256, 384, 512, (256, 512), (360, 480))
# reachable only with a MUNIT_DEBUG_* switch set (MUNIT_DEBUG_NO_WGRAD_PK; MUNIT_DEBUG_NO_HEAD_PK, alone and with
# MUNIT_DEBUG_NO_HEAD_MFMA, for the head kernels of the forward and of the 3-channel backward-data): the op tests never force a
# debug fallback
_HEAD_FALLBACKS = {k + x + s for k in ("conv_head_mfma_kernel", "conv_patch_fwd_kernel") for x in ("", "<bf16_t>")
                   for s in ("", " (padded-domain correlation)")}
DEBUG_ONLY = {"conv_lanes_wgrad_kernel", "conv_lanes_wgrad_kernel<bf16_t>"} | _HEAD_FALLBACKS
# backward-data of a bf16 x against an fp32 dy outside the 3-channel image head: the entry point runs it, but no caller can
# use it (the backward-weight of the same descriptor is refused: "bf16 x with fp32 dy exists for the 3-channel image head
# only"), so munit_amd.ops never plans one and no op test body can drive it.  Named, not covered.
NO_CALLER = {"conv_igemm_kernel<.., 1, %s> phases + fold_kernel<bf16_t>" % ct for ct in ("1", "2", ".")}
SEG_CROPS = tuple(range(64, 513, 32))
# The names of the launch branches only a descriptor with compute != 0 or a bf16 tensor can take.  The dispatch must keep
# telling them apart: a branch that went back to reporting under its fp32 name would leave the coverage tests blind to it.
NON_F32_FORMS = {
    "conv_head_pk_kernel<bf16_t>", "conv_head_pk_kernel<bf16_t> (padded-domain correlation)",
    "conv_igemm_kernel<64, true, 0, 4>", "conv_igemm_kernel<128, true, 0, 4>",
    "conv_igemm_kernel<64, true, 0, 4> x4 sub-pixel phases + frame", "conv_igemm_kernel<128, true, 0, 4> x4 sub-pixel phases + frame",
    "conv_igemm_kernel<.., 0, 1>", "conv_igemm_kernel<.., 0, 2>",
    "conv_igemm_kernel<.., 0, 1> x4 sub-pixel phases + frame", "conv_igemm_kernel<.., 0, 2> x4 sub-pixel phases + frame",
    "conv_igemm_kernel<.., 5> (3 input channels as 4-channel taps, bf16 y)",
    "box2x2_kernel + conv_igemm_kernel<.., 1> (box-sum backward-data)", "box2x2_kernel + conv_igemm_kernel<.., 2> (box-sum backward-data)",
    "conv_igemm_kernel<64, true, 2, 4> (LDS-patch fold)", "conv_igemm_kernel<128, true, 2, 4> (LDS-patch fold)",
    "conv_igemm_kernel<.., 2, 1> (folded gather)", "conv_igemm_kernel<.., 2, 2> (folded gather)",
    "conv_igemm_kernel<.., 1, 5> (3 output channels as 4-channel taps) + fold_kernel<bf16_t>",
    "conv_igemm_kernel<64, true, 1, 4> direct", "conv_igemm_kernel<128, true, 1, 4> direct",
    "conv_igemm_kernel<.., 1, 1> direct", "conv_igemm_kernel<.., 1, 2> direct",
    "conv_igemm_kernel<64, true, 1, 4> phases + fold_kernel<bf16_t>", "conv_igemm_kernel<128, true, 1, 4> phases + fold_kernel<bf16_t>",
    "conv_igemm_kernel<64, true, 1, 4> phases + fold_kernel", "conv_igemm_kernel<128, true, 1, 4> phases + fold_kernel",
    "conv_igemm_kernel<.., 1, 1> phases + fold_kernel", "conv_igemm_kernel<.., 1, 2> phases + fold_kernel",
    "conv_lanes_wgrad_pk_kernel<bf16_t>", "conv_lanes_wgrad_kernel<bf16_t>",
    "conv_wgrad_bf16s_kernel<1> + slab_reduce_kernel", "conv_wgrad_bf16s_kernel<2> + slab_reduce_kernel",
    "conv_wgrad_bf16s_kernel<1> x4 sub-pixel phases + frame",
    "conv_wgrad_kernel<.., 1, true, true> + slab_reduce_kernel", "conv_wgrad_kernel<.., 0, false, true> + slab_reduce_kernel",
    "conv_wgrad_kernel<.., 0, false, true> (3 input channels padded to 4, bf16 dy)",
    "conv_wgrad_kernel<.., 1> + slab_reduce_kernel", "conv_wgrad_kernel<.., 2> + slab_reduce_kernel",
    "conv_wgrad_kernel<.., 1> x4 sub-pixel phases + fp32 frame", "conv_wgrad_kernel<.., 2> x4 sub-pixel phases + fp32 frame",
} | {n for n in _HEAD_FALLBACKS if "<bf16_t>" in n}


@pytest.fixture(scope="module")
def lib():
    from munit_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------------
# layer enumeration
# ------------------------------------------------------------------------------------------------------------------
_SECTION = [None]      # which sub-network the traced code is in (set by bf16s_network_layers' wrappers)


def _trace(run, sections=None):
    """Run `run()` (oracle forward code on meta tensors) and return the conv layers it calls, in call order, as
    (cin, cout, k, stride, pad, pad_type, upsample, act, H, W) at the batch of its input.  H, W are the layer's INPUT
    extent before the fused nearest x2 (what munit_conv_desc holds); act is what the device fuses into the conv (none
    when a norm follows: the norm kernels carry the activation then).  `sections`: a list that receives _SECTION[0] at each
    record."""
    rec = []

    def note():
        if sections is not None:
            sections.append(_SECTION[0])
    st = {"ups": False, "lin_out": None}

    def out(x, cout, k, stride, pad):
        b, _, h, w = x.shape
        return x.new_empty(b, cout, (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1)

    def conv_block(x, w, b, stride, pad, pad_type, norm_fn=None, activ="none"):
        cout, cin, k, _ = w.shape
        ups, st["ups"] = st["ups"], False
        h, wd = x.shape[2:]
        if ups:
            h, wd = h // 2, wd // 2
        rec.append((cin, cout, k, stride, pad, pad_type, int(ups), activ if norm_fn is None else "none", h, wd))
        note()
        return out(x, cout, k, stride, pad)

    def upsample2(x):
        st["ups"] = True
        b, c, h, w = x.shape
        return x.new_empty(b, c, 2 * h, 2 * w)

    def activation(x, kind):
        if st["lin_out"] is not None and x is st["lin_out"][0]:      # the MLP's activation is fused into the linear
            i = st["lin_out"][1]
            rec[i] = rec[i][:7] + (kind,) + rec[i][8:]
        return x

    class _F(object):
        """torch.nn.functional for the oracle module: the bare 1x1 heads and the linears are recorded, the rest passes."""

        def __getattr__(self, name):
            return getattr(torch.nn.functional, name)

        def conv2d(self, x, w, b=None, stride=1):
            cout, cin, k, _ = w.shape
            rec.append((cin, cout, k, stride, 0, "zero", 0, "none", x.shape[2], x.shape[3]))
            note()
            return out(x, cout, k, stride, 0)

        def linear(self, x, w, b=None):
            n, k = w.shape
            rec.append((k, n, 1, 1, 0, "zero", 0, "none", 1, 1))
            note()
            y = x.new_empty(x.shape[0], n)
            st["lin_out"] = (y, len(rec) - 1)
            return y

    saved = O.conv_block, O.upsample2, O.activation, O.F
    O.conv_block, O.upsample2, O.activation, O.F = conv_block, upsample2, activation, _F()
    try:
        run()
    finally:
        O.conv_block, O.upsample2, O.activation, O.F = saved
    assert not st["ups"], "an up-sampling without a conv behind it"
    return rec


def _meta_state(shapes):
    return {k: torch.empty(s, device="meta") for k, s in shapes.items()}


def network_layers(hp):
    """{(layer at batch 1): batch multipliers} of one config: the generators (both layouts, every domain's input_dim)
    at the step's batch, the discriminators at 2B (dis_update feeds fake and real together) and B (gen_update)."""
    size = (hp["crop_image_height"], hp["crop_image_width"])
    layers = {}
    for input_dim in sorted({hp["input_dim_a"], hp["input_dim_b"]}):
        x = torch.empty(1, input_dim, *size, device="meta")
        for double in (True, False):
            g = O.GenView(_meta_state(O.gen_param_shapes(hp["gen"], input_dim, double)), hp["gen"], double)

            def gen():
                c, s = g.encode(x, 1 if double else None)
                g.decode(c, s, 1 if double else None)
            for l in _trace(gen):
                layers.setdefault(l, set()).add(1)
        sd = _meta_state(O.dis_param_shapes(hp["dis"], input_dim))
        for l in _trace(lambda: O.dis_forward(sd, "", x, hp["dis"])):
            layers.setdefault(l, set()).update((1, 2))
    return layers


def production_grid():
    """(config label, hp) of every configuration the step runs in: tests/geometries.ALL and config_256.yaml's networks at
    several crops with reflect and with zero padding."""
    grid = [(name, G.merged_hp(O.default_hp, size, over)) for name, size, over in G.ALL]
    for crop in CROPS_256:
        for pt in ("reflect", "zero"):
            hp = O.default_hp(crop)
            hp["gen"] = dict(hp["gen"], pad_type=pt)
            hp["dis"] = dict(hp["dis"], pad_type=pt)
            grid.append(("config_256 %s %s" % (crop if isinstance(crop, int) else "%dx%d" % crop, pt), hp))
    return grid


F32_MODE = (0, 0, 0)    # (compute, in_dtype, out_dtype) = (MUNIT_COMPUTE_*, MUNIT_DTYPE_*, MUNIT_DTYPE_*): fp32 throughout
F32, BF16 = 0, 1        # MUNIT_DTYPE_*


def _desc(case, which, mode=F32_MODE):
    """munit_conv_desc of an op case (cin, cout, k, stride, pad, pad_type, ups, act, B, H, W) for pass `which`, with the
    arithmetic and tensor types of `mode` (default: fp32 tensors and arithmetic); the activation is fused into the forward
    only (as munit_amd.ops plans the three passes)."""
    from munit_amd._lib import ACT, PAD, ConvDesc
    cin, cout, k, stride, pad, pt, ups, act, b, h, w = case
    compute, in_dt, out_dt = mode
    return ConvDesc(b, h, w, cin, cout, k, k, stride, pad, PAD[pt], int(ups), ACT[act if which == 0 else "none"], 0.2,
                    compute, in_dt, out_dt)


def kernel_names(lib, case, mode=F32_MODE):
    import ctypes
    return tuple(lib.munit_conv2d_kernel_name(ctypes.byref(_desc(case, p, mode)), p).decode() for p in range(3))


def macs(case):
    cin, cout, k, stride, pad, pt, ups, act, b, h, w = case
    ho = ((h << ups) + 2 * pad - k) // stride + 1
    wo = ((w << ups) + 2 * pad - k) // stride + 1
    return b * ho * wo * cout * k * k * cin


def production_cases():
    """{op case: first config label} over the whole grid (batch scaled in)."""
    cases = {}
    for label, hp in production_grid():
        for l, mult in network_layers(hp).items():
            cin, cout, k, stride, pad, pt, ups, act, h, w = l
            for b in BATCHES:
                for m in sorted(mult):
                    cases.setdefault((cin, cout, k, stride, pad, pt, ups, act, b * m, h, w), "%s B=%d" % (label, b))
    return cases


# ------------------------------------------------------------------------------------------------------------------
# the set the op tests cover
# ------------------------------------------------------------------------------------------------------------------
def op_cases():
    """Every conv case of the fp64 op tests, as (cin, cout, k, stride, pad, pad_type, ups, act, B, H, W)."""
    from tests.test_gpu_ops import CONV_CASES, LINEAR_CASES
    from tests.test_gpu_shapes import LAYERS
    cases = list(CONV_CASES)
    cases += [(ci, co, k, s, p, "reflect", u, a, b, h, w) for _, ci, co, k, s, p, u, a, b, h, w in LAYERS]
    cases += [(k, n, 1, 1, 0, "zero", 0, a, b, 1, 1) for b, k, n, a in LINEAR_CASES]
    return cases


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from tests.test_cpu_dispatch import kernel_names
from munit_amd import _lib
print(json.dumps([kernel_names(_lib.load(), tuple(c)) for c in json.loads(sys.argv[2])]))
"""


def covered(lib):
    """{(pass, kernel name)} the op tests run: each case at the default thresholds, and the 4x4 / stride 2 cases again under
    MUNIT_WINO_S2_MIN_BLOCKS=1 (test_conv_stride2_winograd_on_small_shapes).  The library reads that variable once per
    process, so those names come from a child process that only loads the library (no GPU)."""
    cases = op_cases()
    names = [kernel_names(lib, c) for c in cases]
    k4s2 = [c for c in cases if c[2] == 4 and c[3] == 2]
    env = dict(os.environ, MUNIT_WINO_S2_MIN_BLOCKS="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(k4s2)], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    names += [tuple(n) for n in json.loads(r.stdout.strip().splitlines()[-1])]
    return {(p, n[p]) for n in names for p in range(3)}


def dispatch_literals():
    """Every kernel name munit_igemm_kernel_name and munit_conv2d_kernel_name can return, read from their source."""
    out = []
    for fname, func in (("conv_igemm.hip", "munit_igemm_kernel_name"), ("conv_wgrad.hip", "munit_conv2d_kernel_name")):
        src = open(os.path.join(ROOT, "munit_amd", "csrc", fname)).read()
        m = re.search(r"\b%s\(const munit_conv_desc\* d, int pass\) \{(.*?)\n\}" % func, src, re.S)
        assert m, (fname, func)
        out += [s for s in re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1)) if "_kernel" in s]
    return out


def test_every_production_conv_form_is_covered_by_an_op_test(lib):
    cov = covered(lib)
    prod = production_cases()
    missing = {}
    for case, label in prod.items():
        for p, name in enumerate(kernel_names(lib, case)):
            if (p, name) not in cov:
                best = missing.get((p, name))
                if best is None or macs(case) < macs(best[0]):
                    missing[(p, name)] = (case, label)
    assert len(prod) > 1000, len(prod)
    assert not missing, "kernel forms production dispatches to that no op test runs (cheapest layer of each):\n" + "\n".join(
        "  %s %s: %s  (%s, %.2f GMAC)" % (PASSES[p], n, c, lab, macs(c) / 1e9) for (p, n), (c, lab) in sorted(missing.items()))


def F32_FORMS(lib, lits):
    """The literals an fp32 descriptor with fp32 arithmetic can get: those the fp32 op cases and the fp32 production grid take,
    and the fp32 debug fallbacks."""
    names = {n for _, n in covered(lib)} | (DEBUG_ONLY - NON_F32_FORMS)
    return {n for n in lits if n in names}


def test_every_dispatch_branch_is_covered_by_an_op_test(lib):
    lits = dispatch_literals()
    assert len(lits) >= 25, lits
    assert DEBUG_ONLY | NO_CALLER <= set(lits), DEBUG_ONLY | NO_CALLER
    assert NON_F32_FORMS | NO_CALLER == set(lits) - F32_FORMS(lib, lits), (NON_F32_FORMS | NO_CALLER) ^ (set(lits) - F32_FORMS(lib, lits))
    names = {n for _, n in covered(lib) | bf16_covered(lib)}
    assert not names & (DEBUG_ONLY | NO_CALLER), names & (DEBUG_ONLY | NO_CALLER)
    missing = [n for n in lits if n not in names and n not in DEBUG_ONLY | NO_CALLER]
    assert not missing, "kernel names the dispatch can return that no op test runs: %s" % missing


def test_added_cases_keep_their_kernels(lib):
    """The op cases added to reach a form pin that form: a later threshold change cannot quietly move them off it."""
    from tests.test_gpu_ops import CONV_CASES, CONV_CASES_TARGETS, CONV_CASES_TARGETS_S2_MIN1
    assert CONV_CASES_TARGETS and CONV_CASES_TARGETS_S2_MIN1
    small = list(CONV_CASES_TARGETS_S2_MIN1)
    env = dict(os.environ, MUNIT_WINO_S2_MIN_BLOCKS="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(small)], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got_small = dict(zip(small, json.loads(r.stdout.strip().splitlines()[-1])))
    for targets, names in ((CONV_CASES_TARGETS, lambda c: kernel_names(lib, c)), (CONV_CASES_TARGETS_S2_MIN1, got_small.get)):
        for case, want in targets.items():
            assert case in CONV_CASES, case
            if targets is CONV_CASES_TARGETS_S2_MIN1:
                assert case[2] == 4 and case[3] == 2, "only the 4x4 / stride 2 cases run under MUNIT_WINO_S2_MIN_BLOCKS=1"
            for p, (g, w) in enumerate(zip(names(case), want)):
                assert w is None or g == w, (case, PASSES[p], g, w)
    # the cases added for the bf16-storage / bf16-arithmetic forms
    from tests import test_gpu_bf16 as B16, test_gpu_bf16s as B16S
    assert B16S.BF16S_CASES_TARGETS and B16.BF16_CASES_TARGETS
    pinned = {(c, mode): passes for c, mode, passes in bf16_op_cases()}
    dt = {torch.float32: F32, torch.bfloat16: BF16}
    for case, want in B16S.BF16S_CASES_TARGETS.items():
        ci, co, k, s, p_, u, a, b, h, w = case[:10]
        key = ((ci, co, k, s, p_, case[12] if len(case) > 12 else "reflect", u, a, b, h, w), (1, dt[case[10]], dt[case[11]]))
        assert case in B16S.CASES and pinned[key] == (0, 1, 2), case
        for p, (g, w_) in enumerate(zip(kernel_names(lib, *key), want)):
            assert w_ is None or g == w_, (case, PASSES[p], g, w_)
    for case, want in B16.BF16_CASES_TARGETS.items():
        assert case in B16.CASES and pinned[(case, (1, F32, F32))] == (0, 1), case
        for p, (g, w_) in enumerate(zip(kernel_names(lib, case, (1, F32, F32)), want)):
            assert g == w_, (case, PASSES[p], g, w_)


def test_layer_enumeration_matches_the_parameter_list():
    """The hooks see every conv of the networks: one record per conv / linear weight of the generator (one domain of
    AdaINGen) and of the discriminator."""
    hp = O.default_hp(96)
    x = torch.empty(1, 3, 96, 96, device="meta")
    gshapes = O.gen_param_shapes(hp["gen"], 3, False)
    g = O.GenView(_meta_state(gshapes), hp["gen"], False)
    rec = _trace(lambda: g.decode(*g.encode(x)))
    assert len(rec) == sum(1 for k, s in gshapes.items() if k.endswith("weight")), len(rec)
    ups = [l for l in rec if l[6]]
    assert [(l[0], l[1], l[8]) for l in ups] == [(256, 128, 24), (128, 64, 48)], ups
    # the style head on the pooled 1x1 code, then the MLP's three linears with the generator's activation fused into two
    assert [(l[0], l[1], l[7]) for l in rec if l[8:] == (1, 1)] == [(256, 16, "none"), (16, 256, "relu"), (256, 256, "relu"),
                                                                    (256, 4096, "none")], rec
    dshapes = O.dis_param_shapes(hp["dis"], 3)
    drec = _trace(lambda: O.dis_forward(_meta_state(dshapes), "", x, hp["dis"]))
    assert len(drec) == sum(1 for k in dshapes if k.endswith("weight")) == 15
    assert [l[8] for l in drec if l[2] == 1] == [6, 3, 1]          # the heads of the three scales (96, 48, 24 pixels in)


# ------------------------------------------------------------------------------------------------------------------
# the bf16-storage step (`precision: bf16s`)
# ------------------------------------------------------------------------------------------------------------------
BF16S_COMPUTE = 1       # MUNIT_COMPUTE_BF16: ops.set_compute("bf16s") is process-wide, every conv of the step carries it


def bf16s_generator_layers(hp_gen, input_dim, double, size):
    """[(layer at batch 1, (compute, in_dtype, out_dtype))] of one generator in a bf16s step, in call order.  The dtypes are
    those of the trainer's tensors: the content encoder's first conv reads the fp32 image and writes
    ContentEncoder.store_dtype = bf16; every later conv of the content encoder and of the decoder reads bf16 and writes what
    ops.conv2d_fwd_raw gives a bf16 input (bf16 when Cout is a multiple of 64, else fp32: the image head); the style encoder
    and the MLP (fp32 image / fp32 style code in) stay fp32."""
    x = torch.empty(1, input_dim, *size, device="meta")
    g = O.GenView(_meta_state(O.gen_param_shapes(hp_gen, input_dim, double)), hp_gen, double)
    saved = O.content_encoder, O.decoder

    def within(name, fn):
        def wrapped(*a, **k):
            _SECTION[0] = name
            try:
                return fn(*a, **k)
            finally:
                _SECTION[0] = None
        return wrapped

    O.content_encoder, O.decoder = within("content", saved[0]), within("decoder", saved[1])
    sections = []
    try:
        rec = _trace(lambda: g.decode(*g.encode(x, 1 if double else None), 1 if double else None), sections)
    finally:
        O.content_encoder, O.decoder = saved
    out, first = [], True
    for l, sec in zip(rec, sections):
        if sec is None:
            mode = (BF16S_COMPUTE, F32, F32)
        else:
            in_dt = F32 if (sec == "content" and first) else BF16
            out_dt = BF16 if (sec == "content" and first) or l[1] % 64 == 0 else F32
            first = first and sec != "content"
            mode = (BF16S_COMPUTE, in_dt, out_dt)
        out.append((l, mode))
    return out


def bf16s_network_layers(hp):
    """{(layer at batch 1, mode): batch multipliers} of one config in bf16 storage (see network_layers); the discriminators
    run on fp32 images with the step's arithmetic."""
    size = (hp["crop_image_height"], hp["crop_image_width"])
    layers = {}
    for input_dim in sorted({hp["input_dim_a"], hp["input_dim_b"]}):
        for double in (True, False):
            for lm in bf16s_generator_layers(hp["gen"], input_dim, double, size):
                layers.setdefault(lm, set()).add(1)
        x = torch.empty(1, input_dim, *size, device="meta")
        sd = _meta_state(O.dis_param_shapes(hp["dis"], input_dim))
        for l in _trace(lambda: O.dis_forward(sd, "", x, hp["dis"])):
            layers.setdefault((l, (BF16S_COMPUTE, F32, F32)), set()).update((1, 2))
    return layers


def bf16s_production_cases(refused_up_front=False):
    """{(op case, mode): first config label} over production_grid() x BATCHES in bf16 storage, restricted to what
    MUNIT_Trainer accepts in that mode (munit_amd.trainer.bf16s_refusal; semantic_w adds no conv on these tensors).
    refused_up_front=True returns the complement: the configurations the trainer turns away."""
    from munit_amd.trainer import bf16s_refusal
    cases = {}
    for label, hp in production_grid():
        layers = None
        for b in BATCHES:
            if (bf16s_refusal(dict(hp, batch_size=b)) is not None) != refused_up_front:
                continue
            layers = layers or bf16s_network_layers(hp)
            for (l, mode), mult in layers.items():
                cin, cout, k, stride, pad, pt, ups, act, h, w = l
                for m in sorted(mult):
                    cases.setdefault(((cin, cout, k, stride, pad, pt, ups, act, b * m, h, w), mode), "%s B=%d" % (label, b))
    return cases


def bf16_op_cases():
    """[(op case, mode, passes)] of the fp64 op tests that run under ops.set_compute("bf16s") / "bf16" / "f32x3"."""
    from tests.test_gpu_bf16 import CASES as BF16_CASES, WGRAD_CASES
    from tests.test_gpu_bf16s import CASES as BF16S_CASES
    from tests.test_gpu_f32x3 import F32X3_CASES
    from tests.test_gpu_ops import LINEAR_CASES
    from tests.test_gpu_shapes import BF16S_TRUNK_LAYER
    dt = {torch.float32: F32, torch.bfloat16: BF16}
    out = [(c[:5] + (c[12] if len(c) > 12 else "reflect",) + c[5:10], (1, dt[c[10]], dt[c[11]]), (0, 1, 2)) for c in BF16S_CASES]
    ci, co, k, s, p, u, a, b, h, w = BF16S_TRUNK_LAYER
    out.append(((ci, co, k, s, p, "reflect", u, a, b, h, w), (1, BF16, BF16), (0, 1, 2)))
    out += [(tuple(c), (1, F32, F32), (0, 1)) for c in BF16_CASES]     # its dw is held to the mode's loose bound only
    out += [((ci, co, k, s, p, pt, u, "none", b, h, w), (1, F32, F32), (2,)) for ci, co, k, s, p, pt, u, b, h, w in WGRAD_CASES]
    out += [(tuple(c), (2, F32, F32), (0, 1, 2)) for c in F32X3_CASES]
    out += [((k, n, 1, 1, 0, "zero", 0, a, b, 1, 1), (2, F32, F32), (0, 1, 2)) for b, k, n, a in LINEAR_CASES]   # test_linear_f32x3
    return out


def bf16_covered(lib):
    """{(pass, kernel name)} those op tests run; a wgrad-only case covers the wgrad pass only."""
    return {(p, kernel_names(lib, c, mode)[p]) for c, mode, passes in bf16_op_cases() for p in passes}


def test_every_bf16s_production_conv_form_is_covered_by_an_op_test(lib):
    cov = covered(lib) | bf16_covered(lib)
    prod = bf16s_production_cases()
    missing = {}
    for (case, mode), label in prod.items():
        for p, name in enumerate(kernel_names(lib, case, mode)):
            if (p, name) not in cov:
                best = missing.get((p, name))
                if best is None or macs(case) < macs(best[0]):
                    missing[(p, name)] = (case, mode, label)
    assert len(prod) > 1000, len(prod)
    assert not missing, ("kernel forms a bf16-storage step dispatches to that no op test runs (cheapest layer of each, with its "
                         "(compute, in_dtype, out_dtype)):\n" + "\n".join(
                             "  %s %s: %s %s  (%s, %.2f GMAC)" % (PASSES[p], n, c, m, lab, macs(c) / 1e9)
                             for (p, n), (c, m, lab) in sorted(missing.items())))


def test_no_bf16s_production_conv_is_refused(lib):
    """No conv of a configuration the trainer accepts in bf16 storage is one its entry point would refuse at launch (a
    failure inside backward); the configurations the trainer turns away do hold such layers, so the refusal is not idle."""
    def refused(cases):
        return sorted((PASSES[p], n, c, m, lab) for (c, m), lab in cases.items()
                      for p, n in enumerate(kernel_names(lib, c, m)) if n.startswith("refused:") or n == "invalid")
    bad = refused(bf16s_production_cases())
    assert not bad, "bf16-storage layers the entry points refuse:\n" + "\n".join("  %s %s: %s %s (%s)" % r for r in bad[:20])
    away = bf16s_production_cases(refused_up_front=True)
    wide = {k: v for k, v in away.items() if v.startswith("config_256 512 ")}
    assert wide and {r[:2] for r in refused(wide)} == {("wgrad", "refused: bf16 tensors need Cin % 4 == 0, Cout % 4 == 0, "
                                                        "tensors below 2 GiB and B*H*W < 2^23")}, refused(wide)[:4]


# (cin, cout, in_dtype, out_dtype) of default_hp(96)'s generator: the style encoder (fp32), the content encoder (fp32 image ->
# bf16, then bf16), the MLP (fp32), the decoder (bf16 up to the fp32 image head)
BF16S_GENERATOR_96 = ([(3, 64, F32, F32), (64, 128, F32, F32), (128, 256, F32, F32), (256, 256, F32, F32), (256, 256, F32, F32),
                       (256, 16, F32, F32)]
                      + [(3, 64, F32, BF16), (64, 128, BF16, BF16), (128, 256, BF16, BF16)] + [(256, 256, BF16, BF16)] * 8
                      + [(16, 256, F32, F32), (256, 256, F32, F32), (256, 4096, F32, F32)]
                      + [(256, 256, BF16, BF16)] * 8 + [(256, 128, BF16, BF16), (128, 64, BF16, BF16), (64, 3, BF16, F32)])


def test_trainer_refuses_bf16s_configurations_up_front():
    """What a bf16-storage step cannot run is a ValueError of MUNIT_Trainer.__init__ that names the bound, not an error of a
    kernel entry point inside backward."""
    from munit_amd import ops
    from munit_amd.trainer import MUNIT_Trainer, bf16s_refusal
    hp = O.default_hp(512, 32)
    assert bf16s_refusal(dict(hp, batch_size=16)) is None and bf16s_refusal(dict(O.default_hp(256, 32))) is None
    assert "2^23" in bf16s_refusal(hp) and "multiple of 64" in bf16s_refusal(dict(hp, gen=dict(hp["gen"], dim=96)))
    assert "3-channel" in bf16s_refusal(dict(O.default_hp(64, 2), input_dim_a=1, input_dim_b=1))
    small = G.merged_hp(O.default_hp, 64, dict(gen=dict(dim=64, n_res=1), dis=dict(dim=8, n_layer=1, num_scales=1)))
    try:
        for bad, msg in ((dict(batch_size=2048), "batch_size x crop_image_height x crop_image_width < 2\\^23"),
                         (dict(input_dim_a=1, input_dim_b=1), "3-channel images")):
            with pytest.raises(ValueError, match=msg):
                MUNIT_Trainer(dict(small, precision="bf16s", **bad))
    finally:
        ops.set_compute("f32")


def test_bf16s_layer_dtypes_follow_the_trainer():
    """The dtype rule of bf16s_generator_layers, pinned on default_hp(96)'s generator (call order: style encoder, content
    encoder, MLP, decoder)."""
    hp = O.default_hp(96)
    got = [(l[0], l[1], m[1], m[2]) for l, m in bf16s_generator_layers(hp["gen"], 3, False, (96, 96))]
    assert all(m[0] == BF16S_COMPUTE for _, m in bf16s_generator_layers(hp["gen"], 3, False, (96, 96)))
    assert got == BF16S_GENERATOR_96, got


# ------------------------------------------------------------------------------------------------------------------
# the frozen segmentation network
# ------------------------------------------------------------------------------------------------------------------
def seg_case(c, which):
    """Op-case tuple of pass `which` (0 forward, 1 backward-data) of a SEG_CONV_CASES entry (cin, cout, k, stride, pad,
    act, B, H, W): backward-data of a stride-2 odd kernel multiplies by the filter zero-extended to the next even size."""
    cin, cout, k, stride, pad, act, b, h, w = c
    if which == 0:
        return (cin, cout, k, stride, pad, "zero", 0, act, b, h, w)
    return (cin, cout, k + (k % 2 if stride == 2 else 0), stride, pad, "zero", 0, "none", b, h, w)


def seg_key(lib, case, which):
    """(pass, kernel name, cin, cout, filter, stride) of an op-case tuple"""
    return (which, kernel_names(lib, case)[which]) + case[:4]


def seg_production_cases():
    """{(pass, op case): label} of the frozen network over SEG_CROPS x (B, 2B images for B in BATCHES)."""
    from tests import seg_layers as SL
    cases = {}
    for crop in SEG_CROPS:
        for n in sorted({m * b for b in BATCHES for m in (1, 2)}):
            for l in SL.seg_layers(crop, n):
                label = "%s, crop %d, %d images" % (l.name, crop, n)
                cases.setdefault((0, l.case), label)
                cases.setdefault((1, SL.dgrad_case(l)), label)
    return cases


def seg_covered(lib, cases):
    return {seg_key(lib, seg_case(c, p), p) for c in cases for p in (0, 1)}


def seg_missing(lib, cases, prod):
    """`prod`: seg_production_cases(), built once by the caller (195 traces of the network)."""
    cov = seg_covered(lib, cases)
    missing = {}
    for (p, case), label in prod.items():
        key = seg_key(lib, case, p)
        if key not in cov:
            best = missing.get(key)
            if best is None or macs(case) < macs(best[0]):
                missing[key] = (case, label)
    return missing


def test_every_segmentation_conv_form_is_covered_by_a_segmentation_op_case(lib):
    from tests.test_gpu_semantic import SEG_CONV_CASES
    prod = seg_production_cases()
    assert len(prod) > 1000, len(prod)
    missing = seg_missing(lib, SEG_CONV_CASES, prod)
    assert not missing, ("kernel forms the frozen Resnet34_8s dispatches to that no SEG_CONV_CASES entry of the same "
                         "channels / filter / stride runs (cheapest layer of each):\n" + "\n".join(
                             "  %s %s: %s  (%s, %.2f GMAC)" % (PASSES[k[0]], k[1], c, lab, macs(c) / 1e9)
                             for k, (c, lab) in sorted(missing.items())))
    # the generator op cases alone leave the network's forms open (the LDS-patch fold backward-data of layer4 at crop 96
    # among them): the grid above is not vacuous
    open_ = seg_missing(lib, [], prod)
    assert any(k[:2] == (1, "conv_igemm_kernel<.., 2, 3> (LDS-patch fold)") and "crop 96" in lab and k[3] == 512
               for k, (c, lab) in open_.items()), sorted(open_)


def test_segmentation_cases_keep_their_kernels(lib):
    """Every SEG_CONV_CASES entry pins the (forward, backward-data) kernels it was added for."""
    from tests.test_gpu_semantic import SEG_CONV_CASES, SEG_CONV_CASES_TARGETS
    assert set(SEG_CONV_CASES_TARGETS) == set(SEG_CONV_CASES) and len(set(SEG_CONV_CASES)) == len(SEG_CONV_CASES)
    for c, want in SEG_CONV_CASES_TARGETS.items():
        got = tuple(kernel_names(lib, seg_case(c, p))[p] for p in (0, 1))
        assert got == want, (c, got, want)


def test_segmentation_layer_list_matches_the_state_dict():
    """One record per conv weight of the state dict (36 + fc), named after it, with the weight's shape; the stride-2 odd
    kernels carry the even backward-data filter; each block's first convolution takes the skip gradient as `add`, each
    downsample parks its dx."""
    from munit_amd.segmentation import Resnet34_8s
    from tests import seg_layers as SL
    with torch.device("meta"):
        sd = Resnet34_8s().state_dict()
    convs = {k[len("resnet34_8s."):-len(".weight")]: tuple(v.shape) for k, v in sd.items() if v.dim() == 4}
    assert len(convs) == 37
    for crop, n in ((64, 1), (96, 2), (512, 64)):
        layers, batches = SL.trace(crop, n)
        assert batches == [4 * n, 16 * n, 4 * n, n]
        assert len(layers) == 37 and len({l.name for l in layers}) == 37
        for l in layers:
            cin, cout, k, stride, pad, pt, ups, act, b, h, w = l.case
            key = l.name.replace(".downsample", ".downsample.0")
            assert convs[key] == (cout, cin, k, k), (l, convs[key])
            assert l.bias and pt == "zero" and not ups and h == w
            assert l.kd == (k + 1 if stride == 2 else k)
            assert l.add == (l.name.endswith(".conv1") and l.name != "conv1")
            assert l.parked == l.name.endswith(".downsample")
            assert act == ("relu" if l.name.endswith("conv1") else "none")
        by = {l.name: l.case for l in layers}
        assert by["conv1"][8:] == (n, crop, crop) and by["layer1.0.conv1"][8:] == (n, crop // 4, crop // 4)
        assert by["layer2.3.conv2"][8:] == (n, crop // 8, crop // 8)
        assert by["layer3.0.conv1"][8:] == (4 * n, crop // 16, crop // 16)
        assert by["layer4.2.conv2"][8:] == by["fc"][8:] == (16 * n, crop // 32, crop // 32)
        assert [l.name for l in layers if l.case[3] == 2] == ["conv1", "layer2.0.conv1", "layer2.0.downsample"]
