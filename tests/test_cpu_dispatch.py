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
# reachable only with a MUNIT_DEBUG_* switch set (MUNIT_DEBUG_NO_WGRAD_PK): the op tests never force a debug fallback
DEBUG_ONLY = {"conv_lanes_wgrad_kernel"}
SEG_CROPS = tuple(range(64, 513, 32))


@pytest.fixture(scope="module")
def lib():
    from munit_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------------
# layer enumeration
# ------------------------------------------------------------------------------------------------------------------
def _trace(run):
    """Run `run()` (oracle forward code on meta tensors) and return the conv layers it calls, in call order, as
    (cin, cout, k, stride, pad, pad_type, upsample, act, H, W) at the batch of its input.  H, W are the layer's INPUT
    extent before the fused nearest x2 (what munit_conv_desc holds); act is what the device fuses into the conv (none
    when a norm follows: the norm kernels carry the activation then)."""
    rec = []
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
            return out(x, cout, k, stride, 0)

        def linear(self, x, w, b=None):
            n, k = w.shape
            rec.append((k, n, 1, 1, 0, "zero", 0, "none", 1, 1))
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


def _desc(case, which):
    """munit_conv_desc of an op case (cin, cout, k, stride, pad, pad_type, ups, act, B, H, W) for pass `which`: fp32
    tensors and arithmetic; the activation is fused into the forward only (as munit_amd.ops plans the three passes)."""
    from munit_amd._lib import ACT, PAD, ConvDesc
    cin, cout, k, stride, pad, pt, ups, act, b, h, w = case
    return ConvDesc(b, h, w, cin, cout, k, k, stride, pad, PAD[pt], int(ups), ACT[act if which == 0 else "none"], 0.2, 0, 0, 0)


def kernel_names(lib, case):
    import ctypes
    return tuple(lib.munit_conv2d_kernel_name(ctypes.byref(_desc(case, p)), p).decode() for p in range(3))


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


def test_every_dispatch_branch_is_covered_by_an_op_test(lib):
    lits = dispatch_literals()
    assert len(lits) >= 25, lits
    assert DEBUG_ONLY <= set(lits), DEBUG_ONLY
    names = {n for _, n in covered(lib)}
    missing = [n for n in lits if n not in names and n not in DEBUG_ONLY]
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
