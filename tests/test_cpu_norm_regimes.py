"""CPU (no GPU): every regime of the normalisation kernels' split logic that a training step reaches is run by an fp64 op
test.

norm.hip cuts each instance-norm / AdaIN / LayerNorm pass into pixel splits (pick_split, sliced_split) and lays a block
over channel quads and pixel lanes (make_lay); the statistics are folded over the splits by fold_partials / fold_slice or
ln_finish.  `regime` restates that choice in Python.  This file lists every norm call of the step (the oracle's
generators and discriminators on `meta` tensors, with hooks on O.instance_norm / O.adain / O.munit_layer_norm, for every
geometry of tests/geometries.ALL and for configs/config_256.yaml at the crops and batches of tests/test_cpu_dispatch.py;
bf16 storage for config #3's generator, 256x256 batch 32), maps each call to its regime and requires every regime so
reached, plus the edge regimes of EDGES, to be the regime of a case of tests/test_gpu_ops.py::NORM_CASES.  Every case has
a regime of its own, so dropping a case fails here with the regime it leaves uncovered.  The restatement is pinned to the
library by the contract tests (tests/kernel_contract.py): the number of split partials a launch leaves in its NaN-poisoned
workspace is B * nsplit(...) * 2 * C (instance norm, LayerNorm backward) or B * nsplit(...) * 2 (LayerNorm forward)."""
import pytest
import torch

from oracle import munit_oracle as O
from tests import geometries as G
from tests.test_cpu_dispatch import BATCHES, CROPS_256, _meta_state

NT = 256
MAX_SPLIT = 64
SLICE = 64
MAX_NORM_C = 4 * NT


def pick_split(B, HW):
    s = max(1, min(MAX_SPLIT, 2048 // max(1, B)))
    return min(s, max(1, HW // 64))


def sliced(kind, C):
    return kind != "ln" and C % SLICE == 0


def nsplit(kind, B, HW, C):
    """Pixel splits of a pass: norm.hip's pick_split, or sliced_split on the channel-sliced instance-norm path."""
    s = pick_split(B, HW)
    return max(1, s // (C // SLICE)) if sliced(kind, C) else s


def regime(kind, dtype, B, HW, C):
    """(path, dtype, splits, short last split, lanes, ragged fold) of one norm pass.
    path: ln | in_sliced | in_flat (instance norm and AdaIN run the same kernels).  splits: one | multi | cap (nsplit 1,
    between, MAX_SPLIT).  short: the last split holds fewer pixels (LayerNorm: channel quads) than the others.  lanes:
    in_sliced -- 1slice (C = 64), trunc (pick_split not a multiple of the C / 64 slices) or even; otherwise 1quad (C = 4:
    one quad, 256 pixel lanes), idle (256 not a multiple of C / 4: threads with no pixel lane) or full.  ragged: the four
    split groups of the fold add unequal numbers of splits (nsplit > 4, not a multiple of 4)."""
    assert C % 4 == 0 and C <= MAX_NORM_C, C
    ns = nsplit(kind, B, HW, C)
    n = HW * C // 4 if kind == "ln" else HW
    per = -(-n // ns)
    splits = "one" if ns == 1 else "cap" if ns == MAX_SPLIT else "multi"
    if sliced(kind, C):
        slices = C // SLICE
        lanes = "1slice" if slices == 1 else "trunc" if pick_split(B, HW) % slices else "even"
    else:
        cq = C // 4
        lanes = "1quad" if cq == 1 else "idle" if NT % cq else "full"
    path = "ln" if kind == "ln" else "in_sliced" if sliced(kind, C) else "in_flat"
    return (path, dtype, splits, per * ns > n, lanes, ns > 4 and ns % 4 != 0)


def partial_doubles(kind, B, HW, C, backward):
    """Split partials a pass leaves at the front of its workspace: [b][split][2][C] doubles, or [b][split][2] for the
    LayerNorm forward."""
    ns = nsplit(kind, B, HW, C)
    return B * ns * 2 * (1 if (kind == "ln" and not backward) else C)


# regimes no configuration reaches that the op tests must still run, as (regime, why)
EDGES = [
    (("in_flat", "f32", "one", False, "idle", False), "C = 12: QB = 3, lanes that idle; HW = 127, the last one-split extent"),
    (("in_flat", "f32", "multi", False, "1quad", False), "C = 4: one quad, 256 pixel lanes; HW = 128, two splits"),
    (("in_flat", "f32", "multi", True, "idle", False), "C = 68: a partial second fold block; HW = 129, a short last split"),
    (("in_flat", "f32", "multi", True, "idle", True), "B = 33: 2048 / B not a power of two, 62 splits"),
    (("in_flat", "f32", "multi", False, "idle", False), "C = 1020: the largest non-sliced C, 255 quads, one pixel lane"),
    (("in_sliced", "f32", "multi", True, "trunc", True), "C = 192: 64 splits shared out over 3 slices"),
    (("ln", "f32", "one", False, "1quad", False), "HW * C = 8: the smallest unbiased count"),
    (("ln", "f32", "cap", False, "idle", False), "B * nsplit = 576 > 256 partial rows in ln_bwd_param_kernel"),
    (("ln", "f32", "one", False, "idle", False), "C = 1020 in ln_bwd_stats: 255 quads"),
    (("in_flat", "bf16", "multi", True, "idle", True), "the non-sliced path in bf16 storage"),
    (("ln", "bf16", "cap", False, "idle", False), "LayerNorm in bf16 storage with idle lanes"),
]


# ------------------------------------------------------------------------------------------------------------------
# norm calls of the step
# ------------------------------------------------------------------------------------------------------------------
def _trace_norms(run):
    """Run `run()` (oracle forward code on meta tensors) and return its norm calls as (kind, HW, C) at the batch of the
    input."""
    rec = []

    def out(x, cout, k, stride, pad):
        b, _, h, w = x.shape
        return x.new_empty(b, cout, (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1)

    def conv_block(x, w, b, stride, pad, pad_type, norm_fn=None, activ="none"):
        y = out(x, w.shape[0], w.shape[2], stride, pad)
        return norm_fn(y) if norm_fn is not None else y

    def record(kind):
        def f(x, *args):
            rec.append((kind, x.shape[2] * x.shape[3], x.shape[1]))
            return x
        return f

    saved = O.conv_block, O.instance_norm, O.adain, O.munit_layer_norm
    O.conv_block, O.instance_norm, O.adain, O.munit_layer_norm = conv_block, record("in"), record("adain"), record("ln")
    try:
        run()
    finally:
        O.conv_block, O.instance_norm, O.adain, O.munit_layer_norm = saved
    return rec


def network_norms(hp):
    """{(kind, HW, C): (batch multipliers, in the generator)} of one config: generators at the step's batch,
    discriminators at 2B and B (see tests/test_cpu_dispatch.network_layers)."""
    size = (hp["crop_image_height"], hp["crop_image_width"])
    calls = {}
    for input_dim in sorted({hp["input_dim_a"], hp["input_dim_b"]}):
        x = torch.empty(1, input_dim, *size, device="meta")
        for double in (True, False):
            g = O.GenView(_meta_state(O.gen_param_shapes(hp["gen"], input_dim, double)), hp["gen"], double)

            def gen():
                c, s = g.encode(x, 1 if double else None)
                g.decode(c, s, 1 if double else None)
            for c in _trace_norms(gen):
                calls.setdefault(c, (set(), True))[0].add(1)
        sd = _meta_state(O.dis_param_shapes(hp["dis"], input_dim))
        for c in _trace_norms(lambda: O.dis_forward(sd, "", x, hp["dis"])):
            calls.setdefault(c, (set(), False))[0].update((1, 2))
    return calls


def production_regimes():
    """{regime: first (config, kind, B, HW, C) reaching it}: fp32 over tests/geometries.ALL (batch 2) and config_256 at
    CROPS_256 x BATCHES; bf16 storage over config #3's generator (256x256, batch 32)."""
    grid = [(name, G.merged_hp(O.default_hp, size, over), (G.BATCH,)) for name, size, over in G.ALL]
    grid += [("config_256 %s" % (c if isinstance(c, int) else "%dx%d" % c), O.default_hp(c), BATCHES) for c in CROPS_256]
    out = {}
    for label, hp, batches in grid:
        for (kind, hw, c), (mult, _) in network_norms(hp).items():
            for b in batches:
                for m in sorted(mult):
                    out.setdefault(regime(kind, "f32", b * m, hw, c), (label, kind, b * m, hw, c))
    for (kind, hw, c), (mult, in_gen) in network_norms(O.default_hp(256)).items():
        if in_gen:
            out.setdefault(regime(kind, "bf16", 32, hw, c), ("config #3 bf16s", kind, 32, hw, c))
    return out


def case_regimes():
    from tests.test_gpu_ops import NORM_CASES
    return [(regime(kind, dt, B, H * W, C), (kind, dt, B, C, H, W)) for kind, dt, B, C, H, W in NORM_CASES]


def test_every_norm_regime_is_covered_by_an_op_test():
    prod = production_regimes()
    edges = dict(EDGES)
    assert len(edges) == len(EDGES), "a regime listed twice in EDGES"
    cases = case_regimes()
    covered = {}
    for r, c in cases:
        assert r not in covered, "NORM_CASES %s and %s share the regime %s: keep one" % (covered[r], c, r)
        covered[r] = c
    missing = ["  %s  (production: %s)" % (r, prod[r]) for r in prod if r not in covered]
    missing += ["  %s  (edge: %s)" % (r, why) for r, why in EDGES if r not in covered]
    assert not missing, "norm regimes no op test runs:\n" + "\n".join(missing)
    extra = [c for r, c in cases if r not in prod and r not in edges]
    assert not extra, "NORM_CASES whose regime is neither reached by production nor listed in EDGES: %s" % extra


def test_production_reaches_the_main_regimes():
    """The enumeration sees what the step runs: the three paths, fp32 and bf16, at the split cap and below it."""
    prod = production_regimes()
    assert {r[0] for r in prod} == {"ln", "in_sliced", "in_flat"}, sorted(prod)
    assert {r[2] for r in prod} == {"one", "multi", "cap"}, sorted(prod)
    assert any(r[1] == "bf16" for r in prod)
    # config #3's generator: content encoder 64 / 128 / 256 channels at 256 / 128 / 64 pixels, AdaIN trunk, LN decoder
    calls = network_norms(O.default_hp(256))
    assert {(k, c) for (k, hw, c), (m, g) in calls.items() if g} == {("in", 64), ("in", 128), ("in", 256), ("adain", 256),
                                                                       ("ln", 128), ("ln", 64)}, calls


def test_regime_restatement_edges():
    """pick_split / sliced_split at the boundaries the op cases are chosen from."""
    assert [nsplit("in", 2, hw, 4) for hw in (1, 64, 127, 128, 129)] == [1, 1, 1, 2, 2]
    assert nsplit("in", 1, 4096, 64) == 64 and nsplit("in", 1, 1 << 20, 4) == 64
    assert nsplit("in", 33, 4096, 12) == 62
    assert nsplit("in", 2, 4096, 192) == 21 and nsplit("in", 1, 1600, 320) == 5
    assert nsplit("in", 32, 4096, 256) == 16
    assert regime("in", "f32", 2, 129, 68)[3] and not regime("in", "f32", 2, 128, 68)[3]


@pytest.mark.parametrize("C", [1028, 2048, 4096])
def test_norm_entry_points_refuse_more_than_1024_channels(C):
    """Past 1024 channels (256 quads) the quad loops of in_stats / in_bwd_stats (non-sliced) and ln_bwd_stats would run a
    thread-dependent number of times around a __syncthreads(): the entry points refuse such C before launching anything
    (the pointers are never dereferenced)."""
    from ctypes import c_float, c_size_t, c_void_p
    from munit_amd import _lib
    lib = _lib.load()
    p = c_void_p(0x1000)
    big = c_size_t(1 << 40)
    calls = [
        lib.munit_instnorm_fwd(p, p, p, 2, 64, C, None, 0, 0, 0, None, 0, c_float(1e-5), p, big, None),
        lib.munit_instnorm_bwd(p, p, p, p, 2, 64, C, None, None, 0, 0, 0, 0, p, big, None),
        lib.munit_instnorm_fwd_bf16(p, p, p, 2, 64, C, None, 0, 0, 0, None, 0, c_float(1e-5), p, big, None),
        lib.munit_instnorm_bwd_bf16(p, p, p, p, 2, 64, C, None, None, 0, 0, 0, 0, p, big, None),
        lib.munit_layernorm_fwd(p, p, p, 2, 64, C, p, p, 0, c_float(1e-5), p, big, None),
        lib.munit_layernorm_bwd(p, p, p, p, 2, 64, C, p, p, p, p, c_float(0.0), 0, c_float(1e-5), p, big, None),
        lib.munit_layernorm_fwd_bf16(p, p, p, 2, 64, C, p, p, 0, c_float(1e-5), p, big, None),
        lib.munit_layernorm_bwd_bf16(p, p, p, p, 2, 64, C, p, p, p, p, c_float(0.0), 0, c_float(1e-5), p, big, None),
    ]
    assert calls == [-1] * len(calls), calls
