"""CPU (no GPU): the case lists of tests/dann_regimes.py reach every launch regime of dann.hip's batch norm that production
reaches, the restatement of the partition is self-consistent, the exact checks of tests/test_gpu_dann_regimes.py can tell
the three partition faults apart from the kernel as written, the workspace query is what the header states, and the
max-pool's documented NaN / tie rule is torch's own on whatever torch is installed.

Production batch-norm calls are listed by hooking tests/featda_oracle.batch_norm (the classifier's and the segmentation
head's oracles both call it) on `meta` tensors: the feature classifier at the crops of tests/test_cpu_dispatch.CROPS_256
its 16x16 average accepts and at BATCHES, the segmentation head at SEG_CROPS and BATCHES."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dann_regimes as R
from tests import featda_oracle as D
from tests import seghead_oracle as H
from tests.test_cpu_dispatch import BATCHES, CROPS_256, SEG_CROPS, _meta_state


# ----------------------------------------------------------------------------------------------------------------------
# (a) every reached regime is the regime of a case
# ----------------------------------------------------------------------------------------------------------------------
def _trace_bn(run):
    """Run oracle forward code on meta tensors; its batch-norm calls as (R, C)."""
    rec = []

    def record(sd, pre, x, *args, **kw):
        rec.append((x.shape[0] * x.shape[2] * x.shape[3], x.shape[1]))
        return x

    saved = D.batch_norm
    D.batch_norm = record
    try:
        run()
    finally:
        D.batch_norm = saved
    return rec


def classifier_crops():
    """The crops at which domainClassifier's 16x16 average is defined: the code (crop / 4) pooled twice is 16..31."""
    out = []
    for crop in CROPS_256:
        h, w = (crop, crop) if isinstance(crop, int) else crop
        if 16 <= h // 16 <= 31 and 16 <= w // 16 <= 31:
            out.append((h, w))
    return out


def production_calls():
    """{(R, C): first production call with that shape}"""
    calls = {}
    for h, w in classifier_crops():
        for b in BATCHES:
            code = torch.empty(b, 256, h // 4, w // 4, device="meta")
            for rc in _trace_bn(lambda: D.classifier(_meta_state(D.shapes()), code)):
                calls.setdefault(rc, "classifier %dx%d B=%d" % (h, w, b))
    for crop in SEG_CROPS:
        for b in BATCHES:
            code = torch.empty(b, 256, crop // 4, crop // 4, device="meta")
            for rc in _trace_bn(lambda: H.head(_meta_state(H.shapes()), code)):
                calls.setdefault(rc, "head %d B=%d" % (crop, b))
    return calls


def production_regimes(calls=None):
    """{regime: (R, C, label) of the smallest production call reaching it}"""
    out = {}
    for rc, label in sorted((calls or production_calls()).items()):
        out.setdefault(R.regime(*rc), rc + (label,))
    return out


@pytest.fixture(scope="module")
def prod():
    return production_regimes()


def uncovered(cases, prod):
    """Required regimes (production and edges) that no entry of `cases` runs, as text lines."""
    covered = {R.regime(*rc) for rc, _ in cases}
    missing = ["%s  (production: %s)" % (r, prod[r],) for r in prod if r not in covered]
    missing += ["%s  (edge: %s)" % (r, why) for r, why in R.BN_EDGES if r not in covered]
    return missing


def test_every_batchnorm_regime_is_covered_by_a_case(prod):
    edges = dict(R.BN_EDGES)
    assert len(edges) == len(R.BN_EDGES), "a regime listed twice in BN_EDGES"
    assert not set(edges) & set(prod), "BN_EDGES lists regimes production reaches: %s" % (set(edges) & set(prod))
    seen = {}
    for rc, why in R.BN_CASES:
        r = R.regime(*rc)
        assert r not in seen, "BN_CASES %s and %s share the regime %s: keep one" % (seen[r], rc, r)
        seen[r] = rc
    assert len({why for _, why in R.BN_CASES}) == len(R.BN_CASES), "two BN_CASES entries share a reason"
    missing = uncovered(R.BN_CASES, prod)
    assert not missing, "batch-norm regimes no kernel test runs:\n  " + "\n  ".join(missing)
    extra = [rc for rc, _ in R.BN_CASES if R.regime(*rc) not in prod and R.regime(*rc) not in edges]
    assert not extra, "BN_CASES whose regime is neither reached by production nor listed in BN_EDGES: %s" % extra


@pytest.mark.parametrize("i", range(len(R.BN_CASES)))
def test_dropping_a_case_names_the_regime_it_leaves_uncovered(prod, i):
    rc = R.BN_CASES[i][0]
    missing = uncovered(R.BN_CASES[:i] + R.BN_CASES[i + 1:], prod)
    assert len(missing) == 1 and missing[0].startswith(str(R.regime(*rc))), (rc, missing)


def test_production_reaches_the_cap_two_finishing_blocks_and_the_wrap():
    """The enumeration sees what the step runs: launches at the block cap, two finishing blocks, wrapped grids."""
    calls = production_calls()
    assert {c for _, c in calls} == {64, 128, 512}, sorted({c for _, c in calls})
    capped = [rc for rc in calls if R.bn_blocks(*rc) == R.BN_MAX_BLOCKS]
    wrapped = [rc for rc in calls if R.wraps(rc[0] * rc[1] // 4)]
    assert len(capped) > len(calls) // 2 and min(wrapped) == (36864, 512), (len(capped), len(calls), min(wrapped))
    assert (4 * 128 * 128, 512) in wrapped                     # the HD crop 512 at batch 4
    assert calls[(256, 512)] == "head 64 B=1" and calls[(5400, 128)] == "classifier 360x480 B=2"
    prod = production_regimes(calls)
    assert {r[2] for r in prod} == {"multi", "cap"} and {r[5] for r in prod} == {"one", "multi"}
    # what the four cases of test_gpu_featda.test_batchnorm_against_fp64 run: below the cap, one finishing block, no wrap
    old = {R.regime(*rc) for rc in ((7, 64), (2048, 64), (1024, 128), (2 * 31 * 31, 128))}
    assert all(r[2] != "cap" and r[5] == "one" and not r[6] for r in old)
    assert 2 <= min(R.bn_blocks(*rc) for rc in ((2048, 64), (1024, 128), (1922, 128))) and R.bn_blocks(1922, 128) == 31


def test_restatement_at_the_boundaries_the_cases_are_chosen_from():
    assert R.accepted_c() == [4, 8, 16, 32, 64, 128, 256, 512, 1024]
    assert [R.rl(c) for c in (4, 64, 128, 512, 1024)] == [256, 16, 8, 2, 1]
    assert [R.bn_blocks(r, 4) for r in (2, 2048, 2049)] == [1, 1, 2]
    assert [R.bn_blocks(r, 1024) for r in (8, 9, 512, 513)] == [1, 2, 64, 64]
    assert (R.per(513, 1024), R.holding_blocks(513, 1024)) == (9, 57)
    assert (R.per(1030, 512), R.holding_blocks(1030, 512), 1030 - 60 * 17) == (17, 61, 10)
    assert [R.bn_blocks(r, 64) for r in (8064, 8065, 8192, 8193)] == [63, 64, 64, 64] and R.per(8193, 64) == 129
    assert (R.per(5400, 128), 5400 - 63 * 85) == (85, 45)
    assert not R.wraps(16384 * 256) and R.wraps(16384 * 256 + 1)
    assert not R.wraps(16384 * 256) and R.wraps(16385 * 256) and 16385 * 256 == 4194560
    b, h, w, c = R.MAXPOOL_WRAP
    assert b * (h // 2) * (w // 2) * (c // 4) == 4326400 and R.wraps(4326400)
    b, h, w, c = R.AVG16_BWD_WRAP
    assert R.wraps(b * h * w * (c // 4))
    assert [R.finishing_blocks(c) for c in (4, 256, 512, 1024)] == [1, 1, 2, 4]
    assert R.grid_blocks(1) == 1 and R.grid_blocks(257) == 2 and R.grid_blocks(1 << 30) == 16384


# ----------------------------------------------------------------------------------------------------------------------
# (b), (c) the partition model
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", R.BN_SHAPES + R.BN_LARGE_MEAN, ids=str)
def test_every_row_is_visited_exactly_once(rc):
    r, c = rc
    v = R.visits(r, c)
    assert (v[:r] == 1).all() and (v[r:] == 0).all(), (rc, np.flatnonzero(v[:r] != 1)[:8], np.flatnonzero(v[r:])[:8])
    # the blocks are what `regime` says they are
    p, nb, hold = R.per(r, c), R.bn_blocks(r, c), R.holding_blocks(r, c)
    assert (hold - 1) * p < r <= hold * p and hold <= nb and nb * p >= r
    assert (R.regime(r, c)[3] == "absent") == (hold < nb)


@pytest.fixture(scope="module")
def lattice_sums():
    """{(R, C): (x as int64, exact column sums)} on the data the GPU file's exact checks use"""
    out = {}
    for r, c in R.BN_SHAPES:
        x = R.lattice_rows(r, c, 11).numpy().astype(np.int64)
        out[(r, c)] = (x, x.sum(0))
    return out


def test_the_faithful_model_gives_the_exact_column_sums(lattice_sums):
    for rc, (x, want) in lattice_sums.items():
        assert np.array_equal(R.model_column_sums(x), want), rc


@pytest.mark.parametrize("variant", [v for v in R.VARIANTS if v != "faithful"])
def test_a_partition_fault_changes_the_integer_column_sums(lattice_sums, variant):
    """Each fault changes the column sums of every case it affects structurally, and it affects at least one: the exact
    checks of tests/test_gpu_dann_regimes.py (dbeta == dy.sum(0), the two-float mean) are sensitive to it."""
    affected = [rc for rc in R.BN_SHAPES if R.structurally_affected(rc[0], rc[1], variant)]
    want = {"last_block_dropped": set(R.BN_SHAPES),
            "empty_blocks_read": {rc for rc in R.BN_SHAPES if R.regime(*rc)[3] == "absent"},
            "cap_ignored": {rc for rc in R.BN_SHAPES if -(-rc[0] // (8 * R.rl(rc[1]))) > R.BN_MAX_BLOCKS}}[variant]
    assert set(affected) == want and affected, (variant, affected)
    for rc in affected:
        x, exact = lattice_sums[rc]
        got = R.model_column_sums(x, variant)
        assert (got != exact).any(), "%s goes unnoticed at %s" % (variant, rc)
        print(variant, rc, "%d of %d column sums differ" % (int((got != exact).sum()), rc[1]))
    for rc in set(R.BN_SHAPES) - set(affected):
        x, exact = lattice_sums[rc]
        assert np.array_equal(R.model_column_sums(x, variant), exact), (variant, rc)


# ----------------------------------------------------------------------------------------------------------------------
# (d) the workspace query
# ----------------------------------------------------------------------------------------------------------------------
def test_workspace_bytes_is_what_the_header_states():
    from munit_amd import _lib
    lib = _lib.load()
    for c in R.accepted_c():
        want = R.align256(64 * 2 * c * 4) + R.align256(2 * c * 4)
        assert lib.munit_batchnorm_workspace_bytes(c) == want == R.workspace_bytes(c), (c, want)
        # room for the backward's 64 x 2 x C partials, then the 2 C sums
        assert R.part_bytes(c) >= R.BN_MAX_BLOCKS * 2 * c * 4
    assert lib.munit_batchnorm_workspace_bytes(0) == 0 and lib.munit_batchnorm_workspace_bytes(-4) == 0


# ----------------------------------------------------------------------------------------------------------------------
# (e) the max-pool reference
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_torch_max_pool_follows_the_documented_rule_on_special_values(dtype):
    """All 2401 windows over {NaN, -inf, +inf, -0, +0, 1, -1}: value (bitwise: NaN-ness and the sign of zero), index and
    autograd gradient of F.max_pool2d against maxpool_rule -- the reference of the GPU test is known good here."""
    npdt = np.float64 if dtype == torch.float64 else np.float32
    bits = torch.int64 if dtype == torch.float64 else torch.int32
    win = R.special_windows(npdt)
    assert win.shape == (2401, 4) and len({tuple(w.view(np.uint64 if npdt == np.float64 else np.uint32)) for w in win}) == 2401
    dy = np.arange(1, 2402).astype(npdt)
    val, idx, dx = R.maxpool_rule(win, dy)
    x = torch.from_numpy(win.copy()).reshape(2401, 1, 2, 2).requires_grad_(True)
    y, ind = F.max_pool2d(x, 2, return_indices=True)
    (g,) = torch.autograd.grad(y, [x], torch.from_numpy(dy).reshape(2401, 1, 1, 1))
    bad_v = torch.from_numpy(val).view(bits) != y.detach().reshape(-1).view(bits)
    bad_i = torch.from_numpy(idx) != ind.reshape(-1)
    bad_g = torch.from_numpy(dx).view(bits) != g.reshape(2401, 4).view(bits)
    n_bad = int(bad_v.sum()) + int(bad_i.sum()) + int(bad_g.any(1).sum())
    print("max_pool2d %s against the rule: %d disagreements" % (dtype, n_bad))
    assert n_bad == 0, (win[bad_v.numpy()][:4], win[bad_i.numpy()][:4], win[bad_g.any(1).numpy()][:4])
    # the rule's corners, spelled out
    nan, inf = float("nan"), float("inf")
    v, i, _ = R.maxpool_rule(np.array([[nan, 1, nan, inf], [-0.0, 0.0, -0.0, 0.0], [0.0, -0.0, 0.0, -0.0], [1, nan, inf, -1],
                                       [-inf, -inf, -inf, -inf]], dtype=npdt), np.ones(5, dtype=npdt))
    assert list(i) == [2, 0, 0, 1, 0] and np.isnan(v[0]) and np.isnan(v[3])
    assert np.signbit(v[1]) and not np.signbit(v[2]) and v[4] == -inf
