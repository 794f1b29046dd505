"""CPU (no GPU): munit_instnorm_route against a Python restatement of norm.hip's choice between the flat kernels, the
channel-sliced pair and the one-pass forward (onepass_split): fp32, C % 64 == 0, at most 16 splits of at most 256 pixels.

Asked for every instance-norm / AdaIN call of the step -- tests/geometries.ALL, config_256 at the crops and batches of
tests/test_cpu_dispatch.py, fp32 and bf16 storage -- and for the neighbours on both sides of every bound of the rule.  The
restatement is pinned to the launches by tests/test_gpu_norm_onepass.py (the routes of its cases, and the bits they give) and
by the split partials tests/test_gpu_ops.py::test_norm_entry_point_contract counts."""
import os
import re

import pytest

from munit_amd import _lib
from oracle import munit_oracle as O
from tests import geometries as G
from tests.test_cpu_dispatch import BATCHES, CROPS_256
from tests.test_cpu_norm_regimes import MAX_NORM_C, SLICE, network_norms, nsplit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAT, SLICED, ONEPASS = 0, 1, 2
OP_MAX_SPLIT = 16      # splits (waves) of a one-pass block
OP_MAX_PER = 16 * 16   # pixels of a split: 16 pixel lanes x 16 float4 registers per thread


def env_flag(name):
    return os.environ.get(name) is not None      # norm.hip: getenv(name) != nullptr, read once per process


def route(B, HW, C, dtype):
    if B <= 0 or HW <= 0 or C <= 0 or C % 4 or C > MAX_NORM_C:
        return -1
    if C % SLICE or env_flag("MUNIT_DEBUG_NO_SLICED_NORM"):
        return FLAT
    ns = nsplit("in", B, HW, C)
    per = -(-HW // ns)
    if dtype == "f32" and ns <= OP_MAX_SPLIT and per <= OP_MAX_PER and not env_flag("MUNIT_DEBUG_NO_ONEPASS_NORM"):
        return ONEPASS
    return SLICED


def lib_route(B, HW, C, dtype):
    return _lib.load().munit_instnorm_route(B, HW, C, _lib.DTYPE[dtype])


def step_calls():
    """{(B, HW, C)} of the instance-norm / AdaIN calls of the configurations the suite runs."""
    grid = [(G.merged_hp(O.default_hp, size, over), (G.BATCH,)) for _, size, over in G.ALL]
    grid += [(O.default_hp(c), BATCHES) for c in CROPS_256]
    out = set()
    for hp, batches in grid:
        for (kind, hw, c), (mult, _) in network_norms(hp).items():
            if kind != "ln":
                out.update((b * m, hw, c) for b in batches for m in mult)
    return sorted(out)


def test_route_of_every_norm_call_of_the_step():
    calls = step_calls()
    seen = set()
    for B, HW, C in calls:
        for dt in ("f32", "bf16"):
            want = route(B, HW, C, dt)
            assert lib_route(B, HW, C, dt) == want, (B, HW, C, dt, want)
            seen.add((dt, want))
    if not env_flag("MUNIT_DEBUG_NO_ONEPASS_NORM") and not env_flag("MUNIT_DEBUG_NO_SLICED_NORM"):
        assert seen == {("f32", FLAT), ("f32", SLICED), ("f32", ONEPASS), ("bf16", FLAT), ("bf16", SLICED)}, seen
        # the workload's own launch: the residual trunk of config_256 at 256 x 256, batch 8 -- and what stays two-pass
        assert lib_route(8, 64 * 64, 256, "f32") == ONEPASS
        assert lib_route(8, 128 * 128, 128, "f32") == SLICED and lib_route(8, 256 * 256, 64, "f32") == SLICED
        assert lib_route(8, 128 * 128, 256, "f32") == SLICED      # config_HD's trunk: planes above 4096 pixels


# (B, C, H, W): ns splits of per pixels
NEIGHBOURS = [
    ((2, 64, 8, 8), 1, 64, ONEPASS), ((2, 256, 16, 16), 1, 256, ONEPASS), ((1, 128, 87, 3), 2, 131, ONEPASS),
    ((1, 128, 20, 32), 5, 128, ONEPASS), ((3, 192, 32, 32), 5, 205, ONEPASS), ((8, 256, 48, 48), 9, 256, ONEPASS),
    ((8, 256, 64, 64), 16, 256, ONEPASS),
    ((1, 64, 64, 64), 64, 64, SLICED), ((1, 320, 24, 32), 2, 384, SLICED), ((8, 256, 24, 24), 2, 288, SLICED),
    ((2, 192, 64, 64), 21, 196, SLICED), ((2, 48, 16, 16), 4, 64, FLAT),
    # one step across each bound: 17 splits; 257 pixels in the one split a plane of 257 has; C = 60 and 68 around a slice
    ((1, 64, 64, 17), 17, 64, SLICED), ((1, 64, 64, 16), 16, 64, ONEPASS),
    ((1, 64, 257, 1), 4, 65, ONEPASS), ((4, 1024, 257, 1), 1, 257, SLICED), ((4, 1024, 256, 1), 1, 256, ONEPASS),
    ((2, 60, 8, 8), 1, 64, FLAT), ((2, 68, 8, 8), 1, 64, FLAT), ((1, 1024, 16, 16), 1, 256, ONEPASS),
    ((2, 64, 1, 1), 1, 1, ONEPASS), ((32, 128, 32, 32), 8, 128, ONEPASS),
]


@pytest.mark.parametrize("shape,ns,per,want", NEIGHBOURS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_route_at_the_bounds_of_the_rule(shape, ns, per, want):
    B, C, H, W = shape
    HW = H * W
    got_ns = nsplit("in", B, HW, C)
    assert (got_ns, -(-HW // got_ns)) == (ns, per), (shape, got_ns, -(-HW // got_ns))
    if env_flag("MUNIT_DEBUG_NO_ONEPASS_NORM") or env_flag("MUNIT_DEBUG_NO_SLICED_NORM"):
        want = route(B, HW, C, "f32")
    assert route(B, HW, C, "f32") == want and lib_route(B, HW, C, "f32") == want, (shape, route(B, HW, C, "f32"))
    assert lib_route(B, HW, C, "bf16") == min(want, SLICED) == route(B, HW, C, "bf16")


def test_route_refuses_what_the_entry_points_refuse():
    for B, HW, C in [(0, 64, 64), (2, 0, 64), (2, 64, 0), (2, 64, 6), (2, 64, MAX_NORM_C + 4), (-1, 64, 64)]:
        assert lib_route(B, HW, C, "f32") == -1 == route(B, HW, C, "f32"), (B, HW, C)


def test_query_is_declared_in_header_and_signatures():
    header = open(os.path.join(ROOT, "include", "munit_hip.h")).read()
    m = re.search(r"\bint\s+munit_instnorm_route\s*\(([^)]*)\)\s*;", header)
    assert m, "munit_instnorm_route is not declared in include/munit_hip.h"
    assert [a.split()[0] for a in m.group(1).split(",")] == ["int"] * 4, m.group(1)
    restype, argtypes = _lib.SIGNATURES["munit_instnorm_route"]
    from ctypes import c_int
    assert restype is c_int and list(argtypes) == [c_int] * 4
    assert hasattr(_lib.load(), "munit_instnorm_route")
