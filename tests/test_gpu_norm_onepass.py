"""GPU: the one-pass instance-norm / AdaIN route (norm.hip: in_onepass_kernel, in_bwd_onepass_kernel) gives the bits of the
two-pass kernels it replaces.

One child process per route -- the library's default, and MUNIT_DEBUG_NO_ONEPASS_NORM=1, which the library reads once per
process -- runs every case of CASES through munit_amd.ops (instance norm and AdaIN; no activation, ReLU, LeakyReLU, tanh; a
residual with no activation, as the ResBlocks pair them) and saves y, stats, dx and d_adain as .npy.  The parent compares the
two sets bit for bit.  Each child also records munit_instnorm_route for its cases: the shapes aimed at the one-pass route
reach it, their neighbours across each eligibility bound (splits, pixels per split, C % 64, fp32) do not, and both still
match."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

# (dtype, B, C, H, W, route by default): ns = splits, per = pixels of a split (tests/test_cpu_norm_route.py restates them)
CASES = [
    ("f32", 2, 64, 8, 8, 2),       # ns 1, per 64: one wave, 4 values per thread
    ("f32", 2, 256, 16, 16, 2),    # ns 1, per 256: all 16 values of a thread
    ("f32", 1, 128, 87, 3, 2),     # ns 2, per 131: a last split of 130, ragged pixel lanes
    ("f32", 1, 128, 20, 32, 2),    # ns 5, per 128: fold groups of 2, 1, 1, 1 splits
    ("f32", 3, 192, 32, 32, 2),    # ns 5, per 205: a last split of 204, three slices, odd batch
    ("f32", 8, 256, 48, 48, 2),    # ns 9, per 256: 576 threads
    ("f32", 8, 256, 64, 64, 2),    # ns 16, per 256: the residual trunk's own launch, 1024 threads
    ("f32", 1, 64, 64, 64, 1),     # ns 64: too many splits for one block
    ("f32", 1, 320, 24, 32, 1),    # per 384
    ("f32", 8, 256, 24, 24, 1),    # per 288
    ("f32", 2, 192, 64, 64, 1),    # ns 21
    ("f32", 2, 48, 16, 16, 0),     # C % 64 != 0: the flat kernels
    ("bf16", 2, 64, 16, 16, 1),    # bf16 storage keeps the sliced kernels
]
VARIANTS = [(kind, act, res) for kind in ("in", "adain")
            for act, res in (("none", False), ("none", True), ("relu", False), ("lrelu", False), ("tanh", False))]
TENSORS = ("y", "stats", "dx", "d_adain")


def _cid(case):
    return "%s_%dx%dx%dx%d" % case[:5]


def _vid(v):
    return "%s_%s%s" % (v[0], v[1], "_res" if v[2] else "")


def _inputs(case, device):
    """x, residual, dy as channels_last tensors of the case's dtype and the (B, 2C + 11) AdaIN parameter block; the same in
    every process (CPU generator)."""
    dt, B, C, H, W, _ = case
    g = torch.Generator().manual_seed(1000 + 7 * B + C + 31 * H + W)
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32

    def t(scale, shift=0.0):
        v = torch.randn(B, C, H, W, generator=g) * scale + shift
        return v.to(tdt).to(device).contiguous(memory_format=torch.channels_last)
    x, res, dy = t(1.5, 0.25), t(1.0), t(1.0)
    ad = (torch.randn(B, 2 * C + 11, generator=g) + 0.5).to(device)
    return x, res, dy, ad


def _run(case, variant, x, res, dy, ad):
    """One forward and backward through munit_amd.ops; {tensor name: torch tensor}."""
    from munit_amd import ops
    kind, act, with_res = variant
    C = case[2]
    xr = x.clone().requires_grad_(True)
    captured = {}
    if kind == "adain":
        adr = ad.clone().requires_grad_(True)
        y = ops.adain(xr, adr, C + 7, 3, relu=act, residual=res if with_res else None)
    else:
        adr = None
        y = ops.instance_norm(xr, relu=act, residual=res if with_res else None)
    stats = y.grad_fn.saved_tensors[1]
    y.backward(dy)
    captured["y"], captured["stats"], captured["dx"] = y.detach(), stats.detach(), xr.grad
    captured["d_adain"] = adr.grad if adr is not None else torch.zeros(1, device=x.device)
    return captured


def _np(t):
    t = t.detach().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return t.cpu().numpy()


def _child(out):
    from munit_amd import _lib
    lib = _lib.load()
    device = torch.device("cuda:0")
    routes = {}
    for case in CASES:
        dt, B, C, H, W, _ = case
        routes[_cid(case)] = lib.munit_instnorm_route(B, H * W, C, _lib.DTYPE[dt])
        x, res, dy, ad = _inputs(case, device)
        for v in VARIANTS:
            got = _run(case, v, x, res, dy, ad)
            for name in TENSORS:
                np.save(os.path.join(out, "%s.%s.%s.npy" % (_cid(case), _vid(v), name)), _np(got[name]))
    torch.cuda.synchronize()
    with open(os.path.join(out, "routes.json"), "w") as f:
        json.dump(routes, f)
    print("norm routes ok")


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    """{"onepass" | "twopass": directory of the child's .npy files and routes.json}; removed after the module."""
    base = tmp_path_factory.mktemp("norm_onepass")
    dirs = {}
    for tag, debug in (("onepass", False), ("twopass", True)):
        d = base / tag
        d.mkdir()
        env = {k: v for k, v in os.environ.items() if k != "MUNIT_DEBUG_NO_ONEPASS_NORM"}
        if debug:
            env["MUNIT_DEBUG_NO_ONEPASS_NORM"] = "1"
        # 130 forward + backward pairs of at most 8 x 256 x 64 x 64 and their files: seconds; the limit covers a cold start of
        # the runtime many times over
        p = subprocess.run([sys.executable, os.path.abspath(__file__), str(d)], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, cwd=ROOT, env=env, timeout=300)
        out = p.stdout.decode()
        assert p.returncode == 0 and out.strip().endswith("norm routes ok"), out[-3000:]
        dirs[tag] = str(d)
    yield dirs
    shutil.rmtree(str(base), ignore_errors=True)


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_case_reaches_the_route_it_aims_at(routes, case):
    want = case[5]
    got = {tag: json.load(open(os.path.join(d, "routes.json")))[_cid(case)] for tag, d in routes.items()}
    assert got["onepass"] == want, (case, got)
    assert got["twopass"] == min(want, 1), (case, got)


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_one_pass_is_bitwise_the_two_pass_route(routes, case):
    bad = []
    for v in VARIANTS:
        for name in TENSORS:
            f = "%s.%s.%s.npy" % (_cid(case), _vid(v), name)
            a, b = np.load(os.path.join(routes["onepass"], f)), np.load(os.path.join(routes["twopass"], f))
            assert a.shape == b.shape and a.dtype == b.dtype and a.size > 0, f
            bits = np.int16 if a.dtype.itemsize == 2 else np.int32
            ai, bi = a.view(bits), b.view(bits)
            if not np.array_equal(ai, bi):
                bad.append((f, int((ai != bi).sum()), a.size))
            if a.dtype == np.float32:
                assert np.isfinite(a).all(), f
    assert not bad, "tensors that differ between the routes (file, differing elements, elements): %s" % bad


@pytest.mark.parametrize("case", [c for c in CASES if c[5] == 2], ids=_cid)
def test_relu_backward_takes_the_forwards_branch_exactly(case):
    """dy is zero wherever the forward's ReLU passed (y > 0) and 1 where it cut: if the backward re-evaluates the branch the
    forward took, g = dy * relu' is zero everywhere, and dx and d_adain are exactly zero."""
    from munit_amd import _lib, ops
    dt, B, C, H, W, route = case
    assert _lib.load().munit_instnorm_route(B, H * W, C, _lib.DTYPE[dt]) == route
    device = torch.device("cuda:0")
    x, _, _, ad = _inputs(case, device)
    for kind in ("in", "adain"):
        xr = x.clone().requires_grad_(True)
        adr = ad.clone().requires_grad_(True)
        y = ops.adain(xr, adr, C + 7, 3, relu="relu") if kind == "adain" else ops.instance_norm(xr, relu="relu")
        passed = y.detach() > 0
        assert 0 < int(passed.sum()) < y.numel()
        y.backward((~passed).to(y.dtype))
        assert int(torch.count_nonzero(xr.grad)) == 0, (case, kind)
        if kind == "adain":
            own = adr.grad[:, C + 7:2 * C + 7], adr.grad[:, 3:C + 3]
            assert all(int(torch.count_nonzero(t)) == 0 for t in own), (case, kind)


@pytest.mark.parametrize("case", [c for c in CASES if c[5] == 2], ids=_cid)
def test_forward_without_grad_gives_the_same_output(case):
    from munit_amd import ops
    C = case[2]
    x, res, _, ad = _inputs(case, torch.device("cuda:0"))
    for act, r in (("none", res), ("relu", None)):
        want = ops.adain(x.clone().requires_grad_(True), ad, C + 7, 3, relu=act, residual=r).detach()
        with torch.no_grad():
            got = ops.adain(x, ad, C + 7, 3, relu=act, residual=r)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (case, act)


if __name__ == "__main__":
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    _child(sys.argv[1])
