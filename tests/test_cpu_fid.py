"""Host-side checks of FID evaluation (munit_amd/inception_utils.py, csrc/fid.hip, data.get_fid_data_loader): the oracle
against the reference's fixture, the C ABI's declarations and refusals (no device: the pointers are never followed), the
module's interface against the reference's recorded one, and the loader's construction."""
import inspect
import json
import os
import re
import subprocess
import sys
from ctypes import c_float, c_size_t, c_void_p

import numpy as np
import pytest
import torch

from tests import fid_oracle as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_BOUND = 1e-9          # the project's bound on a fixture reproduced in fp64
NEW_SYMBOLS = ("munit_gemm_f32", "munit_fid_moments_workspace_bytes", "munit_fid_moments",
               "munit_sqrt_newton_schulz_workspace_bytes", "munit_sqrt_newton_schulz",
               "munit_frechet_distance_workspace_bytes", "munit_frechet_distance")


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "golden_fid.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from munit_amd import _lib
    return _lib.load()


def _rel(got, ref):
    got, ref = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(ref, dtype=torch.float64)
    return float((got - ref).abs().max() / ref.abs().max())


def test_oracle_reproduces_the_reference_fixture(fixture):
    d, n = fixture["D"], fixture["N"]
    p1, p2 = FO.pools(d, n=n)
    (mu1, s1), (mu2, s2) = FO.cov(p1), FO.cov(p2)
    assert _rel(mu1, fixture["mu1"]) <= FIXTURE_BOUND and _rel(mu2, fixture["mu2"]) <= FIXTURE_BOUND
    assert _rel(s1, fixture["sigma1"]) <= FIXTURE_BOUND and _rel(s2, fixture["sigma2"]) <= FIXTURE_BOUND
    root = FO.sqrt_newton_schulz(s1.mm(s2).unsqueeze(0), fixture["iters"])[0]
    dg = fixture["sqrt_digest"]
    assert _rel(torch.trace(root), dg["trace"]) <= FIXTURE_BOUND
    assert _rel(root.sum(), dg["sum"]) <= FIXTURE_BOUND
    assert _rel(root.norm(), dg["fro"]) <= FIXTURE_BOUND
    for key, val in dg["entries"].items():
        i, j = (int(v) for v in key.split(","))
        assert abs(float(root[i, j]) - val) <= FIXTURE_BOUND * dg["fro"], key
    fd, _ = FO.frechet(mu1, s1, mu2, s2, fixture["iters"])
    assert _rel(fd, fixture["frechet_torch"]) <= FIXTURE_BOUND


def test_newton_schulz_and_scipy_values_of_the_fixture_agree(fixture):
    assert _rel(fixture["frechet_torch"], fixture["frechet_numpy"]) <= 1e-6


def test_host_frechet_distance_reproduces_the_fixture(fixture):
    from munit_amd import inception_utils as IU
    got = IU.numpy_calculate_frechet_distance(*(np.array(fixture[k]) for k in ("mu1", "sigma1", "mu2", "sigma2")))
    assert _rel(got, fixture["frechet_numpy"]) <= FIXTURE_BOUND


@pytest.mark.parametrize("d", [4, 64, 130])
def test_fp32_oracle_stays_close_on_the_parity_cases(d):
    """The premise of the GPU allowance: on N = 4 D pools fp32 stays within 3e-7 of fp64, relative to the sum of the
    magnitudes of the distance's terms (FO.frechet's normaliser)."""
    m = FO.moments(d)
    for iters in (20, 100):
        ref, norm = FO.frechet(*m, iters)
        got, _ = FO.frechet(*m, iters, dtype=torch.float32)
        assert abs(got - ref) <= 3e-7 * norm, (d, iters, got, ref, norm)


def test_new_symbols_are_declared_listed_and_exported(lib):
    from munit_amd import _lib
    header = open(os.path.join(ROOT, "include", "munit_hip.h")).read()
    declared = set(re.findall(r"\b(munit_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "fid.hip" in open(os.path.join(ROOT, "munit_amd", "csrc", "Makefile")).read()


def _err(lib):
    return lib.munit_last_error() or b""


def test_gemm_refusals_without_a_device(lib):
    from munit_amd._lib import GemmProblem
    f = lib.munit_gemm_f32
    ok = (GemmProblem * 2)(GemmProblem(0x100000, 0x200000, 0x300000), GemmProblem(0x400000, 0x500000, 0x600000))
    args = lambda **k: [k.get(n, v) for n, v in (("n", 2), ("M", 8), ("N", 12), ("K", 5), ("lda", 5), ("ldb", 12), ("ldc", 12),
                                                 ("transA", 0))] + [c_float(1.0), c_float(0.0), None]
    assert f(None, *args()) == -1 and b"gemm_f32" in _err(lib)
    for n in (0, 9, -1):
        assert f(ok, *args(n=n)) == -1 and b"gemm_f32: n must be 1..8" in _err(lib)
    for dim in ("M", "N", "K"):
        assert f(ok, *args(**{dim: 0})) == -1 and b"gemm_f32: M, N, K" in _err(lib)
    assert f(ok, *args(lda=4)) == -1 and b"gemm_f32: lda 4 shorter" in _err(lib)
    assert f(ok, *args(transA=1, lda=7)) == -1 and b"gemm_f32: lda 7 shorter" in _err(lib)     # op(A) = A^T: rows of A are M long
    assert f(ok, *args(ldb=11)) == -1 and b"gemm_f32: ldb 11 shorter" in _err(lib)
    assert f(ok, *args(ldc=11)) == -1 and b"gemm_f32: ldc 11 shorter" in _err(lib)
    hole = (GemmProblem * 2)(GemmProblem(0x100000, 0x200000, 0x300000), GemmProblem(0x400000, None, 0x600000))
    assert f(hole, *args()) == -1 and b"gemm_f32: problem 1 has a null pointer" in _err(lib)
    cbytes = (7 * 12 + 12) * 4
    for p in ([(0x100000, 0x200000, 0x100000), (0x400000, 0x500000, 0x600000)],               # C is A
              [(0x100000, 0x200000, 0x200000 + 5 * 12 * 4 - 4), (0x400000, 0x500000, 0x600000)],   # C starts in B's last word
              [(0x100000, 0x200000, 0x300000), (0x300000 + cbytes - 4, 0x500000, 0x600000)],   # A of 1 starts in C of 0's last word
              [(0x100000, 0x200000, 0x300000), (0x400000, 0x500000, 0x300000 + cbytes - 4)]):  # the two C overlap
        tab = (GemmProblem * 2)(*[GemmProblem(*q) for q in p])
        assert f(tab, *args()) == -1 and b"gemm_f32: C of problem" in _err(lib) and b"overlaps" in _err(lib), p


def test_moments_square_root_and_distance_refusals_without_a_device(lib):
    P = c_void_p(0x100000)
    mom, wsm = lib.munit_fid_moments, lib.munit_fid_moments_workspace_bytes
    assert wsm(48, 12) == 48 * 12 * 4 and wsm(1, 12) == 0 and wsm(48, 0) == 0
    need = wsm(48, 12)
    for k in range(4):
        a = [P, P, P, P]
        a[k] = None
        assert mom(a[0], 48, 12, a[1], a[2], a[3], need, None) == -1 and b"fid_moments: null pointer" in _err(lib)
    assert mom(P, 48, 0, P, P, P, need, None) == -1 and b"fid_moments: D must be >= 1" in _err(lib)
    assert mom(P, 1, 12, P, P, P, need, None) == -1 and b"fid_moments: N must be >= 2" in _err(lib)
    assert mom(P, 48, 12, P, P, P, need - 1, None) == -1 and b"fid_moments: workspace too small" in _err(lib)

    ns, wsn = lib.munit_sqrt_newton_schulz, lib.munit_sqrt_newton_schulz_workspace_bytes
    assert wsn(0, 1) == 0 and wsn(12, 0) == 0 and wsn(12, 3) >= 5 * 3 * 144 * 4
    need = wsn(12, 3)
    for k in range(3):
        a = [P, P, P]
        a[k] = None
        assert ns(a[0], 12, 5, 3, a[1], a[2], need, None) == -1 and b"sqrt_newton_schulz: null pointer" in _err(lib)
    assert ns(P, 0, 5, 3, P, P, need, None) == -1 and b"sqrt_newton_schulz: D must be >= 1" in _err(lib)
    assert ns(P, 12, -1, 3, P, P, need, None) == -1 and b"sqrt_newton_schulz: iters must be >= 0" in _err(lib)
    assert ns(P, 12, 5, 0, P, P, need, None) == -1 and b"sqrt_newton_schulz: b must be" in _err(lib)
    assert ns(P, 12, 5, 3, P, P, need - 1, None) == -1 and b"sqrt_newton_schulz: workspace too small" in _err(lib)

    fd, wsf = lib.munit_frechet_distance, lib.munit_frechet_distance_workspace_bytes
    assert wsf(0) == 0 and wsf(12) >= 7 * 144 * 4
    need = wsf(12)
    for k in range(6):
        a = [P] * 6
        a[k] = None
        assert fd(a[0], a[1], a[2], a[3], 12, 400, a[4], a[5], need, None) == -1 and b"frechet_distance: null pointer" in _err(lib)
    assert fd(P, P, P, P, 0, 400, P, P, need, None) == -1 and b"frechet_distance: D must be >= 1" in _err(lib)
    assert fd(P, P, P, P, 12, -1, P, P, need, None) == -1 and b"frechet_distance: iters must be >= 0" in _err(lib)
    assert fd(P, P, P, P, 12, 400, P, P, need - 1, None) == -1 and b"frechet_distance: workspace too small" in _err(lib)
    # sigma1 inside the workspace: the product would be written over its own operand
    assert fd(P, P, P, P, 12, 400, P, P, c_size_t(need), None) == -1 and b"frechet_distance: C of problem 0 overlaps" in _err(lib)


def test_inception_utils_has_the_references_names_and_parameter_lists(fixture):
    from munit_amd import inception_utils as IU
    sigs = fixture["signatures"]
    assert len(sigs) == 8
    for name, rec in sigs.items():
        obj = getattr(IU, name)
        if rec["kind"] == "class":
            assert inspect.isclass(obj)
            for m, params in rec["methods"].items():
                assert list(inspect.signature(getattr(obj, m)).parameters) == params, (name, m)
            continue
        sig = inspect.signature(obj)
        params = list(sig.parameters)
        defaults = {k: repr(p.default) for k, p in sig.parameters.items() if p.default is not p.empty}
        if name == "prepare_inception_metrics":          # the one extension: a trailing net=None
            assert params[-1] == "net" and defaults.pop("net") == "None"
            params = params[:-1]
        assert params == rec["params"] and defaults == rec["defaults"], name


def test_prepare_inception_metrics_refuses_without_net_and_with_parallel(tmp_path):
    from munit_amd import inception_utils as IU
    npz = str(tmp_path / "moments.npz")
    np.savez(npz, mu=np.zeros(4), sigma=np.eye(4))
    with pytest.raises(NotImplementedError, match=r"net="):
        IU.prepare_inception_metrics(npz)
    with pytest.raises(NotImplementedError, match=r"net="):
        IU.load_inception_net()
    with pytest.raises(NotImplementedError, match=r"parallel"):
        IU.prepare_inception_metrics(npz, parallel=True, net=lambda x: x)
    assert callable(IU.prepare_inception_metrics(npz, net=lambda x: x))


def _lists(tmp_path, na, nb):
    fa, fb = tmp_path / "a.txt", tmp_path / "b.txt"
    fa.write_text("".join("a_%d.png extra\n" % i for i in range(na)))
    fb.write_text("".join("b_%d.png\n" % i for i in range(nb)))
    return str(fa), str(fb)


def test_fid_loader_lists_and_length(tmp_path):
    from munit_amd import data
    fa, fb = _lists(tmp_path, 7, 6)
    with pytest.raises(ValueError, match=r"list b has 6 records, list a 7"):
        data.get_fid_data_loader(fa, fb, 2, False, new_size=32)
    fa, fb = _lists(tmp_path, 7, 9)
    loader = data.get_fid_data_loader(fa, fb, 2, True, new_size=32)
    assert len(loader) == 3                                    # drop_last: the seventh sample has no batch
    assert loader.image_paths == ["a_%d.png" % i for i in range(7)] and len(loader.target_paths) == 9
    assert list(inspect.signature(data.get_fid_data_loader).parameters)[:6] == \
        ["file_list_a", "file_list_b", "batch_size", "train", "new_size", "num_workers"]
    assert inspect.signature(data.get_fid_data_loader).parameters["new_size"].default == 256


_SHARD_WORKER = r"""
import sys, torch.distributed as dist
sys.path.insert(0, %(root)r)
from munit_amd import data
dist.init_process_group("gloo", init_method="file://%(rdzv)s", rank=int(sys.argv[1]), world_size=2)
paths = ["a_%%d.png" %% i for i in range(8)]
plain = data.DeviceBatchLoader(paths, None, 2, False, 32, 32, 32, crop=False)
assert plain.world_size == 2 and len(plain) == 2
fid = data.get_fid_data_loader(%(fa)r, %(fb)r, 2, False, new_size=32)
assert len(fid) == 4 and (fid._loader.rank, fid._loader.world_size) == (0, 1)
assert data.shard_indices(8, 2, False, 0, fid._loader.rank, fid._loader.world_size) == [[0, 1], [2, 3], [4, 5], [6, 7]]
dist.barrier()
dist.destroy_process_group()
print("ok")
"""


def test_fid_loader_does_not_shard_under_a_gloo_group_of_two(tmp_path):
    fa, fb = _lists(tmp_path, 8, 8)
    script = tmp_path / "w.py"
    script.write_text(_SHARD_WORKER % dict(root=ROOT, rdzv=str(tmp_path / "rdzv"), fa=fa, fb=fb))
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              cwd=ROOT) for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
