"""GPU tests of dann.hip's batch norm, 2x2 max-pool and 16x16 average in every launch regime (tests/dann_regimes.py): the
entry points through ctypes against fp64 torch, exact checks on integer-lattice data, the workspace partials pinned to the
restated block count, the guard-band contract and every refusal the entry points state.

Bounds: those of tests/test_gpu_featda.test_batchnorm_against_fp64 -- normalised maximum error 1e-5 for y, the two-float
mean and rstd, 5e-5 for dx, dgamma and dbeta -- with one exception that conditioning forces: dx at R = 2 (_dx_bound).
Outputs are prefilled with NaN, so an element a launch does not write shows up in every comparison."""
import time
from ctypes import c_float, c_void_p

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from munit_amd import _lib
from tests import dann_regimes as R
from tests.conv_contract import GUARD_BYTE, Arena, Launches, fill_random, no_nan, poison, stream
from tests.kernel_contract import ERR_ARG, refused
from tests.parity import nerr
from tests.test_gpu_featda import FWD_TOL, GRAD_TOL, _bn_ref, _contract, _rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS, MOM = 1e-5, 0.1
NAN = float("nan")


def _p(t):
    return None if t is None else c_void_p(t.data_ptr())


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


class _BN(object):
    """munit_batchnorm_fwd / _bwd through ctypes on (R, C) device rows; every output starts as NaN."""

    def __init__(self, x, dy, gamma, beta):
        self.lib = _lib.load()
        self.x, self.dy, self.gamma, self.beta = x, dy, gamma, beta
        self.r, self.c = x.shape
        self.nws = self.lib.munit_batchnorm_workspace_bytes(self.c)
        self.ws = torch.full((self.nws,), GUARD_BYTE, dtype=torch.uint8, device=DEV)

    def fwd(self, rm, rv, relu, momentum=MOM, eval_=0):
        y, mean, rstd = _nan(self.r, self.c), _nan(2 * self.c), _nan(self.c)
        self.ws.fill_(GUARD_BYTE)
        _lib.check(self.lib.munit_batchnorm_fwd(_p(self.x), _p(y), None if eval_ else _p(mean), None if eval_ else _p(rstd),
                                                _p(rm), _p(rv), self.r, self.c, _p(self.gamma), _p(self.beta), relu, eval_,
                                                c_float(EPS), c_float(momentum), None if eval_ else _p(self.ws),
                                                0 if eval_ else self.nws, stream()), "batchnorm_fwd")
        torch.cuda.synchronize()
        return y, mean, rstd

    def bwd(self, y, mean, rstd, relu, dg=None, db=None, acc=0.0):
        dx = _nan(self.r, self.c)
        self.ws.fill_(GUARD_BYTE)
        _lib.check(self.lib.munit_batchnorm_bwd(_p(self.x), _p(self.dy), _p(y), _p(self.gamma), _p(mean), _p(rstd), _p(dx),
                                                _p(dg), _p(db), c_float(acc), self.r, self.c, relu, _p(self.ws), self.nws,
                                                stream()), "batchnorm_bwd")
        torch.cuda.synchronize()
        return dx


def _ref32(x, gamma, beta, relu, dy):
    """_bn_ref's formulas evaluated by torch in fp32: what plain fp32 arithmetic makes of this data (dx only)."""
    x = x.float().clone().requires_grad_(True)
    m = x.mean(0)
    v = ((x - m) ** 2).mean(0)
    y = (x - m) * (1 / torch.sqrt(v + EPS)) * gamma.float() + beta.float()
    if relu:
        y = F.relu(y)
    return torch.autograd.grad(y, [x], dy.float())[0]


def _dx_bound(r, e32):
    """5e-5 everywhere; at R = 2 the rule of tests/fid_oracle.allowance, max(floor, 4 e32): with two rows per channel
    g - sum g / R - xhat sum(g xhat) / R cancels to eps rstd^2 of its terms (the comment above bn_dp_combine_kernel), so one
    fp32 rounding of xhat or rstd is amplified by var / eps -- in ANY fp32 evaluation, torch's included (e32)."""
    return max(GRAD_TOL, 4.0 * e32) if r == 2 else GRAD_TOL


FP64_CASES = [(r, c, 0.0) for r, c in R.BN_SHAPES] + [(r, c, 100.0) for r, c in R.BN_LARGE_MEAN]


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", FP64_CASES, ids=lambda c: "%dx%d_mean%g" % c)
def test_batchnorm_against_fp64_in_every_regime(case, relu):
    t0 = time.time()
    r, c, mean = case
    x, dy = _rows(r, c, 1, mean), _rows(r, c, 2)
    g = torch.Generator().manual_seed(3)
    gamma, beta = 1 + 0.3 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)
    xd, dyd, gd, bd = x.to(DEV), dy.to(DEV), gamma.to(DEV), beta.to(DEV)
    on_device = (r, c) in R.BN_DEVICE_REFERENCE           # torch's fp64 on the device: not the code under test
    ry, rm_, rrstd, runb, rdx, rdg, rdb = _bn_ref(xd, gd, bd, relu, dyd) if on_device else _bn_ref(x, gamma, beta, relu, dy)
    bn = _BN(xd, dyd, gd, bd)
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    y, m, rstd = bn.fwd(rm, rv, relu)
    dg, db = _nan(c), _nan(c)                             # acc = 0 must not read them
    dx = bn.bwd(y, m, rstd, relu, dg, db)
    errs = dict(y=nerr(y, ry), mean=nerr(m[:c].double() + m[c:].double(), rm_), rstd=nerr(rstd, rrstd), dx=nerr(dx, rdx),
                dgamma=nerr(dg, rdg), dbeta=nerr(db, rdb))
    e32 = nerr(_ref32(x, gamma, beta, relu, dy), rdx) if r == 2 else None
    bound = _dx_bound(r, e32 or 0.0)
    print("batchnorm", case, "relu", relu, R.regime(r, c), errs)
    if r == 2:
        print("  R = 2: e32 %.3e, kernel dx error %.3e, allowance %.3e" % (e32, errs["dx"], bound))
    if relu:                                              # a y within rounding of 0 may sit on the other side of the kink
        ryh, yh = ry.to(y.device), y
        off = (yh > 0) != (ryh > 0)
        near = (ryh.abs() < 1e-5 * float(ryh.abs().max())) & off
        assert int(near.sum()) == int(off.sum())
    ratio = max(max(errs[k] for k in ("y", "mean", "rstd")) / FWD_TOL, errs["dx"] / bound,
                max(errs["dgamma"], errs["dbeta"]) / GRAD_TOL)
    for k in ("y", "mean", "rstd"):
        assert errs[k] <= FWD_TOL, errs
    assert errs["dx"] <= bound, (errs, e32)
    for k in ("dgamma", "dbeta"):
        assert errs[k] <= GRAD_TOL, errs
    # the running statistics after two calls: momentum 0.1, unbiased variance
    y2, m2, rstd2 = bn.fwd(rm, rv, relu)
    dg2, db2 = _nan(c), _nan(c)
    dx2 = bn.bwd(y2, m2, rstd2, relu, dg2, db2)
    assert nerr(rm, 0.19 * rm_) <= FWD_TOL and nerr(rv, 0.81 + 0.19 * runb) <= FWD_TOL, \
        (nerr(rm, 0.19 * rm_), nerr(rv, 0.81 + 0.19 * runb))
    # a second forward / backward is bitwise the first
    for a, b in ((y, y2), (m, m2), (rstd, rstd2), (dx, dx2), (dg, dg2), (db, db2)):
        assert torch.equal(a, b)
    # null dgamma / dbeta: dx is the same
    assert torch.equal(bn.bwd(y, m, rstd, relu), dx)
    # evaluation mode: the running statistics' formula, nothing updated
    rm0, rv0 = rm.clone(), rv.clone()
    ye, _, _ = bn.fwd(rm, rv, relu, eval_=1)
    xe = xd.double() if on_device else x.double()
    dev = xe.device
    want = (xe - rm0.double().to(dev)) / torch.sqrt(rv0.double().to(dev) + EPS) * gamma.double().to(dev) + beta.double().to(dev)
    want = F.relu(want) if relu else want
    assert nerr(ye, want) <= FWD_TOL and torch.equal(rm, rm0) and torch.equal(rv, rv0)
    print("  %.2f s, worst error / bound %.3f" % (time.time() - t0, ratio))


def test_evaluation_mode_accepts_one_row():
    x, dy = _rows(1, 64, 21), _rows(1, 64, 22)
    gamma, beta = torch.rand(64) + 0.5, torch.rand(64) - 0.5
    rm, rv = torch.randn(64, generator=torch.Generator().manual_seed(23)), torch.rand(64) + 0.5
    for relu in (0, 1):
        rmd, rvd = rm.to(DEV), rv.to(DEV)
        y, _, _ = _BN(x.to(DEV), dy.to(DEV), gamma.to(DEV), beta.to(DEV)).fwd(rmd, rvd, relu, eval_=1)
        want = (x.double() - rm.double()) / torch.sqrt(rv.double() + EPS) * gamma.double() + beta.double()
        assert nerr(y, F.relu(want) if relu else want) <= FWD_TOL
        assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv)


# ---- exact checks on integer-lattice data -------------------------------------------------------------------------------
def _lattice_case(r, c):
    """x and dy on the lattice -3..3 with two constant columns of x (3.0 and 100.0), gamma / beta off the lattice"""
    x, dy = R.lattice_rows(r, c, 11), R.lattice_rows(r, c, 12)
    x[:, 0], x[:, 1] = 3.0, 100.0
    g = torch.Generator().manual_seed(13)
    gamma, beta = 1 + 0.3 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g) + 0.01
    return x, dy, gamma, beta


@pytest.mark.parametrize("rc", R.BN_SHAPES, ids=str)
def test_batchnorm_exact_on_the_lattice(rc):
    """Every fp32 partial sum of the lattice is an integer below 2^24 (3 x 36 864 rows at the most, 6 x for the differences
    from the first row), so whatever the partition, these hold bit for bit; a row dropped, counted twice or read past the
    tensor changes an integer (tests/test_cpu_dann_regimes.py shows it for three such faults)."""
    t0 = time.time()
    r, c = rc
    x, dy, gamma, beta = _lattice_case(r, c)
    bn = _BN(x.to(DEV), dy.to(DEV), gamma.to(DEV), beta.to(DEV))
    old_m, old_v = torch.full((c,), 0.25, device=DEV), torch.full((c,), 1.5, device=DEV)
    rm, rv = old_m.clone(), old_v.clone()
    y, m, rstd = bn.fwd(rm, rv, 0)
    hi, lo = m[:c], m[c:]
    # the two-float mean: mu = x[0] + s / R in double from an exact s -- two roundings of at most 2^-53 max|x| each, and
    # lo keeps 24 bits below hi's 24 (2^-48 |mu|): far inside 2^-46 relative to the column's largest entry
    want = x.double().mean(0)
    err = ((hi.double() + lo.double()).cpu() - want).abs() / x.double().abs().amax(0).clamp_min(1.0)
    assert float(err.max()) <= 2.0 ** -46, (float(err.max()), int(err.argmax()))
    # the constant columns
    const = torch.tensor([3.0, 100.0], device=DEV)
    assert torch.equal(hi[:2], const) and bool((lo[:2] == 0).all()), (hi[:2], lo[:2])
    assert torch.equal(y[:, :2], bn.beta[:2].expand(r, 2)), "y != beta on a constant column"
    one_minus = torch.tensor(1.0, device=DEV) - torch.tensor(MOM, dtype=torch.float32, device=DEV)
    assert torch.equal(rv[:2], (one_minus * old_v)[:2]), rv[:2]
    eps32 = float(torch.tensor(EPS, dtype=torch.float32))
    assert float((rstd[:2].double().cpu() * np.sqrt(eps32) - 1).abs().max()) <= 2.0 ** -23, rstd[:2]
    y1, _, _ = bn.fwd(rm.clone(), rv.clone(), 1)
    assert torch.equal(y1[:, :2], torch.relu(bn.beta[:2]).expand(r, 2)) and torch.equal(y1, torch.relu(y))
    # ReLU off: dbeta is the exact column sum of dy; xhat is exactly 0 on a constant column, so its dgamma is 0
    dg, db = _nan(c), _nan(c)
    dx = bn.bwd(y, m, rstd, 0, dg, db)
    assert torch.equal(db.cpu(), dy.double().sum(0).float()), "dbeta != dy.sum(0)"
    assert bool((dg[:2] == 0).all()) and no_nan(dx)
    # acc = 1: exactly old + (the acc = 0 result)
    prior_g, prior_b = R.lattice_rows(1, c, 14)[0].to(DEV) * 0.5, R.lattice_rows(1, c, 15)[0].to(DEV)
    dg1, db1 = prior_g.clone(), prior_b.clone()
    assert torch.equal(bn.bwd(y, m, rstd, 0, dg1, db1, acc=1.0), dx)
    assert torch.equal(dg1, prior_g + dg) and torch.equal(db1, prior_b + db)
    # momentum 0 leaves the running buffers alone; momentum 1 sets running_mean to float(hi + lo)
    rm0, rv0 = old_m.clone(), old_v.clone()
    y0, m0, _ = bn.fwd(rm0, rv0, 0, momentum=0.0)
    assert torch.equal(rm0, old_m) and torch.equal(rv0, old_v) and torch.equal(y0, y)
    rm1, rv1 = old_m.clone(), old_v.clone()
    bn.fwd(rm1, rv1, 0, momentum=1.0)
    assert torch.equal(rm1, (hi.double() + lo.double()).float()) and torch.equal(m0, m)
    print("lattice %s: %.2f s" % (rc, time.time() - t0))


# ---- the restated block count against what a launch leaves in its workspace ----------------------------------------------
@pytest.mark.parametrize("rc", R.BN_SHAPES, ids=str)
def test_workspace_partials_match_the_restated_block_count(rc):
    r, c = rc
    g = torch.Generator(device=DEV).manual_seed(17)
    x, dy = torch.randn(r, c, device=DEV, generator=g), torch.randn(r, c, device=DEV, generator=g)
    bn = _BN(x, dy, torch.rand(c, device=DEV, generator=g) + 0.5, torch.randn(c, device=DEV, generator=g))
    nb, tail = R.bn_blocks(r, c), R.part_bytes(c)
    assert bn.nws == R.workspace_bytes(c)
    y, m, rstd = bn.fwd(torch.zeros(c, device=DEV), torch.ones(c, device=DEV), 1)
    n = nb * c
    assert bool(torch.isfinite(bn.ws[:4 * n].view(torch.float32)).all()), "fewer than nb * C partials"
    assert bool((bn.ws[4 * n:] == GUARD_BYTE).all()), "the forward wrote past its nb * C partials"
    bn.bwd(y, m, rstd, 1, _nan(c), _nan(c))
    n = 2 * nb * c
    assert bool(torch.isfinite(bn.ws[:4 * n].view(torch.float32)).all()), "fewer than 2 * nb * C partials"
    assert bool((bn.ws[4 * n:tail] == GUARD_BYTE).all()), "the backward wrote past its 2 * nb * C partials"
    assert bool(torch.isfinite(bn.ws[tail:tail + 8 * c].view(torch.float32)).all()), "the 2 C sums are not where the header puts them"
    assert bool((bn.ws[tail + 8 * c:] == GUARD_BYTE).all())


# ---- guard bands and refusals ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", R.BN_CONTRACT, ids=str)
def test_guard_bands_and_refusals_batchnorm(rc):
    lib = _lib.load()
    r, c = rc
    n, nws = r * c * 4, lib.munit_batchnorm_workspace_bytes(c)
    a = Arena(dict(x=n, dy=n, gamma=c * 4, beta=c * 4, rm=c * 4, rv=c * 4, y=n, mean=c * 8, rstd=c * 4, dx=n, dg=c * 4,
                   db=c * 4, ws=nws), torch.device(DEV))
    for i, nm in enumerate(("x", "dy", "gamma", "beta")):
        fill_random(a.view(nm, torch.float32), 60 + i)
    p = a.ptr
    rm, rv = a.view("rm", torch.float32), a.view("rv", torch.float32)

    def fwd(R_=r, C_=c, relu=1, eval_=0, eps=EPS, mom=MOM, mean="mean"):
        rm.fill_(0.25)
        rv.fill_(1.5)
        return lib.munit_batchnorm_fwd(p("x"), p("y"), p(mean) if mean else None, p("rstd"), p("rm"), p("rv"), R_, C_,
                                       p("gamma"), p("beta"), relu, eval_, c_float(eps), c_float(mom), p("ws"), nws, stream())

    def bwd(R_=r, C_=c, relu=1, acc=0.0, y="y"):
        return lib.munit_batchnorm_bwd(p("x"), p("dy"), p(y) if y else None, p("gamma"), p("mean"), p("rstd"), p("dx"),
                                       p("dg"), p("db"), c_float(acc), R_, C_, relu, p("ws"), nws, stream())

    L = _contract(a, ["x", "dy", "gamma", "beta"], ["y", "mean", "rstd"], "batchnorm_fwd %s" % (rc,), fwd)
    assert no_nan(rm) and no_nan(rv) and not bool((rm == 0.25).any())
    fouts = ["y", "mean", "rstd"]
    calls = [("C = %d" % bad, lambda bad=bad: fwd(C_=bad)) for bad in R.BN_REFUSED_C]
    calls += [("R = 0", lambda: fwd(R_=0)), ("R = 1 in training mode", lambda: fwd(R_=1)), ("eps = 0", lambda: fwd(eps=0.0)),
              ("eps = 0 in evaluation mode", lambda: fwd(eps=0.0, eval_=1)), ("momentum 1.5", lambda: fwd(mom=1.5)),
              ("momentum -0.5", lambda: fwd(mom=-0.5)), ("relu = 2", lambda: fwd(relu=2)), ("eval = 2", lambda: fwd(eval_=2)),
              ("mean = NULL in training mode", lambda: fwd(mean=None))]
    for label, call in calls:
        for o in fouts:
            poison(a.view(o, torch.float32), 0)
        a.bytes("ws").fill_(GUARD_BYTE)
        refused(L, call(), fouts, "fwd, " + label, code=ERR_ARG)
        assert bool((rm == 0.25).all()) and bool((rv == 1.5).all()), "fwd, %s: running statistics written" % label
    _lib.check(fwd(), "batchnorm_fwd")
    L = _contract(a, ["x", "dy", "gamma", "y", "mean", "rstd"], ["dx", "dg", "db"], "batchnorm_bwd %s" % (rc,), bwd)
    bouts = ["dx", "dg", "db"]
    calls = [("C = %d" % bad, lambda bad=bad: bwd(C_=bad)) for bad in R.BN_REFUSED_C]
    calls += [("R = 0", lambda: bwd(R_=0)), ("relu = 2", lambda: bwd(relu=2)), ("acc = 0.5", lambda: bwd(acc=0.5)),
              ("relu = 1 with y = NULL", lambda: bwd(y=None))]
    for label, call in calls:
        for o in bouts:
            poison(a.view(o, torch.float32), 0)
        a.bytes("ws").fill_(GUARD_BYTE)
        refused(L, call(), bouts, "bwd, " + label, code=ERR_ARG)
    # relu = 0 needs no y
    for o in bouts:
        poison(a.view(o, torch.float32), 0)
    L.after(bwd(relu=0, y=None), "relu = 0 with y = NULL")
    assert all(no_nan(a.view(o, torch.float32)) for o in bouts)


# ---- 2x2 max-pool ---------------------------------------------------------------------------------------------------------
def _maxpool_raw(x, dy=None):
    """munit_maxpool2_fwd (+ _bwd) on an NHWC device tensor (B, H, W, C): y, the winner bytes, dx into NaN"""
    lib = _lib.load()
    b, h, w, c = x.shape
    y = _nan(b, h // 2, w // 2, c)
    idx = torch.full((b, h // 2, w // 2, c), 0xA5, dtype=torch.uint8, device=DEV)
    _lib.check(lib.munit_maxpool2_fwd(_p(x), _p(y), _p(idx), b, h, w, c, stream()), "maxpool2_fwd")
    dx = None
    if dy is not None:
        dx = _nan(b, h, w, c)
        _lib.check(lib.munit_maxpool2_bwd(_p(dy), _p(idx), _p(dx), b, h, w, c, stream()), "maxpool2_bwd")
    torch.cuda.synchronize()
    return y, idx, dx


def test_maxpool2_special_values_follow_the_documented_rule():
    """All 2401 windows over {NaN, -inf, +inf, -0, +0, 1, -1} (padded to 2404) as one (1, 2, 1202, 4) map, window n at
    column pair n // 4, channel n % 4: y bitwise (NaN-ness, the sign of zero), the winner bytes and dx against
    tests/dann_regimes.maxpool_rule, which tests/test_cpu_dann_regimes.py holds to torch's own kernels."""
    win = R.special_windows(np.float32)
    win = np.concatenate([win, win[:3]])                  # 2404 windows = 601 column pairs x 4 channels
    n = win.shape[0]
    dy = (np.arange(n) + 1).astype(np.float32)
    val, idx, dx = R.maxpool_rule(win, dy)
    # x[0, kh, 2 * ow + kw, c] = win[ow * 4 + c, kh * 2 + kw]
    x = torch.from_numpy(win).reshape(n // 4, 4, 2, 2).permute(2, 0, 3, 1).reshape(1, 2, n // 2, 4).contiguous()
    y, got_idx, got_dx = _maxpool_raw(x.to(DEV), torch.from_numpy(dy).reshape(1, 1, n // 4, 4).to(DEV))
    assert torch.equal(y.cpu().reshape(-1).view(torch.int32), torch.from_numpy(val).view(torch.int32)), "y differs bitwise"
    assert torch.equal(got_idx.cpu().reshape(-1).long(), torch.from_numpy(idx))
    want_dx = torch.from_numpy(dx).reshape(n // 4, 4, 2, 2).permute(2, 0, 3, 1).reshape(1, 2, n // 2, 4)
    assert torch.equal(got_dx.cpu().view(torch.int32), want_dx.contiguous().view(torch.int32))


@pytest.mark.parametrize("shape", R.MAXPOOL_SMALL, ids=str)
def test_maxpool2_small_shapes_against_fp64(shape):
    b, h, w, c = shape
    g = torch.Generator().manual_seed(h * 100 + w + c)
    for lattice in (False, True):
        x = torch.randint(-2, 3, (b, c, h, w), generator=g).float() if lattice else torch.randn(b, c, h, w, generator=g)
        xr = x.double().requires_grad_(True)
        yr = F.max_pool2d(xr, 2)
        dy = torch.randn(yr.shape, generator=g)
        (dxr,) = torch.autograd.grad(yr, [xr], dy.double())
        nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)
        y, idx, dx = _maxpool_raw(nhwc(x), nhwc(dy))
        assert torch.equal(y.cpu().double(), yr.detach().permute(0, 2, 3, 1))
        assert torch.equal(dx.cpu().double(), dxr.permute(0, 2, 3, 1))          # ties: the first maximum in window order
        assert int(idx.max()) <= 3
        assert bool((dx[:, 2 * (h // 2):] == 0).all()) and bool((dx[:, :, 2 * (w // 2):] == 0).all())


def test_maxpool2_past_the_grid_cap():
    """(4, 130, 130, 1024): 4 326 400 output quads and 17 305 600 input quads against 4 194 304 per trip.  No two entries of
    a window are equal (asserted on the host), so the winner is unambiguous and the reference -- torch on the device, not
    the code under test -- must be matched bit for bit, forward and backward."""
    t0 = time.time()
    b, h, w, c = R.MAXPOOL_WRAP
    assert R.wraps(b * (h // 2) * (w // 2) * (c // 4)) and R.wraps(b * h * w * (c // 4))
    # 22 random bits, then the window position in the two lowest: integers below 2^24 (exact in fp32) that cannot tie within
    # a window, while the winner is decided by the random bits wherever they differ
    hi = torch.randint(0, 1 << 22, (b, h, w, c), generator=torch.Generator().manual_seed(31), dtype=torch.int32)
    pos = (torch.arange(h, dtype=torch.int32) % 2 * 2).view(1, h, 1, 1) + (torch.arange(w, dtype=torch.int32) % 2).view(1, 1, w, 1)
    x = (hi * 4 + pos).float() / float(1 << 24)
    k = [x[:, kh::2, kw::2] for kh in (0, 1) for kw in (0, 1)]
    assert not any(bool((k[i] == k[j]).any()) for i in range(4) for j in range(i + 1, 4)), "equal entries in a window"
    xd = x.to(DEV)
    dy = torch.randn(b, h // 2, w // 2, c, device=DEV, generator=torch.Generator(device=DEV).manual_seed(32))
    y, idx, dx = _maxpool_raw(xd, dy)
    kd = torch.stack([xd[:, kh::2, kw::2] for kh in (0, 1) for kw in (0, 1)])
    want_y, want_idx = kd.max(0)
    assert torch.equal(y, want_y) and torch.equal(idx.long(), want_idx)
    assert min(int((want_idx == q).sum()) for q in range(4)) > want_idx.numel() // 5       # every position wins its share
    want_dx = torch.zeros_like(xd)
    for q, (kh, kw) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        want_dx[:, kh::2, kw::2] = torch.where(want_idx == q, dy, torch.zeros_like(dy))
    assert torch.equal(dx, want_dx)
    print("maxpool2 wrap: %.2f s" % (time.time() - t0))


def test_maxpool2_refusals():
    lib = _lib.load()
    b, h, w, c = 1, 4, 4, 8
    nx, ny = b * h * w * c, b * (h // 2) * (w // 2) * c
    a = Arena(dict(x=nx * 4, dy=ny * 4, y=ny * 4, idx=ny * 4, dx=nx * 4), torch.device(DEV))
    fill_random(a.view("x", torch.float32), 70)
    fill_random(a.view("dy", torch.float32), 71)
    p = a.ptr
    L = Launches(a, ["x", "dy"], "maxpool2")
    outs = ["y", "idx", "dx"]                             # idx as a 4-byte region: the poison check reads whole words

    def f(h_=h, w_=w, c_=c, idx="idx"):
        return lib.munit_maxpool2_fwd(p("x"), p("y"), p(idx) if idx else None, b, h_, w_, c_, stream())

    def bw(h_=h, w_=w, c_=c, idx="idx"):
        return lib.munit_maxpool2_bwd(p("dy"), p(idx) if idx else None, p("dx"), b, h_, w_, c_, stream())

    for label, call in (("fwd, H = 1", lambda: f(h_=1)), ("fwd, W = 1", lambda: f(w_=1)), ("fwd, C = 6", lambda: f(c_=6)),
                        ("fwd, idx = NULL", lambda: f(idx=None)), ("bwd, H = 1", lambda: bw(h_=1)),
                        ("bwd, W = 1", lambda: bw(w_=1)), ("bwd, C = 6", lambda: bw(c_=6)),
                        ("bwd, idx = NULL", lambda: bw(idx=None))):
        for o in outs:
            poison(a.view(o, torch.float32), 0)
        refused(L, call(), outs, label, code=ERR_ARG)


# ---- 16x16 average ----------------------------------------------------------------------------------------------------------
def _avg_raw(x):
    lib = _lib.load()
    b, h, w, c = x.shape
    y = _nan(b, c)
    _lib.check(lib.munit_avgpool16_fwd(_p(x), _p(y), b, h, w, c, stream()), "avgpool16_fwd")
    torch.cuda.synchronize()
    return y


def _avg_bwd_raw(dy, h, w):
    lib = _lib.load()
    b, c = dy.shape
    dx = _nan(b, h, w, c)
    _lib.check(lib.munit_avgpool16_bwd(_p(dy), _p(dx), b, h, w, c, stream()), "avgpool16_bwd")
    torch.cuda.synchronize()
    return dx


def _avg_bwd_want(dy, h, w):
    b, c = dy.shape
    want = torch.zeros(b, h, w, c, device=dy.device)
    want[:, :16, :16] = (dy / 256.0)[:, None, None, :]     # a division by 2^8: exact
    return want


@pytest.mark.parametrize("hw", R.AVG16_HW, ids=str)
@pytest.mark.parametrize("c", R.AVG16_C)
def test_avgpool16_every_lane_layout(c, hw):
    """C = 4 (256 lanes, one window position each) to C = 1024 (one lane walks all 256): within 1e-5 of fp64 on random data,
    exact on the lattice (window sums of at most 3 x 256), the backward bitwise dy / 256 inside the window and 0 outside."""
    h, w = hw
    b = 3
    g = torch.Generator().manual_seed(c + h + w)
    x = torch.randn(b, h, w, c, generator=g)
    y = _avg_raw(x.to(DEV))
    assert nerr(y, x[:, :16, :16].double().mean((1, 2))) <= FWD_TOL
    xl = R.lattice_rows(b * h * w, c, 41).reshape(b, h, w, c)
    yl = _avg_raw(xl.to(DEV))
    assert torch.equal(yl.cpu(), (xl[:, :16, :16].double().sum((1, 2)) / 256.0).float())
    dy = torch.randn(b, c, generator=g).to(DEV)
    assert torch.equal(_avg_bwd_raw(dy, h, w), _avg_bwd_want(dy, h, w))


def test_avgpool16_bwd_past_the_grid_cap():
    t0 = time.time()
    b, h, w, c = R.AVG16_BWD_WRAP
    assert R.wraps(b * h * w * (c // 4))
    dy = torch.randn(b, c, device=DEV, generator=torch.Generator(device=DEV).manual_seed(51))
    assert torch.equal(_avg_bwd_raw(dy, h, w), _avg_bwd_want(dy, h, w))
    print("avgpool16_bwd wrap: %.2f s" % (time.time() - t0))


def test_avgpool16_refusals():
    lib = _lib.load()
    b, c = 2, 16
    nx = b * 32 * 16 * c
    a = Arena(dict(x=nx * 4, dy=b * c * 4, y=b * c * 4, dx=nx * 4), torch.device(DEV))
    fill_random(a.view("x", torch.float32), 72)
    fill_random(a.view("dy", torch.float32), 73)
    p = a.ptr
    L = Launches(a, ["x", "dy"], "avgpool16")
    outs = ["y", "dx"]
    f = lambda h, w, c_=c: lib.munit_avgpool16_fwd(p("x"), p("y"), b, h, w, c_, stream())
    bw = lambda h, w, c_=c: lib.munit_avgpool16_bwd(p("dy"), p("dx"), b, h, w, c_, stream())
    for label, call in (("fwd, 15x16", lambda: f(15, 16)), ("fwd, 32x16", lambda: f(32, 16)), ("fwd, 16x15", lambda: f(16, 15)),
                        ("fwd, C = 12", lambda: f(16, 16, 12)), ("bwd, 15x16", lambda: bw(15, 16)),
                        ("bwd, 32x16", lambda: bw(32, 16)), ("bwd, C = 6", lambda: bw(16, 16, 6))):
        for o in outs:
            poison(a.view(o, torch.float32), 0)
        refused(L, call(), outs, label, code=ERR_ARG)
    # the backward has no lanes to lay out: it accepts C = 12 (the forward, whose block is C / 4 quads x 256 / (C / 4)
    # lanes, does not)
    dy = torch.randn(b, 12, device=DEV)
    assert torch.equal(_avg_bwd_raw(dy, 17, 16), _avg_bwd_want(dy, 17, 16))
