"""Contract checks of the normalisation, pooling, loss, optimiser, scaling and image entry points (include/munit_hip.h),
called straight through ctypes.

Not a test module: tests/test_gpu_ops.py runs these.  The harness is tests/conv_contract.py's: every tensor and workspace
is a region of one allocation between NaN guard bands, the workspace is NaN-poisoned before every launch, outputs are
prefilled with two different NaN payloads.  After every launch the guards and the inputs must be bitwise unchanged, the
outputs NaN-free and equal bitwise between the two payloads (every element written, deterministic).  A workspace one byte
short is refused with every output still holding its poison.  Per entry point:
  * norms: `stats` is exactly B*C*2 (instance norm) or B*2 (LayerNorm) floats (the region is that size); d_adain writes
    only its own 2*C columns of a wider row; LayerNorm's acc = 0 into NaN gives finite dgamma / dbeta, acc = 1 exactly
    old + new; the number of split partials left in the workspace is returned, for tests/test_cpu_norm_regimes.py's
    restatement of the split logic to be pinned against;
  * losses: da / db == NULL; munit_weighted_sum at n = 1, 32 and its refusal at 33;
  * optimisers: the gradient stays intact, ExtraAdam mode 0 saves p, modes 1 / 2 leave the saved copy alone, a buffer
    that is not 16-byte aligned is refused by Adam;
  * munit_scale: accumulate 0 into NaN, 1 into a live buffer; munit_act_bwd: all four codes;
  * the segmentation kernels (seg.hip; tests/test_gpu_semantic.py runs these): munit_seg_ce_fwd and _bwd each refuse a
    workspace one byte short of their OWN need, munit_seg_ce_workspace_bytes covers both, the loss does not depend on what
    the workspace held; the max-pool's uint8 winner plane is guarded, every entry in 0..8 and in bounds; every refusal the
    code states (x == y, H % f, W % f, inverse, n % 4, null pointers, norm <= 0, the 2^40 size limit) leaves every output
    untouched."""
import ctypes
from ctypes import c_double, c_float, c_size_t, c_void_p

import torch

from munit_amd import _lib
from tests.conv_contract import (ERR_WORKSPACE, GUARD_BYTE, POISON, _INT, Arena, Launches, bitwise_equal, fill_random,
                                 no_nan, poison, stream)

ERR_ARG = -1
MAX_SPLIT = 64                    # norm.hip: the workspace holds up to B * MAX_SPLIT split partials


def _dev():
    return torch.device("cuda:0")


def _p(a, name, off=0):
    return c_void_p(a.buf.data_ptr() + a.spans[name][0] + off)


def holds_poison(t, k=0):
    es = t.element_size()
    return bool((t.view(_INT[es]) == POISON[es][k]).all())


def leading_finite(t):
    """Number of leading finite elements of a 1-D tensor."""
    f = torch.isfinite(t).to(torch.int64)
    return int(torch.cumprod(f, 0).sum())


def refused(L, rc, outputs, label, code=None, text=None):
    """A refused launch: rc is `code` (or any non-zero with `text` in munit_last_error), every output keeps payload 0 and the
    workspace (if any) its NaN bytes."""
    a = L.a
    torch.cuda.synchronize()
    if code is not None:
        assert rc == code, "%s %s: rc=%d, expected %d" % (L.what, label, rc, code)
    else:
        assert rc != 0, "%s %s: accepted" % (L.what, label)
    if text is not None:
        msg = (_lib.load().munit_last_error() or b"").decode()
        assert text in msg, "%s %s: error text %r" % (L.what, label, msg)
    for o in outputs:
        assert holds_poison(_out_view(a, o)), "%s %s: %s written before the refusal" % (L.what, label, o)
    if "ws" in a.spans:
        assert bool((a.bytes("ws") == GUARD_BYTE).all()), "%s %s: workspace written before the refusal" % (L.what, label)
    L.verify(label + " (refused)")


_ES = {}                          # region name -> element size of its outputs, per arena


def _out_view(a, name):
    return a.bytes(name).view(_INT[_ES.get((id(a), name), 4)])


def _outs(a, **es):
    for n, e in es.items():
        _ES[(id(a), n)] = e


# ------------------------------------------------------------------------------------------------------------------------
# normalisation
# ------------------------------------------------------------------------------------------------------------------------
def _two_payloads(L, launch, outs, label):
    """Launch with outputs poisoned by payload 0, then by payload 1: NaN-free, bitwise equal.  Returns the results."""
    a = L.a
    res = []
    for k in (0, 1):
        for o in outs:
            poison(a.view(o, torch.float32) if _ES.get((id(a), o), 4) == 4 else a.view(o, torch.bfloat16), k)
        a.bytes("ws").fill_(GUARD_BYTE)
        L.after(launch(), "%s, payload %d" % (label, k))
        cur = {o: a.bytes(o).clone() for o in outs}
        cur["ws"] = a.bytes("ws").clone()
        for o in outs:
            assert no_nan(_float(a, o)), "%s %s: NaN in %s (an element not written, or poison read)" % (L.what, label, o)
        res.append(cur)
    for o in outs:
        assert torch.equal(res[0][o], res[1][o]), "%s %s: %s differs between two runs" % (L.what, label, o)
    assert torch.equal(res[0]["ws"], res[1]["ws"]), "%s %s: the workspace partials differ between two runs" % (L.what, label)
    return res[1]


def _float(a, o):
    return a.view(o, torch.float32) if _ES.get((id(a), o), 4) == 4 else a.view(o, torch.bfloat16)


def _partials(a, count_max):
    d = a.bytes("ws")[:count_max * 8].view(torch.float64)
    return leading_finite(d)


def check_instnorm(B, HW, C, bf16=False, adain=True, residual=True, relu=1):
    """munit_instnorm_{fwd,bwd}[_bf16] at (B, HW, C).  AdaIN parameters are columns of a row of ad_ld = 3C + 9 floats with
    b_off = 3, w_off = 2C + 5.  Returns (forward partial doubles, backward partial doubles) found in the workspace."""
    lib = _lib.load()
    es = 2 if bf16 else 4
    dt = torch.bfloat16 if bf16 else torch.float32
    ad_ld, b_off, w_off = 3 * C + 9, 3, 2 * C + 5
    n = B * HW * C
    nws = lib.munit_instnorm_workspace_bytes(B, HW, C)
    a = Arena(dict(x=n * es, res=n * es, dy=n * es, ad=B * ad_ld * 4, y=n * es, stats=B * C * 2 * 4, dx=n * es,
                   dad=B * ad_ld * 4, ws=nws), _dev())
    _outs(a, y=es, dx=es, stats=4, dad=4)
    x = a.view("x", dt)
    fill_random(x, 51)
    x.mul_(1.5).add_(0.25)
    fill_random(a.view("res", dt), 52)
    fill_random(a.view("dy", dt), 53)
    fill_random(a.view("ad", torch.float32), 54)
    a.view("ad", torch.float32).add_(0.5)
    what = "instnorm%s %s" % ("_bf16" if bf16 else "", (B, HW, C, "adain" if adain else "in", residual, relu))
    L = Launches(a, ["x", "res", "dy", "ad"], what, es)
    fwd = lib.munit_instnorm_fwd_bf16 if bf16 else lib.munit_instnorm_fwd
    bwd = lib.munit_instnorm_bwd_bf16 if bf16 else lib.munit_instnorm_bwd
    adp = _p(a, "ad") if adain else None

    def f(nb=nws):
        return fwd(_p(a, "x"), _p(a, "y"), _p(a, "stats"), B, HW, C, adp, ad_ld, w_off, b_off,
                   _p(a, "res") if residual else None, relu, c_float(1e-5), _p(a, "ws"), c_size_t(nb), stream())

    def b(nb=nws, d_adain=True):
        return bwd(_p(a, "x"), _p(a, "dy"), _p(a, "stats"), _p(a, "dx"), B, HW, C, adp,
                   _p(a, "dad") if (adain and d_adain) else None, ad_ld, w_off, b_off, relu, _p(a, "ws"), c_size_t(nb),
                   stream())

    cap = B * MAX_SPLIT * 2 * C
    r = _two_payloads(L, f, ["y", "stats"], "fwd")
    nf = _partials(a, cap)
    # backward: d_adain columns outside [w_off, w_off + C) and [b_off, b_off + C) keep their poison
    dad = a.view("dad", torch.float32).view(B, ad_ld)
    own = torch.zeros(ad_ld, dtype=torch.bool, device=dad.device)
    own[w_off:w_off + C] = True
    own[b_off:b_off + C] = True
    res = []
    for k in (0, 1):
        poison(a.view("dx", dt), k)
        poison(dad, k)
        a.bytes("ws").fill_(GUARD_BYTE)
        L.after(b(), "bwd, payload %d" % k)
        assert no_nan(a.view("dx", dt)), what + " bwd: NaN in dx"
        if adain:
            assert no_nan(dad[:, own]), what + " bwd: NaN in the d_adain columns of the layer"
        assert bool((dad[:, ~own].view(torch.int32) == POISON[4][k]).all()), \
            what + " bwd: d_adain written outside [w_off, w_off + C) and [b_off, b_off + C)"
        res.append((a.bytes("dx").clone(), a.bytes("dad").clone(), a.bytes("ws").clone()))
    assert torch.equal(res[0][0], res[1][0]), what + " bwd: dx differs between two runs"
    if adain:
        assert torch.equal(dad[:, own].clone().view(torch.int32), res[0][1].view(torch.int32).view(B, ad_ld)[:, own]), \
            what + " bwd: d_adain differs between two runs"
    else:
        assert holds_poison(dad, 1), what + " bwd: d_adain written although NULL"
    assert torch.equal(res[0][2], res[1][2]), what + " bwd: the workspace partials differ between two runs"
    nb = _partials(a, cap)
    if adain:     # d_adain == NULL: the same dx
        poison(a.view("dx", dt), 0)
        poison(dad, 0)
        a.bytes("ws").fill_(GUARD_BYTE)
        L.after(b(d_adain=False), "bwd, d_adain = NULL")
        assert torch.equal(a.bytes("dx"), res[1][0]), what + " bwd: dx with d_adain == NULL differs"
        assert holds_poison(dad), what + " bwd: d_adain written although NULL"
    # a workspace one byte short
    for o in ("y", "stats"):
        poison(_float(a, o), 0)
    a.bytes("ws").fill_(GUARD_BYTE)
    refused(L, f(nws - 1), ["y", "stats"], "fwd, workspace one byte short", code=ERR_WORKSPACE)
    a.bytes("stats").copy_(r["stats"])          # valid statistics in front of the refused backward
    L.inputs["stats"] = r["stats"].clone()
    poison(a.view("dx", dt), 0)
    poison(dad, 0)
    a.bytes("ws").fill_(GUARD_BYTE)
    refused(L, b(nws - 1), ["dx", "dad"], "bwd, workspace one byte short", code=ERR_WORKSPACE)
    return nf, nb


def check_layernorm(B, HW, C, bf16=False, relu=1):
    """munit_layernorm_{fwd,bwd}[_bf16] at (B, HW, C).  Returns (forward partial doubles, backward per-channel partial
    doubles) found in the workspace."""
    lib = _lib.load()
    es = 2 if bf16 else 4
    dt = torch.bfloat16 if bf16 else torch.float32
    n = B * HW * C
    nws = lib.munit_layernorm_workspace_bytes(B, HW, C)
    a = Arena(dict(x=n * es, dy=n * es, gamma=C * 4, beta=C * 4, prior_g=C * 4, prior_b=C * 4, y=n * es, stats=B * 2 * 4,
                   dx=n * es, dg=C * 4, db=C * 4, ws=nws), _dev())
    _outs(a, y=es, dx=es, stats=4, dg=4, db=4)
    fill_random(a.view("x", dt), 61)
    a.view("x", dt).mul_(2.0).sub_(0.7)
    fill_random(a.view("dy", dt), 62)
    for i, nm in enumerate(("gamma", "beta", "prior_g", "prior_b")):
        fill_random(a.view(nm, torch.float32), 63 + i)
    a.view("gamma", torch.float32).abs_().add_(0.1)
    what = "layernorm%s %s" % ("_bf16" if bf16 else "", (B, HW, C, relu))
    L = Launches(a, ["x", "dy", "gamma", "beta", "prior_g", "prior_b"], what, es)
    fwd = lib.munit_layernorm_fwd_bf16 if bf16 else lib.munit_layernorm_fwd
    bwd = lib.munit_layernorm_bwd_bf16 if bf16 else lib.munit_layernorm_bwd
    dg, db = a.view("dg", torch.float32), a.view("db", torch.float32)

    def f(nb=nws):
        return fwd(_p(a, "x"), _p(a, "y"), _p(a, "stats"), B, HW, C, _p(a, "gamma"), _p(a, "beta"), relu, c_float(1e-5),
                   _p(a, "ws"), c_size_t(nb), stream())

    def b(acc, nb=nws):
        return bwd(_p(a, "x"), _p(a, "dy"), _p(a, "stats"), _p(a, "dx"), B, HW, C, _p(a, "gamma"), _p(a, "beta"),
                   _p(a, "dg"), _p(a, "db"), c_float(acc), relu, c_float(1e-5), _p(a, "ws"), c_size_t(nb), stream())

    cap = B * MAX_SPLIT * 2 * C
    r = _two_payloads(L, f, ["y", "stats"], "fwd")
    nf = _partials(a, cap)
    for o in ("y", "stats"):
        poison(_float(a, o), 0)
    a.bytes("ws").fill_(GUARD_BYTE)
    refused(L, f(nws - 1), ["y", "stats"], "fwd, workspace one byte short", code=ERR_WORKSPACE)
    a.bytes("stats").copy_(r["stats"])
    L.inputs["stats"] = r["stats"].clone()
    rb = _two_payloads(L, lambda: b(0.0), ["dx", "dg", "db"], "bwd acc = 0 into NaN")
    nb = _partials(a, cap)
    # acc = 1 into a live buffer: exactly old + new (fp32)
    dg.copy_(a.view("prior_g", torch.float32))
    db.copy_(a.view("prior_b", torch.float32))
    a.bytes("ws").fill_(GUARD_BYTE)
    L.after(b(1.0), "bwd acc = 1")
    assert torch.equal(a.bytes("dx"), rb["dx"]), what + " bwd: dx depends on acc"
    assert bitwise_equal(dg, a.view("prior_g", torch.float32) + rb["dg"].view(torch.float32)), what + ": acc = 1 (dgamma)"
    assert bitwise_equal(db, a.view("prior_b", torch.float32) + rb["db"].view(torch.float32)), what + ": acc = 1 (dbeta)"
    for o in ("dx", "dg", "db"):
        poison(_float(a, o), 0)
    a.bytes("ws").fill_(GUARD_BYTE)
    refused(L, b(0.0, nws - 1), ["dx", "dg", "db"], "bwd, workspace one byte short", code=ERR_WORKSPACE)
    return nf, nb


# ------------------------------------------------------------------------------------------------------------------------
# pooling
# ------------------------------------------------------------------------------------------------------------------------
def _plain(sizes, inputs, outs, what, launches):
    """Entry points without a workspace: every (label, launch, outputs) of `launches` under two payloads."""
    a = Arena(sizes, _dev())
    _outs(a, **{o: 4 for o in outs})
    for i, n in enumerate(inputs):
        fill_random(a.view(n, torch.float32), 71 + i)
    L = Launches(a, inputs, what)
    for label, launch, o in launches(a):
        res = []
        for k in (0, 1):
            for nm in o:
                poison(a.view(nm, torch.float32), k)
            L.after(launch(), "%s, payload %d" % (label, k))
            for nm in o:
                assert no_nan(a.view(nm, torch.float32)), "%s %s: NaN in %s" % (what, label, nm)
            res.append([a.bytes(nm).clone() for nm in o])
        assert all(torch.equal(u, v) for u, v in zip(*res)), "%s %s: two runs differ" % (what, label)
    return a


def check_avgpool(B, H, W, C):
    lib = _lib.load()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    nx, ny = B * H * W * C, B * Ho * Wo * C
    _plain(dict(x=nx * 4, dy=ny * 4, y=ny * 4, dx=nx * 4), ["x", "dy"], ["y", "dx"], "avgpool3s2 %s" % ((B, H, W, C),),
           lambda a: [("fwd", lambda: lib.munit_avgpool3s2_fwd(_p(a, "x"), _p(a, "y"), B, H, W, C, stream()), ["y"]),
                      ("bwd", lambda: lib.munit_avgpool3s2_bwd(_p(a, "dy"), _p(a, "dx"), B, H, W, C, stream()), ["dx"])])


def check_gap(B, HW, C):
    lib = _lib.load()
    _plain(dict(x=B * HW * C * 4, dy=B * C * 4, y=B * C * 4, dx=B * HW * C * 4), ["x", "dy"], ["y", "dx"],
           "gap %s" % ((B, HW, C),),
           lambda a: [("fwd", lambda: lib.munit_gap_fwd(_p(a, "x"), _p(a, "y"), B, HW, C, stream()), ["y"]),
                      ("bwd", lambda: lib.munit_gap_bwd(_p(a, "dy"), _p(a, "dx"), B, HW, C, stream()), ["dx"])])


def check_act_bwd(n):
    lib = _lib.load()
    for act in range(4):
        a = _plain(dict(y=n * 4, dy=n * 4, dx=n * 4), ["y", "dy"], ["dx"], "act_bwd %d n=%d" % (act, n),
                   lambda a: [("act", lambda: lib.munit_act_bwd(act, c_float(0.2), _p(a, "y"), _p(a, "dy"), _p(a, "dx"),
                                                               c_size_t(n), stream()), ["dx"])])
        y, g = a.view("y", torch.float32), a.view("dy", torch.float32)
        want = (torch.where(y > 0, g, torch.zeros_like(g)) if act == 1 else
                torch.where(y > 0, g, g * 0.2) if act == 2 else g * (1.0 - y * y) if act == 3 else g)
        assert torch.equal(a.view("dx", torch.float32), want), "act_bwd %d n=%d: wrong values" % (act, n)


def check_scale(n):
    lib = _lib.load()
    a = Arena(dict(x=n * 4, prior=n * 4, y=n * 4), _dev())
    fill_random(a.view("x", torch.float32), 81)
    fill_random(a.view("prior", torch.float32), 82)
    x, y = a.view("x", torch.float32), a.view("y", torch.float32)
    L = Launches(a, ["x", "prior"], "scale n=%d" % n)
    for k in (0, 1):
        poison(y, k)
        L.after(lib.munit_scale(_p(a, "x"), _p(a, "y"), c_size_t(n), c_float(-0.75), 0, stream()), "acc = 0 into NaN")
        assert torch.equal(y, x * -0.75), "scale n=%d: accumulate = 0 must not read y" % n
    y.copy_(a.view("prior", torch.float32))
    L.after(lib.munit_scale(_p(a, "x"), _p(a, "y"), c_size_t(n), c_float(-0.75), 1, stream()), "acc = 1")
    assert torch.equal(y, x * -0.75 + a.view("prior", torch.float32)), "scale n=%d: accumulate = 1" % n


# ------------------------------------------------------------------------------------------------------------------------
# losses
# ------------------------------------------------------------------------------------------------------------------------
def check_l1(npix, C, masked, bf16=False):
    lib = _lib.load()
    es = 2 if bf16 else 4
    dt = torch.bfloat16 if bf16 else torch.float32
    n = npix * C
    nws = lib.munit_loss_workspace_bytes(c_size_t(n))
    a = Arena(dict(a=n * es, b=n * es, mask=npix * 4, gout=4, out=4, da=n * es, db=n * es, ws=nws), _dev())
    _outs(a, out=4, da=es, db=es)
    fill_random(a.view("a", dt), 91)
    fill_random(a.view("b", dt), 92)
    a.view("b", dt)[::7] = a.view("a", dt)[::7]             # exact ties: gradient 0
    a.view("mask", torch.float32).copy_((torch.arange(npix, device=_dev()) % 3 == 0).float())
    a.view("gout", torch.float32).fill_(3.0)
    what = "l1_mean%s %s" % ("_bf16" if bf16 else "", (npix, C, masked))
    L = Launches(a, ["a", "b", "mask", "gout"], what, es)
    fwd = lib.munit_l1_mean_fwd_bf16 if bf16 else lib.munit_l1_mean_fwd
    bwd = lib.munit_l1_mean_bwd_bf16 if bf16 else lib.munit_l1_mean_bwd
    m = _p(a, "mask") if masked else None

    def f(nb=nws):
        return fwd(_p(a, "a"), _p(a, "b"), m, c_size_t(npix), C, _p(a, "out"), _p(a, "ws"), c_size_t(nb), stream())

    _two_payloads(L, f, ["out"], "fwd")
    res = _two_payloads(L, lambda: bwd(_p(a, "a"), _p(a, "b"), m, c_size_t(npix), C, _p(a, "gout"), _p(a, "da"),
                                       _p(a, "db"), stream()), ["da", "db"], "bwd")
    assert torch.equal(a.view("db", dt), -a.view("da", dt)), what + ": db != -da"
    for keep, drop in (("da", "db"), ("db", "da")):
        poison(_float(a, keep), 0)
        poison(_float(a, drop), 0)
        L.after(bwd(_p(a, "a"), _p(a, "b"), m, c_size_t(npix), C, _p(a, "gout"), _p(a, "da") if keep == "da" else None,
                    _p(a, "db") if keep == "db" else None, stream()), "bwd, %s = NULL" % drop)
        assert torch.equal(a.bytes(keep), res[keep]), "%s: %s with %s == NULL differs" % (what, keep, drop)
        assert holds_poison(_float(a, drop)), "%s: %s written although NULL" % (what, drop)
    poison(a.view("out", torch.float32), 0)
    a.bytes("ws").fill_(GUARD_BYTE)
    refused(L, f(nws - 1), ["out"], "fwd, workspace one byte short", text="workspace too small")


def check_mse(n, target):
    lib = _lib.load()
    nws = lib.munit_loss_workspace_bytes(c_size_t(n))
    a = Arena(dict(x=n * 4, gout=4, out=4, dx=n * 4, ws=nws), _dev())
    _outs(a, out=4, dx=4)
    fill_random(a.view("x", torch.float32), 95)
    a.view("gout", torch.float32).fill_(0.5)
    what = "mse_const %s" % ((n, target),)
    L = Launches(a, ["x", "gout"], what)

    def f(nb=nws):
        return lib.munit_mse_const_fwd(_p(a, "x"), c_float(target), c_size_t(n), _p(a, "out"), _p(a, "ws"), c_size_t(nb),
                                       stream())

    _two_payloads(L, f, ["out"], "fwd")
    _two_payloads(L, lambda: lib.munit_mse_const_bwd(_p(a, "x"), c_float(target), c_size_t(n), _p(a, "gout"), _p(a, "dx"),
                                                     stream()), ["dx"], "bwd")
    poison(a.view("out", torch.float32), 0)
    a.bytes("ws").fill_(GUARD_BYTE)
    refused(L, f(nws - 1), ["out"], "fwd, workspace one byte short", text="workspace too small")


def check_weighted_sum():
    lib = _lib.load()
    a = Arena(dict(terms=33 * 4, out=4), _dev())
    _outs(a, out=4)
    t = a.view("terms", torch.float32)
    fill_random(t, 97)
    L = Launches(a, ["terms"], "weighted_sum")
    w = [0.5 + 0.25 * i for i in range(33)]
    ptrs = (c_void_p * 33)(*[a.buf.data_ptr() + a.spans["terms"][0] + 4 * i for i in range(33)])
    wts = (c_float * 33)(*w)
    for n in (1, 32):
        for k in (0, 1):
            poison(a.view("out", torch.float32), k)
            L.after(lib.munit_weighted_sum(ptrs, wts, n, _p(a, "out"), stream()), "n=%d" % n)
            want = sum(float(w[i]) * float(t[i]) for i in range(n))
            got = float(a.view("out", torch.float32))
            assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), ("weighted_sum", n, got, want)
    poison(a.view("out", torch.float32), 0)
    refused(L, lib.munit_weighted_sum(ptrs, wts, 33, _p(a, "out"), stream()), ["out"], "n=33", code=ERR_ARG)


# ------------------------------------------------------------------------------------------------------------------------
# optimisers
# ------------------------------------------------------------------------------------------------------------------------
def check_adam(n):
    lib = _lib.load()
    a = Arena(dict(p=n * 4, g=n * 4, m=n * 4, v=n * 4, ps=n * 4), _dev())
    fill_random(a.view("p", torch.float32), 101)
    fill_random(a.view("g", torch.float32), 102)
    fill_random(a.view("m", torch.float32), 103)
    fill_random(a.view("v", torch.float32), 104)
    a.view("m", torch.float32).mul_(0.1)
    a.view("v", torch.float32).abs_().mul_(0.01)
    start = {nm: a.bytes(nm).clone() for nm in ("p", "m", "v")}
    what = "adam n=%d" % n
    L = Launches(a, ["g"], what)

    def restore():
        for nm, s in start.items():
            a.bytes(nm).copy_(s)

    def adam(off=0, step=7):
        return lib.munit_adam_step(_p(a, "p", off), _p(a, "g", off), _p(a, "m", off), _p(a, "v", off), c_size_t(n - off // 4),
                                   c_double(1e-3), c_double(0.5), c_double(0.999), c_double(1e-8), c_double(1e-2), step,
                                   stream())

    res = []
    for _ in range(2):
        restore()
        L.after(adam(), "step")
        res.append([a.bytes(nm).clone() for nm in ("p", "m", "v")])
        assert all(no_nan(a.view(nm, torch.float32)) for nm in ("p", "m", "v")), what + ": NaN"
    assert all(torch.equal(u, v) for u, v in zip(*res)), what + ": two runs differ"
    if n > 1:
        restore()
        rc = adam(off=4)
        torch.cuda.synchronize()
        assert rc == ERR_ARG, (what, "misaligned buffers accepted", rc)
        assert "16-byte aligned" in (lib.munit_last_error() or b"").decode()
        assert all(torch.equal(a.bytes(nm), s) for nm, s in start.items()), what + ": written before the alignment refusal"
        L.verify("misaligned (refused)")

    # ExtraAdam: mode 0 saves p into p_saved, modes 1 / 2 leave p_saved alone; mode 2 restarts from p_saved
    ps = a.view("ps", torch.float32)

    def extra(mode, step):
        return lib.munit_extraadam_step(_p(a, "p"), _p(a, "g"), _p(a, "m"), _p(a, "v"), _p(a, "ps"), c_size_t(n),
                                        c_double(1e-3), c_double(0.5), c_double(0.999), c_double(1e-8), c_double(1e-2),
                                        step, mode, stream())
    what = "extraadam n=%d" % n
    L.what = what
    results = []
    for k in (0, 1):
        restore()
        poison(ps, k)
        p0 = a.bytes("p").clone()
        L.after(extra(0, 1), "mode 0")
        assert torch.equal(a.bytes("ps"), p0), what + ": mode 0 must save p"
        saved = a.bytes("ps").clone()
        L.after(extra(1, 2), "mode 1")
        assert torch.equal(a.bytes("ps"), saved), what + ": mode 1 wrote p_saved"
        L.after(extra(2, 3), "mode 2")
        assert torch.equal(a.bytes("ps"), saved), what + ": mode 2 wrote p_saved"
        assert all(no_nan(a.view(nm, torch.float32)) for nm in ("p", "m", "v")), what + ": NaN"
        results.append([a.bytes(nm).clone() for nm in ("p", "m", "v")])
    assert all(torch.equal(u, v) for u, v in zip(*results)), what + ": two runs differ"


# ------------------------------------------------------------------------------------------------------------------------
# image pipeline
# ------------------------------------------------------------------------------------------------------------------------
def check_image(B, out_h, out_w):
    """munit_image_preprocess / munit_mask_preprocess on B random images of other sizes (resize, crop, flip)."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(7)
    srcs = [(out_h + 5 + 3 * b, out_w + 11 - 2 * b) for b in range(B)]
    draws = [(b % 2, out_h + 2 + b, out_w + 1 + b, b, 1) for b in range(B)]   # flip, rs_h, rs_w, crop_i, crop_j
    offs, cur = [], 0
    for h, w in srcs:
        offs.append(cur)
        cur += (h * w * 3 + 15) // 16 * 16
    moffs = []
    for h, w in srcs:
        moffs.append(cur)
        cur += (h * w + 15) // 16 * 16
    descs = (_lib.ImageDesc * (2 * B))()
    ksize = 3
    for b, ((h, w), (fl, rh, rw, i, j)) in enumerate(zip(srcs, draws)):
        descs[b] = _lib.ImageDesc(offs[b], h, w, rh, rw, i, j, fl, 0)
        descs[B + b] = _lib.ImageDesc(moffs[b], h, w, 0, 0, i, j, fl, 0)
        ksize = max(ksize, lib.munit_image_ksize(h, rh), lib.munit_image_ksize(w, rw))
    nwi = lib.munit_image_preprocess_workspace_bytes(B, out_h, out_w, ksize)
    nwm = lib.munit_mask_preprocess_workspace_bytes(B, out_h, out_w)
    dsz = ctypes.sizeof(_lib.ImageDesc)
    a = Arena(dict(pool=cur, descs=2 * B * dsz, img=B * out_h * out_w * 3 * 4, mask=B * out_h * out_w * 4, ws=nwi,
                   wsm=nwm), _dev())
    _outs(a, img=4, mask=4)
    a.bytes("pool").copy_(torch.randint(0, 256, (cur,), generator=g, dtype=torch.uint8).to(_dev()))
    for b, (h, w) in enumerate(srcs):           # masks of 0 / 1 values: the x255 branch
        a.bytes("pool")[moffs[b]:moffs[b] + h * w] = a.bytes("pool")[moffs[b]:moffs[b] + h * w] & 1
    a.bytes("descs").copy_(torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(_dev()))
    what = "image_preprocess %s" % ((B, out_h, out_w),)
    L = Launches(a, ["pool", "descs"], what)

    def img(nb=nwi):
        a.bytes("ws").fill_(GUARD_BYTE)
        return lib.munit_image_preprocess(_p(a, "pool"), _p(a, "descs"), B, out_h, out_w, ksize, _p(a, "img"), _p(a, "ws"),
                                          c_size_t(nb), stream())

    def msk(nb=nwm):
        a.bytes("wsm").fill_(GUARD_BYTE)
        return lib.munit_mask_preprocess(_p(a, "pool"), _p(a, "descs", B * dsz), B, out_h, out_w, _p(a, "mask"),
                                         _p(a, "wsm"), c_size_t(nb), stream())

    for label, launch, o in (("image", img, "img"), ("mask", msk, "mask")):
        res = []
        for k in (0, 1):
            poison(a.view(o, torch.float32), k)
            L.after(launch(), "%s, payload %d" % (label, k))
            assert no_nan(a.view(o, torch.float32)), "%s: NaN in the %s output" % (what, label)
            res.append(a.bytes(o).clone())
        assert torch.equal(res[0], res[1]), "%s: two %s runs differ" % (what, label)
    assert float(a.view("img", torch.float32).abs().max()) <= 1.0
    for label, launch, o in (("image", img, "img"), ("mask", msk, "mask")):
        poison(a.view(o, torch.float32), 0)
        rc = launch(a.size("ws" if o == "img" else "wsm") - 1)
        torch.cuda.synchronize()
        assert rc == ERR_WORKSPACE, (what, label, rc)
        assert holds_poison(a.view(o, torch.float32)), "%s: %s written before the workspace refusal" % (what, label)
        L.verify(label + " one byte short (refused)")


# ------------------------------------------------------------------------------------------------------------------------
# the frozen segmentation network's kernels (munit_amd/csrc/seg.hip)
# ------------------------------------------------------------------------------------------------------------------------
SEG_GRID_CAP = 16384 * 256            # seg.hip: grid-stride loops of at most 16384 blocks of 256 threads
NCLS = 19
HEAD_LIMIT = 1 << 40


def _refusals(a, inputs, what, outs, calls, code=ERR_ARG):
    """Every (label, call) must be refused with `code` before anything is written."""
    L = Launches(a, inputs, what)
    for label, call in calls:
        for o in outs:
            poison(a.view(o, torch.float32), 0)
        refused(L, call(), outs, label, code=code)


def check_seg_input(npix):
    lib = _lib.load()
    n = 3 * npix
    what = "seg_input npix=%d" % npix
    a = _plain(dict(x=n * 4, dy=n * 4, y=n * 4, dx=n * 4), ["x", "dy"], ["y", "dx"], what,
               lambda a: [("fwd", lambda: lib.munit_seg_input_fwd(_p(a, "x"), _p(a, "y"), c_size_t(npix), stream()), ["y"]),
                          ("bwd", lambda: lib.munit_seg_input_bwd(_p(a, "dy"), _p(a, "dx"), c_size_t(npix), stream()), ["dx"])])
    _refusals(a, ["x", "dy"], what, ["y", "dx"],
              [("fwd, x = NULL", lambda: lib.munit_seg_input_fwd(None, _p(a, "y"), c_size_t(npix), stream())),
               ("fwd, y = NULL", lambda: lib.munit_seg_input_fwd(_p(a, "x"), None, c_size_t(npix), stream())),
               ("bwd, dy = NULL", lambda: lib.munit_seg_input_bwd(None, _p(a, "dx"), c_size_t(npix), stream())),
               ("bwd, dx = NULL", lambda: lib.munit_seg_input_bwd(_p(a, "dy"), None, c_size_t(npix), stream()))])


def check_space_to_batch(N, H, W, C, f):
    lib = _lib.load()
    n = N * H * W * C
    what = "space_to_batch %s" % ((N, H, W, C, f),)

    def s2b(a, src, dst, inv, h=H, w=W, ff=f):
        return lib.munit_space_to_batch(_p(a, src) if src else None, _p(a, dst) if dst else None, N, h, w, C, ff, inv, stream())

    a = _plain(dict(x=n * 4, y=n * 4, back=n * 4), ["x"], ["y", "back"], what,
               lambda a: [("split", lambda: s2b(a, "x", "y", 0), ["y"]), ("inverse", lambda: s2b(a, "y", "back", 1), ["back"])])
    assert torch.equal(a.bytes("back"), a.bytes("x")), what + ": the inverse does not restore the input"
    calls = [("x == y", lambda: s2b(a, "y", "y", 0)), ("inverse = 2", lambda: s2b(a, "x", "y", 2)),
             ("inverse = -1", lambda: s2b(a, "x", "y", -1)), ("x = NULL", lambda: s2b(a, None, "y", 0)),
             ("y = NULL", lambda: s2b(a, "x", None, 0)), ("f = 0", lambda: s2b(a, "x", "y", 0, ff=0))]
    if f > 1:
        calls += [("H % f", lambda: s2b(a, "x", "y", 0, h=H - 1)), ("W % f", lambda: s2b(a, "x", "y", 1, w=W - 1))]
    keep = a.bytes("y").clone()
    L = Launches(a, ["x"], what)
    for label, call in calls:
        poison(a.view("back", torch.float32), 0)
        refused(L, call(), ["back"], label, code=ERR_ARG)
        assert torch.equal(a.bytes("y"), keep), "%s %s: y written before the refusal" % (what, label)


def check_seg_maxpool(B, H, W, C):
    """munit_maxpool3s2_{fwd,bwd}: the uint8 winner plane is guarded like every tensor, prefilled with two out-of-range
    byte values, and every entry must come back in 0..8 naming an in-bounds element."""
    lib = _lib.load()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    nx, ny = B * H * W * C, B * Ho * Wo * C
    what = "maxpool3s2 %s" % ((B, H, W, C),)
    a = Arena(dict(x=nx * 4, dy=ny * 4, y=ny * 4, idx=ny, dx=nx * 4), _dev())
    _outs(a, y=4, dx=4)
    fill_random(a.view("x", torch.float32), 111)
    a.view("x", torch.float32).sub_(3.0)                # mostly negative: the zero padding must not win
    fill_random(a.view("dy", torch.float32), 112)
    L = Launches(a, ["x", "dy"], what)

    def f(x="x", y="y", idx="idx", b=B):
        return lib.munit_maxpool3s2_fwd(_p(a, x) if x else None, _p(a, y) if y else None, _p(a, idx) if idx else None, b, H,
                                        W, C, stream())

    def bw(dy="dy", idx="idx", dx="dx", c=C):
        return lib.munit_maxpool3s2_bwd(_p(a, dy) if dy else None, _p(a, idx) if idx else None, _p(a, dx) if dx else None, B,
                                        H, W, c, stream())

    res = []
    for k in (0, 1):
        poison(a.view("y", torch.float32), k)
        a.bytes("idx").fill_(0xE0 + k)
        L.after(f(), "fwd, payload %d" % k)
        assert no_nan(a.view("y", torch.float32)), what + " fwd: NaN in y"
        res.append((a.bytes("y").clone(), a.bytes("idx").clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), what + " fwd: two runs differ"
    win = a.bytes("idx").view(B, Ho, Wo, C).long()
    assert int(win.max()) <= 8, what + " fwd: a winner outside 0..8 (an entry not written)"
    row = 2 * torch.arange(Ho, device=win.device).view(1, Ho, 1, 1) - 1 + win // 3
    col = 2 * torch.arange(Wo, device=win.device).view(1, 1, Wo, 1) - 1 + win % 3
    assert bool(((row >= 0) & (row < H) & (col >= 0) & (col < W)).all()), what + " fwd: a winner outside the image"
    x = a.view("x", torch.float32).view(B, H, W, C)
    bi = torch.arange(B, device=win.device).view(B, 1, 1, 1).expand_as(win)
    ci = torch.arange(C, device=win.device).view(1, 1, 1, C).expand_as(win)
    assert torch.equal(x[bi, row, col, ci], a.view("y", torch.float32).view(B, Ho, Wo, C)), what + " fwd: y is not the winner"
    L.inputs["idx"] = a.bytes("idx").clone()
    res = []
    for k in (0, 1):
        poison(a.view("dx", torch.float32), k)
        L.after(bw(), "bwd, payload %d" % k)
        assert no_nan(a.view("dx", torch.float32)), what + " bwd: NaN in dx"
        res.append(a.bytes("dx").clone())
    assert torch.equal(res[0], res[1]), what + " bwd: two runs differ"
    for label, call in (("fwd, x = NULL", lambda: f(x=None)), ("fwd, y = NULL", lambda: f(y=None)),
                        ("fwd, idx = NULL", lambda: f(idx=None)), ("fwd, B = 0", lambda: f(b=0)),
                        ("bwd, dy = NULL", lambda: bw(dy=None)), ("bwd, idx = NULL", lambda: bw(idx=None)),
                        ("bwd, dx = NULL", lambda: bw(dx=None)), ("bwd, C = 0", lambda: bw(c=0))):
        poison(a.view("y", torch.float32), 0)
        poison(a.view("dx", torch.float32), 0)
        refused(L, call(), ["y", "dx"], label, code=ERR_ARG)


def check_add_relu(n):
    lib = _lib.load()
    what = "add_relu n=%d" % n

    def f(a, x="a", r="r", y="y", m=n):
        return lib.munit_add_relu_fwd(_p(a, x) if x else None, _p(a, r) if r else None, _p(a, y) if y else None, c_size_t(m),
                                      stream())

    a = _plain(dict(a=n * 4, r=n * 4, y=n * 4), ["a", "r"], ["y"], what, lambda a: [("fwd", lambda: f(a), ["y"])])
    s = a.view("a", torch.float32) + a.view("r", torch.float32)
    assert torch.equal(a.view("y", torch.float32), torch.where(s > 0, s, torch.zeros_like(s))), what + ": wrong values"
    _refusals(a, ["a", "r"], what, ["y"],
              [("n % 4 = 1", lambda: f(a, m=n + 1)), ("n % 4 = 3", lambda: f(a, m=n - 1)), ("a = NULL", lambda: f(a, x=None)),
               ("r = NULL", lambda: f(a, r=None)), ("y = NULL", lambda: f(a, y=None))])


def check_seg_head(B, h, w, S, masked):
    """munit_seg_ce_fwd / _bwd / munit_seg_labels / munit_seg_ce_workspace_bytes at (B, h, w, S)."""
    lib = _lib.load()
    npix = B * h * S * w * S
    nl = B * h * w * NCLS
    nws = lib.munit_seg_ce_workspace_bytes(B, h, w, S)
    # Each pass's own need restates seg.hip's layout on purpose (one fp32 partial per block of grid_for(npix); the gradient
    # at the up-sampled resolution): the header has one query for both passes, so "one byte short of its own need" can only
    # be probed this way.  A change of that layout has to change these two lines with it.
    need_f = max(1, min((npix + 255) // 256, 16384)) * 4          # one partial sum per block
    need_b = npix * NCLS * 4                                      # the gradient at the up-sampled resolution
    assert nws >= need_f and nws >= need_b, (nws, need_f, need_b)
    a = Arena(dict(lg=nl * 4, labels=npix * 4, mask=npix * 4, gout=4, out=4, dl=nl * 4, lab=npix * 4, ws=nws), _dev())
    _outs(a, out=4, dl=4, lab=4)
    fill_random(a.view("lg", torch.float32), 121)
    a.view("lg", torch.float32).mul_(3.0)
    g = torch.Generator(device=_dev()).manual_seed(122)
    a.view("labels", torch.int32).copy_(torch.randint(0, NCLS, (npix,), generator=g, device=_dev(), dtype=torch.int32))
    a.view("mask", torch.float32).copy_((torch.rand(npix, generator=g, device=_dev()) < 0.4).float())
    a.view("gout", torch.float32).fill_(1.5)
    what = "seg head %s" % ((B, h, w, S, masked),)
    L = Launches(a, ["lg", "labels", "mask", "gout"], what)
    norm = float(npix)

    def args(lg="lg", labels="labels"):
        return (_p(a, lg) if lg else None, _p(a, labels) if labels else None, _p(a, "mask") if masked else None)

    def f(nb=nws, nrm=norm, out="out", ws="ws", dims=(B, h, w, S), **kw):
        return lib.munit_seg_ce_fwd(*args(**kw), *dims, c_float(nrm), _p(a, out) if out else None, _p(a, ws) if ws else None,
                                    c_size_t(nb), stream())

    def bw(nb=nws, nrm=norm, gout="gout", dl="dl", ws="ws", dims=(B, h, w, S), **kw):
        return lib.munit_seg_ce_bwd(*args(**kw), *dims, c_float(nrm), _p(a, gout) if gout else None,
                                    _p(a, dl) if dl else None, _p(a, ws) if ws else None, c_size_t(nb), stream())

    def labels(lg="lg", lab="lab", dims=(B, h, w, S)):
        return lib.munit_seg_labels(_p(a, lg) if lg else None, *dims, _p(a, lab) if lab else None, stream())

    r = _two_payloads(L, f, ["out"], "fwd")
    for fill in (0x00, 0x3F):                   # the loss does not depend on what the workspace held
        poison(a.view("out", torch.float32), 0)
        a.bytes("ws").fill_(fill)
        L.after(f(), "fwd, workspace of 0x%02x bytes" % fill)
        assert torch.equal(a.bytes("out"), r["out"]), what + ": the loss depends on the workspace's content"
    L.after(f(need_f), "fwd, exactly its own need")
    assert torch.equal(a.bytes("out"), r["out"])
    _two_payloads(L, bw, ["dl"], "bwd")
    res = []
    for k in (0, 1):
        poison(a.view("lab", torch.float32), k)
        L.after(labels(), "labels, payload %d" % k)
        lab = a.view("lab", torch.int32)
        assert int(lab.min()) >= 0 and int(lab.max()) < NCLS, what + ": a label outside 0..18 (an entry not written)"
        res.append(a.bytes("lab").clone())
    assert torch.equal(res[0], res[1]), what + ": two label runs differ"

    def refuse(call, label, code=ERR_ARG):
        for o in ("out", "dl", "lab"):
            poison(a.view(o, torch.float32), 0)
        a.bytes("ws").fill_(GUARD_BYTE)
        refused(L, call(), ["out", "dl", "lab"], label, code=code)

    # each pass refuses a workspace one byte short of ITS OWN need
    refuse(lambda: f(need_f - 1), "fwd, workspace one byte short", ERR_WORKSPACE)
    refuse(lambda: bw(need_b - 1), "bwd, workspace one byte short", ERR_WORKSPACE)
    big = (4096, 4096, 4096, 8)                 # 2^36 * 64 pixels: over the 2^40 limit; refused before any launch
    assert big[0] * big[1] * big[2] * big[3] * big[3] * NCLS >= HEAD_LIMIT
    for label, call in (("fwd, logits = NULL", lambda: f(lg=None)), ("fwd, labels = NULL", lambda: f(labels=None)),
                        ("fwd, out = NULL", lambda: f(out=None)), ("fwd, ws = NULL", lambda: f(ws=None)),
                        ("fwd, norm = 0", lambda: f(nrm=0.0)), ("fwd, norm < 0", lambda: f(nrm=-1.0)),
                        ("fwd, B = 0", lambda: f(dims=(0, h, w, S))), ("fwd, S = 0", lambda: f(dims=(B, h, w, 0))),
                        ("fwd, too large", lambda: f(dims=big)),
                        ("bwd, logits = NULL", lambda: bw(lg=None)), ("bwd, labels = NULL", lambda: bw(labels=None)),
                        ("bwd, gout = NULL", lambda: bw(gout=None)), ("bwd, dlogits = NULL", lambda: bw(dl=None)),
                        ("bwd, ws = NULL", lambda: bw(ws=None)), ("bwd, norm = 0", lambda: bw(nrm=0.0)),
                        ("bwd, h = 0", lambda: bw(dims=(B, 0, w, S))), ("bwd, too large", lambda: bw(dims=big)),
                        ("labels, logits = NULL", lambda: labels(lg=None)), ("labels, labels = NULL", lambda: labels(lab=None)),
                        ("labels, w = 0", lambda: labels(dims=(B, h, 0, S))), ("labels, too large", lambda: labels(dims=big))):
        refuse(call, label)
