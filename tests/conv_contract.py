"""Contract checks of the convolution / linear C entry points (include/munit_hip.h), called straight through ctypes.

Not a test module: tests/test_gpu_ops.py runs these on every op case.  Accuracy is the op tests' business; what is checked
here is what the header promises and the trainer relies on, with guard bands and poison values standing in for a memory
checker (none can run on the GPU):
  * every input, output, workspace (exactly the reported *_workspace_bytes) and prepared image (exactly
    munit_conv2d_prepared_weight_bytes) is carved out of one larger allocation at a 4 KiB-aligned offset, between two guards
    of NaN bytes at least as large as the region (64 KiB .. 256 MiB): guards and inputs must be bitwise unchanged after
    every launch, and no NaN may reach an output (the workspace is NaN-poisoned before every launch, so a read of workspace
    the launch did not write, or of memory past a tensor, shows up in the result);
  * outputs prefilled with two different NaN payloads give bitwise equal, NaN-free results (every element written,
    deterministic split-K);
  * the *_prepared entry points with an image built by munit_conv2d_prepare_weights and by _prepare_weights_batch equal the
    wp == NULL calls bitwise;
  * backward-data's `add`, backward-weight's `beta` (0 into NaN, 1 into a live buffer) and db == NULL;
  * a workspace one byte short of the reported size is refused with MUNIT_ERR_WORKSPACE before anything is written."""
import ctypes
from ctypes import byref, c_float, c_size_t, c_void_p

import torch

from munit_amd import _lib, ops

KIB = 1 << 10
ALIGN = 4 * KIB
GUARD_MIN, GUARD_MAX = 64 * KIB, 256 * KIB * KIB
GUARD_BYTE = 0xFF                 # all-ones: a NaN in fp32 and in bf16
# two different NaN payloads to prefill outputs with (int32 / int16 bit patterns of fp32 / bf16 NaNs)
POISON = {4: (0x7FC00A5A, -0x005FF5A6), 2: (0x7FC1, -0x005E)}     # -0x005FF5A6 = 0xFFA00A5A, -0x005E = 0xFFA2
ERR_WORKSPACE = -2
_INT = {4: torch.int32, 2: torch.int16, 1: torch.uint8}


def _up(n, a=ALIGN):
    return (n + a - 1) // a * a


def guard_bytes(n):
    return _up(min(max(GUARD_MIN, n), GUARD_MAX))


class Arena(object):
    """Named regions of one device allocation, each between two guards of GUARD_BYTE; the trailing guard also covers the
    gap up to the next 4 KiB boundary."""

    def __init__(self, sizes, device):
        self.spans, off = {}, 0
        for name, n in sizes.items():
            g = guard_bytes(n)
            self.spans[name] = (off + g, n, g)
            off = _up(off + g + n) + g
        self.buf = torch.full((off,), GUARD_BYTE, dtype=torch.uint8, device=device)

    def bytes(self, name):
        s, n, _ = self.spans[name]
        return self.buf[s:s + n]

    def view(self, name, dtype):
        return self.bytes(name).view(dtype)

    def ptr(self, name):
        return c_void_p(self.buf.data_ptr() + self.spans[name][0])

    def size(self, name):
        return self.spans[name][1]

    def guards_intact(self):
        ok = []
        for s, n, g in self.spans.values():
            ok.append((self.buf[s - g:s] == GUARD_BYTE).all())
            ok.append((self.buf[s + n:_up(s + n) + g] == GUARD_BYTE).all())
        return bool(torch.stack(ok).all())


def fill_random(t, seed):
    g = torch.Generator(device=t.device).manual_seed(seed)
    t.copy_(torch.randn(t.shape, generator=g, device=t.device, dtype=torch.float32))


def poison(t, k):
    es = t.element_size()
    t.view(_INT[es]).fill_(POISON[es][k])


def bitwise_equal(a, b):
    return torch.equal(a.view(_INT[a.element_size()]), b.view(_INT[b.element_size()]))


def no_nan(t):
    return not bool(torch.isnan(t).any())


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


class Launches(object):
    """Inputs filled once and snapshotted; after every launch: guards intact, inputs unchanged."""

    def __init__(self, arena, inputs, what, out_es=4):
        self.a, self.what, self.out_es = arena, what, out_es
        self.inputs = {n: arena.bytes(n).clone() for n in inputs}

    def after(self, rc, label):
        _lib.check(rc, "%s %s" % (self.what, label))
        self.verify(label)

    def verify(self, label):
        torch.cuda.synchronize()
        assert self.a.guards_intact(), "%s %s: a guard band was written" % (self.what, label)
        for n, snap in self.inputs.items():
            assert torch.equal(self.a.bytes(n), snap), "%s %s: input %s was modified" % (self.what, label, n)

    def refused_short(self, call, outputs, label):
        """`call(ws_bytes)` prefills `outputs` with the first NaN payload and launches with one byte less than the reported
        workspace: it must return MUNIT_ERR_WORKSPACE and write nothing (outputs keep the payload, the workspace its NaN
        bytes)."""
        a = self.a
        n = a.size("ws")
        if n == 0:
            return
        rc = call(n - 1)
        assert rc == ERR_WORKSPACE, "%s %s: a workspace one byte short gave rc=%d" % (self.what, label, rc)
        torch.cuda.synchronize()
        for o in outputs:
            t = a.bytes(o).view(_INT[4 if o in ("dw", "db") else self.out_es])
            assert bool((t == POISON[t.element_size()][0]).all()), \
                "%s %s: %s written before the workspace refusal" % (self.what, label, o)
        assert bool((a.bytes("ws") == GUARD_BYTE).all()), "%s %s: workspace written before the refusal" % (self.what, label)
        self.verify(label + " (refused)")


def _prepare(lib, a, pl, which, w_name, names):
    """Build the weight image of pass `which` into region names[0] with munit_conv2d_prepare_weights and into each of
    names[1:] with ONE munit_conv2d_prepare_weights_batch launch over a device table of those items."""
    items = []
    for n in names:
        it = _lib.PrepItem()
        _lib.check(lib.munit_conv2d_prep_item(pl.ref, which, a.ptr(w_name), a.ptr(n), byref(it)), "conv2d_prep_item")
        items.append(it)
    _lib.check(lib.munit_conv2d_prepare_weights(byref(items[0]), stream()), "conv2d_prepare_weights")
    raw = b"".join(bytes(it) for it in items[1:])
    table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(a.buf.device)
    _lib.check(lib.munit_conv2d_prepare_weights_batch(c_void_p(table.data_ptr()), len(items) - 1, stream()),
               "conv2d_prepare_weights_batch")
    torch.cuda.synchronize()
    for n in names[1:]:
        assert torch.equal(a.bytes(n), a.bytes(names[0])), "the batched image %s differs from the single-layer one" % n
    return names


IMAGES = ("wp", "wp_b0", "wp_b1")


def check_fwd(pl, nx, ny, nw, cout, es, device, what):
    lib = _lib.load()
    nimg = pl.prep_bytes[0]
    sizes = dict(x=nx * es, w=nw * 4, bias=cout * 4, y=ny * (4 if pl.d.out_dtype == 0 else 2), ws=pl.ws_fwd)
    if nimg:
        sizes.update({n: nimg for n in IMAGES})
    a = Arena(sizes, device)
    xdt = torch.bfloat16 if pl.d.in_dtype else torch.float32
    ydt = torch.bfloat16 if pl.d.out_dtype else torch.float32
    fill_random(a.view("x", xdt), 11)
    fill_random(a.view("w", torch.float32), 12)
    fill_random(a.view("bias", torch.float32), 13)
    y = a.view("y", ydt)

    def run(wp, ws_bytes=None, k=0, label=""):
        a.bytes("ws").fill_(GUARD_BYTE)
        poison(y, k)
        return lib.munit_conv2d_fwd_prepared(pl.ref, a.ptr("x"), a.ptr("w"), wp, a.ptr("bias"), a.ptr("y"), a.ptr("ws"),
                                             c_size_t(a.size("ws") if ws_bytes is None else ws_bytes), stream())

    L = Launches(a, ["x", "w", "bias"], what + " fwd", y.element_size())
    a.bytes("ws").fill_(GUARD_BYTE)
    poison(y, 0)
    L.after(lib.munit_conv2d_fwd(pl.ref, a.ptr("x"), a.ptr("w"), a.ptr("bias"), a.ptr("y"), a.ptr("ws"),
                                 c_size_t(a.size("ws")), stream()), "plain")
    assert no_nan(y), what + " fwd: NaN in y"
    y0 = y.clone()
    L.after(run(None, k=1), "wp=NULL, second payload")
    assert bitwise_equal(y, y0), what + " fwd: two runs differ (or an element of y is not written)"
    if nimg:
        _prepare(lib, a, pl, 0, "w", IMAGES)
        L.inputs.update({n: a.bytes(n).clone() for n in IMAGES})
        for n in IMAGES:
            L.after(run(a.ptr(n), k=1), "prepared " + n)
            assert bitwise_equal(y, y0), "%s fwd: the prepared call with %s differs from wp=NULL" % (what, n)
    L.refused_short(lambda nb: run(None, nb, k=0), ["y"], "short workspace")


def check_dgrad(pl, nx, ny, nw, es, device, what, with_add=True):
    lib = _lib.load()
    nimg = pl.prep_bytes[1]
    dxdt = torch.bfloat16 if pl.d.in_dtype else torch.float32
    dydt = torch.bfloat16 if pl.d.out_dtype else torch.float32
    sizes = dict(dy=ny * (2 if pl.d.out_dtype else 4), w=nw * 4, add=nx * es, dx=nx * es, ws=pl.ws_dgrad)
    if nimg:
        sizes.update({n: nimg for n in IMAGES})
    a = Arena(sizes, device)
    fill_random(a.view("dy", dydt), 21)
    fill_random(a.view("w", torch.float32), 22)
    fill_random(a.view("add", dxdt), 23)
    dx = a.view("dx", dxdt)

    def run(wp, add, ws_bytes=None, k=0):
        a.bytes("ws").fill_(GUARD_BYTE)
        poison(dx, k)
        return lib.munit_conv2d_dgrad_prepared(pl.ref, a.ptr("dy"), a.ptr("w"), wp, a.ptr("add") if add else None,
                                               a.ptr("dx"), a.ptr("ws"),
                                               c_size_t(a.size("ws") if ws_bytes is None else ws_bytes), stream())

    L = Launches(a, ["dy", "w", "add"], what + " dgrad", dx.element_size())
    a.bytes("ws").fill_(GUARD_BYTE)
    poison(dx, 0)
    L.after(lib.munit_conv2d_dgrad(pl.ref, a.ptr("dy"), a.ptr("w"), None, a.ptr("dx"), a.ptr("ws"), c_size_t(a.size("ws")),
                                   stream()), "plain")
    assert no_nan(dx), what + " dgrad: NaN in dx"
    d0 = dx.clone()
    L.after(run(None, False, k=1), "wp=NULL, second payload")
    assert bitwise_equal(dx, d0), what + " dgrad: two runs differ (or an element of dx is not written)"
    da = None
    if with_add:
        L.after(run(None, True), "add")
        assert no_nan(dx), what + " dgrad: NaN in dx with add"
        assert bitwise_equal(dx, d0 + a.view("add", dxdt)), what + " dgrad: dgrad(add=a) != dgrad() + a"
        da = dx.clone()
    if nimg:
        _prepare(lib, a, pl, 1, "w", IMAGES)
        L.inputs.update({n: a.bytes(n).clone() for n in IMAGES})
        for n in IMAGES:
            L.after(run(a.ptr(n), False, k=1), "prepared " + n)
            assert bitwise_equal(dx, d0), "%s dgrad: the prepared call with %s differs from wp=NULL" % (what, n)
            if with_add:
                L.after(run(a.ptr(n), True), "prepared + add " + n)
                assert bitwise_equal(dx, da), "%s dgrad: the prepared call with %s and add differs" % (what, n)
    L.refused_short(lambda nb: run(None, with_add, nb), ["dx"], "short workspace")


def check_wgrad(pl, nx, ny, nw, cout, es, device, what):
    lib = _lib.load()
    xdt = torch.bfloat16 if pl.d.in_dtype else torch.float32
    dydt = torch.bfloat16 if pl.d.out_dtype else torch.float32
    a = Arena(dict(x=nx * es, dy=ny * (2 if pl.d.out_dtype else 4), prior_w=nw * 4, prior_b=cout * 4, dw=nw * 4,
                   db=cout * 4, ws=pl.ws_wgrad), device)
    fill_random(a.view("x", xdt), 31)
    fill_random(a.view("dy", dydt), 32)
    fill_random(a.view("prior_w", torch.float32), 33)
    fill_random(a.view("prior_b", torch.float32), 34)
    dw, db = a.view("dw", torch.float32), a.view("db", torch.float32)

    def run(beta, with_db=True, ws_bytes=None, fill=0):
        a.bytes("ws").fill_(GUARD_BYTE)
        if fill == "prior":
            dw.copy_(a.view("prior_w", torch.float32))
            db.copy_(a.view("prior_b", torch.float32))
        elif fill == "zero":
            dw.zero_()
            db.zero_()
        else:
            poison(dw, fill)
            poison(db, fill)
        return lib.munit_conv2d_wgrad(pl.ref, a.ptr("x"), a.ptr("dy"), a.ptr("dw"), a.ptr("db") if with_db else None,
                                      c_float(beta), a.ptr("ws"), c_size_t(a.size("ws") if ws_bytes is None else ws_bytes),
                                      stream())

    L = Launches(a, ["x", "dy", "prior_w", "prior_b"], what + " wgrad")
    L.after(run(0.0, fill=0), "beta=0 into NaN")
    assert no_nan(dw) and no_nan(db), what + " wgrad: NaN in dw / db (beta = 0 must not read the old values)"
    w0, b0 = dw.clone(), db.clone()
    L.after(run(0.0, fill=1), "beta=0 into the second NaN payload")
    assert bitwise_equal(dw, w0) and bitwise_equal(db, b0), what + " wgrad: two runs differ (not deterministic)"
    L.after(run(0.0, fill="zero"), "beta=0 into zeros")
    assert bitwise_equal(dw, w0) and bitwise_equal(db, b0), what + " wgrad: beta = 0 result depends on the old dw / db"
    L.after(run(1.0, fill="prior"), "beta=1")
    from tests.parity import nerr
    ew = nerr(dw, a.view("prior_w", torch.float32).double() + w0.double())
    eb = nerr(db, a.view("prior_b", torch.float32).double() + b0.double())
    assert ew <= 1e-6 and eb <= 1e-6, (what + " wgrad: beta = 1 does not accumulate", ew, eb)
    L.after(run(0.0, with_db=False, fill=0), "db=NULL")
    assert bitwise_equal(dw, w0), what + " wgrad: dw with db == NULL differs"
    assert bool((db.view(torch.int32) == POISON[4][0]).all()), what + " wgrad: db written although NULL"
    L.refused_short(lambda nb: run(0.0, ws_bytes=nb, fill=0), ["dw", "db"], "short workspace")


def check_conv_case(case, bf16=False):
    """All contract checks of one op case (cin, cout, k, stride, pad, pad_type, ups, act, B, H, W); bf16: the bf16-storage
    form (bf16 x / y / dy / dx, bf16 arithmetic; the activation stays unfused, as behind every bf16 layer of the trainer)."""
    cin, cout, k, stride, pad, pt, ups, act, b, h, w = case
    device = torch.device("cuda:0")
    prev = ops.get_compute()
    ops.set_compute("bf16s" if bf16 else "f32")
    try:
        dt = 1 if bf16 else 0
        pf = ops._plan(b, h, w, cin, cout, k, k, stride, pad, pt, bool(ups), "none" if bf16 else act, 0.2, dt, dt)
        pb = ops._plan(b, h, w, cin, cout, k, k, stride, pad, pt, bool(ups), "none", 0.2, dt, dt)
    finally:
        ops.set_compute(prev)
    nx, ny, nw = b * h * w * cin, b * pf.ho * pf.wo * cout, cout * k * k * cin
    es = 2 if bf16 else 4
    what = "%s%s" % ("bf16s " if bf16 else "", case)
    check_fwd(pf, nx, ny, nw, cout, es, device, what)
    # `add` exists for fp32 dx only: the trainer fuses the ResBlock skip gradient into fp32 layers (networks.py, ResBlock)
    check_dgrad(pb, nx, ny, nw, es, device, what, with_add=not bf16)
    check_wgrad(pb, nx, ny, nw, cout, es, device, what)


def check_linear(b, k, n, act):
    """munit_linear_fwd / munit_linear_bwd under the same checks.  Their workspace is the largest of the three passes'; one
    byte less may still be enough for a pass, so a short workspace must either give the full-size result bitwise or be
    refused with nothing written."""
    lib = _lib.load()
    device = torch.device("cuda:0")
    nws = lib.munit_linear_workspace_bytes(b, k, n)
    a = Arena(dict(x=b * k * 4, w=n * k * 4, bias=n * 4, dy=b * n * 4, prior_w=n * k * 4, prior_b=n * 4, y=b * n * 4,
                   dx=b * k * 4, dw=n * k * 4, db=n * 4, ws=nws), device)
    for i, name in enumerate(("x", "w", "bias", "dy", "prior_w", "prior_b")):
        fill_random(a.view(name, torch.float32), 41 + i)
    y, dx, dw, db = (a.view(nm, torch.float32) for nm in ("y", "dx", "dw", "db"))
    what = "linear %s" % ((b, k, n, act),)
    L = Launches(a, ["x", "w", "bias", "dy", "prior_w", "prior_b"], what)

    def fwd(k_, ws_bytes=nws):
        a.bytes("ws").fill_(GUARD_BYTE)
        poison(y, k_)
        return lib.munit_linear_fwd(a.ptr("x"), a.ptr("w"), a.ptr("bias"), a.ptr("y"), b, k, n, _lib.ACT[act], c_float(0.2),
                                    a.ptr("ws"), c_size_t(ws_bytes), stream())

    def bwd(beta, fill, with_dx=True, with_db=True, ws_bytes=nws):
        a.bytes("ws").fill_(GUARD_BYTE)
        poison(dx, fill if isinstance(fill, int) else 0)
        if fill == "prior":
            dw.copy_(a.view("prior_w", torch.float32))
            db.copy_(a.view("prior_b", torch.float32))
        else:
            poison(dw, fill)
            poison(db, fill)
        return lib.munit_linear_bwd(a.ptr("x"), a.ptr("w"), a.ptr("dy"), a.ptr("dx") if with_dx else None, a.ptr("dw"),
                                    a.ptr("db") if with_db else None, b, k, n, c_float(beta), a.ptr("ws"), c_size_t(ws_bytes),
                                    stream())

    L.after(fwd(0), "fwd")
    assert no_nan(y), what + ": NaN in y"
    y0 = y.clone()
    L.after(fwd(1), "fwd, second payload")
    assert bitwise_equal(y, y0), what + ": two forward runs differ"
    L.after(bwd(0.0, 0), "bwd")
    assert no_nan(dx) and no_nan(dw) and no_nan(db), what + ": NaN in dx / dw / db"
    g = [t.clone() for t in (dx, dw, db)]
    L.after(bwd(0.0, 1), "bwd, second payload")
    assert all(bitwise_equal(t, t0) for t, t0 in zip((dx, dw, db), g)), what + ": two backward runs differ"
    L.after(bwd(1.0, "prior"), "bwd beta=1")
    from tests.parity import nerr
    assert nerr(dw, a.view("prior_w", torch.float32).double() + g[1].double()) <= 1e-6, what + ": beta = 1 (dw)"
    assert nerr(db, a.view("prior_b", torch.float32).double() + g[2].double()) <= 1e-6, what + ": beta = 1 (db)"
    L.after(bwd(0.0, 0, with_dx=False, with_db=False), "bwd without dx and db")
    assert bitwise_equal(dw, g[1]), what + ": dw without dx / db differs"
    assert bool((dx.view(torch.int32) == POISON[4][0]).all()) and bool((db.view(torch.int32) == POISON[4][0]).all()), \
        what + ": dx / db written although NULL"
    if nws:
        for label, call, outs, ref in (("fwd", lambda: fwd(0, nws - 1), (y,), (y0,)),
                                       ("bwd", lambda: bwd(0.0, 0, ws_bytes=nws - 1), (dx, dw, db), g)):
            rc = call()
            torch.cuda.synchronize()
            if rc == 0:
                L.verify(label + " one byte short (accepted)")
                assert all(bitwise_equal(t, t0) for t, t0 in zip(outs, ref)), what + ": %s with a short workspace" % label
            else:
                assert rc == ERR_WORKSPACE, (what, label, rc)
                L.verify(label + " one byte short (refused)")
                assert all(bool((t.view(torch.int32) == POISON[4][0]).all()) for t in outs), \
                    what + ": %s wrote before refusing a short workspace" % label


class Calls(object):
    """Record the C entry points (by name prefix) called while active."""

    def __init__(self, prefixes):
        self.lib = _lib.load()
        self.names = [n for n in _lib.SIGNATURES if n.startswith(tuple(prefixes))]
        self.calls = []

    def __enter__(self):
        self.saved = {n: getattr(self.lib, n) for n in self.names}
        for n, f in self.saved.items():
            setattr(self.lib, n, (lambda f, n: lambda *a: self.calls.append(n) or f(*a))(f, n))
        return self.calls

    def __exit__(self, *exc):
        for n, f in self.saved.items():
            setattr(self.lib, n, f)
        return False
