"""Contract checks of the synthetic-pair step's entry points -- munit_pair_l1_fwd / _bwd (pointwise.hip) and
munit_seg_ce_gt_fwd / _bwd (seg.hip) -- called straight through ctypes, with tests/kernel_contract.py's harness (guard bands
around every region, NaN-poisoned workspace, two output payloads, refusals that leave every output untouched).

Not a test module: tests/test_gpu_synth.py runs these."""
from ctypes import c_float, c_size_t

import torch

from munit_amd import _lib
from tests.conv_contract import ERR_WORKSPACE, GUARD_BYTE, Arena, Launches, fill_random, poison, stream
from tests.kernel_contract import ERR_ARG, HEAD_LIMIT, NCLS, _dev, _outs, _p, _two_payloads, holds_poison, refused


def check_pair_l1(npix, C):
    lib = _lib.load()
    n = npix * C
    nws = lib.munit_loss_workspace_bytes(c_size_t(n))
    a = Arena(dict(xa=n * 4, xb=n * 4, xab=n * 4, xba=n * 4, gout=4, out=4, dab=n * 4, dba=n * 4, ws=nws), _dev())
    _outs(a, out=4, dab=4, dba=4)
    for i, nm in enumerate(("xa", "xb", "xab", "xba")):
        fill_random(a.view(nm, torch.float32), 131 + i)
    xa, xb = a.view("xa", torch.float32).view(npix, C), a.view("xb", torch.float32).view(npix, C)
    xb[::2] = xa[::2]                                                    # every other pixel aligned
    a.view("xab", torch.float32)[::5] = a.view("xb", torch.float32)[::5]   # exact ties: gradient 0
    a.view("gout", torch.float32).fill_(3.0)
    what = "pair_l1 %s" % ((npix, C),)
    ins = ["xa", "xb", "xab", "xba", "gout"]
    L = Launches(a, ins, what)

    def f(nb=nws, c=C, m=npix, **null):
        ptr = lambda nm: None if null.get(nm) else _p(a, nm)
        return lib.munit_pair_l1_fwd(ptr("xa"), ptr("xb"), ptr("xab"), ptr("xba"), c_size_t(m), c, ptr("out"), ptr("ws"),
                                     c_size_t(nb), stream())

    def b(c=C, m=npix, **null):
        ptr = lambda nm: None if null.get(nm) else _p(a, nm)
        return lib.munit_pair_l1_bwd(ptr("xa"), ptr("xb"), ptr("xab"), ptr("xba"), c_size_t(m), c, ptr("gout"), ptr("dab"),
                                     ptr("dba"), stream())

    r = _two_payloads(L, f, ["out"], "fwd")
    for fill in (0x00, 0x3F):                   # the loss does not depend on what the workspace held
        poison(a.view("out", torch.float32), 0)
        a.bytes("ws").fill_(fill)
        L.after(f(), "fwd, workspace of 0x%02x bytes" % fill)
        assert torch.equal(a.bytes("out"), r["out"]), what + ": the loss depends on the workspace's content"
    res = _two_payloads(L, b, ["dab", "dba"], "bwd")
    for keep, drop in (("dab", "dba"), ("dba", "dab")):
        poison(a.view(keep, torch.float32), 0)
        poison(a.view(drop, torch.float32), 0)
        L.after(b(**{drop: True}), "bwd, %s = NULL" % drop)
        assert torch.equal(a.bytes(keep), res[keep]), "%s: %s with %s == NULL differs" % (what, keep, drop)
        assert holds_poison(a.view(drop, torch.float32)), "%s: %s written although NULL" % (what, drop)

    def refuse(call, label, code=ERR_ARG, text=None):
        for o in ("out", "dab", "dba"):
            poison(a.view(o, torch.float32), 0)
        a.bytes("ws").fill_(GUARD_BYTE)
        refused(L, call(), ["out", "dab", "dba"], label, code=code, text=text)

    refuse(lambda: f(nws - 1), "fwd, workspace one byte short", code=None, text="workspace too small")
    for label, call in ([("fwd, %s = NULL" % nm, (lambda nm: lambda: f(**{nm: True}))(nm))
                         for nm in ("xa", "xb", "xab", "xba", "out", "ws")]
                        + [("bwd, %s = NULL" % nm, (lambda nm: lambda: b(**{nm: True}))(nm))
                           for nm in ("xa", "xb", "xab", "xba", "gout")]
                        + [("fwd, npix = 0", lambda: f(m=0)), ("fwd, C = 0", lambda: f(c=0)), ("fwd, C = 5", lambda: f(c=5)),
                           ("fwd, C = -1", lambda: f(c=-1)), ("bwd, npix = 0", lambda: b(m=0)), ("bwd, C = 0", lambda: b(c=0)),
                           ("bwd, C = 5", lambda: b(c=5))]):
        refuse(call, label)


def check_seg_gt_head(B, h, w, S, masked):
    """munit_seg_ce_gt_fwd / _bwd at (B, h, w, S) with munit_seg_ce_workspace_bytes."""
    lib = _lib.load()
    npix = B * h * S * w * S
    nl = B * h * w * NCLS
    nws = lib.munit_seg_ce_workspace_bytes(B, h, w, S)
    # each pass's own need, restated from seg.hip's layout as tests/kernel_contract.check_seg_head does
    need_f = max(1, min((npix + 255) // 256, 16384)) * 4
    need_b = npix * NCLS * 4
    assert nws >= need_f and nws >= need_b, (nws, need_f, need_b)
    a = Arena(dict(lg=nl * 4, gt=npix * 4, mask=npix * 4, gout=4, out=4, dl=nl * 4, ws=nws), _dev())
    _outs(a, out=4, dl=4)
    fill_random(a.view("lg", torch.float32), 141)
    a.view("lg", torch.float32).mul_(3.0)
    g = torch.Generator(device=_dev()).manual_seed(142)
    a.view("gt", torch.float32).copy_(torch.randint(0, 10, (npix,), generator=g, device=_dev()).float())
    a.view("mask", torch.float32).copy_((torch.rand(npix, generator=g, device=_dev()) < 0.4).float())
    a.view("gout", torch.float32).fill_(1.5)
    what = "seg gt head %s" % ((B, h, w, S, masked),)
    L = Launches(a, ["lg", "gt", "mask", "gout"], what)
    norm = float(npix)

    def args(null):
        return (None if null.get("lg") else _p(a, "lg"), None if null.get("gt") else _p(a, "gt"),
                _p(a, "mask") if masked else None)

    def f(nb=nws, nrm=norm, dims=(B, h, w, S), **null):
        ptr = lambda nm: None if null.get(nm) else _p(a, nm)
        return lib.munit_seg_ce_gt_fwd(*args(null), *dims, c_float(nrm), ptr("out"), ptr("ws"), c_size_t(nb), stream())

    def bw(nb=nws, nrm=norm, dims=(B, h, w, S), **null):
        ptr = lambda nm: None if null.get(nm) else _p(a, nm)
        return lib.munit_seg_ce_gt_bwd(*args(null), *dims, c_float(nrm), ptr("gout"), ptr("dl"), ptr("ws"), c_size_t(nb),
                                       stream())

    r = _two_payloads(L, f, ["out"], "fwd")
    for fill in (0x00, 0x3F):
        poison(a.view("out", torch.float32), 0)
        a.bytes("ws").fill_(fill)
        L.after(f(), "fwd, workspace of 0x%02x bytes" % fill)
        assert torch.equal(a.bytes("out"), r["out"]), what + ": the loss depends on the workspace's content"
    L.after(f(need_f), "fwd, exactly its own need")
    assert torch.equal(a.bytes("out"), r["out"])
    _two_payloads(L, bw, ["dl"], "bwd")

    def refuse(call, label, code=ERR_ARG):
        for o in ("out", "dl"):
            poison(a.view(o, torch.float32), 0)
        a.bytes("ws").fill_(GUARD_BYTE)
        refused(L, call(), ["out", "dl"], label, code=code)

    refuse(lambda: f(need_f - 1), "fwd, workspace one byte short", ERR_WORKSPACE)
    refuse(lambda: bw(need_b - 1), "bwd, workspace one byte short", ERR_WORKSPACE)
    big = (4096, 4096, 4096, 8)
    assert big[0] * big[1] * big[2] * big[3] * big[3] * NCLS >= HEAD_LIMIT
    for label, call in (("fwd, logits = NULL", lambda: f(lg=True)), ("fwd, gt = NULL", lambda: f(gt=True)),
                        ("fwd, out = NULL", lambda: f(out=True)), ("fwd, ws = NULL", lambda: f(ws=True)),
                        ("fwd, norm = 0", lambda: f(nrm=0.0)), ("fwd, norm < 0", lambda: f(nrm=-1.0)),
                        ("fwd, B = 0", lambda: f(dims=(0, h, w, S))), ("fwd, w = -1", lambda: f(dims=(B, h, -1, S))),
                        ("fwd, S = 0", lambda: f(dims=(B, h, w, 0))), ("fwd, too large", lambda: f(dims=big)),
                        ("bwd, logits = NULL", lambda: bw(lg=True)), ("bwd, gt = NULL", lambda: bw(gt=True)),
                        ("bwd, gout = NULL", lambda: bw(gout=True)), ("bwd, dlogits = NULL", lambda: bw(dl=True)),
                        ("bwd, ws = NULL", lambda: bw(ws=True)), ("bwd, norm = 0", lambda: bw(nrm=0.0)),
                        ("bwd, h = 0", lambda: bw(dims=(B, 0, w, S))), ("bwd, too large", lambda: bw(dims=big))):
        refuse(call, label)
