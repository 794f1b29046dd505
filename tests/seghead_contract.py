"""Contract checks of the trainable segmentation head's entry points -- munit_avgpool7_fwd / _bwd and
munit_seg_ce_direct_fwd / _bwd (seg.hip) -- called straight through ctypes, with tests/kernel_contract.py's harness (guard
bands around every region, NaN-poisoned workspace, two output payloads, refusals that leave every output untouched).

Not a test module: tests/test_gpu_seghead.py runs these."""
from ctypes import c_float, c_size_t

import torch

from munit_amd import _lib
from tests.conv_contract import ERR_WORKSPACE, GUARD_BYTE, Arena, Launches, fill_random, poison, stream
from tests.kernel_contract import ERR_ARG, HEAD_LIMIT, _dev, _outs, _p, _plain, _refusals, _two_payloads, refused

POOL_GRID_CAP = 2048 * 256            # seg.hip: the pool's grid-stride loop runs on at most 2048 blocks of 256 threads
POOL_ROWS = 8                         # ... one thread per 4 channels of one column of a strip of 8 rows


def pool_items(B, H, W, C):
    return B * ((H + POOL_ROWS - 1) // POOL_ROWS) * W * (C // 4)


def check_avgpool7(B, H, W, C):
    lib = _lib.load()
    n = B * H * W * C
    what = "avgpool7 %s" % ((B, H, W, C),)

    def f(a, x="x", y="y", dims=(B, H, W, C)):
        return lib.munit_avgpool7_fwd(_p(a, x) if x else None, _p(a, y) if y else None, *dims, stream())

    def b(a, dy="dy", dx="dx", dims=(B, H, W, C)):
        return lib.munit_avgpool7_bwd(_p(a, dy) if dy else None, _p(a, dx) if dx else None, *dims, stream())

    a = _plain(dict(x=n * 4, dy=n * 4, y=n * 4, dx=n * 4), ["x", "dy"], ["y", "dx"], what,
               lambda a: [("fwd", lambda: f(a), ["y"]), ("bwd", lambda: b(a), ["dx"])])
    _refusals(a, ["x", "dy"], what, ["y", "dx"],
              [("fwd, x = NULL", lambda: f(a, x=None)), ("fwd, y = NULL", lambda: f(a, y=None)),
               ("fwd, x == y", lambda: f(a, x="y")), ("fwd, B = 0", lambda: f(a, dims=(0, H, W, C))),
               ("fwd, H = 0", lambda: f(a, dims=(B, 0, W, C))), ("fwd, W = -1", lambda: f(a, dims=(B, H, -1, C))),
               ("fwd, C = 0", lambda: f(a, dims=(B, H, W, 0))), ("fwd, C % 4 = 2", lambda: f(a, dims=(B, H, W, C + 2))),
               ("fwd, too large", lambda: f(a, dims=(1 << 14, 1 << 14, 1 << 10, 4))),
               ("bwd, dy = NULL", lambda: b(a, dy=None)), ("bwd, dx = NULL", lambda: b(a, dx=None)),
               ("bwd, dy == dx", lambda: b(a, dy="dx")), ("bwd, C % 4 = 1", lambda: b(a, dims=(B, H, W, C + 1))),
               ("bwd, H = 0", lambda: b(a, dims=(B, 0, W, C)))])


def check_direct_head(B, h, w, S, K):
    """munit_seg_ce_direct_fwd / _bwd at (B, h, w, S, K) with munit_seg_ce_direct_workspace_bytes."""
    lib = _lib.load()
    npix = B * h * S * w * S
    nl = B * h * w * K
    nws = lib.munit_seg_ce_direct_workspace_bytes(B, h, w, S, K)
    # each pass's own need, restated from seg.hip's layout as tests/kernel_contract.check_seg_head does
    need_f = max(1, min((npix + 255) // 256, 16384)) * 4
    need_b = npix * K * 4
    assert nws >= need_f and nws >= need_b, (nws, need_f, need_b)
    a = Arena(dict(lg=nl * 4, gt=npix * 4, gout=4, out=4, dl=nl * 4, ws=nws), _dev())
    _outs(a, out=4, dl=4)
    fill_random(a.view("lg", torch.float32), 151)
    a.view("lg", torch.float32).mul_(3.0)
    g = torch.Generator(device=_dev()).manual_seed(152)
    a.view("gt", torch.float32).copy_(torch.randint(0, K, (npix,), generator=g, device=_dev()).float())
    a.view("gout", torch.float32).fill_(1.5)
    what = "seg direct head %s" % ((B, h, w, S, K),)
    L = Launches(a, ["lg", "gt", "gout"], what)
    norm = float(npix)

    def f(nb=nws, nrm=norm, dims=(B, h, w, S, K), **null):
        ptr = lambda nm: None if null.get(nm) else _p(a, nm)
        return lib.munit_seg_ce_direct_fwd(ptr("lg"), ptr("gt"), *dims, c_float(nrm), ptr("out"), ptr("ws"), c_size_t(nb),
                                           stream())

    def bw(nb=nws, nrm=norm, dims=(B, h, w, S, K), **null):
        ptr = lambda nm: None if null.get(nm) else _p(a, nm)
        return lib.munit_seg_ce_direct_bwd(ptr("lg"), ptr("gt"), *dims, c_float(nrm), ptr("gout"), ptr("dl"), ptr("ws"),
                                           c_size_t(nb), stream())

    r = _two_payloads(L, f, ["out"], "fwd")
    for fill in (0x00, 0x3F):                   # the loss does not depend on what the workspace held
        poison(a.view("out", torch.float32), 0)
        a.bytes("ws").fill_(fill)
        L.after(f(), "fwd, workspace of 0x%02x bytes" % fill)
        assert torch.equal(a.bytes("out"), r["out"]), what + ": the loss depends on the workspace's content"
    L.after(f(need_f), "fwd, exactly its own need")
    assert torch.equal(a.bytes("out"), r["out"])
    rb = _two_payloads(L, bw, ["dl"], "bwd")
    L.after(bw(need_b), "bwd, exactly its own need")
    assert torch.equal(a.bytes("dl"), rb["dl"])

    def refuse(call, label, code=ERR_ARG):
        for o in ("out", "dl"):
            poison(a.view(o, torch.float32), 0)
        a.bytes("ws").fill_(GUARD_BYTE)
        refused(L, call(), ["out", "dl"], label, code=code)

    refuse(lambda: f(need_f - 1), "fwd, workspace one byte short", ERR_WORKSPACE)
    refuse(lambda: bw(need_b - 1), "bwd, workspace one byte short", ERR_WORKSPACE)
    big = (4096, 4096, 4096, 8, K)
    assert big[0] * big[1] * big[2] * big[3] * big[3] * K >= HEAD_LIMIT
    for label, call in (("fwd, logits = NULL", lambda: f(lg=True)), ("fwd, gt = NULL", lambda: f(gt=True)),
                        ("fwd, out = NULL", lambda: f(out=True)), ("fwd, ws = NULL", lambda: f(ws=True)),
                        ("fwd, norm = 0", lambda: f(nrm=0.0)), ("fwd, norm < 0", lambda: f(nrm=-1.0)),
                        ("fwd, B = 0", lambda: f(dims=(0, h, w, S, K))), ("fwd, w = -1", lambda: f(dims=(B, h, -1, S, K))),
                        ("fwd, S = 0", lambda: f(dims=(B, h, w, 0, K))), ("fwd, S = 3", lambda: f(dims=(B, h, w, 3, K))),
                        ("fwd, S = 16", lambda: f(dims=(B, h, w, 16, K))), ("fwd, K = 1", lambda: f(dims=(B, h, w, S, 1))),
                        ("fwd, K = 33", lambda: f(dims=(B, h, w, S, 33))), ("fwd, too large", lambda: f(dims=big)),
                        ("bwd, logits = NULL", lambda: bw(lg=True)), ("bwd, gt = NULL", lambda: bw(gt=True)),
                        ("bwd, gout = NULL", lambda: bw(gout=True)), ("bwd, dlogits = NULL", lambda: bw(dl=True)),
                        ("bwd, ws = NULL", lambda: bw(ws=True)), ("bwd, norm = 0", lambda: bw(nrm=0.0)),
                        ("bwd, h = 0", lambda: bw(dims=(B, 0, w, S, K))), ("bwd, S = 5", lambda: bw(dims=(B, h, w, 5, K))),
                        ("bwd, K = 0", lambda: bw(dims=(B, h, w, S, 0))), ("bwd, K = 64", lambda: bw(dims=(B, h, w, S, 64))),
                        ("bwd, too large", lambda: bw(dims=big))):
        refuse(call, label)
