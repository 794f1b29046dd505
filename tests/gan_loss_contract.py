"""What the multi-scale GAN-loss entry points (munit_lsgan_* / munit_nsgan_*) share, for tests/test_gpu_outda.py and
tests/test_gpu_nsgan.py: the ctypes call on 1-D device segments, and the alignment and guard-band contract.  A `Family` names
the three C symbols, the value an output holds before the call (so that an unwritten element shows) and the targets the
segments cycle over."""
import collections
from ctypes import c_float, c_size_t, c_void_p

import torch

from munit_amd import _lib
from tests.conv_contract import GUARD_BYTE, Arena, Launches, fill_random, no_nan, poison, stream

DEV = "cuda:0"
Family = collections.namedtuple("Family", "workspace_bytes fwd bwd fill targets")
LSGAN = Family("munit_lsgan_workspace_bytes", "munit_lsgan_fwd", "munit_lsgan_bwd", float("nan"), (0.0, 1.0, 0.5))
NSGAN = Family("munit_nsgan_workspace_bytes", "munit_nsgan_fwd", "munit_nsgan_bwd", 12345.0, (0.0, 1.0))


def cycle(fam, n):
    return [fam.targets[i % len(fam.targets)] for i in range(n)]


def arrays(xs, targets):
    n = len(xs)
    return ((c_void_p * n)(*[x.data_ptr() for x in xs]), (c_size_t * n)(*[x.numel() for x in xs]),
            (c_float * n)(*[float(t) for t in targets]))


def raw(fam, xs, targets, dxs=None, gout=1.0, with_seg=True):
    """fam's fwd + bwd through ctypes on 1-D device segments: out, seg_out, [dx_s]"""
    lib = _lib.load()
    n = len(xs)
    px, pn, pt = arrays(xs, targets)
    out = torch.full((1,), fam.fill, device=DEV)
    seg = torch.full((n,), fam.fill, device=DEV)
    nws = getattr(lib, fam.workspace_bytes)(n)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    p = lambda t: c_void_p(t.data_ptr())
    _lib.check(getattr(lib, fam.fwd)(px, pn, pt, n, p(out), p(seg) if with_seg else None, p(ws), nws, stream()), fam.fwd[6:])
    if dxs is None:
        dxs = [torch.full_like(x, fam.fill) for x in xs]
    g = torch.full((1,), gout, device=DEV)
    pd = (c_void_p * n)(*[d.data_ptr() for d in dxs])
    _lib.check(getattr(lib, fam.bwd)(px, pn, pt, n, p(g), pd, stream()), fam.bwd[6:])
    torch.cuda.synchronize()
    return out, seg, dxs


def segments(sizes, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [(scale * torch.randn(n, generator=g)).float() for n in sizes]


def check_unaligned_segment_starts(fam, scale=1.0):
    """Segments at float offsets 1, 2 and 3 (mod 4) of one allocation, sizes 1, 5 and 257; dx likewise."""
    sizes, offs, targets = [1, 5, 257], [1, 6, 15], cycle(fam, 3)
    host = segments(sizes, 5, scale)
    aligned = [x.to(DEV) for x in host]
    buf = torch.zeros(offs[-1] + sizes[-1] + 3, device=DEV)
    dbuf = torch.full_like(buf, 7.0)
    assert buf.data_ptr() % 16 == 0 and [o % 4 for o in offs] == [1, 2, 3]
    xs, dxs = [], []
    for x, o in zip(aligned, offs):
        buf[o:o + x.numel()].copy_(x)
        xs.append(buf[o:o + x.numel()])
        dxs.append(dbuf[o:o + x.numel()])
    out, seg, dx = raw(fam, aligned, targets, gout=0.75)
    out_u, seg_u, dx_u = raw(fam, xs, targets, dxs=dxs, gout=0.75)
    assert torch.equal(out, out_u) and torch.equal(seg, seg_u)
    for a, b in zip(dx, dx_u):
        assert torch.equal(a, b)
    covered = torch.zeros(buf.numel(), dtype=torch.bool, device=DEV)
    for o, n in zip(offs, sizes):
        covered[o:o + n] = True
    assert bool((dbuf[~covered] == 7.0).all())           # nothing written between the segments


def check_guard_bands(fam, sizes):
    lib = _lib.load()
    n = len(sizes)
    nws = getattr(lib, fam.workspace_bytes)(n)
    spans = {"gout": 4, "out": 4, "seg": 4 * n, "ws": nws}
    for i, m in enumerate(sizes):
        spans["x%d" % i], spans["dx%d" % i] = 4 * m, 4 * m
    a = Arena(spans, torch.device(DEV))
    for i in range(n):
        fill_random(a.view("x%d" % i, torch.float32), 80 + i)
    a.view("gout", torch.float32).fill_(1.5)
    px = (c_void_p * n)(*[a.ptr("x%d" % i).value for i in range(n)])
    pd = (c_void_p * n)(*[a.ptr("dx%d" % i).value for i in range(n)])
    pn, pt = (c_size_t * n)(*sizes), (c_float * n)(*cycle(fam, n))
    inputs = ["x%d" % i for i in range(n)] + ["gout"]
    fwd, bwd = getattr(lib, fam.fwd), getattr(lib, fam.bwd)
    for what, outs, launch in (
            (fam.fwd[6:], ["out", "seg"], lambda: fwd(px, pn, pt, n, a.ptr("out"), a.ptr("seg"), a.ptr("ws"), nws, stream())),
            (fam.bwd[6:], ["dx%d" % i for i in range(n)], lambda: bwd(px, pn, pt, n, a.ptr("gout"), pd, stream()))):
        L = Launches(a, inputs, "%s %s" % (what, sizes))
        res = []
        for k in (0, 1):
            for o in outs:
                poison(a.view(o, torch.float32), k)
            a.bytes("ws").fill_(GUARD_BYTE)
            L.after(launch(), "payload %d" % k)
            for o in outs:
                assert no_nan(a.view(o, torch.float32)), "%s: NaN in %s" % (what, o)
            res.append({o: a.bytes(o).clone() for o in outs})
        for o in outs:
            assert torch.equal(res[0][o], res[1][o]), "%s: %s differs between two runs" % (what, o)
