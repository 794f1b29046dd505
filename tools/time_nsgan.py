"""Time the multi-scale nsgan loss pair (munit_nsgan_fwd + munit_nsgan_bwd) against the LSGAN pair (munit_lsgan_*) on the
same segments of one device, alternating the two in one process.

  python tools/time_nsgan.py [--rounds 11] [--inner 200] [--warmup 20]

Shapes: the loss of a dis_update of config_256.yaml at batch 8 -- one discriminator pass over [fake; real], three scales of
16x16, 8x8 and 4x4 maps, six segments -- and one segment of 2^20 elements.  A round times `inner` forward + backward call
pairs between two device events and reports the time per pair; the two losses take turns round by round.  Prints one JSON
line: per shape and loss the median and min .. max over the rounds, in microseconds per forward + backward pair."""
import argparse
import json
import os
import statistics
import sys
from ctypes import c_float, c_size_t, c_void_p

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if args.rounds < 9:
        sys.exit("at least 9 rounds")
    from munit_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    batch, size, n_layer, scales = 8, 256, 4, 3
    maps = [(size >> s) >> n_layer for s in range(scales)]
    shapes = {"dis_update_256_b8": [batch * m * m for m in maps for _ in (0, 1)], "one_segment_1m": [1 << 20]}
    p = lambda t: c_void_p(t.data_ptr())
    stream = c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = {"rounds": args.rounds, "inner": args.inner, "unit": "us per forward + backward pair"}
    for name, sizes in shapes.items():
        n = len(sizes)
        g = torch.Generator().manual_seed(n)
        xs = [torch.randn(m, generator=g).to(dev) for m in sizes]
        dxs = [torch.empty_like(x) for x in xs]
        px, pd = (c_void_p * n)(*[x.data_ptr() for x in xs]), (c_void_p * n)(*[d.data_ptr() for d in dxs])
        pn, pt = (c_size_t * n)(*sizes), (c_float * n)(*[float(i % 2) for i in range(n)])
        res, gout = torch.empty(1, device=dev), torch.ones(1, device=dev)
        pairs = {}
        for kind in ("nsgan", "lsgan"):
            nws = getattr(lib, "munit_%s_workspace_bytes" % kind)(n)
            ws = torch.empty(nws, dtype=torch.uint8, device=dev)
            fwd, bwd = getattr(lib, "munit_%s_fwd" % kind), getattr(lib, "munit_%s_bwd" % kind)

            def pair(fwd=fwd, bwd=bwd, ws=ws, nws=nws, kind=kind):
                _lib.check(fwd(px, pn, pt, n, p(res), None, p(ws), nws, stream), kind + "_fwd")
                _lib.check(bwd(px, pn, pt, n, p(gout), pd, stream), kind + "_bwd")

            pairs[kind] = pair
        times = {k: [] for k in pairs}
        for fn in pairs.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for kind, fn in pairs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.inner):
                    fn()
                t1.record()
                t1.synchronize()
                times[kind].append(1e3 * t0.elapsed_time(t1) / args.inner)
        out[name] = {"segments": sizes}
        for kind, ts in times.items():
            out[name][kind] = dict(median=round(statistics.median(ts), 2), min=round(min(ts), 2), max=round(max(ts), 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
