"""Time the cross-rank batch norm's kernel chain against the single-process entry points on one device, at the feature
classifier's shapes: munit_batchnorm_dp_stats_local + _fwd_apply + _bwd_local + _bwd_finish with W = 1 (every kernel of a
data-parallel pass, without the two collectives between the halves) against munit_batchnorm_fwd + munit_batchnorm_bwd.

  python tools/time_featda_dp.py [--reps 200] [--rounds 9] [--warmup 20]

The two chains alternate within a round; a round times `reps` back-to-back chains between two device events.  Prints one
JSON line: per shape the median over the rounds (and min .. max) of the per-chain time in microseconds, and the ratio of the
medians.  The all-reduce itself needs two devices and is not part of this figure."""
import argparse
import json
import os
import statistics
import sys
from ctypes import c_float, c_void_p

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(8 * 32 * 32, 128), (8 * 16 * 16, 64)]       # (R, C): the 128- and the 64-channel block at crop 256, batch 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    from munit_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    p = lambda t: c_void_p(t.data_ptr())
    st = lambda: c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"reps": args.reps, "rounds": args.rounds}
    for r, c in SHAPES:
        g = torch.Generator(device=dev).manual_seed(r + c)
        x, dy = torch.randn(r, c, device=dev, generator=g), torch.randn(r, c, device=dev, generator=g)
        gamma, beta = torch.rand(c, device=dev, generator=g) + 0.5, torch.rand(c, device=dev, generator=g)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        mean, rstd = torch.empty(2 * c, device=dev), torch.empty(2 * c, device=dev)
        rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
        dg, db = torch.empty(c, device=dev), torch.empty(c, device=dev)
        xch = torch.empty(4 * c, device=dev)
        nws1, nws = lib.munit_batchnorm_workspace_bytes(c), lib.munit_batchnorm_dp_workspace_bytes(c)
        ws = torch.empty(max(nws1, nws), dtype=torch.uint8, device=dev)     # the cross-rank backward's partials are doubles
        eps, mom, zero = c_float(1e-5), c_float(0.1), c_float(0.0)

        def plain():
            _lib.check(lib.munit_batchnorm_fwd(p(x), p(y), p(mean), p(rstd), p(rm), p(rv), r, c, p(gamma), p(beta), 1, 0, eps, mom,
                                               p(ws), nws1, st()), "fwd")
            _lib.check(lib.munit_batchnorm_bwd(p(x), p(dy), p(y), p(gamma), p(mean), p(rstd), p(dx), p(dg), p(db), zero, r, c, 1,
                                               p(ws), nws1, st()), "bwd")

        def cross():
            _lib.check(lib.munit_batchnorm_dp_stats_local(p(x), r, c, 1, 0, p(xch), xch.numel(), p(ws), nws, st()), "local")
            _lib.check(lib.munit_batchnorm_dp_fwd_apply(p(x), p(y), p(mean), p(rstd), p(rm), p(rv), r, c, 1, p(xch), xch.numel(),
                                                        p(gamma), p(beta), 1, eps, mom, st()), "apply")
            _lib.check(lib.munit_batchnorm_dp_bwd_local(p(x), p(dy), p(y), p(mean), p(rstd), r, c, 1, 1, 0, p(xch), xch.numel(),
                                                        p(ws), nws, st()), "bwd local")
            _lib.check(lib.munit_batchnorm_dp_bwd_finish(p(x), p(dy), p(y), p(gamma), p(mean), p(rstd), p(dx), p(dg), p(db), zero,
                                                         r, c, 1, 1, 0, p(xch), xch.numel(), p(ws), nws, st()), "bwd finish")

        plain()
        ref = (y.clone(), dx.clone())
        cross()
        torch.cuda.synchronize()
        # the same numbers to fp32 rounding (the merged M2 passes through one float per rank)
        err = max(float((y - ref[0]).abs().max() / ref[0].abs().max()), float((dx - ref[1]).abs().max() / ref[1].abs().max()))
        assert err <= 1e-5, err
        times = {"plain": [], "cross": []}
        for fn in (plain, cross):
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for name, fn in (("plain", plain), ("cross", cross)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(1e3 * e0.elapsed_time(e1) / args.reps)
        rec = {k: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
               for k, v in times.items()}
        rec["ratio"] = round(rec["cross"]["median_us"] / rec["plain"]["median_us"], 3)
        rec["max_rel_diff"] = err
        out["R%d_C%d" % (r, c)] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
