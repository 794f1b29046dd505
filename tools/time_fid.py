"""Time the FID kernels (csrc/fid.hip) at the width the evaluation runs at, D = 2048.

  python tools/time_fid.py [--rounds 9] [--inner 10] [--warmup 3] [--iters 400] [--n 900]

(a) one 2048^3 munit_gemm_f32 (A B and A^T B), in TFLOP/s and as a share of the 157.3 TFLOP/s the fp32 matrix instruction
    peaks at -- and, in the same process in alternating rounds, munit_linear_fwd at B = K = N = 2048, the library's only other
    dense product (it computes x w^T, so it is a yardstick for rate only);
(b) the two-problem launch of one Newton-Schulz iteration (Y T and T Z together);
(c) a whole munit_frechet_distance at D = 2048 with `iters` iterations, and munit_fid_moments at N = `n`.
A round times `inner` calls ((c): one call) between two device events; prints one JSON line with the median and min .. max
over the rounds."""
import argparse
import json
import os
import statistics
import sys
from ctypes import c_float, c_void_p

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PEAK_TFLOPS = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--n", type=int, default=900)
    ap.add_argument("--d", type=int, default=2048)
    args = ap.parse_args()
    if args.rounds < 9:
        sys.exit("at least 9 rounds")
    from munit_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    d = args.d
    p = lambda t: c_void_p(t.data_ptr())
    stream = c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator().manual_seed(3)
    mats = [(torch.rand(d, d, generator=g) * 2 - 1).to(dev) for _ in range(3)]
    outs = [torch.empty(d, d, device=dev) for _ in range(2)]
    flop = 2.0 * d * d * d

    def gemm(table, trans_a=0):
        prob = (_lib.GemmProblem * len(table))(*[_lib.GemmProblem(a.data_ptr(), b.data_ptr(), c.data_ptr()) for a, b, c in table])
        return lambda: _lib.check(lib.munit_gemm_f32(prob, len(table), d, d, d, d, d, d, trans_a, c_float(1.0), c_float(0.0),
                                                     stream), "gemm_f32")

    lin_ws = torch.empty(max(1, lib.munit_linear_workspace_bytes(d, d, d)), dtype=torch.uint8, device=dev)

    def linear():
        _lib.check(lib.munit_linear_fwd(p(mats[0]), p(mats[1]), None, p(outs[0]), d, d, d, 0, c_float(0.0), p(lin_ws),
                                        lin_ws.numel(), stream), "linear_fwd")

    def rounds(fns, inner):
        times = {k: [] for k in fns}
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for k, fn in fns.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(inner):
                    fn()
                t1.record()
                t1.synchronize()
                times[k].append(t0.elapsed_time(t1) / inner)
        return times

    def stats(ts, flops=None):
        r = dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))
        if flops is not None:
            r["tflops"] = round(flops / (statistics.median(ts) * 1e-3) / 1e12, 2)
            r["share_of_peak"] = round(r["tflops"] / PEAK_TFLOPS, 3)
        return r

    out = {"D": d, "rounds": args.rounds, "inner": args.inner, "peak_tflops": PEAK_TFLOPS}
    t = rounds({"gemm_f32": gemm([(mats[0], mats[1], outs[0])]), "gemm_f32_transA": gemm([(mats[0], mats[1], outs[0])], 1),
                "linear_fwd": linear, "gemm_f32_two_problems": gemm([(mats[0], mats[2], outs[0]), (mats[2], mats[1], outs[1])])},
               args.inner)
    out["a_one_product"] = {k: stats(t[k], flop) for k in ("gemm_f32", "gemm_f32_transA", "linear_fwd")}
    out["b_two_products_one_launch"] = stats(t["gemm_f32_two_problems"], 2 * flop)

    # (c): the moments kernel at N = n; the distance between the covariances of two pools of 4 D rows (non-singular)
    n = args.n

    def pool_pair(rows):
        return [(torch.randn(rows, d, generator=g) * (0.3 - 0.05 * i) + 0.4 + 0.1 * i).to(dev) for i in range(2)]

    mus = [torch.empty(d, device=dev) for _ in range(2)]
    sigmas = [torch.empty(d, d, device=dev) for _ in range(2)]

    def moments_of(pool, i):
        rows = pool.shape[0]
        ws = torch.empty(lib.munit_fid_moments_workspace_bytes(rows, d), dtype=torch.uint8, device=dev)
        return lambda: _lib.check(lib.munit_fid_moments(p(pool), rows, d, p(mus[i]), p(sigmas[i]), p(ws), ws.numel(), stream),
                                  "fid_moments")

    moments = moments_of(pool_pair(n)[0], 0)
    t = rounds({"fid_moments": moments}, args.inner)
    out["c_fid_moments"] = dict(stats(t["fid_moments"], 2.0 * d * d * n), N=n)
    for i, pool in enumerate(pool_pair(4 * d)):
        moments_of(pool, i)()
    torch.cuda.synchronize()
    fd_ws = torch.empty(lib.munit_frechet_distance_workspace_bytes(d), dtype=torch.uint8, device=dev)
    res = torch.empty(1, device=dev)

    def frechet():
        _lib.check(lib.munit_frechet_distance(p(mus[0]), p(sigmas[0]), p(mus[1]), p(sigmas[1]), d, args.iters, p(res), p(fd_ws),
                                              fd_ws.numel(), stream), "frechet_distance")

    args.warmup = 1
    t = rounds({"frechet_distance": frechet}, 1)
    out["c_frechet_distance"] = dict(stats(t["frechet_distance"], (1 + 3 * args.iters) * flop), iters=args.iters,
                                     value=float(res.cpu()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
