"""Time the Inception-v3 feature trunk of FID evaluation (csrc/inception.hip, munit_amd/inception.py) on the device.

  python tools/time_inception.py [--batches 1,8,32] [--rounds 9] [--inner 20] [--warmup 3] [--out FILE]

Per layer: every distinct convolution shape of the trunk at each batch size -- munit_conv2d_rect_fwd's median time between two
device events, its TFLOP/s (2 M N K over the time) and share of the 157.3 TFLOP/s fp32 matrix peak, the tile the host chose;
for every 1x1 layer munit_gemm_f32 at the same M, N, K (the convolution adds only the bias / ReLU epilogue and the strided
store to it); and torch's own convolution + bias + ReLU on the same device and operands (channels_last, warmed up first so
that its algorithm choice is made), all three timed in alternating rounds of one process.
Whole trunk: WrapInception.forward (input kernel, trunk, final mean) in images/s, next to the fp32 forward of
tests/inception_oracle.py run on the device through torch.
Prints a table and, last, one JSON line (also written to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PEAK_TFLOPS = 157.3


def distinct_layers():
    """[(key, names)]: key = (H, W, Cin, Cout, KH, KW, stride, pad_h, pad_w) in plan order, names = the rows that have it."""
    from munit_amd import inception as I
    steps, _, _ = I.build_plan()
    seen = {}
    for s in steps:
        if s.kind == "conv":
            seen.setdefault((s.src.h, s.src.w) + I._ROW[s.arg][1:], []).append(s.arg)
    return list(seen.items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ctypes import c_float, c_void_p
    from munit_amd import _lib, inception_utils as IU, ops
    lib = _lib.load()
    from tests import inception_oracle as IO
    assert torch.cuda.is_available(), "time_inception.py measures on the device: there is no other path"
    dev = torch.device("cuda:0")
    batches = [int(b) for b in args.batches.split(",")]
    stream = c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def timed(fns, inner):
        """{name: median ms per call}: warm-up of every fn, then `rounds` alternating rounds of `inner` calls each."""
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(inner):
                    fn()
                t1.record()
                t1.synchronize()
                times[k].append(t0.elapsed_time(t1) / inner)
        return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}

    g = torch.Generator().manual_seed(1)
    layers, rows = distinct_layers(), []
    print("%-3s %-34s %7s %6s %6s %8s %8s %7s %6s %8s %6s %8s %6s" % ("B", "layer (first of n)", "M", "N", "K", "tile", "hip ms",
                                                                     "TFLOP/s", "peak", "gemm ms", "ratio", "torch ms", "ratio"))
    for b in batches:
        for (h, w, cin, cout, kh, kw, s, ph, pw), names in layers:
            x = torch.randn(b, h, w, cin, generator=g).to(dev)
            wt = (torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5).to(dev)
            bias = torch.randn(cout, generator=g).to(dev)
            img = ops.rect_weight_image(wt)
            out = ops.conv2d_rect(x, img, bias, kh, kw, s, ph, pw)
            m, n, k = out.shape[0] * out.shape[1] * out.shape[2], cout, kh * kw * cin
            x_t = x.permute(0, 3, 1, 2)                                  # the same memory as a channels_last NCHW tensor
            wt_t = wt.contiguous(memory_format=torch.channels_last)
            # the two library calls with everything prepared (one C call each), so that small layers time the kernel and not
            # the wrapper; torch's call carries its own dispatch cost
            fns = {"hip": ops.conv2d_rect_launch(x, img, bias, kh, kw, s, ph, pw, out=out)[0],
                   "torch": lambda: F.relu(F.conv2d(x_t, wt_t, bias, stride=s, padding=(ph, pw)))}
            if kh == kw == 1:
                c2 = torch.empty(m, n, device=dev)
                prob = (_lib.GemmProblem * 1)(_lib.GemmProblem(x.data_ptr(), img.data_ptr(), c2.data_ptr()))
                fns["gemm"] = lambda: lib.munit_gemm_f32(prob, 1, m, n, k, k, n, n, 0, c_float(1.0), c_float(0.0), stream)
            t = timed(fns, args.inner)
            tf = 2.0 * m * n * k / (t["hip"][0] * 1e-3) / 1e12
            row = dict(B=b, layer=names[0], count=len(names), H=h, W=w, M=m, N=n, K=k, filter=[kh, kw, s, ph, pw],
                       tile=ops.conv2d_rect_tile(b, h, w, cin, cout, kh, kw, s, ph, pw), hip_ms=round(t["hip"][0], 4),
                       hip_min_ms=round(t["hip"][1], 4), hip_max_ms=round(t["hip"][2], 4), tflops=round(tf, 2),
                       share_of_peak=round(tf / PEAK_TFLOPS, 4), torch_ms=round(t["torch"][0], 4),
                       vs_torch=round(t["hip"][0] / t["torch"][0], 3))
            if "gemm" in t:
                row.update(gemm_ms=round(t["gemm"][0], 4), vs_gemm=round(t["hip"][0] / t["gemm"][0], 3))
            rows.append(row)
            print("%-3d %-34s %7d %6d %6d %8s %8.4f %7.2f %6.3f %8s %6s %8.4f %6.2f"
                  % (b, "%s (%d)" % (names[0], len(names)), m, n, k, row["tile"], row["hip_ms"], tf, tf / PEAK_TFLOPS,
                     "%.4f" % row["gemm_ms"] if "gemm_ms" in row else "-", "%.2f" % row["vs_gemm"] if "vs_gemm" in row else "-",
                     row["torch_ms"], row["vs_torch"]))
            sys.stdout.flush()

    # whole trunk: the HIP forward against the oracle's fp32 forward through torch on the device
    state = IO.random_state(0)
    wrap = IU.WrapInception(state)
    dstate = {k: v.to(dev) for k, v in state.items()}
    trunk = []
    for b in batches:
        x = (torch.rand(b, 3, 299, 299, generator=g) * 2 - 1).to(dev)
        t = timed({"hip": lambda: wrap(x), "torch": lambda: IO.features(dstate, x, torch.float32)}, max(1, args.inner // 4))
        err = float((wrap(x) - IO.features(dstate, x, torch.float32)).abs().max())
        rec = dict(B=b, hip_ms=round(t["hip"][0], 3), hip_min_ms=round(t["hip"][1], 3), hip_max_ms=round(t["hip"][2], 3),
                   hip_images_per_s=round(b / (t["hip"][0] * 1e-3), 1), torch_ms=round(t["torch"][0], 3),
                   torch_images_per_s=round(b / (t["torch"][0] * 1e-3), 1), vs_torch=round(t["hip"][0] / t["torch"][0], 3),
                   max_abs_difference=err)
        trunk.append(rec)
        print("trunk B=%d: hip %.3f ms (%.1f images/s)  torch %.3f ms (%.1f images/s)  hip / torch %.2f  max |hip - torch| %.3e"
              % (b, rec["hip_ms"], rec["hip_images_per_s"], rec["torch_ms"], rec["torch_images_per_s"], rec["vs_torch"], err))
    out = json.dumps({"device": torch.cuda.get_device_name(0), "peak_tflops": PEAK_TFLOPS, "rounds": args.rounds,
                      "inner": args.inner, "layers": rows, "trunk": trunk})
    if args.out:
        with open(args.out, "w") as f:
            f.write(out + "\n")
    print(out)


if __name__ == "__main__":
    main()
