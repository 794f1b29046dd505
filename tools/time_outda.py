"""Time the output-level domain adaptation (adaptation.output_classifier_lambda / output_adv_lambda) on one device, at the
production configs' own geometry: output_domain_classifier_sr_update, gen_update with the term against the same trainer
handed output_adv_lambda 0, and the multi-scale LSGAN loss of one batched [sim; real] discriminator pass on its own -- one
ops.lsgan_loss against the same six terms composed from ops.mse_const on batch slices + ops.scalar_sum (forward + backward).

  python tools/time_outda.py [--batch 2] [--size 256] [--steps 20] [--warmup 5]

Prints one JSON line: median and spread (min .. max) of the per-call wall time in ms, host-synchronised around each call."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return dict(median=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from munit_amd import ops
    from munit_amd.trainer import MUNIT_Trainer
    from oracle import munit_oracle as O
    dev = torch.device("cuda:0")
    b = args.batch
    x_a, x_b, m_a, m_b = [t.to(dev) for t in O.synthetic_batch(b, args.size)]
    x_as, x_bs = [t.to(dev) for t in O.synthetic_batch(b, args.size, seed=8)[:2]]
    hp = O.default_hp(args.size, b, 1)
    hp["adaptation"].update(output_classifier_lambda=1, output_adv_lambda=1)
    off = dict(hp, adaptation=dict(hp["adaptation"], output_adv_lambda=0))
    torch.manual_seed(0)
    tr = MUNIT_Trainer(hp).to(dev)
    out = {"batch": b, "size": args.size, "steps": args.steps}
    out["classifier_update_ms"] = timed(lambda: tr.output_domain_classifier_sr_update(x_a, x_as, x_b, x_bs, hp, 0),
                                        args.steps, args.warmup)
    out["gen_update_off_ms"] = timed(lambda: tr.gen_update(x_a, x_b, off, m_a, m_b), args.steps, args.warmup)
    out["gen_update_on_ms"] = timed(lambda: tr.gen_update(x_a, x_b, hp, m_a, m_b), args.steps, args.warmup)
    # the loss alone, on tensors of the three scales' output shapes of one batched pass (2 B images)
    n_down = hp["dis"]["n_layer"]
    maps = [(args.size >> s) >> n_down for s in range(hp["dis"]["num_scales"])]
    outs = [torch.randn(2 * b, 1, m, m, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            for m in maps]
    one = torch.ones((), device=dev)

    def fused():
        torch.autograd.grad(ops.lsgan_loss(outs, [(0.0, 1.0)] * len(outs)), outs, one)

    def composed():
        terms = []
        for o in outs:
            terms += [ops.mse_const(o[:b], 0.0), ops.mse_const(o[b:], 1.0)]
        torch.autograd.grad(ops.scalar_sum(terms), outs, one)

    out["maps"] = maps
    out["loss_lsgan_ms"] = timed(fused, args.steps, args.warmup)
    out["loss_composed_ms"] = timed(composed, args.steps, args.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
