"""Time the feature-level domain adaptation (adaptation.adv_lambda / dfeat_lambda) on one device: gen_update of the config_256
geometry with the fooling term against the same build with both weights at 0, and domain_classifier_sr_update on its own.

  python tools/time_featda.py [--batch 8] [--size 256] [--steps 20] [--warmup 5] [--only on|off]

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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=("off", "on"), default=None, help="time one of the two trainers (for a kernel trace)")
    args = ap.parse_args()
    from munit_amd.trainer import MUNIT_Trainer
    from oracle import munit_oracle as O
    dev = torch.device("cuda:0")
    x_a, x_b, m_a, m_b = [t.to(dev) for t in O.synthetic_batch(args.batch, args.size)]
    out = {"batch": args.batch, "size": args.size, "steps": args.steps}
    for name, ad in (("gen_update_off", {}), ("gen_update_on", dict(adv_lambda=6, dfeat_lambda=1))):
        if args.only and name != "gen_update_" + args.only:
            continue
        hp = O.default_hp(args.size, args.batch, 1)
        hp["adaptation"].update(ad)
        torch.manual_seed(0)
        tr = MUNIT_Trainer(hp).to(dev)
        out[name + "_ms"] = timed(lambda: tr.gen_update(x_a, x_b, hp, m_a, m_b), args.steps, args.warmup)
        if ad:
            out["classifier_update_ms"] = timed(
                lambda: tr.domain_classifier_sr_update(x_a, x_b, False, hp["adaptation"]["dfeat_lambda"], 0), args.steps, args.warmup)
        del tr
    print(json.dumps(out))


if __name__ == "__main__":
    main()
