"""Time what spectral normalisation of the discriminators (dis.norm: sn) costs on one device, on one build in one process:
dis_update + gen_update of config_256.yaml's networks with dis.norm sn against the same step with dis.norm none, the two
trainers taking turns round by round, and the power-iteration call (ops.sn_power_iter) alone on the production table -- the
nine normalised layers of one discriminator: (128, 64), (256, 128), (512, 256) x 4 x 4 at each of three scales.

  python tools/time_sn.py [--batch 8] [--size 256] [--rounds 9] [--inner 5] [--warmup 5]

A round times `inner` iterations of one trainer, host-synchronised at its end; the power iteration is timed between two device
events over 200 calls per round.  Prints one JSON line: median and min .. max over the rounds of the milliseconds per
iteration for both norms and their ratio, and of the microseconds per power-iteration call."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(ts, digits=3):
    return dict(median=round(statistics.median(ts), digits), min=round(min(ts), digits), max=round(max(ts), digits))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from munit_amd import ops
    from munit_amd.trainer import MUNIT_Trainer
    from oracle import munit_oracle as O
    dev = torch.device("cuda:0")
    x_a, x_b, m_a, m_b = [t.to(dev) for t in O.synthetic_batch(args.batch, args.size)]
    trainers = {}
    for norm in ("sn", "none"):
        hp = O.default_hp(args.size, args.batch, 1)
        hp["dis"] = dict(hp["dis"], norm=norm)
        torch.manual_seed(0)
        trainers[norm] = (MUNIT_Trainer(dict(hp)).to(dev), hp)

    def iteration(norm):
        tr, hp = trainers[norm]
        tr.dis_update(x_a, x_b, hp)
        tr.gen_update(x_a, x_b, hp, m_a, m_b)

    for norm in trainers:
        for _ in range(args.warmup):
            iteration(norm)
    torch.cuda.synchronize()
    times = {norm: [] for norm in trainers}
    for _ in range(args.rounds):
        for norm in trainers:
            t0 = time.perf_counter()
            for _ in range(args.inner):
                iteration(norm)
            torch.cuda.synchronize()
            times[norm].append(1e3 * (time.perf_counter() - t0) / args.inner)
    out = {"batch": args.batch, "size": args.size, "rounds": args.rounds, "inner": args.inner,
           "iteration_ms": {norm: spread(ts) for norm, ts in times.items()},
           "ratio_sn_over_none": round(statistics.median(times["sn"]) / statistics.median(times["none"]), 4)}
    # the power iteration alone, on the table of one production discriminator
    dis = trainers["sn"][0].dis_a
    table = ops.sn_table([m.layer() for m in dis._sn])
    calls = 200
    for _ in range(20):
        ops.sn_power_iter(*table)
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            ops.sn_power_iter(*table)
        e1.record()
        e1.synchronize()
        ts.append(1e3 * e0.elapsed_time(e1) / calls)
    out["power_iter_us"] = dict(spread(ts, 2), layers=table[1], max_O=table[2], max_N=table[3],
                                weight_mbytes=round(sum(4 * m.layer()[0].numel() for m in dis._sn) / 2 ** 20, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
