"""Time what the domain-invariant perceptual loss (vgg_w) costs on one device, on one build in one process: dis_update +
gen_update with vgg_w 1 against the same step with vgg_w 0, the two trainers taking turns round by round, on config_256.yaml's
networks at 256 x 256, batch 8, and at config_HD's 512 x 512, batch 4; and, alone at each of the two, the VGG16 forward over
2B images, its backward-data chain, and the two vgg.hip kernel pairs (ops.vgg_input, ops.in_mse).

  python tools/time_vgg.py [--rounds 5] [--inner 3] [--warmup 3] [--configs 256x8,512x4]

The weights are seeded He-normal ones written to a temporary vgg16.weight: timing does not depend on their values.  A round
times `inner` iterations of one trainer, host-synchronised at its end; the parts are timed between two device events.
Prints one JSON line: per configuration the median and min .. max over the rounds of the milliseconds per iteration with and
without the loss, their difference and ratio, and the parts in milliseconds."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(ts, digits=3):
    return dict(median=round(statistics.median(ts), digits), min=round(min(ts), digits), max=round(max(ts), digits))


def timed(fn, rounds, calls):
    """milliseconds per call of fn between two device events, per round"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / calls)
    return spread(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="256x8,512x4", help="comma-separated <crop>x<batch>")
    args = ap.parse_args()
    from munit_amd import ops
    from munit_amd.trainer import MUNIT_Trainer
    from munit_amd.vgg import Vgg16
    from oracle import munit_oracle as O
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = Vgg16()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 4:
                p.normal_(0.0, (2.0 / (p.shape[1] * 9)) ** 0.5)
            else:
                p.normal_(0.0, 0.1)
    out = {"rounds": args.rounds, "inner": args.inner, "configs": {}}
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, "models"))
        torch.save(net.state_dict(), os.path.join(root, "models", "vgg16.weight"))
        for cfg in args.configs.split(","):
            size, batch = (int(v) for v in cfg.split("x"))
            x_a, x_b, m_a, m_b = [t.to(dev) for t in O.synthetic_batch(batch, size)]
            trainers = {}
            for w in (1, 0):
                hp = O.default_hp(size, batch, 1)
                hp["vgg_w"], hp["vgg_model_path"] = w, root
                torch.manual_seed(0)
                trainers[w] = (MUNIT_Trainer(dict(hp)).to(dev), hp)

            def iteration(w):
                tr, hp = trainers[w]
                tr.dis_update(x_a, x_b, hp)
                tr.gen_update(x_a, x_b, hp, m_a, m_b)

            for w in trainers:
                for _ in range(args.warmup):
                    iteration(w)
            torch.cuda.synchronize()
            times = {w: [] for w in trainers}
            for _ in range(args.rounds):
                for w in trainers:
                    t0 = time.perf_counter()
                    for _ in range(args.inner):
                        iteration(w)
                    torch.cuda.synchronize()
                    times[w].append(1e3 * (time.perf_counter() - t0) / args.inner)
            on, off = statistics.median(times[1]), statistics.median(times[0])
            res = {"iteration_ms": {"vgg_w 1": spread(times[1]), "vgg_w 0": spread(times[0])},
                   "added_ms": round(on - off, 3), "ratio": round(on / off, 4)}
            # the parts, on 2B images as gen_update runs them
            vgg = trainers[1][0].vgg
            xs = (ops.nhwc(x_a), ops.nhwc(x_b))
            with torch.no_grad():
                res["vgg_forward_ms"] = timed(lambda: vgg(*xs), args.rounds, 3)
                res["vgg_input_fwd_ms"] = timed(lambda: ops.vgg_input(*xs), args.rounds, 20)
                target = vgg(*xs)
            xg = tuple(x.clone().requires_grad_(True) for x in xs)
            dz = torch.randn_like(target)

            def fwd_bwd():
                vgg(*xg).backward(dz)

            fb = timed(fwd_bwd, args.rounds, 3)
            res["vgg_forward_backward_ms"] = fb
            res["vgg_backward_data_ms"] = round(fb["median"] - res["vgg_forward_ms"]["median"], 3)
            feat = ops.nhwc(target.roll(1, 0)).detach().requires_grad_(True)

            def loss_fb():
                ops.in_mse(feat, target).backward()

            with torch.no_grad():
                res["in_mse_fwd_ms"] = timed(lambda: ops.in_mse(feat, target), args.rounds, 20)
            res["in_mse_fwd_bwd_ms"] = timed(loss_fb, args.rounds, 20)
            res["feature_shape"] = list(target.shape)
            out["configs"][cfg] = res
            del trainers, vgg, target, feat, xg
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
