"""Time the segmentation head's update (adaptation.sem_seg_lambda) on one device: segmentation_head_update of the config_256
geometry at each batch size, and its 512-channel 3x3 convolution on the phase images in its three passes.

  python tools/time_seghead.py [--batches 2,8] [--size 256] [--steps 20] [--warmup 5] [--ckpt seg.pth]

Without --ckpt the head starts from a seeded Resnet34_8s (tests/semantic_oracle.make_model) saved to a temporary file: the
time does not depend on the values.  Prints one JSON line: median and spread (min .. max) of the per-call wall time in ms,
host-synchronised around each call."""
import argparse
import json
import os
import statistics
import sys
import tempfile
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


def conv_passes(images, hw, steps, warmup):
    """forward, backward-data and backward-weight of the head's 512 -> 512 3x3 layer on `images` phase images of hw x hw"""
    from munit_amd import ops
    dev = torch.device("cuda:0")
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)
    x, w = cl(torch.randn(images, 512, hw, hw)), cl(torch.randn(512, 512, 3, 3) * 0.02)
    dy = cl(torch.randn(images, 512, hw, hw))
    return {"fwd_ms": timed(lambda: ops.conv2d_fwd_raw(x, w, None, 1, 1, "zero", False, "none"), steps, warmup),
            "dgrad_ms": timed(lambda: ops.conv2d_dgrad_raw(dy, w, x.shape, 1, 1, "zero", False), steps, warmup),
            "wgrad_ms": timed(lambda: ops.conv2d_wgrad_raw(x, dy, w.shape, 1, 1, "zero", False, want_bias=False), steps, warmup)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2,8")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ckpt", default=None, help="a Resnet34_8s checkpoint (default: a seeded one)")
    args = ap.parse_args()
    from munit_amd.trainer import MUNIT_Trainer
    from oracle import munit_oracle as O
    dev = torch.device("cuda:0")
    ckpt = args.ckpt
    tmp = None
    if ckpt is None:
        from tests import semantic_oracle as S
        tmp = tempfile.TemporaryDirectory()
        ckpt = os.path.join(tmp.name, "seg.pth")
        torch.save(S.make_model(0).state_dict(), ckpt)
    out = {"size": args.size, "steps": args.steps}
    for b in [int(v) for v in args.batches.split(",")]:
        x_a, x_b, _, _ = [t.to(dev) for t in O.synthetic_batch(b, args.size)]
        g = torch.Generator().manual_seed(b)
        t_a, t_b = [torch.randint(0, 10, (b, 1, args.size, args.size), generator=g).float().to(dev) for _ in range(2)]
        hp = O.default_hp(args.size, b, 1)
        hp["adaptation"]["sem_seg_lambda"] = 1
        hp["semantic_ckpt_path"] = ckpt
        torch.manual_seed(0)
        tr = MUNIT_Trainer(hp).to(dev)
        out["segmentation_head_update_b%d_ms" % b] = timed(lambda: tr.segmentation_head_update(x_a, x_b, t_a, t_b, 1.0),
                                                           args.steps, args.warmup)
        n = args.size >> hp["gen"]["n_downsample"]
        out["conv512_3x3_%dx%dx%d" % (16 * b, n // 4, n // 4)] = conv_passes(16 * b, n // 4, args.steps, args.warmup)
        del tr
    print(json.dumps(out))
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
