"""ms per dis_update + gen_update at 256^2 B=8 with semantic_w 0 and 3 in one process, and the per-kernel split of the
semantic path (HIP events around each seg Function and convolution pass of one extra instrumented step).

    python tools/time_semantic.py [--size 256] [--batch 8] [--steps 10] [--warmup 3]

The segmentation network gets deterministic calibrated weights (tests/semantic_oracle.make_model); its arithmetic cost
does not depend on the values."""
import argparse
import json
import os
import sys
import tempfile
import time
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from munit_amd import ops  # noqa: E402
from munit_amd.trainer import MUNIT_Trainer  # noqa: E402
from oracle import munit_oracle as O  # noqa: E402
from tests import semantic_oracle as S  # noqa: E402


def run(hp, xa, xb, ma, mb, steps, warmup):
    torch.manual_seed(0)
    tr = MUNIT_Trainer(hp).to("cuda:0")
    for _ in range(warmup):
        tr.dis_update(xa, xb, hp)
        tr.gen_update(xa, xb, hp, ma, mb)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.dis_update(xa, xb, hp)
        tr.gen_update(xa, xb, hp, ma, mb)
    torch.cuda.synchronize()
    return tr, (time.perf_counter() - t0) * 1e3 / steps


def seg_split(tr, xa, xb, ma, mb):
    """per-kernel-group time of the semantic term alone (label pass, logits pass, head, backward), HIP events"""
    prof, groups = [], defaultdict(float)
    ops.PROFILE = prof
    try:
        mask = torch.cat([ma, mb]).contiguous()
        x_ab, x_ba = xb.clone().requires_grad_(True), xa.clone().requires_grad_(True)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        loss = tr._semantic_loss(xa, xb, x_ab, x_ba, ma, mb)
        e[1].record()
        loss.backward()
        e[2].record()
        torch.cuda.synchronize()
        for which, pl, a, b in prof:
            groups["%s %s" % (("fwd", "dgrad", "wgrad")[which], pl.kname[which])] += a.elapsed_time(b)
        del mask
        return {"seg_forward_ms (labels + logits + loss)": e[0].elapsed_time(e[1]), "seg_backward_ms": e[1].elapsed_time(e[2]),
                "conv_ms_by_kernel": dict(sorted(groups.items(), key=lambda kv: -kv[1]))}
    finally:
        ops.PROFILE = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    xa = (torch.rand(a.batch, 3, a.size, a.size, generator=g) * 2 - 1).cuda().contiguous(memory_format=torch.channels_last)
    xb = (torch.rand(a.batch, 3, a.size, a.size, generator=g) * 2 - 1).cuda().contiguous(memory_format=torch.channels_last)
    ma = (torch.rand(a.batch, 1, a.size, a.size, generator=g) < 0.3).float().cuda()
    mb = (torch.rand(a.batch, 1, a.size, a.size, generator=g) < 0.3).float().cuda()
    out = {}
    hp0 = O.default_hp(a.size, a.batch, 1)
    _, out["ms_semantic_w_0"] = run(hp0, xa, xb, ma, mb, a.steps, a.warmup)
    with tempfile.TemporaryDirectory() as d:
        ck = os.path.join(d, "seg.pth")
        torch.save(S.make_model(0).state_dict(), ck)
        hp3 = O.default_hp(a.size, a.batch, 1)
        hp3["semantic_w"] = 3
        hp3["semantic_ckpt_path"] = ck
        tr, out["ms_semantic_w_3"] = run(hp3, xa, xb, ma, mb, a.steps, a.warmup)
    out["added_ms"] = out["ms_semantic_w_3"] - out["ms_semantic_w_0"]
    out["split"] = seg_split(tr, xa, xb, ma, mb)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
