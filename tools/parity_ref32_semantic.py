"""parity_ref32.py for a step with the semantic loss (GPU box):  python tools/parity_ref32_semantic.py [size] [batch] [full_adaptation]
The HIP trainer's generator gradients AND the oracle's own fp32 evaluation (same weights, inputs, pinned generator and
segmentation-network kinks, the device's pseudo-labels) against the fp64 oracle, worst tensors first."""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from munit_amd import ops  # noqa: E402
from oracle import munit_oracle as O  # noqa: E402
from tests import semantic_oracle as S  # noqa: E402
from tests.parity import run_step_parity  # noqa: E402

size = int(sys.argv[1]) if len(sys.argv) > 1 else 256
batch = int(sys.argv[2]) if len(sys.argv) > 2 else 1
full = int(sys.argv[3]) if len(sys.argv) > 3 else 0
seg, sink = S.make_model(0), []
O.OracleTrainer = S.oracle_trainer_class(seg, lambda: sink)
with tempfile.TemporaryDirectory() as d, ops.kinks(seg=sink):
    ck = os.path.join(d, "seg.pth")
    torch.save(seg.state_dict(), ck)
    rep = run_step_parity(size=size, batch=batch, gen_state=1, iters=1, device="cuda:0", check=False, ref32=True,
                          hp_overrides={"semantic_w": 3, "semantic_ckpt_path": ck, "adaptation": {"full_adaptation": full}})
rows = rep["ref32"][0]
med = lambda k: sorted(r[k] for r in rows)[len(rows) // 2]
print("%d tensors; median L2  HIP %.2e   oracle-fp32 %.2e;  worst max  HIP %.2e   oracle-fp32 %.2e;  loss_rel %.2e" % (
    len(rows), med(2), med(4), max(r[1] for r in rows), max(r[3] for r in rows), rep["loss_rel"]))
for r in sorted(rows, key=lambda r: -max(r[1], r[3]))[:8]:
    print("   %-56s HIP max %.2e l2 %.2e | oracle-fp32 max %.2e l2 %.2e" % (r[0][:56], r[1], r[2], r[3], r[4]))
