"""Golden digests of the synthetic-pair generator step's two terms from the reference (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_synth.py <reference checkout>

`merge_classes` is the reference's own: its definition is cut out of scripts/utils.py with `ast` at generation time and
executed in a namespace that holds `torch` (the module itself imports comet_ml, torchvision models and more, and cannot be
imported here); nothing of it is kept in this repository.  The default dtype is float64 while it runs (and only then), so
that the torch.zeros it allocates does not round the logits to fp32.  The network is scripts/resnet.py's, built and loaded as
tests/golden/make_golden_semantic.py does, with tests/semantic_oracle.make_model(0)'s weights.  The loss is written out
from compute_semantic_seg_loss with a ground truth (scripts/trainer.py:732-767, new_class = 10), the pair loss from
trainer.py:452-464 with recon_criterion_mask (trainer.py:305).  Everything in float64 at 64x64, B=2.

Output: tests/golden/golden_synth.json -- the merged-logit digest, the ground-truth loss plain and masked with the digest
of its input gradient, the pair loss with the digests of its gradients w.r.t. x_ab and x_ba, the aligned share."""
import ast
import json
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.make_golden_semantic import BATCH, SIZE, digest  # noqa: E402


def inputs():
    """(x_trans, gt, mask, pair): the translated images, the ground-truth maps (B, 1, H, W) float64 as the loader
    delivers them, the mask and the (x_a, x_b, x_ab, x_ba) of the pair loss."""
    from tests import semantic_oracle as S
    from tests import synth_oracle as Y
    x_trans = S.rand_images(BATCH, SIZE, 31)
    gt = Y.gt_maps(BATCH, SIZE, 32).unsqueeze(1)
    g = torch.Generator().manual_seed(33)
    mask = torch.zeros(BATCH, 1, SIZE, SIZE, dtype=torch.float64)
    mask[:, :, SIZE // 4:SIZE // 2, :] = 1.0
    mask[:, :, SIZE // 2:] = (torch.rand(BATCH, 1, SIZE // 2, SIZE, generator=g) < 0.3).double()
    return x_trans, gt, mask, Y.pair_inputs(BATCH, SIZE, 34)


def reference_merge_classes(ref):
    path = os.path.join(ref, "scripts", "utils.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "merge_classes"]
    assert len(fn) == 1
    ns = {"torch": torch}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["merge_classes"]


def main(ref):
    sys.path.insert(0, os.path.join(ref, "scripts"))
    import resnet
    from tests import semantic_oracle as S
    ref_merge = reference_merge_classes(ref)

    def merge_classes(output):          # float64 only while the reference's function allocates its result
        torch.set_default_dtype(torch.float64)
        try:
            return ref_merge(output)
        finally:
            torch.set_default_dtype(torch.float32)

    torch.manual_seed(0)
    net = resnet.resnet34(pretrained=False, fully_conv=True, output_stride=8, remove_avg_pool_layer=True)
    net.fc = nn.Conv2d(net.inplanes, 19, 1)
    sd = {k[len("resnet34_8s."):]: v for k, v in S.make_model(0).state_dict().items()}
    net.load_state_dict(sd, strict=True)
    net = net.double().eval()

    def seg(x):
        return F.interpolate(net(x), size=x.shape[2:], mode="bilinear", align_corners=False)

    def transform(img):
        m = torch.tensor((0.485, 0.456, 0.406), dtype=torch.float64).view(1, 3, 1, 1)
        s = torch.tensor((0.229, 0.224, 0.225), dtype=torch.float64).view(1, 3, 1, 1)
        return ((img + 1) / 2.0 - m) / s

    x_trans, gt, mask, (x_a, x_b, x_ab, x_ba) = inputs()
    assert sorted(gt.unique().tolist()) == list(range(10))
    out = {"size": SIZE, "batch": BATCH, "weights_sq": float(sum((v.double() ** 2).sum() for v in sd.values()
                                                                     if v.is_floating_point()))}
    with torch.no_grad():
        out["merged"] = digest(merge_classes(seg(transform(x_trans))))
    for branch in ("masked", "plain"):
        xt = x_trans.clone().requires_grad_(True)
        output = seg(transform(xt))
        target = gt.type(torch.long).squeeze(1)                          # trainer.py:734-737
        output = merge_classes(output)
        new_class = 10
        if branch == "masked":                                           # trainer.py:744-767, mask already at crop size
            m_long = mask.long().squeeze(1)
            tgt = torch.mul(1 - m_long, target) + m_long * new_class
            loss = nn.CrossEntropyLoss()(torch.cat((torch.mul(1 - mask, output), mask), dim=1), tgt)
        else:
            loss = nn.CrossEntropyLoss()(output, target)
        loss.backward()
        out["loss_" + branch] = float(loss.detach())
        out["dx_" + branch] = digest(xt.grad)

    def recon_criterion_mask(input, target, m):                          # trainer.py:305
        return torch.mean(torch.abs(torch.mul((input - target), 1 - m)))

    ab, ba = x_ab.clone().requires_grad_(True), x_ba.clone().requires_grad_(True)
    mask_alignment = (torch.sum(torch.abs(x_a - x_b), 1) == 0).unsqueeze(1)   # trainer.py:455-456
    mask_alignment = mask_alignment.type(torch.DoubleTensor)
    loss = recon_criterion_mask(ab, x_b, 1 - mask_alignment) + recon_criterion_mask(ba, x_a, 1 - mask_alignment)
    loss.backward()
    out["aligned_share"] = float(mask_alignment.mean())
    out["loss_pair"] = float(loss.detach())
    out["d_ab"] = digest(ab.grad)
    out["d_ba"] = digest(ba.grad)
    with open(os.path.join(HERE, "golden_synth.json"), "w") as f:
        json.dump(out, f)
    print({k: v for k, v in out.items() if k.startswith("loss") or k == "aligned_share"})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
