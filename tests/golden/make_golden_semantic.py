"""Golden digests of the semantic-consistency loss from the reference's own scripts/resnet.py (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_semantic.py <reference checkout>

Only scripts/resnet.py is imported, and the network is built with pretrained=False: resnet34(fully_conv=True,
output_stride=8, remove_avg_pool_layer=True) with `fc` swapped for a 1x1 Conv2d(512, 19) (scripts/utils.py:936-956; the
reference's Resnet34_8s itself would download ImageNet weights).  Weights: tests/semantic_oracle.make_model(0) (He-normal
convs, random BN affines, BN statistics calibrated on seeded images), loaded under the reference's module names.  The
loss is written out from compute_semantic_seg_loss (scripts/trainer.py:706-771) with F.interpolate(bilinear,
align_corners=False) for the network's up-sample.  Everything in float64 at 64x64, B=2.

Output: tests/golden/golden_semantic.json -- for the logits, both cross-entropy branches and the input gradients of each
branch: the value (losses) or sum, sum of |.|, sum of squares and 64 seeded samples (tensors)."""
import json
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

SIZE, BATCH, NSAMPLE = 64, 2, 64


def digest(t):
    t = t.detach().double().reshape(-1)
    g = torch.Generator().manual_seed(t.numel())
    idx = torch.randint(0, t.numel(), (NSAMPLE,), generator=g)
    return {"numel": t.numel(), "sum": float(t.sum()), "abs": float(t.abs().sum()), "sq": float((t * t).sum()),
            "idx": idx.tolist(), "val": t[idx].tolist()}


def inputs():
    from tests import semantic_oracle as S
    x_orig = S.rand_images(BATCH, SIZE, 21)
    x_trans = S.rand_images(BATCH, SIZE, 22)
    g = torch.Generator().manual_seed(23)
    mask = torch.zeros(BATCH, 1, SIZE, SIZE, dtype=torch.float64)
    mask[:, :, SIZE // 4:SIZE // 2, :] = 1.0                         # a band of 1s, zeros elsewhere ...
    mask[:, :, SIZE // 2:] = (torch.rand(BATCH, 1, SIZE // 2, SIZE, generator=g) < 0.3).double()   # ... and speckle
    return x_orig, x_trans, mask


def main(ref):
    sys.path.insert(0, os.path.join(ref, "scripts"))
    import resnet                                                   # the reference's scripts/resnet.py, nothing else
    from tests import semantic_oracle as S
    torch.manual_seed(0)
    net = resnet.resnet34(pretrained=False, fully_conv=True, output_stride=8, remove_avg_pool_layer=True)
    net.fc = nn.Conv2d(net.inplanes, 19, 1)
    sd = {k[len("resnet34_8s."):]: v for k, v in S.make_model(0).state_dict().items()}
    net.load_state_dict(sd, strict=True)
    net = net.double().eval()

    def seg(x):                                                      # Resnet34_8s.forward, utils.py:961-971
        return F.interpolate(net(x), size=x.shape[2:], mode="bilinear", align_corners=False)

    def transform(img):                                              # trainer.py:720-725, utils.py:159-174
        m = torch.tensor((0.485, 0.456, 0.406), dtype=torch.float64).view(1, 3, 1, 1)
        s = torch.tensor((0.229, 0.224, 0.225), dtype=torch.float64).view(1, 3, 1, 1)
        return ((img + 1) / 2.0 - m) / s

    x_orig, x_trans, mask = inputs()
    out = {"size": SIZE, "batch": BATCH, "weights_sq": float(sum((v.double() ** 2).sum() for v in sd.values()
                                                                     if v.is_floating_point()))}
    with torch.no_grad():
        target = seg(transform(x_orig)).max(1)[1]
        z = net(transform(x_trans))
    out["logits_low"] = digest(z)
    out["labels"] = digest(target.double())
    for branch in ("masked", "plain"):
        xt = x_trans.clone().requires_grad_(True)
        output = seg(transform(xt))
        if branch == "masked":                                       # trainer.py:746-767, mask already at crop size
            m_long = mask.long().squeeze(1)
            tgt = torch.mul(1 - m_long, target) + m_long * 19
            loss = nn.CrossEntropyLoss()(torch.cat((torch.mul(1 - mask, output), mask), dim=1), tgt)
        else:                                                        # trainer.py:769-770
            loss = nn.CrossEntropyLoss()(output, target)
        loss.backward()
        out["loss_" + branch] = float(loss.detach())
        out["dx_" + branch] = digest(xt.grad)
    with open(os.path.join(HERE, "golden_semantic.json"), "w") as f:
        json.dump(out, f)
    print({k: v for k, v in out.items() if k.startswith("loss")})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
