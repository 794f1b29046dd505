"""Golden digests of the trainable segmentation head from the reference's own scripts/resnet.py (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_seghead.py <reference checkout>

Only scripts/resnet.py is imported, and the network is built with pretrained=False: resnet34(fully_conv=True,
output_stride=8, remove_avg_pool_layer=True) with `fc` swapped for a 1x1 Conv2d(512, 19), as Resnet34_8s builds it
(scripts/utils.py:936-956).  Weights: tests/semantic_oracle.make_model(0), loaded under the reference's module names.  The
head is then put together the way scripts/trainer.py:207-210 does -- Sequential(*children()[7:-1], Conv2d(512, 10, 1)), i.e.
layer4, avgpool and the new last layer -- in training mode with every parameter trainable, the last layer holding
tests/seghead_oracle.make_state's seeded draw.  The loss is written out from segmentation_head_update
(scripts/trainer.py:1303-1318): two forwards, a then b, each up-sampled bilinearly to (size, size), two CrossEntropyLoss
terms, times lamb.  Everything in float64 on 16x16 codes, B = 2, crop 64.

Output: tests/golden/golden_seghead.json -- the state_dict keys and shapes, and for both outputs, every weight gradient
and the running statistics after the call: sum, sum of |.|, sum of squares and 64 seeded samples; the loss as a value."""
import json
import os
import sys

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

CODE, BATCH, SIZE, LAMB, NSAMPLE = 16, 2, 64, 0.5, 64
SEED_CA, SEED_CB, SEED_TA, SEED_TB = 61, 62, 63, 64


def digest(t):
    t = t.detach().double().reshape(-1)
    g = torch.Generator().manual_seed(t.numel())
    idx = torch.randint(0, t.numel(), (NSAMPLE,), generator=g)
    return {"numel": t.numel(), "sum": float(t.sum()), "abs": float(t.abs().sum()), "sq": float((t * t).sum()),
            "idx": idx.tolist(), "val": t[idx].tolist()}


def inputs():
    from tests import seghead_oracle as H
    return (H.code(BATCH, CODE, CODE, SEED_CA), H.code(BATCH, CODE, CODE, SEED_CB),
            H.labels(BATCH, SIZE, SEED_TA), H.labels(BATCH, SIZE, SEED_TB))


def main(ref):
    sys.path.insert(0, os.path.join(ref, "scripts"))
    import resnet                                                   # the reference's scripts/resnet.py, nothing else
    from tests import semantic_oracle as S
    from tests import seghead_oracle as H
    torch.manual_seed(0)
    net = resnet.resnet34(pretrained=False, fully_conv=True, output_stride=8, remove_avg_pool_layer=True)
    net.fc = nn.Conv2d(net.inplanes, 19, 1)
    net.load_state_dict({k[len("resnet34_8s."):]: v for k, v in S.make_model(0).state_dict().items()}, strict=True)
    last_layer = nn.Conv2d(512, 10, kernel_size=1)                   # trainer.py:207
    model = torch.nn.Sequential(*list(net.children())[7:-1], last_layer)      # trainer.py:208-210
    for param in model.parameters():                                 # trainer.py:213-214
        param.requires_grad = True
    model = model.double().train()                                   # the trainer is in training mode during the update
    sd = H.make_state(0)
    with torch.no_grad():
        last_layer.weight.copy_(sd["2.weight"])
        last_layer.bias.copy_(sd["2.bias"])
    out = {"code": CODE, "batch": BATCH, "size": SIZE, "lamb": LAMB,
           "keys": [[k, list(v.shape)] for k, v in model.state_dict().items()],
           "modules": [type(m).__name__ for m in model],
           "weights_sq": float(sum((v.double() ** 2).sum() for v in model.state_dict().values() if v.is_floating_point()))}
    for k, v in model.state_dict().items():                          # the oracle's state is this head's
        assert torch.equal(v.double() if v.is_floating_point() else v, sd[k]), k

    c_a, c_b, target_a, target_b = inputs()
    output_a = model(c_a)                                            # trainer.py:1303-1304
    output_b = model(c_b)
    out["output_a"], out["output_b"] = digest(output_a), digest(output_b)
    output_a = nn.functional.interpolate(input=output_a, size=(SIZE, SIZE), mode="bilinear")
    output_b = nn.functional.interpolate(input=output_b, size=(SIZE, SIZE), mode="bilinear")
    loss1 = nn.CrossEntropyLoss()(output_a, target_a.type(torch.long).squeeze(1))
    loss2 = nn.CrossEntropyLoss()(output_b, target_b.type(torch.long).squeeze(1))
    loss = (loss1 + loss2) * LAMB
    loss.backward()
    out["loss"] = float(loss.detach())
    out["grads"] = {k: digest(p.grad) for k, p in model.named_parameters()}
    out["running"] = {k: digest(v) for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var"))}
    out["tracked"] = int(model.state_dict()["0.0.bn1.num_batches_tracked"])
    with open(os.path.join(HERE, "golden_seghead.json"), "w") as f:
        json.dump(out, f)
    print({"loss": out["loss"], "tracked": out["tracked"], "modules": out["modules"]})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
