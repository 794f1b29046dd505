"""Golden digests of the simulated / real feature classifier from the reference (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_featda.py <reference checkout>

`conv3x3`, `conv1x1`, `BasicBlock` and `domainClassifier` are the reference's own: their definitions are cut out of
scripts/utils.py with `ast` at generation time and executed in a namespace that holds `torch` and `nn` (the module itself
imports comet_ml, torchvision models and more, and cannot be imported here); nothing of them is kept in this repository.
The networks run in float64, in training mode, on tests/featda_oracle.make_state's seeded weights and a seeded
(2, 256, 64, 64) code.  The losses are written out from compute_classifier_sr_loss (scripts/trainer.py:638-667).

Output: tests/golden/golden_featda.json -- the state_dict keys and shapes, digests of the two classifiers' outputs, the
three losses (fool, real, synthetic), the digest of the fooling loss's gradient with respect to the code of classifier a,
and the digests of every running statistic of classifier a after one and after two forward passes."""
import ast
import json
import os
import sys

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.make_golden_semantic import digest  # noqa: E402

BATCH, CODE = 2, 64
SEED_A, SEED_B, SEED_CA, SEED_CB = 41, 42, 43, 44


def reference_classes(ref):
    path = os.path.join(ref, "scripts", "utils.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    want = ("conv3x3", "conv1x1", "BasicBlock", "domainClassifier")
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in want]
    assert sorted(n.name for n in body) == sorted(want)

    class NN(object):
        """torch.nn with one adapter: domainClassifier builds its blocks with stride=True, which the torch the reference was
        written for read as 1 and the current nn.Conv2d refuses as a bool"""
        def __getattr__(self, name):
            return getattr(nn, name)

        @staticmethod
        def Conv2d(*args, **kw):
            if "stride" in kw:
                kw["stride"] = int(kw["stride"])
            return nn.Conv2d(*args, **kw)

    ns = {"torch": torch, "nn": NN()}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns["domainClassifier"]


def running(net):
    return {k: digest(v) for k, v in net.state_dict().items() if k.endswith(("running_mean", "running_var"))}


def main(ref):
    from tests import featda_oracle as D
    cls = reference_classes(ref)
    nets = []
    for seed in (SEED_A, SEED_B):
        net = cls(256).double().train()
        net.load_state_dict(D.make_state(seed), strict=True)
        nets.append(net)
    net_a, net_b = nets
    out = {"batch": BATCH, "code": CODE,
           "keys": [[k, list(v.shape)] for k, v in net_a.state_dict().items()]}
    c_a, c_b = D.code(BATCH, CODE, CODE, SEED_CA), D.code(BATCH, CODE, CODE, SEED_CB)
    ca = c_a.clone().requires_grad_(True)
    o_a, o_b = net_a(ca), net_b(c_b)                                     # forward 1
    out["out_a"], out["out_b"] = o_a.detach().reshape(-1).tolist(), o_b.detach().reshape(-1).tolist()
    out["out_shape"] = list(o_a.shape)
    out["running_1"] = running(net_a)
    out["tracked_1"] = int(net_a.state_dict()["BasicBlock1.bn1.num_batches_tracked"])
    for name, t in (("fool", 0.5), ("synth", 0.0), ("real", 1.0)):      # trainer.py:657-665
        out["loss_" + name] = float((torch.mean((o_a - t) ** 2) + torch.mean((o_b - t) ** 2)).detach())
    (torch.mean((o_a - 0.5) ** 2) + torch.mean((o_b - 0.5) ** 2)).backward()
    out["d_code_fool"] = digest(ca.grad)
    with torch.no_grad():
        net_a(c_b)                                                       # forward 2, another batch
    out["running_2"] = running(net_a)
    out["tracked_2"] = int(net_a.state_dict()["BasicBlock1.bn1.num_batches_tracked"])
    with torch.no_grad():
        o1 = net_a(c_a[:1])                                              # B = 1: .squeeze() drops the batch axis
    out["out_b1_shape"] = list(o1.shape)
    out["out_b1"] = o1.reshape(-1).tolist()
    with open(os.path.join(HERE, "golden_featda.json"), "w") as f:
        json.dump(out, f)
    print({k: v for k, v in out.items() if k.startswith(("loss", "out_"))})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
