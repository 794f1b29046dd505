"""Golden digests of the domain-invariant perceptual loss from the reference's own code (build container only, no GPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vgg.py <reference checkout>

scripts/networks.py is imported for Vgg16.  scripts/utils.py and scripts/trainer.py import torchvision, which is not installed,
so only the two definitions used are taken from them: the source of utils.vgg_preprocess and of
MUNIT_Trainer.compute_vgg_loss is cut out of the files (ast) and executed here with the names they need supplied (torch,
Variable; a stand-in `self` holding nn.InstanceNorm2d(512, affine=False), trainer.py:89).  vgg_preprocess builds its mean with
`tensortype(size).cuda()`: torch.Tensor.cuda is patched to the identity and the default dtype set to float64 for the run, so the
means are float64 like everything else.  Nothing of the source is kept: the fixture holds data only.

Weights: tests/vgg_oracle.make_model(0) (He-normal, small random biases) under the reference's keys.  32x48, B = 2, float64.

Output: tests/golden/golden_vgg.json -- sum, sum of |.|, sum of squares and 64 seeded samples of the preprocessed image, of
relu5_3 of both inputs and of the gradient to the translated image, and the loss."""
import ast
import json
import os
import sys
import types

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

H, W, BATCH, NSAMPLE = 32, 48, 2, 64


def digest(t):
    t = t.detach().double().reshape(-1)
    g = torch.Generator().manual_seed(t.numel())
    idx = torch.randint(0, t.numel(), (NSAMPLE,), generator=g)
    return {"numel": t.numel(), "sum": float(t.sum()), "abs": float(t.abs().sum()), "sq": float((t * t).sum()),
            "idx": idx.tolist(), "val": t[idx].tolist()}


def inputs():
    from tests import vgg_oracle as V
    return V.rand_images(BATCH, H, W, 31), V.rand_images(BATCH, H, W, 32)      # translated image, original image


def cut(path, name):
    """The source of the function or method `name` in the file at `path`, dedented."""
    import textwrap
    src = open(path).read()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.FunctionDef) and node.name == name:
            return textwrap.dedent(ast.get_source_segment(src, node, padded=True))
    raise KeyError(name)


def main(ref):
    scripts = os.path.join(ref, "scripts")
    sys.path.insert(0, scripts)
    import networks as R  # noqa: E402  (the reference's)
    from torch.autograd import Variable
    from tests import vgg_oracle as V
    ns = {"torch": torch, "Variable": Variable}
    exec(compile(cut(os.path.join(scripts, "utils.py"), "vgg_preprocess"), "utils.py", "exec"), ns)
    exec(compile(cut(os.path.join(scripts, "trainer.py"), "compute_vgg_loss"), "trainer.py", "exec"), ns)
    sd = V.make_model(0).state_dict()                   # fp32 parameters, as a weight file holds them
    plain_cuda, plain_dtype = torch.Tensor.cuda, torch.get_default_dtype()
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.set_default_dtype(torch.float64)
    try:
        vgg = R.Vgg16()
        vgg.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
        vgg = vgg.double().eval()
        trainer = types.SimpleNamespace(instancenorm=nn.InstanceNorm2d(512, affine=False))
        x_trans, x_orig = inputs()
        out = {"h": H, "w": W, "batch": BATCH, "keys": list(vgg.state_dict().keys()),
               "shapes": [list(v.shape) for v in vgg.state_dict().values()],
               "weights_sq": float(sum((v.double() ** 2).sum() for v in sd.values()))}
        with torch.no_grad():
            out["preprocessed"] = digest(ns["vgg_preprocess"](x_trans))
            out["relu5_3_trans"] = digest(vgg(ns["vgg_preprocess"](x_trans)))
            out["relu5_3_orig"] = digest(vgg(ns["vgg_preprocess"](x_orig)))
        xt = x_trans.clone().requires_grad_(True)
        loss = ns["compute_vgg_loss"](trainer, vgg, xt, x_orig)
        loss.backward()
        out["loss"] = float(loss.detach())
        out["dx"] = digest(xt.grad)
    finally:
        torch.Tensor.cuda = plain_cuda
        torch.set_default_dtype(plain_dtype)
    with open(os.path.join(HERE, "golden_vgg.json"), "w") as f:
        json.dump(out, f)
    print({"loss": out["loss"], "relu5_3 max sample": max(abs(v) for v in out["relu5_3_trans"]["val"])})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
