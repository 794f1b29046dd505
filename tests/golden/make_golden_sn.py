"""Golden numbers of spectral normalisation in the discriminators (dis.norm: sn) from the reference (build container only, no
GPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sn.py <reference checkout>

`MsImageDis` (with `Conv2dBlock` and `SpectralNorm`) is the reference's own, imported from <reference checkout>/scripts/
networks.py; `weights_init` is cut out of scripts/utils.py with `ast` at generation time and executed in a namespace that holds
`torch.nn.init` and `math` (the module itself cannot be imported here).  Nothing of either is kept in this repository.
torch.Tensor.cuda is patched to the identity for the run.

Network A: MsImageDis(3, dim 8, n_layer 3, num_scales 2, lrelu, reflect, lsgan, norm sn), built in fp32 under a fixed seed
(the construction draws are what is pinned), then evaluated in float64.  Recorded:
  * the state-dict keys in order, named_parameters() in order with requires_grad, the initial state;
  * the state of a copy after weights_init("gaussian") under a second seed, and whether the wrapped convolutions own a `weight`;
  * on two input pairs (2, 3, 32, 32), in this order on ONE network (every forward advances weight_u / weight_v):
    calc_dis_loss(fake, real), calc_gen_loss(fake), calc_dis_loss_sr(sim, real2), calc_gen_loss_sr(sim) -- each with its loss,
    the gradients of the inputs in full, weight_u / weight_v afterwards and, for the two discriminator losses, the gradient of
    every trainable parameter in full.  The inputs are float32 values (randn drawn in float32).
Network B: the same with dim 6 (O = 12 / 24, 96 / 192 columns: nothing a multiple of 64), one calc_gen_loss with all gradients.

Output: tests/golden/golden_sn.json (structure and scalars) and the arrays it names -- float32 where the reference held
float32, float64 otherwise -- in tests/golden/golden_sn.npz (network A) and tests/golden/golden_sn_b.npz (network B): two
files to stay below the size limit of a committed file."""
import ast
import copy
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

HP_A = dict(dim=8, norm="sn", activ="lrelu", n_layer=3, gan_type="lsgan", num_scales=2, pad_type="reflect")
HP_B = dict(HP_A, dim=6)
SEED_A, SEED_INIT, SEED_X, SEED_B = 4321, 4322, 4323, 4324


def reference_weights_init(ref):
    path = os.path.join(ref, "scripts", "utils.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "weights_init"]
    assert len(fn) == 1
    ns = {"init": torch.nn.init, "math": math}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["weights_init"]


class Arrays(object):
    def __init__(self):
        self.data = {}

    def put(self, name, t):
        assert name not in self.data, name
        a = t.detach().cpu().contiguous().numpy().copy()
        if name.startswith(("a.x.", "b.x")):
            assert (a.astype(np.float32) == a).all()
            a = a.astype(np.float32)
        self.data[name] = a
        return name

    def state(self, prefix, net):
        return {k: self.put(prefix + k, v) for k, v in net.state_dict().items()}


def uv(net):
    return {k: v for k, v in net.state_dict().items() if k.endswith(("weight_u", "weight_v"))}


def call(arr, tag, net, fn, inputs, param_grads=True):
    xs = [x.clone().requires_grad_(True) for x in inputs]
    names = [n for n, p in net.named_parameters() if p.requires_grad and param_grads]
    params = [p for _, p in net.named_parameters() if p.requires_grad and param_grads]
    loss = fn(*xs)
    grads = torch.autograd.grad(loss, params + xs)
    rec = {"loss": float(loss.detach()),
           "param_grads": {n: arr.put("%s.grad.%s" % (tag, n), g) for n, g in zip(names, grads)},
           "input_grads": [arr.put("%s.dx%d" % (tag, i), g) for i, g in enumerate(grads[len(params):])],
           "uv_after": {k: arr.put("%s.after.%s" % (tag, k), v) for k, v in uv(net).items()}}
    return rec


def main(ref):
    sys.path.insert(0, os.path.join(ref, "scripts"))
    import networks as R  # noqa: E402  (the reference's)
    weights_init = reference_weights_init(ref)
    plain_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    arr = Arrays()
    try:
        torch.manual_seed(SEED_A)
        net = R.MsImageDis(3, dict(HP_A))
        out = {"hp_a": HP_A, "hp_b": HP_B, "seeds": dict(a=SEED_A, init=SEED_INIT, x=SEED_X, b=SEED_B),
               "state_keys": list(net.state_dict()),
               "named_parameters": [[n, bool(p.requires_grad)] for n, p in net.named_parameters()],
               "n_parameters": len(list(net.parameters())),
               "n_trainable": len([p for p in net.parameters() if p.requires_grad]),
               "initial": arr.state("a.initial.", net)}
        inited = copy.deepcopy(net)
        out["inner_conv_owns_weight_before_forward"] = [
            bool(hasattr(m.module, "weight")) for m in inited.modules() if isinstance(m, R.SpectralNorm)]
        torch.manual_seed(SEED_INIT)
        inited.apply(weights_init("gaussian"))
        out["after_weights_init_gaussian"] = arr.state("a.inited.", inited)

        net = net.double()
        torch.manual_seed(SEED_X)
        fake, real, sim, real2 = (torch.randn(2, 3, 32, 32).double() for _ in range(4))      # fp32 values
        out["inputs"] = {k: arr.put("a.x." + k, v) for k, v in dict(fake=fake, real=real, sim=sim, real2=real2).items()}
        out["calls"] = [
            dict(call(arr, "a.dis", net, net.calc_dis_loss, [fake, real]), fn="calc_dis_loss", inputs=["fake", "real"]),
            dict(call(arr, "a.gen", net, net.calc_gen_loss, [fake], False), fn="calc_gen_loss", inputs=["fake"]),
            dict(call(arr, "a.dis_sr", net, net.calc_dis_loss_sr, [sim, real2]), fn="calc_dis_loss_sr", inputs=["sim", "real2"]),
            dict(call(arr, "a.gen_sr", net, net.calc_gen_loss_sr, [sim], False), fn="calc_gen_loss_sr", inputs=["sim"]),
        ]

        torch.manual_seed(SEED_B)
        net_b = R.MsImageDis(3, dict(HP_B))
        out["b"] = {"initial": arr.state("b.initial.", net_b)}
        net_b = net_b.double()
        x_b = torch.randn(2, 3, 32, 32).double()
        out["b"]["x"] = arr.put("b.x", x_b)
        out["b"]["call"] = dict(call(arr, "b.gen", net_b, net_b.calc_gen_loss, [x_b]), fn="calc_gen_loss")
    finally:
        torch.Tensor.cuda = plain_cuda
    with open(os.path.join(HERE, "golden_sn.json"), "w") as f:
        json.dump(out, f, indent=0)
    np.savez_compressed(os.path.join(HERE, "golden_sn.npz"), **{k: v for k, v in arr.data.items() if k.startswith("a.")})
    np.savez_compressed(os.path.join(HERE, "golden_sn_b.npz"), **{k: v for k, v in arr.data.items() if k.startswith("b.")})
    print({"keys": len(out["state_keys"]), "parameters": out["n_parameters"], "trainable": out["n_trainable"],
           "inner_conv_owns_weight_before_forward": out["inner_conv_owns_weight_before_forward"],
           "losses": [c["loss"] for c in out["calls"]] + [out["b"]["call"]["loss"]], "arrays": len(arr.data)})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
