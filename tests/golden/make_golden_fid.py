"""Golden numbers of the FID arithmetic from the reference's scripts/inception_utils.py (build container only, no GPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fid.py <reference checkout>

The reference module imports torchvision's inception_v3 at its top, and torchvision is not installed: its source is executed
here with a stub module under that name (none of the recorded functions touches it).  Nothing of the source is kept: the
fixture tests/golden/golden_fid.json holds data only --
  * one small case in fp64 (D = 12, N = 48, the pools of tests/fid_oracle.py): torch_cov of both pools,
    sqrt_newton_schulz(sigma1 sigma2, 400) as a digest (trace, sum, Frobenius norm, four entries),
    torch_calculate_frechet_distance and numpy_calculate_frechet_distance;
  * the public names of the module with their parameter lists, as inspect reads them."""
import inspect
import json
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
D, N = 12, 48


def load_reference(checkout):
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.inception = types.ModuleType("torchvision.models.inception")
    tv.models.inception.inception_v3 = None
    for name, mod in (("torchvision", tv), ("torchvision.models", tv.models), ("torchvision.models.inception", tv.models.inception)):
        sys.modules.setdefault(name, mod)
    ns = types.ModuleType("ref_inception_utils")
    with open(os.path.join(checkout, "scripts", "inception_utils.py")) as f:
        exec(compile(f.read(), "inception_utils.py", "exec"), ns.__dict__)
    return ns


def signatures(ns):
    out = {}
    for name, obj in sorted(vars(ns).items()):
        if getattr(obj, "__module__", None) != ns.__name__ or name.startswith("_"):
            continue
        if inspect.isclass(obj):
            out[name] = {"kind": "class", "methods": {m: list(inspect.signature(getattr(obj, m)).parameters)
                                                      for m in ("__init__", "forward")}}
        elif inspect.isfunction(obj):
            sig = inspect.signature(obj)
            out[name] = {"kind": "function", "params": list(sig.parameters),
                         "defaults": {k: repr(p.default) for k, p in sig.parameters.items() if p.default is not p.empty}}
    return out


def main():
    from tests import fid_oracle as FO
    R = load_reference(sys.argv[1])
    p1, p2 = (p.double() for p in FO.pools(D, n=N))
    mu1, mu2 = p1.mean(0), p2.mean(0)
    # torch_cov subtracts the mean through a view of its argument: hand it copies
    s1, s2 = R.torch_cov(p1.clone(), rowvar=False), R.torch_cov(p2.clone(), rowvar=False)
    root = R.sqrt_newton_schulz(s1.mm(s2).unsqueeze(0), 400)[0]
    fd_torch = R.torch_calculate_frechet_distance(mu1, s1, mu2, s2)
    fd_numpy = R.numpy_calculate_frechet_distance(mu1.numpy(), s1.numpy(), mu2.numpy(), s2.numpy())
    fixture = {
        "D": D, "N": N, "iters": 400,
        "mu1": mu1.tolist(), "mu2": mu2.tolist(), "sigma1": s1.tolist(), "sigma2": s2.tolist(),
        "sqrt_digest": {"trace": float(torch.trace(root)), "sum": float(root.sum()), "fro": float(root.norm()),
                        "entries": {"0,0": float(root[0, 0]), "0,11": float(root[0, 11]), "7,3": float(root[7, 3]),
                                    "11,5": float(root[11, 5])}},
        "frechet_torch": float(fd_torch), "frechet_numpy": float(fd_numpy),
        "signatures": signatures(R),
    }
    with open(os.path.join(HERE, "golden_fid.json"), "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
    print("wrote golden_fid.json: frechet torch %.15g numpy %.15g, names %s"
          % (fixture["frechet_torch"], fixture["frechet_numpy"], sorted(fixture["signatures"])))


if __name__ == "__main__":
    main()
