"""Golden record of the reference's label mapping for the synthetic data loader (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_synth_data.py <reference checkout>

`mapping` is the reference's own: its definition is cut out of scripts/utils.py with `ast` at generation time and executed
(the module itself imports comet_ml, torchvision and more, and cannot be imported here); nothing of it is kept in this
repository.  It runs on what MyDatasetSynthetic.transform hands it for each of the 256 grey values of an `L` plane:
to_tensor(x) * 255 in fp32, that is (v / 255f) * 255f (utils.py:532-535).

Output: tests/golden/golden_synth_data.json -- "input": the 256 fp32 values (v / 255f) * 255f, "mapped": the 256 results."""
import ast
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def reference_mapping(ref):
    path = os.path.join(ref, "scripts", "utils.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "mapping"]
    assert len(fn) == 1
    ns = {"torch": torch}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["mapping"]


def main(ref):
    x = torch.arange(256, dtype=torch.uint8).float().div(255) * 255          # ToTensor, then * 255
    assert x.dtype == torch.float32
    out = {"input": x.tolist(), "mapped": reference_mapping(ref)(x.clone()).tolist()}
    with open(os.path.join(HERE, "golden_synth_data.json"), "w") as f:
        json.dump(out, f)
    print({k: out["mapped"][k] for k in (0, 29, 55, 76, 133, 149, 178, 200, 255, 1, 128)})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
