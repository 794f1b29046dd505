"""Golden features of the FID feature network from the reference's scripts/inception_utils.py (build container only, no GPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_inception.py <reference checkout>

The reference's WrapInception.forward is executed as it stands (its source with a stub module under torchvision's name, as
tests/golden/make_golden_fid.py does), in fp64, around a `net` object whose sixteen attributes are the stem convolutions and
Mixed blocks of tests/inception_oracle.py with the weights random_state(0).  What the fixture pins to the reference is
therefore everything forward itself does: the normalisation constants, the resize, the two max pools, the order of the
blocks and the final mean.  Nothing of the source is kept: tests/golden/golden_inception.json holds data only -- for the two
batches of inception_oracle.fixture_inputs() every 8th feature of every image and the sum of each feature row."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
EVERY = 8


def main():
    from make_golden_fid import load_reference
    from tests import inception_oracle as IO
    R = load_reference(sys.argv[1])
    wrap = R.WrapInception(IO.blocks(IO.random_state(0), torch.float64)).double()
    fixture = {"seed": 0, "every": EVERY, "cases": {}}
    for name, x in IO.fixture_inputs().items():
        with torch.no_grad():
            pool = wrap(x)
        assert tuple(pool.shape) == (x.shape[0], 2048) and pool.dtype == torch.float64
        fixture["cases"][name] = {"shape": list(x.shape), "features": pool[:, ::EVERY].tolist(), "row_sums": pool.sum(1).tolist(),
                                  "nonzero": float((pool != 0).double().mean())}
        print("%s %s: max %.6g nonzero %.3f" % (name, tuple(x.shape), float(pool.max()), fixture["cases"][name]["nonzero"]))
    with open(os.path.join(HERE, "golden_inception.json"), "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
