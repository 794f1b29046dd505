"""Golden numbers of the output-level simulated / real losses from the reference (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_outda.py <reference checkout>

`MsImageDis` is the reference's own, imported from <reference checkout>/scripts/networks.py (as make_golden.py imports it);
nothing of it is kept in this repository.  It runs in float64 on tests/outda_oracle.make_state's seeded weights and seeded
(2, 3, 64, 64) images, with config_256.yaml's discriminator block.

Output: tests/golden/golden_outda.json -- calc_dis_loss_sr(sim, real), calc_gen_loss_sr(fake) and calc_dis_loss(sim, real)
(the same numbers as calc_dis_loss_sr: the first argument is held to 0, the second to 1), the per-scale output shapes, and
digests of d calc_gen_loss_sr / d image and of d calc_dis_loss_sr / d (first and last convolution weight)."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.make_golden_semantic import digest  # noqa: E402

BATCH, SIZE = 2, 64
TAG, SEED_SIM, SEED_REAL = "ocls_a.", 51, 52
FIRST, LAST = "cnns.0.0.conv.weight", "cnns.2.4.weight"


def main(ref):
    from oracle import munit_oracle as O
    from tests import outda_oracle as D
    sys.path.insert(0, os.path.join(ref, "scripts"))
    import networks as R  # noqa: E402  (the reference's)
    hp = O.default_hp(SIZE, BATCH, 1)
    net = R.MsImageDis(hp["input_dim_a"], hp["dis"]).double()
    sd = D.make_state(hp, TAG)
    assert list(net.state_dict()) == list(sd)
    net.load_state_dict(sd, strict=True)
    sim, real = D.images(BATCH, 3, SIZE, SEED_SIM), D.images(BATCH, 3, SIZE, SEED_REAL)
    out = {"batch": BATCH, "size": SIZE, "keys": [[k, list(v.shape)] for k, v in net.state_dict().items()]}
    with torch.no_grad():
        out["out_shapes"] = [list(o.shape) for o in net(sim)]
        out["loss_dis"] = float(net.calc_dis_loss(sim, real))
    fake = sim.clone().requires_grad_(True)
    l_gen = net.calc_gen_loss_sr(fake)
    out["loss_gen_sr"] = float(l_gen.detach())
    out["d_image_gen_sr"] = digest(torch.autograd.grad(l_gen, [fake])[0])
    params = dict(net.named_parameters())
    l_dis = net.calc_dis_loss_sr(sim, real)
    out["loss_dis_sr"] = float(l_dis.detach())
    g_first, g_last = torch.autograd.grad(l_dis, [params[FIRST], params[LAST]])
    out["d_first_dis_sr"], out["d_last_dis_sr"] = digest(g_first), digest(g_last)
    with open(os.path.join(HERE, "golden_outda.json"), "w") as f:
        json.dump(out, f)
    print({k: v for k, v in out.items() if k.startswith(("loss", "out_"))})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
