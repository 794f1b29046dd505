"""Golden numbers of the non-saturating GAN loss (dis.gan_type: nsgan) from the reference (build container only, no GPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nsgan.py <reference checkout>

`MsImageDis` is the reference's own, imported from <reference checkout>/scripts/networks.py; nothing of it is kept in this
repository.  Its nsgan branches move their targets with `.cuda()`: torch.Tensor.cuda is patched to the identity for the run.
The network is MsImageDis(3, dim 8, n_layer 2, num_scales 2, lrelu, reflect, nsgan) in float64 under a fixed seed, on two
input pairs of (2, 3, 16, 16): randn, and 40 * randn (the larger logits).

Output: tests/golden/golden_nsgan.json -- the weights, the inputs, calc_dis_loss / calc_gen_loss / calc_dis_loss_sr per pair,
digests of their input gradients, the largest |logit|, and the error calc_gen_loss_sr raises under nsgan."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.make_golden_semantic import digest  # noqa: E402

HP_DIS = dict(dim=8, norm="none", activ="lrelu", n_layer=2, gan_type="nsgan", num_scales=2, pad_type="reflect")
SEED, SCALES = 1234, (1.0, 40.0)


def main(ref):
    sys.path.insert(0, os.path.join(ref, "scripts"))
    import networks as R  # noqa: E402  (the reference's)
    plain_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        torch.manual_seed(SEED)
        net = R.MsImageDis(3, dict(HP_DIS)).double()
        out = {"hp_dis": HP_DIS, "seed": SEED,
               "weights": {k: {"shape": list(v.shape), "data": v.reshape(-1).tolist()} for k, v in net.state_dict().items()},
               "pairs": []}
        worst = 0.0
        for scale in SCALES:
            fake, real = (scale * torch.randn(2, 3, 16, 16, dtype=torch.float64) for _ in range(2))
            rec = {"scale": scale, "fake": fake.reshape(-1).tolist(), "real": real.reshape(-1).tolist()}
            with torch.no_grad():
                worst = max([worst] + [float(o.abs().max()) for x in (fake, real) for o in net(x)])
            x0, x1 = fake.clone().requires_grad_(True), real.clone().requires_grad_(True)
            loss = net.calc_dis_loss(x0, x1)
            g0, g1 = torch.autograd.grad(loss, [x0, x1])
            rec["loss_dis"], rec["d_fake_dis"], rec["d_real_dis"] = float(loss.detach()), digest(g0), digest(g1)
            loss = net.calc_gen_loss(x0)
            rec["loss_gen"], rec["d_fake_gen"] = float(loss.detach()), digest(torch.autograd.grad(loss, [x0])[0])
            loss = net.calc_dis_loss_sr(x0, x1)
            g0, g1 = torch.autograd.grad(loss, [x0, x1])
            rec["loss_dis_sr"], rec["d_sim_dis_sr"], rec["d_real_dis_sr"] = float(loss.detach()), digest(g0), digest(g1)
            out["pairs"].append(rec)
        out["max_abs_logit"] = worst
        try:
            net.calc_gen_loss_sr(fake)
            out["gen_loss_sr_raises"] = None
        except Exception as e:  # noqa: BLE001  (recorded, whatever it is)
            out["gen_loss_sr_raises"] = [type(e).__name__, str(e)]
    finally:
        torch.Tensor.cuda = plain_cuda
    with open(os.path.join(HERE, "golden_nsgan.json"), "w") as f:
        json.dump(out, f)
    print({"max_abs_logit": worst, "gen_loss_sr_raises": out["gen_loss_sr_raises"],
           "losses": [{k: v for k, v in p.items() if k.startswith("loss")} for p in out["pairs"]]})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
