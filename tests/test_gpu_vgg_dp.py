"""GPU: the perceptual loss (vgg_w: 1) under data-parallel training -- two ranks (two fresh processes sharing cuda:0, gloo
backend, tests/test_gpu_dp.py's launcher) run dis_update + gen_update on different half-batches.  The VGG16 is frozen and
every term is a mean over samples normalised per sample, so the all-reduced flat gradient must be the gradient of the joined
batch: checked against the fp64 oracle on the joined batch with every kink pinned, the network's included."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

SIZE, B = 64, 2


def _hp(vgg_dir, batch):
    import bench
    hp = bench.bench_hp(SIZE, batch)
    hp["vgg_w"] = 1
    hp["vgg_model_path"] = vgg_dir
    return hp


def _worker(rank, world, tmpdir, vgg_dir):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    import bench
    from munit_amd import ops
    from munit_amd import trainer as T
    from tests.test_gpu_dp import _step
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(tmpdir, "rdzv"), rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    hp = _hp(vgg_dir, B)
    batch = tuple(t.to(dev) for t in bench.make_batch(B, SIZE, rank))
    torch.manual_seed(1234)
    tr = T.MUNIT_Trainer(dict(hp))
    tr.to(dev)
    assert tr.vgg is not None and T.OVERLAP_EXCHANGE
    with ops.kinks(vgg=True) as k:
        g_dis, g_gen, dis_p, kinks = _step(tr, hp, batch, record=True)
    stages = tr.last_exchange.stages
    assert len(stages) == 2 and all(st["fired"] for st in stages), stages
    torch.save({"g_gen": g_gen, "g_dis": g_dis, "dis_p": dis_p, "kinks": kinks, "vgg": [t.cpu() for t in k.vgg],
                "gen_p": tr.gen_opt.flat_p.detach().cpu().clone(),
                "losses": [float(tr.loss_gen_vgg_a.detach()), float(tr.loss_gen_vgg_b.detach())]},
               os.path.join(tmpdir, "vgg_rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_step_with_vgg_loss_matches_the_oracle_on_the_joined_batch(tmp_path):
    """Two gloo ranks on one GPU, half-batches of 2, vgg_w: 1, the staged gradient exchange (both stages must fire: the
    network's backward adds a contributor to the tensors they are armed on).  Both ranks end with bitwise the same averaged
    gradients and weights.  The averaged generator gradient against the fp64 oracle on the joined batch of 4 (with the
    discriminator weights the ranks stepped to): each rank records the branches of its own samples -- generator,
    discriminators, L1 signs and the VGG16's ReLUs and pool winners -- and the oracle takes them joined along the batch axis,
    so both sides differentiate the same piecewise-linear function.  Bounds: tests/test_gpu_vgg.py's step rule -- every
    tensor <= 5e-5 normalised max and relative L2, or 2 x the error of the oracle itself evaluated in fp32 on the same
    state and pins where that is larger (measured on this batch: worst 4.0e-4 max / 3.3e-4 L2 where the fp32 oracle has
    1.2e-3 / 1.0e-3; medians 5.5e-5 and 1.7e-4).  The two
    perceptual losses of the joined batch are the means of the ranks' (1e-5 relative)."""
    import torch.multiprocessing as mp
    import bench
    from munit_amd.trainer import MUNIT_Trainer
    from oracle import munit_oracle as O
    from tests import parity
    from tests import vgg_oracle as V
    from tests.parity import KINK_FRAC, KINK_NOISE, oracle_states, trainer_named_params
    model = V.make_model(0)
    vgg_dir = str(tmp_path / "run")
    os.makedirs(os.path.join(vgg_dir, "models"))
    torch.save(model.state_dict(), os.path.join(vgg_dir, "models", "vgg16.weight"))
    mp.spawn(_worker, args=(2, str(tmp_path), vgg_dir), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / ("vgg_rank%d.pt" % k), weights_only=True) for k in range(2))
    for key in ("g_gen", "g_dis", "dis_p", "gen_p"):
        assert torch.equal(r0[key], r1[key]), key
    assert len(r0["vgg"]) == len(r1["vgg"]) == 2 * V.N_KINKS

    def joined(a, b):
        """a rank's pass runs [x_b, x_a] (then [x_ba, x_ab]) of ITS samples; the joined batch runs both ranks' x_b, then x_a"""
        return torch.cat([a[:B], b[:B], a[B:], b[B:]], 0)

    sink = [joined(a, b) for a, b in zip(r0["vgg"], r1["vgg"])]
    dev = torch.device("cuda:0")
    hp = _hp(vgg_dir, 2 * B)
    torch.manual_seed(1234)
    tr = MUNIT_Trainer(dict(hp))             # the ranks' initial weights (same seed); hosts the per-tensor views of the flat buffers
    tr.to(dev)
    gnames, dnames = trainer_named_params(tr)
    cls = V.oracle_trainer_class(model, lambda: sink)
    orc = cls(dict(hp), *oracle_states(hp, torch.float64))
    o_gen, o_dis = orc.opt["gen"]["params"], orc.opt["dis"]["params"]
    with torch.no_grad():
        tr.dis_opt.flat_p.copy_(r0["dis_p"].to(dev))        # gen_update on the discriminators the ranks stepped to
        for (n, p), q in list(zip(gnames, o_gen)) + list(zip(dnames, o_dis)):
            q.copy_(p.detach().double().cpu())
    parts = [bench.make_batch(B, SIZE, r) for r in range(2)]
    joint = [torch.cat([parts[0][i], parts[1][i]], 0).double() for i in range(4)]
    (m0, s0), (m1, s1) = r0["kinks"][1], r1["kinks"][1]
    km = O.KinkMasks([torch.cat([a, b], 0) for a, b in zip(m0, m1)], [torch.cat([a, b], 0) for a, b in zip(s0, s1)])
    orc.update_learning_rate()
    # the yardstick first (it must see the weights before the fp64 oracle steps them): the oracle in fp32, same pins
    f32 = lambda st: {k: v.detach().float().clone() for k, v in st.items()}
    orc32 = cls(dict(hp), f32(orc.gen), f32(orc.dis_a), f32(orc.dis_b))
    with parity.pinned(O.KinkMasks(list(km.masks), list(km.l1_signs)), "gen_update in fp32", check=False):
        g32 = orc32.gen_update(*(t.float() for t in joint), apply=False)
    with parity.pinned(km, "gen_update"):
        g_ref = orc.gen_update(joint[0], joint[1], joint[2], joint[3])
    worst, frac = cls.audit_worst
    assert worst <= KINK_NOISE and frac <= KINK_FRAC, cls.audit_worst
    for i, name in enumerate(("loss_gen_vgg_a", "loss_gen_vgg_b")):
        want, got = float(orc.losses[name]), (r0["losses"][i] + r1["losses"][i]) / 2
        assert want > 0 and abs(got - want) <= 1e-5 * want, (name, got, want)
    tr.gen_opt.flat_g.copy_(r0["g_gen"].to(dev))
    rows = []
    for (n, p), g, h in zip(gnames, g_ref, g32):
        if g is None or float(g.abs().max()) < 1e-7:         # conv bias ahead of an instance norm: mathematically zero
            continue
        rows.append((n, parity.nerr(p._munit_grad, g), parity.l2err(p._munit_grad, g), parity.nerr(h, g), parity.l2err(h, g)))
    assert len(rows) >= 80
    med = lambda k: sorted(r[k] for r in rows)[len(rows) // 2]
    print("two ranks with vgg_w 1 vs fp64 oracle on the joined batch: worst max %.2e, worst L2 %.2e, median L2 %.2e; the oracle "
          "in fp32: %.2e, %.2e, %.2e" % (max(r[1] for r in rows), max(r[2] for r in rows), med(2), max(r[3] for r in rows),
                                         max(r[4] for r in rows), med(4)))
    for name, hip_max, hip_l2, r32_max, r32_l2 in rows:
        assert hip_max <= max(5e-5, 2 * r32_max) and hip_l2 <= max(5e-5, 2 * r32_l2), (name, hip_max, hip_l2, r32_max, r32_l2)
    assert med(2) <= max(1e-5, 2 * med(4)), (med(2), med(4))
