"""Host-side checks of output-level domain adaptation (adaptation.output_classifier_lambda / output_adv_lambda): the fp64
oracle against the reference's fixture, the trainer's construction, refusals and checkpoints, the C ABI of the multi-scale
LSGAN loss."""
import ctypes
import json
import os
import re
from ctypes import c_float, c_size_t, c_void_p

import pytest
import torch

from oracle import munit_oracle as O
from tests import outda_oracle as D
from tests.golden.make_golden_outda import BATCH, FIRST, LAST, SEED_REAL, SEED_SIM, SIZE, TAG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("munit_lsgan_workspace_bytes", "munit_lsgan_fwd", "munit_lsgan_bwd")
KEYS = "output_adv_lambda.*output_classifier_lambda"


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "golden_outda.json")) as f:
        return json.load(f)


def _check_digest(got, ref, rel=1e-9):
    t = got.detach().double().reshape(-1)
    assert t.numel() == ref["numel"]
    for key, val, bound in (("sum", float(t.sum()), ref["abs"]), ("abs", float(t.abs().sum()), ref["abs"]),
                            ("sq", float((t * t).sum()), ref["sq"])):
        assert abs(val - ref[key]) <= rel * bound, key
    assert (t[torch.tensor(ref["idx"])] - torch.tensor(ref["val"], dtype=torch.float64)).abs().max().item() \
        <= rel * t.abs().max().item()


def _hp(size=64, **adaptation):
    hp = O.default_hp(size, 2, 1)
    hp["gen"]["n_res"] = 1
    hp["adaptation"].update(adaptation)
    return hp


ON = dict(output_classifier_lambda=1, output_adv_lambda=1)


def test_oracle_reproduces_the_reference_fixture(fixture):
    """tests/outda_oracle.py against the reference's own MsImageDis in fp64: the two losses, calc_dis_loss (the same target
    order: first argument -> 0, second -> 1), the output shapes and three gradients."""
    fx = fixture
    assert (fx["batch"], fx["size"]) == (BATCH, SIZE)
    hp = O.default_hp(SIZE, BATCH, 1)
    sd = D.make_state(hp, TAG)
    assert [[k, list(v.shape)] for k, v in sd.items()] == fx["keys"]
    sim, real = D.images(BATCH, 3, SIZE, SEED_SIM), D.images(BATCH, 3, SIZE, SEED_REAL)
    with torch.no_grad():
        assert [list(o.shape) for o in O.dis_forward(sd, "", sim, hp["dis"])] == fx["out_shapes"] \
            == [[2, 1, 4, 4], [2, 1, 2, 2], [2, 1, 1, 1]]
        l_plain = float(O.dis_loss_d(sd, "", sim, real, hp["dis"]))
        l_swapped = float(D.dis_loss_sr(sd, real, sim, hp["dis"]))
    assert abs(l_plain - fx["loss_dis"]) <= 1e-9 * abs(fx["loss_dis"])
    assert fx["loss_dis"] == fx["loss_dis_sr"] and abs(l_swapped - fx["loss_dis_sr"]) > 1e-3      # the order matters
    fake = sim.clone().requires_grad_(True)
    l_gen = D.gen_loss_sr(sd, fake, hp["dis"])
    assert abs(float(l_gen.detach()) - fx["loss_gen_sr"]) <= 1e-9 * abs(fx["loss_gen_sr"])
    _check_digest(torch.autograd.grad(l_gen, [fake])[0], fx["d_image_gen_sr"])
    for p in sd.values():
        p.requires_grad_(True)
    l_dis = D.dis_loss_sr(sd, sim, real, hp["dis"])
    assert abs(float(l_dis.detach()) - fx["loss_dis_sr"]) <= 1e-9 * abs(fx["loss_dis_sr"])
    g_first, g_last = torch.autograd.grad(l_dis, [sd[FIRST], sd[LAST]])
    _check_digest(g_first, fx["d_first_dis_sr"])
    _check_digest(g_last, fx["d_last_dis_sr"])


def test_trainer_builds_the_classifiers_under_their_own_optimizer(tmp_path):
    from munit_amd.networks import MsImageDis
    from munit_amd.trainer import MUNIT_Trainer
    hp = _hp(**ON)
    hp["input_dim_a"], hp["input_dim_b"], hp["gen_state"] = 3, 1, 0          # both classifiers take input_dim_a
    torch.manual_seed(0)
    tr = MUNIT_Trainer(hp)
    assert tr.use_output_classifier_sr
    nets = (tr.output_classifier_sr_a, tr.output_classifier_sr_b)
    for net in nets:
        assert isinstance(net, MsImageDis) and net.input_dim == hp["input_dim_a"] == 3
        assert list(net.state_dict()) == list(tr.dis_a.state_dict())
        w = net.cnns[0][1].conv.weight
        assert abs(float(w.std()) - 0.02) < 2e-3 and float(net.cnns[0][0].conv.bias.abs().max()) == 0      # "gaussian"
    assert tr.dis_b.input_dim == 1
    opt = tr.output_classif_opt_sr
    assert [id(p) for p in opt._plist] == [id(p) for m in nets for p in m.parameters()]
    assert type(opt).__name__ == "FusedAdam" and opt.flat_p is not None
    mine = {id(p) for p in opt._plist}
    for other in (tr.gen_opt, tr.dis_opt):
        assert not mine & {id(p) for p in other._plist}
    for p in tr.output_classifier_sr_a.parameters():
        assert p._munit_opt is opt and p._munit_grad is not None
    # the scheduler exists and update_learning_rate leaves it at its initial step (trainer.py:1326-1335)
    assert tr.output_scheduler_sr.last_epoch == 0
    before = tr.dis_scheduler.last_epoch
    tr.update_learning_rate()
    assert tr.output_scheduler_sr.last_epoch == 0 and tr.dis_scheduler.last_epoch == before + 1
    for name in ("output_classif_opt_sr_step", "output_domain_classifier_sr_update"):
        assert callable(getattr(MUNIT_Trainer, name))
    off = MUNIT_Trainer(_hp())
    assert not off.use_output_classifier_sr
    assert not hasattr(off, "output_classif_opt_sr") and not hasattr(off, "output_classifier_sr_a")
    # save writes exactly the files it wrote before, with nothing of the classifiers in them
    names = []
    for sub, t in (("off", off), ("on", tr)):
        d = tmp_path / sub
        d.mkdir()
        t.save(str(d), 2)
        names.append(sorted(os.listdir(str(d))))
    assert names[0] == names[1] == ["dis_00000003.pt", "gen_00000003.pt", "optimizer.pt"]
    assert sorted(torch.load(str(tmp_path / "on" / "optimizer.pt"), weights_only=True)) == ["dis", "gen"]
    assert sorted(torch.load(str(tmp_path / "on" / "dis_00000003.pt"), weights_only=True)) == ["a", "b"]


def test_refusals_name_the_keys_and_touch_nothing(monkeypatch):
    from munit_amd import trainer as T
    for prec in ("bf16", "bf16s"):
        hp = _hp(**ON)
        hp["precision"] = prec
        with pytest.raises(NotImplementedError, match=KEYS):
            T.MUNIT_Trainer(hp)
    hp = _hp(**ON)
    hp["optimizer"] = "extraadam"
    with pytest.raises(NotImplementedError, match=KEYS + ".*extrapolation"):
        T.MUNIT_Trainer(hp)
    monkeypatch.setattr(T, "dp_size", lambda: 2)
    with pytest.raises(NotImplementedError, match=KEYS + ".*data-parallel"):
        T.MUNIT_Trainer(_hp(**ON))
    monkeypatch.undo()
    # a trainer built without the classifiers refuses the term and the update before it touches a gradient buffer
    tr = T.MUNIT_Trainer(_hp())
    tr.gen_opt.flat_g.fill_(3.0)
    tr.dis_opt.flat_g.fill_(3.0)
    x = torch.zeros(2, 3, 64, 64)
    with pytest.raises(ValueError, match="output_adv_lambda"):
        tr.gen_update(x, x, _hp(**ON))
    with pytest.raises(ValueError, match="output_classifier_lambda"):
        tr.output_domain_classifier_sr_update(x, x, x, x, _hp(**ON), 0)
    assert bool((tr.gen_opt.flat_g == 3.0).all()) and bool((tr.dis_opt.flat_g == 3.0).all())
    # ... and one built with them refuses a world that grew, likewise
    tr = T.MUNIT_Trainer(_hp(**ON))
    tr.gen_opt.flat_g.fill_(3.0)
    tr.output_classif_opt_sr.flat_g.fill_(3.0)
    monkeypatch.setattr(T, "dp_size", lambda: 2)
    with pytest.raises(NotImplementedError, match=KEYS):
        tr.gen_update(x, x, _hp(**ON))
    with pytest.raises(NotImplementedError, match=KEYS):
        tr.output_domain_classifier_sr_update(x, x, x, x, _hp(**ON), 0)
    assert bool((tr.gen_opt.flat_g == 3.0).all()) and bool((tr.output_classif_opt_sr.flat_g == 3.0).all())


def test_new_symbols_are_declared_listed_and_exported():
    from munit_amd import _lib
    header = open(os.path.join(ROOT, "include", "munit_hip.h")).read()
    declared = set(re.findall(r"\b(munit_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    nws = lib.munit_lsgan_workspace_bytes(3)
    assert nws > 0 and lib.munit_lsgan_workspace_bytes(8) > 0
    assert lib.munit_lsgan_workspace_bytes(0) == 0 and lib.munit_lsgan_workspace_bytes(9) == 0

    # host-side argument checks run before any launch (no device needed): the "device" pointers are never followed
    def arrays(n, length=16):
        return (c_void_p * n)(*[64] * n), (c_size_t * n)(*[length] * n), (c_float * n)(*[0.5] * n)

    px, pn, pt = arrays(3)
    fwd, bwd = lib.munit_lsgan_fwd, lib.munit_lsgan_bwd
    assert fwd(None, pn, pt, 3, 64, None, 64, nws, None) == -1 and b"lsgan_fwd" in lib.munit_last_error()
    assert fwd(px, None, pt, 3, 64, None, 64, nws, None) == -1
    assert fwd(px, pn, None, 3, 64, None, 64, nws, None) == -1
    assert fwd(px, pn, pt, 3, None, None, 64, nws, None) == -1
    assert fwd(px, pn, pt, 3, 64, None, None, nws, None) == -1
    assert fwd(px, pn, pt, 0, 64, None, 64, nws, None) == -1 and b"1..8" in lib.munit_last_error()
    p9 = arrays(9)
    assert fwd(p9[0], p9[1], p9[2], 9, 64, None, 64, nws, None) == -1 and b"1..8" in lib.munit_last_error()
    assert fwd(px, pn, pt, 3, 64, None, 64, nws - 1, None) == -1 and b"workspace" in lib.munit_last_error()
    pz = (c_size_t * 3)(16, 0, 16)
    assert fwd(px, pz, pt, 3, 64, None, 64, nws, None) == -1 and b"segment 1" in lib.munit_last_error()
    hole = (c_void_p * 3)(64, None, 64)
    assert fwd(hole, pn, pt, 3, 64, None, 64, nws, None) == -1
    assert bwd(None, pn, pt, 3, 64, px, None) == -1 and b"lsgan_bwd" in lib.munit_last_error()
    assert bwd(px, pn, pt, 3, None, px, None) == -1
    assert bwd(px, pn, pt, 3, 64, None, None) == -1
    assert bwd(px, pn, pt, 0, 64, px, None) == -1
    assert bwd(p9[0], p9[1], p9[2], 9, 64, p9[0], None) == -1
    assert bwd(px, pz, pt, 3, 64, px, None) == -1
    assert bwd(px, pn, pt, 3, 64, hole, None) == -1
