"""Host-side checks of the non-saturating GAN loss (dis.gan_type: nsgan): the fp64 oracle against the reference's fixture,
the literal and the softplus form against each other, the C ABI of the multi-scale nsgan loss, the trainer's construction
and refusals."""
import json
import os
import re
from ctypes import c_float, c_size_t, c_void_p

import pytest
import torch

from oracle import munit_oracle as O
from tests import nsgan_oracle as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("munit_nsgan_workspace_bytes", "munit_nsgan_fwd", "munit_nsgan_bwd")


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "golden_nsgan.json")) as f:
        fx = json.load(f)
    fx["sd"] = {k: torch.tensor(v["data"], dtype=torch.float64).reshape(v["shape"]) for k, v in fx["weights"].items()}
    for p in fx["pairs"]:
        for k in ("fake", "real"):
            p[k] = torch.tensor(p[k], dtype=torch.float64).reshape(2, 3, 16, 16)
    return fx


def _check_digest(got, ref, rel=1e-9):
    t = got.detach().double().reshape(-1)
    assert t.numel() == ref["numel"]
    for key, val, bound in (("sum", float(t.sum()), ref["abs"]), ("abs", float(t.abs().sum()), ref["abs"]),
                            ("sq", float((t * t).sum()), ref["sq"])):
        assert abs(val - ref[key]) <= rel * bound, key
    assert (t[torch.tensor(ref["idx"])] - torch.tensor(ref["val"], dtype=torch.float64)).abs().max().item() \
        <= rel * t.abs().max().item()


def _hp(size=64, **dis):
    hp = O.default_hp(size, 2, 1)
    hp["gen"]["n_res"] = 1
    hp["dis"] = dict(hp["dis"], **dis)
    return hp


def test_oracle_reproduces_the_reference_fixture(fixture):
    """tests/nsgan_oracle.py against the reference's own MsImageDis (nsgan) in fp64: the three losses and their input
    gradients on both input pairs, at the project's fixture bound of 1e-9 relative (measured 2e-15)."""
    fx, hd = fixture, fixture["hp_dis"]
    assert hd["gan_type"] == "nsgan" and [p["scale"] for p in fx["pairs"]] == [1.0, 40.0]
    assert fx["gen_loss_sr_raises"] == ["NameError", "name 'out1' is not defined"]
    # the literal form is a yardstick only while the sigmoid is far from saturation: the fixture's logits stay below 8
    assert fx["max_abs_logit"] < 8
    worst = N.max_logit(fx["sd"], [p[k] for p in fx["pairs"] for k in ("fake", "real")], hd)
    assert abs(worst - fx["max_abs_logit"]) <= 1e-9 * worst
    for p in fx["pairs"]:
        x0, x1 = p["fake"].clone().requires_grad_(True), p["real"].clone().requires_grad_(True)
        for name, loss, grads in (
                ("dis", N.dis_loss_d(fx["sd"], "", x0, x1, hd), (("d_fake_dis", x0), ("d_real_dis", x1))),
                ("gen", N.dis_loss_g(fx["sd"], "", x0, hd), (("d_fake_gen", x0),)),
                ("dis_sr", N.dis_loss_sr(fx["sd"], x0, x1, hd), (("d_sim_dis_sr", x0), ("d_real_dis_sr", x1)))):
            ref = p["loss_" + name]
            rel = abs(float(loss.detach()) - ref) / abs(ref)
            print("nsgan oracle, scale %g, %s: %.12f rel %.1e" % (p["scale"], name, ref, rel))
            assert rel <= 1e-9
            for (key, x), g in zip(grads, torch.autograd.grad(loss, [x for _, x in grads])):
                _check_digest(g, p[key])


def test_the_literal_and_the_softplus_form_agree_on_the_fixture(fixture):
    fx, hd = fixture, fixture["hp_dis"]
    for p in fx["pairs"]:
        xs = [p["fake"].clone().requires_grad_(True), p["real"].clone().requires_grad_(True)]
        for lit, sp in ((N.dis_loss_d(fx["sd"], "", xs[0], xs[1], hd), N.dis_loss_d(fx["sd"], "", xs[0], xs[1], hd, N.softplus)),
                        (N.dis_loss_g(fx["sd"], "", xs[0], hd), N.dis_loss_g(fx["sd"], "", xs[0], hd, N.softplus)),
                        (N.dis_loss_sr(fx["sd"], xs[0], xs[1], hd), N.dis_loss_sr(fx["sd"], xs[0], xs[1], hd, N.softplus))):
            assert abs(float(lit.detach()) - float(sp.detach())) <= 1e-12 * abs(float(lit.detach()))
            for a, b in zip(torch.autograd.grad(lit, xs, allow_unused=True), torch.autograd.grad(sp, xs, allow_unused=True)):
                assert (a is None) == (b is None)
                if a is not None:
                    assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())


def test_swapped_puts_the_nsgan_losses_into_the_oracle_and_takes_them_out():
    plain = O.dis_loss_d, O.dis_loss_g
    with N.swapped():
        assert (O.dis_loss_d, O.dis_loss_g) == (N.dis_loss_d, N.dis_loss_g)
    assert (O.dis_loss_d, O.dis_loss_g) == plain
    with pytest.raises(ZeroDivisionError):
        with N.swapped():
            1 / 0
    assert (O.dis_loss_d, O.dis_loss_g) == plain


def test_new_symbols_are_declared_listed_and_exported():
    from munit_amd import _lib
    header = open(os.path.join(ROOT, "include", "munit_hip.h")).read()
    declared = set(re.findall(r"\b(munit_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name, twin in zip(NEW, ("munit_lsgan_workspace_bytes", "munit_lsgan_fwd", "munit_lsgan_bwd")):
        assert name in declared and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[twin]                 # the argument lists of the LSGAN pair
    nws = lib.munit_nsgan_workspace_bytes(3)
    assert nws > 0 and lib.munit_nsgan_workspace_bytes(8) > 0
    assert lib.munit_nsgan_workspace_bytes(0) == 0 and lib.munit_nsgan_workspace_bytes(9) == 0

    # host-side argument checks run before any launch (no device needed): the "device" pointers are never followed
    def arrays(n, length=16, t=1.0):
        return (c_void_p * n)(*[64] * n), (c_size_t * n)(*[length] * n), (c_float * n)(*[t] * n)

    px, pn, pt = arrays(3)
    fwd, bwd = lib.munit_nsgan_fwd, lib.munit_nsgan_bwd
    assert fwd(None, pn, pt, 3, 64, None, 64, nws, None) == -1 and b"nsgan_fwd" in lib.munit_last_error()
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
    for bad in (0.5, -1.0, 2.0, 1.0000001, float("nan")):
        ph = (c_float * 3)(0.0, 1.0, bad)
        assert fwd(px, pn, ph, 3, 64, None, 64, nws, None) == -1 and b"target 2 must be 0 or 1" in lib.munit_last_error()
        assert bwd(px, pn, ph, 3, 64, px, None) == -1 and b"nsgan_bwd: target 2" in lib.munit_last_error()
    assert bwd(None, pn, pt, 3, 64, px, None) == -1 and b"nsgan_bwd" in lib.munit_last_error()
    assert bwd(px, None, pt, 3, 64, px, None) == -1
    assert bwd(px, pn, None, 3, 64, px, None) == -1
    assert bwd(px, pn, pt, 3, None, px, None) == -1
    assert bwd(px, pn, pt, 3, 64, None, None) == -1
    assert bwd(px, pn, pt, 0, 64, px, None) == -1
    assert bwd(p9[0], p9[1], p9[2], 9, 64, p9[0], None) == -1
    assert bwd(px, pz, pt, 3, 64, px, None) == -1
    assert bwd(px, pn, pt, 3, 64, hole, None) == -1


def test_the_trainer_constructs_with_nsgan():
    from munit_amd.trainer import MUNIT_Trainer
    torch.manual_seed(0)
    tr = MUNIT_Trainer(_hp(gan_type="nsgan"))
    assert tr.dis_a.gan_type == tr.dis_b.gan_type == "nsgan"
    ref = MUNIT_Trainer(_hp())
    assert list(tr.dis_a.state_dict()) == list(ref.dis_a.state_dict())          # the loss adds no parameter
    with pytest.raises(NotImplementedError, match="undefined variable"):
        tr.dis_a.calc_gen_loss_sr(torch.zeros(2, 3, 64, 64))


def test_nsgan_with_the_output_classifiers_is_refused_naming_both_keys(monkeypatch):
    from munit_amd import trainer as T
    hp = _hp(gan_type="nsgan")
    hp["adaptation"].update(output_classifier_lambda=1, output_adv_lambda=1)
    made = []
    monkeypatch.setattr(T, "MsImageDis", lambda *a, **k: made.append(a) or pytest.fail("a network was built"))
    with pytest.raises(NotImplementedError, match=r"dis\.gan_type: nsgan.*adaptation\.output_adv_lambda.*calc_gen_loss_sr"):
        T.MUNIT_Trainer(hp)
    assert made == []
    monkeypatch.undo()
    # the same pair of weights under lsgan constructs, as before
    hp = _hp()
    hp["adaptation"].update(output_classifier_lambda=1, output_adv_lambda=1)
    assert T.MUNIT_Trainer(hp).use_output_classifier_sr
    # a trainer built with nsgan refuses the term handed to a step, before it touches a gradient buffer
    tr = T.MUNIT_Trainer(_hp(gan_type="nsgan"))
    tr.gen_opt.flat_g.fill_(3.0)
    x = torch.zeros(2, 3, 64, 64)
    with pytest.raises(NotImplementedError, match=r"dis\.gan_type: nsgan.*adaptation\.output_adv_lambda"):
        tr.gen_update(x, x, dict(_hp(gan_type="nsgan"), adaptation=hp["adaptation"]))
    assert bool((tr.gen_opt.flat_g == 3.0).all())


def test_another_gan_type_still_dies_where_a_loss_is_called():
    from munit_amd.networks import MsImageDis
    net = MsImageDis(3, _hp(gan_type="wgan")["dis"])
    x = torch.zeros(2, 3, 64, 64)
    with pytest.raises(AssertionError, match="Unsupported GAN type: wgan"):
        net.calc_dis_loss(x, x)
    with pytest.raises(AssertionError, match="Unsupported GAN type: wgan"):
        net.calc_dis_loss_sr(x, x)
