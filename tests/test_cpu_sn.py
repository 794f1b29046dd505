"""Host-side checks of spectral normalisation in the discriminators (dis.norm: sn): the fp64 oracle against the reference's
fixture (values per pass, the latest-(u, v) gradient rule, the state after every call), the module's keys, parameter order,
requires_grad flags and seeded construction against the same fixture, weights_init, the optimizer's parameter list, the
refusals and the C ABI."""
import os
import re

import pytest
import torch

from oracle import munit_oracle as O
from tests import sn_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("munit_sn_power_iter_workspace_bytes", "munit_sn_power_iter", "munit_sn_act_fwd", "munit_sn_act_bwd_workspace_bytes",
       "munit_sn_act_bwd", "munit_sn_grad_fix")
# the oracle and the reference both run in fp64 on the same numbers: agreement to rounding (measured: see the prints)
FIX_TOL = 1e-10


@pytest.fixture(scope="module")
def fixture():
    return S.load_fixture()


def nerr(a, ref):
    den = float(ref.abs().max())
    return float((a.double() - ref.double()).abs().max()) / (den if den else 1.0)


def _hp(size=64, **dis):
    hp = O.default_hp(size, 2, 1)
    hp["gen"]["n_res"] = 1
    hp["dis"] = dict(hp["dis"], **dis)
    return hp


def check_call(fx, sd, hp_dis, rec, xs, tol, what):
    """one recorded call of the fixture on the oracle state `sd` (advanced in place): loss, gradients, u / v afterwards"""
    arr = fx["arr"]
    xs = [x.clone().requires_grad_(True) for x in xs]
    names = list(rec["param_grads"])
    loss = S.calc(rec["fn"], sd, hp_dis, *xs)
    grads = torch.autograd.grad(loss, [sd[n] for n in names] + xs)
    rel = abs(float(loss.detach()) - rec["loss"]) / abs(rec["loss"])
    errs = {n: nerr(g, arr[rec["param_grads"][n]]) for n, g in zip(names, grads)}
    errs.update({"dx%d" % i: nerr(g, arr[k]) for i, (g, k) in enumerate(zip(grads[len(names):], rec["input_grads"]))})
    errs.update({k: nerr(sd.uv[k], arr[a]) for k, a in rec["uv_after"].items()})
    print("%s %s: loss %.12f rel %.1e, worst of %d tensors %.1e" % (what, rec["fn"], rec["loss"], rel, len(errs),
                                                                   max(errs.values())))
    assert rel <= tol and max(errs.values()) <= tol, (what, rec["fn"], rel, {k: v for k, v in errs.items() if v > tol})


def test_oracle_reproduces_the_reference_fixture(fixture):
    """The four calls on ONE network, in the fixture's order: the fake pass of calc_dis_loss runs with the sigma of one
    iteration, the real pass with that of two, calc_gen_loss with that of three, and so on; every gradient of weight_bar
    carries the sigma term of both passes taken with the latest (u, v)."""
    fx, arr = fixture, fixture["arr"]
    assert fx["hp_a"]["norm"] == "sn" and [c["fn"] for c in fx["calls"]] == ["calc_dis_loss", "calc_gen_loss",
                                                                             "calc_dis_loss_sr", "calc_gen_loss_sr"]
    sd = S.from_full({k: arr[a] for k, a in fx["initial"].items()})
    assert list(sd) == [n for n, rg in fx["named_parameters"] if rg]
    assert list(S.param_shapes(fx["hp_a"], 3)) == fx["state_keys"]
    for rec in fx["calls"]:
        if rec["fn"].startswith("calc_dis"):
            assert list(rec["param_grads"]) == list(sd)           # every trainable parameter, in full
        check_call(fx, sd, fx["hp_a"], rec, [arr[fx["inputs"][k]].double() for k in rec["inputs"]], FIX_TOL, "network A")
    b = fx["b"]
    sd = S.from_full({k: arr[a] for k, a in b["initial"].items()})
    shapes = {tuple(v.shape) for k, v in sd.items() if k.endswith("weight_bar")}
    assert shapes == {(12, 6, 4, 4), (24, 12, 4, 4)}
    check_call(fx, sd, fx["hp_b"], b["call"], [arr[b["x"]].double()], FIX_TOL, "network B")


def test_each_pass_with_its_own_u_v_is_not_what_the_reference_computes(fixture):
    """The rule the fixture pins is a real choice: differentiating every pass's sigma with that pass's own (u, v) moves the
    gradient of weight_bar by far more than the bound."""
    fx, arr = fixture, fixture["arr"]
    sd = S.from_full({k: arr[a] for k, a in fx["initial"].items()})
    rec = fx["calls"][0]
    plain = S._Normalise.forward

    def frozen(ctx, w, sigma, u, v):
        return plain(ctx, w, sigma, u.clone(), v.clone())

    S._Normalise.forward = staticmethod(frozen)
    try:
        xs = [arr[fx["inputs"][k]].double() for k in rec["inputs"]]
        loss = S.calc(rec["fn"], sd, fx["hp_a"], *xs)
        names = [n for n in sd if n.endswith("weight_bar")]
        grads = torch.autograd.grad(loss, [sd[n] for n in names])
    finally:
        S._Normalise.forward = staticmethod(plain)
    assert abs(float(loss.detach()) - rec["loss"]) <= FIX_TOL * rec["loss"]           # the values do not depend on the rule
    worst = max(nerr(g, arr[rec["param_grads"][n]]) for n, g in zip(names, grads))
    print("own-(u, v) rule: worst weight_bar gradient error %.2e" % worst)
    assert worst > 1e-3


def test_module_state_matches_the_reference(fixture):
    """keys, parameter order, requires_grad flags, and -- under the fixture's seed -- the initial state bit for bit"""
    from munit_amd.networks import MsImageDis, SpectralNorm
    fx, arr = fixture, fixture["arr"]
    torch.manual_seed(fx["seeds"]["a"])
    net = MsImageDis(3, dict(fx["hp_a"]))
    assert list(net.state_dict()) == fx["state_keys"]
    assert [[n, p.requires_grad] for n, p in net.named_parameters()] == fx["named_parameters"]
    assert len(list(net.parameters())) == fx["n_parameters"] == 24
    assert len([p for p in net.parameters() if p.requires_grad]) == fx["n_trainable"] == 16
    for k, v in net.state_dict().items():
        ref = arr[fx["initial"][k]]
        assert v.dtype == ref.dtype == torch.float32 and tuple(v.shape) == tuple(ref.shape), k
        assert torch.equal(v, ref), k
    wrapped = [m for m in net.modules() if isinstance(m, SpectralNorm)]
    assert len(wrapped) == 4 and fx["inner_conv_owns_weight_before_forward"] == [False] * 4
    assert not any(hasattr(m.module, "weight") for m in wrapped)
    for s in range(2):                      # the first block of a scale and the final 1x1 convolution stay plain
        assert hasattr(net.cnns[s][0].conv, "weight") and hasattr(net.cnns[s][3], "weight")
    torch.manual_seed(fx["seeds"]["b"])
    net_b = MsImageDis(3, dict(fx["hp_b"]))
    for k, v in net_b.state_dict().items():
        assert torch.equal(v, arr[fx["b"]["initial"][k]]), k


def test_weights_init_passes_the_normalised_layers_by(fixture):
    from munit_amd.networks import MsImageDis
    from munit_amd.utils import weights_init
    fx, arr = fixture, fixture["arr"]
    torch.manual_seed(fx["seeds"]["a"])
    net = MsImageDis(3, dict(fx["hp_a"]))
    before = {k: v.clone() for k, v in net.state_dict().items()}
    torch.manual_seed(fx["seeds"]["init"])
    net.apply(weights_init("gaussian"))
    changed = []
    for k, v in net.state_dict().items():
        assert torch.equal(v, arr[fx["after_weights_init_gaussian"][k]]), k
        if not torch.equal(v, before[k]):
            changed.append(k)
    assert changed and not any(".module." in k for k in changed)      # weight_bar keeps its default init, bias is not zeroed
    assert all(float(net.state_dict()[k].abs().max()) > 0 for k in before if k.endswith("module.bias"))


def test_the_optimizer_sees_bias_before_weight_bar_and_never_u_v():
    from munit_amd.trainer import MUNIT_Trainer
    torch.manual_seed(0)
    hp = _hp(norm="sn", dim=8, n_layer=3, num_scales=2)
    tr = MUNIT_Trainer(hp)
    want = [p for d in (tr.dis_a, tr.dis_b) for n, p in d.named_parameters() if not n.endswith(("weight_u", "weight_v"))]
    assert len(tr.dis_opt._plist) == len(want) == 32 and all(a is b for a, b in zip(tr.dis_opt._plist, want))
    names = [n for n, _ in tr.dis_a.named_parameters()]
    assert names.index("cnns.0.1.conv.module.bias") < names.index("cnns.0.1.conv.module.weight_bar")
    uv = [p for d in (tr.dis_a, tr.dis_b) for n, p in d.named_parameters() if n.endswith(("weight_u", "weight_v"))]
    assert len(uv) == 16 and not any(p.requires_grad for p in uv)
    assert not any(hasattr(p, "_munit_grad") for p in uv) and all(hasattr(p, "_munit_grad") for p in want)
    # u and v are unit vectors, and the state dict round-trips through the reference's keys
    assert all(abs(float(p.norm()) - 1.0) < 1e-6 for p in uv)
    sd = tr._plain(tr.dis_a.state_dict())
    assert "cnns.1.2.conv.module.weight_v" in sd and sd["cnns.1.2.conv.module.weight_v"].shape == (16 * 16,)
    tr2 = MUNIT_Trainer(hp)
    tr2.dis_a.load_state_dict(sd)
    assert all(torch.equal(a, b) for a, b in zip(tr2.dis_a.state_dict().values(), tr.dis_a.state_dict().values()))
    # weights_init at construction (trainer.py:124-127) left weight_bar at nn.Conv2d's default: not N(0, 0.02)
    w = tr.dis_a.cnns[0][2].conv.module.weight_bar.detach()
    bound = 1 / (16 * 16) ** 0.5
    assert float(w.abs().max()) <= bound and float(w.std()) > 0.5 * bound / 3 ** 0.5


def test_refusals(monkeypatch):
    from munit_amd import networks as N
    from munit_amd import trainer as T
    with pytest.raises(NotImplementedError, match="bn"):
        N.Conv2dBlock(4, 4, 3, 1, 1, norm="bn")
    with pytest.raises(NotImplementedError):
        N.LinearBlock(4, 4, norm="sn")
    made = []
    monkeypatch.setattr(T, "MsImageDis", lambda *a, **k: made.append(a) or pytest.fail("a network was built"))
    with pytest.raises(NotImplementedError, match=r"dis\.norm: sn.*fp32 only"):
        T.MUNIT_Trainer(dict(_hp(norm="sn"), precision="bf16s"))
    with pytest.raises(NotImplementedError, match=r"dis\.norm: sn.*fp32 only"):
        T.MUNIT_Trainer(dict(_hp(norm="sn"), precision="bf16"))
    monkeypatch.setattr(T, "dp_size", lambda: 2)
    with pytest.raises(NotImplementedError, match=r"dis\.norm: sn.*data-parallel.*world size 2"):
        T.MUNIT_Trainer(_hp(norm="sn"))
    assert made == []


def test_the_output_classifiers_are_normalised_too():
    from munit_amd.networks import SpectralNorm
    from munit_amd.trainer import MUNIT_Trainer
    hp = _hp(norm="sn", dim=8, n_layer=3, num_scales=2)
    hp["adaptation"].update(output_classifier_lambda=1, output_adv_lambda=1)
    tr = MUNIT_Trainer(hp)
    for net in (tr.output_classifier_sr_a, tr.output_classifier_sr_b):
        assert len([m for m in net.modules() if isinstance(m, SpectralNorm)]) == 4
    assert len(tr.output_classif_opt_sr._plist) == 32


def test_new_symbols_are_declared_listed_and_exported():
    from ctypes import sizeof
    from munit_amd import _lib
    header = open(os.path.join(ROOT, "include", "munit_hip.h")).read()
    declared = set(re.findall(r"\b(munit_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert sizeof(_lib.SnItem) == 48
    # workspace queries and host-side argument checks (no device needed: the "device" pointers are never followed)
    q = lib.munit_sn_power_iter_workspace_bytes
    assert q(9, 512, 4096) >= 9 * (16 * 4096 + 512) * 4 and q(1, 16, 128) > 0
    assert q(0, 16, 128) == 0 and q(1, 0, 128) == 0 and q(1, 16, 0) == 0 and q(1, 16, 8193) == 0
    nws = q(2, 16, 128)
    it = lib.munit_sn_power_iter
    assert it(None, 2, 16, 128, 64, 64, nws, None) == -1 and b"sn_power_iter" in lib.munit_last_error()
    assert it(64, 0, 16, 128, 64, 64, nws, None) == -1
    assert it(64, 2, 16, 128, None, 64, nws, None) == -1
    assert it(64, 2, 16, 8193, 64, 64, 1 << 30, None) == -1 and b"8192" in lib.munit_last_error()
    assert it(64, 2, 16, 128, 64, 64, nws - 1, None) == -2 and b"workspace" in lib.munit_last_error()
    fwd, bwd, fix = lib.munit_sn_act_fwd, lib.munit_sn_act_bwd, lib.munit_sn_grad_fix
    assert fwd(None, 64, 64, 64, 8, 4, 0, 0.2, None) == -1 and fwd(64, None, 64, 64, 8, 4, 0, 0.2, None) == -1
    assert fwd(64, 64, 64, 64, 0, 4, 0, 0.2, None) == -1 and fwd(64, 64, 64, 64, 8, 4, 7, 0.2, None) == -1
    bws = lib.munit_sn_act_bwd_workspace_bytes(8, 4)
    assert bws > 0 and lib.munit_sn_act_bwd_workspace_bytes(0, 4) == 0 and lib.munit_sn_act_bwd_workspace_bytes(8, 0) == 0
    assert bwd(None, 64, 64, 64, 64, 64, 0.0, 64, 8, 4, 0, 0.2, 64, bws, None) == -1
    assert bwd(64, 64, 64, 64, 64, 64, 0.5, 64, 8, 4, 0, 0.2, 64, bws, None) == -1 and b"beta" in lib.munit_last_error()
    assert bwd(64, 64, None, 64, 64, 64, 0.0, 64, 8, 4, 0, 0.2, 64, bws, None) == -1
    assert bwd(64, 64, 64, 64, 64, 64, 0.0, 64, 8, 4, 0, 0.2, 64, bws - 1, None) == -2
    assert fix(None, 64, 64, 64, 4, 2, 2, 3, 1.0, None) == -1 and fix(64, 64, 64, 64, 4, 0, 2, 3, 1.0, None) == -1
    assert fix(64, 64, 64, 64, 4, 2, 2, 3, 2.0, None) == -1 and b"beta" in lib.munit_last_error()
