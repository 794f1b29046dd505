"""Host-side checks of feature-level domain adaptation (adaptation.adv_lambda / dfeat_lambda): the fp64 oracle against the
reference's fixture, the modules' state_dict layout, the trainer's construction, refusals and checkpoints, the C ABI."""
import json
import os
import re

import pytest
import torch

from oracle import munit_oracle as O
from tests import featda_oracle as D
from tests.golden.make_golden_featda import BATCH, CODE, SEED_A, SEED_B, SEED_CA, SEED_CB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("munit_batchnorm_workspace_bytes", "munit_batchnorm_fwd", "munit_batchnorm_bwd", "munit_maxpool2_fwd",
       "munit_maxpool2_bwd", "munit_avgpool16_fwd", "munit_avgpool16_bwd")


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "golden_featda.json")) as f:
        return json.load(f)


def _check_digest(got, ref, rel=1e-9):
    t = got.detach().double().reshape(-1)
    assert t.numel() == ref["numel"]
    for key, val, bound in (("sum", float(t.sum()), ref["abs"]), ("abs", float(t.abs().sum()), ref["abs"]),
                            ("sq", float((t * t).sum()), ref["sq"])):
        assert abs(val - ref[key]) <= rel * bound, key
    assert (t[torch.tensor(ref["idx"])] - torch.tensor(ref["val"], dtype=torch.float64)).abs().max().item() \
        <= rel * t.abs().max().item()


def _hp(size=256, **adaptation):
    hp = O.default_hp(size, 2, 1)
    hp["gen"]["n_res"] = 1
    hp["dis"]["num_scales"] = 1
    hp["adaptation"].update(adaptation)
    return hp


def test_oracle_reproduces_the_reference_fixture(fixture):
    """tests/featda_oracle.py against the reference's own domainClassifier in fp64: outputs, the three losses, the gradient of
    the fooling loss with respect to the code, the running statistics after one and two forward passes, B = 1."""
    fx = fixture
    assert (fx["batch"], fx["code"]) == (BATCH, CODE)
    sd_a, sd_b = D.make_state(SEED_A), D.make_state(SEED_B)
    c_a, c_b = D.code(BATCH, CODE, CODE, SEED_CA), D.code(BATCH, CODE, CODE, SEED_CB)
    ca = c_a.clone().requires_grad_(True)
    o_a, o_b = D.classifier(sd_a, ca), D.classifier(sd_b, c_b)
    assert list(o_a.shape) == fx["out_shape"]
    ref_a, ref_b = torch.tensor(fx["out_a"], dtype=torch.float64), torch.tensor(fx["out_b"], dtype=torch.float64)
    assert (o_a.detach().reshape(-1) - ref_a).abs().max() <= 1e-10 * max(1.0, float(ref_a.abs().max()))
    assert (o_b.detach().reshape(-1) - ref_b).abs().max() <= 1e-10 * max(1.0, float(ref_b.abs().max()))
    for k, ref in fx["running_1"].items():
        _check_digest(sd_a[k], ref)
    assert int(sd_a["BasicBlock1.bn1.num_batches_tracked"]) == fx["tracked_1"] == 1
    for name, synth, fool in (("fool", False, True), ("synth", True, False), ("real", False, False)):
        t = D.target(synth, fool)
        loss = torch.mean((o_a - t) ** 2) + torch.mean((o_b - t) ** 2)
        assert abs(float(loss.detach()) - fx["loss_" + name]) <= 1e-10 * abs(fx["loss_" + name]), name
    (torch.mean((o_a - 0.5) ** 2) + torch.mean((o_b - 0.5) ** 2)).backward()
    _check_digest(ca.grad, fx["d_code_fool"])
    with torch.no_grad():
        D.classifier(sd_a, c_b)
    for k, ref in fx["running_2"].items():
        _check_digest(sd_a[k], ref)
    assert int(sd_a["BasicBlock1.bn1.num_batches_tracked"]) == fx["tracked_2"] == 2
    with torch.no_grad():
        o1 = D.classifier(sd_a, c_a[:1])
    assert list(o1.shape) == fx["out_b1_shape"] == [1]
    assert abs(float(o1) - fx["out_b1"][0]) <= 1e-10


def test_sr_loss_is_the_three_targets(fixture):
    sd_a, sd_b = D.make_state(SEED_A), D.make_state(SEED_B)
    c_a, c_b = D.code(BATCH, CODE, CODE, SEED_CA), D.code(BATCH, CODE, CODE, SEED_CB)
    for name, synth, fool in (("fool", False, True), ("fool", True, True), ("synth", True, False), ("real", False, False)):
        a, b = {k: v.clone() for k, v in sd_a.items()}, {k: v.clone() for k, v in sd_b.items()}
        with torch.no_grad():
            loss = D.sr_loss(a, b, c_a, c_b, synth, fool)
        assert abs(float(loss) - fixture["loss_" + name]) <= 1e-10 * abs(fixture["loss_" + name]), (name, synth)


def test_module_state_dict_is_the_reference_s(fixture):
    from munit_amd.networks import domainClassifier
    net = domainClassifier(256)
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert got == fixture["keys"]
    assert got == [[k, list(s)] for k, s in D.shapes().items()]
    assert net.state_dict()["BasicBlock1.bn1.num_batches_tracked"].dtype == torch.long
    sd = {k: v.float() if v.is_floating_point() else v for k, v in D.make_state(SEED_A).items()}
    net.load_state_dict(sd, strict=True)
    assert torch.equal(net.BasicBlock2.downsample[0].weight, sd["BasicBlock2.downsample.0.weight"])
    assert torch.equal(net.fc.bias, sd["fc.bias"])
    with pytest.raises(ValueError, match="16..31"):
        net(torch.zeros(1, 256, 32, 64))            # refused before any device work
    with pytest.raises(ValueError, match="16..31"):
        net(torch.zeros(1, 256, 64, 128))


def test_trainer_builds_the_classifiers_under_their_own_optimizer():
    from munit_amd.trainer import MUNIT_Trainer
    torch.manual_seed(0)
    tr = MUNIT_Trainer(_hp(adv_lambda=6, dfeat_lambda=1))
    assert tr.use_classifier_sr
    mine = {id(p) for m in (tr.domain_classifier_sr_a, tr.domain_classifier_sr_b) for p in m.parameters()}
    assert len(mine) == 2 * len(D.param_names())
    assert [id(p) for p in tr.classif_opt_sr._plist] == \
        [id(p) for m in (tr.domain_classifier_sr_a, tr.domain_classifier_sr_b) for p in m.parameters()]
    assert type(tr.classif_opt_sr).__name__ == "FusedAdam" and tr.classif_opt_sr.flat_p is not None
    for opt in (tr.gen_opt, tr.dis_opt):
        assert not mine & {id(p) for p in opt._plist}
    for p in tr.domain_classifier_sr_a.parameters():
        assert p._munit_opt is tr.classif_opt_sr and p._munit_grad is not None
    w = tr.domain_classifier_sr_a.BasicBlock1.conv1.weight
    assert abs(float(w.std()) - 0.02) < 2e-3 and float(tr.domain_classifier_sr_a.fc.bias.abs().max()) == 0    # "gaussian"
    assert float(tr.domain_classifier_sr_a.BasicBlock1.bn1.weight.min()) == 1.0                       # untouched by it
    x = _hp(adv_lambda=6, dfeat_lambda=1)
    x["optimizer"] = "extraadam"
    assert type(MUNIT_Trainer(x).classif_opt_sr).__name__ == "FusedExtraAdam"
    off = MUNIT_Trainer(_hp())
    assert not hasattr(off, "classif_opt_sr") and not hasattr(off, "domain_classifier_sr_a")
    for name in ("classif_opt_sr_step", "compute_classifier_sr_loss", "domain_classifier_sr_update"):
        assert callable(getattr(MUNIT_Trainer, name))


def test_refusals_name_the_weight_and_touch_nothing(monkeypatch):
    from munit_amd import trainer as T
    with pytest.raises(ValueError, match="adv_lambda.*dfeat_lambda"):
        T.MUNIT_Trainer(_hp(adv_lambda=6))
    for prec in ("bf16", "bf16s"):
        hp = _hp(adv_lambda=6, dfeat_lambda=1)
        hp["precision"] = prec
        with pytest.raises(NotImplementedError, match="dfeat_lambda"):
            T.MUNIT_Trainer(hp)
    for size in (128, 512):
        with pytest.raises(ValueError, match="dfeat_lambda.*16..31"):
            T.MUNIT_Trainer(_hp(size, dfeat_lambda=1))
    monkeypatch.setattr(T, "dp_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="adv_lambda.*dfeat_lambda.*data-parallel"):
        T.MUNIT_Trainer(_hp(adv_lambda=6, dfeat_lambda=1))
    monkeypatch.undo()
    # the still-unsupported weights stay refused
    for k in ("sem_seg_lambda", "output_classifier_lambda", "output_adv_lambda"):
        with pytest.raises(NotImplementedError, match=k):
            T.MUNIT_Trainer(_hp(**{k: 1}))
    for k in ("domain_adv_w", "vgg_w"):
        hp = _hp()
        hp[k] = 1
        with pytest.raises(NotImplementedError, match=k):
            T.MUNIT_Trainer(hp)
    # a trainer built without the classifiers refuses the term in gen_update before it touches its gradient buffer
    tr = T.MUNIT_Trainer(_hp())
    tr.gen_opt.flat_g.fill_(3.0)
    x = torch.zeros(2, 3, 256, 256)
    with pytest.raises(ValueError, match="adv_lambda"):
        tr.gen_update(x, x, _hp(adv_lambda=6))
    with pytest.raises(ValueError, match="dfeat_lambda"):
        tr.domain_classifier_sr_update(x, x, False, 1.0, 0)
    assert bool((tr.gen_opt.flat_g == 3.0).all())
    # ... and one built with them refuses a world that grew, likewise
    tr = T.MUNIT_Trainer(_hp(adv_lambda=6, dfeat_lambda=1))
    tr.gen_opt.flat_g.fill_(3.0)
    tr.classif_opt_sr.flat_g.fill_(3.0)
    monkeypatch.setattr(T, "dp_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="adv_lambda"):
        tr.gen_update(x, x, _hp(adv_lambda=6, dfeat_lambda=1))
    with pytest.raises(NotImplementedError, match="dfeat_lambda"):
        tr.domain_classifier_sr_update(x, x, False, 1.0, 0)
    assert bool((tr.gen_opt.flat_g == 3.0).all()) and bool((tr.classif_opt_sr.flat_g == 3.0).all())


def test_save_writes_the_same_files(tmp_path):
    from munit_amd.trainer import MUNIT_Trainer
    names = []
    for sub, ad in (("off", {}), ("on", dict(adv_lambda=6, dfeat_lambda=1))):
        d = tmp_path / sub
        d.mkdir()
        torch.manual_seed(0)
        MUNIT_Trainer(_hp(**ad)).save(str(d), 2)
        names.append(sorted(os.listdir(str(d))))
    assert names[0] == names[1] == ["dis_00000003.pt", "gen_00000003.pt", "optimizer.pt"]
    opt = torch.load(str(tmp_path / "on" / "optimizer.pt"), weights_only=True)
    assert sorted(opt) == ["dis", "gen"]
    gen = torch.load(str(tmp_path / "on" / "gen_00000003.pt"), weights_only=True)
    assert not any("classifier" in k for k in gen["2"])


def test_new_symbols_are_declared_listed_and_exported():
    from munit_amd import _lib
    header = open(os.path.join(ROOT, "include", "munit_hip.h")).read()
    declared = set(re.findall(r"\b(munit_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # host-side argument checks run before any launch (no device needed): negative return + munit_last_error
    assert lib.munit_batchnorm_workspace_bytes(64) > 0
    assert lib.munit_maxpool2_fwd(None, None, None, 1, 4, 4, 64, None) == -1
    assert b"maxpool2_fwd" in lib.munit_last_error()
    assert lib.munit_avgpool16_fwd(8, 8, 1, 15, 16, 64, None) == -1 and b"16..31" in lib.munit_last_error()
    assert lib.munit_avgpool16_bwd(8, 8, 1, 16, 32, 64, None) == -1 and b"16..31" in lib.munit_last_error()
    assert lib.munit_maxpool2_bwd(8, 8, 8, 1, 4, 4, 6, None) == -1
    assert lib.munit_batchnorm_fwd(8, 8, 8, 8, 8, 8, 1, 64, 8, 8, 0, 0, 1e-5, 0.1, 8, 1 << 20, None) == -1   # R = 1 in training
    assert b"more than one value" in lib.munit_last_error()
    assert lib.munit_batchnorm_fwd(8, 8, 8, 8, 8, 8, 64, 24, 8, 8, 0, 0, 1e-5, 0.1, 8, 1 << 20, None) == -1  # 256 % (24 / 4) != 0
    assert lib.munit_batchnorm_fwd(8, 8, 8, 8, 8, 8, 64, 64, 8, 8, 0, 0, 1e-5, 0.1, 8, 16, None) == -2       # workspace
    assert lib.munit_batchnorm_bwd(8, 8, None, 8, 8, 8, 8, None, None, 0.0, 64, 64, 1, 8, 1 << 20, None) == -1  # ReLU without y
