"""CPU: the host side of the semantic-consistency loss -- checkpoint layout and loading, the BatchNorm fold, the fp64
oracle's loss formula and the trainer's configuration checks."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import munit_oracle as O
from tests import semantic_oracle as S


@pytest.fixture(scope="module")
def model():
    return S.make_model(0)


def _save(tmp_path, sd, name="seg.pth"):
    p = tmp_path / name
    torch.save(sd, str(p))
    return str(p)


def test_checkpoint_layout_and_strict_load(tmp_path, model):
    from munit_amd.utils import load_segmentation_model
    sd = model.state_dict()
    assert len(sd) == 218 and all(k.startswith("resnet34_8s.") for k in sd)
    assert sum(p.numel() for p in model.parameters()) == 21294419
    m = load_segmentation_model(_save(tmp_path, sd), 19)
    assert not m.training and not any(p.requires_grad for p in m.parameters())
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k])
    bad = dict(sd)
    bad["resnet34_8s.layer3.0.downsample.0.weight_renamed"] = bad.pop("resnet34_8s.layer3.0.downsample.0.weight")
    with pytest.raises(RuntimeError, match="downsample"):
        load_segmentation_model(_save(tmp_path, bad, "bad.pth"), 19)
    short = {k: v for k, v in sd.items() if not k.startswith("resnet34_8s.fc.")}
    with pytest.raises(RuntimeError, match="fc"):
        load_segmentation_model(_save(tmp_path, short, "short.pth"), 19)


def test_bn_fold_equals_eval_bn(model):
    from munit_amd.segmentation import fold_bn
    net = model.resnet34_8s
    g = torch.Generator().manual_seed(1)
    for conv, bn in ((net.conv1, net.bn1), (net.layer2[0].conv1, net.layer2[0].bn1),
                     (net.layer3[0].downsample[0], net.layer3[0].downsample[1])):
        cin = conv.weight.shape[1]
        x = torch.randn(2, cin, 12, 12, generator=g, dtype=torch.float64)
        s, p = conv.stride, conv.padding
        ref = F.batch_norm(F.conv2d(x, conv.weight.double(), None, s, p), bn.running_mean.double(),
                           bn.running_var.double(), bn.weight.double(), bn.bias.double(), False, 0.0, 1e-5)
        w, b = fold_bn(conv.weight, bn)
        got = F.conv2d(x, w, b, s, p)
        assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


def test_oracle_loss_formula():
    g = torch.Generator().manual_seed(2)
    out = torch.randn(2, 19, 8, 8, generator=g, dtype=torch.float64)
    tgt = torch.randint(0, 19, (2, 8, 8), generator=g)
    mask = (torch.rand(2, 1, 8, 8, generator=g) < 0.5).double()
    got = S.ce_loss(out, tgt, mask)
    m = mask.squeeze(1)
    # unmasked pixel: log-sum-exp over the 19 logits and a 20th logit 0; masked pixel: log(19 + e) - 1
    lse = torch.logsumexp(torch.cat([out, torch.zeros(2, 1, 8, 8, dtype=torch.float64)], 1), 1)
    pix = torch.where(m > 0, torch.full_like(m, math.log(19 + math.e) - 1), lse - out.gather(1, tgt[:, None])[:, 0])
    assert abs(got.item() - pix.mean().item()) < 1e-12
    assert abs(S.ce_loss(out, tgt).item() - F.cross_entropy(out, tgt).item()) < 1e-15


def test_constructor_accepts_semantic_with_checkpoint(tmp_path, model):
    from munit_amd.trainer import MUNIT_Trainer
    hp = O.default_hp(64, 1, 1)
    hp["semantic_w"] = 3
    hp["semantic_ckpt_path"] = _save(tmp_path, model.state_dict())
    tr = MUNIT_Trainer(hp)
    seg = tr.segmentation_model
    assert seg is not None and not seg.training
    assert not any(p.requires_grad for p in seg.parameters())
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in seg.state_dict().items())
    # the frozen network is not optimised
    ids = {id(p) for p in seg.parameters()}
    assert not any(id(p) in ids for grp in tr.gen_opt.param_groups for p in grp["params"])
    no_ckpt = O.default_hp(64, 1, 1)
    no_ckpt["semantic_w"] = 3
    with pytest.raises(NotImplementedError, match="semantic_w"):
        MUNIT_Trainer(no_ckpt)


@pytest.mark.parametrize("key,value,exc,match", [("precision", "bf16", NotImplementedError, "fp32"),
                                                 ("crop_image_width", 96, ValueError, "square"),
                                                 ("crop_image_height", 80, ValueError, "multiple of 32")])
def test_constructor_rejects_unsupported_semantic_configs(tmp_path, model, key, value, exc, match):
    from munit_amd.trainer import MUNIT_Trainer
    hp = O.default_hp(64, 1, 1)
    hp["semantic_w"] = 3
    hp["semantic_ckpt_path"] = _save(tmp_path, model.state_dict())
    hp[key] = value
    if key == "crop_image_height":
        hp["crop_image_width"] = value
    with pytest.raises(exc, match=match):
        MUNIT_Trainer(hp)


def test_gen_update_rejects_synthetic_ground_truth(tmp_path, model):
    from munit_amd.trainer import MUNIT_Trainer
    hp = O.default_hp(64, 1, 1)
    hp["semantic_w"] = 3
    hp["semantic_ckpt_path"] = _save(tmp_path, model.state_dict())
    tr = MUNIT_Trainer(hp)
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="semantic_gt"):
        tr.gen_update(x, x, hp, semantic_gt_a=torch.zeros(1, 64, 64), semantic_gt_b=torch.zeros(1, 64, 64))


def _check_digest(got, ref, rel=1e-9):
    t = got.detach().double().reshape(-1)
    assert t.numel() == ref["numel"]
    for key, val, bound in (("sum", float(t.sum()), ref["abs"]), ("abs", float(t.abs().sum()), ref["abs"]),
                            ("sq", float((t * t).sum()), ref["sq"])):
        assert abs(val - ref[key]) <= rel * bound, key
    assert (t[torch.tensor(ref["idx"])] - torch.tensor(ref["val"], dtype=torch.float64)).abs().max().item() <= rel * t.abs().max().item()


def test_oracle_matches_reference_fixture():
    """tests/semantic_oracle.py against digests of the reference's own scripts/resnet.py network and the loss written out
    from compute_semantic_seg_loss (tests/golden/make_golden_semantic.py), float64, 1e-9."""
    import json
    import os
    from tests.golden.make_golden_semantic import inputs
    with open(os.path.join(os.path.dirname(__file__), "golden", "golden_semantic.json")) as f:
        ref = json.load(f)
    m = S.make_model(0)
    sd = S.state(m)
    wsq = float(sum((v.double() ** 2).sum() for k, v in m.state_dict().items() if v.is_floating_point()))
    assert abs(wsq - ref["weights_sq"]) <= 1e-12 * ref["weights_sq"], "make_model(0) no longer builds the fixture's weights"
    x_orig, x_trans, mask = inputs()
    with torch.no_grad():
        _check_digest(S.logits(sd, x_trans, up=False), ref["logits_low"])
    for branch, msk in (("masked", mask), ("plain", None)):
        xt = x_trans.clone().requires_grad_(True)
        loss, labels = S.semantic_loss(sd, x_orig, xt, msk)
        _check_digest(labels.double(), ref["labels"], rel=0.0)
        loss.backward()
        assert abs(loss.item() - ref["loss_" + branch]) <= 1e-9 * abs(ref["loss_" + branch])
        _check_digest(xt.grad, ref["dx_" + branch])
