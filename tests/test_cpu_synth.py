"""CPU: the host side of the synthetic-pair generator step (recon_synth_w, semantic_gt_a / semantic_gt_b) -- the fp64
oracle of tests/synth_oracle.py against the reference fixture, the new C symbols and their host-side refusals, and
gen_update's argument checks."""
import json
import math
import os
import re
from ctypes import c_float, c_size_t, c_void_p

import pytest
import torch
import torch.nn.functional as F

from oracle import munit_oracle as O
from tests import semantic_oracle as S
from tests import synth_oracle as Y
from tests.test_cpu_semantic import _check_digest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("munit_pair_l1_fwd", "munit_pair_l1_bwd", "munit_seg_ce_gt_fwd", "munit_seg_ce_gt_bwd")


@pytest.fixture(scope="module")
def model():
    return S.make_model(0)


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "golden_synth.json")) as f:
        return json.load(f)


def test_merge_table_covers_every_class_once():
    members = [k for m in Y.MEMBERS for k in m]
    assert sorted(members) == list(range(19)) and Y.MEMBERS[0] == () and len(Y.MEMBERS) == 10
    out = torch.arange(19, dtype=torch.float64).view(1, 19, 1, 1) + 1
    assert Y.merge(out).flatten().tolist() == [0, 3, 12, 21, 9, 10, 11, 25, 51, 48]


def test_oracle_gt_loss_formula():
    g = torch.Generator().manual_seed(2)
    out = torch.randn(2, 19, 8, 8, generator=g, dtype=torch.float64)
    gt = torch.randint(0, 10, (2, 1, 8, 8), generator=g).double() + 0.75      # truncated like .type(torch.long)
    mask = (torch.rand(2, 1, 8, 8, generator=g) < 0.5).double()
    merged = Y.merge(out)
    tgt = gt.long().squeeze(1)
    assert abs(Y.ce_gt_loss(out, gt).item() - F.cross_entropy(merged, tgt).item()) < 1e-15
    # unmasked pixel: log-sum-exp over the 10 merged logits and an 11th logit 0; masked pixel: log(10 + e) - 1
    lse = torch.logsumexp(torch.cat([merged, torch.zeros(2, 1, 8, 8, dtype=torch.float64)], 1), 1)
    m = mask.squeeze(1)
    pix = torch.where(m > 0, torch.full_like(m, math.log(10 + math.e) - 1), lse - merged.gather(1, tgt[:, None])[:, 0])
    assert abs(Y.ce_gt_loss(out, gt, mask).item() - pix.mean().item()) < 1e-12
    assert abs(Y.ce_gt_loss(out, gt, torch.ones_like(mask)).item() - Y.MASKED_PIXEL_LOSS) < 1e-12


def test_oracle_matches_reference_fixture(fixture):
    """tests/synth_oracle.py against digests made with the reference's own merge_classes and scripts/resnet.py network and
    the two losses written out from scripts/trainer.py (tests/golden/make_golden_synth.py), float64, 1e-9."""
    from tests.golden.make_golden_synth import inputs
    ref = fixture
    m = S.make_model(0)
    sd = S.state(m)
    wsq = float(sum((v.double() ** 2).sum() for k, v in m.state_dict().items() if v.is_floating_point()))
    assert abs(wsq - ref["weights_sq"]) <= 1e-12 * ref["weights_sq"], "make_model(0) no longer builds the fixture's weights"
    x_trans, gt, mask, (x_a, x_b, x_ab, x_ba) = inputs()
    assert sorted(gt.unique().tolist()) == list(range(10))
    with torch.no_grad():
        _check_digest(Y.merge(S.logits(sd, x_trans)), ref["merged"])
    for branch, msk in (("masked", mask), ("plain", None)):
        xt = x_trans.clone().requires_grad_(True)
        loss = Y.ce_gt_loss(S.logits(sd, xt), gt, msk)
        loss.backward()
        assert abs(loss.item() - ref["loss_" + branch]) <= 1e-9 * abs(ref["loss_" + branch])
        _check_digest(xt.grad, ref["dx_" + branch])
    share = float(Y.alignment(x_a, x_b).mean())
    assert 0.1 <= share <= 0.9 and share == ref["aligned_share"]
    ab, ba = x_ab.clone().requires_grad_(True), x_ba.clone().requires_grad_(True)
    loss = Y.pair_loss(x_a, x_b, ab, ba)
    loss.backward()
    assert abs(loss.item() - ref["loss_pair"]) <= 1e-9 * abs(ref["loss_pair"])
    _check_digest(ab.grad, ref["d_ab"])
    _check_digest(ba.grad, ref["d_ba"])
    # the pinned form used inside a step parity (oracle.munit_oracle.l1_masked without pins) is the same number
    assert Y.pair_loss(x_a, x_b, x_ab, x_ba, O.l1_masked).item() == Y.pair_loss(x_a, x_b, x_ab, x_ba).item()


def test_new_symbols_in_header_and_library():
    import __graft_entry__ as g
    g.build()
    from munit_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "munit_hip.h")).read()
    declared = set(re.findall(r"\b(munit_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "NaN" in header[header.index("munit_seg_ce_gt_fwd") - 1200:header.index("munit_seg_ce_gt_fwd")]
    from munit_amd import ops
    assert callable(ops.pair_l1) and callable(ops.seg_cross_entropy_gt)


def test_new_entry_points_refuse_bad_arguments_on_the_host():
    """NULL pointers, non-positive sizes, C outside 1..4 and a short workspace are refused before any launch (no GPU is
    touched: the pointers handed over are never dereferenced on the host)."""
    import __graft_entry__ as g
    g.build()
    from munit_amd import _lib
    lib = _lib.load()
    p = c_void_p(4096)
    n = c_size_t(16)
    big = c_size_t(1 << 20)
    assert lib.munit_pair_l1_fwd(None, p, p, p, n, 3, p, p, big, None) == -1
    assert lib.munit_pair_l1_fwd(p, p, p, p, c_size_t(0), 3, p, p, big, None) == -1
    assert lib.munit_pair_l1_fwd(p, p, p, p, n, 5, p, p, big, None) == -1
    assert lib.munit_pair_l1_fwd(p, p, p, p, n, 0, p, p, big, None) == -1
    assert lib.munit_pair_l1_fwd(p, p, p, p, n, 3, p, None, big, None) == -1
    need = lib.munit_loss_workspace_bytes(c_size_t(48))
    assert lib.munit_pair_l1_fwd(p, p, p, p, n, 3, p, p, c_size_t(need - 1), None) != 0
    assert b"workspace" in lib.munit_last_error()
    assert lib.munit_pair_l1_bwd(p, p, p, None, n, 3, p, p, p, None) == -1
    assert lib.munit_pair_l1_bwd(p, p, p, p, n, 3, None, p, p, None) == -1
    assert lib.munit_pair_l1_bwd(p, p, p, p, n, 7, p, p, p, None) == -1
    one = c_float(1.0)
    assert lib.munit_seg_ce_gt_fwd(p, None, None, 1, 2, 2, 8, one, p, p, big, None) == -1
    assert lib.munit_seg_ce_gt_fwd(p, p, None, 0, 2, 2, 8, one, p, p, big, None) == -1
    assert lib.munit_seg_ce_gt_fwd(p, p, None, 1, 2, 2, 8, c_float(0.0), p, p, big, None) == -1
    assert lib.munit_seg_ce_gt_fwd(p, p, None, 4096, 4096, 4096, 8, one, p, p, big, None) == -1
    assert lib.munit_seg_ce_gt_fwd(p, p, None, 1, 2, 2, 8, one, p, p, c_size_t(3), None) == -2
    assert lib.munit_seg_ce_gt_bwd(p, p, None, 1, 2, 2, 8, one, None, p, p, big, None) == -1
    assert lib.munit_seg_ce_gt_bwd(p, p, None, 1, 2, 2, 0, one, p, p, p, big, None) == -1
    assert lib.munit_seg_ce_gt_bwd(p, p, None, 1, 2, 2, 8, one, p, p, p, c_size_t(256 * 19 * 4 - 1), None) == -2


def _semantic_trainer(tmp_path, model, **over):
    from munit_amd.trainer import MUNIT_Trainer
    hp = O.default_hp(64, 1, 1)
    hp["semantic_w"] = 3
    p = tmp_path / "seg.pth"
    torch.save(model.state_dict(), str(p))
    hp["semantic_ckpt_path"] = str(p)
    hp.update(over)
    return MUNIT_Trainer(hp), hp


@pytest.mark.parametrize("case", ["only_a", "only_b", "wrong_size", "wrong_rank", "two_channels", "label_10", "label_-1",
                                  "label_nan", "bool"])
def test_gen_update_rejects_bad_ground_truth(tmp_path, model, case):
    tr, hp = _semantic_trainer(tmp_path, model)
    x = torch.zeros(1, 3, 64, 64)
    good = torch.zeros(1, 1, 64, 64)
    a, b = good, good.clone()
    if case == "only_a":
        b = None
    elif case == "only_b":
        a = None
    elif case == "wrong_size":
        b = torch.zeros(1, 1, 32, 32)
    elif case == "wrong_rank":
        a = torch.zeros(64, 64)
    elif case == "two_channels":
        a = torch.zeros(1, 2, 64, 64)
    elif case == "label_10":
        b[0, 0, 63, 63] = 10
    elif case == "label_-1":
        a = torch.zeros(1, 64, 64, dtype=torch.int64)
        a[0, 5, 7] = -1
    elif case == "label_nan":
        a[0, 0, 0, 0] = float("nan")
    elif case == "bool":
        a = torch.zeros(1, 64, 64, dtype=torch.bool)
    before = tr.gen_opt.flat_p.clone()
    with pytest.raises(ValueError, match="semantic_gt"):
        tr.gen_update(x, x, hp, synth=True, semantic_gt_a=a, semantic_gt_b=b)
    assert torch.equal(tr.gen_opt.flat_p, before)


@pytest.mark.parametrize("shape,dtype", [((1, 1, 64, 64), torch.float32), ((1, 64, 64), torch.int64),
                                         ((1, 64, 64), torch.uint8), ((1, 1, 64, 64), torch.float64)])
def test_gen_update_on_the_host_raises_not_implemented_before_any_work(tmp_path, model, shape, dtype):
    """Valid ground truth (labels 0..9, 9.75 truncating to 9 for the float types) on a trainer that was never moved to a
    device: NotImplementedError naming semantic_gt_a / semantic_gt_b, with no gradient zeroed and no weight touched."""
    tr, hp = _semantic_trainer(tmp_path, model, recon_synth_w=1)
    x = torch.zeros(1, 3, 64, 64)
    gt = (torch.arange(64 * 64).view(shape) % 10).to(dtype)
    if dtype.is_floating_point:
        gt = gt + 0.75
    tr.gen_opt.flat_g.fill_(2.0)
    with pytest.raises(NotImplementedError, match="semantic_gt_a / semantic_gt_b run on the device only"):
        tr.gen_update(x, x, hp, synth=True, semantic_gt_a=gt, semantic_gt_b=gt)
    assert bool((tr.gen_opt.flat_g == 2.0).all())


def test_ground_truth_is_truncated_before_the_float32_conversion():
    from munit_amd.trainer import MUNIT_Trainer
    g = torch.full((1, 2, 2), 9.9999999999, dtype=torch.float64)
    out = MUNIT_Trainer._gt_to_device([g, torch.full((1, 2, 2), 3, dtype=torch.int16)], torch.device("cpu"))
    assert out.dtype == torch.float32 and tuple(out.shape) == (2, 2, 2)
    assert out[0].unique().tolist() == [9.0] and out[1].unique().tolist() == [3.0]
