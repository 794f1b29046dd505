"""GPU: the synthetic-pair generator step -- the pair reconstruction loss (recon_synth_w) and the semantic loss against
ground-truth label maps (semantic_gt_a / semantic_gt_b, the 19 logits merged into 10 classes) -- kernels, entry-point
contract and the training step against the fp64 oracle of tests/synth_oracle.py."""
import math

import pytest
import torch
import torch.nn.functional as F

from munit_amd import ops
from oracle import munit_oracle as O
from tests import semantic_oracle as S
from tests import synth_oracle as Y
from tests.conv_contract import Calls
from tests.parity import nerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOSS_GRID_CAP = 1024 * 256            # pointwise.hip: the loss reductions run at most 1024 blocks of 256 threads


def cl(t):
    return t.float().to(DEV).contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------------------------------------------------------
# pair loss
# ------------------------------------------------------------------------------------------------------------------
PAIR_SHAPES = [(2, 5, 7, 3), (1, 1, 1, 1), (2, 16, 16, 1), (2, 64, 64, 3), (2, 3, 5, 4), (1, 513, 512, 2)]


def _pair_case(shape, kind):
    b, h, w, c = shape
    x_a, x_b, x_ab, x_ba = (t.float().double() for t in Y.pair_inputs(b, (h, w), 100 * h + w + c, c=c))
    if kind == "all":
        x_b = x_a.clone()
    elif kind == "none":
        x_b = x_a + 0.5
    elif kind == "one_channel":                  # one pixel per image differs, in its last channel only
        x_b = x_a.clone()
        x_b[:, c - 1, h // 2, w // 2] += 0.25
    x_ab.view(-1)[::7] = x_b.reshape(-1)[::7]       # exact ties: gradient 0
    return x_a, x_b, x_ab, x_ba


@pytest.mark.parametrize("kind", ["box", "all", "none", "one_channel"])
@pytest.mark.parametrize("shape", PAIR_SHAPES, ids=lambda s: "b%d_%dx%d_c%d" % s)
def test_pair_loss_and_gradients(shape, kind):
    """ops.pair_l1 against the fp64 restatement of trainer.py:452-464: loss at 1e-5 relative, gradients at 5e-5 normalised
    max (the bounds of the existing L1 / head tests); without an aligned pixel the loss and both gradients are exactly 0;
    a second backward is bitwise the first."""
    b, h, w, c = shape
    if shape == PAIR_SHAPES[-1]:
        assert b * h * w > LOSS_GRID_CAP
    x_a, x_b, x_ab, x_ba = _pair_case(shape, kind)
    share = float(Y.alignment(x_a, x_b).mean())
    if kind == "box" and h * w > 1:
        assert 0.1 <= share <= 0.9
    if kind == "one_channel":
        assert share == 1.0 - 1.0 / (h * w)
    ab, ba = x_ab.clone().requires_grad_(True), x_ba.clone().requires_grad_(True)
    ref = Y.pair_loss(x_a, x_b, ab, ba)
    ref.backward()
    da, db = cl(x_a).requires_grad_(True), cl(x_b).requires_grad_(True)
    dab, dba = cl(x_ab).requires_grad_(True), cl(x_ba).requires_grad_(True)
    loss = ops.pair_l1(da, db, dab, dba)
    print("pair %s %s: aligned %.3f loss %.8g ref %.8g" % (shape, kind, share, loss.item(), ref.item()))
    (loss * 3.0).backward()
    assert da.grad is None and db.grad is None
    if share == 0.0:
        assert loss.item() == 0.0 and ref.item() == 0.0
        assert torch.count_nonzero(dab.grad) == 0 and torch.count_nonzero(dba.grad) == 0
    else:
        assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item()), (loss.item(), ref.item())
        assert nerr(dab.grad.cpu(), 3.0 * ab.grad) < 5e-5 and nerr(dba.grad.cpu(), 3.0 * ba.grad) < 5e-5
        # sign(0) = 0 at the exact ties, and nothing outside the aligned pixels
        assert torch.equal(dab.grad.cpu() == 0, ab.grad == 0) and torch.equal(dba.grad.cpu() == 0, ba.grad == 0)
    g1, g2 = dab.grad.clone(), dba.grad.clone()
    dab.grad = dba.grad = None
    (ops.pair_l1(da, db, dab, dba) * 3.0).backward()
    assert torch.equal(g1, dab.grad) and torch.equal(g2, dba.grad)


def test_pair_loss_records_its_two_sign_patterns_in_order():
    x_a, x_b, x_ab, x_ba = (cl(t) for t in _pair_case((2, 5, 7, 3), "box"))
    with ops.kinks(l1=True) as k:
        ops.pair_l1(x_a, x_b, x_ab, x_ba)
    rec = k.l1
    assert len(rec) == 2 and torch.equal(rec[0], x_ab > x_b) and torch.equal(rec[1], x_ba > x_a)


# ------------------------------------------------------------------------------------------------------------------
# ground-truth head
# ------------------------------------------------------------------------------------------------------------------
GT_HEAD_CASES = [(2, 4, 4, 8), (16, 32, 32, 8), (2, 3, 5, 8), (2, 4, 6, 1), (2, 6, 4, 2), (2, 5, 7, 4)]


def _gt_head_case(b, h, w, sc, kind, seed):
    g = torch.Generator().manual_seed(seed)
    z = (3 * torch.randn(b, 19, h, w, generator=g, dtype=torch.float64)).float().double()
    H, W = h * sc, w * sc
    gt = torch.randint(0, 10, (b, H, W), generator=g).double()
    gt[:, ::2] += 0.75                             # the loader's floats are truncated, not rounded
    mask = None
    if kind == "masked":
        mask = (torch.rand(b, 1, H, W, generator=g) < 0.4).double()
    elif kind == "all_masked":
        mask = torch.ones(b, 1, H, W, dtype=torch.float64)
    return z, gt, mask


def _gt_head_run(z, gt, mask, sc, norm):
    zd = cl(z).requires_grad_(True)
    gd = gt.float().to(DEV).contiguous()
    md = None if mask is None else mask.float().to(DEV).contiguous()
    loss = ops.seg_cross_entropy_gt(zd, gd, md, sc, norm=norm)
    loss.backward()
    g1 = zd.grad.clone()
    zd.grad = None
    ops.seg_cross_entropy_gt(zd, gd, md, sc, norm=norm).backward()
    assert torch.equal(g1, zd.grad), "a second backward differs"
    return loss, g1


@pytest.mark.parametrize("kind", ["plain", "masked", "all_masked"])
@pytest.mark.parametrize("case", GT_HEAD_CASES, ids=lambda c: "b%d_%dx%d_s%d" % c)
def test_gt_head_loss_and_dlogits(case, kind):
    """ops.seg_cross_entropy_gt against F.interpolate + tests/synth_oracle.ce_gt_loss in fp64, with
    test_head_loss_and_dlogits' bounds: loss 1e-5 relative, dlogits 5e-5 normalised max, a bitwise second backward."""
    b, h, w, sc = case
    z, gt, mask = _gt_head_case(b, h, w, sc, kind, 1000 * h + 10 * w + sc)
    zr = z.clone().requires_grad_(True)
    up = F.interpolate(zr, size=(h * sc, w * sc), mode="bilinear", align_corners=False)
    ref = Y.ce_gt_loss(up, gt, mask) * 2          # norm = half the pixels: the sum of two means
    ref.backward()
    loss, grad = _gt_head_run(z, gt, mask, sc, gt.numel() / 2)
    print("gt head %s %s: loss %.8g ref %.8g" % (case, kind, loss.item(), ref.item()))
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item()), (loss.item(), ref.item())
    if kind == "all_masked":
        assert abs(loss.item() - 2 * (math.log(10 + math.e) - 1)) < 1e-5
        assert torch.count_nonzero(grad) == 0
    else:
        assert nerr(grad.cpu(), zr.grad) < 5e-5, nerr(grad.cpu(), zr.grad)


def test_gt_head_map_of_class_zero_only():
    """Every label 0: the target logit is the constant 0, so the whole gradient comes through the softmax; it is not zero,
    it reaches every one of the 19 logits (class 0 has no member to receive anything else), and the members of a merged
    class receive the same up-sampled-resolution gradient -- checked through the fp64 reference."""
    b, h, w, sc = 2, 4, 4, 8
    z, _, _ = _gt_head_case(b, h, w, sc, "plain", 5)
    gt = torch.zeros(b, h * sc, w * sc, dtype=torch.float64)
    zr = z.clone().requires_grad_(True)
    ref = Y.ce_gt_loss(F.interpolate(zr, scale_factor=sc, mode="bilinear", align_corners=False), gt)
    ref.backward()
    loss, grad = _gt_head_run(z, gt, None, sc, gt.numel())
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    assert nerr(grad.cpu(), zr.grad) < 5e-5
    g = grad.cpu().double()
    assert bool((g.abs().amax((0, 2, 3)) > 0).all()) and bool((g > 0).all())    # softmax only: every entry positive
    for members in Y.MEMBERS:
        for k in members[1:]:
            assert torch.equal(g[:, k], g[:, members[0]])


@pytest.mark.parametrize("bad", [10.0, -1.0, float("nan"), float("inf"), 3.0e9])
def test_gt_head_label_out_of_range_gives_nan_loss_and_finite_gradient(bad):
    """The documented rule (include/munit_hip.h): a device label outside 0..9 is never an index; the loss is NaN, both calls
    return OK and dlogits stays finite."""
    b, h, w, sc = 2, 3, 5, 8
    for kind in ("plain", "masked"):
        z, gt, mask = _gt_head_case(b, h, w, sc, kind, 9)
        gt[1, 7, 11] = bad
        if mask is not None:
            mask[1, 0, 7, 11] = 0.0
        loss, grad = _gt_head_run(z, gt, mask, sc, gt.numel())
        torch.cuda.synchronize()
        assert math.isnan(loss.item())
        assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0


def test_gt_head_rejects_wrong_ground_truth_tensors():
    z = cl(torch.zeros(1, 19, 2, 2))
    with pytest.raises(RuntimeError, match="ground truth"):
        ops.seg_cross_entropy_gt(z, torch.zeros(1, 16, 16, device=DEV, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="ground truth"):
        ops.seg_cross_entropy_gt(z, torch.zeros(1, 8, 16, device=DEV))


# ------------------------------------------------------------------------------------------------------------------
# entry-point contract (tests/synth_contract.py)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix,C", [(1, 1), (5 * 7, 3), (LOSS_GRID_CAP + 1, 2), (64 * 64, 4)])
def test_contract_pair_l1(npix, C):
    from tests import synth_contract as K
    K.check_pair_l1(npix, C)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 5, 3), (1, 5, 2, 8), (8, 96, 96, 8)])
@pytest.mark.parametrize("masked", [False, True])
def test_contract_seg_gt_head(shape, masked):
    from tests import kernel_contract as KC
    from tests import synth_contract as K
    b, h, w, s = shape
    if (b, h) == (8, 96):
        assert b * h * s * w * s > KC.SEG_GRID_CAP
    K.check_seg_gt_head(b, h, w, s, masked)


# ------------------------------------------------------------------------------------------------------------------
# the training step
# ------------------------------------------------------------------------------------------------------------------
SIZE, BATCH = 64, 2
SEG_NAMES = ("munit_seg_", "munit_space_to_batch", "munit_maxpool", "munit_add_relu")
NEW_NAMES = ("munit_pair_l1_fwd", "munit_pair_l1_bwd", "munit_seg_ce_gt_fwd", "munit_seg_ce_gt_bwd")


def _ckpt(tmp_path, model):
    p = tmp_path / "seg.pth"
    torch.save({k: v.cpu() for k, v in model.state_dict().items()}, str(p))
    return str(p)


def _synth_batch():
    """An aligned pair (75 % of the pixels identical), one mask shared by both images and two label maps: the first as the
    reference passes it (host, float, (B, 1, H, W), not whole numbers), the second a device int64 (B, H, W)."""
    x_a, x_b, _, _ = Y.pair_inputs(BATCH, SIZE, 7, dtype=torch.float32)
    g = torch.Generator().manual_seed(8)
    m = (torch.rand(BATCH, 1, SIZE, SIZE, generator=g) > 0.5).float()
    gt_a = (Y.gt_maps(BATCH, SIZE, 9) + 0.5).unsqueeze(1).float()
    gt_b = Y.gt_maps(BATCH, SIZE, 10).long().to(DEV)
    return x_a, x_b, m, gt_a, gt_b


def _synth_parity(tmp_path, monkeypatch, full=0, gen_state=1, semantic_w=3):
    from munit_amd.trainer import MUNIT_Trainer
    from tests.parity import run_step_parity
    seg = S.make_model(0)
    x_a, x_b, m, gt_a, gt_b = _synth_batch()
    assert 0.1 <= float(Y.alignment(x_a, x_b).mean()) <= 0.9
    sink = []
    cls = Y.oracle_trainer_class(seg, lambda: sink, (gt_a.double(), gt_b.cpu().double()))
    monkeypatch.setattr(O, "OracleTrainer", cls)
    monkeypatch.setattr(O, "synthetic_batch", lambda batch, size, seed=7, dtype=torch.float32: (x_a, x_b, m, m.clone()))
    plain = MUNIT_Trainer.gen_update

    def gen_update(self, xa, xb, hp, mask_a=None, mask_b=None):
        return plain(self, xa, xb, hp, mask_a, mask_b, synth=True, semantic_gt_a=gt_a, semantic_gt_b=gt_b)

    monkeypatch.setattr(MUNIT_Trainer, "gen_update", gen_update)
    over = {"recon_synth_w": 1, "adaptation": {"full_adaptation": full}}
    if semantic_w:
        over.update(semantic_w=semantic_w, semantic_ckpt_path=_ckpt(tmp_path, seg))
    with ops.kinks(seg=sink), Calls(SEG_NAMES + NEW_NAMES) as calls:
        rep = run_step_parity(size=SIZE, batch=BATCH, gen_state=gen_state, iters=1, device=DEV, hp_overrides=over)
    print("synthetic step full=%d gen_state=%d semantic_w=%d: pair %.6f sem %.6f grad %.2e max %.2e L2"
          % (full, gen_state, semantic_w, rep["loss_gen_recon_synth"], rep.get("loss_sem_seg", 0.0), rep["grad_nerr"],
             rep["grad_l2"]))
    assert cls.audit_bad == 0                    # the logits pass's kinks
    assert rep["loss_gen_recon_synth"] > 0
    assert calls.count("munit_pair_l1_fwd") == 1 and calls.count("munit_pair_l1_bwd") == 1
    return rep, calls


@pytest.mark.parametrize("mode", ["masked", "full_adaptation", "gen_state0"])
def test_step_parity_of_the_synthetic_iteration(tmp_path, monkeypatch, mode):
    """dis_update + gen_update(synth=True, ground truth, one shared mask) with semantic_w: 3 and recon_synth_w: 1 against
    the fp64 OracleTrainer that adds both terms on its own translations, at 64^2 B=2, with tests/parity.run_step_parity's
    own bounds (every loss 1e-5 relative, every generator gradient 5e-5 with the kinks pinned, Adam moments, weight step).
    With a ground truth only the logits pass runs through the segmentation network: one forward, no label kernel."""
    kw = {"masked": {}, "full_adaptation": dict(full=1), "gen_state0": dict(gen_state=0)}[mode]
    rep, calls = _synth_parity(tmp_path, monkeypatch, **kw)
    assert rep["loss_sem_seg"] > 0
    assert rep["grad_nerr"] <= 5e-5 and rep["grad_l2"] <= 5e-5, rep
    assert calls.count("munit_seg_ce_gt_fwd") == 1 and calls.count("munit_seg_ce_gt_bwd") == 1
    assert calls.count("munit_seg_input_fwd") == 2       # x_ab and x_ba, once: the label pass over x_a / x_b is skipped
    assert not any(n in calls for n in ("munit_seg_labels", "munit_seg_ce_fwd", "munit_seg_ce_bwd"))


def test_step_parity_with_the_pair_term_only(tmp_path, monkeypatch):
    """semantic_w: 0: the ground truth is ignored, as in the reference, and no kernel of the segmentation path launches."""
    rep, calls = _synth_parity(tmp_path, monkeypatch, semantic_w=0)
    assert rep["grad_nerr"] <= 5e-5 and rep["grad_l2"] <= 5e-5, rep
    assert sorted(calls) == ["munit_pair_l1_bwd", "munit_pair_l1_fwd"]


def _trainer(hp, seed):
    from munit_amd.trainer import MUNIT_Trainer
    torch.manual_seed(seed)
    return MUNIT_Trainer(hp).to(DEV)


def _hp(ckpt):
    hp = O.default_hp(SIZE, BATCH, 1)
    hp["semantic_w"] = 3
    hp["semantic_ckpt_path"] = ckpt
    hp["recon_synth_w"] = 1
    return hp


def test_multi_stream_synthetic_step_is_bitwise_the_single_stream_step(tmp_path):
    """Both terms wait for the two branch streams and feed both decoders on the way back: the three-stream schedule must
    not change a bit of the step (tests/test_gpu_semantic.py's test of that name, with the synthetic iteration)."""
    from munit_amd import trainer as T
    hp = _hp(_ckpt(tmp_path, S.make_model(0)))
    x_a, x_b, m, gt_a, gt_b = _synth_batch()
    x_a, x_b, m = x_a.to(DEV), x_b.to(DEV), m.to(DEV)

    def run(streams):
        saved = (ops.SIDE_STREAM_WGRAD, T.BRANCH_STREAMS)
        ops.SIDE_STREAM_WGRAD = T.BRANCH_STREAMS = streams
        try:
            tr = _trainer(hp, 0)
            torch.manual_seed(3)
            for it in range(2):
                tr.iterations = it
                tr.update_learning_rate()
                tr.dis_update(x_a, x_b, hp)
                tr.gen_update(x_a, x_b, hp, m, m, synth=True, semantic_gt_a=gt_a, semantic_gt_b=gt_b)
            torch.cuda.synchronize()
            return (tr.loss_sem_seg.item(), tr.loss_gen_recon_synth.item(), tr.loss_gen_total.item(),
                    tr.gen_opt.flat_g.clone(), tr.gen_opt.flat_p.clone(), tr.dis_opt.flat_p.clone())
        finally:
            ops.SIDE_STREAM_WGRAD, T.BRANCH_STREAMS = saved

    ref = run(False)
    assert ref[0] > 0 and ref[1] > 0
    for _ in range(2):
        got = run(True)
        assert got[:3] == ref[:3]
        assert all(torch.equal(a, b) for a, b in zip(ref[3:], got[3:]))


def test_synth_false_launches_neither_new_kernel(tmp_path):
    """synth=False with recon_synth_w: 1 and no ground truth: the ordinary iteration.  loss_gen_recon_synth stays the
    int 0, the semantic term runs on pseudo-labels, and none of the four new entry points is called; synth=True with
    recon_synth_w: 0 launches no pair kernel either."""
    hp = _hp(_ckpt(tmp_path, S.make_model(0)))
    x_a, x_b, m, gt_a, gt_b = _synth_batch()
    x_a, x_b, m = x_a.to(DEV), x_b.to(DEV), m.to(DEV)
    tr = _trainer(hp, 0)
    logged = {}

    class Exp(object):
        def log_metric(self, k, v):
            logged[k] = v

    with Calls(NEW_NAMES + ("munit_seg_labels", "munit_seg_ce_fwd")) as calls:
        tr.dis_update(x_a, x_b, hp)
        tr.gen_update(x_a, x_b, hp, m, m, Exp())
        torch.cuda.synchronize()
        assert tr.loss_gen_recon_synth == 0 and not torch.is_tensor(tr.loss_gen_recon_synth)
        assert sorted(calls) == ["munit_seg_ce_fwd", "munit_seg_labels"]
        assert "loss_gen_recon_synth" not in logged and "loss_sem_seg" in logged
        del calls[:]
        hp0 = dict(hp, recon_synth_w=0)
        tr.gen_update(x_a, x_b, hp0, m, m, Exp(), True)
        torch.cuda.synchronize()
        assert tr.loss_gen_recon_synth == 0 and logged["loss_gen_recon_synth"] == 0
        assert not any(n.startswith("munit_pair") for n in calls)
        del calls[:]
        tr.gen_update(x_a, x_b, hp, m, m, Exp(), True, gt_a, gt_b)
        torch.cuda.synchronize()
        assert float(logged["loss_gen_recon_synth"]) > 0 and float(tr.loss_gen_recon_synth.detach()) > 0
        total = float(tr.loss_gen_total)
        assert math.isfinite(total) and sorted(calls) == sorted(NEW_NAMES)
