"""Host-side checks of the trainable segmentation head (adaptation.sem_seg_lambda): the fp64 oracle against the reference's
fixture, the module's state_dict layout and loader, the trainer's construction and refusals, the C ABI, the loop's call and
the rule that every convolution form the head dispatches to is run by an op case of tests/test_gpu_seghead.py."""
import json
import math
import os
import re
import sys

import pytest
import torch

from oracle import munit_oracle as O
from tests import seghead_oracle as H
from tests import semantic_oracle as S
from tests.golden.make_golden_seghead import BATCH, CODE, LAMB, SIZE, inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
NEW = ("munit_avgpool7_fwd", "munit_avgpool7_bwd", "munit_seg_ce_direct_workspace_bytes", "munit_seg_ce_direct_fwd",
       "munit_seg_ce_direct_bwd")


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "golden_seghead.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    p = tmp_path_factory.mktemp("seghead") / "seg.pth"
    torch.save(S.make_model(0).state_dict(), str(p))
    return str(p)


def _check_digest(got, ref, rel=1e-9):
    t = got.detach().double().reshape(-1)
    assert t.numel() == ref["numel"]
    for key, val, bound in (("sum", float(t.sum()), ref["abs"]), ("abs", float(t.abs().sum()), ref["abs"]),
                            ("sq", float((t * t).sum()), ref["sq"])):
        assert abs(val - ref[key]) <= rel * bound, key
    assert (t[torch.tensor(ref["idx"])] - torch.tensor(ref["val"], dtype=torch.float64)).abs().max().item() \
        <= rel * t.abs().max().item()


def _hp(size=64, ckpt=None, **adaptation):
    hp = O.default_hp(size, 2, 1)
    hp["gen"]["n_res"] = 1
    hp["dis"]["num_scales"] = 1
    hp["adaptation"].update(adaptation)
    if ckpt is not None:
        hp["semantic_ckpt_path"] = ckpt
    return hp


def test_oracle_reproduces_the_reference_fixture(fixture):
    """tests/seghead_oracle.py against the reference's own layer4 / avgpool / Conv2d Sequential in fp64: both outputs, the
    weighted loss, every weight gradient and the running statistics after the two forwards."""
    fx = fixture
    assert (fx["code"], fx["batch"], fx["size"], fx["lamb"]) == (CODE, BATCH, SIZE, LAMB)
    assert fx["modules"] == ["Sequential", "AvgPool2d", "Conv2d"]
    sd = H.make_state(0)
    assert abs(sum(float((v.double() ** 2).sum()) for v in sd.values() if v.is_floating_point()) - fx["weights_sq"]) \
        <= 1e-12 * fx["weights_sq"]
    ps = H.params(sd)
    for p in ps:
        p.requires_grad_(True)
    c_a, c_b, t_a, t_b = inputs()
    loss, o_a, o_b = H.head_loss(sd, c_a, c_b, t_a, t_b, SIZE)
    _check_digest(o_a, fx["output_a"])
    _check_digest(o_b, fx["output_b"])
    loss = loss * LAMB
    assert abs(float(loss.detach()) - fx["loss"]) <= 1e-9 * abs(fx["loss"])
    grads = torch.autograd.grad(loss, ps)
    assert sorted(fx["grads"]) == sorted(H.param_names())
    for k, g in zip(H.param_names(), grads):
        _check_digest(g, fx["grads"][k])
    assert len(fx["running"]) == 14
    for k, ref in fx["running"].items():
        _check_digest(sd[k], ref)
    assert int(sd["0.0.bn1.num_batches_tracked"]) == int(sd["0.2.bn2.num_batches_tracked"]) == fx["tracked"] == 2


def test_oracle_update_is_two_forwards_and_an_adam_step():
    hp = _hp()
    sd = H.make_state(0)
    before = {k: v.clone() for k, v in sd.items()}
    opt = H.HeadOptimizer(sd, hp)
    c_a, c_b, t_a, t_b = inputs()
    loss, grads = H.head_update(sd, opt, c_a, c_b, t_a, t_b, LAMB, SIZE)
    assert opt.step_count == 1 and float(loss) > 0
    for k, g in zip(H.param_names(), grads):
        step = (sd[k].detach() - before[k]).abs().max().item()
        assert 0 < step <= 1.001 * hp["lr"] + hp["lr"] * hp["weight_decay"] * before[k].abs().max().item(), k   # Adam's first step
        assert float(g.abs().max()) > 0, k
    assert int(sd["0.1.bn1.num_batches_tracked"]) == 2
    # the second forward sees the statistics the first one moved, and the pool counts its padding
    x = torch.ones(1, 4, 3, 3, dtype=torch.float64)
    assert torch.allclose(torch.nn.functional.avg_pool2d(x, 7, 1, 3), torch.full_like(x, 9 / 49))


def test_module_state_dict_is_the_reference_s(fixture, ckpt):
    from munit_amd.segmentation import SegmentationHead, load_segmentation_head
    net = SegmentationHead()
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert got == fixture["keys"]
    assert got == [[k, list(s)] for k, s in H.shapes().items()]
    assert net.state_dict()["0.0.bn1.num_batches_tracked"].dtype == torch.long
    torch.manual_seed(3)
    head = load_segmentation_head(ckpt)
    src = S.make_model(0).state_dict()
    for k, v in head.state_dict().items():
        if k.startswith("0."):
            assert torch.equal(v, src["resnet34_8s.layer4." + k[2:]]), k
    assert head.training and all(p.requires_grad for p in head.parameters())
    assert all(m.training for m in head.modules())
    # nn.Conv2d(512, 10, 1)'s distribution: uniform in +-1/sqrt(fan_in) for the weight and the bias
    bound = 1.0 / math.sqrt(512)
    w, b = head[2].weight.detach(), head[2].bias.detach()
    assert tuple(w.shape) == (10, 512, 1, 1) and tuple(b.shape) == (10,)
    assert float(w.abs().max()) <= bound and float(b.abs().max()) <= bound
    assert float(w.abs().max()) > 0.95 * bound and abs(float(w.std()) - bound / math.sqrt(3)) < 0.05 * bound
    torch.manual_seed(4)
    assert not torch.equal(load_segmentation_head(ckpt)[2].weight, w)          # a fresh draw every time
    # a checkpoint with a missing key is refused, as load_segmentation_model refuses it
    bad = {k: v for k, v in src.items() if k != "resnet34_8s.layer4.1.bn2.running_var"}
    p = os.path.join(os.path.dirname(ckpt), "bad.pth")
    torch.save(bad, p)
    with pytest.raises(RuntimeError, match="layer4.1.bn2.running_var"):
        load_segmentation_head(p)
    for shape in ((1, 256, 6, 8), (1, 256, 8, 10), (1, 128, 8, 8)):
        with pytest.raises(ValueError):
            head(torch.zeros(shape))                                           # refused before any device work


def test_trainer_builds_the_head_under_its_own_optimizer(ckpt):
    from munit_amd.trainer import MUNIT_Trainer
    torch.manual_seed(0)
    tr = MUNIT_Trainer(_hp(ckpt=ckpt, sem_seg_lambda=1))
    assert tr.train_seg and tr.training and tr.segmentation_head.training
    mine = [id(p) for p in tr.segmentation_head.parameters()]
    assert len(mine) == len(H.param_names())
    assert [id(p) for p in tr.segmentation_opt._plist] == mine
    assert type(tr.segmentation_opt).__name__ == "FusedAdam" and tr.segmentation_opt.flat_p is not None
    for opt in (tr.gen_opt, tr.dis_opt):
        assert not set(mine) & {id(p) for p in opt._plist}
    for p in tr.segmentation_head.parameters():
        assert p._munit_opt is tr.segmentation_opt and p._munit_grad is not None
    # created after the trainer's weight initialisation: the checkpoint's weights are kept
    src = S.make_model(0).state_dict()
    assert torch.equal(tr.segmentation_head[0][2].conv2.weight, src["resnet34_8s.layer4.2.conv2.weight"])
    assert torch.equal(tr.segmentation_head[0][0].bn1.weight, src["resnet34_8s.layer4.0.bn1.weight"])
    # the scheduler exists and update_learning_rate does not step it
    lr0 = tr.segmentation_opt.param_groups[0]["lr"]
    last = tr.scheduler_seg.last_epoch
    for _ in range(3):
        tr.update_learning_rate()
    assert tr.scheduler_seg.last_epoch == last and tr.segmentation_opt.param_groups[0]["lr"] == lr0
    for name in ("segmentation_opt_step", "segmentation_head_update"):
        assert callable(getattr(MUNIT_Trainer, name))
    import inspect
    assert list(inspect.signature(MUNIT_Trainer.segmentation_head_update).parameters) == \
        ["self", "x_a", "x_b", "target_a", "target_b", "lamb", "comet_exp"]
    off = MUNIT_Trainer(_hp())
    assert not off.train_seg
    for name in ("segmentation_head", "segmentation_opt", "scheduler_seg"):
        assert not hasattr(off, name)
    with pytest.raises(ValueError, match="sem_seg_lambda"):
        off.segmentation_head_update(torch.zeros(2, 3, 64, 64), torch.zeros(2, 3, 64, 64), torch.zeros(2, 1, 64, 64),
                                     torch.zeros(2, 1, 64, 64), 1.0)


def test_save_and_resume_do_not_carry_the_head(tmp_path, ckpt):
    from munit_amd.trainer import MUNIT_Trainer
    names = []
    for sub, hp in (("off", _hp()), ("on", _hp(ckpt=ckpt, sem_seg_lambda=1))):
        d = tmp_path / sub
        d.mkdir()
        torch.manual_seed(0)
        MUNIT_Trainer(hp).save(str(d), 2)
        names.append(sorted(os.listdir(str(d))))
    assert names[0] == names[1] == ["dis_00000003.pt", "gen_00000003.pt", "optimizer.pt"]
    assert sorted(torch.load(str(tmp_path / "on" / "optimizer.pt"), weights_only=True)) == ["dis", "gen"]


def test_refusals_come_before_any_device_work(monkeypatch, ckpt):
    from munit_amd import trainer as T
    # without a checkpoint the weight stays refused, by name
    with pytest.raises(NotImplementedError, match="adaptation.sem_seg_lambda"):
        T.MUNIT_Trainer(_hp(sem_seg_lambda=1))
    for k in ("domain_adv_w", "vgg_w"):
        hp = _hp(ckpt=ckpt, sem_seg_lambda=1)
        hp[k] = 1
        with pytest.raises(NotImplementedError, match=k + r"(.|\n)*cannot run in the reference"):
            T.MUNIT_Trainer(hp)
    for prec in ("bf16", "bf16s"):
        hp = _hp(ckpt=ckpt, sem_seg_lambda=1)
        hp["precision"] = prec
        with pytest.raises(NotImplementedError, match="sem_seg_lambda.*fp32"):
            T.MUNIT_Trainer(hp)
    hp = _hp(ckpt=ckpt, sem_seg_lambda=1)
    hp["optimizer"] = "extraadam"
    with pytest.raises(NotImplementedError, match="sem_seg_lambda.*extrapolation"):
        T.MUNIT_Trainer(hp)
    for dp in (0, 1):
        monkeypatch.setattr(T, "dp_size", lambda: 2)
        with pytest.raises(NotImplementedError, match="sem_seg_lambda.*data-parallel.*later change"):
            T.MUNIT_Trainer(_hp(ckpt=ckpt, sem_seg_lambda=1, data_parallel=dp))
        monkeypatch.undo()
    hp = _hp(ckpt=ckpt, sem_seg_lambda=1)
    hp["crop_image_width"] = 96
    with pytest.raises(ValueError, match="sem_seg_lambda.*square"):
        T.MUNIT_Trainer(hp)
    for size in (72, 40):                       # codes of 18x18 and 10x10: not multiples of 4
        with pytest.raises(ValueError, match="sem_seg_lambda.*multiples of 4"):
            T.MUNIT_Trainer(_hp(size, ckpt=ckpt, sem_seg_lambda=1))
    hp = _hp(256, ckpt=ckpt, sem_seg_lambda=1)
    hp["gen"]["n_downsample"] = 4
    with pytest.raises(ValueError, match="sem_seg_lambda.*n_downsample"):
        T.MUNIT_Trainer(hp)
    # the update's own argument checks: nothing of the head's gradient buffer is touched
    tr = T.MUNIT_Trainer(_hp(ckpt=ckpt, sem_seg_lambda=1))
    tr.segmentation_opt.flat_g.fill_(3.0)
    x, t = torch.zeros(2, 3, 64, 64), torch.zeros(2, 1, 64, 64)
    for bad, pat in ((torch.zeros(2, 1, 32, 32), "target_a"), (torch.zeros(2, 2, 64, 64), "target_a"),
                     (torch.zeros(2, 1, 64, 64, dtype=torch.bool), "real dtype"), (None, "both label maps"),
                     (torch.full((2, 1, 64, 64), 10.0), "outside 0..9"), ("labels", "tensor")):
        with pytest.raises(ValueError, match=pat):
            tr.segmentation_head_update(x, x, bad, t, 1.0)
    with pytest.raises(ValueError, match="crop size"):
        tr.segmentation_head_update(torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 32, 32), t, t, 1.0)
    monkeypatch.setattr(T, "dp_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="sem_seg_lambda"):
        tr.segmentation_head_update(x, x, t, t, 1.0)
    assert bool((tr.segmentation_opt.flat_g == 3.0).all()) and tr.segmentation_opt._step == 0


def test_new_symbols_are_declared_listed_and_exported():
    from munit_amd import _lib
    header = open(os.path.join(ROOT, "include", "munit_hip.h")).read()
    declared = set(re.findall(r"\b(munit_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # host-side argument checks run before any launch (no device needed): negative return + munit_last_error
    assert lib.munit_seg_ce_direct_workspace_bytes(2, 16, 16, 4, 10) >= 2 * 64 * 64 * 10 * 4
    assert lib.munit_avgpool7_fwd(8, 16, 1, 4, 4, 6, None) == -1 and b"C % 4" in lib.munit_last_error()
    assert lib.munit_avgpool7_fwd(8, 8, 1, 4, 4, 8, None) == -1             # in place
    assert lib.munit_avgpool7_bwd(None, 16, 1, 4, 4, 8, None) == -1 and b"avgpool7_bwd" in lib.munit_last_error()
    assert lib.munit_avgpool7_bwd(8, 16, 1, 0, 4, 8, None) == -1
    for k in (1, 33):
        assert lib.munit_seg_ce_direct_fwd(8, 8, 1, 2, 2, 4, k, 1.0, 8, 8, 1 << 20, None) == -1
        assert b"2..32 classes" in lib.munit_last_error()
    for s in (0, 3, 16):
        assert lib.munit_seg_ce_direct_bwd(8, 8, 1, 2, 2, s, 10, 1.0, 8, 8, 8, 1 << 20, None) == -1
        assert b"scale" in lib.munit_last_error()
    assert lib.munit_seg_ce_direct_fwd(8, 8, 1, 2, 2, 4, 10, 0.0, 8, 8, 1 << 20, None) == -1
    assert lib.munit_seg_ce_direct_fwd(8, 8, 1, 2, 2, 4, 10, 1.0, 8, 8, 3, None) == -2            # workspace
    assert lib.munit_seg_ce_direct_bwd(8, 8, 1, 2, 2, 4, 10, 1.0, 8, 8, 8, 64 * 10 * 4 - 1, None) == -2
    assert lib.munit_seg_ce_direct_fwd(8, 8, 4096, 4096, 4096, 8, 10, 1.0, 8, 8, 1 << 20, None) == -1
    from munit_amd import ops
    for name in ("avgpool7", "seg_cross_entropy_direct"):
        assert callable(getattr(ops, name))


# ---- the loop ------------------------------------------------------------------------------------------------------------------
class _Stub(object):
    def __init__(self, cfg, train_seg):
        self.use_classifier_sr = self.use_output_classifier_sr = False
        if train_seg is not None:
            self.train_seg = train_seg
        self.calls, self.iterations, self.cfg = [], None, cfg

    def update_learning_rate(self):
        self.calls.append(("lr",))

    def dis_update(self, x_a, x_b, hp, comet_exp=None):
        self.calls.append(("dis_update", x_a))

    def gen_update(self, x_a, x_b, hp, mask_a=None, mask_b=None, comet_exp=None, synth=False, semantic_gt_a=None,
                   semantic_gt_b=None):
        self.calls.append(("gen_update", x_a, synth, semantic_gt_a))

    def segmentation_head_update(self, x_a, x_b, target_a, target_b, lamb, comet_exp=None):
        assert comet_exp is None
        self.calls.append(("segmentation_head_update", x_a, x_b, target_a, target_b, lamb))


def test_run_iteration_calls_the_update_where_the_reference_does():
    """scripts/train.py:275-283: inside `synthetic_frequency > 0`, in every iteration, after the synthetic steps, on the
    iteration's synthetic pair and its label maps, with adaptation.sem_seg_lambda."""
    from train_loop import run_iteration
    cfg = _hp(sem_seg_lambda=0.7)
    cfg["synthetic_frequency"], cfg["synthetic_seg_gt"], cfg["ratio_disc_gen"] = 2, 0, 1
    real = tuple(torch.zeros(1) for _ in range(4))
    drawn = []

    def pairs():
        while True:
            drawn.append(tuple(torch.zeros(1) for _ in range(5)))
            yield drawn[-1]

    stub, it_pairs = _Stub(cfg, True), pairs()
    for it in range(3):
        n = len(stub.calls)
        run_iteration(stub, cfg, it, real, it_pairs)
        got = stub.calls[n:]
        s = drawn[-1]
        assert len(drawn) == it + 1                               # one synthetic pair per iteration
        want_head = ("segmentation_head_update", s[0], s[1], s[3], s[4], 0.7)
        assert [c[0] for c in got] == (["lr", "dis_update", "gen_update", "dis_update", "gen_update", "segmentation_head_update"]
                                       if it % 2 == 0 else ["lr", "dis_update", "gen_update", "segmentation_head_update"])
        assert len(got[-1]) == len(want_head) and all(a is b or a == b for a, b in zip(got[-1], want_head))
        if it % 2 == 0:                                            # the pair the synthetic steps used; synthetic_seg_gt: 0
            assert got[3][1] is s[0] and got[4][1] is s[0] and got[4][2] is True and got[4][3] is None
    # not under synthetic_frequency 0, not without pairs, not without the flag (a stub that has no such attribute included)
    off = dict(cfg, synthetic_frequency=0)
    for stub, c, p in ((_Stub(off, True), off, pairs()), (_Stub(cfg, True), cfg, None), (_Stub(cfg, False), cfg, pairs()),
                       (_Stub(cfg, None), cfg, pairs())):
        run_iteration(stub, c, 0, real, p)
        assert "segmentation_head_update" not in [x[0] for x in stub.calls]


# ---- dispatch: every convolution form the head reaches is run by an op case ----------------------------------------------------
HEAD_CROPS, HEAD_BATCHES = (64, 80, 256), (1, 2, 8)


def head_convs(crop, b, n_downsample=2):
    """(name, op case, passes) of the head's seven convolutions and its scoring layer at `crop`, batch `b`: the 3x3 layers
    and the shortcut on the 16 b phase images of the (crop / 4)^2 code, the scoring layer on the plain layout.  Block 0's
    conv1 and downsample read a code without a tape: no backward-data."""
    c = crop >> n_downsample
    p, n = c // 4, 16 * b
    out = [("0.0.conv1", (256, 512, 3, 1, 1, "zero", 0, "none", n, p, p), (0, 2)),
           ("0.0.conv2", (512, 512, 3, 1, 1, "zero", 0, "none", n, p, p), (0, 1, 2)),
           ("0.0.downsample.0", (256, 512, 1, 1, 0, "zero", 0, "none", n, p, p), (0, 2))]
    for i in (1, 2):
        for j in (1, 2):
            out.append(("0.%d.conv%d" % (i, j), (512, 512, 3, 1, 1, "zero", 0, "none", n, p, p), (0, 1, 2)))
    out.append(("2", (512, 10, 1, 1, 0, "zero", 0, "none", b, c, c), (0, 1, 2)))
    return out


def _key(lib, case, which):
    from tests.test_cpu_dispatch import kernel_names
    return (which, kernel_names(lib, case)[which]) + case[:4]


def test_every_head_conv_form_is_covered_by_an_op_case():
    from munit_amd import _lib
    from tests.test_gpu_seghead import HEAD_CONV_CASES, head_op_case
    lib = _lib.load()
    names = [n for n, _, _ in head_convs(64, 1)]
    assert len(names) == 8 and sorted(names[:7] + ["2"]) == sorted(
        k[:-len(".weight")] for k, s in H.shapes().items() if len(s) == 4)
    prod = {}
    for crop in HEAD_CROPS:
        for b in HEAD_BATCHES:
            for name, case, passes in head_convs(crop, b):
                for p in passes:
                    prod.setdefault(_key(lib, case, p), "%s, crop %d, batch %d" % (name, crop, b))
    assert len(prod) >= 12, sorted(prod)
    assert any("wino" in k[1] for k in prod) and any("LDS-patch" in k[1] for k in prod)      # even and odd phase images differ
    covered = {_key(lib, head_op_case(c), p) for c in HEAD_CONV_CASES for p in (0, 1, 2)}
    missing = {k: v for k, v in prod.items() if k not in covered}
    assert not missing, "\n".join("  %s: %s" % kv for kv in sorted(missing.items()))
    assert len(set(HEAD_CONV_CASES)) == len(HEAD_CONV_CASES)
