"""GPU: the semantic-consistency loss (semantic_w > 0) -- the seg kernels, the frozen Resnet34_8s and the training step --
against the fp64 oracle of tests/semantic_oracle.py."""
import pytest
import torch
import torch.nn.functional as F

from munit_amd import ops
from oracle import munit_oracle as O
from tests import semantic_oracle as S
from tests.parity import nerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def cl(t):
    return t.float().to(DEV).contiguous(memory_format=torch.channels_last)


def l2err(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return ((a - ref).norm() / ref.norm().clamp_min(1e-300)).item()


@pytest.fixture(scope="module")
def model():
    return S.make_model(0).to(DEV)


@pytest.fixture(scope="module")
def sd(model):
    return S.state(model)


@pytest.mark.parametrize("n,c,h,w", [(2, 8, 4, 6), (16, 128, 32, 32), (64, 19, 8, 8)])
def test_space_to_batch_round_trip(n, c, h, w):
    x = torch.randn(n, c, h, w, dtype=torch.float64)
    y = ops.space_to_batch_raw(cl(x), 2)
    ref = x.view(n, c, h // 2, 2, w // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(n * 4, c, h // 2, w // 2)
    assert torch.equal(y.cpu().double(), ref.float().double())
    y_before = y.clone()
    back = ops.space_to_batch_raw(y, 2, inverse=True)
    assert torch.equal(y, y_before)
    assert torch.equal(back.cpu().double(), x.float().double())


@pytest.mark.parametrize("b,c,h,w", [(2, 4, 7, 9), (2, 64, 16, 16), (8, 64, 128, 128)])
def test_maxpool_first_max_rule(b, c, h, w):
    g = torch.Generator().manual_seed(b * h)
    x = torch.randint(0, 3, (b, c, h, w), generator=g).double()     # many ties
    xr = x.clone().requires_grad_(True)
    yr, idx = F.max_pool2d(xr, 3, 2, 1, return_indices=True)
    dy = torch.randn(yr.shape, generator=g, dtype=torch.float64)
    yr.backward(dy)
    xd = cl(x).requires_grad_(True)
    ops.SEG_SINK = []
    try:
        y = ops.maxpool3s2(xd)
        win = ops.SEG_SINK[0].cpu().long()            # (b, ho, wo, c): window position kh*3 + kw
    finally:
        ops.SEG_SINK = None
    assert torch.equal(y.cpu().double(), yr.detach())
    # the rule, restated: first maximal element of the window in kh-major order (torch's CPU kernel agrees)
    ho, wo = y.shape[2:]
    kh, kw = win // 3, win % 3
    row = 2 * torch.arange(ho).view(1, ho, 1, 1) - 1 + kh
    col = 2 * torch.arange(wo).view(1, 1, wo, 1) - 1 + kw
    assert torch.equal((row * w + col).permute(0, 3, 1, 2), idx)
    y.backward(cl(dy))
    assert nerr(xd.grad.cpu(), xr.grad) < 1e-6


@pytest.mark.parametrize("cin,cout,k,pad,b,h", [(3, 64, 7, 3, 2, 16), (64, 128, 3, 1, 2, 16), (64, 128, 1, 0, 2, 16),
                                               (3, 64, 7, 3, 2, 256), (64, 128, 3, 1, 2, 64)])
def test_odd_kernel_stride2_dgrad(cin, cout, k, pad, b, h):
    from munit_amd.segmentation import _even
    g = torch.Generator().manual_seed(k * h)
    w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) / (cin * k * k) ** 0.5
    x = torch.randn(b, cin, h, h, generator=g, dtype=torch.float64).requires_grad_(True)
    y = F.conv2d(x, w, None, 2, pad)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    xd = cl(x.detach()).requires_grad_(True)
    yd = ops.frozen_conv(xd, cl(w), None, cl(_even(w)), 2, pad)
    assert nerr(yd.cpu(), y.detach()) < 2e-5
    yd.backward(cl(dy))
    assert nerr(xd.grad.cpu(), x.grad) < 2e-5


def _head_case(b, h, scale, kind, seed):
    g = torch.Generator().manual_seed(seed)
    z = 3 * torch.randn(b, 19, h, h, generator=g, dtype=torch.float64)
    H = h * scale
    labels = torch.randint(0, 19, (b, H, H), generator=g)
    mask = None
    if kind == "masked":
        mask = (torch.rand(b, 1, H, H, generator=g) < 0.4).double()
    elif kind == "all_masked":
        mask = torch.ones(b, 1, H, H, dtype=torch.float64)
    return z, labels, mask


@pytest.mark.parametrize("b,h", [(2, 4), (16, 32)])
@pytest.mark.parametrize("kind", ["plain", "masked", "all_masked"])
def test_head_loss_and_dlogits(b, h, kind):
    z, labels, mask = _head_case(b, h, 8, kind, b * h)
    zr = z.clone().requires_grad_(True)
    up = F.interpolate(zr, scale_factor=8, mode="bilinear", align_corners=False)
    ref = S.ce_loss(up, labels, mask) * 2        # norm = half the pixels: the sum of two means
    ref.backward()
    zd = cl(z).requires_grad_(True)
    md = None if mask is None else mask.float().to(DEV).contiguous()
    loss = ops.seg_cross_entropy(zd, labels.int().to(DEV).contiguous(), md, 8, norm=labels.numel() / 2)
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    if kind == "all_masked":
        assert abs(loss.item() - 2 * S.MASKED_PIXEL_LOSS) < 1e-5
    loss.backward()
    if kind == "all_masked":
        assert torch.count_nonzero(zd.grad) == 0
    else:
        assert nerr(zd.grad.cpu(), zr.grad) < 5e-5
    # deterministic: a second backward is bitwise the same
    g1 = zd.grad.clone()
    zd.grad = None
    ops.seg_cross_entropy(zd, labels.int().to(DEV).contiguous(), md, 8, norm=labels.numel() / 2).backward()
    assert torch.equal(g1, zd.grad)


@pytest.mark.parametrize("b,h", [(2, 4), (16, 32)])
def test_labels_first_max(b, h):
    z, _, _ = _head_case(b, h, 8, "plain", 7 + h)
    z[:, 5] = z[:, 3]                                   # exact ties between classes 3 and 5: 3 wins
    zd = cl(z)
    lab = ops.seg_labels(zd).cpu().long()
    up = F.interpolate(zd.cpu().double(), scale_factor=8, mode="bilinear", align_corners=False)
    ref = up.argmax(1)
    top = up.topk(2, 1).values
    tight = (top[:, 0] - top[:, 1]) < 1e-5
    assert torch.equal(lab[~tight], ref[~tight])
    assert (lab != 5).all()


@pytest.mark.parametrize("b,size", [(2, 64), (2, 256)])
def test_network_logits_and_input_grad(model, sd, b, size):
    x = S.rand_images(b, size, size)
    xd = cl(x).requires_grad_(True)
    ops.SEG_SINK = []
    try:
        z = model(xd)
        pins = S.seg_pins(ops.SEG_SINK)
    finally:
        ops.SEG_SINK = None
    # the oracle takes the device's branch at every ReLU and max-pool kink; the audit allows a disagreement with the
    # oracle's own choice only at rounding-noise margins
    xr = x.clone().requires_grad_(True)
    kinks = []
    zr = S.logits(sd, xr, up=False, kinks=kinks, pins=pins)
    assert S.audit(kinks, pins) == 0
    dz = torch.randn(zr.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    zr.backward(dz)
    assert z.shape == zr.shape
    assert nerr(z.cpu(), zr.detach()) < 5e-5 and l2err(z, zr.detach()) < 5e-5
    z.backward(cl(dz))
    assert nerr(xd.grad.cpu(), xr.grad) < 5e-5 and l2err(xd.grad, xr.grad) < 5e-5


def _ckpt(tmp_path, model):
    p = tmp_path / "seg.pth"
    torch.save({k: v.cpu() for k, v in model.state_dict().items()}, str(p))
    return str(p)


def _trainer(hp, seed):
    from munit_amd.trainer import MUNIT_Trainer
    torch.manual_seed(seed)
    return MUNIT_Trainer(hp).to(DEV)


def _hp(size, batch, ckpt, full_adaptation=0):
    hp = O.default_hp(size, batch, 1)
    hp["semantic_w"] = 3
    hp["semantic_ckpt_path"] = ckpt
    hp["adaptation"]["full_adaptation"] = full_adaptation
    return hp


def _inputs(b, size, seed):
    g = torch.Generator().manual_seed(seed)
    xa = (torch.rand(b, 3, size, size, generator=g) * 2 - 1).to(DEV)
    xb = (torch.rand(b, 3, size, size, generator=g) * 2 - 1).to(DEV)
    ma = (torch.rand(b, 1, size, size, generator=g) < 0.3).float().to(DEV)
    mb = (torch.rand(b, 1, size, size, generator=g) < 0.3).float().to(DEV)
    return xa, xb, ma, mb


def _step(tr, hp, xa, xb, ma, mb):
    torch.manual_seed(11)
    tr.dis_update(xa, xb, hp)
    tr.gen_update(xa, xb, hp, ma, mb)
    torch.cuda.synchronize()


def _semantic_parity(tmp_path, monkeypatch, size, batch, full, **kw):
    from tests.parity import run_step_parity
    seg = S.make_model(0)
    sink = []
    cls = S.oracle_trainer_class(seg, lambda: sink)
    monkeypatch.setattr(O, "OracleTrainer", cls)
    ops.SEG_SINK = sink
    try:
        rep = run_step_parity(size=size, batch=batch, gen_state=1, iters=1, device=DEV,
                              hp_overrides={"semantic_w": 3, "semantic_ckpt_path": _ckpt(tmp_path, seg),
                                            "adaptation": {"full_adaptation": full}}, **kw)
    finally:
        ops.SEG_SINK = None
    assert cls.audit_bad == 0
    assert "loss_sem_seg" in rep and rep["loss_sem_seg"] > 0
    return rep


@pytest.mark.parametrize("full", [0, 1])
def test_step_parity_with_semantic_loss(tmp_path, monkeypatch, full):
    """dis_update + gen_update with semantic_w: 3 against the fp64 OracleTrainer that adds the term through its own
    x_ab / x_ba (tests/parity.run_step_parity's bounds: every loss <= 1e-5 relative, every generator gradient <= 5e-5
    normalised max and relative L2 with the kinks pinned, median <= 1e-5, Adam moments and the weight step), at 64^2 B=2.
    The seg network's kinks and labels are pinned and audited as well."""
    rep = _semantic_parity(tmp_path, monkeypatch, 64, 2, full)
    assert rep["grad_nerr"] <= 5e-5 and rep["grad_l2"] <= 5e-5, rep


def test_step_parity_with_semantic_loss_256(tmp_path, monkeypatch):
    """The same step at 256^2 B=1.  Stated exception: here the fp32 evaluation of the reference
    itself does not meet 5e-5 / median 1e-5.  Every tensor on the x_ba path sits at ~2.8e-5 relative L2 for the oracle
    run in fp32 (torch CPU, direct convolutions, same pinned kinks and labels), median 1.05e-5.  So each generator
    gradient is held to max(5e-5, 3 x that yardstick) and the median to 3 x the yardstick's median.  Measured: HIP worst
    5.9e-5 max / 4.7e-5 L2, median 2.7e-5.  Every loss keeps 1e-5, and the kink audits, Adam moments and weight step keep
    run_step_parity's bounds."""
    from tests.parity import KINK_FRAC, KINK_NOISE
    rep = _semantic_parity(tmp_path, monkeypatch, 256, 1, 0, check=False, ref32=True)
    assert rep["loss_rel"] <= 1e-5, rep["loss_rel"]
    assert rep["kink_worst_rel"] <= KINK_NOISE and rep["kink_disagree_frac"] <= KINK_FRAC
    rows = rep["ref32"][0]
    assert len(rows) > 50
    for name, hip_max, hip_l2, r32_max, r32_l2 in rows:
        assert hip_max <= max(5e-5, 3 * r32_max) and hip_l2 <= max(5e-5, 3 * r32_l2), (name, hip_max, hip_l2, r32_max, r32_l2)
    med = lambda k: sorted(r[k] for r in rows)[len(rows) // 2]
    assert med(2) <= max(1e-5, 3 * med(4)), (med(2), med(4))
    # Adam moments are linear / quadratic in the gradients: twice the per-tensor bound, as run_step_parity holds them
    assert rep["moment_l2"] <= 2 * max(5e-5, 3 * max(r[4] for r in rows)), rep["moment_l2"]
    assert rep["weight_abs"] <= 4.0 * 1e-4 and rep["weight_l2"] <= 2e-4, rep


def test_two_identical_steps_bitwise_equal(tmp_path, model):
    ckpt = _ckpt(tmp_path, model)
    hp = _hp(64, 2, ckpt)
    xa, xb, ma, mb = _inputs(2, 64, 5)
    outs = []
    for _ in range(2):
        tr = _trainer(hp, 0)
        _step(tr, hp, xa, xb, ma, mb)
        outs.append((tr.loss_sem_seg.item(), tr.gen_opt.flat_g.clone(), tr.gen_opt.flat_p.clone()))
    assert outs[0][0] == outs[1][0]
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])


def test_sample_returns_label_maps(tmp_path, model, sd):
    ckpt = _ckpt(tmp_path, model)
    hp = _hp(64, 2, ckpt)
    tr = _trainer(hp, 0)
    xa, xb, _, _ = _inputs(2, 64, 9)
    out = tr.sample(xa, xb)
    assert len(out) == 12
    rgb_a, x_ab1, rgb_ab = out[2], out[3], out[4]
    assert rgb_a.shape == (2, 3, 64, 64) and rgb_ab.shape == (2, 3, 64, 64)
    for img, rgb in ((xa, rgb_a), (x_ab1, rgb_ab), (xb, out[8]), (out[9], out[10])):
        up = S.logits(sd, img.cpu().double())
        top = up.topk(2, 1).values
        sure = ((top[:, 0] - top[:, 1]) > 1e-4).unsqueeze(1).expand(-1, 3, -1, -1)
        ref = S.colorize(up.argmax(1))
        assert torch.equal(rgb.cpu().double()[sure], ref.float().double()[sure])


def test_semantic_off_launches_no_seg_kernel(tmp_path, model):
    hp = O.default_hp(64, 2, 1)
    tr = _trainer(hp, 0)
    assert tr.segmentation_model is None
    xa, xb, ma, mb = _inputs(2, 64, 3)
    ops.SEG_SINK = []
    calls = []
    from munit_amd import _lib
    lib = _lib.load()
    names = [n for n in _lib.SIGNATURES if n.startswith(("munit_seg_", "munit_space_to_batch", "munit_maxpool",
                                                         "munit_add_relu"))]
    saved = {n: getattr(lib, n) for n in names}
    try:
        for n in names:
            f = saved[n]
            setattr(lib, n, (lambda f, n: lambda *a: calls.append(n) or f(*a))(f, n))
        _step(tr, hp, xa, xb, ma, mb)
        assert ops.SEG_SINK == [] and calls == []
    finally:
        for n, f in saved.items():
            setattr(lib, n, f)
        ops.SEG_SINK = None
