"""fp64 torch-CPU restatement of the domain-invariant perceptual loss: vgg_preprocess (scripts/utils.py:1051-1063),
networks.Vgg16 (scripts/networks.py:755-804; NO pool between relu4_3 and conv5_1) and compute_vgg_loss
(scripts/trainer.py:618-636) with nn.InstanceNorm2d(512, affine=False).  It reads the parameters of a munit_amd.vgg.Vgg16
(the reference's state_dict keys)."""
import math

import torch
import torch.nn.functional as F

BGR_MEAN = (103.939, 116.779, 123.680)
# the reference's module tree, restated: (name, input channels, output channels), and the layers a 2x2 pool follows
LAYERS = (("conv1_1", 3, 64), ("conv1_2", 64, 64), ("conv2_1", 64, 128), ("conv2_2", 128, 128), ("conv3_1", 128, 256),
          ("conv3_2", 256, 256), ("conv3_3", 256, 256), ("conv4_1", 256, 512), ("conv4_2", 512, 512), ("conv4_3", 512, 512),
          ("conv5_1", 512, 512), ("conv5_2", 512, 512), ("conv5_3", 512, 512))
POOL_AFTER = ("conv1_2", "conv2_2", "conv3_3")
N_KINKS = len(LAYERS) + len(POOL_AFTER)        # kinks one network forward records: 13 ReLUs and 3 pools, in call order


def state(model, dtype=torch.float64):
    return {k: v.detach().to("cpu", dtype) for k, v in model.state_dict().items()}


def preprocess(x):
    """vgg_preprocess of images in [-1, 1]: RGB -> BGR, [0, 255], minus the Caffe means."""
    b = torch.cat(tuple(reversed(torch.chunk(x, 3, dim=1))), dim=1)
    b = (b + 1) * 255 * 0.5
    return b - torch.tensor(BGR_MEAN, dtype=x.dtype).view(1, 3, 1, 1)


def vgg_pins(sink):
    """The device's kinks of ONE network forward in VGG_SINK order: ReLU sign patterns (B, C, H, W) and the pools' winner
    positions kh * 2 + kw as (B, C, Ho, Wo)."""
    assert len(sink) == N_KINKS, len(sink)
    out = []
    for t in sink:
        t = t.cpu()
        out.append(t.permute(0, 3, 1, 2).long() if t.dtype == torch.uint8 else t)
    return out


def _windows(v):
    b, c, h, w = v.shape
    ho, wo = h // 2, w // 2
    return F.unfold(v[:, :, :2 * ho, :2 * wo], 2, stride=2).view(b, c, 4, ho, wo)


def _relu(v, kinks, pins):
    if kinks is not None:
        kinks.append(("relu", v))
    if pins is not None:
        return v * next(pins).to(v.dtype)
    return F.relu(v)


def _pool(v, kinks, pins):
    if kinks is not None:
        kinks.append(("pool", v))
    if pins is None:
        return F.max_pool2d(v, kernel_size=2, stride=2)
    return _windows(v).gather(2, next(pins).unsqueeze(2)).squeeze(2)


def features(sd, x, kinks=None, pins=None):
    """relu5_3 of Vgg16(vgg_preprocess(x)).  kinks: list receiving the pre-activation of every ReLU and the input of every
    pool, in the order the device path records them; pins: the device's decisions there (vgg_pins), taken instead of the
    oracle's own."""
    pins = iter(pins) if pins is not None else None
    h = preprocess(x)
    for name, _, _ in LAYERS:
        h = _relu(F.conv2d(h, sd[name + ".weight"], sd[name + ".bias"], 1, 1), kinks, pins)
        if name in POOL_AFTER:
            h = _pool(h, kinks, pins)
    return h


def in_mse(f, t):
    """torch.mean((instancenorm(f) - instancenorm(t)) ** 2) with nn.InstanceNorm2d(C, affine=False): biased variance, eps 1e-5"""
    return torch.mean((F.instance_norm(f, eps=1e-5) - F.instance_norm(t, eps=1e-5)) ** 2)


def vgg_loss(sd, img, target, pins_img=None, pins_target=None, kinks_img=None, kinks_target=None):
    """compute_vgg_loss(vgg, img, target).  The reference back-propagates into both arguments; in gen_update the second is an
    original image, which needs no gradient."""
    return in_mse(features(sd, img, kinks_img, pins_img), features(sd, target, kinks_target, pins_target))


def audit(kinks, pins):
    """(worst_rel, disagree_frac) of the device's decisions against the oracle's own: the largest |pre-activation| (ReLU) or
    gap between the window's maximum and the chosen entry (pool), relative to the tensor's largest magnitude, at which the two
    differ, and the share of decisions that differ.  To be held to tests/parity.KINK_NOISE / KINK_FRAC."""
    worst, n_bad, n_all = 0.0, 0, 0
    for (kind, v), pin in zip(kinks, pins):
        v = v.detach()
        scale = max(v.abs().max().item(), 1e-300)
        if kind == "relu":
            bad = (v > 0) != pin.bool()
            margin = v.abs()
        else:
            win = _windows(v)
            margin = win.max(2).values - win.gather(2, pin.unsqueeze(2)).squeeze(2)
            bad = margin > 0
        n_all += bad.numel()
        if bool(bad.any()):
            n_bad += int(bad.sum())
            worst = max(worst, float(margin[bad].max()) / scale)
    return worst, n_bad / max(1, n_all)


def make_model(seed=0):
    """A deterministic Vgg16: He-normal weights, small random biases, from a seeded CPU generator (the real network's 59 MB
    of weights are never committed).  On preprocessed images (magnitude ~1e2) every layer's activations keep that order."""
    from munit_amd.vgg import Vgg16
    g = torch.Generator().manual_seed(seed)
    m = Vgg16()
    with torch.no_grad():
        for name, t in m.state_dict().items():
            if t.dim() == 4:
                fan = t.shape[1] * t.shape[2] * t.shape[3]
                t.copy_(torch.randn(t.shape, generator=g, dtype=torch.float64) * math.sqrt(2.0 / fan))
            else:
                t.copy_(0.1 * torch.randn(t.shape, generator=g, dtype=torch.float64))
    m.eval()
    return m


def rand_images(b, h, w, seed):
    """smooth-ish images in [-1, 1] (the generator's output range)"""
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand((b, 3, max(1, h // 8), max(1, w // 8)), generator=g, dtype=torch.float64)
    x = F.interpolate(lo, size=(h, w), mode="bilinear", align_corners=False)
    x = x + 0.1 * torch.randn((b, 3, h, w), generator=g, dtype=torch.float64)
    return x.clamp(0, 1) * 2 - 1


def oracle_trainer_class(vgg_model, sink, base=None):
    """An OracleTrainer (or `base`, a subclass of it) whose gen_losses adds the two perceptual terms (trainer.py:493-502,
    550-551) on its own translations self._last["x_ba"] / ["x_ab"].  `sink`: a callable returning the ops.kinks(vgg=...) list
    as the HIP gen_update left it -- the target pass over (x_b, x_a), then the pass over (x_ba, x_ab), N_KINKS entries
    each -- or None (unpinned).  The oracle takes the device's branches and audits them; the class keeps the worst audit in
    `audit_worst` = (worst_rel, disagree_frac)."""
    from oracle import munit_oracle as O

    class VggOracleTrainer(base or O.OracleTrainer):
        audit_worst = None

        def gen_losses(self, x_a, x_b, mask_a=None, mask_b=None, s_a=None, s_b=None):
            L = super().gen_losses(x_a, x_b, mask_a, mask_b, s_a, s_b)
            hp = self.hp
            if not hp.get("vgg_w", 0) > 0:
                return L
            sd = state(vgg_model, x_a.dtype)
            rec = sink()
            b = x_a.shape[0]
            trans = torch.cat([self._last["x_ba"], self._last["x_ab"]])
            orig = torch.cat([x_b, x_a])
            if rec is None:
                with torch.no_grad():
                    target = features(sd, orig)
                feat = features(sd, trans)
            else:
                assert len(rec) == 2 * N_KINKS, len(rec)
                pin_t, pin_f = vgg_pins(rec[:N_KINKS]), vgg_pins(rec[N_KINKS:])
                kt, kf = [], []
                with torch.no_grad():
                    target = features(sd, orig, kt, pin_t)
                feat = features(sd, trans, kf, pin_f)
                a_t, a_f = audit(kt, pin_t), audit(kf, pin_f)
                type(self).audit_worst = (max(a_t[0], a_f[0]), max(a_t[1], a_f[1]))
            L["loss_gen_vgg_a"] = in_mse(feat[:b], target[:b])
            L["loss_gen_vgg_b"] = in_mse(feat[b:], target[b:])
            L["loss_gen_total"] = L["loss_gen_total"] + hp["vgg_w"] * (L["loss_gen_vgg_a"] + L["loss_gen_vgg_b"])
            return L

    return VggOracleTrainer
