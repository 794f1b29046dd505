"""fp64 torch-CPU restatement of the semantic-consistency loss (scripts/trainer.py:706-771) and its network, Resnet34_8s
(scripts/utils.py:933-983 over scripts/resnet.py): dilated convolutions as such, BatchNorm in eval mode unfused,
nn.MaxPool2d, F.interpolate(bilinear, align_corners=False), nn.CrossEntropyLoss.  It reads the parameters of a
munit_amd.segmentation.Resnet34_8s (same keys as the reference's state_dict)."""
import math

import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
LAYERS = ((3, 1, 1), (4, 2, 1), (6, 1, 2), (3, 1, 4))     # blocks, first stride, dilation
# a masked pixel's loss: log-sum-exp over nineteen zeros and the mask logit 1, minus that logit
MASKED_PIXEL_LOSS = math.log(19 + math.e) - 1


def state(model, dtype=torch.float64):
    return {k: v.detach().to("cpu", dtype if v.is_floating_point() else v.dtype) for k, v in model.state_dict().items()}


def _bn(x, sd, p, calib=None):
    if calib is not None:       # calibration pass: running statistics := this batch's (momentum=None after one batch)
        n = x.numel() // x.shape[1]
        mean = x.mean((0, 2, 3))
        var = ((x - mean.view(1, -1, 1, 1)) ** 2).sum((0, 2, 3)) / (n - 1)
        sd[p + ".running_mean"].copy_(mean)
        sd[p + ".running_var"].copy_(var)
        calib[p] = (mean, var)
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False,
                        0.0, 1e-5)


def transform(x):
    """seg_transform((x + 1) / 2) (trainer.py:720-725, utils.py:159-174) of images in [-1, 1]."""
    m = torch.tensor(MEAN, dtype=x.dtype).view(1, 3, 1, 1)
    s = torch.tensor(STD, dtype=x.dtype).view(1, 3, 1, 1)
    return ((x + 1) / 2.0 - m) / s


def unphase(t, times):
    """a tensor recorded in the device's phase-major layout (munit_space_to_batch by 2, `times` times) -> plain NCHW"""
    for _ in range(times):
        n, c, h, w = t.shape
        t = t.reshape(n // 4, 2, 2, c, h, w).permute(0, 3, 4, 1, 5, 2).reshape(n // 4, c, 2 * h, 2 * w)
    return t


def seg_pins(sink):
    """The device's kinks in SEG_SINK order (one network forward): ReLU sign patterns in plain NCHW and the max-pool's
    winner positions (B, C, Ho, Wo).  Layer3 records in the 2x2 phase layout, layer4 in the 4x4 one."""
    out = [sink[0].cpu(), sink[1].cpu().permute(0, 3, 1, 2).long()]
    k = 2
    for li, (n, _, _) in enumerate(LAYERS):
        for _ in range(2 * n):
            out.append(unphase(sink[k].cpu(), max(0, li - 1)))
            k += 1
    return out


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
        return F.max_pool2d(v, 3, 2, 1)
    b, c, h, w = v.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    cols = F.unfold(F.pad(v, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(b, c, 9, ho, wo)
    return cols.gather(2, next(pins).unsqueeze(2)).squeeze(2)


def logits(sd, x, up=True, kinks=None, calib=None, pins=None):
    """Resnet34_8s.forward of transform(x); up=False stops before the bilinear up-sample.  kinks: list receiving the
    pre-activations of every ReLU and the inputs of every max-pool, in the order the device path records them.
    pins: the device's decisions at those kinks (seg_pins), taken instead of the oracle's own."""
    pre = "resnet34_8s."
    pins = iter(pins) if pins is not None else None
    h = F.conv2d(transform(x), sd[pre + "conv1.weight"], None, 2, 3)
    h = _bn(h, sd, pre + "bn1", calib)
    h = _relu(h, kinks, pins)
    h = _pool(h, kinks, pins)
    for li, (n, stride, dil) in enumerate(LAYERS):
        for i in range(n):
            p = pre + "layer%d.%d." % (li + 1, i)
            s = stride if i == 0 else 1
            o = _bn(F.conv2d(h, sd[p + "conv1.weight"], None, s, dil, dil), sd, p + "bn1", calib)
            o = _bn(F.conv2d(_relu(o, kinks, pins), sd[p + "conv2.weight"], None, 1, dil, dil), sd, p + "bn2", calib)
            r = h
            if p + "downsample.0.weight" in sd:
                r = _bn(F.conv2d(h, sd[p + "downsample.0.weight"], None, s), sd, p + "downsample.1", calib)
            h = _relu(o + r, kinks, pins)
    z = F.conv2d(h, sd[pre + "fc.weight"], sd[pre + "fc.bias"])
    if not up:
        return z
    return F.interpolate(z, size=x.shape[2:], mode="bilinear", align_corners=False)


def ce_loss(out, target, mask=None):
    """The two branches of compute_semantic_seg_loss (trainer.py:746-771) on up-sampled logits `out` (B, 19, H, W)
    and integer targets (B, H, W); mask (B, 1, H, W) of 0 / 1 or None."""
    if mask is None:
        return F.cross_entropy(out, target)
    m_long = mask.long().squeeze(1)
    tgt = (1 - m_long) * target + m_long * 19
    m = mask.to(out.dtype)
    return F.cross_entropy(torch.cat(((1 - m) * out, m), 1), tgt)


def semantic_loss(sd, x_orig, x_trans, mask=None):
    """seg(x_orig, x_trans, mask): labels from the original image, logits from the translation; returns (loss, labels)."""
    with torch.no_grad():
        labels = logits(sd, x_orig).argmax(1)
    return ce_loss(logits(sd, x_trans), labels, mask), labels


# decode_segmap's Cityscapes train-id colours (scripts/utils.py:994-1013), restated here rather than taken from the code
# under test
PALETTE = ((128, 64, 128), (244, 35, 232), (70, 70, 70), (102, 102, 156), (190, 153, 153), (153, 153, 153),
           (250, 170, 30), (220, 220, 0), (107, 142, 35), (152, 251, 152), (70, 130, 180), (220, 20, 60), (255, 0, 0),
           (0, 0, 142), (0, 0, 70), (0, 60, 100), (0, 80, 100), (0, 0, 230), (119, 11, 32))


def colorize(labels):
    """decode_segmap + ToTensor: (B, H, W) labels -> (B, 3, H, W) in [0, 1]"""
    pal = torch.tensor(PALETTE, dtype=torch.float64) / 255.0
    return pal[labels.long()].permute(0, 3, 1, 2)


def make_model(seed=0, calib_images=None):
    """A deterministic Resnet34_8s: He-normal convolutions, random BN affines, and running statistics calibrated on
    seeded images (each BN's statistics = the batch statistics of its input there, unbiased variance), so that every
    layer sees O(1) activations and the logits are O(1-10) with a meaningful argmax."""
    from munit_amd.segmentation import Resnet34_8s
    g = torch.Generator().manual_seed(seed)
    m = Resnet34_8s(19)
    with torch.no_grad():
        for name, t in m.state_dict().items():
            if name.endswith("num_batches_tracked"):
                continue
            if t.dim() == 4:
                fan = t.shape[1] * t.shape[2] * t.shape[3]
                t.copy_(torch.randn(t.shape, generator=g, dtype=torch.float64) * math.sqrt(2.0 / fan))
            elif name.endswith(".weight"):
                t.copy_(0.5 + torch.rand(t.shape, generator=g, dtype=torch.float64))
            elif name.endswith(".bias"):
                t.copy_(0.1 * torch.randn(t.shape, generator=g, dtype=torch.float64))
        if calib_images is None:
            calib_images = torch.rand((2, 3, 64, 64), generator=g, dtype=torch.float64) * 2 - 1
        sd = state(m)
        logits(sd, calib_images.double(), up=False, calib={})
        for k, v in m.state_dict().items():
            if k.endswith("running_mean") or k.endswith("running_var"):
                v.copy_(sd[k])
    m.eval()
    return m


def rand_images(b, size, seed):
    """smooth-ish images in [-1, 1] (the generator's output range)"""
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand((b, 3, size // 8, size // 8), generator=g, dtype=torch.float64)
    x = F.interpolate(lo, size=(size, size), mode="bilinear", align_corners=False)
    x = x + 0.1 * torch.randn((b, 3, size, size), generator=g, dtype=torch.float64)
    return x.clamp(0, 1) * 2 - 1


def audit(kinks, pins, rel=1e-5):
    """Count the device decisions that differ from the oracle's own where the oracle's margin is not at rounding-noise
    size (|pre-activation| or the gap between the two largest window entries above rel * the tensor's scale)."""
    bad = 0
    for (kind, v), pin in zip(kinks, pins):
        v = v.detach()
        tol = rel * v.abs().max().item()
        if kind == "relu":
            bad += int((((v > 0) != pin.bool()) & (v.abs() > tol)).sum())
        else:
            b, c, h, w = v.shape
            ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            cols = F.unfold(F.pad(v, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(b, c, 9, ho, wo)
            mx = cols.max(2).values
            chosen = cols.gather(2, pin.unsqueeze(2)).squeeze(2)
            bad += int((mx - chosen > tol).sum())
    return bad


def oracle_trainer_class(seg_model, sink, base=None):
    """An OracleTrainer (or `base`, a subclass of it) whose gen_losses adds the semantic term (trainer.py:504-509, 552) on
    its own translations self._last["x_ab"] / ["x_ba"].  `sink`: a callable returning the ops.kinks(seg=...) list as the HIP gen_update
    left it (label pass kinks, labels, logits pass kinks); the oracle takes the device's labels and kink branches and audits
    them (`audit` allows a disagreement only at rounding-noise margins; labels only where the top-2 gap is that small).
    Stacked under tests/synth_oracle.py's class for a whole iteration: an instance whose `synth_call` is True (the call
    being replayed is gen_update(synth=True) with a ground truth) leaves the term to that class."""
    from oracle import munit_oracle as O
    n_k = 2 + 2 * sum(n for n, _, _ in LAYERS)       # kinks recorded per network forward

    class SemanticOracleTrainer(base or O.OracleTrainer):
        audit_bad = None
        synth_call = None

        def gen_losses(self, x_a, x_b, mask_a=None, mask_b=None, s_a=None, s_b=None):
            L = super().gen_losses(x_a, x_b, mask_a, mask_b, s_a, s_b)
            hp = self.hp
            if not hp.get("semantic_w", 0) > 0 or self.synth_call is True:
                return L
            sd = state(seg_model, x_a.dtype)
            rec = sink()
            b = x_a.shape[0]
            if rec is None:                      # unpinned: the oracle's own labels and branches
                with torch.no_grad():
                    labels = logits(sd, torch.cat([x_a, x_b])).argmax(1)
                out = logits(sd, torch.cat([self._last["x_ab"], self._last["x_ba"]]))
                bad = 0
            else:
                assert len(rec) == 2 * n_k + 1, len(rec)
                pin_lab, labels, pin_log = seg_pins(rec[:n_k]), rec[n_k].cpu().long(), seg_pins(rec[n_k + 1:])
                kinks = []
                with torch.no_grad():
                    up = logits(sd, torch.cat([x_a, x_b]), kinks=kinks, pins=pin_lab)
                bad = audit(kinks, pin_lab)
                top = up.topk(2, 1).values
                bad += int(((up.argmax(1) != labels) & ((top[:, 0] - top[:, 1]) > 1e-5 * up.abs().max())).sum())
                kinks = []
                out = logits(sd, torch.cat([self._last["x_ab"], self._last["x_ba"]]), kinks=kinks, pins=pin_log)
                bad += audit(kinks, pin_log)
            type(self).audit_bad = bad
            masked = not hp["adaptation"]["full_adaptation"] and mask_a is not None
            L["loss_sem_seg"] = (ce_loss(out[:b], labels[:b], mask_a if masked else None)
                                 + ce_loss(out[b:], labels[b:], mask_b if masked else None))
            L["loss_gen_total"] = L["loss_gen_total"] + hp["semantic_w"] * L["loss_sem_seg"]
            return L

    return SemanticOracleTrainer
