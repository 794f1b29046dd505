"""fp64 torch-CPU restatement of the two terms of the synthetic-pair generator step: the pair reconstruction loss
(scripts/trainer.py:452-464) and the semantic loss against the simulator's label maps (trainer.py:732-737 with
merge_classes, scripts/utils.py:1330-1353, and the masked form of trainer.py:744-767 with new_class = 10).  The network
and the kink pinning are tests/semantic_oracle.py's."""
import math

import torch
import torch.nn.functional as F

from tests import semantic_oracle as S

# merged class -> its Cityscapes train ids; merged class 0 has no member and stays the constant 0
MEMBERS = ((), (0, 1), (2, 3, 4), (5, 6, 7), (8,), (9,), (10,), (11, 12), (13, 17, 18), (14, 15, 16))
NEW_CLASS = 10
# a masked pixel's loss: log-sum-exp over ten zeros and the mask logit 1, minus that logit
MASKED_PIXEL_LOSS = math.log(NEW_CLASS + math.e) - 1


def merge(out):
    """(B, 19, H, W) logits -> (B, 10, H, W): the sums over each merged class's members, zeros for class 0"""
    cols = [out[:, list(m)].sum(1) if m else torch.zeros_like(out[:, 0]) for m in MEMBERS]
    return torch.stack(cols, 1)


def ce_gt_loss(out, gt, mask=None):
    """compute_semantic_seg_loss with a ground truth on up-sampled 19-class logits `out` (B, 19, H, W); gt (B, H, W) or
    (B, 1, H, W) of any real dtype, truncated like .type(torch.long); mask (B, 1, H, W) of 0 / 1 or None."""
    target = gt.long().reshape(gt.shape[0], gt.shape[-2], gt.shape[-1])
    merged = merge(out)
    if mask is None:
        return F.cross_entropy(merged, target)
    m_long = mask.long().squeeze(1)
    tgt = (1 - m_long) * target + m_long * NEW_CLASS
    m = mask.to(out.dtype)
    return F.cross_entropy(torch.cat(((1 - m) * merged, m), 1), tgt)


def alignment(x_a, x_b):
    """mask_alignment (trainer.py:455-456): 1 where the two images of the pair agree in every channel, (B, 1, H, W)"""
    return (torch.sum(torch.abs(x_a - x_b), 1) == 0).unsqueeze(1).to(x_a.dtype)


def _l1_masked(a, b, mask):
    return torch.mean(torch.abs((a - b) * (1 - mask)))


def pair_loss(x_a, x_b, x_ab, x_ba, l1_masked=_l1_masked):
    """trainer.py:459-464: recon_criterion_mask(x_ab, x_b, 1 - align) + recon_criterion_mask(x_ba, x_a, 1 - align).
    l1_masked: the masked L1 to use (oracle.munit_oracle.l1_masked consumes the pinned signs of a step)."""
    al = alignment(x_a, x_b)
    return l1_masked(x_ab, x_b, 1 - al) + l1_masked(x_ba, x_a, 1 - al)


def pair_inputs(b, size, seed, c=3, dtype=torch.float64):
    """A synthetic pair: x_b equals x_a outside a centred box of half the side and is random inside it (75 % of the
    pixels aligned); x_ab / x_ba are independent random images.  `size`: an int or (height, width)."""
    h, w = (size, size) if isinstance(size, int) else size
    g = torch.Generator().manual_seed(seed)
    x_a = torch.rand(b, c, h, w, generator=g, dtype=torch.float64) * 2 - 1
    x_b = x_a.clone()
    y0, y1, x0, x1 = h // 4, h // 4 + max(1, h // 2), w // 4, w // 4 + max(1, w // 2)
    x_b[:, :, y0:y1, x0:x1] = torch.rand(b, c, y1 - y0, x1 - x0, generator=g, dtype=torch.float64) * 2 - 1
    x_ab = torch.rand(b, c, h, w, generator=g, dtype=torch.float64) * 2 - 1
    x_ba = torch.rand(b, c, h, w, generator=g, dtype=torch.float64) * 2 - 1
    return tuple(t.to(dtype) for t in (x_a, x_b, x_ab, x_ba))


def gt_maps(b, size, seed, block=8):
    """(B, H, W) float64 label maps of seeded block x block squares of integers 0..9; the first ten blocks of every image
    hold the classes 0..9 in order, so every class is present."""
    h, w = (size, size) if isinstance(size, int) else size
    g = torch.Generator().manual_seed(seed)
    nh, nw = -(-h // block), -(-w // block)
    lo = torch.randint(0, 10, (b, nh * nw), generator=g)
    n = min(10, nh * nw)
    lo[:, :n] = torch.arange(n)
    lo = lo.view(b, nh, nw)
    return lo.repeat_interleave(block, 1).repeat_interleave(block, 2)[:, :h, :w].double().contiguous()


def oracle_trainer_class(seg_model, sink, gts, base=None):
    """An OracleTrainer (or `base`, a subclass of it) whose gen_losses adds, after the base terms, the pair reconstruction
    term (recon_synth_w, through oracle.munit_oracle.l1_masked so that the step's last two pinned L1 sign patterns are
    consumed) and the semantic term against the ground truth `gts` = (gt_a, gt_b) (semantic_w) on its own translations.
    `sink`: a callable returning the ops.kinks(seg=...) list as the HIP gen_update left it -- with a ground truth only the logits pass
    records; its kinks are pinned and audited as tests/semantic_oracle.py does.
    Stacked over tests/semantic_oracle.py's class for a whole iteration: an instance whose `synth_call` is False (the call
    being replayed is the real gen_update) adds neither term and leaves the semantic one to that class."""
    from oracle import munit_oracle as O
    n_k = 2 + 2 * sum(n for n, _, _ in S.LAYERS)

    class SynthOracleTrainer(base or O.OracleTrainer):
        audit_bad = None
        synth_call = None

        def gen_losses(self, x_a, x_b, mask_a=None, mask_b=None, s_a=None, s_b=None):
            L = super().gen_losses(x_a, x_b, mask_a, mask_b, s_a, s_b)
            if self.synth_call is False:
                return L
            hp = self.hp
            x_ab, x_ba = self._last["x_ab"], self._last["x_ba"]
            if hp.get("recon_synth_w", 0) > 0:
                L["loss_gen_recon_synth"] = pair_loss(x_a, x_b, x_ab, x_ba, O.l1_masked)
                L["loss_gen_total"] = L["loss_gen_total"] + hp["recon_synth_w"] * L["loss_gen_recon_synth"]
            rec = sink()
            if not hp.get("semantic_w", 0) > 0:
                assert not rec, len(rec)
                type(self).audit_bad = 0
                return L
            sd = S.state(seg_model, x_a.dtype)
            if rec is None:                      # unpinned: the oracle's own branches
                out = S.logits(sd, torch.cat([x_ab, x_ba]))
                type(self).audit_bad = 0
            else:
                assert len(rec) == n_k, len(rec)
                pins = S.seg_pins(rec)
                kinks = []
                out = S.logits(sd, torch.cat([x_ab, x_ba]), kinks=kinks, pins=pins)
                type(self).audit_bad = S.audit(kinks, pins)
            b = x_a.shape[0]
            masked = not hp["adaptation"]["full_adaptation"] and mask_a is not None
            L["loss_sem_seg"] = (ce_gt_loss(out[:b], gts[0], mask_a if masked else None)
                                 + ce_gt_loss(out[b:], gts[1], mask_b if masked else None))
            L["loss_gen_total"] = L["loss_gen_total"] + hp["semantic_w"] * L["loss_sem_seg"]
            return L

    return SynthOracleTrainer
