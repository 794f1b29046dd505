"""fp64 torch-CPU restatement of the non-saturating GAN loss (dis.gan_type: nsgan) of MsImageDis, scripts/networks.py:79-139,
in the reference's literal form: per scale mean(binary_cross_entropy(sigmoid(x), target)), summed over the scales.  The network
is oracle.munit_oracle's dis_forward, so the kinks of a HIP run are pinned through O.pinned as for every other loss.

`swapped()` puts the d-loss and the g-loss in place of oracle.munit_oracle's LSGAN ones while active, so OracleTrainer and
tests/parity.run_step_parity evaluate an nsgan step (tests/outda_oracle.py swaps O.dis_loss_g the same way).

The *_softplus twins evaluate the same quantity as mean(softplus(+-x)), the form the HIP kernels use; the literal form loses
digits beyond |x| ~ 8 and saturates in fp32 from ~16.6 on, so only the twins are a yardstick there."""
import contextlib

import torch
import torch.nn.functional as F

from oracle import munit_oracle as O


def bce(x, target):
    """mean(binary_cross_entropy(sigmoid(x), target)) with a constant target: networks.py:93-97"""
    return F.binary_cross_entropy(torch.sigmoid(x), torch.full_like(x, float(target)))


def softplus(x, target):
    """the same mean as mean(max(z, 0) + log1p(exp(-|z|))), z = x for target 0 and -x for target 1"""
    assert target in (0, 1)
    z = x if target == 0 else -x
    return torch.mean(torch.clamp_min(z, 0) + torch.log1p(torch.exp(-z.abs())))


def dis_loss_d(sd, pre, fake, real, hp_dis, term=bce):
    """calc_dis_loss, nsgan branch (networks.py:92-98): fake -> 0, real -> 1"""
    assert hp_dis["gan_type"] == "nsgan"
    loss = 0
    for o0, o1 in zip(O.dis_forward(sd, pre, fake, hp_dis), O.dis_forward(sd, pre, real, hp_dis)):
        loss = loss + term(o0, 0) + term(o1, 1)
    return loss


def dis_loss_g(sd, pre, fake, hp_dis, term=bce):
    """calc_gen_loss, nsgan branch (networks.py:110-112): fake -> 1"""
    assert hp_dis["gan_type"] == "nsgan"
    loss = 0
    for o0 in O.dis_forward(sd, pre, fake, hp_dis):
        loss = loss + term(o0, 1)
    return loss


def dis_loss_sr(sd, sim, real, hp_dis, term=bce):
    """calc_dis_loss_sr, nsgan branch (networks.py:130-136): simulated -> 0, real -> 1"""
    return dis_loss_d(sd, "", sim, real, hp_dis, term)


@contextlib.contextmanager
def swapped():
    """oracle.munit_oracle evaluates dis_loss_d / dis_loss_g as nsgan while active"""
    plain = O.dis_loss_d, O.dis_loss_g
    O.dis_loss_d, O.dis_loss_g = dis_loss_d, dis_loss_g
    try:
        yield
    finally:
        O.dis_loss_d, O.dis_loss_g = plain


def max_logit(sd, xs, hp_dis):
    with torch.no_grad():
        return max(float(o.abs().max()) for x in xs for o in O.dis_forward(sd, "", x, hp_dis))
