"""fp64 torch-CPU restatement of output-level domain adaptation: the two simulated / real losses of MsImageDis
(scripts/networks.py:117-162), output_domain_classifier_sr_update (scripts/trainer.py:1267-1284) and the term gen_update
adds under adaptation.output_adv_lambda (trainer.py:527-532, 556-557).  The network, the optimizer arithmetic and the step
are oracle.munit_oracle's (dis_forward, adam_update, OracleTrainer); the kinks of a HIP run are pinned through its
KINK_MASKS, in the order the HIP trainer issues the passes.

A classifier is a dict of leaf tensors under MsImageDis's state_dict keys."""
import torch

from oracle import munit_oracle as O


def shapes(hp):
    """both classifiers are built on input_dim_a (trainer.py:182-187)"""
    return O.dis_param_shapes(hp["dis"], hp["input_dim_a"])


def make_state(hp, tag, dtype=torch.float64):
    return O.make_state(shapes(hp), tag, dtype)


def dis_loss_sr(sd, sim, real, hp_dis):
    """calc_dis_loss_sr: simulated -> 0, real -> 1, summed over the scales"""
    assert hp_dis["gan_type"] == "lsgan"
    loss = 0
    for o0, o1 in zip(O.dis_forward(sd, "", sim, hp_dis), O.dis_forward(sd, "", real, hp_dis)):
        loss = loss + torch.mean((o0 - 0) ** 2) + torch.mean((o1 - 1) ** 2)
    return loss


def gen_loss_sr(sd, fake, hp_dis):
    """calc_gen_loss_sr: target 0.5, summed over the scales"""
    assert hp_dis["gan_type"] == "lsgan"
    loss = 0
    for o0 in O.dis_forward(sd, "", fake, hp_dis):
        loss = loss + torch.mean((o0 - 0.5) ** 2)
    return loss


class ClassifierOptimizer(object):
    """output_classif_opt_sr: Adam over the parameters of classifier a, then b; the update takes the plain step()"""

    def __init__(self, sd_a, sd_b, hp):
        assert "extra" not in hp.get("optimizer", "adam")
        self.hp = hp
        self.params = list(sd_a.values()) + list(sd_b.values())
        for p in self.params:
            p.requires_grad_(True)
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        self.step_count = 0

    def step(self, grads):
        hp = self.hp
        self.step_count += 1
        with torch.no_grad():      # the scheduler of this optimizer is never stepped: the learning rate stays hp["lr"]
            for p, g, m, v in zip(self.params, grads, self.m, self.v):
                O.adam_update(p, g, m, v, self.step_count, hp["lr"], hp["beta1"], hp["beta2"], 1e-8, hp["weight_decay"])


def classifier_update(sd_a, sd_b, opt, x_ar, x_as, x_br, x_bs, hp, b_first=False):
    """output_domain_classifier_sr_update: returns the unweighted loss and the gradients of lambda * loss; steps `opt`.
    The reference evaluates classifier b first; b_first False evaluates a first, the order in which the HIP trainer issues
    the two passes (and records their kinks) -- the value is the same."""
    hd = hp["dis"]
    if b_first:
        l_b = dis_loss_sr(sd_b, x_bs, x_br, hd)
        l_a = dis_loss_sr(sd_a, x_as, x_ar, hd)
    else:
        l_a = dis_loss_sr(sd_a, x_as, x_ar, hd)
        l_b = dis_loss_sr(sd_b, x_bs, x_br, hd)
    loss = l_b + l_a
    grads = torch.autograd.grad(hp["adaptation"]["output_classifier_lambda"] * loss, opt.params)
    opt.step(grads)
    return loss.detach(), grads


def oracle_trainer_class(base=None):
    """An OracleTrainer (or `base`, a subclass of it) whose gen_losses adds output_adv_lambda * (calc_gen_loss_sr of
    classifier a on x_ba + of classifier b on x_ab), evaluated right after the two adversarial terms -- where the HIP
    trainer issues it, so that pinned kinks are consumed in the recorded order.  `attach` hands it the classifiers."""
    base = base or O.OracleTrainer

    class OutdaOracleTrainer(base):
        def attach(self, sd_a, sd_b):
            self.cls_a, self.cls_b = sd_a, sd_b
            self.cls_opt = ClassifierOptimizer(sd_a, sd_b, self.hp)
            return self

        def gen_losses(self, x_a, x_b, mask_a=None, mask_b=None, s_a=None, s_b=None):
            hp = self.hp
            lam = hp["adaptation"]["output_adv_lambda"]
            plain, fakes, term = O.dis_loss_g, [], []

            def hooked(sd, pre, fake, hp_dis):
                out = plain(sd, pre, fake, hp_dis)
                fakes.append(fake)
                if len(fakes) == 2 and lam > 0:          # x_ba went through dis_a, x_ab through dis_b
                    term.append(gen_loss_sr(self.cls_a, fakes[0], hp_dis) + gen_loss_sr(self.cls_b, fakes[1], hp_dis))
                return out

            O.dis_loss_g = hooked
            try:
                L = super().gen_losses(x_a, x_b, mask_a, mask_b, s_a, s_b)
            finally:
                O.dis_loss_g = plain
            assert len(fakes) == 2
            if lam > 0:
                L["loss_output_classifier_sr"] = term[0]
                L["loss_gen_total"] = L["loss_gen_total"] + lam * term[0]
            return L

        def output_domain_classifier_sr_update(self, x_ar, x_as, x_br, x_bs):
            loss, grads = classifier_update(self.cls_a, self.cls_b, self.cls_opt, x_ar, x_as, x_br, x_bs, self.hp)
            self.losses["loss_output_classifier_sr_update"] = loss
            return grads

    return OutdaOracleTrainer


def load_into(module, sd):
    """copy an oracle state into a munit_amd.networks.MsImageDis (any device)"""
    own = module.state_dict()
    assert list(own) == list(sd), (list(own), list(sd))
    module.load_state_dict({k: sd[k].detach().to(v.dtype) for k, v in own.items()}, strict=True)


def images(b, c, size, seed, dtype=torch.float64):
    """seeded (B, C, size, size) images in (-1, 1), rounded to fp32 values so that both sides start from the same numbers"""
    g = torch.Generator().manual_seed(seed)
    return (2 * torch.rand(b, c, size, size, generator=g, dtype=torch.float32) - 1).to(dtype)
