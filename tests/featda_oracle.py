"""fp64 torch-CPU restatement of the simulated / real feature classifier (scripts/utils.py:1277-1327, 1370-1392), its
training-mode BatchNorm2d with the running statistics, the three targets of compute_classifier_sr_loss
(scripts/trainer.py:638-667) and the two updates that use it (the fooling term of gen_update, trainer.py:521-525, and
domain_classifier_sr_update, trainer.py:1237-1265), and the step oracle that adds the fooling term (oracle_trainer_class).
The optimizer arithmetic is oracle.munit_oracle's.

A classifier is a dict of tensors under the reference's state_dict keys.  `pins` (optional): what ops.kinks(dann=True) recorded
from a HIP run of the same classifier call -- per call the first max-pool's winners, the ReLU sign pattern behind bn1 and
behind the block tail, then the same three of the second half -- so that both runs differentiate the same piecewise-linear
function; `audit` reports how far from its kink a pinned element that disagrees with the oracle's own choice lies."""
import torch
import torch.nn.functional as F

from oracle import munit_oracle as O

EPS, MOMENTUM = 1e-5, 0.1
PINS_PER_CALL = 6


def shapes():
    """state_dict keys and shapes of domainClassifier(256), in the reference's order"""
    out = {}

    def bn(pre, c):
        out[pre + ".weight"] = (c,)
        out[pre + ".bias"] = (c,)
        out[pre + ".running_mean"] = (c,)
        out[pre + ".running_var"] = (c,)
        out[pre + ".num_batches_tracked"] = ()

    for blk, ci, co in (("BasicBlock1", 256, 128), ("BasicBlock2", 128, 64)):
        out[blk + ".conv1.weight"] = (co, ci, 3, 3)
        bn(blk + ".bn1", co)
        out[blk + ".conv2.weight"] = (co, co, 3, 3)
        bn(blk + ".bn2", co)
        out[blk + ".downsample.0.weight"] = (co, ci, 1, 1)
        bn(blk + ".downsample.1", co)
    out["fc.weight"] = (1, 64)
    out["fc.bias"] = (1,)
    return out


def is_param(key):
    return not key.endswith(("running_mean", "running_var", "num_batches_tracked"))


def make_state(seed, dtype=torch.float64, scale=0.02):
    """seeded weights: N(0, scale) convolutions and head (weights_init("gaussian") has 0.02), BatchNorm weights around 1
    and biases around 0 so that their gradients are exercised, fresh running statistics"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, s in shapes().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(0, dtype=torch.long)
        elif k.endswith("running_mean"):
            sd[k] = torch.zeros(s, dtype=dtype)
        elif k.endswith("running_var"):
            sd[k] = torch.ones(s, dtype=dtype)
        elif ".bn" in k or "downsample.1" in k:
            base = 1.0 if k.endswith("weight") else 0.0
            sd[k] = (base + 0.1 * torch.randn(s, generator=g, dtype=torch.float64)).to(dtype)
        else:
            sd[k] = (scale * torch.randn(s, generator=g, dtype=torch.float64)).to(dtype)
    return sd


def params(sd):
    return [sd[k] for k in shapes() if is_param(k)]


def param_names():
    return [k for k in shapes() if is_param(k)]


class Pins(object):
    def __init__(self, rec):
        self.rec, self.pos = [r.cpu() for r in rec], 0
        self.worst = 0.0            # largest |value| / max|value| among pinned elements that disagree with the oracle's own branch
        self.n_disagree = 0

    def take(self):
        assert self.pos < len(self.rec), "more kinks than recorded"
        self.pos += 1
        return self.rec[self.pos - 1]

    def done(self):
        return self.pos == len(self.rec)


def _relu(x, pins):
    if pins is None:
        return F.relu(x)
    m = pins.take().reshape(x.shape)
    dis = (m != (x > 0)) & (x.detach() != 0)
    if bool(dis.any()):
        pins.n_disagree += int(dis.sum())
        pins.worst = max(pins.worst, float(x.detach()[dis].abs().max()) / float(x.detach().abs().max()))
    return x * m.to(x.dtype)


def _maxpool(x, pins):
    if pins is None:
        return F.max_pool2d(x, 2)
    b, c, h, w = x.shape
    ho, wo = h // 2, w // 2
    idx = pins.take().reshape(b, ho, wo, c).permute(0, 3, 1, 2).long()          # recorded NHWC, window position kh*2 + kw
    win = x[:, :, :2 * ho, :2 * wo].reshape(b, c, ho, 2, wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, c, ho, wo, 4)
    y = win.gather(-1, idx.unsqueeze(-1)).squeeze(-1)
    own = win.detach().max(-1).values
    gap = (own - y.detach()).abs()
    if bool((gap > 0).any()):
        pins.n_disagree += int((gap > 0).sum())
        pins.worst = max(pins.worst, float(gap.max()) / float(x.detach().abs().max()))
    return y


def batch_norm(sd, pre, x, training=True, update=True):
    """nn.BatchNorm2d: batch statistics with the biased variance; the running ones move with the unbiased variance"""
    if not training:
        m, v = sd[pre + ".running_mean"], sd[pre + ".running_var"]
    else:
        m = x.mean((0, 2, 3))
        v = ((x - m[None, :, None, None]) ** 2).mean((0, 2, 3))
        if update:
            n = x.numel() // x.shape[1]
            with torch.no_grad():
                sd[pre + ".running_mean"].mul_(1 - MOMENTUM).add_(MOMENTUM * m.detach())
                sd[pre + ".running_var"].mul_(1 - MOMENTUM).add_(MOMENTUM * v.detach() * n / (n - 1))
                sd[pre + ".num_batches_tracked"] += 1
    xh = (x - m[None, :, None, None]) / torch.sqrt(v[None, :, None, None] + EPS)
    return xh * sd[pre + ".weight"][None, :, None, None] + sd[pre + ".bias"][None, :, None, None]


def basic_block(sd, pre, x, pins=None, training=True):
    out = batch_norm(sd, pre + ".bn1", F.conv2d(x, sd[pre + ".conv1.weight"], padding=1), training)
    out = _relu(out, pins)
    out = batch_norm(sd, pre + ".bn2", F.conv2d(out, sd[pre + ".conv2.weight"], padding=1), training)
    identity = batch_norm(sd, pre + ".downsample.1", F.conv2d(x, sd[pre + ".downsample.0.weight"]), training)
    return _relu(out + identity, pins)


def classifier(sd, x, pins=None, training=True):
    """domainClassifier.forward: (B, 1) for B > 1, (1,) for B = 1 (the reference's .squeeze())"""
    h = _maxpool(x, pins)
    h = basic_block(sd, "BasicBlock1", h, pins, training)
    h = _maxpool(h, pins)
    h = basic_block(sd, "BasicBlock2", h, pins, training)
    h = F.avg_pool2d(h, (16, 16))
    return F.linear(h.squeeze(), sd["fc.weight"], sd["fc.bias"])


def target(domain_synth, fool):
    return 0.5 if fool else (0.0 if domain_synth else 1.0)


def sr_loss(sd_a, sd_b, c_a, c_b, domain_synth=False, fool=False, pins=None):
    """compute_classifier_sr_loss"""
    t = target(domain_synth, fool)
    return torch.mean((classifier(sd_a, c_a, pins) - t) ** 2) + torch.mean((classifier(sd_b, c_b, pins) - t) ** 2)


class ClassifierOptimizer(object):
    """classif_opt_sr: Adam or ExtraAdam over the parameters of classifier a, then b, stepped like classif_opt_sr_step"""

    def __init__(self, sd_a, sd_b, hp):
        self.hp = hp
        self.params = params(sd_a) + params(sd_b)
        for p in self.params:
            p.requires_grad_(True)
        self.extra = "extra" in hp.get("optimizer", "adam")
        self.step_count = 0
        if self.extra:
            self.state = O.ExtraAdamState(self.params, hp["lr"], (hp["beta1"], hp["beta2"]), hp["weight_decay"])
        else:
            self.m = [torch.zeros_like(p) for p in self.params]
            self.v = [torch.zeros_like(p) for p in self.params]
        self.n_extrapolations = self.n_steps = 0

    def step(self, grads, iterations):
        hp = self.hp
        with torch.no_grad():
            if self.extra:
                if iterations % 2 == 0:
                    self.state.extrapolation(grads)
                    self.n_extrapolations += 1
                else:
                    self.state.step(grads)
                    self.n_steps += 1
                return
            self.step_count += 1
            self.n_steps += 1
            for p, g, m, v in zip(self.params, grads, self.m, self.v):
                O.adam_update(p, g, m, v, self.step_count, hp["lr"], hp["beta1"], hp["beta2"], 1e-8, hp["weight_decay"])


def classifier_update(sd_a, sd_b, opt, c_a, c_b, domain_synth, lambda_classifier, iterations, pins=None):
    """domain_classifier_sr_update on the (detached) codes: returns the unweighted loss; steps `opt`"""
    loss = sr_loss(sd_a, sd_b, c_a.detach(), c_b.detach(), domain_synth, False, pins)
    grads = torch.autograd.grad(lambda_classifier * loss, opt.params)
    opt.step(grads, iterations)
    return loss.detach()


def fool_term(sd_a, sd_b, c_a, c_b, pins=None):
    """the adv_lambda term of gen_update: the loss and its gradients with respect to the two codes"""
    c_a = c_a.detach().clone().requires_grad_(True)
    c_b = c_b.detach().clone().requires_grad_(True)
    loss = sr_loss(sd_a, sd_b, c_a, c_b, fool=True, pins=pins)
    g_a, g_b = torch.autograd.grad(loss, [c_a, c_b])
    return loss.detach(), g_a, g_b


def trainer_pins(sink):
    """ops.DANN_SINK of one trainer call.  The two classifiers run on two streams but are issued a-first by the host: the
    first six records are a's."""
    shapes = [tuple(t.shape) for t in sink]
    assert len(sink) == 2 * PINS_PER_CALL and shapes[:PINS_PER_CALL] == shapes[PINS_PER_CALL:]
    return Pins(sink)


def oracle_trainer_class(shared, base=None):
    """An OracleTrainer (or `base`, a subclass of it) whose gen_losses adds, after the base terms, adv_lambda *
    compute_classifier_sr_loss(c_a, c_b, fool=True) on ITS OWN content codes, with the classifiers as the HIP trainer held
    them when its gen_update began (`shared["sd"]`) and the max-pool winners / ReLU signs its gen_update recorded
    (`shared["sink"]`) pinned."""
    class FeatdaOracleTrainer(base or O.OracleTrainer):
        def gen_losses(self, x_a, x_b, mask_a=None, mask_b=None, s_a=None, s_b=None):
            L = super().gen_losses(x_a, x_b, mask_a, mask_b, s_a, s_b)
            lam = self.hp["adaptation"]["adv_lambda"]
            sd_a, sd_b = shared["sd"]
            pins = None if shared.get("sink") is None else trainer_pins(shared["sink"])      # None: unpinned
            L["loss_classifier_sr"] = sr_loss(sd_a, sd_b, self._last["c_a"], self._last["c_b"], fool=True, pins=pins)
            if pins is not None:
                assert pins.done()
                shared["worst"] = max(shared.get("worst", 0.0), pins.worst)
            L["loss_gen_total"] = L["loss_gen_total"] + lam * L["loss_classifier_sr"]
            shared["after"] = (sd_a, sd_b)
            return L

    return FeatdaOracleTrainer


def load_into(module, sd):
    """copy an oracle state into a munit_amd.networks.domainClassifier (any device)"""
    own = module.state_dict()
    assert list(own) == list(sd), (list(own), list(sd))
    module.load_state_dict({k: sd[k].detach().to(v.dtype) for k, v in own.items()}, strict=True)


def code(b, h, w, seed, dtype=torch.float64):
    """a seeded (B, 256, h, w) content code, rounded to fp32 values so that both sides start from the same numbers"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, 256, h, w, generator=g, dtype=torch.float32).to(dtype)
