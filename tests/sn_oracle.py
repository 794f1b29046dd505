"""fp64 torch-CPU restatement of spectral normalisation in the discriminators (dis.norm: sn; SpectralNorm,
scripts/networks.py:885-942, inside Conv2dBlock, networks.py:684-689), on top of oracle.munit_oracle's functions.  Not a test
module.

What the reference computes, pinned by tests/golden/golden_sn.json (tests/test_cpu_sn.py):
  * every forward of a normalised layer advances its state, with W = weight_bar viewed (O, I * kh * kw):
        v <- l2n(W^T u),   u <- l2n(W v),   sigma = u . (W v),   l2n(a) = a / (|a| + 1e-12),
    and the convolution runs with W / sigma -- also under no_grad and in eval();
  * u and v are swapped through `.data`, which autograd does not see: when backward runs, the sigma of EVERY earlier pass is
    differentiated with the u, v of that moment (the latest), while each pass's value keeps its own sigma.  `_Normalise` states
    that rule: d(W / sigma_k) = dW / sigma_k - <g, W> / sigma_k^2 * u_L v_L^T.

A discriminator is an `SnState`: a dict of the trainable leaf tensors under the module's parameter names, in the module's
parameter order (what the optimizer sees: `bias` before `weight_bar`), with the weight_u / weight_v tensors beside it in `.uv`."""
import collections
import contextlib
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import munit_oracle as O

EPS = 1e-12


def l2n(a):
    return a / (a.norm() + EPS)


def load_fixture():
    """tests/golden/golden_sn.json with the arrays it names (golden_sn.npz, golden_sn_b.npz) as tensors under fx["arr"]"""
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(gold, "golden_sn.json")) as f:
        fx = json.load(f)
    fx["arr"] = {}
    for name in ("golden_sn.npz", "golden_sn_b.npz"):
        with np.load(os.path.join(gold, name)) as z:
            fx["arr"].update({k: torch.from_numpy(z[k]) for k in z.files})
    return fx


class SnState(dict):
    """trainable tensors by key (insertion order = the module's parameter order); .uv: weight_u / weight_v by key"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.uv = {}

    def full(self, order=None):
        """everything under the state_dict keys (in `order`, a list of keys, when given)"""
        both = dict(self, **self.uv)
        return collections.OrderedDict((k, both[k]) for k in (order or both))


def is_sn(hp_dis):
    return hp_dis["norm"] == "sn"


def param_shapes(hp_dis, input_dim):
    """names and shapes of MsImageDis's parameters under dis.norm sn, in registration order: the first block of a scale
    (norm 'none') and the final 1x1 convolution stay plain; a normalised convolution is conv.module.{bias, weight_u, weight_v,
    weight_bar}"""
    out = collections.OrderedDict()
    for s in range(hp_dis["num_scales"]):
        d, ci = hp_dis["dim"], input_dim
        for l in range(hp_dis["n_layer"]):
            co = d if l == 0 else 2 * d
            p = "cnns.%d.%d.conv." % (s, l)
            if l == 0:
                out[p + "weight"], out[p + "bias"] = (co, ci, 4, 4), (co,)
            else:
                out[p + "module.bias"], out[p + "module.weight_u"] = (co,), (co,)
                out[p + "module.weight_v"], out[p + "module.weight_bar"] = (ci * 16,), (co, ci, 4, 4)
                d *= 2
            ci = co
        out["cnns.%d.%d.weight" % (s, hp_dis["n_layer"])] = (1, ci, 1, 1)
        out["cnns.%d.%d.bias" % (s, hp_dis["n_layer"])] = (1,)
    return out


def from_full(full, dtype=torch.float64):
    sd = SnState()
    for k, v in full.items():
        t = v.detach().to(dtype).clone()
        if k.endswith(("weight_u", "weight_v")):
            sd.uv[k] = t
        else:
            sd[k] = t.requires_grad_(True)
    return sd


def make_state(hp_dis, input_dim, tag, dtype=torch.float64):
    """deterministic state (O.fill_det); weight_u / weight_v l2-normalised as _make_params leaves them, and rounded to fp32
    values so that a HIP module loaded from it starts from the same numbers"""
    full = collections.OrderedDict()
    for k, shape in param_shapes(hp_dis, input_dim).items():
        t = O.fill_det(tag + k, shape, dtype=torch.float64)
        if k.endswith(("weight_u", "weight_v")):
            t = l2n(O.fill_det(tag + k, shape, scale=1.0, dtype=torch.float64))
        full[k] = t.float().double()
    return from_full(full, dtype)


def load_into(module, sd):
    """copy an SnState into a munit_amd.networks.MsImageDis (any device)"""
    own = module.state_dict()
    full = sd.full()
    assert sorted(own) == sorted(full), (list(own), list(full))
    module.load_state_dict({k: full[k].detach().to(v.dtype) for k, v in own.items()}, strict=True)


def power_iteration(w, u, v):
    """one iteration, in place on u and v; returns sigma (all of it outside autograd, as the reference's `.data`)"""
    with torch.no_grad():
        m = w.detach().reshape(w.shape[0], -1)
        v.copy_(l2n(m.t().mv(u)))
        wv = m.mv(v)
        u.copy_(l2n(wv))
        return u.dot(wv)


class _Normalise(torch.autograd.Function):
    """W / sigma, sigma = u^T W v of the pass; backward with the u, v the state holds THEN"""

    @staticmethod
    def forward(ctx, w, sigma, u, v):
        ctx.save_for_backward(w, sigma)
        ctx.uv = (u, v)              # the state's tensors themselves: later iterations write into them
        return w / sigma

    @staticmethod
    def backward(ctx, g):
        w, sigma = ctx.saved_tensors
        u, v = ctx.uv
        coef = (g * w).sum() / sigma ** 2
        return g / sigma - coef * torch.outer(u, v).reshape(w.shape), None, None, None


def normalised_weight(sd, p):
    """SpectralNorm._update_u_v for the layer whose parameters live under `p` (ends in 'module.')"""
    w, u, v = sd[p + "weight_bar"], sd.uv[p + "weight_u"], sd.uv[p + "weight_v"]
    sigma = power_iteration(w, u, v)
    return _Normalise.apply(w, sigma, u, v)


def dis_forward(sd, pre, x, hp_dis):
    """MsImageDis.forward under dis.norm sn (O.dis_forward for every other norm)"""
    if not is_sn(hp_dis):
        return _PLAIN_DIS_FORWARD(sd, pre, x, hp_dis)
    outs = []
    for s in range(hp_dis["num_scales"]):
        h = x
        p = pre + "cnns.%d." % s
        for l in range(hp_dis["n_layer"]):
            if l == 0:
                w, b = sd[p + "0.conv.weight"], sd[p + "0.conv.bias"]
            else:
                q = p + "%d.conv.module." % l
                w, b = normalised_weight(sd, q), sd[q + "bias"]
            h = O.conv_block(h, w, b, 2, 1, hp_dis["pad_type"], None, hp_dis["activ"])
        l = hp_dis["n_layer"]
        outs.append(F.conv2d(h, sd[p + "%d.weight" % l], sd[p + "%d.bias" % l]))
        x = O.avgpool_3s2(x)
    return outs


_PLAIN_DIS_FORWARD = O.dis_forward


@contextlib.contextmanager
def spectral():
    """Inside the block oracle.munit_oracle's dis_forward -- and with it dis_loss_d / dis_loss_g and the simulated / real
    losses of tests/outda_oracle.py -- knows dis.norm sn; the module's own function is back on exit."""
    before, O.dis_forward = O.dis_forward, dis_forward
    try:
        yield
    finally:
        O.dis_forward = before


def calc(fn, sd, hp_dis, *xs):
    """fn in calc_dis_loss / calc_gen_loss / calc_dis_loss_sr / calc_gen_loss_sr on the state `sd`"""
    from tests import outda_oracle as D
    with spectral():
        if fn == "calc_dis_loss":
            return O.dis_loss_d(sd, "", xs[0], xs[1], hp_dis)
        if fn == "calc_gen_loss":
            return O.dis_loss_g(sd, "", xs[0], hp_dis)
        if fn == "calc_dis_loss_sr":
            return D.dis_loss_sr(sd, xs[0], xs[1], hp_dis)
        if fn == "calc_gen_loss_sr":
            return D.gen_loss_sr(sd, xs[0], hp_dis)
    raise ValueError(fn)


def oracle_trainer_class(base=None):
    """OracleTrainer (or `base`, a subclass of it) whose discriminators -- and output classifiers, when `base` has them --
    are SnStates: every loss graph and every update runs inside `spectral()`."""
    base = base or O.OracleTrainer

    class SnOracleTrainer(base):
        def gen_losses(self, *a, **k):
            with spectral():
                return super().gen_losses(*a, **k)

        def dis_losses(self, *a, **k):
            with spectral():
                return super().dis_losses(*a, **k)

        def output_domain_classifier_sr_update(self, *a, **k):
            with spectral():
                return super().output_domain_classifier_sr_update(*a, **k)

    return SnOracleTrainer
