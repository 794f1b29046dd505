"""fp64 torch-CPU restatement of the trainable segmentation head of adaptation.sem_seg_lambda (scripts/trainer.py:203-223 and
1286-1324 over scripts/resnet.py): layer4 with real dilation-4 convolutions, nn.BatchNorm2d in training mode (batch
statistics, running statistics moved, tests/featda_oracle.batch_norm), F.avg_pool2d(7, 1, 3) with its padding counted, the
1x1 scoring layer, F.interpolate(bilinear, align_corners=False), nn.CrossEntropyLoss, the two-forward update and its Adam
step (oracle.munit_oracle.adam_update).

A head is a dict of tensors under the reference's state_dict keys (0.0.conv1.weight ... 2.bias).  `pins` (optional): what
ops.DANN_SINK recorded from a HIP run of the same call -- per forward the ReLU sign pattern behind bn1 and behind the block
tail of the three blocks, recorded on the device's 4 x 4 phase images (head_pins lays them back out)."""
import math

import torch
import torch.nn.functional as F

from oracle import munit_oracle as O
from tests import featda_oracle as D

CLASSES = 10
PINS_PER_FORWARD = 6
DILATION = 4


def shapes(classes=CLASSES):
    """state_dict keys and shapes of Sequential(layer4, avgpool, Conv2d(512, 10, 1)), in the reference's order"""
    out = {}

    def bn(pre):
        out[pre + ".weight"] = (512,)
        out[pre + ".bias"] = (512,)
        out[pre + ".running_mean"] = (512,)
        out[pre + ".running_var"] = (512,)
        out[pre + ".num_batches_tracked"] = ()

    for i in range(3):
        pre = "0.%d" % i
        out[pre + ".conv1.weight"] = (512, 256 if i == 0 else 512, 3, 3)
        bn(pre + ".bn1")
        out[pre + ".conv2.weight"] = (512, 512, 3, 3)
        bn(pre + ".bn2")
        if i == 0:
            out[pre + ".downsample.0.weight"] = (512, 256, 1, 1)
            bn(pre + ".downsample.1")
    out["2.weight"] = (classes, 512, 1, 1)
    out["2.bias"] = (classes,)
    return out


def is_param(key):
    return D.is_param(key)


def param_names():
    return [k for k in shapes() if is_param(k)]


def params(sd):
    return [sd[k] for k in param_names()]


def make_state(model_seed=0, fc_seed=5, dtype=torch.float64):
    """layer4 of tests/semantic_oracle.make_model(model_seed) under the head's keys and a seeded scoring layer from
    nn.Conv2d(512, 10, 1)'s distribution (uniform in +-1/sqrt(512))"""
    from tests import semantic_oracle as S
    src = S.make_model(model_seed).state_dict()
    g = torch.Generator().manual_seed(fc_seed)
    bound = 1.0 / math.sqrt(512)
    sd = {}
    for k, s in shapes().items():
        if k.startswith("0."):
            v = src["resnet34_8s.layer4." + k[2:]].detach().clone()
            sd[k] = v.to(dtype) if v.is_floating_point() else v
        else:
            sd[k] = ((torch.rand(s, generator=g, dtype=torch.float64) * 2 - 1) * bound).to(dtype)
    assert all(tuple(sd[k].shape) == tuple(s) for k, s in shapes().items())
    return sd


def block(sd, pre, x, pins=None):
    """resnet.BasicBlock of layer4: 3x3, dilation 4, pad 4, stride 1; block 0 has the 1x1 + BN downsample"""
    out = D.batch_norm(sd, pre + ".bn1", F.conv2d(x, sd[pre + ".conv1.weight"], padding=DILATION, dilation=DILATION))
    out = D._relu(out, pins)
    out = D.batch_norm(sd, pre + ".bn2", F.conv2d(out, sd[pre + ".conv2.weight"], padding=DILATION, dilation=DILATION))
    identity = x
    if pre + ".downsample.0.weight" in sd:
        identity = D.batch_norm(sd, pre + ".downsample.1", F.conv2d(x, sd[pre + ".downsample.0.weight"]))
    return D._relu(out + identity, pins)


def head(sd, code, pins=None):
    """segmentation_head(code): (B, 10, h, w) logits at the code's resolution; moves the running statistics"""
    h = code
    for i in range(3):
        h = block(sd, "0.%d" % i, h, pins)
    h = F.avg_pool2d(h, 7, 1, 3)                       # count_include_pad: the divisor is always 49
    return F.conv2d(h, sd["2.weight"], sd["2.bias"])


def ce(out, target, size):
    """trainer.py:1305-1317 for one domain: up-sample to (size, size), CrossEntropyLoss against target.long().squeeze(1)"""
    up = F.interpolate(out, size=(size, size), mode="bilinear", align_corners=False)
    t = target.long()
    return F.cross_entropy(up, t.squeeze(1) if t.dim() == 4 else t)


def head_loss(sd, c_a, c_b, t_a, t_b, size, pins=None):
    """the unweighted loss of segmentation_head_update: two forwards, a then b; also returns the two outputs"""
    o_a = head(sd, c_a, pins)
    o_b = head(sd, c_b, pins)
    return ce(o_a, t_a, size) + ce(o_b, t_b, size), o_a, o_b


class HeadOptimizer(object):
    """segmentation_opt: Adam over the head's parameters, stepped by the plain step()"""

    def __init__(self, sd, hp):
        self.hp = hp
        self.params = params(sd)
        for p in self.params:
            p.requires_grad_(True)
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        self.step_count = 0

    def step(self, grads):
        hp = self.hp
        self.step_count += 1
        with torch.no_grad():
            for p, g, m, v in zip(self.params, grads, self.m, self.v):
                O.adam_update(p, g, m, v, self.step_count, hp["lr"], hp["beta1"], hp["beta2"], 1e-8, hp["weight_decay"])


def head_update(sd, opt, c_a, c_b, t_a, t_b, lamb, size, pins=None):
    """segmentation_head_update on the (detached) codes: returns (weighted loss, gradients); steps `opt`"""
    loss, _, _ = head_loss(sd, c_a.detach(), c_b.detach(), t_a, t_b, size, pins)
    loss = loss * lamb
    grads = torch.autograd.grad(loss, opt.params)
    opt.step(grads)
    return loss.detach(), grads


def unphase4(t):
    """a tensor recorded on the device's 4 x 4 phase images (munit_space_to_batch, f = 4: image (n*4 + py)*4 + px holds the
    pixels (4i + py, 4j + px)) -> plain NCHW"""
    n, c, h, w = t.shape
    return t.reshape(n // 16, 4, 4, c, h, w).permute(0, 3, 4, 1, 5, 2).reshape(n // 16, c, 4 * h, 4 * w)


def head_pins(sink):
    """the ops.kinks(dann=True) list of head forwards (6 records each), laid back out"""
    assert len(sink) % PINS_PER_FORWARD == 0, len(sink)
    return D.Pins([unphase4(t.cpu()) for t in sink])


def load_into(module, sd):
    """copy an oracle state into a munit_amd.segmentation.SegmentationHead (any device)"""
    own = module.state_dict()
    assert list(own) == list(sd), (list(own), list(sd))
    module.load_state_dict({k: sd[k].detach().to(v.dtype) for k, v in own.items()}, strict=True)


def state_of(module, dtype=torch.float64):
    return {k: (v.detach().cpu().to(dtype).clone() if v.is_floating_point() else v.detach().cpu().long().clone())
            for k, v in module.state_dict().items()}


def code(b, h, w, seed, dtype=torch.float64):
    """a seeded (B, 256, h, w) content code: non-negative like the encoder's (it ends in a ReLU), rounded to fp32 values"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, 256, h, w, generator=g, dtype=torch.float32).clamp_min(0).to(dtype)


def labels(b, size, seed, classes=CLASSES):
    """a seeded (B, 1, size, size) float label map of 0..classes-1 in blocks of 4x4 pixels, as the loader delivers it"""
    g = torch.Generator().manual_seed(seed)
    lo = torch.randint(0, classes, (b, 1, (size + 3) // 4, (size + 3) // 4), generator=g)
    return lo.repeat_interleave(4, 2).repeat_interleave(4, 3)[:, :, :size, :size].float().contiguous()
