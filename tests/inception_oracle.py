"""Helper of tests/test_cpu_inception.py and tests/test_gpu_inception.py (neither a test module nor a conftest): a plain-torch
CPU restatement of the feature network of FID evaluation -- torchvision's inception_v3 up to Mixed_7c as the reference's
WrapInception.forward (scripts/inception_utils.py:38-85) runs it -- parameterised by dtype.

In fp64 it is the yardstick; in fp32 it measures what fp32 costs (`e32`), as tests/fid_oracle.py does for the distance.
It is written independently of munit_amd/inception.py: its own copy of the architecture table (TABLE), convolution, batch
norm and ReLU as three torch calls (no folding), the branches joined with torch.cat."""
import types

import torch
import torch.nn.functional as F

BN_EPS = 0.001
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)

# name: (in, out, (KH, KW), stride, (pad_h, pad_w))
TABLE = {}


def _add(name, cin, cout, k=(1, 1), stride=1, pad=(0, 0)):
    TABLE[name] = (cin, cout, k, stride, pad)


_add("Conv2d_1a_3x3", 3, 32, (3, 3), 2)
_add("Conv2d_2a_3x3", 32, 32, (3, 3))
_add("Conv2d_2b_3x3", 32, 64, (3, 3), 1, (1, 1))
_add("Conv2d_3b_1x1", 64, 80)
_add("Conv2d_4a_3x3", 80, 192, (3, 3))
for _n, _cin, _pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
    _add(_n + ".branch1x1", _cin, 64)
    _add(_n + ".branch5x5_1", _cin, 48)
    _add(_n + ".branch5x5_2", 48, 64, (5, 5), 1, (2, 2))
    _add(_n + ".branch3x3dbl_1", _cin, 64)
    _add(_n + ".branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1))
    _add(_n + ".branch3x3dbl_3", 96, 96, (3, 3), 1, (1, 1))
    _add(_n + ".branch_pool", _cin, _pf)
_add("Mixed_6a.branch3x3", 288, 384, (3, 3), 2)
_add("Mixed_6a.branch3x3dbl_1", 288, 64)
_add("Mixed_6a.branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1))
_add("Mixed_6a.branch3x3dbl_3", 96, 96, (3, 3), 2)
for _n, _c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
    _add(_n + ".branch1x1", 768, 192)
    _add(_n + ".branch7x7_1", 768, _c7)
    _add(_n + ".branch7x7_2", _c7, _c7, (1, 7), 1, (0, 3))
    _add(_n + ".branch7x7_3", _c7, 192, (7, 1), 1, (3, 0))
    _add(_n + ".branch7x7dbl_1", 768, _c7)
    _add(_n + ".branch7x7dbl_2", _c7, _c7, (7, 1), 1, (3, 0))
    _add(_n + ".branch7x7dbl_3", _c7, _c7, (1, 7), 1, (0, 3))
    _add(_n + ".branch7x7dbl_4", _c7, _c7, (7, 1), 1, (3, 0))
    _add(_n + ".branch7x7dbl_5", _c7, 192, (1, 7), 1, (0, 3))
    _add(_n + ".branch_pool", 768, 192)
_add("Mixed_7a.branch3x3_1", 768, 192)
_add("Mixed_7a.branch3x3_2", 192, 320, (3, 3), 2)
_add("Mixed_7a.branch7x7x3_1", 768, 192)
_add("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3))
_add("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
_add("Mixed_7a.branch7x7x3_4", 192, 192, (3, 3), 2)
for _n, _cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
    _add(_n + ".branch1x1", _cin, 320)
    _add(_n + ".branch3x3_1", _cin, 384)
    _add(_n + ".branch3x3_2a", 384, 384, (1, 3), 1, (0, 1))
    _add(_n + ".branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
    _add(_n + ".branch3x3dbl_1", _cin, 448)
    _add(_n + ".branch3x3dbl_2", 448, 384, (3, 3), 1, (1, 1))
    _add(_n + ".branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1))
    _add(_n + ".branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
    _add(_n + ".branch_pool", _cin, 192)

STEM = ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3", "Conv2d_3b_1x1", "Conv2d_4a_3x3")
MIXED = ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a",
         "Mixed_7b", "Mixed_7c")


def random_state(seed):
    """A seeded fp32 state dict under torchvision's keys: conv weights N(0, 2 / fan_in), gamma and running_var U(0.5, 1.5),
    beta and running_mean 0.1 * N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, (cin, cout, (kh, kw), _, _) in TABLE.items():
        fan_in = cin * kh * kw
        sd[name + ".conv.weight"] = torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / fan_in) ** 0.5
        sd[name + ".bn.weight"] = torch.rand(cout, generator=g) + 0.5
        sd[name + ".bn.bias"] = 0.1 * torch.randn(cout, generator=g)
        sd[name + ".bn.running_mean"] = 0.1 * torch.randn(cout, generator=g)
        sd[name + ".bn.running_var"] = torch.rand(cout, generator=g) + 0.5
    return sd


def basic_conv(state, name, dtype):
    """BasicConv2d `name`: conv (no bias), eval-mode batch norm, ReLU."""
    _, _, _, stride, pad = TABLE[name]
    w, gamma, beta, mean, var = (state[name + k].to(dtype) for k in
                                 (".conv.weight", ".bn.weight", ".bn.bias", ".bn.running_mean", ".bn.running_var"))

    def run(x):
        y = F.conv2d(x, w, None, stride=stride, padding=pad)
        return F.relu(F.batch_norm(y, mean, var, gamma, beta, training=False, eps=BN_EPS))

    return run


def blocks(state, dtype=torch.float64):
    """The five stem convolutions and the eleven Mixed blocks as callables under torchvision's attribute names."""
    c = lambda name: basic_conv(state, name, dtype)
    net = types.SimpleNamespace()
    for name in STEM:
        setattr(net, name, c(name))

    def inception_a(n):
        def run(x):
            b1 = c(n + ".branch1x1")(x)
            b5 = c(n + ".branch5x5_2")(c(n + ".branch5x5_1")(x))
            b3 = c(n + ".branch3x3dbl_3")(c(n + ".branch3x3dbl_2")(c(n + ".branch3x3dbl_1")(x)))
            bp = c(n + ".branch_pool")(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
            return torch.cat([b1, b5, b3, bp], 1)
        return run

    def inception_b(n):
        def run(x):
            b3 = c(n + ".branch3x3")(x)
            bd = c(n + ".branch3x3dbl_3")(c(n + ".branch3x3dbl_2")(c(n + ".branch3x3dbl_1")(x)))
            return torch.cat([b3, bd, F.max_pool2d(x, kernel_size=3, stride=2)], 1)
        return run

    def inception_c(n):
        def run(x):
            b1 = c(n + ".branch1x1")(x)
            b7 = c(n + ".branch7x7_3")(c(n + ".branch7x7_2")(c(n + ".branch7x7_1")(x)))
            bd = x
            for i in range(1, 6):
                bd = c(n + ".branch7x7dbl_%d" % i)(bd)
            bp = c(n + ".branch_pool")(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
            return torch.cat([b1, b7, bd, bp], 1)
        return run

    def inception_d(n):
        def run(x):
            b3 = c(n + ".branch3x3_2")(c(n + ".branch3x3_1")(x))
            b7 = x
            for i in range(1, 5):
                b7 = c(n + ".branch7x7x3_%d" % i)(b7)
            return torch.cat([b3, b7, F.max_pool2d(x, kernel_size=3, stride=2)], 1)
        return run

    def inception_e(n):
        def run(x):
            b1 = c(n + ".branch1x1")(x)
            b3 = c(n + ".branch3x3_1")(x)
            b3 = torch.cat([c(n + ".branch3x3_2a")(b3), c(n + ".branch3x3_2b")(b3)], 1)
            bd = c(n + ".branch3x3dbl_2")(c(n + ".branch3x3dbl_1")(x))
            bd = torch.cat([c(n + ".branch3x3dbl_3a")(bd), c(n + ".branch3x3dbl_3b")(bd)], 1)
            bp = c(n + ".branch_pool")(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
            return torch.cat([b1, b3, bd, bp], 1)
        return run

    for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        setattr(net, n, inception_a(n))
    net.Mixed_6a = inception_b("Mixed_6a")
    for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        setattr(net, n, inception_c(n))
    net.Mixed_7a = inception_d("Mixed_7a")
    for n in ("Mixed_7b", "Mixed_7c"):
        setattr(net, n, inception_e(n))
    return net


def input_lines(x, dtype=torch.float64):
    """The first five lines of WrapInception.forward: normalise, then resize to 299 x 299 unless x has that size."""
    x = x.to(dtype)
    x = (x + 1.0) / 2.0
    # the reference holds mean and std as fp32 parameters: in any dtype the constants are the fp32 values
    mean, std = (torch.tensor(v).to(device=x.device, dtype=dtype).view(1, -1, 1, 1) for v in (MEAN, STD))
    x = (x - mean) / std
    if x.shape[2] != 299 or x.shape[3] != 299:
        x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=True)
    return x


def trunk(net, x):
    """Lines 46-83 on the normalised input; also returns the (name, shape) of every stage."""
    shapes = []
    for name in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3", "max", "Conv2d_3b_1x1", "Conv2d_4a_3x3", "max") + MIXED:
        x = F.max_pool2d(x, kernel_size=3, stride=2) if name == "max" else getattr(net, name)(x)
        shapes.append((name, tuple(x.shape)))
    return torch.mean(x.view(x.size(0), x.size(1), -1), 2), shapes


def features(state, x, dtype=torch.float64):
    """WrapInception(net).forward(x) for the weights `state`: (B, 2048)."""
    with torch.no_grad():
        return trunk(blocks(state, dtype), input_lines(x, dtype))[0]


def fixture_inputs():
    """The two seeded fp64 batches in [-1, 1] of the fixture and of the whole-trunk GPU cases."""
    g = torch.Generator().manual_seed(20)
    small = torch.rand(2, 3, 64, 48, generator=g, dtype=torch.float64) * 2 - 1
    full = torch.rand(1, 3, 299, 299, generator=g, dtype=torch.float64) * 2 - 1
    return {"small": small.float().double(), "full": full.float().double()}
