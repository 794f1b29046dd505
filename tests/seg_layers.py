"""The 37 frozen convolutions of munit_amd.segmentation.Resnet34_8s for a crop and an image count, read off the module
itself: `Resnet34_8s.forward` runs on `meta` tensors with the five ops it calls (ops.seg_input, frozen_conv, maxpool3s2,
space_to_batch, add_relu) replaced by shape-only stand-ins that record what they are given.  Not a test module:
tests/test_cpu_dispatch.py (which kernel form carries each layer) and tests/test_gpu_semantic.py (the descriptors the
device path really plans equal this list) use it."""
import collections

import torch

from munit_amd import ops
from munit_amd.segmentation import Resnet34_8s

# case: the op-case tuple of tests/test_cpu_dispatch.py (cin, cout, k, stride, pad, pad_type, ups, act, B, H, W) of the
# forward; kd: the filter size backward-data multiplies by (8 / 4 / 2 for the stride-2 odd kernels, else k); add: its
# backward-data carries the block's skip gradient as the `add` operand; parked: its dx goes to the block's link, not on
SegLayer = collections.namedtuple("SegLayer", "name case kd bias add parked")

_NET = []


def _net():
    if not _NET:
        with torch.device("meta"):
            _NET.append(Resnet34_8s())
    return _NET[0]


def trace(crop, images):
    """(layers, batches): the SegLayer of every frozen_conv call of one forward of `images` crop x crop images, in call
    order, and the batch after each space_to_batch call (two splits, two inverses)."""
    net = _net()
    names = {id(v[0]): k for k, v in net.folded(torch.device("meta")).items()}
    layers, batches = [], []

    def seg_input(*xs):
        return xs[0].new_empty(sum(x.shape[0] for x in xs), *xs[0].shape[1:])

    def frozen_conv(x, weight, bias, w_dgrad, stride, pad, act="none", link_in=None, link_out=None):
        b, cin, h, w = x.shape
        cout, cin_w, k, kw = weight.shape
        assert cin_w == cin and kw == k and w_dgrad.shape[:2] == weight.shape[:2] and w_dgrad.shape[2] == w_dgrad.shape[3]
        layers.append(SegLayer(names[id(weight)], (cin, cout, k, stride, pad, "zero", 0, act, b, h, w), w_dgrad.shape[2],
                               bias is not None, link_in is not None, link_out is not None))
        return x.new_empty(b, cout, (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1)

    def maxpool3s2(x):
        b, c, h, w = x.shape
        return x.new_empty(b, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1)

    def space_to_batch(x, f, inverse=False):
        n, c, h, w = x.shape
        y = x.new_empty(n // (f * f), c, h * f, w * f) if inverse else x.new_empty(n * f * f, c, h // f, w // f)
        batches.append(y.shape[0])
        return y

    def add_relu(a, r, link=None):
        assert a.shape == r.shape, (a.shape, r.shape)
        return a.new_empty(a.shape)

    # The five names are swapped on the munit_amd.ops module itself and restored below.  Never call this while device work
    # that goes through ops.frozen_conv and its kin is in flight on another thread: that work would meet the stand-ins.
    stand_ins = dict(seg_input=seg_input, frozen_conv=frozen_conv, maxpool3s2=maxpool3s2, space_to_batch=space_to_batch,
                     add_relu=add_relu)
    saved = {k: getattr(ops, k) for k in stand_ins}
    for k, v in stand_ins.items():
        setattr(ops, k, v)
    try:
        z = net(torch.empty(images, 3, crop, crop, device="meta"))
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
    assert tuple(z.shape) == (images, 19, crop // 8, crop // 8), z.shape
    return layers, batches


def seg_layers(crop, images):
    return trace(crop, images)[0]


def dgrad_case(layer):
    """The op-case tuple munit_conv2d_kernel_name is asked with for the layer's backward-data: the zero-extended filter,
    no activation (ops plans the three passes that way)."""
    cin, cout, k, stride, pad, pt, ups, act, b, h, w = layer.case
    return (cin, cout, layer.kd, stride, pad, pt, ups, "none", b, h, w)


def fwd_call(layer):
    """What ops.conv2d_fwd_raw is called with for the layer: (x shape, weight shape, bias given, stride, pad, pad type,
    up-sample, activation)."""
    cin, cout, k, stride, pad, pt, ups, act, b, h, w = layer.case
    return ((b, cin, h, w), (cout, cin, k, k), layer.bias, stride, pad, pt, bool(ups), act)


def dgrad_call(layer):
    """What ops.conv2d_dgrad_raw is called with: (x shape, weight shape, stride, pad, pad type, up-sample, add given)."""
    cin, cout, k, stride, pad, pt, ups, act, b, h, w = layer.case
    return ((b, cin, h, w), (cout, cin, layer.kd, layer.kd), stride, pad, pt, bool(ups), layer.add)
