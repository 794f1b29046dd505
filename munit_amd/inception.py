"""The Inception-v3 feature trunk of FID evaluation on HIP kernels (csrc/inception.hip through munit_amd.ops).

What the reference's WrapInception (scripts/inception_utils.py:27-85) runs of torchvision's inception_v3: the five stem
convolutions, two max pools, the eleven Mixed blocks -- everything up to the 8 x 8 x 2048 map; AuxLogits and fc are not part of
it.  Inference only, fp32, NHWC.  Every BasicConv2d (conv without bias, BatchNorm2d(eps=0.001) in eval mode, ReLU) is ONE
munit_conv2d_rect_fwd launch: the batch norm is folded into the weights on the host in fp64 and rounded to fp32 once.
The branches of a Mixed block write into the block's output buffer at their channel offsets (the per-pixel strides of the
kernels), so there is no concatenation and no copy anywhere in the trunk.

INCEPTION_CONVS is the architecture: 94 rows (name, Cin, Cout, KH, KW, stride, pad_h, pad_w) under torchvision's
state-dict names, 21,785,568 learnable parameters (torchvision's 27,161,264 less fc and AuxLogits)."""
import collections
import collections.abc

import torch

from . import ops

BN_EPS = 1e-3
IN_HW = 299
FEATURES = 2048


def _rows():
    rows = []

    def c(name, cin, cout, k=(1, 1), s=1, p=(0, 0)):
        rows.append((name, cin, cout, k[0], k[1], s, p[0], p[1]))

    c("Conv2d_1a_3x3", 3, 32, (3, 3), 2)
    c("Conv2d_2a_3x3", 32, 32, (3, 3))
    c("Conv2d_2b_3x3", 32, 64, (3, 3), p=(1, 1))
    c("Conv2d_3b_1x1", 64, 80)
    c("Conv2d_4a_3x3", 80, 192, (3, 3))
    for n, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        c(n + ".branch1x1", cin, 64)
        c(n + ".branch5x5_1", cin, 48)
        c(n + ".branch5x5_2", 48, 64, (5, 5), p=(2, 2))
        c(n + ".branch3x3dbl_1", cin, 64)
        c(n + ".branch3x3dbl_2", 64, 96, (3, 3), p=(1, 1))
        c(n + ".branch3x3dbl_3", 96, 96, (3, 3), p=(1, 1))
        c(n + ".branch_pool", cin, pf)
    c("Mixed_6a.branch3x3", 288, 384, (3, 3), 2)
    c("Mixed_6a.branch3x3dbl_1", 288, 64)
    c("Mixed_6a.branch3x3dbl_2", 64, 96, (3, 3), p=(1, 1))
    c("Mixed_6a.branch3x3dbl_3", 96, 96, (3, 3), 2)
    for n, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        c(n + ".branch1x1", 768, 192)
        c(n + ".branch7x7_1", 768, c7)
        c(n + ".branch7x7_2", c7, c7, (1, 7), p=(0, 3))
        c(n + ".branch7x7_3", c7, 192, (7, 1), p=(3, 0))
        c(n + ".branch7x7dbl_1", 768, c7)
        c(n + ".branch7x7dbl_2", c7, c7, (7, 1), p=(3, 0))
        c(n + ".branch7x7dbl_3", c7, c7, (1, 7), p=(0, 3))
        c(n + ".branch7x7dbl_4", c7, c7, (7, 1), p=(3, 0))
        c(n + ".branch7x7dbl_5", c7, 192, (1, 7), p=(0, 3))
        c(n + ".branch_pool", 768, 192)
    c("Mixed_7a.branch3x3_1", 768, 192)
    c("Mixed_7a.branch3x3_2", 192, 320, (3, 3), 2)
    c("Mixed_7a.branch7x7x3_1", 768, 192)
    c("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), p=(0, 3))
    c("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), p=(3, 0))
    c("Mixed_7a.branch7x7x3_4", 192, 192, (3, 3), 2)
    for n, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        c(n + ".branch1x1", cin, 320)
        c(n + ".branch3x3_1", cin, 384)
        c(n + ".branch3x3_2a", 384, 384, (1, 3), p=(0, 1))
        c(n + ".branch3x3_2b", 384, 384, (3, 1), p=(1, 0))
        c(n + ".branch3x3dbl_1", cin, 448)
        c(n + ".branch3x3dbl_2", 448, 384, (3, 3), p=(1, 1))
        c(n + ".branch3x3dbl_3a", 384, 384, (1, 3), p=(0, 1))
        c(n + ".branch3x3dbl_3b", 384, 384, (3, 1), p=(1, 0))
        c(n + ".branch_pool", cin, 192)
    return tuple(rows)


INCEPTION_CONVS = _rows()
_ROW = {r[0]: r for r in INCEPTION_CONVS}
BN_KEYS = ("weight", "bias", "running_mean", "running_var")


def parameter_count():
    """Learnable parameters of the table: the conv weights and the batch norms' gamma and beta."""
    return sum(cout * cin * kh * kw + 2 * cout for _, cin, cout, kh, kw, _, _, _ in INCEPTION_CONVS)


def out_extent(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


# ---- the launch plan ---------------------------------------------------------------------------------------------------
# Activations live in four flat buffers ("slots"): p and q, which the stem and the blocks alternate between, and t0 / t1 for
# what a branch keeps between its layers.  Ref names a channel slice [lo, lo + c) of an h x w x ctot map held in a slot.
Ref = collections.namedtuple("Ref", "slot h w ctot lo c")
Step = collections.namedtuple("Step", "kind arg src dst")      # kind "conv": arg = row name; "max" / "avg": arg = (stride, pad)


class _Builder(object):
    def __init__(self):
        self.steps, self.slots = [], collections.OrderedDict()

    def _dst(self, slot, h, w, c, ctot, lo):
        ctot = c if ctot is None else ctot
        self.slots[slot] = max(self.slots.get(slot, 0), h * w * ctot)
        return Ref(slot, h, w, ctot, lo, c)

    def conv(self, name, src, slot, ctot=None, lo=0):
        _, cin, cout, kh, kw, s, ph, pw = _ROW[name]
        assert cin == src.c and slot != src.slot, name
        dst = self._dst(slot, out_extent(src.h, kh, s, ph), out_extent(src.w, kw, s, pw), cout, ctot, lo)
        self.steps.append(Step("conv", name, src, dst))
        return dst

    def pool(self, kind, stride, pad, src, slot, ctot=None, lo=0):
        assert slot != src.slot
        dst = self._dst(slot, out_extent(src.h, 3, stride, pad), out_extent(src.w, 3, stride, pad), src.c, ctot, lo)
        self.steps.append(Step(kind, (stride, pad), src, dst))
        return dst

    def whole(self, ref):
        assert ref.lo + ref.c == ref.ctot
        return Ref(ref.slot, ref.h, ref.w, ref.ctot, 0, ref.ctot)


def _other(slot):
    return "q" if slot == "p" else "p"


def build_plan():
    """(steps, slot sizes in floats per image, block outputs): the trunk on a (299, 299, 3) map in slot "in".  `outputs`
    maps each stage name to the Ref of its whole output, for the shape chain the tests check."""
    b = _Builder()
    outs = collections.OrderedDict()
    x = Ref("in", IN_HW, IN_HW, 3, 0, 3)
    for name in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3", "max", "Conv2d_3b_1x1", "Conv2d_4a_3x3", "max"):
        slot = "p" if x.slot == "in" else _other(x.slot)
        x = b.pool("max", 2, 0, x, slot) if name == "max" else b.conv(name, x, slot)
        outs[name if name != "max" else "maxpool%d" % (1 if "maxpool1" not in outs else 2)] = x
    for n, pf in (("Mixed_5b", 32), ("Mixed_5c", 64), ("Mixed_5d", 64)):
        o, ct = _other(x.slot), 224 + pf
        b.conv(n + ".branch1x1", x, o, ct, 0)
        t = b.conv(n + ".branch5x5_1", x, "t0")
        b.conv(n + ".branch5x5_2", t, o, ct, 64)
        t = b.conv(n + ".branch3x3dbl_1", x, "t0")
        t = b.conv(n + ".branch3x3dbl_2", t, "t1")
        b.conv(n + ".branch3x3dbl_3", t, o, ct, 128)
        t = b.pool("avg", 1, 1, x, "t0")
        x = outs[n] = b.whole(b.conv(n + ".branch_pool", t, o, ct, 224))
    n, o = "Mixed_6a", _other(x.slot)
    b.conv(n + ".branch3x3", x, o, 768, 0)
    t = b.conv(n + ".branch3x3dbl_1", x, "t0")
    t = b.conv(n + ".branch3x3dbl_2", t, "t1")
    b.conv(n + ".branch3x3dbl_3", t, o, 768, 384)
    x = outs[n] = b.whole(b.pool("max", 2, 0, x, o, 768, 480))
    for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        o = _other(x.slot)
        b.conv(n + ".branch1x1", x, o, 768, 0)
        t = b.conv(n + ".branch7x7_1", x, "t0")
        t = b.conv(n + ".branch7x7_2", t, "t1")
        b.conv(n + ".branch7x7_3", t, o, 768, 192)
        t = b.conv(n + ".branch7x7dbl_1", x, "t0")
        t = b.conv(n + ".branch7x7dbl_2", t, "t1")
        t = b.conv(n + ".branch7x7dbl_3", t, "t0")
        t = b.conv(n + ".branch7x7dbl_4", t, "t1")
        b.conv(n + ".branch7x7dbl_5", t, o, 768, 384)
        t = b.pool("avg", 1, 1, x, "t0")
        x = outs[n] = b.whole(b.conv(n + ".branch_pool", t, o, 768, 576))
    n, o = "Mixed_7a", _other(x.slot)
    t = b.conv(n + ".branch3x3_1", x, "t0")
    b.conv(n + ".branch3x3_2", t, o, 1280, 0)
    t = b.conv(n + ".branch7x7x3_1", x, "t0")
    t = b.conv(n + ".branch7x7x3_2", t, "t1")
    t = b.conv(n + ".branch7x7x3_3", t, "t0")
    b.conv(n + ".branch7x7x3_4", t, o, 1280, 320)
    x = outs[n] = b.whole(b.pool("max", 2, 0, x, o, 1280, 512))
    for n in ("Mixed_7b", "Mixed_7c"):
        o = _other(x.slot)
        b.conv(n + ".branch1x1", x, o, 2048, 0)
        t = b.conv(n + ".branch3x3_1", x, "t0")
        b.conv(n + ".branch3x3_2a", t, o, 2048, 320)
        b.conv(n + ".branch3x3_2b", t, o, 2048, 704)
        t = b.conv(n + ".branch3x3dbl_1", x, "t0")
        t = b.conv(n + ".branch3x3dbl_2", t, "t1")
        b.conv(n + ".branch3x3dbl_3a", t, o, 2048, 1088)
        b.conv(n + ".branch3x3dbl_3b", t, o, 2048, 1472)
        t = b.pool("avg", 1, 1, x, "t0")
        x = outs[n] = b.whole(b.conv(n + ".branch_pool", t, o, 2048, 1856))
    assert sorted(s.arg for s in b.steps if s.kind == "conv") == sorted(_ROW), "every row of the table runs exactly once"
    return tuple(b.steps), dict(b.slots), outs


# ---- weights -----------------------------------------------------------------------------------------------------------
def fold_bn(w, gamma, beta, mean, var, eps=BN_EPS):
    """Conv (no bias) followed by an eval-mode batch norm as one conv with a bias, in fp64:
    w' = w * gamma / sqrt(var + eps) per output channel, b' = beta - mean * gamma / sqrt(var + eps)."""
    w, gamma, beta, mean, var = (t.detach().to(device="cpu", dtype=torch.float64) for t in (w, gamma, beta, mean, var))
    scale = gamma / torch.sqrt(var + eps)
    return w * scale.view(-1, 1, 1, 1), beta - mean * scale


def _state_dict_of(net):
    if isinstance(net, collections.abc.Mapping):
        return net
    if callable(getattr(net, "state_dict", None)):
        return net.state_dict()
    raise TypeError("munit_amd.inception: a state dict or an object with .state_dict() is expected, got %r" % type(net))


class InceptionV3(object):
    """The trunk with its weights: InceptionV3(state_dict)(pixels) maps (B, 299, 299, 3) normalised pixels (what
    ops.inception_input returns) to the (B, 8, 8, 2048) output of Mixed_7c.

    state_dict: a mapping (or an object with .state_dict(), such as torchvision's module) holding `<name>.conv.weight` and
    `<name>.bn.{weight,bias,running_mean,running_var}` for every row of INCEPTION_CONVS -- torchvision's layout.  AuxLogits.*,
    fc.* and *.num_batches_tracked are ignored.  A missing key raises KeyError naming it, a wrong shape ValueError.  The
    batch norms are folded here, on the host in fp64, and rounded to fp32 once; the images go to a device when the trunk first
    runs there.  The object owns the launch plan and, per device, one set of activation buffers sized for the largest
    batch it has seen (smaller batches run in their heads) plus the prepared launches of each batch size."""

    def __init__(self, state_dict):
        sd = _state_dict_of(state_dict)
        self._host = {}
        for name, cin, cout, kh, kw, _, _, _ in INCEPTION_CONVS:
            keys = [name + ".conv.weight"] + [name + ".bn." + k for k in BN_KEYS]
            for k, shape in zip(keys, [(cout, cin, kh, kw)] + [(cout,)] * 4):
                if k not in sd:
                    raise KeyError(k)
                if tuple(sd[k].shape) != shape:
                    raise ValueError("munit_amd.inception: %s has shape %s, the architecture needs %s"
                                     % (k, tuple(sd[k].shape), shape))
            w, bias = fold_bn(*(sd[k] for k in keys))
            self._host[name] = (ops.rect_weight_image(w.float()), bias.float().contiguous())
        self.steps, self.slot_floats, self.outputs = build_plan()
        self._dev, self._flat, self._bufs = {}, {}, {}

    @staticmethod
    def _device(device):
        """torch.device with its index spelled out: "cuda" and "cuda:0" are one key."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        return device

    def _params(self, device):
        if device not in self._dev:
            self._dev[device] = {n: (w.to(device), b.to(device)) for n, (w, b) in self._host.items()}
        return self._dev[device]

    def _buffers(self, device, batch):
        """The five flat activation buffers of a device, sized for the largest batch seen there (12.4 MB per image:
        0.4 GB at B = 32); a smaller batch -- a loader's short last one -- takes views of their heads.  Growing them drops
        the launches prepared on the old ones."""
        have = self._flat.get(device)
        if have is None or have[0] < batch:
            sizes = dict(self.slot_floats, **{"in": IN_HW * IN_HW * 3})
            for key in [k for k in self._bufs if k[0] == device]:
                del self._bufs[key]
            self._flat[device] = have = None          # release the old set before the new one is taken
            have = self._flat[device] = (batch, {s: torch.empty(batch * n, dtype=torch.float32, device=device)
                                                 for s, n in sizes.items()})
        return have[1]

    def _launches(self, device, batch):
        """(the input buffer, the launches of the plan's steps, the view of the final map) for this device and batch size:
        views and descriptors are made once per batch size (host memory only), a forward pass is then one C call per
        step."""
        device = self._device(device)
        key = (device, batch)
        if key not in self._bufs:
            params = self._params(device)
            flat = self._buffers(device, batch)

            def view(r):
                return flat[r.slot][:batch * r.h * r.w * r.ctot].view(batch, r.h, r.w, r.ctot)[..., r.lo:r.lo + r.c]

            launches = []
            for s in self.steps:
                if s.kind == "conv":
                    _, _, _, kh, kw, st, ph, pw = _ROW[s.arg]
                    w, bias = params[s.arg]
                    launches.append(ops.conv2d_rect_launch(view(s.src), w, bias, kh, kw, st, ph, pw, relu=True, out=view(s.dst))[0])
                else:
                    launches.append(ops.window3_launch(view(s.src), s.kind, s.arg[0], s.arg[1], out=view(s.dst))[0])
            self._bufs[key] = (flat["in"][:batch * IN_HW * IN_HW * 3].view(batch, IN_HW, IN_HW, 3), launches,
                               view(self.outputs["Mixed_7c"]))
        return self._bufs[key]

    def input_buffer(self, device, batch):
        """The (B, 299, 299, 3) buffer the trunk reads for this batch size: what ops.inception_input can write into."""
        return self._launches(device, batch)[0]

    def __call__(self, pixels):
        if pixels.dim() != 4 or tuple(pixels.shape[1:]) != (IN_HW, IN_HW, 3):
            raise RuntimeError("munit_amd.inception: (B, 299, 299, 3) pixels are expected, got %s" % (tuple(pixels.shape),))
        own, launches, result = self._launches(pixels.device, pixels.shape[0])
        if pixels.data_ptr() != own.data_ptr():
            own.copy_(pixels)            # pixels from elsewhere: into the buffer the plan was built on
        for launch in launches:
            launch()
        return result           # the trunk's own buffer: valid until the trunk next runs on this device
