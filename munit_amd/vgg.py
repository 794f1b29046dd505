"""The frozen VGG16 of the domain-invariant perceptual loss (vgg_w; scripts/networks.py:755-804, scripts/utils.py:1051-1063,
scripts/trainer.py:618-636).

`Vgg16` keeps the reference's module tree, so the file the reference's load_vgg16 would have written --
<vgg_model_path>/models/vgg16.weight, a torch.save of Vgg16().state_dict() with the keys conv1_1.weight ... conv5_3.bias --
loads with its own keys.  The reference's loader itself cannot run (it converts a Lua-torch file with load_lua, which torch no
longer has); here nothing is downloaded or converted: the user supplies that file.  The parameters are never trained.

The arithmetic runs on the device through the C ABI (munit_amd/ops.py): vgg_preprocess is ops.vgg_input, the thirteen 3x3
convolutions are ops.frozen_conv with the bias and the ReLU in the epilogue (forward and backward-data only), the three
2x2 max-pools are ops.maxpool2.  The first layer's three input channels need no padding: the forward runs on the
3-channels-as-4-channel-taps form of the implicit GEMM, its backward-data (64 -> 3) on the LDS-patch fold form.  As in the
reference there is NO pool between relu4_3 and conv5_1: relu5_3 has the extent of relu4_3, 1/8 of the image.
"""
import os

import torch
import torch.nn as nn

from . import ops

# (name, input channels, output channels) in forward order; a 2x2 max-pool follows the layers named in POOL_AFTER
LAYERS = (("conv1_1", 3, 64), ("conv1_2", 64, 64), ("conv2_1", 64, 128), ("conv2_2", 128, 128), ("conv3_1", 128, 256),
          ("conv3_2", 256, 256), ("conv3_3", 256, 256), ("conv4_1", 256, 512), ("conv4_2", 512, 512), ("conv4_3", 512, 512),
          ("conv5_1", 512, 512), ("conv5_2", 512, 512), ("conv5_3", 512, 512))
POOL_AFTER = ("conv1_2", "conv2_2", "conv3_3")
MIN_SIDE = 16      # three floor-halvings leave a 2x2 feature plane; on a single pixel the reference's InstanceNorm2d raises


def check_hw(h, w):
    """The image extents the loss takes: the feature plane (h // 8, w // 8) must hold more than one pixel per axis."""
    if h < MIN_SIDE or w < MIN_SIDE:
        raise ValueError("munit_amd: vgg_w > 0 needs images of at least %dx%d (the relu5_3 plane of a smaller one is a single "
                         "pixel, on which the reference's InstanceNorm2d raises); got %dx%d" % (MIN_SIDE, MIN_SIDE, h, w))


class Vgg16(nn.Module):
    """networks.py:755-804.  forward(*images) takes images in [-1, 1] (the generator's range), (B, 3, H, W) each, planar or
    channels_last, applies vgg_preprocess itself, runs all of them as one batch and returns relu5_3 as
    (sum of B, 512, H // 8, W // 8).  Sides that are not multiples of 8 follow the pools' floor."""

    def __init__(self):
        super().__init__()
        for name, cin, cout in LAYERS:
            setattr(self, name, nn.Conv2d(cin, cout, kernel_size=3, stride=1, padding=1))
        self._device_weights = None
        for p in self.parameters():
            p.requires_grad_(False)
        self.register_load_state_dict_post_hook(lambda m, _: m.invalidate())

    def invalidate(self):
        """Drop the cached device weights (after any write to the parameters)."""
        self._device_weights = None

    def _apply(self, fn, *args, **kwargs):
        self._device_weights = None
        return super()._apply(fn, *args, **kwargs)

    def weights(self, device):
        """{name: (w, b)} on `device`: fp32, the weights in channels_last memory."""
        if self._device_weights is not None and self._device_weights[0] == device:
            return self._device_weights[1]
        out = {}
        for name, _, _ in LAYERS:
            conv = getattr(self, name)
            out[name] = (conv.weight.detach().float().to(device).contiguous(memory_format=torch.channels_last),
                         conv.bias.detach().float().to(device).contiguous())
        self._device_weights = (device, out)
        return out

    def forward(self, *images):
        check_hw(*images[0].shape[2:])
        P = self.weights(images[0].device)
        x = ops.vgg_input(*images)
        for name, _, _ in LAYERS:
            w, b = P[name]
            x = ops.frozen_conv(x, w, b, w, stride=1, pad=1, act="relu", sink="vgg")
            if name in POOL_AFTER:
                x = ops.maxpool2(x, sink="vgg")
        return x


def load_vgg16(model_dir):
    """utils.py's load_vgg16(model_dir) without its download and conversion: a Vgg16 with the weights of
    os.path.join(model_dir, "vgg16.weight") (strict: a missing or unexpected key raises), in eval mode with every parameter
    frozen.  Loaded with weights_only; stays on the host, the device copy is made at first use."""
    path = os.path.join(model_dir, "vgg16.weight")
    if not os.path.isfile(path):
        raise FileNotFoundError("munit_amd: %s not found.  vgg_w > 0 needs the VGG16 weights as the reference caches them "
                                "(torch.save of networks.Vgg16().state_dict(), keys conv1_1.weight ... conv5_3.bias); nothing "
                                "is downloaded or converted here" % path)
    model = Vgg16()
    sd = torch.load(path, map_location="cpu", weights_only=True)
    model.load_state_dict(sd, strict=True)
    model.eval()
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def vgg_loss(model, x_trans, x_orig):
    """compute_vgg_loss (trainer.py:618-636) for several image pairs at once: x_trans / x_orig are lists of equal-sized
    batches (e.g. [x_ba, x_ab] and [x_b, x_a]).  The translations run the network as ONE batch with gradient, the originals
    as one batch without (no backward-data is spent on the targets); returns one loss per pair, each the mean over that
    pair's own features."""
    with torch.no_grad():
        target = model(*x_orig)
    sizes = [x.shape[0] for x in x_trans]
    if [x.shape[0] for x in x_orig] != sizes:
        raise ValueError("munit_amd.vgg_loss: the pairs' batch sizes differ (%s translations, %s originals)"
                         % (sizes, [x.shape[0] for x in x_orig]))
    feats = ops.split_batch(model(*x_trans), sizes)
    out, off = [], 0
    for f, n in zip(feats, sizes):
        out.append(ops.in_mse(f, target[off:off + n]))
        off += n
    return out
