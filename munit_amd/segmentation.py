"""The frozen Resnet34_8s of the semantic-consistency loss (scripts/utils.py:933-983, scripts/resnet.py,
scripts/trainer.py:136-142 and 706-771).

`Resnet34_8s` keeps the reference's module tree, so a checkpoint written by the reference loads with its own keys
(`resnet34_8s.conv1.weight`, `resnet34_8s.layer3.0.downsample.1.running_var`, ...).  Its parameters are never trained.
The arithmetic runs on the device through the C ABI (munit_amd/ops.py):

  - every BatchNorm (eval mode, eps 1e-5) is folded into the preceding convolution once, in fp64:
    w * gamma / sqrt(var + eps) and beta - mean * gamma / sqrt(var + eps);
  - the dilated 3x3 convolutions of layer3 (dilation 2) and layer4 (dilation 4) run undilated on phase images: the
    activations are re-laid out once after layer2 and once after layer3 (munit_space_to_batch, f = 2 each time), every
    3x3 then is a pad-1 convolution on a (H/16)^2 or (H/32)^2 image, and the 19-channel logits are laid back out;
  - backward-data of the odd-kernel stride-2 layers (conv1 7x7, layer2.0.conv1 3x3, layer2.0.downsample 1x1) multiplies
    by the filter zero-extended to 8x8 / 4x4 / 2x2: on even inputs the same output extent and the same result, in the
    phase form the backward-data kernels need.

Images must be square with a side that is a multiple of 32 (the logits then split into 4 x 4 phases of even size).

`SegmentationHead` is the trainable head of adaptation.sem_seg_lambda (scripts/trainer.py:203-223, 1286-1324): the
checkpoint's layer4 with its BatchNorms unfolded and in training mode, the 7x7 average the reference keeps, and a fresh
1x1 scoring layer of 10 classes, on a content code.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import networks, ops

NUM_CLASSES = 19
BN_EPS = 1e-5
# Cityscapes train-id palette of decode_segmap (scripts/utils.py:986-1020)
PALETTE = ((128, 64, 128), (244, 35, 232), (70, 70, 70), (102, 102, 156), (190, 153, 153), (153, 153, 153),
           (250, 170, 30), (220, 220, 0), (107, 142, 35), (152, 251, 152), (70, 130, 180), (220, 20, 60), (255, 0, 0),
           (0, 0, 142), (0, 0, 70), (0, 60, 100), (0, 80, 100), (0, 0, 230), (119, 11, 32))


class BasicBlock(nn.Module):
    """Parameter holder with resnet.py's BasicBlock keys (conv1, bn1, conv2, bn2, downsample.{0,1})."""

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=False):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, dilation, dilation=dilation, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, dilation, dilation=dilation, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.stride = stride
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))
        else:
            self.downsample = None


class ResNet34FullyConv(nn.Module):
    """resnet34(fully_conv=True, output_stride=8, remove_avg_pool_layer=True) with a 1x1 scoring conv as `fc`."""

    def __init__(self, num_classes):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        cfg = ((64, 3, 1, 1), (128, 4, 2, 1), (256, 6, 1, 2), (512, 3, 1, 4))   # planes, blocks, stride, dilation
        inplanes = 64
        for li, (planes, n, stride, dil) in enumerate(cfg):
            blocks = []
            for i in range(n):
                ds = i == 0 and (stride != 1 or inplanes != planes)
                blocks.append(BasicBlock(inplanes, planes, stride if i == 0 else 1, dil, ds))
                inplanes = planes
            setattr(self, "layer%d" % (li + 1), nn.Sequential(*blocks))
        self.fc = nn.Conv2d(512, num_classes, 1)


def fold_bn(weight, bn):
    """(w, b) of conv + eval-mode BatchNorm as one conv, in fp64."""
    w = weight.detach().double()
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + BN_EPS)
    return w * scale.view(-1, 1, 1, 1), bn.bias.detach().double() - bn.running_mean.detach().double() * scale


def _even(w):
    """zero-extend an odd kernel to the next even size (bottom / right): backward-data of a stride-2 layer"""
    kh, kw = w.shape[2:]
    return F.pad(w, (0, kw % 2, 0, kh % 2))


class Resnet34_8s(nn.Module):
    """utils.py:936-972.  forward(*images) takes images in [-1, 1] (the generator's range), applies seg_transform of
    (x + 1) / 2 itself, runs all images as one batch and returns the 1/8-resolution logits (B, 19, H/8, W/8); the
    bilinear up-sample to (H, W) lives in the head kernels (seg_loss, seg_labels), which evaluate it on the fly.
    Constructing it fetches nothing: weights come from load_segmentation_model."""

    def __init__(self, num_classes=NUM_CLASSES):
        super().__init__()
        if num_classes != NUM_CLASSES:
            raise ValueError("munit_amd: the segmentation head has %d classes (Cityscapes train ids), got %d"
                             % (NUM_CLASSES, num_classes))
        self.resnet34_8s = ResNet34FullyConv(num_classes)
        self._folded = None
        for p in self.parameters():
            p.requires_grad_(False)
        self.register_load_state_dict_post_hook(lambda m, _: m.invalidate())

    def invalidate(self):
        """Drop the folded device weights (after any write to the parameters or buffers)."""
        self._folded = None

    def _apply(self, fn, *args, **kwargs):
        self._folded = None
        return super()._apply(fn, *args, **kwargs)

    def folded(self, device):
        """{name: (w, b, w_dgrad)} on `device`: BN-folded fp32 weights (channels_last) and their backward-data images."""
        if self._folded is not None and self._folded[0] == device:
            return self._folded[1]
        net = self.resnet34_8s

        def put(w, b, stride):
            w32 = w.float().to(device).contiguous(memory_format=torch.channels_last)
            wd = _even(w).float().to(device).contiguous(memory_format=torch.channels_last) if stride == 2 else w32
            return w32, b.float().to(device), wd

        out = {"conv1": put(*fold_bn(net.conv1.weight, net.bn1), 2)}
        for li in range(1, 5):
            for i, blk in enumerate(getattr(net, "layer%d" % li)):
                name = "layer%d.%d" % (li, i)
                out[name + ".conv1"] = put(*fold_bn(blk.conv1.weight, blk.bn1), blk.stride)
                out[name + ".conv2"] = put(*fold_bn(blk.conv2.weight, blk.bn2), 1)
                if blk.downsample is not None:
                    out[name + ".downsample"] = put(*fold_bn(blk.downsample[0].weight, blk.downsample[1]), blk.stride)
        out["fc"] = put(net.fc.weight.detach().double(), net.fc.bias.detach().double(), 1)
        self._folded = (device, out)
        return out

    def forward(self, *images):
        x0 = images[0]
        h, w = x0.shape[2:]
        if h != w or h % 32:
            raise ValueError("munit_amd: the segmentation network needs square images with a side that is a multiple of "
                             "32, got %dx%d" % (h, w))
        P = self.folded(x0.device)
        x = ops.seg_input(*images)
        x = ops.frozen_conv(x, *P["conv1"], stride=2, pad=3, act="relu")
        x = ops.maxpool3s2(x)
        net = self.resnet34_8s
        for li in range(1, 5):
            if li >= 3:          # dilation 2, then 4: split every image into 2 x 2 phases once more
                x = ops.space_to_batch(x, 2)
            for i, blk in enumerate(getattr(net, "layer%d" % li)):
                x = self._block(x, P, "layer%d.%d" % (li, i), blk.stride, blk.downsample is not None)
        x = ops.frozen_conv(x, *P["fc"], stride=1, pad=0)
        x = ops.space_to_batch(x, 2, inverse=True)
        return ops.space_to_batch(x, 2, inverse=True)

    @staticmethod
    def _block(x, P, name, stride, has_ds):
        link = ops.ResidualLink()
        hid = ops.frozen_conv(x, *P[name + ".conv1"], stride=stride, pad=1, act="relu", link_in=link)
        out = ops.frozen_conv(hid, *P[name + ".conv2"], stride=1, pad=1)
        if has_ds:
            # created after conv1: its backward runs first and parks the gradient that conv1's backward-data adds
            res = ops.frozen_conv(x, *P[name + ".downsample"], stride=stride, pad=0, link_out=link)
            return ops.add_relu(out, res)
        return ops.add_relu(out, x, link=link)


def load_segmentation_model(ckpt_path, classes):
    """utils.py:974-983: a Resnet34_8s with the checkpoint's weights (strict: a missing or unexpected key raises), in
    eval mode with every parameter frozen.  Loaded with weights_only; stays on the host until moved."""
    model = Resnet34_8s(num_classes=classes)
    sd = torch.load(ckpt_path, map_location="cpu", weights_only=True)
    model.load_state_dict(sd, strict=True)
    model.eval()
    for p in model.parameters():
        p.requires_grad_(False)
    return model


HEAD_CLASSES = 10      # the simulator's classes (nn.Conv2d(512, 10, kernel_size=1), trainer.py:207)


class AvgPool7(nn.Module):
    """nn.AvgPool2d(7, padding=3, stride=1) of scripts/resnet.py: no parameters, the divisor is always 49."""

    def forward(self, x):
        return ops.avgpool7(x)


class SegmentationHead(nn.Sequential):
    """Sequential(layer4, avgpool, Conv2d(512, 10, 1)) (trainer.py:207-210) with the reference's state_dict keys:
    0.{0,1,2}.conv1.weight, 0.*.bn{1,2}.*, 0.0.downsample.{0.weight,1.*}, 2.weight, 2.bias.  Every parameter trains; the
    seven BatchNorms normalise with batch statistics and move their running statistics while the module is in training
    mode (networks.BatchNorm2d).

    forward(code): the (B, 256, h, w) content code is split into its 4 x 4 phases once (munit_space_to_batch, f = 4), on
    which layer4's dilation-4 3x3 convolutions are undilated pad-1 ones; batch statistics do not depend on the layout.
    The inverse re-layout, the 7x7 average and the scoring layer follow in the reference's order.  h and w must be
    multiples of 4.  Returns the (B, 10, h, w) logits; the bilinear up-sample lives in ops.seg_cross_entropy_direct.
    The ReLU sign patterns go to ops.DANN_SINK in call order (the blocks are the feature classifier's BasicBlock)."""

    def __init__(self, num_classes=HEAD_CLASSES):
        blocks = [networks.BasicBlock(256, 512), networks.BasicBlock(512, 512), networks.BasicBlock(512, 512)]
        super().__init__(nn.Sequential(*blocks), AvgPool7(), networks.Conv2d(512, num_classes, 1))

    @staticmethod
    def check_code_hw(h, w):
        if h % 4 or w % 4 or h < 4 or w < 4:
            raise ValueError("munit_amd.SegmentationHead: a %dx%d content code does not split into 4 x 4 phases (layer4's "
                             "dilation); both extents must be multiples of 4" % (h, w))

    def forward(self, code):
        x = ops.nhwc(code)
        if x.dim() != 4 or x.shape[1] != 256:
            raise ValueError("munit_amd.SegmentationHead: a (B, 256, h, w) content code expected, got %s" % (tuple(x.shape),))
        self.check_code_hw(x.shape[2], x.shape[3])
        x = ops.space_to_batch(x, 4)
        for blk in self[0]:
            x = blk(x)
        x = ops.space_to_batch(x, 4, inverse=True)
        return self[2](self[1](x))


def load_segmentation_head(ckpt_path, num_classes=HEAD_CLASSES):
    """trainer.py:203-214: the layer4 of the user's Resnet34_8s checkpoint (loaded strictly, with weights_only, as
    load_segmentation_model does) under a scoring layer drawn from nn.Conv2d(512, 10, 1)'s distribution.  Trainable and
    in training mode; stays on the host until moved."""
    pretrained = load_segmentation_model(ckpt_path, NUM_CLASSES)
    head = SegmentationHead(num_classes)
    head[0].load_state_dict(pretrained.resnet34_8s.layer4.state_dict(), strict=True)
    for p in head.parameters():
        p.requires_grad_(True)
    return head


def seg_head_loss(head, c_a, c_b, target_a, target_b, scale):
    """trainer.py:1303-1317: CE(up(head(c_a)), target_a) + CE(up(head(c_b)), target_b) -- two forwards of the head, a then
    b, each with its own batch statistics.  targets: float32 (B, H, W) at the crop size."""
    l_a = ops.seg_cross_entropy_direct(head(c_a), target_a, scale)
    l_b = ops.seg_cross_entropy_direct(head(c_b), target_b, scale)
    return ops.scalar_sum([l_a, l_b])


def seg_loss(model, x_orig, x_trans, mask=None, gt=None):
    """compute_semantic_seg_loss (trainer.py:706-771) summed over image pairs: x_orig / x_trans are lists of equal-sized
    batches (e.g. [x_a, x_b] and [x_ab, x_ba]); returns sum over pairs of the mean cross-entropy between the logits of
    x_trans[i] and the pseudo-labels of x_orig[i] (argmax of the network's output, no gradient).  mask: None (plain
    19-class loss) or one tensor of 0/1 values covering all pairs' pixels in order (the masked 20-class loss).
    gt: a ground-truth map of the simulator's 10 classes covering all pairs' pixels in order (float32, values 0..9).
    With it the label pass over x_orig is skipped, as the reference skips it (trainer.py:733-741), and the logits are
    merged into 10 classes (11 with a mask) inside the head kernel; the labels returned are None."""
    b, _, h, w = x_trans[0].shape
    if gt is not None:
        return ops.seg_cross_entropy_gt(model(*x_trans), gt, mask, scale=8, norm=b * h * w), None
    with torch.no_grad():
        labels = ops.seg_labels(model(*x_orig))
    logits = model(*x_trans)
    return ops.seg_cross_entropy(logits, labels, mask, scale=8, norm=b * h * w), labels


def colorize(labels):
    """decode_segmap + ToTensor (trainer.py:870-900): int labels (B, H, W) -> (B, 3, H, W) float in [0, 1], on the
    labels' device (host code: a display path)."""
    pal = torch.tensor(PALETTE, dtype=torch.uint8)
    rgb = pal[labels.detach().long().cpu()]                  # (B, H, W, 3) uint8
    return (rgb.permute(0, 3, 1, 2).float() / 255.0).to(labels.device)
