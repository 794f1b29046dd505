"""MI355X-native AdaINGen / AdaINGen_double / MsImageDis.

Same class names, constructor arguments, method names and state_dict key layout as the
reference's scripts/networks.py so checkpoints and callers
(scripts/train.py, scripts/test.py) interchange -- but nothing here calls a torch compute
op: every layer dispatches to the HIP kernels through munit_amd.ops, activations stay NHWC
in HBM between kernels, the upsample of the decoder is folded into the following
convolution's gather, bias/activation ride in the conv epilogue, ReLU and the ResBlock
residual add ride in the normalisation kernels, and the AdaIN parameters are read straight
out of the MLP output by column offset.

Parameters are ordinary nn.Parameters of the reference's shapes (OIHW) stored
channels_last; default initialisation consumes the torch RNG exactly like nn.Conv2d /
nn.Linear so `torch.manual_seed(s)` reproduces the reference's initial weights.
"""
import math
import os

import torch
from torch import nn
from torch.nn import init

from . import ops


# --------------------------------------------------------------------------------------
# leaf layers
# --------------------------------------------------------------------------------------
class Conv2d(nn.Module):
    """Stands in for nn.Conv2d (un-padded, networks.py:691-693 / :68 / :472).  Parameter
    names `weight` (O, I, k, k) and `bias` (O,) as in torch."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride = kernel_size, stride
        w = torch.empty(out_channels, in_channels, kernel_size, kernel_size)
        init.kaiming_uniform_(w, a=math.sqrt(5))  # nn.Conv2d.reset_parameters
        self.weight = nn.Parameter(w.contiguous(memory_format=torch.channels_last))
        if bias:
            fan_in = in_channels * kernel_size * kernel_size
            bound = 1 / math.sqrt(fan_in) if fan_in > 0 else 0
            self.bias = nn.Parameter(torch.empty(out_channels).uniform_(-bound, bound))
        else:
            self.register_parameter("bias", None)

    def forward(self, x, pad=0, pad_type="zero", upsample=False, act="none", slope=0.2, out_dtype=None, link=None):
        return ops.conv2d(x, self.weight, self.bias, self.stride, pad, pad_type, upsample, act, slope, out_dtype, link)

    def extra_repr(self):
        return "%d, %d, kernel_size=%d, stride=%d" % (self.in_channels, self.out_channels, self.kernel_size,
                                                      self.stride)


def l2normalize(v, eps=1e-12):
    """networks.py:881-882."""
    return v / (v.norm() + eps)


class SpectralNorm(nn.Module):
    """networks.py:885-942 around a Conv2d (power_iterations 1, the reference's only use).  State as in the reference: the
    wrapped module owns `bias`, `weight_u` (O,), `weight_v` (I * kh * kw, in the reference's (i, kh, kw) column order) and
    `weight_bar` (O, I, kh, kw), in that order, and no `weight` -- so weights_init passes these layers by, as it does there
    (the reference's inner convolution has no `weight` attribute before its first forward).  weight_u / weight_v take no
    gradient and are drawn after the convolution's own parameters: u ~ N(0, 1), then v, both l2-normalised.

    Every forward advances u and v by one power iteration, also under no_grad and in eval(), and runs
    act(conv(pad(x), weight_bar) / sigma + bias): the convolution kernels and their prepared weight images see weight_bar
    alone.  The owner of several wrappers (MsImageDis) iterates all of them in one call and hands each its slot through
    `assign`; a wrapper called on its own iterates itself."""

    def __init__(self, module):
        super().__init__()
        if not isinstance(module, Conv2d):
            raise NotImplementedError("munit_amd.SpectralNorm wraps a munit_amd Conv2d (LinearBlock's norm='sn' is not "
                                      "reachable from any config)")
        self.module = module
        w = module.weight
        height, width = w.shape[0], w[0].numel()
        u = nn.Parameter(l2normalize(torch.empty(height).normal_(0, 1)), requires_grad=False)
        v = nn.Parameter(l2normalize(torch.empty(width).normal_(0, 1)), requires_grad=False)
        w_bar = nn.Parameter(w.data)
        del module._parameters["weight"]
        module.register_parameter("weight_u", u)
        module.register_parameter("weight_v", v)
        module.register_parameter("weight_bar", w_bar)
        self.__dict__["_inv_sigma"] = None       # this forward's 1 / sigma (a device scalar), set by assign()

    def layer(self):
        m = self.module
        return m.weight_bar, m.weight_u, m.weight_v

    def assign(self, inv_sigma):
        self.__dict__["_inv_sigma"] = inv_sigma

    def forward(self, x, pad=0, pad_type="zero", act="none", slope=0.2):
        m = self.module
        inv_sigma, self.__dict__["_inv_sigma"] = self._inv_sigma, None
        if inv_sigma is None:
            inv_sigma = ops.sn_power_iter(*ops.sn_table([self.layer()]))[1:2]
        raw = ops.conv2d(x, m.weight_bar, None, m.stride, pad, pad_type, False, "none")
        return ops.sn_act(raw, m.weight_bar, m.bias, m.weight_u, m.weight_v, inv_sigma, act, slope)


class Linear(nn.Module):
    """Stands in for nn.Linear (networks.py:712)."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        w = torch.empty(out_features, in_features)
        init.kaiming_uniform_(w, a=math.sqrt(5))  # nn.Linear.reset_parameters
        self.weight = nn.Parameter(w)
        if bias:
            bound = 1 / math.sqrt(in_features) if in_features > 0 else 0
            self.bias = nn.Parameter(torch.empty(out_features).uniform_(-bound, bound))
        else:
            self.register_parameter("bias", None)

    def forward(self, x, act="none"):
        return ops.linear(x, self.weight, self.bias, act)


class InstanceNorm2d(nn.Module):
    """nn.InstanceNorm2d(affine=False, track_running_stats=False) (networks.py:657): no state."""

    def __init__(self, num_features, eps=1e-5):
        super().__init__()
        self.num_features, self.eps = num_features, eps

    def forward(self, x, relu=False, residual=None, link=None):
        return ops.instance_norm(x, relu, residual, self.eps, link)


class AdaptiveInstanceNorm2d(nn.Module):
    """networks.py:810-848.  weight/bias are assigned per call by assign_adain_params; the
    dummy running_mean / running_var buffers exist only for state_dict compatibility."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1):
        super().__init__()
        self.num_features, self.eps, self.momentum = num_features, eps, momentum
        self.weight = None
        self.bias = None
        self._params = None  # (adain_params (B, n), weight column offset, bias column offset)
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))

    def forward(self, x, relu=False, residual=None, link=None):
        assert self.weight is not None and self.bias is not None, \
            "Please assign weight and bias before calling AdaIN!"
        sink, first = None, False
        if self._params is not None:
            params, w_off, b_off, sink, first = self._params
        else:
            # weight / bias assigned by hand as flat (B*C,) tensors (reference convention)
            b, c = x.size(0), x.size(1)
            params = torch.cat([self.bias.reshape(b, c), self.weight.reshape(b, c)], dim=1).contiguous()
            w_off, b_off = c, 0
        return ops.adain(x, params, w_off, b_off, relu, residual, self.eps, link, sink, first)

    def __repr__(self):
        return self.__class__.__name__ + "(" + str(self.num_features) + ")"


class LayerNorm(nn.Module):
    """networks.py:851-878 (unbiased std, eps added to std, per-channel gamma/beta)."""

    def __init__(self, num_features, eps=1e-5, affine=True):
        super().__init__()
        self.num_features, self.affine, self.eps = num_features, affine, eps
        if not affine:
            raise NotImplementedError("munit_amd.LayerNorm: affine=False is not on the MUNIT hot path")
        self.gamma = nn.Parameter(torch.Tensor(num_features).uniform_())
        self.beta = nn.Parameter(torch.zeros(num_features))

    def forward(self, x, relu=False):
        return ops.layer_norm(x, self.gamma, self.beta, relu, self.eps)


class Upsample2x(nn.Module):
    """Placeholder keeping nn.Upsample(scale_factor=2)'s slot in Decoder.model
    (networks.py:534); the decoder folds it into the next convolution's gather."""

    def forward(self, x):
        raise RuntimeError("Upsample2x is fused into the following Conv2dBlock; call Decoder.forward")


class _Pad(nn.Module):
    """Keeps the `pad` slot of Conv2dBlock (networks.py:642-649); the padding itself is index
    arithmetic inside the convolution kernels."""

    def __init__(self, kind, padding):
        super().__init__()
        self.kind, self.padding = kind, padding

    def extra_repr(self):
        return "%s, %d" % (self.kind, self.padding)


# --------------------------------------------------------------------------------------
# blocks
# --------------------------------------------------------------------------------------
class Conv2dBlock(nn.Module):
    """networks.py:627-701: activation(norm(conv(pad(x)))), bias always on."""

    def __init__(self, input_dim, output_dim, kernel_size, stride, padding=0, norm="none", activation="relu",
                 pad_type="zero"):
        super().__init__()
        self.use_bias = True
        if pad_type not in ("reflect", "zero"):
            assert pad_type != "replicate", "munit_amd: replicate padding is not implemented (not on the hot path)"
            assert 0, "Unsupported padding type: {}".format(pad_type)
        self.pad = _Pad(pad_type, padding)
        norm_dim = output_dim
        if norm == "in":
            self.norm = InstanceNorm2d(norm_dim)
        elif norm == "ln":
            self.norm = LayerNorm(norm_dim)
        elif norm == "adain":
            self.norm = AdaptiveInstanceNorm2d(norm_dim)
        elif norm == "none" or norm == "sn":
            self.norm = None
        elif norm == "bn":
            raise NotImplementedError("munit_amd: norm=%r is outside the MUNIT hot path (configs use none/in/ln/adain/sn)"
                                      % norm)
        else:
            assert 0, "Unsupported normalization: {}".format(norm)
        if activation not in ("relu", "lrelu", "tanh", "none"):
            if activation in ("prelu", "selu"):
                raise NotImplementedError("munit_amd: activation=%r is not implemented" % activation)
            assert 0, "Unsupported activation: {}".format(activation)
        self.activation = activation
        self.conv = Conv2d(input_dim, output_dim, kernel_size, stride, bias=self.use_bias)
        self.sn = norm == "sn"
        if self.sn:                 # networks.py:684-689: the convolution inside SpectralNorm, keys conv.module.*
            self.conv = SpectralNorm(self.conv)

    def forward(self, x, upsample=False, residual=None, out_dtype=None, link_open=None, link_close=None):
        """link_open / link_close: the ops.ResidualLink of the ResBlock this block opens (its convolution's backward-data
        adds the skip gradient) / closes (its norm's backward parks the skip gradient instead of returning it)."""
        if self.sn:
            if upsample or residual is not None or link_open is not None or (out_dtype not in (None, torch.float32)):
                raise NotImplementedError("munit_amd: a spectrally normalised block is a plain fp32 discriminator layer")
            return self.conv(x, self.pad.padding, self.pad.kind, self.activation)
        if self.norm is None:
            y = self.conv(x, self.pad.padding, self.pad.kind, upsample, self.activation, out_dtype=out_dtype, link=link_open)
            if residual is not None:
                raise NotImplementedError("munit_amd: residual add needs a normalised block")
            return y
        y = self.conv(x, self.pad.padding, self.pad.kind, upsample, "none", out_dtype=out_dtype, link=link_open)
        act = self.activation      # fused into the norm kernels' apply pass (forward and backward): none / relu / lrelu / tanh
        if isinstance(self.norm, LayerNorm):
            assert residual is None
            y = self.norm(y, act)
        else:
            assert residual is None or act == "none"      # out += residual closes a block whose activation is 'none' (networks.py:611-624)
            y = self.norm(y, act, residual, link_close)
        return y


class ResBlock(nn.Module):
    """networks.py:603-624; `out += residual` is fused into the second norm kernel."""

    def __init__(self, dim, norm="in", activation="relu", pad_type="zero"):
        super().__init__()
        model = [Conv2dBlock(dim, dim, 3, 1, 1, norm=norm, activation=activation, pad_type=pad_type),
                 Conv2dBlock(dim, dim, 3, 1, 1, norm=norm, activation="none", pad_type=pad_type)]
        self.model = nn.Sequential(*model)

    def forward(self, x):
        # x feeds the first convolution and the skip connection; in backward the two gradients meet inside that convolution's
        # backward-data (ops.ResidualLink) instead of in a separate element-wise add
        # (fp32 tensors only: the bf16-storage backward-data has no fused `add` on its folded path)
        link = ops.ResidualLink() if (torch.is_grad_enabled() and x.requires_grad and ops.FUSE_SKIP_GRAD and
                                      x.dtype == torch.float32) else None
        h = self.model[0](x, link_open=link)
        return self.model[1](h, residual=x, link_close=link)


class ResBlocks(nn.Module):
    """networks.py:569-580."""

    def __init__(self, num_blocks, dim, norm="in", activation="relu", pad_type="zero"):
        super().__init__()
        self.model = nn.Sequential(*[ResBlock(dim, norm=norm, activation=activation, pad_type=pad_type)
                                     for _ in range(num_blocks)])

    def forward(self, x):
        for blk in self.model:
            x = blk(x)
        return x


class LinearBlock(nn.Module):
    """networks.py:704-749 (norm 'none' only -- what MLP uses)."""

    def __init__(self, input_dim, output_dim, norm="none", activation="relu"):
        super().__init__()
        if norm != "none":
            raise NotImplementedError("munit_amd.LinearBlock: norm=%r is not on the MUNIT hot path" % norm)
        if activation not in ("relu", "lrelu", "tanh", "none"):
            raise NotImplementedError("munit_amd.LinearBlock: activation=%r is not implemented" % activation)
        self.fc = Linear(input_dim, output_dim, bias=True)
        self.norm = None
        self.activation = activation

    def forward(self, x):
        return self.fc(x, self.activation)


class MLP(nn.Module):
    """networks.py:583-597."""

    def __init__(self, input_dim, output_dim, dim, n_blk, norm="none", activ="relu"):
        super().__init__()
        model = [LinearBlock(input_dim, dim, norm=norm, activation=activ)]
        for _ in range(n_blk - 2):
            model += [LinearBlock(dim, dim, norm=norm, activation=activ)]
        model += [LinearBlock(dim, output_dim, norm="none", activation="none")]
        self.model = nn.Sequential(*model)

    def forward(self, x):
        h = x.reshape(x.size(0), -1)
        for blk in self.model:
            h = blk(h)
        return h


# --------------------------------------------------------------------------------------
# encoders / decoder
# --------------------------------------------------------------------------------------
class _GlobalAvgPool(nn.Module):
    def forward(self, x):
        return ops.global_avgpool(x)


class StyleEncoder(nn.Module):
    """networks.py:442-477."""

    def __init__(self, n_downsample, input_dim, dim, style_dim, norm, activ, pad_type):
        super().__init__()
        model = [Conv2dBlock(input_dim, dim, 7, 1, 3, norm=norm, activation=activ, pad_type=pad_type)]
        for _ in range(2):
            model += [Conv2dBlock(dim, 2 * dim, 4, 2, 1, norm=norm, activation=activ, pad_type=pad_type)]
            dim *= 2
        for _ in range(n_downsample - 2):
            model += [Conv2dBlock(dim, dim, 4, 2, 1, norm=norm, activation=activ, pad_type=pad_type)]
        model += [_GlobalAvgPool()]
        model += [Conv2d(dim, style_dim, 1, 1)]
        self.model = nn.Sequential(*model)
        self.output_dim = dim

    def forward(self, x):
        for m in self.model:
            x = m(x)
        return x


class ContentEncoder(nn.Module):
    """networks.py:480-512."""

    def __init__(self, n_downsample, n_res, input_dim, dim, norm, activ, pad_type):
        super().__init__()
        model = [Conv2dBlock(input_dim, dim, 7, 1, 3, norm=norm, activation=activ, pad_type=pad_type)]
        for _ in range(n_downsample):
            model += [Conv2dBlock(dim, 2 * dim, 4, 2, 1, norm=norm, activation=activ, pad_type=pad_type)]
            dim *= 2
        model += [ResBlocks(n_res, dim, norm=norm, activation=activ, pad_type=pad_type)]
        self.model = nn.Sequential(*model)
        self.output_dim = dim
        # build extension (`precision: bf16s`, BASELINE.json config #3): element type in which this encoder's
        # activations -- and through the content code everything the decoder computes up to its 3-channel image head --
        # live in HBM.  None = fp32, the reference's.  The 3-channel input image is always fp32.
        self.store_dtype = None
        # data-parallel exchange (trainer.GradExchange): when `keep_trunk_in` is set, the tensor entering the residual trunk is
        # left in `trunk_in` for the caller to hook (its gradient exists once every trunk weight gradient of this pass has been
        # issued); the caller takes it and clears both
        self.keep_trunk_in = False
        self.trunk_in = None

    def forward(self, x):
        last = len(self.model) - 1
        for i, m in enumerate(self.model):
            if i == last and self.keep_trunk_in:
                self.trunk_in = x
            x = m(x, out_dtype=self.store_dtype) if (i == 0 and self.store_dtype is not None) else m(x)
        return x


class Decoder(nn.Module):
    """networks.py:515-563."""

    def __init__(self, n_upsample, n_res, dim, output_dim, res_norm="adain", activ="relu", pad_type="zero"):
        super().__init__()
        model = [ResBlocks(n_res, dim, res_norm, activ, pad_type=pad_type)]
        for _ in range(n_upsample):
            model += [Upsample2x(),
                      Conv2dBlock(dim, dim // 2, 5, 1, 2, norm="ln", activation=activ, pad_type=pad_type)]
            dim //= 2
        model += [Conv2dBlock(dim, output_dim, 7, 1, 3, norm="none", activation="tanh", pad_type=pad_type)]
        self.model = nn.Sequential(*model)

    def forward(self, x):
        up = False
        for m in self.model:
            if isinstance(m, Upsample2x):
                up = True
            elif isinstance(m, Conv2dBlock):
                x = m(x, upsample=up)
                up = False
            else:
                x = m(x)
        return x


# --------------------------------------------------------------------------------------
# generators
# --------------------------------------------------------------------------------------
def _assign_adain_params(adain_params, model):
    """networks.py:230-239: AdaIN layer l (module order) takes bias = columns [2lC, 2lC+C),
    weight = [2lC+C, 2lC+2C).  Here the slices are column offsets into the one (B, n) tensor
    (read in place by the kernel); .weight / .bias are set to detached views so the
    reference's 'assigned?' assertion and introspection still work."""
    if adain_params.dim() != 2:
        adain_params = adain_params.reshape(adain_params.size(0), -1)
    adain_params = adain_params.contiguous()
    layers = model.__dict__.get("_munit_adain_layers")      # the walk over model.modules() costs ~0.1 ms: once per decoder
    if layers is None:
        layers = [m for m in model.modules() if m.__class__.__name__ == "AdaptiveInstanceNorm2d"]
        model.__dict__["_munit_adain_layers"] = layers
    # When the layers' column ranges tile the tensor exactly (the shipped geometry: the MLP emits get_num_adain_params
    # columns), their backward passes write their slices of ONE gradient buffer and the first layer hands it to autograd
    # (ops.AdainGradSink) -- instead of eight zero-filled (B, n) tensors summed by seven element-wise kernels per decode.
    exact = sum(2 * m.num_features for m in layers) == adain_params.size(1)
    sink = ops.AdainGradSink() if (exact and torch.is_grad_enabled() and adain_params.requires_grad and ops.FUSE_ADAIN_GRAD) else None
    off = 0
    det = adain_params.detach()
    for i, m in enumerate(layers):
        c = m.num_features
        d = m.__dict__                       # plain attributes (set to None in __init__): skip nn.Module.__setattr__'s type checks
        d["_params"] = (adain_params, off + c, off, sink, i == 0)
        d["bias"] = det[:, off:off + c]
        d["weight"] = det[:, off + c:off + 2 * c]
        if adain_params.size(1) > off + 2 * c:
            off += 2 * c


def _num_adain_params(model):
    """networks.py:241-247."""
    n = 0
    for m in model.modules():
        if m.__class__.__name__ == "AdaptiveInstanceNorm2d":
            n += 2 * m.num_features
    return n


class _ApplyRefreshesImages:
    """nn.Module.apply with a tail: the reference's weights_init writes through `m.weight.data` (utils.py:1093-1115), which
    bumps no version counter, so the prepared weight images kept with the parameters (ops._prepared) would go stale unseen.
    After any apply() on a network or on the trainer the optimizers that own its parameters rebuild their images (one launch
    each; nothing happens before the parameters are bound to a device buffer).  Before it, and before _apply() (.to(),
    .float(), ...) moves the weights, the same optimizers settle a step that is still in flight on another stream
    (FusedAdam.step_on)."""

    def _owners(self):
        """The optimizers that own this network's parameters."""
        opts = {}
        for p in self.parameters():
            o = getattr(p, "_munit_opt", None)
            if o is not None:
                opts[id(o)] = o
        return list(opts.values())

    def apply(self, fn):
        owners = self._owners()
        for o in owners:
            o.settle()
        out = super().apply(fn)
        for o in owners:
            o.invalidate_prepared()
        return out

    def _apply(self, fn, *args, **kwargs):
        for o in self._owners():
            o.settle()
        return super()._apply(fn, *args, **kwargs)


class AdaINGen(_ApplyRefreshesImages, nn.Module):
    """networks.py:170-254."""

    def __init__(self, input_dim, params):
        super().__init__()
        dim, style_dim = params["dim"], params["style_dim"]
        n_downsample, n_res = params["n_downsample"], params["n_res"]
        activ, pad_type, mlp_dim = params["activ"], params["pad_type"], params["mlp_dim"]
        self.enc_style = StyleEncoder(4, input_dim, dim, style_dim, norm="none", activ=activ, pad_type=pad_type)
        self.enc_content = ContentEncoder(n_downsample, n_res, input_dim, dim, "in", activ, pad_type=pad_type)
        self.dec = Decoder(n_downsample, n_res, self.enc_content.output_dim, input_dim, res_norm="adain",
                           activ=activ, pad_type=pad_type)
        self.mlp = MLP(style_dim, self.get_num_adain_params(self.dec), mlp_dim, 3, norm="none", activ=activ)

    def forward(self, images):
        content, style_fake = self.encode(images)
        return self.decode(content, style_fake)

    def encode(self, images):
        images = ops.nhwc(images)
        style_fake = self.enc_style(images)
        content = self.enc_content(images)
        return content, style_fake

    def decode(self, content, style):
        adain_params = self.mlp(style)
        self.assign_adain_params(adain_params, self.dec)
        return self.dec(content)

    def assign_adain_params(self, adain_params, model):
        _assign_adain_params(adain_params, model)

    def get_num_adain_params(self, model):
        return _num_adain_params(model)

    def get_adain_param(self, style):
        return self.mlp(style)


class AdaINGen_double(_ApplyRefreshesImages, nn.Module):
    """networks.py:262-388: one shared style encoder, two content encoders / decoders / MLPs."""

    def __init__(self, input_dim, params):
        super().__init__()
        dim, style_dim = params["dim"], params["style_dim"]
        n_downsample, n_res = params["n_downsample"], params["n_res"]
        activ, pad_type, mlp_dim = params["activ"], params["pad_type"], params["mlp_dim"]
        self.enc_style = StyleEncoder(4, input_dim, dim, style_dim, norm="none", activ=activ, pad_type=pad_type)
        self.enc1_content = ContentEncoder(n_downsample, n_res, input_dim, dim, "in", activ, pad_type=pad_type)
        self.enc2_content = ContentEncoder(n_downsample, n_res, input_dim, dim, "in", activ, pad_type=pad_type)
        self.dec1 = Decoder(n_downsample, n_res, self.enc1_content.output_dim, input_dim, res_norm="adain",
                            activ=activ, pad_type=pad_type)
        self.dec2 = Decoder(n_downsample, n_res, self.enc2_content.output_dim, input_dim, res_norm="adain",
                            activ=activ, pad_type=pad_type)
        self.mlp1 = MLP(style_dim, self.get_num_adain_params(self.dec1), mlp_dim, 3, norm="none", activ=activ)
        self.mlp2 = MLP(style_dim, self.get_num_adain_params(self.dec2), mlp_dim, 3, norm="none", activ=activ)

    def forward(self, images, encoder_name):
        content, style_fake = self.encode(images, encoder_name)
        return self.decode(content, style_fake, encoder_name)

    def encode(self, images, encoder_name):
        images = ops.nhwc(images)
        style_fake = self.enc_style(images)
        if encoder_name == 1:
            content = self.enc1_content(images)
        elif encoder_name == 2:
            content = self.enc2_content(images)
        else:
            print("wrong value for encoder_name, must be 0 or 1")
            return None
        return content, style_fake

    def decode(self, content, style, encoder_name):
        if encoder_name == 1:
            adain_params = self.mlp1(style)
            self.assign_adain_params(adain_params, self.dec1)
            images = self.dec1(content)
        elif encoder_name == 2:
            adain_params = self.mlp2(style)
            self.assign_adain_params(adain_params, self.dec2)
            images = self.dec2(content)
        else:
            print("wrong value for encoder_name, must be 0 or 1")
            return None
        return images

    def get_adain_param(self, style, encoder_name):
        if encoder_name == 1:
            return self.mlp1(style)
        if encoder_name == 2:
            return self.mlp2(style)
        print("wrong value for encoder_name, must be 0 or 1")
        return None

    def assign_adain_params(self, adain_params, model):
        _assign_adain_params(adain_params, model)

    def get_num_adain_params(self, model):
        return _num_adain_params(model)


# --------------------------------------------------------------------------------------
# discriminator
# --------------------------------------------------------------------------------------
# calc_dis_loss runs the fake and the real batch through the discriminator as ONE batch (MUNIT_NO_BATCH_DIS_PAIR=1: two passes)
BATCH_DIS_PAIR = os.environ.get("MUNIT_NO_BATCH_DIS_PAIR", "0") != "1"


class MsImageDis(_ApplyRefreshesImages, nn.Module):
    """networks.py:20-162: gan_type lsgan, and nsgan -- the reference's mean(binary_cross_entropy(sigmoid(x), t)) evaluated as
    mean(softplus(+-x)) by one ops.nsgan_loss over all scales (exact where the reference's fp32 sigmoid saturates)."""

    def __init__(self, input_dim, params):
        super().__init__()
        self.n_layer = params["n_layer"]
        self.gan_type = params["gan_type"]
        self.dim = params["dim"]
        self.norm = params["norm"]
        self.activ = params["activ"]
        self.num_scales = params["num_scales"]
        self.pad_type = params["pad_type"]
        self.input_dim = input_dim
        self.cnns = nn.ModuleList()
        for _ in range(self.num_scales):
            self.cnns.append(self._make_net())
        # dis.norm sn: the wrappers of all scales in module order, iterated by ONE call at the top of forward(); the descriptor
        # table lives on the device and is rebuilt when a parameter has moved (.to(device), the optimizer's bind)
        self.__dict__["_sn"] = [m for m in self.modules() if isinstance(m, SpectralNorm)]
        self.__dict__["_sn_table"] = None
        # called at the top of forward() -- calc_dis_loss / calc_gen_loss reach forward() directly, as the reference's do
        # (networks.py:84-85, 104), so a module pre-hook would not see them
        self.__dict__["before_forward"] = None

    def follow(self, gate):
        """The optimizer that owns the parameters hands over its gate (trainer.StepGate): forward() orders its stream behind
        a step still in flight, state_dict() and load_state_dict() settle it.  Forward and hooks hold the gate alone, so a
        deepcopy of this module takes a fresh, idle gate with it and nothing of the optimizer or the trainer."""
        self.__dict__["before_forward"] = gate.wait
        self.register_state_dict_pre_hook(gate.settle)
        self.register_load_state_dict_pre_hook(gate.settle)

    def _make_net(self):
        dim = self.dim
        cnn_x = [Conv2dBlock(self.input_dim, dim, 4, 2, 1, norm="none", activation=self.activ,
                             pad_type=self.pad_type)]
        for _ in range(self.n_layer - 1):
            cnn_x += [Conv2dBlock(dim, dim * 2, 4, 2, 1, norm=self.norm, activation=self.activ,
                                  pad_type=self.pad_type)]
            dim *= 2
        cnn_x += [Conv2d(dim, 1, 1, 1)]
        return nn.Sequential(*cnn_x)

    def downsample(self, x):
        return ops.avgpool3s2(x)

    def forward(self, x):
        if self.before_forward is not None:      # data parallel: order this stream behind a deferred optimizer step (follow)
            self.before_forward()
        x = ops.nhwc(x)
        if self._sn:
            self._sn_iterate()
        outputs = []
        for i, model in enumerate(self.cnns):
            h = x
            for m in model:
                h = m(h)
            outputs.append(h)
            if i + 1 < len(self.cnns):  # the reference also pools after the last scale and discards it
                x = self.downsample(x)
        return outputs

    def _sn_iterate(self):
        """One power iteration of every normalised layer (networks.py:899-911 runs it per layer inside each forward), and each
        wrapper gets the 1 / sigma of this forward."""
        layers = [m.layer() for m in self._sn]
        key = tuple(t.data_ptr() for layer in layers for t in layer)
        if self._sn_table is None or self._sn_table[0] != key:
            self.__dict__["_sn_table"] = (key, ops.sn_table(layers))
        sigma = ops.sn_power_iter(*self._sn_table[1])
        for k, m in enumerate(self._sn):
            m.assign(sigma[2 * k + 1:2 * k + 2])

    def _pair(self, first, second):
        """The discriminator's outputs for a (first -> 0, second -> 1) pair, as (outs, targets) of ops.lsgan_loss /
        ops.nsgan_loss.  BATCH_DIS_PAIR and equal shapes: one pass over [first; second] -- every layer of the discriminator
        is per-sample (no batch statistics), so the two halves of each output are exactly the reference's outs0 / outs1
        (networks.py:84-91) -- half the launches, and the small scales (16x16 ... 4x4 maps), which cannot fill the chip at
        B = 8, cost about the same at 2 B; every target is the pair (0.0, 1.0).  Else two passes, outs0 + outs1: always under
        dis.norm sn, where the second pass runs with the sigma of one more power iteration than the first."""
        if BATCH_DIS_PAIR and not self._sn and first.shape == second.shape and first.dtype == second.dtype:
            nb = first.shape[0]
            n0 = len(ops.MASK_SINK) if ops.MASK_SINK is not None else 0
            outs = self.forward(torch.cat([ops.nhwc(first), ops.nhwc(second)], 0))
            if ops.MASK_SINK is not None:   # parity harness: hand the recorded LeakyReLU branches over in the reference's order
                rec = ops.MASK_SINK[n0:]    # (all layers of the first pass, then all layers of the second pass)
                ops.MASK_SINK[n0:] = [m[:nb] for m in rec] + [m[nb:] for m in rec]
            return outs, [(0.0, 1.0)] * len(outs)
        outs0 = self.forward(first)
        outs1 = self.forward(second)
        return outs0 + outs1, [0.0] * len(outs0) + [1.0] * len(outs1)

    def calc_dis_loss(self, input_fake, input_real):
        if self.gan_type == "nsgan":        # networks.py:92-98: fake -> 0, real -> 1
            return self._multi_scale(ops.nsgan_loss, *self._pair(input_fake, input_real))
        assert self.gan_type == "lsgan", "Unsupported GAN type: {}".format(self.gan_type)
        # lsgan here and in calc_gen_loss stays on ops.mse_const per scale and half, summed by ops.scalar_sum in this order:
        # ops.lsgan_loss would change the launches and the summation order of the benchmarked dis_update / gen_update
        outs, targets = self._pair(input_fake, input_real)
        terms = []
        if isinstance(targets[0], tuple):
            nb = input_fake.shape[0]
            for out in outs:
                terms += [ops.mse_const(out[:nb], 0.0), ops.mse_const(out[nb:], 1.0)]
        else:
            k = len(outs) // 2
            for out0, out1 in zip(outs[:k], outs[k:]):
                terms += [ops.mse_const(out0, 0.0), ops.mse_const(out1, 1.0)]
        return ops.scalar_sum(terms)

    def calc_gen_loss(self, input_fake):
        outs0 = self.forward(input_fake)
        if self.gan_type == "nsgan":        # networks.py:110-112: fake -> 1
            return self._multi_scale(ops.nsgan_loss, outs0, [1.0] * len(outs0))
        assert self.gan_type == "lsgan", "Unsupported GAN type: {}".format(self.gan_type)
        return ops.scalar_sum([ops.mse_const(out0, 1.0) for out0 in outs0])     # not ops.lsgan_loss: see calc_dis_loss

    @staticmethod
    def _multi_scale(loss, outs, targets):
        """loss (ops.lsgan_loss / ops.nsgan_loss) over all scales in one launch pair (in groups of 8 segments when there are
        more scales than that)"""
        per = 2 if isinstance(targets[0], tuple) else 1
        step = max(1, 8 // per)
        if len(outs) <= step:
            return loss(outs, targets)
        return ops.scalar_sum([loss(outs[i:i + step], targets[i:i + step]) for i in range(0, len(outs), step)])

    def calc_dis_loss_sr(self, input_sim, input_real):
        """networks.py:117-139: simulated -> 0, real -> 1, summed over the scales.  One pass over [sim; real] under _pair's
        condition; the loss of all scales and both halves is one kernel pair (ops.lsgan_loss / ops.nsgan_loss)."""
        assert self.gan_type in ("lsgan", "nsgan"), "Unsupported GAN type: {}".format(self.gan_type)
        loss = ops.nsgan_loss if self.gan_type == "nsgan" else ops.lsgan_loss
        return self._multi_scale(loss, *self._pair(input_sim, input_real))

    def calc_gen_loss_sr(self, input_fake):
        """networks.py:141-162 (LSGAN; the reference's nsgan branch there names an undefined variable): target 0.5."""
        if self.gan_type == "nsgan":
            raise NotImplementedError("munit_amd: MsImageDis.calc_gen_loss_sr has no gan_type 'nsgan': the reference's own "
                                      "branch names an undefined variable (out1, networks.py:155) and raises NameError")
        outs0 = self.forward(input_fake)
        assert self.gan_type == "lsgan", "Unsupported GAN type: {}".format(self.gan_type)
        return self._multi_scale(ops.lsgan_loss, outs0, [0.5] * len(outs0))


# --------------------------------------------------------------------------------------
# feature classifier (adaptation.adv_lambda / dfeat_lambda)
# --------------------------------------------------------------------------------------
class BatchNorm2d(nn.Module):
    """Stands in for nn.BatchNorm2d (affine, track_running_stats): parameters `weight`, `bias`, buffers `running_mean`,
    `running_var`, `num_batches_tracked` as in torch.  In training mode every forward normalises with the batch statistics
    and moves the running ones (momentum 0.1, unbiased variance)."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1):
        super().__init__()
        self.num_features, self.eps, self.momentum = num_features, eps, momentum
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        # the count lives on the host (no launch per forward); the buffer receives it whenever state_dict() is read, and a
        # loaded state dict hands its value back
        self._tracked = 0
        self.register_state_dict_pre_hook(self._publish_tracked)

    @staticmethod
    def _publish_tracked(module, prefix, keep_vars):
        module.num_batches_tracked.fill_(module._tracked)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        if prefix + "num_batches_tracked" in state_dict:
            self._tracked = int(state_dict[prefix + "num_batches_tracked"])

    def forward(self, x, relu=False, need_weight_grads=True):
        if self.training:
            self._tracked += 1                 # nn.BatchNorm2d's num_batches_tracked
        return ops.batch_norm(x, self.weight, self.bias, self.running_mean, self.running_var, relu, self.eps, self.momentum,
                              self.training, need_weight_grads)

    def extra_repr(self):
        return "%d, eps=%g, momentum=%g" % (self.num_features, self.eps, self.momentum)


class BasicBlock(nn.Module):
    """scripts/utils.py:1277-1327 as domainClassifier builds it: stride 1 (`stride=True`), a conv1x1 + BatchNorm2d shortcut
    whenever the channel count changes."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1):
        super().__init__()
        if int(stride) != 1:
            raise NotImplementedError("munit_amd.BasicBlock: stride %r (the feature classifier uses stride 1)" % (stride,))
        self.conv1 = Conv2d(inplanes, planes, 3, 1, bias=False)
        self.bn1 = BatchNorm2d(planes)
        self.conv2 = Conv2d(planes, planes, 3, 1, bias=False)
        self.bn2 = BatchNorm2d(planes)
        self.stride = stride
        self.downsample = None
        if inplanes != planes:
            self.downsample = nn.Sequential(Conv2d(inplanes, planes, 1, 1, bias=False), BatchNorm2d(planes))

    def forward(self, x, need_weight_grads=True):
        out = self.bn1(self.conv1(x, 1), True, need_weight_grads)
        out = self.bn2(self.conv2(out, 1), False, need_weight_grads)
        identity = x
        if self.downsample is not None:
            identity = self.downsample[1](self.downsample[0](x), False, need_weight_grads)
        return ops.add_relu(out, identity, dann=True)


class domainClassifier(_ApplyRefreshesImages, nn.Module):
    """scripts/utils.py:1370-1392: MaxPool2d(2) -> BasicBlock(256, 128) -> MaxPool2d(2) -> BasicBlock(128, 64) ->
    AvgPool2d((16, 16)) -> squeeze -> Linear(64, 1) on a content code (B, 256, h, w)."""

    def __init__(self, dim):
        super().__init__()
        self.BasicBlock1 = BasicBlock(256, 128, True)
        self.BasicBlock2 = BasicBlock(128, 64, True)
        self.fc = Linear(64, 1)
        self.output_dim = dim

    @staticmethod
    def check_code_hw(h, w):
        """The 16x16 average followed by Linear(64, 1) needs exactly one window: the twice-pooled map must be 16..31 per axis."""
        ph, pw = h // 2 // 2, w // 2 // 2
        if not (16 <= ph <= 31 and 16 <= pw <= 31):
            raise ValueError("munit_amd.domainClassifier: a %dx%d content code pools to %dx%d; AvgPool2d((16, 16)) + "
                             "Linear(64, 1) need 16..31 on both axes (content codes of 64..127)" % (h, w, ph, pw))

    def forward(self, x, need_weight_grads=True):
        """need_weight_grads False: the backward pass forms the gradient of x only (the generator's use: the classifier's
        weight gradients would be zeroed before any use)."""
        x = ops.nhwc(x)
        if x.dim() != 4 or x.shape[1] != 256:
            raise ValueError("munit_amd.domainClassifier: a (B, 256, h, w) content code expected, got %s" % (tuple(x.shape),))
        self.check_code_hw(x.shape[2], x.shape[3])
        frozen = [] if need_weight_grads else [p for p in self.parameters() if p.requires_grad]
        for p in frozen:
            p.requires_grad_(False)
        try:
            h = ops.maxpool2(x)
            h = self.BasicBlock1(h, need_weight_grads)
            h = ops.maxpool2(h)
            h = self.BasicBlock2(h, need_weight_grads)
            out = self.fc(ops.avgpool16(h))
        finally:
            for p in frozen:
                p.requires_grad_(True)
        return out.reshape(1) if out.shape[0] == 1 else out      # the reference's .squeeze() drops the batch axis at B = 1
