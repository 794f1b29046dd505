"""Host-side helpers of the hot path: config, init, LR schedule, sample grids and output folders (reference:
scripts/utils.py)."""
import math
import os

import torch
import torch.nn.init as init
import yaml
from torch.optim import lr_scheduler

ADAPTATION_DEFAULTS = dict(full_adaptation=0, output_classifier_lambda=0, output_adv_lambda=0,
                           output_classif_freq=1, adv_lambda=0, dfeat_lambda=0, classif_frequency=15,
                           sem_seg_lambda=0,
                           # build extension (no reference counterpart): 1 lets the adaptation terms train data-parallel,
                           # with the feature classifiers' batch-norm statistics taken over all ranks (trainer.py)
                           data_parallel=0)


def get_config(config):
    """utils.py:743-758: yaml.safe_load + default optimizer 'adam'.  Additionally fills the
    `adaptation:` block with zeros when a (stale) config such as config_HD.yaml lacks it
     -- the reference would raise KeyError there."""
    with open(config, "r") as stream:
        conf = yaml.safe_load(stream)
    if "optimizer" not in conf:
        conf["optimizer"] = "adam"
    return normalize_config(conf)


def normalize_config(conf):
    conf.setdefault("optimizer", "adam")
    ad = dict(ADAPTATION_DEFAULTS)
    ad.update(conf.get("adaptation") or {})
    conf["adaptation"] = ad
    for k in ("semantic_w", "domain_adv_w", "vgg_w", "recon_synth_w"):
        conf.setdefault(k, 0)
    conf.setdefault("recon_mask", 0)
    return conf


def get_scheduler(optimizer, hyperparameters, iterations=-1):
    """utils.py:1066-1090."""
    if "lr_policy" not in hyperparameters or hyperparameters["lr_policy"] == "constant":
        scheduler = None
    elif hyperparameters["lr_policy"] == "step":
        if iterations != -1:
            for g in optimizer.param_groups:
                g.setdefault("initial_lr", g["lr"])
        scheduler = lr_scheduler.StepLR(optimizer, step_size=hyperparameters["step_size"],
                                        gamma=hyperparameters["gamma"], last_epoch=iterations)
    else:
        # the reference RETURNS the exception object here instead of raising it (utils.py:1087-1089); kept, because a
        # caller written against the reference sees the same value (and the same failure at the first .step())
        return NotImplementedError("learning rate policy [%s] is not implemented", hyperparameters["lr_policy"])
    return scheduler


def _fill_like_reference(param, fn):
    """Draw into a standard-contiguous CPU tensor (the layout the reference's parameters have, so
    the RNG stream maps to the same logical elements) and copy into the parameter's storage."""
    tmp = torch.empty(tuple(param.shape), dtype=torch.float32)
    fn(tmp)
    with torch.no_grad():
        param.copy_(tmp.to(param.device))


def weights_init(init_type="gaussian"):
    """utils.py:1093-1115: applies to modules whose class name starts with Conv / Linear and
    that own a `weight` (so the *Block wrappers are skipped exactly as in the reference)."""

    def init_fun(m):
        classname = m.__class__.__name__
        if (classname.find("Conv") == 0 or classname.find("Linear") == 0) and hasattr(m, "weight"):
            if init_type == "gaussian":
                _fill_like_reference(m.weight, lambda t: init.normal_(t, 0.0, 0.02))
            elif init_type == "xavier":
                _fill_like_reference(m.weight, lambda t: init.xavier_normal_(t, gain=math.sqrt(2)))
            elif init_type == "kaiming":
                _fill_like_reference(m.weight, lambda t: init.kaiming_normal_(t, a=0, mode="fan_in"))
            elif init_type == "orthogonal":
                _fill_like_reference(m.weight, lambda t: init.orthogonal_(t, gain=math.sqrt(2)))
            elif init_type == "default":
                pass
            else:
                assert 0, "Unsupported initialization: {}".format(init_type)
            if hasattr(m, "bias") and m.bias is not None:
                with torch.no_grad():
                    m.bias.zero_()

    return init_fun


def get_model_list(dirname, key):
    """Checkpoint discovery for resume (utils.py:887-908): among the regular files of `dirname`
    whose name contains both `key` and ".pt", the one that sorts last; None if the directory
    is missing or holds no match."""
    if not os.path.isdir(dirname):
        return None
    names = sorted(n for n in os.listdir(dirname)
                   if key in n and ".pt" in n and os.path.isfile(os.path.join(dirname, n)))
    return os.path.join(dirname, names[-1]) if names else None


def load_segmentation_model(ckpt_path, classes):
    """utils.py:974-983 under the reference's name (munit_amd/segmentation.py)."""
    from .segmentation import load_segmentation_model as load
    return load(ckpt_path, classes)


def mapping(im):
    """Simulator label colours -> class indices, in place on a tensor (utils.py:1356-1366): every element equal to a key
    of munit_amd.data.LABEL_CLASSES becomes its class, in the reference's order; every other value is left alone.
    Returns `im`.  (The synthetic loader applies the same table on the device, csrc/image.hip.)"""
    from .data import LABEL_CLASSES
    for grey, cls in LABEL_CLASSES.items():
        im[im == grey] = cls
    return im


def _save_grid(tensors, nrow, path, pre_add=0.0, pre_mul=1.0):
    """One ops.image_grid, one device-to-host copy, one PIL save with Pillow's defaults (what torchvision's save_image
    does with the array)."""
    from PIL import Image
    from . import ops
    grid = ops.image_grid(tensors, nrow, pre_add, pre_mul)
    Image.fromarray(grid.cpu().numpy()).save(path)


def write_2images(image_outputs, display_image_num, image_directory, postfix, comet_exp=None):
    """utils.py:768-814: the first half of `image_outputs` (the tuple of MUNIT_Trainer.sample) as one grid into
    gen_a2b_<postfix>.jpg, the second half into gen_b2a_<postfix>.jpg -- one row per tensor, its first
    `display_image_num` images, one-channel tensors repeated over three channels, the whole grid min-max scaled
    (make_grid(normalize=True)) on the device (ops.image_grid)."""
    n = len(image_outputs)
    names = ("%s/gen_a2b_%s.jpg" % (image_directory, postfix), "%s/gen_b2a_%s.jpg" % (image_directory, postfix))
    _save_grid(image_outputs[0:n // 2], display_image_num, names[0])
    _save_grid(image_outputs[n // 2:n], display_image_num, names[1])
    if comet_exp is not None:
        comet_exp.log_image(names[0])
        comet_exp.log_image(names[1])


def write_image(x, path, pre_add=0.0, pre_mul=1.0):
    """vutils.save_image((x + pre_add) * pre_mul, path, padding=0, normalize=True) for one image (1, C, H, W)
    (scripts/test.py:123-129 with pre_add, pre_mul = 1, 0.5)."""
    if x.dim() != 4 or x.shape[0] != 1:
        raise ValueError("write_image takes one image (1, C, H, W), got %s" % (tuple(x.shape),))
    _save_grid([x], 1, path, pre_add, pre_mul)


def prepare_sub_folder(output_directory):
    """utils.py:817-834: make sure <output_directory>/checkpoints and <output_directory>/images exist (a folder that has
    to be made is announced on stdout, as the reference does) and return them in that order."""
    made = []
    for name in ("images", "checkpoints"):
        d = os.path.join(output_directory, name)
        if not os.path.exists(d):
            print("Creating directory: %s" % d)
            os.makedirs(d)
        made.append(d)
    return made[1], made[0]
