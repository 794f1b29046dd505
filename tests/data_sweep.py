"""The size sweep of the input-pipeline kernels (munit_amd/csrc/image.hip) -- TEST INFRASTRUCTURE ONLY, not a test module.

Whether a resized pixel is right depends on the per-axis pair (source size s, resized size r) alone, so the sweep lists
pairs, not images.  This module holds

  * the case lists BILINEAR_PAIRS, BILINEAR_2D, NEAREST_PAIRS and the seeded contents of their images and planes;
  * the reference: Pillow itself (transpose, resize to an explicit (rs_w, rs_h), crop) followed by the oracle's to_tensor
    and normalisation (oracle/data_oracle.py), or the plane rules of tests/synth_data_oracle.py;
  * ctypes launchers of munit_image_preprocess, munit_mask_preprocess and munit_label_preprocess from explicit
    descriptors, each returning host tensors (tests/test_gpu_data_sweep.py);
  * numpy models of resample_tables_kernel + image_resample_kernel and of nearest_tables_kernel with a `variant`
    argument.  The faithful variants restate the kernels; the others are the mistakes the sweep has to catch.  The models
    exist only to prove on the CPU that the case lists discriminate (tests/test_cpu_data_sweep.py): no GPU test compares
    against them.
"""
import numpy as np
import torch
from PIL import Image

from munit_amd import _lib
from munit_amd import data as D
from oracle import data_oracle as DO
from tests import synth_data_oracle as SO

# ----------------------------------------------------------------------------------------------------------------------
# case lists
# ----------------------------------------------------------------------------------------------------------------------
BILINEAR_RS = [1, 2, 3, 4, 5, 7, 8, 9, 13, 16, 17, 24, 31, 32, 33, 64]


def bilinear_sources(r):
    """The source sizes swept against the resized size r: up-scaling from one pixel, identity, integer and non-integer
    down-scaling up to 1023 : 1."""
    s = {1, 2, 3, 4, 5, 7, r - 1, r, r + 1, 2 * r - 1, 2 * r, 2 * r + 1, 3 * r + 1, 3 * r // 2, 5 * r // 2 + 1, 10 * r + 3,
         33 * r + 7, 97, 131, 257, 600, 1023}
    return sorted(v for v in s if v >= 1)


BILINEAR_PAIRS = [(s, r) for r in BILINEAR_RS for s in bilinear_sources(r)]               # (source size, resized size)
BILINEAR_2D = [(37, 53, 24, 29), (20, 17, 47, 40), (90, 61, 32, 21), (64, 48, 31, 33)]    # (h, w, rs_h, rs_w)
NEAREST_RS = list(range(1, 70)) + [127, 256, 511, 600]
NEAREST_SS = list(range(1, 70)) + [97, 255, 256, 257, 1000, 1023, 1024, 2047]
NEAREST_PAIRS = [(s, r) for r in NEAREST_RS for s in NEAREST_SS]
# twenty of them with r >= 16 for a window of FAR at the far end of the walk: ten spread over the list, ten at which the
# last FAR indices of the running sum and of the product differ
FAR = 8
NEAREST_FAR_PAIRS = [(1, 16), (9, 22), (17, 28), (25, 34), (33, 40), (45, 49), (61, 61), (69, 67), (257, 127), (2047, 600),
                     (12, 18), (1024, 22), (256, 24), (68, 26), (1024, 30), (24, 33), (42, 45), (48, 54), (60, 65), (44, 66)]
assert len(BILINEAR_PAIRS) == 319 and len(NEAREST_PAIRS) == 5621

OTHER = {"image": 3, "plane": 2}                      # the size of the axis that stays at identity


def swept_hw(n, axis, what="image"):
    """(h, w) of a sweep item with n pixels along `axis` (numpy's numbering: 0 = rows / vertical, 1 = columns /
    horizontal); the other axis is short and stays at identity."""
    return (n, OTHER[what]) if axis == 0 else (OTHER[what], n)


# ----------------------------------------------------------------------------------------------------------------------
# contents
# ----------------------------------------------------------------------------------------------------------------------
def image(k, h, w):
    """The k-th image of a list, (h, w, 3) uint8: uniform noise for even k, a saturated 0 / 255 checkerboard (which
    drives both limits of clip8) for odd k.  Seeded by (k, h, w)."""
    if k % 2:
        a = ((np.add.outer(np.arange(h), np.arange(w)) % 2) * 255).astype(np.uint8)
        return np.ascontiguousarray(np.stack([a, 255 - a, a], -1))
    rng = np.random.RandomState((1000003 * h + 1009 * w + k) % (1 << 32))
    return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)


def plane(kind, h, w, axis):
    """A plane whose neighbours along `axis` never agree.  Label planes (kind 1) carry i % 251 along it, so an index one
    off is another value; mask planes (kind 0) alternate 0 and 255, so an index one off flips the output.  The other axis
    shifts the pattern, so a wrong row shows as well."""
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    along, across = (i, j) if axis == 0 else (j, i)
    if kind == D.KIND_LABEL:
        return ((along + 100 * across) % 251).astype(np.uint8)
    return (((along + across) % 2) * 255).astype(np.uint8)


# ----------------------------------------------------------------------------------------------------------------------
# reference: Pillow + the oracle's tensor conversion
# ----------------------------------------------------------------------------------------------------------------------
def pil_resize(arr, rs_h, rs_w, resample):
    """Image.resize of a uint8 array to an explicit size, as an array."""
    return np.asarray(Image.fromarray(arr).resize((rs_w, rs_h), resample))


def want_image(arr, flip, rs_h, rs_w, crop):
    """(3, h, w) float32: transpose, BILINEAR resize to (rs_w, rs_h), crop = (i, j, h, w), ToTensor, Normalize(.5, .5)."""
    img = Image.fromarray(arr)
    if flip:
        img = img.transpose(DO._FLIP)
    img = img.resize((rs_w, rs_h), DO._BILINEAR)
    i, j, h, w = crop
    img = img.crop((j, i, j + w, i + h))
    return DO.to_tensor(img).sub_(0.5).div_(0.5)


def want_plane(arr, kind, flip, rs_h, rs_w, crop):
    """(1, h, w) float32: the synthetic loader's mask rule (kind 0) or label table (kind 1) behind a NEAREST resize."""
    fn = SO.transform_mask if kind == D.KIND_MASK else SO.transform_label
    return fn(Image.fromarray(arr), bool(flip), (rs_w, rs_h), crop)


def want_mask(arr, flip, crop):
    """(1, h, w) float32: the list loader's mask chain (resize to the crop size, then crop with zero fill)."""
    return DO.transform_mask(Image.fromarray(arr), bool(flip), crop)


def first_diff(got, want):
    """Coordinates of the first differing element, with both values, for a failure message."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shapes %s / %s" % (got.shape, want.shape)
    bad = np.argwhere(~((got == want) | ((got != got) & (want != want))))
    if not len(bad):
        return "no difference"
    at = tuple(int(v) for v in bad[0])
    return "%d elements differ, first at %s: got %r, want %r" % (len(bad), at, got[at].item(), want[at].item())


# ----------------------------------------------------------------------------------------------------------------------
# launchers: the three entry points from explicit descriptors
# ----------------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"


def _upload(arrays, descs):
    """Pack the arrays at 16-byte boundaries and build the descriptors; descs[n] = (which array, rs_h, rs_w, crop_i,
    crop_j, flip, kind).  Returns (device pool, device descriptors)."""
    offs, cur = [], 0
    for a in arrays:
        offs.append(cur)
        cur += (a.size + 15) // 16 * 16
    pool = np.zeros(max(cur, 16), np.uint8)
    for a, o in zip(arrays, offs):
        pool[o:o + a.size] = a.reshape(-1)
    cd = (_lib.ImageDesc * len(descs))()
    for n, (k, rs_h, rs_w, i, j, flip, kind) in enumerate(descs):
        cd[n] = _lib.ImageDesc(offs[k], arrays[k].shape[0], arrays[k].shape[1], rs_h, rs_w, i, j, flip, kind)
    return torch.from_numpy(pool).to(DEV), torch.frombuffer(bytearray(bytes(cd)), dtype=torch.uint8).to(DEV)


def _ptr(t):
    from ctypes import c_void_p
    return c_void_p(t.data_ptr())


def _stream():
    from ctypes import c_void_p
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def needed_ksize(images, params, which=None):
    lib = _lib.load()
    which = range(len(params)) if which is None else which
    ksize = 3
    for k, (flip, rs_h, rs_w, i, j) in zip(which, params):
        ksize = max(ksize, lib.munit_image_ksize(images[k].shape[0], rs_h), lib.munit_image_ksize(images[k].shape[1], rs_w))
    return ksize


def preprocess_images(images, params, out_h, out_w, ksize=None, which=None):
    """munit_image_preprocess straight through ctypes.  params[n] = (flip, rs_h, rs_w, crop_i, crop_j) applies to
    images[which[n]] (images[n] without `which`); ksize defaults to what the batch needs.  Returns the (N, 3, out_h, out_w)
    result on the host (a view of the kernel's NHWC output)."""
    from ctypes import c_size_t
    lib = _lib.load()
    N = len(params)
    which = list(range(N)) if which is None else which
    if ksize is None:
        ksize = needed_ksize(images, params, which)
    pool, descs = _upload(images, [(k, rs_h, rs_w, i, j, flip, 0) for k, (flip, rs_h, rs_w, i, j) in zip(which, params)])
    out = torch.full((N, out_h, out_w, 3), float("nan"), device=DEV)
    nws = lib.munit_image_preprocess_workspace_bytes(N, out_h, out_w, ksize)
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device=DEV)
    rc = lib.munit_image_preprocess(_ptr(pool), _ptr(descs), N, out_h, out_w, ksize, _ptr(out), _ptr(ws), c_size_t(nws),
                                    _stream())
    _lib.check(rc, "munit_image_preprocess")
    torch.cuda.synchronize()
    return out.cpu().permute(0, 3, 1, 2)


def _plane_pass(name, planes, descs, out_h, out_w):
    from ctypes import c_size_t
    lib = _lib.load()
    N = len(descs)
    pool, dd = _upload(planes, descs)
    out = torch.full((N, 1, out_h, out_w), float("nan"), device=DEV)
    nws = getattr(lib, name + "_workspace_bytes")(N, out_h, out_w)
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device=DEV)
    rc = getattr(lib, name)(_ptr(pool), _ptr(dd), N, out_h, out_w, _ptr(out), _ptr(ws), c_size_t(nws), _stream())
    _lib.check(rc, name)
    torch.cuda.synchronize()
    return out.cpu()


def preprocess_labels(planes, kinds, params, out_h, out_w, which=None):
    """munit_label_preprocess straight through ctypes.  params[n] = (flip, rs_h, rs_w, crop_i, crop_j) and kinds[n] apply
    to planes[which[n]].  Returns the (N, 1, out_h, out_w) result on the host."""
    which = list(range(len(params))) if which is None else which
    descs = [(k, rs_h, rs_w, i, j, flip, kind) for k, kind, (flip, rs_h, rs_w, i, j) in zip(which, kinds, params)]
    return _plane_pass("munit_label_preprocess", planes, descs, out_h, out_w)


def preprocess_masks(planes, params, out_h, out_w, which=None):
    """munit_mask_preprocess straight through ctypes.  params[n] = (flip, crop_i, crop_j) applies to planes[which[n]]; the
    entry point reads no (rs_h, rs_w).  Returns the (N, 1, out_h, out_w) result on the host."""
    which = list(range(len(params))) if which is None else which
    descs = [(k, 0, 0, i, j, flip, 0) for k, (flip, i, j) in zip(which, params)]
    return _plane_pass("munit_mask_preprocess", planes, descs, out_h, out_w)


# ----------------------------------------------------------------------------------------------------------------------
# numpy models of the table kernels
# ----------------------------------------------------------------------------------------------------------------------
PRECISION_BITS = 32 - 8 - 2


def window(in_size, rs_size, xx):
    """(raw lower end, raw upper end) of resample_tables_kernel's window for the indices xx (an array) of the resized
    axis, before the clamps to [0, in_size]: the (int) casts of center -+ support + 0.5."""
    xx = np.asarray(xx)
    scale = in_size / rs_size
    support = max(scale, 1.0)
    center = (xx + 0.5) * scale
    return np.trunc(center - support + 0.5).astype(np.int64), np.trunc(center + support + 0.5).astype(np.int64)


def resample_matrix(in_size, rs_size, variant="faithful"):
    """The (rs_size, in_size) int64 matrix of fixed-point coefficients that resample_tables_kernel writes for a whole
    resized axis (row xx holds its window, zero elsewhere).
      faithful  the kernel as written: everything in double, coefficients rounded by +0.5
      f32       the weights, their sum and the fixed-point conversion in fp32 (the window still in double)
      trunc     coefficients truncated instead of rounded
      noround   the faithful coefficients (the variant changes model_resample)"""
    f = np.float32 if variant == "f32" else np.float64
    scale = in_size / rs_size
    filterscale = max(scale, 1.0)
    support = filterscale
    ss = 1.0 / filterscale
    K = np.zeros((rs_size, in_size), np.int64)
    for xx in range(rs_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        if xmax <= 0:
            continue
        x = np.arange(xmax)
        arg = ((x + xmin).astype(f) - f(center) + f(0.5)) * f(ss)
        w = np.maximum(f(1.0) - np.abs(arg), f(0.0)).astype(f)
        ww = np.cumsum(w, dtype=f)[-1]          # a running sum in index order, as the kernel's loop
        if ww != 0:
            w = (w / ww).astype(f)
        fixed = (w * f(1 << PRECISION_BITS)).astype(f)
        if variant != "trunc":
            fixed = np.where(fixed < 0, f(-0.5) + fixed, f(0.5) + fixed).astype(f)
        K[xx, xmin:xmin + xmax] = np.trunc(fixed).astype(np.int64)
    return K


def _clip8(v):
    return np.clip(v >> PRECISION_BITS, 0, 255)


def model_resample(arr, rs_h, rs_w, variant="faithful"):
    """image_resample_kernel on a whole (h, w, c) uint8 image: the horizontal pass, rounded to uint8, then the vertical
    pass.  Both passes always run, also on an axis at identity, as in the kernel.  `noround` keeps the horizontal result
    as a real number instead."""
    h, w = arr.shape[:2]
    kx, ky = resample_matrix(w, rs_w, variant), resample_matrix(h, rs_h, variant)
    half = 1 << (PRECISION_BITS - 1)
    hor = np.einsum("xk,ykc->yxc", kx, arr.astype(np.int64))
    if variant == "noround":
        v = np.einsum("yk,kxc->yxc", ky.astype(np.float64), hor.astype(np.float64)) / float(1 << (2 * PRECISION_BITS))
        return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)
    hor = _clip8(hor + half)
    return _clip8(np.einsum("yk,kxc->yxc", ky, hor) + half).astype(np.uint8)


def nearest_table(in_size, rs_size, variant="faithful"):
    """nearest_tables_kernel's source index for every index of the resized axis (-1 = none).
      faithful  the running sum xo += a from a * 0.5, as ImagingScaleAffine walks
      product   (x + 0.5) * a, which rounds differently"""
    a = in_size / rs_size
    if variant == "product":
        xo = (np.arange(rs_size) + 0.5) * a
    else:
        xo = np.cumsum(np.concatenate(([a * 0.5], np.full(rs_size - 1, a))))
    xin = np.trunc(xo).astype(np.int64)
    return np.where((xo >= 0) & (xin < in_size), xin, -1)


def model_nearest(arr, rs_h, rs_w, variant="faithful"):
    """A NEAREST resize of an (h, w) plane through nearest_table; positions without a source pixel read 0."""
    ty, tx = nearest_table(arr.shape[0], rs_h, variant), nearest_table(arr.shape[1], rs_w, variant)
    out = arr[np.maximum(ty, 0)][:, np.maximum(tx, 0)].copy()
    out[ty < 0, :] = 0
    out[:, tx < 0] = 0
    return out
