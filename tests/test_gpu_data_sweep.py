"""GPU: the input-pipeline kernels of munit_amd/csrc/image.hip against Pillow over a sweep of (source size, resized size)
pairs, crops and flips, through the C ABI.  Every comparison is exact (torch.equal): the resamplers are integer work on
tables computed in double, and the float stage performs the oracle's fp32 operations in the oracle's order.

Whether a resized pixel is right depends on the per-axis pair alone, so the sweeps resize one axis and leave the other at
identity; four 2-D cases add the uint8 rounding between the two passes.  The case lists, their contents, the reference and
the launchers live in tests/data_sweep.py; tests/test_cpu_data_sweep.py shows on the CPU that the lists catch a
restatement with fp32 or truncated coefficients, without the rounding between the passes, or with the NEAREST index taken
from a product instead of the running sum."""
import numpy as np
import pytest
import torch

from tests import data_sweep as S

pytestmark = pytest.mark.gpu

AXES = pytest.mark.parametrize("axis", [1, 0], ids=["horizontal", "vertical"])
T = 16                                # the window of the 2-D cases


def _same(got, want, what):
    assert torch.equal(got, want), "%s: %s" % (what, S.first_diff(got.numpy(), want.numpy()))


# ------------------------------------------------------------------------------------------------------------------
# BILINEAR
# ------------------------------------------------------------------------------------------------------------------
@AXES
def test_bilinear_sweep(axis):
    """Images of 3 x s resized to 3 x r (horizontal) or of s x 3 to r x 3 (vertical), the whole resized image, flip 0 and
    1.  One launch per r holds all its s, so up-scaling from one pixel, identity and down-scaling by up to 1023 share a
    launch and its ksize_max (2047 taps at r = 1)."""
    for r in S.BILINEAR_RS:
        items = [(k, s) for k, (s, rr) in enumerate(S.BILINEAR_PAIRS) if rr == r]
        images = [S.image(k, *S.swept_hw(s, axis)) for k, s in items]
        rs_h, rs_w = S.swept_hw(r, axis)
        which = list(range(len(images))) * 2
        params = [(flip, rs_h, rs_w, 0, 0) for flip in (0, 1) for _ in images]
        got = S.preprocess_images(images, params, rs_h, rs_w, which=which)
        assert got.shape == (len(params), 3, rs_h, rs_w)
        for n, (k, p) in enumerate(zip(which, params)):
            want = S.want_image(images[k], p[0], rs_h, rs_w, (0, 0, rs_h, rs_w))
            _same(got[n], want, "BILINEAR s=%d r=%d axis=%d flip=%d" % (items[k][1], r, axis, p[0]))


def _windows(rs_h, rs_w):
    """The four corners of the resized image, crop = rs - T on both axes among them, and one interior window."""
    return [(0, 0), (0, rs_w - T), (rs_h - T, 0), (rs_h - T, rs_w - T), ((rs_h - T) // 2, (rs_w - T) // 2)]


def _two_d_batch():
    images = [S.image(k, h, w) for k, (h, w, rs_h, rs_w) in enumerate(S.BILINEAR_2D)]
    which, params = [], []
    for k, (h, w, rs_h, rs_w) in enumerate(S.BILINEAR_2D):
        for flip in (0, 1):
            for i, j in _windows(rs_h, rs_w):
                which.append(k)
                params.append((flip, rs_h, rs_w, i, j))
    return images, which, params


def test_bilinear_2d_windows_in_one_launch():
    """The four 2-D cases (down and up on both axes, and one of each), 16 x 16 windows at the four corners and inside, both
    flips: 40 descriptors of other sizes and ratios in one launch."""
    images, which, params = _two_d_batch()
    got = S.preprocess_images(images, params, T, T, which=which)
    for n, (k, (flip, rs_h, rs_w, i, j)) in enumerate(zip(which, params)):
        want = S.want_image(images[k], flip, rs_h, rs_w, (i, j, T, T))
        _same(got[n], want, "BILINEAR 2-D %s flip=%d window at (%d, %d)" % (S.BILINEAR_2D[k], flip, i, j))


@pytest.mark.parametrize("case", range(len(S.BILINEAR_2D)), ids=["%dx%d_to_%dx%d" % c for c in S.BILINEAR_2D])
def test_bilinear_2d_whole(case):
    h, w, rs_h, rs_w = S.BILINEAR_2D[case]
    img = S.image(case, h, w)
    got = S.preprocess_images([img], [(0, rs_h, rs_w, 0, 0), (1, rs_h, rs_w, 0, 0)], rs_h, rs_w, which=[0, 0])
    for flip in (0, 1):
        want = S.want_image(img, flip, rs_h, rs_w, (0, 0, rs_h, rs_w))
        _same(got[flip], want, "BILINEAR 2-D %s flip=%d, whole" % (S.BILINEAR_2D[case], flip))


def test_ksize_max_slack_changes_nothing():
    """The batch of the 2-D windows with the ksize_max it needs and with five more: bitwise the same output."""
    images, which, params = _two_d_batch()
    need = S.needed_ksize(images, params, which)
    assert need == 7                                                    # 90 -> 32: ceil(2.8125) * 2 + 1
    a = S.preprocess_images(images, params, T, T, ksize=need, which=which).contiguous()
    b = S.preprocess_images(images, params, T, T, ksize=need + 5, which=which).contiguous()
    assert not torch.isnan(a).any() and not torch.isnan(b).any()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), S.first_diff(a.numpy(), b.numpy())


def test_all_byte_values_through_the_float_chain():
    """One identity image that holds every byte value in every channel: (v / 255 - 0.5) / 0.5 in fp32 equals the oracle's
    chain for all 256 values, and all 256 floats are distinct."""
    img = np.stack([np.roll(np.arange(256), 37 * c).reshape(16, 16) for c in range(3)], -1).astype(np.uint8)
    got = S.preprocess_images([img], [(0, 16, 16, 0, 0), (1, 16, 16, 0, 0)], 16, 16, which=[0, 0])
    for flip in (0, 1):
        _same(got[flip], S.want_image(img, flip, 16, 16, (0, 0, 16, 16)), "identity, flip=%d" % flip)
    chain = torch.arange(256, dtype=torch.float32).div(255).sub_(0.5).div_(0.5)
    for c in range(3):
        _same(got[0, c], chain[torch.from_numpy(img[:, :, c].astype(np.int64))], "channel %d against the fp32 chain" % c)
        assert len(set(got[0, c].flatten().tolist())) == 256
    assert got[0].min() == -1.0 and got[0].max() == 1.0


# ------------------------------------------------------------------------------------------------------------------
# NEAREST
# ------------------------------------------------------------------------------------------------------------------
def _check_planes(planes, kinds, params, out_h, out_w, what):
    got = S.preprocess_labels(planes, kinds, params, out_h, out_w)
    assert got.shape == (len(planes), 1, out_h, out_w)
    for n, (p, kind, (flip, rs_h, rs_w, i, j)) in enumerate(zip(planes, kinds, params)):
        want = S.want_plane(p, kind, flip, rs_h, rs_w, (i, j, out_h, out_w))
        _same(got[n], want, "NEAREST %s flip=%d kind=%d" % (what(n), flip, kind))


@AXES
def test_nearest_sweep(axis):
    """Planes of 2 x s resized to 2 x r (horizontal) or of s x 2 to r x 2 (vertical) for all 5 621 pairs, the whole resized
    plane, both flips; one launch per r with all its s.  Half the planes are label maps (i % 251 along the swept axis, through
    the label table), half are masks (0 / 255 alternating, through the mask rule): either way a source index one off is
    another output."""
    cache = {(s, kind): S.plane(kind, *S.swept_hw(s, axis, "plane"), axis) for s in S.NEAREST_SS for kind in (0, 1)}
    for r in S.NEAREST_RS:
        rs_h, rs_w = S.swept_hw(r, axis, "plane")
        planes, kinds, params, sizes = [], [], [], []
        for n, s in enumerate(S.NEAREST_SS):
            for flip in (0, 1):
                kind = (n + flip) & 1
                planes.append(cache[s, kind])
                kinds.append(kind)
                params.append((flip, rs_h, rs_w, 0, 0))
                sizes.append(s)
        assert sum(kinds) * 2 == len(kinds)
        _check_planes(planes, kinds, params, rs_h, rs_w, lambda n: "s=%d r=%d axis=%d" % (sizes[n], r, axis))


@AXES
def test_nearest_window_at_the_far_end(axis):
    """Twenty pairs with r >= 16, a window of 8 at crop = r - 8: the table keeps the end of a walk that starts at index 0.
    At ten of the pairs a walk started at the window, or an index from the product, ends elsewhere."""
    crop = [r - S.FAR for s, r in S.NEAREST_FAR_PAIRS]
    out_h, out_w = S.swept_hw(S.FAR, axis, "plane")
    planes, kinds, params, names = [], [], [], []
    for n, (s, r) in enumerate(S.NEAREST_FAR_PAIRS):
        rs_h, rs_w = S.swept_hw(r, axis, "plane")
        for flip in (0, 1):
            kind = (n + flip) & 1
            planes.append(S.plane(kind, *S.swept_hw(s, axis, "plane"), axis))
            kinds.append(kind)
            params.append((flip, rs_h, rs_w, crop[n] if axis == 0 else 0, crop[n] if axis == 1 else 0))
            names.append("s=%d r=%d axis=%d crop=%d" % (s, r, axis, crop[n]))
    _check_planes(planes, kinds, params, out_h, out_w, lambda n: names[n])


MASK_SIDES = [1, 2, 7, 16, 33, 97, 257]


@pytest.mark.parametrize("out", [(5, 6), (16, 16), (33, 31)], ids=lambda o: "%dx%d" % o)
def test_mask_preprocess_sweep(out):
    """munit_mask_preprocess, the other use of the NEAREST table: the whole mask resized to the output size, then cropped
    at the image's offsets with zero fill.  Masks of every size of MASK_SIDES x MASK_SIDES, 0 / 1 (the x255 rule) and
    0 / 255, both flips, five offsets -- the last one, (out_h, 0), leaves nothing of the mask."""
    out_h, out_w = out
    rng = np.random.RandomState(31 * out_h + out_w)
    planes, top = [], []
    for sh in MASK_SIDES:
        for sw in MASK_SIDES:
            for v in (1, 255):
                planes.append(((rng.rand(sh, sw) > 0.5) * v).astype(np.uint8))
                top.append(v)
    crops = [(0, 0), (1, 0), (0, 3), (out_h - 1, out_w - 1), (out_h, 0)]
    which, params = [], []
    for k in range(len(planes)):
        for flip in (0, 1):
            for i, j in crops:
                which.append(k)
                params.append((flip, i, j))
    got = S.preprocess_masks(planes, params, out_h, out_w, which=which)
    assert got.shape == (len(params), 1, out_h, out_w)
    fired = 0
    for n, (k, (flip, i, j)) in enumerate(zip(which, params)):
        want = S.want_mask(planes[k], flip, (i, j, out_h, out_w))
        _same(got[n], want, "mask %s (0 / %d) -> %s flip=%d crop=(%d, %d)" % (planes[k].shape, top[k], out, flip, i, j))
        if i == out_h:
            assert got[n].abs().sum() == 0
        fired += top[k] == 1 and got[n].max() == 1.0
    assert fired > 100                                                  # the x255 rule gave ones, not 1 / 255
