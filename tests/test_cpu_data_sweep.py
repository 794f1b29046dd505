"""CPU: conditions on the size sweep of the input-pipeline kernels (tests/data_sweep.py) -- no device.

The GPU sweep (tests/test_gpu_data_sweep.py) compares the kernels with Pillow at a list of (source size, resized size)
pairs.  Here the lists themselves are put to the test: a numpy model of the table kernels as written equals Pillow on every
case (which also detects a Pillow whose resampler differs from the one the kernels restate), every plausible mistake in
the restatement differs from Pillow on at least one case, the lists reach the branches of the window arithmetic, and
munit_image_ksize is never shorter than the longest window, so the clamp to ksize_max in resample_tables_kernel never
decides a result."""
import numpy as np
import PIL

from munit_amd import _lib
from munit_amd import data as D
from oracle import data_oracle as DO
from tests import data_sweep as S


def _bilinear_1d():
    """(s, r, axis, image, Pillow's resize) of every pair on both axes, the images the GPU sweep uses."""
    for axis in (1, 0):
        for k, (s, r) in enumerate(S.BILINEAR_PAIRS):
            img = S.image(k, *S.swept_hw(s, axis))
            rs_h, rs_w = S.swept_hw(r, axis)
            yield s, r, axis, img, S.pil_resize(img, rs_h, rs_w, DO._BILINEAR)


def _bilinear_2d():
    for k, (h, w, rs_h, rs_w) in enumerate(S.BILINEAR_2D):
        img = S.image(k, h, w)
        yield img, rs_h, rs_w, S.pil_resize(img, rs_h, rs_w, DO._BILINEAR)


def _nearest_1d():
    for axis in (1, 0):
        for k, (s, r) in enumerate(S.NEAREST_PAIRS):
            p = S.plane(k % 2, *S.swept_hw(s, axis, "plane"), axis)
            rs_h, rs_w = S.swept_hw(r, axis, "plane")
            yield s, r, axis, p, S.pil_resize(p, rs_h, rs_w, DO._NEAREST)


def test_lists_are_the_stated_ones():
    assert len(S.BILINEAR_PAIRS) == 319 == len(set(S.BILINEAR_PAIRS))
    assert len(S.NEAREST_PAIRS) == 5621 == len(set(S.NEAREST_PAIRS))
    assert len(S.BILINEAR_2D) == 4
    assert len(set(S.NEAREST_FAR_PAIRS)) == 20 and set(S.NEAREST_FAR_PAIRS) <= set(S.NEAREST_PAIRS)
    assert all(r >= 16 for s, r in S.NEAREST_FAR_PAIRS)
    assert min(min(p) for p in S.BILINEAR_PAIRS + S.NEAREST_PAIRS) == 1
    assert max(s for s, r in S.NEAREST_PAIRS) == 2047 and max(r for s, r in S.NEAREST_PAIRS) == 600
    for h, w, rs_h, rs_w in S.BILINEAR_2D:
        assert rs_h >= 16 and rs_w >= 16                     # the GPU test cuts 16 x 16 windows at the corners


def test_faithful_models_equal_pillow():
    print("Pillow %s" % PIL.__version__)
    for s, r, axis, img, want in _bilinear_1d():
        got = S.model_resample(img, *S.swept_hw(r, axis))
        assert np.array_equal(got, want), "BILINEAR s=%d r=%d axis=%d: %s" % (s, r, axis, S.first_diff(got, want))
    for img, rs_h, rs_w, want in _bilinear_2d():
        got = S.model_resample(img, rs_h, rs_w)
        assert np.array_equal(got, want), "BILINEAR %s -> %s: %s" % (img.shape[:2], (rs_h, rs_w), S.first_diff(got, want))
    for s, r, axis, p, want in _nearest_1d():
        got = S.model_nearest(p, *S.swept_hw(r, axis, "plane"))
        assert np.array_equal(got, want), "NEAREST s=%d r=%d axis=%d: %s" % (s, r, axis, S.first_diff(got, want))


def test_every_variant_is_caught():
    """A condition on the inputs: each mistaken restatement differs from Pillow somewhere in the lists.  A count of 0 after
    an edit of the lists or of the contents means that the list is wrong, not this condition."""
    pairs = {v: set() for v in ("f32", "trunc", "noround")}
    for s, r, axis, img, want in _bilinear_1d():
        for v in pairs:
            if not np.array_equal(S.model_resample(img, *S.swept_hw(r, axis), v), want):
                pairs[v].add((s, r))
    two_d = {v: 0 for v in pairs}
    for img, rs_h, rs_w, want in _bilinear_2d():
        for v in pairs:
            two_d[v] += not np.array_equal(S.model_resample(img, rs_h, rs_w, v), want)
    product = set()
    for s, r, axis, p, want in _nearest_1d():
        if not np.array_equal(S.model_nearest(p, *S.swept_hw(r, axis, "plane"), "product"), want):
            product.add((s, r))
    far = 0
    for k, (s, r) in enumerate(S.NEAREST_FAR_PAIRS):
        p = S.plane(k % 2, *S.swept_hw(s, 1, "plane"), 1)
        want = S.pil_resize(p, 2, r, DO._NEAREST)[:, r - S.FAR:]
        assert np.array_equal(S.model_nearest(p, 2, r)[:, r - S.FAR:], want), (s, r)
        far += not np.array_equal(S.model_nearest(p, 2, r, "product")[:, r - S.FAR:], want)
    n, n2 = len(S.BILINEAR_PAIRS), len(S.BILINEAR_2D)
    print("Pillow %s" % PIL.__version__)
    print("fp32 coefficients: %d of %d pairs, %d of %d 2-D cases" % (len(pairs["f32"]), n, two_d["f32"], n2))
    print("truncated coefficients: %d of %d pairs, %d of %d 2-D cases" % (len(pairs["trunc"]), n, two_d["trunc"], n2))
    print("no uint8 rounding between the passes: %d of %d pairs, %d of %d 2-D cases"
          % (len(pairs["noround"]), n, two_d["noround"], n2))
    print("NEAREST index from the product: %d of %d pairs" % (len(product), len(S.NEAREST_PAIRS)))
    assert len(pairs["f32"]) >= 1
    assert len(pairs["trunc"]) >= 1
    assert two_d["noround"] >= 1          # with one axis at identity the second rounding changes nothing: the 2-D cases decide
    assert len(product) >= 1
    print("NEAREST index from the product, window at the far end: %d of %d pairs" % (far, len(S.NEAREST_FAR_PAIRS)))
    assert far >= 1


def test_lists_reach_the_branches_of_the_window_arithmetic():
    lib = _lib.load()
    low = high = one_tap = 0
    for s, r in S.BILINEAR_PAIRS:
        lo, hi = S.window(s, r, np.arange(r))
        low += bool((lo < 0).any())                              # the clamp at 0 changes the window
        high += bool((hi > s).any())                             # the clamp at the source size does
        one_tap += bool((np.minimum(hi, s) - np.maximum(lo, 0) == 1).any())
    below = sum(s < r for s, r in S.BILINEAR_PAIRS)
    at = sum(s == r for s, r in S.BILINEAR_PAIRS)
    above = sum(s > r for s, r in S.BILINEAR_PAIRS)
    integer = sum(s > r and s % r == 0 for s, r in S.BILINEAR_PAIRS)      # centers on n + 0.5: ties of the + 0.5 casts
    ksizes = sorted(set(lib.munit_image_ksize(s, r) for s, r in S.BILINEAR_PAIRS))
    print("pairs with a window clamped at 0: %d, clamped at the source size: %d, with a one-tap window: %d"
          % (low, high, one_tap))
    print("scale below 1: %d, at 1: %d, above 1: %d, integer above 1: %d" % (below, at, above, integer))
    print("munit_image_ksize: %d values from %d to %d" % (len(ksizes), ksizes[0], ksizes[-1]))
    assert low >= 1 and high >= 1 and one_tap >= 1
    assert below >= 1 and at >= 1 and above >= 1 and integer >= 1
    assert ksizes[0] == 3 and 5 in ksizes and ksizes[-1] >= 69
    assert ksizes[-1] == 2047                                    # 1023 -> 1
    # the 2-D cases scale both ways on both axes between them
    assert any(h < rh for h, w, rh, rw in S.BILINEAR_2D) and any(h > rh for h, w, rh, rw in S.BILINEAR_2D)
    assert any(w < rw for h, w, rh, rw in S.BILINEAR_2D) and any(w > rw for h, w, rh, rw in S.BILINEAR_2D)
    # NEAREST: both directions, identity, and the planes of either kind on every resized size
    assert any(s < r for s, r in S.NEAREST_PAIRS) and any(s == r for s, r in S.NEAREST_PAIRS)
    assert any(s > r for s, r in S.NEAREST_PAIRS)
    assert {D.KIND_MASK, D.KIND_LABEL} == {0, 1}


def test_ksize_covers_the_longest_window():
    """munit_image_ksize(s, r) >= the longest clamped window of the tables for every s, r in 1..256: `if (xmax > ksize_max)`
    in resample_tables_kernel never fires when the host sizes ksize_max with this function.  The bound is reached (the
    printed margin is 0), so nothing shorter would do."""
    lib = _lib.load()
    worst = -1 << 30
    for r in range(1, 257):
        xx = np.arange(r)
        for s in range(1, 257):
            lo, hi = S.window(s, r, xx)
            longest = int((np.minimum(hi, s) - np.maximum(lo, 0)).max())
            k = lib.munit_image_ksize(s, r)
            assert k >= longest, (s, r, k, longest)
            worst = max(worst, longest - k)
    print("longest window minus munit_image_ksize, at most: %d" % worst)
    assert worst == 0
    assert lib.munit_image_ksize(0, 5) == 0 and lib.munit_image_ksize(5, 0) == 0
