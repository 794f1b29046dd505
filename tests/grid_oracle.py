"""Oracle of munit_image_grid_u8 (include/munit_hip.h) in numpy, and the inputs the grid tests share.  Not a test module.

grid_u8 restates the seven steps of the entry point -- the reference's __write_images (scripts/utils.py:768-784) with
torchvision's make_grid(normalize=True, padding=0) and save_image written out -- with every operation rounded to fp32
explicitly.  The one step that is not fp32 is the reference's own: `max(hi - lo, 1e-5)` is formed from python floats, i.e.
in double, and rounded to fp32 once when torch's device kernel takes it as the divisor; that kernel multiplies by the fp32
reciprocal of the scalar, and so does the oracle.

A source is what the C ABI calls one: a flat fp32 buffer holding n images of H x W with 1 or 3 channels, planar
([n][C][H][W], layout 0) or interleaved ([n][H][W][C], layout 1)."""
import numpy as np

F = np.float32
PLANAR, INTERLEAVED = 0, 1


def source(x, layout):
    """Source descriptor of the logical (n, C, H, W) array x laid out in memory as `layout` says."""
    x = np.asarray(x, dtype=F)
    n, c, _, _ = x.shape
    flat = x.reshape(-1) if layout == PLANAR else x.transpose(0, 2, 3, 1).reshape(-1)
    return dict(data=np.ascontiguousarray(flat), n=n, channels=c, layout=layout)


def logical(src, H, W):
    """The (n, C, H, W) view of a source."""
    n, c = src["n"], src["channels"]
    if src["layout"] == PLANAR:
        return src["data"][:n * c * H * W].reshape(n, c, H, W)
    return src["data"][:n * c * H * W].reshape(n, H, W, c).transpose(0, 3, 1, 2)


def grid_shape(nmaps, nrow):
    xmaps = min(nrow, nmaps)
    return xmaps, (nmaps + xmaps - 1) // xmaps


def grid_u8(srcs, H, W, nrow, pre_add=0.0, pre_mul=1.0):
    """The (ymaps * H, xmaps * W, 3) uint8 grid of the sources."""
    vs = []
    for s in srcs:
        x = logical(s, H, W)
        v = ((x + F(pre_add)).astype(F) * F(pre_mul)).astype(F)                    # step 1: two roundings
        vs.append(np.repeat(v, 3, axis=1) if s["channels"] == 1 else v)           # step 2
    v = np.concatenate(vs, 0)
    lo, hi = F(v.min()), F(v.max())                                                # step 3
    d = F(max(float(hi) - float(lo), 1e-5))                                        # step 4: python floats, rounded once
    r = F(F(1.0) / d)
    t = ((v - lo).astype(F) * r).astype(F)
    q = ((t * F(255.0)).astype(F) + F(0.5)).astype(F)                              # step 6: rounded separately
    u = np.clip(q, F(0.0), F(255.0)).astype(np.uint8)                              # truncating
    nmaps = v.shape[0]
    xmaps, ymaps = grid_shape(nmaps, nrow)                                         # step 5
    out = np.zeros((ymaps * H, xmaps * W, 3), np.uint8)
    for m in range(nmaps):
        cy, cx = divmod(m, xmaps)
        out[cy * H:(cy + 1) * H, cx * W:(cx + 1) * W] = u[m].transpose(1, 2, 0)    # step 7: interleaved
    return out


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
POISON = (F(1e6), F(-1e6), F(np.nan))          # what the images beyond nrow hold: they must not count


def mixed_batches(seed, H, W, specs, nrow, constant=None):
    """One logical (B, C, H, W) fp32 array per spec (B, C, layout): values in (-1, 1) -- or `constant` everywhere -- with
    the minimum of everything used, -3, as the first element of the first image and the maximum, 3, as the last element
    of the last image used.  Images past the first min(B, nrow) of a tensor hold POISON."""
    rng = np.random.RandomState(seed)
    out = []
    for B, C, _ in specs:
        if constant is None:
            x = rng.uniform(-1.0, 1.0, (B, C, H, W)).astype(F)
        else:
            x = np.full((B, C, H, W), constant, F)
        for b in range(min(B, nrow), B):
            x[b] = np.resize(np.array(POISON, F), (C, H, W))
        out.append(x)
    if constant is None:
        out[0][0, 0, 0, 0] = F(-3.0)
        out[-1][min(specs[-1][0], nrow) - 1, -1, -1, -1] = F(3.0)
    return out


def lattice_values():
    """For every k in 0..254 the fp32 nearest (k + 0.5) / 255 and its two neighbours -- where t * 255 + 0.5 crosses from
    byte k to k + 1 -- then 0 and 1: 767 values in [0, 1]."""
    c = (np.arange(255, dtype=np.float64) + 0.5) / 255.0
    c = c.astype(F)
    vals = np.stack([np.nextafter(c, F(-1.0)), c, np.nextafter(c, F(2.0))], 1).reshape(-1)
    return np.concatenate([vals, np.array([0.0, 1.0], F)]).astype(F)


def lattice_batches(lo, hi, H=8, W=8):
    """Two (2, 3, H, W) arrays holding lo + v * (hi - lo), in fp32, for the lattice values v (767 of the 768 elements; the
    last repeats hi): with lo, hi = 0, 1 the values themselves."""
    v = lattice_values()
    x = (F(lo) + (v * F(F(hi) - F(lo))).astype(F)).astype(F)
    x[-2], x[-1] = F(lo), F(hi)
    assert 4 * 3 * H * W >= x.size
    x = np.concatenate([x, np.full(4 * 3 * H * W - x.size, F(hi), F)])
    assert x.min() == F(lo) and x.max() == F(hi)
    x = x.reshape(4, 3, H, W)
    return [x[:2].copy(), x[2:].copy()]
