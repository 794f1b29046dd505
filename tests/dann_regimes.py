"""The launch regimes of munit_amd/csrc/dann.hip's batch norm and pools -- TEST INFRASTRUCTURE ONLY, not a test module.

munit_batchnorm_fwd / _bwd lay a block of 256 threads over C / 4 channel quads x rl = 256 / (C / 4) row lanes, cut the R
rows into bn_blocks(R, C) <= 64 blocks of per = ceil(R / nb) rows (block b owns [b per, min((b + 1) per, R)), lane l of it
the rows r0 + l, r0 + l + rl, ...), finish the per-block partials with ceil(C / 256) blocks of one thread per channel, and
run the apply and dx kernels as grid-stride loops over R * C / 4 quads on at most 16384 blocks.  This module restates that
geometry (`regime`), lists the cases of tests/test_gpu_dann_regimes.py with the reason each is there, and holds a numpy
model of the partition with a `variant` argument: the faithful variant visits every row once, the others are the mistakes
the exact checks on integer-lattice data have to catch.  The model exists only to prove on the CPU that the case list
discriminates (tests/test_cpu_dann_regimes.py); no GPU test compares against it.  The restatement is pinned to the library
by the GPU file: the number of partial rows a launch leaves in a poisoned workspace is bn_blocks(R, C)."""
import numpy as np

NT = 256
BN_MAX_BLOCKS = 64
BN_MAX_C = 1024
GRID_CAP_BLOCKS = 16384
GRID_CAP = GRID_CAP_BLOCKS * NT                       # quads one trip of a grid-stride loop covers


def accepted_c():
    """Every C bn_check accepts: a multiple of 4 up to 1024 whose quarter divides 256."""
    return [c for c in range(4, BN_MAX_C + 1, 4) if NT % (c // 4) == 0]


def rl(C):
    return NT // (C // 4)


def bn_blocks(R, C):
    return max(1, min(BN_MAX_BLOCKS, -(-R // (8 * rl(C)))))


def per(R, C, nb=None):
    nb = bn_blocks(R, C) if nb is None else nb
    return -(-R // nb)


def finishing_blocks(C):
    return -(-C // NT)


def grid_blocks(quads):
    return max(1, min(-(-quads // NT), GRID_CAP_BLOCKS))


def wraps(quads):
    """A grid-stride loop over `quads` items takes a second trip."""
    return quads > GRID_CAP


def align256(n):
    return (n + 255) // 256 * 256


def part_bytes(C):
    return align256(BN_MAX_BLOCKS * 2 * C * 4)


def workspace_bytes(C):
    return part_bytes(C) + align256(2 * C * 4)


def holding_blocks(R, C):
    """Blocks that own at least one row."""
    return -(-R // per(R, C))


def regime(R, C):
    """(lanes, rl, blocks, last, idle, finishing, wrap) of one batch-norm launch.
    lanes: 1quad (C = 4: one quad, 256 row lanes) | mid | 1lane (C = 1024: 256 quads, one row lane, nothing to add over
    the lanes); rl: the number of row lanes itself -- the length of the in-block reduction and the row stride of a lane.
    blocks: one | multi | cap (nb = 1, between, 64).
    last: full (every block owns `per` rows) | short (the last block owns fewer) | absent (blocks that own no row exist; the
    last block that owns rows may be short as well).
    idle: some row lane of a block that owns rows gets no row (that block has fewer rows than lanes).
    finishing: one | multi (C > 256: the one-thread-per-channel kernels run over several blocks).
    wrap: the apply and dx kernels take a second trip of their grid-stride loop."""
    assert C in accepted_c() and R >= 1, (R, C)
    n, p, lanes_n = bn_blocks(R, C), per(R, C), rl(C)
    hold = holding_blocks(R, C)
    tail = R - (hold - 1) * p
    lanes = "1quad" if C == 4 else "1lane" if lanes_n == 1 else "mid"
    blocks = "one" if n == 1 else "cap" if n == BN_MAX_BLOCKS else "multi"
    last = "absent" if hold < n else "short" if tail < p else "full"
    return (lanes, lanes_n, blocks, last, tail < lanes_n, "multi" if finishing_blocks(C) > 1 else "one",
            wraps(R * (C // 4)))


# ----------------------------------------------------------------------------------------------------------------------
# case lists: every entry names the reason it is there, and every entry has a regime of its own
# (tests/test_cpu_dann_regimes.py), so dropping one leaves a regime without a test
# ----------------------------------------------------------------------------------------------------------------------
BN_CASES = [
    # the edges of what the entry points accept
    ((2, 4), "the smallest accepted R in training mode; one quad, 254 of the 256 row lanes idle"),
    ((257, 4), "one block; exactly one row lane takes a second row"),
    ((2049, 4), "the smallest two-block launch at C = 4 (1025 + 1024 rows): a short last block"),
    ((5, 1024), "one row lane per quad; the finishing kernels over 4 blocks"),
    ((9, 1024), "two blocks of 5 and 4 rows at one row lane"),
    ((513, 1024), "capped with per = 9: 57 blocks own rows, 7 own none"),
    ((1030, 512), "rl = 2; capped with per = 17: 60 full blocks, one of 10 rows, 3 that own none"),
    ((8193, 64), "the smallest launch past the cap's exact fit at the classifier's C = 64: per = 129, last block 66"),
    ((16385, 1024), "the smallest shape whose apply / dx grids wrap: 4 194 560 quads against 4 194 304"),
    # the smallest production call of every regime production reaches
    ((256, 512), "the smallest call of the segmentation head (crop 64, batch 1): 16 full blocks of 16 rows"),
    ((5400, 128), "the classifier's first block at 360x480, batch 2: capped, per = 85, last block 45"),
    ((256, 64), "the classifier's second block at crop 256, batch 1: two full blocks at 16 row lanes"),
    ((576, 64), "the classifier's second block at crop 384, batch 1: 5 blocks of 116 rows, the last of 112"),
    ((8192, 64), "the classifier's second block at crop 256, batch 32: the cap's exact fit, 64 blocks of 8 x 16 rows"),
    ((1024, 128), "the classifier's first block at crop 256, batch 1: 16 full blocks at 8 row lanes"),
    ((2700, 128), "the classifier's first block at 360x480, batch 1: 43 blocks of 63 rows, the last of 54"),
    ((4096, 128), "the classifier's first block at crop 256, batch 4: the cap's exact fit at 8 row lanes"),
    ((1024, 512), "the segmentation head at crop 64, batch 4: capped, two finishing blocks, no wrap"),
    ((36864, 512), "the segmentation head at crop 384, batch 4: the smallest production call whose apply / dx grids wrap"),
]
BN_SHAPES = [rc for rc, _ in BN_CASES]
BN_DEVICE_REFERENCE = [(16385, 1024), (36864, 512)]   # their fp64 reference is torch's on the device (not the code under test)
BN_LARGE_MEAN = [(3, 64), (1030, 512)]                # a channel mean of 100 against unit spread
BN_CONTRACT = [(513, 1024), (1030, 512), (2, 4)]      # the guard-band contract
BN_REFUSED_C = [0, 2, 6, 12, 2048]

# regimes no production call reaches that the kernel tests must still run, as (regime, why)
BN_EDGES = [
    (("1quad", 256, "one", "full", True, "one", False), "R = 2: fewer rows than row lanes"),
    (("1quad", 256, "one", "full", False, "one", False), "C = 4 with every lane busy, one block"),
    (("1quad", 256, "multi", "short", False, "one", False), "C = 4 over two blocks"),
    (("1lane", 1, "one", "full", False, "multi", False), "C = 1024: no reduction over lanes, four finishing blocks"),
    (("1lane", 1, "multi", "short", False, "multi", False), "C = 1024 over two unequal blocks"),
    (("1lane", 1, "cap", "absent", False, "multi", False), "the capped launch with blocks that own no row"),
    (("mid", 2, "cap", "absent", False, "multi", False), "empty blocks behind a short block, at the head's C"),
    (("mid", 16, "cap", "short", False, "one", False), "the first R past the cap's exact fit"),
    (("1lane", 1, "cap", "short", False, "multi", True), "the first quad count past the grid cap"),
]

MAXPOOL_SMALL = [(1, 2, 3, 4), (1, 3, 2, 12), (2, 3, 3, 4), (1, 5, 7, 1024)]          # (B, H, W, C)
MAXPOOL_WRAP = (4, 130, 130, 1024)                    # 4 326 400 output quads against 4 194 304: both passes wrap
AVG16_C = [4, 16, 256, 1024]
AVG16_HW = [(16, 16), (16, 31), (31, 16)]
AVG16_BWD_WRAP = (18, 31, 31, 1024)                   # 4 428 288 input quads


# ----------------------------------------------------------------------------------------------------------------------
# numpy model of the row partition
# ----------------------------------------------------------------------------------------------------------------------
VARIANTS = ("faithful", "last_block_dropped", "empty_blocks_read", "cap_ignored")


def visits(R, C, variant="faithful"):
    """How often each row index is added into the column sums by the partial kernels, as an int64 vector that reaches one
    block past whatever a variant can read (entries from R on are reads past the tensor).
    faithful            block b: [b per, min((b + 1) per, R)), lane l: r0 + l, r0 + l + rl, ...
    last_block_dropped  the last block that owns rows does not run (a grid one block short)
    empty_blocks_read   r1 = r0 + per where r0 >= R: a block that owns no row reads `per` rows past the tensor
    cap_ignored         `per` is computed from the uncapped block count ceil(R / (8 rl)) while only 64 blocks run"""
    assert variant in VARIANTS, variant
    lanes = rl(C)
    nb = bn_blocks(R, C)
    p = per(R, C)
    if variant == "cap_ignored":
        p = per(R, C, max(1, -(-R // (8 * lanes))))
    hold = -(-R // p)
    out = np.zeros(max(R, nb * p) + p, dtype=np.int64)
    for b in range(nb):
        if variant == "last_block_dropped" and b == min(hold, nb) - 1:
            continue
        r0 = b * p
        r1 = (b + 1) * p if (variant == "empty_blocks_read" and r0 >= R) else min((b + 1) * p, R)
        for l in range(lanes):
            out[r0 + l:max(r0 + l, r1):lanes] += 1
    return out


def model_column_sums(x, variant="faithful", past=7):
    """Integer column sums of the (R, C) integer array x under `variant`; rows past R read as the constant `past` (what
    lies behind a tensor is not zero)."""
    R, C = x.shape
    v = visits(R, C, variant)
    return v[:R] @ x.astype(np.int64) + past * int(v[R:].sum())


def structurally_affected(R, C, variant):
    """Whether `variant` visits the rows of (R, C) differently from the faithful model."""
    return not np.array_equal(visits(R, C, variant), visits(R, C))


def lattice_rows(R, C, seed):
    """(R, C) fp32 rows on the integer lattice -3..3 (tests/lattice.py): every fp32 partial sum of a column, of its
    differences from the first row and of a 16x16 window is an integer below 2^24, so it is exact in any order."""
    from tests.lattice import lattice
    return lattice((R, C), seed, range(-3, 4)).float()


# ----------------------------------------------------------------------------------------------------------------------
# the max-pool's rule on special values
# ----------------------------------------------------------------------------------------------------------------------
SPECIALS = (float("nan"), float("-inf"), float("inf"), -0.0, 0.0, 1.0, -1.0)


def special_windows(dtype=np.float64):
    """All 7^4 = 2401 windows (0,0) (0,1) (1,0) (1,1) over SPECIALS, as a (2401, 4) array."""
    v = np.array(SPECIALS, dtype=dtype)
    i = np.indices((7, 7, 7, 7)).reshape(4, -1).T
    return v[i]


def maxpool_rule(win, dy):
    """dann.hip's documented rule on (N, 4) windows: the first maximum in window order wins, and any NaN replaces the
    current best (so the LAST NaN of a window wins, and no number displaces a NaN).  Returns (value, winner, dx) with
    dx[n, k] = dy[n] where k won and +0 elsewhere."""
    best, idx = win[:, 0].copy(), np.zeros(win.shape[0], dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for k in range(1, 4):
            v = win[:, k]
            take = (v > best) | np.isnan(v)
            best = np.where(take, v, best)
            idx = np.where(take, k, idx)
    dx = np.where(np.arange(4)[None, :] == idx[:, None], dy[:, None], 0.0).astype(win.dtype)
    return best, idx, dx
