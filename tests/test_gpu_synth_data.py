"""GPU: the synthetic paired loader -- munit_label_preprocess through the C ABI and munit_amd.data's synthetic chain
against the PIL + torch-CPU oracle of tests/synth_data_oracle.py.  Every comparison is exact (torch.equal): the plane
chain is integer work plus a table, the image chain is munit_image_preprocess's, bit-identical to Pillow."""
import ctypes
import os
import random
import sys
from ctypes import c_size_t, c_void_p

import numpy as np
import pytest
import torch
from PIL import Image

from munit_amd import _lib
from munit_amd import data as D
from oracle import data_oracle as DO
from tests import synth_data_oracle as SO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GRID_CAP = 8192 * 256                 # image.hip: grid_for caps the grid at 8192 workgroups of 256 threads
COLOURS = np.array([0, 29, 55, 76, 133, 149, 178, 200, 255], np.uint8)      # the simulator's label greys


# ------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------
def _pair(rng, h, w, rect):
    """(image_a, image_b, rect): b equals a outside rect = (r0, r1, c0, c1); inside it a < 128 and b = a + 128, so every
    positive-weight average over pixels of the rectangle differs."""
    a = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    r0, r1, c0, c1 = rect
    a[r0:r1, c0:c1] >>= 1
    b = a.copy()
    b[r0:r1, c0:c1] += 128
    return a, b


def _labels(rng, h, w):
    """A label map: blocks of the simulator's colours with some stray grey values that mapping() leaves alone."""
    m = COLOURS[rng.randint(0, len(COLOURS), (h, w))]
    stray = rng.rand(h, w) < 0.1
    m[stray] = rng.randint(0, 256, int(stray.sum())).astype(np.uint8)
    return m


def _support(in_size, rs_size, xx):
    """[lo, hi) of the source indices Pillow's BILINEAR resample may read for index xx of the resized axis."""
    if in_size == rs_size:
        return xx, xx + 1             # no Resize at all: the pixel itself
    scale = in_size / rs_size
    support = max(scale, 1.0)
    center = (xx + 0.5) * scale
    return max(int(center - support + 0.5), 0), min(int(center + support + 0.5), in_size)


def _rect_maps(src_h, src_w, draw, rect):
    """(touched, core) boolean (out_h, out_w) maps of a crop: output pixels whose resample window meets the rectangle of
    the (flipped) source, and those whose window lies inside it."""
    flip, rs_h, rs_w, i, j, th, tw = draw
    r0, r1, c0, c1 = rect
    if flip:
        c0, c1 = src_w - c1, src_w - c0
    rows = [_support(src_h, rs_h, i + y) for y in range(th)]
    cols = [_support(src_w, rs_w, j + x) for x in range(tw)]
    rt = np.array([lo < r1 and hi > r0 for lo, hi in rows])
    ct = np.array([lo < c1 and hi > c0 for lo, hi in cols])
    rc = np.array([lo >= r0 and hi <= r1 for lo, hi in rows])
    cc = np.array([lo >= c0 and hi <= c1 for lo, hi in cols])
    return np.outer(rt, ct), np.outer(rc, cc)


def _run(samples, draws):
    """launch_synth_transform on the current stream; samples[b] = (a, b, mask, sem_a, sem_b) uint8 arrays."""
    dev = torch.device(DEV)
    cols = list(zip(*samples))
    out, ev, keep = D.launch_synth_transform(cols[0], cols[1], cols[2], cols[3], cols[4], draws, dev,
                                             torch.cuda.current_stream(dev))
    ev.synchronize()
    return out


def _want(sample, draw, new_size):
    flip, rs_h, rs_w, i, j, th, tw = draw
    a, b, m, sa, sb = sample
    return SO.transform_synthetic(Image.fromarray(a), Image.fromarray(b), Image.fromarray(m), Image.fromarray(sa),
                                  Image.fromarray(sb), bool(flip), new_size, (i, j, th, tw))


def _check_batch(samples, draws, new_size):
    out = _run(samples, draws)
    B, th, tw = len(samples), draws[0][5], draws[0][6]
    x_as, x_bs, mask_s, sem_a, sem_b = out
    for x in (x_as, x_bs):
        assert x.shape == (B, 3, th, tw) and x.dtype == torch.float32
        assert x.is_contiguous(memory_format=torch.channels_last)
    for p in (mask_s, sem_a, sem_b):
        assert p.shape == (B, 1, th, tw) and p.dtype == torch.float32 and p.is_contiguous()
    names = ("x_as", "x_bs", "mask_s", "sem_a", "sem_b")
    for b, (s, d) in enumerate(zip(samples, draws)):
        assert DO.resized_hw(s[1].shape[1], s[1].shape[0], new_size) == (d[1], d[2])
        for name, got, want in zip(names, out, _want(s, d, new_size)):
            got = got[b].cpu()
            assert torch.equal(got, want), "%s of sample %d: %d elements differ" % (name, b, (got != want).sum().item())
    return out


def _planes(planes, kinds, params, out_h, out_w):
    """munit_label_preprocess straight through ctypes.  params[n] = (flip, rs_h, rs_w, crop_i, crop_j).
    Returns the (N, 1, out_h, out_w) result on the host."""
    lib = _lib.load()
    N = len(planes)
    offs, cur = [], 0
    for p in planes:
        offs.append(cur)
        cur += (p.size + 15) // 16 * 16
    pool = np.zeros(cur, np.uint8)
    descs = (_lib.ImageDesc * N)()
    for n, (p, k, (flip, rs_h, rs_w, i, j)) in enumerate(zip(planes, kinds, params)):
        pool[offs[n]:offs[n] + p.size] = p.reshape(-1)
        descs[n] = _lib.ImageDesc(offs[n], p.shape[0], p.shape[1], rs_h, rs_w, i, j, flip, k)
    dpool = torch.from_numpy(pool).to(DEV)
    ddesc = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(DEV)
    out = torch.full((N, 1, out_h, out_w), float("nan"), device=DEV)
    nws = lib.munit_label_preprocess_workspace_bytes(N, out_h, out_w)
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device=DEV)
    rc = lib.munit_label_preprocess(c_void_p(dpool.data_ptr()), c_void_p(ddesc.data_ptr()), N, out_h, out_w,
                                    c_void_p(out.data_ptr()), c_void_p(ws.data_ptr()), c_size_t(nws),
                                    c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "munit_label_preprocess")
    torch.cuda.synchronize()
    return out.cpu()


def _plane_want(plane, kind, param, out_h, out_w):
    flip, rs_h, rs_w, i, j = param
    fn = SO.transform_mask if kind == D.KIND_MASK else SO.transform_label
    return fn(Image.fromarray(plane), bool(flip), (rs_w, rs_h), (i, j, out_h, out_w))


def _check_planes(planes, kinds, params, out_h, out_w):
    got = _planes(planes, kinds, params, out_h, out_w)
    for n, (p, k, pr) in enumerate(zip(planes, kinds, params)):
        want = _plane_want(p, k, pr, out_h, out_w)
        assert torch.equal(got[n], want), "plane %d (kind %d): %d pixels differ" % (n, k, (got[n] != want).sum().item())
    return got


# ------------------------------------------------------------------------------------------------------------------
# 1, 2: the whole chain at explicit draws
# ------------------------------------------------------------------------------------------------------------------
def test_downscale_crop_flip_bit_exact_and_pair_alignment():
    """Three pairs of other sizes, new_size 32, crop 24 x 20; flips 1, 0, 1; corners at (0, 0), at the maximum and inside.
    The planes have other sizes than their image, at non-integer ratios (smaller, ~1.5x larger, and one of each per
    sample), so the accumulator tables decide the source pixel.  x_as equals x_bs exactly outside the transformed
    rectangle and nowhere inside it."""
    rng = np.random.RandomState(11)
    th, tw = 24, 20
    sizes = [(37, 53), (64, 48), (90, 61)]                       # (h, w): 53x37, 48x64, 61x90 as w x h
    rects = [(6, 30, 10, 40), (20, 52, 12, 36), (40, 70, 25, 50)]
    psizes = [[(20, 31), (23, 29), (37, 53)], [(97, 70), (95, 73), (41, 33)], [(133, 93), (57, 40), (61, 47)]]
    draws = [(1, 32, 45, 0, 0, th, tw), (0, 42, 32, 42 - th, 32 - tw, th, tw), (1, 47, 32, 11, 5, th, tw)]
    samples = []
    for (h, w), rect, ps in zip(sizes, rects, psizes):
        a, b = _pair(rng, h, w, rect)
        mask = (rng.rand(*ps[0]) > 0.5).astype(np.uint8) * 255
        samples.append((a, b, mask, _labels(rng, *ps[1]), _labels(rng, *ps[2])))
    x_as, x_bs, _, sem_a, _ = _check_batch(samples, draws, 32)
    diff = (x_as - x_bs).abs().sum(1).cpu().numpy()
    for b, ((h, w), rect, d) in enumerate(zip(sizes, rects, draws)):
        touched, core = _rect_maps(h, w, d, rect)
        assert (~touched).sum() > 20 and core.sum() > 20, (b, (~touched).sum(), core.sum())
        assert (diff[b][~touched] == 0).all(), "pair %d differs outside the transformed rectangle" % b
        assert (diff[b][core] != 0).all(), "pair %d is equal inside the transformed rectangle" % b
    classes = set(sem_a.cpu().unique().tolist())
    assert set(range(9)) <= classes and len(classes) > 9        # mapped colours and stray values that stay


def test_upscale_and_identity_bit_exact():
    """20 x 17 sources: new_size 40 (up-scaling by 40 / 17) and new_size 17, the short side (no Resize at all)."""
    rng = np.random.RandomState(12)
    h, w = 17, 20
    psizes = [[(17, 20), (11, 13), (26, 31)], [(9, 7), (17, 20), (40, 47)]]
    samples = []
    for ps in psizes:
        a, b = _pair(rng, h, w, (4, 12, 5, 15))
        mask = (rng.rand(*ps[0]) > 0.5).astype(np.uint8)           # 0 / 1 masks: the x255 branch
        samples.append((a, b, mask, _labels(rng, *ps[1]), _labels(rng, *ps[2])))
    assert DO.resized_hw(w, h, 40) == (40, 47)
    _check_batch(samples, [(1, 40, 47, 3, 9, 32, 36), (0, 40, 47, 8, 11, 32, 36)], 40)
    _check_batch(samples, [(0, 40, 47, 0, 0, 40, 47), (1, 40, 47, 0, 0, 40, 47)], 40)       # the whole resized image
    assert DO.resized_hw(w, h, 17) == (17, 20)
    _check_batch(samples, [(0, 17, 20, 2, 5, 12, 14), (1, 17, 20, 5, 6, 12, 14)], 17)


# ------------------------------------------------------------------------------------------------------------------
# 3, 4, 5: the plane kernel alone
# ------------------------------------------------------------------------------------------------------------------
def test_mask_rule():
    rng = np.random.RandomState(13)
    S, T = 30, 10
    window = (0, S, S, 5, 5)                                       # no resize; crop 10 x 10 at (5, 5)
    only01 = np.zeros((S, S), np.uint8)
    only01[5:15, 5:15] = rng.randint(0, 2, (T, T))
    only01[0, 0] = only01[29, 29] = only01[4, 5] = only01[15, 14] = 255       # outside the window: the rule looks at the crop
    edge = np.zeros((S, S), np.uint8)
    edge[:, 0::2], edge[:, 1::2] = 127, 128                        # 127 / 255 < 0.5 < 128 / 255
    zero = np.zeros((S, S), np.uint8)
    single = np.zeros((S, S), np.uint8)
    single[14, 14] = 1                                             # the last pixel of the window
    small = rng.randint(0, 3, (S, S)).astype(np.uint8)             # maximum 2: to_tensor only, everything below 0.5
    mixed = rng.randint(0, 256, (S, S)).astype(np.uint8)
    one255 = (rng.rand(S, S) > 0.5).astype(np.uint8)
    one255[10, 10] = 255                                           # {0, 1} with one 255 inside the window: the 1s are lost
    planes = [only01, edge, zero, single, small, mixed, one255]
    got = _check_planes(planes, [0] * len(planes), [window] * len(planes), T, T)
    assert set(got.unique().tolist()) == {0.0, 1.0}
    assert torch.equal(got[0, 0], torch.from_numpy(only01[5:15, 5:15].astype(np.float32)))
    assert torch.equal(got[1, 0], torch.from_numpy((edge[5:15, 5:15] == 128).astype(np.float32)))
    assert got[2].sum() == 0 and got[3].sum() == 1 and got[3, 0, 9, 9] == 1 and got[4].sum() == 0
    assert got[6].sum() == 1 and got[6, 0, 5, 5] == 1
    # the same planes flipped, through a resize to 45 x 41 and a window of other sides
    _check_planes(planes, [0] * len(planes), [(1, 41, 45, 7, 13, )] * len(planes), 23, 17)


def test_label_maps_all_grey_values():
    """One 16 x 16 plane holds all 256 grey values; resized up by 2 and down by 2, flipped and not."""
    plane = np.arange(256, dtype=np.uint8).reshape(16, 16)
    table = torch.tensor(D.LABEL_TABLE, dtype=torch.float32)
    up = _check_planes([plane, plane], [1, 1], [(0, 32, 32, 0, 0), (1, 32, 32, 0, 0)], 32, 32)
    assert torch.equal(up[0, 0, ::2, ::2], table.view(16, 16))                 # every value, mapped or kept
    assert torch.equal(up[0, 0, 1::2, 1::2], table.view(16, 16))
    assert torch.equal(up[1, 0], up[0, 0].flip(1))
    vals = set(up.unique().tolist())
    assert vals == set(float(t) for t in D.LABEL_TABLE) and len(vals) == 256 - 8      # eight colours fold onto 1..8
    down = _check_planes([plane, plane], [1, 1], [(0, 8, 8, 0, 0), (1, 8, 8, 0, 0)], 8, 8)
    assert torch.equal(down[0, 0], table.view(16, 16)[1::2, 1::2])
    # the same plane as a mask: maximum 255, so v >= 128 counts
    m = _check_planes([plane], [0], [(0, 32, 32, 0, 0)], 32, 32)
    assert torch.equal(m[0, 0, ::2, ::2], (torch.arange(256).view(16, 16) >= 128).float())


def test_grid_stride_wrap_and_reduction_across_workgroups():
    """Nine 64 x 64 planes resized to 512 x 512: more pixels than the capped grid has threads, so the last planes are
    written by the second trip of the grid-stride loop, and every mask's maximum is reduced across many workgroups."""
    rng = np.random.RandomState(14)
    N, S, T = 9, 64, 512
    assert N * T * T > GRID_CAP and 8 * T * T <= GRID_CAP          # plane 8 is entirely the second trip
    kinds = [1, 0, 0, 1, 0, 1, 1, 0, 0]
    planes = []
    for n, k in enumerate(kinds):
        planes.append(_labels(rng, S, S) if k else (rng.rand(S, S) > 0.5).astype(np.uint8) * 255)
    planes[2] = (rng.rand(S, S) > 0.5).astype(np.uint8)            # a 0 / 1 mask
    planes[7] = np.zeros((S, S), np.uint8)
    planes[7][63, 63] = 1                                          # maximum 1, seen by the last workgroups only
    planes[8] = np.zeros((S, S), np.uint8)
    planes[8][0, 0], planes[8][63, 63] = 1, 2                      # maximum 2 in the second trip: the 1 must NOT count
    params = [(n % 2, T, T, 0, 0) for n in range(N)]
    got = _check_planes(planes, kinds, params, T, T)
    assert got[7].sum() == 64 and got[8].sum() == 0 and got[2].sum() == 64 * int(planes[2].sum())


# ------------------------------------------------------------------------------------------------------------------
# 6: guard bands and bad arguments
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (6, 24, 20), (3, 7, 300), (5, 130, 129)], ids=lambda s: "n%d_%dx%d" % s)
def test_contract_label_preprocess(shape):
    """The contract of the other image entry points (tests/kernel_contract.check_image): every tensor between NaN guard
    bands, two poison payloads give the same NaN-free output, inputs and guards stay untouched, and every refusal -- a
    workspace one byte short, null pointers, non-positive sizes -- leaves the output and the workspace unwritten.  Some
    descriptors place the window partly outside the resized plane: those positions read nothing and give 0, as PIL's crop
    does."""
    from tests import kernel_contract as KC
    from tests.conv_contract import ERR_WORKSPACE, GUARD_BYTE, Arena, Launches, no_nan, poison, stream
    lib = _lib.load()
    N, out_h, out_w = shape
    rng = np.random.RandomState(15)
    srcs = [(out_h + 3 + 2 * n, max(1, out_w - 2 + 3 * n)) for n in range(N)]
    kinds = [n % 2 for n in range(N)]
    params = [(n % 2, out_h + 2 + n, out_w + 1 + n, n % 3, 1) for n in range(N)]      # flip, rs_h, rs_w, crop_i, crop_j
    if N > 2:
        params[1] = (1, out_h + 1, out_w + 1, -2, 4)              # above the top, past the right edge
        params[2] = (0, out_h, out_w - 1 if out_w > 1 else 1, 3, -1)      # past the bottom, left of the left edge
    planes = [rng.randint(0, 256, s).astype(np.uint8) for s in srcs]
    planes[0] = (planes[0] & 1).astype(np.uint8)                   # a 0 / 1 mask: the x255 branch
    offs, cur = [], 0
    for p in planes:
        offs.append(cur)
        cur += (p.size + 15) // 16 * 16
    descs = (_lib.ImageDesc * N)()
    host = np.zeros(cur, np.uint8)
    for n, (p, k, (fl, rh, rw, i, j)) in enumerate(zip(planes, kinds, params)):
        host[offs[n]:offs[n] + p.size] = p.reshape(-1)
        descs[n] = _lib.ImageDesc(offs[n], p.shape[0], p.shape[1], rh, rw, i, j, fl, k)
    nws = lib.munit_label_preprocess_workspace_bytes(N, out_h, out_w)
    a = Arena(dict(pool=cur, descs=N * ctypes.sizeof(_lib.ImageDesc), out=N * out_h * out_w * 4, ws=nws), torch.device(DEV))
    a.bytes("pool").copy_(torch.from_numpy(host).to(DEV))
    a.bytes("descs").copy_(torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(DEV))
    what = "label_preprocess %s" % (shape,)
    L = Launches(a, ["pool", "descs"], what)
    out = a.view("out", torch.float32)

    def call(pool="pool", dsc="descs", n=N, h=out_h, w=out_w, o="out", ws="ws", nb=nws):
        a.bytes("ws").fill_(GUARD_BYTE)
        return lib.munit_label_preprocess(a.ptr(pool) if pool else None, a.ptr(dsc) if dsc else None, n, h, w,
                                          a.ptr(o) if o else None, a.ptr(ws) if ws else None, c_size_t(nb), stream())

    res = []
    for k in (0, 1):
        poison(out, k)
        L.after(call(), "payload %d" % k)
        assert no_nan(out), what + ": NaN in the output (an element not written)"
        res.append(a.bytes("out").clone())
    assert torch.equal(res[0], res[1]), what + ": two runs differ"
    got = out.view(N, 1, out_h, out_w).cpu()
    for n, (p, k, pr) in enumerate(zip(planes, kinds, params)):
        want = _plane_want(p, k, pr, out_h, out_w)
        assert torch.equal(got[n], want), "%s plane %d: %d pixels differ" % (what, n, (got[n] != want).sum().item())
    refusals = [("workspace one byte short", dict(nb=nws - 1), ERR_WORKSPACE), ("pool = NULL", dict(pool=None), KC.ERR_ARG),
                ("descs = NULL", dict(dsc=None), KC.ERR_ARG), ("out = NULL", dict(o=None), KC.ERR_ARG),
                ("ws = NULL", dict(ws=None), KC.ERR_ARG), ("N = 0", dict(n=0), KC.ERR_ARG), ("N < 0", dict(n=-1), KC.ERR_ARG),
                ("out_h = 0", dict(h=0), KC.ERR_ARG), ("out_w < 0", dict(w=-5), KC.ERR_ARG)]
    for label, kw, code in refusals:
        poison(out, 0)
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc == code, (what, label, rc)
        assert lib.munit_last_error(), (what, label)
        assert KC.holds_poison(out), "%s: output written before the refusal (%s)" % (what, label)
        assert bool((a.bytes("ws") == GUARD_BYTE).all()), "%s: workspace written before the refusal (%s)" % (what, label)
        L.verify(label + " (refused)")


# ------------------------------------------------------------------------------------------------------------------
# 7, 8: the loader and the example
# ------------------------------------------------------------------------------------------------------------------
SIZE, BATCH = 64, 2                   # the smallest geometry of tests/test_gpu_synth.py


def _write_dataset(tmp_path, n, seed):
    """n synthetic samples as PNG files (images of other sizes with an aligned pair, planes of other sizes than their
    image) and the five list files.  Returns (list files, per-list paths)."""
    rng = np.random.RandomState(seed)
    names = ("a", "b", "mask", "sema", "semb")
    paths = {k: [] for k in names}
    for k in range(n):
        h, w = int(rng.randint(70, 100)), int(rng.randint(70, 110))
        a, b = _pair(rng, h, w, (h // 4, 3 * h // 4, w // 4, 3 * w // 4))
        ph, pw = int(rng.randint(40, 140)), int(rng.randint(40, 140))
        mask = np.kron((rng.rand(ph // 8 + 1, pw // 8 + 1) > 0.5), np.ones((8, 8)))[:ph, :pw].astype(np.uint8)
        mask = mask * (255 if k % 2 else 1)
        planes = {"a": a, "b": b, "mask": mask, "sema": COLOURS[rng.randint(0, 9, (ph, pw))],
                  "semb": COLOURS[rng.randint(0, 9, (h, w))]}
        for name in names:
            p = tmp_path / ("%s%d.png" % (name, k))
            Image.fromarray(planes[name]).save(p)
            paths[name].append(str(p))
    lists = []
    for name in names:
        f = tmp_path / (name + ".txt")
        f.write_text("".join(p + "\n" for p in paths[name]))
        lists.append(str(f))
    return lists, paths


def _oracle_batch(ld, paths, idx, replay, new_size):
    outs = []
    for k in idx:
        ims = [Image.open(paths[n][k]).convert("RGB" if n in ("a", "b") else "L") for n in ("a", "b", "mask", "sema", "semb")]
        flip, rs_h, rs_w, i, j, th, tw = ld.draw(ims[1].size[0], ims[1].size[1], replay)
        outs.append(SO.transform_synthetic(*ims, bool(flip), new_size, (i, j, th, tw)))
    return [torch.stack(c) for c in zip(*outs)]


def test_loader_end_to_end_feeds_the_synthetic_step(tmp_path):
    """Five samples in batches of two over two epochs (two batches each, one sample dropped), the random stream replayed
    on the host: every tensor is bit-equal to the oracle and is what the trainer accepts; one dis_update +
    gen_update(synth=True) on a loader batch gives finite losses and bit for bit the loss_gen_recon_synth of the same step
    fed the oracle's tensors."""
    from munit_amd.trainer import MUNIT_Trainer
    from oracle import munit_oracle as O
    lists, paths = _write_dataset(tmp_path, 5, 21)
    ld = D.get_synthetic_data_loader(*lists, BATCH, True, new_size=SIZE, height=SIZE, width=SIZE, num_workers=2, seed=13,
                                     rank=0, world_size=1)
    assert len(ld) == 2 and len(ld.dataset) == 5
    replay = random.Random()
    replay.setstate(ld._rng.getstate())
    first = None
    for epoch in range(2):
        order = D.shard_indices(5, BATCH, True, ld.seed + ld.epoch)
        n = 0
        for batch, idx in zip(ld, order):
            x_as, x_bs, mask_s, sem_a, sem_b = batch
            for x in (x_as, x_bs):
                assert x.shape == (BATCH, 3, SIZE, SIZE) and x.dtype == torch.float32 and x.device.type == "cuda"
                assert x.is_contiguous(memory_format=torch.channels_last)
            for p in (mask_s, sem_a, sem_b):
                assert p.shape == (BATCH, 1, SIZE, SIZE) and p.dtype == torch.float32 and p.is_contiguous()
            want = _oracle_batch(ld, paths, idx, replay, SIZE)
            for name, got, w in zip(("x_as", "x_bs", "mask_s", "sem_a", "sem_b"), batch, want):
                assert torch.equal(got.cpu(), w), "epoch %d batch %d: %s differs" % (epoch, n, name)
            assert set(mask_s.unique().tolist()) <= {0.0, 1.0} and int(sem_a.max()) <= 8
            gts = MUNIT_Trainer._check_semantic_gt(x_as, sem_a, sem_b)
            assert [tuple(g.shape) for g in gts] == [(BATCH, SIZE, SIZE)] * 2
            if first is None:
                first = (batch, want)
            n += 1
        assert n == 2
    one = ld.dataset[3]
    assert [tuple(t.shape) for t in one] == [(3, SIZE, SIZE)] * 2 + [(1, SIZE, SIZE)] * 3

    hp = O.default_hp(SIZE, BATCH, 1)
    hp["recon_synth_w"] = 1

    def step(x_as, x_bs, mask_s, sem_a, sem_b):
        torch.manual_seed(0)
        tr = MUNIT_Trainer(hp).to(DEV)
        torch.manual_seed(3)
        tr.dis_update(x_as, x_bs, hp)
        tr.gen_update(x_as, x_bs, hp, mask_s, mask_s, None, True, sem_a, sem_b)
        torch.cuda.synchronize()
        return tr

    got = step(*first[0])
    w = [t.to(DEV) for t in first[1]]
    ref = step(w[0].contiguous(memory_format=torch.channels_last), w[1].contiguous(memory_format=torch.channels_last), *w[2:])
    for name in ("loss_dis_total", "loss_gen_total", "loss_gen_recon_synth"):
        v = float(getattr(got, name))
        assert v == v and abs(v) != float("inf") and v > 0, (name, v)
    a, b = got.loss_gen_recon_synth.detach(), ref.loss_gen_recon_synth.detach()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (float(a), float(b))


def test_train_loop_example_runs_the_synthetic_iteration(tmp_path, monkeypatch):
    """examples/train_loop.py with the five list arguments: two iterations at 64 x 64, B = 2, the synthetic branch entered
    in each (a loader of one batch per epoch, so the second iteration needs the restart); without the arguments no
    synthetic iteration runs."""
    import yaml
    import bench
    from munit_amd.trainer import MUNIT_Trainer
    rng = np.random.RandomState(9)
    for dom in ("trainA", "trainB"):
        (tmp_path / dom).mkdir()
        for k in range(4):
            Image.fromarray(rng.randint(0, 256, (80 + k, 96, 3)).astype(np.uint8)).save(tmp_path / dom / ("i%d.png" % k))
    (tmp_path / "synth").mkdir()
    lists, _ = _write_dataset(tmp_path / "synth", 3, 22)
    hp = bench.bench_hp(SIZE, BATCH)
    hp.update(new_size=SIZE, data_root=str(tmp_path), num_workers=2, ratio_disc_gen=1, recon_synth_w=1,
              synthetic_frequency=1, synthetic_seg_gt=1)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump(hp))
    calls = []
    plain = MUNIT_Trainer.gen_update

    def gen_update(self, x_a, x_b, hp_, mask_a=None, mask_b=None, comet_exp=None, synth=False, semantic_gt_a=None,
                   semantic_gt_b=None):
        calls.append((bool(synth), semantic_gt_a is not None and semantic_gt_b is not None, tuple(x_a.shape)))
        return plain(self, x_a, x_b, hp_, mask_a, mask_b, comet_exp, synth, semantic_gt_a, semantic_gt_b)

    monkeypatch.setattr(MUNIT_Trainer, "gen_update", gen_update)
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_loop
    args = ["--config", str(cfg), "--iters", "2"]
    tr = train_loop.main(args + ["--synth-list-a", lists[0], "--synth-list-b", lists[1], "--synth-mask-list", lists[2],
                                 "--seg-list-a", lists[3], "--seg-list-b", lists[4]])
    assert tr.iterations == 1
    assert [c[0] for c in calls] == [False, True, False, True]
    assert all(c[1] for c in calls if c[0]) and all(c[2] == (BATCH, 3, SIZE, SIZE) for c in calls)
    v = float(tr.loss_gen_recon_synth)
    assert v == v and v > 0
    del calls[:]
    train_loop.main(args)
    assert [c[0] for c in calls] == [False, False]
    del calls[:]
    hp.update(data_list_train_a_synth=lists[0], data_list_train_b_synth=lists[1], data_list_train_b_seg_synth=lists[2],
              seg_list_a=lists[3], seg_list_b=lists[4])
    cfg.write_text(yaml.safe_dump(hp))
    train_loop.main(["--config", str(cfg), "--iters", "1"])     # the config keys alone select the loader
    assert [c[0] for c in calls] == [False, True]
