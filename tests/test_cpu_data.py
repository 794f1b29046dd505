"""Host logic of the input pipeline (no GPU): list readers, Resize size rule, epoch sharding, batch packing,
and the data oracle's own invariants."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from munit_amd import data as D            # noqa: E402
from munit_amd._lib import ImageDesc       # noqa: E402
from oracle import data_oracle as O        # noqa: E402


def test_resize_size_rule_matches_oracle():
    for (w, h, s) in [(1024, 768, 256), (300, 500, 256), (256, 400, 256), (400, 256, 256), (256, 256, 256),
                      (77, 113, 64), (113, 77, 200), (500, 500, 100), (640, 480, None)]:
        rs = O.resize_size(w, h, s)
        want = (w, h) if rs is None else rs
        assert D.resize_size(w, h, s) == want


def test_list_readers(tmp_path):
    f = tmp_path / "l.txt"
    f.write_text("a/b.png\n c.jpg  extra\n")
    assert D.default_flist_reader(str(f)) == ["a/b.png", "c.jpg  extra"]
    assert D.default_txt_reader(str(f)) == [["a/b.png"], ["c.jpg", "extra"]]


def test_make_dataset_recurses_and_filters(tmp_path):
    (tmp_path / "sub").mkdir()
    for n in ("x.png", "y.txt", "sub/z.JPG", "sub/w.gif"):
        (tmp_path / n).write_bytes(b"0")
    got = sorted(os.path.relpath(p, tmp_path) for p in D.make_dataset(str(tmp_path)))
    assert got == ["sub/z.JPG", "x.png"]
    with pytest.raises(AssertionError):
        D.make_dataset(str(tmp_path / "missing"))


def test_shard_indices_partition_and_drop_last():
    full = D.shard_indices(23, 4, True, 5)
    assert len(full) == 5 and all(len(b) == 4 for b in full)
    flat = [i for b in full for i in b]
    assert len(set(flat)) == 20 and set(flat) <= set(range(23))
    assert D.shard_indices(23, 4, True, 5) == full                # same seed, same epoch order
    assert D.shard_indices(23, 4, True, 6) != full
    r0 = D.shard_indices(23, 4, True, 5, 0, 2)
    r1 = D.shard_indices(23, 4, True, 5, 1, 2)
    a = {i for b in r0 for i in b}
    b = {i for b in r1 for i in b}
    assert not (a & b) and len(r0) == len(r1) == 2                # disjoint shards of the same permutation
    assert D.shard_indices(10, 3, False, 0) == [[0, 1, 2], [3, 4, 5], [6, 7, 8]]


def test_draw_order_and_bounds():
    ld = D.DeviceBatchLoader(["a"] * 4, None, 2, True, 256, 256, 256, rank=0, world_size=1)
    rng = random.Random(3)
    ref = random.Random(3)
    flip, rs_h, rs_w, i, j, th, tw = ld.draw(1024, 768, rng)
    assert flip == (1 if ref.random() < 0.5 else 0)
    assert (rs_w, rs_h) == (341, 256) and (th, tw) == (256, 256)
    assert i == 0                                               # height already equals the crop: no draw consumed
    assert j == ref.randint(0, 341 - 256)
    test = D.DeviceBatchLoader(["a"], None, 1, False, 256, 256, 256, rank=0, world_size=1)
    assert test.draw(300, 300, random.Random(0))[0] == 0        # no flip outside training
    with pytest.raises(ValueError):
        D.DeviceBatchLoader(["a"], None, 1, True, 128, 256, 256, rank=0, world_size=1).draw(300, 300, random.Random(0))


def test_pack_batch_layout():
    arrays = [np.zeros((5, 7, 3), np.uint8), np.zeros((4, 4, 3), np.uint8)]
    masks = [np.zeros((5, 7), np.uint8), np.zeros((9, 3), np.uint8)]
    draws = [(1, 5, 7, 0, 1, 4, 4), (0, 4, 4, 0, 0, 4, 4)]
    descs, offs, moffs, total = D.pack_batch(arrays, masks, draws)
    assert ctypes.sizeof(ImageDesc) == 40
    assert offs[0] == 256 and offs[1] == 256 + 112 and all(o % 16 == 0 for o in offs + moffs)
    assert moffs[0] >= offs[1] + 48 and total >= moffs[1] + 27
    assert (descs[0].src_h, descs[0].src_w, descs[0].flip, descs[0].crop_j) == (5, 7, 1, 1)
    assert (descs[3].src_h, descs[3].src_w, descs[3].src_off) == (9, 3, moffs[1])


def test_pack_batch_without_masks_still_reserves_the_mask_descriptors():
    arrays = [np.zeros((5, 7, 3), np.uint8), np.zeros((4, 4, 3), np.uint8)]
    draws = [(1, 5, 7, 0, 1, 4, 4), (0, 4, 4, 0, 0, 4, 4)]
    descs, offs, moffs, total = D.pack_batch(arrays, None, draws)
    assert len(descs) == 4 and bytes(descs)[2 * ctypes.sizeof(ImageDesc):] == bytes(2 * ctypes.sizeof(ImageDesc))
    assert moffs == [] and offs[0] == 256 and offs == [256, 256 + 112] and total == 256 + 112 + 48
    assert (descs[1].src_off, descs[1].rs_h, descs[1].rs_w, descs[1].kind) == (offs[1], 4, 4, 0)


def test_pack_batch_mask_descriptors_carry_the_draw_but_no_resized_size():
    arrays = [np.zeros((5, 7, 3), np.uint8), np.zeros((4, 4, 3), np.uint8)]
    masks = [np.zeros((5, 7), np.uint8), np.zeros((9, 3), np.uint8)]
    draws = [(1, 5, 7, 0, 1, 4, 4), (0, 6, 5, 2, 1, 4, 4)]
    descs, offs, moffs, total = D.pack_batch(arrays, masks, draws)
    assert len(descs) == 4 and len(moffs) == 2
    for b, (m, d) in enumerate(zip(masks, draws)):
        md = descs[2 + b]
        assert (md.rs_h, md.rs_w, md.kind) == (0, 0, 0)
        assert (md.crop_i, md.crop_j, md.flip) == (d[3], d[4], d[0])
        assert (md.src_h, md.src_w, md.src_off) == (m.shape[0], m.shape[1], moffs[b])
        assert (descs[b].rs_h, descs[b].rs_w) == (d[1], d[2])           # the image descriptors do carry it


def _mask_batch(rng):
    """2 images + 2 masks with different source sizes, as launch_transform stages them."""
    arrays = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((5, 7), (9, 4))]
    masks = [rng.randint(0, 256, (h, w)).astype(np.uint8) for h, w in ((6, 3), (5, 11))]
    draws = [(1, 5, 7, 0, 1, 4, 4), (0, 9, 4, 3, 0, 4, 4)]
    return D._image_groups(arrays, masks), 1, draws, arrays + masks


def _synth_batch(rng):
    """3 synthetic samples with the sizes of test_cpu_synth_data.test_packed_batch_layout."""
    sizes, psizes = [(37, 53), (64, 48), (90, 61)], [(20, 31), (97, 70), (90, 61)]
    cols = [[rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes] for _ in range(2)]
    cols += [[rng.randint(0, 256, (h, w)).astype(np.uint8) for h, w in psizes] for _ in range(3)]
    draws = [(1, 45, 32, 3, 0, 24, 20), (0, 32, 42, 8, 22, 24, 20), (1, 47, 32, 0, 5, 24, 20)]
    return D._synth_groups(*cols), 2, draws, [a for col in cols for a in col]


@pytest.mark.parametrize("batch", [_mask_batch, _synth_batch])
def test_host_half_of_the_launch_fills_a_plain_buffer(batch):
    groups, n_img, draws, payloads = batch(np.random.RandomState(1))
    descs, offs, total, th, tw = D._lay_out(groups, n_img, draws, "unequal crop sizes")
    assert (th, tw) == draws[0][5:] and len(offs) == len(payloads) == len(descs)
    buf = np.full(total + 64, 0xA5, np.uint8)
    D._fill(buf, descs, offs, groups)
    head = bytes(descs)
    assert buf[:len(head)].tobytes() == head
    written = np.zeros(total + 64, bool)
    written[:len(head)] = True
    for d, o, a in zip(descs, offs, payloads):                         # payloads in descriptor order
        assert d.src_off == o and o % 16 == 0 and o >= (len(head) + 255) // 256 * 256
        assert np.array_equal(buf[o:o + a.nbytes], a.reshape(-1))
        assert not written[o:o + a.nbytes].any()
        written[o:o + a.nbytes] = True
    assert written[:total].sum() == len(head) + sum(a.nbytes for a in payloads)
    assert (buf[~written] == 0xA5).all() and not written[total:].any()  # gaps and everything from `total` on: untouched


def test_launch_transform_refuses_bad_batches_on_the_host():
    """Every refusal comes from the host half: no device, stream or library call is reached (device and stream are None)."""
    good = np.zeros((8, 8, 3), np.uint8)
    draw = (0, 8, 8, 0, 0, 8, 8)

    def launch(arrays, draws, masks=None):
        return D.launch_transform(arrays, masks, draws, None, None)

    with pytest.raises(ValueError, match=r"images must be uint8 \(H, W, 3\) arrays"):
        launch([good.astype(np.float32)], [draw])
    with pytest.raises(ValueError, match=r"images must be uint8 \(H, W, 3\) arrays"):
        launch([good, np.zeros((8, 8), np.uint8)], [draw, draw])
    with pytest.raises(ValueError, match="crop=False needs equally sized images inside a batch"):
        launch([good, good], [draw, (0, 8, 8, 0, 0, 8, 7)])
    for outside in ((0, 8, 8, 1, 0, 8, 8), (0, 8, 8, 0, 1, 8, 8), (0, 8, 8, -1, 0, 8, 8), (0, 8, 8, 0, -1, 8, 8)):
        with pytest.raises(ValueError, match=r"crop window \(-?\d,-?\d,8,8\) outside the resized image \(8,8\)"):
            launch([good, good], [draw, outside], masks=[good[:, :, 0], good[:, :, 0]])


def test_loader_refuses_cpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    ld = D.DeviceBatchLoader(["a.png"], None, 1, False, None, 4, 4, rank=0, world_size=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        iter(ld).__next__()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.transform_batch([np.zeros((4, 4, 3), np.uint8)], None, [(0, 4, 4, 0, 0, 4, 4)])


def test_oracle_identity_and_range():
    from PIL import Image
    rng = np.random.RandomState(0)
    arr = rng.randint(0, 256, (40, 60, 3)).astype(np.uint8)
    t = O.transform_image(Image.fromarray(arr), False, None, None)
    want = (torch.from_numpy(arr).permute(2, 0, 1).float() / 255 - 0.5) / 0.5
    assert torch.equal(t, want) and t.min() >= -1 and t.max() <= 1
    tf = O.transform_image(Image.fromarray(arr), True, None, (3, 5, 20, 30))
    assert torch.equal(tf, want.flip(2)[:, 3:23, 5:35])
    m = (rng.rand(40, 60) > 0.5).astype(np.uint8)
    mt = O.transform_mask(Image.fromarray(m), False, (0, 0, 40, 60))
    assert torch.equal(mt[0], torch.from_numpy(m).float() / 255 * 255)
