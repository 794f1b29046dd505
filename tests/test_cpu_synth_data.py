"""CPU: the host side of the synthetic paired loader (munit_amd.data.get_synthetic_data_loader) -- the label table
against the reference's own mapping (tests/golden/golden_synth_data.json), the public signature, the host refusals, the
layout of a packed batch, length and sharding, the new C symbols and the refusal to iterate without a device."""
import ctypes
import inspect
import json
import os
import random
import re
from ctypes import c_size_t, c_void_p

import numpy as np
import pytest
import torch

from munit_amd import data as D
from munit_amd import utils as U
from tests import synth_data_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("munit_label_preprocess_workspace_bytes", "munit_label_preprocess")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "golden_synth_data.json")) as f:
        return json.load(f)


def test_float_chain_returns_every_grey_value(golden):
    """to_tensor(x) * 255 in fp32 gives back every byte, in torch and in numpy: the reference's equality tests in mapping()
    see whole numbers, so an integer table is its float chain."""
    v = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(v.float().div(255) * 255, v.float())
    n = np.arange(256, dtype=np.uint8).astype(np.float32)
    assert np.array_equal(n / np.float32(255) * np.float32(255), n)
    assert golden["input"] == v.float().tolist()


def test_label_table_equals_the_reference_mapping(golden):
    assert len(D.LABEL_TABLE) == 256
    assert [float(t) for t in D.LABEL_TABLE] == golden["mapped"]
    mapped = [v for v in range(256) if D.LABEL_TABLE[v] != v]
    assert mapped == sorted(k for k in D.LABEL_CLASSES if k) and D.LABEL_TABLE[0] == 0


def test_utils_mapping_equals_the_golden_and_works_in_place(golden):
    x = torch.tensor(golden["input"], dtype=torch.float32).view(1, 16, 16)
    y = U.mapping(x)
    assert y is x and x.flatten().tolist() == golden["mapped"]
    assert SO.mapping(torch.tensor(golden["input"])).tolist() == golden["mapped"]      # the test oracle's restatement


def test_signature_is_the_reference_s():
    sig = inspect.signature(D.get_synthetic_data_loader)
    names = list(sig.parameters)
    assert names[:12] == ["file_list_a", "file_list_b", "mask_list", "sem_list_a", "sem_list_b", "batch_size", "train",
                          "new_size", "height", "width", "num_workers", "crop"]
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(new_size=256, height=256, width=256, num_workers=4, crop=True)
    assert sig.parameters[names[-1]].kind is inspect.Parameter.VAR_KEYWORD and len(names) == 13


def _files(tmp_path, sizes, plane_sizes=None, n_lists=5):
    """PNG files of the given (w, h) sizes and the five list files; returns (list paths, per-list file paths)."""
    from PIL import Image
    rng = np.random.RandomState(3)
    names = ("a", "b", "mask", "sema", "semb")
    paths = {n: [] for n in names}
    for k, (w, h) in enumerate(sizes):
        pw, ph = (w, h) if plane_sizes is None else plane_sizes[k]
        for n in names:
            p = tmp_path / ("%s%d.png" % (n, k))
            if n in ("a", "b"):
                Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(p)
            else:
                Image.fromarray(rng.randint(0, 256, (ph, pw)).astype(np.uint8)).save(p)
            paths[n].append(str(p))
    lists = []
    for n in names[:n_lists]:
        f = tmp_path / (n + ".txt")
        f.write_text("".join(p + " extra_column\n" for p in paths[n]))
        lists.append(str(f))
    return lists, paths


def _loader(lists, batch=2, **kw):
    kw.setdefault("rank", 0)
    kw.setdefault("world_size", 1)
    return D.get_synthetic_data_loader(lists[0], lists[1], lists[2], lists[3], lists[4], batch, True, **kw)


def test_lists_of_different_length_are_refused(tmp_path):
    lists, paths = _files(tmp_path, [(40, 36)] * 3)
    short = tmp_path / "short.txt"
    short.write_text(paths["semb"][0] + "\n")
    for pos in range(5):
        bad = list(lists)
        bad[pos] = str(short)
        with pytest.raises(ValueError, match="differ in length"):
            _loader(bad, new_size=32, height=24, width=20)


def test_pair_of_different_sizes_is_refused_and_names_both_files(tmp_path):
    from PIL import Image
    lists, paths = _files(tmp_path, [(40, 36), (40, 36)])
    Image.fromarray(np.zeros((36, 41, 3), np.uint8)).save(paths["b"][1])
    ld = _loader(lists, new_size=32, height=24, width=20)
    rng = random.Random(0)
    ld.draw_batch([0], [ld.decode_sample(0)], rng)
    with pytest.raises(ValueError) as e:
        ld.draw_batch([0, 1], [ld.decode_sample(0), ld.decode_sample(1)], rng)
    assert paths["a"][1] in str(e.value) and paths["b"][1] in str(e.value) and "differ in size" in str(e.value)


def test_crop_larger_than_the_resized_image_is_refused(tmp_path):
    lists, _ = _files(tmp_path, [(40, 36)])
    for h, w in ((33, 20), (24, 36)):            # resized image: 32 rows, int(32 * 40 / 36) = 35 columns
        ld = _loader(lists, batch=1, new_size=32, height=h, width=w)
        with pytest.raises(ValueError, match="larger than the resized image"):
            ld.draw_batch([0], [ld.decode_sample(0)], random.Random(0))
    ld = _loader(lists, batch=1, new_size=32, height=32, width=35)
    assert ld.draw_batch([0], [ld.decode_sample(0)], random.Random(0))[0][1:] == (32, 35, 0, 0, 32, 35)


def test_flip_is_drawn_whatever_train_says_and_crop_is_ignored(tmp_path):
    lists, _ = _files(tmp_path, [(40, 36)])
    for train in (True, False):
        for crop in (True, False):
            ld = D.get_synthetic_data_loader(*lists, 1, train, 32, 24, 20, 2, crop, rank=0, world_size=1, seed=5)
            rng = random.Random(1)
            draws = [ld.draw_batch([0], [ld.decode_sample(0)], rng)[0] for _ in range(40)]
            assert {d[0] for d in draws} == {0, 1}
            assert all(d[5:] == (24, 20) and 0 <= d[3] <= 8 and 0 <= d[4] <= 15 for d in draws)
            # the order of the draws: flip, then row, then column of the crop corner
            replay = random.Random(1)
            first = (1 if replay.random() < 0.5 else 0, replay.randint(0, 8), replay.randint(0, 15))
            assert (draws[0][0], draws[0][3], draws[0][4]) == first


def test_decode_converts_to_rgb_and_l(tmp_path):
    """A palette file is read through its palette (`.convert("L")`), not as raw indices."""
    from PIL import Image
    lists, paths = _files(tmp_path, [(12, 10)])
    pal = Image.fromarray(np.arange(120, dtype=np.uint8).reshape(10, 12) % 3, mode="P")
    pal.putpalette([0, 0, 0, 200, 200, 200, 255, 255, 255] + [0] * (253 * 3))
    pal.save(paths["sema"][0])
    Image.fromarray(np.full((10, 12), 77, np.uint8)).save(paths["a"][0])          # a grey file as image_a
    ld = _loader(lists, batch=1, new_size=10, height=8, width=8)
    a, b, m, sa, sb = ld.decode_sample(0)
    assert a.shape == (10, 12, 3) and a.dtype == np.uint8 and int(a.min()) == int(a.max()) == 77
    assert b.shape == (10, 12, 3) and m.shape == sa.shape == sb.shape == (10, 12)
    assert sorted(np.unique(sa).tolist()) == [0, 200, 255]


def test_packed_batch_layout():
    rng = np.random.RandomState(0)
    B = 3
    sizes = [(37, 53), (64, 48), (90, 61)]
    psizes = [(20, 31), (97, 70), (90, 61)]
    ia = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    ib = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    planes = [[rng.randint(0, 256, (h, w)).astype(np.uint8) for h, w in psizes] for _ in range(3)]
    draws = [(1, 45, 32, 3, 0, 24, 20), (0, 32, 42, 8, 22, 24, 20), (1, 47, 32, 0, 5, 24, 20)]
    descs, offs, total = D.pack_synth_batch(ia, ib, planes[0], planes[1], planes[2], draws)
    assert len(descs) == 5 * B and len(offs) == 5 * B
    items = ia + ib + planes[0] + planes[1] + planes[2]
    spans = []
    for n, (d, o, a) in enumerate(zip(descs, offs, items)):
        g, b = divmod(n, B)
        flip, rs_h, rs_w, i, j, _, _ = draws[b]
        # one draw reaches all five descriptors of a sample; the planes carry the resized IMAGE's size
        assert (d.flip, d.rs_h, d.rs_w, d.crop_i, d.crop_j) == (flip, rs_h, rs_w, i, j), n
        assert (d.src_h, d.src_w) == a.shape[:2] and d.src_off == o
        assert d.kind == (D.KIND_LABEL if g >= 3 else D.KIND_MASK) and (g < 3 or d.kind == 1) and (g != 2 or d.kind == 0)
        assert o % 16 == 0 and o >= 5 * B * ctypes.sizeof(D.ImageDesc)
        spans.append((o, o + a.nbytes))
    spans.sort()
    assert all(e <= s for (_, e), (s, _) in zip(spans, spans[1:])) and spans[-1][1] <= total
    assert ctypes.sizeof(D.ImageDesc) == 40          # the layout munit_image_preprocess reads is unchanged


def test_launch_synth_transform_refuses_bad_batches_on_the_host():
    """Every refusal comes from the host half: no device, stream or library call is reached (device and stream are None)."""
    img, plane = np.zeros((8, 8, 3), np.uint8), np.zeros((5, 6), np.uint8)
    draw = (0, 8, 8, 0, 0, 8, 8)

    def launch(draws=(draw, draw), **bad):
        cols = dict(a=[img, img], b=[img, img], mask=[plane, plane], sem_a=[plane, plane], sem_b=[plane, plane])
        for name, x in bad.items():
            cols[name] = [cols[name][0], x]
        return D.launch_synth_transform(cols["a"], cols["b"], cols["mask"], cols["sem_a"], cols["sem_b"], list(draws), None,
                                        None)

    for name in ("a", "b"):
        with pytest.raises(ValueError, match=r"images must be uint8 \(H, W, 3\) arrays"):
            launch(**{name: img.astype(np.float32)})
    with pytest.raises(ValueError, match=r"images must be uint8 \(H, W, 3\) arrays"):
        launch(a=img[:, :, 0], b=img[:, :, 0])
    with pytest.raises(ValueError, match="every sample of a batch needs the same crop size"):
        launch(draws=(draw, (0, 8, 8, 0, 0, 7, 8)))
    for outside in ((0, 8, 8, 1, 0, 8, 8), (0, 8, 8, 0, 1, 8, 8), (0, 8, 8, -1, 0, 8, 8), (0, 8, 8, 0, -1, 8, 8)):
        with pytest.raises(ValueError, match=r"crop window \(-?\d,-?\d,8,8\) outside the resized image \(8,8\)"):
            launch(draws=(draw, outside))
    with pytest.raises(ValueError, match=r"the images of a synthetic pair differ in size: \(8, 8\) vs \(8, 9\)"):
        launch(b=np.zeros((8, 9, 3), np.uint8))
    for name in ("mask", "sem_a", "sem_b"):
        for bad in (np.zeros((0, 6), np.uint8), np.zeros((5, 6, 1), np.uint8), plane.astype(np.float32)):
            with pytest.raises(ValueError, match=r"masks and label maps must be non-empty uint8 \(H, W\) arrays"):
                launch(**{name: bad})


def test_len_and_sharding(tmp_path):
    lists, _ = _files(tmp_path, [(30, 30)] * 9)
    assert len(_loader(lists, batch=2, new_size=30, height=8, width=8)) == 4
    r0 = _loader(lists, batch=2, new_size=30, height=8, width=8, rank=0, world_size=2, seed=3)
    r1 = _loader(lists, batch=2, new_size=30, height=8, width=8, rank=1, world_size=2, seed=3)
    assert len(r0) == len(r1) == 2 and len(r0.dataset) == 9
    s0 = D.shard_indices(9, 2, True, r0.seed + r0.epoch, 0, 2)
    s1 = D.shard_indices(9, 2, True, r1.seed + r1.epoch, 1, 2)
    seen = [k for b in s0 + s1 for k in b]
    assert len(s0) == len(s1) == 2 and len(set(seen)) == 8 and set(seen) <= set(range(9))
    assert r0._rng.random() != r1._rng.random()          # each rank draws its own flips and crops


def test_new_symbols_in_header_and_library():
    import __graft_entry__ as g
    g.build()
    from munit_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "munit_hip.h")).read()
    declared = set(re.findall(r"\b(munit_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"int kind;", header) and "reserved;" not in header
    assert [f[0] for f in _lib.ImageDesc._fields_][-1] == "kind"


def test_entry_point_refuses_bad_arguments_on_the_host():
    """NULL pointers, non-positive sizes and a short workspace are refused before any launch (no GPU is touched: the
    pointers handed over are never dereferenced on the host)."""
    import __graft_entry__ as g
    g.build()
    from munit_amd import _lib
    lib = _lib.load()
    p = c_void_p(4096)
    need = lib.munit_label_preprocess_workspace_bytes(6, 24, 20)
    assert need >= 6 * (24 + 20 + 1) * 4 and need % 256 == 0

    def call(pool=p, descs=p, n=6, h=24, w=20, out=p, ws=p, nb=need):
        return lib.munit_label_preprocess(pool, descs, n, h, w, out, ws, c_size_t(nb), None)

    for kw in (dict(pool=None), dict(descs=None), dict(out=None), dict(ws=None)):
        assert call(**kw) == -1 and b"null pointer" in lib.munit_last_error()
    for kw in (dict(n=0), dict(n=-3), dict(h=0), dict(w=-1)):
        assert call(**kw) == -1 and b"bad shape" in lib.munit_last_error()
    assert call(nb=need - 1) == -2 and b"workspace" in lib.munit_last_error()


def test_iterating_without_a_device_raises(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    lists, _ = _files(tmp_path, [(30, 30)] * 2)
    ld = _loader(lists, batch=2, new_size=30, height=8, width=8)
    with pytest.raises(RuntimeError, match="no HIP device"):
        next(iter(ld))
    with pytest.raises(RuntimeError, match="no HIP device"):
        ld.dataset[0]
