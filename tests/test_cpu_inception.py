"""Host-side checks of the Inception-v3 feature trunk (munit_amd/inception.py, csrc/inception.hip, inception_utils): the
architecture table against its three pins, the oracle against the reference's fixture, the batch-norm fold, the state-dict
ingestion, the C ABI's declarations and refusals (no device: the pointers are never followed) and the example loop's cadence."""
import json
import os
import re
import sys
from ctypes import byref, c_int, c_void_p

import pytest
import torch
import torch.nn.functional as F

from tests import inception_oracle as IO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_BOUND = 1e-9          # the project's bound on a fixture reproduced in fp64
NEW_SYMBOLS = ("munit_conv2d_rect_out_hw", "munit_conv2d_rect_tile", "munit_conv2d_rect_fwd", "munit_window3_fwd",
               "munit_inception_input")
FORMS = [(3, 3, 2, 0, 0), (3, 3, 1, 0, 0), (3, 3, 1, 1, 1), (1, 1, 1, 0, 0), (5, 5, 1, 2, 2),
         (1, 7, 1, 0, 3), (7, 1, 1, 3, 0), (1, 3, 1, 0, 1), (3, 1, 1, 1, 0)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from munit_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def state():
    return IO.random_state(0)


@pytest.fixture(scope="module")
def oracle_runs(state):
    """{case: (features fp64, stage shapes)} of the fixture's two inputs -- computed once."""
    net = IO.blocks(state, torch.float64)
    with torch.no_grad():
        return {name: IO.trunk(net, IO.input_lines(x)) for name, x in IO.fixture_inputs().items()}


# ---- the table ---------------------------------------------------------------------------------------------------------
def test_table_rows_parameters_and_oracle_copy():
    from munit_amd import inception as I
    assert len(I.INCEPTION_CONVS) == 94 and len({r[0] for r in I.INCEPTION_CONVS}) == 94
    assert I.parameter_count() == 21785568 == 27161264 - 2049000 - 3326696
    assert sum(r[2] for r in I.INCEPTION_CONVS) == 17216
    # the oracle's own copy of the table says the same
    assert {r[0]: (r[1], r[2], (r[3], r[4]), r[5], (r[6], r[7])) for r in I.INCEPTION_CONVS} == IO.TABLE
    # every filter form of the network is one of the nine the GPU tests run
    assert {r[3:] for r in I.INCEPTION_CONVS} == set(FORMS)


def test_shape_chain_of_the_plan_and_of_the_oracle(oracle_runs):
    from munit_amd import inception as I
    steps, slots, outs = I.build_plan()
    chain = [(n, r.h, r.w, r.ctot) for n, r in outs.items()]
    # the extents and widths of the reference's comments (scripts/inception_utils.py:45-84)
    assert [c[1] for c in chain] == [149, 147, 147, 73, 73, 71, 35, 35, 35, 35, 17, 17, 17, 17, 17, 8, 8, 8]
    assert all(c[1] == c[2] for c in chain)
    assert [c[3] for c in chain[:7]] == [32, 32, 64, 64, 80, 192, 192]
    assert [c[3] for c in chain[7:]] == [256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048, 2048]
    # every block's `in` is the previous stage's width, and the four slots never alias within a step
    width = {n: c for n, _, _, c in chain}
    prev = dict(zip(IO.MIXED, ("maxpool2",) + IO.MIXED[:-1]))
    for name, cin, *_ in I.INCEPTION_CONVS:
        block, _, branch = name.partition(".")
        if block in prev and (branch.endswith("_1") or branch in ("branch1x1", "branch_pool", "branch3x3")):
            assert cin == width[prev[block]], name                 # the rows that read the block's input
    assert all(s.src.slot != s.dst.slot for s in steps)
    assert sum(s.kind == "conv" for s in steps) == 94 and sum(s.kind == "max" for s in steps) == 4 \
        and sum(s.kind == "avg" for s in steps) == 9
    # the oracle walks the same chain on the 299 x 299 input (NCHW shapes)
    _, shapes = oracle_runs["full"]
    assert [(s[2], s[3], s[1]) for _, s in shapes] == [(c[1], c[2], c[3]) for c in chain]


def test_oracle_reproduces_the_reference_fixture(oracle_runs):
    with open(os.path.join(ROOT, "tests", "golden", "golden_inception.json")) as f:
        fixture = json.load(f)
    for name, rec in fixture["cases"].items():
        feats, _ = oracle_runs[name]
        want = torch.tensor(rec["features"], dtype=torch.float64)
        top = float(want.abs().max())
        assert tuple(feats.shape) == (rec["shape"][0], 2048)
        assert float((feats[:, ::fixture["every"]] - want).abs().max()) <= FIXTURE_BOUND * top, name
        sums = torch.tensor(rec["row_sums"], dtype=torch.float64)
        assert float(((feats.sum(1) - sums).abs() / sums.abs()).max()) <= FIXTURE_BOUND, name
        assert float((feats != 0).double().mean()) >= 0.8


# ---- weights -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS, ids=lambda f: "k%dx%ds%dp%d-%d" % f)
def test_batch_norm_fold_equals_conv_bn_relu(form):
    from munit_amd import inception as I
    kh, kw, s, ph, pw = form
    g = torch.Generator().manual_seed(kh * 10 + kw)
    x = torch.randn(2, 6, 9, 11, generator=g, dtype=torch.float64)
    w = torch.randn(8, 6, kh, kw, generator=g, dtype=torch.float64)
    gamma, var = torch.rand(8, generator=g, dtype=torch.float64) + 0.5, torch.rand(8, generator=g, dtype=torch.float64) + 0.5
    beta, mean = torch.randn(8, generator=g, dtype=torch.float64), torch.randn(8, generator=g, dtype=torch.float64)
    want = F.relu(F.batch_norm(F.conv2d(x, w, None, stride=s, padding=(ph, pw)), mean, var, gamma, beta, training=False,
                               eps=0.001))
    wf, bf = I.fold_bn(w, gamma, beta, mean, var)
    assert wf.dtype == torch.float64 and bf.dtype == torch.float64
    got = F.relu(F.conv2d(x, wf, bf, stride=s, padding=(ph, pw)))
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # the kernel's image: row (kh * KW + kw) * Cin + ci holds the Cout weights of that tap and channel
    from munit_amd import ops
    img = ops.rect_weight_image(wf.float())
    assert tuple(img.shape) == (kh * kw * 6, 8) and img.is_contiguous()
    assert torch.equal(img[((kh - 1) * kw + (kw - 1)) * 6 + 4], wf.float()[:, 4, kh - 1, kw - 1])


def test_state_dict_ingestion(state):
    from munit_amd import inception as I
    extras = dict(state)
    extras.update({"AuxLogits.conv0.conv.weight": torch.zeros(128, 768, 1, 1), "fc.weight": torch.zeros(1000, 2048),
                   "fc.bias": torch.zeros(1000), "Conv2d_1a_3x3.bn.num_batches_tracked": torch.tensor(0)})
    net = I.InceptionV3(extras)
    plain = I.InceptionV3(state)
    assert sorted(net._host) == sorted(plain._host) == sorted(IO.TABLE)
    assert all(torch.equal(net._host[n][0], plain._host[n][0]) and torch.equal(net._host[n][1], plain._host[n][1])
               for n in IO.TABLE)
    w, b = plain._host["Mixed_6b.branch7x7_2"]
    assert tuple(w.shape) == (7 * 128, 128) and tuple(b.shape) == (128,) and w.dtype == b.dtype == torch.float32
    wf, bf = I.fold_bn(*(state["Mixed_6b.branch7x7_2" + k] for k in
                         (".conv.weight", ".bn.weight", ".bn.bias", ".bn.running_mean", ".bn.running_var")))
    assert torch.equal(b, bf.float()) and torch.equal(w.view(1, 7, 128, 128), wf.float().permute(2, 3, 1, 0))

    class Module(object):                                     # anything with .state_dict(), such as a torchvision module
        def state_dict(self):
            return state
    assert torch.equal(I.InceptionV3(Module())._host["Conv2d_1a_3x3"][0], plain._host["Conv2d_1a_3x3"][0])
    with pytest.raises(TypeError, match=r"state_dict"):
        I.InceptionV3(3)
    missing = dict(state)
    del missing["Mixed_7a.branch7x7x3_3.bn.running_var"]
    with pytest.raises(KeyError, match=r"Mixed_7a\.branch7x7x3_3\.bn\.running_var"):
        I.InceptionV3(missing)
    wrong = dict(state)
    wrong["Mixed_6c.branch7x7_2.conv.weight"] = torch.zeros(160, 160, 7, 1)          # 7x1 where 1x7 belongs
    with pytest.raises(ValueError, match=r"Mixed_6c\.branch7x7_2\.conv\.weight has shape \(160, 160, 7, 1\)"):
        I.InceptionV3(wrong)


def test_wrap_inception_takes_the_three_kinds_of_net(state):
    from munit_amd import inception as I, inception_utils as IU
    net = I.InceptionV3(state)
    assert IU.WrapInception(net).net is net
    assert isinstance(IU.WrapInception(state).net, I.InceptionV3)


def test_load_inception_net_fails_in_the_two_specified_ways(tmp_path, monkeypatch):
    from munit_amd import inception_utils as IU
    monkeypatch.delenv(IU.CKPT_ENV, raising=False)
    with pytest.raises(NotImplementedError) as e:
        IU.load_inception_net()
    assert "MUNIT_INCEPTION_CKPT" in str(e.value) and "net=" in str(e.value)
    monkeypatch.setenv(IU.CKPT_ENV, str(tmp_path / "nothing_here.pth"))
    with pytest.raises(FileNotFoundError, match=r"nothing_here\.pth"):
        IU.load_inception_net()
    with pytest.raises(NotImplementedError, match=r"parallel"):
        IU.load_inception_net(parallel=True)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_listed_and_exported(lib):
    from munit_amd import _lib
    header = open(os.path.join(ROOT, "include", "munit_hip.h")).read()
    declared = set(re.findall(r"\b(munit_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "inception.hip" in open(os.path.join(ROOT, "munit_amd", "csrc", "Makefile")).read()


def _err(lib):
    return lib.munit_last_error() or b""


def _desc(**k):
    from munit_amd._lib import RectDesc
    v = dict(B=2, H=9, W=11, Cin=16, x_ld=16, Cout=80, y_ld=80, KH=1, KW=7, stride=1, pad_h=0, pad_w=3, relu=1)
    v.update(k)
    return RectDesc(*[v[n] for n, _ in RectDesc._fields_])


def test_conv_rect_refusals_without_a_device(lib):
    f = lib.munit_conv2d_rect_fwd
    X, Wk, Bi, Y = (c_void_p(a) for a in (0x100000, 0x200000, 0x300000, 0x400000))
    ho, wo = c_int(), c_int()
    assert lib.munit_conv2d_rect_out_hw(byref(_desc()), byref(ho), byref(wo)) == 0 and (ho.value, wo.value) == (9, 11)
    assert lib.munit_conv2d_rect_out_hw(byref(_desc(KH=3, KW=3, stride=2, pad_w=0)), byref(ho), byref(wo)) == 0 \
        and (ho.value, wo.value) == (4, 5)
    assert f(None, X, Wk, Bi, Y, -1, None) == -1 and b"conv2d_rect_fwd: null descriptor" in _err(lib)
    for k in range(4):
        a = [X, Wk, Bi, Y]
        a[k] = None
        assert f(byref(_desc()), a[0], a[1], a[2], a[3], -1, None) == -1 and b"conv2d_rect_fwd: null pointer" in _err(lib)
    assert f(byref(_desc(x_ld=15)), X, Wk, Bi, Y, -1, None) == -1 and b"x_ld 15 shorter than its slice of 16" in _err(lib)
    assert f(byref(_desc(y_ld=79)), X, Wk, Bi, Y, -1, None) == -1 and b"y_ld 79 shorter than its slice of 80" in _err(lib)
    for s in (0, 3):
        assert f(byref(_desc(stride=s)), X, Wk, Bi, Y, -1, None) == -1 and b"stride must be 1 or 2" in _err(lib)
    assert f(byref(_desc(pad_w=4)), X, Wk, Bi, Y, -1, None) == -1 and b"pads (0, 4)" in _err(lib)
    assert f(byref(_desc(pad_h=1)), X, Wk, Bi, Y, -1, None) == -1 and b"pads (1, 3)" in _err(lib)        # KH = 1 takes no pad
    assert f(byref(_desc(W=5, pad_w=0)), X, Wk, Bi, Y, -1, None) == -1 and b"output extent below 1" in _err(lib)
    assert f(byref(_desc(Cin=0)), X, Wk, Bi, Y, -1, None) == -1 and b"must be >= 1" in _err(lib)
    assert f(byref(_desc()), X, Wk, Bi, Y, 3, None) == -1 and b"tile must be" in _err(lib)
    xbytes = (2 * 9 * 11 - 1) * 16 * 4 + 16 * 4
    assert f(byref(_desc()), X, Wk, Bi, X, -1, None) == -1 and b"y overlaps x" in _err(lib)
    assert f(byref(_desc()), X, Wk, Bi, c_void_p(0x100000 + xbytes - 4), -1, None) == -1 and b"y overlaps x" in _err(lib)
    assert f(byref(_desc()), X, Wk, Bi, Wk, -1, None) == -1 and b"y overlaps the weights" in _err(lib)
    assert lib.munit_conv2d_rect_tile(byref(_desc())) == 1 and lib.munit_conv2d_rect_tile(byref(_desc(B=4096))) == 0
    assert lib.munit_conv2d_rect_tile(byref(_desc(B=4096, Cout=64, y_ld=64))) == 2
    assert lib.munit_conv2d_rect_tile(byref(_desc(stride=3))) == -1


def test_window_and_input_refusals_without_a_device(lib):
    f = lib.munit_window3_fwd
    X, Y = c_void_p(0x100000), c_void_p(0x400000)
    args = lambda **k: [k.get(n, v) for n, v in (("B", 2), ("H", 9), ("W", 11), ("C", 16), ("x_ld", 16), ("y_ld", 16), ("mode", 0),
                                                 ("stride", 2), ("pad", 0))] + [None]
    assert f(None, Y, *args()) == -1 and b"window3_fwd: null pointer" in _err(lib)
    assert f(X, None, *args()) == -1 and b"window3_fwd: null pointer" in _err(lib)
    assert f(X, Y, *args(C=6, x_ld=8, y_ld=8)) == -1 and b"C % 4 == 0 is required, got 6" in _err(lib)
    assert f(X, Y, *args(mode=2)) == -1 and b"mode must be" in _err(lib)
    assert f(X, Y, *args(x_ld=12)) == -1 and b"x_ld 12 shorter" in _err(lib)
    assert f(X, Y, *args(y_ld=12)) == -1 and b"y_ld 12 shorter" in _err(lib)
    assert f(X, Y, *args(x_ld=18)) == -1 and b"multiples of 4" in _err(lib)
    assert f(c_void_p(0x100004), Y, *args()) == -1 and b"16-byte aligned" in _err(lib)
    for s in (0, 3):
        assert f(X, Y, *args(stride=s)) == -1 and b"stride must be 1 or 2" in _err(lib)
    assert f(X, Y, *args(pad=2)) == -1 and b"pad must be 0 or 1" in _err(lib)
    assert f(X, Y, *args(H=2)) == -1 and b"output extent below 1" in _err(lib)
    assert f(X, X, *args()) == -1 and b"y overlaps x" in _err(lib)

    g = lib.munit_inception_input
    assert g(None, 0, 2, 64, 48, Y, None) == -1 and b"inception_input: null pointer" in _err(lib)
    assert g(X, 0, 2, 64, 48, None, None) == -1 and b"inception_input: null pointer" in _err(lib)
    assert g(X, 2, 2, 64, 48, Y, None) == -1 and b"layout must be" in _err(lib)
    assert g(X, 0, 0, 64, 48, Y, None) == -1 and b"must be >= 1" in _err(lib)
    assert g(X, 1, 2, 64, 48, c_void_p(0x100000 + 2 * 3 * 64 * 48 * 4 - 4), None) == -1 and b"y overlaps x" in _err(lib)


def test_ops_refuse_host_tensors_and_bad_slices():
    from munit_amd import ops
    with pytest.raises(RuntimeError, match=r"HIP device"):
        ops.inception_input(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match=r"HIP device"):
        ops.window3(torch.zeros(1, 8, 8, 4), "max", 2, 0)
    with pytest.raises(RuntimeError, match=r"HIP device"):
        ops.conv2d_rect(torch.zeros(1, 8, 8, 4), torch.zeros(4, 4), torch.zeros(4), 1, 1)


# ---- the example loop's cadence ----------------------------------------------------------------------------------------
def _train_loop():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import train_loop as TL
    finally:
        sys.path.pop(0)
    return TL


def test_fid_wiring_of_the_example_loop(monkeypatch):
    """build_fid hands the config's keys to the loader and the metric as scripts/train.py:119-130 does, and an evaluation is
    one quiet call of the metric on a fresh loader."""
    from munit_amd import data, inception_utils as IU
    TL = _train_loop()
    calls = []
    monkeypatch.setattr(data, "get_fid_data_loader", lambda *a, **k: calls.append(("loader", a, k)) or "loader-%d" % len(calls))
    monkeypatch.setattr(IU, "prepare_inception_metrics", lambda **k: calls.append(("metric", k)) or
                        (lambda trainer, loader, prints=True, use_torch=True: calls.append(("run", trainer, loader, prints)) or 12.5))
    config = {"data_list_fid_a": "a.txt", "data_list_fid_b": "b.txt", "batch_size_fid": 1, "new_size": 256, "num_workers": 2,
              "inception_moment_path": "moments.npz", "eval_fid": 1}
    fid = TL.build_fid(config)
    assert calls == [("metric", {"inception_moment": "moments.npz", "parallel": False})]        # no loader until it is needed
    assert TL.evaluate_fid("trainer", fid) == 12.5 and TL.evaluate_fid("trainer", fid) == 12.5
    assert calls[1] == ("loader", ("a.txt", "b.txt", 1), {"train": False, "new_size": 256, "num_workers": 2})
    assert calls[2] == ("run", "trainer", "loader-2", False)
    assert [c[0] for c in calls] == ["metric", "loader", "run", "loader", "run"]                # a fresh loader per evaluation


def test_fid_every_cadence():
    TL = _train_loop()
    on = {"eval_fid": 1}
    assert [it for it in range(10) if TL.fid_due(on, it, 3)] == [2, 5, 8]
    assert not any(TL.fid_due(on, it, 0) for it in range(10))                       # the default: never
    assert not any(TL.fid_due({"eval_fid": 0}, it, 3) for it in range(10))
    assert not any(TL.fid_due({}, it, 3) for it in range(10))
    assert TL.fid_due(on, 0, 1)
