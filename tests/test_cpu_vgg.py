"""CPU: the host side of the domain-invariant perceptual loss (vgg_w) -- the weight file's layout and loading, the fp64 oracle
against the reference's own digests, the trainer's configuration checks, and which convolution kernels the frozen VGG16
dispatches to."""
import json
import os

import pytest
import torch

from oracle import munit_oracle as O
from tests import vgg_oracle as V

# networks.Vgg16().state_dict() of the reference: thirteen Conv2d(., ., 3, 1, 1), weight then bias
REF_KEYS = [n + s for n in ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2",
                            "conv4_3", "conv5_1", "conv5_2", "conv5_3") for s in (".weight", ".bias")]
REF_CHANNELS = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
                (512, 512), (512, 512), (512, 512)]


@pytest.fixture(scope="module")
def model():
    return V.make_model(0)


@pytest.fixture(scope="module")
def vgg_dir(tmp_path_factory, model):
    """<vgg_model_path> with models/vgg16.weight inside, as the reference's load_vgg16 would have left it"""
    root = tmp_path_factory.mktemp("vgg")
    os.makedirs(str(root / "models"))
    torch.save(model.state_dict(), str(root / "models" / "vgg16.weight"))
    return str(root)


def _golden():
    with open(os.path.join(os.path.dirname(__file__), "golden", "golden_vgg.json")) as f:
        return json.load(f)


def test_state_dict_is_the_references(model):
    sd = model.state_dict()
    assert list(sd) == REF_KEYS
    shapes = [s for cin, cout in REF_CHANNELS for s in ((cout, cin, 3, 3), (cout,))]
    assert [tuple(v.shape) for v in sd.values()] == shapes
    ref = _golden()                                   # ... and the list the reference's own module gave
    assert ref["keys"] == REF_KEYS and [tuple(s) for s in ref["shapes"]] == shapes
    assert sum(p.numel() for p in model.parameters()) == 14714688
    assert not model.training and not any(p.requires_grad for p in model.parameters())
    assert all(c.kernel_size == (3, 3) and c.stride == (1, 1) and c.padding == (1, 1) for c in model.children())


def test_load_vgg16_is_strict_and_names_a_missing_file(tmp_path, vgg_dir, model):
    from munit_amd.vgg import load_vgg16
    m = load_vgg16(os.path.join(vgg_dir, "models"))
    assert not m.training and not any(p.requires_grad for p in m.parameters())
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in m.state_dict().items())
    with pytest.raises(FileNotFoundError) as e:
        load_vgg16(str(tmp_path))
    assert os.path.join(str(tmp_path), "vgg16.weight") in str(e.value)
    sd = dict(model.state_dict())
    short = {k: v for k, v in sd.items() if k != "conv5_3.bias"}
    torch.save(short, str(tmp_path / "vgg16.weight"))
    with pytest.raises(RuntimeError, match="conv5_3.bias"):
        load_vgg16(str(tmp_path))
    extra = dict(sd, **{"conv5_4.weight": sd["conv5_3.weight"]})
    torch.save(extra, str(tmp_path / "vgg16.weight"))
    with pytest.raises(RuntimeError, match="conv5_4"):
        load_vgg16(str(tmp_path))


def test_device_weight_cache_is_dropped_on_writes(model):
    import copy
    m = copy.deepcopy(model)
    m._device_weights = ("sentinel", {})
    m.load_state_dict(model.state_dict())
    assert m._device_weights is None
    m._device_weights = ("sentinel", {})
    m.double()
    assert m._device_weights is None
    m.float()
    w = m.weights(torch.device("cpu"))
    assert m.weights(torch.device("cpu")) is w
    assert w["conv1_1"][0].is_contiguous(memory_format=torch.channels_last) and w["conv1_1"][0].shape == (64, 3, 3, 3)
    m.invalidate()
    assert m._device_weights is None


def _check_digest(got, ref, rel):
    t = got.detach().double().reshape(-1)
    assert t.numel() == ref["numel"]
    for key, val, bound in (("sum", float(t.sum()), ref["abs"]), ("abs", float(t.abs().sum()), ref["abs"]),
                            ("sq", float((t * t).sum()), ref["sq"])):
        assert abs(val - ref[key]) <= rel * bound, (key, val, ref[key])
    err = (t[torch.tensor(ref["idx"])] - torch.tensor(ref["val"], dtype=torch.float64)).abs().max().item()
    assert err <= rel * t.abs().max().item(), err


def test_oracle_matches_reference_fixture(model):
    """tests/vgg_oracle.py against digests of the reference's own Vgg16, vgg_preprocess and compute_vgg_loss
    (tests/golden/make_golden_vgg.py), float64.  Bound 1e-9 relative, the semantic fixture's: both sides are float64
    evaluations of the same thirteen convolutions and differ by summation order at most."""
    from tests.golden.make_golden_vgg import inputs
    ref = _golden()
    sd = V.state(model)
    wsq = float(sum((v.double() ** 2).sum() for v in model.state_dict().values()))
    assert abs(wsq - ref["weights_sq"]) <= 1e-12 * ref["weights_sq"], "make_model(0) no longer builds the fixture's weights"
    x_trans, x_orig = inputs()
    assert tuple(x_trans.shape) == (ref["batch"], 3, ref["h"], ref["w"])
    with torch.no_grad():
        _check_digest(V.preprocess(x_trans), ref["preprocessed"], 1e-12)
        f_orig = V.features(sd, x_orig)
        _check_digest(V.features(sd, x_trans), ref["relu5_3_trans"], 1e-9)
        _check_digest(f_orig, ref["relu5_3_orig"], 1e-9)
    assert tuple(f_orig.shape) == (ref["batch"], 512, ref["h"] // 8, ref["w"] // 8)      # no pool behind relu4_3
    xt = x_trans.clone().requires_grad_(True)
    loss = V.vgg_loss(sd, xt, x_orig)
    loss.backward()
    assert abs(loss.item() - ref["loss"]) <= 1e-9 * abs(ref["loss"])
    _check_digest(xt.grad, ref["dx"], 1e-9)
    # the pinned path with the oracle's own decisions is the unpinned one, and its audit is clean
    kinks = []
    with torch.no_grad():
        V.features(sd, x_orig, kinks=kinks)
    pins = [(v > 0) if kind == "relu" else V._windows(v).argmax(2) for kind, v in kinks]
    assert len(pins) == V.N_KINKS
    with torch.no_grad():
        assert torch.equal(V.features(sd, x_orig, pins=pins), f_orig)
    assert V.audit(kinks, pins) == (0.0, 0.0)
    flipped = [p.clone() for p in pins]
    at = kinks[0][1].abs().flatten().argmax()
    flipped[0].view(-1)[at] = ~flipped[0].view(-1)[at]
    worst, frac = V.audit(kinks, flipped)
    assert worst == 1.0 and frac > 0


def _hp(vgg_dir, size=64, **kw):
    hp = O.default_hp(size, 1, 1)
    hp["vgg_w"] = 1
    if vgg_dir is not None:
        hp["vgg_model_path"] = vgg_dir
    hp.update(kw)
    return hp


def test_constructor_builds_the_frozen_network_outside_the_state_dict(vgg_dir, model):
    from munit_amd.trainer import MUNIT_Trainer
    from munit_amd.vgg import Vgg16
    torch.manual_seed(0)
    tr = MUNIT_Trainer(_hp(vgg_dir))
    assert isinstance(tr.vgg, Vgg16) and not tr.vgg.training and not any(p.requires_grad for p in tr.vgg.parameters())
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in tr.vgg.state_dict().items())   # not re-initialised
    torch.manual_seed(0)
    plain = MUNIT_Trainer(O.default_hp(64, 1, 1))
    assert plain.vgg is None
    assert list(tr.state_dict()) == list(plain.state_dict())
    assert not list(tr.instancenorm.parameters()) and not list(tr.instancenorm.buffers())
    ids = {id(p) for p in tr.vgg.parameters()}
    assert not any(id(p) in ids for opt in (tr.gen_opt, tr.dis_opt) for grp in opt.param_groups for p in grp["params"])
    assert not any(id(p) in ids for p in tr.parameters())


def test_constructor_and_gen_update_refusals(tmp_path, vgg_dir):
    from munit_amd import ops
    from munit_amd.trainer import MUNIT_Trainer
    with pytest.raises(NotImplementedError, match=r"vgg_w \(without a vgg_model_path(.|\n)*cannot run in the reference"):
        MUNIT_Trainer(_hp(None))
    with pytest.raises(NotImplementedError, match="domain_adv_w"):
        MUNIT_Trainer(_hp(vgg_dir, domain_adv_w=1))
    with pytest.raises(FileNotFoundError) as e:
        MUNIT_Trainer(_hp(str(tmp_path)))
    assert os.path.join(str(tmp_path), "models", "vgg16.weight") in str(e.value)
    try:
        with pytest.raises(NotImplementedError, match="vgg_w > 0 runs in fp32 only"):
            MUNIT_Trainer(_hp(vgg_dir, precision="bf16"))
    finally:
        ops.set_compute("f32")
    for h, w in ((8, 8), (15, 64), (64, 12)):
        with pytest.raises(ValueError, match="at least 16x16"):
            MUNIT_Trainer(_hp(vgg_dir, crop_image_height=h, crop_image_width=w))
    # a trainer built without the network, handed vgg_w > 0 for a step: refused before any device work (host tensors would
    # be refused by the first op otherwise, with another error)
    plain = MUNIT_Trainer(O.default_hp(64, 1, 1))
    x = torch.zeros(1, 3, 64, 64)
    for hp in (_hp(vgg_dir), _hp(None)):
        with pytest.raises(ValueError, match="constructed with vgg_w > 0"):
            plain.gen_update(x, x, hp)
    # ... and a step on images too small for the network
    tr = MUNIT_Trainer(_hp(vgg_dir))
    small = torch.zeros(1, 3, 8, 8)
    with pytest.raises(ValueError, match="at least 16x16"):
        tr.gen_update(small, small, _hp(vgg_dir))


def test_vgg_kink_channel_and_sink_arguments():
    from munit_amd import ops
    assert ops.VGG_SINK is None
    mine = []
    with ops.kinks(vgg=mine, seg=True) as k:
        assert ops.VGG_SINK is mine and k.vgg is mine and k.seg == [] and k.dann is None
        with ops.kinks(vgg=None) as off:
            assert ops.VGG_SINK is None and off.vgg is None and off.seg is k.seg
        assert ops.VGG_SINK is mine
    assert ops.VGG_SINK is None and ops.SEG_SINK is None
    assert ops._POOLS["maxpool2"].sink == "dann"          # the table's entry is untouched by maxpool2(x, sink="vgg")
    with pytest.raises(ValueError, match="sink"):
        ops.maxpool2(torch.zeros(1, 4, 2, 2), sink="seg")


# ------------------------------------------------------------------------------------------------------------------
# which kernels the network's convolutions run on (tests/test_cpu_dispatch.py's treatment of the segmentation network)
# ------------------------------------------------------------------------------------------------------------------
VGG_CROPS = (64, 128, 256, 512)
VGG_IMAGES = (2, 4, 8, 16)           # images per network pass: 2B for B = 1 .. 8


def vgg_layers(h, w, n):
    """(name, op case (cin, cout, k, stride, pad, act, B, H, W)) of the thirteen layers on n images of h x w"""
    out = []
    for name, cin, cout in V.LAYERS:
        out.append((name, (cin, cout, 3, 1, 1, "relu", n, h, w)))
        if name in V.POOL_AFTER:
            h, w = h // 2, w // 2
    return out


def vgg_key(lib, case, which):
    """(pass, kernel name, cin, cout, filter, stride): the form classes of tests/test_cpu_dispatch.seg_key"""
    from tests.test_cpu_dispatch import kernel_names, seg_case
    c = seg_case(case, which)
    return (which, kernel_names(lib, c)[which]) + c[:4]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from munit_amd import _lib
    return _lib.load()


def test_every_vgg_conv_form_is_covered_by_a_vgg_op_case(lib):
    from tests.test_gpu_vgg import NETWORK_SHAPES, VGG_CONV_CASES
    shapes = [(c, c, n) for c in VGG_CROPS for n in VGG_IMAGES] + [(h, w, b) for b, h, w in NETWORK_SHAPES]
    prod = {}
    for h, w, n in shapes:
        for name, case in vgg_layers(h, w, n):
            for p in (0, 1):
                prod.setdefault(vgg_key(lib, case, p), "%s, %dx%d, %d images" % (name, h, w, n))
    assert len(prod) >= 18                             # nine channel classes, two passes
    assert not any(k[1].startswith("refused") or k[1] == "invalid" for k in prod), prod
    covered = {vgg_key(lib, c, p) for c in VGG_CONV_CASES for p in (0, 1)}
    missing = {k: v for k, v in prod.items() if k not in covered}
    assert not missing, "kernel forms the frozen VGG16 dispatches to that no VGG_CONV_CASES entry runs:\n" + "\n".join(
        "  %s: %s" % kv for kv in sorted(missing.items()))
    # the first layer has three channels on one side in both passes and runs on existing kernels, with no channel padding
    assert prod.keys() >= {(0, "conv_igemm_kernel<.., 5> (3 input channels as 4-channel taps)", 3, 64, 3, 1),
                           (1, "conv_igemm_kernel<.., 2, 3> (LDS-patch fold)", 3, 64, 3, 1)}


def test_vgg_cases_keep_their_kernels(lib):
    from tests.test_gpu_vgg import VGG_CONV_CASES, VGG_CONV_CASES_TARGETS
    assert list(VGG_CONV_CASES_TARGETS) == VGG_CONV_CASES and len(set(VGG_CONV_CASES)) == len(VGG_CONV_CASES)
    for c, want in VGG_CONV_CASES_TARGETS.items():
        got = tuple(vgg_key(lib, c, p)[1] for p in (0, 1))
        assert got == want, (c, got, want)
