"""GPU tests of spectral normalisation in the discriminators (dis.norm: sn): the power-iteration kernels, the
scale-bias-activation pair and the rank-1 correction against fp64 torch on the host, their guard-band contract, MsImageDis
against the reference's fixture (tests/golden/golden_sn.json) and tests/sn_oracle.py, and whole iterations of the trainer
against the oracle trainer.

Bounds (the project's own, tests/test_gpu_outda.py): a loss within 1e-5 relative of fp64, forward tensors within 1e-5
normalised maximum error, gradients within 5e-5, repeated runs bitwise equal; weights after an optimizer step within 4 lr and
2e-4 relative L2 per tensor."""
import ctypes
from ctypes import c_float

import pytest
import torch

from munit_amd import _lib, ops
from oracle import munit_oracle as O
from tests import outda_oracle as D
from tests import sn_oracle as S
from tests.conv_contract import GUARD_BYTE, Arena, Calls, Launches, fill_random, no_nan, poison, stream
from tests.parity import l2err, load_into_trainer, nerr, oracle_states, pinned, record, trainer_named_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL, GRAD_TOL, LOSS_TOL = 1e-5, 5e-5, 1e-5
NEW = ("munit_sn_",)
ACTS = ("none", "relu", "lrelu", "tanh")


@pytest.fixture(scope="module")
def fixture():
    return S.load_fixture()


# ---- power iteration ----------------------------------------------------------------------------------------------------
def _layer(o, i, seed):
    """a random (O, I, 4, 4) weight -- nothing symmetric in (i, kh, kw) -- with unit u, v, on the host in fp32"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(o, i, 4, 4, generator=g) / (16 * i) ** 0.5
    return w, S.l2n(torch.randn(o, generator=g)), S.l2n(torch.randn(i * 16, generator=g))


def _to_dev(layer):
    w, u, v = layer
    return w.to(DEV).contiguous(memory_format=torch.channels_last), u.to(DEV), v.to(DEV)


def _iterate_fp64(layers, calls):
    """[(u, v, sigma) per layer] after each of `calls` iterations, in fp64 from the fp32 start (v in the reference's column
    order: weight_bar.view(O, -1))"""
    state = [(w.double(), u.double().clone(), v.double().clone()) for w, u, v in layers]
    out = []
    for _ in range(calls):
        sigmas = [float(S.power_iteration(w, u, v)) for w, u, v in state]
        out.append([(u.clone(), v.clone(), s) for (_, u, v), s in zip(state, sigmas)])
    return out


SIZES = {"smallest": [(16, 8)], "no_tile_multiple": [(12, 6), (24, 12)], "production_multi_block": [(512, 256)],
         "one_table": [(16, 8), (12, 6), (512, 256), (24, 12)]}


@pytest.mark.parametrize("case", sorted(SIZES))
def test_power_iteration_against_fp64(case):
    host = [_layer(o, i, 31 + k) for k, (o, i) in enumerate(SIZES[case])]
    dev = [_to_dev(l) for l in host]
    table = ops.sn_table(dev)
    assert table[1:] == (len(host), max(o for o, _ in SIZES[case]), max(16 * i for _, i in SIZES[case]))
    want = _iterate_fp64(host, 3)
    sigmas = []
    for call in range(3):
        sigma = ops.sn_power_iter(*table)
        sigmas.append(sigma)
        torch.cuda.synchronize()
        for k, ((_, u, v), (ur, vr, sr)) in enumerate(zip(dev, want[call])):
            es = abs(float(sigma[2 * k]) - sr) / sr
            ei = abs(float(sigma[2 * k + 1]) - 1 / sr) * sr
            eu, ev = nerr(u, ur), nerr(v, vr)
            print("power iteration %s layer %d call %d: sigma %.6f rel %.1e, 1/sigma %.1e, u %.1e, v %.1e"
                  % (case, k, call + 1, sr, es, ei, eu, ev))
            assert max(es, ei, eu, ev) <= FWD_TOL
            # v in the weight's memory order (kh, kw, i) instead would be a permutation of the right answer
            wrong = vr.reshape(-1, 4, 4).permute(1, 2, 0).reshape(-1)
            assert nerr(wrong, vr) > 0.1
    # the same three calls from the same start: bitwise the same state and sigmas
    again = [_to_dev(l) for l in host]
    table2 = ops.sn_table(again)
    for call in range(3):
        assert torch.equal(ops.sn_power_iter(*table2), sigmas[call])
    torch.cuda.synchronize()
    for (_, u, v), (_, u2, v2) in zip(dev, again):
        assert torch.equal(u, u2) and torch.equal(v, v2)
    if case == "one_table":     # a layer's result does not depend on its neighbours in the table
        for k, l in enumerate(host):
            alone = [_to_dev(l)]
            s = ops.sn_power_iter(*ops.sn_table(alone))
            torch.cuda.synchronize()
            assert torch.equal(s, sigmas[0][2 * k:2 * k + 2])


def test_power_iteration_guard_bands():
    lib = _lib.load()
    layers = [_layer(12, 6, 41), _layer(24, 12, 42)]
    n, max_o, max_n = 2, 24, 192
    nws = lib.munit_sn_power_iter_workspace_bytes(n, max_o, max_n)
    spans = {"table": n * ctypes.sizeof(_lib.SnItem), "sigma": 8 * n, "ws": nws}
    for k, (w, u, v) in enumerate(layers):
        spans.update({"w%d" % k: 4 * w.numel(), "u%d" % k: 4 * u.numel(), "v%d" % k: 4 * v.numel()})
    a = Arena(spans, torch.device(DEV))
    items = []
    for k, (w, u, v) in enumerate(layers):
        a.view("w%d" % k, torch.float32).copy_(w.permute(0, 2, 3, 1).reshape(-1))      # [O][KH][KW][I]
        o, i = w.shape[:2]
        items.append(_lib.SnItem(a.ptr("w%d" % k).value, a.ptr("u%d" % k).value, a.ptr("v%d" % k).value, o, 4, 4, i, k))
    arr = (_lib.SnItem * n)(*items)
    a.bytes("table").copy_(torch.frombuffer(bytearray(ctypes.string_at(ctypes.addressof(arr), ctypes.sizeof(arr))),
                                            dtype=torch.uint8))
    L = Launches(a, ["table", "w0", "w1"], "sn_power_iter")
    outs = ["sigma", "u0", "v0", "u1", "v1"]
    res = []

    def reset(payload):
        for k, (w, u, v) in enumerate(layers):
            a.view("u%d" % k, torch.float32).copy_(u)
            poison(a.view("v%d" % k, torch.float32), payload)       # v is written before it is read
        poison(a.view("sigma", torch.float32), payload)
        a.bytes("ws").fill_(GUARD_BYTE)

    for payload in (0, 1):
        reset(payload)
        L.after(lib.munit_sn_power_iter(a.ptr("table"), n, max_o, max_n, a.ptr("sigma"), a.ptr("ws"), nws, stream()),
                "payload %d" % payload)
        assert all(no_nan(a.view(o, torch.float32)) for o in outs)
        res.append({o: a.bytes(o).clone() for o in outs})
    assert all(torch.equal(res[0][o], res[1][o]) for o in outs)
    want = _iterate_fp64(layers, 1)[0]
    for k, (ur, vr, sr) in enumerate(want):
        assert nerr(a.view("u%d" % k, torch.float32), ur) <= FWD_TOL and nerr(a.view("v%d" % k, torch.float32), vr) <= FWD_TOL
        assert abs(float(a.view("sigma", torch.float32)[2 * k]) - sr) <= FWD_TOL * sr
    # a workspace one byte short is refused before anything is written
    reset(0)
    before = {o: a.bytes(o).clone() for o in outs}
    rc = lib.munit_sn_power_iter(a.ptr("table"), n, max_o, max_n, a.ptr("sigma"), a.ptr("ws"), nws - 1, stream())
    torch.cuda.synchronize()
    assert rc == -2 and all(torch.equal(before[o], a.bytes(o)) for o in outs)
    L.verify("one byte short")


# ---- scale-bias-activation, its backward, the rank-1 correction ---------------------------------------------------------
def _act64(z, act):
    return {"none": z, "relu": z.clamp_min(0), "lrelu": torch.where(z > 0, z, 0.2 * z), "tanh": torch.tanh(z)}[act]


def _act_case(shape, seed):
    """raw, bias, dy on the host (fp32) and a sigma; dy leans on raw so that coef = sum dz raw / sigma^2 is a sum of mostly
    positive terms, not a cancellation: its fp32 error is then relative to its size, like the other outputs'"""
    b, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(b, c, h, w, generator=g)
    bias = 0.3 * torch.randn(c, generator=g)
    dy = 0.5 * raw + 0.5 * torch.randn(b, c, h, w, generator=g)
    return raw, bias, dy, 1.7 + 0.01 * seed


# (2, 16, 8, 8) and (3, 12, 5, 7): the shapes of the issue (h != w, an odd batch; both take the four-channel path);
# (2, 6, 5, 3) and (1, 70, 3, 3): channel counts that are no multiple of 4 (the one-channel path, within and beyond 64 lanes);
# (1, 272, 2, 3): more than 64 lanes x 4 channels; (3, 64, 128, 128): 3.1 M elements, beyond one sweep of every grid
ACT_SHAPES = [(2, 16, 8, 8), (3, 12, 5, 7), (2, 6, 5, 3), (1, 70, 3, 3), (1, 272, 2, 3), (3, 64, 128, 128)]


@pytest.mark.parametrize("shape", ACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scale_bias_activation_against_fp64(shape):
    raw_h, bias_h, dy_h, sig = _act_case(shape, sum(shape))
    nhwc = lambda t: t.to(DEV).contiguous(memory_format=torch.channels_last)
    raw, dy, bias = nhwc(raw_h), nhwc(dy_h), bias_h.to(DEV)
    sigma = torch.tensor([sig, 1.0 / sig], dtype=torch.float32, device=DEV)
    inv = sigma[1:2]
    inv64 = float(inv.cpu().double())
    for act in ACTS:
        y = ops.sn_act_fwd_raw(raw, inv, bias, act)
        z = raw_h.double() * inv64 + bias_h.double().reshape(1, -1, 1, 1)
        y64 = _act64(z, act)
        # backward from dy and the HIP run's own y (its ReLU branches), in fp64
        yd = y.cpu().double()
        dact = {"none": torch.ones_like(yd), "relu": (yd > 0).double(), "lrelu": torch.where(yd > 0, 1.0, 0.2),
                "tanh": 1 - yd * yd}[act]
        dz = dy_h.double() * dact
        want = dict(draw=dz * inv64, db=dz.sum(dim=(0, 2, 3)), coef=(dz * raw_h.double()).sum() * inv64 ** 2)
        draw, db, coef = ops.sn_act_bwd_raw(dy, y, raw, inv, act)
        e = dict(y=nerr(y, y64), draw=nerr(draw, want["draw"]), db=nerr(db, want["db"]),
                 coef=abs(float(coef) - float(want["coef"])) / abs(float(want["coef"])))
        print("sn_act %s %s: %s" % (shape, act, {k: "%.1e" % v for k, v in e.items()}))
        assert e["y"] <= FWD_TOL and max(e["draw"], e["db"], e["coef"]) <= GRAD_TOL, (act, e)
        assert draw.shape == raw.shape and ops._is_nhwc(draw) and ops._is_nhwc(y)
        # again: bitwise; accumulated into a live db: the same sums on top; without the reductions: the same draw
        draw2, db2, coef2 = ops.sn_act_bwd_raw(dy, y, raw, inv, act)
        assert torch.equal(draw, draw2) and torch.equal(db, db2) and torch.equal(coef, coef2)
        live = torch.full_like(db, 2.0)
        _, db3, _ = ops.sn_act_bwd_raw(dy, y, raw, inv, act, db=live, beta=1.0)
        assert db3 is live and torch.equal(live, db + 2.0)
        draw4, db4, coef4 = ops.sn_act_bwd_raw(dy, y, None, inv, act, reduce=False)
        assert db4 is None and coef4 is None and torch.equal(draw4, draw)
    # no bias: the same without it
    y0 = ops.sn_act_fwd_raw(raw, inv, None, "lrelu")
    assert nerr(y0, _act64(raw_h.double() * inv64, "lrelu")) <= FWD_TOL


@pytest.mark.parametrize("shape,act", [((3, 12, 5, 7), "lrelu"), ((2, 6, 5, 3), "tanh")])
def test_scale_bias_activation_guard_bands(shape, act):
    lib = _lib.load()
    b, c, h, w = shape
    npix, n = b * h * w, b * h * w * c
    nws = lib.munit_sn_act_bwd_workspace_bytes(npix, c)
    a = Arena({"raw": 4 * n, "dy": 4 * n, "bias": 4 * c, "inv": 4, "y": 4 * n, "draw": 4 * n, "db": 4 * c, "coef": 4, "ws": nws},
              torch.device(DEV))
    for k, name in enumerate(("raw", "dy", "bias")):
        fill_random(a.view(name, torch.float32), 90 + k)
    a.view("inv", torch.float32).fill_(0.6)
    L = Launches(a, ["raw", "dy", "bias", "inv"], "sn_act %s %s" % (shape, act))
    code, slope = _lib.ACT[act], c_float(0.2)
    fwd = lambda: lib.munit_sn_act_fwd(a.ptr("raw"), a.ptr("inv"), a.ptr("bias"), a.ptr("y"), npix, c, code, slope, stream())
    bwd = lambda ws_bytes=nws: lib.munit_sn_act_bwd(a.ptr("dy"), a.ptr("y"), a.ptr("raw"), a.ptr("inv"), a.ptr("draw"),
                                                    a.ptr("db"), c_float(0.0), a.ptr("coef"), npix, c, code, slope,
                                                    a.ptr("ws"), ws_bytes, stream())
    for what, outs, launch in (("fwd", ["y"], fwd), ("bwd", ["draw", "db", "coef"], bwd)):
        res = []
        for k in (0, 1):
            for o in outs:
                poison(a.view(o, torch.float32), k)
            a.bytes("ws").fill_(GUARD_BYTE)
            L.after(launch(), "%s payload %d" % (what, k))
            assert all(no_nan(a.view(o, torch.float32)) for o in outs), what
            res.append({o: a.bytes(o).clone() for o in outs})
        assert all(torch.equal(res[0][o], res[1][o]) for o in outs), what
        if what == "fwd":
            L.inputs["y"] = a.bytes("y").clone()          # an input of the backward from here on
    for o in ("draw", "db", "coef"):
        poison(a.view(o, torch.float32), 0)
    before = {o: a.bytes(o).clone() for o in ("draw", "db", "coef")}
    rc = bwd(nws - 1)
    torch.cuda.synchronize()
    assert rc == -2 and all(torch.equal(before[o], a.bytes(o)) for o in before)
    L.verify("bwd one byte short")


@pytest.mark.parametrize("o,i", [(12, 6), (16, 8), (130, 3)])
def test_rank_one_correction(o, i):
    """dw -= coef u (x) v, in the weight's memory order with v in the reference's column order; beta 0 writes -coef u (x) v.
    Every element is one product chain of three fp32 factors: 5e-5 is far above its rounding."""
    w, u, v = _layer(o, i, 50 + o)
    _, ud, vd = _to_dev((w, u, v))
    coef = torch.tensor([0.37], device=DEV)
    want = -0.37 * torch.outer(u.double(), v.double()).reshape(o, i, 4, 4)
    fresh = ops.sn_grad_fix_raw(coef, ud, vd, (o, i, 4, 4))
    assert fresh.shape == (o, i, 4, 4) and ops._is_nhwc(fresh) and nerr(fresh, want) <= GRAD_TOL
    g = torch.Generator().manual_seed(o)
    live_h = torch.randn(o, i, 4, 4, generator=g)
    live = live_h.to(DEV).contiguous(memory_format=torch.channels_last)
    out = ops.sn_grad_fix_raw(coef, ud, vd, (o, i, 4, 4), dw=live, beta=1.0)
    assert out is live and nerr(live, live_h.double() + want) <= GRAD_TOL
    again = ops.sn_grad_fix_raw(coef, ud, vd, (o, i, 4, 4))
    assert torch.equal(fresh, again)


# ---- MsImageDis on the fixture --------------------------------------------------------------------------------------------
def _fixture_module(fx, which="a"):
    from munit_amd.networks import MsImageDis
    arr = fx["arr"]
    initial = fx["initial"] if which == "a" else fx["b"]["initial"]
    net = MsImageDis(3, dict(fx["hp_a"] if which == "a" else fx["hp_b"]))
    net.load_state_dict({k: arr[a] for k, a in initial.items()})           # the reference's keys, key for key
    return net.to(DEV), S.from_full({k: arr[a] for k, a in initial.items()})


def _run_call(net, rec, xs_host, bound):
    """one recorded call on the HIP module; -> (loss, {name: parameter gradient}, [input gradients], kinks)"""
    names = [n for n, p in net.named_parameters() if p.requires_grad]
    params = [p for _, p in net.named_parameters() if p.requires_grad]

    def hip():
        xs = [ops.nhwc(x.float().to(DEV)).requires_grad_(True) for x in xs_host]
        loss = getattr(net, rec["fn"])(*xs)
        if bound is None:
            grads = torch.autograd.grad(loss, params + xs)
            return loss, dict(zip(names, grads)), list(grads[len(params):])
        bound.zero_grad()
        loss.backward()             # bare: the gradients land in the flat buffer, some through the side stream
        ops.join_side_streams()
        return loss, {n: p._munit_grad.clone() for n, p in zip(names, params)}, [x.grad for x in xs]

    (loss, pg, xg), km, _ = record(hip)
    return loss, pg, xg, km


@pytest.mark.parametrize("mode", ["autograd", "flat_side_stream", "flat_one_stream"])
def test_module_against_the_fixture(fixture, mode, monkeypatch):
    """The reference's four calls in the fixture's order on one module: losses, every gradient the fixture holds, u / v after
    each call -- against the reference's own numbers; the parameter gradients of the two generator-side calls, which the
    fixture leaves out, against tests/sn_oracle.py on the HIP run's kinks.  autograd: a stand-alone module; flat_*: its
    parameters bound to an optimizer's flat buffers, backward-weight and the rank-1 corrections on the side stream or not."""
    from munit_amd.trainer import FusedAdam
    fx, arr = fixture, fixture["arr"]
    ops.set_compute("f32")
    monkeypatch.setattr(ops, "SIDE_STREAM_WGRAD", mode != "flat_one_stream")
    net, sd = _fixture_module(fx)
    bound = None
    if mode != "autograd":
        bound = FusedAdam([p for p in net.parameters() if p.requires_grad], lr=1e-4, betas=(0.5, 0.999), weight_decay=1e-4)
        bound.bind(torch.device(DEV))
    for rec in fx["calls"]:
        xs = [arr[fx["inputs"][k]].double() for k in rec["inputs"]]
        with Calls(NEW) as calls:
            loss, pg, xg, km = _run_call(net, rec, xs, bound)
        passes = len(xs)
        assert calls.count("munit_sn_power_iter") == passes                # one call per forward covers every layer
        assert calls.count("munit_sn_act_fwd") == calls.count("munit_sn_act_bwd") == calls.count("munit_sn_grad_fix") == 4 * passes
        rs = [x.clone().requires_grad_(True) for x in xs]
        with pinned(km, rec["fn"]):
            l_ref = S.calc(rec["fn"], sd, fx["hp_a"], *rs)
        g_ref = torch.autograd.grad(l_ref, list(sd.values()) + rs)
        rel = abs(float(loss.detach()) - rec["loss"]) / abs(rec["loss"])
        errs = {"dx%d" % i: nerr(g, arr[k]) for i, (g, k) in enumerate(zip(xg, rec["input_grads"]))}
        errs.update({n: nerr(pg[n], arr[k]) for n, k in rec["param_grads"].items()})
        errs.update({"oracle " + n: nerr(pg[n], g) for n, g in zip(sd, g_ref)})
        state = net.state_dict()
        uv = {k: nerr(state[k], arr[a]) for k, a in rec["uv_after"].items()}
        print("%s %s: loss rel %.1e, worst gradient %.1e, worst u / v %.1e" % (mode, rec["fn"], rel, max(errs.values()),
                                                                              max(uv.values())))
        assert rel <= LOSS_TOL, (rec["fn"], float(loss.detach()), rec["loss"])
        assert max(errs.values()) <= GRAD_TOL, {k: v for k, v in errs.items() if v > GRAD_TOL}
        assert max(uv.values()) <= FWD_TOL, {k: v for k, v in uv.items() if v > FWD_TOL}
        assert all(not p.requires_grad and p.grad is None for n, p in net.named_parameters() if n.endswith(("_u", "_v")))


def test_module_with_no_multiple_of_64(fixture):
    fx, arr = fixture, fixture["arr"]
    ops.set_compute("f32")
    net, _ = _fixture_module(fx, "b")
    rec = fx["b"]["call"]
    loss, pg, xg, _ = _run_call(net, rec, [arr[fx["b"]["x"]].double()], None)
    errs = {n: nerr(pg[n], arr[k]) for n, k in rec["param_grads"].items()}
    errs["dx"] = nerr(xg[0], arr[rec["input_grads"][0]])
    state = net.state_dict()
    uv = max(nerr(state[k], arr[a]) for k, a in rec["uv_after"].items())
    rel = abs(float(loss.detach()) - rec["loss"]) / abs(rec["loss"])
    print("network B: loss rel %.1e, worst gradient %.1e, worst u / v %.1e" % (rel, max(errs.values()), uv))
    assert rel <= LOSS_TOL and max(errs.values()) <= GRAD_TOL and uv <= FWD_TOL, errs


def test_forward_under_no_grad_and_in_eval_still_iterates(fixture):
    fx, arr = fixture, fixture["arr"]
    ops.set_compute("f32")
    net, sd = _fixture_module(fx)
    x = arr[fx["inputs"]["fake"]]
    net.eval()
    with torch.no_grad(), Calls(NEW) as calls:
        outs = net(x.to(DEV))
    assert calls.count("munit_sn_power_iter") == 1 and calls.count("munit_sn_act_fwd") == 4
    with S.spectral():
        ref = O.dis_forward(sd, "", x.double(), fx["hp_a"])
    assert max(nerr(o, r) for o, r in zip(outs, ref)) <= FWD_TOL
    state = net.state_dict()
    first = {k: state[k].clone() for k in sd.uv}
    assert max(nerr(first[k], sd.uv[k]) for k in sd.uv) <= FWD_TOL
    assert all(not torch.equal(first[k].cpu(), arr[fx["initial"][k]]) for k in sd.uv)      # the state moved
    with torch.no_grad():
        net(x.to(DEV))
    with S.spectral():
        O.dis_forward(sd, "", x.double(), fx["hp_a"])
    state = net.state_dict()
    assert max(nerr(state[k], sd.uv[k]) for k in sd.uv) <= FWD_TOL
    assert all(not torch.equal(state[k], first[k]) for k in sd.uv)


def test_a_block_on_its_own_iterates_itself():
    """Conv2dBlock(norm='sn') outside MsImageDis: every forward runs its own one-layer power iteration"""
    from munit_amd.networks import Conv2dBlock
    torch.manual_seed(3)
    blk = Conv2dBlock(6, 12, 4, 2, 1, norm="sn", activation="lrelu", pad_type="reflect").to(DEV)
    m = blk.conv.module
    w, b = m.weight_bar.detach().cpu().double(), m.bias.detach().cpu().double()
    u, v = m.weight_u.detach().cpu().double().clone(), m.weight_v.detach().cpu().double().clone()
    x = torch.randn(2, 6, 8, 8)
    for _ in range(2):
        y = blk(x.to(DEV))
        sigma = S.power_iteration(w, u, v)
        ref = O.conv_block(x.double(), w / sigma, b, 2, 1, "reflect", None, "lrelu")
        assert nerr(y, ref) <= FWD_TOL and nerr(m.weight_u, u) <= FWD_TOL and nerr(m.weight_v, v) <= FWD_TOL


# ---- the trainer ------------------------------------------------------------------------------------------------------------
def _hp(**over):
    hp = O.default_hp(64, 2, 1)
    hp["gen"]["n_res"] = 1
    hp["dis"] = dict(hp["dis"], norm="sn")
    for k, v in over.items():
        hp[k] = dict(hp[k], **v) if isinstance(v, dict) else v
    return hp


def _batch(seed=7):
    return [t.to(DEV) for t in O.synthetic_batch(2, 64, seed=seed)]


def _styles(hp, seed):
    torch.manual_seed(seed)
    return (torch.randn(2, hp["gen"]["style_dim"], 1, 1).double(), torch.randn(2, hp["gen"]["style_dim"], 1, 1).double())


def _sequence(hp, iters):
    """dis_update + gen_update (and the classifier update when the output classifiers exist) against the fp64 oracle trainer
    whose discriminators are tests/sn_oracle.py's: every loss, the discriminator gradients and every weight after each call.
    Before a call the oracle takes over the HIP trainer's weights and u / v (tests/parity.py: Adam's first steps are
    sign-like, so two runs otherwise drift); its optimizer moments and step counts carry over."""
    from munit_amd.trainer import MUNIT_Trainer
    outda = hp["adaptation"]["output_adv_lambda"] > 0
    gen = oracle_states(hp, torch.float64)[0]
    dis_a, dis_b = (S.make_state(hp["dis"], 3, tag) for tag in ("dis_a.", "dis_b."))
    cls = [S.make_state(hp["dis"], 3, tag) for tag in ("ocls_a.", "ocls_b.")] if outda else []
    orc = S.oracle_trainer_class(D.oracle_trainer_class() if outda else None)(hp, gen, dis_a, dis_b)
    tr = MUNIT_Trainer(dict(hp))
    load_into_trainer(tr, gen, {}, {})
    nets = [(tr.dis_a, dis_a), (tr.dis_b, dis_b)]
    if outda:
        orc.attach(*cls)
        nets += [(tr.output_classifier_sr_a, cls[0]), (tr.output_classifier_sr_b, cls[1])]
    for net, sd in nets:
        S.load_into(net, sd)
    tr.to(DEV)
    x_a, x_b, m_a, m_b = _batch()
    x_as, x_bs = _batch(seed=8)[:2]
    ox = {k: v.double().cpu() for k, v in dict(x_a=x_a, x_b=x_b, m_a=m_a, m_b=m_b, x_as=x_as, x_bs=x_bs).items()}
    gnames, _ = trainer_named_params(tr)
    trainable = lambda net: [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    dnames = [("a." + n, p) for n, p in trainable(tr.dis_a)] + [("b." + n, p) for n, p in trainable(tr.dis_b)]
    groups = [("gen", gnames, orc.opt["gen"]["params"]), ("dis", dnames, orc.opt["dis"]["params"])]
    if outda:
        cnames = [("a." + n, p) for n, p in trainable(tr.output_classifier_sr_a)] + \
                 [("b." + n, p) for n, p in trainable(tr.output_classifier_sr_b)]
        groups.append(("cls", cnames, orc.cls_opt.params))
    assert all(len(names) == len(params) for _, names, params in groups)
    null, lr, worst = set(), hp["lr"], dict(loss=0.0, dis_grad=0.0, weight_abs=0.0, weight_l2=0.0, uv=0.0, kink=0.0)

    def sync():
        with torch.no_grad():
            for _, names, params in groups:
                for (n, p), q in zip(names, params):
                    q.copy_(p.detach().double().cpu())
            for net, sd in nets:
                state = net.state_dict()
                for k, t in sd.uv.items():
                    t.copy_(state[k].double().cpu())

    def compare(what, losses):
        for k in losses:
            mine, v = getattr(tr, k), float(orc.losses[k])
            mine = float(mine.detach()) if torch.is_tensor(mine) else float(mine)
            rel = abs(mine - v) / max(1.0, abs(v))
            worst["loss"] = max(worst["loss"], rel)
            assert rel <= LOSS_TOL, (what, k, mine, v, rel)
        for grp, names, params in groups:
            for (n, p), q in zip(names, params):
                if grp + "." + n in null:
                    continue
                a, r = p.detach().double().cpu(), q.detach()
                worst["weight_abs"] = max(worst["weight_abs"], float((a - r).abs().max()))
                worst["weight_l2"] = max(worst["weight_l2"], l2err(a, r))
                assert float((a - r).abs().max()) <= 4.0 * lr and l2err(a, r) <= 2e-4, (what, grp, n, worst)
        for net, sd in nets:
            state = net.state_dict()
            worst["uv"] = max([worst["uv"]] + [nerr(state[k], t) for k, t in sd.uv.items()])
        assert worst["uv"] <= FWD_TOL, (what, worst)

    def run(what, seed, hip, oracle):
        km = record(hip, seed)[1]
        with pinned(km, what) as audit:
            out = oracle()
        worst["kink"] = max(worst["kink"], audit.worst_rel)
        return out

    for it in range(iters):
        tr.iterations = orc.iterations = it
        tr.update_learning_rate()
        orc.update_learning_rate()
        sync()
        sa, sb = _styles(hp, 100 + it)
        d_ref = run("dis", 100 + it, lambda: tr.dis_update(x_a, x_b, hp), lambda: orc.dis_update(ox["x_a"], ox["x_b"], sa, sb))
        for (n, p), g in zip(dnames, d_ref):
            worst["dis_grad"] = max(worst["dis_grad"], nerr(p._munit_grad, g))
        assert worst["dis_grad"] <= GRAD_TOL, worst
        compare("dis_update %d" % it, ("loss_dis_a", "loss_dis_b", "loss_dis_total"))
        sync()
        sa, sb = _styles(hp, 200 + it)
        g_ref = run("gen", 200 + it, lambda: tr.gen_update(x_a, x_b, hp, m_a, m_b),
                    lambda: orc.gen_update(ox["x_a"], ox["x_b"], ox["m_a"], ox["m_b"], sa, sb))
        for (n, _), g in zip(gnames, g_ref):
            if g is None or float(g.abs().max()) < 1e-7:
                null.add("gen." + n)
        compare("gen_update %d" % it, [k for k in orc.losses if k.startswith("loss_gen") or k == "loss_output_classifier_sr"])
        if outda:
            assert float(tr.loss_output_classifier_sr) > 0
            sync()
            run("cls", 300 + it, lambda: tr.output_domain_classifier_sr_update(x_a, x_as, x_b, x_bs, hp, it),
                lambda: orc.output_domain_classifier_sr_update(ox["x_a"], ox["x_as"], ox["x_b"], ox["x_bs"]))
            compare("classifier update %d" % it, ("loss_output_classifier_sr_update",))
        assert all(not p.requires_grad for net, _ in nets for n, p in net.named_parameters() if n.endswith(("_u", "_v")))
        assert all(p.requires_grad for net, _ in nets for n, p in net.named_parameters() if not n.endswith(("_u", "_v")))
    assert tr.gen_opt._step == orc.opt["gen"]["step"] == iters and tr.dis_opt._step == orc.opt["dis"]["step"] == iters
    print("sn sequence %s: %s" % ({k: hp[k] for k in ("gen_state", "optimizer")}, {k: "%.2e" % v for k, v in worst.items()}))


def test_iteration_against_the_oracle_shared_generator():
    _sequence(_hp(), 1)


def test_iteration_against_the_oracle_separate_generators():
    _sequence(_hp(gen_state=0), 1)


def test_iterations_against_the_oracle_extraadam():
    # an extrapolation, then a step; two iterations, so on narrower networks (the production widths run in the tests above)
    _sequence(_hp(optimizer="extraadam", gen=dict(dim=32, mlp_dim=64), dis=dict(dim=32)), 2)


def test_iteration_against_the_oracle_with_the_output_classifiers():
    _sequence(_hp(adaptation=dict(output_classifier_lambda=2, output_adv_lambda=1.5)), 1)


def test_checkpoint_roundtrip_reproduces_the_next_step_bitwise(tmp_path):
    from munit_amd.trainer import MUNIT_Trainer
    hp = _hp(dis=dict(dim=16))
    x_a, x_b, m_a, m_b = _batch()

    def fresh(seed):
        torch.manual_seed(seed)
        return MUNIT_Trainer(dict(hp)).to(DEV)

    def step(t):
        torch.manual_seed(5)
        t.update_learning_rate(); t.dis_update(x_a, x_b, hp); t.gen_update(x_a, x_b, hp, m_a, m_b)

    a = fresh(11)
    step(a)
    a.save(str(tmp_path), 0)
    saved = torch.load(str(tmp_path / "dis_00000001.pt"), map_location="cpu", weights_only=True)
    assert "cnns.0.1.conv.module.weight_u" in saved["a"] and "cnns.2.3.conv.module.weight_bar" in saved["b"]
    b = fresh(12)                                      # other weights, other u / v
    assert b.resume(str(tmp_path), hp) == 1
    for t in (a, b):
        step(t)
    torch.cuda.synchronize()
    assert float(a.loss_gen_total) == float(b.loss_gen_total) and float(a.loss_dis_total) == float(b.loss_dis_total)
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), n


def test_norm_none_issues_no_spectral_call():
    from munit_amd.trainer import MUNIT_Trainer
    hp = _hp(dis=dict(norm="none"))
    torch.manual_seed(0)
    tr = MUNIT_Trainer(dict(hp)).to(DEV)
    x_a, x_b, m_a, m_b = _batch()
    with Calls(NEW) as calls:
        tr.dis_update(x_a, x_b, hp)
        tr.gen_update(x_a, x_b, hp, m_a, m_b)
        torch.cuda.synchronize()
    assert calls == []
    # ... and under sn the same step does: one power iteration per discriminator forward (two in dis_update's two-pass pair,
    # one in gen_update, per discriminator)
    hp = _hp()
    tr = MUNIT_Trainer(dict(hp)).to(DEV)
    with Calls(NEW) as calls:
        tr.dis_update(x_a, x_b, hp)
        tr.gen_update(x_a, x_b, hp, m_a, m_b)
        torch.cuda.synchronize()
    assert calls.count("munit_sn_power_iter") == 6 and calls.count("munit_sn_act_fwd") == 6 * 9
    assert calls.count("munit_sn_grad_fix") == 4 * 9          # dis_update alone forms weight gradients
