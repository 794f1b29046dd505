"""GPU tests of feature-level domain adaptation (adaptation.adv_lambda / dfeat_lambda): the kernels of dann.hip against fp64
torch on the host, their guard-band contract, the six convolution forms the classifier reaches, the whole classifier and the
two updates of the trainer against tests/featda_oracle.py.

Bounds (the project's own, tests/test_gpu_synth.py and tests/parity.py): a loss within 1e-5 relative of the fp64 oracle,
gradients within 5e-5 normalised maximum error, a second backward bitwise equal to the first.  Forward tensors: 1e-5
normalised maximum error -- a few dozen fp32 roundings of 6e-8 each on O(1) values."""
from ctypes import c_float, c_void_p

import pytest
import torch
import torch.nn.functional as F

from munit_amd import _lib, ops
from oracle import munit_oracle as O
from tests import featda_oracle as D
from tests.conv_contract import (ERR_WORKSPACE, GUARD_BYTE, POISON, Arena, Calls, Launches, fill_random, no_nan, poison,
                                 stream)
from tests.parity import nerr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL, GRAD_TOL, LOSS_TOL = 1e-5, 5e-5, 1e-5
NEW = ("munit_batchnorm", "munit_maxpool2", "munit_avgpool16")


def _nhwc(t):
    return t.to(DEV, torch.float32).contiguous(memory_format=torch.channels_last)


def _rows(r, c, seed, mean=0.0):
    """(R, C) rows as a logical (1, C, R, 1) NHWC tensor; fp32 values"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(r, c, generator=g) * (0.5 + torch.rand(c, generator=g)) + mean + torch.randn(c, generator=g)
    return x.float()


def _bn_ref(x, gamma, beta, relu, dy):
    """fp64 training-mode batch norm of (R, C) rows: y, mean, rstd, unbiased variance, dx, dgamma, dbeta"""
    x = x.double().requires_grad_(True)
    gamma, beta = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    m = x.mean(0)
    v = ((x - m) ** 2).mean(0)
    rstd = 1 / torch.sqrt(v + 1e-5)
    y = (x - m) * rstd * gamma + beta
    if relu:
        y = F.relu(y)
    dx, dg, db = torch.autograd.grad(y, [x, gamma, beta], dy.double())
    return y.detach(), m.detach(), rstd.detach(), v.detach() * x.shape[0] / (x.shape[0] - 1), dx, dg, db


def _as4(rows):
    r, c = rows.shape
    return rows.reshape(1, r, 1, c).permute(0, 3, 1, 2).to(DEV)          # logical (1, C, R, 1), NHWC memory


def _bn_raw(x, dy, gamma, beta, rm, rv, relu, with_w=True, eval_=0):
    """munit_batchnorm_fwd + _bwd through ctypes on (R, C) device rows; returns y, mean, rstd, dx, dgamma, dbeta"""
    lib = _lib.load()
    r, c = x.shape
    y, dx = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(2 * c, device=DEV), torch.empty(c, device=DEV)      # the mean as high + low parts
    dg, db = torch.full((c,), 7.0, device=DEV), torch.full((c,), 7.0, device=DEV)
    nws = lib.munit_batchnorm_workspace_bytes(c)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    p = lambda t: c_void_p(t.data_ptr())
    _lib.check(lib.munit_batchnorm_fwd(p(x), p(y), p(mean), p(rstd), p(rm), p(rv), r, c, p(gamma), p(beta), relu, eval_,
                                       c_float(1e-5), c_float(0.1), p(ws), nws, stream()), "bn fwd")
    if eval_:
        return y
    _lib.check(lib.munit_batchnorm_bwd(p(x), p(dy), p(y), p(gamma), p(mean), p(rstd), p(dx), p(dg) if with_w else None,
                                       p(db) if with_w else None, c_float(0.0), r, c, relu, p(ws), nws, stream()), "bn bwd")
    torch.cuda.synchronize()
    return y, mean, rstd, dx, dg, db


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("rc", [(7, 64), (2048, 64), (1024, 128), (2 * 31 * 31, 128)])
def test_batchnorm_against_fp64(rc, relu):
    r, c = rc
    mean = 100.0 if rc == (2048, 64) else 0.0          # one case with a channel mean of 100 against unit spread
    x, dy = _rows(r, c, 1, mean), _rows(r, c, 2)
    g = torch.Generator().manual_seed(3)
    gamma, beta = 1 + 0.3 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)
    ry, rm_, rrstd, runb, rdx, rdg, rdb = _bn_ref(x, gamma, beta, relu, dy)
    xd, dyd, gd, bd = x.to(DEV), dy.to(DEV), gamma.to(DEV), beta.to(DEV)
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    y, m, rstd, dx, dg, db = _bn_raw(xd, dyd, gd, bd, rm, rv, relu)
    errs = dict(y=nerr(y, ry), mean=nerr(m[:c].double() + m[c:].double(), rm_), rstd=nerr(rstd, rrstd), dx=nerr(dx, rdx), dgamma=nerr(dg, rdg),
                dbeta=nerr(db, rdb))
    print("batchnorm", rc, relu, errs)
    if relu:                                            # a y within rounding of 0 may sit on the other side of the kink
        near = (ry.abs() < 1e-5 * float(ry.abs().max())) & ((y.cpu() > 0) != (ry > 0))
        assert int(near.sum()) == int(((y.cpu() > 0) != (ry > 0)).sum())
    for k in ("y", "mean", "rstd"):
        assert errs[k] <= FWD_TOL, errs
    for k in ("dx", "dgamma", "dbeta"):
        assert errs[k] <= GRAD_TOL, errs
    # the running statistics after two calls: momentum 0.1, unbiased variance
    y2, _, _, dx2, dg2, db2 = _bn_raw(xd, dyd, gd, bd, rm, rv, relu)
    want_m = 0.19 * rm_
    want_v = 0.81 + 0.19 * runb
    assert nerr(rm, want_m) <= FWD_TOL and nerr(rv, want_v) <= FWD_TOL, (nerr(rm, want_m), nerr(rv, want_v))
    # a second forward / backward is bitwise the first
    for a, b in ((y, y2), (dx, dx2), (dg, dg2), (db, db2)):
        assert torch.equal(a, b)
    # null dgamma / dbeta leave the buffers untouched, dx is the same
    _, _, _, dx3, dg3, db3 = _bn_raw(xd, dyd, gd, bd, rm.clone(), rv.clone(), relu, with_w=False)
    assert torch.equal(dx3, dx) and bool((dg3 == 7.0).all()) and bool((db3 == 7.0).all())
    # evaluation mode: the running statistics' formula, nothing updated
    rm0, rv0 = rm.clone(), rv.clone()
    ye = _bn_raw(xd, dyd, gd, bd, rm, rv, relu, eval_=1)
    want = (x.double() - rm0.cpu().double()) / torch.sqrt(rv0.cpu().double() + 1e-5) * gamma.double() + beta.double()
    want = F.relu(want) if relu else want
    assert nerr(ye, want) <= FWD_TOL and torch.equal(rm, rm0) and torch.equal(rv, rv0)


def test_batchnorm_function_accumulates_into_bound_buffers():
    """ops.batch_norm: gradients of the parameters the ordinary way, and straight into `_munit_grad` buffers when bound."""
    x = _as4(_rows(512, 64, 5)).requires_grad_(True)
    gamma = torch.nn.Parameter(torch.rand(64, device=DEV) + 0.5)
    beta = torch.nn.Parameter(torch.rand(64, device=DEV))
    rm, rv = torch.zeros(64, device=DEV), torch.ones(64, device=DEV)
    y = ops.batch_norm(x, gamma, beta, rm, rv, relu=True)
    dy = torch.randn_like(y)
    dx, dg, db = torch.autograd.grad(y, [x, gamma, beta], dy, retain_graph=True)
    gamma._munit_grad, beta._munit_grad = torch.ones(64, device=DEV), torch.ones(64, device=DEV)
    y2 = ops.batch_norm(x, gamma, beta, rm, rv, relu=True)
    (dx2,) = torch.autograd.grad(y2, [x], dy, allow_unused=True)
    assert torch.equal(dx, dx2) and torch.equal(y, y2)
    assert torch.allclose(gamma._munit_grad, 1 + dg, rtol=1e-6, atol=1e-6) and torch.allclose(beta._munit_grad, 1 + db, rtol=1e-6, atol=1e-6)
    gamma._munit_grad.fill_(1.0)
    y3 = ops.batch_norm(x, gamma, beta, rm, rv, relu=True, need_weight_grads=False)
    (dx3,) = torch.autograd.grad(y3, [x], dy)
    assert torch.equal(dx3, dx) and bool((gamma._munit_grad == 1.0).all())


@pytest.mark.parametrize("hw", [(2, 2), (5, 7), (64, 64), (65, 80)])
@pytest.mark.parametrize("lattice", [False, True])
def test_maxpool2_against_torch(hw, lattice):
    h, w = hw
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randint(-2, 3, (2, 64, h, w), generator=g).float() if lattice else torch.randn(2, 64, h, w, generator=g)
    xr = x.double().requires_grad_(True)
    yr = F.max_pool2d(xr, 2)
    dy = torch.randn(yr.shape, generator=g)
    (dxr,) = torch.autograd.grad(yr, [xr], dy.double())
    xd = _nhwc(x).requires_grad_(True)
    with ops.kinks(dann=True) as k:
        y = ops.maxpool2(xd)
    sink = k.dann
    assert torch.equal(y.cpu().double(), yr.detach())
    # dx into a buffer full of NaN: every element written once, zeros on the losers and in the dropped row / column
    lib = _lib.load()
    dx = torch.full((2, 64, h, w), float("nan"), device=DEV).contiguous(memory_format=torch.channels_last)
    dyd = _nhwc(dy)
    _lib.check(lib.munit_maxpool2_bwd(c_void_p(dyd.data_ptr()), c_void_p(sink[0].data_ptr()), c_void_p(dx.data_ptr()), 2, h, w,
                                      64, stream()), "maxpool2_bwd")
    assert not bool(torch.isnan(dx).any())
    assert torch.equal(dx.cpu().double(), dxr)          # torch's tie rule: the first maximum in row-major window order
    assert bool((dx[:, :, 2 * (h // 2):, :] == 0).all()) and bool((dx[:, :, :, 2 * (w // 2):] == 0).all())
    assert int(sink[0].max()) <= 3
    (dxa,) = torch.autograd.grad(y, [xd], dyd)
    assert torch.equal(dxa, dx)


@pytest.mark.parametrize("hw", [(16, 16), (16, 20), (31, 31)])
def test_avgpool16_against_torch(hw):
    h, w = hw
    g = torch.Generator().manual_seed(h + w)
    x = torch.randn(2, 64, h, w, generator=g)
    xr = x.double().requires_grad_(True)
    yr = F.avg_pool2d(xr, (16, 16)).squeeze()
    dy = torch.randn(2, 64, generator=g)
    (dxr,) = torch.autograd.grad(yr, [xr], dy.double())
    xd = _nhwc(x).requires_grad_(True)
    y = ops.avgpool16(xd)
    assert tuple(y.shape) == (2, 64) and nerr(y, yr) <= FWD_TOL
    (dx,) = torch.autograd.grad(y, [xd], dy.to(DEV))
    assert torch.equal(dx.cpu().double(), dxr)          # dy / 256 is exact
    (dx2,) = torch.autograd.grad(ops.avgpool16(xd), [xd], dy.to(DEV))
    assert torch.equal(dx, dx2)


# ---- guard bands (the contract of tests/kernel_contract.py / tests/conv_contract.py) -----------------------------------
def _contract(a, inputs, outs, what, launch, es=None):
    """outputs poisoned with two NaN payloads: guards and inputs intact, outputs NaN-free and bitwise equal"""
    es = es or {}
    L = Launches(a, inputs, what)
    res = []
    for k in (0, 1):
        for o in outs:
            if es.get(o, 4) == 1:
                a.bytes(o).fill_(0xA5 + k)
            else:
                poison(a.view(o, torch.float32), k)
        if "ws" in a.spans:
            a.bytes("ws").fill_(GUARD_BYTE)
        L.after(launch(), "payload %d" % k)
        for o in outs:
            if es.get(o, 4) == 4:
                assert no_nan(a.view(o, torch.float32)), "%s: NaN in %s" % (what, o)
        res.append({o: a.bytes(o).clone() for o in outs})
    for o in outs:
        assert torch.equal(res[0][o], res[1][o]), "%s: %s differs between two runs" % (what, o)
    return L


@pytest.mark.parametrize("rc", [(7, 64), (2 * 31 * 31, 128)])
def test_guard_bands_batchnorm(rc):
    lib = _lib.load()
    r, c = rc
    n, nws = r * c * 4, lib.munit_batchnorm_workspace_bytes(c)
    a = Arena(dict(x=n, dy=n, gamma=c * 4, beta=c * 4, rm=c * 4, rv=c * 4, y=n, mean=c * 8, rstd=c * 4, dx=n, dg=c * 4,
                   db=c * 4, ws=nws), torch.device(DEV))
    for i, nm in enumerate(("x", "dy", "gamma", "beta")):
        fill_random(a.view(nm, torch.float32), 60 + i)
    p = a.ptr

    def fwd(ws_bytes=nws, eval_=0):
        a.view("rm", torch.float32).fill_(0.25)
        a.view("rv", torch.float32).fill_(1.5)
        return lib.munit_batchnorm_fwd(p("x"), p("y"), p("mean"), p("rstd"), p("rm"), p("rv"), r, c, p("gamma"), p("beta"), 1,
                                       eval_, c_float(1e-5), c_float(0.1), p("ws"), ws_bytes, stream())

    L = _contract(a, ["x", "dy", "gamma", "beta"], ["y", "mean", "rstd"], "batchnorm_fwd %s" % (rc,), fwd)
    assert no_nan(a.view("rm", torch.float32)) and no_nan(a.view("rv", torch.float32))
    for o in ("y", "mean", "rstd"):
        poison(a.view(o, torch.float32), 0)
    a.bytes("ws").fill_(GUARD_BYTE)
    assert fwd(nws - 1) == ERR_WORKSPACE
    torch.cuda.synchronize()
    for o in ("y", "mean", "rstd"):
        assert bool((a.view(o, torch.int32) == POISON[4][0]).all())
    assert bool((a.bytes("ws") == GUARD_BYTE).all())
    assert bool((a.view("rm", torch.float32) == 0.25).all())          # refused: the running statistics are untouched
    L.verify("refused")
    _lib.check(fwd(), "batchnorm_fwd")

    def bwd(ws_bytes=nws):
        return lib.munit_batchnorm_bwd(p("x"), p("dy"), p("y"), p("gamma"), p("mean"), p("rstd"), p("dx"), p("dg"), p("db"),
                                       c_float(0.0), r, c, 1, p("ws"), ws_bytes, stream())

    L = _contract(a, ["x", "dy", "gamma", "y", "mean", "rstd"], ["dx", "dg", "db"], "batchnorm_bwd %s" % (rc,), bwd)
    for o in ("dx", "dg", "db"):
        poison(a.view(o, torch.float32), 0)
    a.bytes("ws").fill_(GUARD_BYTE)
    assert bwd(nws - 1) == ERR_WORKSPACE
    torch.cuda.synchronize()
    for o in ("dx", "dg", "db"):
        assert bool((a.view(o, torch.int32) == POISON[4][0]).all())
    L.verify("refused")
    # evaluation mode needs no workspace and writes y alone
    _contract(a, ["x", "gamma", "beta", "rm", "rv", "mean", "rstd"], ["y"], "batchnorm_fwd eval",
              lambda: lib.munit_batchnorm_fwd(p("x"), p("y"), None, None, p("rm"), p("rv"), r, c, p("gamma"), p("beta"), 0, 1,
                                              c_float(1e-5), c_float(0.1), None, 0, stream()))


@pytest.mark.parametrize("hw", [(5, 7), (65, 80)])
def test_guard_bands_maxpool2(hw):
    lib = _lib.load()
    h, w = hw
    b, c = 2, 64
    nx, ny = b * h * w * c, b * (h // 2) * (w // 2) * c
    a = Arena(dict(x=nx * 4, dy=ny * 4, y=ny * 4, idx=ny, dx=nx * 4), torch.device(DEV))
    fill_random(a.view("x", torch.float32), 70)
    fill_random(a.view("dy", torch.float32), 71)
    p = a.ptr
    _contract(a, ["x", "dy"], ["y", "idx"], "maxpool2_fwd %s" % (hw,),
              lambda: lib.munit_maxpool2_fwd(p("x"), p("y"), p("idx"), b, h, w, c, stream()), es={"idx": 1})
    assert int(a.bytes("idx").max()) <= 3
    _contract(a, ["x", "dy", "idx"], ["dx"], "maxpool2_bwd %s" % (hw,),
              lambda: lib.munit_maxpool2_bwd(p("dy"), p("idx"), p("dx"), b, h, w, c, stream()))


@pytest.mark.parametrize("hw", [(16, 16), (31, 17)])
def test_guard_bands_avgpool16(hw):
    lib = _lib.load()
    h, w = hw
    b, c = 2, 64
    nx = b * h * w * c
    a = Arena(dict(x=nx * 4, dy=b * c * 4, y=b * c * 4, dx=nx * 4), torch.device(DEV))
    fill_random(a.view("x", torch.float32), 72)
    fill_random(a.view("dy", torch.float32), 73)
    p = a.ptr
    _contract(a, ["x", "dy"], ["y"], "avgpool16_fwd %s" % (hw,),
              lambda: lib.munit_avgpool16_fwd(p("x"), p("y"), b, h, w, c, stream()))
    _contract(a, ["x", "dy"], ["dx"], "avgpool16_bwd %s" % (hw,),
              lambda: lib.munit_avgpool16_bwd(p("dy"), p("dx"), b, h, w, c, stream()))


# ---- the six convolution forms of the classifier at crop 256 ------------------------------------------------------------
@pytest.mark.parametrize("form", [(3, 256, 128, 32), (3, 128, 128, 32), (1, 256, 128, 32), (3, 128, 64, 16), (3, 64, 64, 16),
                                  (1, 128, 64, 16)])
def test_conv_forms_against_fp64(form):
    k, ci, co, hw = form
    g = torch.Generator().manual_seed(k * 1000 + ci + co)
    x = torch.randn(2, ci, hw, hw, generator=g)
    w = torch.randn(co, ci, k, k, generator=g) * 0.05
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = F.conv2d(xr, wr, padding=k // 2)
    dy = torch.randn(yr.shape, generator=g)
    dxr, dwr = torch.autograd.grad(yr, [xr, wr], dy.double())
    ops.set_compute("f32")
    xd, wd = _nhwc(x).requires_grad_(True), _nhwc(w).requires_grad_(True)
    y = ops.conv2d(xd, wd, None, 1, k // 2, "zero")
    dx, dw = torch.autograd.grad(y, [xd, wd], _nhwc(dy))
    errs = (nerr(y, yr), nerr(dx, dxr), nerr(dw, dwr))
    print("conv form", form, errs)
    assert errs[0] <= FWD_TOL and errs[1] <= GRAD_TOL and errs[2] <= GRAD_TOL, errs


# ---- the whole classifier ----------------------------------------------------------------------------------------------------
def _module(seed):
    from munit_amd.networks import domainClassifier
    net = domainClassifier(256)
    sd = D.make_state(seed)
    D.load_into(net, sd)
    return net.to(DEV), sd


def _run_module(net, c, t, need_weight_grads=True):
    """one forward + backward of mean((net(c) - t)^2) with the kinks recorded: loss, output, d code, weight gradients"""
    ops.set_compute("f32")
    cd = _nhwc(c).requires_grad_(True)
    with ops.kinks(dann=True) as k:
        out = net(cd, need_weight_grads)
    sink = k.dann
    loss = ops.mse_const(out, t)
    ps = [p for p in net.parameters()]
    grads = torch.autograd.grad(loss, [cd] + (ps if need_weight_grads else []), allow_unused=True)
    ops.join_side_streams()
    torch.cuda.synchronize()
    return loss, out, grads[0], list(grads[1:]), sink


@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("hw", [(64, 64), (64, 80)])
def test_classifier_against_the_oracle(b, hw):
    net, sd = _module(41)
    c = D.code(b, hw[0], hw[1], 43)
    for name, synth, fool in (("fool", False, True), ("synth", True, False), ("real", False, False)):
        t = D.target(synth, fool)
        before = {k: v.clone() for k, v in sd.items()}
        loss, out, dc, dws, sink = _run_module(net, c, t)
        assert len(sink) == D.PINS_PER_CALL
        pins = D.Pins(sink)
        cr = c.clone().requires_grad_(True)
        ps = D.params(sd)
        for p in ps:
            p.requires_grad_(True)
        o_ref = D.classifier(sd, cr, pins)
        assert pins.done() and pins.worst <= 1e-5, (pins.worst, pins.n_disagree)     # pinned only within rounding of a kink
        l_ref = torch.mean((o_ref - t) ** 2)
        g_ref = torch.autograd.grad(l_ref, [cr] + ps)
        assert tuple(out.shape) == tuple(o_ref.shape) == ((1,) if b == 1 else (b, 1))
        rel = abs(float(loss) - float(l_ref)) / abs(float(l_ref))
        e_out, e_dc = nerr(out, o_ref), nerr(dc, g_ref[0])
        e_w = {n: nerr(g, r) for n, g, r in zip(D.param_names(), dws, g_ref[1:])}
        print("classifier B=%d %s %s: loss rel %.2e out %.2e d code %.2e worst weight grad %.2e (%s), %d pinned"
              % (b, hw, name, rel, e_out, e_dc, max(e_w.values()), max(e_w, key=e_w.get), pins.n_disagree))
        assert rel <= LOSS_TOL and e_out <= FWD_TOL and e_dc <= GRAD_TOL
        assert max(e_w.values()) <= GRAD_TOL, e_w
        own = net.state_dict()
        for k in sd:
            if k.endswith(("running_mean", "running_var")):
                assert nerr(own[k], sd[k]) <= FWD_TOL, k
                assert not torch.equal(sd[k], before[k])
            elif k.endswith("num_batches_tracked"):
                assert int(own[k]) == int(sd[k])
        for p in ps:
            p.requires_grad_(False)


def test_classifier_without_weight_gradients_is_bitwise_the_same():
    net, _ = _module(41)
    c = D.code(2, 64, 64, 43)
    for p in net.parameters():
        p._munit_grad = torch.zeros_like(p)            # what binding to an optimizer's flat buffer provides
    _, _, dc, _, _ = _run_module(net, c, 0.5)
    assert any(bool((p._munit_grad != 0).any()) for p in net.parameters())
    for p in net.parameters():
        p._munit_grad.fill_(3.0)
    loss, _, dc2, dws, _ = _run_module(net, c, 0.5, need_weight_grads=False)
    assert torch.equal(dc, dc2)
    assert all(bool((p._munit_grad == 3.0).all()) for p in net.parameters())
    assert all(p.requires_grad for p in net.parameters())
    _, _, dc3, _, _ = _run_module(net, c, 0.5, need_weight_grads=False)
    assert torch.equal(dc2, dc3)                        # a second backward is bitwise the first
    with pytest.raises(ValueError, match="16..31"):
        net(torch.zeros(1, 256, 32, 64, device=DEV))


# ---- the trainer's two updates ------------------------------------------------------------------------------------------------
def _hp(optimizer="adam", **adaptation):
    hp = O.default_hp(256, 2, 1)
    hp["gen"]["n_res"] = 1
    hp["dis"]["num_scales"] = 1
    hp["optimizer"] = optimizer
    hp["adaptation"].update(adaptation)
    return hp


def _trainer(hp, seed=0):
    from munit_amd.trainer import MUNIT_Trainer
    torch.manual_seed(seed)
    return MUNIT_Trainer(hp).to(DEV)


def _batch():
    x_a, x_b, m_a, m_b = O.synthetic_batch(2, 256)
    return [t.to(DEV) for t in (x_a, x_b, m_a, m_b)]


def _oracle_of(tr):
    sd_a = {k: v.detach().cpu().double().clone() for k, v in tr.domain_classifier_sr_a.state_dict().items()}
    sd_b = {k: v.detach().cpu().double().clone() for k, v in tr.domain_classifier_sr_b.state_dict().items()}
    sd_a = {k: (v.long() if k.endswith("tracked") else v) for k, v in sd_a.items()}
    sd_b = {k: (v.long() if k.endswith("tracked") else v) for k, v in sd_b.items()}
    return sd_a, sd_b


def _codes(tr, x_a, x_b):
    with torch.no_grad():
        return (tr._content_enc(1)(ops.nhwc(x_a)).cpu().double(), tr._content_enc(2)(ops.nhwc(x_b)).cpu().double())


def _compare_classifiers(tr, sd_a, sd_b, what, lr, opt=None):
    """Running statistics as forward tensors; the weights by tests/parity.py's rule for an optimizer step (Adam's first steps
    are sign-like -- |step| ~ lr whatever |g| is -- so an element whose gradient is below fp32 noise may step the other way:
    at most 4 lr in absolute terms and 2e-4 relative L2 per tensor); the Adam moments, linear / quadratic in the gradients,
    within 2 x 5e-5 relative L2 (`opt`: the oracle's optimizer after the same step)."""
    from tests.parity import l2err
    worst = dict(stat=0.0, weight_abs=0.0, weight_l2=0.0, moment_l2=0.0)
    for net, sd in ((tr.domain_classifier_sr_a, sd_a), (tr.domain_classifier_sr_b, sd_b)):
        own = net.state_dict()
        for k, v in sd.items():
            if k.endswith("tracked"):
                assert int(own[k]) == int(v), (what, k)
            elif k.endswith(("running_mean", "running_var")):
                worst["stat"] = max(worst["stat"], nerr(own[k], v))
                assert nerr(own[k], v) <= FWD_TOL, (what, k, nerr(own[k], v))
            else:
                a, r = own[k].detach().double().cpu(), v.detach()
                worst["weight_abs"] = max(worst["weight_abs"], float((a - r).abs().max()))
                worst["weight_l2"] = max(worst["weight_l2"], l2err(a, r))
                assert float((a - r).abs().max()) <= 4.0 * lr and l2err(a, r) <= 2e-4, (what, k, worst)
    if opt is not None:
        ms, vs = (opt.state.m, opt.state.v) if opt.extra else (opt.m, opt.v)
        for (mv, vv), om, ov in zip(tr.classif_opt_sr._views, ms, vs):
            worst["moment_l2"] = max(worst["moment_l2"], l2err(mv, om), l2err(vv, ov))
        assert worst["moment_l2"] <= 2 * GRAD_TOL, (what, worst)
    return worst


_pins = D.trainer_pins


@pytest.mark.parametrize("optimizer", ["adam", "extraadam"])
def test_the_sequence_of_updates_against_the_oracle(optimizer):
    """dis_update, gen_update, domain_classifier_sr_update(real), gen_update(synth=True), domain_classifier_sr_update(synth)
    at crop 256, batch 2: the classifier side of every step -- loss_classifier_sr, its share of loss_gen_total, the
    classifier update's loss, the Adam moments and the classifiers' weights after each optimizer step, and their running
    statistics -- against
    tests/featda_oracle.py run on the content codes the HIP encoders produced.  Every loss and every generator gradient of the
    step against the full fp64 step oracle: test_step_parity_with_the_fooling_term."""
    hp = _hp(optimizer, adv_lambda=6, dfeat_lambda=1)
    tr = _trainer(hp)
    x_a, x_b, m_a, m_b = _batch()
    sd_a, sd_b = _oracle_of(tr)
    opt = D.ClassifierOptimizer(sd_a, sd_b, hp)
    tr.dis_update(x_a, x_b, hp)
    for it, synth in ((0, False), (1, True)):
        tr.iterations = it
        c_a, c_b = _codes(tr, x_a, x_b)
        with ops.kinks(dann=True) as k:
            tr.gen_update(x_a, x_b, hp, m_a, m_b, synth=synth)
        torch.cuda.synchronize()
        sink = k.dann
        assert len(sink) == 2 * D.PINS_PER_CALL
        l_ref, _, _ = D.fool_term(sd_a, sd_b, c_a, c_b, pins=_pins(sink))
        rel = abs(float(tr.loss_classifier_sr) - float(l_ref)) / abs(float(l_ref))
        print("gen_update it %d (%s): loss_classifier_sr %.6f rel %.2e" % (it, optimizer, float(tr.loss_classifier_sr), rel))
        assert rel <= LOSS_TOL
        total = float(tr.loss_gen_total)
        parts = (hp["gan_w"] * (float(tr.loss_gen_adv_a) + float(tr.loss_gen_adv_b))
                 + hp["recon_x_w"] * (float(tr.loss_gen_recon_x_a) + float(tr.loss_gen_recon_x_b))
                 + hp["recon_s_w"] * (float(tr.loss_gen_recon_s_a) + float(tr.loss_gen_recon_s_b))
                 + hp["recon_c_w"] * (float(tr.loss_gen_recon_c_a) + float(tr.loss_gen_recon_c_b))
                 + hp["recon_x_cyc_w"] * (float(tr.loss_gen_cycrecon_x_a) + float(tr.loss_gen_cycrecon_x_b))
                 + 6 * float(l_ref))
        assert abs(total - parts) <= 1e-5 * abs(parts), (total, parts)
        _compare_classifiers(tr, sd_a, sd_b, "after gen_update %d" % it, hp["lr"])      # weights untouched, running statistics moved
        # the classifier's own update on the generator's NEW weights
        c_a, c_b = _codes(tr, x_a, x_b)
        with ops.kinks(dann=True) as k:
            tr.domain_classifier_sr_update(x_a, x_b, synth, hp["adaptation"]["dfeat_lambda"], it)
        torch.cuda.synchronize()
        sink = k.dann
        l_ref = D.classifier_update(sd_a, sd_b, opt, c_a, c_b, synth, hp["adaptation"]["dfeat_lambda"], it,
                                    pins=_pins(sink))
        rel = abs(float(tr.loss_classifier_sr_update) - float(l_ref)) / abs(float(l_ref))
        worst = _compare_classifiers(tr, sd_a, sd_b, "after classifier update %d" % it, hp["lr"], opt)
        print("classifier update it %d (%s): loss %.6f rel %.2e, %s" % (it, optimizer, float(l_ref), rel, worst))
        assert rel <= LOSS_TOL
    if optimizer == "extraadam":
        assert (opt.n_extrapolations, opt.n_steps) == (1, 1)
        assert tr.classif_opt_sr._step == 2 and not tr.classif_opt_sr._has_copy
    else:
        assert tr.classif_opt_sr._step == 2


def _step_parity(monkeypatch, iters, **over):
    """tests/parity.run_step_parity (every loss 1e-5 relative, every generator gradient 5e-5 normalised max and relative L2
    with the kinks pinned, Adam moments, the weight step) at crop 256, batch 2, n_res 1, num_scales 1 with adv_lambda: 6 /
    dfeat_lambda: 1: dis_update, gen_update, domain_classifier_sr_update(real), dis_update, gen_update(synth=True),
    domain_classifier_sr_update(synth).  The classifier updates run on the HIP side between the compared steps (their own
    parity: test_the_sequence_of_updates_against_the_oracle), so the second gen_update meets classifiers that have stepped."""
    from munit_amd.trainer import MUNIT_Trainer
    from tests.parity import run_step_parity
    shared = {"reused": [], "n": 0}
    monkeypatch.setattr(O, "OracleTrainer", D.oracle_trainer_class(shared))
    plain = MUNIT_Trainer.gen_update

    def gen_update(self, xa, xb, hp, mask_a=None, mask_b=None):
        synth = shared["n"] % 2 == 1
        shared["n"] += 1
        shared["sd"] = _oracle_of(self)
        with ops.kinks(dann=True) as k:
            plain(self, xa, xb, hp, mask_a, mask_b, synth=synth)
        shared["sink"] = k.dann
        shared["reused"].append(self.fwd_reused)
        torch.cuda.synchronize()
        # the oracle of this gen_update runs next and moves shared["sd"]'s running statistics: compared afterwards
        with ops.kinks(mask=None, l1=None):         # the classifier's own update is not part of the compared step
            shared["stats"] = {pre + k: v.clone() for pre, m in (("a.", self.domain_classifier_sr_a),
                                                                  ("b.", self.domain_classifier_sr_b))
                               for k, v in m.state_dict().items()}
            self.domain_classifier_sr_update(xa, xb, synth, hp["adaptation"]["dfeat_lambda"], self.iterations)

    monkeypatch.setattr(MUNIT_Trainer, "gen_update", gen_update)
    hp_over = {"gen": {"n_res": 1}, "dis": {"num_scales": 1}, "adaptation": {"adv_lambda": 6, "dfeat_lambda": 1}}
    hp_over.update(over)
    rep = run_step_parity(size=256, batch=2, gen_state=1, iters=iters, device=DEV, hp_overrides=hp_over)
    # the running statistics the HIP gen_update left (before the classifier update that followed) against the oracle's
    sd_a, sd_b = shared["after"]
    for pre, sd in (("a.", sd_a), ("b.", sd_b)):
        for k, v in sd.items():
            if k.endswith(("running_mean", "running_var")):
                assert nerr(shared["stats"][pre + k], v) <= FWD_TOL, (pre + k, nerr(shared["stats"][pre + k], v))
    print("featda step parity %s: loss_classifier_sr %.6f, losses %.2e rel, gradients %.2e max %.2e L2, pinned kinks %.2e"
          % (over, rep["loss_classifier_sr"], rep["loss_rel"], rep["grad_nerr"], rep["grad_l2"], shared["worst"]))
    assert rep["loss_classifier_sr"] > 0 and shared["worst"] <= 5e-5           # tests/parity.KINK_NOISE
    assert rep["grad_nerr"] <= GRAD_TOL and rep["grad_l2"] <= GRAD_TOL and rep["loss_rel"] <= LOSS_TOL, rep
    return rep, shared


def test_step_parity_with_the_fooling_term(monkeypatch):
    """Every loss (loss_classifier_sr and loss_gen_total with its 6 x share included) and every generator gradient of the
    real and of the synthetic iteration against the fp64 OracleTrainer that adds the term on its own content codes."""
    rep, shared = _step_parity(monkeypatch, iters=2)
    assert shared["reused"] == [False, False] and shared["n"] == 2


def test_fooling_term_on_the_reused_forward_matches_the_plain_step():
    """reuse_dis_forward: 1 -- gen_update continues from dis_update's forward and tape: the term is built on the kept codes
    and its gradient reaches the encoders through them.  Bounds of test_gpu_step.test_reuse_dis_forward_matches_the_plain_step
    against the plain step (which test_step_parity_with_the_fooling_term holds to the oracle): every loss bit for bit, the
    generator gradient to fp32 summation order (1e-5 relative L2)."""
    from tests.parity import l2err
    x_a, x_b, m_a, m_b = _batch()
    res = []
    for reuse in (0, 1):
        hp = _hp(adv_lambda=6, dfeat_lambda=1)
        hp["reuse_dis_forward"] = reuse
        tr = _trainer(hp)
        tr.dis_update(x_a, x_b, hp)
        tr.gen_update(x_a, x_b, hp, m_a, m_b)
        torch.cuda.synchronize()
        assert tr.fwd_reused == bool(reuse)
        res.append((tr.gen_opt.flat_g.clone(), {n: float(getattr(tr, n).detach()) for n in vars(tr)
                                                if n.startswith("loss_") and torch.is_tensor(getattr(tr, n))}))
    assert "loss_classifier_sr" in res[0][1] and res[0][1] == res[1][1]
    assert l2err(res[1][0], res[0][0]) <= 1e-5, l2err(res[1][0], res[0][0])


def test_multi_stream_gen_update_is_bitwise_the_single_stream_one(monkeypatch):
    from munit_amd import trainer as T
    hp = _hp(adv_lambda=6, dfeat_lambda=1)
    x_a, x_b, m_a, m_b = _batch()
    res = []
    for streams in (True, False):
        monkeypatch.setattr(T, "BRANCH_STREAMS", streams)
        tr = _trainer(hp)
        tr.gen_update(x_a, x_b, hp, m_a, m_b)
        torch.cuda.synchronize()
        res.append((tr.gen_opt.flat_g.clone(), tr.loss_classifier_sr.clone(), tr.loss_gen_total.clone(),
                    tr.domain_classifier_sr_a.BasicBlock2.bn2.running_var.clone()))
        assert bool((tr.classif_opt_sr.flat_g == 0).all())       # no classifier weight gradient is formed in gen_update
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert float(res[0][0].abs().max()) > 0


def test_zero_weights_launch_none_of_the_new_kernels():
    hp = _hp()
    tr = _trainer(hp)
    x_a, x_b, m_a, m_b = _batch()
    with Calls(NEW) as calls:
        tr.dis_update(x_a, x_b, hp)
        tr.gen_update(x_a, x_b, hp, m_a, m_b)
        torch.cuda.synchronize()
    assert calls == [] and tr.loss_classifier_sr == 0
    on = _hp(adv_lambda=6, dfeat_lambda=1)
    tr = _trainer(on)
    with Calls(NEW) as calls:
        tr.gen_update(x_a, x_b, on, m_a, m_b)
        torch.cuda.synchronize()
    # two classifiers: 2 max-pools, 6 batch norms and 1 average each, forward and backward
    assert calls.count("munit_maxpool2_fwd") == calls.count("munit_maxpool2_bwd") == 4
    assert calls.count("munit_batchnorm_fwd") == calls.count("munit_batchnorm_bwd") == 12
    assert calls.count("munit_avgpool16_fwd") == calls.count("munit_avgpool16_bwd") == 2
