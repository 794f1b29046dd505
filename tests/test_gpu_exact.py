"""GPU: zero-tolerance checks of values (tests/lattice.py holds the argument, the inputs and the fp64 reference;
tests/test_cpu_lattice.py checks the conditions on the reference without a device; DESIGN.md, "Bit-exact checks on
integer-lattice data").

a. Exact regime: every convolution case the suite lists (CONV_CASES in fp32, test_gpu_bf16's CASES / WGRAD_CASES in the bf16
   compute mode, F32X3_CASES, test_gpu_bf16s's CASES, LINEAR_CASES), at its own shape, on small-integer data whose exact
   results are on the bf16 grid: forward with bias and the case's activation, backward-data with and without `add`,
   backward-weight and db at beta = 0 and accumulating at beta = 1 must EQUAL the integer reference.  A tanh case runs with
   act = "none" (same kernels: tests/test_cpu_lattice.py).  The backward of a fused LeakyReLU multiplies dy by 0.2 and leaves
   the lattice, so there the three passes are driven on the lattice dy through the raw entry points (what _Conv2d.backward
   calls after munit_act_bwd) and munit_act_bwd is compared with the single fp32 product apart.
b. Rounding regime (bf16-storage cases): dense odd lattices whose exact outputs leave the bf16 grid and hit ties; y and dx
   must equal one_rounding / two_rounding of the exact result (the model follows from the kernel name), dw and db the exact
   integers.
c. munit_l1_mean_bwd(_bf16), munit_scale, munit_add_relu_fwd, munit_act_bwd, munit_avgpool3s2_fwd/bwd, munit_gap_fwd/bwd:
   exact on lattice data with power-of-two divisors (the average pool: the single fp32 division).
d. The norm kernels writing bf16 and the tanh image head reading bf16: per element |got - ref| <= ulp_bf16(ref) / 2 +
   T * max|ref| with T the fp32 bound of the pass (2e-5 forward, 1e-4 backward), and the signed mean rounding error within
   +/- 0.05 ulp.

"Equal" is torch.equal on the values (+0 and -0 compare equal; a NaN does not)."""
import pytest
import torch

from tests import lattice as L
from tests.lattice import BF, F32

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def to_dev(t, dtype=F32):
    t = t.to(dtype).to(dev())
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.contiguous()


@pytest.fixture(scope="module")
def lib():
    from munit_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def restore_compute():
    from munit_amd import ops
    yield
    ops.set_compute("f32")


def same(got, want, what):
    """Assert got == want element for element; on a mismatch report how many differ and the first few coordinates (which
    border, tile edge or channel residue), with both values."""
    got = got.detach().cpu()
    want = want.to(got.dtype)
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    bad = (got != want) | (got != got)
    idx = bad.nonzero()[:8].tolist()
    rows = [(tuple(i), float(got[tuple(i)]), float(want[tuple(i)])) for i in idx]
    raise AssertionError("%s: %d of %d elements differ; first (index, got, want): %s" % (what, int(bad.sum()), bad.numel(), rows))


def run_conv_case(lib, entry, inp, act, exact):
    """Drive the three passes of one case through munit_amd.ops and compare every result with the reference.  exact: the
    exact regime (adds the beta = 1 accumulation)."""
    from munit_amd import ops
    case, compute, din, dout = entry
    cin, cout, k, stride, pad, pt, ups, _, B, H, W = case
    ref = L.conv_reference(case, inp["x"], inp["w"], inp["b"], inp["dy"], act=act)
    if exact:       # on the reference, before the device is looked at
        cond = L.exact_regime_conditions(entry, inp, ref)
        assert all(cond.values()), cond
    names = L.kernel_names(lib, entry, act)
    rep = 2 if L.twin(case) else 1      # twin batch: the device runs every sample twice, the reference once
    cat = lambda t: torch.cat([t] * rep) if rep > 1 else t
    what = lambda s: "%s %s [%s]" % (L.case_id(entry), s, " | ".join(names))

    ops.set_compute(compute)
    xd = to_dev(cat(inp["x"]), din).requires_grad_(True)
    wd = to_dev(inp["w"]).requires_grad_(True)
    bd = to_dev(inp["b"]).requires_grad_(True)
    y = ops.conv2d(xd, wd, bd, stride, pad, pt, bool(ups), act, out_dtype=dout)
    assert y.dtype == dout
    same(y, cat(L.activated(ref["pre"], act, dout)), what("forward"))

    dx_bf16 = din == BF
    model = L.dgrad_rounding_model(names[1], dx_bf16, False)
    dyd = to_dev(cat(inp["dy"]), dout)
    gd = to_dev(cat(ref["g"]), dout)            # gradient at the pre-activation output: what backward-data / -weight receive
    shape = tuple(xd.shape)
    if act == "lrelu":
        got = ops.act_bwd_raw("lrelu", L.LRELU_SLOPE, y.detach(), dyd)
        dy32 = cat(inp["dy"]).float()
        same(got, torch.where(cat(ref["pre"]) > 0, dy32, dy32 * torch.tensor(L.LRELU_SLOPE, dtype=F32)), what("act_bwd"))
        dx = ops.conv2d_dgrad_raw(gd, wd.detach(), shape, stride, pad, pt, bool(ups), x_dtype=din)
        dw, db = ops.conv2d_wgrad_raw(xd.detach(), gd, tuple(wd.shape), stride, pad, pt, bool(ups))
    else:
        y.backward(dyd)
        dx, dw, db = xd.grad, wd.grad, bd.grad
    assert dx.dtype == din and dw.dtype == F32 and db.dtype == F32
    same(dx, cat(L.expected_dx(ref, model, din)), what("backward-data (%s rounding)" % model))
    same(dw, rep * ref["dw"], what("backward-weight"))
    same(db, rep * ref["db"], what("db"))

    addd = to_dev(cat(inp["add"]), din)
    if L.dgrad_takes_add(names[1], dx_bf16):
        model = L.dgrad_rounding_model(names[1], dx_bf16, True)
        dxa = ops.conv2d_dgrad_raw(gd, wd.detach(), shape, stride, pad, pt, bool(ups), add=addd, x_dtype=din)
        same(dxa, cat(L.expected_dx(ref, model, din, inp["add"])), what("backward-data + add (%s rounding)" % model))
    else:       # the folded gathers have no bf16 `add`: refused, not computed wrongly
        with pytest.raises(RuntimeError, match="add"):
            ops.conv2d_dgrad_raw(gd, wd.detach(), shape, stride, pad, pt, bool(ups), add=addd, x_dtype=din)
    if exact:
        dwb, dbb = to_dev(inp["dw0"]), to_dev(inp["db0"])
        ops.conv2d_wgrad_raw(xd.detach(), gd, tuple(wd.shape), stride, pad, pt, bool(ups), dw=dwb, db=dbb, beta=1.0)
        same(dwb, inp["dw0"] + rep * ref["dw"], what("backward-weight, beta = 1"))
        same(dbb, inp["db0"] + rep * ref["db"], what("db, beta = 1"))
    return ref


@pytest.mark.parametrize("entry", [e for e in L.exact_cases() if e not in [l[0] for l in L.LEFT_OUT]], ids=L.case_id)
def test_exact_regime(lib, entry):
    act = "none" if entry[0][7] == "tanh" else entry[0][7]
    run_conv_case(lib, entry, L.exact_inputs(entry), act, exact=True)


@pytest.mark.parametrize("entry", L.rounding_cases(), ids=L.case_id)
def test_rounding_regime(lib, entry):
    case, compute, din, dout = entry
    inp = L.rounding_inputs(entry)
    ref = run_conv_case(lib, entry, inp, "none", exact=False)
    for name, t, dt in (("y", ref["pre"], dout), ("dx", ref["dx"], din)):       # the case did leave the grid
        assert dt != BF or 1 - float(L.exactly_bf16(t).double().mean()) >= 0.2, (entry, name)


# ------------------------------------------------------------------------------------------------------------------------
# c. losses and pointwise kernels
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_l1_mean_backward_is_exact(dtype, masked):
    """N = 2 * 64 * 8 * 8 = 2^13 and gout = 2^-3: da = -db = sign(a - b) * 2^-16 exactly (0 where a == b, and under the mask);
    the loss itself is an integer sum over 2^13."""
    from munit_amd import ops
    shape = (2, 64, 8, 8)
    a, b = L.lattice(shape, 21, range(-2, 3)), L.lattice(shape, 22, range(-2, 3))
    assert 0.1 < float((a == b).double().mean()) < 0.4
    m = L.lattice((2, 1, 8, 8), 23, (0, 1)) if masked else None
    ad, bd = to_dev(a, dtype).requires_grad_(True), to_dev(b, dtype).requires_grad_(True)
    out = ops.l1_mean(ad, bd, to_dev(m) if masked else None)
    keep = (1 - m) if masked else torch.ones(1, dtype=torch.float64)
    same(out, ((a - b).abs() * keep).sum() / a.numel(), "l1 forward")
    gout = 2.0 ** -3
    torch.autograd.backward([out], [torch.tensor(gout, device=dev())])
    g = gout / a.numel() * torch.sign(a - b) * keep
    assert bool(L.exactly_bf16(g).all()) and ad.grad.dtype == dtype
    same(ad.grad, g, "l1 da")
    same(bd.grad, -g, "l1 db")


def test_pointwise_kernels_are_exact():
    from munit_amd import ops
    x = L.lattice((1027,), 31, range(-9, 10))
    for alpha in (0.25, 3.0, -2.0):
        same(ops.scale_(to_dev(x), alpha), x * alpha, "scale %g" % alpha)
    a, r = L.lattice((2, 64, 5, 7), 32, range(-3, 4)), L.lattice((2, 64, 5, 7), 33, range(-3, 4))
    dy = L.lattice((2, 64, 5, 7), 34, range(-5, 6))
    ad, rd = to_dev(a).requires_grad_(True), to_dev(r).requires_grad_(True)
    y = ops.add_relu(ad, rd)
    same(y, (a + r).clamp_min(0), "add_relu forward")
    y.backward(to_dev(dy))
    same(ad.grad, dy * (a + r > 0), "add_relu da")
    same(rd.grad, dy * (a + r > 0), "add_relu dr")
    yy, g = L.lattice((1, 3, 7, 9), 35, range(-2, 3)), L.lattice((1, 3, 7, 9), 36, range(-7, 8))
    same(ops.act_bwd_raw("relu", 0.0, to_dev(yy), to_dev(g)), g * (yy > 0), "act_bwd relu")
    g32 = g.float()
    same(ops.act_bwd_raw("lrelu", L.LRELU_SLOPE, to_dev(yy), to_dev(g)),
         torch.where(yy > 0, g32, g32 * torch.tensor(L.LRELU_SLOPE, dtype=F32)), "act_bwd lrelu")


@pytest.mark.parametrize("shape", [(2, 3, 9, 13), (1, 5, 1, 4), (2, 64, 4, 6), (1, 3, 2, 2)], ids=lambda s: "%dx%dx%dx%d" % s)
def test_avgpool_is_exact(shape):
    """Window counts are 9, 6, 4, 3, 2 or 1.  Backward: dy in multiples of 36 makes every dy / count an integer.  Forward: the
    window sum is an integer, the kernel divides it once in fp32."""
    from munit_amd import ops
    import torch.nn.functional as F
    from oracle import munit_oracle as O
    x = L.lattice(shape, 41, range(-4, 5))
    xr = x.clone().requires_grad_(True)
    yr = O.avgpool_3s2(xr)
    dy = 36 * L.lattice(tuple(yr.shape), 42, range(-2, 3))
    yr.backward(dy)
    assert bool((xr.grad == xr.grad.round()).all())
    sums = F.avg_pool2d(x, 3, stride=2, padding=1, divisor_override=1)
    cnt = F.avg_pool2d(torch.ones_like(x), 3, stride=2, padding=1, divisor_override=1)
    xd = to_dev(x).requires_grad_(True)
    y = ops.avgpool3s2(xd)
    same(y, sums.float() / cnt.float(), "avgpool forward")
    y.backward(to_dev(dy))
    same(xd.grad, xr.grad, "avgpool backward")


def test_global_avgpool_is_exact():
    from munit_amd import ops
    shape = (3, 100, 8, 8)          # HW = 64
    x, dy = L.lattice(shape, 43, range(-4, 5)), L.lattice((3, 100, 1, 1), 44, range(-4, 5))
    xd = to_dev(x).requires_grad_(True)
    y = ops.global_avgpool(xd)
    same(y, x.sum(dim=(2, 3), keepdim=True) / 64, "gap forward")
    y.backward(to_dev(dy))
    same(xd.grad, (dy / 64).expand(shape), "gap backward")


# ------------------------------------------------------------------------------------------------------------------------
# d. bf16 outputs that are not exact: rounded to nearest, per element
# ------------------------------------------------------------------------------------------------------------------------
def _held(got, ref, tol, what, keep=None, rounded=True):
    excess, mean, mean_mag, n = L.rounding_check(got, ref, tol, keep)
    print("measured: %s excess over ulp/2 + %g max: %.3g, signed mean error %.4f ulp (towards zero: %.4f), %d elements"
          % (what, tol, excess, mean, mean_mag, n))
    assert excess <= 0, (what, excess)
    if rounded:
        assert abs(mean) <= 0.05 and abs(mean_mag) <= 0.05, (what, mean, mean_mag)


@pytest.mark.parametrize("shape", L.NORM_SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
@pytest.mark.parametrize("kind", L.NORM_KINDS)
def test_bf16_norms_round_to_nearest(kind, shape):
    from munit_amd import ops
    C = shape[1]
    d = L.norm_inputs(kind, shape)
    leaves = {n: d[n].clone().requires_grad_(True) for n in ("x", "params", "gamma", "beta") if n in d}
    pre = L.norm_pre(kind, d, leaves)
    ops.set_compute("bf16s")
    xd = to_dev(d["x"], BF).requires_grad_(True)
    if kind == "in":
        y = ops.instance_norm(xd)
    elif kind == "in_res":
        y = ops.instance_norm(xd, relu=False, residual=to_dev(d["res"], BF))
    elif kind == "adain_relu":
        y = ops.adain(xd, to_dev(d["params"]), C, 0, relu=True)
    else:
        y = ops.layer_norm(xd, to_dev(d["gamma"]), to_dev(d["beta"]), relu=True)
    assert y.dtype == BF
    keep, yr = None, pre
    if kind.endswith("relu"):
        # elements within T * max of the kink are left out of the forward comparison (<= 1 %); everywhere else the device
        # took the reference's branch, and the reference's backward takes the device's branches
        near = L.near_kink(pre.detach(), L.FWD_TOL)
        assert float(near.double().mean()) <= 0.01
        mask = (y.detach().float() > 0).cpu()
        assert not bool((((pre.detach() > 0) != mask) & ~near).any()), "a ReLU branch differs away from the kink"
        keep, yr = ~near, torch.where(mask, pre, torch.zeros_like(pre))
    _held(y, yr, L.FWD_TOL, "%s y" % kind, keep)
    yr.backward(d["dy"])
    y.backward(to_dev(d["dy"], BF))
    assert xd.grad.dtype == BF
    _held(xd.grad, leaves["x"].grad, L.BWD_TOL, "%s dx" % kind)


@pytest.mark.parametrize("entry", L.HEAD_CASES, ids=L.case_id)
def test_tanh_head_reads_bf16(entry):
    """The image head of a bf16-storage generator: bf16 activations in, fp32 weights, an fp32 image out.  Nothing is rounded
    to bf16, so the per-element bound is the fp32 forward bound alone."""
    from munit_amd import ops
    from oracle import munit_oracle as O
    cin, cout, k, stride, pad, pt, ups, act, B, H, W = entry[0]
    x = L.rne_bf16(L.rnd((B, cin, H, W), 1)).double()
    w = L.rnd((cout, cin, k, k), 2, (2.0 / (cin * k * k)) ** 0.5).float().double()
    b = L.rnd((cout,), 3, 0.1).float().double()
    yr = O.conv_block(x, w, b, stride, pad, pt, None, act)
    ops.set_compute("bf16s")
    y = ops.conv2d(to_dev(x, BF), to_dev(w), to_dev(b), stride, pad, pt, False, act, out_dtype=F32)
    assert y.dtype == F32
    err = float((y.double().cpu() - yr).abs().max())
    print("measured: tanh head max |got - ref| = %.3g, bound %.3g" % (err, L.FWD_TOL * float(yr.abs().max())))
    assert err <= L.FWD_TOL * float(yr.abs().max()), err
