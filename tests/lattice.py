"""Helper of tests/test_gpu_exact.py and tests/test_cpu_lattice.py (neither a test module nor a conftest): convolution data
on a small-integer lattice, the fp64 reference of every pass, and the rounding models of a bf16 output.

The argument ("Bit-exact checks on integer-lattice data"): on small-integer inputs every product and every partial
sum of a convolution is an integer far below 2^24 -- in fp32, in bf16 operands (integers up to 256 are exact) and in the
three-way bf16 split -- so every correct kernel, whatever its tiling, split over K, Winograd or sub-pixel form, must
produce the SAME BITS as the integer reference.  A wrong tap, pixel, channel, tail or border fold changes an integer.

Exact regime (exact_inputs): x in {-1, 0, 1} with a quarter non-zero, w in 4 x {-1, 0, 1} uniform, dy in 4 x {-1, 0, 1} with a
quarter non-zero.  The multiplier 4 keeps the Winograd transforms of munit_amd/csrc/wino.h on the integers: G of
F(2x2, 3x3) and of F(3x3, 2x2) carries 1/2, so G g G^T carries 1/4 (forward, backward-data, the merged sub-pixel filters
-- sums of up to four weights -- alike), and the G-type transform of dy in the Winograd backward-weight (G^T S G applied to
the slab sums in wino_wgrad_reduce_kernel) divides sums of x * dy by 4.  No form of wino.h needs a larger power of two.
bias (4 x {-1, 0, 1}), `add` (16 x {-1, 0, 1}) and the backward-weight accumulation buffers keep every sum on the bf16 grid
at its magnitude (multiples of 4 up to 1024, of 16 up to 4096), so every rounding of the exact regime is the identity.

Rounding regime (rounding_inputs): dense odd lattices whose amplitudes are chosen per case so that the exact outputs
leave the bf16 grid (>= 20 % of each bf16 output tensor) and hit exact ties (>= 1 % over the case list); a half-integer
bias.  A bf16 output then pins round-to-nearest-even and WHERE the kernel rounds:
  one_rounding   rne_bf16(exact)
  two_rounding   backward-data forms that keep the padded-domain gradient in bf16 and fold it (fold_kernel<bf16_t>): the exact
                 gradient w.r.t. the padded (and up-sampled) input is rounded to bf16, pushed through the adjoint of pad /
                 upsample, `add` is added, and the sum is rounded once more.
Which one a case takes is decided from munit_conv2d_kernel_name (dgrad_rounding_model), never per case."""
import ctypes

import torch
import torch.nn.functional as F

from oracle import munit_oracle as O

BF, F32 = torch.bfloat16, torch.float32
LRELU_SLOPE = 0.2


def lattice(shape, seed, values=(-1, 0, 1), density=None):
    """fp64 tensor with entries from the small set `values`.  density None: uniform over `values`; else that share of the
    entries is drawn uniformly from the non-zero values and the rest is 0."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor(sorted(values), dtype=torch.float64)
    if density is None:
        return vals[torch.randint(len(vals), tuple(shape), generator=g)]
    nz = vals[vals != 0]
    t = nz[torch.randint(len(nz), tuple(shape), generator=g)]
    return t * (torch.rand(tuple(shape), generator=g) < density)


def rne_bf16(t):
    """Round to nearest even into bf16 (CPU); tests/test_cpu_lattice.py pins it against bit arithmetic."""
    return t.float().bfloat16()


def exactly_bf16(t):
    return rne_bf16(t).double() == t.double()


def ulp_bf16(t):
    """Spacing of the bf16 grid at |t| (8 significant bits), elementwise, as fp64; at 0 that of the smallest normal."""
    _, e = torch.frexp(t.double().abs().clamp_min(2.0 ** -126))          # |t| = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(t, dtype=torch.float64), e - 8)


def is_tie(t):
    """Exact values that lie half-way between two bf16 neighbours."""
    return (rne_bf16(t).double() - t.double()).abs() * 2 == ulp_bf16(t)


# ------------------------------------------------------------------------------------------------------------------------
# the case lists of the suite, in one form: (case, compute, din, dout) with case = (cin, cout, k, stride, pad, pad_type, ups,
# act, B, H, W)
# ------------------------------------------------------------------------------------------------------------------------
def _bf16s_case(c):
    return (c[:5] + (c[12] if len(c) > 12 else "reflect",) + c[5:10], "bf16s", c[10], c[11])


def exact_cases():
    """Every convolution case the suite lists, once per (case, arithmetic, tensor types): CONV_CASES in fp32, test_gpu_bf16's
    CASES and WGRAD_CASES under the bf16 compute mode, F32X3_CASES, test_gpu_bf16s's CASES (with BF16S_CASES_TARGETS) and
    LINEAR_CASES as the 1x1 convolutions ops.linear runs."""
    from tests import test_gpu_bf16 as B16, test_gpu_bf16s as B16S, test_gpu_f32x3 as X3, test_gpu_ops as T
    out = [(tuple(c), "f32", F32, F32) for c in T.CONV_CASES]
    out += [((k, n, 1, 1, 0, "zero", 0, a, b, 1, 1), "f32", F32, F32) for b, k, n, a in T.LINEAR_CASES]
    out += [(tuple(c), "bf16", F32, F32) for c in B16.CASES]
    out += [((ci, co, k, s, p, pt, u, "none", b, h, w), "bf16", F32, F32) for ci, co, k, s, p, pt, u, b, h, w in B16.WGRAD_CASES]
    out += [(tuple(c), "f32x3", F32, F32) for c in X3.F32X3_CASES]
    out += [_bf16s_case(c) for c in B16S.CASES]
    seen, uniq = set(), []
    for e in out:
        if e not in seen:
            seen.add(e)
            uniq.append(e)
    return uniq


def rounding_cases():
    """The bf16-storage cases (none of them runs on Winograd: tests/test_cpu_lattice.py checks the names)."""
    from tests import test_gpu_bf16s as B16S
    return [_bf16s_case(c) for c in B16S.CASES]


# Cases left out of the exact regime because their CPU reference exceeds about 10 s: (case entry, reason, the smallest
# same-kernel sibling that runs in its place).  At most two; none is needed -- the largest reference, the 6 x 192 x 192 layer,
# takes the twin-batch trick (twin) and about 1 s.
LEFT_OUT = []


def twin(case):
    from tests.test_gpu_ops import TWIN_CASES
    return case in TWIN_CASES


def case_id(entry):
    c, compute, din, dout = entry
    dt = {F32: "f", BF: "b"}
    return "%s_%s%s_c%d-%d_k%ds%d_%s_u%d_%s_b%d_%dx%d" % ((compute, dt[din], dt[dout]) + c[:4] + c[5:])


_COMPUTE_CODE = {"f32": 0, "bf16": 1, "bf16s": 1, "f32x3": 2}


def kernel_names(lib, entry, act=None):
    """(forward, backward-data, backward-weight) kernel names of an entry, as munit_amd.ops plans the three passes (the
    activation is fused into the forward only).  act: override the case's activation."""
    from munit_amd._lib import ACT, PAD, ConvDesc
    (cin, cout, k, stride, pad, pt, ups, a, b, h, w), compute, din, dout = entry
    a = a if act is None else act
    names = []
    for p in range(3):
        d = ConvDesc(b, h, w, cin, cout, k, k, stride, pad, PAD[pt], int(ups), ACT[a if p == 0 else "none"], LRELU_SLOPE,
                     _COMPUTE_CODE[compute], int(din == BF), int(dout == BF))
        names.append(lib.munit_conv2d_kernel_name(ctypes.byref(d), p).decode())
    return tuple(names)


def dgrad_rounding_model(dgrad_name, dx_bf16, has_add):
    """"one" or "two" roundings of a bf16 dx, from the backward-data kernel name: the forms that write the padded-domain
    gradient as bf16 and fold it afterwards round twice.  A `direct` form (1x1, no padding) writes dx itself, but an `add`
    operand sends it through the same fold kernel (munit_conv2d_kernel_name reports the name of the call without `add`), so
    with `add` it rounds twice as well.  An fp32 dx is never rounded."""
    if not dx_bf16:
        return "one"
    if "fold_kernel<bf16_t>" in dgrad_name or (has_add and dgrad_name.endswith(" direct")):
        return "two"
    return "one"


def dgrad_takes_add(dgrad_name, dx_bf16):
    """The folded gathers (LDS-patch fold, folded gather) refuse `add` with a bf16 dx (include/munit_hip.h: `add` exists for
    the fp32 ResBlock layers; the entry point returns an error, which the exact test asserts)."""
    return not (dx_bf16 and ("LDS-patch fold" in dgrad_name or "folded gather" in dgrad_name))


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
def _out_hw(case):
    cin, cout, k, stride, pad, pt, ups, act, B, H, W = case
    return ((H << ups) + 2 * pad - k) // stride + 1, ((W << ups) + 2 * pad - k) // stride + 1


def exact_inputs(entry):
    """Lattice operands of the exact regime at the case's own shape (the reference batch of a twin case is half of it)."""
    case = entry[0]
    cin, cout, k, stride, pad, pt, ups, act, B, H, W = case
    n = B // 2 if twin(case) else B
    ho, wo = _out_hw(case)
    t3 = (-1, 0, 1)
    return dict(x=lattice((n, cin, H, W), 1, t3, 0.25), w=4 * lattice((cout, cin, k, k), 2, t3), b=4 * lattice((cout,), 3, t3),
                dy=4 * lattice((n, cout, ho, wo), 4, t3, 0.25), add=16 * lattice((n, cin, H, W), 5, t3),
                dw0=lattice((cout, cin, k, k), 6, range(-8, 9)), db0=lattice((cout,), 7, range(-8, 9)))


def _var(a):
    return a * (a + 1) / 3.0       # variance of the uniform lattice {-a..a}


def _amp(k_terms, var_other, sigma=600.0, cap=15):
    for a in range(1, cap + 1):
        if k_terms * var_other * _var(a) >= sigma * sigma:
            return a
    return cap


def rounding_amplitudes(case):
    """(ax, aw, ady): dense lattices {-a..a}; x as the issue suggests ({-4..4}), w and dy the smallest amplitudes that give the
    output and dx a standard deviation of about 600 (from the contraction lengths), so that most values lie above 256 where
    the bf16 grid is coarser than the integers.  Every partial sum stays below 6400 * 4 * 15 < 2^24."""
    cin, cout, k, stride, pad, pt, ups, act, B, H, W = case
    ax = 4
    aw = _amp(cin * k * k, _var(ax))
    ady = _amp(cout * k * k * (4 if ups else 1) // (stride * stride), _var(aw))
    return ax, aw, ady


def rounding_inputs(entry):
    case = entry[0]
    cin, cout, k, stride, pad, pt, ups, act, B, H, W = case
    ho, wo = _out_hw(case)
    ax, aw, ady = rounding_amplitudes(case)
    return dict(x=lattice((B, cin, H, W), 11, range(-ax, ax + 1)), w=lattice((cout, cin, k, k), 12, range(-aw, aw + 1)),
                b=lattice((cout,), 13, range(-3, 4)) / 2, dy=lattice((B, cout, ho, wo), 14, range(-ady, ady + 1)),
                add=lattice((B, cin, H, W), 15, range(-255, 256)))


# ------------------------------------------------------------------------------------------------------------------------
# fp64 reference
# ------------------------------------------------------------------------------------------------------------------------
def lrelu_f32(v):
    """The reference of a fused LeakyReLU: float32(v) * float32(0.2) on the negative side, in fp32."""
    v = v.float()
    return torch.where(v > 0, v, v * torch.tensor(LRELU_SLOPE, dtype=torch.float32))


def conv_reference(case, x, w, b, dy, act=None):
    """Exact reference of the three passes on the oracle's own graph.  Returns a dict of fp64 tensors:
    pre (bias added, before the activation), g (the gradient at pre: dy through a ReLU's mask; dy itself otherwise -- a
    LeakyReLU's backward is checked apart, its dy * 0.2 leaves the lattice), gpad (gradient w.r.t. the padded, up-sampled
    input), dx, dw, db, and `fold`: the adjoint of pad / upsample as a function of a padded-domain gradient."""
    cin, cout, k, stride, pad, pt, ups, a, B, H, W = case
    a = a if act is None else act
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    xp = O.pad2d(O.upsample2(xr) if ups else xr, pad, pt)
    pre = F.conv2d(xp, wr, br, stride=stride)
    g = dy * (pre.detach() > 0) if a == "relu" else dy
    gpad, dw, db = torch.autograd.grad(pre, [xp, wr, br], g, retain_graph=True)

    def fold(gp):
        return torch.autograd.grad(xp, xr, gp, retain_graph=True)[0] if xp is not xr else gp

    return dict(pre=pre.detach(), g=g, gpad=gpad, dx=fold(gpad), dw=dw, db=db, fold=fold)


def activated(pre, act, out_dtype):
    """Expected forward output in its own dtype: bias, then activation, then ONE rounding."""
    if act == "lrelu":
        y = lrelu_f32(pre)
    elif act == "relu":
        y = pre.clamp_min(0)
    else:
        assert act == "none", act
        y = pre
    return rne_bf16(y) if out_dtype == BF else y.float()


def one_rounding(exact, add=None):
    return rne_bf16(exact if add is None else exact + add)


def two_rounding(ref, add=None):
    s = ref["fold"](rne_bf16(ref["gpad"]).double())
    return rne_bf16(s if add is None else s + add)


def expected_dx(ref, model, dx_dtype, add=None):
    if dx_dtype != BF:
        return (ref["dx"] if add is None else ref["dx"] + add).float()
    return two_rounding(ref, add) if model == "two" else one_rounding(ref["dx"], add)


def integers_below_2_24(t):
    return bool((t == t.round()).all()) and float(t.abs().max()) < 2.0 ** 24


def exact_regime_conditions(entry, inp, ref):
    """{name: bool}: every value of the exact regime's reference is on the bf16 grid (inputs, the pre-activation output, the
    padded-domain gradient, dx with and without `add`) and the fp32 weight / bias gradients are integers below 2^24, with
    and without the accumulation buffers."""
    add = inp["add"]
    c = {n: bool(exactly_bf16(inp[n]).all()) for n in ("x", "w", "b", "dy", "add")}
    c.update(pre=bool(exactly_bf16(ref["pre"]).all()), gpad=bool(exactly_bf16(ref["gpad"]).all()),
             dx=bool(exactly_bf16(ref["dx"]).all()), dx_add=bool(exactly_bf16(ref["dx"] + add).all()),
             dw=integers_below_2_24(2 * ref["dw"].abs() + inp["dw0"].abs()), db=integers_below_2_24(2 * ref["db"].abs() + inp["db0"].abs()))
    return c


# ------------------------------------------------------------------------------------------------------------------------
# part d: kernels whose bf16 output is not exact (norms)
# ------------------------------------------------------------------------------------------------------------------------
NORM_KINDS = ("in", "in_res", "adain_relu", "ln_relu")
NORM_SHAPES = ((2, 64, 12, 10), (2, 256, 33, 17))
FWD_TOL, BWD_TOL = 2e-5, 1e-4          # tests/test_gpu_ops.py: the fp32 bounds of a forward / backward pass
# the tanh image head read from a bf16 tensor (fp32 image out): the suite's case and the ragged one of CONV_CASES
HEAD_CASES = [((64, 3, 7, 1, 3, "reflect", 0, "tanh", 2, 16, 12), "bf16s", BF, F32),
              ((64, 3, 7, 1, 3, "reflect", 0, "tanh", 1, 9, 37), "bf16s", BF, F32)]


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def norm_inputs(kind, shape):
    """bf16-valued fp64 inputs of one norm case (as tests/test_gpu_bf16s.py::test_norms_bf16_storage draws them)."""
    B, C, H, W = shape
    q = lambda t: rne_bf16(t).double()
    d = dict(x=q(rnd(shape, 7) * 2 + 0.5), dy=q(rnd(shape, 12)))
    if kind == "in_res":
        d["res"] = q(rnd(shape, 8))
    elif kind == "adain_relu":
        d["params"] = rnd((B, 2 * C), 9).float().double()
    elif kind == "ln_relu":
        d["gamma"], d["beta"] = (rnd((C,), 10).abs() + 0.1).float().double(), rnd((C,), 11, 0.1).float().double()
    return d


def norm_pre(kind, d, leaves):
    """fp64 pre-activation of a norm case on the leaves `leaves` (dict of tensors requiring grad)."""
    C = d["x"].shape[1]
    if kind == "in":
        return O.instance_norm(leaves["x"])
    if kind == "in_res":
        return O.instance_norm(leaves["x"]) + d["res"]
    if kind == "adain_relu":
        return O.adain(leaves["x"], leaves["params"][:, C:], leaves["params"][:, :C])
    return O.munit_layer_norm(leaves["x"], leaves["gamma"], leaves["beta"])


def near_kink(pre, tol):
    """Elements of a ReLU's pre-activation within tol * max of zero: the branch the device takes there is not determined."""
    return pre.abs() <= tol * pre.abs().max()


def rounding_check(got, ref, tol, keep=None):
    """Per-element criterion of a bf16 output: |got - ref| <= ulp_bf16(ref) / 2 + tol * max|ref|, and the signed mean of
    (got - ref) / ulp over the non-zero reference elements, plain (rounding down gives about -0.5) and with the sign of the
    reference taken out (truncation gives about -0.5; round-to-nearest about 0 in both).  Returns (worst excess over the
    bound, signed mean, signed mean towards zero, elements checked)."""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    keep = torch.ones_like(ref, dtype=torch.bool) if keep is None else keep
    ulp = ulp_bf16(ref)
    excess = ((got - ref).abs() - (ulp / 2 + tol * ref.abs().max()))[keep]
    nz = keep & (ref != 0)
    e = ((got - ref) / ulp)[nz]
    return float(excess.max()), float(e.mean()), float((e * torch.sign(ref)[nz]).mean()), int(keep.sum())
