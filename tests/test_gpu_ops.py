"""GPU: every HIP kernel (through the C ABI via munit_amd.ops) against the fp64 CPU oracle
on the same seeded inputs.  Tolerances (normalised max error = max|d| / max|ref|, SURVEY.md
section 8c): forward 1e-4 (we assert the tighter 2e-5 the fp32 MFMA chain actually gives),
gradients 1e-2 (asserted 1e-4)."""
import pytest
import torch

from oracle import munit_oracle as O
from tests.parity import nerr

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-5
BWD_TOL = 1e-4


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale)


CONV_CASES = [
    # cin, cout, k, stride, pad, pad_type, ups, act, B, H, W
    (3, 64, 7, 1, 3, "reflect", 0, "relu", 2, 20, 24),      # first encoder layer (K=147, unaligned)
    (64, 128, 4, 2, 1, "reflect", 0, "relu", 2, 16, 16),    # down-sampling
    (128, 256, 4, 2, 1, "reflect", 0, "none", 1, 12, 20),
    (256, 256, 3, 1, 1, "reflect", 0, "none", 2, 8, 8),     # resblock conv
    (256, 128, 5, 1, 2, "reflect", 1, "none", 2, 6, 8),     # upsample x2 + 5x5
    (128, 64, 5, 1, 2, "reflect", 1, "none", 1, 9, 7),
    (256, 128, 5, 1, 2, "reflect", 1, "relu", 2, 12, 10),   # large enough for the box-sum backward-data (H, W >= 8)
    (128, 64, 5, 1, 2, "reflect", 1, "none", 1, 8, 19),
    (64, 3, 7, 1, 3, "reflect", 0, "tanh", 2, 16, 12),      # image head (N=3)
    (3, 64, 4, 2, 1, "reflect", 0, "lrelu", 2, 16, 16),     # D first layer (K=48)
    (256, 512, 4, 2, 1, "reflect", 0, "lrelu", 2, 4, 4),    # D last layer
    (512, 1, 1, 1, 0, "zero", 0, "none", 2, 4, 4),          # D head
    (256, 16, 1, 1, 0, "zero", 0, "none", 3, 1, 1),         # style head on 1x1
    (32, 48, 3, 1, 1, "zero", 0, "relu", 2, 9, 11),         # zero pad, odd sizes, odd channels
    (36, 20, 4, 2, 1, "reflect", 0, "none", 2, 9, 11),      # unaligned Cin, odd sizes with stride 2
    (64, 64, 4, 2, 1, "reflect", 0, "none", 2, 2, 2),       # tiniest reflect case (2x2 -> 1x1)
    # stride-1 reflect layers whose backward-data folds <= 2 padded positions per axis: direct-to-LDS tiles + LDS patch
    (256, 256, 3, 1, 1, "reflect", 0, "none", 2, 20, 24),   # several M-tiles, rows that straddle tile boundaries
    (64, 96, 3, 1, 1, "reflect", 0, "relu", 1, 4, 5),       # smallest extent with at most one mirror per row (H = 4)
    (64, 64, 5, 1, 2, "reflect", 0, "none", 2, 7, 9),       # pad 2: two mirrored rows per edge
    (32, 64, 7, 1, 3, "reflect", 0, "none", 1, 10, 13),     # pad 3
    (64, 64, 3, 1, 1, "reflect", 0, "none", 1, 3, 3),       # H = 3: row 1 mirrors both ways -> register-path fallback
    # 3-channel head on the 4x4x1 MFMA kernel: ragged tile edges, two 64-channel passes, zero padding
    (64, 3, 7, 1, 3, "reflect", 0, "tanh", 1, 9, 37),
    (128, 3, 7, 1, 3, "zero", 0, "none", 2, 8, 20),
    # three INPUT channels on the direct-to-LDS 4-channel-tap path: ragged sizes, stride 2, 5x5 (K-tile tail of zero taps)
    (3, 64, 7, 1, 3, "reflect", 0, "relu", 1, 13, 37),
    (3, 128, 4, 2, 1, "reflect", 0, "lrelu", 2, 10, 14),
    (3, 32, 5, 1, 2, "zero", 0, "none", 2, 9, 11),
    (32, 3, 5, 1, 2, "reflect", 0, "none", 2, 9, 11),        # 3 output channels, not 7x7: backward-data on that path too
    # Winograd F(2x2, 3x3) path (conv_wino.hip): partial 8x8-tile blocks, zero and reflect padding, fused activations,
    # K = 9 chunks of 8, two N-blocks, the smallest extent, and one block-aligned trunk-like shape
    (64, 128, 3, 1, 1, "zero", 0, "lrelu", 2, 20, 12),
    (72, 64, 3, 1, 1, "reflect", 0, "relu", 1, 18, 34),
    (8, 64, 3, 1, 1, "reflect", 0, "none", 3, 2, 2),
    (128, 256, 3, 1, 1, "reflect", 0, "none", 1, 32, 48),
    (64, 64, 3, 1, 1, "reflect", 0, "none", 1, 2, 2),       # one tile: the backward-weight chunk is 7/8 empty
    (64, 192, 3, 1, 1, "zero", 0, "none", 3, 6, 10),        # 45 tiles: ragged last chunk, zero padding, three N-blocks
    # 4x4 / stride 2 layers as F(3x3, 2x2) over the four input phases: zero padding, ragged 3x3 tiles, a 26x26 output
    (64, 64, 4, 2, 1, "zero", 0, "lrelu", 2, 10, 14),
    (8, 128, 4, 2, 1, "reflect", 0, "none", 1, 52, 52),
    # sub-pixel layers at the extents of the 64x64 step tests: several 8x8-tile blocks per axis in the backward-data
    (256, 128, 5, 1, 2, "reflect", 1, "none", 2, 16, 16),
    (128, 64, 5, 1, 2, "reflect", 1, "none", 1, 32, 32),
    # F(3x3, 2x2) forms that production reaches at the default thresholds and no case above does (tests/test_cpu_dispatch.py
    # lists them; CONV_CASES_TARGETS pins them): the reflect backward-weight FAST loader (config_256.yaml at a 96x96 crop,
    # batch 2), the same loader on one 8-tile chunk (through test_conv_stride2_winograd_on_small_shapes), and the zero-padded
    # forward, backward-data and backward-weight at a real grid size (the discriminator of a zero-padded config_256 at a
    # 384x384 crop, batch 3: fake + real = 6 samples; twin batch, see TWIN_CASES)
    (64, 128, 4, 2, 1, "reflect", 0, "none", 2, 96, 96),
    (64, 128, 4, 2, 1, "reflect", 0, "none", 2, 12, 12),
    (64, 128, 4, 2, 1, "zero", 0, "none", 6, 192, 192),
]

# cases whose second half of the batch repeats the first: the kernels run the full batch, the fp64 reference half of it
# (tests/test_gpu_shapes.py, TWIN_BATCH)
TWIN_CASES = {(64, 128, 4, 2, 1, "zero", 0, "none", 6, 192, 192)}


# the linears of the op tests as (B, K, N, act): test_linear and test_linear_entry_points (the MLP's 4096-wide output)
LINEAR_CASES = [(5, 16, 256, "relu"), (5, 256, 4096, "relu")]

# CONV_CASES entries added to reach a kernel form no other op test runs, with the kernel each pass must take (None: any);
# tests/test_cpu_dispatch.py asserts these names on the CPU
_S2W = " + wino_wgrad_reduce_kernel"
CONV_CASES_TARGETS = {
    (64, 128, 4, 2, 1, "reflect", 0, "none", 2, 96, 96): (None, None, "conv_wino_wgrad_kernel<true, true, false>" + _S2W),
    (64, 128, 4, 2, 1, "zero", 0, "none", 6, 192, 192): ("conv_wino_kernel<1, 1>", "conv_wino_kernel<1, 2>",
                                                         "conv_wino_wgrad_kernel<true, false, false>" + _S2W),
}
# the same under MUNIT_WINO_S2_MIN_BLOCKS=1 (test_conv_stride2_winograd_on_small_shapes)
CONV_CASES_TARGETS_S2_MIN1 = {
    (64, 128, 4, 2, 1, "reflect", 0, "none", 2, 12, 12): ("conv_wino_kernel<0, 1>", None,
                                                         "conv_wino_wgrad_kernel<true, true, false>" + _S2W),
}


def ref_conv(x, w, b, stride, pad, pad_type, ups, act):
    if ups:
        x = O.upsample2(x)
    return O.conv_block(x, w, b, stride, pad, pad_type, None, act)


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "c%d-%d_k%ds%d_%s_u%d_%s" % (c[0], c[1], c[2], c[3], c[5], c[6], c[7]))
def test_conv_fwd_bwd(case):
    from munit_amd import ops
    cin, cout, k, stride, pad, pt, ups, act, B, H, W = case
    twin = case in TWIN_CASES
    nref = B // 2 if twin else B
    x = rnd((nref, cin, H, W), 1)
    w = rnd((cout, cin, k, k), 2, (2.0 / (cin * k * k)) ** 0.5)
    b = rnd((cout,), 3, 0.1)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    yr = ref_conv(xr, wr, br, stride, pad, pt, ups, act)
    dy = rnd(tuple(yr.shape), 4)
    yr.backward(dy)
    gx, gw, gb = xr.grad, wr.grad, br.grad
    if twin:      # the device sums each distinct sample twice into the parameter gradients
        x, dy, yr = torch.cat([x, x]), torch.cat([dy, dy]), torch.cat([yr, yr]).detach()
        gx, gw, gb = torch.cat([gx, gx]), 2 * gw, 2 * gb

    xd = x.float().to(dev()).requires_grad_(True)
    wd = w.float().to(dev()).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bd = b.float().to(dev()).requires_grad_(True)
    y = ops.conv2d(xd, wd, bd, stride, pad, pt, bool(ups), act)
    assert tuple(y.shape) == tuple(yr.shape)
    assert nerr(y, yr) <= FWD_TOL, nerr(y, yr)
    y.backward(dy.float().to(dev()))
    if twin:
        assert torch.equal(y[B // 2:], y[:B // 2]) and torch.equal(xd.grad[B // 2:], xd.grad[:B // 2]), "twin samples differ"
    assert nerr(xd.grad, gx) <= BWD_TOL, ("dx", nerr(xd.grad, gx))
    assert nerr(wd.grad, gw) <= BWD_TOL, ("dw", nerr(wd.grad, gw))
    assert nerr(bd.grad, gb) <= BWD_TOL, ("db", nerr(bd.grad, gb))


def test_conv_stride2_winograd_on_small_shapes():
    """The F(3x3, 2x2) kernel of the 4x4 / stride 2 layers only takes shapes that fill the chip (no split over K); the
    library reads MUNIT_WINO_S2_MIN_BLOCKS once per process, so a child process with the threshold at 1 pushes the small
    stride-2 cases of CONV_CASES (ragged 3x3 tiles, zero padding, one-block grids) through it."""
    import os, subprocess, sys
    env = dict(os.environ, MUNIT_WINO_S2_MIN_BLOCKS="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_ops.py"), "-q", "-x", "-m", "gpu",
                        "-k", "test_conv_fwd_bwd and k4s2", "-p", "no:cacheprovider"], env=env, cwd=root, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-2000:]


def test_conv_wgrad_accumulates_into_buffer():
    """The trainer path: backward-weight adds into a preallocated buffer (beta = 1)."""
    from munit_amd import ops
    x = rnd((2, 64, 8, 8), 1).float().to(dev())
    w = rnd((64, 64, 3, 3), 2, 0.05).float().to(dev()).contiguous(memory_format=torch.channels_last)
    b = rnd((64,), 3).float().to(dev())
    dy = rnd((2, 64, 8, 8), 4).float().to(dev())
    dw0, db0 = ops.conv2d_wgrad_raw(x, dy, w.shape, 1, 1, "reflect", False)
    dw, db = dw0.clone(), db0.clone()
    ops.conv2d_wgrad_raw(x, dy, w.shape, 1, 1, "reflect", False, dw=dw, db=db, beta=1.0)
    assert nerr(dw, 2 * dw0) <= 1e-6 and nerr(db, 2 * db0) <= 1e-6


def test_linear():
    from munit_amd import ops
    x = rnd((5, 16), 1)
    w = rnd((256, 16), 2, 0.2)
    b = rnd((256,), 3, 0.1)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    yr = torch.clamp_min(torch.nn.functional.linear(xr, wr, br), 0)
    dy = rnd(tuple(yr.shape), 4)
    yr.backward(dy)
    xd, wd, bd = (t.float().to(dev()).requires_grad_(True) for t in (x, w, b))
    y = ops.linear(xd, wd, bd, "relu")
    assert nerr(y, yr) <= FWD_TOL
    y.backward(dy.float().to(dev()))
    assert nerr(xd.grad, xr.grad) <= BWD_TOL
    assert nerr(wd.grad, wr.grad) <= BWD_TOL
    assert nerr(bd.grad, br.grad) <= BWD_TOL


@pytest.mark.parametrize("shape", [(2, 64, 16, 16), (3, 256, 8, 8), (1, 128, 31, 17), (2, 48, 5, 7)])
@pytest.mark.parametrize("mode", ["in", "in_relu", "adain_relu", "adain_res", "in_lrelu", "adain_tanh", "adain_lrelu"])
def test_instance_norm(shape, mode):
    from munit_amd import ops
    B, C, H, W = shape
    x = rnd(shape, 1, 1.7) + 0.4
    res = rnd(shape, 5)
    params = rnd((B, 4 * C), 2) + 0.5
    w_off, b_off = 3 * C, C
    xr = x.clone().requires_grad_(True)
    pr = params.clone().requires_grad_(True)
    rr = res.clone().requires_grad_(True)
    if mode.startswith("adain"):
        yr = O.adain(xr, pr[:, w_off:w_off + C], pr[:, b_off:b_off + C])
    else:
        yr = O.instance_norm(xr)
    if mode.endswith("lrelu"):        # networks.py:672 nn.LeakyReLU(0.2) behind a norm (networks.py:695-701): fused into the norm kernels
        yr = torch.nn.functional.leaky_relu(yr, 0.2)
    elif mode.endswith("tanh"):
        yr = torch.tanh(yr)
    elif mode.endswith("relu"):
        yr = torch.clamp_min(yr, 0)
    if mode.endswith("res"):
        yr = yr + rr
    dy = rnd(shape, 4)
    yr.backward(dy)

    xd = x.float().to(dev()).requires_grad_(True)
    pd = params.float().to(dev()).requires_grad_(True)
    rd = res.float().to(dev()).requires_grad_(True)
    relu = "lrelu" if mode.endswith("lrelu") else "tanh" if mode.endswith("tanh") else mode.endswith("relu")
    residual = rd if mode.endswith("res") else None
    if mode.startswith("adain"):
        y = ops.adain(xd, pd, w_off, b_off, relu, residual)
    else:
        y = ops.instance_norm(xd, relu, residual)
    assert nerr(y, yr) <= FWD_TOL, nerr(y, yr)
    y.backward(dy.float().to(dev()))
    assert nerr(xd.grad, xr.grad) <= BWD_TOL, nerr(xd.grad, xr.grad)
    if mode.startswith("adain"):
        assert nerr(pd.grad, pr.grad) <= BWD_TOL, nerr(pd.grad, pr.grad)
    if mode.endswith("res"):
        assert nerr(rd.grad, rr.grad) <= 1e-6


@pytest.mark.parametrize("shape", [(2, 128, 16, 16), (1, 64, 33, 9), (3, 64, 8, 8)])
@pytest.mark.parametrize("relu", [False, True, "lrelu", "tanh"])
def test_layer_norm(shape, relu):
    from munit_amd import ops
    B, C, H, W = shape
    x = rnd(shape, 1, 2.0) - 0.7
    g = torch.rand(C, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    bt = rnd((C,), 3, 0.3)
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, g, bt))
    yr = O.munit_layer_norm(xr, gr, br)
    if relu == "lrelu":
        yr = torch.nn.functional.leaky_relu(yr, 0.2)
    elif relu == "tanh":
        yr = torch.tanh(yr)
    elif relu:
        yr = torch.clamp_min(yr, 0)
    dy = rnd(shape, 4)
    yr.backward(dy)
    xd, gd, bd = (t.float().to(dev()).requires_grad_(True) for t in (x, g, bt))
    y = ops.layer_norm(xd, gd, bd, relu)
    assert nerr(y, yr) <= FWD_TOL, nerr(y, yr)
    y.backward(dy.float().to(dev()))
    assert nerr(xd.grad, xr.grad) <= BWD_TOL, nerr(xd.grad, xr.grad)
    assert nerr(gd.grad, gr.grad) <= BWD_TOL
    assert nerr(bd.grad, br.grad) <= BWD_TOL


@pytest.mark.parametrize("shape", [(2, 3, 16, 16), (1, 3, 9, 13), (2, 3, 2, 2), (1, 5, 1, 4)])
def test_avgpool(shape):
    from munit_amd import ops
    x = rnd(shape, 1)
    xr = x.clone().requires_grad_(True)
    yr = O.avgpool_3s2(xr)
    dy = rnd(tuple(yr.shape), 2)
    yr.backward(dy)
    xd = x.float().to(dev()).requires_grad_(True)
    y = ops.avgpool3s2(xd)
    assert tuple(y.shape) == tuple(yr.shape)
    assert nerr(y, yr) <= 1e-6
    y.backward(dy.float().to(dev()))
    assert nerr(xd.grad, xr.grad) <= 1e-6


def test_global_avgpool():
    from munit_amd import ops
    x = rnd((3, 256, 16, 16), 1)
    xr = x.clone().requires_grad_(True)
    yr = xr.mean(dim=(2, 3), keepdim=True)
    dy = rnd(tuple(yr.shape), 2)
    yr.backward(dy)
    xd = x.float().to(dev()).requires_grad_(True)
    y = ops.global_avgpool(xd)
    assert nerr(y, yr) <= 1e-6
    y.backward(dy.float().to(dev()))
    assert nerr(xd.grad, xr.grad) <= 1e-6


@pytest.mark.parametrize("masked", [False, True])
def test_l1_mean(masked):
    from munit_amd import ops
    a, b = rnd((2, 3, 17, 19), 1), rnd((2, 3, 17, 19), 2)
    m = (torch.rand(2, 1, 17, 19, generator=torch.Generator().manual_seed(3)) > 0.5).double() if masked else None
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    lr = O.l1_masked(ar, br, m) if masked else O.l1(ar, br)
    (lr * 12.0).backward()
    ad, bd = (t.float().to(dev()).requires_grad_(True) for t in (a, b))
    md = m.float().to(dev()) if masked else None
    l = ops.l1_mean(ad, bd, md)
    assert abs(float(l) - float(lr)) <= 1e-6 * abs(float(lr))
    torch.autograd.backward([l], [torch.tensor(12.0, device=dev())])
    assert nerr(ad.grad, ar.grad) <= 1e-6 and nerr(bd.grad, br.grad) <= 1e-6


def test_l1_mean_content_and_style_shapes():
    from munit_amd import ops
    for shape in [(2, 256, 8, 8), (3, 16, 1, 1)]:
        a, b = rnd(shape, 1), rnd(shape, 2)
        l = ops.l1_mean(a.float().to(dev()), b.float().to(dev()))
        assert abs(float(l) - float(O.l1(a, b))) <= 1e-6 * float(O.l1(a, b))


def test_mse_const_and_scalar_sum():
    from munit_amd import ops
    xs = [rnd((2, 1, 4, 4), 1), rnd((2, 1, 2, 2), 2), rnd((2, 1, 1, 1), 3)]
    xr = [t.clone().requires_grad_(True) for t in xs]
    lr = sum(torch.mean((t - 1) ** 2) for t in xr)
    (3.0 * lr).backward()
    xd = [t.float().to(dev()).requires_grad_(True) for t in xs]
    l = ops.scalar_sum([ops.mse_const(t, 1.0) for t in xd])
    assert abs(float(l) - float(lr)) <= 1e-6 * float(lr)
    torch.autograd.backward([l], [torch.tensor(3.0, device=dev())])
    for d, r in zip(xd, xr):
        assert nerr(d.grad, r.grad) <= 1e-6


def test_adam_matches_torch_semantics():
    from munit_amd import ops
    n = 1003
    p, g = rnd((n,), 1), rnd((n,), 2, 0.01)
    m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    pd, gd = p.float().to(dev()).contiguous(), g.float().to(dev()).contiguous()
    md, vd = torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    pr = p.clone()
    for step in (1, 2, 3):
        O.adam_update(pr, g, m, v, step, 1e-4, 0.5, 0.999, 1e-8, 1e-4)
        ops.adam_step(pd, gd, md, vd, 1e-4, 0.5, 0.999, 1e-8, 1e-4, step)
    # p is O(1) in fp32: each of the 3 updates rounds to ~6e-8 * |p|
    ep, em, ev = float((pd.double().cpu() - pr).abs().max()), nerr(md, m), nerr(vd, v)
    assert ep <= 2e-6 and em <= 1e-6 and ev <= 1e-6, (ep, em, ev)


def test_extraadam_kernel_matches_oracle():
    from munit_amd import ops
    n = 777
    p0 = rnd((n,), 1)
    gs = [rnd((n,), 10 + k, 0.3) for k in range(5)]
    pr = [p0.clone()]
    st = O.ExtraAdamState(pr, 1e-3, (0.5, 0.999), 1e-4)
    pd = p0.float().to(dev()).contiguous()
    md, vd, sd = torch.zeros(n, device=dev()), torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    has_copy = False
    for k, mode in enumerate(["extrapolation", "step", "extrapolation", "extrapolation", "step"]):
        getattr(st, mode)([gs[k]])
        code = 2 if mode == "step" else (1 if has_copy else 0)
        has_copy = mode != "step"
        ops.extraadam_step(pd, gs[k].float().to(dev()).contiguous(), md, vd, sd, 1e-3, 0.5, 0.999, 1e-8, 1e-4, k + 1, code)
        assert float((pd.double().cpu() - pr[0]).abs().max()) <= 2e-6, (k, mode)
    assert nerr(md, st.m[0]) <= 1e-6 and nerr(vd, st.v[0]) <= 1e-6


def test_cpu_tensor_is_refused():
    """No CPU fallback: the product path must fail loudly off-device."""
    from munit_amd import ops
    with pytest.raises(RuntimeError):
        ops.conv2d(torch.zeros(1, 3, 8, 8), torch.zeros(4, 3, 3, 3), None, 1, 1, "reflect")


def test_linear_entry_points():
    """munit_linear_fwd / munit_linear_bwd (the named C entry points of nn.Linear) straight through ctypes."""
    import ctypes
    from munit_amd import _lib
    lib = _lib.load()
    B, K, N = 5, 256, 4096
    x, w, b, dy = rnd((B, K), 1), rnd((N, K), 2, 0.05), rnd((N,), 3, 0.1), rnd((B, N), 4)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    yr = torch.relu(xr @ wr.t() + br)
    yr.backward(dy)
    d = dev()
    xd, wd, bd = (t.float().to(d).contiguous() for t in (x, w, b))
    y = torch.empty(B, N, device=d)
    nws = lib.munit_linear_workspace_bytes(B, K, N)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=d)
    vp = ctypes.c_void_p
    st = vp(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.munit_linear_fwd(vp(xd.data_ptr()), vp(wd.data_ptr()), vp(bd.data_ptr()), vp(y.data_ptr()), B, K, N,
                                    _lib.ACT["relu"], ctypes.c_float(0.2), vp(ws.data_ptr()), ctypes.c_size_t(nws), st), "linear_fwd")
    assert nerr(y, yr) <= FWD_TOL
    g = (dy * (yr > 0)).float().to(d).contiguous()      # gradient at the pre-activation output
    dx, dw, db = torch.empty_like(xd), torch.empty_like(wd), torch.empty_like(bd)
    _lib.check(lib.munit_linear_bwd(vp(xd.data_ptr()), vp(wd.data_ptr()), vp(g.data_ptr()), vp(dx.data_ptr()),
                                    vp(dw.data_ptr()), vp(db.data_ptr()), B, K, N, ctypes.c_float(0.0), vp(ws.data_ptr()),
                                    ctypes.c_size_t(nws), st), "linear_bwd")
    assert nerr(dx, xr.grad) <= BWD_TOL and nerr(dw, wr.grad) <= BWD_TOL and nerr(db, br.grad) <= BWD_TOL


# ------------------------------------------------------------------------------------------------------------------------
# contract of the raw C entry points (tests/conv_contract.py): guard bands, NaN poison, full writes, determinism, prepared
# images, `add`, `beta`, db == NULL and the workspace size -- on every op case, the BASELINE-shape layers and the linears
# ------------------------------------------------------------------------------------------------------------------------
def _contract_cases():
    from tests.test_gpu_shapes import LAYERS
    return list(CONV_CASES) + [(ci, co, k, s, p, "reflect", u, a, b, h, w) for _, ci, co, k, s, p, u, a, b, h, w in LAYERS]


def _bf16s_form(c):
    """The kinds of layer the bf16-storage trainer runs on bf16 tensors: 64-multiples of channels on both sides, reflect
    padding, 4x4 / stride 2 down-sampling, 3x3 trunk, nearest x2 + 5x5 up-sampling."""
    cin, cout, k, stride, pad, pt, ups, act, B, H, W = c
    kind = (k, stride, pad, ups) in ((4, 2, 1, 0), (3, 1, 1, 0), (5, 1, 2, 1))
    return cin % 64 == 0 and cout % 64 == 0 and pt == "reflect" and kind


_CID = lambda c: "c%d-%d_k%ds%d_%s_u%d_%s_b%d_%dx%d" % (c[0], c[1], c[2], c[3], c[5], c[6], c[7], c[8], c[9], c[10])


@pytest.mark.parametrize("case", _contract_cases(), ids=_CID)
def test_conv_entry_point_contract(case):
    from tests.conv_contract import check_conv_case
    check_conv_case(case)


@pytest.mark.parametrize("case", [c for c in _contract_cases() if _bf16s_form(c)], ids=_CID)
def test_conv_entry_point_contract_bf16_storage(case):
    from tests.conv_contract import check_conv_case
    check_conv_case(case, bf16=True)


@pytest.mark.parametrize("case", LINEAR_CASES, ids=lambda c: "b%d_%d-%d_%s" % c)
def test_linear_entry_point_contract(case):
    from tests.conv_contract import check_linear
    check_linear(*case)


# ------------------------------------------------------------------------------------------------------------------------
# normalisation at the shapes where the split logic changes regime (tests/test_cpu_norm_regimes.py maps every case to its
# regime and requires each regime production reaches, and each edge it lists, to be run here; every case has a regime of
# its own)
# ------------------------------------------------------------------------------------------------------------------------
NORM_CASES = [
    # kind, dtype, B, C, H, W
    ("in", "f32", 2, 64, 1, 1),             # HW = 1
    ("in", "f32", 2, 16, 8, 8),             # HW = 64: one split
    ("adain", "f32", 3, 12, 127, 1),        # HW = 127: the last one-split extent; C = 12: QB = 3, idle lanes
    ("in", "f32", 2, 4, 16, 8),             # HW = 128: two splits; C = 4: one quad, 256 pixel lanes
    ("adain", "f32", 2, 68, 43, 3),         # HW = 129: a short last split; C = 68: a partial second fold block
    ("adain", "f32", 33, 12, 64, 64),       # B = 33: 62 splits
    ("in", "f32", 1, 64, 64, 64),           # B = 1, HW = 4096: the 64-split cap
    ("adain", "f32", 32, 128, 32, 32),      # B = 32
    ("adain", "f32", 2, 192, 64, 64),       # 3 slices: 64 / 3 -> 21 splits, short last split
    ("in", "f32", 1, 320, 24, 32),          # 5 slices: 12 / 5 -> 2 splits
    ("adain", "f32", 1, 128, 20, 32),       # 2 slices, 5 splits
    ("adain", "f32", 1, 1024, 16, 16),      # the largest C: 16 slices
    ("in", "f32", 1, 1020, 16, 8),          # the largest non-sliced C: 255 quads
    ("in", "f32", 1, 16, 64, 64),           # non-sliced at the cap
    ("adain", "f32", 1, 16, 2, 64),
    ("in", "f32", 1, 16, 5, 64),
    ("adain", "f32", 1, 64, 2, 64),
    ("in", "f32", 1, 64, 5, 64),
    ("adain", "f32", 1, 64, 43, 3),
    ("in", "f32", 1, 64, 107, 3),
    ("adain", "f32", 1, 128, 87, 3),
    ("in", "f32", 1, 128, 2, 64),
    ("ln", "f32", 2, 4, 1, 2),              # HW * C = 8
    ("ln", "f32", 9, 12, 64, 64),           # 9 x 64 = 576 partial rows in ln_bwd_param_kernel
    ("ln", "f32", 2, 1020, 4, 4),           # the largest C of ln_bwd_stats: 255 quads
    ("ln", "f32", 1, 16, 64, 64),
    ("ln", "f32", 1, 16, 2, 64),
    ("ln", "f32", 1, 16, 5, 64),
    ("ln", "f32", 1, 16, 97, 2),
    ("ln", "f32", 1, 16, 107, 3),
    ("adain", "bf16", 32, 256, 64, 64),     # bf16 storage: config #3's trunk, 4 slices x 16 splits
    ("in", "bf16", 33, 12, 64, 64),         # bf16, non-sliced, 62 splits
    ("in", "bf16", 1, 64, 64, 64),          # bf16, sliced at the cap
    ("ln", "bf16", 1, 12, 64, 64),
    ("ln", "bf16", 1, 16, 64, 64),
]
_NID = lambda c: "%s_%s_b%d_c%d_%dx%d" % c
ACT_CODES = ("none", "relu", "lrelu", "tanh")
BF16_OUT, BF16_DX = 8e-3, 1.2e-2          # tests/test_gpu_bf16s.py: bf16 outputs / dx


def _norm_setup(case, i):
    """Activation code and residual of case i (cycled over NORM_CASES); ReLU / LeakyReLU never with a residual, so the
    reference can take the device's branches from the sign of y."""
    act = ACT_CODES[i % 4]
    return act, act in ("none", "tanh") and case[0] != "ln" and (i // 4) % 2 == 0


def _pin(pre, y_dev, act):
    """The reference's ReLU / LeakyReLU on the branches the device took (tests/test_gpu_shapes.py, pinned_relu)."""
    from tests.test_gpu_shapes import KINK_FRAC, KINK_NOISE
    mask = (y_dev.detach().float() > 0).cpu()
    dis = (pre.detach() > 0) != mask
    n = int(dis.sum())
    if n:
        worst = float(pre.detach()[dis].abs().max()) / float(pre.detach().abs().max())
        assert worst <= KINK_NOISE and n <= KINK_FRAC * pre.numel(), (n, worst)
    if act == "relu":
        return torch.where(mask, pre, torch.zeros_like(pre))
    return torch.where(mask, pre, pre * 0.2)


def _act_ref(pre, y_dev, act):
    if act in ("relu", "lrelu"):
        return _pin(pre, y_dev, act)
    return torch.tanh(pre) if act == "tanh" else pre


def run_norm(kind, dt, shape, act, residual, x=None, seed=1):
    """Device norm (ops) and its fp64 reference on the same (fp32- or bf16-rounded) values.  Returns
    [(name, device tensor, reference, tolerance)], including the statistics, compared directly."""
    from munit_amd import ops
    B, C, H, W = shape
    q = (lambda t: t.float().bfloat16().double()) if dt == "bf16" else (lambda t: t.float().double())
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32
    fwd_tol, dx_tol = (BF16_OUT, BF16_DX) if dt == "bf16" else (FWD_TOL, BWD_TOL)
    x = q(rnd(shape, seed, 1.7) + 0.4 if x is None else x)
    dy = q(rnd(shape, seed + 3))
    res = q(rnd(shape, seed + 4))
    cl = lambda t: t.to(tdt).to(dev()).contiguous(memory_format=torch.channels_last)
    xr, xd = x.clone().requires_grad_(True), cl(x).requires_grad_(True)
    out, extra = [], []
    prev = ops.get_compute()
    ops.set_compute("bf16s" if dt == "bf16" else "f32")
    try:
        if kind == "ln":
            g = torch.rand(C, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64) + 0.2
            bt = rnd((C,), seed + 2, 0.3)
            gr, br = g.clone().requires_grad_(True), bt.clone().requires_grad_(True)
            gd, bd = g.float().to(dev()).requires_grad_(True), bt.float().to(dev()).requires_grad_(True)
            y = ops.layer_norm(xd, gd, bd, act)
            pre = O.munit_layer_norm(xr, gr, br)
            flat = x.reshape(B, -1)
            st_ref = torch.stack([flat.mean(1), flat.std(1, unbiased=True)], 1)
            extra = [("dgamma", gd, gr), ("dbeta", bd, br)]
            stats_of = lambda: y.grad_fn.saved_tensors[1]
        else:
            rd = cl(res) if residual else None
            if kind == "adain":
                params = rnd((B, 4 * C), seed + 2) + 0.5
                w_off, b_off = 3 * C, C
                pr, pd = params.clone().requires_grad_(True), params.float().to(dev()).requires_grad_(True)
                y = ops.adain(xd, pd, w_off, b_off, act, rd)
                pre = O.adain(xr, pr[:, w_off:w_off + C], pr[:, b_off:b_off + C])
                extra = [("d_adain", pd, pr)]
            else:
                y = ops.instance_norm(xd, act, rd)
                pre = O.instance_norm(xr)
            mu = x.mean(dim=(2, 3))
            var = ((x - mu[:, :, None, None]) ** 2).mean(dim=(2, 3))
            st_ref = torch.stack([mu, 1.0 / torch.sqrt(var + 1e-5)], 2)
            stats_of = lambda: y.grad_fn.saved_tensors[1]
        yr = _act_ref(pre, y, act)
        if residual:
            yr = yr + res
        stats = stats_of()
        out.append(("y", y, yr, fwd_tol))
        out.append(("mean", stats[..., 0], st_ref[..., 0], FWD_TOL))
        out.append(("std" if kind == "ln" else "rstd", stats[..., 1], st_ref[..., 1], FWD_TOL))
        yr.backward(dy)
        y.backward(cl(dy))
    finally:
        ops.set_compute(prev)
    out.append(("dx", xd.grad, xr.grad, dx_tol))
    out += [(n, d.grad, r.grad, BWD_TOL) for n, d, r in extra]
    return out


def _assert_all(results, what):
    errs = {n: nerr(d, r) for n, d, r, _ in results}
    bad = {n: e for (n, d, r, tol), e in zip(results, errs.values()) if not e <= tol}
    assert not bad, (what, bad, errs)


@pytest.mark.parametrize("i", range(len(NORM_CASES)), ids=lambda i: _NID(NORM_CASES[i]))
def test_norm_regime(i):
    kind, dt, B, C, H, W = NORM_CASES[i]
    act, residual = _norm_setup(NORM_CASES[i], i)
    _assert_all(run_norm(kind, dt, (B, C, H, W), act, residual, seed=i + 1), (NORM_CASES[i], act, residual))


@pytest.mark.parametrize("kind", ["in", "adain"])
def test_norm_constant_plane(kind):
    """Variance 0 in every third channel: AdaIN gives its bias there, all gradients finite and equal to the fp64 ones."""
    B, C, H, W = 2, 68, 9, 15
    x = rnd((B, C, H, W), 3, 1.3)
    x[:, ::3] = rnd((B, C, 1, 1), 4)[:, ::3]
    res = run_norm(kind, "f32", (B, C, H, W), "relu" if kind == "adain" else "none", False, x=x)
    for n, d, r, _ in res:
        assert bool(torch.isfinite(d.detach().float()).all()), (kind, n)
    _assert_all(res, kind)


@pytest.mark.parametrize("kind", ["in", "adain", "ln"])
def test_norm_large_mean(kind):
    """Offset 1e3, spread 1e-2 (the fp64 reference runs on the same fp32 values): the pivot keeps the variance free of
    cancellation, so the statistics hold the fp32 bound.  y, dx and the parameter gradients are computed from the fp32
    mean, whose rounding (ulp(1e3) = 6e-5 against a spread of 1e-2) shifts every normalised value of a plane alike: they
    are held to that, eight ulps of the mean in units of the standard deviation."""
    B, C, H, W = 2, 64 if kind != "ln" else 12, 16, 16
    x = (1e3 + rnd((B, C, H, W), 5, 1e-2)).float().double()
    res = run_norm(kind, "f32", (B, C, H, W), "none", False, x=x)
    cond = 8 * 2.0 ** -24 * 1e3 / 1e-2
    _assert_all([(n, d, r, t if n in ("mean", "rstd", "std") else max(t, cond)) for n, d, r, t in res], kind)


@pytest.mark.parametrize("H,W", [(h, w) for h in range(1, 6) for w in range(1, 6)])
def test_avgpool_borders(H, W):
    from munit_amd import ops
    x = rnd((1, 64, H, W), H * 10 + W)
    xr = x.clone().requires_grad_(True)
    yr = O.avgpool_3s2(xr)
    dy = rnd(tuple(yr.shape), 2)
    yr.backward(dy)
    xd = x.float().to(dev()).requires_grad_(True)
    y = ops.avgpool3s2(xd)
    assert tuple(y.shape) == tuple(yr.shape) and nerr(y, yr) <= 1e-6
    y.backward(dy.float().to(dev()))
    assert nerr(xd.grad, xr.grad) <= 1e-6


def test_avgpool_pyramid():
    """The discriminator's input pyramid at batch 8: 256 -> 128 -> 64, three channels."""
    from munit_amd import ops
    x = rnd((8, 3, 256, 256), 9)
    xr = x.clone().requires_grad_(True)
    yr = O.avgpool_3s2(O.avgpool_3s2(xr))
    dy = rnd(tuple(yr.shape), 2)
    yr.backward(dy)
    xd = x.float().to(dev()).requires_grad_(True)
    y = ops.avgpool3s2(ops.avgpool3s2(xd))
    assert tuple(y.shape) == (8, 3, 64, 64) and nerr(y, yr) <= 1e-6
    y.backward(dy.float().to(dev()))
    assert nerr(xd.grad, xr.grad) <= 1e-6


@pytest.mark.parametrize("shape,positive", [((2, 256, 1, 1), False), ((8, 256, 32, 32), True), ((3, 100, 7, 7), False)])
def test_global_avgpool_shapes(shape, positive):
    from munit_amd import ops
    x = rnd(shape, 1)
    if positive:
        x = x.clamp_min(0)
    xr = x.clone().requires_grad_(True)
    yr = xr.mean(dim=(2, 3), keepdim=True)
    dy = rnd(tuple(yr.shape), 2)
    yr.backward(dy)
    xd = x.float().to(dev()).requires_grad_(True)
    y = ops.global_avgpool(xd)
    assert nerr(y, yr) <= 1e-6
    y.backward(dy.float().to(dev()))
    assert nerr(xd.grad, xr.grad) <= 1e-6


@pytest.mark.parametrize("shape,masked", [((1, 1, 1, 1), False), ((1, 1, 1, 262145), False), ((8, 3, 256, 256), True),
                                          ((8, 256, 64, 64), False)], ids=["n1", "n262145", "image_masked", "content"])
def test_l1_mean_sizes(shape, masked):
    """One element; one past a full pass of 1024 x 256 threads (the grid-stride wrap of the partial kernel); the image
    reconstruction with a mask and the content code of config_256 at batch 8.  Every seventh element has a == b exactly:
    gradient 0, as torch.sign."""
    from munit_amd import ops
    a, b = rnd(shape, 1).float().double(), rnd(shape, 2).float().double()
    b.view(-1)[::7] = a.view(-1)[::7]
    m = None
    if masked:
        B, _, H, W = shape
        m = (torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(3)) > 0.5).double()
    lr = O.l1_masked(a, b, m) if masked else O.l1(a, b)
    ad, bd = (t.float().to(dev()).requires_grad_(True) for t in (a, b))
    l = ops.l1_mean(ad, bd, m.float().to(dev()) if masked else None)
    assert abs(float(l) - float(lr)) <= 1e-6 * abs(float(lr))
    torch.autograd.backward([l], [torch.tensor(12.0, device=dev())])
    g = 12.0 * torch.sign(a - b) / a.numel()
    if masked:
        g = g * (1 - m)
    assert nerr(ad.grad, g) <= 1e-6 and nerr(bd.grad, -g) <= 1e-6
    assert bool((ad.grad.cpu().view(-1)[::7] == 0).all())


def test_l1_mean_bf16_content_code():
    """bf16 storage: the content-code reconstruction of config #3 (32 x 256 x 64 x 64)."""
    from munit_amd import ops
    shape = (32, 256, 64, 64)
    a, b = rnd(shape, 13).float().bfloat16(), rnd(shape, 14).float().bfloat16()
    ad = a.to(dev()).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bd = b.to(dev()).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    a, b = a.double(), b.double()
    out = ops.l1_mean(ad, bd)
    ref = float((a - b).abs().mean())
    assert out.dtype == torch.float32 and abs(float(out.detach()) - ref) <= 1e-6 * ref
    out.backward()
    g = torch.sign(a - b) / a.numel()
    assert nerr(ad.grad, g) <= BF16_OUT and nerr(bd.grad, -g) <= BF16_OUT


@pytest.mark.parametrize("target", [0.0, 1.0])
def test_mse_const_sizes(target):
    """n = 1 and the discriminator outputs of config #2 (256 x 256, batch 8): 16 x 16, 8 x 8, 4 x 4."""
    from munit_amd import ops
    for shape in [(1, 1, 1, 1), (8, 1, 16, 16), (8, 1, 8, 8), (8, 1, 4, 4)]:
        x = rnd(shape, 5)
        xr = x.clone().requires_grad_(True)
        lr = torch.mean((xr - target) ** 2)
        (3.0 * lr).backward()
        xd = x.float().to(dev()).requires_grad_(True)
        l = ops.mse_const(xd, target)
        assert abs(float(l) - float(lr)) <= 1e-6 * float(lr), (shape, target)
        torch.autograd.backward([l], [torch.tensor(3.0, device=dev())])
        assert nerr(xd.grad, xr.grad) <= 1e-6, (shape, target)


ADAM_WRAP = 2048 * 256 * 4 + 5      # past one grid-stride pass of the float4 loop, with a 1-element tail


@pytest.mark.parametrize("n", [1, 3, ADAM_WRAP])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("step", [1, 1000])
def test_adam_sizes(n, wd, step):
    """One update from a live state against O.adam_update in fp64: bias correction at steps 1 and 1000, weight decay 0 and
    1e-2, the scalar tail alone (n = 1, 3) and the grid-stride wrap."""
    from munit_amd import ops
    p, g = rnd((n,), 1).float().double(), rnd((n,), 2, 0.01).float().double()
    m, v = rnd((n,), 3, 0.01).float().double(), (rnd((n,), 4, 0.01) ** 2).float().double()
    pd, gd, md, vd = (t.float().to(dev()).contiguous() for t in (p, g, m, v))
    O.adam_update(p, g, m, v, step, 1e-4, 0.5, 0.999, 1e-8, wd)
    ops.adam_step(pd, gd, md, vd, 1e-4, 0.5, 0.999, 1e-8, wd, step)
    ep, em, ev = float((pd.double().cpu() - p).abs().max()), nerr(md, m), nerr(vd, v)
    assert ep <= 2e-6 and em <= 1e-6 and ev <= 1e-6, (ep, em, ev)


def test_extraadam_wrap():
    """ExtraAdam modes 0, 1, 2 (first extrapolation, a further one, the step) at the grid-stride wrap size."""
    from munit_amd import ops
    n = ADAM_WRAP
    p0 = rnd((n,), 1).float().double()
    gs = [rnd((n,), 10 + k, 0.3).float().double() for k in range(3)]
    pr = [p0.clone()]
    st = O.ExtraAdamState(pr, 1e-3, (0.5, 0.999), 1e-2)
    pd = p0.float().to(dev()).contiguous()
    md, vd, sd = torch.zeros(n, device=dev()), torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    for k, (mode, code) in enumerate([("extrapolation", 0), ("extrapolation", 1), ("step", 2)]):
        getattr(st, mode)([gs[k]])
        ops.extraadam_step(pd, gs[k].float().to(dev()).contiguous(), md, vd, sd, 1e-3, 0.5, 0.999, 1e-8, 1e-2, k + 1, code)
        assert float((pd.double().cpu() - pr[0]).abs().max()) <= 2e-6, (k, mode)
    assert nerr(md, st.m[0]) <= 1e-6 and nerr(vd, st.v[0]) <= 1e-6


# ------------------------------------------------------------------------------------------------------------------------
# contract of the non-conv entry points (tests/kernel_contract.py)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(NORM_CASES)), ids=lambda i: _NID(NORM_CASES[i]))
def test_norm_entry_point_contract(i):
    """Guards, poison, full writes, determinism, d_adain columns, LayerNorm acc, the short workspace -- and the split
    partials left in the workspace equal tests/test_cpu_norm_regimes.py's restatement of the split logic."""
    from tests import kernel_contract as K
    from tests.test_cpu_norm_regimes import partial_doubles
    kind, dt, B, C, H, W = NORM_CASES[i]
    act, residual = _norm_setup(NORM_CASES[i], i)
    code = ACT_CODES.index(act)
    if kind == "ln":
        nf, nb = K.check_layernorm(B, H * W, C, dt == "bf16", code)
    else:
        nf, nb = K.check_instnorm(B, H * W, C, dt == "bf16", kind == "adain", residual, code)
    want = (partial_doubles(kind, B, H * W, C, False), partial_doubles(kind, B, H * W, C, True))
    assert (nf, nb) == want, ("split partials in the workspace", NORM_CASES[i], (nf, nb), want)


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 64), (2, 2, 3, 64), (1, 5, 4, 64), (8, 256, 256, 3), (3, 13, 7, 5)])
def test_pool_entry_point_contract(B, H, W, C):
    from tests import kernel_contract as K
    K.check_avgpool(B, H, W, C)
    K.check_gap(B, H * W, C)


def test_pointwise_entry_point_contract():
    from tests import kernel_contract as K
    for n in (1, 3, 1027, 262145):
        K.check_act_bwd(n)
        K.check_scale(n)
    K.check_weighted_sum()


@pytest.mark.parametrize("npix,C,masked,bf16", [(1, 1, False, False), (262145, 1, True, False), (8 * 64 * 64, 3, True, False),
                                               (2 * 16 * 16, 256, False, True), (262145, 2, True, True)])
def test_loss_entry_point_contract(npix, C, masked, bf16):
    from tests import kernel_contract as K
    K.check_l1(npix, C, masked, bf16)
    if not bf16:
        K.check_mse(npix * C, float(masked))


@pytest.mark.parametrize("n", [1, 3, 1027, ADAM_WRAP])
def test_optimizer_entry_point_contract(n):
    from tests import kernel_contract as K
    K.check_adam(n)


@pytest.mark.parametrize("B,h,w", [(1, 8, 8), (3, 17, 12)])
def test_image_entry_point_contract(B, h, w):
    from tests import kernel_contract as K
    K.check_image(B, h, w)


def test_kinks_records_one_relu_mask_and_two_l1_signs():
    """ops.kinks around a conv with a ReLU and an L1 term: the mask is the sign of the output, the L1 term records, a nested
    kinks(mask=None) switches only that channel off, and every sink is None afterwards."""
    from munit_amd import ops
    cl = lambda t: t.float().to(dev()).contiguous(memory_format=torch.channels_last)
    x, w = cl(rnd((1, 4, 8, 8), 1)), cl(rnd((4, 4, 3, 3), 2, 0.2))
    a, b = cl(rnd((1, 4, 8, 8), 3)), cl(rnd((1, 4, 8, 8), 4))
    with ops.kinks(mask=True, l1=True) as k:
        y = ops.conv2d(x, w, None, 1, 1, "reflect", False, "relu")
        ops.l1_mean(a, b)
        with ops.kinks(mask=None):
            ops.conv2d(x, w, None, 1, 1, "reflect", False, "relu")
            ops.l1_mean(a, b)
    assert len(k.mask) == 1 and torch.equal(k.mask[0], y > 0) and 0 < int(k.mask[0].sum()) < y.numel()
    assert len(k.l1) == 2 and torch.equal(k.l1[0], a > b) and torch.equal(k.l1[1], a > b)
    assert (ops.MASK_SINK, ops.L1_SINK, ops.SEG_SINK, ops.DANN_SINK) == (None, None, None, None)


def _half_up(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


# public function -> (library symbols' stem, output extent or None for (B, C), the kinks channel of its winners, the library
# takes (B, H*W, C)): the test's own statement of what each wrapper has to hand to the library, not read from ops._POOLS
_POOL_CALLS = {
    "avgpool3s2": ("munit_avgpool3s2", _half_up, None, False),
    "global_avgpool": ("munit_gap", lambda h, w: (1, 1), None, True),
    "maxpool3s2": ("munit_maxpool3s2", _half_up, "seg", False),
    "avgpool7": ("munit_avgpool7", lambda h, w: (h, w), None, False),
    "maxpool2": ("munit_maxpool2", lambda h, w: (h // 2, w // 2), "dann", False),
    "avgpool16": ("munit_avgpool16", None, None, False),
}
_POOL_SHAPES = [("avgpool3s2", (2, 3, 5, 7)), ("avgpool3s2", (1, 1, 1, 1)), ("global_avgpool", (2, 66, 3, 5)),
                ("maxpool3s2", (1, 3, 5, 7)), ("maxpool3s2", (1, 2, 1, 1)), ("avgpool7", (1, 4, 9, 5)), ("avgpool7", (1, 4, 1, 1)),
                ("maxpool2", (1, 4, 5, 3)), ("avgpool16", (2, 8, 17, 31))]


@pytest.mark.parametrize("layout", ["channels_last", "nchw"])
@pytest.mark.parametrize("name,shape", _POOL_SHAPES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_pool_wrappers_equal_direct_library_calls(name, shape, layout):
    """Each public pooling function, forward and backward, bit for bit against direct calls of its two library symbols on
    dense NHWC copies, writing into buffers filled with NaN (0xEE for the winners) beforehand; and what it leaves in the
    kink sinks: the max-pools their winners, once, in their own channel, the average pools nothing."""
    from munit_amd import _lib, ops
    lib = _lib.load()
    stem, extent, channel, flat = _POOL_CALLS[name]
    b, c, h, w = shape
    x = rnd(shape, 11).float().to(dev())
    x = x.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else x.contiguous()
    x.requires_grad_(True)
    with ops.kinks(seg=True, dann=True) as k:
        y = getattr(ops, name)(x)
    out_shape = (b, c) if extent is None else (b, c) + extent(h, w)
    assert tuple(y.shape) == out_shape and y.dtype == torch.float32
    if name in ("global_avgpool", "avgpool16"):                  # a non-contiguous view: every second column of (.., 2C, ..)
        dy = rnd((b, 2 * c) + out_shape[2:], 12).float().to(dev())[:, ::2]
        assert not dy.is_contiguous()
    else:
        dy = rnd(out_shape, 12).float().to(dev())               # plain NCHW: the wrapper makes it NHWC
    y.backward(dy)

    nan = float("nan")
    dims = (b, h * w, c) if flat else (b, h, w, c)
    rows = lambda t: t.permute(0, 2, 3, 1).contiguous() if t.dim() == 4 else t.contiguous()      # dense NHWC / (B, C)
    x_raw, dy_raw = rows(x.detach()), rows(dy)
    y_raw = torch.full(dy_raw.shape, nan, device=dev())
    dx_raw = torch.full(x_raw.shape, nan, device=dev())
    win = (torch.full(dy_raw.shape, 0xEE, dtype=torch.uint8, device=dev()),) if channel else ()
    wp = tuple(ops._p(t) for t in win)
    _lib.check(getattr(lib, stem + "_fwd")(ops._p(x_raw), ops._p(y_raw), *wp, *dims, ops._stream()), stem + "_fwd")
    _lib.check(getattr(lib, stem + "_bwd")(ops._p(dy_raw), *wp, ops._p(dx_raw), *dims, ops._stream()), stem + "_bwd")
    assert not torch.isnan(y_raw).any() and not torch.isnan(dx_raw).any()
    assert torch.equal(rows(y.detach()), y_raw)
    assert torch.equal(rows(x.grad), dx_raw)
    got = {"seg": k.seg, "dann": k.dann}
    for ch, entries in got.items():
        assert len(entries) == (1 if ch == channel else 0), (ch, len(entries))
    if channel:
        assert got[channel][0].dtype == torch.uint8 and torch.equal(got[channel][0], win[0]) and int(win[0].max()) < 9
    assert ops.SEG_SINK is None and ops.DANN_SINK is None


@pytest.mark.parametrize("shape", [(1, 6, 4, 4), (1, 4, 1, 4)])
def test_maxpool2_refuses_its_precondition_before_any_launch(shape):
    from munit_amd import ops
    x = rnd(shape, 1).float().to(dev())
    with ops.kinks(seg=True, dann=True) as k:
        with pytest.raises(RuntimeError, match=r"munit_amd\.maxpool2: needs H, W >= 2 and C %% 4 == 0, got \(%d, %d, %d, %d\)" % shape):
            ops.maxpool2(x)
    assert k.seg == [] and k.dann == []
