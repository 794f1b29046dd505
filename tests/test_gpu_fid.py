"""FID evaluation on the GPU (csrc/fid.hip through munit_amd.ops, munit_amd/inception_utils.py, data.get_fid_data_loader).

The dense product is pinned three ways: bit for bit on integer-lattice data (indexing, tails, leading dimensions -- no
tolerance), elementwise under the fmaf-chain bound (K + 2) 2^-24 (|alpha| |op A| |B| + |beta_eye| I) on random data, and under
the guard-band contract of tests/conv_contract.py.  The square root and the distance are held against tests/fid_oracle.py in
fp64 with an allowance that is measured, not chosen: max(4 e32, 16 * 2^-24), e32 being the error of the same oracle run in
fp32 on the same case (see fid_oracle's docstring).  Every test prints the figures it asserts on."""
import functools
from ctypes import c_float, c_size_t, c_void_p

import numpy as np
import pytest
import torch

from tests import fid_oracle as FO
from tests.lattice import lattice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GEMM_SHAPES = [(1, 1, 1), (3, 5, 2), (16, 16, 4), (17, 15, 5), (128, 128, 16), (129, 127, 33), (130, 130, 130),
               (272, 272, 272), (256, 384, 20)]
SCALINGS = [(1.0, 0.0), (-0.5, 1.5)]
COUNTS = [1, 2, 3, 8]


def _operands(m, n, k, trans_a, count, seed, kind):
    """`count` fp64 (A, B) pairs: A is (k, m) under trans_a, else (m, k)."""
    out = []
    for p in range(count):
        sa, sb = ((k, m) if trans_a else (m, k)), (k, n)
        if kind == "lattice":
            out.append((lattice(sa, seed + 2 * p, range(-3, 4)), lattice(sb, seed + 2 * p + 1, range(-3, 4))))
        else:
            g = torch.Generator().manual_seed(seed + p)
            out.append((torch.randn(sa, generator=g).double(), torch.randn(sb, generator=g).double()))
    return out


def _expected(a, b, trans_a, alpha, beta_eye):
    """fp64 (result, |op A| |B|) -- the epilogue written as the kernel documents it: alpha * acc + (row == col) * beta_eye."""
    opa = a.t() if trans_a else a
    eye = torch.eye(opa.shape[0], b.shape[1], dtype=torch.float64)
    return alpha * opa.matmul(b) + beta_eye * eye, opa.abs().matmul(b.abs())


@pytest.mark.parametrize("trans_a", [0, 1])
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_gemm_lattice_is_bit_exact(shape, trans_a):
    from munit_amd import ops
    m, n, k = shape
    for alpha, beta_eye in SCALINGS:
        for count in COUNTS:
            pairs = _operands(m, n, k, trans_a, count, 100 * count, "lattice")
            a_dev = [a.float().to(DEV) for a, _ in pairs]
            b_dev = [b.float().to(DEV) for _, b in pairs]
            got = ops.gemm(a_dev, b_dev, trans_a=bool(trans_a), alpha=alpha, beta_eye=beta_eye)
            for p, (a, b) in enumerate(pairs):
                want, _ = _expected(a, b, trans_a, alpha, beta_eye)
                assert float(want.abs().max()) < 2.0 ** 24
                assert torch.equal(got[p].cpu(), want.float()), (shape, trans_a, alpha, beta_eye, count, p)
    single = ops.gemm(a_dev[0], b_dev[0], trans_a=bool(trans_a), alpha=alpha, beta_eye=beta_eye)
    assert torch.equal(single, got[0])


@pytest.mark.parametrize("trans_a", [0, 1])
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_gemm_random_within_the_chain_bound(shape, trans_a):
    from munit_amd import ops
    m, n, k = shape
    worst = 0.0
    for alpha, beta_eye in SCALINGS:
        for count in COUNTS:
            pairs = _operands(m, n, k, trans_a, count, 7 * count, "random")
            pairs = [(a.float().double(), b.float().double()) for a, b in pairs]
            got = ops.gemm([a.float().to(DEV) for a, _ in pairs], [b.float().to(DEV) for _, b in pairs],
                           trans_a=bool(trans_a), alpha=alpha, beta_eye=beta_eye)
            for p, (a, b) in enumerate(pairs):
                want, absprod = _expected(a, b, trans_a, alpha, beta_eye)
                bound = FO.chain_bound(k, alpha, absprod, beta_eye)
                err = (got[p].cpu().double() - want).abs()
                ratio = float((err / bound.clamp_min(1e-300)).max())
                worst = max(worst, ratio)
                assert bool((err <= bound).all()), (shape, trans_a, alpha, beta_eye, count, p, ratio)
    print("gemm %s transA %d: worst error / chain bound %.3f" % (shape, trans_a, worst))


@pytest.mark.parametrize("extra", [3, 5, 8])
@pytest.mark.parametrize("trans_a", [0, 1])
def test_gemm_leading_dimensions_with_nan_padding(trans_a, extra):
    """Row strides beyond the rows (aligned and unaligned ones), NaN in every padding word: none is read, none is written."""
    from munit_amd import ops
    m, n, k = 129, 127, 33
    (a, b), = _operands(m, n, k, trans_a, 1, 5, "lattice")

    def padded(t):
        buf = torch.full((t.shape[0], t.shape[1] + extra), float("nan"), dtype=torch.float32, device=DEV)
        buf[:, :t.shape[1]] = t.float().to(DEV)
        return buf

    abuf, bbuf = padded(a), padded(b)
    cbuf = torch.full((m, n + extra), float("nan"), dtype=torch.float32, device=DEV)
    ops.gemm(abuf[:, :a.shape[1]], bbuf[:, :n], trans_a=bool(trans_a), alpha=-0.5, beta_eye=1.5, out=cbuf[:, :n])
    want, _ = _expected(a, b, trans_a, -0.5, 1.5)
    assert torch.equal(cbuf[:, :n].cpu(), want.float())
    assert bool(torch.isnan(cbuf[:, n:]).all()) and bool(torch.isnan(abuf[:, a.shape[1]:]).all())


@pytest.mark.parametrize("shape,trans_a", [((17, 15, 5), 0), ((129, 127, 33), 1), ((130, 130, 130), 0)])
def test_gemm_contract(shape, trans_a):
    """Three problems in one launch between guard bands: guards and inputs bitwise unchanged, every output element written
    under both NaN payloads, the two results bitwise equal; overlapping C is refused with nothing written."""
    from munit_amd import _lib
    from tests import conv_contract as CC
    lib = _lib.load()
    m, n, k = shape
    count = 3
    sizes = {}
    for p in range(count):
        sizes.update({"a%d" % p: m * k * 4, "b%d" % p: k * n * 4, "c%d" % p: m * n * 4})
    arena = CC.Arena(sizes, torch.device(DEV))
    inputs = [nm for nm in sizes if nm[0] in "ab"]
    for i, nm in enumerate(inputs):
        CC.fill_random(arena.view(nm, torch.float32), 60 + i)
    outs = [arena.view("c%d" % p, torch.float32) for p in range(count)]
    L = CC.Launches(arena, inputs, "gemm_f32 %s transA %d" % (shape, trans_a))
    lda = m if trans_a else k

    def run(payload, table=None):
        for o in outs:
            CC.poison(o, payload)
        if table is None:
            table = [(arena.ptr("a%d" % p).value, arena.ptr("b%d" % p).value, arena.ptr("c%d" % p).value) for p in range(count)]
        prob = (_lib.GemmProblem * count)(*[_lib.GemmProblem(*t) for t in table])
        return lib.munit_gemm_f32(prob, count, m, n, k, lda, n, n, trans_a, c_float(-0.5), c_float(1.5), CC.stream())

    L.after(run(0), "first payload")
    assert all(CC.no_nan(o) for o in outs)
    first = [o.clone() for o in outs]
    L.after(run(1), "second payload")
    assert all(CC.bitwise_equal(o, f) for o, f in zip(outs, first))
    for p in range(count):
        a = arena.view("a%d" % p, torch.float32).cpu().double().view((k, m) if trans_a else (m, k))
        b = arena.view("b%d" % p, torch.float32).cpu().double().view(k, n)
        want, absprod = _expected(a, b, trans_a, -0.5, 1.5)
        assert bool(((first[p].cpu().double().view(m, n) - want).abs() <= FO.chain_bound(k, -0.5, absprod, 1.5)).all())
    # C of problem 2 is B of problem 0: refused, and nothing is written
    bad = [(arena.ptr("a%d" % p).value, arena.ptr("b%d" % p).value, arena.ptr("c%d" % p).value) for p in range(count)]
    bad[2] = (bad[2][0], bad[2][1], bad[0][1])
    assert run(0, bad) == -1 and b"overlaps" in lib.munit_last_error()
    L.verify("refused overlap")
    assert all(bool((o.view(torch.int32) == CC.POISON[4][0]).all()) for o in outs)


# ---- moments ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(2, 1), (5, 3), (48, 12), (520, 130), (300, 272)])
def test_fid_moments_against_fp64(n, d):
    from munit_amd import ops
    pool = FO.pools(d, n=n)[0]
    dev = pool.to(DEV)
    before = dev.clone()
    mu, sigma = ops.fid_moments(dev)
    assert torch.equal(dev.view(torch.int32), before.view(torch.int32)), "the pool was modified"
    mu64, sigma64 = FO.cov(pool)
    xc = pool.double() - mu64
    mu_bound = (n + 2) * FO.U32 * pool.double().abs().sum(0) / n
    sigma_bound = FO.chain_bound(n, 1.0 / (n - 1), xc.abs().t().matmul(xc.abs()))
    emu, esig = (mu.cpu().double() - mu64).abs(), (sigma.cpu().double() - sigma64).abs()
    print("fid_moments (%d, %d): mu error / bound %.3f, sigma error / bound %.3f"
          % (n, d, float((emu / mu_bound).max()), float((esig / sigma_bound.clamp_min(1e-300)).max())))
    assert bool((emu <= mu_bound).all()) and bool((esig <= sigma_bound).all())
    from munit_amd import inception_utils as IU
    assert torch.equal(IU.torch_cov(dev), sigma) and torch.equal(IU.torch_cov(dev.t().contiguous(), rowvar=True), sigma)


def test_fid_moments_constant_column_on_the_lattice():
    from munit_amd import ops
    n, d = 37, 70
    pool = lattice((n, d), 3, range(-4, 5))
    pool[:, 17] = 3.0
    pool[:, 69] = -2.0
    mu, sigma = ops.fid_moments(pool.float().to(DEV))
    mu, sigma = mu.cpu(), sigma.cpu()
    assert float(mu[17]) == 3.0 and float(mu[69]) == -2.0
    for c in (17, 69):
        assert bool((sigma[c] == 0).all()) and bool((sigma[:, c] == 0).all())
    assert bool((sigma.diagonal()[:17] > 0).all())


# ---- square root and distance ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _product(d, seed):
    """The fp32 product sigma1 sigma2 of a generated case (rounded from fp64), on the host."""
    _, s1, _, s2 = FO.moments(d, seed)
    return s1.double().mm(s2.double()).float()


@functools.lru_cache(maxsize=None)
def _roots(d, seed, iters):
    p = _product(d, seed).unsqueeze(0)
    return FO.sqrt_newton_schulz(p, iters)[0], FO.sqrt_newton_schulz(p, iters, torch.float32)[0]


@pytest.mark.parametrize("iters", [0, 1, 20, 400])
@pytest.mark.parametrize("d", [1, 4, 64, 130, 272])
def test_sqrt_newton_schulz_against_fp64(d, iters):
    from munit_amd import inception_utils as IU
    for batch in (1, 3):
        a = torch.stack([_product(d, s) for s in range(batch)]).to(DEV)
        got = IU.sqrt_newton_schulz(a, iters).cpu()
        for s in range(batch):
            r64, r32 = _roots(d, s, iters)
            e32, ehip = FO.matrix_err(r32, r64), FO.matrix_err(got[s], r64)
            print("sqrt_newton_schulz D %d iters %d batch %d matrix %d: e32 %.3e hip %.3e allowance %.3e"
                  % (d, iters, batch, s, e32, ehip, FO.allowance(e32)))
            assert ehip <= FO.allowance(e32), (d, iters, batch, s, ehip, e32)


@pytest.mark.parametrize("iters", [0, 1, 20, 400])
@pytest.mark.parametrize("d", [1, 4, 64, 130, 272])
def test_frechet_distance_against_fp64(d, iters):
    from munit_amd import ops
    m = FO.moments(d)
    ref, norm = FO.frechet(*m, iters)
    f32, _ = FO.frechet(*m, iters, dtype=torch.float32)
    got = float(ops.frechet_distance(*(t.to(DEV) for t in m), iters=iters).cpu())
    e32, ehip = abs(f32 - ref) / norm, abs(got - ref) / norm
    print("frechet_distance D %d iters %d: fp64 %.9g hip %.9g e32 %.3e hip %.3e allowance %.3e"
          % (d, iters, ref, got, e32, ehip, FO.allowance(e32)))
    assert ehip <= FO.allowance(e32), (d, iters, got, ref, e32)


def test_frechet_distance_short_workspace_and_reproducibility():
    from munit_amd import _lib
    from tests import conv_contract as CC
    lib = _lib.load()
    d = 130
    m = [t.to(DEV) for t in FO.moments(d)]
    need = lib.munit_frechet_distance_workspace_bytes(d)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.empty(1, dtype=torch.float32, device=DEV)
    p = lambda t: c_void_p(t.data_ptr())

    def run(ws_bytes):
        CC.poison(out, 0)
        return lib.munit_frechet_distance(p(m[0]), p(m[1]), p(m[2]), p(m[3]), d, 20, p(out), p(ws), c_size_t(ws_bytes), CC.stream())

    assert run(need - 1) == -1 and b"frechet_distance: workspace too small" in lib.munit_last_error()
    torch.cuda.synchronize()
    assert int(out.view(torch.int32)) == CC.POISON[4][0]
    _lib.check(run(need), "frechet_distance")
    first = out.clone()
    ws.fill_(0xFF)
    _lib.check(run(need), "frechet_distance")
    assert CC.bitwise_equal(out, first) and CC.no_nan(out)


def test_full_width_square_root_and_distance():
    """D = 2048, the width the evaluation runs at: one iteration of the square root, two of the distance.

    Measured on MI355X: square root 3.04e-6 of the largest entry against e32 9.1e-7 (allowance 3.6e-6), distance 5.3e-9
    (e32 5.3e-9).  The square root is the case closest to its allowance in this file: the kernel's value is one k-ordered
    chain of 2048 terms per element and repeats bit for bit, while e32 is what the host's blocked fp32 BLAS makes of the
    same product (1.2e-6 .. 1.3e-6 with another CPU's kernels), so the margin moves with the host, not with the device."""
    from munit_amd import ops
    d = 2048
    m = FO.moments(d, n=4096)
    prod = m[1].double().mm(m[3].double()).float()
    r64 = FO.sqrt_newton_schulz(prod.unsqueeze(0), 1)[0]
    r32 = FO.sqrt_newton_schulz(prod.unsqueeze(0), 1, torch.float32)[0]
    got = ops.sqrt_newton_schulz(prod.unsqueeze(0).to(DEV), 1)[0].cpu()
    e32, ehip = FO.matrix_err(r32, r64), FO.matrix_err(got, r64)
    print("sqrt_newton_schulz D 2048 iters 1: e32 %.3e hip %.3e allowance %.3e" % (e32, ehip, FO.allowance(e32)))
    assert ehip <= FO.allowance(e32)
    ref, norm = FO.frechet(*m, 2)
    f32, _ = FO.frechet(*m, 2, dtype=torch.float32)
    hip = float(ops.frechet_distance(*(t.to(DEV) for t in m), iters=2).cpu())
    e32, ehip = abs(f32 - ref) / norm, abs(hip - ref) / norm
    print("frechet_distance D 2048 iters 2: fp64 %.9g hip %.9g e32 %.3e hip %.3e allowance %.3e"
          % (ref, hip, e32, ehip, FO.allowance(e32)))
    assert ehip <= FO.allowance(e32)


# ---- loader and end to end ---------------------------------------------------------------------------------------------
def _write_images(folder, count, h, w, seed):
    """PNG files of four flat random colours (one per quadrant) under noise; returns their paths."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    paths = []
    for i in range(count):
        base = rng.randint(40, 216, size=(2, 2, 3)).repeat(h // 2 + 1, 0).repeat(w // 2 + 1, 1)[:h, :w]
        img = np.clip(base + rng.randint(-30, 31, size=(h, w, 3)), 0, 255).astype(np.uint8)
        paths.append(str(folder / ("img_%02d.png" % i)))
        Image.fromarray(img).save(paths[-1])
    return paths


def _lists(folder, paths):
    fa, fb = folder / "list_a.txt", folder / "list_b.txt"
    fa.write_text("".join(p + "\n" for p in paths))
    fb.write_text("".join("%s/never_opened_%d.png\n" % (folder, i) for i in range(len(paths) + 1)))
    return str(fa), str(fb)


def test_fid_loader_batches(tmp_path):
    from munit_amd import data
    paths = _write_images(tmp_path, 6, 40, 56, 1)
    fa, fb = _lists(tmp_path, paths)
    pairs = list(data.get_fid_data_loader(fa, fb, 2, False, new_size=32))
    plain = list(data.DeviceBatchLoader(paths, None, 2, False, 32, 32, 32, crop=False, rank=0, world_size=1))
    assert len(pairs) == 3 and len(plain) == 3
    for (x_a, x_b), want in zip(pairs, plain):
        assert tuple(x_a.shape) == (2, 3, 32, 44)
        assert torch.equal(x_a.view(torch.int32), want.view(torch.int32))
        host = x_a.cpu()
        assert torch.equal(x_b.cpu().view(torch.int32), ((host - 0.5) / 0.5).view(torch.int32))
    # list order: batch k holds files 2k and 2k + 1
    singles = [data.DeviceBatchLoader([p], None, 1, False, 32, 32, 32, crop=False, rank=0, world_size=1) for p in paths]
    for k, (x_a, _) in enumerate(pairs):
        for j in range(2):
            assert torch.equal(x_a[j].cpu(), next(iter(singles[2 * k + j]))[0].cpu())


def _quadrant_means(x):
    """(B, 3, H, W) -> (B, 12): the mean of each quadrant of each channel, through the global average pool."""
    from munit_amd import ops
    h, w = x.shape[2] // 2, x.shape[3] // 2
    feats = [ops.global_avgpool(x[:, :, i * h:(i + 1) * h, j * w:(j + 1) * w]).reshape(x.shape[0], 3)
             for i in range(2) for j in range(2)]
    return torch.cat(feats, 1).contiguous()


def test_inception_metrics_end_to_end(tmp_path):
    from oracle import munit_oracle as O
    from munit_amd import data, inception_utils as IU
    from munit_amd.trainer import MUNIT_Trainer
    hp = O.default_hp(64, 1, 1)
    hp["gen"]["n_res"] = 1
    hp["guided"] = 1
    torch.manual_seed(11)
    trainer = MUNIT_Trainer(dict(hp))
    trainer.to(DEV)
    paths = _write_images(tmp_path, 48, 64, 64, 2)
    fa, fb = _lists(tmp_path, paths)
    mu2, sigma2 = FO.cov(FO.pools(12, seed=1, n=48)[1])
    npz = str(tmp_path / "moments.npz")
    np.savez(npz, mu=mu2.numpy(), sigma=sigma2.numpy())
    loader = lambda: data.get_fid_data_loader(fa, fb, 4, False, new_size=64)
    metrics = IU.prepare_inception_metrics(npz, net=_quadrant_means)
    fid = metrics(trainer, loader(), prints=False)
    assert isinstance(fid, float) and trainer.training
    pool = IU.accumulate_inception_activations(trainer, loader(), _quadrant_means).cpu()
    assert tuple(pool.shape) == (48, 12)
    m2 = (mu2.float(), sigma2.float())
    ref, norm = FO.frechet(*FO.cov(pool), *m2, 400)
    mu32, sigma32 = FO.cov(pool, torch.float32)
    f32, _ = FO.frechet(mu32, sigma32, *m2, 400, dtype=torch.float32)
    e32, ehip = abs(f32 - ref) / norm, abs(fid - ref) / norm
    print("end to end: fp64 %.9g hip %.9g e32 %.3e hip %.3e allowance %.3e" % (ref, fid, e32, ehip, FO.allowance(e32)))
    assert ehip <= FO.allowance(e32)
    from scipy import linalg
    host = pool.numpy()
    mu1, sigma1 = host.mean(0), np.cov(host, rowvar=False)
    root = linalg.sqrtm(sigma1.dot(sigma2.numpy())).real
    want = float(((mu1 - mu2.numpy()) ** 2).sum() + np.trace(sigma1) + np.trace(sigma2.numpy()) - 2 * np.trace(root))
    got = metrics(trainer, loader(), prints=False, use_torch=False)
    assert isinstance(got, float) and abs(got - want) <= 1e-6 * abs(want), (got, want)
    # moments of another width are refused
    np.savez(npz, mu=np.zeros(5), sigma=np.eye(5))
    with pytest.raises(ValueError, match="12 wide"):
        IU.prepare_inception_metrics(npz, net=_quadrant_means)(trainer, loader(), prints=False)
