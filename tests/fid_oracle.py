"""Helper of tests/test_cpu_fid.py and tests/test_gpu_fid.py (neither a test module nor a conftest): a torch-CPU
restatement of the reference's FID arithmetic (scripts/inception_utils.py: torch_cov, sqrt_newton_schulz,
torch_calculate_frechet_distance), parameterised by dtype, and the generator of the parity cases.

In fp64 it is the yardstick.  In fp32 it is the measure of what fp32 costs: the reference's own arithmetic in another
summation order than the HIP kernels', so its distance from the fp64 value (`e32`) is the size of error any fp32 evaluation
of the recurrence makes; the GPU tests allow the kernels max(4 e32, 16 * 2^-24) (ALLOW_FACTOR, ALLOW_FLOOR).

Parity cases (pools): N = 4 D rows, column scales spread over at most a factor 3, so that the product sigma1 sigma2 has a
condition number of 6..32 at D = 4 / 64 / 130 / 272 and the fp32 distance stays within 3e-7 of fp64 (relative to the sum of
its terms' magnitudes) at 20, 100 and 400 iterations.
With N ~ D the condition number reaches 1e5 and the fp32 error grows with the iteration count (4e-6 at 400): such cases measure
the conditioning of the recurrence, not a kernel, and are not parity cases."""
import torch

ALLOW_FACTOR = 4.0
ALLOW_FLOOR = 16 * 2.0 ** -24
U32 = 2.0 ** -24


def cov(pool, dtype=torch.float64):
    """(mu, sigma) as torch_cov(pool, rowvar=False) and torch.mean(pool, 0) give them: centred first."""
    x = pool.to(dtype)
    mu = x.mean(0)
    xc = x - mu
    return mu, (1.0 / (x.shape[0] - 1)) * xc.t().matmul(xc)


def sqrt_newton_schulz(a, iters, dtype=torch.float64):
    """The reference's recurrence on a (b, D, D), unchanged."""
    a = a.to(dtype)
    b, d = a.shape[0], a.shape[1]
    norm = a.mul(a).sum(dim=(1, 2)).sqrt()
    y = a / norm.view(b, 1, 1)
    eye = torch.eye(d, dtype=dtype).expand(b, d, d)
    z = eye.clone()
    for _ in range(iters):
        t = 0.5 * (3.0 * eye - z.bmm(y))
        y = y.bmm(t)
        z = t.bmm(z)
    return y * norm.sqrt().view(b, 1, 1)


def frechet(mu1, sigma1, mu2, sigma2, iters, dtype=torch.float64):
    """(distance, normaliser): the distance of torch_calculate_frechet_distance with `iters` iterations, and
    |dmu|^2 + tr sigma1 + tr sigma2 + 2 tr sqrt -- the sum of the magnitudes of its terms, which errors are measured against."""
    mu1, sigma1, mu2, sigma2 = (t.to(dtype) for t in (mu1, sigma1, mu2, sigma2))
    diff = mu1 - mu2
    root = sqrt_newton_schulz(sigma1.mm(sigma2).unsqueeze(0), iters, dtype)[0]
    dd, t1, t2, tr = diff.dot(diff), torch.trace(sigma1), torch.trace(sigma2), torch.trace(root)
    return float(dd + t1 + t2 - 2 * tr), float(dd + t1 + t2 + 2 * tr.abs())


def pools(d, seed=0, n=None, spread=3.0):
    """Two seeded fp32 pools (N, D), N = 4 D unless given: randn * logspace(0, log10(spread), D) * 0.3 + 0.4, and a second
    one with the scales flipped, * 0.25 + 0.5."""
    assert spread <= 3.0
    n = 4 * d if n is None else n
    g = torch.Generator().manual_seed(1000 * d + seed)
    scales = torch.logspace(0, float(torch.log10(torch.tensor(spread, dtype=torch.float64))), d, dtype=torch.float64)
    p1 = torch.randn(n, d, generator=g, dtype=torch.float64) * scales * 0.3 + 0.4
    p2 = torch.randn(n, d, generator=g, dtype=torch.float64) * scales.flip(0) * 0.25 + 0.5
    return p1.float(), p2.float()


def moments(d, seed=0, n=None):
    """fp32 (mu1, sigma1, mu2, sigma2) of the two pools, rounded from their fp64 moments."""
    p1, p2 = pools(d, seed, n)
    (m1, s1), (m2, s2) = cov(p1), cov(p2)
    return m1.float(), s1.float(), m2.float(), s2.float()


def allowance(e32):
    return max(ALLOW_FACTOR * e32, ALLOW_FLOOR)


def matrix_err(got, ref64):
    """Largest elementwise error over the largest entry of the fp64 matrix."""
    return float((got.double() - ref64).abs().max() / ref64.abs().max())


def chain_bound(k, alpha, absprod, beta_eye=0.0):
    """Elementwise bound of one k-ordered fp32 fmaf chain of length k followed by alpha * acc + beta_eye * I:
    (k + 2) 2^-24 (|alpha| (|op A| |B|) + |beta_eye| I), absprod = |op A| |B| in fp64."""
    eye = torch.eye(absprod.shape[-2], absprod.shape[-1], dtype=torch.float64)
    return (k + 2) * U32 * (abs(alpha) * absprod + abs(beta_eye) * eye)
