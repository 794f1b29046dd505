"""FID evaluation: the reference's scripts/inception_utils.py with its arithmetic on HIP kernels.

Same names and parameter lists as the reference:
  WrapInception(net).forward(x)                                inception_utils.py:27-85
  torch_cov(m, rowvar=False)                                   inception_utils.py:90-120
  sqrt_newton_schulz(A, numIters, dtype=None)                  inception_utils.py:125-140
  numpy_calculate_frechet_distance(mu1, sigma1, mu2, sigma2)   inception_utils.py:145-202   (host, scipy)
  torch_calculate_frechet_distance(mu1, sigma1, mu2, sigma2)   inception_utils.py:205-241
  accumulate_inception_activations(trainer, fid_loader, net)   inception_utils.py:246-254
  load_inception_net(parallel=False)                           inception_utils.py:258-264   (reads MUNIT_INCEPTION_CKPT)
  prepare_inception_metrics(inception_moment, parallel=False)  inception_utils.py:271-308   (+ net=, see below)

The covariance, the 400 Newton-Schulz iterations on the 2048 x 2048 product and the distance itself run in
libmunit_hip.so (csrc/fid.hip: munit_fid_moments, munit_sqrt_newton_schulz, munit_frechet_distance, all on the exact-fp32
dense product munit_gemm_f32).  There is no CPU path for the `torch_*` functions: a host tensor raises.

The feature network is the Inception-v3 trunk of munit_amd/inception.py (csrc/inception.hip): the input normalisation and
resize, 94 convolutions with their batch norms folded in, the 3 x 3 pools and the final 8 x 8 mean, all HIP kernels.  Its
weights are torchvision's `inception_v3` state dict; nothing here downloads it: load_inception_net reads the file named by
the environment variable MUNIT_INCEPTION_CKPT.  The reference builds the network with transform_input=False, so the
normalisation of WrapInception.forward is the only one -- there is no second one inside the network.  Any other feature
network still plugs in as `prepare_inception_metrics(..., net=f)`: a callable mapping a (B, 3, H, W) image batch in [-1, 1]
to (B, D) fp32 device features.  DESIGN.md section 10.7.
"""
import os

import numpy as np
import torch

from . import ops

NEWTON_SCHULZ_ITERS = 400    # torch_calculate_frechet_distance, inception_utils.py:234


CKPT_ENV = "MUNIT_INCEPTION_CKPT"

_NO_CKPT = (
    "munit_amd.inception_utils: the Inception-v3 trunk needs torchvision's inception_v3 weights, and nothing here downloads "
    "them: set the environment variable " + CKPT_ENV + " to the state-dict file (inception_v3_google-*.pth), or pass your "
    "own feature network as prepare_inception_metrics(inception_moment, net=f): a callable from a (B, 3, H, W) image batch "
    "in [-1, 1] to (B, D) fp32 device features.")


class WrapInception(object):
    """The reference's wrapper of torchvision's inception_v3 on HIP kernels.  net: a munit_amd.inception.InceptionV3, a
    state-dict mapping, or any object with .state_dict() (a torchvision module).  forward(x): a (B, 3, H, W) fp32 device
    batch in [-1, 1], planar or channels_last -> (B, 2048) fp32 pool features: ((x + 1) / 2 - mean) / std, the bilinear
    resize (align_corners=True) to 299 x 299 unless x has that size, the trunk, the mean over the 8 x 8 map."""

    def __init__(self, net):
        from .inception import InceptionV3
        self.net = net if isinstance(net, InceptionV3) else InceptionV3(net)

    def forward(self, x):
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 4 or x.shape[0] < 1 or x.shape[1] != 3:
            raise RuntimeError("munit_amd.inception_utils: WrapInception takes a (B, 3, H, W) batch on a HIP device (no CPU "
                               "fallback exists); got %s" % (getattr(x, "device", type(x)),))
        # straight into the trunk's own input buffer
        pixels = ops.inception_input(x, out=self.net.input_buffer(x.device, x.shape[0]))
        return ops.pixel_mean(self.net(pixels))

    __call__ = forward


def torch_cov(m, rowvar=False):
    """Covariance of the variables of a 2-D device tensor m: columns are variables and rows observations, or the other way
    round with rowvar.  Centred first, then Xc^T Xc / (N - 1) (munit_fid_moments).  Unlike the reference, whose `m -= mean`
    writes through a view, m is left unchanged."""
    if m.dim() != 2:
        raise ValueError("torch_cov: a 2-D tensor (observations x variables) is expected, got %d dimensions" % m.dim())
    pool = m.t().contiguous() if rowvar else m.contiguous()
    return ops.fid_moments(pool)[1]


def sqrt_newton_schulz(A, numIters, dtype=None):
    """Matrix square root of A (b, D, D) by numIters Newton-Schulz iterations (munit_sqrt_newton_schulz).  dtype: None or
    fp32, the only arithmetic there is."""
    if dtype not in (None, torch.float32, "torch.cuda.FloatTensor"):
        raise ValueError("sqrt_newton_schulz: fp32 only, got dtype %r" % (dtype,))
    return ops.sqrt_newton_schulz(A.contiguous(), numIters)


def numpy_calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """Frechet distance between N(mu1, sigma1) and N(mu2, sigma2) on the host with scipy's sqrtm (the `use_torch=False`
    path): |mu1 - mu2|^2 + tr(sigma1 + sigma2 - 2 sqrt(sigma1 sigma2)).  A non-finite root is retried with eps on both
    diagonals; a root with a real imaginary part on its diagonal (beyond 1e-3) is an error."""
    from scipy import linalg          # lazily: only this path needs scipy
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    assert mu1.shape == mu2.shape, "Training and test mean vectors have different lengths"
    assert sigma1.shape == sigma2.shape, "Training and test covariances have different dimensions"
    root = linalg.sqrtm(sigma1.dot(sigma2))
    if not np.isfinite(root).all():
        print("fid calculation produces singular product; adding %s to diagonal of cov estimates" % eps)
        ridge = eps * np.eye(sigma1.shape[0])
        root = linalg.sqrtm((sigma1 + ridge).dot(sigma2 + ridge))
    if np.iscomplexobj(root):
        if not np.allclose(np.diagonal(root).imag, 0, atol=1e-3):
            raise ValueError("Imaginary component {}".format(np.max(np.abs(root.imag))))
        root = root.real
    delta = mu1 - mu2
    return delta.dot(delta) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(root)


def torch_calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """The same distance on the device, the square root by 400 Newton-Schulz iterations like the reference
    (munit_frechet_distance): a 0-d device tensor.  eps is accepted and unused, as in the reference."""
    assert mu1.shape == mu2.shape, "Training and test mean vectors have different lengths"
    assert sigma1.shape == sigma2.shape, "Training and test covariances have different dimensions"
    return ops.frechet_distance(mu1.contiguous(), sigma1.contiguous(), mu2.contiguous(), sigma2.contiguous(),
                                NEWTON_SCHULZ_ITERS)


def accumulate_inception_activations(trainer, fid_loader, net):
    """Translate every (x_a, x_b) batch of fid_loader with trainer.sample_fid and run the feature network over the result;
    returns the (N, D) pool."""
    pool = []
    for images_a_fid, images_b_fid in fid_loader:
        with torch.no_grad():
            batch_fake = trainer.sample_fid(images_a_fid, images_b_fid)
            pool.append(net(batch_fake))
    return torch.cat(pool, 0)


def load_inception_net(parallel=False):
    """WrapInception over the state dict in the file the environment variable MUNIT_INCEPTION_CKPT names (torchvision's
    inception_v3_google-*.pth).  Never downloads and searches no cache: without the variable NotImplementedError, with a
    missing file FileNotFoundError."""
    if parallel:
        raise NotImplementedError("munit_amd.inception_utils: parallel=True (nn.DataParallel over the feature network) is "
                                  "not supported; evaluate on one device")
    path = os.environ.get(CKPT_ENV)
    if not path:
        raise NotImplementedError(_NO_CKPT)
    if not os.path.isfile(path):
        raise FileNotFoundError("munit_amd.inception_utils: %s names %r, which is not a file" % (CKPT_ENV, path))
    return WrapInception(torch.load(path, map_location="cpu", weights_only=True))


def prepare_inception_metrics(inception_moment, parallel=False, net=None):
    """Returns get_inception_metrics(trainer, fid_loader, prints=True, use_torch=True) -> FID as a Python float, against
    the moments `mu` (D,) and `sigma` (D, D) stored in the .npz file `inception_moment`.  net: the feature network (the one
    extension over the reference's parameter list; None: load_inception_net(), the Inception trunk with the weights
    MUNIT_INCEPTION_CKPT names)."""
    if parallel:
        raise NotImplementedError("munit_amd.inception_utils: parallel=True (nn.DataParallel over the feature network) is "
                                  "not supported; evaluate on one device")
    with np.load(inception_moment) as moments:
        data_mu, data_sigma = moments["mu"], moments["sigma"]
    if net is None:
        net = load_inception_net(parallel)

    def get_inception_metrics(trainer, fid_loader, prints=True, use_torch=True):
        if prints:
            print("Gathering activations...")
        pool = accumulate_inception_activations(trainer, fid_loader, net)
        if pool.dim() != 2 or pool.dtype != torch.float32:
            raise RuntimeError("munit_amd.inception_utils: net must return (B, D) fp32 features, the pool is %s %s"
                               % (tuple(pool.shape), pool.dtype))
        d = pool.shape[1]
        if data_mu.shape != (d,) or data_sigma.shape != (d, d):
            raise ValueError("munit_amd.inception_utils: %s holds moments of shape %s / %s, the features are %d wide"
                             % (inception_moment, data_mu.shape, data_sigma.shape, d))
        if prints:
            print("Calculating means and covariances...")
        if use_torch:
            mu, sigma = ops.fid_moments(pool.contiguous())
        else:
            host = pool.cpu().numpy()
            mu, sigma = np.mean(host, axis=0), np.cov(host, rowvar=False)
        if prints:
            print("Covariances calculated, getting FID...")
        if use_torch:
            fid = torch_calculate_frechet_distance(
                mu, sigma,
                torch.tensor(data_mu).float().to(pool.device), torch.tensor(data_sigma).float().to(pool.device))
            fid = float(fid.cpu().numpy())
        else:
            fid = float(numpy_calculate_frechet_distance(mu, sigma, data_mu, data_sigma))
        return fid

    return get_inception_metrics
