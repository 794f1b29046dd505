// Kernels of the simulated / real feature classifier behind adaptation.adv_lambda / dfeat_lambda (scripts/utils.py:1277-1327,
// 1370-1392: MaxPool2d(2) -> BasicBlock(256, 128) -> MaxPool2d(2) -> BasicBlock(128, 64) -> AvgPool2d((16, 16)) -> Linear):
// training-mode BatchNorm2d, the 2x2 / stride-2 max-pool and the 16x16 average.  The convolutions run through
// munit_conv2d_*, the block tail through munit_add_relu_fwd, the head through munit_linear_* / munit_mse_const_*.
// fp32, NHWC, every global access a 16-byte vector along C (the uint8 winner map: 4 bytes).  All reductions are two-stage
// in a fixed order (per-block partials in the workspace, one finishing pass): no atomics, bitwise reproducible.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int BN_MAX_BLOCKS = 64;   // partial rows of a batch-norm reduction
constexpr int BN_MAX_C = 1024;

unsigned grid_for(long long n) { return (unsigned)std::max<long long>(1, std::min<long long>((n + NT - 1) / NT, 16384)); }

// ---- batch norm ------------------------------------------------------------------------------------------------------
// A block of 256 threads covers C / 4 column groups x rl = 256 / (C / 4) row lanes; block b owns the rows [b * per, (b + 1) * per).
int bn_blocks(long long R, int C) {
  const int rl = NT / (C / 4);
  return (int)std::max<long long>(1, std::min<long long>(BN_MAX_BLOCKS, (R + 8ll * rl - 1) / (8ll * rl)));
}

// sum over the block's row lanes in lane order; lane 0 of every column group returns the total
__device__ inline f32x4 block_rows_sum(f32x4 v, int c4, int lane, int C4, int rl, f32x4* red) {
  red[lane * C4 + c4] = v;
  __syncthreads();
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  if (lane == 0)
    for (int l = 0; l < rl; ++l) s += red[l * C4 + c4];
  __syncthreads();
  return s;
}

// mode 0: part[b][c] = sum of (x - x[0][c]) over the block's rows (shifted by the first row, so that a channel mean that is
// large against the spread costs no digits); mode 1: sum of (x - mean)^2 (the second pass of the variance)
__global__ void bn_partial_kernel(const float* __restrict__ x, const float* __restrict__ mean, long long R, int C, int mode,
                                  float* __restrict__ part) {
  __shared__ f32x4 red[NT];
  const int C4 = C >> 2, rl = NT / C4;      // C4 divides NT (host check): every thread has a slot
  const int c4 = threadIdx.x % C4, lane = threadIdx.x / C4;
  const long long per = (R + gridDim.x - 1) / gridDim.x;
  const long long r0 = (long long)blockIdx.x * per, r1 = r0 + per < R ? r0 + per : R;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 m = ld4((mode ? mean : x) + 4 * c4);
  const f32x4 lo = mode ? ld4(mean + C + 4 * c4) : acc;
  for (long long r = r0 + lane; r < r1; r += rl) {
    const f32x4 d = (ld4(x + r * C + 4 * c4) - m) - lo;
    acc += mode ? d * d : d;
  }
  const f32x4 s = block_rows_sum(acc, c4, lane, C4, rl, red);
  if (lane == 0) st4(part + (long long)blockIdx.x * C + 4 * c4, s);
}

// mode 0: mean = x[0][c] + sum of the partials / R, kept as two floats mean[c] + mean[C + c] (the fp32 rounding of a mean of 100
// is 4e-6 of a unit spread, which a sum over thousands of rows in the backward would amplify).  mode 1: rstd[c] = 1 / sqrt(var + eps) with the biased variance, and
// the running statistics move by `momentum` (running_var with the unbiased variance).
__global__ void bn_finish_kernel(const float* __restrict__ x, const float* __restrict__ part, int nb, long long R, int C,
                                 int mode, float eps, float momentum, float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ run_mean,
                                 float* __restrict__ run_var) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = 0.0;
  for (int i = 0; i < nb; ++i) s += (double)part[(long long)i * C + c];
  if (mode == 0) {
    const double mu = (double)x[c] + s / (double)R;
    const float hi = (float)mu;
    mean[c] = hi;
    mean[C + c] = (float)(mu - (double)hi);
    return;
  }
  const double var = s / (double)R;
  rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (run_mean) {
    const float m = (float)((double)mean[c] + (double)mean[C + c]);
    const float unb = (float)(s / (double)(R - 1));
    run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * m;
    run_var[c] = (1.f - momentum) * run_var[c] + momentum * unb;
  }
}

__device__ inline f32x4 relu4(f32x4 v) {
  return f32x4{v[0] > 0.f ? v[0] : 0.f, v[1] > 0.f ? v[1] : 0.f, v[2] > 0.f ? v[2] : 0.f, v[3] > 0.f ? v[3] : 0.f};
}
__device__ inline f32x4 rsqrt_eps4(f32x4 v, float eps) {
  return f32x4{1.f / sqrtf(v[0] + eps), 1.f / sqrtf(v[1] + eps), 1.f / sqrtf(v[2] + eps), 1.f / sqrtf(v[3] + eps)};
}

// y = act((x - mean) * rstd * gamma + beta); eval: mean / var are the running statistics
__global__ void bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd_or_var,
                                const float* __restrict__ gamma, const float* __restrict__ beta, long long R, int C, int relu,
                                int eval, float eps, float* __restrict__ y) {
  const int C4 = C >> 2;
  const long long total = R * C4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = 4 * (int)(i % C4);
    f32x4 rs = ld4(rstd_or_var + c);
    f32x4 d = ld4(x + 4 * i) - ld4(mean + c);
    if (eval) rs = rsqrt_eps4(rs, eps);
    else d -= ld4(mean + C + c);
    f32x4 v = d * rs * ld4(gamma + c) + ld4(beta + c);
    st4(y + 4 * i, relu ? relu4(v) : v);
  }
}

// part[b][0][c] = sum of g, part[b][1][c] = sum of g * xhat over the block's rows, g = dy gated by y > 0 behind a ReLU
__global__ void bn_bwd_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ y,
                                      const float* __restrict__ mean, const float* __restrict__ rstd, long long R, int C,
                                      int relu, float* __restrict__ part) {
  __shared__ f32x4 red[NT];
  const int C4 = C >> 2, rl = NT / C4;
  const int c4 = threadIdx.x % C4, lane = threadIdx.x / C4;
  const long long per = (R + gridDim.x - 1) / gridDim.x;
  const long long r0 = (long long)blockIdx.x * per, r1 = r0 + per < R ? r0 + per : R;
  f32x4 sg = f32x4{0.f, 0.f, 0.f, 0.f}, sgx = sg;
  const f32x4 m = ld4(mean + 4 * c4), lo = ld4(mean + C + 4 * c4), rs = ld4(rstd + 4 * c4);
  for (long long r = r0 + lane; r < r1; r += rl) {
    const long long o = r * C + 4 * c4;
    f32x4 g = ld4(dy + o);
    if (relu) {
      const f32x4 yy = ld4(y + o);
      g = f32x4{yy[0] > 0.f ? g[0] : 0.f, yy[1] > 0.f ? g[1] : 0.f, yy[2] > 0.f ? g[2] : 0.f, yy[3] > 0.f ? g[3] : 0.f};
    }
    sg += g;
    sgx += g * (((ld4(x + o) - m) - lo) * rs);
  }
  const f32x4 a = block_rows_sum(sg, c4, lane, C4, rl, red);
  const f32x4 b = block_rows_sum(sgx, c4, lane, C4, rl, red);
  if (lane == 0) {
    st4(part + ((long long)blockIdx.x * 2 + 0) * C + 4 * c4, a);
    st4(part + ((long long)blockIdx.x * 2 + 1) * C + 4 * c4, b);
  }
}

// sums[0][c] = sum g, sums[1][c] = sum g * xhat (the tail of the workspace); dbeta / dgamma = acc * old + those, when given
__global__ void bn_bwd_finish_kernel(const float* __restrict__ part, int nb, int C, float acc, float* __restrict__ sums,
                                     float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double a = 0.0, b = 0.0;
  for (int i = 0; i < nb; ++i) {
    a += (double)part[((long long)i * 2 + 0) * C + c];
    b += (double)part[((long long)i * 2 + 1) * C + c];
  }
  sums[c] = (float)a;
  sums[C + c] = (float)b;
  if (dbeta) dbeta[c] = (acc != 0.f ? acc * dbeta[c] : 0.f) + (float)a;
  if (dgamma) dgamma[c] = (acc != 0.f ? acc * dgamma[c] : 0.f) + (float)b;
}

// dx = gamma * rstd * (g - sum_g / R - xhat * sum_gx / R)
__global__ void bn_bwd_dx_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ y,
                                 const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ rstd,
                                 const float* __restrict__ sums, long long R, int C, int relu, float inv_r,
                                 float* __restrict__ dx) {
  const int C4 = C >> 2;
  const long long total = R * C4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = 4 * (int)(i % C4);
    f32x4 g = ld4(dy + 4 * i);
    if (relu) {
      const f32x4 yy = ld4(y + 4 * i);
      g = f32x4{yy[0] > 0.f ? g[0] : 0.f, yy[1] > 0.f ? g[1] : 0.f, yy[2] > 0.f ? g[2] : 0.f, yy[3] > 0.f ? g[3] : 0.f};
    }
    const f32x4 rs = ld4(rstd + c);
    const f32x4 xh = ((ld4(x + 4 * i) - ld4(mean + c)) - ld4(mean + C + c)) * rs;
    st4(dx + 4 * i, ld4(gamma + c) * rs * (g - ld4(sums + c) * inv_r - xh * (ld4(sums + C + c) * inv_r)));
  }
}

size_t bn_part_bytes(int C) { return align_up((size_t)BN_MAX_BLOCKS * 2 * C * sizeof(float), 256); }

int bn_check(long long R, int C, const char* what) {
  MUNIT_CHECK_ARG(R > 0 && R < (1ll << 40) / BN_MAX_C, "%s: R = %lld rows out of range", what, R);
  MUNIT_CHECK_ARG(C >= 4 && C <= BN_MAX_C && C % 4 == 0 && NT % (C / 4) == 0,
                  "%s: C = %d (a multiple of 4 up to %d whose quarter divides %d)", what, C, BN_MAX_C, NT);
  return MUNIT_OK;
}

// ---- batch norm across data-parallel ranks ---------------------------------------------------------------------------------
// W ranks hold R_local rows each of one joined batch of N = W * R_local rows.  Every rank reduces its own rows with the
// kernels above and writes the result into ITS row of an exchange buffer whose other rows it zeroes; the host sums the
// buffers of all ranks (an all-reduce: adding zeros is exact, so every rank then holds bitwise the same W rows, whatever
// order the collective adds in), and a finishing kernel merges the rows in rank order, in double.

// forward rows: xch[r][0..2C) = the local mean (high parts, low parts), xch[r][2C..3C) = M2 = sum of (x - local mean)^2
__global__ void bn_dp_stats_row_kernel(const float* __restrict__ part, int nb, int C, int W, int rank,
                                       const float* __restrict__ mean_local, float* __restrict__ xch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= W * 3 * C) return;
  const int row = i / (3 * C), j = i % (3 * C);
  float v = 0.f;
  if (row == rank) {
    if (j < 2 * C) {
      v = mean_local[j];
    } else {
      double s = 0.0;
      for (int b = 0; b < nb; ++b) s += (double)part[(long long)b * C + (j - 2 * C)];
      v = (float)s;
    }
  }
  xch[i] = v;
}

// the pairwise merge of W equal-sized parts (Chan et al.): mean = sum of the means / W, M2 = sum of the M2 + R_local * sum of
// (mean_r - mean)^2; rstd with the biased variance M2 / N, the running statistics with the unbiased M2 / (N - 1).  rstd is
// kept as two floats like the mean, rstd[c] + rstd[C + c]: with few rows per channel xhat^2 is close to 1, the backward's
// g - sum_g / N - xhat * sum_gx / N cancels to eps * rstd^2 of its terms, and a rounding of rstd to fp32 would be 1e-2 of dx
__global__ void bn_dp_combine_kernel(const float* __restrict__ xch, int W, long long R_local, int C, float eps, float momentum,
                                     float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ run_mean,
                                     float* __restrict__ run_var) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double ms = 0.0;
  for (int r = 0; r < W; ++r) {
    const float* row = xch + (long long)r * 3 * C;
    ms += (double)row[c] + (double)row[C + c];
  }
  const double mu = ms / (double)W;
  double m2 = 0.0, d2 = 0.0;
  for (int r = 0; r < W; ++r) {
    const float* row = xch + (long long)r * 3 * C;
    const double d = ((double)row[c] + (double)row[C + c]) - mu;
    m2 += (double)row[2 * C + c];
    d2 += d * d;
  }
  const double n = (double)W * (double)R_local;
  const double M2 = m2 + (double)R_local * d2;
  const float hi = (float)mu;
  mean[c] = hi;
  mean[C + c] = (float)(mu - (double)hi);
  const double rs = 1.0 / sqrt(M2 / n + (double)eps);
  const float rhi = (float)rs;
  rstd[c] = rhi;
  rstd[C + c] = (float)(rs - (double)rhi);
  run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * (float)mu;
  if (n > 1.0) run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)(M2 / (n - 1.0));
}

// The backward of the joined batch in double.  With two rows per channel (one per rank) xhat is +-1 / sqrt(1 + eps / var) and
// g - sum_g / N - xhat * sum_gx / N cancels to eps * rstd^2 of its terms, so every fp32 rounding on the way (of xhat, of a
// partial sum, of a total in the exchange buffer) would show 1e3 to 1e5 times larger in dx.  The local sums therefore
// accumulate in double and cross the ranks as two floats each (high part, low part), like the mean.

// part[b][0][c] = sum of g, part[b][1][c] = sum of g * xhat over the block's rows, in double; g = dy gated by y > 0
__global__ void bn_dp_bwd_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ y,
                                         const float* __restrict__ mean, const float* __restrict__ rstd, long long R, int C,
                                         int relu, double* __restrict__ part) {
  __shared__ double red[2 * 4 * NT];
  const int C4 = C >> 2, rl = NT / C4;
  const int c4 = threadIdx.x % C4, lane = threadIdx.x / C4;
  const long long per = (R + gridDim.x - 1) / gridDim.x;
  const long long r0 = (long long)blockIdx.x * per, r1 = r0 + per < R ? r0 + per : R;
  const f32x4 m = ld4(mean + 4 * c4), lo = ld4(mean + C + 4 * c4), rh = ld4(rstd + 4 * c4), rlo = ld4(rstd + C + 4 * c4);
  double sg[4] = {0.0, 0.0, 0.0, 0.0}, sgx[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long r = r0 + lane; r < r1; r += rl) {
    const long long o = r * C + 4 * c4;
    const f32x4 g = ld4(dy + o), xx = ld4(x + o);
    const f32x4 yy = relu ? ld4(y + o) : f32x4{1.f, 1.f, 1.f, 1.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double gk = yy[k] > 0.f ? (double)g[k] : 0.0;
      const double xh = (((double)xx[k] - (double)m[k]) - (double)lo[k]) * ((double)rh[k] + (double)rlo[k]);
      sg[k] += gk;
      sgx[k] += gk * xh;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    red[(0 * NT + lane * C4 + c4) * 4 + k] = sg[k];
    red[(1 * NT + lane * C4 + c4) * 4 + k] = sgx[k];
  }
  __syncthreads();
  if (lane == 0) {   // the row lanes in lane order
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double a = 0.0, b = 0.0;
      for (int l = 0; l < rl; ++l) {
        a += red[(0 * NT + l * C4 + c4) * 4 + k];
        b += red[(1 * NT + l * C4 + c4) * 4 + k];
      }
      part[((long long)blockIdx.x * 2 + 0) * C + 4 * c4 + k] = a;
      part[((long long)blockIdx.x * 2 + 1) * C + 4 * c4 + k] = b;
    }
  }
}

// backward rows of 4C floats: xch[r][0..C) = the local sum of g, xch[r][C..2C) = the local sum of g * xhat (high parts),
// xch[r][2C..4C) = their low parts
__global__ void bn_dp_bwd_row_kernel(const double* __restrict__ part, int nb, int C, int W, int rank, float* __restrict__ xch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= W * 4 * C) return;
  const int row = i / (4 * C), j = i % (4 * C);
  float v = 0.f;
  if (row == rank) {
    const int k = (j / C) & 1, c = j % C;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part[((long long)b * 2 + k) * C + c];
    const float hi = (float)s;
    v = j < 2 * C ? hi : (float)(s - (double)hi);
  }
  xch[i] = v;
}

// sums = the totals over all ranks in double (for dx); dbeta / dgamma = acc * old + the LOCAL sums (the optimizer's gradient
// exchange averages them like every other weight gradient)
__global__ void bn_dp_bwd_finish_kernel(const float* __restrict__ xch, int W, int rank, int C, float acc, double* __restrict__ sums,
                                        float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double a = 0.0, b = 0.0;
  for (int r = 0; r < W; ++r) {
    const float* row = xch + (long long)r * 4 * C;
    a += (double)row[c] + (double)row[2 * C + c];
    b += (double)row[C + c] + (double)row[3 * C + c];
  }
  sums[c] = a;
  sums[C + c] = b;
  const float* own = xch + (long long)rank * 4 * C;   // the high part IS the sum rounded to fp32
  if (dbeta) dbeta[c] = (acc != 0.f ? acc * dbeta[c] : 0.f) + own[c];
  if (dgamma) dgamma[c] = (acc != 0.f ? acc * dgamma[c] : 0.f) + own[C + c];
}

// dx = gamma * rstd * (g - sum_g / N - xhat * sum_gx / N), in double, rounded once
__global__ void bn_dp_bwd_dx_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ y,
                                    const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ rstd,
                                    const double* __restrict__ sums, long long R, int C, int relu, double inv_n,
                                    float* __restrict__ dx) {
  const int C4 = C >> 2;
  const long long total = R * C4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = 4 * (int)(i % C4);
    const f32x4 g = ld4(dy + 4 * i), xx = ld4(x + 4 * i), ga = ld4(gamma + c);
    const f32x4 yy = relu ? ld4(y + 4 * i) : f32x4{1.f, 1.f, 1.f, 1.f};
    const f32x4 m = ld4(mean + c), lo = ld4(mean + C + c), rh = ld4(rstd + c), rlo = ld4(rstd + C + c);
    f32x4 out;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double rs = (double)rh[k] + (double)rlo[k];
      const double xh = (((double)xx[k] - (double)m[k]) - (double)lo[k]) * rs;
      const double gk = yy[k] > 0.f ? (double)g[k] : 0.0;
      out[k] = (float)((double)ga[k] * rs * (gk - sums[c + k] * inv_n - xh * (sums[C + c + k] * inv_n)));
    }
    st4(dx + 4 * i, out);
  }
}

// the workspace of the cross-rank entry points: the partials (in double in the backward), then 2C doubles (the local mean of
// the forward as floats, the totals of the backward)
size_t bn_dp_part_bytes(int C) { return 2 * bn_part_bytes(C); }

constexpr int BN_DP_MAX_W = 64;

int bn_dp_check(long long R_local, int C, int W, int rank, const void* xch, size_t xch_floats, int per_row, const char* what,
                bool joined = true) {
  int rc = bn_check(R_local, C, what);
  if (rc) return rc;
  MUNIT_CHECK_ARG(W >= 1 && W <= BN_DP_MAX_W && rank >= 0 && rank < W, "%s: W = %d ranks (1..%d), rank %d", what, W,
                  BN_DP_MAX_W, rank);
  MUNIT_CHECK_ARG(!joined || (long long)W * R_local >= 2, "%s: the joined batch needs more than one value per channel (W * R_local = %lld)",
                  what, (long long)W * R_local);
  MUNIT_CHECK_ARG(xch != nullptr, "%s: null pointer (exchange buffer)", what);
  MUNIT_CHECK_ARG(xch_floats >= (size_t)W * per_row * C, "%s: exchange buffer of %zu floats < W * %d * C = %zu", what,
                  xch_floats, per_row, (size_t)W * per_row * C);
  return MUNIT_OK;
}

// ---- 2x2 / stride-2 max-pool -------------------------------------------------------------------------------------------
// one thread: one output pixel x 4 channels.  The first maximum in window order (0,0) (0,1) (1,0) (1,1) wins; a NaN counts as
// a maximum, as in torch's kernels.
__global__ void maxpool2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, unsigned char* __restrict__ idx, int B,
                                    int H, int W, int C, int Ho, int Wo) {
  const int C4 = C >> 2;
  const long long total = (long long)B * Ho * Wo * C4;
  for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
    long long r = o;
    const int c = 4 * (int)(r % C4); r /= C4;
    const int ow = (int)(r % Wo); r /= Wo;
    const int oh = (int)(r % Ho); r /= Ho;
    const long long b = r;
    const float* p = x + ((b * H + 2 * oh) * W + 2 * ow) * C + c;
    f32x4 best = ld4(p);
    unsigned win = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const f32x4 v = ld4(p + ((long long)(k >> 1) * W + (k & 1)) * C);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (v[j] > best[j] || v[j] != v[j]) {
          best[j] = v[j];
          win = (win & ~(0xFFu << (8 * j))) | ((unsigned)k << (8 * j));
        }
      }
    }
    st4(y + 4 * o, best);
    *reinterpret_cast<unsigned*>(idx + 4 * o) = win;
  }
}
// one thread: one INPUT pixel x 4 channels, written exactly once: dy where the pixel won its window, else 0
__global__ void maxpool2_bwd_kernel(const float* __restrict__ dy, const unsigned char* __restrict__ idx, float* __restrict__ dx,
                                    int B, int H, int W, int C, int Ho, int Wo) {
  const int C4 = C >> 2;
  const long long total = (long long)B * H * W * C4;
  for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
    long long r = o;
    const int c = 4 * (int)(r % C4); r /= C4;
    const int w = (int)(r % W); r /= W;
    const int h = (int)(r % H); r /= H;
    const long long b = r;
    f32x4 g = f32x4{0.f, 0.f, 0.f, 0.f};
    if ((h >> 1) < Ho && (w >> 1) < Wo) {
      const long long q = ((b * Ho + (h >> 1)) * Wo + (w >> 1)) * C + c;
      const unsigned win = *reinterpret_cast<const unsigned*>(idx + q);
      const unsigned k = (unsigned)((h & 1) * 2 + (w & 1));
      const f32x4 d = ld4(dy + q);
#pragma unroll
      for (int j = 0; j < 4; ++j) g[j] = ((win >> (8 * j)) & 0xFFu) == k ? d[j] : 0.f;
    }
    st4(dx + 4 * o, g);
  }
}

// ---- 16x16 average -------------------------------------------------------------------------------------------------------
// one block per image: C / 4 column groups x rl lanes; a lane sums the window positions p = lane, lane + rl, ... (p = h * 16 + w)
__global__ void avgpool16_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int C) {
  __shared__ f32x4 red[NT];
  const int C4 = C >> 2, rl = NT / C4;
  const int c4 = threadIdx.x % C4, lane = threadIdx.x / C4;
  const long long b = blockIdx.x;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int p = lane; p < 256; p += rl) acc += ld4(x + ((b * H + (p >> 4)) * W + (p & 15)) * C + 4 * c4);
  const f32x4 s = block_rows_sum(acc, c4, lane, C4, rl, red);
  if (lane == 0) st4(y + b * C + 4 * c4, s * (1.f / 256.f));
}
__global__ void avgpool16_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int B, int H, int W, int C) {
  const int C4 = C >> 2;
  const long long total = (long long)B * H * W * C4;
  for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
    long long r = o;
    const int c = 4 * (int)(r % C4); r /= C4;
    const int w = (int)(r % W); r /= W;
    const int h = (int)(r % H); r /= H;
    const long long b = r;
    const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
    st4(dx + 4 * o, (h < 16 && w < 16) ? ld4(dy + b * C + c) * (1.f / 256.f) : z);
  }
}

int pool_check(int B, int H, int W, int C, const char* what) {
  MUNIT_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "%s: bad shape (B, H, W > 0; C %% 4 == 0)", what);
  MUNIT_CHECK_ARG((long long)B * H * W * C < (1ll << 40), "%s: too large", what);
  return MUNIT_OK;
}

}  // namespace

extern "C" size_t munit_batchnorm_workspace_bytes(int C) {
  if (C <= 0) return 0;
  return bn_part_bytes(C) + align_up((size_t)2 * C * sizeof(float), 256);
}

extern "C" int munit_batchnorm_fwd(const float* x, float* y, float* mean, float* rstd, float* running_mean, float* running_var,
                                   long long R, int C, const float* gamma, const float* beta, int relu, int eval, float eps,
                                   float momentum, void* ws, size_t ws_bytes, munit_stream_t stream) {
  int rc = bn_check(R, C, "batchnorm_fwd");
  if (rc) return rc;
  MUNIT_CHECK_ARG(x && y && gamma && beta && running_mean && running_var, "batchnorm_fwd: null pointer");
  MUNIT_CHECK_ARG((relu == 0 || relu == 1) && (eval == 0 || eval == 1) && eps > 0.f, "batchnorm_fwd: bad relu / eval / eps");
  hipStream_t st = (hipStream_t)stream;
  const unsigned ga = grid_for(R * (C / 4));
  if (eval) {
    hipLaunchKernelGGL(bn_apply_kernel, dim3(ga), dim3(NT), 0, st, x, (const float*)running_mean, (const float*)running_var,
                       gamma, beta, R, C, relu, 1, eps, y);
    MUNIT_CHECK_LAUNCH("batchnorm_fwd (eval)");
    return MUNIT_OK;
  }
  MUNIT_CHECK_ARG(mean && rstd && ws, "batchnorm_fwd: null pointer (mean / rstd / ws)");
  MUNIT_CHECK_ARG(R >= 2, "batchnorm_fwd: training mode needs more than one value per channel (R = %lld)", R);
  MUNIT_CHECK_ARG(momentum >= 0.f && momentum <= 1.f, "batchnorm_fwd: momentum %g", (double)momentum);
  if (ws_bytes < munit_batchnorm_workspace_bytes(C)) {
    munit_set_error("batchnorm_fwd: workspace %zu < %zu", ws_bytes, munit_batchnorm_workspace_bytes(C));
    return MUNIT_ERR_WORKSPACE;
  }
  float* part = reinterpret_cast<float*>(ws);
  const int nb = bn_blocks(R, C);
  const dim3 gf((C + NT - 1) / NT);
  hipLaunchKernelGGL(bn_partial_kernel, dim3(nb), dim3(NT), 0, st, x, (const float*)nullptr, R, C, 0, part);
  MUNIT_CHECK_LAUNCH("batchnorm_fwd (sum)");
  hipLaunchKernelGGL(bn_finish_kernel, gf, dim3(NT), 0, st, x, (const float*)part, nb, R, C, 0, eps, momentum, mean, rstd,
                     (float*)nullptr, (float*)nullptr);
  MUNIT_CHECK_LAUNCH("batchnorm_fwd (mean)");
  hipLaunchKernelGGL(bn_partial_kernel, dim3(nb), dim3(NT), 0, st, x, (const float*)mean, R, C, 1, part);
  MUNIT_CHECK_LAUNCH("batchnorm_fwd (squares)");
  hipLaunchKernelGGL(bn_finish_kernel, gf, dim3(NT), 0, st, x, (const float*)part, nb, R, C, 1, eps, momentum, mean, rstd,
                     running_mean, running_var);
  MUNIT_CHECK_LAUNCH("batchnorm_fwd (rstd)");
  hipLaunchKernelGGL(bn_apply_kernel, dim3(ga), dim3(NT), 0, st, x, (const float*)mean, (const float*)rstd, gamma, beta, R, C,
                     relu, 0, eps, y);
  MUNIT_CHECK_LAUNCH("batchnorm_fwd (apply)");
  return MUNIT_OK;
}

extern "C" int munit_batchnorm_bwd(const float* x, const float* dy, const float* y, const float* gamma, const float* mean,
                                   const float* rstd, float* dx, float* dgamma, float* dbeta, float acc, long long R, int C,
                                   int relu, void* ws, size_t ws_bytes, munit_stream_t stream) {
  int rc = bn_check(R, C, "batchnorm_bwd");
  if (rc) return rc;
  MUNIT_CHECK_ARG(x && dy && gamma && mean && rstd && dx && ws, "batchnorm_bwd: null pointer");
  MUNIT_CHECK_ARG(relu == 0 || (relu == 1 && y), "batchnorm_bwd: the ReLU branch needs y");
  MUNIT_CHECK_ARG(acc == 0.f || acc == 1.f, "batchnorm_bwd: acc must be 0 or 1");
  if (ws_bytes < munit_batchnorm_workspace_bytes(C)) {
    munit_set_error("batchnorm_bwd: workspace %zu < %zu", ws_bytes, munit_batchnorm_workspace_bytes(C));
    return MUNIT_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  float* part = reinterpret_cast<float*>(ws);
  float* sums = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + bn_part_bytes(C));
  const int nb = bn_blocks(R, C);
  hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3(nb), dim3(NT), 0, st, x, dy, y, mean, rstd, R, C, relu, part);
  MUNIT_CHECK_LAUNCH("batchnorm_bwd (sums)");
  hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3((C + NT - 1) / NT), dim3(NT), 0, st, (const float*)part, nb, C, acc, sums,
                     dgamma, dbeta);
  MUNIT_CHECK_LAUNCH("batchnorm_bwd (finish)");
  hipLaunchKernelGGL(bn_bwd_dx_kernel, dim3(grid_for(R * (C / 4))), dim3(NT), 0, st, x, dy, y, gamma, mean, rstd,
                     (const float*)sums, R, C, relu, (float)(1.0 / (double)R), dx);
  MUNIT_CHECK_LAUNCH("batchnorm_bwd (dx)");
  return MUNIT_OK;
}

extern "C" size_t munit_batchnorm_dp_workspace_bytes(int C) {
  if (C <= 0) return 0;
  return bn_dp_part_bytes(C) + align_up((size_t)2 * C * sizeof(double), 256);
}

extern "C" int munit_batchnorm_dp_stats_local(const float* x, long long R_local, int C, int W, int rank, float* xch,
                                              size_t xch_floats, void* ws, size_t ws_bytes, munit_stream_t stream) {
  int rc = bn_dp_check(R_local, C, W, rank, xch, xch_floats, 3, "batchnorm_dp_stats_local");
  if (rc) return rc;
  MUNIT_CHECK_ARG(x && ws, "batchnorm_dp_stats_local: null pointer");
  if (ws_bytes < munit_batchnorm_dp_workspace_bytes(C)) {
    munit_set_error("batchnorm_dp_stats_local: workspace %zu < %zu", ws_bytes, munit_batchnorm_dp_workspace_bytes(C));
    return MUNIT_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  float* part = reinterpret_cast<float*>(ws);
  float* mean_local = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + bn_dp_part_bytes(C));
  const int nb = bn_blocks(R_local, C);
  hipLaunchKernelGGL(bn_partial_kernel, dim3(nb), dim3(NT), 0, st, x, (const float*)nullptr, R_local, C, 0, part);
  MUNIT_CHECK_LAUNCH("batchnorm_dp_stats_local (sum)");
  hipLaunchKernelGGL(bn_finish_kernel, dim3((C + NT - 1) / NT), dim3(NT), 0, st, x, (const float*)part, nb, R_local, C, 0, 0.f,
                     0.f, mean_local, (float*)nullptr, (float*)nullptr, (float*)nullptr);
  MUNIT_CHECK_LAUNCH("batchnorm_dp_stats_local (mean)");
  hipLaunchKernelGGL(bn_partial_kernel, dim3(nb), dim3(NT), 0, st, x, (const float*)mean_local, R_local, C, 1, part);
  MUNIT_CHECK_LAUNCH("batchnorm_dp_stats_local (squares)");
  hipLaunchKernelGGL(bn_dp_stats_row_kernel, dim3((W * 3 * C + NT - 1) / NT), dim3(NT), 0, st, (const float*)part, nb, C, W, rank,
                     (const float*)mean_local, xch);
  MUNIT_CHECK_LAUNCH("batchnorm_dp_stats_local (row)");
  return MUNIT_OK;
}

extern "C" int munit_batchnorm_dp_fwd_apply(const float* x, float* y, float* mean, float* rstd, float* running_mean,
                                            float* running_var, long long R_local, int C, int W, const float* xch,
                                            size_t xch_floats, const float* gamma, const float* beta, int relu, float eps,
                                            float momentum, munit_stream_t stream) {
  // N >= 2 is stats_local's to refuse (every pass begins there); one row merges to M2 = 0 and leaves running_var alone
  int rc = bn_dp_check(R_local, C, W, 0, xch, xch_floats, 3, "batchnorm_dp_fwd_apply", false);
  if (rc) return rc;
  MUNIT_CHECK_ARG(x && y && mean && rstd && gamma && beta && running_mean && running_var, "batchnorm_dp_fwd_apply: null pointer");
  MUNIT_CHECK_ARG((relu == 0 || relu == 1) && eps > 0.f, "batchnorm_dp_fwd_apply: bad relu / eps");
  MUNIT_CHECK_ARG(momentum >= 0.f && momentum <= 1.f, "batchnorm_dp_fwd_apply: momentum %g", (double)momentum);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bn_dp_combine_kernel, dim3((C + NT - 1) / NT), dim3(NT), 0, st, xch, W, R_local, C, eps, momentum, mean, rstd,
                     running_mean, running_var);
  MUNIT_CHECK_LAUNCH("batchnorm_dp_fwd_apply (combine)");
  // y takes the high part of rstd alone (6e-8 of y, inside the forward's bound); the low part is for the backward's xhat
  hipLaunchKernelGGL(bn_apply_kernel, dim3(grid_for(R_local * (C / 4))), dim3(NT), 0, st, x, (const float*)mean,
                     (const float*)rstd, gamma, beta, R_local, C, relu, 0, eps, y);
  MUNIT_CHECK_LAUNCH("batchnorm_dp_fwd_apply (apply)");
  return MUNIT_OK;
}

extern "C" int munit_batchnorm_dp_bwd_local(const float* x, const float* dy, const float* y, const float* mean,
                                            const float* rstd, long long R_local, int C, int relu, int W, int rank, float* xch,
                                            size_t xch_floats, void* ws, size_t ws_bytes, munit_stream_t stream) {
  int rc = bn_dp_check(R_local, C, W, rank, xch, xch_floats, 4, "batchnorm_dp_bwd_local");
  if (rc) return rc;
  MUNIT_CHECK_ARG(x && dy && mean && rstd && ws, "batchnorm_dp_bwd_local: null pointer");
  MUNIT_CHECK_ARG(relu == 0 || (relu == 1 && y), "batchnorm_dp_bwd_local: the ReLU branch needs y");
  if (ws_bytes < munit_batchnorm_dp_workspace_bytes(C)) {
    munit_set_error("batchnorm_dp_bwd_local: workspace %zu < %zu", ws_bytes, munit_batchnorm_dp_workspace_bytes(C));
    return MUNIT_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(ws);
  const int nb = bn_blocks(R_local, C);
  hipLaunchKernelGGL(bn_dp_bwd_partial_kernel, dim3(nb), dim3(NT), 0, st, x, dy, y, mean, rstd, R_local, C, relu, part);
  MUNIT_CHECK_LAUNCH("batchnorm_dp_bwd_local (sums)");
  hipLaunchKernelGGL(bn_dp_bwd_row_kernel, dim3((W * 4 * C + NT - 1) / NT), dim3(NT), 0, st, (const double*)part, nb, C, W, rank,
                     xch);
  MUNIT_CHECK_LAUNCH("batchnorm_dp_bwd_local (row)");
  return MUNIT_OK;
}

extern "C" int munit_batchnorm_dp_bwd_finish(const float* x, const float* dy, const float* y, const float* gamma,
                                             const float* mean, const float* rstd, float* dx, float* dgamma, float* dbeta,
                                             float acc, long long R_local, int C, int relu, int W, int rank, const float* xch,
                                             size_t xch_floats, void* ws, size_t ws_bytes, munit_stream_t stream) {
  int rc = bn_dp_check(R_local, C, W, rank, xch, xch_floats, 4, "batchnorm_dp_bwd_finish");
  if (rc) return rc;
  MUNIT_CHECK_ARG(x && dy && gamma && mean && rstd && dx && ws, "batchnorm_dp_bwd_finish: null pointer");
  MUNIT_CHECK_ARG(relu == 0 || (relu == 1 && y), "batchnorm_dp_bwd_finish: the ReLU branch needs y");
  MUNIT_CHECK_ARG(acc == 0.f || acc == 1.f, "batchnorm_dp_bwd_finish: acc must be 0 or 1");
  if (ws_bytes < munit_batchnorm_dp_workspace_bytes(C)) {
    munit_set_error("batchnorm_dp_bwd_finish: workspace %zu < %zu", ws_bytes, munit_batchnorm_dp_workspace_bytes(C));
    return MUNIT_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  double* sums = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + bn_dp_part_bytes(C));
  hipLaunchKernelGGL(bn_dp_bwd_finish_kernel, dim3((C + NT - 1) / NT), dim3(NT), 0, st, xch, W, rank, C, acc, sums, dgamma, dbeta);
  MUNIT_CHECK_LAUNCH("batchnorm_dp_bwd_finish (finish)");
  hipLaunchKernelGGL(bn_dp_bwd_dx_kernel, dim3(grid_for(R_local * (C / 4))), dim3(NT), 0, st, x, dy, y, gamma, mean, rstd,
                     (const double*)sums, R_local, C, relu, 1.0 / ((double)W * (double)R_local), dx);
  MUNIT_CHECK_LAUNCH("batchnorm_dp_bwd_finish (dx)");
  return MUNIT_OK;
}

extern "C" int munit_maxpool2_fwd(const float* x, float* y, unsigned char* idx, int B, int H, int W, int C,
                                  munit_stream_t stream) {
  int rc = pool_check(B, H, W, C, "maxpool2_fwd");
  if (rc) return rc;
  MUNIT_CHECK_ARG(x && y && idx && H >= 2 && W >= 2, "maxpool2_fwd: bad args (H, W >= 2)");
  const int Ho = H / 2, Wo = W / 2;
  hipLaunchKernelGGL(maxpool2_fwd_kernel, dim3(grid_for((long long)B * Ho * Wo * (C / 4))), dim3(NT), 0, (hipStream_t)stream, x,
                     y, idx, B, H, W, C, Ho, Wo);
  MUNIT_CHECK_LAUNCH("maxpool2_fwd");
  return MUNIT_OK;
}

extern "C" int munit_maxpool2_bwd(const float* dy, const unsigned char* idx, float* dx, int B, int H, int W, int C,
                                  munit_stream_t stream) {
  int rc = pool_check(B, H, W, C, "maxpool2_bwd");
  if (rc) return rc;
  MUNIT_CHECK_ARG(dy && idx && dx && H >= 2 && W >= 2, "maxpool2_bwd: bad args (H, W >= 2)");
  hipLaunchKernelGGL(maxpool2_bwd_kernel, dim3(grid_for((long long)B * H * W * (C / 4))), dim3(NT), 0, (hipStream_t)stream, dy,
                     idx, dx, B, H, W, C, H / 2, W / 2);
  MUNIT_CHECK_LAUNCH("maxpool2_bwd");
  return MUNIT_OK;
}

extern "C" int munit_avgpool16_fwd(const float* x, float* y, int B, int H, int W, int C, munit_stream_t stream) {
  int rc = pool_check(B, H, W, C, "avgpool16_fwd");
  if (rc) return rc;
  MUNIT_CHECK_ARG(x && y, "avgpool16_fwd: null pointer");
  MUNIT_CHECK_ARG(H >= 16 && H <= 31 && W >= 16 && W <= 31, "avgpool16_fwd: the map must be 16..31 on both axes, got %dx%d", H, W);
  MUNIT_CHECK_ARG(C <= BN_MAX_C && NT % (C / 4) == 0, "avgpool16_fwd: C = %d (its quarter must divide %d)", C, NT);
  hipLaunchKernelGGL(avgpool16_fwd_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, x, y, H, W, C);
  MUNIT_CHECK_LAUNCH("avgpool16_fwd");
  return MUNIT_OK;
}

extern "C" int munit_avgpool16_bwd(const float* dy, float* dx, int B, int H, int W, int C, munit_stream_t stream) {
  int rc = pool_check(B, H, W, C, "avgpool16_bwd");
  if (rc) return rc;
  MUNIT_CHECK_ARG(dy && dx, "avgpool16_bwd: null pointer");
  MUNIT_CHECK_ARG(H >= 16 && H <= 31 && W >= 16 && W <= 31, "avgpool16_bwd: the map must be 16..31 on both axes, got %dx%d", H, W);
  hipLaunchKernelGGL(avgpool16_bwd_kernel, dim3(grid_for((long long)B * H * W * (C / 4))), dim3(NT), 0, (hipStream_t)stream, dy,
                     dx, B, H, W, C);
  MUNIT_CHECK_LAUNCH("avgpool16_bwd");
  return MUNIT_OK;
}
