// Kernels of the domain-invariant perceptual loss (vgg_w; scripts/trainer.py:618-636, scripts/utils.py:1051-1063): the input
// transform of the frozen VGG16 and the loss on its relu5_3 features, mean((IN(f) - IN(t))^2) with IN = InstanceNorm2d(512,
// affine=False).  The network's convolutions run through munit_conv2d_*, its pools through munit_maxpool2_*.  No atomics: every
// result is bitwise reproducible.
#include "common.h"

namespace {

constexpr int NT = 256;

unsigned grid_for(long long n) { return (unsigned)std::max<long long>(1, std::min<long long>((n + NT - 1) / NT, 16384)); }

// Caffe VGG means of the B, G, R planes (utils.py:1059-1061)
__constant__ float c_bgr_mean[3] = {103.939f, 116.779f, 123.680f};

// y[p][c] = (x[p][2 - c] + 1) * 255 * 0.5 - mean[c]: the reference's operations in its order, so the result is torch's bit for bit
__global__ void vgg_input_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % 3);
    const float v = x[i - c + (2 - c)];
    y[i] = (v + 1.f) * 255.f * 0.5f - c_bgr_mean[c];
  }
}
__global__ void vgg_input_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % 3);
    dx[i] = 127.5f * dy[i - c + (2 - c)];
  }
}

// ---------------------------------------------------------------------------------------
// in_mse.  A block = (sample b, slice of SL channels): QB channel quads x PL pixel lanes, so a pixel's slice is one 128-byte
// line read by 8 lanes as float4s (norm.hip's channel-sliced layout with a narrower slice: the planes here are small, 4 ..
// 4096 pixels, and the grid B x C / 32 has to fill the chip without a pixel split).  Statistics are summed in fp64 relative to a
// pivot (the plane's first pixel), per thread over its pixels, then over the pixel lanes in lane order.
// ---------------------------------------------------------------------------------------
constexpr int SL = 32;
constexpr int QB = SL / 4;
constexpr int PL = NT / QB;
constexpr double IN_EPS = 1e-5;

// Sum v[0..3] over the pixel lanes of the thread's quad, in lane order.  The totals are valid in threads < QB (quad = tid).
__device__ inline void sum_lanes(double (&v)[4], double* red, int tid) {
  __syncthreads();   // the last use of red is over
#pragma unroll
  for (int k = 0; k < 4; ++k) red[tid * 4 + k] = v[k];
  __syncthreads();
  if (tid < QB) {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int pl = 0; pl < PL; ++pl) {
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] += red[(pl * QB + tid) * 4 + k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = a[k];
  }
}

// stats[m][b][c][2] = (mean, 1 / sqrt(var + eps)) of map m (0: f, 1: t); partial[b][slice] = sum over the slice of (nf - nt)^2
__global__ __launch_bounds__(NT) void in_mse_fwd_kernel(const float* __restrict__ f, const float* __restrict__ t, int HW, int C,
                                                        float* __restrict__ stats, double* __restrict__ partial) {
  __shared__ double red[NT * 4];
  __shared__ float s_stat[2][SL][2];
  __shared__ double s_quad[QB];
  const int tid = threadIdx.x, q = tid % QB, pl = tid / QB;
  const int b = blockIdx.y, B = gridDim.y, c = blockIdx.x * SL + q * 4;
  const bool on = c < C;
  const size_t base = (size_t)b * HW * C + c;
  for (int m = 0; m < 2; ++m) {
    const float* x = (m == 0 ? f : t) + base;
    const f32x4 piv = on ? ld4(x) : f32x4{0.f, 0.f, 0.f, 0.f};
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    if (on)
      for (int p = pl; p < HW; p += PL) {
        const f32x4 v = ld4(x + (size_t)p * C);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double d = (double)v[k] - (double)piv[k];
          s1[k] += d;
          s2[k] += d * d;
        }
      }
    sum_lanes(s1, red, tid);
    sum_lanes(s2, red, tid);
    if (tid < QB) {   // tid is the quad: channels c .. c + 3 of this thread (pl == 0)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double md = s1[k] / HW;
        double var = s2[k] / HW - md * md;
        var = var > 0.0 ? var : 0.0;
        const float mean = (float)((double)piv[k] + md), rstd = (float)(1.0 / sqrt(var + IN_EPS));
        s_stat[m][tid * 4 + k][0] = mean;
        s_stat[m][tid * 4 + k][1] = rstd;
        if (on) {
          float* st = stats + (((size_t)m * B + b) * C + c + k) * 2;
          st[0] = mean;
          st[1] = rstd;
        }
      }
    }
  }
  __syncthreads();
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (on)
    for (int p = pl; p < HW; p += PL) {
      const f32x4 vf = ld4(f + base + (size_t)p * C), vt = ld4(t + base + (size_t)p * C);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float nf = (vf[k] - s_stat[0][q * 4 + k][0]) * s_stat[0][q * 4 + k][1];
        const float nt = (vt[k] - s_stat[1][q * 4 + k][0]) * s_stat[1][q * 4 + k][1];
        const float d = nf - nt;
        acc[k] += (double)d * (double)d;
      }
    }
  sum_lanes(acc, red, tid);
  if (tid < QB) s_quad[tid] = ((acc[0] + acc[1]) + acc[2]) + acc[3];
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < QB; ++i) s += s_quad[i];
    partial[(size_t)b * gridDim.x + blockIdx.x] = s;
  }
}

// out[0] = (sum of partial[0..n)) / count: thread i adds partial[i], partial[i + NT], ... in order, thread 0 the NT sums in order
__global__ __launch_bounds__(NT) void in_mse_final_kernel(const double* __restrict__ partial, int n, double count,
                                                          float* __restrict__ out) {
  __shared__ double red[NT];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += NT) s += partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int i = 0; i < NT; ++i) tot += red[i];
    out[0] = (float)(tot / count);
  }
}

// df = (g - mean_hw(g) - nf * mean_hw(g * nf)) * rstd_f with g = 2 gout (nf - nt) / count; nf, nt by the forward's expression
__global__ __launch_bounds__(NT) void in_mse_bwd_kernel(const float* __restrict__ f, const float* __restrict__ t,
                                                        const float* __restrict__ stats, int HW, int C, double count,
                                                        const float* __restrict__ gout, float* __restrict__ df) {
  __shared__ double red[NT * 4];
  __shared__ float s_mean[2][SL];
  const int tid = threadIdx.x, q = tid % QB, pl = tid / QB;
  const int b = blockIdx.y, B = gridDim.y, c = blockIdx.x * SL + q * 4;
  const bool on = c < C;
  const size_t base = (size_t)b * HW * C + c;
  const float scale = (float)(2.0 * (double)gout[0] / count);
  float mf[4] = {0.f, 0.f, 0.f, 0.f}, rf[4] = {0.f, 0.f, 0.f, 0.f}, mt[4] = {0.f, 0.f, 0.f, 0.f}, rt[4] = {0.f, 0.f, 0.f, 0.f};
  if (on) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float* sf = stats + ((size_t)b * C + c + k) * 2;
      const float* st = stats + (((size_t)B + b) * C + c + k) * 2;
      mf[k] = sf[0]; rf[k] = sf[1];
      mt[k] = st[0]; rt[k] = st[1];
    }
  }
  double sg[4] = {0.0, 0.0, 0.0, 0.0}, sgn[4] = {0.0, 0.0, 0.0, 0.0};
  if (on)
    for (int p = pl; p < HW; p += PL) {
      const f32x4 vf = ld4(f + base + (size_t)p * C), vt = ld4(t + base + (size_t)p * C);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float nf = (vf[k] - mf[k]) * rf[k];
        const float nt = (vt[k] - mt[k]) * rt[k];
        const float g = scale * (nf - nt);
        sg[k] += (double)g;
        sgn[k] += (double)g * (double)nf;
      }
    }
  sum_lanes(sg, red, tid);
  sum_lanes(sgn, red, tid);
  if (tid < QB) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s_mean[0][tid * 4 + k] = (float)(sg[k] / HW);
      s_mean[1][tid * 4 + k] = (float)(sgn[k] / HW);
    }
  }
  __syncthreads();
  if (!on) return;
  for (int p = pl; p < HW; p += PL) {
    const f32x4 vf = ld4(f + base + (size_t)p * C), vt = ld4(t + base + (size_t)p * C);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float nf = (vf[k] - mf[k]) * rf[k];
      const float nt = (vt[k] - mt[k]) * rt[k];
      const float g = scale * (nf - nt);
      o[k] = (g - s_mean[0][q * 4 + k] - nf * s_mean[1][q * 4 + k]) * rf[k];
    }
    st4(df + base + (size_t)p * C, o);
  }
}

int in_mse_slices(int C) { return (C + SL - 1) / SL; }

bool in_mse_shape_ok(int B, int HW, int C) {
  return B > 0 && B <= 65535 && HW > 0 && C > 0 && C % 4 == 0 && (long long)B * HW * C < (1ll << 40);
}

}  // namespace

extern "C" int munit_vgg_input_fwd(const float* x, float* y, size_t npix, munit_stream_t stream) {
  MUNIT_CHECK_ARG(x && y && x != y, "vgg_input_fwd: null or aliased pointer");
  if (npix == 0) return MUNIT_OK;
  const long long n = 3ll * (long long)npix;
  hipLaunchKernelGGL(vgg_input_fwd_kernel, dim3(grid_for(n)), dim3(NT), 0, (hipStream_t)stream, x, y, n);
  MUNIT_CHECK_LAUNCH("vgg_input_fwd");
  return MUNIT_OK;
}

extern "C" int munit_vgg_input_bwd(const float* dy, float* dx, size_t npix, munit_stream_t stream) {
  MUNIT_CHECK_ARG(dy && dx && dy != dx, "vgg_input_bwd: null or aliased pointer");
  if (npix == 0) return MUNIT_OK;
  const long long n = 3ll * (long long)npix;
  hipLaunchKernelGGL(vgg_input_bwd_kernel, dim3(grid_for(n)), dim3(NT), 0, (hipStream_t)stream, dy, dx, n);
  MUNIT_CHECK_LAUNCH("vgg_input_bwd");
  return MUNIT_OK;
}

extern "C" size_t munit_in_mse_workspace_bytes(int B, int C) {
  if (B <= 0 || C <= 0) return 0;
  return align_up((size_t)B * in_mse_slices(C) * sizeof(double), 256);
}

extern "C" int munit_in_mse_fwd(const float* f, const float* t, int B, int HW, int C, float* out, float* stats, void* ws,
                                size_t ws_bytes, munit_stream_t stream) {
  MUNIT_CHECK_ARG(f && t && out && stats && ws, "in_mse_fwd: null pointer");
  MUNIT_CHECK_ARG(in_mse_shape_ok(B, HW, C), "in_mse_fwd: bad shape B=%d HW=%d C=%d (C %% 4 == 0, B <= 65535)", B, HW, C);
  const size_t need = munit_in_mse_workspace_bytes(B, C);
  if (ws_bytes < need) {
    munit_set_error("in_mse_fwd: workspace %zu < %zu", ws_bytes, need);
    return MUNIT_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  double* partial = reinterpret_cast<double*>(ws);
  const int ns = in_mse_slices(C);
  hipLaunchKernelGGL(in_mse_fwd_kernel, dim3(ns, B), dim3(NT), 0, st, f, t, HW, C, stats, partial);
  MUNIT_CHECK_LAUNCH("in_mse_fwd");
  hipLaunchKernelGGL(in_mse_final_kernel, dim3(1), dim3(NT), 0, st, partial, B * ns, (double)B * HW * C, out);
  MUNIT_CHECK_LAUNCH("in_mse_final");
  return MUNIT_OK;
}

extern "C" int munit_in_mse_bwd(const float* f, const float* t, const float* stats, int B, int HW, int C, const float* gout,
                                float* df, munit_stream_t stream) {
  MUNIT_CHECK_ARG(f && t && stats && gout && df, "in_mse_bwd: null pointer");
  MUNIT_CHECK_ARG(df != f && df != t, "in_mse_bwd: df aliases an input");
  MUNIT_CHECK_ARG(in_mse_shape_ok(B, HW, C), "in_mse_bwd: bad shape B=%d HW=%d C=%d (C %% 4 == 0, B <= 65535)", B, HW, C);
  hipLaunchKernelGGL(in_mse_bwd_kernel, dim3(in_mse_slices(C), B), dim3(NT), 0, (hipStream_t)stream, f, t, stats, HW, C,
                     (double)B * HW * C, gout, df);
  MUNIT_CHECK_LAUNCH("in_mse_bwd");
  return MUNIT_OK;
}
