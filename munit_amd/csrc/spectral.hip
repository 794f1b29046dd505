// Spectral normalisation of the discriminators' convolutions (dis.norm: sn, scripts/networks.py:885-942): the power
// iteration over all normalised layers of a module in four launches, the scale-bias-activation that follows the raw
// convolution (conv(x, W / sigma) = conv(x, W) / sigma), its backward with the two reductions the weight gradient needs,
// and the rank-1 correction of that gradient.  fp32 throughout, every reduction in a fixed order (no atomics).
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int SN_ROWS1 = 32;       // rows of W per block of the W^T u partials, at least
constexpr int SN_CHUNKS = 16;      // ... and at most this many row chunks per layer
constexpr int SN_ROWS2 = 4;        // rows of W per block of W v (one per wave)
constexpr int SN_MAX_N = 8192;     // columns of W the third launch keeps in LDS (32 KiB)
constexpr int SN_BWD_PARTS = 512;  // blocks of the backward's first stage, at most
constexpr float SN_EPS = 1e-12f;   // l2normalize's eps (networks.py:881)

__host__ __device__ inline int sn_rows_per_chunk(int O) {
  const int r = (O + SN_CHUNKS - 1) / SN_CHUNKS;
  return r > SN_ROWS1 ? r : SN_ROWS1;
}
__host__ __device__ inline int sn_chunks(int O) { const int r = sn_rows_per_chunk(O); return (O + r - 1) / r; }

// floats of workspace per layer: the W^T u partials [chunk][column], then s = W v
inline size_t sn_layer_floats(int max_O, int max_N) {
  return align_up((size_t)sn_chunks(max_O) * max_N, 64) + align_up((size_t)max_O, 64);
}

__device__ inline float block_sum(float v, float* red) {      // all threads get the total; red: NT / 64 floats
  v = wave_sum(v);
  __syncthreads();                                             // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// column m of the weight's memory order [KH][KW][I] -> column of the reference's (i, kh, kw) order
__device__ inline int sn_ref_col(int m, int KHW, int I) {
  const int i = m % I, k = m / I;
  return i * KHW + k;
}

__device__ inline bool sn_layer_ok(const munit_sn_item& it, int max_O, int max_N) {
  const int N = it.KH * it.KW * it.I;
  return it.O >= 1 && N >= 1 && it.O <= max_O && N <= max_N;
}

// launch 1: partial[chunk][m] = sum over the chunk's rows o of W[o][m] u[o]      grid (column tiles, chunks, layers)
__global__ __launch_bounds__(NT) void sn_wtu_kernel(const munit_sn_item* __restrict__ items, int max_O, int max_N,
                                                    float* __restrict__ ws, size_t layer_floats) {
  const munit_sn_item it = items[blockIdx.z];
  if (!sn_layer_ok(it, max_O, max_N)) return;
  const int N = it.KH * it.KW * it.I;
  const int rows = sn_rows_per_chunk(it.O), chunk = blockIdx.y;
  const int m = blockIdx.x * NT + threadIdx.x;
  if (chunk >= sn_chunks(it.O) || m >= N) return;
  const int o0 = chunk * rows, o1 = min(it.O, o0 + rows);
  const float* w = it.w + (size_t)o0 * N + m;
  float acc = 0.f;
  for (int o = o0; o < o1; ++o, w += N) acc += *w * it.u[o];
  ws[blockIdx.z * layer_floats + (size_t)chunk * N + m] = acc;
}

// launch 2: t[m] = sum of the partials in chunk order, left in chunk 0's row (a thread reads and writes its own column only)
//                                                                                grid (column tiles, layers)
__global__ __launch_bounds__(NT) void sn_t_kernel(const munit_sn_item* __restrict__ items, int max_O, int max_N,
                                                  float* __restrict__ ws, size_t layer_floats) {
  const munit_sn_item it = items[blockIdx.y];
  if (!sn_layer_ok(it, max_O, max_N)) return;
  const int N = it.KH * it.KW * it.I;
  const int m = blockIdx.x * NT + threadIdx.x;
  if (m >= N) return;
  float* lws = ws + blockIdx.y * layer_floats;
  const int chunks = sn_chunks(it.O);
  float t = 0.f;
  for (int c = 0; c < chunks; ++c) t += lws[(size_t)c * N + m];
  lws[m] = t;
}

// launch 3: v = t / (|t| + eps) (every block of a layer forms the same v in LDS; the first writes it, in the reference's
// column order), s[o] = W[o] . v for this block's SN_ROWS2 rows                 grid (row blocks, layers)
__global__ __launch_bounds__(NT) void sn_wv_kernel(const munit_sn_item* __restrict__ items, int max_O, int max_N,
                                                   float* __restrict__ ws, size_t layer_floats, size_t s_off) {
  __shared__ float vs[SN_MAX_N];
  __shared__ float red[NT / 64];
  const munit_sn_item it = items[blockIdx.y];
  if (!sn_layer_ok(it, max_O, max_N)) return;
  const int N = it.KH * it.KW * it.I, KHW = it.KH * it.KW;
  const int o0 = blockIdx.x * SN_ROWS2;
  if (o0 >= it.O) return;
  float* lws = ws + blockIdx.y * layer_floats;
  float sq = 0.f;
  for (int m = threadIdx.x; m < N; m += NT) {
    const float t = lws[m];
    vs[m] = t;
    sq += t * t;
  }
  const float norm = sqrtf(block_sum(sq, red)) + SN_EPS;
  for (int m = threadIdx.x; m < N; m += NT) {
    const float v = vs[m] / norm;
    vs[m] = v;
    if (blockIdx.x == 0) it.v[sn_ref_col(m, KHW, it.I)] = v;
  }
  __syncthreads();
  float* s = lws + s_off;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int r = wave; r < SN_ROWS2; r += NT / 64) {
    const int o = o0 + r;
    if (o >= it.O) break;
    const float* w = it.w + (size_t)o * N;
    float acc = 0.f;
    for (int m = lane; m < N; m += 64) acc += w[m] * vs[m];
    acc = wave_sum(acc);
    if (lane == 0) s[o] = acc;
  }
}

// launch 4: u = s / (|s| + eps), sigma = u . s                                   grid (layers)
__global__ __launch_bounds__(NT) void sn_sigma_kernel(const munit_sn_item* __restrict__ items, int max_O, int max_N,
                                                      const float* __restrict__ ws, size_t layer_floats, size_t s_off,
                                                      float* __restrict__ sigma) {
  __shared__ float red[NT / 64];
  const munit_sn_item it = items[blockIdx.x];
  if (!sn_layer_ok(it, max_O, max_N)) return;
  const float* s = ws + blockIdx.x * layer_floats + s_off;
  float sq = 0.f;
  for (int o = threadIdx.x; o < it.O; o += NT) sq += s[o] * s[o];
  const float norm = sqrtf(block_sum(sq, red)) + SN_EPS;
  float dot = 0.f;
  for (int o = threadIdx.x; o < it.O; o += NT) {
    const float u = s[o] / norm;
    it.u[o] = u;
    dot += u * s[o];
  }
  dot = block_sum(dot, red);
  if (threadIdx.x == 0) {
    sigma[2 * it.slot] = dot;
    sigma[2 * it.slot + 1] = 1.f / dot;
  }
}

inline int grid_for(long long n) {
  return (int)std::max<long long>(1, std::min<long long>((n + NT - 1) / NT, 2048));
}

// V consecutive floats (V = 1 or 4; 4 needs 16-byte aligned addresses)
template <int V> struct Vec;
template <> struct Vec<1> {
  float e[1];
  __device__ static Vec ld(const float* p) { return Vec{{*p}}; }
  __device__ void st(float* p) const { *p = e[0]; }
};
template <> struct Vec<4> {
  float e[4];
  __device__ static Vec ld(const float* p) { const f32x4 v = ld4(p); return Vec{{v[0], v[1], v[2], v[3]}}; }
  __device__ void st(float* p) const { st4(p, f32x4{e[0], e[1], e[2], e[3]}); }
};

template <int V>
__global__ void sn_act_fwd_kernel(const float* __restrict__ raw, const float* __restrict__ inv_sigma,
                                  const float* __restrict__ bias, float* __restrict__ y, long long n, int C, int act,
                                  float slope) {
  const float inv = *inv_sigma;
  const long long nv = n / V;
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < nv; j += (long long)gridDim.x * blockDim.x) {
    const long long i = j * V;
    const Vec<V> r = Vec<V>::ld(raw + i);
    Vec<V> b{}, o;
    if (bias) b = Vec<V>::ld(bias + (int)(i % C));
#pragma unroll
    for (int k = 0; k < V; ++k) o.e[k] = apply_act(r.e[k] * inv + b.e[k], act, slope);
    o.st(y + i);
  }
}

__device__ inline float sn_act_grad(float g, float yy, int act, float slope) {
  if (act == MUNIT_ACT_RELU) return yy > 0.f ? g : 0.f;
  if (act == MUNIT_ACT_LRELU) return yy > 0.f ? g : g * slope;
  if (act == MUNIT_ACT_TANH) return g * (1.f - yy * yy);
  return g;
}

// backward without the reductions (the layer's parameters take no gradient): draw = dy act'(y) / sigma
template <int V>
__global__ void sn_act_bwd_plain_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                        const float* __restrict__ inv_sigma, float* __restrict__ draw, long long n, int act,
                                        float slope) {
  const float inv = *inv_sigma;
  const long long nv = n / V;
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < nv; j += (long long)gridDim.x * blockDim.x) {
    const Vec<V> g = Vec<V>::ld(dy + j * V), yy = Vec<V>::ld(y + j * V);
    Vec<V> o;
#pragma unroll
    for (int k = 0; k < V; ++k) o.e[k] = sn_act_grad(g.e[k], yy.e[k], act, slope) * inv;
    o.st(draw + j * V);
  }
}

// Stage 1 of the full backward.  The block is CW channel lanes (V channels each) x NT / CW pixel rows; block b takes the
// pixels b * rows + r, stepping by parts * rows.  part_db[b][c] = its sum of dz, part_coef[b] = its sum of dz * raw.
// V = 4 needs C % 4 == 0 and 16-byte aligned tensors.
template <int V>
__global__ __launch_bounds__(NT) void sn_act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                        const float* __restrict__ raw,
                                                        const float* __restrict__ inv_sigma, float* __restrict__ draw,
                                                        long long npix, int C, int cw_log2, int act, float slope,
                                                        float* __restrict__ part_db, float* __restrict__ part_coef) {
  __shared__ float red[V * NT];
  __shared__ float red4[NT / 64];
  const float inv = *inv_sigma;
  const int CW = 1 << cw_log2, rows = NT >> cw_log2;
  const int cl = threadIdx.x & (CW - 1), pl = threadIdx.x >> cw_log2;
  float coef = 0.f;
  for (int c0 = 0; c0 < C; c0 += CW * V) {
    const int c = c0 + cl * V;
    float sdb[V];
#pragma unroll
    for (int k = 0; k < V; ++k) sdb[k] = 0.f;
    if (c < C) {
      for (long long p = (long long)blockIdx.x * rows + pl; p < npix; p += (long long)gridDim.x * rows) {
        const long long i = p * C + c;
        const Vec<V> g = Vec<V>::ld(dy + i), yy = Vec<V>::ld(y + i), r = Vec<V>::ld(raw + i);
        Vec<V> o;
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const float dz = sn_act_grad(g.e[k], yy.e[k], act, slope);
          o.e[k] = dz * inv;
          sdb[k] += dz;
          coef += dz * r.e[k];
        }
        o.st(draw + i);
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < V; ++k) red[k * NT + threadIdx.x] = sdb[k];
    __syncthreads();
    if (pl == 0 && c < C) {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float s = sdb[k];
        for (int r = 1; r < rows; ++r) s += red[k * NT + (r << cw_log2) + cl];
        part_db[(size_t)blockIdx.x * C + c + k] = s;
      }
    }
  }
  coef = block_sum(coef, red4);
  if (threadIdx.x == 0) part_coef[blockIdx.x] = coef;
}

// Stage 2: db[c] (+)= sum over the blocks of part_db, coef = sum of part_coef / sigma^2 (by the first block)
__global__ __launch_bounds__(NT) void sn_act_bwd_finish_kernel(const float* __restrict__ part_db,
                                                               const float* __restrict__ part_coef, int parts, int C,
                                                               const float* __restrict__ inv_sigma, float* __restrict__ db,
                                                               int accumulate, float* __restrict__ coef) {
  __shared__ float red4[NT / 64];
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c < C && db) {
    float s = 0.f;
    for (int b = 0; b < parts; ++b) s += part_db[(size_t)b * C + c];
    db[c] = accumulate ? db[c] + s : s;
  }
  if (blockIdx.x == 0 && coef) {
    float s = 0.f;
    for (int b = threadIdx.x; b < parts; b += NT) s += part_coef[b];
    s = block_sum(s, red4);
    const float inv = *inv_sigma;
    if (threadIdx.x == 0) *coef = s * inv * inv;
  }
}

__global__ void sn_grad_fix_kernel(float* __restrict__ dw, const float* __restrict__ coef, const float* __restrict__ u,
                                   const float* __restrict__ v, long long total, int N, int KHW, int I, int accumulate) {
  const float k = *coef;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int o = (int)(i / N), m = (int)(i % N);
    const float fix = k * (u[o] * v[sn_ref_col(m, KHW, I)]);
    dw[i] = accumulate ? dw[i] - fix : -fix;
  }
}

// blocks of the backward's first stage and log2 of its channel lanes (16 .. 64), each lane taking V channels
int sn_bwd_parts(long long npix, int C, int V, int* cw_log2) {
  int l = 4;
  while (l < 6 && (1 << l) * V < C) ++l;
  *cw_log2 = l;
  const int rows = NT >> l;
  return (int)std::max<long long>(1, std::min<long long>((npix + rows - 1) / rows, SN_BWD_PARTS));
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" size_t munit_sn_power_iter_workspace_bytes(int n, int max_O, int max_N) {
  if (n < 1 || max_O < 1 || max_N < 1 || max_N > SN_MAX_N) return 0;
  return (size_t)n * sn_layer_floats(max_O, max_N) * sizeof(float);
}

extern "C" int munit_sn_power_iter(const munit_sn_item* items_dev, int n, int max_O, int max_N, float* sigma, void* ws,
                                   size_t ws_bytes, munit_stream_t stream) {
  MUNIT_CHECK_ARG(items_dev && sigma && ws && n >= 1 && n <= 65535, "sn_power_iter: bad table (n=%d)", n);
  MUNIT_CHECK_ARG(max_O >= 1 && max_N >= 1, "sn_power_iter: bad extents (max_O=%d, max_N=%d)", max_O, max_N);
  MUNIT_CHECK_ARG(max_N <= SN_MAX_N, "sn_power_iter: a weight with %d columns (Cin * KH * KW) is beyond the %d this kernel "
                  "keeps on chip", max_N, SN_MAX_N);
  if (ws_bytes < munit_sn_power_iter_workspace_bytes(n, max_O, max_N)) {
    munit_set_error("sn_power_iter: workspace too small (%zu < %zu bytes)", ws_bytes,
                    munit_sn_power_iter_workspace_bytes(n, max_O, max_N));
    return MUNIT_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  float* wsf = reinterpret_cast<float*>(ws);
  const size_t lf = sn_layer_floats(max_O, max_N), s_off = align_up((size_t)sn_chunks(max_O) * max_N, 64);
  hipLaunchKernelGGL(sn_wtu_kernel, dim3(cdiv(max_N, NT), sn_chunks(max_O), n), dim3(NT), 0, st, items_dev, max_O, max_N,
                     wsf, lf);
  MUNIT_CHECK_LAUNCH("sn_wtu");
  hipLaunchKernelGGL(sn_t_kernel, dim3(cdiv(max_N, NT), n), dim3(NT), 0, st, items_dev, max_O, max_N, wsf, lf);
  MUNIT_CHECK_LAUNCH("sn_t");
  hipLaunchKernelGGL(sn_wv_kernel, dim3(cdiv(max_O, SN_ROWS2), n), dim3(NT), 0, st, items_dev, max_O, max_N, wsf, lf,
                     s_off);
  MUNIT_CHECK_LAUNCH("sn_wv");
  hipLaunchKernelGGL(sn_sigma_kernel, dim3(n), dim3(NT), 0, st, items_dev, max_O, max_N, wsf, lf, s_off, sigma);
  MUNIT_CHECK_LAUNCH("sn_sigma");
  return MUNIT_OK;
}

extern "C" int munit_sn_act_fwd(const float* raw, const float* inv_sigma, const float* bias, float* y, size_t npix, int C,
                                int act, float slope, munit_stream_t stream) {
  MUNIT_CHECK_ARG(raw && inv_sigma && y && npix > 0 && C >= 1, "sn_act_fwd: bad args");
  MUNIT_CHECK_ARG(act >= MUNIT_ACT_NONE && act <= MUNIT_ACT_TANH, "sn_act_fwd: unknown activation %d", act);
  const long long n = (long long)npix * C;
  if (C % 4 == 0 && aligned16(raw) && aligned16(y) && aligned16(bias))
    hipLaunchKernelGGL(sn_act_fwd_kernel<4>, dim3(grid_for(n / 4)), dim3(NT), 0, (hipStream_t)stream, raw, inv_sigma, bias, y,
                       n, C, act, slope);
  else
    hipLaunchKernelGGL(sn_act_fwd_kernel<1>, dim3(grid_for(n)), dim3(NT), 0, (hipStream_t)stream, raw, inv_sigma, bias, y, n,
                       C, act, slope);
  MUNIT_CHECK_LAUNCH("sn_act_fwd");
  return MUNIT_OK;
}

extern "C" size_t munit_sn_act_bwd_workspace_bytes(size_t npix, int C) {
  if (npix == 0 || C < 1) return 0;
  const size_t parts = std::min<size_t>(npix, SN_BWD_PARTS);      // whatever lane shape the call takes
  return align_up(parts * C * sizeof(float), 256) + parts * sizeof(float);
}

extern "C" int munit_sn_act_bwd(const float* dy, const float* y, const float* raw, const float* inv_sigma, float* draw,
                                float* db, float beta, float* coef, size_t npix, int C, int act, float slope, void* ws,
                                size_t ws_bytes, munit_stream_t stream) {
  MUNIT_CHECK_ARG(dy && y && inv_sigma && draw && npix > 0 && C >= 1, "sn_act_bwd: bad args");
  MUNIT_CHECK_ARG(act >= MUNIT_ACT_NONE && act <= MUNIT_ACT_TANH, "sn_act_bwd: unknown activation %d", act);
  MUNIT_CHECK_ARG(beta == 0.f || beta == 1.f, "sn_act_bwd: beta must be 0 or 1, got %g", (double)beta);
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)npix * C;
  const bool vec = C % 4 == 0 && aligned16(dy) && aligned16(y) && aligned16(draw) && aligned16(raw);
  if (!db && !coef) {
    if (vec)
      hipLaunchKernelGGL(sn_act_bwd_plain_kernel<4>, dim3(grid_for(n / 4)), dim3(NT), 0, st, dy, y, inv_sigma, draw, n, act,
                         slope);
    else
      hipLaunchKernelGGL(sn_act_bwd_plain_kernel<1>, dim3(grid_for(n)), dim3(NT), 0, st, dy, y, inv_sigma, draw, n, act,
                         slope);
    MUNIT_CHECK_LAUNCH("sn_act_bwd_plain");
    return MUNIT_OK;
  }
  MUNIT_CHECK_ARG(raw && ws, "sn_act_bwd: db / coef need raw and a workspace");
  if (ws_bytes < munit_sn_act_bwd_workspace_bytes(npix, C)) {
    munit_set_error("sn_act_bwd: workspace too small (%zu < %zu bytes)", ws_bytes, munit_sn_act_bwd_workspace_bytes(npix, C));
    return MUNIT_ERR_WORKSPACE;
  }
  int l;
  const int parts = sn_bwd_parts((long long)npix, C, vec ? 4 : 1, &l);
  float* part_db = reinterpret_cast<float*>(ws);
  float* part_coef = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + align_up((size_t)parts * C * sizeof(float), 256));
  if (vec)
    hipLaunchKernelGGL(sn_act_bwd_kernel<4>, dim3(parts), dim3(NT), 0, st, dy, y, raw, inv_sigma, draw, (long long)npix, C, l,
                       act, slope, part_db, part_coef);
  else
    hipLaunchKernelGGL(sn_act_bwd_kernel<1>, dim3(parts), dim3(NT), 0, st, dy, y, raw, inv_sigma, draw, (long long)npix, C, l,
                       act, slope, part_db, part_coef);
  MUNIT_CHECK_LAUNCH("sn_act_bwd");
  hipLaunchKernelGGL(sn_act_bwd_finish_kernel, dim3(cdiv(C, NT)), dim3(NT), 0, st, part_db, part_coef, parts, C, inv_sigma,
                     db, (int)(beta != 0.f), coef);
  MUNIT_CHECK_LAUNCH("sn_act_bwd_finish");
  return MUNIT_OK;
}

extern "C" int munit_sn_grad_fix(float* dw, const float* coef, const float* u, const float* v, int O, int KH, int KW, int I,
                                 float beta, munit_stream_t stream) {
  MUNIT_CHECK_ARG(dw && coef && u && v && O >= 1 && KH >= 1 && KW >= 1 && I >= 1, "sn_grad_fix: bad args");
  MUNIT_CHECK_ARG(beta == 0.f || beta == 1.f, "sn_grad_fix: beta must be 0 or 1, got %g", (double)beta);
  const int N = KH * KW * I;
  const long long total = (long long)O * N;
  hipLaunchKernelGGL(sn_grad_fix_kernel, dim3(grid_for(total)), dim3(NT), 0, (hipStream_t)stream, dw, coef, u, v, total, N,
                     KH * KW, I, (int)(beta != 0.f));
  MUNIT_CHECK_LAUNCH("sn_grad_fix");
  return MUNIT_OK;
}
