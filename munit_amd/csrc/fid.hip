// FID evaluation (scripts/inception_utils.py): a batched dense fp32 product on the f32-input matrix instruction, and on
// top of it the feature moments (torch_cov), the Newton-Schulz matrix square root and the Frechet distance.
//
// munit_gemm_f32: C_p = alpha * op(A_p) * B_p + beta_eye * I, row-major, up to 8 problems of one shape in one launch.
//   128x128 output tile per 256-thread workgroup, 32-deep k tiles, four waves of 2x2 v_mfma_f32_32x32x2_f32 tiles each
//   (four independent accumulators per wave).  Both operands sit k-major in LDS -- As[k][m], Bs[k][n] -- so a fragment
//   read is 32 consecutive words per lane half (conflict free) and a k step costs two paired reads for 4 matrix
//   instructions of 64 cycles; the reads run one k step ahead of the matrix instructions.  The next k tile travels
//   global -> registers while the current one is multiplied and is written to the other LDS buffer afterwards: one
//   barrier per k tile.  Every output element is one k-ordered
//   fmaf chain (zero-filled tails add exact zeros), no split-K, no atomics: bitwise repeatable.
#include <algorithm>
#include <cstdint>
#include "common.h"

namespace {
constexpr int NT = 256;
constexpr int BM = 128, BN = 128, BK = 32;
// row strides (floats) of the k-major LDS images: 132 keeps rows 16-byte aligned for the straight 128-bit copies (B, and A
// under transA); the transposing word writes of a row-major A tile use 129, where the 8 k-quads x 4 rows of a lane half
// fall on 32 different banks ((4c + j) * 129 + m = 4c + j + m mod 32)
constexpr int LDS_LD = 132;
constexpr int LDS_LD_T = 129;
constexpr int KM_PASSES = BK / (NT / 32);        // k-major tile: 32 lanes x 4 words per row, NT / 32 rows per pass
constexpr int MM_QUADS = BK / 4;                 // m-major tile: BK / 4 lanes x 4 words per row
constexpr int MM_ROWS = NT / MM_QUADS, MM_PASSES = BM / MM_ROWS;
static_assert(KM_PASSES == MM_PASSES, "one staging array shape for both tile forms");
constexpr int STAGE = KM_PASSES;

struct GemmArgs {
  const float* A[MUNIT_GEMM_MAX];
  const float* B[MUNIT_GEMM_MAX];
  float* C[MUNIT_GEMM_MAX];
  int M, N, K, lda, ldb, ldc;
  float alpha, beta_eye;
  int vecA, vecB;   // every A / B pointer is 16-byte aligned and its leading dimension a multiple of 4
};

// BK x 128 tile whose source rows run along k (B, or A under transA): rows k0.., columns c0.. of src[rows][cols]
__device__ inline void load_kmajor(const float* __restrict__ src, int ld, int rows, int cols, int k0, int c0, bool vec,
                                   f32x4 (&out)[STAGE]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < KM_PASSES; ++i) {
    const int gr = k0 + (t >> 5) + (NT / 32) * i, gc = c0 + (t & 31) * 4;
    const float* p = src + (size_t)gr * ld + gc;
    if (vec && gr < rows && gc + 3 < cols) {
      out[i] = ld4(p);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) out[i][e] = (gr < rows && gc + e < cols) ? p[e] : 0.f;
    }
  }
}
__device__ inline void store_kmajor(float* lds, const f32x4 (&v)[STAGE]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < KM_PASSES; ++i) st4(lds + ((t >> 5) + (NT / 32) * i) * LDS_LD + (t & 31) * 4, v[i]);
}

// 128 x BK tile of a row-major A[M][K]: rows r0.., columns k0..; lands transposed (k-major) in LDS
__device__ inline void load_mmajor(const float* __restrict__ src, int ld, int rows, int cols, int r0, int k0, bool vec,
                                   f32x4 (&out)[STAGE]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < MM_PASSES; ++i) {
    const int gr = r0 + t / MM_QUADS + MM_ROWS * i, gc = k0 + (t % MM_QUADS) * 4;
    const float* p = src + (size_t)gr * ld + gc;
    if (vec && gr < rows && gc + 3 < cols) {
      out[i] = ld4(p);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) out[i][e] = (gr < rows && gc + e < cols) ? p[e] : 0.f;
    }
  }
}
__device__ inline void store_mmajor(float* lds, const f32x4 (&v)[STAGE]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < MM_PASSES; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) lds[((t % MM_QUADS) * 4 + e) * LDS_LD_T + t / MM_QUADS + MM_ROWS * i] = v[i][e];
}

template <bool TRANSA>
__global__ __launch_bounds__(NT) void gemm_f32_kernel(const GemmArgs a) {
  constexpr int SA = TRANSA ? LDS_LD : LDS_LD_T;
  __shared__ __attribute__((aligned(16))) float As[2][BK * LDS_LD];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK * LDS_LD];
  const int p = blockIdx.z;
  const float* __restrict__ A = a.A[p];
  const float* __restrict__ B = a.B[p];
  float* __restrict__ C = a.C[p];
  const int M = a.M, N = a.N, K = a.K;
  const int tiles_n = (N + BN - 1) / BN;
  const int m0 = (int)(blockIdx.x / tiles_n) * BM, n0 = (int)(blockIdx.x % tiles_n) * BN;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int l31 = lane & 31, h = lane >> 5;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  f32x4 ra[STAGE], rb[STAGE];
  const int nk = (K + BK - 1) / BK;
  if (TRANSA) load_kmajor(A, a.lda, K, M, 0, m0, a.vecA != 0, ra);
  else load_mmajor(A, a.lda, M, K, m0, 0, a.vecA != 0, ra);
  load_kmajor(B, a.ldb, K, N, 0, n0, a.vecB != 0, rb);
  if (TRANSA) store_kmajor(As[0], ra); else store_mmajor(As[0], ra);
  store_kmajor(Bs[0], rb);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) {
      const int k0 = (kt + 1) * BK;
      if (TRANSA) load_kmajor(A, a.lda, K, M, k0, m0, a.vecA != 0, ra);
      else load_mmajor(A, a.lda, M, K, m0, k0, a.vecA != 0, ra);
      load_kmajor(B, a.ldb, K, N, k0, n0, a.vecB != 0, rb);
    }
    const float* as = As[cur] + wm + l31;
    const float* bs = Bs[cur] + wn + l31;
    // fragments of k step s + 1 are read while the four matrix instructions of step s run
    float fa[2][2], fb[2][2];
    fa[0][0] = as[h * SA]; fa[0][1] = as[h * SA + 32];
    fb[0][0] = bs[h * LDS_LD]; fb[0][1] = bs[h * LDS_LD + 32];
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);   // the two paired LDS reads of step 0
#pragma unroll
    for (int s = 0; s < BK / 2; ++s) {
      const int c = s & 1, kn = 2 * s + 2 + h;
      if (s + 1 < BK / 2) {
        fa[c ^ 1][0] = as[kn * SA]; fa[c ^ 1][1] = as[kn * SA + 32];
        fb[c ^ 1][0] = bs[kn * LDS_LD]; fb[c ^ 1][1] = bs[kn * LDS_LD + 32];
      }
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][0], fb[c][0], acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][0], fb[c][1], acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][1], fb[c][0], acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][1], fb[c][1], acc[1][1], 0, 0, 0);
      // keep that order in the emitted code: the reads of step s + 1, then the matrix instructions of step s
      if (s + 1 < BK / 2) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    }
    if (kt + 1 < nk) {
      // the other buffer was last read in iteration kt-1, before that iteration's barrier
      if (TRANSA) store_kmajor(As[cur ^ 1], ra); else store_mmajor(As[cur ^ 1], ra);
      store_kmajor(Bs[cur ^ 1], rb);
    }
    __syncthreads();
  }

  // C/D map of the 32x32 forms: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn + j * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row < M && col < N) C[(size_t)row * a.ldc + col] = a.alpha * acc[i][j][r] + (row == col ? a.beta_eye : 0.f);
      }
    }
}

__device__ inline double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// sum over the NT threads of a block, fixed order; sh: NT / 64 doubles, free to reuse after the call returns
__device__ inline double block_sum_f64(double v, double* sh) {
  v = wave_sum_f64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// torch_cov's first half for 64 feature columns per block: mu = column mean, xc = pool - mu (pool is left alone)
__global__ __launch_bounds__(NT) void fid_center_kernel(const float* __restrict__ pool, int N, int D,
                                                        float* __restrict__ mu, float* __restrict__ xc) {
  __shared__ double part[4][64];
  __shared__ float mean[64];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + c;
  double s = 0.0;
  if (col < D)
    for (int r = g; r < N; r += 4) s += (double)pool[(size_t)r * D + col];
  part[g][c] = s;
  __syncthreads();
  if (g == 0) {
    const float m = (float)(((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) / (double)N);
    mean[c] = m;
    if (col < D) mu[col] = m;
  }
  __syncthreads();
  if (col < D) {
    const float m = mean[c];
    for (int r = g; r < N; r += 4) xc[(size_t)r * D + col] = pool[(size_t)r * D + col] - m;
  }
}

constexpr int NORM_PARTS = 256;

// sum(A o A) of matrix blockIdx.y, stage 1: NORM_PARTS partial sums per matrix
__global__ __launch_bounds__(NT) void ns_norm_partial_kernel(const float* __restrict__ A, long long n2,
                                                             double* __restrict__ partial) {
  __shared__ double sh[4];
  const float* a = A + (size_t)blockIdx.y * n2;
  double s = 0.0;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n2; i += (long long)NORM_PARTS * NT)
    s += (double)a[i] * (double)a[i];
  s = block_sum_f64(s, sh);
  if (threadIdx.x == 0) partial[(size_t)blockIdx.y * NORM_PARTS + blockIdx.x] = s;
}
// stage 2: normA = sqrt(sum)
__global__ __launch_bounds__(NT) void ns_norm_finish_kernel(const double* __restrict__ partial, float* __restrict__ norm) {
  __shared__ double sh[4];
  const double s = block_sum_f64(partial[(size_t)blockIdx.x * NORM_PARTS + threadIdx.x], sh);
  if (threadIdx.x == 0) norm[blockIdx.x] = (float)sqrt(s);
}
// Y = A / normA, Z = I
__global__ __launch_bounds__(NT) void ns_init_kernel(const float* __restrict__ A, const float* __restrict__ norm, int D,
                                                     long long n2, float* __restrict__ Y, float* __restrict__ Z) {
  const float nrm = norm[blockIdx.y];
  const size_t base = (size_t)blockIdx.y * n2;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n2; i += (long long)gridDim.x * NT) {
    Y[base + i] = A[base + i] / nrm;
    Z[base + i] = (i / D == i % D) ? 1.f : 0.f;
  }
}
// sA = Y * sqrt(normA)
__global__ __launch_bounds__(NT) void ns_final_kernel(const float* __restrict__ Y, const float* __restrict__ norm,
                                                      long long n2, float* __restrict__ sA) {
  const float s = sqrtf(norm[blockIdx.y]);
  const size_t base = (size_t)blockIdx.y * n2;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n2; i += (long long)gridDim.x * NT)
    sA[base + i] = Y[base + i] * s;
}

// |mu1 - mu2|^2 + tr sigma1 + tr sigma2 - 2 tr covmean: one block, four fixed-order sums in double, one rounding
__global__ __launch_bounds__(NT) void frechet_finish_kernel(const float* __restrict__ mu1, const float* __restrict__ s1,
                                                            const float* __restrict__ mu2, const float* __restrict__ s2,
                                                            const float* __restrict__ cm, int D, float* __restrict__ out) {
  __shared__ double sh[4];
  double dd = 0.0, t1 = 0.0, t2 = 0.0, tc = 0.0;
  for (int i = threadIdx.x; i < D; i += NT) {
    const double d = (double)mu1[i] - (double)mu2[i];
    const size_t ii = (size_t)i * D + i;
    dd += d * d;
    t1 += (double)s1[ii];
    t2 += (double)s2[ii];
    tc += (double)cm[ii];
  }
  dd = block_sum_f64(dd, sh);
  t1 = block_sum_f64(t1, sh);
  t2 = block_sum_f64(t2, sh);
  tc = block_sum_f64(tc, sh);
  if (threadIdx.x == 0) out[0] = (float)(dd + t1 + t2 - 2.0 * tc);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
size_t matrix_bytes(int rows, int cols, int ld) { return ((size_t)(rows - 1) * (size_t)ld + (size_t)cols) * sizeof(float); }

// `name` prefixes the error text; every check runs before the launch
int gemm_run(const char* name, const munit_gemm_problem* prob, int n, int M, int N, int K, int lda, int ldb, int ldc,
             int transA, float alpha, float beta_eye, hipStream_t st) {
  MUNIT_CHECK_ARG(prob, "%s: null problem table", name);
  MUNIT_CHECK_ARG(n >= 1 && n <= MUNIT_GEMM_MAX, "%s: n must be 1..%d, got %d", name, MUNIT_GEMM_MAX, n);
  MUNIT_CHECK_ARG(M >= 1 && N >= 1 && K >= 1, "%s: M, N, K must be >= 1, got %d %d %d", name, M, N, K);
  const int a_rows = transA ? K : M, a_cols = transA ? M : K;
  MUNIT_CHECK_ARG(lda >= a_cols, "%s: lda %d shorter than its row of %d", name, lda, a_cols);
  MUNIT_CHECK_ARG(ldb >= N, "%s: ldb %d shorter than its row of %d", name, ldb, N);
  MUNIT_CHECK_ARG(ldc >= N, "%s: ldc %d shorter than its row of %d", name, ldc, N);
  const size_t a_bytes = matrix_bytes(a_rows, a_cols, lda), b_bytes = matrix_bytes(K, N, ldb),
               c_bytes = matrix_bytes(M, N, ldc);
  for (int p = 0; p < n; ++p)
    MUNIT_CHECK_ARG(prob[p].A && prob[p].B && prob[p].C, "%s: problem %d has a null pointer", name, p);
  for (int p = 0; p < n; ++p)
    for (int q = 0; q < n; ++q) {
      MUNIT_CHECK_ARG(!ranges_overlap(prob[p].C, c_bytes, prob[q].A, a_bytes) &&
                          !ranges_overlap(prob[p].C, c_bytes, prob[q].B, b_bytes),
                      "%s: C of problem %d overlaps an operand of problem %d", name, p, q);
      MUNIT_CHECK_ARG(p == q || !ranges_overlap(prob[p].C, c_bytes, prob[q].C, c_bytes),
                      "%s: C of problem %d overlaps C of problem %d", name, p, q);
    }
  GemmArgs a{};
  a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldb = ldb; a.ldc = ldc;
  a.alpha = alpha; a.beta_eye = beta_eye;
  a.vecA = lda % 4 == 0; a.vecB = ldb % 4 == 0;
  for (int p = 0; p < n; ++p) {
    a.A[p] = prob[p].A; a.B[p] = prob[p].B; a.C[p] = prob[p].C;
    a.vecA = a.vecA && aligned16(prob[p].A);
    a.vecB = a.vecB && aligned16(prob[p].B);
  }
  const long long tiles = (long long)cdiv(M, BM) * cdiv(N, BN);
  MUNIT_CHECK_ARG(tiles <= 0x7fffffffLL, "%s: too many output tiles", name);
  const dim3 grid((unsigned)tiles, 1, (unsigned)n);
  if (transA) hipLaunchKernelGGL(gemm_f32_kernel<true>, grid, dim3(NT), 0, st, a);
  else hipLaunchKernelGGL(gemm_f32_kernel<false>, grid, dim3(NT), 0, st, a);
  MUNIT_CHECK_LAUNCH("gemm_f32");
  return MUNIT_OK;
}

int elementwise_blocks(long long n) { return (int)std::min<long long>(1024, (n + NT - 1) / NT); }

// workspace of the square root: [partial sums | norms] then Y0 Y1 Z0 Z1 T, b matrices each
size_t ns_head_bytes(int b) { return align_up((size_t)b * NORM_PARTS * sizeof(double) + (size_t)b * sizeof(float), 256); }
size_t ns_workspace_bytes(int D, int b) {
  if (D < 1 || b < 1) return 0;
  return ns_head_bytes(b) + 5 * (size_t)b * (size_t)D * (size_t)D * sizeof(float);
}

// the recurrence on checked arguments
int ns_run(const char* name, const float* A, int D, int iters, int b, float* sA, void* ws, hipStream_t st) {
  const long long n2 = (long long)D * D;
  double* partial = reinterpret_cast<double*>(ws);
  float* norm = reinterpret_cast<float*>(partial + (size_t)b * NORM_PARTS);
  float* mats = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + ns_head_bytes(b));
  const size_t bn2 = (size_t)b * n2;
  float* Y[2] = {mats, mats + bn2};
  float* Z[2] = {mats + 2 * bn2, mats + 3 * bn2};
  float* T = mats + 4 * bn2;
  const int eb = elementwise_blocks(n2);

  hipLaunchKernelGGL(ns_norm_partial_kernel, dim3(NORM_PARTS, b), dim3(NT), 0, st, A, n2, partial);
  MUNIT_CHECK_LAUNCH("ns_norm_partial");
  hipLaunchKernelGGL(ns_norm_finish_kernel, dim3(b), dim3(NT), 0, st, partial, norm);
  MUNIT_CHECK_LAUNCH("ns_norm_finish");
  hipLaunchKernelGGL(ns_init_kernel, dim3(eb, b), dim3(NT), 0, st, A, norm, D, n2, Y[0], Z[0]);
  MUNIT_CHECK_LAUNCH("ns_init");

  int cur = 0;
  munit_gemm_problem prob[MUNIT_GEMM_MAX];
  for (int it = 0; it < iters; ++it, cur ^= 1) {
    // T = 1.5 I - 0.5 Z Y
    for (int m0 = 0; m0 < b; m0 += MUNIT_GEMM_MAX) {
      const int n = std::min((int)MUNIT_GEMM_MAX, b - m0);
      for (int i = 0; i < n; ++i) prob[i] = {Z[cur] + (size_t)(m0 + i) * n2, Y[cur] + (size_t)(m0 + i) * n2, T + (size_t)(m0 + i) * n2};
      if (const int rc = gemm_run(name, prob, n, D, D, D, D, D, D, 0, -0.5f, 1.5f, st)) return rc;
    }
    // Y <- Y T and Z <- T Z, both in one launch
    for (int m0 = 0; m0 < b; m0 += MUNIT_GEMM_MAX / 2) {
      const int n = std::min((int)MUNIT_GEMM_MAX / 2, b - m0);
      for (int i = 0; i < n; ++i) {
        const size_t off = (size_t)(m0 + i) * n2;
        prob[2 * i] = {Y[cur] + off, T + off, Y[cur ^ 1] + off};
        prob[2 * i + 1] = {T + off, Z[cur] + off, Z[cur ^ 1] + off};
      }
      if (const int rc = gemm_run(name, prob, 2 * n, D, D, D, D, D, D, 0, 1.f, 0.f, st)) return rc;
    }
  }
  hipLaunchKernelGGL(ns_final_kernel, dim3(eb, b), dim3(NT), 0, st, Y[cur], norm, n2, sA);
  MUNIT_CHECK_LAUNCH("ns_final");
  return MUNIT_OK;
}
}  // namespace

extern "C" int munit_gemm_f32(const munit_gemm_problem* prob, int n, int M, int N, int K, int lda, int ldb, int ldc,
                              int transA, float alpha, float beta_eye, munit_stream_t stream) {
  return gemm_run("gemm_f32", prob, n, M, N, K, lda, ldb, ldc, transA, alpha, beta_eye, (hipStream_t)stream);
}

extern "C" size_t munit_fid_moments_workspace_bytes(int N, int D) {
  return (N >= 2 && D >= 1) ? (size_t)N * (size_t)D * sizeof(float) : 0;
}

extern "C" int munit_fid_moments(const float* pool, int N, int D, float* mu, float* sigma, void* ws, size_t ws_bytes,
                                 munit_stream_t stream) {
  MUNIT_CHECK_ARG(pool && mu && sigma && ws, "fid_moments: null pointer");
  MUNIT_CHECK_ARG(D >= 1, "fid_moments: D must be >= 1, got %d", D);
  MUNIT_CHECK_ARG(N >= 2, "fid_moments: N must be >= 2, got %d", N);
  MUNIT_CHECK_ARG(ws_bytes >= munit_fid_moments_workspace_bytes(N, D), "fid_moments: workspace too small");
  float* xc = reinterpret_cast<float*>(ws);
  hipLaunchKernelGGL(fid_center_kernel, dim3(cdiv(D, 64)), dim3(NT), 0, (hipStream_t)stream, pool, N, D, mu, xc);
  MUNIT_CHECK_LAUNCH("fid_center");
  const munit_gemm_problem prob = {xc, xc, sigma};
  return gemm_run("fid_moments", &prob, 1, D, D, N, D, D, D, 1, 1.0f / (float)(N - 1), 0.f, (hipStream_t)stream);
}

extern "C" size_t munit_sqrt_newton_schulz_workspace_bytes(int D, int b) { return ns_workspace_bytes(D, b); }

extern "C" int munit_sqrt_newton_schulz(const float* A, int D, int iters, int b, float* sA, void* ws, size_t ws_bytes,
                                        munit_stream_t stream) {
  MUNIT_CHECK_ARG(A && sA && ws, "sqrt_newton_schulz: null pointer");
  MUNIT_CHECK_ARG(D >= 1, "sqrt_newton_schulz: D must be >= 1, got %d", D);
  MUNIT_CHECK_ARG(iters >= 0, "sqrt_newton_schulz: iters must be >= 0, got %d", iters);
  MUNIT_CHECK_ARG(b >= 1 && b <= 65535, "sqrt_newton_schulz: b must be 1..65535, got %d", b);
  MUNIT_CHECK_ARG(ws_bytes >= ns_workspace_bytes(D, b), "sqrt_newton_schulz: workspace too small");
  return ns_run("sqrt_newton_schulz", A, D, iters, b, sA, ws, (hipStream_t)stream);
}

extern "C" size_t munit_frechet_distance_workspace_bytes(int D) {
  if (D < 1) return 0;
  return 2 * align_up((size_t)D * (size_t)D * sizeof(float), 256) + ns_workspace_bytes(D, 1);
}

extern "C" int munit_frechet_distance(const float* mu1, const float* sigma1, const float* mu2, const float* sigma2, int D,
                                      int iters, float* out, void* ws, size_t ws_bytes, munit_stream_t stream) {
  MUNIT_CHECK_ARG(mu1 && sigma1 && mu2 && sigma2 && out && ws, "frechet_distance: null pointer");
  MUNIT_CHECK_ARG(D >= 1, "frechet_distance: D must be >= 1, got %d", D);
  MUNIT_CHECK_ARG(iters >= 0, "frechet_distance: iters must be >= 0, got %d", iters);
  MUNIT_CHECK_ARG(ws_bytes >= munit_frechet_distance_workspace_bytes(D), "frechet_distance: workspace too small");
  const size_t mat = align_up((size_t)D * (size_t)D * sizeof(float), 256);
  float* prod = reinterpret_cast<float*>(ws);
  float* root = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + mat);
  void* ns_ws = reinterpret_cast<char*>(ws) + 2 * mat;
  const munit_gemm_problem prob = {sigma1, sigma2, prod};
  if (const int rc = gemm_run("frechet_distance", &prob, 1, D, D, D, D, D, D, 0, 1.f, 0.f, (hipStream_t)stream)) return rc;
  if (const int rc = ns_run("frechet_distance", prod, D, iters, 1, root, ns_ws, (hipStream_t)stream)) return rc;
  hipLaunchKernelGGL(frechet_finish_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, mu1, sigma1, mu2, sigma2, root, D,
                     out);
  MUNIT_CHECK_LAUNCH("frechet_finish");
  return MUNIT_OK;
}
