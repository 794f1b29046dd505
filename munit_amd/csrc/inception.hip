// Inception-v3 feature trunk of FID evaluation (scripts/inception_utils.py:27-85): inference only, fp32, NHWC.
//
// munit_conv2d_rect_fwd: y = relu?(conv(x, w) + bias) for a KH x KW filter with its own pad per axis, as an implicit GEMM on
//   the exact-fp32 matrix instruction (v_mfma_f32_32x32x2_f32), built like munit_gemm_f32 (fid.hip): M = B*Ho*Wo output
//   pixels, N = Cout, K = KH*KW*Cin with k = (kh*KW + kw)*Cin + ci.  The weights arrive as the k-major image wk[K][Cout], so
//   the B operand is a straight copy; the A operand is gathered from x (one 128-bit load per four channels of a tap when
//   Cin, x_ld and the pointer allow it, word loads otherwise) and lands transposed in LDS.  Both operands sit k-major in
//   LDS, 32-deep k tiles, double buffered, one barrier per k tile.  256 threads = 2 x 2 waves; three tile shapes, 128 x 128
//   (2 x 2 matrix tiles per wave), 128 x 64 (2 x 1) and 64 x 64 (one per wave), chosen on the host: the small one while
//   128 x 128 tiles would leave CUs idle, else the 128-row tile that pads Cout least.  Tails in M, N and K
//   are zero-filled in LDS; border taps are zeros.  Every output is one k-ordered fmaf chain from 0, then + bias, then
//   ReLU: no split-K, no atomics, and the chain does not depend on the tile shape or on B.
//   x_ld / y_ld are per-pixel channel strides: a layer reads a channel slice of a wider buffer and writes into a channel
//   slice of the block's concatenated output; channels outside the slices are neither read nor written.
// munit_window3_fwd: 3 x 3 max / average window (F.max_pool2d(3, 2), F.avg_pool2d(3, 1, 1)) with the same two strides.
// munit_inception_input: WrapInception.forward's normalisation and bilinear resize to 299 x 299 in one launch.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include "common.h"

namespace {
constexpr int NT = 256;
constexpr int BK = 32;
constexpr int OUT_HW = 299;

struct RectArgs {
  const float* x;
  const float* w;
  const float* bias;
  float* y;
  int H, W, Cin, x_ld, Cout, y_ld, KW, stride, pad_h, pad_w, relu, Ho, Wo, M, K;
  int vecA, vecB;   // 128-bit loads: x / wk 16-byte aligned with Cin and x_ld / Cout multiples of 4
};

template <int BM, int BN>
__global__ __launch_bounds__(NT) void conv_rect_kernel(const RectArgs a) {
  constexpr int TI = BM / 64, TJ = BN / 64;        // 32 x 32 matrix tiles per wave
  constexpr int SA = BM + 1;                       // transposing word writes: 8 k-quads x 4 rows on 32 different banks
  constexpr int SB = BN + 4;                       // straight 128-bit copies: rows stay 16-byte aligned
  constexpr int AP = BM / (NT / 8);                // A tile: 8 lanes x 4 words per pixel row, NT / 8 rows per pass
  constexpr int BL = BN / 4, BR = NT / BL, BP = BK / BR;   // B tile: BL lanes x 4 words per k row, BR rows per pass
  __shared__ __attribute__((aligned(16))) float As[2][BK * SA];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK * SB];
  const float* __restrict__ x = a.x;
  const float* __restrict__ wk = a.w;
  const int M = a.M, N = a.Cout, K = a.K;
  const int tiles_n = (N + BN - 1) / BN;
  const int m0 = (int)(blockIdx.x / tiles_n) * BM, n0 = (int)(blockIdx.x % tiles_n) * BN;
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wm = (wave >> 1) * (BM / 2), wn = (wave & 1) * (BN / 2);
  const int l31 = lane & 31, h = lane >> 5;

  // the AP output pixels whose patch rows this thread gathers: top-left tap and image base, fixed over the k loop
  int ih0[AP], iw0[AP];
  long long pbase[AP];
#pragma unroll
  for (int i = 0; i < AP; ++i) {
    const int m = m0 + (t >> 3) + (NT / 8) * i;
    if (m < M) {
      const int ow = m % a.Wo, r = m / a.Wo;
      const int oh = r % a.Ho, b = r / a.Ho;
      ih0[i] = oh * a.stride - a.pad_h;
      iw0[i] = ow * a.stride - a.pad_w;
      pbase[i] = (long long)b * a.H * a.W;
    } else {
      ih0[i] = -(1 << 20);      // every tap of a tail row fails the bounds test below
      iw0[i] = 0;
      pbase[i] = 0;
    }
  }

  auto load_a = [&](int k0, f32x4(&out)[AP]) {
    const int kq = k0 + (t & 7) * 4;
    if (a.vecA) {
      const int tap = kq / a.Cin, ci = kq - tap * a.Cin;
      const int kh = tap / a.KW, kw = tap - kh * a.KW;
#pragma unroll
      for (int i = 0; i < AP; ++i) {
        const int ih = ih0[i] + kh, iw = iw0[i] + kw;
        const bool ok = kq < K && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
        if (ok) out[i] = ld4(x + (size_t)(pbase[i] + (long long)ih * a.W + iw) * a.x_ld + ci);
        else out[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = kq + e;
        const int tap = k / a.Cin, ci = k - tap * a.Cin;
        const int kh = tap / a.KW, kw = tap - kh * a.KW;
#pragma unroll
        for (int i = 0; i < AP; ++i) {
          const int ih = ih0[i] + kh, iw = iw0[i] + kw;
          const bool ok = k < K && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
          out[i][e] = ok ? x[(size_t)(pbase[i] + (long long)ih * a.W + iw) * a.x_ld + ci] : 0.f;
        }
      }
    }
  };
  auto store_a = [&](float* lds, const f32x4(&v)[AP]) {
#pragma unroll
    for (int i = 0; i < AP; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) lds[((t & 7) * 4 + e) * SA + (t >> 3) + (NT / 8) * i] = v[i][e];
  };
  auto load_b = [&](int k0, f32x4(&out)[BP]) {
#pragma unroll
    for (int i = 0; i < BP; ++i) {
      const int gr = k0 + t / BL + BR * i, gc = n0 + (t % BL) * 4;
      const float* p = wk + (size_t)gr * N + gc;
      if (a.vecB && gr < K && gc + 3 < N) {
        out[i] = ld4(p);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) out[i][e] = (gr < K && gc + e < N) ? p[e] : 0.f;
      }
    }
  };
  auto store_b = [&](float* lds, const f32x4(&v)[BP]) {
#pragma unroll
    for (int i = 0; i < BP; ++i) st4(lds + (t / BL + BR * i) * SB + (t % BL) * 4, v[i]);
  };

  f32x16 acc[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  f32x4 ra[AP], rb[BP];
  const int nk = (K + BK - 1) / BK;
  load_a(0, ra);
  load_b(0, rb);
  store_a(As[0], ra);
  store_b(Bs[0], rb);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) {
      load_a((kt + 1) * BK, ra);
      load_b((kt + 1) * BK, rb);
    }
    const float* as = As[cur] + wm + l31;
    const float* bs = Bs[cur] + wn + l31;
    // fragments of k step s + 1 are read while the matrix instructions of step s run
    float fa[2][TI], fb[2][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i) fa[0][i] = as[h * SA + 32 * i];
#pragma unroll
    for (int j = 0; j < TJ; ++j) fb[0][j] = bs[h * SB + 32 * j];
#pragma unroll
    for (int s = 0; s < BK / 2; ++s) {
      const int c = s & 1, kn = 2 * s + 2 + h;
      if (s + 1 < BK / 2) {
#pragma unroll
        for (int i = 0; i < TI; ++i) fa[c ^ 1][i] = as[kn * SA + 32 * i];
#pragma unroll
        for (int j = 0; j < TJ; ++j) fb[c ^ 1][j] = bs[kn * SB + 32 * j];
      }
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][i], fb[c][j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) {
      // the other buffer was last read in iteration kt - 1, before that iteration's barrier
      store_a(As[cur ^ 1], ra);
      store_b(Bs[cur ^ 1], rb);
    }
    __syncthreads();
  }

  // C/D map of the 32x32 forms: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int col = n0 + wn + j * 32 + l31;
    const float bv = col < N ? a.bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row < M && col < N) {
          float v = acc[i][j][r] + bv;
          if (a.relu) v = v > 0.f ? v : 0.f;
          a.y[(size_t)row * a.y_ld + col] = v;
        }
      }
  }
}

// one thread per output pixel and four channels; taps in window order (kh-major)
template <bool MAX>
__global__ __launch_bounds__(NT) void window3_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int C4,
                                                     int x_ld, int y_ld, int Ho, int Wo, int stride, int pad,
                                                     long long total) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    const int cq = (int)(i % C4);
    const long long pix = i / C4;
    const int ow = (int)(pix % Wo);
    const long long r = pix / Wo;
    const int oh = (int)(r % Ho);
    const long long b = r / Ho;
    f32x4 acc;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = MAX ? -INFINITY : 0.f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int ih = oh * stride - pad + kh, iw = ow * stride - pad + kw;
        if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) {
          const f32x4 v = ld4(x + (size_t)((b * H + ih) * W + iw) * x_ld + cq * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = MAX ? (v[e] > acc[e] || v[e] != v[e] ? v[e] : acc[e]) : acc[e] + v[e];
        }
      }
    if (!MAX) {
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = acc[e] / 9.f;      // count_include_pad: the divisor is always 9
    }
    st4(y + (size_t)pix * y_ld + cq * 4, acc);
  }
}

// ((x + 1) / 2 - mean) / std of one source element; sc: element stride between channels, c: channel
__device__ inline float inception_norm(const float* __restrict__ p, int c) {
  const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f);
  const float sd = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
  return ((p[0] + 1.0f) / 2.0f - mean) / sd;
}

// one thread per output pixel; bilinear with align_corners = True as torch evaluates it in fp32:
// scale = (in - 1) / (out - 1), src = scale * dst, i0 = (int)src, lambda1 = src - i0, lambda0 = 1 - lambda1
__global__ __launch_bounds__(NT) void inception_input_kernel(const float* __restrict__ x, long long sb, long long sc,
                                                             long long sh, long long sw, int H, int W,
                                                             float* __restrict__ y, long long total) {
  const bool same = H == OUT_HW && W == OUT_HW;
  const float scale_h = (float)(H - 1) / (float)(OUT_HW - 1), scale_w = (float)(W - 1) / (float)(OUT_HW - 1);
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    const int ox = (int)(i % OUT_HW);
    const long long r = i / OUT_HW;
    const int oy = (int)(r % OUT_HW);
    const long long b = r / OUT_HW;
    const float* xb = x + b * sb;
    float* out = y + i * 3;
    if (same) {
#pragma unroll
      for (int c = 0; c < 3; ++c) out[c] = inception_norm(xb + c * sc + oy * sh + ox * sw, c);
      continue;
    }
    const float fy = scale_h * (float)oy, fx = scale_w * (float)ox;
    const int y0 = (int)fy, x0 = (int)fx;
    const int yp = y0 < H - 1 ? 1 : 0, xp = x0 < W - 1 ? 1 : 0;
    const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
    const float ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* pc = xb + c * sc;
      const float v00 = inception_norm(pc + y0 * sh + x0 * sw, c);
      const float v01 = inception_norm(pc + y0 * sh + (x0 + xp) * sw, c);
      const float v10 = inception_norm(pc + (y0 + yp) * sh + x0 * sw, c);
      const float v11 = inception_norm(pc + (y0 + yp) * sh + (x0 + xp) * sw, c);
      out[c] = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool overlap(const void* p, size_t pn, const void* q, size_t qn) {
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(p), q0 = reinterpret_cast<uintptr_t>(q);
  return p0 < q0 + qn && q0 < p0 + pn;
}
// bytes from the first to the last word of a channel slice of npix pixels
size_t slice_bytes(long long npix, int ld, int c) { return ((size_t)(npix - 1) * (size_t)ld + (size_t)c) * sizeof(float); }
int grid_for(long long total) { return (int)std::min<long long>(4096, (total + NT - 1) / NT); }

constexpr int CU_COUNT_DEFAULT = 256;   // MI355X; what the tile choice assumes where no device can be asked
constexpr int MAX_DEVICES = 64;

// compute units of the current device, asked once per device (the choice below changes speed only, never a result)
int cu_count() {
  static int cached[MAX_DEVICES] = {};
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) {
    (void)hipGetLastError();
    return CU_COUNT_DEFAULT;
  }
  if (cached[dev] > 0) return cached[dev];
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) {
    (void)hipGetLastError();
    return CU_COUNT_DEFAULT;
  }
  return cached[dev] = n;
}
constexpr int TILE_128 = 0, TILE_64 = 1, TILE_128x64 = 2;

// geometry alone: the checks shared by the three conv entry points
int rect_check(const char* name, const munit_rect_desc* d, int* Ho, int* Wo) {
  MUNIT_CHECK_ARG(d, "%s: null descriptor", name);
  MUNIT_CHECK_ARG(d->B >= 1 && d->H >= 1 && d->W >= 1 && d->Cin >= 1 && d->Cout >= 1,
                  "%s: B, H, W, Cin, Cout must be >= 1, got %d %d %d %d %d", name, d->B, d->H, d->W, d->Cin, d->Cout);
  MUNIT_CHECK_ARG(d->KH >= 1 && d->KW >= 1 && d->KH <= 15 && d->KW <= 15, "%s: KH, KW must be 1..15, got %d %d", name,
                  d->KH, d->KW);
  MUNIT_CHECK_ARG(d->x_ld >= d->Cin, "%s: x_ld %d shorter than its slice of %d", name, d->x_ld, d->Cin);
  MUNIT_CHECK_ARG(d->y_ld >= d->Cout, "%s: y_ld %d shorter than its slice of %d", name, d->y_ld, d->Cout);
  MUNIT_CHECK_ARG(d->stride == 1 || d->stride == 2, "%s: stride must be 1 or 2, got %d", name, d->stride);
  MUNIT_CHECK_ARG(d->pad_h >= 0 && d->pad_h <= (d->KH - 1) / 2 && d->pad_w >= 0 && d->pad_w <= (d->KW - 1) / 2,
                  "%s: pads (%d, %d) must be 0..(K - 1) / 2 of a %d x %d filter", name, d->pad_h, d->pad_w, d->KH, d->KW);
  MUNIT_CHECK_ARG(d->H + 2 * d->pad_h >= d->KH && d->W + 2 * d->pad_w >= d->KW,
                  "%s: output extent below 1 (%d x %d input, %d x %d filter)", name, d->H, d->W, d->KH, d->KW);
  *Ho = (d->H + 2 * d->pad_h - d->KH) / d->stride + 1;
  *Wo = (d->W + 2 * d->pad_w - d->KW) / d->stride + 1;
  const long long M = (long long)d->B * *Ho * *Wo, K = (long long)d->KH * d->KW * d->Cin;
  MUNIT_CHECK_ARG(M <= 0x7fffffffLL - 256 && K <= 0x7fffffffLL - 256 && (long long)d->B * d->H * d->W <= 0x7fffffffLL,
                  "%s: more than 2^31 pixels or filter taps", name);
  return MUNIT_OK;
}

int rect_tile(const munit_rect_desc* d, int Ho, int Wo) {
  const long long M = (long long)d->B * Ho * Wo;
  if ((long long)cdiv(M, 128) * cdiv(d->Cout, 128) < cu_count()) return TILE_64;
  // enough 128-row tiles to fill the device: the narrower tile where it pads Cout less (Cout 32..64, 192, 320 of the trunk)
  return cdiv(d->Cout, 64) * 64 < cdiv(d->Cout, 128) * 128 ? TILE_128x64 : TILE_128;
}
}  // namespace

extern "C" int munit_conv2d_rect_out_hw(const munit_rect_desc* d, int* Ho, int* Wo) {
  MUNIT_CHECK_ARG(Ho && Wo, "conv2d_rect_out_hw: null pointer");
  return rect_check("conv2d_rect_out_hw", d, Ho, Wo);
}

extern "C" int munit_conv2d_rect_tile(const munit_rect_desc* d) {
  int Ho, Wo;
  if (rect_check("conv2d_rect_tile", d, &Ho, &Wo)) return MUNIT_ERR_ARG;
  return rect_tile(d, Ho, Wo);
}

extern "C" int munit_conv2d_rect_fwd(const munit_rect_desc* d, const float* x, const float* wk, const float* bias, float* y,
                                     int tile, munit_stream_t stream) {
  int Ho, Wo;
  if (const int rc = rect_check("conv2d_rect_fwd", d, &Ho, &Wo)) return rc;
  MUNIT_CHECK_ARG(x && wk && bias && y, "conv2d_rect_fwd: null pointer");
  MUNIT_CHECK_ARG(tile >= -1 && tile <= TILE_128x64, "conv2d_rect_fwd: tile must be -1 (chosen here), 0, 1 or 2, got %d", tile);
  const long long M = (long long)d->B * Ho * Wo;
  const int K = d->KH * d->KW * d->Cin;
  const size_t xb = slice_bytes((long long)d->B * d->H * d->W, d->x_ld, d->Cin), yb = slice_bytes(M, d->y_ld, d->Cout);
  MUNIT_CHECK_ARG(!overlap(y, yb, x, xb), "conv2d_rect_fwd: y overlaps x");
  MUNIT_CHECK_ARG(!overlap(y, yb, wk, (size_t)K * d->Cout * sizeof(float)) && !overlap(y, yb, bias, d->Cout * sizeof(float)),
                  "conv2d_rect_fwd: y overlaps the weights or the bias");
  if (tile < 0) tile = rect_tile(d, Ho, Wo);
  const int bm = tile == TILE_64 ? 64 : 128, bn = tile == TILE_128 ? 128 : 64;
  const long long tiles = (long long)cdiv(M, bm) * cdiv(d->Cout, bn);
  MUNIT_CHECK_ARG(tiles <= 0x7fffffffLL, "conv2d_rect_fwd: too many output tiles");
  RectArgs a{};
  a.x = x; a.w = wk; a.bias = bias; a.y = y;
  a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.x_ld = d->x_ld; a.Cout = d->Cout; a.y_ld = d->y_ld; a.KW = d->KW;
  a.stride = d->stride; a.pad_h = d->pad_h; a.pad_w = d->pad_w; a.relu = d->relu != 0;
  a.Ho = Ho; a.Wo = Wo; a.M = (int)M; a.K = K;
  a.vecA = d->Cin % 4 == 0 && d->x_ld % 4 == 0 && aligned16(x);
  a.vecB = d->Cout % 4 == 0 && aligned16(wk);
  if (tile == TILE_128) hipLaunchKernelGGL((conv_rect_kernel<128, 128>), dim3((unsigned)tiles), dim3(NT), 0, (hipStream_t)stream, a);
  else if (tile == TILE_128x64) hipLaunchKernelGGL((conv_rect_kernel<128, 64>), dim3((unsigned)tiles), dim3(NT), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((conv_rect_kernel<64, 64>), dim3((unsigned)tiles), dim3(NT), 0, (hipStream_t)stream, a);
  MUNIT_CHECK_LAUNCH("conv2d_rect_fwd");
  return MUNIT_OK;
}

extern "C" int munit_window3_fwd(const float* x, float* y, int B, int H, int W, int C, int x_ld, int y_ld, int mode,
                                 int stride, int pad, munit_stream_t stream) {
  MUNIT_CHECK_ARG(x && y, "window3_fwd: null pointer");
  MUNIT_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && C >= 1, "window3_fwd: B, H, W, C must be >= 1, got %d %d %d %d", B, H, W, C);
  MUNIT_CHECK_ARG(mode == MUNIT_WINDOW_MAX || mode == MUNIT_WINDOW_AVG, "window3_fwd: mode must be 0 (max) or 1 (avg), got %d",
                  mode);
  MUNIT_CHECK_ARG(C % 4 == 0, "window3_fwd: C %% 4 == 0 is required, got %d", C);
  MUNIT_CHECK_ARG(x_ld >= C, "window3_fwd: x_ld %d shorter than its slice of %d", x_ld, C);
  MUNIT_CHECK_ARG(y_ld >= C, "window3_fwd: y_ld %d shorter than its slice of %d", y_ld, C);
  MUNIT_CHECK_ARG(x_ld % 4 == 0 && y_ld % 4 == 0 && aligned16(x) && aligned16(y),
                  "window3_fwd: x, y must be 16-byte aligned and x_ld, y_ld multiples of 4");
  MUNIT_CHECK_ARG(stride == 1 || stride == 2, "window3_fwd: stride must be 1 or 2, got %d", stride);
  MUNIT_CHECK_ARG(pad == 0 || pad == 1, "window3_fwd: pad must be 0 or 1, got %d", pad);
  MUNIT_CHECK_ARG(H + 2 * pad >= 3 && W + 2 * pad >= 3, "window3_fwd: output extent below 1 (%d x %d input)", H, W);
  const int Ho = (H + 2 * pad - 3) / stride + 1, Wo = (W + 2 * pad - 3) / stride + 1;
  const long long in_pix = (long long)B * H * W, out_pix = (long long)B * Ho * Wo;
  MUNIT_CHECK_ARG(in_pix <= 0x7fffffffLL, "window3_fwd: more than 2^31 pixels");
  MUNIT_CHECK_ARG(!overlap(y, slice_bytes(out_pix, y_ld, C), x, slice_bytes(in_pix, x_ld, C)), "window3_fwd: y overlaps x");
  const long long total = out_pix * (C / 4);
  if (mode == MUNIT_WINDOW_MAX)
    hipLaunchKernelGGL(window3_kernel<true>, dim3(grid_for(total)), dim3(NT), 0, (hipStream_t)stream, x, y, H, W, C / 4, x_ld,
                       y_ld, Ho, Wo, stride, pad, total);
  else
    hipLaunchKernelGGL(window3_kernel<false>, dim3(grid_for(total)), dim3(NT), 0, (hipStream_t)stream, x, y, H, W, C / 4, x_ld,
                       y_ld, Ho, Wo, stride, pad, total);
  MUNIT_CHECK_LAUNCH("window3_fwd");
  return MUNIT_OK;
}

extern "C" int munit_inception_input(const float* x, int layout, int B, int H, int W, float* y, munit_stream_t stream) {
  MUNIT_CHECK_ARG(x && y, "inception_input: null pointer");
  MUNIT_CHECK_ARG(layout == 0 || layout == 1, "inception_input: layout must be 0 (planar) or 1 (interleaved), got %d", layout);
  MUNIT_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "inception_input: B, H, W must be >= 1, got %d %d %d", B, H, W);
  const long long in_pix = (long long)B * H * W, total = (long long)B * OUT_HW * OUT_HW;
  MUNIT_CHECK_ARG(in_pix <= 0x7fffffffLL / 3 && total <= 0x7fffffffLL / 3, "inception_input: more than 2^31 elements");
  MUNIT_CHECK_ARG(!overlap(y, (size_t)total * 3 * sizeof(float), x, (size_t)in_pix * 3 * sizeof(float)),
                  "inception_input: y overlaps x");
  const long long hw = (long long)H * W;
  const long long sb = 3 * hw, sc = layout ? 1 : hw, sh = layout ? 3LL * W : W, sw = layout ? 3 : 1;
  hipLaunchKernelGGL(inception_input_kernel, dim3(grid_for(total)), dim3(NT), 0, (hipStream_t)stream, x, sb, sc, sh, sw, H, W, y,
                     total);
  MUNIT_CHECK_LAUNCH("inception_input");
  return MUNIT_OK;
}
