// Kernels of the frozen Resnet34_8s behind the semantic-consistency loss (scripts/trainer.py:706-771, scripts/utils.py:933-983,
// scripts/resnet.py): input transform, max-pool, basic-block tail, the space-to-batch re-layout that turns the dilated
// 3x3 convolutions of layer3 / layer4 into undilated ones, and the bilinear x8 + cross-entropy head.  The convolutions
// themselves run through munit_conv2d_* (BatchNorm folded into their weights at load time).  All passes are gathers: no
// atomics, so every result is bitwise reproducible.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int NCLS = 19;   // Cityscapes train ids (load_segmentation_model(ckpt, 19))

unsigned grid_for(long long n) { return (unsigned)std::max<long long>(1, std::min<long long>((n + NT - 1) / NT, 16384)); }

// ImageNet statistics of seg_transform (scripts/utils.py:165-174)
__constant__ float c_mean[3] = {0.485f, 0.456f, 0.406f};
__constant__ float c_std[3] = {0.229f, 0.224f, 0.225f};

__global__ void seg_input_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % 3);
    const float t = (x[i] + 1.f) / 2.f;
    y[i] = (t - c_mean[c]) / c_std[c];
  }
}
__global__ void seg_input_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % 3);
    dx[i] = dy[i] / c_std[c] / 2.f;
  }
}

// space-to-batch: y[(n*f + py)*f + px][i][j][c] = x[n][i*f + py][j*f + px][c]; inverse: x is phase-major, y plain
__global__ void relayout_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W, int C, int f,
                                int inverse) {
  const int Hs = H / f, Ws = W / f;
  const long long total = (long long)N * H * W * C;
  for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
    // o indexes the phase-major tensor [N*f*f][Hs][Ws][C]
    long long r = o;
    const int c = (int)(r % C); r /= C;
    const int j = (int)(r % Ws); r /= Ws;
    const int i = (int)(r % Hs); r /= Hs;
    const int px = (int)(r % f); r /= f;
    const int py = (int)(r % f); r /= f;
    const long long n = r;
    const long long s = (((n * H) + (long long)i * f + py) * W + (long long)j * f + px) * C + c;
    if (inverse) y[s] = x[o];   // x phase-major, y plain
    else y[o] = x[s];
  }
}

// 3x3 / stride 2 / pad 1 max-pool (nn.MaxPool2d(3, 2, 1), scripts/resnet.py).  Padding never wins (every window holds a
// real element).  Ties: the FIRST maximal element in window order (kh-major, then kw), as torch's kernels do; idx keeps
// that window position 0..8 for the backward and the parity audit.
__global__ void maxpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, unsigned char* __restrict__ idx,
                                   int B, int H, int W, int C, int Ho, int Wo) {
  const long long total = (long long)B * Ho * Wo * C;
  for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
    long long r = o;
    const int c = (int)(r % C); r /= C;
    const int ow = (int)(r % Wo); r /= Wo;
    const int oh = (int)(r % Ho); r /= Ho;
    const long long b = r;
    float best = 0.f;
    int bi = -1;
    for (int kh = 0; kh < 3; ++kh) {
      const int h = 2 * oh - 1 + kh;
      if (h < 0 || h >= H) continue;
      for (int kw = 0; kw < 3; ++kw) {
        const int w = 2 * ow - 1 + kw;
        if (w < 0 || w >= W) continue;
        const float v = x[((b * H + h) * W + w) * C + c];
        if (bi < 0 || v > best) {
          best = v;
          bi = kh * 3 + kw;
        }
      }
    }
    y[o] = best;
    idx[o] = (unsigned char)bi;
  }
}
// dx[h][w] = sum of dy over the windows whose recorded winner is (h, w), in fixed window order
__global__ void maxpool_bwd_kernel(const float* __restrict__ dy, const unsigned char* __restrict__ idx,
                                   float* __restrict__ dx, int B, int H, int W, int C, int Ho, int Wo) {
  const long long total = (long long)B * H * W * C;
  for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
    long long r = o;
    const int c = (int)(r % C); r /= C;
    const int w = (int)(r % W); r /= W;
    const int h = (int)(r % H); r /= H;
    const long long b = r;
    float acc = 0.f;
    for (int kh = 0; kh < 3; ++kh) {
      const int t = h + 1 - kh;
      if (t < 0 || (t & 1) || (t >> 1) >= Ho) continue;
      const int oh = t >> 1;
      for (int kw = 0; kw < 3; ++kw) {
        const int u = w + 1 - kw;
        if (u < 0 || (u & 1) || (u >> 1) >= Wo) continue;
        const long long q = ((b * Ho + oh) * Wo + (u >> 1)) * C + c;
        if (idx[q] == kh * 3 + kw) acc += dy[q];
      }
    }
    dx[o] = acc;
  }
}

// BasicBlock tail: y = relu(a + r)  (out += residual; out = relu(out), scripts/resnet.py)
__global__ void add_relu_kernel(const float* __restrict__ a, const float* __restrict__ r, float* __restrict__ y, long long n4) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const f32x4 s = ld4(a + 4 * i) + ld4(r + 4 * i);
    st4(y + 4 * i, f32x4{s[0] > 0.f ? s[0] : 0.f, s[1] > 0.f ? s[1] : 0.f, s[2] > 0.f ? s[2] : 0.f, s[3] > 0.f ? s[3] : 0.f});
  }
}

// F.interpolate(mode="bilinear", align_corners=False) from an h-long axis to H = h*S: source taps and weights of output
// coordinate o (torch's area_pixel_compute_source_index with scale h/H, clamped at 0)
struct Tap {
  int i0, i1;
  float l0, l1;
};
__device__ inline Tap tap_of(int o, int h, float scale) {
  float src = ((float)o + 0.5f) * scale - 0.5f;
  src = src < 0.f ? 0.f : src;
  Tap t;
  t.i0 = (int)src;
  t.i1 = t.i0 + (t.i0 < h - 1 ? 1 : 0);
  t.l1 = src - (float)t.i0;
  t.l0 = 1.f - t.l1;
  return t;
}
// the 19 up-sampled logits of one output pixel (torch's order: h0l * (w0l*v00 + w1l*v01) + h1l * (w0l*v10 + w1l*v11))
__device__ inline void up_logits(const float* __restrict__ lg, long long b, int h, int w, const Tap& ty, const Tap& tx,
                                 float* z) {
  const float* p00 = lg + ((b * h + ty.i0) * w + tx.i0) * NCLS;
  const float* p01 = lg + ((b * h + ty.i0) * w + tx.i1) * NCLS;
  const float* p10 = lg + ((b * h + ty.i1) * w + tx.i0) * NCLS;
  const float* p11 = lg + ((b * h + ty.i1) * w + tx.i1) * NCLS;
#pragma unroll
  for (int k = 0; k < NCLS; ++k)
    z[k] = ty.l0 * (tx.l0 * p00[k] + tx.l1 * p01[k]) + ty.l1 * (tx.l0 * p10[k] + tx.l1 * p11[k]);
}

// cross-entropy of one pixel (trainer.py:746-771).  Unmasked branch (mask == NULL): 19 classes.  Masked branch: logits
// (1-m)*z with m appended as the 20th logit, target (1-long(m))*label + long(m)*19.  g (optional) receives
// d loss / d z (19 values) for unit upstream gradient.
__device__ inline float pixel_ce(const float* z, int label, const float* mask, long long pix, float* g) {
  // fixed 20 entries so that every loop unrolls and zz stays in registers; the unmasked branch gives class 19 exp() = 0
  float zz[NCLS + 1];
  int t = label;
  float m = 0.f;
  if (mask) {
    m = mask[pix];
    const int ml = (int)m;
    t = (1 - ml) * label + ml * NCLS;
  }
#pragma unroll
  for (int k = 0; k < NCLS; ++k) zz[k] = mask ? (1.f - m) * z[k] : z[k];
  zz[NCLS] = mask ? m : -INFINITY;
  float mx = zz[0];
#pragma unroll
  for (int k = 1; k <= NCLS; ++k) mx = fmaxf(mx, zz[k]);
  float se = 0.f;
#pragma unroll
  for (int k = 0; k <= NCLS; ++k) se += expf(zz[k] - mx);
  const float lse = mx + logf(se);
  float zt = 0.f;
#pragma unroll
  for (int k = 0; k <= NCLS; ++k) zt = k == t ? zz[k] : zt;
  if (g) {
    const float sc = mask ? 1.f - m : 1.f;
#pragma unroll
    for (int k = 0; k < NCLS; ++k) g[k] = sc * (expf(zz[k] - lse) - (k == t ? 1.f : 0.f));
  }
  return lse - zt;
}

// What differs between the cross-entropy heads, per output pixel p = (b, y, x) with row / column taps ty / tx: loss() is the
// pixel's loss, grad() writes classes() values sc * d loss / d z at g[p * classes()].  Heads travel to the kernels by value;
// KC is seg_up_adjoint_kernel's.
struct PseudoHead {   // pseudo-labels (semantic_w)
  static constexpr int KC = NCLS;
  const int* labels;
  const float* mask;
  int classes() const { return NCLS; }
  __device__ inline float loss(const float* __restrict__ lg, long long b, int h, int w, const Tap& ty, const Tap& tx,
                               long long p) const {
    float z[NCLS];
    up_logits(lg, b, h, w, ty, tx, z);
    return pixel_ce(z, labels[p], mask, p, nullptr);
  }
  __device__ inline void grad(const float* __restrict__ lg, long long b, int h, int w, const Tap& ty, const Tap& tx,
                              long long p, float sc, float* __restrict__ g) const {
    float z[NCLS], d[NCLS];
    up_logits(lg, b, h, w, ty, tx, z);
    pixel_ce(z, labels[p], mask, p, d);
#pragma unroll
    for (int k = 0; k < NCLS; ++k) g[p * NCLS + k] = sc * d[k];
  }
};
// ---- cross-entropy against a ground-truth map of the simulator's 10 classes (trainer.py:732-737, utils.py:1330-1353) ----
constexpr int NMRG = 10;
// cross-entropy of one pixel on the 19 logits merged into 10: merged class 0 is the constant 0, the others the sums of
// their Cityscapes members.  Unmasked branch (mask == NULL): 10 classes.  Masked branch: logits (1-m)*merged with m
// appended as the 11th logit, target (1-long(m))*gt + long(m)*10.  gt is the loader's float label, truncated like
// .type(torch.long); no array is ever indexed by it.  A label outside 0..9 (or NaN / inf) makes the pixel's loss NaN and
// its gradient 0.  g (optional) receives d loss / d z (19 values: a merged class's gradient goes to each member).
__device__ inline float pixel_ce_gt(const float* z, float gt, const float* mask, long long pix, float* g) {
  // fixed 11 entries so that every loop unrolls and zz stays in registers; the unmasked branch gives class 10 exp() = 0
  float zz[NMRG + 1];
  zz[0] = 0.f;
  zz[1] = z[0] + z[1];
  zz[2] = z[2] + z[3] + z[4];
  zz[3] = z[5] + z[6] + z[7];
  zz[4] = z[8];
  zz[5] = z[9];
  zz[6] = z[10];
  zz[7] = z[11] + z[12];
  zz[8] = z[13] + z[17] + z[18];
  zz[9] = z[14] + z[15] + z[16];
  const bool ok = gt > -1.f && gt < (float)NMRG;     // what truncates into 0..9; false for NaN
  int t = ok ? (int)gt : -1;
  float m = 0.f;
  if (mask) {
    m = mask[pix];
    const int ml = (int)m;
    t = ok ? (1 - ml) * t + ml * NMRG : -1;
#pragma unroll
    for (int k = 0; k < NMRG; ++k) zz[k] = (1.f - m) * zz[k];
  }
  zz[NMRG] = mask ? m : -INFINITY;
  float mx = zz[0];
#pragma unroll
  for (int k = 1; k <= NMRG; ++k) mx = fmaxf(mx, zz[k]);
  float se = 0.f;
#pragma unroll
  for (int k = 0; k <= NMRG; ++k) se += expf(zz[k] - mx);
  const float lse = mx + logf(se);
  float zt = 0.f;
#pragma unroll
  for (int k = 0; k <= NMRG; ++k) zt = k == t ? zz[k] : zt;
  if (g) {
    const float sc = ok ? (mask ? 1.f - m : 1.f) : 0.f;
    float dm[NMRG];      // entry 0 (the constant class) is never read
#pragma unroll
    for (int k = 1; k < NMRG; ++k) dm[k] = sc * (expf(zz[k] - lse) - (k == t ? 1.f : 0.f));
    g[0] = g[1] = dm[1];
    g[2] = g[3] = g[4] = dm[2];
    g[5] = g[6] = g[7] = dm[3];
    g[8] = dm[4];
    g[9] = dm[5];
    g[10] = dm[6];
    g[11] = g[12] = dm[7];
    g[13] = g[17] = g[18] = dm[8];
    g[14] = g[15] = g[16] = dm[9];
  }
  return ok ? lse - zt : NAN;
}

struct GtHead {   // 10-class ground truth (semantic_gt)
  static constexpr int KC = NCLS;
  const float* gt;
  const float* mask;
  int classes() const { return NCLS; }
  __device__ inline float loss(const float* __restrict__ lg, long long b, int h, int w, const Tap& ty, const Tap& tx,
                               long long p) const {
    float z[NCLS];
    up_logits(lg, b, h, w, ty, tx, z);
    return pixel_ce_gt(z, gt[p], mask, p, nullptr);
  }
  __device__ inline void grad(const float* __restrict__ lg, long long b, int h, int w, const Tap& ty, const Tap& tx,
                              long long p, float sc, float* __restrict__ g) const {
    float z[NCLS], d[NCLS];
    up_logits(lg, b, h, w, ty, tx, z);
    pixel_ce_gt(z, gt[p], mask, p, d);
#pragma unroll
    for (int k = 0; k < NCLS; ++k) g[p * NCLS + k] = sc * d[k];
  }
};

// adjoint of the bilinear up-sample as a gather: dl[b][i][j][k] = sum over the output pixels whose taps touch (i, j), in
// fixed row / column order (the taps of row y reach i0(y) <= i <= i0(y) + 1, so y lies within S rows of [i*S, (i+1)*S))
template <int KC>   // KC: the class count when it is a compile-time constant, 0: the run-time value Krt
__global__ void seg_up_adjoint_kernel(const float* __restrict__ g, int B, int h, int w, int S, int Krt, float* __restrict__ dl) {
  const int NCLS = KC ? KC : Krt;
  const int H = h * S, W = w * S;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  const long long total = (long long)B * h * w * NCLS;
  for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
    long long r = o;
    const int k = (int)(r % NCLS); r /= NCLS;
    const int j = (int)(r % w); r /= w;
    const int i = (int)(r % h); r /= h;
    const long long b = r;
    const int y0 = max(0, (i - 1) * S), y1 = min(H, (i + 2) * S);
    const int x0 = max(0, (j - 1) * S), x1 = min(W, (j + 2) * S);
    float acc = 0.f;
    for (int y = y0; y < y1; ++y) {
      const Tap ty = tap_of(y, h, sy);
      if (ty.i0 != i && ty.i1 != i) continue;
      const float wy = (ty.i0 == i ? ty.l0 : 0.f) + (ty.i1 == i ? ty.l1 : 0.f);
      float row = 0.f;
      for (int x = x0; x < x1; ++x) {
        const Tap tx = tap_of(x, w, sx);
        if (tx.i0 != j && tx.i1 != j) continue;
        const float wx = (tx.i0 == j ? tx.l0 : 0.f) + (tx.i1 == j ? tx.l1 : 0.f);
        row += wx * g[(((b * H) + y) * W + x) * NCLS + k];
      }
      acc += wy * row;
    }
    dl[o] = acc;
  }
}

// ---- K-class head of the trainable segmentation head (trainer.py:1303-1318): plain cross-entropy, no mask, no merge ----
// One class at a time, recomputing the up-sampled logit in each of the passes (no K-entry array: K is a run-time value and
// the kernel stays free of scratch); tap order as up_logits.
struct Taps4 {
  const float *p00, *p01, *p10, *p11;
  float y0, y1, x0, x1;
  __device__ inline float at(int k) const { return y0 * (x0 * p00[k] + x1 * p01[k]) + y1 * (x0 * p10[k] + x1 * p11[k]); }
};
__device__ inline Taps4 taps_of(const float* __restrict__ lg, long long b, int h, int w, int K, const Tap& ty, const Tap& tx) {
  Taps4 t;
  t.p00 = lg + ((b * h + ty.i0) * w + tx.i0) * K;
  t.p01 = lg + ((b * h + ty.i0) * w + tx.i1) * K;
  t.p10 = lg + ((b * h + ty.i1) * w + tx.i0) * K;
  t.p11 = lg + ((b * h + ty.i1) * w + tx.i1) * K;
  t.y0 = ty.l0, t.y1 = ty.l1, t.x0 = tx.l0, t.x1 = tx.l1;
  return t;
}
// log-sum-exp of the K up-sampled logits and the target's logit.  gt: the loader's float label, truncated like
// .type(torch.long) and never used as an index; ok is false for a label outside 0..K-1, NaN or infinite.
__device__ inline float direct_lse(const Taps4& t, int K, float gt, bool* ok, int* tgt, float* zt) {
  *ok = gt > -1.f && gt < (float)K;
  *tgt = *ok ? (int)gt : -1;
  float mx = t.at(0);
  for (int k = 1; k < K; ++k) mx = fmaxf(mx, t.at(k));
  float se = 0.f, z_t = 0.f;
  for (int k = 0; k < K; ++k) {
    const float z = t.at(k);
    se += expf(z - mx);
    z_t = k == *tgt ? z : z_t;
  }
  *zt = z_t;
  return mx + logf(se);
}
struct DirectHead {   // K-class head (sem_seg_lambda)
  static constexpr int KC = 0;
  const float* gt;
  int K;
  int classes() const { return K; }
  __device__ inline float loss(const float* __restrict__ lg, long long b, int h, int w, const Tap& ty, const Tap& tx,
                               long long p) const {
    const Taps4 t = taps_of(lg, b, h, w, K, ty, tx);
    bool ok;
    int tgt;
    float zt;
    const float lse = direct_lse(t, K, gt[p], &ok, &tgt, &zt);
    return ok ? lse - zt : NAN;
  }
  __device__ inline void grad(const float* __restrict__ lg, long long b, int h, int w, const Tap& ty, const Tap& tx,
                              long long p, float sc, float* __restrict__ g) const {
    const Taps4 t = taps_of(lg, b, h, w, K, ty, tx);
    bool ok;
    int tgt;
    float zt;
    const float lse = direct_lse(t, K, gt[p], &ok, &tgt, &zt);
    for (int k = 0; k < K; ++k) g[p * K + k] = ok ? sc * (expf(t.at(k) - lse) - (k == tgt ? 1.f : 0.f)) : 0.f;
  }
};

// per-block partial sums of the head's pixel losses over pixels [0, npix)
template <class Head>
__global__ void seg_ce_loss_kernel(Head hd, const float* __restrict__ lg, int B, int h, int w, int S, float* __restrict__ part) {
  __shared__ float red[NT / 64];
  const int H = h * S, W = w * S;
  const long long npix = (long long)B * H * W;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  float acc = 0.f;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(p % W);
    const int y = (int)((p / W) % H);
    const long long b = p / ((long long)W * H);
    acc += hd.loss(lg, b, h, w, tap_of(y, h, sy), tap_of(x, w, sx), p);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < NT / 64; ++i) s += red[i];
    part[blockIdx.x] = s;
  }
}
__global__ void seg_ce_final_kernel(const float* __restrict__ part, int nb, double inv_n, float* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < nb; ++i) s += (double)part[i];
    *out = (float)(s * inv_n);
  }
}
// g[p][k] = gout/n * d ce(p) / d z_k at the up-sampled resolution
template <class Head>
__global__ void seg_ce_grad_kernel(Head hd, const float* __restrict__ lg, int B, int h, int w, int S,
                                   const float* __restrict__ gout, float inv_n, float* __restrict__ g) {
  const int H = h * S, W = w * S;
  const long long npix = (long long)B * H * W;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  const float sc = *gout * inv_n;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(p % W);
    const int y = (int)((p / W) % H);
    const long long b = p / ((long long)W * H);
    hd.grad(lg, b, h, w, tap_of(y, h, sy), tap_of(x, w, sx), p, sc, g);
  }
}

// ---- nn.AvgPool2d(7, stride 1, padding 3), padding counted: y = (sum of x over the 7x7 window clipped to the map) / 49 ----
// One thread owns 4 channels of one column over a strip of POOL_ROWS rows: per input row it forms the 7-tap row sum
// (7 16-byte reads, consecutive lanes on consecutive channels) and keeps the last 7 row sums in registers; every output is
// the sum of those 7 in fixed order (no subtraction, so no drift along the strip).  The operator is symmetric: its own adjoint.
constexpr int POOL_ROWS = 8;
constexpr int POOL_GRID_CAP = 2048;
__global__ void avgpool7_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int H, int W, int C) {
  const int CG = C / 4;
  const int strips = (H + POOL_ROWS - 1) / POOL_ROWS;
  const long long total = (long long)B * strips * W * CG;
  for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
    long long r = o;
    const int cg = (int)(r % CG); r /= CG;
    const int j = (int)(r % W); r /= W;
    const int s = (int)(r % strips); r /= strips;
    const long long b = r;
    const int r0 = s * POOL_ROWS, r1 = min(H, r0 + POOL_ROWS);
    const int j0 = max(0, j - 3), j1 = min(W - 1, j + 3);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 q0 = zero, q1 = zero, q2 = zero, q3 = zero, q4 = zero, q5 = zero, q6 = zero;
    for (int ii = r0 - 3; ii < r1 + 3; ++ii) {
      f32x4 hs = zero;
      if (ii >= 0 && ii < H) {
        const float* row = x + ((b * H + ii) * W) * (long long)C + 4 * cg;
        for (int jj = j0; jj <= j1; ++jj) hs += ld4(row + (long long)jj * C);
      }
      q0 = q1, q1 = q2, q2 = q3, q3 = q4, q4 = q5, q5 = q6, q6 = hs;
      const int i = ii - 3;
      if (i >= r0) st4(y + ((b * H + i) * W + j) * (long long)C + 4 * cg, (((((q0 + q1) + q2) + q3) + q4) + q5 + q6) / 49.f);
    }
  }
}

// argmax over the 19 up-sampled logits (first maximal class on ties: torch's max(1)[1])
__global__ void seg_labels_kernel(const float* __restrict__ lg, int B, int h, int w, int S, int* __restrict__ labels) {
  const int H = h * S, W = w * S;
  const long long npix = (long long)B * H * W;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(p % W);
    const int y = (int)((p / W) % H);
    const long long b = p / ((long long)W * H);
    // one class at a time (no 19-entry array: keeps the kernel free of spills)
    const Taps4 t = taps_of(lg, b, h, w, NCLS, tap_of(y, h, sy), tap_of(x, w, sx));
    int best = 0;
    float bz = 0.f;
    for (int k = 0; k < NCLS; ++k) {
      const float zk = t.at(k);
      if (k == 0 || zk > bz) {
        best = k;
        bz = zk;
      }
    }
    labels[p] = best;
  }
}

int check_head(const float* lg, const void* labels, int B, int h, int w, int S) {
  MUNIT_CHECK_ARG(lg && labels && B > 0 && h > 0 && w > 0 && S > 0, "seg head: bad args");
  MUNIT_CHECK_ARG((long long)B * h * S * w * S * NCLS < (1ll << 40), "seg head: too large");
  return MUNIT_OK;
}
long long head_pix(int B, int h, int w, int S) { return (long long)B * h * S * w * S; }

// Forward of a cross-entropy head: per-block partials of the pixel losses in ws, then their sum / norm in out.
template <class Head>
int launch_ce_fwd(const char* what, Head hd, const float* logits, int B, int h, int w, int S, float norm, float* out, void* ws,
                  size_t ws_bytes, munit_stream_t stream) {
  MUNIT_CHECK_ARG(out && ws && norm > 0.f, "%s: bad args", what);
  const long long np = head_pix(B, h, w, S);
  const unsigned nb = grid_for(np);
  if (ws_bytes < (size_t)nb * sizeof(float)) {
    munit_set_error("%s: workspace %zu < %zu", what, ws_bytes, (size_t)nb * sizeof(float));
    return MUNIT_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  float* part = reinterpret_cast<float*>(ws);
  hipLaunchKernelGGL(seg_ce_loss_kernel<Head>, dim3(nb), dim3(NT), 0, st, hd, logits, B, h, w, S, part);
  MUNIT_CHECK_LAUNCH(what);
  hipLaunchKernelGGL(seg_ce_final_kernel, dim3(1), dim3(64), 0, st, part, (int)nb, 1.0 / (double)norm, out);
  MUNIT_CHECK_LAUNCH("seg_ce_final");
  return MUNIT_OK;
}
// Backward: the full-resolution pixel gradients in ws, then the up-sample's adjoint into dlogits.
template <class Head>
int launch_ce_bwd(const char* what, Head hd, const float* logits, int B, int h, int w, int S, float norm, const float* gout,
                  float* dlogits, void* ws, size_t ws_bytes, munit_stream_t stream) {
  MUNIT_CHECK_ARG(gout && dlogits && ws && norm > 0.f, "%s: bad args", what);
  const long long np = head_pix(B, h, w, S);
  const int K = hd.classes();
  const size_t need = (size_t)np * K * sizeof(float);
  if (ws_bytes < need) {
    munit_set_error("%s: workspace %zu < %zu", what, ws_bytes, need);
    return MUNIT_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  float* g = reinterpret_cast<float*>(ws);
  hipLaunchKernelGGL(seg_ce_grad_kernel<Head>, dim3(grid_for(np)), dim3(NT), 0, st, hd, logits, B, h, w, S, gout, 1.f / norm, g);
  MUNIT_CHECK_LAUNCH(what);
  hipLaunchKernelGGL(seg_up_adjoint_kernel<Head::KC>, dim3(grid_for((long long)B * h * w * K)), dim3(NT), 0, st, g, B, h, w, S,
                     K, dlogits);
  MUNIT_CHECK_LAUNCH("seg_up_adjoint");
  return MUNIT_OK;
}

}  // namespace

extern "C" int munit_seg_input_fwd(const float* x, float* y, size_t npix, munit_stream_t stream) {
  MUNIT_CHECK_ARG(x && y, "seg_input_fwd: null pointer");
  if (npix == 0) return MUNIT_OK;
  const long long n = 3ll * (long long)npix;
  hipLaunchKernelGGL(seg_input_fwd_kernel, dim3(grid_for(n)), dim3(NT), 0, (hipStream_t)stream, x, y, n);
  MUNIT_CHECK_LAUNCH("seg_input_fwd");
  return MUNIT_OK;
}

extern "C" int munit_seg_input_bwd(const float* dy, float* dx, size_t npix, munit_stream_t stream) {
  MUNIT_CHECK_ARG(dy && dx, "seg_input_bwd: null pointer");
  if (npix == 0) return MUNIT_OK;
  const long long n = 3ll * (long long)npix;
  hipLaunchKernelGGL(seg_input_bwd_kernel, dim3(grid_for(n)), dim3(NT), 0, (hipStream_t)stream, dy, dx, n);
  MUNIT_CHECK_LAUNCH("seg_input_bwd");
  return MUNIT_OK;
}

extern "C" int munit_space_to_batch(const float* x, float* y, int N, int H, int W, int C, int f, int inverse,
                                    munit_stream_t stream) {
  MUNIT_CHECK_ARG(x && y && x != y && N > 0 && H > 0 && W > 0 && C > 0 && f >= 1, "space_to_batch: bad args");
  MUNIT_CHECK_ARG(H % f == 0 && W % f == 0, "space_to_batch: %dx%d not a multiple of %d", H, W, f);
  MUNIT_CHECK_ARG(inverse == 0 || inverse == 1, "space_to_batch: inverse must be 0 or 1");
  const long long n = (long long)N * H * W * C;
  hipLaunchKernelGGL(relayout_kernel, dim3(grid_for(n)), dim3(NT), 0, (hipStream_t)stream, x, y, N, H, W, C, f, inverse);
  MUNIT_CHECK_LAUNCH("space_to_batch");
  return MUNIT_OK;
}

extern "C" int munit_maxpool3s2_fwd(const float* x, float* y, unsigned char* idx, int B, int H, int W, int C,
                                    munit_stream_t stream) {
  MUNIT_CHECK_ARG(x && y && idx && B > 0 && H > 0 && W > 0 && C > 0, "maxpool_fwd: bad args");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(grid_for((long long)B * Ho * Wo * C)), dim3(NT), 0, (hipStream_t)stream, x, y,
                     idx, B, H, W, C, Ho, Wo);
  MUNIT_CHECK_LAUNCH("maxpool_fwd");
  return MUNIT_OK;
}

extern "C" int munit_maxpool3s2_bwd(const float* dy, const unsigned char* idx, float* dx, int B, int H, int W, int C,
                                    munit_stream_t stream) {
  MUNIT_CHECK_ARG(dy && idx && dx && B > 0 && H > 0 && W > 0 && C > 0, "maxpool_bwd: bad args");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(grid_for((long long)B * H * W * C)), dim3(NT), 0, (hipStream_t)stream, dy, idx,
                     dx, B, H, W, C, Ho, Wo);
  MUNIT_CHECK_LAUNCH("maxpool_bwd");
  return MUNIT_OK;
}

extern "C" int munit_add_relu_fwd(const float* a, const float* r, float* y, size_t n, munit_stream_t stream) {
  MUNIT_CHECK_ARG(a && r && y && n % 4 == 0, "add_relu_fwd: bad args (n %% 4 == 0)");
  if (n == 0) return MUNIT_OK;
  hipLaunchKernelGGL(add_relu_kernel, dim3(grid_for((long long)n / 4)), dim3(NT), 0, (hipStream_t)stream, a, r, y,
                     (long long)n / 4);
  MUNIT_CHECK_LAUNCH("add_relu_fwd");
  return MUNIT_OK;
}

extern "C" size_t munit_seg_ce_workspace_bytes(int B, int h, int w, int S) {
  return munit_seg_ce_direct_workspace_bytes(B, h, w, S, NCLS);
}

extern "C" int munit_seg_ce_fwd(const float* logits, const int* labels, const float* mask, int B, int h, int w, int S,
                                float norm, float* out, void* ws, size_t ws_bytes, munit_stream_t stream) {
  int rc = check_head(logits, labels, B, h, w, S);
  if (rc) return rc;
  return launch_ce_fwd("seg_ce_fwd", PseudoHead{labels, mask}, logits, B, h, w, S, norm, out, ws, ws_bytes, stream);
}

extern "C" int munit_seg_ce_bwd(const float* logits, const int* labels, const float* mask, int B, int h, int w, int S,
                                float norm, const float* gout, float* dlogits, void* ws, size_t ws_bytes,
                                munit_stream_t stream) {
  int rc = check_head(logits, labels, B, h, w, S);
  if (rc) return rc;
  return launch_ce_bwd("seg_ce_bwd", PseudoHead{labels, mask}, logits, B, h, w, S, norm, gout, dlogits, ws, ws_bytes, stream);
}

extern "C" int munit_seg_labels(const float* logits, int B, int h, int w, int S, int* labels, munit_stream_t stream) {
  int rc = check_head(logits, labels, B, h, w, S);
  if (rc) return rc;
  const long long np = head_pix(B, h, w, S);
  hipLaunchKernelGGL(seg_labels_kernel, dim3(grid_for(np)), dim3(NT), 0, (hipStream_t)stream, logits, B, h, w, S, labels);
  MUNIT_CHECK_LAUNCH("seg_labels");
  return MUNIT_OK;
}

// The same head against a ground-truth map (see pixel_ce_gt)
extern "C" int munit_seg_ce_gt_fwd(const float* logits, const float* gt, const float* mask, int B, int h, int w, int S,
                                   float norm, float* out, void* ws, size_t ws_bytes, munit_stream_t stream) {
  int rc = check_head(logits, gt, B, h, w, S);
  if (rc) return rc;
  return launch_ce_fwd("seg_ce_gt_fwd", GtHead{gt, mask}, logits, B, h, w, S, norm, out, ws, ws_bytes, stream);
}

extern "C" int munit_seg_ce_gt_bwd(const float* logits, const float* gt, const float* mask, int B, int h, int w, int S,
                                   float norm, const float* gout, float* dlogits, void* ws, size_t ws_bytes,
                                   munit_stream_t stream) {
  int rc = check_head(logits, gt, B, h, w, S);
  if (rc) return rc;
  return launch_ce_bwd("seg_ce_gt_bwd", GtHead{gt, mask}, logits, B, h, w, S, norm, gout, dlogits, ws, ws_bytes, stream);
}

// ---- trainable segmentation head (adaptation.sem_seg_lambda) ----
namespace {
int check_pool(const float* x, const float* y, int B, int H, int W, int C, const char* what) {
  MUNIT_CHECK_ARG(x && y && x != y && B > 0 && H > 0 && W > 0 && C > 0, "%s: bad args", what);
  MUNIT_CHECK_ARG(C % 4 == 0, "%s: C %% 4 == 0 required, got %d", what, C);
  MUNIT_CHECK_ARG((long long)B * H * W * C < (1ll << 40), "%s: too large", what);
  return MUNIT_OK;
}
void launch_pool(const float* x, float* y, int B, int H, int W, int C, hipStream_t st) {
  const long long n = (long long)B * ((H + POOL_ROWS - 1) / POOL_ROWS) * W * (C / 4);
  const unsigned nb = (unsigned)std::max<long long>(1, std::min<long long>((n + NT - 1) / NT, POOL_GRID_CAP));
  hipLaunchKernelGGL(avgpool7_kernel, dim3(nb), dim3(NT), 0, st, x, y, B, H, W, C);
}
int check_direct(const float* lg, const float* gt, int B, int h, int w, int S, int K, const char* what) {
  MUNIT_CHECK_ARG(lg && gt && B > 0 && h > 0 && w > 0, "%s: bad args", what);
  MUNIT_CHECK_ARG(S == 1 || S == 2 || S == 4 || S == 8, "%s: scale must be 1, 2, 4 or 8, got %d", what, S);
  MUNIT_CHECK_ARG(K >= 2 && K <= 32, "%s: 2..32 classes, got %d", what, K);
  MUNIT_CHECK_ARG((long long)B * h * S * w * S * K < (1ll << 40), "%s: too large", what);
  return MUNIT_OK;
}
}  // namespace

extern "C" int munit_avgpool7_fwd(const float* x, float* y, int B, int H, int W, int C, munit_stream_t stream) {
  int rc = check_pool(x, y, B, H, W, C, "avgpool7_fwd");
  if (rc) return rc;
  launch_pool(x, y, B, H, W, C, (hipStream_t)stream);
  MUNIT_CHECK_LAUNCH("avgpool7_fwd");
  return MUNIT_OK;
}

extern "C" int munit_avgpool7_bwd(const float* dy, float* dx, int B, int H, int W, int C, munit_stream_t stream) {
  int rc = check_pool(dy, dx, B, H, W, C, "avgpool7_bwd");
  if (rc) return rc;
  launch_pool(dy, dx, B, H, W, C, (hipStream_t)stream);      // symmetric windows: the operator is its own adjoint
  MUNIT_CHECK_LAUNCH("avgpool7_bwd");
  return MUNIT_OK;
}

extern "C" size_t munit_seg_ce_direct_workspace_bytes(int B, int h, int w, int S, int K) {
  const long long np = head_pix(B, h, w, S);
  const size_t part = align_up((size_t)grid_for(np) * sizeof(float), 256);
  const size_t grad = align_up((size_t)np * K * sizeof(float), 256);
  return std::max(part, grad);
}

extern "C" int munit_seg_ce_direct_fwd(const float* logits, const float* gt, int B, int h, int w, int S, int K, float norm,
                                       float* out, void* ws, size_t ws_bytes, munit_stream_t stream) {
  int rc = check_direct(logits, gt, B, h, w, S, K, "seg_ce_direct_fwd");
  if (rc) return rc;
  return launch_ce_fwd("seg_ce_direct_fwd", DirectHead{gt, K}, logits, B, h, w, S, norm, out, ws, ws_bytes, stream);
}

extern "C" int munit_seg_ce_direct_bwd(const float* logits, const float* gt, int B, int h, int w, int S, int K, float norm,
                                       const float* gout, float* dlogits, void* ws, size_t ws_bytes, munit_stream_t stream) {
  int rc = check_direct(logits, gt, B, h, w, S, K, "seg_ce_direct_bwd");
  if (rc) return rc;
  return launch_ce_bwd("seg_ce_direct_bwd", DirectHead{gt, K}, logits, B, h, w, S, norm, gout, dlogits, ws, ws_bytes, stream);
}
