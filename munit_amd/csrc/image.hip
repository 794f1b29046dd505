// Input pipeline on the device: the per-image transform chain of the reference's loaders
//   RandomHorizontalFlip -> Resize(new_size) -> RandomCrop(h, w) -> ToTensor -> Normalize(0.5, 0.5)
// (scripts/utils.py:192-250, 680-740; MyDataset.transform utils.py:296-345) applied to a batch of
// decoded uint8 images of different sizes in one pass, writing the normalised NHWC float batch the
// convolutions read.  Only the crop window is ever computed.
//
// Resize arithmetic is Pillow's (the reference calls PIL through torchvision; requirements.txt pins
// Pillow==6.2.0, same resampler as today's): ImagingResample with the BILINEAR filter -- a separable
// anti-aliased triangle filter, coefficients computed in double and rounded to 22-bit fixed point,
// horizontal pass then vertical pass with a uint8 rounding between them -- restated here so that the
// result is bit-identical to Image.resize.  Masks use the NEAREST path (ImagingScaleAffine: source
// index tables from a running double accumulator); so do the mask and the label maps of the synthetic
// pairs (MyDatasetSynthetic.transform, utils.py:483-553), whose chain differs: munit_label_preprocess.
//
// The way out is here too: munit_image_grid_u8 turns a list of float image batches into the uint8 sample grid that the
// reference's write_2images saves (utils.py:768-814: torchvision's make_grid(normalize=True, padding=0) and save_image's
// x255 + 0.5), byte for byte what torch's op sequence gives on the device.
#include "common.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;

__device__ inline double bilinear_filter(double x) {
  if (x < 0.0) x = -x;
  if (x < 1.0) return 1.0 - x;
  return 0.0;
}

__device__ inline int clip8(int v) {
  v >>= PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// One thread per (sample, axis, output index of the crop window): window start, length and the
// fixed-point coefficients of Pillow's precompute_coeffs + normalize_coeffs_8bpc.
//   tab layout per sample: [rows: out_h x (2 + ksize)] [cols: out_w x (2 + ksize)] ints
__global__ void resample_tables_kernel(const munit_image_desc* __restrict__ descs, int B, int out_h, int out_w,
                                       int ksize_max, int* __restrict__ tab) {
  const int per = (out_h + out_w) * (2 + ksize_max);
  const int total = B * (out_h + out_w);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int b = i / (out_h + out_w);
    const int r = i - b * (out_h + out_w);
    const munit_image_desc d = descs[b];
    const bool is_row = r < out_h;
    const int in_size = is_row ? d.src_h : d.src_w;
    const int rs_size = is_row ? d.rs_h : d.rs_w;
    const int xx = is_row ? d.crop_i + r : d.crop_j + (r - out_h);   // index in the resized image
    int* t = tab + (long long)b * per + (long long)r * (2 + ksize_max);

    const double scale = (double)in_size / (double)rs_size;
    double filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 1.0 * filterscale;
    const double center = 0.0 + (xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    if (xmax > ksize_max) xmax = ksize_max;   // cannot happen when the host sized ksize_max from the same formula
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += bilinear_filter((x + xmin - center + 0.5) * ss);
    t[0] = xmin;
    t[1] = xmax;
    for (int x = 0; x < ksize_max; ++x) {
      int c = 0;
      if (x < xmax) {
        double w = bilinear_filter((x + xmin - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        c = w < 0.0 ? (int)(-0.5 + w * (double)(1 << PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << PRECISION_BITS));
      }
      t[2 + x] = c;
    }
  }
}

// One thread per output pixel: horizontal pass over the rows of its vertical window (each rounded to
// uint8 as Pillow's intermediate image is), vertical pass, then ToTensor (/255) and Normalize
// ((t - 0.5) / 0.5) in fp32 -- the same operation order as torchvision, so the floats match bit for bit.
__global__ void image_resample_kernel(const unsigned char* __restrict__ pool,
                                      const munit_image_desc* __restrict__ descs, int B, int out_h, int out_w,
                                      int ksize_max, const int* __restrict__ tab, float* __restrict__ out) {
  const int per = (out_h + out_w) * (2 + ksize_max);
  const long long total = (long long)B * out_h * out_w;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / ((long long)out_h * out_w));
    const int rem = (int)(i - (long long)b * out_h * out_w);
    const int y = rem / out_w, x = rem - y * out_w;
    const munit_image_desc d = descs[b];
    const unsigned char* src = pool + d.src_off;
    const int* ty = tab + (long long)b * per + (long long)y * (2 + ksize_max);
    const int* tx = tab + (long long)b * per + (long long)(out_h + x) * (2 + ksize_max);
    const int ymin = ty[0], ymax = ty[1], xmin = tx[0], xmax = tx[1];
    int v0 = 1 << (PRECISION_BITS - 1), v1 = v0, v2 = v0;
    for (int yy = 0; yy < ymax; ++yy) {
      const unsigned char* row = src + (long long)(ymin + yy) * d.src_w * 3;
      int h0 = 1 << (PRECISION_BITS - 1), h1 = h0, h2 = h0;
      for (int k = 0; k < xmax; ++k) {
        int sx = xmin + k;
        if (d.flip) sx = d.src_w - 1 - sx;
        const int c = tx[2 + k];
        h0 += row[sx * 3 + 0] * c;
        h1 += row[sx * 3 + 1] * c;
        h2 += row[sx * 3 + 2] * c;
      }
      const int cy = ty[2 + yy];
      v0 += clip8(h0) * cy;
      v1 += clip8(h1) * cy;
      v2 += clip8(h2) * cy;
    }
    float* o = out + i * 3;
    o[0] = (__fdiv_rn((float)clip8(v0), 255.f) - 0.5f) / 0.5f;
    o[1] = (__fdiv_rn((float)clip8(v1), 255.f) - 0.5f) / 0.5f;
    o[2] = (__fdiv_rn((float)clip8(v2), 255.f) - 0.5f) / 0.5f;
  }
}

// NEAREST index tables (ImagingScaleAffine): one thread per (sample, axis) walks xo += a0 in double.
//   tab layout per sample: [out_h row indices][out_w column indices] (-1 = no source pixel)
// windowed 0 (munit_mask_preprocess): the plane is resized to (out_w, out_h) and the table covers all of it.
// windowed 1 (munit_label_preprocess): the plane is resized to the descriptor's (rs_w, rs_h) and the table keeps
// the window [crop, crop + out) of that walk.  The accumulator always starts at index 0: (x + 0.5) * a rounds
// differently from the running sum, and Pillow uses the running sum.  Window positions outside [0, rs) get -1.
__global__ void nearest_tables_kernel(const munit_image_desc* __restrict__ descs, int B, int out_h, int out_w,
                                      int windowed, int* __restrict__ tab) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * B) return;
  const int b = i >> 1;
  const bool is_row = (i & 1) == 0;
  const munit_image_desc d = descs[b];
  const int in_size = is_row ? d.src_h : d.src_w;
  const int n = is_row ? out_h : out_w;
  const int rs = windowed ? (is_row ? d.rs_h : d.rs_w) : n;
  const int crop = windowed ? (is_row ? d.crop_i : d.crop_j) : 0;
  int* t = tab + (long long)b * (out_h + out_w) + (is_row ? 0 : out_h);
  if (windowed)
    for (int x = 0; x < n; ++x) t[x] = -1;
  long long end = (long long)crop + n;
  if (end > rs) end = rs;
  const double a = (double)in_size / (double)rs;
  double xo = 0.0 + a * 0.5;
  for (long long x = 0; x < end; ++x) {
    if (x >= crop) {
      const int xin = xo < 0.0 ? -1 : (int)xo;
      t[x - crop] = (xin >= 0 && xin < in_size) ? xin : -1;
    }
    xo += a;
  }
}

// Mask chain of MyDataset.transform (utils.py:318-330): flip, NEAREST resize of the whole mask to the
// crop size (width, height), then crop((j, i, j+w, i+h)) of that image -- positions past its edge read 0
// (PIL crop semantics; the reference crops the already crop-sized mask at the image's offsets) -- and
// the per-sample maximum for the "max == 1 -> x255" rule.
__global__ void mask_gather_kernel(const unsigned char* __restrict__ pool, const munit_image_desc* __restrict__ descs,
                                   int B, int out_h, int out_w, const int* __restrict__ tab,
                                   float* __restrict__ out, int* __restrict__ vmax) {
  const long long total = (long long)B * out_h * out_w;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / ((long long)out_h * out_w));
    const int rem = (int)(i - (long long)b * out_h * out_w);
    const int y = rem / out_w, x = rem - y * out_w;
    const munit_image_desc d = descs[b];
    const int my = y + d.crop_i, mx = x + d.crop_j;
    int v = 0;
    if (my < out_h && mx < out_w) {
      const int* t = tab + (long long)b * (out_h + out_w);
      const int sy = t[my];
      int sx = t[out_h + mx];
      if (sy >= 0 && sx >= 0) {
        if (d.flip) sx = d.src_w - 1 - sx;
        v = pool[d.src_off + (long long)sy * d.src_w + sx];
      }
    }
    out[i] = (float)v;
    if (v > 0) atomicMax(&vmax[b], v);
  }
}

__global__ void mask_scale_kernel(float* __restrict__ out, const int* __restrict__ vmax, int B, int hw) {
  const long long total = (long long)B * hw;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / hw);
    float t = __fdiv_rn(out[i], 255.f);       // ToTensor
    if (vmax[b] == 1) t = t * 255.f;          // utils.py:326-329
    out[i] = t;
  }
}

// mapping() of the reference (utils.py:1356-1366) on a grey value: the simulator's nine label colours become class
// indices, every other value stays what it is.  (v / 255f) * 255f == v for all 256 bytes, so this integer table is the
// reference's to_tensor(x) * 255 followed by the fp32 equality tests.
__device__ inline int label_class(int v) {
  switch (v) {
    case 255: return 8;
    case 200: return 7;
    case 178: return 6;
    case 149: return 5;
    case 133: return 4;
    case 76: return 3;
    case 55: return 2;
    case 29: return 1;
    default: return v;
  }
}

constexpr int LABEL_BLOCK = 256;

// Plane chain of MyDatasetSynthetic.transform (utils.py:495-543) for the mask (kind 0) and the two label maps (kind 1):
// flip, NEAREST resize to the resized image's (rs_w, rs_h), crop at (crop_i, crop_j).  One thread per output pixel.
// Label planes are finished here (mapping); mask planes store the grey value and take the maximum of their crop window
// -- reduced in LDS first, so a workgroup issues one global atomic per plane it touches -- for label_finish_kernel.
__global__ void __launch_bounds__(LABEL_BLOCK)
label_gather_kernel(const unsigned char* __restrict__ pool, const munit_image_desc* __restrict__ descs, int N, int out_h,
                    int out_w, const int* __restrict__ tab, float* __restrict__ out, int* __restrict__ vmax) {
  __shared__ int smax[LABEL_BLOCK];     // 256 consecutive pixels touch at most 256 planes
  const long long hw = (long long)out_h * out_w;
  const long long total = (long long)N * hw;
  for (long long base = (long long)blockIdx.x * LABEL_BLOCK; base < total; base += (long long)gridDim.x * LABEL_BLOCK) {
    const int b0 = (int)(base / hw);
    smax[threadIdx.x] = 0;
    __syncthreads();
    const long long i = base + threadIdx.x;
    if (i < total) {
      const int b = (int)(i / hw);
      const int rem = (int)(i - (long long)b * hw);
      const int y = rem / out_w, x = rem - y * out_w;
      const munit_image_desc d = descs[b];
      const int* t = tab + (long long)b * (out_h + out_w);
      const int sy = t[y];
      int sx = t[out_h + x];
      int v = 0;
      if (sy >= 0 && sx >= 0) {
        if (d.flip) sx = d.src_w - 1 - sx;
        v = pool[d.src_off + (long long)sy * d.src_w + sx];
      }
      if (d.kind != 0) {
        out[i] = (float)label_class(v);
      } else {
        out[i] = (float)v;
        if (v > 0) atomicMax(&smax[b - b0], v);
      }
    }
    __syncthreads();
    const int m = smax[threadIdx.x];
    if (m > 0) atomicMax(&vmax[b0 + threadIdx.x], m);   // slot k is cleared by thread k itself: no barrier needed
  }
}

// Mask rule of utils.py:537-543 in integers: to_tensor (x255 when the crop's maximum is 1), then > 0.5 -> 1, < 0.5 -> 0.
// No byte lands on 0.5 (v / 255 for v = 127, 128 is 0.498, 0.502).
__global__ void label_finish_kernel(const munit_image_desc* __restrict__ descs, float* __restrict__ out,
                                    const int* __restrict__ vmax, int N, long long hw) {
  const long long total = (long long)N * hw;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / hw);
    if (descs[b].kind != 0) continue;
    const int v = (int)out[i];
    out[i] = (vmax[b] == 1 ? v == 1 : v >= 128) ? 1.0f : 0.0f;
  }
}

int grid_for(long long n) { return (int)std::min<long long>((n + 255) / 256, 8192); }

// ---- sample grids: make_grid(normalize=True, padding=0) + save_image's byte conversion (munit_image_grid_u8) -------------
constexpr int GRID_MAX_SRC = 16;
constexpr int GRID_NT = 256;
constexpr int GRID_RANGE_BLOCKS = 512;    // most (min, max) partials the range pass writes: the size of the workspace
constexpr int GRID_PACK_BLOCKS = 2048;
constexpr long long GRID_MAX_OUT_BYTES = 2147483647LL;   // pixel and element indices of this file fit an int

// The sources, handed to both kernels by value.  Source s owns the elements [elems[s], elems[s + 1]) of the range pass and
// the grid cells [first[s], first[s + 1]).
struct GridArgs {
  const float* data[GRID_MAX_SRC];
  long long elems[GRID_MAX_SRC + 1];
  int first[GRID_MAX_SRC + 1];
  int channels[GRID_MAX_SRC];
  int layout[GRID_MAX_SRC];
  int nsrc;
};

// minimum and maximum over the 256 threads of a block, in every thread (fminf / fmaxf skip a NaN operand)
__device__ inline void block_min_max256(float& lo, float& hi, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off, 64));
    hi = fmaxf(hi, __shfl_xor(hi, off, 64));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[wave] = lo;
    red[4 + wave] = hi;
  }
  __syncthreads();
  lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
  hi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
}

// Range pass: partial[2 b], partial[2 b + 1] = minimum and maximum of (x + pre_add) * pre_mul over the elements block b
// visits.  A source may start at any 4-byte boundary, so every load is a scalar one.  The channel of a one-channel source
// is read once: repeating it three times changes neither extreme.
__global__ void __launch_bounds__(GRID_NT)
grid_range_kernel(GridArgs a, float pre_add, float pre_mul, float* __restrict__ partial) {
  __shared__ float red[8];
  const long long total = a.elems[a.nsrc];
  float lo = INFINITY, hi = -INFINITY;
  int s = 0;
  for (long long i = (long long)blockIdx.x * GRID_NT + threadIdx.x; i < total; i += (long long)gridDim.x * GRID_NT) {
    while (i >= a.elems[s + 1]) ++s;            // i only grows, and i < total = elems[nsrc] ends the walk
    const float v = (a.data[s][i - a.elems[s]] + pre_add) * pre_mul;
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  block_min_max256(lo, hi, red);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = lo;
    partial[2 * blockIdx.x + 1] = hi;
  }
}

// Pack pass: every block reduces the partials to (lo, hi) itself -- minimum and maximum do not depend on the order -- and
// writes whole pixels of the [ymaps * H][xmaps * W][3] byte grid, three byte stores each (W * 3 is in general no multiple
// of 4 and `out` has no alignment to speak of, so nothing wider is attempted).  Cells past nmaps are written as 0.
//   t = (v - lo) * (1 / d),  d = max(hi - lo, 1e-5): torch's device kernel for `tensor / python_float` multiplies by the
//   fp32 reciprocal of the scalar; hi - lo is formed in double and rounded once, as the reference's python floats are.
__global__ void __launch_bounds__(GRID_NT)
grid_pack_kernel(GridArgs a, int H, int W, int xmaps, int ymaps, int nmaps, float pre_add, float pre_mul,
                 const float* __restrict__ partial, int nparts, unsigned char* __restrict__ out) {
  __shared__ float red[8];
  float lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < nparts; i += GRID_NT) {
    lo = fminf(lo, partial[2 * i]);
    hi = fmaxf(hi, partial[2 * i + 1]);
  }
  block_min_max256(lo, hi, red);
  const float d = (float)fmax((double)hi - (double)lo, 1e-5);
  const float r = __fdiv_rn(1.0f, d);
  const long long row = (long long)xmaps * W;
  const long long total = (long long)ymaps * H * row;
  for (long long p = (long long)blockIdx.x * GRID_NT + threadIdx.x; p < total; p += (long long)gridDim.x * GRID_NT) {
    const int y = (int)(p / row), x = (int)(p - (long long)y * row);
    const int cy = y / H, iy = y - cy * H, cx = x / W, ix = x - cx * W;
    const int m = cy * xmaps + cx;
    unsigned char px[3] = {0, 0, 0};
    if (m < nmaps) {
      int s = 0;
      while (m >= a.first[s + 1]) ++s;          // m < nmaps = first[nsrc] ends the walk
      const int C = a.channels[s];
      const long long img = m - a.first[s];
      const float* __restrict__ src = a.data[s];
      const long long hw = (long long)H * W;
      const long long pos = (long long)iy * W + ix;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int cs = C == 3 ? c : 0;
        const long long idx = a.layout[s] == 0 ? (img * C + cs) * hw + pos : (img * hw + pos) * C + cs;
        const float v = (src[idx] + pre_add) * pre_mul;
        const float t = (v - lo) * r;
        const float q = fminf(fmaxf(t * 255.0f + 0.5f, 0.0f), 255.0f);
        px[c] = (unsigned char)(int)q;
      }
    }
    unsigned char* o = out + p * 3;
    o[0] = px[0];
    o[1] = px[1];
    o[2] = px[2];
  }
}

}  // namespace

extern "C" int munit_image_ksize(int src_size, int rs_size) {
  if (src_size <= 0 || rs_size <= 0) return 0;
  double scale = (double)src_size / (double)rs_size;
  if (scale < 1.0) scale = 1.0;
  const double support = 1.0 * scale;
  return (int)ceil(support) * 2 + 1;
}

extern "C" size_t munit_image_preprocess_workspace_bytes(int B, int out_h, int out_w, int ksize_max) {
  return align_up((size_t)B * (out_h + out_w) * (2 + ksize_max) * sizeof(int), 256);
}

extern "C" int munit_image_preprocess(const unsigned char* pool, const munit_image_desc* descs, int B, int out_h,
                                      int out_w, int ksize_max, float* out, void* ws, size_t ws_bytes,
                                      munit_stream_t stream) {
  MUNIT_CHECK_ARG(pool && descs && out && ws, "image_preprocess: null pointer");
  MUNIT_CHECK_ARG(B > 0 && out_h > 0 && out_w > 0 && ksize_max >= 3, "image_preprocess: bad shape");
  if (ws_bytes < munit_image_preprocess_workspace_bytes(B, out_h, out_w, ksize_max)) {
    munit_set_error("image_preprocess: workspace %zu < %zu", ws_bytes,
                    munit_image_preprocess_workspace_bytes(B, out_h, out_w, ksize_max));
    return MUNIT_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  int* tab = reinterpret_cast<int*>(ws);
  hipLaunchKernelGGL(resample_tables_kernel, dim3(grid_for((long long)B * (out_h + out_w))), dim3(256), 0, st, descs, B,
                     out_h, out_w, ksize_max, tab);
  MUNIT_CHECK_LAUNCH("resample_tables");
  hipLaunchKernelGGL(image_resample_kernel, dim3(grid_for((long long)B * out_h * out_w)), dim3(256), 0, st, pool, descs,
                     B, out_h, out_w, ksize_max, tab, out);
  MUNIT_CHECK_LAUNCH("image_resample");
  return MUNIT_OK;
}

extern "C" size_t munit_mask_preprocess_workspace_bytes(int B, int out_h, int out_w) {
  return align_up((size_t)B * (out_h + out_w + 1) * sizeof(int), 256);
}

extern "C" int munit_mask_preprocess(const unsigned char* pool, const munit_image_desc* descs, int B, int out_h,
                                     int out_w, float* out, void* ws, size_t ws_bytes, munit_stream_t stream) {
  MUNIT_CHECK_ARG(pool && descs && out && ws, "mask_preprocess: null pointer");
  MUNIT_CHECK_ARG(B > 0 && out_h > 0 && out_w > 0, "mask_preprocess: bad shape");
  if (ws_bytes < munit_mask_preprocess_workspace_bytes(B, out_h, out_w)) {
    munit_set_error("mask_preprocess: workspace %zu < %zu", ws_bytes, munit_mask_preprocess_workspace_bytes(B, out_h, out_w));
    return MUNIT_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  int* tab = reinterpret_cast<int*>(ws);
  int* vmax = tab + (size_t)B * (out_h + out_w);
  if (hipMemsetAsync(vmax, 0, (size_t)B * sizeof(int), st) != hipSuccess) {
    munit_set_error("mask_preprocess: memset failed");
    return MUNIT_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(nearest_tables_kernel, dim3(cdiv(2 * B, 64)), dim3(64), 0, st, descs, B, out_h, out_w, 0, tab);
  MUNIT_CHECK_LAUNCH("nearest_tables");
  hipLaunchKernelGGL(mask_gather_kernel, dim3(grid_for((long long)B * out_h * out_w)), dim3(256), 0, st, pool, descs, B,
                     out_h, out_w, tab, out, vmax);
  MUNIT_CHECK_LAUNCH("mask_gather");
  hipLaunchKernelGGL(mask_scale_kernel, dim3(grid_for((long long)B * out_h * out_w)), dim3(256), 0, st, out, vmax, B,
                     out_h * out_w);
  MUNIT_CHECK_LAUNCH("mask_scale");
  return MUNIT_OK;
}

extern "C" size_t munit_label_preprocess_workspace_bytes(int N, int out_h, int out_w) {
  return align_up((size_t)N * (out_h + out_w + 1) * sizeof(int), 256);
}

extern "C" int munit_label_preprocess(const unsigned char* pool, const munit_image_desc* descs, int N, int out_h,
                                      int out_w, float* out, void* ws, size_t ws_bytes, munit_stream_t stream) {
  MUNIT_CHECK_ARG(pool && descs && out && ws, "label_preprocess: null pointer");
  MUNIT_CHECK_ARG(N > 0 && out_h > 0 && out_w > 0, "label_preprocess: bad shape");
  if (ws_bytes < munit_label_preprocess_workspace_bytes(N, out_h, out_w)) {
    munit_set_error("label_preprocess: workspace %zu < %zu", ws_bytes, munit_label_preprocess_workspace_bytes(N, out_h, out_w));
    return MUNIT_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  int* tab = reinterpret_cast<int*>(ws);
  int* vmax = tab + (size_t)N * (out_h + out_w);
  if (hipMemsetAsync(vmax, 0, (size_t)N * sizeof(int), st) != hipSuccess) {
    munit_set_error("label_preprocess: memset failed");
    return MUNIT_ERR_LAUNCH;
  }
  const long long total = (long long)N * out_h * out_w;
  hipLaunchKernelGGL(nearest_tables_kernel, dim3(cdiv(2 * N, 64)), dim3(64), 0, st, descs, N, out_h, out_w, 1, tab);
  MUNIT_CHECK_LAUNCH("nearest_tables");
  hipLaunchKernelGGL(label_gather_kernel, dim3(grid_for(total)), dim3(LABEL_BLOCK), 0, st, pool, descs, N, out_h, out_w, tab,
                     out, vmax);
  MUNIT_CHECK_LAUNCH("label_gather");
  hipLaunchKernelGGL(label_finish_kernel, dim3(grid_for(total)), dim3(256), 0, st, descs, out, vmax, N,
                     (long long)out_h * out_w);
  MUNIT_CHECK_LAUNCH("label_finish");
  return MUNIT_OK;
}

extern "C" size_t munit_image_grid_workspace_bytes(int nsrc, int H, int W, int nrow) {
  if (nsrc < 1 || nsrc > GRID_MAX_SRC || H < 1 || W < 1 || nrow < 1) return 0;
  return align_up((size_t)GRID_RANGE_BLOCKS * 2 * sizeof(float), 256);
}

extern "C" int munit_image_grid_u8(const munit_grid_src* src, int nsrc, int H, int W, int nrow, float pre_add, float pre_mul,
                                   unsigned char* out, void* ws, size_t ws_bytes, munit_stream_t stream) {
  MUNIT_CHECK_ARG(src && out && ws, "image_grid: null pointer");
  MUNIT_CHECK_ARG(nsrc >= 1 && nsrc <= GRID_MAX_SRC, "image_grid: nsrc must be 1..%d, got %d", GRID_MAX_SRC, nsrc);
  MUNIT_CHECK_ARG(H > 0 && W > 0 && nrow > 0, "image_grid: bad shape");
  GridArgs a;
  a.nsrc = nsrc;
  a.elems[0] = 0;
  a.first[0] = 0;
  const long long hw = (long long)H * W;
  long long nmaps = 0;
  for (int s = 0; s < nsrc; ++s) {
    MUNIT_CHECK_ARG(src[s].data, "image_grid: source %d is null", s);
    MUNIT_CHECK_ARG(src[s].n >= 1, "image_grid: source %d holds %d images", s, src[s].n);
    MUNIT_CHECK_ARG(src[s].channels == 1 || src[s].channels == 3, "image_grid: source %d has %d channels (1 or 3)", s,
                    src[s].channels);
    MUNIT_CHECK_ARG(src[s].layout == 0 || src[s].layout == 1, "image_grid: source %d has layout %d (0 planar, 1 interleaved)",
                    s, src[s].layout);
    nmaps += src[s].n;
    // every cell is part of the output, so this bounds nmaps, the element counts and the products below as well
    MUNIT_CHECK_ARG(nmaps <= GRID_MAX_OUT_BYTES / 3 / hw, "image_grid: output above %lld bytes", GRID_MAX_OUT_BYTES);
    a.data[s] = src[s].data;
    a.channels[s] = src[s].channels;
    a.layout[s] = src[s].layout;
    a.elems[s + 1] = a.elems[s] + (long long)src[s].n * src[s].channels * hw;
    a.first[s + 1] = (int)nmaps;
  }
  const int xmaps = (int)std::min<long long>(nrow, nmaps);
  const int ymaps = (int)((nmaps + xmaps - 1) / xmaps);
  MUNIT_CHECK_ARG((long long)ymaps * xmaps <= GRID_MAX_OUT_BYTES / 3 / hw, "image_grid: output above %lld bytes",
                  GRID_MAX_OUT_BYTES);
  if (ws_bytes < munit_image_grid_workspace_bytes(nsrc, H, W, nrow)) {
    munit_set_error("image_grid: workspace %zu < %zu", ws_bytes, munit_image_grid_workspace_bytes(nsrc, H, W, nrow));
    return MUNIT_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  float* partial = reinterpret_cast<float*>(ws);
  const int nparts = (int)std::min<long long>((a.elems[nsrc] + GRID_NT - 1) / GRID_NT, GRID_RANGE_BLOCKS);
  hipLaunchKernelGGL(grid_range_kernel, dim3(nparts), dim3(GRID_NT), 0, st, a, pre_add, pre_mul, partial);
  MUNIT_CHECK_LAUNCH("grid_range");
  const long long pixels = (long long)ymaps * xmaps * hw;
  const int blocks = (int)std::min<long long>((pixels + GRID_NT - 1) / GRID_NT, GRID_PACK_BLOCKS);
  hipLaunchKernelGGL(grid_pack_kernel, dim3(blocks), dim3(GRID_NT), 0, st, a, H, W, xmaps, ymaps, (int)nmaps, pre_add,
                     pre_mul, partial, nparts, out);
  MUNIT_CHECK_LAUNCH("grid_pack");
  return MUNIT_OK;
}
