// Spatial entropy of gaze heat-map images (5_Metrics/entropy_calculators.py:145-180, SpatialEntropyCalculator.compute) for a batch
// of ragged images in one call: luminance, min-max normalisation, the Shannon entropy of the pixels in bits, all in fp64.
// include/eyegaze_hip.h states the contract; DESIGN.md §8n the layout, the numerics and the measurements.
//
// No atomics.  A workgroup owns EG_IMAGE_ENTROPY_CHUNK consecutive pixels of one image, whatever the batch: block (image, chunk).
// Inside a chunk a lane owns groups of GW consecutive pixels, group t, t + 256, ... and adds its pixels in ascending order; the
// lanes are added by the fixed-order block sum.  So a chunk's partials depend on the image alone, and every fold over chunks runs
// in ascending order: an image alone and inside any batch gives the same bytes.
//   launch 1: per chunk (min, max) of the luminance
//   launch 2: folds its image's (min, max) in ascending order, then per chunk (sum q, sum q ln q)
//   launch 3: one thread per image adds the chunks in ascending order: H = (ln S - T / S) / ln 2
#include "common.h"

namespace {

constexpr int CHUNK = EG_IMAGE_ENTROPY_CHUNK;
constexpr int MAX_PIX = 1 << 24;
static_assert(CHUNK % (256 * 16) == 0, "a chunk is whole rounds of 256 lanes x 16 pixels");

__device__ __forceinline__ double block_sum256(double v, double* red) {      // recprep.hip's block_sum_d: 256 threads, fixed order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) red[w] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// numpy's min / max: a NaN on either side stays
__device__ __forceinline__ double nan_min(double a, double b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

__device__ __forceinline__ double block_min256(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = nan_min(v, __shfl_xor(v, o, 64));
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) red[w] = v;
  __syncthreads();
  return nan_min(nan_min(nan_min(red[0], red[1]), red[2]), red[3]);
}
__device__ __forceinline__ double block_max256(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = nan_max(v, __shfl_xor(v, o, 64));
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) red[w] = v;
  __syncthreads();
  return nan_max(nan_max(nan_max(red[0], red[1]), red[2]), red[3]);
}

// numpy's (0.299 R + 0.587 G) + 0.114 B: three rounded products, two rounded sums
__device__ __forceinline__ double luma(double r, double g, double b) {
#pragma clang fp contract(off)
  const double x = 0.299 * r, y = 0.587 * g, z = 0.114 * b;
  const double xy = x + y;
  return xy + z;
}

struct Image {
  const unsigned char* u8;     // elem 0
  const double* f64;           // elem 1
  int npix, layout;
  bool ok, wide;               // wide: uint8, grey or pixel-interleaved, on a 16-byte boundary
};

__device__ __forceinline__ Image image_of(const eg_image_batch_desc& d, int i) {
  Image im;
  im.npix = d.npix[i], im.layout = d.layout[i];
  im.ok = im.npix >= 1 && im.npix <= d.max_pix && im.layout >= 0 && im.layout <= 2;
  const long long off = d.off[i];
  im.u8 = (const unsigned char*)d.data + off;
  im.f64 = (const double*)d.data + off;
  im.wide = d.elem == 0 && im.layout != 2 && ((unsigned long long)im.u8 & 15) == 0;
  return im;
}

template <typename T>
__device__ __forceinline__ double pixel_at(const T* __restrict__ p, int layout, int npix, int i) {
  if (layout == 0) return (double)p[i];
  if (layout == 1) return luma((double)p[3 * (long long)i], (double)p[3 * (long long)i + 1], (double)p[3 * (long long)i + 2]);
  return luma((double)p[i], (double)p[(long long)npix + i], (double)p[2 * (long long)npix + i]);
}

__device__ __forceinline__ unsigned byte_of(const unsigned* w, int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xffu; }

// f(luminance) for every pixel of chunk `chunk` that this lane owns, in ascending pixel order
template <typename F>
__device__ __forceinline__ void for_lane_pixels(const Image& im, const int elem, const int chunk, F&& f) {
  const int p0 = chunk * CHUNK, p1 = min(im.npix, p0 + CHUNK), t = threadIdx.x;
  if (im.wide) {
    // 16 pixels per group: one 16-byte load (grey) or three (interleaved RGB, 48 bytes); a chunk starts on a multiple of 16 pixels
    for (int g = p0 + 16 * t; g < p1; g += 16 * 256) {
      if (g + 16 <= p1) {
        if (im.layout == 0) {
          const uint4 v = *(const uint4*)(im.u8 + g);
          const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int k = 0; k < 16; ++k) f((double)byte_of(w, k));
        } else {
          const uint4* src = (const uint4*)(im.u8 + 3 * (long long)g);
          const uint4 a = src[0], b = src[1], c = src[2];
          const unsigned w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
          for (int k = 0; k < 16; ++k) f(luma((double)byte_of(w, 3 * k), (double)byte_of(w, 3 * k + 1), (double)byte_of(w, 3 * k + 2)));
        }
      } else {                                                              // the image's ragged last group
        for (int i = g; i < p1; ++i) f(pixel_at(im.u8, im.layout, im.npix, i));
      }
    }
  } else if (elem == 0) {
    for (int i = p0 + t; i < p1; i += 256) f(pixel_at(im.u8, im.layout, im.npix, i));
  } else {
    for (int i = p0 + t; i < p1; i += 256) f(pixel_at(im.f64, im.layout, im.npix, i));
  }
}

// workspace: minmax [n_images][chunks][2], then sums [n_images][chunks][2]; chunks = ceil(max_pix / CHUNK)
__global__ __launch_bounds__(256) void image_minmax_kernel(const eg_image_batch_desc d, const int chunks, double* __restrict__ minmax) {
  __shared__ double red[4];
  const int i = blockIdx.x, c = blockIdx.y;
  const Image im = image_of(d, i);
  if (!im.ok || (long long)c * CHUNK >= im.npix) return;
  double lo = INFINITY, hi = -INFINITY;
  for_lane_pixels(im, d.elem, c, [&](double g) { lo = nan_min(lo, g), hi = nan_max(hi, g); });
  lo = block_min256(lo, red), hi = block_max256(hi, red);
  if (threadIdx.x == 0) {
    double* out = minmax + ((long long)i * chunks + c) * 2;
    out[0] = lo, out[1] = hi;
  }
}

__global__ __launch_bounds__(256) void image_sums_kernel(const eg_image_batch_desc d, const int chunks, const double eps,
                                                         const double* __restrict__ minmax, double* __restrict__ sums) {
  __shared__ double red[4], s_lo, s_hi;
  const int i = blockIdx.x, c = blockIdx.y;
  const Image im = image_of(d, i);
  if (!im.ok || (long long)c * CHUNK >= im.npix) return;
  double lo = 0.0, den = 1.0;
  if (d.normalize) {
    if (threadIdx.x == 0) {
      const int n = (im.npix + CHUNK - 1) / CHUNK;
      const double* mm = minmax + (long long)i * chunks * 2;
      double a = mm[0], b = mm[1];
      for (int k = 1; k < n; ++k) a = nan_min(a, mm[2 * k]), b = nan_max(b, mm[2 * k + 1]);
      s_lo = a, s_hi = b;
    }
    __syncthreads();
    lo = s_lo, den = (s_hi - s_lo) + 1e-10;
  }
  const bool norm = d.normalize != 0;
  double S = 0.0, T = 0.0;
  for_lane_pixels(im, d.elem, c, [&](double g) {
    const double q = fabs(norm ? (g - lo) / den : g) + eps;
    S += q;
    if (q > 0.0 || q != q) T += q * log(q);                                // q == 0 (eps == 0) adds nothing, as scipy's entr
  });
  S = block_sum256(S, red), T = block_sum256(T, red);
  if (threadIdx.x == 0) {
    double* out = sums + ((long long)i * chunks + c) * 2;
    out[0] = S, out[1] = T;
  }
}

__global__ __launch_bounds__(256) void image_finish_kernel(const eg_image_batch_desc d, const int chunks, const double* __restrict__ sums,
                                                           double* __restrict__ entropy) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d.n_images) return;
  const Image im = image_of(d, i);
  if (!im.ok) return;
  const int n = (im.npix + CHUNK - 1) / CHUNK;
  const double* s = sums + (long long)i * chunks * 2;
  double S = s[0], T = s[1];
  for (int k = 1; k < n; ++k) S += s[2 * k], T += s[2 * k + 1];
  entropy[i] = (log(S) - T / S) / 0.693147180559945309417232121458;
}

}  // namespace

extern "C" int64_t eg_image_entropy_workspace_doubles(int n_images, int max_pix) {
  if (n_images <= 0 || max_pix < 1 || max_pix > MAX_PIX) return -1;
  return 4 * (int64_t)n_images * ((max_pix + CHUNK - 1) / CHUNK);
}

extern "C" int eg_image_entropy(const eg_image_batch_desc* d, double eps, double* workspace, int64_t workspace_capacity, double* entropy,
                                void* stream) {
  EG_CHECK(d && d->data && d->off && d->npix && d->layout && workspace && entropy, "eg_image_entropy: null pointer");
  EG_CHECK(d->n_images > 0, "eg_image_entropy: n_images=%d must be > 0", d->n_images);
  EG_CHECK(d->max_pix >= 1 && d->max_pix <= MAX_PIX, "eg_image_entropy: max_pix=%d outside [1, %d]", d->max_pix, MAX_PIX);
  EG_CHECK(d->elem == 0 || d->elem == 1, "eg_image_entropy: elem=%d is neither 0 (uint8) nor 1 (float64)", d->elem);
  EG_CHECK(eps >= 0.0, "eg_image_entropy: eps=%g must be >= 0", eps);
  const int64_t need = eg_image_entropy_workspace_doubles(d->n_images, d->max_pix);
  EG_CHECK(need <= workspace_capacity, "eg_image_entropy: the images need %lld workspace doubles, the workspace's capacity is %lld",
           (long long)need, (long long)workspace_capacity);
  const int chunks = (d->max_pix + CHUNK - 1) / CHUNK;                       // <= 2048: fits grid.y
  hipStream_t s = (hipStream_t)stream;
  double* minmax = workspace;
  double* sums = workspace + 2 * (int64_t)d->n_images * chunks;
  if (d->normalize) {
    hipLaunchKernelGGL(image_minmax_kernel, dim3(d->n_images, chunks), dim3(256), 0, s, *d, chunks, minmax);
    EG_LAUNCH_CHECK("image_minmax");
  }
  hipLaunchKernelGGL(image_sums_kernel, dim3(d->n_images, chunks), dim3(256), 0, s, *d, chunks, eps, minmax, sums);
  EG_LAUNCH_CHECK("image_sums");
  hipLaunchKernelGGL(image_finish_kernel, dim3((d->n_images + 255) / 256), dim3(256), 0, s, *d, chunks, sums, entropy);
  EG_LAUNCH_CHECK("image_finish");
  return 0;
}
