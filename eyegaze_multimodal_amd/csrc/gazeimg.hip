// Gaze heat-map images on the device (1_Data/processed/multimodal_dataset.py:67-83, :151-154): eg_gaze_resize turns ragged uint8
// RGB images into one [n, F, W, 3] uint8 store with Pillow's antialiased bilinear resample, byte for byte; eg_gaze_batch gathers a
// training batch out of that store, flips, jitters, normalises and writes the image encoder's input in one launch.
// include/eyegaze_hip.h states both contracts; DESIGN.md §8o the arithmetic, the layout and the measurements.
//
// Everything is integer or table arithmetic, so the outputs do not depend on the batch an image sits in: no atomics, no float
// reduction (the one sum, the luminance of an image, is an integer).
//   resize, launch 1 (horizontal): block (image, group of H_ROWS source rows); a row is staged in LDS once by 16-byte loads, threads
//                                  run over (x_out, channel) and read their taps from LDS; out: the uint8 intermediate (h, W, 3)
//   resize, launch 2 (vertical):   threads run over VEC consecutive bytes of an output row (VEC = 16, 4 or 1: the widest that keeps
//                                  every row of W * 3 bytes aligned) and loop over the taps' rows
//   batch:                         block (sample j, player pl); pass 1 (contrast only) sums the image's luminance, pass 2 writes
#include "common.h"

namespace {

constexpr int MAX_SIDE = EG_GAZE_MAX_SIDE;       // source h, w
constexpr int MIN_OUT = EG_GAZE_MIN_OUT, MAX_OUT = EG_GAZE_MAX_OUT;
constexpr int PRECISION_BITS = 22;
constexpr int H_ROWS = 4;                        // source rows per block of the horizontal pass

// one axis' table at 32-bit word `at` of tabs: [0] ksize, [1 .. out] xmin, [1 + out .. 2 out] count, then k [out][ksize]
struct AxisTable {
  const int32_t* xmin;
  const int32_t* count;
  const int32_t* k;
  int ksize;
};
__device__ __forceinline__ AxisTable axis_table(const int32_t* __restrict__ tabs, long long at, int out) {
  AxisTable t;
  const int32_t* p = tabs + at;
  t.ksize = p[0], t.xmin = p + 1, t.count = p + 1 + out, t.k = p + 1 + 2 * out;
  return t;
}

// clip(acc >> 22, 0, 255).  Written on the unsigned value ON PURPOSE: from `min(max(acc >> 22, 0), 255)` packed two to a word hipcc
// (ROCm 7.2) forms v_ashr_pk_u8_i32, and on the MI355X that instruction left the upper half of its destination register as it was
// while the compiler took it for zero -- bytes 2 and 3 of every packed word came out OR-ed with stale register contents
// (DESIGN.md §8o).  tests/test_gpu_gaze_images.py catches it; no kernel of this file may contain that instruction.
__device__ __forceinline__ uint32_t clip8(int acc) { return min((uint32_t)max(acc, 0) >> PRECISION_BITS, 255u); }

__device__ __forceinline__ bool served(int h, int w) { return h >= 1 && h <= MAX_SIDE && w >= 1 && w <= MAX_SIDE; }

// horizontal pass: image i, rows [H_ROWS blockIdx.y, + H_ROWS): (h, w, 3) -> mid (h, W, 3)
__global__ __launch_bounds__(256) void gaze_resize_h_kernel(const eg_gaze_resize_desc d, unsigned char* __restrict__ ws) {
  __shared__ uint4 row4[(MAX_SIDE * 3 + 15) / 16 + 1];                       // one source row from its 16-byte boundary on
  const unsigned char* row = (const unsigned char*)row4;
  const int i = blockIdx.x, h = d.h[i], w = d.w[i];
  if (!served(h, w)) return;
  const int r0 = blockIdx.y * H_ROWS;
  if (r0 >= h) return;
  const int W = d.W, nout = 3 * W;
  const AxisTable t = axis_table(d.tabs, d.htab[i], W);
  const unsigned char* src = d.data + d.off[i];                               // 16-byte aligned (the contract)
  unsigned char* mid = ws + d.mid_off[i];
  for (int r = r0; r < min(h, r0 + H_ROWS); ++r) {
    const long long b0 = (long long)r * w * 3;                               // the row's first byte, inside the image
    const int a = (int)(b0 & 15);
    const uint4* g = (const uint4*)(src + (b0 - a));                        // the image's padded end is a multiple of 16 too
    const int nvec = (a + 3 * w + 15) >> 4;
    __syncthreads();                                                          // the previous row's readers are done
    for (int v = threadIdx.x; v < nvec; v += 256) row4[v] = g[v];
    __syncthreads();
    unsigned char* out = mid + (long long)r * nout;
    for (int o = threadIdx.x; o < nout; o += 256) {
      const int xx = o / 3, c = o - 3 * xx;
      const int n = t.count[xx];
      const unsigned char* p = row + a + 3 * t.xmin[xx] + c;
      const int32_t* k = t.k + (long long)xx * t.ksize;
      int acc = 1 << (PRECISION_BITS - 1);
      for (int x = 0; x < n; ++x) acc += (int)p[3 * x] * k[x];
      out[o] = (unsigned char)clip8(acc);
    }
  }
}

__device__ __forceinline__ int byte_of(const uint32_t* w, int j) { return (int)((w[j >> 2] >> (8 * (j & 3))) & 0xffu); }

// VEC bytes as 32-bit words in registers (bytes are taken out and put back by shifts: nothing is addressed)
template <int VEC> struct Bytes;
template <> struct Bytes<16> {
  static constexpr int WORDS = 4;
  __device__ static __forceinline__ void ld(const unsigned char* p, uint32_t* w) {
    const uint4 v = *(const uint4*)p;
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  }
  __device__ static __forceinline__ void st(unsigned char* p, const uint32_t* w) { *(uint4*)p = make_uint4(w[0], w[1], w[2], w[3]); }
};
template <> struct Bytes<4> {
  static constexpr int WORDS = 1;
  __device__ static __forceinline__ void ld(const unsigned char* p, uint32_t* w) { w[0] = *(const uint32_t*)p; }
  __device__ static __forceinline__ void st(unsigned char* p, const uint32_t* w) { *(uint32_t*)p = w[0]; }
};
template <> struct Bytes<1> {
  static constexpr int WORDS = 1;
  __device__ static __forceinline__ void ld(const unsigned char* p, uint32_t* w) { w[0] = *p; }
  __device__ static __forceinline__ void st(unsigned char* p, const uint32_t* w) { *p = (unsigned char)w[0]; }
};

// vertical pass: mid (h, W, 3) -> store[i] (F, W, 3); a thread owns VEC consecutive bytes of one output row
template <int VEC>
__global__ __launch_bounds__(256) void gaze_resize_v_kernel(const eg_gaze_resize_desc d, const unsigned char* __restrict__ ws,
                                                            unsigned char* __restrict__ store) {
  typedef Bytes<VEC> B;
  const int i = blockIdx.x, h = d.h[i], w = d.w[i];
  if (!served(h, w)) return;
  const int F = d.F, rowb = 3 * d.W, chunks = rowb / VEC;                     // VEC divides W * 3 (the launcher chose it so)
  const int g = blockIdx.y * 256 + threadIdx.x;
  if (g >= F * chunks) return;
  const int y = g / chunks, at = (g - y * chunks) * VEC;
  const AxisTable t = axis_table(d.tabs, d.vtab[i], F);
  const int n = t.count[y];
  const int32_t* k = t.k + (long long)y * t.ksize;
  const unsigned char* p = ws + d.mid_off[i] + (long long)t.xmin[y] * rowb + at;
  int acc[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[e] = 1 << (PRECISION_BITS - 1);
  for (int x = 0; x < n; ++x) {
    uint32_t v[B::WORDS];
    B::ld(p + (long long)x * rowb, v);
    const int kx = k[x];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] += byte_of(v, e) * kx;
  }
  uint32_t o[B::WORDS] = {};
#pragma unroll
  for (int e = 0; e < VEC; ++e) o[e >> 2] |= clip8(acc[e]) << (8 * (e & 3));
  B::st(store + ((long long)i * F + y) * rowb + at, o);
}

// ---------------------------------------------------------------------------------------------------------------
// the batch
// ---------------------------------------------------------------------------------------------------------------
struct Jitter {
  float fb, fc, m;          // brightness factor, contrast factor, the rounded mean luminance as a float
  bool bright_first;
};

// Pillow's two enhancers on one uint8 value: black + fb (v - black) and m + fc (v - m), every product and sum rounded on its own.
// The pragma is what keeps them apart: __fmul_rn / __fadd_rn are plain operators to hipcc, and under its default contraction
// m + fc * d became one fused multiply-add, which moved a byte of the fixture.
__device__ __forceinline__ int brighten(int v, float fb) {
#pragma clang fp contract(off)
  const float x = (float)v * fb;
  return (int)fminf(fmaxf(x, 0.0f), 255.0f);
}
__device__ __forceinline__ int contrast_of(int v, float fc, float m) {
#pragma clang fp contract(off)
  const float d = (float)v - m;
  const float t = fc * d;
  const float x = m + t;
  return (int)fminf(fmaxf(x, 0.0f), 255.0f);
}
// (1 - amount) + (2 amount) u, each operation rounded
__device__ __forceinline__ float jitter_factor(float amount, float u) {
#pragma clang fp contract(off)
  const float a = 1.0f - amount, b = 2.0f * amount;
  const float c = b * u;
  return a + c;
}
__device__ __forceinline__ int luminance(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

__device__ __forceinline__ int block_sum_int(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

struct Pixel { int r, g, b; };

// what pass 2 does to one pixel: jitter, table, channel mean
template <bool AUG>
__device__ __forceinline__ void finish_pixel(Pixel p, const Jitter& jt, const float* __restrict__ norm, float& r, float& g, float& b,
                                             float& mean) {
  if (AUG) {
    if (jt.bright_first) {
      p.r = contrast_of(brighten(p.r, jt.fb), jt.fc, jt.m), p.g = contrast_of(brighten(p.g, jt.fb), jt.fc, jt.m);
      p.b = contrast_of(brighten(p.b, jt.fb), jt.fc, jt.m);
    } else {
      p.r = brighten(contrast_of(p.r, jt.fc, jt.m), jt.fb), p.g = brighten(contrast_of(p.g, jt.fc, jt.m), jt.fb);
      p.b = brighten(contrast_of(p.b, jt.fc, jt.m), jt.fb);
    }
  }
  r = norm[p.r], g = norm[256 + p.g], b = norm[512 + p.b];
  const float rg = r + g;                                                     // (no product near: nothing to contract)
  mean = __fdiv_rn(rg + b, 3.0f);
}

__device__ __forceinline__ Pixel pixel_of(const uint32_t (&w)[3], int e) {     // pixel e of the 4 that 12 bytes hold
  return Pixel{byte_of(w, 3 * e), byte_of(w, 3 * e + 1), byte_of(w, 3 * e + 2)};
}

struct BatchArgs {
  const unsigned char* store;
  const int32_t* pair_img;
  const int32_t* win_pair;
  const int32_t* order;
  const float* norm;
  const float* factors;
  float* img[2];
  float* rgb[2];
  int n_images, F, W, first, n;
  uint32_t seed_lo, seed_hi;
  float hflip_p, brightness, contrast;
};

// VEC4: W % 4 == 0 and F * W % 4 == 0 -- every image and every row starts on a 4-byte boundary, 4 pixels are 3 words, and a
// mirrored group of 4 is a group of 4
template <bool AUG, bool VEC4>
__global__ __launch_bounds__(256) void gaze_batch_kernel(const BatchArgs a) {
  __shared__ float norm[768];
  __shared__ int red[4];
  const int j = blockIdx.x >> 1, pl = blockIdx.x & 1;
  const int wdw = a.order[a.first + j];
  const int im = a.pair_img[2 * a.win_pair[wdw] + pl];
  if (im < 0 || im >= a.n_images) return;                                    // (whole block: no barrier is left behind)
  const int F = a.F, W = a.W, npix = F * W;
  const unsigned char* src = a.store + (long long)im * npix * 3;
  for (int t = threadIdx.x; t < 768; t += 256) norm[t] = a.norm[t];
  Jitter jt{1.0f, 1.0f, 0.0f, true};
  bool flip = false;
  if (AUG) {
    if (a.factors) {
      const float* f = a.factors + 4 * (2 * j + pl);
      flip = f[0] != 0.0f, jt.fb = f[1], jt.fc = f[2], jt.bright_first = f[3] != 0.0f;
    } else {
      const uint32_t i = 2u * (uint32_t)(a.first + j) + (uint32_t)pl;
      const float ufl = (float)(eg_hash(a.seed_lo, a.seed_hi, EG_SITE_IMG_FLIP, i) >> 8) * 0x1p-24f;
      const float ub = (float)(eg_hash(a.seed_lo, a.seed_hi, EG_SITE_IMG_BRIGHT, i) >> 8) * 0x1p-24f;
      const float uc = (float)(eg_hash(a.seed_lo, a.seed_hi, EG_SITE_IMG_CONTRAST, i) >> 8) * 0x1p-24f;
      flip = ufl < a.hflip_p;
      jt.fb = jitter_factor(a.brightness, ub);
      jt.fc = jitter_factor(a.contrast, uc);
      jt.bright_first = (eg_hash(a.seed_lo, a.seed_hi, EG_SITE_IMG_ORDER, i) >> 31) == 0;
    }
    // the mean luminance of the image as it stands when contrast is applied; fc == 1 leaves every value alone, whatever the mean
    int sum = 0;
    if (jt.fc != 1.0f) {
      const bool pre = jt.bright_first;
      if (VEC4) {
        for (int q = threadIdx.x; q < npix / 4; q += 256) {
          const uint32_t* s = (const uint32_t*)(src + 12ll * q);
          const uint32_t w[3] = {s[0], s[1], s[2]};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            Pixel p = pixel_of(w, e);
            if (pre) p.r = brighten(p.r, jt.fb), p.g = brighten(p.g, jt.fb), p.b = brighten(p.b, jt.fb);
            sum += luminance(p.r, p.g, p.b);
          }
        }
      } else {
        for (int q = threadIdx.x; q < npix; q += 256) {
          Pixel p{src[3ll * q], src[3ll * q + 1], src[3ll * q + 2]};
          if (pre) p.r = brighten(p.r, jt.fb), p.g = brighten(p.g, jt.fb), p.b = brighten(p.b, jt.fb);
          sum += luminance(p.r, p.g, p.b);
        }
      }
    }
    sum = block_sum_int(sum, red);                                            // (also the barrier behind the table's staging)
    jt.m = (float)(int)((double)sum / (double)npix + 0.5);
  } else {
    __syncthreads();
  }
  float* img = a.img[pl] + (long long)j * npix;
  float* rgb = a.rgb[pl] ? a.rgb[pl] + (long long)j * 3 * npix : nullptr;
  if (VEC4) {
    const int gpr = W / 4;                                                    // groups of 4 pixels per row
    for (int q = threadIdx.x; q < npix / 4; q += 256) {
      const int y = q / gpr, gx = q - y * gpr;
      const int sq = flip ? y * gpr + (gpr - 1 - gx) : q;                     // the mirrored group, read backwards below
      const uint32_t* s = (const uint32_t*)(src + 12ll * sq);
      const uint32_t w[3] = {s[0], s[1], s[2]};
      f32x4 r, g, b, m;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float fr, fg, fb_, fm;
        finish_pixel<AUG>(pixel_of(w, flip ? 3 - e : e), jt, norm, fr, fg, fb_, fm);
        r[e] = fr, g[e] = fg, b[e] = fb_, m[e] = fm;
      }
      *(f32x4*)(img + 4ll * q) = m;
      if (rgb) {
        *(f32x4*)(rgb + 4ll * q) = r;
        *(f32x4*)(rgb + npix + 4ll * q) = g;
        *(f32x4*)(rgb + 2ll * npix + 4ll * q) = b;
      }
    }
  } else {
    for (int q = threadIdx.x; q < npix; q += 256) {
      const int y = q / W, x = q - y * W;
      const long long sp = flip ? (long long)y * W + (W - 1 - x) : q;
      float fr, fg, fb_, fm;
      finish_pixel<AUG>(Pixel{src[3 * sp], src[3 * sp + 1], src[3 * sp + 2]}, jt, norm, fr, fg, fb_, fm);
      img[q] = fm;
      if (rgb) rgb[q] = fr, rgb[npix + q] = fg, rgb[2ll * npix + q] = fb_;
    }
  }
}

bool aligned(const void* p, int to) { return ((uintptr_t)p & (uintptr_t)(to - 1)) == 0; }

}  // namespace

extern "C" int64_t eg_gaze_resize_workspace_bytes(int n_images, int64_t sum_h, int W) {
  if (n_images <= 0 || sum_h < n_images || sum_h > (int64_t)n_images * MAX_SIDE || W < MIN_OUT || W > MAX_OUT) return -1;
  return 3 * (int64_t)W * sum_h + 16 * (int64_t)n_images;                     // every intermediate starts on a 16-byte boundary
}

extern "C" int eg_gaze_resize(const eg_gaze_resize_desc* d, uint8_t* workspace, int64_t workspace_bytes, uint8_t* store, void* stream) {
  EG_CHECK(d && d->data && d->off && d->h && d->w && d->mid_off && d->tabs && d->htab && d->vtab && workspace && store,
           "eg_gaze_resize: null pointer");
  EG_CHECK(d->n_images > 0, "eg_gaze_resize: n_images=%d must be > 0", d->n_images);
  EG_CHECK(d->F >= MIN_OUT && d->F <= MAX_OUT, "eg_gaze_resize: F=%d outside [%d, %d]", d->F, MIN_OUT, MAX_OUT);
  EG_CHECK(d->W >= MIN_OUT && d->W <= MAX_OUT, "eg_gaze_resize: W=%d outside [%d, %d]", d->W, MIN_OUT, MAX_OUT);
  EG_CHECK(d->max_h >= 1 && d->max_h <= MAX_SIDE, "eg_gaze_resize: max_h=%d outside [1, %d]", d->max_h, MAX_SIDE);
  const int64_t need = eg_gaze_resize_workspace_bytes(d->n_images, d->sum_h, d->W);
  EG_CHECK(need >= 0, "eg_gaze_resize: sum_h=%lld is not the sum of %d heights in [1, %d]", (long long)d->sum_h, d->n_images, MAX_SIDE);
  EG_CHECK(need <= workspace_bytes, "eg_gaze_resize: the images need %lld workspace bytes, the workspace has %lld", (long long)need,
           (long long)workspace_bytes);
  EG_CHECK(aligned(d->data, 16) && aligned(workspace, 16) && aligned(store, 16),
           "eg_gaze_resize: data, workspace and store must start on 16-byte boundaries");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(gaze_resize_h_kernel, dim3(d->n_images, (d->max_h + H_ROWS - 1) / H_ROWS), dim3(256), 0, s, *d, workspace);
  EG_LAUNCH_CHECK("gaze_resize_h");
  const int rowb = 3 * d->W;
  const int vec = rowb % 16 == 0 ? 16 : rowb % 4 == 0 ? 4 : 1;
  const dim3 grid(d->n_images, (d->F * (rowb / vec) + 255) / 256);
  if (vec == 16) hipLaunchKernelGGL(gaze_resize_v_kernel<16>, grid, dim3(256), 0, s, *d, workspace, store);
  else if (vec == 4) hipLaunchKernelGGL(gaze_resize_v_kernel<4>, grid, dim3(256), 0, s, *d, workspace, store);
  else hipLaunchKernelGGL(gaze_resize_v_kernel<1>, grid, dim3(256), 0, s, *d, workspace, store);
  EG_LAUNCH_CHECK("gaze_resize_v");
  return 0;
}

extern "C" int eg_gaze_batch(const uint8_t* store, int n_images, int F, int W, const int32_t* pair_img, const int32_t* win_pair,
                             const int32_t* order, int order_len, int first, int n, const float* norm, uint32_t seed_lo,
                             uint32_t seed_hi, float hflip_p, float brightness, float contrast, const float* factors, float* img1,
                             float* img2, float* rgb1, float* rgb2, void* stream) {
  EG_CHECK(store && pair_img && win_pair && order && norm && img1 && img2, "eg_gaze_batch: null pointer");
  EG_CHECK(n > 0 && n_images > 0, "eg_gaze_batch: bad shape n=%d n_images=%d", n, n_images);
  EG_CHECK(F >= MIN_OUT && F <= MAX_OUT, "eg_gaze_batch: F=%d outside [%d, %d]", F, MIN_OUT, MAX_OUT);
  EG_CHECK(W >= MIN_OUT && W <= MAX_OUT, "eg_gaze_batch: W=%d outside [%d, %d]", W, MIN_OUT, MAX_OUT);
  EG_CHECK(first >= 0 && (long long)first + n <= (long long)order_len, "eg_gaze_batch: samples [%d, %d + %d) outside the order of %d",
           first, first, n, order_len);
  EG_CHECK(hflip_p >= 0.0f && hflip_p <= 1.0f, "eg_gaze_batch: hflip_p=%g outside [0, 1]", (double)hflip_p);
  EG_CHECK(brightness >= 0.0f && brightness < 1.0f, "eg_gaze_batch: brightness=%g outside [0, 1)", (double)brightness);
  EG_CHECK(contrast >= 0.0f && contrast < 1.0f, "eg_gaze_batch: contrast=%g outside [0, 1)", (double)contrast);
  EG_CHECK(!rgb1 == !rgb2, "eg_gaze_batch: rgb1 and rgb2 come together or not at all");
  BatchArgs a;
  a.store = store, a.pair_img = pair_img, a.win_pair = win_pair, a.order = order, a.norm = norm, a.factors = factors;
  a.img[0] = img1, a.img[1] = img2, a.rgb[0] = rgb1, a.rgb[1] = rgb2;
  a.n_images = n_images, a.F = F, a.W = W, a.first = first, a.n = n;
  a.seed_lo = seed_lo, a.seed_hi = seed_hi, a.hflip_p = hflip_p, a.brightness = brightness, a.contrast = contrast;
  const bool aug = factors || hflip_p != 0.0f || brightness != 0.0f || contrast != 0.0f;
  const bool vec4 = W % 4 == 0 && aligned(store, 4) && aligned(img1, 16) && aligned(img2, 16) && (!rgb1 || (aligned(rgb1, 16) && aligned(rgb2, 16)));
  const dim3 grid(2 * n), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (aug && vec4) hipLaunchKernelGGL((gaze_batch_kernel<true, true>), grid, block, 0, s, a);
  else if (aug) hipLaunchKernelGGL((gaze_batch_kernel<true, false>), grid, block, 0, s, a);
  else if (vec4) hipLaunchKernelGGL((gaze_batch_kernel<false, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((gaze_batch_kernel<false, false>), grid, block, 0, s, a);
  EG_LAUNCH_CHECK("gaze_batch");
  return 0;
}
