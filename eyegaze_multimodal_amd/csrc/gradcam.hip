// Grad-CAM of the spectrogram CNN's second convolution on the device (eeg_metrics.py:811-953):
//   eg_gradcam_accumulate: p1 (pooled conv-1 output) and d2 (gradient of conv-2's output), in the padded channel-last layouts stated
//   at the top of spec.hip, -> one 64 x 64 heat map per sample, added per class.
// Per image n:  wgt[c] = mean over the interior of d2[n][..][c];  cam_n = relu(sum_c wgt[c] * (b2[c] + conv3x3(p1[n], w2[c]))).
// The sum over c goes INTO the filter -- sum_c wgt[c] conv(p1, w2[c]) = conv(p1, sum_c wgt[c] w2[c]) -- so an image costs one
// 3 x 3 x 32 filter build (noise) and a single-output convolution: 288 MACs per pixel instead of 64 x 288, and conv-2's pre-ReLU
// output exists nowhere.
//
// Launch 1, gradcam_maps_kernel: one 1024-thread workgroup per (stream, sample).  Its four 256-thread quarters walk the sample's C
// images, quarter q the channels q, q + 4, ...; w2 (72 KB fp32) sits in LDS once per workgroup.  Per image and quarter:
//   A  the d2 interior in 16-B loads, thread <-> (8 channels, pixel slot), eight loads in flight; the 32 slots are summed by three
//      wave shuffles and one LDS step in a fixed order -> wgt[64];
//   B  the filter [tap][32 channels] and the bias from the LDS copy of w2;
//   C  the convolution, lane <-> (pixel, 8 channels): nine 16-B loads per pixel quarter (neighbouring lanes read neighbouring
//      bytes; a pixel's taps re-read what the L1 holds), four lanes summed by two shuffles, ReLU, added to the quarter's map in LDS.
// The quarters' maps are added in ascending order and divided by C: scratch[stream][sample][Hp][Wp], the only intermediate in
// global memory (1/C of the per-image map set).
// Launch 2, gradcam_resize_kernel: grid (16 tiles of 256 output pixels, ncls + 1).  Workgroup (tile, c) walks the samples whose
// label is c in ascending order (c = ncls: the labels outside [0, ncls), whose maps are written and counted nowhere): the two
// streams' maps averaged, resized with F.interpolate's bilinear weights (align_corners = False), written to cams and added into a
// register; one read-modify-write of class_sum at the end.  No float atomics, every sum in a fixed order.
#include "common.h"

namespace {

constexpr int GC_C1 = 32, GC_C2 = 64, GC_K = GC_C1 * 9;          // w2 [64][32][3][3]: 288 weights per output channel
constexpr int GC_OUT = 64, GC_OPIX = GC_OUT * GC_OUT;             // the heat map the reference resizes to
constexpr int GC_MAX_CLS = 16, GC_MAX_HW = 4096, GC_LIST = 1024;
constexpr int GC_QF = 4 * GC_C2 + GC_C2 + 292;                    // a quarter's floats besides its map: red[4][64] wgt[64] filt[288 + bias]
constexpr int GC_LDS_MAX = 160 * 1024;

__host__ __device__ constexpr int gc_lds_floats(int HW) { return GC_C2 * GC_K + GC_C2 + 4 * (GC_QF + HW); }

// eight consecutive elements as they lie in memory (16 B of a 16-bit type, 32 B of fp32): held raw while more loads are requested,
// converted where they are consumed
template <typename T> struct Raw8 { u32x4 v; };
template <> struct Raw8<float> { f32x4 a, b; };
template <typename T> __device__ __forceinline__ Raw8<T> raw8_zero() { Raw8<T> r; r.v = (u32x4){0u, 0u, 0u, 0u}; return r; }
template <> __device__ __forceinline__ Raw8<float> raw8_zero<float>() { Raw8<float> r; r.a = r.b = (f32x4){0.f, 0.f, 0.f, 0.f}; return r; }
template <typename T> __device__ __forceinline__ Raw8<T> raw8_ld(const T* p) { Raw8<T> r; r.v = *(const u32x4*)p; return r; }
template <> __device__ __forceinline__ Raw8<float> raw8_ld<float>(const float* p) {
  Raw8<float> r;
  r.a = *(const f32x4*)p;
  r.b = *(const f32x4*)(p + 4);
  return r;
}
__device__ __forceinline__ void raw8_floats(const Raw8<float>& r, float v[8]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e] = r.a[e]; v[4 + e] = r.b[e]; }
}
__device__ __forceinline__ void raw8_floats(const Raw8<bf16_t>& r, float v[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(r.v[i] << 16);
    v[2 * i + 1] = __uint_as_float(r.v[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ void raw8_floats(const Raw8<f16_t>& r, float v[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t w = r.v[i];
    const f32x2 t = __builtin_convertvector(__builtin_bit_cast(f16x2, w), f32x2);
    v[2 * i] = t[0];
    v[2 * i + 1] = t[1];
  }
}

template <typename T>
__global__ __launch_bounds__(1024) void gradcam_maps_kernel(const T* __restrict__ p1, const T* __restrict__ d2, const float* __restrict__ w2,
                                                            const float* __restrict__ b2, const float* __restrict__ grad_scale,
                                                            float* __restrict__ maps, int C, int Hp, int Wp) {
  extern __shared__ __attribute__((aligned(16))) float gsm[];
  constexpr int UA = sizeof(T) == 2 ? 8 : 4, UC = sizeof(T) == 2 ? 4 : 2;     // loads in flight per thread: 32 / 48 registers' worth
  const int HW = Hp * Wp, rowpx = Wp + 4;
  float* const Wl = gsm;                        // [64][288]
  float* const Bl = Wl + GC_C2 * GC_K;          // [64]
  const int tid = threadIdx.x, q = tid >> 8, t = tid & 255, lane = tid & 63, wq = t >> 6;
  float* const red = Bl + GC_C2 + q * (GC_QF + HW);       // [4 waves][64]
  float* const wgt = red + 4 * GC_C2;                     // [64]
  float* const filt = wgt + GC_C2;                        // [9 taps][32] + bias at [288]
  float* const macc = filt + 292;                         // [HW]
  for (int i = tid; i < GC_C2 * GC_K; i += 1024) Wl[i] = w2[i];
  if (tid < GC_C2) Bl[tid] = b2[tid];
  for (int i = t; i < HW; i += 256) macc[i] = 0.f;
  const float inv = 1.0f / (float)HW;
  const float scale = grad_scale ? *grad_scale : 1.0f;
  const size_t img_px = (size_t)(Hp + 2) * rowpx;
  __syncthreads();
  for (int c0 = 0; c0 < C; c0 += 4) {
    const int c = c0 + q;
    const bool active = c < C;                            // per quarter, so per wave
    const size_t n = (size_t)blockIdx.x * C + c;
    if (active) {
      // A: channel sums of the gradient's interior
      const T* dimg = d2 + n * img_px * GC_C2;
      const int c8 = (t & 7) * 8, slot = t >> 3;
      float acc[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll 1
      for (int p0 = 0; p0 < HW; p0 += 32 * UA) {
        Raw8<T> r[UA];
#pragma unroll
        for (int u = 0; u < UA; ++u) {
          const int pix = p0 + u * 32 + slot;
          r[u] = raw8_zero<T>();
          if (pix < HW) {
            const int y = pix / Wp, x = pix - y * Wp;
            r[u] = raw8_ld<T>(dimg + ((size_t)(y + 1) * rowpx + (x + 1)) * GC_C2 + c8);
          }
        }
#pragma unroll
        for (int u = 0; u < UA; ++u) {
          float v[8];
          raw8_floats(r[u], v);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] += v[e];
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {                       // the wave's eight slots: lanes l, l ^ 8, l ^ 16, l ^ 32
        acc[e] += __shfl_xor(acc[e], 8);
        acc[e] += __shfl_xor(acc[e], 16);
        acc[e] += __shfl_xor(acc[e], 32);
      }
      if (lane < 8) {
#pragma unroll
        for (int e = 0; e < 8; ++e) red[wq * GC_C2 + lane * 8 + e] = acc[e];
      }
    }
    __syncthreads();
    if (active && t < GC_C2) wgt[t] = (((red[t] + red[GC_C2 + t]) + red[2 * GC_C2 + t]) + red[3 * GC_C2 + t]) * inv / scale;
    __syncthreads();
    if (active) {
      // B: filt[tap][ci] = sum_c wgt[c] w2[c][ci][tap], bias = sum_c wgt[c] b2[c]
      for (int j = t; j <= GC_K; j += 256) {
        float s = 0.f;
        if (j < GC_K) {
#pragma unroll 8
          for (int k = 0; k < GC_C2; ++k) s = fmaf(wgt[k], Wl[k * GC_K + j], s);
          const int ci = j / 9, tap = j - ci * 9;
          filt[tap * GC_C1 + ci] = s;
        } else {
#pragma unroll 8
          for (int k = 0; k < GC_C2; ++k) s = fmaf(wgt[k], Bl[k], s);
          filt[GC_K] = s;
        }
      }
    }
    __syncthreads();
    if (active) {
      // C: the single-output convolution over the padded image (pixel (y, x)'s window starts at padded (y, x))
      const T* pimg = p1 + n * img_px * GC_C1;
      const int k8 = (t & 3) * 8, pl = t >> 2;
      const float bias = filt[GC_K];
#pragma unroll 1
      for (int p0 = 0; p0 < HW; p0 += 64 * UC) {
        float acc[UC];
        const T* base[UC];
        bool ok[UC];
#pragma unroll
        for (int u = 0; u < UC; ++u) {
          const int pix = p0 + u * 64 + pl;
          ok[u] = pix < HW;
          const int y = ok[u] ? pix / Wp : 0, x = ok[u] ? pix - y * Wp : 0;
          base[u] = pimg + ((size_t)y * rowpx + x) * GC_C1 + k8;
          acc[u] = 0.f;
        }
#pragma unroll 1
        for (int ky = 0; ky < 3; ++ky) {                  // one window row per trip: 3 UC loads in flight
          Raw8<T> r[3][UC];
#pragma unroll
          for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int u = 0; u < UC; ++u) {
              r[kx][u] = raw8_zero<T>();
              if (ok[u]) r[kx][u] = raw8_ld<T>(base[u] + ((size_t)ky * rowpx + kx) * GC_C1);
            }
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const float* fp = filt + (ky * 3 + kx) * GC_C1 + k8;
            const f32x4 fa = *(const f32x4*)fp, fb = *(const f32x4*)(fp + 4);
#pragma unroll
            for (int u = 0; u < UC; ++u) {
              float v[8];
              raw8_floats(r[kx][u], v);
              float s = acc[u];
#pragma unroll
              for (int e = 0; e < 4; ++e) s = fmaf(fa[e], v[e], s);
#pragma unroll
              for (int e = 0; e < 4; ++e) s = fmaf(fb[e], v[4 + e], s);
              acc[u] = s;
            }
          }
        }
#pragma unroll
        for (int u = 0; u < UC; ++u) {
          float s = acc[u];
          s += __shfl_xor(s, 1);
          s += __shfl_xor(s, 2);
          const int pix = p0 + u * 64 + pl;
          if ((t & 3) == 0 && pix < HW) macc[pix] += fmaxf(s + bias, 0.f);      // the same thread owns this pixel for every image
        }
      }
    }
    // (the next image's first LDS write that an unfinished reader could see is filt's, two barriers from here)
  }
  __syncthreads();
  const int qs = GC_QF + HW;
  const float* m0 = Bl + GC_C2 + GC_QF;
  const float invc = 1.0f / (float)C;
  for (int i = tid; i < HW; i += 1024)
    maps[(size_t)blockIdx.x * HW + i] = (((m0[i] + m0[qs + i]) + m0[2 * qs + i]) + m0[3 * qs + i]) * invc;
}

// F.interpolate(mode = "bilinear", align_corners = False): source index and weight of output index o (upsample_bilinear2d's
// area_pixel_compute_source_index; the products are kept apart so that no fused multiply-add changes the index arithmetic)
__device__ __forceinline__ void gc_source(int o, int in, int& i0, int& i1, float& l1) {
  const float scale = (float)in / (float)GC_OUT;
  float src = __fsub_rn(__fmul_rn(scale, (float)o + 0.5f), 0.5f);
  src = src < 0.f ? 0.f : src;
  i0 = min((int)src, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = __fsub_rn(src, (float)i0);
}

__global__ __launch_bounds__(256) void gradcam_resize_kernel(const float* __restrict__ maps, const int64_t* __restrict__ labels,
                                                             float* __restrict__ cams, float* __restrict__ class_sum,
                                                             int* __restrict__ class_count, int B, int Hp, int Wp, int ncls) {
  __shared__ int list[GC_LIST];
  __shared__ int cnt;
  const int t = threadIdx.x, cls = blockIdx.y, HW = Hp * Wp;
  const int o = blockIdx.x * 256 + t, oy = o >> 6, ox = o & 63;
  int y0, y1, x0, x1;
  float ly, lx;
  gc_source(oy, Hp, y0, y1, ly);
  gc_source(ox, Wp, x0, x1, lx);
  const float hy = 1.f - ly, hx = 1.f - lx;
  const int i00 = y0 * Wp + x0, i01 = y0 * Wp + x1, i10 = y1 * Wp + x0, i11 = y1 * Wp + x1;
  const float* s1 = maps;                       // stream 1: [B][HW]
  const float* s2 = maps + (size_t)B * HW;      // stream 2
  float acc = 0.f;
  int total = 0;
  for (int base = 0; base < B; base += GC_LIST) {
    const int lim = min(B, base + GC_LIST);
    if (t < 64) {                               // wave 0: this chunk's samples of the class, ascending
      int count = 0;
      for (int j = base; j < lim; j += 64) {
        const int idx = j + t;
        bool f = false;
        if (idx < lim) {
          const int64_t lab = labels[idx];
          const bool in_range = lab >= 0 && lab < ncls;
          f = cls < ncls ? (in_range && lab == cls) : !in_range;
        }
        const unsigned long long mask = __ballot(f);
        if (f) list[count + __popcll(mask & ((1ull << t) - 1ull))] = idx;
        count += __popcll(mask);
      }
      if (t == 0) cnt = count;
    }
    __syncthreads();
    const int n = cnt;
    total += n;
    for (int i = 0; i < n; i += 4) {
      float a[4][4];
      int bs[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        bs[u] = list[min(i + u, n - 1)];
        const float* m1 = s1 + (size_t)bs[u] * HW;
        const float* m2 = s2 + (size_t)bs[u] * HW;
        a[u][0] = (m1[i00] + m2[i00]) * 0.5f;
        a[u][1] = (m1[i01] + m2[i01]) * 0.5f;
        a[u][2] = (m1[i10] + m2[i10]) * 0.5f;
        a[u][3] = (m1[i11] + m2[i11]) * 0.5f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (i + u < n) {
          const float v = hy * (hx * a[u][0] + lx * a[u][1]) + ly * (hx * a[u][2] + lx * a[u][3]);
          cams[(size_t)bs[u] * GC_OPIX + o] = v;
          acc += v;
        }
    }
    __syncthreads();
  }
  if (cls < ncls) {
    class_sum[(size_t)cls * GC_OPIX + o] += acc;
    if (blockIdx.x == 0 && t == 0) class_count[cls] += total;
  }
}

bool gradcam_shape_ok(int B, int C, int Hp, int Wp) {
  return B >= 1 && B < 65536 && C >= 1 && C < 65536 && Hp >= 4 && Wp >= 4 && Hp % 4 == 0 && Wp % 4 == 0 &&
         (long long)Hp * Wp <= GC_MAX_HW && (long long)2 * B * C < (1ll << 31);
}

}  // namespace

extern "C" int64_t eg_gradcam_scratch_elems(int B, int C, int Hp, int Wp) {
  if (!gradcam_shape_ok(B, C, Hp, Wp)) return -1;
  return (int64_t)2 * B * Hp * Wp;              // the channel means of both streams: [2][B][Hp][Wp]
}

extern "C" int eg_gradcam_accumulate(const void* p1, const void* d2, const float* w2, const float* b2, const float* grad_scale,
                                     const int64_t* labels, float* cams, float* class_sum, int32_t* class_count, float* scratch,
                                     int64_t scratch_elems, int B, int C, int Hp, int Wp, int ncls, int dtype, void* stream) {
  const char* who = "eg_gradcam_accumulate";
  if (eg_dtype_check(who, dtype, true)) return 1;
  EG_CHECK(p1 && d2 && w2 && b2 && labels && cams && class_sum && class_count && scratch, "%s: null pointer", who);
  EG_CHECK(B >= 1 && C >= 1, "%s: bad shape B=%d C=%d", who, B, C);
  EG_CHECK(Hp >= 4 && Wp >= 4 && Hp % 4 == 0 && Wp % 4 == 0, "%s: Hp=%d Wp=%d must be positive multiples of 4", who, Hp, Wp);
  EG_CHECK(ncls >= 1 && ncls <= GC_MAX_CLS, "%s: ncls=%d outside [1, 16]", who, ncls);
  EG_CHECK(gradcam_shape_ok(B, C, Hp, Wp), "%s: bad shape B=%d C=%d Hp=%d Wp=%d (at most %d pixels per image)", who, B, C, Hp, Wp,
           GC_MAX_HW);
  const long long need = (long long)2 * B * Hp * Wp;
  EG_CHECK(scratch_elems >= need, "%s: scratch holds %lld floats, %lld are needed", who, (long long)scratch_elems, need);
  EG_CHECK((((uintptr_t)p1 | (uintptr_t)d2) & 15) == 0, "%s: p1 and d2 must be 16-byte aligned", who);
  static_assert(gc_lds_floats(GC_MAX_HW) * 4 <= GC_LDS_MAX, "gradcam_maps_kernel: LDS");
  const int lds = gc_lds_floats(Hp * Wp) * 4;
  hipStream_t s = (hipStream_t)stream;
  eg_dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    static const hipError_t attr =
        hipFuncSetAttribute((const void*)gradcam_maps_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, GC_LDS_MAX);
    (void)attr;
    hipLaunchKernelGGL(gradcam_maps_kernel<T>, dim3(2 * B), dim3(1024), lds, s, (const T*)p1, (const T*)d2, w2, b2, grad_scale, scratch, C,
                       Hp, Wp);
  });
  hipLaunchKernelGGL(gradcam_resize_kernel, dim3(GC_OPIX / 256, ncls + 1), dim3(256), 0, s, (const float*)scratch, labels, cams,
                     class_sum, (int*)class_count, B, Hp, Wp, ncls);
  EG_LAUNCH_CHECK("gradcam_accumulate");
  return 0;
}
