// Gaze pair analysis on the device (6_Utils/error_analysis.py:277-358, :460-464): the reference's
// compute_gaze_distance and compute_gaze_overlap for every pair of a resident uint8 image store in two launches, and the cosine of
// compute_feature_correlation.  include/eyegaze_hip.h states the contracts.
//
// A pixel is g = ((t0 + t1) + t2) / 3.0f with t_c = norm[c][v_c], the table staged in LDS: tensor.mean(dim=0), bit for bit.
//   launch 1 (image):  min and max of g (fp32, order-free) and the fp64 sums S = sum g, Sy = sum fl32(g y), Sx = sum fl32(g x),
//                      A = sum |g| -> workspace [n_images][8] doubles (S, Sy, Sx, A, min, max, 0, 0)
//   launch 2 (pair):   g of both images again, the masks (g - min) / ((max - min) + 1e-8f) > threshold, integer counts, the row
// No atomics.  Every float sum has ONE order, which depends on nothing but (F, W): thread t owns the 16-pixel chunks t, t + 256, ...
// in ascending order, then pixel 16 nch + t of the tail; lanes fold by a fixed butterfly, waves in ascending order through LDS.  A
// chunk is 48 bytes: three 16-byte loads where the image starts on a 16-byte boundary, 48 byte loads where it does not -- the same
// pixels to the same thread either way, so the bytes of a row do not depend on where in the store its images lie.
#include "common.h"

#include <math.h>

namespace {

constexpr int THREADS = 256, WAVES = THREADS / EG_WAVE;
constexpr int CHUNK_PIX = 16, CHUNK_BYTES = 3 * CHUNK_PIX;
constexpr int MIN_OUT = EG_GAZE_MIN_OUT, MAX_OUT = EG_GAZE_MAX_OUT;
constexpr int WS_FIELDS = 8;                     // doubles per image in the workspace

__device__ __forceinline__ uint32_t byte_of(const uint32_t* w, int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xffu; }

// 48 bytes from p as 12 words; wide: p is on a 16-byte boundary
__device__ __forceinline__ void load_chunk(const unsigned char* __restrict__ p, bool wide, uint32_t (&w)[12]) {
  if (wide) {
    const uint4* q = (const uint4*)p;
    const uint4 a = q[0], b = q[1], c = q[2];
    w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
    w[8] = c.x, w[9] = c.y, w[10] = c.z, w[11] = c.w;
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i)
      w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
  }
}

// tensor.mean(dim=0) of one pixel: two rounded sums and a correctly rounded division
__device__ __forceinline__ float gray_of(const float* norm, uint32_t r, uint32_t g, uint32_t b) {
#pragma clang fp contract(off)
  const float rg = norm[r] + norm[256 + g];
  return __fdiv_rn(rg + norm[512 + b], 3.0f);
}

struct ImageSums {
  double S, Sy, Sx, A;
  float mn, mx;
  // gray * y_coords and gray * x_coords are rounded fp32 products (torch's); the sums are fp64
  __device__ __forceinline__ void add(float g, int y, int x) {
#pragma clang fp contract(off)
    const float gy = g * (float)y, gx = g * (float)x;
    S += (double)g, Sy += (double)gy, Sx += (double)gx, A += (double)fabsf(g);
    mn = fminf(mn, g), mx = fmaxf(mx, g);
  }
};

__device__ __forceinline__ double wave_sum_f64(double v) {                    // every lane ends with the same bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void stage_table(float* norm, const float* __restrict__ src) {
  for (int t = threadIdx.x; t < 768; t += THREADS) norm[t] = src[t];
  __syncthreads();
}

// launch 1: workgroup = image
__global__ __launch_bounds__(THREADS) void gaze_image_stats_kernel(const unsigned char* __restrict__ store, int F, int W,
                                                                   const float* __restrict__ norm_g, double* __restrict__ ws) {
  __shared__ float norm[768];
  __shared__ double red[WAVES][4];
  __shared__ float redm[WAVES][2];
  stage_table(norm, norm_g);
  const int im = blockIdx.x, npix = F * W, nch = npix / CHUNK_PIX;
  const unsigned char* src = store + (long long)im * npix * 3;
  const bool wide = ((uintptr_t)src & 15) == 0;
  ImageSums s{0.0, 0.0, 0.0, 0.0, INFINITY, -INFINITY};
  for (int c = threadIdx.x; c < nch; c += THREADS) {
    uint32_t w[12];
    load_chunk(src + (long long)CHUNK_BYTES * c, wide, w);
    int y = (CHUNK_PIX * c) / W, x = CHUNK_PIX * c - y * W;
#pragma unroll
    for (int e = 0; e < CHUNK_PIX; ++e) {
      s.add(gray_of(norm, byte_of(w, 3 * e), byte_of(w, 3 * e + 1), byte_of(w, 3 * e + 2)), y, x);
      if (++x == W) x = 0, ++y;
    }
  }
  const int p = CHUNK_PIX * nch + threadIdx.x;                                // the tail: fewer than 16 pixels
  if (p < npix) {
    const int y = p / W, x = p - y * W;
    s.add(gray_of(norm, src[3ll * p], src[3ll * p + 1], src[3ll * p + 2]), y, x);
  }
  s.S = wave_sum_f64(s.S), s.Sy = wave_sum_f64(s.Sy), s.Sx = wave_sum_f64(s.Sx), s.A = wave_sum_f64(s.A);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s.mn = fminf(s.mn, __shfl_xor(s.mn, o, 64)), s.mx = fmaxf(s.mx, __shfl_xor(s.mx, o, 64));
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wv][0] = s.S, red[wv][1] = s.Sy, red[wv][2] = s.Sx, red[wv][3] = s.A, redm[wv][0] = s.mn, redm[wv][1] = s.mx;
  __syncthreads();
  if (threadIdx.x < 4) {                                                      // waves in ascending order
    double v = red[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < WAVES; ++k) v += red[k][threadIdx.x];
    ws[(long long)WS_FIELDS * im + threadIdx.x] = v;
  } else if (threadIdx.x == 4 || threadIdx.x == 5) {
    const int k = threadIdx.x - 4;
    float v = redm[0][k];
#pragma unroll
    for (int j = 1; j < WAVES; ++j) v = k ? fmaxf(v, redm[j][k]) : fminf(v, redm[j][k]);
    ws[(long long)WS_FIELDS * im + threadIdx.x] = (double)v;
  } else if (threadIdx.x < WS_FIELDS) {
    ws[(long long)WS_FIELDS * im + threadIdx.x] = 0.0;
  }
}

struct Mask {
  float mn, d, thr;
  // (gray - min) / ((max - min) + 1e-8f) > threshold, every operation a rounded fp32 one
  __device__ __forceinline__ int of(float g) const {
#pragma clang fp contract(off)
    const float c = g - mn;
    return __fdiv_rn(c, d) > thr ? 1 : 0;
  }
};
__device__ __forceinline__ Mask mask_of(const double* __restrict__ row, float thr) {
#pragma clang fp contract(off)
  const float mn = (float)row[4], mx = (float)row[5];                         // floats stored as doubles: exact
  const float span = mx - mn;
  return Mask{mn, span + 1e-8f, thr};
}

// the reference's centre of mass: the LITERAL (112, 112) when total < 1e-8, whatever F and W are
__device__ __forceinline__ void centre_of(const double* __restrict__ row, double& cy, double& cx) {
  const double S = row[0];
  if (S < 1e-8) cy = 112.0, cx = 112.0;
  else cy = row[1] / S, cx = row[2] / S;
}

// launch 2: workgroup = pair
__global__ __launch_bounds__(THREADS) void gaze_pair_kernel(const unsigned char* __restrict__ store, int n_images, int F, int W,
                                                            const int32_t* __restrict__ pair_img, const float* __restrict__ norm_g,
                                                            float threshold, const double* __restrict__ ws, double* __restrict__ out) {
  __shared__ float norm[768];
  __shared__ int red[WAVES][3];
  const int pr = blockIdx.x;
  const int ia = pair_img[2ll * pr], ib = pair_img[2ll * pr + 1];
  if (ia < 0 || ia >= n_images || ib < 0 || ib >= n_images) return;           // (whole block: no barrier is left behind)
  stage_table(norm, norm_g);
  const int npix = F * W, nch = npix / CHUNK_PIX;
  const unsigned char* sa = store + (long long)ia * npix * 3;
  const unsigned char* sb = store + (long long)ib * npix * 3;
  const bool wa = ((uintptr_t)sa & 15) == 0, wb = ((uintptr_t)sb & 15) == 0;
  const double* ra = ws + (long long)WS_FIELDS * ia;
  const double* rb = ws + (long long)WS_FIELDS * ib;
  const Mask ma = mask_of(ra, threshold), mb = mask_of(rb, threshold);
  int na = 0, nb = 0, ni = 0;
  for (int c = threadIdx.x; c < nch; c += THREADS) {
    uint32_t a[12], b[12];
    load_chunk(sa + (long long)CHUNK_BYTES * c, wa, a);
    load_chunk(sb + (long long)CHUNK_BYTES * c, wb, b);
#pragma unroll
    for (int e = 0; e < CHUNK_PIX; ++e) {
      const int qa = ma.of(gray_of(norm, byte_of(a, 3 * e), byte_of(a, 3 * e + 1), byte_of(a, 3 * e + 2)));
      const int qb = mb.of(gray_of(norm, byte_of(b, 3 * e), byte_of(b, 3 * e + 1), byte_of(b, 3 * e + 2)));
      na += qa, nb += qb, ni += qa & qb;
    }
  }
  const int p = CHUNK_PIX * nch + threadIdx.x;
  if (p < npix) {
    const int qa = ma.of(gray_of(norm, sa[3ll * p], sa[3ll * p + 1], sa[3ll * p + 2]));
    const int qb = mb.of(gray_of(norm, sb[3ll * p], sb[3ll * p + 1], sb[3ll * p + 2]));
    na += qa, nb += qb, ni += qa & qb;
  }
  na = wave_sum_int(na), nb = wave_sum_int(nb), ni = wave_sum_int(ni);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wv][0] = na, red[wv][1] = nb, red[wv][2] = ni;
  __syncthreads();
  if (threadIdx.x != 0) return;
  na = nb = ni = 0;
#pragma unroll
  for (int k = 0; k < WAVES; ++k) na += red[k][0], nb += red[k][1], ni += red[k][2];
  const int uni = na + nb - ni;
  double cya, cxa, cyb, cxb;
  centre_of(ra, cya, cxa);
  centre_of(rb, cyb, cxb);
  double dist;
  {
#pragma clang fp contract(off)
    const double dy = cya - cyb, dx = cxa - cxb;
    const double yy = dy * dy, xx = dx * dx;
    dist = sqrt(yy + xx);
  }
  double* o = out + (long long)EG_GAZE_PAIR_FIELDS * pr;
  o[0] = dist;
  o[1] = uni == 0 ? 0.0 : (double)__fdiv_rn((float)ni, (float)uni);           // (intersection / union).item(): an fp32 quotient
  o[2] = cya, o[3] = cxa, o[4] = cyb, o[5] = cxb;
  o[6] = (double)ni, o[7] = (double)uni, o[8] = (double)na, o[9] = (double)nb;
  o[10] = ra[0], o[11] = rb[0], o[12] = ra[3], o[13] = rb[3];
}

// one wave per row: lane l owns columns l, l + 64, ... in ascending order
__global__ __launch_bounds__(THREADS) void row_cosine_kernel(const float* __restrict__ a, const float* __restrict__ b, int N, int D,
                                                             float* __restrict__ out) {
  const int row = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= N) return;                                                       // (whole wave; the kernel has no barrier)
  const float* pa = a + (long long)row * D;
  const float* pb = b + (long long)row * D;
  double dot = 0.0, na = 0.0, nb = 0.0;
  for (int d = lane; d < D; d += EG_WAVE) {
#pragma clang fp contract(off)
    const double x = (double)pa[d], y = (double)pb[d];
    const double xy = x * y, xx = x * x, yy = y * y;
    dot += xy, na += xx, nb += yy;
  }
  dot = wave_sum_f64(dot), na = wave_sum_f64(na), nb = wave_sum_f64(nb);
  if (lane == 0) {
#pragma clang fp contract(off)
    const double den = fmax(sqrt(na), 1e-12) * fmax(sqrt(nb), 1e-12);         // F.normalize's clamp on either norm
    out[row] = (float)(dot / den);
  }
}

bool aligned(const void* p, int to) { return ((uintptr_t)p & (uintptr_t)(to - 1)) == 0; }

}  // namespace

extern "C" int64_t eg_gaze_pair_stats_workspace_bytes(int n_images) {
  if (n_images <= 0) return -1;
  return (int64_t)n_images * WS_FIELDS * (int64_t)sizeof(double);
}

extern "C" int eg_gaze_pair_stats(const uint8_t* store, int n_images, int F, int W, const int32_t* pair_img, int n_pairs,
                                  const float* norm, float threshold, void* workspace, int64_t workspace_bytes, double* out,
                                  void* stream) {
  EG_CHECK(store && pair_img && norm && workspace && out, "eg_gaze_pair_stats: null pointer");
  EG_CHECK(n_images > 0 && n_pairs > 0, "eg_gaze_pair_stats: bad shape n_images=%d n_pairs=%d", n_images, n_pairs);
  EG_CHECK(F >= MIN_OUT && F <= MAX_OUT, "eg_gaze_pair_stats: F=%d outside [%d, %d]", F, MIN_OUT, MAX_OUT);
  EG_CHECK(W >= MIN_OUT && W <= MAX_OUT, "eg_gaze_pair_stats: W=%d outside [%d, %d]", W, MIN_OUT, MAX_OUT);
  EG_CHECK(isfinite(threshold), "eg_gaze_pair_stats: threshold=%g is not finite", (double)threshold);
  const int64_t need = eg_gaze_pair_stats_workspace_bytes(n_images);
  EG_CHECK(need <= workspace_bytes, "eg_gaze_pair_stats: %d images need %lld workspace bytes, the workspace has %lld", n_images,
           (long long)need, (long long)workspace_bytes);
  EG_CHECK(aligned(workspace, 8) && aligned(out, 8), "eg_gaze_pair_stats: workspace and out must start on 8-byte boundaries");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(gaze_image_stats_kernel, dim3(n_images), dim3(THREADS), 0, s, store, F, W, norm, (double*)workspace);
  EG_LAUNCH_CHECK("gaze_image_stats");
  hipLaunchKernelGGL(gaze_pair_kernel, dim3(n_pairs), dim3(THREADS), 0, s, store, n_images, F, W, pair_img, norm, threshold,
                     (const double*)workspace, out);
  EG_LAUNCH_CHECK("gaze_pair");
  return 0;
}

extern "C" int eg_row_cosine(const float* a, const float* b, int N, int D, float* out, void* stream) {
  EG_CHECK(a && b && out, "eg_row_cosine: null pointer");
  EG_CHECK(N > 0, "eg_row_cosine: N=%d must be > 0", N);
  EG_CHECK(D >= 1 && D <= EG_ROW_COSINE_MAX_D, "eg_row_cosine: D=%d outside [1, %d]", D, EG_ROW_COSINE_MAX_D);
  hipLaunchKernelGGL(row_cosine_kernel, dim3((N + WAVES - 1) / WAVES), dim3(THREADS), 0, (hipStream_t)stream, a, b, N, D, out);
  EG_LAUNCH_CHECK("row_cosine");
  return 0;
}
