// Small per-sample kernels around the encoder: sequence assembly (CLS / shared tokens), pooling +
// symmetric fusion operands, the final class projection fused with cross-entropy, and their backward forms.
// These touch [B, d]-sized data; they are latency-bound, so each is a single short launch.
#include "common.h"

namespace {

// dst[b, off + r, :] = src[(b % src_nb), r, :] (+ pos[off + r, :])      src fp32 (parameters such as cls_token)
template <typename T>
__global__ void rows_bcast_f32_kernel(const float* __restrict__ src, const float* __restrict__ pos, T* __restrict__ dst,
                                      int NB, int S, int D, int R, int off, int src_nb) {
  const int b = blockIdx.y, r = blockIdx.x;
  const float* s = src + ((size_t)(b % src_nb) * R + r) * D;
  T* d = dst + ((size_t)b * S + off + r) * D;
  for (int n = threadIdx.x; n < D; n += blockDim.x) {
    float v = s[n];
    if (pos) v += pos[(size_t)(off + r) * D + n];
    Elem<T>::st(d + n, v);
  }
}

// dst[b_dst0 + b, off + r, :] = src[b_src0 + b, off + r, :]   (copy the shared synchrony tokens to stream 2)
template <typename T>
__global__ void rows_copy_kernel(T* __restrict__ seq, int S, int D, int R, int off, int b_src0, int b_dst0) {
  const int b = blockIdx.y, r = blockIdx.x;
  const T* s = seq + ((size_t)(b_src0 + b) * S + off + r) * D;
  T* d = seq + ((size_t)(b_dst0 + b) * S + off + r) * D;
  for (int n = threadIdx.x; n < D; n += blockDim.x) d[n] = s[n];
}

// pooling + fusion operands (D:1193-1212, D:933-938, D:1222-1223)
//   z [2B, S, D]; stream 1 = samples [0,B), stream 2 = [B,2B)
//   cls1/cls2 fp32 [B,D]; comb [B,3D] = [a+b, a*b, |a-b|]; zf[:, D:2D] = mean_{s>=off} z1, zf[:, 2D:3D] = same for z2
//   ibs_pool fp32+T [B,D] = mean_{1<=s<1+n_ibs} z1   (n_ibs may be 0)
template <typename T>
__global__ void pool_fuse_fwd_kernel(const T* __restrict__ z, float* __restrict__ cls1, float* __restrict__ cls2,
                                     T* __restrict__ comb, T* __restrict__ zf, float* __restrict__ ibs_pool_f,
                                     T* __restrict__ ibs_pool, int B, int S, int D, int off, int n_ibs, int ibs_first) {
  const int b = blockIdx.x;
  const T* z1 = z + (size_t)b * S * D;
  const T* z2 = z + (size_t)(b + B) * S * D;
  for (int n = threadIdx.x; n < D; n += blockDim.x) {
    const float a = Elem<T>::ld(z1 + n), c = Elem<T>::ld(z2 + n);
    cls1[(size_t)b * D + n] = a;
    cls2[(size_t)b * D + n] = c;
    Elem<T>::st(comb + (size_t)b * 3 * D + n, a + c);
    Elem<T>::st(comb + (size_t)b * 3 * D + D + n, a * c);
    Elem<T>::st(comb + (size_t)b * 3 * D + 2 * D + n, fabsf(a - c));
    float m1 = 0.f, m2 = 0.f;
#pragma unroll 8
    for (int s = off; s < S; ++s) {          // unrolled: 16 independent 2-byte loads in flight instead of 2
      m1 += Elem<T>::ld(z1 + (size_t)s * D + n);
      m2 += Elem<T>::ld(z2 + (size_t)s * D + n);
    }
    const float inv = 1.0f / (float)(S - off);
    Elem<T>::st(zf + (size_t)b * 3 * D + D + n, m1 * inv);
    Elem<T>::st(zf + (size_t)b * 3 * D + 2 * D + n, m2 * inv);
    if (n_ibs > 0) {
      float mi = 0.f;
      for (int s = ibs_first; s < ibs_first + n_ibs; ++s) mi += Elem<T>::ld(z1 + (size_t)s * D + n);
      mi /= (float)n_ibs;
      ibs_pool_f[(size_t)b * D + n] = mi;
      Elem<T>::st(ibs_pool + (size_t)b * D + n, mi);
    }
  }
}

// backward of the above: writes the full dz [2B, S, D] (zeros where nothing flows)
template <typename T>
__device__ __forceinline__ void pool_fuse_bwd_sample(const int b, const T* __restrict__ z, const T* __restrict__ dcomb,
                                                     const T* __restrict__ dzf, const float* __restrict__ gcls1,
                                                     const float* __restrict__ gcls2, const T* __restrict__ dibs_pool,
                                                     const float* __restrict__ gibs_pool, T* __restrict__ dz, int B, int S, int D,
                                                     int off, int n_ibs, int ibs_first) {
  const T* z1 = z + (size_t)b * S * D;
  const T* z2 = z + (size_t)(b + B) * S * D;
  T* d1 = dz + (size_t)b * S * D;
  T* d2 = dz + (size_t)(b + B) * S * D;
  const float invp = 1.0f / (float)(S - off);
  for (int n = threadIdx.x; n < D; n += blockDim.x) {
    const float a = Elem<T>::ld(z1 + n), c = Elem<T>::ld(z2 + n);
    const float g0 = Elem<T>::ld(dcomb + (size_t)b * 3 * D + n);
    const float g1 = Elem<T>::ld(dcomb + (size_t)b * 3 * D + D + n);
    const float g2 = Elem<T>::ld(dcomb + (size_t)b * 3 * D + 2 * D + n);
    const float sg = (a > c) ? 1.f : ((a < c) ? -1.f : 0.f);
    float da = g0 + g1 * c + g2 * sg;
    float dc = g0 + g1 * a - g2 * sg;
    if (gcls1) da += gcls1[(size_t)b * D + n];
    if (gcls2) dc += gcls2[(size_t)b * D + n];
    const float dm1 = Elem<T>::ld(dzf + (size_t)b * 3 * D + D + n) * invp;
    const float dm2 = Elem<T>::ld(dzf + (size_t)b * 3 * D + 2 * D + n) * invp;
    float di = 0.f;
    if (n_ibs > 0) {
      if (dibs_pool) di += Elem<T>::ld(dibs_pool + (size_t)b * D + n);
      if (gibs_pool) di += gibs_pool[(size_t)b * D + n];
      di /= (float)n_ibs;
    }
    for (int s = 0; s < S; ++s) {
      float v1 = 0.f, v2 = 0.f;
      if (s == 0) { v1 = da; v2 = dc; }
      if (s >= off) { v1 += dm1; v2 += dm2; }
      if (n_ibs > 0 && s >= ibs_first && s < ibs_first + n_ibs) v1 += di;
      Elem<T>::st(d1 + (size_t)s * D + n, v1);
      Elem<T>::st(d2 + (size_t)s * D + n, v2);
    }
  }
}
template <typename T>
__global__ void pool_fuse_bwd_kernel(const T* __restrict__ z, const T* __restrict__ dcomb, const T* __restrict__ dzf,
                                     const float* __restrict__ gcls1, const float* __restrict__ gcls2,
                                     const T* __restrict__ dibs_pool, const float* __restrict__ gibs_pool,
                                     T* __restrict__ dz, int B, int S, int D, int off, int n_ibs, int ibs_first) {
  pool_fuse_bwd_sample<T>(blockIdx.x, z, dcomb, dzf, gcls1, gcls2, dibs_pool, gibs_pool, dz, B, S, D, off, n_ibs, ibs_first);
}

// logits = h W^T + b  (ncls <= 16), per-sample CE; one wave per sample (D:1104-1105 / 1078 + D:1244 / 1250)
// one wave, one sample b whose K hidden values start at hrow (global or LDS)
template <typename T>
__device__ __forceinline__ void classifier_ce_fwd_row(const T* hrow, const float* __restrict__ W, const float* __restrict__ bias,
                                                      const long long* __restrict__ labels, float* __restrict__ logits,
                                                      float* __restrict__ sample_loss, const int b, int K, int ncls,
                                                      const int lane) {
  float lg[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) lg[c] = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float x = Elem<T>::ld(hrow + k);
#pragma unroll
    for (int c = 0; c < 16; ++c)
      if (c < ncls) lg[c] += x * W[(size_t)c * K + k];
  }
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < 16; ++c)
    if (c < ncls) {
      lg[c] = wave_sum(lg[c]) + bias[c];
      mx = fmaxf(mx, lg[c]);
    }
  if (lane == 0) {
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c)
      if (c < ncls) {
        logits[(size_t)b * ncls + c] = lg[c];
        se += expf(lg[c] - mx);
      }
    if (labels && sample_loss) {
      const int y = (int)labels[b];
      float ly = 0.f;
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (c == y) ly = lg[c];
      sample_loss[b] = (mx + logf(se)) - ly;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void classifier_ce_fwd_kernel(const T* __restrict__ h, const float* __restrict__ W,
                                                                const float* __restrict__ bias,
                                                                const long long* __restrict__ labels,
                                                                float* __restrict__ logits, float* __restrict__ sample_loss,
                                                                int B, int K, int ncls) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  classifier_ce_fwd_row<T>(h + (size_t)b * K, W, bias, labels, logits, sample_loss, b, K, ncls, lane);
}

// *out = mean(v[0..n)) by one 256-thread workgroup.  COHERENT: v was written by other workgroups of the same launch (the loads
// bypass this CU's vector cache).
template <bool COHERENT>
__device__ __forceinline__ void block_mean256(const float* v, float* __restrict__ out, int n, float* red) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256)
    s += COHERENT ? __hip_atomic_load(v + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : v[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = red[0] / (float)n;
}

__global__ void mean_kernel(const float* __restrict__ v, float* __restrict__ out, int n) {
  __shared__ float red[256];
  block_mean256<false>(v, out, n, red);
}

// dlogits[b,c] = gloss * (softmax - onehot)/B + glogits[b,c];  dh[b,k] = (sum_c dlogits[b,c] W[c,k]) * gate(h>0)*gate_scale
// dl[c] = d loss / d logits[b, c] (0 for c >= ncls)
__device__ __forceinline__ void classifier_dlogits_row(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                       const float* __restrict__ gloss, const float* __restrict__ glogits,
                                                       const int b, int B, int ncls, float (&dl)[16]) {
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    dl[c] = 0.f;
    if (c < ncls) mx = fmaxf(mx, logits[(size_t)b * ncls + c]);
  }
  float se = 0.f;
#pragma unroll
  for (int c = 0; c < 16; ++c)
    if (c < ncls) {
      dl[c] = expf(logits[(size_t)b * ncls + c] - mx);
      se += dl[c];
    }
  const float gl = (gloss && labels) ? *gloss / (float)B : 0.f;
  const int y = labels ? (int)labels[b] : -1;
#pragma unroll
  for (int c = 0; c < 16; ++c)
    if (c < ncls) {
      float d = gl * (dl[c] / se - (c == y ? 1.f : 0.f));
      if (glogits) d += glogits[(size_t)b * ncls + c];
      dl[c] = d;
    }
}

// one wave, one sample: dlogits row and the gated dh row
template <typename T>
__device__ __forceinline__ void classifier_ce_bwd_row(const int b, const int lane, const T* __restrict__ h,
                                                      const float* __restrict__ W, const float* __restrict__ logits,
                                                      const long long* __restrict__ labels, const float* __restrict__ gloss,
                                                      const float* __restrict__ glogits, float* __restrict__ dlogits,
                                                      T* __restrict__ dh, int B, int K, int ncls, int use_gate,
                                                      float gate_scale) {
  float dl[16];
  classifier_dlogits_row(logits, labels, gloss, glogits, b, B, ncls, dl);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 16; ++c)
      if (c < ncls) dlogits[(size_t)b * ncls + c] = dl[c];
  }
  for (int k = lane; k < K; k += 64) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c)
      if (c < ncls) s += dl[c] * W[(size_t)c * K + k];
    if (use_gate) s = Elem<T>::ld(h + (size_t)b * K + k) > 0.f ? s * gate_scale : 0.f;
    Elem<T>::st(dh + (size_t)b * K + k, s);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void classifier_ce_bwd_kernel(const T* __restrict__ h, const float* __restrict__ W,
                                                                const float* __restrict__ logits,
                                                                const long long* __restrict__ labels,
                                                                const float* __restrict__ gloss,
                                                                const float* __restrict__ glogits,
                                                                float* __restrict__ dlogits, T* __restrict__ dh, int B,
                                                                int K, int ncls, int use_gate, float gate_scale) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  classifier_ce_bwd_row<T>(b, lane, h, W, logits, labels, gloss, glogits, dlogits, dh, B, K, ncls, use_gate, gate_scale);
}

// dW[c,k] = sum_b dlogits[b,c] h[b,k];  db[c] = sum_b dlogits[b,c]      grid = (ncls, ceil(K/64)); 64 columns x 4 batch lanes
template <typename T>
__global__ __launch_bounds__(256) void classifier_wgrad_kernel(const T* __restrict__ h, const float* __restrict__ dlogits,
                                                               float* __restrict__ dW, float* __restrict__ db, int B, int K,
                                                               int ncls) {
  __shared__ float red[4][64], redb[4];
  const int c = blockIdx.x, k = blockIdx.y * 64 + (threadIdx.x & 63), bl = threadIdx.x >> 6;
  float s = 0.f, sb = 0.f;
#pragma unroll 8
  for (int b = bl; b < B; b += 4) {
    const float dl = dlogits[(size_t)b * ncls + c];
    if (k < K) s = fmaf(dl, Elem<T>::ld(h + (size_t)b * K + k), s);
    sb += dl;
  }
  red[bl][threadIdx.x & 63] = s;
  if ((threadIdx.x & 63) == 0) redb[bl] = sb;
  __syncthreads();
  if (bl == 0) {
    const int kk = threadIdx.x & 63;
    if (k < K) dW[(size_t)c * K + k] = red[0][kk] + red[1][kk] + red[2][kk] + red[3][kk];
    if (blockIdx.y == 0 && kk == 0) db[c] = redb[0] + redb[1] + redb[2] + redb[3];
  }
}

// out[s, :] = sum_b dseq[b, s, :]  (position-embedding gradient; row 0 is also the cls_token gradient)
// grid = (rows, ceil(D/64)); 64 columns x 4 batch lanes per block
template <typename T>
__global__ __launch_bounds__(256) void batch_rowsum_kernel(const T* __restrict__ dseq, float* __restrict__ out, int NB, int S,
                                                           int D) {
  __shared__ float red[4][64];
  const int s = blockIdx.x, n = blockIdx.y * 64 + (threadIdx.x & 63), bl = threadIdx.x >> 6;
  float a = 0.f;
  if (n < D) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;   // four independent loads in flight per thread
    int b = bl;
    for (; b + 12 < NB; b += 16) {
      a0 += Elem<T>::ld(dseq + ((size_t)b * S + s) * D + n);
      a1 += Elem<T>::ld(dseq + ((size_t)(b + 4) * S + s) * D + n);
      a2 += Elem<T>::ld(dseq + ((size_t)(b + 8) * S + s) * D + n);
      a3 += Elem<T>::ld(dseq + ((size_t)(b + 12) * S + s) * D + n);
    }
    for (; b < NB; b += 4) a0 += Elem<T>::ld(dseq + ((size_t)b * S + s) * D + n);
    a = (a0 + a1) + (a2 + a3);
  }
  red[bl][threadIdx.x & 63] = a;
  __syncthreads();
  if (bl == 0 && n < D) {
    const int c = threadIdx.x & 63;
    out[(size_t)s * D + n] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
  }
}

// dst[b, r, :] = (src[b, off+r, :] (+ src[b+B2, off+r, :])) * (gate[b, r, :] > 0 ? gate_scale : 0)
//   dst rows are addressed by a rowmap (e.g. the zero-padded dY buffer of the strided-conv backward)
template <typename T>
__global__ void rows_gather_gate_kernel(const T* __restrict__ src, const T* __restrict__ gate, T* __restrict__ dst,
                                        RowMap dmap, int S, int D, int R, int off, int pair_shift, float gate_scale) {
  const int b = blockIdx.y, r = blockIdx.x;
  const T* s = src + ((size_t)b * S + off + r) * D;
  const T* s2 = pair_shift ? src + ((size_t)(b + pair_shift) * S + off + r) * D : nullptr;
  const T* gt = gate ? gate + ((size_t)b * R + r) * D : nullptr;
  T* d = dst + row_off(dmap, b * R + r);
  for (int n = threadIdx.x * 4; n < D; n += blockDim.x * 4) {
    float v[4];
    load4(s + n, v);
    if (s2) {
      float w[4];
      load4(s2 + n, w);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += w[e];
    }
    if (gt) {
      float gv[4];
      load4(gt + n, gv);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = gv[e] > 0.f ? v[e] * gate_scale : 0.f;
    }
    store4(d + n, v);
  }
}

// FuzzyGatingFusion.forward (3_Models/fusion/fuzzy_gating_fusion.py:297-390), one thread per sample, K <= 16 classes.
// prm = [tau_img, tau_eeg, c_unrel_img, c_unrel_eeg, ls_rel_img, ls_rel_eeg, ls_unrel_img, ls_unrel_eeg, beta0..3]
// mode: 0 full, 1 no_temperature, 2 no_fuzzification, 3 fixed_weights
__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float entropy_k(const float* z, int K, float eps_log) {
  float mx = -INFINITY, se = 0.f, h = 0.f;
  for (int c = 0; c < K; ++c) mx = fmaxf(mx, z[c]);
  for (int c = 0; c < K; ++c) se += expf(z[c] - mx);
  for (int c = 0; c < K; ++c) {
    const float p = expf(z[c] - mx) / se;
    h -= p * logf(p + eps_log);
  }
  return h;
}
__global__ void fuzzy_gate_fwd_kernel(const float* __restrict__ zi, const float* __restrict__ ze, const float* __restrict__ prm,
                                      float* __restrict__ fused, float* __restrict__ alpha_out, int B, int K, int mode,
                                      float eps_temp, float eps_log, float eps_div) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float a[16], e[16];
  float ti = 1.f, te = 1.f;
  if (mode == 0 || mode == 2) { ti = softplus_f(prm[0]) + eps_temp; te = softplus_f(prm[1]) + eps_temp; }
  for (int c = 0; c < K; ++c) { a[c] = zi[(size_t)b * K + c] / ti; e[c] = ze[(size_t)b * K + c] / te; }
  const float Hi = entropy_k(a, K, eps_log), He = entropy_k(e, K, eps_log);
  float al;
  if (mode == 3) {
    al = 0.5f;
  } else if (mode == 2) {
    const float hmax = logf((float)K);
    const float ci = fmaxf(1.0f - Hi / (hmax + eps_div), 0.f), ce = fmaxf(1.0f - He / (hmax + eps_div), 0.f);
    al = fminf(fmaxf(ci / (ci + ce + eps_div), 0.f), 1.f);
  } else {
    auto mu = [&](float x, float c, float ls) { const float s = expf(ls); return expf(-((x - c) * (x - c)) / (2.f * s * s + eps_div)); };
    const float ir = mu(Hi, 0.f, prm[4]), iu = mu(Hi, prm[2], prm[6]);
    const float er = mu(He, 0.f, prm[5]), eu = mu(He, prm[3], prm[7]);
    const float w[4] = {ir * eu, iu * er, ir * er, iu * eu};
    float num = 0.f, den = 0.f;
    for (int k = 0; k < 4; ++k) { num += w[k] / (1.f + expf(-prm[8 + k])); den += w[k]; }
    al = fminf(fmaxf(num / (den + eps_div), 0.f), 1.f);
  }
  alpha_out[b] = al;
  for (int c = 0; c < K; ++c) fused[(size_t)b * K + c] = al * a[c] + (1.f - al) * e[c];
}

// FuzzyGatingFusion backward: given d fused [B,K] and (optionally) d alpha [B], the gradients of both logit sets and of the
// 12 scalar parameters.  One thread per sample recomputes the forward (12 scalars, K <= 16 logits) and applies the chain rule
// by hand; parameter gradients are reduced over the block into partial[blockIdx][12] (summed in block order by the caller).
//   clamp(): torch passes the gradient where min <= x <= max (inclusive), as does this kernel.
__device__ __forceinline__ void entropy_bwd_k(const float* z, int K, float eps_log, float dH, float* dz) {
  // H = -sum p log(p + eps); dH/dp_c = -(log(p_c + eps) + p_c / (p_c + eps)); soft-max: dz_j = p_j (g_j - sum_c p_c g_c)
  float mx = -INFINITY, se = 0.f;
  for (int c = 0; c < K; ++c) mx = fmaxf(mx, z[c]);
  for (int c = 0; c < K; ++c) se += expf(z[c] - mx);
  float pg = 0.f;
  for (int c = 0; c < K; ++c) {
    const float p = expf(z[c] - mx) / se;
    pg += p * (-(logf(p + eps_log) + p / (p + eps_log)));
  }
  for (int c = 0; c < K; ++c) {
    const float p = expf(z[c] - mx) / se;
    const float g = -(logf(p + eps_log) + p / (p + eps_log));
    dz[c] += dH * p * (g - pg);
  }
}

__global__ __launch_bounds__(128) void fuzzy_gate_bwd_kernel(const float* __restrict__ zi, const float* __restrict__ ze,
                                                             const float* __restrict__ prm, const float* __restrict__ dfused,
                                                             const float* __restrict__ dalpha, float* __restrict__ dzi,
                                                             float* __restrict__ dze, float* __restrict__ partial, int B, int K,
                                                             int mode, float eps_temp, float eps_log, float eps_div) {
  __shared__ float red[2][12];
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  float dp[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) dp[i] = 0.f;
  if (b < B) {
    float a[16], e[16], da[16], de[16];
    float ti = 1.f, te = 1.f;
    const bool temp = (mode == 0 || mode == 2);
    if (temp) { ti = softplus_f(prm[0]) + eps_temp; te = softplus_f(prm[1]) + eps_temp; }
    for (int c = 0; c < K; ++c) { a[c] = zi[(size_t)b * K + c] / ti; e[c] = ze[(size_t)b * K + c] / te; }
    const float Hi = entropy_k(a, K, eps_log), He = entropy_k(e, K, eps_log);
    // ---- forward pieces needed again ----
    float al_pre = 0.5f;
    float ir = 0.f, iu = 0.f, er = 0.f, eu = 0.f, num = 0.f, den = 0.f, th[4] = {0.f, 0.f, 0.f, 0.f};
    float ci = 0.f, ce = 0.f, ci_raw = 0.f, ce_raw = 0.f;
    auto D_of = [&](float ls) { const float s = expf(ls); return 2.f * s * s + eps_div; };
    if (mode == 2) {
      const float hmax = logf((float)K);
      ci_raw = 1.0f - Hi / (hmax + eps_div); ce_raw = 1.0f - He / (hmax + eps_div);
      ci = fmaxf(ci_raw, 0.f); ce = fmaxf(ce_raw, 0.f);
      al_pre = ci / (ci + ce + eps_div);
    } else if (mode != 3) {
      ir = expf(-(Hi * Hi) / D_of(prm[4]));
      iu = expf(-((Hi - prm[2]) * (Hi - prm[2])) / D_of(prm[6]));
      er = expf(-(He * He) / D_of(prm[5]));
      eu = expf(-((He - prm[3]) * (He - prm[3])) / D_of(prm[7]));
      const float w[4] = {ir * eu, iu * er, ir * er, iu * eu};
      for (int k = 0; k < 4; ++k) { th[k] = 1.f / (1.f + expf(-prm[8 + k])); num += w[k] * th[k]; den += w[k]; }
      al_pre = num / (den + eps_div);
    }
    const float al = fminf(fmaxf(al_pre, 0.f), 1.f);
    // ---- fusion: fused = al * a + (1 - al) * e ----
    float dal = dalpha ? dalpha[b] : 0.f;
    for (int c = 0; c < K; ++c) {
      const float g = dfused[(size_t)b * K + c];
      da[c] = al * g;
      de[c] = (1.f - al) * g;
      dal += g * (a[c] - e[c]);
    }
    if (!(al_pre >= 0.f && al_pre <= 1.f)) dal = 0.f;
    float dHi = 0.f, dHe = 0.f;
    if (mode == 2) {
      const float s = ci + ce + eps_div, hmax = logf((float)K);
      const float dci = dal * (ce + eps_div) / (s * s), dce = -dal * ci / (s * s);
      if (ci_raw >= 0.f) dHi = -dci / (hmax + eps_div);
      if (ce_raw >= 0.f) dHe = -dce / (hmax + eps_div);
    } else if (mode != 3) {
      const float dd = den + eps_div;
      const float dnum = dal / dd, dden = -dal * num / (dd * dd);
      const float w[4] = {ir * eu, iu * er, ir * er, iu * eu};
      float dw[4];
      for (int k = 0; k < 4; ++k) {
        dw[k] = dnum * th[k] + dden;
        dp[8 + k] = dnum * w[k] * th[k] * (1.f - th[k]);
      }
      const float dir = dw[0] * eu + dw[2] * er, deu = dw[0] * ir + dw[3] * iu;
      const float diu = dw[1] * er + dw[3] * eu, der = dw[1] * iu + dw[2] * ir;
      // mu(x; c, ls) = exp(-(x-c)^2 / D), D = 2 exp(2 ls) + eps:  d/dx = mu * (-2 (x-c) / D), d/dc = -d/dx,
      //                                                          d/dls = mu * (x-c)^2 / D^2 * 4 exp(2 ls)
      auto mu_bwd = [&](float x, float c, float ls, float m, float dm, float& dx, float& dc, float& dls) {
        const float D = D_of(ls), s2 = expf(2.f * ls), t = x - c;
        const float gx = dm * m * (-2.f * t / D);
        dx += gx;
        dc -= gx;
        dls += dm * m * (t * t) / (D * D) * 4.f * s2;
      };
      float dummy = 0.f;
      mu_bwd(Hi, 0.f, prm[4], ir, dir, dHi, dummy, dp[4]);
      mu_bwd(Hi, prm[2], prm[6], iu, diu, dHi, dp[2], dp[6]);
      mu_bwd(He, 0.f, prm[5], er, der, dHe, dummy, dp[5]);
      mu_bwd(He, prm[3], prm[7], eu, deu, dHe, dp[3], dp[7]);
    }
    if (mode != 3) {
      entropy_bwd_k(a, K, eps_log, dHi, da);
      entropy_bwd_k(e, K, eps_log, dHe, de);
    }
    // ---- temperature: a = z / T, T = softplus(tau) + eps ----
    float dTi = 0.f, dTe = 0.f;
    for (int c = 0; c < K; ++c) {
      dzi[(size_t)b * K + c] = da[c] / ti;
      dze[(size_t)b * K + c] = de[c] / te;
      dTi -= da[c] * a[c] / ti;
      dTe -= de[c] * e[c] / te;
    }
    if (temp) {
      dp[0] = dTi / (1.f + expf(-prm[0]));   // softplus' = sigmoid
      dp[1] = dTe / (1.f + expf(-prm[1]));
    }
  }
  // block reduction of the 12 parameter gradients (2 waves of 64)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const float v = wave_sum(dp[i]);
    if (lane == 0) red[wv][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < 12) partial[(size_t)blockIdx.x * 12 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x];
}


// ------------------------------------------------------------------------------------------------
// Fused forms of the step's [B, d]-sized tail (d_model == 256, 16-bit compute dtypes).  Each replaces several of the launches
// above with one; the arithmetic keeps their order (same MFMA shape and K order as gemm_nt_kernel / tn_body, same rounding
// points, same summation trees), so every output has the bits the separate launches give.
// ------------------------------------------------------------------------------------------------

// eg_token_grad_tail: ONE pass over dseq [NB, S, D] gives out[s, :] = sum_b dseq[b, s, :] (batch_rowsum_kernel's sum: sixteen
// chains over b mod 16 -- lane bl of that kernel keeps chains bl, bl + 4, bl + 8, bl + 12 and folds its tail rows into the first
// -- combined as ((c0 + c4) + (c8 + c12)) per lane and then lane 0 + 1 + 2 + 3), the cls_token copy of row 0, and the gated
// rows dst[b, s - off, :] of rows_gather_gate_kernel.  grid = (S, D / 64); 256 threads = 16 chains x 16 four-column lanes.
template <typename T>
__global__ __launch_bounds__(256) void token_grad_tail_kernel(const T* __restrict__ dseq, const T* __restrict__ gate,
                                                              T* __restrict__ dst, RowMap dmap, float* __restrict__ out,
                                                              float* __restrict__ cls_out, int NB, int S, int D, int R, int off,
                                                              float gate_scale) {
  __shared__ float red[16][64];
  const int s = blockIdx.x, tx = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int n = blockIdx.y * 64 + tx * 4;
  const int bl = r & 3, j = r >> 2;
  const int iters = NB - 12 - bl > 0 ? (NB - 12 - bl + 15) / 16 : 0;   // trips of batch_rowsum_kernel's 16-row loop for lane bl
  const bool gather = s >= off && s - off < R;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  // rows b0, b0 + step, ... (cnt <= 8 of them): every load is requested before the first sum or store, the sums then run in row order
  auto rows8 = [&](int b0, int step, int cnt) {
    u32x2 dv[8], gv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int b = b0 + step * min(u, cnt - 1);
      dv[u] = *(const u32x2*)(dseq + ((size_t)b * S + s) * D + n);
      if (gather) gv[u] = *(const u32x2*)(gate + ((size_t)b * R + (s - off)) * D + n);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (u < cnt) {
        const int b = b0 + step * u;
        float v[4];
        load4((const T*)&dv[u], v);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += v[e];
        if (gather) {
          float g4[4];
          load4((const T*)&gv[u], g4);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = g4[e] > 0.f ? v[e] * gate_scale : 0.f;
          store4(dst + row_off(dmap, b * R + (s - off)) + n, v);
        }
      }
    }
  };
  for (int i = 0; i < iters; i += 8) rows8(r + 16 * i, 16, min(8, iters - i));
  if (j == 0) {
    const int b0 = bl + 16 * iters;
    if (b0 < NB) rows8(b0, 4, (NB - b0 + 3) / 4);      // at most three rows
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[r][tx * 4 + e] = acc[e];
  __syncthreads();
  if (threadIdx.x < 64) {
    const int c = threadIdx.x;
    float a[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) a[l] = (red[l][c] + red[l + 4][c]) + (red[l + 8][c] + red[l + 12][c]);
    const float t = a[0] + a[1] + a[2] + a[3];
    const int col = blockIdx.y * 64 + c;
    out[(size_t)s * D + col] = t;
    if (s == 0 && cls_out) cls_out[col] = t;
  }
}

constexpr int HD = 256;            // d_model of the fused head kernels
constexpr int HK = 3 * HD;         // width of comb / zf
constexpr int HP = HD + 8;         // LDS pitch (elements) of a 16-row operand image: 528 B, 16-B aligned, conflict-free b128 reads

// One wave, one 16 x 16 output tile: X[16 rows, 32 KS] * W[16 rows, 32 KS]^T.  The operand order (weights first) and the
// ascending k-steps in one accumulator are gemm_nt_kernel's, so the sums carry its bits.  Both operands come straight from global
// memory (L2-resident) as MFMA fragments: xrow / wrow are this lane's row, 8 g elements in.  What these launches cost is dependent
// load round trips, so a wave requests EVERY fragment of its product (2 KS 16-B loads per lane) before the first MFMA: one trip.
template <typename T, int KS>
__device__ __forceinline__ f32x4 slice_mma(const T* __restrict__ xrow, const T* __restrict__ wrow) {
  typedef typename H16<T>::frag frag;
  frag wf[KS], xf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) wf[ks] = *(const frag*)(wrow + 32 * ks);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) xf[ks] = *(const frag*)(xrow + 32 * ks);
  __builtin_amdgcn_sched_barrier(0);      // keep the loads above in one clause (the scheduler would sink them to their uses)
  f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) acc = H16<T>::mfma(wf[ks], xf[ks], acc);
  return acc;
}

// classifier_ce_fwd_row for R rows of one wave at once (hidden rows hs, hs + pitch, ...; samples b0 .. b0 + nrows - 1 are stored),
// K = 256, at most NC classes.  Every sum is that function's: per lane k = lane, lane + 64, ... ascending in one chain, wave_sum's
// butterfly, then the bias; the CE in class order.  What differs is when the loads are requested: there each class's weight is
// loaded behind its own `c < ncls` test and used at once, a dependent round trip per class and k-step (12 per row at 3 classes:
// 4.6 us per row, measured in-kernel); here all of them are requested before the first use (classes beyond ncls re-read the
// last class and are dropped), and the R x NC wave sums are independent chains that interleave.
template <typename T, int R, int NC>
__device__ __forceinline__ void classifier_ce_fwd_rows(const T* hs, const int pitch, const float* __restrict__ W,
                                                       const float* __restrict__ bias, const long long* __restrict__ labels,
                                                       float* __restrict__ logits, float* __restrict__ sample_loss, const int b0,
                                                       const int nrows, const int ncls, const int lane) {
  float w[NC][HD / 64], bs[NC], lg[R][NC];
  int y[R];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int cc = min(c, ncls - 1);
#pragma unroll
    for (int i = 0; i < HD / 64; ++i) w[c][i] = W[(size_t)cc * HD + lane + 64 * i];
    bs[c] = bias[cc];
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    y[r] = (labels && sample_loss && r < nrows) ? (int)labels[b0 + r] : -1;
#pragma unroll
    for (int c = 0; c < NC; ++c) lg[r][c] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < HD / 64; ++i)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float x = Elem<T>::ld(hs + (size_t)r * pitch + lane + 64 * i);
#pragma unroll
      for (int c = 0; c < NC; ++c) lg[r][c] += x * w[c][i];
    }
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int c = 0; c < NC; ++c) lg[r][c] = wave_sum(lg[r][c]) + bs[c];
  if (lane != 0) return;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (r >= nrows) break;
    const int b = b0 + r;
    float mx = -INFINITY, se = 0.f, ly = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < ncls) mx = fmaxf(mx, lg[r][c]);
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < ncls) {
        logits[(size_t)b * ncls + c] = lg[r][c];
        se += expf(lg[r][c] - mx);
        if (c == y[r]) ly = lg[r][c];
      }
    if (labels && sample_loss) sample_loss[b] = (mx + logf(se)) - ly;
  }
}

// Whether this workgroup is the LAST of `total` to arrive at *ctr (every thread of the workgroup calls it; `flag` is a word of LDS).
// What the workgroup stored before is visible to the whole device by then, and the last one may read what the others stored --
// with loads that bypass the vector cache (block_mean256<true>).  It also puts the counter back to zero for the next launch.
// ONE thread runs the device-scope fences, behind a barrier that has completed every wave's stores: on gfx950 a release at that
// scope is an L2 write-back (buffer_wbl2) and an acquire an invalidate (buffer_inv), which the XCD's L2 takes one at a time.
// With __threadfence() in every wave (256 waves, four fences each) these fences WERE the launch: 42 us of 42.
__device__ __forceinline__ bool last_arrival(unsigned int* ctr, const int total, int* flag) {
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const bool last = atomicAdd(ctr, 1u) == (unsigned)(total - 1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (last) *ctr = 0u;
    *flag = last;
  }
  __syncthreads();
  return *flag != 0;
}

// The head products are sliced over the GPU: a 256-thread workgroup owns 16 samples and HSL output columns, wave w the 16-column
// tile HSL s + 16 w.  blockIdx.x = group * (N / HSL) + slice.
constexpr int HSL = 64;

template <typename T>
struct HeadsFwd {
  const T* comb; T* zf; T* hcl; const T* Wsf; const T* Wc0;
  const float* bsf; const float* bc0; const float* W3; const float* b3;
  const long long* labels; float* logits; float* sloss; float* loss; unsigned int* counter;
  const eg_step_state* st;
  int B, ncls;
  DropCfg d1;
};

// eg_heads_fwd, launch 1: zf[:, :256] = comb Wsf^T + b.  grid = groups x 4 column slices.
template <typename T>
__global__ __launch_bounds__(256) void heads_fwd_sf_kernel(HeadsFwd<T> p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int m = (blockIdx.x / (HD / HSL)) * 16 + l15;        // rows beyond B: operands clamped, nothing stored
  const int n0 = (blockIdx.x % (HD / HSL)) * HSL + 16 * wave;
  const f32x4 acc = slice_mma<T, HK / 32>(p.comb + (size_t)min(m, p.B - 1) * HK + 8 * g, p.Wsf + (size_t)(n0 + l15) * HK + 8 * g);
  const int n = n0 + 4 * g;
  float bv[4], v[4];
  load4(p.bsf + n, bv);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = acc[e] + bv[e];
  if (m < p.B) store4(p.zf + (size_t)m * HK + n, v);
}

// eg_heads_fwd, launch 2 (the launch boundary hands it every column of zf): hcl = dropout(relu(zf Wc0^T + b)), same grid.  The
// pieces that need all 256 columns of hcl go to the workgroup that finishes LAST, found with device counters (no workgroup ever
// waits for another): per group of 16 samples (counter[1 + group]) the class projection and the per-sample CE on that group's
// rows of hcl, read back past this CU's vector cache into LDS; over the launch (counter[0], with labels) the mean of the
// per-sample losses in mean_kernel's order.  Whoever consumes a counter resets it, so the next launch or graph replay starts clean.
template <typename T>
__global__ __launch_bounds__(256) void heads_fwd_cls_kernel(HeadsFwd<T> p) {
  __shared__ __attribute__((aligned(16))) T hs[16][HP];
  __shared__ float red[256];
  __shared__ int last_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int grp = blockIdx.x / (HD / HSL), ngrp = gridDim.x / (HD / HSL);
  const int m0 = grp * 16, m = m0 + l15;
  const int n0 = (blockIdx.x % (HD / HSL)) * HSL + 16 * wave;
  const f32x4 acc = slice_mma<T, HK / 32>(p.zf + (size_t)min(m, p.B - 1) * HK + 8 * g, p.Wc0 + (size_t)(n0 + l15) * HK + 8 * g);
  uint32_t seed_lo = 0, seed_hi = 0;
  if (p.d1.thresh) {
    seed_lo = p.st->seed_lo;
    seed_hi = p.st->seed_hi;
  }
  {
    const int n = n0 + 4 * g;
    float bv[4], v[4];
    load4(p.bc0 + n, bv);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaxf(acc[e] + bv[e], 0.f);
    eg_dropout_run<4>(v, p.d1, seed_lo, seed_hi, (uint32_t)m * (uint32_t)HD + (uint32_t)n);
    if (m < p.B) store4(p.hcl + (size_t)m * HD + n, v);
  }
  if (!last_arrival(p.counter + 1 + grp, HD / HSL, &last_s)) return;
  for (int c = tid; c < 16 * (HD / 4); c += 256) {            // the group's 16 x 256 rows of hcl, 8-B pieces
    const int r = c / (HD / 4), ch = c % (HD / 4);
    const T* src = p.hcl + (size_t)min(m0 + r, p.B - 1) * HD + ch * 4;
    *(unsigned long long*)&hs[r][ch * 4] = __hip_atomic_load((const unsigned long long*)src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  {
    const int b0 = m0 + 4 * wave, nrows = min(4, p.B - b0);      // four rows per wave
    if (nrows > 0) {
      if (p.ncls <= 4)
        classifier_ce_fwd_rows<T, 4, 4>(&hs[4 * wave][0], HP, p.W3, p.b3, p.labels, p.logits, p.sloss, b0, nrows, p.ncls, lane);
      else
        classifier_ce_fwd_rows<T, 4, 16>(&hs[4 * wave][0], HP, p.W3, p.b3, p.labels, p.logits, p.sloss, b0, nrows, p.ncls, lane);
    }
  }
  if (!p.labels || !last_arrival(p.counter, ngrp, &last_s)) return;
  block_mean256<true>(p.sloss, p.loss, p.B, red);
}

// dW[n0 .. n0+63][k0 .. k0+63] = sum_m dY[m, n] X[m, k] (+ db = column sums of dY, from the k0 == 0 tiles) for M <= 256 rows,
// with the bits of eg_gemm_tn + eg_reduce_partials at that size: rows [0, 128) and [128, M) are two slabs, each one MFMA chain
// over ascending 32-row steps (tn_body's operand order: X first), the slabs added last; the bias sums run over 16-row halves of
// every 32-row step as tn_tile_colsum's do.  Rows >= M are staged as zeros (exact).  smem: 2 x 64 x TNP elements.
constexpr int TNP = 128 + 8;       // pitch (elements) of the transposed [64 columns][128 rows] operand images
template <typename T>
__device__ __forceinline__ void small_tn_tile(const T* __restrict__ dY, const int ldy, const T* __restrict__ X, const int ldx,
                                              float* __restrict__ dW, float* __restrict__ db, const int M, const int K,
                                              const int tile, char* smem) {
  typedef typename H16<T>::frag frag;
  T (*Yt)[TNP] = (T(*)[TNP])smem;
  T (*Xt)[TNP] = (T(*)[TNP])(smem + 64 * TNP * sizeof(T));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int tiles_k = K / 64;
  const int n0 = (tile / tiles_k) * 64, k0 = (tile % tiles_k) * 64;
  const int nsplit = M > 128 ? 2 : 1;
  // 4 waves: wave w takes k rows 16 w .. + 15 and all four 16-column tiles; 8 waves: tiles 2 (w / 4) and 2 (w / 4) + 1 only
  const int kw = wave & 3, t0 = (wave >> 2) * 2, t1 = blockDim.x == 512 ? t0 + 2 : 4;
  f32x4 acc[2][4];
#pragma unroll
  for (int sp = 0; sp < 2; ++sp)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[sp][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float bsplit[2] = {0.f, 0.f};
  for (int sp = 0; sp < nsplit; ++sp) {
    if (sp) __syncthreads();
    for (int c = tid; c < 1024; c += blockDim.x) {
      const int row = c >> 3, ch = c & 7;
      const int m = 128 * sp + row;
      u32x4 y = {0u, 0u, 0u, 0u}, x = {0u, 0u, 0u, 0u};
      if (m < M) {
        y = *(const u32x4*)(dY + (size_t)m * ldy + n0 + ch * 8);
        x = *(const u32x4*)(X + (size_t)m * ldx + k0 + ch * 8);
      }
      const uint16_t* ye = (const uint16_t*)&y;
      const uint16_t* xe = (const uint16_t*)&x;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        *(uint16_t*)&Yt[ch * 8 + e][row] = ye[e];
        *(uint16_t*)&Xt[ch * 8 + e][row] = xe[e];
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const frag xf = *(const frag*)&Xt[16 * kw + l15][32 * ks + 8 * g];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t >= t0 && t < t1) {
          const frag yf = *(const frag*)&Yt[16 * t + l15][32 * ks + 8 * g];
          acc[sp][t] = H16<T>::mfma(xf, yf, acc[sp][t]);
        }
    }
    if (db && k0 == 0 && tid < 64) {
      float bh[2] = {0.f, 0.f};
      for (int sub = 0; sub < 4; ++sub)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          float cs = 0.f;
#pragma unroll
          for (int i = 0; i < 16; ++i) cs += H16<T>::ld(Yt[tid][32 * sub + 16 * half + i]);
          bh[half] += cs;
        }
      bsplit[sp] = bh[0] + bh[1];
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (t >= t0 && t < t1) {
      const int n = n0 + 16 * t + l15, k = k0 + 16 * kw + 4 * g;
      f32x4 o = acc[0][t];
      if (nsplit == 2) o += acc[1][t];
      *(f32x4*)(dW + (size_t)n * K + k) = o;
    }
  if (db && k0 == 0 && tid < 64) db[n0 + tid] = nsplit == 2 ? bsplit[0] + bsplit[1] : bsplit[0];
}
constexpr int TN_SMEM = 2 * 64 * TNP * 2;    // 34 816 B

// classifier_dlogits_row for at most NC classes with every load requested before the first use (classes beyond ncls re-read the
// last one and give 0): the same arithmetic in the same order.  There each logit is loaded behind its own `c < ncls` test.
template <int NC>
__device__ __forceinline__ void classifier_dlogits_row_pre(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                           const float* __restrict__ gloss, const float* __restrict__ glogits,
                                                           const int b, int B, int ncls, float (&dl)[NC]) {
  float lg[NC], ge[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int cc = min(c, ncls - 1);
    lg[c] = logits[(size_t)b * ncls + cc];
    ge[c] = glogits ? glogits[(size_t)b * ncls + cc] : 0.f;
  }
  const float gl = (gloss && labels) ? *gloss / (float)B : 0.f;
  const int y = labels ? (int)labels[b] : -1;
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < ncls) mx = fmaxf(mx, lg[c]);
  float se = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    dl[c] = 0.f;
    if (c < ncls) {
      dl[c] = expf(lg[c] - mx);
      se += dl[c];
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < ncls) {
#pragma clang fp contract(off)      // there the product is rounded before the upstream gradient, loaded behind its own test, is added
      float d = gl * (dl[c] / se - (c == y ? 1.f : 0.f));
      if (glogits) d += ge[c];
      dl[c] = d;
    }
}

// eg_classifier_ce_bwd_fused: classifier_ce_bwd_kernel's rows (blocks [0, nce)) and classifier_wgrad_kernel's sums (blocks
// [nce, ..): one per 64 columns of h, all classes) in ONE launch.  A weight-gradient block derives the dlogits itself (the same
// function of logits / labels / upstream gradients the row blocks store) instead of waiting for another launch to have written
// them, and stages its [B, 64] slice of h in LDS with every load in flight at once; the sums keep classifier_wgrad_kernel's order
// (four lanes over b mod 4, ascending b, then lane 0 + 1 + 2 + 3).  B <= 256.
// What the launch cost was dependent trips, measured in-kernel (B = 256, 3 classes): a row block's loads sat one by one behind
// their `c < ncls` tests (6.4 us), and a weight block's batch loop waited for four LDS reads per sample, 64 samples in a row
// (16.4 us of the launch's 23.5).  So the body is built for at most NC = 4 or 16 classes: every load of a phase is requested before
// its first use (classes beyond ncls re-read the last one and are dropped), and the batch loop reads a sample's dlogits as 16-B
// vectors (zero beyond ncls: exact) eight samples ahead.  The sums and their order are unchanged.
template <typename T, int NC>
__device__ __forceinline__ void classifier_ce_bwd_fused_body(const T* __restrict__ h, const float* __restrict__ W,
                                                             const float* __restrict__ logits, const long long* __restrict__ labels,
                                                             const float* __restrict__ gloss, const float* __restrict__ glogits,
                                                             float* __restrict__ dlogits, T* __restrict__ dh, float* __restrict__ dW,
                                                             float* __restrict__ db, int B, int K, int ncls, int use_gate,
                                                             float gate_scale, int nce, T (*hts)[64], float (*dls)[16],
                                                             float (*red)[64], float* redb) {
  const int lane = threadIdx.x & 63, bl = threadIdx.x >> 6;
  if ((int)blockIdx.x < nce) {                                 // classifier_ce_bwd_row's sample, one per wave
    const int b = blockIdx.x * 4 + bl;
    if (b >= B) return;
    float dl[NC];
    classifier_dlogits_row_pre<NC>(logits, labels, gloss, glogits, b, B, ncls, dl);
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < ncls) dlogits[(size_t)b * ncls + c] = dl[c];
    }
    for (int k0 = lane; k0 < K; k0 += 256) {
      float w[4][NC], hv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kk = min(k0 + 64 * j, K - 1);
#pragma unroll
        for (int c = 0; c < NC; ++c) w[j][c] = W[(size_t)min(c, ncls - 1) * K + kk];
        hv[j] = use_gate ? Elem<T>::ld(h + (size_t)b * K + kk) : 1.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (c < ncls) s += dl[c] * w[j][c];
        if (use_gate) s = hv[j] > 0.f ? s * gate_scale : 0.f;
        if (k0 + 64 * j < K) Elem<T>::st(dh + (size_t)b * K + k0 + 64 * j, s);
      }
    }
    return;
  }
  const int kb = (blockIdx.x - nce) * 64, k = kb + lane;
  const bool wide = kb + 64 <= K && K % 8 == 0;
  for (int c = threadIdx.x; c < B * 8; c += 256) {           // 16-B chunks of the [B, 64] slice
    const int b = c >> 3, ch = c & 7;
    if (wide) *(u32x4*)&hts[b][ch * 8] = *(const u32x4*)(h + (size_t)b * K + kb + ch * 8);
    else
      for (int e = 0; e < 8; ++e)
        if (kb + ch * 8 + e < K) hts[b][ch * 8 + e] = h[(size_t)b * K + kb + ch * 8 + e];
  }
  for (int b = threadIdx.x; b < B; b += 256) {
    float dl[NC];
    classifier_dlogits_row_pre<NC>(logits, labels, gloss, glogits, b, B, ncls, dl);
#pragma unroll
    for (int c = 0; c < NC; ++c) dls[b][c] = dl[c];
  }
  __syncthreads();
  float s[NC], sb[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) s[c] = sb[c] = 0.f;
#pragma unroll 8
  for (int b = bl; b < B; b += 4) {
    const float hv = H16<T>::ld(hts[b][lane]);
#pragma unroll
    for (int c4 = 0; c4 < NC; c4 += 4) {
      const f32x4 d4 = *(const f32x4*)&dls[b][c4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (k < K) s[c4 + e] = fmaf(d4[e], hv, s[c4 + e]);
        sb[c4 + e] += d4[e];
      }
    }
  }
  // the four batch lanes combined, class by class
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < ncls) {
      red[bl][lane] = s[c];
      if (lane == 0) redb[bl] = sb[c];
      __syncthreads();
      if (bl == 0) {
        if (k < K) dW[(size_t)c * K + k] = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
        if (kb == 0 && lane == 0) db[c] = redb[0] + redb[1] + redb[2] + redb[3];
      }
      __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(256) void classifier_ce_bwd_fused_kernel(const T* __restrict__ h, const float* __restrict__ W,
                                                                      const float* __restrict__ logits,
                                                                      const long long* __restrict__ labels,
                                                                      const float* __restrict__ gloss,
                                                                      const float* __restrict__ glogits,
                                                                      float* __restrict__ dlogits, T* __restrict__ dh,
                                                                      float* __restrict__ dW, float* __restrict__ db, int B,
                                                                      int K, int ncls, int use_gate, float gate_scale, int nce) {
  __shared__ __attribute__((aligned(16))) T hts[256][64];
  __shared__ __attribute__((aligned(16))) float dls[256][16];
  __shared__ float red[4][64], redb[4];
  if (ncls <= 4)
    classifier_ce_bwd_fused_body<T, 4>(h, W, logits, labels, gloss, glogits, dlogits, dh, dW, db, B, K, ncls, use_gate, gate_scale, nce,
                                       hts, dls, red, redb);
  else
    classifier_ce_bwd_fused_body<T, 16>(h, W, logits, labels, gloss, glogits, dlogits, dh, dW, db, B, K, ncls, use_gate, gate_scale, nce,
                                        hts, dls, red, redb);
}

// eg_heads_bwd_chain, launch 1: blocks [0, 12 nrt): dzf = dhcl Wc0, one (16 samples, 64 of the 768 columns) slice each, all
// columns stored; blocks [12 nrt, 12 nrt + 48): classifier.0's weight and bias gradient tiles (dhcl^T zf), which need nothing of
// this launch and fill the CUs the slices leave free.
template <typename T>
__global__ __launch_bounds__(256) void heads_bwd_dzf_kernel(const T* __restrict__ dhcl, const T* __restrict__ c0T,
                                                            const T* __restrict__ zf, T* __restrict__ dzf,
                                                            float* __restrict__ dWc0, float* __restrict__ dbc0, int B, int nsl) {
  __shared__ __attribute__((aligned(16))) char smem[TN_SMEM];
  if ((int)blockIdx.x >= nsl) {
    small_tn_tile<T>(dhcl, HD, zf, HK, dWc0, dbc0, B, HK, blockIdx.x - nsl, smem);
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int m = (blockIdx.x / (HK / HSL)) * 16 + l15;
  const int n0 = (blockIdx.x % (HK / HSL)) * HSL + 16 * wave;
  const f32x4 acc = slice_mma<T, HD / 32>(dhcl + (size_t)min(m, B - 1) * HD + 8 * g, c0T + (size_t)(n0 + l15) * HD + 8 * g);
  const float v[4] = {acc[0] + 0.f, acc[1] + 0.f, acc[2] + 0.f, acc[3] + 0.f};   // (gemm_nt's bias-free epilogue adds 0)
  if (m < B) store4(dzf + (size_t)m * HK + n0 + 4 * g, v);
}

// eg_heads_bwd_chain, launch 2 (every column of dzf[:, :256] is there at the launch boundary): dcomb = dzf[:, :256] Wsf, same slices.
template <typename T>
__global__ __launch_bounds__(256) void heads_bwd_dcomb_kernel(const T* __restrict__ dzf, const T* __restrict__ sfT,
                                                              T* __restrict__ dcomb, int B) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int m = (blockIdx.x / (HK / HSL)) * 16 + l15;
  const int n0 = (blockIdx.x % (HK / HSL)) * HSL + 16 * wave;
  const f32x4 acc = slice_mma<T, HD / 32>(dzf + (size_t)min(m, B - 1) * HK + 8 * g, sfT + (size_t)(n0 + l15) * HD + 8 * g);
  const float v[4] = {acc[0] + 0.f, acc[1] + 0.f, acc[2] + 0.f, acc[3] + 0.f};
  if (m < B) store4(dcomb + (size_t)m * HK + n0 + 4 * g, v);
}

// eg_heads_bwd_pool: blocks [0, B): pool_fuse_bwd_kernel's samples; blocks [B, B + 48): symmetric_fusion.proj's weight and
// bias gradient tiles (dzf[:, :256]^T comb).
template <typename T>
__global__ __launch_bounds__(256) void heads_bwd_pool_kernel(const T* __restrict__ z, const T* __restrict__ dcomb,
                                                             const T* __restrict__ dzf, const float* __restrict__ gcls1,
                                                             const float* __restrict__ gcls2, const T* __restrict__ dibs_pool,
                                                             const float* __restrict__ gibs_pool, T* __restrict__ dz,
                                                             const T* __restrict__ comb, float* __restrict__ dWsf,
                                                             float* __restrict__ dbsf, int B, int S, int D, int off, int n_ibs,
                                                             int ibs_first) {
  __shared__ __attribute__((aligned(16))) char smem[TN_SMEM];
  if ((int)blockIdx.x >= B) {
    small_tn_tile<T>(dzf, HK, comb, HK, dWsf, dbsf, B, HK, blockIdx.x - B, smem);
    return;
  }
  pool_fuse_bwd_sample<T>(blockIdx.x, z, dcomb, dzf, gcls1, gcls2, dibs_pool, gibs_pool, dz, B, S, D, off, n_ibs, ibs_first);
}

}  // namespace

extern "C" int eg_rows_bcast_f32(const float* src, const float* pos, void* seq, int NB, int S, int D, int R, int off,
                                 int src_nb, int dtype, void* stream) {
  if (eg_dtype_check("eg_rows_bcast_f32", dtype, true)) return 1;
  EG_CHECK(src && seq && NB > 0 && R > 0 && off >= 0 && off + R <= S && src_nb > 0, "eg_rows_bcast_f32: bad arguments");
  dim3 grid(R, NB);
  hipStream_t s = (hipStream_t)stream;
  eg_dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(rows_bcast_f32_kernel<T>, grid, dim3(256), 0, s, src, pos, (T*)seq, NB, S, D, R, off, src_nb);
  });
  EG_LAUNCH_CHECK("rows_bcast_f32");
  return 0;
}

extern "C" int eg_rows_copy(void* seq, int S, int D, int R, int off, int b_src0, int b_dst0, int nb, int dtype,
                            void* stream) {
  if (eg_dtype_check("eg_rows_copy", dtype, true)) return 1;
  EG_CHECK(seq && nb > 0 && R > 0 && off >= 0 && off + R <= S, "eg_rows_copy: bad arguments");
  dim3 grid(R, nb);
  hipStream_t s = (hipStream_t)stream;
  eg_dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(rows_copy_kernel<T>, grid, dim3(256), 0, s, (T*)seq, S, D, R, off, b_src0, b_dst0);
  });
  EG_LAUNCH_CHECK("rows_copy");
  return 0;
}

extern "C" int eg_pool_fuse_fwd(const void* z, float* cls1, float* cls2, void* comb, void* zf, float* ibs_pool_f,
                                void* ibs_pool, int B, int S, int D, int off, int n_ibs, int ibs_first, int dtype,
                                void* stream) {
  if (eg_dtype_check("eg_pool_fuse_fwd", dtype, true)) return 1;
  EG_CHECK(z && cls1 && cls2 && comb && zf, "eg_pool_fuse_fwd: null pointer");
  EG_CHECK(B > 0 && off > 0 && off < S, "eg_pool_fuse_fwd: bad shape");
  EG_CHECK(n_ibs == 0 || (ibs_pool_f && ibs_pool && ibs_first >= 1 && ibs_first + n_ibs <= S), "eg_pool_fuse_fwd: ibs range");
  hipStream_t s = (hipStream_t)stream;
  eg_dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(pool_fuse_fwd_kernel<T>, dim3(B), dim3(256), 0, s, (const T*)z, cls1, cls2, (T*)comb, (T*)zf, ibs_pool_f,
                       (T*)ibs_pool, B, S, D, off, n_ibs, ibs_first);
  });
  EG_LAUNCH_CHECK("pool_fuse_fwd");
  return 0;
}

extern "C" int eg_pool_fuse_bwd(const void* z, const void* dcomb, const void* dzf, const float* gcls1, const float* gcls2,
                                const void* dibs_pool, const float* gibs_pool, void* dz, int B, int S, int D, int off,
                                int n_ibs, int ibs_first, int dtype, void* stream) {
  if (eg_dtype_check("eg_pool_fuse_bwd", dtype, true)) return 1;
  EG_CHECK(z && dcomb && dzf && dz, "eg_pool_fuse_bwd: null pointer");
  EG_CHECK(B > 0 && off > 0 && off < S, "eg_pool_fuse_bwd: bad shape");
  hipStream_t s = (hipStream_t)stream;
  eg_dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(pool_fuse_bwd_kernel<T>, dim3(B), dim3(256), 0, s, (const T*)z, (const T*)dcomb, (const T*)dzf, gcls1, gcls2,
                       (const T*)dibs_pool, gibs_pool, (T*)dz, B, S, D, off, n_ibs, ibs_first);
  });
  EG_LAUNCH_CHECK("pool_fuse_bwd");
  return 0;
}

extern "C" int eg_classifier_ce_fwd(const void* h, const float* W, const float* bias, const int64_t* labels,
                                    float* logits, float* sample_loss, float* loss, int B, int K, int ncls, int dtype,
                                    void* stream) {
  if (eg_dtype_check("eg_classifier_ce_fwd", dtype, true)) return 1;
  EG_CHECK(h && W && bias && logits, "eg_classifier_ce_fwd: null pointer");
  EG_CHECK(B > 0 && K > 0 && ncls > 0 && ncls <= 16, "eg_classifier_ce_fwd: ncls=%d must be in [1,16]", ncls);
  EG_CHECK(!labels || (sample_loss && loss), "eg_classifier_ce_fwd: labels need sample_loss and loss outputs");
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((B + 3) / 4);
  eg_dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(classifier_ce_fwd_kernel<T>, grid, dim3(256), 0, s, (const T*)h, W, bias, (const long long*)labels, logits,
                       sample_loss, B, K, ncls);
  });
  if (labels) hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, s, sample_loss, loss, B);
  EG_LAUNCH_CHECK("classifier_ce_fwd");
  return 0;
}

extern "C" int eg_classifier_ce_bwd(const void* h, const float* W, const float* logits, const int64_t* labels,
                                    const float* gloss, const float* glogits, float* dlogits, void* dh, float* dW,
                                    float* db, int B, int K, int ncls, int use_gate, float gate_scale, int dtype,
                                    void* stream) {
  if (eg_dtype_check("eg_classifier_ce_bwd", dtype, true)) return 1;
  EG_CHECK(h && W && logits && dlogits && dh && dW && db, "eg_classifier_ce_bwd: null pointer");
  EG_CHECK(B > 0 && K > 0 && ncls > 0 && ncls <= 16, "eg_classifier_ce_bwd: bad shape");
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((B + 3) / 4);
  eg_dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(classifier_ce_bwd_kernel<T>, grid, dim3(256), 0, s, (const T*)h, W, logits, (const long long*)labels, gloss,
                       glogits, dlogits, (T*)dh, B, K, ncls, use_gate, gate_scale);
    hipLaunchKernelGGL(classifier_wgrad_kernel<T>, dim3(ncls, (K + 63) / 64), dim3(256), 0, s, (const T*)h, dlogits, dW, db, B, K, ncls);
  });
  EG_LAUNCH_CHECK("classifier_ce_bwd");
  return 0;
}

extern "C" int eg_batch_rowsum(const void* dseq, float* out, int NB, int S, int D, int rows, int dtype, void* stream) {
  if (eg_dtype_check("eg_batch_rowsum", dtype, true)) return 1;
  EG_CHECK(dseq && out && NB > 0 && rows > 0 && rows <= S, "eg_batch_rowsum: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  eg_dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(batch_rowsum_kernel<T>, dim3(rows, (D + 63) / 64), dim3(256), 0, s, (const T*)dseq, out, NB, S, D);
  });
  EG_LAUNCH_CHECK("batch_rowsum");
  return 0;
}

extern "C" int eg_rows_gather_gate(const void* src, const void* gate, void* dst, eg_rowmap dmap, int nb, int S, int D,
                                   int R, int off, int pair_shift, float gate_scale, int dtype, void* stream) {
  if (eg_dtype_check("eg_rows_gather_gate", dtype, true)) return 1;
  EG_CHECK(src && dst && nb > 0 && R > 0 && off >= 0 && off + R <= S && D % 4 == 0, "eg_rows_gather_gate: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(R, nb);
  eg_dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(rows_gather_gate_kernel<T>, grid, dim3(64), 0, s, (const T*)src, (const T*)gate, (T*)dst, to_rowmap(dmap), S, D, R,
                       off, pair_shift, gate_scale);
  });
  EG_LAUNCH_CHECK("rows_gather_gate");
  return 0;
}

// ------------------------------------------------------------------------------------------------
// fused tail entry points (16-bit compute dtypes, d_model == 256)
// ------------------------------------------------------------------------------------------------
extern "C" int eg_token_grad_tail(const void* dseq, const void* gate, void* dst, eg_rowmap dmap, float* pos_grad,
                                  float* cls_grad, int NB, int S, int D, int R, int off, float gate_scale, int dtype,
                                  void* stream) {
  if (eg_dtype_check("eg_token_grad_tail", dtype, false)) return 1;
  EG_CHECK(dseq && gate && dst && pos_grad, "eg_token_grad_tail: null pointer");
  EG_CHECK(NB > 0 && S > 0 && R > 0 && off >= 0 && off + R <= S, "eg_token_grad_tail: bad shape NB=%d S=%d R=%d off=%d", NB, S, R, off);
  EG_CHECK(D > 0 && D % 64 == 0, "eg_token_grad_tail: D=%d must be a multiple of 64", D);
  EG_CHECK(dmap.row_stride % 4 == 0 && dmap.group_stride % 4 == 0, "eg_token_grad_tail: destination rows must be 8-B aligned");
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(S, D / 64);
  eg_dispatch_16(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(token_grad_tail_kernel<T>, grid, dim3(256), 0, s, (const T*)dseq, (const T*)gate, (T*)dst, to_rowmap(dmap), pos_grad,
                       cls_grad, NB, S, D, R, off, gate_scale);
  });
  EG_LAUNCH_CHECK("token_grad_tail");
  return 0;
}

template <typename T>
static void launch_heads_fwd(const void* comb, void* zf, void* hcl, const void* Wsf, const float* bsf, const void* Wc0,
                             const float* bc0, const float* W3, const float* b3, const int64_t* labels, float* logits,
                             float* sloss, float* loss, uint32_t* counter, int B, int ncls, float drop_p, uint32_t drop_site,
                             const eg_step_state* state, hipStream_t s) {
  HeadsFwd<T> p;
  p.comb = (const T*)comb; p.zf = (T*)zf; p.hcl = (T*)hcl; p.Wsf = (const T*)Wsf; p.Wc0 = (const T*)Wc0;
  p.bsf = bsf; p.bc0 = bc0; p.W3 = W3; p.b3 = b3;
  p.labels = (const long long*)labels; p.logits = logits; p.sloss = sloss; p.loss = loss; p.counter = counter;
  p.st = state; p.B = B; p.ncls = ncls; p.d1 = make_drop(drop_p, drop_site);
  const dim3 grid(((B + 15) / 16) * (HD / HSL));
  hipLaunchKernelGGL(heads_fwd_sf_kernel<T>, grid, dim3(256), 0, s, p);
  hipLaunchKernelGGL(heads_fwd_cls_kernel<T>, grid, dim3(256), 0, s, p);
}

extern "C" int eg_heads_fwd(const void* comb, void* zf, void* hcl, const void* Wsf, const float* bsf, const void* Wc0,
                            const float* bc0, const float* W3, const float* b3, const int64_t* labels, float* logits,
                            float* sample_loss, float* loss, uint32_t* counter, int B, int D, int ncls, float drop_p,
                            uint32_t drop_site, const eg_step_state* state, int dtype, void* stream) {
  if (eg_dtype_check("eg_heads_fwd", dtype, false)) return 1;
  EG_CHECK(comb && zf && hcl && Wsf && bsf && Wc0 && bc0 && W3 && b3 && logits, "eg_heads_fwd: null pointer");
  EG_CHECK(D == HD, "eg_heads_fwd: d_model=%d (the fused heads are built for 256)", D);
  EG_CHECK(B > 0 && ncls > 0 && ncls <= 16, "eg_heads_fwd: B=%d, ncls=%d must be in [1,16]", B, ncls);
  EG_CHECK(!labels || (sample_loss && loss && counter), "eg_heads_fwd: labels need sample_loss, loss and the launch counter");
  EG_CHECK(drop_p >= 0.f && drop_p < 1.f && (drop_p == 0.f || state), "eg_heads_fwd: dropout needs the step state");
  EG_CHECK(((uintptr_t)comb | (uintptr_t)zf | (uintptr_t)hcl | (uintptr_t)Wsf | (uintptr_t)Wc0 | (uintptr_t)bsf | (uintptr_t)bc0) % 16 == 0,
           "eg_heads_fwd: alignment");
  EG_CHECK(counter, "eg_heads_fwd: the launch counters (1 + ceil(B / 16) zeroed words) are needed with and without labels");
  hipStream_t s = (hipStream_t)stream;
  eg_dispatch_16(dtype, [&](auto t) {
    launch_heads_fwd<typename decltype(t)::type>(comb, zf, hcl, Wsf, bsf, Wc0, bc0, W3, b3, labels, logits, sample_loss, loss, counter, B,
                                                 ncls, drop_p, drop_site, state, s);
  });
  EG_LAUNCH_CHECK("heads_fwd");
  return 0;
}

extern "C" int eg_classifier_ce_bwd_fused(const void* h, const float* W, const float* logits, const int64_t* labels,
                                          const float* gloss, const float* glogits, float* dlogits, void* dh, float* dW,
                                          float* db, int B, int K, int ncls, int use_gate, float gate_scale, int dtype,
                                          void* stream) {
  if (eg_dtype_check("eg_classifier_ce_bwd_fused", dtype, false)) return 1;
  EG_CHECK(h && W && logits && dlogits && dh && dW && db, "eg_classifier_ce_bwd_fused: null pointer");
  EG_CHECK(B > 0 && B <= 256 && K > 0 && ncls > 0 && ncls <= 16, "eg_classifier_ce_bwd_fused: bad shape B=%d (<= 256) K=%d ncls=%d", B, K, ncls);
  EG_CHECK((uintptr_t)h % 16 == 0, "eg_classifier_ce_bwd_fused: alignment");
  hipStream_t s = (hipStream_t)stream;
  const int nce = (B + 3) / 4;
  dim3 grid(nce + (K + 63) / 64);
  eg_dispatch_16(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(classifier_ce_bwd_fused_kernel<T>, grid, dim3(256), 0, s, (const T*)h, W, logits, (const long long*)labels, gloss,
                       glogits, dlogits, (T*)dh, dW, db, B, K, ncls, use_gate, gate_scale, nce);
  });
  EG_LAUNCH_CHECK("classifier_ce_bwd_fused");
  return 0;
}

extern "C" int eg_heads_bwd_chain(const void* dhcl, const void* c0T, const void* sfT, const void* zf, void* dzf, void* dcomb,
                                  float* dWc0, float* dbc0, int B, int D, int dtype, void* stream) {
  if (eg_dtype_check("eg_heads_bwd_chain", dtype, false)) return 1;
  EG_CHECK(dhcl && c0T && sfT && zf && dzf && dcomb && dWc0 && dbc0, "eg_heads_bwd_chain: null pointer");
  EG_CHECK(D == HD, "eg_heads_bwd_chain: d_model=%d (the fused heads are built for 256)", D);
  EG_CHECK(B > 0 && B <= 256, "eg_heads_bwd_chain: B=%d (the in-launch weight gradients sum at most 256 rows)", B);
  EG_CHECK(((uintptr_t)dhcl | (uintptr_t)c0T | (uintptr_t)sfT | (uintptr_t)zf | (uintptr_t)dzf | (uintptr_t)dcomb | (uintptr_t)dWc0) % 16 == 0,
           "eg_heads_bwd_chain: alignment");
  hipStream_t s = (hipStream_t)stream;
  const int nsl = ((B + 15) / 16) * (HK / HSL);
  eg_dispatch_16(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(heads_bwd_dzf_kernel<T>, dim3(nsl + (HD / 64) * (HK / 64)), dim3(256), 0, s, (const T*)dhcl, (const T*)c0T,
                       (const T*)zf, (T*)dzf, dWc0, dbc0, B, nsl);
    hipLaunchKernelGGL(heads_bwd_dcomb_kernel<T>, dim3(nsl), dim3(256), 0, s, (const T*)dzf, (const T*)sfT, (T*)dcomb, B);
  });
  EG_LAUNCH_CHECK("heads_bwd_chain");
  return 0;
}

extern "C" int eg_heads_bwd_pool(const void* z, const void* dcomb, const void* dzf, const float* gcls1, const float* gcls2,
                                 const void* dibs_pool, const float* gibs_pool, void* dz, const void* comb, float* dWsf,
                                 float* dbsf, int B, int S, int D, int off, int n_ibs, int ibs_first, int dtype, void* stream) {
  if (eg_dtype_check("eg_heads_bwd_pool", dtype, false)) return 1;
  EG_CHECK(z && dcomb && dzf && dz && comb && dWsf && dbsf, "eg_heads_bwd_pool: null pointer");
  EG_CHECK(D == HD, "eg_heads_bwd_pool: d_model=%d (the fused heads are built for 256)", D);
  EG_CHECK(B > 0 && B <= 256 && off > 0 && off < S, "eg_heads_bwd_pool: bad shape B=%d (<= 256) S=%d off=%d", B, S, off);
  EG_CHECK(n_ibs == 0 || (ibs_first >= 1 && ibs_first + n_ibs <= S), "eg_heads_bwd_pool: ibs range");
  EG_CHECK(((uintptr_t)dzf | (uintptr_t)comb | (uintptr_t)dWsf) % 16 == 0, "eg_heads_bwd_pool: alignment");
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(B + (HD / 64) * (HK / 64));
  eg_dispatch_16(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(heads_bwd_pool_kernel<T>, grid, dim3(256), 0, s, (const T*)z, (const T*)dcomb, (const T*)dzf, gcls1, gcls2,
                       (const T*)dibs_pool, gibs_pool, (T*)dz, (const T*)comb, dWsf, dbsf, B, S, D, off, n_ibs, ibs_first);
  });
  EG_LAUNCH_CHECK("heads_bwd_pool");
  return 0;
}

// ------------------------------------------------------------------------------------------------
// The loss of the multimodal logit-fusion step and its gradients on the [B, K] logits, in ONE single-workgroup launch
// (train_multimodal_fuzzy_fusion.py:436-460): L = CE(fused) + l_img CE(z_img / T_img) + l_eeg CE(z_eeg / T_eeg) + l_reg R(T),
// temperatures DETACHED in the auxiliary terms (fuzzy_gating_fusion.py:334), R = relu(T - t_max) + relu(t_min - T) over both
// temperatures (:392-419), T = softplus(tau) + eps_temp.  As torch autograd on 2 x [B, 3] tensors this was ~70 tiny launches with
// 10-40 us of host time between them: 0.8 ms of idle GPU per step of BASELINE configs[4].
//   losses[5] = total, ce, aux_img, aux_eeg, reg
//   dfused    = dL/dfused  (feed eg_fuzzy_gate_bwd);  daux_img / daux_eeg = the auxiliary terms' direct gradients on the logits
//   dtau[2]   = l_reg dR/dtau_img, l_reg dR/dtau_eeg
// every gradient is multiplied by the loss scale of `state` when its scaler is on (GradScaler.scale(loss).backward(), :462).
// Summation over the batch in a fixed order (deterministic).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fusion_loop_loss_kernel(const float* __restrict__ fused, const float* __restrict__ zi,
                                                               const float* __restrict__ ze, const long long* __restrict__ labels,
                                                               const float* __restrict__ prm, float* __restrict__ losses,
                                                               float* __restrict__ dfused, float* __restrict__ dai,
                                                               float* __restrict__ dae, float* __restrict__ dtau, int B, int K,
                                                               int mode, float eps_temp, float l_img, float l_eeg, float l_reg,
                                                               float t_min, float t_max, const eg_step_state* st) {
  __shared__ float red[3][256];
  const float scale = (st && st->scaler_on) ? st->loss_scale : 1.0f;
  float ti = 1.f, te = 1.f;
  if (mode == 0 || mode == 2) { ti = softplus_f(prm[0]) + eps_temp; te = softplus_f(prm[1]) + eps_temp; }
  const float invB = 1.0f / (float)B;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int b = threadIdx.x; b < B; b += 256) {
    const int y = (int)labels[b];
    const float* rows[3] = {fused + (size_t)b * K, zi + (size_t)b * K, ze + (size_t)b * K};
    float* outs[3] = {dfused + (size_t)b * K, dai + (size_t)b * K, dae + (size_t)b * K};
    const float tdiv[3] = {1.f, ti, te};
    const float wgt[3] = {1.f, l_img, l_eeg};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      float z[16], mx = -INFINITY, se = 0.f;
      for (int c = 0; c < K; ++c) { z[c] = rows[q][c] / tdiv[q]; mx = fmaxf(mx, z[c]); }
      for (int c = 0; c < K; ++c) se += expf(z[c] - mx);
      const float lse = mx + logf(se);
      acc[q] += lse - z[y];                                    // -log softmax(z)[y]
      const float g = wgt[q] * invB * scale / tdiv[q];
      for (int c = 0; c < K; ++c) outs[q][c] = (expf(z[c] - lse) - (c == y ? 1.f : 0.f)) * g;
    }
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) red[q][threadIdx.x] = acc[q];
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot[3] = {0.f, 0.f, 0.f};
    for (int q = 0; q < 3; ++q) {
      for (int i = 0; i < 256; ++i) tot[q] += red[q][i];
      tot[q] *= invB;
    }
    // the regulariser always reads the learnable temperatures (fuzzy_gating_fusion.py:392-419), whatever the mode
    const float Ti = softplus_f(prm[0]) + eps_temp, Te = softplus_f(prm[1]) + eps_temp;
    const float reg = fmaxf(Ti - t_max, 0.f) + fmaxf(t_min - Ti, 0.f) + fmaxf(Te - t_max, 0.f) + fmaxf(t_min - Te, 0.f);
    auto sig = [](float x) { return 1.0f / (1.0f + expf(-x)); };
    dtau[0] = l_reg * scale * ((Ti > t_max ? 1.f : 0.f) - (Ti < t_min ? 1.f : 0.f)) * sig(prm[0]);
    dtau[1] = l_reg * scale * ((Te > t_max ? 1.f : 0.f) - (Te < t_min ? 1.f : 0.f)) * sig(prm[1]);
    losses[1] = tot[0]; losses[2] = tot[1]; losses[3] = tot[2]; losses[4] = reg;
    losses[0] = tot[0] + l_img * tot[1] + l_eeg * tot[2] + l_reg * reg;
  }
}

extern "C" int eg_fusion_loop_loss(const float* fused, const float* z_img, const float* z_eeg, const int64_t* labels,
                                   const float* params, float* losses, float* dfused, float* daux_img, float* daux_eeg,
                                   float* dtau, int B, int K, int mode, float eps_temp, float lambda_aux_img,
                                   float lambda_aux_eeg, float lambda_reg, float t_min, float t_max, const eg_step_state* state,
                                   void* stream) {
  EG_CHECK(fused && z_img && z_eeg && labels && params && losses && dfused && daux_img && daux_eeg && dtau,
           "eg_fusion_loop_loss: null pointer");
  EG_CHECK(B > 0 && K > 1 && K <= 16 && mode >= 0 && mode <= 3, "eg_fusion_loop_loss: bad shape / mode");
  hipLaunchKernelGGL(fusion_loop_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, fused, z_img, z_eeg,
                     (const long long*)labels, params, losses, dfused, daux_img, daux_eeg, dtau, B, K, mode, eps_temp,
                     lambda_aux_img, lambda_aux_eeg, lambda_reg, t_min, t_max, state);
  EG_LAUNCH_CHECK("fusion_loop_loss");
  return 0;
}

extern "C" int eg_fuzzy_gate_bwd(const float* z_img, const float* z_eeg, const float* params, const float* dfused,
                                 const float* dalpha, float* dz_img, float* dz_eeg, float* partial, int B, int K, int mode,
                                 float eps_temp, float eps_log, float eps_div, void* stream) {
  EG_CHECK(z_img && z_eeg && params && dfused && dz_img && dz_eeg && partial, "eg_fuzzy_gate_bwd: null pointer");
  EG_CHECK(B > 0 && K > 1 && K <= 16 && mode >= 0 && mode <= 3, "eg_fuzzy_gate_bwd: bad shape / mode");
  hipLaunchKernelGGL(fuzzy_gate_bwd_kernel, dim3((B + 127) / 128), dim3(128), 0, (hipStream_t)stream, z_img, z_eeg, params,
                     dfused, dalpha, dz_img, dz_eeg, partial, B, K, mode, eps_temp, eps_log, eps_div);
  EG_LAUNCH_CHECK("fuzzy_gate_bwd");
  return 0;
}

extern "C" int eg_fuzzy_gate_fwd(const float* z_img, const float* z_eeg, const float* params, float* fused, float* alpha,
                                 int B, int K, int mode, float eps_temp, float eps_log, float eps_div, void* stream) {
  EG_CHECK(z_img && z_eeg && params && fused && alpha, "eg_fuzzy_gate_fwd: null pointer");
  EG_CHECK(B > 0 && K > 1 && K <= 16 && mode >= 0 && mode <= 3, "eg_fuzzy_gate_fwd: bad shape / mode");
  hipLaunchKernelGGL(fuzzy_gate_fwd_kernel, dim3((B + 127) / 128), dim3(128), 0, (hipStream_t)stream, z_img, z_eeg, params,
                     fused, alpha, B, K, mode, eps_temp, eps_log, eps_div);
  EG_LAUNCH_CHECK("fuzzy_gate_fwd");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Evaluation tail of one batch on the device (T:258-314 per batch: argmax, confusion matrix, loss sum), so that an evaluation loop
// syncs the host once at its end instead of twice per batch.  One workgroup: B is a few thousand rows at the most and ncls <= 16.
// The batch's histogram is built in LDS (LDS atomics) and added to the running matrix with plain loads and stores: launches on one
// stream are ordered, so the read-modify-write of confusion / loss_sum needs no global atomic.
// ---------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void eval_accumulate_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                              const float* __restrict__ loss, int* __restrict__ pred,
                                                              int* __restrict__ confusion, float* __restrict__ loss_sum, int B, int ncls) {
  __shared__ int hist[16 * 16];
  const int tid = threadIdx.x;
  hist[tid] = 0;
  __syncthreads();
  for (int b = tid; b < B; b += 256) {
    const float* row = logits + (size_t)b * ncls;
    float best = row[0];
    int arg = 0;
    for (int c = 1; c < ncls; ++c) {
      const float v = row[c];
      if (v > best) { best = v; arg = c; }         // strict: the lowest index wins a tie
    }
    pred[b] = arg;
    if (confusion) {
      const long long y = labels[b];
      if (y >= 0 && y < ncls) atomicAdd(&hist[(int)y * ncls + arg], 1);      // (a label outside the classes counts nowhere)
    }
  }
  __syncthreads();
  if (confusion && tid < ncls * ncls) confusion[tid] += hist[tid];
  if (tid == 0 && loss && loss_sum) *loss_sum += *loss;
}
}  // namespace

extern "C" int eg_eval_accumulate(const float* logits, const int64_t* labels, const float* loss, int32_t* pred, int32_t* confusion,
                                  float* loss_sum, int B, int ncls, void* stream) {
  EG_CHECK(ncls >= 1 && ncls <= 16, "eg_eval_accumulate: ncls=%d outside [1, 16]", ncls);
  EG_CHECK(B > 0, "eg_eval_accumulate: B=%d", B);
  EG_CHECK(logits && pred, "eg_eval_accumulate: null logits or pred");
  EG_CHECK(!confusion || labels, "eg_eval_accumulate: a confusion matrix needs labels");
  hipLaunchKernelGGL(eval_accumulate_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, (const long long*)labels, loss, pred,
                     confusion, loss_sum, B, ncls);
  EG_LAUNCH_CHECK("eval_accumulate");
  return 0;
}
