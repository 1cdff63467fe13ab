// Statistics of the attention probabilities of one stage, for the cross-attention analysis (5_Metrics/eeg_metrics.py:465-594), computed
// from the stage's q|k|v rows and lse without ever storing P[w, h, q, k] = exp(q.k / sqrt(DK) - lse[w, h, q]):
//   diag[b, q]     = 1/(2H) sum_h (P[b, h, q, q] + P[b + NB/2, h, q, q])          per sample, written
//   map_sum[q, k] += sum_b 1/(2H) sum_h (P[b, h, q, k] + P[b + NB/2, h, q, k])    over the batch, read-modify-written
// Sample b < NB/2 owns windows b and b + NB/2; layouts and the kv_shift pairing are those of attention_long.hip.
//
// Ownership: one workgroup per (64-query tile, 64-key tile, sample split p).  It walks samples [p chunk, (p + 1) chunk) in ascending
// b, per sample the two windows, per window the heads, and adds every (window, head) pair's 64 x 64 probabilities into ONE register
// tile that lives for the whole walk.  A sample's 2 H pairs are never split across workgroups, so the workgroups with
// query tile == key tile each own their samples' diag rows outright.  P == 1 (the tiles alone fill the GPU): the workgroup adds its
// tile, scaled by 1/(2H), into map_sum itself.  P > 1: it stores the unscaled tile to scratch[p], and a second launch adds the P
// partials in ascending p, scales, and adds into map_sum.  Every sum has a fixed order and one writer: no atomics, two runs agree
// bit for bit.  Rows / keys >= S of a ragged tile are masked to zero and never stored.  All offsets are 64 bit.
//
// 16-bit: four waves of 16 queries x 64 keys.  The pair's K tile goes through LDS as attnhead.h's head image (a 64-wide head: two
// images, one behind the other), double-buffered, the next pair's global loads (K chunks, the lane's Q fragment, its lse) issued before
// this pair's MFMAs; scores^T = K Q^T as DK / 32 chained v_mfma_f32_16x16x32_{bf16,f16} per 16 x 16 tile (key on rows, query on lanes),
// so lane (l15, g) of wave w holds query 16 w + l15, keys 16 kt + 4 g + r in s[kt][r].
// fp32: a thread per (query, 16 keys), hd_dot<DK> and expf -- the arithmetic of attn_long_probs_kernel element for element.
#include "attnhead.h"

namespace {

constexpr int LT = 64;                    // queries and keys of a tile
constexpr int IMG = LT * 64;              // bytes of one 64-row image of a 32-wide 16-bit half of a head slice
constexpr int TILE = LT * LT;             // floats of a partial tile in scratch, [query][key]
constexpr int FILL = 512;                 // workgroups the sample split aims at most at: about twice the MI355X's 256 CUs

// host: the launch shape, a function of (NB, S) alone -- never of the device -- so the scratch size is a host-only number and the
// order of every sum is fixed by the shapes
struct StatsPlan { int nt, tiles, chunk, P; };
inline StatsPlan stats_plan(int NB, int S) {
  StatsPlan pl;
  pl.nt = (S + LT - 1) / LT;
  pl.tiles = pl.nt * pl.nt;
  const int nsamp = NB / 2;
  const int fit = FILL / pl.tiles;
  const int pmax = pl.tiles >= FILL / 2 ? 1 : nsamp < fit ? nsamp : fit;
  pl.chunk = (nsamp + pmax - 1) / pmax;
  pl.P = (nsamp + pl.chunk - 1) / pl.chunk;       // no empty split
  return pl;
}

struct Walk {                             // what both kernels derive from blockIdx
  int tile, p, q0, k0, b0, npair;
};
__device__ __forceinline__ Walk stats_walk(int NB, int H, int nt, int chunk) {
  Walk w;
  w.tile = blockIdx.x % (nt * nt);
  w.p = blockIdx.x / (nt * nt);
  w.q0 = (w.tile / nt) * LT;
  w.k0 = (w.tile % nt) * LT;
  w.b0 = w.p * chunk;
  w.npair = (min(NB / 2, w.b0 + chunk) - w.b0) * 2 * H;
  return w;
}
// pair i of the walk: sample b0 + i / 2H, its window i / H % 2 (b, then b + NB/2), head i % H
struct Pair { int b, w, h; };
__device__ __forceinline__ Pair stats_pair(int i, int b0, int NB, int H) {
  const int bi = i / (2 * H), r = i - bi * 2 * H, wi = r / H;
  return {b0 + bi, b0 + bi + wi * (NB / 2), r - wi * H};
}

// ------------------------------------------------------------------------------------------------
// 16-bit
// ------------------------------------------------------------------------------------------------
template <typename T, int DK>
__global__ __launch_bounds__(256) void attn_stats_kernel(const T* __restrict__ qkv, const float* __restrict__ lse,
                                                         float* __restrict__ map_sum, float* __restrict__ diag,
                                                         float* __restrict__ scratch, int NB, int S, int H, int kv_shift, int nt,
                                                         int chunk, int P) {
  constexpr int NH = DK / 32;
  constexpr float SCALE = hd_scale<DK>();
  __shared__ __attribute__((aligned(16))) char sm[2][NH * IMG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
  const Walk wk = stats_walk(NB, H, nt, chunk);
  const int D = H * DK;
  const long long ld = 3ll * D;
  const int q = wk.q0 + wave * 16 + l15;
  const bool qok = q < S;
  const int klim = qok ? S - wk.k0 - 4 * g : 0;          // key 16 kt + r of this lane's column block is real iff 16 kt + r < klim
  const bool on_diag = wk.q0 == wk.k0;                   // workgroup-uniform
  const bool diag_lane = g == (l15 >> 2);                // this lane's s[wave][l15 & 3] is P[q, q]

  // a pair's global loads: this thread's 16-B chunk of each half of the K tile (row tid >> 2, chunk tid & 3), the lane's Q fragments, its lse
  u32x4 rk[NH];
  FR<T> qn[NH];
  float ln;
  auto request = [&](int i) {
    const Pair pr = stats_pair(i, wk.b0, NB, H);
    const int bk = (pr.w + kv_shift) % NB;
    const T* kbase = qkv + (long long)bk * S * ld + D + pr.h * DK;
    const T* qrow = qkv + ((long long)pr.w * S + q) * ld + pr.h * DK;
    const int krow = wk.k0 + (tid >> 2);
#pragma unroll
    for (int hf = 0; hf < NH; ++hf) {
      rk[hf] = (u32x4){0u, 0u, 0u, 0u};
      if (krow < S) rk[hf] = *(const u32x4*)(kbase + (long long)krow * ld + 32 * hf + (tid & 3) * 8);
      qn[hf] = hd_frag_global<T>(qrow + 32 * hf + g * 8, qok);
    }
    ln = qok ? lse[((long long)pr.w * H + pr.h) * S + q] : 0.f;
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int hf = 0; hf < NH; ++hf) *(u32x4*)(sm[buf] + hf * IMG + hd_img_off(tid >> 2, tid & 3)) = rk[hf];
  };

  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[4] = {zero4, zero4, zero4, zero4};
  float dsum = 0.f;
  const float inv = 0.5f / (float)H;
  FR<T> qf[NH];
  float lq;
  request(0);
  stage(0);
#pragma unroll
  for (int hf = 0; hf < NH; ++hf) qf[hf] = qn[hf];
  lq = ln;
  __syncthreads();
  for (int i = 0; i < wk.npair; ++i) {
    const int cur = i & 1;
    const bool more = i + 1 < wk.npair;
    if (more) request(i + 1);
    const char* kimg = sm[cur];
    f32x4 pr4[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      f32x4 s = zero4;
#pragma unroll
      for (int hf = 0; hf < NH; ++hf) s = H16<T>::mfma(hd_frag_row<T>(kimg + hf * IMG, kt * 16 + l15, g), qf[hf], s);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv = kt * 16 + r < klim ? __expf(s[r] * SCALE - lq) : 0.f;
        pr4[kt][r] = pv;
        acc[kt][r] += pv;
      }
    }
    if (on_diag) {
      const f32x4 d4 = wave == 0 ? pr4[0] : wave == 1 ? pr4[1] : wave == 2 ? pr4[2] : pr4[3];
      const int r = l15 & 3;
      dsum += r == 0 ? d4[0] : r == 1 ? d4[1] : r == 2 ? d4[2] : d4[3];
      if ((i + 1) % (2 * H) == 0) {                      // the sample's last pair: its diag row has this one writer
        const int b = wk.b0 + i / (2 * H);
        if (diag_lane && qok) diag[(long long)b * S + q] = dsum * inv;
        dsum = 0.f;
      }
    }
    if (more) {
      stage(cur ^ 1);
#pragma unroll
      for (int hf = 0; hf < NH; ++hf) qf[hf] = qn[hf];
      lq = ln;
    }
    __syncthreads();
  }
  if (P == 1) {
    if (qok) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (kt * 16 + r < klim) map_sum[(long long)q * S + wk.k0 + kt * 16 + 4 * g + r] += acc[kt][r] * inv;
    }
  } else {
    float* out = scratch + ((long long)wk.p * (nt * nt) + wk.tile) * TILE + (wave * 16 + l15) * LT + 4 * g;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[kt * 16 + r] = acc[kt][r];
  }
}

// ------------------------------------------------------------------------------------------------
// fp32: thread (ql = tid & 63, kg = tid >> 6) owns query q0 + ql and keys k0 + 16 kg .. + 15; the K tile in LDS, read as a broadcast
// ------------------------------------------------------------------------------------------------
template <int DK>
__global__ __launch_bounds__(256) void attn_stats_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ lse,
                                                             float* __restrict__ map_sum, float* __restrict__ diag,
                                                             float* __restrict__ scratch, int NB, int S, int H, int kv_shift, int nt,
                                                             int chunk, int P) {
  constexpr float SCALE = hd_scale<DK>();
  __shared__ __attribute__((aligned(16))) float Kl[LT * DK];
  const int tid = threadIdx.x, ql = tid & 63, kg = tid >> 6;
  const Walk wk = stats_walk(NB, H, nt, chunk);
  const int D = H * DK;
  const long long ld = 3ll * D;
  const int q = wk.q0 + ql;
  const bool qok = q < S;
  const int klim = qok ? S - wk.k0 - 16 * kg : 0;        // key j of this thread's block is real iff j < klim
  const bool diag_thread = wk.q0 == wk.k0 && kg == (ql >> 4);
  float acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.f;
  float dsum = 0.f;
  const float inv = 0.5f / (float)H;
  for (int i = 0; i < wk.npair; ++i) {
    const Pair pr = stats_pair(i, wk.b0, NB, H);
    const int bk = (pr.w + kv_shift) % NB;
    const float* kbase = qkv + (long long)bk * S * ld + D + pr.h * DK;
    __syncthreads();
    for (int e = tid; e < LT * (DK / 4); e += 256) {
      const int r = e / (DK / 4), c = e % (DK / 4);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (wk.k0 + r < S) v = *(const f32x4*)(kbase + (long long)(wk.k0 + r) * ld + 4 * c);
      *(f32x4*)(Kl + r * DK + 4 * c) = v;
    }
    float qv[DK];
#pragma unroll
    for (int d = 0; d < DK; ++d) qv[d] = qok ? qkv[((long long)pr.w * S + q) * ld + pr.h * DK + d] : 0.f;
    const float lq = qok ? lse[((long long)pr.w * H + pr.h) * S + q] : 0.f;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float pv = j < klim ? expf(hd_dot<DK>(qv, Kl + (16 * kg + j) * DK) * SCALE - lq) : 0.f;
      acc[j] += pv;
      if (diag_thread && j == (ql & 15)) dsum += pv;
    }
    if (diag_thread && (i + 1) % (2 * H) == 0) {
      if (qok) diag[(long long)pr.b * S + q] = dsum * inv;
      dsum = 0.f;
    }
  }
  if (P == 1) {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j < klim) map_sum[(long long)q * S + wk.k0 + 16 * kg + j] += acc[j] * inv;
  } else {
    float* out = scratch + ((long long)wk.p * (nt * nt) + wk.tile) * TILE + ql * LT + 16 * kg;
#pragma unroll
    for (int j = 0; j < 16; ++j) out[j] = acc[j];
  }
}

// map_sum += 1/(2H) * (the P partial tiles, added in ascending p); a thread per tile element, elements outside [S, S] skipped.
// Workgroups of one wave, so that the few tiles of a short window still spread over the CUs; the loads of eight partials are in
// flight together, the additions stay in order.
constexpr int RED_THREADS = 64;
__global__ __launch_bounds__(RED_THREADS) void attn_stats_reduce_kernel(const float* __restrict__ scratch, float* __restrict__ map_sum,
                                                                        int S, int H, int nt, int P) {
  const long long n = (long long)nt * nt * TILE;
  const long long e = (long long)blockIdx.x * RED_THREADS + threadIdx.x;
  if (e >= n) return;
  const int tile = (int)(e / TILE), ql = (int)(e % TILE) / LT, kl = (int)(e % LT);
  const int q = (tile / nt) * LT + ql, k = (tile % nt) * LT + kl;
  if (q >= S || k >= S) return;
  float s = 0.f;
#pragma unroll 8
  for (int p = 0; p < P; ++p) s += scratch[(long long)p * n + e];
  map_sum[(long long)q * S + k] += s * (0.5f / (float)H);
}

int stats_check(const char* who, int NB, int S, int H, int head_dim, int kv_shift, int dtype) {
  if (hd_check(who, NB, S, H, kv_shift, dtype, 0.f, nullptr, EG_ATTN_LONG_MAX_S, false)) return 1;
  EG_CHECK((NB & 1) == 0, "%s: NB=%d must be even (sample b owns windows b and b + NB/2)", who, NB);
  EG_CHECK(head_dim == 32 || head_dim == 64, "%s: head_dim=%d: the kernels are built for head widths 32 and 64", who, head_dim);
  return 0;
}

}  // namespace

extern "C" int64_t eg_attention_stats_scratch_elems(int NB, int S, int H) {
  if (NB < 2 || (NB & 1) || S < 1 || S > EG_ATTN_LONG_MAX_S || H < 1) return -1;
  const StatsPlan pl = stats_plan(NB, S);
  return pl.P == 1 ? 0 : (int64_t)pl.P * pl.tiles * TILE;
}

extern "C" int eg_attention_stats(const void* qkv, const float* lse, float* map_sum, float* diag, float* scratch, int64_t scratch_elems,
                                  int NB, int S, int H, int head_dim, int kv_shift, int dtype, void* stream) {
  const char* who = "eg_attention_stats";
  if (stats_check(who, NB, S, H, head_dim, kv_shift, dtype)) return 1;
  const StatsPlan pl = stats_plan(NB, S);
  const long long need = pl.P == 1 ? 0 : (long long)pl.P * pl.tiles * TILE;
  EG_CHECK(qkv && lse && map_sum && diag && (scratch || need == 0), "%s: null pointer", who);
  EG_CHECK(scratch_elems >= need, "%s: scratch holds %lld floats, %lld are needed", who, (long long)scratch_elems, need);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(pl.P * pl.tiles), block(256);
  auto launch = [&](auto dk) {
    constexpr int DK = decltype(dk)::value;
    if (dtype == EG_F32)
      hipLaunchKernelGGL(attn_stats_f32_kernel<DK>, grid, block, 0, s, (const float*)qkv, lse, map_sum, diag, scratch, NB, S, H, kv_shift,
                         pl.nt, pl.chunk, pl.P);
    else
      eg_dispatch_16(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((attn_stats_kernel<T, DK>), grid, block, 0, s, (const T*)qkv, lse, map_sum, diag, scratch, NB, S, H, kv_shift,
                           pl.nt, pl.chunk, pl.P);
      });
  };
  if (head_dim == 64) launch(eg_int<64>{});
  else launch(eg_int<32>{});
  if (pl.P > 1)
    hipLaunchKernelGGL(attn_stats_reduce_kernel, dim3(pl.tiles * (TILE / RED_THREADS)), dim3(RED_THREADS), 0, s, (const float*)scratch, map_sum, S, H,
                       pl.nt, pl.P);
  EG_LAUNCH_CHECK(who + 3);
  return 0;
}
