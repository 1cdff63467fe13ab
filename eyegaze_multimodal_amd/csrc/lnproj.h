// Steps 2-4 of the LayerNorm-backward + backward-data launch (lnproj.hip's header comment), written once for its two callers:
//   * ln_bwd_proj_kernel (lnproj.hip): dy and x arrive as two resident tiles by LDS-DMA;
//   * the backward instantiation of ffn_chain_kernel with its norm-1 tail (ffn.hip): the dy rows are the rows that epilogue 2 has
//     just rounded into the resident tile, x comes straight into registers in the half-wave layout (XREG).
// Device code only, in the manner of rowtile.h: every helper takes the lane constants as arguments.  A half-wave hw = tid / 32
// (0 .. 7) owns rows hw, hw + 8, .. (10 rows) of the 80-row tile, its lane l = lane % 32 the row's 16-B piece l.
#pragma once
#include "rowtile.h"

constexpr int LP_ROWS_PER_HW = RT_ROWS / 8;   // 10
constexpr int LP_SUMS_B = 8 * 2 * 256 * 4;    // 16,384 B: [half-wave][dg | db][256] fp32 in front of the epilogue images

template <typename T>
struct LnProjArgs {
  const T* dy; const T* x; const float* stats; const float* gamma; const T* Wf;
  T* dr; T* dyo; T* dC; float* partial;
  const eg_step_state* st;
  int M;
  DropCfg d1, d2;
};

// host: the descriptor's own checks, shared by eg_ln_bwd_proj (dy required) and eg_ffn_bwd_ln_proj (dy comes from the launch itself)
static inline int lp_check_desc(const eg_ln_bwd_proj_desc* d, const char* who, bool need_dy) {
  EG_CHECK(d && (d->dy || !need_dy) && d->x && d->stats && d->gamma && d->W_frag && d->dx && d->dx_drop && d->dC && d->partial,
           "%s: null operand", who);
  EG_CHECK(d->dtype == EG_BF16 || d->dtype == EG_F16, "%s: 16-bit compute dtypes only (got %d)", who, d->dtype);
  EG_CHECK(d->M > 0 && d->d_model == RT_COLS, "%s: M=%d, d_model=%d (256 only)", who, d->M, d->d_model);
  EG_CHECK(d->partial_capacity_blocks >= eg_ln_bwd_proj_blocks(d->M),
           "%s: the partial buffer holds %d rows, the launch writes %d", who, d->partial_capacity_blocks, eg_ln_bwd_proj_blocks(d->M));
  EG_CHECK((long long)d->M * RT_COLS < (1ll << 32), "%s: M*D exceeds the 32-bit dropout index", who);
  EG_CHECK(d->drop1_p >= 0.f && d->drop1_p < 1.f && d->drop2_p >= 0.f && d->drop2_p < 1.f, "%s: dropout p", who);
  EG_CHECK((d->drop1_p == 0.f && d->drop2_p == 0.f) || d->state, "%s: dropout needs a step state", who);
  EG_CHECK(((uintptr_t)d->dy | (uintptr_t)d->x | (uintptr_t)d->W_frag | (uintptr_t)d->dx | (uintptr_t)d->dx_drop | (uintptr_t)d->dC) % 16 == 0,
           "%s: operands must be 16-B aligned", who);
  return 0;
}
template <typename T>
static inline LnProjArgs<T> lp_make_args(const eg_ln_bwd_proj_desc* d) {
  LnProjArgs<T> p;
  p.dy = (const T*)d->dy; p.x = (const T*)d->x; p.stats = d->stats; p.gamma = d->gamma; p.Wf = (const T*)d->W_frag;
  p.dr = (T*)d->dx; p.dyo = (T*)d->dx_drop; p.dC = (T*)d->dC; p.partial = d->partial; p.st = d->state; p.M = d->M;
  p.d1 = make_drop(d->drop1_p, d->drop1_site);
  p.d2 = make_drop(d->drop2_p, d->drop2_site);
  return p;
}

// the four W fragments of k-step s = 0 .. 7 (chunk s / 4, step s % 4 of rt_frag_elem<4, 4>); wu = this wave's part, wl = 16 lane
template <typename T>
__device__ __forceinline__ void lp_req_w(const char* wu, uint32_t wl, int s, typename H16<T>::frag (&w)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = *(const typename H16<T>::frag*)(wu + rt_frag_elem<4, 4>(s >> 2, 0, s & 3, j) * 2 + wl);
}

// mean and rstd of the half-wave's 10 rows (zero beyond M)
__device__ __forceinline__ void lp_stats(const float* stats, int M, int m0, int hw, float (&mean)[LP_ROWS_PER_HW],
                                         float (&rstd)[LP_ROWS_PER_HW]) {
#pragma unroll
  for (int j = 0; j < LP_ROWS_PER_HW; ++j) {
    const int m = m0 + hw + 8 * j;
    mean[j] = 0.f; rstd[j] = 0.f;
    if (m < M) { mean[j] = stats[2 * (size_t)m]; rstd[j] = stats[2 * (size_t)m + 1]; }
  }
}

// ---- 2. LayerNorm backward, a half-wave per row (layernorm_bwd256_kernel's arithmetic): dr and dyo leave as 512-B rows, dyo also
//         replaces the dy piece of tile ty in place.  x: XREG ? the lane's pieces xr[j] : tile tx ----
template <typename T, bool XREG>
__device__ __forceinline__ void lp_ln_rows(const LnProjArgs<T> p, char* ty, const char* tx, const u32x4 (&xr)[XREG ? LP_ROWS_PER_HW : 1],
                                           int m0, int hw, int l, const float (&g)[8], const float (&mean)[LP_ROWS_PER_HW],
                                           const float (&rstd)[LP_ROWS_PER_HW], bool drop, uint32_t seed_lo, uint32_t seed_hi,
                                           float (&dg)[8], float (&db)[8]) {
#pragma unroll
  for (int j = 0; j < LP_ROWS_PER_HW; ++j) {
    const int r = hw + 8 * j;
    const int m = m0 + r;
    const bool ok = m < p.M;
    char* const py = ty + r * RT_ROWB + rt_piece(r, l);
    float xv[8], dv[8];
    if constexpr (XREG) load8((const T*)&xr[j], xv);
    else load8((const T*)(tx + r * RT_ROWB + rt_piece(r, l)), xv);
    load8((const T*)py, dv);
    if (!ok) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { xv[e] = 0.f; dv[e] = 0.f; }
    }
    float o[8];
    eg_ln_bwd_row8(xv, dv, g, mean[j], rstd[j], dg, db, o);
    if (!ok) {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = 0.f;
    }
    if (ok) store8(p.dr + (size_t)m * RT_COLS + l * 8, o);
    if (drop && ok) {
      const uint32_t idx = (uint32_t)m * 256u + (uint32_t)(l * 8);
      eg_dropout_run<8>(o, p.d1, seed_lo, seed_hi, idx);
      eg_dropout_run<8>(o, p.d2, seed_lo, seed_hi, idx);
    }
    if (ok) store8(p.dyo + (size_t)m * RT_COLS + l * 8, o);
    store8((T*)py, o);                             // (zeros for rows beyond M) the piece becomes part of the A operand
  }
}

// gain / bias sums of the tile: [half-wave][dg | db][256] through LDS (red: LP_SUMS_B bytes that nobody else uses until the launch
// ends), then one sum per column into partial[blockIdx.x][512].  Holds one barrier.
__device__ __forceinline__ void lp_sums(float* partial, float* red, const float (&dg)[8], const float (&db)[8], int tid, int hw, int l) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[(hw * 2 + 0) * 256 + l * 8 + e] = dg[e];
    red[(hw * 2 + 1) * 256 + l * 8 + e] = db[e];
  }
  __syncthreads();
  for (int i = tid; i < 512; i += 256) {
    const int which = i >> 8, n = i & 255;
    float s = 0.f;
#pragma unroll
    for (int h = 0; h < 8; ++h) s += red[(h * 2 + which) * 256 + n];
    partial[(size_t)blockIdx.x * 512 + i] = s;
  }
}

// ---- 3. dC = dyo * W^T over K = 256: a wave owns 80 x 64, fragments two k-steps ahead (wr holds k-steps 0 and 1 on entry);
// ---- 4. epilogue: per 16-row tile through the wave-private fp32 image timg ----
template <typename T>
__device__ __forceinline__ void lp_product(T* dC, int M, const char* ty, typename H16<T>::frag (&wr)[2][4], const char* wu, uint32_t wl,
                                           float* timg, int m0, int lane, int wn) {
  typedef typename H16<T>::frag frag;
  const int l15 = lane & 15, g4 = lane >> 4;
  f32x4 acc[5][4];
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int sw7 = rt_swz(l15);
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    frag xf[5];
    rt_frags<T>(ty, l15, g4, sw7, s, xf);
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = H16<T>::mfma(wr[s & 1][j], xf[i], acc[i][j]);
    if (s + 2 < 8) lp_req_w<T>(wu, wl, s + 2, wr[s & 1]);
  }
  const int er = lane >> 2, ec = lane & 3;
  const int n = 64 * wn + 16 * ec;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int m = m0 + 16 * i + er;
    rt_image_put(timg, acc[i], lane);
    if (m0 + 16 * i >= M) break;                   // workgroup-uniform: tiles wholly beyond M
    float v[16];
    rt_image_get(timg, lane, v);
    if (m < M) rt_store16(dC + (size_t)m * RT_COLS + n, v);
  }
}
