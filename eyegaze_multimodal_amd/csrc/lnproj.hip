// LayerNorm backward + the backward-data product that consumes it, in ONE launch over 80-row tiles (d_model = 256):
//   dr   = LayerNormBackward(dy; x, mean, rstd, gamma)          (A:293 backward: gradient of the pre-norm sum, the residual path's)
//   dyo  = dropout(dr)                                         (the branch dropout of A:292: what flows into out_proj's backward)
//   dC   = dyo * W[256, 256]^T                                 (A:213 backward: grad_input of out_proj, W in fragment order)
//   partial[workgroup][0:256 | 256:512] = this tile's sums of dy * xhat | dy  (gain / bias gradients, reduced by eg_reduce_*)
// As two launches (eg_layernorm_bwd, eg_gemm_nt) the masked rows are written, read back by the product's A-operand DMA, and each launch
// pays its own ramp: 16 + 14 us per layer at the benchmark size.  Here the LayerNorm arithmetic FILLS the resident A tile of an
// eg_ffn_chain-style product (weights as MFMA fragments straight from L2, no streamed operand -- so no HBM-latency DMA sits in front of
// the fragment loads in the waves' in-order vmcnt queues, the reason the streamed form of this tile was dropped).
//
// One 256-thread workgroup per 80 rows, two per CU (80 KB of LDS):
//   1. LDS-DMA: dy rows -> tile Y, x rows -> tile X (two resident tiles of rowtile.h, where the DMA map, the swizzle, the fragment
//      order and the image epilogue of steps 3 and 4 are written down);
//   2. a half-wave per row (32 lanes x 8 elements), rows hw, hw + 8, ..: EXACTLY layernorm_bwd256_kernel's arithmetic and reduction
//      order (dr and dyo are bit-identical to eg_layernorm_bwd's); dr and dyo leave as 512-B rows, dyo also replaces the dy piece in
//      tile Y in place -- tile Y becomes the product's A operand;
//   3. dC: a wave owns 80 x 64 (5 x 4 accumulator tiles), K = 256 in 8 k-steps, weight fragments two k-steps ahead (eg_pack_table
//      modes 5 / 6: rt_frag_elem<4, 4>); same k-ordered MFMA chains as eg_gemm_nt: dC is bit-identical to it;
//   4. epilogue through the wave-private fp32 image (in tile X, free by then): 16-bit stores of dC.
#include "rowtile.h"

namespace {

constexpr int PR = RT_ROWS;
constexpr int PD = RT_COLS;
constexpr int P_T = RT_TILEB;                 // 40,960 B per tile
constexpr int P_LDS = 2 * P_T;                // 81,920 B

template <typename T>
struct LnProjArgs {
  const T* dy; const T* x; const float* stats; const float* gamma; const T* Wf;
  T* dr; T* dyo; T* dC; float* partial;
  const eg_step_state* st;
  int M;
  DropCfg d1, d2;
};

template <typename T>
__global__ __launch_bounds__(256, 2) void ln_bwd_proj_kernel(LnProjArgs<T> p) {
  typedef typename H16<T>::frag frag;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const ty = smem;                       // dy rows, then dyo rows: the product's A operand
  char* const tx = smem + P_T;                 // x rows; later the gain / bias sums and the epilogue image
  const int tid = threadIdx.x, lane = tid & 63;
  const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g4 = lane >> 4;
  const int m0 = blockIdx.x * PR;

  // ---- 1. both tiles by LDS-DMA, their instructions interleaved (rows beyond M repeat row M - 1) ----
#pragma unroll
  for (int i = 0; i < RT_DMA_PER_WAVE; ++i) {
    const size_t row = (size_t)min(m0 + rt_dma_row(wn, lane, i), p.M - 1);
    rt_dma_issue((const char*)(p.dy + row * PD), ty, wn, lane, i);
    rt_dma_issue((const char*)(p.x + row * PD), tx, wn, lane, i);
  }
  // weight fragments of the first two k-steps and this half-wave's statistics travel meanwhile
  const char* const wu = (const char*)(p.Wf + rt_frag_elem<4, 4>(0, wn, 0, 0));
  const uint32_t wl = (uint32_t)lane * 16u;
  frag wr[2][4];
  auto req_w = [&](int s, int slot) {            // k-step s = 0 .. 7: chunk s / 4, step s % 4
#pragma unroll
    for (int j = 0; j < 4; ++j)
      wr[slot][j] = *(const frag*)(wu + rt_frag_elem<4, 4>(s >> 2, 0, s & 3, j) * 2 + wl);
  };
  const int l = lane & 31, hw = tid >> 5;        // half-wave hw = 0 .. 7 owns rows hw, hw + 8, .. (10 rows)
  float mean[10], rstd[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) {
    const int m = m0 + hw + 8 * j;
    mean[j] = 0.f; rstd[j] = 0.f;
    if (m < p.M) { mean[j] = p.stats[2 * (size_t)m]; rstd[j] = p.stats[2 * (size_t)m + 1]; }
  }
  float g[8], dg[8], db[8];
  load8(p.gamma + l * 8, g);
#pragma unroll
  for (int e = 0; e < 8; ++e) { dg[e] = 0.f; db[e] = 0.f; }
  uint32_t seed_lo = 0, seed_hi = 0;
  const bool drop = (p.d1.thresh | p.d2.thresh) != 0;
  if (drop) { seed_lo = p.st->seed_lo; seed_hi = p.st->seed_hi; }
  req_w(0, 0);
  req_w(1, 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- 2. LayerNorm backward, a half-wave per row (layernorm_bwd256_kernel's arithmetic) ----
#pragma unroll
  for (int j = 0; j < 10; ++j) {
    const int r = hw + 8 * j;
    const int m = m0 + r;
    const bool ok = m < p.M;
    char* const py = ty + r * RT_ROWB + rt_piece(r, l);
    const char* const px = tx + r * RT_ROWB + rt_piece(r, l);
    float xv[8], dv[8];
    load8((const T*)px, xv);
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
    if (ok) store8(p.dr + (size_t)m * PD + l * 8, o);
    if (drop && ok) {
      const uint32_t idx = (uint32_t)m * 256u + (uint32_t)(l * 8);
      eg_dropout_run<8>(o, p.d1, seed_lo, seed_hi, idx);
      eg_dropout_run<8>(o, p.d2, seed_lo, seed_hi, idx);
    }
    if (ok) store8(p.dyo + (size_t)m * PD + l * 8, o);
    store8((T*)py, o);                           // (zeros for rows beyond M) the piece becomes part of the A operand
  }
  __syncthreads();                               // tile Y = dyo complete; tile X is free

  // gain / bias sums of the tile: [half-wave][dg | db][256] through LDS (tile X), then one sum per column
  {
    float* red = (float*)tx;                     // [8][2][256]
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
      p.partial[(size_t)blockIdx.x * 512 + i] = s;
    }
  }

  // ---- 3. dC = dyo * W^T over K = 256 ----
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
    if (s + 2 < 8) req_w(s + 2, s & 1);
  }

  // ---- 4. epilogue: per 16-row tile through the wave-private fp32 image (tile X, behind the 16 KB of sums) ----
  float* timg = (float*)(tx + 16384 + wn * RT_IMGB);
  const int er = lane >> 2, ec = lane & 3;
  const int n = 64 * wn + 16 * ec;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int m = m0 + 16 * i + er;
    rt_image_put(timg, acc[i], lane);
    if (m0 + 16 * i >= p.M) break;                 // workgroup-uniform: tiles wholly beyond M
    float v[16];
    rt_image_get(timg, lane, v);
    if (m < p.M) rt_store16(p.dC + (size_t)m * PD + n, v);
  }
}

template <typename T>
static int lnproj_launch(const eg_ln_bwd_proj_desc* d, hipStream_t s) {
  LnProjArgs<T> p;
  p.dy = (const T*)d->dy; p.x = (const T*)d->x; p.stats = d->stats; p.gamma = d->gamma; p.Wf = (const T*)d->W_frag;
  p.dr = (T*)d->dx; p.dyo = (T*)d->dx_drop; p.dC = (T*)d->dC; p.partial = d->partial; p.st = d->state; p.M = d->M;
  p.d1 = make_drop(d->drop1_p, d->drop1_site);
  p.d2 = make_drop(d->drop2_p, d->drop2_site);
  eg_launch_lds<ln_bwd_proj_kernel<T>, P_LDS>(dim3((d->M + PR - 1) / PR), dim3(256), s, p);
  EG_LAUNCH_CHECK("ln_bwd_proj");
  return 0;
}

}  // namespace

extern "C" int eg_ln_bwd_proj_blocks(int M) { return M > 0 ? (M + PR - 1) / PR : 0; }

extern "C" int eg_ln_bwd_proj(const eg_ln_bwd_proj_desc* d, void* stream) {
  EG_CHECK(d && d->dy && d->x && d->stats && d->gamma && d->W_frag && d->dx && d->dx_drop && d->dC && d->partial,
           "eg_ln_bwd_proj: null operand");
  EG_CHECK(d->dtype == EG_BF16 || d->dtype == EG_F16, "eg_ln_bwd_proj: 16-bit compute dtypes only (got %d)", d->dtype);
  EG_CHECK(d->M > 0 && d->d_model == PD, "eg_ln_bwd_proj: M=%d, d_model=%d (256 only)", d->M, d->d_model);
  EG_CHECK(d->partial_capacity_blocks >= eg_ln_bwd_proj_blocks(d->M),
           "eg_ln_bwd_proj: the partial buffer holds %d rows, the launch writes %d", d->partial_capacity_blocks, eg_ln_bwd_proj_blocks(d->M));
  EG_CHECK((long long)d->M * PD < (1ll << 32), "eg_ln_bwd_proj: M*D exceeds the 32-bit dropout index");
  EG_CHECK(d->drop1_p >= 0.f && d->drop1_p < 1.f && d->drop2_p >= 0.f && d->drop2_p < 1.f, "eg_ln_bwd_proj: dropout p");
  EG_CHECK((d->drop1_p == 0.f && d->drop2_p == 0.f) || d->state, "eg_ln_bwd_proj: dropout needs a step state");
  EG_CHECK(((uintptr_t)d->dy | (uintptr_t)d->x | (uintptr_t)d->W_frag | (uintptr_t)d->dx | (uintptr_t)d->dx_drop | (uintptr_t)d->dC) % 16 == 0,
           "eg_ln_bwd_proj: operands must be 16-B aligned");
  hipStream_t s = (hipStream_t)stream;
  return eg_dispatch_16(d->dtype, [&](auto t) { return lnproj_launch<typename decltype(t)::type>(d, s); });
}
