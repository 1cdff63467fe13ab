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
#include "lnproj.h"

namespace {

constexpr int PR = RT_ROWS;
constexpr int PD = RT_COLS;
constexpr int P_T = RT_TILEB;                 // 40,960 B per tile
constexpr int P_LDS = 2 * P_T;                // 81,920 B

// steps 2-4 are lnproj.h's device functions, shared with the norm-1 tail of eg_ffn_bwd_ln_proj (ffn.hip)
template <typename T>
__global__ __launch_bounds__(256, 2) void ln_bwd_proj_kernel(LnProjArgs<T> p) {
  typedef typename H16<T>::frag frag;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const ty = smem;                       // dy rows, then dyo rows: the product's A operand
  char* const tx = smem + P_T;                 // x rows; later the gain / bias sums and the epilogue image
  const int tid = threadIdx.x, lane = tid & 63;
  const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);
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
  const int l = lane & 31, hw = tid >> 5;        // half-wave hw = 0 .. 7 owns rows hw, hw + 8, .. (10 rows)
  float mean[LP_ROWS_PER_HW], rstd[LP_ROWS_PER_HW];
  lp_stats(p.stats, p.M, m0, hw, mean, rstd);
  float g[8], dg[8], db[8];
  load8(p.gamma + l * 8, g);
#pragma unroll
  for (int e = 0; e < 8; ++e) { dg[e] = 0.f; db[e] = 0.f; }
  uint32_t seed_lo = 0, seed_hi = 0;
  const bool drop = (p.d1.thresh | p.d2.thresh) != 0;
  if (drop) { seed_lo = p.st->seed_lo; seed_hi = p.st->seed_hi; }
  lp_req_w<T>(wu, wl, 0, wr[0]);
  lp_req_w<T>(wu, wl, 1, wr[1]);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- 2. LayerNorm backward, a half-wave per row ----
  const u32x4 nox[1] = {(u32x4){0u, 0u, 0u, 0u}};
  lp_ln_rows<T, false>(p, ty, tx, nox, m0, hw, l, g, mean, rstd, drop, seed_lo, seed_hi, dg, db);
  __syncthreads();                               // tile Y = dyo complete; tile X is free

  lp_sums(p.partial, (float*)tx, dg, db, tid, hw, l);

  // ---- 3. dC = dyo * W^T over K = 256;  4. epilogue through the wave-private fp32 image (tile X, behind the 16 KB of sums) ----
  lp_product<T>(p.dC, p.M, ty, wr, wu, wl, (float*)(tx + LP_SUMS_B + wn * RT_IMGB), m0, lane, wn);
}

template <typename T>
static int lnproj_launch(const eg_ln_bwd_proj_desc* d, hipStream_t s) {
  const LnProjArgs<T> p = lp_make_args<T>(d);
  eg_launch_lds<ln_bwd_proj_kernel<T>, P_LDS>(dim3((d->M + PR - 1) / PR), dim3(256), s, p);
  EG_LAUNCH_CHECK("ln_bwd_proj");
  return 0;
}

}  // namespace

extern "C" int eg_ln_bwd_proj_blocks(int M) { return M > 0 ? (M + PR - 1) / PR : 0; }

extern "C" int eg_ln_bwd_proj(const eg_ln_bwd_proj_desc* d, void* stream) {
  if (int rc = lp_check_desc(d, "eg_ln_bwd_proj", true)) return rc;
  hipStream_t s = (hipStream_t)stream;
  return eg_dispatch_16(d->dtype, [&](auto t) { return lnproj_launch<typename decltype(t)::type>(d, s); });
}
