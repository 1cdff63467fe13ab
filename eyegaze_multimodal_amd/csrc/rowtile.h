// The pieces of the row-tile kernel family (ffn.hip, lnproj.hip, attnblock.hip; widegemm.hip shares the image epilogue), each written
// once.  Device code only; every helper takes lane, l15 = lane & 15, g4 = lane >> 4, sw7 = rt_swz(l15) and the wave index as ARGUMENTS
// and never rebuilds them from threadIdx: ffn.hip and attnblock.hip derive them from an opaque copy of the lane id so that addresses are
// recomputed per chunk instead of being hoisted out of the chunk loop and spilled.
//   * resident tile: 80 rows x 256 16-bit columns in LDS, 512-B rows of 32 16-B pieces; piece `pos` of row r sits at position
//     pos ^ 2 (r & 7) -- free of bank conflicts under ds_read_b128's lane groups on 256-B and 512-B rows (pos ^ (r & 7) is two ways
//     conflicted there: SQ_LDS_BANK_CONFLICT 44 % of the LDS cycles);
//   * weights in FRAGMENT ORDER (eg_pack_table modes 3-8): [chunk][wave: 4][k-step: KS][tile: TJ][lane: 64] x 8 elements, so a
//     fragment load is one contiguous 1-KB read per wave;
//   * final epilogue: per 16-row tile the wave's four accumulator tiles pass through a wave-private fp32 image [16][RT_IMG_PITCH]; lane
//     (er = lane / 4, ec = lane % 4) then owns the 16 consecutive columns 16 ec .. of row er.
// (attnblock.hip's [rows][32] head images are not a row-tile piece: their layout and reads are attnhead.h's.)
// The ring kernels' K-loop fragment reads (tn_body256, wide_tile, rs_gemm_kernel) stay where they are: a compiler-visible LDS load
// after an LDS-DMA gets a vmcnt(0) in front of it, which is why those sit behind counted waits.
#pragma once
#include "common.h"

constexpr int RT_ROWS = 80;                          // rows of the resident tile (5 MFMA row tiles)
constexpr int RT_COLS = 256;                         // d_model
constexpr int RT_ROWB = RT_COLS * 2;                 // 512 B per row
constexpr int RT_TILEB = RT_ROWS * RT_ROWB;          // 40,960 B
constexpr int RT_IMG_PITCH = 68;                     // fp32 image pitch (floats): 64 + 4
constexpr int RT_IMGB = 16 * RT_IMG_PITCH * 4;       // one wave's image: 4,352 B

// 16 B per lane, global -> LDS (the LDS side is lane-linear: base + 16 lane)
__device__ __forceinline__ void eg_dma16(const char* g, char* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

// swizzle of a row, and the byte offset WITHIN the row of its 16-B piece `pos`
__device__ __forceinline__ int rt_swz(int row) { return (row & 7) << 1; }
__device__ __forceinline__ int rt_piece(int row, int pos) { return (pos ^ rt_swz(row)) << 4; }

// Resident-tile load: DMA instruction q = wn + 4 i (i = 0 .. 9 per wave) moves rows 2q, 2q + 1: lane -> row half lane / 32, LDS
// piece position lane % 32 holding the row's piece pos ^ 2 (row & 7).  The caller clamps rt_dma_row() to a row that exists and passes
// that row's first byte; two tiles interleave by issuing both inside one loop.
constexpr int RT_DMA_PER_WAVE = 10;
__device__ __forceinline__ int rt_dma_row(int wn, int lane, int i) { return 2 * (wn + 4 * i) + (lane >> 5); }
__device__ __forceinline__ void rt_dma_issue(const char* grow, char* tile, int wn, int lane, int i) {
  eg_dma16(grow + rt_piece(rt_dma_row(wn, lane, i), lane & 31), tile + (wn + 4 * i) * 1024);
}

// the five A fragments of k-step s (rows l15 + 16 i, 16-bit columns 32 s + 8 g4 ..) of an image with ROWB-byte rows
template <typename T, int ROWB = RT_ROWB>
__device__ __forceinline__ void rt_frags(const char* tile, int l15, int g4, int sw7, int s, typename H16<T>::frag (&xf)[5]) {
#pragma unroll
  for (int i = 0; i < 5; ++i) xf[i] = *(const typename H16<T>::frag*)(tile + (l15 + 16 * i) * ROWB + (((4 * s + g4) ^ sw7) << 4));
}

// columns n .. n + 15 (n % 16 == 0) of row r of the resident tile, as its two 16-B pieces
__device__ __forceinline__ void rt_tile_row16(const char* tile, int r, int n, u32x4& e0, u32x4& e1) {
  e0 = *(const u32x4*)(tile + r * RT_ROWB + rt_piece(r, n >> 3));
  e1 = *(const u32x4*)(tile + r * RT_ROWB + rt_piece(r, (n >> 3) + 1));
}

// Image transposition in its two halves: four accumulator tiles (MFMA layout: lane holds columns 16 j + 4 g4 .. + 3 of row l15) into
// the wave-private image, then v = columns 16 ec .. + 15 of row er.  The kernels leave their unrolled tile loop BETWEEN the halves once
// a tile lies wholly beyond the last row; with that exit in front of the store the compiler no longer unrolled eg_ffn_chain's loop
// (one rolled body indexing the accumulators: 1544 vector instructions fewer in the listing, more spills), so the halves stay apart.
__device__ __forceinline__ void rt_image_put(float* timg, const f32x4 (&acc)[4], int lane) {
  const int l15 = lane & 15, g4 = lane >> 4;
#pragma unroll
  for (int j = 0; j < 4; ++j) *(f32x4*)(timg + l15 * RT_IMG_PITCH + 16 * j + 4 * g4) = acc[j];
}
__device__ __forceinline__ void rt_image_get(const float* timg, int lane, float (&v)[16]) {
  const int er = lane >> 2, ec = lane & 3;
  load8(timg + er * RT_IMG_PITCH + 16 * ec, v);
  load8(timg + er * RT_IMG_PITCH + 16 * ec + 8, v + 8);
}

// ---- steps of the row epilogue on a lane's 16 consecutive values (eg_gemm_nt's order) ----
// both dropout sites on the two 8-element halves; idx = element index of v[0]
__device__ __forceinline__ void rt_dropout16(float (&v)[16], const DropCfg& d1, const DropCfg& d2, uint32_t seed_lo, uint32_t seed_hi,
                                             uint32_t idx) {
  if (d1.thresh | d2.thresh) {
    float (&v0)[8] = *(float (*)[8])v;
    float (&v1)[8] = *(float (*)[8])(v + 8);
    eg_dropout_run<8>(v0, d1, seed_lo, seed_hi, idx);
    eg_dropout_run<8>(v0, d2, seed_lo, seed_hi, idx);
    eg_dropout_run<8>(v1, d1, seed_lo, seed_hi, idx + 8);
    eg_dropout_run<8>(v1, d2, seed_lo, seed_hi, idx + 8);
  }
}
template <typename T>
__device__ __forceinline__ void rt_add16(float (&v)[16], const u32x4& e0, const u32x4& e1) {
  float rv[16];
  load8((const T*)&e0, rv);
  load8((const T*)&e1, rv + 8);
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] += rv[j];
}
template <typename T>
__device__ __forceinline__ void rt_store16(T* pc, const float (&v)[16]) {
  store8(pc, v);
  store8(pc + 8, v + 8);
}
// + bias, dropout sites, + residual (its two raw pieces), store; LNF: vv = what was stored, for eg_epilogue_layernorm256.
// STORE = false (the lean forms of eg_attn_block_fwd / eg_ffn_chain): the row is not written and pc is not read; vv still holds the
// values rounded to 16 bit, so the LayerNorm that follows sees what a keeping launch would have stored.
template <typename T, bool LNF, bool STORE = true>
__device__ __forceinline__ void rt_row_epilogue(float (&v)[16], const float (&bv)[16], const DropCfg& d1, const DropCfg& d2,
                                                uint32_t seed_lo, uint32_t seed_hi, uint32_t idx, bool has_res, const u32x4& e0,
                                                const u32x4& e1, T* pc, float (&vv)[16]) {
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] += bv[j];
  rt_dropout16(v, d1, d2, seed_lo, seed_hi, idx);
  if (has_res) rt_add16<T>(v, e0, e1);
  if constexpr (STORE) rt_store16(pc, v);
  if (LNF) {
#pragma unroll
    for (int j = 0; j < 16; ++j) vv[j] = round_store<T>(v[j]);
  }
}

// fragment order: element offset of (chunk c, wave wn, k-step s, tile j, lane) in a [chunk][4][KS][TJ][64] x 8 image.
// <8, 2> / <4, 4>: eg_ffn_chain's W1 / W2 (pack modes 3, 4 / 5, 6; <4, 4> also eg_ln_bwd_proj's W);  <8, 3> / <2, 4>:
// eg_attn_block_fwd's Wqkv / Wo (modes 7 / 8)
template <int KS, int TJ>
constexpr size_t rt_frag_elem(size_t c, int wn, int s, int j, int lane = 0) {
  return c * (4 * KS * TJ * 512) + (size_t)wn * (KS * TJ * 512) + (size_t)((s * TJ + j) * 512) + (size_t)(lane * 8);
}
