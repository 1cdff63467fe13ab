// The pieces of the attention family (attention.hip, attention_long.hip, attnblock.hip), each written once: the LDS image of a head
// slice, its MFMA operand reads, and the argument check of the two stand-alone cores.  d_k = 32 everywhere but in attention_long.hip,
// whose kernels also come 64 wide: a 64-wide head slice is TWO of the images below, [half][rows][32], and every piece here serves a half.
//   * head image: [rows][32] 16-bit elements = 64-B rows of four 16-B chunks.  The two 32-B halves of a row are SWAPPED when
//     (row >> 2) & 1: a transposed read touches 8 consecutive rows per lane group at one 32-B half, and with the swap those land in 8
//     distinct 32-B slots of the 256-B bank row instead of 4 slots twice;
//   * row read (hd_frag_row): lane (l15, g) takes chunk g of row `row` -- the A / B operand with the row on the MFMA's rows / lanes;
//   * transposed read (hd_frag_tr, ds_read_b64_tr_b16): k-slot 8 g + j of the fragment <-> row rbase + 16 (j >> 2) + 4 g + (j & 3),
//     column 16 dt + (lane & 15).  That is the order in which a 16 x 16 accumulator pair holds its rows (lane group g: rows 4 g .. 4 g + 3
//     of each tile), so two score accumulators packed by hd_pack_frag ARE the matching operand: no LDS round trip for P or dS;
//   * dropout index of element (row r of head-row space, key k): r * Sp2 + k with the EVEN row pitch Sp2 = (S + 1) & ~1.  One hash
//     serves the two elements of an aligned pair (common.h: eg_dropout_run), and with an even pitch a pair never straddles two rows.
// attnblock.hip's forward is bit-identical to eg_attention_fwd (tests/test_gpu_attnblock.py) because both read these definitions.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(8))) short s16x8;

// T = bf16_t or f16_t: the 16-bit storage type; FR<T> = its MFMA operand fragment (8 elements per lane)
template <typename T> using FR = typename H16<T>::frag;

constexpr float HD_SCALE = 0.17677669529663687f;  // 1/sqrt(32)
template <int DK> constexpr float hd_scale() { return DK == 32 ? HD_SCALE : 0.125f; }   // 1/sqrt(DK), DK = 32 or 64
constexpr int HD_MAX_S = 160;                     // eg_attention_*: a whole window's scores in one wave's registers (SP = 96 / 128 / 160)

template <typename T>
__device__ __forceinline__ FR<T> hd_frag_global(const T* p, bool valid) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if (valid) v = *(const u32x4*)p;
  return __builtin_bit_cast(FR<T>, v);
}
// byte offset of 16-B chunk c4 of a row
__device__ __forceinline__ int hd_img_off(int row, int c4) {
  return row * 64 + ((((c4 >> 1) ^ ((row >> 2) & 1))) << 5) + ((c4 & 1) << 4);
}
template <typename T>
__device__ __forceinline__ FR<T> hd_frag_row(const char* img, int row, int g) {
  return *(const FR<T>*)(img + hd_img_off(row, g));
}
template <typename T>
__device__ __forceinline__ FR<T> hd_frag_tr(const char* img, int rbase, int dt, int lane) {
  const int g = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
  s16x4 part[2];
#pragma unroll
  for (int h2 = 0; h2 < 2; ++h2) {
    const int row = rbase + 16 * h2 + 4 * g + qq;
    const int off = row * 64 + ((dt ^ (g & 1)) << 5) + pp * 8;
    part[h2] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(img + off));
  }
  s16x8 t = {part[0][0], part[0][1], part[0][2], part[0][3], part[1][0], part[1][1], part[1][2], part[1][3]};
  return __builtin_bit_cast(FR<T>, t);
}
// hd_frag_tr of an image that ends at row rbase + 16: the upper 16 rows are zero k-slots and are not read
template <typename T>
__device__ __forceinline__ FR<T> hd_frag_tr_lo(const char* img, int rbase, int dt, int lane) {
  const int g = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
  const int row = rbase + 4 * g + qq;
  const int off = row * 64 + ((dt ^ (g & 1)) << 5) + pp * 8;
  const s16x4 part = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(img + off));
  s16x8 t = {part[0], part[1], part[2], part[3], 0, 0, 0, 0};
  return __builtin_bit_cast(FR<T>, t);
}
// two accumulator tiles (key / query tiles 2 n, 2 n + 1) -> the operand whose k-slots hd_frag_tr's map names
template <typename T>
__device__ __forceinline__ FR<T> hd_pack_frag(const f32x4& a, const f32x4& b) {
  u32x4 v;
  v[0] = H16<T>::pack2(a[0], a[1]);
  v[1] = H16<T>::pack2(a[2], a[3]);
  v[2] = H16<T>::pack2(b[0], b[1]);
  v[3] = H16<T>::pack2(b[2], b[3]);
  return __builtin_bit_cast(FR<T>, v);
}
// the fp32 parity kernels' dot product: one fmaf chain in ascending d
template <int DK>
__device__ __forceinline__ float hd_dot(const float* a, const float* b) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < DK; ++d) s = fmaf(a[d], b[d], s);
  return s;
}
__device__ __forceinline__ float hd_dot32(const float* a, const float* b) { return hd_dot<32>(a, b); }

// host: the argument check of eg_attention_* (max_s = HD_MAX_S, idx32: element indices of the dropout hash are 32 bit) and of
// eg_attention_long_* (max_s = EG_ATTN_LONG_MAX_S, 64-bit indices).  The dtype comes first, so the entry points call it before
// they look at their pointers.
static inline int hd_check(const char* who, int NB, int S, int H, int kv_shift, int dtype, float p, const void* st, int max_s, bool idx32) {
  if (eg_dtype_check(who, dtype, true)) return 1;
  EG_CHECK(NB > 0 && S > 0 && H > 0, "%s: bad shape NB=%d S=%d H=%d", who, NB, S, H);
  EG_CHECK(S <= max_s, "%s: S=%d exceeds the %s limit of %d", who, S, idx32 ? "register-resident" : "long-attention", max_s);
  EG_CHECK(kv_shift >= 0 && kv_shift < NB, "%s: kv_shift=%d out of range", who, kv_shift);
  EG_CHECK(p >= 0.f && p < 1.f && (p == 0.f || st), "%s: dropout p=%f needs a step state", who, (double)p);
  EG_CHECK(!idx32 || (long long)NB * H * S * (S + 1) < (1ll << 32), "%s: NB*H*S*S exceeds the 32-bit dropout index", who);
  return 0;
}
