// Multi-head attention core for short sequences (S <= 160, d_k = 32) on gfx950.
// One wave owns one (sample, head): the whole S x S score matrix of a head lives in that wave's registers.
//   scores^T tile = K_tile(16 keys x 32) * Q_tile^T            -> v_mfma_f32_16x16x32_bf16, key on rows, query on lanes
//   soft-max over keys = in-register over tiles + 2 cross-lane steps (lanes l, l^16, l^32, l^48 share a query)
//   O^T = V^T * P^T: the score accumulators ARE the P^T operand (no LDS round trip); V^T fragments come from a
//   row-major LDS image through ds_read_b64_tr_b16 with the key permutation the accumulator layout implies
//   (attnhead.h: the image, its reads and the permutation).
// Backward recomputes P from the saved log-sum-exp (flash style) in a single sweep over the key tiles (attn_bwd1_kernel):
// every 16 x 16 block of P / dS is formed once and feeds dQ, dK and dV; delta = rowsum(dO * O).
#include "attnhead.h"

namespace {

// The rows of a head slice into its LDS image, in two halves, so that a kernel can request SEVERAL images (and whatever else its
// prologue reads) before the first wait: every load -> wait -> LDS store pair left to itself cost one HBM latency (stamped: 9 200
// cycles for the three images of the single-sweep backward, 28 % of a wave's lifetime).  Chunk id = first + 128 i: row id / 4, 16-B
// chunk id % 4; rows >= S are stored as zeros.
template <typename T, int NCH>
__device__ __forceinline__ void rows_request(u32x4 (&r)[NCH], const T* src, long long ld, int S, int first) {
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int id = first + 128 * i;
    const int row = id >> 2, c4 = id & 3;
    r[i] = (u32x4){0u, 0u, 0u, 0u};
    if (row < S) r[i] = *(const u32x4*)(src + (long long)row * ld + c4 * 8);
  }
}
template <int NCH>
__device__ __forceinline__ void rows_store(char* img, const u32x4 (&r)[NCH], int SP, int first) {
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int id = first + 128 * i;
    if (id < SP * 4) *(u32x4*)(img + hd_img_off(id >> 2, id & 3)) = r[i];
  }
}

template <typename T, int SP>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const T* __restrict__ qkv, T* __restrict__ ctx,
                                                       float* __restrict__ lse, int NB, int S, int H, int kv_shift,
                                                       DropCfg dc, const eg_step_state* st) {
  constexpr int NKT = SP / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // two waves share one (window, head): they split the staging of V and take alternate query tiles
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, role = wave & 1;
  const int l15 = lane & 15, g = lane >> 4;
  int pid = blockIdx.x * 2 + (wave >> 1);
  const bool valid = pid < NB * H;
  if (!valid) pid = NB * H - 1;
  const int b = pid / H, h = pid % H;
  const int bk = (b + kv_shift) % NB;
  const int D = H * 32;
  const long long ld = 3ll * D;
  const T* qbase = qkv + (long long)b * S * ld + h * 32;
  const T* kbase = qkv + (long long)bk * S * ld + D + h * 32;
  const T* vbase = kbase + D;
  char* vimg = smem + (wave >> 1) * (SP * 64);
  constexpr int NCH = SP / 32;
  u32x4 rv[NCH];
  rows_request<T, NCH>(rv, vbase, ld, S, lane + 64 * role);    // (stored below, after every other request of the prologue)
  const int nkt = (S + 15) >> 4;
  FR<T> kf[NKT];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    const int key = kt * 16 + l15;
    kf[kt] = hd_frag_global<T>(kbase + (long long)key * ld + g * 8, key < S);
  }
  uint32_t seed_lo = 0, seed_hi = 0;
  if (dc.thresh) { seed_lo = st->seed_lo; seed_hi = st->seed_hi; }
  rows_store<NCH>(vimg, rv, SP, lane + 64 * role);
  __syncthreads();
  // (Requesting every query tile's fragment before the loop, unrolling it, and a one-register tail key tile for S = 16 n + 1 were
  // measured on this kernel too: 52.9 -> 65.7 us at SP = 128, 69.3 -> 84.4 us at SP = 160, 27.7 -> 30.4 us at SP = 96 -- more registers,
  // one wave per SIMD fewer.  Only the batched prologue stayed.)
  for (int qt = role; qt < nkt; qt += 2) {
    const int q = qt * 16 + l15;
    const FR<T> qf = hd_frag_global<T>(qbase + (long long)q * ld + g * 8, q < S);
    f32x4 s[NKT];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      s[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (kt < nkt) {   // wave-uniform: key tiles beyond the sequence cost nothing (S = 65 uses 5 of the 6 tiles)
        s[kt] = H16<T>::mfma(kf[kt], qf, s[kt]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kt * 16 + 4 * g + r;
          const float v = key < S ? s[kt][r] * HD_SCALE : -INFINITY;
          s[kt][r] = v;
          mx = fmaxf(mx, v);
        }
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      if (kt < nkt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __expf(s[kt][r] - mx);
          s[kt][r] = p;
          sum += p;
        }
      }
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;
    if (g == 0 && q < S && valid) lse[((long long)b * H + h) * S + q] = mx + __logf(sum);
    const uint32_t rowidx = (uint32_t)((b * H + h) * S + q) * (uint32_t)((S + 1) & ~1);  // even row pitch: aligned pairs
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      if (kt < nkt) {
        float pv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) pv[r] = s[kt][r] * inv;
        eg_dropout_run<4>(pv, dc, seed_lo, seed_hi, rowidx + (uint32_t)(kt * 16 + 4 * g));
#pragma unroll
        for (int r = 0; r < 4; ++r) s[kt][r] = pv[r];
      }
    }
    f32x4 o[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int kp = 0; kp < NKT / 2; ++kp) {
      if (2 * kp < nkt) {
        const FR<T> pf = hd_pack_frag<T>(s[2 * kp], s[2 * kp + 1]);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const FR<T> vf = hd_frag_tr<T>(vimg, 32 * kp, dt, lane);
          o[dt] = H16<T>::mfma(vf, pf, o[dt]);
        }
      }
    }
    if (q < S && valid) {
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        float v[4] = {o[dt][0], o[dt][1], o[dt][2], o[dt][3]};
        store4(ctx + ((long long)b * S + q) * D + h * 32 + 16 * dt + 4 * g, v);
      }
    }
  }
}


// ------------------------------------------------------------------------------------------------
// Single-sweep backward: every 16 x 16 block of P / dS is computed ONCE.
// (A two-pass backward -- dQ with key rows / query lanes, then dK / dV in the transposed layout -- evaluates exp and the dropout hash
// of each block twice and is VALU-issue-bound on exactly that.)  Here a wave owns alternate KEY tiles and walks all query tiles in
// pairs.  Per block it forms, in the key-rows / query-lanes layout, P*mask and dS; dS goes straight into the dQ MFMA of its query tile (B operand:
// query lanes, key k-slots -- the other key tile of the pair is a zero half), and both are TRANSPOSED through a 2-KB
// wave-private LDS image (written as 8-B row pieces, read back with ds_read_b64_tr_b16 as B operands with key lanes and the
// query pair in the k-slots) for the dV / dK MFMAs of the wave's key tile.  dK / dV of a key tile are complete in the wave
// (16 registers, stored once per key tile); dQ accumulates per query tile across the wave's key tiles (8 registers per tile) and
// the two waves of a head exchange halves through LDS in a fixed order (bit-reproducible).  Registers: 8 NKT + 16 accumulators
// instead of the 16 NKT of a query-major sweep, LDS 23 KB per head at SP = 96: three workgroups per CU.
// ------------------------------------------------------------------------------------------------
// NKTX > 0: the tile count is a compile-time constant and, with TAIL, the last key tile holds ONE valid key (S = 16 n + 1: the
// S = 65 windows of the benchmark); <SP, 0, false> is the general form.
// IR: the rows of the LDS images, apart from the tile capacity SP (which governs NKT, the pair loop and accq).  Windows of up to 80
// tokens are staged in 80-row images (IR = 80 at SP = 96): 40 192 B per workgroup instead of 46 592 and 128 registers without
// scratch memory instead of 153, four workgroups per CU instead of three (2048 workgroups of the benchmark: two full rounds instead
// of 2.67).  At 128 registers WITH scratch memory (what the bound alone compiles to: 136 B per lane) the step is 0.18 ms slower than
// at three per CU; without any, 0.04 ms faster.
constexpr int bwd1_lds(int IR) { return 2 * (3 * IR * 64 + 2 * IR * 4 + 2 * 2 * 32 * 32); }
constexpr int bwd1_wg(int SP, int IR) { return IR < SP ? 4 : SP <= 96 ? 3 : 2; }      // workgroups per CU: registers AND LDS
// A transposed read covers 32 rows from rbase.  At rbase = 64 its upper 16 lie beyond an 80-row image; they are rows >= S, zeros
// in a full image, so they are zero k-slots here (and what follows the image in LDS is never an MFMA operand).
template <typename T, int SP, int IR>
__device__ __forceinline__ FR<T> bwd1_frag_tr(const char* img, int rbase, int dt, int lane) {
  if (IR == SP || rbase + 32 <= IR) return hd_frag_tr<T>(img, rbase, dt, lane);
  return hd_frag_tr_lo<T>(img, rbase, dt, lane);
}

// One key tile of the single-sweep backward (attn_bwd1_kernel): all of the wave's query pairs against key tile kt.
template <typename T, int SP, int IR, int NKTX, bool tail>
__device__ __forceinline__ void bwd1_key_tile(const int kt, const int S, const int nkt, const bool valid, const int lane, const char* kimg,
                                              const char* qimg, const char* doimg, const float* lsel, const float* dl, char* pimg,
                                              char* simg, const T* vbase, const long long ld, FR<T>& vnext, f32x4 (&accq)[SP / 16][2],
                                              const DropCfg& dc, const uint32_t seed_lo, const uint32_t seed_hi, const uint32_t headidx,
                                              const uint32_t Sp2, T* dqkv, const int bk, const int h, const int D) {
  constexpr int NKT = SP / 16;
  const int l15 = lane & 15, g = lane >> 4;
  const int qq = l15 >> 2, pp = l15 & 3;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  const int key = kt * 16 + l15;
  const FR<T> kfr = hd_frag_row<T>(kimg, key, g);       // the staged image (zero rows beyond S) instead of a second global read
  const FR<T> vfr = vnext;                                   // requested one key tile ahead
  {
    const int key2 = key + 32;
    vnext = hd_frag_global<T>(vbase + (long long)key2 * ld + g * 8, key2 < S && kt + 2 < nkt);
  }
  FR<T> ktr[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) ktr[dt] = bwd1_frag_tr<T, SP, IR>(kimg, 32 * (kt >> 1), dt, lane);
  f32x4 dk[2] = {zero4, zero4}, dv[2] = {zero4, zero4};
#pragma unroll
  for (int qp = 0; qp < NKT / 2; ++qp) {
    if (2 * qp < nkt) {
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int qt = 2 * qp + h2;
        const int off = (16 * h2 + l15) * 32 + g * 8;      // the block in the wave's images: query slot 16 h2 + l15, keys 4g .. 4g+3
        if (NKTX ? qt >= NKTX : qt >= nkt) {                // a query tile beyond the sequence: zero slots, no work
          *(u32x2*)(pimg + off) = (u32x2){0u, 0u};
          *(u32x2*)(simg + off) = (u32x2){0u, 0u};
          continue;
        }
        const int q = qt * 16 + l15;
        const FR<T> qf = hd_frag_row<T>(qimg, q, g);
        const FR<T> dof = hd_frag_row<T>(doimg, q, g);
        const float lq = lsel[q], dq = dl[q];
        // (at 128 registers the key tile's K rows are read again for every block: one ds_read_b128 instead of four held registers)
        const FR<T> kfb = IR < SP ? hd_frag_row<T>(kimg, key, g) : kfr;
        const f32x4 sT = H16<T>::mfma(kfb, qf, zero4);
        const f32x4 dpT = H16<T>::mfma(vfr, dof, zero4);
        float pd[4] = {0.f, 0.f, 0.f, 0.f};
        f32x4 dsv = zero4;
        if (tail) {
          const float m0 = eg_dropout(1.f, dc, seed_lo, seed_hi, (headidx + (uint32_t)q) * Sp2 + (uint32_t)(kt * 16 + 4 * g));
          const float p = (g == 0 && q < S) ? __expf(sT[0] * HD_SCALE - lq) : 0.f;
          pd[0] = p * m0;
          dsv[0] = p * (dpT[0] * m0 - dq);
        } else {
          float m[4] = {1.f, 1.f, 1.f, 1.f};
          eg_dropout_run<4>(m, dc, seed_lo, seed_hi, (headidx + (uint32_t)q) * Sp2 + (uint32_t)(kt * 16 + 4 * g));
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int kk = kt * 16 + 4 * g + r;
            const float p = (kk < S && q < S) ? __expf(sT[r] * HD_SCALE - lq) : 0.f;
            pd[r] = p * m[r];
            dsv[r] = p * (dpT[r] * m[r] - dq);
          }
        }
        // dQ of this query tile: dS is the B operand as it stands (query lanes, key k-slots); the other key tile of the pair is zero
        const FR<T> dsf = (kt & 1) ? hd_pack_frag<T>(zero4, dsv) : hd_pack_frag<T>(dsv, zero4);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) accq[qt][dt] = H16<T>::mfma(ktr[dt], dsf, accq[qt][dt]);
        // the block into the wave's images (8 B of a 32-B row)
        u32x2 pw, sw;
        pw[0] = H16<T>::pack2(pd[0], pd[1]);   pw[1] = H16<T>::pack2(pd[2], pd[3]);
        sw[0] = H16<T>::pack2(dsv[0], dsv[1]); sw[1] = H16<T>::pack2(dsv[2], dsv[3]);
        *(u32x2*)(pimg + off) = pw;
        *(u32x2*)(simg + off) = sw;
      }
      // dV, dK of this key tile: the transposed blocks (key lanes, the query pair in the k-slots) against dO^T / Q^T
      s16x4 pa[2], sa[2];
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int off = (16 * h2 + 4 * g + qq) * 32 + pp * 8;
        pa[h2] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(pimg + off));
        sa[h2] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(simg + off));
      }
      const s16x8 pt = {pa[0][0], pa[0][1], pa[0][2], pa[0][3], pa[1][0], pa[1][1], pa[1][2], pa[1][3]};
      const s16x8 stt = {sa[0][0], sa[0][1], sa[0][2], sa[0][3], sa[1][0], sa[1][1], sa[1][2], sa[1][3]};
      const FR<T> pdf = __builtin_bit_cast(FR<T>, pt), dsT = __builtin_bit_cast(FR<T>, stt);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const FR<T> dotr = bwd1_frag_tr<T, SP, IR>(doimg, 32 * qp, dt, lane);
        dv[dt] = H16<T>::mfma(dotr, pdf, dv[dt]);
        const FR<T> qtr = bwd1_frag_tr<T, SP, IR>(qimg, 32 * qp, dt, lane);
        dk[dt] = H16<T>::mfma(qtr, dsT, dk[dt]);
      }
    }
  }
  if (key < S && valid) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      float a[4] = {dk[dt][0] * HD_SCALE, dk[dt][1] * HD_SCALE, dk[dt][2] * HD_SCALE, dk[dt][3] * HD_SCALE};
      float c[4] = {dv[dt][0], dv[dt][1], dv[dt][2], dv[dt][3]};
      T* row = dqkv + ((long long)bk * S + key) * ld + h * 32 + 16 * dt + 4 * g;
      store4(row + D, a);
      store4(row + 2 * D, c);
    }
  }
}

template <typename T, int SP, int NKTX, bool TAIL, int IR = SP>
__global__ __launch_bounds__(256, bwd1_wg(SP, IR)) void attn_bwd1_kernel(const T* __restrict__ qkv, const T* __restrict__ ctx,
                                                        const T* __restrict__ dctx, const float* __restrict__ lse,
                                                        T* __restrict__ dqkv, int NB, int S, int H, int kv_shift,
                                                        DropCfg dc, const eg_step_state* st) {
  constexpr int NKT = SP / 16;
  constexpr int IMG = IR * 64;
  constexpr int SCR = 2 * 32 * 32;                            // one wave's P and dS images: [32 query slots][16 keys] each
  constexpr int WB = 3 * IMG + 2 * IR * 4 + 2 * SCR;
  static_assert(IR % 16 == 0 && IR <= SP && WB == bwd1_lds(IR) / 2, "attn_bwd1: image rows");
  static_assert(2 * (NKT / 2) * 2 * 64 * 16 <= 3 * IMG, "attn_bwd1: the dQ exchange buffer lies inside the three dead images");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // (IR < SP: the wave id as a scalar, so that the head's indices and base addresses are scalars too and not vector registers)
  const int lane = threadIdx.x & 63, wave = IR < SP ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : threadIdx.x >> 6, role = wave & 1;
  const int l15 = lane & 15, g = lane >> 4;
  int pid = blockIdx.x * 2 + (wave >> 1);
  const bool valid = pid < NB * H;
  if (!valid) pid = NB * H - 1;
  const int b = pid / H, h = pid % H;
  const int bk = (b + kv_shift) % NB;
  const int D = H * 32;
  const long long ld = 3ll * D;
  const T* qbase = qkv + (long long)b * S * ld + h * 32;
  const T* kbase = qkv + (long long)bk * S * ld + D + h * 32;
  const T* vbase = kbase + D;
  const T* dobase = dctx + (long long)b * S * D + h * 32;
  const T* obase = ctx + (long long)b * S * D + h * 32;
  char* base = smem + (wave >> 1) * WB;
  char* qimg = base;
  char* kimg = base + IMG;
  char* doimg = base + 2 * IMG;
  float* lsel = (float*)(base + 3 * IMG);
  float* dl = lsel + IR;
  char* pimg = base + 3 * IMG + 2 * IR * 4 + role * SCR;
  char* simg = pimg + 32 * 32;
  // every global read of the prologue is requested before the first wait: the three images (this wave's half) and the lane's
  // dO / O rows and log-sum-exp for delta = rowsum(dO * O)
  constexpr int NCH = (IR + 31) / 32;                        // 16-B chunks per lane and image: IR * 4 / 128, rounded up (rows_store
                                                             // drops the chunks of rows >= IR, rows_request reads none: IR >= S)
  const int first = lane + 64 * role;
  u32x4 rq[NCH], rk[NCH], rd[NCH];
  rows_request<T, NCH>(rq, qbase, ld, S, first);
  rows_request<T, NCH>(rk, kbase, ld, S, first);
  rows_request<T, NCH>(rd, dobase, D, S, first);
  constexpr int NQ = (IR + 127) / 128;                       // delta rows per lane (query first + 128 j)
  // On 80-row images the lane's dO row is read back from the dO image after a barrier instead of fetched a second time: 16
  // registers and four global loads fewer across the prologue's wait (same elements in the same order: delta keeps its bits).
  // Worth 0.013 ms per step against the second fetch, both at 128 registers without scratch memory.
  constexpr bool DIMG = IR < SP;
  u32x4 da[NQ][4], oa[NQ][4];
  float lq0[NQ];
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    const int qd = first + 128 * j;
    lq0[j] = 0.f;
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) { da[j][c4] = (u32x4){0u, 0u, 0u, 0u}; oa[j][c4] = (u32x4){0u, 0u, 0u, 0u}; }
    if (qd < S) {
      lq0[j] = lse[((long long)b * H + h) * S + qd];
#pragma unroll
      for (int c4 = 0; c4 < 4; ++c4) {
        if (!DIMG) da[j][c4] = *(const u32x4*)(dobase + (long long)qd * D + c4 * 8);
        oa[j][c4] = *(const u32x4*)(obase + (long long)qd * D + c4 * 8);
      }
    }
  }
  rows_store<NCH>(qimg, rq, IR, first);
  rows_store<NCH>(kimg, rk, IR, first);
  rows_store<NCH>(doimg, rd, IR, first);
  if (DIMG) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const int qd = first + 128 * j;
      if (qd < IR) {
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) da[j][c4] = *(const u32x4*)(doimg + hd_img_off(qd, c4));
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    const int qd = first + 128 * j;
    if (qd < IR) {
      float dsum = 0.f;
#pragma unroll
      for (int c4 = 0; c4 < 4; ++c4) {
        float a[8], o[8];
        load8((const T*)&da[j][c4], a);
        load8((const T*)&oa[j][c4], o);
#pragma unroll
        for (int e = 0; e < 8; ++e) dsum += a[e] * o[e];
      }
      lsel[qd] = lq0[j];
      dl[qd] = dsum;
    }
  }
  const int nkt = (S + 15) >> 4;        // (run-time also when NKTX names it: the pair loop below keeps one basic block per pair --
                                        //  with a constant count the scheduler hoisted every pair's operand reads and spilled 31 registers)
  if (IR < SP) __builtin_assume(nkt <= IR / 16);   // launch_bwd: S <= IR, so the accumulators of query tiles >= IR / 16 are dead registers
  uint32_t seed_lo = 0, seed_hi = 0;
  if (dc.thresh) { seed_lo = st->seed_lo; seed_hi = st->seed_hi; }
  const uint32_t headidx = (uint32_t)((b * H + h) * S);
  const uint32_t Sp2 = (uint32_t)((S + 1) & ~1);
  __syncthreads();

  f32x4 accq[NKT][2];
#pragma unroll
  for (int qt = 0; qt < NKT; ++qt)
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) accq[qt][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int qq = l15 >> 2, pp = l15 & 3;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // A last key tile with a single valid key (TAIL) evaluates one accumulator register per lane instead of four, and the second
  // query tile of a pair is skipped when it lies beyond the sequence (odd tile counts): at S = 65 the wave with key tiles 0, 2, 4
  // did 18 full blocks against the other's 12; now 10 + 5 quarter blocks against 10.  The tail tile is its own copy of the body
  // (compile-time flag), so neither copy carries a branch inside its unrolled blocks.
  FR<T> vnext = hd_frag_global<T>(vbase + (long long)(role * 16 + l15) * ld + g * 8, role * 16 + l15 < S && role < nkt);
  const int nfull = TAIL ? NKTX - 1 : nkt;
#define EG_BWD1_ARGS(lane) S, nkt, valid, lane, kimg, qimg, doimg, lsel, dl, pimg, simg, vbase, ld, vnext, accq, dc, seed_lo, seed_hi, headidx, Sp2, dqkv, bk, h, D
  for (int kt = role; kt < nfull; kt += 2) bwd1_key_tile<T, SP, IR, NKTX, false>(kt, EG_BWD1_ARGS(lane));
  // With 128 registers (IR < SP) whatever the tail tile and the dQ exchange derive from the lane id is formed behind the loop: the
  // compiler computed those addresses in front of it and carried them across it in scratch memory.
  int lane_t = lane;
  if (IR < SP) asm volatile("" : "+v"(lane_t));
  if (TAIL && role == ((NKTX - 1) & 1)) bwd1_key_tile<T, SP, IR, NKTX, true>(NKTX - 1, EG_BWD1_ARGS(lane_t));
#undef EG_BWD1_ARGS
  int lane_x = lane;
  if (IR < SP) asm volatile("" : "+v"(lane_x));
  const int l15x = lane_x & 15, gx = lane_x >> 4;

  // ---- dQ: role 0 finishes query tiles [0, NKT/2), role 1 the rest; each hands the other its partial of the other's tiles ----
  __syncthreads();                                            // the images are dead: they carry the partials
  f32x4* xbuf = (f32x4*)base;                                 // [2 roles][NKT/2][2][64 lanes]
#pragma unroll
  for (int i = 0; i < NKT / 2; ++i) {
    const int qt = (1 - role) * (NKT / 2) + i;                // a tile the OTHER wave finishes
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      // Both candidates are pinned in registers before the choice: left to itself the compiler turns "role ? accq[i] : accq[j]" (as a
      // select or as a branch) into ONE load from a role-dependent address, which puts all of accq in scratch memory for the whole
      // kernel (784 us against 421 us per step when that happened to the S = 65 instantiation).
      f32x4 lo = accq[i][dt], hi = accq[NKT / 2 + i][dt];
      asm volatile("" : "+v"(lo), "+v"(hi));
      xbuf[((role * (NKT / 2) + i) * 2 + dt) * 64 + lane_x] = role ? lo : hi;
    }
    (void)qt;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NKT / 2; ++i) {
    const int qt = role * (NKT / 2) + i;
    const int q = qt * 16 + l15x;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const f32x4 other = xbuf[(((1 - role) * (NKT / 2) + i) * 2 + dt) * 64 + lane_x];
      f32x4 lo = accq[i][dt], hi = accq[NKT / 2 + i][dt];
      asm volatile("" : "+v"(lo), "+v"(hi));
      const f32x4 mine = role ? hi : lo;
      const f32x4 tot = role ? other + mine : mine + other;    // fixed order: role 0's partial + role 1's partial
      if (q < S && valid) {
        float v[4] = {tot[0] * HD_SCALE, tot[1] * HD_SCALE, tot[2] * HD_SCALE, tot[3] * HD_SCALE};
        store4(dqkv + ((long long)b * S + q) * ld + h * 32 + 16 * dt + 4 * gx, v);
      }
    }
  }
}


// ------------------------------------------------------------------------------------------------
// Exact-fp32 attention (EG_F32): the parity path.  One workgroup per (sample, head), one thread per query
// (forward, dQ) or per key (dK, dV); Q/K/V/dO head slices live in LDS and are read as broadcasts.
// Plain fmaf chains, no MFMA: this path exists to pin the orchestration bit-tight against the fp32 oracle.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn_fwd_f32_kernel(const float* __restrict__ qkv, float* __restrict__ ctx,
                                                           float* __restrict__ lse, int NB, int S, int H, int kv_shift,
                                                           DropCfg dc, const eg_step_state* st) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Kl = (float*)smem;       // [S][32]
  float* Vl = Kl + S * 32;        // [S][32]
  const int pid = blockIdx.x, b = pid / H, h = pid % H, bk = (b + kv_shift) % NB, D = H * 32;
  const long long ld = 3ll * D;
  for (int i = threadIdx.x; i < S * 32; i += blockDim.x) {
    const int r = i >> 5, d = i & 31;
    Kl[i] = qkv[((long long)bk * S + r) * ld + D + h * 32 + d];
    Vl[i] = qkv[((long long)bk * S + r) * ld + 2 * D + h * 32 + d];
  }
  __syncthreads();
  const int q = threadIdx.x;
  if (q >= S) return;
  float qv[32], o[32];
#pragma unroll
  for (int d = 0; d < 32; ++d) { qv[d] = qkv[((long long)b * S + q) * ld + h * 32 + d]; o[d] = 0.f; }
  float mx = -INFINITY;
  for (int k = 0; k < S; ++k) mx = fmaxf(mx, hd_dot32(qv, Kl + k * 32) * HD_SCALE);
  float sum = 0.f;
  for (int k = 0; k < S; ++k) sum += expf(hd_dot32(qv, Kl + k * 32) * HD_SCALE - mx);
  const float inv = 1.0f / sum;
  uint32_t seed_lo = 0, seed_hi = 0;
  if (dc.thresh) { seed_lo = st->seed_lo; seed_hi = st->seed_hi; }
  const uint32_t rowidx = (uint32_t)((b * H + h) * S + q) * (uint32_t)((S + 1) & ~1);
  for (int k = 0; k < S; ++k) {
    float p = expf(hd_dot32(qv, Kl + k * 32) * HD_SCALE - mx) * inv;
    if (dc.thresh) p = eg_dropout(p, dc, seed_lo, seed_hi, rowidx + (uint32_t)k);
#pragma unroll
    for (int d = 0; d < 32; ++d) o[d] = fmaf(p, Vl[k * 32 + d], o[d]);
  }
  lse[((long long)b * H + h) * S + q] = mx + logf(sum);
#pragma unroll
  for (int d = 0; d < 32; ++d) ctx[((long long)b * S + q) * D + h * 32 + d] = o[d];
}

__global__ __launch_bounds__(256) void attn_bwd_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ ctx,
                                                           const float* __restrict__ dctx, const float* __restrict__ lse,
                                                           float* __restrict__ dqkv, int NB, int S, int H, int kv_shift,
                                                           DropCfg dc, const eg_step_state* st) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Ql = (float*)smem;        // [S][32]
  float* Kl = Ql + S * 32;
  float* Vl = Kl + S * 32;
  float* Dl = Vl + S * 32;         // dO
  float* lsel = Dl + S * 32;       // [S]
  float* dl = lsel + S;            // [S]  delta = rowsum(dO * O)
  const int pid = blockIdx.x, b = pid / H, h = pid % H, bk = (b + kv_shift) % NB, D = H * 32;
  const long long ld = 3ll * D;
  for (int i = threadIdx.x; i < S * 32; i += blockDim.x) {
    const int r = i >> 5, d = i & 31;
    Ql[i] = qkv[((long long)b * S + r) * ld + h * 32 + d];
    Kl[i] = qkv[((long long)bk * S + r) * ld + D + h * 32 + d];
    Vl[i] = qkv[((long long)bk * S + r) * ld + 2 * D + h * 32 + d];
    Dl[i] = dctx[((long long)b * S + r) * D + h * 32 + d];
  }
  for (int r = threadIdx.x; r < S; r += blockDim.x) {
    lsel[r] = lse[((long long)b * H + h) * S + r];
    float s = 0.f;
    for (int d = 0; d < 32; ++d)
      s = fmaf(dctx[((long long)b * S + r) * D + h * 32 + d], ctx[((long long)b * S + r) * D + h * 32 + d], s);
    dl[r] = s;
  }
  __syncthreads();
  uint32_t seed_lo = 0, seed_hi = 0;
  if (dc.thresh) { seed_lo = st->seed_lo; seed_hi = st->seed_hi; }
  const uint32_t headidx = (uint32_t)((b * H + h) * S);
  const int t = threadIdx.x;
  if (t < S) {
    // thread = query t: dQ
    float acc[32];
#pragma unroll
    for (int d = 0; d < 32; ++d) acc[d] = 0.f;
    for (int k = 0; k < S; ++k) {
      const float p = expf(hd_dot32(Ql + t * 32, Kl + k * 32) * HD_SCALE - lsel[t]);
      float dp = hd_dot32(Dl + t * 32, Vl + k * 32);
      if (dc.thresh) dp = eg_dropout(dp, dc, seed_lo, seed_hi, (headidx + (uint32_t)t) * (uint32_t)((S + 1) & ~1) + (uint32_t)k);
      const float ds = p * (dp - dl[t]);
#pragma unroll
      for (int d = 0; d < 32; ++d) acc[d] = fmaf(ds, Kl[k * 32 + d], acc[d]);
    }
#pragma unroll
    for (int d = 0; d < 32; ++d) dqkv[((long long)b * S + t) * ld + h * 32 + d] = acc[d] * HD_SCALE;
    // thread = key t: dK, dV
    float ak[32], av[32];
#pragma unroll
    for (int d = 0; d < 32; ++d) { ak[d] = 0.f; av[d] = 0.f; }
    for (int q = 0; q < S; ++q) {
      const float p = expf(hd_dot32(Ql + q * 32, Kl + t * 32) * HD_SCALE - lsel[q]);
      const float dpr = hd_dot32(Dl + q * 32, Vl + t * 32);
      float m = 1.0f;
      if (dc.thresh) m = eg_dropout(1.0f, dc, seed_lo, seed_hi, (headidx + (uint32_t)q) * (uint32_t)((S + 1) & ~1) + (uint32_t)t);
      const float pd = p * m, ds = p * (dpr * m - dl[q]);
#pragma unroll
      for (int d = 0; d < 32; ++d) {
        av[d] = fmaf(pd, Dl[q * 32 + d], av[d]);
        ak[d] = fmaf(ds, Ql[q * 32 + d], ak[d]);
      }
    }
#pragma unroll
    for (int d = 0; d < 32; ++d) {
      dqkv[((long long)bk * S + t) * ld + D + h * 32 + d] = ak[d] * HD_SCALE;
      dqkv[((long long)bk * S + t) * ld + 2 * D + h * 32 + d] = av[d];
    }
  }
}

template <typename T, int SP>
void launch_fwd(const void* qkv, void* ctx, float* lse, int NB, int S, int H, int kv_shift, DropCfg dc, const eg_step_state* st,
                hipStream_t s) {
  const int nblk = (NB * H + 1) / 2;
  hipLaunchKernelGGL((attn_fwd_kernel<T, SP>), dim3(nblk), dim3(256), 2 * SP * 64, s, (const T*)qkv, (T*)ctx, lse,
                     NB, S, H, kv_shift, dc, st);
}
template <typename T, int SP>
void launch_bwd(const void* qkv, const void* ctx, const void* dctx, const float* lse, void* dqkv, int NB, int S, int H,
                int kv_shift, DropCfg dc, const eg_step_state* st, hipStream_t s) {
  const int nblk = (NB * H + 1) / 2;
  // The single sweep (each P / dS block evaluated once; key-major, see attn_bwd1_kernel) is the only 16-bit backward.  Against the two-pass
  // kernel it replaced: cfg3 step 3.87 -> 3.78 ms, cfg5 5.63 -> 5.54 ms (SP = 96); once accq stayed in registers (see the kernel; with
  // 272 B of scratch per lane it had lost at SP = 128) a5 (SP = 128) 7.38 -> 7.04 ms, a5c32 (SP = 160, 186 registers, two waves per
  // SIMD) 14.49 -> 13.84 ms.
  // Windows of up to 80 tokens (the S = 65 of the benchmark, the S = 73 of cfg5 / mm5) take the 80-row images: four workgroups per CU.
  if (SP == 96 && S == 65)           // class token + 64 positions: exact tile count, single-key tail tile
    eg_launch_lds<attn_bwd1_kernel<T, 96, 5, true, 80>, bwd1_lds(80)>(dim3(nblk), dim3(256), s, (const T*)qkv, (const T*)ctx,
                                                                      (const T*)dctx, lse, (T*)dqkv, NB, S, H, kv_shift, dc, st);
  else if (SP == 96 && S <= 80)
    eg_launch_lds<attn_bwd1_kernel<T, 96, 0, false, 80>, bwd1_lds(80)>(dim3(nblk), dim3(256), s, (const T*)qkv, (const T*)ctx,
                                                                       (const T*)dctx, lse, (T*)dqkv, NB, S, H, kv_shift, dc, st);
  else
    eg_launch_lds<attn_bwd1_kernel<T, SP, 0, false>, bwd1_lds(SP)>(dim3(nblk), dim3(256), s, (const T*)qkv, (const T*)ctx,
                                                                   (const T*)dctx, lse, (T*)dqkv, NB, S, H, kv_shift, dc, st);
}

// the 16-bit kernels' instantiation for (dtype, S): f(type tag, SP tag), SP = the tile-padded capacity 96 / 128 / HD_MAX_S
template <typename F>
void dispatch_16_sp(int dtype, int S, F&& f) {
  eg_dispatch_16(dtype, [&](auto t) {
    if (S <= 96) f(t, eg_int<96>{});
    else if (S <= 128) f(t, eg_int<128>{});
    else f(t, eg_int<HD_MAX_S>{});
  });
}

}  // namespace

extern "C" int eg_attention_fwd(const void* qkv, void* ctx, float* lse, int NB, int S, int H, int kv_shift, int dtype,
                                float drop_p, uint32_t drop_site, const eg_step_state* state, void* stream) {
  if (hd_check("eg_attention_fwd", NB, S, H, kv_shift, dtype, drop_p, state, HD_MAX_S, true)) return 1;
  EG_CHECK(qkv && ctx && lse, "eg_attention_fwd: null pointer");
  DropCfg dc = make_drop(drop_p, drop_site);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == EG_F32) {
    hipLaunchKernelGGL(attn_fwd_f32_kernel, dim3(NB * H), dim3(256), 2 * S * 32 * 4, s, (const float*)qkv, (float*)ctx, lse,
                       NB, S, H, kv_shift, dc, state);
    EG_LAUNCH_CHECK("attention_fwd_f32");
    return 0;
  }
  dispatch_16_sp(dtype, S, [&](auto t, auto sp) {
    launch_fwd<typename decltype(t)::type, decltype(sp)::value>(qkv, ctx, lse, NB, S, H, kv_shift, dc, state, s);
  });
  EG_LAUNCH_CHECK("attention_fwd");
  return 0;
}

extern "C" int eg_attention_bwd(const void* qkv, const void* ctx, const void* dctx, const float* lse, void* dqkv, int NB,
                                int S, int H, int kv_shift, int dtype, float drop_p, uint32_t drop_site,
                                const eg_step_state* state, void* stream) {
  if (hd_check("eg_attention_bwd", NB, S, H, kv_shift, dtype, drop_p, state, HD_MAX_S, true)) return 1;
  EG_CHECK(qkv && ctx && dctx && lse && dqkv, "eg_attention_bwd: null pointer");
  DropCfg dc = make_drop(drop_p, drop_site);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == EG_F32) {
    const int lds = (4 * S * 32 + 2 * S) * 4;
    static bool attr = false;
    if (!attr) {
      (void)hipFuncSetAttribute((const void*)attn_bwd_f32_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (4 * HD_MAX_S * 32 + 2 * HD_MAX_S) * 4);
      attr = true;
    }
    hipLaunchKernelGGL(attn_bwd_f32_kernel, dim3(NB * H), dim3(256), lds, s, (const float*)qkv, (const float*)ctx,
                       (const float*)dctx, lse, (float*)dqkv, NB, S, H, kv_shift, dc, state);
    EG_LAUNCH_CHECK("attention_bwd_f32");
    return 0;
  }
  dispatch_16_sp(dtype, S, [&](auto t, auto sp) {
    launch_bwd<typename decltype(t)::type, decltype(sp)::value>(qkv, ctx, dctx, lse, dqkv, NB, S, H, kv_shift, dc, state, s);
  });
  EG_LAUNCH_CHECK("attention_bwd");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Attention probabilities for the analysis hooks (eeg_metrics.py:433-452 reads them through a forward hook on the
// attention-dropout module): probs[b, h, q, k] = exp(q.k / sqrt(32) - lse[b, h, q]) in fp32.  Not on the training path.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void attn_probs_kernel(const T* __restrict__ qkv, const float* __restrict__ lse,
                                                         float* __restrict__ probs, int NB, int S, int H, int kv_shift) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Ql = (float*)smem;   // [S][33]
  float* Kl = Ql + S * 33;    // [S][33]
  const int pid = blockIdx.x, b = pid / H, h = pid % H, bk = (b + kv_shift) % NB, D = H * 32;
  const long long ld = 3ll * D;
  for (int i = threadIdx.x; i < S * 32; i += blockDim.x) {
    const int r = i >> 5, d = i & 31;
    Ql[r * 33 + d] = Elem<T>::ld(qkv + ((long long)b * S + r) * ld + h * 32 + d);
    Kl[r * 33 + d] = Elem<T>::ld(qkv + ((long long)bk * S + r) * ld + D + h * 32 + d);
  }
  __syncthreads();
  const float* lrow = lse + ((long long)b * H + h) * S;
  float* out = probs + ((long long)b * H + h) * S * S;
  for (int i = threadIdx.x; i < S * S; i += blockDim.x) {
    const int q = i / S, k = i - q * S;
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < 32; ++d) acc = fmaf(Ql[q * 33 + d], Kl[k * 33 + d], acc);
    out[i] = expf(acc * HD_SCALE - lrow[q]);
  }
}

extern "C" int eg_attention_probs(const void* qkv, const float* lse, float* probs, int NB, int S, int H, int kv_shift,
                                  int dtype, void* stream) {
  if (hd_check("eg_attention_probs", NB, S, H, kv_shift, dtype, 0.f, nullptr, HD_MAX_S, true)) return 1;
  EG_CHECK(qkv && lse && probs, "eg_attention_probs: null pointer");
  const int lds = 2 * S * 33 * 4;
  hipStream_t s = (hipStream_t)stream;
  eg_dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(attn_probs_kernel<T>, dim3(NB * H), dim3(256), lds, s, (const T*)qkv, lse, probs, NB, S, H, kv_shift);
  });
  EG_LAUNCH_CHECK("attention_probs");
  return 0;
}
