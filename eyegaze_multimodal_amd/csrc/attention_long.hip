// Multi-head attention core for long sequences (1 <= S <= 2048) on gfx950: flash-style tiling, head width DK = 32 or 64.
// Same layouts as attention.hip (qkv [NB*S, 3D], ctx [NB*S, D], lse [NB, H, S] natural-log logsumexp of the scaled scores,
// kv_shift pairs query window b with key / value window (b + kv_shift) mod NB), so the engine's buffers are shared.
//
// 16-bit forward: one workgroup per (window, head, 64-query tile); wave w owns queries 16 w .. 16 w + 15 of the tile.
//   K / V tiles of 64 keys stream through LDS, double-buffered (the next tile's global loads are issued before the current
//   tile's MFMAs and written to the other buffer after them: one barrier per tile).
//   scores^T = K_tile * Q^T (v_mfma_f32_16x16x32_{bf16,f16}: key on rows, query on lanes), online soft-max in registers
//   (running max and a per-lane partial of the running sum; lanes l, l^16, l^32, l^48 share a query), P rounded to the
//   16-bit type and fed to O^T = V^T * P^T as the B operand without an LDS round trip (the key permutation of attnhead.h).
// 16-bit backward (deterministic: every output element has exactly one writer, no atomics):
//   delta = rowsum(dO * O) into caller scratch [NB, H, S];
//   dK / dV: one workgroup per (key window, head, 64-key tile) walks every query tile of the paired query window
//            (kv_shift is a bijection between windows, so the key tile has exactly one owner);
//   dQ:      one workgroup per (query window, head, 64-query tile) walks every key tile.
// fp32 (the parity path): one thread per query / key with fmaf chains and the operation order of attention.hip's fp32
// kernels (three passes max / sum / output in the forward), K / V / Q / dO tiles streamed through LDS.
// Dropout: element e = ((w H + h) S + q) Sp2 + key in 64 bits, Sp2 = (S + 1) & ~1 (common.h: eg_hash_pair64); below 2^32
// the masks equal those of attention.hip bit for bit.  The index does not depend on the head width.
// Head width: every kernel is a template on DK.  A DK-wide head slice in LDS is DK / 32 of attnhead.h's 32-wide images, one behind
// the other ([half][64 rows][64 B]), so the header's reads serve each half as they are: a score is DK / 32 chained MFMAs over the
// halves in ascending d, an output (P V, dV, dK, dQ) is DK / 16 accumulator tiles, tile dt reading half dt >> 1, column block dt & 1.
// DK = 32 is one half, one MFMA and two tiles: the kernel this file held before it had the parameter.
#include "attnhead.h"

namespace {

constexpr int LT = 64;                    // rows per tile: queries of a workgroup, keys of a K / V tile
constexpr int IMG = LT * 64;              // bytes of one 64-row image of a 32-wide 16-bit half of a head slice

// ---- tile staging (the head image, its operand reads and the dropout index: attnhead.h) ----
// one 16-B chunk per 32-wide half of a 64-row tile per thread (256 threads: row tid >> 2, chunk tid & 3); rows >= nrows read as zero
template <int DK> struct TileChunks { u32x4 c[DK / 32]; };
template <typename T, int DK>
__device__ __forceinline__ TileChunks<DK> tile_request(const T* src, long long ld, int row0, int S, int tid) {
  const int row = row0 + (tid >> 2);
  TileChunks<DK> v;
#pragma unroll
  for (int hf = 0; hf < DK / 32; ++hf) {
    v.c[hf] = (u32x4){0u, 0u, 0u, 0u};
    if (row < S) v.c[hf] = *(const u32x4*)(src + (long long)row * ld + 32 * hf + (tid & 3) * 8);
  }
  return v;
}
template <int DK>
__device__ __forceinline__ void tile_store(char* img, const TileChunks<DK>& v, int tid) {
#pragma unroll
  for (int hf = 0; hf < DK / 32; ++hf) *(u32x4*)(img + hf * IMG + hd_img_off(tid >> 2, tid & 3)) = v.c[hf];
}
// a row's DK / 32 operand fragments from global memory (lane group g: elements 32 hf + 8 g .. + 7)
template <typename T, int DK>
__device__ __forceinline__ void frags_global(FR<T> (&f)[DK / 32], const T* row, int g, bool valid) {
#pragma unroll
  for (int hf = 0; hf < DK / 32; ++hf) f[hf] = hd_frag_global<T>(row + 32 * hf + g * 8, valid);
}
// one 16 x 16 tile of image-row . fragment products over the whole head width: DK / 32 chained MFMAs, ascending d
template <typename T, int DK>
__device__ __forceinline__ f32x4 dot_tile(const char* img, int row, int g, const FR<T> (&f)[DK / 32]) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int hf = 0; hf < DK / 32; ++hf) acc = H16<T>::mfma(hd_frag_row<T>(img + hf * IMG, row, g), f[hf], acc);
  return acc;
}
// the transposed operand of output tile dt (columns 16 dt .. 16 dt + 15 of the head slice)
template <typename T>
__device__ __forceinline__ FR<T> out_frag_tr(const char* img, int rbase, int dt, int lane) {
  return hd_frag_tr<T>(img + (dt >> 1) * IMG, rbase, dt & 1, lane);
}

// (window, head, tile) of a workgroup: tiles fastest, so the workgroups of one head run side by side and share its K / V in L2
struct TileIdx { int w, h, t; };
__device__ __forceinline__ TileIdx tile_idx(int ntile, int H) {
  const int t = blockIdx.x % ntile, pid = blockIdx.x / ntile;
  return {pid / H, pid % H, t};
}

// ------------------------------------------------------------------------------------------------
// 16-bit forward
// ------------------------------------------------------------------------------------------------
template <typename T, int DK>
__global__ __launch_bounds__(256) void attn_long_fwd_kernel(const T* __restrict__ qkv, T* __restrict__ ctx, float* __restrict__ lse,
                                                            int NB, int S, int H, int kv_shift, DropCfg dc, const eg_step_state* st) {
  constexpr int ND = DK / 16;                                     // output tiles
  constexpr float SCALE = hd_scale<DK>();
  __shared__ __attribute__((aligned(16))) char sm[2][2][DK / 32 * IMG];    // [buffer][K, V]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
  const int ntile = (S + LT - 1) / LT;
  const TileIdx ti = tile_idx(ntile, H);
  const int b = ti.w, h = ti.h, bk = (b + kv_shift) % NB, D = H * DK;
  const long long ld = 3ll * D;
  const T* qbase = qkv + (long long)b * S * ld + h * DK;
  const T* kbase = qkv + (long long)bk * S * ld + D + h * DK;
  const T* vbase = kbase + D;
  const int q = ti.t * LT + wave * 16 + l15;
  TileChunks<DK> rk = tile_request<T, DK>(kbase, ld, 0, S, tid), rv = tile_request<T, DK>(vbase, ld, 0, S, tid);
  FR<T> qf[DK / 32];
  frags_global<T, DK>(qf, qbase + (long long)q * ld, g, q < S);
  uint32_t seed_lo = 0, seed_hi = 0;
  if (dc.thresh) { seed_lo = st->seed_lo; seed_hi = st->seed_hi; }
  const uint64_t rowe = (uint64_t)(((long long)b * H + h) * S + q) * (uint64_t)((S + 1) & ~1);
  tile_store<DK>(sm[0][0], rk, tid);
  tile_store<DK>(sm[0][1], rv, tid);
  __syncthreads();
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 o[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) o[dt] = zero4;
  float m = -INFINITY, l = 0.f;                 // running max (shared by the query's 4 lanes), the lane's partial running sum
  for (int t = 0; t < ntile; ++t) {
    const int cur = t & 1, kv0 = t * LT;
    const bool more = t + 1 < ntile;
    if (more) {
      rk = tile_request<T, DK>(kbase, ld, kv0 + LT, S, tid);
      rv = tile_request<T, DK>(vbase, ld, kv0 + LT, S, tid);
    }
    const char* kimg = sm[cur][0];
    const char* vimg = sm[cur][1];
    const bool full = kv0 + LT <= S;           // workgroup-uniform: only the last tile masks keys
    f32x4 s[4];
    float tmax = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      s[kt] = dot_tile<T, DK>(kimg, kt * 16 + l15, g, qf);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = (full || kv0 + kt * 16 + 4 * g + r < S) ? s[kt][r] * SCALE : -INFINITY;
        s[kt][r] = v;
        tmax = fmaxf(tmax, v);
      }
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float mnew = fmaxf(m, tmax);          // finite: every tile holds at least one valid key
    const float alpha = __expf(m - mnew);       // 0 at the first tile (m = -inf)
    m = mnew;
    float psum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __expf(s[kt][r] - m);
        s[kt][r] = p;
        psum += p;
      }
    l = l * alpha + psum;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) o[dt] *= alpha;
    if (dc.thresh) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        float pv[4] = {s[kt][0], s[kt][1], s[kt][2], s[kt][3]};
        eg_dropout_run64<4>(pv, dc, seed_lo, seed_hi, rowe + (uint64_t)(kv0 + kt * 16 + 4 * g));
#pragma unroll
        for (int r = 0; r < 4; ++r) s[kt][r] = pv[r];
      }
    }
#pragma unroll
    for (int kp = 0; kp < 2; ++kp) {
      const FR<T> pf = hd_pack_frag<T>(s[2 * kp], s[2 * kp + 1]);
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) o[dt] = H16<T>::mfma(out_frag_tr<T>(vimg, 32 * kp, dt, lane), pf, o[dt]);
    }
    if (more) {
      tile_store<DK>(sm[cur ^ 1][0], rk, tid);
      tile_store<DK>(sm[cur ^ 1][1], rv, tid);
    }
    __syncthreads();
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (q < S) {
    if (g == 0) lse[((long long)b * H + h) * S + q] = m + __logf(l);
    const float inv = 1.0f / l;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
      float v[4] = {o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv};
      store4(ctx + ((long long)b * S + q) * D + h * DK + 16 * dt + 4 * g, v);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// delta = rowsum(dO * O) per (window, head, query), into [NB, H, S] (16-bit and fp32)
// ------------------------------------------------------------------------------------------------
template <typename T, int DK>
__global__ __launch_bounds__(256) void attn_long_delta_kernel(const T* __restrict__ ctx, const T* __restrict__ dctx,
                                                              float* __restrict__ delta, long long n, int S, int H) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int q = (int)(i % S);
  const long long wh = i / S;
  const int h = (int)(wh % H);
  const long long w = wh / H;
  const long long off = (w * S + q) * (long long)(H * DK) + h * DK;
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < DK / 8; ++c) {
    float a[8], o[8];
    load8(dctx + off + 8 * c, a);
    load8(ctx + off + 8 * c, o);
#pragma unroll
    for (int e = 0; e < 8; ++e) s = fmaf(a[e], o[e], s);
  }
  delta[i] = s;
}

// ------------------------------------------------------------------------------------------------
// 16-bit dK / dV: one workgroup per (key window, head, 64-key tile); query rows / key lanes
// ------------------------------------------------------------------------------------------------
template <typename T, int DK>
__global__ __launch_bounds__(256) void attn_long_dkdv_kernel(const T* __restrict__ qkv, const T* __restrict__ dctx,
                                                             const float* __restrict__ lse, const float* __restrict__ delta,
                                                             T* __restrict__ dqkv, int NB, int S, int H, int kv_shift, DropCfg dc,
                                                             const eg_step_state* st) {
  constexpr int ND = DK / 16;
  constexpr float SCALE = hd_scale<DK>();
  __shared__ __attribute__((aligned(16))) char sm[2][2][DK / 32 * IMG];    // [buffer][Q, dO]
  __shared__ __attribute__((aligned(16))) float rows[2][2][LT];  // [buffer][lse, delta]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
  const int ntile = (S + LT - 1) / LT;
  const TileIdx ti = tile_idx(ntile, H);
  const int bk = ti.w, h = ti.h, b = (bk - kv_shift + NB) % NB, D = H * DK;   // the one query window that reads key window bk
  const long long ld = 3ll * D;
  const T* qbase = qkv + (long long)b * S * ld + h * DK;
  const T* kbase = qkv + (long long)bk * S * ld + D + h * DK;
  const T* vbase = kbase + D;
  const T* dobase = dctx + (long long)b * S * D + h * DK;
  const float* lrow = lse + ((long long)b * H + h) * S;
  const float* drow = delta + ((long long)b * H + h) * S;
  const int key = ti.t * LT + wave * 16 + l15;
  // this thread's share of a query tile: its chunks of Q and of dO, and (threads 0..127) one lse / delta value
  auto request = [&](int q0, TileChunks<DK>& rq, TileChunks<DK>& rd, float& rl) {
    rq = tile_request<T, DK>(qbase, ld, q0, S, tid);
    rd = tile_request<T, DK>(dobase, D, q0, S, tid);
    rl = 0.f;
    const int qr = q0 + (tid & 63);
    if (tid < 128 && qr < S) rl = tid < 64 ? lrow[qr] : drow[qr];
  };
  auto store = [&](int buf, const TileChunks<DK>& rq, const TileChunks<DK>& rd, float rl) {
    tile_store<DK>(sm[buf][0], rq, tid);
    tile_store<DK>(sm[buf][1], rd, tid);
    if (tid < 128) rows[buf][tid >> 6][tid & 63] = rl;
  };
  TileChunks<DK> rq, rd;
  float rl;
  request(0, rq, rd, rl);
  FR<T> kfr[DK / 32], vfr[DK / 32];
  frags_global<T, DK>(kfr, kbase + (long long)key * ld, g, key < S);
  frags_global<T, DK>(vfr, vbase + (long long)key * ld, g, key < S);
  uint32_t seed_lo = 0, seed_hi = 0;
  if (dc.thresh) { seed_lo = st->seed_lo; seed_hi = st->seed_hi; }
  const uint64_t Sp2 = (uint64_t)((S + 1) & ~1);
  const long long headrow = ((long long)b * H + h) * S;
  store(0, rq, rd, rl);
  __syncthreads();
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 dk[ND], dv[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) dk[dt] = dv[dt] = zero4;
  for (int t = 0; t < ntile; ++t) {
    const int cur = t & 1, q0 = t * LT;
    const bool more = t + 1 < ntile;
    if (more) request(q0 + LT, rq, rd, rl);
    const char* qimg = sm[cur][0];
    const char* doimg = sm[cur][1];
    const float* lsel = rows[cur][0];
    const float* dl = rows[cur][1];
#pragma unroll
    for (int qp = 0; qp < 2; ++qp) {
      f32x4 pd2[2], ds2[2];
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int r16 = 32 * qp + 16 * h2;                 // first query of the 16-row block, within the tile
        const f32x4 s = dot_tile<T, DK>(qimg, r16 + l15, g, kfr);
        const f32x4 dp = dot_tile<T, DK>(doimg, r16 + l15, g, vfr);
        const f32x4 l4 = *(const f32x4*)(lsel + r16 + 4 * g);
        const f32x4 d4 = *(const f32x4*)(dl + r16 + 4 * g);
        // One hash serves the elements (q, key) and (q, key ^ 1), which sit in neighbouring lanes: a lane hashes two of its
        // four query rows (even keys rows 0-1, odd keys rows 2-3) and takes the other two from lane ^ 1.
        uint32_t hh[4] = {0u, 0u, 0u, 0u};
        if (dc.thresh) {
          const uint32_t odd = (uint32_t)key & 1u;
          const uint64_t ea = (uint64_t)(headrow + q0 + r16 + 4 * g + 2 * (int)odd) * Sp2 + (uint64_t)key;
          const uint32_t ha = eg_hash_pair64(seed_lo, seed_hi, dc.site, ea >> 1);
          const uint32_t hb = eg_hash_pair64(seed_lo, seed_hi, dc.site, (ea + Sp2) >> 1);
          const uint32_t pa = (uint32_t)__shfl_xor((int)ha, 1, 64), pb = (uint32_t)__shfl_xor((int)hb, 1, 64);
          hh[0] = odd ? pa : ha; hh[1] = odd ? pb : hb;
          hh[2] = odd ? ha : pa; hh[3] = odd ? hb : pb;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qq = q0 + r16 + 4 * g + r;
          const float p = (key < S && qq < S) ? __expf(s[r] * SCALE - l4[r]) : 0.f;
          float mk = 1.0f;
          if (dc.thresh) {
            const uint32_t half = ((uint32_t)key & 1u) ? (hh[r] >> 16) : (hh[r] & 0xFFFFu);
            mk = half >= dc.thresh ? dc.scale : 0.0f;
          }
          pd2[h2][r] = p * mk;
          ds2[h2][r] = p * (dp[r] * mk - d4[r]);
        }
      }
      const FR<T> pdf = hd_pack_frag<T>(pd2[0], pd2[1]);
      const FR<T> dsf = hd_pack_frag<T>(ds2[0], ds2[1]);
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) {
        dv[dt] = H16<T>::mfma(out_frag_tr<T>(doimg, 32 * qp, dt, lane), pdf, dv[dt]);
        dk[dt] = H16<T>::mfma(out_frag_tr<T>(qimg, 32 * qp, dt, lane), dsf, dk[dt]);
      }
    }
    if (more) store(cur ^ 1, rq, rd, rl);
    __syncthreads();
  }
  if (key < S) {
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
      float a[4] = {dk[dt][0] * SCALE, dk[dt][1] * SCALE, dk[dt][2] * SCALE, dk[dt][3] * SCALE};
      float c[4] = {dv[dt][0], dv[dt][1], dv[dt][2], dv[dt][3]};
      T* row = dqkv + ((long long)bk * S + key) * ld + h * DK + 16 * dt + 4 * g;
      store4(row + D, a);
      store4(row + 2 * D, c);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// 16-bit dQ: one workgroup per (query window, head, 64-query tile); key rows / query lanes
// ------------------------------------------------------------------------------------------------
template <typename T, int DK>
__global__ __launch_bounds__(256) void attn_long_dq_kernel(const T* __restrict__ qkv, const T* __restrict__ dctx,
                                                           const float* __restrict__ lse, const float* __restrict__ delta,
                                                           T* __restrict__ dqkv, int NB, int S, int H, int kv_shift, DropCfg dc,
                                                           const eg_step_state* st) {
  constexpr int ND = DK / 16;
  constexpr float SCALE = hd_scale<DK>();
  __shared__ __attribute__((aligned(16))) char sm[2][2][DK / 32 * IMG];    // [buffer][K, V]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
  const int ntile = (S + LT - 1) / LT;
  const TileIdx ti = tile_idx(ntile, H);
  const int b = ti.w, h = ti.h, bk = (b + kv_shift) % NB, D = H * DK;
  const long long ld = 3ll * D;
  const T* qbase = qkv + (long long)b * S * ld + h * DK;
  const T* kbase = qkv + (long long)bk * S * ld + D + h * DK;
  const T* vbase = kbase + D;
  const T* dobase = dctx + (long long)b * S * D + h * DK;
  const int q = ti.t * LT + wave * 16 + l15;
  TileChunks<DK> rk = tile_request<T, DK>(kbase, ld, 0, S, tid), rv = tile_request<T, DK>(vbase, ld, 0, S, tid);
  FR<T> qf[DK / 32], dof[DK / 32];
  frags_global<T, DK>(qf, qbase + (long long)q * ld, g, q < S);
  frags_global<T, DK>(dof, dobase + (long long)q * D, g, q < S);
  const long long hq = ((long long)b * H + h) * S + q;
  const float lq = q < S ? lse[hq] : 0.f, dq = q < S ? delta[hq] : 0.f;
  uint32_t seed_lo = 0, seed_hi = 0;
  if (dc.thresh) { seed_lo = st->seed_lo; seed_hi = st->seed_hi; }
  const uint64_t rowe = (uint64_t)hq * (uint64_t)((S + 1) & ~1);
  tile_store<DK>(sm[0][0], rk, tid);
  tile_store<DK>(sm[0][1], rv, tid);
  __syncthreads();
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) acc[dt] = zero4;
  for (int t = 0; t < ntile; ++t) {
    const int cur = t & 1, kv0 = t * LT;
    const bool more = t + 1 < ntile;
    if (more) {
      rk = tile_request<T, DK>(kbase, ld, kv0 + LT, S, tid);
      rv = tile_request<T, DK>(vbase, ld, kv0 + LT, S, tid);
    }
    const char* kimg = sm[cur][0];
    const char* vimg = sm[cur][1];
    f32x4 ds[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const f32x4 sT = dot_tile<T, DK>(kimg, kt * 16 + l15, g, qf);
      const f32x4 dpT = dot_tile<T, DK>(vimg, kt * 16 + l15, g, dof);
      float dpv[4] = {dpT[0], dpT[1], dpT[2], dpT[3]};
      eg_dropout_run64<4>(dpv, dc, seed_lo, seed_hi, rowe + (uint64_t)(kv0 + kt * 16 + 4 * g));
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kv0 + kt * 16 + 4 * g + r;
        const float p = key < S ? __expf(sT[r] * SCALE - lq) : 0.f;
        ds[kt][r] = p * (dpv[r] - dq);
      }
    }
#pragma unroll
    for (int kp = 0; kp < 2; ++kp) {
      const FR<T> dsf = hd_pack_frag<T>(ds[2 * kp], ds[2 * kp + 1]);
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) acc[dt] = H16<T>::mfma(out_frag_tr<T>(kimg, 32 * kp, dt, lane), dsf, acc[dt]);
    }
    if (more) {
      tile_store<DK>(sm[cur ^ 1][0], rk, tid);
      tile_store<DK>(sm[cur ^ 1][1], rv, tid);
    }
    __syncthreads();
  }
  if (q < S) {
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
      float v[4] = {acc[dt][0] * SCALE, acc[dt][1] * SCALE, acc[dt][2] * SCALE, acc[dt][3] * SCALE};
      store4(dqkv + ((long long)b * S + q) * ld + h * DK + 16 * dt + 4 * g, v);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// fp32: one thread per query (forward, dQ) or key (dK, dV), 128 threads per workgroup, 64-row tiles of the other side in LDS.
// The arithmetic of every output element is that of attention.hip's fp32 kernels, in the same order (DK = 64: the same chains,
// twice as long).
// ------------------------------------------------------------------------------------------------
constexpr int F32_THREADS = 128;

// rows [row0, row0 + 64) of a DK-wide fp32 head slice into dst [64][DK]; rows >= S read as zero
template <int DK>
__device__ __forceinline__ void f32_tile_load(float* dst, const float* src, long long ld, int row0, int S) {
  for (int i = threadIdx.x; i < LT * (DK / 4); i += F32_THREADS) {
    const int r = i / (DK / 4), c = i % (DK / 4);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row0 + r < S) v = *(const f32x4*)(src + (long long)(row0 + r) * ld + 4 * c);
    *(f32x4*)(dst + r * DK + 4 * c) = v;
  }
}

template <int DK>
__global__ __launch_bounds__(F32_THREADS) void attn_long_fwd_f32_kernel(const float* __restrict__ qkv, float* __restrict__ ctx,
                                                                        float* __restrict__ lse, int NB, int S, int H, int kv_shift,
                                                                        DropCfg dc, const eg_step_state* st) {
  constexpr float SCALE = hd_scale<DK>();
  __shared__ __attribute__((aligned(16))) float Kl[LT * DK];
  __shared__ __attribute__((aligned(16))) float Vl[LT * DK];
  const int ntile = (S + F32_THREADS - 1) / F32_THREADS, nkv = (S + LT - 1) / LT;
  const TileIdx ti = tile_idx(ntile, H);
  const int b = ti.w, h = ti.h, bk = (b + kv_shift) % NB, D = H * DK;
  const long long ld = 3ll * D;
  const float* kbase = qkv + (long long)bk * S * ld + D + h * DK;
  const float* vbase = kbase + D;
  const int q = ti.t * F32_THREADS + threadIdx.x;
  const bool valid = q < S;
  float qv[DK], o[DK];
#pragma unroll
  for (int d = 0; d < DK; ++d) { qv[d] = valid ? qkv[((long long)b * S + q) * ld + h * DK + d] : 0.f; o[d] = 0.f; }
  // pass 1: max, pass 2: sum, pass 3: P V -- as attn_fwd_f32_kernel
  float mx = -INFINITY, sum = 0.f, inv = 0.f;
  uint32_t seed_lo = 0, seed_hi = 0;
  if (dc.thresh) { seed_lo = st->seed_lo; seed_hi = st->seed_hi; }
  const uint64_t rowe = (uint64_t)(((long long)b * H + h) * S + q) * (uint64_t)((S + 1) & ~1);
  for (int pass = 0; pass < 3; ++pass) {
    for (int t = 0; t < nkv; ++t) {
      const int k0 = t * LT, nk = min(LT, S - k0);
      __syncthreads();
      f32_tile_load<DK>(Kl, kbase, ld, k0, S);
      if (pass == 2) f32_tile_load<DK>(Vl, vbase, ld, k0, S);
      __syncthreads();
      if (pass == 0) {
        for (int k = 0; k < nk; ++k) mx = fmaxf(mx, hd_dot<DK>(qv, Kl + k * DK) * SCALE);
      } else if (pass == 1) {
        for (int k = 0; k < nk; ++k) sum += expf(hd_dot<DK>(qv, Kl + k * DK) * SCALE - mx);
      } else {
        for (int k = 0; k < nk; ++k) {
          float p = expf(hd_dot<DK>(qv, Kl + k * DK) * SCALE - mx) * inv;
          if (dc.thresh) p = eg_dropout64(p, dc, seed_lo, seed_hi, rowe + (uint64_t)(k0 + k));
#pragma unroll
          for (int d = 0; d < DK; ++d) o[d] = fmaf(p, Vl[k * DK + d], o[d]);
        }
      }
    }
    if (pass == 1) inv = 1.0f / sum;
  }
  if (!valid) return;
  lse[((long long)b * H + h) * S + q] = mx + logf(sum);
#pragma unroll
  for (int d = 0; d < DK; d += 4) *(f32x4*)(ctx + ((long long)b * S + q) * D + h * DK + d) = (f32x4){o[d], o[d + 1], o[d + 2], o[d + 3]};
}

template <int DK>
__global__ __launch_bounds__(F32_THREADS) void attn_long_dq_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ dctx,
                                                                       const float* __restrict__ lse, const float* __restrict__ delta,
                                                                       float* __restrict__ dqkv, int NB, int S, int H, int kv_shift,
                                                                       DropCfg dc, const eg_step_state* st) {
  constexpr float SCALE = hd_scale<DK>();
  __shared__ __attribute__((aligned(16))) float Kl[LT * DK];
  __shared__ __attribute__((aligned(16))) float Vl[LT * DK];
  const int ntile = (S + F32_THREADS - 1) / F32_THREADS, nkv = (S + LT - 1) / LT;
  const TileIdx ti = tile_idx(ntile, H);
  const int b = ti.w, h = ti.h, bk = (b + kv_shift) % NB, D = H * DK;
  const long long ld = 3ll * D;
  const float* kbase = qkv + (long long)bk * S * ld + D + h * DK;
  const float* vbase = kbase + D;
  const int t_ = ti.t * F32_THREADS + threadIdx.x;
  const bool valid = t_ < S;
  const long long hq = ((long long)b * H + h) * S + t_;
  float qv[DK], dov[DK], acc[DK];
#pragma unroll
  for (int d = 0; d < DK; ++d) {
    qv[d] = valid ? qkv[((long long)b * S + t_) * ld + h * DK + d] : 0.f;
    dov[d] = valid ? dctx[((long long)b * S + t_) * D + h * DK + d] : 0.f;
    acc[d] = 0.f;
  }
  const float lq = valid ? lse[hq] : 0.f, dq = valid ? delta[hq] : 0.f;
  uint32_t seed_lo = 0, seed_hi = 0;
  if (dc.thresh) { seed_lo = st->seed_lo; seed_hi = st->seed_hi; }
  const uint64_t rowe = (uint64_t)hq * (uint64_t)((S + 1) & ~1);
  for (int t = 0; t < nkv; ++t) {
    const int k0 = t * LT, nk = min(LT, S - k0);
    __syncthreads();
    f32_tile_load<DK>(Kl, kbase, ld, k0, S);
    f32_tile_load<DK>(Vl, vbase, ld, k0, S);
    __syncthreads();
    for (int k = 0; k < nk; ++k) {
      const float p = expf(hd_dot<DK>(qv, Kl + k * DK) * SCALE - lq);
      float dp = hd_dot<DK>(dov, Vl + k * DK);
      if (dc.thresh) dp = eg_dropout64(dp, dc, seed_lo, seed_hi, rowe + (uint64_t)(k0 + k));
      const float ds = p * (dp - dq);
#pragma unroll
      for (int d = 0; d < DK; ++d) acc[d] = fmaf(ds, Kl[k * DK + d], acc[d]);
    }
  }
  if (!valid) return;
#pragma unroll
  for (int d = 0; d < DK; ++d) dqkv[((long long)b * S + t_) * ld + h * DK + d] = acc[d] * SCALE;
}

template <int DK>
__global__ __launch_bounds__(F32_THREADS) void attn_long_dkdv_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ dctx,
                                                                         const float* __restrict__ lse, const float* __restrict__ delta,
                                                                         float* __restrict__ dqkv, int NB, int S, int H, int kv_shift,
                                                                         DropCfg dc, const eg_step_state* st) {
  constexpr float SCALE = hd_scale<DK>();
  __shared__ __attribute__((aligned(16))) float Ql[LT * DK];
  __shared__ __attribute__((aligned(16))) float Dl[LT * DK];
  __shared__ float lsel[LT], dl[LT];
  const int ntile = (S + F32_THREADS - 1) / F32_THREADS, nq = (S + LT - 1) / LT;
  const TileIdx ti = tile_idx(ntile, H);
  const int bk = ti.w, h = ti.h, b = (bk - kv_shift + NB) % NB, D = H * DK;
  const long long ld = 3ll * D;
  const float* qbase = qkv + (long long)b * S * ld + h * DK;
  const float* dobase = dctx + (long long)b * S * D + h * DK;
  const float* lrow = lse + ((long long)b * H + h) * S;
  const float* drow = delta + ((long long)b * H + h) * S;
  const int t_ = ti.t * F32_THREADS + threadIdx.x;       // this thread's key
  const bool valid = t_ < S;
  float kv[DK], vv[DK], ak[DK], av[DK];
#pragma unroll
  for (int d = 0; d < DK; ++d) {
    kv[d] = valid ? qkv[((long long)bk * S + t_) * ld + D + h * DK + d] : 0.f;
    vv[d] = valid ? qkv[((long long)bk * S + t_) * ld + 2 * D + h * DK + d] : 0.f;
    ak[d] = 0.f;
    av[d] = 0.f;
  }
  uint32_t seed_lo = 0, seed_hi = 0;
  if (dc.thresh) { seed_lo = st->seed_lo; seed_hi = st->seed_hi; }
  const long long headrow = ((long long)b * H + h) * S;
  const uint64_t Sp2 = (uint64_t)((S + 1) & ~1);
  for (int t = 0; t < nq; ++t) {
    const int q0 = t * LT, nqr = min(LT, S - q0);
    __syncthreads();
    f32_tile_load<DK>(Ql, qbase, ld, q0, S);
    f32_tile_load<DK>(Dl, dobase, D, q0, S);
    if (threadIdx.x < LT) {
      const int qr = q0 + threadIdx.x;
      lsel[threadIdx.x] = qr < S ? lrow[qr] : 0.f;
      dl[threadIdx.x] = qr < S ? drow[qr] : 0.f;
    }
    __syncthreads();
    for (int i = 0; i < nqr; ++i) {
      const float p = expf(hd_dot<DK>(Ql + i * DK, kv) * SCALE - lsel[i]);
      const float dpr = hd_dot<DK>(Dl + i * DK, vv);
      float mk = 1.0f;
      if (dc.thresh) mk = eg_dropout64(1.0f, dc, seed_lo, seed_hi, (uint64_t)(headrow + q0 + i) * Sp2 + (uint64_t)t_);
      const float pd = p * mk, ds = p * (dpr * mk - dl[i]);
#pragma unroll
      for (int d = 0; d < DK; ++d) {
        av[d] = fmaf(pd, Dl[i * DK + d], av[d]);
        ak[d] = fmaf(ds, Ql[i * DK + d], ak[d]);
      }
    }
  }
  if (!valid) return;
#pragma unroll
  for (int d = 0; d < DK; ++d) {
    dqkv[((long long)bk * S + t_) * ld + D + h * DK + d] = ak[d] * SCALE;
    dqkv[((long long)bk * S + t_) * ld + 2 * D + h * DK + d] = av[d];
  }
}

// ------------------------------------------------------------------------------------------------
// Attention probabilities for the analysis hooks: probs[b, h, q, k] = exp(q.k / sqrt(DK) - lse[b, h, q]) in fp32, the arithmetic
// of attn_probs_kernel.  One workgroup per (window, head, 16 query rows); a thread per key, no LDS sized by S; 64-bit offsets.
// ------------------------------------------------------------------------------------------------
constexpr int PROBS_ROWS = 16;

template <typename T, int DK>
__global__ __launch_bounds__(256) void attn_long_probs_kernel(const T* __restrict__ qkv, const float* __restrict__ lse,
                                                              float* __restrict__ probs, int NB, int S, int H, int kv_shift) {
  constexpr float SCALE = hd_scale<DK>();
  __shared__ float Ql[PROBS_ROWS][DK];
  __shared__ float lq[PROBS_ROWS];
  const int ntile = (S + PROBS_ROWS - 1) / PROBS_ROWS;
  const TileIdx ti = tile_idx(ntile, H);
  const int b = ti.w, h = ti.h, bk = (b + kv_shift) % NB, D = H * DK;
  const long long ld = 3ll * D;
  const int q0 = ti.t * PROBS_ROWS, nq = min(PROBS_ROWS, S - q0);
  for (int i = threadIdx.x; i < PROBS_ROWS * DK; i += 256) {
    const int r = i / DK, d = i % DK;
    Ql[r][d] = r < nq ? Elem<T>::ld(qkv + ((long long)b * S + q0 + r) * ld + h * DK + d) : 0.f;
  }
  if (threadIdx.x < PROBS_ROWS) lq[threadIdx.x] = (int)threadIdx.x < nq ? lse[((long long)b * H + h) * S + q0 + threadIdx.x] : 0.f;
  __syncthreads();
  float* out = probs + (((long long)b * H + h) * S + q0) * (long long)S;
  for (int k = threadIdx.x; k < S; k += 256) {
    float kv[DK];
#pragma unroll
    for (int d = 0; d < DK; ++d) kv[d] = Elem<T>::ld(qkv + ((long long)bk * S + k) * ld + D + h * DK + d);
    for (int r = 0; r < nq; ++r) {
      float acc = 0.f;
#pragma unroll
      for (int d = 0; d < DK; ++d) acc = fmaf(Ql[r][d], kv[d], acc);
      out[(long long)r * S + k] = expf(acc * SCALE - lq[r]);
    }
  }
}

// ---- host: the three launch sequences, each stated once for both families of entry points ----
// eg_attention_long_* are head_dim = 32; eg_attention_dk_* pass theirs on.  `who` is the entry point's name.
int attn_long_check(const char* who, int NB, int S, int H, int head_dim, int kv_shift, int dtype, float p, const void* st) {
  if (hd_check(who, NB, S, H, kv_shift, dtype, p, st, EG_ATTN_LONG_MAX_S, false)) return 1;
  EG_CHECK(head_dim == 32 || head_dim == 64, "%s: head_dim=%d: the kernels are built for head widths 32 and 64", who, head_dim);
  // one workgroup per (window, head, 16-row tile) at most: the grid's x dimension
  EG_CHECK((long long)NB * H * ((S + PROBS_ROWS - 1) / PROBS_ROWS) < (1ll << 31), "%s: NB*H=%lld heads exceed the grid", who,
           (long long)NB * H);
  return 0;
}

inline int long_blocks(int NB, int H, int S, int rows) { return NB * H * ((S + rows - 1) / rows); }

// f(eg_int<32 or 64>): the head width as a compile-time size
template <typename F>
inline void dispatch_dk(int head_dim, F&& f) {
  if (head_dim == 64) f(eg_int<64>{});
  else f(eg_int<32>{});
}

int long_fwd(const char* who, const void* qkv, void* ctx, float* lse, int NB, int S, int H, int head_dim, int kv_shift, int dtype,
             float drop_p, uint32_t drop_site, const eg_step_state* state, void* stream) {
  if (attn_long_check(who, NB, S, H, head_dim, kv_shift, dtype, drop_p, state)) return 1;
  EG_CHECK(qkv && ctx && lse, "%s: null pointer", who);
  const DropCfg dc = make_drop(drop_p, drop_site);
  hipStream_t s = (hipStream_t)stream;
  dispatch_dk(head_dim, [&](auto dk) {
    constexpr int DK = decltype(dk)::value;
    if (dtype == EG_F32)
      hipLaunchKernelGGL(attn_long_fwd_f32_kernel<DK>, dim3(long_blocks(NB, H, S, F32_THREADS)), dim3(F32_THREADS), 0, s,
                         (const float*)qkv, (float*)ctx, lse, NB, S, H, kv_shift, dc, state);
    else
      eg_dispatch_16(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((attn_long_fwd_kernel<T, DK>), dim3(long_blocks(NB, H, S, LT)), dim3(256), 0, s, (const T*)qkv, (T*)ctx, lse,
                           NB, S, H, kv_shift, dc, state);
      });
  });
  EG_LAUNCH_CHECK(who + 3);
  return 0;
}

int long_bwd(const char* who, const void* qkv, const void* ctx, const void* dctx, const float* lse, void* dqkv, int NB, int S, int H,
             int head_dim, int kv_shift, int dtype, float drop_p, uint32_t drop_site, const eg_step_state* state, float* scratch,
             int64_t scratch_elems, void* stream) {
  if (attn_long_check(who, NB, S, H, head_dim, kv_shift, dtype, drop_p, state)) return 1;
  EG_CHECK(qkv && ctx && dctx && lse && dqkv && scratch, "%s: null pointer", who);
  const long long n = (long long)NB * H * S;
  EG_CHECK(scratch_elems >= n, "%s: scratch holds %lld floats, NB*H*S = %lld are needed", who, (long long)scratch_elems, n);
  const DropCfg dc = make_drop(drop_p, drop_site);
  hipStream_t s = (hipStream_t)stream;
  const dim3 dgrid((unsigned)((n + 255) / 256));
  const float* delta = scratch;
  // delta -> dK / dV -> dQ
  dispatch_dk(head_dim, [&](auto dk) {
    constexpr int DK = decltype(dk)::value;
    if (dtype == EG_F32) {
      const dim3 grid(long_blocks(NB, H, S, F32_THREADS)), block(F32_THREADS);
      const float *q = (const float*)qkv, *d = (const float*)dctx;
      hipLaunchKernelGGL((attn_long_delta_kernel<float, DK>), dgrid, dim3(256), 0, s, (const float*)ctx, d, scratch, n, S, H);
      hipLaunchKernelGGL(attn_long_dkdv_f32_kernel<DK>, grid, block, 0, s, q, d, lse, delta, (float*)dqkv, NB, S, H, kv_shift, dc,
                         state);
      hipLaunchKernelGGL(attn_long_dq_f32_kernel<DK>, grid, block, 0, s, q, d, lse, delta, (float*)dqkv, NB, S, H, kv_shift, dc, state);
    } else {
      eg_dispatch_16(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        const dim3 grid(long_blocks(NB, H, S, LT)), block(256);
        const T *q = (const T*)qkv, *d = (const T*)dctx;
        hipLaunchKernelGGL((attn_long_delta_kernel<T, DK>), dgrid, dim3(256), 0, s, (const T*)ctx, d, scratch, n, S, H);
        hipLaunchKernelGGL((attn_long_dkdv_kernel<T, DK>), grid, block, 0, s, q, d, lse, delta, (T*)dqkv, NB, S, H, kv_shift, dc, state);
        hipLaunchKernelGGL((attn_long_dq_kernel<T, DK>), grid, block, 0, s, q, d, lse, delta, (T*)dqkv, NB, S, H, kv_shift, dc, state);
      });
    }
  });
  EG_LAUNCH_CHECK(who + 3);
  return 0;
}

int long_probs(const char* who, const void* qkv, const float* lse, float* probs, int NB, int S, int H, int head_dim, int kv_shift,
               int dtype, void* stream) {
  if (attn_long_check(who, NB, S, H, head_dim, kv_shift, dtype, 0.f, nullptr)) return 1;
  EG_CHECK(qkv && lse && probs, "%s: null pointer", who);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(long_blocks(NB, H, S, PROBS_ROWS));
  dispatch_dk(head_dim, [&](auto dk) {
    constexpr int DK = decltype(dk)::value;
    eg_dispatch_dtype(dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      hipLaunchKernelGGL((attn_long_probs_kernel<T, DK>), grid, dim3(256), 0, s, (const T*)qkv, lse, probs, NB, S, H, kv_shift);
    });
  });
  EG_LAUNCH_CHECK(who + 3);
  return 0;
}

}  // namespace

extern "C" int eg_attention_long_fwd(const void* qkv, void* ctx, float* lse, int NB, int S, int H, int kv_shift, int dtype,
                                     float drop_p, uint32_t drop_site, const eg_step_state* state, void* stream) {
  return long_fwd("eg_attention_long_fwd", qkv, ctx, lse, NB, S, H, 32, kv_shift, dtype, drop_p, drop_site, state, stream);
}

extern "C" int eg_attention_long_bwd(const void* qkv, const void* ctx, const void* dctx, const float* lse, void* dqkv, int NB,
                                     int S, int H, int kv_shift, int dtype, float drop_p, uint32_t drop_site,
                                     const eg_step_state* state, float* scratch, int64_t scratch_elems, void* stream) {
  return long_bwd("eg_attention_long_bwd", qkv, ctx, dctx, lse, dqkv, NB, S, H, 32, kv_shift, dtype, drop_p, drop_site, state, scratch,
                  scratch_elems, stream);
}

extern "C" int eg_attention_long_probs(const void* qkv, const float* lse, float* probs, int NB, int S, int H, int kv_shift,
                                       int dtype, void* stream) {
  return long_probs("eg_attention_long_probs", qkv, lse, probs, NB, S, H, 32, kv_shift, dtype, stream);
}

extern "C" int eg_attention_dk_fwd(const void* qkv, void* ctx, float* lse, int NB, int S, int H, int head_dim, int kv_shift, int dtype,
                                   float drop_p, uint32_t drop_site, const eg_step_state* state, void* stream) {
  return long_fwd("eg_attention_dk_fwd", qkv, ctx, lse, NB, S, H, head_dim, kv_shift, dtype, drop_p, drop_site, state, stream);
}

extern "C" int eg_attention_dk_bwd(const void* qkv, const void* ctx, const void* dctx, const float* lse, void* dqkv, int NB, int S,
                                   int H, int head_dim, int kv_shift, int dtype, float drop_p, uint32_t drop_site,
                                   const eg_step_state* state, float* scratch, int64_t scratch_elems, void* stream) {
  return long_bwd("eg_attention_dk_bwd", qkv, ctx, dctx, lse, dqkv, NB, S, H, head_dim, kv_shift, dtype, drop_p, drop_site, state,
                  scratch, scratch_elems, stream);
}

extern "C" int eg_attention_dk_probs(const void* qkv, const float* lse, float* probs, int NB, int S, int H, int head_dim, int kv_shift,
                                     int dtype, void* stream) {
  return long_probs("eg_attention_dk_probs", qkv, lse, probs, NB, S, H, head_dim, kv_shift, dtype, stream);
}
