// Wide-tile NT GEMM for the products whose output is one d_model-wide row block (N == 256, any K % 64 == 0, 16-bit operands):
//   C[M, 256] = epilogue(A[M, K] * W[256, K]^T)     out-proj, FFN-2, every backward-data product of the encoder, both 1-D convs
//
// Why a second tile: with N == 256 the 128x128 tile launches M/128 x 2 = 520 workgroups at the benchmark size -- 0.68 of one
// resident round -- and each pair of workgroups pulls the same A rows through two CUs' load paths.  Here ONE workgroup owns 160
// rows x all 256 columns: A crosses the load path once, the grid (208 workgroups for 33 280 rows) is a single round, and the
// K loop is fed by LDS-DMA (global_load_lds, 16 B per lane) through a 3-stage ring with ONE raw barrier per 64-deep K step and
// counted s_waitcnt vmcnt(N) waits, so two K steps of loads are always in flight behind the MFMAs.
//   512 threads = 8 waves as 2 (row halves of 80) x 4 (column groups of 64); a wave holds 5 x 4 accumulator tiles (80 VGPRs).
//   LDS rows are 128 B (one K step) with the 16-B-chunk XOR swizzle on the DMA's per-lane SOURCE address and on the fragment
//   reads (conflict-free ds_read_b128).  Epilogue: accumulators -> wave-private fp32 LDS image (rowtile.h; in the drained ring) ->
//   whole 128-B row segments with bias / activation / gate / dropout / second output / residual, exactly gemm_nt_kernel's order
//   (dropout, residual and stores are rowtile.h's row steps; activation, gate and second output are this kernel's own).
// Arithmetic is the same k-ordered MFMA chain as gemm_nt_kernel (bit-identical results).
//
// The row count is a template parameter: 160 as above, or 128 (row halves of 64, 4 x 4 accumulator tiles per wave, a 16 KB A
// stage: 48 KB per K step instead of 52).  wide_pick_rows chooses on the host, from M and the CU count, the tile with fewer
// resident rounds and, on a tie, fewer staged bytes per CU: M = 32 768 is ONE round of 256 workgroups on the 128-row tile
// (205 on 160 rows, with more bytes each), M = 33 280 stays on 160 rows (208 workgroups; 260 would be two rounds).
// gemm_nt_wide_batch_kernel runs up to EG_GEMM_BATCH_MAX such products (own operands, row maps, M and K) as ONE grid: a
// workgroup finds its product and row tile from the prefix table in the kernel arguments.
#include "rowtile.h"
#include <stdlib.h>

namespace {

constexpr int WBN = 256;
constexpr int WST_W = WBN * 128;                                             // 32 KB of W per stage
constexpr int WNST = 3;
constexpr int wide_lds(int BM) { return WNST * (BM * 128 + WST_W); }         // 160 rows: 159,744 B; 128 rows: 147,456 B

template <typename T>
struct WideNT {
  const T* A; const T* W; T* C; const float* bias; const T* residual; const T* gate; T* out_pre;
  const eg_step_state* st;
  RowMap a, c, r, pm;
  int M, N, K, ldw;
  DropCfg d1, d2;
  float gate_scale;
};

// one BM x 256 output tile starting at row m0 of product p
template <typename T, int ACT, int BM>
__device__ __forceinline__ void wide_tile(const WideNT<T>& args, const int m0, char* smem) {
  typedef typename H16<T>::frag frag;
  const WideNT<T> p = args;                                    // by value: the stores below cannot alias it
  static_assert(BM == 160 || BM == 128, "row halves of 80 or 64");
  constexpr int WST_A = BM * 128, WSTAGE = WST_A + WST_W;      // A stage: 20 KB or 16 KB
  constexpr int NA = BM / 8;                                   // A DMA instructions per stage: 20 or 16
  constexpr int NAW = (NA + 7) / 8;                            // ... of one wave, at most: 3 or 2
  constexpr int HM = BM / 2, TI = BM / 32;                     // rows and 16-row accumulator tiles of a wave: 80 / 5 or 64 / 4
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int l15 = lane & 15, g4 = lane >> 4;
  const int nk = p.K >> 6;

  // ---- DMA addressing: an instruction moves 8 rows x 128 B; lane -> row lane/8, LDS chunk position lane%8 holding global
  //      chunk pos ^ (row & 7).  A: 20 instructions per stage (waves 0-3 issue 3, waves 4-7 issue 2) or 16 (2 per wave);
  //      W: 32 (4 per wave). ----
  const int drow = lane >> 3, dpos = lane & 7;
  const int dsw = (dpos ^ drow) << 4;                        // (8q + drow) & 7 == drow
  const char* asrc[NAW];
#pragma unroll
  for (int i = 0; i < NAW; ++i) {
    const int r = 8 * (wave + 8 * i) + drow;
    asrc[i] = (const char*)(p.A + row_off(p.a, min(m0 + min(r, BM - 1), p.M - 1))) + dsw;
  }
  const char* wsrc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) wsrc[i] = (const char*)(p.W + (size_t)(8 * (wave + 8 * i) + drow) * (size_t)p.ldw) + dsw;
  const int na = (NA % 8 != 0 && wave >= NA % 8) ? NAW - 1 : NAW;   // A instructions of this wave per stage
  auto issue = [&](int kt, int slot) {
    char* sa = smem + slot * WSTAGE;
    const size_t ko = (size_t)kt * 128;
#pragma unroll
    for (int i = 0; i < NAW; ++i)
      if (i < na) eg_dma16(asrc[i] + ko, sa + (wave + 8 * i) * 1024);
#pragma unroll
    for (int i = 0; i < 4; ++i) eg_dma16(wsrc[i] + ko, sa + WST_A + (wave + 8 * i) * 1024);
  };

  f32x4 acc[TI][4];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  issue(0, 0);
  if (nk > 1) issue(1, 1);
  int slot = 0;
  for (int kt = 0; kt < nk; ++kt) {
    // this wave's part of stage kt has landed once at most the next stage's DMAs are outstanding
    if (kt + 1 < nk) {
      if (NA % 8 != 0 && wave < NA % 8) asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // stage kt visible; stage kt-1 no longer read by anyone
    if (kt + 2 < nk) issue(kt + 2, slot == 0 ? 2 : slot - 1);        // (kt+2) % 3 == (slot + 2) % 3
    asm volatile("" ::: "memory");
    const char* sa = smem + slot * WSTAGE + (HM * wm + l15) * 128;
    const char* sw = smem + slot * WSTAGE + WST_A + (64 * wn + l15) * 128;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int ch = ((kk * 4 + g4) ^ (l15 & 7)) << 4;
      frag xf[TI], wf[4];
#pragma unroll
      for (int i = 0; i < TI; ++i) xf[i] = *(const frag*)(sa + i * 16 * 128 + ch);
#pragma unroll
      for (int j = 0; j < 4; ++j) wf[j] = *(const frag*)(sw + j * 16 * 128 + ch);
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = H16<T>::mfma(wf[j], xf[i], acc[i][j]);
    }
    slot = slot == 2 ? 0 : slot + 1;
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");       // every wave has left the ring: it becomes epilogue scratch

  // ---- epilogue: per 16-row tile through the wave-private fp32 image; a lane then owns 16 consecutive columns of a row ----
  float* timg = (float*)(smem + wave * RT_IMGB);
  uint32_t seed_lo = 0, seed_hi = 0;
  if (p.d1.thresh | p.d2.thresh) { seed_lo = p.st->seed_lo; seed_hi = p.st->seed_hi; }
  const int er = lane >> 2, ec = lane & 3;                   // row of the tile, 16-column group
  const int n = 64 * wn + 16 * ec;
  float bv[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) bv[j] = 0.f;
  if (p.bias) { load8(p.bias + n, bv); load8(p.bias + n + 8, bv + 8); }
  // the epilogue operand (residual, else gate) of all of this lane's rows is requested up front: one exposed latency, not TI
  const T* const eop = p.residual ? p.residual : p.gate;
  const RowMap& emap = p.residual ? p.r : p.c;
  u32x4 eraw[TI][2];
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    eraw[i][0] = (u32x4){0u, 0u, 0u, 0u};
    eraw[i][1] = (u32x4){0u, 0u, 0u, 0u};
    const int m = m0 + HM * wm + 16 * i + er;
    if (eop && m < p.M) {
      const T* pe = eop + row_off(emap, m) + n;
      eraw[i][0] = *(const u32x4*)pe;
      eraw[i][1] = *(const u32x4*)(pe + 8);
    }
  }
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    const int m = m0 + HM * wm + 16 * i + er;
    rt_image_put(timg, acc[i], lane);
    if (m0 + HM * wm + 16 * i >= p.M) break;                 // wave-uniform: tiles wholly beyond M
    float v[16];
    rt_image_get(timg, lane, v);
    if (m < p.M) {
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = eg_act<ACT>(v[j] + bv[j]);
      const long long coff = row_off(p.c, m) + n;
      if (p.gate) {
        float gv[16];
        if (!p.residual) {
          load8((const T*)&eraw[i][0], gv);
          load8((const T*)&eraw[i][1], gv + 8);
        } else {
          load8(p.gate + coff, gv);
          load8(p.gate + coff + 8, gv + 8);
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = gv[j] > 0.f ? v[j] * p.gate_scale : 0.f;
      }
      rt_dropout16(v, p.d1, p.d2, seed_lo, seed_hi, (uint32_t)m * (uint32_t)p.N + (uint32_t)n);
      if (p.out_pre) rt_store16(p.out_pre + row_off(p.pm, m) + n, v);
      if (p.residual) rt_add16<T>(v, eraw[i][0], eraw[i][1]);
      rt_store16(p.C + coff, v);
    }
  }
}

template <typename T, int ACT, int BM>
__global__ __launch_bounds__(512, 2) void gemm_nt_wide_kernel(WideNT<T> p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  wide_tile<T, ACT, BM>(p, blockIdx.x * BM, smem);
}

// Several products as one grid.  Workgroups [tile_end[i-1], tile_end[i]) are the row tiles of product i, in the host's order
// (deepest K first, so the short products fill the last round); tile t of every product covers the same rows, and where the
// per-product tile counts are multiples of the XCD count -- the convolution phases -- it lands on the same XCD in each.
template <typename T>
struct WideBatch {
  WideNT<T> prob[EG_GEMM_BATCH_MAX];
  int tile_end[EG_GEMM_BATCH_MAX];
  int n;
};

template <typename T, int ACT, int BM>
__global__ __launch_bounds__(512, 2) void gemm_nt_wide_batch_kernel(WideBatch<T> b) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int blk = blockIdx.x;
  int pi = 0, t0 = 0;
#pragma unroll
  for (int i = 1; i < EG_GEMM_BATCH_MAX; ++i)
    if (i < b.n && blk >= b.tile_end[i - 1]) { pi = i; t0 = b.tile_end[i - 1]; }
  wide_tile<T, ACT, BM>(b.prob[pi], (blk - t0) * BM, smem);
}

template <typename T>
static WideNT<T> wide_args(const eg_gemm_desc* d) {
  WideNT<T> p;
  p.A = (const T*)d->A; p.W = (const T*)d->W; p.C = (T*)d->C; p.bias = d->bias;
  p.residual = (const T*)d->residual; p.gate = (const T*)d->gate; p.out_pre = (T*)d->out_pre; p.st = d->state;
  p.a = to_rowmap(d->a); p.c = to_rowmap(d->c); p.r = to_rowmap(d->r); p.pm = to_rowmap(d->p);
  p.M = d->M; p.N = d->N; p.K = d->K; p.ldw = d->ldw;
  p.d1 = make_drop(d->drop1_p, d->drop1_site);
  p.d2 = make_drop(d->drop2_p, d->drop2_site);
  p.gate_scale = d->gate_scale == 0.f ? 1.0f : d->gate_scale;
  return p;
}

// process-wide knobs: the forced tile (0 = by rule) and the row floor below which a product keeps the 128x128 tile
int g_force_rows = [] { const char* e = getenv("EYEGAZE_WIDE_TILE"); const int v = e ? atoi(e) : 0; return v == 128 || v == 160 ? v : 0; }();
int g_min_rows = 1024;                         // the head products (M = batch) keep the 128x128 tile

int device_cus() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    return n;
  }();
  return cus;
}

// fewer resident rounds first (a workgroup holds a CU: 144 KB or 156 KB of LDS), then fewer staged rows (A + W) per CU
int wide_pick_rows(long long tiles160, long long tiles128, int cus) {
  if (cus < 1) cus = 1;
  const long long r160 = (tiles160 + cus - 1) / cus, r128 = (tiles128 + cus - 1) / cus;
  if (r160 != r128) return r160 < r128 ? 160 : 128;
  return r160 * (160 + WBN) < r128 * (128 + WBN) ? 160 : 128;
}

template <typename T, int ACT, int BM>
static void wide_launch_one(const eg_gemm_desc* d, hipStream_t s) {
  eg_launch_lds<gemm_nt_wide_kernel<T, ACT, BM>, wide_lds(BM)>(dim3((d->M + BM - 1) / BM), dim3(512), s, wide_args<T>(d));
}

template <typename T, int BM>
static int wide_launch(const eg_gemm_desc* d, hipStream_t s) {
  if (d->act == EG_ACT_RELU) wide_launch_one<T, EG_ACT_RELU, BM>(d, s);
  else if (d->act == EG_ACT_GELU) wide_launch_one<T, EG_ACT_GELU, BM>(d, s);
  else wide_launch_one<T, EG_ACT_NONE, BM>(d, s);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

template <typename T, int ACT, int BM>
static void wide_launch_batch_one(const eg_gemm_desc* const* d, int n, hipStream_t s) {
  WideBatch<T> b;
  int end = 0;
  for (int i = 0; i < EG_GEMM_BATCH_MAX; ++i) {
    b.prob[i] = wide_args<T>(d[i < n ? i : 0]);
    if (i < n) end += (d[i]->M + BM - 1) / BM;
    b.tile_end[i] = end;
  }
  b.n = n;
  eg_launch_lds<gemm_nt_wide_batch_kernel<T, ACT, BM>, wide_lds(BM)>(dim3(end), dim3(512), s, b);
}

template <typename T, int BM>
static int wide_launch_batch(const eg_gemm_desc* const* d, int n, hipStream_t s) {
  const int act = d[0]->act;
  if (act == EG_ACT_RELU) wide_launch_batch_one<T, EG_ACT_RELU, BM>(d, n, s);
  else if (act == EG_ACT_GELU) wide_launch_batch_one<T, EG_ACT_GELU, BM>(d, n, s);
  else wide_launch_batch_one<T, EG_ACT_NONE, BM>(d, n, s);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

// eligibility + launch; returns -1 when the product does not fit this kernel (caller falls back)
bool eg_wide_gemm_ok(const eg_gemm_desc* d) {
  if ((d->dtype != EG_BF16 && d->dtype != EG_F16) || d->N != WBN || d->K % 64 != 0 || d->K < 128) return false;
  if (d->a_seg_len || !d->C) return false;
  if (d->M < g_min_rows) return false;
  // the epilogue reads residual / gate rows and writes out_pre rows as 16-B vectors: misaligned bases keep the 128x128 tile
  if (((uintptr_t)d->residual | (uintptr_t)d->gate | (uintptr_t)d->out_pre | (uintptr_t)d->C | (uintptr_t)d->A | (uintptr_t)d->W) % 16)
    return false;
  return d->ldw % 8 == 0;
}

int eg_wide_gemm_try(const eg_gemm_desc* d, hipStream_t s) {
  if (!eg_wide_gemm_ok(d)) return -1;
  const int rows = g_force_rows ? g_force_rows : eg_gemm_wide_rows(d->M, device_cus());
  return eg_dispatch_16(d->dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return rows == 128 ? wide_launch<T, 128>(d, s) : wide_launch<T, 160>(d, s);
  });
}

// the epilogue steps a product takes (one bit each) and its activation; the products of a batch must agree on them
int eg_wide_gemm_kind(const eg_gemm_desc* d) {
  return (d->bias ? 1 : 0) | (d->residual ? 2 : 0) | (d->gate ? 4 : 0) | (d->out_pre ? 8 : 0) |
         (d->drop1_p > 0.f ? 16 : 0) | (d->drop2_p > 0.f ? 32 : 0) | (d->act << 8);
}

// every product fits this kernel and they agree on dtype and epilogue: they can run as one grid
bool eg_wide_gemm_batch_ok(const eg_gemm_desc* descs, int n) {
  if (n < 1 || n > EG_GEMM_BATCH_MAX) return false;
  for (int i = 0; i < n; ++i)
    if (!eg_wide_gemm_ok(descs + i) || descs[i].dtype != descs[0].dtype || eg_wide_gemm_kind(descs + i) != eg_wide_gemm_kind(descs))
      return false;
  return true;
}

// 0: launched as one grid; -1: not eligible (the caller launches the products one by one); -2: launch error
int eg_wide_gemm_batch_try(const eg_gemm_desc* descs, int n, hipStream_t s) {
  if (!eg_wide_gemm_batch_ok(descs, n)) return -1;
  const eg_gemm_desc* d[EG_GEMM_BATCH_MAX];
  for (int i = 0; i < n; ++i) d[i] = descs + i;
  for (int i = 1; i < n; ++i)                     // stable insertion sort, deepest K first
    for (int j = i; j > 0 && d[j]->K > d[j - 1]->K; --j) { const eg_gemm_desc* t = d[j]; d[j] = d[j - 1]; d[j - 1] = t; }
  long long t160 = 0, t128 = 0;
  for (int i = 0; i < n; ++i) { t160 += (d[i]->M + 159) / 160; t128 += (d[i]->M + 127) / 128; }
  const int rows = g_force_rows ? g_force_rows : wide_pick_rows(t160, t128, device_cus());
  if ((rows == 128 ? t128 : t160) > 0x7fffffffll) return -1;     // the tiles must fit one grid
  return eg_dispatch_16(d[0]->dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return rows == 128 ? wide_launch_batch<T, 128>(d, n, s) : wide_launch_batch<T, 160>(d, n, s);
  });
}

extern "C" int eg_gemm_wide_rows(int M, int cus) {
  if (M < 1) return 0;
  return wide_pick_rows(((long long)M + 159) / 160, ((long long)M + 127) / 128, cus);
}

extern "C" int eg_gemm_wide_config(int tile_rows, int min_rows) {
  EG_CHECK(tile_rows == -1 || tile_rows == 0 || tile_rows == 128 || tile_rows == 160, "eg_gemm_wide_config: tile_rows=%d", tile_rows);
  EG_CHECK(min_rows == -1 || min_rows >= 1, "eg_gemm_wide_config: min_rows=%d", min_rows);
  if (tile_rows >= 0) g_force_rows = tile_rows;
  if (min_rows >= 1) g_min_rows = min_rows;
  return 0;
}
