// Chained product pair of the position-wise feed-forward block (A:272) in ONE launch, forward and backward-data alike:
//   H[M, F]   = epi1(A[M, 256] * W1[F, 256]^T)      epi1: + bias1, ReLU, gate (ReLU backward), dropout      -> stored (backward and
//   C[M, 256] = epi2(H[M, F]   * W2[256, F]^T)                                                                 weight gradients need it)
//   forward : A = y1, W1 = linear1, W2 = linear2, epi2 = + bias2, dropout x2, + residual (the A rows themselves) -> r2
//   backward: A = dY, W1 = linear2^T, gate = saved hidden rows, W2 = linear1^T, epi2 = + residual (dr)           -> dy1
// As two launches the pair moves H through HBM twice (write, read back: 2 x 68 MB per layer and direction at the benchmark
// size) and A / the residual once more; here the hidden rows only leave the chip once, as the stored result.
//
// Design (gfx950), one 256-thread workgroup (4 waves = 4 column groups, one per SIMD) per 80 rows, TWO workgroups per CU (80 KB
// of LDS each): the two row halves of a CU share nothing, so they run as independent workgroups whose phases drift apart -- one's
// MFMA bursts sit beside the other's epilogue / barrier / store phases (as one 512-thread workgroup every wave hit the same
// barrier and the matrix pipe idled through each epilogue):
//   * the A tile [80 x 256] stays in LDS for the whole launch (40 KB: the resident tile of rowtile.h, which also holds the DMA map,
//     the swizzle, the fragment order of the weights and the image epilogue used below); it is the
//     B operand of every product-1 MFMA and, in the forward pass, the residual of the final epilogue (no second HBM read);
//   * the hidden dimension is walked in chunks of 128 columns: product 1 gives a wave 80 x 32 of the chunk (5 x 2 accumulator
//     tiles over K = 256), its epilogue writes the 16-bit chunk into one of TWO 20 KB LDS buffers (one barrier per chunk), from
//     where (a) all threads stream it to HBM as whole 256-B row segments and (b) product 2 reads it back as the B operand of
//     the wave's 80 x 64 part of C (5 x 4 accumulator tiles that live in registers across all chunks);
//   * the loop is SKEWED by one phase.  Per wave:  product 1 (0), epilogue 1 (0);  then for c = 1 .. nch - 1:  barrier,
//     product 1 (c) with the H store of chunk c - 1 spread over its k-steps, { epilogue 1 (c) BESIDE product 2 (c - 1) };  then
//     barrier, H store (nch - 1), product 2 (nch - 1), barrier, epilogue 2.  Epilogue 1 is vector work only, product 2 a chain of
//     LDS reads and MFMAs that leaves most issue slots empty; they touch different accumulators and different halves of the chunk
//     image, and in one scheduling region per tile the MFMAs run under the hash / pack arithmetic;
//   * WEIGHTS NEVER TOUCH LDS: a wave's W1 / W2 fragments (pre-packed in fragment order, rt_frag_elem: one contiguous 1-KB read each,
//     L2-resident, 1 MB per layer) go straight into registers through rolling rings four / two k-steps ahead, so the LDS pipe only carries
//     the activation fragments: 0.5 KB per MFMA in product 1, 0.25 KB in product 2 -- below the 0.5 KB / MFMA at which LDS and
//     matrix pipes balance, which the 128 x 128 and 160 x 256 tiles (weights through LDS) sit on;
//   * the backward gate ("the saved hidden value is > 0": ReLU and dropout cut together) travels as ONE BIT per element: the
//     forward launch writes it in MFMA-lane order (40 bits of one 8-byte word per lane and chunk), the backward launch of the
//     same geometry reads one word per lane and chunk, two chunks ahead -- 4.3 MB per layer instead of re-reading the 68 MB of
//     hidden rows, and no HBM-latency loads in front of the weight fragments in the waves' in-order vmcnt queues (with the gate
//     rows themselves loaded into registers the backward form took 75 us against 68 us for the two launches).  The hidden
//     rows themselves remain accepted as the gate (eg_ffn_desc.gate) for callers without a forward launch of this kernel.
// Arithmetic: the same k-ordered chains of v_mfma_f32_16x16x32 as eg_gemm_nt's kernels and the same epilogue order and dropout
// indices, so H and C are bit-identical to the two-launch path.
// eg_ffn_bwd_ln_proj: the backward form going on, in the same launch, with norm-1's backward and out_proj's backward-data product on
// the C rows it has just completed (the TAIL flag below; steps 2-4 of lnproj.hip through lnproj.h, bit-identical to that launch).
#include <type_traits>
#include "lnproj.h"

namespace {

constexpr int FR = RT_ROWS;                   // rows per workgroup
constexpr int FD = RT_COLS;                   // d_model: K of product 1, N of product 2
constexpr int FC = 128;                       // hidden columns per chunk
constexpr int F_XT = RT_TILEB;                // 40,960 B
constexpr int F_HT = FR * FC * 2;             // 20,480 B
constexpr int F_LDS = F_XT + 2 * F_HT;        // 81,920 B = half the LDS of a CU

// The merged phase's pinned interleave for one tile of epilogue 1 and its share of a k-step's MFMAs: LEAD vector instructions
// first (they cover the latency of the fragment reads), then PER vector instructions behind each MFMA.
template <int LEAD, int PER>
__device__ __forceinline__ void ffn_pin() {
  __builtin_amdgcn_sched_group_barrier(0x2, LEAD, 0);
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x2, PER, 0);
  }
}

template <typename T>
struct FfnArgs {
  const T* A; const T* W1; const T* W2; T* H; T* C; const float* bias1; const float* bias2; const T* gate; const T* residual;
  const unsigned long long* bits_in; unsigned long long* bits_out;
  const float* ln_gamma; const float* ln_beta; T* LN_OUT; float* ln_stats;   // LNF: y = LayerNorm(C) in the final epilogue
  const eg_step_state* st;
  long long lda, ldh, ldc, ldg, ldr;
  int M, F, relu, res_in_lds;
  DropCfg dh, dc1, dc2;
  float gate_scale;
};

// EPI selects epilogue 1's bias / ReLU at compile time: 3 = bias + ReLU (the forward pass), 0 = neither (the backward pass),
// 4 = as the descriptor says at run time (a per-value select on the flag -- 80 extra vector instructions per chunk).
// LNF: the layer's second LayerNorm runs on the completed C rows in the final epilogue (eg_epilogue_layernorm256).
// KEEP = false is the LEAN form of a forward that nobody differentiates (<T, 0, 0, 3, true> only): H, C and the LayerNorm statistics
// are never stored, LN_OUT is the launch's only global store.  The hidden chunk still passes through LDS rounded to 16 bit as
// product 2's operand and C is still rounded to 16 bit in front of the LayerNorm, so LN_OUT is bit-identical to the keeping form's.
// TAIL (<T, 2, 0, 0, false, true> only: the backward pass behind eg_ffn_bwd_ln_proj): the launch goes on with norm-1's backward and
// out_proj's backward-data product on the rows it has just completed -- steps 2-4 of ln_bwd_proj_kernel (lnproj.h) on q's operands.
// Epilogue 2 leaves the rounded C rows in the resident tile xt (dead after the last product 1) as well as in C (when given); the
// LayerNorm input rows come straight into registers in the half-wave layout, requested in front of epilogue 2.  LDS of the tail:
//   xt [0, 40 KB)        dy1 rows (epilogue 2) -> dyo rows in place (step 2) -> A operand of step 3
//   hb [0, 17 KB)        epilogue 2's four images; then [0, 16 KB) the gain / bias sums, [16 KB, 33 KB) step 4's four images
struct FfnNoTail {};
template <typename T, int GATE, int BOUT, int EPI, bool LNF = false, bool KEEP = true, bool TAIL = false, bool DROP = false>
__global__ __launch_bounds__(256, 2) void ffn_chain_kernel(FfnArgs<T> p, std::conditional_t<TAIL, LnProjArgs<T>, FfnNoTail> q) {
  static_assert(!TAIL || (GATE == 2 && BOUT == 0 && EPI == 0 && !LNF && KEEP), "the norm-1 tail follows the backward form only");
  typedef typename H16<T>::frag frag;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const xt = smem;
  char* const hb = smem + F_XT;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);     // wave = column group
  const int l15 = lane & 15, g4 = lane >> 4;
  const int m0 = blockIdx.x * FR;
  const int nch = p.F / FC;
  // The stored rows of chunk c - 1 leave under product 1 (c), one 16-B piece per thread behind five of its k-steps, instead of in a
  // phase of their own behind the barrier -- where the registers allow it: the run-time epilogue (EPI = 4) and the row gate
  // (GATE = 1) have none to spare and keep the store phase.
  constexpr bool SPREAD = KEEP && EPI != 4 && GATE != 1;

  // ---- A tile (rows beyond M repeat row M - 1) ----
#pragma unroll
  for (int i = 0; i < RT_DMA_PER_WAVE; ++i) {
    const int row = min(m0 + rt_dma_row(wn, lane, i), p.M - 1);
    rt_dma_issue((const char*)(p.A + (size_t)row * (size_t)p.lda), xt, wn, lane, i);
  }

  // ---- weight fragment streams (global -> registers): the weights arrive in FRAGMENT ORDER (eg_pack_table modes 3-6), so a
  //      fragment load is one contiguous 1-KB read per wave.  (Row-major weights cost 64 L1 tag look-ups per load -- 16 rows x
  //      64 B per quarter wave -- and made the launch tag-rate-bound: 98 us against 72 us for the two launches it replaces.) ----
  const char* const w1u = (const char*)(p.W1 + rt_frag_elem<8, 2>(0, wn, 0, 0));    // this wave's part of chunk 0
  const char* const w2u = (const char*)(p.W2 + rt_frag_elem<4, 4>(0, wn, 0, 0));
  const uint32_t wl = (uint32_t)lane * 16u;                                      // wave-uniform base + 32-bit lane offset: saddr loads
  // Rolling rings, four (W1) / two (W2) k-steps ahead of their MFMAs and running on across chunk boundaries.  (Requesting a
  // whole chunk's fragments one phase ahead -- 16 + 16 live fragments -- was built: 67-88 spilled registers; the 256-register
  // budget of two waves per SIMD is spent on the 5 x 4 + 5 x 2 accumulator tiles.)
  frag w1r[4][2], w2r[2][4];
  auto req_w1 = [&](int c, int s, int slot) {
#pragma unroll
    for (int j = 0; j < 2; ++j) w1r[slot][j] = *(const frag*)(w1u + rt_frag_elem<8, 2>(c, 0, s, j) * 2 + wl);
  };
  auto req_w2 = [&](int c, int s, int slot) {
#pragma unroll
    for (int j = 0; j < 4; ++j) w2r[slot][j] = *(const frag*)(w2u + rt_frag_elem<4, 4>(c, 0, s, j) * 2 + wl);
  };
#pragma unroll
  for (int s = 0; s < 4; ++s) req_w1(0, s, s);

  f32x4 acc2[5][4];
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc2[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  uint32_t seed_lo = 0, seed_hi = 0;
  if (p.dh.thresh | p.dc1.thresh | p.dc2.thresh) { seed_lo = p.st->seed_lo; seed_hi = p.st->seed_hi; }

  // ---- weights into the Infinity Cache: in a training step a launch finds its 1 MB of weights in HBM (written a whole step
  //      earlier), and because all workgroups walk the chunks in lock-step each chunk's first touch stalled every one of them
  //      (74 us against 62 us when a replayed launch finds them cached).  So every workgroup touches its 1/grid share of ALL
  //      chunks' 128-B lines here, where the wave waits for its HBM-resident A rows anyway: by the time chunk 1 is needed the
  //      lines sit in the memory-side cache, one XCD's L2 miss away. ----
  uint32_t touched = 0;
  if (wn < 2) {
    const char* wb = (const char*)(wn == 0 ? p.W1 : p.W2);
    const int lines = p.F * FD * 2 / 128;                    // per matrix
    const int per = (lines + gridDim.x - 1) / gridDim.x;
    for (int t = lane; t < per; t += 64) {
      const int g = blockIdx.x * per + t;
      if (g < lines) touched += *(const uint32_t*)(wb + (size_t)g * 128);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's part of the A tile has landed (and the first fragments)
  asm volatile("" :: "v"(touched));
  __syncthreads();                                           // ... and everybody else's

  // gate bit words: [workgroup][chunk][wave][lane]
  const unsigned long long* const bits_p = p.bits_in ? p.bits_in + ((size_t)blockIdx.x * nch * 4 + wn) * 64 + lane : nullptr;
  unsigned long long gnext0 = 0, gnext1 = 0;
  if (GATE == 2) {
    gnext0 = bits_p[0];
    if (nch > 1) gnext1 = bits_p[256];
  }
  const int rbase = l15;                                     // row of tile i within the workgroup: rbase + 16 i
  // epilogue-1 lane constants, formed per chunk behind an opaque lane id (not carried across the loop: the merged phase has no
  // register to spare): byte offset of this lane's 8-B slot (row l15, hidden column 32 wn + 16 j + 4 g4 of the chunk) in the
  // swizzled chunk image -- tile row i adds the immediate 4096 i -- and the dropout PAIR index of (row m0 + l15, column 32 wn + 4 g4)
  struct E1Lane { int ha[2]; uint32_t pairc; };
  auto e1_lane = [&](int c, int l15o, int g4o) __attribute__((always_inline)) {
    E1Lane e;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int hcol = 32 * wn + 16 * j + 4 * g4o;
      e.ha[j] = l15o * 256 + (((hcol >> 3) ^ rt_swz(l15o)) << 4) + ((hcol & 4) << 1);
    }
    e.pairc = (((uint32_t)(m0 + l15o) * (uint32_t)p.F + (uint32_t)(32 * wn + 4 * g4o)) >> 1) + (uint32_t)(FC / 2) * (uint32_t)c;
    return e;
  };
  const uint32_t pairF = 8u * (uint32_t)p.F;                 // 16 rows further

  // ---- the chunk loop, skewed by one phase: epilogue 1 of chunk c runs BESIDE product 2 of chunk c - 1 ----
  //   before the loop  product 1 (0), epilogue 1 (0)
  //   iteration c      barrier, H store (c - 1) [under product 1 where SPREAD], product 1 (c), { epilogue 1 (c)  ||  product 2 (c - 1) }
  //   behind the loop  barrier, H store (nch - 1), product 2 (nch - 1)
  // Epilogue 1 is vector work only and product 2 a chain of LDS reads and MFMAs that leaves most issue slots empty; they use
  // different accumulators and different halves of hb (epilogue 1 (c) writes hb[c & 1], product 2 (c - 1) reads hb[(c - 1) & 1]),
  // so one barrier per chunk still does: it publishes chunk c and retires every read of the other half before epilogue 1
  // (c + 1) overwrites it; the H store (c) and product 2 (c) read hb[c & 1] between that barrier and the next one.
  f32x4 acc1[5][2];
  float b1[2][4];
  u32x2 gt[5][2];
  // gate bits of a lane and chunk: word g (= tile rows 0-2 | 3-4 ... see below) collects, in the order the epilogue visits them, the
  // flags of its 32-bit stores (two values each): flag of the even value in the low half, of the odd value in the high half,
  // first store highest.  20 stores -> two words of 10 + 10 bits per half.
  uint32_t gw[2] = {0u, 0u};

  // epilogue-1 operands of chunk c, requested before the product-1 MFMAs that hide them
  auto req_e1 = [&](int c) __attribute__((always_inline)) {
    const int f0 = FC * c + 32 * wn + 4 * g4;                // hidden column of accumulator register q of tile j: f0 + 16 j + q
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) b1[j][q] = 0.f;
      if (EPI == 3 || (EPI == 4 && p.bias1)) load4(p.bias1 + f0 + 16 * j, b1[j]);
    }
    if (GATE == 1) {
      int rb = rbase;
      asm volatile("" : "+v"(rb));                             // addresses are recomputed per chunk, not kept (and spilled) across the loop
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const int m = min(m0 + rb + 16 * i, p.M - 1);
#pragma unroll
        for (int j = 0; j < 2; ++j) gt[i][j] = *(const u32x2*)(p.gate + (size_t)m * (size_t)p.ldg + f0 + 16 * j);
      }
    }
    if (GATE == 2) {                                           // this chunk's word was requested two chunks ago
      gw[0] = (uint32_t)gnext0;
      gw[1] = (uint32_t)(gnext0 >> 32);
      gnext0 = gnext1;
      if (c + 2 < nch) gnext1 = bits_p[(size_t)(c + 2) * 256];
    }
  };

  // ---- product 1: acc1[i][j] = sum_k W1[hidden][k] * A[row][k] ----
  auto product1 = [&](int c, int cst = -1) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc1[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int lo = lane;
    asm volatile("" : "+v"(lo));                               // (its fragment addresses: recomputed per chunk, not kept across the loop)
    const int l15o = lo & 15, g4o = lo >> 4, sw7o = rt_swz(l15o);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      frag xf[5];
      rt_frags<T>(xt, l15o, g4o, sw7o, s, xf);
#pragma unroll
      for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc1[i][j] = H16<T>::mfma(w1r[s & 3][j], xf[i], acc1[i][j]);
      if (s < 4) req_w1(c, s + 4, s & 3);
      else if (c + 1 < nch) req_w1(c + 1, s - 4, s & 3);
      if (SPREAD && cst >= 0 && s >= 1 && s <= 5) {            // one 16-B piece per thread of chunk cst's stored rows behind k-steps 1-5
        const int ps = s - 1, r = 16 * ps + (tid >> 4), ch = tid & 15;
        const u32x4 o = *(const u32x4*)(hb + (cst & 1) * F_HT + r * 256 + rt_piece(r, ch));
        if (m0 + r < p.M) *(u32x4*)(p.H + (size_t)(m0 + r) * (size_t)p.ldh + FC * cst + 8 * ch) = o;
      }
    }
  };

  // ---- product 2: acc2[i][j] += sum_h W2[col][h] * H[row][h] over the chunk's 128 hidden columns; group g = 5 s + i is k-step s
  //      of tile row i: one fragment read and four MFMAs ----
  auto p2_frag = [&](const char* hc, int g, int l15o, int g4o) __attribute__((always_inline)) {
    return *(const frag*)(hc + (l15o + 16 * (g % 5)) * (FC * 2) + (((4 * (g / 5) + g4o) ^ rt_swz(l15o)) << 4));
  };
  auto p2_group = [&](int g, const frag& hf) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc2[g % 5][j] = H16<T>::mfma(w2r[(g / 5) & 1][j], hf, acc2[g % 5][j]);
  };

  // ---- epilogue 1 of tile t = 2 i + j (MFMA layout: lane holds 4 consecutive hidden columns of row l15) -> 16-bit chunk image in LDS ----
  // Vector-instruction count matters here: 817 vector instructions per wave and chunk against 160 MFMAs before this form.
  // DROP is p.dh.thresh != 0 as a type: a run-time branch per tile would end the scheduling region that product 2 shares.
  auto e1_tile = [&](int t, char* hc, const E1Lane& el, uint32_t (&ow)[2]) __attribute__((always_inline)) {
    const int i = t >> 1, j = t & 1;                          // store pair 2t, 2t+1 of this chunk
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[q] = acc1[i][j][q];
      if (EPI == 3 || EPI == 4) v[q] += b1[j][q];
      if (EPI == 3) v[q] = fmaxf(v[q], 0.f);
      if (EPI == 4 && p.relu) v[q] = fmaxf(v[q], 0.f);
    }
    if (GATE == 1) {
      float gv[4];
      load4((const T*)&gt[i][j], gv);
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = gv[q] > 0.f ? v[q] * p.gate_scale : 0.f;
    }
    if (GATE == 2) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = (2 * t + (q >> 1)) % 10;              // position among the word's 10 stores
        int m;                                               // 0 or -1 (as asm: the compiler turns the builtin back into and + compare + select)
        asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m) : "v"(gw[t / 5]), "n"((9 - n) + 16 * (q & 1)));
        v[q] = __uint_as_float(__float_as_uint(v[q] * p.gate_scale) & (uint32_t)m);
      }
    }
    if (DROP) {                                             // = eg_dropout_run<4> at element (m0 + l15 + 16 i) * F + f0 + 16 j
      const uint32_t e = el.pairc + (uint32_t)(8 * j) + (uint32_t)i * pairF;
      const uint32_t h0 = eg_hash(seed_lo, seed_hi, p.dh.site, e), h1 = eg_hash(seed_lo, seed_hi, p.dh.site, e + 1u);
      v[0] = (h0 & 0xFFFFu) >= p.dh.thresh ? v[0] * p.dh.scale : 0.0f;
      v[1] = (h0 >> 16) >= p.dh.thresh ? v[1] * p.dh.scale : 0.0f;
      v[2] = (h1 & 0xFFFFu) >= p.dh.thresh ? v[2] * p.dh.scale : 0.0f;
      v[3] = (h1 >> 16) >= p.dh.thresh ? v[3] * p.dh.scale : 0.0f;
    }
    const u32x2 pk = pack4<T>(v);
    *(u32x2*)(hc + el.ha[j] + 4096 * i) = pk;
    if (BOUT) {                                              // "stored value > 0", taken from the stored 16-bit patterns:
#pragma unroll
      for (int h = 0; h < 2; ++h) {                          // min(max(as int16, 0), 1) per half = 1 exactly for +x, x != 0
        uint32_t z, f;                                         // (as asm: three instructions per store; the elementwise builtins
        asm("v_pk_max_i16 %0, %1, 0" : "=v"(z) : "v"(pk[h]));                      // came back as compare / select / permute chains)
        asm("v_pk_min_u16 %0, %1, %2" : "=v"(f) : "v"(z), "v"(0x00010001u));
        ow[t / 5] = (ow[t / 5] << 1) | f;
      }
    }
  };

  // ---- the merged phase: tile t of epilogue 1 (c) beside groups 2t, 2t + 1 of product 2 (c - 1), each tile and its eight MFMAs a
  //      scheduling region of their own (the regions keep epilogue 1's values dying tile by tile: one region over the whole
  //      phase computed all ten tiles' values first and spilled).  Two fragments are live at a time, not a k-step's five.
  //      Product 2 (c - 1) requests the W2 fragments of chunk c's first two k-steps without a test: chunk c exists. ----
  auto merged = [&](int c, uint32_t (&ow)[2]) __attribute__((always_inline)) {
    char* const hc = hb + (c & 1) * F_HT;
    const char* const hp = hb + ((c & 1) ^ 1) * F_HT;
    int lo = lane;
    asm volatile("" : "+v"(lo));                               // product 2's addresses are recomputed per chunk, not kept across the loop
    const int l15o = lo & 15, g4o = lo >> 4;
    const E1Lane el = e1_lane(c, l15o, g4o);
#pragma unroll
    for (int t = 0; t < 10; ++t) {                             // tile t beside groups 2t, 2t + 1
      const frag hf0 = p2_frag(hp, 2 * t, l15o, g4o), hf1 = p2_frag(hp, 2 * t + 1, l15o, g4o);
      e1_tile(t, hc, el, ow);
      p2_group(2 * t, hf0);
      p2_group(2 * t + 1, hf1);
#pragma unroll
      for (int u = 0; u < 2; ++u)
        if ((2 * t + u) % 5 == 4) {                            // k-step s is through: its ring slot takes k-step s + 2
          const int s = (2 * t + u) / 5;
          if (s < 2) req_w2(c - 1, s + 2, s & 1);
          else req_w2(c, s - 2, s & 1);
        }
      if (DROP) ffn_pin<16, 8>();
      else ffn_pin<2, 2>();
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // chunk 0 has no product 2 beside its epilogue 1
  auto e1_alone = [&](uint32_t (&ow)[2]) __attribute__((always_inline)) {
    int lo = lane;
    asm volatile("" : "+v"(lo));
    const E1Lane el = e1_lane(0, lo & 15, lo >> 4);
#pragma unroll
    for (int t = 0; t < 10; ++t) {
      e1_tile(t, hb, el, ow);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // chunk c is complete in LDS: its gate bits, the barrier, and the stored result: whole 256-B row segments, 16 B per thread
  auto publish = [&](int c, const uint32_t (&ow)[2], bool store = true) __attribute__((always_inline)) {
    const char* const hc = hb + (c & 1) * F_HT;
    if (BOUT) p.bits_out[((size_t)blockIdx.x * nch + c) * 256 + wn * 64 + lane] = (unsigned long long)ow[0] | ((unsigned long long)ow[1] << 32);
    __syncthreads();        // chunk c is complete in LDS; nobody reads buffer (c+1)&1 (chunk c-1) any more
    if (KEEP && store) {
      int tq = tid >> 4;
      asm volatile("" : "+v"(tq));                             // (same: no loop-invariant address registers)
#pragma unroll
      for (int ps = 0; ps < 5; ++ps) {
        const int r = 16 * ps + tq, ch = tid & 15;
        const u32x4 o = *(const u32x4*)(hc + r * 256 + rt_piece(r, ch));
        if (m0 + r < p.M) *(u32x4*)(p.H + (size_t)(m0 + r) * (size_t)p.ldh + FC * c + 8 * ch) = o;
      }
    }
  };

  {
    uint32_t ow[2] = {0u, 0u};
    req_e1(0);
    product1(0);
    e1_alone(ow);
#pragma unroll
    for (int s = 0; s < 2; ++s) req_w2(0, s, s);               // the W2 ring starts here: product 2 (0) is a whole product 1 away
    for (int c = 1; c < nch; ++c) {
      publish(c - 1, ow, !SPREAD);
      ow[0] = 0u; ow[1] = 0u;
      req_e1(c);
      product1(c, SPREAD ? c - 1 : -1);
      merged(c, ow);
    }
    publish(nch - 1, ow);
    // product 2 of the last chunk (no further weight fragments)
    const char* const hp = hb + ((nch - 1) & 1) * F_HT;
    int lo = lane;
    asm volatile("" : "+v"(lo));
    const int l15o = lo & 15, g4o = lo >> 4;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      frag hf[5];
#pragma unroll
      for (int i = 0; i < 5; ++i) hf[i] = p2_frag(hp, 5 * s + i, l15o, g4o);
#pragma unroll
      for (int i = 0; i < 5; ++i) p2_group(5 * s + i, hf[i]);
      if (s < 2) req_w2(nch - 1, s + 2, s & 1);
    }
    __builtin_amdgcn_sched_barrier(0);                         // (the last MFMAs stay in front of the barrier, out of epilogue 2's registers)
  }
  __syncthreads();          // every wave has left the chunk buffers: they become the fp32 image of the final epilogue

  // ---- epilogue 2: per 16-row tile through the wave-private fp32 image; a lane then owns 16 consecutive columns of a row ----
  float* timg = (float*)(hb + wn * RT_IMGB);
  const int er = lane >> 2, ec = lane & 3;
  const int n = 64 * wn + 16 * ec;
  float bv[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) bv[j] = 0.f;
  if (p.bias2) { load8(p.bias2 + n, bv); load8(p.bias2 + n + 8, bv + 8); }
  u32x4 eraw[5][2];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    eraw[i][0] = (u32x4){0u, 0u, 0u, 0u};
    eraw[i][1] = (u32x4){0u, 0u, 0u, 0u};
    const int r = 16 * i + er;
    if (p.res_in_lds) {
      rt_tile_row16(xt, r, n, eraw[i][0], eraw[i][1]);
    } else if (p.residual && m0 + r < p.M) {
      const T* pe = p.residual + (size_t)(m0 + r) * (size_t)p.ldr + n;
      eraw[i][0] = *(const u32x4*)pe;
      eraw[i][1] = *(const u32x4*)(pe + 8);
    }
  }
  // TAIL: the LayerNorm input rows of this half-wave (rows hw + 8 j, piece l) and their statistics travel under epilogue 2
  const int tl = lane & 31, thw = tid >> 5;
  u32x4 xr[TAIL ? LP_ROWS_PER_HW : 1];
  float mean[TAIL ? LP_ROWS_PER_HW : 1], rstd[TAIL ? LP_ROWS_PER_HW : 1];
  if constexpr (TAIL) {
#pragma unroll
    for (int j = 0; j < LP_ROWS_PER_HW; ++j) {
      const int m = min(m0 + thw + 8 * j, q.M - 1);    // (rows beyond M repeat row M - 1, as the tile load does; step 2 zeroes them)
      xr[j] = *(const u32x4*)(q.x + (size_t)m * FD + tl * 8);
    }
    lp_stats(q.stats, q.M, m0, thw, mean, rstd);
  }
  float vv[LNF ? 5 : 1][16];                       // LNF: the stored C values of this lane's rows, for the LayerNorm below
  if (LNF) {
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
      for (int j = 0; j < 16; ++j) vv[i][j] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int m = m0 + 16 * i + er;
    rt_image_put(timg, acc2[i], lane);
    if (m0 + 16 * i >= p.M) break;                 // workgroup-uniform: tiles wholly beyond M
    float v[16];
    rt_image_get(timg, lane, v);
    if constexpr (TAIL) {
      if (m < p.M) {
        rt_row_epilogue<T, false, false>(v, bv, p.dc1, p.dc2, seed_lo, seed_hi, (uint32_t)m * (uint32_t)FD + (uint32_t)n,
                                         p.residual != nullptr, eraw[i][0], eraw[i][1], (T*)nullptr, vv[0]);
        if (p.C) rt_store16(p.C + (size_t)m * (size_t)p.ldc + n, v);
        const int r = 16 * i + er;                   // the same 16-bit values into the resident tile: step 2's dy rows
        store8((T*)(xt + r * RT_ROWB + rt_piece(r, n >> 3)), v);
        store8((T*)(xt + r * RT_ROWB + rt_piece(r, (n >> 3) + 1)), v + 8);
      }
    } else if (m < p.M)
      rt_row_epilogue<T, LNF, KEEP>(v, bv, p.dc1, p.dc2, seed_lo, seed_hi, (uint32_t)m * (uint32_t)FD + (uint32_t)n, p.residual != nullptr,
                                    eraw[i][0], eraw[i][1], KEEP ? p.C + (size_t)m * (size_t)p.ldc + n : nullptr, vv[LNF ? i : 0]);
  }
  if constexpr (TAIL) {
    // gain, the out_proj fragments of the first two k-steps and the dropout seed; then steps 2-4 of ln_bwd_proj_kernel
    const char* const wu = (const char*)(q.Wf + rt_frag_elem<4, 4>(0, wn, 0, 0));
    frag wr[2][4];
    float g[8], dg[8], db[8];
    load8(q.gamma + tl * 8, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) { dg[e] = 0.f; db[e] = 0.f; }
    const bool drop = (q.d1.thresh | q.d2.thresh) != 0;
    uint32_t qs_lo = 0, qs_hi = 0;
    if (drop) { qs_lo = q.st->seed_lo; qs_hi = q.st->seed_hi; }
    lp_req_w<T>(wu, wl, 0, wr[0]);
    lp_req_w<T>(wu, wl, 1, wr[1]);
    __syncthreads();                               // xt holds the tile's dy1 rows; epilogue 2's images are free
    lp_ln_rows<T, true>(q, xt, nullptr, xr, m0, thw, tl, g, mean, rstd, drop, qs_lo, qs_hi, dg, db);
    __syncthreads();                               // xt = dyo complete
    lp_sums(q.partial, (float*)hb, dg, db, tid, thw, tl);
    lp_product<T>(q.dC, q.M, xt, wr, wu, wl, (float*)(hb + LP_SUMS_B + wn * RT_IMGB), m0, lane, wn);
  }
  if constexpr (LNF)
    eg_epilogue_layernorm256<T>(vv, (float*)(hb + 4 * RT_IMGB), wn, lane, min(FR, p.M - m0), (size_t)m0, p.ln_gamma, p.ln_beta,
                                p.LN_OUT, KEEP ? p.ln_stats : nullptr);
}

template <typename T>
static FfnArgs<T> ffn_make_args(const eg_ffn_desc* d) {
  FfnArgs<T> p;
  p.A = (const T*)d->A; p.W1 = (const T*)d->W1; p.W2 = (const T*)d->W2; p.H = (T*)d->H; p.C = (T*)d->C;
  p.bits_in = (const unsigned long long*)d->gate_bits_in; p.bits_out = (unsigned long long*)d->gate_bits_out;
  p.bias1 = d->bias1; p.bias2 = d->bias2; p.gate = (const T*)d->gate; p.residual = (const T*)d->residual; p.st = d->state;
  p.lda = d->lda; p.ldh = d->ldh; p.ldc = d->ldc; p.ldg = d->ldg; p.ldr = d->ldr;
  p.M = d->M; p.F = d->F;
  p.relu = d->act1 == EG_ACT_RELU;
  p.res_in_lds = d->residual && d->residual == d->A && d->ldr == d->lda;
  p.dh = make_drop(d->drop_h_p, d->drop_h_site);
  p.dc1 = make_drop(d->drop_c1_p, d->drop_c1_site);
  p.dc2 = make_drop(d->drop_c2_p, d->drop_c2_site);
  p.gate_scale = d->gate_scale == 0.f ? 1.0f : d->gate_scale;
  p.ln_gamma = d->ln_gamma; p.ln_beta = d->ln_beta; p.LN_OUT = (T*)d->ln_out; p.ln_stats = d->ln_stats;
  return p;
}

template <typename T>
static int ffn_launch(const eg_ffn_desc* d, hipStream_t s) {
  const FfnArgs<T> p = ffn_make_args<T>(d);
  const FfnNoTail nt;
  const dim3 grid((d->M + FR - 1) / FR);
  // DROP (dropout on the hidden rows) is a template flag: a run-time test inside the kernel splits the merged phase's scheduling regions
#define FFN_LAUNCH_K(G_, B_, E_, L_, K_, T_, Q_)                                                                  \
  do {                                                                                                            \
    if (p.dh.thresh) eg_launch_lds<ffn_chain_kernel<T, G_, B_, E_, L_, K_, T_, true>, F_LDS>(grid, dim3(256), s, p, Q_);  \
    else eg_launch_lds<ffn_chain_kernel<T, G_, B_, E_, L_, K_, T_, false>, F_LDS>(grid, dim3(256), s, p, Q_);             \
  } while (0)
#define FFN_LAUNCH(G_, B_, E_, L_) FFN_LAUNCH_K(G_, B_, E_, L_, true, false, nt)
  const int gsel = d->gate_bits_in ? 2 : d->gate ? 1 : 0;
  const bool bout = d->gate_bits_out != nullptr;
  const bool lnf = d->ln_out != nullptr;                                                                      // (forward form only, checked below)
  if (!d->H) FFN_LAUNCH_K(0, 0, 3, true, false, false, nt);                                                       // lean (forward form, LNF, no bits: checked below)
  else if (gsel == 0 && d->bias1 && p.relu) {                                                                 // the forward pass
    if (lnf) { if (bout) FFN_LAUNCH(0, 1, 3, true); else FFN_LAUNCH(0, 0, 3, true); }
    else { if (bout) FFN_LAUNCH(0, 1, 3, false); else FFN_LAUNCH(0, 0, 3, false); }
  }
  else if (gsel == 2 && !d->bias1 && !p.relu) FFN_LAUNCH(2, 0, 0, false);                                    // the backward pass
  else if (gsel == 1 && !d->bias1 && !p.relu) FFN_LAUNCH(1, 0, 0, false);
  else if (gsel == 2) FFN_LAUNCH(2, 0, 4, false);                                                             // anything else
  else if (gsel == 1) FFN_LAUNCH(1, 0, 4, false);
  else if (bout) FFN_LAUNCH(0, 1, 4, false);
  else FFN_LAUNCH(0, 0, 4, false);
  EG_LAUNCH_CHECK("ffn_chain");
  return 0;
}

// the backward form with the norm-1 tail: one instantiation per dtype
template <typename T>
static int ffn_tail_launch(const eg_ffn_desc* f, const eg_ln_bwd_proj_desc* n, hipStream_t s) {
  const FfnArgs<T> p = ffn_make_args<T>(f);
  const LnProjArgs<T> q = lp_make_args<T>(n);
  const dim3 grid((f->M + FR - 1) / FR);
  FFN_LAUNCH_K(2, 0, 0, false, true, true, q);
#undef FFN_LAUNCH
#undef FFN_LAUNCH_K
  EG_LAUNCH_CHECK("ffn_bwd_ln_proj");
  return 0;
}

// the descriptor's own checks, for eg_ffn_chain and (tail: H required, C optional) eg_ffn_bwd_ln_proj
static int ffn_check_desc(const eg_ffn_desc* d, const char* who, bool tail) {
  EG_CHECK(d && d->A && d->W1 && d->W2, "%s: null operand", who);
  EG_CHECK(d->dtype == EG_BF16 || d->dtype == EG_F16, "%s: 16-bit compute dtypes only (got %d)", who, d->dtype);
  const bool lean = !tail && !d->H && !d->C;
  EG_CHECK(tail || lean || (d->H && d->C), "%s: H and C are both given (the keeping form) or both null (the lean form); got %s only", who,
           d->H ? "H" : "C");
  EG_CHECK(!lean || (d->bias1 && d->act1 == EG_ACT_RELU && !d->gate && !d->gate_bits_in),
           "%s: the lean form (H and C null) serves the forward form only: bias1, ReLU, no gate, no gate_bits_in", who);
  EG_CHECK(!lean || d->ln_out, "%s: the lean form (H and C null) needs ln_out, its only result", who);
  EG_CHECK(!lean || !d->gate_bits_out, "%s: the lean form (H and C null) writes no gate_bits_out", who);
  EG_CHECK(d->M > 0 && d->F > 0 && d->F % FC == 0, "%s: M=%d, F=%d (F must be a multiple of %d)", who, d->M, d->F, FC);
  EG_CHECK(d->act1 == EG_ACT_NONE || d->act1 == EG_ACT_RELU, "%s: act1 %d", who, d->act1);
  EG_CHECK(d->lda >= FD && d->lda % 8 == 0 && (lean || (d->ldh >= d->F && d->ldh % 8 == 0 && (!d->C || (d->ldc >= FD && d->ldc % 8 == 0)))),
           "%s: row strides must be 16-B multiples covering the rows", who);
  EG_CHECK(!d->gate || (d->ldg >= d->F && d->ldg % 4 == 0), "%s: gate stride", who);
  EG_CHECK(!(d->gate_bits_out && (d->gate_bits_in || d->gate)), "%s: a launch either writes gate bits or applies a gate", who);
  EG_CHECK(((uintptr_t)d->gate_bits_in | (uintptr_t)d->gate_bits_out) % 8 == 0, "%s: gate bit words must be 8-B aligned", who);
  EG_CHECK(!d->residual || (d->ldr >= FD && d->ldr % 8 == 0), "%s: residual stride", who);
  EG_CHECK((long long)d->M * d->F < (1ll << 32), "%s: M*F exceeds the 32-bit dropout index", who);
  EG_CHECK(!d->ln_out || (d->ln_gamma && d->ln_beta && (lean || d->ldc == FD) &&!d->gate && !d->gate_bits_in && d->bias1 && d->act1 == EG_ACT_RELU &&
                          (uintptr_t)d->ln_out % 16 == 0),
           "%s: the fused LayerNorm serves the forward form (bias + ReLU, no gate) with contiguous C rows", who);
  const float ps[3] = {d->drop_h_p, d->drop_c1_p, d->drop_c2_p};
  for (float q : ps) EG_CHECK(q >= 0.f && q < 1.f, "%s: dropout p", who);
  EG_CHECK((ps[0] == 0.f && ps[1] == 0.f && ps[2] == 0.f) || d->state, "%s: dropout needs a step state", who);
  EG_CHECK(((uintptr_t)d->A | (uintptr_t)d->W1 | (uintptr_t)d->W2 | (uintptr_t)d->H | (uintptr_t)d->C | (uintptr_t)d->gate |
            (uintptr_t)d->residual) % 16 == 0, "%s: operands must be 16-B aligned", who);
  return 0;
}

}  // namespace

extern "C" int eg_ffn_chain(const eg_ffn_desc* d, void* stream) {
  if (int rc = ffn_check_desc(d, "eg_ffn_chain", false)) return rc;
  hipStream_t s = (hipStream_t)stream;
  return eg_dispatch_16(d->dtype, [&](auto t) { return ffn_launch<typename decltype(t)::type>(d, s); });
}

extern "C" int eg_ffn_bwd_ln_proj(const eg_ffn_desc* f, const eg_ln_bwd_proj_desc* n, void* stream) {
  static const char who[] = "eg_ffn_bwd_ln_proj";
  EG_CHECK(f && n, "%s: null descriptor", who);
  if (int rc = ffn_check_desc(f, who, true)) return rc;
  if (int rc = lp_check_desc(n, who, false)) return rc;
  EG_CHECK(f->gate_bits_in, "%s: f must be the backward form: gate_bits_in is not set", who);
  EG_CHECK(!f->bias1 && f->act1 == EG_ACT_NONE && !f->gate && !f->gate_bits_out && !f->ln_out,
           "%s: f must be the backward form: no bias1, act1, gate, gate_bits_out or ln_out", who);
  EG_CHECK(f->H, "%s: f->H (the hidden gradient rows) must be given; only f->C may be NULL", who);
  EG_CHECK(!n->dy || n->dy == f->C, "%s: n->dy must be NULL or f->C (the LayerNorm reads the rows the launch itself completes)", who);
  EG_CHECK(n->M == f->M, "%s: n->M=%d differs from f->M=%d", who, n->M, f->M);
  EG_CHECK(n->dtype == f->dtype, "%s: n->dtype=%d differs from f->dtype=%d", who, n->dtype, f->dtype);
  hipStream_t s = (hipStream_t)stream;
  return eg_dispatch_16(f->dtype, [&](auto t) { return ffn_tail_launch<typename decltype(t)::type>(f, n, s); });
}

extern "C" int64_t eg_ffn_gate_bits_bytes(int M, int F) {
  if (M <= 0 || F <= 0) return 0;
  return (int64_t)((M + FR - 1) / FR) * (F / FC) * 256 * 8;
}
