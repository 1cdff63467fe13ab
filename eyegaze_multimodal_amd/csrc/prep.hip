// Staging kernels: input windows [B,C,T] -> channel-last padded rows, fp32 master parameters -> compute-dtype
// copies in the layouts the GEMMs read.  All HBM-bound, coalesced on both sides via an LDS transpose.
#include <stdarg.h>
#include <stdio.h>

#include <algorithm>
#include <cmath>

#include "rowtile.h"      // rt_frag_elem: the fragment order that modes 3-8 write

thread_local char eg_err_buf[512] = {0};
int eg_fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(eg_err_buf, sizeof(eg_err_buf), fmt, ap);
  va_end(ap);
  return 1;
}
extern "C" const char* eg_last_error(void) { return eg_err_buf; }
extern "C" int eg_abi_version(void) { return EG_ABI_VERSION; }
extern "C" int eg_device_info(int* cu_count, char* arch, int arch_len) {
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
    return eg_fail("eg_device_info: no HIP device");
  if (cu_count) *cu_count = prop.multiProcessorCount;
  if (arch && arch_len > 0) snprintf(arch, arch_len, "%s", prop.gcnArchName);
  return 0;
}

namespace {

// x [NB, C, T] f32 -> xt [NB, Tp, Cp]; one block = 256 consecutive padded time steps of one window
template <typename T>
__global__ __launch_bounds__(256) void window_pack_kernel(const float* __restrict__ x, T* __restrict__ xt, int C, int Tn,
                                                          int Cp, int pad_front, int Tp) {
  extern __shared__ float tile[];  // [256][Cp + 1]
  const int nb = blockIdx.y, tp0 = blockIdx.x * 256, tid = threadIdx.x;
  const int pitch = Cp + 1;
  const int t = tp0 + tid - pad_front;
  const bool tv = t >= 0 && t < Tn && tp0 + tid < Tp;
  const float* xb = x + (size_t)nb * C * Tn;
  for (int c = 0; c < Cp; ++c) tile[tid * pitch + c] = (tv && c < C) ? xb[(size_t)c * Tn + t] : 0.f;
  __syncthreads();
  const int rows = min(256, Tp - tp0);
  const int nchunk = rows * Cp / 8;
  T* ob = xt + ((size_t)nb * Tp + tp0) * Cp;
  for (int ch = tid; ch < nchunk; ch += 256) {
    const int e = ch * 8, r = e / Cp, c = e % Cp;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tile[r * pitch + c + j];
    store8(ob + e, v);
  }
}

template <typename T>
__global__ void cast_kernel(const float* __restrict__ src, T* __restrict__ dst, long long n) {
  const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i + 4 <= n) {
    float v[4];
    load4(src + i, v);
    store4(dst + i, v);
  } else {
    for (long long j = i; j < n; ++j) Elem<T>::st(dst + j, src[j]);
  }
}

// src [R, Cc] -> dst[c * ldd + r]
template <typename T>
__global__ __launch_bounds__(256) void transpose_cast_kernel(const float* __restrict__ src, T* __restrict__ dst, int R,
                                                             int Cc, int ldd) {
  __shared__ float tile[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int r = r0 + i, c = c0 + tx;
    tile[i][tx] = (r < R && c < Cc) ? src[(size_t)r * Cc + c] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, r = r0 + tx;
    if (c < Cc && r < R) Elem<T>::st(dst + (size_t)c * ldd + r, tile[tx][i]);
  }
}

// w [N, Cin, k] -> dst [N, Kp]: dst[n][tap*Cp + c] = w[n][c][tap]
template <typename T>
__global__ void pack_conv_weight_kernel(const float* __restrict__ w, T* __restrict__ dst, int N, int Cin, int k, int Cp,
                                        int Kp) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)N * Kp) return;
  const int n = (int)(i / Kp), kk = (int)(i % Kp);
  const int tap = kk / Cp, c = kk % Cp;
  const float v = (tap < k && c < Cin) ? w[((size_t)n * Cin + c) * k + tap] : 0.f;
  Elem<T>::st(dst + i, v);
}

// backward-data weights: dst[p][c][j*N + n] = w[n][c][s*(J-1-j) + p]   (0 when the tap index exceeds k-1)
template <typename T>
__global__ void pack_convT_weight_kernel(const float* __restrict__ w, T* __restrict__ dst, int N, int Cin, int k, int s,
                                         int J) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long per_phase = (long long)Cin * J * N;
  if (i >= per_phase * s) return;
  const int p = (int)(i / per_phase);
  const long long rem = i % per_phase;
  const int c = (int)(rem / (J * N));
  const int jn = (int)(rem % (J * N));
  const int j = jn / N, n = jn % N;
  const int tap = s * (J - 1 - j) + p;
  const float v = tap < k ? w[((size_t)n * Cin + c) * k + tap] : 0.f;
  Elem<T>::st(dst + i, v);
}

// table-driven parameter staging: ONE launch re-casts / transposes every weight of the model.
// mode 0: dst[i] = cast(src[i]) over rows*cols contiguous elements; mode 1: dst[c*ldd + r] = cast(src[r*cols + c]);
// mode 2: like 0 but the destination is fp32 (bias vectors gathered into fused buffers); modes 3-6: eg_ffn_chain's fragment
// order (16-bit dtypes).  Each block handles one 32x32 tile (mode 1), 1024 elements (modes 0/2) or 2048 elements (modes 3-6);
// blk0 is the entry's first block.
// one block of one table entry (modes 0-8); `lb` is the block's index within the entry.  Shared by pack_table_kernel and
// pack_table_ex_kernel, so both write the same bytes.
// the shifts by which a fragment-order mode decodes tile j, k-step s, wave and chunk from its destination index (in 8-element
// pieces) are those of rt_frag_elem<KS, TJ>
template <int KS, int TJ>
constexpr bool frag_shifts_ok(int sh_j, int sh_s, int sh_wn, int sh_c) {
  return rt_frag_elem<KS, TJ>(0, 0, 0, 1) == (size_t)8 << sh_j && rt_frag_elem<KS, TJ>(0, 0, 1, 0) == (size_t)8 << sh_s &&
         rt_frag_elem<KS, TJ>(0, 1, 0, 0) == (size_t)8 << sh_wn && rt_frag_elem<KS, TJ>(1, 0, 0, 0) == (size_t)8 << sh_c &&
         rt_frag_elem<KS, TJ>(0, 0, 0, 0, 1) == 8;
}
struct PackArgs {
  uint64_t src, dst;
  int rows, cols, ldd, mode;
};
template <typename T>
__device__ __forceinline__ void pack_block(const PackArgs& e, const int lb, float (*tile)[33]) {
  const float* src = (const float*)e.src;
  if (e.mode == 1) {
    const int tiles_c = (e.cols + 31) / 32;
    const int r0 = (lb / tiles_c) * 32, c0 = (lb % tiles_c) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
      const int r = r0 + i, c = c0 + tx;
      tile[i][tx] = (r < e.rows && c < e.cols) ? src[(size_t)r * e.cols + c] : 0.f;
    }
    __syncthreads();
    T* dst = (T*)e.dst;
    for (int i = ty; i < 32; i += 8) {
      const int c = c0 + i, r = r0 + tx;
      if (c < e.cols && r < e.rows) Elem<T>::st(dst + (size_t)c * e.ldd + r, tile[tx][i]);
    }
  } else if (e.mode == 7 || e.mode == 8) {
    // eg_attn_block_fwd's fragment order (16-bit dtypes), source fp32 [256, 256] = one of q_proj / k_proj / v_proj (mode 7, part
    // e.ldd = 0 / 1 / 2 into the shared [chunk c: 4][wave: 4][k-step s: 8][tile j: 3][lane] image, tile t = 3 wave + j of the chunk
    // = head t / 6, part (t % 6) / 2, half t % 2) or out_proj (mode 8: [chunk c: 4][wave: 4][k-step s: 2][tile j: 4][lane]).
    const int u = lb * 256 + threadIdx.x;                  // 8192 chunks of 8 elements per [256, 256] source
    const int lane = u & 63, l15 = lane & 15, g4 = lane >> 4;
    int n, k0;
    size_t q;                                              // destination element
    if (e.mode == 7) {
      const int s8 = (u >> 6) & 7, half = (u >> 9) & 1, th = (u >> 10) & 1, c = u >> 11;
      const int t = th * 6 + e.ldd * 2 + half, wn = t / 3, j = t % 3;
      n = (2 * c + th) * 32 + 16 * half + l15; k0 = 32 * s8 + 8 * g4;
      q = rt_frag_elem<8, 3>(c, wn, s8, j, lane);
    } else {
      static_assert(frag_shifts_ok<2, 4>(6, 8, 9, 11), "mode 8 decodes [chunk][wave][k-step: 2][tile: 4][lane]");
      const int j = (u >> 6) & 3, s2 = (u >> 8) & 1, wn = (u >> 9) & 3, c = u >> 11;
      n = 64 * wn + 16 * j + l15; k0 = 64 * c + 32 * s2 + 8 * g4;
      q = (size_t)u * 8;
    }
    if (u < 8192) {
      float v[8];
      load8(src + (size_t)n * 256 + k0, v);
      if constexpr (sizeof(T) == 2) store8((T*)e.dst + q, v);
    }
  } else if (e.mode >= 3 && e.mode <= 6) {
    // MFMA-fragment order of eg_ffn_chain's weights: destination chunk q (8 elements) is what lane q%64 of a wave loads as
    // its operand of one v_mfma_f32_16x16x32, so a fragment load is ONE contiguous 1-KB read.  The logical matrix is the source
    // (modes 3, 5) or its transpose (modes 4, 6); role 1 = [F, 256] (modes 3, 4), role 2 = [256, F] (modes 5, 6).
    const int q = lb * 256 + threadIdx.x;
    const bool tr = e.mode == 4 || e.mode == 6;
    const int lane = q & 63, l15 = lane & 15, g4 = lane >> 4;
    int n, k0, N, K;
    static_assert(frag_shifts_ok<8, 2>(6, 7, 10, 12) && frag_shifts_ok<4, 4>(6, 8, 10, 12), "the decodes below are rt_frag_elem's inverse");
    if (e.mode <= 4) {                       // role 1: [chunk c][wn][s: 8][j: 2][lane]
      const int j = (q >> 6) & 1, s8 = (q >> 7) & 7, wn = (q >> 10) & 3, c = q >> 12;
      n = 128 * c + 32 * wn + 16 * j + l15; k0 = 32 * s8 + 8 * g4;
      K = 256; N = tr ? e.cols : e.rows;
    } else {                                 // role 2: [chunk c][wn][s: 4][j: 4][lane]
      const int j = (q >> 6) & 3, s4 = (q >> 8) & 3, wn = (q >> 10) & 3, c = q >> 12;
      n = 64 * wn + 16 * j + l15; k0 = 128 * c + 32 * s4 + 8 * g4;
      N = 256; K = tr ? e.rows : e.cols;
    }
    if ((long long)q * 8 < (long long)e.rows * e.cols) {
      float v[8];
      if (!tr) load8(src + (size_t)n * K + k0, v);
      else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = src[(size_t)(k0 + i) * N + n];
      }
      if constexpr (sizeof(T) == 2) store8((T*)e.dst + (size_t)q * 8, v);
    }
  } else {
    const long long n = (long long)e.rows * e.cols;
    const long long i0 = (long long)lb * 1024 + threadIdx.x * 4;
    if (e.mode == 2) {
      float* dst = (float*)e.dst;
      for (long long i = i0; i < min(n, i0 + 4); ++i) dst[i] = src[i];
    } else {
      T* dst = (T*)e.dst;
      if (i0 + 4 <= n) {
        float v[4];
        load4(src + i0, v);
        store4(dst + i0, v);
      } else {
        for (long long i = i0; i < n; ++i) Elem<T>::st(dst + i, src[i]);
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void pack_table_kernel(const eg_pack_entry* __restrict__ tab, int nent) {
  __shared__ float tile[32][33];
  __shared__ int ent_s;
  const eg_pack_entry e = tab[eg_find_entry(tab, nent, (int)blockIdx.x, &ent_s)];
  const PackArgs a = {e.src, e.dst, e.rows, e.cols, e.ldd, e.mode};
  pack_block<T>(a, blockIdx.x - e.blk0, tile);
}

// eg_pack_table_ex: the modes above plus the two convolution weight layouts (1024 destination elements per block in the
// block count):
//   mode 9  = pack_conv_weight_kernel:  rows = N, cols = Cin, p0 = k, p1 = Cp, p2 = Kp
//   mode 10 = pack_convT_weight_kernel: rows = N, cols = Cin, p0 = k, p1 = stride, p2 = J
// Both go through LDS (the reverse of unpack_conv_wgrad_kernel): a block takes whole UNITS of the entry, strided by the
// entry's block count.  A unit's source is contiguous runs of w [N, Cin, k] and its destination is contiguous runs of dst;
// the (c, tap) -> (tap, c) / phase transposition is done by the LDS addressing.
//   mode 9 unit  = (n, CT channels): reads w[n][c0 .. c0+CT)[0 .. k), one run; writes k runs of CT at dst[n][tap*Cp + c0];
//                  the unit with c0 == 0 also zeroes the row's tail [k*Cp, Kp).
//   mode 10 unit = (32 rows n, CT channels): reads 32 runs of CT*k; writes stride*CT*J runs of 32 at dst[p][c][j*N + n0].
// A kernel size too long for the staging buffer takes the element-wise gather of the stand-alone kernels instead.
constexpr int PACK_STAGE = 4096;   // floats of LDS behind modes 9 / 10
constexpr int PACK_NT = 32;        // rows n of a mode-10 unit
template <typename T>
__global__ __launch_bounds__(256) void pack_table_ex_kernel(const eg_pack_entry_ex* __restrict__ tab, int nent) {
  __shared__ float stage[PACK_STAGE];
  __shared__ int ent_s;
  static_assert(PACK_STAGE >= 32 * 33, "modes 0-8 use the buffer as a [32][33] tile");
  const eg_pack_entry_ex e = tab[eg_find_entry(tab, nent, (int)blockIdx.x, &ent_s)];
  const int lb = blockIdx.x - e.blk0;
  if (e.mode < 9) {
    const PackArgs a = {e.src, e.dst, e.rows, e.cols, e.ldd, e.mode};
    pack_block<T>(a, lb, (float (*)[33])stage);
    return;
  }
  const float* w = (const float*)e.src;
  T* dst = (T*)e.dst;
  const int N = e.rows, Cin = e.cols, k = e.p0;
  const int ks = k | 1;   // odd pitch: lanes that walk c at a fixed tap hit distinct banks
  if (e.mode == 9) {
    const int Cp = e.p1, Kp = e.p2;
    const int CT = min(min(Cp, 64), PACK_STAGE / ks);
    if (CT > 0) {
      const int cchunks = (Cp + CT - 1) / CT;
      const long long units = (long long)N * cchunks;
      for (long long u = lb; u < units; u += e.nblk) {
        const int n = (int)(u / cchunks), c0 = (int)(u % cchunks) * CT;
        const int cn = min(CT, Cp - c0);              // destination channels of this unit
        const int cs = max(0, min(cn, Cin - c0));     // of which the source has this many
        const float* wr = w + ((size_t)n * Cin + c0) * k;
        for (int i = threadIdx.x; i < cs * k; i += 256) stage[(i / k) * ks + i % k] = wr[i];
        __syncthreads();
        T* dr = dst + (size_t)n * Kp;
        for (int i = threadIdx.x; i < cn * k; i += 256) {
          const int tap = i / cn, cc = i % cn;
          Elem<T>::st(dr + (size_t)tap * Cp + c0 + cc, cc < cs ? stage[cc * ks + tap] : 0.f);
        }
        if (c0 == 0)
          for (int i = k * Cp + threadIdx.x; i < Kp; i += 256) Elem<T>::st(dr + i, 0.f);
        __syncthreads();
      }
      return;
    }
    const long long total = (long long)N * Kp;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long i = (long long)lb * 1024 + u * 256 + threadIdx.x;
      if (i >= total) break;
      const int n = (int)(i / Kp), kk = (int)(i % Kp);
      const int tap = kk / Cp, c = kk % Cp;
      const float v = (tap < k && c < Cin) ? w[((size_t)n * Cin + c) * k + tap] : 0.f;
      Elem<T>::st(dst + i, v);
    }
  } else {
    const int s = e.p1, J = e.p2;
    constexpr int NP = PACK_NT + 1;   // stage[(cc*ks + tap)*NP + nn]: conflict-free on the way in and on the way out
    const int CT = min(min(Cin, 4), PACK_STAGE / (ks * NP));
    if (CT > 0) {
      const int cchunks = (Cin + CT - 1) / CT, nchunks = (N + PACK_NT - 1) / PACK_NT;
      const long long units = (long long)nchunks * cchunks;
      for (long long u = lb; u < units; u += e.nblk) {
        const int n0 = (int)(u / cchunks) * PACK_NT, c0 = (int)(u % cchunks) * CT;
        const int cn = min(CT, Cin - c0), nn_n = min(PACK_NT, N - n0);
        const int run = cn * k;                       // contiguous source floats per row n
        for (int i = threadIdx.x; i < nn_n * run; i += 256) {
          const int nn = i / run, r = i % run;
          stage[((r / k) * ks + r % k) * NP + nn] = w[((size_t)(n0 + nn) * Cin + c0) * k + r];
        }
        __syncthreads();
        const int per_c = J * nn_n, per_p = cn * per_c;
        for (int i = threadIdx.x; i < s * per_p; i += 256) {
          const int p = i / per_p, r = i % per_p;
          const int cc = r / per_c, jn = r % per_c;
          const int j = jn / nn_n, nn = jn % nn_n;
          const int tap = s * (J - 1 - j) + p;
          Elem<T>::st(dst + (((size_t)p * Cin + c0 + cc) * J + j) * N + n0 + nn, tap < k ? stage[(cc * ks + tap) * NP + nn] : 0.f);
        }
        __syncthreads();
      }
      return;
    }
    const long long per_phase = (long long)Cin * J * N;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long i = (long long)lb * 1024 + u * 256 + threadIdx.x;
      if (i >= per_phase * s) break;
      const int p = (int)(i / per_phase);
      const long long rem = i % per_phase;
      const int c = (int)(rem / (J * N));
      const int jn = (int)(rem % (J * N));
      const int j = jn / N, n = jn % N;
      const int tap = s * (J - 1 - j) + p;
      const float v = tap < k ? w[((size_t)n * Cin + c) * k + tap] : 0.f;
      Elem<T>::st(dst + i, v);
    }
  }
}

}  // namespace

// Host-side audit of an eg_pack_table_ex table (a HOST copy of it), run when the table is built: block ranges, per-mode shape
// rules, alignment, and -- wherever the caller states the extents of the buffers behind src / dst -- that no block reads or
// writes past them.  The convolution modes must state both extents.
extern "C" int eg_pack_table_ex_check(const eg_pack_entry_ex* table, int nentries, int dtype, int* total_blocks) {
  if (eg_dtype_check("eg_pack_table_ex_check", dtype, true)) return 1;
  EG_CHECK(table && nentries > 0 && total_blocks, "eg_pack_table_ex_check: bad arguments");
  long long blk = 0;
  for (int i = 0; i < nentries; ++i) {
    const eg_pack_entry_ex& e = table[i];
    EG_CHECK(e.src && e.dst, "eg_pack_table_ex_check: entry %d: null src / dst", i);
    EG_CHECK(e.rows > 0 && e.cols > 0, "eg_pack_table_ex_check: entry %d: bad shape rows=%d cols=%d", i, e.rows, e.cols);
    EG_CHECK(e.mode >= 0 && e.mode <= 10, "eg_pack_table_ex_check: entry %d: unknown mode %d", i, e.mode);
    EG_CHECK(e.src_elems >= 0 && e.dst_elems >= 0, "eg_pack_table_ex_check: entry %d: negative extent", i);
    const long long rc = (long long)e.rows * e.cols;
    long long need_src = rc, need_dst = rc, nblk = 0;
    unsigned src_al = 4, dst_al = 2;
    if (e.mode == 0 || e.mode == 2) {
      nblk = (rc + 1023) / 1024;
      if (e.mode == 0 && rc >= 4) { src_al = 16; dst_al = dtype == EG_F32 ? 16 : 8; }
      if (e.mode == 2) dst_al = 4;
    } else if (e.mode == 1) {
      EG_CHECK(e.ldd >= e.rows, "eg_pack_table_ex_check: entry %d: transpose ldd=%d < rows=%d", i, e.ldd, e.rows);
      nblk = (long long)((e.rows + 31) / 32) * ((e.cols + 31) / 32);
      need_dst = (long long)(e.cols - 1) * e.ldd + e.rows;
    } else if (e.mode <= 8) {
      EG_CHECK(dtype != EG_F32, "eg_pack_table_ex_check: entry %d: fragment mode %d needs a 16-bit dtype", i, e.mode);
      src_al = 16; dst_al = 16;
      nblk = rc / 2048;
      if (e.mode == 3 || e.mode == 6)
        EG_CHECK(e.cols == 256 && e.rows % 128 == 0, "eg_pack_table_ex_check: entry %d: mode %d needs src [F, 256], F %% 128 == 0", i, e.mode);
      else if (e.mode == 4 || e.mode == 5)
        EG_CHECK(e.rows == 256 && e.cols % 128 == 0, "eg_pack_table_ex_check: entry %d: mode %d needs src [256, F], F %% 128 == 0", i, e.mode);
      else {
        EG_CHECK(e.rows == 256 && e.cols == 256, "eg_pack_table_ex_check: entry %d: mode %d needs src [256, 256]", i, e.mode);
        if (e.mode == 7) {
          EG_CHECK(e.ldd >= 0 && e.ldd <= 2, "eg_pack_table_ex_check: entry %d: mode 7 part %d not in 0..2", i, e.ldd);
          need_dst = 3 * rc;      // the shared q|k|v image
        }
      }
    } else {
      const int N = e.rows, Cin = e.cols, k = e.p0;
      EG_CHECK(k > 0, "eg_pack_table_ex_check: entry %d: kernel size %d", i, k);
      EG_CHECK(e.src_elems > 0 && e.dst_elems > 0, "eg_pack_table_ex_check: entry %d: mode %d must state src_elems and dst_elems", i, e.mode);
      need_src = (long long)N * Cin * k;
      if (e.mode == 9) {
        const int Cp = e.p1, Kp = e.p2;
        EG_CHECK(Cp >= Cin && Kp >= (long long)k * Cp, "eg_pack_table_ex_check: entry %d: Cp=%d Kp=%d too small", i, Cp, Kp);
        need_dst = (long long)N * Kp;
      } else {
        const int s = e.p1, J = e.p2;
        EG_CHECK(s > 0 && J == (k + s - 1) / s, "eg_pack_table_ex_check: entry %d: stride=%d J=%d do not match k=%d", i, s, J, k);
        need_dst = (long long)s * Cin * J * N;
      }
      EG_CHECK(need_dst < (1ll << 31), "eg_pack_table_ex_check: entry %d: %lld destination elements", i, need_dst);
      nblk = (need_dst + 1023) / 1024;
    }
    EG_CHECK(nblk > 0 && e.nblk == nblk, "eg_pack_table_ex_check: entry %d: nblk=%d, mode %d at this shape takes %lld", i, e.nblk, e.mode, nblk);
    EG_CHECK(e.blk0 == blk, "eg_pack_table_ex_check: entry %d: blk0=%d, expected %lld", i, e.blk0, blk);
    EG_CHECK(e.src % src_al == 0 && e.dst % dst_al == 0, "eg_pack_table_ex_check: entry %d: alignment (mode %d)", i, e.mode);
    EG_CHECK(e.src_elems == 0 || need_src <= e.src_elems, "eg_pack_table_ex_check: entry %d: reads %lld elements of a %lld-element source",
             i, need_src, (long long)e.src_elems);
    EG_CHECK(e.dst_elems == 0 || need_dst <= e.dst_elems, "eg_pack_table_ex_check: entry %d: writes %lld elements of a %lld-element destination",
             i, need_dst, (long long)e.dst_elems);
    blk += nblk;
    EG_CHECK(blk < (1ll << 31), "eg_pack_table_ex_check: too many blocks");
  }
  *total_blocks = (int)blk;
  return 0;
}

extern "C" int eg_pack_table_ex(const eg_pack_entry_ex* table, int nentries, int total_blocks, int dtype, void* stream) {
  if (eg_dtype_check("eg_pack_table_ex", dtype, true)) return 1;
  EG_CHECK(table && nentries > 0 && total_blocks > 0, "eg_pack_table_ex: bad arguments");
  eg_dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(pack_table_ex_kernel<T>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, table, nentries);
  });
  EG_LAUNCH_CHECK("pack_table_ex");
  return 0;
}

extern "C" int eg_pack_table(const eg_pack_entry* table, int nentries, int total_blocks, int dtype, void* stream) {
  if (eg_dtype_check("eg_pack_table", dtype, true)) return 1;
  EG_CHECK(table && nentries > 0 && total_blocks > 0, "eg_pack_table: bad arguments");
  eg_dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(pack_table_kernel<T>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, table, nentries);
  });
  EG_LAUNCH_CHECK("pack_table");
  return 0;
}

extern "C" int eg_window_pack(const float* x, void* xt, int NB, int C, int T, int Cp, int pad_front, int Tp, int dtype,
                              void* stream) {
  if (eg_dtype_check("eg_window_pack", dtype, true)) return 1;
  EG_CHECK(x && xt, "eg_window_pack: null pointer");
  EG_CHECK(NB > 0 && C > 0 && T > 0, "eg_window_pack: bad shape NB=%d C=%d T=%d", NB, C, T);
  EG_CHECK(Cp >= C && Cp % 8 == 0 && Cp <= 256, "eg_window_pack: Cp=%d must be a multiple of 8 in [C, 256]", Cp);
  EG_CHECK(pad_front >= 0 && Tp >= T + pad_front, "eg_window_pack: Tp=%d < T+pad_front", Tp);
  dim3 grid((Tp + 255) / 256, NB);
  const size_t lds = 256 * (Cp + 1) * sizeof(float);
  eg_dispatch_dtype(dtype, [&](auto t) {
    using E = typename decltype(t)::type;      // (T is the window length here)
    hipLaunchKernelGGL(window_pack_kernel<E>, grid, dim3(256), lds, (hipStream_t)stream, x, (E*)xt, C, T, Cp, pad_front, Tp);
  });
  EG_LAUNCH_CHECK("window_pack");
  return 0;
}

extern "C" int eg_cast(const float* src, void* dst, int64_t n, int dtype, void* stream) {
  if (eg_dtype_check("eg_cast", dtype, true)) return 1;
  EG_CHECK(src && dst && n > 0, "eg_cast: bad arguments");
  EG_CHECK(((uintptr_t)src % 16 == 0) && ((uintptr_t)dst % 8 == 0), "eg_cast: alignment");
  const long long nt = (n + 3) / 4;
  dim3 grid((unsigned)((nt + 255) / 256));
  eg_dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(cast_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, src, (T*)dst, (long long)n);
  });
  EG_LAUNCH_CHECK("cast");
  return 0;
}

extern "C" int eg_transpose_cast(const float* src, void* dst, int R, int Cc, int ldd, int dtype, void* stream) {
  if (eg_dtype_check("eg_transpose_cast", dtype, true)) return 1;
  EG_CHECK(src && dst && R > 0 && Cc > 0 && ldd >= R, "eg_transpose_cast: bad arguments");
  dim3 grid((Cc + 31) / 32, (R + 31) / 32);
  eg_dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(transpose_cast_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, src, (T*)dst, R, Cc, ldd);
  });
  EG_LAUNCH_CHECK("transpose_cast");
  return 0;
}

extern "C" int eg_pack_conv_weight(const float* w, void* dst, int N, int Cin, int k, int Cp, int Kp, int dtype,
                                   void* stream) {
  if (eg_dtype_check("eg_pack_conv_weight", dtype, true)) return 1;
  EG_CHECK(w && dst && N > 0 && Cin > 0 && k > 0, "eg_pack_conv_weight: bad arguments");
  EG_CHECK(Cp >= Cin && Kp >= k * Cp, "eg_pack_conv_weight: Cp=%d Kp=%d too small", Cp, Kp);
  const long long n = (long long)N * Kp;
  dim3 grid((unsigned)((n + 255) / 256));
  eg_dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(pack_conv_weight_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, w, (T*)dst, N, Cin, k, Cp, Kp);
  });
  EG_LAUNCH_CHECK("pack_conv_weight");
  return 0;
}

extern "C" int eg_pack_convT_weight(const float* w, void* dst, int N, int Cin, int k, int stride, int dtype,
                                    void* stream) {
  if (eg_dtype_check("eg_pack_convT_weight", dtype, true)) return 1;
  EG_CHECK(w && dst && N > 0 && Cin > 0 && k > 0 && stride > 0, "eg_pack_convT_weight: bad arguments");
  const int J = (k + stride - 1) / stride;
  const long long n = (long long)stride * Cin * J * N;
  dim3 grid((unsigned)((n + 255) / 256));
  eg_dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(pack_convT_weight_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, w, (T*)dst, N, Cin, k, stride, J);
  });
  EG_LAUNCH_CHECK("pack_convT_weight");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Window normalisation of the data path (1_Data/processed/dual_eeg_dataset.py:142-168, 194-202).
//   raw [N, 2, C, T] f32 (window n: player-1 channels then player-2 channels, as the shards store them)
//   -> eeg1 [N, C, T], eeg2 [N, C, T] f32
//   mode 0 (enable_preprocessing = False, the yaml default): (x - mean(x)) / (std_pop(x) + 1e-8) over the whole window
//   mode 1 (enable_preprocessing = True): common-average reference (subtract the channel mean at every time step),
//          then per-channel (v - mean) / (std_pop + 1e-8)
// One block per (window, player).  Sums run in double: the reference reduces in float32 with pairwise summation, a
// double accumulator is at least as accurate, and the pass is bandwidth-bound either way (three reads from L2, one write).
// ---------------------------------------------------------------------------------------------
namespace {

__device__ __forceinline__ double block_sum_d(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];
  return s;
}

// How a (window, player)'s C channel rows of T floats are addressed.  window_normalize_rows below is written once against
// this interface, so the two launches share every load order, accumulator and reduction (bit-equal outputs).
//   flat element e = c * T + t of the window; a cursor walks e = threadIdx.x, threadIdx.x + blockDim.x, ...
struct ContiguousRows {            // rows back to back: the shards' [C, T] window
  const float* x;
  int T;
  struct Cursor { long long e; };
  __device__ __forceinline__ Cursor begin() const { return {(long long)threadIdx.x}; }
  __device__ __forceinline__ void next(Cursor& p) const { p.e += blockDim.x; }
  __device__ __forceinline__ float at(const Cursor& p) const { return x[p.e]; }
  __device__ __forceinline__ const float* row(int c) const { return x + (long long)c * T; }
};
struct StridedRows {               // rows `ld` floats apart: a window inside a recording of the resident store
  const float* x;
  long long ld;
  int T;
  struct Cursor { long long e; long long off; int t; };   // off = c * ld + t for e = c * T + t
  __device__ __forceinline__ Cursor begin() const {
    Cursor p = {(long long)threadIdx.x, 0, (int)threadIdx.x};
    while (p.t >= T) p.t -= T, p.off += ld;
    p.off += p.t;
    return p;
  }
  __device__ __forceinline__ void next(Cursor& p) const {
    p.e += blockDim.x;
    p.off += blockDim.x;
    p.t += blockDim.x;
    while (p.t >= T) p.t -= T, p.off += ld - T;
  }
  __device__ __forceinline__ float at(const Cursor& p) const { return x[p.off]; }
  __device__ __forceinline__ const float* row(int c) const { return x + (long long)c * ld; }
};

template <class Rows>
__device__ __forceinline__ void window_normalize_rows(const Rows in, float* __restrict__ y, int C, int T, int mode, float* car,
                                                      double* red) {
  const long long CT = (long long)C * T;
  if (mode == 2) {            // eg_window_cut: the window as stored
    for (auto p = in.begin(); p.e < CT; in.next(p)) y[p.e] = in.at(p);
    return;
  }
  if (mode == 0) {
    double s = 0.0;
    for (auto p = in.begin(); p.e < CT; in.next(p)) s += (double)in.at(p);
    const double mean = block_sum_d(s, red) / (double)CT;
    const float meanf = (float)mean;
    double q = 0.0;
    for (auto p = in.begin(); p.e < CT; in.next(p)) {
      const double d = (double)in.at(p) - mean;
      q += d * d;
    }
    const float stdf = (float)sqrt(block_sum_d(q, red) / (double)CT);
    const float den = stdf + 1e-8f;
    for (auto p = in.begin(); p.e < CT; in.next(p)) y[p.e] = (in.at(p) - meanf) / den;
    return;
  }
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += in.row(c)[t];
    car[t] = s / (float)C;
  }
  __syncthreads();
  for (int c = 0; c < C; ++c) {
    const float* xc = in.row(c);
    double s = 0.0;
    for (int t = threadIdx.x; t < T; t += blockDim.x) s += (double)(xc[t] - car[t]);
    const double mean = block_sum_d(s, red) / (double)T;
    const float meanf = (float)mean;
    double q = 0.0;
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
      const double d = (double)(xc[t] - car[t]) - mean;
      q += d * d;
    }
    const float den = (float)sqrt(block_sum_d(q, red) / (double)T) + 1e-8f;
    for (int t = threadIdx.x; t < T; t += blockDim.x) y[(long long)c * T + t] = ((xc[t] - car[t]) - meanf) / den;
  }
}

__global__ __launch_bounds__(256) void window_normalize_kernel(const float* __restrict__ raw, float* __restrict__ eeg1,
                                                               float* __restrict__ eeg2, int C, int T, int mode) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double red[4];
  const int n = blockIdx.x >> 1, who = blockIdx.x & 1;
  const long long CT = (long long)C * T;
  const ContiguousRows in = {raw + ((long long)n * 2 + who) * CT, T};
  window_normalize_rows(in, (who ? eeg2 : eeg1) + (long long)n * CT, C, T, mode, (float*)smem /* [T] (mode 1) */, red);
}

// The same arithmetic on windows cut out of device-resident recordings (include/eyegaze_hip.h: eg_window_gather).  One block
// per (batch window, player); the tables are trusted (data.validate_store checks them once, on the host); every offset is 64-bit
// and every access a 4-byte one, since a row may start at any float of the store.
__global__ __launch_bounds__(256) void window_gather_kernel(const eg_window_gather_desc d, const int32_t* __restrict__ order,
                                                            int first, float* __restrict__ eeg1, float* __restrict__ eeg2,
                                                            int64_t* __restrict__ labels, int mode) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double red[4];
  const int j = blockIdx.x >> 1, who = blockIdx.x & 1;
  const int w = order[(long long)first + j];
  const int p = d.win_pair[w];
  const long long len = d.pair_len[p];
  const StridedRows in = {d.data + d.pair_off[p] + (long long)who * d.C * len + d.win_start[w], len, d.T};
  if (labels && who == 0 && threadIdx.x == 0) labels[j] = d.win_label[w];
  window_normalize_rows(in, (who ? eeg2 : eeg1) + (long long)j * d.C * d.T, d.C, d.T, mode, (float*)smem, red);
}

}  // namespace

// mode 0 / 1: eg_window_gather's; 2: eg_window_cut's copy (no entry point passes a mode it has not checked)
static int window_gather_launch(const eg_window_gather_desc* d, const int32_t* order, int first, int n, float* eeg1, float* eeg2,
                                int64_t* labels, int mode, void* stream) {
  hipLaunchKernelGGL(window_gather_kernel, dim3(2 * n), dim3(256), mode == 1 ? (size_t)d->T * 4 : 0, (hipStream_t)stream, *d, order,
                     first, eeg1, eeg2, labels, mode);
  EG_LAUNCH_CHECK("window_gather");
  return 0;
}

extern "C" int eg_window_normalize(const float* raw, float* eeg1, float* eeg2, int N, int C, int T, int mode, void* stream) {
  EG_CHECK(raw && eeg1 && eeg2, "eg_window_normalize: null pointer");
  EG_CHECK(N > 0 && C > 0 && T > 0, "eg_window_normalize: bad shape N=%d C=%d T=%d", N, C, T);
  EG_CHECK(mode == 0 || mode == 1, "eg_window_normalize: mode %d (0 = window z-score, 1 = CAR + channel z-score)", mode);
  EG_CHECK(T <= 16384, "eg_window_normalize: T=%d exceeds the 16384-sample staging row", T);
  hipLaunchKernelGGL(window_normalize_kernel, dim3(2 * N), dim3(256), mode ? (size_t)T * 4 : 0, (hipStream_t)stream, raw, eeg1,
                     eeg2, C, T, mode);
  EG_LAUNCH_CHECK("window_normalize");
  return 0;
}

extern "C" int eg_window_gather(const eg_window_gather_desc* d, const int32_t* order, int order_len, int first, int n, float* eeg1,
                                float* eeg2, int64_t* labels, int mode, void* stream) {
  EG_CHECK(d && d->data && d->pair_off && d->pair_len && d->win_pair && d->win_start && order && eeg1 && eeg2,
           "eg_window_gather: null pointer");
  EG_CHECK(n > 0 && d->C > 0 && d->T > 0, "eg_window_gather: bad shape n=%d C=%d T=%d", n, d->C, d->T);
  EG_CHECK(d->n_pairs > 0 && d->n_windows > 0, "eg_window_gather: empty tables (n_pairs=%d n_windows=%d)", d->n_pairs, d->n_windows);
  EG_CHECK(mode == 0 || mode == 1, "eg_window_gather: mode %d (0 = window z-score, 1 = CAR + channel z-score)", mode);
  EG_CHECK(d->T <= 16384, "eg_window_gather: T=%d exceeds the 16384-sample staging row", d->T);
  EG_CHECK(first >= 0 && (long long)first + n <= (long long)order_len, "eg_window_gather: windows [%d, %d + %d) outside the order of %d",
           first, first, n, order_len);
  EG_CHECK(!labels || d->win_label, "eg_window_gather: labels requested but the descriptor has no win_label");
  return window_gather_launch(d, order, first, n, eeg1, eeg2, labels, mode, stream);
}

extern "C" int eg_window_cut(const eg_window_gather_desc* d, const int32_t* order, int order_len, int first, int n, float* eeg1,
                             float* eeg2, int64_t* labels, void* stream) {
  EG_CHECK(d && d->data && d->pair_off && d->pair_len && d->win_pair && d->win_start && order && eeg1 && eeg2,
           "eg_window_cut: null pointer");
  EG_CHECK(n > 0 && d->C > 0 && d->T > 0, "eg_window_cut: bad shape n=%d C=%d T=%d", n, d->C, d->T);
  EG_CHECK(d->n_pairs > 0 && d->n_windows > 0, "eg_window_cut: empty tables (n_pairs=%d n_windows=%d)", d->n_pairs, d->n_windows);
  EG_CHECK(d->T <= 16384, "eg_window_cut: T=%d exceeds the 16384-sample staging row", d->T);
  EG_CHECK(first >= 0 && (long long)first + n <= (long long)order_len, "eg_window_cut: windows [%d, %d + %d) outside the order of %d",
           first, first, n, order_len);
  EG_CHECK(!labels || d->win_label, "eg_window_cut: labels requested but the descriptor has no win_label");
  return window_gather_launch(d, order, first, n, eeg1, eeg2, labels, 2 /* internal: as stored */, stream);
}

// ---------------------------------------------------------------------------------------------
// Window augmentation of the training forward (include/eyegaze_hip.h: eg_window_augment states the index formulas): Gaussian
// noise, channel dropout, time masks, all drawn from eg_hash -- the seed comes from eg_step_state, so a captured launch draws
// anew at every replay.  Streaming: one WAVE takes AUG_SPAN consecutive samples of one row (player, window, channel), so the
// row's drop decision and the window's at most 8 mask intervals are wave-uniform (scalar registers), computed once per unit.
// A dropped row is written without being read; a 16-byte chunk that lies inside a mask is neither read nor given noise.
// Every element is read and written by the same lane, so out may alias in.
// ---------------------------------------------------------------------------------------------
namespace {

constexpr uint32_t AUG_SPAN = 1024;   // samples per unit: 4 rounds of 16 bytes per lane (VEC), 16 rounds of 4 bytes otherwise

struct AugMasks {
  uint32_t start[8], len[8];          // len 0: unused
};
__device__ __forceinline__ bool aug_masked(const AugMasks& m, uint32_t t) {
  bool z = false;
#pragma unroll
  for (int j = 0; j < 8; ++j) z |= (t - m.start[j]) < m.len[j];
  return z;
}
// Box-Muller on pair q of the flat element index: n0 for the even element, n1 for the odd one
__device__ __forceinline__ void aug_noise_pair(uint32_t lo, uint32_t hi, uint32_t q, float& n0, float& n1) {
  const float u1 = ((float)(eg_hash(lo, hi, EG_SITE_AUG_NOISE_R, q) >> 9) + 0.5f) * 0x1p-23f;
  const float u2 = (float)(eg_hash(lo, hi, EG_SITE_AUG_NOISE_T, q) >> 8) * 0x1p-24f;
  const float r = sqrtf(-2.0f * logf(u1));
  float s, c;
  sincospif(2.0f * u2, &s, &c);
  n0 = __fmul_rn(r, c);
  n1 = __fmul_rn(r, s);
}

// VEC: T % 4 == 0 and 16-byte aligned buffers, so every row starts on a 16-byte boundary and on an even flat index
template <bool VEC>
__global__ __launch_bounds__(256) void window_augment_kernel(const float* in1, const float* in2, float* out1, float* out2, int N,
                                                             int C, int T, float noise_std, uint32_t chan_thresh, int n_masks,
                                                             int mask_max_len, const eg_step_state* __restrict__ state) {
  const uint32_t lo = state->seed_lo, hi = state->seed_hi;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t NC = (uint32_t)N * (uint32_t)C;                  // rows per player; 2 NC T < 2^32 (host check)
  const uint32_t Tn = (uint32_t)T, segs = (Tn + AUG_SPAN - 1) / AUG_SPAN;
  const uint64_t units = 2ull * NC * segs;                        // <= 2 NC T
  const uint32_t Lm = min((uint32_t)mask_max_len, Tn);
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + wave; u < units; u += (uint64_t)gridDim.x * 4) {
    const uint32_t row = (uint32_t)u / segs, seg = (uint32_t)u % segs;
    const uint32_t pl = row >= NC ? 1u : 0u, rp = row - pl * NC, w = rp / (uint32_t)C;
    const float* src = (pl ? in2 : in1) + (size_t)rp * Tn;
    float* dst = (pl ? out2 : out1) + (size_t)rp * Tn;
    const uint32_t e0 = row * Tn;                                 // flat index of the row's first sample
    const uint32_t t0 = seg * AUG_SPAN, t1 = min(t0 + AUG_SPAN, Tn);
    bool dropped = false;
    if (chan_thresh) {
      const uint32_t h = eg_hash(lo, hi, EG_SITE_AUG_CHAN, row >> 1);
      dropped = ((row & 1u) ? (h >> 16) : (h & 0xFFFFu)) < chan_thresh;
    }
    if (dropped) {
      if (VEC) {
        for (uint32_t t = t0 + lane * 4; t < t1; t += 256) *(f32x4*)(dst + t) = (f32x4){0.f, 0.f, 0.f, 0.f};
      } else {
        for (uint32_t t = t0 + lane; t < t1; t += 64) dst[t] = 0.f;
      }
      continue;
    }
    AugMasks m;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      m.start[j] = m.len[j] = 0;
      if (j < n_masks) {
        const uint32_t h = eg_hash(lo, hi, EG_SITE_AUG_TIME, w * 8u + j);
        m.len[j] = 1u + (uint32_t)(((uint64_t)(h & 0xFFFFu) * Lm) >> 16);
        m.start[j] = (uint32_t)(((uint64_t)(h >> 16) * (Tn - m.len[j] + 1u)) >> 16);
      }
    }
    if (VEC) {
      for (uint32_t t = t0 + lane * 4; t < t1; t += 256) {
        bool z[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) z[i] = aug_masked(m, t + i);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (!(z[0] && z[1] && z[2] && z[3])) {
          v = *(const f32x4*)(src + t);
          if (noise_std > 0.f) {
            const uint32_t q = (e0 + t) >> 1;
            float n[4];
            aug_noise_pair(lo, hi, q, n[0], n[1]);
            aug_noise_pair(lo, hi, q + 1, n[2], n[3]);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = __fmaf_rn(noise_std, n[i], v[i]);
          }
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (z[i]) v[i] = 0.f;
        }
        *(f32x4*)(dst + t) = v;
      }
    } else {
      for (uint32_t t = t0 + lane; t < t1; t += 64) {
        float v = 0.f;
        if (!aug_masked(m, t)) {
          v = src[t];
          if (noise_std > 0.f) {
            const uint32_t e = e0 + t;
            float n0, n1;
            aug_noise_pair(lo, hi, e >> 1, n0, n1);
            v = __fmaf_rn(noise_std, (e & 1u) ? n1 : n0, v);
          }
        }
        dst[t] = v;
      }
    }
  }
}

}  // namespace

extern "C" int eg_window_augment(const float* in1, const float* in2, float* out1, float* out2, int N, int C, int T, float noise_std,
                                 float chan_drop_p, int n_masks, int mask_max_len, const eg_step_state* state, void* stream) {
  EG_CHECK(in1 && in2 && out1 && out2, "eg_window_augment: null pointer (in1=%p in2=%p out1=%p out2=%p)", (const void*)in1,
           (const void*)in2, (void*)out1, (void*)out2);
  EG_CHECK(state, "eg_window_augment: null state (the seed is read from eg_step_state)");
  EG_CHECK(N > 0 && C > 0 && T > 0, "eg_window_augment: bad shape N=%d C=%d T=%d", N, C, T);
  EG_CHECK(std::isfinite(noise_std) && noise_std >= 0.f, "eg_window_augment: noise_std=%g must be finite and >= 0", (double)noise_std);
  EG_CHECK(chan_drop_p >= 0.f && chan_drop_p < 1.f, "eg_window_augment: chan_drop_p=%g outside [0, 1)", (double)chan_drop_p);
  EG_CHECK(n_masks >= 0 && n_masks <= 8, "eg_window_augment: n_masks=%d outside [0, 8]", n_masks);
  EG_CHECK(n_masks == 0 || mask_max_len >= 1, "eg_window_augment: mask_max_len=%d must be >= 1 when n_masks > 0", mask_max_len);
  const long long nc = (long long)N * C;
  EG_CHECK(nc < (1ll << 31) && 2 * nc * T < (1ll << 32), "eg_window_augment: 2*N*C*T = 2*%d*%d*%d does not fit 32-bit element indices",
           N, C, T);
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    hipDeviceProp_t prop;
    const bool ok = hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess;
    cus = ok && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  // memory-bound: 8 blocks (32 waves) per CU cover the chip, the unit-stride loop takes the rest
  const long long units = 2 * nc * ((T + (long long)AUG_SPAN - 1) / AUG_SPAN);
  const dim3 gd((unsigned)std::min<long long>((units + 3) / 4, 8ll * cus)), bd(256);
  const uint32_t thresh = make_drop(chan_drop_p, EG_SITE_AUG_CHAN).thresh;
  const bool vec = T % 4 == 0 && ((uintptr_t)in1 | (uintptr_t)in2 | (uintptr_t)out1 | (uintptr_t)out2) % 16 == 0;
  if (vec)
    hipLaunchKernelGGL(window_augment_kernel<true>, gd, bd, 0, (hipStream_t)stream, in1, in2, out1, out2, N, C, T, noise_std, thresh,
                       n_masks, mask_max_len, state);
  else
    hipLaunchKernelGGL(window_augment_kernel<false>, gd, bd, 0, (hipStream_t)stream, in1, in2, out1, out2, N, C, T, noise_std, thresh,
                       n_masks, mask_max_len, state);
  EG_LAUNCH_CHECK("window_augment");
  return 0;
}
