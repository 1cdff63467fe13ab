// Recording-level preprocessing of the data path (2_Preprocessing/scripts/preprocess_eeg_windows.py:145-172): zero-phase
// Butterworth band-pass (scipy.signal.filtfilt, restated), common-average reference and per-channel z-score over WHOLE recordings
// that already lie in device memory, in place.  include/eyegaze_hip.h states the contracts; DESIGN.md §8l the layout and numbers.
#include <algorithm>

#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// filtfilt.  The recurrence is sequential in time and is NOT reformulated (its fp64 rounding is the specification: the poles of
// a 0.5 Hz edge sit at z ~ 1), so the parallelism is over rows: one lane owns one row, one wave = one block takes 64 consecutive
// rows.  Samples move through LDS in tiles of RP_TT time steps: global reads and writes run along time (lane = time step, one
// row after the other), the recurrence reads and writes the tile transposed (lane = row).  A tile row is RP_TT + 1 elements, an
// odd stride: lane r at a fixed t hits bank (r + t) % 32 for floats and the bank pair starting at 2 (r + t) % 64 for doubles --
// all distinct within a 32-lane half.  The extension is computed from the row when a tile is loaded.
// ---------------------------------------------------------------------------------------------
constexpr int RP_ROWS = 64;            // rows per block = lanes of the wave
constexpr int RP_TT = 64;              // time steps per tile
constexpr int RP_LD = RP_TT + 1;
constexpr int RP_MAXC = 17;            // coefficients: ncoef in [2, RP_MAXC]

struct IirCoef {                       // zero-padded behind ncoef: the padded recurrence gives the same bits (x + 0 = x)
  double b[RP_MAXC], a[RP_MAXC], zi[RP_MAXC - 1];
};

// scipy's transposed direct form II, NS = number of states kept in registers.  EXACT: every product and sum rounded on its own, as
// scipy's compiled loop rounds them; otherwise the compiler contracts them into multiply-adds.  Both are correct to fp64, but the
// recurrence amplifies the difference by the filter's conditioning: for the 0.5-50 Hz band it stays below the f32 output's rounding,
// for a 0.5-4 Hz band at 250 Hz it reaches 1e-4 of the signal.
template <int NS, bool EXACT>
struct Tdf2 {
  double z[NS];
  __device__ __forceinline__ void start(const IirCoef& k, double x0) {
#pragma unroll
    for (int i = 0; i < NS; ++i) z[i] = k.zi[i] * x0;
  }
  __device__ __forceinline__ double step(const IirCoef& k, double x) {
    if (EXACT) {
#pragma clang fp contract(off)
      const double y = z[0] + k.b[0] * x;
#pragma unroll
      for (int i = 0; i < NS - 1; ++i) z[i] = z[i + 1] + k.b[i + 1] * x - k.a[i + 1] * y;
      z[NS - 1] = k.b[NS] * x - k.a[NS] * y;
      return y;
    }
    const double y = z[0] + k.b[0] * x;
#pragma unroll
    for (int i = 0; i < NS - 1; ++i) z[i] = z[i + 1] + k.b[i + 1] * x - k.a[i + 1] * y;
    z[NS - 1] = k.b[NS] * x - k.a[NS] * y;
    return y;
  }
};

// sample e of row x (L samples, first x0, last xl) extended oddly by pad on both sides, formed in f32 as scipy forms it for an
// f32 input; L > pad.  One load and no branch, so that a tile's loads of all rows are in flight together.
__device__ __forceinline__ float odd_ext(const float* __restrict__ x, float x0, float xl, int L, int pad, int e) {
  const int t = e - pad;
  const float v = x[t < 0 ? -t : t < L ? t : 2 * L - 2 - t];
  return t < 0 ? 2.f * x0 - v : t < L ? v : 2.f * xl - v;
}

template <int NS, bool EXACT>
__global__ __launch_bounds__(RP_ROWS) void recording_filtfilt_kernel(const eg_recording_rows_desc d, const IirCoef k, const int pad,
                                                                     double* __restrict__ ws) {
  __shared__ float ftile[RP_ROWS * RP_LD];
  __shared__ double dtile[RP_ROWS * RP_LD];
  __shared__ long long s_off[RP_ROWS], s_wso[RP_ROWS];
  __shared__ int s_ext[RP_ROWS];                       // extended length of the block's row, 0 for a row that is not there
  __shared__ float s_x0[RP_ROWS], s_xl[RP_ROWS];       // the row's first and last sample: the odd extension's pivots
  const int lane = threadIdx.x;
  const long long row = (long long)blockIdx.x * RP_ROWS + lane;
  int len = 0;
  if (row < d.n_rows) len = d.row_len[row];
  const int E = len > pad ? len + 2 * pad : 0;         // (a row no longer than the padding is the wrapper's ValueError)
  s_ext[lane] = E;
  s_off[lane] = E ? d.row_off[row] : 0;                // a row that is not there points at float 0 / double 0, never read past
  s_wso[lane] = E ? d.ws_off[row] : 0;
  s_x0[lane] = E ? d.data[s_off[lane]] : 0.f;
  s_xl[lane] = E ? d.data[s_off[lane] + len - 1] : 0.f;
  __syncthreads();
  int Emax = 0;
  for (int i = 0; i < RP_ROWS; ++i) Emax = max(Emax, s_ext[i]);
  if (Emax == 0) return;

  Tdf2<NS, EXACT> f;
  double ylast = 0.0;
  // forward: extended row -> workspace (fp64).  The next tile's loads are requested before this tile's recurrence and held in
  // registers, so their latency passes under it: one wave has nobody else to hide it.
  float pre_f[RP_ROWS];
  const auto request_fwd = [&](int t0) {       // unconditional: a lane past the row's end reads the row's (or the store's) first float
    const int e = t0 + lane;
#pragma unroll
    for (int rr = 0; rr < RP_ROWS; ++rr) {
      const int Er = s_ext[rr];
      pre_f[rr] = odd_ext(d.data + s_off[rr], s_x0[rr], s_xl[rr], max(Er - 2 * pad, 1), pad, e < Er ? e : pad);
    }
  };
  request_fwd(0);
  for (int t0 = 0; t0 < Emax; t0 += RP_TT) {
    const int e = t0 + lane;
#pragma unroll
    for (int rr = 0; rr < RP_ROWS; ++rr) ftile[rr * RP_LD + lane] = pre_f[rr];
    __syncthreads();
    if (t0 + RP_TT < Emax) request_fwd(t0 + RP_TT);
    for (int t = 0; t < RP_TT; ++t) {
      if (t0 + t < E) {
        const double x = (double)ftile[lane * RP_LD + t];
        if (t0 + t == 0) f.start(k, x);
        ylast = f.step(k, x);
        dtile[lane * RP_LD + t] = ylast;
      }
    }
    __syncthreads();
#pragma unroll 8
    for (int rr = 0; rr < RP_ROWS; ++rr)
      if (e < s_ext[rr]) ws[s_wso[rr] + e] = dtile[rr * RP_LD + lane];
  }
  __threadfence_block();
  __syncthreads();                                     // the workspace rows were written by other lanes of this wave
  // backward: workspace, last sample first -> the row, padding dropped, rounded to f32 once
  double pre_d[RP_ROWS];
  const auto request_bwd = [&](int t0) {       // unconditional, as above: past the row's end its (or the workspace's) first double
    const int e = t0 + lane;
#pragma unroll
    for (int rr = 0; rr < RP_ROWS; ++rr) pre_d[rr] = ws[s_wso[rr] + (e < s_ext[rr] ? e : 0)];
  };
  f.start(k, ylast);
  const int t_top = ((Emax - 1) / RP_TT) * RP_TT;
  request_bwd(t_top);
  for (int t0 = t_top; t0 >= 0; t0 -= RP_TT) {
    const int e = t0 + lane;
#pragma unroll
    for (int rr = 0; rr < RP_ROWS; ++rr) dtile[rr * RP_LD + lane] = pre_d[rr];
    __syncthreads();
    if (t0 >= RP_TT) request_bwd(t0 - RP_TT);
    for (int t = RP_TT - 1; t >= 0; --t)
      if (t0 + t < E) ftile[lane * RP_LD + t] = (float)f.step(k, dtile[lane * RP_LD + t]);
    __syncthreads();
#pragma unroll 8
    for (int rr = 0; rr < RP_ROWS; ++rr) {
      const int Er = s_ext[rr];
      if (e >= pad && e < Er - pad) d.data[s_off[rr] + (e - pad)] = ftile[rr * RP_LD + lane];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// CAR + z-score (eg_window_normalize's mode 1 arithmetic, on rows longer than any LDS row): a sample-parallel pass, every
// thread reading its sample of the group's C rows in channel order and writing them back, then one block per row.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void recording_car_kernel(const eg_recording_rows_desc d) {
  const long long r0 = (long long)blockIdx.x * d.C;
  const int L = d.row_len[r0];
  for (long long t = (long long)blockIdx.y * 256 + threadIdx.x; t < L; t += (long long)gridDim.y * 256) {
    float s = 0.f;
    for (int c = 0; c < d.C; ++c) s += d.data[d.row_off[r0 + c] + t];
    const float car = s / (float)d.C;
    for (int c = 0; c < d.C; ++c) {
      float* p = d.data + d.row_off[r0 + c] + t;
      *p = *p - car;
    }
  }
}

__device__ __forceinline__ double block_sum_d(double v, double* red) {      // prep.hip's, so that the sums round alike
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

__global__ __launch_bounds__(256) void recording_zscore_kernel(const eg_recording_rows_desc d) {
  __shared__ double red[4];
  float* x = d.data + d.row_off[blockIdx.x];
  const int L = d.row_len[blockIdx.x];
  double s = 0.0;
  for (int t = threadIdx.x; t < L; t += 256) s += (double)x[t];
  const double mean = block_sum_d(s, red) / (double)L;
  const float meanf = (float)mean;
  double q = 0.0;
  for (int t = threadIdx.x; t < L; t += 256) {
    const double dv = (double)x[t] - mean;
    q += dv * dv;
  }
  const float den = (float)sqrt(block_sum_d(q, red) / (double)L) + 1e-8f;
  for (int t = threadIdx.x; t < L; t += 256) x[t] = (x[t] - meanf) / den;
}

int rows_desc_check(const char* who, const eg_recording_rows_desc* d) {
  EG_CHECK(d && d->data && d->row_off && d->row_len, "%s: null pointer", who);
  EG_CHECK(d->n_rows > 0, "%s: n_rows=%d must be > 0", who, d->n_rows);
  EG_CHECK(d->C > 0, "%s: C=%d must be > 0", who, d->C);
  return 0;
}

}  // namespace

namespace {

template <bool EXACT>
int launch_filtfilt(const char* who, const eg_recording_rows_desc* d, const double* b, const double* a, const double* zi, int ncoef,
                    double* workspace, int64_t workspace_need, int64_t workspace_capacity, void* stream) {
  if (rows_desc_check(who, d)) return 1;
  EG_CHECK(d->ws_off && b && a && zi && workspace, "%s: null pointer", who);
  EG_CHECK(ncoef >= 2 && ncoef <= RP_MAXC, "%s: ncoef=%d outside [2, %d]", who, ncoef, RP_MAXC);
  EG_CHECK(a[0] == 1.0, "%s: a[0]=%g must be 1 (normalise the coefficients)", who, a[0]);
  EG_CHECK(workspace_need > 0 && workspace_need <= workspace_capacity,
           "%s: the rows need %lld workspace doubles, the workspace's capacity is %lld", who, (long long)workspace_need,
           (long long)workspace_capacity);
  IirCoef k = {};
  for (int i = 0; i < ncoef; ++i) k.b[i] = b[i], k.a[i] = a[i];
  for (int i = 0; i + 1 < ncoef; ++i) k.zi[i] = zi[i];
  const dim3 grid((unsigned)((d->n_rows + RP_ROWS - 1) / RP_ROWS)), block(RP_ROWS);
  if (ncoef == 9)      // the reference's order-4 band-pass: its eight states and nothing else
    hipLaunchKernelGGL((recording_filtfilt_kernel<8, EXACT>), grid, block, 0, (hipStream_t)stream, *d, k, 3 * ncoef, workspace);
  else
    hipLaunchKernelGGL((recording_filtfilt_kernel<RP_MAXC - 1, EXACT>), grid, block, 0, (hipStream_t)stream, *d, k, 3 * ncoef, workspace);
  EG_LAUNCH_CHECK("recording_filtfilt");
  return 0;
}

}  // namespace

extern "C" int eg_recording_filtfilt(const eg_recording_rows_desc* d, const double* b, const double* a, const double* zi, int ncoef,
                                     double* workspace, int64_t workspace_need, int64_t workspace_capacity, void* stream) {
  return launch_filtfilt<false>("eg_recording_filtfilt", d, b, a, zi, ncoef, workspace, workspace_need, workspace_capacity, stream);
}

extern "C" int eg_recording_filtfilt_exact(const eg_recording_rows_desc* d, const double* b, const double* a, const double* zi, int ncoef,
                                           double* workspace, int64_t workspace_need, int64_t workspace_capacity, void* stream) {
  return launch_filtfilt<true>("eg_recording_filtfilt_exact", d, b, a, zi, ncoef, workspace, workspace_need, workspace_capacity, stream);
}

namespace {

// the CAR launch of both entry points
int launch_car(const char* who, const eg_recording_rows_desc* d, void* stream) {
  if (rows_desc_check(who, d)) return 1;
  EG_CHECK(d->n_rows % d->C == 0, "%s: n_rows=%d is no multiple of C=%d", who, d->n_rows, d->C);
  const int chunks = d->max_len > 0 ? (int)std::min<long long>(((long long)d->max_len + 255) / 256, 4096) : 1;
  hipLaunchKernelGGL(recording_car_kernel, dim3(d->n_rows / d->C, chunks), dim3(256), 0, (hipStream_t)stream, *d);
  EG_LAUNCH_CHECK("recording_car");
  return 0;
}

}  // namespace

extern "C" int eg_recording_car(const eg_recording_rows_desc* d, void* stream) { return launch_car("eg_recording_car", d, stream); }

extern "C" int eg_recording_car_zscore(const eg_recording_rows_desc* d, void* stream) {
  if (launch_car("eg_recording_car_zscore", d, stream)) return 1;
  hipLaunchKernelGGL(recording_zscore_kernel, dim3(d->n_rows), dim3(256), 0, (hipStream_t)stream, *d);
  EG_LAUNCH_CHECK("recording_zscore");
  return 0;
}
