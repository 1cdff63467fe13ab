// Trial features of the hyperscanning extractor (2_Preprocessing/scripts/extract_eeg_features.py): Welch PSD and band energies,
// the analytic signal of a band-filtered trial at any length, the pair sums of six connectivity metrics and the segment
// coherence; and the spectral entropy of the entropy analysis (5_Metrics/entropy_calculators.py), which shares the
// Welch loop.  include/eyegaze_hip.h states the contracts; DESIGN.md §8m the layout, the numerics and the measurements.
#include <algorithm>

#include "common.h"

namespace {

typedef double2 cplx;

__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cplx cmulc(cplx a, cplx b) { return {a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y}; }   // a conj(b)

__device__ __forceinline__ double block_sum256(double v, double* red) {      // recprep.hip's block_sum_d: 256 threads, fixed order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) red[w] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---------------------------------------------------------------------------------------------
// The 256-point transform of the Welch PSD and of the coherence: 256 threads, 256 complex doubles in LDS, decimation in
// frequency, so bin k ends at the bit-reversed index -- read there, never moved.  tw[k] = exp(-2 pi i k / 256), k < 128.
// ---------------------------------------------------------------------------------------------
constexpr int NFFT = EG_TRIAL_MIN_LEN, NBIN = EG_TRIAL_NBINS;

__device__ __forceinline__ void fft256_twiddles(cplx* tw) {
  if (threadIdx.x < NFFT / 2) {
    double s, c;
    sincospi(-2.0 * threadIdx.x / NFFT, &s, &c);
    tw[threadIdx.x] = {c, s};
  }
}
__device__ __forceinline__ void fft256(cplx* buf, const cplx* tw) {
  const int t = threadIdx.x;
  for (int half = NFFT / 2; half >= 1; half >>= 1) {
    __syncthreads();
    if (t < NFFT / 2) {
      const int j = t & (half - 1), i0 = ((t - j) << 1) + j, i1 = i0 + half;
      const cplx u = buf[i0], v = buf[i1];
      buf[i0] = {u.x + v.x, u.y + v.y};
      buf[i1] = cmul({u.x - v.x, u.y - v.y}, tw[j * (NFFT / 2 / half)]);
    }
  }
  __syncthreads();
}
__device__ __forceinline__ int bin_at(int k) { return (int)(__brev((unsigned)k) >> 24); }

struct BandBins {
  int k0[EG_TRIAL_MAX_BANDS], k1[EG_TRIAL_MAX_BANDS], n;
};

// scipy.signal.welch(x, fs, nperseg=256) of one row of L >= 256 samples by the whole block: thread t returns bin t's PSD in fp64,
// not yet rounded (0 for t >= 129).  eg_trial_welch and eg_trial_spectral_entropy both run this loop.
__device__ __forceinline__ double welch_row_bin(const float* __restrict__ x, const int L, const double fs, cplx* buf, cplx* tw, double* red) {
  const int t = threadIdx.x;
  fft256_twiddles(tw);
  const double w = 0.5 - 0.5 * cospi(2.0 * t / NFFT);                   // periodic Hann
  const double scale = 1.0 / (fs * block_sum256(w * w, red));
  const int nseg = (L - NFFT) / (NFFT / 2) + 1;
  double acc = 0.0;
  for (int s = 0; s < nseg; ++s) {
    const double v = (double)x[s * (NFFT / 2) + t];
    const double mean = block_sum256(v, red) * (1.0 / NFFT);           // (its barriers also end the last segment's reads of buf)
    buf[t] = {(v - mean) * w, 0.0};
    fft256(buf, tw);
    if (t < NBIN) {
      const cplx X = buf[bin_at(t)];
      acc += X.x * X.x + X.y * X.y;
    }
  }
  double p = acc / nseg * scale;
  if (t > 0 && t < NBIN - 1) p *= 2.0;
  return p;
}

__global__ __launch_bounds__(256) void trial_welch_kernel(const eg_recording_rows_desc d, const double fs, const BandBins bb,
                                                          float* __restrict__ psd, float* __restrict__ energy, int32_t* nonfinite) {
  __shared__ cplx buf[NFFT], tw[NFFT / 2];
  __shared__ double red[4];
  __shared__ float ps[NBIN];
  const int row = blockIdx.x, t = threadIdx.x, L = d.row_len[row];
  if (L < NFFT || L > d.max_len) return;
  const double p = welch_row_bin(d.data + d.row_off[row], L, fs, buf, tw, red);
  if (t < NBIN) {
    const float pf = (float)p;
    psd[(long long)row * NBIN + t] = pf;
    ps[t] = pf;
    if (nonfinite && !isfinite(pf)) *nonfinite = 1;
  }
  __syncthreads();
  if (t < bb.n) {
    double s = 0.0;
    for (int k = bb.k0[t]; k <= bb.k1[t]; ++k) s += (double)ps[k];
    energy[(long long)row * bb.n + t] = bb.k1[t] >= bb.k0[t] ? (float)(s / (bb.k1[t] - bb.k0[t] + 1)) : 0.f;
  }
}

// Spectral entropy (5_Metrics/entropy_calculators.py:323-344): the Shannon entropy in bits of the row's Welch PSD, from the fp64
// bins BEFORE they are rounded.  q = |p| + eps, S = sum q, T = sum q ln q, H = (ln S - T / S) / ln 2; a bin with q == 0 (eps == 0)
// adds nothing, as scipy's entr.  A NaN or Inf of the row reaches S and makes H NaN.
__global__ __launch_bounds__(256) void trial_spectral_entropy_kernel(const eg_recording_rows_desc d, const double fs, const double eps,
                                                                     float* __restrict__ psd, double* __restrict__ entropy) {
  __shared__ cplx buf[NFFT], tw[NFFT / 2];
  __shared__ double red[4];
  const int row = blockIdx.x, t = threadIdx.x, L = d.row_len[row];
  if (L < NFFT || L > d.max_len) return;
  const double p = welch_row_bin(d.data + d.row_off[row], L, fs, buf, tw, red);
  if (psd && t < NBIN) psd[(long long)row * NBIN + t] = (float)p;
  const double q = t < NBIN ? fabs(p) + eps : 0.0;
  const double S = block_sum256(q, red);
  const double T = block_sum256(q > 0.0 || q != q ? q * log(q) : 0.0, red);
  if (t == 0) entropy[row] = (log(S) - T / S) / 0.693147180559945309417232121458;
}

// ---------------------------------------------------------------------------------------------
// Coherence.  Spectra: one block per row, X [row][max_seg][129] as float2 and Pxx [row][129] into the workspace.  Pairs: one block
// per (trial, matrix, i), thread f sums X_i conj X_j over the segments in fp64 for one j after the other; the bins are added by
// the block in a fixed order.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void trial_coh_spectra_kernel(const eg_recording_rows_desc d, const int max_seg, float* __restrict__ pxx,
                                                                float2* __restrict__ spec) {
  __shared__ cplx buf[NFFT], tw[NFFT / 2];
  const int row = blockIdx.x, t = threadIdx.x, L = d.row_len[row];
  const int nseg = L / NFFT;
  if (nseg < 1 || nseg > max_seg) return;
  const float* x = d.data + d.row_off[row];
  fft256_twiddles(tw);
  const double w = (double)(float)(0.5 - 0.5 * cospi(2.0 * t / (NFFT - 1)));       // np.hanning(256).astype(float32)
  double acc = 0.0;
  for (int s = 0; s < nseg; ++s) {
    buf[t] = {(double)x[s * NFFT + t] * w, 0.0};
    fft256(buf, tw);
    if (t < NBIN) {
      const cplx X = buf[bin_at(t)];
      acc += X.x * X.x + X.y * X.y;
      spec[((long long)row * max_seg + s) * NBIN + t] = {(float)X.x, (float)X.y};
    }
    __syncthreads();
  }
  if (t < NBIN) pxx[(long long)row * NBIN + t] = (float)(acc / nseg);
}

__device__ __forceinline__ long long con_index(int g, int m, int metric, int band, int nbands, int C) {
  return ((((long long)g * 3 + m) * 7 + metric) * nbands + band) * C * C;
}

__global__ __launch_bounds__(256) void trial_coh_pairs_kernel(const eg_recording_rows_desc d, const int max_seg, const float* __restrict__ pxx,
                                                              const float2* __restrict__ spec, float* __restrict__ con, const int band,
                                                              const int nbands) {
  __shared__ double red[4];
  const int C = d.C, i = blockIdx.x, m = blockIdx.y, g = blockIdx.z, f = threadIdx.x;
  const long long r0 = (long long)g * 2 * C;
  const long long ri = r0 + (m == 1 ? C : 0) + i, rj0 = r0 + (m == 0 ? 0 : C);
  const int nseg = d.row_len[ri] / NFFT;
  if (nseg < 1 || nseg > max_seg) return;
  float* out = con + con_index(g, m, 5, band, nbands, C) + (long long)i * C;
  const float2* xi = spec + ri * max_seg * NBIN + f;
  const double pi_ = f < NBIN ? (double)pxx[ri * NBIN + f] : 0.0;
  for (int j = 0; j < C; ++j) {
    double coh = 0.0;
    if (f < NBIN) {
      const float2* xj = spec + (rj0 + j) * max_seg * NBIN + f;
      double re = 0.0, im = 0.0;
      for (int s = 0; s < nseg; ++s) {
        const float2 a = xi[(long long)s * NBIN], b = xj[(long long)s * NBIN];
        re += (double)a.x * b.x + (double)a.y * b.y;
        im += (double)a.y * b.x - (double)a.x * b.y;
      }
      re /= nseg, im /= nseg;
      coh = (re * re + im * im) / (pi_ * (double)pxx[(rj0 + j) * NBIN + f] + 1e-8);
    }
    const double total = block_sum256(coh, red);
    if (f == 0) out[j] = (float)(total / NBIN);
  }
}

// ---------------------------------------------------------------------------------------------
// Analytic signal.  Both DFTs of length L are chirp-z transforms: X[k] = w[k] sum_n (x[n] w[n]) conj(w)[k - n], w[n] =
// exp(-i pi n^2 / L), the sum a circular convolution of length M = 2^p >= 2 L - 1 through two FFTs and the stored spectrum of
// the chirp.  The FFTs run in place without a reordering pass: decimation in frequency forward (natural order in, bit-reversed
// out), the pointwise product in bit-reversed order, decimation in time backward (bit-reversed in, natural out).  A row whose M
// fits AN_LDS_M transforms in LDS, a longer one in its own workspace doubles; the code is the same.
// ---------------------------------------------------------------------------------------------
constexpr int AN_THREADS = 1024;
constexpr int AN_LDS_M = 8192;                                  // 8192 complex doubles = 128 KiB of the CU's 160
constexpr int AN_MAX_M = 2 * EG_TRIAL_MAX_LEN;

static inline int pow2_at_least(int n) {
  int m = 1;
  while (m < n) m <<= 1;
  return m;
}
__device__ __forceinline__ int dev_pow2_at_least(int n) { return n <= 1 ? 1 : 1 << (32 - __clz(n - 1)); }

template <bool GLOBAL>
__device__ __forceinline__ void an_sync() {
  if (GLOBAL) __threadfence_block();
  __syncthreads();
}

// tw[k] = exp(-2 pi i k / Mmax), k < Mmax / 2; tws = Mmax / M
template <bool GLOBAL>
__device__ __forceinline__ void fft_dif(cplx* buf, int M, const cplx* __restrict__ tw, int tws) {
  for (int half = M >> 1; half >= 1; half >>= 1) {
    an_sync<GLOBAL>();
    const int ts = tws * ((M >> 1) / half);
    for (int t = threadIdx.x; t < (M >> 1); t += AN_THREADS) {
      const int j = t & (half - 1), i0 = ((t - j) << 1) + j, i1 = i0 + half;
      const cplx u = buf[i0], v = buf[i1];
      buf[i0] = {u.x + v.x, u.y + v.y};
      buf[i1] = cmul({u.x - v.x, u.y - v.y}, tw[j * ts]);
    }
  }
  an_sync<GLOBAL>();
}
// the inverse of fft_dif up to the factor M
template <bool GLOBAL>
__device__ __forceinline__ void fft_dit_inverse(cplx* buf, int M, const cplx* __restrict__ tw, int tws) {
  for (int half = 1; half <= (M >> 1); half <<= 1) {
    an_sync<GLOBAL>();
    const int ts = tws * ((M >> 1) / half);
    for (int t = threadIdx.x; t < (M >> 1); t += AN_THREADS) {
      const int j = t & (half - 1), i0 = ((t - j) << 1) + j, i1 = i0 + half;
      const cplx u = buf[i0], v = cmulc(buf[i1], tw[j * ts]);
      buf[i0] = {u.x + v.x, u.y + v.y};
      buf[i1] = {u.x - v.x, u.y - v.y};
    }
  }
  an_sync<GLOBAL>();
}

__global__ __launch_bounds__(256) void trial_twiddle_kernel(cplx* __restrict__ tw, const int Mmax) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < Mmax / 2) {
    double s, c;
    sincospi(-2.0 * k / Mmax, &s, &c);
    tw[k] = {c, s};
  }
}

// per trial: W[n] = exp(-i pi (n^2 mod 2 L) / L), n < L, behind B = FFT of the chirp conj(W) laid out circularly over M
__global__ __launch_bounds__(AN_THREADS) void trial_chirp_kernel(const eg_recording_rows_desc d, const int64_t* __restrict__ chirp_off,
                                                                 double* __restrict__ ws, const int Mmax) {
  const int g = blockIdx.x, L = d.row_len[(long long)g * 2 * d.C];
  const int M = dev_pow2_at_least(2 * L - 1);
  if (L < 1 || L > d.max_len || M > Mmax) return;
  cplx* B = (cplx*)(ws + chirp_off[g]);
  cplx* W = B + M;
  for (int n = threadIdx.x; n < M; n += AN_THREADS) B[n] = {0.0, 0.0};
  an_sync<true>();
  for (int n = threadIdx.x; n < L; n += AN_THREADS) {
    const unsigned long long q = ((unsigned long long)n * n) % (unsigned long long)(2 * L);
    double s, c;
    sincospi((double)q / (double)L, &s, &c);
    W[n] = {c, -s};
    B[n] = {c, s};
    if (n) B[M - n] = {c, s};
  }
  fft_dif<true>(B, M, (const cplx*)ws, Mmax / M);
}

template <bool GLOBAL>
__device__ __forceinline__ void chirp_dft(cplx* buf, int M, const cplx* __restrict__ B, const cplx* __restrict__ tw, int tws) {
  fft_dif<GLOBAL>(buf, M, tw, tws);
  for (int n = threadIdx.x; n < M; n += AN_THREADS) buf[n] = cmul(buf[n], B[n]);
  fft_dit_inverse<GLOBAL>(buf, M, tw, tws);
}

template <bool GLOBAL>
__device__ __forceinline__ void analytic_row(cplx* buf, const float* __restrict__ x, int L, int M, const cplx* __restrict__ B,
                                             const cplx* __restrict__ W, const cplx* __restrict__ tw, int tws, float* __restrict__ amp,
                                             float* __restrict__ cs, float* __restrict__ sn) {
  const double inv_m = 1.0 / M;
  for (int n = threadIdx.x; n < M; n += AN_THREADS) {
    cplx v = {0.0, 0.0};
    if (n < L) {
      const double xv = (double)x[n];
      v = {xv * W[n].x, xv * W[n].y};
    }
    buf[n] = v;
  }
  chirp_dft<GLOBAL>(buf, M, B, tw, tws);
  // X[k] = W[k] buf[k] / M; the inverse DFT of h X is conj(DFT(conj(h X))) / L, so the second transform's input is conj(h X) W
  for (int n = threadIdx.x; n < M; n += AN_THREADS) {
    cplx v = {0.0, 0.0};
    if (n < L) {
      const double h = n == 0 || 2 * n == L ? 1.0 : 2 * n < L ? 2.0 : 0.0;
      const cplx X = cmul(W[n], buf[n]);
      v = cmul({X.x * inv_m * h, -X.y * inv_m * h}, W[n]);
    }
    buf[n] = v;
  }
  chirp_dft<GLOBAL>(buf, M, B, tw, tws);
  const double inv = inv_m / L;
  for (int n = threadIdx.x; n < L; n += AN_THREADS) {
    const cplx y = cmul(W[n], buf[n]);
    const double zr = y.x * inv, zi = -y.y * inv;
    const double a = sqrt(zr * zr + zi * zi);
    amp[n] = (float)a;
    cs[n] = a > 0.0 ? (float)(zr / a) : 1.f;
    sn[n] = a > 0.0 ? (float)(zi / a) : 0.f;
  }
}

__global__ __launch_bounds__(AN_THREADS) void trial_analytic_kernel(const eg_recording_rows_desc d, const int64_t* __restrict__ chirp_off,
                                                                    float* __restrict__ amp, float* __restrict__ cs, float* __restrict__ sn,
                                                                    double* __restrict__ ws, const int Mmax, const int lds_m) {
  extern __shared__ __align__(16) unsigned char an_lds[];
  const long long row = blockIdx.x;
  const int L = d.row_len[row];
  const int M = dev_pow2_at_least(2 * L - 1);
  if (L < 1 || L > d.max_len || M > Mmax) return;
  const cplx* B = (const cplx*)(ws + chirp_off[row / (2 * d.C)]);
  const cplx* W = B + M;
  const long long off = d.row_off[row];
  if (M <= lds_m)
    analytic_row<false>((cplx*)an_lds, d.data + off, L, M, B, W, (const cplx*)ws, Mmax / M, amp + off, cs + off, sn + off);
  else
    analytic_row<true>((cplx*)(ws + d.ws_off[row]), d.data + off, L, M, B, W, (const cplx*)ws, Mmax / M, amp + off, cs + off, sn + off);
}

// ---------------------------------------------------------------------------------------------
// Pair sums.  Row statistics first (one block per row, fp64 sums as the z-score's).  Then one block per (trial, matrix, 32 x 32
// tile of pairs, chunk of PK_TS samples): four waves, each a 16 x 16 tile; the chunk passes through LDS PK_KT samples at a time
// as four planes per side -- zs(x), zs(a), cos, sin -- rows past C and samples past the chunk as zeros, which add nothing to any
// of the six sums.  Per four samples six v_mfma_f32_16x16x4_f32 (x x, a a, c c + s s, s c - c s); sign and |.| of Im P on the
// vector unit in the MFMA's own result layout (lane: column lane % 16, rows 4 (lane / 16) + r), Im P from two rounded
// products.  Stages are added in fp64 in registers; partials [trial][matrix][chunk][6][C][C] f32; trial_pair_finish_kernel adds
// the chunks in ascending order in fp64.
// ---------------------------------------------------------------------------------------------
constexpr int PK_TS = 256, PK_KT = 32, PK_LD = PK_KT + 4, PK_TILE = 32;

__global__ __launch_bounds__(256) void trial_rowstats_kernel(const eg_recording_rows_desc d, const float* __restrict__ amp,
                                                             float* __restrict__ stats) {
  __shared__ double red[4];
  const int row = blockIdx.x, L = d.row_len[row];
  if (L < 1 || L > d.max_len) return;
  const long long off = d.row_off[row];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float* v = (p ? amp : d.data) + off;
    double s = 0.0;
    for (int t = threadIdx.x; t < L; t += 256) s += (double)v[t];
    const double mean = block_sum256(s, red) / L;
    double q = 0.0;
    for (int t = threadIdx.x; t < L; t += 256) {
      const double dv = (double)v[t] - mean;
      q += dv * dv;
    }
    const double var = block_sum256(q, red) / L;
    if (threadIdx.x == 0) {
      stats[4 * row + 2 * p] = (float)mean;
      stats[4 * row + 2 * p + 1] = (float)sqrt(var) + 1e-8f;
    }
  }
}

// s_i c_j - c_i s_j from two ROUNDED products: contracted into a multiply-add it leaves, for a channel with itself, the first
// product's rounding residue, whose sign would count in the PLI
__device__ __forceinline__ float im_two_products(float si, float cj, float ci, float sj) {
#pragma clang fp contract(off)
  const float a = si * cj, b = ci * sj;
  return a - b;
}

__global__ __launch_bounds__(256) void trial_pairs_kernel(const eg_recording_rows_desc d, const float* __restrict__ amp,
                                                          const float* __restrict__ cs, const float* __restrict__ sn,
                                                          const float* __restrict__ stats, float* __restrict__ part, const int max_split) {
  __shared__ __align__(16) float sm[2][4][PK_TILE][PK_LD];
  __shared__ long long s_off[2][PK_TILE];
  __shared__ float s_stat[2][PK_TILE][4];
  const int C = d.C, tiles = (C + PK_TILE - 1) / PK_TILE;
  const int split = blockIdx.x / (tiles * tiles), tile = blockIdx.x % (tiles * tiles);
  const int m = blockIdx.y, g = blockIdx.z;
  const long long r0 = (long long)g * 2 * C;
  const int L = d.row_len[r0];
  const int t_begin = split * PK_TS, t_end = min(L, t_begin + PK_TS);
  if (t_begin >= L || L > d.max_len) return;
  const int i0 = (tile / tiles) * PK_TILE, j0 = (tile % tiles) * PK_TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < 2 * PK_TILE) {
    const int side = tid / PK_TILE, r = tid % PK_TILE;
    const int ch = (side ? j0 : i0) + r;
    const bool second = side ? m != 0 : m == 1;           // which player the side's rows belong to
    const long long row = r0 + (second ? C : 0) + ch;
    s_off[side][r] = ch < C ? d.row_off[row] : -1;
#pragma unroll
    for (int q = 0; q < 4; ++q) s_stat[side][r][q] = ch < C ? stats[4 * row + q] : 1.f;
  }
  __syncthreads();
  const int wi = (wave >> 1) * 16, wj = (wave & 1) * 16;
  // a stage's 32 samples are summed in f32 (the MFMA's fma chain, the vector adds), the stages in fp64: a chain of 256 f32 adds of
  // values near 1 would alone cost 5e-7 of a mean
  double sum[6][4] = {};
  for (int t0 = t_begin; t0 < t_end; t0 += PK_KT) {
    // stage: element e = ((side * 4 + plane) * 32 + row) * 32 + t; a wave reads 32 consecutive samples of two rows at a time
#pragma unroll 4
    for (int e = tid; e < 2 * 4 * PK_TILE * PK_KT; e += 256) {
      const int t = e % PK_KT, r = (e / PK_KT) % PK_TILE, plane = (e / (PK_KT * PK_TILE)) % 4, side = e / (PK_KT * PK_TILE * 4);
      const long long off = s_off[side][r];
      float v = 0.f;
      if (off >= 0 && t0 + t < t_end) {
        const float* src = plane == 0 ? d.data : plane == 1 ? amp : plane == 2 ? cs : sn;
        v = src[off + t0 + t];
        if (plane < 2) v = (v - s_stat[side][r][2 * plane]) / s_stat[side][r][2 * plane + 1];
      }
      sm[side][plane][r][t] = v;
    }
    __syncthreads();
    const int ar = wi + (lane & 15), br = wj + (lane & 15), kk = lane >> 4;
    f32x4 acc_xx = {0.f, 0.f, 0.f, 0.f}, acc_aa = acc_xx, acc_re = acc_xx, acc_im = acc_xx;
    float sgn[4] = {0.f, 0.f, 0.f, 0.f}, mag[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k0 = 0; k0 < PK_KT; k0 += 4) {
      const float xi = sm[0][0][ar][k0 + kk], xj = sm[1][0][br][k0 + kk];
      const float ai = sm[0][1][ar][k0 + kk], aj = sm[1][1][br][k0 + kk];
      const float ci = sm[0][2][ar][k0 + kk], cj = sm[1][2][br][k0 + kk];
      const float si = sm[0][3][ar][k0 + kk], sj = sm[1][3][br][k0 + kk];
      acc_xx = __builtin_amdgcn_mfma_f32_16x16x4f32(xi, xj, acc_xx, 0, 0, 0);
      acc_aa = __builtin_amdgcn_mfma_f32_16x16x4f32(ai, aj, acc_aa, 0, 0, 0);
      acc_re = __builtin_amdgcn_mfma_f32_16x16x4f32(ci, cj, acc_re, 0, 0, 0);
      acc_im = __builtin_amdgcn_mfma_f32_16x16x4f32(si, cj, acc_im, 0, 0, 0);
      acc_re = __builtin_amdgcn_mfma_f32_16x16x4f32(si, sj, acc_re, 0, 0, 0);
      acc_im = __builtin_amdgcn_mfma_f32_16x16x4f32(-ci, sj, acc_im, 0, 0, 0);
    }
    const int jr = wj + (lane & 15), ir = wi + 4 * (lane >> 4);
#pragma unroll
    for (int t4 = 0; t4 < PK_KT; t4 += 4) {
      const f32x4 cj = *(const f32x4*)&sm[1][2][jr][t4], sj = *(const f32x4*)&sm[1][3][jr][t4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const f32x4 ci = *(const f32x4*)&sm[0][2][ir + r][t4], si = *(const f32x4*)&sm[0][3][ir + r][t4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float im = im_two_products(si[q], cj[q], ci[q], sj[q]);
          sgn[r] += im > 0.f ? 1.f : im < 0.f ? -1.f : 0.f;
          mag[r] += fabsf(im);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sum[0][r] += (double)acc_xx[r], sum[1][r] += (double)acc_aa[r], sum[2][r] += (double)acc_re[r], sum[3][r] += (double)acc_im[r];
      sum[4][r] += (double)sgn[r], sum[5][r] += (double)mag[r];
    }
    __syncthreads();
  }
  const int j = j0 + wj + (lane & 15);
  float* base = part + ((((long long)g * 3 + m) * max_split + split) * 6) * C * C;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + wi + 4 * (lane >> 4) + r;
    if (i < C && j < C) {
      const long long o = (long long)i * C + j, cc = (long long)C * C;
#pragma unroll
      for (int q = 0; q < 6; ++q) base[q * cc + o] = (float)sum[q][r];
    }
  }
}

__global__ __launch_bounds__(256) void trial_pair_finish_kernel(const eg_recording_rows_desc d, const float* __restrict__ part,
                                                                const int max_split, float* __restrict__ con, const int band,
                                                                const int nbands) {
  const int C = d.C, m = blockIdx.y, g = blockIdx.z;
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int L = d.row_len[(long long)g * 2 * C];
  if (e >= C * C || L < 1 || L > d.max_len) return;
  const int nsplit = (L + PK_TS - 1) / PK_TS;
  const long long cc = (long long)C * C;
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < nsplit; ++k) {
    const float* p = part + ((((long long)g * 3 + m) * max_split + k) * 6) * cc + e;
#pragma unroll
    for (int q = 0; q < 6; ++q) s[q] += (double)p[q * cc];
  }
  if (m < 2 && e / C == e % C) s[3] = 0.0;               // Im P of a channel with itself: the MFMA's fma chain leaves a residue
  const double n = (double)L;
  const auto out = [&](int metric, double v) { con[con_index(g, m, metric, band, nbands, C) + e] = (float)v; };
  out(0, s[0] / n);
  out(1, s[1] / n);
  out(2, sqrt(s[2] * s[2] + s[3] * s[3]) / n);
  out(3, fabs(s[4]) / n);
  out(4, fabs(s[3] / n) / (s[5] / n + 1e-8));
  out(6, s[3] == 0.0 && s[2] >= 0.0 ? 0.0 : atan2(s[3], s[2]));
}

// pairs: the rows are trials of two players (every entry point but the spectral entropy, whose rows are single recordings)
int trial_desc_check(const char* who, const eg_recording_rows_desc* d, bool pairs = true) {
  EG_CHECK(d && d->data && d->row_off && d->row_len, "%s: null pointer", who);
  EG_CHECK(d->n_rows > 0, "%s: n_rows=%d must be > 0", who, d->n_rows);
  EG_CHECK(d->C > 0, "%s: C=%d must be > 0", who, d->C);
  if (pairs)
    EG_CHECK(d->n_rows % (2 * (long long)d->C) == 0, "%s: n_rows=%d is no multiple of 2 C=%lld (two players per trial)", who, d->n_rows,
             2 * (long long)d->C);
  else
    EG_CHECK(d->n_rows % d->C == 0, "%s: n_rows=%d is no multiple of C=%d", who, d->n_rows, d->C);
  EG_CHECK(d->max_len >= EG_TRIAL_MIN_LEN && d->max_len <= EG_TRIAL_MAX_LEN, "%s: max_len=%d outside [%d, %d]", who, d->max_len,
           EG_TRIAL_MIN_LEN, EG_TRIAL_MAX_LEN);
  return 0;
}

int band_check(const char* who, int band, int nbands) {
  EG_CHECK(nbands >= 1 && nbands <= EG_TRIAL_MAX_BANDS, "%s: nbands=%d outside [1, %d]", who, nbands, EG_TRIAL_MAX_BANDS);
  EG_CHECK(band >= 0 && band < nbands, "%s: band=%d outside [0, %d)", who, band, nbands);
  return 0;
}

}  // namespace

extern "C" int eg_trial_welch(const eg_recording_rows_desc* d, double fs, const int32_t* band_k0, const int32_t* band_k1, int nbands,
                              float* psd, float* energy, int32_t* nonfinite, void* stream) {
  if (trial_desc_check("eg_trial_welch", d)) return 1;
  EG_CHECK(psd && energy && (nbands == 0 || (band_k0 && band_k1)), "eg_trial_welch: null pointer");
  EG_CHECK(fs > 0.0, "eg_trial_welch: fs=%g must be > 0", fs);
  EG_CHECK(nbands >= 0 && nbands <= EG_TRIAL_MAX_BANDS, "eg_trial_welch: nbands=%d outside [0, %d]", nbands, EG_TRIAL_MAX_BANDS);
  BandBins bb = {};
  bb.n = nbands;
  for (int i = 0; i < nbands; ++i) {
    EG_CHECK(band_k0[i] >= 0 && band_k0[i] < NBIN && band_k1[i] >= -1 && band_k1[i] < NBIN,
             "eg_trial_welch: band %d covers bins [%d, %d], outside [0, %d]", i, band_k0[i], band_k1[i], NBIN - 1);
    bb.k0[i] = band_k0[i], bb.k1[i] = band_k1[i];
  }
  hipLaunchKernelGGL(trial_welch_kernel, dim3(d->n_rows), dim3(256), 0, (hipStream_t)stream, *d, fs, bb, psd, energy, nonfinite);
  EG_LAUNCH_CHECK("trial_welch");
  return 0;
}

extern "C" int eg_trial_spectral_entropy(const eg_recording_rows_desc* d, double fs, double eps, float* psd, double* entropy, void* stream) {
  if (trial_desc_check("eg_trial_spectral_entropy", d, false)) return 1;
  EG_CHECK(entropy, "eg_trial_spectral_entropy: null pointer");
  EG_CHECK(fs > 0.0, "eg_trial_spectral_entropy: fs=%g must be > 0", fs);
  EG_CHECK(eps >= 0.0, "eg_trial_spectral_entropy: eps=%g must be >= 0", eps);
  hipLaunchKernelGGL(trial_spectral_entropy_kernel, dim3(d->n_rows), dim3(256), 0, (hipStream_t)stream, *d, fs, eps, psd, entropy);
  EG_LAUNCH_CHECK("trial_spectral_entropy");
  return 0;
}

extern "C" int64_t eg_trial_analytic_twiddle_doubles(int max_len) {
  if (max_len < EG_TRIAL_MIN_LEN || max_len > EG_TRIAL_MAX_LEN) return -1;
  return pow2_at_least(2 * max_len - 1);                // Mmax / 2 complex
}

namespace {

// the checks both analytic entry points share; *Mmax = the largest transform
int analytic_check(const char* who, const eg_recording_rows_desc* d, const int64_t* chirp_off, const double* workspace,
                   int64_t workspace_need, int64_t workspace_capacity, int* Mmax) {
  if (trial_desc_check(who, d)) return 1;
  EG_CHECK(d->ws_off && chirp_off && workspace, "%s: null pointer", who);
  *Mmax = pow2_at_least(2 * d->max_len - 1);
  // the least any table can need: the twiddles, one trial's chirp tables at the smallest length
  const int64_t least = (int64_t)*Mmax + 2 * (2 * EG_TRIAL_MIN_LEN) + 2 * EG_TRIAL_MIN_LEN;
  EG_CHECK(workspace_need >= least && workspace_need <= workspace_capacity,
           "%s: the rows need %lld workspace doubles (at least %lld), the workspace's capacity is %lld", who,
           (long long)workspace_need, (long long)least, (long long)workspace_capacity);
  static_assert(AN_MAX_M == 131072, "Mmax is bounded by max_len's check");
  return 0;
}

}  // namespace

extern "C" int eg_trial_analytic_tables(const eg_recording_rows_desc* d, const int64_t* chirp_off, double* workspace,
                                        int64_t workspace_need, int64_t workspace_capacity, void* stream) {
  int Mmax;
  if (analytic_check("eg_trial_analytic_tables", d, chirp_off, workspace, workspace_need, workspace_capacity, &Mmax)) return 1;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(trial_twiddle_kernel, dim3((Mmax / 2 + 255) / 256), dim3(256), 0, s, (cplx*)workspace, Mmax);
  EG_LAUNCH_CHECK("trial_twiddle");
  hipLaunchKernelGGL(trial_chirp_kernel, dim3(d->n_rows / (2 * d->C)), dim3(AN_THREADS), 0, s, *d, chirp_off, workspace, Mmax);
  EG_LAUNCH_CHECK("trial_chirp");
  return 0;
}

extern "C" int eg_trial_analytic(const eg_recording_rows_desc* d, const int64_t* chirp_off, float* amp, float* cs, float* sn,
                                 double* workspace, int64_t workspace_need, int64_t workspace_capacity, void* stream) {
  int Mmax;
  if (analytic_check("eg_trial_analytic", d, chirp_off, workspace, workspace_need, workspace_capacity, &Mmax)) return 1;
  EG_CHECK(amp && cs && sn, "eg_trial_analytic: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int lds_m = std::min(Mmax, AN_LDS_M);
  // per call, so on whichever device is current: the attribute belongs to the device's copy of the kernel
  const hipError_t attr = hipFuncSetAttribute((const void*)trial_analytic_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                              AN_LDS_M * (int)sizeof(cplx));
  EG_CHECK(attr == hipSuccess, "eg_trial_analytic: raising the dynamic LDS limit to %d bytes: %s", AN_LDS_M * (int)sizeof(cplx),
           hipGetErrorString(attr));
  hipLaunchKernelGGL(trial_analytic_kernel, dim3(d->n_rows), dim3(AN_THREADS), lds_m * sizeof(cplx), s, *d, chirp_off, amp, cs, sn,
                     workspace, Mmax, lds_m);
  EG_LAUNCH_CHECK("trial_analytic");
  return 0;
}

extern "C" int64_t eg_trial_pairs_workspace_floats(int n_rows, int C, int max_len) {
  if (n_rows <= 0 || C <= 0 || n_rows % (2 * (long long)C) || max_len < EG_TRIAL_MIN_LEN || max_len > EG_TRIAL_MAX_LEN) return -1;
  const int64_t splits = (max_len + PK_TS - 1) / PK_TS;
  return 4 * (int64_t)n_rows + (int64_t)(n_rows / (2 * C)) * 3 * splits * 6 * C * C;
}

extern "C" int eg_trial_pairs(const eg_recording_rows_desc* d, const float* amp, const float* cs, const float* sn, float* workspace,
                              int64_t workspace_capacity, float* con, int band, int nbands, void* stream) {
  if (trial_desc_check("eg_trial_pairs", d)) return 1;
  EG_CHECK(amp && cs && sn && workspace && con, "eg_trial_pairs: null pointer");
  if (band_check("eg_trial_pairs", band, nbands)) return 1;
  const int64_t need = eg_trial_pairs_workspace_floats(d->n_rows, d->C, d->max_len);
  EG_CHECK(need <= workspace_capacity, "eg_trial_pairs: the rows need %lld workspace floats, the workspace's capacity is %lld",
           (long long)need, (long long)workspace_capacity);
  const int trials = d->n_rows / (2 * d->C), splits = (d->max_len + PK_TS - 1) / PK_TS, tiles = (d->C + PK_TILE - 1) / PK_TILE;
  EG_CHECK((long long)splits * tiles * tiles < (1ll << 31) && trials <= 65535, "eg_trial_pairs: %d trials of C=%d exceed the grid", trials,
           d->C);
  hipStream_t s = (hipStream_t)stream;
  float* stats = workspace;
  float* part = workspace + 4 * (int64_t)d->n_rows;
  hipLaunchKernelGGL(trial_rowstats_kernel, dim3(d->n_rows), dim3(256), 0, s, *d, amp, stats);
  EG_LAUNCH_CHECK("trial_rowstats");
  hipLaunchKernelGGL(trial_pairs_kernel, dim3(splits * tiles * tiles, 3, trials), dim3(256), 0, s, *d, amp, cs, sn, stats, part, splits);
  EG_LAUNCH_CHECK("trial_pairs");
  hipLaunchKernelGGL(trial_pair_finish_kernel, dim3((d->C * d->C + 255) / 256, 3, trials), dim3(256), 0, s, *d, part, splits, con, band,
                     nbands);
  EG_LAUNCH_CHECK("trial_pair_finish");
  return 0;
}

extern "C" int64_t eg_trial_coherence_workspace_floats(int n_rows, int max_len) {
  if (n_rows <= 0 || max_len < EG_TRIAL_MIN_LEN || max_len > EG_TRIAL_MAX_LEN) return -1;
  return (int64_t)n_rows * NBIN * (1 + 2 * (int64_t)(max_len / NFFT));
}

extern "C" int eg_trial_coherence(const eg_recording_rows_desc* d, float* workspace, int64_t workspace_capacity, float* con, int band,
                                  int nbands, void* stream) {
  if (trial_desc_check("eg_trial_coherence", d)) return 1;
  EG_CHECK(workspace && con, "eg_trial_coherence: null pointer");
  if (band_check("eg_trial_coherence", band, nbands)) return 1;
  const int64_t need = eg_trial_coherence_workspace_floats(d->n_rows, d->max_len);
  EG_CHECK(need <= workspace_capacity, "eg_trial_coherence: the rows need %lld workspace floats, the workspace's capacity is %lld",
           (long long)need, (long long)workspace_capacity);
  const int trials = d->n_rows / (2 * d->C), max_seg = d->max_len / NFFT;
  EG_CHECK(trials <= 65535, "eg_trial_coherence: %d trials exceed the grid", trials);
  hipStream_t s = (hipStream_t)stream;
  float* pxx = workspace;
  float2* spec = (float2*)(workspace + (int64_t)d->n_rows * NBIN);
  hipLaunchKernelGGL(trial_coh_spectra_kernel, dim3(d->n_rows), dim3(256), 0, s, *d, max_seg, pxx, spec);
  EG_LAUNCH_CHECK("trial_coh_spectra");
  hipLaunchKernelGGL(trial_coh_pairs_kernel, dim3(d->C, 3, trials), dim3(256), 0, s, *d, max_seg, pxx, spec, con, band, nbands);
  EG_LAUNCH_CHECK("trial_coh_pairs");
  return 0;
}
