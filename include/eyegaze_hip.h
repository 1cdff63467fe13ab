/*
 * eyegaze_hip.h — C ABI of libeyegaze_hip.so: the MI355X (gfx950) kernels behind the reference's
 * dual-stream window classifier hot path
 *     run_experiments.py -> 4_Experiments/scripts/train_art.py::train_epoch/evaluate
 *       -> 3_Models/backbones/dual_eeg_transformer.py::DualEEGTransformer.forward (+ art.py encoder)
 *       -> loss -> backward -> clip -> AdamW.
 *
 * The reference has no FFI of its own (it is pure PyTorch); its seam is the nn.Module interface
 * (dual_eeg_transformer.py:995-1021 ctor, :1110-1253 forward).  A maintainer binds this library with
 * ctypes from a drop-in `DualEEGTransformer` (see INTEGRATION.md and
 * eyegaze_multimodal_amd/dual_eeg_transformer.py).  Each entry point below names the reference lines
 * whose arithmetic it replaces ("D:" = dual_eeg_transformer.py, "A:" = art.py, "T:" = train_art.py).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc'ed or owned by a torch tensor) unless marked host;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); all work is stream-ordered,
 *     nothing synchronises, nothing allocates;
 *   - dtype: EG_F32 (exact fp32 path, v_mfma_f32_16x16x4_f32) or EG_BF16 (bf16 storage, fp32 accumulate,
 *     v_mfma_f32_16x16x32_bf16).  Parameters, gradients, optimiser state, LayerNorm statistics,
 *     soft-max statistics and losses are always fp32;
 *   - return value: 0 on success, non-zero on a rejected call (eg_last_error() gives the text).
 *     Shape/argument checks happen on the host BEFORE any launch.
 */
#ifndef EYEGAZE_HIP_H
#define EYEGAZE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EG_ABI_VERSION 5
enum { EG_F32 = 0, EG_BF16 = 1, EG_F16 = 2 };
enum { EG_ACT_NONE = 0, EG_ACT_RELU = 1, EG_ACT_GELU = 2 };

int eg_abi_version(void);
const char* eg_last_error(void);
/* fills cu_count / arch name of the current device (host pointers) */
int eg_device_info(int* cu_count, char* arch, int arch_len);

/* Device-resident per-step scalars.  Kernels read them from memory (not from kernel arguments) so a
 * captured hipGraph of one training step replays correctly with a new seed / learning rate. */
typedef struct eg_step_state {
  uint32_t seed_lo, seed_hi; /* dropout seed of this step */
  float lr;                  /* learning rate (cosine schedule, T:409/494) */
  float bias_corr1;          /* 1 - beta1^t */
  float bias_corr2;          /* 1 - beta2^t */
  float grad_scale;          /* multiplies gradients before clipping (1/world_size for a summed all-reduce) */
  float clip_coef;           /* written by eg_clip_coef: min(1, max_norm/(norm+1e-6)) (T:221) */
  float grad_norm;           /* written by eg_clip_coef: global L2 norm before clipping (after un-scaling) */
  /* dynamic loss scaling (fp16 path; torch.cuda.amp.GradScaler semantics, train_multimodal_fuzzy_fusion.py:435-472).
   * These four words live on the device across steps; eg_set_step_state leaves them alone unless asked to reset. */
  float loss_scale;          /* the loss gradient fed to backward is multiplied by this; eg_clip_coef divides it out */
  uint32_t found_inf;        /* written by eg_clip_coef: 1 when the gradient norm is not finite -> eg_adamw skips the step */
  uint32_t good_steps;       /* consecutive finite steps since the last change of loss_scale */
  uint32_t opt_steps;        /* optimiser steps actually taken (skipped steps do not count); t of the bias corrections
                                when use_dev_t != 0 */
  uint32_t use_dev_t;        /* 0: bias_corr1/2 come from the host; 1: eg_adamw derives them from opt_steps + 1 */
  uint32_t skipped;          /* total skipped steps */
  uint32_t scaler_on;        /* 0: loss_scale is 1 and non-finite gradients are NOT intercepted (the reference's fp32 loop) */
  uint32_t _pad;
} eg_step_state;
/* Publishes the host-side scalars of a step.  They travel as KERNEL ARGUMENTS (copied at launch), so a host that runs
 * many steps ahead of the device can never overwrite a value a queued step still has to read.  reset_scaler: 0 leaves the
 * loss-scaling words alone; 1 enables scaling (loss_scale = init_scale, scaler_on = 1); 2 disables it (loss_scale = 1,
 * scaler_on = 0); 1 and 2 also zero found_inf / good_steps / opt_steps / skipped. */
int eg_set_step_state(eg_step_state* state, uint32_t seed_lo, uint32_t seed_hi, float lr, float bias_corr1,
                      float bias_corr2, float grad_scale, int reset_scaler, float init_scale, int use_dev_t, void* stream);

/* Grouped row addressing: row r of a logical [M, *] matrix starts at element
 *   (r / rows_per_group) * group_stride + (r % rows_per_group) * row_stride
 * rows_per_group == 0 means plain rows (r * row_stride).  This is how the strided 1-D convolutions read
 * overlapping windows of a channel-last, zero-padded signal as GEMM rows without an im2col copy. */
typedef struct eg_rowmap {
  int64_t row_stride;
  int64_t group_stride;
  int32_t rows_per_group;
  int32_t _pad;
} eg_rowmap;

/* ---------------------------------------------------------------------------------------------
 * Input staging — D:1127-1128 feed, 1_Data/processed/dual_eeg_dataset.py:236-248 layout [B,C,T] f32
 * x [NB, C, T] f32  ->  xt [NB, Tp, Cp] (dtype), channel-last, `pad_front` zero time steps in front,
 * zeros behind up to Tp, channels C..Cp-1 zero.  Coalesced reads along T, LDS transpose.
 * ------------------------------------------------------------------------------------------- */
int eg_window_pack(const float* x, void* xt, int NB, int C, int T, int Cp, int pad_front, int Tp, int dtype,
                   void* stream);
/* data-path normalisation (1_Data/processed/dual_eeg_dataset.py:142-168 when enable_preprocessing, :201-202 otherwise):
 *   raw [N, 2, C, T] f32 (player-1 window, player-2 window) -> eeg1, eeg2 [N, C, T] f32
 *   mode 0: per-window global z-score, population std + 1e-8
 *   mode 1: common-average reference, then per-channel z-score, population std + 1e-8 */
int eg_window_normalize(const float* raw, float* eeg1, float* eeg2, int N, int C, int T, int mode, void* stream);

/* The same normalisation on windows cut out of recordings that stay in device memory (data.py: the recording store).
 * Pair p holds its two players' channels as [2][C][pair_len[p]] f32 at float offset pair_off[p] of `data`; window w lies in pair
 * win_pair[w] and starts at sample win_start[w].  Window j of the batch is w = order[first + j]; channel c of its player `who` is
 * the T floats at
 *     data + pair_off[win_pair[w]] + (who * C + c) * pair_len[win_pair[w]] + win_start[w]         (64-bit arithmetic)
 * and eeg1 / eeg2 [n, C, T] receive them normalised in `mode` with the arithmetic of eg_window_normalize -- one body, two
 * addressings -- so they are, bit for bit, what eg_window_normalize gives on the same raw windows.  labels[j] = win_label[w]
 * (labels may be null; it must be null when win_label is).  Rows may start at any float: every access is 4 bytes wide.
 * Every pointer of the descriptor is a DEVICE pointer; the descriptor itself is host memory, as is eg_attn_block_desc.
 * The tables are trusted: whoever builds them proves 0 <= win_start[w], win_start[w] + T <= pair_len[win_pair[w]], every pair
 * inside `data`, and 0 <= order[i] < n_windows (data.validate_store).  Refused on the host: null pointers, n / C / T <= 0, empty
 * tables, mode outside {0, 1}, T > 16384, first < 0 or first + n > order_len, labels without win_label. */
typedef struct eg_window_gather_desc {
  const float* data;
  const int64_t* pair_off;    /* [n_pairs]   float offset of the pair in data */
  const int32_t* pair_len;    /* [n_pairs]   samples per channel row of the pair */
  const int32_t* win_pair;    /* [n_windows] */
  const int32_t* win_start;   /* [n_windows] */
  const int64_t* win_label;   /* [n_windows] or null */
  int32_t n_pairs, n_windows, C, T;
} eg_window_gather_desc;
int eg_window_gather(const eg_window_gather_desc* d, const int32_t* order, int order_len, int first, int n, float* eeg1,
                     float* eeg2, int64_t* labels, int mode, void* stream);

/* eg_window_gather's addressing, tables, order, outputs and labels without a normalisation: eeg1 / eeg2 [n, C, T] receive the
 * windows AS STORED, bit for bit (a store whose recordings were preprocessed whole, below, is cut this way).  Refused on the
 * host: what eg_window_gather refuses (there is no mode). */
int eg_window_cut(const eg_window_gather_desc* d, const int32_t* order, int order_len, int first, int n, float* eeg1,
                  float* eeg2, int64_t* labels, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Recording-level preprocessing (2_Preprocessing/scripts/preprocess_eeg_windows.py:145-172, preprocess_eeg): zero-phase
 * band-pass, common-average reference, per-channel z-score, over WHOLE recordings, in place, before windows are cut.
 * Both entry points work on n_rows channel rows of f32: row r is the row_len[r] floats at data + row_off[r]; rows are ragged;
 * C consecutive rows are one player's recording and share a length.  Every pointer of the descriptor is a DEVICE pointer; the
 * descriptor itself is host memory.  The tables are trusted: whoever builds them proves that every row lies inside `data`, that
 * rows do not overlap, that row_len[r] > 3 * ncoef, that lengths are equal inside a group of C and that ws_off is the running
 * sum of row_len + 6 * ncoef (data.preprocess_recordings).  max_len only sizes grids: a wrong value costs time, not bounds.
 * ------------------------------------------------------------------------------------------- */
typedef struct eg_recording_rows_desc {
  float* data;
  const int64_t* row_off;     /* [n_rows] float offset of the row in data */
  const int32_t* row_len;     /* [n_rows] samples of the row */
  const int64_t* ws_off;      /* [n_rows] offset (doubles) of the row's row_len + 6 ncoef workspace doubles; filtfilt only */
  int32_t n_rows, C, max_len, _pad;
} eg_recording_rows_desc;
/* scipy.signal.filtfilt(b, a, x) with its defaults, restated, over every row: pad = 3 ncoef; the row is extended oddly by pad
 * samples on both sides, 2 x[0] - x[pad..1] in front and 2 x[L-1] - x[L-2..L-pad-1] behind, IN FLOAT32 (scipy forms the
 * extension in its input's dtype); the forward pass runs over the extended row from state zi * ext[0], the backward pass over the
 * forward output, reversed, from state zi * (last forward output); the padding is dropped and the result rounded to f32 once.
 * Both passes and the intermediate (workspace: sum over rows of row_len + 2 pad doubles) are fp64; the recurrence is scipy's
 * transposed direct form II in its order: y = z[0] + b[0] x; z[i] = z[i+1] + b[i+1] x - a[i+1] y; z[n-1] = b[n] x - a[n] y.
 * b, a [ncoef], zi [ncoef - 1] are HOST doubles and travel as kernel arguments.  One lane owns one row and walks it
 * sequentially; a wave (one block) takes 64 consecutive rows.  Refused on the host: null pointers, n_rows <= 0, C <= 0, ncoef
 * outside [2, 17], a[0] != 1, workspace_capacity < workspace_need (both in doubles; workspace_need is the caller's sum). */
int eg_recording_filtfilt(const eg_recording_rows_desc* d, const double* b, const double* a, const double* zi, int ncoef,
                          double* workspace, int64_t workspace_need, int64_t workspace_capacity, void* stream);
/* eg_recording_filtfilt with every product and sum of the recurrence rounded on its own (no contracted multiply-adds): the
 * arithmetic of scipy's compiled loop, operation by operation.  For the narrow low bands of the trial features (0.5-4 Hz at 250 Hz)
 * the recurrence amplifies the rounding difference of a contracted multiply-add to 1e-4 of the signal; this entry point stays
 * on scipy's side of it.  Same arguments, same refusals; about three times the time per launch (measured: DESIGN.md §8m). */
int eg_recording_filtfilt_exact(const eg_recording_rows_desc* d, const double* b, const double* a, const double* zi, int ncoef,
                                double* workspace, int64_t workspace_need, int64_t workspace_capacity, void* stream);
/* preprocess_eeg's steps 2-3, in place: per group of C rows and per sample car = (sum over c in channel order, f32) / C,
 * v = x - car; per row out = (v - mean) / (std_pop + 1e-8) with mean and variance accumulated in double and rounded to f32
 * before use (eg_window_normalize's mode 1 arithmetic).  Two launches: a sample-parallel CAR pass, then one block per row.
 * Refused on the host: null pointers, n_rows <= 0, C <= 0, n_rows % C != 0. */
int eg_recording_car_zscore(const eg_recording_rows_desc* d, void* stream);
/* The CAR pass of eg_recording_car_zscore on its own -- the same kernel, so bit for bit that pass -- and no z-score
 * (2_Preprocessing/scripts/extract_eeg_features.py:183-186).  Refused on the host: what eg_recording_car_zscore refuses. */
int eg_recording_car(const eg_recording_rows_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Trial features (2_Preprocessing/scripts/extract_eeg_features.py): Welch PSD and band energies, the analytic
 * signal of a band-filtered trial, the pair sums of six connectivity metrics and the segment coherence.  All four work on
 * eg_recording_rows_desc rows with 2 C consecutive rows per TRIAL -- player 1's C channels, then player 2's -- of one length
 * L in [256, 65536].  Connectivity goes to con [n_trials][3][7][nbands][C][C] f32: matrix 0 = intra-brain player 1, 1 =
 * intra-brain player 2, 2 = inter-brain (rows: player 1, columns: player 2); metric order pearson, power_corr, plv, pli, wpli,
 * coherence, phase_diff.  The tables are trusted as above; additionally max_len must be the largest row_len (it sizes
 * workspaces; every kernel skips a row longer than max_len, so nothing is written out of bounds).  Every entry point refuses
 * on the host: null pointers, n_rows <= 0, C <= 0, n_rows % (2 C) != 0, max_len outside [256, 65536], a workspace below its need.
 * ------------------------------------------------------------------------------------------- */
#define EG_TRIAL_MIN_LEN 256
#define EG_TRIAL_MAX_LEN 65536
#define EG_TRIAL_NBINS 129
#define EG_TRIAL_MAX_BANDS 8
/* scipy.signal.welch(x, fs, nperseg=256) with its defaults, restated, per row: segments of 256 at a hop of 128 (no padding of
 * the tail), each minus its mean, periodic Hann window, 256-point FFT in LDS in fp64, |X|^2 / (fs sum w^2), bins 1..127
 * doubled, mean over the segments, rounded to f32 once: psd [n_rows][129].  energy [n_rows][nbands] = the mean of
 * psd[band_k0[b] .. band_k1[b]] (bins, inclusive; 0 for an empty range); band_k0 / band_k1 are HOST arrays.  *nonfinite
 * (device, may be null) is set to 1 when any psd value is not finite -- a NaN or Inf of the input reaches every bin of its row
 * through the filter -- and left alone otherwise.  Refused too: fs <= 0, nbands outside [0, 8], a bin outside [0, 128]. */
int eg_trial_welch(const eg_recording_rows_desc* d, double fs, const int32_t* band_k0, const int32_t* band_k1, int nbands,
                   float* psd, float* energy, int32_t* nonfinite, void* stream);
/* Doubles of workspace eg_trial_analytic needs besides the tables' own: the twiddle table of the largest transform (host only;
 * -1: max_len outside [256, 65536]). */
int64_t eg_trial_analytic_twiddle_doubles(int max_len);
/* The tables eg_trial_analytic reads, written into its workspace (doubles): [0, twiddle_doubles) the twiddles of the largest
 * transform; at chirp_off[g] (device, [n_rows / (2 C)], even) trial g's 2 M + 2 L doubles -- the spectrum of the circular chirp
 * filter and the chirp w[n] = exp(-i pi (n^2 mod 2 L) / L), the angle formed in integers -- M the smallest power of two
 * >= 2 L - 1.  They depend on the lengths alone: build them once and run eg_trial_analytic on as many band signals of the same
 * rows as there are.  Two launches: twiddles, one block per trial.  workspace_need is the caller's total for both entry points. */
int eg_trial_analytic_tables(const eg_recording_rows_desc* d, const int64_t* chirp_off, double* workspace, int64_t workspace_need,
                             int64_t workspace_capacity, void* stream);
/* scipy.signal.hilbert along time at every row's own length L, restated in fp64: DFT of length L, weights 1, 2..2, (1 at L/2
 * when L is even), 0..0, inverse DFT.  One path for every L: both transforms are chirp-z (Bluestein) transforms over a
 * power-of-two FFT of size M, from the tables eg_trial_analytic_tables wrote into the same workspace for the same descriptor.
 * Per row, f32, at the row's own offset row_off[r] of three planes shaped as `data`: amp = |z|, cs + i sn = z / |z|, (1, 0)
 * where |z| == 0.  `data` (the band signal) is only read.  ws_off[r] (even) is the row's own 2 M workspace doubles where
 * M > 8192 (a shorter row transforms in LDS and its ws_off is not read).  One launch, one block per row. */
int eg_trial_analytic(const eg_recording_rows_desc* d, const int64_t* chirp_off, float* amp, float* cs, float* sn,
                      double* workspace, int64_t workspace_need, int64_t workspace_capacity, void* stream);
/* Floats of workspace eg_trial_pairs needs (host only; -1: bad shape): 4 per row + 6 C C per trial, matrix and 256-sample split
 * of max_len. */
int64_t eg_trial_pairs_workspace_floats(int n_rows, int C, int max_len);
/* Six metrics of every channel pair (i, j) of the three matrices, over all L samples of the band signal x = data, its amplitude
 * a and unit phasor u = cs + i sn (eg_trial_analytic's planes), P_t = u_i(t) conj(u_j(t)), zs(v) = (v - mean) / (std_pop + 1e-8):
 *   pearson = mean zs(x_i) zs(x_j); power_corr = the same on a; plv = |mean P|; phase_diff = angle(mean P);
 *   pli = |mean sign(Im P)|; wpli = |mean Im P| / (mean |Im P| + 1e-8)
 * written to con[.][.][m][band] for m in {0, 1, 2, 3, 4, 6}.  Time is split over workgroups in chunks of 256 samples; the four
 * product sums of a chunk are f32 MFMA GEMMs over time, sign and |.| sums vector work on the same tiles with Im P formed from two
 * rounded products; the chunks are added in ascending order in fp64 by a second launch, so the result is bit-reproducible.  On
 * the diagonal of an intra matrix Im P counts as exactly 0: pli = wpli = phase_diff = 0.  Refused too: band outside
 * [0, nbands), nbands outside [1, 8]. */
int eg_trial_pairs(const eg_recording_rows_desc* d, const float* amp, const float* cs, const float* sn, float* workspace,
                   int64_t workspace_capacity, float* con, int band, int nbands, void* stream);
/* Floats of workspace eg_trial_coherence needs (host only; -1: bad shape): per row 129 (1 + 2 (max_len / 256)). */
int64_t eg_trial_coherence_workspace_floats(int n_rows, int max_len);
/* compute_coherence_fast / compute_inter_coherence (:409-462, :590-648) of the band signal: L / 256 segments of 256 without
 * overlap, symmetric Hann window (np.hanning, rounded to f32), 256-point FFT in fp64, Pxx = mean |X|^2, Pxy = mean X_i conj X_j,
 * con[.][.][5][band][i][j] = the mean over the 129 bins of |Pxy|^2 / (Pxx_i Pxx_j + 1e-8).  The 1e-8 is absolute: the rows are
 * not rescaled.  Two launches: spectra per row, then one block per (trial, matrix, i). */
int eg_trial_coherence(const eg_recording_rows_desc* d, float* workspace, int64_t workspace_capacity, float* con, int band,
                       int nbands, void* stream);
/* Spectral entropy (5_Metrics/entropy_calculators.py:323-344) per row: eg_trial_welch's segment loop -- the same
 * device function -- and, from the fp64 PSD BEFORE it is rounded to f32, q_k = |p_k| + eps, S = sum q_k, T = sum q_k ln q_k,
 * entropy[row] = (ln S - T / S) / ln 2 in bits, a double; both sums through the fixed-order block sum; a bin with q_k == 0 (only
 * where eps == 0) adds nothing.  eps is absolute (the calculator's 1e-10 on uV^2 / Hz).  psd [n_rows][129] (may be null) receives
 * exactly eg_trial_welch's floats.  The rows are ANY channel rows: single recordings, any C (the descriptor's C only has to divide
 * n_rows).  There is no flag: a NaN or Inf in a row makes that row's entropy NaN and touches no other row.  A row shorter than
 * 256 or longer than max_len is skipped.  One launch, one block per row.  Refused on the host: null pointers (d, its data and
 * tables, entropy), n_rows <= 0, C <= 0, n_rows % C != 0, max_len outside [256, 65536], fs <= 0, eps < 0. */
int eg_trial_spectral_entropy(const eg_recording_rows_desc* d, double fs, double eps, float* psd, double* entropy, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Spatial entropy of gaze heat-map images (5_Metrics/entropy_calculators.py:145-180) for a batch of ragged images
 * in one call.  Every pointer of the descriptor is a DEVICE pointer; the descriptor itself is host memory.  The tables are
 * trusted: whoever builds them proves that every image lies inside `data` (npix elements for grey, 3 npix for RGB, from element
 * off) and starts on a 16-byte boundary (an image that does not is still computed, through narrow loads).
 * All arithmetic is fp64.  Luminance g = (0.299 R + 0.587 G) + 0.114 B, every product and sum rounded on its own (numpy's
 * bits); with normalize: q = |(g - min) / ((max - min) + 1e-10)| + eps over the image's own min and max, without: q = |g| + eps;
 * S = sum q, T = sum q ln q (a pixel with q == 0 adds nothing), entropy[i] = (ln S - T / S) / ln 2 in bits.  A constant image
 * gives log2(npix).  No atomics: a workgroup owns EG_IMAGE_ENTROPY_CHUNK consecutive pixels of one image; launch 1 writes per
 * chunk (min, max), launch 2 folds its image's (min, max) in ascending order and writes per chunk (S, T), launch 3 adds an
 * image's chunks in ascending order.  So an image alone and inside any batch gives the same bytes, as do two runs.
 * An image with npix outside [1, max_pix] or a layout outside {0, 1, 2} is skipped on the device: its entropy is not written.
 * Refused on the host, before any launch: null pointers, n_images <= 0, max_pix outside [1, 2^24], elem outside {0, 1}, eps < 0,
 * a workspace below eg_image_entropy_workspace_doubles(n_images, max_pix).
 * ------------------------------------------------------------------------------------------- */
#define EG_IMAGE_ENTROPY_CHUNK 8192
typedef struct eg_image_batch_desc {
  const void* data;            /* every image's elements back to back; each image starts on a 16-byte boundary */
  const int64_t* off;          /* [n_images] element offset */
  const int32_t* npix;         /* [n_images] H * W */
  const int32_t* layout;       /* [n_images] 0 grey (H, W), 1 RGB pixel-interleaved (H, W, 3), 2 RGB planar (3, H, W) */
  int32_t n_images, max_pix, elem /* 0 uint8, 1 float64 */, normalize;
} eg_image_batch_desc;
/* Doubles of workspace eg_image_entropy needs: 4 per image and chunk of max_pix (host only; -1: bad shape). */
int64_t eg_image_entropy_workspace_doubles(int n_images, int max_pix);
int eg_image_entropy(const eg_image_batch_desc* d, double eps, double* workspace, int64_t workspace_capacity, double* entropy,
                     void* stream);

/* ---------------------------------------------------------------------------------------------
 * Exact t-SNE of [N, D] embeddings into two components (sklearn.manifold.TSNE with method="exact"; 5_Metrics/eeg_metrics.py:676-703,
 * DESIGN.md §8p) in stages.  Every stage is a deterministic function of its inputs: no atomics, every sum across lanes or
 * workgroups in fp64 and in a fixed order, so two runs give the same bytes.  Inputs are only read.  All pointers are device
 * pointers; matrices are dense row-major [N, N].  Every entry refuses on the host, before any launch: null pointers (stats of
 * eg_tsne_gradient / eg_tsne_update may be null), N outside [2, EG_TSNE_MAX_N], and a workspace below eg_tsne_workspace_bytes(N).
 *
 * eg_tsne_sqdist: dist[i][j] = sum_d (x_id - x_jd)^2 from the differences themselves, each squared and added in fp64 in ascending
 *   d, rounded once to f32: symmetric, zero diagonal.  Also refused: D outside [1, EG_TSNE_MAX_D].
 * eg_tsne_affinities: sklearn's _binary_search_perplexity, one workgroup per row i.  beta = 1 and an open bracket at the start; a
 *   step computes over j != i  p_j = exp(-dist_ij beta), S = sum p_j (1e-8 if 0), H = ln S + beta (sum dist_ij p_j) / S, all fp64,
 *   and ends the search when |H - ln perplexity| <= 1e-5; otherwise H too large: beta is the lower end, doubled while the upper
 *   end is open, else moved half way to it; H too small: the mirror image with halving.  A counted loop of at most 100 steps.
 *   cond[i][j] = p_j / S at the last beta evaluated (0 on the diagonal), beta[i] = that beta, steps[i] = the number of times beta
 *   moved (100: the search ran out).  Also refused: perplexity <= 0 or >= N, cond == dist.
 * eg_tsne_joint: P_ij = max((c_ij + c_ji) / T, 2^-52) with T = max(2 sum_all c, 2^-52), zero diagonal, symmetric.  Three launches:
 *   row sums, their fold, the tiles.  P may be written over the storage of dist; P == cond is refused.
 * eg_tsne_gradient: sklearn's _kl_divergence at one degree of freedom, fp64 throughout: w_ij = 1 / (1 + |y_i - y_j|^2),
 *   Z = sum_{i != j} w_ij, Q_ij = max(w_ij / Z, 2^-52), grad_i = 4 sum_j (e P_ij - Q_ij) w_ij (y_i - y_j) rounded once to f32, and
 *   with stats: stats[0] = sum_{i != j} e P_ij ln(max(e P_ij, 2^-52) / Q_ij); e = exaggeration.  Launch 1 writes per-workgroup
 *   sums of w, launch 2 folds them (every workgroup in the same order) and streams P once with the whole Y in LDS (8 N bytes), a
 *   third folds the per-workgroup KL sums when stats is given.  Y on an 8-byte boundary.  Also refused: exaggeration <= 0.
 * eg_tsne_update: sklearn's _gradient_descent body, every product and sum a rounded f32 operation: gains += 0.2 where
 *   update grad < 0, else gains *= 0.8; gains = max(gains, min_gain); g = grad gains; update = momentum update - learning_rate g;
 *   Y += update; with stats: stats[1] = sum g^2 in fp64.  Y, update and gains [N, 2] are updated in place, grad is only read.
 *   One workgroup.  Also refused: learning_rate <= 0, momentum < 0, min_gain <= 0.
 * ------------------------------------------------------------------------------------------- */
#define EG_TSNE_MAX_N 16384
#define EG_TSNE_MAX_D 4096
/* Bytes of workspace eg_tsne_joint and eg_tsne_gradient need for N points (host only; -1: N out of range). */
int64_t eg_tsne_workspace_bytes(int N);
int eg_tsne_sqdist(const float* X, int N, int D, float* dist, void* stream);
int eg_tsne_affinities(const float* dist, int N, double perplexity, float* cond, double* beta, int32_t* steps, void* stream);
int eg_tsne_joint(const float* cond, int N, void* workspace, int64_t workspace_bytes, float* P, void* stream);
int eg_tsne_gradient(const float* Y, const float* P, double exaggeration, int N, void* workspace, int64_t workspace_bytes,
                     float* grad, double* stats, void* stream);
int eg_tsne_update(float* Y, float* update, float* gains, const float* grad, int N, float momentum, float learning_rate,
                   float min_gain, double* stats, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gaze heat-map images as the multimodal trainer's input (1_Data/processed/multimodal_dataset.py:67-83): resized
 * once into a uint8 store, then one launch per training batch.  All of it is integer or table arithmetic and bit-exact.
 *
 * eg_gaze_resize: n_images pixel-interleaved (h, w, 3) uint8 images back to back in `data`, image i at BYTE offset off[i], ->
 * store [n_images, F, W, 3] uint8, the bytes of Pillow's Image.resize((W, F), BILINEAR): its antialiased two-pass resample,
 * horizontally into a uint8 intermediate (h, W, 3) in the workspace (at byte offset mid_off[i]), then vertically.  One axis
 * (in -> out) is a table of out rows (xmin, count, k[ksize]) built by the host in fp64 (gaze.resize_tables):
 *   scale = in / out, fscale = max(scale, 1), support = fscale, ksize = 2 ceil(support) + 1, center = (xx + 0.5) scale,
 *   xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), in), count = xmax - xmin,
 *   w[x] = max(0, 1 - |(x + xmin - center + 0.5) / fscale|) divided by their sequential sum, k[x] = int(0.5 + w[x] 2^22)
 * and a pixel is clip((2^21 + sum_x src[xmin + x] k[x]) >> 22, 0, 255) in 32-bit integers.  A table lies at 32-bit word htab[i]
 * (horizontal, w[i] -> W) or vtab[i] (vertical, h[i] -> F) of `tabs` as [0] ksize, [1 .. out] xmin, [1 + out .. 2 out] count, then
 * k [out][ksize].  Two launches, no atomics: the horizontal pass stages a source row in LDS once by 16-byte loads and runs its
 * threads over (x_out, channel); the vertical pass runs its threads over 16, 4 or 1 consecutive bytes of an output row (the widest
 * that divides W * 3) and loops over the taps' rows.  An image alone and inside any batch gives the same bytes.
 * Served: 1 <= h, w <= EG_GAZE_MAX_SIDE, EG_GAZE_MIN_OUT <= F, W <= EG_GAZE_MAX_OUT.  An image whose h or w is outside is skipped
 * on the device: its store rows are not written.  Every pointer of the descriptor is a DEVICE pointer; the descriptor itself is
 * host memory.  The tables are trusted (gaze.validate_resize_tables, gaze.GazeImageStore prove them): every image inside `data`,
 * off[i] and mid_off[i] multiples of 16 with `data` readable up to the next multiple of 16 behind every image, mid_off the running
 * sum of 3 W h[i] rounded up to 16, 0 <= xmin, xmin + count <= in, count <= ksize.  max_h only sizes the grid; sum_h is the sum of
 * the heights.  Refused on the host, before any launch: null pointers, n_images <= 0, F / W / max_h outside the served range, a
 * sum_h that no n_images heights give, a workspace below eg_gaze_resize_workspace_bytes(n_images, sum_h, W), data / workspace /
 * store off a 16-byte boundary.
 * ------------------------------------------------------------------------------------------- */
#define EG_GAZE_MAX_SIDE 4096
#define EG_GAZE_MIN_OUT 8
#define EG_GAZE_MAX_OUT 512
typedef struct eg_gaze_resize_desc {
  const uint8_t* data;
  const int64_t* off;          /* [n_images] byte offset of the image, a multiple of 16 */
  const int32_t* h;            /* [n_images] */
  const int32_t* w;            /* [n_images] */
  const int64_t* mid_off;      /* [n_images] byte offset of the image's (h, W, 3) intermediate in the workspace, a multiple of 16 */
  const int32_t* tabs;         /* every distinct axis table */
  const int64_t* htab;         /* [n_images] word offset in tabs of the table w[i] -> W */
  const int64_t* vtab;         /* [n_images] word offset in tabs of the table h[i] -> F */
  int64_t sum_h;
  int32_t n_images, max_h, F, W;
} eg_gaze_resize_desc;
/* Bytes of workspace eg_gaze_resize needs: 3 W sum_h + 16 n_images (host only; -1: n_images <= 0, sum_h outside
 * [n_images, 4096 n_images], W outside the served range). */
int64_t eg_gaze_resize_workspace_bytes(int n_images, int64_t sum_h, int W);
int eg_gaze_resize(const eg_gaze_resize_desc* d, uint8_t* workspace, int64_t workspace_bytes, uint8_t* store, void* stream);

/* One training batch out of the store, in ONE launch, addressed as eg_window_gather addresses its windows: sample j of the batch is
 * window w = order[first + j], and its player pl reads image store[pair_img[2 win_pair[w] + pl]] ([F, W, 3] uint8).  Outputs:
 * img1 / img2 [n, F, W] f32 (player 1 / 2; what ImageEngine.forward takes) and, unless null, rgb1 / rgb2 [n, 3, F, W] f32 (the
 * reference's own tensors; both or neither).
 *   rgb[c][y][x] = norm[c][v]      norm [3][256] f32 (device), filled by the host with (float32(v) / 255 - mean_c) / std_c in torch
 *                                  fp32 operations (gaze.normalise_table): ToTensor followed by Normalize, exact by construction
 *   img[y][x]    = ((r + g) + b) / 3.0f, the division correctly rounded: tensor.mean(dim=0)
 * Augmentation runs iff hflip_p, brightness, contrast are not all 0 (or factors is given), each (j, pl) on its own, on the uint8
 * pixels v before the table, from counter i = 2 (first + j) + pl and H(site) = eg_hash(seed_lo, seed_hi, site, i) of
 * csrc/common.h, u(site) = (H(site) >> 8) 2^-24:
 *   flip (x mirrored) iff u(IMG_FLIP) < hflip_p;  fb = (1 - brightness) + (2 brightness) u(IMG_BRIGHT), fc likewise from contrast and
 *   u(IMG_CONTRAST), every operation a rounded fp32 one;  brightness goes first iff H(IMG_ORDER) >> 31 == 0
 *   brightness: v' = uint8(trunc(clip(float32(v) fb, 0, 255)))
 *   contrast:   v' = uint8(trunc(clip(m + fc (float32(v) - m), 0, 255))), product and sum rounded separately (no fused multiply-
 *               add); m = int(mean_L + 0.5), mean_L the fp64 mean over the image AS IT STANDS when contrast is applied of
 *               L = (19595 R + 38470 G + 7471 B + 32768) >> 16 (an integer sum: its order is free)
 * These are PIL.ImageEnhance.Brightness / Contrast on the resized image, byte for byte.  factors (device, [2 n][4] f32, may be
 * null) replaces the draws of image 2 j + pl by (flip != 0, fb, fc, brightness first != 0): it exists for parity tests against
 * Pillow at given factors, no product path passes it.  One workgroup per (j, pl); with contrast the image is read twice (luminance
 * sum, then the write).  The tables are trusted (gaze.GazeImageStore.batch validates pair_img; order and win_pair are
 * ResidentWindows'); an image index outside [0, n_images) is skipped on the device.  Refused on the host: null pointers (rgb* and
 * factors may be null), n <= 0, n_images <= 0, F / W outside the served range, first < 0 or first + n > order_len, hflip_p outside
 * [0, 1], brightness or contrast outside [0, 1) or not finite, one of rgb1 / rgb2 without the other. */
int eg_gaze_batch(const uint8_t* store, int n_images, int F, int W, const int32_t* pair_img, const int32_t* win_pair,
                  const int32_t* order, int order_len, int first, int n, const float* norm, uint32_t seed_lo, uint32_t seed_hi,
                  float hflip_p, float brightness, float contrast, const float* factors, float* img1, float* img2, float* rgb1,
                  float* rgb2, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gaze pair analysis over the store (6_Utils/error_analysis.py:277-358 compute_gaze_distance / compute_gaze_overlap):
 * the per-pair table of the reference's spatial-sensitivity analysis in two launches.  store [n_images, F, W, 3] uint8, pair_img
 * [n_pairs, 2] int32, norm [3][256] f32 (the table of eg_gaze_batch, or float32(v) / 255 in every channel for raw ToTensor
 * tensors), out [n_pairs][EG_GAZE_PAIR_FIELDS] f64; all device pointers.  A pixel is t_c = norm[c][v_c],
 * g = ((t0 + t1) + t2) / 3.0f, the division correctly rounded and nothing fused: tensor.mean(dim=0), bit for bit.
 *   launch 1, workgroup = image (EVERY image of the store, once): min and max of g in fp32, and in fp64 S = sum g,
 *     Sy = sum fl32(g float(y)), Sx = sum fl32(g float(x)), A = sum |g| -- the products rounded to fp32 as torch rounds them, the
 *     sums in ONE order that depends only on (F, W): per-thread strided partials, a fixed butterfly inside the wave, the waves in
 *     ascending order.  -> workspace [n_images][8] f64: S, Sy, Sx, A, min, max, 0, 0.
 *   launch 2, workgroup = pair (a, b): g of both images again, q = (g - min) / ((max - min) + 1e-8f) in rounded fp32 operations,
 *     the masks q > threshold, integer counts na, nb, inter.  The row:
 *       [0] distance = sqrt((cy_a - cy_b)^2 + (cx_a - cx_b)^2) in fp64, a centre being (Sy / S, Sx / S), or the reference's LITERAL
 *           (112, 112) when S < 1e-8, whatever F and W are
 *       [1] overlap = double(float(inter) / float(union)), union = na + nb - inter; 0.0 when union == 0
 *       [2..5] cy_a, cx_a, cy_b, cx_b   [6..9] inter, union, na, nb   [10..13] S_a, S_b, A_a, A_b
 * No atomics: a row's bytes depend on its two images alone, not on the batch, the run, or where in the store the images lie
 * (16-byte loads where an image starts on a 16-byte boundary, byte loads where not, the same pixels to the same thread).
 * A pair with an image index outside [0, n_images) is skipped on the device: its row is not written.  Inputs are only read.
 * Refused on the host, before any launch: null pointers, n_images <= 0, n_pairs <= 0, F / W outside [EG_GAZE_MIN_OUT,
 * EG_GAZE_MAX_OUT], a threshold that is not finite, a workspace below eg_gaze_pair_stats_workspace_bytes(n_images), workspace or
 * out off an 8-byte boundary.
 *
 * eg_row_cosine: out[i] = float(dot / (max(sqrt(|a_i|^2), 1e-12) max(sqrt(|b_i|^2), 1e-12))) for rows of two [N, D] f32 arrays
 * (error_analysis.py:460-464: F.normalize on both, then the sum of products), dot and both squared norms in fp64, one wave per
 * row, lane l over columns l, l + 64, ... then a fixed butterfly.  Refused on the host: null pointers, N <= 0, D outside
 * [1, EG_ROW_COSINE_MAX_D].
 * ------------------------------------------------------------------------------------------- */
#define EG_GAZE_PAIR_FIELDS 14
#define EG_ROW_COSINE_MAX_D 4096
/* Bytes of workspace eg_gaze_pair_stats needs: 64 per image (host only; -1: n_images <= 0). */
int64_t eg_gaze_pair_stats_workspace_bytes(int n_images);
int eg_gaze_pair_stats(const uint8_t* store, int n_images, int F, int W, const int32_t* pair_img, int n_pairs, const float* norm,
                       float threshold, void* workspace, int64_t workspace_bytes, double* out, void* stream);
int eg_row_cosine(const float* a, const float* b, int N, int D, float* out, void* stream);

/* Training-time window augmentation in ONE launch (the reference lab's EEG recipe, 4_Experiments/experiments_list.md:304-310:
 * Gaussian noise, channel dropout, time masks).  in1/in2 -> out1/out2, each [N, C, T] f32, contiguous; out may alias in; player
 * pl = 0 for buffer 1 and 1 for buffer 2.  Every draw is counter-based: H(site, i) = eg_hash(state->seed_lo, state->seed_hi,
 * site, i), the full 32-bit word of csrc/common.h; half(site, e) = the 16-bit half of H(site, e >> 1) that eg_dropout uses for
 * element e (low half for even e, high half for odd e).  The seed is read from *state on the device, so a captured launch
 * draws anew at every replay; *state is only read.  Applied in this order:
 *   noise (noise_std > 0): element e = ((pl N + w) C + c) T + t, pair q = e >> 1 (pairs run over the flat index: with odd T a
 *     pair straddles two rows);  u1 = ((H(NOISE_R, q) >> 9) + 0.5f) 2^-23  (exact in fp32, inside (0, 1));
 *     u2 = (H(NOISE_T, q) >> 8) 2^-24;  r = sqrtf(-2 logf(u1));  (s, c) = sincospif(2 u2);  n = r c for even e, r s for odd e;
 *     y = fmaf(noise_std, n, x)
 *   channel dropout (chan_drop_p > 0): row e = (pl N + w) C + c is kept iff half(CHAN, e) >= round(chan_drop_p 65536); a dropped
 *     row is exact 0.0f, a kept row is NOT rescaled (a dead electrode); the two players draw independently
 *   time masks (n_masks in [0, 8]): mask j of window w: h = H(TIME, 8 w + j), L = min(mask_max_len, T),
 *     len = 1 + (((h & 0xFFFF) L) >> 16), start = ((h >> 16) (T - len + 1)) >> 16; samples [start, start + len) are exact 0.0f in
 *     every channel of BOTH players (their windows stay aligned)
 * Zeros win over noise; with noise_std == 0 every element that is not zeroed is copied bit for bit.  Refused on the host:
 * null pointers, N / C / T <= 0, noise_std negative or not finite, chan_drop_p outside [0, 1), n_masks outside [0, 8],
 * mask_max_len < 1 with n_masks > 0, 2 N C T >= 2^32. */
#define EG_SITE_AUG_NOISE_R 8   /* sites 1-7 and >= 16 are taken (engine.py: SITE_*, _layer_sites) */
#define EG_SITE_AUG_NOISE_T 9
#define EG_SITE_AUG_CHAN    10
#define EG_SITE_AUG_TIME    11
#define EG_SITE_IMG_FLIP     12  /* eg_gaze_batch's draws (above); 12-15 were the last free sites below 16 */
#define EG_SITE_IMG_BRIGHT   13
#define EG_SITE_IMG_CONTRAST 14
#define EG_SITE_IMG_ORDER    15
int eg_window_augment(const float* in1, const float* in2, float* out1, float* out2, int N, int C, int T,
                      float noise_std, float chan_drop_p, int n_masks, int mask_max_len,
                      const eg_step_state* state, void* stream);

/* Parameter staging (fp32 master -> compute dtype copies), run once per optimiser step.
 *   eg_cast:             n contiguous elements
 *   eg_transpose_cast:   src [R, Cc] f32 -> dst[c*ldd + r]         (weights for backward-data GEMMs)
 *   eg_pack_conv_weight: w [N, Cin, k] f32 -> dst [N, Kp], dst[n][tap*Cp + c] = w[n][c][tap], zero padded
 *                        (D:154,158 Conv1d weights in the tap-major order the channel-last GEMM rows need)
 *   eg_pack_convT_weight: backward-data weights of the stride-s conv, one matrix per output phase p:
 *                        dst[p][c][j*N + n] = w[n][c][s*(J-1-j) + p] (0 where the tap is > k-1), J = ceil(k/s)
 */
/* eg_pack_table: all of the above casts / transposes of one model in ONE launch.  `table` is a DEVICE array; entry i owns
 * blocks [blk0, blk0 + nblk): mode 0 cast (1024 elements per block), 1 transpose-cast (one 32x32 tile per block),
 * 2 fp32 copy (fused bias vectors); 3-6 eg_ffn_chain's MFMA-fragment order of a 16-bit weight (2048 elements per block; the
 * source is fp32 [rows, cols]): 3 role 1 = src [F, 256], 4 role 1 = src^T (src [256, F]), 5 role 2 = src [256, F],
 * 6 role 2 = src^T (src [F, 256]); see eg_ffn_desc; 7 / 8 eg_attn_block_fwd's fragment order of a [256, 256] projection weight
 * (7: q / k / v_proj with ldd = 0 / 1 / 2, 8: out_proj; 2048 elements per block).  src / dst are absolute device addresses. */
typedef struct eg_pack_entry {
  uint64_t src, dst;
  int32_t rows, cols, ldd, mode, blk0, nblk;
} eg_pack_entry;
int eg_pack_table(const eg_pack_entry* table, int nentries, int total_blocks, int dtype, void* stream);
/* eg_pack_table_ex: eg_pack_table's modes 0-8 (same bytes) plus the two convolution weight layouts, so that ONE launch stages
 * every weight of a step:
 *   mode 9  = eg_pack_conv_weight:  rows = N, cols = Cin, p0 = k, p1 = Cp, p2 = Kp       (N * Kp destination elements)
 *   mode 10 = eg_pack_convT_weight: rows = N, cols = Cin, p0 = k, p1 = stride, p2 = J    (stride * Cin * J * N elements)
 * both counted at 1024 destination elements per block (nblk; which elements a block serves is the kernel's business: it
 * stages whole (row, channel-chunk) units through LDS).  src_elems / dst_elems are the extents (fp32 source elements, destination
 * elements) of the buffers behind src / dst from those addresses on, 0 = not stated (modes 9 / 10 must state both).
 * eg_pack_table_ex_check audits a HOST copy of the table when it is built -- block ranges, per-mode shape rules, alignment and
 * the stated extents -- and returns the launch's block count; eg_pack_table_ex launches the DEVICE copy. */
typedef struct eg_pack_entry_ex {
  uint64_t src, dst;
  int32_t rows, cols, ldd, mode, blk0, nblk;
  int32_t p0, p1, p2, p3;
  int64_t src_elems, dst_elems;
} eg_pack_entry_ex;
int eg_pack_table_ex_check(const eg_pack_entry_ex* table, int nentries, int dtype, int* total_blocks);
int eg_pack_table_ex(const eg_pack_entry_ex* table, int nentries, int total_blocks, int dtype, void* stream);
int eg_cast(const float* src, void* dst, int64_t n, int dtype, void* stream);
int eg_transpose_cast(const float* src, void* dst, int R, int Cc, int ldd, int dtype, void* stream);
int eg_pack_conv_weight(const float* w, void* dst, int N, int Cin, int k, int Cp, int Kp, int dtype, void* stream);
int eg_pack_convT_weight(const float* w, void* dst, int N, int Cin, int k, int stride, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * eg_gemm_nt — the MFMA workhorse.  Y = epilogue(A[M,K] * W[N,K]^T)
 *   replaces: Conv1d+ReLU+Dropout (D:154-171) via grouped rows, q/k/v/out projections (A:203-213),
 *   FeedForward linears (A:272), head linears (D:939, D:1100-1105, D:1074-1079), tokenizer / spectrogram
 *   projections (D:81-86, D:863-868) and every backward-data product.
 *   epilogue, in this order:  v = acc + bias[n]; v = act(v); v = gate>0 ? v*gate_scale : 0; v = drop1(v);
 *   v = drop2(v); if (out_pre) out_pre = v; v += residual; C = v
 *   K % (128/sizeof(elem)) == 0, N % 8 == 0; rows beyond M are neither read past nor written.
 * ------------------------------------------------------------------------------------------- */
typedef struct eg_gemm_desc {
  const void* A;        /* activations, rows addressed by `a` */
  const void* W;        /* [N, ldw] row-major, K contiguous */
  void* C;              /* rows addressed by `c` */
  const float* bias;    /* [N] fp32 or NULL */
  const void* residual; /* rows addressed by `r`, same dtype, or NULL */
  const void* gate;     /* rows addressed by `c`; output zeroed where gate <= 0 (ReLU backward), or NULL */
  void* out_pre;        /* rows addressed by `p`; value before the residual add, or NULL */
  const eg_step_state* state; /* dropout seed; may be NULL when both p are 0 */
  eg_rowmap a, c, r, p; /* p addresses out_pre */
  int32_t M, N, K, ldw;
  int32_t act;
  int32_t dtype;
  float drop1_p, drop2_p;
  uint32_t drop1_site, drop2_site;
  float gate_scale; /* 1/(1-p) of the dropout that followed the gated ReLU in the forward pass, else 1 */
  int32_t a_seg_len;    /* 0, or: an A row is K/a_seg_len segments of a_seg_len contiguous elements ... */
  int64_t a_seg_stride; /* ... a_seg_stride elements apart (rows of a 2-D convolution window, D:74) */
} eg_gemm_desc;
int eg_gemm_nt(const eg_gemm_desc* d, void* stream);
/* Which kernel eg_gemm_nt launches for `d` (no launch; a measurement aid so that per-launch timings can be attributed):
 * EG_ROUTE_TILED gemm_nt_kernel (128x128 tile), EG_ROUTE_WIDE gemm_nt_wide_kernel (160x256, N == 256),
 * EG_ROUTE_ROWSTREAM rs_gemm_kernel (K == 256, register-stationary weights). */
enum { EG_ROUTE_TILED = 0, EG_ROUTE_WIDE = 1, EG_ROUTE_ROWSTREAM = 2 };
int eg_gemm_nt_route(const eg_gemm_desc* d);
/* The wide kernel's row tile: 160 or 128 rows x 256 columns.  eg_gemm_wide_rows is the host rule for an M-row product on
 * `cus` compute units (one workgroup per CU at a time): the tile with fewer resident rounds, on a tie the one that stages
 * fewer bytes per CU.  EYEGAZE_WIDE_TILE=128|160 forces a tile for the process; eg_gemm_wide_config does the same at run time
 * (tile_rows 0 = by rule) and sets the row count below which a product keeps the 128x128 tile (default 1024); -1 leaves a
 * setting as it is.  Every tile gives the same bits. */
int eg_gemm_wide_rows(int M, int cus);
int eg_gemm_wide_config(int tile_rows, int min_rows);
/* eg_gemm_nt_batch — n <= EG_GEMM_BATCH_MAX products of one dtype and one epilogue kind (the same activation and the same
 * set of bias / gate / dropout / out_pre / residual steps), each with its own operands, row maps, M and K.  Where every
 * product fits the wide kernel (N == 256, 16-bit, see eg_gemm_nt_route) they run as ONE grid, deepest K first; otherwise as n
 * eg_gemm_nt launches.  The results are those of n eg_gemm_nt calls, bit for bit.  All checks are made before any launch.
 * eg_gemm_nt_batch_route: 1 = one grid, 0 = n launches, -1 = refused (eg_last_error says why); no launch. */
#define EG_GEMM_BATCH_MAX 8
int eg_gemm_nt_batch(const eg_gemm_desc* descs, int n, void* stream);
int eg_gemm_nt_batch_route(const eg_gemm_desc* descs, int n);

/* ---------------------------------------------------------------------------------------------
 * eg_ffn_chain — the two products of the position-wise feed-forward block (A:264-272) in one launch, d_model == 256:
 *   H[M,F]   = drop_h(gate(act1(A[M,256] * W1[F,256]^T + bias1)))       stored (backward and the weight gradients read it)
 *   C[M,256] = drop_c2(drop_c1(H * W2[256,F]^T + bias2)) + residual
 *   forward  (A:272 linear1 -> ReLU -> dropout -> linear2, then A:294 dropout + residual): A = residual = LayerNorm-1 rows
 *   backward-data of the same block: A = dY, W1 = linear2^T, gate = the saved H rows (value zeroed where gate <= 0, else
 *   scaled by gate_scale), W2 = linear1^T, residual = the gradient arriving on the skip path.
 *   Bit-identical to the two eg_gemm_nt launches it replaces (same MFMA chains, epilogue order and dropout indices m*N + n);
 *   the hidden rows cross HBM once (the stored H) instead of three times.  16-bit dtypes, F % 128 == 0, strides in elements.
 *   LEAN form (a forward that nobody differentiates): H and C both NULL.  Then nothing but ln_out is stored -- the hidden chunk
 *   still passes through LDS rounded to 16 bit and C is still rounded before the LayerNorm, so ln_out has the bits of the keeping
 *   form.  It needs the forward form (bias1, ReLU, no gate, no gate_bits_in), ln_out, and no gate_bits_out; ln_stats is not
 *   written; ldh / ldc are not read.  One of H and C alone is refused, as is every other partial combination, before any launch.
 * ------------------------------------------------------------------------------------------- */
typedef struct eg_ffn_desc {
  const void* A;        /* [M, 256], row stride lda */
  const void* W1;       /* [F, 256] in fragment order: eg_pack_table mode 3 (or 4 from the transposed parameter) */
  const void* W2;       /* [256, F] in fragment order: eg_pack_table mode 5 (or 6) */
  void* H;              /* [M, F], row stride ldh; NULL together with C: the lean form */
  void* C;              /* [M, 256], row stride ldc; NULL together with H */
  const float* bias1;   /* [F] or NULL */
  const float* bias2;   /* [256] or NULL */
  const void* gate;     /* [M, F], row stride ldg, or NULL */
  /* The same gate as one bit per element ("stored H value > 0"), written by a launch with gate_bits_out set and read by a
   * later launch with gate_bits_in set (then `gate` is not read).  Opaque, in the kernel's own lane order: valid only between
   * launches with equal M and F; size eg_ffn_gate_bits_bytes(M, F). */
  void* gate_bits_out;
  const void* gate_bits_in;
  const void* residual; /* [M, 256], row stride ldr, or NULL; may alias A (then it is taken from the on-chip A tile) */
  const eg_step_state* state;
  int64_t lda, ldh, ldc, ldg, ldr;
  int32_t M, F, act1, dtype;
  float drop_h_p, drop_c1_p, drop_c2_p;
  uint32_t drop_h_site, drop_c1_site, drop_c2_site;
  float gate_scale;
  /* optional (forward): the layer's second LayerNorm (A:295, norm2) on the completed C rows, in the same launch:
   * ln_out = LayerNorm(C) * gamma + beta, ln_stats as eg_layernorm_fwd's.  NULL ln_out = off; needs ldc == 256. */
  const float* ln_gamma;
  const float* ln_beta;
  void* ln_out;         /* out [M, 256] contiguous */
  float* ln_stats;      /* out [M, 2] or NULL */
} eg_ffn_desc;
int eg_ffn_chain(const eg_ffn_desc* d, void* stream);
int64_t eg_ffn_gate_bits_bytes(int M, int F);

/* ---------------------------------------------------------------------------------------------
 * eg_ln_bwd_proj — LayerNorm backward (d_model = 256) and the backward-data product that consumes it, one launch over 80-row tiles:
 *   dx = LayerNorm backward of dy (what eg_layernorm_bwd writes, bit for bit), dx_drop = dropout1(dropout2(dx)) (ditto),
 *   dC = dx_drop * W^T with W[256, 256] pre-packed in fragment order (eg_pack_table mode 5 / 6; bit-identical to eg_gemm_nt),
 *   partial[block][512] = the block's gain | bias gradient sums (eg_ln_bwd_proj_blocks(M) rows; reduce with eg_reduce_partials).
 *   Replaces autograd's backward of `norm1` (A:293) + of `out_proj` (A:213) of an encoder layer.  16-bit dtypes.
 * ------------------------------------------------------------------------------------------- */
typedef struct eg_ln_bwd_proj_desc {
  const void* dy;       /* [M, 256] gradient of the LayerNorm output */
  const void* x;        /* [M, 256] the LayerNorm input */
  const float* stats;   /* [M, 2] mean, rstd of the forward */
  const float* gamma;   /* [256] */
  const void* W_frag;   /* 256 x 256 elements in fragment order */
  void* dx;             /* out [M, 256] */
  void* dx_drop;        /* out [M, 256] */
  void* dC;             /* out [M, 256] */
  float* partial;       /* out [blocks, 512] */
  const eg_step_state* state;
  int32_t M, d_model, dtype, partial_capacity_blocks;
  float drop1_p, drop2_p;
  uint32_t drop1_site, drop2_site;
} eg_ln_bwd_proj_desc;
int eg_ln_bwd_proj(const eg_ln_bwd_proj_desc* d, void* stream);
int eg_ln_bwd_proj_blocks(int M);   /* rows of `partial` a launch over M rows writes */

/* ---------------------------------------------------------------------------------------------
 * eg_ffn_bwd_ln_proj — eg_ffn_chain in its backward form with eg_ln_bwd_proj as the launch's tail: both kernels walk the same
 *   80-row tiles, so the rows C that the first completes (dy1, the gradient of the norm-1 output) stay on the chip as the second's dy.
 *   f: the backward form only -- gate_bits_in and H set; no bias1, act1, gate, gate_bits_out or ln_out.  f->C may be NULL: then dy1
 *      is not stored at all.
 *   n: as for eg_ln_bwd_proj with n->dy NULL or equal to f->C; n->M == f->M, equal dtypes, d_model == 256, and `partial` with at
 *      least eg_ln_bwd_proj_blocks(M) rows.
 *   H, C (when given), dx, dx_drop, dC and every row of `partial` have the bits of eg_ffn_chain(f) followed by eg_ln_bwd_proj(n) on
 *   that C: same tiles, arithmetic and summation order.  Every check of both descriptors is made before the launch.
 * ------------------------------------------------------------------------------------------- */
int eg_ffn_bwd_ln_proj(const eg_ffn_desc* f, const eg_ln_bwd_proj_desc* n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * eg_attn_block_fwd — the attention half of a post-LN encoder layer in ONE launch, a workgroup per WINDOW (S <= 80 rows):
 *   q|k|v = x Wqkv^T + b (A:203-205) -> softmax(q k^T / sqrt(32)), attention dropout, P v per head (A:206-212) ->
 *   r1 = x + dropout(ctx Wo^T + bo) (A:213, A:292-293's residual; the LayerNorm stays eg_layernorm_fwd).
 *   Stored: qkv [NB*S, 768], lse [NB, 8, S], ctx [NB*S, 256] (what eg_attention_bwd and the weight gradients read) and r1.
 *   Bit-identical to eg_gemm_nt (q|k|v) -> eg_attention_fwd (kv_shift 0) -> eg_gemm_nt (out-proj, drop1 = out_drop, residual x).
 *   16-bit dtypes, d_model == 256, 8 heads; rows contiguous (stride 256 / 768).  Weights in fragment order: wqkv_frag by three
 *   eg_pack_table entries of mode 7 (ldd = 0, 1, 2 for q_proj, k_proj, v_proj, same dst), wo_frag by one entry of mode 8.
 *   LEAN form (a forward that nobody differentiates): qkv, ctx, lse and r1 ALL NULL.  Then ln_out is required and is the launch's
 *   only result (same bits as the keeping form's: r1 is still rounded to 16 bit before the LayerNorm); ln_stats may be NULL and
 *   is not written.  Some but not all of the four NULL is refused before any launch.
 * ------------------------------------------------------------------------------------------- */
typedef struct eg_attn_block_desc {
  const void* x;          /* [NB*S, 256] */
  const void* wqkv_frag;  /* 768 x 256 elements, eg_pack_table mode 7 */
  const void* wo_frag;    /* 256 x 256 elements, eg_pack_table mode 8 */
  const float* bqkv;      /* [768] = q_proj.bias | k_proj.bias | v_proj.bias */
  const float* bo;        /* [256] */
  void* qkv;              /* out [NB*S, 768]    -- these four: all given, or all NULL (the lean form) */
  void* ctx;              /* out [NB*S, 256] */
  float* lse;             /* out [NB, 8, S] */
  void* r1;               /* out [NB*S, 256] */
  const eg_step_state* state;
  int32_t NB, S, d_model, num_heads, dtype;
  float attn_drop_p, out_drop_p;
  uint32_t attn_drop_site, out_drop_site;
  /* optional: the layer's first LayerNorm (A:293, norm1 of the post-LN layer) on the completed rows, in the same launch:
   * ln_out = LayerNorm(r1) * gamma + beta, ln_stats[2 m] = mean, [2 m + 1] = rstd (what eg_layernorm_fwd writes).  NULL ln_out = off. */
  const float* ln_gamma;
  const float* ln_beta;
  void* ln_out;           /* out [NB*S, 256] */
  float* ln_stats;        /* out [NB*S, 2] or NULL */
} eg_attn_block_desc;
int eg_attn_block_fwd(const eg_attn_block_desc* d, void* stream);
int eg_attn_block_ok(int S, int d_model, int num_heads, int dtype);   /* 1 when eg_attn_block_fwd serves this geometry */

/* ---------------------------------------------------------------------------------------------
 * eg_gemm_tn — weight-gradient product  dW[N,K] = sum_m dY[m,n] * X[m,k]  (fp32 result)
 *   replaces autograd's grad_weight of every Linear / Conv1d above.  Reads both operands row-major
 *   (rows = the reduction index) and transposes on the LDS read (ds_read_b64_tr_b16).  The reduction over
 *   M is split over `splits` workgroups; partial slabs [splits, slab] fp32 go to `partial` and
 *   eg_reduce_partials sums them (deterministic, no atomics).  With has_bias the column sums of dY (the bias
 *   gradient) are produced by the same launch; slab = (N/part_rows) * (part_rows*K + part_rows).
 * ------------------------------------------------------------------------------------------- */
typedef struct eg_gemm_tn_desc {
  const void* dY; /* [M, N] rows addressed by `y` */
  const void* X;  /* [M, K] rows addressed by `x` */
  float* partial; /* [splits, N, K] fp32 workspace */
  eg_rowmap y, x;
  int32_t M, N, K, splits;
  int32_t dtype;
  int64_t x_tile_stride; /* 0/128 = contiguous X rows; else elements between consecutive 128-column tiles */
  int32_t part_rows;     /* 0 = N.  One split's slab is N/part_rows parts of [part_rows x K | part_rows bias sums]: */
  int32_t has_bias;      /* the layout of consecutive (weight, bias) parameters, so ONE eg_reduce_partials writes both */
  int32_t tile;          /* 0 / 128: 128 x 128 tiles (256 threads); 256: 256 x 256 tiles (512 threads; 16-bit dtypes, N and K
                            multiples of 256, contiguous X rows): half the operand traffic per output, same partial slabs */
} eg_gemm_tn_desc;
int eg_gemm_tn(const eg_gemm_tn_desc* d, void* stream);
/* Grouped form: every weight-gradient product of the encoder in ONE launch (plain row-major operands, common
 * reduction length M, common split count).  `probs` is a DEVICE array; problem i owns blocks [blk0, blk0 + tiles*splits)
 * and writes its [splits, slab] partial slabs at `partial`.  eg_reduce_table sums many slab sets in one launch
 * (n and stride must be multiples of 4 floats). */
typedef struct eg_tn_problem {
  uint64_t dY, X, partial;
  int64_t ldy, ldx;
  int32_t N, K, part_rows, has_bias, blk0, _pad;
} eg_tn_problem;
/* entry i owns blocks [blk0, blk0 + nblk): nblk = ceil(n/4 / 256) when splits <= EG_REDUCE_WIDE_SPLITS (one float4 column
 * per thread, splits walked in order), else ceil(n/4 / 8) (8 float4 columns x 32 split lanes, for many short slabs) */
#define EG_REDUCE_WIDE_SPLITS 8
typedef struct eg_reduce_entry {
  uint64_t partial, out;
  int64_t n, stride;
  int32_t splits, blk0;
} eg_reduce_entry;
int eg_gemm_tn_grouped(const eg_tn_problem* probs, int nprob, int total_blocks, int M, int splits, int dtype, void* stream);
/* The same table served by 256 x 256 tiles (16-bit dtypes; every N and K a multiple of 256; blk0 counts
 * (N/256) * (K/256) * splits blocks per problem): half the operand traffic per output, bit-identical partial slabs. */
int eg_gemm_tn_grouped256(const eg_tn_problem* probs, int nprob, int total_blocks, int M, int splits, int dtype, void* stream);
int eg_reduce_table(const eg_reduce_entry* table, int nentries, int total_blocks, void* stream);
/* out[i] = (accumulate ? out[i] : 0) + sum_s partial[s*split_stride + i]; used for dW, db, LayerNorm dgamma/dbeta.  `partial` is
 * scratch: with splits >= 2048 over a short vector the sum runs in two stages and stage 1 overwrites rows of `partial`. */
int eg_reduce_partials(float* partial, float* out, int64_t n, int splits, int64_t split_stride, int accumulate,
                       void* stream);
/* conv weight gradient back to the parameter layout: dW[n][c][tap] = sum_s partial[s][n][tap*Cp + c] */
int eg_unpack_conv_wgrad(const float* partial, float* dW, int splits, int N, int Cin, int k, int Cp, int Kp,
                         void* stream);
/* column sums: out_partial[blk, n] = sum over the block's rows of Y[m, n]; rows addressed by `y` */
int eg_colsum(const void* Y, eg_rowmap y, int M, int N, float* partial, int nblk, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * LayerNorm(eps=1e-5) over the last dim  — A:283,286,293,295,306,328; D:952,968,972
 *   fwd: y = (x-mean)*rstd*gamma+beta, stats [M,2] = (mean, rstd)
 *   bwd: dx from dy; per-block partial dgamma/dbeta [nblk, 2, D] (sum with eg_reduce_partials); `partial` holds
 *        partial_capacity_blocks such rows and nblk beyond that is rejected on the host before any launch;
 *        optional dx_drop = dropout-masked dx (the gradient entering the branch whose output was dropped
 *        before the residual add: drop1/drop2 of A:293,295 and the FeedForward's own final dropout A:272)
 * ------------------------------------------------------------------------------------------- */
int eg_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* stats, int M, int D,
                     int dtype, void* stream);
int eg_layernorm_bwd(const void* dy, const void* x, const float* stats, const float* gamma, void* dx, void* dx_drop,
                     float* partial, int nblk, int partial_capacity_blocks, int M, int D, int dtype, float drop1_p,
                     uint32_t drop1_site, float drop2_p, uint32_t drop2_site, const eg_step_state* state, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-head attention core on a fused [NB*S, 3*D] q|k|v buffer — A:206-212; cross form D:967,971
 *   head h of sample b attends over the keys/values of sample (b + kv_shift) mod NB
 *   (kv_shift = 0: Siamese self-attention; kv_shift = NB/2: CrossBrainAttention, both directions at once).
 *   d_k must be 32.  lse [NB, H, S] = log-sum-exp of the scaled scores (for the backward recompute).
 *   attention-probability dropout (A:210) uses site `drop_site`.
 * ------------------------------------------------------------------------------------------- */
int eg_attention_fwd(const void* qkv, void* ctx, float* lse, int NB, int S, int H, int kv_shift, int dtype,
                     float drop_p, uint32_t drop_site, const eg_step_state* state, void* stream);
int eg_attention_bwd(const void* qkv, const void* ctx, const void* dctx, const float* lse, void* dqkv, int NB, int S,
                     int H, int kv_shift, int dtype, float drop_p, uint32_t drop_site, const eg_step_state* state,
                     void* stream);
/* probs[NB, H, S, S] (fp32) = softmax rows recomputed from qkv and the forward's lse: what a forward hook on the
 * attention-dropout module receives as input (5_Metrics/eeg_metrics.py:433-452).  Analysis only. */
int eg_attention_probs(const void* qkv, const float* lse, float* probs, int NB, int S, int H, int kv_shift, int dtype,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * Long-sequence attention core (1 <= S <= EG_ATTN_LONG_MAX_S): the contract of eg_attention_fwd / _bwd / _probs (same
 * layouts, same lse, same kv_shift pairing) with flash-style tiling; eg_attention_fwd and friends keep S <= 160.
 *   bwd: `scratch` holds at least NB*H*S floats (delta = rowsum(dctx * ctx) per window, head and query); deterministic,
 *        no atomics: two runs give bit-identical dqkv.
 *   dropout: element ((w*H + h)*S + q)*Sp2 + key (Sp2 = (S+1) & ~1) indexed in 64 bits; for indices below 2^32 the
 *        masks are those of eg_attention_fwd / _bwd.
 * ------------------------------------------------------------------------------------------- */
#define EG_ATTN_LONG_MAX_S 2048
int eg_attention_long_fwd(const void* qkv, void* ctx, float* lse, int NB, int S, int H, int kv_shift, int dtype,
                          float drop_p, uint32_t drop_site, const eg_step_state* state, void* stream);
int eg_attention_long_bwd(const void* qkv, const void* ctx, const void* dctx, const float* lse, void* dqkv, int NB, int S,
                          int H, int kv_shift, int dtype, float drop_p, uint32_t drop_site, const eg_step_state* state,
                          float* scratch, int64_t scratch_elems, void* stream);
int eg_attention_long_probs(const void* qkv, const float* lse, float* probs, int NB, int S, int H, int kv_shift, int dtype,
                            void* stream);

/* ---------------------------------------------------------------------------------------------
 * The long-sequence core with the head width as an argument: head_dim = d_model / num_heads is 32 or 64, anything else is
 * refused.  qkv [NB*S, 3*H*head_dim], ctx [NB*S, H*head_dim], lse [NB, H, S], scores scaled by 1/sqrt(head_dim); S, kv_shift,
 * scratch (NB*H*S floats), dropout indices and determinism as eg_attention_long_*.  head_dim = 32 launches exactly what
 * eg_attention_long_* launch; head_dim = 64 serves every S from 1 up (there is no 64-wide register-resident core).
 * ------------------------------------------------------------------------------------------- */
int eg_attention_dk_fwd(const void* qkv, void* ctx, float* lse, int NB, int S, int H, int head_dim, int kv_shift, int dtype,
                        float drop_p, uint32_t drop_site, const eg_step_state* state, void* stream);
int eg_attention_dk_bwd(const void* qkv, const void* ctx, const void* dctx, const float* lse, void* dqkv, int NB, int S, int H,
                        int head_dim, int kv_shift, int dtype, float drop_p, uint32_t drop_site, const eg_step_state* state,
                        float* scratch, int64_t scratch_elems, void* stream);
int eg_attention_dk_probs(const void* qkv, const float* lse, float* probs, int NB, int S, int H, int head_dim, int kv_shift,
                          int dtype, void* stream);

/* Statistics of the attention probabilities P[w,h,q,k] = exp(q.k/sqrt(head_dim) - lse[w,h,q]) of one attention stage, from the
 * stage's q|k|v rows and lse (layouts and kv_shift pairing of eg_attention_dk_*), without storing P.  NB is even; sample b < NB/2
 * owns windows b and b + NB/2 (stream 1 / stream 2 of a Siamese layer, the two directions of the cross stage).
 *   diag[b, q]     = 1/(2H) sum_h (P[b,h,q,q] + P[b+NB/2,h,q,q])                  written, [NB/2, S] fp32
 *   map_sum[q, k] += sum_b 1/(2H) sum_h (P[b,h,q,k] + P[b+NB/2,h,q,k])            read-modify-write, [S, S] fp32: zero it once,
 *                    issue every batch's call on one stream, read after the last (as eg_eval_accumulate's outputs)
 * head_dim 32 or 64, 1 <= S <= EG_ATTN_LONG_MAX_S, dtype bf16 / fp16 / f32.  scratch: at least
 * eg_attention_stats_scratch_elems(NB, S, H) floats, contents irrelevant on entry (0 floats: the tiles alone fill the GPU and
 * scratch may be NULL; -1: bad shape).  Deterministic, no atomics. */
int64_t eg_attention_stats_scratch_elems(int NB, int S, int H);            /* host only, no device needed */
int eg_attention_stats(const void* qkv, const float* lse, float* map_sum, float* diag, float* scratch, int64_t scratch_elems,
                       int NB, int S, int H, int head_dim, int kv_shift, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sequence assembly and heads (all [B, d]-sized, latency-bound single launches)
 *   eg_rows_bcast_f32  seq[b, off+r, :] = src[b % src_nb, r, :] + pos[off+r, :]   (cls_token expand + pos, D:1157,1178)
 *   eg_rows_copy       seq[b_dst0+b, off+r, :] = seq[b_src0+b, off+r, :]          (shared IBS tokens, D:1163-1165)
 *   eg_pool_fuse_fwd   cls slices, mean pools, symmetric-fusion operands          (D:1193-1212, D:933-938, D:1222-1223)
 *   eg_classifier_ce_* last Linear(K -> ncls<=16) fused with cross-entropy         (D:1104, D:1078, D:1244, D:1250)
 *   eg_batch_rowsum    out[s,:] = sum_b dseq[b,s,:]  (pos_embed / cls_token gradients)
 *   eg_rows_gather_gate dst rows = (src[b, off+r] (+ src[b+pair_shift, off+r])) * relu-gate * gate_scale
 * ------------------------------------------------------------------------------------------- */
int eg_rows_bcast_f32(const float* src, const float* pos, void* seq, int NB, int S, int D, int R, int off, int src_nb,
                      int dtype, void* stream);
int eg_rows_copy(void* seq, int S, int D, int R, int off, int b_src0, int b_dst0, int nb, int dtype, void* stream);
int eg_pool_fuse_fwd(const void* z, float* cls1, float* cls2, void* comb, void* zf, float* ibs_pool_f, void* ibs_pool,
                     int B, int S, int D, int off, int n_ibs, int ibs_first, int dtype, void* stream);
int eg_pool_fuse_bwd(const void* z, const void* dcomb, const void* dzf, const float* gcls1, const float* gcls2,
                     const void* dibs_pool, const float* gibs_pool, void* dz, int B, int S, int D, int off, int n_ibs,
                     int ibs_first, int dtype, void* stream);
int eg_classifier_ce_fwd(const void* h, const float* W, const float* bias, const int64_t* labels, float* logits,
                         float* sample_loss, float* loss, int B, int K, int ncls, int dtype, void* stream);
int eg_classifier_ce_bwd(const void* h, const float* W, const float* logits, const int64_t* labels, const float* gloss,
                         const float* glogits, float* dlogits, void* dh, float* dW, float* db, int B, int K, int ncls,
                         int use_gate, float gate_scale, int dtype, void* stream);
int eg_batch_rowsum(const void* dseq, float* out, int NB, int S, int D, int rows, int dtype, void* stream);
int eg_rows_gather_gate(const void* src, const void* gate, void* dst, eg_rowmap dmap, int nb, int S, int D, int R,
                        int off, int pair_shift, float gate_scale, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused forms of the launches above for the training step's tail (bf16 / fp16, d_model == 256).  Each gives the bits of the
 * launches it replaces: same MFMA shape and K order as eg_gemm_nt / eg_gemm_tn, same rounding points, same summation trees.
 *   eg_heads_fwd       after eg_pool_fuse_fwd: zf[:, :256] = comb Wsf^T + bsf; hcl = dropout(relu(zf Wc0^T + bc0)) (site
 *                      drop_site, the state's seed); logits = hcl W3^T + b3; with labels the per-sample CE and its mean.
 *                      Wsf / Wc0 [256, 768] in the compute dtype, W3 [ncls, 256] fp32.  Two launches, one per product, each
 *                      sliced over (16 samples, 64 output columns) workgroups.  `counter` is 1 + ceil(B / 16) zero-initialised
 *                      device words (always needed): word 1 + i finds the last workgroup of sample group i, which does that
 *                      group's class projection and CE, word 0 the last group, which takes the mean; all left at zero again.
 *   eg_classifier_ce_bwd_fused  eg_classifier_ce_bwd (rows and the last Linear's weight / bias gradient) in one launch; B <= 256
 *   eg_heads_bwd_chain dzf [B, 768] = dhcl c0T^T, dcomb [B, 768] = dzf[:, :256] sfT^T (c0T / sfT [768, 256]) and
 *                      dWc0 [256, 768] = dhcl^T zf, dbc0 = colsum(dhcl), summed in-launch; B <= 256.  Two launches, one per
 *                      product, sliced like eg_heads_fwd's; the weight-gradient tiles ride in the first
 *   eg_heads_bwd_pool  eg_pool_fuse_bwd plus dWsf [256, 768] = dzf[:, :256]^T comb, dbsf = colsum(dzf[:, :256]); B <= 256
 *   eg_token_grad_tail ONE pass over dseq [NB, S, D]: pos_grad[s, :] = sum_b dseq[b, s, :] (eg_batch_rowsum's order), cls_grad =
 *                      pos_grad row 0 (may be NULL), and eg_rows_gather_gate's rows dst[b, r, :] = dseq[b, off + r, :] gated by
 *                      gate[b, r, :] > 0.  D % 64 == 0.
 * ------------------------------------------------------------------------------------------- */
int eg_heads_fwd(const void* comb, void* zf, void* hcl, const void* Wsf, const float* bsf, const void* Wc0, const float* bc0,
                 const float* W3, const float* b3, const int64_t* labels, float* logits, float* sample_loss, float* loss,
                 uint32_t* counter, int B, int D, int ncls, float drop_p, uint32_t drop_site, const eg_step_state* state,
                 int dtype, void* stream);
int eg_classifier_ce_bwd_fused(const void* h, const float* W, const float* logits, const int64_t* labels, const float* gloss,
                               const float* glogits, float* dlogits, void* dh, float* dW, float* db, int B, int K, int ncls,
                               int use_gate, float gate_scale, int dtype, void* stream);
int eg_heads_bwd_chain(const void* dhcl, const void* c0T, const void* sfT, const void* zf, void* dzf, void* dcomb, float* dWc0,
                       float* dbc0, int B, int D, int dtype, void* stream);
int eg_heads_bwd_pool(const void* z, const void* dcomb, const void* dzf, const float* gcls1, const float* gcls2,
                      const void* dibs_pool, const float* gibs_pool, void* dz, const void* comb, float* dWsf, float* dbsf, int B,
                      int S, int D, int off, int n_ibs, int ibs_first, int dtype, void* stream);
int eg_token_grad_tail(const void* dseq, const void* gate, void* dst, eg_rowmap dmap, float* pos_grad, float* cls_grad, int NB,
                       int S, int D, int R, int off, float gate_scale, int dtype, void* stream);

/* eg_eval_accumulate — the per-batch tail of an evaluation loop (T:258-314) on the device, one launch of one workgroup:
 *   pred[b] = argmax_c logits[b][c] (lowest index on ties, as torch.argmax on finite values);
 *   confusion[labels[b]][pred[b]] += 1 (row-major [ncls][ncls]; NULL = no matrix; a label outside [0, ncls) counts nowhere);
 *   *loss_sum += *loss (either NULL = no sum).
 * confusion and loss_sum are read-modify-written with plain loads and stores: zero them once, then issue every batch's call on one
 * stream and read them after the last.  1 <= ncls <= 16, B > 0; a confusion matrix needs labels. */
int eg_eval_accumulate(const float* logits, const int64_t* labels, const float* loss, int32_t* pred, int32_t* confusion,
                       float* loss_sum, int B, int ncls, void* stream);

/* Batch-level auxiliary losses (3_Models/backbones/dual_eeg_transformer.py:1255-1371), fp32, each with the gradient of the
 * loss w.r.t. the [B, D] tokens it reads (upstream gradient 1; the caller scales).  B <= 1024.
 *   eg_aux_symmetry  F.mse_loss(cls1, cls2)                                                                    :1255-1260
 *   eg_aux_infonce   cross_entropy(normalize(ibs) normalize(cat[cls1, cls2])^T / temperature, arange(B))       :1262-1304
 *                    work: 3*B*D + 4*B + 2*B*B floats
 *   eg_aux_supcon    supervised contrastive loss over normalize(ibs) with the reference's 1e-8 guards, mean over the rows
 *                    that have a same-label partner, 0 (and zero gradient) if none has                          :1306-1371
 *                    work: B*D + 5*B + B*B + 4 floats */
int eg_aux_symmetry(const float* cls1, const float* cls2, float* loss, float* d_cls1, float* d_cls2, int B, int D, void* stream);
int eg_aux_infonce(const float* ibs, const float* cls1, const float* cls2, float temperature, float* loss, float* d_ibs,
                   float* d_cls1, float* d_cls2, float* work, int B, int D, void* stream);
int eg_aux_supcon(const float* ibs, const int64_t* labels, float temperature, float* loss, float* d_ibs, float* work, int B,
                  int D, void* stream);

/* FuzzyGatingFusion.forward — 3_Models/fusion/fuzzy_gating_fusion.py:297-390 (config 5's logit-level fusion).
 * params = [tau_img, tau_eeg, c_unreliable_img, c_unreliable_eeg, log_sigma_reliable_img, log_sigma_reliable_eeg,
 *           log_sigma_unreliable_img, log_sigma_unreliable_eeg, beta[4]] (12 device floats);
 * mode 0 full, 1 no_temperature, 2 no_fuzzification, 3 fixed_weights.
 * eg_fuzzy_gate_bwd: what autograd computes through that forward — dz_img, dz_eeg [B,K] and the 12 parameter gradients as
 *   per-workgroup partials partial[ceil(B/128)][12] (sum them in block order with eg_reduce_partials), from dfused [B,K] and
 *   dalpha [B] (or NULL).  torch.clamp semantics: the gradient passes where min <= x <= max. */
/* The loss of the multimodal logit-fusion step and its gradients on the [B, K] logits in one launch --
 * 4_Experiments/scripts/train_multimodal_fuzzy_fusion.py:436-460: total = CE(fused) + lambda_aux_img CE(z_img / T_img) +
 * lambda_aux_eeg CE(z_eeg / T_eeg) + lambda_reg R(T), temperatures detached in the auxiliary terms (fuzzy_gating_fusion.py:334),
 * R the temperature regulariser (:392-419).  losses[5] = total, ce, aux_img, aux_eeg, reg; dfused = d total / d fused (the upstream
 * gradient of eg_fuzzy_gate_bwd); daux_img / daux_eeg = the auxiliary terms' direct gradients on z_img / z_eeg; dtau[2] = the
 * regulariser's gradients on tau_img, tau_eeg.  Every gradient is multiplied by state->loss_scale when the scaler is on. */
int eg_fusion_loop_loss(const float* fused, const float* z_img, const float* z_eeg, const int64_t* labels, const float* params,
                        float* losses, float* dfused, float* daux_img, float* daux_eeg, float* dtau, int B, int K, int mode,
                        float eps_temp, float lambda_aux_img, float lambda_aux_eeg, float lambda_reg, float t_min, float t_max,
                        const eg_step_state* state, void* stream);
int eg_fuzzy_gate_fwd(const float* z_img, const float* z_eeg, const float* params, float* fused, float* alpha, int B,
                      int K, int mode, float eps_temp, float eps_log, float eps_div, void* stream);
int eg_fuzzy_gate_bwd(const float* z_img, const float* z_eeg, const float* params, const float* dfused, const float* dalpha,
                      float* dz_img, float* dz_eeg, float* partial, int B, int K, int mode, float eps_temp, float eps_log,
                      float eps_div, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Optimiser over flat fp32 buffers — clip_grad_norm_(1.0) + AdamW (T:221-222, T:401-405)
 *   eg_grad_sqnorm: partial[blk] = sum of squares;  eg_clip_coef: state->grad_norm / clip_coef (no host sync)
 *   eg_adamw: p *= 1-lr*wd; m,v update with g*grad_scale*clip_coef/loss_scale; p -= lr/bc1 * m/(sqrt(v)/sqrt(bc2)+eps);
 *             the whole step is skipped when state->scaler_on && state->found_inf (GradScaler.step)
 * ------------------------------------------------------------------------------------------- */
int eg_grad_sqnorm(const float* g, int64_t n, float* partial, int nblk, void* stream);
/* Gradient accumulation over micro-batches: acc[i] = first ? g[i] : acc[i] + g[i] for i < n, one fp32 addition per element
 * (bit-identical to torch.add; inf / NaN propagate, which is what lets one overflowing micro-batch skip the whole update).
 *   first != 0: acc is overwritten without being read (stale contents, NaN included, do not leak through).
 *   sq_partial != NULL: the same pass writes sq_partial[blk] = sum of acc_new[i]^2 for all nblk entries (blocks without
 *     elements write 0) -- eg_grad_sqnorm's contract, so eg_clip_coef(sq_partial, nblk, ...) consumes it unchanged.
 *   n is a positive multiple of 4 and both pointers are 16-B aligned (any bucket range of the flat buffers qualifies);
 *   1 <= nblk <= 1024 when sq_partial is given.  The grid is sized from the CU count, not from n. */
int eg_grad_accumulate(float* acc, const float* g, int64_t n, int first, float* sq_partial, int nblk, void* stream);
int eg_clip_coef(const float* partial, int nblk, float max_norm, eg_step_state* state, void* stream);
/* eg_grad_sqnorm + eg_clip_coef as ONE launch: the same nblk partials (also left in `partial`) and the same bits in
 * state->grad_norm / clip_coef / found_inf.  The workgroup that finishes last sums the partials; `counter` is one zeroed
 * uint32 in device memory that the launch leaves at zero again (one launch at a time per counter). */
int eg_grad_sqnorm_clip(const float* g, int64_t n, float* partial, int nblk, float max_norm, eg_step_state* state,
                        uint32_t* counter, void* stream);
int eg_adamw(float* p, const float* g, float* m, float* v, int64_t n, float beta1, float beta2, float eps,
             float weight_decay, const eg_step_state* state, void* stream);
int eg_fill_f32(float* p, int64_t n, float value, void* stream);
/* per-group form of eg_adamw for optimisers with parameter groups (train_multimodal_fuzzy_fusion.py:395-432: one learning
 * rate / weight decay per group): lr = state->lr * lr_mult. */
int eg_adamw_group(float* p, const float* g, float* m, float* v, int64_t n, float beta1, float beta2, float eps,
                   float weight_decay, float lr_mult, const eg_step_state* state, void* stream);
/* GradScaler.update() on the device (train_multimodal_fuzzy_fusion.py:471-472): after the optimiser kernels of a step.
 *   found_inf: loss_scale *= backoff, good_steps = 0, skipped += 1
 *   else:      opt_steps += 1, good_steps += 1; good_steps == growth_interval -> loss_scale *= growth, good_steps = 0
 * With scaler_on == 0 only opt_steps advances. */
int eg_scaler_update(eg_step_state* state, float growth, float backoff, int growth_interval, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Inter-stream synchrony ("IBS") features — D:473-819 (connectivity matrices), D:178-470 (scalar variant)
 *   eg_ibs_analytic: per signal x[T] (one window channel): rFFT, then for every band the FFT-mask band-pass
 *       (D:527-560) and FFT Hilbert transform (D:562-591) -> xb, phase [nbands, nsig, T]; stats [nbands, nsig, 4] =
 *       (mean, 1/(std_unbiased+1e-8)) of xb and of xb^2 (D:707-708, 751-752); spec [nsig, nbin] complex bins
 *   eg_ibs_pairs:  conn [B, nbands, 7, C, C] = [PLV, PLI, wPLI, Coherence, Power_Corr, Phase_Diff, Time_Corr]
 *       (D:593-758) for signals ordered [player1 windows | player2 windows] x C channels
 *   eg_ibs_scalar: feats [B, 7*nout_bands] global features of bands band0.. (D:436-461)
 *   eg_ibs_inorm:  token rows [B, nbands*nfeat, C*C] with InstanceNorm1d over the token axis (D:897-901)
 *   eg_gelu_fwd/bwd: GELU(erf)+dropout of the tokenizer bottleneck (D:865-866)
 * eg_stft_logmag — D:98-118: reflect-padded, hann-windowed n_fft-point DFT magnitudes, first F bins, log(.+1e-8)
 *   x [nsig, T] -> img [nsig, F, 1 + T/hop] fp32
 * ------------------------------------------------------------------------------------------- */
int eg_ibs_analytic(const float* x, float* xb, float* phase, float* stats, float* spec, int nsig, int T, float fs,
                    int nbin, const float* band_lo, const float* band_hi, int nbands, void* stream);
int eg_ibs_pairs(const float* xb, const float* phase, const float* stats, const float* spec, float* conn, int B, int C,
                 int T, float fs, int nbin, const float* band_lo, const float* band_hi, int nbands, void* stream);
int eg_ibs_scalar(const float* xb, const float* phase, const float* spec, float* feats, int B, int C, int T, float fs,
                  int nbin, const float* band_lo, const float* band_hi, int nbands, int band0, int nout_bands, int ld,
                  void* stream);
int eg_ibs_inorm(const float* conn, const int* fidx, const float* gamma, const float* beta, void* out, float* xhat, int B,
                 int nbands, int nfeat, int E, int use_norm, int dtype, void* stream);
/* eg_ibs_inorm for the analyses that run forward only.  zero_band in [-1, nbands): the nfeat tokens of that
 * band enter the instance norm as exact zeros (what a hook that zeroes conn[:, band] causes: the mean and variance of every
 * token move), -1: none.  xhat may be NULL: not stored.  zero_band = -1 with xhat gives eg_ibs_inorm's bits in out and xhat;
 * zero_band = b gives the bits of eg_ibs_inorm on a copy of conn whose band b is zero. */
int eg_ibs_inorm_band(const float* conn, const int* fidx, const float* gamma, const float* beta, void* out, float* xhat, int B,
                      int nbands, int nfeat, int E, int use_norm, int zero_band, int dtype, void* stream);
/* Per-class sums of the connectivity matrices of one batch (conn [B, nbands, 7, E] fp32 as eg_ibs_pairs writes it, fidx the
 * nfeat selected features, labels [B] int64):
 *   class_sum[c, band, f, e] += sum over b with labels[b] == c of conn[b, band, fidx[f], e]     [ncls, nbands, nfeat, E] fp32
 *   class_count[c]           += the number of such b                                            [ncls] int32
 * both read-modify-written: zero them once, issue every batch's call on one stream, read after the last (as eg_attention_stats'
 * map_sum).  A label outside [0, ncls) counts in no class (eg_eval_accumulate's rule); 1 <= ncls <= 16.  scratch: at least
 * eg_ibs_class_accumulate_scratch_elems(...) floats, contents irrelevant on entry (0: one split, scratch may be NULL; -1: bad
 * shape).  The launch shape and the scratch size follow from the shapes alone; samples are added in ascending order inside a
 * split and the splits in ascending order: deterministic, no atomics. */
int64_t eg_ibs_class_accumulate_scratch_elems(int B, int nbands, int nfeat, int E, int ncls);   /* host only, no device needed */
int eg_ibs_class_accumulate(const float* conn, const int* fidx, const int64_t* labels, float* class_sum, int32_t* class_count,
                            float* scratch, int64_t scratch_elems, int B, int nbands, int nfeat, int E, int ncls, void* stream);
/* InstanceNorm affine gradients: dgamma[e] = sum_m dy[m,e]*xhat[m,e], dbeta[e] = sum_m dy[m,e], as nsplit row-split
 * partials partial[sp][0][e] (gamma) | partial[sp][1][e] (beta); sum them in order with eg_reduce_partials */
int eg_affine_grad(const void* dy, const float* xhat, float* partial, int nsplit, int M, int E, int dtype, void* stream);
int eg_gelu_fwd(const void* u, void* h, int64_t n, int dtype, float drop_p, uint32_t drop_site, const eg_step_state* state,
                void* stream);
int eg_gelu_bwd(const void* u, const void* dh, void* du, int64_t n, int dtype, float drop_p, uint32_t drop_site,
                const eg_step_state* state, void* stream);
int eg_stft_logmag(const float* x, const float* window, float* img, int nsig, int T, int n_fft, int hop, int F,
                   void* stream);
/* band_lo / band_hi above are HOST arrays of nbands floats (<= 8 bands); every other pointer is a device pointer. */

/* ---------------------------------------------------------------------------------------------
 * 2-D CNN over the STFT image — D:70-77, 124-127.  Conv2d(1,32,3,p1)+ReLU+MaxPool2 is a direct kernel
 * (K = 9 is too shallow for MFMA); Conv2d(32,64,3,p1)+ReLU runs through eg_gemm_nt on segmented channel-last rows
 * (a_seg_len = 4*32); AdaptiveAvgPool2d(4,4) emits PyTorch's (c, py, px) flatten order.
 *   p1 [nimg, Hp+2, Wp+4, 32] zero-padded, out2 [nimg, Hp+2, Wp, 64], d2 [nimg, Hp+2, Wp+4, 64], dp1 [nimg, Hp+2, Wp, 32]
 *   eg_spec_conv1_bwd writes partial [nimg, 320] = (dW[32][9] | db[32]) for eg_reduce_partials
 *   eg_pack_conv2d_weight: dst[n][(ky*4+kx)*Cin + c] = w[n][c][ky][kx]; transposed: dst[c][(ky*4+kx)*N + n] = w[n][c][2-ky][2-kx]
 * ------------------------------------------------------------------------------------------- */
int eg_spec_conv1_fwd(const float* img, const float* w, const float* bias, void* p1, int nimg, int F, int nfr, int dtype,
                      void* stream);
int eg_spec_conv1_bwd(const float* img, const float* w, const float* bias, const void* dp1, float* partial, int nimg,
                      int F, int nfr, int dtype, void* stream);
/* eg_spec_conv1_fwd / _bwd stage one whole zero-padded image per workgroup: ((F+2)*(nfr+2) + 320) * 4 bytes of LDS forward, 10240
 * more backward.  A shape that needs more than 64 KiB is refused on the host before any launch; the banded entry points serve it:
 * a workgroup is (image, band of band_rows pooled rows) and stages the 2*band_rows + 2 input rows of its band
 * (((2*band_rows+2)*(nfr+2) + 320) * 4 bytes forward, 10240 more backward, at most 64 KiB).  Same operator, layouts and per-output
 * multiply-add chain: the interior of p1 is eg_spec_conv1_fwd's bit for bit (the pad frame is not written), and
 *   eg_spec_conv1_bwd_banded writes partial [nimg * nbands, 320], nbands = ceil(Hp / band_rows), row im*nbands + band =
 *   the band's (dW[32][9] | db[32]), every row whole by one workgroup (no atomics; sum with eg_reduce_partials over nimg*nbands).
 * band_rows: any value in [1, Hp] whose LDS fits.  eg_spec_conv1_band_rows(F, nfr) is the production choice, a function of the
 * shape alone: 0 = the whole-image backward fits 64 KiB, use eg_spec_conv1_fwd / _bwd (every shape up to e.g. 64 x 17, 72 x 120);
 * else 16, or 8 where 16 rows do not fit (nfr > 395); -1 = no band fits (nfr > 748).  224 x 224: 16 (7 bands), 512 x 512: 8 (32). */
int eg_spec_conv1_band_rows(int F, int nfr);      /* host only, no device needed */
int eg_spec_conv1_fwd_banded(const float* img, const float* w, const float* bias, void* p1, int nimg, int F, int nfr,
                             int band_rows, int dtype, void* stream);
int eg_spec_conv1_bwd_banded(const float* img, const float* w, const float* bias, const void* dp1, float* partial, int nimg,
                             int F, int nfr, int band_rows, int dtype, void* stream);
int eg_spec_avgpool_fwd(const void* out2, void* pooled, int nimg, int Hp, int Wp, int dtype, void* stream);
int eg_spec_avgpool_bwd(const void* out2, const void* dpooled, void* d2, int nimg, int Hp, int Wp, int dtype, void* stream);
int eg_pack_conv2d_weight(const float* w, void* dst, int N, int Cin, int transposed, int dtype, void* stream);
int eg_unpack_conv2d_wgrad(float* partial /* scratch: reduced in place when splits > 64 */, float* dW, int splits, int N, int Cin, void* stream);
/* Weight gradient of Conv2d(32,64,3,p1) (autograd's grad_weight of D:74) as a flat correlation over the padded pixel index q
 * (16-bit operands): partial[split][n][(ky*4+kx)*32 + c] = sum over the split's q of d2[q + rowpx + 1][n] * p1[q + ky*rowpx + kx][c],
 * Q = nimg*(Hp+2)*rowpx pixels, rowpx = Wp + 4.  The pads of d2 must be zero (eg_spec_avgpool_bwd writes interiors only); p1 must hold
 * p1_rows >= Q + 2*rowpx + 2 readable pixel rows.  The slabs are the ones eg_unpack_conv2d_wgrad reduces (pad taps kx = 3 are not
 * written).  bias_partial (optional): per split the column sums of the gradient rows = autograd's grad_bias, for eg_reduce_partials.
 * eg_conv2d_wgrad_flat_splits: the largest split count <= want whose 256-pixel-aligned splits all own pixels. */
int eg_conv2d_wgrad_flat(const void* d2, const void* p1, float* partial, float* bias_partial /* [splits][64] or NULL */, long long Q,
                         long long p1_rows, int rowpx, int splits, int dtype, void* stream);
int eg_conv2d_wgrad_flat_splits(long long Q, int want);
/* Conv2d(32,64,3,p1) forward (D:74, + the ReLU of D:75 when act = EG_ACT_RELU; cin 32, nout 64, W = eg_pack_conv2d_weight(transposed 0))
 * and its backward-data (autograd's grad_input: in = d2, cin 64, nout 32, W = the transposed packing, out = dp1) on the same flat
 * pixel index, 16-bit operands:
 *   out[g*Wp + x][n] = act(bias[n] + sum_{ky,kx,c} in[q + ky*rowpx + kx][c] * W[n][(ky*4+kx)*cin + c]), q = g*rowpx + x, x < Wp,
 * for all Q = nimg*(Hp+2)*rowpx pixel slots; `in` must hold in_rows >= Q + 2*rowpx + 2 readable pixel rows; `splits` = workgroups wanted. */
int eg_conv2d_flat(const void* in, const void* W, const float* bias, void* out, long long Q, long long in_rows, int rowpx, int Wp,
                   int cin, int nout, int act, int splits, int dtype, void* stream);
/* Grad-CAM of Conv2d(32,64,3,p1) (eeg_metrics.py:775-793, 897-937) from p1 [2*B*C][Hp+2][Wp+4][32] and
 * d2 [2*B*C][Hp+2][Wp+4][64] (the padded channel-last layouts of eg_spec_conv1_fwd / eg_spec_avgpool_bwd, compute dtype; images
 * [0, B*C) are stream 1, the rest stream 2), w2 [64][32][3][3] and b2 [64] (fp32, torch layout), labels [B] int64:
 *   wgt[n][c] = mean over the Hp x Wp interior of d2[n][..][c] (/ *grad_scale when grad_scale is not NULL: one device float)
 *   cam_n     = relu(sum_c wgt[n][c] * (b2[c] + conv3x3(p1[n], w2[c])))  -- as ONE convolution with the filter sum_c wgt[n][c] w2[c]
 *   cam_b     = (mean over C of stream 1's cam_n + mean over C of stream 2's) / 2, resized to 64 x 64 as
 *               F.interpolate(mode="bilinear", align_corners=False) does
 *   cams[b] = cam_b                                  [B, 64, 64] fp32, written
 *   class_sum[labels[b]] += cam_b, class_count[labels[b]] += 1      [ncls, 64, 64] fp32 / [ncls] int32, read-modify-written (zero
 *               them once, issue every batch's call on one stream); a label outside [0, ncls) counts in no class, its cams row
 *               is still written; 1 <= ncls <= 16.
 * Hp, Wp: positive multiples of 4, Hp * Wp <= 4096.  scratch: at least eg_gradcam_scratch_elems(...) floats (the channel means of
 * both streams, [2][B][Hp][Wp]), contents irrelevant on entry (-1: bad shape).  Two launches; samples are added in ascending
 * order: deterministic, no float atomics. */
int64_t eg_gradcam_scratch_elems(int B, int C, int Hp, int Wp);   /* host only, no device needed */
int eg_gradcam_accumulate(const void* p1, const void* d2, const float* w2, const float* b2, const float* grad_scale,
                          const int64_t* labels, float* cams, float* class_sum, int32_t* class_count, float* scratch,
                          int64_t scratch_elems, int B, int C, int Hp, int Wp, int ncls, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EYEGAZE_HIP_H */
