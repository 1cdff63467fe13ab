"""ctypes binding of libeyegaze_hip.so (C ABI declared in include/eyegaze_hip.h).

The library is mandatory: importing this module without it raises.  There is NO CPU fallback anywhere in
the package — the product path is the HIP path or nothing.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "libeyegaze_hip.so"

EG_F32, EG_BF16, EG_F16 = 0, 1, 2
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
ABI_VERSION = 5
GEMM_BATCH_MAX = 8      # EG_GEMM_BATCH_MAX


class EgError(RuntimeError):
    pass


class RowMap(C.Structure):
    _fields_ = [("row_stride", C.c_int64), ("group_stride", C.c_int64), ("rows_per_group", C.c_int32), ("_pad", C.c_int32)]


def rowmap(row_stride: int, group_stride: int = 0, rows_per_group: int = 0) -> RowMap:
    return RowMap(int(row_stride), int(group_stride), int(rows_per_group), 0)


class StepState(C.Structure):
    _fields_ = [("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("lr", C.c_float), ("bias_corr1", C.c_float),
                ("bias_corr2", C.c_float), ("grad_scale", C.c_float), ("clip_coef", C.c_float), ("grad_norm", C.c_float),
                ("loss_scale", C.c_float), ("found_inf", C.c_uint32), ("good_steps", C.c_uint32), ("opt_steps", C.c_uint32),
                ("use_dev_t", C.c_uint32), ("skipped", C.c_uint32), ("scaler_on", C.c_uint32), ("_pad", C.c_uint32)]


STATE_WORDS = C.sizeof(StepState) // 4   # 16


class GemmDesc(C.Structure):
    _fields_ = [("A", C.c_void_p), ("W", C.c_void_p), ("C", C.c_void_p), ("bias", C.c_void_p), ("residual", C.c_void_p),
                ("gate", C.c_void_p), ("out_pre", C.c_void_p), ("state", C.c_void_p),
                ("a", RowMap), ("c", RowMap), ("r", RowMap), ("p", RowMap),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("ldw", C.c_int32),
                ("act", C.c_int32), ("dtype", C.c_int32),
                ("drop1_p", C.c_float), ("drop2_p", C.c_float), ("drop1_site", C.c_uint32), ("drop2_site", C.c_uint32),
                ("gate_scale", C.c_float), ("a_seg_len", C.c_int32), ("a_seg_stride", C.c_int64)]


class FfnDesc(C.Structure):
    _fields_ = [("A", C.c_void_p), ("W1", C.c_void_p), ("W2", C.c_void_p), ("H", C.c_void_p), ("C", C.c_void_p),
                ("bias1", C.c_void_p), ("bias2", C.c_void_p), ("gate", C.c_void_p), ("gate_bits_out", C.c_void_p),
                ("gate_bits_in", C.c_void_p), ("residual", C.c_void_p),
                ("state", C.c_void_p),
                ("lda", C.c_int64), ("ldh", C.c_int64), ("ldc", C.c_int64), ("ldg", C.c_int64), ("ldr", C.c_int64),
                ("M", C.c_int32), ("F", C.c_int32), ("act1", C.c_int32), ("dtype", C.c_int32),
                ("drop_h_p", C.c_float), ("drop_c1_p", C.c_float), ("drop_c2_p", C.c_float),
                ("drop_h_site", C.c_uint32), ("drop_c1_site", C.c_uint32), ("drop_c2_site", C.c_uint32),
                ("gate_scale", C.c_float),
                ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p), ("ln_out", C.c_void_p), ("ln_stats", C.c_void_p)]


class LnBwdProjDesc(C.Structure):
    _fields_ = [("dy", C.c_void_p), ("x", C.c_void_p), ("stats", C.c_void_p), ("gamma", C.c_void_p), ("W_frag", C.c_void_p),
                ("dx", C.c_void_p), ("dx_drop", C.c_void_p), ("dC", C.c_void_p), ("partial", C.c_void_p), ("state", C.c_void_p),
                ("M", C.c_int32), ("d_model", C.c_int32), ("dtype", C.c_int32), ("partial_capacity_blocks", C.c_int32),
                ("drop1_p", C.c_float), ("drop2_p", C.c_float), ("drop1_site", C.c_uint32), ("drop2_site", C.c_uint32)]


class AttnBlockDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("wqkv_frag", C.c_void_p), ("wo_frag", C.c_void_p), ("bqkv", C.c_void_p), ("bo", C.c_void_p),
                ("qkv", C.c_void_p), ("ctx", C.c_void_p), ("lse", C.c_void_p), ("r1", C.c_void_p), ("state", C.c_void_p),
                ("NB", C.c_int32), ("S", C.c_int32), ("d_model", C.c_int32), ("num_heads", C.c_int32), ("dtype", C.c_int32),
                ("attn_drop_p", C.c_float), ("out_drop_p", C.c_float), ("attn_drop_site", C.c_uint32), ("out_drop_site", C.c_uint32),
                ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p), ("ln_out", C.c_void_p), ("ln_stats", C.c_void_p)]


class WindowGatherDesc(C.Structure):
    _fields_ = [("data", C.c_void_p), ("pair_off", C.c_void_p), ("pair_len", C.c_void_p), ("win_pair", C.c_void_p),
                ("win_start", C.c_void_p), ("win_label", C.c_void_p),
                ("n_pairs", C.c_int32), ("n_windows", C.c_int32), ("C", C.c_int32), ("T", C.c_int32)]


class RecordingRowsDesc(C.Structure):
    _fields_ = [("data", C.c_void_p), ("row_off", C.c_void_p), ("row_len", C.c_void_p), ("ws_off", C.c_void_p),
                ("n_rows", C.c_int32), ("C", C.c_int32), ("max_len", C.c_int32), ("_pad", C.c_int32)]


class ImageBatchDesc(C.Structure):
    _fields_ = [("data", C.c_void_p), ("off", C.c_void_p), ("npix", C.c_void_p), ("layout", C.c_void_p),
                ("n_images", C.c_int32), ("max_pix", C.c_int32), ("elem", C.c_int32), ("normalize", C.c_int32)]


IMAGE_ENTROPY_CHUNK = 8192      # EG_IMAGE_ENTROPY_CHUNK


class GazeResizeDesc(C.Structure):
    _fields_ = [("data", C.c_void_p), ("off", C.c_void_p), ("h", C.c_void_p), ("w", C.c_void_p), ("mid_off", C.c_void_p),
                ("tabs", C.c_void_p), ("htab", C.c_void_p), ("vtab", C.c_void_p), ("sum_h", C.c_int64),
                ("n_images", C.c_int32), ("max_h", C.c_int32), ("F", C.c_int32), ("W", C.c_int32)]


GAZE_MAX_SIDE, GAZE_MIN_OUT, GAZE_MAX_OUT = 4096, 8, 512      # EG_GAZE_MAX_SIDE, EG_GAZE_MIN_OUT, EG_GAZE_MAX_OUT
TSNE_MAX_N, TSNE_MAX_D = 16384, 4096                          # EG_TSNE_MAX_N, EG_TSNE_MAX_D
GAZE_PAIR_FIELDS, ROW_COSINE_MAX_D = 14, 4096                 # EG_GAZE_PAIR_FIELDS, EG_ROW_COSINE_MAX_D


class PackEntry(C.Structure):
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("rows", C.c_int32), ("cols", C.c_int32), ("ldd", C.c_int32),
                ("mode", C.c_int32), ("blk0", C.c_int32), ("nblk", C.c_int32)]


class PackEntryEx(C.Structure):
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("rows", C.c_int32), ("cols", C.c_int32), ("ldd", C.c_int32),
                ("mode", C.c_int32), ("blk0", C.c_int32), ("nblk", C.c_int32), ("p0", C.c_int32), ("p1", C.c_int32),
                ("p2", C.c_int32), ("p3", C.c_int32), ("src_elems", C.c_int64), ("dst_elems", C.c_int64)]


class TNProblem(C.Structure):
    _fields_ = [("dY", C.c_uint64), ("X", C.c_uint64), ("partial", C.c_uint64), ("ldy", C.c_int64), ("ldx", C.c_int64),
                ("N", C.c_int32), ("K", C.c_int32), ("part_rows", C.c_int32), ("has_bias", C.c_int32), ("blk0", C.c_int32),
                ("_pad", C.c_int32)]


class ReduceEntry(C.Structure):
    _fields_ = [("partial", C.c_uint64), ("out", C.c_uint64), ("n", C.c_int64), ("stride", C.c_int64),
                ("splits", C.c_int32), ("blk0", C.c_int32)]


class GemmTNDesc(C.Structure):
    _fields_ = [("dY", C.c_void_p), ("X", C.c_void_p), ("partial", C.c_void_p), ("y", RowMap), ("x", RowMap),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("splits", C.c_int32), ("dtype", C.c_int32),
                ("x_tile_stride", C.c_int64), ("part_rows", C.c_int32), ("has_bias", C.c_int32), ("tile", C.c_int32)]


_P, _I, _L, _F, _U = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_uint32

# name -> argtypes; every function returns int (0 = ok).  Mirrors include/eyegaze_hip.h exactly.
SIGNATURES = {
    "eg_device_info": [C.POINTER(C.c_int), C.c_char_p, _I],
    "eg_window_pack": [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "eg_pack_table": [_P, _I, _I, _I, _P],
    "eg_pack_table_ex_check": [_P, _I, _I, C.POINTER(C.c_int)],
    "eg_pack_table_ex": [_P, _I, _I, _I, _P],
    "eg_cast": [_P, _P, _L, _I, _P],
    "eg_transpose_cast": [_P, _P, _I, _I, _I, _I, _P],
    "eg_pack_conv_weight": [_P, _P, _I, _I, _I, _I, _I, _I, _P],
    "eg_pack_convT_weight": [_P, _P, _I, _I, _I, _I, _I, _P],
    "eg_gemm_nt": [C.POINTER(GemmDesc), _P],
    "eg_gemm_nt_route": [C.POINTER(GemmDesc)],
    "eg_gemm_wide_rows": [_I, _I],
    "eg_gemm_wide_config": [_I, _I],
    "eg_gemm_nt_batch": [C.POINTER(GemmDesc), _I, _P],
    "eg_gemm_nt_batch_route": [C.POINTER(GemmDesc), _I],
    "eg_ffn_chain": [C.POINTER(FfnDesc), _P],
    "eg_ln_bwd_proj": [C.POINTER(LnBwdProjDesc), _P],
    "eg_ln_bwd_proj_blocks": [_I],
    "eg_ffn_bwd_ln_proj": [C.POINTER(FfnDesc), C.POINTER(LnBwdProjDesc), _P],
    "eg_attn_block_fwd": [C.POINTER(AttnBlockDesc), _P],
    "eg_attn_block_ok": [_I, _I, _I, _I],
    "eg_gemm_tn": [C.POINTER(GemmTNDesc), _P],
    "eg_reduce_partials": [_P, _P, _L, _I, _L, _I, _P],
    "eg_gemm_tn_grouped": [_P, _I, _I, _I, _I, _I, _P],
    "eg_gemm_tn_grouped256": [_P, _I, _I, _I, _I, _I, _P],
    "eg_reduce_table": [_P, _I, _I, _P],
    "eg_unpack_conv_wgrad": [_P, _P, _I, _I, _I, _I, _I, _I, _P],
    "eg_colsum": [_P, RowMap, _I, _I, _P, _I, _I, _P],
    "eg_layernorm_fwd": [_P, _P, _P, _P, _P, _I, _I, _I, _P],
    "eg_layernorm_bwd": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _U, _F, _U, _P, _P],
    "eg_attention_fwd": [_P, _P, _P, _I, _I, _I, _I, _I, _F, _U, _P, _P],
    "eg_attention_bwd": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _U, _P, _P],
    "eg_window_normalize": [_P, _P, _P, _I, _I, _I, _I, _P],
    "eg_window_gather": [C.POINTER(WindowGatherDesc), _P, _I, _I, _I, _P, _P, _P, _I, _P],
    "eg_window_cut": [C.POINTER(WindowGatherDesc), _P, _I, _I, _I, _P, _P, _P, _P],
    "eg_recording_filtfilt": [C.POINTER(RecordingRowsDesc), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), _I,
                              _P, _L, _L, _P],
    "eg_recording_filtfilt_exact": [C.POINTER(RecordingRowsDesc), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                    _I, _P, _L, _L, _P],
    "eg_recording_car_zscore": [C.POINTER(RecordingRowsDesc), _P],
    "eg_recording_car": [C.POINTER(RecordingRowsDesc), _P],
    "eg_trial_welch": [C.POINTER(RecordingRowsDesc), C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, _P, _P, _P, _P],
    "eg_trial_analytic_twiddle_doubles": [_I],                       # returns int64_t: trial_analytic_twiddle_doubles() below
    "eg_trial_analytic_tables": [C.POINTER(RecordingRowsDesc), _P, _P, _L, _L, _P],
    "eg_trial_analytic": [C.POINTER(RecordingRowsDesc), _P, _P, _P, _P, _P, _L, _L, _P],
    "eg_trial_pairs_workspace_floats": [_I, _I, _I],                 # returns int64_t: trial_pairs_workspace_floats() below
    "eg_trial_pairs": [C.POINTER(RecordingRowsDesc), _P, _P, _P, _P, _L, _P, _I, _I, _P],
    "eg_trial_coherence_workspace_floats": [_I, _I],                 # returns int64_t: trial_coherence_workspace_floats() below
    "eg_trial_coherence": [C.POINTER(RecordingRowsDesc), _P, _L, _P, _I, _I, _P],
    "eg_trial_spectral_entropy": [C.POINTER(RecordingRowsDesc), C.c_double, C.c_double, _P, _P, _P],
    "eg_image_entropy_workspace_doubles": [_I, _I],                  # returns int64_t: image_entropy_workspace_doubles() below
    "eg_image_entropy": [C.POINTER(ImageBatchDesc), C.c_double, _P, _L, _P, _P],
    "eg_tsne_workspace_bytes": [_I],                                 # returns int64_t: tsne_workspace_bytes() below
    "eg_tsne_sqdist": [_P, _I, _I, _P, _P],
    "eg_tsne_affinities": [_P, _I, C.c_double, _P, _P, _P, _P],
    "eg_tsne_joint": [_P, _I, _P, _L, _P, _P],
    "eg_tsne_gradient": [_P, _P, C.c_double, _I, _P, _L, _P, _P, _P],
    "eg_tsne_update": [_P, _P, _P, _P, _I, _F, _F, _F, _P, _P],
    "eg_gaze_resize_workspace_bytes": [_I, _L, _I],                  # returns int64_t: gaze_resize_workspace_bytes() below
    "eg_gaze_resize": [C.POINTER(GazeResizeDesc), _P, _L, _P, _P],
    "eg_gaze_batch": [_P, _I, _I, _I, _P, _P, _P, _I, _I, _I, _P, _U, _U, _F, _F, _F, _P, _P, _P, _P, _P, _P],
    "eg_gaze_pair_stats_workspace_bytes": [_I],                      # returns int64_t: gaze_pair_stats_workspace_bytes() below
    "eg_gaze_pair_stats": [_P, _I, _I, _I, _P, _I, _P, _F, _P, _L, _P, _P],
    "eg_row_cosine": [_P, _P, _I, _I, _P, _P],
    "eg_window_augment": [_P, _P, _P, _P, _I, _I, _I, _F, _F, _I, _I, _P, _P],
    "eg_attention_probs": [_P, _P, _P, _I, _I, _I, _I, _I, _P],
    "eg_attention_long_fwd": [_P, _P, _P, _I, _I, _I, _I, _I, _F, _U, _P, _P],
    "eg_attention_long_bwd": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _U, _P, _P, _L, _P],
    "eg_attention_long_probs": [_P, _P, _P, _I, _I, _I, _I, _I, _P],
    "eg_attention_dk_fwd": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _U, _P, _P],
    "eg_attention_dk_bwd": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _U, _P, _P, _L, _P],
    "eg_attention_dk_probs": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "eg_attention_stats_scratch_elems": [_I, _I, _I],          # returns int64_t: attn_stats_scratch_elems() below
    "eg_attention_stats": [_P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _P],
    "eg_rows_bcast_f32": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "eg_rows_copy": [_P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "eg_pool_fuse_fwd": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "eg_pool_fuse_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "eg_classifier_ce_fwd": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "eg_classifier_ce_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _I, _P],
    "eg_batch_rowsum": [_P, _P, _I, _I, _I, _I, _I, _P],
    "eg_rows_gather_gate": [_P, _P, _P, RowMap, _I, _I, _I, _I, _I, _I, _F, _I, _P],
    "eg_heads_fwd": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _U, _P, _I, _P],
    "eg_classifier_ce_bwd_fused": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _I, _P],
    "eg_heads_bwd_chain": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "eg_heads_bwd_pool": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "eg_token_grad_tail": [_P, _P, _P, RowMap, _P, _P, _I, _I, _I, _I, _I, _F, _I, _P],
    "eg_eval_accumulate": [_P, _P, _P, _P, _P, _P, _I, _I, _P],
    "eg_grad_sqnorm": [_P, _L, _P, _I, _P],
    "eg_grad_accumulate": [_P, _P, _L, _I, _P, _I, _P],
    "eg_clip_coef": [_P, _I, _F, _P, _P],
    "eg_grad_sqnorm_clip": [_P, _L, _P, _I, _F, _P, _P, _P],
    "eg_adamw": [_P, _P, _P, _P, _L, _F, _F, _F, _F, _P, _P],
    "eg_fill_f32": [_P, _L, _F, _P],
    "eg_adamw_group": [_P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _P, _P],
    "eg_set_step_state": [_P, _U, _U, _F, _F, _F, _F, _I, _F, _I, _P],
    "eg_scaler_update": [_P, _F, _F, _I, _P],
    "eg_aux_symmetry": [_P, _P, _P, _P, _P, _I, _I, _P],
    "eg_aux_infonce": [_P, _P, _P, _F, _P, _P, _P, _P, _P, _I, _I, _P],
    "eg_aux_supcon": [_P, _P, _F, _P, _P, _P, _I, _I, _P],
    "eg_fuzzy_gate_fwd": [_P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _F, _P],
    "eg_fusion_loop_loss": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _F, _F, _F, _F, _P, _P],
    "eg_fuzzy_gate_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _F, _P],
    "eg_ibs_analytic": [_P, _P, _P, _P, _P, _I, _I, _F, _I, _P, _P, _I, _P],
    "eg_ibs_pairs": [_P, _P, _P, _P, _P, _I, _I, _I, _F, _I, _P, _P, _I, _P],
    "eg_ibs_scalar": [_P, _P, _P, _P, _I, _I, _I, _F, _I, _P, _P, _I, _I, _I, _I, _P],
    "eg_affine_grad": [_P, _P, _P, _I, _I, _I, _I, _P],
    "eg_ibs_inorm": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "eg_ibs_inorm_band": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "eg_ibs_class_accumulate_scratch_elems": [_I, _I, _I, _I, _I],   # returns int64_t: ibs_class_scratch_elems() below
    "eg_ibs_class_accumulate": [_P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _P],
    "eg_gelu_fwd": [_P, _P, _L, _I, _F, _U, _P, _P],
    "eg_gelu_bwd": [_P, _P, _P, _L, _I, _F, _U, _P, _P],
    "eg_stft_logmag": [_P, _P, _P, _I, _I, _I, _I, _I, _P],
    "eg_spec_conv1_fwd": [_P, _P, _P, _P, _I, _I, _I, _I, _P],
    "eg_spec_conv1_bwd": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "eg_spec_conv1_band_rows": [_I, _I],                             # returns the band height itself: spec_conv1_band_rows() below
    "eg_spec_conv1_fwd_banded": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "eg_spec_conv1_bwd_banded": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "eg_spec_avgpool_fwd": [_P, _P, _I, _I, _I, _I, _P],
    "eg_spec_avgpool_bwd": [_P, _P, _P, _I, _I, _I, _I, _P],
    "eg_pack_conv2d_weight": [_P, _P, _I, _I, _I, _I, _P],
    "eg_unpack_conv2d_wgrad": [_P, _P, _I, _I, _I, _P],
    "eg_conv2d_wgrad_flat": [_P, _P, _P, _P, _L, _L, _I, _I, _I, _P],
    "eg_conv2d_wgrad_flat_splits": [_L, _I],
    "eg_conv2d_flat": [_P, _P, _P, _P, _L, _L, _I, _I, _I, _I, _I, _I, _I, _P],
    "eg_gradcam_scratch_elems": [_I, _I, _I, _I],                    # returns int64_t: gradcam_scratch_elems() below
    "eg_gradcam_accumulate": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _P],
}
_lib = None


def lib() -> C.CDLL:
    """Loads the library once; raises EgError when it is missing or its ABI differs (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise EgError(f"{LIB_PATH} is missing: build it with `python -m eyegaze_multimodal_amd.build` "
                      "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    l = C.CDLL(str(LIB_PATH))
    l.eg_abi_version.restype = C.c_int
    if l.eg_abi_version() != ABI_VERSION:
        raise EgError(f"ABI mismatch: library {l.eg_abi_version()} vs binding {ABI_VERSION}")
    l.eg_last_error.restype = C.c_char_p
    for name, args in SIGNATURES.items():
        fn = getattr(l, name, None)
        if fn is None:
            continue  # optional (not yet built) entry points are reported by exported_symbols()
        fn.argtypes = args
        fn.restype = C.c_int
    _lib = l
    return l


def gate_bits_bytes(M: int, F: int) -> int:
    """Size of the gate bit image eg_ffn_chain writes / reads for an [M, F] hidden tensor (eg_ffn_gate_bits_bytes)."""
    l = lib()
    l.eg_ffn_gate_bits_bytes.restype = C.c_int64
    l.eg_ffn_gate_bits_bytes.argtypes = [C.c_int, C.c_int]
    return int(l.eg_ffn_gate_bits_bytes(M, F))


def attn_stats_scratch_elems(NB: int, S: int, H: int) -> int:
    """Floats of scratch eg_attention_stats needs for this shape (host only; 0: none, -1: bad shape)"""
    l = lib()
    l.eg_attention_stats_scratch_elems.restype = C.c_int64
    return int(l.eg_attention_stats_scratch_elems(NB, S, H))


def ibs_class_scratch_elems(B: int, nbands: int, nfeat: int, E: int, ncls: int) -> int:
    """Floats of scratch eg_ibs_class_accumulate needs for this shape (host only; 0: none, -1: bad shape)"""
    l = lib()
    l.eg_ibs_class_accumulate_scratch_elems.restype = C.c_int64
    return int(l.eg_ibs_class_accumulate_scratch_elems(B, nbands, nfeat, E, ncls))


def gradcam_scratch_elems(B: int, Cn: int, Hp: int, Wp: int) -> int:
    """Floats of scratch eg_gradcam_accumulate needs for B samples of Cn channels (host only; -1: bad shape)"""
    l = lib()
    l.eg_gradcam_scratch_elems.restype = C.c_int64
    return int(l.eg_gradcam_scratch_elems(B, Cn, Hp, Wp))


def trial_analytic_twiddle_doubles(max_len: int) -> int:
    """Doubles at the head of eg_trial_analytic's workspace: the twiddle table for rows up to max_len (host only; -1: bad length)"""
    l = lib()
    l.eg_trial_analytic_twiddle_doubles.restype = C.c_int64
    return int(l.eg_trial_analytic_twiddle_doubles(max_len))


def trial_pairs_workspace_floats(n_rows: int, Cn: int, max_len: int) -> int:
    """Floats of workspace eg_trial_pairs needs (host only; -1: bad shape)"""
    l = lib()
    l.eg_trial_pairs_workspace_floats.restype = C.c_int64
    return int(l.eg_trial_pairs_workspace_floats(n_rows, Cn, max_len))


def trial_coherence_workspace_floats(n_rows: int, max_len: int) -> int:
    """Floats of workspace eg_trial_coherence needs (host only; -1: bad shape)"""
    l = lib()
    l.eg_trial_coherence_workspace_floats.restype = C.c_int64
    return int(l.eg_trial_coherence_workspace_floats(n_rows, max_len))


def image_entropy_workspace_doubles(n_images: int, max_pix: int) -> int:
    """Doubles of workspace eg_image_entropy needs (host only; -1: bad shape)"""
    l = lib()
    l.eg_image_entropy_workspace_doubles.restype = C.c_int64
    return int(l.eg_image_entropy_workspace_doubles(n_images, max_pix))


def gaze_resize_workspace_bytes(n_images: int, sum_h: int, W: int) -> int:
    """Bytes of workspace eg_gaze_resize needs for n_images images of sum_h rows in all (host only; -1: bad shape)"""
    l = lib()
    l.eg_gaze_resize_workspace_bytes.restype = C.c_int64
    return int(l.eg_gaze_resize_workspace_bytes(n_images, sum_h, W))


def gaze_pair_stats_workspace_bytes(n_images: int) -> int:
    """Bytes of workspace eg_gaze_pair_stats needs for a store of n_images (host only; -1: n_images <= 0)"""
    l = lib()
    l.eg_gaze_pair_stats_workspace_bytes.restype = C.c_int64
    return int(l.eg_gaze_pair_stats_workspace_bytes(n_images))


def spec_conv1_band_rows(F: int, nfr: int) -> int:
    """Pooled rows per band of conv-1 for F x nfr images (host only): 0 = the whole-image kernels, -1 = no band fits the LDS"""
    return int(lib().eg_spec_conv1_band_rows(F, nfr))


def tsne_workspace_bytes(N: int) -> int:
    """Bytes of workspace eg_tsne_joint and eg_tsne_gradient need for N points (host only; -1: N out of range)"""
    l = lib()
    l.eg_tsne_workspace_bytes.restype = C.c_int64
    return int(l.eg_tsne_workspace_bytes(N))


def exported_symbols():
    l = lib()
    return {n: hasattr(l, n) for n in list(SIGNATURES) + ["eg_abi_version", "eg_last_error"]}


CALLS = 0  # number of C-ABI calls issued so far (graph.py uses it to skip empty capture segments)


def call(name: str, *args):
    global CALLS
    CALLS += 1
    l = lib()
    rc = getattr(l, name)(*args)
    if rc != 0:
        raise EgError(f"{name}: {l.eg_last_error().decode()}")


def ptr(t) -> int:
    """Device (or host) address of a torch tensor / None."""
    return 0 if t is None else t.data_ptr()
