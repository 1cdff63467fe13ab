"""Step engine: sequences the C-ABI kernels (include/eyegaze_hip.h) for one forward / backward / optimiser
step of the dual-stream window classifier.  torch is used for device memory, streams and (in ddp.py)
torch.distributed only; every arithmetic op on the path is a HIP kernel from libeyegaze_hip.so.

Data layout in HBM (NB = 2B windows: stream 1 = samples [0,B), stream 2 = [B,2B); M = NB*S token rows):
  xt      [NB, Tp, Cp]      channel-last, zero-padded input windows (k//2 in front)           compute dtype
  h0pad   [NB, R0, d]       conv-0 output, k//2 zero rows in front/behind (R0 = U*stride)      compute dtype
  seq/x_l [M, d]            token rows [CLS | IBS | spec | temporal], row-major                compute dtype
  qkv_l   [M, 3d]  ctx_l [M, d]  r1/r2 (pre-LN sums) [M, d]  hff_l [M, d_ff]                   compute dtype
  lse_l   [NB, H, S]  LN stats [M, 2]  logits / losses                                          fp32
  parameters, gradients, AdamW moments: ONE flat fp32 buffer each (16-B aligned segments, registration order)

What is stated once here:
  geometry()        the front end's and the sequence's row / column counts for (cfg, T, dtype), device-free
  LAYOUTS           every packed weight layout: shape, pack operation, source, and the direction and route that read it
  EngineBase        device / dtype fields, step state, timed launches, gemm / wgrad, allocation and pack recording from LAYOUTS
                    and the pack table (also ImageEngine's base)
  ForwardEngine     the encoder forward: routes, its stages of LAYOUTS, the launches, ONE forward body that asks the engine where
                    each stage's rows go (_rows)
  Engine            training: per-layer saved activations, the backward in stages, accumulation, the optimiser
  InferenceEngine   forward only: a ping-pong pair + scratch on demand, the forward-reading layouts, the training calls refused
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import os
from collections import namedtuple
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib as L
from . import tokens, wgrad_plan
from ._lib import EG_BF16, EG_F16, EG_F32, GemmDesc, GemmTNDesc, StepState, call, ptr, rowmap

# dropout site ids (any fixed numbering works: the mask depends on (seed, site, element index))
SITE_CONV0, SITE_CONV1, SITE_SPEC, SITE_IBSTOK, SITE_IBSGEN, SITE_CLS, SITE_IBSCLS = 1, 2, 3, 4, 5, 6, 7
# eg_window_augment's own sites (EG_SITE_AUG_* of include/eyegaze_hip.h; the kernel names them, no call passes them)
SITE_AUG_NOISE_R, SITE_AUG_NOISE_T, SITE_AUG_CHAN, SITE_AUG_TIME = 8, 9, 10, 11
# eg_gaze_batch's own sites (EG_SITE_IMG_*; gaze.py); with them every site below 16 is taken
SITE_IMG_FLIP, SITE_IMG_BRIGHT, SITE_IMG_CONTRAST, SITE_IMG_ORDER = 12, 13, 14, 15


@dataclasses.dataclass(frozen=True)
class WindowAugmentation:
    """Training-time augmentation of the input windows (eg_window_augment): additive Gaussian noise, whole
    channels zeroed without rescaling, `time_mask_num` zeroed intervals of 1 .. time_mask_max_length samples per window, the
    same for both players.  Refuses what the C entry point refuses.  An instance with everything off is `not enabled`:
    DualEEGTransformer.augmentation treats it as None."""
    gaussian_noise_std: float = 0.0
    channel_dropout_prob: float = 0.0
    time_mask_max_length: int = 0
    time_mask_num: int = 0

    def __post_init__(self):
        for name in ("gaussian_noise_std", "channel_dropout_prob"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise ValueError(f"{name} must be a number (got {v!r})")
        for name in ("time_mask_max_length", "time_mask_num"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"{name} must be an integer (got {v!r})")
        if not (math.isfinite(self.gaussian_noise_std) and self.gaussian_noise_std >= 0.0):
            raise ValueError(f"gaussian_noise_std must be finite and >= 0 (got {self.gaussian_noise_std!r})")
        if not 0.0 <= self.channel_dropout_prob < 1.0:
            raise ValueError(f"channel_dropout_prob must lie in [0, 1) (got {self.channel_dropout_prob!r})")
        if not 0 <= self.time_mask_num <= 8:
            raise ValueError(f"time_mask_num must lie in [0, 8] (got {self.time_mask_num!r})")
        if self.time_mask_max_length < (1 if self.time_mask_num > 0 else 0):
            raise ValueError(f"time_mask_max_length must be >= 1 when time_mask_num > 0, and never negative "
                             f"(got {self.time_mask_max_length!r})")

    @property
    def enabled(self) -> bool:
        return self.gaussian_noise_std > 0.0 or self.channel_dropout_prob > 0.0 or self.time_mask_num > 0


def scramble_seed(seed: int) -> int:
    """splitmix64 finalizer: the 64-bit word whose halves eg_step_state.seed_lo / seed_hi carry to the dropout hash."""
    m = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


_reduce_blocks = wgrad_plan.reduce_blocks


def _layer_sites(l: int):
    b = 16 + 8 * l
    return dict(attn=b, drop1=b + 1, ffn_a=b + 2, ffn_b=b + 3, drop2=b + 4)


def _attn_prefix(l) -> str:
    """parameter prefix of attention stage l: an encoder layer's index, or "x" for the cross-attention block"""
    return "cross_attn.cross_attn." if l == "x" else f"encoder.layers.{l}.mha."


def _align(n: int, a: int) -> int:
    return (n + a - 1) // a * a


ATTN_SHORT_MAX_S = 160      # eg_attention_fwd / _bwd / _probs: a whole window's scores in registers (csrc/attention.hip)
ATTN_LONG_MAX_S = 2048      # eg_attention_long_*: flash-style tiles (csrc/attention_long.hip, EG_ATTN_LONG_MAX_S)


# Row and column counts of the front end and the token sequence for one (cfg, T, dtype), from geometry():
#   k, s, pad   convolution kernel, stride, padding          Cp      input channels, padded to 8
#   T1, T2      conv-0 / conv-1 output rows per window       J       tap blocks per stride phase of conv-1's backward-data
#   K0          conv-0 GEMM depth (zero-padded to the K-tile)  Tp    padded input rows per window
#   U           backward-data rows per phase                 R0      padded conv-0 output rows per window (U * s)
#   RY          padded dY rows per window (backward-data)    off     first temporal token row: 1 (CLS) + IBS + spectrogram tokens
#   S           tokens per window
Geometry = namedtuple("Geometry", "k s pad Cp T1 T2 J K0 Tp U R0 RY off S")


def geometry(cfg, T: int, dtype: int = EG_BF16) -> Geometry:
    """The one statement of the front end's arithmetic; needs no device and checks nothing (sequence_length does).  The dtype only
    sets the GEMM K-tile behind K0 and Tp."""
    k, s = cfg.conv_kernel_size, cfg.conv_stride
    pad, Cp = k // 2, _align(cfg.in_channels, 8)
    T1 = (T + 2 * pad - k) // s + 1
    T2 = (T1 + 2 * pad - k) // s + 1
    J = (k + s - 1) // s
    K0 = _align(k * Cp, 32 if dtype == EG_F32 else 64)
    U = (T1 + 2 * pad + s - 1) // s
    off = 1 + cfg.num_ibs_tokens + (cfg.in_channels if cfg.use_spectrogram else 0)
    return Geometry(k, s, pad, Cp, T1, T2, J, K0, _align(max(T + 2 * pad, s * (T1 - 1) + K0 // Cp + 1), 8), U, U * s,
                    T2 + 2 * (J - 1), off, off + T2)


def sequence_length(cfg, T: int) -> int:
    """Token count S = 1 (CLS) + IBS tokens + spectrogram tokens + T2 of a model config at window length T, after the checks
    that need no device: S within the positional table and the attention core's limit, and (with IBS) 64 <= T <= 2048, the
    synchrony kernels' range.  Raises EgError naming the limit that fails."""
    geo = geometry(cfg, T)
    s, S = geo.s, geo.S
    if geo.T2 < 1:
        raise L.EgError(f"window length {T} is too short for the two stride-{s} convolutions")
    if S > cfg.max_len:
        raise L.EgError(f"sequence length {S} exceeds max_len {cfg.max_len} of the positional table")
    if S > ATTN_LONG_MAX_S:
        raise L.EgError(f"sequence length {S} exceeds the attention core's limit of {ATTN_LONG_MAX_S}")
    if cfg.use_ibs and not 64 <= T <= 2048:
        raise L.EgError(f"window length {T}: the IBS synchrony kernels need 64 <= T <= 2048")
    return S


ATTN_HEAD_DIMS = (32, 64)   # head widths the attention kernels are built for (csrc/attention_long.hip; the short core and the block: 32)


def attention_head_dim(cfg) -> int:
    """Head width d_model / num_heads of a model config, 32 or 64; needs no device.  Raises EgError naming both otherwise."""
    d, H = cfg.d_model, cfg.num_heads
    if H <= 0 or d % H != 0 or d // H not in ATTN_HEAD_DIMS:
        raise L.EgError(f"HIP attention core needs d_model/num_heads == 32 or 64 (got {d}/{H})")
    return d // H


class FlatParams:
    """All parameters of a module as views of one flat fp32 buffer (+ a flat gradient buffer).
    Segment offsets are multiples of 4 floats so every kernel can use 16-B accesses."""

    def __init__(self, module: torch.nn.Module):
        self.module = module
        self.names: List[str] = []
        self.params: List[torch.nn.Parameter] = []
        self.offsets: Dict[str, int] = {}
        off = 0
        for n, p in module.named_parameters():
            self.names.append(n)
            self.params.append(p)
            self.offsets[n] = off
            off += _align(p.numel(), 4)
        self.total = off
        self.flat: Optional[torch.Tensor] = None
        self.grad: Optional[torch.Tensor] = None
        self.acc: Optional[torch.Tensor] = None      # gradient accumulator over micro-batches (accumulator(): made on first use)

    def ensure(self, device: torch.device, need_grad: bool = True):
        """(Re)flattens when the module was moved / re-created since the last call.  need_grad=False (the forward-only route)
        leaves the gradient buffer to the first caller that needs one."""
        ok = self.flat is not None and self.flat.device == device
        if ok:
            base = self.flat.data_ptr()
            for n, p in zip(self.names, self.params):
                if p.data_ptr() != base + 4 * self.offsets[n] or p.dtype != torch.float32:
                    ok = False
                    break
        if ok:
            if need_grad and self.grad is None:
                self.grad = torch.zeros(self.total, device=device, dtype=torch.float32)
            return
        flat = torch.zeros(self.total, device=device, dtype=torch.float32)
        for n, p in zip(self.names, self.params):
            o = self.offsets[n]
            flat[o:o + p.numel()].copy_(p.data.reshape(-1).to(device=device, dtype=torch.float32))
            p.data = flat[o:o + p.numel()].view(p.shape)
        self.flat = flat
        self.grad = torch.zeros(self.total, device=device, dtype=torch.float32) if need_grad else None
        self.acc = None                # belongs to the buffers it was made beside: re-made on the next accumulator()

    def accumulator(self) -> torch.Tensor:
        """fp32 buffer of the gradient buffer's length and device that Engine.accumulate sums micro-batch gradients into.  It
        exists only once gradient accumulation is used, and never outlives a re-flatten."""
        if self.acc is None:
            self.acc = torch.zeros_like(self.grad)
        return self.acc

    def p_ptr(self, name: str) -> int:
        return self.flat.data_ptr() + 4 * self.offsets[name]

    def g_ptr(self, name: str) -> int:
        return self.grad.data_ptr() + 4 * self.offsets[name]

    def grad_view(self, name: str, p: torch.nn.Parameter) -> torch.Tensor:
        o = self.offsets[name]
        return self.grad[o:o + p.numel()].view(p.shape)

    def has(self, name: str) -> bool:
        return name in self.offsets


def conv_bwd_data_phases(k: int, s: int, pad: int, T1: int):
    """The work a strided convolution's backward-data needs, per stride phase ph: [(ph, u0, n, j0)].  Phase ph gives the input
    gradient's padded rows t = u*s + ph from J = ceil(k/s) tap blocks, block j holding tap s*(J-1-j) + ph.  Rows u0 .. u0+n-1
    are the ones with pad <= t < pad + T1 (the rest are padding, which no reader touches); j0 = 1 when block 0's tap lies
    beyond the kernel (a block of zeros in the transposed weights), else 0.  Phases without a real row are left out."""
    J = (k + s - 1) // s
    U = (T1 + 2 * pad + s - 1) // s
    out = []
    for ph in range(s):
        u0 = max(0, -((ph - pad) // s))
        u1 = min(U - 1, (pad + T1 - 1 - ph) // s)
        if u1 >= u0:
            out.append((ph, u0, u1 - u0 + 1, 1 if J > 1 and s * (J - 1) + ph > k - 1 else 0))
    return out


class EngineBase:
    """What every step engine is built on: device / dtype fields, the step state, timed launches, the GEMM and weight-gradient
    wrappers, the table-driven parameter staging from LAYOUTS.  A subclass names its stages (_stages) and the layouts it holds
    (_held), allocates a, w (_alloc_w), g, and ends with _init_state."""
    tn_cap = 0      # floats of g["partial"], the split-K partials of wgrad (a subclass sizes it)

    def __init__(self, model, B: int, device, dtype: int):
        device = torch.device(device)
        self.model, self.B, self.device, self.dtype = model, B, device, dtype
        self.tdtype = {EG_BF16: torch.bfloat16, EG_F16: torch.float16, EG_F32: torch.float32}[dtype]
        self.es = 4 if dtype == EG_F32 else 2
        self.bk = 32 if dtype == EG_F32 else 64
        self.fp: FlatParams = model._flat
        self.stream = 0
        self.cus = torch.cuda.get_device_properties(device).multi_processor_count if device.type == "cuda" else 256
        self.a, self.w, self.g = {}, {}, {}     # activations, packed weights, backward temporaries (allocated on the first backward)
        self.probes = {}        # tag -> (start_event, end_event) recorded around that launch
        self.probe_all = None   # list of (start, end, flops, bytes, shape, route) of every timed launch when bench.py enables it
        self.probe_pool = None  # bench.py's pre-created event pairs (see _probe_pair)
        # fp16 has 5 exponent bits: gradients are carried at loss_scale x their value (torch.cuda.amp.GradScaler semantics,
        # train_multimodal_fuzzy_fusion.py:435-472); the scale, the overflow flag and the step counter live in eg_step_state
        self.scaler_on = False
        self.scaler_cfg = dict(init_scale=65536.0, growth=2.0, backoff=0.5, growth_interval=2000)
        # the recorded pack table (pack_params)
        self._plan, self._plan_launches, self._plan_ex = [], [], False
        self._plan_key, self._plan_dev, self._plan_n, self._plan_blocks = None, None, 0, 0
        # the routes pack_params keys its table on.  Off here: an engine that has them resolves them (_resolve_routes)
        self.fused_tail = self.pack_unused = False
        self.fuse_ffn = self.attn_block = self.ln_proj = False

    def _init_state(self, state_dev: Optional[torch.Tensor]):
        """state_dev: a shared eg_step_state, initialised once by whoever created it (DualEEGTransformer._state_for).  Every engine
        of one model (one per batch shape: the ragged tail batch of an epoch gets its own workspace) must step ONE optimiser
        count, ONE loss scale and ONE overflow history; an engine given no state creates (and initialises) its own."""
        if state_dev is not None:
            self.state_dev = state_dev
        else:
            self.state_dev = torch.zeros(L.STATE_WORDS, dtype=torch.int32, device=self.device)
            self.set_state(seed=0, lr=0.0, step=1, grad_scale=1.0, reset_scaler=(1 if self.scaler_on else 2),
                           init_scale=self.scaler_cfg["init_scale"])

    def _t(self, *shape, dtype=None):
        return torch.zeros(*shape, device=self.device, dtype=dtype or self.tdtype)

    def _cur_stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream if self.device.type == "cuda" else 0

    # ------------------------------------------------------------------------------------------
    # step state
    # ------------------------------------------------------------------------------------------
    def set_state(self, seed: int, lr: float, step: int, grad_scale: float = 1.0, beta1=0.9, beta2=0.999,
                  reset_scaler: int = 0, init_scale: float = 65536.0, use_dev_t: bool = False):
        """Publishes this step's host scalars.  They travel as kernel ARGUMENTS of a one-thread launch on the current
        stream (eg_set_step_state), so the host may run any number of steps ahead: a queued step can never observe a later
        step's seed / lr / bias corrections (a pinned staging buffer re-used per step could be overwritten before its copy ran).
        reset_scaler: 0 keep the device's loss-scaling words, 1 enable dynamic loss scaling at init_scale, 2 disable."""
        seed = scramble_seed(seed)     # consecutive step seeds must not share their low / high words (common.h: eg_hash)
        # with loss scaling a step may be skipped on the device: the device's own count of taken steps feeds the bias corrections
        use_dev_t = bool(use_dev_t) or self.scaler_on
        call("eg_set_step_state", self.state_dev.data_ptr(), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, float(lr),
             1.0 - beta1 ** step, 1.0 - beta2 ** step, float(grad_scale), int(reset_scaler), float(init_scale),
             int(use_dev_t), self._cur_stream())

    def reset_scaler(self, init_scale: float = 65536.0, growth: float = 2.0, backoff: float = 0.5, growth_interval: int = 2000):
        """(re)starts dynamic loss scaling with GradScaler's parameters (fp16 engines only)"""
        self.scaler_cfg = dict(init_scale=init_scale, growth=growth, backoff=backoff, growth_interval=growth_interval)
        self.scaler_on = True
        self.set_state(seed=0, lr=0.0, step=1, reset_scaler=1, init_scale=init_scale)

    @property
    def loss_scale_dev(self) -> torch.Tensor:
        """the device-resident loss scale as a 1-element fp32 view of eg_step_state (word 8)"""
        return self.state_dev.view(torch.float32)[8:9]

    def read_state(self) -> StepState:
        host = self.state_dev.cpu()
        st = StepState()
        C.memmove(C.addressof(st), host.data_ptr(), C.sizeof(st))
        return st

    @property
    def st_ptr(self) -> int:
        return self.state_dev.data_ptr()

    # ------------------------------------------------------------------------------------------
    # thin wrappers
    # ------------------------------------------------------------------------------------------
    def gemm(self, A, W, Cout, M, N, K, *, a=None, c=None, r=None, p=None, ldw=None, bias=0, residual=0, gate=0,
             out_pre=0, act=0, drop1=(0.0, 0), drop2=(0.0, 0), gate_scale=1.0, tag=None, seg=(0, 0)):
        dsc = self._gemm_desc(A, W, Cout, M, N, K, a, c, r, p, ldw, bias, residual, gate, out_pre, act, drop1, drop2,
                              gate_scale, seg)
        probe = self._timed(lambda: (2.0 * M * N * K, self._gemm_bytes(M, N, K, a, seg, residual, gate, out_pre, Cout),
                                     (M, N, K), L.lib().eg_gemm_nt_route(C.byref(dsc))), tag)
        call("eg_gemm_nt", C.byref(dsc), self.stream)
        self._timed_end(probe)

    def gemm_batch(self, items):
        """eg_gemm_nt_batch: the products `items` -- dicts of gemm()'s arguments, one dtype and one epilogue kind -- as ONE
        wide-tile launch where all of them fit it, else one launch each; the bits of len(items) gemm() calls either way."""
        dflt = dict(a=None, c=None, r=None, p=None, ldw=None, bias=0, residual=0, gate=0, out_pre=0, act=0, drop1=(0.0, 0),
                    drop2=(0.0, 0), gate_scale=1.0)
        descs = (GemmDesc * len(items))()
        for i, it in enumerate(items):
            descs[i] = self._gemm_desc(it["A"], it["W"], it["C"], it["M"], it["N"], it["K"], *[it.get(k, v) for k, v in dflt.items()])

        def work():                         # bench.py: one timed launch carrying the work of all its products
            nbytes = sum(self._gemm_bytes(it["M"], it["N"], it["K"], it.get("a"), (0, 0), it.get("residual", 0), it.get("gate", 0),
                                          it.get("out_pre", 0), it["C"]) for it in items)
            return (sum(2.0 * it["M"] * it["N"] * it["K"] for it in items), nbytes,
                    (sum(it["M"] for it in items), items[0]["N"], max(it["K"] for it in items)),
                    L.lib().eg_gemm_nt_route(C.byref(descs[0])))
        probe = self._timed(work)
        call("eg_gemm_nt_batch", descs, len(items), self.stream)
        self._timed_end(probe)

    def _probe_pair(self):
        """A (start, end) event pair for a timed launch: from bench.py's pre-created pool when there is one -- creating a
        hipEvent costs the host far more than recording one, and fresh events inside the timed region made short runs host-bound."""
        if self.probe_pool:
            return self.probe_pool.pop()
        return (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))

    def _timed(self, work, tag=None):
        """Before a launch that bench.py times (_timed_end follows it): with probe_all a list, HIP events go around EVERY such
        launch and work() -- (flops, algorithmic HBM bytes, shape, route) -- is appended behind them; else `tag` may name a pair."""
        probe = self.probes.get(tag) if tag else None
        if self.probe_all is not None:
            probe = self._probe_pair()
            self.probe_all.append((probe[0], probe[1], *work()))
        if probe:
            probe[0].record(torch.cuda.current_stream(self.device))
        return probe

    def _timed_end(self, probe):
        if probe:
            probe[1].record(torch.cuda.current_stream(self.device))

    def _gemm_bytes(self, M, N, K, a, seg, residual, gate, out_pre, Cout=1) -> float:
        """Algorithmic HBM bytes of one gemm_nt launch: every distinct operand element read once, every output element
        written once (overlapping conv rows count once; the weights count once)."""
        es = self.es
        if a is not None and a.rows_per_group > 0 and not seg[0]:
            groups = M // a.rows_per_group
            a_elems = groups * ((a.rows_per_group - 1) * min(a.row_stride, K) + K)
        elif seg[0]:                       # segmented rows (spectrogram conv): K elements per row drawn from K/seg_len runs
            a_elems = M * K if a is None else min(M * K, M * max(a.row_stride, 1) + K)
        else:
            a_elems = M * K
        outs = (1 if Cout else 0) + (1 if out_pre else 0)
        ins = (1 if residual else 0) + (1 if gate else 0)
        return float(es * (a_elems + N * K + (outs + ins) * M * N) + 4 * N)

    def _gemm_desc(self, A, W, Cout, M, N, K, a, c, r, p, ldw, bias, residual, gate, out_pre, act, drop1, drop2, gate_scale,
                   seg=(0, 0)):
        dsc = GemmDesc()
        dsc.a_seg_len, dsc.a_seg_stride = seg
        dsc.A, dsc.W, dsc.C = A, W, Cout or None
        dsc.bias, dsc.residual, dsc.gate, dsc.out_pre = bias or None, residual or None, gate or None, out_pre or None
        dsc.state = self.st_ptr
        dsc.a = a or rowmap(K)
        dsc.c = c or rowmap(N)
        dsc.r = r or dsc.c
        dsc.p = p or dsc.c
        dsc.M, dsc.N, dsc.K, dsc.ldw = M, N, K, ldw or K
        dsc.act, dsc.dtype = act, self.dtype
        dsc.drop1_p, dsc.drop1_site = drop1
        dsc.drop2_p, dsc.drop2_site = drop2
        dsc.gate_scale = gate_scale
        return dsc

    def _packed(self, names, N, K) -> bool:
        """`name.weight` / `name.bias` of the product [N, K] back to back in the flat buffers (wgrad_plan.packed)"""
        return wgrad_plan.packed(self.fp.offsets, names, N, K)

    def wgrad(self, dY, X, out_w, M, N, K, *, y=None, x=None, out_b=0, conv=None, split_out=None, x_tile_stride=0,
              conv2d=None, linear=None):
        """dW = dY^T X (+ db = colsum dY).
        linear=[prefix, ...]: the product feeds N/len(linear) rows to each `prefix.weight` / `prefix.bias`; when those
        parameters are laid out back to back in the flat buffer (they are: registration order) the bias sums are fused
        into the GEMM launch and ONE reduce writes every weight and bias gradient.
        conv / conv2d: tap-major partials are un-permuted into the parameter layout; out_b via a column-sum launch."""
        tiles = ((N + 127) // 128) * ((K + 127) // 128)
        fused = linear is not None and (N // len(linear)) % 4 == 0 and self._packed(linear, N, K)
        slab = N * K + (N if fused else 0)
        # one resident round: 256 CUs x 3 workgroups; rounding the split count UP would leave a nearly empty second round
        splits = max(1, min((M + 127) // 128, max(1, 768 // tiles), self.tn_cap // slab))
        # big products on 16-bit operands: 256 x 256 tiles, one 512-thread workgroup per CU (conv-1: 25 tiles x 10 row splits)
        big = self.dtype != EG_F32 and N % 256 == 0 and K % 256 == 0 and not x_tile_stride and M * N * K >= (1 << 34)
        if big:
            t256 = (N // 256) * (K // 256)
            splits = max(1, min((M + 63) // 64, max(1, self.cus // t256), self.tn_cap // slab))
        dsc = GemmTNDesc()
        dsc.tile = 256 if big else 128
        dsc.dY, dsc.X, dsc.partial = dY, X, ptr(self.g["partial"])
        dsc.y = y or rowmap(N)
        dsc.x = x or rowmap(K)
        dsc.M, dsc.N, dsc.K, dsc.splits, dsc.dtype = M, N, K, splits, self.dtype
        dsc.x_tile_stride = x_tile_stride
        if fused:
            dsc.part_rows, dsc.has_bias = N // len(linear), 1
        call("eg_gemm_tn", C.byref(dsc), self.stream)
        pp = ptr(self.g["partial"])
        if fused:
            call("eg_reduce_partials", pp, self.fp.g_ptr(linear[0] + ".weight"), slab, splits, slab, 0, self.stream)
            return
        if linear is not None:  # non-contiguous parameters: per-parameter reduces + a column-sum launch
            P = N // len(linear)
            split_out = [(self.fp.g_ptr(n + ".weight"), i * P, P) for i, n in enumerate(linear)]
            out_b = [(self.fp.g_ptr(n + ".bias"), i * P, P) for i, n in enumerate(linear)]
        if conv2d is not None:
            call("eg_unpack_conv2d_wgrad", pp, out_w, splits, conv2d[0], conv2d[1], self.stream)
        elif conv is not None:
            cin, kk, cp = conv
            call("eg_unpack_conv_wgrad", pp, out_w, splits, N, cin, kk, cp, K, self.stream)
        elif split_out is not None:
            for gp, row0, rows in split_out:
                call("eg_reduce_partials", pp + 4 * row0 * K, gp, rows * K, splits, N * K, 0, self.stream)
        else:
            call("eg_reduce_partials", pp, out_w, N * K, splits, N * K, 0, self.stream)
        if out_b:
            nblk = min(512, (M + 63) // 64)
            call("eg_colsum", dY, dsc.y, M, N, ptr(self.g["cspart"]), nblk, self.dtype, self.stream)
            if isinstance(out_b, (list, tuple)):
                for gp, col0, cols in out_b:
                    call("eg_reduce_partials", ptr(self.g["cspart"]) + 4 * col0, gp, cols, nblk, N, 0, self.stream)
            else:
                call("eg_reduce_partials", ptr(self.g["cspart"]), out_b, N, nblk, N, 0, self.stream)

    # ------------------------------------------------------------------------------------------
    # parameter staging
    # ------------------------------------------------------------------------------------------
    # table-driven staging: _pack_body walks LAYOUTS once per plan; the p_* operations record cast / transpose / ... entries,
    # replayed as ONE launch per step, and what no table mode carries as launches of their own, issued on every pack_params
    def p_cast(self, src, dst, n):
        self._plan.append((src, dst, 1, n, 0, 0))

    def p_copy(self, src, dst, n):
        self._plan.append((src, dst, 1, n, 0, 2))

    def p_transpose(self, src, dst, R, Cc, ldd):
        self._plan.append((src, dst, R, Cc, ldd, 1))

    def p_frag(self, src, dst, R, Cc, mode, part=0):
        """fragment order of the fp32 parameter src [R, Cc]: eg_ffn_chain's (eg_pack_table modes 3-6) or eg_attn_block_fwd's
        (mode 7 with part = 0 / 1 / 2 for q / k / v_proj, mode 8 for out_proj)."""
        self._plan.append((src, dst, R, Cc, part, mode))

    def p_conv(self, src, dst, N, Cin, k, Cp, Kp):
        """eg_pack_conv_weight as an entry of the pack table (fused route) or as its own launch"""
        if self._plan_ex:
            self._plan.append((src, dst, N, Cin, 0, 9, k, Cp, Kp))
        else:
            self._plan_launches.append(("eg_pack_conv_weight", src, dst, N, Cin, k, Cp, Kp))

    def p_convT(self, src, dst, N, Cin, k, s):
        """eg_pack_convT_weight, likewise"""
        if self._plan_ex:
            self._plan.append((src, dst, N, Cin, 0, 10, k, s, (k + s - 1) // s))
        else:
            self._plan_launches.append(("eg_pack_convT_weight", src, dst, N, Cin, k, s))

    def p_conv2d(self, src, dst, Cout, Cin, transposed):
        """eg_pack_conv2d_weight: no table mode carries it, so always its own launch"""
        self._plan_launches.append(("eg_pack_conv2d_weight", src, dst, Cout, Cin, transposed))

    def _alloc_w(self) -> Dict[str, torch.Tensor]:
        d, F = self.cfg.d_model, getattr(self.cfg, "d_ff", None)       # (the image engine has no feed-forward stage)
        return {f"{lay.key}{l}": self._t(*lay.shape(d, F, self), dtype=(torch.float32 if lay.op == "copy" else None))
                for stage, _, l in self._stages() for group in LAYOUTS[stage] for lay in self._held(group, l, True)}

    def _pack_body(self, record: bool):
        """What pack_params does before the table launch: a walk of LAYOUTS when the plan is (re)recorded, then the launches that
        the walk left beside the table."""
        if record:
            self._plan, self._plan_launches = [], []
            d, F, fp = self.cfg.d_model, getattr(self.cfg, "d_ff", None), self.fp
            for stage, pre, l in self._stages():
                for group in LAYOUTS[stage]:
                    held = self._held(group, l, bool(self.pack_unused))
                    for i in range(len(group[0].src)):
                        for lay in held:
                            t = self.w[f"{lay.key}{l}"]
                            src, dst, args = fp.p_ptr(pre + lay.src[i]), ptr(t), lay.args(d, F, self)
                            # source i: the next args[0] elements (cast, copy) or columns (transpose: ldd = the buffer's width)
                            # of the buffer; a fragment layout takes the source index as its part
                            off = 0 if lay.op == "frag" else i * args[0] * t.element_size()
                            extra = (t.shape[1],) if lay.op == "transpose" else (i,) if lay.op == "frag" else ()
                            getattr(self, "p_" + lay.op)(src, dst + off, *args, *extra)
        for name, *args in self._plan_launches:
            call(name, *args, self.dtype, self.stream)

    def _extent_after(self, addr: int, elsize: int) -> int:
        """elements of size `elsize` between `addr` and the end of the engine / parameter buffer that holds it (0: not found)"""
        bufs = list(self.w.values()) + [self.fp.flat]
        for t in bufs:
            lo = t.data_ptr()
            hi = lo + t.numel() * t.element_size()
            if lo <= addr < hi:
                return (hi - addr) // elsize
        return 0

    def pack_params(self):
        ex = bool(self.fused_tail)          # eg_pack_table_ex carries the convolution layouts too; the image engine keeps eg_pack_table
        # the routing flags decide which layouts _pack_body records, so a flag flipped on a live engine re-records the plan
        key = (self.fp.flat.data_ptr(), ex, bool(self.pack_unused), self.fuse_ffn, self.attn_block, self.ln_proj)
        self._plan_ex = ex
        record = self._plan_key != key
        self._pack_body(record)
        if record:
            ents = ((L.PackEntryEx if ex else L.PackEntry) * len(self._plan))()
            blk = 0
            for e, ent in zip(ents, self._plan):
                src, dst, R, Cc, ldd, mode = ent[:6]
                if mode == 9:
                    nb = (R * ent[8] + 1023) // 1024
                elif mode == 10:
                    nb = (ent[7] * Cc * ent[8] * R + 1023) // 1024
                else:
                    nb = (((R + 31) // 32) * ((Cc + 31) // 32) if mode == 1 else (R * Cc) // 2048 if mode >= 3 else
                          (R * Cc + 1023) // 1024)
                e.src, e.dst, e.rows, e.cols, e.ldd, e.mode, e.blk0, e.nblk = src, dst, R, Cc, ldd, mode, blk, nb
                if ex:
                    if mode >= 9:
                        e.p0, e.p1, e.p2 = ent[6:9]
                    e.src_elems = self._extent_after(src, 4)
                    e.dst_elems = self._extent_after(dst, 4 if mode == 2 else self.es)
                blk += nb
            if ex:      # host-side audit of every entry (block ranges, shapes, alignment, extents) before the table is ever launched
                total = C.c_int(0)
                call("eg_pack_table_ex_check", C.cast(ents, C.c_void_p), len(self._plan), self.dtype, C.byref(total))
                if total.value != blk:
                    raise L.EgError(f"pack table: {total.value} blocks audited, {blk} planned")
            raw = torch.frombuffer(bytearray(bytes(ents)), dtype=torch.uint8)
            self._plan_dev = raw.to(self.device)
            self._plan_n, self._plan_blocks, self._plan_key = len(self._plan), blk, key
        call("eg_pack_table_ex" if ex else "eg_pack_table", ptr(self._plan_dev), self._plan_n, self._plan_blocks, self.dtype,
             self.stream)


# ------------------------------------------------------------------------------------------------
# packed weight layouts of every engine: the one declaration that allocation and pack recording are derived from
# ------------------------------------------------------------------------------------------------
# w[key + stage]: one packed form of a parameter (or, with several sources, of the parameters that share the buffer)
#   shape   (d, F, engine) -> shape of the buffer; fp32 for "copy", else the compute dtype
#   op      cast | copy | transpose | frag | conv | convT | conv2d: the p_* operation that fills it
#   args    (d, F, engine) -> that operation's arguments behind (src, dst), for one source
#   src     parameter names under the stage's prefix; part i of the buffer comes from src[i]
#   bwd     read by the backward; else by the forward
#   route   the route attribute that decides whether anything reads it (None: always read) ...
#   fused   ... namely when that route is on (True) or off (False)
Layout = namedtuple("Layout", "key shape op args src bwd route fused", defaults=(False, None, False))


def _lay(key, shape, op, args, *src, **kw):
    return Layout(key, shape, op, args, src, **kw)


_QKV = ("q_proj.weight", "k_proj.weight", "v_proj.weight")
_BLOCK, _LNPROJ, _FFN = "attn_block", "ln_proj", "fuse_ffn"
# stage -> groups in recording order; the layouts of one group are recorded source by source (q: each of them, k: each of them, ...).
# "attn" is recorded per encoder layer and for the cross-attention block "x", which has no fused route; "ffn" per encoder layer.
LAYOUTS = {
    "front": [
        (_lay("conv0", lambda d, F, e: (d, e.K0), "conv", lambda d, F, e: (d, e.C, e.k, e.Cp, e.K0), "temporal_conv.convs.0.weight"),),
        (_lay("conv1", lambda d, F, e: (d, e.k * d), "conv", lambda d, F, e: (d, d, e.k, d, e.k * d), "temporal_conv.convs.1.weight"),),
        (_lay("conv1T", lambda d, F, e: (e.s, d, e.J * d), "convT", lambda d, F, e: (d, d, e.k, e.s), "temporal_conv.convs.1.weight",
              bwd=True),),
        (_lay("pos", lambda d, F, e: (e.cfg.max_len, d), "cast", lambda d, F, e: (e.cfg.max_len * d,), "pos_embed.pos_embed.weight"),)],
    "attn": [
        (_lay("qkv", lambda d, F, e: (3 * d, d), "cast", lambda d, F, e: (d * d,), *_QKV, route=_BLOCK),
         _lay("qkvT", lambda d, F, e: (d, 3 * d), "transpose", lambda d, F, e: (d, d), *_QKV, bwd=True),
         _lay("bqkv", lambda d, F, e: (3 * d,), "copy", lambda d, F, e: (d,), "q_proj.bias", "k_proj.bias", "v_proj.bias")),
        (_lay("o", lambda d, F, e: (d, d), "cast", lambda d, F, e: (d * d,), "out_proj.weight", route=_BLOCK),),
        (_lay("oT", lambda d, F, e: (d, d), "transpose", lambda d, F, e: (d, d), "out_proj.weight", bwd=True, route=_LNPROJ),),
        # out_proj^T in MFMA-fragment order (eg_pack_table mode 6) for eg_ln_bwd_proj
        (_lay("oTf", lambda d, F, e: (d * d,), "frag", lambda d, F, e: (d, d, 6), "out_proj.weight", bwd=True, route=_LNPROJ, fused=True),),
        # eg_attn_block_fwd's fragment-ordered q|k|v (mode 7, part = source index) and out-proj (mode 8) weights
        (_lay("wqkvb", lambda d, F, e: (3 * d * d,), "frag", lambda d, F, e: (d, d, 7), *_QKV, route=_BLOCK, fused=True),),
        (_lay("wob", lambda d, F, e: (d * d,), "frag", lambda d, F, e: (d, d, 8), "out_proj.weight", route=_BLOCK, fused=True),)],
    "ffn": [
        (_lay("w1", lambda d, F, e: (F, d), "cast", lambda d, F, e: (F * d,), "linear1.weight", route=_FFN),),
        (_lay("w1T", lambda d, F, e: (d, F), "transpose", lambda d, F, e: (F, d), "linear1.weight", bwd=True, route=_FFN),),
        (_lay("w2", lambda d, F, e: (d, F), "cast", lambda d, F, e: (d * F,), "linear2.weight", route=_FFN),),
        (_lay("w2T", lambda d, F, e: (F, d), "transpose", lambda d, F, e: (d, F), "linear2.weight", bwd=True, route=_FFN),),
        # the same four matrices in eg_ffn_chain's MFMA-fragment order (modes 3-6): forward products 1, 2; backward product
        # 1 = linear2^T, 2 = linear1^T
        (_lay("w1f", lambda d, F, e: (F * d,), "frag", lambda d, F, e: (F, d, 3), "linear1.weight", route=_FFN, fused=True),),
        (_lay("w2f", lambda d, F, e: (F * d,), "frag", lambda d, F, e: (d, F, 5), "linear2.weight", route=_FFN, fused=True),),
        (_lay("w2Tf", lambda d, F, e: (F * d,), "frag", lambda d, F, e: (d, F, 4), "linear2.weight", bwd=True, route=_FFN, fused=True),),
        (_lay("w1Tf", lambda d, F, e: (F * d,), "frag", lambda d, F, e: (F, d, 6), "linear1.weight", bwd=True, route=_FFN, fused=True),)],
    "heads": [
        (_lay("sf", lambda d, F, e: (d, 3 * d), "cast", lambda d, F, e: (3 * d * d,), "symmetric_fusion.proj.weight"),),
        (_lay("sfT", lambda d, F, e: (3 * d, d), "transpose", lambda d, F, e: (d, 3 * d), "symmetric_fusion.proj.weight", bwd=True),),
        (_lay("c0", lambda d, F, e: (d, 3 * d), "cast", lambda d, F, e: (3 * d * d,), "classifier.0.weight"),),
        (_lay("c0T", lambda d, F, e: (3 * d, d), "transpose", lambda d, F, e: (d, 3 * d), "classifier.0.weight", bwd=True),)],
    "ibs": [
        (_lay("i0", lambda d, F, e: (d // 2, d), "cast", lambda d, F, e: ((d // 2) * d,), "ibs_classifier.0.weight"),),
        (_lay("i0T", lambda d, F, e: (d, _align(d // 2, e.bk)), "transpose", lambda d, F, e: (d // 2, d), "ibs_classifier.0.weight",
              bwd=True),)],
    # the token families (tokens.py).  "cnn" is the 2-D CNN of the spectrogram tokens and of the image engine: conv-2's weights
    # tap-major for the forward and transposed for the backward-data (eg_pack_conv2d_weight), the two projections
    "cnn": [
        (_lay("spc2", lambda d, F, e: (64, 384), "conv2d", lambda d, F, e: (64, 32, 0), "spec_conv.3.weight"),),
        (_lay("spc2T", lambda d, F, e: (32, 768), "conv2d", lambda d, F, e: (64, 32, 1), "spec_conv.3.weight", bwd=True),),
        (_lay("spp0", lambda d, F, e: (2 * d, 1024), "cast", lambda d, F, e: (2 * d * 1024,), "proj.0.weight"),),
        (_lay("spp0T", lambda d, F, e: (1024, 2 * d), "transpose", lambda d, F, e: (2 * d, 1024), "proj.0.weight", bwd=True),),
        (_lay("spp3", lambda d, F, e: (d, 2 * d), "cast", lambda d, F, e: (d * 2 * d,), "proj.3.weight"),),
        (_lay("spp3T", lambda d, F, e: (2 * d, d), "transpose", lambda d, F, e: (d, 2 * d), "proj.3.weight", bwd=True),)],
    "ibs_tok": [    # matrix-form synchrony tokens: the bottleneck over the C x C connectivity entries
        (_lay("ib0", lambda d, F, e: (64, e.C * e.C), "cast", lambda d, F, e: (64 * e.C * e.C,), "bottleneck.0.weight"),),
        (_lay("ib0T", lambda d, F, e: (e.C * e.C, 64), "transpose", lambda d, F, e: (64, e.C * e.C), "bottleneck.0.weight", bwd=True),),
        (_lay("ib3", lambda d, F, e: (d, 64), "cast", lambda d, F, e: (d * 64,), "bottleneck.3.weight"),),
        (_lay("ib3T", lambda d, F, e: (64, d), "transpose", lambda d, F, e: (d, 64), "bottleneck.3.weight", bwd=True),)],
    "ibs_gen": [    # scalar-form synchrony token: 28 features, zero-padded to the K-tile as a 1-tap convolution
        (_lay("ig0", lambda d, F, e: (2 * d, 64), "conv", lambda d, F, e: (2 * d, 28, 1, 28, 64), "0.weight"),),
        (_lay("ig3", lambda d, F, e: (d, 2 * d), "cast", lambda d, F, e: (d * 2 * d,), "3.weight"),),
        (_lay("ig3T", lambda d, F, e: (2 * d, d), "transpose", lambda d, F, e: (d, 2 * d), "3.weight", bwd=True),)],
}
_ALL_LAYOUTS = [lay for groups in LAYOUTS.values() for group in groups for lay in group]
# forward layout of an unfused route -> the fragment-ordered layout of the same parameters that the fused route reads instead
_FUSED_TWIN = {u.key: f for u in _ALL_LAYOUTS for f in _ALL_LAYOUTS
               if u.route and not (u.bwd or f.bwd or u.fused) and (f.route, f.src, f.fused) == (u.route, u.src, True)}


# Where one encoder stage's rows go, as the engine answers ForwardEngine._rows; None = not stored (the lean launches).
#   qkv, lse, ctx   q|k|v rows, log-sum-exps, context rows          r1, st1, y1   pre-LN sum, statistics and output rows of norm1
#   hff, gbits      hidden rows and their gate bits (an engine without them runs at p = 0)
#   r2, st2         pre-LN sum and statistics of norm2              out           the stage's output rows
# The cross-attention stage "x" fills the attention half and `out` (its normed rows); the final norm "norm" only st2 and out.
Rows = namedtuple("Rows", "qkv lse ctx r1 st1 y1 hff gbits r2 st2 out", defaults=(None,) * 11)


def _heads_counters(B: int, device) -> torch.Tensor:
    """eg_heads_fwd's last-workgroup counters: one for the launch and one per group of 16 samples; each launch leaves them zero"""
    return torch.zeros(1 + (B + 15) // 16, device=device, dtype=torch.int32)


def _head_tensors(cfg, B: int):
    """{name: (shape, is fp32)} of what the heads write (compute dtype unless fp32), device-free"""
    d, nc = cfg.d_model, cfg.num_classes
    t = {"cls1": ((B, d), True), "cls2": ((B, d), True), "comb": ((B, 3 * d), False), "zf": ((B, 3 * d), False), "hcl": ((B, d), False),
         "logits": ((B, nc), True), "sloss": ((B,), True), "loss": ((1,), True)}
    if cfg.use_ibs:
        t.update({"ibs_pool_f": ((B, d), True), "ibs_pool": ((B, d), False), "hib": ((B, d // 2), False),
                  "ibs_logits": ((B, nc), True), "ibs_sloss": ((B,), True), "ibs_loss": ((1,), True)})
    return t


class ForwardEngine(EngineBase):
    """The encoder forward for a fixed (B, T), shared by the training and the inference engine: geometry, forward routes, the packed
    layouts (LAYOUTS), the launches of the front end, an encoder layer, the cross-attention stage and the heads, and ONE forward
    body.  A subclass allocates `a` (_alloc), says which layouts it holds (_held) and where each stage's rows go (_rows)."""

    def __init__(self, model, B: int, T: int, device: torch.device, dtype: int, state_dev: Optional[torch.Tensor] = None):
        """state_dev: the model's shared eg_step_state (see _init_state)"""
        super().__init__(model, B, device, dtype)
        cfg = model.cfg
        self.cfg, self.T = cfg, T
        self.head_dim = attention_head_dim(cfg)
        if cfg.conv_layers != 2:
            raise L.EgError("HIP path implements the reference's 2-layer temporal conv front-end (conv_layers=2)")
        if cfg.d_model % 64 != 0 or cfg.d_ff % 64 != 0:
            raise L.EgError("d_model and d_ff must be multiples of 64")
        self.NB, self.C = 2 * B, cfg.in_channels
        self.geo = geometry(cfg, T, dtype)
        for name, v in self.geo._asdict().items():      # k, s, pad, Cp, T1, T2, J, K0, Tp, U, R0, RY, off, S as plain attributes
            setattr(self, name, v)
        self.n_ibs = cfg.num_ibs_tokens
        self.n_spec = self.C if cfg.use_spectrogram else 0
        sequence_length(cfg, T)                         # its checks
        self.M = self.NB * self.S
        self._resolve_routes()
        self._alloc()
        tokens.alloc(self)
        self._init_state(state_dev)

    def _resolve_routes(self):
        """Every route of the forward, decided once from the compute dtype, the shapes and the surviving switches; nothing else in
        this module reads the environment (but Engine._resolve_routes for the backward's, and _wgrad_pieces).  Tests assign the plain
        attributes on a live engine."""
        cfg, dtype, env = self.cfg, self.dtype, os.environ
        half = dtype != EG_F32
        # S > 160: the long-sequence attention core (eg_attention_long_*) at all four call sites; S <= 160 keeps the short one
        # 64-wide heads: the same core through eg_attention_dk_* at EVERY S (the short core and the fused block are 32 wide only)
        wide = self.head_dim != 32
        self.attn_long = self.S > ATTN_SHORT_MAX_S or wide
        self._attn_core = "eg_attention_dk" if wide else "eg_attention_long" if self.attn_long else "eg_attention"
        self._attn_heads = (cfg.num_heads, self.head_dim) if wide else (cfg.num_heads,)    # H [, head_dim] of the core's arguments
        # attention half of an encoder layer (q|k|v projection, attention core, out-proj + dropout + residual) as ONE launch with a
        # workgroup per window (csrc/attnblock.hip): 16-bit compute dtypes, d_model == 256, 8 heads, S <= 80
        self.attn_block = bool(env.get("EYEGAZE_ATTN_BLOCK", "1") != "0" and half
                               and L.lib().eg_attn_block_ok(self.S, cfg.d_model, cfg.num_heads, dtype))
        # feed-forward pair as one launch (csrc/ffn.hip): 16-bit compute dtypes, d_model == 256, d_ff a multiple of 128
        self.fuse_ffn = half and cfg.d_model == 256 and cfg.d_ff % 128 == 0
        # the two LayerNorms of an encoder layer as the tail of the launches that complete their input rows (eg_attn_block_fwd ->
        # norm1, eg_ffn_chain forward -> norm2) instead of two launches that re-read them; the statistics are summed in another order
        # than eg_layernorm_fwd's, so the step agrees with EYEGAZE_LN_FUSE=0 to rounding, not bit for bit
        self.ln_fuse = env.get("EYEGAZE_LN_FUSE", "1") != "0"
        # the step's small-launch tail on its fused kernels (16-bit compute dtypes): the convolution weight layouts inside the
        # one table-driven pack launch, the heads' forward as pooling + ONE chained launch, their backward as three, and the
        # position / cls / conv-1 gradient rows from ONE pass over dseq.  Same bits as the separate launches, which remain the
        # route for fp32 and for the shapes the fused kernels do not cover (see _fused_heads); tests set this attribute to
        # False to compare the two routes.
        self.fused_tail = half
        # False: pack_params skips the layouts that the routes chosen above never read (see _held); True packs every one
        self.pack_unused = False

    # ------------------------------------------------------------------------------------------
    # packed weights: the stages of LAYOUTS that EngineBase's two walks (_alloc_w, _pack_body) visit
    # ------------------------------------------------------------------------------------------
    def _reads(self, lay, l) -> bool:
        """whether a route chosen NOW reads layout `lay` of stage l (the cross-attention block "x" has no fused route)"""
        return lay.route is None or (bool(getattr(self, lay.route)) and l != "x") == lay.fused

    def _stages(self):
        """(stage of LAYOUTS, parameter prefix, key suffix) in recording order"""
        yield "front", "", ""
        for l in range(self.cfg.num_layers):
            yield "attn", f"encoder.layers.{l}.mha.", l
            yield "ffn", f"encoder.layers.{l}.ffn.", l
        if self.cfg.use_cross_attention:
            yield "attn", "cross_attn.cross_attn.", "x"
        yield "heads", "", ""
        if self.cfg.use_ibs:
            yield "ibs", "", ""
        if self.cfg.use_spectrogram:
            yield "cnn", "spectrogram_generator.", ""
        if self.cfg.use_ibs:
            yield ("ibs_tok", "ibs_tokenizer.", "") if self.cfg.use_robust_ibs else ("ibs_gen", "ibs_generator.proj.", "")

    def _pack_body(self, record: bool):
        super()._pack_body(record)
        tokens.pack(self)           # (the one packed buffer that is no layout of one parameter)

    def _head_alloc(self) -> Dict[str, torch.Tensor]:
        a = {n: self._t(*shape, dtype=(torch.float32 if is32 else None)) for n, (shape, is32) in _head_tensors(self.cfg, self.B).items()}
        a["heads_ctr"] = _heads_counters(self.B, self.device)
        return a

    def attn_unfused_fwd(self, x, l, kv_shift, sites, p, R: Rows):
        """Stage l's forward as three launches: q|k|v = x W^T + b (A:203-205) fused over the three projections (the row-stream
        GEMM at K = 256), the attention core, out-proj + dropout + residual.  kv_shift = B pairs window b with b + B (D:966-974)."""
        M, d = self.M, self.cfg.d_model
        pre, qkv, lse, ctx, r = _attn_prefix(l), R.qkv, R.lse, R.ctx, R.r1
        self.gemm(ptr(x), ptr(self.w[f"qkv{l}"]), ptr(qkv), M, 3 * d, d, bias=ptr(self.w[f"bqkv{l}"]))
        call(self._attn_core + "_fwd", ptr(qkv), ptr(ctx), ptr(lse), self.NB, self.S, *self._attn_heads,
             kv_shift, self.dtype, p, sites["attn"], self.st_ptr, self.stream)
        self._probs_hook(self.model.get_submodule(pre + "dropout"), qkv, lse, kv_shift)
        self._attn_stats(l, qkv, lse, kv_shift)
        self.gemm(ptr(ctx), ptr(self.w[f"o{l}"]), ptr(r), M, d, d, bias=self.fp.p_ptr(pre + "out_proj.bias"),
                  drop1=(p, sites["drop1"]), residual=ptr(x))

    def attn_block_fwd(self, x, l, p, sites, R: Rows, ln=None):
        """eg_attn_block_fwd (csrc/attnblock.hip): A:202-213 + the residual of A:292-293 for encoder layer l in one launch.
        R without q|k|v rows: the lean, forward-only form -- nothing but ln's rows is stored (no q|k|v, lse, ctx, r1, no statistics)"""
        w, fp, d = self.w, self.fp, self.cfg.d_model
        pre, qkv, lse, ctx, r1, lean = _attn_prefix(l), R.qkv, R.lse, R.ctx, R.r1, R.qkv is None
        dsc = L.AttnBlockDesc()
        dsc.x, dsc.wqkv_frag, dsc.wo_frag = ptr(x), ptr(w[f"wqkvb{l}"]), ptr(w[f"wob{l}"])
        dsc.bqkv, dsc.bo = ptr(w[f"bqkv{l}"]), fp.p_ptr(pre + "out_proj.bias")
        dsc.qkv, dsc.ctx, dsc.lse, dsc.r1 = ptr(qkv), ptr(ctx), ptr(lse), ptr(r1)
        dsc.state = self.st_ptr
        dsc.NB, dsc.S, dsc.d_model, dsc.num_heads, dsc.dtype = self.NB, self.S, d, self.cfg.num_heads, self.dtype
        dsc.attn_drop_p, dsc.attn_drop_site = p, sites["attn"]
        dsc.out_drop_p, dsc.out_drop_site = p, sites["drop1"]
        if ln is not None:                  # (gain name, output rows, statistics): norm1 in the same launch
            dsc.ln_gamma, dsc.ln_beta = fp.p_ptr(ln[0] + ".weight"), fp.p_ptr(ln[0] + ".bias")
            dsc.ln_out, dsc.ln_stats = ptr(ln[1]), ptr(ln[2])

        def work():                         # bench.py: timed like the eg_gemm_nt launches, as its own kernel (route 8)
            M, S, H = self.M, self.S, self.cfg.num_heads
            flops = 2.0 * M * d * 3 * d + 2.0 * M * d * d + 4.0 * self.NB * H * S * S * (d // H)
            nbytes = self.es * (M * d * 3 + M * 3 * d + 4 * d * d) + 4 * (self.NB * H * S + 4 * d)    # x, ctx, r1 | qkv | weights | lse, biases
            if ln is not None:
                nbytes += self.es * M * d + 8 * M + 8 * d                                             # norm1 rows, statistics, gain / bias
            if lean:
                nbytes = self.es * (2 * M * d + 4 * d * d) + 4 * 4 * d + 8 * d                        # x, norm1 rows | weights | biases, gain / bias
            return flops, float(nbytes), (M, 3 * d, d), 8
        probe = self._timed(work)
        call("eg_attn_block_fwd", C.byref(dsc), self.stream)
        self._timed_end(probe)

    def ffn(self, A, W1f, W2f, H, Cout, M, F, *, bias1=0, bias2=0, act1=0, residual=0, gate=0, bits_out=0, bits_in=0,
            drop_h=(0.0, 0), drop_c1=(0.0, 0), drop_c2=(0.0, 0), gate_scale=1.0, ln=None, ln_tail=None):
        """eg_ffn_chain: H = epi1(A W1^T), C = epi2(H W2^T) in one launch (weights in fragment order).
        ln_tail (an eg_ln_bwd_proj descriptor; the backward form only): eg_ffn_bwd_ln_proj, the same launch going on with that
        LayerNorm backward and product on its own C rows, which are stored only if Cout is given."""
        d = self.cfg.d_model
        dsc = L.FfnDesc()
        dsc.A, dsc.W1, dsc.W2, dsc.H, dsc.C = A, W1f, W2f, H or None, Cout or None      # (both None: the forward-only form, ln's rows alone)
        dsc.bias1, dsc.bias2, dsc.gate, dsc.residual = bias1 or None, bias2 or None, gate or None, residual or None
        dsc.gate_bits_out, dsc.gate_bits_in = bits_out or None, bits_in or None
        dsc.state = self.st_ptr
        dsc.lda, dsc.ldh, dsc.ldc, dsc.ldg, dsc.ldr = d, F, d, F, d
        dsc.M, dsc.F, dsc.act1, dsc.dtype = M, F, act1, self.dtype
        dsc.drop_h_p, dsc.drop_h_site = drop_h
        dsc.drop_c1_p, dsc.drop_c1_site = drop_c1
        dsc.drop_c2_p, dsc.drop_c2_site = drop_c2
        dsc.gate_scale = gate_scale
        if ln is not None:                  # (gain name, output rows, statistics): norm2 in the same launch
            dsc.ln_gamma, dsc.ln_beta = self.fp.p_ptr(ln[0] + ".weight"), self.fp.p_ptr(ln[0] + ".bias")
            dsc.ln_out, dsc.ln_stats = ptr(ln[1]), ptr(ln[2])

        def work():                         # bench.py: timed like the eg_gemm_nt launches, as its own kernel (route 4)
            es = self.es
            nbytes = es * (M * d * (2 + (1 if residual and residual != A else 0)) + M * F * (1 + (1 if gate else 0)) + 2 * F * d) \
                + (M * F // 8 if (bits_out or bits_in) else 0) + 4 * (F + d) + ((es * M * d + 8 * M + 8 * d) if ln is not None else 0)
            if not H:
                nbytes = es * (2 * M * d + 2 * F * d) + 4 * (F + d) + 8 * d                           # A, norm2 rows | weights | biases, gain / bias
            flops = 4.0 * M * F * d
            if ln_tail is not None:         # dy1 itself moves only when it is stored; + x, dr, dyo, dC | W | statistics, gain, partials
                nbytes += es * (M * d * (4 - (0 if Cout else 1)) + d * d) + 8 * M + 4 * d + 8 * d * self.ln_proj_blocks
                flops += 2.0 * M * d * d
            return flops, float(nbytes), (M, F, d), 4
        probe = self._timed(work)
        if ln_tail is not None:
            call("eg_ffn_bwd_ln_proj", C.byref(dsc), C.byref(ln_tail), self.stream)
        else:
            call("eg_ffn_chain", C.byref(dsc), self.stream)
        self._timed_end(probe)

    def _probs_hook(self, drop_module, qkv, lse, kv_shift):
        """Analysis contract (5_Metrics/eeg_metrics.py:433-452): a forward hook on an attention-dropout module receives
        the probabilities [B, H, S, S] as its input, once per stream / direction in the reference's call order.  Only
        runs when such a hook is registered; the hook's return value does not feed back into the HIP path."""
        if not (drop_module._forward_hooks or drop_module._forward_pre_hooks):
            return
        NB, B, S, H = self.NB, self.B, self.S, self.cfg.num_heads
        probs = torch.empty(NB, H, S, S, device=self.device, dtype=torch.float32)
        call(self._attn_core + "_probs", ptr(qkv), ptr(lse), ptr(probs), NB, S, *self._attn_heads, kv_shift, self.dtype, self.stream)
        was = drop_module.training
        drop_module.training = False      # the module call is only the hook carrier: identity, no torch RNG use
        try:
            drop_module(probs[:B])
            drop_module(probs[B:])
        finally:
            drop_module.training = was

    def _attn_stats(self, l, qkv, lse, kv_shift):
        """Where a stage's q|k|v rows and lse are complete.  Only the inference engine reduces them (InferenceEngine.attn_stats)."""

    def _conn_stats(self):
        """Where a["ib_conn"] is complete, after any hook on ibs_matrix_generator (tokens.forward).  Only the inference engine
        reduces it (InferenceEngine.conn_stats)."""

    def ln_fwd(self, x, gname, y, stats):
        call("eg_layernorm_fwd", ptr(x), self.fp.p_ptr(gname + ".weight"), self.fp.p_ptr(gname + ".bias"), ptr(y),
             ptr(stats), self.M, self.cfg.d_model, self.dtype, self.stream)

    # ------------------------------------------------------------------------------------------
    # forward
    # ------------------------------------------------------------------------------------------
    def _forward(self, eeg1: torch.Tensor, eeg2: torch.Tensor, labels: Optional[torch.Tensor], train: bool, pack: bool = True):
        """The forward of both engines: pack, front end, layers, final norm, cross stage, heads"""
        cfg = self.cfg
        self.stream = self._cur_stream()
        p = cfg.dropout if train else 0.0
        p01 = 0.1 if train else 0.0
        self.train_flags = (p, p01, train)
        if pack:
            self.pack_params()
        x = self._front_end_fwd(eeg1, eeg2, train, p01, self.a.get("h1"))
        self._encode(x, labels, train, p)

    def _encode(self, x, labels, train: bool, p: float):
        """Token rows x -> the heads' results: layers, final norm, cross stage, heads"""
        cfg = self.cfg
        # encoder (A:292-295, 326-328), both streams batched (Siamese weights)
        for l in range(cfg.num_layers):
            x = self._layer_fwd(l, x, p)
        R = self._rows("norm", x)
        self.ln_fwd(x, "encoder.norm", R.out, R.st2)
        z = R.out
        if cfg.use_cross_attention:
            # D:966-974: both directions in one launch each (kv_shift = B pairs window b with b+B)
            R = self._rows("x", z)
            self.attn_unfused_fwd(z, "x", self.B, _layer_sites(cfg.num_layers), p, R)
            self.ln_fwd(R.r1, "cross_attn.norm", R.out, R.st1)
            z = R.out
        self._heads_fwd(z, labels, train, p)

    def _layer_fwd(self, l: int, x, p: float):
        """Encoder layer l on the rows x, by the routes: fused block or three launches, LayerNorm fused or separate, feed-forward
        chain or two GEMMs.  Returns the layer's output rows."""
        M, F, w, fp = self.M, self.cfg.d_ff, self.w, self.fp
        pre, sites, R = f"encoder.layers.{l}.", _layer_sites(l), self._rows(l, x)
        if self.attn_block:     # q|k|v projection + attention core + out-proj / dropout / residual: one launch, a workgroup per window
            self.attn_block_fwd(x, l, p, sites, R, ln=((pre + "ln1", R.y1, R.st1) if self.ln_fuse else None))
            if R.qkv is not None:
                self._probs_hook(self.model.encoder.layers[l].mha.dropout, R.qkv, R.lse, 0)
                self._attn_stats(l, R.qkv, R.lse, 0)
        else:
            self.attn_unfused_fwd(x, l, 0, sites, p, R)
        if not (self.attn_block and self.ln_fuse):
            self.ln_fwd(R.r1, pre + "ln1", R.y1, R.st1)
        if self.fuse_ffn:       # linear1 -> ReLU -> dropout -> linear2 -> dropout x2 -> + residual in one launch (A:272, A:294)
            # an engine that keeps no gate bits runs at p = 0: its descriptor names no dropout site
            drops = {} if R.gbits is None else dict(drop_h=(p, sites["ffn_a"]), drop_c1=(p, sites["ffn_b"]), drop_c2=(p, sites["drop2"]),
                                                    bits_out=ptr(R.gbits))
            self.ffn(ptr(R.y1), ptr(w[f"w1f{l}"]), ptr(w[f"w2f{l}"]), ptr(R.hff), ptr(R.r2), M, F,
                     bias1=fp.p_ptr(pre + "ffn.linear1.bias"), bias2=fp.p_ptr(pre + "ffn.linear2.bias"), act1=L.ACT_RELU,
                     residual=ptr(R.y1), ln=((pre + "ln2", R.out, R.st2) if self.ln_fuse else None), **drops)
        else:
            self.ffn_unfused_fwd(R.y1, l, R.hff, R.r2, p, sites)
        if not (self.fuse_ffn and self.ln_fuse):
            self.ln_fwd(R.r2, pre + "ln2", R.out, R.st2)
        return R.out

    def ffn_unfused_fwd(self, y1, l, hff, r2, p, sites):
        """Layer l's feed-forward pair as two launches: linear1 + ReLU + dropout, linear2 + dropout x2 + residual (A:272, A:294)"""
        M, d, F, w, fp, pre = self.M, self.cfg.d_model, self.cfg.d_ff, self.w, self.fp, f"encoder.layers.{l}."
        self.gemm(ptr(y1), ptr(w[f"w1{l}"]), ptr(hff), M, F, d, bias=fp.p_ptr(pre + "ffn.linear1.bias"),
                  act=L.ACT_RELU, drop1=(p, sites["ffn_a"]))
        self.gemm(ptr(hff), ptr(w[f"w2{l}"]), ptr(r2), M, d, F, bias=fp.p_ptr(pre + "ffn.linear2.bias"),
                  drop1=(p, sites["ffn_b"]), drop2=(p, sites["drop2"]), residual=ptr(y1))

    def _front_end_fwd(self, eeg1, eeg2, train: bool, p01: float, h1, tokenise: bool = True):
        """Input windows -> token rows a["x0"] (returned): window pack, conv-0, conv-1 (+ positions), the CLS rows and the optional
        token families.  h1: conv-1's pre-activation copy, which only the backward reads (None: not written).  tokenise=False
        leaves the matrix-form synchrony token rows unwritten (tokens.forward)."""
        cfg, d = self.cfg, self.cfg.d_model
        B, NB, S, a, w, fp, es, st = self.B, self.NB, self.S, self.a, self.w, self.fp, self.es, self.stream
        for x in (eeg1, eeg2):
            if x.dtype != torch.float32 or not x.is_contiguous() or tuple(x.shape) != (B, self.C, self.T):
                raise L.EgError(f"input windows must be contiguous f32 [{B},{self.C},{self.T}], got {tuple(x.shape)} {x.dtype}")
        aug = getattr(self.model, "augmentation", None) if train else None
        if aug is not None:
            if not isinstance(aug, WindowAugmentation):
                raise L.EgError(f"model.augmentation must be a WindowAugmentation or None, got {type(aug).__name__}")
            if aug.enabled:
                # one launch into the engine's own copy; everything below -- the pack, the token families -- reads the copy, the
                # caller's tensors are never written.  The seed is this step's (eg_step_state), so a replayed graph draws anew.
                if "aug" not in a:
                    a["aug"] = torch.empty(2, B, self.C, self.T, device=self.device, dtype=torch.float32)
                call("eg_window_augment", ptr(eeg1), ptr(eeg2), ptr(a["aug"][0]), ptr(a["aug"][1]), B, self.C, self.T,
                     float(aug.gaussian_noise_std), float(aug.channel_dropout_prob), int(aug.time_mask_num),
                     int(aug.time_mask_max_length), self.st_ptr, st)
                eeg1, eeg2 = a["aug"][0], a["aug"][1]
        for i, x in enumerate((eeg1, eeg2)):
            call("eg_window_pack", ptr(x), ptr(a["xt"]) + i * B * self.Tp * self.Cp * es, B, self.C, self.T, self.Cp,
                 self.pad, self.Tp, self.dtype, st)
        # K1: conv0 as a GEMM over overlapping channel-last rows (D:154,171)
        self.gemm(ptr(a["xt"]), ptr(w["conv0"]), ptr(a["h0pad"]) + self.pad * d * es, NB * self.T1, d, self.K0,
                  a=rowmap(self.s * self.Cp, self.Tp * self.Cp, self.T1), c=rowmap(d, self.R0 * d, self.T1),
                  bias=fp.p_ptr("temporal_conv.convs.0.bias"), act=L.ACT_RELU, drop1=(p01, SITE_CONV0))
        # K2: conv1, epilogue writes token rows [off:] of the sequence with the positional rows added (D:158,171,174; A:120-126)
        self.gemm(ptr(a["h0pad"]), ptr(w["conv1"]), ptr(a["x0"]) + self.off * d * es, NB * self.T2, d, self.k * d,
                  a=rowmap(self.s * d, self.R0 * d, self.T2), c=rowmap(d, S * d, self.T2),
                  r=rowmap(d, 0, self.T2), p=rowmap(d), bias=fp.p_ptr("temporal_conv.convs.1.bias"), act=L.ACT_RELU,
                  drop1=(p01, SITE_CONV1), residual=ptr(w["pos"]) + self.off * d * es, out_pre=ptr(h1), tag="conv1_fwd")
        # CLS rows (D:1157) + pos row 0
        call("eg_rows_bcast_f32", fp.p_ptr("cls_token"), fp.p_ptr("pos_embed.pos_embed.weight"), ptr(a["x0"]), NB, S, d, 1,
             0, 1, self.dtype, st)
        tokens.forward(self, eeg1, eeg2, train, tokenise)
        return a["x0"]

    def _heads_fwd(self, z, labels, train: bool, p: float):
        """Pooling, symmetric fusion, classifier(s) and the losses on the final token rows z (D:1193-1213)"""
        cfg, d = self.cfg, self.cfg.d_model
        B, S, a, w, fp, st = self.B, self.S, self.a, self.w, self.fp, self.stream
        self.z_final = z
        # heads (D:1193-1213)
        call("eg_pool_fuse_fwd", ptr(z), ptr(a["cls1"]), ptr(a["cls2"]), ptr(a["comb"]), ptr(a["zf"]),
             ptr(a.get("ibs_pool_f")), ptr(a.get("ibs_pool")), B, S, d, self.off, self.n_ibs, 1, self.dtype, st)
        lab = ptr(labels) if labels is not None else 0
        if self._fused_heads():     # both products, the class projection, the per-sample CE and its mean: one launch
            call("eg_heads_fwd", ptr(a["comb"]), ptr(a["zf"]), ptr(a["hcl"]), ptr(w["sf"]), fp.p_ptr("symmetric_fusion.proj.bias"),
                 ptr(w["c0"]), fp.p_ptr("classifier.0.bias"), fp.p_ptr("classifier.3.weight"), fp.p_ptr("classifier.3.bias"), lab,
                 ptr(a["logits"]), ptr(a["sloss"]), ptr(a["loss"]), ptr(a["heads_ctr"]), B, d, cfg.num_classes, p, SITE_CLS,
                 self.st_ptr, self.dtype, st)
        else:
            self.gemm(ptr(a["comb"]), ptr(w["sf"]), ptr(a["zf"]), B, d, 3 * d, c=rowmap(3 * d),
                      bias=fp.p_ptr("symmetric_fusion.proj.bias"))
            self.gemm(ptr(a["zf"]), ptr(w["c0"]), ptr(a["hcl"]), B, d, 3 * d, bias=fp.p_ptr("classifier.0.bias"),
                      act=L.ACT_RELU, drop1=(p, SITE_CLS))
            call("eg_classifier_ce_fwd", ptr(a["hcl"]), fp.p_ptr("classifier.3.weight"), fp.p_ptr("classifier.3.bias"), lab,
                 ptr(a["logits"]), ptr(a["sloss"]), ptr(a["loss"]), B, d, cfg.num_classes, self.dtype, st)
        if cfg.use_ibs:
            p3 = 0.3 if train else 0.0
            self.gemm(ptr(a["ibs_pool"]), ptr(w["i0"]), ptr(a["hib"]), B, d // 2, d, bias=fp.p_ptr("ibs_classifier.0.bias"),
                      act=L.ACT_RELU, drop1=(p3, SITE_IBSCLS))
            call("eg_classifier_ce_fwd", ptr(a["hib"]), fp.p_ptr("ibs_classifier.3.weight"), fp.p_ptr("ibs_classifier.3.bias"),
                 lab, ptr(a["ibs_logits"]), ptr(a["ibs_sloss"]), ptr(a["ibs_loss"]), B, d // 2, cfg.num_classes, self.dtype, st)
        self.labels = labels

    def _fused_heads(self, backward: bool = False) -> bool:
        """the fused head kernels cover 16-bit compute dtypes at d_model == 256 with at most 16 classes; their in-launch weight
        gradients (backward) sum at most 256 samples, and need classifier.0 / symmetric_fusion.proj each laid out as weight then
        bias in the flat gradient buffer (as eg_gemm_tn's fused-bias reduce does)"""
        ok = bool(self.fused_tail) and self.dtype != EG_F32 and self.cfg.d_model == 256 and self.cfg.num_classes <= 16
        if ok and backward:
            d = self.cfg.d_model
            ok = self.B <= 256 and all(self._packed([n], d, 3 * d) for n in ("classifier.0", "symmetric_fusion.proj"))
        return ok

# What Engine.backward decides once, before its first launch, and every stage reads:
#   p, train        dropout probability of the forward this backward belongs to, and whether that was a training forward
#   sc, sc01        1 / (1 - p) of the encoder's and the heads' dropout, of the front end's
#   seg             hears the name of each gradient segment as it completes (on_segment, or nobody)
#   grouped         the encoder's weight gradients as one grouped launch ...
#   pieced          ... cut in two pieces, the first launched after the plan's split layer
#   defer_norms     the two norms outside the layers leave their gain / bias partials to the grouped reduce
#   gx              the cross-attention block's weight gradients ride in the grouped launch
#   fused_heads     the heads' backward as three launches (_fused_heads)
#   fused_tokens    position / cls / conv-1 gradient rows from one pass over dseq
#   dY1             ungrouped route: ONE buffer for the masked gradient that enters a branch
BwdDecisions = namedtuple("BwdDecisions", "p train sc sc01 seg grouped pieced defer_norms gx has_drop fused_heads fused_tokens dY1 until")
BWD_UNTIL = (None, "spec_conv2")        # Engine.backward's `until`: the full backward, or the analysis cut


class Engine(ForwardEngine):
    """Workspace + kernel sequencing of the training step for a fixed (B, T): the shared forward over per-layer saved
    activations, the backward, gradient accumulation and the optimiser."""
    LN_PARTIAL_BLOCKS = 2048      # rows of [2, d] the LayerNorm-backward scratch partial buffer holds (g["lnpart"])
    SQ_BLOCKS = 1024              # squared-norm partials of the flat gradient buffer (g["sqpart"]) that eg_clip_coef sums
    GROUP_MIN_ROWS = 4096         # token rows below which the per-product weight-gradient launches (many splits) are the better shape
    tn_cap = 24 * 1024 * 1024     # floats (96 MB) of TN split-K partials: sized for the largest product (conv-1 weights / FFN)

    def __init__(self, model, B: int, T: int, device: torch.device, dtype: int, state_dev: Optional[torch.Tensor] = None):
        self._wg_key = self._wg_plan = None     # the grouped weight-gradient plan and the gradient buffer it was made for
        self._wg_cross, self._ln_slot = False, {}
        self._ranges_key = None
        self._acc_norm_ready = False   # g["sqpart"] holds the norm partials of the whole accumulator (accumulate(norm=True))
        super().__init__(model, B, T, device, dtype, state_dev)

    def _resolve_routes(self):
        """The forward's routes (ForwardEngine) and the backward's, from the same inputs"""
        super()._resolve_routes()
        cfg, dtype, env = self.cfg, self.dtype, os.environ
        half = dtype != EG_F32
        self.scaler_on = dtype == EG_F16 and env.get("EYEGAZE_LOSS_SCALING", "1") != "0"
        # LayerNorm backward: a block walks 8 rows per trip with TWO trips in flight (112 registers: four 256-thread blocks per CU).
        # All blocks must be resident at once -- a late block starts when an early one ends and doubles the launch -- so at most
        # 4 blocks per CU: 33 280 rows = 1024 blocks x 4.06 trips (round 2: 1040 x 4 with one trip in flight)
        env_nb = env.get("EYEGAZE_LN_BLOCKS")
        trips = max(1, self.M // 8192)
        self.LN_BLOCKS = int(env_nb) if env_nb else min(self.LN_PARTIAL_BLOCKS, 4 * self.cus,
                                                        max(1, (self.M + 8 * trips - 1) // (8 * trips)))
        if not 1 <= self.LN_BLOCKS <= self.LN_PARTIAL_BLOCKS:
            # round 2: a sweep at 2080 blocks stored past the 2048-row partial buffer (GPU memory access fault); refuse, never clamp
            raise L.EgError(f"EYEGAZE_LN_BLOCKS={env_nb} is outside [1, {self.LN_PARTIAL_BLOCKS}] (rows of the LayerNorm-backward "
                            "partial buffer)")
        self.ln_nblk_cap = max(self.LN_BLOCKS, (self.M + 63) // 64)
        # norm1's backward and out_proj's backward-data product as one launch over 80-row tiles (eg_ln_bwd_proj): bit-identical to the
        # two launches (the gain / bias partials are grouped by tile instead of by LayerNorm block: equal to fp32 rounding)
        self.ln_proj = half and cfg.d_model == 256
        self.ln_proj_blocks = L.lib().eg_ln_bwd_proj_blocks(self.M) if self.ln_proj else 0
        # the feed-forward backward launch goes on with norm1's backward and out_proj's backward-data product on the rows it has just
        # completed (eg_ffn_bwd_ln_proj): same tiles and arithmetic as the two launches, bit for bit; dy1 never reaches memory.
        # (fuse_ffn implies the gate-bit route: the forward launch of a training engine always leaves the bit image.)
        self.ffn_ln_proj = bool(self.fuse_ffn and self.ln_proj)
        # True: optimizer_step takes the gradient norm and the clip coefficient in ONE launch (eg_grad_sqnorm_clip, same bits)
        # instead of eg_grad_sqnorm + eg_clip_coef.  Off by default: tests/test_gpu_accum.py counts the trainer's eg_grad_sqnorm calls
        self.fused_norm_clip = False
        # conv-1 backward-data as one batched launch over the real rows and the non-zero taps (conv1_bwd_data); False, or
        # EYEGAZE_CONV1_BWD_BATCH=0, keeps one full launch per stride phase
        self.conv1_bwd_batch = env.get("EYEGAZE_CONV1_BWD_BATCH", "1") != "0"

    def _held(self, group, l, every: bool):
        """Every layout is allocated (tests flip routes on a live engine), but a fragment layout only where its route was on at
        construction.  Recorded are the layouts that the routes chosen now read -- the row-major q|k|v and out_proj of an encoder
        layer belong to the unfused attention route, out_proj^T to the separate backward-data product when eg_ln_bwd_proj is off,
        the four row-major feed-forward matrices to the unfused feed-forward route -- and with pack_unused = True every row-major
        one as well."""
        return [lay for lay in group if self._reads(lay, l) or (every and not lay.fused)]

    def _alloc(self):
        cfg, d, F, L_ = self.cfg, self.cfg.d_model, self.cfg.d_ff, self.cfg.num_layers
        NB, M, S, H = self.NB, self.M, self.S, self.cfg.num_heads
        f32 = torch.float32
        self.w = self._alloc_w()
        a = {"xt": self._t(NB, self.Tp, self.Cp), "h0pad": self._t(NB, self.R0, d), "h1": self._t(NB * self.T2, d), "x0": self._t(M, d)}
        rows, stats = (lambda: self._t(M, d)), (lambda: self._t(M, 2, dtype=f32))
        for l in range(L_):
            a.update({f"qkv{l}": self._t(M, 3 * d), f"lse{l}": self._t(NB, H, S, dtype=f32), f"ctx{l}": rows(), f"r1_{l}": rows(),
                      f"st1_{l}": stats(), f"y1_{l}": rows(), f"hff{l}": self._t(M, F), f"r2_{l}": rows(), f"st2_{l}": stats(),
                      f"x{l + 1}": rows()})
            if self.fuse_ffn:           # ReLU / dropout gate of the hidden rows, one bit per element (forward -> backward)
                a[f"gbits{l}"] = torch.zeros(L.gate_bits_bytes(M, F) // 8, device=self.device, dtype=torch.int64)
        a["stf"], a["zn"] = stats(), rows()
        if cfg.use_cross_attention:
            a.update(qkvx=self._t(M, 3 * d), lsex=self._t(NB, H, S, dtype=f32), ctxx=rows(), rx=rows(), stx=stats(), zc=rows())
        a.update(self._head_alloc())
        self.a = a

    def _rows(self, l, x=None) -> Rows:
        """Stage l's rows in the saved activations: an encoder layer's index, "norm" (the final norm) or "x" (the cross-attention
        block, which is an unfused layer's attention half under other names)"""
        a = self.a
        if l == "norm":
            return Rows(st2=a["stf"], out=a["zn"])
        if l == "x":
            return Rows(a["qkvx"], a["lsex"], a["ctxx"], a["rx"], a["stx"], out=a["zc"])
        return Rows(a[f"qkv{l}"], a[f"lse{l}"], a[f"ctx{l}"], a[f"r1_{l}"], a[f"st1_{l}"], a[f"y1_{l}"], a[f"hff{l}"],
                    a.get(f"gbits{l}"), a[f"r2_{l}"], a[f"st2_{l}"], a[f"x{l + 1}"])

    def forward(self, eeg1: torch.Tensor, eeg2: torch.Tensor, labels: Optional[torch.Tensor], train: bool):
        self._forward(eeg1, eeg2, labels, train)

    def _alloc_bwd(self):
        if self.g:
            return
        d, F, M, B, NB = self.cfg.d_model, self.cfg.d_ff, self.M, self.B, self.NB
        g = {}
        for n in ("dzA", "dzB", "dr", "drm", "dctx", "dy1"):
            g[n] = self._t(M, d)
        g["dqkv"] = self._t(M, 3 * d)
        g["dh"] = self._t(M, F)
        g["dzf"] = self._t(B, 3 * d)
        g["dcomb"] = self._t(B, 3 * d)
        g["dhcl"] = self._t(B, d)
        g["dlogits"] = self._t(B, self.cfg.num_classes, dtype=torch.float32)
        if self.cfg.use_ibs:
            g["dhib"] = self._t(B, d // 2)
            g["dibs_pool"] = self._t(B, d)
            g["dibs_logits"] = self._t(B, self.cfg.num_classes, dtype=torch.float32)
        g["dy1pad"] = self._t(NB, self.RY, d)
        g["dh0pad"] = self._t(NB, self.R0, d)
        g["possum"] = self._t(self.S, d, dtype=torch.float32)
        g["one"] = torch.ones(1, device=self.device, dtype=torch.float32)
        g["partial"] = self._t(self.tn_cap, dtype=torch.float32)
        g["lnpart"] = self._t(self.LN_PARTIAL_BLOCKS * 2 * max(d, 8), dtype=torch.float32)
        g["cspart"] = self._t(512 * max(3 * d, F), dtype=torch.float32)
        if self.attn_long:          # delta = rowsum(dctx * ctx) of eg_attention_long_bwd, [NB, H, S]
            g["attn_delta"] = self._t(NB * self.cfg.num_heads * self.S, dtype=torch.float32)
        self.g = g
        tokens.alloc_bwd(self)

    def check_overflow_and_update_scaler(self):
        """autograd path at fp16: flags a non-finite gradient norm (eg_step_state.found_inf) and adapts the internal loss scale,
        as the native optimiser step does between eg_clip_coef and eg_scaler_update -- without touching parameters."""
        self._alloc_bwd()
        self.stream = self._cur_stream()
        nblk, sq = self.SQ_BLOCKS, ptr(self._sqpart())
        self._acc_norm_ready = False
        call("eg_grad_sqnorm", ptr(self.fp.grad), self.fp.total, sq, nblk, self.stream)
        call("eg_clip_coef", sq, nblk, 0.0, self.st_ptr, self.stream)
        c = self.scaler_cfg
        call("eg_scaler_update", self.st_ptr, c["growth"], c["backoff"], c["growth_interval"], self.stream)

    def conv1_bwd_data(self, sc01, batch=None):
        """dh0 = conv-1's backward-data (gated by h0 > 0, scaled by sc01): stride phase ph gives rows t = u*s + ph of dh0pad
        from J taps of dy1pad.
        batch (default self.conv1_bwd_batch): the phases as ONE eg_gemm_nt_batch call that skips what the result does not
        need -- the leading tap block of a phase whose tap s*(J-1) + ph lies beyond the kernel (zeros in conv1T) and the rows
        that fall into dh0pad's pads, which nothing reads (conv-0's weight gradient starts at row `pad`; the buffer is zeroed
        once, at allocation).  False: one full launch per phase.  The real rows of dh0 are the same bits either way."""
        d, es, s, J, g, a, w = self.cfg.d_model, self.es, self.s, self.J, self.g, self.a, self.w
        NB = self.NB
        if not (self.conv1_bwd_batch if batch is None else batch):
            for ph in range(s):
                self.gemm(ptr(g["dy1pad"]), ptr(w["conv1T"]) + ph * d * J * d * es, ptr(g["dh0pad"]) + ph * d * es,
                          NB * self.U, d, J * d, a=rowmap(d, self.RY * d, self.U), c=rowmap(s * d, self.R0 * d, self.U),
                          gate=ptr(a["h0pad"]) + ph * d * es, gate_scale=sc01)
            return
        items = []
        for ph, u0, n, j0 in conv_bwd_data_phases(self.k, s, self.pad, self.T1):
            row = (u0 * s + ph) * d * es
            items.append(dict(A=ptr(g["dy1pad"]) + (u0 + j0) * d * es, W=ptr(w["conv1T"]) + (ph * d * J * d + j0 * d) * es,
                              C=ptr(g["dh0pad"]) + row, M=NB * n, N=d, K=(J - j0) * d, ldw=J * d,
                              a=rowmap(d, self.RY * d, n), c=rowmap(s * d, self.R0 * d, n),
                              gate=ptr(a["h0pad"]) + row, gate_scale=sc01))
        for i in range(0, len(items), L.GEMM_BATCH_MAX):
            self.gemm_batch(items[i:i + L.GEMM_BATCH_MAX])

    # ------------------------------------------------------------------------------------------
    # grouped weight gradients of the encoder: ONE launch for all 4*L products, ONE reduce launch
    # ------------------------------------------------------------------------------------------
    def _ln_splits(self, name: str) -> int:
        """partial rows that the backward of LayerNorm `name` leaves (eg_ln_bwd_proj's tiles for a layer's ln1, else LN_BLOCKS)"""
        return self.ln_proj_blocks if (self.ln_proj and name.endswith(".ln1")) else self.LN_BLOCKS

    def _wgrad_group_plan(self):
        """The grouped launch's tables (wgrad_plan.plan) for the current gradient buffer, or None: too few rows, or parameters
        not laid out for the fused reduces.  Allocates the per-layer dY operands and the partial buffers the tables point into."""
        fp = self.fp
        if self._wg_key == fp.grad.data_ptr():
            return self._wg_plan
        self._wg_key, self._wg_plan = fp.grad.data_ptr(), None
        cfg, d, F, M, g = self.cfg, self.cfg.d_model, self.cfg.d_ff, self.M, self.g
        lay = wgrad_plan.layout(cfg, self.dtype, self.cus, fp.offsets) if M >= self.GROUP_MIN_ROWS else None
        if lay is None:
            return None
        self._wg_cross, self._ln_slot = lay.wg_cross, lay.ln_slot
        for l in range(cfg.num_layers):
            g[f"dYo{l}"], g[f"dYf{l}"] = self._t(M, d), self._t(M, d)
            g[f"dqkv{l}"], g[f"dh{l}"] = self._t(M, 3 * d), self._t(M, F)
        if lay.wg_cross:
            g["dYo_x"], g["dqkv_x"] = self._t(M, d), self._t(M, 3 * d)
        g["wg_partial"] = self._t(lay.smax * lay.total, dtype=torch.float32)
        g["lnpart_all"] = self._t(len(lay.ln_slot) * self.ln_nblk_cap * 2 * d, dtype=torch.float32)
        addr = {}
        for _, dyn, xn, _, _, _ in lay.probs:
            addr[dyn], addr[xn] = ptr(g[dyn]), ptr(self.a[xn])
        self._wg_plan = wgrad_plan.plan(lay, cfg, addr, ptr(g["wg_partial"]), ptr(g["lnpart_all"]), ptr(fp.grad), fp.offsets,
                                        self.ln_nblk_cap, self._ln_splits, self.device)
        return self._wg_plan

    def _wgrad_group_launch(self, piece, seg, cross=False):
        """piece: None = every encoder layer in one launch; else one of `_wg_plan['pieces']` (data-parallel runs) or its
        'whole_norms'.  seg then hears which gradient buckets are complete: "cross" when the cross-attention block's products
        rode in this launch, and the piece's layers, last first."""
        pl = self._wg_plan if piece is None else piece
        call(self._wg_plan["entry"], ptr(pl["tp"]), pl["n"], pl["blocks"], self.M, pl["splits"], self.dtype, self.stream)
        call("eg_reduce_table", ptr(pl["rt"]), pl["nr"], pl["rblocks"], self.stream)
        if cross:
            seg("cross")
        for l in reversed(pl["layers"]):
            seg(f"layer{l}")

    def ln_bwd_proj(self, dy, x, stats, gname, wfrag, dx, dx_drop, dC, d1=(0.0, 0), slot=None):
        """eg_ln_bwd_proj: LayerNorm backward + the backward-data product dC = dx_drop W^T in one launch (csrc/lnproj.hip)"""
        dsc = self._ln_bwd_proj_desc(dy, x, stats, gname, wfrag, dx, dx_drop, dC, d1, slot)
        call("eg_ln_bwd_proj", C.byref(dsc), self.stream)
        if slot is None:
            self._reduce_ln_partials(dsc.partial, gname, self.ln_proj_blocks)

    def _ln_bwd_proj_desc(self, dy, x, stats, gname, wfrag, dx, dx_drop, dC, d1, slot):
        """the descriptor of eg_ln_bwd_proj; dy None: the rows come from the launch itself (eg_ffn_bwd_ln_proj)"""
        lp, cap = self._ln_partials(slot)
        dsc = L.LnBwdProjDesc()
        dsc.dy, dsc.x, dsc.stats, dsc.gamma, dsc.W_frag = ptr(dy), ptr(x), ptr(stats), self.fp.p_ptr(gname + ".weight"), ptr(wfrag)
        dsc.dx, dsc.dx_drop, dsc.dC, dsc.partial, dsc.state = ptr(dx), ptr(dx_drop), ptr(dC), lp, self.st_ptr
        dsc.M, dsc.d_model, dsc.dtype, dsc.partial_capacity_blocks = self.M, self.cfg.d_model, self.dtype, cap
        dsc.drop1_p, dsc.drop1_site = d1
        return dsc

    def ln_bwd(self, dy, x, stats, gname, dx, dx_drop=None, d1=(0.0, 0), d2=(0.0, 0), slot=None):
        """slot: index into the deferred gain/bias partial buffer (reduced by the grouped reduce at the end of backward)"""
        d = self.cfg.d_model
        lp, cap = self._ln_partials(slot)
        call("eg_layernorm_bwd", ptr(dy), ptr(x), ptr(stats), self.fp.p_ptr(gname + ".weight"), ptr(dx), ptr(dx_drop),
             lp, self.LN_BLOCKS, cap, self.M, d, self.dtype, d1[0], d1[1], d2[0], d2[1], self.st_ptr, self.stream)
        if slot is None:
            self._reduce_ln_partials(lp, gname, self.LN_BLOCKS)

    def _ln_partials(self, slot):
        """(address, rows of [2, d]) of a LayerNorm backward's gain / bias partials: the scratch buffer, or a slot of the deferred one"""
        if slot is None:
            return ptr(self.g["lnpart"]), self.LN_PARTIAL_BLOCKS
        return ptr(self.g["lnpart_all"]) + 4 * slot * self.ln_nblk_cap * 2 * self.cfg.d_model, self.ln_nblk_cap

    def _reduce_ln_partials(self, lp, gname, nblk):
        """sums the nblk rows of [gain | bias] partials at lp into the gradients of LayerNorm `gname`"""
        d, fp = self.cfg.d_model, self.fp
        if fp.offsets[gname + ".bias"] == fp.offsets[gname + ".weight"] + d:   # (gain | bias) back to back
            call("eg_reduce_partials", lp, fp.g_ptr(gname + ".weight"), 2 * d, nblk, 2 * d, 0, self.stream)
        else:
            call("eg_reduce_partials", lp, fp.g_ptr(gname + ".weight"), d, nblk, 2 * d, 0, self.stream)
            call("eg_reduce_partials", lp + 4 * d, fp.g_ptr(gname + ".bias"), d, nblk, 2 * d, 0, self.stream)

    def ln_bwd_residual(self, dy, x, stats, gname, dmasked, d1, d2=(0.0, 0), slot=None):
        """Backward of the LayerNorm behind a residual sum whose branch ends in dropout: `dmasked` receives the gradient that
        enters the branch (masked by d1 / d2); returns the buffer that holds the gradient of the residual path -- g["dr"] with
        dropout active, else `dmasked` itself (no mask: one gradient serves both)."""
        if self.train_flags[0] > 0:
            self.ln_bwd(dy, x, stats, gname, self.g["dr"], dmasked, d1=d1, d2=d2, slot=slot)
            return self.g["dr"]
        self.ln_bwd(dy, x, stats, gname, dmasked, None, slot=slot)
        return dmasked

    @staticmethod
    def _wgrad_pieces(listening: bool) -> bool:
        """Whether backward cuts the grouped weight-gradient launch in two pieces (see wgrad_plan.plan): with a gradient reducer
        listening (data parallel) it does; EYEGAZE_WGRAD_PIECES=1 forces the cut without a reducer (bit-identity tests), =0
        forbids it.  The one switch read per backward and not at construction: tests flip it on a live engine."""
        pcs = os.environ.get("EYEGAZE_WGRAD_PIECES", "")
        return pcs != "0" and (listening or pcs == "1")

    # ------------------------------------------------------------------------------------------
    # backward.  g* arguments are optional fp32 device tensors (gradients of the module's outputs);
    # gloss / gloss_ibs are 1-element fp32 device tensors (d total / d loss_ce, d total / d loss_ibs_cls).
    # Gradients land in the flat gradient buffer (overwritten, not accumulated).
    # ------------------------------------------------------------------------------------------
    def backward(self, gloss=None, gloss_ibs=None, glogits=None, gcls1=None, gcls2=None, gibs_logits=None,
                 gibs_token=None, on_segment=None, prescaled: bool = False, until: Optional[str] = None):
        """Each stage takes the gradient rows and the free row buffer and returns that pair for the next stage.
        until="spec_conv2" (the analysis backward of predict.gradcam_statistics): the same launches with the same arguments in the
        same order, cut once g["sp_d2"] -- the gradient of the spectrogram CNN's second convolution -- is complete: the grouped
        weight-gradient launch, the spectrogram projections' weight gradients and everything after eg_spec_avgpool_bwd are not
        issued.  g["sp_d2"] has the full backward's bits; the flat gradient buffer is left partly written."""
        if until not in BWD_UNTIL:
            raise L.EgError(f"backward(until={until!r}): one of {BWD_UNTIL}")
        if until is not None and not self.cfg.use_spectrogram:
            raise L.EgError("backward(until=\"spec_conv2\") needs a model with spectrogram tokens")
        self._alloc_bwd()
        self.stream = self._cur_stream()
        b = self._bwd_decisions(on_segment)._replace(until=until)
        gr = self._scale_incoming(prescaled, gloss=gloss, gloss_ibs=gloss_ibs, glogits=glogits, gcls1=gcls1, gcls2=gcls2,
                                  gibs_logits=gibs_logits, gibs_token=gibs_token)
        dz, free = self._heads_bwd(b, gr)
        if self.cfg.use_cross_attention:
            dz, free = self._cross_bwd(b, dz, free)
        dz, free = self._final_norm_bwd(b, dz, free)
        for l in reversed(range(self.cfg.num_layers)):
            dz, free = self._layer_bwd(b, l, dz, free)
        if until is None:
            self._wgrad_group_bwd(b)
            self._front_end_bwd(b, dz)
        else:       # of the front end's backward only the spectrogram branch, down to conv-2's output gradient
            tokens.backward(self, dz, until=until)

    def _bwd_decisions(self, on_segment) -> BwdDecisions:
        p, p01, train = self.train_flags
        plan = self._wgrad_group_plan()
        grouped = plan is not None
        pieced = grouped and len(plan["pieces"]) == 2 and self._wgrad_pieces(on_segment is not None)
        return BwdDecisions(
            p=p, train=train, sc=(1.0 / (1.0 - p) if p > 0 else 1.0), sc01=(1.0 / (1.0 - p01) if p01 > 0 else 1.0),
            seg=on_segment or (lambda name: None), grouped=grouped, pieced=pieced,
            # no reducer waits for the encoder.norm / cross buckets: the gain / bias partials of the two norms outside the layers
            # are summed by the grouped reduce launch at the end of backward instead of a 16-workgroup launch each
            defer_norms=grouped and not pieced and on_segment is None and plan["whole_norms"] is not None,
            gx=self.cfg.use_cross_attention and grouped and self._wg_cross, has_drop=p > 0,
            fused_heads=self._fused_heads(backward=True),
            fused_tokens=bool(self.fused_tail) and self.dtype != EG_F32 and self.cfg.d_model % 64 == 0,
            dY1=self.g["drm"] if p > 0 else self.g["dr"], until=None)

    def _scale_incoming(self, prescaled: bool, **grads):
        """every gradient entering the backward is multiplied by the device-resident loss scale (no host sync); the optimiser
        kernels divide it out again (eg_clip_coef / eg_adamw)"""
        if self.scaler_on and not prescaled:
            ls = self.loss_scale_dev
            return {k: None if t is None else t * ls for k, t in grads.items()}
        return grads

    def _heads_bwd(self, b, gr):
        """Heads and pooling: the incoming gradients -> the gradient of the final token rows, in g["dzA"]"""
        cfg, d, B, S, a, w, fp, g, st = self.cfg, self.cfg.d_model, self.B, self.S, self.a, self.w, self.fp, self.g, self.stream
        lab = ptr(self.labels) if self.labels is not None else 0
        # fused -- launch 1: CE backward rows + classifier.3's gradients; launch 2: both backward-data products chained per 16
        # samples + classifier.0's gradients; (launch 3, below: pool backward + symmetric_fusion.proj's gradients)
        call("eg_classifier_ce_bwd_fused" if b.fused_heads else "eg_classifier_ce_bwd", ptr(a["hcl"]), fp.p_ptr("classifier.3.weight"),
             ptr(a["logits"]), lab, ptr(gr["gloss"]), ptr(gr["glogits"]), ptr(g["dlogits"]), ptr(g["dhcl"]),
             fp.g_ptr("classifier.3.weight"), fp.g_ptr("classifier.3.bias"), B, d, cfg.num_classes, 1, b.sc, self.dtype, st)
        if b.fused_heads:
            call("eg_heads_bwd_chain", ptr(g["dhcl"]), ptr(w["c0T"]), ptr(w["sfT"]), ptr(a["zf"]), ptr(g["dzf"]), ptr(g["dcomb"]),
                 fp.g_ptr("classifier.0.weight"), fp.g_ptr("classifier.0.bias"), B, d, self.dtype, st)
        else:
            self.gemm(ptr(g["dhcl"]), ptr(w["c0T"]), ptr(g["dzf"]), B, 3 * d, d)
            self.wgrad(ptr(g["dhcl"]), ptr(a["zf"]), 0, B, d, 3 * d, linear=["classifier.0"])
            self.gemm(ptr(g["dzf"]), ptr(w["sfT"]), ptr(g["dcomb"]), B, 3 * d, d, a=rowmap(3 * d))
            self.wgrad(ptr(g["dzf"]), ptr(a["comb"]), 0, B, d, 3 * d, y=rowmap(3 * d), linear=["symmetric_fusion.proj"])
        dibs = None
        if cfg.use_ibs:
            sc3 = 1.0 / 0.7 if b.train else 1.0
            call("eg_classifier_ce_bwd", ptr(a["hib"]), fp.p_ptr("ibs_classifier.3.weight"), ptr(a["ibs_logits"]), lab,
                 ptr(gr["gloss_ibs"]), ptr(gr["gibs_logits"]), ptr(g["dibs_logits"]), ptr(g["dhib"]),
                 fp.g_ptr("ibs_classifier.3.weight"), fp.g_ptr("ibs_classifier.3.bias"), B, d // 2, cfg.num_classes, 1, sc3,
                 self.dtype, st)
            if w["i0T"].shape[1] != d // 2:
                raise L.EgError("ibs_classifier hidden width must be a multiple of the GEMM K-tile")
            self.gemm(ptr(g["dhib"]), ptr(w["i0T"]), ptr(g["dibs_pool"]), B, d, d // 2)
            self.wgrad(ptr(g["dhib"]), ptr(a["ibs_pool"]), 0, B, d // 2, d, linear=["ibs_classifier.0"])
            dibs = g["dibs_pool"]
        z, dz = self.z_final, g["dzA"]
        pool = (ptr(z), ptr(g["dcomb"]), ptr(g["dzf"]), ptr(gr["gcls1"]), ptr(gr["gcls2"]), ptr(dibs), ptr(gr["gibs_token"]), ptr(dz))
        if b.fused_heads:
            call("eg_heads_bwd_pool", *pool, ptr(a["comb"]), fp.g_ptr("symmetric_fusion.proj.weight"),
                 fp.g_ptr("symmetric_fusion.proj.bias"), B, S, d, self.off, self.n_ibs, 1, self.dtype, st)
        else:
            call("eg_pool_fuse_bwd", *pool, B, S, d, self.off, self.n_ibs, 1, self.dtype, st)
        b.seg("heads")
        return dz, g["dzB"]

    def _attn_stage_bwd(self, b, l, x_in, dr, drm, kv_shift, site_attn, dx_out, dqkv, defer, dctx_done=False):
        """Attention stage l backward.  dr: grad of the pre-LN sum (residual path), drm: same, masked by the branch dropout;
        defer: the stage's weight gradients ride in the grouped launch."""
        M, d, NB, S, w, g = self.M, self.cfg.d_model, self.NB, self.S, self.w, self.g
        pre, R = _attn_prefix(l), self._rows(l)
        if not defer:
            self.wgrad(ptr(drm), ptr(R.ctx), 0, M, d, d, linear=[pre + "out_proj"])
        if not dctx_done:       # (eg_ln_bwd_proj has written dctx together with dr / drm)
            self.gemm(ptr(drm), ptr(w[f"oT{l}"]), ptr(g["dctx"]), M, d, d)
        delta = (ptr(g["attn_delta"]), g["attn_delta"].numel()) if self.attn_long else ()    # (the long core's scratch)
        call(self._attn_core + "_bwd", ptr(R.qkv), ptr(R.ctx), ptr(g["dctx"]), ptr(R.lse),
             ptr(dqkv), NB, S, *self._attn_heads, kv_shift, self.dtype, b.p, site_attn, self.st_ptr, *delta, self.stream)
        if not defer:
            self.wgrad(ptr(dqkv), ptr(x_in), 0, M, 3 * d, d, linear=[pre + n for n in ("q_proj", "k_proj", "v_proj")])
        self.gemm(ptr(dqkv), ptr(w[f"qkvT{l}"]), ptr(dx_out), M, d, 3 * d, residual=ptr(dr))

    def _norm_slot(self, b, name):
        return self._ln_slot.get(name) if b.defer_norms else None

    def _cross_bwd(self, b, dz, free):
        a, g, xs = self.a, self.g, _layer_sites(self.cfg.num_layers)
        drm = g["dYo_x"] if b.gx else b.dY1      # gx: its weight gradients ride in the grouped launch
        drx = self.ln_bwd_residual(dz, a["rx"], a["stx"], "cross_attn.norm", drm, (b.p, xs["drop1"]),
                                   slot=self._norm_slot(b, "cross_attn.norm"))
        self._attn_stage_bwd(b, "x", a["zn"], drx, drm, self.B, xs["attn"], free, g["dqkv_x"] if b.gx else g["dqkv"], b.gx)
        if not b.gx:
            b.seg("cross")
        return free, dz

    def _final_norm_bwd(self, b, dz, free):
        """final encoder norm (A:328)"""
        self.ln_bwd(dz, self.a[f"x{self.cfg.num_layers}"], self.a["stf"], "encoder.norm", free, slot=self._norm_slot(b, "encoder.norm"))
        b.seg("encoder.norm")
        return free, dz

    def _layer_bwd(self, b, l, dz, free):
        M, d, F, a, w, g, p, grouped = self.M, self.cfg.d_model, self.cfg.d_ff, self.a, self.w, self.g, b.p, b.grouped
        pre, sites = f"encoder.layers.{l}.", _layer_sites(l)
        # with the grouped weight-gradient launch every layer keeps its own dY operands until the end of backward
        dYf = g[f"dYf{l}"] if grouped else b.dY1
        dYo = g[f"dYo{l}"] if grouped else b.dY1
        dh = g[f"dh{l}"] if grouped else g["dh"]
        dqkv = g[f"dqkv{l}"] if grouped else g["dqkv"]
        s2 = self._ln_slot[pre + "ln2"] if grouped else None
        s1 = self._ln_slot[pre + "ln1"] if grouped else None
        dr = self.ln_bwd_residual(dz, a[f"r2_{l}"], a[f"st2_{l}"], pre + "ln2", dYf, (p, sites["ffn_b"]), (p, sites["drop2"]),
                                  slot=s2)
        if not grouped:
            self.wgrad(ptr(dYf), ptr(a[f"hff{l}"]), 0, M, d, F, linear=[pre + "ffn.linear2"])
        tail = self.ffn_ln_proj and self.fuse_ffn and self.ln_proj
        if tail:
            # the same launch, going on with norm1's backward and out_proj's backward-data product: dy1 stays on the chip
            self.ffn(ptr(dYf), ptr(w[f"w2Tf{l}"]), ptr(w[f"w1Tf{l}"]), ptr(dh), 0, M, F, residual=ptr(dr),
                     bits_in=ptr(a[f"gbits{l}"]), gate_scale=b.sc,
                     ln_tail=self._ln_bwd_proj_desc(None, a[f"r1_{l}"], a[f"st1_{l}"], pre + "ln1", w[f"oTf{l}"], g["dr"], dYo, g["dctx"],
                                                    (p, sites["drop1"]) if b.has_drop else (0.0, 0), s1))
            if s1 is None:
                self._reduce_ln_partials(self._ln_partials(None)[0], pre + "ln1", self.ln_proj_blocks)
        elif self.fuse_ffn:
            # dH = gate(dY W2) (stored: the weight gradients read it) and dy1 = dH W1 + dr in one launch; the gate is the
            # bit image the forward launch of this layer left
            self.ffn(ptr(dYf), ptr(w[f"w2Tf{l}"]), ptr(w[f"w1Tf{l}"]), ptr(dh), ptr(g["dy1"]), M, F, residual=ptr(dr),
                     bits_in=ptr(a[f"gbits{l}"]), gate_scale=b.sc)
        else:
            self.gemm(ptr(dYf), ptr(w[f"w2T{l}"]), ptr(dh), M, F, d, gate=ptr(a[f"hff{l}"]), gate_scale=b.sc)
        if not grouped:
            self.wgrad(ptr(dh), ptr(a[f"y1_{l}"]), 0, M, F, d, linear=[pre + "ffn.linear1"])
        if not self.fuse_ffn:
            self.gemm(ptr(dh), ptr(w[f"w1T{l}"]), ptr(g["dy1"]), M, d, F, residual=ptr(dr))
        if tail:
            dr = g["dr"]
        elif self.ln_proj:      # norm1 backward + out_proj backward-data in one launch
            self.ln_bwd_proj(g["dy1"], a[f"r1_{l}"], a[f"st1_{l}"], pre + "ln1", w[f"oTf{l}"], g["dr"], dYo, g["dctx"],
                             d1=(p, sites["drop1"]) if b.has_drop else (0.0, 0), slot=s1)
            dr = g["dr"]
        else:
            dr = self.ln_bwd_residual(g["dy1"], a[f"r1_{l}"], a[f"st1_{l}"], pre + "ln1", dYo, (p, sites["drop1"]), slot=s1)
        self._attn_stage_bwd(b, l, a[f"x{l}"], dr, dYo, 0, sites["attn"], free, dqkv, grouped, dctx_done=self.ln_proj)
        if not grouped:
            b.seg(f"layer{l}")
        elif b.pieced and b.until is None and l == self._wg_plan["split_layer"]:
            # upper half of the encoder: its weight gradients are complete -> reduce them now, hand the buckets to the
            # all-reduce while the lower layers' backward-data chain keeps the compute stream busy
            self._wgrad_group_launch(self._wg_plan["pieces"][0], b.seg, b.gx)
        return free, dz

    def _wgrad_group_bwd(self, b):
        """the grouped weight-gradient launch, or the second of its two pieces, once every layer's operands are complete"""
        if b.grouped and b.pieced:
            self._wgrad_group_launch(self._wg_plan["pieces"][1], b.seg)
        elif b.grouped:
            self._wgrad_group_launch(self._wg_plan["whole_norms"] if b.defer_norms else None, b.seg, b.gx)

    def _front_end_bwd(self, b, dseq):
        """The gradient of the token rows -> positional table / cls token (A:120-126, D:1157), the token families, conv-1, conv-0"""
        d, NB, S, a, g, fp, es, st, sc01 = self.cfg.d_model, self.NB, self.S, self.a, self.g, self.fp, self.es, self.stream, b.sc01
        # conv1 backward: dY = dseq[:, off:, :] * relu/dropout gate
        ymap = rowmap(d, self.RY * d, self.T2)
        dy1 = ptr(g["dy1pad"]) + (self.J - 1) * d * es
        if b.fused_tokens:      # ONE pass over dseq: position sums, the cls_token copy and conv-1's gated dY rows
            call("eg_token_grad_tail", ptr(dseq), ptr(a["h1"]), dy1, ymap,
                 fp.g_ptr("pos_embed.pos_embed.weight"), fp.g_ptr("cls_token"), NB, S, d, self.T2, self.off, sc01, self.dtype, st)
        else:
            call("eg_batch_rowsum", ptr(dseq), fp.g_ptr("pos_embed.pos_embed.weight"), NB, S, d, S, self.dtype, st)
            call("eg_cast", fp.g_ptr("pos_embed.pos_embed.weight"), fp.g_ptr("cls_token"), d, EG_F32, st)
        tokens.backward(self, dseq)
        b.seg("tokens")         # positions, token generators, the extra heads: everything registered between conv-1 and the encoder
        if not b.fused_tokens:
            call("eg_rows_gather_gate", ptr(dseq), ptr(a["h1"]), dy1, ymap, NB, S, d,
                 self.T2, self.off, 0, sc01, self.dtype, st)
        self.wgrad(dy1, ptr(a["h0pad"]), fp.g_ptr("temporal_conv.convs.1.weight"), NB * self.T2, d, self.k * d, y=ymap,
                   x=rowmap(self.s * d, self.R0 * d, self.T2), out_b=fp.g_ptr("temporal_conv.convs.1.bias"),
                   conv=(d, self.k, d))
        b.seg("conv1")          # 6.5 MB of the front end's 7 MB: reduces under the backward-data phases and conv-0's gradient
        self.conv1_bwd_data(sc01)
        h0map = rowmap(d, self.R0 * d, self.T1)
        self.wgrad(ptr(g["dh0pad"]) + self.pad * d * es, ptr(a["xt"]), fp.g_ptr("temporal_conv.convs.0.weight"),
                   NB * self.T1, d, self.K0, y=h0map, x=rowmap(self.s * self.Cp, self.Tp * self.Cp, self.T1),
                   out_b=fp.g_ptr("temporal_conv.convs.0.bias"), conv=(self.C, self.k, self.Cp))
        b.seg("frontend")

    # ------------------------------------------------------------------------------------------
    # gradient accumulation: one optimiser step from several micro-batches (no reference counterpart: T is one batch per step)
    # ------------------------------------------------------------------------------------------
    def _sqpart(self) -> torch.Tensor:
        """squared-norm partials of the flat gradient buffer (SQ_BLOCKS floats), made on first use"""
        if "sqpart" not in self.g:
            self.g["sqpart"] = self._t(self.SQ_BLOCKS, dtype=torch.float32)
        return self.g["sqpart"]

    def bucket_ranges(self) -> Dict[str, Tuple[int, int]]:
        """ddp.bucket_ranges of this model: segment name (as backward's on_segment emits it) -> [begin, end) in floats."""
        key = self.fp.grad.data_ptr()
        if self._ranges_key != key:
            from .ddp import bucket_ranges
            fp = self.fp
            self._ranges = bucket_ranges(fp.names, fp.offsets, fp.total, self.cfg.num_layers, self.cfg.use_cross_attention)
            self._ranges_key = key
        return self._ranges

    def accumulate(self, first: bool, segment: Optional[str] = None, norm: bool = False) -> torch.Tensor:
        """Adds the flat gradient buffer (the last backward's gradients) into the model's accumulator, or overwrites the
        accumulator with it when `first` (its previous contents are then never read) -- eg_grad_accumulate, on the current stream.
        segment: one bucket of bucket_ranges() instead of the whole buffer (the data-parallel hook of the last micro-step
        accumulates each bucket as backward releases it).  norm: the same pass leaves the squared-norm partials of the NEW
        accumulator for optimizer_step(accumulated=True, norm_ready=True); whole buffer only.  Returns the accumulator."""
        self._alloc_bwd()
        self.stream = self._cur_stream()
        acc = self.fp.accumulator()
        if segment is None:
            b, e = 0, self.fp.total
        else:
            rg = self.bucket_ranges()
            if segment not in rg:
                raise L.EgError(f"accumulate: no gradient bucket named {segment!r} (have {sorted(rg)})")
            b, e = rg[segment]
            if norm:
                raise L.EgError("accumulate: the fused norm partials cover the whole buffer, not one bucket")
        sq = ptr(self._sqpart()) if norm else 0
        self._acc_norm_ready = False
        if e > b:
            call("eg_grad_accumulate", ptr(acc) + 4 * b, ptr(self.fp.grad) + 4 * b, e - b, int(bool(first)), sq,
                 self.SQ_BLOCKS if norm else 0, self.stream)
        self._acc_norm_ready = bool(norm)
        return acc

    # ------------------------------------------------------------------------------------------
    # optimiser: clip_grad_norm_(max_norm) + AdamW on the flat buffers (T:221-222)
    # ------------------------------------------------------------------------------------------
    def optimizer_step(self, m: torch.Tensor, v: torch.Tensor, max_norm: float = 1.0, betas=(0.9, 0.999), eps=1e-8,
                       weight_decay=0.01, accumulated: bool = False, norm_ready: bool = False):
        """accumulated: the gradients are the accumulator's (Engine.accumulate) instead of the last backward's.
        norm_ready: this engine's last accumulate(norm=True) has left the squared-norm partials of exactly those gradients, so
        eg_grad_sqnorm's pass over the buffer is not repeated."""
        self._alloc_bwd()
        self.stream = self._cur_stream()
        nblk, sq = self.SQ_BLOCKS, ptr(self._sqpart())
        if accumulated and self.fp.acc is None:
            raise L.EgError("optimizer_step(accumulated=True) without a preceding Engine.accumulate")
        if norm_ready and not (accumulated and self._acc_norm_ready):
            raise L.EgError("optimizer_step(norm_ready=True): no norm partials of the whole accumulator from this engine")
        grad = self.fp.acc if accumulated else self.fp.grad
        self._acc_norm_ready = False
        if norm_ready or not self.fused_norm_clip:
            if not norm_ready:
                call("eg_grad_sqnorm", ptr(grad), self.fp.total, sq, nblk, self.stream)
            call("eg_clip_coef", sq, nblk, max_norm, self.st_ptr, self.stream)
        else:       # squared-norm partials and the coefficient in one launch (the last workgroup to finish sums the partials)
            if "sq_ctr" not in self.g:
                self.g["sq_ctr"] = torch.zeros(1, device=self.device, dtype=torch.int32)
            call("eg_grad_sqnorm_clip", ptr(grad), self.fp.total, sq, nblk, max_norm, self.st_ptr,
                 ptr(self.g["sq_ctr"]), self.stream)
        call("eg_adamw", ptr(self.fp.flat), ptr(grad), ptr(m), ptr(v), self.fp.total, betas[0], betas[1], eps,
             weight_decay, self.st_ptr, self.stream)
        if self.scaler_on:      # GradScaler.update(): back off after an overflow, grow after growth_interval clean steps
            c = self.scaler_cfg
            call("eg_scaler_update", self.st_ptr, c["growth"], c["backoff"], c["growth_interval"], self.stream)


# ------------------------------------------------------------------------------------------------
# forward-only route
# ------------------------------------------------------------------------------------------------
def _inference_tensors(cfg, B: int, T: int, dtype: int):
    """The inference engine's own workspace, device-free: ({name: (shape, is fp32)}, same for the shared scratch set);
    compute-dtype tensors have is fp32 False.  InferenceEngine allocates exactly these."""
    d, F, H = cfg.d_model, cfg.d_ff, cfg.num_heads
    geo = geometry(cfg, T, dtype)
    NB, S = 2 * B, sequence_length(cfg, T)
    M = NB * S
    a = {"xt": ((NB, geo.Tp, geo.Cp), False), "h0pad": ((NB, geo.R0, d), False),
         "xa": ((M, d), False), "xb": ((M, d), False), "y1": ((M, d), False),       # layer input / output ping-pong, normed mid-layer rows
         **_head_tensors(cfg, B)}
    sc = {"qkv": ((M, 3 * d), False), "lse": ((NB, H, S), True), "ctx": ((M, d), False), "r": ((M, d), False),
          "hff": ((M, F), False), "st": ((M, 2), True)}
    return a, sc


def inference_workspace_bytes(cfg, B: int, T: int, dtype: int) -> Tuple[int, int]:
    """(with the shared scratch set, without it): bytes of the activations an InferenceEngine of this shape holds, device-free.
    Independent of num_layers.  Not counted: the packed parameters `w`, the few counter words of the fused heads, and the buffers of
    the optional token families (tokens.alloc), which are the training engine's."""
    es = 4 if dtype == EG_F32 else 2
    a, sc = _inference_tensors(cfg, B, T, dtype)

    lean, scratch = (sum(math.prod(shape) * (4 if f32 else es) for shape, f32 in tab.values()) for tab in (a, sc))
    return lean + scratch, lean


class AttnStats:
    """A request to InferenceEngine.attn_stats.  stage: "cross" or an encoder layer index; map_sum [S, S] f32 is added to, diag
    [B, S] f32 -- the current batch's rows of a caller's buffer -- is written, scratch holds at least
    _lib.attn_stats_scratch_elems(2 B, S, H) floats."""

    def __init__(self, where, map_sum: torch.Tensor, diag: torch.Tensor, scratch: torch.Tensor):
        self.stage = "x" if where == "cross" else int(where)
        self.map_sum, self.diag, self.scratch = map_sum, diag, scratch


class ConnStats:
    """A request to InferenceEngine.conn_stats.  labels [B] i64 -- the current batch's; class_sum [ncls, nbands, nfeat, C, C] f32 and
    class_count [ncls] i32 are added to; scratch holds at least _lib.ibs_class_scratch_elems(B, nbands, nfeat, C * C, ncls) floats."""

    def __init__(self, labels: torch.Tensor, class_sum: torch.Tensor, class_count: torch.Tensor, scratch: torch.Tensor):
        self.labels, self.class_sum, self.class_count, self.scratch = labels, class_sum, class_count, scratch


class InferenceEngine(ForwardEngine):
    """Forward-only engine for a fixed (B, T): predicts without saving what a backward would read.  No per-layer activations (two
    ping-pong row buffers + one for the normed mid-layer rows), no backward workspace, no backward weight layouts -- _held's one
    rule (no `bwd`, no `fused`) over every stage of LAYOUTS, the token families' among them -- always p = 0, and
    it neither reads nor writes the model's step state, forward counter or seeds.  Where a layer half has a lean launch
    (eg_attn_block_fwd / eg_ffn_chain with only ln_out stored) it takes it; every other launch is the training engine's, writing
    into ONE shared scratch set allocated on first need.  Same bits as Engine.forward(train=False)."""
    TRAINING_CALLS = ("backward", "accumulate", "optimizer_step", "set_state", "check_overflow_and_update_scaler")

    def _init_state(self, state_dev):
        # a private all-zero state that no launch writes: at p = 0 no kernel reads a seed, and eg_set_step_state is never called
        self.state_dev = torch.zeros(L.STATE_WORDS, dtype=torch.int32, device=self.device)

    def _held(self, group, l, every: bool):
        """Only what the forward reads: each forward layout, or in its place the fragment layout that the fused route reads instead"""
        return [lay if self._reads(lay, l) else _FUSED_TWIN[lay.key] for lay in group if not (lay.bwd or lay.fused)]

    def _alloc(self):
        self.w = self._alloc_w()
        shapes, self._sc_shapes = _inference_tensors(self.cfg, self.B, self.T, self.dtype)
        a = {n: self._t(*shape, dtype=(torch.float32 if is32 else None)) for n, (shape, is32) in shapes.items()}
        a["x0"] = a["xa"]                                  # the front end and the token families write the token rows here
        a["heads_ctr"] = _heads_counters(self.B, self.device)
        self.a = a
        self.sc = {}                                       # the shared scratch set: qkv, lse, ctx, r, hff, st -- see _scratch
        self.routes_taken = []                             # (layer, "attn" | "ffn", "lean" | "scratch") of the last forward
        self.attn_stats: Optional[AttnStats] = None        # a plain attribute: the stage whose probabilities the next forwards reduce
        self.conn_stats: Optional[ConnStats] = None        # likewise: where the next forwards add their connectivity matrices

    def _scratch(self, name: str) -> torch.Tensor:
        if name not in self.sc:
            shape, is32 = self._sc_shapes[name]
            self.sc[name] = self._t(*shape, dtype=(torch.float32 if is32 else None))
        return self.sc[name]

    def _rows(self, l, x) -> Rows:
        """Stage l's rows: the output goes to the one of the ping-pong pair that x is not (the pair also serves the final norm and
        the cross-attention stage), the normed mid-layer rows to y1, and everything else either nowhere -- the lean launch: fused
        block, LayerNorm fused, no hook on that layer / feed-forward chain, LayerNorm fused -- or into the shared scratch set."""
        a, s = self.a, self._scratch
        out = a["xb"] if x is a["xa"] else a["xa"]
        if l == "norm":
            return Rows(st2=s("st"), out=out)
        if l == "x":
            return Rows(s("qkv"), s("lse"), s("ctx"), s("r"), s("st"), out=out)
        drop = self.model.encoder.layers[l].mha.dropout
        wanted = drop._forward_hooks or drop._forward_pre_hooks or (self.attn_stats is not None and self.attn_stats.stage == l)
        lean_attn = self.attn_block and self.ln_fuse and not wanted
        lean_ffn = self.fuse_ffn and self.ln_fuse
        self.routes_taken += [(l, "attn", "lean" if lean_attn else "scratch"), (l, "ffn", "lean" if lean_ffn else "scratch")]
        attn = (None,) * 5 if lean_attn else (s("qkv"), s("lse"), s("ctx"), s("r"), s("st"))
        ffn = (None,) * 4 if lean_ffn else (s("hff"), None, s("r"), s("st"))
        return Rows(*attn, a["y1"], *ffn, out)

    def _attn_stats(self, l, qkv, lse, kv_shift):
        """eg_attention_stats on the requested stage: the batch's mean-over-heads-and-directions map added into map_sum, its
        per-sample diagonals written to diag -- from q|k|v and lse, no [NB, H, S, S] tensor (predict.attention_statistics)"""
        st = self.attn_stats
        if st is None or st.stage != l:
            return
        for name, t, shape in (("map_sum", st.map_sum, (self.S, self.S)), ("diag", st.diag, (self.B, self.S))):
            if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != qkv.device:
                raise L.EgError(f"attn_stats.{name} must be a contiguous f32 {list(shape)} tensor on {qkv.device}")
        call("eg_attention_stats", ptr(qkv), ptr(lse), ptr(st.map_sum), ptr(st.diag), ptr(st.scratch), st.scratch.numel(),
             self.NB, self.S, self.cfg.num_heads, self.head_dim, kv_shift, self.dtype, self.stream)

    def _conn_stats(self):
        """eg_ibs_class_accumulate on the batch's matrices: per-class sums and counts added into the request's tensors, no
        [N, ..., C, C] tensor anywhere (predict.connectivity_statistics)"""
        st = self.conn_stats
        if st is None:
            return
        conn, nf = self.a["ib_conn"], self.cfg.num_ibs_features
        ncls = st.class_count.numel()
        for name, t, shape, dt in (("labels", st.labels, (self.B,), torch.int64),
                                   ("class_sum", st.class_sum, (ncls, self.ib["nb"], nf, self.C, self.C), torch.float32),
                                   ("class_count", st.class_count, (ncls,), torch.int32)):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != conn.device:
                raise L.EgError(f"conn_stats.{name} must be a contiguous {dt} {list(shape)} tensor on {conn.device}")
        if st.scratch.dtype != torch.float32 or not st.scratch.is_contiguous() or st.scratch.device != conn.device:
            raise L.EgError(f"conn_stats.scratch must be a contiguous f32 tensor on {conn.device}")
        call("eg_ibs_class_accumulate", ptr(conn), ptr(self.a["ib_fidx"]), ptr(st.labels), ptr(st.class_sum), ptr(st.class_count),
             ptr(st.scratch), st.scratch.numel(), self.B, self.ib["nb"], nf, self.C * self.C, ncls, self.stream)

    def forward(self, eeg1: torch.Tensor, eeg2: torch.Tensor, labels: Optional[torch.Tensor] = None, pack: bool = True):
        """pack=False: the packed weights of an earlier call still hold (a caller walking many batches packs once)"""
        self.routes_taken = []
        self._forward(eeg1, eeg2, labels, False, pack=pack or self._plan_key is None)

    def forward_band_masks(self, eeg1: torch.Tensor, eeg2: torch.Tensor, bands, each, pack: bool = True):
        """One forward per entry of `bands` -- None: the plain model; an int b: the model with band b of the connectivity matrices
        zeroed, what eeg_metrics.py's FrequencyMaskHook causes -- sharing everything the mask does not touch: the front end, the
        spectrogram tokens, eg_ibs_analytic / eg_ibs_pairs, the hook dispatch and the conn_stats reduction run once; per entry
        run the tokeniser (eg_ibs_inorm_band, no xhat), the layers, the final norm, the cross stage and the heads, then each(i)
        is called and reads a["logits"].  The front end writes the token rows into one more [NB, S, d] buffer (allocated on first
        need), which no layer overwrites: _rows sends layer 0's output to xa.  A model without matrix-form synchrony tokens has
        nothing to mask (the reference registers no hook then): one plain forward, whose logits serve every entry."""
        cfg = self.cfg
        bands = list(bands)
        if not (cfg.use_ibs and cfg.use_robust_ibs):
            self.forward(eeg1, eeg2, None, pack=pack)
            for i in range(len(bands)):
                each(i)
            return
        for b in bands:
            if b is not None and not (isinstance(b, int) and 0 <= b < self.ib["nb"]):
                raise L.EgError(f"forward_band_masks: a band is None or an int in [0, {self.ib['nb']}), got {b!r}")
        self.routes_taken = []
        self.stream = self._cur_stream()
        self.train_flags = (0.0, 0.0, False)
        if pack or self._plan_key is None:
            self.pack_params()
        a = self.a
        if "xf" not in self.sc:
            self.sc["xf"] = self._t(self.M, cfg.d_model)
        a["x0"] = self.sc["xf"]
        try:
            x = self._front_end_fwd(eeg1, eeg2, False, 0.0, None, tokenise=False)
            for i, b in enumerate(bands):
                tokens.ibs_tokens(self, False, zero_band=-1 if b is None else b)
                self._encode(x, None, False, 0.0)
                each(i)
        finally:
            a["x0"] = a["xa"]


def _refused(name: str):
    def method(self, *a, **k):
        raise L.EgError(f"{name}() on an inference engine: it keeps no activations and has no backward workspace "
                        "(use DualEEGTransformer.forward / Engine for training)")
    return method


for _name in InferenceEngine.TRAINING_CALLS:
    setattr(InferenceEngine, _name, _refused(_name))
