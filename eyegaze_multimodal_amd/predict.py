"""Running a trained model over whole datasets (the reference's evaluate() loop, T:258-314, and the re-built models of
analyze_eeg.py / eeg_metrics.py): DualEEGTransformer.predict's forward-only engine batch by batch, with the per-batch tail --
argmax, confusion matrix, loss sum -- kept on the device (eg_eval_accumulate), so that the host syncs once, at the end.
attention_statistics is eeg_metrics.py's extract_attention_weights (:465-594) over the same walk: the mean attention map and the
per-sample diagonals reduced on the device from each batch's q|k|v rows (eg_attention_stats), never a [B, H, S, S] tensor.

predict_loader walks a data.ResidentWindows store instead (--resident: gather launch -> engine, no window visits the host), and
predict_recording classifies one whole recording pair at any stride.  connectivity_statistics and
frequency_sensitivity are eeg_metrics.py's class-mean connectivity matrices (:183-311) and band-masking sensitivity (:318-413)
with the matrices consumed where eg_ibs_pairs leaves them.  gradcam_statistics is compute_gradcam_batch (:811-953):
an eval forward of the training engine, the backward cut at the spectrogram CNN's second convolution and ONE eg_gradcam_accumulate
per batch -- no activation or gradient of that layer visits the host; embedding_features is
extract_features_for_embedding (:602-673) over the inference engine, and embedding_maps turns its features into the t-SNE maps of
run_embedding_analysis (analyze_eeg.py:560-640) on the device (embedding.py).

    python -m eyegaze_multimodal_amd.predict --config CONFIG.yaml --checkpoint best_model.pt --out FILE.npz [--resident]
                                             [--recording-preprocessing] (raw recordings; needs --resident)
                                             [--attention-stats [cross|LAYER]] [--connectivity-stats]
                                             [--frequency-sensitivity] [--gradcam [--gradcam-max-samples N]]
                                             [--embedding DIR [--embedding-max-samples N]]
"""
from __future__ import annotations

import argparse
from pathlib import Path
from typing import Any, Dict, Optional

import numpy as np
import torch

from ._lib import EgError, attn_stats_scratch_elems, call, gradcam_scratch_elems, ptr


class _PredictWalk:
    """The per-batch body and the result of a prediction walk, whichever way its batches arrive: forward on the inference engine
    (weights packed once per engine), logits kept, argmax / confusion matrix / loss sum on the device (eg_eval_accumulate)."""

    def __init__(self, model, N: int, with_labels: bool):
        self.model, self.N, ncls = model, N, model.cfg.num_classes
        self.dev = dev = next(model.parameters()).device
        self.logits = torch.empty(N, ncls, device=dev)
        self.pred = torch.empty(N, device=dev, dtype=torch.int32)
        self.cm = torch.zeros(ncls, ncls, device=dev, dtype=torch.int32) if with_labels else None
        self.loss_sum = torch.zeros(1, device=dev) if with_labels else None
        self.packed, self.nb, self.i = set(), 0, 0

    def batch(self, eeg1, eeg2, labels):
        """the next batch: device tensors [B, C, T], labels [B] or None; fills rows [i, i + B) of the walk"""
        model, i = self.model, self.i
        x1, x2, y = model._check_windows(eeg1, eeg2, labels)
        B, ncls = x1.shape[0], model.cfg.num_classes
        eng = model.inference_engine(B, x1.shape[2], self.dev)
        eng.forward(x1, x2, y, pack=id(eng) not in self.packed)
        self.packed.add(id(eng))
        self.logits[i:i + B].copy_(eng.a["logits"])
        call("eg_eval_accumulate", ptr(eng.a["logits"]), ptr(y), ptr(eng.a["loss"]) if y is not None else 0,
             self.pred.data_ptr() + 4 * i, ptr(self.cm), ptr(self.loss_sum), B, ncls, eng.stream)
        self.nb += 1
        self.i += B

    def result(self) -> Dict[str, Any]:
        from .train_art import macro_metrics_from_confusion
        out = {"logits": self.logits, "predictions": self.pred.long()}
        if self.cm is not None:
            out["confusion"] = self.cm.cpu().numpy()                 # the one host sync
            out["loss"] = float(self.loss_sum) / self.nb
            out["metrics"] = macro_metrics_from_confusion(out["confusion"])
        return out


@torch.no_grad()
def predict_windows(model, eeg1: torch.Tensor, eeg2: torch.Tensor, labels: Optional[torch.Tensor] = None,
                    batch_size: int = 256) -> Dict[str, Any]:
    """eeg1, eeg2: f32 [N, C, T] in device memory or (pinned) host memory; labels: [N] or None.  Walks the windows in batches of
    batch_size (the ragged tail as a batch of its own shape), packs the weights once per engine, and returns
      logits [N, ncls] f32 and predictions [N] i64 (device tensors), and with labels also
      confusion [ncls, ncls] (numpy, [true][predicted]), loss (mean of the batches' cross-entropy means, as Trainer.evaluate
      reports it) and metrics (train_art.macro_metrics_from_confusion)."""
    N = eeg1.shape[0]
    if batch_size < 1 or N < 1:
        raise ValueError(f"predict_windows needs N >= 1 windows and batch_size >= 1 (got {N}, {batch_size})")
    walk = _PredictWalk(model, N, labels is not None)
    for i in range(0, N, batch_size):
        up = lambda t: None if t is None else t[i:i + batch_size].to(walk.dev, non_blocking=True)
        walk.batch(up(eeg1), up(eeg2), up(labels))
    return walk.result()


@torch.no_grad()
def predict_loader(model, loader) -> Dict[str, Any]:
    """predict_windows over a loader's device batches (data.ResidentWindows: each batch goes from the gather launch straight into
    the inference engine, nothing crosses the host).  Returns predict_windows' dict plus labels [N] i64 (device)."""
    if loader.n < 1:
        raise ValueError("predict_loader needs at least one window")
    N = len(loader._order()) if not loader.drop_last else len(loader) * loader.B
    walk = _PredictWalk(model, N, True)
    labels = torch.empty(N, device=walk.dev, dtype=torch.int64)
    for b in loader:
        labels[walk.i:walk.i + b["labels"].shape[0]].copy_(b["labels"])
        walk.batch(b["eeg1"], b["eeg2"], b["labels"])
    return {**walk.result(), "labels": labels}


def majority_vote(predictions, num_classes: int) -> int:
    """the class most windows predict; a tie goes to the lowest class id"""
    counts = np.bincount(np.asarray(predictions, dtype=np.int64).reshape(-1), minlength=num_classes)
    return int(np.argmax(counts))            # argmax returns the first of equal maxima


def recording_starts(length: int, window: int, stride: int) -> np.ndarray:
    """window starts i * stride of a recording of `length` samples; the tail shorter than a window is dropped, as the
    reference's enumeration drops it (dual_eeg_dataset.py:62-120)"""
    if stride < 1 or window < 1:
        raise ValueError(f"window={window} and stride={stride} must be >= 1")
    return np.arange(0 if length < window else (length - window) // stride + 1, dtype=np.int64) * stride


@torch.no_grad()
def predict_recording(model, rec1, rec2, stride: Optional[int] = None, batch_size: int = 256,
                      preprocessing: bool = False, recording_preprocessing=None) -> Dict[str, Any]:
    """Classifies a whole recording pair at any stride.  rec1, rec2: (C, L) arrays or tensors (the shorter length and the smaller
    channel count count); the window length is the one model.cfg implies (4 * max_len), stride defaults to it.  The pair is
    uploaded once as a one-pair recording store; every batch is cut and normalised on the device (eg_window_gather) and goes
    straight into the inference engine.  Returns starts [n] (numpy i64), logits [n, ncls] f32 and predictions [n] i64 (device
    tensors) and vote (majority_vote of the predictions).
    recording_preprocessing = {sampling_rate, filter_low, filter_high}: for RAW recordings -- each player's recording goes whole
    through data.preprocess_recordings (band-pass, CAR over the channels that count, z-score) before the pair is cut to the
    common length, and the windows are cut as stored (eg_window_cut); it excludes preprocessing=True."""
    from .data import DeviceRecordings, preprocess_recordings, recording_preprocessing_args, validate_store
    prep = recording_preprocessing_args(recording_preprocessing) if recording_preprocessing is not None else None
    if prep is not None and preprocessing:
        raise ValueError("predict_recording: recording_preprocessing already normalises; preprocessing=True would do it twice")
    dev = next(model.parameters()).device
    T = 4 * model.cfg.max_len
    stride = T if stride is None else int(stride)
    r1, r2 = (torch.as_tensor(np.asarray(r) if not torch.is_tensor(r) else r, dtype=torch.float32) for r in (rec1, rec2))
    if r1.dim() != 2 or r2.dim() != 2:
        raise ValueError(f"predict_recording needs (C, L) recordings, got {tuple(r1.shape)} and {tuple(r2.shape)}")
    C, L = min(r1.shape[0], r2.shape[0]), min(r1.shape[1], r2.shape[1])
    starts = recording_starts(L, T, stride)
    n = len(starts)
    if n < 1 or batch_size < 1:
        raise ValueError(f"predict_recording: recordings of {L} samples hold no window of {T} (batch_size {batch_size})")
    validate_store({"channels": C, "window_size": T, "count": n, "pairs": [{"offset": 0, "length": L}],
                    "window_pair": [0] * n, "windows": [{"start": int(s)} for s in starts]}, 2 * C * L)
    if prep is not None:
        r1, r2 = preprocess_recordings([r1[:C], r2[:C]], device=dev, **prep)
    data = torch.stack([r1[:C, :L], r2[:C, :L]]).to(dev).contiguous().reshape(-1)
    store = DeviceRecordings(data, [0], [L], np.zeros(n, np.int32), starts, None, C, T)
    order = torch.arange(n, dtype=torch.int32, device=dev)
    walk = _PredictWalk(model, n, False)
    mode = 2 if prep is not None else 1 if preprocessing else 0
    for i in range(0, n, batch_size):
        x1, x2, _ = store.gather(order, i, min(batch_size, n - i), mode)
        walk.batch(x1, x2, None)
    out = walk.result()
    return {"starts": starts, **out, "vote": majority_vote(out["predictions"].cpu().numpy(), model.cfg.num_classes)}


CLASS_NAMES = ["Single", "Competition", "Cooperation"]          # eeg_metrics.py:558


@torch.no_grad()
def attention_statistics(model, eeg1: torch.Tensor, eeg2: torch.Tensor, labels: torch.Tensor, batch_size: int = 256,
                         max_samples: Optional[int] = 200, where="cross", class_names=None) -> Dict[str, Any]:
    """extract_attention_weights (eeg_metrics.py:465-594) without the probabilities: windows and batches as predict_windows;
    where: "cross" (the reference's cross_attn.cross_attn.dropout) or an encoder layer index (that layer's self-attention, the two
    streams in place of the two directions).  max_samples is tested before each batch, as the reference does, so the n windows
    that count are whole batches (None: all).  Returns, under the reference's keys,
      mean_map [S, S] f32 numpy: mean over the n samples of the mean over heads and the two directions;
      diagonal_stats {class name: {mean_diagonal_vector [S], mean_diagonal_value, count}} for the classes that occurred;
    and diagonals [n, S] (numpy, every sample's diagonal of its own map), count = n, logits [n, ncls] f32 and predictions [n]
    i64 (device tensors, the bits of model.predict).  A model without cross attention and where="cross": {} (the reference warns
    and returns {}).  map_sum and the diagonals stay on the device for the whole walk; the host syncs once, at the end."""
    from .engine import AttnStats
    cfg = model.cfg
    if where == "cross":
        if not cfg.use_cross_attention:
            return {}
    elif not (isinstance(where, int) and 0 <= where < cfg.num_layers):
        raise ValueError(f"where must be \"cross\" or an encoder layer index below {cfg.num_layers}, got {where!r}")
    N, ncls = eeg1.shape[0], cfg.num_classes
    if batch_size < 1 or N < 1 or labels is None or labels.shape[0] != N or (max_samples is not None and max_samples < 1):
        raise ValueError(f"attention_statistics needs N >= 1 labelled windows, batch_size >= 1 and max_samples >= 1 or None "
                         f"(got {N}, {batch_size}, {max_samples})")
    n = N if max_samples is None else min(N, -(-max_samples // batch_size) * batch_size)
    dev = next(model.parameters()).device
    logits = torch.empty(n, ncls, device=dev)
    pred = torch.empty(n, device=dev, dtype=torch.int32)
    map_sum = diags = None
    packed, scratch = set(), {}
    for i in range(0, n, batch_size):
        up = lambda t: t[i:min(i + batch_size, n)].to(dev, non_blocking=True)
        x1, x2, _ = model._check_windows(up(eeg1), up(eeg2), None)
        B = x1.shape[0]
        eng = model.inference_engine(B, x1.shape[2], dev)
        if map_sum is None:
            map_sum = torch.zeros(eng.S, eng.S, device=dev)
            diags = torch.empty(n, eng.S, device=dev)
        if id(eng) not in scratch:
            need = attn_stats_scratch_elems(eng.NB, eng.S, cfg.num_heads)
            if need < 0:
                raise EgError(f"eg_attention_stats does not cover NB={eng.NB} S={eng.S} H={cfg.num_heads}")
            scratch[id(eng)] = torch.empty(need, device=dev)
        eng.attn_stats = AttnStats(where, map_sum, diags[i:i + B], scratch[id(eng)])
        try:
            eng.forward(x1, x2, None, pack=id(eng) not in packed)
        finally:
            eng.attn_stats = None           # the engine is model.predict's too: its next forward takes the lean routes again
        packed.add(id(eng))
        logits[i:i + B].copy_(eng.a["logits"])
        call("eg_eval_accumulate", ptr(eng.a["logits"]), 0, 0, pred.data_ptr() + 4 * i, 0, 0, B, ncls, eng.stream)
    d = diags.cpu().numpy()                                      # the one host sync
    y = labels[:n].cpu().numpy().astype(np.int64)
    names = CLASS_NAMES if class_names is None else list(class_names)
    stats = {}
    for c in dict.fromkeys(y.tolist()):                          # first-occurrence order, as the reference's defaultdict
        v = d[y == c].mean(axis=0)
        stats[names[c] if 0 <= c < len(names) else str(c)] = {"mean_diagonal_vector": v, "mean_diagonal_value": v.mean(),
                                                             "count": int((y == c).sum())}
    return {"mean_map": (map_sum / n).cpu().numpy(), "diagonal_stats": stats, "diagonals": d, "count": n, "logits": logits,
            "predictions": pred.long()}


BAND_NAMES = ["broadband", "delta", "theta", "alpha", "beta", "gamma"]      # eeg_metrics.py:372


@torch.no_grad()
def connectivity_statistics(model, eeg1: torch.Tensor, eeg2: torch.Tensor, labels: torch.Tensor, batch_size: int = 256,
                            max_samples: Optional[int] = None, class_names=None) -> Dict[str, Any]:
    """extract_ibs_matrices -> compute_mean_ibs_by_class -> compute_ibs_difference (eeg_metrics.py:183-311) without the per-sample
    matrices: windows, batches and the whole-batch rule of max_samples as attention_statistics; every batch's [B, 6, nfeat, C, C]
    matrices -- after any forward hook on model.ibs_matrix_generator -- are added per class on the device
    (eg_ibs_class_accumulate), the host syncs once, at the end.  Returns
      class_mean {class name: [nbands, nfeat, C, C] f32 numpy} for every name (zeros for a class that never occurred),
      class_count {class name: int}, difference (Cooperation - Competition, when both names exist), count = n,
      logits [n, ncls] f32 and predictions [n] i64 (device tensors, the bits of model.predict).
    A model without matrix-form synchrony tokens: {} (the reference warns and captures nothing)."""
    from .engine import ConnStats
    from ._lib import ibs_class_scratch_elems
    cfg = model.cfg
    N, ncls = eeg1.shape[0], cfg.num_classes
    if batch_size < 1 or N < 1 or labels is None or labels.shape[0] != N or (max_samples is not None and max_samples < 1):
        raise ValueError(f"connectivity_statistics needs N >= 1 labelled windows, batch_size >= 1 and max_samples >= 1 or None "
                         f"(got {N}, {batch_size}, {max_samples})")
    if not (cfg.use_ibs and cfg.use_robust_ibs):
        return {}
    names = CLASS_NAMES if class_names is None else list(class_names)
    if not 1 <= len(names) <= 16:
        raise ValueError(f"connectivity_statistics serves 1 to 16 class names, got {len(names)}")
    n = N if max_samples is None else min(N, -(-max_samples // batch_size) * batch_size)
    dev = next(model.parameters()).device
    logits = torch.empty(n, ncls, device=dev)
    pred = torch.empty(n, device=dev, dtype=torch.int32)
    class_sum = None
    class_count = torch.zeros(len(names), device=dev, dtype=torch.int32)
    packed, scratch = set(), {}
    for i in range(0, n, batch_size):
        up = lambda t: t[i:min(i + batch_size, n)].to(dev, non_blocking=True)
        x1, x2, y = model._check_windows(up(eeg1), up(eeg2), up(labels))
        B = x1.shape[0]
        eng = model.inference_engine(B, x1.shape[2], dev)
        nb, nf, Cn = eng.ib["nb"], cfg.num_ibs_features, eng.C
        if class_sum is None:
            class_sum = torch.zeros(len(names), nb, nf, Cn, Cn, device=dev)
        if id(eng) not in scratch:
            need = ibs_class_scratch_elems(B, nb, nf, Cn * Cn, len(names))
            if need < 0:
                raise EgError(f"eg_ibs_class_accumulate does not cover B={B} nbands={nb} nfeat={nf} C={Cn} ncls={len(names)}")
            scratch[id(eng)] = torch.empty(need, device=dev)
        eng.conn_stats = ConnStats(y, class_sum, class_count, scratch[id(eng)])
        try:
            eng.forward(x1, x2, None, pack=id(eng) not in packed)
        finally:
            eng.conn_stats = None           # the engine is model.predict's too
        packed.add(id(eng))
        logits[i:i + B].copy_(eng.a["logits"])
        call("eg_eval_accumulate", ptr(eng.a["logits"]), 0, 0, pred.data_ptr() + 4 * i, 0, 0, B, ncls, eng.stream)
    counts = class_count.cpu().numpy()                           # the one host sync
    mean = (class_sum / class_count.clamp(min=1).float().view(-1, 1, 1, 1, 1)).cpu().numpy()
    out = {"class_mean": {name: mean[c] for c, name in enumerate(names)},
           "class_count": {name: int(counts[c]) for c, name in enumerate(names)}, "count": n, "logits": logits,
           "predictions": pred.long()}
    if "Cooperation" in names and "Competition" in names:
        out["difference"] = mean[names.index("Cooperation")] - mean[names.index("Competition")]
    return out


GRADCAM_TARGETS = ("predicted", "label")
GRADCAM_SIZE = 64                                               # eeg_metrics.py:930: every map is resized to 64 x 64


def _gradcam_batch(model, eng, x1, x2, y, target, cams, class_sum, class_count, scratch, ncls_names):
    """One batch of gradcam_statistics on the training engine `eng`: eval forward, analysis backward from the one-hot of the chosen
    logit, one eg_gradcam_accumulate.  cams: this batch's rows [B, 64, 64].  Returns the batch's logits (a copy)."""
    ncls = model.cfg.num_classes
    # the bookkeeping of every forward of the training engines: the forward counter moves, so the backward of an older autograd
    # forward is refused ("newer forward") instead of reading this batch's activations
    logits = model._run_forward(eng, x1, x2, None, train=False)["logits"]
    idx = logits.argmax(dim=1) if target == "predicted" else y
    one_hot = (idx.view(-1, 1) == torch.arange(ncls, device=logits.device).view(1, -1)).float()      # on the device, no host sync
    eng.backward(glogits=one_hot, until="spec_conv2")           # fp16: scaled by the device-resident loss scale as any backward
    sp, fp, pre = eng.sp, eng.fp, "spectrogram_generator.spec_conv.3."
    call("eg_gradcam_accumulate", ptr(eng.a["sp_p1"]), ptr(eng.g["sp_d2"]), fp.p_ptr(pre + "weight"), fp.p_ptr(pre + "bias"),
         ptr(eng.loss_scale_dev) if eng.scaler_on else 0, ptr(y), ptr(cams), ptr(class_sum), ptr(class_count), ptr(scratch),
         scratch.numel(), eng.B, eng.C, sp["Hp"], sp["Wp"], ncls_names, eng.dtype, eng.stream)
    return logits


@torch.no_grad()
def gradcam_statistics(model, eeg1: torch.Tensor, eeg2: torch.Tensor, labels: torch.Tensor, batch_size: int = 256,
                       max_samples: Optional[int] = 100, target: str = "predicted", class_names=None) -> Dict[str, Any]:
    """compute_gradcam_batch (eeg_metrics.py:811-953) without the hooks: eval mode, score = the sum over the batch of each sample's
    chosen logit -- target "predicted" (the reference's choice: the argmax) or "label" (the alternative its comment names) --,
    Grad-CAM of spectrogram_generator.spec_conv[3] per image, the mean over the channels and the two streams, resized to 64 x 64,
    bucketed by the TRUE label.  Windows, batches and the whole-batch rule of max_samples as attention_statistics; class buckets
    as connectivity_statistics.  Returns
      class_mean {class name: [64, 64] f32 numpy} for every name (zeros for a class that never occurred), class_count {name: int},
      cams [n, 64, 64] f32 (device, one map per sample), count = n, logits [n, ncls] f32 and predictions [n] i64 (device).
    A model without spectrogram tokens: {} (the reference prints an error and returns {}).
    Every batch runs the TRAINING engine of its shape (the inference engine keeps no activations): an eval forward, the backward
    cut once the gradient of that layer's output is complete (Engine.backward(until="spec_conv2")) and one eg_gradcam_accumulate;
    cams, the class sums and counts stay on the device, the host syncs once, at the end.  No parameter, p.grad, optimiser state,
    step state or loss-scaler state is written, but the flat gradient buffer's contents are unspecified afterwards: a call
    between a native backward and its optimiser step loses that backward.  An autograd backward of a forward made before the
    call is refused (the engine keeps one step's activations)."""
    cfg = model.cfg
    N, ncls = eeg1.shape[0], cfg.num_classes
    if batch_size < 1 or N < 1 or labels is None or labels.shape[0] != N or (max_samples is not None and max_samples < 1):
        raise ValueError(f"gradcam_statistics needs N >= 1 labelled windows, batch_size >= 1 and max_samples >= 1 or None "
                         f"(got {N}, {batch_size}, {max_samples})")
    if target not in GRADCAM_TARGETS:
        raise ValueError(f"target must be one of {GRADCAM_TARGETS}, got {target!r}")
    if not cfg.use_spectrogram:
        return {}
    names = CLASS_NAMES if class_names is None else list(class_names)
    if not 1 <= len(names) <= 16:
        raise ValueError(f"gradcam_statistics serves 1 to 16 class names, got {len(names)}")
    n = N if max_samples is None else min(N, -(-max_samples // batch_size) * batch_size)
    dev = next(model.parameters()).device
    G = GRADCAM_SIZE
    logits = torch.empty(n, ncls, device=dev)
    pred = torch.empty(n, device=dev, dtype=torch.int32)
    cams = torch.empty(n, G, G, device=dev)
    class_sum = torch.zeros(len(names), G, G, device=dev)
    class_count = torch.zeros(len(names), device=dev, dtype=torch.int32)
    scratch = {}
    for i in range(0, n, batch_size):
        up = lambda t: t[i:min(i + batch_size, n)].to(dev, non_blocking=True)
        x1, x2, y = model._check_windows(up(eeg1), up(eeg2), up(labels))
        B = x1.shape[0]
        eng = model.engine(B, x1.shape[2], dev)
        if id(eng) not in scratch:
            need = gradcam_scratch_elems(B, eng.C, eng.sp["Hp"], eng.sp["Wp"])
            if need < 0:
                raise EgError(f"eg_gradcam_accumulate does not cover B={B} C={eng.C} Hp={eng.sp['Hp']} Wp={eng.sp['Wp']}")
            scratch[id(eng)] = torch.empty(need, device=dev)
        lg = _gradcam_batch(model, eng, x1, x2, y, target, cams[i:i + B], class_sum, class_count, scratch[id(eng)], len(names))
        logits[i:i + B].copy_(lg)
        call("eg_eval_accumulate", ptr(lg), 0, 0, pred.data_ptr() + 4 * i, 0, 0, B, ncls, eng.stream)
    counts = class_count.cpu().numpy()                           # the one host sync
    mean = (class_sum / class_count.clamp(min=1).float().view(-1, 1, 1)).cpu().numpy()
    return {"class_mean": {name: mean[c] for c, name in enumerate(names)},
            "class_count": {name: int(counts[c]) for c, name in enumerate(names)}, "cams": cams, "count": n, "logits": logits,
            "predictions": pred.long()}


@torch.no_grad()
def embedding_features(model, eeg1: torch.Tensor, eeg2: torch.Tensor, labels: torch.Tensor, batch_size: int = 256) -> Dict[str, Any]:
    """extract_features_for_embedding (eeg_metrics.py:602-673) over the inference engine: windows and batches as predict_windows,
    every batch's tokens gathered on the device, one copy to the host at the end.  Returns numpy arrays under the reference's keys:
      cls1, cls2 [N, d] (and ibs_token [N, d] when the model has synchrony tokens) -- the bits of model.predict --,
      z_fuse [N, 3 d] = cat(cls1, cls2, |cls1 - cls2|) (the reference's proxy of the fused features),
      y_true [N] (the labels as given) and y_pred [N] i64 (the argmax of model.predict's logits)."""
    cfg = model.cfg
    N, ncls, d = eeg1.shape[0], cfg.num_classes, cfg.d_model
    if batch_size < 1 or N < 1 or labels is None or labels.shape[0] != N:
        raise ValueError(f"embedding_features needs N >= 1 labelled windows and batch_size >= 1 (got {N}, {batch_size})")
    dev = next(model.parameters()).device
    keys = {"cls1": "cls1", "cls2": "cls2", **({"ibs_token": "ibs_pool_f"} if cfg.use_ibs else {})}
    feats = {k: torch.empty(N, d, device=dev) for k in keys}
    pred = torch.empty(N, device=dev, dtype=torch.int32)
    packed = set()
    for i in range(0, N, batch_size):
        up = lambda t: t[i:i + batch_size].to(dev, non_blocking=True)
        x1, x2, _ = model._check_windows(up(eeg1), up(eeg2), None)
        B = x1.shape[0]
        eng = model.inference_engine(B, x1.shape[2], dev)
        eng.forward(x1, x2, None, pack=id(eng) not in packed)
        packed.add(id(eng))
        for k, src in keys.items():
            feats[k][i:i + B].copy_(eng.a[src])
        call("eg_eval_accumulate", ptr(eng.a["logits"]), 0, 0, pred.data_ptr() + 4 * i, 0, 0, B, ncls, eng.stream)
    z = torch.cat([feats["cls1"], feats["cls2"], (feats["cls1"] - feats["cls2"]).abs()], dim=-1)
    out = {"z_fuse": z.cpu().numpy(), **{k: v.cpu().numpy() for k, v in feats.items()}}
    out["y_true"] = labels.cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    out["y_pred"] = pred.cpu().numpy().astype(np.int64)
    return out


def embedding_maps(model, eeg1: torch.Tensor, eeg2: torch.Tensor, labels: torch.Tensor, batch_size: int = 256,
                   max_samples: Optional[int] = None, out_dir=None, class_names=None, perplexity: float = 30.0, max_iter: int = 1000,
                   random_state: int = 42) -> Dict[str, Any]:
    """The t-SNE half of run_embedding_analysis (analyze_eeg.py:560-640): embedding_features over the first max_samples windows
    (None: all), then embedding.tsne (compute_tsne's arguments: perplexity 30, 1000 iterations, PCA init) of z_fuse and, when the
    model has synchrony tokens, of ibs_token.  Returns {feature: {"coords" [N, 2] f32 numpy, "kl_divergence", "n_iter"}} plus
    y_true and y_pred; with out_dir also writes tsne_<feature>.csv there under the reference's columns.  The exact method holds
    N x N matrices: more than 16384 windows raise -- pass max_samples, nothing is subsampled silently."""
    from . import embedding as E
    from ._lib import TSNE_MAX_N
    N = eeg1.shape[0]
    if max_samples is not None and max_samples < 2:
        raise ValueError(f"embedding_maps needs max_samples >= 2 or None, got {max_samples}")
    n = N if max_samples is None else min(N, max_samples)
    if not 2 <= n <= TSNE_MAX_N:
        raise ValueError(f"embedding_maps: exact t-SNE serves 2 to {TSNE_MAX_N} windows, got {n}: set max_samples")
    feats = embedding_features(model, eeg1[:n], eeg2[:n], labels[:n], batch_size)
    names = CLASS_NAMES if class_names is None else list(class_names)
    out = {"y_true": feats["y_true"], "y_pred": feats["y_pred"]}
    for key in ("z_fuse", "ibs_token"):
        if key not in feats:
            continue
        Y, kl, it = E.tsne(feats[key], perplexity=perplexity, max_iter=max_iter, init="pca", random_state=random_state)
        out[key] = {"coords": Y.cpu().numpy(), "kl_divergence": kl, "n_iter": it}
        if out_dir is not None:
            Path(out_dir).mkdir(parents=True, exist_ok=True)
            E.write_tsne_csv(Path(out_dir) / f"tsne_{key}.csv", out[key]["coords"], feats["y_true"], feats["y_pred"], names)
    return out


def band_metrics_from_confusion(cm) -> Dict[str, float]:
    """{"accuracy", "f1"} of compute_frequency_sensitivity (eeg_metrics.py:403-411) from a confusion matrix cm[true][predicted]:
    accuracy_score and the macro F1 of precision_recall_fscore_support(average="macro", zero_division=0), which averages over
    the classes that occur in the labels or in the predictions -- train_art.macro_metrics_from_confusion's rule."""
    from .train_art import macro_metrics_from_confusion
    m = macro_metrics_from_confusion(cm)
    return {"accuracy": m["eval/accuracy"], "f1": m["eval/f1"]}


@torch.no_grad()
def frequency_sensitivity(model, eeg1: torch.Tensor, eeg2: torch.Tensor, labels: torch.Tensor, batch_size: int = 256,
                          band_names=None) -> Dict[str, Any]:
    """compute_frequency_sensitivity (eeg_metrics.py:318-413) in ONE walk instead of one per band: every batch makes one
    InferenceEngine.forward_band_masks call over [None, 0, ..., nbands - 1], so the front end, the spectrogram tokens and the
    synchrony matrices are computed once and only the tokeniser and the encoder run per variant; argmax and the confusion counts
    stay on the device (eg_eval_accumulate), the host syncs once, at the end.  Returns
      sensitivity {band name: {"accuracy", "f1"}} with that band masked, baseline (the same pair, nothing masked),
      confusion [1 + nbands, ncls, ncls] (numpy, [variant][true][predicted]; variant 0 is the baseline),
      logits [1 + nbands, N, ncls] f32 (device).
    A model without matrix-form synchrony tokens has nothing to mask (the reference registers no hook): every band equals the
    baseline."""
    from . import tokens
    cfg = model.cfg
    names = BAND_NAMES if band_names is None else list(band_names)
    nbands = len(tokens.ROBUST_BANDS)
    N, ncls = eeg1.shape[0], cfg.num_classes
    if batch_size < 1 or N < 1 or labels is None or labels.shape[0] != N or len(names) != nbands:
        raise ValueError(f"frequency_sensitivity needs N >= 1 labelled windows, batch_size >= 1 and {nbands} band names "
                         f"(got {N}, {batch_size}, {len(names)})")
    dev = next(model.parameters()).device
    bands = [None] + list(range(nbands))
    logits = torch.empty(len(bands), N, ncls, device=dev)
    pred = torch.empty(N, device=dev, dtype=torch.int32)
    cm = torch.zeros(len(bands), ncls, ncls, device=dev, dtype=torch.int32)
    packed = set()
    for i in range(0, N, batch_size):
        up = lambda t: t[i:i + batch_size].to(dev, non_blocking=True)
        x1, x2, y = model._check_windows(up(eeg1), up(eeg2), up(labels))
        B = x1.shape[0]
        eng = model.inference_engine(B, x1.shape[2], dev)

        def each(v):
            logits[v, i:i + B].copy_(eng.a["logits"])
            call("eg_eval_accumulate", ptr(eng.a["logits"]), ptr(y), 0, pred.data_ptr() + 4 * i, ptr(cm[v]), 0, B, ncls, eng.stream)
        eng.forward_band_masks(x1, x2, bands, each, pack=id(eng) not in packed)
        packed.add(id(eng))
    conf = cm.cpu().numpy()                                      # the one host sync
    return {"sensitivity": {name: band_metrics_from_confusion(conf[1 + b]) for b, name in enumerate(names)},
            "baseline": band_metrics_from_confusion(conf[0]), "confusion": conf, "logits": logits}


def main(args):
    from . import train_art as TA
    from .data import ResidentWindows, WindowShards
    if not torch.cuda.is_available():
        raise SystemExit("predict.py (HIP) needs an MI355X: there is no CPU fallback")
    config = TA.load_config(args.config)
    device = torch.device("cuda", 0)
    model = TA.build_model(config, args.dtype).to(device)
    ck = torch.load(args.checkpoint, map_location="cpu", weights_only=False)
    model.load_state_dict(ck.get("model_state_dict", ck))
    d, t = config["data"], config["training"]
    ebs, pre = t["per_device_eval_batch_size"], d.get("enable_preprocessing", False)
    # (callers that build `args` themselves, from before the two flags existed, leave them out)
    conn_stats, band_masks = getattr(args, "connectivity_stats", False), getattr(args, "frequency_sensitivity", False)
    gradcam, embedding = getattr(args, "gradcam", False), getattr(args, "embedding", None)
    if getattr(args, "recording_preprocessing", False):
        d["recording_preprocessing"] = True                          # the three values come from the YAML's data section
    if args.resident:
        d["resident"] = True
    TA.recording_preprocessing_of(config)                            # raises unless the store is walked (--resident / data.resident)
    if d.get("resident", False):
        # the store is walked directly: gather launch -> inference engine, batch by batch; no window visits the host
        stores = TA.prepare_store(config, TA.store_dir(config))
        ld = ResidentWindows(stores[args.split], ebs, device, preprocessing=pre)
        out = predict_loader(model, ld)
        y = out["labels"].cpu()
        if args.attention_stats is not None or conn_stats or band_masks or gradcam or embedding:
            x1, x2 = (torch.cat(p) for p in zip(*((b["eeg1"], b["eeg2"]) for b in ld)))     # stays on the device
    else:
        shards = TA.prepare_shards(config, Path(t["output_dir"]) / "window_shards")
        ld = WindowShards(shards[args.split], ebs, device, preprocessing=pre)
        parts = [(b["eeg1"].cpu(), b["eeg2"].cpu(), b["labels"].cpu()) for b in ld]
        x1, x2, y = (torch.cat(p).pin_memory() for p in zip(*parts))
        out = predict_windows(model, x1, x2, y, batch_size=ebs)
    extra = {}
    if args.attention_stats is not None:
        where = "cross" if args.attention_stats == "cross" else int(args.attention_stats)
        st = attention_statistics(model, x1, x2, y, batch_size=t["per_device_eval_batch_size"], max_samples=args.attention_max_samples,
                                  where=where)
        if st:
            extra = {"attn_mean_map": st["mean_map"], "attn_diagonals": st["diagonals"],
                     **{f"attn_class_{k}_mean_diagonal": v["mean_diagonal_vector"] for k, v in st["diagonal_stats"].items()}}
    if conn_stats:
        st = connectivity_statistics(model, x1, x2, y, batch_size=ebs)
        if st:
            extra.update({f"conn_class_{k}_mean": v for k, v in st["class_mean"].items()})
            extra["conn_class_count"] = np.array(list(st["class_count"].values()), dtype=np.int64)
            if "difference" in st:
                extra["conn_difference"] = st["difference"]
    if band_masks:
        st = frequency_sensitivity(model, x1, x2, y, batch_size=ebs)
        for k, v in st["sensitivity"].items():
            extra[f"band_{k}_accuracy"], extra[f"band_{k}_f1"] = v["accuracy"], v["f1"]
        extra["band_confusion"] = st["confusion"]
    if gradcam:
        st = gradcam_statistics(model, x1, x2, y, batch_size=ebs, max_samples=getattr(args, "gradcam_max_samples", 100))
        if st:
            extra.update({f"gradcam_class_{k}_mean": v for k, v in st["class_mean"].items()})
            extra["gradcam_class_count"] = np.array(list(st["class_count"].values()), dtype=np.int64)
    if embedding:
        st = embedding_maps(model, x1, x2, y, batch_size=ebs, max_samples=getattr(args, "embedding_max_samples", None), out_dir=embedding)
        for k in ("z_fuse", "ibs_token"):
            if k in st:
                extra[f"tsne_{k}"], extra[f"tsne_{k}_kl_divergence"] = st[k]["coords"], st[k]["kl_divergence"]
    np.savez(args.out, logits=out["logits"].cpu().numpy(), predictions=out["predictions"].cpu().numpy(), labels=y.numpy(),
             confusion=out["confusion"], loss=out["loss"], **{k.replace("/", "_"): v for k, v in out["metrics"].items()}, **extra)
    print(" ".join(f"{k}: {v:.4f}" for k, v in {"eval/loss": out["loss"], **out["metrics"]}.items()))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="Predict with a trained Dual EEG Transformer over the window shards (MI355X HIP engine)")
    ap.add_argument("--config", type=str, required=True)
    ap.add_argument("--checkpoint", type=str, required=True)
    ap.add_argument("--out", type=str, required=True)
    ap.add_argument("--split", type=str, default="test", choices=["train", "test"])
    ap.add_argument("--dtype", type=str, default=None, choices=[None, "bf16", "fp16", "f32"])
    ap.add_argument("--resident", action="store_true",
                    help="walk the device-resident recording store (also: data.resident in the config) instead of the window shards")
    ap.add_argument("--recording-preprocessing", action="store_true",
                    help="raw recordings: band-pass (data.filter_low..data.filter_high Hz at data.sampling_rate), CAR and z-score every "
                         "whole recording on the device when the store is built (also: data.recording_preprocessing in the config); "
                         "needs --resident")
    ap.add_argument("--attention-stats", type=str, nargs="?", const="cross", default=None, metavar="cross|LAYER",
                    help="also reduce the attention probabilities of the cross stage (default) or of encoder layer LAYER: "
                         "attn_mean_map, attn_diagonals and attn_class_<name>_mean_diagonal in the output file")
    ap.add_argument("--attention-max-samples", type=int, default=200, help="the reference's max_samples (whole batches until reached)")
    ap.add_argument("--connectivity-stats", action="store_true",
                    help="also average the connectivity matrices per class on the device: conn_class_<name>_mean, conn_difference "
                         "(Cooperation - Competition) and conn_class_count in the output file")
    ap.add_argument("--frequency-sensitivity", action="store_true",
                    help="also classify with each frequency band of the connectivity matrices masked, in one walk: "
                         "band_<name>_accuracy, band_<name>_f1 and band_confusion in the output file")
    ap.add_argument("--gradcam", action="store_true",
                    help="also compute the class-mean Grad-CAM maps of the spectrogram CNN on the device: gradcam_class_<name>_mean "
                         "[64, 64] and gradcam_class_count in the output file")
    ap.add_argument("--gradcam-max-samples", type=int, default=100, help="the reference's max_samples (whole batches until reached)")
    ap.add_argument("--embedding", type=str, default=None, metavar="DIR",
                    help="also map z_fuse (and ibs_token) with exact t-SNE on the device: tsne_z_fuse.csv / tsne_ibs_token.csv in DIR, "
                         "tsne_<feature> and tsne_<feature>_kl_divergence in the output file")
    ap.add_argument("--embedding-max-samples", type=int, default=None,
                    help="map the first N windows only (the exact method serves at most 16384; more without this flag is an error)")
    main(ap.parse_args())
