"""Running a trained model over whole datasets (the reference's evaluate() loop, T:258-314, and the re-built models of
analyze_eeg.py / eeg_metrics.py): DualEEGTransformer.predict's forward-only engine batch by batch, with the per-batch tail --
argmax, confusion matrix, loss sum -- kept on the device (eg_eval_accumulate), so that the host syncs once, at the end.
attention_statistics is eeg_metrics.py's extract_attention_weights (:465-594) over the same walk: the mean attention map and the
per-sample diagonals reduced on the device from each batch's q|k|v rows (eg_attention_stats), never a [B, H, S, S] tensor.

    python -m eyegaze_multimodal_amd.predict --config CONFIG.yaml --checkpoint best_model.pt --out FILE.npz [--attention-stats [cross|LAYER]]
"""
from __future__ import annotations

import argparse
from pathlib import Path
from typing import Any, Dict, Optional

import numpy as np
import torch

from ._lib import EgError, attn_stats_scratch_elems, call, ptr


@torch.no_grad()
def predict_windows(model, eeg1: torch.Tensor, eeg2: torch.Tensor, labels: Optional[torch.Tensor] = None,
                    batch_size: int = 256) -> Dict[str, Any]:
    """eeg1, eeg2: f32 [N, C, T] in device memory or (pinned) host memory; labels: [N] or None.  Walks the windows in batches of
    batch_size (the ragged tail as a batch of its own shape), packs the weights once per engine, and returns
      logits [N, ncls] f32 and predictions [N] i64 (device tensors), and with labels also
      confusion [ncls, ncls] (numpy, [true][predicted]), loss (mean of the batches' cross-entropy means, as Trainer.evaluate
      reports it) and metrics (train_art.macro_metrics_from_confusion)."""
    from .train_art import macro_metrics_from_confusion
    N, ncls = eeg1.shape[0], model.cfg.num_classes
    dev = next(model.parameters()).device
    if batch_size < 1 or N < 1:
        raise ValueError(f"predict_windows needs N >= 1 windows and batch_size >= 1 (got {N}, {batch_size})")
    logits = torch.empty(N, ncls, device=dev)
    pred = torch.empty(N, device=dev, dtype=torch.int32)
    cm = torch.zeros(ncls, ncls, device=dev, dtype=torch.int32) if labels is not None else None
    loss_sum = torch.zeros(1, device=dev) if labels is not None else None
    packed, nb = set(), 0
    for i in range(0, N, batch_size):
        up = lambda t: None if t is None else t[i:i + batch_size].to(dev, non_blocking=True)
        x1, x2, y = model._check_windows(up(eeg1), up(eeg2), up(labels))
        B = x1.shape[0]
        eng = model.inference_engine(B, x1.shape[2], dev)
        eng.forward(x1, x2, y, pack=id(eng) not in packed)
        packed.add(id(eng))
        logits[i:i + B].copy_(eng.a["logits"])
        call("eg_eval_accumulate", ptr(eng.a["logits"]), ptr(y), ptr(eng.a["loss"]) if y is not None else 0,
             pred.data_ptr() + 4 * i, ptr(cm), ptr(loss_sum), B, ncls, eng.stream)
        nb += 1
    out = {"logits": logits, "predictions": pred.long()}
    if labels is not None:
        out["confusion"] = cm.cpu().numpy()                      # the one host sync
        out["loss"] = float(loss_sum) / nb
        out["metrics"] = macro_metrics_from_confusion(out["confusion"])
    return out


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


def main(args):
    from . import train_art as TA
    from .data import WindowShards
    if not torch.cuda.is_available():
        raise SystemExit("predict.py (HIP) needs an MI355X: there is no CPU fallback")
    config = TA.load_config(args.config)
    device = torch.device("cuda", 0)
    model = TA.build_model(config, args.dtype).to(device)
    ck = torch.load(args.checkpoint, map_location="cpu", weights_only=False)
    model.load_state_dict(ck.get("model_state_dict", ck))
    d, t = config["data"], config["training"]
    shards = TA.prepare_shards(config, Path(t["output_dir"]) / "window_shards")
    ld = WindowShards(shards[args.split], t["per_device_eval_batch_size"], device, preprocessing=d.get("enable_preprocessing", False))
    parts = [(b["eeg1"].cpu(), b["eeg2"].cpu(), b["labels"].cpu()) for b in ld]
    x1, x2, y = (torch.cat(p).pin_memory() for p in zip(*parts))
    out = predict_windows(model, x1, x2, y, batch_size=t["per_device_eval_batch_size"])
    extra = {}
    if args.attention_stats is not None:
        where = "cross" if args.attention_stats == "cross" else int(args.attention_stats)
        st = attention_statistics(model, x1, x2, y, batch_size=t["per_device_eval_batch_size"], max_samples=args.attention_max_samples,
                                  where=where)
        if st:
            extra = {"attn_mean_map": st["mean_map"], "attn_diagonals": st["diagonals"],
                     **{f"attn_class_{k}_mean_diagonal": v["mean_diagonal_vector"] for k, v in st["diagonal_stats"].items()}}
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
    ap.add_argument("--attention-stats", type=str, nargs="?", const="cross", default=None, metavar="cross|LAYER",
                    help="also reduce the attention probabilities of the cross stage (default) or of encoder layer LAYER: "
                         "attn_mean_map, attn_diagonals and attn_class_<name>_mean_diagonal in the output file")
    ap.add_argument("--attention-max-samples", type=int, default=200, help="the reference's max_samples (whole batches until reached)")
    main(ap.parse_args())
