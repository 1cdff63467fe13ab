"""Running a trained model over whole datasets (the reference's evaluate() loop, T:258-314, and the re-built models of
analyze_eeg.py / eeg_metrics.py): DualEEGTransformer.predict's forward-only engine batch by batch, with the per-batch tail --
argmax, confusion matrix, loss sum -- kept on the device (eg_eval_accumulate), so that the host syncs once, at the end.

    python -m eyegaze_multimodal_amd.predict --config CONFIG.yaml --checkpoint best_model.pt --out FILE.npz
"""
from __future__ import annotations

import argparse
from pathlib import Path
from typing import Any, Dict, Optional

import numpy as np
import torch

from ._lib import call, ptr


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
    np.savez(args.out, logits=out["logits"].cpu().numpy(), predictions=out["predictions"].cpu().numpy(), labels=y.numpy(),
             confusion=out["confusion"], loss=out["loss"], **{k.replace("/", "_"): v for k, v in out["metrics"].items()})
    print(" ".join(f"{k}: {v:.4f}" for k, v in {"eval/loss": out["loss"], **out["metrics"]}.items()))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="Predict with a trained Dual EEG Transformer over the window shards (MI355X HIP engine)")
    ap.add_argument("--config", type=str, required=True)
    ap.add_argument("--checkpoint", type=str, required=True)
    ap.add_argument("--out", type=str, required=True)
    ap.add_argument("--split", type=str, default="test", choices=["train", "test"])
    ap.add_argument("--dtype", type=str, default=None, choices=[None, "bf16", "fp16", "f32"])
    main(ap.parse_args())
