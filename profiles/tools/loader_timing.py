"""Shard loader against device-resident recordings -> profiles/resident_loader_timing.json.

    python profiles/tools/loader_timing.py OUT.json [WORKDIR]

Synthetic recordings from a seed (randn * 3e-5 + 1e-3, the EEG-like scale of the data tests), cut at window 1024 / stride 256
into BOTH caches under WORKDIR (a temporary directory by default): 32 pairs x 256 windows at C = 8 (B = 256) and 16 pairs x 256
windows at C = 32 (B = 128), i.e. 32 batches per epoch with no ragged tail.  Everything is shuffled; sides alternate inside a
round and every figure is given for each of 3 rounds, so the spread is on the page.
  loader    wall ms per batch over 7 epochs (224 batches) of iterating a loader and dropping its batches, one synchronise at the
            end; WindowShards is built once outside the timed region (train_art builds one per epoch: not charged here) and reads
            shards that the build just wrote, i.e. from the page cache -- both favour the shard side
  launch    eg_window_gather against eg_window_normalize on a batch of the same shape, HIP events around 200 launches
  epoch     ms per step of Trainer.train_step (bf16; cfg3 on the C = 8 data, a5c32 on the C = 32 data) over 4 epochs (128 steps)
            fed by WindowShards, by ResidentWindows, and by ONE fixed device batch (bench.py's condition), one synchronise at the end;
            and, to take the resident-fed step apart, by the fixed batch behind one eg_window_normalize launch per step and by the
            gather launch cutting the same windows every step
  size      bytes on disk of both caches for this data, and computed for a split of N windows over P pairs
A run that finds no GPU fails."""
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))

W, STRIDE, ROUNDS = 1024, 256, 3
DATA = {"cfg3": dict(C=8, B=256, pairs=32, nwin=256), "a5c32": dict(C=32, B=128, pairs=16, nwin=256)}


def spread(xs):
    return {"runs": [round(x, 4) for x in xs], "mean": round(float(np.mean(xs)), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def dir_bytes(p: Path) -> int:
    return sum(f.stat().st_size for f in p.rglob("*") if f.is_file())


def store_bytes(n_windows: int, n_pairs: int, C: int, window: int = W, stride: int = STRIDE) -> int:
    """sum over pairs of 2 C ((nwin_p - 1) stride + window) floats = 2 C (stride N + (window - stride) P) floats"""
    return 4 * 2 * C * (stride * n_windows + (window - stride) * n_pairs)


def shard_bytes(n_windows: int, C: int, window: int = W) -> int:
    return 4 * 2 * C * window * n_windows


def make_data(root: Path, C, pairs, nwin, **_):
    from eyegaze_multimodal_amd.data import build_recording_store, build_window_shards
    rng = np.random.default_rng(C)
    L = (nwin - 1) * STRIDE + W
    recs = {f"r{i}_{w}": (rng.standard_normal((C, L), dtype=np.float32) * 3e-5 + 1e-3).astype(np.float32) for i in range(pairs) for w in (1, 2)}
    items = [{"player1": f"r{i}_1", "player2": f"r{i}_2", "class": str(i % 3)} for i in range(pairs)]
    l2i = {"0": 0, "1": 1, "2": 2}
    t0 = time.perf_counter()
    build_window_shards(items, None, l2i, root / "shards", W, STRIDE, recordings=recs)
    t1 = time.perf_counter()
    build_recording_store(items, None, l2i, root / "store", W, STRIDE, recordings=recs)
    t2 = time.perf_counter()
    n = pairs * nwin
    return {"windows": n, "pairs": pairs, "shard_bytes_on_disk": dir_bytes(root / "shards"), "store_bytes_on_disk": dir_bytes(root / "store"),
            "shard_bytes_computed": shard_bytes(n, C), "store_bytes_computed": store_bytes(n, pairs, C),
            "build_shards_s": round(t1 - t0, 2), "build_store_s": round(t2 - t1, 2)}


def loader_alone(torch, loaders, epochs=7):
    res = {k: [] for k in loaders}
    epoch = [0]

    def walk(ld, n_epochs):
        nb = 0
        for _ in range(n_epochs):
            epoch[0] += 1
            ld.set_epoch(epoch[0])
            for b in ld:
                nb += 1
        torch.cuda.synchronize()
        return nb
    for ld in loaders.values():
        walk(ld, 1)
    for _ in range(ROUNDS):
        for k, ld in loaders.items():
            t0 = time.perf_counter()
            nb = walk(ld, epochs)
            res[k].append((time.perf_counter() - t0) / nb * 1e3)
    return {f"{k}_ms_per_batch": spread(v) for k, v in res.items()}, nb


def launches(torch, resident, B, C, reps=200, warm=20):
    from eyegaze_multimodal_amd._lib import call, ptr
    dev = resident.device
    raw = torch.randn(B, 2, C, W, device=dev) * 3e-5 + 1e-3
    o1, o2 = torch.empty(B, C, W, device=dev), torch.empty(B, C, W, device=dev)
    order = torch.from_numpy(np.random.default_rng(0).permutation(resident.n).astype(np.int32)).to(dev)
    fns = {"window_normalize": lambda: call("eg_window_normalize", ptr(raw), ptr(o1), ptr(o2), B, C, W, 0, torch.cuda.current_stream().cuda_stream),
           "window_gather": lambda: resident.store.gather(order, 0, B, 0)}       # includes its three output allocations (cached blocks)
    res = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            for _ in range(warm):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            res[k].append(a.elapsed_time(b) * 1e3 / reps)
    return {f"{k}_us": spread(v) for k, v in res.items()}


def trainer_config(workload, C):
    from bench import WORKLOADS
    kw = WORKLOADS[workload][0]
    return {
        "ablation": {"use_spectrogram": kw["use_spectrogram"], "use_ibs": kw["use_ibs"], "ibs_mode": "robust", "ibs_instance_norm": True,
                     "ibs_feature_type": "all", "use_cross_attention": kw["use_cross_attention"]},
        "model": {"in_channels": C, "num_labels": 3, "d_model": 256, "num_layers": 6, "num_heads": 8, "d_ff": 1024, "conv_kernel_size": 25,
                  "conv_stride": 4, "conv_layers": 2, "spec_n_fft": 128, "spec_hop_length": 64, "spec_freq_bins": 64},
        "data": {"window_size": W, "stride": STRIDE, "sampling_rate": 256, "random_seed": 42},
        "training": {"num_train_epochs": 1, "learning_rate": 1e-4, "weight_decay": 0.01, "dropout": 0.1, "use_sym_loss": False,
                     "use_ibs_loss": False, "use_ibs_cls_loss": True, "use_ibs_contrastive": False, "lambda_ibs_cls": 0.5},
        "system": {"seed": 42},
    }


def epochs_fed(torch, workload, C, loaders, epochs=4, warm=20):
    from eyegaze_multimodal_amd._lib import call, ptr
    from eyegaze_multimodal_amd.train_art import Trainer
    dev = torch.device("cuda", 0)
    tr = Trainer(trainer_config(workload, C), dev, compute_dtype="bf16")
    fixed = next(iter(loaders["resident"]))
    fixed = (fixed["eeg1"].clone(), fixed["eeg2"].clone(), fixed["labels"].clone())
    per_epoch = len(loaders["resident"])
    epoch = [0]

    def fed(ld):
        n = 0
        for _ in range(epochs):
            epoch[0] += 1
            ld.set_epoch(epoch[0])
            for b in ld:
                tr.train_step(b["eeg1"], b["eeg2"], b["labels"])
                n += 1
        return n

    def fed_fixed():
        for _ in range(epochs * per_epoch):
            tr.train_step(*fixed)
        return epochs * per_epoch
    # two more feeds that take the resident-fed step apart: the fixed batch with ONE normalisation launch per step in front of it,
    # and the gather launch cutting the SAME windows every step (no iterator, no new data)
    B = fixed[0].shape[0]
    raw = torch.randn(B, 2, C, W, device=dev) * 3e-5 + 1e-3
    res_ld = loaders["resident"]
    same_order = torch.from_numpy(np.random.default_rng(0).permutation(res_ld.n).astype(np.int32)).to(dev)

    def fed_fixed_normalize():
        for _ in range(epochs * per_epoch):
            x1, x2 = torch.empty(B, C, W, device=dev), torch.empty(B, C, W, device=dev)
            call("eg_window_normalize", ptr(raw), ptr(x1), ptr(x2), B, C, W, 0, torch.cuda.current_stream().cuda_stream)
            tr.train_step(x1, x2, fixed[2])
        return epochs * per_epoch

    def fed_same_gather():
        for _ in range(epochs * per_epoch):
            tr.train_step(*res_ld.store.gather(same_order, 0, B, 0))
        return epochs * per_epoch
    sides = {"shards": lambda: fed(loaders["shards"]), "resident": lambda: fed(loaders["resident"]), "fixed_batch": fed_fixed,
             "fixed_batch_plus_normalize_launch": fed_fixed_normalize, "resident_same_windows_every_step": fed_same_gather}
    for _ in range(warm):
        tr.train_step(*fixed)
    torch.cuda.synchronize()
    res = {k: [] for k in sides}
    for _ in range(ROUNDS):
        for k, fn in sides.items():
            t0 = time.perf_counter()
            n = fn()
            torch.cuda.synchronize()
            res[k].append((time.perf_counter() - t0) / n * 1e3)
    out = {f"{k}_ms_per_step": spread(v) for k, v in res.items()}
    f = out["fixed_batch_ms_per_step"]
    for k in ("shards", "resident", "fixed_batch_plus_normalize_launch", "resident_same_windows_every_step"):
        s = out[f"{k}_ms_per_step"]
        out[f"{k}_minus_fixed_ms"] = round(s["mean"] - f["mean"], 4)
        out[f"{k}_own_spread_ms"] = round(s["max"] - s["min"], 4)
        out[f"{k}_slower_than_fixed_by_more_than_own_spread"] = bool(s["mean"] - f["mean"] > s["max"] - s["min"])
    out["steps_per_measurement"] = epochs * per_epoch
    del tr
    torch.cuda.empty_cache()
    return out


def main(out_path, workdir=None):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("loader_timing.py measures on the GPU; none found")
    from eyegaze_multimodal_amd.data import ResidentWindows, WindowShards
    res = {"window": W, "stride": STRIDE, "rounds": ROUNDS, "dtype": "bf16", "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory(dir=workdir) as tmp:
        for workload, spec in DATA.items():
            root = Path(tmp) / workload
            C, B = spec["C"], spec["B"]
            r = {"C": C, "B": B, "size": make_data(root, **spec)}
            t0 = time.perf_counter()
            resident = ResidentWindows(root / "store", B, "cuda", shuffle=True, seed=1)
            torch.cuda.synchronize()
            r["resident_construction_s"] = round(time.perf_counter() - t0, 3)
            loaders = {"shards": WindowShards(root / "shards", B, "cuda", shuffle=True, seed=1), "resident": resident}
            r["loader"], r["loader_batches_per_measurement"] = loader_alone(torch, loaders)
            r["launch"] = launches(torch, resident, B, C)
            r["epoch"] = epochs_fed(torch, workload, C, loaders)
            res[workload] = r
            print(json.dumps({workload: r}), flush=True)
            del loaders, resident
            torch.cuda.empty_cache()
    lab = {"windows": 28683, "C": 32, "shard_bytes": shard_bytes(28683, 32),
           "store_bytes_by_pairs": {str(p): store_bytes(28683, p, 32) for p in (500, 1000, 2000, 3000)}}
    res["lab_split_computed"] = lab
    Path(out_path).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "resident_loader_timing.json", sys.argv[2] if len(sys.argv) > 2 else None)
