"""Gaze images on the device -> profiles/gaze_timing.json.

    timeout 600 python profiles/tools/gaze_timing.py OUT.json [--runs 7] [--images 64] [--batch 256]

One GPU.  Every figure is HIP events around the entry point's call(s) alone, inputs already on the device, `runs` runs after two
warm-ups, every run listed, the median quoted:
  resize   `images` synthetic frames of 1080 x 1920 x 3 -> 224 x 224 in one eg_gaze_resize call (its two launches together), and
           GazeImageStore.from_arrays of the same frames by wall clock, upload and sync included
  batch    eg_gaze_batch at n = `batch`, 224 x 224, without augmentation, with the reference's augmentation, and with rgb outputs
Bytes are computed from the shapes (what the algorithm has to move: sources once, intermediates written and read twice, outputs
once); the share is bytes / time over the measured copy rate of the MI355X (6.29 TB/s, float4 copy).
Where Pillow is installed the same resizes run on the host in one thread."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))

COPY_BYTES_PER_S = 6.29e12
H, W_SRC, SIDE = 1080, 1920, 224


def frames(rng, n):
    import numpy as np
    yy, xx = np.mgrid[:H, :W_SRC].astype(np.float32)
    out = []
    for _ in range(n):
        cy, cx, s = rng.uniform(200, 880), rng.uniform(300, 1600), rng.uniform(40, 200)
        blob = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
        img = np.stack([255 * blob, 180 * np.sqrt(blob), 60 * (1 - blob)], axis=2) + rng.integers(0, 12, (H, W_SRC, 3))
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def timed(fn, runs):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def entry(ms, nbytes):
    med = statistics.median(ms)
    return {"ms": [round(v, 4) for v in ms], "median_ms": round(med, 4), "bytes": int(nbytes), "TB_per_s": round(nbytes / med / 1e9, 3),
            "share_of_copy_rate": round(nbytes / (med * 1e-3) / COPY_BYTES_PER_S, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    import numpy as np
    import torch
    from eyegaze_multimodal_amd import _lib as L
    from eyegaze_multimodal_amd import gaze as G
    if not torch.cuda.is_available():
        raise SystemExit("gaze_timing.py measures on the GPU: there is none here")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    res = {"device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(), "copy_bytes_per_s": COPY_BYTES_PER_S}
    ims = frames(rng, args.images)
    n = len(ims)
    # ---- eg_gaze_resize alone: the tables of _resize_batch, built once
    size = H * W_SRC * 3
    data = torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims])).to(dev)          # 1080 * 1920 * 3 is a multiple of 16
    mid_one = -(-(3 * SIDE * H) // 16) * 16
    tabs_h, tabs_v = G.resize_tables(W_SRC, SIDE), G.resize_tables(H, SIDE)
    tabs = torch.from_numpy(np.concatenate([tabs_h, tabs_v])).to(dev)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    t = [i64([i * size for i in range(n)]), i32([H] * n), i32([W_SRC] * n), i64([i * mid_one for i in range(n)]), i64([0] * n),
         i64([tabs_h.size] * n)]
    need = L.gaze_resize_workspace_bytes(n, n * H, SIDE)
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    store = torch.empty(n, SIDE, SIDE, 3, dtype=torch.uint8, device=dev)
    desc = L.GazeResizeDesc(L.ptr(data), L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]), L.ptr(t[3]), L.ptr(tabs), L.ptr(t[4]), L.ptr(t[5]), n * H, n, H,
                            SIDE, SIDE)
    st = torch.cuda.current_stream().cuda_stream
    ms = timed(lambda: L.call("eg_gaze_resize", ctypes.byref(desc), L.ptr(work), need, L.ptr(store), st), args.runs)
    mid = n * H * SIDE * 3
    res["resize"] = {"images": n, "from": [H, W_SRC], "to": [SIDE, SIDE],
                     **entry(ms, n * size + mid + 2 * mid + n * SIDE * SIDE * 3)}
    t0 = time.perf_counter()
    whole = G.GazeImageStore.from_arrays(ims, SIDE, dev)
    torch.cuda.synchronize()
    res["resize"]["from_arrays_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
    res["resize"]["equal_to_entry_point"] = bool(torch.equal(whole.data, store))
    try:
        import PIL
        from PIL import Image
        t0 = time.perf_counter()
        ref = [np.array(Image.fromarray(im).resize((SIDE, SIDE), Image.BILINEAR)) for im in ims]
        res["resize"]["pillow"] = {"version": PIL.__version__, "wall_ms": round(1e3 * (time.perf_counter() - t0), 2),
                                   "equal_bytes": bool(np.array_equal(np.stack(ref), store.cpu().numpy()))}
    except ImportError:
        res["resize"]["pillow"] = None
    del data, work
    # ---- eg_gaze_batch
    B = args.batch
    pair_img = torch.from_numpy(rng.integers(0, n, (B, 2)).astype(np.int32)).to(dev)
    ids = torch.arange(B, dtype=torch.int32, device=dev)
    img_bytes, out_bytes = 2 * B * SIDE * SIDE * 3, 2 * B * SIDE * SIDE * 4
    aug = G.GazeAugmentation()
    res["batch"] = {"n": B, "size": [SIDE, SIDE],
                    "plain": entry(timed(lambda: whole.batch(pair_img, ids, ids, 0, B), args.runs), img_bytes + out_bytes),
                    "augmented": entry(timed(lambda: whole.batch(pair_img, ids, ids, 0, B, aug, 7), args.runs), 2 * img_bytes + out_bytes),
                    "augmented_rgb": entry(timed(lambda: whole.batch(pair_img, ids, ids, 0, B, aug, 7, rgb=True), args.runs),
                                           2 * img_bytes + 4 * out_bytes)}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
