"""
TEST INFRASTRUCTURE -- the fixture of the gaze image path, written by the libraries the reference's MultimodalDataset
calls (1_Data/processed/multimodal_dataset.py:67-83): Pillow's Image.resize(BILINEAR) and ImageEnhance.Brightness / Contrast (what
torchvision's Resize and ColorJitter run on a PIL image), and torch for ToTensor + Normalize -- float32(v) / 255, minus the float32
mean, divided by the float32 std, the operations torchvision.transforms.functional runs (torchvision itself is not needed for
them).  Runs only where Pillow is; the file holds pixels and numbers only.

Inputs: seeded uint8 RGB images, alternately noise and smooth blobs like heat maps, at sizes chosen for a reason:
  10x7      upscaled on both axes          37x53     odd sizes, a little over 2:1
  24x16     the target transposed          16x24     the target itself (identity tables)
  300x17    long and thin: a ratio of 18.75 down, 1.4 up
  5x1000    ratio 41.7: 85 taps            3x4096    the widest served row
  135x240   a 1080p frame's shape          1x1       one pixel
Stored: every input; Pillow's resize of each to (F, W) = (16, 24) and of three of them to (64, 64); for every resized (16, 24) image
ImageEnhance at the factor pairs (brightness, contrast) of PAIRS -- the factors 0.8, 0.93, 1.0, 1.13 and 1.1999 each once as a
brightness and once as a contrast factor, 1.0 making a pair brightness-only or contrast-only -- in both orders; the normalised tensors
[3, 16, 24] and their mean(0).

Usage:  python tests/make_golden_gaze_images.py
"""
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

SEED = 20241021
SIZES = [(10, 7), (37, 53), (24, 16), (16, 24), (300, 17), (5, 1000), (3, 4096), (135, 240), (1, 1)]      # (h, w)
SMALL, LARGE = (16, 24), (64, 64)                                                                        # (F, W)
LARGE_OF = ["37x53", "300x17", "135x240"]
FACTORS = [0.8, 0.93, 1.0, 1.13, 1.1999]
PAIRS = [(FACTORS[i], FACTORS[(i + 1) % 5]) for i in range(5)]                                            # (brightness, contrast)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FILE_LIMIT = 600_000


def name_of(h, w):
    return f"{h}x{w}"


def images(rng):
    out = {}
    for i, (h, w) in enumerate(SIZES):
        if i % 2 == 0:
            img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        else:                                                             # a few Gaussian blobs per channel on a dark floor
            yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
            img = np.zeros((h, w, 3), np.float64)
            for c in range(3):
                for _ in range(3):
                    cy, cx, s = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.08, 0.3) * max(h, w)
                    img[..., c] += rng.uniform(80, 255) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
            img = np.clip(img + 12, 0, 255).astype(np.uint8)
        out[name_of(h, w)] = img
    return out


def build():
    import torch
    from PIL import Image, ImageEnhance
    import PIL
    rng = np.random.default_rng(SEED)
    out = {"seed": np.int64(SEED), "pillow": np.asarray(PIL.__version__), "names": np.asarray([name_of(*s) for s in SIZES]),
           "large_of": np.asarray(LARGE_OF), "factors": np.asarray(PAIRS, np.float64), "mean": np.asarray(MEAN), "std": np.asarray(STD)}
    mean, std = torch.as_tensor(MEAN, dtype=torch.float32), torch.as_tensor(STD, dtype=torch.float32)
    for name, img in images(rng).items():
        out[f"input/{name}"] = img
        pil = Image.fromarray(img)
        small = pil.resize((SMALL[1], SMALL[0]), Image.BILINEAR)
        out[f"small/{name}"] = np.array(small)
        if name in LARGE_OF:
            out[f"large/{name}"] = np.array(pil.resize((LARGE[1], LARGE[0]), Image.BILINEAR))
        for i, (fb, fc) in enumerate(PAIRS):
            out[f"jitter/{name}/{i}/bc"] = np.array(ImageEnhance.Contrast(ImageEnhance.Brightness(small).enhance(fb)).enhance(fc))
            out[f"jitter/{name}/{i}/cb"] = np.array(ImageEnhance.Brightness(ImageEnhance.Contrast(small).enhance(fc)).enhance(fb))
        t = torch.from_numpy(out[f"small/{name}"]).permute(2, 0, 1).contiguous().to(torch.float32).div(255)      # ToTensor
        t = t.sub(mean[:, None, None]).div(std[:, None, None])                                                    # Normalize
        out[f"rgb/{name}"], out[f"mean/{name}"] = t.numpy(), t.mean(dim=0).numpy()
    return out


if __name__ == "__main__":
    out = build()
    path = REPO / "tests" / "golden" / "gaze_images.npz"
    np.savez_compressed(path, **out)
    assert path.stat().st_size < FILE_LIMIT, path.stat().st_size
    print(f"{path.name}: {path.stat().st_size / 1e3:.0f} kB, {len(out)} arrays, Pillow {out['pillow']}")
