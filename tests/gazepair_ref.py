"""CPU restatement of the gaze pair analysis (include/eyegaze_hip.h states the contracts of eg_gaze_pair_stats and
eg_row_cosine): the reference's compute_gaze_distance and compute_gaze_overlap (6_Utils/error_analysis.py:277-358) on the uint8
store, written from the formulas alone in numpy -- rounded fp32 operations where torch runs fp32 ones, math.fsum where the device
sums in fp64 -- so that it is a second statement of what csrc/gazepair.hip computes, not a call into it.  Also the seeded images of
tests/golden/gaze_pairs.npz (the generator and the tests draw them from here) and every error bound the tests use, each derived
where it is stated.  tests/test_gaze_pairs_host.py pins it to the reference's own outputs."""
import math

import numpy as np

from tests import gazeimg_ref as IR

FIELDS = ("distance", "overlap", "cy_a", "cx_a", "cy_b", "cx_b", "inter", "union", "na", "nb", "S_a", "S_b", "A_a", "A_b")
U32, U64 = 2.0 ** -24, 2.0 ** -53          # unit roundoffs of fp32 and fp64
DEFAULT_CENTRE = 112.0                     # error_analysis.py:302, a literal: it does not follow H and W


# ---------------------------------------------------------------------------------------------------------------
# the fixture's images
# ---------------------------------------------------------------------------------------------------------------
SIZES = [(8, 8), (16, 24), (17, 23), (64, 64)]                                 # (F, W)
N_SEEDED = 6                                                                   # per size: blob, noise, blob, noise, blob, blob
ZERO, CONST = 6, 7                                                             # then an all-zero and a constant image
CONST_RGB = (200, 90, 30)
PAIRS = [(0, 1), (2, 3), (4, 5), (0, 2), (0, 4), (1, 1), (ZERO, 0), (ZERO, ZERO), (CONST, 0), (CONST, ZERO), (3, 5), (1, 3)]
BIG = (224, 224)                                                               # one pair: outputs only, images from the seed


def blob_image(rng, h: int, w: int) -> np.ndarray:
    """a few Gaussian blobs per channel on a dark floor, as tests/make_golden_gaze_images.py draws its heat maps"""
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    img = np.zeros((h, w, 3), np.float64)
    for c in range(3):
        for _ in range(3):
            cy, cx, s = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.08, 0.3) * max(h, w)
            img[..., c] += rng.uniform(80, 255) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    return np.clip(img + 12, 0, 255).astype(np.uint8)


def noise_image(rng, h: int, w: int) -> np.ndarray:
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def seeded_images(seed: int, h: int, w: int, n: int = N_SEEDED) -> np.ndarray:
    """[n, h, w, 3] uint8: blob, noise, blob, noise, then blobs"""
    rng = np.random.default_rng(seed)
    return np.stack([noise_image(rng, h, w) if i in (1, 3) else blob_image(rng, h, w) for i in range(n)])


def with_extras(seeded: np.ndarray) -> np.ndarray:
    _, h, w, _ = seeded.shape
    const = np.broadcast_to(np.asarray(CONST_RGB, np.uint8), (1, h, w, 3))
    return np.concatenate([seeded, np.zeros((1, h, w, 3), np.uint8), const])


# ---------------------------------------------------------------------------------------------------------------
# tables and pixels
# ---------------------------------------------------------------------------------------------------------------
def raw_table() -> np.ndarray:
    """ToTensor alone: float32(v) / 255 in every channel"""
    v = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    return np.stack([v, v, v])


def tables():
    return {"norm": IR.normalise_table(), "raw": raw_table()}


def gray(img: np.ndarray, table: np.ndarray) -> np.ndarray:
    """(F, W, 3) uint8 -> (F, W) f32: ((t0 + t1) + t2) / 3.0f, tensor.mean(dim=0) bit for bit"""
    return IR.to_tensors(img, table)[1]


def image_stats(g: np.ndarray) -> dict:
    """S, Sy, Sx, A of one image exactly (math.fsum over the fp32 terms, the products rounded to fp32 as torch rounds them), the
    fp32 min and max, and the absolute term sums Ty = sum |fl32(g y)|, Tx = sum |fl32(g x)| that the bounds below read"""
    F, W = g.shape
    gy = (g * np.arange(F, dtype=np.float32)[:, None]).astype(np.float32)
    gx = (g * np.arange(W, dtype=np.float32)[None, :]).astype(np.float32)
    f = lambda a: math.fsum(a.astype(np.float64).ravel().tolist())
    return {"S": f(g), "Sy": f(gy), "Sx": f(gx), "A": f(np.abs(g)), "Ty": f(np.abs(gy)), "Tx": f(np.abs(gx)),
            "min": np.float32(g.min()), "max": np.float32(g.max()), "n": F * W}


def centre(st: dict):
    if st["S"] < 1e-8:
        return DEFAULT_CENTRE, DEFAULT_CENTRE
    return st["Sy"] / st["S"], st["Sx"] / st["S"]


def mask(g: np.ndarray, st: dict, threshold: float = 0.1) -> np.ndarray:
    """(g - min) / ((max - min) + 1e-8f) > threshold: rounded fp32 operations, 1e-8 and the threshold as float32 scalars"""
    d = np.float32(np.float32(st["max"] - st["min"]) + np.float32(1e-8))
    return ((g - st["min"]).astype(np.float32) / d).astype(np.float32) > np.float32(threshold)


def pair_row(ga: np.ndarray, gb: np.ndarray, threshold: float = 0.1, sa: dict = None, sb: dict = None) -> dict:
    sa, sb = sa or image_stats(ga), sb or image_stats(gb)
    ma, mb = mask(ga, sa, threshold), mask(gb, sb, threshold)
    na, nb, inter = int(ma.sum()), int(mb.sum()), int((ma & mb).sum())
    union = na + nb - inter
    (cya, cxa), (cyb, cxb) = centre(sa), centre(sb)
    return {"distance": float(np.sqrt((cya - cyb) ** 2 + (cxa - cxb) ** 2)),
            "overlap": float(np.float32(inter) / np.float32(union)) if union else 0.0,
            "cy_a": cya, "cx_a": cxa, "cy_b": cyb, "cx_b": cxb, "inter": inter, "union": union, "na": na, "nb": nb,
            "S_a": sa["S"], "S_b": sb["S"], "A_a": sa["A"], "A_b": sb["A"]}


def pair_table(store: np.ndarray, pair_img, table: np.ndarray, threshold: float = 0.1):
    """rows (list of pair_row dicts) and the per-image stats they were made from"""
    used = sorted({int(i) for p in pair_img for i in p})
    g = {i: gray(store[i], table) for i in used}
    st = {i: image_stats(g[i]) for i in used}
    return [pair_row(g[a], g[b], threshold, st[a], st[b]) for a, b in np.asarray(pair_img).tolist()], st


# ---------------------------------------------------------------------------------------------------------------
# bounds.  Summing n terms t_i in floating point with unit roundoff u, in ANY order, errs by at most (n - 1) u sum |t_i| to first
# order (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4); n u is used below, which also pays the second order.
# ---------------------------------------------------------------------------------------------------------------
def sum_bounds(st: dict, u: float = U64) -> dict:
    """|computed - exact| for S, Sy, Sx, A summed at unit roundoff u"""
    n = st["n"]
    return {"S": n * u * st["A"], "Sy": n * u * st["Ty"], "Sx": n * u * st["Tx"], "A": n * u * st["A"]}


def centre_bounds(st: dict, u: float):
    """|c' - c| for c = Sk / S computed from sums of unit roundoff u and one rounded division:
    c' = (Sk + dk) / (S + ds) (1 + e), |dk| <= n u Tk, |ds| <= n u A, |e| <= u, so to first order
    |c' - c| <= n u (Tk + |c| A) / |S| + u |c|; 2 u |c| pays for the rounding of the value read back (.item()) as well.  A centre
    from the default branch is the literal on both sides: 0."""
    if st["S"] < 1e-8:
        return 0.0, 0.0
    n, (cy, cx) = st["n"], centre(st)
    return (n * u * (st["Ty"] + abs(cy) * st["A"]) / abs(st["S"]) + 2 * u * abs(cy),
            n * u * (st["Tx"] + abs(cx) * st["A"]) / abs(st["S"]) + 2 * u * abs(cx))


def distance_bound(sa: dict, sb: dict, u: float, distance: float = 0.0) -> float:
    """the distance is 1-Lipschitz in each of its four coordinates: the sum of their bounds; its own fp64 arithmetic (two
    differences, two squares, a sum and a root, each within 2^-53 relative) adds at most 8 * 2^-53 of the distance"""
    return sum(centre_bounds(sa, u)) + sum(centre_bounds(sb, u)) + 8 * U64 * abs(distance)


def well_conditioned(st: dict) -> bool:
    """the fixture's condition on an image: centre-of-mass branch with S >= 1 and sum |g| / |S| <= 16, or default branch with
    S <= -1 or S == 0 -- then an fp32 sum in any order (error <= n 2^-24 A <= 2^-6 A at 512 x 512) decides total < 1e-8 as fp64"""
    return (st["S"] >= 1.0 and st["A"] <= 16.0 * abs(st["S"])) or st["S"] <= -1.0 or (st["S"] == 0.0 and st["A"] == 0.0)


# ---------------------------------------------------------------------------------------------------------------
# cosine
# ---------------------------------------------------------------------------------------------------------------
def row_cosine(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """fp64: dot / (max(|a|, 1e-12) max(|b|, 1e-12)), F.normalize's clamp on either norm"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.sqrt((a * a).sum(-1)), np.sqrt((b * b).sum(-1))
    return (a * b).sum(-1) / (np.maximum(na, 1e-12) * np.maximum(nb, 1e-12))


COSINE_D = [1, 3, 64, 257, 4096]
COSINE_N = 5


def cosine_inputs(seed: int, D: int):
    """a, b [5, D] f32: correlated rows, row 3 of a all zero (the clamp), row 4 of b = -a"""
    rng = np.random.default_rng(seed + D)
    a = rng.standard_normal((COSINE_N, D)).astype(np.float32)
    b = (0.6 * a + 0.8 * rng.standard_normal((COSINE_N, D))).astype(np.float32)
    a[3] = 0.0
    b[4] = -a[4]
    return a, b
