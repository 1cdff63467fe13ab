"""CPU replica of the 64-bit-index dropout mask of the long-sequence attention core (csrc/common.h: eg_hash_pair64 /
eg_dropout64): the pair index's high word moves seed_hi, so below 2^32 the mask is tests.helpers.hip_keep_mask's."""
import numpy as np


def hip_keep_mask64(seed: int, site: int, idx: np.ndarray, p: float) -> np.ndarray:
    """keep[i] for 64-bit element indices idx: one 32-bit hash per PAIR of consecutive elements, 16 bits each."""
    from eyegaze_multimodal_amd.engine import scramble_seed
    M = np.uint64(0xFFFFFFFF)
    seed = scramble_seed(seed)
    seed_lo, seed_hi = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    idx = np.asarray(idx).astype(np.uint64)
    pair = idx >> np.uint64(1)
    hi = (seed_hi + (pair >> np.uint64(32)) * np.uint64(0x9E3779B9)) & M
    k = np.uint64((site * 0x9E3779B9) & 0xFFFFFFFF)
    a = ((seed_lo ^ k) * np.uint64(0x85EBCA6B)) & M
    a ^= a >> np.uint64(15)
    b = (((hi + k) & M) * np.uint64(0xC2B2AE35)) & M
    b ^= b >> np.uint64(13)
    x = (pair & M) ^ a
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M
    x ^= x >> np.uint64(15)
    x = (x + b) & M
    x = (x * np.uint64(0x846CA68B)) & M
    x ^= x >> np.uint64(16)
    half = np.where((idx & np.uint64(1)) == 1, x >> np.uint64(16), x & np.uint64(0xFFFF))
    return half >= np.uint64(int(p * 65536.0 + 0.5))


def attn_element_index(w: int, H: int, S: int) -> np.ndarray:
    """[H, S, S] element indices ((w*H + h)*S + q)*Sp2 + key of query window w, in 64 bits"""
    Sp2 = (S + 1) & ~1
    h = np.arange(H, dtype=np.uint64).reshape(H, 1, 1)
    q = np.arange(S, dtype=np.uint64).reshape(1, S, 1)
    k = np.arange(S, dtype=np.uint64).reshape(1, 1, S)
    return ((np.uint64(w * H) + h) * np.uint64(S) + q) * np.uint64(Sp2) + k
