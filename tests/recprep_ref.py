"""TEST INFRASTRUCTURE -- a sequential float64 numpy restatement of the recording preprocessing: what
eg_recording_filtfilt and eg_recording_car_zscore state, sample by sample, with no scipy.  One (C, L) float32 recording at a
time; the recurrence runs over time in Python and over the channels in numpy."""
import numpy as np


def lfilter_tdf2(b, a, x, z):
    """scipy's transposed direct form II in its order of operations; x (C, n) f64, z (C, ncoef - 1) f64 (updated in place)"""
    n = len(b) - 1
    y = np.empty_like(x)
    for t in range(x.shape[1]):
        xt = x[:, t]
        yt = z[:, 0] + b[0] * xt
        for i in range(n - 1):
            z[:, i] = z[:, i + 1] + b[i + 1] * xt - a[i + 1] * yt
        z[:, n - 1] = b[n] * xt - a[n] * yt
        y[:, t] = yt
    return y


def odd_ext(x, pad):
    """the odd extension in x's own dtype (float32 in, float32 out), as scipy.signal.filtfilt forms it"""
    front = 2 * x[:, :1] - x[:, pad:0:-1]
    back = 2 * x[:, -1:] - x[:, -2:-pad - 2:-1]
    return np.concatenate([front, x, back], axis=1)


def filtfilt_ref(b, a, zi, x):
    """x (C, L) float32 -> (C, L) float64, not yet rounded: scipy.signal.filtfilt(b, a, x, axis=1) with its defaults"""
    x = np.asarray(x, dtype=np.float32)
    pad = 3 * len(b)
    if x.shape[1] <= pad:
        raise ValueError(f"a row of {x.shape[1]} samples is not longer than the padding of {pad}")
    ext = odd_ext(x, pad).astype(np.float64)
    fwd = lfilter_tdf2(b, a, ext, zi[None, :] * ext[:, :1])
    bwd = lfilter_tdf2(b, a, fwd[:, ::-1].copy(), zi[None, :] * fwd[:, -1:])[:, ::-1]
    return bwd[:, pad:-pad]


def car_zscore_ref(x):
    """x (C, L) float32 (filtered) -> float32: common-average reference, then the per-channel z-score (population std + 1e-8),
    in eg_recording_car_zscore's arithmetic: the channel sum in float32 in channel order, mean and variance in float64 rounded
    to float32 before use"""
    x = np.asarray(x, dtype=np.float32)
    s = np.zeros(x.shape[1], np.float32)
    for c in range(x.shape[0]):
        s = s + x[c]
    v = x - (s / np.float32(x.shape[0]))[None, :]
    v64 = v.astype(np.float64)
    mean = v64.sum(axis=1, keepdims=True) / x.shape[1]
    std = np.sqrt(((v64 - mean) ** 2).sum(axis=1, keepdims=True) / x.shape[1])
    return (v - mean.astype(np.float32)) / (std.astype(np.float32) + np.float32(1e-8))


def preprocess_ref(b, a, zi, x):
    return car_zscore_ref(filtfilt_ref(b, a, zi, x).astype(np.float32))
