"""Host-side design of the recording band-pass: the coefficients of the reference's
`scipy.signal.butter(order, [low, high], 'band')` and the steady-state `lfilter_zi`, restated in numpy alone -- the package has
no scipy dependency.  The route is scipy's own, step by step (iirfilter: Butterworth prototype poles -> lp2bp_zpk -> bilinear_zpk
-> zpk2tf's np.poly), so that the coefficients are scipy's to the last bit wherever numpy's `poly` and `solve` round alike."""
from __future__ import annotations

import numpy as np

MAX_NCOEF = 17          # eg_recording_filtfilt's upper bound on len(b) == len(a)


def butter_bandpass(order: int, low_hz: float, high_hz: float, fs: float, high_clamp: float = 0.99):
    """(b, a) float64, each 2 * order + 1 long, of the digital Butterworth band-pass [low_hz, high_hz] at sampling rate fs.
    The band edges are normalised as the reference does (preprocess_eeg_windows.py:119-121): low = low_hz / (fs / 2),
    high = min(high_hz / (fs / 2), high_clamp); the entropy calculator clamps at 0.999 (entropy_calculators.py:273)."""
    if int(order) != order or order < 1:
        raise ValueError(f"butter_bandpass: order {order} must be an integer >= 1")
    order = int(order)
    if 2 * order + 1 > MAX_NCOEF:
        raise ValueError(f"butter_bandpass: order {order} gives {2 * order + 1} coefficients, more than {MAX_NCOEF}")
    if not fs > 0:
        raise ValueError(f"butter_bandpass: sampling rate {fs} must be > 0")
    nyquist = fs / 2
    low, high = low_hz / nyquist, min(high_hz / nyquist, high_clamp)
    if not low_hz > 0:
        raise ValueError(f"butter_bandpass: low edge {low_hz} Hz must be > 0")
    if not low < high:
        raise ValueError(f"butter_bandpass: band [{low_hz}, {high_hz}] Hz is empty at fs = {fs} (normalised [{low}, {high}])")
    # buttap: the prototype's poles on the unit circle (the middle one of an odd order exactly real)
    p = -np.exp(1j * np.pi * np.arange(-order + 1, order, 2) / (2 * order))
    # iirfilter: pre-warp at fs = 2
    warped = 2 * 2.0 * np.tan(np.pi * np.asarray([low, high]) / 2.0)
    bw = float(warped[1] - warped[0])
    wo = float(np.sqrt(warped[0] * warped[1]))
    # lp2bp_zpk: every pole splits in two, `order` zeros go to the origin
    p_lp = (p * bw / 2).astype(complex)
    p_bp = np.concatenate((p_lp + np.sqrt(p_lp ** 2 - wo ** 2), p_lp - np.sqrt(p_lp ** 2 - wo ** 2)))
    z_bp = np.zeros(order, dtype=complex)
    k_bp = 1 * bw ** order
    # bilinear_zpk at fs = 2: the zeros at infinity move to Nyquist
    fs2 = 4.0
    z_z = np.append((fs2 + z_bp) / (fs2 - z_bp), -np.ones(order))
    p_z = (fs2 + p_bp) / (fs2 - p_bp)
    k_z = k_bp * np.real(np.prod(fs2 - z_bp) / np.prod(fs2 - p_bp))
    # zpk2tf
    b = np.atleast_1d(k_z) * np.poly(z_z)
    a = np.atleast_1d(np.poly(p_z))
    if np.iscomplexobj(b):
        b = b.real.copy()
    if np.iscomplexobj(a):                     # np.poly returns real coefficients for conjugate pairs; rounding may leave them unpaired
        a = a.real.copy()
    return np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(a, dtype=np.float64)


def lfilter_zi(b, a):
    """scipy.signal.lfilter_zi: the state of the transposed direct form II that a unit step has settled into, the solution of
    (I - companion(a).T) zi = b[1:] - a[1:] b[0].  len(b) == len(a) >= 2 and a[0] == 1."""
    b, a = np.atleast_1d(np.asarray(b, dtype=np.float64)), np.atleast_1d(np.asarray(a, dtype=np.float64))
    if b.ndim != 1 or a.ndim != 1 or len(a) != len(b) or len(a) < 2:
        raise ValueError(f"lfilter_zi: b and a must be 1-D, equally long and >= 2 long (got {b.shape}, {a.shape})")
    if a[0] != 1.0:
        raise ValueError(f"lfilter_zi: a[0] = {a[0]} must be 1")
    n = len(a)
    companion = np.zeros((n - 1, n - 1))
    companion[0] = -a[1:] / (1.0 * a[0])
    companion[list(range(1, n - 1)), list(range(0, n - 2))] = 1
    return np.linalg.solve(np.eye(n - 1) - companion.T, b[1:] - a[1:] * b[0])
