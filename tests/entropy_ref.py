"""TEST INFRASTRUCTURE -- a numpy restatement of both entropies of the entropy analysis in the closed form the
device uses, with no scipy: q = |v| + eps, S = sum q, T = sum q ln q, H = (ln S - T / S) / ln 2.  The zero-phase filter comes from
tests/recprep_ref, the Welch PSD from tests/trialfeat_ref, the coefficients from eyegaze_multimodal_amd.entropy."""
import numpy as np

from eyegaze_multimodal_amd import entropy as E
from eyegaze_multimodal_amd.filters import lfilter_zi
from tests import recprep_ref as R
from tests import trialfeat_ref as T

EPS = 1e-10


def shannon_bits(v, eps=EPS):
    """the closed form over the last axis, float64; a q of 0 adds nothing (scipy's entr)"""
    q = np.abs(np.asarray(v, np.float64)) + eps
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(q == 0, 0.0, q * np.log(q))
        S = q.sum(axis=-1)
        return (np.log(S) - t.sum(axis=-1) / S) / np.log(2.0)


def filtered_ref(x, fs=250.0, low=0.5, high=50.0, order=4, round32=True):
    """the calculator's band-pass of a (C, L) float32 recording; round32: rounded to float32 as the device's row store rounds it"""
    b, a = E.entropy_band_coefficients(low, high, fs, order)
    y = R.filtfilt_ref(b, a, lfilter_zi(b, a), np.asarray(x, np.float32))
    return y.astype(np.float32) if round32 else y


def spectral_entropy_of_rows(rows, fs=250.0, eps=EPS):
    """(C, L) rows as they are (no filter) -> (C,) bits"""
    return shannon_bits(T.welch_ref(np.asarray(rows), fs), eps)


def spectral_entropy_ref(x, fs=250.0, low=0.5, high=50.0, order=4, apply_filter=True, round32=True):
    """SpectralEntropyCalculator.compute for one (C, L) float32 recording"""
    rows = filtered_ref(x, fs, low, high, order, round32) if apply_filter else np.asarray(x, np.float32)
    return spectral_entropy_of_rows(rows, fs)


def grayscale_ref(image):
    """_to_grayscale as float64 values, flat: numpy's (0.299 R + 0.587 G) + 0.114 B"""
    image = np.asarray(image)
    lay = E.image_layout(image.shape)
    if lay == E.GREY:
        return image.astype(np.float64).reshape(-1)
    if lay == E.PLANAR:
        image = np.transpose(image, (1, 2, 0))
    return (0.299 * image[:, :, 0] + 0.587 * image[:, :, 1] + 0.114 * image[:, :, 2]).astype(np.float64).reshape(-1)


def spatial_entropy_ref(image, normalize=True, eps=EPS):
    """SpatialEntropyCalculator.compute for one uint8 or float64 image"""
    g = grayscale_ref(image)
    if normalize:
        g = (g - g.min()) / (g.max() - g.min() + 1e-10)
    return float(shannon_bits(g, eps))
