"""float64 numpy model of zen_amd/pcm/pcm_convert.h, shared by tests/test_pcm_model.py (CPU) and tests/test_gpu_pcm.py.

Every intermediate the C code rounds to binary32 is rounded to float32 here by an explicit astype; the rounding to an
integer is done in float64, where v + 0.5 is exact for every binary32 v in the int16 range."""
import numpy as np

F = np.float32


def to_float(s):
    """wav.h:77-78: (float)s / 32767.f"""
    return np.asarray(s, np.int16).astype(F) / F(32767)


def stereo_mix(interleaved):
    """wav.h:101-105 on widened samples: (L + R) / 2.0f"""
    f = to_float(interleaved)
    return ((f[0::2] + f[1::2]).astype(F) / F(2)).astype(F)


def round_sat(v32):
    """halves away from zero, saturated to int16, NaN -> 0"""
    v = np.asarray(v32, F).astype(np.float64)
    with np.errstate(invalid="ignore"):
        r = np.where(v >= 0, np.floor(v + .5), np.ceil(v - .5))
    r = np.where(np.isnan(v), 0.0, r)
    return np.clip(r, -32768, 32767).astype(np.int16)


def from_float(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return round_sat((np.asarray(x, F) * F(32767)).astype(F))


def peak_of(y):
    y = np.asarray(y, F)
    return F(max(-1 * np.min(y), np.max(y))) if y.size else F(0)


def from_float_peak(y, peak):
    y = np.asarray(y, F)
    if F(peak) == 0:
        return np.zeros(y.shape, np.int16)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return from_float((y / F(peak)).astype(F))


def from_float_gain(y, gain):
    with np.errstate(over="ignore", invalid="ignore"):
        return round_sat((np.asarray(y, F) * F(gain)).astype(F))
