"""float64 numpy model of the 24-bit half of zen_amd/pcm/pcm_convert.h, shared by tests/test_pcm24_model.py (CPU) and
tests/test_gpu_pcm24.py, in the style of tests/pcm_model.py.

Every intermediate the C code rounds to binary32 is rounded to float32 here by an explicit astype; the rounding to an
integer is done in float64, where v + 0.5 is exact for every binary32 v in the 24-bit range.  Packed samples are uint8
arrays of three little-endian bytes per sample; codes are int32."""
import numpy as np

F = np.float32
SCALE = F(8388608)            # 2^23: the reader's divisor (zen_amd/cli/wav.h:85) and the writer's multiplier
LO, HI = -8388608, 8388607


def load(b):
    """three little-endian bytes per sample -> sign-extended int32 codes"""
    b = np.asarray(b, np.uint8).reshape(-1, 3)
    u = b[:, 0].astype(np.int32) + 256 * b[:, 1].astype(np.int32) + 65536 * b[:, 2].astype(np.int32)
    return np.where(u >= 1 << 23, u - (1 << 24), u).astype(np.int32)


def store(v):
    """int32 codes -> three little-endian bytes per sample: the value modulo 2^24"""
    u = (np.asarray(v, np.int64).reshape(-1) % (1 << 24)).astype(np.uint32)
    out = np.empty((u.size, 3), np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = u % 256, (u // 256) % 256, u // 65536
    return out.reshape(-1)


def to_float(v):
    """wav.h:85: (float)v / 8388608.f"""
    return (np.asarray(v, np.int32).astype(F) / SCALE).astype(F)


def stereo_mix(interleaved):
    """wav.h:101-105 on widened samples: (L + R) / 2.0f"""
    f = to_float(interleaved)
    return ((f[0::2] + f[1::2]).astype(F) / F(2)).astype(F)


def widen(packed, channels=1):
    """packed bytes of `channels` interleaved samples -> the floats the engines are fed"""
    v = load(packed)
    return to_float(v) if channels == 1 else stereo_mix(v)


def round_sat(v32):
    """halves away from zero, saturated to 24 bits, NaN -> 0"""
    v = np.asarray(v32, F).astype(np.float64)
    with np.errstate(invalid="ignore"):
        r = np.where(v >= 0, np.floor(v + .5), np.ceil(v - .5))
    r = np.where(np.isnan(v), 0.0, r)
    return np.clip(r, LO, HI).astype(np.int32)


def from_float(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return round_sat((np.asarray(x, F) * SCALE).astype(F))


def peak_of(y):
    y = np.asarray(y, F)
    return F(max(-1 * np.min(y), np.max(y))) if y.size else F(0)


def from_float_peak(y, peak):
    y = np.asarray(y, F)
    if F(peak) == 0:
        return np.zeros(y.shape, np.int32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return from_float((y / F(peak)).astype(F))


def from_float_gain(y, gain):
    with np.errstate(over="ignore", invalid="ignore"):
        return round_sat((np.asarray(y, F) * F(gain)).astype(F))


def boundary_values():
    """the values v at which the rounding or the saturation decides, as float32 (the issue's list), for GAIN with gain 1
    and for PEAK with peak 2^23 / plain with x = v / 2^23 (the division and the product by a power of two are exact)"""
    f = F
    tiny = np.finfo(F).tiny
    v = [0.5, -0.5, 1.5, -1.5, f(0.49999997), -f(0.49999997), 4194303.5, -4194303.5, 8388606.5, -8388606.5, 8388607.5,
         8388607, 8388608, -8388608, -8388609, 1e10, -1e10, np.inf, -np.inf, np.nan, -0.0, 0.0, tiny / 4, -tiny / 4, f(1e-45)]
    return np.array(v, F)
