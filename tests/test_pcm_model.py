"""CPU tier: zen_amd/pcm/pcm_convert.h -- the arithmetic the kernels of libzen_hip_pcm.so run -- compiled for the host and
compared with the float64 numpy model of tests/pcm_model.py, value for value."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import pcm_model as M  # noqa: E402

SHIM = r"""
#include <stddef.h>
#include "pcm_convert.h"
void t_to_float(const int16_t* s, size_t n, float* d) { for (size_t i = 0; i < n; ++i) d[i] = pcm16_to_float(s[i]); }
void t_stereo(const int16_t* s, size_t n, float* d) { for (size_t i = 0; i < n; ++i) d[i] = stereo_to_mono(s[2 * i], s[2 * i + 1]); }
void t_from_float(const float* x, size_t n, int16_t* d) { for (size_t i = 0; i < n; ++i) d[i] = float_to_pcm16(x[i]); }
void t_peak(const float* y, size_t n, float peak, int16_t* d) { for (size_t i = 0; i < n; ++i) d[i] = float_to_pcm16_peak(y[i], peak); }
void t_gain(const float* y, size_t n, float gain, int16_t* d) { for (size_t i = 0; i < n; ++i) d[i] = float_to_pcm16_gain(y[i], gain); }
float t_peak_of(float mn, float mx) { return pcm16_peak_of(mn, mx); }
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("pcm_shim")
    src, so = str(d / "shim.c"), str(d / "shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    # as C99, with the flags the header asks of every file that includes it
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                           os.path.join(ROOT, "zen_amd", "pcm"), src, "-o", so, "-lm"])
    L = C.CDLL(so)
    L.t_peak_of.restype = C.c_float
    L.t_peak_of.argtypes = [C.c_float, C.c_float]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def c_from_float(L, x):
    x = np.ascontiguousarray(x, np.float32)
    d = np.empty(x.size, np.int16)
    L.t_from_float(_p(x), C.c_size_t(x.size), _p(d))
    return d


ALL16 = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)


def test_pcm16_to_float_all_65536_values(shim):
    d = np.empty(ALL16.size, np.float32)
    shim.t_to_float(_p(ALL16), C.c_size_t(ALL16.size), _p(d))
    assert np.array_equal(d, np.float32(ALL16) / np.float32(32767))
    assert np.array_equal(d, M.to_float(ALL16))


def test_round_trip_is_the_identity_for_all_65536_values(shim):
    assert np.array_equal(c_from_float(shim, M.to_float(ALL16)), ALL16)
    assert np.array_equal(M.from_float(M.to_float(ALL16)), ALL16)


def test_stereo_mix_is_wav_h_formula_in_float32(shim):
    rng = np.random.default_rng(3)
    lr = rng.integers(-32768, 32768, 2 * 100000).astype(np.int16)
    lr[:8] = [32767, 32767, -32768, -32768, 32767, -32768, 1, 0]
    d = np.empty(lr.size // 2, np.float32)
    shim.t_stereo(_p(lr), C.c_size_t(d.size), _p(d))
    f = np.float32(lr) / np.float32(32767)
    assert np.array_equal(d, (f[0::2] + f[1::2]) / np.float32(2.0))
    assert np.array_equal(d, M.stereo_mix(lr))


def boundary_values():
    """for k in -40000..40000: the float32 nearest to (k + 1/2) / 32767 and its two neighbours on each side"""
    k = np.arange(-40000, 40001, dtype=np.float64)
    c = ((k + .5) / 32767.0).astype(np.float32)
    out = [c]
    lo = hi = c
    for _ in range(2):
        lo = np.nextafter(lo, np.float32(-np.inf))
        hi = np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return np.concatenate(out)


def special_values():
    f = np.float32
    tiny = np.finfo(np.float32).tiny
    half = f(0.49999997) / f(32767)
    v = [0.0, -0.0, half, -half, f(0.49999997), -f(0.49999997), f(0.5) / f(32767), -f(0.5) / f(32767), 1.0, -1.0, 1.0000305, -1.0000305,
         2.0, -2.0, np.inf, -np.inf, np.nan, tiny, -tiny, tiny / 4, -tiny / 4, f(1e-45), -f(1e-45), 3.4e38, -3.4e38,
         f(32767.5) / f(32767), -f(32768.5) / f(32767), f(32768) / f(32767), -f(32768) / f(32767)]
    return np.array(v, np.float32)


def test_float_to_pcm16_boundaries_and_specials(shim):
    x = np.concatenate([special_values(), boundary_values()])
    got, want = c_from_float(shim, x), M.from_float(x)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (x[bad[:5]], got[bad[:5]], want[bad[:5]])
    # the value floorf(v + 0.5f) gets wrong: 0.49999997f rounds to 0, not 1
    v = np.array([0.49999997, -0.49999997, 0.5, -0.5, 1.4999999, 2.5], np.float32)
    d = np.empty(v.size, np.int16)
    shim.t_gain(_p(v), C.c_size_t(v.size), C.c_float(1.0), _p(d))
    assert d.tolist() == [0, 0, 1, -1, 1, 3]
    s = c_from_float(shim, np.array([np.nan, np.inf, -np.inf, 2.0, -2.0, 1.0, -1.0, 1.0000305, -1.0000305], np.float32))
    assert s.tolist() == [0, 32767, -32768, 32767, -32768, 32767, -32767, 32767, -32768]


def test_float_to_pcm16_agrees_with_the_wrapping_encoder_below_full_scale(shim):
    """wav.h:132 is (int16) lroundf(x * 32767.f): identical wherever |x * 32767| < 32767.5"""
    rng = np.random.default_rng(11)
    x = rng.uniform(-1.2, 1.2, 1 << 20).astype(np.float32)
    v = (x * np.float32(32767)).astype(np.float32).astype(np.float64)
    wrap = np.where(v >= 0, np.floor(v + .5), np.ceil(v - .5)).astype(np.int64).astype(np.int16)   # modulo 2^16
    inside = np.abs(v) < 32767.5
    got = c_from_float(shim, x)
    assert np.array_equal(got[inside], wrap[inside]) and inside.sum() > 800000
    assert np.all(np.abs(got[~inside].astype(np.int32)) >= 32767)


def test_float_to_pcm16_ten_million_random(shim):
    rng = np.random.default_rng(5)
    for _ in range(5):
        x = rng.uniform(-1.2, 1.2, 2 * 10 ** 6 + 1).astype(np.float32)
        assert np.array_equal(c_from_float(shim, x), M.from_float(x))


def test_peak_and_gain_scalings(shim):
    rng = np.random.default_rng(7)
    y = rng.uniform(-2.9e4, 2.9e4, 1 << 20).astype(np.float32)
    y[:4] = [0.0, -0.0, 3e4, -3.1e4]
    peak = M.peak_of(y)
    assert peak == np.float32(3.1e4) and shim.t_peak_of(np.min(y), np.max(y)) == peak
    d = np.empty(y.size, np.int16)
    shim.t_peak(_p(y), C.c_size_t(y.size), C.c_float(peak), _p(d))
    assert np.array_equal(d, M.from_float_peak(y, peak))
    assert d.min() == -32767 and d.max() < 32767
    for gain in (32767.0 / 3.1e4, 2 * 32767.0 / 3.1e4, 1.0, 0.37):
        shim.t_gain(_p(y), C.c_size_t(y.size), C.c_float(gain), _p(d))
        assert np.array_equal(d, M.from_float_gain(y, gain)), gain
    shim.t_gain(_p(y), C.c_size_t(y.size), C.c_float(2 * 32767.0 / 3.1e4), _p(d))
    assert (d == 32767).sum() > 10 and (d == -32768).sum() > 10 and (np.abs(d.astype(np.int32)) < 32767).sum() > 1000
    # silence: the command line tool divides 0 by 0; PEAK mode writes zeros
    z = np.zeros(64, np.float32)
    shim.t_peak(_p(z), C.c_size_t(64), C.c_float(0.0), _p(d))
    assert not d[:64].any()


def test_boundaries_through_the_peak_path(shim):
    """x = y / peak lands on the same half-integer neighbourhoods when peak is a power of two"""
    x = boundary_values()
    y = (x * np.float32(16384)).astype(np.float32)
    d = np.empty(y.size, np.int16)
    shim.t_peak(_p(y), C.c_size_t(y.size), C.c_float(16384.0), _p(d))
    assert np.array_equal(d, M.from_float_peak(y, 16384.0))
    assert np.array_equal(d, M.from_float(x))
