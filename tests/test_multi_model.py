"""CPU tier: the arithmetic of libzen_hip_multi.so (zen_amd/multi/zen_hip_multi.h).  tests/multi_model.py is the contract; here
it is held against zen_amd/pcm/pcm_convert.h compiled for the host -- the functions the kernels of multi_kernels.hip call --
walked over frames by a C shim exactly as the header states the layout."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import multi_model as M  # noqa: E402
import pcm_model as P  # noqa: E402

from zen_amd import multi  # noqa: E402

SHIM = r"""
#include <stddef.h>
#include <string.h>
#include "pcm_convert.h"
void t_split_i16(const int16_t* s, int ch, size_t n, float* rows, size_t stride)
{
	for (size_t f = 0; f < n; ++f) for (int c = 0; c < ch; ++c) rows[c * stride + f] = pcm16_to_float(s[f * ch + c]);
}
void t_split_f32(const float* s, int ch, size_t n, float* rows, size_t stride)
{
	for (size_t f = 0; f < n; ++f) for (int c = 0; c < ch; ++c) memcpy(&rows[c * stride + f], &s[f * ch + c], 4);
}
void t_minmax(const float* rows, int ch, size_t n, size_t stride, float* mm)
{
	for (int c = 0; c < ch; ++c) for (size_t f = 0; f < n; ++f) { mm[0] = fminf(mm[0], rows[c * stride + f]); mm[1] = fmaxf(mm[1], rows[c * stride + f]); }
}
float t_peak_of(float mn, float mx) { return pcm16_peak_of(mn, mx); }
void t_join_i16(const float* rows, int ch, size_t n, size_t stride, int mode, float scale, int16_t* d)
{
	for (size_t f = 0; f < n; ++f) for (int c = 0; c < ch; ++c)
		d[f * ch + c] = mode == ZEN_PCM_MODE_PEAK ? float_to_pcm16_peak(rows[c * stride + f], scale) : float_to_pcm16_gain(rows[c * stride + f], scale);
}
void t_join_f32(const float* rows, int ch, size_t n, size_t stride, float* d)
{
	for (size_t f = 0; f < n; ++f) for (int c = 0; c < ch; ++c) memcpy(&d[f * ch + c], &rows[c * stride + f], 4);
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("multi_shim")
    src, so = str(d / "shim.c"), str(d / "shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                           os.path.join(ROOT, "zen_amd", "pcm"), src, "-o", so, "-lm"])
    L = C.CDLL(so)
    L.t_peak_of.restype = C.c_float
    L.t_peak_of.argtypes = [C.c_float, C.c_float]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def c_split(L, x):
    n, ch = x.shape
    rows = np.empty((ch, n), np.float32)
    (L.t_split_i16 if x.dtype == np.int16 else L.t_split_f32)(_p(x), C.c_int(ch), C.c_size_t(n), _p(rows), C.c_size_t(n))
    return rows


def c_join(L, rows, fmt, mode=M.GAIN, scale=32767.0):
    ch, n = rows.shape
    if fmt == M.F32:
        d = np.empty((n, ch), np.float32)
        L.t_join_f32(_p(rows), C.c_int(ch), C.c_size_t(n), C.c_size_t(n), _p(d))
    else:
        d = np.empty((n, ch), np.int16)
        L.t_join_i16(_p(rows), C.c_int(ch), C.c_size_t(n), C.c_size_t(n), C.c_int(mode), C.c_float(scale), _p(d))
    return d


def c_peak(L, rows):
    rows = np.ascontiguousarray(rows, np.float32)
    mm = np.array([np.inf, -np.inf], np.float32)
    L.t_minmax(_p(rows), C.c_int(rows.shape[0]), C.c_size_t(rows.shape[1]), C.c_size_t(rows.shape[1]), _p(mm))
    return mm, np.float32(L.t_peak_of(C.c_float(mm[0]), C.c_float(mm[1])))


def test_the_bindings_constants_are_the_models_and_the_pcm_headers():
    assert (multi.I16, multi.F32, multi.PEAK, multi.GAIN) == (M.I16, M.F32, M.PEAK, M.GAIN) == (0, 1, 0, 1)
    hdr = open(os.path.join(ROOT, "zen_amd", "pcm", "pcm_convert.h")).read()
    assert "ZEN_PCM_MODE_PEAK = 0, ZEN_PCM_MODE_GAIN = 1" in hdr
    assert multi.MAX_CHANNELS == 8


@pytest.mark.parametrize("ch", range(1, 9))
def test_float_round_trip_is_bitwise_with_nan_payloads(shim, ch):
    rng = np.random.default_rng(ch)
    bits = rng.integers(0, 1 << 32, (1003, ch), dtype=np.uint64).astype(np.uint32)
    bits[:6, 0] = [0x7fc00000, 0x7fa00001, 0xffc12345, 0x7f800001, 0x80000000, 0x00000001]    # quiet and signalling NaNs, -0, a denormal
    x = bits.view(np.float32)
    rows = M.split(x)
    assert rows.shape == (ch, 1003) and np.array_equal(rows.view(np.uint32), bits.T)
    back = M.join(rows, M.F32, mode=M.PEAK)             # the mode is ignored
    assert np.array_equal(back.view(np.uint32), bits)
    assert np.array_equal(c_split(shim, x).view(np.uint32), rows.view(np.uint32))
    assert np.array_equal(c_join(shim, rows, M.F32).view(np.uint32), bits)


@pytest.mark.parametrize("ch", (1, 2, 3, 8))
def test_all_65536_int16_values_through_split_and_gain_join(shim, ch):
    all16 = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    n = -(-all16.size // ch)
    x = np.resize(all16, n * ch).reshape(n, ch)
    rows = M.split(x)
    assert np.array_equal(rows, (np.float32(x) / np.float32(32767)).T)
    assert np.array_equal(c_split(shim, x), rows)
    back = M.join(rows, M.I16, M.GAIN, 32767.0)
    assert np.array_equal(back, x) and np.array_equal(c_join(shim, rows, M.I16, M.GAIN, 32767.0), x)


def test_one_peak_per_stem_over_all_its_channels(shim):
    rng = np.random.default_rng(9)
    rows = rng.uniform(-1000, 1000, (3, 777)).astype(np.float32)
    rows[2, 500] = -5000.25                              # the peak sits in a channel other than 0
    rows[1, 3] = 4000.5
    assert M.minmax(rows) == (np.float32(-5000.25), np.float32(4000.5)) and M.peak(rows) == np.float32(5000.25)
    mm, pk = c_peak(shim, rows)
    assert mm.tolist() == [-5000.25, 4000.5] and pk == M.peak(rows)
    got = M.join(rows, M.I16, M.PEAK)
    assert np.array_equal(got, c_join(shim, rows, M.I16, M.PEAK, pk))
    assert got[500, 2] == -32767 and np.abs(got[:, :2].astype(np.int32)).max() < 32767 * 0.81   # channels 0 and 1 keep their level below channel 2
    for c in range(3):                                   # every channel divided by the same number: not by its own peak
        assert np.array_equal(got[:, c], P.from_float_peak(rows[c], np.float32(5000.25)))
    assert not np.array_equal(got[:, 0], P.from_float_peak(rows[0], P.peak_of(rows[0])))
    # NaNs are ignored by the peak and narrow to 0
    rows[0, ::5] = np.nan
    mm, pk = c_peak(shim, rows)
    assert pk == M.peak(rows) == np.float32(5000.25)
    got = M.join(rows, M.I16, M.PEAK)
    assert np.array_equal(got, c_join(shim, rows, M.I16, M.PEAK, pk)) and not got[::5, 0].any()
    # all zeros: the peak is 0 and the output zeros; nothing but NaNs: the same
    z = np.zeros((2, 64), np.float32)
    mm, pk = c_peak(shim, z)
    assert M.peak(z) == 0 and pk == 0 and not M.join(z, M.I16, M.PEAK).any() and not c_join(shim, z, M.I16, M.PEAK, pk).any()
    nn = np.full((2, 8), np.nan, np.float32)
    assert M.peak(nn) == 0 and not M.join(nn, M.I16, M.PEAK).any()
    # C = 1: the PCM model's peak, i.e. what `zen offline` normalises by
    one = rows[1:2]
    assert M.peak(one) == P.peak_of(one[0]) and np.array_equal(M.join(one, M.I16, M.PEAK)[:, 0], P.from_float_peak(one[0], P.peak_of(one[0])))


def test_the_minmax_reduction_has_the_same_bits_in_any_order(shim):
    rng = np.random.default_rng(10)
    rows = rng.uniform(-3, 3, (4, 4099)).astype(np.float32)
    want = M.minmax(rows)
    for seed in range(4):
        perm = np.random.default_rng(seed).permutation(rows.size)
        shuffled = rows.ravel()[perm].reshape(4, -1)
        mm, _ = c_peak(shim, shuffled)
        assert (mm[0], mm[1]) == want


def test_convert_functions_on_the_host_agree_with_the_model_in_both_modes(shim):
    rng = np.random.default_rng(11)
    rows = rng.uniform(-2.9e4, 2.9e4, (5, 20011)).astype(np.float32)
    rows[:, :4] = [0.0, -0.0, 3e4, -3.1e4]
    rows[3, 7:10] = [np.inf, -np.inf, np.nan]
    pk = M.peak(rows)
    assert pk == np.float32(np.inf)
    rows[3, 7:9] = [1.5, -2.5]
    pk = M.peak(rows)
    assert pk == np.float32(3.1e4)
    assert np.array_equal(c_join(shim, rows, M.I16, M.PEAK, pk), M.join(rows, M.I16, M.PEAK))
    for gain in (32767.0 / 3.1e4, 2 * 32767.0 / 3.1e4, 1.0, 0.37):
        got = c_join(shim, rows, M.I16, M.GAIN, gain)
        assert np.array_equal(got, M.join(rows, M.I16, M.GAIN, gain)), gain
    sat = M.join(rows, M.I16, M.GAIN, 2 * 32767.0 / 3.1e4)
    assert (sat == 32767).any() and (sat == -32768).any()


def test_stems_model_normalises_each_stem_once():
    x = (np.random.default_rng(12).uniform(-0.5, 0.5, (300, 2)) * 32767).astype(np.int16)
    sep = lambda r: (r * np.float32(0.5), r - r * np.float32(0.5))  # noqa: E731
    out, peaks = M.stems(x, sep)
    rows = M.split(x)
    assert peaks[0] == M.peak(rows * np.float32(0.5)) and out["harm"].shape == x.shape and out["harm"].dtype == np.int16
    assert np.abs(out["harm"].astype(np.int32)).max() == 32767
    out, peaks = M.stems(x.astype(np.float32), sep)
    assert not peaks.any() and np.array_equal(out["harm"], (x.astype(np.float32) * np.float32(0.5)))
