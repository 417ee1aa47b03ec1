"""CPU tier: the 24-bit half of zen_amd/pcm/pcm_convert.h -- the arithmetic the packed-24-bit kernels of libzen_hip_pcm.so
run -- compiled for the host as C99 and compared with the numpy model of tests/pcm24_model.py, value for value; and the
same functions once more in a stand-alone C program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import pcm24_model as M  # noqa: E402

SHIM = r"""
#include <stddef.h>
#include "pcm_convert.h"
void t_load(const uint8_t* p, size_t n, int32_t* d) { for (size_t i = 0; i < n; ++i) d[i] = pcm24_load(p + 3 * i); }
void t_store(const int32_t* v, size_t n, uint8_t* p) { for (size_t i = 0; i < n; ++i) pcm24_store(p + 3 * i, v[i]); }
void t_to_float(const int32_t* v, size_t n, float* d) { for (size_t i = 0; i < n; ++i) d[i] = pcm24_to_float(v[i]); }
void t_stereo(const int32_t* v, size_t n, float* d) { for (size_t i = 0; i < n; ++i) d[i] = pcm24_stereo_to_mono(v[2 * i], v[2 * i + 1]); }
void t_from_float(const float* x, size_t n, int32_t* d) { for (size_t i = 0; i < n; ++i) d[i] = float_to_pcm24(x[i]); }
void t_peak(const float* y, size_t n, float peak, int32_t* d) { for (size_t i = 0; i < n; ++i) d[i] = float_to_pcm24_peak(y[i], peak); }
void t_gain(const float* y, size_t n, float gain, int32_t* d) { for (size_t i = 0; i < n; ++i) d[i] = float_to_pcm24_gain(y[i], gain); }
int t_sample_bytes(int fmt) { return pcm_sample_bytes(fmt); }
"""

# The stand-alone program: the boundary list and a strided sweep of the codes through every 24-bit function, with the
# answers worked out in integer arithmetic beside them; any sanitizer report ends it with a status that is not 0.
SAN_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "pcm_convert.h"
static int fails = 0;
static void expect(int32_t got, int32_t want, const char* what, double v)
{
	if (got != want) {
		fprintf(stderr, "%s(%.9g): got %d, want %d\n", what, v, (int)got, (int)want);
		++fails;
	}
}
int main(void)
{
	static const float v[] = {0.5f, -0.5f, 1.5f, -1.5f, 0.49999997f, -0.49999997f, 4194303.5f, -4194303.5f, 8388606.5f, -8388606.5f,
	                          8388607.5f, 8388607.f, 8388608.f, -8388608.f, -8388609.f, 1e10f, -1e10f, INFINITY, -INFINITY, NAN, -0.0f, 1e-45f};
	static const int32_t want[] = {1, -1, 2, -2, 0, 0, 4194304, -4194304, 8388607, -8388607,
	                               8388607, 8388607, 8388607, -8388608, -8388608, 8388607, -8388608, 8388607, -8388608, 0, 0, 0};
	uint8_t* heap = (uint8_t*)malloc(3); /* exactly three bytes: a load or store that touches a fourth is reported */
	size_t i;
	int32_t k;
	if (!heap)
		return 2;
	for (i = 0; i < sizeof(v) / sizeof(v[0]); ++i) {
		expect(float_to_pcm24_gain(v[i], 1.0f), want[i], "gain", v[i]);
		expect(float_to_pcm24_peak(v[i], 8388608.f), want[i], "peak", v[i]);
		expect(float_to_pcm24(v[i] / 8388608.f), want[i], "plain", v[i]);
		expect(float_to_pcm24_peak(v[i], 0.f), 0, "peak0", v[i]);
	}
	for (k = -8388608; k <= 8388607 + 4098; k += 4099) { /* a stride coprime to 2^24, and the last code */
		const int32_t c = k > 8388607 ? 8388607 : k;
		pcm24_store(heap, c);
		expect(pcm24_load(heap), c, "store/load", c);
		expect(float_to_pcm24(pcm24_to_float(c)), c, "round trip", c);
	}
	pcm24_store(heap, -1);           /* values outside 24 bits: the low three bytes, no shift of a negative value */
	expect(pcm24_load(heap), -1, "store/load", -1);
	pcm24_store(heap, INT32_MIN);
	expect(pcm24_load(heap), 0, "store/load", (double)INT32_MIN);
	pcm24_store(heap, INT32_MAX);
	expect(pcm24_load(heap), -1, "store/load", (double)INT32_MAX);
	if (pcm24_stereo_to_mono(8388607, 8388606) != 16777213.f / 16777216.f || pcm_sample_bytes(1) != 3)
		++fails;
	free(heap);
	return fails ? 1 : 0;
}
"""

CFLAGS = ["-std=c99", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "zen_amd", "pcm")]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("pcm24_shim")
    src, so = str(d / "shim.c"), str(d / "shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    # as C99, with the flags the header asks of every file that includes it
    subprocess.check_call(["gcc"] + CFLAGS + ["-fPIC", "-shared", src, "-o", so, "-lm"])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def c_call(fn, src, out_dtype, *scalars):
    src = np.ascontiguousarray(src)
    d = np.empty(src.size, out_dtype)
    fn(_p(src), C.c_size_t(src.size), *scalars, _p(d))
    return d


@pytest.fixture(scope="module")
def all24():
    """every code once, and its packed bytes by the model"""
    k = np.arange(M.LO, M.HI + 1, dtype=np.int32)
    return k, M.store(k)


def test_all_codes_load_and_widen(shim, all24):
    k, packed = all24
    got = np.empty(k.size, np.int32)
    shim.t_load(_p(packed), C.c_size_t(k.size), _p(got))
    assert np.array_equal(got, k) and np.array_equal(M.load(packed), k)
    f = c_call(shim.t_to_float, k, np.float32)
    assert np.array_equal(f, M.to_float(k))
    assert np.array_equal(f.astype(np.float64) * 8388608.0, k.astype(np.float64))        # exact for every code


def test_round_trip_is_the_identity_for_all_codes(shim, all24):
    k, _ = all24
    f = M.to_float(k)
    assert np.array_equal(c_call(shim.t_from_float, f, np.int32), k)
    assert np.array_equal(M.from_float(f), k)


def test_store_then_load_is_the_identity_for_all_codes(shim, all24):
    k, packed = all24
    b = np.zeros(3 * k.size, np.uint8)
    shim.t_store(_p(k), C.c_size_t(k.size), _p(b))
    assert np.array_equal(b, packed)
    back = np.empty(k.size, np.int32)
    shim.t_load(_p(b), C.c_size_t(k.size), _p(back))
    assert np.array_equal(back, k)


def test_boundaries_and_specials_plain_peak_and_gain(shim):
    v = M.boundary_values()
    want = M.from_float_gain(v, 1.0)
    # the model's own answers for the values the issue names, in its order
    assert want[:20].tolist() == [1, -1, 2, -2, 0, 0, 4194304, -4194304, 8388607, -8388607, 8388607, 8388607, 8388607, -8388608,
                                  -8388608, 8388607, -8388608, 8388607, -8388608, 0] and not want[20:].any()
    assert np.array_equal(c_call(shim.t_gain, v, np.int32, C.c_float(1.0)), want)
    assert np.array_equal(c_call(shim.t_peak, v, np.int32, C.c_float(8388608.0)), want)
    assert np.array_equal(M.from_float_peak(v, 8388608.0), want)
    with np.errstate(invalid="ignore"):
        x = (v / M.SCALE).astype(np.float32)
    assert np.array_equal(c_call(shim.t_from_float, x, np.int32), M.from_float(x))
    assert np.array_equal(M.from_float(x)[:20], want[:20])
    # a peak that is no power of two, and silence
    for peak in (3.0, 0.37, 8388607.0):
        y = (v * np.float32(peak) / M.SCALE).astype(np.float32)
        assert np.array_equal(c_call(shim.t_peak, y, np.int32, C.c_float(peak)), M.from_float_peak(y, peak)), peak
    assert not c_call(shim.t_peak, v, np.int32, C.c_float(0.0)).any()
    assert [shim.t_sample_bytes(f) for f in (0, 1, 2, -1)] == [2, 3, 0, 0]


def test_half_integer_neighbourhoods(shim):
    """k + 1/2 and its float32 neighbours around zero, around 2^22 (where the spacing of binary32 becomes 1/2) and up to
    full scale, both signs"""
    top = np.concatenate([np.arange(4194304 - 70000, 4194304 + 70000), np.arange(8388608 - 70000, 8388608)])
    k = np.concatenate([np.arange(-70000, 70001), top, -top - 1]).astype(np.float64)
    c = (k + .5).astype(np.float32)
    vs = [c, np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))]
    v = np.concatenate(vs)
    assert np.array_equal(c_call(shim.t_gain, v, np.int32, C.c_float(1.0)), M.from_float_gain(v, 1.0))
    x = (v / M.SCALE).astype(np.float32)
    assert np.array_equal(c_call(shim.t_from_float, x, np.int32), M.from_float(x))


def test_ten_million_random_floats(shim):
    rng = np.random.default_rng(5)
    for i in range(5):
        x = rng.uniform(-1.2, 1.2, 2 * 10 ** 6 + 1).astype(np.float32)
        if i == 4:
            x = (x * np.float32(2.0 ** -9)).astype(np.float32)     # low levels: where the fraction has bits to round
        assert np.array_equal(c_call(shim.t_from_float, x, np.int32), M.from_float(x))
    y = rng.uniform(-2.9e4, 2.9e4, 1 << 20).astype(np.float32)
    assert np.array_equal(c_call(shim.t_peak, y, np.int32, C.c_float(2.9e4)), M.from_float_peak(y, 2.9e4))
    for gain in (8388608.0 / 2.9e4, 2 * 8388608.0 / 2.9e4, 0.37):
        assert np.array_equal(c_call(shim.t_gain, y, np.int32, C.c_float(gain)), M.from_float_gain(y, gain)), gain
    d = c_call(shim.t_gain, y, np.int32, C.c_float(2 * 8388608.0 / 2.9e4))
    assert (d == M.HI).sum() > 10 and (d == M.LO).sum() > 10 and (np.abs(d) < M.HI).sum() > 1000


def test_stereo_mix_at_full_scale_with_an_odd_sum(shim):
    rng = np.random.default_rng(3)
    lr = rng.integers(M.LO, M.HI + 1, 2 * 100000).astype(np.int32)
    lr[:10] = [M.HI, M.HI - 1, M.LO, M.LO + 1, M.HI, M.HI, M.LO, M.LO, M.HI, M.LO]
    d = np.empty(lr.size // 2, np.float32)
    shim.t_stereo(_p(lr), C.c_size_t(d.size), _p(d))
    f = np.float32(lr) / np.float32(8388608)
    assert np.array_equal(d, (f[0::2] + f[1::2]) / np.float32(2.0))
    assert np.array_equal(d, M.stereo_mix(lr))
    # 2^24 - 3 and -(2^24 - 1) have 24 significant bits: the sum and its half are exact
    assert d[0] == np.float32(16777213.0 / 16777216.0) and d[1] == np.float32(-16777215.0 / 16777216.0)
    assert np.array_equal(M.widen(M.store(lr), 2), d)


def test_standalone_program_under_the_sanitizers(tmp_path):
    """the only sanitized code of this work: a C program of its own, run directly"""
    src, exe = tmp_path / "san_main.c", tmp_path / "san_main"
    src.write_text(SAN_MAIN)
    subprocess.check_call(["gcc"] + CFLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", str(src), "-o", str(exe), "-lm"])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
