"""CPU tier: tests/repet_model.py -- the model the GPU tier compares libzen_hip_repet.so with bit for bit -- against REPET as
the paper writes it, in float64 with numpy.fft, written out below: the spectrogram, the beat spectrum, the repeating segment
and both outputs.  The parity target is that independent computation, never the library.  Then the properties of the median
rule, of a strictly periodic clip, and the quality condition on the synthetic family of DESIGN.md section 17."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import repet_model as M  # noqa: E402

FS = M.FAMILY_FS
# The largest deviations measured on PARITY below, each relative to the largest magnitude of the float64 quantity
# (DESIGN.md section 17 lists them), times 4:
TOL = {"V": 4 * 1.16e-7, "b": 4 * 1.07e-6, "S": 4 * 1.35e-7, "background": 4 * 2.25e-7, "foreground": 4 * 1.46e-6}
PARITY = [c for c in M.FAMILY if c[0] == 0]      # the five shapes of the family, seed 0


# ------------------------------------------------------------------------------------------------ float64 REPET
def ref_repet(x, fs, N, p, highpass=M.HIGHPASS):
    """V, b (the normalised beat spectrum), S, background, foreground in float64"""
    x = np.asarray(x, np.float64)
    H, n = N // 2, x.size
    m = -(-n // H) + 1
    w = 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(N) / N)
    xp = np.concatenate([np.zeros(H), x, np.zeros((m + 1) * H - H - n)])
    X = np.fft.fft(np.stack([xp[k * H:k * H + N] * w for k in range(m)]), axis=1)
    V = np.abs(X[:, :H + 1])
    L = 64
    while L < 2 * m:
        L *= 2
    P = np.abs(np.fft.fft(V * V, L, axis=0)) ** 2
    a = np.fft.ifft(P, axis=0).real[:m] * L                  # the engine's inverse transform is unnormalised
    braw = (a / (m - np.arange(m))[:, None]).sum(axis=1)
    b = braw / braw[0]
    S = np.stack([np.median(V[l::p], axis=0) for l in range(p)])
    Sk = S[np.arange(m) % p]
    Mk = np.where(V > 0, np.minimum(Sk, V) / np.where(V > 0, V, 1.0), 0.0)
    kc = int(math.ceil(highpass * N / fs)) if highpass > 0 else 0
    Mk[:, :kc] = 1.0
    full = np.concatenate([Mk, Mk[:, 1:H][:, ::-1]], axis=1)
    G = np.fft.ifft(X * full, axis=1).real * N
    d = N * (w[:H] + w[H:])
    t = np.arange(n)
    bg = (G[t // H, H + t % H] + G[t // H + 1, t % H]) / d[t % H]
    return V, b, S, bg, x - bg


def rel(got, ref):
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref)) / np.max(np.abs(ref)))


@pytest.fixture(scope="module")
def family(oracle):
    """every clip of the family with the model's result: the period found, and the outputs with the true period"""
    oracle.lib()
    out = {}
    for key in M.FAMILY:
        seed, N, P, R = key
        x, bg, fg = M.family_clip(seed, N, P, R)
        tmin, tmax = M.family_bounds(N)
        found = M.separate(x, FS, N, 0, tmin, tmax)
        given = M.separate(x, FS, N, P, keep=True)
        out[key] = (x, bg, fg, found, given)
    return out


@pytest.mark.parametrize("key", PARITY, ids=lambda k: "N%d_p%d_r%d" % k[1:])
def test_every_step_against_float64_repet(family, key):
    seed, N, P, R = key
    x, _, _, found, given = family[key]
    V, b, S, bg, fg = ref_repet(x, FS, N, P)
    braw = found.braw.astype(np.float64)
    dev = {"V": rel(given.V, V), "b": rel(braw / braw[0], b), "S": rel(given.S, S), "background": rel(given.background, bg),
           "foreground": rel(given.foreground, fg)}
    print(key, dev)
    for k, v in dev.items():
        assert v <= TOL[k], (k, v, TOL[k])
    assert given.V.dtype == given.S.dtype == given.background.dtype == given.foreground.dtype == np.float32


# ------------------------------------------------------------------------------------------------ tables and sizes
def test_tables_and_sizes():
    for N in (64, 256, 8192):
        w, d = M.window(N), M.divisor(N)
        assert w.dtype == d.dtype == np.float32 and w.size == N and d.size == N // 2
        assert abs(float(w[0]) - 0.08) < 1e-7 and float(w[N // 2]) == 1.0
        assert np.max(np.abs(d.astype(np.float64) - 1.08 * N)) <= 1.08 * N * 2.0 ** -22      # w[i] + w[i + H] = 1.08
    assert [M.n_frames(n, 128) for n in (1, 128, 129, 256)] == [2, 2, 3, 3]
    assert [M.lag_points(m) for m in (2, 32, 33, 8192, 8193, 16384)] == [64, 64, 128, 16384, 32768, 32768]
    assert M.lag_bounds(44100.0, 1024) == (35, 344) and M.lag_bounds(8000.0, 128, *M.family_bounds(256))[0] == 4
    assert M.cutoff_bin(8000.0, 256, 100.0) == 4 and M.cutoff_bin(8000.0, 256, 0.0) == 0


# ------------------------------------------------------------------------------------------------ the median rule
def test_median_rule_odd_even_ties_and_a_partial_last_segment():
    f = np.float32
    V = np.array([[1, 9], [5, 9], [3, 2], [7, 2], [2, 9], [4, 1], [6, 2]], f)       # m = 7
    S = M.segment_median(V, 2)          # l = 0: frames 0, 2, 4, 6 (even); l = 1: frames 1, 3, 5 (odd)
    assert np.array_equal(S, np.array([[(f(2) + f(3)) * f(0.5), (f(2) + f(9)) * f(0.5)], [5, 2]], f))
    S = M.segment_median(V, 3)          # a partial last segment: l = 0 has 3 values, l = 1 and 2 have 2
    assert np.array_equal(S, np.array([[6, 2], [3.5, 9], [3.5, 1.5]], f))
    S = M.segment_median(V, 6)          # r = 2: l = 0 has the frames 0 and 6, the others their own value
    assert np.array_equal(S[0], np.array([3.5, 5.5], f)) and np.array_equal(S[1:], V[1:6])
    ties = np.array([[2, 0], [2, 0], [1, 0], [2, 5], [1, 0], [2, 0]], f)
    assert np.array_equal(M.segment_median(ties, 1), np.array([[2, 0]], f))
    rng = np.random.default_rng(5)
    for m, p in ((40, 7), (41, 8), (256, 1), (300, 9)):
        V = rng.integers(0, 6, (m, 5)).astype(f)
        want = np.stack([np.median(V[l::p].astype(np.float64), axis=0) for l in range(p)])
        assert np.array_equal(M.segment_median(V, p).astype(np.float64), want)       # small integers: the mean of two is exact
    big = np.array([[3e38], [3e38], [1.0], [3e38]], f)
    assert np.isinf(M.segment_median(big, 1)[0, 0])      # (s[1] + s[2]) * 0.5f in float32, as the device adds


# ------------------------------------------------------------------------------------------------ find_period
def test_find_period_rules():
    m = 120
    b = np.zeros(m, np.float32)
    b[0] = 1.0
    b[::10] = 0.5
    b[0] = 1.0
    assert M.find_period(b, 4, 1000)[0] == 10
    assert 0.4 < M.find_period(b, 4, 1000)[1] < 0.5               # eight peaks of 0.5, each less the mean of its window, over floor(90 / 10)
    assert M.find_period(b, 31, 1000) == (0, 0.0)                                      # l = 90: candidates end at 30
    assert M.find_period(np.zeros(m, np.float32), 4, 1000) == (0, 0.0)
    assert M.find_period(np.full(m, 3.0, np.float32), 4, 1000) == (0, 0.0)            # a constant: no J is positive
    bad = b.copy()
    bad[0] = np.nan
    assert M.find_period(bad, 4, 1000) == (0, 0.0) and M.find_period(b[:5], 2, 1000) == (0, 0.0)


# ------------------------------------------------------------------------------------------------ a periodic clip
def test_a_strictly_periodic_clip_is_its_own_background(oracle):
    oracle.lib()
    N, p, reps = 256, 11, 9
    H = N // 2
    rng = np.random.default_rng(8)
    x = np.tile(rng.uniform(-0.5, 0.5, p * H), reps).astype(np.float32)
    r = M.separate(x, FS, N, p, highpass=0.0, keep=True)
    inner = slice(p * H, x.size - p * H)
    # away from the edges every column holds one value nine times over: S = V there, the mask is exactly 1
    assert np.all(r.M[p:-p - 1] == 1.0)
    scale = float(np.max(np.abs(x)))
    assert np.max(np.abs(r.background[inner] - x[inner])) <= 2e-6 * scale and np.max(np.abs(r.foreground[inner])) <= 2e-6 * scale
    assert np.array_equal(r.foreground, (x - r.background).astype(np.float32))


def test_no_period_gives_silence_and_the_input(oracle):
    oracle.lib()
    x = np.zeros(3000, np.float32)
    x[5] = -0.0
    r = M.separate(x, FS, 256)
    assert r.period == 0 and r.braw[0] == 0 and np.array_equal(r.foreground.view(np.uint32), x.view(np.uint32))
    assert np.all(r.background.view(np.uint32) == 0)


# ------------------------------------------------------------------------------------------------ the quality condition
def test_the_model_finds_the_period_of_all_twenty_clips(family):
    assert len(family) == 20
    for key, (_, _, _, found, _) in family.items():
        assert found.period == key[2], (key, found.period)
        assert found.score > 0


def test_the_foreground_gains_ten_decibels_on_all_twenty_clips(family):
    gains = {}
    for key, (x, _, fg, _, given) in family.items():
        gains[key] = M.sdr(fg, given.foreground) - M.sdr(fg, x)
    print("foreground SDR gain: min %.2f dB, max %.2f dB" % (min(gains.values()), max(gains.values())))
    for key, g in gains.items():
        assert g >= 10.0, (key, g)
    # with the period found the outputs are those of the period given: same frames, same median
    for key, (_, _, _, found, given) in family.items():
        assert np.array_equal(found.background.view(np.uint32), given.background.view(np.uint32))
