"""CPU tier: the model of the time-stretch library (tests/tsm_model.py) against what it stands for -- its integer phase
arithmetic against libm, its vocoder against the float64 restatement and against the signals a vocoder must keep: a steady
sine comes back as that sine, alpha = 1 is the identity, clicks land where the ratio puts them, and the harmonic / percussive
route keeps clicks sharper than the vocoder alone.  The bounds are the model's own measured figures."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tsm_model as M  # noqa: E402

TURN = 4294967296.0
# measured on 200000 normal pairs and the grid below: 3.98e-9 turns; the bound is that times 4
ATAN_BOUND = 1.6e-8
# the phase is cut to 2^-22 turns (2 pi 2^-22 in angle) and the product of two float32 table values adds a few 2^-24
CS_BOUND = 2.0 * math.pi * 2.0 ** -22 + 4.0 * 2.0 ** -24
FREQ = 0.0437                 # cycles per sample: off every bin of both frames
ALPHAS = (0.5, 0.8, 1.25, 1.5, 2.0, 3.3)
# the model's minimum over ALPHAS with the engine's float32 transform (alpha 3.3 at frame 256, alpha 0.8 at frame 1024); the
# floor is that minus 6 dB
SNR_MEASURED_MIN = {256: 92.476, 1024: 121.564}
SNR_FLOOR = {N: v - 6.0 for N, v in SNR_MEASURED_MIN.items()}
# crest factor of hp over pv on sine + clicks at frames 1024 / 64, alpha 1.5: 7.70 dB on the model; asserted at half of it
HP_MARGIN_DB = 3.85


def turns_error(got, y, x):
    ref = np.arctan2(np.asarray(y, np.float64), np.asarray(x, np.float64)) / (2.0 * np.pi)
    d = got.astype(np.float64) / TURN - ref
    return np.abs((d + 0.5) % 1.0 - 0.5).max()


def test_atan2turns_against_libm_on_a_grid_and_random_pairs():
    rng = np.random.default_rng(0)
    x, y = rng.normal(size=200000).astype(np.float32), rng.normal(size=200000).astype(np.float32)
    worst = turns_error(M.atan2turns(y, x), y, x)
    g = np.linspace(-1.0, 1.0, 801).astype(np.float32)
    gy, gx = (a.ravel() for a in np.meshgrid(g, g))
    keep = (gx != 0) | (gy != 0)
    worst = max(worst, turns_error(M.atan2turns(gy[keep], gx[keep]), gy[keep], gx[keep]))
    print("atan2turns: %.3g turns from libm at the most" % worst)
    assert worst <= ATAN_BOUND


def test_atan2turns_on_the_axes_and_diagonals_is_exact():
    one, zero = np.float32(1), np.float32(0)
    cases = [((zero, one), 0), ((one, one), 1 << 29), ((one, zero), 1 << 30), ((one, -one), 3 << 29), ((zero, -one), 1 << 31),
             ((-one, -one), 5 << 29), ((-one, zero), 3 << 30), ((-one, one), 7 << 29), ((zero, zero), 0), ((-zero, zero), 0)]
    for (y, x), want in cases:
        assert int(M.atan2turns(y, x)) == want, (y, x)
    # -0 is not < 0: the phase of (x, -0) is that of (x, +0)
    assert int(M.atan2turns(np.float32(-0.0), np.float32(-1))) == 1 << 31


def test_cs_against_libm():
    rng = np.random.default_rng(1)
    psi = np.concatenate([rng.integers(0, 1 << 32, 200000, dtype=np.uint64), np.arange(0, 1 << 32, 1 << 21, dtype=np.uint64)])
    c, s = M.cs(psi)
    ang = 2.0 * np.pi * psi.astype(np.float64) / TURN
    worst = max(np.abs(c - np.cos(ang)).max(), np.abs(s - np.sin(ang)).max())
    print("cs: %.3g from libm at the most" % worst)
    assert worst <= CS_BOUND
    assert M.cs(np.array([0, 1 << 30], np.uint64))[0][0] == 1.0 and M.cs(np.array([1 << 30], np.uint64))[1][0] == 1.0


def test_low_phase_bits_do_not_reach_cs():
    psi = np.array([0x12345400, 0x123457FF], np.uint64)
    c, s = M.cs(psi)
    assert c[0] == c[1] and s[0] == s[1]


@pytest.mark.parametrize("N", [64, 256])
def test_psi_equals_theta_at_alpha_one(oracle, N):
    rng = np.random.default_rng(N)
    x = rng.uniform(-1, 1, 9 * N // 4 + 5).astype(np.float32)
    r = M.stretch_pv(x, N, 1.0, keep=True)
    assert all(b - a == N // 4 for a, b in zip(r.a, r.a[1:]))
    assert np.array_equal(r.psi, r.theta)
    snr = 10 * math.log10(np.sum(x.astype(np.float64) ** 2) / np.sum((r.out.astype(np.float64) - x) ** 2))
    assert r.out.size == x.size and snr > 120.0, snr


def test_the_scaled_deviation_is_rounded_towards_zero():
    assert list(M.trunc_div(np.array([-7, 7, -8, 8, -1, 0]), 4)) == [-1, 1, -2, 2, 0, 0]
    assert -7 // 4 == -2                         # what the model must not use
    # one bin, two frames: theta moves back by 5 words more than Omega(k, Ha); Hs / Ha = 64 / 49 leaves a remainder
    N, Hs, Ha, k = 256, 64, 49, 3
    unit = (1 << 32) // N
    theta = np.array([[0] * 4, [0] * 4], np.int64)
    theta[0, k] = 1000
    theta[1, k] = (1000 + k * Ha * unit - 5) & M.MASK
    mag = np.zeros((2, 4), np.float32)
    mag[:, k] = 1.0
    own, psi = M.recurrence(mag, theta, [0, Ha], N)
    assert list(own[1]) == [k] * 4
    assert -5 * Hs // Ha == -7 and int(M.trunc_div(-5 * Hs, Ha)) == -6
    assert int(psi[1, k]) == (1000 + k * Hs * unit - 6) & M.MASK


def test_peaks_and_owners_at_the_edges_plateaus_and_ties():
    f = np.float32
    H = 8

    def own(v):
        return list(M.owners(M.peaks(np.asarray(v, f))))
    assert list(M.peaks(np.zeros(H + 1, f))) == [True] * (H + 1) and own(np.zeros(H + 1)) == list(range(H + 1))      # silence
    assert own([1, 1, 1, 1, 1, 1, 1, 1, 1]) == list(range(9))                                                       # one plateau: no peak
    assert list(np.flatnonzero(M.peaks(np.array([5, 1, 0, 0, 0, 0, 0, 1, 5], f)))) == [0, 8]                          # bins 0 and H
    assert own([5, 1, 0, 0, 0, 0, 0, 1, 5]) == [0, 0, 0, 0, 0, 8, 8, 8, 8]                                            # bin 4 is tied: the lower
    assert list(np.flatnonzero(M.peaks(np.array([1, 5, 1, 0, 0, 0, 1, 5, 1], f)))) == [1, 7]                          # bins 1 and H - 1
    assert own([1, 5, 1, 0, 0, 0, 1, 5, 1]) == [1, 1, 1, 1, 1, 7, 7, 7, 7]
    assert list(np.flatnonzero(M.peaks(np.array([0, 2, 2, 0, 0, 3, 0, 0, 0], f)))) == [5]                             # a plateau of two is no peak
    assert list(np.flatnonzero(M.peaks(np.array([0, 3, 0, 4, 0, 0, 0, 0, 0], f)))) == [3]                             # two bins apart: the larger only


@pytest.mark.parametrize("N", [256, 1024])
def test_a_steady_sine_comes_back_as_that_sine(oracle, N):
    x = M.sine(4000 if N == 256 else 12000, FREQ)
    worst = np.inf
    for alpha in ALPHAS:
        y = M.stretch_pv(x, N, alpha)
        snr, amp = M.sine_snr(y, FREQ, 2 * N)
        ref = M.sine_snr(M.stretch_pv_f64(x, N, alpha), FREQ, 2 * N)[0]
        print("frame %d alpha %.2f: %.2f dB (float64 with libm phases: %.2f dB), amplitude %.6f" % (N, alpha, snr, ref, amp))
        assert y.size == int(math.floor(x.size * alpha)) and abs(amp - 0.5) < 1e-5
        worst = min(worst, snr)
    assert worst >= SNR_FLOOR[N], worst


@pytest.mark.parametrize("Np", [16, 256])
@pytest.mark.parametrize("alpha", [0.77, 1.0, 1.3, 2.0, 4.0])
def test_clicks_through_overlap_add_land_where_the_ratio_puts_them(Np, alpha):
    """"Every click lands within Np / 2 of alpha t" holds for alpha >= 1: there the frames are at most Hs apart in the input,
    the frame whose position is nearest a click carries it at a weight of at least 0.5, and it comes out at most
    Hs / 2 (1 - 1 / alpha) + 1 samples from alpha t.  For 0.5 < alpha < 1 (0.77 here) the frames are up to 2 Hs apart: every
    click is still inside a frame, but its weight can fall to 0.25 at 0.77, so that is the height asserted there.  At
    alpha <= 0.5 the frames are Np or more apart and a click between two of them has weight 0 -- overlap-add drops material
    when it shortens that far -- so no landing can be asserted and no such ratio is in the list."""
    amp, every, first, n = 0.9, 700, 333, 6000
    y = M.stretch_ola(M.clicks(n, every, first, amp), Np, alpha)
    assert y.size == int(math.floor(n * alpha))
    for t in range(first, n, every):
        c = int(round(alpha * t))
        lo, hi = max(c - Np // 2, 0), min(c + Np // 2 + 1, y.size)
        if hi <= lo:
            continue
        assert y[lo:hi].max() >= (0.5 if alpha >= 1 else 0.25) * amp - 1e-6, (t, alpha)
    if alpha == 1.0:
        assert np.abs(y - M.clicks(n, every, first, amp)).max() <= 2.0 ** -23


def test_overlap_add_at_alpha_one_returns_the_sum_of_its_inputs():
    rng = np.random.default_rng(3)
    p, r = rng.uniform(-1, 1, 1000).astype(np.float32), rng.uniform(-1, 1, 1000).astype(np.float32)
    y = M.stretch_ola(p, 64, 1.0, r)
    want = p + r
    assert np.abs(y - want).max() <= 2.0 ** -22            # one ulp of values below 2


def test_hp_keeps_clicks_sharper_than_the_vocoder_alone(oracle):
    x = M.sine_and_clicks(8192)
    st = oracle.HPR(8000.0, 256, 2.5, 7, oracle.TIME_CAUSAL).process_stream(x)
    hp = M.stretch_hp(st["H"], st["P"], 1024, 64, 1.5, st["R"])
    pv = M.stretch_pv(x, 1024, 1.5)
    margin = M.crest_db(hp) - M.crest_db(pv)
    print("crest factor: hp %.2f dB, pv %.2f dB, margin %.2f dB" % (M.crest_db(hp), M.crest_db(pv), margin))
    assert hp.size == pv.size == 12288 and margin >= HP_MARGIN_DB
