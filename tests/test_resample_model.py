"""CPU tier of the resampler's contract (tests/resample_model.py, the arithmetic of zen_amd/resample/zen_hip_resample.h): the
model against a float64 restatement without a table, the quality it gives on sines, the rejection of what would alias, pieces
against the whole, the integer geometry on its edges and the length rule of the pitch shift."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import resample_model as M  # noqa: E402

RATIOS = [(147, 160), (160, 147), (1, 4), (4, 1), (1048573, 1048575), (61858, 65536)]
QUALITY_RATIOS = [(147, 160), (160, 147), (1, 2), (2, 1), (53, 63), (1, 4), (4, 1)]
SNR_FLOOR = {8: 70.0, 16: 95.0, 32: 115.0}          # a prototype of the contract gave 80 / 105 / 128 dB: 10 dB of margin
ALIAS_CEILING = {8: -65.0, 16: -95.0, 32: -120.0}   # the prototype gave -72 / -103 / -142 dB


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("Z", [8, 16, 32])
@pytest.mark.parametrize("num,den", RATIOS)
def test_model_against_the_float64_restatement(num, den, Z):
    """uniform noise in [-1, 1], 700 samples: the 512-phase interpolation is the dominant term (2.5e-6 in the prototype), the
    bound a factor of two above it"""
    x = np.random.default_rng(num + Z).uniform(-1, 1, 700).astype(np.float32)
    y, ref = M.resample(x, num, den, Z), M.resample_f64(x, num, den, Z)
    assert y.dtype == np.float32 and y.size == ref.size == M.n_out(num, den, 700)
    err = float(np.abs(y.astype(np.float64) - ref).max())
    print("ratio %d/%d Z %d: max abs difference %.3g" % (num, den, Z, err))
    assert err <= 5e-6, err


@pytest.mark.parametrize("Z", [8, 16, 32])
@pytest.mark.parametrize("num,den", QUALITY_RATIOS)
def test_sines_come_out_as_sines(num, den, Z):
    """amplitude 0.5, n = 6000, at 0.05 and 0.5 of the narrower band's edge"""
    edge = 0.5 * min(1.0, num / den)                 # in cycles per input sample
    for part in (0.05, 0.5):
        f_in = part * edge
        y = M.resample(M.sine(6000, f_in), num, den, Z)
        snr, amp = M.sine_fit(y, f_in * den / num, M.skip(num, den, Z))
        print("ratio %d/%d Z %d at %.2f of the edge: SNR %.1f dB, amplitude %.6f" % (num, den, Z, part, snr, amp))
        assert snr >= SNR_FLOOR[Z], (part, snr)
        assert abs(amp - 0.5) < 1e-3, amp


@pytest.mark.parametrize("Z", [8, 16, 32])
@pytest.mark.parametrize("num,den", [(1, 2), (53, 63)])
def test_a_tone_above_the_new_nyquist_is_rejected(num, den, Z):
    """a tone at 1.15 times the new Nyquist would fold to 0.85 of it: what is left of it, against its amplitude going in"""
    f_in = 1.15 * 0.5 * num / den                    # cycles per input sample
    y = M.resample(M.sine(6000, f_in), num, den, Z).astype(np.float64)
    m = M.skip(num, den, Z)
    level = 20.0 * math.log10(math.sqrt(2.0 * np.mean(y[m:-m] ** 2)) / 0.5)
    print("ratio %d/%d Z %d: the tone comes out at %.1f dB" % (num, den, Z, level))
    assert level <= ALIAS_CEILING[Z], level


@pytest.mark.parametrize("num,den,Z", [(147, 160, 16), (4, 1, 8), (1, 4, 32), (61858, 65536, 16), (1048573, 1048575, 8)])
def test_pieces_equal_the_whole(num, den, Z):
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, 5000).astype(np.float32)
    whole = M.resample(x, num, den, Z)
    inner = np.sort(rng.integers(0, whole.size + 1, 12))
    cuts = [0] + list(inner) + [int(inner[5]) + 1, whole.size]          # a single-output piece among them
    cuts = sorted(int(c) for c in cuts if c <= whole.size)
    got = M.pieces(x, num, den, Z, cuts)
    assert np.array_equal(bits(got), bits(whole))
    # a window wider than the span gives the same bits; one short of it is refused
    lo, cnt = M.span(num, den, Z, x.size, 1000, 7)
    wide = M.resample(x[max(lo - 5, 0):lo + cnt + 9], num, den, Z, 1000, 7, x.size, max(lo - 5, 0))
    assert np.array_equal(bits(wide), bits(whole[1000:1007]))
    with pytest.raises(AssertionError):
        M.resample(x[lo + 1:lo + cnt], num, den, Z, 1000, 7, x.size, lo + 1)


def test_the_polyphase_rows_are_the_interpolated_coefficients():
    for num, den, Z in ((147, 160, 16), (4096, 4095, 8), (1, 4, 32)):
        rows = M.polyphase(num, den, Z)
        t = np.arange(3 * num, dtype=np.int64)
        _, rem, p, mu = M.positions(num, den, t)
        assert np.array_equal(bits(rows[rem]), bits(M.coefficients(M.table(num, den, Z), p, mu)))


def test_table_shape_and_symmetry():
    for num, den, Z in ((1, 1, 8), (147, 160, 16), (1, 4, 32), (4, 1, 32)):
        W, T, _ = M.geometry(num, den, Z)
        h = M.table(num, den, Z)
        assert h.shape == (513, T) and h.dtype == np.float32
        c = min(1.0, num / den) * M.QUALITIES[Z][0]
        assert h[0, W - 1] == np.float32(c) and abs(float(h[512, W]) - c) < 1e-6      # d = 0: the centre tap
        assert abs(float(h[512, 0])) <= 1.001 * c / float(np.i0(M.QUALITIES[Z][1]))         # d = -W: the window's edge, 1 / I0(beta)
        assert np.allclose(h[0, :W - 1], h[0, W:2 * W - 1][::-1], atol=1e-7)            # h(d) = h(-d)
    assert M.geometry(1, 4, 32) == (128, 256, 1) and M.geometry(147, 160, 16) == (18, 36, 1) and M.geometry(4097, 4096, 8) == (8, 16, 0)
    assert M.geometry(4096, 4097, 8)[2] == 1 and M.geometry(2 * 4097, 2 * 4096, 8)[2] == 0 and M.geometry(8194, 4096, 8)[2] == 0


def test_n_out_and_span_on_their_edges():
    assert M.n_out(1, 4, 1) == 1 and M.n_out(1, 4, 4) == 1 and M.n_out(1, 4, 5) == 2 and M.n_out(4, 1, 1) == 4
    assert M.n_out(147, 160, 160) == 147 and M.n_out(147, 160, 161) == 148 and M.n_out(294, 320, 161) == 148
    assert M.n_out(4, 1, 1 << 40) == 1 << 42 and M.n_out(1048573, 1048575, 1 << 40) == -(-(1048573 << 40) // 1048575)
    # every output's position lies inside the row
    for num, den in RATIOS:
        for n in (1, 2, 699, 700):
            last = M.n_out(num, den, n) - 1
            assert (last * den) // num <= n - 1 and (last + 1) * den >= n * num
    W = M.geometry(147, 160, 16)[0]
    assert M.span(147, 160, 16, 5000, 0, 1) == (0, W + 1)                           # clipped at the front
    assert M.span(147, 160, 16, 5000, 1000, 1) == (1088 - W + 1, 2 * W)             # 1000 * 160 // 147 = 1088
    lo, cnt = M.span(147, 160, 16, 5000, 0, M.n_out(147, 160, 5000))
    assert (lo, cnt) == (0, 5000)
    lo, cnt = M.span(147, 160, 16, 5000, M.n_out(147, 160, 5000) - 1, 1)
    assert lo + cnt == 5000                                                         # clipped at the end
    assert M.span(4, 1, 8, 1, 0, 4) == (0, 1) and M.span(1, 4, 32, 1 << 40, 0, 1) == (0, 129)
    far = (1 << 40) * 4 - 1
    assert M.span(4, 1, 8, 1 << 40, far, 1) == ((1 << 40) - 8, 8)
    with pytest.raises(AssertionError):
        M.span(147, 160, 16, 5000, M.n_out(147, 160, 5000), 1)
    with pytest.raises(AssertionError):
        M.reduced(1, 5)
    with pytest.raises(AssertionError):
        M.reduced(1048577, 1048576)


def test_positions_at_far_offsets_are_exact_integers():
    """t near 2^41 with den = 1048575: the products stay below 2^63 and agree with Python's integers"""
    num, den = 1048573, 1048575
    t0 = (1 << 41) - 12345
    i, rem, p, mu = M.positions(num, den, t0 + np.arange(50, dtype=np.int64))
    for k in range(50):
        a = (t0 + k) * den
        f = ((a % num) << 32) // num
        assert (int(i[k]), int(rem[k]), int(p[k])) == (a // num, a % num, f >> 23) and float(mu[k]) == (f & 0x7FFFFF) / 2.0 ** 23


def test_the_shift_keeps_the_length_within_three_samples():
    """for every whole s in +-24: ceil(floor(n alpha) num / den) is n - 3 .. n, alpha = den / num"""
    rng = np.random.default_rng(12)
    lengths = [1, 2, 3, 4, 5, 7, 255, 256, 3000, 3072, 44100, 10 ** 7] + [int(v) for v in rng.integers(1, 10 ** 7, 40)]
    for s in range(-24, 25):
        num, den = M.ratio_for_shift(s)
        assert 0.25 <= num / den <= 4.0 and math.gcd(num, den) == 1
        unreduced = num * (65536 // den)            # off 65536 / 2^(s / 12) by half a unit at the most
        assert abs(den / num - 2.0 ** (s / 12.0)) <= 0.51 / unreduced * 2.0 ** (s / 12.0)
        for n in lengths:
            _, _, alpha, m, k = M.shift_lengths(n, s)
            assert m == int(math.floor(n * alpha))
            if m:
                assert n - 3 <= k <= n, (s, n, m, k)
    assert M.ratio_for_shift(0) == (1, 1) and M.ratio_for_shift(12) == (1, 2) and M.ratio_for_shift(-24) == (4, 1)
    assert M.ratio_for_shift(3) == (55109, 65536)
