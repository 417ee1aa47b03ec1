"""CPU tier of the pitch tracker (zen_amd/pitch): tests/pitch_model.py, the model the GPU tier compares against bit for bit,
checked here against what it models -- its autocorrelation against a float64 evaluation of the definition, the README
claim of the reference's demo ("pitch tracking is improved with real-time harmonic separation") on a fixed input, and the
edge chunks pinned to the values the model gives today."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pitch_model as M  # noqa: E402

FS = M.FS


def autocorr64(x):
    n = x.size
    spec = np.fft.rfft(x.astype(np.float64), 2 * n)
    return np.fft.irfft(np.abs(spec) ** 2, 2 * n)[:n]


def autocorr_inputs(n, seed=100):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    tone = 0.3 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 440 * t + .3) + 0.1 * np.sin(2 * np.pi * 660 * t + 1.)
    noise = rng.uniform(-1, 1, n)
    return {"tone": tone, "noise": noise, "constant": np.full(n, 0.37), "tone+noise": tone + 0.2 * noise}


@pytest.mark.parametrize("n", [64, 256, 4096, 16384])
def test_autocorrelation_against_float64(oracle, n):
    """max |r / 2N - r64| / r64[0].  Measured with seeds 100..102 (tone / noise / constant / tone+noise):
         N = 64     1.6e-7  1.0e-7  1.0e-7  1.9e-7
         N = 256    1.8e-7  4.6e-8  1.3e-7  1.9e-7
         N = 4096   3.0e-7  7.1e-8  2.0e-7  3.1e-7
         N = 16384  2.8e-7  5.1e-8  2.3e-7  3.0e-7
    The bound is 4 x the largest of them.  The NSDF itself is not asserted on: towards t -> N its denominator is the energy
    of a couple of samples and the float32 transform error is amplified."""
    for name, x in autocorr_inputs(n).items():
        x = x.astype(np.float32)
        ref = autocorr64(x)
        err = np.max(np.abs(M.autocorr(x).astype(np.float64) / (2 * n) - ref)) / ref[0]
        print(n, name, "%.3e" % err)
        assert err <= 4 * 3.1e-7, (n, name, err)


def test_prefix_is_the_stated_association():
    """runs of 64 summed left to right, the totals summed left to right, P[k] = earlier totals + the sum within the run"""
    rng = np.random.default_rng(3)
    for n in (32, 64, 256):
        x = rng.uniform(-1, 1, n).astype(np.float32)
        run = min(64, n)
        want = [0.0]
        base = 0.0
        for r in range(n // run):
            inner = 0.0
            for i in range(run):
                inner = inner + float(x[r * run + i]) * float(x[r * run + i])
                want.append(base + inner)
            base = base + inner
            want[-1] = base
        assert np.array_equal(M.prefix(x), np.array(want))
    assert M.prefix(np.ones(32, np.float32))[-1] == 32.0


def test_key_maxima_rule_on_hand_made_rows():
    f = np.float32
    a = np.zeros(32, f)                          # T = 10
    a[:3] = [1.0, 0.5, -0.1]                     # the first non-positive index is 2: p = 2, then on to 5
    a[5:9] = [0.2, 0.6, 0.6, 0.1]                # a plateau: the earlier of the equal values
    a[12:17] = [0.3, 0.2, 0.4, 0.1, 0.4]         # two candidates in one run (12 is no candidate: a[11] = 0 < 0.3 makes it one)
    a[20:23] = [0.1, 0.2, 0.3]                   # rising into a non-positive value: 22 is a candidate (a[23] = 0)
    a[30:32] = [0.5, 0.9]                        # index 31 is never examined; 30 has a[31] above it
    assert M.key_maxima(a) == [6, 14, 22]
    a[12] = 0.4                                  # equal to the later candidates of its run: the earliest stays
    assert M.key_maxima(a) == [6, 12, 22]
    b = np.full(32, 0.5, f)                      # no non-positive value at all: p = T = 10, no candidate anywhere
    assert M.key_maxima(b) == []
    b[11] = 0.7
    assert M.key_maxima(b) == [11]
    pitch, period, clarity = M.choose(b, 3200.0)
    assert (pitch, period, clarity) == (f(3200.0) / f(11), f(11), f(0.7))      # symmetric neighbours: the parabola stays at 11


def test_the_claim_harmonic_separation_helps_the_tracker(oracle):
    """fs 44100, N 4096, 14 chunks: a five-partial tone at 163.3 Hz under drum bursts of amplitude 3.  Behind the oracle's causal
    harmonic output (hop 4096, beta 2.5) every chunk is within 1 Hz; on the raw mix at least 8 of the 14 are lost.
    Measured: with HPR worst 0.546 Hz (chunk 0, 163.846); without, 10 chunks return -1."""
    f0 = 163.3
    x = M.claim_input(3.0)
    assert x.dtype == np.float32 and x.size == 14 * 4096
    harm = oracle.HPR(FS, 4096, 2.5, oracle.OUTPUT_HARMONIC, oracle.TIME_CAUSAL).process_stream(x)["H"]
    with_hpr = M.track(harm, FS, 4096)[0]
    without = M.track(x, FS, 4096)[0]
    print("with HPR", with_hpr, "worst", np.max(np.abs(with_hpr - f0)))
    print("without ", without)
    assert with_hpr.size == 14 and np.all(np.abs(with_hpr - f0) <= 1.0)
    lost = (without == -1) | (np.abs(without - f0) > 1.0)
    assert np.sum(lost) >= 8


# ------------------------------------------------------------------------------------------------ edge chunks, N = 4096
@pytest.fixture(scope="module")
def edges(oracle):
    return {k: M.chunk(v[:4096]) for k, v in M.edge_inputs(4096).items()}


def test_zeros_have_no_key_maximum(edges):
    pitch, period, clarity, a = edges["zeros"]
    assert np.all(a == 0) and M.key_maxima(a) == []
    assert (pitch, period, clarity) == (-1, 0, 0)


def test_60_hz_is_found_and_not_reported(edges):
    pitch, period, clarity, a = edges["sine60"]
    assert pitch == -1 and abs(period - FS / 60.0) < 0.01 and abs(clarity - 1) < 1e-3      # 734.9988, 1.0
    assert len(M.key_maxima(a)) == 5


def test_30_hz_first_positive_lobe_outlasts_T(edges):
    """the NSDF's first positive lobe lasts a quarter period, 367 samples: at N = 4096 the scan starts behind it (T = 1365) and
    finds the period; at N = 1024 (T = 341) the lobe outlasts T, the scan starts inside it, and the chunk is shorter than the
    period: no key maximum"""
    pitch, period, clarity, a = edges["sine30"]
    short = M.chunk(M.edge_inputs(1024)["sine30"][:1024])
    assert np.all(short[3][:1023 // 3 + 1] > 0) and int(np.flatnonzero(short[3] <= 0)[0]) > 1023 // 3       # 378
    assert M.key_maxima(short[3]) == [] and short[:3] == (-1, 0, 0)
    assert int(np.flatnonzero(a <= 0)[0]) < (4096 - 1) // 3
    assert pitch == -1 and abs(period - FS / 30.0) < 0.01                                   # 1469.9967
    assert len(M.key_maxima(a)) == 2


def test_440_hz(edges):
    pitch, period, clarity, a = edges["sine440"]
    assert abs(pitch - 440.0) <= 0.01                                                       # 439.99988
    assert abs(period - FS / 440.0) < 1e-3 and clarity > 0.9999


def test_constant_chunk_is_decided_by_the_last_bit(edges):
    """the NSDF of a constant is 1 everywhere up to rounding: no non-positive value, p = T, and the candidates are whatever the
    last bits make of it; the winner sits where the rounding error is largest, at the end of the row"""
    pitch, period, clarity, a = edges["constant"]
    assert np.all(np.abs(a[:3072] - 1) < 1e-5) and np.all(a > 0)
    keys = M.key_maxima(a)
    assert len(keys) == 1 and keys[0] >= (4096 - 1) // 3
    assert pitch == -1 and period == np.float32(4092.2505) and clarity == np.float32(1.0001296)


def test_square_wave_of_period_16(edges):
    pitch, period, clarity, a = edges["square16"]
    assert len(M.key_maxima(a)) == 255
    assert period == np.float32(16.000858) and clarity == np.float32(1.0000004) and pitch == np.float32(FS) / period
