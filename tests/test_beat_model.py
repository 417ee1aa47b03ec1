"""CPU tier of the beat tracker: tests/beat_model.py is the contract the kernels of zen_amd/beat are held to bit for bit
(tests/test_gpu_beat.py), so the model itself is checked here -- its onset function against the textbook form, its ordered
sums against plain loops, its independence of how a stream is cut into calls, what it finds on click tracks of known tempo,
and the claim the feature rests on: does the percussive stream in front of the tracker help."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import beat_model as M  # noqa: E402

f32 = np.float32
FS, HOP = 44100.0, 512


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def intervals(beat):
    return np.diff(np.flatnonzero(np.asarray(beat) > 0))


# ================================================================================================ parameters
def test_accepted_and_refused_pairs():
    for fs, hop in M.ACCEPTED:
        assert M.accepted(fs, hop), (fs, hop)
    for fs, hop in M.REFUSED + ((44100.0, 96), (44100.0, 4096), (44100.0, 32)):
        assert not M.accepted(fs, hop), (fs, hop)
    # the demo's own case: the period of 80 bpm is 129 hops, one more than the 128 lags the comb filter bank has
    assert M.periods(44100.0, 256)[0] == 129 and M.periods(22050.0, 128)[0] == 129
    assert M.periods(FS, HOP)[20] == 43 and M.rh(43) == 22 and M.r2(43) == 86 and M.rh(44) == 22


# ================================================================================================ onset function
ODF_BOUND = 4 * 9.565e-4          # 4 x the largest relative difference found, see below


def test_rational_onset_function_against_the_textbook_form(oracle):
    """The model forms no phase: directions are unit vectors, the prediction m1 e^{i(2 phi1 - phi2)} is two complex
    products.  Against the float64 evaluation with atan2 and cos on the same spectra, 120 hops each, the largest relative
    difference of an onset value (absolute where the textbook value is 0) was: tone 2.52e-4, noise 6.95e-8, clicks 2.38e-7,
    silence 0, click track 9.565e-4 -- the large ones at hops whose onset value is 1e-5 of the signal's peak, where the
    cancellation in m^2 + m1^2 - 2 m m1 cos costs either form its digits.  Asserted at 4 x the largest."""
    oracle.lib()
    n = HOP * 120
    rng = np.random.default_rng(0)
    t = np.arange(n) / FS
    clicks = np.zeros(n)
    clicks[::9000] = 1.0
    sigs = {"tone": 0.5 * np.sin(2 * np.pi * 441 * t), "noise": 0.5 * rng.uniform(-1, 1, n), "clicks": clicks, "silence": np.zeros(n),
            "click track": M.click_track(120, seconds=n / FS)}
    for name, x in sigs.items():
        x = x.astype(f32)
        a, b = M.Onset(FS, HOP).run(x).astype(np.float64), M.odf_textbook(x, FS, HOP)
        d = np.abs(a - b)
        rel = np.where(b > 0, d / np.where(b > 0, b, 1.0), d)
        print("%s: largest relative difference %.3e (hop %d of onset values up to %.1f)" % (name, rel.max(), rel.argmax(), b.max()))
        assert rel.max() <= ODF_BOUND, name
        if name == "silence":
            assert not a.any() and not b.any()
        else:
            assert b.max() > 100


def test_first_frames_see_zeros_in_front_of_the_stream(oracle):
    """frame 0 is the first hop behind `hop` zeros, under the window rotated by half a frame; X_-1 = X_-2 = 0 makes every
    direction (1, 0) and the first onset value the sum of the magnitudes"""
    oracle.lib()
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, 128).astype(f32)
    on = M.Onset(8000.0, 64)
    row = on.frame(x[:64])
    win = M.tables(8000.0, 64).win
    assert np.array_equal(row.real[:64], x[:64] * win[64:]) and not row.real[64:].any() and not row.imag.any()
    spec = oracle.fft_c2c(row)
    want = M.ordered_sum(np.sqrt(spec.real * spec.real + spec.imag * spec.imag))
    assert bits(on.hop_value(x[:64])) == bits(want)
    row = on.frame(x[64:])
    assert np.array_equal(row.real[64:], x[:64] * win[:64]) and np.array_equal(row.real[:64], x[64:] * win[64:])


# ================================================================================================ ordered sums
def test_ordered_sums_against_plain_loops():
    rng = np.random.default_rng(2)
    # the onset sum: 64 columns left to right, then the halving tree
    for n in (128, 1024, 4096):
        v = (rng.uniform(0, 1, n) ** 8 * 1e3).astype(f32)
        p = [f32(0)] * 64
        for lane in range(64):
            acc = v[lane]
            for i in range(64 + lane, n, 64):
                acc = f32(acc + v[i])
            p[lane] = acc
        s = 32
        while s:
            for lane in range(s):
                p[lane] = f32(p[lane] + p[lane + s])
            s >>= 1
        assert bits(M.ordered_sum(v)) == bits(p[0]), n
    # thr: windows of at most 16, left to right
    for n in (512, 128):
        x = rng.uniform(0, 2, n).astype(f32)
        want = np.empty(n, f32)
        for i in range(n):
            lo, hi = max(0, i - 8), min(n, i + 8)
            acc = f32(0)
            for q in range(lo, hi):
                acc = f32(acc + x[q])
            want[i] = max(f32(x[i] - f32(acc / f32(hi - lo))), f32(0))
        assert np.array_equal(bits(M.thr(x)), bits(want)), n
    # the autocorrelation: one sum per lag, left to right
    y = M.thr(rng.uniform(0, 2, 512).astype(f32))
    want = np.empty(512, f32)
    for lag in (0, 1, 2, 43, 86, 255, 256, 400, 510, 511):
        acc = f32(0)
        for i in range(512 - lag):
            acc = f32(acc + f32(y[i] * y[i + lag]))
        want[lag] = f32(acc / f32(512 - lag))
        assert bits(M.acf(y)[lag]) == bits(want[lag]), lag
    # the comb filter bank: a = 1..4, b' = 1-a..a-1
    a = M.acf(y)
    r = M.tables(FS, HOP).rayleigh
    c = M.comb(a, r)
    assert c.size == 128 and c[0] == 0 and c[127] == 0
    for i in (2, 3, 43, 86, 127):
        acc = f32(0)
        for k in range(1, 5):
            for o in range(1 - k, k):
                acc = f32(acc + f32(f32(a[k * i + o - 1] * r[i]) / f32(2 * k - 1)))
        assert bits(c[i - 1]) == bits(acc), i


# ================================================================================================ cutting
def test_a_stream_cut_into_calls_gives_equal_bits(oracle):
    oracle.lib()
    fs, hop, n_hops = 8000.0, 64, 300
    x = M.edge_inputs(fs, hop, n_hops)["beats"]
    whole = M.Beat(fs, hop).run(x)
    assert whole[2].sum() >= 3
    for step in (1, 7):
        b = M.Beat(fs, hop)
        parts = [b.run(x[i * hop:(i + step) * hop]) for i in range(0, n_hops, step)]
        for k in range(4):
            assert np.array_equal(bits(np.concatenate([p[k] for p in parts])), bits(whole[k])), (step, k)
    b = M.Beat(fs, hop)
    b.run(x[:100 * hop])
    b.reset()
    again = b.run(x)
    assert all(np.array_equal(bits(again[k]), bits(whole[k])) for k in range(4))


# ================================================================================================ click tracks
# bpm -> (the last 8 beat intervals in hops, the final tempo): what the model gives with the oracle's transform, pinned.  A
# prototype on numpy's transform gave the same intervals and tempi; the grid is 2 bpm and bp is rounded to whole hops, so
# 90 bpm (57.4 hops) is tracked at bp = 59 -> 87.6 bpm, 120 (43.07) at 44 -> 117.5, 150 (34.45) at 35 -> 147.7.
PINNED = {90: ([57, 57, 58, 57, 58, 57, 57, 58], 87.59269),
          120: ([43, 43, 43, 43, 43, 43, 44, 43], 117.453835),
          150: ([35, 34, 35, 34, 34, 35, 34, 35], 147.65625)}


@pytest.mark.parametrize("bpm", sorted(PINNED))
def test_click_track_is_followed(oracle, bpm):
    """20 s at 44100/512: decaying noise bursts of 400 samples every 60/bpm s plus a 220 Hz tone at 0.2"""
    oracle.lib()
    odf, score, beat, tempo = M.track(M.click_track(bpm), FS, HOP)
    iv = intervals(beat)
    print("%d bpm: last intervals %s, final tempo %.5f" % (bpm, iv[-8:].tolist(), tempo[-1]))
    assert abs(np.median(iv[-8:]) - 60.0 * FS / (bpm * HOP)) <= 1.0
    assert abs(float(tempo[-1]) - bpm) <= 3.0
    assert iv[-8:].tolist() == PINNED[bpm][0] and tempo[-1] == f32(PINNED[bpm][1])
    assert np.all(score > 0) and odf.size == int(20 * FS) // HOP


# ================================================================================================ the claim
def test_the_claim_percussive_separation_in_front_of_the_tracker(oracle):
    """The 120 bpm click track under ten partials of 110 Hz of total amplitude 1.0 whose amplitudes step every 0.37 s, off
    the beat (beat_model.claim_input), 20 s; tracked as it is and behind oracle.HPR (causal, hop 1024, beta 2.5, percussive
    output).  Error: |interval - 43.066| in hops.  Pinned as measured: both lock on (every interval from the 6th on is 43
    +- 1 either way); with the separation the mean error over all 38 intervals is 0.940 hops against 1.207 without, over the
    last 8 it is 0.066 against 0.175, and the final tempo is 120.19 bpm against 117.45.  So on this input the separation
    helps, modestly: the tracker alone already copes with the steps of the harmonic mix."""
    oracle.lib()
    x = M.claim_input()
    m = x.size // 1024 * 1024
    perc = oracle.HPR(FS, 1024, 2.5, oracle.OUTPUT_PERCUSSIVE, oracle.TIME_CAUSAL).process_stream(x[:m])["P"]
    ideal = 60.0 * FS / (120 * HOP)
    res = {}
    for name, sig in (("with", perc), ("without", x[:m])):
        _, _, beat, tempo = M.track(sig, FS, HOP)
        iv = intervals(beat)
        res[name] = (iv, float(np.mean(np.abs(iv - ideal))), float(np.mean(np.abs(iv[-8:] - ideal))), float(tempo[-1]))
        print("%s HPR: %d intervals %s, mean error %.4f, last 8 %.4f, final tempo %.3f" % ((name, iv.size, iv.tolist()) + res[name][1:]))
    w, wo = res["with"], res["without"]
    assert w[0].size == wo[0].size == 38
    assert np.all(np.abs(w[0][5:] - 43) <= 1) and np.all(np.abs(wo[0][5:] - 43) <= 1)
    assert abs(w[1] - 0.940) < 0.001 and abs(wo[1] - 1.207) < 0.001
    assert abs(w[2] - 0.066) < 0.001 and abs(wo[2] - 0.175) < 0.001
    assert abs(w[3] - 120.185) < 0.01 and abs(wo[3] - 117.454) < 0.01
    assert w[1] < wo[1] and w[2] < wo[2] and abs(w[3] - 120) < abs(wo[3] - 120)
