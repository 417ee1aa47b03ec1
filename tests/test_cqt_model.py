"""CPU checks of tests/cqt_model.py, the step-by-step model of libzen_hip_cqt.so: the plan of the four prototype shapes, the
model against an independent float64 restatement of the construction written here with numpy.fft (no oracle, no model code),
the phase in which neighbouring slices meet, the toy separation and the soft masks.  No device and no library: the model
alone.

Measured here (float32 model against the float64 restatement, largest absolute difference over the largest absolute value
of the float64 side), on the shapes (256, 4, 300, 8000, n 1000) and (1024, 12, 60, 8000, n 3000):
    coefficients 1.13e-7 and 1.21e-7; V 1.73e-7 and 1.68e-7; inverse(forward(x)) against x 1.53e-7 and 1.95e-7;
    harm + perc + resid against x (hard masks) 1.89e-7 and 2.41e-7; harm + perc against x (soft masks) 1.53e-7 and 2.27e-7.
The bounds below are 4 x those: float-order headroom, as DESIGN.md section 18 has them.  The restatement itself gives a
random clip back to a few 1e-15 (bound 1e-13: the structural check).
"""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cqt_model as M  # noqa: E402

SHAPES = [(256, 4, 300.0, 8000.0, 1000), (256, 12, 100.0, 8000.0, 129), (1024, 12, 60.0, 8000.0, 3000), (64, 3, 500.0, 8000.0, 100)]
# 4 x the distances in the docstring, per shape index
BOUND = {0: {"c": 4 * 1.13e-7, "V": 4 * 1.73e-7, "inv": 4 * 1.53e-7, "hard": 4 * 1.89e-7, "soft": 4 * 1.53e-7},
         2: {"c": 4 * 1.21e-7, "V": 4 * 1.68e-7, "inv": 4 * 1.95e-7, "hard": 4 * 2.41e-7, "soft": 4 * 2.27e-7}}


# ================================================================================================ the float64 restatement
class Ref:
    """The construction again, in float64 with numpy.fft, from the formulas of zen_hip_cqt.h: full band windows (nb, N + 1)
    rather than per-bin tables, ifft * M and fft of numpy rather than the engine's transforms."""

    def __init__(self, Ls, B, fmin, fs):
        N, r = Ls // 2, 2.0 ** (1.0 / B)
        p = [0, max(4, int(math.floor(fmin * Ls / fs + 0.5)))]
        while True:
            nx = max(p[-1] + 4, int(math.floor(p[-1] * r + 0.5)))
            if nx > N - 4:
                break
            p.append(nx)
        p.append(N)
        nb = len(p)
        g = np.zeros((nb, N + 1))
        for k in range(nb):
            if k > 0:
                for b in range(p[k - 1], p[k] + 1):
                    g[k, b] = 0.5 - 0.5 * math.cos(math.pi * (b - p[k - 1]) / (p[k] - p[k - 1]))
            if k < nb - 1:
                for b in range(p[k], p[k + 1] + 1):
                    g[k, b] = 0.5 + 0.5 * math.cos(math.pi * (b - p[k]) / (p[k + 1] - p[k]))
        width = max(p[min(k + 1, nb - 1)] - p[max(k - 1, 0)] - 1 for k in range(nb))
        Mc = 32
        while Mc < width:
            Mc *= 2
        self.Ls, self.N, self.p, self.nb, self.M, self.g = Ls, N, p, nb, Mc, g
        self.gd = g / (Mc * (g * g).sum(0))
        self.h = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(Ls) / Ls)
        self.s = self.h / (self.h ** 2 + np.roll(self.h, N) ** 2)

    def forward(self, x):
        N, Ls, M_, nb = self.N, self.Ls, self.M, self.nb
        ns = -(-x.size // N) + 1
        xp = np.zeros((ns + 1) * N)
        xp[N:N + x.size] = x
        c = np.zeros((ns, nb, M_), complex)
        for q in range(ns):
            F = np.fft.fft(xp[q * N:q * N + Ls] * self.h)
            for k in range(nb):
                buf = np.zeros(M_, complex)
                for b in np.nonzero(self.g[k])[0]:
                    buf[b % M_] += F[b] * self.g[k, b]
                c[q, k] = np.fft.ifft(buf) * M_
        return c

    def matrix(self, c):
        ns, nb, M_ = c.shape
        A = np.zeros(((ns + 1) * M_ // 2, nb), complex)
        for q in range(ns):
            A[q * M_ // 2:q * M_ // 2 + M_] += c[q].T
        return A

    def inverse(self, c, n, mask=None):
        ns, nb, M_ = c.shape
        N, Ls = self.N, self.Ls
        out = np.zeros((ns + 1) * N)
        for q in range(ns):
            cq = c[q] if mask is None else c[q] * mask[q * M_ // 2:q * M_ // 2 + M_].T
            Y = np.zeros(Ls, complex)
            for k in range(nb):
                G = np.fft.fft(cq[k])
                for b in np.nonzero(self.g[k])[0]:
                    Y[b] += G[b % M_] * self.gd[k, b]
            Y[0], Y[N] = Y[0].real, Y[N].real
            Y[N + 1:] = np.conj(Y[1:N][::-1])
            out[q * N:q * N + Ls] += np.fft.ifft(Y).real * self.s
        return out[N:N + n]


def rel(got, want):
    return float(np.abs(np.asarray(got, np.complex128) - want).max() / np.abs(want).max())


def clip(n, seed=0):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


# ================================================================================================ the plan
def test_plan_of_the_prototype_shapes():
    want = {0: (15, 64), 1: (29, 32), 2: (52, 64), 3: (8, 32)}
    for i, (Ls, B, fmin, fs, _) in enumerate(SHAPES):
        pl = M.Plan(fs, Ls, B, fmin)
        assert (pl.nb, pl.M) == want[i], (i, pl.nb, pl.M)
        assert pl.p[0] == 0 and pl.p[-1] == Ls // 2 and min(np.diff(pl.p)) >= 4
        assert pl.p == Ref(Ls, B, fmin, fs).p
    pl = M.Plan(8000.0, 256, 4, 300.0)
    assert pl.p[:4] == [0, 10, 14, 18] and pl.p[-3:] == [88, 105, 128]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d_%d" % s[:2])
def test_tables_partition_the_spectrum_and_the_duals_undo_the_bands(shape):
    """gL + gU and M (gL gdL + gU gdU) are 1 to 2 ulp of float32 (each table is one rounding of a double: half an ulp per
    value, two values per sum); gU is 0 exactly at the centres; the slice window and its dual undo each other at hop N alike"""
    Ls, B, fmin, fs, _ = shape
    pl = M.Plan(fs, Ls, B, fmin)
    gL, gU, gdL, gdU = (t.astype(np.float64) for t in (pl.gL, pl.gU, pl.gdL, pl.gdU))
    ulp = 2.0 ** -23
    assert np.abs(gL + gU - 1).max() <= 2 * ulp
    assert np.abs(pl.M * (gL * gdL + gU * gdU) - 1).max() <= 2 * ulp
    assert np.all(pl.gU[pl.p] == 0) and np.all(pl.gL[pl.p] == 1) and np.all(pl.kb[pl.p] == np.arange(pl.nb))
    assert np.all(np.diff(pl.kb) >= 0) and pl.kb[0] == 0 and pl.kb[-1] == pl.nb - 1
    h, s = pl.h.astype(np.float64), pl.s.astype(np.float64)
    N = Ls // 2
    assert np.abs(Ls * (h[:N] * s[:N] + h[N:] * s[N:]) - 1).max() <= 2 * ulp
    assert np.abs(h[:N] + h[N:] - 1).max() <= 2 * ulp
    ref = Ref(Ls, B, fmin, fs)
    lower = ref.g[pl.kb, np.arange(N + 1)]
    assert np.abs(lower - gL).max() <= ulp and ref.M == pl.M


def test_fewer_than_three_bands_and_bad_parameters_are_refused():
    assert M.centres(8000.0, 64, 3, 3900.0) == [0, 32]
    with pytest.raises(AssertionError):
        M.Plan(8000.0, 64, 3, 3900.0)
    with pytest.raises(AssertionError):
        M.Plan(8000.0, 96, 3, 300.0)
    # 0.2 s of columns (200 at 8000 Hz, M 32, slice 256) made odd upward and clamped to the 64 columns; 12 bands made odd
    assert M.Plan(8000.0, 256, 12, 100.0).default_lengths(129) == (64, 13)
    assert M.Plan(8000.0, 1024, 12, 60.0).default_lengths(3000) == (101, 13)


# ================================================================================================ against the restatement
def test_the_restatement_reconstructs():
    """the structural check: analysis then synthesis in float64 gives the clip back"""
    for Ls, B, fmin, fs, n in SHAPES:
        ref = Ref(Ls, B, fmin, fs)
        x = clip(n).astype(np.float64)
        assert np.abs(ref.inverse(ref.forward(x), n) - x).max() <= 1e-13


@pytest.fixture(scope="module", params=[0, 2], ids=["256_4", "1024_12"])
def pair(request, oracle):
    """the model and the restatement on one random clip of the first or the third shape"""
    oracle.lib()
    Ls, B, fmin, fs, n = SHAPES[request.param]
    x = clip(n, seed=request.param)
    pl, ref = M.Plan(fs, Ls, B, fmin), Ref(Ls, B, fmin, fs)
    c = M.forward(x, pl)
    rc = ref.forward(x.astype(np.float64))
    return request.param, x, pl, ref, c, rc


def test_coefficients_and_magnitudes_against_float64(pair):
    i, x, pl, ref, c, rc = pair
    assert c.shape == rc.shape
    d = rel(c, rc)
    print("coefficients: %.3g" % d)
    assert d <= BOUND[i]["c"]
    V, rV = M.magnitude(M.overlap(c, pl)), np.abs(ref.matrix(rc))
    d = rel(V, rV)
    print("V: %.3g" % d)
    assert V.shape == rV.shape and d <= BOUND[i]["V"]


def test_inverse_of_forward_is_the_clip(pair):
    i, x, pl, ref, c, rc = pair
    d = rel(M.inverse(c, pl, x.size), x.astype(np.float64))
    print("inverse(forward(x)) - x: %.3g" % d)
    assert d <= BOUND[i]["inv"]


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_the_stems_sum_to_the_clip(pair, soft):
    i, x, pl, ref, c, rc = pair
    Ls, B, fmin, fs, n = SHAPES[i]
    r = M.separate(x, fs, Ls, B, fmin, soft=soft)
    total = r.harmonic.astype(np.float64) + r.percussive + r.residual
    d = rel(total, x.astype(np.float64))
    print("stems - x (%s): %.3g" % ("soft" if soft else "hard", d))
    assert d <= BOUND[i]["soft" if soft else "hard"]
    if soft:
        assert np.all(r.residual.view(np.uint32) == 0), "the soft residual is +0"
        mh, mp, mr = M.masks(r.H, r.P, soft=True)
        assert mr is None and np.abs(mh.astype(np.float64) + mp - (r.H * r.H + r.P * r.P > 0)).max() <= 2.0 ** -23
    else:
        mh, mp, mr = M.masks(r.H, r.P, 2.0)
        assert np.all(mh + mp + mr == 1), "the hard masks are a partition"
        assert mh.sum() > 0 and mp.sum() > 0 and mr.sum() > 0


# ================================================================================================ phase, the toy separation
TOY = dict(Ls=1024, B=12, fmin=60.0, fs=8000.0, n=8000)


def test_slices_meet_in_phase(oracle):
    """a stationary sinusoid at an odd-centred band: V of that band varies by less than 10 % over the interior columns; with
    the bins of a band folded at their index relative to the centre instead, neighbouring slices cancel there"""
    oracle.lib()
    pl = M.Plan(TOY["fs"], TOY["Ls"], TOY["B"], TOY["fmin"])
    k = next(k for k in range(10, pl.nb - 1) if pl.p[k] % 2 == 1)
    f0 = pl.p[k] * TOY["fs"] / TOY["Ls"]
    x = np.sin(2 * np.pi * f0 * np.arange(TOY["n"]) / TOY["fs"]).astype(np.float32)
    F = M.slices(x, pl)
    col = M.magnitude(M.overlap(M.fold(F, pl), pl))[pl.M:-pl.M, k]
    print("V of band %d (centre %d): %.1f .. %.1f" % (k, pl.p[k], col.min(), col.max()))
    assert col.max() > 100 and (col.max() - col.min()) / col.max() < 0.1

    def fold_centred(F):
        ns = F.shape[0]
        buf = np.zeros((ns, pl.nb, pl.M), np.complex64)
        for kk in range(pl.nb):
            b = pl.band_bins[kk]
            buf[:, kk, (b - pl.p[kk]) % pl.M] = F[:, b] * pl.band_g[kk]
        return np.fft.ifft(buf, axis=2) * pl.M

    bad = np.abs(M.overlap(fold_centred(F).astype(np.complex64), pl))[pl.M:-pl.M, k]
    assert (bad.max() - bad.min()) / bad.max() > 0.5, "a centred fold index does not add up"


@pytest.fixture(scope="module")
def toy(oracle):
    oracle.lib()
    x, sine, clicks = M.family_clip(TOY["n"], TOY["fs"])
    return x, sine, M.separate(x, TOY["fs"], TOY["Ls"], TOY["B"], TOY["fmin"], beta=2.0, lh=31, lp=7)


def test_the_toy_separation(toy):
    """440.3 Hz plus a click of 5 every 1000 samples, medians 31 columns / 7 bands, beta 2.  The float64 prototype gave
    0.046 rms, 4.36 and 0.046 rms."""
    x, sine, r = toy
    at = np.arange(0, TOY["n"], 1000)
    harm_err = float(np.sqrt(np.mean((r.harmonic.astype(np.float64) - sine) ** 2)))
    perc_at = float(np.abs(r.percussive[at]).mean())
    perc_else = float(np.sqrt(np.mean(np.delete(r.percussive.astype(np.float64), at) ** 2)))
    print("harmonic - sine %.4f rms, percussive at the clicks %.3f, elsewhere %.4f rms" % (harm_err, perc_at, perc_else))
    assert harm_err <= 0.1
    assert perc_at >= 3.5
    assert perc_else <= 0.1


def test_the_toy_band_is_steady(toy):
    x, sine, r = toy
    k = int(np.argmax(r.V.sum(0)))
    col = r.V[r.pl.M:-r.pl.M, k]
    lo, hi = np.percentile(col, 5), np.percentile(col, 95)
    print("band %d: %.0f .. %.0f" % (k, lo, hi))
    assert 450 <= lo and hi <= 550
