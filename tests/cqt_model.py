"""CPU model of libzen_hip_cqt.so (zen_amd/cqt): an invertible constant-Q transform -- a sliced non-stationary Gabor transform
in matrix form -- and the single-pass harmonic / percussive / residual separation in its domain, written out step by step.

The arithmetic is the contract of zen_amd/cqt/zen_hip_cqt.h and DESIGN.md section 18, and the kernels give the same bits.
Every float operation of the sample path is one of + - * / sqrt compare in float32, one rounding each (numpy's element-wise
float32 operations are such operations); every table is computed in double with math.cos and rounded once; the transforms are
the engine's complex FFT (oracle.fft_c2c) and the medians the engine's (oracle.median_filter).
"""
import math

import numpy as np

f32 = np.float32
WMIN = 4
MAX_SLICES = 4096
TIME_ANTICAUSAL, FREQUENCY = 1, 2


def _fft_rows(z, inverse=False):
    """the unnormalised transform of every row of a (rows, points) complex64 array"""
    from oracle import oracle as o
    z = np.ascontiguousarray(z, np.complex64)
    out = np.empty_like(z)
    for i in range(z.shape[0]):
        out[i] = o.fft_c2c(z[i], inverse=inverse)
    return out


def _median(V, length, direction):
    from oracle import oracle as o
    return o.median_filter(np.ascontiguousarray(V, f32), length, direction)


# ------------------------------------------------------------------------------------------------ the plan and its tables
def centres(fs, Ls, B, fmin):
    """the band centres in bins of the slice: 0, the first band, constant-Q (at least WMIN bins apart) up to N - WMIN, N"""
    fs, N, r = float(f32(fs)), Ls // 2, 2.0 ** (1.0 / B)
    p = [0, max(WMIN, int(math.floor(fmin * Ls / fs + 0.5)))]
    if p[1] > N - WMIN:
        return [0, N]
    while True:
        nx = max(p[-1] + WMIN, int(math.floor(p[-1] * r + 0.5)))
        if nx > N - WMIN:
            break
        p.append(nx)
    p.append(N)
    return p


class Plan:
    """fs, Ls, N, B, fmin, p (centres), nb, M and the tables kb, gL, gU, gdL, gdU (N + 1 values each), h, s (Ls values)"""

    def __init__(self, fs, Ls, B, fmin):
        assert Ls >= 64 and Ls <= 32768 and Ls & (Ls - 1) == 0 and 1 <= B <= 96 and fmin > 0 and fs > 0
        self.fs, self.Ls, self.N, self.B, self.fmin = float(f32(fs)), Ls, Ls // 2, B, fmin
        p, N = centres(fs, Ls, B, fmin), Ls // 2
        assert len(p) >= 3, "fewer than 3 bands"
        self.p, self.nb = p, len(p)
        nb = self.nb
        width = max(p[min(k + 1, nb - 1)] - p[max(k - 1, 0)] - 1 for k in range(nb))
        M = 32
        while M < width:
            M *= 2
        self.M = M
        kb, gL, gU = np.zeros(N + 1, np.int32), np.zeros(N + 1, f32), np.zeros(N + 1, f32)
        for k in range(nb - 1):
            a, c = p[k], p[k + 1]
            for b in range(a, c):
                kb[b] = k
                gL[b] = f32(0.5 + 0.5 * math.cos(math.pi * (b - a) / (c - a)))      # band k falls
                gU[b] = f32(0.5 - 0.5 * math.cos(math.pi * (b - a) / (c - a)))      # band k + 1 rises
        kb[N], gL[N], gU[N] = nb - 1, f32(1.0), f32(0.0)
        den = [M * (float(gL[b]) * float(gL[b]) + float(gU[b]) * float(gU[b])) for b in range(N + 1)]
        self.kb, self.gL, self.gU = kb, gL, gU
        self.gdL = np.array([float(gL[b]) / den[b] for b in range(N + 1)]).astype(f32)
        self.gdU = np.array([float(gU[b]) / den[b] for b in range(N + 1)]).astype(f32)
        h = [0.5 - 0.5 * math.cos(2.0 * math.pi * i / Ls) for i in range(Ls)]
        self.h = np.array(h).astype(f32)
        self.s = np.array([(h[i] / (h[i] * h[i] + h[(i + N) % Ls] * h[(i + N) % Ls])) / Ls for i in range(Ls)]).astype(f32)
        self.centre = np.array([p[kb[b]] == b for b in range(N + 1)])
        # band k: its bins p[k-1] < b < p[k+1] inside [0, N] and its weight there
        self.band_bins, self.band_g = [], []
        for k in range(nb):
            lo, hi = (p[k - 1] + 1 if k else 0), (p[k + 1] - 1 if k < nb - 1 else N)
            b = np.arange(lo, hi + 1)
            self.band_bins.append(b)
            self.band_g.append(np.where(b >= p[k], gL[b], gU[b]).astype(f32))

    def n_slices(self, n):
        return -(-n // self.N) + 1

    def columns(self, n):
        return (self.n_slices(n) + 1) * self.M // 2

    def default_lengths(self, n):
        """(lh, lp): 0.2 s of columns and one octave of bands, made odd upward and clamped to the matrix"""
        T = self.columns(n)
        lh = int(math.floor(0.2 * self.fs * self.M / self.Ls))
        lh += 1 - lh % 2
        lp = self.B + (1 - self.B % 2)
        return min(lh, T), min(lp, self.nb)


# ------------------------------------------------------------------------------------------------ steps 1-3
def slices(x, pl):
    """step 1: F_q of every slice, (ns, Ls) complex64"""
    x = np.asarray(x, f32)
    N, Ls, ns = pl.N, pl.Ls, pl.n_slices(x.size)
    xp = np.zeros((ns + 1) * N, f32)
    xp[N:N + x.size] = x
    rows = np.zeros((ns, Ls), np.complex64)
    for q in range(ns):
        rows[q].real = xp[q * N:q * N + Ls] * pl.h
    return _fft_rows(rows)


def fold(F, pl):
    """step 2: c_q[k], (ns, nb, M) complex64: the band's bins at their absolute index mod M, then the inverse transform"""
    ns = F.shape[0]
    buf = np.zeros((ns, pl.nb, pl.M), np.complex64)
    for k in range(pl.nb):
        b, g = pl.band_bins[k], pl.band_g[k]
        buf.real[:, k, b % pl.M] = F.real[:, b] * g
        buf.imag[:, k, b % pl.M] = F.imag[:, b] * g
    return _fft_rows(buf.reshape(ns * pl.nb, pl.M), inverse=True).reshape(ns, pl.nb, pl.M)


def overlap(c, pl):
    """step 3: A[t][k], (T, nb) complex64: the halves of neighbouring slices added, the earlier slice first"""
    ns, nb, M = c.shape
    half = M // 2
    A = np.empty(((ns + 1) * half, nb), np.complex64)
    for q in range(ns + 1):
        if q == 0:
            a = c[0][:, :half]
        elif q == ns:
            a = c[ns - 1][:, half:]
        else:
            a = np.empty((nb, half), np.complex64)
            a.real = c[q - 1].real[:, half:] + c[q].real[:, :half]
            a.imag = c[q - 1].imag[:, half:] + c[q].imag[:, :half]
        A[q * half:(q + 1) * half] = a.T
    return A


def magnitude(A):
    re, im = A.real.astype(f32), A.imag.astype(f32)
    return np.sqrt(re * re + im * im).astype(f32)


def forward(x, pl):
    return fold(slices(x, pl), pl)


def spectrogram(x, pl):
    return magnitude(overlap(forward(x, pl), pl))


# ------------------------------------------------------------------------------------------------ steps 4-5
def medians(V, lh, lp):
    return _median(V, lh, TIME_ANTICAUSAL), _median(V, lp, FREQUENCY)


def masks(H, P, beta=2.0, soft=False):
    """(harmonic, percussive, residual) masks, float32; the residual mask of the soft form is None: that stem is +0"""
    one, zero = f32(1.0), f32(0.0)
    if soft:
        hh, pp = H * H, P * P
        d = hh + pp
        safe = np.where(d > 0, d, one)
        return np.where(d > 0, hh / safe, zero).astype(f32), np.where(d > 0, pp / safe, zero).astype(f32), None
    beta = f32(beta)
    mh = H > beta * P
    mp = ~mh & (P >= beta * H)
    return np.where(mh, one, zero), np.where(mp, one, zero), np.where(~mh & ~mp, one, zero)


# ------------------------------------------------------------------------------------------------ steps 6-7
def synthesis(c, pl, n, mask=None):
    """steps 6-7: the n samples back from the coefficients (ns, nb, M); mask: None or (T, nb) float32"""
    ns, nb, M = c.shape
    N, Ls, half = pl.N, pl.Ls, M // 2
    assert ns == pl.n_slices(n)
    cm = np.array(c, np.complex64)
    if mask is not None:
        for q in range(ns):
            m = mask[q * half:q * half + M].T
            cm[q].real = c[q].real * m
            cm[q].imag = c[q].imag * m
    G = _fft_rows(cm.reshape(ns * nb, M)).reshape(ns, nb, M)
    b = np.arange(N + 1)
    lo, up = G[:, pl.kb, b % M], G[:, np.minimum(pl.kb + 1, nb - 1), b % M]
    re = np.where(pl.centre, lo.real * pl.gdL, lo.real * pl.gdL + up.real * pl.gdU).astype(f32)
    im = np.where(pl.centre, lo.imag * pl.gdL, lo.imag * pl.gdL + up.imag * pl.gdU).astype(f32)
    im[:, 0] = 0.0
    im[:, N] = 0.0
    Y = np.empty((ns, Ls), np.complex64)
    Y.real[:, :N + 1], Y.imag[:, :N + 1] = re, im
    Y.real[:, N + 1:], Y.imag[:, N + 1:] = re[:, 1:N][:, ::-1], np.negative(im[:, 1:N][:, ::-1])
    y = _fft_rows(Y, inverse=True).real.astype(f32)
    t = np.arange(n)
    q, i = t // N, t % N
    return (y[q, N + i] * pl.s[N + i] + y[q + 1, i] * pl.s[i]).astype(f32)


def inverse(c, pl, n):
    return synthesis(c, pl, n)


# ------------------------------------------------------------------------------------------------ the whole call
class Result:
    pass


def separate(x, fs, Ls, B, fmin, beta=2.0, soft=False, lh=0, lp=0, want=(True, True, True)):
    """One clip.  Returns an object with harmonic, percussive, residual (float32, the clip's length; None where not wanted),
    the plan pl and c, V, H, P."""
    x = np.asarray(x, f32)
    r = Result()
    pl = r.pl = Plan(fs, Ls, B, fmin)
    assert x.size >= 1 and pl.n_slices(x.size) <= MAX_SLICES
    dh, dp = pl.default_lengths(x.size)
    r.lh, r.lp = lh or dh, lp or dp
    r.c = forward(x, pl)
    r.V = magnitude(overlap(r.c, pl))
    r.H, r.P = medians(r.V, r.lh, r.lp)
    mk = masks(r.H, r.P, beta, soft)
    stems = []
    for k in range(3):
        if not want[k]:
            stems.append(None)
        elif mk[k] is None:
            stems.append(np.zeros(x.size, f32))
        else:
            stems.append(synthesis(r.c, pl, x.size, mk[k]))
    r.harmonic, r.percussive, r.residual = stems
    return r


# ------------------------------------------------------------------------------------------------ inputs of the tests
def family_clip(n, fs=8000.0, f0=440.3, every=1000, height=5.0, seed=None, noise=0.0):
    """(mixture, sine, clicks) float32: a sine of f0 Hz plus a click of `height` every `every` samples from sample 0 on, and
    with a seed uniform noise of amplitude `noise` in the mixture"""
    t = np.arange(n)
    sine = np.sin(2 * np.pi * f0 * t / fs)
    clicks = np.zeros(n)
    clicks[::every] = height
    mix = sine + clicks
    if seed is not None:
        mix = mix + noise * np.random.default_rng(seed).uniform(-1, 1, n)
    return mix.astype(f32), sine.astype(f32), clicks.astype(f32)
