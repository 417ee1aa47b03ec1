"""CPU tier: tests/repsim_model.py -- the model the GPU tier compares libzen_hip_repsim.so with bit for bit -- against REPET-SIM
as the paper writes it, in float64 with numpy.fft and a matrix product, written out below.  The parity target is that
independent computation, never the library.  Then fma32 against exact rational arithmetic, the properties of the selection,
and the quality condition on the synthetic family of DESIGN.md section 19."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import repet_model as RM  # noqa: E402
import repsim_model as M  # noqa: E402

FS = M.FAMILY_FS
f32 = np.float32
# The largest deviations measured on PARITY below, each relative to the largest magnitude of the float64 quantity
# (DESIGN.md section 19 lists them), times 4:
TOL = {"V": 4 * 1.30e-7, "S": 4 * 3.32e-6, "U": 4 * 1.69e-7, "background": 4 * 2.47e-7, "foreground": 4 * 1.46e-6}
PARITY = [c for c in M.FAMILY if c[0] == 0]      # the five shapes of the family, seed 0


# ------------------------------------------------------------------------------------------------ fma32
def exact_fma(a, b, c):
    """float32(a b + c) through rational arithmetic.  The rounding is done here, on the integers: handing numpy the double
    nearest the exact value would be the double rounding fma32 avoids."""
    a, b, c = float(a), float(b), float(c)
    v = Fraction(a) * Fraction(b) + Fraction(c)
    if v == 0:      # -0 only as (-0) + (-0); an exact cancellation gives +0
        neg = a * b == 0 and c == 0 and math.copysign(1, a) * math.copysign(1, b) < 0 and math.copysign(1, c) < 0
        return f32(-0.0) if neg else f32(0.0)
    sign, v = (-1 if v < 0 else 1), abs(v)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    while Fraction(2) ** e > v:
        e -= 1
    while Fraction(2) ** (e + 1) <= v:
        e += 1
    q = Fraction(2) ** (max(e, -126) - 23)          # the spacing of float32 at v (the subnormal spacing below 2^-126)
    n, rest = divmod(v, q)
    n = int(n)
    if rest * 2 > q or (rest * 2 == q and n & 1):
        n += 1
    return f32(sign * float(n * q)) if n * q < Fraction(2) ** 128 else f32(sign * math.inf)


def test_fma32_is_correctly_rounded():
    rng = np.random.default_rng(11)
    n = 3000
    cases = []
    a, b = rng.uniform(-2, 2, n).astype(f32), rng.uniform(-2, 2, n).astype(f32)
    cases.append((a, b, rng.uniform(-4, 4, n).astype(f32)))                                         # ordinary
    sc = lambda: (rng.uniform(0.5, 2, n) * 2.0 ** rng.integers(-60, 60, n) * rng.choice([-1, 1], n)).astype(f32)  # noqa: E731
    cases.append((sc(), sc(), sc()))                                                                # widely scaled
    # near ties: the product's low bits sit at half a unit of c's last place
    c = rng.uniform(1, 2, n).astype(f32)
    a = (1 + rng.integers(0, 1 << 12, n) * 2.0 ** -12).astype(f32)
    b = (np.float64(2.0 ** -24) * (1 + rng.integers(-2, 3, n) * 2.0 ** -11)).astype(f32)
    cases.append((a, b, c))
    cases.append((a, (-b).astype(f32), c))
    # subnormal results and operands
    tiny = lambda: (rng.uniform(-1, 1, n) * 2.0 ** rng.integers(-75, -60, n)).astype(f32)          # noqa: E731
    cases.append((tiny(), tiny(), (rng.integers(-40, 40, n) * 1.401298464324817e-45).astype(f32)))
    cases.append(((rng.integers(-9, 9, n) * 1.401298464324817e-45).astype(f32), rng.uniform(-3, 3, n).astype(f32),
                  (rng.integers(-9, 9, n) * 1.401298464324817e-45).astype(f32)))
    for a, b, c in cases:
        got = M.fma32(a, b, c)
        assert got.dtype == f32
        want = np.array([exact_fma(x, y, z) for x, y, z in zip(a, b, c)], f32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the signs of zero, the infinities and NaN of the IEEE operation
    z = M.fma32(f32([-0.0, 0.0, -0.0, -1e-30]), f32([0.0, 0.0, 0.0, 1e-30]), f32([-0.0, -0.0, 0.0, 0.0]))
    assert list(np.signbit(z)) == [True, False, False, True] and np.all(z == 0)
    big = M.fma32(f32([3e38, 3e38, np.inf]), f32([2.0, 2.0, 0.0]), f32([0.0, -np.inf, 1.0]))
    assert big[0] == np.inf and big[1] == -np.inf and np.isnan(big[2])


def test_the_chain_is_symmetric_and_padding_is_harmless():
    rng = np.random.default_rng(5)
    V = rng.uniform(-1, 1, (9, 7)).astype(f32)
    D = M.gram(V)
    assert np.array_equal(D.view(np.uint32), D.T.view(np.uint32))
    assert np.array_equal(M.gram(np.hstack([V, np.zeros((9, 3), f32)])).view(np.uint32), D.view(np.uint32))
    S = M.similarity(np.vstack([V, np.zeros((1, 7), f32)]))
    assert np.all(S[9].view(np.uint32) == 0) and np.all(S[:, 9].view(np.uint32) == 0), "an all-zero row: +0"
    assert np.all(np.abs(np.diagonal(S)[:9] - 1) < 3e-7)


# ------------------------------------------------------------------------------------------------ float64 REPET-SIM
def ref_select(S, t, dd, k):
    rows, m = S.shape
    out = []
    for a in range(rows):
        row, acc = np.where(S[a] > t, S[a], -np.inf), []
        while len(acc) < k and np.max(row) > -np.inf:
            j = int(np.argmax(row))
            acc.append(j)
            row[max(0, j - dd + 1):j + dd] = -np.inf
        out.append(acc)
    return out


def ref_repsim(x, fs, N, t, dd, k, highpass, idx=None):
    """V, S, the selection (lists), U, background, foreground in float64; idx: the selection to use instead"""
    x = np.asarray(x, np.float64)
    H, n = N // 2, x.size
    m = -(-n // H) + 1
    w = 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(N) / N)
    xp = np.concatenate([np.zeros(H), x, np.zeros((m + 1) * H - H - n)])
    X = np.fft.fft(np.stack([xp[a * H:a * H + N] * w for a in range(m)]), axis=1)
    V = np.abs(X[:, :H + 1])
    nrm = np.sqrt(np.sum(V * V, axis=1))
    den = nrm[:, None] * nrm[None, :]
    S = np.where(den > 0, (V @ V.T) / np.where(den > 0, den, 1.0), 0.0)
    sel = ref_select(S, t, dd, k)
    use = sel if idx is None else idx
    U = np.stack([np.median(V[list(js)], axis=0) if len(js) else np.zeros(H + 1) for js in use])
    Mk = np.where(V > 0, np.minimum(U, V) / np.where(V > 0, V, 1.0), 0.0)
    kc = int(math.ceil(highpass * N / fs)) if highpass > 0 else 0
    Mk[:, :kc] = 1.0
    full = np.concatenate([Mk, Mk[:, 1:H][:, ::-1]], axis=1)
    G = np.fft.ifft(X * full, axis=1).real * N
    d = N * (w[:H] + w[H:])
    s = np.arange(n)
    bg = (G[s // H, H + s % H] + G[s // H + 1, s % H]) / d[s % H]
    return V, S, sel, U, bg, x - bg


def rel(got, ref):
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref)) / np.max(np.abs(ref)))


@pytest.fixture(scope="module")
def family(oracle):
    """every clip of the family with the model's result"""
    oracle.lib()
    out = {}
    for key in M.FAMILY:
        seed, N, P, Q, reps = key
        x, bg, fg = M.family_clip(seed, N, P, Q, reps)
        out[key] = (x, bg, fg, M.family_separate(x, N, keep=True))
    return out


@pytest.mark.parametrize("key", PARITY, ids=lambda k: "N%d_p%d_q%d_r%d" % k[1:])
def test_every_step_against_float64_repsim(family, key):
    """U and the stems with the float64 code fed the model's own selection: the selection is discontinuous in S"""
    seed, N, P, Q, reps = key
    x, _, _, got = family[key]
    idx = [list(got.idx[a, :got.counts[a]]) for a in range(len(got.counts))]
    V, S, _, U, bg, fg = ref_repsim(x, FS, N, M.FAMILY_THRESHOLD, 2, M.FAMILY_NUMBER, 0.0, idx)
    dev = {"V": rel(got.V, V), "S": rel(got.S, S), "U": rel(got.U, U), "background": rel(got.background, bg), "foreground": rel(got.foreground, fg)}
    print(key, dev)
    for k, v in dev.items():
        assert v <= TOL[k], (k, v, TOL[k])
    assert got.V.dtype == got.S.dtype == got.U.dtype == got.background.dtype == got.foreground.dtype == np.float32


def test_the_selection_is_the_float64_codes_on_every_frame_of_the_family(family):
    """Every frame of the twenty clips selects the same six frames in float32 and in float64.  A pattern that comes back brings
    frames whose similarities differ by less than float32 resolves, so the order of acceptance may differ between two such
    frames (7 of the 3212 frames of the family, by at most 6.6e-7 in S): where it does, the float64 similarities of the two
    frames at the same place of the order are within the deviation S is allowed above."""
    frames = swapped = 0
    for key, (x, _, _, got) in family.items():
        _, S, sel = ref_repsim(x, FS, key[1], M.FAMILY_THRESHOLD, 2, M.FAMILY_NUMBER, 0.0)[:3]
        assert M.distance_frames(M.family_distance(key[1]), FS, key[1] // 2, len(sel)) == 2
        for a, js in enumerate(sel):
            mine = [int(j) for j in got.idx[a, :got.counts[a]]]
            assert sorted(mine) == sorted(js), (key, a, mine, js)
            frames += 1
            if mine != js:
                swapped += 1
                assert max(abs(S[a, p] - S[a, q]) for p, q in zip(mine, js)) <= TOL["S"], (key, a, mine, js)
    print("frames %d, of which %d accept two near-equal frames in the other order" % (frames, swapped))


# ------------------------------------------------------------------------------------------------ the selection
def test_selection_properties_on_random_matrices_with_ties():
    rng = np.random.default_rng(3)
    levels = np.array([0.0, 0.1, 0.25, 0.5, 0.5, 0.75, 0.9, 1.0], f32)
    for m, dd, k, t in ((40, 1, 5, 0.0), (40, 3, 10, 0.0), (97, 5, 40, 0.5), (30, 33, 4, 0.0), (64, 2, 256, 0.2), (50, 4, 7, 0.9)):
        S = levels[rng.integers(0, levels.size, (m, m))]
        S[3] = 0.0
        S[5, 7] = np.nan
        idx, counts = M.select(S, t, min(dd, m), k)
        assert idx.shape == (m, k) and idx.dtype == np.int32 and counts[3] == 0
        for a in range(m):
            c, js = counts[a], idx[a, :counts[a]]
            assert np.all(idx[a, c:] == -1) and np.all((js >= 0) & (js < m)) and len(set(js)) == c
            vals = S[a, js]
            assert np.all(vals > f32(t)), "accepted values are above the threshold (a NaN is not)"
            assert np.all(np.diff(vals) <= 0), "values do not rise along the order of acceptance"
            assert all(abs(int(p) - int(q)) >= dd for i, p in enumerate(js) for q in js[:i]), "accepted frames are dd apart"
            free = [b for b in range(m) if S[a, b] > f32(t) and all(abs(b - int(j)) >= dd for j in js)]
            assert c == k or not free, "c_a = k wherever a greedy pick was still possible"
            if c:
                first = int(np.flatnonzero(S[a] == np.nanmax(np.where(S[a] > f32(t), S[a], -np.inf)))[0])
                assert js[0] == first, "the first index wins ties"
            for i in range(1, c):                           # every pick: the first index of the largest value still free
                ok = [b for b in range(m) if S[a, b] > f32(t) and all(abs(b - int(j)) >= dd for j in js[:i])]
                best = max(S[a, b] for b in ok)
                assert js[i] == min(b for b in ok if S[a, b] == best)


def test_median_over_selected_frames():
    V = np.array([[1, 9], [5, 9], [3, 2], [7, 2], [2, 9]], f32)
    idx = np.array([[4, 0, 2, -1], [1, 3, -1, -1], [0, 1, 2, 3], [-1, -1, -1, -1]], np.int32)
    U = M.gather_median(V, idx, np.array([3, 2, 4, 0], np.int32))
    assert np.array_equal(U, np.array([[2, 9], [6, 5.5], [4, 5.5], [0, 0]], f32)) and not np.any(np.signbit(U[3]))
    big = M.gather_median(np.array([[3e38], [3e38]], f32), np.array([[0, 1]], np.int32), np.array([2], np.int32))
    assert np.isinf(big[0, 0])      # (s[0] + s[1]) * 0.5f in float32, as the device adds


def test_a_silent_clip_gives_silence_and_the_input(oracle):
    oracle.lib()
    x = np.zeros(3000, np.float32)
    x[5] = -0.0
    r = M.separate(x, FS, 256, keep=True)
    assert np.all(r.counts == 0) and np.all(r.idx == -1) and np.all(r.S.view(np.uint32) == 0)
    assert np.all(r.background.view(np.uint32) == 0) and np.array_equal(r.foreground.view(np.uint32), x.view(np.uint32))


# ------------------------------------------------------------------------------------------------ the quality condition
def test_the_family_has_no_single_period_and_every_frame_finds_six(family):
    assert len(family) == 20
    for key, (_, _, _, got) in family.items():
        assert np.all(got.counts == M.FAMILY_NUMBER), (key, got.counts.min())


def test_the_foreground_gains_eight_decibels_and_beats_repet_by_one(family, oracle):
    oracle.lib()
    gains, margins = {}, {}
    for key, (x, _, fg, got) in family.items():
        seed, N, P, Q, reps = key
        mine = M.sdr(fg, got.foreground)
        gains[key] = mine - M.sdr(fg, x)
        repet = max(M.sdr(fg, RM.separate(x, FS, N, p, highpass=0.0).foreground) for p in (P, Q * P))
        margins[key] = mine - repet
    print("foreground SDR gain: min %.2f dB, max %.2f dB; over REPET with the better of its two periods: min %.2f dB, max %.2f dB"
          % (min(gains.values()), max(gains.values()), min(margins.values()), max(margins.values())))
    for key in family:
        assert gains[key] >= 8.0, (key, gains[key])
        assert margins[key] >= 1.0, (key, margins[key])
