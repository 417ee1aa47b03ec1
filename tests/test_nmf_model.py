"""CPU checks of tests/nmf_model.py, the model libzen_hip_nmf.so is compared with bit for bit: the segmented chain against exact
rationals, the initial values against splitmix64 in Python integers, the float32 model against a float64 restatement, the
Kullback-Leibler divergence from iteration to iteration, the held rows, and whether it separates the two-timbre family at
all.  The bounds are derived in DESIGN.md section 20 from what the committed model shows."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import nmf_model as M  # noqa: E402

f32 = np.float32

# the largest deviations of the float32 model from the float64 restatement over the family after its 60
# iterations, relative to the largest magnitude of the float64 quantity; the test allows 4 x each.
MEASURED_DEVIATION = {"W": 4.9e-6, "H": 5.5e-6, "L": 1.2e-6, "stems": 1.1e-6}
# the largest relative rise of the divergence from one iteration to the next (free and fixed dictionaries): none was seen
MEASURED_KL_RISE = 0.0
# the smallest SDR gain of a stem over the mixture the committed model shows on the family, in dB; the test allows 2 dB less
MEASURED_MIN_GAIN = {256: 5.0, 512: 16.5}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ sdot
def round_f32(q):
    """the float32 nearest to the rational q, ties to even, subnormals included"""
    if q == 0:
        return f32(0)
    sign = -1 if q < 0 else 1
    q = abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    e = max(e, -126)
    ulp = Fraction(2) ** (e - 23)
    n = q / ulp
    k = n.numerator // n.denominator
    rem = n - k
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and k & 1):
        k += 1
    return f32(sign * float(k * ulp))


def exact_sdot(u, v):
    total = None
    for l0 in range(0, len(u), M.SEGMENT):
        c = Fraction(0)
        for a, b in zip(u[l0:l0 + M.SEGMENT], v[l0:l0 + M.SEGMENT]):
            c = Fraction(float(round_f32(Fraction(float(a)) * Fraction(float(b)) + c)))
        total = c if total is None else Fraction(float(round_f32(total + c)))
    return round_f32(total)


def sdot_values(kind, L, rng):
    if kind == "ordinary":
        return rng.uniform(0, 1, L).astype(f32), rng.uniform(0, 1, L).astype(f32)
    if kind == "scaled":
        return (rng.uniform(0, 1, L) * 10.0 ** rng.integers(-20, 12, L)).astype(f32), (rng.uniform(0, 1, L) * 10.0 ** rng.integers(-12, 8, L)).astype(f32)
    if kind == "near_tie":      # products that end half a unit in the last place of the running sum
        u = (1 + rng.integers(0, 4, L) * 2.0 ** -12).astype(f32)
        v = (1 + rng.integers(0, 4, L) * 2.0 ** -12).astype(f32)
        u[::3] = f32(2.0 ** -24)
        v[::3] = f32(1 + 2.0 ** -23)
        return u, v
    return (rng.uniform(0, 1, L) * 2.0 ** -100).astype(f32), (rng.uniform(0, 1, L) * 2.0 ** -40).astype(f32)     # subnormal sums


@pytest.mark.parametrize("kind", ["ordinary", "scaled", "near_tie", "subnormal"])
def test_sdot_is_the_segmented_fma_chain_of_exact_rationals(kind):
    rng = np.random.default_rng(["ordinary", "scaled", "near_tie", "subnormal"].index(kind))
    for L in (1, 2, 7, 255, 256, 257, 513):
        u, v = sdot_values(kind, L, rng)
        got, want = M.sdot(u, v), exact_sdot(u, v)
        assert bits(got) == bits(want), (kind, L, got, want)
        assert bits(M.row_sums(u[None, :])[0]) == bits(exact_sdot(u, np.ones(L, f32))), (kind, L)
    if kind == "subnormal":
        assert 0 < float(M.sdot(*sdot_values(kind, 7, rng))) < 2.0 ** -126


def test_sdot_segments_are_summed_in_rising_order():
    """three segments whose sums differ by the order they are added in"""
    u = np.zeros(513, f32)
    u[0], u[256], u[512] = 1.0, 2.0 ** -24, 2.0 ** -24
    one = np.ones(513, f32)
    assert M.sdot(u, one) == f32(1.0)                   # (1 + 2^-24) + 2^-24: both adds round back to 1
    assert M.sdot(u[::-1].copy(), one) == f32(1.0 + 2.0 ** -23)
    m = M.chain_product(np.stack([u, u[::-1]]), np.stack([one, one]).T)
    assert m.shape == (2, 2) and m[0, 0] == f32(1.0) and m[1, 1] == f32(1.0 + 2.0 ** -23)


# ------------------------------------------------------------------------------------------------ init
def test_init_is_splitmix64():
    # the first outputs of splitmix64 seeded with 0 and with 1234567, as published with the generator
    assert [M.splitmix64(0, i) for i in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert [M.splitmix64(1234567, i) for i in range(2)] == [6457827717110365317, 3203168211198807973]
    for seed in (0, 1, 0xFFFFFFFFFFFFFFFF, 123456789012345):
        got = M.init(seed, 300)
        want = np.array([(((M.splitmix64(seed, i)) >> 40) + 1) * 2.0 ** -24 for i in range(300)], np.float64)
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)
        assert got.min() > 0 and got.max() <= 1
    assert not np.array_equal(M.init(0, 50), M.init(1, 50))


# ------------------------------------------------------------------------------------------------ against float64
def fit64(V, W, H, fixed, iterations):
    """the same iteration with numpy's float64 `@`: no segments, the same clamps"""
    V, W, H = (np.array(a, np.float64) for a in (V, W, H))
    eps, K = float(M.EPS), W.shape[0]
    for _ in range(iterations):
        Q = V / np.maximum(H.T @ W, eps)
        H = H * (W @ Q.T) / np.maximum(W.sum(1), eps)[:, None]
        if fixed < K:
            Q = V / np.maximum(H.T @ W, eps)
            W[fixed:] = W[fixed:] * (H[fixed:] @ Q) / np.maximum(H[fixed:].sum(1), eps)[:, None]
    return W, H


@pytest.fixture(scope="module")
def family(oracle):
    """per (seed, N): the mixture, the sources, the two dictionaries and the model's separation, computed once"""
    oracle.lib()
    out = {}
    for seed, N in M.FAMILY:
        x, a, b = M.family_clip(seed, N)
        dicts = M.family_dictionaries(seed, N)
        out[seed, N] = (x, a, b, dicts, M.separate(x, N, dicts, M.FAMILY_ITERATIONS, seed=seed, keep=True))
    return out


def rel(a32, a64):
    return float(np.abs(np.asarray(a32, np.float64) - a64).max() / np.abs(a64).max())


def test_float32_model_stays_near_the_float64_restatement(family):
    worst = {k: 0.0 for k in MEASURED_DEVIATION}
    for (seed, N), (x, a, b, dicts, sep) in family.items():
        # a free fit from the family's initial values, and the separation with the dictionaries held
        xa = M.family_source(0, seed, N, 0)
        Va = M.R.magnitude(M.R.spectra(xa, N))
        W0, H0 = M.initial(seed, M.FAMILY_COMPONENTS, N // 2 + 1, Va.shape[0])
        W64, H64 = fit64(Va, W0, H0, 0, M.FAMILY_ITERATIONS)
        worst["W"] = max(worst["W"], rel(dicts[0], W64))
        K = 2 * M.FAMILY_COMPONENTS
        Wm = np.concatenate(dicts)
        Hm0 = M.init(seed + 1, K * sep.V.shape[0]).reshape(K, -1)
        W64, H64 = fit64(sep.V, Wm, Hm0, K, M.FAMILY_ITERATIONS)
        worst["H"] = max(worst["H"], rel(sep.H, H64))
        lam64 = H64.T @ W64
        worst["L"] = max(worst["L"], rel(M.model(sep.W, sep.H), lam64))
        groups = np.repeat([0, 1], M.FAMILY_COMPONENTS)
        for g in range(2):
            lg = H64[groups == g].T @ W64[groups == g]
            m64 = np.where(lam64 > 0, lg / np.where(lam64 > 0, lam64, 1.0), 0.0)
            full = np.concatenate([m64, m64[:, 1:-1][:, ::-1]], axis=1)
            frames = np.fft.ifft(sep.X.astype(np.complex128) * full, axis=1).real * N
            Hh = N // 2
            t = np.arange(x.size)
            d = M.R.divisor(N).astype(np.float64)
            s64 = (frames[t // Hh, Hh + t % Hh] + frames[t // Hh + 1, t % Hh]) / d[t % Hh]
            worst["stems"] = max(worst["stems"], rel(sep.stems[g], s64))
    print("deviation of the float32 model from float64:", worst)
    for k, v in worst.items():
        assert v <= 4 * MEASURED_DEVIATION[k], (k, v)


@pytest.mark.parametrize("fixed", [0, 12], ids=["free", "held"])
def test_divergence_does_not_rise(family, fixed):
    worst = 0.0
    for (seed, N), (x, a, b, dicts, sep) in family.items():
        K = 2 * M.FAMILY_COMPONENTS
        W0 = np.concatenate(dicts) if fixed else M.init(seed, K * (N // 2 + 1)).reshape(K, -1)
        H0 = M.init(seed + 1, K * sep.V.shape[0]).reshape(K, -1)
        kl = []
        M.fit(sep.V, W0, H0, fixed, 30 if N == 256 else 12, each=lambda i, W, H: kl.append(M.kl_divergence(sep.V, W, H)))
        kl = np.array(kl)
        assert kl[-1] < 0.5 * kl[0]
        worst = max(worst, float(np.max((kl[1:] - kl[:-1]) / kl[:-1])))
    print("largest relative rise of the divergence:", worst)
    assert worst <= 4 * MEASURED_KL_RISE


# ------------------------------------------------------------------------------------------------ held rows
def test_held_rows_keep_every_bit():
    rng = np.random.default_rng(5)
    K, F, m = 5, 33, 40
    V = rng.uniform(0, 1, (m, F)).astype(f32)
    W0, H0 = M.initial(3, K, F, m)
    W, H = M.fit(V, W0, H0, K, 3)
    assert np.array_equal(bits(W), bits(W0)) and not np.array_equal(bits(H), bits(H0))
    for fixed in (1, 4):
        W, H = M.fit(V, W0, H0, fixed, 3)
        assert np.array_equal(bits(W[:fixed]), bits(W0[:fixed]))
        assert all(not np.array_equal(bits(W[k]), bits(W0[k])) for k in range(fixed, K))
    W, _ = M.fit(V, W0, H0, 0, 1)
    assert all(not np.array_equal(bits(W[k]), bits(W0[k])) for k in range(K))


def test_clamps_keep_zero_rows_and_columns_finite():
    """an all-zero spectrum, an all-zero activation row and an all-zero frame: the clamps divide by eps, nothing is a NaN"""
    rng = np.random.default_rng(6)
    K, F, m = 4, 17, 9
    V = rng.uniform(0, 1, (m, F)).astype(f32)
    V[3] = 0
    W0, H0 = M.initial(1, K, F, m)
    W0[1] = 0
    H0[2] = 0
    W, H = M.fit(V, W0, H0, 0, 2)
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(H)) and np.all(W[1] == 0) and np.all(H[2] == 0) and np.all(H[:, 3] == 0)
    masks = M.group_masks(W, H, [0, 0, 1, -1], 2)
    assert np.all(np.isfinite(masks)) and np.all(masks[:, 3] == 0)


# ------------------------------------------------------------------------------------------------ does it separate?
def test_family_is_separated(family):
    gains = {256: [], 512: []}
    for (seed, N), (x, a, b, dicts, sep) in family.items():
        for src, est in ((a, sep.stems[0]), (b, sep.stems[1])):
            gains[N].append(M.sdr(src, est) - M.sdr(src, x))
    for N, g in gains.items():
        print("frame %d: SDR gains over the mixture %.1f .. %.1f dB" % (N, min(g), max(g)))
    for N, g in gains.items():
        assert min(g) >= MEASURED_MIN_GAIN[N] - 2.0, (N, min(g))
