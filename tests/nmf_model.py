"""CPU model of libzen_hip_nmf.so (zen_amd/nmf): non-negative matrix factorisation of the magnitude spectrogram with the
Kullback-Leibler divergence and multiplicative updates (Lee and Seung 2001), dictionaries learned per source and held fixed
on the mixture (Smaragdis and Brown 2003, Virtanen 2007), written out step by step.

The arithmetic is the contract of zen_amd/nmf/zen_hip_nmf.h and DESIGN.md section 20, and the kernels give the same bits.
The frames, the magnitudes and the resynthesis are tests/repet_model.py's.  Every sum of a product is the segmented chain
`sdot`: float32 fma chains (tests/repsim_model.py's fma32, a correctly rounded float32 fma on numpy arrays) over segments of
256 indices in rising order from +0, the segment sums added in rising order.
"""
import numpy as np

import repet_model as R
from repsim_model import fma32

f32 = np.float32
MAX_COMPONENTS = 256
MAX_FRAMES = R.MAX_FRAMES
SEGMENT = 256
EPS = f32(2.0 ** -40)
MASK64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ initial values
def splitmix64(seed, i):
    """value i of the splitmix64 stream of `seed`, in Python integers"""
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def init(seed, count):
    """float32((x >> 40) + 1) 2^-24 of every value: in (0, 1], exact"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & MASK64) + (np.arange(count, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (((z >> np.uint64(40)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24).astype(f32)


# ------------------------------------------------------------------------------------------------ the segmented chain
def chain_product(A, B):
    """C[i][j] = sdot over l of (A[i][l], B[l][j]) for A (I, L) and B (L, J), every element at once"""
    A, B = np.asarray(A, f32), np.asarray(B, f32)
    L = A.shape[1]
    assert B.shape[0] == L and L >= 1
    total = None
    for l0 in range(0, L, SEGMENT):
        c = np.zeros((A.shape[0], B.shape[1]), f32)
        for l in range(l0, min(l0 + SEGMENT, L)):
            c = fma32(A[:, l][:, None], B[l][None, :], c)
        with np.errstate(over="ignore"):
            total = c if total is None else (total + c).astype(f32)
    return total


def sdot(u, v):
    u, v = np.asarray(u, f32).reshape(1, -1), np.asarray(v, f32).reshape(-1, 1)
    return chain_product(u, v)[0, 0]


def row_sums(A):
    """sdot of every row with ones"""
    A = np.asarray(A, f32)
    return chain_product(A, np.ones((A.shape[1], 1), f32))[:, 0]


# ------------------------------------------------------------------------------------------------ one iteration
def model(W, H):
    """L[a][f] = the chain over k of (H[k][a], W[k][f]); K <= 256, so one segment"""
    assert W.shape[0] <= SEGMENT
    return chain_product(np.asarray(H, f32).T, W)


def ratio(V, W, H):
    """(Q, L): Q = V / max(L, eps)"""
    lam = model(W, H)
    with np.errstate(all="ignore"):
        return (np.asarray(V, f32) / np.maximum(lam, EPS)).astype(f32), lam


def update_h(W, Q, H):
    """H'[k][a] = (H[k][a] P[k][a]) / max(s[k], eps), P = W Q^T, s = the row sums of W"""
    P = chain_product(W, np.asarray(Q, f32).T)
    s = row_sums(W)
    with np.errstate(all="ignore"):
        return ((np.asarray(H, f32) * P).astype(f32) / np.maximum(s, EPS)[:, None]).astype(f32)


def update_w(H, Q, W, fixed=0):
    """W'[k][f] = (W[k][f] G[k][f]) / max(t[k], eps) for k >= fixed, G = H Q, t = the row sums of H; the rows below stay"""
    W = np.array(W, f32)
    if fixed < W.shape[0]:
        G = chain_product(H[fixed:], Q)
        t = row_sums(H[fixed:])
        with np.errstate(all="ignore"):
            W[fixed:] = ((W[fixed:] * G).astype(f32) / np.maximum(t, EPS)[:, None]).astype(f32)
    return W


def iterate(V, W, H, fixed=0):
    """(W', H') after one iteration"""
    K = W.shape[0]
    H = update_h(W, ratio(V, W, H)[0], H)
    if fixed < K:
        W = update_w(H, ratio(V, W, H)[0], W, fixed)
    return W, H


def fit(V, W, H, fixed=0, iterations=100, each=None):
    """(W, H) after `iterations`; each(i, W, H) is called with every state, the initial one (i = 0) included"""
    W, H = np.array(W, f32), np.array(H, f32)
    if each:
        each(0, W, H)
    for i in range(iterations):
        W, H = iterate(V, W, H, fixed)
        if each:
            each(i + 1, W, H)
    return W, H


def kl_divergence(V, W, H):
    """sum of V log(V / L) - V + L in float64 on the float32 states (0 log 0 = 0), L = H^T W in float64"""
    V = np.asarray(V, np.float64)
    lam = np.asarray(H, np.float64).T @ np.asarray(W, np.float64)
    with np.errstate(all="ignore"):
        t = np.where(V > 0, V * np.log(V / lam), 0.0)
    return float(np.sum(t - V + lam))


# ------------------------------------------------------------------------------------------------ stems
def group_masks(W, H, groups, n_groups):
    """M_g = L_g / L where L > 0, else +0: (n_groups, m, F); L_g is the chain over the components of group g in rising k"""
    W, H = np.asarray(W, f32), np.asarray(H, f32)
    groups = np.asarray(groups)
    lam = model(W, H)
    M = np.zeros((n_groups,) + lam.shape, f32)
    for g in range(n_groups):
        ks = np.flatnonzero(groups == g)
        lg = model(W[ks], H[ks]) if ks.size else np.zeros_like(lam)
        with np.errstate(all="ignore"):
            M[g] = np.where(lam > 0, lg / np.where(lam > 0, lam, f32(1)), f32(0)).astype(f32)
    return M


def stems(X, W, H, groups, n_groups, n):
    """(n_groups, n) float32: every group's mask through tests/repet_model.py's resynthesis"""
    M = group_masks(W, H, groups, n_groups)
    return np.stack([R.resynthesis(X, M[g], n) for g in range(n_groups)])


# ------------------------------------------------------------------------------------------------ the whole call
class Result:
    pass


def process(x, N, W, H, fixed=0, iterations=100, groups=None, n_groups=0, keep=False):
    """One clip: what zen_hip_nmf_process_* leaves.  Returns an object with W, H, stems (None without groups) and, with
    keep, X and V."""
    x = np.asarray(x, f32)
    H_ = N // 2
    m = R.n_frames(x.size, H_)
    W, H = np.asarray(W, f32), np.asarray(H, f32)
    K = W.shape[0]
    assert x.size >= 1 and m <= MAX_FRAMES and 1 <= K <= MAX_COMPONENTS and W.shape == (K, H_ + 1) and H.shape == (K, m) and 0 <= fixed <= K
    r = Result()
    X = R.spectra(x, N)
    V = R.magnitude(X)
    r.W, r.H = fit(V, W, H, fixed, iterations)
    r.stems = stems(X, r.W, r.H, groups, n_groups, x.size) if groups is not None else None
    if keep:
        r.X, r.V = X, V
    return r


def initial(seed, K, F, m):
    """(W, H) as the binding and the demo start them: W from `seed`, H from `seed + 1`"""
    return init(seed, K * F).reshape(K, F), init(seed + 1, K * m).reshape(K, m)


def train(x, N, K, iterations=100, seed=0):
    """the dictionary zen_amd.nmf.train learns"""
    x = np.asarray(x, f32)
    W, H = initial(seed, K, N // 2 + 1, R.n_frames(x.size, N // 2))
    return process(x, N, W, H, 0, iterations).W


def separate(x, N, dictionaries, iterations=100, free=0, seed=0, keep=False):
    """what zen_amd.nmf.separate computes: the Result of process with the dictionaries held"""
    x = np.asarray(x, f32)
    F, m = N // 2 + 1, R.n_frames(x.size, N // 2)
    fixed = sum(d.shape[0] for d in dictionaries)
    K = fixed + free
    groups = [g for g, d in enumerate(dictionaries) for _ in range(d.shape[0])] + [len(dictionaries)] * free
    W = np.concatenate(list(dictionaries) + ([init(seed, free * F).reshape(free, F)] if free else [])).astype(f32)
    return process(x, N, W, init(seed + 1, K * m).reshape(K, m), fixed, iterations, groups, len(dictionaries) + (1 if free else 0), keep)


# ------------------------------------------------------------------------------------------------ inputs of the tests
FAMILY_FS = 8000.0
FAMILY_NOTES = ((220.0, 277.0, 330.0, 415.0), (247.0, 311.0, 370.0, 466.0))
FAMILY_HARMONICS = ((1, 2, 3), (1, 3, 5))
FAMILY_COMPONENTS, FAMILY_ITERATIONS = 6, 60
FAMILY = tuple((seed, N) for seed in range(4) for N in (256, 512))


def family_source(which, seed, N, part):
    """Source `which` (0: A, harmonics 1 2 3; 1: B, harmonics 1 3 5; each at 1 / h): 12 Hann-shaped notes of four hops at
    seeded random positions in a clip of 40 hops + 37 samples.  part: 0 the training clip, 1 the test clip -- drawn apart."""
    H = N // 2
    n = 40 * H + 37
    rng = np.random.default_rng(100000 * part + 1000 * seed + 10 * N + which)
    L = 4 * H
    hann = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(L) / L)
    t = np.arange(L) / FAMILY_FS
    x = np.zeros(n)
    for _ in range(12):
        f0 = FAMILY_NOTES[which][int(rng.integers(0, 4))]
        o = int(rng.integers(0, n - L + 1))
        note = sum(np.sin(2 * np.pi * h * f0 * t + rng.uniform(0, 2 * np.pi)) / h for h in FAMILY_HARMONICS[which])
        x[o:o + L] += 0.25 * hann * note
    return x.astype(f32)


def family_clip(seed, N):
    """(mixture, source A, source B) of the test part"""
    a, b = family_source(0, seed, N, 1), family_source(1, seed, N, 1)
    return (a + b).astype(f32), a, b


def family_dictionaries(seed, N, K=FAMILY_COMPONENTS, iterations=FAMILY_ITERATIONS):
    """the two dictionaries learned from the training part, with the model"""
    return [train(family_source(w, seed, N, 0), N, K, iterations, seed) for w in (0, 1)]


sdr = R.sdr

