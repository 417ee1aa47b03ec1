"""CPU model of libzen_hip_pitch.so (zen_amd/pitch): the McLeod pitch method on one chunk, written out step by step.

The arithmetic is the contract of DESIGN.md section 13 and the kernels give the same bits: both transforms are the
engine's complex FFT (oracle.fft_c2c), the power spectrum is two float32 multiplies and one add, the energy term is a
double prefix sum with a fixed association, the NSDF is one double division rounded once to float32, and the peak rule
and the parabola are float32, one IEEE operation at a time.  numpy's element-wise float32 / float64 operations are such
operations, and numpy.cumsum accumulates sequentially, left to right.
"""
import numpy as np

FS = 44100.0
K_CUTOFF = 0.93          # share of the highest peak a chosen peak must reach
SMALL_CUTOFF = 0.5       # peaks at or below this are not interpolated
LOWER_PITCH_CUTOFF = 80.0
RUN = 64                 # samples per run of the energy prefix


def _fft(z, inverse=False):
    from oracle import oracle as o
    return o.fft_c2c(z, inverse=inverse)


def autocorr(x):
    """r[0..N): real part of the unnormalised inverse transform of |FFT_2N(x ++ zeros)|^2"""
    x = np.asarray(x, np.float32)
    n = x.size
    z = np.zeros(2 * n, np.complex64)
    z.real[:n] = x
    z = _fft(z)
    re, im = z.real.copy(), z.imag.copy()
    p = np.zeros(2 * n, np.complex64)
    p.real = re * re + im * im          # float32: two multiplies, one add
    return _fft(p, inverse=True).real[:n].copy()


def prefix(x):
    """P[0..N] in double: P[k] = (totals of the runs of 64 before k, summed in order) + (the samples of k's run before k,
    summed in order)"""
    x = np.asarray(x, np.float32)
    n = x.size
    run = min(RUN, n)
    q = x.astype(np.float64) * x.astype(np.float64)          # exact
    inner = np.cumsum(q.reshape(n // run, run), axis=1)       # inner[r, i] = q[r*run] + ... + q[r*run + i], left to right
    base = np.concatenate([[0.0], np.cumsum(inner[:, -1])])   # base[r] = the totals of runs 0 .. r-1, left to right
    p = np.empty(n + 1, np.float64)
    for r in range(n // run):
        p[r * run] = base[r]
        p[r * run + 1:(r + 1) * run] = base[r] + inner[r, :-1]
    p[n] = base[n // run]
    return p


def nsdf(x):
    x = np.asarray(x, np.float32)
    n = x.size
    r = autocorr(x)
    p = prefix(x)
    tau = np.arange(n)
    m = (p[n - tau] - p[0]) + (p[n] - p[tau])
    a = np.zeros(n, np.float32)
    ok = m > 0
    a[ok] = (r[ok].astype(np.float64) / (float(n) * m[ok])).astype(np.float32)
    return a


def key_maxima(a):
    """indices of the key maxima of an NSDF row, in increasing order"""
    n = a.size
    p = (n - 1) // 3
    nonpos = np.flatnonzero(a <= 0)
    if nonpos.size and nonpos[0] < p:
        p = int(nonpos[0])
    while p < n - 1 and not a[p] > 0:
        p += 1
    keys = []
    best = -1                        # the best candidate of the current run of positive values
    a = a.tolist()                   # (the same values as Python floats: the loop below is a few times faster on them)
    for i in range(p, n - 1):
        if a[i] > 0:
            if i >= 1 and a[i] > a[i - 1] and a[i] >= a[i + 1] and (best < 0 or a[i] > a[best]):
                best = i
        else:
            if best >= 0:
                keys.append(best)
            best = -1
    if best >= 0:
        keys.append(best)
    return keys


def choose(a, fs):
    """(pitch, period, clarity) as float32 from an NSDF row"""
    f32 = np.float32
    hi = f32(0)
    est = []
    for i in key_maxima(a):
        hi = max(hi, a[i])
        if a[i] > f32(SMALL_CUTOFF):
            den = (a[i + 1] + a[i - 1]) - f32(2) * a[i]
            delta = a[i - 1] - a[i + 1]
            if den == 0:
                e = (f32(i), a[i])
            else:
                e = (f32(i) + delta / (f32(2) * den), a[i] - (delta * delta) / (f32(8) * den))
            est.append(e)
            hi = max(hi, e[1])
    if not est:
        return f32(-1), f32(0), f32(0)
    cut = f32(K_CUTOFF * float(hi))
    period, clarity = next(e for e in est if e[1] >= cut)
    pitch = f32(fs) / period
    return (pitch if pitch > f32(LOWER_PITCH_CUTOFF) else f32(-1)), period, clarity


def chunk(x, fs=FS):
    """(pitch, period, clarity, nsdf row) of one chunk"""
    a = nsdf(x)
    return choose(a, fs) + (a,)


def track(x, fs, n, step=None, n_chunks=None):
    """chunks x[c*step : c*step + n]: (pitch, period, clarity) as (n_chunks,) float32 arrays and the NSDF rows (n_chunks, n)"""
    x = np.asarray(x, np.float32)
    step = n if step is None else step
    if n_chunks is None:
        n_chunks = 0 if x.size < n else (x.size - n) // step + 1
    out = [np.empty(n_chunks, np.float32) for _ in range(3)]
    rows = np.empty((n_chunks, n), np.float32)
    for c in range(n_chunks):
        pitch, period, clarity, a = chunk(x[c * step:c * step + n], fs)
        out[0][c], out[1][c], out[2][c], rows[c] = pitch, period, clarity, a
    return out[0], out[1], out[2], rows


# ------------------------------------------------------------------------------------------------ inputs of the tests
def tone(n, fs=FS, f0=163.3, amps=(.30, .22, .15, .08, .05), start=0):
    t = (start + np.arange(n)) / fs
    return sum(a * np.sin(2 * np.pi * f0 * (k + 1) * t) for k, a in enumerate(amps))


def claim_input(amp=3.0, n=14 * 4096, fs=FS):
    """the harmonic tone under drum bursts of DESIGN.md section 13: float32, 14 chunks of 4096"""
    x = tone(n, fs)
    rng = np.random.default_rng(7)
    for s in range(1500, n, 5513):
        if s < n - 1200:
            x[s:s + 1200] += amp * np.exp(-np.arange(1200) / 150.0) * rng.uniform(-1, 1, 1200)
    return x.astype(np.float32)


def edge_inputs(n, fs=FS, seed=0):
    """name -> float32 signal of 5 chunks' length (the callers cut it with their own step)"""
    rng = np.random.default_rng(seed + n)
    length = 5 * (n + 7)
    t = np.arange(length) / fs
    noise = rng.uniform(-1, 1, length)
    sig = {
        "zeros": np.zeros(length),
        "sine60": 0.5 * np.sin(2 * np.pi * 60.0 * t),
        "sine30": 0.5 * np.sin(2 * np.pi * 30.0 * t),
        "sine440": 0.5 * np.sin(2 * np.pi * 440.0 * t),
        "constant": np.full(length, 0.37),
        "square16": np.where(np.arange(length) % 16 < 8, 1.0, -1.0),
        "tone": tone(length, fs),
        "noise": 0.5 * noise,
        "tone+noise": tone(length, fs) + 0.1 * noise,
    }
    return {k: v.astype(np.float32) for k, v in sig.items()}
