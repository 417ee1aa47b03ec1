"""GPU tier: libzen_hip_cqt.so (zen_amd/cqt) -- the sliced constant-Q transform and the separation in its domain.  Tolerance 0
everywhere: coefficients, magnitudes and stems are compared bit for bit against tests/cqt_model.py, no element left out.
Device calls go through run_separate below: NaNs around the input rows (a kernel that read outside the samples of its call
would carry them into a result) and sentinels around every output row."""
import gc
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import cqt_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
TOO_BIG, BAD = 1, 2
# (Ls, B, fmin, fs, n): M at the FFT's minimum with 8 bands; one sample, exactly one hop, one over, several slices; M = 64 far
# below the band positions (the fold wraps many times); B = 1 (a wide top band, M large against Ls, few bands overlapping)
CASES = [(64, 3, 500.0, 8000.0, 100), (256, 4, 300.0, 8000.0, 1), (256, 4, 300.0, 8000.0, 128), (256, 4, 300.0, 8000.0, 129),
         (256, 4, 300.0, 8000.0, 1000), (1024, 12, 60.0, 8000.0, 3000), (256, 1, 300.0, 8000.0, 700)]
THIRD = (1024, 12, 60.0, 8000.0, 3000)


@pytest.fixture(scope="module")
def cqt(oracle):
    """The library of this feature, built on demand (the session fixture of conftest.py builds the one it links against)."""
    import zen_amd
    from zen_amd import cqt as mod
    mod.load()
    zen_amd.init(0)
    oracle.lib()
    return mod


@pytest.fixture(autouse=True)
def nothing_of_this_module_outlives_its_test():
    """A frame that `pytest.raises(...) as e` keeps in a reference cycle holds its session and device buffers until the cycle
    collector runs, at some point of a later test; collected here, every handle and buffer of a test is gone, and the device
    idle, before the next test starts."""
    yield
    import zen_amd
    gc.collect()
    zen_amd.synchronize()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype != np.complex64 else a.view(np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    g, w = np.asarray(got), np.asarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    diff = np.flatnonzero(bits(g).ravel() != bits(w).ravel())
    assert diff.size == 0, "%s differs from the model in %d places, the first at word %d: %r != %r" % (
        what, diff.size, diff[0], bits(g).ravel()[diff[0]], bits(w).ravel()[diff[0]])


def clip(n, seed):
    """a sine, clicks and noise: harmonic, percussive and residual cells all occur"""
    return M.family_clip(n, 8000.0, 440.3, 250, 5.0, seed=seed, noise=0.3)[0]


_models = {}


def model(case, seed, soft=False, lh=0, lp=0):
    """the model's separation of clip(n, seed) at `case`, computed once"""
    key = (case, seed, soft, lh, lp)
    if key not in _models:
        Ls, B, fmin, fs, n = case
        _models[key] = M.separate(clip(n, seed), fs, Ls, B, fmin, soft=soft, lh=lh, lp=lp)
    return _models[key]


def run_separate(cq, x, want=(True, True, True), lead=(0, 0, 0, 0), pad=(0, 0)):
    """x: (n_clips, n) rows.  `lead` floats in front of the input and the three output buffers, `pad` floats between the rows
    (input, outputs).  Returns the three stems, None for one that was not asked for."""
    import zen_amd
    x = np.asarray(x, np.float32).reshape(cq.n_clips, -1)
    C, n = x.shape
    in_stride, out_stride = n + pad[0], n + pad[1]
    in_host = np.full(lead[0] + C * in_stride + 8, np.nan, np.float32)
    for c in range(C):
        in_host[lead[0] + c * in_stride:lead[0] + c * in_stride + n] = x[c]
    inp = zen_amd.DeviceBuffer.from_host(in_host)
    outs = [zen_amd.DeviceBuffer.from_host(np.full(lead[1 + k] + C * out_stride + 8, SENTINEL, np.float32)) for k in range(3)]
    cq.separate_device(inp.offset(lead[0]), in_stride, *(outs[k].offset(lead[1 + k]) if want[k] else None for k in range(3)), out_stride=out_stride)
    zen_amd.synchronize()
    assert np.array_equal(inp.download(), in_host, equal_nan=True), "the input buffer was written"
    res = []
    for k in range(3):
        got = outs[k].download()
        if not want[k]:
            assert np.all(got == SENTINEL)
            res.append(None)
            continue
        ld = lead[1 + k]
        assert np.all(got[:ld] == SENTINEL) and np.all(got[ld + C * out_stride:] == SENTINEL)
        rows = got[ld:ld + C * out_stride].reshape(C, out_stride)
        assert np.all(rows[:, n:] == SENTINEL), "written beyond the samples of the call"
        res.append(rows[:, :n].copy())
    return res


def stems_of(r):
    return (r.harmonic, r.percussive, r.residual)


NAMES = ("harmonic", "percussive", "residual")


# ================================================================================================ every step on every shape
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d_%d_n%d" % (c[0], c[1], c[4]))
def test_forward_spectrogram_and_separation(cqt, case):
    import zen_amd
    Ls, B, fmin, fs, n = case
    x = clip(n, 1)
    hard, soft = model(case, 1), model(case, 1, soft=True)
    pl = hard.pl
    cq = cqt.Cqt(fs, Ls, B, fmin, 1, n)
    sh = cq.shape()
    assert (sh["slices"], sh["bands"], sh["m"], sh["columns"]) == (pl.n_slices(n), pl.nb, pl.M, pl.columns(n))
    assert (sh["lh"], sh["lp"]) == pl.default_lengths(n) == (hard.lh, hard.lp)
    # forward: sentinels behind the coefficients, NaNs around the input
    ns, nb, Mc, T = sh["slices"], pl.nb, pl.M, sh["columns"]
    d_in = zen_amd.DeviceBuffer.from_host(np.concatenate([[np.nan], x, [np.nan] * 3]).astype(np.float32))
    d_c = zen_amd.DeviceBuffer.from_host(np.full(ns * nb * Mc * 2 + 4, SENTINEL, np.float32))
    cq.forward_device(d_in.offset(1), n, d_c)
    zen_amd.synchronize()
    got = d_c.download()
    assert np.all(got[ns * nb * Mc * 2:] == SENTINEL)
    assert_same_bits(got[:ns * nb * Mc * 2].view(np.complex64).reshape(ns, nb, Mc), hard.c, "coefficients")
    # spectrogram: a row stride of nb + 3 and a lead of one float
    vs = nb + 3
    d_v = zen_amd.DeviceBuffer.from_host(np.full(1 + T * vs + 4, SENTINEL, np.float32))
    cq.spectrogram_device(d_in.offset(1), n, d_v.offset(1), vs)
    zen_amd.synchronize()
    got = d_v.download()
    rows = got[1:1 + T * vs].reshape(T, vs)
    assert got[0] == SENTINEL and np.all(got[1 + T * vs:] == SENTINEL) and np.all(rows[:, nb:] == SENTINEL)
    assert_same_bits(rows[:, :nb], hard.V, "V")
    # the three stems, hard then soft
    for k, (g, w) in enumerate(zip(run_separate(cq, x), stems_of(hard))):
        assert_same_bits(g[0], w, "hard " + NAMES[k])
    cq.set_params(soft=True)
    for k, (g, w) in enumerate(zip(run_separate(cq, x, lead=(0, 1, 2, 3)), stems_of(soft))):
        assert_same_bits(g[0], w, "soft " + NAMES[k])
    assert np.all(bits(soft.residual) == 0)
    if n >= 700:
        mk = M.masks(hard.H, hard.P)
        assert all(m.sum() > 0 for m in mk), "the clip exercises all three hard masks"


def test_the_largest_transform(cqt):
    """Ls = 32768: the two-kernel FFT handle on the slices, hundreds of bands, M = 512"""
    case = (32768, 48, 60.0, 44100.0, 2 * 16384 + 5)
    Ls, B, fmin, fs, n = case
    x = M.family_clip(n, fs, 440.3, 5000, 5.0, seed=3, noise=0.3)[0]
    want = M.separate(x, fs, Ls, B, fmin)
    assert want.pl.nb > 300 and want.pl.M == 512 and want.pl.n_slices(n) == 4
    cq = cqt.Cqt(fs, Ls, B, fmin, 1, n)
    assert_same_bits(cq.forward(x), want.c, "coefficients")
    assert_same_bits(cq.spectrogram(x), want.V, "V")
    for k, (g, w) in enumerate(zip(run_separate(cq, x), stems_of(want))):
        assert_same_bits(g[0], w, NAMES[k])


# ================================================================================================ clips, strides, outputs
def test_three_clips_in_one_call_each_equal_the_clip_alone(cqt):
    Ls, B, fmin, fs, n = case = CASES[4]
    x = np.stack([clip(n, s) for s in (1, 2, 3)])
    cq = cqt.Cqt(fs, Ls, B, fmin, 3, n)
    got = run_separate(cq, x, lead=(1, 2, 0, 1), pad=(3, 5))
    for c, seed in enumerate((1, 2, 3)):
        for k, w in enumerate(stems_of(model(case, seed))):
            assert_same_bits(got[k][c], w, "%s of clip %d" % (NAMES[k], c))
    assert_same_bits(cq.forward(x), np.stack([model(case, s).c for s in (1, 2, 3)]), "coefficients of three clips")
    assert_same_bits(cq.spectrogram(x), np.stack([model(case, s).V for s in (1, 2, 3)]), "V of three clips")
    assert not np.array_equal(got[0][0], got[0][1])


@pytest.mark.parametrize("lead,pad", [((0, 0, 0, 0), (0, 0)), ((1, 1, 1, 1), (0, 0)), ((2, 2, 1, 0), (1, 3)), ((0, 0, 0, 0), (4, 4)), ((4, 4, 4, 4), (1, 1))],
                         ids=["aligned", "lead1", "lead2_pad", "pad4", "lead4_pad1"])
def test_padded_strides_and_leads(cqt, lead, pad):
    """two clips: 16-byte aligned rows take the 16-byte stores, a lead of 1 or 2 floats or an odd stride the single words"""
    Ls, B, fmin, fs, n = case = CASES[3]
    x = np.stack([clip(n, 1), clip(n, 2)])
    got = run_separate(cqt.Cqt(fs, Ls, B, fmin, 2, n), x, lead=lead, pad=pad)
    for c, seed in enumerate((1, 2)):
        for k, w in enumerate(stems_of(model(case, seed))):
            assert_same_bits(got[k][c], w, "%s of clip %d" % (NAMES[k], c))


def test_each_output_on_its_own(cqt):
    Ls, B, fmin, fs, n = case = CASES[4]
    x = clip(n, 1)
    cq = cqt.Cqt(fs, Ls, B, fmin, 1, n)
    for k in range(3):
        want = tuple(j == k for j in range(3))
        got = run_separate(cq, x, want=want, lead=(0, 1, 1, 1))
        assert [g is None for g in got] == [not w for w in want]
        assert_same_bits(got[k][0], stems_of(model(case, 1))[k], NAMES[k] + " alone")
    run_separate(cq, x, want=(False, False, False))


def test_inverse_of_forward_is_the_models(cqt):
    import zen_amd
    for case in (CASES[0], CASES[4], THIRD):
        Ls, B, fmin, fs, n = case
        m = model(case, 1)
        want = M.inverse(m.c, m.pl, n)
        cq = cqt.Cqt(fs, Ls, B, fmin, 1, n)
        assert_same_bits(cq.inverse(cq.forward(clip(n, 1))), want, "inverse(forward(x))")
        # a caller's coefficients off an 8-byte boundary, the output off a 16-byte one
        d_c = zen_amd.DeviceBuffer.from_host(np.concatenate([[SENTINEL], m.c.view(np.float32).ravel()]).astype(np.float32))
        d_o = zen_amd.DeviceBuffer.from_host(np.full(n + 6, SENTINEL, np.float32))
        cq.inverse_device(d_c.offset(1), d_o.offset(3), n)
        zen_amd.synchronize()
        got = d_o.download()
        assert np.all(got[:3] == SENTINEL) and np.all(got[3 + n:] == SENTINEL)
        assert_same_bits(got[3:3 + n], want, "inverse from an odd address")


def test_median_lengths_of_the_caller(cqt):
    import zen_amd
    Ls, B, fmin, fs, n = THIRD
    x = clip(n, 1)
    want = model(THIRD, 1, lh=31, lp=7)
    cq = cqt.Cqt(fs, Ls, B, fmin, 1, n, lh=31, lp=7)
    assert (cq.shape()["lh"], cq.shape()["lp"]) == (31, 7)
    for k, (g, w) in enumerate(zip(run_separate(cq, x), stems_of(want))):
        assert_same_bits(g[0], w, NAMES[k] + " at 31 / 7")
    assert not np.array_equal(bits(want.harmonic), bits(model(THIRD, 1).harmonic)), "the lengths are visible"
    # a length above its dimension: refused, the handle keeps 31 / 7 and no output is touched
    L = cqt.load()
    T, nb = cq.columns, cq.n_bands
    assert L.zen_hip_cqt_set_params(cq._h, 2.0, 0, 31, nb + 1) == TOO_BIG and b"bands" in L.zen_hip_cqt_last_error()
    assert L.zen_hip_cqt_set_params(cq._h, 2.0, 0, T + 1, 7) == TOO_BIG and b"columns" in L.zen_hip_cqt_last_error()
    with pytest.raises(zen_amd.ZgException):
        cq.set_params(lp=nb + 1)
    assert L.zen_hip_cqt_set_params(cq._h, 0.5, 0, 0, 0) == BAD and L.zen_hip_cqt_set_params(cq._h, 2.0, 0, -1, 0) == BAD
    assert L.zen_hip_cqt_set_params(cq._h, float("nan"), 0, 0, 0) == BAD
    assert (cq.shape()["lh"], cq.shape()["lp"]) == (31, 7)
    for k, (g, w) in enumerate(zip(run_separate(cq, x), stems_of(want))):
        assert_same_bits(g[0], w, NAMES[k] + " after the refusals")
    # the whole dimension is the longest length taken (T is even: T + 1 taps)
    cq.set_params(lh=T, lp=nb)
    full = M.separate(x, fs, Ls, B, fmin, lh=T, lp=nb)
    for k, (g, w) in enumerate(zip(run_separate(cq, x), stems_of(full))):
        assert_same_bits(g[0], w, NAMES[k] + " at T / nb")


# ================================================================================================ arguments, memory, the program
def test_bad_arguments_are_refused_and_touch_nothing(cqt):
    import zen_amd
    L = cqt.load()
    Ls, B, fmin, fs, n = CASES[4]
    cq = cqt.Cqt(fs, Ls, B, fmin, 2, n)
    x = np.stack([clip(n, 1), clip(n, 2)])
    inp = zen_amd.DeviceBuffer.from_host(x)
    out = zen_amd.DeviceBuffer.from_host(np.full(6 * n + 8, SENTINEL, np.float32))
    o = [out.offset(2 * n * k) for k in range(3)]
    before = cq.stats()
    cases = [(None, inp.ptr, n, o[0], o[1], o[2], n),
             (cq._h, None, n, o[0], o[1], o[2], n),
             (cq._h, inp.ptr, n - 1, o[0], o[1], o[2], n),            # in_stride below the clip
             (cq._h, inp.ptr, n, o[0], o[1], o[2], n - 1),            # out_stride below the clip
             (cq._h, inp.ptr + 2, n, o[0], o[1], o[2], n),            # misaligned input
             (cq._h, inp.ptr, n, o[0] + 1, o[1], o[2], n),
             (cq._h, inp.ptr, n, o[0], o[1] + 2, o[2], n),
             (cq._h, inp.ptr, n, None, None, o[2] + 3, n)]
    for args in cases:
        for f in (L.zen_hip_cqt_separate_device, L.zen_hip_cqt_separate_host):
            assert f(*args) == BAD and L.zen_hip_cqt_last_error() != b""
    assert L.zen_hip_cqt_forward_device(cq._h, inp.ptr, n - 1, o[0]) == BAD and L.zen_hip_cqt_forward_device(cq._h, inp.ptr, n, None) == BAD
    assert L.zen_hip_cqt_forward_device(cq._h, inp.ptr, n, o[0] + 1) == BAD and L.zen_hip_cqt_forward_device(cq._h, None, n, o[0]) == BAD
    assert L.zen_hip_cqt_spectrogram_device(cq._h, inp.ptr, n, o[0], cq.n_bands - 1) == BAD
    assert L.zen_hip_cqt_spectrogram_device(cq._h, inp.ptr, n, None, cq.n_bands) == BAD
    assert L.zen_hip_cqt_inverse_device(cq._h, None, o[0], n) == BAD and L.zen_hip_cqt_inverse_device(cq._h, inp.ptr, None, n) == BAD
    assert L.zen_hip_cqt_inverse_device(cq._h, inp.ptr, o[0], n - 1) == BAD and L.zen_hip_cqt_inverse_device(cq._h, inp.ptr + 1, o[0], n) == BAD
    with pytest.raises(zen_amd.ZenHipError) as e:
        cqt.Cqt(fs, 48, B, fmin, 1, n)
    assert e.value.code == BAD
    zen_amd.synchronize()
    assert cq.stats() == before
    assert np.all(out.download() == SENTINEL) and np.array_equal(inp.download(), x.ravel())
    got = cq.separate(x)                                                # the handle is still good
    assert_same_bits(got[0][1], model(CASES[4], 2).harmonic, "after the refusals")


def test_host_call_equals_device_call_and_later_calls_allocate_nothing(cqt):
    import zen_amd
    Ls, B, fmin, fs, n = case = CASES[4]
    x = np.stack([clip(n, 1), clip(n, 2)])
    cq = cqt.Cqt(fs, Ls, B, fmin, 2, n)
    zen_amd.synchronize()
    st0, mc0 = cq.stats(), zen_amd.memcheck()
    sh = cq.shape()
    ns, nb, Mc, T, N = sh["slices"], sh["bands"], sh["m"], sh["columns"], Ls // 2
    assert sh["run"] == ns
    assert st0["allocations"] == 12 and st0["calls"] == 0
    assert st0["device_bytes"] == 2 * ns * (8 * Ls + 8 * nb * Mc) + 8 * sh["run"] * nb * Mc + 12 * T * nb + 16 * (N + 1) + 8 * Ls \
        + 4 * (N + 1 + nb) + 16 * 2 * n, "the header's formula"
    host = cq.separate(x)
    dev = run_separate(cq, x)
    for k in range(3):
        assert_same_bits(host[k], dev[k], "host against device, " + NAMES[k])
        for c, seed in enumerate((1, 2)):
            assert_same_bits(host[k][c], stems_of(model(case, seed))[k], "host %s of clip %d" % (NAMES[k], c))
    only = cq.separate(x, harmonic=False, residual=False)
    assert only[0] is None and only[2] is None
    assert_same_bits(only[1], host[1], "percussive alone from the host call")
    one = cqt.Cqt(fs, Ls, B, fmin, 1, n).separate(x[1])
    assert one[0].shape == (n,)
    assert_same_bits(one[0], model(case, 2).harmonic, "one clip, one dimension")
    cq.profile(True)
    cq.separate(x)
    prof = cq.profile_get()
    assert list(prof) == list(cqt.KERNELS)
    launches = {"slice": 1, "slice_fft": 1, "fold": 1, "band_ifft": 1, "overlap": 2, "median_time": 2, "median_freq": 2}
    for name, p in prof.items():
        assert p["launches"] == launches.get(name, 6) and p["ms"] > 0 and p["bytes"] > 0, name
    cq.profile(False)
    cq.forward(x)
    cq.spectrogram(x)
    zen_amd.synchronize()
    st1, mc1 = cq.stats(), zen_amd.memcheck()
    assert st1["allocations"] == st0["allocations"] and st1["device_bytes"] == st0["device_bytes"]
    assert st1["calls"] == 6 and st1["clips"] == 8
    if mc1["redzone_bytes"]:
        assert mc1["corrupt_words"] == 0


def test_a_stem_goes_through_runs_of_slices(cqt):
    """Ls = 32768 with B = 1: 11 bands of M = 16384 coefficients, 1.4 MB per slice, so the stem's scratch of 32 MiB holds 23 of
    the clip's 26 slices: two runs, the second of 3.  The largest M and the two-kernel FFT handle as well."""
    Ls, B, fmin, fs, n = 32768, 1, 60.0, 44100.0, 24 * 16384 + 7
    x = M.family_clip(n, fs, 440.3, 30000, 5.0, seed=5, noise=0.3)[0]
    want = M.separate(x, fs, Ls, B, fmin, lh=31, lp=3)
    cq = cqt.Cqt(fs, Ls, B, fmin, 1, n, lh=31, lp=3)
    sh = cq.shape()
    assert (sh["slices"], sh["bands"], sh["m"], sh["run"]) == (26, 11, 16384, 23) == (want.pl.n_slices(n), want.pl.nb, want.pl.M, 23)
    for k, (g, w) in enumerate(zip(run_separate(cq, x), stems_of(want))):
        assert_same_bits(g[0], w, NAMES[k])
    assert_same_bits(cq.inverse(want.c), M.inverse(want.c, want.pl, n), "inverse in two runs")


def write_wav_float32(path, x, fs):
    """mono IEEE-float WAV: the samples reach the program bit for bit"""
    x = np.ascontiguousarray(x, "<f4")
    hdr = b"RIFF" + struct.pack("<I", 36 + x.nbytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 3, 1, fs, fs * 4, 4, 32)
    with open(path, "wb") as f:
        f.write(hdr + b"data" + struct.pack("<I", x.nbytes) + x.tobytes())


def read_wav_pcm16(path):
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[8:12] == b"WAVE" and b[12:16] == b"fmt " and b[36:40] == b"data"
    fmt, ch, fs, _, _, width = struct.unpack("<HHIIHH", b[20:36])
    assert (fmt, ch, width) == (1, 1, 16)
    return fs, np.frombuffer(b[44:44 + struct.unpack("<I", b[40:44])[0]], dtype="<i2")


def pcm16(x):
    """`zen offline`: the stem over its peak (a silent stem as it is), then cli/wav.h: (int16) lroundf(x * 32767.f)"""
    x = x.astype(np.float32)
    peak = max(-x.min(), x.max())
    if peak > 0:
        x = x / np.float32(peak)
    v = (x * np.float32(32767.0)).astype(np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int16)


def test_zen_cqt_program_writes_the_models_stems(cqt, tmp_path):
    from zen_amd.addon_build import cqt as addon
    Ls, B, fmin, fs, n = THIRD
    x = clip(n, 1)
    wav, prefix = str(tmp_path / "clip.wav"), str(tmp_path / "out")
    write_wav_float32(wav, x, int(fs))
    base = [addon.build_demo(), wav, "-o", prefix, "--slice", str(Ls), "--bpo", str(B), "--fmin", "60"]
    for extra, want in (([], model(THIRD, 1)), (["--soft-mask"], model(THIRD, 1, soft=True)), (["--beta", "3"], M.separate(x, fs, Ls, B, fmin, beta=3.0))):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout == "plan: 52 bands, 64 coefficients per band and slice, 500.00 columns per second\n"
        for suffix, stem in zip(("_harm.wav", "_perc.wav", "_residual.wav"), stems_of(want)):
            got_fs, got = read_wav_pcm16(prefix + suffix)
            assert got_fs == int(fs) and np.array_equal(got, pcm16(stem)), (extra, suffix)
    r = subprocess.run(base[:5] + ["48"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 1 and "power of two in 64..32768" in r.stderr


def test_memcheck_is_clean_after_the_module(cqt):
    import zen_amd
    rep = zen_amd.memcheck()
    assert rep["corrupt_words"] == 0 and rep["bounds_violations"] == 0, rep["first_message"]
