"""GPU tier: libzen_hip_repet.so (zen_amd/repet) -- REPET on device rows.  Tolerance 0 everywhere: the repeating segment, the
beat spectrum, the background and the foreground are compared bit for bit against tests/repet_model.py.  Device calls go
through run_device below: NaNs around the input rows (a kernel that read outside the samples of its call would carry them
into a result) and sentinels around every output row."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import repet_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
FS = M.FAMILY_FS
BAD, UNSUPPORTED = 2, 5
CROSSOVER = 32          # ZEN_HIP_REPET_REGISTER_SEGMENTS: counts above it are sorted in LDS


@pytest.fixture(scope="module")
def repet():
    """The library of this feature, built on demand (the session fixture of conftest.py builds the one it links against)."""
    import zen_amd
    from zen_amd import repet as mod
    mod.load()
    zen_amd.init(0)
    assert mod.REGISTER_SEGMENTS == CROSSOVER
    return mod


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    g, w = np.asarray(got), np.asarray(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    diff = np.flatnonzero(bits(g).ravel() != bits(w).ravel())
    assert diff.size == 0, "%s differs from the model in %d places, the first at %d: %r != %r" % (
        what, diff.size, diff[0], g.ravel()[diff[0]], w.ravel()[diff[0]])


# ================================================================================================ the segment median alone
PALETTE = np.array([0.0, 0.0, 1e-45, 3e-41, 1.1754944e-38, 0.25, 0.5, 1.0, 1.0, 2.0, 3.0, 7.5, 1e30, 3e38], np.float32)
SEGMENTS = (2, 3, 4, 5, 8, 9, 16, 17, CROSSOVER - 1, CROSSOVER, CROSSOVER + 1, 64, 65, 128, 255, 256)


def median_case(repet, rng, m, p, bins, v_stride, s_stride, lead):
    """one launch on a V of m rows quantised to a few levels (ties), with zeros, denormals and large values; `lead` floats in
    front of both buffers move them off a 16-byte boundary"""
    import zen_amd
    V = PALETTE[rng.integers(0, PALETTE.size, (m, bins))]
    v_host = np.full(lead + m * v_stride + 8, np.nan, np.float32)
    for k in range(m):
        v_host[lead + k * v_stride:lead + k * v_stride + bins] = V[k]
    s_host = np.full(lead + p * s_stride + 8, SENTINEL, np.float32)
    v_dev, s_dev = zen_amd.DeviceBuffer.from_host(v_host), zen_amd.DeviceBuffer.from_host(s_host)
    repet.segment_median_device(v_dev.offset(lead), m, bins, v_stride, p, s_dev.offset(lead), s_stride)
    zen_amd.synchronize()
    assert np.array_equal(v_dev.download(), v_host, equal_nan=True), "V was written"
    got = s_dev.download()
    assert np.all(got[:lead] == SENTINEL) and np.all(got[lead + p * s_stride:] == SENTINEL)
    rows = got[lead:lead + p * s_stride].reshape(p, s_stride)
    assert np.all(rows[:, bins:] == SENTINEL), "written beyond the bins of a row"
    assert_same_bits(rows[:, :bins], M.segment_median(V, p), "S at m %d p %d bins %d strides %d %d" % (m, p, bins, v_stride, s_stride))


@pytest.mark.parametrize("bins,v_stride,s_stride,lead", [(33, 33, 33, 0), (33, 40, 36, 0), (129, 129, 129, 1), (129, 136, 132, 0), (129, 136, 132, 2)],
                         ids=["33_tight", "33_padded", "129_tight_off16", "129_padded", "129_padded_off16"])
def test_segment_median_every_count(repet, bins, v_stride, s_stride, lead):
    """r = 2 .. 256 with the last segment whole, one frame long and one frame short, on both sides of the crossover between
    the register networks and the LDS sort; padded strides on 16-byte boundaries take the 16-byte path, the others single words"""
    rng = np.random.default_rng(bins + v_stride + lead)
    for r in SEGMENTS:
        p = 3 if r > 64 else 5
        for rest in (p, 1, p - 1):                      # m mod p = 0, 1, p - 1
            m = (r - 1) * p + rest
            assert M.segments(m, p) == r and m % p == rest % p
            median_case(repet, rng, m, p, bins, v_stride, s_stride, lead)


def test_segment_median_more_than_one_block_and_a_long_period(repet):
    rng = np.random.default_rng(1)
    median_case(repet, rng, 2 * 70 + 1, 70, 1025, 1028, 1028, 0)        # r = 3: 5 blocks of bins, 18 of rows, the 16-byte path with a tail
    median_case(repet, rng, 40 * 7, 7, 300, 301, 300, 0)                # r = 40 in LDS, 5 blocks of bins, the last one ragged
    median_case(repet, rng, 9 * 66 - 1, 66, 70, 72, 72, 0)              # r = 9


def test_segment_median_refuses_one_and_257_segments(repet):
    import zen_amd
    L = repet.load()
    v = zen_amd.DeviceBuffer.from_host(np.ones(257 * 4, np.float32))
    s = zen_amd.DeviceBuffer.from_host(np.full(40, SENTINEL, np.float32))
    assert L.zen_hip_repet_segment_median_device(v.ptr, 10, 4, 4, 10, s.ptr, 4, None) == UNSUPPORTED      # r = 1
    assert L.zen_hip_repet_segment_median_device(v.ptr, 257, 4, 4, 1, s.ptr, 4, None) == UNSUPPORTED      # r = 257
    assert L.zen_hip_repet_segment_median_device(v.ptr, 10, 4, 3, 2, s.ptr, 4, None) == BAD
    assert L.zen_hip_repet_segment_median_device(v.ptr + 2, 10, 4, 4, 2, s.ptr, 4, None) == BAD
    zen_amd.synchronize()
    assert np.all(s.download() == SENTINEL)
    assert L.zen_hip_repet_segment_median_device(v.ptr, 256, 4, 4, 1, s.ptr, 4, None) == 0                # r = 256 is the last one taken
    zen_amd.synchronize()
    assert np.all(s.download()[:4] == 1.0) and np.all(s.download()[4:] == SENTINEL)


# ================================================================================================ the whole call
def run_device(rp, x, periods=None, want=(True, True), lead=(0, 0, 0), pad=(0, 0), braw=False):
    """x: (n_clips, n) rows.  `lead` floats in front of the input / background / foreground rows, `pad` floats between the rows
    (input, outputs).  Returns (background, foreground, periods used[, braw]); None for an output that was not asked for."""
    import zen_amd
    x = np.asarray(x, np.float32).reshape(rp.n_clips, -1)
    C, n = x.shape
    in_stride, out_stride = n + pad[0], n + pad[1]
    in_host = np.full(lead[0] + C * in_stride + 8, np.nan, np.float32)
    for c in range(C):
        in_host[lead[0] + c * in_stride:lead[0] + c * in_stride + n] = x[c]
    inp = zen_amd.DeviceBuffer.from_host(in_host)
    outs = [zen_amd.DeviceBuffer.from_host(np.full(lead[1 + k] + C * out_stride + 8, SENTINEL, np.float32)) for k in range(2)]
    ret = rp.separate_device(inp.offset(lead[0]), in_stride, n, periods, *(outs[k].offset(lead[1 + k]) if want[k] else None for k in range(2)),
                             out_stride=out_stride, braw=braw)
    zen_amd.synchronize()
    assert np.array_equal(inp.download(), in_host, equal_nan=True), "the input buffer was written"
    res = []
    for k in range(2):
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
    return tuple(res) + ((ret[0], ret[1]) if braw else (ret,))


@pytest.fixture(scope="module")
def three(oracle):
    """three clips of the family at N = 256 with periods of 9, 12 and 17 frames, cut to one length that is no multiple of H"""
    oracle.lib()
    n = 13861
    x = np.stack([M.family_clip(0, 256, P, R)[0][:n] for P, R in ((9, 12), (12, 10), (17, 9))])
    assert n % 128 == 37
    model = {hp: [M.separate(x[c], FS, 256, p, highpass=hp) for c, p in enumerate((9, 12, 17))] for hp in (100.0, 0.0)}
    return x, model


@pytest.mark.parametrize("highpass", [100.0, 0.0], ids=["highpass_on", "highpass_off"])
def test_three_clips_with_their_periods_given(repet, three, highpass):
    x, model = three
    assert M.cutoff_bin(FS, 256, 100.0) == 4            # inside the 129 bins
    rp = repet.Repet(FS, 256, n_clips=3, max_samples=x.shape[1] + 100, highpass_hz=highpass)
    bg, fg, used = run_device(rp, x, [9, 12, 17], lead=(1, 2, 3), pad=(3, 5))
    assert used == [9, 12, 17] and rp.stats()["searches"] == 0
    for c in range(3):
        assert_same_bits(bg[c], model[highpass][c].background, "background of clip %d" % c)
        assert_same_bits(fg[c], model[highpass][c].foreground, "foreground of clip %d" % c)
    assert not np.array_equal(bits(model[100.0][0].background), bits(model[0.0][0].background)), "the high-pass is visible"


def test_each_output_on_its_own(repet, three):
    x, model = three
    rp = repet.Repet(FS, 256, n_clips=3, max_samples=x.shape[1])
    bg, none, _ = run_device(rp, x, [9, 12, 17], want=(True, False))
    assert none is None
    none, fg, _ = run_device(rp, x, [9, 12, 17], want=(False, True), lead=(0, 1, 1))
    assert none is None
    for c in range(3):
        assert_same_bits(bg[c], model[100.0][c].background, "background alone, clip %d" % c)
        assert_same_bits(fg[c], model[100.0][c].foreground, "foreground alone, clip %d" % c)
    run_device(rp, x, [9, 12, 17], want=(False, False))


@pytest.mark.parametrize("n", [1, 128])
def test_the_shortest_clips_with_a_period_of_one_frame(repet, oracle, n):
    oracle.lib()
    x = np.random.default_rng(n).uniform(-1, 1, n).astype(np.float32)
    want = M.separate(x, FS, 256, 1)
    bg, fg, used = run_device(repet.Repet(FS, 256, max_samples=128), x, [1], lead=(1, 1, 1))
    assert used == [1] and M.n_frames(n, 128) == 2
    assert_same_bits(bg[0], want.background, "background")
    assert_same_bits(fg[0], want.foreground, "foreground")


@pytest.fixture(scope="module")
def two(oracle):
    """two clips of the family with periods of 12 and 9 frames, one length, and the model with the period found"""
    oracle.lib()
    n = 13861
    x = np.stack([M.family_clip(0, 256, 12, 10)[0][:n], M.family_clip(0, 256, 9, 12)[0]])
    tmin, tmax = M.family_bounds(256)
    return x, (tmin, tmax), [M.separate(r, FS, 256, 0, tmin, tmax) for r in x]


def test_two_clips_whose_period_is_found(repet, two):
    x, (tmin, tmax), model = two
    assert [r.period for r in model] == [12, 9]
    rp = repet.Repet(FS, 256, n_clips=2, max_samples=x.shape[1], tmin_s=tmin, tmax_s=tmax)
    bg, fg, used, braw = run_device(rp, x, None, lead=(3, 0, 1), pad=(1, 2), braw=True)
    assert used == [12, 9] and rp.stats()["searches"] == 2
    for c in range(2):
        assert_same_bits(braw[c], model[c].braw, "braw of clip %d" % c)
        assert_same_bits(bg[c], model[c].background, "background of clip %d" % c)
        assert_same_bits(fg[c], model[c].foreground, "foreground of clip %d" % c)
    given = run_device(rp, x, [12, 9])
    assert_same_bits(given[0], bg, "background with the period given")
    assert_same_bits(given[1], fg, "foreground with the period given")
    # one found, one given: the given clip's beat spectrum row is left alone
    bg2, fg2, used2, braw2 = run_device(rp, x, [0, 9], braw=True)
    assert used2 == [12, 9] and np.all(np.isnan(braw2[1]))
    assert_same_bits(braw2[0], model[0].braw, "braw of clip 0")
    assert_same_bits(bg2, bg, "mixed call")
    # the beat spectrum alone, on the device
    import zen_amd
    m = M.n_frames(x.shape[1], 128)
    out = zen_amd.DeviceBuffer.from_host(np.full(2 * (m + 3) + 1, SENTINEL, np.float32))
    rp.beat_spectrum_device(zen_amd.DeviceBuffer.from_host(x), x.shape[1], x.shape[1], out.offset(1), m + 3)
    zen_amd.synchronize()
    got = out.download()
    rows = got[1:].reshape(2, m + 3)
    assert got[0] == SENTINEL and np.all(rows[:, m:] == SENTINEL)
    assert_same_bits(rows[:, :m], np.stack([r.braw for r in model]), "beat_spectrum_device")


def test_a_silent_clip_has_no_period(repet, oracle):
    oracle.lib()
    x = np.zeros(3000, np.float32)
    x[7] = -0.0
    rp = repet.Repet(FS, 256, max_samples=3000)
    bg, fg, used, braw = run_device(rp, x, None, braw=True, lead=(1, 1, 1))
    assert used == [0] and np.all(bits(braw) == 0)
    assert np.all(bits(bg) == 0), "the background is +0"
    assert_same_bits(fg[0], x, "the foreground is the input")


def test_the_largest_lag_transform(repet, oracle):
    """N = 64 and 8200 frames: L = 32768, the two-step transform; p = 40 gives 205 segments, sorted in LDS"""
    import zen_amd
    oracle.lib()
    n = 8199 * 32 - 5
    x = (0.3 * np.random.default_rng(3).uniform(-1, 1, n)).astype(np.float32)
    m = M.n_frames(n, 32)
    assert m == 8200 and M.lag_points(m) == 32768 and M.segments(m, 40) == 205
    want = M.separate(x, FS, 64, 40, keep=True)
    rp = repet.Repet(FS, 64, max_samples=n)
    bg, fg, used = run_device(rp, x, [40])
    assert_same_bits(bg[0], want.background, "background")
    assert_same_bits(fg[0], want.foreground, "foreground")
    out = zen_amd.DeviceBuffer(m)
    rp.beat_spectrum_device(zen_amd.DeviceBuffer.from_host(x), n, n, out, m)
    zen_amd.synchronize()
    assert_same_bits(out.download(), M.beat_spectrum_raw(want.V), "braw at L = 32768")


# ================================================================================================ arguments, memory, the program
def test_host_call_equals_device_call_and_later_calls_allocate_nothing(repet, two):
    import zen_amd
    x, (tmin, tmax), model = two
    rp = repet.Repet(FS, 256, n_clips=2, max_samples=x.shape[1] + 64, tmin_s=tmin, tmax_s=tmax)
    zen_amd.synchronize()
    st0, mc0 = rp.stats(), zen_amd.memcheck()
    assert st0["allocations"] == 9 and st0["calls"] == 0
    bg, fg, used, braw = rp.run(x, braw=True)
    assert used == [12, 9]
    for c in range(2):
        assert_same_bits(bg[c], model[c].background, "host background")
        assert_same_bits(fg[c], model[c].foreground, "host foreground")
        assert_same_bits(braw[c], model[c].braw, "host braw")
    dev = run_device(rp, x, None)
    assert_same_bits(dev[0], bg, "device against host")
    assert_same_bits(dev[1], fg, "device against host")
    only_bg = rp.run(x[:, :5000], [12, 9], foreground=False)
    assert only_bg[1] is None and only_bg[0].shape == (2, 5000)
    one = repet.Repet(FS, 256, max_samples=x.shape[1]).run(x[1], [9])
    assert_same_bits(one[0], model[1].background, "one clip, one dimension")
    rp.profile(True)
    rp.run(x)
    prof = rp.profile_get()
    assert list(prof) == list(repet.KERNELS)
    for name, p in prof.items():
        assert p["launches"] == {"frame": 1, "fft": 1, "magnitude": 1, "lag_fft": 4}.get(name, 2) and p["ms"] > 0 and p["bytes"] > 0, name
    rp.profile(False)
    zen_amd.synchronize()
    st1, mc1 = rp.stats(), zen_amd.memcheck()
    assert st1["allocations"] == st0["allocations"] and st1["device_bytes"] == st0["device_bytes"]
    assert st1["calls"] == 4 and st1["clips"] == 8 and st1["searches"] == 6
    if mc1["redzone_bytes"]:
        assert mc1["live_allocations"] == mc0["live_allocations"] and mc1["corrupt_words"] == 0


def test_bad_arguments_are_refused_and_touch_nothing(repet):
    import ctypes as C

    import zen_amd
    L = repet.load()
    n = 2000
    rp = repet.Repet(FS, 256, max_samples=n)
    x = np.random.default_rng(0).uniform(-1, 1, n).astype(np.float32)
    inp = zen_amd.DeviceBuffer.from_host(x)
    out = zen_amd.DeviceBuffer.from_host(np.full(2 * n, SENTINEL, np.float32))
    p = (C.c_size_t * 1)(5)
    m = M.n_frames(n, 128)
    before = rp.stats()
    cases = [(None, inp.ptr, n, n, p, n, BAD),
             (rp._h, None, n, n, p, n, BAD),
             (rp._h, inp.ptr, n - 1, n, p, n, BAD),             # in_stride below the clip
             (rp._h, inp.ptr, n, n, p, n - 1, BAD),             # out_stride below the clip
             (rp._h, inp.ptr, n, 0, p, n, BAD),                 # no samples
             (rp._h, inp.ptr, n + 1, n + 1, p, n + 1, BAD),     # more than max_samples
             (rp._h, inp.ptr + 2, n, n, p, n, BAD),
             (rp._h, inp.ptr, n, n, (C.c_size_t * 1)(m), n, UNSUPPORTED),       # one segment
             (rp._h, inp.ptr, n, n, (C.c_size_t * 1)(m + 5), n, UNSUPPORTED)]
    for hh, a, in_stride, cnt, per, out_stride, code in cases:
        for f in (L.zen_hip_repet_separate_device, L.zen_hip_repet_separate_host):
            assert f(hh, a, in_stride, cnt, per, out.ptr, out.offset(n), out_stride, None, None, 0) == code
            assert L.zen_hip_repet_last_error() != b""
    assert L.zen_hip_repet_separate_device(rp._h, inp.ptr, n, n, p, out.ptr + 1, None, n, None, None, 0) == BAD
    assert L.zen_hip_repet_set_params(rp._h, 0.0, 8.0, 100.0) == BAD and L.zen_hip_repet_set_params(rp._h, 2.0, 1.0, 100.0) == BAD
    assert L.zen_hip_repet_set_params(rp._h, 0.8, 8.0, -1.0) == BAD
    with pytest.raises(zen_amd.ZenHipError) as e:
        repet.Repet(FS, 48)
    assert e.value.code == BAD
    zen_amd.synchronize()
    assert rp.stats() == before
    assert np.all(out.download() == SENTINEL) and np.array_equal(inp.download(), x)
    # 257 segments are refused, 256 are taken; the handle is still good
    long = repet.Repet(FS, 64, max_samples=32 * 300)
    y = np.zeros(32 * 256 - 3, np.float32)
    assert M.n_frames(y.size, 32) == 257
    with pytest.raises(zen_amd.ZenHipError) as e:
        long.run(y, [1])
    assert e.value.code == UNSUPPORTED and "257 segments" in str(e.value)
    assert long.run(y[:-32], [1])[2] == [1]
    assert rp.run(x, [5])[0].shape == (n,)


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
    v = (x.astype(np.float32) * np.float32(32767.0)).astype(np.float64)    # cli/wav.h: (int16) lroundf(x * 32767.f)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int16)


def test_zen_repet_program_writes_the_models_stems(repet, oracle, tmp_path):
    """a family clip as an 800 Hz recording: its period of 12 frames is 1.92 s, inside the program's 0.8..8 s"""
    from zen_amd.addon_build import repet as addon
    oracle.lib()
    x = M.family_clip(2, 256, 12, 10)[0]
    want = M.separate(x, 800.0, 256, 0, highpass=10.0)
    assert want.period == 12
    wav, prefix = str(tmp_path / "clip.wav"), str(tmp_path / "out")
    write_wav_float32(wav, x, 800)
    r = subprocess.run([addon.build_demo(), wav, "-o", prefix, "--nfft", "256", "--highpass", "10"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "period: 12 frames, 1.9200 s\n"
    fs, bg = read_wav_pcm16(prefix + "_background.wav")
    assert fs == 800 and np.array_equal(bg, pcm16(want.background))
    assert np.array_equal(read_wav_pcm16(prefix + "_foreground.wav")[1], pcm16(want.foreground))
    given = M.separate(x, 800.0, 256, 12, highpass=10.0)
    r = subprocess.run([addon.build_demo(), wav, "-o", prefix, "--nfft", "256", "--highpass", "10", "--period", "1.92"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and r.stdout == "period: 12 frames, 1.9200 s\n"
    assert np.array_equal(read_wav_pcm16(prefix + "_background.wav")[1], pcm16(given.background))
    r = subprocess.run([addon.build_demo(), wav, "-o", prefix, "--nfft", "64", "--period", "0.04"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True)
    assert r.returncode == 1 and "segments, outside 2..256" in r.stderr       # 483 frames at a period of one: the program says so


def test_memcheck_is_clean_after_the_module(repet):
    import zen_amd
    rep = zen_amd.memcheck()
    assert rep["corrupt_words"] == 0 and rep["bounds_violations"] == 0, rep["first_message"]
