"""GPU tier: libzen_hip_multi.so (zen_amd/multi) -- interleaved multichannel audio through the engines' rows.  Tolerance 0
everywhere: float results are compared bit for bit and int16 results with ==, against the numpy model of tests/multi_model.py
applied to the ORACLE's output for each channel ALONE (44.1 kHz, beta 2)."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import multi_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
FS = 44100.0
NAN_BITS = 0x7fc0beef           # the sentinel of float buffers: a NaN whose payload a stray copy would not reproduce
SENT16 = 12345                  # the sentinel of int16 buffers
GUARD = 16
ZEN = os.path.join(ROOT, "zen_amd", "bin", "zen")


@pytest.fixture(scope="module")
def multi():
    """The library of this feature, built on demand (the session fixture of conftest.py builds the one it links against)."""
    import zen_amd
    from zen_amd import multi as mod
    mod.load()
    zen_amd.init(0)
    return mod


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def audio16(n, channels, seed, level=0.4):
    """[n, channels] int16: noise, a sine of its own per channel and clicks, each channel at its own level"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    cols = []
    for c in range(channels):
        x = level / (1 + c) * rng.uniform(-1, 1, n) + 0.3 * np.sin(2 * np.pi * (440 + 110 * c) * t)
        for s in range(150 + 70 * c, n, 901):
            x[s:s + 20] += 0.25
        cols.append(np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16))
    return np.ascontiguousarray(np.stack(cols, 1))


# ================================================================================================ the kernels alone
def sentinel_like(n, dtype):
    if np.dtype(dtype) == np.int16:
        return np.full(n, SENT16, np.int16)
    return np.full(n, NAN_BITS, np.uint32).view(np.float32)


def is_sentinel(a):
    return np.all(a == SENT16) if a.dtype == np.int16 else np.all(u32(a) == NAN_BITS)


def frames_for(n, ch, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.int16:
        x = rng.integers(-32768, 32768, (n, ch)).astype(np.int16)
        x.ravel()[:4] = np.array([32767, -32768, 0, -1], np.int16)[:x.size]
        return x
    bits = rng.integers(0, 1 << 32, (n, ch), dtype=np.uint64).astype(np.uint32)
    bits.ravel()[:4] = np.array([0x7fa00001, 0xffc12345, 0x80000000, 0x00000001], np.uint32)[:bits.size]   # NaN payloads, -0, a denormal
    return bits.view(np.float32)


def rows_image(rows, stride):
    """one lead element, the rows `stride` apart, GUARD behind: sentinels wherever no row element is"""
    ch, n = rows.shape
    img = sentinel_like(1 + ch * stride + GUARD, np.float32)
    for c in range(ch):
        img[1 + c * stride:1 + c * stride + n] = rows[c]
    return img


def check_rows_image(got, rows, stride):
    ch, n = rows.shape
    mask = np.ones(got.size, bool)
    for c in range(ch):
        seg = slice(1 + c * stride, 1 + c * stride + n)
        assert np.array_equal(u32(got[seg]), u32(rows[c])), "row %d" % c
        mask[seg] = False
    assert is_sentinel(got[mask]), "a sentinel around the rows was overwritten"


KERNEL_LENGTHS = (0, 1, 7, 64, 1003)


@pytest.mark.parametrize("dtype", (np.int16, np.float32), ids=("i16", "f32"))
@pytest.mark.parametrize("ch", (1, 2, 3, 5, 8))
def test_split_kernel_against_the_model(multi, ch, dtype):
    """source and destination one element off a 16-byte boundary, row_stride = n + 5, sentinels everywhere else.  4099 frames
    in addition to the listed lengths: more than one tile for every channel count"""
    import zen_amd
    fmt = multi.I16 if dtype == np.int16 else multi.F32
    before = zen_amd.memcheck()
    for n in KERNEL_LENGTHS + (4099,):
        x = frames_for(n, ch, dtype, 100 + n)
        stride = n + 5
        src_img = np.concatenate([sentinel_like(1, dtype), x.ravel(), sentinel_like(GUARD, dtype)])
        src = zen_amd.DeviceBuffer.from_host(src_img)
        dst = zen_amd.DeviceBuffer.from_host(sentinel_like(1 + ch * stride + GUARD, np.float32))
        assert src.ptr % 16 == 0 and dst.ptr % 16 == 0
        multi.split(fmt, src.offset(1), ch, n, dst.offset(1), stride)
        zen_amd.synchronize()
        check_rows_image(dst.download(), M.split(x), stride)
        assert np.array_equal(src.download().view(np.uint8), src_img.view(np.uint8)), "the source was written"
    after = zen_amd.memcheck()
    assert after["corrupt_words"] == before["corrupt_words"] and after["bounds_violations"] == before["bounds_violations"]


@pytest.mark.parametrize("kind", ("f32", "i16_gain", "i16_peak"))
@pytest.mark.parametrize("ch", (1, 2, 3, 5, 8))
def test_peak_and_join_kernels_against_the_model(multi, ch, kind):
    import zen_amd
    fmt, dtype = (multi.F32, np.float32) if kind == "f32" else (multi.I16, np.int16)
    before = zen_amd.memcheck()
    for n in KERNEL_LENGTHS + (4099,):
        rng = np.random.default_rng(200 + n)
        if kind == "f32":
            rows = np.ascontiguousarray(frames_for(n, ch, np.float32, 300 + n).T)
        else:
            rows = rng.uniform(-3e4, 3e4, (ch, n)).astype(np.float32)
            rows.ravel()[:6] = np.array([0.0, -0.0, np.nan, 0.5, -0.5, 2.5], np.float32)[:rows.size]
            if n >= 64:
                rows[ch - 1, n // 2] = -31000.0            # the peak: in the last channel
        stride = n + 5
        img = rows_image(rows, stride)
        src = zen_amd.DeviceBuffer.from_host(img)
        dst_img = sentinel_like(1 + n * ch + GUARD, dtype)
        dst = zen_amd.DeviceBuffer.from_host(dst_img)
        mm = zen_amd.DeviceBuffer.from_host(np.array([np.inf, -np.inf], np.float32))
        gain = np.float32(2 * 32767.0 / 31000.0)
        if kind == "i16_peak":
            multi.peak(src.offset(1), ch, n, stride, mm)
            multi.join(fmt, src.offset(1), ch, n, stride, dst.offset(1), mode=multi.PEAK, minmax_dev=mm)
            want = M.join(rows, M.I16, M.PEAK)
        elif kind == "i16_gain":
            multi.join(fmt, src.offset(1), ch, n, stride, dst.offset(1), mode=multi.GAIN, gain=float(gain))
            want = M.join(rows, M.I16, M.GAIN, gain)
        else:
            multi.join(fmt, src.offset(1), ch, n, stride, dst.offset(1), mode=multi.PEAK)      # the mode is ignored
            want = M.join(rows, M.F32)
        zen_amd.synchronize()
        got = dst.download()
        assert np.array_equal(got[1:1 + n * ch].view(np.uint8), want.ravel().view(np.uint8)), (n, "samples")
        assert is_sentinel(got[:1]) and is_sentinel(got[1 + n * ch:]), (n, "a sentinel around the frames was overwritten")
        assert np.array_equal(u32(src.download()), u32(img)), "the rows were written"
        if kind == "i16_peak":
            mn, mx = M.minmax(rows)
            assert mm.download().tolist() == [mn, mx], n        # ==: the contract leaves the sign of a zero open
            if n >= 64:
                assert M.peak(rows) == np.float32(31000.0) and want[n // 2, ch - 1] == -32767
    after = zen_amd.memcheck()
    assert after["corrupt_words"] == before["corrupt_words"] and after["bounds_violations"] == before["bounds_violations"]


def test_peak_kernel_accumulates_and_ignores_nans(multi):
    import zen_amd
    rng = np.random.default_rng(5)
    rows = rng.uniform(-1000, 1000, (3, 2500)).astype(np.float32)
    rows[1, ::7] = np.nan
    rows[2, 2499] = 7000.75
    rows[0, 0] = -5000.25
    src = zen_amd.DeviceBuffer.from_host(rows)
    mm = zen_amd.DeviceBuffer.from_host(np.array([np.inf, -np.inf], np.float32))
    for b, e in ((0, 5), (5, 5), (5, 1301), (1301, 2500)):      # pieces of every row, folded in one after the other
        multi.peak(src.offset(b), 3, e - b, 2500, mm)
    zen_amd.synchronize()
    assert mm.download().tolist() == [-5000.25, 7000.75]
    z = zen_amd.DeviceBuffer.from_host(np.zeros((2, 515), np.float32))
    mm = zen_amd.DeviceBuffer.from_host(np.array([np.inf, -np.inf], np.float32))
    out = zen_amd.DeviceBuffer.from_host(np.full(2 * 515, 77, np.int16))
    multi.peak(z, 2, 515, 515, mm)
    multi.join(multi.I16, z, 2, 515, 515, out, mode=multi.PEAK, minmax_dev=mm)
    zen_amd.synchronize()
    assert np.all(mm.download() == 0) and not out.download().any()


# ================================================================================================ offline two-pass
HOPS = (256, 64)                # the pair tests/test_gpu_ragged.py uses
_refs = {}


def offline_reference(oracle, x16, soft=False, sse=False):
    """the oracle's (harm rows, perc rows) [C, n] of the int16 clip x16 [n, C], channel by channel"""
    key = (x16.tobytes(), x16.shape, soft, sse)
    if key not in _refs:
        hs, ps = [], []
        for row in M.split(x16):
            o = oracle.HPRIOffline(FS, HOPS[0], HOPS[1], 2.0, 2.0)
            if sse:
                o.use_sse_filter()
            if soft:
                o.use_soft_mask()
            h, p, r = o.process(row)
            assert not r.any()
            hs.append(h)
            ps.append(p)
        _refs[key] = (np.stack(hs), np.stack(ps))
    return _refs[key]


def make_offline(multi, ch, soft=False, sse=False):
    g = multi.Offline(FS, HOPS[0], HOPS[1], 2.0, 2.0, channels=ch)
    if sse:
        g.use_sse_filter()
    if soft:
        g.use_soft_mask()
    return g


def check_offline(multi, g, x16, rh, rp):
    """float32, int16 PEAK and int16 GAIN through the host call, against the model on the oracle's rows"""
    xf = np.ascontiguousarray(M.split(x16).T)
    out = g.process(xf)
    assert out["harm"].dtype == np.float32 and out["harm"].shape == xf.shape and not g.peaks.any()
    assert np.array_equal(u32(out["harm"]), u32(M.join(rh, M.F32))) and np.array_equal(u32(out["perc"]), u32(M.join(rp, M.F32)))
    out = g.process(x16, mode=multi.PEAK)
    assert out["harm"].dtype == np.int16 and out["harm"].shape == x16.shape
    assert g.peaks.tobytes() == np.array([M.peak(rh), M.peak(rp)], np.float32).tobytes(), (g.peaks, M.peak(rh), M.peak(rp))
    assert np.array_equal(out["harm"], M.join(rh, M.I16, M.PEAK)) and np.array_equal(out["perc"], M.join(rp, M.I16, M.PEAK))
    gain = np.float32(1.7 * 32767.0)
    out = g.process(x16, mode=multi.GAIN, gain=float(gain))
    assert not g.peaks.any()
    assert np.array_equal(out["harm"], M.join(rh, M.I16, M.GAIN, gain)) and np.array_equal(out["perc"], M.join(rp, M.I16, M.GAIN, gain))


@pytest.mark.parametrize("n", (1, 300, 2000))
@pytest.mark.parametrize("ch", (1, 2, 3))
def test_offline_every_channel_equals_the_oracle_on_that_channel_alone(multi, oracle, ch, n):
    x16 = audio16(n, ch, seed=10 * ch + n % 7)
    rh, rp = offline_reference(oracle, x16)
    check_offline(multi, make_offline(multi, ch), x16, rh, rp)
    if ch > 1 and n == 2000:        # the test's own premise: one peak for the stem, and it is not every channel's own
        assert M.peak(rh) == max(M.peak(rh[c:c + 1]) for c in range(ch)) and len({float(M.peak(rh[c:c + 1])) for c in range(ch)}) == ch


@pytest.mark.parametrize("variant", ("soft", "sse"))
def test_offline_soft_mask_and_sse(multi, oracle, variant):
    x16 = audio16(2000, 2, seed=31)
    kw = dict(soft=variant == "soft", sse=variant == "sse")
    rh, rp = offline_reference(oracle, x16, **kw)
    check_offline(multi, make_offline(multi, 2, **kw), x16, rh, rp)


def test_offline_device_call_null_outputs_staging_and_refusals(multi, oracle):
    import zen_amd
    n, ch = 2000, 2
    x16 = audio16(n, ch, seed=41)
    rh, rp = offline_reference(oracle, x16)
    g = make_offline(multi, ch)
    # one output NULL
    out = g.process(x16, want=("perc",))
    assert sorted(out) == ["perc"] and np.array_equal(out["perc"], M.join(rp, M.I16, M.PEAK))
    assert g.peaks.tobytes() == np.array([0, M.peak(rp)], np.float32).tobytes()
    out = g.process(x16, want=("harm",))
    assert np.array_equal(out["harm"], M.join(rh, M.I16, M.PEAK)) and g.peaks[1] == 0
    # a second call of the same size allocates nothing; a smaller one neither; a larger one grows
    both = g.process(x16)
    st = g.stats()
    assert st["row_stride"] == n and st["allocations"] == 3 and st["device_bytes"] == 24 + 3 * ch * n * 4 + 3 * ch * n * 2
    again = g.process(x16)
    assert g.stats()["allocations"] == 3 and g.stats()["calls"] == st["calls"] + 1
    assert np.array_equal(again["harm"], both["harm"]) and np.array_equal(again["perc"], both["perc"])
    g.process(x16[:300])
    assert g.stats()["allocations"] == 3 and g.stats()["row_stride"] == n
    # the device call: same samples as the host call, peaks on the device, sentinels behind the frames untouched
    d_in = zen_amd.DeviceBuffer.from_host(x16)
    d_out = [zen_amd.DeviceBuffer.from_host(np.full(n * ch + GUARD, SENT16, np.int16)) for _ in range(2)]
    d_pk = zen_amd.DeviceBuffer.from_host(np.full(2, -1.0, np.float32))
    g.process_device(multi.I16, d_in, n, harm=d_out[0], perc=d_out[1], mode=multi.PEAK, peaks_dev=d_pk)
    zen_amd.synchronize()
    for d, name in zip(d_out, ("harm", "perc")):
        got = d.download()
        assert np.array_equal(got[:n * ch].reshape(n, ch), both[name]) and np.all(got[n * ch:] == SENT16), name
    assert d_pk.download().tobytes() == np.array([M.peak(rh), M.peak(rp)], np.float32).tobytes()
    assert g.stats()["allocations"] == 3, "the device call uses the rows the host call sized"
    # overlapping buffers are refused and nothing is touched
    big = np.full(3 * n * ch, 77, np.int16)
    big[:n * ch] = x16.ravel()
    keep = big.copy()
    p = lambda a: a.ctypes.data  # noqa: E731
    L = multi.load()
    calls = g.stats()["calls"]
    for harm, perc in ((big[n * ch - 4:], None), (big[n * ch:], big[2 * n * ch - 1:]), (None, big[:8])):
        rc = L.zen_hip_multi_offline_host(g._h, multi.I16, p(big), n, None if harm is None else p(harm), None if perc is None else p(perc),
                                          multi.PEAK, 1.0, None)
        assert rc == zen_amd.lib.E_BAD_ARG and b"overlap" in L.zen_hip_multi_last_error()
    assert np.array_equal(big, keep) and g.stats()["calls"] == calls
    with pytest.raises(zen_amd.ZenHipError) as e:
        g.process_device(multi.I16, d_in, n, harm=d_in.offset(2), mode=multi.GAIN)
    assert e.value.code == zen_amd.lib.E_BAD_ARG and "overlap" in str(e.value)
    assert np.array_equal(d_in.download().reshape(n, ch), x16)
    with pytest.raises(zen_amd.ZenHipError) as e:                       # the two peaks are a buffer like the others
        g.process_device(multi.I16, d_in, n, harm=d_out[0], mode=multi.PEAK, peaks_dev=d_out[0].offset(2))
    assert e.value.code == zen_amd.lib.E_BAD_ARG and "peaks_dev overlaps" in str(e.value)
    d_pk.upload(np.full(2, -1.0, np.float32))
    g.process_device(multi.I16, d_in, 0, harm=d_out[0], perc=d_out[1], mode=multi.PEAK, peaks_dev=d_pk)   # an empty call touches nothing
    zen_amd.synchronize()
    assert d_pk.download().tolist() == [-1.0, -1.0] and np.array_equal(d_out[0].download()[:n * ch].reshape(n, ch), both["harm"])
    # a larger clip grows the staging: two allocations more (the rows and the host call's frames)
    x2 = audio16(2300, ch, seed=43)
    rh2, rp2 = offline_reference(oracle, x2)
    out = g.process(x2)
    assert g.stats()["allocations"] == 5 and g.stats()["row_stride"] == 2300
    assert np.array_equal(out["harm"], M.join(rh2, M.I16, M.PEAK)) and np.array_equal(out["perc"], M.join(rp2, M.I16, M.PEAK))


# ================================================================================================ realtime block
RT_HOP = 128
ALL = 7


def realtime_reference(oracle, x16, soft=False, sse=False):
    """{"harm" | "perc" | "resid": rows [C, n]} of the oracle's causal engine, channel by channel"""
    outs = {"harm": [], "perc": [], "resid": []}
    for row in M.split(x16):
        o = oracle.HPR(FS, RT_HOP, 2.0, ALL, oracle.TIME_CAUSAL)
        if sse:
            o.use_sse_filter()
        if soft:
            o.use_soft_mask()
        r = o.process_stream(row)
        for name, k in (("harm", "H"), ("perc", "P"), ("resid", "R")):
            outs[name].append(r[k])
    return {k: np.stack(v) for k, v in outs.items()}


@pytest.mark.parametrize("ch", (1, 2))
def test_realtime_blocks_however_they_are_cut(multi, oracle, ch):
    n_hops = 40
    x16 = audio16(n_hops * RT_HOP, ch, seed=50 + ch)
    xf = np.ascontiguousarray(M.split(x16).T)
    ref = realtime_reference(oracle, x16)
    gain = np.float32(0.8 * 32767.0)

    def cut(rt, x, hops, **kw):
        parts, at = [], 0
        for h in hops:
            parts.append(rt.process(x[at * RT_HOP:(at + h) * RT_HOP], **kw))
            at += h
        assert at == n_hops
        return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}

    rt = multi.Realtime(FS, RT_HOP, 2.0, ALL, channels=ch, max_hops=64)
    one = cut(rt, xf, (40,))
    for k in ("harm", "perc", "resid"):
        assert one[k].dtype == np.float32 and np.array_equal(u32(one[k]), u32(M.join(ref[k], M.F32))), k
    rt.reset()
    pieces = cut(rt, xf, (1, 5, 34))
    for k in one:
        assert np.array_equal(u32(pieces[k]), u32(one[k])), k
    # _reset followed by a rerun is identical; this time int16 in GAIN mode
    rt.reset()
    one16 = cut(rt, x16, (40,), gain=float(gain))
    rt.reset()
    pieces16 = cut(rt, x16, (1, 5, 34), gain=float(gain))
    for k in one16:
        assert one16[k].dtype == np.int16 and np.array_equal(one16[k], M.join(ref[k], M.I16, M.GAIN, gain)), k
        assert np.array_equal(pieces16[k], one16[k]), k
    # max_hops = 8 forces slices (40 hops: five; 34: five, the last of two hops) and gives the same bits
    sl = multi.Realtime(FS, RT_HOP, 2.0, ALL, channels=ch, max_hops=8)
    sliced = cut(sl, xf, (40,))
    sl.reset()
    sliced2 = cut(sl, x16, (1, 5, 34), gain=float(gain))
    for k in one:
        assert np.array_equal(u32(sliced[k]), u32(one[k])) and np.array_equal(sliced2[k], one16[k]), k


def test_realtime_device_call_output_flags_and_refusals(multi, oracle):
    import zen_amd
    ch, n_hops = 2, 12
    n = n_hops * RT_HOP
    x16 = audio16(n, ch, seed=61)
    ref = realtime_reference(oracle, x16)
    rt = multi.Realtime(FS, RT_HOP, 2.0, zen_amd.OUTPUT_PERCUSSIVE, channels=ch, max_hops=5)
    out = rt.process(x16, gain=32767.0)
    assert sorted(out) == ["perc"] and np.array_equal(out["perc"], M.join(ref["perc"], M.I16, M.GAIN, 32767.0))
    rt.reset()
    d_in = zen_amd.DeviceBuffer.from_host(x16)
    d_p = zen_amd.DeviceBuffer.from_host(np.full(n * ch + GUARD, SENT16, np.int16))
    rt.process_device(multi.I16, d_in, n_hops, perc=d_p, gain=32767.0)
    zen_amd.synchronize()
    got = d_p.download()
    assert np.array_equal(got[:n * ch].reshape(n, ch), out["perc"]) and np.all(got[n * ch:] == SENT16)
    for kw in (dict(harm=d_p), dict(perc=d_in.offset(4))):           # an output without its flag; an output over the input
        with pytest.raises(zen_amd.ZenHipError) as e:
            rt.process_device(multi.I16, d_in, n_hops, gain=1.0, **kw)
        assert e.value.code == zen_amd.lib.E_BAD_ARG
    with pytest.raises(ValueError):
        rt.process(x16[:100])


# ================================================================================================ end to end: zen-stems
def write_wav_pcm16(path, frames, fs=44100):
    frames = np.asarray(frames, dtype="<i2")
    ch = 1 if frames.ndim == 1 else frames.shape[1]
    data = frames.tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, ch, fs, fs * 2 * ch, 2 * ch, 16)
                + b"data" + struct.pack("<I", len(data)) + data)


def read_wav_pcm16(path):
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[8:12] == b"WAVE" and b[12:16] == b"fmt " and b[36:40] == b"data"
    fmt, ch, fs, rate, block, bits = struct.unpack("<HHIIHH", b[20:36])
    assert (fmt, bits, block, rate) == (1, 16, 2 * ch, fs * 2 * ch)
    n = struct.unpack("<I", b[40:44])[0]
    return ch, np.frombuffer(b[44:44 + n], dtype="<i2").astype(np.int16).reshape(-1, ch)


@pytest.fixture(scope="module")
def stems_exe(multi):
    from zen_amd.addon_build import multi as addon
    return addon.build_demo()


E2E = ["--hps", "1024", "2.0", "256", "2.0"]
E2E_N = 20000


def run_stems(exe, wav, prefix, extra=()):
    r = subprocess.run([exe, wav, "-o", prefix] + E2E + list(extra), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return read_wav_pcm16(prefix + "_harm.wav"), read_wav_pcm16(prefix + "_perc.wav")


def run_zen_offline(wav, prefix):
    r = subprocess.run([ZEN, "offline", "-i", wav] + E2E + ["-o", prefix], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return read_wav_pcm16(prefix + "_harm.wav"), read_wav_pcm16(prefix + "_perc.wav")


def test_stems_of_a_stereo_file_with_equal_channels_are_zen_offlines_mono_files(stems_exe, tmp_path):
    """(L + L) / 2 == L exactly: `zen offline` separates L, zen-stems separates L twice, and the joint peak of two equal
    channels is the channel's own"""
    left = audio16(E2E_N, 1, seed=70)[:, 0]
    wav = str(tmp_path / "same.wav")
    write_wav_pcm16(wav, np.stack([left, left], 1))
    (ch_h, sh), (ch_p, sp) = run_stems(stems_exe, wav, str(tmp_path / "st"))
    (_, zh), (_, zp) = run_zen_offline(wav, str(tmp_path / "off"))
    assert ch_h == ch_p == 2 and sh.shape == sp.shape == (E2E_N, 2) and zh.shape == (E2E_N, 1)
    for got, want in ((sh, zh), (sp, zp)):
        assert np.abs(want.astype(np.int32)).max() == 32767 and np.count_nonzero(want) > E2E_N // 2, "the stems are not silent"
        assert np.array_equal(got[:, 0], want[:, 0]) and np.array_equal(got[:, 1], want[:, 0])


def test_stems_of_a_mono_file_are_zen_offlines(stems_exe, tmp_path):
    mono = audio16(E2E_N, 1, seed=71)[:, 0]
    wav = str(tmp_path / "mono.wav")
    write_wav_pcm16(wav, mono)
    (ch_h, sh), (ch_p, sp) = run_stems(stems_exe, wav, str(tmp_path / "st"))
    (_, zh), (_, zp) = run_zen_offline(wav, str(tmp_path / "off"))
    assert ch_h == ch_p == 1 and np.array_equal(sh, zh) and np.array_equal(sp, zp) and np.count_nonzero(sp) > E2E_N // 2


@pytest.mark.parametrize("flags", ((), ("--soft-mask",)), ids=("hard", "soft"))
def test_stems_of_a_stereo_file_are_the_models(stems_exe, oracle, tmp_path, flags):
    x16 = audio16(E2E_N, 2, seed=72)
    wav = str(tmp_path / "lr.wav")
    write_wav_pcm16(wav, x16)
    (ch_h, sh), (ch_p, sp) = run_stems(stems_exe, wav, str(tmp_path / "st"), flags)

    def separate(row):
        o = oracle.HPRIOffline(FS, 1024, 256, 2.0, 2.0)
        if flags:
            o.use_soft_mask()
        h, p, _ = o.process(row)
        return h, p
    want, peaks = M.stems(x16, separate)
    assert ch_h == ch_p == 2 and np.array_equal(sh, want["harm"]) and np.array_equal(sp, want["perc"])
    # the stereo image: only the louder channel reaches full scale, the other keeps its distance
    top = np.abs(sh.astype(np.int32)).max(axis=0)
    assert top.max() == 32767 and top.min() < 32767 and peaks[0] > 0


def test_stems_refuses_nine_channels(stems_exe, tmp_path):
    wav = str(tmp_path / "nine.wav")
    write_wav_pcm16(wav, np.zeros((64, 9), np.int16))
    r = subprocess.run([stems_exe, wav, "-o", str(tmp_path / "st")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "9 channels" in r.stderr and "at most 8" in r.stderr
    assert not os.path.exists(str(tmp_path / "st_harm.wav"))
