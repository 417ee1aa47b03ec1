"""GPU tier: libzen_hip_resample.so (zen_amd/resample) -- band-limited rate conversion of device rows, and the pitch shift on
top of it and the time stretch.  Tolerance 0 everywhere: every output is compared bit for bit against tests/resample_model.py.
Device calls go through run_device below: NaNs around every input window (a kernel that read outside the window of its call
would carry them into a result) and sentinels around every output row."""
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import resample_model as M  # noqa: E402
import tsm_model  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
FS = 8000.0
BAD = 2
RATIOS = [(147, 160), (160, 147), (1, 4), (4, 1), (1048573, 1048575), (61858, 65536), (1, 1)]
TILE = 256


@pytest.fixture(scope="module")
def resample():
    """The library of this feature, built on demand (the session fixture of conftest.py builds the one it links against)."""
    import zen_amd
    from zen_amd import resample as mod
    mod.load()
    zen_amd.init(0)
    return mod


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same_bits(got, want, what):
    g, w = np.asarray(got), np.asarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    diff = np.flatnonzero(bits(g).ravel() != bits(w).ravel())
    assert diff.size == 0, "%s differs from the model in %d places, the first at %d: %r != %r" % (
        what, diff.size, diff[0], g.ravel()[diff[0]], w.ravel()[diff[0]])


def run_device(rs, windows, in_first, n_total, out_first, out_count, lead=(0, 0), pad=(0, 0)):
    """windows: (rows, in_count) float32, the samples from in_first on of every row.  `lead` floats in front of the input and
    of the output buffer, `pad` floats between the rows.  NaNs everywhere around the windows, sentinels around the output
    rows.  Returns the (rows, out_count) outputs."""
    import zen_amd
    windows = np.asarray(windows, np.float32)
    R, cnt = windows.shape
    in_stride, out_stride = cnt + pad[0], out_count + pad[1]
    host = np.full(lead[0] + R * in_stride + 8, np.nan, np.float32)
    for r in range(R):
        host[lead[0] + r * in_stride:lead[0] + r * in_stride + cnt] = windows[r]
    d_in = zen_amd.DeviceBuffer.from_host(host)
    out = zen_amd.DeviceBuffer.from_host(np.full(lead[1] + R * out_stride + 8, SENTINEL, np.float32))
    rs.run_device(d_in.offset(lead[0]), in_stride, in_first, cnt, n_total, out_first, out_count, out.offset(lead[1]), out_stride, R)
    zen_amd.synchronize()
    assert np.array_equal(d_in.download(), host, equal_nan=True), "the input buffer was written"
    got = out.download()
    assert np.all(got[:lead[1]] == SENTINEL) and np.all(got[lead[1] + R * out_stride:] == SENTINEL)
    rows = got[lead[1]:lead[1] + R * out_stride].reshape(R, out_stride)
    assert np.all(rows[:, out_count:] == SENTINEL), "written beyond the outputs of the call"
    return rows[:, :out_count].copy()


def whole(rs, x, lead=(0, 0), pad=(0, 0)):
    x = np.atleast_2d(np.asarray(x, np.float32))
    return run_device(rs, x, 0, x.shape[1], 0, rs.n_out(x.shape[1]), lead, pad)


# ================================================================================================ whole rows
@pytest.mark.parametrize("Z", [8, 16, 32])
@pytest.mark.parametrize("num,den", RATIOS)
def test_whole_rows_of_every_length(resample, num, den, Z):
    """n in {1, 2, W - 1, W, T + 1, 700, 5000}, one row and three, tight and padded rows, buffers on and off a 16-byte boundary"""
    rs = resample.Resampler(num, den, Z)
    W, T = rs.W, rs.T
    assert (W, T) == M.geometry(num, den, Z)[:2]
    for k, n in enumerate((1, 2, W - 1, W, T + 1, 700, 5000)):
        rng = np.random.default_rng(1000 * k + Z)
        R = 3 if k % 2 else 1
        x = rng.uniform(-1, 1, (R, n)).astype(np.float32)
        got = whole(rs, x, lead=(1, 3) if k % 3 else (0, 0), pad=(3, 5) if R == 3 else (0, 0))
        assert got.shape == (R, M.n_out(num, den, n))
        for r in range(R):
            assert_same_bits(got[r], M.resample(x[r], num, den, Z), "row %d of n %d at %d/%d Z %d" % (r, n, num, den, Z))


@pytest.mark.parametrize("num,den,Z", [(147, 160, 16), (4, 1, 8), (1, 4, 32), (61858, 65536, 16)])
def test_tile_edges(resample, num, den, Z):
    """out_count in {TILE - 1, TILE, TILE + 1, 2 TILE + 1}, from the start of the row and from an odd output on"""
    assert resample.TILE == TILE
    rs = resample.Resampler(num, den, Z)
    n = 5000
    x = np.random.default_rng(5).uniform(-1, 1, (2, n)).astype(np.float32)
    want = np.stack([M.resample(x[r], num, den, Z) for r in range(2)])
    for first in (0, 333):
        for count in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
            lo, cnt = rs.span(n, first, count)
            assert (lo, cnt) == M.span(num, den, Z, n, first, count)
            got = run_device(rs, x[:, lo:lo + cnt], lo, n, first, count, lead=(1, 1), pad=(1, 2))
            assert_same_bits(got, want[:, first:first + count], "outputs %d + %d at %d/%d" % (first, count, num, den))


@pytest.mark.parametrize("num,den,Z", [(147, 160, 16), (160, 147, 8), (1, 4, 32), (4, 1, 16), (1048573, 1048575, 8)])
def test_pieces_are_the_whole(resample, num, den, Z):
    """a 5000-sample row cut at random places, single-output pieces among them, each through span"""
    rs = resample.Resampler(num, den, Z)
    rng = np.random.default_rng(17)
    x = rng.uniform(-1, 1, 5000).astype(np.float32)
    want = M.resample(x, num, den, Z)
    inner = [int(v) for v in np.sort(rng.integers(1, want.size, 9))]
    cuts = sorted(set([0, want.size] + inner + [inner[2] + 1, inner[6] + 1]))
    assert any(b - a == 1 for a, b in zip(cuts, cuts[1:]))
    parts = []
    for a, b in zip(cuts, cuts[1:]):
        lo, cnt = rs.span(x.size, a, b - a)
        parts.append(run_device(rs, x[None, lo:lo + cnt], lo, x.size, a, b - a, lead=(a % 4, b % 4))[0])
    assert_same_bits(np.concatenate(parts), want, "the pieces at %d/%d" % (num, den))
    assert_same_bits(rs.pieces(x, cuts), want, "Resampler.pieces")
    # a window wider than the span: the same bits
    first = want.size // 3
    lo, cnt = rs.span(x.size, first, 200)
    wide = run_device(rs, x[None, lo - 3:lo + cnt + 2], lo - 3, x.size, first, 200)[0]
    assert_same_bits(wide, want[first:first + 200], "a wider window")


@pytest.mark.parametrize("num,den,Z", [(1048573, 1048575, 16), (1048575, 524288, 8), (1048575, 262144, 8), (262147, 1048575, 8), (4, 1, 8)])
def test_far_offsets(resample, num, den, Z):
    """n_total = 2^40 and outputs up to the row's end -- near 2^40 with den = 1048575, near 2^41 at a ratio near 2, near 2^42 at a
    ratio near 4: t den reaches 2^60, the most the contract's bounds allow (n_out den <= n_total num + den).  Every 64-bit
    product on a few hundred outputs, from a window of a few hundred samples."""
    assert math.gcd(num, den) == 1
    rs = resample.Resampler(num, den, Z)
    n_total = 1 << 40
    total = M.n_out(num, den, n_total)
    assert total * den >= (1 << 58) or num == 4            # n_total num: 2^58 going down by 4; 4 / 1: the polyphase route near 2^42
    rng = np.random.default_rng(40)
    for first, count in ((total - 300, 300), (total - 70000, 257), (total // 2 + 12345, 300 if num >= den else 64)):
        lo, cnt = rs.span(n_total, first, count)
        assert (lo, cnt) == M.span(num, den, Z, n_total, first, count)
        x = rng.uniform(-1, 1, cnt).astype(np.float32)
        got = run_device(rs, x[None], lo, n_total, first, count, lead=(1, 2))[0]
        assert_same_bits(got, M.resample(x, num, den, Z, first, count, n_total, lo), "outputs %d + %d of 2^40 at %d/%d" % (first, count, num, den))


# ================================================================================================ routes
def test_both_routes_give_the_same_bits(resample, monkeypatch):
    rng = np.random.default_rng(23)
    x = rng.uniform(-1, 1, (2, 3000)).astype(np.float32)
    for num, den, Z in ((147, 160, 16), (160, 147, 32), (1, 4, 8), (4096, 4095, 8), (53, 63, 16)):
        poly = resample.Resampler(num, den, Z)
        monkeypatch.setenv("ZEN_HIP_RESAMPLE", "poly=0")
        interp = resample.Resampler(num, den, Z)
        monkeypatch.delenv("ZEN_HIP_RESAMPLE")
        a, b = whole(poly, x), whole(interp, x)
        assert_same_bits(a, b, "polyphase against interpolating at %d/%d" % (num, den))
        assert_same_bits(a[1], M.resample(x[1], num, den, Z), "polyphase at %d/%d" % (num, den))
        sp, si = poly.stats(), interp.stats()
        assert (sp["poly_calls"], sp["interp_calls"], sp["allocations"]) == (1, 0, 2)
        assert (si["poly_calls"], si["interp_calls"], si["allocations"]) == (0, 1, 1)
        assert sp["device_bytes"] == 4 * (513 + num) * (-(-poly.T // 8) * 8)


def test_the_threshold_between_the_routes(resample):
    """num = 4096 takes the polyphase route and 4097 the interpolating one, read from the stats; both are the model's"""
    x = np.random.default_rng(29).uniform(-1, 1, 2000).astype(np.float32)
    for num, den, poly in ((4096, 4097, True), (4097, 4096, False), (4096, 1025, True), (4097, 16384, False)):
        rs = resample.Resampler(num, den, 8)
        assert resample.geometry(num, den, 8)[2] == (resample.ROUTE_POLY if poly else resample.ROUTE_INTERP)
        assert_same_bits(whole(rs, x)[0], M.resample(x, num, den, 8), "%d/%d" % (num, den))
        st = rs.stats()
        assert (st["poly_calls"], st["interp_calls"]) == ((1, 0) if poly else (0, 1))
        assert st["calls"] == 1 and st["rows"] == 1 and st["outputs"] == M.n_out(num, den, 2000)


# ================================================================================================ sample values
@pytest.mark.parametrize("num,den,Z", [(147, 160, 8), (4, 1, 16), (61858, 65536, 32)])
def test_denormals_signed_zeros_and_large_magnitudes(resample, num, den, Z):
    rng = np.random.default_rng(31)
    n = 1500
    tiny = (rng.integers(1, 1 << 23, n, dtype=np.uint32) | (rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31))).view(np.float32)   # denormals
    small = (rng.uniform(-1, 1, n) * 1e-37).astype(np.float32)           # products and sums fall below the normal range
    zeros = np.where(rng.integers(0, 2, n) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    mixed = rng.uniform(-1, 1, n).astype(np.float32)
    mixed[::3] = -0.0
    mixed[1::7] = tiny[1::7]
    large = (rng.uniform(-1, 1, n) * 1e30).astype(np.float32)
    x = np.stack([tiny, small, zeros, mixed, large])
    rs = resample.Resampler(num, den, Z)
    got = whole(rs, x)
    for r, name in enumerate(("denormals", "tiny values", "signed zeros", "a mixture", "magnitudes up to 1e30")):
        assert_same_bits(got[r], M.resample(x[r], num, den, Z), name)
    assert np.all(bits(got[2]) == 0), "zeros of either sign come out as +0"
    assert np.any((got[0] != 0) & (np.abs(got[0]) < 1.1754944e-38)), "denormal results are kept"


# ================================================================================================ the host call, arguments
def test_host_call_and_later_device_calls_allocate_nothing(resample):
    import zen_amd
    rng = np.random.default_rng(37)
    x = rng.uniform(-1, 1, (3, 2003)).astype(np.float32)
    rs = resample.Resampler(2 * 147, 2 * 160, 16)
    assert (rs.num, rs.den) == (147, 160)
    zen_amd.synchronize()
    st0 = rs.stats()
    assert st0["allocations"] == 2 and st0["calls"] == 0
    first = rs.profile_get()
    assert first["expand"]["launches"] == 1 and first["expand"]["ms"] > 0 and first["fir"]["launches"] == 0
    want = np.stack([M.resample(x[r], 147, 160, 16) for r in range(3)])
    assert_same_bits(rs.run(x), want, "run_host on three rows")
    assert_same_bits(rs.run(x[1]), want[1], "run_host on one row")
    assert_same_bits(resample.convert(x, 48000, 44100), want, "convert")
    # padded host rows, NaNs between them and sentinels around the outputs
    L = resample.load()
    n_out = want.shape[1]
    host = np.full(1 + 3 * 2010, np.nan, np.float32)
    host[1:].reshape(3, 2010)[:, :2003] = x
    out = np.full(3 + 3 * (n_out + 5), SENTINEL, np.float32)
    assert L.zen_hip_resample_run_host(rs._h, host[1:].ctypes.data, 2010, 2003, out[3:].ctypes.data, n_out + 5, 3) == 0
    rows = out[3:].reshape(3, n_out + 5)
    assert np.all(out[:3] == SENTINEL) and np.all(rows[:, n_out:] == SENTINEL)
    assert_same_bits(rows[:, :n_out].copy(), want, "padded host rows")
    rs.profile(True)
    whole(rs, x)
    prof = rs.profile_get()
    assert list(prof) == list(resample.KERNELS) and prof["expand"]["launches"] == 0
    assert prof["fir"]["launches"] == 1 and prof["fir"]["ms"] > 0 and prof["fir"]["bytes"] == 4 * 3 * (2003 + n_out)
    rs.profile(False)
    st1 = rs.stats()
    assert st1["allocations"] == st0["allocations"] and st1["device_bytes"] == st0["device_bytes"]
    assert st1["calls"] == 4 and st1["rows"] == 10 and st1["poly_calls"] == 4


def test_calls_on_a_created_stream(resample):
    import ctypes as C

    import zen_amd
    lib = zen_amd.load()
    st = C.c_void_p()
    assert lib.zen_hip_stream_create(C.byref(st)) == 0 and st.value
    rs = None
    try:
        x = np.random.default_rng(41).uniform(-1, 1, 3001).astype(np.float32)
        rs = resample.Resampler(160, 147, 16)
        rs.set_stream(st)
        n_out = rs.n_out(x.size)
        d_in = zen_amd.DeviceBuffer.from_host(x)
        out = zen_amd.DeviceBuffer.from_host(np.full(n_out + 2, SENTINEL, np.float32))
        rs.run_device(d_in, x.size, 0, x.size, x.size, 0, n_out, out.offset(1), n_out)
        zen_amd.synchronize(st)
        got = out.download()
        assert got[0] == SENTINEL and got[-1] == SENTINEL
        assert_same_bits(got[1:-1], M.resample(x, 160, 147, 16), "on a created stream")
        assert_same_bits(rs.run(x), got[1:-1], "the host call on the same stream")
    finally:
        lib.zen_hip_synchronize(st)
        if rs is not None:
            rs.set_stream(None)
        lib.zen_hip_stream_destroy(st)


def test_bad_arguments_are_refused_and_touch_nothing(resample):
    import zen_amd
    L = resample.load()
    n = 2000
    rs = resample.Resampler(147, 160, 16)
    n_out = rs.n_out(n)
    x = np.random.default_rng(0).uniform(-1, 1, n).astype(np.float32)
    inp = zen_amd.DeviceBuffer.from_host(x)
    out = zen_amd.DeviceBuffer.from_host(np.full(2 * n, SENTINEL, np.float32))
    before = rs.stats()
    h, i, o = rs._h, inp.ptr, out.ptr
    lo, cnt = rs.span(n, 500, 100)
    #        handle in in_stride in_first in_count n_total out_first out_count out out_stride rows
    cases = [(None, i, n, 0, n, n, 0, n_out, o, n_out, 1),
             (h, None, n, 0, n, n, 0, n_out, o, n_out, 1),
             (h, i, n, 0, n, n, 0, n_out, None, n_out, 1),
             (h, i + 2, n, 0, n, n, 0, n_out, o, n_out, 1),              # misaligned
             (h, i, n, 0, n, n, 0, n_out, o + 1, n_out, 1),
             (h, i, n, 0, n, 0, 0, n_out, o, n_out, 1),                  # an empty row
             (h, i, n, 0, n, (1 << 40) + 1, 0, n_out, o, n_out, 1),      # a row too long
             (h, i, n, 0, n, n, 0, 0, o, n_out, 1),                      # no outputs
             (h, i, n, 0, n, n, 0, n_out + 1, o, n_out + 1, 1),          # outputs beyond the row's
             (h, i, n, 0, n, n, n_out, 1, o, 1, 1),
             (h, i, n, 0, n + 1, n, 0, n_out, o, n_out, 1),              # a window beyond the row
             (h, i, n, n, 1, n, 0, n_out, o, n_out, 1),
             (h, i, n, lo + 1, cnt - 1, n, 500, 100, o, 100, 1),         # a window short of the span at its front
             (h, i, n, lo, cnt - 1, n, 500, 100, o, 100, 1),             # and at its end
             (h, i, n, 0, 0, n, 500, 100, o, 100, 1),
             (h, i, cnt - 1, lo, cnt, n, 500, 100, o, 100, 1),           # in_stride below the window
             (h, i, n, 0, n, n, 0, n_out, o, n_out - 1, 1),              # out_stride below the outputs
             (h, i, n, 0, n, n, 0, n_out, o, n_out, 0),                  # no rows
             (h, i, n, 0, n, n, 0, n_out, o, n_out, 65536),
             (h, i, n, 0, n, n, 0, n_out, i, n_out, 1),                  # in place
             (h, i, n, 0, n, n, 0, n_out, i + 4 * (n - 1), n_out, 1),    # the output row begins on the input's last sample
             (h, i + 4 * 100, 100, 0, 100, 100, 0, 10, i, 101, 2)]       # the second output row reaches into the input
    for c in cases:
        assert L.zen_hip_resample_run_device(*c) == BAD, c
        assert L.zen_hip_resample_last_error() != b""
    assert L.zen_hip_resample_run_host(h, x.ctypes.data, n, 0, x.ctypes.data, n, 1) == BAD
    tmp = np.empty(n_out, np.float32)
    assert L.zen_hip_resample_run_host(h, x.ctypes.data, n - 1, n, tmp.ctypes.data, n_out, 2) == BAD
    assert L.zen_hip_resample_run_host(h, x.ctypes.data, n, n, tmp.ctypes.data, n_out - 1, 1) == BAD
    assert L.zen_hip_resample_run_host(h, x.ctypes.data, n, n, None, n_out, 1) == BAD
    with pytest.raises(zen_amd.ZenHipError) as e:
        resample.Resampler(1, 5)
    assert e.value.code == BAD
    zen_amd.synchronize()
    assert rs.stats() == before
    assert np.all(out.download() == SENTINEL) and np.array_equal(inp.download(), x)
    # rows that touch without overlapping are taken, and the handle is still good
    both = zen_amd.DeviceBuffer.from_host(np.concatenate([x, np.full(n_out, SENTINEL, np.float32)]))
    rs.run_device(both, n, 0, n, n, 0, n_out, both.offset(n), n_out)
    zen_amd.synchronize()
    assert_same_bits(both.download()[n:], M.resample(x, 147, 160, 16), "the output right behind the input")


# ================================================================================================ the pitch shift
@pytest.mark.parametrize("s", [3, -5])
def test_shift_on_stems_against_the_models(resample, oracle, s):
    """length 3000, frames 256 / 32: tsm_model.stretch_hp followed by the resample model, padded to 3000, bit for bit"""
    oracle.lib()
    harm, perc = tsm_model.sine(3000, 0.0437, 0.3), tsm_model.clicks(3000, 700, 333)
    resid = (0.01 * np.random.default_rng(s + 50).uniform(-1, 1, 3000)).astype(np.float32)
    num, den, alpha, m, k = M.shift_lengths(3000, s)
    assert resample.shift_plan(3000, s) == (num, den, alpha, m, k) and 2997 <= k <= 3000
    for r in (resid, None):
        stretched = tsm_model.stretch_hp(harm, perc, 256, 32, alpha, r)
        assert stretched.size == m
        got = resample.shift(harm, perc, r, FS, s, nfft=256, nfft_ola=32, quality=16)
        assert got.shape == (3000,)
        assert_same_bits(got, M.shift(stretched, 3000, s, 16), "the shift by %d semitones" % s)
        assert np.all(bits(got[k:]) == 0)


@pytest.mark.parametrize("s", [3, -5, 12])
def test_a_shifted_sine_keeps_its_length_and_moves_its_pitch(resample, oracle, s):
    """a 440 Hz sine at 8 kHz, n = 8000: n samples back, a sine at 440 2^(s / 12) Hz by the model tests' fit"""
    oracle.lib()
    n = 8000
    x = tsm_model.sine(n, 440.0 / FS)
    zero = np.zeros(n, np.float32)
    y = resample.shift(x, zero, None, FS, s, nfft=1024, nfft_ola=64, quality=16)
    assert y.shape == (n,)
    num, den = M.ratio_for_shift(s)
    f_out = 440.0 / FS * den / num
    assert abs(f_out * FS - 440.0 * 2.0 ** (s / 12.0)) < 0.02
    snr, amp = M.sine_fit(y, f_out, 2048)          # two frames of the vocoder at each end, the resampler's own ends within them
    print("shift by %d: %.3f Hz, SNR %.1f dB, amplitude %.4f" % (s, f_out * FS, snr, amp))
    # the vocoder's steady sine at this frame is good to better than 40 dB (tests/test_tsm_model.py's floor is far above);
    # a sine at any other pitch would leave a fit near 0 dB
    assert snr > 40.0 and abs(amp - 0.5) < 0.01, (snr, amp)


def test_shift_hpr_against_the_model_on_the_oracles_stems(resample, oracle):
    """3000 samples are padded to 12 hops of 256; the engine's causal block call writes the three stems the oracle's stream gives"""
    x = tsm_model.sine_and_clicks(3000, every=700, first=333)
    xp = np.zeros(3072, np.float32)
    xp[:3000] = x
    st = oracle.HPR(FS, 256, 2.5, 7, oracle.TIME_CAUSAL).process_stream(xp)
    got = resample.shift_hpr(x, FS, 3, hpr_hop=256, beta=2.5, nfft=256, nfft_ola=32, quality=8)
    alpha = M.shift_lengths(3072, 3)[2]
    want = M.shift(tsm_model.stretch_hp(st["H"], st["P"], 256, 32, alpha, st["R"]), 3072, 3, 8)
    assert_same_bits(got, want, "shift_hpr")


# ================================================================================================ the program
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
    """the program's samples: divided by the largest magnitude where that is above 1, then cli/wav.h: (int16) lroundf(x * 32767.f)"""
    x = x.astype(np.float32)
    peak = np.abs(x).max()
    if peak > 1:
        x = x / np.float32(peak)
    v = (x * np.float32(32767.0)).astype(np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int16)


def test_zen_shift_program_writes_the_bindings_samples(resample, oracle, tmp_path):
    from zen_amd import tsm
    from zen_amd.addon_build import resample as addon
    x = tsm_model.sine_and_clicks(3000, every=700, first=333)
    wav, out = str(tmp_path / "clip.wav"), str(tmp_path / "out.wav")
    write_wav_float32(wav, x, 8000)
    exe = addon.build_demo()
    args = [exe, wav, "-s", "3", "-o", out, "--nfft", "256", "--nfft-ola", "32", "--hpr-hop", "256", "--quality", "8"]
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr
    num, den, alpha, m, k = M.shift_lengths(3072, 3)
    assert r.stdout == "3072 samples in, %d stretched, %d resampled, 3072 out, 3 semitones by %d / %d\n" % (m, k, num, den)
    fs, got = read_wav_pcm16(out)
    assert fs == 8000 and np.array_equal(got, pcm16(resample.shift_hpr(x, FS, 3, hpr_hop=256, beta=2.5, nfft=256, nfft_ola=32, quality=8)))
    r = subprocess.run(args + ["--plain"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.endswith(", vocoder alone\n")
    xp = np.zeros(3072, np.float32)
    xp[:3000] = x
    plain = M.shift(tsm.Tsm(FS, 256, 32, 1, 3072, alpha).pv(xp, alpha), 3072, 3, 8)
    assert np.array_equal(read_wav_pcm16(out)[1], pcm16(plain))
    # the other form: 8000 -> 11025 Hz
    r = subprocess.run([exe, wav, "--rate", "11025", "-o", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr
    want = resample.convert(x, 8000, 11025)
    assert r.stdout == "3000 samples at 8000 Hz in, %d at 11025 Hz out, quality 16\n" % want.size
    fs, got = read_wav_pcm16(out)
    assert fs == 11025 and np.array_equal(got, pcm16(want)) and want.size == M.n_out(441, 320, 3000)
    assert_same_bits(want, M.resample(x, 441, 320, 16), "convert")


def test_memcheck_is_clean_after_the_module(resample):
    import zen_amd
    rep = zen_amd.memcheck()
    assert rep["corrupt_words"] == 0 and rep["bounds_violations"] == 0, rep["first_message"]
