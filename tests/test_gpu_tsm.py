"""GPU tier: libzen_hip_tsm.so (zen_amd/tsm) -- time-scale modification on device rows.  Tolerance 0 everywhere: the phases,
the cosine / sine pairs, the magnitudes, owners and synthesis phases of the vocoder and the three kinds of output are compared
bit for bit against tests/tsm_model.py.  Device calls go through run_device below: NaNs around the input rows (a kernel that
read outside the samples of its call would carry them into a result) and sentinels around every output row."""
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
import tsm_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
FS = 8000.0
BAD = 2


@pytest.fixture(scope="module")
def tsm():
    """The library of this feature, built on demand (the session fixture of conftest.py builds the one it links against)."""
    import zen_amd
    from zen_amd import tsm as mod
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


# ================================================================================================ the two table functions alone
def test_cs_device_on_every_table_pair(tsm):
    """all 2^22 pairs (a, b) of table entries, each with random bits below the ten that are cut"""
    import zen_amd
    rng = np.random.default_rng(22)
    psi = (np.arange(1 << 22, dtype=np.uint32) << np.uint32(10)) | rng.integers(0, 1 << 10, 1 << 22, dtype=np.uint32)
    d_in = zen_amd.DeviceBuffer.from_host(np.concatenate([np.zeros(1, np.uint32), psi]))          # off a 16-byte boundary
    d_out = zen_amd.DeviceBuffer.from_host(np.full(2 * psi.size + 3, SENTINEL, np.float32))
    tsm.cs_device(d_in.offset(1), psi.size, d_out.offset(1))
    zen_amd.synchronize()
    got = d_out.download()
    assert got[0] == SENTINEL and np.all(got[-2:] == SENTINEL)
    c, s = M.cs(psi)
    pairs = got[1:-2].reshape(-1, 2)
    assert_same_bits(pairs[:, 0], c, "cos")
    assert_same_bits(pairs[:, 1], s, "sin")
    c2, s2 = tsm.cs(psi[:1000])
    assert_same_bits(c2, c[:1000], "tsm.cs")
    assert_same_bits(s2, s[:1000], "tsm.cs")


def phase_palette():
    """magnitudes: zero, denormals, the smallest normal, 1e-30, 1, 3e38, and on both sides of every boundary (2 i + 1) / 512 at
    which i = rne(256 q) steps -- the boundary itself (a tie for rne) and its two neighbours"""
    edge = ((2.0 * np.arange(257) + 1.0) / 512.0).astype(np.float32)
    near = np.concatenate([np.nextafter(edge, np.float32(0)), edge, np.nextafter(edge, np.float32(2))])
    few = np.array([0.0, 1e-45, 3e-41, 1.1754942e-38, 1.1754944e-38, 1e-30, 0.5, 1.0, 2.0, 3e38], np.float32)
    return np.concatenate([few, near]).astype(np.float32)


def test_phase_device_on_the_palette_and_random_pairs(tsm):
    """the full product of the palette with itself under all four sign pairs (equal magnitudes and -0 among them), 200000
    normal pairs and 200000 pairs of random finite bit patterns"""
    import zen_amd
    rng = np.random.default_rng(7)
    p = phase_palette()
    re, im = (a.ravel() for a in np.meshgrid(p, p))
    one = np.float32(1)
    xs = [np.concatenate([re * sr for sr in (one, one, -one, -one)]), rng.normal(size=200000).astype(np.float32)]
    ys = [np.concatenate([im * si for si in (one, -one, one, -one)]), rng.normal(size=200000).astype(np.float32)]
    raw = rng.integers(0, 1 << 32, 400000, dtype=np.uint64).astype(np.uint32)
    raw = np.where((raw & np.uint32(0x7F800000)) == np.uint32(0x7F800000), raw & np.uint32(0x807FFFFF), raw).view(np.float32)  # finite
    xs.append(raw[:200000])
    ys.append(raw[200000:])
    x, y = np.concatenate(xs), np.concatenate(ys)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(y)) and np.any(np.signbit(x) & (x == 0))
    z = np.full(2 * x.size + 3, np.nan, np.float32)
    z[1:-2:2], z[2:-1:2] = x, y
    d_in = zen_amd.DeviceBuffer.from_host(z)
    d_out = zen_amd.DeviceBuffer.from_host(np.full(x.size + 2, 0xDEADBEEF, np.uint32))
    tsm.phase_device(d_in.offset(1), x.size, d_out.offset(1))
    zen_amd.synchronize()
    got = d_out.download()
    assert got[0] == 0xDEADBEEF and got[-1] == 0xDEADBEEF
    assert_same_bits(got[1:-1], M.atan2turns(y, x), "theta")
    assert_same_bits(tsm.phase(x[:999], y[:999]), M.atan2turns(y[:999], x[:999]), "tsm.phase")


# ================================================================================================ the whole call
def device_rows(x, stride, lead):
    import zen_amd
    C, n = x.shape
    host = np.full(lead + C * stride + 8, np.nan, np.float32)
    for c in range(C):
        host[lead + c * stride:lead + c * stride + n] = x[c]
    return zen_amd.DeviceBuffer.from_host(host), host


def run_device(ts, kind, stems, alpha, lead=(0, 0, 0, 0), pad=(0, 0)):
    """stems: the (n_clips, n) rows the call takes (pv: one; ola: perc, resid or None; hp: harm, perc, resid or None).  `lead`
    floats in front of each input buffer and of the output, `pad` floats between the rows (inputs, output).  Returns the
    (n_clips, n_out) output."""
    import zen_amd
    first = np.asarray(stems[0], np.float32).reshape(ts.n_clips, -1)
    C, n = first.shape
    n_out = int(math.floor(n * alpha))
    in_stride, out_stride = n + pad[0], n_out + pad[1]
    ins = [None if s is None else device_rows(np.asarray(s, np.float32).reshape(C, n), in_stride, lead[i]) for i, s in enumerate(stems)]
    ptrs = [None if b is None else b[0].offset(lead[i]) for i, b in enumerate(ins)]
    ld = lead[3]
    out = zen_amd.DeviceBuffer.from_host(np.full(ld + C * out_stride + 8, SENTINEL, np.float32))
    call = {"pv": ts.pv_device, "ola": ts.ola_device, "hp": ts.hp_device}[kind]
    call(*ptrs, in_stride, n, alpha, out.offset(ld), out_stride)
    zen_amd.synchronize()
    for b in ins:
        assert b is None or np.array_equal(b[0].download(), b[1], equal_nan=True), "an input buffer was written"
    got = out.download()
    assert np.all(got[:ld] == SENTINEL) and np.all(got[ld + C * out_stride:] == SENTINEL)
    rows = got[ld:ld + C * out_stride].reshape(C, out_stride)
    assert np.all(rows[:, n_out:] == SENTINEL), "written beyond the samples of the call"
    return rows[:, :n_out].copy()


def stems_for(kind, rng, C, n):
    if kind == "quantised":
        return [np.stack([M.quantised(rng, n) for _ in range(C)]) for _ in range(3)]
    return [rng.uniform(-1, 1, (C, n)).astype(np.float32) for _ in range(3)]


def whole_case(tsm, N, Np, alpha, n, C, kind, lead, pad, seed):
    """inspect, pv, ola with and without the second row, hp with and without it: everything against the model, clip by clip"""
    rng = np.random.default_rng(seed)
    harm, perc, resid = stems_for(kind, rng, C, n)
    ts = tsm.Tsm(FS, N, Np, n_clips=C, max_samples=n, max_alpha=alpha)
    model = [M.stretch_pv(harm[c], N, alpha, keep=True) for c in range(C)]
    mag, theta, owner, psi = ts.inspect(harm, alpha)
    assert mag.shape == (C, ts.frames(n, alpha), N // 2 + 1)
    for c in range(C):
        what = "clip %d at frame %d alpha %g n %d" % (c, N, alpha, n)
        assert_same_bits(mag[c], model[c].mag, "mag of " + what)
        assert_same_bits(theta[c], model[c].theta, "theta of " + what)
        assert_same_bits(owner[c], model[c].own, "owner of " + what)
        assert_same_bits(psi[c], model[c].psi, "psi of " + what)
        if alpha == 1.0:
            assert np.array_equal(psi[c], theta[c])
    pv = run_device(ts, "pv", [harm], alpha, lead, pad)
    ola1 = run_device(ts, "ola", [perc, None], alpha, lead, pad)
    ola2 = run_device(ts, "ola", [perc, resid], alpha, lead, pad)
    hp1 = run_device(ts, "hp", [harm, perc, None], alpha, lead, pad)
    hp2 = run_device(ts, "hp", [harm, perc, resid], alpha, lead, pad)
    for c in range(C):
        what = " of clip %d at frames %d / %d alpha %g n %d" % (c, N, Np, alpha, n)
        m1, m2 = M.stretch_ola(perc[c], Np, alpha), M.stretch_ola(perc[c], Np, alpha, resid[c])
        assert_same_bits(pv[c], model[c].out, "pv" + what)
        assert_same_bits(ola1[c], m1, "ola" + what)
        assert_same_bits(ola2[c], m2, "ola with the residual" + what)
        assert_same_bits(hp1[c], (model[c].out + m1).astype(np.float32), "hp" + what)
        assert_same_bits(hp2[c], (model[c].out + m2).astype(np.float32), "hp with the residual" + what)
    return ts


ALPHAS = (0.25, 0.77, 1.0, 1.3, 4.0)         # Ha_m = 4 Hs; alternating; Hs; alternating; Hs / 4, the smallest


@pytest.mark.parametrize("alpha", ALPHAS)
def test_frame_64_under_a_wave_on_the_shortest_clips(tsm, oracle, alpha):
    """33 bins; Hs = 16: clips of 1, Hs - 1, Hs, Hs + 1 samples (from 4 on at alpha 0.25, where fewer leave no output)"""
    oracle.lib()
    for n in (1, 15, 16, 17):
        if int(math.floor(n * alpha)) >= 1:
            whole_case(tsm, 64, 16, alpha, n, 1, "random", (1, 2, 3, 1), (0, 0), n)
    whole_case(tsm, 64, 16, alpha, 6001, 1, "quantised", (0, 0, 0, 0), (0, 0), 1)


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("kind", ["random", "quantised"])
def test_frame_256_three_clips_with_padded_and_odd_strides(tsm, oracle, alpha, kind):
    """129 bins: a wave boundary plus one; rows 3 and 5 floats apart from tight, buffers off a 16-byte boundary"""
    oracle.lib()
    whole_case(tsm, 256, 256, alpha, 2003, 3, kind, (1, 2, 3, 1), (3, 5), 2)


@pytest.mark.parametrize("alpha,kind,Np", [(0.77, "random", 256), (1.3, "quantised", 16), (4.0, "random", 256), (1.0, "random", 16)])
def test_frame_2048_more_than_one_item_per_thread_of_the_walk(tsm, oracle, alpha, kind, Np):
    """1025 bins: two bins per thread of the walk, 17 ballot words per frame"""
    oracle.lib()
    whole_case(tsm, 2048, Np, alpha, 6000, 1, kind, (0, 1, 0, 2), (0, 0), 3)


def test_frames_4096_and_8192_take_the_widest_walks(tsm, oracle):
    """2049 and 4097 bins: three and five bins per thread"""
    oracle.lib()
    whole_case(tsm, 4096, 256, 1.3, 5000, 1, "random", (0, 0, 0, 0), (0, 0), 4)
    whole_case(tsm, 8192, 4096, 0.77, 9000, 1, "quantised", (0, 0, 0, 0), (0, 0), 5)


def test_a_silent_clip_and_a_steady_sine(tsm, oracle):
    oracle.lib()
    ts = tsm.Tsm(FS, 256, 32, max_samples=4000, max_alpha=2.0)
    z = np.zeros(3000, np.float32)
    z[7] = -0.0
    assert np.all(bits(run_device(ts, "hp", [z, z, z], 1.7)) == 0), "silence stays +0"
    x = M.sine(4000, 0.0437)
    y = run_device(ts, "pv", [x], 1.5)[0]
    assert_same_bits(y, M.stretch_pv(x, 256, 1.5), "the stretched sine")
    snr, amp = M.sine_snr(y, 0.0437, 512)
    assert snr > 92.476 - 6.0 and abs(amp - 0.5) < 1e-5, (snr, amp)         # the model tests' floor at frame 256


# ================================================================================================ arguments, memory, the program
def test_host_call_equals_device_call_and_later_calls_allocate_nothing(tsm, oracle):
    import zen_amd
    oracle.lib()
    rng = np.random.default_rng(11)
    n, alpha = 3001, 1.3
    harm, perc, resid = stems_for("random", rng, 2, n)
    ts = tsm.Tsm(FS, 256, 32, n_clips=2, max_samples=n + 64, max_alpha=2.0)
    zen_amd.synchronize()
    st0, mc0 = ts.stats(), zen_amd.memcheck()
    assert st0["allocations"] == 11 and st0["calls"] == 0
    want = np.stack([M.stretch_hp(harm[c], perc[c], 256, 32, alpha, resid[c]) for c in range(2)])
    assert_same_bits(ts.hp(harm, perc, alpha, resid), want, "host hp")
    assert_same_bits(run_device(ts, "hp", [harm, perc, resid], alpha), want, "device hp")
    assert_same_bits(ts.pv(harm, alpha), np.stack([M.stretch_pv(harm[c], 256, alpha) for c in range(2)]), "pv through the binding")
    assert_same_bits(ts.ola(perc, alpha), np.stack([M.stretch_ola(perc[c], 32, alpha) for c in range(2)]), "ola through the binding")
    one = tsm.Tsm(FS, 256, 32, max_samples=n, max_alpha=alpha).hp(harm[1], perc[1], alpha)
    assert_same_bits(one, M.stretch_hp(harm[1], perc[1], 256, 32, alpha), "one clip, one dimension")
    ts.profile(True)
    ts.hp(harm, perc, alpha, resid)
    prof = ts.profile_get()
    assert list(prof) == list(tsm.KERNELS)
    for name, p in prof.items():
        assert p["launches"] == 1 and p["ms"] > 0 and p["bytes"] > 0, name
    ts.profile(False)
    zen_amd.synchronize()
    st1, mc1 = ts.stats(), zen_amd.memcheck()
    assert st1["allocations"] == st0["allocations"] and st1["device_bytes"] == st0["device_bytes"]
    assert st1["calls"] == 5 and st1["clips"] == 10
    if mc1["redzone_bytes"]:
        assert mc1["live_allocations"] == mc0["live_allocations"] and mc1["corrupt_words"] == 0


def test_a_session_with_the_defaults_takes_its_longest_clip_length(tsm, oracle):
    """frames 4096 / 256 at up to 4: 524224 samples, the most whose output fits the overlap-add route's 16384 frames"""
    oracle.lib()
    ts = tsm.Tsm(44100.0)
    assert ts.max_samples == 524224 and (ts.nfft, ts.nfft_ola, ts.max_alpha) == (4096, 256, 4.0)
    import zen_amd
    with pytest.raises(zen_amd.ZenHipError) as e:
        tsm.Tsm(44100.0, max_samples=ts.max_samples + 64)
    assert e.value.code == BAD and "16384 frames" in str(e.value)
    x = np.random.default_rng(9).uniform(-1, 1, 3000).astype(np.float32)
    assert_same_bits(ts.hp(x, x[::-1].copy(), 4.0), M.stretch_hp(x, x[::-1], 4096, 256, 4.0), "hp with the defaults")


@pytest.mark.parametrize("with_resid", [True, False])
def test_host_call_on_three_clips_with_padded_host_rows(tsm, oracle, with_resid):
    """zen_hip_tsm_stretch_hp_host itself: the host rows 7 (in) and 5 (out) floats apart from tight, off a 16-byte boundary,
    NaNs between the input rows and sentinels around the output rows -- the copies go row by row"""
    oracle.lib()
    L = tsm.load()
    rng = np.random.default_rng(31)
    C, n, alpha, N, Np = 3, 2003, 1.3, 256, 32
    n_out = int(math.floor(n * alpha))
    in_stride, out_stride = n + 7, n_out + 5
    stems = stems_for("random", rng, C, n)[:3 if with_resid else 2]
    hosts = []
    for k, s in enumerate(stems):
        buf = np.full(1 + k + C * in_stride, np.nan, np.float32)
        buf[1 + k:].reshape(C, in_stride)[:, :n] = s
        hosts.append(buf)
    keep = [b.copy() for b in hosts]
    out = np.full(3 + C * out_stride, SENTINEL, np.float32)
    ts = tsm.Tsm(FS, N, Np, n_clips=C, max_samples=n + 100, max_alpha=2.0)
    ptrs = [b[1 + k:].ctypes.data for k, b in enumerate(hosts)] + [None] * (3 - len(hosts))
    rc = L.zen_hip_tsm_stretch_hp_host(ts._h, ptrs[0], ptrs[1], ptrs[2], in_stride, n, alpha, out[3:].ctypes.data, out_stride)
    assert rc == 0, L.zen_hip_tsm_last_error()
    for b, k in zip(hosts, keep):
        assert np.array_equal(b, k, equal_nan=True), "an input row was written"
    rows = out[3:].reshape(C, out_stride)
    assert np.all(out[:3] == SENTINEL) and np.all(rows[:, n_out:] == SENTINEL), "written outside the output rows"
    for c in range(C):
        want = M.stretch_hp(stems[0][c], stems[1][c], N, Np, alpha, stems[2][c] if with_resid else None)
        assert_same_bits(rows[c, :n_out], want, "host hp of clip %d" % c)
    # padded on one side only
    tight = np.full(C * n_out, SENTINEL, np.float32)
    assert L.zen_hip_tsm_stretch_hp_host(ts._h, ptrs[0], ptrs[1], ptrs[2], in_stride, n, alpha, tight.ctypes.data, n_out) == 0
    assert_same_bits(tight.reshape(C, n_out), rows[:, :n_out].copy(), "tight output rows")


def test_calls_on_a_created_stream(tsm, oracle):
    """set_stream and the stream argument of the two kernels alone: the work is queued on a stream of the caller's and is
    there once that stream is waited for"""
    import ctypes as C

    import zen_amd
    oracle.lib()
    lib = zen_amd.load()
    st = C.c_void_p()
    assert lib.zen_hip_stream_create(C.byref(st)) == 0 and st.value
    ts = None
    try:
        rng = np.random.default_rng(41)
        n, alpha = 2003, 1.3
        n_out = int(math.floor(n * alpha))
        x, p = rng.uniform(-1, 1, (2, n)).astype(np.float32)
        ts = tsm.Tsm(FS, 256, 32, max_samples=n, max_alpha=alpha)
        ts.set_stream(st)
        d_x, d_p = zen_amd.DeviceBuffer.from_host(x), zen_amd.DeviceBuffer.from_host(p)
        out = zen_amd.DeviceBuffer.from_host(np.full(n_out + 2, SENTINEL, np.float32))
        ts.hp_device(d_x, d_p, None, n, n, alpha, out.offset(1), n_out)
        re, im = rng.normal(size=(2, 5000)).astype(np.float32)
        psi = rng.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32)
        d_z, d_psi = zen_amd.DeviceBuffer.from_host(np.stack([re, im], 1)), zen_amd.DeviceBuffer.from_host(psi)
        d_th, d_cs = zen_amd.DeviceBuffer(5000, np.uint32), zen_amd.DeviceBuffer(10000)
        tsm.phase_device(d_z, 5000, d_th, st)
        tsm.cs_device(d_psi, 5000, d_cs, st)
        zen_amd.synchronize(st)
        got = out.download()
        assert got[0] == SENTINEL and got[-1] == SENTINEL
        assert_same_bits(got[1:-1], M.stretch_hp(x, p, 256, 32, alpha), "hp on a created stream")
        assert_same_bits(d_th.download(), M.atan2turns(im, re), "phase on a created stream")
        c, s = M.cs(psi)
        assert_same_bits(d_cs.download().reshape(-1, 2), np.stack([c, s], 1), "cs on a created stream")
        assert_same_bits(ts.hp(x, p, alpha), got[1:-1], "the host call on the same stream")
    finally:
        lib.zen_hip_synchronize(st)
        if ts is not None:
            ts.set_stream(None)             # the handle outlives the stream
        lib.zen_hip_stream_destroy(st)


def test_bad_arguments_are_refused_and_touch_nothing(tsm):
    import zen_amd
    L = tsm.load()
    n = 2000
    ts = tsm.Tsm(FS, 256, 32, max_samples=n, max_alpha=2.0)
    x = np.random.default_rng(0).uniform(-1, 1, n).astype(np.float32)
    inp = zen_amd.DeviceBuffer.from_host(x)
    out = zen_amd.DeviceBuffer.from_host(np.full(4 * n, SENTINEL, np.float32))
    before = ts.stats()
    nan, inf = float("nan"), float("inf")
    cases = [(None, inp.ptr, n, n, 1.5, out.ptr, 2 * n),
             (ts._h, None, n, n, 1.5, out.ptr, 2 * n),
             (ts._h, inp.ptr, n, n, 1.5, None, 2 * n),
             (ts._h, inp.ptr, n - 1, n, 1.5, out.ptr, 2 * n),          # in_stride below the clip
             (ts._h, inp.ptr, n, n, 1.5, out.ptr, 1.5 * n - 1),        # out_stride below the output
             (ts._h, inp.ptr, n, 0, 1.5, out.ptr, 2 * n),              # no samples
             (ts._h, inp.ptr, n + 1, n + 1, 1.5, out.ptr, 2 * n),      # more than max_samples
             (ts._h, inp.ptr, n, n, 2.5, out.ptr, 4 * n),              # more output than create sized
             (ts._h, inp.ptr, n, 3, 0.25, out.ptr, 4 * n),             # no output sample
             (ts._h, inp.ptr + 2, n, n, 1.5, out.ptr, 2 * n),
             (ts._h, inp.ptr, n, n, 1.5, out.ptr + 1, 2 * n)]
    cases += [(ts._h, inp.ptr, n, n, a, out.ptr, 4 * n) for a in (0.2, 4.5, nan, inf, -1.0)]
    for hh, a, in_stride, cnt, alpha, o, out_stride in cases:
        out_stride = int(out_stride)
        assert L.zen_hip_tsm_stretch_pv_device(hh, a, in_stride, cnt, alpha, o, out_stride) == BAD
        assert L.zen_hip_tsm_last_error() != b""
        assert L.zen_hip_tsm_stretch_ola_device(hh, a, a, in_stride, cnt, alpha, o, out_stride) == BAD
        assert L.zen_hip_tsm_stretch_hp_device(hh, a, a, a, in_stride, cnt, alpha, o, out_stride) == BAD
    assert L.zen_hip_tsm_stretch_hp_device(ts._h, inp.ptr, None, None, n, n, 1.5, out.ptr, 2 * n) == BAD
    assert L.zen_hip_tsm_stretch_hp_device(ts._h, inp.ptr, inp.ptr, inp.ptr + 1, n, n, 1.5, out.ptr, 2 * n) == BAD
    assert L.zen_hip_tsm_inspect_device(ts._h, inp.ptr, n, n, 1.5, out.ptr + 2, None, None, None) == BAD
    assert L.zen_hip_tsm_inspect_device(ts._h, inp.ptr, n, n, 1.5, None, None, out.ptr + 1, None) == BAD
    assert L.zen_hip_tsm_inspect_device(ts._h, inp.ptr, n, n, 4.5, None, None, None, None) == BAD
    with pytest.raises(zen_amd.ZenHipError) as e:
        tsm.Tsm(FS, 48)
    assert e.value.code == BAD
    zen_amd.synchronize()
    assert ts.stats() == before
    assert np.all(out.download() == SENTINEL) and np.array_equal(inp.download(), x)
    # the handle is still good, and every output of inspect may be left out
    ts.inspect_device(inp, n, n, 1.5)
    assert ts.pv(x, 2.0).shape == (2 * n,)


def test_stretch_hpr_against_the_model_on_the_oracles_stems(tsm, oracle):
    """3000 samples are padded to 12 hops of 256; the engine's causal block call writes the three stems the oracle's stream
    gives, and hp and pv read them on the device"""
    x = M.sine_and_clicks(3000, every=700, first=333)
    xp = np.zeros(3072, np.float32)
    xp[:3000] = x
    st = oracle.HPR(FS, 256, 2.5, 7, oracle.TIME_CAUSAL).process_stream(xp)
    hp, pv = tsm.stretch_hpr(x, FS, 1.3, hpr_hop=256, beta=2.5, nfft=256, nfft_ola=32)
    assert hp.size == pv.size == int(math.floor(3072 * 1.3))
    assert_same_bits(pv, M.stretch_pv(xp, 256, 1.3), "the vocoder alone")
    assert_same_bits(hp, M.stretch_hp(st["H"], st["P"], 256, 32, 1.3, st["R"]), "hp on the engine's stems")


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


def test_zen_stretch_program_writes_the_models_samples(tsm, oracle, tmp_path):
    from zen_amd.addon_build import tsm as addon
    x = M.sine_and_clicks(3000, every=700, first=333)
    xp = np.zeros(3072, np.float32)
    xp[:3000] = x
    st = oracle.HPR(8000.0, 256, 2.5, 7, oracle.TIME_CAUSAL).process_stream(xp)
    wav, out = str(tmp_path / "clip.wav"), str(tmp_path / "out.wav")
    write_wav_float32(wav, x, 8000)
    args = [addon.build_demo(), wav, "-a", "1.3", "-o", out, "--nfft", "256", "--nfft-ola", "32", "--hpr-hop", "256"]
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "3072 samples in, 3993 out, ratio 1.3\n"
    fs, got = read_wav_pcm16(out)
    assert fs == 8000 and np.array_equal(got, pcm16(M.stretch_hp(st["H"], st["P"], 256, 32, 1.3, st["R"])))
    r = subprocess.run(args + ["--plain"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and r.stdout == "3072 samples in, 3993 out, ratio 1.3, vocoder alone\n"
    assert np.array_equal(read_wav_pcm16(out)[1], pcm16(M.stretch_pv(xp, 256, 1.3)))
    r = subprocess.run(args[:6] + ["--nfft", "48"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 1 and "power of two in 64..8192" in r.stderr


def test_memcheck_is_clean_after_the_module(tsm):
    import zen_amd
    rep = zen_amd.memcheck()
    assert rep["corrupt_words"] == 0 and rep["bounds_violations"] == 0, rep["first_message"]
