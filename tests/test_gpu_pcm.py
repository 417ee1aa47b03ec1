"""GPU tier: libzen_hip_pcm.so (zen_amd/pcm) -- 16-bit PCM host I/O.  Tolerance 0 everywhere: int16 results are compared
with ==, against the numpy model of tests/pcm_model.py applied to the ORACLE's float outputs (and, in PEAK mode, against
the command line tool's own peak_normalise + WAV encoder, compiled here from zen_amd/cli/wav.h)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import pcm_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
FS = 44100.0
H, P, R = 1, 2, 4       # ZEN_HIP_OUTPUT_*
KEYS = (("H", "harm"), ("P", "perc"), ("R", "resid"))


@pytest.fixture(scope="module")
def pcm():
    """The library of this feature, built on demand (the session fixture of conftest.py builds the ones it links against)."""
    import zen_amd
    from zen_amd import pcm as mod
    from zen_amd.addon_build import pcm as addon
    if not os.path.exists(addon.OUT):
        addon.build()
    mod.load()
    zen_amd.init(0)
    yield mod
    mod.release_all()


@pytest.fixture(scope="module")
def cli_encode(tmp_path_factory):
    """peak_normalise (zen_amd/cli/main.cpp:86-92, restated: it is a static function of main.cpp) followed by
    zen::wav::encode_pcm16_mono of zen_amd/cli/wav.h itself; returns the samples of the WAV file it wrote."""
    d = tmp_path_factory.mktemp("cli_encode")
    src, so = str(d / "enc.cpp"), str(d / "enc.so")
    with open(src, "w") as f:
        f.write(r"""
#include <algorithm>
#include "wav.h"
extern "C" int cli_encode(const float* y, size_t n, const char* path)
{
	std::vector<float> x(y, y + n);
	auto limits = std::minmax_element(x.begin(), x.end());
	const float real_max = std::max(-1 * (*limits.first), *limits.second);
	for (std::size_t j = 0; j < n; ++j)
		x[j] /= real_max;
	zen::wav::encode_pcm16_mono(x, 44100, path);
	return 0;
}
""")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "zen_amd", "cli"),
                           src, "-o", so])
    L = C.CDLL(so)

    def run(y):
        y = np.ascontiguousarray(y, np.float32)
        path = str(d / "out.wav")
        L.cli_encode(y.ctypes.data_as(C.c_void_p), C.c_size_t(y.size), path.encode())
        raw = open(path, "rb").read()
        return np.frombuffer(raw[44:44 + 2 * y.size], dtype="<i2").astype(np.int16)
    return run


def audio16(n, seed, channels=1, level=0.5, click=0.9):
    """random int16 audio plus a sine and clicks"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    out = []
    for c in range(channels):
        x = level * rng.uniform(-1, 1, n) + 0.3 * np.sin(2 * np.pi * (440 + 110 * c) * t)
        for s in range(1500 + 700 * c, n, 9001):
            x[s:s + 30] += click
        out.append(np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16))
    return out[0] if channels == 1 else np.stack(out, 1).reshape(-1).copy()


def widen(x16, channels):
    return M.to_float(x16) if channels == 1 else M.stereo_mix(x16)


# ================================================================================================ the kernels alone
LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 4095, 1000003)
GUARD = 16


def offsets():
    """(source offset, destination offset) in samples from a 16-byte boundary: every source offset against a moving
    destination offset, every destination offset against an aligned source"""
    return [(k, (3 * k + 1) % 8) for k in range(8)] + [(0, k) for k in range(8)]


@pytest.mark.parametrize("channels", (1, 2))
def test_to_float_kernel_lengths_and_alignments(pcm, channels):
    import zen_amd
    rng = np.random.default_rng(1)
    nmax = max(LENGTHS)
    src_h = rng.integers(-32768, 32768, (nmax + 8) * channels).astype(np.int16)
    src = zen_amd.DeviceBuffer.from_host(src_h)
    dst = zen_amd.DeviceBuffer(nmax + 8 + 2 * GUARD)
    sentinel = np.full(dst.n, 12345.0, np.float32)
    for n in LENGTHS:
        for so, do in offsets():
            dst.upload(sentinel)
            pcm.to_float(src.offset(so), channels, n, dst.offset(GUARD + do))
            zen_amd.synchronize()
            got = dst.download(n + 2 * GUARD + do)
            want = widen(src_h[so:so + n * channels], channels)
            assert np.array_equal(got[GUARD + do:GUARD + do + n], want), (n, so, do)
            assert np.all(got[:GUARD + do] == 12345.0) and np.all(got[GUARD + do + n:] == 12345.0), (n, so, do)


def test_to_float_kernel_all_65536_values(pcm):
    import zen_amd
    s = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    src, dst = zen_amd.DeviceBuffer.from_host(s), zen_amd.DeviceBuffer(s.size)
    pcm.to_float(src.ptr, 1, s.size, dst.ptr)
    zen_amd.synchronize()
    f = dst.download()
    assert np.array_equal(f, np.float32(s) / np.float32(32767))
    # and back: the round trip is the identity (gain 32767 is the plain encoder)
    back = zen_amd.DeviceBuffer(s.size, np.int16)
    pcm.from_float(dst.ptr, s.size, back.ptr, mode=pcm.GAIN, gain=32767.0)
    zen_amd.synchronize()
    assert np.array_equal(back.download(), s)
    # stereo pairs of extreme values
    lr = np.array([32767, 32767, -32768, -32768, 32767, -32768, -1, 0] * 4, np.int16)
    src2, dst2 = zen_amd.DeviceBuffer.from_host(lr), zen_amd.DeviceBuffer(lr.size // 2)
    pcm.to_float(src2.ptr, 2, lr.size // 2, dst2.ptr)
    zen_amd.synchronize()
    assert np.array_equal(dst2.download(), M.stereo_mix(lr))


def minmax_buffer(zen_amd, pairs=1):
    return zen_amd.DeviceBuffer.from_host(np.array([np.inf, -np.inf] * pairs, np.float32))


@pytest.mark.parametrize("mode", ("peak", "gain"))
def test_from_float_kernel_lengths_and_alignments(pcm, mode):
    import zen_amd
    rng = np.random.default_rng(2)
    nmax = max(LENGTHS)
    y = rng.uniform(-3e4, 3e4, nmax + 8).astype(np.float32)
    y[:16] = [0.0, -0.0, np.nan, np.inf, -np.inf, 3e4, -3e4, 1e-40, 0.5, -0.5, 1.5, 2.5, 29999.5, -29999.5, 7.49999952, 1e9]
    src = zen_amd.DeviceBuffer.from_host(y)
    dst = zen_amd.DeviceBuffer(nmax + 8 + 2 * GUARD, np.int16)
    sentinel = np.full(dst.n, 12345, np.int16)
    mm = zen_amd.DeviceBuffer.from_host(np.array([-20000.0, 31000.0], np.float32))
    gain = np.float32(2 * 32767.0 / 31000.0)
    for n in LENGTHS:
        for do, so in offsets():
            dst.upload(sentinel)
            if mode == "peak":
                pcm.from_float(src.offset(so), n, dst.offset(GUARD + do), mode=pcm.PEAK, minmax_dev=mm.ptr)
                want = M.from_float_peak(y[so:so + n], 31000.0)
            else:
                pcm.from_float(src.offset(so), n, dst.offset(GUARD + do), mode=pcm.GAIN, gain=float(gain))
                want = M.from_float_gain(y[so:so + n], gain)
            zen_amd.synchronize()
            got = dst.download(n + 2 * GUARD + do)
            assert np.array_equal(got[GUARD + do:GUARD + do + n], want), (n, so, do)
            assert np.all(got[:GUARD + do] == 12345) and np.all(got[GUARD + do + n:] == 12345), (n, so, do)


def test_from_float_kernel_half_integer_boundaries(pcm):
    import zen_amd
    k = np.arange(-40000, 40001, dtype=np.float64)
    c = ((k + .5) / 32767.0).astype(np.float32)
    xs = [c]
    lo = hi = c
    for _ in range(2):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        xs += [lo, hi]
    x = np.concatenate(xs + [np.array([0.49999997, -0.49999997, 1.0000305, -1.0000305, 2, -2], np.float32)])
    src, dst = zen_amd.DeviceBuffer.from_host(x), zen_amd.DeviceBuffer(x.size, np.int16)
    pcm.from_float(src.ptr, x.size, dst.ptr, mode=pcm.GAIN, gain=32767.0)
    zen_amd.synchronize()
    assert np.array_equal(dst.download(), M.from_float(x))
    pcm.from_float(src.ptr, x.size, dst.ptr, mode=pcm.GAIN, gain=1.0)      # v = x itself: 0.49999997 must give 0
    zen_amd.synchronize()
    assert np.array_equal(dst.download(), M.from_float_gain(x, 1.0))
    mm = zen_amd.DeviceBuffer.from_host(np.array([-1.0, 0.25], np.float32))
    pcm.from_float(src.ptr, x.size, dst.ptr, mode=pcm.PEAK, minmax_dev=mm.ptr)
    zen_amd.synchronize()
    assert np.array_equal(dst.download(), M.from_float(x))                # peak 1: x / 1 is x


def test_peak_kernel(pcm):
    import zen_amd
    rng = np.random.default_rng(4)
    n = 1000003
    base = rng.uniform(-1000, 1000, n).astype(np.float32)
    cases = {}
    for name, pos in (("first", 0), ("last", n - 1), ("middle", n // 2 + 1)):
        a = base.copy()
        a[pos] = -5000.25
        a[(pos + 777) % n] = 4000.5
        cases["min_" + name] = a
        b = base.copy()
        b[pos] = 7000.75
        cases["max_" + name] = b
    cases["all_negative"] = -np.abs(base) - 1
    cases["all_positive"] = np.abs(base) + 1
    cases["short"] = base[:7]
    cases["one"] = base[:1]
    for name, a in cases.items():
        for off in (0, 1, 3):
            if off >= a.size:
                continue
            src, mm = zen_amd.DeviceBuffer.from_host(a), minmax_buffer(zen_amd)
            pcm.peak(src.offset(off), a.size - off, mm.ptr)
            zen_amd.synchronize()
            got = mm.download()
            assert got[0] == np.min(a[off:]) and got[1] == np.max(a[off:]), (name, off, got)
    # NaNs are ignored
    a = base[:5000].copy()
    a[::7] = np.nan
    src, mm = zen_amd.DeviceBuffer.from_host(a), minmax_buffer(zen_amd)
    pcm.peak(src.ptr, a.size, mm.ptr)
    zen_amd.synchronize()
    assert mm.download().tolist() == [np.nanmin(a), np.nanmax(a)]
    # accumulation over several calls, and n == 0 leaves the words alone
    mm = minmax_buffer(zen_amd)
    src = zen_amd.DeviceBuffer.from_host(base)
    cuts = (0, 5, 4101, 4101, 500000, n)
    for b, e in zip(cuts[:-1], cuts[1:]):
        pcm.peak(src.offset(b), e - b, mm.ptr)
    zen_amd.synchronize()
    assert mm.download().tolist() == [np.min(base), np.max(base)]
    # all zeros: peak 0, PEAK output zeros
    z = zen_amd.DeviceBuffer.from_host(np.zeros(4099, np.float32))
    mm = minmax_buffer(zen_amd)
    pcm.peak(z.ptr, 4099, mm.ptr)
    out = zen_amd.DeviceBuffer.from_host(np.full(4099, 77, np.int16))
    pcm.from_float(z.ptr, 4099, out.ptr, mode=pcm.PEAK, minmax_dev=mm.ptr)
    zen_amd.synchronize()
    assert np.all(mm.download() == 0) and not out.download().any()


def test_kernel_entry_points_refuse_bad_arguments(pcm):
    import zen_amd
    d = zen_amd.DeviceBuffer(64)
    for call in (lambda: pcm.to_float(d.ptr, 3, 8, d.ptr), lambda: pcm.to_float(None, 1, 8, d.ptr),
                 lambda: pcm.from_float(d.ptr, 8, d.ptr, mode=7), lambda: pcm.from_float(d.ptr, 8, d.ptr, mode=pcm.PEAK, minmax_dev=None),
                 lambda: pcm.to_float(d.ptr + 1, 1, 8, d.ptr), lambda: pcm.peak(d.ptr, 8, None)):
        with pytest.raises(zen_amd.ZenHipError) as e:
            call()
        assert e.value.code == zen_amd.lib.E_BAD_ARG and "pcm_" in str(e.value)


# ================================================================================================ realtime block engine
RT_CONFIGS = {
    "hop1024_perc": dict(hop=1024, flags=P, n_hops=24),
    "hop256_all": dict(hop=256, flags=H | P | R, n_hops=60),
    "hop512_sse": dict(hop=512, flags=H | P | R, n_hops=40, sse=True),
    "hop1024_soft": dict(hop=1024, flags=H | P | R, n_hops=24, soft=True),
    "hop512_stereo": dict(hop=512, flags=H | P, n_hops=30, channels=2),
}


def make_engines(oracle, cfg):
    import zen_amd
    g = zen_amd.HPR(FS, cfg["hop"], 2.0, cfg["flags"], zen_amd.TIME_CAUSAL)
    o = oracle.HPR(FS, cfg["hop"], 2.0, cfg["flags"], oracle.TIME_CAUSAL)
    for e in (g, o):
        if cfg.get("sse"):
            e.use_sse_filter()
        if cfg.get("soft"):
            e.use_soft_mask()
    return g, o


def rt_case(oracle, cfg, seed=0, level=0.5):
    ch = cfg.get("channels", 1)
    x16 = audio16(cfg["hop"] * cfg["n_hops"], seed, ch, level)
    g, o = make_engines(oracle, cfg)
    ref = o.process_stream(widen(x16, ch))
    wanted = [(k, name) for (k, name), bit in zip(KEYS, (H, P, R)) if cfg["flags"] & bit]
    return g, x16, ch, ref, wanted


def run_pcm(pcm, g, x16, ch, wanted, **kw):
    n = x16.size // ch
    outs = {name: np.full(n, 12345, np.int16) for _, name in wanted}
    peaks = pcm.hpr_process_host(g, x16, channels=ch, **outs, **kw)
    return outs, peaks


@pytest.mark.parametrize("name", sorted(RT_CONFIGS))
@pytest.mark.parametrize("pieces", ("one_piece", "ragged_pieces"))
def test_realtime_block_against_the_oracle(pcm, oracle, cli_encode, name, pieces):
    cfg = RT_CONFIGS[name]
    g, x16, ch, ref, wanted = rt_case(oracle, cfg)
    piece_hops = 0 if pieces == "one_piece" else 7          # 24 / 60 / 40 / 30 hops: several pieces, the last one shorter
    assert pieces == "one_piece" or cfg["n_hops"] % 7 != 0
    try:
        outs, peaks = run_pcm(pcm, g, x16, ch, wanted, mode=pcm.PEAK, piece_hops=piece_hops)
        assert pcm.host_stats()["n_pieces"] == (1 if pieces == "one_piece" else -(-cfg["n_hops"] // 7))
        for i, (k, nm) in enumerate(KEYS):
            if (k, nm) not in wanted:
                assert peaks[i] == 0
                continue
            pk = M.peak_of(ref[k])
            assert peaks[i].tobytes() == pk.tobytes(), (k, peaks[i], pk)
            assert np.array_equal(outs[nm], M.from_float_peak(ref[k], pk)), k
            if pk != 0:      # (an all-zero output -- the residual of the SSE and soft-mask paths: the tool divides 0 by 0, PEAK writes zeros)
                assert np.array_equal(outs[nm], cli_encode(ref[k])), k    # what peak_normalise + the WAV encoder write
            else:
                assert not outs[nm].any() and not ref[k].any(), k
        # GAIN on the same engine type, fresh state
        g.reset_buffers()
        for k, nm in wanted:
            pk = M.peak_of(ref[k])
            gain = np.float32(0.9 * 32767.0) / pk if pk != 0 else np.float32(1.0)
            o2, none = run_pcm(pcm, g, x16, ch, [(k, nm)], mode=pcm.GAIN, gain=float(gain), piece_hops=piece_hops)
            assert none is None and np.array_equal(o2[nm], M.from_float_gain(ref[k], gain)), k
            g.reset_buffers()
    finally:
        pcm.release(g)


@pytest.mark.parametrize("piece_hops, n_pieces", ((1, 9), (1000, 1)), ids=("every_piece_one_hop", "piece_longer_than_the_block"))
def test_realtime_piece_size_edges(pcm, oracle, piece_hops, n_pieces):
    """the two ends of the piece rule on a block of 9 hops: as many pieces as hops, and a piece clamped to the block; both
    give the model's samples, so the same samples as each other"""
    cfg = dict(RT_CONFIGS["hop256_all"], n_hops=9)
    g, x16, ch, ref, wanted = rt_case(oracle, cfg, seed=3)
    try:
        outs, peaks = run_pcm(pcm, g, x16, ch, wanted, mode=pcm.PEAK, piece_hops=piece_hops)
        st = pcm.host_stats()
        assert st["n_pieces"] == n_pieces and st["piece_frames"] == 9 * 256 // n_pieces
        for i, (k, nm) in enumerate(KEYS):
            pk = M.peak_of(ref[k])
            assert peaks[i].tobytes() == pk.tobytes(), (k, peaks[i], pk)
            assert np.array_equal(outs[nm], M.from_float_peak(ref[k], pk)), k
        g.reset_buffers()
        outs, none = run_pcm(pcm, g, x16, ch, wanted, mode=pcm.GAIN, gain=1.5, piece_hops=piece_hops)
        st = pcm.host_stats()
        assert none is None and st["n_pieces"] == n_pieces and st["piece_frames"] == 9 * 256 // n_pieces
        for k, nm in wanted:
            assert np.array_equal(outs[nm], M.from_float_gain(ref[k], 1.5)), k
    finally:
        pcm.release(g)


def test_realtime_two_calls_equal_one_call_and_float_path(pcm, oracle):
    import zen_amd
    cfg = RT_CONFIGS["hop256_all"]
    g, x16, ch, ref, wanted = rt_case(oracle, cfg, seed=5)
    g2, _ = make_engines(oracle, cfg)
    g3, _ = make_engines(oracle, cfg)
    gain = 1.5
    try:
        whole, _ = run_pcm(pcm, g, x16, ch, wanted, mode=pcm.GAIN, gain=gain)
        cut = 23 * cfg["hop"]
        a, _ = run_pcm(pcm, g2, x16[:cut].copy(), ch, wanted, mode=pcm.GAIN, gain=gain, piece_hops=5)
        b, _ = run_pcm(pcm, g2, x16[cut:].copy(), ch, wanted, mode=pcm.GAIN, gain=gain)
        for k, nm in wanted:
            assert np.array_equal(np.concatenate([a[nm], b[nm]]), whole[nm]), k
            assert np.array_equal(whole[nm], M.from_float_gain(ref[k], gain)), k
        # the float call of the same engine type followed by the model; then a PCM call continues that engine's state
        xf = widen(x16, ch)
        fo = {nm: np.zeros(cut, np.float32) for _, nm in wanted}
        g3.process_host(xf[:cut].copy(), **fo)
        for k, nm in wanted:
            assert np.array_equal(M.from_float_gain(fo[nm], gain), a[nm]), k
        b3, _ = run_pcm(pcm, g3, x16[cut:].copy(), ch, wanted, mode=pcm.GAIN, gain=gain)
        for k, nm in wanted:
            assert np.array_equal(b3[nm], b[nm]), k
    finally:
        for e in (g, g2, g3):
            pcm.release(e)


def test_realtime_pinned_and_pageable_buffers(pcm, oracle):
    cfg = RT_CONFIGS["hop1024_perc"]
    g, x16, ch, ref, wanted = rt_case(oracle, cfg, seed=9)
    pin_in, pin_out = pcm.PinnedPCM(x16.size), pcm.PinnedPCM(x16.size)
    try:
        pin_in.array[:] = x16
        pk = pcm.hpr_process_host(g, pin_in.array, perc=pin_out.array, mode=pcm.PEAK, piece_hops=5)
        st = pcm.host_stats()
        assert st["input_pinned"] and st["outputs_pinned"] and st["n_pieces"] == 5
        want = M.from_float_peak(ref["P"], M.peak_of(ref["P"]))
        assert np.array_equal(pin_out.array, want) and pk[1] == M.peak_of(ref["P"])
        g.reset_buffers()
        out = np.zeros(x16.size, np.int16)
        pcm.hpr_process_host(g, x16, perc=out, mode=pcm.PEAK, piece_hops=5)      # pageable: registered for the call
        assert np.array_equal(out, want)
        g.reset_buffers()
        pcm.hpr_process_host(g, x16, perc=pin_out.array, mode=pcm.GAIN, gain=2.0)   # mixed
        assert np.array_equal(pin_out.array, M.from_float_gain(ref["P"], 2.0))
    finally:
        pcm.release(g)
        pin_in.free()
        pin_out.free()


def test_realtime_saturation_in_gain_mode(pcm, oracle):
    cfg = dict(hop=1024, flags=H | P | R, n_hops=24)
    g, x16, ch, ref, wanted = rt_case(oracle, cfg, seed=13, level=1.0)     # full-scale noise
    try:
        for k, nm in wanted:
            gain = np.float32(2 * 32767.0) / M.peak_of(ref[k])
            want = M.from_float_gain(ref[k], gain)
            # an error of the test, not a pass, if the case does not clip on both sides and leave samples unclipped
            assert (want == 32767).any() and (want == -32768).any() and (np.abs(want.astype(np.int32)) < 32767).any(), k
            unclipped = np.abs(ref[k].astype(np.float64) * np.float64(gain)) < 32767
            assert unclipped.any() and (~unclipped).any()
            out, _ = run_pcm(pcm, g, x16, ch, [(k, nm)], mode=pcm.GAIN, gain=float(gain), piece_hops=9)
            assert np.array_equal(out[nm], want), k
            g.reset_buffers()
    finally:
        pcm.release(g)


def test_realtime_refusals_leave_the_engine_untouched(pcm, oracle):
    import zen_amd
    cfg = RT_CONFIGS["hop256_all"]
    g, x16, ch, ref, wanted = rt_case(oracle, cfg, seed=21)
    n = x16.size
    cut = 20 * cfg["hop"]
    lib = pcm.load()
    o = {nm: np.zeros(n, np.int16) for _, nm in wanted}
    big = np.zeros(2 * n, np.int16)
    multi = zen_amd.HPR(FS, 256, 2.0, P, zen_amd.TIME_CAUSAL, True, 2, 0)
    try:
        first, _ = run_pcm(pcm, g, x16[:cut].copy(), ch, wanted, mode=pcm.GAIN, gain=1.25)
        bad = [
            lambda: pcm.hpr_process_host(g, big[:n], perc=big[n - 8:2 * n - 8], mode=pcm.GAIN),                  # input / output
            lambda: pcm.hpr_process_host(g, x16, harm=big[:n], perc=big[n - 1:2 * n - 1], mode=pcm.GAIN),        # output / output
            lambda: pcm.hpr_process_host(g, x16, harm=o["harm"], resid=o["harm"], mode=pcm.PEAK),
            lambda: pcm._ck(lib.zen_hip_pcm_hpr_process_host(g._h, x16.ctypes.data, 3, 4, o["perc"].ctypes.data, None, None, 0, 1.0, None, 0)),
            lambda: pcm._ck(lib.zen_hip_pcm_hpr_process_host(g._h, x16.ctypes.data, 0, 4, o["perc"].ctypes.data, None, None, 0, 1.0, None, 0)),
            lambda: pcm._ck(lib.zen_hip_pcm_hpr_process_host(g._h, None, 1, 4, None, o["perc"].ctypes.data, None, 0, 1.0, None, 0)),
            lambda: pcm._ck(lib.zen_hip_pcm_hpr_process_host(g._h, x16.ctypes.data, 1, 4, None, o["perc"].ctypes.data, None, 5, 1.0, None, 0)),
            lambda: pcm.hpr_process_host(multi, x16[:512].copy(), perc=o["perc"][:512], mode=pcm.GAIN),
        ]
        for i, call in enumerate(bad):
            with pytest.raises(zen_amd.ZenHipError) as e:
                call()
            assert e.value.code == zen_amd.lib.E_BAD_ARG and len(str(e.value)) > 30, i
        # the engine's state is where the first call left it
        rest, _ = run_pcm(pcm, g, x16[cut:].copy(), ch, wanted, mode=pcm.GAIN, gain=1.25)
        for k, nm in wanted:
            assert np.array_equal(np.concatenate([first[nm], rest[nm]]), M.from_float_gain(ref[k], 1.25)), k
    finally:
        pcm.release(g)
        pcm.release(multi)


def test_engine_stays_on_the_context_stream_and_release_puts_it_back(pcm, oracle):
    """the header's stream contract: float calls after a PCM call still work (on the context's stream), and after
    release the engine works on the null stream again"""
    cfg = RT_CONFIGS["hop1024_perc"]
    g, x16, ch, ref, wanted = rt_case(oracle, cfg, seed=31)
    xf = widen(x16, ch)
    cut = 10 * 1024
    a = np.zeros(cut, np.int16)
    pcm.hpr_process_host(g, x16[:cut].copy(), perc=a, mode=pcm.GAIN, gain=1.0)
    mid = np.zeros(4 * 1024, np.float32)
    g.process_host(xf[cut:cut + 4096].copy(), perc=mid)
    pcm.release(g)
    pcm.release(g)                                           # unknown handle by now: fine
    end = np.zeros(xf.size - cut - 4096, np.float32)
    g.process_host(xf[cut + 4096:].copy(), perc=end)
    assert np.array_equal(a, M.from_float_gain(ref["P"][:cut], 1.0))
    assert np.array_equal(np.concatenate([mid, end]), ref["P"][cut:])


# ================================================================================================ offline two-pass engine
def offline_case(oracle, n, seed, channels=1, soft=False, hops=(1024, 256), loud_at=None):
    import zen_amd
    x16 = audio16(n, seed, channels, level=0.2, click=0.2)
    if loud_at is not None:                                  # the clip's loudest event
        x16 = x16.copy()
        v = x16.reshape(n, channels)                         # a loud tone for the harmonic output, a click in it for the percussive
        v[loud_at:loud_at + 5000] = (0.95 * 32767 * np.sin(2 * np.pi * 1000 * np.arange(5000) / FS)).astype(np.int16)[:, None]
        v[loud_at + 2500:loud_at + 2540] = 32767
    g = zen_amd.HPRIOffline(FS, hops[0], hops[1], 2.0, 2.0)
    o = oracle.HPRIOffline(FS, hops[0], hops[1], 2.0, 2.0)
    if soft:
        g.use_soft_mask()
        o.use_soft_mask()
    rh, rp, rr = o.process(widen(x16, channels))
    assert not rr.any()
    return g, x16, rh, rp


@pytest.mark.parametrize("soft", (False, True), ids=("hard", "soft"))
@pytest.mark.parametrize("channels", (1, 2), ids=("mono", "stereo"))
def test_offline_short_clip(pcm, oracle, cli_encode, soft, channels):
    n = 30011
    g, x16, rh, rp = offline_case(oracle, n, 40 + channels, channels, soft)
    hh, pp, rr = (np.full(n, 12345, np.int16) for _ in range(3))
    try:
        pk = pcm.hpri_process(g, x16, channels=channels, harm=hh, perc=pp, resid=rr, mode=pcm.PEAK)
        assert pcm.host_stats()["n_pieces"] == 1
        assert pk.tobytes() == np.array([M.peak_of(rh), M.peak_of(rp), 0], np.float32).tobytes()
        assert np.array_equal(hh, M.from_float_peak(rh, pk[0])) and np.array_equal(pp, M.from_float_peak(rp, pk[1]))
        assert np.array_equal(hh, cli_encode(rh)) and np.array_equal(pp, cli_encode(rp))     # what `zen offline` writes
        assert not rr.any()
        # GAIN, NULL outputs
        gain = np.float32(2 * 32767.0) / M.peak_of(rp)
        pp2, rr2 = np.full(n, 12345, np.int16), np.full(n, 12345, np.int16)
        assert pcm.hpri_process(g, x16, channels=channels, perc=pp2, resid=rr2, mode=pcm.GAIN, gain=float(gain)) is None
        want = M.from_float_gain(rp, gain)
        assert (want == 32767).any() and (want == -32768).any() and (np.abs(want.astype(np.int32)) < 32767).any()
        assert np.array_equal(pp2, want) and not rr2.any()
        hh2 = np.full(n, 12345, np.int16)
        pcm.hpri_process(g, x16, channels=channels, harm=hh2, mode=pcm.GAIN, gain=0.5)
        assert np.array_equal(hh2, M.from_float_gain(rh, 0.5))
    finally:
        pcm.release(g)


@pytest.mark.parametrize("soft", (False, True), ids=("hard", "soft"))
def test_offline_clip_of_several_ranges(pcm, oracle, soft):
    """>= 3 ranges, the last one ragged, the clip's loudest event in the last range: the peak is the whole clip's"""
    range_samples = 32768
    n = 3 * range_samples + 9001
    g, x16, rh, rp = offline_case(oracle, n, 50, 2 if soft else 1, soft, loud_at=3 * range_samples + 2000)
    ch = 2 if soft else 1
    hh, pp, rr = (np.full(n, 12345, np.int16) for _ in range(3))
    try:
        pk = pcm.hpri_process(g, x16, channels=ch, harm=hh, perc=pp, resid=rr, mode=pcm.PEAK, range_samples=range_samples)
        st = pcm.host_stats()
        assert st["n_pieces"] == 4 and st["piece_frames"] == range_samples
        for ref in (rh, rp):     # the test's own premise: the extreme sits in the last range
            assert np.argmax(np.abs(ref)) >= 3 * range_samples and M.peak_of(ref[:3 * range_samples]) < M.peak_of(ref)
        assert pk.tobytes() == np.array([M.peak_of(rh), M.peak_of(rp), 0], np.float32).tobytes()
        assert np.array_equal(hh, M.from_float_peak(rh, pk[0])) and np.array_equal(pp, M.from_float_peak(rp, pk[1]))
        assert not rr.any()
        gain = np.float32(32767.0) / M.peak_of(rp)
        pp2 = np.full(n, 12345, np.int16)
        pcm.hpri_process(g, x16, channels=ch, perc=pp2, mode=pcm.GAIN, gain=float(gain), range_samples=range_samples)
        assert pcm.host_stats()["n_pieces"] == 4
        assert np.array_equal(pp2, M.from_float_gain(rp, gain))
        # pinned buffers, default parameters of the engine family on a second handle's worth of state: same samples
        pin_in, pin_out = pcm.PinnedPCM(x16.size), pcm.PinnedPCM(n)
        pin_in.array[:] = x16
        pcm.hpri_process(g, pin_in.array, channels=ch, harm=pin_out.array, mode=pcm.PEAK, range_samples=range_samples)
        assert np.array_equal(pin_out.array, hh)
        pin_in.free()
        pin_out.free()
    finally:
        pcm.release(g)


def test_offline_ranges_shorter_than_their_halo(pcm, oracle):
    """ranges of 16384 samples at hops 4096 / 256, whose look-ahead is longer than a range: the input is all up before the
    last range is reached, and a range that has nothing to add still records that its input is up"""
    range_samples = 16384
    n = 6 * range_samples + 5003
    g, x16, rh, rp = offline_case(oracle, n, 70, hops=(4096, 256))
    hh, pp, rr = (np.full(n, 12345, np.int16) for _ in range(3))
    try:
        n_ranges = -(-n // range_samples)
        in_end = [min(n, g.range_halo(n, k * range_samples, min(n, (k + 1) * range_samples))[1]) for k in range(n_ranges)]
        # the test's own premise
        assert any(in_end[k] <= in_end[k - 1] for k in range(1, n_ranges)), in_end
        assert any(in_end[k] >= n for k in range(n_ranges - 1)), in_end
        pk = pcm.hpri_process(g, x16, harm=hh, perc=pp, resid=rr, mode=pcm.PEAK, range_samples=range_samples)
        st = pcm.host_stats()
        assert st["n_pieces"] == n_ranges == 7 and st["piece_frames"] == range_samples
        assert pk.tobytes() == np.array([M.peak_of(rh), M.peak_of(rp), 0], np.float32).tobytes()
        assert np.array_equal(hh, M.from_float_peak(rh, pk[0])) and np.array_equal(pp, M.from_float_peak(rp, pk[1]))
        assert not rr.any()
    finally:
        pcm.release(g)


def test_offline_refusals(pcm, oracle):
    import zen_amd
    n = 20000
    g, x16, rh, rp = offline_case(oracle, n, 60)
    big = np.zeros(2 * n, np.int16)
    out = np.zeros(n, np.int16)
    lib = pcm.load()
    batch = zen_amd.HPRIOffline(FS, 1024, 256, 2.0, 2.0, n_clips=2)
    try:
        bad = [
            lambda: pcm.hpri_process(g, big[:n], perc=big[n - 4:2 * n - 4], mode=pcm.GAIN),
            lambda: pcm.hpri_process(g, x16, harm=big[:n], perc=big[n - 4:2 * n - 4], mode=pcm.GAIN),
            lambda: pcm.hpri_process(g, x16, harm=out, resid=out, mode=pcm.GAIN),
            lambda: pcm._ck(lib.zen_hip_pcm_hpri_process(g._h, x16.ctypes.data, 3, 100, out.ctypes.data, None, None, 0, 1.0, None, 0)),
            lambda: pcm._ck(lib.zen_hip_pcm_hpri_process(g._h, None, 1, 100, out.ctypes.data, None, None, 0, 1.0, None, 0)),
            lambda: pcm._ck(lib.zen_hip_pcm_hpri_process(batch._h, x16.ctypes.data, 1, n, out.ctypes.data, None, None, 0, 1.0, None, 0)),
        ]
        for i, call in enumerate(bad):
            with pytest.raises(zen_amd.ZenHipError) as e:
                call()
            assert e.value.code == zen_amd.lib.E_BAD_ARG and len(str(e.value)) > 30, i
        pcm.hpri_process(g, x16, perc=out, mode=pcm.PEAK)
        assert np.array_equal(out, M.from_float_peak(rp, M.peak_of(rp)))
    finally:
        pcm.release(g)
        pcm.release(batch)
