"""GPU tier: packed 24-bit samples through libzen_hip_pcm.so (zen_amd/pcm).  Tolerance 0 everywhere: bytes are compared
with ==, against the numpy models of tests/pcm24_model.py and tests/pcm_model.py applied to what the FLOAT calls of the same
engines return for the model's widened input -- which tests/test_gpu_pcm.py ties to the oracle."""
import ctypes
import os
import sys
import wave

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pcm24_model as M   # noqa: E402
import pcm_model as M16   # noqa: E402

pytestmark = pytest.mark.gpu
FS = 44100.0
H, P, R = 1, 2, 4       # ZEN_HIP_OUTPUT_*
GROUP = 16              # samples of a body group: 48 bytes
# a full grid's worth of body groups: 8 workgroups of 256 threads per CU, one group per thread and turn (256 CUs: MI355X;
# with fewer the stride loop below only turns more often)
FULL_GRID_GROUPS = 8 * 256 * 256


@pytest.fixture(scope="module")
def pcm():
    import zen_amd
    from zen_amd import pcm as mod
    from zen_amd.addon_build import pcm as addon
    if not os.path.exists(addon.OUT):
        addon.build()
    mod.load()
    zen_amd.init(0)
    before = zen_amd.memcheck()
    yield mod
    mod.release_all()
    # the memory checker at the end of the module: red zones and poison were on throughout (conftest.py), and nothing was
    # found in this module's time (the counters are cumulative over the session)
    rep = zen_amd.memcheck()
    assert rep["redzone_bytes"] >= 4096 or os.environ.get("ZEN_HIP_REDZONE") == "0"
    assert rep["corrupt_words"] == before["corrupt_words"] and rep["bounds_violations"] == before["bounds_violations"], rep["first_message"]


def random24(n, seed):
    return np.random.default_rng(seed).integers(M.LO, M.HI + 1, n).astype(np.int32)


def audio24(n, seed, channels=1, level=0.5, click=0.9):
    """random 24-bit audio plus a sine and clicks, packed: 3 * n * channels bytes of interleaved frames"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    out = []
    for c in range(channels):
        x = level * rng.uniform(-1, 1, n) + 0.3 * np.sin(2 * np.pi * (440 + 110 * c) * t)
        for s in range(1500 + 700 * c, n, 9001):
            x[s:s + 30] += click
        out.append(np.clip(np.round(x * 8388607), M.LO, M.HI).astype(np.int32))
    v = out[0] if channels == 1 else np.stack(out, 1).reshape(-1)
    return M.store(v)


def narrow(fmt_bits, y, mode, scale):
    """the model's bytes of a float output: fmt_bits 24 -> packed uint8, 16 -> int16"""
    if fmt_bits == 24:
        return M.store(M.from_float_peak(y, scale) if mode == "peak" else M.from_float_gain(y, scale))
    return M16.from_float_peak(y, scale) if mode == "peak" else M16.from_float_gain(y, scale)


# ================================================================================================ the kernels alone
LENGTHS = (0, 1, 5, 15, 16, 17, 47, 48, 49, 65, 4097)
GUARD = 16


@pytest.mark.parametrize("channels", (1, 2), ids=("mono", "stereo"))
def test_unpack_kernel_lengths_and_alignments(pcm, channels):
    import zen_amd
    nmax = max(LENGTHS)
    src_h = np.random.default_rng(1).integers(0, 256, 3 * channels * nmax + 16).astype(np.uint8)
    src_h[:12] = [255, 255, 127, 0, 0, 128, 255, 255, 255, 1, 0, 0]          # both ends of the range, -1, 1
    src = zen_amd.DeviceBuffer.from_host(src_h)
    dst = zen_amd.DeviceBuffer(nmax + 2 * GUARD + 1)
    assert src.ptr % 16 == 0 and dst.ptr % 16 == 0
    sentinel = np.full(dst.n, 12345.0, np.float32)
    for n in LENGTHS:
        for so in range(16):                       # every byte offset of the source from a 16-byte boundary
            for do in (0, 1):                      # the float side on a 16-byte boundary, and off it
                dst.upload(sentinel)
                pcm.to_float(src.ptr + so, channels, n, dst.offset(GUARD + do), fmt=pcm.I24)
                zen_amd.synchronize()
                got = dst.download()
                want = M.widen(src_h[so:so + 3 * channels * n], channels)
                assert np.array_equal(got[GUARD + do:GUARD + do + n], want), (n, so, do)
                assert np.all(got[:GUARD + do] == 12345.0) and np.all(got[GUARD + do + n:] == 12345.0), (n, so, do)


def test_unpack_kernel_second_turn_of_the_stride_loop(pcm):
    """one group more than a full grid takes in one turn, plus a tail of 5; from an aligned and from an odd address"""
    import zen_amd
    n = GROUP * (FULL_GRID_GROUPS + 1) + 5
    src_h = np.random.default_rng(2).integers(0, 256, 3 * n + 16).astype(np.uint8)
    src = zen_amd.DeviceBuffer.from_host(src_h)
    dst = zen_amd.DeviceBuffer(n + 2 * GUARD)
    for so in (0, 7):
        dst.upload(np.full(dst.n, 12345.0, np.float32))
        pcm.to_float(src.ptr + so, 1, n, dst.offset(GUARD), fmt=pcm.I24)
        zen_amd.synchronize()
        got = dst.download()
        assert np.array_equal(got[GUARD:GUARD + n], M.widen(src_h[so:so + 3 * n])), so
        assert np.all(got[:GUARD] == 12345.0) and np.all(got[GUARD + n:] == 12345.0), so


def pack_inputs(n, seed):
    """floats for the packing kernel at the scale of a separator's output (|y| up to 3e4), specials in front"""
    y = np.random.default_rng(seed).uniform(-3e4, 3e4, n).astype(np.float32)
    y[:16] = [0.0, -0.0, np.nan, np.inf, -np.inf, 3e4, -3e4, 1e-40, 0.5, -0.5, 1.5, 2.5, 29999.5, -29999.5, 7.49999952, 1e9]
    return y


@pytest.mark.parametrize("mode", ("peak", "gain"))
def test_pack_kernel_lengths_and_alignments(pcm, mode):
    import zen_amd
    nmax = max(LENGTHS)
    y = pack_inputs(nmax + 4, 3)
    src = zen_amd.DeviceBuffer.from_host(y)
    dst = zen_amd.DeviceBuffer(3 * nmax + 2 * GUARD + 16, np.uint8)
    assert src.ptr % 16 == 0 and dst.ptr % 16 == 0
    sentinel = np.full(dst.n, 0xA5, np.uint8)
    mm = zen_amd.DeviceBuffer.from_host(np.array([-20000.0, 31000.0], np.float32))
    gain = np.float32(2 * 8388608.0 / 31000.0)         # clips on both sides
    for n in LENGTHS:
        for do in range(16):                       # every byte offset of the destination from a 16-byte boundary
            for so in (0, 1):                      # the float side on a 16-byte boundary, and off it
                dst.upload(sentinel)
                if mode == "peak":
                    pcm.from_float(src.offset(so), n, dst.ptr + GUARD + do, mode=pcm.PEAK, minmax_dev=mm.ptr, fmt=pcm.I24)
                    want = M.store(M.from_float_peak(y[so:so + n], 31000.0))
                else:
                    pcm.from_float(src.offset(so), n, dst.ptr + GUARD + do, mode=pcm.GAIN, gain=float(gain), fmt=pcm.I24)
                    want = M.store(M.from_float_gain(y[so:so + n], gain))
                zen_amd.synchronize()
                got = dst.download()
                b, e = GUARD + do, GUARD + do + 3 * n
                assert np.array_equal(got[b:e], want), (n, so, do)
                # guard BYTES directly in front of and behind the 3 n bytes
                assert np.all(got[:b] == 0xA5) and np.all(got[e:] == 0xA5), (n, so, do)


def test_pack_kernel_boundaries_and_second_turn(pcm):
    import zen_amd
    v = M.boundary_values()
    src, dst = zen_amd.DeviceBuffer.from_host(v), zen_amd.DeviceBuffer(3 * v.size, np.uint8)
    pcm.from_float(src.ptr, v.size, dst.ptr, mode=pcm.GAIN, gain=1.0, fmt=pcm.I24)
    zen_amd.synchronize()
    want = M.from_float_gain(v, 1.0)
    assert want[:6].tolist() == [1, -1, 2, -2, 0, 0] and want[10:15].tolist() == [M.HI, M.HI, M.HI, M.LO, M.LO]
    assert np.array_equal(dst.download(), M.store(want))
    mm = zen_amd.DeviceBuffer.from_host(np.array([-8388608.0, 1.0], np.float32))        # peak 2^23: x = v / 2^23 exactly
    pcm.from_float(src.ptr, v.size, dst.ptr, mode=pcm.PEAK, minmax_dev=mm.ptr, fmt=pcm.I24)
    zen_amd.synchronize()
    assert np.array_equal(dst.download(), M.store(want))
    # silence in PEAK mode: zeros
    mm0 = zen_amd.DeviceBuffer.from_host(np.zeros(2, np.float32))
    pcm.from_float(src.ptr, v.size, dst.ptr, mode=pcm.PEAK, minmax_dev=mm0.ptr, fmt=pcm.I24)
    zen_amd.synchronize()
    assert not dst.download().any()
    # one group more than a full grid takes in one turn, plus 5, at an odd destination
    n = GROUP * (FULL_GRID_GROUPS + 1) + 5
    y = pack_inputs(n, 4)
    big, out = zen_amd.DeviceBuffer.from_host(y), zen_amd.DeviceBuffer(3 * n + 2 * GUARD, np.uint8)
    out.upload(np.full(out.n, 0xA5, np.uint8))
    g = np.float32(8388608.0 / 3e4)
    pcm.from_float(big.ptr, n, out.ptr + GUARD + 3, mode=pcm.GAIN, gain=float(g), fmt=pcm.I24)
    zen_amd.synchronize()
    got = out.download()
    assert np.array_equal(got[GUARD + 3:GUARD + 3 + 3 * n], M.store(M.from_float_gain(y, g)))
    assert np.all(got[:GUARD + 3] == 0xA5) and np.all(got[GUARD + 3 + 3 * n:] == 0xA5)


def test_all_codes_on_the_device(pcm):
    """all 2^24 codes through the unpacking kernel in one launch, and through both kernels: the identity"""
    import zen_amd
    k = np.arange(M.LO, M.HI + 1, dtype=np.int32)
    packed = M.store(k)
    src, f = zen_amd.DeviceBuffer.from_host(packed), zen_amd.DeviceBuffer(k.size)
    pcm.to_float(src.ptr, 1, k.size, f.ptr, fmt=pcm.I24)
    zen_amd.synchronize()
    got = f.download()
    assert np.array_equal(got, k.astype(np.float32) / np.float32(8388608))
    back = zen_amd.DeviceBuffer(3 * k.size, np.uint8)
    pcm.from_float(f.ptr, k.size, back.ptr, mode=pcm.GAIN, gain=8388608.0, fmt=pcm.I24)
    zen_amd.synchronize()
    assert np.array_equal(back.download(), packed)
    # stereo pairs of extreme values, at full scale with an odd sum
    lr = np.array([M.HI, M.HI - 1, M.LO, M.LO + 1, M.HI, M.LO, -1, 0] * 4, np.int32)
    src2, dst2 = zen_amd.DeviceBuffer.from_host(M.store(lr)), zen_amd.DeviceBuffer(lr.size // 2)
    pcm.to_float(src2.ptr, 2, lr.size // 2, dst2.ptr, fmt=pcm.I24)
    zen_amd.synchronize()
    assert np.array_equal(dst2.download(), M.stereo_mix(lr))


# ================================================================================================ I16 through the format calls
def test_i16_through_the_format_calls_gives_the_existing_calls_bytes(pcm):
    """one shape of tests/test_gpu_pcm.py (hop 256, all outputs, 60 hops; the offline clip of 30011 frames) through the calls
    that take a format, with I16 both ways, against the int16 calls themselves"""
    import zen_amd
    L = pcm.load()
    rng = np.random.default_rng(6)
    n = 4095
    x16 = rng.integers(-32768, 32768, 2 * n + 8).astype(np.int16)
    src = zen_amd.DeviceBuffer.from_host(x16)
    fa, fb = zen_amd.DeviceBuffer(n + 8), zen_amd.DeviceBuffer(n + 8)
    for ch in (1, 2):
        for so in (0, 3):
            pcm.to_float(src.offset(so), ch, n, fa.offset(1))
            pcm._ck(L.zen_hip_pcm_unpack(pcm.I16, src.offset(so), ch, n, fb.offset(1), None))
            zen_amd.synchronize()
            assert np.array_equal(fa.download()[1:n + 1], fb.download()[1:n + 1]), (ch, so)
    y = pack_inputs(n + 8, 7)
    ysrc = zen_amd.DeviceBuffer.from_host(y)
    oa, ob = zen_amd.DeviceBuffer(n + 8, np.int16), zen_amd.DeviceBuffer(n + 8, np.int16)
    mm = zen_amd.DeviceBuffer.from_host(np.array([-20000.0, 31000.0], np.float32))
    for mode, gain in ((pcm.PEAK, 1.0), (pcm.GAIN, 1.7)):
        pcm.from_float(ysrc.offset(1), n, oa.offset(3), mode=mode, gain=gain, minmax_dev=mm.ptr)
        pcm._ck(L.zen_hip_pcm_pack(pcm.I16, ysrc.offset(1), n, mode, gain, mm.ptr, ob.offset(3), None))
        zen_amd.synchronize()
        assert np.array_equal(oa.download()[3:n + 3], ob.download()[3:n + 3]), mode
    # the two host calls
    hop, n_hops = 256, 60
    xb = rng.integers(-20000, 20000, hop * n_hops).astype(np.int16)
    ga, gb = (zen_amd.HPR(FS, hop, 2.0, H | P | R, zen_amd.TIME_CAUSAL) for _ in range(2))
    a = [np.zeros(xb.size, np.int16) for _ in range(3)]
    b = [np.zeros(xb.size, np.int16) for _ in range(3)]
    pk = (ctypes.c_float * 3)()
    try:
        pa = pcm.hpr_process_host(ga, xb, harm=a[0], perc=a[1], resid=a[2], mode=pcm.PEAK, piece_hops=7)
        pcm._ck(L.zen_hip_pcm_hpr_process_host_fmt(gb._h, pcm.I16, xb.ctypes.data, 1, n_hops, pcm.I16, b[0].ctypes.data, b[1].ctypes.data,
                                                   b[2].ctypes.data, pcm.PEAK, 1.0, pk, 7))
        assert pa.tobytes() == np.array(pk, np.float32).tobytes() and all(np.array_equal(u, v) and u.any() for u, v in zip(a, b))
    finally:
        pcm.release(ga)
        pcm.release(gb)
    n = 30011
    xo = rng.integers(-8000, 8000, 2 * n).astype(np.int16)
    oa_, ob_ = (zen_amd.HPRIOffline(FS, 1024, 256, 2.0, 2.0) for _ in range(2))
    a = [np.full(n, 77, np.int16) for _ in range(3)]
    b = [np.full(n, 77, np.int16) for _ in range(3)]
    try:
        pa = pcm.hpri_process(oa_, xo, channels=2, harm=a[0], perc=a[1], resid=a[2], mode=pcm.PEAK)
        pcm._ck(L.zen_hip_pcm_hpri_process_fmt(ob_._h, pcm.I16, xo.ctypes.data, 2, n, pcm.I16, b[0].ctypes.data, b[1].ctypes.data,
                                               b[2].ctypes.data, pcm.PEAK, 1.0, pk, 0))
        assert pa.tobytes() == np.array(pk, np.float32).tobytes() and all(np.array_equal(u, v) for u, v in zip(a, b))
        assert a[0].any() and a[1].any() and not a[2].any()
    finally:
        pcm.release(oa_)
        pcm.release(ob_)


# ================================================================================================ realtime block engine
RT = dict(hop=256, n_hops=40, flags=H | P | R)


@pytest.fixture(scope="module")
def rt_case(pcm):
    """I24 stereo in, and what the float call of a fresh engine returns for the model's widened input; computed once"""
    import zen_amd
    x24 = audio24(RT["hop"] * RT["n_hops"], 0, channels=2)
    xf = M.widen(x24, 2)
    eng = zen_amd.HPR(FS, RT["hop"], 2.0, RT["flags"], zen_amd.TIME_CAUSAL)
    ref = {k: np.zeros(xf.size, np.float32) for k in ("harm", "perc", "resid")}
    eng.process_host(xf, **ref)
    for v in ref.values():
        v.setflags(write=False)
    assert all(v.any() for v in ref.values())
    return x24, xf, ref


def new_rt():
    import zen_amd
    return zen_amd.HPR(FS, RT["hop"], 2.0, RT["flags"], zen_amd.TIME_CAUSAL)


@pytest.mark.parametrize("piece_hops", (7, 0), ids=("ragged_pieces", "one_piece"))
def test_realtime_block_i24(pcm, rt_case, piece_hops):
    x24, xf, ref = rt_case
    assert RT["n_hops"] % 7 != 0
    n = xf.size
    g = new_rt()
    try:
        outs = {k: np.full(3 * n, 0xA5, np.uint8) for k in ref}
        peaks = pcm.hpr_process_host(g, x24, channels=2, mode=pcm.PEAK, piece_hops=piece_hops, **outs)
        assert pcm.host_stats()["n_pieces"] == (-(-RT["n_hops"] // 7) if piece_hops else 1)
        for i, k in enumerate(("harm", "perc", "resid")):
            pk = M.peak_of(ref[k])
            assert peaks[i].tobytes() == pk.tobytes(), (k, peaks[i], pk)
            assert np.array_equal(outs[k], narrow(24, ref[k], "peak", pk)), k
        # P alone as I16 in GAIN mode, from the same 24-bit input: 24 in, 16 out
        g.reset_buffers()
        gain = np.float32(0.9 * 32767.0) / M.peak_of(ref["perc"])
        p16 = np.full(n, 12345, np.int16)
        assert pcm.hpr_process_host(g, x24, channels=2, perc=p16, mode=pcm.GAIN, gain=float(gain), piece_hops=piece_hops) is None
        assert np.array_equal(p16, narrow(16, ref["perc"], "gain", gain))
    finally:
        pcm.release(g)


def test_realtime_two_calls_equal_one_pinned_equals_pageable(pcm, rt_case):
    x24, xf, ref = rt_case
    n, hop = xf.size, RT["hop"]
    gain = np.float32(8388608.0 / 4) / M.peak_of(ref["harm"])
    want = {k: narrow(24, ref[k], "gain", gain) for k in ref}
    g, g2 = new_rt(), new_rt()
    pin_in, pins = pcm.PinnedPCM(2 * n, pcm.I24), {k: pcm.PinnedPCM(n, pcm.I24) for k in ref}
    try:
        cut = 23 * hop
        a = {k: np.zeros(3 * cut, np.uint8) for k in ref}
        b = {k: np.zeros(3 * (n - cut), np.uint8) for k in ref}
        pcm.hpr_process_host(g, x24[:6 * cut].copy(), channels=2, mode=pcm.GAIN, gain=float(gain), piece_hops=5, **a)
        pcm.hpr_process_host(g, x24[6 * cut:].copy(), channels=2, mode=pcm.GAIN, gain=float(gain), **b)
        for k in ref:
            assert np.array_equal(np.concatenate([a[k], b[k]]), want[k]), k
        # pinned buffers: asynchronous copies; the same bytes
        assert pin_in.array.dtype == np.uint8 and pin_in.array.size == 6 * n
        pin_in.array[:] = x24
        pcm.hpr_process_host(g2, pin_in.array, channels=2, mode=pcm.GAIN, gain=float(gain), piece_hops=7, **{k: p.array for k, p in pins.items()})
        st = pcm.host_stats()
        assert st["input_pinned"] and st["outputs_pinned"] and st["n_pieces"] == 6
        for k in ref:
            assert np.array_equal(pins[k].array, want[k]), k
    finally:
        pcm.release(g)
        pcm.release(g2)
        pin_in.free()
        for p in pins.values():
            p.free()


def test_realtime_refusals_in_the_formats_bytes(pcm, rt_case):
    """two I24 outputs 3 n - 1 bytes apart overlap, 3 n apart they do not; outputs of two formats in one call are the
    binding's to refuse; the engine's state is untouched by the refusals"""
    import zen_amd
    x24, xf, ref = rt_case
    n = xf.size
    g = new_rt()
    big = np.zeros(6 * n + 8, np.uint8)
    try:
        with pytest.raises(zen_amd.ZenHipError) as e:
            pcm.hpr_process_host(g, x24, channels=2, harm=big[:3 * n], perc=big[3 * n - 1:6 * n - 1], mode=pcm.GAIN)
        assert e.value.code == zen_amd.lib.E_BAD_ARG and "overlap" in str(e.value)
        with pytest.raises(zen_amd.ZenHipError) as e:
            pcm._ck(pcm.load().zen_hip_pcm_hpr_process_host_fmt(g._h, 2, x24.ctypes.data, 2, 4, pcm.I24, big.ctypes.data, None, None, 1, 1.0, None, 0))
        assert e.value.code == zen_amd.lib.E_BAD_ARG and "(got 2)" in str(e.value)
        with pytest.raises(AssertionError):
            pcm.hpr_process_host(g, x24, channels=2, harm=big[:3 * n], perc=np.zeros(n, np.int16), mode=pcm.GAIN)
        gain = np.float32(1000.0)
        pcm.hpr_process_host(g, x24, channels=2, harm=big[:3 * n], perc=big[3 * n:6 * n], mode=pcm.GAIN, gain=float(gain))     # 3 n apart
        assert np.array_equal(big[:3 * n], narrow(24, ref["harm"], "gain", gain))
        assert np.array_equal(big[3 * n:6 * n], narrow(24, ref["perc"], "gain", gain)) and not big[6 * n:].any()
    finally:
        pcm.release(g)


# ================================================================================================ offline two-pass engine
OFF_N, OFF_RANGE = 50000, 16384


@pytest.fixture(scope="module")
def offline_refs(pcm):
    """per (channels, soft): the packed clip and the float call's stems for the model's widened input; computed once"""
    import zen_amd
    refs = {}
    for channels in (1, 2):
        x24 = audio24(OFF_N, 40 + channels, channels, level=0.2, click=0.2)
        xf = M.widen(x24, channels)
        for soft in (False, True):
            eng = zen_amd.HPRIOffline(FS, 1024, 256, 2.0, 2.0)
            if soft:
                eng.use_soft_mask()
            rh, rp, rr = eng.process(xf)
            assert rh.any() and rp.any() and not rr.any()
            for a in (rh, rp):
                a.setflags(write=False)
            refs[channels, soft] = (x24, rh, rp)
    return refs


def new_offline(soft, hops=(1024, 256)):
    import zen_amd
    g = zen_amd.HPRIOffline(FS, hops[0], hops[1], 2.0, 2.0)
    if soft:
        g.use_soft_mask()
    return g


@pytest.mark.parametrize("soft", (False, True), ids=("hard", "soft"))
@pytest.mark.parametrize("channels", (1, 2), ids=("mono", "stereo"))
def test_offline_four_ranges(pcm, offline_refs, channels, soft):
    """50 000 frames in ranges of 16384: four ranges, the last one ragged, each upload starting at the sample the last one's
    halo ended on.  (The engine ends its halos on hops of pass 1, so in this pipeline every piece starts on a 16-byte
    boundary of its staging buffer; the other fifteen residues are the kernel tests' above.)"""
    x24, rh, rp = offline_refs[channels, soft]
    n = OFF_N
    g = new_offline(soft)
    try:
        ends = [min(n, g.range_halo(n, b, min(n, b + OFF_RANGE))[1]) for b in range(0, n, OFF_RANGE)]
        assert len(ends) == 4 and ends[0] < ends[1] < ends[-1] == n, ends                          # several uploads, the last to the clip's end
        hh, pp, rr = (np.full(3 * n, 0xA5, np.uint8) for _ in range(3))
        pk = pcm.hpri_process(g, x24, channels=channels, harm=hh, perc=pp, resid=rr, mode=pcm.PEAK, range_samples=OFF_RANGE)
        st = pcm.host_stats()
        assert st["n_pieces"] == 4 and st["piece_frames"] == OFF_RANGE
        assert pk.tobytes() == np.array([M.peak_of(rh), M.peak_of(rp), 0], np.float32).tobytes()
        assert np.array_equal(hh, narrow(24, rh, "peak", pk[0])) and np.array_equal(pp, narrow(24, rp, "peak", pk[1]))
        assert not rr.any()                                    # 3 n zero bytes
        # PEAK into I16 from the same 24-bit clip
        h16, p16, r16 = (np.full(n, 12345, np.int16) for _ in range(3))
        pk16 = pcm.hpri_process(g, x24, channels=channels, harm=h16, perc=p16, resid=r16, mode=pcm.PEAK, range_samples=OFF_RANGE)
        assert pk16.tobytes() == pk.tobytes()
        assert np.array_equal(h16, narrow(16, rh, "peak", pk[0])) and np.array_equal(p16, narrow(16, rp, "peak", pk[1])) and not r16.any()
    finally:
        pcm.release(g)


def test_offline_ranges_shorter_than_their_halo(pcm):
    """ranges of 16384 samples at hops 4096 / 256, whose look-ahead is longer than a range: a range that has nothing to add
    still records that its input is up; 16-bit in, 24-bit out -- what the separation computed is kept"""
    import zen_amd
    n = 3 * OFF_RANGE + 5003
    x24 = audio24(n, 70, 1, level=0.2, click=0.2)
    x16 = (M.load(x24) >> 8).astype(np.int16)
    g = new_offline(False, hops=(4096, 256))
    try:
        n_ranges = -(-n // OFF_RANGE)
        in_end = [min(n, g.range_halo(n, k * OFF_RANGE, min(n, (k + 1) * OFF_RANGE))[1]) for k in range(n_ranges)]
        assert any(in_end[k] <= in_end[k - 1] for k in range(1, n_ranges)), in_end         # the test's own premise
        rh, rp, _ = zen_amd.HPRIOffline(FS, 4096, 256, 2.0, 2.0).process(M16.to_float(x16))
        hh, pp = np.full(3 * n, 0xA5, np.uint8), np.full(3 * n, 0xA5, np.uint8)
        pk = pcm.hpri_process(g, x16, harm=hh, perc=pp, mode=pcm.PEAK, range_samples=OFF_RANGE)
        assert pcm.host_stats()["n_pieces"] == n_ranges == 4
        assert pk.tobytes() == np.array([M.peak_of(rh), M.peak_of(rp), 0], np.float32).tobytes()
        assert np.array_equal(hh, narrow(24, rh, "peak", pk[0])) and np.array_equal(pp, narrow(24, rp, "peak", pk[1]))
    finally:
        pcm.release(g)


def write_wav(path, frames, channels, width):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(int(FS))
        w.writeframes(frames.tobytes())


def read_wav(path):
    with wave.open(str(path), "rb") as w:
        return w.getnchannels(), w.getsampwidth(), w.getframerate(), w.readframes(w.getnframes())


def test_offline_wav(pcm, tmp_path):
    """one second of 24-bit stereo written with the standard library: the stems' frames are the offline test's model on the
    float call's output, at the file's depth and at 16 bits"""
    import zen_amd
    n = int(FS)
    x24 = audio24(n, 90, 2, level=0.2, click=0.2)
    write_wav(tmp_path / "in.wav", x24, 2, 3)
    rh, rp, _ = zen_amd.HPRIOffline(FS, 4096, 256, 2.5, 2.5).process(M.widen(x24, 2))
    pk = pcm.offline_wav(str(tmp_path / "in.wav"), str(tmp_path / "h.wav"), str(tmp_path / "p.wav"))
    assert pk.tobytes() == np.array([M.peak_of(rh), M.peak_of(rp)], np.float32).tobytes()
    for name, ref, peak in (("h.wav", rh, pk[0]), ("p.wav", rp, pk[1])):
        ch, width, rate, frames = read_wav(tmp_path / name)
        assert (ch, width, rate) == (1, 3, int(FS)) and frames == narrow(24, ref, "peak", peak).tobytes(), name
    pcm.offline_wav(str(tmp_path / "in.wav"), str(tmp_path / "h16.wav"), str(tmp_path / "p16.wav"), bits=16)
    for name, ref, peak in (("h16.wav", rh, pk[0]), ("p16.wav", rp, pk[1])):
        ch, width, rate, frames = read_wav(tmp_path / name)
        assert (ch, width, rate) == (1, 2, int(FS)) and frames == narrow(16, ref, "peak", peak).astype("<i2").tobytes(), name
    # a 16-bit file keeps its depth; other widths and files that are no WAV files are refused
    x16 = (M.load(x24) >> 8).astype("<i2")
    write_wav(tmp_path / "in16.wav", x16, 2, 2)
    pcm.offline_wav(str(tmp_path / "in16.wav"), str(tmp_path / "h2.wav"), str(tmp_path / "p2.wav"))
    assert read_wav(tmp_path / "h2.wav")[1] == 2
    write_wav(tmp_path / "in8.wav", np.zeros(n, np.uint8), 1, 1)
    with pytest.raises(ValueError):
        pcm.offline_wav(str(tmp_path / "in8.wav"), str(tmp_path / "x.wav"), str(tmp_path / "y.wav"))
    (tmp_path / "junk.wav").write_bytes(b"not a wav file at all")
    with pytest.raises(wave.Error):
        pcm.offline_wav(str(tmp_path / "junk.wav"), str(tmp_path / "x.wav"), str(tmp_path / "y.wav"))
    with pytest.raises(ValueError):
        pcm.offline_wav(str(tmp_path / "in.wav"), str(tmp_path / "x.wav"), str(tmp_path / "y.wav"), bits=32)
