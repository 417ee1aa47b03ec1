"""GPU tier: libzen_hip_beat.so (zen_amd/beat) -- the onset function and the beat tracker on device rows.  Tolerance 0
everywhere: the onset function, the score, the beat flags and the tempo are compared bit for bit against tests/beat_model.py.
Every device call goes through run_device below: NaNs around the input rows (a kernel that read outside the hops of its call
would carry them into a result) and sentinels around every output row."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import beat_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
NAMES = ("odf", "score", "beat", "tempo")
FS, HOP, HOPS = 8000.0, 64, 600          # the shape of the cutting tests: 38 400 samples per stream


@pytest.fixture(scope="module")
def beat():
    """The library of this feature, built on demand (the session fixture of conftest.py builds the one it links against)."""
    import zen_amd
    from zen_amd import beat as mod
    mod.load()
    zen_amd.init(0)
    return mod


_model = {}


def model(oracle, key, x, fs, hop):
    """the model's four rows for the streams of `x` (n_streams, m), computed once per key"""
    full = (key, fs, hop, x.shape)
    if full not in _model:
        oracle.lib()
        _model[full] = M.track(x, fs, hop)
    return _model[full]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_device(bt, x, lead=(0, 0, 0, 0, 0), pad=(0, 0), want=(True, True, True, True), cuts=None, before=None):
    """x: (n_streams, n_hops * hop) rows.  `lead` floats in front of the input / odf / score / beat / tempo rows, `pad` floats
    between the rows (input, outputs).  `cuts`: the hops of each call (default: one call of all); `before(i)` runs in front of
    call i.  Returns the four results as (n_streams, n_hops) arrays, None for one that was not asked for."""
    import zen_amd
    x = np.asarray(x, np.float32).reshape(bt.n_streams, -1)
    S, span = x.shape
    hop = bt.hop
    n_hops = span // hop
    assert span == n_hops * hop
    cuts = [n_hops] if cuts is None else cuts
    assert sum(cuts) == n_hops
    in_stride, out_stride = span + pad[0], n_hops + pad[1]
    in_host = np.full(lead[0] + S * in_stride + 8, np.nan, np.float32)
    for s in range(S):
        in_host[lead[0] + s * in_stride:lead[0] + s * in_stride + span] = x[s]
    inp = zen_amd.DeviceBuffer.from_host(in_host)
    outs = [zen_amd.DeviceBuffer.from_host(np.full(lead[1 + k] + S * out_stride + 8, SENTINEL, np.float32)) for k in range(4)]
    c0 = 0
    for i, c in enumerate(cuts):
        if before:
            before(i)
        bt.run_device(inp.offset(lead[0] + c0 * hop), in_stride, c, *(outs[k].offset(lead[1 + k] + c0) if want[k] else None for k in range(4)),
                      out_stride=out_stride)
        c0 += c
    zen_amd.synchronize()
    assert np.array_equal(inp.download(), in_host, equal_nan=True), "the input buffer was written"
    res = []
    for k in range(4):
        got = outs[k].download()
        if not want[k]:
            assert np.all(got == SENTINEL), "%s was not asked for" % NAMES[k]
            res.append(None)
            continue
        ld = lead[1 + k]
        assert np.all(got[:ld] == SENTINEL) and np.all(got[ld + S * out_stride:] == SENTINEL), NAMES[k]
        rows = got[ld:ld + S * out_stride].reshape(S, out_stride)
        assert np.all(rows[:, n_hops:] == SENTINEL), "%s written beyond the hops of the call" % NAMES[k]
        res.append(rows[:, :n_hops].copy())
    return res


def assert_equals_model(got, want, what):
    for k in range(4):
        if got[k] is None:
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, NAMES[k], g.shape, w.shape)
        diff = np.flatnonzero(bits(g).ravel() != bits(w).ravel())
        assert diff.size == 0, "%s: %s differs from the model in %d places, the first at %d: %r != %r" % (
            what, NAMES[k], diff.size, diff[0], g.ravel()[diff[0]], w.ravel()[diff[0]])


# ================================================================================================ against the model
@pytest.mark.parametrize("fs,hop,n_hops", [(8000.0, 64, 600), (16000.0, 128, 200), (44100.0, 512, 150), (48000.0, 2048, 40)])
def test_edge_inputs_three_streams(beat, oracle, fs, hop, n_hops):
    """zeros, a constant, noise, clicks, a tone and a click track, three streams per call with padded strides and rows that
    start 4, 8 or 12 bytes past a 16-byte boundary.  600 hops of the click track at 8000/64 are ten beats and as many tempo
    estimates; 40 hops at 48000/2048 (frames of 4096) reach the first prediction at hop 10."""
    sig = M.edge_inputs(fs, hop, n_hops)
    names = list(sig)
    assert names == ["zeros", "constant", "noise", "clicks", "tone", "beats"]
    bt = beat.Beat(fs, hop, n_streams=3)
    for g in range(2):
        group = names[3 * g:3 * g + 3]
        x = np.stack([sig[n] for n in group])
        want = model(oracle, ("edge", g), x, fs, hop)
        bt.reset()
        got = run_device(bt, x, lead=(1 + g, g % 4, (g + 1) % 4, (g + 2) % 4, (g + 3) % 4), pad=(3 + g, 5 - g))
        assert_equals_model(got, want, "%g/%d %s" % (fs, hop, group))
        if g == 1:
            beats = want[2][2]
            assert want[2].sum(axis=1).min() >= 1 and np.all(want[3] >= 79.0) and np.all(want[3] <= 161.0)
            if n_hops == 600:       # what the click track is there for
                assert beats.sum() >= 6, "at least 5 tempo estimates behind the first beat"
                assert abs(float(want[3][2][-1]) - 126.0) <= 6.0


@pytest.fixture(scope="module")
def cutting(oracle):
    """the three streams of the cutting tests and the model's rows"""
    sig = M.edge_inputs(FS, HOP, HOPS, seed=1)
    x = np.stack([sig["beats"], sig["noise"], sig["clicks"]])
    return x, model(oracle, "cutting", x, FS, HOP)


@pytest.mark.parametrize("cuts", ["one", "ones", "uneven"])
def test_a_stream_cut_into_calls_gives_the_same_bits(beat, cutting, cuts):
    x, want = cutting
    plan = {"one": [HOPS], "ones": [1] * HOPS, "uneven": [7, 64, HOPS - 71]}[cuts]
    got = run_device(beat.Beat(FS, HOP, n_streams=3), x, lead=(3, 1, 2, 3, 0), pad=(1, 2), cuts=plan)
    assert_equals_model(got, want, "calls of %s" % cuts)


@pytest.mark.parametrize("max_hops", [16, 0])
def test_slices_of_max_hops_give_the_same_bits_one_track_launch_each(beat, cutting, max_hops):
    x, want = cutting
    bt = beat.Beat(FS, HOP, n_streams=3, max_hops=max_hops)
    bt.profile(True)
    got = run_device(bt, x, lead=(2, 0, 1, 2, 3), pad=(2, 1))
    assert_equals_model(got, want, "max_hops %d" % max_hops)
    slices = -(-HOPS // (max_hops or 4096))
    prof = bt.profile_get()
    assert list(prof) == list(beat.KERNELS)
    for name, p in prof.items():
        assert p["launches"] == slices and p["ms"] > 0 and p["bytes"] > 0, name
    assert all(p["launches"] == 0 for p in bt.profile_get().values())
    assert bt.stats()["slices"] == slices and bt.stats()["hops"] == 3 * HOPS


def test_reset_in_the_middle_starts_a_fresh_session(beat, oracle, cutting):
    x, want = cutting
    half = 301 * HOP
    bt = beat.Beat(FS, HOP, n_streams=3, max_hops=128)
    got = run_device(bt, x, cuts=[301, HOPS - 301], before=lambda i: bt.reset() if i == 1 else None)
    fresh = model(oracle, "cutting-second-half", x[:, half:], FS, HOP)
    assert_equals_model([g[:, :301] for g in got], [w[:, :301] for w in want], "before the reset")
    assert_equals_model([g[:, 301:] for g in got], fresh, "behind the reset")
    assert not np.array_equal(bits(fresh[1]), bits(want[1][:, 301:])), "the reset is visible in the scores"


def test_no_hops_and_each_output_on_its_own(beat, cutting):
    x, want = cutting
    x, want = x[:1, :80 * HOP], [w[:1, :80] for w in want]
    bt = beat.Beat(FS, HOP)
    for k in range(4):
        bt.reset()
        got = run_device(bt, x, want=tuple(j == k for j in range(4)), lead=(1, 1, 1, 1, 1))
        assert_equals_model(got, want, "only %s" % NAMES[k])
    bt.reset()
    run_device(bt, x, want=(False, False, False, False))
    before = bt.stats()
    got = run_device(bt, x[:, :0])
    assert all(g.size == 0 for g in got)
    bt.run_device(None, 0, 0)                                  # nothing to read: no input needed
    assert bt.stats() == before
    assert bt.run(np.zeros(HOP - 1, np.float32))[0].shape == (0,)
    bt.reset()                                                 # none of that moved the state
    assert_equals_model(run_device(bt, x), want, "behind the empty calls")


def test_run_host_equals_run_device(beat, cutting):
    x, want = cutting
    bt = beat.Beat(FS, HOP, n_streams=3, max_hops=100)
    host = bt.run(x[:, :450 * HOP])
    assert host[0].shape == (3, 450)
    assert_equals_model(list(host), [w[:, :450] for w in want], "run_host")
    rest = bt.run(x[:, 450 * HOP:])                            # the session goes on across host calls
    assert_equals_model(list(rest), [w[:, 450:] for w in want], "run_host, second call")
    one = beat.Beat(FS, HOP).run(x[0, :100 * HOP])
    assert one[0].shape == (100,)
    assert_equals_model([o[None] for o in one], [w[:1, :100] for w in want], "one stream")


# ================================================================================================ arguments, memory
def test_bad_arguments_are_refused_and_touch_nothing(beat):
    import ctypes as C

    import zen_amd
    cnt = 4
    L, BAD = beat.load(), 2
    h = C.c_void_p()
    for fs, hop in M.REFUSED + ((44100.0, 96), (44100.0, 4096)):
        assert L.zen_hip_beat_create(fs, hop, 1, 0, C.byref(h)) == BAD
    assert L.zen_hip_beat_create(FS, HOP, 0, 0, C.byref(h)) == BAD and h.value is None
    bt = beat.Beat(FS, HOP)
    x = M.edge_inputs(FS, HOP, cnt)["noise"]
    inp = zen_amd.DeviceBuffer.from_host(x)
    out = zen_amd.DeviceBuffer.from_host(np.full(4 * cnt, SENTINEL, np.float32))
    o = [out.offset(k * cnt) for k in range(4)]
    cases = [(None, inp.ptr, cnt * HOP, o[0], o[3], cnt),          # null handle
             (bt._h, None, cnt * HOP, o[0], o[3], cnt),            # null input
             (bt._h, inp.ptr, cnt * HOP - 1, o[0], o[3], cnt),     # in_stride below the hops of a row
             (bt._h, inp.ptr, cnt * HOP, o[0], o[3], cnt - 1),     # out_stride below the hops of a row
             (bt._h, inp.ptr + 2, cnt * HOP, o[0], o[3], cnt),     # pointers that are not 4-byte aligned
             (bt._h, inp.ptr, cnt * HOP, o[0] + 1, o[3], cnt),
             (bt._h, inp.ptr, cnt * HOP, o[0], o[3] + 2, cnt)]
    before = bt.stats()
    for hh, a, in_stride, p0, p3, out_stride in cases:
        for f in (L.zen_hip_beat_run_device, L.zen_hip_beat_run_host):
            assert f(hh, a, in_stride, cnt, p0, o[1], o[2], p3, out_stride) == BAD
            assert L.zen_hip_beat_last_error() != b""
    with pytest.raises(zen_amd.ZenHipError) as e:
        beat.Beat(44100.0, 256)
    assert e.value.code == BAD
    zen_amd.synchronize()
    assert bt.stats() == before
    assert np.all(out.download() == SENTINEL) and np.array_equal(inp.download(), x)
    # the handle is still good
    assert bt.run(x)[0].shape == (cnt,) and bt.stats()["hops"] == cnt


def test_calls_after_create_allocate_nothing(beat):
    import zen_amd
    for fs, hop, cnt in ((FS, HOP, 40), (48000.0, 2048, 9)):
        x = M.edge_inputs(fs, hop, cnt)["noise"]
        inp = zen_amd.DeviceBuffer.from_host(x)
        outs = [zen_amd.DeviceBuffer.from_host(np.full(cnt, SENTINEL, np.float32)) for _ in range(4)]
        bt = beat.Beat(fs, hop, max_hops=4)
        zen_amd.synchronize()
        st0, mc0 = bt.stats(), zen_amd.memcheck()
        assert st0["allocations"] == 10 and st0["device_bytes"] >= 4 * (16 * hop + 32 + 4 * hop) and st0["hops"] == 0
        for _ in range(3):
            bt.run_device(inp, cnt * hop, cnt, *outs, out_stride=cnt)
        bt.reset()
        bt.run(x)
        zen_amd.synchronize()
        st1, mc1 = bt.stats(), zen_amd.memcheck()
        assert st1["allocations"] == st0["allocations"] and st1["device_bytes"] == st0["device_bytes"]
        assert st1["hops"] == 4 * cnt and st1["slices"] == 4 * -(-cnt // 4)
        if mc1["redzone_bytes"]:
            assert mc1["allocations"] == mc0["allocations"] and mc1["live_allocations"] == mc0["live_allocations"]
            assert mc1["corrupt_words"] == 0


# ================================================================================================ behind the separation
@pytest.fixture(scope="module")
def claim(beat, oracle):
    """the input of the claim (tests/test_beat_model.py): track_hpr's two columns and the model's"""
    x = M.claim_input()
    with_hpr, without = beat.track_hpr(x, 44100.0)
    m = x.size // 1024 * 1024
    perc = oracle.HPR(44100.0, 1024, 2.5, oracle.OUTPUT_PERCUSSIVE, oracle.TIME_CAUSAL).process_stream(x[:m])["P"]
    return x, with_hpr, without, M.track(perc, 44100.0, 512), M.track(x[:m], 44100.0, 512)


def test_track_hpr_on_the_device_equals_the_model_on_the_oracles_percussive_stream(claim):
    x, with_hpr, without, want_with, want_without = claim
    assert with_hpr[0].shape == without[0].shape == (x.size // 1024 * 2,)
    assert_equals_model(list(with_hpr), list(want_with), "with the separation")
    assert_equals_model(list(without), list(want_without), "without the separation")
    assert with_hpr[2].sum() >= 10 and without[2].sum() >= 10


def write_wav_float32(path, x, fs):
    """mono IEEE-float WAV: the samples reach the program bit for bit"""
    x = np.ascontiguousarray(x, "<f4")
    hdr = b"RIFF" + np.uint32(36 + x.nbytes).tobytes() + b"WAVEfmt " + np.uint32(16).tobytes()
    hdr += np.array([3, 1], "<u2").tobytes() + np.array([fs, fs * 4], "<u4").tobytes() + np.array([4, 32], "<u2").tobytes()
    hdr += b"data" + np.uint32(x.nbytes).tobytes()
    with open(path, "wb") as f:
        f.write(hdr + x.tobytes())


def test_beat_track_program_prints_the_models_beat_times(claim, tmp_path):
    from zen_amd.addon_build import beat as addon
    x, _, _, want_with, want_without = claim
    wav = str(tmp_path / "claim.wav")
    write_wav_float32(wav, x, 44100)
    r = subprocess.run([addon.build_demo(), wav], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    assert len(lines) == 3 and lines[2] == ""
    for line, title, want in ((lines[0], "+HPR", want_with), (lines[1], "-HPR", want_without)):
        times = M.beat_times(want[2], 512, 44100.0)
        assert times.size >= 10
        assert line == "%s beat timestamps: " % title + "".join("%.4f " % t for t in times), line
