"""GPU tier: libzen_hip_pitch.so (zen_amd/pitch) -- the McLeod pitch method on device rows.  Tolerance 0 everywhere: pitch,
period, clarity and the whole NSDF rows are compared bit for bit against tests/pitch_model.py.  Every device call goes
through run_device below: NaNs around the input rows (a kernel that read outside its chunks' span would carry them into a
result) and sentinels around every output row."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import pitch_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
FS = M.FS
SENTINEL = 12345.0
NAMES = ("pitch", "period", "clarity", "nsdf")


@pytest.fixture(scope="module")
def pitch():
    """The library of this feature, built on demand (the session fixture of conftest.py builds the one it links against)."""
    import zen_amd
    from zen_amd import pitch as mod
    mod.load()
    zen_amd.init(0)
    return mod


_model = {}


def model(oracle, key, x, n, step, n_chunks, fs=FS):
    """the model's four results for chunks of `x`, computed once per key"""
    full = (key, n, step, n_chunks)
    if full not in _model:
        oracle.lib()
        _model[full] = M.track(x, fs, n, step, n_chunks)
    return _model[full]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_device(pt, x, n_chunks, step, lead=(0, 0, 0, 0, 0), pad=(0, 0), want=(True, True, True, True)):
    """x: (n_streams, span) rows, span = (n_chunks - 1) * step + n.  `lead` floats in front of the input / pitch / period /
    clarity / nsdf rows, `pad` floats between the rows (input, outputs: in chunks).  Returns the four results as
    (n_streams, n_chunks[, n]) arrays, None for one that was not asked for."""
    import zen_amd
    x = np.asarray(x, np.float32).reshape(pt.n_streams, -1)
    S, span = x.shape
    n = pt.n
    assert n_chunks == 0 or span == (n_chunks - 1) * step + n
    in_stride, out_stride = span + pad[0], n_chunks + pad[1]
    in_host = np.full(lead[0] + S * in_stride + 8, np.nan, np.float32)
    for s in range(S):
        in_host[lead[0] + s * in_stride:lead[0] + s * in_stride + span] = x[s]
    inp = zen_amd.DeviceBuffer.from_host(in_host)
    per = (1, 1, 1, n)
    outs = [zen_amd.DeviceBuffer.from_host(np.full(lead[1 + k] + S * out_stride * per[k] + 8, SENTINEL, np.float32)) for k in range(4)]
    pt.run_device(inp.offset(lead[0]), in_stride, n_chunks, step, *(outs[k].offset(lead[1 + k]) if want[k] else None for k in range(4)),
                  out_stride=out_stride)
    zen_amd.synchronize()
    assert np.array_equal(inp.download(), in_host, equal_nan=True), "the input buffer was written"
    res = []
    for k in range(4):
        got = outs[k].download()
        if not want[k]:
            assert np.all(got == SENTINEL), "%s was not asked for" % NAMES[k]
            res.append(None)
            continue
        ld, w = lead[1 + k], per[k]
        assert np.all(got[:ld] == SENTINEL) and np.all(got[ld + S * out_stride * w:] == SENTINEL), NAMES[k]
        rows = got[ld:ld + S * out_stride * w].reshape(S, out_stride * w)
        assert np.all(rows[:, n_chunks * w:] == SENTINEL), "%s written beyond the chunks of the call" % NAMES[k]
        rows = rows[:, :n_chunks * w].copy()
        res.append(rows.reshape(S, n_chunks, n) if k == 3 else rows)
    return res


def assert_equals_model(got, want, what):
    for k in range(4):
        if got[k] is None:
            continue
        diff = np.flatnonzero(bits(got[k]).ravel() != bits(want[k]).ravel())
        assert diff.size == 0, "%s: %s differs from the model in %d places, the first at %d: %r != %r" % (
            what, NAMES[k], diff.size, diff[0], got[k].ravel()[diff[0]], np.asarray(want[k]).ravel()[diff[0]])


# ================================================================================================ against the model
@pytest.mark.parametrize("n", [32, 64, 256, 4096, 16384])
def test_edge_inputs_three_streams_three_steps(pitch, oracle, n):
    """5 chunks of the nine inputs of pitch_model.edge_inputs, three streams per call with padded strides, at step n, n / 4
    (overlap) and n + 7 (gaps; rows that start 4, 8 or 12 bytes past a 16-byte boundary).  n = 32 is a single run shorter than
    64 samples; n = 16384 is the 32768-point transform with its scratch buffer and more than 64 KB of LDS in pick."""
    sig = M.edge_inputs(n)
    names = list(sig)
    pt = pitch.Pitch(FS, n, n_streams=3, max_chunks=5)
    for si, step in enumerate((n, n // 4, n + 7)):
        span = 4 * step + n
        for g in range(3):
            group = names[3 * g:3 * g + 3]
            want = [np.stack([model(oracle, name, sig[name], n, step, 5)[k] for name in group]) for k in range(4)]
            got = run_device(pt, np.stack([sig[name][:span] for name in group]), 5, step,
                             lead=(1 + (si + g) % 3, g % 4, (g + 1) % 4, (g + 2) % 4, (g + 3) % 4), pad=(g + si, g))
            assert_equals_model(got, want, "n %d step %d %s" % (n, step, group))
    assert np.all(model(oracle, "zeros", sig["zeros"], n, n, 5)[0] == -1)
    if n == 4096:       # what the inputs are there for
        assert np.all(np.abs(model(oracle, "sine440", sig["sine440"], n, n, 5)[0] - 440.0) < 0.01)
        assert np.all(model(oracle, "sine60", sig["sine60"], n, n, 5)[0] == -1) and np.all(model(oracle, "sine60", sig["sine60"], n, n, 5)[1] > 700)


def test_slices_of_max_chunks_give_the_same_bits(pitch, oracle):
    n, step, cnt = 256, 100, 11
    span = (cnt - 1) * step + n
    rng = np.random.default_rng(5)
    x = np.stack([(M.tone(span, f0=700.0) + 0.2 * rng.uniform(-1, 1, span)), 0.5 * rng.uniform(-1, 1, span)]).astype(np.float32)
    want = [np.stack([model(oracle, ("slices", s), x[s], n, step, cnt)[k] for s in range(2)]) for k in range(4)]
    small = run_device(pitch.Pitch(FS, n, n_streams=2, max_chunks=4), x, cnt, step, lead=(1, 1, 2, 3, 1), pad=(3, 2))
    large = run_device(pitch.Pitch(FS, n, n_streams=2, max_chunks=16), x, cnt, step)
    default = run_device(pitch.Pitch(FS, n, n_streams=2), x, cnt, step)
    assert_equals_model(small, want, "max_chunks 4")
    assert_equals_model(large, want, "max_chunks 16")
    assert_equals_model(default, want, "default max_chunks")


def test_no_chunks_and_each_output_on_its_own(pitch, oracle):
    n, cnt = 64, 3
    x = M.edge_inputs(n)["tone+noise"][:cnt * n]
    want = [r[None] for r in model(oracle, "own", x, n, n, cnt)]
    pt = pitch.Pitch(FS, n)
    for k in range(4):
        got = run_device(pt, x, cnt, n, want=tuple(j == k for j in range(4)))
        assert_equals_model(got, want, "only %s" % NAMES[k])
    run_device(pt, x, cnt, n, want=(False, False, False, False))
    got = run_device(pt, x[:0], 0, n)
    assert all(g.size == 0 for g in got)
    pt.run_device(None, 0, 0)                                  # nothing to read: no input needed
    assert pt.run(np.zeros(n - 1, np.float32))[0].shape == (0,)


def test_run_host_equals_run_device(pitch, oracle):
    n, cnt = 256, 7
    sig = M.edge_inputs(n)
    for step in (n, n // 4, n + 7):
        span = (cnt - 1) * step + n
        rng = np.random.default_rng(step)
        x = np.stack([(M.tone(span, f0=900.0) + 0.3 * rng.uniform(-1, 1, span)), 0.5 * rng.uniform(-1, 1, span)]).astype(np.float32)
        pt = pitch.Pitch(FS, n, n_streams=2, max_chunks=3)
        dev = run_device(pt, x, cnt, step)
        host = pt.run(x, step=step, nsdf=True)
        assert host[0].shape == (2, cnt) and host[3].shape == (2, cnt, n)
        assert_equals_model(list(host), dev, "run_host step %d" % step)
        assert_equals_model(dev, [np.stack([model(oracle, ("host", step, s), x[s], n, step, cnt)[k] for s in range(2)]) for k in range(4)],
                            "run_device step %d" % step)
    one = pitch.Pitch(FS, n).run(sig["sine440"][:5 * n])
    assert one[0].shape == (5,)
    assert_equals_model([o[None] for o in one] + [None], [r[None] for r in model(oracle, "sine440", sig["sine440"], n, n, 5)], "one stream")


# ================================================================================================ arguments, memory
def test_bad_arguments_are_refused_and_touch_nothing(pitch):
    import ctypes as C

    import zen_amd
    n, cnt = 64, 4
    L, BAD = pitch.load(), 2
    h = C.c_void_p()
    for bad_n in (0, 16, 48, 100, 32768):
        assert L.zen_hip_pitch_create(FS, bad_n, 1, 0, C.byref(h)) == BAD
    assert L.zen_hip_pitch_create(FS, n, 0, 0, C.byref(h)) == BAD and h.value is None
    pt = pitch.Pitch(FS, n)
    x = M.edge_inputs(n)["tone"][:cnt * n]
    inp = zen_amd.DeviceBuffer.from_host(x)
    out = zen_amd.DeviceBuffer.from_host(np.full(3 * cnt + cnt * n, SENTINEL, np.float32))
    o = [out.offset(k * cnt) for k in range(4)]
    cases = [(None, inp.ptr, cnt, n, o[0], o[3], cnt),          # null handle
             (pt._h, None, cnt, n, o[0], o[3], cnt),            # null input
             (pt._h, inp.ptr, cnt, 0, o[0], o[3], cnt),         # step 0
             (pt._h, inp.ptr, cnt, n, o[0], o[3], cnt - 1),     # out_stride below the chunks of a row
             (pt._h, inp.ptr + 2, cnt, n, o[0], o[3], cnt),     # pointers that are not 4-byte aligned
             (pt._h, inp.ptr, cnt, n, o[0] + 1, o[3], cnt),
             (pt._h, inp.ptr, cnt, n, o[0], o[3] + 2, cnt)]
    before = pt.stats()
    for hh, a, c, step, p0, p3, out_stride in cases:
        for f in (L.zen_hip_pitch_run_device, L.zen_hip_pitch_run_host):
            assert f(hh, a, n * cnt, c, step, p0, o[1], o[2], p3, out_stride) == BAD
            assert L.zen_hip_pitch_last_error() != b""
    with pytest.raises(zen_amd.ZenHipError) as e:
        pitch.Pitch(FS, 3000)
    assert e.value.code == BAD
    zen_amd.synchronize()
    assert pt.stats() == before
    assert np.all(out.download() == SENTINEL) and np.array_equal(inp.download(), x)
    # the handle is still good
    assert pt.run(x)[0].shape == (cnt,) and pt.stats()["chunks"] == cnt


def test_calls_after_create_allocate_nothing(pitch):
    import zen_amd
    for n, cnt in ((4096, 9), (16384, 5)):
        x = M.edge_inputs(n)["tone+noise"][:5 * n]
        inp = zen_amd.DeviceBuffer.from_host(np.tile(x, 2)[:cnt * n])
        outs = [zen_amd.DeviceBuffer.from_host(np.full(cnt * w, SENTINEL, np.float32)) for w in (1, 1, 1, n)]
        pt = pitch.Pitch(FS, n, max_chunks=4)
        zen_amd.synchronize()
        st0, mc0 = pt.stats(), zen_amd.memcheck()
        assert st0["allocations"] == 7 and st0["device_bytes"] >= 4 * (16 + 8 + 4 + 4) * n and st0["chunks"] == 0
        for _ in range(3):
            pt.run_device(inp, cnt * n, cnt, n, *outs, out_stride=cnt)
        pt.run(x)
        zen_amd.synchronize()
        st1, mc1 = pt.stats(), zen_amd.memcheck()
        assert st1["allocations"] == st0["allocations"] and st1["device_bytes"] == st0["device_bytes"]
        assert st1["chunks"] == 3 * cnt + 5
        if mc1["redzone_bytes"]:
            assert mc1["allocations"] == mc0["allocations"] and mc1["live_allocations"] == mc0["live_allocations"]
            assert mc1["corrupt_words"] == 0


def test_profile_counts_the_launches(pitch):
    n, cnt = 256, 6
    pt = pitch.Pitch(FS, n, max_chunks=4)
    pt.profile(True)
    pt.run(M.edge_inputs(n)["tone"][:cnt * n])
    prof = pt.profile_get()
    assert list(prof) == list(pitch.KERNELS)
    for name, p in prof.items():
        assert p["launches"] == 2 and p["ms"] > 0 and p["bytes"] > 0, name       # two slices: 4 + 2 chunks
    assert all(p["launches"] == 0 for p in pt.profile_get().values())


# ================================================================================================ behind the separation
@pytest.fixture(scope="module")
def claim(pitch, oracle):
    """the 14-chunk input of the claim (tests/test_pitch_model.py): track_hpr's two columns and the model's"""
    x = M.claim_input(3.0)
    with_hpr, without = pitch.track_hpr(x, FS, 4096)
    harm = oracle.HPR(FS, 4096, 2.5, oracle.OUTPUT_HARMONIC, oracle.TIME_CAUSAL).process_stream(x)["H"]
    return x, with_hpr, without, M.track(harm, FS, 4096)[0], M.track(x, FS, 4096)[0]


def test_track_hpr_on_the_device_equals_the_model_on_the_oracles_harmonic_stream(claim):
    x, with_hpr, without, want_with, want_without = claim
    assert with_hpr.shape == without.shape == (14,)
    assert np.array_equal(bits(with_hpr), bits(want_with)), (with_hpr, want_with)
    assert np.array_equal(bits(without), bits(want_without)), (without, want_without)
    assert np.all(np.abs(with_hpr - 163.3) <= 1.0) and np.sum(without == -1) >= 8


def write_wav_float32(path, x, fs):
    """mono IEEE-float WAV: the samples reach the program bit for bit"""
    x = np.ascontiguousarray(x, "<f4")
    hdr = b"RIFF" + np.uint32(36 + x.nbytes).tobytes() + b"WAVEfmt " + np.uint32(16).tobytes()
    hdr += np.array([3, 1], "<u2").tobytes() + np.array([fs, fs * 4], "<u4").tobytes() + np.array([4, 32], "<u2").tobytes()
    hdr += b"data" + np.uint32(x.nbytes).tobytes()
    with open(path, "wb") as f:
        f.write(hdr + x.tobytes())


def test_pitch_track_program_prints_what_track_hpr_gives(claim, tmp_path):
    from zen_amd.addon_build import pitch as addon
    x, with_hpr, without, _, _ = claim
    wav = str(tmp_path / "claim.wav")
    write_wav_float32(wav, x, 44100)
    r = subprocess.run([addon.build_demo(), wav], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 14
    for c, line in enumerate(lines):
        assert line == "t: %.3f,\tpitch (+HPR): %.2f,\tpitch (-HPR): %.2f" % (c * 4096 / 44100.0, with_hpr[c], without[c]), (c, line)
