"""GPU tier: libzen_hip_live.so (zen_amd/live) -- the two-pass separation as a stream.  Tolerance 0 everywhere: what the pushes
and finish hand out, put end to end, is compared with == against oracle.HPRIOffline.process of the WHOLE clip (44.1 kHz,
beta 2), and dry against the input.  Every device session goes through stream_device below: no synchronise between its
calls (they are queued back to back), the count every call reports against zen_hip_live_produces / _pending asked just
before and against the closed form, NaNs around the input rows (a kernel that read beyond a push would carry them into a
result) and sentinels around the output rows."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import live_model as M  # noqa: E402
import ragged_model as R  # noqa: E402

pytestmark = pytest.mark.gpu
FS = M.FS
SENTINEL = 12345.0
CASES = M.cases()


@pytest.fixture(scope="module")
def live():
    """The library of this feature, built on demand (the session fixture of conftest.py builds the one it links against)."""
    import zen_amd
    from zen_amd import live as mod
    mod.load()
    zen_amd.init(0)
    return mod


_refs = {}


def reference(oracle, hop_h, hop_p, n, soft=False, sse=False, seed=0):
    """(clip, harm, perc): the clip of n samples made from `seed`, and what the oracle's HPRIOffline gives for the whole of it"""
    key = (hop_h, hop_p, n, soft, sse, seed)
    if key not in _refs:
        x = M.clip(n, seed)
        h, p = R.oracle_per_clip(oracle, hop_h, hop_p, [x], soft=soft, sse=sse)
        _refs[key] = (x, h[0], p[0])
    return _refs[key]


def stream_device(lv, x, pushes, lead=(0, 0, 0, 0), pad=(0, 0), want=(True, True, True), finish=True):
    """x: (n,) or (n_streams, n).  The clip through push_device in pieces of `pushes` samples and finish_device, every call's
    rows behind the previous call's in one buffer per output; `lead` floats in front of the input / harm / perc / dry rows and
    `pad` floats between the rows (input, outputs).  Returns ([harm, perc, dry] as (n_streams, delivered) arrays or None, counts)."""
    import zen_amd
    x = np.asarray(x, np.float32).reshape(lv.n_streams, -1)
    S, n = x.shape
    in_stride, out_stride = n + pad[0], n + pad[1]
    in_host = np.full(lead[0] + S * in_stride + 8, np.nan, np.float32)
    for s in range(S):
        in_host[lead[0] + s * in_stride:lead[0] + s * in_stride + n] = x[s]
    inp = zen_amd.DeviceBuffer.from_host(in_host)
    outs = [zen_amd.DeviceBuffer.from_host(np.full(lead[1 + k] + S * out_stride + 8, SENTINEL, np.float32)) for k in range(3)]

    def out_ptrs(tot):
        return [outs[k].offset(lead[1 + k] + tot) if want[k] else None for k in range(3)]
    at = tot = 0
    counts = []
    for m in pushes:
        expect = lv.produces(m)
        assert expect == M.delivered_after(at + m, lv.hop_h, lv.latency) - tot
        got = lv.push_device(inp.offset(lead[0] + at), m, in_stride, *out_ptrs(tot), out_stride=out_stride)
        assert got == expect, "push_device reports %d samples, produces() said %d" % (got, expect)
        at, tot = at + m, tot + got
        counts.append(got)
        assert lv.pending() == at - tot and lv.stats()["pushed"] == at and lv.stats()["delivered"] == tot
    if finish:
        assert at == n
        expect = lv.pending()
        got = lv.finish_device(*out_ptrs(tot), out_stride=out_stride)
        assert got == expect == n - tot
        assert lv.pending() == 0 and lv.stats()["pushed"] == 0
        tot += got
        counts.append(got)
    zen_amd.synchronize()
    assert np.array_equal(inp.download(), in_host, equal_nan=True), "the input buffer was written"
    res = []
    for k in range(3):
        got = outs[k].download()
        if not want[k]:
            assert np.all(got == SENTINEL), "output %d was not asked for" % k
            res.append(None)
            continue
        ld = lead[1 + k]
        assert np.all(got[:ld] == SENTINEL) and np.all(got[ld + S * out_stride:] == SENTINEL), k
        rows = got[ld:ld + S * out_stride].reshape(S, out_stride)
        assert np.all(rows[:, tot:] == SENTINEL), "output %d written at or beyond what the calls reported" % k
        res.append(rows[:, :tot].copy())
    return res, counts


# ================================================================================================ against the oracle
@pytest.mark.parametrize("idx", range(len(CASES)), ids=[M.case_id(c) for c in CASES])
def test_core_cases_against_the_oracle_on_the_whole_clip(live, oracle, idx):
    """the 36 cases of the CPU tier through push_device / finish_device; rows that start 0..12 bytes past a 16-byte boundary
    (scalar heads and tails, unaligned sources), sessions sized for pushes of hop_h (larger pushes run in slices), of
    2 * hop_h + 17 and of 3 * hop_h"""
    hop_h, hop_p, n, pushes, soft, sse = CASES[idx]
    x, rh, rp = reference(oracle, hop_h, hop_p, n, soft, sse)
    lv = live.Live(FS, hop_h, hop_p, 2.0, 2.0, max_push=(hop_h, 2 * hop_h + 17, 3 * hop_h)[idx % 3])
    if soft:
        lv.use_soft_mask()
    if sse:
        lv.use_sse_filter()
    (harm, perc, dry), counts = stream_device(lv, x, pushes, lead=(idx % 4, (idx + 1) % 4, (idx + 2) % 4, (idx + 3) % 4), pad=(idx % 3, 0))
    assert harm.shape == (1, n)
    assert np.array_equal(harm[0], rh), "harmonic differs from the oracle"
    assert np.array_equal(perc[0], rp), "percussive differs from the oracle"
    assert np.array_equal(dry[0], x), "dry is not the input"
    assert counts[-1] <= lv.latency + hop_h


def test_default_geometry_4096_256(live, oracle):
    """lag_h = 1: pushes of exactly hop_h deliver nothing until the latency has gone by and hop_h per call from then on"""
    n = 5 * 4096 + 100
    x, rh, rp = reference(oracle, 4096, 256, n)
    lv = live.Live(FS, 4096, 256, 2.0, 2.0, max_push=4096)
    assert lv.latency == 4096 + 2816
    (harm, perc, dry), counts = stream_device(lv, x, M.fixed_pushes(n, 4096))
    assert np.array_equal(harm[0], rh) and np.array_equal(perc[0], rp) and np.array_equal(dry[0], x)
    assert counts == [0, 4096 - 2816, 4096, 4096, 4096, 0, n - 4 * 4096 + 2816]


def test_pushes_of_hop_h_deliver_hop_h_once_the_latency_has_gone_by(live, oracle):
    n = 12 * 1024
    x, rh, rp = reference(oracle, 1024, 256, n)
    lv = live.Live(FS, 1024, 256, 2.0, 2.0)
    assert lv.latency == 5888
    (harm, perc, dry), counts = stream_device(lv, x, [1024] * 12)
    assert counts[:5] == [0] * 5 and counts[5] == 6 * 1024 - 5888 and counts[6:12] == [1024] * 6 and counts[12] == 5888
    assert np.array_equal(harm[0], rh) and np.array_equal(perc[0], rp) and np.array_equal(dry[0], x)


def test_two_streams_odd_strides_unaligned_rows(live, oracle):
    n = 7 * 1024 + 259
    a, b = reference(oracle, 1024, 256, n, seed=1), reference(oracle, 1024, 256, n, seed=2)
    lv = live.Live(FS, 1024, 256, 2.0, 2.0, n_streams=2, max_push=1500)
    x = np.stack([a[0], b[0]])
    (harm, perc, dry), _ = stream_device(lv, x, M.random_pushes(n, 1024, 5), lead=(1, 1, 1, 1), pad=(3, 5))
    for s, ref in enumerate((a, b)):
        assert np.array_equal(harm[s], ref[1]) and np.array_equal(perc[s], ref[2]) and np.array_equal(dry[s], ref[0]), s
    assert not np.array_equal(perc[0], perc[1])


def test_outputs_that_are_not_asked_for(live, oracle):
    n = 5123
    x, rh, rp = reference(oracle, 256, 64, n)
    lv = live.Live(FS, 256, 64, 2.0, 2.0, max_push=512)
    for want in ((True, False, False), (False, True, False), (False, False, True), (False, False, False)):
        res, _ = stream_device(lv, x, M.fixed_pushes(n, 300), want=want)
        for got, ref in zip(res, (rh, rp, x)):
            assert got is None or np.array_equal(got[0], ref)


def test_values_at_and_beyond_produced_survive_every_call(live, oracle):
    """every call into fresh sentinel-filled rows, looked at before the next one"""
    import zen_amd
    n = 7 * 1024 + 259
    refs = [reference(oracle, 1024, 256, n, seed=s) for s in (1, 2)]
    x = np.stack([r[0] for r in refs])
    inp = zen_amd.DeviceBuffer.from_host(x)
    lv = live.Live(FS, 1024, 256, 2.0, 2.0, n_streams=2, max_push=1024)
    stride = lv.latency + 1024 + 8          # (finish hands out fewer than latency + hop_h samples)
    got = [[], [], []]
    at = 0
    for m in M.random_pushes(n, 1024, 9) + [None]:
        outs = [zen_amd.DeviceBuffer.from_host(np.full(1 + 2 * stride, SENTINEL, np.float32)) for _ in range(3)]
        ptrs = [o.offset(1) for o in outs]
        cnt = lv.finish_device(*ptrs, out_stride=stride) if m is None else lv.push_device(inp.offset(at), m, n, *ptrs, out_stride=stride)
        at += m or 0
        for k in range(3):
            host = outs[k].download()
            rows = host[1:].reshape(2, stride)
            assert host[0] == SENTINEL and np.all(rows[:, cnt:] == SENTINEL), (k, m, cnt)
            got[k].append(rows[:, :cnt].copy())
    for k in range(3):
        whole = np.concatenate(got[k], axis=1)
        for s in range(2):
            assert np.array_equal(whole[s], (refs[s][1], refs[s][2], refs[s][0])[k]), (k, s)


def test_six_pushes_and_finish_queued_without_a_synchronise(live, oracle):
    n = 7 * 1024 + 259
    x, rh, rp = reference(oracle, 1024, 256, n, seed=1)
    lv = live.Live(FS, 1024, 256, 2.0, 2.0, max_push=2048)
    pushes = [1024, 2048, 1, 2047, 1500, n - 6620]
    (harm, perc, dry), counts = stream_device(lv, x, pushes)       # (stream_device synchronises once, after finish)
    assert len(counts) == 7
    assert np.array_equal(harm[0], rh) and np.array_equal(perc[0], rp) and np.array_equal(dry[0], x)


# ================================================================================================ host calls, the offline call
def test_host_calls_equal_the_device_calls(live, oracle):
    n = 7 * 1024 + 259
    refs = [reference(oracle, 1024, 256, n, seed=s) for s in (1, 2)]
    x = np.stack([r[0] for r in refs])
    pushes = M.random_pushes(n, 1024, 5)
    dev, counts = stream_device(live.Live(FS, 1024, 256, 2.0, 2.0, n_streams=2, max_push=1500), x, pushes)
    lv = live.Live(FS, 1024, 256, 2.0, 2.0, n_streams=2, max_push=1500)
    parts, at = [], 0
    for m in pushes:
        parts.append(lv.push(x[:, at:at + m]))
        at += m
    parts.append(lv.finish())
    assert [p[0].shape[1] for p in parts] == counts
    for k in range(3):
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), dev[k]), k
    # one stream, one output
    one = live.Live(FS, 1024, 256, 2.0, 2.0)
    h, p, d = one.push(x[0], want=(False, True, False))
    assert h is None and d is None and p.shape == (n - n % 1024 - 5888,)
    rest = one.finish(want=(False, True, False))[1]
    assert np.array_equal(np.concatenate([p, rest]), refs[0][2])


def test_one_push_of_everything_equals_the_offline_device_call(live):
    import zen_amd
    n = 20000
    x = M.clip(n, 4)
    lv = live.Live(FS, 1024, 256, 2.0, 2.0, max_push=4096)
    (harm, perc, dry), counts = stream_device(lv, x, [n])
    assert counts == [n - n % 1024 - 5888, n % 1024 + 5888]
    inp = zen_amd.DeviceBuffer.from_host(x)
    want = [zen_amd.DeviceBuffer.from_host(np.full(n, SENTINEL, np.float32)) for _ in range(2)]
    zen_amd.HPRIOffline(FS, 1024, 256, 2.0, 2.0, n_clips=1).process_device(inp.ptr, n, n, harm=want[0].ptr, perc=want[1].ptr)
    zen_amd.synchronize()
    assert np.array_equal(harm[0], want[0].download()) and np.array_equal(perc[0], want[1].download())
    assert np.array_equal(dry[0], x) and np.any(perc != 0)


# ================================================================================================ state
def test_reset_in_mid_stream_and_a_second_stream_after_finish_equal_a_fresh_handle(live, oracle):
    n = 5123
    x, rh, rp = reference(oracle, 256, 64, n)
    other = M.clip(3000, 9)
    lv = live.Live(FS, 256, 64, 2.0, 2.0, max_push=700)
    stream_device(lv, other, M.fixed_pushes(3000, 700))                     # a whole stream first
    second, _ = stream_device(lv, x, M.fixed_pushes(n, 300))
    stream_device(lv, other, [700, 700, 700, 1], finish=False)              # half a stream, dropped
    assert lv.pending() > 0
    lv.reset()
    assert lv.pending() == 0 and lv.produces(0) == 0
    third, _ = stream_device(lv, x, M.fixed_pushes(n, 300))
    fresh, _ = stream_device(live.Live(FS, 256, 64, 2.0, 2.0, max_push=700), x, M.fixed_pushes(n, 300))
    for k, ref in enumerate((rh, rp, x)):
        assert np.array_equal(fresh[k][0], ref), k
        assert np.array_equal(second[k], fresh[k]) and np.array_equal(third[k], fresh[k]), k


def test_steady_state_allocates_nothing(live):
    import zen_amd
    hop = 1024
    x = M.clip(53 * hop, 6)
    inp = zen_amd.DeviceBuffer.from_host(x)
    outs = [zen_amd.DeviceBuffer.from_host(np.full(6912, SENTINEL, np.float32)) for _ in range(3)]      # (finish: latency + hop_h)
    lv = live.Live(FS, hop, 256, 2.0, 2.0, max_push=hop)
    ptrs = [o.ptr for o in outs]
    for i in range(3):
        lv.push_device(inp.offset(i * hop), hop, hop, *ptrs, out_stride=hop)
    zen_amd.synchronize()
    st0, mc0 = lv.stats(), zen_amd.memcheck()
    assert st0["allocations"] > 0 and st0["device_bytes"] > 0
    for i in range(3, 53):
        lv.push_device(inp.offset(i * hop), hop, hop, *ptrs, out_stride=hop)
    got = lv.finish_device(*ptrs, out_stride=6912)
    assert got == 5888
    zen_amd.synchronize()
    st1, mc1 = lv.stats(), zen_amd.memcheck()
    assert st1["allocations"] == st0["allocations"] and st1["device_bytes"] == st0["device_bytes"]
    if mc1["redzone_bytes"]:
        assert mc1["allocations"] == mc0["allocations"] and mc1["live_allocations"] == mc0["live_allocations"]
        assert mc1["corrupt_words"] == 0


# ================================================================================================ arguments
def test_bad_arguments_are_refused_and_touch_nothing(live, oracle):
    import zen_amd
    n = 5123
    x, rh, rp = reference(oracle, 256, 64, n)
    lv = live.Live(FS, 256, 64, 2.0, 2.0, max_push=512)
    L, BAD, UNSUPPORTED = live.load(), 2, 5
    lat = lv.latency
    m = (lat // 256 + 2) * 256                                  # a push of whole blocks that delivers cnt samples
    cnt = m - lat
    assert 0 < cnt < n and lv.produces(m) == cnt
    in_host = np.concatenate([x, np.zeros(m, np.float32)])      # (a refused push reads nothing; room for it all the same)
    inp = zen_amd.DeviceBuffer.from_host(in_host)
    out = zen_amd.DeviceBuffer.from_host(np.full(3 * n, SENTINEL, np.float32))
    o = [out.offset(k * n) for k in range(3)]
    got = C.c_size_t(77)
    cases = [(None, inp.ptr, m, m, o[0], cnt),                  # null handle
             (lv._h, None, m, m, o[0], cnt),                    # null input
             (lv._h, inp.ptr, m, m - 1, o[0], cnt),             # in_stride below the push
             (lv._h, inp.ptr, m, m, o[0], cnt - 1),             # out_stride below what the push delivers
             (lv._h, inp.ptr + 2, m, m, o[0], cnt),             # pointers that are not 4-byte aligned
             (lv._h, inp.ptr, m, m, o[0] + 1, cnt)]
    for h, a, mm, in_stride, harm, out_stride in cases:
        assert L.zen_hip_live_push_device(h, a, mm, in_stride, harm, o[1], o[2], out_stride, C.byref(got)) == BAD
        assert L.zen_hip_live_last_error() != b"" and got.value == 77
    beyond = live.max_samples(256, 64) + 1
    assert beyond == (1 << 24) * 64
    assert L.zen_hip_live_push_device(lv._h, inp.ptr, beyond, beyond, o[0], o[1], o[2], beyond, C.byref(got)) == UNSUPPORTED
    assert L.zen_hip_live_finish_device(None, o[0], o[1], o[2], n, C.byref(got)) == BAD
    assert lv.pending() == 0 and lv.stats()["pushed"] == 0
    with pytest.raises(zen_amd.ZgException):
        live.Live(FS, 1024, 768, 2.0, 2.0)
    # the filter and the masks are chosen before the stream begins
    lv.use_soft_mask()
    lv.push_device(inp.ptr, 100, 100)
    for f in (lv.use_soft_mask, lv.use_sse_filter):
        with pytest.raises(zen_amd.ZenHipError) as e:
            f()
        assert e.value.code == BAD
    lv.reset()
    zen_amd.synchronize()
    assert np.all(out.download() == SENTINEL) and np.array_equal(inp.download(), in_host)
    # the handle is still good (soft masks now)
    x, rh, rp = reference(oracle, 256, 64, n, soft=True)
    (harm, perc, dry), _ = stream_device(lv, x, M.fixed_pushes(n, 512))
    assert np.array_equal(harm[0], rh) and np.array_equal(perc[0], rp) and np.array_equal(dry[0], x)


# ================================================================================================ past 2^24
def test_past_two_to_the_24_the_stale_branches(live):
    """(1024, 256), n = 2^24 + 1025: (float)n = n - 1, both padders ask for one block fewer than the true ceiling
    (tests/test_live_model.py) and the last sample of each output comes from the stale branch of the end mapping.  One-second
    pushes; compared with zen_hip_hpri_process_device on the same samples up to the last 8192, and there with the oracle:
    the offline device call gives another LAST sample of each output (it does not take the stale branches), the oracle decides
    (DESIGN.md section 12).  tests/golden/live_past_2p24.npz holds the last 8192 samples of oracle.HPRIOffline.process of
    this input (a few minutes on one thread), and its last 16 input samples to tie the seed to the fixture."""
    import zen_amd
    gold = np.load(os.path.join(HERE, "golden", "live_past_2p24.npz"))
    n = (1 << 24) + 1025
    assert int(gold["n"]) == n and int(gold["seed"]) == 2024
    rng = np.random.default_rng(2024)
    x = (0.25 * rng.uniform(-1, 1, n)).astype(np.float32)
    t = np.arange(n, dtype=np.float64) / FS
    x += (0.3 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32)
    x[::44100 // 3] += 0.7
    assert np.array_equal(x[-16:], gold["input_tail"]), "the input made from the seed is not the fixture's"
    inp = zen_amd.DeviceBuffer.from_host(x)
    outs = [zen_amd.DeviceBuffer.from_host(np.full(n + 4, SENTINEL, np.float32)) for _ in range(3)]
    lv = live.Live(FS, 1024, 256, 2.0, 2.0, max_push=44100)
    at = tot = 0
    while at < n:
        m = min(44100, n - at)
        tot += lv.push_device(inp.offset(at), m, n, *(o.offset(tot) for o in outs), out_stride=n)
        at += m
    assert tot == n // 1024 * 1024 - 5888
    tot += lv.finish_device(*(o.offset(tot) for o in outs), out_stride=n)
    assert tot == n
    want = [zen_amd.DeviceBuffer.from_host(np.full(n + 4, SENTINEL, np.float32)) for _ in range(2)]
    zen_amd.HPRIOffline(FS, 1024, 256, 2.0, 2.0, n_clips=1).process_device(inp.ptr, n, n, harm=want[0].ptr, perc=want[1].ptr)
    zen_amd.synchronize()
    got = [o.download() for o in outs]
    assert np.array_equal(got[2][:n], x), "dry is not the input"
    for k, name in enumerate(("harm", "perc")):
        w = want[k].download()
        assert np.all(got[k][n:] == SENTINEL) and np.all(w[n:] == SENTINEL)
        diff = np.flatnonzero(got[k][:n - 8192] != w[:n - 8192])
        assert diff.size == 0, "%s: %d samples differ from the offline call, the first at %d of %d" % (name, diff.size, diff[0], n)
        diff = np.flatnonzero(got[k][n - 8192:n] != gold[name])
        print("%s: %d of the last 8192 samples differ from the oracle%s; the offline device call: %d" % (
            name, diff.size, (", the first at %d" % (n - 8192 + diff[0])) if diff.size else "", int(np.sum(w[n - 8192:n] != gold[name]))))
        assert diff.size == 0, "%s: %d of the last 8192 samples differ from the oracle, the first at %d of %d" % (
            name, diff.size, n - 8192 + diff[0], n)


# ================================================================================================ profiling
ENGINE_CLASSES = ("stft", "freq_filter", "time_filter", "istft", "finalize", "rt_fused")


def test_profile_counts_the_launches_and_leaves_the_outputs_alone(live, oracle):
    """pushes of 100 / 256 / 156 samples and finish at (256, 64) are four slices: four feeds; a mid wherever pass 1 ran (not in
    the first push, whose 100 samples stay in the carry); one out, in finish (the latency of 5760 samples is beyond the clip).
    The counters are drained by profile_get and stay at zero while profiling is off; the rows handed out under profiling are
    those handed out without it"""
    x, rh, rp = reference(oracle, 256, 64, 512)
    lv = live.Live(FS, 256, 64, 2.0, 2.0, max_push=256)
    assert lv.latency == 5760
    pushes = [100, 256, 156]
    plain, _ = stream_device(lv, x, pushes)
    lv.profile(True)
    timed, _ = stream_device(lv, x, pushes)
    prof = lv.profile_get()
    print(prof)
    assert list(prof) == list(live.KERNELS)
    assert [p["launches"] for p in prof.values()] == [4, 3, 1]
    for name, p in prof.items():
        assert p["bytes"] > 0 and p["ms"] >= 0, name
    eng = lv.profile_get_engine()
    assert list(eng) == ["pass1", "pass2"] and all(tuple(v) == ENGINE_CLASSES for v in eng.values())
    ms, n = (C.c_double * 6)(), (C.c_ulonglong * 6)()
    for ps in (0, 3):
        assert live.load().zen_hip_live_profile_get_engine(lv._h, ps, ms, n) == 2
    zero = {"ms": 0.0, "bytes": 0, "launches": 0}
    assert all(p == zero for p in lv.profile_get().values())
    lv.profile(False)
    off, _ = stream_device(lv, x, pushes)
    assert all(p == zero for p in lv.profile_get().values())
    for k, want in enumerate((rh, rp, x)):
        assert np.array_equal(plain[k][0], want)
        assert np.array_equal(timed[k], plain[k]) and np.array_equal(off[k], plain[k])
