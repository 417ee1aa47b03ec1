"""GPU tier: libzen_hip_ragged.so (zen_amd/ragged) -- clips of unequal length in one offline call.  Tolerance 0 everywhere:
row c of a batch is compared with == against oracle.HPRIOffline.process of that clip ALONE (44.1 kHz, beta 2).  Every device
call goes through run_device below, which also checks what the call must leave alone: zeros in [lens[c], max(lens)) of each
output row, sentinels at and beyond max(lens) and in the gap up to the stride, and the input buffer (whose gaps hold NaNs: a
kernel that read beyond a clip would carry them into a result)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ragged_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
FS = M.FS
SENTINEL = 12345.0
LENS_1024 = [1, 255, 1024, 2049, 2559, 2816, 3071, 3072, 7 * 1024 + 259, 12 * 1024 + 17, 0]
LENS_256 = [1, 63, 256, 257, 767, 768, 1859, 5115, 5120, 8465]


@pytest.fixture(scope="module")
def ragged():
    """The library of this feature, built on demand (the session fixture of conftest.py builds the one it links against)."""
    import zen_amd
    from zen_amd import ragged as mod
    mod.load()
    zen_amd.init(0)
    return mod


_refs = {}


def reference(oracle, hop_h, hop_p, n, seed, soft=False, sse=False):
    """(clip, harm, perc): the clip of n samples made from `seed`, and what the oracle's HPRIOffline gives for it alone"""
    key = (hop_h, hop_p, n, seed, soft, sse)
    if key not in _refs:
        x = M.clip(n, seed)
        h, p = M.oracle_per_clip(oracle, hop_h, hop_p, [x], soft=soft, sse=sse)
        _refs[key] = (x, h[0], p[0])
    return _refs[key]


def references(oracle, hop_h, hop_p, lens, soft=False, sse=False, seeds=None):
    seeds = range(len(lens)) if seeds is None else seeds
    return [reference(oracle, hop_h, hop_p, n, s, soft, sse) for n, s in zip(lens, seeds)]


class Batch:
    """Device buffers of one call: the input matrix (NaNs wherever no clip sample is) and sentinel-filled outputs, each `lead`
    floats into its allocation so that the rows need not start on a 16-byte boundary."""

    def __init__(self, clips, stride, out_stride, lead=(0, 0, 0)):
        import zen_amd
        self.n, self.stride, self.out_stride, self.lead = len(clips), stride, out_stride, lead
        self.lens = [c.size for c in clips]
        self.in_host = np.full(lead[0] + self.n * stride + 8, np.nan, np.float32)
        for c, x in enumerate(clips):
            self.in_host[lead[0] + c * stride:lead[0] + c * stride + x.size] = x
        self.inp = zen_amd.DeviceBuffer.from_host(self.in_host)
        self.out_total = max(lead[1], lead[2]) + self.n * out_stride + 8
        self.outs = [zen_amd.DeviceBuffer.from_host(np.full(self.out_total, SENTINEL, np.float32)) for _ in range(2)]

    def args(self, harm=True, perc=True):
        return (self.inp.offset(self.lead[0]), self.lens, self.stride, self.outs[0].offset(self.lead[1]) if harm else None,
                self.outs[1].offset(self.lead[2]) if perc else None, self.out_stride)

    def check(self, refs, harm=True, perc=True):
        """after a synchronise: every row against its reference, and everything the call must not have touched"""
        mx = max(self.lens)
        assert np.array_equal(self.inp.download(), self.in_host, equal_nan=True), "the input buffer was written"
        for k, (wanted, name) in enumerate(((harm, "harmonic"), (perc, "percussive"))):
            got = self.outs[k].download()
            lead = self.lead[1 + k]
            if not wanted:
                assert np.all(got == SENTINEL), "%s was not asked for" % name
                continue
            assert np.all(got[:lead] == SENTINEL) and np.all(got[lead + self.n * self.out_stride:] == SENTINEL), name
            rows = got[lead:lead + self.n * self.out_stride].reshape(self.n, self.out_stride)
            for c, n in enumerate(self.lens):
                assert np.array_equal(rows[c, :n], refs[c][1 + k]), "%s of clip %d (%d samples) differs from the oracle" % (name, c, n)
                assert np.all(rows[c, n:mx] == 0.0) and not np.any(np.signbit(rows[c, n:mx])), (name, c, "tail is not zeros")
                assert np.all(rows[c, mx:] == SENTINEL), (name, c, "written at or beyond max(lens)")


def run_device(ragged, handle, refs, stride=None, out_stride=None, lead=(0, 0, 0), harm=True, perc=True):
    import zen_amd
    clips = [r[0] for r in refs]
    mx = max(c.size for c in clips)
    b = Batch(clips, mx if stride is None else stride, mx if out_stride is None else out_stride, lead)
    handle.process_device(*b.args(harm, perc))
    zen_amd.synchronize()
    b.check(refs, harm, perc)
    return b


# ================================================================================================ against the oracle
@pytest.mark.parametrize("variant", ("hard", "soft", "sse"))
def test_1024_256_against_the_oracle_per_clip(ragged, oracle, variant):
    """the lengths whose percussive output differs without the per-clip splice (tests/test_ragged_model.py), a clip of one
    sample, an empty clip; hard: rows that start 4, 8 and 12 bytes past a 16-byte boundary with odd strides (scalar heads and
    tails, unaligned sources), soft / sse: aligned rows"""
    soft, sse = variant == "soft", variant == "sse"
    refs = references(oracle, 1024, 256, LENS_1024, soft, sse)
    rg = ragged.Ragged(FS, 1024, 256, 2.0, 2.0, n_clips=len(LENS_1024))
    if soft:
        rg.use_soft_mask()
    if sse:
        rg.use_sse_filter()
    mx = max(LENS_1024)
    if variant == "hard":
        run_device(ragged, rg, refs, stride=mx + 5, out_stride=mx + 3, lead=(1, 2, 3))
    else:
        run_device(ragged, rg, refs, stride=mx + 12, out_stride=mx + 4)


def test_256_64_clips_shorter_than_the_lag(ragged, oracle):
    """lag_h = 11: clips shorter than lag_h hops, whose padded pass-1 length is below twice the shift"""
    refs = references(oracle, 256, 64, LENS_256)
    rg = ragged.Ragged(FS, 256, 64, 2.0, 2.0, n_clips=len(LENS_256))
    lag_h = oracle.HPR(FS, 256, 2.0, oracle.OUTPUT_PERCUSSIVE, oracle.TIME_ANTICAUSAL).lag
    assert lag_h == 11 and M.padded(LENS_256[0], 256, lag_h) < 2 * lag_h * 256
    run_device(ragged, rg, refs, out_stride=max(LENS_256) + 1, lead=(0, 1, 0))


def test_one_output_only(ragged, oracle):
    lens = [2049, 3072, 0, 1024]
    refs = references(oracle, 1024, 256, lens, seeds=(3, 7, 10, 2))
    rg = ragged.Ragged(FS, 1024, 256, 2.0, 2.0, n_clips=4)
    run_device(ragged, rg, refs, harm=False)
    run_device(ragged, rg, refs, perc=False)


# ================================================================================================ against the equal-length call
def test_equal_lengths_equal_the_batch_call_of_the_engine(ragged):
    import zen_amd
    n, rows = 5000, 3
    clips = [M.clip(n, 20 + c) for c in range(rows)]
    b = Batch(clips, n + 4, n + 4)
    rg = ragged.Ragged(FS, 1024, 256, 2.0, 2.0, n_clips=rows)
    rg.process_device(*b.args())
    eq = zen_amd.HPRIOffline(FS, 1024, 256, 2.0, 2.0, n_clips=rows)
    want = [zen_amd.DeviceBuffer.from_host(np.full(rows * (n + 4), SENTINEL, np.float32)) for _ in range(2)]
    eq.process_device(b.inp.ptr, n, n + 4, harm=want[0].ptr, perc=want[1].ptr, out_stride=n + 4)
    zen_amd.synchronize()
    for k in range(2):
        got = b.outs[k].download()[:rows * (n + 4)]
        assert np.array_equal(got, want[k].download()), ("harmonic", "percussive")[k]
        assert np.any(got.reshape(rows, n + 4)[:, :n] != 0)


# ================================================================================================ state, queueing
def test_second_call_with_other_lengths_equals_a_fresh_handle(ragged, oracle):
    """the engines' state, the cached scratch (which only grows) and the table slots carry nothing from call to call"""
    first = references(oracle, 1024, 256, [7 * 1024 + 259, 2816, 3071], seeds=(8, 5, 6))
    second = references(oracle, 1024, 256, [2049, 3072, 1024], seeds=(3, 7, 2))
    rg = ragged.Ragged(FS, 1024, 256, 2.0, 2.0, n_clips=3)
    run_device(ragged, rg, first)
    reused = run_device(ragged, rg, second)
    fresh = run_device(ragged, ragged.Ragged(FS, 1024, 256, 2.0, 2.0, n_clips=3), second)
    for k in range(2):
        assert np.array_equal(reused.outs[k].download(), fresh.outs[k].download())


def test_calls_queued_back_to_back_keep_their_own_lengths(ragged, oracle):
    """no synchronise between the calls: the second call's table must not reach the first call's kernels.  More calls than
    the handle has table slots, alternating between two sets of lengths."""
    import zen_amd
    sets = [references(oracle, 1024, 256, [7 * 1024 + 259, 2816, 3071], seeds=(8, 5, 6)),
            references(oracle, 1024, 256, [2049, 3072, 1024], seeds=(3, 7, 2))]
    rg = ragged.Ragged(FS, 1024, 256, 2.0, 2.0, n_clips=3)
    run_device(ragged, rg, sets[0])             # scratch at its final size: the queued calls below allocate nothing
    batches = []
    for i in range(6):
        refs = sets[i % 2]
        mx = max(r[0].size for r in refs)
        batches.append((Batch([r[0] for r in refs], mx, mx), refs))
    for b, _ in batches:
        rg.process_device(*b.args())
    zen_amd.synchronize()
    for b, refs in batches:
        b.check(refs)


# ================================================================================================ host call
def test_host_call_with_separate_buffers_equals_the_device_call(ragged, oracle):
    lens = [2559, 0, 12 * 1024 + 17, 1, 3072]
    refs = references(oracle, 1024, 256, lens, seeds=(4, 10, 9, 0, 7))
    rg = ragged.Ragged(FS, 1024, 256, 2.0, 2.0, n_clips=len(lens))
    dev = run_device(ragged, rg, refs)
    harm, perc = rg.process([r[0] for r in refs])
    mx = max(lens)
    for k, outs in enumerate((harm, perc)):
        rows = dev.outs[k].download()[:len(lens) * mx].reshape(len(lens), mx)
        for c, n in enumerate(lens):
            assert outs[c].size == n and np.array_equal(outs[c], rows[c, :n]), (k, c)
            assert np.array_equal(outs[c], refs[c][1 + k])
    only_perc = rg.process([r[0] for r in refs], want=(False, True))
    assert only_perc[0] is None and all(np.array_equal(a, b) for a, b in zip(only_perc[1], perc))


# ================================================================================================ arguments
def test_bad_arguments_touch_nothing(ragged, oracle):
    import zen_amd
    lens = [2049, 1024]
    refs = references(oracle, 1024, 256, lens, seeds=(3, 2))
    rg = ragged.Ragged(FS, 1024, 256, 2.0, 2.0, n_clips=2)
    b = Batch([r[0] for r in refs], 2049, 2049)
    L, E_BAD_ARG = ragged.load(), 2
    inp, _, _, harm, perc, _ = b.args()
    lens_c = (C.c_size_t * 2)(*lens)
    cases = [(None, lens_c, 2049, 2049), (inp, None, 2049, 2049), (inp, lens_c, 2048, 2049), (inp, lens_c, 2049, 2048)]
    for a, ln, stride, out_stride in cases:
        assert L.zen_hip_ragged_process_device(rg._h, a, ln, stride, harm, perc, out_stride) == E_BAD_ARG
        assert L.zen_hip_ragged_last_error() != b""
    assert L.zen_hip_ragged_process_device(None, inp, lens_c, 2049, harm, perc, 2049) == E_BAD_ARG
    with pytest.raises(zen_amd.ZenHipError):
        rg.process_device(inp, lens, 2048, harm, perc, 2049)
    with pytest.raises(zen_amd.ZgException):
        ragged.Ragged(FS, 1024, 768, 2.0, 2.0, n_clips=2)
    # all lengths zero: OK, and nothing is written (a NULL input stays an error)
    zeros = (C.c_size_t * 2)(0, 0)
    assert L.zen_hip_ragged_process_device(rg._h, inp, zeros, 0, harm, perc, 0) == 0
    assert L.zen_hip_ragged_process_device(rg._h, None, zeros, 0, harm, perc, 0) == E_BAD_ARG
    zen_amd.synchronize()
    assert np.array_equal(b.inp.download(), b.in_host, equal_nan=True)
    for k in range(2):
        assert np.all(b.outs[k].download() == SENTINEL)
    rg.process_device(*b.args())                # the handle is still good
    zen_amd.synchronize()
    b.check(refs)


# ================================================================================================ profiling
ENGINE_CLASSES = ("stft", "freq_filter", "time_filter", "istft", "finalize", "rt_fused")


def test_profile_counts_the_launches_and_leaves_the_outputs_alone(ragged, oracle):
    """one device call with both outputs is one pack, one splice and one trim; the counters are drained by profile_get and
    stay at zero while profiling is off; the rows written under profiling are those written without it"""
    refs = references(oracle, 256, 64, [300, 1])
    rg = ragged.Ragged(FS, 256, 64, 2.0, 2.0, n_clips=2)
    plain = run_device(ragged, rg, refs)
    rg.profile(True)
    timed = run_device(ragged, rg, refs)
    prof = rg.profile_get()
    print(prof)
    assert list(prof) == list(ragged.KERNELS)
    for name, p in prof.items():
        assert p["launches"] == 1 and p["bytes"] > 0 and p["ms"] >= 0, name
    eng = rg.profile_get_engine()
    assert list(eng) == ["pass1", "pass2"] and all(tuple(v) == ENGINE_CLASSES for v in eng.values())
    ms, n = (C.c_double * 6)(), (C.c_ulonglong * 6)()
    for ps in (0, 3):
        assert ragged.load().zen_hip_ragged_profile_get_engine(rg._h, ps, ms, n) == 2
    zero = {"ms": 0.0, "bytes": 0, "launches": 0}
    assert all(p == zero for p in rg.profile_get().values())
    rg.profile(False)
    off = run_device(ragged, rg, refs)
    assert all(p == zero for p in rg.profile_get().values())
    for k in range(2):
        want = plain.outs[k].download()
        assert np.array_equal(timed.outs[k].download(), want) and np.array_equal(off.outs[k].download(), want)
