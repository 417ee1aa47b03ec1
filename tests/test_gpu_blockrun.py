"""GPU tests of the block-run library (zen_amd/blockrun): block calls of the headline configuration served by the run
kernel, through zen_amd.HPR, at tolerance 0 -- against the CPU oracle and against the base library's own path (off = 1)
-- and the engine's state after such a call: per-hop calls, copy_output, use_sse_filter and reset_buffers go on from it
as they go on from a call of the base library.

Hop 1024, S-noise (i.i.d. uniform(-1, 1)).  The library serves a call only on an engine whose buffers the base library
has already sized (zen_hip_blockrun.h), so every engine here is primed with one block call and reset; how many calls the
run kernel then served is read from zen_hip_blockrun_stats, so that no case passes on forwarded calls."""
import numpy as np
import pytest

from oracle import oracle as o

pytestmark = pytest.mark.gpu
FS, HOP, BETA = 44100.0, 1024, 2.0
P = o.OUTPUT_PERCUSSIVE
S_MAX, HOPS_MAX = 3, 3 * 37


@pytest.fixture(scope="module")
def z():
    import zen_amd
    zen_amd.init(0)
    assert zen_amd.lib.load_blockrun(), "libzen_hip_blockrun.so must load on the GPU tier"
    zen_amd.blockrun_set("min_items", 0)
    yield zen_amd
    zen_amd.blockrun_set("min_items", 4096)
    zen_amd.blockrun_set("run_len", 0)
    zen_amd.blockrun_set("off", 0)


@pytest.fixture(scope="module")
def noise():
    """three streams of S-noise and the oracle's percussive stream of each: computed once, read only"""
    x = np.random.default_rng(0).uniform(-1, 1, (S_MAX, HOPS_MAX * HOP)).astype(np.float32)
    ref = np.stack([o.HPR(FS, HOP, BETA, P, o.TIME_CAUSAL).process_stream(x[s])["P"] for s in range(S_MAX)])
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


def primed_engine(z, S, M, x):
    """an engine whose buffers the base library has sized for block calls of M hops, back in its initial state"""
    m = max(M, 2)
    eng = z.HPR(FS, HOP, BETA, z.OUTPUT_PERCUSSIVE, z.TIME_CAUSAL, True, S, m)
    d_in = z.DeviceBuffer.from_host(np.ascontiguousarray(x[:S, :m * HOP]))
    d_out = z.DeviceBuffer(S * m * HOP)
    z.blockrun_set("off", 1)
    eng.process(d_in.ptr, m, m * HOP, None, d_out.ptr, None, m * HOP)
    z.blockrun_set("off", 0)
    eng.reset_buffers()
    z.synchronize()
    return eng


def three_calls(z, x, S, M, run_len, off):
    """three consecutive block calls of M hops on S streams; returns the (S, 3 * M * HOP) output and the calls served by the run kernel"""
    n = 3 * M * HOP
    eng = primed_engine(z, S, M, x)
    d_in = z.DeviceBuffer.from_host(np.ascontiguousarray(x[:S, :n]))
    d_out = z.DeviceBuffer(S * n)
    d_out.zero()
    z.blockrun_set("run_len", run_len)
    z.blockrun_set("off", off)
    routed0 = z.blockrun_stats()[0]
    try:
        for k in range(3):
            eng.process(d_in.offset(k * M * HOP), M, n, None, d_out.offset(k * M * HOP), None, n)
        z.synchronize()
    finally:
        z.blockrun_set("off", 0)
        z.blockrun_set("run_len", 0)
    return d_out.download().reshape(S, n), z.blockrun_stats()[0] - routed0


_base = {}


@pytest.mark.parametrize("run_len", [1, 2, 5, 37, 64])
@pytest.mark.parametrize("n_hops", [1, 2, 37])
@pytest.mark.parametrize("n_streams", [1, 3])
def test_three_calls_equal_oracle_and_base(z, noise, n_streams, n_hops, run_len):
    """tail and carry cross calls; runs of one hop (every hop through the fix-up), runs that end inside a call, one run per
    stream (37) and a run length beyond the call (64)"""
    x, ref = noise
    if (n_streams, n_hops) not in _base:
        _base[(n_streams, n_hops)] = three_calls(z, x, n_streams, n_hops, 0, off=1)
    base, base_routed = _base[(n_streams, n_hops)]
    got, routed = three_calls(z, x, n_streams, n_hops, run_len, off=0)
    assert base_routed == 0 and routed == 3
    n = 3 * n_hops * HOP
    assert np.array_equal(base, ref[:n_streams, :n]), "the base path differs from the oracle"
    assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), "run kernel differs from the base path"
    assert np.array_equal(got, ref[:n_streams, :n]) and np.any(got != 0)


def test_default_partition_many_runs_equals_base_and_oracle_window(z):
    """run_len 0 as bench.py runs it, on a call of more workgroups than one per CU: 2500 hops in 768 runs of 3 or 4; every
    sample against the base path, the last 16 hops against the oracle (a causal output hop depends on input hops i-2 .. i)"""
    M, K = 2500, 16
    x = np.random.default_rng(1).uniform(-1, 1, (1, M * HOP)).astype(np.float32)
    out = {}
    for off in (1, 0):
        eng = primed_engine(z, 1, M, x)
        d_in, d_out = z.DeviceBuffer.from_host(x), z.DeviceBuffer(M * HOP)
        z.blockrun_set("off", off)
        routed0 = z.blockrun_stats()[0]
        try:
            eng.process(d_in.ptr, M, M * HOP, None, d_out.ptr, None, M * HOP)
            z.synchronize()
        finally:
            z.blockrun_set("off", 0)
        assert z.blockrun_stats()[0] - routed0 == (0 if off else 1)
        out[off] = d_out.download()
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
    want = o.HPR(FS, HOP, BETA, P, o.TIME_CAUSAL).process_stream(x[0, (M - K - 2) * HOP:])["P"][2 * HOP:]
    assert np.array_equal(out[0][(M - K) * HOP:], want) and np.any(want != 0)


def test_per_hop_calls_and_copy_output_go_on_from_a_routed_call(z, noise):
    """block call (routed) -> four process_next_hop + copy_output -> block call (routed) -> copy_output of the whole block"""
    x, ref = noise
    A, B, C = 7, 4, 6
    n = (A + B + C) * HOP
    eng = primed_engine(z, 1, A, x)
    d_in = z.DeviceBuffer.from_host(np.ascontiguousarray(x[0, :n]))
    d_out = z.DeviceBuffer(n)
    d_out.zero()
    d_blk = z.DeviceBuffer(C * HOP)
    z.blockrun_set("run_len", 3)
    routed0 = z.blockrun_stats()[0]
    try:
        eng.process(d_in.ptr, A, n, None, d_out.ptr, None, n)
        for i in range(A, A + B):
            eng.process_next_hop(d_in.offset(i * HOP))
            eng.copy_output(z.OUTPUT_PERCUSSIVE, d_out.offset(i * HOP))
        eng.process(d_in.offset((A + B) * HOP), C, n, None, d_out.offset((A + B) * HOP), None, n)
        eng.copy_output(z.OUTPUT_PERCUSSIVE, d_blk.ptr)
        z.synchronize()
    finally:
        z.blockrun_set("run_len", 0)
    assert z.blockrun_stats()[0] - routed0 == 2
    got = d_out.download()
    assert np.array_equal(got, ref[0, :n])
    assert np.array_equal(d_blk.download(), ref[0, (A + B) * HOP:n])


def test_use_sse_filter_after_a_routed_call_reads_the_kept_magnitude_rows(z, noise):
    """the box filter over time of the first hops after the switch reads the magnitude rows of the block's last frames"""
    x, _ = noise
    A, B = 9, 5
    n = (A + B) * HOP
    eng = primed_engine(z, 1, A, x)
    d_in = z.DeviceBuffer.from_host(np.ascontiguousarray(x[0, :n]))
    d_out = z.DeviceBuffer(n)
    d_out.zero()
    z.blockrun_set("run_len", 4)
    routed0 = z.blockrun_stats()[0]
    try:
        eng.process(d_in.ptr, A, n, None, d_out.ptr, None, n)
        eng.use_sse_filter()
        eng.process(d_in.offset(A * HOP), B, n, None, d_out.offset(A * HOP), None, n)
        z.synchronize()
    finally:
        z.blockrun_set("run_len", 0)
    assert z.blockrun_stats()[0] - routed0 == 1   # (the SSE call is the base library's)
    ora = o.HPR(FS, HOP, BETA, P, o.TIME_CAUSAL)
    want = ora.process_stream(x[0, :A * HOP])["P"]
    ora.use_sse_filter()
    want = np.concatenate([want, ora.process_stream(x[0, A * HOP:n])["P"]])
    assert np.array_equal(d_out.download(), want)


def test_reset_buffers_after_a_routed_call_gives_an_identical_rerun(z, noise):
    x, ref = noise
    M = 11
    eng = primed_engine(z, 3, M, x)
    d_in = z.DeviceBuffer.from_host(np.ascontiguousarray(x[:, :M * HOP]))
    outs = []
    z.blockrun_set("run_len", 4)
    routed0 = z.blockrun_stats()[0]
    try:
        for _ in range(2):
            d_out = z.DeviceBuffer(3 * M * HOP)
            d_out.zero()
            eng.process(d_in.ptr, M, M * HOP, None, d_out.ptr, None, M * HOP)
            z.synchronize()
            outs.append(d_out.download().reshape(3, -1))
            eng.reset_buffers()
    finally:
        z.blockrun_set("run_len", 0)
    assert z.blockrun_stats()[0] - routed0 == 2
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.array_equal(outs[0], ref[:, :M * HOP])


def test_output_rows_that_are_not_16_byte_aligned(z, noise):
    """the fix-up launch adds the runs' first hops 16 bytes at a time where the caller's rows allow it: here they do not"""
    x, ref = noise
    M = 13
    eng = primed_engine(z, 3, M, x)
    d_in = z.DeviceBuffer.from_host(np.ascontiguousarray(x[:, :M * HOP]))
    d_out = z.DeviceBuffer(3 * (M * HOP + 3) + 1)
    d_out.zero()
    z.blockrun_set("run_len", 3)
    routed0 = z.blockrun_stats()[0]
    try:
        eng.process(d_in.ptr, M, M * HOP, None, d_out.offset(1), None, M * HOP + 3)
        z.synchronize()
    finally:
        z.blockrun_set("run_len", 0)
    assert z.blockrun_stats()[0] - routed0 == 1
    got = d_out.download()
    for s in range(3):
        assert np.array_equal(got[1 + s * (M * HOP + 3):][:M * HOP], ref[s, :M * HOP]), s
    assert got[0] == 0 and np.all(got[1 + M * HOP:][:3] == 0)
