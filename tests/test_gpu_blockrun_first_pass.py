"""GPU tests of the run kernel's first analysis pass (zen_amd/blockrun/blockrun_first_pass.h) and of the magnitude image
without its unread mirrored columns (blockrun_kernel.hip FwdOut): routed block calls at tolerance 0, against the CPU oracle
and bit for bit against the base library's own path (off = 1).

Settings as tests/test_gpu_blockrun.py: hop 1024, min_items 0, every engine primed with one block call of the base library
and reset, the calls the run kernel served read from zen_hip_blockrun_stats.

The S-noise seed is chosen so that, in every tested call, the percussive mask is set in at least one and clear in at least
one bin of 2041 .. 2048 (the rows' middle: medians over the mirrored columns 2049 .. 2071) and of 4073 .. 4095 (the rows' end:
medians over the mirrored columns 4050 .. 4095 and the border replica): a small float64 model of the row checks that before
anything runs on the GPU, so a wrong column there flips a mask of the call."""
import numpy as np
import pytest

from oracle import oracle as o

pytestmark = pytest.mark.gpu
FS, HOP, BETA, NFFT, TAPS = 44100.0, 1024, 2.0, 4096, 47
P = o.OUTPUT_PERCUSSIVE
S_MAX, HOPS_MAX, SEED = 3, 3 * 9, 4
MID_BINS, END_BINS = np.arange(2041, 2049), np.arange(4073, 4096)


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


def oracle_streams(x):
    ref = np.stack([o.HPR(FS, HOP, BETA, P, o.TIME_CAUSAL).process_stream(x[s])["P"] for s in range(x.shape[0])])
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


@pytest.fixture(scope="module")
def noise():
    """three streams of S-noise and the oracle's percussive stream of each: computed once, read only"""
    return oracle_streams(np.random.default_rng(SEED).uniform(-1, 1, (S_MAX, HOPS_MAX * HOP)).astype(np.float32))


def model_masks(prev, cur):
    """percussive hard mask of one causal frame at the bins MID_BINS and END_BINS: float64 magnitudes of the zero-padded
    windowed frame, brute-force 47-tap median over frequency with replicate border, H = |S| of the same row"""
    i = np.arange(2 * HOP, dtype=np.float32)
    w = np.sqrt(np.float32(0.5) * (np.float32(1) - np.cos(np.float32(2) * np.float32(3.14159265359) * i / np.float32(2 * HOP))))
    half = np.abs(np.fft.rfft(np.concatenate([prev, cur]).astype(np.float64) * w.astype(np.float64), NFFT))
    mag = np.concatenate([half, half[-2:0:-1]])
    pad = np.concatenate([np.full(TAPS // 2, mag[0]), mag, np.full(TAPS // 2, mag[-1])])
    bins = np.concatenate([MID_BINS, END_BINS])
    med = np.array([np.median(pad[k:k + TAPS]) for k in bins])
    mask = med / (mag[bins] + np.finfo(np.float32).eps) >= BETA
    return mask[:len(MID_BINS)], mask[len(MID_BINS):]


def assert_masks_flip_in_every_call(x, S, M):
    for c in range(3):
        mid, end = [], []
        for s in range(S):
            for f in range(c * M, (c + 1) * M):
                prev = x[s, (f - 1) * HOP:f * HOP] if f > 0 else np.zeros(HOP, np.float32)
                a, b = model_masks(prev, x[s, f * HOP:(f + 1) * HOP])
                mid.append(a)
                end.append(b)
        for name, m in (("2041..2048", np.concatenate(mid)), ("4073..4095", np.concatenate(end))):
            assert m.any() and not m.all(), "call %d of (%d streams, %d hops): no set and clear mask in bins %s" % (c, S, M, name)


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


def check_against_oracle_and_base(z, x, ref, S, M, run_len, base_cache, key):
    if key not in base_cache:
        base_cache[key] = three_calls(z, x, S, M, 0, off=1)
    base, base_routed = base_cache[key]
    got, routed = three_calls(z, x, S, M, run_len, off=0)
    assert base_routed == 0 and routed == 3
    n = 3 * M * HOP
    assert np.array_equal(base, ref[:S, :n]), "the base path differs from the oracle"
    assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), "run kernel differs from the base path"
    assert np.array_equal(got, ref[:S, :n])
    return got


_base = {}


@pytest.mark.parametrize("run_len", [1, 2, 0])
@pytest.mark.parametrize("n_hops", [1, 2, 9])
@pytest.mark.parametrize("n_streams", [1, 3])
def test_noise_three_calls_equal_oracle_and_base(z, noise, n_streams, n_hops, run_len):
    x, ref = noise
    assert_masks_flip_in_every_call(x, n_streams, n_hops)
    got = check_against_oracle_and_base(z, x, ref, n_streams, n_hops, run_len, _base, (n_streams, n_hops))
    assert np.any(got != 0)


def degenerate(kind):
    x = np.zeros((S_MAX, HOPS_MAX * HOP), np.float32)
    if kind == "impulse":
        x[:, ::HOP] = 1.0   # a unit impulse at sample 0 of each hop
    else:
        x[:, 0::2], x[:, 1::2] = 1.0, -1.0
    return x


_degenerate = {}


@pytest.mark.parametrize("run_len", [2, 0])
@pytest.mark.parametrize("kind", ["impulse", "alternating"])
def test_impulse_and_alternating_input_equal_oracle_and_base(z, kind, run_len):
    """thread-local sums that cancel exactly and rows whose energy sits in single bins: zeros and signs of zeros"""
    if kind not in _degenerate:
        _degenerate[kind] = oracle_streams(degenerate(kind)) + ({},)
    x, ref, cache = _degenerate[kind]
    check_against_oracle_and_base(z, x, ref, S_MAX, 9, run_len, cache, kind)


def test_use_sse_filter_after_a_routed_call_reads_rows_copied_from_the_image(z, noise):
    """the magnitude ring rows of the call's last frames are copied from the image, whose upper half is no longer complete"""
    x, _ = noise
    A, B = 6, 4
    n = (A + B) * HOP
    out = {}
    for off in (1, 0):
        eng = primed_engine(z, 1, A, x)
        d_in = z.DeviceBuffer.from_host(np.ascontiguousarray(x[0, :n]))
        d_out = z.DeviceBuffer(n)
        d_out.zero()
        z.blockrun_set("off", off)
        routed0 = z.blockrun_stats()[0]
        try:
            eng.process(d_in.ptr, A, n, None, d_out.ptr, None, n)
            eng.use_sse_filter()
            eng.process(d_in.offset(A * HOP), B, n, None, d_out.offset(A * HOP), None, n)
            z.synchronize()
        finally:
            z.blockrun_set("off", 0)
        assert z.blockrun_stats()[0] - routed0 == (0 if off else 1)   # (the SSE call is the base library's)
        out[off] = d_out.download()
    ora = o.HPR(FS, HOP, BETA, P, o.TIME_CAUSAL)
    want = ora.process_stream(x[0, :A * HOP])["P"]
    ora.use_sse_filter()
    want = np.concatenate([want, ora.process_stream(x[0, A * HOP:n])["P"]])
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
    assert np.array_equal(out[0], want) and np.any(want != 0)
