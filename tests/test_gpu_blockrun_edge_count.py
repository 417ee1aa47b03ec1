"""GPU tests of the run kernel's counted edge masks (zen_amd/blockrun/blockrun_edge_count.h): the percussive masks of bin
N/2 and of the bins N - 23 .. N - 1 are counted by one wave instead of selected by a third median stream, and FwdOut computes
|S[N/2]| in thread 0 alone.  Routed block calls at tolerance 0 against the CPU oracle and bit for bit against the base
library's own path (off = 1).

Settings as tests/test_gpu_blockrun_first_pass.py: hop 1024, min_items 0, every engine primed with one block call of the base
library and reset, the calls the run kernel served read from zen_hip_blockrun_stats.

A case in which no edge mask ever changes proves nothing, so a CPU-only test (no GPU marker) recomputes the 24 masks of every
frame from the oracle's magnitude rows -- 47-tap median with the replicate border, float32 divide, as hps.cu has it -- checks
them against the oracle's own mask row, and asserts which bins take both values over the 37 hops of stream 0:
  - beta 2 (the headline setting), S-noise seed 0: every bin but N - 1.  Bin N - 1 cannot: its window holds column N - 1 and
    24 border replicas of it, 25 of 47 keys, so its median IS mag[1] = H and P / (H + Eps) < 1 < beta for every input.
  - beta 1, the same noise scaled by 0.25: all 24.  There bin N - 1 is fl(m / (m + Eps)) >= 1, which holds exactly when
    m + Eps rounds back to m (m of about 2 and above); the scale puts mag[1] on both sides of that.
Both inputs run on the GPU below."""
import numpy as np
import pytest

from oracle import oracle as o

gpu = pytest.mark.gpu
FS, HOP, BETA, NFFT, TAPS = 44100.0, 1024, 2.0, 4096, 47
P = o.OUTPUT_PERCUSSIVE
S_MAX, HOPS_MAX, SEED = 3, 3 * 37, 0
BETA_ONE, SCALE_ONE = 1.0, 0.25
EDGE_BINS = np.concatenate([[NFFT // 2], np.arange(NFFT - TAPS // 2, NFFT)])
EPS = np.float32(np.finfo(np.float32).eps)


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


def s_noise():
    return np.random.default_rng(SEED).uniform(-1, 1, (S_MAX, HOPS_MAX * HOP)).astype(np.float32)


def make_input(kind):
    """(input, beta, whether the oracle defines the output)"""
    if kind == "noise":
        return s_noise(), BETA, True
    if kind == "noise_beta1":
        return s_noise() * np.float32(SCALE_ONE), BETA_ONE, True
    if kind == "impulse":
        x = np.zeros((S_MAX, HOPS_MAX * HOP), np.float32)
        x[:, ::HOP] = 1.0   # a unit impulse at sample 0 of each hop
        return x, BETA, True
    if kind == "alternating":
        x = np.zeros((S_MAX, HOPS_MAX * HOP), np.float32)
        x[:, 0::2], x[:, 1::2] = 1.0, -1.0
        return x, BETA, True
    assert kind == "nonfinite"
    x = s_noise()
    x[0, HOP + 300] = np.nan   # second hop: rows of NaN magnitudes in the frames that hold it
    x[1, HOP + 700] = np.inf   # inf - inf in the transform: NaN and inf magnitudes side by side
    return x, BETA, False      # (the oracle's median of NaNs depends on its sort: compared with the base path only)


_inputs = {}


def input_and_reference(kind):
    """computed once per kind, read only; the oracle's percussive streams where it defines them"""
    if kind not in _inputs:
        x, beta, defined = make_input(kind)
        ref = None
        if defined:
            ref = np.stack([o.HPR(FS, HOP, beta, P, o.TIME_CAUSAL).process_stream(x[s])["P"] for s in range(S_MAX)])
            ref.setflags(write=False)
        x.setflags(write=False)
        _inputs[kind] = (x, beta, ref, {})
    return _inputs[kind]


def oracle_edge_masks(x, beta):
    """the 24 edge masks of every frame of one stream, from the oracle's magnitude rows; (n_hops, 24) bool, column j as EDGE_BINS"""
    h = o.HPR(FS, HOP, beta, P, o.TIME_CAUSAL)
    r = h.stft_width - h.lag
    out = []
    for i in range(x.size // HOP):
        h.process_next_hop(x[i * HOP:(i + 1) * HOP])
        mag, hrow = h.matrix("s_mag")[r], h.matrix("harmonic_matrix")[r]
        pad = np.concatenate([np.full(TAPS // 2, mag[0]), mag, np.full(TAPS // 2, mag[-1])])
        med = np.array([np.sort(pad[k:k + TAPS])[TAPS // 2] for k in EDGE_BINS], np.float32)
        bits = (med / (hrow[EDGE_BINS] + EPS)) >= np.float32(beta)
        assert np.array_equal(bits, h.matrix("percussive_mask")[r][EDGE_BINS] != 0), "frame %d: not the oracle's own masks" % i
        out.append(bits)
    return np.array(out)


def test_edge_masks_take_both_values_in_the_oracle():
    x, beta, _ = make_input("noise")
    m = oracle_edge_masks(x[0, :37 * HOP], beta)
    both = m.any(axis=0) & ~m.all(axis=0)
    assert both[:-1].all(), "beta 2: bins without a set and a clear mask: %s" % EDGE_BINS[:-1][~both[:-1]]
    assert not m[:, -1].any()   # bin N - 1: median == mag[1] == H (module docstring)
    x, beta, _ = make_input("noise_beta1")
    m = oracle_edge_masks(x[0, :37 * HOP], beta)
    both = m.any(axis=0) & ~m.all(axis=0)
    assert both.all(), "beta 1: bins without a set and a clear mask: %s" % EDGE_BINS[~both]


def primed_engine(z, S, M, x, beta):
    """an engine whose buffers the base library has sized for block calls of M hops, back in its initial state"""
    m = max(M, 2)
    eng = z.HPR(FS, HOP, beta, z.OUTPUT_PERCUSSIVE, z.TIME_CAUSAL, True, S, m)
    d_in = z.DeviceBuffer.from_host(np.ascontiguousarray(x[:S, :m * HOP]))
    d_out = z.DeviceBuffer(S * m * HOP)
    z.blockrun_set("off", 1)
    eng.process(d_in.ptr, m, m * HOP, None, d_out.ptr, None, m * HOP)
    z.blockrun_set("off", 0)
    eng.reset_buffers()
    z.synchronize()
    return eng


def three_calls(z, x, beta, S, M, run_len, off):
    """three consecutive block calls of M hops on S streams; returns the (S, 3 * M * HOP) output and the calls served by the run kernel"""
    n = 3 * M * HOP
    eng = primed_engine(z, S, M, x, beta)
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


@gpu
@pytest.mark.parametrize("run_len", [1, 5, 64])
@pytest.mark.parametrize("n_hops", [1, 2, 37])
@pytest.mark.parametrize("n_streams", [1, 3])
@pytest.mark.parametrize("kind", ["noise", "noise_beta1", "impulse", "alternating", "nonfinite"])
def test_three_routed_calls_equal_oracle_and_base(z, kind, n_streams, n_hops, run_len):
    x, beta, ref, base_cache = input_and_reference(kind)
    key = (n_streams, n_hops)
    if key not in base_cache:
        base_cache[key] = three_calls(z, x, beta, n_streams, n_hops, 0, off=1)
    base, base_routed = base_cache[key]
    got, routed = three_calls(z, x, beta, n_streams, n_hops, run_len, off=0)
    assert base_routed == 0 and routed == 3
    n = 3 * n_hops * HOP
    assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), "run kernel differs from the base path"
    if ref is not None:
        assert np.array_equal(base, ref[:n_streams, :n]), "the base path differs from the oracle"
        assert np.array_equal(got, ref[:n_streams, :n])
        assert np.any(got != 0) or not kind.startswith("noise")   # (a flat row has no percussive part: the impulse's output is zero)
    else:
        assert np.isnan(got).any() and np.isfinite(got).any()   # the sample reached the call, and did not take everything


@gpu
def test_use_sse_filter_after_a_routed_call(z):
    """the magnitude rows a later use_sse_filter() reads are copied from the image, bin N/2 (thread 0's branch) among them"""
    x, beta, _, _ = input_and_reference("noise")
    A, B = 6, 4
    n = (A + B) * HOP
    out = {}
    for off in (1, 0):
        eng = primed_engine(z, 1, A, x, beta)
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
    ora = o.HPR(FS, HOP, beta, P, o.TIME_CAUSAL)
    want = ora.process_stream(x[0, :A * HOP])["P"]
    ora.use_sse_filter()
    want = np.concatenate([want, ora.process_stream(x[0, A * HOP:n])["P"]])
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
    assert np.array_equal(out[0], want) and np.any(want != 0)


@gpu
def test_four_per_hop_calls_with_copy_output_go_on_from_a_routed_call(z):
    """the state contract: Y rows, input tail, carry and magnitude rows as the base library leaves them"""
    x, beta, ref, _ = input_and_reference("noise")
    A, B = 7, 4
    n = (A + B) * HOP
    out = {}
    for off in (1, 0):
        eng = primed_engine(z, 1, A, x, beta)
        d_in = z.DeviceBuffer.from_host(np.ascontiguousarray(x[0, :n]))
        d_out = z.DeviceBuffer(n)
        d_out.zero()
        z.blockrun_set("run_len", 3)
        z.blockrun_set("off", off)
        routed0 = z.blockrun_stats()[0]
        try:
            eng.process(d_in.ptr, A, n, None, d_out.ptr, None, n)
            for i in range(A, A + B):
                eng.process_next_hop(d_in.offset(i * HOP))
                eng.copy_output(z.OUTPUT_PERCUSSIVE, d_out.offset(i * HOP))
            z.synchronize()
        finally:
            z.blockrun_set("off", 0)
            z.blockrun_set("run_len", 0)
        assert z.blockrun_stats()[0] - routed0 == (0 if off else 1)
        out[off] = d_out.download()
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
    assert np.array_equal(out[0], ref[0, :n])
