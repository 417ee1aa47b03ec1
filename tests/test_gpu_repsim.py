"""GPU tier: libzen_hip_repsim.so (zen_amd/repsim) -- REPET-SIM on device rows.  Tolerance 0 everywhere: the similarity matrix on
both routes (the matrix cores and the vector ALU), the selection, the median over the selected frames, the background and the
foreground are compared bit for bit against tests/repsim_model.py.  NaNs stand around the inputs (a kernel that read outside
the elements of its call would carry them into a result) and sentinels around every output."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import repsim_model as M  # noqa: E402
from test_gpu_repet import PALETTE, pcm16, read_wav_pcm16, write_wav_float32  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
ISENTINEL = -777
FS = M.FAMILY_FS
BAD = 2
f32 = np.float32


@pytest.fixture(scope="module")
def repsim():
    """The library of this feature, built on demand (the session fixture of conftest.py builds the one it links against)."""
    import zen_amd
    from zen_amd import repsim as mod
    mod.load()
    zen_amd.init(0)
    return mod


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    g, w = np.asarray(got), np.asarray(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    diff = np.flatnonzero(bits(g).ravel() != bits(w).ravel())
    assert diff.size == 0, "%s differs from the model in %d places, the first at %d: %r != %r" % (
        what, diff.size, diff[0], g.ravel()[diff[0]], w.ravel()[diff[0]])


def rows_into(host, lead, stride, A):
    for a in range(A.shape[0]):
        host[lead + a * stride:lead + a * stride + A.shape[1]] = A[a]


def rows_out(got, lead, stride, rows, cols, sentinel):
    """the (rows, cols) block of a downloaded buffer, everything around it still the sentinel"""
    assert np.all(got[:lead] == sentinel) and np.all(got[lead + rows * stride:] == sentinel)
    block = got[lead:lead + rows * stride].reshape(rows, stride)
    assert np.all(block[:, cols:] == sentinel), "written beyond the elements of a row"
    return block[:, :cols].copy()


def round4(v):
    return (v + 3) & ~3


# ================================================================================================ the similarity alone
SIM_M = (1, 2, 31, 32, 33, 64, 65, 127, 128, 129, 160)
SIM_BINS = (1, 2, 3, 33, 129, 130)
KINDS = ("uniform", "palette", "denormal")
_sim_cache = {}


def sim_values(kind, m, bins):
    """(V, the model's S), computed once per case: `uniform` has both signs; `palette` a few levels with zeros, so that equal
    sums tie; `denormal` rows of denormals and rows at 1e-30, whose products underflow, beside ordinary rows.  Row m // 2 is
    all zeros."""
    key = (kind, m, bins)
    if key not in _sim_cache:
        rng = np.random.default_rng(1000 * KINDS.index(kind) + 7 * m + bins)
        if kind == "uniform":
            V = rng.uniform(-1, 1, (m, bins)).astype(f32)
        elif kind == "palette":
            V = f32([0, 0, 0.25, 0.5, 1, 1, 2, 3])[rng.integers(0, 8, (m, bins))]
        else:
            scale = f32([1e-44, 3e-41, 1e-38, 1e-30, 1e-30, 1e-19, 1e-8, 1.0])[rng.integers(0, 8, m)]
            V = (rng.uniform(-1, 1, (m, bins)).astype(f32) * scale[:, None]).astype(f32)
        if m >= 2:
            V[m // 2] = 0
        _sim_cache[key] = (V, M.similarity(V))
    return _sim_cache[key]


def sim_case(repsim, V, want, v_stride, s_stride, lead):
    import zen_amd
    m, bins = V.shape
    v_host = np.full(lead + m * v_stride + 8, np.nan, f32)
    rows_into(v_host, lead, v_stride, V)
    v_dev = zen_amd.DeviceBuffer.from_host(v_host)
    got = {}
    for route in (repsim.ROUTE_MFMA, repsim.ROUTE_VALU):
        s_dev = zen_amd.DeviceBuffer.from_host(np.full(lead + m * s_stride + 8, SENTINEL, f32))
        repsim.similarity_device(v_dev.offset(lead), m, bins, v_stride, s_dev.offset(lead), s_stride, route)
        zen_amd.synchronize()
        got[route] = rows_out(s_dev.download(), lead, s_stride, m, m, SENTINEL)
    assert np.array_equal(v_dev.download(), v_host, equal_nan=True), "V was written"
    what = "S at m %d bins %d strides %d %d lead %d" % (m, bins, v_stride, s_stride, lead)
    for route, name in ((repsim.ROUTE_VALU, "the vector route"), (repsim.ROUTE_MFMA, "the matrix-core route")):
        S = got[route]
        assert np.array_equal(bits(S), bits(S.T)), "%s: %s is not symmetric" % (name, what)
        if m >= 2:
            assert np.all(bits(S[m // 2]) == 0) and np.all(bits(S[:, m // 2]) == 0), "%s: the all-zero row is not +0" % name
        assert_same_bits(S, want, "%s: %s" % (name, what))
    assert_same_bits(got[repsim.ROUTE_MFMA], got[repsim.ROUTE_VALU], "the two routes: " + what)


LAYOUTS = {"tight": (0, 0, 0), "padded": (4, 4, 0), "padded_off16": (4, 8, 1), "tight_off16": (0, 0, 2), "odd_stride": (1, 3, 0)}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind", KINDS)
def test_similarity_both_routes(repsim, kind, layout):
    """every m and bins on both sides of the 32 x 32 tile, the 128 x 128 block and the chunk of 32 bins; strides padded to 16
    bytes take the 16-byte loads, the others single words"""
    vpad, spad, lead = LAYOUTS[layout]
    for m in SIM_M:
        for bins in SIM_BINS:
            V, want = sim_values(kind, m, bins)
            v_stride = round4(bins) + vpad if layout.startswith("padded") else bins + vpad
            s_stride = round4(m) + spad if layout.startswith("padded") else m + spad
            sim_case(repsim, V, want, v_stride, s_stride, lead)


def test_similarity_default_route_and_more_than_one_block_each_way(repsim):
    import zen_amd
    rng = np.random.default_rng(2)
    V = rng.uniform(0, 1, (300, 70)).astype(f32)
    V[150] = 0                  # the all-zero row sim_case looks for
    want = M.similarity(V)
    sim_case(repsim, V, want, 72, 300, 0)
    v_dev, s_dev = zen_amd.DeviceBuffer.from_host(V), zen_amd.DeviceBuffer(300 * 300)
    repsim.similarity_device(v_dev, 300, 70, 70, s_dev, 300)
    zen_amd.synchronize()
    assert_same_bits(s_dev.download().reshape(300, 300), want, "the default route")


# ================================================================================================ the selection alone
def select_case(repsim, S, t, dd, k, s_stride, lead):
    import zen_amd
    m = S.shape[0]
    s_host = np.full(lead + m * s_stride + 8, np.nan, f32)
    rows_into(s_host, lead, s_stride, S)
    s_dev = zen_amd.DeviceBuffer.from_host(s_host)
    idx_dev = zen_amd.DeviceBuffer.from_host(np.full(3 + m * k + 5, ISENTINEL, np.int32))
    cnt_dev = zen_amd.DeviceBuffer.from_host(np.full(2 + m + 5, ISENTINEL, np.int32))
    repsim.select_device(s_dev.offset(lead), m, s_stride, t, dd, k, idx_dev.offset(3), cnt_dev.offset(2))
    zen_amd.synchronize()
    assert np.array_equal(s_dev.download(), s_host, equal_nan=True), "S was written"
    idx = rows_out(idx_dev.download(), 3, k, m, k, ISENTINEL)
    counts = rows_out(cnt_dev.download(), 2, m, 1, m, ISENTINEL)[0]
    want_idx, want_counts = M.select(S, t, min(dd, m), k)
    what = "m %d dd %d k %d t %g stride %d lead %d" % (m, dd, k, t, s_stride, lead)
    assert np.array_equal(counts, want_counts), "counts at " + what
    assert np.array_equal(idx, want_idx), "idx at " + what


@pytest.mark.parametrize("m", [1, 5, 64, 65, 300])
def test_select_on_a_quantised_matrix(repsim, m):
    """few levels, so that the largest value is there many times over and the first index must win; an all-zero row (no
    candidate at t = 0) and a row holding a NaN (never a candidate)"""
    rng = np.random.default_rng(m)
    levels = f32([0.0, 0.0, 0.125, 0.25, 0.5, 0.5, 0.75, 0.875, 1.0])
    S = levels[rng.integers(0, levels.size, (m, m))]
    S[m // 3] = 0
    S[m // 2, rng.integers(0, m)] = np.nan
    if m > 5:
        S[m // 2, 3] = np.nan
        S[m - 1] = np.nan
    case = 0
    for dd in (1, 2, 5, m + 3):
        for k in (1, 2, 31, 32, 33, 256):
            for t in (0.0, 0.5):
                s_stride, lead = ((m, 0), (round4(m) + 4, 0), (m + 1, 1))[case % 3]
                select_case(repsim, S, t, dd, k, s_stride, lead)
                case += 1


# ================================================================================================ the median alone
COUNTS = (0, 1, 2, 3, 8, 9, 31, 32, 33, 64, 65, 128, 255, 256)


def median_case(repsim, rng, counts, k, m, bins, v_stride, u_stride, lead):
    """one launch on a V of m rows quantised to a few levels (ties), with zeros, denormals and values whose sum overflows; the
    frames' counts are mixed, their indices random"""
    import zen_amd
    rows = len(counts)
    V = PALETTE[rng.integers(0, PALETTE.size, (m, bins))]
    idx = np.full((rows, k), -1, np.int32)
    for a, c in enumerate(counts):
        idx[a, :c] = rng.permutation(m)[:c] if c <= m else rng.integers(0, m, c)
    v_host = np.full(lead + m * v_stride + 8, np.nan, f32)
    rows_into(v_host, lead, v_stride, V)
    v_dev = zen_amd.DeviceBuffer.from_host(v_host)
    u_dev = zen_amd.DeviceBuffer.from_host(np.full(lead + rows * u_stride + 8, SENTINEL, f32))
    idx_dev, cnt_dev = zen_amd.DeviceBuffer.from_host(idx), zen_amd.DeviceBuffer.from_host(np.asarray(counts, np.int32))
    repsim.gather_median_device(v_dev.offset(lead), m, bins, v_stride, idx_dev, cnt_dev, rows, k, u_dev.offset(lead), u_stride)
    zen_amd.synchronize()
    assert np.array_equal(v_dev.download(), v_host, equal_nan=True), "V was written"
    assert np.array_equal(idx_dev.download().reshape(rows, k), idx) and np.array_equal(cnt_dev.download(), counts)
    U = rows_out(u_dev.download(), lead, u_stride, rows, bins, SENTINEL)
    want = M.gather_median(V, idx, np.asarray(counts, np.int32))
    for a, c in enumerate(counts):                   # against numpy.sort directly as well
        if c:
            s = np.sort(V[idx[a, :c]], axis=0)
            with np.errstate(over="ignore"):
                assert np.array_equal(bits(want[a]), bits(s[(c - 1) // 2] if c & 1 else (s[c // 2 - 1] + s[c // 2]) * f32(0.5)))
    assert_same_bits(U, want, "U at k %d m %d bins %d strides %d %d lead %d" % (k, m, bins, v_stride, u_stride, lead))
    assert np.all(bits(U[np.asarray(counts) == 0]) == 0), "no frame: +0"


@pytest.mark.parametrize("bins,v_stride,u_stride,lead", [(33, 33, 33, 0), (33, 40, 36, 0), (129, 129, 129, 1), (129, 136, 132, 0), (129, 136, 132, 2)],
                         ids=["33_tight", "33_padded", "129_tight_off16", "129_padded", "129_padded_off16"])
def test_gather_median_every_count_in_one_launch(repsim, bins, v_stride, u_stride, lead):
    """counts on both sides of every network and of the crossover between the registers and LDS, three frames each, shuffled"""
    rng = np.random.default_rng(bins + v_stride + lead)
    counts = [int(c) for c in rng.permutation(np.repeat(COUNTS, 3))]
    median_case(repsim, rng, counts, 256, 300, bins, v_stride, u_stride, lead)
    # a k that needs no LDS, and one whose longest column is padded to 64
    median_case(repsim, rng, [c for c in counts if c <= 32], 32, 300, bins, v_stride, u_stride, lead)
    median_case(repsim, rng, [c for c in counts if c <= 40] + [40, 39], 40, 45, bins, v_stride, u_stride, lead)


def test_gather_median_more_than_one_block_of_bins(repsim):
    rng = np.random.default_rng(1)
    median_case(repsim, rng, [3, 100, 0, 17, 33, 6, 2], 100, 120, 1025, 1028, 1028, 0)     # the 16-byte path with a tail, 5 blocks
    median_case(repsim, rng, [5, 40, 1, 128], 128, 200, 300, 301, 300, 0)                   # single words, the last block ragged


# ================================================================================================ the whole call
def run_device(rs, x, want=(True, True), lead=(0, 0, 0), pad=(0, 0), selection=False):
    """x: (n_clips, n) rows.  `lead` floats in front of the input / background / foreground rows, `pad` floats between the rows
    (input, outputs).  Returns (background, foreground[, counts, indices]); None for an output that was not asked for."""
    import zen_amd
    x = np.asarray(x, np.float32).reshape(rs.n_clips, -1)
    C, n = x.shape
    m, k = M.R.n_frames(n, rs.hop), rs.number
    in_stride, out_stride = n + pad[0], n + pad[1]
    in_host = np.full(lead[0] + C * in_stride + 8, np.nan, np.float32)
    rows_into(in_host, lead[0], in_stride, x)
    inp = zen_amd.DeviceBuffer.from_host(in_host)
    outs = [zen_amd.DeviceBuffer.from_host(np.full(lead[1 + o] + C * out_stride + 8, SENTINEL, np.float32)) for o in range(2)]
    cnt = zen_amd.DeviceBuffer.from_host(np.full(1 + C * m + 4, ISENTINEL, np.int32))
    idx = zen_amd.DeviceBuffer.from_host(np.full(1 + C * m * k + 4, ISENTINEL, np.int32))
    rs.separate_device(inp.offset(lead[0]), in_stride, n, *(outs[o].offset(lead[1 + o]) if want[o] else None for o in range(2)),
                       out_stride=out_stride, counts=cnt.offset(1) if selection else None, indices=idx.offset(1) if selection else None)
    zen_amd.synchronize()
    assert np.array_equal(inp.download(), in_host, equal_nan=True), "the input buffer was written"
    res = []
    for o in range(2):
        got = outs[o].download()
        if not want[o]:
            assert np.all(got == SENTINEL)
            res.append(None)
            continue
        res.append(rows_out(got, lead[1 + o], out_stride, C, n, SENTINEL))
    if not selection:
        assert np.all(cnt.download() == ISENTINEL) and np.all(idx.download() == ISENTINEL)
        return tuple(res)
    return tuple(res) + (rows_out(cnt.download(), 1, C * m, 1, C * m, ISENTINEL).reshape(C, m),
                         rows_out(idx.download(), 1, C * m * k, 1, C * m * k, ISENTINEL).reshape(C, m, k))


def family_session(repsim, N, n_clips, max_samples):
    return repsim.Repsim(FS, N, n_clips, max_samples, M.FAMILY_THRESHOLD, M.family_distance(N), M.FAMILY_NUMBER, 0.0)


@pytest.mark.parametrize("shape", M.SHAPES, ids=lambda s: "N%d_p%d_q%d_r%d" % s)
def test_one_clip_of_each_family_shape(repsim, oracle, shape):
    oracle.lib()
    N = shape[0]
    x = M.family_clip(0, *shape)[0]
    want = M.family_separate(x, N)
    bg, fg, counts, idx = run_device(family_session(repsim, N, 1, x.size), x, selection=True)
    assert np.array_equal(counts[0], want.counts) and np.array_equal(idx[0], want.idx)
    assert np.all(counts == M.FAMILY_NUMBER)
    assert_same_bits(bg[0], want.background, "background")
    assert_same_bits(fg[0], want.foreground, "foreground")


@pytest.fixture(scope="module")
def three(oracle):
    """three different clips of the family at N = 256, cut to one length that is no multiple of H, with the model's results at
    the family's settings"""
    oracle.lib()
    n = 13861
    x = np.stack([M.family_clip(seed, 256, P, Q, reps)[0][:n] for seed, (P, Q, reps) in ((1, (6, 3, 24)), (2, (9, 4, 24)), (3, (12, 3, 18)))])
    assert n % 128 == 37
    return x, [M.family_separate(r, 256) for r in x]


def test_three_clips_in_one_call_padded_strides_and_an_odd_lead(repsim, three):
    x, model = three
    rs = family_session(repsim, 256, 3, x.shape[1] + 100)
    bg, fg, counts, idx = run_device(rs, x, lead=(1, 2, 3), pad=(3, 5), selection=True)
    for c in range(3):
        assert np.array_equal(counts[c], model[c].counts) and np.array_equal(idx[c], model[c].idx), "the selection of clip %d" % c
        assert_same_bits(bg[c], model[c].background, "background of clip %d" % c)
        assert_same_bits(fg[c], model[c].foreground, "foreground of clip %d" % c)
    assert rs.stats()["bands"] == 3 and rs.stats()["clips"] == 3


def test_each_output_on_its_own(repsim, three):
    x, model = three
    rs = family_session(repsim, 256, 3, x.shape[1])
    bg, none = run_device(rs, x, want=(True, False))
    assert none is None
    none, fg = run_device(rs, x, want=(False, True), lead=(0, 1, 1))
    assert none is None
    for c in range(3):
        assert_same_bits(bg[c], model[c].background, "background alone, clip %d" % c)
        assert_same_bits(fg[c], model[c].foreground, "foreground alone, clip %d" % c)
    none, none2, counts, idx = run_device(rs, x, want=(False, False), selection=True)
    assert none is None and none2 is None and np.array_equal(counts[2], model[2].counts) and np.array_equal(idx[1], model[1].idx)


@pytest.mark.parametrize("option", ["mfma=0", "mfma=1,band=128"], ids=["vector_route", "bands_of_128"])
def test_the_other_route_and_narrow_bands_give_the_same(repsim, three, monkeypatch, option):
    """110 frames per clip are one band of 128; a clip of 300 frames goes through three"""
    x, model = three
    monkeypatch.setenv("ZEN_HIP_REPSIM", option)
    rs = family_session(repsim, 256, 3, x.shape[1])
    bg, fg = run_device(rs, x)
    for c in range(3):
        assert_same_bits(bg[c], model[c].background, "background of clip %d" % c)
        assert_same_bits(fg[c], model[c].foreground, "foreground of clip %d" % c)
    prof_route = "similarity_valu" if option == "mfma=0" else "similarity_mfma"
    rs.profile(True)
    run_device(rs, x)
    prof = rs.profile_get()
    assert prof[prof_route]["launches"] == 3 and prof["similarity_mfma"]["launches"] + prof["similarity_valu"]["launches"] == 3
    y = M.family_clip(0, 64, 9, 3, 33)[0]
    assert M.R.n_frames(y.size, 32) == 300
    want = M.separate(y, FS, 64, 0.0, 2.5 * 32 / FS, 20, 0.0)
    long = repsim.Repsim(FS, 64, 1, y.size, 0.0, 2.5 * 32 / FS, 20, 0.0)
    bg, fg, counts, idx = run_device(long, y, selection=True)
    assert long.stats()["bands"] == (3 if "band" in option else 1)
    assert np.array_equal(counts[0], want.counts) and np.array_equal(idx[0], want.idx)
    assert_same_bits(bg[0], want.background, "background of 300 frames")
    assert_same_bits(fg[0], want.foreground, "foreground of 300 frames")


def test_a_silent_clip(repsim, oracle):
    oracle.lib()
    x = np.zeros(3000, np.float32)
    x[7] = -0.0
    bg, fg, counts, idx = run_device(repsim.Repsim(FS, 256, max_samples=3000), x, lead=(1, 1, 1), selection=True)
    assert np.all(counts == 0) and np.all(idx == -1)
    assert np.all(bits(bg) == 0), "the background is +0"
    assert_same_bits(fg[0], x, "the foreground is x - 0")


@pytest.mark.parametrize("n", [1, 128, 129])
def test_the_shortest_clips_and_more_neighbours_asked_for_than_frames(repsim, oracle, n):
    """n = 1, H, H + 1: two and three frames under the default k of 100"""
    oracle.lib()
    x = np.random.default_rng(n).uniform(-1, 1, n).astype(np.float32)
    want = M.separate(x, FS, 256, distance_s=0.0)
    rs = repsim.Repsim(FS, 256, max_samples=129, distance_s=0.0)
    bg, fg, counts, idx = run_device(rs, x, lead=(1, 1, 1), selection=True)
    assert idx.shape[2] == 100 and np.array_equal(counts[0], want.counts) and np.array_equal(idx[0], want.idx)
    assert counts.max() == M.R.n_frames(n, 128)
    assert_same_bits(bg[0], want.background, "background")
    assert_same_bits(fg[0], want.foreground, "foreground")


@pytest.fixture(scope="module")
def two_seconds(oracle):
    oracle.lib()
    x = M.family_clip(1, 256, 9, 4, 24)[0][:16000]
    return x, M.separate(x, FS, 256)


def test_the_defaults_on_two_seconds(repsim, two_seconds):
    """t = 0, one second (63 frames) apart, k = 100, the high-pass at 100 Hz: 126 frames, two or three frames per median"""
    x, want = two_seconds
    assert M.distance_frames(M.DISTANCE, FS, 128, 126) == 63 and M.R.cutoff_bin(FS, 256, M.HIGHPASS) == 4 and want.counts.max() <= 3
    bg, fg, counts, idx = run_device(repsim.Repsim(FS, 256, max_samples=16000), x, selection=True)
    assert np.array_equal(counts[0], want.counts) and np.array_equal(idx[0], want.idx)
    assert_same_bits(bg[0], want.background, "background")
    assert_same_bits(fg[0], want.foreground, "foreground")
    b2, f2 = repsim.separate(x, FS, 256)
    assert_same_bits(b2, want.background, "repsim.separate")
    assert_same_bits(f2, want.foreground, "repsim.separate")


# ================================================================================================ arguments, memory, the program
def test_host_call_equals_device_call_and_later_calls_allocate_nothing(repsim, three, two_seconds):
    import zen_amd
    x, model = three
    rs = family_session(repsim, 256, 3, x.shape[1] + 64)
    zen_amd.synchronize()
    st0, mc0 = rs.stats(), zen_amd.memcheck()
    assert st0["allocations"] == 10 and st0["calls"] == 0
    bg, fg, counts, idx = rs.run(x, selection=True)
    for c in range(3):
        assert np.array_equal(counts[c], model[c].counts) and np.array_equal(idx[c], model[c].idx)
        assert_same_bits(bg[c], model[c].background, "host background")
        assert_same_bits(fg[c], model[c].foreground, "host foreground")
    dev = run_device(rs, x)
    assert_same_bits(dev[0], bg, "device against host")
    assert_same_bits(dev[1], fg, "device against host")
    only_bg = rs.run(x[:, :5000], foreground=False)
    assert only_bg[1] is None and only_bg[0].shape == (3, 5000)
    y, want = two_seconds
    one = repsim.Repsim(FS, 256, max_samples=y.size).run(y)
    assert_same_bits(one[0], want.background, "one clip, one dimension")
    rs.profile(True)
    rs.run(x)
    prof = rs.profile_get()
    assert list(prof) == list(repsim.KERNELS)
    ran = [name for name, p in prof.items() if p["launches"]]
    assert len(ran) == 9 and ("similarity_mfma" in ran) != ("similarity_valu" in ran)
    for name in ran:
        p = prof[name]
        assert p["launches"] == (1 if name in ("frame", "fft", "magnitude") else 3) and p["ms"] > 0 and p["bytes"] > 0, name
    rs.profile(False)
    zen_amd.synchronize()
    st1, mc1 = rs.stats(), zen_amd.memcheck()
    assert st1["allocations"] == st0["allocations"] and st1["device_bytes"] == st0["device_bytes"]
    assert st1["calls"] == 4 and st1["clips"] == 12 and st1["bands"] == 12
    if mc1["redzone_bytes"]:
        assert mc1["live_allocations"] == mc0["live_allocations"] and mc1["corrupt_words"] == 0


def test_bad_arguments_are_refused_and_touch_nothing(repsim):
    import zen_amd
    L = repsim.load()
    n = 2000
    rs = repsim.Repsim(FS, 256, max_samples=n)
    x = np.random.default_rng(0).uniform(-1, 1, n).astype(np.float32)
    inp = zen_amd.DeviceBuffer.from_host(x)
    out = zen_amd.DeviceBuffer.from_host(np.full(2 * n, SENTINEL, np.float32))
    ints = zen_amd.DeviceBuffer.from_host(np.full(4000, ISENTINEL, np.int32))
    before = rs.stats()
    cases = [(None, inp.ptr, n, n, n),
             (rs._h, None, n, n, n),
             (rs._h, inp.ptr, n - 1, n, n),             # in_stride below the clip
             (rs._h, inp.ptr, n, n, n - 1),             # out_stride below the clip
             (rs._h, inp.ptr, n, 0, n),                 # no samples
             (rs._h, inp.ptr, n + 1, n + 1, n + 1),     # more than max_samples
             (rs._h, inp.ptr + 2, n, n, n)]
    for hh, a, in_stride, cnt, out_stride in cases:
        for f in (L.zen_hip_repsim_separate_device, L.zen_hip_repsim_separate_host):
            assert f(hh, a, in_stride, cnt, out.ptr, out.offset(n), out_stride, None, None) == BAD
            assert L.zen_hip_repsim_last_error() != b""
    assert L.zen_hip_repsim_separate_device(rs._h, inp.ptr, n, n, out.ptr + 1, None, n, None, None) == BAD
    assert L.zen_hip_repsim_separate_device(rs._h, inp.ptr, n, n, out.ptr, None, n, ints.ptr + 2, None) == BAD
    for t, d, k, hp in ((-0.1, 1, 100, 100), (1.0, 1, 100, 100), (np.nan, 1, 100, 100), (0, -1, 100, 100), (0, np.inf, 100, 100), (0, 1, 0, 100),
                        (0, 1, 257, 100), (0, 1, 100, -1)):
        assert L.zen_hip_repsim_set_params(rs._h, t, d, k, hp) == BAD
    # the kernels alone
    S, I = out.ptr, ints.ptr
    assert L.zen_hip_repsim_similarity_device(inp.ptr, 10, 4, 3, S, 10, 0, None) == BAD         # v_stride below the bins
    assert L.zen_hip_repsim_similarity_device(inp.ptr, 10, 4, 4, S, 9, 0, None) == BAD          # s_stride below m
    assert L.zen_hip_repsim_similarity_device(inp.ptr, 10, 4, 4, S, 10, 3, None) == BAD         # no such route
    assert L.zen_hip_repsim_similarity_device(inp.ptr, 10, 4, 4, S + 2, 10, 0, None) == BAD
    assert L.zen_hip_repsim_select_device(inp.ptr, 10, 9, 0.0, 1, 5, I, I + 400, None) == BAD
    assert L.zen_hip_repsim_select_device(inp.ptr, 10, 10, 0.0, 0, 5, I, I + 400, None) == BAD
    assert L.zen_hip_repsim_select_device(inp.ptr, 10, 10, 0.0, 1, 257, I, I + 400, None) == BAD
    assert L.zen_hip_repsim_gather_median_device(inp.ptr, 10, 4, 4, I, I + 400, 10, 257, S, 4, None) == BAD
    assert L.zen_hip_repsim_gather_median_device(inp.ptr, 10, 4, 4, I, I + 400, 10, 5, S, 3, None) == BAD
    with pytest.raises(zen_amd.ZenHipError) as e:
        repsim.Repsim(FS, 48)
    assert e.value.code == BAD
    zen_amd.synchronize()
    assert rs.stats() == before
    assert np.all(out.download() == SENTINEL) and np.all(ints.download() == ISENTINEL) and np.array_equal(inp.download(), x)
    assert rs.run(x)[0].shape == (n,)          # the handle is still good


def test_zen_repsim_program_writes_the_models_stems(repsim, oracle, tmp_path):
    """a family clip as an 800 Hz recording through the program's options"""
    from zen_amd.addon_build import repsim as addon
    oracle.lib()
    x = M.family_clip(2, 256, 6, 3, 24)[0]
    want = M.separate(x, 800.0, 256, 0.25, 0.3, 6, 10.0)
    assert M.distance_frames(0.3, 800.0, 128, 146) == 2
    wav, prefix = str(tmp_path / "clip.wav"), str(tmp_path / "out")
    write_wav_float32(wav, x, 800)
    r = subprocess.run([addon.build_demo(), wav, "-o", prefix, "--nfft", "256", "--highpass", "10", "--distance", "0.3", "--number", "6",
                        "--threshold", "0.25"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "frames: %d, a median over %.2f frames in the mean\n" % (want.counts.size, want.counts.mean())
    fs, bg = read_wav_pcm16(prefix + "_background.wav")
    assert fs == 800 and np.array_equal(bg, pcm16(want.background))
    assert np.array_equal(read_wav_pcm16(prefix + "_foreground.wav")[1], pcm16(want.foreground))
    r = subprocess.run([addon.build_demo(), wav, "-o", prefix, "--number", "300"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True)
    assert r.returncode == 1 and "outside 1..256" in r.stderr


def test_memcheck_is_clean_after_the_module(repsim):
    import zen_amd
    rep = zen_amd.memcheck()
    assert rep["corrupt_words"] == 0 and rep["bounds_violations"] == 0, rep["first_message"]


def test_the_longest_clip_selects_the_models_frames(repsim, oracle):
    """16384 frames of 64 samples: sixteen bands of 1024 rows, a row of S that fills 64 KiB of LDS.  The model's similarity of so
    many frames is out of a test's reach, its rows are not: 70 frames spread over the bands, the first and the last among them,
    must select what the model selects from their rows of S."""
    oracle.lib()
    n = 16383 * 32
    rng = np.random.default_rng(16384)
    x = (rng.uniform(-1, 1, n) * np.repeat(rng.uniform(0.05, 1, n // 32 + 1), 32)[:n]).astype(np.float32)
    rs = repsim.Repsim(FS, 64, 1, n, 0.0, 2.5 * 32 / FS, 9, 0.0)
    bg, fg, counts, idx = rs.run(x, selection=True)
    assert counts.shape == (16384,) and idx.shape == (16384, 9) and rs.stats()["bands"] == 16
    V = M.R.magnitude(M.R.spectra(x, 64))
    rows = np.unique(np.concatenate([np.arange(0, 16384, 257), [1023, 1024, 16382, 16383]]))
    D = np.zeros((rows.size, 16384), f32)
    diag = np.zeros(16384, f32)
    for f in range(V.shape[1]):
        D = M.fma32(V[rows, f][:, None], V[:, f][None, :], D)
        diag = M.fma32(V[:, f], V[:, f], diag)
    nrm = np.sqrt(diag).astype(f32)
    den = (nrm[rows][:, None] * nrm[None, :]).astype(f32)
    S = np.where(den > 0, D / np.where(den > 0, den, f32(1)), f32(0)).astype(f32)
    want_idx, want_counts = M.select(S, 0.0, 3, 9)
    assert np.array_equal(counts[rows], want_counts) and np.array_equal(idx[rows], want_idx)
    assert np.all(counts == 9) and np.all(np.isfinite(bg)) and np.array_equal(bits(fg), bits(x - bg))
