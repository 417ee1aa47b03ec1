"""GPU tier: libzen_hip_nmf.so (zen_amd/nmf) -- supervised NMF of the magnitude spectrogram on device rows.  Tolerance 0
everywhere: the three products on both routes (the matrix cores and the vector ALU), the dictionaries, the activations and the
stems are compared bit for bit against tests/nmf_model.py.  NaNs stand around the inputs (a kernel that read outside the
elements of its call would carry them into a result) and sentinels around every output."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import nmf_model as M  # noqa: E402
from test_gpu_repet import pcm16, read_wav_pcm16, write_wav_float32  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
FS = M.FAMILY_FS
BAD = 2
f32 = np.float32


@pytest.fixture(scope="module")
def nmf():
    """The library of this feature, built on demand (the session fixture of conftest.py builds the one it links against)."""
    import zen_amd
    from zen_amd import nmf as mod
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


def round4(v):
    return (v + 3) & ~3


class Rows:
    """A matrix in device memory as a layout has it: `lead` floats in front, rows `stride` apart, `fill` everywhere else"""

    def __init__(self, A, layout, fill=np.nan):
        import zen_amd
        pad, self.lead = LAYOUTS[layout]
        self.rows, self.cols = A.shape
        self.stride = round4(self.cols) + pad if layout.startswith("padded") else self.cols + pad
        self.host = np.full(self.lead + self.rows * self.stride + 8, fill, f32)
        for r in range(self.rows):
            self.host[self.lead + r * self.stride:self.lead + r * self.stride + self.cols] = A[r]
        self.dev = zen_amd.DeviceBuffer.from_host(self.host)
        self.ptr = self.dev.offset(self.lead)

    def untouched(self):
        return np.array_equal(bits(self.dev.download()), bits(self.host))

    def block(self, sentinel=SENTINEL):
        """the matrix as it is now, everything around it still the sentinel"""
        got = self.dev.download()
        end = self.lead + self.rows * self.stride
        still = np.isnan if sentinel != sentinel else (lambda a: a == sentinel)
        assert np.all(still(got[:self.lead])) and np.all(still(got[end:]))
        b = got[self.lead:end].reshape(self.rows, self.stride)
        assert np.all(still(b[:, self.cols:])), "written beyond the elements of a row"
        return b[:, :self.cols].copy()


# padding behind a row (on top of the round-up to 4 for the padded ones) and floats in front of the first row
LAYOUTS = {"tight": (0, 0), "padded": (4, 0), "padded_off16": (4, 1), "tight_off16": (0, 2), "odd_stride": (3, 0)}

# ================================================================================================ the three products alone
# (K, F, m): every K in {1, 2, 3, 31, 32, 33, 64, 65, 255, 256}, F in {1, 2, 33, 129, 255, 256, 257, 513} and m in {1, 2, 31,
# 33, 127, 128, 129, 255, 256, 257, 513} is there: both sides of the tiles (32, 128) and of the segment (256) in every
# product's reduction and outputs.  Two triples are large in more than one dimension.
TRIPLES = ((1, 1, 1), (2, 2, 255), (3, 33, 31), (31, 129, 33), (32, 255, 127), (33, 256, 128), (64, 257, 129), (65, 513, 255), (255, 33, 256),
           (256, 257, 513), (3, 129, 513), (2, 513, 2), (2, 1, 257))
KINDS = ("uniform", "palette", "scaled")
PALETTE = f32([0, 0, 0, 0.25, 0.5, 1, 1, 0.75])
SCALES = f32([1e-44, 1e-38, 1e-30, 1e-19, 1e-8, 1.0])
_cache = {}


def values(kind, K, F, m):
    """V, W, H, an arbitrary Q and the model's results, computed once per case.  `uniform`: (0, 1]; `palette`: eight levels
    with zeros, an all-zero spectrum, an all-zero activation row and an all-zero frame and bin, where the clamps act and sums
    tie; `scaled`: rows scaled down to the denormals, whose products underflow."""
    key = (kind, K, F, m)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(1000 * KINDS.index(kind) + 7 * K + 3 * F + m)

    def draw(rows, cols):
        if kind == "palette":
            A = PALETTE[rng.integers(0, 8, (rows, cols))]
            A[rows // 2] = 0
            A[:, cols // 3] = 0
            return A
        A = (1.0 - rng.uniform(0, 1, (rows, cols))).astype(f32)
        if kind == "scaled":
            A = (A * SCALES[rng.integers(0, SCALES.size, rows)][:, None]).astype(f32)
        return A
    V, W, H, Q = draw(m, F), draw(K, F), draw(K, m), draw(m, F)
    if kind != "scaled":
        Q = (Q * f32(3)).astype(f32)
    want = {"ratio": M.ratio(V, W, H), "update_h": M.update_h(W, Q, H), "update_w": M.update_w(H, Q, W, 0)}
    _cache[key] = (V, W, H, Q, want)
    return _cache[key]


def products_case(nmf, kind, layout, K, F, m):
    import zen_amd
    V, W, H, Q, want = values(kind, K, F, m)
    v, w, h, q = (Rows(A, layout) for A in (V, W, H, Q))
    what = "%s %s K %d F %d m %d" % (kind, layout, K, F, m)
    got = {}
    for route in (nmf.ROUTE_MFMA, nmf.ROUTE_VALU):
        qo, lo = Rows(np.full((m, F), SENTINEL, f32), layout, SENTINEL), Rows(np.full((m, F), SENTINEL, f32), layout, SENTINEL)
        nmf.ratio_device(v, v.stride, w, w.stride, h, h.stride, K, F, m, qo, qo.stride, lo, lo.stride, route)
        qn = Rows(np.full((m, F), SENTINEL, f32), layout, SENTINEL)
        nmf.ratio_device(v, v.stride, w, w.stride, h, h.stride, K, F, m, qn, qn.stride, None, 0, route)
        ho = Rows(np.full((K, m), SENTINEL, f32), layout, SENTINEL)
        nmf.update_h_device(w, w.stride, q, q.stride, h, h.stride, K, F, m, ho, ho.stride, route)
        outs = {}
        for fixed in sorted({0, 1, K - 1, K}):
            outs[fixed] = Rows(np.full((K, F), SENTINEL, f32), layout, SENTINEL)
            nmf.update_w_device(h, h.stride, q, q.stride, w, w.stride, K, F, m, fixed, outs[fixed], outs[fixed].stride, route)
        zen_amd.synchronize()
        name = ("the matrix-core route: " if route == nmf.ROUTE_MFMA else "the vector route: ") + what
        got[route] = (qo.block(), lo.block(), ho.block(), outs[0].block())
        assert_same_bits(got[route][0], want["ratio"][0], "Q, " + name)
        assert_same_bits(got[route][1], want["ratio"][1], "L, " + name)
        assert_same_bits(qn.block(), want["ratio"][0], "Q without L, " + name)
        assert_same_bits(got[route][2], want["update_h"], "H', " + name)
        for fixed, o in outs.items():
            full = o.block()
            assert np.all(full[:fixed] == SENTINEL), "a held row was written: fixed %d, %s" % (fixed, name)
            assert_same_bits(full[fixed:], want["update_w"][fixed:], "W' from row %d, %s" % (fixed, name))
    for a, b, n in zip(got[nmf.ROUTE_MFMA], got[nmf.ROUTE_VALU], ("Q", "L", "H'", "W'")):
        assert_same_bits(a, b, "the two routes, %s: %s" % (n, what))
    assert v.untouched() and w.untouched() and h.untouched() and q.untouched(), "an input was written: " + what
    if kind == "palette" and K >= 2:          # the clamps: an all-zero spectrum divides by eps and stays +0
        assert np.all(bits(got[nmf.ROUTE_MFMA][2][K // 2]) == 0) and np.all(bits(got[nmf.ROUTE_MFMA][3][K // 2]) == 0)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind", KINDS)
def test_products_alone_both_routes(nmf, kind, layout):
    """strides padded to 16 bytes take the 16-byte loads, the others single words; the model's results are cached per case"""
    for K, F, m in TRIPLES:
        products_case(nmf, kind, layout, K, F, m)


def test_products_default_route_and_in_place(nmf):
    """the default route, and the updates with the output on the input as a session runs them"""
    import zen_amd
    K, F, m = 33, 129, 130
    V, W, H, Q, want = values("uniform", K, F, m)
    v, w, h, q = (Rows(A, "padded") for A in (V, W, H, Q))
    qo = Rows(np.full((m, F), SENTINEL, f32), "padded", SENTINEL)
    nmf.ratio_device(v, v.stride, w, w.stride, h, h.stride, K, F, m, qo, qo.stride)
    nmf.update_h_device(w, w.stride, q, q.stride, h, h.stride, K, F, m, h, h.stride)
    zen_amd.synchronize()
    assert_same_bits(qo.block(), want["ratio"][0], "Q on the default route")
    assert_same_bits(h.block(np.nan), want["update_h"], "H' in place")
    h2 = Rows(H, "padded")
    nmf.update_w_device(h2, h2.stride, q, q.stride, w, w.stride, K, F, m, 2, w, w.stride)
    zen_amd.synchronize()
    got_w = w.block(np.nan)
    assert_same_bits(got_w[:2], W[:2], "the held rows")
    assert_same_bits(got_w[2:], want["update_w"][2:], "W' in place")


# ================================================================================================ the whole call
N = 256
HOP = N // 2
KF = 2 * M.FAMILY_COMPONENTS


@pytest.fixture(scope="module")
def clips(oracle):
    """three mixtures of the family at frame 256 with spectra and magnitudes, and two dictionaries (a few iterations of the
    model on a training clip each)"""
    oracle.lib()
    x = np.stack([M.family_clip(seed, N)[0] for seed in range(3)])
    dicts = [M.train(M.family_source(w, 0, N, 0), N, M.FAMILY_COMPONENTS, 5, seed=w) for w in (0, 1)]
    return x, np.concatenate(dicts)


_process_cache = {}


def model_process(x, W, H, fixed, iterations, groups, n_groups):
    key = (x.tobytes(), W.tobytes(), H.tobytes(), fixed, iterations, None if groups is None else tuple(groups), n_groups)
    if key not in _process_cache:
        _process_cache[key] = M.process(x, N, W, H, fixed, iterations, groups, n_groups)
    return _process_cache[key]


def run_device(session, x, W, H, fixed, iterations, groups=None, n_groups=0, layout="tight", shared_w=False):
    """x (C, n), W (C, K, F) or (K, F) shared, H (C, K, m).  Returns (W, H, stems) as the call left them."""
    import zen_amd
    C, n = x.shape
    K, m = H.shape[1], H.shape[2]
    F = W.shape[-1]
    xin = Rows(x, layout)
    w = Rows(W.reshape(-1, F), layout)
    h = Rows(H.reshape(-1, m), layout)
    G = n_groups if groups is not None else 0
    out = Rows(np.full((max(G, 1) * C, n), SENTINEL, f32), layout, SENTINEL)
    session.process_device(xin, xin.stride, n, w, w.stride, 0 if shared_w else K * w.stride, h, h.stride, K * h.stride, fixed, iterations, groups,
                           n_groups, out if groups is not None else None, out.stride)
    zen_amd.synchronize()
    assert xin.untouched(), "the input was written"
    wb, hb, sb = w.block(np.nan), h.block(np.nan), out.block()
    if groups is None:
        assert np.all(sb == SENTINEL)
    return wb.reshape(W.shape), hb.reshape(H.shape), sb.reshape(max(G, 1), C, n) if groups is not None else None


def start(seed, m, K=KF, F=HOP + 1):
    return M.init(seed, K * F).reshape(K, F), M.init(seed + 1, K * m).reshape(K, m)


@pytest.mark.parametrize("iterations", [0, 1, 7])
@pytest.mark.parametrize("fixed", [0, KF], ids=["free", "held"])
def test_one_clip_against_the_model(nmf, clips, iterations, fixed):
    x, D = clips
    m = M.R.n_frames(x.shape[1], HOP)
    W0, H0 = start(5, m)
    if fixed:
        W0 = D
    groups = [0] * 6 + [1] * 6
    want = model_process(x[0], W0, H0, fixed, iterations, groups, 2)
    s = nmf.Nmf(FS, N, KF, 1, x.shape[1])
    W, H, stems = run_device(s, x[:1], W0[None], H0[None], fixed, iterations, groups, 2, "padded" if iterations == 1 else "tight")
    assert_same_bits(W[0], want.W, "W")
    assert_same_bits(H[0], want.H, "H")
    assert_same_bits(stems[:, 0], want.stems, "stems")
    if fixed:
        assert_same_bits(W[0], D, "held spectra")
    if iterations == 7:
        assert np.abs(stems.sum(0)[0] - x[0]).max() < 1e-4, "two groups that hold every component add up to the clip"


def test_three_clips_in_one_call_are_each_the_clip_alone(nmf, clips):
    x, D = clips
    m = M.R.n_frames(x.shape[1], HOP)
    groups = [0] * 6 + [1] * 6
    s = nmf.Nmf(FS, N, KF, 3, x.shape[1] + 50)
    # free: a dictionary per clip, odd strides and leads
    WH = [start(10 + c, m) for c in range(3)]
    W, H, stems = run_device(s, x, np.stack([a for a, _ in WH]), np.stack([b for _, b in WH]), 3, 2, groups, 2, "padded_off16")
    for c in range(3):
        want = model_process(x[c], WH[c][0], WH[c][1], 3, 2, groups, 2)
        assert_same_bits(W[c], want.W, "W of clip %d" % c)
        assert_same_bits(H[c], want.H, "H of clip %d" % c)
        assert_same_bits(stems[:, c], want.stems, "stems of clip %d" % c)
    # held: one dictionary for all of them
    W, H, stems = run_device(s, x, D, np.stack([b for _, b in WH]), KF, 2, groups, 2, "odd_stride", shared_w=True)
    assert_same_bits(W, D, "the shared dictionary")
    for c in range(3):
        want = model_process(x[c], D, WH[c][1], KF, 2, groups, 2)
        assert_same_bits(H[c], want.H, "H of clip %d under the shared dictionary" % c)
        assert_same_bits(stems[:, c], want.stems, "stems of clip %d under the shared dictionary" % c)
    st = s.stats()
    assert st["calls"] == 2 and st["clips"] == 6 and st["iterations"] == 12


def test_groups_a_component_in_no_stem_and_a_fit_only_call(nmf, clips):
    x, D = clips
    m = M.R.n_frames(x.shape[1], HOP)
    _, H0 = start(7, m)
    s = nmf.Nmf(FS, N, KF, 1, x.shape[1])
    for groups, G in (([0] * 5 + [-1] + [0] * 6, 1), ([0, 1] * 5 + [-1, 1], 2), (list(range(KF)), KF), ([-1] * 11 + [3], KF)):
        want = model_process(x[1], D, H0, KF, 2, groups, G)
        W, H, stems = run_device(s, x[1:2], D[None], H0[None], KF, 2, groups, G, "tight_off16")
        assert_same_bits(H[0], want.H, "H with %d groups" % G)
        assert_same_bits(stems[:, 0], want.stems, "stems with %d groups" % G)
    assert np.all(stems[:3] == 0), "a group without a component is silent"
    W, H, stems = run_device(s, x[1:2], D[None], H0[None], KF, 2)
    assert stems is None
    assert_same_bits(H[0], want.H, "H of a fit alone")


def test_vector_route_session_and_host_call_equal_the_device_call(nmf, clips, monkeypatch):
    import zen_amd
    x, D = clips
    m = M.R.n_frames(x.shape[1], HOP)
    W0, H0 = start(3, m)
    groups = [0] * 6 + [1] * 5 + [-1]
    want = model_process(x[2], W0, H0, 4, 3, groups, 2)
    monkeypatch.setenv("ZEN_HIP_NMF", "mfma=0")
    sv = nmf.Nmf(FS, N, KF, 1, x.shape[1])
    monkeypatch.delenv("ZEN_HIP_NMF")
    sm = nmf.Nmf(FS, N, KF, 1, x.shape[1])
    zen_amd.synchronize()
    st0, mc0 = sm.stats(), zen_amd.memcheck()
    assert st0["allocations"] == 10 and st0["calls"] == 0
    for s, route in ((sv, "valu"), (sm, "mfma")):
        s.profile(True)
        W, H, stems = run_device(s, x[2:3], W0[None], H0[None], 4, 3, groups, 2)
        prof = s.profile_get()
        assert list(prof) == list(nmf.KERNELS)
        other = "mfma" if route == "valu" else "valu"
        assert prof["ratio_" + route]["launches"] == 6 and prof["update_h_" + route]["launches"] == 3 and prof["update_w_" + route]["launches"] == 3
        assert all(prof[k + other]["launches"] == 0 for k in ("ratio_", "update_h_", "update_w_"))
        assert prof["mask"]["launches"] == 2 and prof["ifft"]["launches"] == 2 and prof["overlap_add"]["launches"] == 2 and prof["fft"]["ms"] > 0
        s.profile(False)
        assert_same_bits(W[0], want.W, "W on " + route)
        assert_same_bits(H[0], want.H, "H on " + route)
        assert_same_bits(stems[:, 0], want.stems, "stems on " + route)
    W, H, stems = sm.run(x[2], W0, H0, 4, 3, groups, 2)
    assert_same_bits(W, want.W, "W of the host call")
    assert_same_bits(H, want.H, "H of the host call")
    assert_same_bits(stems, want.stems, "stems of the host call")
    zen_amd.synchronize()
    st1, mc1 = sm.stats(), zen_amd.memcheck()
    assert st1["allocations"] == st0["allocations"] and st1["device_bytes"] == st0["device_bytes"] and st1["calls"] == 2
    if mc1["redzone_bytes"]:
        assert mc1["live_allocations"] == mc0["live_allocations"] and mc1["corrupt_words"] == 0


@pytest.mark.parametrize("n", [1, HOP - 1, HOP, HOP + 1])
def test_the_shortest_clips(nmf, oracle, n):
    oracle.lib()
    x = np.random.default_rng(n).uniform(-1, 1, n).astype(f32)
    m = M.R.n_frames(n, HOP)
    W0, H0 = start(n, m, 3)
    want = model_process(x, W0, H0, 1, 2, [0, 1, 1], 2)
    W, H, stems = run_device(nmf.Nmf(FS, N, 3, 1, HOP + 1), x[None], W0[None], H0[None], 1, 2, [0, 1, 1], 2, "tight_off16")
    assert_same_bits(W[0], want.W, "W")
    assert_same_bits(H[0], want.H, "H")
    assert_same_bits(stems[:, 0], want.stems, "stems")


@pytest.mark.parametrize("route", ["mfma", "valu"])
@pytest.mark.parametrize("frame,n", [(1024, 5 * 512 + 37), (64, 599 * 32 - 5)], ids=["513_bins", "600_frames"])
def test_reductions_split_by_segments_over_workgroups(nmf, oracle, monkeypatch, route, frame, n):
    """A session splits an update whose reduction has more than one segment over workgroups and adds the segments' sums in
    order: 513 bins are three segments in the update of H, 600 frames three (the last of 88) in the update of W; two of five
    spectra are held, so the rows of the product start behind them.  The kernels alone (above) walk the same segments in
    sequence; both are the model's bits."""
    oracle.lib()
    x = np.random.default_rng(frame).uniform(-1, 1, n).astype(f32)
    m = M.R.n_frames(n, frame // 2)
    assert (frame, m) in ((1024, 7), (64, 600))
    W0, H0 = start(frame, m, 5, frame // 2 + 1)
    groups = [0, 0, 1, 1, -1]
    want = M.process(x, frame, W0, H0, 2, 2, groups, 2)
    monkeypatch.setenv("ZEN_HIP_NMF", "mfma=%d" % (route == "mfma"))
    s = nmf.Nmf(FS, frame, 5, 1, n)
    W, H, stems = run_device(s, x[None], W0[None], H0[None], 2, 2, groups, 2, "padded")
    assert_same_bits(W[0], want.W, "W")
    assert_same_bits(H[0], want.H, "H")
    assert_same_bits(stems[:, 0], want.stems, "stems")
    # the same updates through the calls that walk the segments in sequence
    Q = M.ratio(want.V if hasattr(want, "V") else M.R.magnitude(M.R.spectra(x, frame)), W0, H0)[0]
    q, w, h = Rows(Q, "padded"), Rows(W0, "padded"), Rows(H0, "padded")
    ho, wo = Rows(np.full(H0.shape, SENTINEL, f32), "padded", SENTINEL), Rows(np.full(W0.shape, SENTINEL, f32), "padded", SENTINEL)
    r = nmf.ROUTE_MFMA if route == "mfma" else nmf.ROUTE_VALU
    nmf.update_h_device(w, w.stride, q, q.stride, h, h.stride, 5, frame // 2 + 1, m, ho, ho.stride, r)
    nmf.update_w_device(h, h.stride, q, q.stride, w, w.stride, 5, frame // 2 + 1, m, 0, wo, wo.stride, r)
    import zen_amd
    zen_amd.synchronize()
    assert_same_bits(ho.block(), M.update_h(W0, Q, H0), "H' in sequence")
    assert_same_bits(wo.block(), M.update_w(H0, Q, W0), "W' in sequence")


def test_the_binding_functions_against_the_model(nmf, clips):
    x, D = clips
    a = M.family_source(0, 1, N, 0)
    assert_same_bits(nmf.train(a, FS, 4, N, 3, seed=2), M.train(a, N, 4, 3, 2), "train")
    want = M.separate(x[0], N, [D[:6], D[6:]], 3, free=2, seed=4)
    got = nmf.separate(x[0], FS, [D[:6], D[6:]], iterations=3, free=2, seed=4)
    assert len(got) == 3
    assert_same_bits(np.stack(got), want.stems, "separate with two free components")
    W0, H0 = M.initial(1, 3, HOP + 1, M.R.n_frames(x.shape[1], HOP))
    wantd = M.process(x[1], N, W0, H0, 0, 2, [0, 1, 2], 3)
    W, H, stems = nmf.decompose(x[1], FS, 3, N, 2, seed=1)
    assert_same_bits(W, wantd.W, "decompose W")
    assert_same_bits(H, wantd.H, "decompose H")
    assert_same_bits(stems, wantd.stems, "decompose stems")


def test_the_longest_clip_one_iteration(nmf, oracle):
    """16384 frames of 64 samples, four components, one free iteration: the reductions over the frames cross 64 segments.
    With four components and 33 bins the whole model is within a test's reach, so every row and column is compared."""
    oracle.lib()
    n, K = 16383 * 32, 4
    rng = np.random.default_rng(16384)
    x = (rng.uniform(-1, 1, n) * np.repeat(rng.uniform(0.05, 1, n // 32 + 1), 32)[:n]).astype(f32)
    W0, H0 = M.initial(0, K, 33, 16384)
    V = M.R.magnitude(M.R.spectra(x, 64))
    Ww, Hw = M.fit(V, W0, H0, 1, 1)
    s = nmf.Nmf(FS, 64, K, 1, n)
    W, H, _ = s.run(x, W0, H0, 1, 1)
    assert_same_bits(H, Hw, "H of 16384 frames")
    assert_same_bits(W, Ww, "W over 64 segments")
    assert_same_bits(W[0], W0[0], "the held row")


# ================================================================================================ arguments, the program
def test_bad_arguments_are_refused_and_touch_nothing(nmf, clips):
    import zen_amd
    L = nmf.load()
    err = L.zen_hip_nmf_last_error
    x, D = clips
    n = 1000
    m = M.R.n_frames(n, HOP)
    K, F = 4, HOP + 1
    s = nmf.Nmf(FS, N, K, 2, n)
    inp = zen_amd.DeviceBuffer.from_host(np.zeros(2 * n, f32))
    w = zen_amd.DeviceBuffer.from_host(np.full(2 * K * F, SENTINEL, f32))
    h = zen_amd.DeviceBuffer.from_host(np.full(2 * K * m, SENTINEL, f32))
    out = zen_amd.DeviceBuffer.from_host(np.full(2 * 2 * n, SENTINEL, f32))
    import ctypes
    g_ok = (ctypes.c_int * K)(0, 1, -1, 0)
    good = dict(hh=s._h, i=inp.ptr, istr=n, n=n, w=w.ptr, ws=F, wcs=K * F, h=h.ptr, hs=m, hcs=K * m, fixed=0, it=1, g=g_ok, G=2, o=out.ptr, os=n)
    before = s.stats()

    def call(f, **kw):
        a = dict(good)
        a.update(kw)
        return f(a["hh"], a["i"], a["istr"], a["n"], a["w"], a["ws"], a["wcs"], a["h"], a["hs"], a["hcs"], a["fixed"], a["it"], a["g"], a["G"],
                 a["o"], a["os"])
    cases = [(dict(hh=None), b"null handle"), (dict(i=None), b"null input"), (dict(w=None), b"null input"), (dict(h=None), b"null input"),
             (dict(i=inp.ptr + 2), b"4-byte alignment"), (dict(w=w.ptr + 1), b"4-byte alignment"), (dict(o=out.ptr + 2), b"4-byte alignment"),
             (dict(n=0), b"samples per clip"), (dict(n=n + 1, istr=n + 1, os=n + 1), b"samples per clip"), (dict(istr=n - 1), b"in_stride"),
             (dict(fixed=K + 1), b"spectra held"), (dict(it=-1), b"iterations"), (dict(ws=F - 1), b"w_stride"), (dict(hs=m - 1), b"h_stride"),
             (dict(wcs=0), b"race on W"), (dict(wcs=0, fixed=K - 1), b"race on W"), (dict(wcs=K * F - 1), b"below a clip"),
             (dict(hcs=0), b"below a clip"), (dict(hcs=K * m - 1), b"below a clip"), (dict(G=0), b"groups outside 1.."),
             (dict(G=K + 1), b"groups outside 1.."), (dict(g=(ctypes.c_int * K)(0, 2, 0, 0)), b"outside -1..1"),
             (dict(g=(ctypes.c_int * K)(0, -2, 0, 0)), b"outside -1..1"), (dict(o=None), b"place for the stems"), (dict(os=n - 1), b"out_stride")]
    for kw, text in cases:
        for f in (L.zen_hip_nmf_process_device, L.zen_hip_nmf_process_host):
            assert call(f, **kw) == BAD and text in err(), (kw, err())
    with pytest.raises(zen_amd.ZenHipError) as e:
        nmf.Nmf(FS, 48)
    assert e.value.code == BAD
    with pytest.raises(zen_amd.ZenHipError):
        nmf.Nmf(FS, N, 257)
    zen_amd.synchronize()
    assert s.stats() == before
    assert np.all(w.download() == SENTINEL) and np.all(h.download() == SENTINEL) and np.all(out.download() == SENTINEL)
    # one dictionary for both clips is fine with every spectrum held, and the handle is still good
    w.upload(np.tile(M.init(1, K * F), 2))
    h.upload(M.init(2, 2 * K * m))
    assert call(L.zen_hip_nmf_process_device, wcs=0, fixed=K) == 0
    zen_amd.synchronize()
    assert np.all(np.isfinite(out.download())) and s.stats()["calls"] == 1


def peak(x):
    p = max(-x.min(), x.max())
    return (x / p).astype(f32) if p > 0 else x


def test_zen_nmf_program_trains_and_separates(nmf, oracle, tmp_path):
    """two dictionaries trained by the program from isolated clips, then the mixture through them with one free component"""
    from zen_amd.addon_build import nmf as addon
    oracle.lib()
    exe = addon.build_demo()
    a, b = M.family_source(0, 2, N, 0), M.family_source(1, 2, N, 0)
    x = M.family_clip(2, N)[0]
    paths = {k: str(tmp_path / (k + ".wav")) for k in ("a", "b", "mix")}
    for k, v in zip(("a", "b", "mix"), (a, b, x)):
        write_wav_float32(paths[k], v, 8000)
    want_d = []
    for k, v, seed in (("a", a, 3), ("b", b, 4)):
        r = subprocess.run([exe, "train", paths[k], "-o", str(tmp_path / (k + ".znmf")), "--nfft", "256", "--components", "3", "--iterations", "4",
                            "--seed", str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout == "frames: 42, 3 spectra of 129 bins after 4 iterations\n"
        want_d.append(M.train(v, N, 3, 4, seed))
        W, nfft, fs = nmf.load_znmf(str(tmp_path / (k + ".znmf")))
        assert nfft == 256 and fs == 8000.0
        assert_same_bits(W, want_d[-1], "the dictionary of " + k)
    prefix = str(tmp_path / "out")
    r = subprocess.run([exe, "separate", paths["mix"], "-d", str(tmp_path / "a.znmf"), "-d", str(tmp_path / "b.znmf"), "-o", prefix, "--free", "1",
                        "--iterations", "3", "--seed", "9"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "frames: 42, 6 spectra held and 1 learned, 3 stems after 3 iterations\n"
    want = M.separate(x, N, want_d, 3, free=1, seed=9)
    for g in range(3):
        fs, got = read_wav_pcm16(prefix + "_%d.wav" % g)
        assert fs == 8000 and np.array_equal(got, pcm16(peak(want.stems[g]))), "stem %d" % g
    assert not os.path.exists(prefix + "_3.wav")
    r = subprocess.run([exe, "separate", paths["mix"], "-d", paths["a"], "-o", prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True)
    assert r.returncode == 1 and "no .znmf file" in r.stderr


def test_memcheck_is_clean_after_the_module(nmf):
    import zen_amd
    rep = zen_amd.memcheck()
    assert rep["corrupt_words"] == 0 and rep["bounds_violations"] == 0, rep["first_message"]
