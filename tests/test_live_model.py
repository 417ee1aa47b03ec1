"""CPU tier of the live sessions (zen_amd/live): the contract of zen_hip_live.h as a numpy model on the oracle's streaming
engine (tests/live_model.py) equals oracle.HPRIOffline.process of the whole clip, bit for bit, whatever the push sizes; the
same model with zeros in place of the kept tail does not; the delivery counts are the closed form of the header; the float
padder never asks for fewer blocks than a stream below the bound has already run; the header is C99; every function it
declares is exported by libzen_hip_live.so and bound in zen_amd/live.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import live_model as M  # noqa: E402
import ragged_model as R  # noqa: E402

HDR = os.path.join(ROOT, "zen_amd", "live", "zen_hip_live.h")
CASES = M.cases()

_refs = {}


def reference(oracle, hop_h, hop_p, n, soft=False, sse=False, seed=0):
    """(clip, harm, perc): the clip of n samples, and what the oracle's HPRIOffline gives for the whole of it"""
    key = (hop_h, hop_p, n, soft, sse, seed)
    if key not in _refs:
        x = M.clip(n, seed)
        h, p = R.oracle_per_clip(oracle, hop_h, hop_p, [x], soft=soft, sse=sse)
        _refs[key] = (x, h[0], p[0])
    return _refs[key]


# ---- the model against the oracle -----------------------------------------------------------------------------------------
def test_there_are_36_cases():
    assert len(CASES) == 36 and len({M.case_id(c) for c in CASES}) == 36
    assert all(sum(c[3]) == c[2] for c in CASES)
    assert any(0 in c[3] for c in CASES), "no push of nothing among the random sizes"


@pytest.mark.parametrize("case", CASES, ids=M.case_id)
def test_model_equals_the_oracle_on_the_whole_clip(oracle, case):
    hop_h, hop_p, n, pushes, soft, sse = case
    x, rh, rp = reference(oracle, hop_h, hop_p, n, soft, sse)
    model = M.LiveModel(oracle, hop_h, hop_p, soft=soft, sse=sse)
    harm, perc, dry, counts = M.run(model, x, pushes)
    assert harm.size == n and perc.size == n
    assert np.array_equal(harm, rh), "harmonic differs"
    assert np.array_equal(perc, rp), "percussive differs"
    assert np.array_equal(dry, x), "dry is not the input"
    assert n < hop_h or np.any(perc != 0)
    # what every call handed out: the closed form, and never more than the header promises for finish
    at = 0
    for m, got in zip(pushes, counts):
        assert got == M.delivered_after(at + m, hop_h, model.latency) - M.delivered_after(at, hop_h, model.latency)
        at += m
    assert counts[-1] == n - M.delivered_after(n, hop_h, model.latency) <= model.latency + hop_h


@pytest.mark.parametrize("n", (3072, 2049))
def test_zeros_in_place_of_the_kept_tail_differ(oracle, n):
    """the lengths that see the splice at (1024, 256): pass 2 must read the last sh1 samples of Q a second time"""
    x, rh, rp = reference(oracle, 1024, 256, n)
    harm, perc, _, _ = M.run(M.LiveModel(oracle, 1024, 256, keep_tail=False), x, M.random_pushes(n, 1024, 7))
    assert np.array_equal(harm, rh)                          # pass 1 does not see the splice
    assert not np.array_equal(perc, rp)
    harm, perc, _, _ = M.run(M.LiveModel(oracle, 1024, 256), x, M.random_pushes(n, 1024, 7))
    assert np.array_equal(harm, rh) and np.array_equal(perc, rp)


def test_a_second_stream_after_finish_and_after_reset(oracle):
    x, rh, rp = reference(oracle, 256, 64, 5123)
    model = M.LiveModel(oracle, 256, 64)
    M.run(model, M.clip(1999, 3), [1000, 999])
    model.push(x[:700])
    model.reset()
    harm, perc, dry, _ = M.run(model, x, M.fixed_pushes(5123, 300))
    assert np.array_equal(harm, rh) and np.array_equal(perc, rp) and np.array_equal(dry, x)


def test_counts_for_random_push_sequences():
    """produces / pending are host arithmetic on (pushed, delivered): the closed form for every prefix of a random sequence"""
    rng = np.random.default_rng(11)
    for hop_h, lat in ((4096, 4096 + 2816), (1024, 5888), (256, 11 * 256 + 11 * 64), (128, 0)):
        pushed = delivered = 0
        for m in rng.integers(0, 3 * hop_h, 200):
            m = int(m)
            produces = M.delivered_after(pushed + m, hop_h, lat) - delivered
            assert 0 <= produces <= m + hop_h - 1
            pushed, delivered = pushed + m, delivered + produces
            pending = pushed - delivered
            assert delivered == max(0, pushed // hop_h * hop_h - lat)
            assert pushed % hop_h <= pending < lat + hop_h
        # pushes of exactly hop_h: nothing until the latency has gone by, hop_h per call from then on
        got = [M.delivered_after((k + 1) * hop_h, hop_h, lat) - M.delivered_after(k * hop_h, hop_h, lat) for k in range(40)]
        first = lat // hop_h
        assert not any(got[:first]) and got[first] == (first + 1) * hop_h - lat and all(g == hop_h for g in got[first + 1:])


# ---- the float padder's bound -----------------------------------------------------------------------------------------------
def blocks_asked(n, hop):
    """ceilf((float)n / (float)hop) of hps.cu:109-126, for an array of lengths"""
    return np.ceil(n.astype(np.float32) / np.float32(hop)).astype(np.int64)


@pytest.fixture(scope="module")
def live_so():
    from zen_amd.addon_build import live as addon
    if not os.path.exists(addon.OUT):
        addon.build()
    return addon.OUT


@pytest.mark.parametrize("hops", ((4096, 256), (1024, 256), (256, 64), (128, 128), (16384, 32), (768, 256), (384, 192), (300, 100)),
                         ids=lambda h: "%dx%d" % h)
def test_below_the_bound_the_padder_never_asks_for_fewer_blocks_than_have_run(live_so, hops):
    """finish needs floor(n / hop) <= ceilf((float)n / (float)hop) for both hops (zen_hip_live.h, "The bound").  Checked at
    every block boundary's neighbourhood for block counts around every power of two, at the float spacing changes, at the
    bound itself and at random lengths; and just beyond the bound of a power-of-two hop a length exists that breaks it."""
    from zen_amd import live
    hop_h, hop_p = hops
    bound = live.max_samples(hop_h, hop_p)
    pow2 = hop_p & (hop_p - 1) == 0
    assert bound == ((1 << 24) * hop_p - 1 if pow2 else 1 << 24)
    rng = np.random.default_rng(hop_h + hop_p)
    for hop in (hop_h, hop_p):
        ks = [0, 1, 2, 3]
        for e in range(2, 41):
            ks += [(1 << e) + d for d in (-3, -2, -1, 0, 1, 2, 3)] + [3 << (e - 1), (3 << (e - 1)) + 1]
        ks += [int(k) for k in rng.integers(0, bound // hop + 1, 20000)]
        ks += [bound // hop - d for d in range(0, 2000)]
        k = np.array(sorted({k for k in ks if 0 <= k}), dtype=np.int64)
        offs = np.array([-3, -2, -1, 0, 1, 2, 3, hop // 2, hop - 1], dtype=np.int64)
        n = (k[:, None] * hop + offs[None, :]).reshape(-1)
        n = np.concatenate([n, rng.integers(0, bound + 1, 200000), 2 ** np.arange(0, 41) + 1, 2 ** np.arange(1, 41) - 1,
                            np.array([bound, bound - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 1025])])
        n = np.unique(n[(n >= 0) & (n <= bound)])
        assert n[-1] == bound
        run, asked = n // hop, blocks_asked(n, hop)
        bad = np.flatnonzero(run > asked)
        assert bad.size == 0, "n = %d: %d blocks of %d have run, the padder asks for %d" % (n[bad[0]], run[bad[0]], hop, asked[bad[0]])
    if pow2:
        # (float)(2^24 * hop_p + hop_p) ties to even, down to 2^24 * hop_p: one block fewer than have run
        n = np.array([(1 << 24) * hop_p + hop_p], dtype=np.int64)
        assert n[0] > bound and n[0] // hop_p == blocks_asked(n, hop_p)[0] + 1


def test_above_two_to_the_24_the_padder_can_lose_a_block_below_the_true_ceiling():
    """the case the GPU tier runs: n = 2^24 + 1025 at (1024, 256): (float)n = n - 1, both padders ask for one block fewer than
    the true ceiling -- and still for no fewer than have run"""
    n = (1 << 24) + 1025
    assert int(np.float32(n)) == n - 1
    for hop in (1024, 256):
        asked = int(blocks_asked(np.array([n]), hop)[0])
        assert asked == -(-n // hop) - 1 and asked >= n // hop


# ---- the boundary -----------------------------------------------------------------------------------------------------------
def declared_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zen_hip_live_[a-z0-9_]+)\s*\(", hdr)))


def test_header_symbols_are_bound_and_exported(live_so):
    from zen_amd import lib, live
    L = ctypes.CDLL(live_so)
    names = declared_symbols()
    wanted = ["create", "destroy", "set_stream", "use_sse_filter", "use_soft_mask", "reset", "latency", "produces", "pending",
              "push_device", "finish_device", "push_host", "finish_host", "stats", "profile", "profile_get", "profile_get_engine",
              "last_error", "version"]
    assert all("zen_hip_live_" + w in names for w in wanted)
    for n in names:
        assert hasattr(L, n), "libzen_hip_live.so does not export %s" % n
    assert set(names) == {s[0] for s in live.SYMBOLS}
    assert not any(s[0].startswith("zen_hip_live") for s in lib.SYMBOLS)


def test_library_loads_without_gpu_and_checks_arguments_first(live_so):
    from zen_amd import live
    L = live.load()
    assert b"gfx950" in L.zen_hip_live_version()
    assert L.zen_hip_live_push_device(None, None, 0, 0, None, None, None, 0, None) == 2
    assert b"null" in L.zen_hip_live_last_error()
    assert L.zen_hip_live_finish_host(None, None, None, None, 0, None) == 2
    assert L.zen_hip_live_produces(None, 1, None) == 2 and L.zen_hip_live_reset(None) == 2
    h = ctypes.c_void_p()
    assert L.zen_hip_live_create(44100.0, 1024, 768, 2.0, 2.0, 0, 1, 0, ctypes.byref(h)) == 3      # hops not divisible
    assert L.zen_hip_live_create(44100.0, 1024, 256, 2.0, 2.0, 0, 0, 0, ctypes.byref(h)) == 2      # zero streams
    out = ctypes.c_ulonglong()
    assert L.zen_hip_live_max_samples(1024, 768, ctypes.byref(out)) == 3
    assert L.zen_hip_live_destroy(None) == 0


def test_library_finds_the_engine_library_beside_itself(live_so):
    out = subprocess.run(["readelf", "-d", live_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    assert "libzen_hip.so" in out and "$ORIGIN" in out


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "zen_hip_live.h"\nint main(void){zen_hip_live_t h = 0; zen_hip_live_stats_t s; s.pushed = 0;'
                   ' return h != 0 || s.pushed || ZEN_HIP_OK;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.dirname(HDR), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_kernels_add_without_contraction_or_fast_math():
    from zen_amd.addon_build import live as addon
    assert "-ffp-contract=off" in addon.FLAGS and "-fno-fast-math" in addon.FLAGS
    assert not any("fast-math" in f and f != "-fno-fast-math" for f in addon.FLAGS)
