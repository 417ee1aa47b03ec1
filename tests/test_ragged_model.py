"""CPU tier of the ragged offline batches (zen_amd/ragged): the splice mapping of zen_hip_ragged.h as a numpy model on the
oracle's streaming engine equals oracle.HPRIOffline.process of every clip alone, bit for bit; the same model without the
splice does not, on the lengths the GPU tier uses; the header is C99; every function it declares is exported by
libzen_hip_ragged.so and bound in zen_amd/ragged.py; plan_groups against brute force."""
import ctypes
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ragged_model as M  # noqa: E402

HDR = os.path.join(ROOT, "zen_amd", "ragged", "zen_hip_ragged.h")


def lengths_for(hop_h, hop_p):
    return [1, hop_p - 1, hop_h, hop_h + 1, 3 * hop_h - 1, 3 * hop_h, 7 * hop_h + hop_p + 3, 20 * hop_h - 5, 20 * hop_h,
            33 * hop_h + 17]


# ---- the model against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", (False, True), ids=("hard", "soft"))
@pytest.mark.parametrize("hops", ((256, 64), (512, 128), (128, 128)), ids=lambda h: "%dx%d" % h)
def test_splice_model_equals_the_oracle_per_clip(oracle, hops, soft):
    hop_h, hop_p = hops
    lens = lengths_for(hop_h, hop_p)
    clips = M.clips_for(lens)
    harm, perc = M.ragged_model(oracle, hop_h, hop_p, clips, soft=soft)
    rh, rp = M.oracle_per_clip(oracle, hop_h, hop_p, clips, soft=soft)
    for n, a, b, c, d in zip(lens, harm, rh, perc, rp):
        assert a.size == n and c.size == n
        assert np.array_equal(a, b), "harmonic differs for the clip of %d samples" % n
        assert np.array_equal(c, d), "percussive differs for the clip of %d samples" % n
        assert n < hop_h or np.any(c != 0)


def test_the_lengths_cover_short_clips_and_long_second_passes(oracle):
    """clips shorter than lag_h hops (padded1 < 2 * sh1: an in-place "copy from j - sh1" would read before the row), and clips
    whose padded pass-2 length exceeds their padded pass-1 length"""
    short, long2 = 0, 0
    for hop_h, hop_p in ((256, 64), (512, 128), (128, 128)):
        lag_h = oracle.HPR(M.FS, hop_h, 2.0, oracle.OUTPUT_PERCUSSIVE, oracle.TIME_ANTICAUSAL).lag
        lag_p = oracle.HPR(M.FS, hop_p, 2.0, oracle.OUTPUT_PERCUSSIVE, oracle.TIME_ANTICAUSAL).lag
        for n in lengths_for(hop_h, hop_p):
            p1, p2 = M.padded(n, hop_h, lag_h), M.padded(n, hop_p, lag_p)
            assert (p1 // hop_h, p1) == oracle.chunk_padder(n, hop_h, lag_h)
            assert (p2 // hop_p, p2) == oracle.chunk_padder(n, hop_p, lag_p)
            short += p1 < 2 * lag_h * hop_h
            long2 += p2 > p1
    assert short > 0 and long2 > 0, (short, long2)


@pytest.mark.parametrize("soft", (False, True), ids=("hard", "soft"))
def test_gpu_tier_lengths_at_1024_256(oracle, soft):
    """the batch tests/test_gpu_ragged.py runs, on the model: equal to the oracle with the splice"""
    lens = [1, 255, 1024, 2049, 2559, 2816, 3071, 3072, 7 * 1024 + 259, 12 * 1024 + 17, 0]
    clips = M.clips_for(lens)
    harm, perc = M.ragged_model(oracle, 1024, 256, clips, soft=soft)
    rh, rp = M.oracle_per_clip(oracle, 1024, 256, clips, soft=soft)
    for n, a, b, c, d in zip(lens, harm, rh, perc, rp):
        assert np.array_equal(a, b) and np.array_equal(c, d), n


def test_without_the_splice_the_fixture_lengths_differ(oracle):
    """plain zero padding (every row handled as a clip of the longest length) is NOT the clip alone: the lengths of the GPU
    tier see the per-clip splice point"""
    lens = [3072, 2049, 12 * 1024 + 17]
    clips = M.clips_for(lens)
    harm, perc = M.ragged_model(oracle, 1024, 256, clips, splice=False)
    rh, rp = M.oracle_per_clip(oracle, 1024, 256, clips)
    for i in (0, 1):
        assert np.array_equal(harm[i], rh[i])                    # pass 1 does not see the splice
        assert not np.array_equal(perc[i], rp[i]), lens[i]
        first = int(np.flatnonzero(perc[i] != rp[i])[0])
        assert first >= 1536, (lens[i], first)                   # nothing before the stale tail can reach differs
    assert np.array_equal(perc[2], rp[2])                        # the longest clip is its own padding


# ---- the boundary -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged_so():
    from zen_amd.addon_build import ragged as addon
    if not os.path.exists(addon.OUT):
        addon.build()
    return addon.OUT


def declared_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zen_hip_ragged_[a-z0-9_]+)\s*\(", hdr)))


def test_header_symbols_are_bound_and_exported(ragged_so):
    from zen_amd import lib, ragged
    L = ctypes.CDLL(ragged_so)
    names = declared_symbols()
    assert len(names) >= 9 and "zen_hip_ragged_process_device" in names and "zen_hip_ragged_process_host" in names
    for n in names:
        assert hasattr(L, n), "libzen_hip_ragged.so does not export %s" % n
    assert set(names) == {s[0] for s in ragged.SYMBOLS}
    assert not any(s[0].startswith("zen_hip_ragged") for s in lib.SYMBOLS)


def test_library_loads_without_gpu_and_checks_arguments_first(ragged_so):
    from zen_amd import ragged
    L = ragged.load()
    assert b"gfx950" in L.zen_hip_ragged_version()
    assert L.zen_hip_ragged_process_device(None, None, None, 0, None, None, 0) == 2
    assert b"null" in L.zen_hip_ragged_last_error()
    assert L.zen_hip_ragged_process_host(None, None, None, None, None) == 2
    h = ctypes.c_void_p()
    assert L.zen_hip_ragged_create(44100.0, 1024, 768, 2.0, 2.0, 0, 4, ctypes.byref(h)) == 3      # hops not divisible
    assert L.zen_hip_ragged_create(44100.0, 1024, 256, 2.0, 2.0, 0, 0, ctypes.byref(h)) == 2      # zero clips
    assert L.zen_hip_ragged_destroy(None) == 0


def test_library_finds_the_engine_library_beside_itself(ragged_so):
    out = subprocess.run(["readelf", "-d", ragged_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    assert "libzen_hip.so" in out and "$ORIGIN" in out


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "zen_hip_ragged.h"\nint main(void){zen_hip_ragged_t h = 0; return h != 0 || ZEN_HIP_OK;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.dirname(HDR), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_kernels_add_without_contraction_or_fast_math():
    from zen_amd.addon_build import ragged as addon
    assert "-ffp-contract=off" in addon.FLAGS and "-fno-fast-math" in addon.FLAGS
    assert not any("fast-math" in f and f != "-fno-fast-math" for f in addon.FLAGS)


# ---- plan_groups ------------------------------------------------------------------------------------------------------------
def partitions(items, group):
    """every way to put `items` into unordered groups of at most `group`"""
    if not items:
        yield []
        return
    first, rest = items[0], items[1:]
    for k in range(0, min(group - 1, len(rest)) + 1):
        for others in itertools.combinations(rest, k):
            left = [x for x in rest if x not in others]
            for p in partitions(left, group):
                yield [[first] + list(others)] + p


def test_plan_groups_against_brute_force():
    from zen_amd.ragged import plan_groups
    rng = np.random.default_rng(5)
    cases = [[5], [3, 3, 3], [10, 1, 1], [1, 2, 3], [7, 7, 1, 9, 2, 2, 8]]
    cases += [list(rng.integers(0, 50, int(n))) for n in rng.integers(1, 8, 12)]
    for lens in cases:
        for group in (1, 2, 3, 4, 9):
            groups, frac = plan_groups(lens, group)
            assert sorted(i for g in groups for i in g) == list(range(len(lens)))
            assert all(1 <= len(g) <= group for g in groups)
            assert len(groups) == -(-len(lens) // group)
            flat = [int(lens[i]) for g in groups for i in g]
            assert flat == sorted(flat, reverse=True)                       # sorted, consecutive
            cost = sum(max(int(lens[i]) for i in g) for g in groups)        # x group rows: what the calls cost
            best = min(sum(max(int(lens[i]) for i in g) for g in p) for p in partitions(list(range(len(lens))), group))
            assert cost == best, (lens, group)
            pad = sum(len(g) * max(int(lens[i]) for i in g) for g in groups)
            assert frac == (sum(int(x) for x in lens) / pad if pad else 1.0)
            assert 0.0 < frac <= 1.0
    assert plan_groups([], 4) == ([], 1.0)
    assert plan_groups([4, 4, 4, 4], 2)[1] == 1.0
    assert plan_groups([10, 20, 30, 40], 4) == ([[3, 2, 1, 0]], 100 / 160)
