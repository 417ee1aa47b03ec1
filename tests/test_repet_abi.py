"""CPU-side checks of the repet library's boundary (zen_amd/repet/zen_hip_repet.h): the header is plain C, every function it
declares is exported by libzen_hip_repet.so and bound in zen_amd/repet.py, the library loads without a GPU and refuses bad
arguments before it touches a device, its two host functions (the period search and the tables) are the model's bit for bit,
and it is built with the arithmetic contract's flags."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HDR = os.path.join(ROOT, "zen_amd", "repet", "zen_hip_repet.h")
sys.path.insert(0, HERE)
import repet_model as M  # noqa: E402

BAD, UNSUPPORTED = 2, 5


@pytest.fixture(scope="module")
def repet_so():
    from zen_amd.addon_build import repet as addon
    if not os.path.exists(addon.OUT):
        addon.build()
    return addon.OUT


def declared_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zen_hip_repet_[a-z0-9_]+)\s*\(", hdr)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_header_symbols_are_bound_and_exported(repet_so):
    from zen_amd import lib, repet
    L = ctypes.CDLL(repet_so)
    names = declared_symbols()
    assert len(names) == 15 and "zen_hip_repet_separate_device" in names and "zen_hip_repet_segment_median_device" in names
    for n in names:
        assert hasattr(L, n), "libzen_hip_repet.so does not export %s" % n
    assert set(names) == {s[0] for s in repet.SYMBOLS}
    assert not any(s[0].startswith("zen_hip_repet") for s in lib.SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", repet_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    syms = [line.split()[-1] for line in out.splitlines() if line.strip()]
    assert {s for s in syms if s.startswith("zen_hip_")} == set(names)
    assert not [s for s in syms if "zen_addon" in s], "zen_amd/addon is header-only with internal linkage"


def test_library_loads_without_gpu_and_checks_arguments_first(repet_so):
    from zen_amd import repet
    L = repet.load()
    err = L.zen_hip_repet_last_error
    assert b"gfx950" in L.zen_hip_repet_version()
    h = ctypes.c_void_p()
    for nfft in (48, 16384, 0, 32):
        assert L.zen_hip_repet_create(44100.0, nfft, 1, 1000, ctypes.byref(h)) == BAD and b"power of two in 64..8192" in err()
    assert L.zen_hip_repet_create(44100.0, 2048, 0, 1000, ctypes.byref(h)) == BAD and b"zero clips" in err()
    assert L.zen_hip_repet_create(44100.0, 2048, 1, 1000, None) == BAD
    assert L.zen_hip_repet_create(0.0, 2048, 1, 1000, ctypes.byref(h)) == BAD and b"sample rate" in err()
    assert L.zen_hip_repet_create(44100.0, 2048, 1, 0, ctypes.byref(h)) == BAD
    # 16383 hops of 1024 are 16384 frames: one sample more is one frame too many
    assert L.zen_hip_repet_create(44100.0, 2048, 1, 16383 * 1024 + 1, ctypes.byref(h)) == BAD and b"16384 frames" in err()
    assert L.zen_hip_repet_create(8000.0, 64, 1, 1 << 40, ctypes.byref(h)) == BAD and b"16384 frames" in err()
    assert h.value is None
    assert L.zen_hip_repet_separate_device(None, None, 0, 0, None, None, None, 0, None, None, 0) == BAD and b"null handle" in err()
    assert L.zen_hip_repet_separate_host(None, None, 0, 0, None, None, None, 0, None, None, 0) == BAD and b"null handle" in err()
    assert L.zen_hip_repet_beat_spectrum_device(None, None, 0, 0, None, 0) == BAD and b"null handle" in err()
    assert L.zen_hip_repet_stats(None, None) == BAD and L.zen_hip_repet_profile(None, 1) == BAD
    assert L.zen_hip_repet_set_stream(None, None) == BAD and L.zen_hip_repet_set_params(None, 0.8, 8.0, 100.0) == BAD
    assert L.zen_hip_repet_profile_get(None, None, None, None) == BAD
    assert L.zen_hip_repet_destroy(None) == 0
    # the kernel alone: refused before a device is touched
    assert L.zen_hip_repet_segment_median_device(None, 10, 4, 4, 2, None, 4, None) == BAD
    assert L.zen_hip_repet_segment_median_device(16, 10, 4, 3, 2, 32, 4, None) == BAD
    assert L.zen_hip_repet_segment_median_device(16, 10, 0, 4, 2, 32, 4, None) == BAD
    assert L.zen_hip_repet_segment_median_device(18, 10, 4, 4, 2, 32, 4, None) == BAD
    assert L.zen_hip_repet_segment_median_device(16, 10, 4, 4, 10, 32, 4, None) == UNSUPPORTED and b"1 segments" in err()
    assert L.zen_hip_repet_segment_median_device(16, 257, 4, 4, 1, 32, 4, None) == UNSUPPORTED and b"257 segments" in err()
    assert L.zen_hip_repet_segment_median_device(16, 10, 4, 4, 0, 32, 4, None) == UNSUPPORTED


def test_repet_is_registered_beside_the_others():
    import zen_amd
    from zen_amd import addon_build
    assert addon_build.LIBRARIES["repet"] is addon_build.repet is zen_amd.repet_build
    assert addon_build.repet.FLAGS is addon_build.FLAGS and addon_build.repet.DEMO.endswith(os.path.join("bin", "zen-repet"))
    assert zen_amd.repet.Repet and addon_build.repet.OUT.endswith("libzen_hip_repet.so")


@pytest.mark.parametrize("N", [64, 256, 8192])
def test_host_tables_are_the_models_bit_for_bit(repet_so, N):
    from zen_amd import repet
    w, d = repet.table(N, repet.TABLE_WINDOW), repet.table(N, repet.TABLE_DIVISOR)
    assert w.size == N and d.size == N // 2
    assert np.array_equal(bits(w), bits(M.window(N))) and np.array_equal(bits(d), bits(M.divisor(N)))


def test_table_refuses_bad_frames_and_short_buffers(repet_so):
    from zen_amd import repet
    L = repet.load()
    out = np.full(300, 7.0, np.float32)
    p = out.ctypes.data
    for nfft in (48, 16384, 32):
        assert L.zen_hip_repet_table(nfft, repet.TABLE_WINDOW, p, out.size) == BAD
    assert L.zen_hip_repet_table(256, 2, p, out.size) == BAD and L.zen_hip_repet_table(256, repet.TABLE_WINDOW, None, 256) == BAD
    assert L.zen_hip_repet_table(256, repet.TABLE_WINDOW, p, 255) == BAD and b"256" in L.zen_hip_repet_last_error()
    assert L.zen_hip_repet_table(256, repet.TABLE_DIVISOR, p, 128) == 0 and np.all(out[128:] == 7.0)


def same_search(repet, braw, jmin, jmax):
    want = M.find_period(braw, jmin, jmax)
    got = repet.find_period(braw, jmin, jmax)
    assert got[0] == want[0] and np.float64(got[1]).view(np.uint64) == np.float64(want[1]).view(np.uint64), (got, want)
    return got


def test_find_period_is_the_models_on_the_family(repet_so, oracle):
    """the beat spectra of the 20 clips: the model's period, which is the true one, and its score as the same double"""
    from zen_amd import repet
    oracle.lib()
    for seed, N, P, R in M.FAMILY:
        x, _, _ = M.family_clip(seed, N, P, R)
        braw = M.beat_spectrum_raw(M.magnitude(M.spectra(x, N)))
        jmin, jmax = M.lag_bounds(M.FAMILY_FS, N // 2, *M.family_bounds(N))
        assert jmin == 4
        assert same_search(repet, braw, jmin, jmax)[0] == P


def test_find_period_is_the_models_on_random_beat_spectra(repet_so):
    from zen_amd import repet
    rng = np.random.default_rng(17)
    found = 0
    for k in range(200):
        m = int(rng.integers(8, 401))
        braw = rng.uniform(0, 1, m).astype(np.float32)
        if k % 4 == 0:                              # peaks every q lags on a falling floor, as a beat spectrum has
            q = int(rng.integers(3, 40))
            braw = (0.3 * rng.uniform(0, 1, m) * np.linspace(1, 0.5, m)).astype(np.float32)
            braw[::q] += np.float32(0.6)
        braw[0] = np.float32(rng.uniform(1, 2))
        if k % 25 == 1:
            braw[:] = 0
        elif k % 25 == 2:
            braw[:] = braw[0]
        elif k % 25 == 3:
            braw[0] = np.nan
        elif k % 25 == 4:
            braw[0] = np.inf
        elif k % 25 == 5:
            braw[int(rng.integers(1, m))] = np.nan  # a NaN inside: never the largest, and it poisons the means it is in
        jmin = int(rng.integers(2, 6))
        jmax = int(rng.integers(jmin, 500))
        p, _ = same_search(repet, braw, jmin, jmax)
        assert p == 0 or (jmin <= p <= min(jmax, (3 * m // 4) // 3))
        if k % 25 in (1, 2, 3, 4):
            assert p == 0
        found += p > 0
    assert found >= 50
    assert repet.find_period(np.zeros(0, np.float32), 2, 10) == (0, 0.0)
    L = repet.load()
    assert L.zen_hip_repet_find_period(None, 5, 2, 10, None, None) == BAD


def test_library_finds_the_engine_library_beside_itself(repet_so):
    out = subprocess.run(["readelf", "-d", repet_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    assert "libzen_hip.so" in out and "$ORIGIN" in out


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "zen_hip_repet.h"\nint main(void){zen_hip_repet_stats_t s; s.calls = 0; return ZEN_HIP_REPET_KERNELS - 11 + ZEN_HIP_OK '
                   '+ ZEN_HIP_REPET_TABLE_DIVISOR - 1 + ZEN_HIP_REPET_MAX_SEGMENTS - 256 + (int)s.calls;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.dirname(HDR), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_build_keeps_the_arithmetic_contract_and_the_engines_apart():
    """no fast-math flag, contraction off, no flag that flushes denormals; the sources see the public headers, their own and
    zen_amd/addon's only -- nothing of csrc, the engines' median networks included; nothing was added to the shared headers"""
    from zen_amd.addon_build import repet as addon
    assert "-ffp-contract=off" in addon.FLAGS and "-fno-fast-math" in addon.FLAGS and not addon.FILE_FLAGS
    assert not any(("fast-math" in f and f != "-fno-fast-math") or "denormal" in f or "ftz" in f for f in addon.FLAGS)
    assert sorted(os.listdir(addon.SRC)) == ["repet.hip", "repet_kernels.h", "repet_kernels.hip", "repet_main.cpp", "zen_hip_repet.h"]
    for name in os.listdir(addon.SRC):
        text = open(os.path.join(addon.SRC, name)).read()
        assert "csrc/" not in re.sub(r"//.*", "", text) and "median_net.h" not in text, name
        for inc in re.findall(r'#include "([^"]+)"', text):
            assert inc in ("zen_hip.h", "zen_hip_repet.h", "repet_kernels.h", "wav.h", "demo.h", "../addon/addon_host.h", "../addon/stft_host.h", "../addon/stft_args.h",
                           "../addon/stft_kernels.h", "../addon/median_select.h"), (name, inc)
    assert sorted(os.listdir(os.path.join(ROOT, "zen_amd", "addon"))) == ["addon_host.h", "hpri_pair.h", "median_select.h", "row_walk.h", "stft_args.h", "stft_host.h", "stft_kernels.h"]


def test_demo_program_is_built_and_states_its_usage(repet_so):
    from zen_amd.addon_build import repet as addon
    exe = addon.build_demo()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 2 and "usage: zen-repet in.wav -o prefix" in r.stderr and "256 repetitions" in r.stderr
