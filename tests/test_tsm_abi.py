"""CPU-side checks of the time-stretch library's boundary (zen_amd/tsm/zen_hip_tsm.h): the header is plain C, every function
it declares is exported by libzen_hip_tsm.so and bound in zen_amd/tsm.py, the library loads without a GPU and refuses bad
arguments before it touches a device, its two host functions (the framing and the tables) are the model's bit for bit, it is
built with the arithmetic contract's flags, and it is registered beside the eleven add-ons from before it without moving them."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HDR = os.path.join(ROOT, "zen_amd", "tsm", "zen_hip_tsm.h")
sys.path.insert(0, HERE)
import tsm_model as M  # noqa: E402

BAD = 2


@pytest.fixture(scope="module")
def tsm_so():
    from zen_amd.addon_build import tsm as addon
    if not os.path.exists(addon.OUT):
        addon.build()
    return addon.OUT


def declared_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zen_hip_tsm_[a-z0-9_]+)\s*\(", hdr)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_header_symbols_are_bound_and_exported(tsm_so):
    from zen_amd import lib, tsm
    L = ctypes.CDLL(tsm_so)
    names = declared_symbols()
    assert len(names) == 17 and "zen_hip_tsm_stretch_hp_device" in names and "zen_hip_tsm_inspect_device" in names
    for n in names:
        assert hasattr(L, n), "libzen_hip_tsm.so does not export %s" % n
    assert set(names) == {s[0] for s in tsm.SYMBOLS}
    assert not any(s[0].startswith("zen_hip_tsm") for s in lib.SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", tsm_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    syms = [line.split()[-1] for line in out.splitlines() if line.strip()]
    assert {s for s in syms if s.startswith("zen_hip_")} == set(names)
    assert not [s for s in syms if "zen_addon" in s], "zen_amd/addon is header-only with internal linkage"


def test_library_loads_without_gpu_and_checks_arguments_first(tsm_so):
    from zen_amd import tsm
    L = tsm.load()
    err = L.zen_hip_tsm_last_error
    assert b"gfx950" in L.zen_hip_tsm_version()
    h = ctypes.c_void_p()

    def create(fs=44100.0, nfft=4096, nfft_ola=256, clips=1, n=1000, alpha=4.0, out=ctypes.byref(h)):
        return L.zen_hip_tsm_create(fs, nfft, nfft_ola, clips, n, alpha, out)
    for nfft in (48, 16384, 0, 32):
        assert create(nfft=nfft) == BAD and b"power of two in 64..8192" in err()
    for nfft_ola in (8, 8192, 0, 48):
        assert create(nfft_ola=nfft_ola) == BAD and b"power of two in 16..4096" in err()
    assert create(clips=0) == BAD and b"zero clips" in err()
    assert create(out=None) == BAD
    assert create(fs=0.0) == BAD and b"sample rate" in err()
    for alpha in (0.2, 4.5, float("nan"), float("inf")):
        assert create(alpha=alpha) == BAD and b"outside 0.25..4" in err()
    assert create(n=0) == BAD
    assert create(n=3, alpha=0.25) == BAD and b"1 sample at the least" in err()
    # frames of 64 at overlap 4: (n_out - 1) / 16 + 4 <= 16384 holds up to 16381 * 16 output samples
    assert create(nfft=64, nfft_ola=4096, n=16381 * 16 + 1, alpha=1.0) == BAD and b"16384 frames" in err()
    # overlap-add frames of 16 at overlap 2: (n_out - 1) / 8 + 2 <= 16384 holds up to 16383 * 8 output samples
    assert create(nfft=8192, nfft_ola=16, n=16383 * 8 + 1, alpha=1.0) == BAD and b"16384 frames" in err()
    assert create(n=1 << 40) == BAD and b"16384 frames" in err()
    assert h.value is None
    # a long clip made shorter fits: 40 million samples at a quarter are 4887 frames of 2048; past the checks the call needs a device
    rc = create(nfft=8192, nfft_ola=4096, n=40000000, alpha=0.25)
    assert rc != BAD
    if rc == 0:
        assert L.zen_hip_tsm_destroy(h) == 0
        h.value = None
    assert L.zen_hip_tsm_stretch_pv_device(None, None, 0, 0, 1.0, None, 0) == BAD and b"null handle" in err()
    assert L.zen_hip_tsm_stretch_ola_device(None, None, None, 0, 0, 1.0, None, 0) == BAD and b"null handle" in err()
    assert L.zen_hip_tsm_stretch_hp_device(None, None, None, None, 0, 0, 1.0, None, 0) == BAD and b"null handle" in err()
    assert L.zen_hip_tsm_stretch_hp_host(None, None, None, None, 0, 0, 1.0, None, 0) == BAD and b"null handle" in err()
    assert L.zen_hip_tsm_inspect_device(None, None, 0, 0, 1.0, None, None, None, None) == BAD and b"null handle" in err()
    assert L.zen_hip_tsm_stats(None, None) == BAD and L.zen_hip_tsm_profile(None, 1) == BAD
    assert L.zen_hip_tsm_set_stream(None, None) == BAD and L.zen_hip_tsm_profile_get(None, None, None, None) == BAD
    assert L.zen_hip_tsm_destroy(None) == 0
    # the two kernels alone: refused before a device is touched; nothing to do is no device call either
    assert L.zen_hip_tsm_phase_device(None, 4, 16, None) == BAD and L.zen_hip_tsm_phase_device(16, 4, None, None) == BAD
    assert L.zen_hip_tsm_phase_device(18, 4, 16, None) == BAD and L.zen_hip_tsm_phase_device(16, 4, 34, None) == BAD
    assert L.zen_hip_tsm_cs_device(None, 4, 16, None) == BAD and L.zen_hip_tsm_cs_device(16, 4, None, None) == BAD
    assert L.zen_hip_tsm_cs_device(17, 4, 16, None) == BAD and L.zen_hip_tsm_cs_device(16, 4, 18, None) == BAD
    assert L.zen_hip_tsm_phase_device(16, 0, 16, None) == 0 and L.zen_hip_tsm_cs_device(16, 0, 16, None) == 0


def test_tsm_is_registered_in_a_table_of_its_own():
    import zen_amd
    from zen_amd import addon_build
    assert addon_build.LIBRARIES["tsm"] is addon_build.tsm is zen_amd.tsm_build
    assert addon_build.tsm.FLAGS is addon_build.FLAGS and not addon_build.tsm.FILE_FLAGS
    assert addon_build.tsm.SOURCES == ["tsm_kernels.hip", "tsm.hip"] and addon_build.tsm.OUT.endswith("libzen_hip_tsm.so")
    assert zen_amd.tsm.Tsm and addon_build.tsm.DEMO.endswith(os.path.join("bin", "zen-stretch"))


@pytest.mark.parametrize("N", [64, 256, 8192])
def test_host_tables_are_the_models_bit_for_bit(tsm_so, N):
    from zen_amd import tsm
    w, D = tsm.table(N, tsm.TABLE_WINDOW), tsm.table(N, tsm.TABLE_PV_DIVISOR)
    assert w.size == N and D.size == N // 4
    assert np.array_equal(bits(w), bits(M.window(N))) and np.array_equal(bits(D), bits(M.pv_divisor(N)))
    Np = N // 4                 # 16, 64, 2048
    wp, d2 = tsm.table(Np, tsm.TABLE_WINDOW), tsm.table(Np, tsm.TABLE_OLA_DIVISOR)
    assert np.array_equal(bits(wp), bits(M.window(Np))) and np.array_equal(bits(d2), bits(M.ola_divisor(Np)))


def test_trigonometric_tables_are_the_models_bit_for_bit(tsm_so):
    from zen_amd import tsm
    A, B, T, c = (tsm.table(0, k) for k in (tsm.TABLE_COARSE, tsm.TABLE_FINE, tsm.TABLE_ATAN, tsm.TABLE_CONSTANTS))
    assert A.shape == (2048, 2) and B.shape == (2048, 2) and T.shape == (257,) and T.dtype == np.uint32
    assert np.array_equal(bits(A), bits(M.coarse())) and np.array_equal(bits(B), bits(M.fine()))
    assert np.array_equal(T.astype(np.int64), M.atan_table()) and T[0] == 0 and T[256] == 1 << 29
    assert np.array_equal(bits(c), bits(np.array([M.C3, M.K], np.float32)))


def test_table_refuses_bad_frames_and_short_buffers(tsm_so):
    from zen_amd import tsm
    L = tsm.load()
    out = np.full(300, 7.0, np.float32)
    p = out.ctypes.data
    for nfft in (48, 16384, 8):
        assert L.zen_hip_tsm_table(nfft, tsm.TABLE_WINDOW, p, out.size) == BAD
    assert L.zen_hip_tsm_table(32, tsm.TABLE_PV_DIVISOR, p, out.size) == BAD and L.zen_hip_tsm_table(8192, tsm.TABLE_OLA_DIVISOR, p, 1 << 20) == BAD
    assert L.zen_hip_tsm_table(256, 7, p, out.size) == BAD and L.zen_hip_tsm_table(256, tsm.TABLE_WINDOW, None, 256) == BAD
    assert L.zen_hip_tsm_table(256, tsm.TABLE_WINDOW, p, 255) == BAD and b"256" in L.zen_hip_tsm_last_error()
    assert L.zen_hip_tsm_table(0, tsm.TABLE_ATAN, p, 256) == BAD and L.zen_hip_tsm_table(0, tsm.TABLE_COARSE, p, 4095) == BAD
    assert L.zen_hip_tsm_table(256, tsm.TABLE_OLA_DIVISOR, p, 128) == 0 and np.all(out[128:] == 7.0)


def test_positions_are_the_models(tsm_so):
    from zen_amd import tsm
    rng = np.random.default_rng(5)
    cases = [(1, 64, 4, 1.0), (4, 64, 4, 0.25), (6000, 256, 4, 0.77), (6000, 16, 2, 4.0), (31, 64, 4, 1.3), (5000, 2048, 4, 1.0),
             (15, 64, 4, 4.0), (16, 64, 4, 1.0), (17, 64, 4, 1.0), (200000, 8192, 4, 1.5), (100000, 4096, 2, 1.0 / 3.0)]
    cases += [(int(rng.integers(1, 20000)), 1 << int(rng.integers(4, 14)), int(rng.choice([2, 4])), float(rng.uniform(0.25, 4.0))) for _ in range(60)]
    for n, N, V, alpha in cases:
        if int(np.floor(n * alpha)) == 0:
            continue
        n_out, m, a = tsm.positions(n, N, V, alpha)
        want = M.positions(n, N, V, alpha)
        assert (n_out, m) == want[:2] and list(a) == want[2], (n, N, V, alpha)
        assert np.all(np.diff(a) >= 1) and (alpha != 1.0 or np.all(np.diff(a) == N // V))
    L = tsm.load()
    no, m = ctypes.c_size_t(), ctypes.c_size_t()
    a = (ctypes.c_longlong * 8)()

    def pos(n=100, frame=64, overlap=4, alpha=1.0, cap=8):
        return L.zen_hip_tsm_positions(n, frame, overlap, alpha, ctypes.byref(no), ctypes.byref(m), a, cap)
    assert pos(n=0) == BAD and pos(n=3, alpha=0.25) == BAD and b"no output sample" in L.zen_hip_tsm_last_error()
    assert pos(frame=48) == BAD and pos(frame=8) == BAD and pos(overlap=3) == BAD
    assert pos(alpha=0.2) == BAD and pos(alpha=float("nan")) == BAD and pos(alpha=4.01) == BAD
    assert pos(n=100, cap=8) == BAD and b"10 frames" in L.zen_hip_tsm_last_error()      # 99 / 16 + 4 = 10 frames
    assert L.zen_hip_tsm_positions(100, 64, 4, 1.0, None, ctypes.byref(m), None, 0) == BAD
    assert pos(n=64, cap=8) == 0 and (no.value, m.value) == (64, 7) and list(a)[:7] == [16 * (i - 1) for i in range(7)]


def test_longest_clip_fits_both_routes_and_one_frame_more_does_not(tsm_so):
    from zen_amd import tsm
    for nfft, nfft_ola, alpha in ((4096, 256, 4.0), (64, 4096, 1.0), (8192, 16, 0.25), (2048, 512, 1.3), (8192, 4096, 0.25)):
        n = tsm.longest_clip(nfft, nfft_ola, alpha)
        assert max(tsm.positions(n, nfft, 4, alpha)[1], tsm.positions(n, nfft_ola, 2, alpha)[1]) <= tsm.MAX_FRAMES
        more = n + int(max(nfft // 4, nfft_ola // 2) * 5 / alpha) + 1
        assert max(tsm.positions(more, nfft, 4, alpha)[1], tsm.positions(more, nfft_ola, 2, alpha)[1]) > tsm.MAX_FRAMES
    assert tsm.longest_clip(4096, 256, 4.0) == 524224


def test_library_finds_the_engine_library_beside_itself(tsm_so):
    out = subprocess.run(["readelf", "-d", tsm_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    assert "libzen_hip.so" in out and "$ORIGIN" in out


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "zen_hip_tsm.h"\nint main(void){zen_hip_tsm_stats_t s; s.calls = 0; return ZEN_HIP_TSM_KERNELS - 8 + ZEN_HIP_OK '
                   '+ ZEN_HIP_TSM_TABLE_CONSTANTS - 6 + ZEN_HIP_TSM_MAX_FRAMES - 16384 + (int)s.calls;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.dirname(HDR), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_build_keeps_the_arithmetic_contract_and_the_engines_apart():
    """no fast-math flag, contraction off, no flag that flushes denormals, no flags of a file's own; the sources see the public
    headers, their own and zen_amd/addon's only -- nothing of csrc; no inline assembly and no atomics; nothing was added to the
    shared headers"""
    from zen_amd.addon_build import tsm as addon
    assert "-ffp-contract=off" in addon.FLAGS and "-fno-fast-math" in addon.FLAGS and not addon.FILE_FLAGS
    assert not any(("fast-math" in f and f != "-fno-fast-math") or "denormal" in f or "ftz" in f for f in addon.FLAGS)
    assert sorted(os.listdir(addon.SRC)) == ["tsm.hip", "tsm_kernels.h", "tsm_kernels.hip", "tsm_main.cpp", "zen_hip_tsm.h"]
    for name in os.listdir(addon.SRC):
        text = open(os.path.join(addon.SRC, name)).read()
        code = re.sub(r"//.*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
        assert "csrc/" not in code and "asm" not in code and "atomic" not in code, name
        for inc in re.findall(r'#include "([^"]+)"', text):
            assert inc in ("zen_hip.h", "zen_hip_tsm.h", "tsm_kernels.h", "wav.h", "demo.h", "../addon/addon_host.h"), (name, inc)
    assert sorted(os.listdir(os.path.join(ROOT, "zen_amd", "addon"))) == ["addon_host.h", "hpri_pair.h", "median_select.h", "row_walk.h", "stft_args.h", "stft_host.h", "stft_kernels.h"]


def test_demo_program_is_built_and_states_its_usage(tsm_so):
    from zen_amd.addon_build import tsm as addon
    exe = addon.build_demo()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 2 and "usage: zen-stretch in.wav -a ratio -o out.wav" in r.stderr and "--plain" in r.stderr
    r = subprocess.run([exe, "in.wav", "-a", "5", "-o", "out.wav"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 2


def test_demo_program_names_the_way_out_for_a_long_recording(tsm_so, tmp_path):
    """110000 samples, padded to 110592, at 1.3 are 143769 output samples: more than 16383 * 8, the most an overlap-add frame of 16
    takes; the program says so, and how to go on, before it touches a device"""
    import struct
    from zen_amd.addon_build import tsm as addon
    x = np.zeros(110000, "<f4")
    wav = str(tmp_path / "long.wav")
    with open(wav, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + x.nbytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 3, 1, 8000, 32000, 4, 32) + b"data"
                + struct.pack("<I", x.nbytes) + x.tobytes())
    r = subprocess.run([addon.build_demo(), wav, "-a", "1.3", "-o", str(tmp_path / "out.wav"), "--nfft-ola", "16"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 1 and "16384 overlap-add frames of 8" in r.stderr and "--nfft-ola" in r.stderr
    assert not os.path.exists(str(tmp_path / "out.wav"))
