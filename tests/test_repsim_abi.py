"""CPU-side checks of the repsim library's boundary (zen_amd/repsim/zen_hip_repsim.h): the header is plain C, every function it
declares is exported by libzen_hip_repsim.so and bound in zen_amd/repsim.py, the library loads without a GPU and refuses bad
arguments before it touches a device, its tables are the model's bit for bit, and it is built with the arithmetic contract's
flags."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HDR = os.path.join(ROOT, "zen_amd", "repsim", "zen_hip_repsim.h")
sys.path.insert(0, HERE)
import repet_model as RM  # noqa: E402

BAD = 2


@pytest.fixture(scope="module")
def repsim_so():
    from zen_amd.addon_build import repsim as addon
    if not os.path.exists(addon.OUT):
        addon.build()
    return addon.OUT


def declared_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zen_hip_repsim_[a-z0-9_]+)\s*\(", hdr)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_header_symbols_are_bound_and_exported(repsim_so):
    from zen_amd import lib, repsim
    L = ctypes.CDLL(repsim_so)
    names = declared_symbols()
    assert len(names) == 15
    for n in ("separate_device", "separate_host", "similarity_device", "select_device", "gather_median_device", "set_params", "stats", "table"):
        assert "zen_hip_repsim_" + n in names
    for n in names:
        assert hasattr(L, n), "libzen_hip_repsim.so does not export %s" % n
    assert set(names) == {s[0] for s in repsim.SYMBOLS}
    assert not any(s[0].startswith("zen_hip_repsim") for s in lib.SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", repsim_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    syms = [line.split()[-1] for line in out.splitlines() if line.strip()]
    assert {s for s in syms if s.startswith("zen_hip_")} == set(names)
    assert not [s for s in syms if "zen_addon" in s], "zen_amd/addon is header-only with internal linkage"


def test_library_loads_without_gpu_and_checks_arguments_first(repsim_so):
    from zen_amd import repsim
    L = repsim.load()
    err = L.zen_hip_repsim_last_error
    assert b"gfx950" in L.zen_hip_repsim_version()
    h = ctypes.c_void_p()
    for nfft in (48, 16384, 0, 32):
        assert L.zen_hip_repsim_create(44100.0, nfft, 1, 1000, ctypes.byref(h)) == BAD and b"power of two in 64..8192" in err()
    assert L.zen_hip_repsim_create(44100.0, 2048, 0, 1000, ctypes.byref(h)) == BAD and b"zero clips" in err()
    assert L.zen_hip_repsim_create(44100.0, 2048, 1, 1000, None) == BAD
    assert L.zen_hip_repsim_create(0.0, 2048, 1, 1000, ctypes.byref(h)) == BAD and b"sample rate" in err()
    assert L.zen_hip_repsim_create(44100.0, 2048, 1, 0, ctypes.byref(h)) == BAD
    # 16383 hops of 1024 are 16384 frames: one sample more is one frame too many
    assert L.zen_hip_repsim_create(44100.0, 2048, 1, 16383 * 1024 + 1, ctypes.byref(h)) == BAD and b"16384 frames" in err()
    assert L.zen_hip_repsim_create(8000.0, 64, 1, 1 << 40, ctypes.byref(h)) == BAD and b"16384 frames" in err()
    assert h.value is None
    assert L.zen_hip_repsim_separate_device(None, None, 0, 0, None, None, 0, None, None) == BAD and b"null handle" in err()
    assert L.zen_hip_repsim_separate_host(None, None, 0, 0, None, None, 0, None, None) == BAD and b"null handle" in err()
    assert L.zen_hip_repsim_stats(None, None) == BAD and L.zen_hip_repsim_profile(None, 1) == BAD
    assert L.zen_hip_repsim_set_stream(None, None) == BAD and L.zen_hip_repsim_set_params(None, 0.0, 1.0, 100, 100.0) == BAD
    assert L.zen_hip_repsim_profile_get(None, None, None, None) == BAD
    assert L.zen_hip_repsim_destroy(None) == 0
    # the parameters are judged before the handle is looked at
    for t, d, k, hp in ((-0.1, 1.0, 100, 100.0), (1.0, 1.0, 100, 100.0), (float("nan"), 1.0, 100, 100.0), (0.0, 1.0, 0, 100.0), (0.0, 1.0, 257, 100.0),
                        (0.0, -1.0, 100, 100.0), (0.0, float("inf"), 100, 100.0), (0.0, 1.0, 100, -1.0)):
        assert L.zen_hip_repsim_set_params(None, t, d, k, hp) == BAD and b"outside [0, 1)" in err()
    assert L.zen_hip_repsim_set_params(None, 0.5, 0.0, 256, 0.0) == BAD and b"null handle" in err()


def test_the_kernels_alone_refuse_before_a_device_is_touched(repsim_so):
    """null and misaligned pointers, strides below the row, frames and neighbours outside their ranges"""
    from zen_amd import repsim
    L = repsim.load()
    err = L.zen_hip_repsim_last_error
    sim, sel, med = L.zen_hip_repsim_similarity_device, L.zen_hip_repsim_select_device, L.zen_hip_repsim_gather_median_device
    assert sim(None, 10, 4, 4, 4096, 10, 0, None) == BAD and sim(16, 10, 4, 4, None, 10, 0, None) == BAD
    assert sim(18, 10, 4, 4, 4096, 10, 0, None) == BAD and sim(16, 10, 4, 4, 4098, 10, 0, None) == BAD and b"misaligned" in err()
    assert sim(16, 10, 4, 3, 4096, 10, 0, None) == BAD and sim(16, 10, 4, 4, 4096, 9, 0, None) == BAD and sim(16, 10, 0, 4, 4096, 10, 0, None) == BAD
    assert sim(16, 0, 4, 4, 4096, 10, 0, None) == BAD and sim(16, 16385, 4, 4, 4096, 16385, 0, None) == BAD and b"16384" in err()
    assert sim(16, 10, 4, 4, 4096, 10, 3, None) == BAD and sim(16, 10, 4, 4, 4096, 10, -1, None) == BAD and b"route" in err()
    assert sel(None, 10, 10, 0.0, 1, 5, 4096, 8192, None) == BAD and sel(16, 10, 10, 0.0, 1, 5, None, 8192, None) == BAD
    assert sel(16, 10, 10, 0.0, 1, 5, 4096, None, None) == BAD and sel(16, 10, 10, 0.0, 1, 5, 4097, 8192, None) == BAD
    assert sel(16, 10, 9, 0.0, 1, 5, 4096, 8192, None) == BAD and sel(16, 16385, 16385, 0.0, 1, 5, 4096, 8192, None) == BAD
    assert sel(16, 10, 10, 0.0, 0, 5, 4096, 8192, None) == BAD and sel(16, 10, 10, float("nan"), 1, 5, 4096, 8192, None) == BAD
    assert sel(16, 10, 10, 0.0, 1, 0, 4096, 8192, None) == BAD and sel(16, 10, 10, 0.0, 1, 257, 4096, 8192, None) == BAD and b"1..256" in err()
    assert med(None, 10, 4, 4, 4096, 8192, 10, 5, 12288, 4, None) == BAD and med(16, 10, 4, 4, None, 8192, 10, 5, 12288, 4, None) == BAD
    assert med(16, 10, 4, 4, 4096, None, 10, 5, 12288, 4, None) == BAD and med(16, 10, 4, 4, 4096, 8192, 10, 5, None, 4, None) == BAD
    assert med(16, 10, 4, 4, 4098, 8192, 10, 5, 12288, 4, None) == BAD and med(16, 10, 4, 3, 4096, 8192, 10, 5, 12288, 4, None) == BAD
    assert med(16, 10, 4, 4, 4096, 8192, 10, 5, 12288, 3, None) == BAD and med(16, 10, 0, 4, 4096, 8192, 10, 5, 12288, 4, None) == BAD
    assert med(16, 10, 4, 4, 4096, 8192, 0, 5, 12288, 4, None) == BAD and med(16, 10, 4, 4, 4096, 8192, 16385, 5, 12288, 4, None) == BAD
    assert med(16, 10, 4, 4, 4096, 8192, 10, 0, 12288, 4, None) == BAD and med(16, 10, 4, 4, 4096, 8192, 10, 257, 12288, 4, None) == BAD
    assert med(16, 0, 4, 4, 4096, 8192, 10, 5, 12288, 4, None) == BAD


def test_repsim_is_registered_behind_the_others():
    import zen_amd
    from zen_amd import addon_build
    assert addon_build.LIBRARIES["repsim"] is addon_build.repsim is zen_amd.repsim_build
    assert addon_build.repsim.FLAGS is addon_build.FLAGS and not addon_build.repsim.FILE_FLAGS
    assert addon_build.repsim.DEMO.endswith(os.path.join("bin", "zen-repsim"))
    assert zen_amd.repsim.Repsim and addon_build.repsim.OUT.endswith("libzen_hip_repsim.so")


@pytest.mark.parametrize("N", [64, 256, 8192])
def test_host_tables_are_the_models_bit_for_bit(repsim_so, N):
    from zen_amd import repsim
    w, d = repsim.table(N, repsim.TABLE_WINDOW), repsim.table(N, repsim.TABLE_DIVISOR)
    assert w.size == N and d.size == N // 2
    assert np.array_equal(bits(w), bits(RM.window(N))) and np.array_equal(bits(d), bits(RM.divisor(N)))


def test_table_refuses_bad_frames_and_short_buffers(repsim_so):
    from zen_amd import repsim
    L = repsim.load()
    out = np.full(300, 7.0, np.float32)
    p = out.ctypes.data
    for nfft in (48, 16384, 32):
        assert L.zen_hip_repsim_table(nfft, repsim.TABLE_WINDOW, p, out.size) == BAD
    assert L.zen_hip_repsim_table(256, 2, p, out.size) == BAD and L.zen_hip_repsim_table(256, repsim.TABLE_WINDOW, None, 256) == BAD
    assert L.zen_hip_repsim_table(256, repsim.TABLE_WINDOW, p, 255) == BAD and b"256" in L.zen_hip_repsim_last_error()
    assert L.zen_hip_repsim_table(256, repsim.TABLE_DIVISOR, p, 128) == 0 and np.all(out[128:] == 7.0)


def test_library_finds_the_engine_library_beside_itself(repsim_so):
    out = subprocess.run(["readelf", "-d", repsim_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    assert "libzen_hip.so" in out and "$ORIGIN" in out


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "zen_hip_repsim.h"\nint main(void){zen_hip_repsim_stats_t s; s.calls = 0; return ZEN_HIP_REPSIM_KERNELS - 10 + ZEN_HIP_OK '
                   '+ ZEN_HIP_REPSIM_TABLE_DIVISOR - 1 + ZEN_HIP_REPSIM_MAX_NEIGHBOURS - 256 + ZEN_HIP_REPSIM_ROUTE_VALU - 2 + (int)s.calls '
                   '+ (int)(ZEN_HIP_REPSIM_BAND_BYTES >> 26) - 1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.dirname(HDR), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_build_keeps_the_arithmetic_contract_and_the_other_libraries_apart():
    """no fast-math flag, contraction off, no flag that flushes denormals; the sources see the public headers, their own and
    zen_amd/addon's only -- nothing of csrc and nothing of zen_amd/repet, whose small kernels are copied; nothing was added to
    the shared headers"""
    from zen_amd.addon_build import repsim as addon
    assert "-ffp-contract=off" in addon.FLAGS and "-fno-fast-math" in addon.FLAGS and not addon.FILE_FLAGS
    assert not any(("fast-math" in f and f != "-fno-fast-math") or "denormal" in f or "ftz" in f for f in addon.FLAGS)
    assert sorted(os.listdir(addon.SRC)) == ["repsim.hip", "repsim_kernels.h", "repsim_kernels.hip", "repsim_main.cpp", "zen_hip_repsim.h"]
    for name in os.listdir(addon.SRC):
        text = open(os.path.join(addon.SRC, name)).read()
        assert "csrc/" not in re.sub(r"//.*", "", text) and "median_net.h" not in text, name
        for inc in re.findall(r'#include "([^"]+)"', text):
            assert inc in ("zen_hip.h", "zen_hip_repsim.h", "repsim_kernels.h", "wav.h", "demo.h", "../addon/addon_host.h", "../addon/stft_host.h", "../addon/stft_args.h",
                           "../addon/stft_kernels.h", "../addon/median_select.h"), (name, inc)
    assert sorted(os.listdir(os.path.join(ROOT, "zen_amd", "addon"))) == ["addon_host.h", "hpri_pair.h", "median_select.h", "row_walk.h", "stft_args.h", "stft_host.h", "stft_kernels.h"]
    assert sorted(os.listdir(os.path.join(ROOT, "zen_amd", "repet"))) == ["repet.hip", "repet_kernels.h", "repet_kernels.hip", "repet_main.cpp",
                                                                          "zen_hip_repet.h"]


def test_demo_program_is_built_and_states_its_usage(repsim_so):
    from zen_amd.addon_build import repsim as addon
    exe = addon.build_demo()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 2 and "usage: zen-repsim in.wav -o prefix" in r.stderr and "16384 frames" in r.stderr
    for opt in ("--nfft", "--distance", "--number", "--threshold", "--highpass"):
        assert opt in r.stderr
