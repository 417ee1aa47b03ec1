"""CPU-side checks of the resample library's boundary (zen_amd/resample/zen_hip_resample.h): the header is plain C, every
function it declares is exported by libzen_hip_resample.so and bound in zen_amd/resample.py, the library loads without a GPU
and refuses bad arguments before it touches a device, its host functions (the table, the geometry, the output count, the span
and the ratio of a shift) are the model's bit for bit, it is built with the arithmetic contract's flags, and it is registered
in a table of its own beside the twelve add-ons from before it without moving them."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HDR = os.path.join(ROOT, "zen_amd", "resample", "zen_hip_resample.h")
sys.path.insert(0, HERE)
import resample_model as M  # noqa: E402

BAD = 2
RATIOS = [(147, 160), (160, 147), (1, 4), (4, 1), (1048573, 1048575), (61858, 65536), (1, 1)]


@pytest.fixture(scope="module")
def resample_so():
    from zen_amd.addon_build import resample as addon
    if not os.path.exists(addon.OUT):
        addon.build()
    return addon.OUT


def declared_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zen_hip_resample_[a-z0-9_]+)\s*\(", hdr)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_header_symbols_are_bound_and_exported(resample_so):
    from zen_amd import lib, resample
    L = ctypes.CDLL(resample_so)
    names = declared_symbols()
    assert len(names) == 15 and "zen_hip_resample_run_device" in names and "zen_hip_resample_ratio_for_shift" in names
    for n in names:
        assert hasattr(L, n), "libzen_hip_resample.so does not export %s" % n
    assert set(names) == {s[0] for s in resample.SYMBOLS}
    assert not any(s[0].startswith("zen_hip_resample") for s in lib.SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", resample_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    syms = [line.split()[-1] for line in out.splitlines() if line.strip()]
    assert {s for s in syms if s.startswith("zen_hip_")} == set(names)
    assert not [s for s in syms if "zen_addon" in s], "zen_amd/addon is header-only with internal linkage"


def test_library_loads_without_gpu_and_checks_arguments_first(resample_so):
    from zen_amd import resample
    L = resample.load()
    err = L.zen_hip_resample_last_error
    assert b"gfx950" in L.zen_hip_resample_version()
    h = ctypes.c_void_p()

    def create(num=147, den=160, quality=16, out=ctypes.byref(h)):
        return L.zen_hip_resample_create(num, den, quality, out)
    assert create(out=None) == BAD and b"null handle" in err()
    assert create(num=0) == BAD and create(den=0) == BAD
    for num, den in ((1, 5), (5, 1), (100, 401), (1 << 21, 1 << 18)):
        assert create(num=num, den=den) == BAD and b"outside 1/4..4" in err(), (num, den)
    for num, den in ((1048577, 1048576), (1048576, 1048577), ((1 << 21) + 1, 1 << 21)):
        assert create(num=num, den=den) == BAD and b"above 2^20" in err(), (num, den)
    for q in (0, 7, 12, 64, -8):
        assert create(quality=q) == BAD and b"none of 8, 16, 32" in err()
    assert h.value is None
    # a ratio that reduces into the range is taken: past the checks the call needs a device
    rc = create(num=3 << 20, den=2 << 20)
    assert rc != BAD
    if rc == 0:
        assert L.zen_hip_resample_destroy(h) == 0
        h.value = None
    assert L.zen_hip_resample_run_device(None, 16, 10, 0, 10, 10, 0, 5, 4096, 5, 1) == BAD and b"null handle" in err()
    assert L.zen_hip_resample_run_host(None, 16, 10, 10, 4096, 10, 1) == BAD and b"null handle" in err()
    assert L.zen_hip_resample_stats(None, None) == BAD and L.zen_hip_resample_profile(None, 1) == BAD
    assert L.zen_hip_resample_set_stream(None, None) == BAD and L.zen_hip_resample_profile_get(None, None, None, None) == BAD
    assert L.zen_hip_resample_destroy(None) == 0


def test_host_functions_refuse_bad_arguments(resample_so):
    from zen_amd import resample
    L = resample.load()
    a, b = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    w, t, r = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int()
    pa, pb = ctypes.byref(a), ctypes.byref(b)
    assert L.zen_hip_resample_n_out(147, 160, 0, pa) == BAD and L.zen_hip_resample_n_out(147, 160, (1 << 40) + 1, pa) == BAD
    assert L.zen_hip_resample_n_out(147, 160, 10, None) == BAD and L.zen_hip_resample_n_out(1, 5, 10, pa) == BAD
    assert L.zen_hip_resample_n_out(4, 1, 1 << 40, pa) == 0 and a.value == 1 << 42
    assert L.zen_hip_resample_span(147, 160, 16, 5000, 0, 0, pa, pb) == BAD
    assert L.zen_hip_resample_span(147, 160, 16, 5000, 4594, 1, pa, pb) == BAD and b"a row that has 4594" in L.zen_hip_resample_last_error()
    assert L.zen_hip_resample_span(147, 160, 16, 5000, 4000, 595, pa, pb) == BAD
    assert L.zen_hip_resample_span(147, 160, 9, 5000, 0, 1, pa, pb) == BAD and L.zen_hip_resample_span(147, 160, 16, 5000, 0, 1, None, pb) == BAD
    assert L.zen_hip_resample_span(147, 160, 16, 0, 0, 1, pa, pb) == BAD
    assert L.zen_hip_resample_geometry(147, 160, 16, None, ctypes.byref(t), ctypes.byref(r)) == BAD
    assert L.zen_hip_resample_geometry(147, 160, 15, ctypes.byref(w), ctypes.byref(t), ctypes.byref(r)) == BAD
    assert L.zen_hip_resample_geometry(9, 2, 16, ctypes.byref(w), ctypes.byref(t), ctypes.byref(r)) == BAD
    out = np.full(513 * 36 + 4, 7.0, np.float32)
    assert L.zen_hip_resample_table(147, 160, 16, None, out.size) == BAD and L.zen_hip_resample_table(147, 160, 16, out.ctypes.data, 513 * 36 - 1) == BAD
    assert b"18468" in L.zen_hip_resample_last_error()
    assert L.zen_hip_resample_table(147, 160, 16, out.ctypes.data, 513 * 36) == 0 and np.all(out[513 * 36:] == 7.0) and not np.any(out[:513 * 36] == 7.0)
    for s in (24.5, -24.001, float("nan"), float("inf")):
        assert L.zen_hip_resample_ratio_for_shift(s, pa, pb) == BAD and b"outside -24..24" in L.zen_hip_resample_last_error()
    assert L.zen_hip_resample_ratio_for_shift(3.0, None, pb) == BAD


@pytest.mark.parametrize("Z", [8, 16, 32])
def test_table_and_geometry_are_the_models_bit_for_bit(resample_so, Z):
    from zen_amd import resample
    for num, den in RATIOS + [(2 * 147, 2 * 160), (53, 63), (4097, 4096)]:
        W, T, route = resample.geometry(num, den, Z)
        assert (W, T, route) == M.geometry(num, den, Z), (num, den)
        h = resample.table(num, den, Z)
        assert h.shape == (513, T) and np.array_equal(bits(h), bits(M.table(num, den, Z))), (num, den, Z)


def test_n_out_and_span_are_the_models(resample_so):
    from zen_amd import resample
    rng = np.random.default_rng(8)
    for num, den in RATIOS:
        for n in [1, 2, 3, 699, 700, 1 << 40] + [int(v) for v in rng.integers(1, 1 << 40, 20)]:
            total = resample.n_out(num, den, n)
            assert total == M.n_out(num, den, n), (num, den, n)
            for Z in (8, 16, 32):
                firsts = {0, total - 1, total // 2} | {int(v) for v in rng.integers(0, total, 4)}
                for first in firsts:
                    for count in {1, min(7, total - first), min(100000, total - first), total - first}:
                        assert resample.span(num, den, Z, n, first, count) == M.span(num, den, Z, n, first, count), (num, den, Z, n, first, count)
    assert resample.TILE == 256 and resample.PHASES == M.PHASES and resample.MAX_POLY == M.MAX_POLY


def test_ratio_for_shift_is_the_models(resample_so):
    from zen_amd import resample
    for s in list(range(-24, 25)) + [0.5, -0.37, 11.99, 23.999, -24.0, 1e-9]:
        assert resample.ratio_for_shift(s) == M.ratio_for_shift(s), s
    assert resample.ratio_for_shift(12) == (1, 2) and resample.ratio_for_shift(-24) == (4, 1) and resample.ratio_for_shift(0) == (1, 1)
    for n in (3000, 3072, 44100, 10 ** 7):
        for s in (-24, -5, 3, 7, 24):
            assert resample.shift_plan(n, s) == M.shift_lengths(n, s)
    assert resample.ratio_of_rates(48000, 44100) == (147, 160) and resample.ratio_of_rates(44100.0, 96000.0) == (320, 147)
    with pytest.raises(ValueError):
        resample.ratio_of_rates(44100.5, 48000)


def test_resample_is_registered_in_a_table_of_its_own():
    import zen_amd
    from zen_amd import _addon, addon_build, resample
    assert resample.load and list(addon_build.LIBRARIES)[-2:] == ["tsm", "resample"]
    assert addon_build.LIBRARIES["resample"] is addon_build.resample is zen_amd.resample_build
    assert addon_build.resample.FLAGS is addon_build.FLAGS and tuple(addon_build.resample.demo_links) == ("tsm",)
    assert addon_build.resample.SOURCES == ["resample_kernels.hip", "resample.hip"] and addon_build.resample.OUT.endswith("libzen_hip_resample.so")
    assert zen_amd.resample.Resampler and addon_build.resample.DEMO.endswith(os.path.join("bin", "zen-shift"))
    assert "LIBRARIES[name]" in open(_addon.__file__).read()


def test_library_finds_the_engine_library_beside_itself(resample_so):
    out = subprocess.run(["readelf", "-d", resample_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    assert "libzen_hip.so" in out and "$ORIGIN" in out and "libzen_hip_tsm" not in out


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "zen_hip_resample.h"\nint main(void){zen_hip_resample_stats_t s; s.calls = 0; return ZEN_HIP_RESAMPLE_KERNELS - 2 + '
                   'ZEN_HIP_OK + ZEN_HIP_RESAMPLE_TILE - 256 + ZEN_HIP_RESAMPLE_PHASES - 512 + ZEN_HIP_RESAMPLE_MAX_POLY - 4096 + '
                   'ZEN_HIP_RESAMPLE_ROUTE_POLY - 1 + (int)s.calls;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.dirname(HDR), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_build_keeps_the_arithmetic_contract_and_the_engines_apart():
    """no fast-math flag, contraction off, no flag that flushes denormals, no flags of a file's own; the sources see the public
    headers, their own, tsm's public header (the demo) and zen_amd/addon's only -- nothing of csrc; no inline assembly and no
    atomics; nothing was added to the shared headers"""
    from zen_amd.addon_build import resample as addon
    assert "-ffp-contract=off" in addon.FLAGS and "-fno-fast-math" in addon.FLAGS and not addon.FILE_FLAGS
    assert not any(("fast-math" in f and f != "-fno-fast-math") or "denormal" in f or "ftz" in f for f in addon.FLAGS)
    assert sorted(os.listdir(addon.SRC)) == ["resample.hip", "resample_kernels.h", "resample_kernels.hip", "resample_main.cpp", "zen_hip_resample.h"]
    for name in os.listdir(addon.SRC):
        text = open(os.path.join(addon.SRC, name)).read()
        code = re.sub(r"//.*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
        assert "csrc/" not in code and "asm" not in code and "atomic" not in code, name
        allowed = ("zen_hip.h", "zen_hip_resample.h", "resample_kernels.h", "wav.h", "demo.h", "../addon/addon_host.h")
        for inc in re.findall(r'#include "([^"]+)"', text):
            assert inc in allowed or (name == "resample_main.cpp" and inc == "zen_hip_tsm.h"), (name, inc)
    assert sorted(os.listdir(os.path.join(ROOT, "zen_amd", "addon"))) == ["addon_host.h", "hpri_pair.h", "median_select.h", "row_walk.h", "stft_args.h", "stft_host.h", "stft_kernels.h"]


def test_demo_program_is_built_and_states_its_usage(resample_so):
    from zen_amd.addon_build import resample as addon
    exe = addon.build_demo()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 2 and "usage: zen-shift in.wav -s semitones -o out.wav" in r.stderr and "--rate hertz" in r.stderr
    for args in (["in.wav", "-s", "25", "-o", "out.wav"], ["in.wav", "-s", "3", "--rate", "8000", "-o", "out.wav"], ["in.wav", "-o", "out.wav"],
                 ["in.wav", "-s", "3", "-o", "out.wav", "--quality", "12"]):
        r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert r.returncode == 2, args
    out = subprocess.run(["readelf", "-d", exe], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    assert "libzen_hip_resample.so" in out and "libzen_hip_tsm.so" in out and "libzen_hip.so" in out


def test_demo_program_refuses_a_rate_out_of_range_before_a_device(resample_so, tmp_path):
    import struct
    from zen_amd.addon_build import resample as addon
    x = np.zeros(1000, "<f4")
    wav = str(tmp_path / "clip.wav")
    with open(wav, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + x.nbytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 3, 1, 8000, 32000, 4, 32) + b"data"
                + struct.pack("<I", x.nbytes) + x.tobytes())
    r = subprocess.run([addon.build_demo(), wav, "--rate", "40000", "-o", str(tmp_path / "out.wav")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 1 and "outside 1/4..4" in r.stderr
    assert not os.path.exists(str(tmp_path / "out.wav"))
