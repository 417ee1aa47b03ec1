"""CPU-side checks of the pitch library's boundary (zen_amd/pitch/zen_hip_pitch.h): the header is plain C, every function it
declares is exported by libzen_hip_pitch.so and bound in zen_amd/pitch.py, the library loads without a GPU and refuses bad
arguments before it touches a device, and it is built with the arithmetic contract's flags."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "zen_amd", "pitch", "zen_hip_pitch.h")


@pytest.fixture(scope="module")
def pitch_so():
    from zen_amd.addon_build import pitch as addon
    if not os.path.exists(addon.OUT):
        addon.build()
    return addon.OUT


def declared_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zen_hip_pitch_[a-z0-9_]+)\s*\(", hdr)))


def test_header_symbols_are_bound_and_exported(pitch_so):
    from zen_amd import lib, pitch
    L = ctypes.CDLL(pitch_so)
    names = declared_symbols()
    assert len(names) == 10 and "zen_hip_pitch_run_device" in names and "zen_hip_pitch_profile_get" in names
    for n in names:
        assert hasattr(L, n), "libzen_hip_pitch.so does not export %s" % n
    assert set(names) == {s[0] for s in pitch.SYMBOLS}
    assert not any(s[0].startswith("zen_hip_pitch") for s in lib.SYMBOLS)


def test_library_loads_without_gpu_and_checks_arguments_first(pitch_so):
    from zen_amd import pitch
    L = pitch.load()
    assert b"gfx950" in L.zen_hip_pitch_version()
    h = ctypes.c_void_p()
    for n in (0, 16, 48, 4095, 32768):
        assert L.zen_hip_pitch_create(44100.0, n, 1, 0, ctypes.byref(h)) == 2 and b"power of two" in L.zen_hip_pitch_last_error()
    assert L.zen_hip_pitch_create(44100.0, 4096, 0, 0, ctypes.byref(h)) == 2
    assert L.zen_hip_pitch_create(44100.0, 4096, 1, 0, None) == 2
    assert h.value is None
    assert L.zen_hip_pitch_run_device(None, None, 0, 0, 1, None, None, None, None, 0) == 2
    assert L.zen_hip_pitch_run_host(None, None, 0, 0, 1, None, None, None, None, 0) == 2
    assert L.zen_hip_pitch_stats(None, None) == 2 and L.zen_hip_pitch_profile(None, 1) == 2
    assert L.zen_hip_pitch_destroy(None) == 0


def test_library_finds_the_engine_library_beside_itself(pitch_so):
    out = subprocess.run(["readelf", "-d", pitch_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    assert "libzen_hip.so" in out and "$ORIGIN" in out


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "zen_hip_pitch.h"\nint main(void){zen_hip_pitch_stats_t s; s.chunks = 0; return ZEN_HIP_PITCH_KERNELS - 5 + ZEN_HIP_OK '
                   '+ (int)s.chunks;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.dirname(HDR), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_build_keeps_the_arithmetic_contract_and_the_engines_apart():
    """no fast-math flag, contraction off; the sources see the public headers only"""
    from zen_amd.addon_build import pitch as addon
    assert "-ffp-contract=off" in addon.FLAGS and "-fno-fast-math" in addon.FLAGS
    assert not any("fast-math" in f and f != "-fno-fast-math" for f in addon.FLAGS)
    for name in os.listdir(addon.SRC):
        text = open(os.path.join(addon.SRC, name)).read()
        assert "csrc/" not in re.sub(r"//.*", "", text), name
        for inc in re.findall(r'#include "([^"]+)"', text):
            assert inc in ("zen_hip.h", "zen_hip_pitch.h", "pitch_kernels.h", "wav.h", "demo.h", "../addon/addon_host.h"), (name, inc)


def test_demo_program_is_built_and_states_its_usage(pitch_so):
    from zen_amd.addon_build import pitch as addon
    exe = addon.build_demo()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 2 and "usage: pitch-track in.wav" in r.stderr
