"""CPU-side checks of the PCM16 boundary (zen_amd/pcm/zen_hip_pcm.h): the header is C99, every function it declares is
exported by libzen_hip_pcm.so and bound in zen_amd/pcm.py, and the library loads without a GPU.  The engine's own symbol
table (zen_amd.lib.SYMBOLS == include/zen_hip.h, tests/test_abi.py) is not touched by the new bindings."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "zen_amd", "pcm", "zen_hip_pcm.h")


@pytest.fixture(scope="module")
def pcm_so():
    from zen_amd.addon_build import pcm as addon
    if not os.path.exists(addon.OUT):
        addon.build()
    return addon.OUT


def declared_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zen_hip_pcm_[a-z0-9_]+)\s*\(", hdr)))


def test_header_symbols_are_bound_and_exported(pcm_so):
    from zen_amd import lib, pcm
    L = ctypes.CDLL(pcm_so)
    names = declared_symbols()
    assert len(names) >= 9 and "zen_hip_pcm_hpr_process_host" in names and "zen_hip_pcm_hpri_process" in names
    for n in names:
        assert hasattr(L, n), "libzen_hip_pcm.so does not export %s" % n
    assert set(names) == {s[0] for s in pcm.SYMBOLS}
    assert not any(s[0].startswith("zen_hip_pcm") for s in lib.SYMBOLS)


def test_library_loads_without_gpu(pcm_so):
    from zen_amd import pcm
    L = pcm.load()
    assert b"gfx950" in L.zen_hip_pcm_version()
    assert L.zen_hip_pcm_last_error() == b""
    # argument checks come before anything touches a device
    assert L.zen_hip_pcm_to_float(None, 3, 8, None, None) == 2 and b"channels" in L.zen_hip_pcm_last_error()
    assert L.zen_hip_pcm_hpr_process_host(None, None, 1, 1, None, None, None, 0, 1.0, None, 0) == 2
    assert L.zen_hip_pcm_release(12345) == 0        # unknown handle: nothing to do


def test_library_finds_the_engine_library_beside_itself(pcm_so):
    out = subprocess.run(["readelf", "-d", pcm_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    assert "libzen_hip.so" in out and "$ORIGIN" in out


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "zen_hip_pcm.h"\nint main(void){return ZEN_HIP_PCM_PEAK + ZEN_HIP_OK;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.dirname(HDR), "-c", str(src), "-o", str(tmp_path / "t.o")])
    conv = tmp_path / "c.c"
    conv.write_text('#include "pcm_convert.h"\nint main(void){return float_to_pcm16(pcm16_to_float(0)) + stereo_to_mono(0, 0) > 1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.dirname(HDR), "-c", str(conv),
                           "-o", str(tmp_path / "c.o")])


def test_kernel_sources_keep_the_arithmetic_contract():
    """no fast-math flag, contraction off, and the rounding is not floorf(v + 0.5f)"""
    from zen_amd.addon_build import pcm as addon
    assert "-ffp-contract=off" in addon.FLAGS and "-fno-fast-math" in addon.FLAGS
    assert not any("fast-math" in f and f != "-fno-fast-math" for f in addon.FLAGS)
    conv = open(os.path.join(ROOT, "zen_amd", "pcm", "pcm_convert.h")).read()
    code = re.sub(r"/\*.*?\*/", "", conv, flags=re.S)
    assert "floorf" not in code and "__fdividef" not in code and "/ 32767.f" in code
