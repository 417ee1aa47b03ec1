"""CPU-side checks of the beat library's boundary (zen_amd/beat/zen_hip_beat.h): the header is plain C, every function it
declares is exported by libzen_hip_beat.so and bound in zen_amd/beat.py, the library loads without a GPU and refuses bad
arguments before it touches a device, its host tables are the model's bit for bit, and it is built with the arithmetic
contract's flags."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HDR = os.path.join(ROOT, "zen_amd", "beat", "zen_hip_beat.h")
sys.path.insert(0, HERE)
import beat_model as M  # noqa: E402


@pytest.fixture(scope="module")
def beat_so():
    from zen_amd.addon_build import beat as addon
    if not os.path.exists(addon.OUT):
        addon.build()
    return addon.OUT


def declared_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zen_hip_beat_[a-z0-9_]+)\s*\(", hdr)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_header_symbols_are_bound_and_exported(beat_so):
    from zen_amd import beat, lib
    L = ctypes.CDLL(beat_so)
    names = declared_symbols()
    assert len(names) == 12 and "zen_hip_beat_run_device" in names and "zen_hip_beat_table" in names
    for n in names:
        assert hasattr(L, n), "libzen_hip_beat.so does not export %s" % n
    assert set(names) == {s[0] for s in beat.SYMBOLS}
    assert not any(s[0].startswith("zen_hip_beat") for s in lib.SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", beat_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    syms = [line.split()[-1] for line in out.splitlines() if line.strip()]
    assert {s for s in syms if s.startswith("zen_hip_")} == set(names)
    assert not [s for s in syms if "zen_addon" in s], "zen_amd/addon is header-only with internal linkage"


def test_library_loads_without_gpu_and_checks_arguments_first(beat_so):
    from zen_amd import beat
    L = beat.load()
    assert b"gfx950" in L.zen_hip_beat_version()
    h = ctypes.c_void_p()
    for hop in (96, 4096, 0, 32):
        assert L.zen_hip_beat_create(44100.0, hop, 1, 0, ctypes.byref(h)) == 2 and b"power of two" in L.zen_hip_beat_last_error()
    for fs, hop in M.REFUSED:
        assert not M.accepted(fs, hop)
        assert L.zen_hip_beat_create(fs, hop, 1, 0, ctypes.byref(h)) == 2 and b"beat periods" in L.zen_hip_beat_last_error()
    assert L.zen_hip_beat_create(44100.0, 512, 0, 0, ctypes.byref(h)) == 2
    assert L.zen_hip_beat_create(44100.0, 512, 1, 0, None) == 2
    assert L.zen_hip_beat_create(0.0, 512, 1, 0, ctypes.byref(h)) == 2
    assert h.value is None
    assert L.zen_hip_beat_run_device(None, None, 0, 0, None, None, None, None, 0) == 2
    assert L.zen_hip_beat_run_host(None, None, 0, 0, None, None, None, None, 0) == 2
    assert L.zen_hip_beat_stats(None, None) == 2 and L.zen_hip_beat_profile(None, 1) == 2 and L.zen_hip_beat_reset(None) == 2
    assert L.zen_hip_beat_destroy(None) == 0


def test_beat_is_registered_beside_the_four():
    import zen_amd
    from zen_amd import addon_build
    assert addon_build.LIBRARIES["beat"] is addon_build.beat is zen_amd.beat_build
    assert addon_build.beat.FLAGS is addon_build.FLAGS and addon_build.beat.DEMO.endswith(os.path.join("bin", "beat-track"))
    assert zen_amd.beat.Beat and addon_build.beat.OUT.endswith("libzen_hip_beat.so")


@pytest.mark.parametrize("fs,hop", M.ACCEPTED)
def test_host_tables_are_the_models_bit_for_bit(beat_so, fs, hop):
    """zen_hip_beat_table needs no device: the window, the periods, the tempi, both weightings for every distinct period, the
    Rayleigh weighting and every row of the transition matrix"""
    from zen_amd import beat
    t = M.tables(fs, hop)
    assert M.accepted(fs, hop) and t.bp[0] <= 128 and t.bp[-1] >= 4 and t.bp == sorted(t.bp, reverse=True)
    assert np.array_equal(bits(beat.table(fs, hop, beat.TABLE_WINDOW)), bits(t.win)) and t.win.size == 2 * hop
    assert np.array_equal(beat.table(fs, hop, beat.TABLE_PERIOD), np.array(t.bp, np.float32))
    assert np.array_equal(bits(beat.table(fs, hop, beat.TABLE_TEMPO)), bits(t.tempo))
    for b in sorted(set(t.bp)):
        w1, w2 = beat.table(fs, hop, beat.TABLE_PAST, b), beat.table(fs, hop, beat.TABLE_FUTURE, b)
        assert w1.size == M.r2(b) - M.rh(b) + 1 and w2.size == b
        assert np.array_equal(bits(w1), bits(t.w1[b])), b
        assert np.array_equal(bits(w2), bits(t.w2[b])), b
    assert np.array_equal(bits(beat.table(fs, hop, beat.TABLE_RAYLEIGH)), bits(t.rayleigh)) and t.rayleigh[0] == 0
    for i in range(M.N_TEMPI):
        assert np.array_equal(bits(beat.table(fs, hop, beat.TABLE_TRANSITION, i)), bits(t.trans[i])), i
    # what the formulas are: the past window peaks one period back, the tempi are those of the grid within the rounding of bp
    b = t.bp[20]
    assert int(np.argmax(t.w1[b])) == b and t.w1[b][b] == 1.0
    assert np.all(np.abs(t.tempo - (80 + 2 * np.arange(41))) <= (80 + 2 * np.arange(41)) * 0.5 / np.array(t.bp) + 1e-3)


def test_table_refuses_what_create_refuses_and_short_buffers(beat_so):
    from zen_amd import beat
    L = beat.load()
    out = np.empty(4096, np.float32)
    p = out.ctypes.data
    for fs, hop in M.REFUSED + ((44100.0, 96), (44100.0, 4096)):
        assert L.zen_hip_beat_table(fs, hop, beat.TABLE_TEMPO, 0, p, out.size) == 2
    assert L.zen_hip_beat_table(44100.0, 512, beat.TABLE_TEMPO, 0, p, 40) == 2 and b"41" in L.zen_hip_beat_last_error()
    assert L.zen_hip_beat_table(44100.0, 512, beat.TABLE_TEMPO, 0, None, 41) == 2
    assert L.zen_hip_beat_table(44100.0, 512, 7, 0, p, out.size) == 2
    assert L.zen_hip_beat_table(44100.0, 512, beat.TABLE_PAST, 3, p, out.size) == 2        # 3 is no period of 44100/512
    assert L.zen_hip_beat_table(44100.0, 512, beat.TABLE_TRANSITION, 41, p, out.size) == 2
    out[:] = 7.0
    assert L.zen_hip_beat_table(44100.0, 512, beat.TABLE_TEMPO, 0, p, 41) == 0 and np.all(out[41:] == 7.0)


def test_library_finds_the_engine_library_beside_itself(beat_so):
    out = subprocess.run(["readelf", "-d", beat_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    assert "libzen_hip.so" in out and "$ORIGIN" in out


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "zen_hip_beat.h"\nint main(void){zen_hip_beat_stats_t s; s.hops = 0; return ZEN_HIP_BEAT_KERNELS - 4 + ZEN_HIP_OK '
                   '+ ZEN_HIP_BEAT_TABLE_TRANSITION - 6 + (int)s.hops;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.dirname(HDR), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_build_keeps_the_arithmetic_contract_and_the_engines_apart():
    """no fast-math flag, contraction off, no flag that flushes denormals; the sources see the public headers only; nothing
    was added to the shared headers or to the pitch library"""
    from zen_amd.addon_build import beat as addon
    assert "-ffp-contract=off" in addon.FLAGS and "-fno-fast-math" in addon.FLAGS and not addon.FILE_FLAGS
    assert not any(("fast-math" in f and f != "-fno-fast-math") or "denormal" in f or "ftz" in f for f in addon.FLAGS)
    for name in os.listdir(addon.SRC):
        text = open(os.path.join(addon.SRC, name)).read()
        assert "csrc/" not in re.sub(r"//.*", "", text), name
        for inc in re.findall(r'#include "([^"]+)"', text):
            assert inc in ("zen_hip.h", "zen_hip_beat.h", "beat_kernels.h", "beat_tables.h", "wav.h", "demo.h", "../addon/addon_host.h"), (name, inc)
    assert sorted(os.listdir(os.path.join(ROOT, "zen_amd", "addon"))) == ["addon_host.h", "hpri_pair.h", "median_select.h", "row_walk.h", "stft_args.h", "stft_host.h", "stft_kernels.h"]


def test_demo_program_is_built_and_states_its_usage(beat_so):
    from zen_amd.addon_build import beat as addon
    exe = addon.build_demo()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 2 and "usage: beat-track in.wav" in r.stderr
