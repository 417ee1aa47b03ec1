"""CPU-side checks of the cqt library's boundary (zen_amd/cqt/zen_hip_cqt.h): the header is plain C, every function it declares
is exported by libzen_hip_cqt.so and bound in zen_amd/cqt.py, the library loads without a GPU and refuses bad arguments before
it touches a device, its two host functions (the plan and the tables) are the model's bit for bit, and it is built with the
arithmetic contract's flags."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HDR = os.path.join(ROOT, "zen_amd", "cqt", "zen_hip_cqt.h")
sys.path.insert(0, HERE)
import cqt_model as M  # noqa: E402

TOO_BIG, BAD, UNSUPPORTED = 1, 2, 5
SHAPES = [(256, 4, 300.0, 8000.0), (256, 12, 100.0, 8000.0), (1024, 12, 60.0, 8000.0), (64, 3, 500.0, 8000.0), (256, 1, 300.0, 8000.0),
          (32768, 48, 60.0, 44100.0), (16384, 12, 60.0, 44100.0), (4096, 96, 27.5, 22050.0)]


@pytest.fixture(scope="module")
def cqt_so():
    from zen_amd.addon_build import cqt as addon
    if not os.path.exists(addon.OUT):
        addon.build()
    return addon.OUT


def declared_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zen_hip_cqt_[a-z0-9_]+)\s*\(", hdr)))


def test_header_symbols_are_bound_and_exported(cqt_so):
    from zen_amd import cqt, lib
    L = ctypes.CDLL(cqt_so)
    names = declared_symbols()
    assert len(names) == 17 and "zen_hip_cqt_separate_device" in names and "zen_hip_cqt_inverse_device" in names
    for n in names:
        assert hasattr(L, n), "libzen_hip_cqt.so does not export %s" % n
    assert set(names) == {s[0] for s in cqt.SYMBOLS}
    assert not any(s[0].startswith("zen_hip_cqt") for s in lib.SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", cqt_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    syms = [line.split()[-1] for line in out.splitlines() if line.strip()]
    assert {s for s in syms if s.startswith("zen_hip_")} == set(names)
    assert not [s for s in syms if "zen_addon" in s], "zen_amd/addon is header-only with internal linkage"
    assert len(cqt.KERNELS) == 12


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d_%d" % s[:2])
def test_plan_and_tables_are_the_models_bit_for_bit(cqt_so, shape):
    from zen_amd import cqt
    Ls, B, fmin, fs = shape
    pl = M.Plan(fs, Ls, B, fmin)
    nb, m, p = cqt.plan(fs, Ls, B, fmin)
    assert (nb, m) == (pl.nb, pl.M) and p.tolist() == pl.p
    want = {cqt.TABLE_KB: pl.kb, cqt.TABLE_GL: pl.gL, cqt.TABLE_GU: pl.gU, cqt.TABLE_GDL: pl.gdL, cqt.TABLE_GDU: pl.gdU, cqt.TABLE_H: pl.h,
            cqt.TABLE_S: pl.s}
    for which, w in want.items():
        got = cqt.table(fs, Ls, B, fmin, which)
        assert got.dtype == w.dtype and got.shape == w.shape
        assert np.array_equal(got.view(np.uint32), w.view(np.uint32)), "table %d" % which


def test_plan_of_the_issue(cqt_so):
    from zen_amd import cqt
    nb, m, p = cqt.plan(8000.0, 256, 4, 300.0)
    assert (nb, m) == (15, 64) and p[:4].tolist() == [0, 10, 14, 18] and p[-3:].tolist() == [88, 105, 128]
    assert cqt.plan(8000.0, 256, 12, 100.0)[:2] == (29, 32) and cqt.plan(8000.0, 1024, 12, 60.0)[:2] == (52, 64)
    assert cqt.plan(8000.0, 64, 3, 500.0)[:2] == (8, 32)


def test_plan_and_table_refuse_bad_parameters_and_short_buffers(cqt_so):
    from zen_amd import cqt
    L = cqt.load()
    err = L.zen_hip_cqt_last_error
    nb, m = ctypes.c_size_t(77), ctypes.c_size_t(77)
    out = np.full(300, 7, np.int32)
    for Ls in (48, 96, 32, 65536, 0):
        assert L.zen_hip_cqt_plan(8000.0, Ls, 4, 300.0, ctypes.byref(nb), ctypes.byref(m), None, 0) == BAD and b"power of two in 64..32768" in err()
    assert L.zen_hip_cqt_plan(8000.0, 256, 0, 300.0, ctypes.byref(nb), ctypes.byref(m), None, 0) == BAD and b"bands per octave" in err()
    assert L.zen_hip_cqt_plan(8000.0, 256, 97, 300.0, ctypes.byref(nb), ctypes.byref(m), None, 0) == BAD
    assert L.zen_hip_cqt_plan(8000.0, 256, 4, 0.0, ctypes.byref(nb), ctypes.byref(m), None, 0) == BAD and b"lowest band" in err()
    assert L.zen_hip_cqt_plan(0.0, 256, 4, 300.0, ctypes.byref(nb), ctypes.byref(m), None, 0) == BAD and b"sample rate" in err()
    assert L.zen_hip_cqt_plan(8000.0, 64, 3, 3900.0, ctypes.byref(nb), ctypes.byref(m), None, 0) == BAD and b"fewer than 3" in err()
    assert L.zen_hip_cqt_plan(8000.0, 64, 3, 1e300, ctypes.byref(nb), ctypes.byref(m), None, 0) == BAD
    assert (nb.value, m.value) == (77, 77)
    assert L.zen_hip_cqt_plan(8000.0, 256, 4, 300.0, None, None, out.ctypes.data, 14) == BAD and b"15" in err() and np.all(out == 7)
    assert L.zen_hip_cqt_plan(8000.0, 256, 4, 300.0, None, None, out.ctypes.data, 15) == 0 and out[14] == 128 and np.all(out[15:] == 7)
    out[:] = 7
    p = out.ctypes.data
    assert L.zen_hip_cqt_table(8000.0, 256, 4, 300.0, 7, p, 300) == BAD and L.zen_hip_cqt_table(8000.0, 256, 4, 300.0, -1, p, 300) == BAD
    assert L.zen_hip_cqt_table(8000.0, 256, 4, 300.0, cqt.TABLE_KB, None, 300) == BAD
    assert L.zen_hip_cqt_table(8000.0, 256, 4, 300.0, cqt.TABLE_KB, p, 128) == BAD and b"129" in err()
    assert L.zen_hip_cqt_table(8000.0, 256, 4, 300.0, cqt.TABLE_H, p, 255) == BAD and L.zen_hip_cqt_table(8000.0, 48, 4, 300.0, cqt.TABLE_H, p, 300) == BAD
    assert np.all(out == 7)
    assert L.zen_hip_cqt_table(8000.0, 256, 4, 300.0, cqt.TABLE_KB, p, 129) == 0 and out[128] == 14 and np.all(out[129:] == 7)


def test_library_loads_without_gpu_and_checks_arguments_first(cqt_so):
    from zen_amd import cqt
    L = cqt.load()
    err = L.zen_hip_cqt_last_error
    assert b"gfx950" in L.zen_hip_cqt_version()
    h = ctypes.c_void_p()
    create = L.zen_hip_cqt_create
    for Ls in (48, 96, 1000):
        assert create(8000.0, Ls, 4, 300.0, 1, 1000, ctypes.byref(h)) == BAD and b"power of two in 64..32768" in err()
    for Ls in (32, 65536, 0):
        assert create(8000.0, Ls, 4, 300.0, 1, 1000, ctypes.byref(h)) == BAD and b"power of two in 64..32768" in err()
    for B in (0, 97, -3):
        assert create(8000.0, 256, B, 300.0, 1, 1000, ctypes.byref(h)) == BAD and b"bands per octave" in err()
    assert create(8000.0, 64, 3, 3900.0, 1, 100, ctypes.byref(h)) == BAD and b"fewer than 3" in err()
    # 4095 hops of 128 are 4096 slices: one sample more is one slice too many
    assert create(8000.0, 256, 4, 300.0, 1, 4095 * 128 + 1, ctypes.byref(h)) == BAD and b"4096 slices" in err()
    assert create(8000.0, 256, 4, 300.0, 1, 1 << 40, ctypes.byref(h)) == BAD and b"4096 slices" in err()
    assert create(8000.0, 256, 4, 300.0, 0, 1000, ctypes.byref(h)) == BAD and create(8000.0, 256, 4, 300.0, 1, 0, ctypes.byref(h)) == BAD
    assert create(8000.0, 256, 4, 300.0, 1, 1000, None) == BAD
    assert create(float("nan"), 256, 4, 300.0, 1, 1000, ctypes.byref(h)) == BAD and b"sample rate" in err()
    assert create(8000.0, 256, 4, float("inf"), 1, 1000, ctypes.byref(h)) == BAD
    assert create(8000.0, 256, 4, 300.0, 1 << 17, 1000, ctypes.byref(h)) == BAD and b"n_clips" in err()
    # 65536 clips of 4096 slices of 15 bands: more rows than one batched transform takes
    assert create(8000.0, 256, 4, 300.0, 1 << 16, 4095 * 128, ctypes.byref(h)) == UNSUPPORTED and b"batched transform" in err()
    assert h.value is None
    assert L.zen_hip_cqt_separate_device(None, None, 0, None, None, None, 0) == BAD and b"null handle" in err()
    assert L.zen_hip_cqt_separate_host(None, None, 0, None, None, None, 0) == BAD and b"null handle" in err()
    assert L.zen_hip_cqt_forward_device(None, None, 0, None) == BAD and L.zen_hip_cqt_spectrogram_device(None, None, 0, None, 0) == BAD
    assert L.zen_hip_cqt_inverse_device(None, None, None, 0) == BAD
    assert L.zen_hip_cqt_stats(None, None) == BAD and L.zen_hip_cqt_shape(None, None) == BAD and L.zen_hip_cqt_profile(None, 1) == BAD
    assert L.zen_hip_cqt_set_stream(None, None) == BAD and L.zen_hip_cqt_set_params(None, 2.0, 0, 0, 0) == BAD
    assert L.zen_hip_cqt_profile_get(None, None, None, None) == BAD
    assert L.zen_hip_cqt_destroy(None) == 0


def test_cqt_is_registered_beside_the_others():
    import zen_amd
    from zen_amd import addon_build
    assert addon_build.LIBRARIES["cqt"] is addon_build.cqt is zen_amd.cqt_build
    assert addon_build.cqt.FLAGS is addon_build.FLAGS and addon_build.cqt.DEMO.endswith(os.path.join("bin", "zen-cqt"))
    assert zen_amd.cqt.Cqt and addon_build.cqt.OUT.endswith("libzen_hip_cqt.so")


def test_library_finds_the_engine_library_beside_itself(cqt_so):
    out = subprocess.run(["readelf", "-d", cqt_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    assert "libzen_hip.so" in out and "$ORIGIN" in out


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "zen_hip_cqt.h"\nint main(void){zen_hip_cqt_stats_t s; zen_hip_cqt_shape_t g; s.calls = 0; g.run = 0; return '
                   'ZEN_HIP_CQT_KERNELS - 12 + ZEN_HIP_OK + ZEN_HIP_CQT_TABLE_S - 6 + ZEN_HIP_CQT_MAX_SLICES - 4096 + (int)s.calls + (int)g.run;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.dirname(HDR), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_build_keeps_the_arithmetic_contract_and_the_engines_apart():
    """no fast-math flag, contraction off, no flag that flushes denormals; the sources see the public headers, their own and
    zen_amd/addon's only -- nothing of csrc; nothing was added to the shared headers"""
    from zen_amd.addon_build import cqt as addon
    assert "-ffp-contract=off" in addon.FLAGS and "-fno-fast-math" in addon.FLAGS and not addon.FILE_FLAGS
    assert not any(("fast-math" in f and f != "-fno-fast-math") or "denormal" in f or "ftz" in f for f in addon.FLAGS)
    assert sorted(os.listdir(addon.SRC)) == ["cqt.hip", "cqt_kernels.h", "cqt_kernels.hip", "cqt_main.cpp", "zen_hip_cqt.h"]
    for name in os.listdir(addon.SRC):
        text = open(os.path.join(addon.SRC, name)).read()
        assert "csrc/" not in re.sub(r"//.*", "", text), name
        for inc in re.findall(r'#include "([^"]+)"', text):
            assert inc in ("zen_hip.h", "zen_hip_cqt.h", "cqt_kernels.h", "wav.h", "demo.h", "../addon/addon_host.h"), (name, inc)
    assert sorted(os.listdir(os.path.join(ROOT, "zen_amd", "addon"))) == ["addon_host.h", "hpri_pair.h", "median_select.h", "row_walk.h", "stft_args.h", "stft_host.h", "stft_kernels.h"]


def test_demo_program_is_built_and_states_its_usage(cqt_so):
    from zen_amd.addon_build import cqt as addon
    exe = addon.build_demo()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 2 and "usage: zen-cqt in.wav -o prefix" in r.stderr and "--soft-mask" in r.stderr and "4096 slices" in r.stderr
