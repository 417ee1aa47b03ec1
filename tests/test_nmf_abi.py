"""CPU-side checks of the nmf library's boundary (zen_amd/nmf/zen_hip_nmf.h): the header is plain C, every function it declares
is exported by libzen_hip_nmf.so and bound in zen_amd/nmf.py, the library loads without a GPU and refuses bad arguments before
it touches a device, its initial values and tables are the model's bit for bit, it is built with the arithmetic contract's
flags, and a .znmf file round-trips."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HDR = os.path.join(ROOT, "zen_amd", "nmf", "zen_hip_nmf.h")
sys.path.insert(0, HERE)
import nmf_model as M  # noqa: E402

BAD = 2


@pytest.fixture(scope="module")
def nmf_so():
    from zen_amd.addon_build import nmf as addon
    if not os.path.exists(addon.OUT):
        addon.build()
    return addon.OUT


def declared_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zen_hip_nmf_[a-z0-9_]+)\s*\(", hdr)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_header_symbols_are_bound_and_exported(nmf_so):
    from zen_amd import lib, nmf
    L = ctypes.CDLL(nmf_so)
    names = declared_symbols()
    assert len(names) == 15
    for n in ("process_device", "process_host", "ratio_device", "update_h_device", "update_w_device", "init", "stats", "table", "set_stream",
              "profile", "profile_get", "last_error", "version", "create", "destroy"):
        assert "zen_hip_nmf_" + n in names
    for n in names:
        assert hasattr(L, n), "libzen_hip_nmf.so does not export %s" % n
    assert set(names) == {s[0] for s in nmf.SYMBOLS}
    assert not any(s[0].startswith("zen_hip_nmf") for s in lib.SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", nmf_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    syms = [line.split()[-1] for line in out.splitlines() if line.strip()]
    assert {s for s in syms if s.startswith("zen_hip_")} == set(names)
    assert not [s for s in syms if "zen_addon" in s], "zen_amd/addon is header-only with internal linkage"


def test_library_loads_without_gpu_and_checks_arguments_first(nmf_so):
    from zen_amd import nmf
    L = nmf.load()
    err = L.zen_hip_nmf_last_error
    assert b"gfx950" in L.zen_hip_nmf_version()
    h = ctypes.c_void_p()
    for nfft in (48, 16384, 0, 32):
        assert L.zen_hip_nmf_create(44100.0, nfft, 8, 1, 1000, ctypes.byref(h)) == BAD and b"power of two in 64..8192" in err()
    assert L.zen_hip_nmf_create(44100.0, 2048, 8, 0, 1000, ctypes.byref(h)) == BAD and b"zero clips" in err()
    assert L.zen_hip_nmf_create(44100.0, 2048, 8, 1, 1000, None) == BAD
    assert L.zen_hip_nmf_create(0.0, 2048, 8, 1, 1000, ctypes.byref(h)) == BAD and b"sample rate" in err()
    for K in (0, 257, 1 << 40):
        assert L.zen_hip_nmf_create(44100.0, 2048, K, 1, 1000, ctypes.byref(h)) == BAD and b"outside 1..256" in err()
    assert L.zen_hip_nmf_create(44100.0, 2048, 8, 1, 0, ctypes.byref(h)) == BAD
    # 16383 hops of 1024 are 16384 frames: one sample more is one frame too many
    assert L.zen_hip_nmf_create(44100.0, 2048, 8, 1, 16383 * 1024 + 1, ctypes.byref(h)) == BAD and b"16384 frames" in err()
    assert L.zen_hip_nmf_create(8000.0, 64, 8, 1, 1 << 40, ctypes.byref(h)) == BAD and b"16384 frames" in err()
    assert h.value is None
    args = (None, 0, 0, None, 0, 0, None, 0, 0, 0, 0, None, 0, None, 0)
    assert L.zen_hip_nmf_process_device(None, *args) == BAD and b"null handle" in err()
    assert L.zen_hip_nmf_process_host(None, *args) == BAD and b"null handle" in err()
    assert L.zen_hip_nmf_stats(None, None) == BAD and L.zen_hip_nmf_profile(None, 1) == BAD
    assert L.zen_hip_nmf_set_stream(None, None) == BAD and L.zen_hip_nmf_profile_get(None, None, None, None) == BAD
    assert L.zen_hip_nmf_destroy(None) == 0
    assert L.zen_hip_nmf_init(0, 4, None) == BAD and b"null output" in err()
    assert L.zen_hip_nmf_init(0, 4, 18) == BAD and b"misaligned" in err()


def test_the_kernels_alone_refuse_before_a_device_is_touched(nmf_so):
    """null and misaligned pointers, strides below the row, components, frames and bins outside their ranges, a bad route,
    more rows held than there are: the addresses are never read"""
    from zen_amd import nmf
    L = nmf.load()
    err = L.zen_hip_nmf_last_error
    ratio, uph, upw = L.zen_hip_nmf_ratio_device, L.zen_hip_nmf_update_h_device, L.zen_hip_nmf_update_w_device
    K, F, m = 4, 9, 10
    A, B, Cc, D, E = 4096, 8192, 12288, 16384, 20480

    def good_ratio(**kw):
        a = dict(v=A, vs=F, w=B, ws=F, h=Cc, hs=m, K=K, F=F, m=m, q=D, qs=F, lam=E, ls=F, route=0)
        a.update(kw)
        return ratio(a["v"], a["vs"], a["w"], a["ws"], a["h"], a["hs"], a["K"], a["F"], a["m"], a["q"], a["qs"], a["lam"], a["ls"], a["route"], None)

    for kw, text in ((dict(v=None), b"null or misaligned"), (dict(w=None), b"null or misaligned"), (dict(h=None), b"null or misaligned"),
                     (dict(q=None), b"null or misaligned"), (dict(v=A + 2), b"null or misaligned"), (dict(q=D + 1), b"null or misaligned"),
                     (dict(lam=E + 2), b"null or misaligned"), (dict(vs=F - 1), b"stride below its row"), (dict(ws=F - 1), b"stride below its row"),
                     (dict(hs=m - 1), b"stride below its row"), (dict(qs=F - 1), b"stride below its row"), (dict(ls=F - 1), b"stride below its row"),
                     (dict(K=0), b"components, outside 1..256"), (dict(K=257), b"components, outside 1..256"),
                     (dict(m=0, hs=0), b"frames, outside 1..16384"), (dict(m=16385, hs=16385), b"frames, outside 1..16384"),
                     (dict(F=0), b"bins, outside"), (dict(route=3), b"unknown route 3"), (dict(route=-1), b"unknown route -1")):
        assert good_ratio(**kw) == BAD and text in err(), (kw, err())

    def good_uph(**kw):
        a = dict(w=A, ws=F, q=B, qs=F, h=Cc, hs=m, K=K, F=F, m=m, out=D, os=m, route=0)
        a.update(kw)
        return uph(a["w"], a["ws"], a["q"], a["qs"], a["h"], a["hs"], a["K"], a["F"], a["m"], a["out"], a["os"], a["route"], None)

    for kw, text in ((dict(w=None), b"null or misaligned"), (dict(q=None), b"null or misaligned"), (dict(h=None), b"null or misaligned"),
                     (dict(out=None), b"null or misaligned"), (dict(out=D + 3), b"null or misaligned"), (dict(ws=F - 1), b"stride below its row"),
                     (dict(qs=F - 1), b"stride below its row"), (dict(hs=m - 1), b"stride below its row"), (dict(os=m - 1), b"stride below its row"),
                     (dict(K=257), b"components, outside 1..256"), (dict(m=16385, hs=16385, os=16385), b"frames, outside 1..16384"),
                     (dict(route=7), b"unknown route 7")):
        assert good_uph(**kw) == BAD and text in err(), (kw, err())

    def good_upw(**kw):
        a = dict(h=A, hs=m, q=B, qs=F, w=Cc, ws=F, K=K, F=F, m=m, fixed=1, out=D, os=F, route=0)
        a.update(kw)
        return upw(a["h"], a["hs"], a["q"], a["qs"], a["w"], a["ws"], a["K"], a["F"], a["m"], a["fixed"], a["out"], a["os"], a["route"], None)

    for kw, text in ((dict(h=None), b"null or misaligned"), (dict(q=None), b"null or misaligned"), (dict(w=None), b"null or misaligned"),
                     (dict(out=None), b"null or misaligned"), (dict(w=Cc + 2), b"null or misaligned"), (dict(hs=m - 1), b"stride below its row"),
                     (dict(qs=F - 1), b"stride below its row"), (dict(ws=F - 1), b"stride below its row"), (dict(os=F - 1), b"stride below its row"),
                     (dict(K=0), b"components, outside 1..256"), (dict(m=0, hs=0), b"frames, outside 1..16384"), (dict(fixed=K + 1), b"spectra held"),
                     (dict(route=3), b"unknown route 3")):
        assert good_upw(**kw) == BAD and text in err(), (kw, err())
    assert good_upw(fixed=K) == 0        # nothing to update: returns before a device is touched


def test_nmf_is_registered_behind_the_others_and_the_pinned_tables_stand():
    import zen_amd
    from zen_amd import addon_build
    assert addon_build.LIBRARIES["nmf"] is addon_build.nmf is zen_amd.nmf_build
    assert addon_build.nmf.SOURCES == ["nmf_kernels.hip", "nmf.hip"]
    assert addon_build.nmf.FLAGS is addon_build.FLAGS and not addon_build.nmf.FILE_FLAGS
    assert addon_build.nmf.DEMO.endswith(os.path.join("bin", "zen-nmf"))
    from zen_amd import nmf
    assert nmf.Nmf and addon_build.nmf.OUT.endswith("libzen_hip_nmf.so")


@pytest.mark.parametrize("seed", [0, 1, 2 ** 64 - 1, 987654321])
def test_init_gives_the_models_bits(nmf_so, seed):
    from zen_amd import nmf
    got = nmf.init(seed, 1000)
    assert np.array_equal(bits(got), bits(M.init(seed, 1000))) and got.min() > 0 and got.max() <= 1
    assert float(got[0]) == ((M.splitmix64(seed, 0) >> 40) + 1) * 2.0 ** -24
    assert nmf.init(seed, 0).size == 0


@pytest.mark.parametrize("N", [64, 256, 8192])
def test_host_tables_are_the_models_bit_for_bit(nmf_so, N):
    from zen_amd import nmf
    w, d = nmf.table(N, nmf.TABLE_WINDOW), nmf.table(N, nmf.TABLE_DIVISOR)
    assert w.size == N and d.size == N // 2
    assert np.array_equal(bits(w), bits(M.R.window(N))) and np.array_equal(bits(d), bits(M.R.divisor(N)))


def test_table_refuses_bad_frames_and_short_buffers(nmf_so):
    from zen_amd import nmf
    L = nmf.load()
    out = np.full(300, 7.0, np.float32)
    p = out.ctypes.data
    for nfft in (48, 16384, 32):
        assert L.zen_hip_nmf_table(nfft, nmf.TABLE_WINDOW, p, out.size) == BAD
    assert L.zen_hip_nmf_table(256, 2, p, out.size) == BAD and L.zen_hip_nmf_table(256, nmf.TABLE_WINDOW, None, 256) == BAD
    assert L.zen_hip_nmf_table(256, nmf.TABLE_WINDOW, p, 255) == BAD and b"256" in L.zen_hip_nmf_last_error()
    assert L.zen_hip_nmf_table(256, nmf.TABLE_DIVISOR, p, 128) == 0 and np.all(out[128:] == 7.0)


def test_library_finds_the_engine_library_beside_itself(nmf_so):
    out = subprocess.run(["readelf", "-d", nmf_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    assert "libzen_hip.so" in out and "$ORIGIN" in out


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "zen_hip_nmf.h"\nint main(void){zen_hip_nmf_stats_t s; s.calls = 0; return ZEN_HIP_NMF_KERNELS - 12 + ZEN_HIP_OK '
                   '+ ZEN_HIP_NMF_TABLE_DIVISOR - 1 + ZEN_HIP_NMF_MAX_COMPONENTS - 256 + ZEN_HIP_NMF_ROUTE_VALU - 2 + (int)s.calls '
                   '+ ZEN_HIP_NMF_MAX_FRAMES - 16384 + ZEN_HIP_NMF_SEGMENT - 256;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.dirname(HDR), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_build_keeps_the_arithmetic_contract_and_the_other_libraries_apart():
    """no fast-math flag, contraction off, no flag that flushes denormals, no flags per file; the sources see the public
    header, their own two and zen_amd/addon's only; the pinned directories keep exactly their files"""
    from zen_amd.addon_build import nmf as addon
    assert "-ffp-contract=off" in addon.FLAGS and "-fno-fast-math" in addon.FLAGS and not addon.FILE_FLAGS
    assert not any(("fast-math" in f and f != "-fno-fast-math") or "denormal" in f or "ftz" in f for f in addon.FLAGS)
    assert sorted(os.listdir(addon.SRC)) == ["nmf.hip", "nmf_kernels.h", "nmf_kernels.hip", "nmf_main.cpp", "zen_hip_nmf.h"]
    for name in os.listdir(addon.SRC):
        text = open(os.path.join(addon.SRC, name)).read()
        assert "csrc/" not in re.sub(r"//.*", "", text), name
        assert "asm" not in re.sub(r"//.*", "", text).split(), name
        for inc in re.findall(r'#include "([^"]+)"', text):
            assert inc in ("zen_hip.h", "zen_hip_nmf.h", "nmf_kernels.h", "wav.h", "demo.h", "../addon/addon_host.h", "../addon/stft_host.h", "../addon/stft_args.h",
                           "../addon/stft_kernels.h"), (name, inc)
    zen = os.path.join(ROOT, "zen_amd")
    assert sorted(os.listdir(os.path.join(zen, "addon"))) == ["addon_host.h", "hpri_pair.h", "median_select.h", "row_walk.h", "stft_args.h", "stft_host.h", "stft_kernels.h"]
    assert sorted(os.listdir(os.path.join(zen, "repet"))) == ["repet.hip", "repet_kernels.h", "repet_kernels.hip", "repet_main.cpp", "zen_hip_repet.h"]
    assert sorted(os.listdir(os.path.join(zen, "repsim"))) == ["repsim.hip", "repsim_kernels.h", "repsim_kernels.hip", "repsim_main.cpp",
                                                               "zen_hip_repsim.h"]


def test_demo_program_is_built_and_states_its_usage(nmf_so):
    from zen_amd.addon_build import nmf as addon
    exe = addon.build_demo()
    for argv in ([exe], [exe, "train"], [exe, "separate", "mix.wav", "-o", "prefix"], [exe, "nonsense", "a.wav"]):
        r = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert r.returncode == 2 and "usage: zen-nmf train in.wav -o dict.znmf" in r.stderr and "16384 frames" in r.stderr
        assert "zen-nmf separate mix.wav -d a.znmf" in r.stderr
        for opt in ("--nfft", "--components", "--iterations", "--seed", "--free"):
            assert opt in r.stderr


def test_a_znmf_file_round_trips(nmf_so, tmp_path):
    """the documented layout byte for byte, and what the reader refuses"""
    import struct
    from zen_amd import nmf
    W = M.init(9, 3 * 33).reshape(3, 33)
    path = str(tmp_path / "d.znmf")
    nmf.save_znmf(path, W, 64, 8000.0)
    raw = open(path, "rb").read()
    assert raw[:4] == b"ZNMF" and struct.unpack("<IIIf", raw[4:20]) == (1, 64, 3, 8000.0) and len(raw) == 20 + 4 * 99
    assert raw[20:] == W.astype("<f4").tobytes()
    W2, nfft, fs = nmf.load_znmf(path)
    assert nfft == 64 and fs == 8000.0 and np.array_equal(bits(W2), bits(W))
    for bad in (raw[:19], b"ZNMG" + raw[4:], raw[:-1], raw[:4] + struct.pack("<I", 2) + raw[8:]):
        open(path, "wb").write(bad)
        with pytest.raises(ValueError):
            nmf.load_znmf(path)
