"""CPU-side checks of the multichannel library's boundary (zen_amd/multi/zen_hip_multi.h): the header is plain C, every function
it declares is exported by libzen_hip_multi.so and bound in zen_amd/multi.py, the library loads without a GPU and refuses bad
arguments before it touches a device, it is registered beside beat, and its sources see the public headers only."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HDR = os.path.join(ROOT, "zen_amd", "multi", "zen_hip_multi.h")


@pytest.fixture(scope="module")
def multi_so():
    from zen_amd.addon_build import multi as addon
    if not os.path.exists(addon.OUT):
        addon.build()
    return addon.OUT


def declared_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zen_hip_multi_[a-z0-9_]+)\s*\(", hdr)))


def test_header_symbols_are_bound_and_exported(multi_so):
    from zen_amd import lib, multi
    L = ctypes.CDLL(multi_so)
    names = declared_symbols()
    assert len(names) == 21 and "zen_hip_multi_split" in names and "zen_hip_multi_realtime_host" in names
    for n in names:
        assert hasattr(L, n), "libzen_hip_multi.so does not export %s" % n
    assert set(names) == {s[0] for s in multi.SYMBOLS}
    assert not any(s[0].startswith("zen_hip_multi") for s in lib.SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", multi_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    syms = [line.split()[-1] for line in out.splitlines() if line.strip()]
    assert {s for s in syms if s.startswith("zen_hip_")} == set(names)
    assert not [s for s in syms if "zen_addon" in s], "zen_amd/addon is header-only with internal linkage"


def test_library_loads_without_gpu_and_checks_arguments_first(multi_so):
    from zen_amd import multi
    L = multi.load()
    err = L.zen_hip_multi_last_error
    assert b"gfx950" in L.zen_hip_multi_version()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    h = ctypes.c_void_p()
    for ch in (0, 9, -1):
        assert L.zen_hip_multi_split(multi.I16, p, ch, 4, p, 4, None) == 2
        assert err() == b"multi_split: channels must be 1..8 (got %d)" % ch
        assert L.zen_hip_multi_peak(p, ch, 4, 4, p, None) == 2 and err().startswith(b"multi_peak: channels must be 1..8")
        assert L.zen_hip_multi_join(multi.F32, p, ch, 4, 4, multi.GAIN, 1.0, None, p, None) == 2 and err().startswith(b"multi_join: channels must be 1..8")
        assert L.zen_hip_multi_offline_create(44100.0, 1024, 256, 2.0, 2.0, 0, ch, ctypes.byref(h)) == 2
        assert err() == b"multi_offline_create: channels must be 1..8 (got %d)" % ch
        assert L.zen_hip_multi_realtime_create(44100.0, 256, 2.0, 7, ch, 0, ctypes.byref(h)) == 2
        assert err() == b"multi_realtime_create: channels must be 1..8 (got %d)" % ch
    assert h.value is None
    # formats, modes, null pointers, alignment and the row stride, all before a device is touched
    assert L.zen_hip_multi_split(2, p, 2, 4, p, 4, None) == 2 and b"format" in err()
    assert L.zen_hip_multi_split(multi.I16, None, 2, 4, p, 4, None) == 2 and b"null interleaved buffer" in err()
    assert L.zen_hip_multi_split(multi.I16, p, 2, 4, None, 4, None) == 2 and b"null rows" in err()
    assert L.zen_hip_multi_split(multi.I16, p, 2, 4, p, 3, None) == 2 and err() == b"multi_split: row_stride 3 below the 4 frames of a row"
    assert L.zen_hip_multi_split(multi.I16, p + 1, 2, 4, p, 4, None) == 2 and b"2-byte alignment" in err()
    assert L.zen_hip_multi_split(multi.F32, p + 2, 2, 4, p, 4, None) == 2 and b"4-byte alignment" in err()
    assert L.zen_hip_multi_join(multi.I16, p, 2, 4, 4, 5, 1.0, None, p, None) == 2 and b"mode" in err()
    assert L.zen_hip_multi_join(multi.I16, p, 2, 4, 4, multi.PEAK, 1.0, None, p, None) == 2 and b"minmax_dev" in err()
    assert L.zen_hip_multi_peak(p, 2, 4, 4, None, None) == 2 and b"minmax_dev" in err()
    # n_frames == 0 is legal and touches nothing: not even the pointers are looked at
    assert L.zen_hip_multi_split(multi.I16, None, 2, 0, None, 0, None) == 0
    assert L.zen_hip_multi_peak(None, 2, 0, 0, None, None) == 0
    assert L.zen_hip_multi_join(multi.I16, None, 2, 0, 0, multi.GAIN, 1.0, None, None, None) == 0
    # null handles
    assert L.zen_hip_multi_offline_create(44100.0, 1024, 256, 2.0, 2.0, 0, 2, None) == 2 and err() == b"multi_offline_create: null handle"
    assert L.zen_hip_multi_realtime_create(44100.0, 256, 2.0, 7, 2, 0, None) == 2 and err() == b"multi_realtime_create: null handle"
    assert L.zen_hip_multi_offline_device(None, 0, p, 4, p, None, 0, 1.0, None) == 2 and err() == b"multi_offline_device: null handle"
    assert L.zen_hip_multi_offline_host(None, 0, p, 4, p, None, 0, 1.0, None) == 2 and err() == b"multi_offline_host: null handle"
    assert L.zen_hip_multi_realtime_device(None, 0, p, 4, p, None, None, 1.0) == 2 and err() == b"multi_realtime_device: null handle"
    assert L.zen_hip_multi_realtime_host(None, 0, p, 4, p, None, None, 1.0) == 2 and err() == b"multi_realtime_host: null handle"
    for f in ("offline_use_sse_filter", "offline_use_soft_mask", "realtime_use_sse_filter", "realtime_use_soft_mask", "realtime_reset"):
        assert getattr(L, "zen_hip_multi_" + f)(None) == 2 and err() == ("multi_%s: null handle" % f).encode()
    assert L.zen_hip_multi_offline_set_stream(None, None) == 2 and L.zen_hip_multi_realtime_set_stream(None, None) == 2
    assert L.zen_hip_multi_stats(None, None) == 2
    assert L.zen_hip_multi_offline_destroy(None) == 0 and L.zen_hip_multi_realtime_destroy(None) == 0


def test_binding_refuses_shapes_and_dtypes_before_the_library():
    from zen_amd import multi
    with pytest.raises(TypeError):
        multi._frames(np.zeros((4, 2), np.float64), 2)
    with pytest.raises(ValueError):
        multi._frames(np.zeros((4, 3), np.int16), 2)
    x, fmt = multi._frames(np.zeros((6, 2), np.int16)[::2], 2)
    assert fmt == multi.I16 and x.flags.c_contiguous and x.shape == (3, 2)
    x, fmt = multi._frames(np.zeros(5, np.float32), 1)
    assert fmt == multi.F32 and x.shape == (5, 1)


def test_multi_is_registered_beside_beat():
    import zen_amd
    from zen_amd import addon_build
    assert addon_build.LIBRARIES["multi"] is addon_build.multi is zen_amd.multi_build
    assert addon_build.multi.FLAGS is addon_build.FLAGS and not addon_build.multi.FILE_FLAGS
    assert addon_build.multi.DEMO.endswith(os.path.join("bin", "zen-stems"))
    assert addon_build.multi.SOURCES == ["multi_kernels.hip", "multi.hip"]
    assert os.path.join(ROOT, "zen_amd", "pcm", "pcm_convert.h") in addon_build.multi.deps()
    assert zen_amd.multi.Offline and zen_amd.multi.Realtime and addon_build.multi.OUT.endswith("libzen_hip_multi.so")


def test_library_finds_the_engine_library_beside_itself(multi_so):
    out = subprocess.run(["readelf", "-d", multi_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    assert "libzen_hip.so" in out and "$ORIGIN" in out and "libzen_hip_pcm" not in out


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "zen_hip_multi.h"\nint main(void){zen_hip_multi_stats_t s; s.calls = 0; return ZEN_HIP_MULTI_MAX_CHANNELS - 8 + ZEN_HIP_OK '
                   '+ ZEN_HIP_MULTI_F32 - 1 + ZEN_HIP_MULTI_GAIN - 1 + ZEN_HIP_MULTI_I16 + ZEN_HIP_MULTI_PEAK + (int)s.calls;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.dirname(HDR), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_sources_see_the_listed_headers_only_and_nothing_of_the_engines():
    from zen_amd.addon_build import multi as addon
    assert "-ffp-contract=off" in addon.FLAGS and "-fno-fast-math" in addon.FLAGS
    assert sorted(os.listdir(addon.SRC)) == ["multi.hip", "multi_kernels.h", "multi_kernels.hip", "multi_stems.cpp", "zen_hip_multi.h"]
    allowed = ("zen_hip.h", "zen_hip_multi.h", "multi_kernels.h", "wav.h", "demo.h", "../addon/addon_host.h", "../pcm/pcm_convert.h")
    for name in os.listdir(addon.SRC):
        text = open(os.path.join(addon.SRC, name)).read()
        assert "csrc/" not in re.sub(r"//.*", "", text), name
        for inc in re.findall(r'#include "([^"]+)"', text):
            assert inc in allowed, (name, inc)
    # the sample arithmetic is pcm_convert.h's, called, not restated
    kernels = open(os.path.join(addon.SRC, "multi_kernels.hip")).read()
    assert '#include "../pcm/pcm_convert.h"' in kernels and "32767" not in kernels
    for fn in ("pcm16_to_float", "float_to_pcm16_gain", "float_to_pcm16_peak", "pcm16_peak_of"):
        assert fn in kernels, fn
    assert sorted(os.listdir(os.path.join(ROOT, "zen_amd", "addon"))) == ["addon_host.h", "hpri_pair.h", "median_select.h", "row_walk.h", "stft_args.h", "stft_host.h", "stft_kernels.h"]


def test_wav_writer_keeps_the_channels(tmp_path):
    """encode_pcm16_interleaved of zen_amd/cli/wav.h: the header of a 3-channel file and its samples, read back by wav.h's own loader"""
    src, exe = tmp_path / "w.cpp", tmp_path / "w"
    src.write_text(r"""
#include <cstdio>
#include "wav.h"
int main(int, char** argv)
{
	std::vector<int16_t> pcm = {1, -2, 3, 32767, -32768, 0, 7, 8, 9};
	zen::wav::encode_pcm16_interleaved(pcm, 3, 48000, argv[1]);
	zen::wav::AudioData fd;
	zen::wav::load(fd, argv[1]);
	printf("%d %d %zu %zu", fd.channelCount, fd.sampleRate, fd.frameSize, fd.samples.size());
	for (float v : fd.samples) printf(" %d", (int)lroundf(v * 32767.f));
	return 0;
}
""")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "zen_amd", "cli"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe), str(tmp_path / "o.wav")], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    assert out == "3 48000 6 9 1 -2 3 32767 -32768 0 7 8 9"
    raw = open(tmp_path / "o.wav", "rb").read()
    assert len(raw) == 44 + 18 and raw[22] == 3 and int.from_bytes(raw[28:32], "little") == 48000 * 6 and int.from_bytes(raw[40:44], "little") == 18


def test_demo_program_is_built_and_states_its_usage(multi_so):
    from zen_amd import multi  # noqa: F401
    from zen_amd.addon_build import multi as addon
    exe = addon.build_demo()
    assert exe.endswith(os.path.join("bin", "zen-stems"))
    for args in ([], ["--hps", "1", "2"], ["a.wav", "b.wav"]):
        r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert r.returncode == 2 and "usage: zen-stems in.wav [-o prefix] [--hps hop_h beta_h hop_p beta_p] [--soft-mask] [--sse]" in r.stderr
