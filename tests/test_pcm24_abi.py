"""CPU-side checks of the sample-format calls of zen_amd/pcm/zen_hip_pcm.h: the five names are declared, exported and bound,
every refusal -- unknown formats, bad channel counts, null pointers, buffers that overlap in their own format's bytes --
comes with ZEN_HIP_E_BAD_ARG and a message before a device is touched, and pack24 / unpack24 are each other's inverse."""
import ctypes as C
import functools
import os
import re
import subprocess
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "zen_amd", "pcm", "zen_hip_pcm.h")
NEW = ("zen_hip_pcm_sample_bytes", "zen_hip_pcm_unpack", "zen_hip_pcm_pack", "zen_hip_pcm_hpr_process_host_fmt",
       "zen_hip_pcm_hpri_process_fmt")
BAD_ARG = 2
HANDLE = 0x1000          # never dereferenced: every call below is refused before the engine is asked anything


@pytest.fixture(scope="module")
def L():
    from zen_amd import pcm
    from zen_amd.addon_build import pcm as addon
    if not os.path.exists(addon.OUT):
        addon.build()
    return pcm.load()


def on_a_thread_of_its_own(test):
    """the library's message is per thread and stays until the next failure: calls that are refused run on a thread that ends
    with the test, so the suite's own thread still finds the message empty (tests/test_pcm_abi.py looks)"""
    @functools.wraps(test)
    def run(*args, **kw):
        box = []

        def body():
            try:
                test(*args, **kw)
            except BaseException as e:      # noqa: B902 -- handed to the test's thread below
                box.append(e)
        t = threading.Thread(target=body)
        t.start()
        t.join()
        if box:
            raise box[0]
    return run


def refused(L, rc, *words):
    msg = L.zen_hip_pcm_last_error().decode()
    assert rc == BAD_ARG and all(w in msg for w in words), (rc, msg)


def test_the_five_names_are_declared_exported_and_bound(L):
    from zen_amd import pcm
    from zen_amd.addon_build import pcm as addon
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(zen_hip_pcm_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", addon.OUT], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    bound = {s[0] for s in pcm.SYMBOLS}
    for n in NEW:
        assert n in declared and n in exported and n in bound and hasattr(L, n), n
    assert "ZEN_HIP_PCM_I16 = 0, ZEN_HIP_PCM_I24 = 1" in hdr and (pcm.I16, pcm.I24) == (0, 1)
    # the four int16 entry points stay, with their signatures
    for n in ("zen_hip_pcm_to_float(const int16_t* src_dev", "zen_hip_pcm_from_float(const float* src_dev",
              "zen_hip_pcm_hpr_process_host(zen_hip_hpr_t h, const int16_t* in_host", "zen_hip_pcm_hpri_process(zen_hip_hpri_t h, const int16_t* audio_host"):
        assert n in hdr, n


def test_sample_bytes(L):
    assert [L.zen_hip_pcm_sample_bytes(f) for f in (0, 1, 2, 3, -1, 1 << 20)] == [2, 3, 0, 0, 0, 0]


@on_a_thread_of_its_own
def test_kernel_calls_refuse_before_a_device_is_touched(L):
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    for fmt in (2, -1, 77):
        refused(L, L.zen_hip_pcm_unpack(fmt, p, 1, 8, p, None), "pcm_unpack", "format", "(got %d)" % fmt)
        refused(L, L.zen_hip_pcm_pack(fmt, p, 8, 1, 1.0, None, p, None), "pcm_pack", "format", "(got %d)" % fmt)
    for fmt in (0, 1):
        for ch in (0, 3):
            refused(L, L.zen_hip_pcm_unpack(fmt, p, ch, 8, p, None), "pcm_unpack", "channels", "(got %d)" % ch)
        refused(L, L.zen_hip_pcm_unpack(fmt, None, 1, 8, p, None), "pcm_unpack", "null")
        refused(L, L.zen_hip_pcm_unpack(fmt, p, 1, 8, None, None), "pcm_unpack", "null")
        refused(L, L.zen_hip_pcm_unpack(fmt, p, 1, 8, p + 2, None), "pcm_unpack", "alignment")     # the float side
        refused(L, L.zen_hip_pcm_pack(fmt, p, 8, 5, 1.0, None, p, None), "pcm_pack", "mode", "(got 5)")
        refused(L, L.zen_hip_pcm_pack(fmt, None, 8, 1, 1.0, None, p, None), "pcm_pack", "null")
        refused(L, L.zen_hip_pcm_pack(fmt, p, 8, 0, 1.0, None, p, None), "pcm_pack", "null")         # PEAK without minmax
        refused(L, L.zen_hip_pcm_pack(fmt, p + 1, 8, 1, 1.0, None, p, None), "pcm_pack", "alignment")
    # an odd packed address is refused for I16 alone (for I24 it is served: tests/test_gpu_pcm24.py)
    refused(L, L.zen_hip_pcm_unpack(0, p + 1, 1, 8, p, None), "alignment")
    refused(L, L.zen_hip_pcm_pack(0, p, 8, 1, 1.0, None, p + 1, None), "alignment")
    # n == 0 is nothing to do, in any valid format
    assert L.zen_hip_pcm_unpack(1, None, 1, 0, None, None) == 0 and L.zen_hip_pcm_pack(1, None, 0, 1, 1.0, None, None, None) == 0
    # the int16 calls keep their words
    assert L.zen_hip_pcm_to_float(None, 3, 8, None, None) == BAD_ARG
    assert L.zen_hip_pcm_last_error() == b"pcm_to_float: channels must be 1 or 2 (got 3)"
    assert L.zen_hip_pcm_from_float(p, 8, 7, 1.0, None, p, None) == BAD_ARG
    assert L.zen_hip_pcm_last_error() == b"pcm_from_float: mode must be ZEN_HIP_PCM_PEAK or ZEN_HIP_PCM_GAIN (got 7)"


@pytest.mark.parametrize("call", ("zen_hip_pcm_hpr_process_host_fmt", "zen_hip_pcm_hpri_process_fmt"))
@on_a_thread_of_its_own
def test_host_calls_refuse_formats_channels_and_nulls(L, call):
    f = getattr(L, call)
    who = call[len("zen_hip_"):]
    buf = (C.c_char * 4096)()
    p = C.addressof(buf)
    for in_fmt, out_fmt, which, bad in ((2, 0, "input", 2), (0, 2, "output", 2), (-3, 1, "input", -3), (1, 99, "output", 99)):
        refused(L, f(HANDLE, in_fmt, p, 1, 4, out_fmt, p + 2048, None, None, 1, 1.0, None, 0), who, which, "format", "(got %d)" % bad)
    for ch in (0, 3, -1):
        refused(L, f(HANDLE, 1, p, ch, 4, 1, p + 2048, None, None, 1, 1.0, None, 0), who, "channels", "(got %d)" % ch)
    refused(L, f(HANDLE, 1, p, 1, 4, 1, p + 2048, None, None, 9, 1.0, None, 0), who, "mode", "(got 9)")
    refused(L, f(None, 1, p, 1, 4, 1, p + 2048, None, None, 1, 1.0, None, 0), who, "null")
    if call.endswith("host_fmt"):        # (the offline call's: test_overlap_is_measured_in_the_formats_bytes)
        refused(L, f(HANDLE, 1, None, 1, 4, 1, p + 2048, None, None, 1, 1.0, None, 0), who, "null")


@pytest.mark.parametrize("fmt, sb", ((0, 2), (1, 3)), ids=("i16", "i24"))
@on_a_thread_of_its_own
def test_overlap_is_measured_in_the_formats_bytes(L, fmt, sb):
    """two outputs of n samples sb * n - 1 bytes apart overlap, sb * n apart they do not.  The offline call looks at the
    buffers before it looks for the audio and before it asks its engine anything: with no audio the call that passes the
    overlap check is refused one line later, for that, and the handle is never touched."""
    n = 1000
    buf = (C.c_char * (8 * n))()
    p = C.addressof(buf)
    f = L.zen_hip_pcm_hpri_process_fmt
    refused(L, f(HANDLE, 1, None, 1, n, fmt, p, p + sb * n - 1, None, 0, 1.0, None, 0), "pcm_hpri_process_fmt", "overlap")
    refused(L, f(HANDLE, 1, None, 1, n, fmt, p, p + sb * n, None, 0, 1.0, None, 0), "pcm_hpri_process_fmt", "null argument")
    refused(L, f(HANDLE, 1, None, 1, n, fmt, p, None, p + sb * n - 1, 0, 1.0, None, 0), "overlap")        # harmonic / residual
    refused(L, f(HANDLE, 1, None, 1, n, fmt, p + sb * n, p, p + 2 * sb * n, 0, 1.0, None, 0), "null argument")
    # the input counts in ITS format's bytes and its channels: 2 * sb * n bytes of stereo input
    refused(L, f(HANDLE, fmt, p, 2, n, 1 - fmt, p + 2 * sb * n - 1, None, None, 0, 1.0, None, 0), "overlap")


def test_header_still_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "zen_hip_pcm.h"\n'
                   "int main(void){return ZEN_HIP_PCM_I16 + ZEN_HIP_PCM_I24 + ZEN_HIP_PCM_PEAK + ZEN_HIP_OK\n"
                   " + (int)(sizeof(&zen_hip_pcm_unpack) + sizeof(&zen_hip_pcm_pack) + sizeof(&zen_hip_pcm_sample_bytes)\n"
                   " + sizeof(&zen_hip_pcm_hpr_process_host_fmt) + sizeof(&zen_hip_pcm_hpri_process_fmt)) * 0;}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.dirname(HDR), "-c", str(src), "-o", str(tmp_path / "t.o")])
    conv = tmp_path / "c.c"
    conv.write_text('#include "pcm_convert.h"\nint main(void){unsigned char b[3]; pcm24_store(b, float_to_pcm24(pcm24_to_float(5)));\n'
                    "return pcm24_load(b) - 5 + float_to_pcm16(pcm16_to_float(0)) + pcm_sample_bytes(ZEN_PCM_FMT_I24) - 3;}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-ffp-contract=off", "-I", os.path.dirname(HDR), str(conv),
                           "-o", str(tmp_path / "c"), "-lm"])
    assert subprocess.call([str(tmp_path / "c")]) == 0


def test_pack24_and_unpack24_round_trip():
    from zen_amd import pcm
    rng = np.random.default_rng(24)
    v = rng.integers(-8388608, 8388608, 100003).astype(np.int32)
    v[:6] = [0, 1, -1, 8388607, -8388608, 0x123456]
    b = pcm.pack24(v)
    assert b.dtype == np.uint8 and b.size == 3 * v.size and b.flags["C_CONTIGUOUS"]
    assert b[:18].tolist() == [0, 0, 0, 1, 0, 0, 255, 255, 255, 255, 255, 127, 0, 0, 128, 0x56, 0x34, 0x12]
    back = pcm.unpack24(b)
    assert back.dtype == np.int32 and np.array_equal(back, v)
    assert np.array_equal(pcm.pack24(pcm.unpack24(b)), b)
    assert pcm.pack24(np.zeros(0, np.int32)).size == 0 and pcm.unpack24(np.zeros(0, np.uint8)).size == 0
