"""The C++ host mirror (zen_amd/libzen/hps.cpp) and its helper threads (zen_amd/libzen/host_threads.h) without a device.  CPU tier.

tests/cpp/fake_zen_hip.cpp stands in for libzen_hip.so (a cheap, fixed function of the input; the sink contract of
include/zen_hip.h with a staging buffer that is poisoned after every call) and tests/cpp/test_hps_host.cpp drives
HPRIOffline<GPU>::process through both size paths, the prefaulter, the deferred free of the by-value clip, two threads at
once and an engine that breaks the sink contract.  Built plain (which also counts the threads left at exit: one), under the
thread sanitizer, and under ASAN+UBSAN; nothing from zen_amd/*.so is linked."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_sanitizers import SAN  # noqa: E402

BUILDS = {"plain": ["-O2"], "tsan": ["-fsanitize=thread", "-O1", "-g"], "asan_ubsan": SAN}


def test_no_thread_is_left_to_itself():
    """every helper thread of the host layer has an owner that joins it, and the vectors-first path of rounds 4-5 is gone"""
    words = ["".join(w) for w in (("detach", "()"), ("ZEN_PROCESS_", "PLAIN"))]   # (spelt so that this file does not match)
    for top in ("zen_amd", "tools", "tests"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".cpp", ".h", ".hip", ".sh", ".py")):
                    txt = open(os.path.join(d, f), errors="replace").read()
                    assert not any(w in txt for w in words), os.path.join(d, f)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_host_mirror_against_the_fake_engine(tmp_path, build):
    exe = str(tmp_path / ("test_hps_host_" + build))
    zdir = os.path.join(ROOT, "zen_amd")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-pthread"] + BUILDS[build] +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(zdir, "libzen"),
                           os.path.join(ROOT, "tests", "cpp", "test_hps_host.cpp"),
                           os.path.join(ROOT, "tests", "cpp", "fake_zen_hip.cpp"),
                           os.path.join(zdir, "libzen", "hps.cpp"), "-o", exe])
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "passed" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    for word in ("ThreadSanitizer", "AddressSanitizer", "runtime error"):
        assert word not in r.stderr, r.stderr[-3000:]
