"""CPU test of the run kernel's counted edge masks (zen_amd/blockrun/blockrun_edge_count.h): the header compiled as plain C++
(tests/cpp/test_blockrun_edge_count_host.cpp, behind tests/cpp/host_shim) and run against the selection it replaces, the
median of znet::medians<47, ...> (zen_amd/csrc/median_net.h) through hard_mask_exact (zen_amd/csrc/masks.h): all 24 edge bins
of rows built with the kernel's mirror and border rules, more than 10^6 windows over six betas (inclusive and strict
thresholds), ties, elements at the decision boundary, zeros, subnormals, FLT_MAX, +inf and NaN patterns.  No mismatch is
allowed.

The host compiler is the one hipcc drives, called as plain C++: no device code, no GPU, no library of the project.  A second
build of the same stand-alone program runs under ASan + UBSan."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_blockrun_edge_count_host.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def compile_host(exe, extra):
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-ffp-contract=off", "-Wall"] + extra
                          + ["-I", os.path.join(ROOT, "tests", "cpp", "host_shim"), SRC, "-o", exe])


def run(exe, unit):
    r = subprocess.run([exe, str(unit)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_counted_edge_masks_equal_the_selected_median_through_the_hard_mask(tmp_path):
    exe = str(tmp_path / "edge_count_host")
    compile_host(exe, ["-O2"])
    out = run(exe, 1000)
    m = re.search(r"selected median: (\d+) windows, 0 mismatches,", out)
    assert m and int(m.group(1)) >= 10 ** 6
    assert "(strict threshold)" in out and "(inclusive threshold)" in out
    assert "outputs that took both values: 24 of 24" in out


def test_edge_count_host_program_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "edge_count_host_san")
    # (no -g and not -O1: debug information for the unrolled 47-key network takes the compiler two minutes)
    compile_host(exe, ["-O2", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    out = run(exe, 200)
    assert ", 0 mismatches," in out
