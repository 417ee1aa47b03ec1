"""CPU test of the run kernel's first analysis pass (zen_amd/blockrun/blockrun_first_pass.h): the header compiled as plain
C++ (tests/cpp/test_blockrun_first_pass_host.cpp, behind tests/cpp/host_shim) and run against the generic
butterfly<16, false, true, true, .> of zen_amd/csrc/fft_dev.h with the table the engine builds (make_twiddles of
libzen_hip.so): 2^20 random inputs of each main kind and the special ones, on bits (+0 == -0).  The program also asserts
the table symmetry the conjugate shortcut relies on: the shipped case is "holds", and the fallback is checked on the same
table and on a perturbed one.

The host compiler is the one hipcc drives (the header's packed forms use clang's vector extensions), called as plain C++:
no device code, no GPU.  A second build of the same stand-alone program runs under ASan + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_blockrun_first_pass_host.cpp")
LIBDIR = os.path.join(ROOT, "zen_amd")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(os.path.join(LIBDIR, "libzen_hip.so")):
        from zen_amd import build
        build.build()


def compile_host(exe, extra):
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-ffp-contract=off", "-Wall"] + extra
                          + ["-I", os.path.join(ROOT, "tests", "cpp", "host_shim"), SRC, "-o", exe,
                             "-L", LIBDIR, "-lzen_hip", "-Wl,-rpath," + LIBDIR])


def run(exe, n):
    r = subprocess.run([exe, str(n)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_first_pass_equals_generic_butterfly_on_bits(tmp_path):
    exe = str(tmp_path / "first_pass_host")
    compile_host(exe, ["-O2"])
    out = run(exe, 1 << 20)
    assert "table symmetry of the engine's 4096-point table: holds" in out   # the shipped case: SYM
    assert ", 0 mismatches," in out


def test_first_pass_host_program_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "first_pass_host_san")
    compile_host(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    out = run(exe, 1 << 14)
    assert ", 0 mismatches," in out
