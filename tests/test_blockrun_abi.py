"""CPU-side checks of the block-run library's boundary (zen_amd/blockrun/zen_hip_blockrun.h): the header is plain C, every
function it declares is exported by libzen_hip_blockrun.so and bound in zen_amd/lib.py, the kernel file is built with the
arithmetic contract's flags, and the partition of a call's hops into runs (blockrun_partition.h, plain C: compiled here
for the host) puts every hop into exactly one run, never crosses a stream and keeps the runs within one hop of each other."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "zen_amd", "blockrun")
HDR = os.path.join(SRC, "zen_hip_blockrun.h")


@pytest.fixture(scope="module")
def blockrun_so():
    from zen_amd.addon_build import blockrun as addon
    if not os.path.exists(addon.OUT):
        addon.build()
    return addon.OUT


def declared_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zen_hip_blockrun_[a-z0-9_]+)\s*\(", hdr)))


def test_header_symbols_are_bound_and_exported(blockrun_so):
    from zen_amd import lib
    L = ctypes.CDLL(blockrun_so)
    names = declared_symbols()
    assert names == ["zen_hip_blockrun_process", "zen_hip_blockrun_set", "zen_hip_blockrun_stats"]
    for n in names:
        assert hasattr(L, n), "libzen_hip_blockrun.so does not export %s" % n
    assert set(names) == {s[0] for s in lib.BLOCKRUN_SYMBOLS}
    assert dict((s[0], s[2]) for s in lib.SYMBOLS)["zen_hip_hpr_process"] == lib.BLOCKRUN_SYMBOLS[0][2], "same contract, same signature"
    out = subprocess.run(["nm", "-D", "--defined-only", blockrun_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {s for s in exported if s.startswith("zen_hip_")} == set(names)


def test_library_loads_without_gpu_and_checks_settings(blockrun_so):
    from zen_amd import lib
    L = lib.load_blockrun()
    assert L, "libzen_hip_blockrun.so is built and must load"
    assert L.zen_hip_blockrun_set(b"run_len", 5) == 0 and L.zen_hip_blockrun_set(b"run_len", 0) == 0
    assert L.zen_hip_blockrun_set(b"nonsense", 1) == 2 and b"unknown key" in lib.load().zen_hip_last_error()
    assert L.zen_hip_blockrun_set(b"off", -1) == 2 and L.zen_hip_blockrun_set(None, 1) == 2
    # a null handle is the base library's to refuse: forwarded, counted
    before = lib.blockrun_stats()
    assert L.zen_hip_blockrun_process(None, None, 4, 4096, None, None, None, 4096) == 2
    after = lib.blockrun_stats()
    assert after == (before[0], before[1] + 1)


def test_library_finds_the_engine_library_beside_itself(blockrun_so):
    out = subprocess.run(["readelf", "-d", blockrun_so], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    assert "libzen_hip.so" in out and "$ORIGIN" in out


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "zen_hip_blockrun.h"\n#include "blockrun_partition.h"\n'
                   'int main(void){zen_blockrun_part p = zen_blockrun_partition(1, 8, 3, 0); return p.base_len - p.base_len + ZEN_HIP_OK;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I", SRC,
                           "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_build_keeps_the_arithmetic_contract_and_is_registered():
    from zen_amd import addon_build
    a = addon_build.blockrun
    assert addon_build.LIBRARIES["blockrun"] is a and a.DEMO is None and a.OUT.endswith("libzen_hip_blockrun.so")
    flags = a.FLAGS + a.FILE_FLAGS["blockrun_kernel.hip"]
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags
    assert not any("fast-math" in f and f != "-fno-fast-math" for f in flags)
    from zen_amd import build as zbuild
    for f in zbuild.FILE_FLAGS["rt_fused.hip"]:
        assert f in a.FILE_FLAGS["blockrun_kernel.hip"], "the scheduler flags of rt_fused.hip"
    # every csrc header its sources include makes its objects stale
    deps = {os.path.relpath(d, os.path.join(ROOT, "zen_amd")) for d in a.extra_deps}
    for name in os.listdir(SRC):
        for inc in re.findall(r'#include "\.\./(csrc/[^"]+)"', open(os.path.join(SRC, name)).read()):
            assert inc in deps, (name, inc)
    assert all(os.path.exists(d) for d in a.extra_deps)


# ---- the partition ------------------------------------------------------------------------------------------------------------
SHIM = r"""
#include "blockrun_partition.h"
int part(int streams, int hops, int slots, int run_len, int* rps, int* base_len, int* n_long)
{
	zen_blockrun_part p = zen_blockrun_partition(streams, hops, slots, run_len);
	*rps = p.runs_per_stream; *base_len = p.base_len; *n_long = p.n_long;
	return streams * p.runs_per_stream;
}
void run_of(int streams, int hops, int slots, int run_len, int run, int* stream, int* first, int* len)
{
	zen_blockrun_part p = zen_blockrun_partition(streams, hops, slots, run_len);
	zen_blockrun_run(&p, run, stream, first, len);
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("blockrun_shim")
    (d / "shim.c").write_text(SHIM)
    so = str(d / "shim.so")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-O1", "-shared", "-fPIC", "-I", SRC, str(d / "shim.c"), "-o", so])
    return ctypes.CDLL(so)


def runs_of(shim, streams, hops, slots, run_len):
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    n = shim.part(streams, hops, slots, run_len, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    out = []
    for r in range(n):
        shim.run_of(streams, hops, slots, run_len, r, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        out.append((a.value, b.value, c.value))
    return out


CASES = [(1, 25840, 768, 0), (1, 1, 768, 0), (1, 2, 768, 0), (3, 37, 768, 0), (3, 37, 768, 1), (3, 37, 768, 2), (3, 37, 768, 5),
         (3, 37, 768, 37), (3, 37, 768, 64), (1, 37, 6, 0), (7, 1000, 24, 0), (5, 100003, 768, 0), (2, 500, 768, 0), (1, 769, 768, 0),
         (16, 3000, 768, 0), (1000, 3, 768, 0), (1, 25840, 768, 8), (4, 6460, 912, 0)]


@pytest.mark.parametrize("streams,hops,slots,run_len", CASES)
def test_partition_covers_every_hop_once_within_its_stream(shim, streams, hops, slots, run_len):
    runs = runs_of(shim, streams, hops, slots, run_len)
    assert len(runs) % streams == 0 and 1 <= len(runs) // streams <= hops           # (hops < slots: never more runs than hops)
    nxt = {s: 0 for s in range(streams)}
    for s, first, n in runs:                                                          # in launch order: consecutive within a stream
        assert 0 <= s < streams and n >= 1 and first == nxt[s] and first + n <= hops  # no gap, no overlap, never across a stream
        nxt[s] = first + n
    assert all(v == hops for v in nxt.values())                                       # every hop in exactly one run
    lens = [n for _, _, n in runs]
    assert max(lens) - min(lens) <= 1
    if run_len:
        assert max(lens) <= run_len
        assert len(runs) // streams == -(-hops // run_len)


def test_partition_of_the_headline_call(shim):
    """25 840 hops on 3 x 256 slots: four runs per slot, 8 or 9 hops each -- at most one hop of imbalance in 33"""
    runs = runs_of(shim, 1, 25840, 768, 0)
    assert len(runs) == 4 * 768 and {n for _, _, n in runs} == {8, 9}
