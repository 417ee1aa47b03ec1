"""CPU-side checks of what the add-on libraries (zen_amd/pcm, ragged, live, pitch) share: the headers of zen_amd/addon stay
private to each library (its own error message, nothing of theirs exported), the sources see the public headers and those
only, and the one builder (zen_amd/addon_build.py) recompiles what is stale and nothing else."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pcm", "ragged", "live", "pitch")


@pytest.fixture(scope="module")
def addons():
    """the four libraries, built where absent"""
    from zen_amd import addon_build
    assert tuple(addon_build.LIBRARIES)[:4] == NAMES
    four = {n: addon_build.LIBRARIES[n] for n in NAMES}
    for a in four.values():
        if not os.path.exists(a.OUT):
            a.build()
    return four


# ---- one error message per library ------------------------------------------------------------------------------------------
CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import importlib
order = sys.argv[2].split(",")
L = {n: importlib.import_module("zen_amd." + n).load() for n in order}
h = ctypes.c_void_p()
fail = {
    "pcm": lambda l: l.zen_hip_pcm_to_float(None, 3, 8, None, None),
    "ragged": lambda l: l.zen_hip_ragged_create(44100.0, 1024, 256, 2.0, 2.0, 0, 0, ctypes.byref(h)),
    "live": lambda l: l.zen_hip_live_create(44100.0, 1024, 768, 2.0, 2.0, 0, 1, 0, ctypes.byref(h)),
    "pitch": lambda l: l.zen_hip_pitch_create(44100.0, 48, 1, 0, ctypes.byref(h)),
}
codes = {n: fail[n](L[n]) for n in order}
msgs = {n: getattr(L[n], "zen_hip_%s_last_error" % n)().decode() for n in order}
print(json.dumps({"codes": codes, "msgs": msgs}))
"""
MESSAGES = {"pcm": (2, "pcm_to_float: channels must be 1 or 2 (got 3)"),
            "ragged": (2, "ragged_create: null handle or zero clips"),
            "live": (3, "hop_h and hop_p should be evenly divisible"),
            "pitch": (2, "pitch_create: chunk length 48 is not a power of two in 32..16384")}


@pytest.mark.parametrize("order", (NAMES, NAMES[::-1]), ids=("pcm_first", "pitch_first"))
def test_every_library_keeps_its_own_error_message(addons, order):
    """all four in one process, each refused a call before the messages are read: whichever was loaded first (a fresh process
    per order: the load order decides which definition a shared symbol would resolve to), each holds its own"""
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, ",".join(order)], stdout=subprocess.PIPE, universal_newlines=True, check=True)
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for n in NAMES:
        assert (got["codes"][n], got["msgs"][n]) == MESSAGES[n], n


# ---- nothing shared leaks out -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_library_exports_its_header_and_nothing_of_the_shared_code(addons, name):
    a = addons[name]
    out = subprocess.run(["nm", "-D", "--defined-only", a.OUT], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    syms = [line.split()[-1] for line in out.splitlines() if line.strip()]
    assert not [s for s in syms if "zen_addon" in s], "zen_amd/addon is header-only with internal linkage"
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(a.SRC, "zen_hip_%s.h" % name)).read(), flags=re.S)
    declared = set(re.findall(r"\b(zen_hip_%s_[a-z0-9_]+)\s*\(" % name, hdr))
    assert declared and {s for s in syms if s.startswith("zen_hip_")} == declared


# ---- the build ----------------------------------------------------------------------------------------------------------------
ALLOWED = {"pcm": ("zen_hip.h", "zen_hip_pcm.h", "pcm_convert.h", "pcm_kernels.h", "../addon/addon_host.h", "../csrc/host_pipe.h"),
           "ragged": ("zen_hip.h", "zen_hip_ragged.h", "ragged_kernels.h", "../addon/hpri_pair.h", "../addon/row_walk.h"),
           "live": ("zen_hip.h", "zen_hip_live.h", "live_kernels.h", "../addon/hpri_pair.h", "../addon/row_walk.h"),
           "addon": ("zen_hip.h", "addon_host.h", "stft_args.h")}


@pytest.mark.parametrize("name", sorted(ALLOWED))
def test_sources_see_the_public_headers_only(name):
    """as tests/test_pitch_abi.py has it for pitch: nothing of the engines' sources; pcm's one declared exception is
    csrc/host_pipe.h (shared with the float pipelines)"""
    src = os.path.join(ROOT, "zen_amd", name)
    for f in os.listdir(src):
        text = re.sub(r"//.*", "", open(os.path.join(src, f)).read())
        if name == "pcm":
            text = text.replace('#include "../csrc/host_pipe.h"', "", 1)
        assert "csrc/" not in text, f
        for inc in re.findall(r'#include "([^"]+)"', open(os.path.join(src, f)).read()):
            assert inc in ALLOWED[name], (f, inc)


def test_one_list_of_flags_for_all(addons):
    from zen_amd import addon_build
    assert all(a.FLAGS is addon_build.FLAGS for a in addons.values())


def test_former_builder_names_are_the_table_entries():
    """`from zen_amd import pcm_build` of earlier callers: the same handle, with what they used of the module"""
    import zen_amd
    from zen_amd import addon_build
    for n in NAMES:
        a = getattr(zen_amd, n + "_build")
        assert a is addon_build.LIBRARIES[n] and a.OUT.endswith("libzen_hip_%s.so" % n) and os.path.isdir(a.SRC) and callable(a.build)
    assert zen_amd.pitch_build.DEMO.endswith(os.path.join("bin", "pitch-track")) and callable(zen_amd.pitch_build.build_demo)
    assert all(getattr(zen_amd, n + "_build").DEMO is None for n in ("pcm", "ragged", "live"))


EVERY_NAME = ("pcm", "ragged", "live", "pitch", "blockrun", "beat", "multi", "repet", "cqt", "repsim", "nmf", "tsm", "resample")


def test_one_table_holds_every_library():
    """the thirteen in the order they are built, in the module's only dictionary of Addons, one entry per library directory on
    disk; every entry is the module-level object of its name and shares the one list of flags"""
    from zen_amd import addon_build
    tables = [k for k, v in vars(addon_build).items() if isinstance(v, dict) and v and all(isinstance(a, addon_build.Addon) for a in v.values())]
    assert tables == ["LIBRARIES"]
    assert tuple(addon_build.LIBRARIES) == EVERY_NAME
    for n, a in addon_build.LIBRARIES.items():
        assert a is getattr(addon_build, n) and a.name == n and a.FLAGS is addon_build.FLAGS
    pkg = os.path.join(ROOT, "zen_amd")
    on_disk = {d for d in os.listdir(pkg) if os.path.exists(os.path.join(pkg, d, "zen_hip_%s.h" % d))}
    assert on_disk == set(EVERY_NAME)
    assert {n for n, a in addon_build.LIBRARIES.items() if a.DEMO is None} == {"pcm", "ragged", "live", "blockrun"}


def mtimes(addons):
    return {n: [os.path.getmtime(p) for p in a.objects() + [a.OUT]] for n, a in addons.items()}


def test_builder_recompiles_what_is_stale_and_nothing_else(addons):
    """a library and its objects older than the shared headers: exactly those are made again; a build right after compiles nothing"""
    for a in addons.values():
        a.build()                       # (whatever state the tree was in: up to date now)
    before = mtimes(addons)
    assert before == mtimes(addons) and all(len(v) == 3 for v in before.values())
    for a in addons.values():
        a.build()
    assert mtimes(addons) == before, "a second build right after the first compiled or linked something"
    stale = addons["ragged"]
    hdrs = [os.path.join(ROOT, "zen_amd", "addon", f) for f in os.listdir(os.path.join(ROOT, "zen_amd", "addon"))]
    assert len(hdrs) == 7
    old = min(os.path.getmtime(p) for p in hdrs) - 3600
    for p in stale.objects() + [stale.OUT]:
        os.utime(p, (old, old))
    for a in addons.values():
        a.build()
    after = mtimes(addons)
    for n in NAMES:
        if n == "ragged":
            assert all(t >= b for t, b in zip(after[n], before[n])) and all(t > old for t in after[n]), "the stale library was not rebuilt"
        else:
            assert after[n] == before[n], "%s was up to date and was rebuilt" % n
    for a in addons.values():
        a.build()
    assert mtimes(addons) == after


# ---- the calls every handle answers, refused the same way in every library ----------------------------------------------------
HANDLE_LIBRARIES = ("pitch", "beat", "live", "ragged", "repet", "cqt", "repsim", "nmf", "tsm", "resample")


@pytest.mark.parametrize("name", HANDLE_LIBRARIES)
def test_null_handles_are_refused_with_the_librarys_own_words(name):
    """set_stream, profile, profile_get and stats on a null handle, without a device: the code and the message each library
    has always given (ragged has no stats call)"""
    import importlib
    L = importlib.import_module("zen_amd." + name).load()
    err = getattr(L, "zen_hip_%s_last_error" % name)
    call = lambda fn, *args: (getattr(L, "zen_hip_%s_%s" % (name, fn))(*args), err().decode())   # noqa: E731
    assert call("set_stream", None, None) == (2, "%s_set_stream: null handle" % name)
    assert call("profile", None, 1) == (2, "null handle")
    assert call("profile_get", None, None, None, None) == (2, "%s_profile_get: null argument" % name)
    if name != "ragged":
        assert call("stats", None, None) == (2, "%s_stats: null argument" % name)


# ---- the programs ---------------------------------------------------------------------------------------------------------------
PROGRAMS = {"pitch": ("pitch-track", []), "beat": ("beat-track", []), "multi": ("zen-stems", []), "repet": ("zen-repet", ["-o", "out"]),
            "cqt": ("zen-cqt", ["-o", "out"]), "repsim": ("zen-repsim", ["-o", "out"]), "nmf": ("zen-nmf", ["-o", "out.znmf"]),
            "tsm": ("zen-stretch", ["-a", "1.5", "-o", "out.wav"]), "resample": ("zen-shift", ["-s", "3", "-o", "out.wav"])}


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_program_reports_a_file_it_cannot_open(name, tmp_path):
    """every program reads its recording before it touches a device: a path that does not exist ends it with status 1 and one
    line, the program's name in front of cli/wav.h's message"""
    from zen_amd import addon_build
    prog, args = PROGRAMS[name]
    exe = addon_build.LIBRARIES[name].build_demo()
    assert exe.endswith(os.path.join("bin", prog))
    missing = str(tmp_path / "absent.wav")
    argv = [exe] + (["train"] if name == "nmf" else []) + [missing] + args
    r = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, cwd=str(tmp_path))
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "%s: cannot open %s\n" % (prog, missing))
