"""Builds the add-on libraries for gfx950 with hipcc: zen_amd/libzen_hip_<name>.so from zen_amd/<name>/, each a library of
its own on top of libzen_hip.so's C ABI (blockrun: on top of the engine's state as well), and the demo programs zen_amd/bin/pitch-track, zen_amd/bin/beat-track,
zen_amd/bin/zen-stems, zen_amd/bin/zen-repet, zen_amd/bin/zen-cqt, zen_amd/bin/zen-repsim, zen_amd/bin/zen-nmf, zen_amd/bin/zen-stretch and zen_amd/bin/zen-shift (plain g++: they reach the GPU through C ABIs only).

    python zen_amd/addon_build.py [name ...] [--force]         # no name: all of them

Every library links against libzen_hip.so (zen_amd/build.py builds that one first) and finds it beside itself ($ORIGIN).
-ffp-contract=off and no fast-math flag, for all of them: every float operation of their kernels is a single IEEE operation,
one rounding each -- the contract of pcm/pcm_convert.h (the division, the products and the rounding are those of the host
code in zen_amd/cli/wav.h), the one add P1 + R1 of ragged and live, DESIGN.md section 13 for pitch, section 15 for beat, section 17 for repet, section 18 for cqt (whose host tables are part of it), section 19 for repsim, section 20 for nmf, section 21 for tsm and section 22 for resample (whose host tables are part of it).
"""
import glob
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BASE = os.path.join(HERE, "libzen_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall",
         "-I", os.path.join(ROOT, "include")]


class Addon:
    """One add-on: zen_amd/<name>/<sources> -> zen_amd/build_<name>/*.o -> zen_amd/libzen_hip_<name>.so.  `extra_deps`: files
    outside its directory whose change makes its objects stale; `build_demo`: a step behind the link."""

    def __init__(self, name, sources, extra_deps=(), build_demo=None, title=None, file_flags=None):
        self.name, self.SOURCES, self.build_demo, self.title = name, list(sources), build_demo, title or name
        self.SRC = os.path.join(HERE, name)
        self.OUT = os.path.join(HERE, "libzen_hip_%s.so" % name)
        self.OBJDIR = os.path.join(HERE, "build_" + name)
        self.FLAGS = FLAGS
        self.FILE_FLAGS = dict(file_flags or {})   # source -> flags of its own behind FLAGS (as build.py's FILE_FLAGS)
        self.extra_deps = [os.path.join(HERE, *d.split("/")) for d in extra_deps]

    def deps(self):
        hdrs = [os.path.join(self.SRC, f) for f in os.listdir(self.SRC) if f.endswith(".h")]
        hdrs += glob.glob(os.path.join(HERE, "addon", "*.h")) + self.extra_deps
        hdrs.append(os.path.join(ROOT, "include", "zen_hip.h"))
        hdrs.append(os.path.abspath(__file__))   # the flags live here
        return hdrs

    def objects(self):
        return [os.path.join(self.OBJDIR, s.replace(".hip", ".o")) for s in self.SOURCES]

    def _compile(self, src):
        obj = os.path.join(self.OBJDIR, src.replace(".hip", ".o"))
        srcp = os.path.join(self.SRC, src)
        newest = max(os.path.getmtime(p) for p in [srcp] + self.deps())
        if os.path.exists(obj) and os.path.getmtime(obj) >= newest:
            return obj, False
        subprocess.check_call([HIPCC] + self.FLAGS + self.FILE_FLAGS.get(src, []) + ["-c", srcp, "-o", obj])
        return obj, True

    def build(self, force=False, verbose=False):
        """Compiles the stale objects in parallel; links where an object was compiled or libzen_hip.so is newer."""
        if not os.path.exists(BASE):
            raise RuntimeError("%s not built: zen_amd/build.py first (the %s library links against it)" % (BASE, self.title))
        os.makedirs(self.OBJDIR, exist_ok=True)
        if force:
            for f in os.listdir(self.OBJDIR):
                os.remove(os.path.join(self.OBJDIR, f))
        with ThreadPoolExecutor(max_workers=len(self.SOURCES)) as ex:
            res = list(ex.map(self._compile, self.SOURCES))
        if any(r[1] for r in res) or not os.path.exists(self.OUT) or os.path.getmtime(self.OUT) < os.path.getmtime(BASE):
            subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", self.OUT] + [r[0] for r in res]
                                  + ["-L", HERE, "-lzen_hip", "-Wl,-rpath,$ORIGIN"])
            if verbose:
                print("built", self.OUT)
        if self.build_demo:
            self.build_demo(verbose)
        return self.OUT


def _build_demo(name, source, exe, verbose, extra=()):
    """zen_amd/bin/<exe> from zen_amd/<name>/<source>, against libzen_hip_<name>.so and libzen_hip.so; made again where the
    source, the library's header, cli/wav.h or the library is newer.  `extra`: further add-ons whose libraries the program
    links and whose headers it sees (they are built first where they are absent)."""
    src, out = os.path.join(HERE, name), os.path.join(HERE, "libzen_hip_%s.so" % name)
    srcs = [os.path.join(src, source), os.path.join(src, "zen_hip_%s.h" % name), os.path.join(HERE, "cli", "wav.h"), out]
    more, libs = [], []
    for e in extra:
        if not os.path.exists(EVERY_LIBRARY[e].OUT):
            EVERY_LIBRARY[e].build(verbose=verbose)
        srcs += [os.path.join(HERE, e, "zen_hip_%s.h" % e), EVERY_LIBRARY[e].OUT]
        more += ["-I", os.path.join(HERE, e)]
        libs.append("-lzen_hip_" + e)
    if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(p) for p in srcs):
        return exe
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           "-I", src, "-I", os.path.join(HERE, "cli")] + more + [srcs[0], "-o", exe, "-L", HERE, "-lzen_hip_" + name] + libs
                          + ["-lzen_hip", "-Wl,-rpath,$ORIGIN/.."])
    if verbose:
        print("built", exe)
    return exe


DEMO = os.path.join(HERE, "bin", "pitch-track")
BEAT_DEMO = os.path.join(HERE, "bin", "beat-track")
STEMS_DEMO = os.path.join(HERE, "bin", "zen-stems")
REPET_DEMO = os.path.join(HERE, "bin", "zen-repet")
CQT_DEMO = os.path.join(HERE, "bin", "zen-cqt")
REPSIM_DEMO = os.path.join(HERE, "bin", "zen-repsim")
NMF_DEMO = os.path.join(HERE, "bin", "zen-nmf")
STRETCH_DEMO = os.path.join(HERE, "bin", "zen-stretch")
SHIFT_DEMO = os.path.join(HERE, "bin", "zen-shift")


def build_demo(verbose=False):
    return _build_demo("pitch", "pitch_track.cpp", DEMO, verbose)


def build_beat_demo(verbose=False):
    return _build_demo("beat", "beat_track.cpp", BEAT_DEMO, verbose)


def build_stems_demo(verbose=False):
    return _build_demo("multi", "multi_stems.cpp", STEMS_DEMO, verbose)


def build_repet_demo(verbose=False):
    return _build_demo("repet", "repet_main.cpp", REPET_DEMO, verbose)


def build_cqt_demo(verbose=False):
    return _build_demo("cqt", "cqt_main.cpp", CQT_DEMO, verbose)


def build_repsim_demo(verbose=False):
    return _build_demo("repsim", "repsim_main.cpp", REPSIM_DEMO, verbose)


def build_nmf_demo(verbose=False):
    return _build_demo("nmf", "nmf_main.cpp", NMF_DEMO, verbose)


def build_stretch_demo(verbose=False):
    return _build_demo("tsm", "tsm_main.cpp", STRETCH_DEMO, verbose)


def build_shift_demo(verbose=False):
    return _build_demo("resample", "resample_main.cpp", SHIFT_DEMO, verbose, extra=("tsm",))


pcm = Addon("pcm", ["pcm_kernels.hip", "pcm_pipe.hip"], extra_deps=["csrc/host_pipe.h"], title="PCM")
ragged = Addon("ragged", ["ragged_kernels.hip", "ragged.hip"])
live = Addon("live", ["live_kernels.hip", "live.hip"])
pitch = Addon("pitch", ["pitch_kernels.hip", "pitch.hip"], build_demo=build_demo)
ADDONS = {a.name: a for a in (pcm, ragged, live, pitch)}   # on the C ABI alone
# blockrun shares the engine's state with libzen_hip.so at compile time (csrc/hpr_engine.h) and compiles the fused kernel's
# headers into a kernel of its own: the csrc headers it includes make its objects stale, and its kernel file gets the
# scheduler flags build.py gives rt_fused.hip, plus fft_dev.h's LDS-only barrier between the passes of a transform (a run
# keeps loads and stores in flight across them) and its folded image addresses (with them the run kernel fits its 168
# registers without scratch; without, it spills 5).
blockrun = Addon("blockrun", ["blockrun_kernel.hip", "blockrun.hip"],
                 extra_deps=["csrc/hpr_engine.h", "csrc/rt_fused.h", "csrc/common.h", "csrc/bounds.h", "csrc/memguard.h", "csrc/masks.h",
                             "csrc/fft_dev.h", "csrc/median47_core.h", "csrc/median_net.h"],
                 file_flags={"blockrun_kernel.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp", "-mllvm", "-amdgpu-use-amdgpu-trackers=1",
                                                     "-DZEN_FFT_LDS_BARRIER", "-DZEN_FFT_FOLD_ADDR", "-Wno-unused-function"]})
ENGINE_ADDONS = {blockrun.name: blockrun}                  # on the engine's own state
# beat came after the four of ADDONS and is, like them, on the C ABI alone; beat_track.cpp is the demo's, not the library's
beat = Addon("beat", ["beat_kernels.hip", "beat.hip"], build_demo=build_beat_demo)
# multi (interleaved multichannel audio through the engines' rows) shares the sample arithmetic of pcm/pcm_convert.h;
# multi_stems.cpp is the demo's, not the library's
multi = Addon("multi", ["multi_kernels.hip", "multi.hip"], extra_deps=["pcm/pcm_convert.h"], build_demo=build_stems_demo)
# repet (repeating background against foreground) is on the C ABI alone as well; repet_main.cpp is the demo's, not the library's
repet = Addon("repet", ["repet_kernels.hip", "repet.hip"], build_demo=build_repet_demo)
# cqt (a sliced constant-Q transform and the separation in its domain) is on the C ABI alone too; cqt_main.cpp is the demo's
cqt = Addon("cqt", ["cqt_kernels.hip", "cqt.hip"], build_demo=build_cqt_demo)
# repsim (REPET-SIM: the repeating background found from the similarity matrix, the tree's one matrix-core kernel) is on the C
# ABI alone as well; repsim_main.cpp is the demo's
repsim = Addon("repsim", ["repsim_kernels.hip", "repsim.hip"], build_demo=build_repsim_demo)
LATER_ADDONS = {beat.name: beat, multi.name: multi, repet.name: repet, cqt.name: cqt, repsim.name: repsim}
# nmf (supervised factorisation of the magnitude spectrogram: three matrix products per iteration on the matrix cores) came
# after the five of LATER_ADDONS and is, like them, on the C ABI alone; nmf_main.cpp is the demo's
nmf = Addon("nmf", ["nmf_kernels.hip", "nmf.hip"], build_demo=build_nmf_demo)
FACTOR_ADDONS = {nmf.name: nmf}
ALL_ADDONS = {**ADDONS, **ENGINE_ADDONS, **LATER_ADDONS, **FACTOR_ADDONS}
# tsm (time-scale modification: the harmonic stem through a phase-locked vocoder, the percussive one through overlap-add) is on
# the C ABI alone as well; tsm_main.cpp is the demo's.  It has a table of its own: the eleven of ALL_ADDONS are the ones from
# before it, and EVERY_ADDON is the lookup of the loader and of the command line.
tsm = Addon("tsm", ["tsm_kernels.hip", "tsm.hip"], build_demo=build_stretch_demo)
STRETCH_ADDONS = {tsm.name: tsm}
EVERY_ADDON = {**ALL_ADDONS, **STRETCH_ADDONS}
# resample (band-limited rate conversion by a rational ratio, and with tsm in front the pitch shift) is on the C ABI alone as
# well; resample_main.cpp is the demo's, and links tsm's library too.  It has a table of its own again: EVERY_ADDON stays the
# twelve from before it, and EVERY_LIBRARY is the lookup of the loader and of the command line.
resample = Addon("resample", ["resample_kernels.hip", "resample.hip"], build_demo=build_shift_demo)
SHIFT_ADDONS = {resample.name: resample}
EVERY_LIBRARY = {**EVERY_ADDON, **SHIFT_ADDONS}


if __name__ == "__main__":
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or list(EVERY_LIBRARY)
    for n in names:
        EVERY_LIBRARY[n].build(force="--force" in sys.argv, verbose=True)
