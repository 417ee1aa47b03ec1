"""Builds the add-on libraries for gfx950 with hipcc: zen_amd/libzen_hip_<name>.so from zen_amd/<name>/, each a library of
its own on top of libzen_hip.so's C ABI (blockrun: on top of the engine's state as well), and the demo programs zen_amd/bin/<program>
of the libraries that have one (plain g++: they reach the GPU through C ABIs only).  LIBRARIES, at the end, is the table of them.

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
    outside its directory whose change makes its objects stale; `demo`: (source, program, further add-ons it links) of the
    program zen_amd/bin/<program>, a step behind the link -- DEMO is its path, None where the library has no program."""

    def __init__(self, name, sources, extra_deps=(), demo=None, title=None, file_flags=None):
        self.name, self.SOURCES, self.title = name, list(sources), title or name
        self.demo_source, exe, self.demo_links = demo or (None, None, ())
        self.DEMO = exe and os.path.join(HERE, "bin", exe)
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
        if self.DEMO:
            self.build_demo(verbose)
        return self.OUT

    def build_demo(self, verbose=False):
        """zen_amd/bin/<program> from the add-on's demo source, against its library and libzen_hip.so; made again where the
        source, the library's header, cli/wav.h, cli/demo.h or the library is newer.  The further add-ons it links are built
        first where they are absent; it sees their headers too."""
        name, exe = self.name, self.DEMO
        srcs = [os.path.join(self.SRC, self.demo_source), os.path.join(self.SRC, "zen_hip_%s.h" % name), os.path.join(HERE, "cli", "wav.h"),
                os.path.join(HERE, "cli", "demo.h"), self.OUT]
        more, libs = [], []
        for e in self.demo_links:
            if not os.path.exists(LIBRARIES[e].OUT):
                LIBRARIES[e].build(verbose=verbose)
            srcs += [os.path.join(HERE, e, "zen_hip_%s.h" % e), LIBRARIES[e].OUT]
            more += ["-I", os.path.join(HERE, e)]
            libs.append("-lzen_hip_" + e)
        if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(p) for p in srcs):
            return exe
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                               "-I", self.SRC, "-I", os.path.join(HERE, "cli")] + more + [srcs[0], "-o", exe, "-L", HERE, "-lzen_hip_" + name] + libs
                              + ["-lzen_hip", "-Wl,-rpath,$ORIGIN/.."])
        if verbose:
            print("built", exe)
        return exe


pcm = Addon("pcm", ["pcm_kernels.hip", "pcm_pipe.hip"], extra_deps=["csrc/host_pipe.h"], title="PCM")
ragged = Addon("ragged", ["ragged_kernels.hip", "ragged.hip"])
live = Addon("live", ["live_kernels.hip", "live.hip"])
pitch = Addon("pitch", ["pitch_kernels.hip", "pitch.hip"], demo=("pitch_track.cpp", "pitch-track", ()))
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
beat = Addon("beat", ["beat_kernels.hip", "beat.hip"], demo=("beat_track.cpp", "beat-track", ()))
# multi (interleaved multichannel audio through the engines' rows) shares the sample arithmetic of pcm/pcm_convert.h
multi = Addon("multi", ["multi_kernels.hip", "multi.hip"], extra_deps=["pcm/pcm_convert.h"], demo=("multi_stems.cpp", "zen-stems", ()))
repet = Addon("repet", ["repet_kernels.hip", "repet.hip"], demo=("repet_main.cpp", "zen-repet", ()))
cqt = Addon("cqt", ["cqt_kernels.hip", "cqt.hip"], demo=("cqt_main.cpp", "zen-cqt", ()))
repsim = Addon("repsim", ["repsim_kernels.hip", "repsim.hip"], demo=("repsim_main.cpp", "zen-repsim", ()))
nmf = Addon("nmf", ["nmf_kernels.hip", "nmf.hip"], demo=("nmf_main.cpp", "zen-nmf", ()))
tsm = Addon("tsm", ["tsm_kernels.hip", "tsm.hip"], demo=("tsm_main.cpp", "zen-stretch", ()))
# zen-shift stretches with tsm's library before it resamples
resample = Addon("resample", ["resample_kernels.hip", "resample.hip"], demo=("resample_main.cpp", "zen-shift", ("tsm",)))
# The one table: every library by name, in the order they are built.  The loader (_addon.load), the programs' further
# add-ons and the command line look names up here; blockrun alone is on the engine's own state, the rest on the C ABI alone.
LIBRARIES = {a.name: a for a in (pcm, ragged, live, pitch, blockrun, beat, multi, repet, cqt, repsim, nmf, tsm, resample)}


if __name__ == "__main__":
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or list(LIBRARIES)
    for n in names:
        LIBRARIES[n].build(force="--force" in sys.argv, verbose=True)
