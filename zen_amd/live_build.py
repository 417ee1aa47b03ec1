"""Builds zen_amd/libzen_hip_live.so (zen_amd/live: the two-pass separation as a stream, on top of libzen_hip.so's C ABI) for gfx950
with hipcc.

The library links against libzen_hip.so (zen_amd/build.py builds that one first) and finds it beside itself ($ORIGIN).
-ffp-contract=off and no fast-math flag: the one float operation of the kernels, P1 + R1, is a single IEEE add.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "live")
OUT = os.path.join(HERE, "libzen_hip_live.so")
OBJDIR = os.path.join(HERE, "build_live")
BASE = os.path.join(HERE, "libzen_hip.so")
SOURCES = ["live_kernels.hip", "live.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall",
         "-I", os.path.join(os.path.dirname(HERE), "include")]


def _deps():
    hdrs = [os.path.join(SRC, f) for f in os.listdir(SRC) if f.endswith(".h")]
    hdrs.append(os.path.join(os.path.dirname(HERE), "include", "zen_hip.h"))
    hdrs.append(os.path.abspath(__file__))   # the flags live here
    return hdrs


def _compile(src):
    obj = os.path.join(OBJDIR, src.replace(".hip", ".o"))
    srcp = os.path.join(SRC, src)
    newest = max(os.path.getmtime(p) for p in [srcp] + _deps())
    if os.path.exists(obj) and os.path.getmtime(obj) >= newest:
        return obj, False
    subprocess.check_call([HIPCC] + FLAGS + ["-c", srcp, "-o", obj])
    return obj, True


def build(force=False, verbose=False):
    if not os.path.exists(BASE):
        raise RuntimeError("%s not built: zen_amd/build.py first (the live library links against it)" % BASE)
    os.makedirs(OBJDIR, exist_ok=True)
    if force:
        for f in os.listdir(OBJDIR):
            os.remove(os.path.join(OBJDIR, f))
    with ThreadPoolExecutor(max_workers=len(SOURCES)) as ex:
        res = list(ex.map(_compile, SOURCES))
    if any(r[1] for r in res) or not os.path.exists(OUT) or os.path.getmtime(OUT) < os.path.getmtime(BASE):
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + [r[0] for r in res]
                              + ["-L", HERE, "-lzen_hip", "-Wl,-rpath,$ORIGIN"])
        if verbose:
            print("built", OUT)
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
