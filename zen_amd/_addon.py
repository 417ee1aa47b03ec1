"""What the ctypes bindings of the add-on libraries (one module per entry of addon_build.LIBRARIES but blockrun) share: loading, the return-code
check and the profile getters.  No fallback: a missing library that cannot be built raises."""
import ctypes as C
import os

from . import lib as _zl

_HERE = os.path.dirname(os.path.abspath(__file__))
_libs = {}

ENGINE_CLASSES = ("stft", "freq_filter", "time_filter", "istft", "finalize", "rt_fused")


def load(name, symbols):
    """libzen_hip_<name>.so with `symbols` ((name, restype, argtypes), ...) bound; loaded once.  ZEN_HIP_<NAME>_SO names another
    file, which must exist; the default file is built first where it is absent (zen_amd/addon_build.py; needs hipcc and a
    built libzen_hip.so).  Raises if that fails."""
    if name not in _libs:
        env_var = "ZEN_HIP_%s_SO" % name.upper()
        so = os.environ.get(env_var) or os.path.join(_HERE, "libzen_hip_%s.so" % name)
        if not os.path.exists(so):
            if env_var in os.environ:
                raise ImportError("%s does not exist" % so)
            from . import addon_build
            addon_build.LIBRARIES[name].build()
        _zl.load()                      # the same libzen_hip.so for both bindings (found again beside this one by its rpath)
        L = C.CDLL(so)
        for sym, res, args in symbols:
            f = getattr(L, sym)
            f.restype = res
            f.argtypes = args
        _libs[name] = L
    return _libs[name]


def check(rc, last_error, zg_codes=()):
    """Raises what return code `rc` stands for, with the library's message: ZgException for the codes of `zg_codes` (the
    reference's own exception), ZenHipError for every other."""
    if rc:
        msg = last_error().decode()
        raise (_zl.ZgException if rc in zg_codes else _zl.ZenHipError)(rc, msg)


def profile_get(ck, fn, handle, kernels):
    """{kernel: {"ms", "bytes", "launches"}} since the last call; synchronises."""
    k = len(kernels)
    ms, by, n = (C.c_double * k)(), (C.c_ulonglong * k)(), (C.c_ulonglong * k)()
    ck(fn(handle, ms, by, n))
    return {name: {"ms": ms[i], "bytes": by[i], "launches": n[i]} for i, name in enumerate(kernels)}


def profile_get_engine(ck, fn, handle):
    """The engines' per-class kernel times of pass 1 and pass 2, as HPRIOffline.profile_get_all."""
    out = {}
    for ps in (1, 2):
        ms, n = (C.c_double * 6)(), (C.c_ulonglong * 6)()
        ck(fn(handle, ps, ms, n))
        out["pass%d" % ps] = {k: {"ms": ms[i], "launches": n[i]} for i, k in enumerate(ENGINE_CLASSES)}
    return out
