"""What the ctypes bindings of the add-on libraries (one module per entry of addon_build.LIBRARIES but blockrun) share, the
Python side of zen_amd/addon/addon_host.h: loading and the return-code check (Library), the handle every session class owns
(Owner, Profiled, Handle), the profile getters and what the STFT bindings repeat.  A binding module states its library's
name, SYMBOLS, KERNELS and Stats once and writes its own calls.  No fallback: a missing library that cannot be built raises."""
import ctypes as C
import os

import numpy as np

from . import lib as _zl

_HERE = os.path.dirname(os.path.abspath(__file__))
_libs = {}

ENGINE_CLASSES = ("stft", "freq_filter", "time_filter", "istft", "finalize", "rt_fused")

# the ctypes shorthands of the SYMBOLS tables
_vp, _sz, _i, _f, _d = C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_double
_pd, _pull, _psz = C.POINTER(C.c_double), C.POINTER(C.c_ulonglong), C.POINTER(C.c_size_t)


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


def ptr(b):
    """a DeviceBuffer, a raw device address or None"""
    return getattr(b, "ptr", b)


def as_dict(s):
    """a ctypes Structure as {field: value}"""
    return {f[0]: getattr(s, f[0]) for f in s._fields_}


class Library:
    """libzen_hip_<name>.so as its binding module states it: the name and SYMBOLS, the codes that raise ZgException, and for
    the handle classes below KERNELS (the order of zen_hip_<name>_profile_get) and the Stats structure.  A module takes
    `load` and `check` (its `_ck`) from here."""

    def __init__(self, name, symbols, zg_codes=(), kernels=(), stats=None):
        self.name, self.symbols, self.zg_codes, self.kernels, self.stats = name, symbols, zg_codes, kernels, stats
        self.stem = "zen_hip_%s_" % name

    def load(self):
        """Load the library, building it first where it is absent (_addon.load).  Raises if that fails."""
        return load(self.name, self.symbols)

    def fn(self, short):
        """zen_hip_<name>_<short>"""
        return getattr(self.load(), self.stem + short)

    def check(self, rc):
        if rc:
            check(rc, self.fn("last_error"), self.zg_codes)

    def stft_table(self, nfft, which):
        """the window (nfft values) or the overlap divisor (nfft / 2 values) as a float32 array; needs no device"""
        out = np.empty(nfft if which == 0 else nfft // 2, np.float32)       # TABLE_WINDOW is 0 in every STFT library
        self.check(self.fn("table")(nfft, which, out.ctypes.data, out.size))
        return out


class Owner:
    """The C handle of a session class, in `_h`: made by zen_hip_<name>_<_prefix>create, destroyed once, when the object goes
    or at _close(), and never where the constructor raised before there was one.  `_L` is the loaded library, resolved at
    construction, so that a method calls self._L.zen_hip_<name>_<function>(self._h, ...) without loading or looking up again.
    A subclass states `_lib`, its module's Library."""
    _lib, _prefix = None, ""

    def _create(self, *args):
        self._L = self._lib.load()
        h = C.c_void_p()
        self._lib.check(self._fn("create")(*args, C.byref(h)))
        self._h = h.value

    def _fn(self, short):
        return getattr(self._L, self._lib.stem + self._prefix + short)

    def _close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._fn("destroy")(h)

    def __del__(self):
        self._close()

    def set_stream(self, stream):
        self._lib.check(self._fn("set_stream")(self._h, stream))


class Profiled(Owner):
    """... whose library times its kernels: the library's KERNELS name the rows of profile_get."""

    def profile(self, enable=True):
        self._lib.check(self._fn("profile")(self._h, int(bool(enable))))

    def profile_get(self):
        """{kernel: {"ms", "bytes", "launches"}} since the last call; synchronises."""
        return profile_get(self._lib.check, self._fn("profile_get"), self._h, self._lib.kernels)


class Handle(Profiled):
    """... and counts what it did: addon_host.h's Handle<K> as Python sees it."""

    def stats(self):
        st = self._lib.stats()
        self._lib.check(self._fn("stats")(self._h, C.byref(st)))
        return as_dict(st)


class EngineProfiled:
    """beside Profiled, for the libraries that drive the two-pass engine"""

    def profile_get_engine(self):
        """The engines' per-class kernel times, as HPRIOffline.profile_get_all."""
        return profile_get_engine(self._lib.check, self._fn("profile_get_engine"), self._h)


# ---- what the STFT bindings (repet, repsim, nmf: zen_amd/addon/stft_host.h) and the other clip-wise sessions repeat -----------
def n_frames(n, nfft):
    return -(-n // (nfft // 2)) + 1


def clips(x, n_clips):
    """x, float32 of shape (n,) for one clip or (n_clips, n), as (the contiguous (n_clips, n) array, whether it was one clip)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return x.reshape(n_clips, -1), x.ndim == 1


def pick(one):
    """what shapes a (n_clips, ...) result, or None, like the input: row 0 for one clip, the array itself otherwise"""
    return (lambda a: None if a is None else a[0]) if one else (lambda a: a)
