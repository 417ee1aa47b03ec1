"""ctypes binding of libzen_hip_live.so (zen_amd/live/zen_hip_live.h): the two-pass separation (HPR-I) as a stream with a
fixed latency.  No fallback: a missing library raises.

    lv = live.Live(44100.0, 4096, 256, 2.0, 2.0, max_push=4096)
    for block in blocks:                                 # float32, any sizes
        harm, perc, dry = lv.push(block)                 # what has become ready: lv.latency samples behind the input
    harm, perc, dry = lv.finish()                        # the rest; together: zen offline's samples of the whole clip
"""
import ctypes as C

import numpy as np

from . import _addon
from ._addon import _f, _i, _pd, _psz, _pull, _sz, _vp
from . import lib as _zl

KERNELS = ("feed", "mid", "out")


class Stats(C.Structure):
    _fields_ = [("pushed", C.c_ulonglong), ("delivered", C.c_ulonglong), ("device_bytes", C.c_ulonglong),
                ("allocations", C.c_ulonglong)]


# every symbol zen_amd/live/zen_hip_live.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("zen_hip_live_last_error", C.c_char_p, []),
    ("zen_hip_live_version", C.c_char_p, []),
    ("zen_hip_live_max_samples", _i, [_sz, _sz, _pull]),
    ("zen_hip_live_create", _i, [_f, _sz, _sz, _f, _f, _i, _sz, _sz, C.POINTER(_vp)]),
    ("zen_hip_live_destroy", _i, [_vp]),
    ("zen_hip_live_set_stream", _i, [_vp, _vp]),
    ("zen_hip_live_use_sse_filter", _i, [_vp]),
    ("zen_hip_live_use_soft_mask", _i, [_vp]),
    ("zen_hip_live_reset", _i, [_vp]),
    ("zen_hip_live_latency", _i, [_vp, _psz]),
    ("zen_hip_live_produces", _i, [_vp, _sz, _psz]),
    ("zen_hip_live_pending", _i, [_vp, _psz]),
    ("zen_hip_live_push_device", _i, [_vp, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _psz]),
    ("zen_hip_live_finish_device", _i, [_vp, _vp, _vp, _vp, _sz, _psz]),
    ("zen_hip_live_push_host", _i, [_vp, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _psz]),
    ("zen_hip_live_finish_host", _i, [_vp, _vp, _vp, _vp, _sz, _psz]),
    ("zen_hip_live_stats", _i, [_vp, C.POINTER(Stats)]),
    ("zen_hip_live_profile", _i, [_vp, _i]),
    ("zen_hip_live_profile_get", _i, [_vp, _pd, _pull, _pull]),
    ("zen_hip_live_profile_get_engine", _i, [_vp, _i, _pd, _pull]),
]

_lib = _addon.Library("live", SYMBOLS, (_zl.E_HOPS_NOT_DIVISIBLE,), KERNELS, Stats)
load, _ck = _lib.load, _lib.check


def max_samples(hop_h, hop_p):
    """The longest stream a session of these hops accepts (the float padder's range); host arithmetic only."""
    out = C.c_ulonglong()
    _ck(load().zen_hip_live_max_samples(hop_h, hop_p, C.byref(out)))
    return out.value


class Live(_addon.Handle, _addon.EngineProfiled):
    """zen_hip_live_t: one session of n_streams streams in lock step."""
    _lib = _lib

    def __init__(self, fs, hop_h=4096, hop_p=256, beta_h=2.0, beta_p=2.0, nocopybord=False, n_streams=1, max_push=0):
        self._create(fs, hop_h, hop_p, beta_h, beta_p, int(nocopybord), n_streams, max_push)
        self.n_streams, self.hop_h, self.hop_p = n_streams, hop_h, hop_p
        n = C.c_size_t()
        _ck(self._L.zen_hip_live_latency(self._h, C.byref(n)))
        self.latency = n.value

    def use_sse_filter(self):
        _ck(self._L.zen_hip_live_use_sse_filter(self._h))

    def use_soft_mask(self):
        _ck(self._L.zen_hip_live_use_soft_mask(self._h))

    def reset(self):
        _ck(self._L.zen_hip_live_reset(self._h))

    def produces(self, m):
        n = C.c_size_t()
        _ck(self._L.zen_hip_live_produces(self._h, m, C.byref(n)))
        return n.value

    def pending(self):
        n = C.c_size_t()
        _ck(self._L.zen_hip_live_pending(self._h, C.byref(n)))
        return n.value

    def push_device(self, in_dev, m, in_stride, harm=None, perc=None, dry=None, out_stride=0):
        """Device pointers (ints, e.g. DeviceBuffer.ptr).  Asynchronous on the handle's stream; returns the samples written to
        each output row."""
        n = C.c_size_t()
        _ck(self._L.zen_hip_live_push_device(self._h, in_dev, m, in_stride, harm, perc, dry, out_stride, C.byref(n)))
        return n.value

    def finish_device(self, harm=None, perc=None, dry=None, out_stride=0):
        n = C.c_size_t()
        _ck(self._L.zen_hip_live_finish_device(self._h, harm, perc, dry, out_stride, C.byref(n)))
        return n.value

    def _outs(self, cnt, want):
        shape = (cnt,) if self.n_streams == 1 else (self.n_streams, cnt)
        return [np.empty(shape, np.float32) if w else None for w in want]

    def push(self, x, want=(True, True, True)):
        """x: float32, (m,) for one stream or (n_streams, m).  Returns (harm, perc, dry) of what has become ready, shaped like
        x (None for an output that is not wanted).  Synchronous."""
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(self.n_streams, -1)
        m = x.shape[1]
        cnt = self.produces(m)
        outs = self._outs(cnt, want)
        n = C.c_size_t()
        _ck(self._L.zen_hip_live_push_host(self._h, x.ctypes.data if m else None, m, m, *(o.ctypes.data if o is not None and cnt else None
                                                                                           for o in outs), cnt, C.byref(n)))
        assert n.value == cnt
        return tuple(outs)

    def finish(self, want=(True, True, True)):
        """The rest of the stream; the session is reset.  Synchronous."""
        cnt = self.pending()
        outs = self._outs(cnt, want)
        n = C.c_size_t()
        _ck(self._L.zen_hip_live_finish_host(self._h, *(o.ctypes.data if o is not None and cnt else None for o in outs), cnt, C.byref(n)))
        assert n.value == cnt
        return tuple(outs)
