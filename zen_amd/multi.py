"""ctypes binding of libzen_hip_multi.so (zen_amd/multi/zen_hip_multi.h): interleaved multichannel audio through the engines'
rows, every channel kept.  No fallback: a missing library raises.

    stems = multi.Offline(44100.0, 4096, 256, channels=2).process(x)       # x: [n_frames, 2] int16 or float32
    stems["harm"], stems["perc"]                                           # same shape and dtype as x
    rt = multi.Realtime(44100.0, 256, channels=2)
    out = rt.process(block)                                                # [n_hops * 256, 2] -> "harm", "perc", "resid"
"""
import ctypes as C

import numpy as np

from . import _addon
from ._addon import _f, _i, _sz, _vp
from . import lib as _zl

I16, F32 = 0, 1
PEAK, GAIN = 0, 1
MAX_CHANNELS = 8


class Stats(C.Structure):
    _fields_ = [("calls", C.c_ulonglong), ("device_bytes", C.c_ulonglong), ("allocations", C.c_ulonglong), ("row_stride", C.c_ulonglong)]


# every symbol zen_amd/multi/zen_hip_multi.h declares: (name, restype, argtypes)
_u = C.c_uint
SYMBOLS = [
    ("zen_hip_multi_last_error", C.c_char_p, []),
    ("zen_hip_multi_version", C.c_char_p, []),
    ("zen_hip_multi_split", _i, [_i, _vp, _i, _sz, _vp, _sz, _vp]),
    ("zen_hip_multi_peak", _i, [_vp, _i, _sz, _sz, _vp, _vp]),
    ("zen_hip_multi_join", _i, [_i, _vp, _i, _sz, _sz, _i, _f, _vp, _vp, _vp]),
    ("zen_hip_multi_offline_create", _i, [_f, _sz, _sz, _f, _f, _i, _i, C.POINTER(_vp)]),
    ("zen_hip_multi_offline_destroy", _i, [_vp]),
    ("zen_hip_multi_offline_use_sse_filter", _i, [_vp]),
    ("zen_hip_multi_offline_use_soft_mask", _i, [_vp]),
    ("zen_hip_multi_offline_set_stream", _i, [_vp, _vp]),
    ("zen_hip_multi_offline_device", _i, [_vp, _i, _vp, _sz, _vp, _vp, _i, _f, _vp]),
    ("zen_hip_multi_offline_host", _i, [_vp, _i, _vp, _sz, _vp, _vp, _i, _f, _vp]),
    ("zen_hip_multi_stats", _i, [_vp, C.POINTER(Stats)]),
    ("zen_hip_multi_realtime_create", _i, [_f, _sz, _f, _u, _i, _sz, C.POINTER(_vp)]),
    ("zen_hip_multi_realtime_destroy", _i, [_vp]),
    ("zen_hip_multi_realtime_use_sse_filter", _i, [_vp]),
    ("zen_hip_multi_realtime_use_soft_mask", _i, [_vp]),
    ("zen_hip_multi_realtime_reset", _i, [_vp]),
    ("zen_hip_multi_realtime_set_stream", _i, [_vp, _vp]),
    ("zen_hip_multi_realtime_device", _i, [_vp, _i, _vp, _sz, _vp, _vp, _vp, _f]),
    ("zen_hip_multi_realtime_host", _i, [_vp, _i, _vp, _sz, _vp, _vp, _vp, _f]),
]

_lib = _addon.Library("multi", SYMBOLS)
load, _ck, _ptr = _lib.load, _lib.check, _addon.ptr


def _fmt(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.int16:
        return I16
    if dtype == np.float32:
        return F32
    raise TypeError("multichannel audio is int16 or float32, not %s" % dtype)


def _frames(x, channels):
    """x as a C-contiguous [n_frames, channels] array of its own dtype, and its format"""
    x = np.asarray(x)
    fmt = _fmt(x.dtype)
    if x.ndim == 1 and channels == 1:
        x = x.reshape(-1, 1)
    if x.ndim != 2 or x.shape[1] != channels:
        raise ValueError("expected an array [n_frames, %d], got shape %s" % (channels, x.shape))
    return np.ascontiguousarray(x), fmt


# ---- the kernels alone, on device pointers -----------------------------------------------------------------------------------
def split(fmt, src_dev, channels, n_frames, dst_rows_dev, row_stride, stream=None):
    _ck(load().zen_hip_multi_split(fmt, _ptr(src_dev), channels, n_frames, _ptr(dst_rows_dev), row_stride, stream))


def peak(rows_dev, channels, n_frames, row_stride, minmax_dev, stream=None):
    _ck(load().zen_hip_multi_peak(_ptr(rows_dev), channels, n_frames, row_stride, _ptr(minmax_dev), stream))


def join(fmt, rows_dev, channels, n_frames, row_stride, dst_dev, mode=GAIN, gain=32767.0, minmax_dev=None, stream=None):
    _ck(load().zen_hip_multi_join(fmt, _ptr(rows_dev), channels, n_frames, row_stride, mode, gain, _ptr(minmax_dev), _ptr(dst_dev), stream))


class Offline(_addon.Owner):
    """zen_hip_multi_offline_t: the two-pass separation of every channel of an interleaved clip."""
    _lib, _prefix = _lib, "offline_"

    def __init__(self, fs, hop_h=4096, hop_p=256, beta_h=2.0, beta_p=2.0, nocopybord=False, channels=2):
        self._create(fs, hop_h, hop_p, beta_h, beta_p, int(nocopybord), channels)
        self.channels = channels
        self.peaks = None

    def use_sse_filter(self):
        _ck(self._L.zen_hip_multi_offline_use_sse_filter(self._h))

    def use_soft_mask(self):
        _ck(self._L.zen_hip_multi_offline_use_soft_mask(self._h))

    def stats(self):
        st = Stats()
        _ck(self._L.zen_hip_multi_stats(self._h, C.byref(st)))
        return _addon.as_dict(st)

    def process_device(self, fmt, in_dev, n_frames, harm=None, perc=None, mode=PEAK, gain=32767.0, peaks_dev=None):
        """DeviceBuffers or device addresses of interleaved frames.  Asynchronous on the handle's stream."""
        _ck(self._L.zen_hip_multi_offline_device(self._h, fmt, _ptr(in_dev), n_frames, _ptr(harm), _ptr(perc), mode, gain, _ptr(peaks_dev)))

    def process(self, x, mode=PEAK, gain=32767.0, want=("harm", "perc")):
        """x: [n_frames, channels], int16 or float32.  Returns {"harm": ..., "perc": ...} of x's shape and dtype (only the
        stems of `want`); self.peaks: the two peaks of an int16 PEAK call.  Synchronous."""
        x, fmt = _frames(x, self.channels)
        outs = {k: np.empty_like(x) for k in ("harm", "perc") if k in want}
        pk = np.zeros(2, np.float32)
        p = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        _ck(self._L.zen_hip_multi_offline_host(self._h, fmt, p(x), x.shape[0], p(outs.get("harm")), p(outs.get("perc")), mode, gain,
                                               pk.ctypes.data))
        self.peaks = pk
        return outs


class Realtime(_addon.Owner):
    """zen_hip_multi_realtime_t: the causal separation of every channel, block by block; the state carries over."""
    _lib, _prefix = _lib, "realtime_"
    NAMES = (("harm", _zl.OUTPUT_HARMONIC), ("perc", _zl.OUTPUT_PERCUSSIVE), ("resid", _zl.OUTPUT_RESIDUAL))

    def __init__(self, fs, hop=256, beta=2.0, output_flags=_zl.OUTPUT_HARMONIC | _zl.OUTPUT_PERCUSSIVE | _zl.OUTPUT_RESIDUAL, channels=2,
                 max_hops=0):
        self._create(fs, hop, beta, output_flags, channels, max_hops)
        self.hop, self.channels, self.flags = hop, channels, output_flags

    def use_sse_filter(self):
        _ck(self._L.zen_hip_multi_realtime_use_sse_filter(self._h))

    def use_soft_mask(self):
        _ck(self._L.zen_hip_multi_realtime_use_soft_mask(self._h))

    def reset(self):
        _ck(self._L.zen_hip_multi_realtime_reset(self._h))

    def process_device(self, fmt, in_dev, n_hops, harm=None, perc=None, resid=None, gain=32767.0):
        """DeviceBuffers or device addresses of interleaved frames.  Asynchronous on the handle's stream."""
        _ck(self._L.zen_hip_multi_realtime_device(self._h, fmt, _ptr(in_dev), n_hops, _ptr(harm), _ptr(perc), _ptr(resid), gain))

    def process(self, x, gain=32767.0):
        """x: [n_hops * hop, channels], int16 or float32 (whole hops).  Returns {"harm", "perc", "resid"} (those of the
        output flags) of x's shape and dtype.  Synchronous."""
        x, fmt = _frames(x, self.channels)
        if x.shape[0] % self.hop:
            raise ValueError("%d frames are not whole hops of %d" % (x.shape[0], self.hop))
        outs = {k: np.empty_like(x) for k, bit in self.NAMES if self.flags & bit}
        p = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        _ck(self._L.zen_hip_multi_realtime_host(self._h, fmt, p(x), x.shape[0] // self.hop, p(outs.get("harm")), p(outs.get("perc")),
                                                p(outs.get("resid")), gain))
        return outs
