"""ctypes binding of libzen_hip_pitch.so (zen_amd/pitch/zen_hip_pitch.h): the McLeod pitch method on chunks of rows, on the
device.  No fallback: a missing library raises.

    pt = pitch.Pitch(44100.0, 4096)
    f0, period, clarity = pt.run(x)                      # float32 samples -> one value per chunk of 4096
    with_hpr, without = pitch.track_hpr(x, 44100.0, 4096)  # the harmonic separation in front, all on the device
"""
import ctypes as C

import numpy as np

from . import _addon
from ._addon import _f, _i, _pd, _pull, _sz, _vp
from . import lib as _zl

KERNELS = ("pad", "fft_forward", "power", "fft_inverse", "pick")


class Stats(C.Structure):
    _fields_ = [("chunks", C.c_ulonglong), ("device_bytes", C.c_ulonglong), ("allocations", C.c_ulonglong)]


# every symbol zen_amd/pitch/zen_hip_pitch.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("zen_hip_pitch_last_error", C.c_char_p, []),
    ("zen_hip_pitch_version", C.c_char_p, []),
    ("zen_hip_pitch_create", _i, [_f, _sz, _sz, _sz, C.POINTER(_vp)]),
    ("zen_hip_pitch_destroy", _i, [_vp]),
    ("zen_hip_pitch_set_stream", _i, [_vp, _vp]),
    ("zen_hip_pitch_run_device", _i, [_vp, _vp, _sz, _sz, _sz, _vp, _vp, _vp, _vp, _sz]),
    ("zen_hip_pitch_run_host", _i, [_vp, _vp, _sz, _sz, _sz, _vp, _vp, _vp, _vp, _sz]),
    ("zen_hip_pitch_stats", _i, [_vp, C.POINTER(Stats)]),
    ("zen_hip_pitch_profile", _i, [_vp, _i]),
    ("zen_hip_pitch_profile_get", _i, [_vp, _pd, _pull, _pull]),
]

_lib = _addon.Library("pitch", SYMBOLS, kernels=KERNELS, stats=Stats)
load, _ck, _ptr = _lib.load, _lib.check, _addon.ptr


class Pitch(_addon.Handle):
    """zen_hip_pitch_t: chunks of n samples of n_streams rows per call."""
    _lib = _lib

    def __init__(self, fs, n=4096, n_streams=1, max_chunks=0):
        self._create(fs, n, n_streams, max_chunks)
        self.fs, self.n, self.n_streams = fs, n, n_streams

    def run_device(self, in_dev, in_stride, n_chunks, step=None, pitch=None, period=None, clarity=None, nsdf=None, out_stride=0):
        """DeviceBuffers or device addresses (ints, e.g. DeviceBuffer.offset(k)).  Asynchronous on the handle's stream."""
        _ck(self._L.zen_hip_pitch_run_device(self._h, _ptr(in_dev), in_stride, n_chunks, self.n if step is None else step, _ptr(pitch),
                                             _ptr(period), _ptr(clarity), _ptr(nsdf), out_stride))

    def n_chunks(self, samples, step=None):
        step = self.n if step is None else step
        return 0 if samples < self.n else (samples - self.n) // step + 1

    def run(self, x, step=None, nsdf=False):
        """x: float32, (m,) for one stream or (n_streams, m); every whole chunk x[c*step : c*step + n] of it.  Returns (pitch,
        period, clarity), each (n_chunks,) or (n_streams, n_chunks), and with nsdf=True the NSDF rows (..., n_chunks, n) as a
        fourth.  Synchronous."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        one = x.ndim == 1
        x = x.reshape(self.n_streams, -1)
        m = x.shape[1]
        step = self.n if step is None else step
        cnt = self.n_chunks(m, step)
        outs = [np.empty((self.n_streams, cnt), np.float32) for _ in range(3)]
        rows = np.empty((self.n_streams, cnt, self.n), np.float32) if nsdf else None
        _ck(self._L.zen_hip_pitch_run_host(self._h, x.ctypes.data if cnt else None, m, cnt, step, *(o.ctypes.data if cnt else None for o in outs),
                                           rows.ctypes.data if nsdf and cnt else None, cnt))
        res = outs + ([rows] if nsdf else [])
        return tuple(r[0] if one else r for r in res)


class HprTracker:
    """The harmonic separation (causal, hop = n, harmonic output) and the tracker behind it, on one device buffer of two rows:
    the samples and their harmonic part.  Sized for up to max_chunks chunks per call."""

    def __init__(self, fs, n=4096, beta=2.5, max_chunks=64):
        self.n, self.max_chunks = n, max_chunks
        self.hpr = _zl.HPR(fs, n, beta, _zl.OUTPUT_HARMONIC, _zl.TIME_CAUSAL)
        self.pitch = Pitch(fs, n, n_streams=2)
        self.rows = _zl.DeviceBuffer(2 * max_chunks * n)
        self.out = _zl.DeviceBuffer(2 * max_chunks)

    def upload(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        cnt = x.size // self.n
        assert cnt <= self.max_chunks
        self.rows.upload(x[:cnt * self.n])
        return cnt

    def run_device(self, cnt):
        """`cnt` chunks already in row 0 of self.rows: separation and both trackers, queued; self.out rows: without, with HPR"""
        n, row = self.n, self.max_chunks * self.n
        self.hpr.process(self.rows.ptr, cnt, in_stride=row, harm=self.rows.offset(row), out_stride=row)
        self.pitch.run_device(self.rows, row, cnt, pitch=self.out, out_stride=self.max_chunks)

    def download(self, cnt):
        got = self.out.download().reshape(2, self.max_chunks)
        return got[1, :cnt].copy(), got[0, :cnt].copy()


def track_hpr(x, fs, n, beta=2.5):
    """The pitch of every whole chunk of n samples of x, (with, without) the harmonic separation in front of the tracker:
    zen_hip_hpr_process at hop n (causal, OUTPUT_HARMONIC) writes the harmonic stream into device memory and the tracker
    reads it there."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    cnt = x.size // n
    if cnt == 0:
        return np.empty(0, np.float32), np.empty(0, np.float32)
    t = HprTracker(fs, n, beta, max_chunks=cnt)
    t.upload(x)
    t.run_device(cnt)
    return t.download(cnt)
