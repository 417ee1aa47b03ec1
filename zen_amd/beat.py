"""ctypes binding of libzen_hip_beat.so (zen_amd/beat/zen_hip_beat.h): the complex-domain onset function and the beat
tracker of Stark, Davies and Plumbley on hops of rows, on the device.  No fallback: a missing library raises.

    bt = beat.Beat(44100.0, 512)
    odf, score, flag, tempo = bt.run(x)                  # float32 samples -> one value per hop of 512
    seconds = beat.beat_times(flag, 512, 44100.0)
    with_hpr, without = beat.track_hpr(x, 44100.0)        # the percussive separation in front, all on the device
"""
import ctypes as C

import numpy as np

from . import _addon
from ._addon import _f, _i, _pd, _pull, _sz, _vp
from . import lib as _zl

KERNELS = ("frame", "fft", "csd", "track")
OUTPUTS = ("odf", "score", "beat", "tempo")
TABLE_WINDOW, TABLE_PERIOD, TABLE_TEMPO, TABLE_PAST, TABLE_FUTURE, TABLE_RAYLEIGH, TABLE_TRANSITION = range(7)
N_TEMPI = 41


class Stats(C.Structure):
    _fields_ = [("hops", C.c_ulonglong), ("slices", C.c_ulonglong), ("device_bytes", C.c_ulonglong), ("allocations", C.c_ulonglong)]


# every symbol zen_amd/beat/zen_hip_beat.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("zen_hip_beat_last_error", C.c_char_p, []),
    ("zen_hip_beat_version", C.c_char_p, []),
    ("zen_hip_beat_create", _i, [_f, _sz, _sz, _sz, C.POINTER(_vp)]),
    ("zen_hip_beat_destroy", _i, [_vp]),
    ("zen_hip_beat_reset", _i, [_vp]),
    ("zen_hip_beat_set_stream", _i, [_vp, _vp]),
    ("zen_hip_beat_run_device", _i, [_vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _sz]),
    ("zen_hip_beat_run_host", _i, [_vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _sz]),
    ("zen_hip_beat_stats", _i, [_vp, C.POINTER(Stats)]),
    ("zen_hip_beat_profile", _i, [_vp, _i]),
    ("zen_hip_beat_profile_get", _i, [_vp, _pd, _pull, _pull]),
    ("zen_hip_beat_table", _i, [_f, _sz, _i, _sz, _vp, _sz]),
]

_lib = _addon.Library("beat", SYMBOLS, kernels=KERNELS, stats=Stats)
load, _ck, _ptr = _lib.load, _lib.check, _addon.ptr


def table(fs, hop, which, index=0):
    """One host table of (fs, hop) as a float32 array; needs no device.  `index`: the period b of TABLE_PAST / TABLE_FUTURE,
    the row of TABLE_TRANSITION."""
    out = np.empty(max(2 * hop, 256), np.float32)
    _ck(load().zen_hip_beat_table(fs, hop, which, index, out.ctypes.data, out.size))
    b = int(index)
    length = {TABLE_WINDOW: 2 * hop, TABLE_PAST: 2 * b - (b + 1) // 2 + 1, TABLE_FUTURE: b, TABLE_RAYLEIGH: 128}.get(which, N_TEMPI)
    return out[:length].copy()


def beat_times(beat, hop, fs):
    """the seconds of the hops a beat row flags: hop index * hop / fs"""
    return np.flatnonzero(np.asarray(beat) > 0) * hop / float(fs)


class Beat(_addon.Handle):
    """zen_hip_beat_t: hops of `hop` samples of n_streams rows per call; the state carries over from call to call."""
    _lib = _lib

    def __init__(self, fs, hop=512, n_streams=1, max_hops=0):
        self._create(fs, hop, n_streams, max_hops)
        self.fs, self.hop, self.n_streams = fs, hop, n_streams

    def reset(self):
        _ck(self._L.zen_hip_beat_reset(self._h))

    def run_device(self, in_dev, in_stride, n_hops, odf=None, score=None, beat=None, tempo=None, out_stride=0):
        """DeviceBuffers or device addresses (ints, e.g. DeviceBuffer.offset(k)).  Asynchronous on the handle's stream."""
        _ck(self._L.zen_hip_beat_run_device(self._h, _ptr(in_dev), in_stride, n_hops, _ptr(odf), _ptr(score), _ptr(beat), _ptr(tempo), out_stride))

    def run(self, x):
        """x: float32, (m,) for one stream or (n_streams, m); every whole hop of it.  Returns (odf, score, beat, tempo), each
        (n_hops,) or (n_streams, n_hops).  Synchronous."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        one = x.ndim == 1
        x = x.reshape(self.n_streams, -1)
        m = x.shape[1]
        cnt = m // self.hop
        outs = [np.empty((self.n_streams, cnt), np.float32) for _ in range(4)]
        _ck(self._L.zen_hip_beat_run_host(self._h, x.ctypes.data if cnt else None, m, cnt, *(o.ctypes.data if cnt else None for o in outs), cnt))
        return tuple(r[0] if one else r for r in outs)


class HprTracker:
    """The percussive separation (causal, hop = hpr_hop, percussive output) and the tracker behind it, on one device buffer
    of two rows: the samples and their percussive part.  Sized for up to max_samples samples per call, a multiple of both
    hops."""

    def __init__(self, fs, hop=512, hpr_hop=1024, beta=2.5, max_samples=1 << 20):
        self.hop, self.hpr_hop, self.row = hop, hpr_hop, max_samples
        assert max_samples % hop == 0 and max_samples % hpr_hop == 0
        self.hpr = _zl.HPR(fs, hpr_hop, beta, _zl.OUTPUT_PERCUSSIVE, _zl.TIME_CAUSAL)
        self.beat = Beat(fs, hop, n_streams=2)
        self.rows = _zl.DeviceBuffer(2 * max_samples)
        self.out = _zl.DeviceBuffer(4 * 2 * (max_samples // hop))

    def upload(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        unit = max(self.hop, self.hpr_hop)
        m = x.size // unit * unit
        assert m <= self.row
        self.rows.upload(x[:m])
        return m

    def run_device(self, m):
        """`m` samples already in row 0 of self.rows: separation and both trackers, queued; self.out: four results of two
        rows each -- without, with HPR"""
        cap = self.row // self.hop
        self.hpr.process(self.rows.ptr, m // self.hpr_hop, in_stride=self.row, perc=self.rows.offset(self.row), out_stride=self.row)
        self.beat.run_device(self.rows, self.row, m // self.hop, *(self.out.offset(k * 2 * cap) for k in range(4)), out_stride=cap)

    def download(self, m):
        """(with, without): each the four rows (odf, score, beat, tempo) of m / hop values"""
        cap, cnt = self.row // self.hop, m // self.hop
        got = self.out.download().reshape(4, 2, cap)
        return tuple(got[:, 1, :cnt].copy()), tuple(got[:, 0, :cnt].copy())


def track_hpr(x, fs, hop=512, hpr_hop=1024, beta=2.5):
    """(odf, score, beat, tempo) of every whole hop of x, (with, without) the percussive separation in front of the tracker:
    zen_hip_hpr_process at hop hpr_hop (causal, OUTPUT_PERCUSSIVE) writes the percussive stream into device memory and the
    tracker reads it there.  x is cut to a multiple of both hops."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    unit = max(hop, hpr_hop)
    m = x.size // unit * unit
    if m == 0:
        e = tuple(np.empty(0, np.float32) for _ in range(4))
        return e, e
    t = HprTracker(fs, hop, hpr_hop, beta, max_samples=m)
    t.upload(x)
    t.run_device(m)
    return t.download(m)
