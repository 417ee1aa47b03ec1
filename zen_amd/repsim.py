"""ctypes binding of libzen_hip_repsim.so (zen_amd/repsim/zen_hip_repsim.h): REPET-SIM, the repeating background of a
recording against its foreground where the repetition has no single period, on the device.  No fallback: a missing library
raises.

    background, foreground = repsim.separate(x, 44100.0)                     # float32 samples
    rs = repsim.Repsim(44100.0, 2048, n_clips=2, max_samples=n)                # a session: several clips per call
    bg, fg = rs.run(clips)
"""
import ctypes as C

import numpy as np

from . import _addon
from ._addon import _d, _f, _i, _pd, _pull, _sz, _vp

KERNELS = ("frame", "fft", "magnitude", "similarity_mfma", "similarity_valu", "select", "gather_median", "mask", "ifft", "overlap_add")
TABLE_WINDOW, TABLE_DIVISOR = range(2)
ROUTE_DEFAULT, ROUTE_MFMA, ROUTE_VALU = range(3)
MAX_NEIGHBOURS, MAX_FRAMES, REGISTER_NEIGHBOURS = 256, 16384, 32
THRESHOLD, DISTANCE, NUMBER, HIGHPASS = 0.0, 1.0, 100, 100.0


class Stats(C.Structure):
    _fields_ = [("calls", C.c_ulonglong), ("clips", C.c_ulonglong), ("bands", C.c_ulonglong), ("device_bytes", C.c_ulonglong),
                ("allocations", C.c_ulonglong)]


# every symbol zen_amd/repsim/zen_hip_repsim.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("zen_hip_repsim_last_error", C.c_char_p, []),
    ("zen_hip_repsim_version", C.c_char_p, []),
    ("zen_hip_repsim_create", _i, [_f, _sz, _sz, _sz, C.POINTER(_vp)]),
    ("zen_hip_repsim_destroy", _i, [_vp]),
    ("zen_hip_repsim_set_stream", _i, [_vp, _vp]),
    ("zen_hip_repsim_set_params", _i, [_vp, _d, _d, _sz, _d]),
    ("zen_hip_repsim_separate_device", _i, [_vp, _vp, _sz, _sz, _vp, _vp, _sz, _vp, _vp]),
    ("zen_hip_repsim_separate_host", _i, [_vp, _vp, _sz, _sz, _vp, _vp, _sz, _vp, _vp]),
    ("zen_hip_repsim_similarity_device", _i, [_vp, _sz, _sz, _sz, _vp, _sz, _i, _vp]),
    ("zen_hip_repsim_select_device", _i, [_vp, _sz, _sz, _f, _sz, _sz, _vp, _vp, _vp]),
    ("zen_hip_repsim_gather_median_device", _i, [_vp, _sz, _sz, _sz, _vp, _vp, _sz, _sz, _vp, _sz, _vp]),
    ("zen_hip_repsim_stats", _i, [_vp, C.POINTER(Stats)]),
    ("zen_hip_repsim_profile", _i, [_vp, _i]),
    ("zen_hip_repsim_profile_get", _i, [_vp, _pd, _pull, _pull]),
    ("zen_hip_repsim_table", _i, [_sz, _i, _vp, _sz]),
]

_lib = _addon.Library("repsim", SYMBOLS, kernels=KERNELS, stats=Stats)
load, _ck, _ptr = _lib.load, _lib.check, _addon.ptr
n_frames, table = _addon.n_frames, _lib.stft_table


def similarity_device(v_dev, m, bins, v_stride, s_dev, s_stride, route=ROUTE_DEFAULT, stream=None):
    """the similarity matrix alone on device memory: DeviceBuffers or device addresses.  Asynchronous on `stream`."""
    _ck(load().zen_hip_repsim_similarity_device(_ptr(v_dev), m, bins, v_stride, _ptr(s_dev), s_stride, route, stream))


def select_device(s_dev, m, s_stride, threshold, distance, number, idx_dev, counts_dev, stream=None):
    """the selection alone: idx_dev receives m rows of `number` int32, counts_dev m int32.  Asynchronous on `stream`."""
    _ck(load().zen_hip_repsim_select_device(_ptr(s_dev), m, s_stride, threshold, distance, number, _ptr(idx_dev), _ptr(counts_dev), stream))


def gather_median_device(v_dev, m, bins, v_stride, idx_dev, counts_dev, rows, number, u_dev, u_stride, stream=None):
    """the median over the selected frames alone.  Asynchronous on `stream`."""
    _ck(load().zen_hip_repsim_gather_median_device(_ptr(v_dev), m, bins, v_stride, _ptr(idx_dev), _ptr(counts_dev), rows, number, _ptr(u_dev),
                                                   u_stride, stream))


class Repsim(_addon.Handle):
    """zen_hip_repsim_t: n_clips clips of up to max_samples samples per call, each separated on its own"""
    _lib = _lib

    def __init__(self, fs, nfft=2048, n_clips=1, max_samples=1 << 20, threshold=None, distance_s=None, number=None, highpass_hz=None):
        self._create(fs, nfft, n_clips, max_samples)
        self.fs, self.nfft, self.hop, self.n_clips, self.max_samples = fs, nfft, nfft // 2, n_clips, max_samples
        self.number = NUMBER
        if any(v is not None for v in (threshold, distance_s, number, highpass_hz)):
            self.set_params(THRESHOLD if threshold is None else threshold, DISTANCE if distance_s is None else distance_s,
                            NUMBER if number is None else number, HIGHPASS if highpass_hz is None else highpass_hz)

    def set_params(self, threshold=THRESHOLD, distance_s=DISTANCE, number=NUMBER, highpass_hz=HIGHPASS):
        _ck(self._L.zen_hip_repsim_set_params(self._h, threshold, distance_s, number, highpass_hz))
        self.number = number

    def separate_device(self, in_dev, in_stride, n, background=None, foreground=None, out_stride=0, counts=None, indices=None):
        """DeviceBuffers or device addresses; counts: n_clips * m int32, indices: n_clips * m * number int32.  Asynchronous."""
        _ck(self._L.zen_hip_repsim_separate_device(self._h, _ptr(in_dev), in_stride, n, _ptr(background), _ptr(foreground), out_stride, _ptr(counts),
                                                   _ptr(indices)))

    def run(self, x, background=True, foreground=True, selection=False):
        """x: float32, (n,) for one clip or (n_clips, n).  Returns (background, foreground[, counts, indices]); an output that
        was not asked for is None; counts is (n_clips, m) and indices (n_clips, m, number) int32, -1 behind a frame's count.
        Synchronous."""
        x, one = _addon.clips(x, self.n_clips)
        pick = _addon.pick(one)
        n = x.shape[1]
        m = n_frames(n, self.nfft)
        bg = np.empty_like(x) if background else None
        fg = np.empty_like(x) if foreground else None
        cnt = np.empty((self.n_clips, m), np.int32) if selection else None
        idx = np.empty((self.n_clips, m, self.number), np.int32) if selection else None
        _ck(self._L.zen_hip_repsim_separate_host(self._h, x.ctypes.data, n, n, bg.ctypes.data if background else None,
                                                 fg.ctypes.data if foreground else None, n, cnt.ctypes.data if selection else None,
                                                 idx.ctypes.data if selection else None))
        res = (pick(bg), pick(fg))
        return res + (pick(cnt), pick(idx)) if selection else res


def separate(x, fs, nfft=2048, threshold=THRESHOLD, distance_s=DISTANCE, number=NUMBER, highpass_hz=HIGHPASS):
    """(background, foreground) of one clip of float32 samples: for every frame the median over its `number` most similar
    frames (similarity above `threshold`, at least `distance_s` seconds apart) is the repeating background's share of it."""
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    rs = Repsim(fs, nfft, 1, x.size, threshold, distance_s, number, highpass_hz)
    return rs.run(x)
