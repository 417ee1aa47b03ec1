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

KERNELS = ("frame", "fft", "magnitude", "similarity_mfma", "similarity_valu", "select", "gather_median", "mask", "ifft", "overlap_add")
TABLE_WINDOW, TABLE_DIVISOR = range(2)
ROUTE_DEFAULT, ROUTE_MFMA, ROUTE_VALU = range(3)
MAX_NEIGHBOURS, MAX_FRAMES, REGISTER_NEIGHBOURS = 256, 16384, 32
THRESHOLD, DISTANCE, NUMBER, HIGHPASS = 0.0, 1.0, 100, 100.0


class Stats(C.Structure):
    _fields_ = [("calls", C.c_ulonglong), ("clips", C.c_ulonglong), ("bands", C.c_ulonglong), ("device_bytes", C.c_ulonglong),
                ("allocations", C.c_ulonglong)]


# every symbol zen_amd/repsim/zen_hip_repsim.h declares: (name, restype, argtypes)
_vp, _sz, _i, _f, _d = C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_double
_pd, _pull = C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)
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


def load():
    """Load libzen_hip_repsim.so, building it first where it is absent (_addon.load).  Raises if that fails."""
    return _addon.load("repsim", SYMBOLS)


def _ck(rc):
    _addon.check(rc, load().zen_hip_repsim_last_error)


def _ptr(b):
    """a DeviceBuffer, a raw device address or None"""
    return getattr(b, "ptr", b)


def n_frames(n, nfft):
    return -(-n // (nfft // 2)) + 1


def table(nfft, which):
    """the window (nfft values) or the overlap divisor (nfft / 2 values) as a float32 array; needs no device"""
    out = np.empty(nfft if which == TABLE_WINDOW else nfft // 2, np.float32)
    _ck(load().zen_hip_repsim_table(nfft, which, out.ctypes.data, out.size))
    return out


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


class Repsim:
    """zen_hip_repsim_t: n_clips clips of up to max_samples samples per call, each separated on its own"""

    def __init__(self, fs, nfft=2048, n_clips=1, max_samples=1 << 20, threshold=None, distance_s=None, number=None, highpass_hz=None):
        h = C.c_void_p()
        _ck(load().zen_hip_repsim_create(fs, nfft, n_clips, max_samples, C.byref(h)))
        self._h = h.value
        self.fs, self.nfft, self.hop, self.n_clips, self.max_samples = fs, nfft, nfft // 2, n_clips, max_samples
        self.number = NUMBER
        if any(v is not None for v in (threshold, distance_s, number, highpass_hz)):
            self.set_params(THRESHOLD if threshold is None else threshold, DISTANCE if distance_s is None else distance_s,
                            NUMBER if number is None else number, HIGHPASS if highpass_hz is None else highpass_hz)

    def __del__(self):
        if getattr(self, "_h", None):
            load().zen_hip_repsim_destroy(self._h)
            self._h = None

    def set_stream(self, stream):
        _ck(load().zen_hip_repsim_set_stream(self._h, stream))

    def set_params(self, threshold=THRESHOLD, distance_s=DISTANCE, number=NUMBER, highpass_hz=HIGHPASS):
        _ck(load().zen_hip_repsim_set_params(self._h, threshold, distance_s, number, highpass_hz))
        self.number = number

    def stats(self):
        st = Stats()
        _ck(load().zen_hip_repsim_stats(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in Stats._fields_}

    def separate_device(self, in_dev, in_stride, n, background=None, foreground=None, out_stride=0, counts=None, indices=None):
        """DeviceBuffers or device addresses; counts: n_clips * m int32, indices: n_clips * m * number int32.  Asynchronous."""
        _ck(load().zen_hip_repsim_separate_device(self._h, _ptr(in_dev), in_stride, n, _ptr(background), _ptr(foreground), out_stride, _ptr(counts),
                                                  _ptr(indices)))

    def run(self, x, background=True, foreground=True, selection=False):
        """x: float32, (n,) for one clip or (n_clips, n).  Returns (background, foreground[, counts, indices]); an output that
        was not asked for is None; counts is (n_clips, m) and indices (n_clips, m, number) int32, -1 behind a frame's count.
        Synchronous."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        one = x.ndim == 1
        x = x.reshape(self.n_clips, -1)
        n = x.shape[1]
        m = n_frames(n, self.nfft)
        bg = np.empty_like(x) if background else None
        fg = np.empty_like(x) if foreground else None
        cnt = np.empty((self.n_clips, m), np.int32) if selection else None
        idx = np.empty((self.n_clips, m, self.number), np.int32) if selection else None
        _ck(load().zen_hip_repsim_separate_host(self._h, x.ctypes.data, n, n, bg.ctypes.data if background else None,
                                                fg.ctypes.data if foreground else None, n, cnt.ctypes.data if selection else None,
                                                idx.ctypes.data if selection else None))
        pick = (lambda a: None if a is None else a[0]) if one else (lambda a: a)
        res = (pick(bg), pick(fg))
        return res + (pick(cnt), pick(idx)) if selection else res

    def profile(self, enable=True):
        _ck(load().zen_hip_repsim_profile(self._h, int(bool(enable))))

    def profile_get(self):
        """{kernel: {"ms", "bytes", "launches"}} since the last call; synchronises."""
        return _addon.profile_get(_ck, load().zen_hip_repsim_profile_get, self._h, KERNELS)


def separate(x, fs, nfft=2048, threshold=THRESHOLD, distance_s=DISTANCE, number=NUMBER, highpass_hz=HIGHPASS):
    """(background, foreground) of one clip of float32 samples: for every frame the median over its `number` most similar
    frames (similarity above `threshold`, at least `distance_s` seconds apart) is the repeating background's share of it."""
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    rs = Repsim(fs, nfft, 1, x.size, threshold, distance_s, number, highpass_hz)
    return rs.run(x)
