"""ctypes binding of libzen_hip_repet.so (zen_amd/repet/zen_hip_repet.h): REPET, the repeating background of a recording
against its foreground, on the device.  No fallback: a missing library raises.

    background, foreground, period_s = repet.separate(x, 44100.0)           # float32 samples; the period is found
    rp = repet.Repet(44100.0, 2048, n_clips=2, max_samples=n)                 # a session: several clips per call
    bg, fg, periods = rp.run(clips)                                           # periods in frames of nfft / 2
"""
import ctypes as C

import numpy as np

from . import _addon
from ._addon import _d, _f, _i, _pd, _psz, _pull, _sz, _vp

KERNELS = ("frame", "fft", "magnitude", "lag_rows", "lag_fft", "power", "braw", "median", "mask", "ifft", "overlap_add")
TABLE_WINDOW, TABLE_DIVISOR = range(2)
MAX_SEGMENTS, MAX_FRAMES, REGISTER_SEGMENTS = 256, 16384, 32


class Stats(C.Structure):
    _fields_ = [("calls", C.c_ulonglong), ("clips", C.c_ulonglong), ("searches", C.c_ulonglong), ("device_bytes", C.c_ulonglong),
                ("allocations", C.c_ulonglong)]


# every symbol zen_amd/repet/zen_hip_repet.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("zen_hip_repet_last_error", C.c_char_p, []),
    ("zen_hip_repet_version", C.c_char_p, []),
    ("zen_hip_repet_create", _i, [_f, _sz, _sz, _sz, C.POINTER(_vp)]),
    ("zen_hip_repet_destroy", _i, [_vp]),
    ("zen_hip_repet_set_stream", _i, [_vp, _vp]),
    ("zen_hip_repet_set_params", _i, [_vp, _d, _d, _d]),
    ("zen_hip_repet_separate_device", _i, [_vp, _vp, _sz, _sz, _psz, _vp, _vp, _sz, _psz, _vp, _sz]),
    ("zen_hip_repet_separate_host", _i, [_vp, _vp, _sz, _sz, _psz, _vp, _vp, _sz, _psz, _vp, _sz]),
    ("zen_hip_repet_beat_spectrum_device", _i, [_vp, _vp, _sz, _sz, _vp, _sz]),
    ("zen_hip_repet_segment_median_device", _i, [_vp, _sz, _sz, _sz, _sz, _vp, _sz, _vp]),
    ("zen_hip_repet_stats", _i, [_vp, C.POINTER(Stats)]),
    ("zen_hip_repet_profile", _i, [_vp, _i]),
    ("zen_hip_repet_profile_get", _i, [_vp, _pd, _pull, _pull]),
    ("zen_hip_repet_find_period", _i, [_vp, _sz, _sz, _sz, _psz, _pd]),
    ("zen_hip_repet_table", _i, [_sz, _i, _vp, _sz]),
]

_lib = _addon.Library("repet", SYMBOLS, kernels=KERNELS, stats=Stats)
load, _ck, _ptr = _lib.load, _lib.check, _addon.ptr
n_frames, table = _addon.n_frames, _lib.stft_table


def find_period(braw, jmin, jmax):
    """(period in frames, its score) of a beat spectrum, (0, 0.0) where there is none; on the host, needs no device"""
    braw = np.ascontiguousarray(braw, np.float32)
    p, score = C.c_size_t(), C.c_double()
    _ck(load().zen_hip_repet_find_period(braw.ctypes.data if braw.size else None, braw.size, jmin, jmax, C.byref(p), C.byref(score)))
    return p.value, score.value


def segment_median_device(v_dev, m, bins, v_stride, period, s_dev, s_stride, stream=None):
    """the strided median alone on device memory: DeviceBuffers or device addresses.  Asynchronous on `stream`."""
    _ck(load().zen_hip_repet_segment_median_device(_ptr(v_dev), m, bins, v_stride, period, _ptr(s_dev), s_stride, stream))


class Repet(_addon.Handle):
    """zen_hip_repet_t: n_clips clips of up to max_samples samples per call, each with a period of its own"""
    _lib = _lib

    def __init__(self, fs, nfft=2048, n_clips=1, max_samples=1 << 20, tmin_s=None, tmax_s=None, highpass_hz=None):
        self._create(fs, nfft, n_clips, max_samples)
        self.fs, self.nfft, self.hop, self.n_clips, self.max_samples = fs, nfft, nfft // 2, n_clips, max_samples
        if tmin_s is not None or tmax_s is not None or highpass_hz is not None:
            self.set_params(0.8 if tmin_s is None else tmin_s, 8.0 if tmax_s is None else tmax_s, 100.0 if highpass_hz is None else highpass_hz)

    def set_params(self, tmin_s=0.8, tmax_s=8.0, highpass_hz=100.0):
        _ck(self._L.zen_hip_repet_set_params(self._h, tmin_s, tmax_s, highpass_hz))

    def _periods(self, periods):
        if periods is None:
            return None
        p = [int(v) for v in np.atleast_1d(periods)]
        assert len(p) == self.n_clips
        return (C.c_size_t * self.n_clips)(*p)

    def separate_device(self, in_dev, in_stride, n, periods=None, background=None, foreground=None, out_stride=0, braw=False):
        """DeviceBuffers or device addresses.  Returns the periods used (frames) and, with braw, the (n_clips, m) beat spectra
        of the clips whose period was found (rows of NaN for the others).  Waits only where a period is found."""
        used = (C.c_size_t * self.n_clips)()
        m = n_frames(n, self.nfft)
        b = np.full((self.n_clips, m), np.nan, np.float32) if braw else None
        _ck(self._L.zen_hip_repet_separate_device(self._h, _ptr(in_dev), in_stride, n, self._periods(periods), _ptr(background), _ptr(foreground),
                                                  out_stride, used, b.ctypes.data if braw else None, m))
        return (list(used), b) if braw else list(used)

    def beat_spectrum_device(self, in_dev, in_stride, n, braw_dev, braw_stride):
        _ck(self._L.zen_hip_repet_beat_spectrum_device(self._h, _ptr(in_dev), in_stride, n, _ptr(braw_dev), braw_stride))

    def run(self, x, periods=None, background=True, foreground=True, braw=False):
        """x: float32, (n,) for one clip or (n_clips, n).  Returns (background, foreground, periods used in frames[, braw]); an
        output that was not asked for is None.  Synchronous."""
        x, one = _addon.clips(x, self.n_clips)
        pick = _addon.pick(one)
        n = x.shape[1]
        m = n_frames(n, self.nfft)
        bg = np.empty_like(x) if background else None
        fg = np.empty_like(x) if foreground else None
        b = np.full((self.n_clips, m), np.nan, np.float32) if braw else None
        used = (C.c_size_t * self.n_clips)()
        _ck(self._L.zen_hip_repet_separate_host(self._h, x.ctypes.data, n, n, self._periods(periods), bg.ctypes.data if background else None,
                                                fg.ctypes.data if foreground else None, n, used, b.ctypes.data if braw else None, m))
        res = (pick(bg), pick(fg), list(used))
        return res + (pick(b),) if braw else res


def separate(x, fs, nfft=2048, period_s=None, highpass_hz=100.0):
    """(background, foreground, period in seconds) of one clip of float32 samples; period_s: the period of the accompaniment
    where it is known (rounded to whole frames of nfft / 2), None to find it.  A period of 0.0 comes back where none was found:
    the background is silence and the foreground is x."""
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    hop = nfft // 2
    rp = Repet(fs, nfft, 1, x.size, highpass_hz=highpass_hz)
    periods = None if period_s is None else [max(1, int(round(period_s * fs / hop)))]
    bg, fg, used = rp.run(x, periods)
    return bg, fg, used[0] * hop / float(fs)
