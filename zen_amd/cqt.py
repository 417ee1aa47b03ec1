"""ctypes binding of libzen_hip_cqt.so (zen_amd/cqt/zen_hip_cqt.h): an invertible constant-Q transform (a sliced
non-stationary Gabor transform) and the harmonic / percussive / residual separation in its domain, on the device.  No
fallback: a missing library raises.

    harm, perc, resid = cqt.separate(x, 44100.0)                              # float32 samples, one clip
    cq = cqt.Cqt(44100.0, 16384, 12, 60.0, n_clips=2, n_samples=n)            # a session: clips of one length per call
    c = cq.forward(clips); V = cq.spectrogram(clips); y = cq.inverse(c)       # (2, ns, nb, M) complex64, (2, T, nb), (2, n)
"""
import ctypes as C

import numpy as np

from . import _addon
from ._addon import _d, _f, _i, _pd, _psz, _pull, _sz, _vp
from . import lib as _zl

KERNELS = ("slice", "slice_fft", "fold", "band_ifft", "overlap", "median_time", "median_freq", "mask", "band_fft", "gather", "slice_ifft",
           "overlap_add")
TABLE_KB, TABLE_GL, TABLE_GU, TABLE_GDL, TABLE_GDU, TABLE_H, TABLE_S = range(7)
MAX_SLICES, MAX_BANDS_PER_OCTAVE = 4096, 96


class Stats(C.Structure):
    _fields_ = [("calls", C.c_ulonglong), ("clips", C.c_ulonglong), ("device_bytes", C.c_ulonglong), ("allocations", C.c_ulonglong)]


class Shape(C.Structure):
    _fields_ = [("slices", C.c_size_t), ("bands", C.c_size_t), ("m", C.c_size_t), ("columns", C.c_size_t), ("run", C.c_size_t),
                ("lh", C.c_size_t), ("lp", C.c_size_t)]


# every symbol zen_amd/cqt/zen_hip_cqt.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("zen_hip_cqt_last_error", C.c_char_p, []),
    ("zen_hip_cqt_version", C.c_char_p, []),
    ("zen_hip_cqt_plan", _i, [_f, _sz, _i, _d, _psz, _psz, _vp, _sz]),
    ("zen_hip_cqt_table", _i, [_f, _sz, _i, _d, _i, _vp, _sz]),
    ("zen_hip_cqt_create", _i, [_f, _sz, _i, _d, _sz, _sz, C.POINTER(_vp)]),
    ("zen_hip_cqt_destroy", _i, [_vp]),
    ("zen_hip_cqt_set_stream", _i, [_vp, _vp]),
    ("zen_hip_cqt_set_params", _i, [_vp, _f, _i, _i, _i]),
    ("zen_hip_cqt_shape", _i, [_vp, C.POINTER(Shape)]),
    ("zen_hip_cqt_stats", _i, [_vp, C.POINTER(Stats)]),
    ("zen_hip_cqt_forward_device", _i, [_vp, _vp, _sz, _vp]),
    ("zen_hip_cqt_spectrogram_device", _i, [_vp, _vp, _sz, _vp, _sz]),
    ("zen_hip_cqt_inverse_device", _i, [_vp, _vp, _vp, _sz]),
    ("zen_hip_cqt_separate_device", _i, [_vp, _vp, _sz, _vp, _vp, _vp, _sz]),
    ("zen_hip_cqt_separate_host", _i, [_vp, _vp, _sz, _vp, _vp, _vp, _sz]),
    ("zen_hip_cqt_profile", _i, [_vp, _i]),
    ("zen_hip_cqt_profile_get", _i, [_vp, _pd, _pull, _pull]),
]

_lib = _addon.Library("cqt", SYMBOLS, (1,), KERNELS, Stats)
load, _ck, _ptr = _lib.load, _lib.check, _addon.ptr      # code 1, ZEN_HIP_E_FILTER_TOO_BIG, is the reference's exception


def plan(fs, slice_len, bands_per_octave, fmin):
    """(nb, M, centres): the bands of the plan, the coefficients per band and slice, the band centres in bins; needs no device"""
    nb, m = C.c_size_t(), C.c_size_t()
    _ck(load().zen_hip_cqt_plan(fs, slice_len, bands_per_octave, fmin, C.byref(nb), C.byref(m), None, 0))
    p = np.empty(nb.value, np.int32)
    _ck(load().zen_hip_cqt_plan(fs, slice_len, bands_per_octave, fmin, None, None, p.ctypes.data, p.size))
    return nb.value, m.value, p


def table(fs, slice_len, bands_per_octave, fmin, which):
    """one host table of the plan: TABLE_KB as int32, the others as float32; needs no device"""
    out = np.empty(slice_len if which >= TABLE_H else slice_len // 2 + 1, np.int32 if which == TABLE_KB else np.float32)
    _ck(load().zen_hip_cqt_table(fs, slice_len, bands_per_octave, fmin, which, out.ctypes.data, out.size))
    return out


class Cqt(_addon.Handle):
    """zen_hip_cqt_t: n_clips clips of exactly n_samples samples per call"""
    _lib = _lib

    def __init__(self, fs, slice_len=16384, bands_per_octave=12, fmin=60.0, n_clips=1, n_samples=1 << 20, beta=0.0, soft=False, lh=0, lp=0):
        self._create(fs, slice_len, bands_per_octave, fmin, n_clips, n_samples)
        self.fs, self.slice_len, self.n_clips, self.n_samples = fs, slice_len, n_clips, n_samples
        if beta or soft or lh or lp:
            self.set_params(beta, soft, lh, lp)
        sh = self.shape()
        self.n_slices, self.n_bands, self.m, self.columns = sh["slices"], sh["bands"], sh["m"], sh["columns"]

    def set_params(self, beta=0.0, soft=False, lh=0, lp=0):
        """0 stands for the default: beta 2, 0.2 s of columns, one octave of bands"""
        _ck(self._L.zen_hip_cqt_set_params(self._h, beta, int(bool(soft)), lh, lp))

    def shape(self):
        sh = Shape()
        _ck(self._L.zen_hip_cqt_shape(self._h, C.byref(sh)))
        return _addon.as_dict(sh)

    # ---- device memory: DeviceBuffers or device addresses; asynchronous on the handle's stream
    def forward_device(self, in_dev, in_stride, coef_dev):
        _ck(self._L.zen_hip_cqt_forward_device(self._h, _ptr(in_dev), in_stride, _ptr(coef_dev)))

    def spectrogram_device(self, in_dev, in_stride, v_dev, v_stride):
        _ck(self._L.zen_hip_cqt_spectrogram_device(self._h, _ptr(in_dev), in_stride, _ptr(v_dev), v_stride))

    def inverse_device(self, coef_dev, out_dev, out_stride):
        _ck(self._L.zen_hip_cqt_inverse_device(self._h, _ptr(coef_dev), _ptr(out_dev), out_stride))

    def separate_device(self, in_dev, in_stride, harmonic=None, percussive=None, residual=None, out_stride=0):
        _ck(self._L.zen_hip_cqt_separate_device(self._h, _ptr(in_dev), in_stride, _ptr(harmonic), _ptr(percussive), _ptr(residual), out_stride))

    # ---- host arrays; synchronous
    def _clips(self, x):
        x, one = _addon.clips(x, self.n_clips)
        assert x.shape[1] == self.n_samples, "the session takes clips of %d samples" % self.n_samples
        return x, _addon.pick(one)

    def forward(self, x):
        """x: float32, (n,) for one clip or (n_clips, n).  The coefficients, (ns, nb, M) or (n_clips, ns, nb, M) complex64."""
        x, pick = self._clips(x)
        d_in = _zl.DeviceBuffer.from_host(x)
        d_c = _zl.DeviceBuffer(self.n_clips * self.n_slices * self.n_bands * self.m, np.complex64)
        self.forward_device(d_in, self.n_samples, d_c)
        _zl.synchronize()
        return pick(d_c.download().reshape(self.n_clips, self.n_slices, self.n_bands, self.m))

    def spectrogram(self, x):
        """the magnitudes V, (T, nb) or (n_clips, T, nb) float32"""
        x, pick = self._clips(x)
        d_in = _zl.DeviceBuffer.from_host(x)
        d_v = _zl.DeviceBuffer(self.n_clips * self.columns * self.n_bands)
        self.spectrogram_device(d_in, self.n_samples, d_v, self.n_bands)
        _zl.synchronize()
        return pick(d_v.download().reshape(self.n_clips, self.columns, self.n_bands))

    def inverse(self, c):
        """the samples back from coefficients shaped as forward returns them"""
        c = np.ascontiguousarray(c, dtype=np.complex64)
        one = c.ndim == 3
        assert c.size == self.n_clips * self.n_slices * self.n_bands * self.m
        d_c = _zl.DeviceBuffer.from_host(c)
        d_out = _zl.DeviceBuffer(self.n_clips * self.n_samples)
        self.inverse_device(d_c, d_out, self.n_samples)
        _zl.synchronize()
        y = d_out.download().reshape(self.n_clips, self.n_samples)
        return y[0] if one else y

    def separate(self, x, harmonic=True, percussive=True, residual=True):
        """(harmonic, percussive, residual) of x, (n,) or (n_clips, n) float32; a stem that was not asked for is None"""
        x, pick = self._clips(x)
        out = [np.empty_like(x) if w else None for w in (harmonic, percussive, residual)]
        _ck(self._L.zen_hip_cqt_separate_host(self._h, x.ctypes.data, self.n_samples, *(None if o is None else o.ctypes.data for o in out),
                                              self.n_samples))
        return tuple(pick(o) for o in out)


def separate(x, fs, slice_len=16384, bands_per_octave=12, fmin=60.0, beta=0.0, soft=False):
    """(harmonic, percussive, residual) of one clip of float32 samples"""
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    return Cqt(fs, slice_len, bands_per_octave, fmin, 1, x.size, beta=beta, soft=soft).separate(x)
