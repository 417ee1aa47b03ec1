"""ctypes binding of libzen_hip_tsm.so (zen_amd/tsm/zen_hip_tsm.h): time-scale modification on the device -- the harmonic
stem through a phase-locked phase vocoder, the percussive stem and the residual through overlap-add on short frames, and
their sum.  No fallback: a missing library raises.

    ts = tsm.Tsm(44100.0, 4096, 256, max_samples=n)
    y = ts.hp(harm, perc, 1.5, resid)                                  # float32 rows -> floor(n * 1.5) samples each
    hp_out, pv_only = tsm.stretch_hpr(x, 44100.0, 1.5)                   # the separation in front, all on the device
"""
import ctypes as C
import math

import numpy as np

from . import _addon
from ._addon import _d, _f, _i, _pd, _psz, _pull, _sz, _vp
from . import lib as _zl

KERNELS = ("frame", "fft", "analysis", "peaks", "walk", "spectrum", "ifft", "overlap_add")
TABLE_WINDOW, TABLE_PV_DIVISOR, TABLE_OLA_DIVISOR, TABLE_COARSE, TABLE_FINE, TABLE_ATAN, TABLE_CONSTANTS = range(7)
MAX_FRAMES = 16384


class Stats(C.Structure):
    _fields_ = [("calls", C.c_ulonglong), ("clips", C.c_ulonglong), ("device_bytes", C.c_ulonglong), ("allocations", C.c_ulonglong)]


# every symbol zen_amd/tsm/zen_hip_tsm.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("zen_hip_tsm_last_error", C.c_char_p, []),
    ("zen_hip_tsm_version", C.c_char_p, []),
    ("zen_hip_tsm_create", _i, [_f, _sz, _sz, _sz, _sz, _d, C.POINTER(_vp)]),
    ("zen_hip_tsm_destroy", _i, [_vp]),
    ("zen_hip_tsm_set_stream", _i, [_vp, _vp]),
    ("zen_hip_tsm_stretch_pv_device", _i, [_vp, _vp, _sz, _sz, _d, _vp, _sz]),
    ("zen_hip_tsm_stretch_ola_device", _i, [_vp, _vp, _vp, _sz, _sz, _d, _vp, _sz]),
    ("zen_hip_tsm_stretch_hp_device", _i, [_vp, _vp, _vp, _vp, _sz, _sz, _d, _vp, _sz]),
    ("zen_hip_tsm_stretch_hp_host", _i, [_vp, _vp, _vp, _vp, _sz, _sz, _d, _vp, _sz]),
    ("zen_hip_tsm_inspect_device", _i, [_vp, _vp, _sz, _sz, _d, _vp, _vp, _vp, _vp]),
    ("zen_hip_tsm_phase_device", _i, [_vp, _sz, _vp, _vp]),
    ("zen_hip_tsm_cs_device", _i, [_vp, _sz, _vp, _vp]),
    ("zen_hip_tsm_stats", _i, [_vp, C.POINTER(Stats)]),
    ("zen_hip_tsm_profile", _i, [_vp, _i]),
    ("zen_hip_tsm_profile_get", _i, [_vp, _pd, _pull, _pull]),
    ("zen_hip_tsm_positions", _i, [_sz, _sz, _sz, _d, _psz, _psz, _vp, _sz]),
    ("zen_hip_tsm_table", _i, [_sz, _i, _vp, _sz]),
]

_lib = _addon.Library("tsm", SYMBOLS, kernels=KERNELS, stats=Stats)
load, _ck, _ptr = _lib.load, _lib.check, _addon.ptr


def n_out(n, alpha):
    return int(math.floor(float(n) * alpha))


def longest_clip(nfft, nfft_ola, max_alpha):
    """the most samples per clip a handle of these frames takes at max_alpha: its output makes at most 16384 frames on either route"""
    return int(min((MAX_FRAMES - 4) * (nfft // 4), (MAX_FRAMES - 2) * (nfft_ola // 2)) / max_alpha)


def table(nfft, which):
    """One host table; needs no device.  The window and the two divisors as float32 arrays, the cosine / sine tables as
    (2048, 2) float32 arrays, the arctangent table as a uint32 array, the constants (c3, K) as two float32 values."""
    length = {TABLE_WINDOW: nfft, TABLE_PV_DIVISOR: nfft // 4, TABLE_OLA_DIVISOR: nfft // 2, TABLE_COARSE: 4096, TABLE_FINE: 4096,
              TABLE_ATAN: 257, TABLE_CONSTANTS: 2}.get(which, 1)
    out = np.empty(max(length, 1), np.uint32 if which == TABLE_ATAN else np.float32)
    _ck(load().zen_hip_tsm_table(nfft, which, out.ctypes.data, out.size))
    return out.reshape(-1, 2) if which in (TABLE_COARSE, TABLE_FINE) else out


def positions(n, frame, overlap, alpha):
    """(n_out, M, the M analysis positions as an int64 array) of either route; on the host, needs no device"""
    no, m = C.c_size_t(), C.c_size_t()
    _ck(load().zen_hip_tsm_positions(n, frame, overlap, alpha, C.byref(no), C.byref(m), None, 0))
    a = np.empty(m.value, np.int64)
    _ck(load().zen_hip_tsm_positions(n, frame, overlap, alpha, C.byref(no), C.byref(m), a.ctypes.data, a.size))
    return no.value, m.value, a


def phase_device(re_im_dev, count, theta_dev, stream=None):
    """atan2turns alone on device memory: DeviceBuffers or device addresses.  Asynchronous on `stream`."""
    _ck(load().zen_hip_tsm_phase_device(_ptr(re_im_dev), count, _ptr(theta_dev), stream))


def cs_device(psi_dev, count, cos_sin_dev, stream=None):
    _ck(load().zen_hip_tsm_cs_device(_ptr(psi_dev), count, _ptr(cos_sin_dev), stream))


def phase(re, im):
    """the u32 phases of (re, im) pairs, through the device.  Synchronous."""
    z = np.stack([np.asarray(re, np.float32).ravel(), np.asarray(im, np.float32).ravel()], 1)
    d_in, d_out = _zl.DeviceBuffer.from_host(z), _zl.DeviceBuffer(max(z.shape[0], 1), np.uint32)
    phase_device(d_in, z.shape[0], d_out)
    _zl.synchronize()
    return d_out.download(z.shape[0])


def cs(psi):
    """(cos, sin) of u32 phases as two float32 arrays, through the device.  Synchronous."""
    psi = np.ascontiguousarray(psi, np.uint32).ravel()
    d_in, d_out = _zl.DeviceBuffer.from_host(psi), _zl.DeviceBuffer(max(2 * psi.size, 1))
    cs_device(d_in, psi.size, d_out)
    _zl.synchronize()
    got = d_out.download(2 * psi.size).reshape(-1, 2)
    return got[:, 0].copy(), got[:, 1].copy()


class Tsm(_addon.Handle):
    """zen_hip_tsm_t: n_clips clips of up to max_samples samples per call, stretched alike by up to max_alpha"""
    _lib = _lib

    def __init__(self, fs, nfft=4096, nfft_ola=256, n_clips=1, max_samples=None, max_alpha=4.0):
        """max_samples None: longest_clip(nfft, nfft_ola, max_alpha), 11.9 s at 44.1 kHz with the defaults"""
        if max_samples is None:
            max_samples = longest_clip(nfft, nfft_ola, max_alpha)
        self._create(fs, nfft, nfft_ola, n_clips, max_samples, max_alpha)
        self.fs, self.nfft, self.nfft_ola, self.n_clips, self.max_samples, self.max_alpha = fs, nfft, nfft_ola, n_clips, max_samples, max_alpha

    def frames(self, n, alpha):
        return (n_out(n, alpha) - 1) // (self.nfft // 4) + 4

    # device rows: DeviceBuffers or device addresses; asynchronous on the handle's stream
    def pv_device(self, in_dev, in_stride, n, alpha, out_dev, out_stride):
        _ck(self._L.zen_hip_tsm_stretch_pv_device(self._h, _ptr(in_dev), in_stride, n, alpha, _ptr(out_dev), out_stride))

    def ola_device(self, perc_dev, resid_dev, in_stride, n, alpha, out_dev, out_stride):
        _ck(self._L.zen_hip_tsm_stretch_ola_device(self._h, _ptr(perc_dev), _ptr(resid_dev), in_stride, n, alpha, _ptr(out_dev), out_stride))

    def hp_device(self, harm_dev, perc_dev, resid_dev, in_stride, n, alpha, out_dev, out_stride):
        _ck(self._L.zen_hip_tsm_stretch_hp_device(self._h, _ptr(harm_dev), _ptr(perc_dev), _ptr(resid_dev), in_stride, n, alpha, _ptr(out_dev),
                                                  out_stride))

    def inspect_device(self, in_dev, in_stride, n, alpha, mag=None, theta=None, owner=None, psi=None):
        _ck(self._L.zen_hip_tsm_inspect_device(self._h, _ptr(in_dev), in_stride, n, alpha, _ptr(mag), _ptr(theta), _ptr(owner), _ptr(psi)))

    # host rows: float32, (n,) for one clip or (n_clips, n); synchronous
    def _rows(self, x):
        x, one = _addon.clips(x, self.n_clips)
        return one, x

    def _through_device(self, alpha, call, *stems):
        one, first = self._rows(stems[0])
        n = first.shape[1]
        no = n_out(n, alpha)
        bufs = [None if s is None else _zl.DeviceBuffer.from_host(self._rows(s)[1]) for s in stems]
        out = _zl.DeviceBuffer(max(self.n_clips * no, 1))
        call(*bufs, n, n, alpha, out, no)
        _zl.synchronize()
        y = out.download(self.n_clips * no).reshape(self.n_clips, no)
        return y[0] if one else y

    def pv(self, x, alpha):
        """the vocoder alone: floor(n alpha) samples per clip"""
        return self._through_device(alpha, self.pv_device, x)

    def ola(self, perc, alpha, resid=None):
        """overlap-add alone, of perc (+ resid)"""
        return self._through_device(alpha, self.ola_device, perc, resid)

    def hp(self, harm, perc, alpha, resid=None):
        """pv(harm) + ola(perc (+ resid)) through zen_hip_tsm_stretch_hp_host"""
        one, harm = self._rows(harm)
        perc = self._rows(perc)[1]
        resid = None if resid is None else self._rows(resid)[1]
        n = harm.shape[1]
        assert perc.shape == harm.shape and (resid is None or resid.shape == harm.shape)
        no = n_out(n, alpha)
        out = np.empty((self.n_clips, max(no, 0)), np.float32)
        _ck(self._L.zen_hip_tsm_stretch_hp_host(self._h, harm.ctypes.data, perc.ctypes.data, None if resid is None else resid.ctypes.data, n, n, alpha,
                                                out.ctypes.data, no))
        return out[0] if one else out

    def inspect(self, x, alpha):
        """(mag, theta, owner, psi) of steps 2-4, each (n_clips, M, nfft / 2 + 1) -- (M, nfft / 2 + 1) for a one-dimensional x"""
        one, x = self._rows(x)
        n = x.shape[1]
        shape = (self.n_clips, self.frames(n, alpha), self.nfft // 2 + 1)
        cnt = shape[0] * shape[1] * shape[2]
        outs = [_zl.DeviceBuffer(cnt, t) for t in (np.float32, np.uint32, np.uint16, np.uint32)]
        self.inspect_device(_zl.DeviceBuffer.from_host(x), n, n, alpha, *outs)
        _zl.synchronize()
        got = tuple(o.download().reshape(shape) for o in outs)
        return tuple(g[0] for g in got) if one else got


def stretch_hpr(x, fs, alpha, hpr_hop=1024, beta=2.5, nfft=4096, nfft_ola=256):
    """(hp_out, pv_only_out) of one clip of float32 samples, each floor(n alpha) samples, n the length of x padded with zeros to
    a multiple of hpr_hop: one zen_hip_hpr_process call at hop hpr_hop (causal, all three outputs) writes the harmonic, the
    percussive and the residual stream into device memory; the harmonic one goes through the vocoder and the other two through
    overlap-add there (hp_out), and the mixture through the vocoder alone (pv_only_out), so the difference can be heard and
    measured."""
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    n = -(-x.size // hpr_hop) * hpr_hop
    if n == 0:
        return np.empty(0, np.float32), np.empty(0, np.float32)
    xp = np.zeros(n, np.float32)
    xp[:x.size] = x
    no = n_out(n, alpha)
    flags = _zl.OUTPUT_HARMONIC | _zl.OUTPUT_PERCUSSIVE | _zl.OUTPUT_RESIDUAL
    hpr = _zl.HPR(fs, hpr_hop, beta, flags, _zl.TIME_CAUSAL)
    ts = Tsm(fs, nfft, nfft_ola, 1, n, alpha)
    rows = _zl.DeviceBuffer(4 * n)                      # the samples, harm, perc, resid
    out = _zl.DeviceBuffer(2 * no)
    rows.upload(xp)
    hpr.process(rows.ptr, n // hpr_hop, in_stride=n, harm=rows.offset(n), perc=rows.offset(2 * n), resid=rows.offset(3 * n), out_stride=n)
    ts.hp_device(rows.offset(n), rows.offset(2 * n), rows.offset(3 * n), n, n, alpha, out, no)
    ts.pv_device(rows, n, n, alpha, out.offset(no), no)
    _zl.synchronize()
    got = out.download()
    return got[:no].copy(), got[no:].copy()
