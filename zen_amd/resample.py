"""ctypes binding of libzen_hip_resample.so (zen_amd/resample/zen_hip_resample.h): band-limited sample-rate conversion of
device rows by a rational ratio, and with the time stretch of zen_amd/tsm in front the pitch shift.  No fallback: a missing
library raises.

    y = resample.convert(x, 48000, 44100)                              # float32 row(s) -> ceil(n * 147 / 160) samples each
    rs = resample.Resampler(147, 160, quality=16); y = rs.run(x)        # the same, the handle kept
    y = resample.shift_hpr(x, 44100.0, +3)                              # three semitones up, same length, all on the device
"""
import ctypes as C
import math

import numpy as np

from . import _addon
from ._addon import _d, _i, _pd, _psz, _pull, _sz, _vp
from . import lib as _zl

KERNELS = ("expand", "fir")
TILE, PHASES, MAX_TAPS, MAX_POLY, MAX_ROWS = 256, 512, 256, 4096, 65535
ROUTE_INTERP, ROUTE_POLY = 0, 1
QUALITIES = (8, 16, 32)


class Stats(C.Structure):
    _fields_ = [("calls", C.c_ulonglong), ("rows", C.c_ulonglong), ("outputs", C.c_ulonglong), ("poly_calls", C.c_ulonglong),
                ("interp_calls", C.c_ulonglong), ("device_bytes", C.c_ulonglong), ("allocations", C.c_ulonglong)]


# every symbol zen_amd/resample/zen_hip_resample.h declares: (name, restype, argtypes)
_ull = C.c_ulonglong
SYMBOLS = [
    ("zen_hip_resample_last_error", C.c_char_p, []),
    ("zen_hip_resample_version", C.c_char_p, []),
    ("zen_hip_resample_create", _i, [_ull, _ull, _i, C.POINTER(_vp)]),
    ("zen_hip_resample_destroy", _i, [_vp]),
    ("zen_hip_resample_set_stream", _i, [_vp, _vp]),
    ("zen_hip_resample_run_device", _i, [_vp, _vp, _sz, _ull, _sz, _ull, _ull, _sz, _vp, _sz, _sz]),
    ("zen_hip_resample_run_host", _i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz]),
    ("zen_hip_resample_stats", _i, [_vp, C.POINTER(Stats)]),
    ("zen_hip_resample_profile", _i, [_vp, _i]),
    ("zen_hip_resample_profile_get", _i, [_vp, _pd, _pull, _pull]),
    ("zen_hip_resample_n_out", _i, [_ull, _ull, _ull, _pull]),
    ("zen_hip_resample_span", _i, [_ull, _ull, _i, _ull, _ull, _ull, _pull, _pull]),
    ("zen_hip_resample_geometry", _i, [_ull, _ull, _i, _psz, _psz, C.POINTER(_i)]),
    ("zen_hip_resample_table", _i, [_ull, _ull, _i, _vp, _sz]),
    ("zen_hip_resample_ratio_for_shift", _i, [_d, _pull, _pull]),
]

_lib = _addon.Library("resample", SYMBOLS, kernels=KERNELS, stats=Stats)
load, _ck, _ptr = _lib.load, _lib.check, _addon.ptr


# ------------------------------------------------------------------------------------------------ host arithmetic, no device
def n_out(num, den, n_total):
    """ceil(n_total num / den)"""
    out = C.c_ulonglong()
    _ck(load().zen_hip_resample_n_out(num, den, n_total, C.byref(out)))
    return out.value


def span(num, den, quality, n_total, out_first, out_count):
    """(in_first, in_count): the window of the row that the outputs out_first .. out_first + out_count need"""
    a, b = C.c_ulonglong(), C.c_ulonglong()
    _ck(load().zen_hip_resample_span(num, den, quality, n_total, out_first, out_count, C.byref(a), C.byref(b)))
    return a.value, b.value


def geometry(num, den, quality):
    """(W, T, route)"""
    w, t, r = C.c_size_t(), C.c_size_t(), C.c_int()
    _ck(load().zen_hip_resample_geometry(num, den, quality, C.byref(w), C.byref(t), C.byref(r)))
    return w.value, t.value, r.value


def table(num, den, quality):
    """h, (513, T) float32"""
    T = geometry(num, den, quality)[1]
    out = np.empty((PHASES + 1, T), np.float32)
    _ck(load().zen_hip_resample_table(num, den, quality, out.ctypes.data, out.size))
    return out


def ratio_for_shift(semitones):
    """(num, den) of a pitch shift by `semitones`: num = llround(65536 / 2^(s / 12)) over 65536, reduced"""
    a, b = C.c_ulonglong(), C.c_ulonglong()
    _ck(load().zen_hip_resample_ratio_for_shift(float(semitones), C.byref(a), C.byref(b)))
    return a.value, b.value


def ratio_of_rates(fs_in, fs_out):
    """(num, den) = fs_out / fs_in for two whole-numbered rates"""
    a, b = int(round(fs_out)), int(round(fs_in))
    if a != fs_out or b != fs_in or a <= 0 or b <= 0:
        raise ValueError("sample rates must be positive whole numbers: %r -> %r" % (fs_in, fs_out))
    g = math.gcd(a, b)
    return a // g, b // g


# ------------------------------------------------------------------------------------------------ the handle
class Resampler(_addon.Handle):
    """zen_hip_resample_t: rows converted by num / den at one quality"""
    _lib = _lib

    def __init__(self, num, den, quality=16):
        self._create(num, den, quality)
        g = math.gcd(num, den)
        self.num, self.den, self.quality = num // g, den // g, quality
        self.W, self.T, _ = geometry(num, den, quality)

    def n_out(self, n_total):
        return n_out(self.num, self.den, n_total)

    def span(self, n_total, out_first, out_count):
        return span(self.num, self.den, self.quality, n_total, out_first, out_count)

    def run_device(self, in_dev, in_stride, in_first, in_count, n_total, out_first, out_count, out_dev, out_stride, n_rows=1):
        """device rows: DeviceBuffers or device addresses; asynchronous on the handle's stream"""
        _ck(self._L.zen_hip_resample_run_device(self._h, _ptr(in_dev), in_stride, in_first, in_count, n_total, out_first, out_count, _ptr(out_dev),
                                                out_stride, n_rows))

    def run(self, x):
        """host rows: float32, (n,) or (rows, n) -> (n_out,) or (rows, n_out), through zen_hip_resample_run_host; synchronous"""
        x = np.ascontiguousarray(x, dtype=np.float32)
        one = x.ndim == 1
        x = x.reshape(1, -1) if one else x
        rows, n = x.shape
        out = np.empty((rows, self.n_out(n)), np.float32)
        _ck(self._L.zen_hip_resample_run_host(self._h, x.ctypes.data, n, n, out.ctypes.data, out.shape[1], rows))
        return out[0] if one else out

    def pieces(self, x, cuts):
        """one host row made in pieces: the outputs cuts[k] .. cuts[k + 1] of every piece from the window span() names, each
        window uploaded and converted on its own, the pieces concatenated -- the bits of run(x).  Synchronous."""
        x = np.ascontiguousarray(x, dtype=np.float32).ravel()
        out = []
        for a, b in zip(cuts, cuts[1:]):
            if b <= a:
                continue
            lo, cnt = self.span(x.size, a, b - a)
            d_in, d_out = _zl.DeviceBuffer.from_host(x[lo:lo + cnt]), _zl.DeviceBuffer(b - a)
            self.run_device(d_in, cnt, lo, cnt, x.size, a, b - a, d_out, b - a)
            _zl.synchronize()
            out.append(d_out.download())
        return np.concatenate(out) if out else np.empty(0, np.float32)


def convert(x, fs_in, fs_out, quality=16):
    """float32 row(s) at fs_in -> the same at fs_out (whole-numbered rates, their ratio within 1/4..4)"""
    num, den = ratio_of_rates(fs_in, fs_out)
    return Resampler(num, den, quality).run(x)


# ------------------------------------------------------------------------------------------------ the pitch shift
def shift_plan(n, semitones):
    """(num, den, alpha, stretched, resampled) of n samples shifted by `semitones`: stretched by alpha = den / num into
    floor(n alpha) samples, brought back by num / den into ceil(. num / den), which is n - 3 .. n"""
    num, den = ratio_for_shift(semitones)
    alpha = float(den) / float(num)
    m = int(math.floor(float(n) * alpha))
    return num, den, alpha, m, (n_out(num, den, m) if m else 0)


def _shift_device(ts, rs, harm, perc, resid, stride, n, alpha, m, k, scratch, out):
    """stems on the device -> scratch (m samples, the stretch) -> out (k samples of n, the rest zeros)"""
    ts.hp_device(harm, perc, resid, stride, n, alpha, scratch, m)
    rs.run_device(scratch, m, 0, m, m, 0, k, out, n)


def shift(harm, perc, resid, fs, semitones, nfft=4096, nfft_ola=256, quality=16):
    """One clip's stems (float32 rows of n samples; resid may be None) at another pitch and the same length: the time stretch of
    zen_amd/tsm by alpha = den / num (the harmonic row through the vocoder, the others through overlap-add), then this
    library by num / den, device to device; the n - 3 .. n samples that gives are padded with zeros to n."""
    from . import tsm
    harm = np.ascontiguousarray(harm, np.float32).ravel()
    n = harm.size
    num, den, alpha, m, k = shift_plan(n, semitones)
    if n == 0 or m == 0:
        raise ValueError("a clip of %d samples leaves nothing to shift" % n)
    stems = [harm, np.ascontiguousarray(perc, np.float32).ravel(), None if resid is None else np.ascontiguousarray(resid, np.float32).ravel()]
    assert all(s is None or s.size == n for s in stems)
    ts = tsm.Tsm(fs, nfft, nfft_ola, 1, n, alpha)
    rs = Resampler(num, den, quality)
    bufs = [None if s is None else _zl.DeviceBuffer.from_host(s) for s in stems]
    scratch, out = _zl.DeviceBuffer(m), _zl.DeviceBuffer(n)
    out.zero()
    _shift_device(ts, rs, bufs[0], bufs[1], bufs[2], n, n, alpha, m, k, scratch, out)
    _zl.synchronize()
    return out.download()


def shift_hpr(x, fs, semitones, hpr_hop=1024, beta=2.5, nfft=4096, nfft_ola=256, quality=16):
    """One clip of float32 samples at another pitch, the causal separation in front as tsm.stretch_hpr has it: the clip padded
    with zeros to a multiple of hpr_hop (n samples), one zen_hip_hpr_process call writes the three stems into device memory,
    they are stretched and resampled there.  Returns n samples."""
    from . import tsm
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    n = -(-x.size // hpr_hop) * hpr_hop
    if n == 0:
        return np.empty(0, np.float32)
    xp = np.zeros(n, np.float32)
    xp[:x.size] = x
    num, den, alpha, m, k = shift_plan(n, semitones)
    flags = _zl.OUTPUT_HARMONIC | _zl.OUTPUT_PERCUSSIVE | _zl.OUTPUT_RESIDUAL
    hpr = _zl.HPR(fs, hpr_hop, beta, flags, _zl.TIME_CAUSAL)
    ts = tsm.Tsm(fs, nfft, nfft_ola, 1, n, alpha)
    rs = Resampler(num, den, quality)
    rows = _zl.DeviceBuffer(4 * n)                      # the samples, harm, perc, resid
    scratch, out = _zl.DeviceBuffer(m), _zl.DeviceBuffer(n)
    out.zero()
    rows.upload(xp)
    hpr.process(rows.ptr, n // hpr_hop, in_stride=n, harm=rows.offset(n), perc=rows.offset(2 * n), resid=rows.offset(3 * n), out_stride=n)
    _shift_device(ts, rs, rows.offset(n), rows.offset(2 * n), rows.offset(3 * n), n, n, alpha, m, k, scratch, out)
    _zl.synchronize()
    return out.download()
