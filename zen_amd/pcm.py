"""ctypes binding of libzen_hip_pcm.so (zen_amd/pcm/zen_hip_pcm.h): 16-bit PCM host I/O for the engines of zen_amd.lib.

The engines stay float-only; this module takes the engine objects of zen_amd.lib (anything with the C handle in `_h`:
HPR, HPRIOffline; HPRRealtime through its p_impl) and numpy int16 arrays.  No fallback: a missing library raises.

    eng = zen_amd.HPR(44100.0, 1024, 2.0, zen_amd.OUTPUT_PERCUSSIVE, zen_amd.TIME_CAUSAL)
    perc = np.empty(x16.size, np.int16)
    peaks = pcm.hpr_process_host(eng, x16, perc=perc)           # PEAK mode: what `zen fakert` would write
    pcm.release(eng)                                            # before the engine goes
"""
import ctypes as C

import numpy as np

from . import _addon
from . import lib as _zl

PEAK, GAIN = 0, 1


class _HostStats(C.Structure):
    _fields_ = [("n_pieces", C.c_size_t), ("piece_frames", C.c_size_t), ("input_pinned", C.c_int),
                ("outputs_pinned", C.c_int), ("setup_ms", C.c_double), ("tail_ms", C.c_double), ("total_ms", C.c_double)]


# every symbol zen_amd/pcm/zen_hip_pcm.h declares: (name, restype, argtypes)
_vp, _sz, _i, _f = C.c_void_p, C.c_size_t, C.c_int, C.c_float
_pf = C.POINTER(C.c_float)
SYMBOLS = [
    ("zen_hip_pcm_last_error", C.c_char_p, []),
    ("zen_hip_pcm_version", C.c_char_p, []),
    ("zen_hip_pcm_to_float", _i, [_vp, _i, _sz, _vp, _vp]),
    ("zen_hip_pcm_peak", _i, [_vp, _sz, _vp, _vp]),
    ("zen_hip_pcm_from_float", _i, [_vp, _sz, _i, _f, _vp, _vp, _vp]),
    ("zen_hip_pcm_hpr_process_host", _i, [_vp, _vp, _i, _sz, _vp, _vp, _vp, _i, _f, _pf, _sz]),
    ("zen_hip_pcm_hpri_process", _i, [_vp, _vp, _i, _sz, _vp, _vp, _vp, _i, _f, _pf, _sz]),
    ("zen_hip_pcm_host_stats_get", _i, [C.POINTER(_HostStats)]),
    ("zen_hip_pcm_release", _i, [_vp]),
    ("zen_hip_pcm_release_all", _i, []),
]

def load():
    """Load libzen_hip_pcm.so, building it first where it is absent (_addon.load).  Raises if that fails."""
    return _addon.load("pcm", SYMBOLS)


def _ck(rc):
    _addon.check(rc, load().zen_hip_pcm_last_error)


def _handle(engine):
    engine = getattr(engine, "p_impl", engine)      # HPRRealtime wraps an HPR
    return engine, engine._h


def _ptr16(a, n, what):
    if a is None:
        return None
    assert isinstance(a, np.ndarray) and a.dtype == np.int16 and a.flags["C_CONTIGUOUS"] and a.size == n, what
    return a.ctypes.data_as(C.c_void_p)


# ---- the kernels alone: device pointers (ints / c_void_p, e.g. DeviceBuffer.ptr), asynchronous on `stream` ----------------
def to_float(src_dev, channels, n_frames, dst_dev, stream=None):
    _ck(load().zen_hip_pcm_to_float(src_dev, channels, n_frames, dst_dev, stream))


def peak(src_dev, n, minmax_dev, stream=None):
    """Folds min / max of n floats into the two floats at minmax_dev (which the caller initialised to +inf, -inf)."""
    _ck(load().zen_hip_pcm_peak(src_dev, n, minmax_dev, stream))


def from_float(src_dev, n, dst_dev, mode=PEAK, gain=1.0, minmax_dev=None, stream=None):
    _ck(load().zen_hip_pcm_from_float(src_dev, n, mode, gain, minmax_dev, dst_dev, stream))


# ---- host to host -----------------------------------------------------------------------------------------------------------
def hpr_process_host(engine, x, channels=1, harm=None, perc=None, resid=None, mode=PEAK, gain=1.0, piece_hops=0):
    """zen_hip_pcm_hpr_process_host: x = n_hops * hop frames of `channels` interleaved int16, the wanted outputs int16 arrays
    of n_hops * hop samples (numpy arrays, pageable or views of pinned memory).  Synchronous.  Returns the three peaks
    (harmonic, percussive, residual) in PEAK mode, None in GAIN mode."""
    eng, h = _handle(engine)
    assert isinstance(x, np.ndarray) and x.dtype == np.int16 and x.flags["C_CONTIGUOUS"] and x.size % (eng.hop * channels) == 0
    n_hops = x.size // (eng.hop * channels)
    n = n_hops * eng.hop
    pk = (C.c_float * 3)()
    _ck(load().zen_hip_pcm_hpr_process_host(h, x.ctypes.data_as(C.c_void_p), channels, n_hops, _ptr16(harm, n, "harm"),
                                            _ptr16(perc, n, "perc"), _ptr16(resid, n, "resid"), mode, gain, pk, piece_hops))
    return np.array(pk, dtype=np.float32) if mode == PEAK else None


def hpri_process(engine, audio, channels=1, harm=None, perc=None, resid=None, mode=PEAK, gain=1.0, range_samples=0):
    """zen_hip_pcm_hpri_process: audio = n frames of `channels` interleaved int16; outputs int16 arrays of n samples or None."""
    eng, h = _handle(engine)
    assert getattr(eng, "n_clips", 1) == 1, "host calls take a handle of one clip"
    assert isinstance(audio, np.ndarray) and audio.dtype == np.int16 and audio.flags["C_CONTIGUOUS"] and audio.size % channels == 0
    n = audio.size // channels
    pk = (C.c_float * 3)()
    _ck(load().zen_hip_pcm_hpri_process(h, audio.ctypes.data_as(C.c_void_p), channels, n, _ptr16(harm, n, "harm"),
                                        _ptr16(perc, n, "perc"), _ptr16(resid, n, "resid"), mode, gain, pk, range_samples))
    return np.array(pk, dtype=np.float32) if mode == PEAK else None


def host_stats():
    """What the last host-to-host call of this thread did: pieces, pinned or not, setup / tail / total ms."""
    st = _HostStats()
    _ck(load().zen_hip_pcm_host_stats_get(C.byref(st)))
    return {k: getattr(st, k) for k, _ in _HostStats._fields_}


def release(engine):
    """Frees the staging context of this engine and puts it back on the null stream.  Call it BEFORE the engine object goes."""
    _, h = _handle(engine)
    if h:
        _ck(load().zen_hip_pcm_release(h))


def release_all():
    _ck(load().zen_hip_pcm_release_all())


class PinnedPCM:
    """n int16 of pinned host memory (zen_hip_host_alloc_mapped) as a numpy array."""

    def __init__(self, n):
        h, d = C.c_void_p(), C.c_void_p()
        _zl._ck(_zl.load().zen_hip_host_alloc_mapped(max(n, 1) * 2, 0, C.byref(h), C.byref(d)))
        self._h = h.value
        self.array = np.ctypeslib.as_array(C.cast(h, C.POINTER(C.c_int16)), shape=(n,))

    def free(self):
        if getattr(self, "_h", None):
            self.array = None
            _zl.load().zen_hip_host_free(self._h)
            self._h = None

    def __del__(self):
        self.free()
