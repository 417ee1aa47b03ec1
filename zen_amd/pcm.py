"""ctypes binding of libzen_hip_pcm.so (zen_amd/pcm/zen_hip_pcm.h): 16- and 24-bit PCM host I/O for the engines of zen_amd.lib.

The engines stay float-only; this module takes the engine objects of zen_amd.lib (anything with the C handle in `_h`:
HPR, HPRIOffline; HPRRealtime through its p_impl) and numpy arrays: int16 for 16-bit samples (I16), uint8 holding three
little-endian bytes per sample for packed 24-bit samples (I24; pack24 / unpack24 convert from and to int32).  No fallback:
a missing library raises.

    eng = zen_amd.HPR(44100.0, 1024, 2.0, zen_amd.OUTPUT_PERCUSSIVE, zen_amd.TIME_CAUSAL)
    perc = np.empty(x16.size, np.int16)
    peaks = pcm.hpr_process_host(eng, x16, perc=perc)           # PEAK mode: what `zen fakert` would write
    pcm.release(eng)                                            # before the engine goes

    pcm.offline_wav("in.wav", "harm.wav", "perc.wav")           # a 16- or 24-bit WAV file through the offline engine
"""
import ctypes as C

import numpy as np

from . import _addon
from ._addon import _f, _i, _sz, _vp
from . import lib as _zl

PEAK, GAIN = 0, 1
I16, I24 = 0, 1                     # ZEN_HIP_PCM_I16 / _I24: 2 and 3 bytes per sample, little-endian, packed


class _HostStats(C.Structure):
    _fields_ = [("n_pieces", C.c_size_t), ("piece_frames", C.c_size_t), ("input_pinned", C.c_int),
                ("outputs_pinned", C.c_int), ("setup_ms", C.c_double), ("tail_ms", C.c_double), ("total_ms", C.c_double)]


# every symbol zen_amd/pcm/zen_hip_pcm.h declares: (name, restype, argtypes)
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
    ("zen_hip_pcm_sample_bytes", _sz, [_i]),
    ("zen_hip_pcm_unpack", _i, [_i, _vp, _i, _sz, _vp, _vp]),
    ("zen_hip_pcm_pack", _i, [_i, _vp, _sz, _i, _f, _vp, _vp, _vp]),
    ("zen_hip_pcm_hpr_process_host_fmt", _i, [_vp, _i, _vp, _i, _sz, _i, _vp, _vp, _vp, _i, _f, _pf, _sz]),
    ("zen_hip_pcm_hpri_process_fmt", _i, [_vp, _i, _vp, _i, _sz, _i, _vp, _vp, _vp, _i, _f, _pf, _sz]),
]

_lib = _addon.Library("pcm", SYMBOLS)
load, _ck = _lib.load, _lib.check


def _handle(engine):
    engine = getattr(engine, "p_impl", engine)      # HPRRealtime wraps an HPR
    return engine, engine._h


_DTYPES = {I16: (np.dtype(np.int16), 1), I24: (np.dtype(np.uint8), 3)}      # format -> (dtype, array elements per sample)


def pack24(v):
    """int32 array of 24-bit codes -> uint8 array of 3 n bytes, little-endian (the low three bytes of each value)."""
    v = np.ascontiguousarray(v, np.int32).reshape(-1)
    return np.ascontiguousarray(v.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1)


def unpack24(b):
    """uint8 array of 3 n bytes -> int32 array of n sign-extended codes; the inverse of pack24."""
    b = np.ascontiguousarray(b, np.uint8).reshape(-1, 3)
    w = np.zeros((b.shape[0], 4), np.uint8)
    w[:, :3] = b
    w[:, 3] = np.where(b[:, 2] & 0x80, 0xFF, 0)
    return w.view("<i4").reshape(-1).astype(np.int32)


def _fmt_of(a, what):
    assert isinstance(a, np.ndarray) and a.flags["C_CONTIGUOUS"], what
    for fmt, (dt, _) in _DTYPES.items():
        if a.dtype == dt:
            return fmt
    raise TypeError("%s: int16 (I16) or uint8 (I24, three bytes per sample) arrays, not %s" % (what, a.dtype))


def _outputs(outs, n):
    """the one format of the outputs that are not None (I16 where there is none) and their pointers"""
    fmts = {_fmt_of(a, name) for name, a in outs if a is not None}
    assert len(fmts) <= 1, "all outputs of a call have one format"
    fmt = fmts.pop() if fmts else I16
    for name, a in outs:
        assert a is None or a.size == n * _DTYPES[fmt][1], name
    return fmt, [None if a is None else a.ctypes.data_as(C.c_void_p) for _, a in outs]


# ---- the kernels alone: device pointers (ints / c_void_p, e.g. DeviceBuffer.ptr), asynchronous on `stream` ----------------
def to_float(src_dev, channels, n_frames, dst_dev, stream=None, fmt=I16):
    if fmt == I16:
        _ck(load().zen_hip_pcm_to_float(src_dev, channels, n_frames, dst_dev, stream))
    else:
        _ck(load().zen_hip_pcm_unpack(fmt, src_dev, channels, n_frames, dst_dev, stream))


def peak(src_dev, n, minmax_dev, stream=None):
    """Folds min / max of n floats into the two floats at minmax_dev (which the caller initialised to +inf, -inf)."""
    _ck(load().zen_hip_pcm_peak(src_dev, n, minmax_dev, stream))


def from_float(src_dev, n, dst_dev, mode=PEAK, gain=1.0, minmax_dev=None, stream=None, fmt=I16):
    if fmt == I16:
        _ck(load().zen_hip_pcm_from_float(src_dev, n, mode, gain, minmax_dev, dst_dev, stream))
    else:
        _ck(load().zen_hip_pcm_pack(fmt, src_dev, n, mode, gain, minmax_dev, dst_dev, stream))


# ---- host to host -----------------------------------------------------------------------------------------------------------
def hpr_process_host(engine, x, channels=1, harm=None, perc=None, resid=None, mode=PEAK, gain=1.0, piece_hops=0):
    """zen_hip_pcm_hpr_process_host(_fmt): x = n_hops * hop frames of `channels` interleaved samples, int16 (I16) or uint8
    with three bytes per sample (I24); the wanted outputs arrays of n_hops * hop samples, all int16 or all uint8, whatever x
    is (numpy arrays, pageable or views of pinned memory).  Synchronous.  Returns the three peaks (harmonic, percussive,
    residual) in PEAK mode, None in GAIN mode."""
    eng, h = _handle(engine)
    in_fmt = _fmt_of(x, "x")
    per = eng.hop * channels * _DTYPES[in_fmt][1]
    assert x.size % per == 0
    n_hops = x.size // per
    out_fmt, (ph, pp, pr) = _outputs((("harm", harm), ("perc", perc), ("resid", resid)), n_hops * eng.hop)
    pk = (C.c_float * 3)()
    xp = x.ctypes.data_as(C.c_void_p)
    if in_fmt == I16 and out_fmt == I16:
        _ck(load().zen_hip_pcm_hpr_process_host(h, xp, channels, n_hops, ph, pp, pr, mode, gain, pk, piece_hops))
    else:
        _ck(load().zen_hip_pcm_hpr_process_host_fmt(h, in_fmt, xp, channels, n_hops, out_fmt, ph, pp, pr, mode, gain, pk, piece_hops))
    return np.array(pk, dtype=np.float32) if mode == PEAK else None


def hpri_process(engine, audio, channels=1, harm=None, perc=None, resid=None, mode=PEAK, gain=1.0, range_samples=0):
    """zen_hip_pcm_hpri_process(_fmt): audio = n frames of `channels` interleaved samples, int16 (I16) or uint8 with three
    bytes per sample (I24); outputs arrays of n samples, all int16 or all uint8, or None."""
    eng, h = _handle(engine)
    assert getattr(eng, "n_clips", 1) == 1, "host calls take a handle of one clip"
    in_fmt = _fmt_of(audio, "audio")
    per = channels * _DTYPES[in_fmt][1]
    assert audio.size % per == 0
    n = audio.size // per
    out_fmt, (ph, pp, pr) = _outputs((("harm", harm), ("perc", perc), ("resid", resid)), n)
    pk = (C.c_float * 3)()
    ap = audio.ctypes.data_as(C.c_void_p)
    if in_fmt == I16 and out_fmt == I16:
        _ck(load().zen_hip_pcm_hpri_process(h, ap, channels, n, ph, pp, pr, mode, gain, pk, range_samples))
    else:
        _ck(load().zen_hip_pcm_hpri_process_fmt(h, in_fmt, ap, channels, n, out_fmt, ph, pp, pr, mode, gain, pk, range_samples))
    return np.array(pk, dtype=np.float32) if mode == PEAK else None


def offline_wav(in_path, harm_path, perc_path, bits=None, hop_h=4096, beta_h=2.5, hop_p=256, beta_p=2.5, soft_mask=False):
    """A 16- or 24-bit PCM WAV file (mono or stereo) through the offline engine, the way `zen offline` does it, without a
    sample converted on the host: the file's frames go up as they are, hpri_process normalises each stem to its peak, and
    two mono files come back at the input's depth, or at `bits` (16 or 24).  Returns the peaks (harmonic, percussive).
    Raises what the standard library's wave module raises for a file it cannot open, ValueError for any other width."""
    import wave
    fmts = {16: I16, 24: I24}
    with wave.open(in_path, "rb") as w:
        width, channels, rate = 8 * w.getsampwidth(), w.getnchannels(), w.getframerate()
        if width not in fmts:
            raise ValueError("%s: %d-bit samples; 16- and 24-bit PCM are read" % (in_path, width))
        if channels not in (1, 2):
            raise ValueError("%s: %d channels; mono and stereo are read" % (in_path, channels))
        raw = w.readframes(w.getnframes())
    out_bits = width if bits is None else bits
    if out_bits not in fmts:
        raise ValueError("bits=%r; 16 and 24 are written" % (bits,))
    audio = np.frombuffer(raw, np.uint8 if width == 24 else "<i2")
    n = audio.size // (channels * _DTYPES[fmts[width]][1])
    dt, per = _DTYPES[fmts[out_bits]]
    harm, perc = np.zeros(n * per, dt), np.zeros(n * per, dt)
    eng = _zl.HPRIOffline(float(rate), hop_h, hop_p, beta_h, beta_p)
    if soft_mask:
        eng.use_soft_mask()
    try:
        peaks = hpri_process(eng, np.ascontiguousarray(audio), channels, harm=harm, perc=perc, mode=PEAK)
    finally:
        release(eng)
    for path, a in ((harm_path, harm), (perc_path, perc)):
        with wave.open(path, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(out_bits // 8)
            w.setframerate(rate)
            w.writeframes(a.tobytes())
    return peaks[:2]


def host_stats():
    """What the last host-to-host call of this thread did: pieces, pinned or not, setup / tail / total ms."""
    st = _HostStats()
    _ck(load().zen_hip_pcm_host_stats_get(C.byref(st)))
    return _addon.as_dict(st)


def release(engine):
    """Frees the staging context of this engine and puts it back on the null stream.  Call it BEFORE the engine object goes."""
    _, h = _handle(engine)
    if h:
        _ck(load().zen_hip_pcm_release(h))


def release_all():
    _ck(load().zen_hip_pcm_release_all())


class PinnedPCM:
    """n samples of pinned host memory (zen_hip_host_alloc_mapped) as a numpy array: n int16 (I16) or 3 n uint8 (I24)."""

    def __init__(self, n, fmt=I16):
        dt, per = _DTYPES[fmt]
        h, d = C.c_void_p(), C.c_void_p()
        _zl._ck(_zl.load().zen_hip_host_alloc_mapped(max(n, 1) * per * dt.itemsize, 0, C.byref(h), C.byref(d)))
        self._h = h.value
        ctype = C.c_int16 if fmt == I16 else C.c_uint8
        self.array = np.ctypeslib.as_array(C.cast(h, C.POINTER(ctype)), shape=(n * per,))

    def free(self):
        if getattr(self, "_h", None):
            self.array = None
            _zl.load().zen_hip_host_free(self._h)
            self._h = None

    def __del__(self):
        self.free()
