"""ctypes binding of libzen_hip_nmf.so (zen_amd/nmf/zen_hip_nmf.h): supervised non-negative matrix factorisation of the
magnitude spectrogram (Kullback-Leibler, multiplicative updates) on the device -- two pitched, sustained sources separated
by their spectra.  No fallback: a missing library raises.

    Wa = nmf.train(a, 44100.0, 32)                          # a dictionary per source, from isolated material
    Wb = nmf.train(b, 44100.0, 32)
    sa, sb = nmf.separate(mix, 44100.0, [Wa, Wb])           # the dictionaries held, the activations learned
    sa, sb, rest = nmf.separate(mix, 44100.0, [Wa, Wb], free=8)
    W, H, stems = nmf.decompose(x, 44100.0, 8)              # unsupervised: one stem per component
"""
import ctypes as C
import struct

import numpy as np

from . import _addon
from ._addon import _f, _i, _pd, _pull, _sz, _vp

KERNELS = ("frame", "fft", "magnitude", "ratio_mfma", "ratio_valu", "update_h_mfma", "update_h_valu", "update_w_mfma", "update_w_valu", "mask",
           "ifft", "overlap_add")
TABLE_WINDOW, TABLE_DIVISOR = range(2)
ROUTE_DEFAULT, ROUTE_MFMA, ROUTE_VALU = range(3)
MAX_COMPONENTS, MAX_FRAMES, SEGMENT = 256, 16384, 256
ITERATIONS = 100
ZNMF_MAGIC, ZNMF_VERSION = b"ZNMF", 1


class Stats(C.Structure):
    _fields_ = [("calls", C.c_ulonglong), ("clips", C.c_ulonglong), ("iterations", C.c_ulonglong), ("device_bytes", C.c_ulonglong),
                ("allocations", C.c_ulonglong)]


# every symbol zen_amd/nmf/zen_hip_nmf.h declares: (name, restype, argtypes)
_process = [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _sz, _sz, _sz, _i, _vp, _sz, _vp, _sz]
SYMBOLS = [
    ("zen_hip_nmf_last_error", C.c_char_p, []),
    ("zen_hip_nmf_version", C.c_char_p, []),
    ("zen_hip_nmf_create", _i, [_f, _sz, _sz, _sz, _sz, C.POINTER(_vp)]),
    ("zen_hip_nmf_destroy", _i, [_vp]),
    ("zen_hip_nmf_set_stream", _i, [_vp, _vp]),
    ("zen_hip_nmf_process_device", _i, _process),
    ("zen_hip_nmf_process_host", _i, _process),
    ("zen_hip_nmf_ratio_device", _i, [_vp, _sz, _vp, _sz, _vp, _sz, _sz, _sz, _sz, _vp, _sz, _vp, _sz, _i, _vp]),
    ("zen_hip_nmf_update_h_device", _i, [_vp, _sz, _vp, _sz, _vp, _sz, _sz, _sz, _sz, _vp, _sz, _i, _vp]),
    ("zen_hip_nmf_update_w_device", _i, [_vp, _sz, _vp, _sz, _vp, _sz, _sz, _sz, _sz, _sz, _vp, _sz, _i, _vp]),
    ("zen_hip_nmf_stats", _i, [_vp, C.POINTER(Stats)]),
    ("zen_hip_nmf_profile", _i, [_vp, _i]),
    ("zen_hip_nmf_profile_get", _i, [_vp, _pd, _pull, _pull]),
    ("zen_hip_nmf_init", _i, [C.c_ulonglong, _sz, _vp]),
    ("zen_hip_nmf_table", _i, [_sz, _i, _vp, _sz]),
]

_lib = _addon.Library("nmf", SYMBOLS, kernels=KERNELS, stats=Stats)
load, _ck, _ptr = _lib.load, _lib.check, _addon.ptr
n_frames, table = _addon.n_frames, _lib.stft_table


def init(seed, count):
    """`count` initial values in (0, 1] from `seed` (splitmix64) as a float32 array; needs no device"""
    out = np.empty(count, np.float32)
    _ck(load().zen_hip_nmf_init(seed & 0xFFFFFFFFFFFFFFFF, out.size, out.ctypes.data))
    return out


def ratio_device(v_dev, v_stride, w_dev, w_stride, h_dev, h_stride, components, bins, frames, q_dev, q_stride, lam_dev=None, lam_stride=0,
                 route=ROUTE_DEFAULT, stream=None):
    """Q = V / max(H^T W, eps) alone on device memory (and the model L where lam_dev is given).  Asynchronous on `stream`."""
    _ck(load().zen_hip_nmf_ratio_device(_ptr(v_dev), v_stride, _ptr(w_dev), w_stride, _ptr(h_dev), h_stride, components, bins, frames, _ptr(q_dev),
                                        q_stride, _ptr(lam_dev), lam_stride, route, stream))


def update_h_device(w_dev, w_stride, q_dev, q_stride, h_dev, h_stride, components, bins, frames, out_dev, out_stride, route=ROUTE_DEFAULT, stream=None):
    """H' = H (W Q^T) / max(rowsum W, eps) alone.  Asynchronous on `stream`."""
    _ck(load().zen_hip_nmf_update_h_device(_ptr(w_dev), w_stride, _ptr(q_dev), q_stride, _ptr(h_dev), h_stride, components, bins, frames,
                                           _ptr(out_dev), out_stride, route, stream))


def update_w_device(h_dev, h_stride, q_dev, q_stride, w_dev, w_stride, components, bins, frames, fixed, out_dev, out_stride, route=ROUTE_DEFAULT,
                    stream=None):
    """W' = W (H Q) / max(rowsum H, eps) for the rows from `fixed` on, alone.  Asynchronous on `stream`."""
    _ck(load().zen_hip_nmf_update_w_device(_ptr(h_dev), h_stride, _ptr(q_dev), q_stride, _ptr(w_dev), w_stride, components, bins, frames, fixed,
                                           _ptr(out_dev), out_stride, route, stream))


class Nmf(_addon.Handle):
    """zen_hip_nmf_t: n_clips clips of up to max_samples samples per call, each factorised on its own with `components`
    components"""
    _lib = _lib

    def __init__(self, fs, nfft=2048, components=32, n_clips=1, max_samples=1 << 20):
        self._create(fs, nfft, components, n_clips, max_samples)
        self.fs, self.nfft, self.hop, self.bins = fs, nfft, nfft // 2, nfft // 2 + 1
        self.components, self.n_clips, self.max_samples = components, n_clips, max_samples

    def process_device(self, in_dev, in_stride, n, w_dev, w_stride, w_clip_stride, h_dev, h_stride, h_clip_stride, fixed, iterations, groups=None,
                       n_groups=0, stems=None, out_stride=0):
        """DeviceBuffers or device addresses; groups: None (a fit only) or `components` ints in -1..n_groups-1.  Asynchronous."""
        g = None if groups is None else (C.c_int * self.components)(*[int(v) for v in groups])
        _ck(self._L.zen_hip_nmf_process_device(self._h, _ptr(in_dev), in_stride, n, _ptr(w_dev), w_stride, w_clip_stride, _ptr(h_dev), h_stride,
                                               h_clip_stride, fixed, iterations, g, n_groups, _ptr(stems), out_stride))

    def run(self, x, W, H=None, fixed=0, iterations=ITERATIONS, groups=None, n_groups=0, seed=0):
        """x: float32, (n,) for one clip or (n_clips, n).  W: (K, F) -- one dictionary for every clip, which needs fixed == K
        -- or (n_clips, K, F); H: (n_clips, K, m), or None for zen_hip_nmf_init(seed + 1) on every clip.  Returns (W, H,
        stems): copies after `iterations`, stems (n_groups, n_clips, n) or None without groups; for a one-dimensional x the
        clip axis is dropped.  Synchronous."""
        x, one = _addon.clips(x, self.n_clips)
        n = x.shape[1]
        m, K, F = n_frames(n, self.nfft), self.components, self.bins
        W = np.array(W, dtype=np.float32, order="C")
        shared = W.ndim == 2 and self.n_clips > 1
        W = W.reshape((K, F) if shared else (self.n_clips, K, F))
        H = np.tile(init(seed + 1, K * m).reshape(1, K, m), (self.n_clips, 1, 1)) if H is None else np.array(H, dtype=np.float32, order="C")
        H = H.reshape(self.n_clips, K, m)
        g = None if groups is None else (C.c_int * K)(*[int(v) for v in groups])
        stems = np.empty((n_groups, self.n_clips, n), np.float32) if groups is not None else None
        _ck(self._L.zen_hip_nmf_process_host(self._h, x.ctypes.data, n, n, W.ctypes.data, F, 0 if shared else K * F, H.ctypes.data, m, K * m, fixed,
                                             iterations, g, n_groups, stems.ctypes.data if stems is not None else None, n))
        if one:
            return W.reshape(K, F), H[0], None if stems is None else stems[:, 0]
        return W, H, stems


def _clip(x):
    return np.ascontiguousarray(x, dtype=np.float32).ravel()


def train(x, fs, components, nfft=2048, iterations=ITERATIONS, seed=0):
    """The dictionary of one source: (components, nfft / 2 + 1) float32 spectra learned from the clip x, W starting from
    init(seed) and H from init(seed + 1)."""
    x = _clip(x)
    W0 = init(seed, components * (nfft // 2 + 1))
    return Nmf(fs, nfft, components, 1, x.size).run(x, W0, None, 0, iterations, seed=seed)[0]


def separate(x, fs, dictionaries, nfft=None, iterations=ITERATIONS, free=0, seed=0):
    """One stem per dictionary ((K_i, F) arrays, held fixed) of the clip x; free > 0 appends that many components learned on
    the mixture (from init(seed)), which form a last stem of their own.  Returns the list of stems."""
    x = _clip(x)
    dictionaries = [np.asarray(d, np.float32) for d in dictionaries]
    F = dictionaries[0].shape[1]
    nfft = 2 * (F - 1) if nfft is None else nfft
    assert all(d.ndim == 2 and d.shape[1] == nfft // 2 + 1 for d in dictionaries), "dictionaries of the frame's bins"
    fixed = sum(d.shape[0] for d in dictionaries)
    groups = [g for g, d in enumerate(dictionaries) for _ in range(d.shape[0])] + [len(dictionaries)] * free
    W = np.concatenate(dictionaries + ([init(seed, free * F).reshape(free, F)] if free else []))
    n_groups = len(dictionaries) + (1 if free else 0)
    stems = Nmf(fs, nfft, fixed + free, 1, x.size).run(x, W, None, fixed, iterations, groups, n_groups, seed)[2]
    return [stems[g] for g in range(n_groups)]


def decompose(x, fs, components, nfft=2048, iterations=ITERATIONS, seed=0):
    """(W, H, stems): an unsupervised factorisation of the clip x and one stem per component, (components, n)."""
    x = _clip(x)
    W0 = init(seed, components * (nfft // 2 + 1))
    return Nmf(fs, nfft, components, 1, x.size).run(x, W0, None, 0, iterations, list(range(components)), components, seed)


def save_znmf(path, W, nfft, fs):
    """A dictionary as a .znmf file (little-endian): b"ZNMF", uint32 version 1, uint32 nfft, uint32 K, float32 fs, K rows of
    nfft / 2 + 1 float32 -- what zen-nmf reads and writes."""
    W = np.ascontiguousarray(W, np.float32)
    assert W.ndim == 2 and W.shape[1] == nfft // 2 + 1
    with open(path, "wb") as f:
        f.write(ZNMF_MAGIC + struct.pack("<IIIf", ZNMF_VERSION, nfft, W.shape[0], fs))
        f.write(W.astype("<f4").tobytes())


def load_znmf(path):
    """(W, nfft, fs) of a .znmf file"""
    with open(path, "rb") as f:
        head = f.read(20)
        if len(head) != 20 or head[:4] != ZNMF_MAGIC:
            raise ValueError("%s is no .znmf file" % path)
        version, nfft, K, fs = struct.unpack("<IIIf", head[4:])
        if version != ZNMF_VERSION:
            raise ValueError("%s: version %d" % (path, version))
        body = f.read()
    F = nfft // 2 + 1
    if len(body) != 4 * K * F:
        raise ValueError("%s: %d bytes of spectra, %d x %d expected" % (path, len(body), K, F))
    return np.frombuffer(body, "<f4").astype(np.float32).reshape(K, F), nfft, fs
