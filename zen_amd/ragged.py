"""ctypes binding of libzen_hip_ragged.so (zen_amd/ragged/zen_hip_ragged.h): the two-pass offline engine on a batch of
clips of UNEQUAL length.  No fallback: a missing library raises.

    rg = ragged.Ragged(44100.0, 4096, 256, 2.0, 2.0, n_clips=len(clips))
    harm, perc = rg.process(clips)                      # lists of float32 arrays, one per clip, each of its clip's length

    groups, fraction = ragged.plan_groups([len(c) for c in clips], 16)   # a large library: sorted groups of 16 clips
"""
import ctypes as C

import numpy as np

from . import _addon
from ._addon import _f, _i, _pd, _psz, _pull, _sz, _vp
from . import lib as _zl

KERNELS = ("pack", "splice", "trim")

# every symbol zen_amd/ragged/zen_hip_ragged.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("zen_hip_ragged_last_error", C.c_char_p, []),
    ("zen_hip_ragged_version", C.c_char_p, []),
    ("zen_hip_ragged_create", _i, [_f, _sz, _sz, _f, _f, _i, _sz, C.POINTER(_vp)]),
    ("zen_hip_ragged_destroy", _i, [_vp]),
    ("zen_hip_ragged_set_stream", _i, [_vp, _vp]),
    ("zen_hip_ragged_use_sse_filter", _i, [_vp]),
    ("zen_hip_ragged_use_soft_mask", _i, [_vp]),
    ("zen_hip_ragged_process_device", _i, [_vp, _vp, _psz, _sz, _vp, _vp, _sz]),
    ("zen_hip_ragged_process_host", _i, [_vp, C.POINTER(_vp), _psz, C.POINTER(_vp), C.POINTER(_vp)]),
    ("zen_hip_ragged_hop_counts", _i, [_vp, _sz, _psz, _psz]),
    ("zen_hip_ragged_profile", _i, [_vp, _i]),
    ("zen_hip_ragged_profile_get", _i, [_vp, _pd, _pull, _pull]),
    ("zen_hip_ragged_profile_get_engine", _i, [_vp, _i, _pd, _pull]),
]

_lib = _addon.Library("ragged", SYMBOLS, (_zl.E_HOPS_NOT_DIVISIBLE,), KERNELS)
load, _ck = _lib.load, _lib.check


def _lens(lens, n_clips):
    assert len(lens) == n_clips, "one length per clip of the handle (%d), got %d" % (n_clips, len(lens))
    return (C.c_size_t * n_clips)(*[int(n) for n in lens])


class Ragged(_addon.Profiled, _addon.EngineProfiled):
    """zen_hip_ragged_t: HPRIOffline on n_clips clips of unequal length per call."""
    _lib = _lib

    def __init__(self, fs, hop_h=4096, hop_p=256, beta_h=2.0, beta_p=2.0, nocopybord=False, n_clips=1):
        self._create(fs, hop_h, hop_p, beta_h, beta_p, int(nocopybord), n_clips)
        self.n_clips = n_clips

    def use_sse_filter(self):
        _ck(self._L.zen_hip_ragged_use_sse_filter(self._h))

    def use_soft_mask(self):
        _ck(self._L.zen_hip_ragged_use_soft_mask(self._h))

    def hop_counts(self, max_len):
        a, b = C.c_size_t(), C.c_size_t()
        _ck(self._L.zen_hip_ragged_hop_counts(self._h, max_len, C.byref(a), C.byref(b)))
        return a.value, b.value

    def process_device(self, audio_dev, lens, stride, harm=None, perc=None, out_stride=None):
        """Device pointers (ints, e.g. DeviceBuffer.ptr): row c of audio_dev holds lens[c] samples; each output row gets them
        followed by zeros up to max(lens).  Asynchronous on the handle's stream."""
        out_stride = stride if out_stride is None else out_stride
        _ck(self._L.zen_hip_ragged_process_device(self._h, audio_dev, _lens(lens, self.n_clips), stride, harm, perc, out_stride))

    def process(self, clips, want=(True, True)):
        """clips: n_clips float32 arrays of any lengths (zero included).  Returns (list_harm, list_perc): per clip an array
        of the clip's length (None for an output that is not wanted).  Synchronous."""
        assert len(clips) == self.n_clips, "one clip per row of the handle (%d), got %d" % (self.n_clips, len(clips))
        clips = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1) for c in clips]
        n = self.n_clips
        outs = [[np.empty(c.size, np.float32) for c in clips] if w else None for w in want]

        def ptrs(arrays):
            if arrays is None:
                return None
            return (C.c_void_p * n)(*[a.ctypes.data if a.size else None for a in arrays])
        _ck(self._L.zen_hip_ragged_process_host(self._h, ptrs(clips), _lens([c.size for c in clips], n), ptrs(outs[0]), ptrs(outs[1])))
        return outs[0], outs[1]


def plan_groups(lengths, group):
    """Cuts a library into batches for a Ragged handle of `group` rows: the clips sorted by length, in consecutive groups of at
    most `group`, filled from the LONGEST clip down (the short group, if any, holds the shortest clips).  A call on a handle
    of `group` rows costs group x (its longest clip): over all ways to put the clips into groups of at most `group`, this one
    has the smallest sum of the groups' longest clips (its k-th group's longest clip is the (k * group + 1)-th longest of the
    library, and no grouping can have fewer than k * group + 1 clips in groups whose maxima are at least that long).
    Returns (groups, fraction): lists of indices into `lengths`, and sum(lengths) / sum(len(g) * longest clip of g) -- the
    share of the padded samples that are the clips' own (1.0 for an empty library).  Pure host arithmetic."""
    group = int(group)
    assert group >= 1
    order = sorted(range(len(lengths)), key=lambda i: (-int(lengths[i]), i))
    groups = [order[i:i + group] for i in range(0, len(order), group)]
    padded = sum(len(g) * int(lengths[g[0]]) for g in groups)
    total = sum(int(n) for n in lengths)
    return groups, (total / padded if padded else 1.0)
