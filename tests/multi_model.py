"""numpy model of libzen_hip_multi.so's arithmetic (zen_amd/multi/zen_hip_multi.h), shared by tests/test_multi_model.py (CPU),
tests/test_multi_abi.py and tests/test_gpu_multi.py.  The sample formulas are tests/pcm_model.py's (the model of
zen_amd/pcm/pcm_convert.h); what is added here is the layout -- interleaved frames [n_frames, C] against planar rows
[C, n_frames] -- and the one peak per stem over all its channels."""
import numpy as np

import pcm_model as P

F = np.float32
I16, F32 = 0, 1
PEAK, GAIN = 0, 1


def split(x):
    """x: [n_frames, C] int16 or float32 -> rows [C, n_frames] float32; float32 is copied bit for bit"""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return np.ascontiguousarray(P.to_float(x).T)
    assert x.dtype == np.float32
    return np.ascontiguousarray(x.view(np.uint32).T).view(F)


def minmax(rows):
    """(min, max) over all rows, NaNs ignored; (+inf, -inf) where there is no number at all"""
    r = np.asarray(rows, F).ravel()
    r = r[~np.isnan(r)]
    return (F(np.min(r)), F(np.max(r))) if r.size else (F(np.inf), F(-np.inf))


def peak(rows):
    """pcm16_peak_of(min, max) of a stem: max(-min, max), one number for all its channels; 0 where the stem holds no number"""
    mn, mx = minmax(rows)
    return F(max(-1 * mn, mx)) if mn <= mx else F(0)


def join(rows, fmt, mode=GAIN, gain=32767.0, peak_value=None):
    """rows [C, n_frames] float32 -> [n_frames, C]; F32: the bits; I16: narrowed in GAIN or PEAK mode (peak_value: the
    stem's peak, default peak(rows))"""
    rows = np.asarray(rows, F)
    if fmt == F32:
        return np.ascontiguousarray(rows.view(np.uint32).T).view(F)
    if mode == GAIN:
        return np.ascontiguousarray(P.from_float_gain(rows, gain).T)
    pk = peak(rows) if peak_value is None else F(peak_value)
    return np.ascontiguousarray(P.from_float_peak(rows, pk).T)


def stems(x, separate, mode=PEAK, gain=32767.0):
    """The offline call: x [n_frames, C]; separate(row) -> (harm, perc) of one channel alone.  Returns ({"harm", "perc"} of
    x's shape and dtype, peaks[2] -- zeros unless int16 PEAK)."""
    x = np.asarray(x)
    fmt = I16 if x.dtype == np.int16 else F32
    rows = split(x)
    sep = [separate(r) for r in rows]
    out, peaks = {}, np.zeros(2, F)
    for k, name in enumerate(("harm", "perc")):
        y = np.stack([s[k] for s in sep]) if len(sep) else np.zeros((0, 0), F)
        if fmt == I16 and mode == PEAK:
            peaks[k] = peak(y)
        out[name] = join(y, fmt, mode, gain, peaks[k])
    return out, peaks
