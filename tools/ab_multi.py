#!/usr/bin/env python3
"""Multichannel separation (zen_amd/multi) against today's route, in one process; one JSON line and profiles/multi_ab.json.

The clip: --seconds (300) of stereo int16 at 44.1 kHz, separated offline at hops 4096 / 256 into PCM16 stems, PEAK mode.
  A  today's route: host deinterleave + widen, zen_hip_hpri_process once per channel (the pipelined host call of the mono
     engine), host joint peak over the channels of a stem, host narrow + interleave (numpy, float32 throughout)
  B  the new host call: zen_hip_multi_offline_host -- int16 frames up, split / engine with n_clips = 2 / peak / join on the
     device, int16 frames down.  Unpipelined: its copies do not overlap its kernels.
Legs A and B are interleaved (A B A B ...), --repeats rounds after one warm-up round each, wall time around calls that end
in a synchronise.  Before that, in the same run, the two routes' stems are compared sample for sample.
  K  the three kernels alone on device buffers of --kernel-scale (4) times the clip's frames (635 MB of frames and rows for
     int16: past the 256 MiB the device's last-level cache holds): split, peak and join for int16 (6, 4 and 6 bytes per
     sample; join in PEAK mode, dividing by the peak that leg `peak` has just found in the random rows it reads, and in GAIN
     mode) and split and join for float32 (8 bytes per sample), each between two HIP events, interleaved, --repeats rounds;
     the split legs read frames made from those rows and write rows of their own, so every leg works on real samples;
     bytes per second next to the box's tuned copy kernel (tools/ubench_copy, bench.py's HBM denominator).
On the GPU box, under a time limit of its own:  timeout -k 10 600 python tools/ab_multi.py"""
import json
import os
import sys
import time

import numpy as np

from _ab import arguments, bench, ROOT, summary, timed, zen_amd
import pcm_model
from zen_amd import multi

FS, HOP_H, HOP_P = 44100.0, 4096, 256


def clip(n, channels, seed=0):
    """[n, channels] int16: a chord and noise per channel, a click every half second, the channels at different levels"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / FS
    cols = []
    for c in range(channels):
        x = 0.25 * np.sin(2 * np.pi * (220 + 55 * c) * t) + 0.15 * np.sin(2 * np.pi * (660 + 30 * c) * t) + 0.1 / (1 + c) * rng.uniform(-1, 1, n)
        x[::22050] += 0.5
        cols.append(np.round(np.clip(x, -1, 1) * 32767).astype(np.int16))
    return np.ascontiguousarray(np.stack(cols, 1))


class Today:
    """route A: everything around the mono engine on the host"""

    def __init__(self):
        self.eng = zen_amd.HPRIOffline(FS, HOP_H, HOP_P, 2.0, 2.0)
        self.parts = {}

    def run(self, x16):
        t0 = time.perf_counter()
        rows = [np.ascontiguousarray(x16[:, c]).astype(np.float32) / np.float32(32767) for c in range(x16.shape[1])]
        t1 = time.perf_counter()
        sep = [self.eng.process(r, out=(np.empty(r.size, np.float32), np.empty(r.size, np.float32), None))[:2] for r in rows]   # no residual
        t2 = time.perf_counter()
        out = {}
        for k, name in enumerate(("harm", "perc")):
            peak = np.float32(max(max(-1 * s[k].min(), s[k].max()) for s in sep))
            y = np.empty(x16.shape, np.int16)
            for c, s in enumerate(sep):
                y[:, c] = pcm_model.from_float_peak(s[k], peak)
            out[name] = y
        t3 = time.perf_counter()
        self.parts = {"host_split_ms": (t1 - t0) * 1e3, "engine_calls_ms": (t2 - t1) * 1e3, "host_peak_join_ms": (t3 - t2) * 1e3}
        return out


def kernel_leg(n, channels, repeats):
    """`rows` keeps its random samples throughout: the split legs write rows of their own.  minmax is initialised and peak
    has run before the PEAK join of a round is timed, so that join divides by the rows' real peak."""
    rng = np.random.default_rng(1)
    out = {}
    rows_host = rng.uniform(-1, 1, channels * n).astype(np.float32)
    rows = zen_amd.DeviceBuffer.from_host(rows_host)
    split_rows = zen_amd.DeviceBuffer(channels * n)
    mm = zen_amd.DeviceBuffer(2)
    legs = {}
    for name, fmt, dtype in (("i16", multi.I16, np.int16), ("f32", multi.F32, np.float32)):
        frames = zen_amd.DeviceBuffer(n * channels, dtype)
        multi.join(fmt, rows, channels, n, n, frames, mode=multi.GAIN, gain=32767.0)      # frames worth splitting: the rows' own
        b = np.dtype(dtype).itemsize
        legs["split_" + name] = (lambda fmt=fmt, frames=frames: multi.split(fmt, frames, channels, n, split_rows, n), (b + 4) * n * channels)
        out_frames = zen_amd.DeviceBuffer(n * channels, dtype)
        if fmt == multi.I16:
            legs["join_i16_peak"] = (lambda o=out_frames: multi.join(multi.I16, rows, channels, n, n, o, mode=multi.PEAK, minmax_dev=mm), 6 * n * channels)
            legs["join_i16_gain"] = (lambda o=out_frames: multi.join(multi.I16, rows, channels, n, n, o, mode=multi.GAIN, gain=30000.0), 6 * n * channels)
        else:
            legs["join_f32"] = (lambda o=out_frames: multi.join(multi.F32, rows, channels, n, n, o), 8 * n * channels)
    legs = dict([("peak", (lambda: multi.peak(rows, channels, n, n, mm), 4 * n * channels))] + list(legs.items()))   # peak first: PEAK join reads its words
    times = {k: [] for k in legs}
    for r in range(repeats + 1):
        mm.upload(np.array([np.inf, -np.inf], np.float32))
        for k, (f, _) in legs.items():
            ms = timed(f)
            if r:                        # round 0 warms up
                times[k].append(ms)
    got = mm.download()
    out["minmax_at_the_end"] = [float(got[0]), float(got[1])]
    out["minmax_of_the_rows"] = [float(rows_host.min()), float(rows_host.max())]
    out["rows_unchanged"] = bool(np.array_equal(rows.download(), rows_host))
    for k, (_, nbytes) in legs.items():
        s = summary(times[k])
        s["bytes"] = nbytes
        s["GBps"] = nbytes / (s["median_ms"] * 1e-3) / 1e9
        out[k] = s
    return out


def main():
    a = arguments(seconds=300.0, channels=2, repeats=5, kernel_scale=4, out=os.path.join(ROOT, "profiles", "multi_ab.json"))
    zen_amd.init(0)
    n = int(a.seconds * FS)
    x16 = clip(n, a.channels)
    today, new = Today(), multi.Offline(FS, HOP_H, HOP_P, 2.0, 2.0, channels=a.channels)
    ra, rb = today.run(x16), new.process(x16)            # warm-up of both, and the comparison
    same = {k: bool(np.array_equal(ra[k], rb[k])) for k in ("harm", "perc")}
    ta, tb, parts = [], [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        today.run(x16)
        t1 = time.perf_counter()
        new.process(x16)
        t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3)
        tb.append((t2 - t1) * 1e3)
        parts.append(today.parts)
    copy = bench.tuned_copy_record()
    rec = {"tool": "tools/ab_multi.py", "device": zen_amd.device_name(), "fs": FS, "hops": [HOP_H, HOP_P], "channels": a.channels,
           "frames": n, "seconds": a.seconds, "format": "int16 in, int16 PEAK out", "same_samples": same,
           "today_host_route": dict(summary(ta), parts_median_ms={k: float(np.median([p[k] for p in parts])) for k in parts[0]}),
           "multi_offline_host": dict(summary(tb), pipelined=False, staging=new.stats()),
           "speedup_median": float(np.median(ta) / np.median(tb)),
           "kernel_frames": a.kernel_scale * n,
           "kernels": kernel_leg(a.kernel_scale * n, a.channels, a.repeats), "tuned_copy": copy}
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    k = rec["kernels"]
    return 0 if all(same.values()) and k["rows_unchanged"] and k["minmax_at_the_end"] == k["minmax_of_the_rows"] else 1


if __name__ == "__main__":
    sys.exit(main())
