#!/usr/bin/env python3
"""Time-scale modification (zen_amd/tsm) on stems that are resident on the device, in one process; one JSON line.  GPU only:
there is no fallback.

Workloads, both at 44.1 kHz and alpha = 1.5, the vocoder's frame 4096:
  long    one clip of three minutes.  Its 11.9 million output samples are 11 631 vocoder frames; on the overlap-add route a
          frame of 256 would make 93 000 frames, beyond the 16384 a handle takes on either route, so this leg runs the
          overlap-add frame 2048 (11 629 frames) -- the leg with the longest walk.
  batch   64 clips of 30 s in one call, frames 4096 / 256: 1941 vocoder frames per clip, 64 walks side by side.
Per workload:
  hp      one zen_hip_tsm_stretch_hp_device call (harmonic, percussive and residual rows in, one row out), --repeats rounds
          after a warm-up, each between two HIP events; pv and ola alone the same way, interleaved with it.
  From a second, profiled set of rounds: the event times of every kernel with its bytes and achieved GB/s, the bandwidth-shaped
  ones (frame, analysis, peaks, spectrum, overlap_add) as a share of the device copy rate measured in the same run
  (bench.device_copy_bandwidth), and the walk in microseconds per frame.
  model   the numpy model (tests/tsm_model.py) on the host on the first --model-seconds of the long clip, scaled to its length.
On the GPU box, under a time limit of its own:  timeout -k 10 900 python tools/ab_tsm.py > profiles/tsm_ab.json"""
import time

import numpy as np

from _ab import arguments, bench, emit, summary, timed, zen_amd
from zen_amd import tsm

FS = 44100.0
BANDWIDTH_SHAPED = ("frame", "analysis", "peaks", "spectrum", "overlap_add")


def stems(n, clips, seed):
    """three rows per clip standing in for the separation's: the test signal, a click train and low noise"""
    rng = np.random.default_rng(seed)
    harm = np.stack([bench.s_music(n, seed=seed + c) for c in range(clips)]).astype(np.float32)
    perc = np.zeros((clips, n), np.float32)
    perc[:, 1000::22050] = 0.8
    resid = (0.01 * rng.uniform(-1, 1, (clips, n))).astype(np.float32)
    return harm, perc, resid


def workload(name, seconds, clips, nfft, nfft_ola, alpha, a, copy_bw):
    n = int(seconds * FS)
    n_out = tsm.n_out(n, alpha)
    ts = tsm.Tsm(FS, nfft, nfft_ola, clips, n, alpha)
    frames = ts.frames(n, alpha)
    harm, perc, resid = stems(n, clips, a.seed)
    d = [zen_amd.DeviceBuffer.from_host(s) for s in (harm, perc, resid)]
    out = zen_amd.DeviceBuffer(clips * n_out)
    legs = {"hp": lambda: ts.hp_device(d[0], d[1], d[2], n, n, alpha, out, n_out),
            "pv": lambda: ts.pv_device(d[0], n, n, alpha, out, n_out),
            "ola": lambda: ts.ola_device(d[1], d[2], n, n, alpha, out, n_out)}
    for _ in range(a.warmup):
        for run in legs.values():
            run()
    zen_amd.synchronize()
    t = {k: [] for k in legs}
    for _ in range(a.repeats):
        for k, run in legs.items():
            t[k].append(timed(run))
    res = {k: summary(v) for k, v in t.items()}
    for v in res.values():
        v["times_real_time"] = clips * seconds / (v["median_ms"] * 1e-3)
    ts.profile(True)                        # events around every launch slow the call down: kept apart from the timings above
    for _ in range(a.profiled):
        legs["hp"]()
    prof = ts.profile_get()
    ts.profile(False)
    kern = {}
    for kn, v in prof.items():
        gbps = (v["bytes"] / (v["ms"] * 1e-3) / 1e9) if v["ms"] > 0 else None
        kern[kn] = {"ms_per_call": v["ms"] / a.profiled, "bytes_per_call": v["bytes"] // a.profiled, "launches_per_call": v["launches"] // a.profiled,
                    "GBps": gbps}
        if kn in BANDWIDTH_SHAPED and gbps and copy_bw:
            kern[kn]["frac_of_device_copy"] = gbps / copy_bw
    kern["walk"]["us_per_frame"] = 1e3 * kern["walk"]["ms_per_call"] / frames
    kern["total_ms_per_call"] = sum(v["ms"] for v in prof.values()) / a.profiled
    return {"name": name, "seconds": seconds, "clips": clips, "samples": n, "samples_out": n_out, "nfft": nfft, "nfft_ola": nfft_ola, "alpha": alpha,
            "vocoder_frames_per_clip": frames, "legs": res, "kernels": kern, "device_bytes": ts.stats()["device_bytes"]}, harm[0]


def main():
    a = arguments(alpha=1.5, long_seconds=180.0, batch_seconds=30.0, batch_clips=64, repeats=5, warmup=1, profiled=2, model_seconds=2.0, seed=4242)
    zen_amd.init(0)
    copy_bw = bench.device_copy_bandwidth(zen_amd)
    long, x = workload("long", a.long_seconds, 1, 4096, 2048, a.alpha, a, copy_bw)
    batch, _ = workload("batch", a.batch_seconds, a.batch_clips, 4096, 256, a.alpha, a, copy_bw)
    import tsm_model
    cut = x[:int(a.model_seconds * FS)]
    t0 = time.perf_counter()
    tsm_model.stretch_hp(cut, cut, 4096, 2048, a.alpha, cut)
    model_s = time.perf_counter() - t0
    emit(__file__, {
        "repeats": a.repeats, "warmup": a.warmup, "fs": FS, "seed": a.seed,
        "device_copy_GBps": copy_bw, "workloads": [long, batch],
        "host_model": {"seconds_of_audio": a.model_seconds, "wall_s": model_s, "scaled_to_the_long_clip_s": model_s * a.long_seconds / a.model_seconds,
                       "over_the_device_call": model_s * a.long_seconds / a.model_seconds / (long["legs"]["hp"]["median_ms"] * 1e-3)},
    })


if __name__ == "__main__":
    main()
