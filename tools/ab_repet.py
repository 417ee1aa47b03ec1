#!/usr/bin/env python3
"""REPET (zen_amd/repet) on a clip that is resident on the device, in one process; one JSON line.

Workload: three minutes of mono audio at 44.1 kHz, frame 2048 (7753 frames of 1025 bins): 86 frames (2.0 s) of the project's
test signal (bench.s_music) repeated as the accompaniment, a gliding tone with a slow tremolo in front of it.
  G91   one zen_hip_repet_separate_device call with the period given, 86 frames: 91 segments, the median's LDS path
  G31   the same with 258 frames given (6.0 s): 31 segments, the median's register path
  F     the same call with the period found (the beat spectrum, one wait, the search on the host)
        The three legs are interleaved (G91 G31 F G91 ...), --repeats rounds after a warm-up, each between two HIP events.
        From a second, profiled set of rounds: the event times of every kernel with its bytes and achieved GB/s.
  M     the segment-median kernel alone (zen_hip_repet_segment_median_device) on a V of the clip's shape, both periods,
        --median-launches launches between two events; its bytes (V read once, S written once) per second against the device
        copy rate bench.py measures on the same box (device_copy_GBps).  The V of this clip is 32 MB: it fits the Infinity
        Cache, so the rate is not an HBM rate; the copy rate it is held against is measured on 1 GiB.
  H     the host route for the same step: V to the host, numpy.median over the repetitions, S back to the device; wall time.
On the GPU box, under a time limit of its own:  timeout -k 10 600 python tools/ab_repet.py > profiles/repet_ab.json"""
import time

import numpy as np

from _ab import arguments, bench, emit, kernels, summary, timed, zen_amd
from zen_amd import repet

FS, NFFT = 44100.0, 2048
HOP, BINS = NFFT // 2, NFFT // 2 + 1


def clip(seconds, period_frames, seed):
    n = int(seconds * FS)
    one = bench.s_music(period_frames * HOP, seed=seed).astype(np.float64)
    t = np.arange(n)
    phi = 2 * np.pi * np.cumsum(0.01 + 0.004 * np.sin(2 * np.pi * t / (n / 2.7)) + 0.01 * t / n)
    fg = 0.2 * np.sin(phi) * (0.5 + 0.5 * np.sin(2 * np.pi * t / (n / 3.3)))
    return (np.tile(one, n // one.size + 1)[:n] + fg).astype(np.float32)


def main():
    a = arguments(seconds=180.0, period=86, long_period=258, repeats=10, warmup=2, profiled=2, median_launches=50, seed=4242)
    zen_amd.init(0)
    x = clip(a.seconds, a.period, a.seed)
    n = x.size
    m = repet.n_frames(n, NFFT)
    rp = repet.Repet(FS, NFFT, 1, n)
    inp = zen_amd.DeviceBuffer.from_host(x)
    bg, fg = zen_amd.DeviceBuffer(n), zen_amd.DeviceBuffer(n)
    used = {}

    def leg(name, periods):
        def run():
            used[name] = rp.separate_device(inp, n, n, periods, bg, fg, n)
        return run
    legs = {"G91": leg("G91", [a.period]), "G31": leg("G31", [a.long_period]), "F": leg("F", None)}
    for _ in range(a.warmup):
        for run in legs.values():
            run()
    zen_amd.synchronize()
    t = {k: [] for k in legs}
    for _ in range(a.repeats):
        for k, run in legs.items():
            t[k].append(timed(run))
    res = {k: summary(v) for k, v in t.items()}
    for k, v in res.items():
        v["times_real_time"] = a.seconds / (v["median_ms"] * 1e-3)
        v["period_frames"] = used[k][0]
        v["segments"] = -(-m // used[k][0]) if used[k][0] else None

    kern = {}
    for k, run in legs.items():        # events around every launch slow the calls down: kept apart from the timings above
        rp.profile(True)
        for _ in range(a.profiled):
            run()
        kern[k] = kernels(rp.profile_get(), a.profiled)
        rp.profile(False)

    # legs M and H: the step alone on a V of the clip's shape
    stride = (BINS + 3) // 4 * 4
    rng = np.random.default_rng(a.seed)
    v_host = rng.uniform(0, 1, (m, stride)).astype(np.float32)
    v_dev = zen_amd.DeviceBuffer.from_host(v_host)
    copy_bw = bench.device_copy_bandwidth(zen_amd)
    median = {}
    for p in (a.period, a.long_period):
        s_dev = zen_amd.DeviceBuffer(p * stride)

        def launches(p=p, s_dev=s_dev):
            for _ in range(a.median_launches):
                repet.segment_median_device(v_dev, m, BINS, stride, p, s_dev, stride)
        launches()
        zen_amd.synchronize()
        ts = [timed(launches) / a.median_launches for _ in range(5)]
        nbytes = 4 * BINS * (m + p)
        got = s_dev.download().reshape(p, stride)[:, :BINS]
        t0 = time.perf_counter()
        back = v_dev.download().reshape(m, stride)
        s_host = np.stack([np.median(back[l::p, :BINS], axis=0) for l in range(p)]).astype(np.float32)
        up = zen_amd.DeviceBuffer.from_host(s_host)
        zen_amd.synchronize()
        host_ms = 1e3 * (time.perf_counter() - t0)
        up.free()
        ms = float(np.median(ts))
        median["p%d" % p] = {"segments": -(-m // p), "path": "registers" if -(-m // p) <= repet.REGISTER_SEGMENTS else "lds",
                             "kernel_ms": ms, "min_ms": float(min(ts)), "max_ms": float(max(ts)), "bytes": nbytes,
                             "GBps": nbytes / (ms * 1e-3) / 1e9, "frac_of_device_copy": nbytes / (ms * 1e-3) / 1e9 / copy_bw if copy_bw else None,
                             "host_route_ms": host_ms, "host_route_over_kernel": host_ms / ms,
                             # float32 medians of an even count: numpy averages in float32 as well; equal up to that rounding
                             "max_abs_difference_from_numpy_median": float(np.max(np.abs(got - s_host)))}

    emit(__file__, {
        "repeats": a.repeats, "warmup": a.warmup,
        "workload": {"fs": FS, "nfft": NFFT, "seconds": a.seconds, "samples": n, "frames": m, "bins": BINS, "seed": a.seed,
                     "signal": "%d frames of bench.s_music repeated under a gliding tone" % a.period},
        "legs": res, "kernels": kern, "segment_median_alone": median, "device_copy_GBps": copy_bw,
        "period_found_is_the_true_one": used["F"][0] == a.period, "device_bytes": rp.stats()["device_bytes"],
    })


if __name__ == "__main__":
    main()
