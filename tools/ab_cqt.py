#!/usr/bin/env python3
"""The constant-Q add-on (zen_amd/cqt) on a clip that is resident on the device, in one process; one JSON line.

Workload: 30 s of mono audio at 44.1 kHz (the project's test signal, bench.s_music), slice 16384, 12 bands per octave from
60 Hz: 163 slices of about a hundred bands of 1024 coefficients, some 130 MB of coefficients.
  S3    one zen_hip_cqt_separate_device call, all three stems, hard masks
  S1    the same with the harmonic stem alone
  SOFT  the three stems with the soft masks (the residual is not synthesised)
  F     zen_hip_cqt_forward_device alone (steps 1-2 and the copy into the caller's buffer)
  I     zen_hip_cqt_inverse_device alone on those coefficients
        The legs are interleaved (S3 S1 SOFT F I S3 ...), --repeats rounds after a warm-up, each between two HIP events; every
        leg is quoted as a multiple of real time.
From a second, profiled set of S3 rounds: the event times of every step with its bytes and achieved GB/s, and for the six
kernels of this library (slice, fold, overlap, mask, gather, overlap_add) that rate against the device copy rate bench.py
measures on the same box (tools/ubench_copy.hip).  The transforms and the medians are the engine's kernels and are listed
with their times only.
On the GPU box, under a time limit of its own:  timeout -k 10 600 python tools/ab_cqt.py > profiles/cqt_ab.json"""
import numpy as np

from _ab import arguments, bench, emit, summary, timed, zen_amd
from zen_amd import cqt

OWN = ("slice", "fold", "overlap", "mask", "gather", "overlap_add")


def main():
    a = arguments(seconds=30.0, fs=44100.0, slice=16384, bpo=12, fmin=60.0, repeats=10, warmup=2, profiled=3, seed=4242)
    zen_amd.init(0)
    n = int(a.seconds * a.fs)
    x = bench.s_music(n, seed=a.seed).astype(np.float32)
    cq = cqt.Cqt(a.fs, a.slice, a.bpo, a.fmin, 1, n)
    sh = cq.shape()
    inp = zen_amd.DeviceBuffer.from_host(x)
    stems = [zen_amd.DeviceBuffer(n) for _ in range(3)]
    back = zen_amd.DeviceBuffer(n)
    coef = zen_amd.DeviceBuffer(sh["slices"] * sh["bands"] * sh["m"], np.complex64)

    def s3():
        cq.set_params(soft=False)
        cq.separate_device(inp, n, stems[0], stems[1], stems[2], n)

    def s1():
        cq.set_params(soft=False)
        cq.separate_device(inp, n, stems[0], None, None, n)

    def soft():
        cq.set_params(soft=True)
        cq.separate_device(inp, n, stems[0], stems[1], stems[2], n)

    legs = {"S3": s3, "S1": s1, "SOFT": soft, "F": lambda: cq.forward_device(inp, n, coef), "I": lambda: cq.inverse_device(coef, back, n)}
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
        v["times_real_time"] = a.seconds / (v["median_ms"] * 1e-3)
    round_trip = float(np.max(np.abs(back.download() - x)))

    copy_bw = bench.device_copy_bandwidth(zen_amd)
    cq.profile(True)            # events around every launch slow the calls down: kept apart from the timings above
    for _ in range(a.profiled):
        s3()
    prof = cq.profile_get()
    cq.profile(False)
    kern = {}
    for name, v in prof.items():
        gbps = (v["bytes"] / (v["ms"] * 1e-3) / 1e9) if v["ms"] > 0 else None
        kern[name] = {"ms_per_call": v["ms"] / a.profiled, "launches_per_call": v["launches"] // a.profiled, "own_kernel": name in OWN}
        if name in OWN:
            kern[name].update({"bytes_per_call": v["bytes"] // a.profiled, "GBps": gbps,
                               "frac_of_device_copy": gbps / copy_bw if gbps and copy_bw else None})
    kern["total_ms_per_call"] = sum(v["ms"] for v in prof.values()) / a.profiled

    emit(__file__, {
        "repeats": a.repeats, "warmup": a.warmup,
        "workload": {"fs": a.fs, "slice": a.slice, "bands_per_octave": a.bpo, "fmin": a.fmin, "seconds": a.seconds, "samples": n, "seed": a.seed,
                     "signal": "bench.s_music", "shape": sh, "coefficient_bytes": 8 * sh["slices"] * sh["bands"] * sh["m"]},
        "legs": res, "kernels_of_S3": kern, "device_copy_GBps": copy_bw, "round_trip_max_abs_error": round_trip,
        "device_bytes": cq.stats()["device_bytes"],
    })


if __name__ == "__main__":
    main()
