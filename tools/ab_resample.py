#!/usr/bin/env python3
"""Rate conversion and pitch shift (zen_amd/resample) on rows that are resident on the device, in one process; one JSON line.
GPU only: there is no fallback.

Workloads:
  batch   64 rows of 30 s, 48 kHz -> 44.1 kHz (147 / 160) and 44.1 kHz -> 48 kHz (160 / 147), at each quality, on the polyphase
          route and (a second handle, created under ZEN_HIP_RESAMPLE=poly=0) on the interpolating one.
  long    one row of three minutes at 44.1 kHz by the ratios of +3 and -3 semitones (55109 / 65536 and 4871 / 4096: both above
          the polyphase route's 4096 rows, so the interpolating route alone), at each quality.
Per workload the legs run in alternating rounds after a warm-up, each zen_hip_resample_run_device call between two HIP events.
Per leg: the median time, the bytes the call moves (windows in + outputs out) and their rate, as a share of the device copy
rate measured in the same run (bench.device_copy_bandwidth: the tuned copy kernel of tools/bin), the float operations of the
contract (2 T per output, 5 T on the interpolating route) and their rate -- which of the two roofs the kernel sits under and by
how much.
  model   the numpy model (tests/resample_model.py) on the first --model-seconds of a row, scaled to the long row.
  shift   the whole shift_hpr composition on three minutes at +3 semitones, device to device, with the share of each library:
          the separation (libzen_hip), the stretch (libzen_hip_tsm, overlap-add frame 2048 as tools/ab_tsm.py's long leg) and the
          resampler.
On the GPU box, under a time limit of its own:  timeout -k 10 900 python tools/ab_resample.py > profiles/resample_ab.json"""
import os
import time

import numpy as np

from _ab import arguments, bench, emit, summary, timed, zen_amd
from zen_amd import resample, tsm


def handle(num, den, quality, poly):
    if poly:
        return resample.Resampler(num, den, quality)
    os.environ["ZEN_HIP_RESAMPLE"] = "poly=0"
    try:
        return resample.Resampler(num, den, quality)
    finally:
        del os.environ["ZEN_HIP_RESAMPLE"]


def legs_of(name, x_dev, rows, n, ratios, routes, a, copy_bw, seconds):
    """every (ratio, quality, route) of a workload on the same device rows, in alternating rounds"""
    legs = {}
    out = zen_amd.DeviceBuffer(rows * max(resample.n_out(nu, de, n) for nu, de in ratios))
    for num, den in ratios:
        for q in resample.QUALITIES:
            for poly in routes:
                poly = poly and resample.geometry(num, den, q)[2] == resample.ROUTE_POLY
                key = "%d/%d q%d %s" % (num, den, q, "poly" if poly else "interp")
                if key in legs:
                    continue
                rs = handle(num, den, q, poly)
                no = rs.n_out(n)
                legs[key] = (rs, no, lambda rs=rs, no=no: rs.run_device(x_dev, n, 0, n, n, 0, no, out, no, rows))
    for _ in range(a.warmup):
        for _, _, run in legs.values():
            run()
    zen_amd.synchronize()
    t = {k: [] for k in legs}
    for _ in range(a.repeats):
        for k, (_, _, run) in legs.items():
            t[k].append(timed(run))
    res = {}
    for k, (rs, no, _) in legs.items():
        v = summary(t[k])
        st = rs.stats()
        route = "poly" if st["poly_calls"] else "interp"
        moved = 4 * rows * (n + no)
        flops = rows * no * rs.T * (2 if route == "poly" else 5)
        s = v["median_ms"] * 1e-3
        v.update({"ratio": [rs.num, rs.den], "quality": rs.quality, "route": route, "W": rs.W, "T": rs.T, "outputs_per_row": no,
                  "bytes_moved": moved, "GBps": moved / s / 1e9, "frac_of_device_copy": (moved / s / 1e9) / copy_bw if copy_bw else None,
                  "flops": flops, "TFLOPs": flops / s / 1e12, "Goutputs_per_s": rows * no / s / 1e9,
                  "times_real_time": rows * seconds / s, "table_bytes": st["device_bytes"]})
        res[k] = v
    return {"name": name, "rows": rows, "seconds": seconds, "samples": n, "legs": res}


def shift_leg(x, fs, semitones, a):
    """shift_hpr by hand, an event between the libraries"""
    hop, nfft, nfft_ola = 1024, 4096, 2048
    n = -(-x.size // hop) * hop
    xp = np.zeros(n, np.float32)
    xp[:x.size] = x
    num, den, alpha, m, k = resample.shift_plan(n, semitones)
    flags = zen_amd.OUTPUT_HARMONIC | zen_amd.OUTPUT_PERCUSSIVE | zen_amd.OUTPUT_RESIDUAL
    hpr = zen_amd.HPR(fs, hop, 2.5, flags, zen_amd.TIME_CAUSAL)
    ts = tsm.Tsm(fs, nfft, nfft_ola, 1, n, alpha)
    rs = resample.Resampler(num, den, 16)
    rows, mid, out = zen_amd.DeviceBuffer(4 * n), zen_amd.DeviceBuffer(m), zen_amd.DeviceBuffer(n)
    rows.upload(xp)
    out.zero()
    steps = {"separation": lambda: hpr.process(rows.ptr, n // hop, in_stride=n, harm=rows.offset(n), perc=rows.offset(2 * n), resid=rows.offset(3 * n),
                                               out_stride=n),
             "stretch": lambda: ts.hp_device(rows.offset(n), rows.offset(2 * n), rows.offset(3 * n), n, n, alpha, mid, m),
             "resample": lambda: rs.run_device(mid, m, 0, m, m, 0, k, out, n)}
    t = {s: [] for s in steps}
    for r in range(a.warmup + a.repeats):
        hpr.reset_buffers()
        for s, run in steps.items():
            v = timed(run)
            if r >= a.warmup:
                t[s].append(v)
    res = {s: summary(v) for s, v in t.items()}
    total = sum(v["median_ms"] for v in res.values())
    for v in res.values():
        v["share"] = v["median_ms"] / total
    return {"semitones": semitones, "ratio": [num, den], "alpha": alpha, "samples": n, "stretched": m, "resampled": k, "nfft": nfft,
            "nfft_ola": nfft_ola, "hpr_hop": hop, "steps": res, "total_ms": total, "times_real_time": (n / fs) / (total * 1e-3)}


def main():
    a = arguments(batch_seconds=30.0, batch_rows=64, long_seconds=180.0, repeats=7, warmup=2, model_seconds=2.0, seed=4242)
    zen_amd.init(0)
    copy_bw = bench.device_copy_bandwidth(zen_amd)
    work = []
    # batch: 30 s rows at 48 kHz going down; the same device memory read as 30 s rows at 44.1 kHz going up
    n = int(a.batch_seconds * 48000)
    one = bench.s_music(n, seed=a.seed, fs=48000.0)
    x = np.stack([np.roll(one, 997 * r) for r in range(a.batch_rows)])
    d = zen_amd.DeviceBuffer.from_host(x)
    work.append(legs_of("batch 48k -> 44.1k", d, a.batch_rows, n, [(147, 160)], (True, False), a, copy_bw, a.batch_seconds))
    n_up = int(a.batch_seconds * 44100)
    work.append(legs_of("batch 44.1k -> 48k", d, a.batch_rows, n_up, [(160, 147)], (True, False), a, copy_bw, a.batch_seconds))
    d.free()
    n_long = int(a.long_seconds * 44100)
    xl = bench.s_music(n_long, seed=a.seed + 1)
    d = zen_amd.DeviceBuffer.from_host(xl)
    ratios = [resample.ratio_for_shift(3), resample.ratio_for_shift(-3)]
    long = legs_of("long +-3 semitones", d, 1, n_long, ratios, (True,), a, copy_bw, a.long_seconds)
    work.append(long)
    d.free()
    import resample_model
    cut = xl[:int(a.model_seconds * 44100)]
    t0 = time.perf_counter()
    resample_model.resample(cut, ratios[0][0], ratios[0][1], 16)
    model_s = time.perf_counter() - t0
    device_ms = long["legs"]["%d/%d q16 interp" % ratios[0]]["median_ms"]
    emit(__file__, {
        "repeats": a.repeats, "warmup": a.warmup, "seed": a.seed,
        "device_copy_GBps": copy_bw, "tile": resample.TILE, "workloads": work, "shift_hpr": shift_leg(xl, 44100.0, 3, a),
        "host_model": {"seconds_of_audio": a.model_seconds, "wall_s": model_s, "scaled_to_the_long_row_s": model_s * a.long_seconds / a.model_seconds,
                       "over_the_device_call": model_s * a.long_seconds / a.model_seconds / (device_ms * 1e-3)},
    })


if __name__ == "__main__":
    main()
