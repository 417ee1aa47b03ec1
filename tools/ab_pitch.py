#!/usr/bin/env python3
"""The pitch tracker (zen_amd/pitch) on an hour of audio that is resident on the device, in one process; one JSON line.

Workload: --seconds (3600) at 44.1 kHz, chunks of 4096 (38 759 of them): one minute of the project's test signal (bench.s_music)
repeated -- a minute is no whole number of chunks, so the chunks differ.
  P  the tracker alone on the samples: one zen_hip_pitch_run_device call, all three results
  T  track_hpr: zen_hip_hpr_process (causal, hop 4096, beta 2.5, harmonic output) and the tracker on both rows (samples and
     harmonic stream), one call each
     Legs P and T are interleaved (P T P T ...), --repeats rounds after a warm-up, timed with HIP events.  Before that, in the
     same run, P's three results and T's two pitch rows are compared bit for bit with tests/pitch_model.py on every
     --check-every-th chunk (the model takes milliseconds per chunk; for T the model's input is the harmonic stream
     downloaded from the device, which the GPU tier pins to the oracle).  From a second, profiled set of rounds: the event
     times of pad / forward FFT / power / inverse FFT / pick with their bytes and achieved GB/s next to the box's tuned copy
     kernel (tools/ubench_copy, bench.py's HBM denominator), and for T the engine's per-class kernel times.
  C  wall time of one chunk through zen_hip_pitch_run_host, pinned host to pinned host: --calls (2000) after --call-warmup (200);
     median, 99th percentile, maximum.
"condition": one chunk completes within its own duration (4096 / fs = 92.9 ms) at the MAXIMUM over leg C's run.
On the GPU box, under a time limit of its own:  timeout -k 10 600 python tools/ab_pitch.py > pitch_ab.json"""
import time

import numpy as np

from _ab import arguments, bench, emit, kernels, summary, timed, zen_amd
import pitch_model
from zen_amd import pitch

FS = 44100.0


def main():
    a = arguments(seconds=3600.0, chunk=4096, beta=2.5, repeats=10, warmup=2, profiled=2, calls=2000, call_warmup=200, check_every=97, seed=4242)
    assert a.repeats >= 10 and a.calls >= 2000 and a.call_warmup >= 200
    copy = bench.tuned_copy_record()        # a process of its own, before this one opens the device
    zen_amd.init(0)
    L = pitch.load()
    n = a.chunk
    cnt = int(a.seconds * FS) // n
    minute = bench.s_music(int(60 * FS), seed=a.seed)
    x = np.tile(minute, -(-cnt * n // minute.size))[:cnt * n]

    alone = pitch.Pitch(FS, n)
    inp = zen_amd.DeviceBuffer.from_host(x)
    out_p = [zen_amd.DeviceBuffer(cnt) for _ in range(3)]
    both = pitch.HprTracker(FS, n, a.beta, max_chunks=cnt)
    both.upload(x)

    def leg_p():
        alone.run_device(inp, cnt * n, cnt, n, *out_p, out_stride=cnt)

    def leg_t():
        both.run_device(cnt)

    # the same bits as the model, on every check_every-th chunk
    leg_p()
    leg_t()
    zen_amd.synchronize()
    got_p = [o.download() for o in out_p]
    got_with, got_without = both.download(cnt)
    harm = both.rows.download()[cnt * n:]
    picked = list(range(0, cnt, a.check_every))
    same = {"chunks_checked": len(picked), "pitch": True, "period": True, "clarity": True, "track_hpr_with": True, "track_hpr_without": True}
    for c in picked:
        want = pitch_model.chunk(x[c * n:(c + 1) * n], FS)
        for k, name in enumerate(("pitch", "period", "clarity")):
            same[name] &= bool(got_p[k][c:c + 1].view(np.uint32)[0] == np.float32(want[k]).view(np.uint32))
        same["track_hpr_without"] &= bool(got_without[c:c + 1].view(np.uint32)[0] == np.float32(want[0]).view(np.uint32))
        want_h = pitch_model.chunk(harm[c * n:(c + 1) * n], FS)
        same["track_hpr_with"] &= bool(got_with[c:c + 1].view(np.uint32)[0] == np.float32(want_h[0]).view(np.uint32))
    found = {"P": float(np.mean(got_p[0] > 0)), "T_with": float(np.mean(got_with > 0)), "T_without": float(np.mean(got_without > 0))}
    del harm, got_p

    for _ in range(a.warmup):
        leg_p()
        leg_t()
    zen_amd.synchronize()
    t = {"P": [], "T": []}
    for _ in range(a.repeats):
        t["P"].append(timed(leg_p))
        t["T"].append(timed(leg_t))
    res = {k: summary(v) for k, v in t.items()}
    for k, v in res.items():
        v["times_real_time"] = cnt * n / FS / (v["median_ms"] * 1e-3)
        v["chunks_per_s"] = cnt * (1 if k == "P" else 2) / (v["median_ms"] * 1e-3)

    # profiled rounds (events around every launch slow the calls down: kept apart from the timings above)
    alone.profile(True)
    both.pitch.profile(True)
    both.hpr.profile(True)
    for _ in range(a.profiled):
        leg_p()
        leg_t()
    kern = {"P": kernels(alone.profile_get(), a.profiled), "T": kernels(both.pitch.profile_get(), a.profiled)}
    eng = {k: v["ms"] / a.profiled for k, v in both.hpr.profile_get_all().items() if v["launches"]}
    alone.profile(False)
    both.pitch.profile(False)
    both.hpr.profile(False)
    tuned = max(copy.get("tuned_copy_median_shape_GBps", 0.0), copy.get("tuned_copy_1GiB_GBps", 0.0)) or None
    device_bytes = {"P": alone.stats()["device_bytes"], "T_tracker": both.pitch.stats()["device_bytes"]}
    del both, alone, inp, out_p

    # leg C: wall time of one chunk, pinned host to pinned host
    chunk_ms = 1e3 * n / FS
    one = pitch.Pitch(FS, n, max_chunks=1)
    pin_in = zen_amd.PinnedHost(n)
    pin_out = zen_amd.PinnedHost(3)
    ptr = [pin_out.array.ctypes.data + 4 * k for k in range(3)]
    ts = []
    for i in range(a.call_warmup + a.calls):
        off = (i * n + 7919 * i) % (x.size - n)
        pin_in.array[:] = x[off:off + n]
        t0 = time.perf_counter()
        rc = L.zen_hip_pitch_run_host(one._h, pin_in.array.ctypes.data, n, 1, n, ptr[0], ptr[1], ptr[2], None, 1)
        t1 = time.perf_counter()
        assert rc == 0, L.zen_hip_pitch_last_error()
        ts.append(1e3 * (t1 - t0))
    ts = np.array(ts[a.call_warmup:])
    leg_c = {"calls": int(ts.size), "median_ms": float(np.median(ts)), "p99_ms": float(np.percentile(ts, 99)), "max_ms": float(ts.max()),
             "chunk_ms": chunk_ms, "max_over_chunk": float(ts.max() / chunk_ms), "within_the_chunk_at_the_maximum": bool(ts.max() < chunk_ms)}

    emit(__file__, {
        "repeats": a.repeats, "warmup": a.warmup,
        "workload": {"seconds": a.seconds, "chunks": cnt, "chunk": n, "fs": FS, "beta": a.beta, "seed": a.seed,
                     "signal": "one minute of bench.s_music, repeated"},
        "legs": res, "same_bits_as_the_model": same, "share_of_chunks_with_a_pitch": found,
        "kernels": kern, "tuned_copy_GBps": tuned, "tuned_copy_record": copy,
        "kernels_frac_of_tuned_copy": {leg: {kn: (kern[leg][kn]["GBps"] / tuned if tuned and kern[leg][kn]["GBps"] else None)
                                             for kn in pitch.KERNELS} for leg in kern},
        "T_engine_class_ms_per_round": eng,
        "one_chunk_run_host_wall": leg_c,
        "condition_one_chunk_within_its_duration_at_the_maximum": leg_c["within_the_chunk_at_the_maximum"],
        "device_bytes": device_bytes,
    })


if __name__ == "__main__":
    main()
