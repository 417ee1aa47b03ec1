#!/usr/bin/env python3
"""The beat tracker (zen_amd/beat) on audio that is resident on the device, in one process; one JSON line.

Workloads at 44.1 kHz, hop 512, from one minute of the project's test signal (bench.s_music) with a click every 0.5 s on top,
repeated:
  B  64 streams of --batch-seconds (30) in one session (each stream starts --skew samples further into the signal)
  H  one stream of --seconds (3600): 310 078 hops, slices of 4096
     Legs B and H are interleaved (B H B H ...), --repeats rounds after a warm-up, each round a reset and one
     zen_hip_beat_run_device call with all four results, timed with HIP events.  Before that, in the same run, the results are
     compared bit for bit with tests/beat_model.py: the onset function on every --check-every-th hop of every stream (the
     model of one hop needs the three hops in front of it only), and score, beat and tempo on every hop of the first and the
     last stream of B and of the first --model-hops hops of H (the tracker's model walks the device's onset row from the start).
     From a second, profiled set of rounds: the event times of frame / FFT / csd / track with their bytes and achieved GB/s,
     and the track kernel's time per hop and per tempo estimate (all of its time over the beats: an upper bound).
  D  device time of one hop through the whole chain, one stream: --calls (2000) single-hop zen_hip_beat_run_device calls after
     --call-warmup (200), each between two HIP events.
  C  wall time of one hop through zen_hip_beat_run_host, pinned host to pinned host, the same number of calls.
"condition": one hop completes on the device within its own duration (512 / fs = 11.6 ms) at the MAXIMUM over leg D.
On the GPU box, under a time limit of its own:  timeout -k 10 600 python tools/ab_beat.py > beat_ab.json"""
import time

import numpy as np

from _ab import arguments, bench, emit, kernels, per_call, summary, timed, zen_amd
import beat_model
from zen_amd import beat

FS, HOP = 44100.0, 512


def same_bits(a, b):
    return bool(np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32)))


def check_onsets(x, odf, every):
    """the device's onset values of one stream against the model of single hops: hop t from the hops t-3 .. t alone (two hops
    of run-in give the model its two earlier spectra; in front of the stream there are zeros either way)"""
    ok, n = True, 0
    for t in range(0, odf.size, every):
        lo = max(0, t - 3)
        lead = np.zeros((3 - (t - lo)) * HOP, np.float32)
        got = beat_model.Onset(FS, HOP).run(np.concatenate([lead, x[lo * HOP:(t + 1) * HOP]]))[-1]
        ok &= same_bits(got, odf[t])
        n += 1
    return ok, n


def check_tracker(odf, score, flag, tempo):
    want = beat_model.Tracker(FS, HOP).run(odf)
    return same_bits(want[0], score) and same_bits(want[1], flag) and same_bits(want[2], tempo)


def main():
    a = arguments(seconds=3600.0, batch_seconds=30.0, streams=64, skew=7919, repeats=10, warmup=2, profiled=2, calls=2000, call_warmup=200,
                  check_every=97, model_hops=20000, seed=4242)
    zen_amd.init(0)
    L = beat.load()
    S = a.streams
    hb, hh = int(a.batch_seconds * FS) // HOP, int(a.seconds * FS) // HOP
    minute = bench.s_music(int(60 * FS), seed=a.seed).astype(np.float32)
    minute[::int(0.5 * FS)] += 0.8
    xh = np.tile(minute, -(-hh * HOP // minute.size))[:hh * HOP]
    xb = np.stack([xh[s * a.skew:s * a.skew + hb * HOP] for s in range(S)])

    legs = {}
    for name, x, n_streams, hops in (("B", xb, S, hb), ("H", xh[None], 1, hh)):
        bt = beat.Beat(FS, HOP, n_streams=n_streams)
        inp = zen_amd.DeviceBuffer.from_host(x)
        outs = [zen_amd.DeviceBuffer(n_streams * hops) for _ in range(4)]

        def run(bt=bt, inp=inp, outs=outs, hops=hops):
            bt.reset()
            bt.run_device(inp, hops * HOP, hops, *outs, out_stride=hops)
        legs[name] = {"beat": bt, "run": run, "outs": outs, "x": x, "hops": hops, "streams": n_streams, "in": inp}

    # the same bits as the model
    same = {}
    for name, g in legs.items():
        g["run"]()
        zen_amd.synchronize()
        got = [o.download().reshape(g["streams"], g["hops"]) for o in g["outs"]]
        ok, n = True, 0
        for s in range(g["streams"]):
            o, c = check_onsets(g["x"][s], got[0][s], a.check_every)
            ok, n = ok and o, n + c
        m = min(a.model_hops, g["hops"])
        rows = sorted({0, g["streams"] - 1})
        same[name] = {"onset_hops_checked": n, "onset": ok, "tracker_streams_checked": rows, "tracker_hops_each": m,
                      "tracker": all(check_tracker(got[0][s][:m], got[1][s][:m], got[2][s][:m], got[3][s][:m]) for s in rows)}
        g["beats"] = int(got[2].sum())
        g["tempo_median"] = float(np.median(got[3]))

    for _ in range(a.warmup):
        for g in legs.values():
            g["run"]()
    zen_amd.synchronize()
    t = {k: [] for k in legs}
    for _ in range(a.repeats):
        for k, g in legs.items():
            t[k].append(timed(g["run"]))
    res = {k: summary(v) for k, v in t.items()}
    for k, v in res.items():
        g = legs[k]
        v["times_real_time"] = g["streams"] * g["hops"] * HOP / FS / (v["median_ms"] * 1e-3)
        v["hops_per_s"] = g["streams"] * g["hops"] / (v["median_ms"] * 1e-3)
        v["hops"], v["streams"], v["beats"], v["tempo_median"] = g["hops"], g["streams"], g["beats"], g["tempo_median"]

    # profiled rounds (events around every launch slow the calls down: kept apart from the timings above)
    kern = {}
    for k, g in legs.items():
        g["beat"].profile(True)
        for _ in range(a.profiled):
            g["run"]()
        kern[k] = kernels(g["beat"].profile_get(), a.profiled)
        g["beat"].profile(False)
        tr = kern[k]["track"]["ms_per_round"]
        # one workgroup per stream walks its hops: the streams of B run side by side, so per hop of a stream
        kern[k]["track_us_per_hop_of_a_stream"] = 1e3 * tr / g["hops"]
        kern[k]["track_us_per_tempo_estimate_upper_bound"] = 1e3 * tr / max(1, g["beats"] // g["streams"])
    device_bytes = {k: g["beat"].stats()["device_bytes"] for k, g in legs.items()}
    legs.clear()

    # legs D and C: one hop at a time
    hop_ms = 1e3 * HOP / FS
    one = beat.Beat(FS, HOP, max_hops=1)
    inp = zen_amd.DeviceBuffer.from_host(xh[:(a.call_warmup + a.calls) * HOP])
    outs = [zen_amd.DeviceBuffer(1) for _ in range(4)]
    td = []
    for i in range(a.call_warmup + a.calls):
        td.append(timed(lambda: one.run_device(inp.offset(i * HOP), HOP, 1, *outs, out_stride=1)))
        zen_amd.synchronize()
    leg_d = per_call(td[a.call_warmup:], hop_ms)
    one.reset()
    pin_in, pin_out = zen_amd.PinnedHost(HOP), zen_amd.PinnedHost(4)
    ptr = [pin_out.array.ctypes.data + 4 * k for k in range(4)]
    tc = []
    for i in range(a.call_warmup + a.calls):
        pin_in.array[:] = xh[i * HOP:(i + 1) * HOP]
        t0 = time.perf_counter()
        rc = L.zen_hip_beat_run_host(one._h, pin_in.array.ctypes.data, HOP, 1, ptr[0], ptr[1], ptr[2], ptr[3], 1)
        t1 = time.perf_counter()
        assert rc == 0, L.zen_hip_beat_last_error()
        tc.append(1e3 * (t1 - t0))
    leg_c = per_call(tc[a.call_warmup:], hop_ms, within=False)

    emit(__file__, {
        "repeats": a.repeats, "warmup": a.warmup,
        "workload": {"fs": FS, "hop": HOP, "seconds": a.seconds, "batch_seconds": a.batch_seconds, "streams": S, "skew": a.skew, "seed": a.seed,
                     "signal": "one minute of bench.s_music with a click every 0.5 s, repeated"},
        "legs": res, "same_bits_as_the_model": same, "kernels": kern,
        "one_hop_device": leg_d, "one_hop_run_host_wall": leg_c,
        "condition_one_hop_within_its_duration_at_the_maximum": leg_d["within_the_hop_at_the_maximum"],
        "device_bytes": device_bytes,
    })


if __name__ == "__main__":
    main()
