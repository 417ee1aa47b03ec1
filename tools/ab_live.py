#!/usr/bin/env python3
"""The two-pass separation as a live session (zen_amd/live) against the whole-clip call, in one process; one JSON line.

Workload: one clip of --seconds (600) at 44.1 kHz from a fixed seed, 4096 / 256, beta 2, hard masks.
  A  the whole clip through zen_hip_hpri_process_device on an n_clips == 1 handle: the yardstick
  B  the same clip through a device-resident session, in pushes of hop_h, 8 * hop_h, 1 s and 10 s, plus finish; one session
     per push size, sized for it (max_push = the push)
     Legs A and B are interleaved (A B1 B2 B3 B4 A ...), --repeats rounds after a warm-up, timed with HIP events; B's
     outputs are compared with A's in the same run.  From a second, profiled set of rounds: the event times of feed / mid /
     out with their bytes and achieved GB/s next to the box's tuned copy kernel (tools/ubench_copy, bench.py's HBM
     denominator), and the engines' per-class kernel times of A and of every B.
  C  per-push wall time of zen_hip_live_push_host, pinned host to pinned host, pushes of hop_h, for 1 and 2 streams:
     --pushes (2000) after --push-warmup (200); median, 99th percentile, maximum.
"condition": a push of hop_h completes within the hop's own duration (hop_h / fs) at the MAXIMUM over leg C's run.
Also: device_bytes of a session at max_push = hop_h and at 1 s.
On the GPU box, under a time limit of its own:  timeout -k 10 600 python tools/ab_live.py > live_ab.json"""
import ctypes as C
import time

import numpy as np

from _ab import arguments, bench, class_ms, emit, kernels, per_call, summary, timed, zen_amd
from zen_amd import live

FS = 44100.0


def main():
    a = arguments(seconds=600.0, hop_h=4096, hop_p=256, repeats=10, warmup=2, profiled=2, pushes=2000, push_warmup=200, seed=4242)
    assert a.repeats >= 10 and a.pushes >= 2000 and a.push_warmup >= 200
    copy = bench.tuned_copy_record()        # a process of its own, before this one opens the device
    zen_amd.init(0)
    L = live.load()
    n, hop = int(a.seconds * FS), a.hop_h
    x = bench.s_music(n, seed=a.seed)
    inp = zen_amd.DeviceBuffer.from_host(x)
    mk = (FS, a.hop_h, a.hop_p, 2.0, 2.0)
    sizes = {"hop_h": hop, "8_hop_h": 8 * hop, "1_s": int(FS), "10_s": int(10 * FS)}

    offline = zen_amd.HPRIOffline(*mk, n_clips=1)
    out_a = [zen_amd.DeviceBuffer(n) for _ in range(2)]
    sessions = {name: live.Live(*mk, max_push=m) for name, m in sizes.items()}
    out_b = [zen_amd.DeviceBuffer(n) for _ in range(3)]          # shared by the four B legs: compared after each warm-up run

    def leg_a():
        offline.process_device(inp.ptr, n, n, harm=out_a[0].ptr, perc=out_a[1].ptr)

    def leg_b(name):
        lv, m = sessions[name], sizes[name]
        at = tot = 0
        while at < n:
            mm = min(m, n - at)
            tot += lv.push_device(inp.offset(at), mm, n, *(o.offset(tot) for o in out_b), out_stride=n)
            at += mm
        tot += lv.finish_device(*(o.offset(tot) for o in out_b), out_stride=n)
        assert tot == n

    leg_a()
    zen_amd.synchronize()
    ref = [o.download() for o in out_a]
    same = {}
    for name in sizes:
        for o in out_b:
            o.zero()
        leg_b(name)
        zen_amd.synchronize()
        same[name] = {"harm": bool(np.array_equal(out_b[0].download(), ref[0])), "perc": bool(np.array_equal(out_b[1].download(), ref[1])),
                      "dry": bool(np.array_equal(out_b[2].download(), x))}
    del ref
    for _ in range(a.warmup):
        leg_a()
        for name in sizes:
            leg_b(name)
    zen_amd.synchronize()

    t = {"A": []}
    t.update({name: [] for name in sizes})
    for _ in range(a.repeats):
        t["A"].append(timed(leg_a))
        for name in sizes:
            t[name].append(timed(lambda: leg_b(name)))
    res = {k: summary(v) for k, v in t.items()}
    for k, v in res.items():
        v["times_real_time"] = a.seconds / (v["median_ms"] * 1e-3)
    ratio = {name: {"B_over_A": res[name]["median_ms"] / res["A"]["median_ms"], "pushes": -(-n // sizes[name]),
                    "us_per_push": 1e3 * res[name]["median_ms"] / -(-n // sizes[name])} for name in sizes}

    # profiled rounds (events around every launch slow the calls down: kept apart from the timings above)
    offline.profile(True)
    for _ in range(a.profiled):
        leg_a()
    eng = {"A": class_ms(offline.profile_get_all(), a.profiled)}
    offline.profile(False)
    kern = {}
    for name, lv in sessions.items():
        lv.profile(True)
        for _ in range(a.profiled):
            leg_b(name)
        kern[name] = kernels(lv.profile_get(), a.profiled)
        eng[name] = class_ms(lv.profile_get_engine(), a.profiled)
        lv.profile(False)
    tuned = max(copy.get("tuned_copy_median_shape_GBps", 0.0), copy.get("tuned_copy_1GiB_GBps", 0.0)) or None
    device_bytes = {"max_push_hop_h": sessions["hop_h"].stats()["device_bytes"], "max_push_1_s": sessions["1_s"].stats()["device_bytes"]}
    del sessions, out_a, out_b

    # leg C: wall time per push, pinned host to pinned host
    hop_ms = 1e3 * hop / FS
    leg_c = {}
    for S in (1, 2):
        lv = live.Live(*mk, n_streams=S, max_push=hop)
        pin_in = zen_amd.PinnedHost(S * hop)
        pin_out = [zen_amd.PinnedHost(S * hop) for _ in range(3)]
        ptr = [p.array.ctypes.data for p in pin_out]
        got = C.c_size_t()
        ts = []
        for i in range(a.push_warmup + a.pushes):
            for s in range(S):
                off = ((i * hop) + s * 7919) % (n - hop)
                pin_in.array[s * hop:(s + 1) * hop] = x[off:off + hop]
            t0 = time.perf_counter()
            rc = L.zen_hip_live_push_host(lv._h, pin_in.array.ctypes.data, hop, hop, ptr[0], ptr[1], ptr[2], hop, C.byref(got))
            t1 = time.perf_counter()
            assert rc == 0, L.zen_hip_live_last_error()
            ts.append(1e3 * (t1 - t0))
        assert got.value == hop
        leg_c["%d_stream%s" % (S, "s" if S > 1 else "")] = per_call(ts[a.push_warmup:], hop_ms, "pushes")
        del lv

    emit(__file__, {
        "repeats": a.repeats, "warmup": a.warmup,
        "workload": {"seconds": a.seconds, "samples": n, "hop_h": a.hop_h, "hop_p": a.hop_p, "beta": 2.0, "mask": "hard", "fs": FS,
                     "seed": a.seed, "push_samples": sizes},
        "legs": res, "B_over_A": ratio, "same_samples_as_A": same,
        "new_kernels": kern, "tuned_copy_GBps": tuned, "tuned_copy_record": copy,
        "new_kernels_frac_of_tuned_copy": {name: {kn: (kern[name][kn]["GBps"] / tuned if tuned and kern[name][kn]["GBps"] else None)
                                                  for kn in live.KERNELS} for name in sizes},
        "engine_class_ms_per_round": eng,
        "per_push_wall": leg_c,
        "condition_push_of_hop_h_within_the_hop_at_the_maximum": all(v["within_the_hop_at_the_maximum"] for v in leg_c.values()),
        "device_bytes": device_bytes,
    })


if __name__ == "__main__":
    main()
