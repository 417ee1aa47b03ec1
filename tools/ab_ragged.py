#!/usr/bin/env python3
"""A library of clips of unequal length through the offline engine, four ways, interleaved in one process (A B C D A B C D ...,
--repeats rounds after a warm-up), timed with HIP events on device-resident data; one JSON line.

Workload: --clips (64) clips at 44.1 kHz, lengths uniform in [--min-seconds, --max-seconds] (20 .. 40 s) from a fixed seed,
4096 / 256, beta 2, hard masks.
  A  one at a time: each clip alone through zen_hip_hpri_process_device on an n_clips == 1 handle
  B  one ragged call (zen_amd/ragged), n_clips = --clips
  C  sorted groups: ragged.plan_groups(lengths, --group) on a ragged handle of --group rows
  D  the ceiling: the equal-length call zen_hip_hpri_process_device on --clips x max(lengths) (NOT the same results: every
     row is treated as a clip of the longest length)
Reported: audio-seconds per second and milliseconds per leg with the repeat-to-repeat spread; from a second, profiled set of
rounds the event times of pack / splice / trim with their bytes and achieved GB/s next to the box's tuned copy kernel
(tools/ubench_copy, bench.py's HBM denominator), and the engines' per-class kernel times of B and D.
"requirement": the better of B and C is faster than A by more than A's spread (max - min).
On the GPU box, under a time limit of its own:  timeout -k 10 600 python tools/ab_ragged.py > ragged_ab.json"""
import numpy as np

from _ab import arguments, bench, class_ms, emit, kernels, timed, zen_amd
from zen_amd import ragged

FS = 44100.0


def summary(ts, audio_seconds):
    med = float(np.median(ts))
    return {"median_ms": med, "min_ms": float(min(ts)), "max_ms": float(max(ts)), "spread_ms": float(max(ts) - min(ts)),
            "runs": len(ts), "audio_seconds_per_second": audio_seconds / (med * 1e-3),
            "audio_seconds_per_second_min": audio_seconds / (max(ts) * 1e-3), "audio_seconds_per_second_max": audio_seconds / (min(ts) * 1e-3)}


def main():
    a = arguments(clips=64, group=16, min_seconds=20.0, max_seconds=40.0, hop_h=4096, hop_p=256, repeats=12, warmup=2, profiled=4, seed=20251)
    assert a.repeats >= 10, "at least 10 repeats per leg"
    copy = bench.tuned_copy_record()        # a process of its own, before this one opens the device
    zen_amd.init(0)
    ragged.load()
    rng = np.random.default_rng(a.seed)
    lens = [int(v) for v in rng.integers(int(a.min_seconds * FS), int(a.max_seconds * FS) + 1, a.clips)]
    C, mx = a.clips, max(lens)
    stride = -(-mx // 64) * 64
    base = bench.s_music(int((a.max_seconds + 65) * FS), seed=4242)
    host = np.zeros((C, stride), np.float32)
    for c, n in enumerate(lens):
        off = int(rng.integers(0, int(60 * FS)))
        host[c, :n] = base[off:off + n]
    inp = zen_amd.DeviceBuffer.from_host(host)
    out = {leg: [zen_amd.DeviceBuffer(C * stride) for _ in range(2)] for leg in "ABD"}
    audio_seconds = sum(lens) / FS
    mk = (FS, a.hop_h, a.hop_p, 2.0, 2.0)

    one = zen_amd.HPRIOffline(*mk, n_clips=1)
    rg_all = ragged.Ragged(*mk, n_clips=C)
    rg_grp = ragged.Ragged(*mk, n_clips=a.group)
    equal = zen_amd.HPRIOffline(*mk, n_clips=C)
    groups, fraction = ragged.plan_groups(lens, a.group)
    # leg C works on the library in sorted order: group g = rows [g * group, ...) of a sorted copy (what a caller that
    # loads its files in plan order has); the short last group, if any, is filled up with empty rows
    order = [i for g in groups for i in g]
    inp_sorted = zen_amd.DeviceBuffer.from_host(host[order])
    glens = [[lens[i] for i in g] + [0] * (a.group - len(g)) for g in groups]
    rows_c = -(-C // a.group) * a.group
    out["C"] = [zen_amd.DeviceBuffer(rows_c * stride) for _ in range(2)]
    inp_c = inp_sorted
    if rows_c != C:
        pad = np.zeros((rows_c, stride), np.float32)
        pad[:C] = host[order]
        inp_c = zen_amd.DeviceBuffer.from_host(pad)

    def leg_a():
        for c, n in enumerate(lens):
            one.process_device(inp.offset(c * stride), n, stride, harm=out["A"][0].offset(c * stride),
                               perc=out["A"][1].offset(c * stride), out_stride=stride)

    def leg_b():
        rg_all.process_device(inp.ptr, lens, stride, harm=out["B"][0].ptr, perc=out["B"][1].ptr, out_stride=stride)

    def leg_c():
        for g, gl in enumerate(glens):
            o = g * a.group * stride
            rg_grp.process_device(inp_c.offset(o), gl, stride, harm=out["C"][0].offset(o), perc=out["C"][1].offset(o), out_stride=stride)

    def leg_d():
        equal.process_device(inp.ptr, mx, stride, harm=out["D"][0].ptr, perc=out["D"][1].ptr, out_stride=stride)

    legs = (("A", leg_a), ("B", leg_b), ("C", leg_c), ("D", leg_d))
    for _ in range(a.warmup):
        for _, f in legs:
            f()
    zen_amd.synchronize()
    # same samples: every clip of B and of C against the clip alone (A)
    same = {}
    ref = [out["A"][k].download().reshape(C, stride) for k in range(2)]
    got_b = [out["B"][k].download().reshape(C, stride) for k in range(2)]
    got_c = [out["C"][k].download().reshape(rows_c, stride) for k in range(2)]
    same["B_equals_A"] = all(bool(np.array_equal(got_b[k][c, :n], ref[k][c, :n])) for k in range(2) for c, n in enumerate(lens))
    same["C_equals_A"] = all(bool(np.array_equal(got_c[k][r, :lens[c]], ref[k][c, :lens[c]])) for k in range(2) for r, c in enumerate(order))
    same["B_tails_zero"] = all(bool(np.all(got_b[k][c, n:mx] == 0)) for k in range(2) for c, n in enumerate(lens))
    del ref, got_b, got_c

    t = {name: [] for name, _ in legs}
    for _ in range(a.repeats):
        for name, f in legs:
            t[name].append(timed(f))
    res = {name: summary(ts, (C * mx / FS) if name == "D" else audio_seconds) for name, ts in t.items()}
    res["D"]["note"] = "audio seconds of D count every row at the longest length: what the equal-length call processes"

    # profiled rounds (events around every launch slow the calls down: kept apart from the timings above)
    rg_all.profile(True)
    rg_grp.profile(True)
    equal.profile(True)
    for _ in range(a.profiled):
        leg_b()
        leg_c()
        leg_d()
    kern = {}
    for name, h in (("B", rg_all), ("C", rg_grp)):
        kern[name] = kernels(h.profile_get(), a.profiled)
    eng = {"B": class_ms(rg_all.profile_get_engine(), a.profiled), "C": class_ms(rg_grp.profile_get_engine(), a.profiled),
           "D": class_ms(equal.profile_get_all(), a.profiled)}
    rg_all.profile(False)
    rg_grp.profile(False)
    equal.profile(False)

    tuned = max(copy.get("tuned_copy_median_shape_GBps", 0.0), copy.get("tuned_copy_1GiB_GBps", 0.0)) or None
    best = min(("B", "C"), key=lambda n: res[n]["median_ms"])
    b_minus_d = res["B"]["median_ms"] - res["D"]["median_ms"]
    engine_diff = eng["B"]["total_ms_per_round"] - eng["D"]["total_ms_per_round"]
    explained = kern["B"]["total_ms_per_round"] + engine_diff
    emit(__file__, {
        "repeats": a.repeats, "warmup": a.warmup,
        "workload": {"clips": C, "group": a.group, "hop_h": a.hop_h, "hop_p": a.hop_p, "beta": 2.0, "mask": "hard", "fs": FS,
                     "seed": a.seed, "min_samples": min(lens), "max_samples": mx, "audio_seconds": audio_seconds,
                     "padded_work_fraction_one_call": sum(lens) / (C * mx), "padded_work_fraction_sorted_groups": fraction,
                     "hops_B": rg_all.hop_counts(mx)},
        "legs": res, "same_samples": same,
        "speedup_over_A": {n: res["A"]["median_ms"] / res[n]["median_ms"] for n in ("B", "C", "D")},
        "requirement_best_of_B_C_beats_A_by_more_than_the_spread": bool(
            res[best]["median_ms"] < res["A"]["median_ms"] - max(res["A"]["spread_ms"], res[best]["spread_ms"])),
        "best_of_B_C": best,
        "new_kernels": kern, "tuned_copy_GBps": tuned, "tuned_copy_record": copy,
        "new_kernels_frac_of_tuned_copy_B": {kn: (kern["B"][kn]["GBps"] / tuned if tuned and kern["B"][kn]["GBps"] else None)
                                             for kn in ragged.KERNELS},
        "engine_class_ms_per_round": eng,
        "B_minus_D": {"wall_ms": b_minus_d, "new_kernels_ms": kern["B"]["total_ms_per_round"], "engine_kernels_B_minus_D_ms": engine_diff,
                      "explained_ms": explained, "unexplained_ms": b_minus_d - explained,
                      "spread_ms": max(res["B"]["spread_ms"], res["D"]["spread_ms"]),
                      "accounted_within_spread": bool(abs(b_minus_d - explained) <= max(res["B"]["spread_ms"], res["D"]["spread_ms"]))},
    })


if __name__ == "__main__":
    main()
