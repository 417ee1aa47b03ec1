#!/usr/bin/env python3
"""The REPET-SIM add-on (zen_amd/repsim) on a clip that is resident on the device, in one process; one JSON line.

Workload: three minutes of mono audio at 44.1 kHz (the project's test signal, bench.s_music), frame 2048: 7753 frames of
1025 bins, the library's defaults (t = 0, one second apart, k = 100, high-pass 100 Hz).
  W     one zen_hip_repsim_separate_device call, both stems, the similarity on the matrix cores
  WV    the same in a session created under ZEN_HIP_REPSIM="mfma=0": the similarity on the vector ALU
  SM    zen_hip_repsim_similarity_device alone on the clip's V, the matrix-core route
  SV    the same, the vector route
  SEL   zen_hip_repsim_select_device alone on that S
  GM    zen_hip_repsim_gather_median_device alone on V and that selection
        The legs are interleaved (W WV SM SV SEL GM W ...), --repeats rounds after a warm-up, each between two HIP events.
SM and SV are quoted in TFLOP/s, counting 2 m^2 bins, against 122 TFLOP/s (the figure quoted for an untuned LDS-tiled f32
GEMM on the same instruction) and the 157.3 TFLOP/s peak of the f32 matrix and vector rate.
GM is quoted against the device copy rate bench.py measures on the same box (tools/ubench_copy.hip) by the bytes it gathers
and writes; V itself is 32 MB and stays in the caches, so that is a rate of cache reads, not of memory traffic.
From a second, profiled set of W rounds: the event times of every step.
The host route, once: V copied to the host, S = V V^T over the norms in numpy (float32, the BLAS numpy has), the selection
and the medians of the first --host-frames frames in numpy (the seconds for all frames are those times m / host_frames), U
copied back.
On the GPU box, under a time limit of its own:  timeout -k 10 600 python tools/ab_repsim.py > profiles/repsim_ab.json"""
import os
import time

import numpy as np

from _ab import arguments, bench, emit, summary, timed, zen_amd
from zen_amd import repsim

GUIDE_TFLOPS, PEAK_TFLOPS = 122.0, 157.3


def host_select(S, dd, k):
    rows, m = S.shape
    idx, counts = np.full((rows, k), -1, np.int32), np.zeros(rows, np.int32)
    cand = np.where(S > 0, S, -np.inf).astype(np.float32)
    cols, every = np.arange(m), np.arange(rows)
    for c in range(k):
        j = np.argmax(cand, axis=1)
        live = cand[every, j] > -np.inf
        if not live.any():
            break
        idx[live, c] = j[live]
        counts += live
        cand[live[:, None] & (np.abs(cols[None, :] - j[:, None]) < dd)] = -np.inf
    return idx, counts


def main():
    a = arguments(seconds=180.0, fs=44100.0, nfft=2048, repeats=10, warmup=2, profiled=3, host_frames=512, seed=4242)
    zen_amd.init(0)
    n, H = int(a.seconds * a.fs), a.nfft // 2
    bins, m = H + 1, repsim.n_frames(n, a.nfft)
    k, dd = repsim.NUMBER, max(1, int(np.ceil(repsim.DISTANCE * a.fs / H)))
    x = bench.s_music(n, seed=a.seed).astype(np.float32)
    rs = repsim.Repsim(a.fs, a.nfft, 1, n)
    os.environ["ZEN_HIP_REPSIM"] = "mfma=0"
    rv = repsim.Repsim(a.fs, a.nfft, 1, n)
    del os.environ["ZEN_HIP_REPSIM"]
    inp = zen_amd.DeviceBuffer.from_host(x)
    bg, fg = zen_amd.DeviceBuffer(n), zen_amd.DeviceBuffer(n)
    # the kernels alone work on a V of the clip made here (numpy's transform: close to the library's, not its bits)
    xp = np.zeros((m + 1) * H, np.float32)
    xp[H:H + n] = x
    w = repsim.table(a.nfft, repsim.TABLE_WINDOW)
    frames = np.lib.stride_tricks.as_strided(xp, (m, a.nfft), (4 * H, 4))
    v_stride = (bins + 3) & ~3
    V = np.zeros((m, v_stride), np.float32)
    V[:, :bins] = np.abs(np.fft.rfft(frames * w, axis=1)).astype(np.float32)
    s_stride = (m + 3) & ~3
    v_dev, s_dev, u_dev = zen_amd.DeviceBuffer.from_host(V), zen_amd.DeviceBuffer(m * s_stride), zen_amd.DeviceBuffer(m * v_stride)
    idx_dev, cnt_dev = zen_amd.DeviceBuffer(m * k, np.int32), zen_amd.DeviceBuffer(m, np.int32)

    legs = {
        "W": lambda: rs.separate_device(inp, n, n, bg, fg, n),
        "WV": lambda: rv.separate_device(inp, n, n, bg, fg, n),
        "SM": lambda: repsim.similarity_device(v_dev, m, bins, v_stride, s_dev, s_stride, repsim.ROUTE_MFMA),
        "SV": lambda: repsim.similarity_device(v_dev, m, bins, v_stride, s_dev, s_stride, repsim.ROUTE_VALU),
        "SEL": lambda: repsim.select_device(s_dev, m, s_stride, 0.0, dd, k, idx_dev, cnt_dev),
        "GM": lambda: repsim.gather_median_device(v_dev, m, bins, v_stride, idx_dev, cnt_dev, m, k, u_dev, v_stride),
    }
    for _ in range(a.warmup):
        for run in legs.values():
            run()
    zen_amd.synchronize()
    t = {name: [] for name in legs}
    for _ in range(a.repeats):
        for name, run in legs.items():
            t[name].append(timed(run))
    res = {name: summary(v) for name, v in t.items()}
    for name in ("W", "WV"):
        res[name]["times_real_time"] = a.seconds / (res[name]["median_ms"] * 1e-3)
    flop = 2.0 * m * m * bins
    for name in ("SM", "SV"):
        tf = flop / (res[name]["median_ms"] * 1e-3) / 1e12
        res[name].update({"TFLOPs": tf, "frac_of_guide_gemm_122": tf / GUIDE_TFLOPS, "frac_of_peak_157": tf / PEAK_TFLOPS})
    counts = cnt_dev.download()
    copy_bw = bench.device_copy_bandwidth(zen_amd)
    gm_bytes = 4 * (int(counts.sum()) * (bins + 1) + m * (bins + 1))
    gbps = gm_bytes / (res["GM"]["median_ms"] * 1e-3) / 1e9
    res["GM"].update({"bytes": gm_bytes, "GBps": gbps, "frac_of_device_copy": gbps / copy_bw if copy_bw else None,
                      "note": "V is %d MB and cache-resident: gathered rows are cache reads" % (V.nbytes >> 20)})

    rs.profile(True)            # events around every launch slow the calls down: kept apart from the timings above
    for _ in range(a.profiled):
        legs["W"]()
    prof = rs.profile_get()
    rs.profile(False)
    kern = {name: {"ms_per_call": v["ms"] / a.profiled, "launches_per_call": v["launches"] // a.profiled} for name, v in prof.items()}
    kern["total_ms_per_call"] = sum(v["ms"] for v in prof.values()) / a.profiled

    # the host route, once
    host = {}
    t0 = time.perf_counter()
    Vh = v_dev.download().reshape(m, v_stride)
    host["v_to_host_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    nrm = np.sqrt(np.einsum("ij,ij->i", Vh, Vh))
    den = np.outer(nrm, nrm)
    S = np.where(den > 0, (Vh @ Vh.T) / np.where(den > 0, den, 1), 0).astype(np.float32)
    host["similarity_s"] = time.perf_counter() - t0
    hf = min(a.host_frames, m)
    t0 = time.perf_counter()
    hidx, hcnt = host_select(S[:hf], dd, k)
    host["select_s_for_host_frames"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    U = np.zeros((hf, v_stride), np.float32)
    for r in range(hf):
        if hcnt[r]:
            U[r] = np.median(Vh[hidx[r, :hcnt[r]]], axis=0)
    host["median_s_for_host_frames"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    u_dev.upload(np.zeros((m, v_stride), np.float32))
    zen_amd.synchronize()
    host["u_to_device_s"] = time.perf_counter() - t0
    host["host_frames"] = hf
    host["all_frames_s"] = (host["v_to_host_s"] + host["similarity_s"] + host["u_to_device_s"]
                            + (host["select_s_for_host_frames"] + host["median_s_for_host_frames"]) * m / hf)
    host["device_steps_3_to_5_ms"] = sum(kern[s]["ms_per_call"] for s in ("similarity_mfma", "select", "gather_median"))

    emit(__file__, {
        "repeats": a.repeats, "warmup": a.warmup,
        "workload": {"fs": a.fs, "nfft": a.nfft, "seconds": a.seconds, "samples": n, "frames": m, "bins": bins, "seed": a.seed, "signal": "bench.s_music",
                     "threshold": repsim.THRESHOLD, "distance_frames": dd, "number": k, "highpass_hz": repsim.HIGHPASS,
                     "mean_frames_per_median": float(counts.mean()), "similarity_flop": flop},
        "legs": res, "kernels_of_W": kern, "device_copy_GBps": copy_bw, "host_route": host,
        "device_bytes": rs.stats()["device_bytes"], "bands_per_call": rs.stats()["bands"] // (a.warmup + a.repeats + a.profiled),
    })


if __name__ == "__main__":
    main()
