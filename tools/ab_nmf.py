#!/usr/bin/env python3
"""The NMF add-on (zen_amd/nmf) on a clip that is resident on the device, in one process; one JSON line.

Workload: three minutes of mono audio at 44.1 kHz (the project's test signal, bench.s_music), frame 2048: 7753 frames of
1025 bins.
  FIT    one zen_hip_nmf_process_device call: a free fit, K = 64, --iterations (100) iterations, no stems, the matrix cores
  FITV   the same in a session created under ZEN_HIP_NMF="mfma=0": the products on the vector ALU
  SEP    a supervised separation: 32 + 32 held spectra, --iterations iterations, two stems, the matrix cores
  SEPV   the same on the vector ALU
  RM RV  zen_hip_nmf_ratio_device alone (H^T W, reduction K) on the two routes, K = 64
  HM HV  zen_hip_nmf_update_h_device alone (W Q^T, reduction over the bins)
  WM WV  zen_hip_nmf_update_w_device alone (H Q, reduction over the frames, K x F outputs)
The legs are interleaved (FIT FITV SEP SEPV RM RV ...), --repeats rounds after a warm-up, each between two HIP events; W and H
are put back to their initial values before every whole call, outside the events.
The products are quoted in TFLOP/s, counting 2 K F m, against 91.9 TFLOP/s (the similarity kernel of zen_amd/repsim), 122
TFLOP/s (the figure quoted for an untuned LDS-tiled f32 GEMM on the same instruction) and the 157.3 TFLOP/s peak.
From a second, profiled set of FIT and SEP rounds: the event times of every step; the mask kernel is quoted against the device
copy rate bench.py measures on the same box (tools/ubench_copy.hip) by the bytes it reads and writes.
The host route: the same iteration in numpy (float32 `@`, the BLAS numpy has) for --host-iterations iterations on V copied to
the host; the seconds for --iterations are those times iterations / host_iterations.
On the GPU box, under a time limit of its own:  timeout -k 10 600 python tools/ab_nmf.py > profiles/nmf_ab.json"""
import os
import time

import numpy as np

from _ab import arguments, bench, emit, summary, timed, zen_amd
from zen_amd import nmf

REPSIM_TFLOPS, GUIDE_TFLOPS, PEAK_TFLOPS = 91.9, 122.0, 157.3


def host_iterations(V, W, H, fixed, iterations):
    eps, K = np.float32(2.0 ** -40), W.shape[0]
    for _ in range(iterations):
        Q = V / np.maximum(H.T @ W, eps)
        H = H * (W @ Q.T) / np.maximum(W.sum(1), eps)[:, None]
        if fixed < K:
            Q = V / np.maximum(H.T @ W, eps)
            W[fixed:] = W[fixed:] * (H[fixed:] @ Q) / np.maximum(H[fixed:].sum(1), eps)[:, None]
    return W, H


def main():
    a = arguments(seconds=180.0, fs=44100.0, nfft=2048, components=64, iterations=100, repeats=5, warmup=1, profiled=2, host_iterations=5, seed=4242)
    zen_amd.init(0)
    n, H = int(a.seconds * a.fs), a.nfft // 2
    F, m, K = H + 1, nmf.n_frames(n, a.nfft), a.components
    x = bench.s_music(n, seed=a.seed).astype(np.float32)
    sm = nmf.Nmf(a.fs, a.nfft, K, 1, n)
    os.environ["ZEN_HIP_NMF"] = "mfma=0"
    sv = nmf.Nmf(a.fs, a.nfft, K, 1, n)
    del os.environ["ZEN_HIP_NMF"]
    inp = zen_amd.DeviceBuffer.from_host(x)
    fs4 = (F + 3) & ~3
    ms4 = (m + 3) & ~3
    W0 = np.zeros((K, fs4), np.float32)
    W0[:, :F] = nmf.init(0, K * F).reshape(K, F)
    H0 = np.zeros((K, ms4), np.float32)
    H0[:, :m] = nmf.init(1, K * m).reshape(K, m)
    w_dev, h_dev = zen_amd.DeviceBuffer.from_host(W0), zen_amd.DeviceBuffer.from_host(H0)
    stems = zen_amd.DeviceBuffer(2 * n)
    groups = [0] * (K // 2) + [1] * (K - K // 2)
    # the products alone work on a V of the clip made here (numpy's transform: close to the library's, not its bits)
    xp = np.zeros((m + 1) * H, np.float32)
    xp[H:H + n] = x
    win = nmf.table(a.nfft, nmf.TABLE_WINDOW)
    frames = np.lib.stride_tricks.as_strided(xp, (m, a.nfft), (4 * H, 4))
    V = np.zeros((m, fs4), np.float32)
    V[:, :F] = np.abs(np.fft.rfft(frames * win, axis=1)).astype(np.float32)
    v_dev, q_dev = zen_amd.DeviceBuffer.from_host(V), zen_amd.DeviceBuffer(m * fs4)
    w2, h2 = zen_amd.DeviceBuffer(K * fs4), zen_amd.DeviceBuffer(K * ms4)

    def whole(session, fixed, with_stems):
        def run():
            session.process_device(inp, n, n, w_dev, fs4, K * fs4, h_dev, ms4, K * ms4, fixed, a.iterations, groups if with_stems else None, 2,
                                   stems if with_stems else None, n)
        return run

    def alone(f, route):
        if f == "R":
            return lambda: nmf.ratio_device(v_dev, fs4, w_dev, fs4, h_dev, ms4, K, F, m, q_dev, fs4, None, 0, route)
        if f == "H":
            return lambda: nmf.update_h_device(w_dev, fs4, q_dev, fs4, h_dev, ms4, K, F, m, h2, ms4, route)
        return lambda: nmf.update_w_device(h_dev, ms4, q_dev, fs4, w_dev, fs4, K, F, m, 0, w2, fs4, route)

    legs = {"FIT": whole(sm, 0, False), "FITV": whole(sv, 0, False), "SEP": whole(sm, K, True), "SEPV": whole(sv, K, True)}
    for f in "RHW":
        legs[f + "M"] = alone(f, nmf.ROUTE_MFMA)
        legs[f + "V"] = alone(f, nmf.ROUTE_VALU)

    def reset():
        w_dev.upload(W0)
        h_dev.upload(H0)
        zen_amd.synchronize()

    reset()
    legs["RM"]()        # Q for the updates alone
    for _ in range(a.warmup):
        for run in legs.values():
            reset()
            run()
    zen_amd.synchronize()
    t = {name: [] for name in legs}
    for _ in range(a.repeats):
        for name, run in legs.items():
            reset()
            t[name].append(timed(run))
    res = {name: summary(v) for name, v in t.items()}
    for name in ("FIT", "FITV", "SEP", "SEPV"):
        res[name]["times_real_time"] = a.seconds / (res[name]["median_ms"] * 1e-3)
        res[name]["ms_per_iteration"] = res[name]["median_ms"] / max(a.iterations, 1)
    flop = 2.0 * K * F * m
    for name in ("RM", "RV", "HM", "HV", "WM", "WV"):
        tf = flop / (res[name]["median_ms"] * 1e-3) / 1e12
        res[name].update({"TFLOPs": tf, "frac_of_repsim_91.9": tf / REPSIM_TFLOPS, "frac_of_guide_gemm_122": tf / GUIDE_TFLOPS,
                          "frac_of_peak_157": tf / PEAK_TFLOPS})
    res["RM"]["note"] = "reduction of %d links, two chunks of 32: the epilogue's division and %d MB of V in and Q out dominate" % (K, (2 * V.nbytes) >> 20)
    res["WM"]["note"] = "%d x %d outputs are %d workgroups of 128 x 128 on 256 compute units, each walking %d segments in sequence" % (
        K, F, -(-K // 128) * -(-F // 128), -(-m // 256))
    copy_bw = bench.device_copy_bandwidth(zen_amd)

    kern = {}
    for label, session, fixed, with_stems in (("FIT", sm, 0, False), ("SEP", sm, K, True)):
        session.profile(True)       # events around every launch slow the calls down: kept apart from the timings above
        for _ in range(a.profiled):
            reset()
            whole(session, fixed, with_stems)()
        prof = session.profile_get()
        session.profile(False)
        k = {name: {"ms_per_call": v["ms"] / a.profiled, "launches_per_call": v["launches"] // a.profiled,
                    "GBps": (v["bytes"] / v["ms"] / 1e6) if v["ms"] > 0 else None} for name, v in prof.items()}
        for name in ("ratio_mfma", "update_h_mfma", "update_w_mfma"):
            if prof[name]["launches"]:
                k[name]["TFLOPs"] = flop * prof[name]["launches"] / (prof[name]["ms"] * 1e-3) / 1e12
        for name in ("mask", "overlap_add", "magnitude", "frame"):
            if k[name]["GBps"] and copy_bw:
                k[name]["frac_of_device_copy"] = k[name]["GBps"] / copy_bw
        k["total_ms_per_call"] = sum(v["ms"] for v in prof.values()) / a.profiled
        kern[label] = k

    # the host route
    host = {}
    t0 = time.perf_counter()
    Vh = v_dev.download().reshape(m, fs4)[:, :F].copy()
    host["v_to_host_s"] = time.perf_counter() - t0
    for label, fixed in (("free", 0), ("held", K)):
        t0 = time.perf_counter()
        host_iterations(Vh, W0[:, :F].copy(), H0[:, :m].copy(), fixed, a.host_iterations)
        dt = time.perf_counter() - t0
        host[label + "_s_for_host_iterations"] = dt
        host[label + "_s_for_all_iterations"] = dt * a.iterations / max(a.host_iterations, 1)
    host["host_iterations"] = a.host_iterations
    host["threads"] = os.cpu_count() if "OMP_NUM_THREADS" not in os.environ else int(os.environ["OMP_NUM_THREADS"])

    emit(__file__, {
        "repeats": a.repeats, "warmup": a.warmup,
        "workload": {"fs": a.fs, "nfft": a.nfft, "seconds": a.seconds, "samples": n, "frames": m, "bins": F, "components": K, "iterations": a.iterations,
                     "seed": a.seed, "signal": "bench.s_music", "product_flop": flop},
        "legs": res, "kernels": kern, "device_copy_GBps": copy_bw, "host_route": host, "device_bytes": sm.stats()["device_bytes"],
    })


if __name__ == "__main__":
    main()
