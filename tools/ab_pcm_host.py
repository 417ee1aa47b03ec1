#!/usr/bin/env python3
"""Float host call against PCM16 host call (zen_amd/pcm) on the same engine configuration and the same audio, interleaved in
one process (A B A B ..., --pairs rounds after a warm-up), from pinned and from pageable buffers; one JSON line.

Shapes: the headline block (hop 1024, 25 840 hops; percussive only, and all three outputs) through zen_hip_hpr_process_host /
zen_hip_pcm_hpr_process_host, and --seconds (default one hour) of mono audio through zen_hip_hpri_process /
zen_hip_pcm_hpri_process at 4096 / 2.5 / 256 / 2.5.  Two comparisons per shape:
  gain: PCM16 GAIN call against the float call alone (the link traffic, like for like);
  peak: PCM16 PEAK call against the float call PLUS what its caller does next today on one host thread, compiled -O2 as the
        command line tool is: peak_normalise (cli/main.cpp:86-92) and the encoder's loop (cli/wav.h:130-132) over every output,
        and for the offline shape wav.h:77-78's widening loop in front.
"requirement": the PCM16 median is below the float median by more than the float call's own spread (max - min).
On the GPU box, under a time limit of its own:  timeout -k 10 900 python tools/ab_pcm_host.py > pcm16_host_ab.json"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench      # noqa: E402  (s_music: the project's test signal)
import zen_amd    # noqa: E402
from zen_amd import pcm  # noqa: E402

FS, LINK_GBPS = 44100.0, 57.0      # the host link as tools/probe_pcie.cpp measured it, each way

HOST_LOOPS = r"""
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
extern "C" void host_post(float* x, size_t n, int16_t* pcm)
{
	auto limits = std::minmax_element(x, x + n);                                   // peak_normalise
	const float real_max = std::max(-1 * (*limits.first), *limits.second);
	for (std::size_t j = 0; j < n; ++j)
		x[j] /= real_max;
	for (std::size_t i = 0; i < n; ++i)                                            // encode_pcm16_mono's loop
		pcm[i] = (int16_t)lroundf(x[i] * 32767.f);
}
extern "C" void host_widen(const int16_t* s, size_t n, float* x)
{
	for (std::size_t i = 0; i < n; ++i)
		x[i] = (float)s[i] / 32767.f;
}
"""


def host_loops():
    d = tempfile.mkdtemp(prefix="ab_pcm_")
    src, so = os.path.join(d, "loops.cpp"), os.path.join(d, "loops.so")
    with open(src, "w") as f:
        f.write(HOST_LOOPS)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", so])
    return C.CDLL(so)


def ms(f):
    t0 = time.perf_counter()
    f()
    return 1e3 * (time.perf_counter() - t0)


def summary(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "spread_ms": float(max(ts) - min(ts)),
            "runs": len(ts)}


def kernels_alone_ms(n, n_out):
    """the three new kernels on device-resident data of this shape's size (HIP events, best of 3): their share of a call"""
    x16 = zen_amd.DeviceBuffer(n, np.int16)
    f = zen_amd.DeviceBuffer(n)
    mm = zen_amd.DeviceBuffer.from_host(np.array([np.inf, -np.inf], np.float32))
    x16.zero()
    out = {}
    for name, call in (("to_float", lambda: pcm.to_float(x16.ptr, 1, n, f.ptr)), ("peak", lambda: pcm.peak(f.ptr, n, mm.ptr)),
                       ("from_float", lambda: pcm.from_float(f.ptr, n, x16.ptr, mode=pcm.GAIN, gain=1.0))):
        best = 1e30
        for _ in range(4):
            a, b = zen_amd.Event(), zen_amd.Event()
            a.record()
            call()
            b.record()
            best = min(best, a.elapsed_ms(b))
        out[name] = best
    for b in (x16, f, mm):
        b.free()
    return {"to_float_ms": out["to_float"], "peak_ms_per_output": out["peak"], "from_float_ms_per_output": out["from_float"],
            "gain_call_ms": out["to_float"] + n_out * out["from_float"],
            "peak_call_ms": out["to_float"] + n_out * (out["peak"] + out["from_float"]),
            "GBps": {"to_float": 6e-6 * n / out["to_float"], "peak": 4e-6 * n / out["peak"], "from_float": 6e-6 * n / out["from_float"]}}


def run_shape(name, x, make_engine, outputs, loops, pairs, warmup, offline, pinned):
    """outputs: names of the host outputs the calls fill ('harm', 'perc', 'resid')"""
    n = x.size
    x16h = np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)
    keep = []
    if pinned:
        def f32(m):
            p = zen_amd.PinnedHost(m)
            keep.append(p)
            return p.array

        def i16(m):
            p = pcm.PinnedPCM(m)
            keep.append(p)
            return p.array
    else:
        def f32(m):
            return np.zeros(m, np.float32)

        def i16(m):
            return np.zeros(m, np.int16)
    xf, x16 = f32(n), i16(n)
    x16[:] = x16h
    loops.host_widen(x16.ctypes.data_as(C.c_void_p), C.c_size_t(n), xf.ctypes.data_as(C.c_void_p))
    fo = {k: f32(n) for k in outputs}
    po = {k: i16(n) for k in outputs}
    enc = {k: np.zeros(n, np.int16) for k in outputs if not (offline and k == "resid")}     # the encoder's own (pageable) vectors
    eng_f, eng_p = make_engine(), make_engine()
    if offline:
        def call_float():
            eng_f.process(xf, out=(fo.get("harm"), fo.get("perc"), fo.get("resid")))

        def call_pcm(mode, gain):
            return pcm.hpri_process(eng_p, x16, harm=po.get("harm"), perc=po.get("perc"), resid=po.get("resid"), mode=mode, gain=gain)
    else:
        def call_float():
            eng_f.process_host(xf, **fo)

        def call_pcm(mode, gain):
            return pcm.hpr_process_host(eng_p, x16, mode=mode, gain=gain, **po)

    def host_after():
        t = 0.0
        if offline:
            t += ms(lambda: loops.host_widen(x16.ctypes.data_as(C.c_void_p), C.c_size_t(n), xf.ctypes.data_as(C.c_void_p)))
        for k in enc:
            t += ms(lambda: loops.host_post(fo[k].ctypes.data_as(C.c_void_p), C.c_size_t(n), enc[k].ctypes.data_as(C.c_void_p)))
        return t

    for _ in range(warmup):
        call_float()
        call_pcm(pcm.GAIN, 1.0)
        peaks = call_pcm(pcm.PEAK, 1.0)
    gain = float(np.float32(32767.0) / max(float(np.max(peaks)), 1e-30))
    t = {"float": [], "host_after": [], "pcm_gain": [], "pcm_peak": []}
    tails, stats = [], None
    for _ in range(pairs):
        t["float"].append(ms(call_float))
        t["host_after"].append(host_after())
        t["pcm_gain"].append(ms(lambda: call_pcm(pcm.GAIN, gain)))
        t["pcm_peak"].append(ms(lambda: call_pcm(pcm.PEAK, 1.0)))
        stats = pcm.host_stats()
        tails.append(stats["tail_ms"])
    # same samples on both sides (PEAK against the host's own normalise + encode of the float call's outputs)
    same = all(bool(np.array_equal(enc[k], po[k])) for k in enc)
    n_down = len(enc)
    fl, g, p = summary(t["float"]), summary(t["pcm_gain"]), summary(t["pcm_peak"])
    fplus = summary([a + b for a, b in zip(t["float"], t["host_after"])])
    kern = kernels_alone_ms(n, n_down)
    res = {"shape": name, "buffers": "pinned" if pinned else "pageable", "samples": n, "outputs": list(outputs), "pieces": stats["n_pieces"],
           "piece_frames": stats["piece_frames"], "float": fl, "host_after": summary(t["host_after"]), "float_plus_host": fplus,
           "pcm_gain": g, "pcm_peak": p, "peak_tail_ms_median": float(np.median(tails)),
           "peak_tail_share": float(np.median(tails)) / p["median_ms"],
           "ratio_gain": fl["median_ms"] / g["median_ms"], "ratio_peak": fplus["median_ms"] / p["median_ms"],
           "requirement_gain": bool(g["median_ms"] < fl["median_ms"] - fl["spread_ms"]),
           "requirement_peak": bool(p["median_ms"] < fplus["median_ms"] - fplus["spread_ms"]),
           "peak_equals_host_normalise_and_encode": same,
           "link_GBps": {"float_up": 4e-6 * n / fl["median_ms"], "float_down": 4e-6 * n * n_down / fl["median_ms"],
                         "pcm_gain_up": 2e-6 * n / g["median_ms"], "pcm_gain_down": 2e-6 * n * n_down / g["median_ms"],
                         "of_GBps_each_way": LINK_GBPS},
           "new_kernels_alone": kern, "new_kernels_share_gain": kern["gain_call_ms"] / g["median_ms"],
           "new_kernels_share_peak": kern["peak_call_ms"] / p["median_ms"]}
    pcm.release(eng_p)
    eng_f = eng_p = None
    for k in keep:
        k.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--hops", type=int, default=25840)
    ap.add_argument("--shapes", default="block_perc,block_all,offline")
    ap.add_argument("--buffers", default="pinned,pageable")
    a = ap.parse_args()
    assert a.pairs >= 5
    zen_amd.init(0)
    pcm.load()
    loops = host_loops()
    ALL = zen_amd.OUTPUT_HARMONIC | zen_amd.OUTPUT_PERCUSSIVE | zen_amd.OUTPUT_RESIDUAL
    results = []
    for shape in a.shapes.split(","):
        if shape == "offline":
            n = int(a.seconds * FS)
            base = bench.s_music(int(60 * FS), seed=4242)
            x = np.tile(base, -(-n // base.size))[:n].copy()
            mk, outs, off = (lambda: zen_amd.HPRIOffline(FS, 4096, 256, 2.5, 2.5)), ("harm", "perc", "resid"), True
        else:
            x = bench.s_music(a.hops * 1024, seed=0)
            flags = zen_amd.OUTPUT_PERCUSSIVE if shape == "block_perc" else ALL
            mk = (lambda flags=flags: zen_amd.HPR(FS, 1024, 2.0, flags, zen_amd.TIME_CAUSAL, True, 1, 0))
            outs, off = (("perc",) if shape == "block_perc" else ("harm", "perc", "resid")), False
        for buf in a.buffers.split(","):
            results.append(run_shape(shape, x, mk, outs, loops, a.pairs, a.warmup, off, buf == "pinned"))
            print("# %s %s: float %.2f ms, pcm gain %.2f ms, float+host %.2f ms, pcm peak %.2f ms" % (
                shape, buf, results[-1]["float"]["median_ms"], results[-1]["pcm_gain"]["median_ms"],
                results[-1]["float_plus_host"]["median_ms"], results[-1]["pcm_peak"]["median_ms"]), file=sys.stderr, flush=True)
    pinned = [r for r in results if r["buffers"] == "pinned"]
    print(json.dumps({"tool": "tools/ab_pcm_host.py", "device": zen_amd.device_name(), "pairs": a.pairs, "warmup": a.warmup,
                      "requirement_met_pinned": bool(pinned and all(r["requirement_gain"] and r["requirement_peak"] for r in pinned)),
                      "results": results}))


if __name__ == "__main__":
    main()
