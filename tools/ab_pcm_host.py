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
On the GPU box, under a time limit of its own:  timeout -k 10 900 python tools/ab_pcm_host.py > pcm16_host_ab.json

--fmt i16,i24 (default i16: the record above).  For i24 the same shapes are timed over three routes, interleaved in one process
on engines of one configuration (A B C A B C ...), PEAK mode, same audio at both depths:
  i24:   the packed 24-bit call (zen_hip_pcm_*_fmt with ZEN_HIP_PCM_I24 both ways), 3 bytes per sample each way;
  i16:   the int16 call, 2 bytes per sample each way (both also in GAIN mode, where pieces come down under the kernels
         of later ones as the float call's do: the like-for-like comparison of the link traffic);
  float: today's route for a 24-bit file -- wav.h:80-86's unpack-and-widen loop on the host, the float call, then on one host
         thread the peak search, the scaling, the rounding and the packing of every output (compiled -O2).
and the two 24-bit kernels are timed alone on one resident piece (HIP events, best of 5) beside the link's own copy of that
piece's bytes from / to pinned memory and a device-to-device copy of them, all in the same run: "kernels_hidden" says whether
each kernel's time is below the link's copy time for the piece.  Nothing is asserted: the record states what was measured.
  timeout -k 10 900 python tools/ab_pcm_host.py --fmt i24 > pcm24_host_ab.json"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

from _ab import bench, emit, summary, timed, zen_amd
from zen_amd import pcm

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
extern "C" void host_widen24(const uint8_t* data, size_t n, float* x)              // wav.h:80-86
{
	for (std::size_t i = 0; i < n; ++i) {
		int32_t v = data[3 * i] | (data[3 * i + 1] << 8) | (data[3 * i + 2] << 16);
		if (v & 0x800000)
			v |= ~0xFFFFFF;
		x[i] = (float)v / 8388608.f;
	}
}
extern "C" void host_post24(float* x, size_t n, uint8_t* pcm)                      // peak, scale, round, saturate, pack
{
	auto limits = std::minmax_element(x, x + n);
	const float real_max = std::max(-1 * (*limits.first), *limits.second);
	for (std::size_t j = 0; j < n; ++j)
		x[j] /= real_max;
	for (std::size_t i = 0; i < n; ++i) {
		long v = lroundf(x[i] * 8388608.f);
		v = v > 8388607 ? 8388607 : v < -8388608 ? -8388608 : v;
		pcm[3 * i] = (uint8_t)(v & 255);
		pcm[3 * i + 1] = (uint8_t)((v >> 8) & 255);
		pcm[3 * i + 2] = (uint8_t)((v >> 16) & 255);
	}
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
            best = min(best, timed(call))
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


def kernels24_alone(piece):
    """the two 24-bit kernels on one resident piece of `piece` samples, beside the copies of its 3 * piece bytes: over the link
    from / to pinned memory, and device to device (HIP events, best of 5, all in this run)"""
    L = zen_amd.lib.load()
    packed, f, back = zen_amd.DeviceBuffer(3 * piece, np.uint8), zen_amd.DeviceBuffer(piece), zen_amd.DeviceBuffer(3 * piece, np.uint8)
    pin = pcm.PinnedPCM(piece, pcm.I24)
    pin.array[:] = np.random.default_rng(1).integers(0, 256, 3 * piece).astype(np.uint8)
    packed.upload(pin.array)
    calls = (("unpack", lambda: pcm.to_float(packed.ptr, 1, piece, f.ptr, fmt=pcm.I24)),
             ("pack", lambda: pcm.from_float(f.ptr, piece, back.ptr, mode=pcm.GAIN, gain=8388608.0, fmt=pcm.I24)),
             ("link_up", lambda: zen_amd.lib._ck(L.zen_hip_memcpy_h2d_async(packed.ptr, pin.array.ctypes.data, 3 * piece, None))),
             ("link_down", lambda: zen_amd.lib._ck(L.zen_hip_memcpy_d2h_async(pin.array.ctypes.data, back.ptr, 3 * piece, None))),
             ("device_copy", lambda: zen_amd.lib._ck(L.zen_hip_memcpy_d2d(back.ptr, packed.ptr, 3 * piece, None))))
    out = {}
    for name, call in calls:
        best = 1e30
        for _ in range(6):
            a, b = zen_amd.Event(), zen_amd.Event()
            a.record()
            call()
            b.record()
            zen_amd.synchronize()
            best = min(best, a.elapsed_ms(b))
        out[name + "_ms"] = best
    pcm.to_float(packed.ptr, 1, piece, f.ptr, fmt=pcm.I24)
    pcm.from_float(f.ptr, piece, back.ptr, mode=pcm.GAIN, gain=8388608.0, fmt=pcm.I24)
    zen_amd.synchronize()
    identity = bool(np.array_equal(back.download(), packed.download()))
    for b in (packed, f, back):
        b.free()
    pin.free()
    out.update({"piece_samples": piece, "unpack_then_pack_is_identity": identity,
                "GBps": {"unpack": 7e-6 * piece / out["unpack_ms"], "pack": 7e-6 * piece / out["pack_ms"],
                         "link_up": 3e-6 * piece / out["link_up_ms"], "link_down": 3e-6 * piece / out["link_down_ms"],
                         "device_copy": 6e-6 * piece / out["device_copy_ms"]},
                "kernels_hidden": bool(out["unpack_ms"] < out["link_up_ms"] and out["pack_ms"] < out["link_down_ms"])})
    return out


def run_shape_i24(name, x, make_engine, outputs, loops, pairs, warmup, offline, pinned):
    """the three routes of a 24-bit caller, PEAK mode; the int16 route on the same audio at 16 bits"""
    n = x.size
    v24 = np.clip(np.round(x * 8388607.0), -8388608, 8388607).astype(np.int32)
    keep = []

    def buf(m, fmt):
        if fmt is None:
            p = zen_amd.PinnedHost(m) if pinned else None
            a = p.array if pinned else np.zeros(m, np.float32)
        else:
            p = pcm.PinnedPCM(m, fmt) if pinned else None
            a = p.array if pinned else np.zeros(m * (3 if fmt == pcm.I24 else 1), np.uint8 if fmt == pcm.I24 else np.int16)
        if p is not None:
            keep.append(p)
        return a
    x24, x16, xf = buf(n, pcm.I24), buf(n, pcm.I16), buf(n, None)
    x24[:] = pcm.pack24(v24)
    x16[:] = (v24 >> 8).astype(np.int16)
    o24 = {k: buf(n, pcm.I24) for k in outputs}
    o16 = {k: buf(n, pcm.I16) for k in outputs}
    fo = {k: buf(n, None) for k in outputs}
    enc = {k: np.zeros(3 * n, np.uint8) for k in outputs if not (offline and k == "resid")}     # the encoder's own (pageable) bytes
    eng = {r: make_engine() for r in ("i24", "i16", "float")}
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    if offline:
        def call_pcm(e, xin, o, mode=pcm.PEAK, gain=1.0):
            return pcm.hpri_process(e, xin, harm=o.get("harm"), perc=o.get("perc"), resid=o.get("resid"), mode=mode, gain=gain)

        def call_float():
            eng["float"].process(xf, out=(fo.get("harm"), fo.get("perc"), fo.get("resid")))
    else:
        def call_pcm(e, xin, o, mode=pcm.PEAK, gain=1.0):
            return pcm.hpr_process_host(e, xin, mode=mode, gain=gain, **o)

        def call_float():
            eng["float"].process_host(xf, **fo)

    def route_float():
        t = {"widen": ms(lambda: loops.host_widen24(p(x24), C.c_size_t(n), p(xf))), "call": ms(call_float), "post": 0.0}
        for k in enc:
            t["post"] += ms(lambda: loops.host_post24(p(fo[k]), C.c_size_t(n), p(enc[k])))
        return t
    for _ in range(warmup):
        call_pcm(eng["i24"], x24, o24, pcm.GAIN)
        call_pcm(eng["i16"], x16, o16, pcm.GAIN)
        peaks = call_pcm(eng["i24"], x24, o24)
        call_pcm(eng["i16"], x16, o16)
        route_float()
    top = max(float(np.max(peaks)), 1e-30)
    t = {"i24": [], "i16": [], "i24_gain": [], "i16_gain": [], "float_widen": [], "float_call": [], "float_post": []}
    stats = None
    for _ in range(pairs):
        t["i24_gain"].append(ms(lambda: call_pcm(eng["i24"], x24, o24, pcm.GAIN, 8388608.0 / top)))
        stats_gain = pcm.host_stats()
        t["i16_gain"].append(ms(lambda: call_pcm(eng["i16"], x16, o16, pcm.GAIN, 32767.0 / top)))
        t["i24"].append(ms(lambda: call_pcm(eng["i24"], x24, o24)))
        stats = pcm.host_stats()
        t["i16"].append(ms(lambda: call_pcm(eng["i16"], x16, o16)))
        r = route_float()
        for k in ("widen", "call", "post"):
            t["float_" + k].append(r[k])
    same = all(bool(np.array_equal(enc[k], o24[k])) for k in enc)
    n_down = len(enc)
    s24, s16, sfc = summary(t["i24"]), summary(t["i16"]), summary(t["float_call"])
    g24, g16 = summary(t["i24_gain"]), summary(t["i16_gain"])
    whole = summary([a + b + c for a, b, c in zip(t["float_widen"], t["float_call"], t["float_post"])])
    res = {"shape": name, "fmt": "i24", "mode": "peak", "buffers": "pinned" if pinned else "pageable", "samples": n, "outputs": list(outputs),
           "pieces": stats["n_pieces"], "piece_frames": stats["piece_frames"], "peak_tail_ms": stats["tail_ms"],
           "pieces_gain": stats_gain["n_pieces"], "piece_frames_gain": stats_gain["piece_frames"],
           "i24_call": s24, "i16_call": s16, "i24_gain_call": g24, "i16_gain_call": g16, "float_call_alone": sfc, "host_widen24": summary(t["float_widen"]),
           "host_peak_scale_round_pack": summary(t["float_post"]), "float_route": whole,
           "ratio_i24_over_i16": s24["median_ms"] / s16["median_ms"], "ratio_float_call_over_i24": sfc["median_ms"] / s24["median_ms"],
           "ratio_float_route_over_i24": whole["median_ms"] / s24["median_ms"],
           "expect_i24_below_float_call_alone": bool(s24["median_ms"] < sfc["median_ms"]),
           "gain_ratio_i24_over_i16": g24["median_ms"] / g16["median_ms"], "gain_ratio_float_call_over_i24": sfc["median_ms"] / g24["median_ms"],
           "gain_expect_i24_below_float_call_alone": bool(g24["median_ms"] < sfc["median_ms"]),
           "i24_equals_host_route_bytes": same,
           "link_GBps": {"i24_up": 3e-6 * n / s24["median_ms"], "i24_down": 3e-6 * n * n_down / s24["median_ms"],
                         "i16_up": 2e-6 * n / s16["median_ms"], "i16_down": 2e-6 * n * n_down / s16["median_ms"],
                         "float_up": 4e-6 * n / sfc["median_ms"], "float_down": 4e-6 * n * n_down / sfc["median_ms"],
                         "of_GBps_each_way": LINK_GBPS},
           "kernels_alone_on_a_piece": kernels24_alone(int(stats["piece_frames"]))}
    for e in ("i24", "i16"):
        pcm.release(eng[e])
    eng.clear()
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
    ap.add_argument("--fmt", default="i16", help="i16, i24 or both: which caller's routes are timed")
    a = ap.parse_args()
    assert a.pairs >= 5
    zen_amd.init(0)
    pcm.load()
    loops = host_loops()
    ALL = zen_amd.OUTPUT_HARMONIC | zen_amd.OUTPUT_PERCUSSIVE | zen_amd.OUTPUT_RESIDUAL
    results, results24 = [], []
    fmts = a.fmt.split(",")
    assert fmts and all(f in ("i16", "i24") for f in fmts)
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
            if "i24" in fmts:
                r = run_shape_i24(shape, x, mk, outs, loops, a.pairs, a.warmup, off, buf == "pinned")
                results24.append(r)
                print("# i24 %s %s: i24 %.2f ms, i16 %.2f ms, float call %.2f ms, float route %.2f ms" % (
                    shape, buf, r["i24_call"]["median_ms"], r["i16_call"]["median_ms"], r["float_call_alone"]["median_ms"],
                    r["float_route"]["median_ms"]), file=sys.stderr, flush=True)
            if "i16" not in fmts:
                continue
            results.append(run_shape(shape, x, mk, outs, loops, a.pairs, a.warmup, off, buf == "pinned"))
            print("# %s %s: float %.2f ms, pcm gain %.2f ms, float+host %.2f ms, pcm peak %.2f ms" % (
                shape, buf, results[-1]["float"]["median_ms"], results[-1]["pcm_gain"]["median_ms"],
                results[-1]["float_plus_host"]["median_ms"], results[-1]["pcm_peak"]["median_ms"]), file=sys.stderr, flush=True)
    pinned = [r for r in results if r["buffers"] == "pinned"]
    record = {"pairs": a.pairs, "warmup": a.warmup}
    if "i16" in fmts:
        record.update({"requirement_met_pinned": bool(pinned and all(r["requirement_gain"] and r["requirement_peak"] for r in pinned)),
                       "results": results})
    if "i24" in fmts:
        record["results_i24"] = results24
    emit(__file__, record)


if __name__ == "__main__":
    main()
