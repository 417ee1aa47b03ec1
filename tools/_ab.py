"""The frame the A/B tools of the add-on libraries (tools/ab_<library>.py) share: the path bootstrap (the repository and tests/
importable: bench, zen_amd and the CPU models), the command line, the clocks, the summaries every record carries and the JSON
line.  A tool keeps its workload, its options' defaults and its figures."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]
import bench      # noqa: E402,F401  (s_music: the project's test signal; the copy rates the kernels are held against)
import zen_amd    # noqa: E402


def arguments(**defaults):
    """the parsed command line: --some-option for every some_option=default, of the default's type"""
    ap = argparse.ArgumentParser()
    for name, default in defaults.items():
        ap.add_argument("--" + name.replace("_", "-"), type=type(default), default=default)
    return ap.parse_args()


def summary(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "spread_ms": float(max(ts) - min(ts)),
            "runs": len(ts)}


def timed(f):
    """ms on the device between two events around f()"""
    a, b = zen_amd.Event(), zen_amd.Event()
    a.record()
    f()
    b.record()
    return a.elapsed_ms(b)


def kernels(prof, rounds):
    """a handle's profile_get() over `rounds` rounds: per kernel ms, bytes and launches per round and the achieved GB/s"""
    out = {kn: {"ms_per_round": v["ms"] / rounds, "bytes_per_round": v["bytes"] // rounds, "launches_per_round": v["launches"] // rounds,
                "GBps": (v["bytes"] / (v["ms"] * 1e-3) / 1e9) if v["ms"] > 0 else None} for kn, v in prof.items()}
    out["total_ms_per_round"] = sum(v["ms"] for v in prof.values()) / rounds
    return out


def class_ms(prof, calls):
    """profile_get_engine() / HPRIOffline.profile_get_all() over `calls` calls: ms per call of every kernel class that ran"""
    out = {ps: {k: v["ms"] / calls for k, v in d.items() if v["launches"]} for ps, d in prof.items()}
    out["total_ms_per_round"] = sum(v for ps in ("pass1", "pass2") for v in out[ps].values())
    return out


def per_call(ts, hop_ms, count="calls", within=True):
    """single calls held against the duration of the hop each covers: median, 99th percentile, maximum, and with `within`
    whether the slowest stayed inside the hop"""
    ts = np.asarray(ts)
    out = {count: int(ts.size), "median_ms": float(np.median(ts)), "p99_ms": float(np.percentile(ts, 99)), "max_ms": float(ts.max()),
           "hop_ms": hop_ms, "max_over_hop": float(ts.max() / hop_ms)}
    return dict(out, within_the_hop_at_the_maximum=bool(ts.max() < hop_ms)) if within else out


def emit(tool, record):
    """the tool's one JSON line: which tool (its __file__) measured on which device, then the tool's own keys"""
    print(json.dumps(dict({"tool": "tools/" + os.path.basename(tool), "device": zen_amd.device_name()}, **record)))
