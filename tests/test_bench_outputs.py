"""bench.py's plain run and `--dump-outputs DIR`: the plain line carries the headline alone (everything else is `--full`'s), and
the arrays the timed path computed in its last step land in DIR/<name>.npy, float32, within the size budget, the same on every
run of the same arguments -- and the same samples the oracle computes."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FS = 44100.0


def bench():
    spec = importlib.util.spec_from_file_location("bench", BENCH)
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def run(args, timeout=600, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, BENCH] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_dump_outputs_writes_small_outputs_whole_and_samples_large_ones_within_the_budget(tmp_path):
    b = bench()
    rng = np.random.default_rng(5)
    small, big = rng.standard_normal(1000).astype(np.float32), rng.standard_normal(300000).astype(np.float32)
    budget = 400000
    b.dump_outputs(str(tmp_path / "a"), {"small": small, "big": big}, budget=budget)
    b.dump_outputs(str(tmp_path / "b"), {"small": small, "big": big.copy()}, budget=budget)
    got = {k: np.load(str(tmp_path / "a" / (k + ".npy"))) for k in ("small", "big")}
    assert sorted(os.listdir(str(tmp_path / "a"))) == ["big.npy", "small.npy"]
    assert all(v.dtype == np.float32 and v.ndim == 1 for v in got.values())
    assert np.array_equal(got["small"], small)                            # under its share: whole
    share = budget // 4 // 2
    idx = np.unique(np.random.default_rng(0).integers(0, big.size, share))
    assert 0.8 * share < got["big"].size <= share and np.array_equal(got["big"], big[idx])
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))) <= budget + 2 * 256
    again = np.load(str(tmp_path / "b" / "big.npy"))                      # the same positions on every run
    assert np.array_equal(again, got["big"])
    assert b.DUMP_BYTES <= 64 * 10 ** 6


def test_plain_dry_line_has_no_legs_and_full_adds_them():
    plain = run(["--gpus", "2", "--dry", "--backend", "gloo", "--hops", "100", "--steps", "1"], timeout=240)
    assert plain["n_gpus"] == 2 and plain["ranks_reported"] == 2 and plain["config"]["units_all_ranks"] == 200
    assert "offline_batch_sharded" not in plain and "offline_host_sharded" not in plain
    full = run(["--gpus", "2", "--dry", "--backend", "gloo", "--hops", "100", "--steps", "1", "--full"], timeout=240)
    assert full["offline_batch_sharded"]["ranks_reported"] == 2


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_of_the_headline_block_bit_exact_vs_oracle(tmp_path):
    """The headline block (hop 1024, P only, causal, hard mask), 256 hops per step: the plain line holds the headline and no leg,
    and percussive.npy is the last step's output.  Every step feeds the same block again with the state the previous one left,
    and a causal output hop depends on input hops i-2 .. i only: from the second step on, a step's output is the oracle's on the
    block with the block's own last two hops in front -- whatever the number of steps."""
    from oracle import oracle as o
    hop, M = 1024, 256
    common = ["--hops", str(M), "--warmup", "1", "--settle-ms", "0"]
    a = run(common + ["--steps", "3", "--dump-outputs", str(tmp_path / "a")])
    assert a["steps"] == 3 and a["warmup"] == 1 and a["ms_per_step"] > 0 and a["value"] > 0
    assert a["unit"] == "hops/s" and a["higher_is_better"] is True and a["dtype"] == "f32"
    for k in ("legs", "cpu_baseline", "gpu_over_cpu", "detail"):
        assert k not in a, k
    assert "per_hop_api_us" not in a["config"] and "all_outputs_hops_per_s" not in a["config"]
    assert os.listdir(str(tmp_path / "a")) == ["percussive.npy"]
    got = np.load(str(tmp_path / "a" / "percussive.npy"))
    assert got.dtype == np.float32 and got.size == M * hop
    run(common + ["--steps", "1", "--dump-outputs", str(tmp_path / "b")])
    assert np.array_equal(np.load(str(tmp_path / "b" / "percussive.npy")), got)
    x = bench().s_music(M * hop, seed=0)
    ref = o.HPR(FS, hop, 2.0, o.OUTPUT_PERCUSSIVE, o.TIME_CAUSAL).process_stream(np.concatenate([x[-2 * hop:], x]))["P"]
    assert np.array_equal(got, ref[2 * hop:])


@pytest.mark.gpu
def test_offline_batch_dump_is_every_clip_bit_exact_vs_oracle(tmp_path):
    from oracle import oracle as o
    C, secs = 2, 2.0
    j = run(["--workload", "offline_batch", "--clips", str(C), "--clip-seconds", str(secs), "--steps", "2", "--warmup", "1",
             "--settle-ms", "0", "--dump-outputs", str(tmp_path)])
    assert j["steps"] == 2 and j["ms_per_step"] > 0 and "cpu_baseline" not in j
    assert sorted(os.listdir(str(tmp_path))) == ["harmonic.npy", "percussive.npy"]
    h, p = np.load(str(tmp_path / "harmonic.npy")), np.load(str(tmp_path / "percussive.npy"))
    n = int(secs * FS)
    assert h.dtype == p.dtype == np.float32 and h.size == p.size == C * n
    b = bench()
    for c in range(C):
        rh, rp, _ = o.HPRIOffline(FS, 4096, 256, 2.0, 2.0).process(b.s_music(n, seed=7000 + c))
        assert np.array_equal(h[c * n:(c + 1) * n], rh) and np.array_equal(p[c * n:(c + 1) * n], rp), c
