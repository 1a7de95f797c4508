"""bench.py's own N-rank launcher on the GPU (VERDICT r05 "Next round" 1): the plain command
`python3 bench.py --gpus 2 ...`, with no torch.distributed.run around it, must measure two ranks.
Both ranks share the box's one GPU (--share-gpu) and exchange their write segments over gloo."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_gpus2_launches_two_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo",
                        "--share-gpu", "--steps", "5", "--warmup", "2", "--no-cpu-baseline", "--deadline", "240"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2
    assert res["config"]["parallelism"] == "replicas2"
    assert res["value"] > 0 and res["steps"] == 5
    assert res["amdahl"]["predicted_speedup_vs_1gpu"] == pytest.approx(2 * 1.1 / 1.3, abs=1e-3)


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_round(orc, tmp_path):
    """A plain run (no --full) prints the headline fields only and, with --dump-outputs, writes the
    Get responses of its last timed round: bit-exact with the CPU oracle fed the same seeded
    batches (the device generators equal the oracle's), so two runs give identical files."""
    import numpy as np

    W, R, pf, ks, steps, warm, pool = 2000, 18000, 4096, 10_000, 3, 2, 4
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warm), "--ops-per-gpu", str(W + R), "--log2-slots", "16", "--prefill", str(pf),
                        "--key-space", str(ks), "--pool", str(pool), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["steps"] == steps and res["value"] > 0 and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx((W + R) / res["ms_per_step"] / 1e3, rel=1e-3)
    for moved in ("roofline", "round", "variants", "cpu_baseline"):
        assert moved not in res
    got = {n: np.load(tmp_path / (n + ".npy")) for n in ("get_flags", "get_vals_lo", "get_vals_hi")}
    assert sorted(f.name for f in tmp_path.iterdir()) == sorted(n + ".npy" for n in got)
    assert got["get_flags"].dtype == np.float32 and got["get_vals_lo"].dtype == got["get_vals_hi"].dtype == np.float64

    seed0 = 0x4E52475055310001  # bench.py's rank-0 seeds: batch p has keys 3p, values 3p + 1, Get keys 3p + 2
    om = orc.HashMap()
    om.prefill_range(pf, 1)
    P = min(pool, steps + warm)
    rounds = [i % P for i in range(warm)] + [i % P for i in range(steps)]
    for b in rounds:
        om.replay(orc.gen_uniform(W, seed0 + 3 * b, ks), orc.gen_raw(W, seed0 + 3 * b + 1))
    v, f = om.get_batch(orc.gen_uniform(R, seed0 + 3 * rounds[-1] + 2, ks))
    assert 0 < f.sum() < R  # both found and absent keys
    v = v * (f != 0)
    np.testing.assert_array_equal(got["get_flags"], f.astype(np.float32))
    np.testing.assert_array_equal(got["get_vals_lo"], (v & np.uint64(0xFFFFFFFF)).astype(np.float64))
    np.testing.assert_array_equal(got["get_vals_hi"], (v >> np.uint64(32)).astype(np.float64))
