"""GPU: every bench.py config at N = 1 runs through the same timed loop the driver's bench uses
(warm-up, timed steps, the kernel_timing steps after them) and reports its golden parity, so a
config that no secondary line covers (route, wal, many, c2_sharded, c3_partitioned, c5_2d, the
overlapped c2c3 / c4 steps) cannot rot between rounds.  Times are not asserted."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


@pytest.mark.parametrize("args", [
    ["--config", "route"],
    ["--config", "wal"],
    ["--config", "many"],
    ["--config", "c2_sharded"],
    ["--config", "c3_partitioned"],
    ["--config", "c5_2d"],
    ["--config", "c2c3", "--overlap", "1"],
    ["--config", "c4", "--overlap", "1"],
    ["--config", "c2c3", "--fresh-build", "0"],
], ids=lambda a: "_".join(x.lstrip("-") for x in a[1:]))
def test_bench_config_one_gpu(args):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH, *args, "--full", "--steps", "4", "--warmup", "1", "--kernel-reps", "2",
                        "--no-cpu-baseline", "--no-secondary", "--no-host-inclusive"],
                       capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["value"] > 0
    assert d["parity"].startswith("bit-exact"), d["parity"]
    assert d["cpu_fallbacks"] == 0
    assert d["kernel_timing"]["reps"] == 2


def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """Without --full the line carries the headline figure and nothing that takes work of its own
    after the timed steps; --dump-outputs writes the last timed step's filter and answers, which
    equal the oracle's for the same (deterministic) keys."""
    import numpy as np

    import keygen as kg
    from oracle import oracle_c as oc

    n = 100_003
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--keys", str(n),
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "Mkeys/s" and d["higher_is_better"] is True and d["dtype"] == "u64" and d["metric"]
    assert abs(d["value"] - 2 * n / (d["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * d["value"]
    for moved in ("parity", "kernel_timing", "cpu_baseline", "host_inclusive", "secondary"):
        assert moved not in d, moved
    assert d["cpu_fallbacks"] == 0 and d["roofline"]["achieved"] > 0
    m, k = d["config"]["num_bits"], d["config"]["num_hashes"]
    assert (m, k) == oc.params(n, 0.01)
    ref_bits = oc.build(m, k, kg.key16(np.arange(n)), n, stride=16)
    ref_ans = oc.probe(ref_bits, m, k, kg.key16(kg.probe_indices(n)), n, stride=16)
    words, ans = np.load(tmp_path / "out" / "filter_bits.npy"), np.load(tmp_path / "out" / "answers.npy")
    assert words.dtype == np.float64 and ans.dtype == np.float32
    assert d["outputs"]["arrays"]["answers"] == {"elements": n, "written": n, "dtype": "float32"}
    got = words.astype("<u4").view(np.uint8)
    assert np.array_equal(got[:ref_bits.size], ref_bits) and not got[ref_bits.size:].any()
    assert np.array_equal(ans, ref_ans)
