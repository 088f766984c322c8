"""Time the batched memtable lookup (seb_dev_run_index, seb_dev_runs_search) on the two shapes the engine produces.
Keys are keygen.key16; the probe batch is 10,000,000 keys in random order, half of them present in the active run:
even q -> key16(4 r) (present), odd q -> key16(4 r + 1) (in neither run), r uniform over the active run's entries.

  flush     one run of 50,000 entries, key16(4 i): a full memtable, the reference's flush size
  two_runs  the same batch against that active run and an immutable run of 131,072 entries: 5,000 of the active
            run's keys (a tenth of them) and key16(4 j + 2), key16(4 j + 3) over the same key range, so the keys
            the active run does not decide bisect the whole of the second run and find nothing

Values are 100 bytes, every 16th entry is a tombstone, sequences are i + 1.  Before any timing the device's six
outputs for the whole batch must equal the host half (seb_runs_search).  Then, with seb.Timer (no L2-flushing
fence), --warmup + --steps searches per shape; the index build (which ends in its own synchronise) is timed by
the host clock.  Printed with the times: the DESIGN.md 5.14 model = streams / 4.4 TB/s + gathers / 249 G/s with
gathers = undecided keys x ceil(log2(n_r + 1)) per run and streams = 16 key bytes + 26 output bytes per key, and
the gather rate the measured time amounts to.  One JSON line per shape; no pass/fail threshold.

    python tools/memget_bench.py [--out profiles/memget_bench.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "storage-engines_amd")]

import keygen as kg  # noqa: E402

STREAM_TBS = 4.4   # the 16-B vector stream rate
GATHER_GS = 249.0  # dependent 16-B gathers from an L2-resident table
PROBES = 10_000_000
ACTIVE, IMMUTABLE, SHARED = 50_000, 131_072, 5_000
SHAPES = ("flush", "two_runs")


def make_run(idx: np.ndarray):
    """The run of key16(idx) for sorted, distinct idx: (keys u8, key_off, val_off, deleted, seq)."""
    n = idx.size
    keys = kg.key16(idx).reshape(-1)
    dele = (np.arange(n) % 16 == 15).astype(np.uint8)
    voff = np.concatenate([[0], np.cumsum(np.where(dele == 1, 0, 100))]).astype(np.uint64)
    return keys, np.arange(n + 1, dtype=np.uint64) * np.uint64(16), voff, dele, np.arange(1, n + 1, dtype=np.uint64)


def make_shape(name: str):
    """(the runs' arrays, active first; the probe batch as an (n, 16) u8 array)."""
    rng = np.random.default_rng(14)
    runs = [make_run(4 * np.arange(ACTIVE, dtype=np.int64))]
    if name == "two_runs":
        own = IMMUTABLE - SHARED
        j = np.arange(own // 2, dtype=np.int64)
        shared = 4 * np.sort(rng.choice(ACTIVE, SHARED, replace=False)).astype(np.int64)
        runs.append(make_run(np.sort(np.concatenate([shared, 4 * j + 2, 4 * j + 3]))))
        assert runs[1][3].size == IMMUTABLE
    r = np.random.default_rng(15).integers(0, ACTIVE, PROBES)
    return runs, kg.key16(np.where(np.arange(PROBES) % 2 == 0, 4 * r, 4 * r + 1))


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def upload(torch, seb, runs, probes):
    """(dev_runs, their index tensors, the device key batch, the six output tensors, index build ms per run)."""
    dev = torch.device("cuda", 0)
    druns, indexes, index_ms = [], [], []
    for keys, koff, voff, dele, seq in runs:
        t = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev) for a in (keys, koff, voff, dele, seq)]
        run = seb.dev_run(*t)
        ix = torch.empty(seb.dev_run_index_size(run.n), dtype=torch.uint8, device=dev)
        seb.dev_run_index(run, ix)  # warm-up: the first launch loads the code object
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seb.dev_run_index(run, ix)
        index_ms.append(round((time.perf_counter() - t0) * 1e3, 4))
        druns.append(run)
        indexes.append(ix)
    n = probes.shape[0]
    dk = seb.dev_keys(torch.from_numpy(probes).to(dev), n=n, stride=16)
    outs = [torch.empty(n, dtype=d, device=dev) for d in (torch.uint8, torch.uint8, torch.int32, torch.int64, torch.int32,
                                                           torch.int64)]
    return druns, indexes, dk, outs, index_ms


def time_search(torch, seb, dk, druns, indexes, outs, steps, warmup):
    t = [seb.Timer() for _ in range(2)]
    ms = []
    for step in range(warmup + steps):
        t[0].record()
        seb.dev_runs_search(dk, druns, indexes, *outs)
        t[1].record()
        torch.cuda.synchronize()
        if step >= warmup:
            ms.append(t[0].elapsed_ms(t[1]))
    return ms


def run_shape(torch, seb, name, steps, warmup):
    runs, probes = make_shape(name)
    druns, indexes, dk, outs, index_ms = upload(torch, seb, runs, probes)
    for o in outs:
        o.view(torch.uint8).fill_(0xA5)
    seb.dev_runs_search(dk, druns, indexes, *outs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = seb.runs_search(probes, [seb.host_run(k, ko, vo, d, s) for k, ko, vo, d, s in runs])
    host_ms = (time.perf_counter() - t0) * 1e3
    views = (np.uint8, np.uint8, np.uint32, np.uint64, np.uint32, np.uint64)
    for o, w, v, what in zip(outs, want, views, ("status", "run", "entry", "vloc", "vlen", "seq")):
        assert np.array_equal(o.cpu().numpy().view(v), w), f"{what} differs from the host half"
    status, run = want[0], want[1]
    ms = time_search(torch, seb, dk, druns, indexes, outs, steps, warmup)
    n = probes.shape[0]
    undecided, gathers = n, 0
    per_run = []
    for r, arrays in enumerate(runs):
        levels = int(arrays[3].size).bit_length()  # ceil(log2(n_r + 1))
        gathers += undecided * levels
        per_run.append({"entries": int(arrays[3].size), "levels": levels, "keys_in": undecided})
        undecided -= int((run == r).sum())
    stream_bytes = n * (16 + 26)
    model_ms = stream_bytes / (STREAM_TBS * 1e12) * 1e3 + gathers / (GATHER_GS * 1e9) * 1e3
    out = {"bench": "memget", "shape": name, "keys": n, "runs": per_run, "found": int((status == 1).sum()),
           "tombstones": int((status == 2).sum()), "none": int((status == 0).sum()), "gathers": gathers,
           "stream_bytes": stream_bytes, "model_ms": round(model_ms, 4), "steps": steps, "warmup": warmup,
           "search": stats(ms), "index_build_ms": index_ms, "host_one_thread_ms": round(host_ms, 1)}
    med = out["search"]["median_ms"]
    out["gather_rate_gs"] = round(gathers / (med * 1e-3) / 1e9, 1)
    out["model_share_of_measured"] = round(model_ms / med, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=[*SHAPES, "both"], default="both")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    import seb_bloom as seb

    seb.device_check(0)
    torch.cuda.set_device(0)
    for name in (SHAPES if a.shape == "both" else (a.shape,)):
        line = json.dumps(run_shape(torch, seb, name, a.steps, a.warmup))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
