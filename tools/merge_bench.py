"""Time the batched compaction merge (seb_dev_merge_count, seb_dev_merge_plan, seb_dev_merge_emit) on the two
shapes the engine produces, with the `lsm` layout's entries: 16-byte keys (keygen.key16), 100-byte values, one
deleted byte per entry (one in 16 set), 125 bytes per entry image, 32 entries per 4 KiB block.

  l0          4 runs x 250,000 entries over the whole key range, 5% of the keys in two runs
  compaction  16 runs, 10M entries: 4 L0-like runs of 250,000 + 12 consecutive disjoint runs of 750,000 (the
              input of tools/sst_bench.py's compaction shape)

Before any timing the device's five output arrays and sizes must equal the host half (seb_merge_emit) byte
for byte.  Then, with seb.Timer (no L2-flushing fence), --warmup + --steps steps per shape, count, plan and
emit timed separately (count and plan end in their own synchronise, the emit is followed by one).
Yardsticks, printed with the times: the byte floor = (the pool read once + the survivors' key and value bytes
read and written) / the 4.4 TB/s stream rate of DESIGN.md 5.7, and the host half on one thread over the same
input.  One JSON line per shape; no pass/fail threshold.

    python tools/merge_bench.py [--out profiles/merge_bench.jsonl]
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

VAL = 100
ENTRY = 9 + 16 + VAL
PER_BLOCK = 32
BLOCK = 4096
STREAM_TBS = 4.4  # the 16-B vector stream rate


def go_sorted(k: np.ndarray) -> np.ndarray:
    be = k.view(">u8").reshape(len(k), 2)
    return k[np.lexsort((be[:, 1], be[:, 0]))]


def run_blocks(keys: np.ndarray, run: int, rng) -> tuple[np.ndarray, np.ndarray]:
    """One sorted run's data section: (blocks x 4096 bytes, true block lengths)."""
    m = len(keys)
    nblk = -(-m // PER_BLOCK)
    ent = np.zeros((nblk * PER_BLOCK, ENTRY), np.uint8)
    ent[:m, 0] = 16
    ent[:m, 4] = VAL
    ent[:m, 8] = rng.integers(0, 16, m) == 5
    ent[:m, 9:25] = keys
    ent[:m, 25] = run  # the value names its run
    ent[:m, 26:] = rng.integers(0, 256, (m, VAL - 1), dtype=np.uint8)
    pool = np.zeros((nblk, BLOCK), np.uint8)
    pool[:, 4:4 + PER_BLOCK * ENTRY] = ent.reshape(nblk, PER_BLOCK * ENTRY)
    cnt = np.full(nblk, PER_BLOCK, np.uint32)
    cnt[-1] = (m - 1) % PER_BLOCK + 1
    pool[:, :4] = cnt.view(np.uint8).reshape(nblk, 4)
    return pool, (4 + cnt * ENTRY).astype(np.uint16)


def l0_runs(first_index: int, step: int):
    """4 sorted key arrays of 250,000 keys each: 952,380 distinct keys, 47,620 of them (5%) in two runs."""
    shared, distinct = 47_620, 952_380
    rng = np.random.default_rng(3)
    idx = rng.permutation(distinct)
    keys = kg.key16(first_index + step * idx.astype(np.int64))
    owner = np.concatenate([np.arange(shared) % 4, (np.arange(shared) + 1) % 4, np.arange(distinct - shared) % 4])
    which = np.concatenate([np.arange(shared), np.arange(shared), np.arange(shared, distinct)])
    return [go_sorted(keys[which[owner == r]]) for r in range(4)]


def make_shape(name: str):
    runs = l0_runs(1, 2)  # odd indices
    if name == "compaction":
        lower = go_sorted(kg.key16(np.arange(9_000_000, dtype=np.int64) * 2))  # even indices: disjoint from L0's
        runs += [lower[r * 750_000:(r + 1) * 750_000] for r in range(12)]
    rng = np.random.default_rng(17)
    pools, blens, run_begin = [], [], [0]
    for r, keys in enumerate(runs):
        p, b = run_blocks(keys, r, rng)
        pools.append(p)
        blens.append(b)
        run_begin.append(run_begin[-1] + len(b))
    return np.concatenate(pools).reshape(-1), np.concatenate(blens), run_begin


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def run_shape(torch, seb, name, steps, warmup, host):
    dev = torch.device("cuda", 0)
    pool, blen, rb = make_shape(name)
    nb = len(blen)
    dpool = torch.from_numpy(pool).to(dev)
    dblen = torch.from_numpy(blen.view(np.int16)).to(dev)
    dcnt = torch.empty(nb, dtype=torch.int16, device=dev)
    run_entries = seb.dev_merge_count(dpool, dblen, rb, dcnt)
    n = sum(run_entries)
    ws = torch.empty(seb.dev_merge_workspace_size(n, nb, len(rb) - 1), dtype=torch.uint8, device=dev)
    sizes = seb.dev_merge_plan(dpool, dblen, rb, dcnt, ws)
    _, n_out, kb, vb, shadowed, _ = sizes
    keys = torch.empty(kb, dtype=torch.uint8, device=dev)
    vals = torch.empty(vb, dtype=torch.uint8, device=dev)
    koff = torch.empty(n_out + 1, dtype=torch.int64, device=dev)
    voff = torch.empty(n_out + 1, dtype=torch.int64, device=dev)
    dele = torch.empty(n_out, dtype=torch.uint8, device=dev)
    for t in (keys, vals, dele):
        t.fill_(0xA5)
    seb.dev_merge_emit(dpool, sizes, ws, keys, koff, vals, voff, dele)
    torch.cuda.synchronize()
    # bit-exact check against the host half, which is also the one-thread yardstick: one walk with stores (it
    # refuses sizes that are not its own plan's, so the device's sizes are checked on the way)
    t0 = time.perf_counter()
    want = seb.merge_emit(pool, blen, rb, sizes=sizes)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert sizes == want[5], (sizes, want[5])
    for got, ref, what in ((keys, want[0], "keys"), (koff, want[1].view(np.int64), "key_off"), (vals, want[2], "vals"),
                           (voff, want[3].view(np.int64), "val_off"), (dele, want[4], "deleted")):
        assert np.array_equal(got.cpu().numpy(), ref), f"{what} differs from the host half"
    del want
    t = [seb.Timer() for _ in range(4)]
    count_ms, plan_ms, emit_ms = [], [], []
    for step in range(warmup + steps):
        t[0].record()
        seb.dev_merge_count(dpool, dblen, rb, dcnt)
        t[1].record()
        seb.dev_merge_plan(dpool, dblen, rb, dcnt, ws)
        t[2].record()
        seb.dev_merge_emit(dpool, sizes, ws, keys, koff, vals, voff, dele)
        t[3].record()
        torch.cuda.synchronize()
        if step >= warmup:
            count_ms.append(t[0].elapsed_ms(t[1]))
            plan_ms.append(t[1].elapsed_ms(t[2]))
            emit_ms.append(t[2].elapsed_ms(t[3]))
    floor_bytes = pool.size + 2 * (kb + vb)
    out = {"bench": "merge", "shape": name, "runs": len(rb) - 1, "entries_in": n, "entries_out": n_out, "shadowed": shadowed,
           "blocks": nb, "pool_bytes": int(pool.size), "key_bytes": kb, "val_bytes": vb, "workspace_bytes": ws.numel(),
           "steps": steps, "warmup": warmup, "count": stats(count_ms), "plan": stats(plan_ms), "emit": stats(emit_ms),
           "floor_ms": round(floor_bytes / (STREAM_TBS * 1e12) * 1e3, 4)}
    total = out["count"]["median_ms"] + out["plan"]["median_ms"] + out["emit"]["median_ms"]
    out["total_median_ms"] = round(total, 4)
    out["floor_share_of_total"] = round(out["floor_ms"] / total, 4)
    if host:
        out["host_one_thread_ms"] = round(host_ms, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["l0", "compaction", "both"], default="both")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="leave the one-thread host yardstick out of the line")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    import seb_bloom as seb

    seb.device_check(0)
    torch.cuda.set_device(0)
    for name in (("l0", "compaction") if a.shape == "both" else (a.shape,)):
        line = json.dumps(run_shape(torch, seb, name, a.steps, a.warmup, not a.no_host))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
