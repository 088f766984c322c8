"""Time the WAL replay (seb_dev_wal_replay_plan, seb_dev_wal_replay_emit) on the two shapes the engine produces,
with keygen.wal_image's layout: 16-byte keys (keygen.key16), 100-byte values, a Delete (no value) every 16th
record, sequence i + 1.

  flush     50,000 records, all keys distinct: a full memtable, the reference's flush size
  recovery  2,000,000 records whose keys are drawn uniformly from 3,295,000, so that about a quarter of the
            records are overwritten by a later record of their key

Before any timing the device's six output arrays and sizes must equal the host half (seb_wal_replay_emit) byte
for byte.  Then, with seb.Timer (no L2-flushing fence), --warmup + --steps steps per shape, plan and emit timed
separately (the plan ends in its own synchronise, the emit is followed by one).  Yardsticks, printed with the
times: the byte floor = (the image read once + the 32-byte sort records written and read once per pass + the
survivors' key and value bytes read and written) / the 4.4 TB/s stream rate of DESIGN.md 5.7, and the host half
on one thread over the same input (it stands in for the reference, whose sorted-slice insert per record is
quadratic).  One JSON line per shape; no pass/fail threshold.

    python tools/replay_bench.py [--out profiles/replay_bench.jsonl]
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

STREAM_TBS = 4.4  # the 16-B vector stream rate
TILE = 1024
SHAPES = {"flush": (50_000, None), "recovery": (2_000_000, 3_295_000)}


def make_shape(name: str):
    """(image u8, offsets u64[n + 1]); the CRC fields stay zero: the replay does not read them."""
    n, universe = SHAPES[name]
    img, off = kg.wal_image(n, seal=False)
    if universe is not None:
        draws = np.random.default_rng(5).integers(0, universe, n)
        keys = kg.key16(draws.astype(np.int64))
        st = off[:-1].astype(np.int64)
        for b in range(16):
            img[st + 21 + b] = keys[:, b]
    return img, off


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def run_shape(torch, seb, name, steps, warmup, host):
    dev = torch.device("cuda", 0)
    img, off = make_shape(name)
    n = len(off) - 1
    dimg = torch.from_numpy(img).to(dev)
    doff = torch.from_numpy(off.view(np.int64)).to(dev)
    ws = torch.empty(seb.dev_wal_replay_workspace_size(n), dtype=torch.uint8, device=dev)
    sizes = seb.dev_wal_replay_plan(dimg, doff, ws)
    _, n_out, kb, vb, overwritten, tombstones, _, _ = sizes
    keys = torch.empty(kb, dtype=torch.uint8, device=dev)
    vals = torch.empty(vb, dtype=torch.uint8, device=dev)
    koff = torch.empty(n_out + 1, dtype=torch.int64, device=dev)
    voff = torch.empty(n_out + 1, dtype=torch.int64, device=dev)
    dele = torch.empty(n_out, dtype=torch.uint8, device=dev)
    seq = torch.empty(n_out, dtype=torch.int64, device=dev)
    for t in (keys, vals, dele):
        t.fill_(0xA5)
    seb.dev_wal_replay_emit(dimg, doff, sizes, ws, keys, koff, vals, voff, dele, seq)
    torch.cuda.synchronize()
    # bit-exact check against the host half, which is also the one-thread yardstick: one walk with stores (it
    # refuses sizes that are not its own plan's, so the device's sizes are checked on the way)
    t0 = time.perf_counter()
    want = seb.wal_replay_emit(img, off, sizes=sizes)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert sizes == want[6], (sizes, want[6])
    for got, ref, what in ((keys, want[0], "keys"), (koff, want[1].view(np.int64), "key_off"), (vals, want[2], "vals"),
                           (voff, want[3].view(np.int64), "val_off"), (dele, want[4], "deleted"),
                           (seq, want[5].view(np.int64), "seq")):
        assert np.array_equal(got.cpu().numpy(), ref), f"{what} differs from the host half"
    del want
    t = [seb.Timer() for _ in range(3)]
    plan_ms, emit_ms = [], []
    for step in range(warmup + steps):
        t[0].record()
        seb.dev_wal_replay_plan(dimg, doff, ws)
        t[1].record()
        seb.dev_wal_replay_emit(dimg, doff, sizes, ws, keys, koff, vals, voff, dele, seq)
        t[2].record()
        torch.cuda.synchronize()
        if step >= warmup:
            plan_ms.append(t[0].elapsed_ms(t[1]))
            emit_ms.append(t[1].elapsed_ms(t[2]))
    tiles = -(-n // TILE)
    passes = max(tiles - 1, 0).bit_length()
    floor_bytes = int(img.size) + 32 * n * 2 * (passes + 1) + 2 * (kb + vb)
    out = {"bench": "replay", "shape": name, "records_in": n, "entries_out": n_out, "overwritten": overwritten,
           "tombstones": tombstones, "image_bytes": int(img.size), "key_bytes": kb, "val_bytes": vb, "tiles": tiles,
           "passes": passes, "workspace_bytes": ws.numel(), "steps": steps, "warmup": warmup, "plan": stats(plan_ms),
           "emit": stats(emit_ms), "floor_ms": round(floor_bytes / (STREAM_TBS * 1e12) * 1e3, 4)}
    total = out["plan"]["median_ms"] + out["emit"]["median_ms"]
    out["total_median_ms"] = round(total, 4)
    out["floor_share_of_total"] = round(out["floor_ms"] / total, 4)
    if host:
        out["host_one_thread_ms"] = round(host_ms, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["flush", "recovery", "both"], default="both")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="leave the one-thread host yardstick out of the line")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    import seb_bloom as seb

    seb.device_check(0)
    torch.cuda.set_device(0)
    for name in (("flush", "recovery") if a.shape == "both" else (a.shape,)):
        line = json.dumps(run_shape(torch, seb, name, a.steps, a.warmup, not a.no_host))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
