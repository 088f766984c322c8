"""Time the miss path of the block-id step on getpath_bench's trees with NO file resident: every
located cell of the bench's 10,000,000-key batch is a miss, and its (slot, block offset) pair must be numbered
among the distinct pairs in order of first appearance.

  device  seb_dev_block_ids_plan + seb_dev_block_ids_emit on the cells where the locate left them; max_uniq = the
          tree's block count (the number of blocks in the files that are not resident)
  host    what a caller did before: D2H of cand and blocks, seb_blocks_dedup, H2D of bid.  The slot -> file number
          gather seb_blocks_dedup's interface needs is timed apart and not counted.

Before any timing the device's bid and read list must equal the host's for the whole batch (the read list's slots
mapped to file numbers).  Then --warmup + --steps device rounds (seb.Timer events around the plan and the emit; the
plan synchronises, so its event time holds the host's wait as well) and --host-steps host rounds (wall clock).

Model, written before the first run: the kernels read the cells' 10 bytes four times (insert, flags, rank, emit;
the issue's sketch has two) and write 4 bytes of bid, 44 bytes per cell, against DESIGN.md 5.7's 4.4 TB/s; on top
come the table's atomics, for which no rate has been measured on this part: the tool prints the miss cells per
second the plan reached beside the 249 G/s gather ceiling of 5.7, for comparison only (a cell costs at least two
table accesses in the insert pass and one dependent probe chain in each of the three later passes).
One JSON line per shape; no pass/fail threshold.

    python tools/blockids_bench.py [--shape lsm|lsm_wide|both] [--out profiles/blockids_bench.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "storage-engines_amd"), os.path.join(ROOT, "tools")]

import keygen as kg  # noqa: E402
from getpath_bench import SHAPES, build_tree, med  # noqa: E402

STREAM_BYTES_PER_S = 4.4e12
GATHER_PER_S = 249e9          # DESIGN.md 5.7, for comparison only


def note(msg):
    print(f"blockids_bench: {msg}", file=sys.stderr, flush=True)


def run_shape(torch, seb, lay, shape, steps, warmup, host_steps):
    dev = torch.device("cuda", 0)
    note(f"{shape}: building the tree")
    tree = build_tree(torch, seb, lay)
    reg, _, _, blen, nfiles, entries, _ = tree
    n = lay["probes"]
    keys = torch.from_numpy(kg.key16(kg.lsm_probe_indices(lay)).reshape(-1)).to(dev)
    dk = seb.dev_keys(keys, n=n, stride=16)
    cap = reg.max_candidates()
    cells = n * cap
    cand = torch.zeros(cells, dtype=torch.int16, device=dev)
    blocks = torch.zeros(cells, dtype=torch.int64, device=dev)
    reg.multiget_list_dev(dk, cand, cap)
    reg.locate_dev(dk, cand, blocks, cap)
    slot_file = np.zeros(65536, np.uint64)
    for slot, (file_num, _level) in reg.slots().items():
        slot_file[slot] = file_num
    max_uniq = int(blen.numel())
    ws = torch.empty(seb.dev_block_ids_workspace_size(cells, max_uniq), dtype=torch.uint8, device=dev)
    bid = torch.empty(cells, dtype=torch.int32, device=dev)
    us = torch.empty(max_uniq, dtype=torch.int16, device=dev)
    ub = torch.empty(max_uniq, dtype=torch.int64, device=dev)
    t = [seb.Timer() for _ in range(3)]

    def device_round():
        t[0].record()
        sz = seb.dev_block_ids_plan(cand, blocks, cells, None, None, 0, max_uniq, ws)
        t[1].record()
        seb.dev_block_ids_emit(cand, blocks, cells, None, None, 0, max_uniq, 0, sz, ws, bid, us, ub)
        t[2].record()
        torch.cuda.synchronize()
        return sz

    hbid = torch.empty(cells, dtype=torch.int32).pin_memory()

    def host_round():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hc = cand.cpu().numpy().view(np.uint16)
        hb = blocks.cpu().numpy().view(np.uint64)
        t1 = time.perf_counter()
        files = slot_file[hc]
        files[hc == 0xFFFF] = 2**64 - 1
        t2 = time.perf_counter()
        out = seb.blocks_dedup(files, hb)
        t3 = time.perf_counter()
        hbid.copy_(torch.from_numpy(out[0].view(np.int32)))
        bid_back = hbid.to(dev)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        return out, bid_back, dict(d2h=t1 - t0, slot_to_file=t2 - t1, dedup=t3 - t2, h2d=t4 - t3)

    # the device's answer equals the host's for the whole batch, before anything is timed
    note(f"{shape}: {cells} cells located; comparing the device's answer with seb_blocks_dedup's")
    sz = device_round()
    (want_bid, want_files, want_blocks), bid_back, _ = host_round()
    assert torch.equal(bid, bid_back), "bid differs from seb_blocks_dedup's"
    hus = us[: sz.uniq].cpu().numpy().view(np.uint16)
    assert np.array_equal(slot_file[hus], want_files) and np.array_equal(ub[: sz.uniq].cpu().numpy().view(np.uint64), want_blocks), \
        "the read list differs from seb_blocks_dedup's"
    assert sz.uniq == want_files.size and sz.resident == 0 and sz.bad == 0
    del want_bid, bid_back

    note(f"{shape}: equal ({sz.uniq} distinct pairs); timing")
    plan_ms, emit_ms = [], []
    for step in range(warmup + steps):
        device_round()
        if step >= warmup:
            plan_ms.append(t[0].elapsed_ms(t[1]))
            emit_ms.append(t[1].elapsed_ms(t[2]))
    host = []
    for _ in range(host_steps):
        host.append(host_round()[2])
        note(f"{shape}: host round {len(host)} of {host_steps}: {sum(host[-1].values()):.1f} s")
    hm = {k: round(float(np.median([h[k] for h in host])) * 1e3, 3) for k in host[0]} if host else {}
    p, e = med(plan_ms), med(emit_ms)
    line = {"bench": "blockids", "shape": shape, "files": nfiles, "sst_entries": entries, "pool_blocks": max_uniq,
            "small": bool(lay["probes"] != SHAPES[shape]["probes"]), "keys": n, "cap": cap, "cells": cells,
            "misses": sz.misses, "uniq": sz.uniq, "max_uniq": max_uniq,
            "table_slots": 1 << max(2, (2 * min(max_uniq, cells) - 1).bit_length()),
            "workspace_bytes": int(ws.numel()), "steps": steps, "warmup": warmup, "host_steps": host_steps,
            "plan_ms": p, "emit_ms": e, "device_ms": round(p + e, 4),
            "plan_ms_min_max": [round(min(plan_ms), 4), round(max(plan_ms), 4)],
            "model_stream_ms": round(44 * cells / STREAM_BYTES_PER_S * 1e3, 4),
            "miss_cells_per_s_plan": round(sz.misses / (p * 1e-3) / 1e9, 3), "miss_cells_per_s_unit": "G/s",
            "gather_ceiling_g_s_for_comparison_only": GATHER_PER_S / 1e9,
            "host_ms": hm, "host_total_ms": round(hm.get("d2h", 0) + hm.get("dedup", 0) + hm.get("h2d", 0), 3),
            "checked": "bid and the read list equal to seb_blocks_dedup's for the whole batch"}
    if host:
        line["host_over_device"] = round(line["host_total_ms"] / line["device_ms"], 1)
    reg.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=[*SHAPES, "both"], default="both")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=2)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--small", action="store_true", help="a hundredth of every size: a trial of the tool, not a measurement")
    a = ap.parse_args()

    import torch

    import seb_bloom as seb

    seb.device_check(0)
    torch.cuda.set_device(0)
    for shape in (SHAPES if a.shape == "both" else (a.shape,)):
        lay = SHAPES[shape]
        if a.small:
            lay = {k: v // 100 if k.endswith("_keys") or k == "probes" else v for k, v in lay.items()}
        line = json.dumps(run_shape(torch, seb, lay, shape, a.steps, a.warmup, a.host_steps))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
