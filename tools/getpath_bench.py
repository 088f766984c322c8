"""Time the batched Get behind the memtable lookup, with and without the compaction of undecided keys,
on the bench's LSM layouts: keygen.lsm_files' 28-file `lsm` or 244-file `lsm_wide` registry, every file a real
SSTable from the device builder (keys key16(2 i), 100-byte values), the files' data sections resident on the
device as the block pool, every index registered.

The batch is keygen.lsm_probe_indices' 10,000,000 keys; a fraction f of its positions, chosen at random, is
replaced by keys drawn at random from one 50,000-entry memtable run (every 16th entry a tombstone), so with random
hits every cache line of the batch holds keys of both kinds.  seb_dev_runs_search gives mem_status once per f;
both pipelines start behind it:

  A  (the whole batch)  MultiGet list -> locate -> block ids -> block search -> resolve -> seb_dev_get_join
  B  (undecided only)   seb_dev_get_compact_plan + _emit -> the same five steps on m keys -> seb_dev_get_join_rows

"block ids" maps (slot, block offset) to a block of the pool, in both pipelines: --ids torch with a few torch
element-wise ops (what a caller had to write before DESIGN.md 5.17), --ids lib with seb_dev_block_ids_resident (every
file of these trees is resident), --ids both with the two alternating in one process, a JSON line each.  The
stage's time is reported apart; for lib also its byte rate over 14 bytes per cell (2 of cand, 8 of blocks, 4 of
bid).  Before any timing, A's and B's outputs for the whole batch must be equal: status and source for every key,
col, vloc and vlen for the undecided ones; and the library's bid must equal the torch path's for the whole batch.
Then A and B alternate in one process, --warmup + --steps times, seb.Timer events (no L2-flushing fence) between the
stages; the median of each stage and of each pipeline's total is reported, with the byte rates the compaction and the
two join launches reached against the streams they move:
  compaction  2 n status bytes (read by the plan and by the emit) + 16 n key bytes + 20 m bytes written
  join rows   n (1 + 8 + 4) read + 16 n written, then m (4 + 1 + 1 + 2 + 8 + 4) read + 15 m scattered
One JSON line per (shape, f, block-id stage); no pass/fail threshold.

    python tools/getpath_bench.py [--shape lsm|lsm_wide|both] [--ids torch|lib|both] [--out profiles/getpath_bench.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "storage-engines_amd")]

import keygen as kg  # noqa: E402

RUN_ENTRIES = 50_000
VALUE_BYTES = 100
FRACTIONS = (0.0, 0.1, 0.5, 0.9)
SHAPES = {"lsm": kg.LSM_LAYOUT, "lsm_wide": kg.LSM_WIDE_LAYOUT}


def build_tree(torch, seb, lay):
    """(registry, first_block: slot -> the file's first block in the pool, pool, blen, files, entries, res: the
    residency table (res_first, res_count) as seb_dev_block_ids_* take it, one u32 per slot in use)."""
    dev = torch.device("cuda", 0)
    files = kg.lsm_files(lay)
    counts = [len(idx) for _, _, idx in files]
    total = int(sum(counts))
    keys = torch.empty(total * 16, dtype=torch.uint8, device=dev)
    at = 0
    for _, _, idx in files:
        keys[16 * at: 16 * (at + len(idx))] = torch.from_numpy(kg.key16(2 * idx).reshape(-1)).to(dev)
        at += len(idx)
    dk = seb.dev_keys(keys, n=total, stride=16)
    vals = torch.zeros(total * VALUE_BYTES, dtype=torch.uint8, device=dev)
    voff = torch.arange(total + 1, dtype=torch.int64, device=dev) * VALUE_BYTES
    file_begin = np.concatenate([[0], np.cumsum(counts)]).tolist()
    ws = torch.empty(seb.dev_sst_workspace_size(total, len(files)), dtype=torch.uint8, device=dev)
    sizes = seb.dev_sst_plan(dk, voff, file_begin, ws)
    assert all(s[4] == 0 for s in sizes)
    nblocks = sum(s[0] for s in sizes)
    pool = torch.empty(sum(s[1] for s in sizes), dtype=torch.uint8, device=dev)
    index = torch.empty(sum(s[2] for s in sizes), dtype=torch.uint8, device=dev)
    meta = torch.empty(sum(s[3] for s in sizes), dtype=torch.uint8, device=dev)
    blen = torch.empty(nblocks, dtype=torch.int16, device=dev)
    seb.dev_sst_encode(dk, vals, voff, None, file_begin, sizes, ws, pool, index, meta, blen)
    torch.cuda.synchronize()
    del vals, voff, ws, meta
    hindex = index.cpu().numpy().tobytes()
    reg = seb.Registry(0)
    first_block = torch.full((65536,), -1, dtype=torch.int64, device=dev)
    res_first, res_count = np.full(65536, 2**32 - 1, np.uint32), np.zeros(65536, np.uint32)
    at = at_index = at_block = 0
    for (level, file_num, idx), s in zip(files, sizes):
        m, k = seb.params(len(idx), 0.01)
        w = seb.new_words(m, device=dev)
        seb.dev_build(seb.dev_keys(keys[16 * at: 16 * (at + len(idx))], n=len(idx), stride=16), w, m, k)
        block = m.to_bytes(8, "little") + k.to_bytes(4, "little") + seb.words_to_bits(w, m).tobytes()
        slot = reg.put(file_num, level, block, kg.key16_bytes(int(2 * idx[0])), kg.key16_bytes(int(2 * idx[-1])))
        reg.put_index(file_num, hindex[at_index: at_index + s[2]])
        first_block[slot] = at_block
        res_first[slot], res_count[slot] = at_block, s[0]
        at += len(idx)
        at_index += s[2]
        at_block += s[0]
    slots = int(np.nonzero(res_count)[0].max()) + 1
    res = tuple(torch.from_numpy(a[:slots].view(np.int32).copy()).to(dev) for a in (res_first, res_count))
    return reg, first_block, pool, blen, len(files), total, res


def make_run(torch, seb, lay):
    """One memtable run of RUN_ENTRIES key16 keys over the tree's key range, half of them also in the SSTables."""
    rng = np.random.default_rng(lay["seed"] + 2)
    span = 2 * lay["l1_files"] * lay["l1_keys"]
    idx = np.sort(rng.choice(span, RUN_ENTRIES, replace=False)).astype(np.int64)
    dele = (np.arange(RUN_ENTRIES) % 16 == 15).astype(np.uint8)
    voff = np.concatenate([[0], np.cumsum(np.where(dele == 1, 0, VALUE_BYTES))]).astype(np.int64)
    dev = torch.device("cuda", 0)
    run = seb.dev_run(torch.from_numpy(kg.key16(idx).reshape(-1)).to(dev),
                      (torch.arange(RUN_ENTRIES + 1, dtype=torch.int64) * 16).to(dev), torch.from_numpy(voff).to(dev),
                      torch.from_numpy(dele).to(dev), torch.arange(1, RUN_ENTRIES + 1, dtype=torch.int64).to(dev))
    ix = torch.empty(seb.dev_run_index_size(run.n), dtype=torch.uint8, device=dev)
    seb.dev_run_index(run, ix)
    return run, ix, idx


class Steps:
    """The five SSTable steps on up to `n` keys, with their buffers."""

    def __init__(self, torch, seb, reg, first_block, pool, blen, n, cap, res):
        dev = torch.device("cuda", 0)
        self.torch, self.seb, self.reg, self.first_block, self.pool, self.blen, self.cap = torch, seb, reg, first_block, pool, blen, cap
        self.res_first, self.res_count = res
        self.cand = torch.zeros(n * cap, dtype=torch.int16, device=dev)
        self.blocks = torch.zeros(n * cap, dtype=torch.int64, device=dev)
        self.bid = torch.zeros(n * cap, dtype=torch.int32, device=dev)
        self.cells = torch.zeros(n * cap, dtype=torch.int32, device=dev)
        self.status = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.col = torch.zeros(n, dtype=torch.int16, device=dev)
        self.vloc = torch.zeros(n, dtype=torch.int64, device=dev)
        self.vlen = torch.zeros(n, dtype=torch.int32, device=dev)

    def stages(self, dk, ids="torch"):
        """[(name, callable)] for the batch dk; ids: the block-id stage by torch ops or by the library."""
        torch, seb, cap, k = self.torch, self.seb, self.cap, dk.n * self.cap

        def bid_torch():
            first = self.first_block[self.cand[:k].to(torch.int64) & 0xFFFF]
            first = torch.where((self.blocks[:k] < 0) | (first < 0), -1, first + (self.blocks[:k] >> 12))
            self.bid[:k].copy_(first)

        def bid_lib():
            seb.dev_block_ids_resident(self.cand, self.blocks, k, self.res_first, self.res_count, self.res_first.numel(),
                                       self.bid)

        bid = bid_lib if ids == "lib" else bid_torch

        return [("list", lambda: self.reg.multiget_list_dev(dk, self.cand, cap)),
                ("locate", lambda: self.reg.locate_dev(dk, self.cand, self.blocks, cap)),
                ("block_ids", bid),
                ("search", lambda: seb.dev_search_blocks(dk, self.bid, cap, self.pool, self.blen, self.cells)),
                ("resolve", lambda: seb.dev_resolve_rows(self.cells, self.bid, dk.n, cap, self.status, self.col, self.vloc,
                                                         self.vlen))]


def run_pipeline(seb, stages, timers):
    """Runs the stages in order, a timer event in front of each and one behind the last."""
    for (_, fn), t in zip(stages, timers):
        t.record()
        fn()
    timers[len(stages)].record()


def med(x):
    return round(float(np.median(x)), 4)


def run_fraction(torch, seb, lay, tree, run, ix, run_idx, f, steps, warmup, shape, modes=("torch",)):
    """One JSON-ready dict per mode of the block-id stage; with two modes they alternate step by step."""
    reg, first_block, pool, blen, nfiles, entries, res = tree
    dev = torch.device("cuda", 0)
    n = lay["probes"]
    rng = np.random.default_rng(lay["seed"] + 3 + int(100 * f))
    pidx = kg.lsm_probe_indices(lay)
    hit = rng.random(n) < f
    pidx = np.where(hit, run_idx[rng.integers(0, RUN_ENTRIES, n)], pidx)
    keys = torch.from_numpy(kg.key16(pidx).reshape(-1)).to(dev)
    dk = seb.dev_keys(keys, n=n, stride=16)
    cap = reg.max_candidates()
    mem_status = torch.zeros(n, dtype=torch.uint8, device=dev)
    mem_vloc = torch.zeros(n, dtype=torch.int64, device=dev)
    mem_vlen = torch.zeros(n, dtype=torch.int32, device=dev)
    seb.dev_runs_search(dk, [run], [ix], mem_status, vloc=mem_vloc, vlen=mem_vlen)
    A = Steps(torch, seb, reg, first_block, pool, blen, n, cap, res)
    B = Steps(torch, seb, reg, first_block, pool, blen, n, cap, res)
    a_status = torch.zeros(n, dtype=torch.uint8, device=dev)
    a_source = torch.zeros(n, dtype=torch.uint8, device=dev)
    b_out = [torch.zeros(n, dtype=d, device=dev) for d in (torch.uint8, torch.uint8, torch.int16, torch.int64, torch.int32)]
    ws = torch.empty(seb.dev_get_compact_workspace_size(n), dtype=torch.uint8, device=dev)
    out_keys = torch.empty(16 * n, dtype=torch.uint8, device=dev)
    row = torch.empty(n, dtype=torch.int32, device=dev)
    state = {}

    def plan():
        state["sizes"] = seb.dev_get_compact_plan(dk, mem_status, ws)

    def emit():
        state["ck"], _ = seb.dev_get_compact_emit(dk, mem_status, state["sizes"], ws, out_keys, None, row)

    def b_stage(name, ids):
        return lambda: dict(B.stages(state["ck"], ids))[name]()

    def join_rows():
        seb.dev_get_join_rows(mem_status, n, row, state["sizes"].undecided, B.status, *b_out, mem_vloc=mem_vloc,
                              mem_vlen=mem_vlen, sst_col=B.col, sst_vloc=B.vloc, sst_vlen=B.vlen)

    def pipelines(ids):
        a = A.stages(dk, ids) + [("join", lambda: seb.dev_get_join(mem_status, A.status, n, a_status, a_source))]
        b = ([("compact_plan", plan), ("compact_emit", emit)] +
             [(name, b_stage(name, ids)) for name in ("list", "locate", "block_ids", "search", "resolve")] +
             [("join_rows", join_rows)])
        return a, b

    stages_of = {ids: pipelines(ids) for ids in modes}
    a_stages, b_stages = stages_of[modes[0]]
    ta = [seb.Timer() for _ in range(len(a_stages) + 1)]
    tb = [seb.Timer() for _ in range(len(b_stages) + 1)]

    # the library's block ids equal the torch path's for the whole batch, before any timing
    if "lib" in modes:
        t_stages, _ = pipelines("torch")
        run_pipeline(seb, t_stages, ta)
        want_bid = A.bid.clone()
        A.bid.fill_(0x5A5A5A5A)
        run_pipeline(seb, stages_of["lib"][0], ta)
        torch.cuda.synchronize()
        assert torch.equal(A.bid, want_bid), "seb_dev_block_ids_resident's bid differs from the torch path's"
        del want_bid
    # all outputs of the whole batch equal between A and B, before any timing
    run_pipeline(seb, a_stages, ta)
    run_pipeline(seb, b_stages, tb)
    torch.cuda.synchronize()
    m = state["sizes"].undecided
    und = (mem_status != 1) & (mem_status != 2)
    assert int(und.sum()) == m and state["sizes"].key_bytes == 16 * m
    assert torch.equal(row[:m].to(torch.int64), torch.nonzero(und).reshape(-1)), "row is not the undecided keys in order"
    assert torch.equal(b_out[0], a_status) and torch.equal(b_out[1], a_source), "status / source differ between A and B"
    for name, b, a in (("col", b_out[2], A.col), ("vloc", b_out[3], A.vloc), ("vlen", b_out[4], A.vlen)):
        assert torch.equal(b[und], a[und]), f"{name} differs between A and B on the undecided keys"
    found = int((a_status == 1).sum())
    del und

    times = {ids: {"A": [], "B": []} for ids in modes}
    stage_ms = {ids: {"A": {name: [] for name, _ in a_stages}, "B": {name: [] for name, _ in b_stages}} for ids in modes}
    for step in range(warmup + steps):
        for ids in modes:
            sa, sb_ = stages_of[ids]
            run_pipeline(seb, sa, ta)
            run_pipeline(seb, sb_, tb)
            torch.cuda.synchronize()
            if step < warmup:
                continue
            for which, stages, t in (("A", sa, ta), ("B", sb_, tb)):
                times[ids][which].append(t[0].elapsed_ms(t[len(stages)]))
                for j, (name, _) in enumerate(stages):
                    stage_ms[ids][which][name].append(t[j].elapsed_ms(t[j + 1]))
    compact_bytes = 2 * n + 16 * n + 20 * m
    join_bytes = n * 13 + 16 * n + m * 20 + 15 * m
    lines = []
    for ids in modes:
        tm = times[ids]
        a_ms, b_ms = med(tm["A"]), med(tm["B"])
        sa = {k: med(v) for k, v in stage_ms[ids]["A"].items()}
        sb = {k: med(v) for k, v in stage_ms[ids]["B"].items()}
        compact_ms = sb["compact_plan"] + sb["compact_emit"]
        line = {"bench": "getpath", "shape": shape, "ids": ids, "alternating": list(modes), "files": nfiles,
                "sst_entries": entries, "pool_blocks": int(blen.numel()),
                "small": bool(lay["probes"] != SHAPES[shape]["probes"]), "keys": n, "cap": cap, "cells": n * cap,
                "cells_B": m * cap, "run_entries": RUN_ENTRIES, "f_target": f, "decided": n - m, "undecided": m,
                "f_measured": round((n - m) / n, 4), "found": found, "steps": steps, "warmup": warmup,
                "A_ms": {"median": a_ms, "min": round(min(tm["A"]), 4), "max": round(max(tm["A"]), 4)},
                "B_ms": {"median": b_ms, "min": round(min(tm["B"]), 4), "max": round(max(tm["B"]), 4)},
                "B_over_A": round(b_ms / a_ms, 4),
                "A_stage_ms": sa, "B_stage_ms": sb,
                "block_ids_model_ms": {"A": round(14 * n * cap / 4.4e12 * 1e3, 4), "B": round(14 * m * cap / 4.4e12 * 1e3, 4)},
                "block_ids_gb_s": {"A": round(14 * n * cap / (sa["block_ids"] * 1e-3) / 1e9, 1),
                                   "B": round(14 * m * cap / (max(sb["block_ids"], 1e-6) * 1e-3) / 1e9, 1)},
                "compact_ms": round(compact_ms, 4), "compact_bytes": compact_bytes,
                "compact_gb_s": round(compact_bytes / (compact_ms * 1e-3) / 1e9, 1),
                "compact_emit_gb_s": round((n + 16 * n + 20 * m) / (sb["compact_emit"] * 1e-3) / 1e9, 1),
                "join_rows_bytes": join_bytes, "join_rows_gb_s": round(join_bytes / (sb["join_rows"] * 1e-3) / 1e9, 1),
                "checked": "A and B equal on status and source for every key, on col / vloc / vlen for the undecided ones" +
                           ("; the library's bid equal to the torch path's for the whole batch" if "lib" in modes else "")}
        lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=[*SHAPES, "both"], default="both")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--fractions", default=",".join(str(f) for f in FRACTIONS))
    ap.add_argument("--ids", choices=["torch", "lib", "both"], default="torch",
                    help="the block-id stage: torch ops, seb_dev_block_ids_resident, or both alternating in one process")
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
        tree = build_tree(torch, seb, lay)
        run, ix, run_idx = make_run(torch, seb, lay)
        for f in (float(x) for x in a.fractions.split(",")):
            modes = ("torch", "lib") if a.ids == "both" else (a.ids,)
            for rec in run_fraction(torch, seb, lay, tree, run, ix, run_idx, f, a.steps, a.warmup, shape, modes):
                line = json.dumps(rec)
                print(line, flush=True)
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "a") as fh:
                        fh.write(line + "\n")
            torch.cuda.empty_cache()
        tree[0].close()
        del tree, run, ix
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
