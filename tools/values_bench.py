"""Time the Get path's last step, the gather of a batch's found values into one dense buffer,
against the torch formulation a caller had to write before it, on tools/getpath_bench.py's `lsm` tree: 28 real
SSTables from the device builder (keys key16(2 i), 100-byte values), their data sections resident on the device as
the block pool, and one 50,000-entry memtable run (every 16th entry a tombstone) with random value bytes.

The batch is --keys keys (default 2,000,000) in random order: a fraction `found` of them present, of which a share
`mem` is drawn from the run's live entries and the rest from the SSTables' keys outside the run; the others are
odd keys, which no file and no run holds.  Pipeline B of the Get path (runs search, compact, list, locate, block
ids, search, resolve, join rows) runs once per shape and leaves status, source, run, vloc and vlen on the device;
then, alternating in one process:

  B  seb_dev_get_values_plan + seb_dev_get_values_emit
  T  torch: lengths -> cumsum -> (one .item() for the total, as the plan synchronises) -> repeat_interleave of each
     key's source offset, output offset and source id by its length, plus a ramp, into one index per output byte;
     then one indexed read and one masked write per source array

Outputs (out_off and out_vals) are compared equal first.  --warmup + --steps rounds, seb.Timer events around each
call; medians.  B's bytes for the model of DESIGN.md 5.18: 15 n read by the plan and again by the emit, 8 (n + 1) of
out_off, the values written, and 227 bytes of source lines per found value (a 100-byte value at a random address
touches (100 + 127) / 128 lines of 128 B on average); the emit's 13 n workspace bytes written and read back, and
out_off read back by the copy, are reported apart as `ws_bytes`.  One JSON line per shape; no pass/fail threshold.

    python tools/values_bench.py [--keys N] [--out profiles/values_bench.jsonl] [--small]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "storage-engines_amd"), os.path.join(ROOT, "tools")]

import getpath_bench as gb  # noqa: E402
import keygen as kg  # noqa: E402

SHAPES = [(1.0, 0.0), (1.0, 0.1), (1.0, 0.5), (0.5, 0.0), (0.5, 0.1), (0.5, 0.5)]  # (found fraction, memtable share)
STREAM_TB_S = 4.4  # DESIGN.md 5.7's measured stream rate


def batch_indices(lay, run_idx, n, found, mem, rng):
    """Key indices (key16 arguments) of the batch: present keys from the run's live entries and from the SSTables'
    keys outside the run, absent keys odd and outside the run."""
    span = lay["l1_files"] * lay["l1_keys"]
    live = run_idx[np.arange(run_idx.size) % 16 != 15]
    n_found = int(round(n * found))
    n_mem = int(round(n_found * mem))
    in_run = np.zeros(2 * span + 2, bool)
    in_run[run_idx] = True

    def outside_run(count, odd):
        got = np.zeros(0, np.int64)
        while got.size < count:
            c = 2 * rng.integers(0, span, 2 * (count - got.size) + 16) + odd
            got = np.concatenate([got, c[~in_run[c]]])
        return got[:count]

    sst, absent = outside_run(n_found - n_mem, 0), outside_run(n - n_found, 1)
    idx = np.concatenate([live[rng.integers(0, live.size, n_mem)], sst, absent])
    assert idx.size == n
    return idx[rng.permutation(n)]


def get_locations(torch, seb, tree, run, ix, keys, n):
    """Pipeline B of the Get path on the batch: (status u8, source u8, run u8, vloc i64, vlen i32) on the device."""
    reg, first_block, pool, blen, _, _, res = tree
    dev = torch.device("cuda", 0)
    dk = seb.dev_keys(keys, n=n, stride=16)
    cap = reg.max_candidates()
    mem_status = torch.zeros(n, dtype=torch.uint8, device=dev)
    mem_run = torch.zeros(n, dtype=torch.uint8, device=dev)
    mem_vloc = torch.zeros(n, dtype=torch.int64, device=dev)
    mem_vlen = torch.zeros(n, dtype=torch.int32, device=dev)
    seb.dev_runs_search(dk, [run], [ix], mem_status, run=mem_run, vloc=mem_vloc, vlen=mem_vlen)
    ws = torch.empty(seb.dev_get_compact_workspace_size(n), dtype=torch.uint8, device=dev)
    plan = seb.dev_get_compact_plan(dk, mem_status, ws)
    m = plan.undecided
    ck, row = seb.dev_get_compact_emit(dk, mem_status, plan, ws, torch.empty(16 * max(m, 1), dtype=torch.uint8, device=dev), None,
                                       torch.empty(max(m, 1), dtype=torch.int32, device=dev))
    steps = gb.Steps(torch, seb, reg, first_block, pool, blen, max(m, 1), cap, res)
    for _, fn in steps.stages(ck, "lib"):
        fn()
    out = [torch.zeros(n, dtype=d, device=dev) for d in (torch.uint8, torch.uint8, torch.int16, torch.int64, torch.int32)]
    seb.dev_get_join_rows(mem_status, n, row, m, steps.status, *out, mem_vloc=mem_vloc, mem_vlen=mem_vlen, sst_col=steps.col,
                          sst_vloc=steps.vloc, sst_vlen=steps.vlen)
    torch.cuda.synchronize()
    return out[0], out[1], mem_run, out[3], out[4]


def torch_values(torch, status, source, run, vloc, vlen, sources):
    """The torch formulation: sources = [pool, run 0's values, ...]; returns (out_off i64 n + 1, out_vals u8)."""
    n = status.numel()
    lens = torch.where(status == 1, vlen, 0).to(torch.int64)
    out_off = torch.zeros(n + 1, dtype=torch.int64, device=status.device)
    torch.cumsum(lens, 0, out=out_off[1:])
    total = int(out_off[-1].item())
    sid = torch.where(source == 1, 0, run.to(torch.int64) + 1)
    which = torch.repeat_interleave(sid, lens, output_size=total)
    idx = torch.repeat_interleave(vloc - out_off[:-1], lens, output_size=total) + torch.arange(total, device=status.device)
    out = torch.empty(total, dtype=torch.uint8, device=status.device)
    for s, arr in enumerate(sources):
        mask = which == s
        out[mask] = arr[idx[mask]]
    return out_off, out


def run_shape(torch, seb, lay, tree, run, ix, run_idx, run_vals, n, found, mem, steps, warmup):
    dev = torch.device("cuda", 0)
    pool = tree[2]
    rng = np.random.default_rng(lay["seed"] + 7 + int(100 * found) + int(1000 * mem))
    keys = torch.from_numpy(kg.key16(batch_indices(lay, run_idx, n, found, mem, rng)).reshape(-1)).to(dev)
    status, source, mrun, vloc, vlen = get_locations(torch, seb, tree, run, ix, keys, n)
    ws = torch.empty(seb.dev_get_values_workspace_size(n), dtype=torch.uint8, device=dev)
    args = (status, source, mrun, vloc, vlen, n, [run_vals], pool)
    sizes = seb.dev_get_values_plan(*args, ws)
    out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    out_vals = torch.empty(max(sizes.val_bytes, 1), dtype=torch.uint8, device=dev)
    seb.dev_get_values_emit(*args, sizes, ws, out_off, out_vals)
    t_off, t_vals = torch_values(torch, status, source, mrun, vloc, vlen, [pool, run_vals])
    torch.cuda.synchronize()
    assert torch.equal(out_off, t_off), "out_off differs between the library and the torch formulation"
    assert t_vals.numel() == sizes.val_bytes and torch.equal(out_vals[: sizes.val_bytes], t_vals), "out_vals differs"
    found_n, mem_n = sizes.found, int(((status == 1) & (source == 0)).sum())
    del t_off, t_vals
    tp, te, tt = [], [], []
    t = [seb.Timer() for _ in range(5)]
    for step in range(warmup + steps):
        t[0].record()
        sz = seb.dev_get_values_plan(*args, ws)
        t[1].record()
        seb.dev_get_values_emit(*args, sz, ws, out_off, out_vals)
        t[2].record()
        torch.cuda.synchronize()
        t[3].record()
        r = torch_values(torch, status, source, mrun, vloc, vlen, [pool, run_vals])
        t[4].record()
        torch.cuda.synchronize()
        del r
        if step >= warmup:
            tp.append(t[0].elapsed_ms(t[1])), te.append(t[1].elapsed_ms(t[2])), tt.append(t[3].elapsed_ms(t[4]))
    b = [p + e for p, e in zip(tp, te)]
    model_bytes = 30 * n + 8 * (n + 1) + sizes.val_bytes + 227 * found_n
    ws_bytes = 2 * 13 * n + 8 * n
    b_ms = gb.med(b)
    return {"bench": "values", "shape": "lsm", "keys": n, "found_target": found, "mem_target": mem, "found": found_n,
            "from_memtable": mem_n, "val_bytes": sizes.val_bytes, "pool_bytes": int(pool.numel()), "run_entries": gb.RUN_ENTRIES,
            "steps": steps, "warmup": warmup,
            "B_ms": {"median": b_ms, "min": round(min(b), 4), "max": round(max(b), 4)},
            "B_plan_ms": gb.med(tp), "B_emit_ms": gb.med(te),
            "T_ms": {"median": gb.med(tt), "min": round(min(tt), 4), "max": round(max(tt), 4)},
            "B_over_T": round(b_ms / gb.med(tt), 4),
            "model_bytes": model_bytes, "ws_bytes": ws_bytes, "model_ms": round(model_bytes / (STREAM_TB_S * 1e12) * 1e3, 4),
            "B_gb_s": round(model_bytes / (b_ms * 1e-3) / 1e9, 1), "emit_gb_s": round((model_bytes - 15 * n) / (gb.med(te) * 1e-3) / 1e9, 1),
            "checked": "out_off and out_vals equal between the library and the torch formulation"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=2_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--small", action="store_true", help="a hundredth of every size: a trial of the tool, not a measurement")
    a = ap.parse_args()

    import torch

    import seb_bloom as seb

    seb.device_check(0)
    torch.cuda.set_device(0)
    lay = gb.SHAPES["lsm"]
    n = a.keys
    if a.small:
        lay = {k: v // 100 if k.endswith("_keys") or k == "probes" else v for k, v in lay.items()}
        n = max(n // 100, 1000)
    tree = gb.build_tree(torch, seb, lay)
    run, ix, run_idx = gb.make_run(torch, seb, lay)
    live_bytes = gb.VALUE_BYTES * int((np.arange(gb.RUN_ENTRIES) % 16 != 15).sum())
    run_vals = torch.randint(0, 256, (live_bytes,), dtype=torch.uint8, device="cuda")
    for found, mem in SHAPES:
        rec = run_shape(torch, seb, lay, tree, run, ix, run_idx, run_vals, n, found, mem, a.steps, a.warmup)
        rec["small"] = bool(a.small)
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
        torch.cuda.empty_cache()
    tree[0].close()


if __name__ == "__main__":
    main()
