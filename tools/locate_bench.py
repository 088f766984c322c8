"""Time the registry's block locator behind a MultiGet (seb_registry_locate_dev after
seb_registry_multiget_list_dev) on the bench's LSM layouts: keygen.lsm_files' 28-file `lsm` or
244-file `lsm_wide` registry and their 10M-key batch (half present).

Each file's sparse index is ASSUMED, not taken from a real SSTable: every 32nd key of the file, with
BlockOffset 4096 * block.  32 entries per 4 KiB block corresponds to roughly 100-byte values with
16-byte keys (lsm/sstable_builder.go:113-117 starts a block when the next entry would overflow it).

Timed with seb.Timer (no L2-flushing completion fence), 30 warm-up + 20 timed steps, the regime of
bench.py's secondary lines: first multiget_list_dev alone, then multiget_list_dev + locate_dev, then
locate_dev alone on the same rows.
Before timing, the first 100K keys' answers are checked against a host bisection.  Prints one JSON
line: both times, the live cells, the dependent 16-B gathers per live cell (the bisection's probe
count, replayed on the host) and the gather rate the added time implies as a fraction of
bench.gather_ceiling().  No pass/fail threshold.

    python tools/locate_bench.py [--wide] [--out profiles/locate_bench.jsonl]
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

ENTRIES_PER_BLOCK = 32
NO_BLOCK = np.uint64(2**64 - 1)


def index_block(idx: np.ndarray) -> tuple[bytes, np.ndarray]:
    """The encoded index of a file holding keys key16(2 * idx): every 32nd key, offset 4096 * block.
    Returns (block bytes, the index entries' key numbers)."""
    first = 2 * idx[::ENTRIES_PER_BLOCK]
    ent = np.zeros(len(first), dtype=np.dtype([("ks", "<u4"), ("bo", "<u8"), ("key", "u1", 16)]))
    assert ent.dtype.itemsize == 28
    ent["ks"] = 16
    ent["bo"] = 4096 * np.arange(len(first), dtype=np.uint64)
    ent["key"] = kg.key16(first)
    return np.uint32(len(first)).tobytes() + ent.tobytes(), first


def bisect_steps(n_entries: int, pos: np.ndarray) -> np.ndarray:
    """Probes of the locator's upper-bound bisection over n_entries for cells whose answer (the
    count of entries <= key) is pos: the loop of k_locate replayed."""
    a = np.zeros(len(pos), np.int64)
    b = np.full(len(pos), n_entries, np.int64)
    steps = np.zeros(len(pos), np.int64)
    while True:
        live = a < b
        if not live.any():
            return steps
        mid = (a + b) >> 1
        steps += live
        right = live & (mid < pos)  # entry mid <= key
        a = np.where(right, mid + 1, a)
        b = np.where(live & ~right, mid, b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide", action="store_true", help="the 244-file lsm_wide layout (default: lsm, 28 files)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--sample", type=int, default=100_000, help="keys checked against the host bisection")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()

    import torch

    import bench
    import seb_bloom as seb

    seb.device_check(0)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lay = kg.LSM_WIDE_LAYOUT if a.wide else kg.LSM_LAYOUT
    files = kg.lsm_files(lay)
    reg = seb.Registry(0)
    first_of = {}  # slot -> the index entries' key numbers (key16(i) sorts as i does)
    index_bytes = 0
    for level, file_num, idx in files:
        m, k = seb.params(len(idx), 0.01)
        keys = torch.from_numpy(kg.key16(2 * idx)).to(dev)
        w = seb.new_words(m, device=dev)
        seb.dev_build(seb.dev_keys(keys, n=len(idx), stride=16), w, m, k)
        block = m.to_bytes(8, "little") + k.to_bytes(4, "little") + seb.words_to_bits(w, m).tobytes()
        slot = reg.put(file_num, level, block, kg.key16_bytes(int(2 * idx[0])), kg.key16_bytes(int(2 * idx[-1])))
        iblock, first = index_block(idx)
        reg.put_index(file_num, iblock)
        first_of[slot] = first
        index_bytes += 40 * len(first)  # device arrays: 16-B prefix, offset, key offset, 16 key bytes
    n = lay["probes"]
    pidx = kg.lsm_probe_indices(lay)
    pk = seb.dev_keys(torch.from_numpy(kg.key16(pidx)).to(dev), n=n, stride=16)
    cap = reg.max_candidates()
    rows = torch.zeros(n * cap, dtype=torch.int16, device=dev)
    blocks = torch.zeros(n * cap, dtype=torch.int64, device=dev)
    reg.multiget_list_dev(pk, rows, cap)
    reg.locate_dev(pk, rows, blocks, cap)
    torch.cuda.synchronize()

    # the answers, once, against the host bisection; and the work of the whole call
    cand = rows.cpu().numpy().view(np.uint16).reshape(n, cap)
    got = blocks.cpu().numpy().view(np.uint64).reshape(n, cap)
    live_cells, gathers, checked = 0, 0, 0
    for slot, first in first_of.items():
        sel = cand == slot
        pos = np.searchsorted(first, pidx[np.nonzero(sel)[0]], side="right")  # row-major: the first keys' cells first
        live_cells += int(sel.sum())
        gathers += int(bisect_steps(len(first), pos).sum())
        s = sel[: a.sample]
        want = np.where(pos[: int(s.sum())] > 0, np.uint64(4096) * (pos[: int(s.sum())] - 1).astype(np.uint64), NO_BLOCK)
        assert np.array_equal(got[: a.sample][s], want), f"slot {slot}: locate differs from the host bisection"
        checked += int(s.sum())
    pad = cand[: a.sample] == 0xFFFF
    assert (got[: a.sample][pad] == NO_BLOCK).all(), "a padded cell holds a block offset"

    def timed(step):
        for _ in range(a.warmup):
            step()
        t = [seb.Timer() for _ in range(a.steps + 1)]
        t[0].record()
        for j in range(a.steps):
            step()
            t[j + 1].record()
        torch.cuda.synchronize()
        return [t[j].elapsed_ms(t[j + 1]) for j in range(a.steps)]

    def both():
        reg.multiget_list_dev(pk, rows, cap)
        reg.locate_dev(pk, rows, blocks, cap)

    mg = timed(lambda: reg.multiget_list_dev(pk, rows, cap))
    mgl = timed(both)
    alone = timed(lambda: reg.locate_dev(pk, rows, blocks, cap))  # the rows of the last MultiGet, again and again
    ceiling, src = bench.gather_ceiling()
    added_ms = float(np.median(mgl) - np.median(mg))
    rate = gathers / (added_ms * 1e-3) / 1e9 if added_ms > 0 else None
    line = {
        "tool": "locate_bench", "layout": "lsm_wide" if a.wide else "lsm", "files": len(files), "keys": n, "cap": cap,
        "index": f"ASSUMED: every {ENTRIES_PER_BLOCK}nd key of each file, offset 4096 * block (not from a real SSTable)",
        "index_entries": int(sum(len(f) for f in first_of.values())), "index_device_bytes": index_bytes,
        "steps": a.steps, "warmup": a.warmup,
        "multiget_ms": {"median": round(float(np.median(mg)), 4), "min": round(min(mg), 4), "max": round(max(mg), 4)},
        "multiget_locate_ms": {"median": round(float(np.median(mgl)), 4), "min": round(min(mgl), 4),
                               "max": round(max(mgl), 4)},
        "locate_added_ms": round(added_ms, 4),
        "locate_alone_ms": {"median": round(float(np.median(alone)), 4), "min": round(min(alone), 4),
                            "max": round(max(alone), 4)},
        "cells": n * cap, "live_cells": live_cells, "gathers": gathers,
        "gathers_per_live_cell": round(gathers / max(live_cells, 1), 3),
        "locate_ggathers_s": round(rate, 3) if rate else None,
        "gather_ceiling_ggathers_s": ceiling, "gather_ceiling_source": src,
        "gather_rate_of_ceiling": round(rate / ceiling, 4) if rate and ceiling else None,
        "checked": f"{checked} live cells of the first {a.sample} keys equal the host bisection",
        "multiget_order_fallbacks": int(seb.lib().seb_multiget_order_fallbacks()),
    }
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    reg.close()


if __name__ == "__main__":
    main()
