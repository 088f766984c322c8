"""Time the B-tree's read side: the structural check of a page-file image and Get of a key batch.

  tree    --keys-in-tree (10,000,000) 16-byte keys with 100-byte values, bulk-loaded page at a time by numpy: 34
          cells per leaf (a full V2 leaf of this shape), --fanout (170) children per internal page; depth 4, 1.2 GB.
          The keys are distinct random u64s, big-endian, followed by 8 random bytes, in key order.
  batch   --keys (10,000,000) 16-byte keys: all present, or half of them absent (a present key with its last byte
          changed, so it reaches the same leaf), each shuffled and sorted: four batches
  device  seb_dev_bt_get with seb.Timer events around the call; seb_dev_bt_check (which synchronises) with a host
          clock around it
  host    seb_bt_get on the first --host-keys keys of each batch; wall clock

Before any timing the device's kind, level and counts must equal the host half's, and its (status, leaf, pos, vloc,
vlen) the host half's on the first --host-keys keys of every batch.

The LDS copy of the root is a build switch (-DSEB_BT_LDS_ROOT=1, off by default; tools/diag_lib.sh): run this tool once per
library (SEB_LIB_PATH) and compare the lines; `lib` records which one ran.

Dependent loads per key, counted from the code (seb_btree.h bt_page_step): per page the header, and per bisection
step a directory entry, the cell's header at that offset and the key bytes behind the header, three loads that each
need the one before; ceil(log2(cells + 1)) steps per page.  `dependent_loads` multiplies that out for this tree and
`gathers_per_s_g` divides by the time, to set beside the 249 G/s L2-resident gather ceiling of DESIGN.md 5.3 / 5.7.
One JSON line per run; no pass/fail threshold.

    python tools/btree_bench.py [--keys-in-tree N] [--keys N] [--host-keys N] [--out profiles/btree_bench.jsonl]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "storage-engines_amd")]

PAGE = 4096
GATHER_PER_S = 249e9
LEAF_CELL = 1 + 1 + 16 + 100  # varint 16, varint 100, key, value
LEAF_CELLS = (PAGE - 10) // (LEAF_CELL + 2)
NODE_CELL = 1 + 4 + 16


def note(msg):
    print(f"btree_bench: {msg}", file=sys.stderr, flush=True)


def med(xs):
    return round(float(np.median(xs)), 4)


def be32(a):
    return np.asarray(a, dtype=">u4").view(np.uint8).reshape(-1, 4)


def be16(a):
    return np.asarray(a, dtype=">u2").view(np.uint8).reshape(-1, 2)


def header(pages, kind, cells, right, cell_bytes):
    pages[:, 0] = kind
    pages[:, 1:3] = be16(cells)
    pages[:, 3:7] = be32(right)
    pages[:, 7:9] = be16(PAGE - cells.astype(np.int64) * cell_bytes)
    pages[:, 9] = 2


def build_tree(rng, n, fanout):
    """(image u8, keys (n, 16) in key order, cells per level from the root down)."""
    first = np.unique(rng.integers(0, 2**63, int(n * 1.01), dtype=np.uint64))[:n]
    assert first.size == n
    keys = np.empty((n, 16), np.uint8)
    keys[:, :8] = first.astype(">u8").view(np.uint8).reshape(n, 8)
    keys[:, 8:] = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    L = -(-n // LEAF_CELLS)
    levels = []
    leaves = np.zeros((L, PAGE), np.uint8)
    cells = np.full(L, LEAF_CELLS, np.int64)
    cells[-1] = n - (L - 1) * LEAF_CELLS
    right = np.arange(2, L + 2, dtype=np.int64)
    right[-1] = 0
    header(leaves, 2, cells, right, LEAF_CELL)
    for j in range(LEAF_CELLS):
        rows = np.arange(j, n, LEAF_CELLS)
        pg, off = np.arange(rows.size), PAGE - LEAF_CELL * (j + 1)
        leaves[pg, 10 + 2 * j: 12 + 2 * j] = be16(np.full(rows.size, off))
        leaves[pg, off] = 16
        leaves[pg, off + 1] = 100
        leaves[pg, off + 2: off + 18] = keys[rows]
        leaves[pg, off + 18: off + 118] = (rows[:, None] + np.arange(100)[None, :]).astype(np.uint8)  # value byte b of key r = r + b
    levels.append(leaves)
    shape = [LEAF_CELLS]
    low, ids, next_id = keys[::LEAF_CELLS], np.arange(1, L + 1, dtype=np.int64), L + 1
    while ids.size > 1:
        P = -(-ids.size // fanout)
        pages = np.zeros((P, PAGE), np.uint8)
        kids = np.full(P, fanout, np.int64)
        kids[-1] = ids.size - (P - 1) * fanout
        header(pages, 1, kids - 1, ids[::fanout], NODE_CELL)  # the first child is the right pointer
        for j in range(1, fanout):
            rows = np.arange(j, ids.size, fanout)
            pg, off = np.arange(rows.size), PAGE - NODE_CELL * j
            pages[pg, 10 + 2 * (j - 1): 12 + 2 * (j - 1)] = be16(np.full(rows.size, off))
            pages[pg, off] = 16
            pages[pg, off + 1: off + 5] = be32(ids[rows])
            pages[pg, off + 5: off + 21] = low[rows]
        levels.append(pages)
        shape.append(fanout - 1)
        low, ids, next_id = low[::fanout], np.arange(next_id, next_id + P, dtype=np.int64), next_id + P
    shape[-1] = int(levels[-1][0, 1]) * 256 + int(levels[-1][0, 2])  # the root's cells
    meta = np.zeros((1, PAGE), np.uint8)
    meta[0, :16] = np.array([0x42545245, int(ids[0]), next_id, 0], dtype=">u4").view(np.uint8)
    return np.concatenate([meta] + levels).reshape(-1), keys, shape[::-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys-in-tree", type=int, default=10_000_000)
    ap.add_argument("--keys", type=int, default=10_000_000)
    ap.add_argument("--host-keys", type=int, default=None, help="keys of each batch that the host half answers (default: all)")
    ap.add_argument("--fanout", type=int, default=170)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()

    import torch

    import seb_bloom as seb

    seb.device_check(0)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(21)
    n, nprobe = a.keys_in_tree, a.keys
    host_keys = nprobe if a.host_keys is None else min(a.host_keys, nprobe)
    note(f"building a tree of {n} keys")
    t0 = time.perf_counter()
    image, keys, shape = build_tree(rng, n, a.fanout)
    build_s = time.perf_counter() - t0
    meta = seb.bt_open(image)
    nbytes = meta.num_pages * PAGE
    d_image = torch.from_numpy(image).to(dev)
    kind = torch.empty(meta.num_pages, dtype=torch.uint8, device=dev)
    level = torch.empty(meta.num_pages, dtype=torch.uint8, device=dev)
    note(f"{meta.num_pages} pages, cells per level {shape}; the check on both sides")
    t0 = time.perf_counter()
    h_kind, h_level, h_stats = seb.bt_check(image, meta)
    host_check_ms = (time.perf_counter() - t0) * 1e3
    stats = seb.dev_bt_check(d_image, nbytes, meta, kind, level)
    assert stats == h_stats and stats["keys"] == n and stats["bad"] == 0, (stats, h_stats)
    assert np.array_equal(kind.cpu().numpy(), h_kind) and np.array_equal(level.cpu().numpy(), h_level)
    check_ms = []
    for step in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seb.dev_bt_check(d_image, nbytes, meta, kind, level)
        if step >= a.warmup:
            check_ms.append((time.perf_counter() - t0) * 1e3)

    present = keys[rng.integers(0, n, nprobe)]
    half = present.copy()
    half[nprobe // 2:, 15] ^= 0x55
    half = half[rng.permutation(nprobe)]
    order = lambda k: k[np.argsort(k[:, :8].copy().view(">u8").reshape(-1), kind="stable")]  # noqa: E731
    batches = {"shuffled_present": present, "sorted_present": order(present), "shuffled_half_absent": half,
               "sorted_half_absent": order(half)}
    steps = [math.ceil(math.log2(c + 1)) for c in shape]
    dependent = sum(1 + 3 * s for s in steps)
    status = torch.empty(nprobe, dtype=torch.uint8, device=dev)
    source = torch.empty(nprobe, dtype=torch.uint8, device=dev)
    leaf = torch.empty(nprobe, dtype=torch.int32, device=dev)
    pos = torch.empty(nprobe, dtype=torch.int32, device=dev)
    vloc = torch.empty(nprobe, dtype=torch.int64, device=dev)
    vlen = torch.empty(nprobe, dtype=torch.int32, device=dev)
    t = [seb.Timer(), seb.Timer()]
    line = {"bench": "btree", "device": torch.cuda.get_device_name(0), "lib": os.path.relpath(seb.LIB_PATH, ROOT),
            "keys_in_tree": n, "pages": int(meta.num_pages), "image_bytes": int(nbytes), "depth": stats["depth"],
            "cells_per_level": shape, "bisection_steps_per_level": steps, "dependent_loads": dependent, "keys": nprobe,
            "host_keys": host_keys, "steps": a.steps, "warmup": a.warmup, "build_s": round(build_s, 1),
            "small": bool(n != 10_000_000 or nprobe != 10_000_000),
            "check_ms": med(check_ms), "check_ms_min_max": [round(min(check_ms), 4), round(max(check_ms), 4)],
            "host_check_ms": round(host_check_ms, 1), "batches": {}}
    for name, probe in batches.items():
        note(f"{name}: the host half on {host_keys} keys, then the comparison and the timing")
        t0 = time.perf_counter()
        want = seb.bt_get(image, meta, probe[:host_keys])
        host_ms = (time.perf_counter() - t0) * 1e3
        dk = seb.dev_keys(torch.from_numpy(probe.reshape(-1)).to(dev), n=nprobe, stride=16)
        got = []
        for step in range(a.warmup + a.steps):
            t[0].record()
            seb.dev_bt_get(d_image, nbytes, meta, dk, status, leaf, pos, vloc, vlen, source)
            t[1].record()
            torch.cuda.synchronize()
            if step >= a.warmup:
                got.append(t[0].elapsed_ms(t[1]))
        for label, d, w in zip(("status", "leaf", "pos", "vloc", "vlen"), (status, leaf, pos, vloc, vlen), want):
            assert np.array_equal(d[:host_keys].cpu().numpy().view(w.dtype), w), f"{name}: {label} differs from the host half's"
        found = int((status == seb.GET_FOUND).sum())
        assert int((status == seb.GET_ERROR).sum()) == 0
        line["batches"][name] = {"get_ms": med(got), "get_ms_min_max": [round(min(got), 4), round(max(got), 4)], "found": found,
                                 "keys_per_s_g": round(nprobe / (med(got) * 1e-3) / 1e9, 3),
                                 "gathers_per_s_g": round(nprobe * dependent / (med(got) * 1e-3) / 1e9, 1),
                                 "share_of_gather_ceiling": round(nprobe * dependent / (med(got) * 1e-3) / GATHER_PER_S, 3),
                                 "host_ms": round(host_ms, 1), "host_ms_per_batch": round(host_ms * nprobe / max(host_keys, 1), 1)}
        del dk
    line["checked"] = ("kind, level and the counts equal to the host half's; status / leaf / pos / vloc / vlen equal to the host "
                       "half's on the first host_keys keys of every batch; no ERROR in any batch")
    out = json.dumps(line)
    print(out, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
