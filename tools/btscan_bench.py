"""Time the B-tree's range scans: the leaf directory of a page-file image, and Scan of a range batch.

  tree      tools/btree_bench.py's: --keys-in-tree (10,000,000) 16-byte keys with 100-byte values, bulk-loaded; depth 4,
            1.2 GB
  dir       seb_dev_bt_dir_build (which synchronises) with a host clock around it, beside seb_dev_bt_check timed the same
            way in the same loop; the host half once
  batches   --ranges (1,000,000) ranges of --span (10) entries, and ranges / 1000 ranges of span * 1000 entries: range r
            is [key i, key i + span) for a random i; each shuffled and sorted by start: four batches
  device    per batch the plan (synchronises; host clock), the cells (seb.Timer events), the two gathers (plan + emit
            each; host clock with a synchronise behind the emit)
  host      seb_bt_scan on the first --host-ranges ranges of each batch; wall clock
  get       the sanity ratio: seb_dev_bt_get on the 2 R bounds of the batch, from this library and, with --parent-lib, from
            a second library (the parent commit's, tools/rev_lib.sh) loaded beside it, the two ALTERNATED step by step

Before any timing the device's directory must equal the host half's bytes whole, and the device's range_status,
range_off and entry arrays and both gathers' bytes the host half's on the first --host-ranges ranges of every batch.
One JSON line per run; no pass/fail threshold.

    python tools/btscan_bench.py [--keys-in-tree N] [--ranges N] [--host-ranges N] [--parent-lib PATH] [--out profiles/btscan_bench.jsonl]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "storage-engines_amd"), os.path.join(ROOT, "tools")]

from btree_bench import PAGE, build_tree, med  # noqa: E402


def note(msg):
    print(f"btscan_bench: {msg}", file=sys.stderr, flush=True)


def spread(xs):
    return [round(min(xs), 4), round(max(xs), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys-in-tree", type=int, default=10_000_000)
    ap.add_argument("--ranges", type=int, default=1_000_000)
    ap.add_argument("--span", type=int, default=10)
    ap.add_argument("--host-ranges", type=int, default=20_000, help="ranges of each batch that the host half answers")
    ap.add_argument("--fanout", type=int, default=170)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="a second libseb_bloom.so whose seb_dev_bt_get is alternated with this one's")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()

    import torch

    import seb_bloom as seb

    seb.device_check(0)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(21)
    n = a.keys_in_tree
    note(f"building a tree of {n} keys")
    image, keys, shape = build_tree(rng, n, a.fanout)
    meta = seb.bt_open(image)
    nbytes = meta.num_pages * PAGE
    d_image = torch.from_numpy(image).to(dev)
    kind = torch.empty(meta.num_pages, dtype=torch.uint8, device=dev)
    level = torch.empty(meta.num_pages, dtype=torch.uint8, device=dev)
    h_kind, h_level, h_stats = seb.bt_check(image, meta)
    t0 = time.perf_counter()
    h_dir, h_info = seb.bt_dir_build(image, meta, h_kind, h_level)
    host_dir_ms = (time.perf_counter() - t0) * 1e3
    d_dir = torch.empty(seb.bt_dir_bytes(meta.num_pages), dtype=torch.uint8, device=dev)
    ws = torch.empty(seb.dev_bt_dir_workspace_size(meta.num_pages), dtype=torch.uint8, device=dev)
    assert seb.dev_bt_check(d_image, nbytes, meta, kind, level) == h_stats
    info = seb.dev_bt_dir_build(d_image, nbytes, meta, kind, level, d_dir, ws)
    assert info == h_info and info["keys"] == n and np.array_equal(d_dir.cpu().numpy(), h_dir), "the device's directory differs"
    check_ms, dir_ms = [], []
    for step in range(a.warmup + a.steps):
        for fn, acc in ((lambda: seb.dev_bt_check(d_image, nbytes, meta, kind, level), check_ms),
                        (lambda: seb.dev_bt_dir_build(d_image, nbytes, meta, kind, level, d_dir, ws), dir_ms)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if step >= a.warmup:
                acc.append((time.perf_counter() - t0) * 1e3)
    line = {"bench": "btscan", "device": torch.cuda.get_device_name(0), "lib": os.path.relpath(seb.LIB_PATH, ROOT),
            "keys_in_tree": n, "pages": int(meta.num_pages), "image_bytes": int(nbytes), "dir": info, "dir_bytes": int(d_dir.numel()),
            "steps": a.steps, "warmup": a.warmup, "small": bool(n != 10_000_000 or a.ranges != 1_000_000),
            "dir_build_ms": med(dir_ms), "dir_build_ms_min_max": spread(dir_ms), "check_ms": med(check_ms),
            "check_ms_min_max": spread(check_ms), "host_dir_build_ms": round(host_dir_ms, 1), "batches": {}}

    parent = None
    if a.parent_lib:
        parent = C.CDLL(a.parent_lib)
        parent.seb_dev_bt_get.restype = C.c_int
        parent.seb_dev_bt_get.argtypes = seb._SIGS["seb_dev_bt_get"][1]
        line["parent_lib"] = os.path.relpath(a.parent_lib, ROOT)

    def batch(R, span, sort):
        at = rng.integers(0, n - span - 1, R)
        if sort:
            at = np.sort(at)
        return np.ascontiguousarray(keys[at]), np.ascontiguousarray(keys[at + span])

    t = [seb.Timer(), seb.Timer()]
    shapes = (("many_short", a.ranges, a.span), ("few_long", max(a.ranges // 1000, 1), a.span * 1000))
    for label, R, span in shapes:
        for sort in (False, True):
            name = f"{label}_{'sorted' if sort else 'shuffled'}"
            starts, ends = batch(R, span, sort)
            hr = min(a.host_ranges, R)
            note(f"{name}: {R} ranges of {span}; the host half on {hr} ranges, the comparison, the timing")
            t0 = time.perf_counter()
            want = seb.bt_scan(image, meta, h_dir, starts[:hr], ends[:hr])
            host_ms = (time.perf_counter() - t0) * 1e3
            ks = seb.dev_keys(torch.from_numpy(starts.reshape(-1)).to(dev), n=R, stride=16)
            ke = seb.dev_keys(torch.from_numpy(ends.reshape(-1)).to(dev), n=R, stride=16)
            both = seb.dev_keys(torch.from_numpy(np.concatenate([starts, ends]).reshape(-1)).to(dev), n=2 * R, stride=16)
            rs = torch.empty(R, dtype=torch.uint8, device=dev)
            sws = torch.empty(seb.dev_bt_scan_workspace_size(R), dtype=torch.uint8, device=dev)
            sz = seb.dev_bt_scan_plan(d_image, nbytes, meta, d_dir, ks, ke, 0, rs, sws)
            E = sz.entries
            assert E == R * span
            ro = torch.empty(R + 1, dtype=torch.int64, device=dev)
            st, so = torch.empty(E, dtype=torch.uint8, device=dev), torch.empty(E, dtype=torch.uint8, device=dev)
            kl, vl = torch.empty(E, dtype=torch.int64, device=dev), torch.empty(E, dtype=torch.int64, device=dev)
            kn, vn = torch.empty(E, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.int32, device=dev)
            gws = torch.empty(seb.dev_get_values_workspace_size(E), dtype=torch.uint8, device=dev)
            off = torch.empty(E + 1, dtype=torch.int64, device=dev)
            dense = {"key": torch.empty(E * 16, dtype=torch.uint8, device=dev), "val": torch.empty(E * 100, dtype=torch.uint8, device=dev)}
            g_status = torch.empty(2 * R, dtype=torch.uint8, device=dev)
            g_vloc = torch.empty(2 * R, dtype=torch.int64, device=dev)
            g_vlen = torch.empty(2 * R, dtype=torch.int32, device=dev)
            ms = {k: [] for k in ("plan", "cells", "gather_keys", "gather_vals", "get_2r", "get_2r_parent")}

            def gather(loc, length, out):
                gsz = seb.dev_get_values_plan(st, so, None, loc, length, E, [], d_image, gws, pool_bytes=nbytes)
                seb.dev_get_values_emit(st, so, None, loc, length, E, [], d_image, gsz, gws, off, out, pool_bytes=nbytes)
                torch.cuda.synchronize()
                return gsz.val_bytes

            def wall(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                return (time.perf_counter() - t0) * 1e3

            for step in range(a.warmup + a.steps):
                got = {"plan": wall(lambda: seb.dev_bt_scan_plan(d_image, nbytes, meta, d_dir, ks, ke, 0, rs, sws))}
                t[0].record()
                seb.dev_bt_scan_cells(d_image, nbytes, meta, d_dir, sz, sws, ro, st, so, kl, kn, vl, vn)
                t[1].record()
                torch.cuda.synchronize()
                got["cells"] = t[0].elapsed_ms(t[1])
                got["gather_keys"] = wall(lambda: gather(kl, kn, dense["key"]))
                if step == 0:
                    hE = int(want["range_off"][hr])
                    assert np.array_equal(off[: hE + 1].cpu().numpy().view(np.uint64), want["key_off"]), f"{name}: key_off"
                    assert np.array_equal(dense["key"][: int(want["key_off"][hE])].cpu().numpy(), want["keys"]), f"{name}: keys"
                got["gather_vals"] = wall(lambda: gather(vl, vn, dense["val"]))
                if step == 0:
                    assert np.array_equal(off[: hE + 1].cpu().numpy().view(np.uint64), want["val_off"]), f"{name}: val_off"
                    assert np.array_equal(dense["val"][: int(want["val_off"][hE])].cpu().numpy(), want["vals"]), f"{name}: vals"
                    assert np.array_equal(rs[:hr].cpu().numpy(), want["range_status"]) and not bool(rs.any())
                    assert np.array_equal(ro[: hr + 1].cpu().numpy().view(np.uint64), want["range_off"])
                    for label2, d, w in (("status", st, "status"), ("source", so, "source"), ("kloc", kl, "kloc"), ("klen", kn, "klen"),
                                         ("vloc", vl, "vloc"), ("vlen", vn, "vlen")):
                        assert np.array_equal(d[:hE].cpu().numpy().view(want[w].dtype), want[w]), f"{name}: {label2} differs from the host half's"
                for which, fn in (("get_2r", lambda: seb.lib().seb_dev_bt_get), ("get_2r_parent", lambda: parent.seb_dev_bt_get if parent else None)):
                    f = fn()
                    if f is None:
                        continue
                    t[0].record()
                    rc = f(d_image.data_ptr(), nbytes, C.byref(meta), C.byref(both), g_status.data_ptr(), None, None, g_vloc.data_ptr(),
                           g_vlen.data_ptr(), None, None)
                    t[1].record()
                    torch.cuda.synchronize()
                    assert rc == 0
                    got[which] = t[0].elapsed_ms(t[1])
                if step >= a.warmup:
                    for k, v in got.items():
                        ms[k].append(v)
            row = {"ranges": R, "span": span, "entries": int(E), "host_ranges": hr, "host_ms": round(host_ms, 1),
                   "host_ms_per_batch": round(host_ms * R / hr, 1)}
            for k, v in ms.items():
                if v:
                    row[k + "_ms"], row[k + "_ms_min_max"] = med(v), spread(v)
            row["scan_total_ms"] = round(sum(row[k + "_ms"] for k in ("plan", "cells", "gather_keys", "gather_vals")), 4)
            row["plan_over_get_2r"] = round(row["plan_ms"] / row["get_2r_ms"], 2)
            line["batches"][name] = row
            del ks, ke, both
    line["checked"] = ("the directory's bytes equal to the host half's, whole; range_status, range_off, the six entry arrays and both "
                       "gathers' offsets and bytes equal to the host half's on the first host_ranges ranges of every batch")
    out = json.dumps(line)
    print(out, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
