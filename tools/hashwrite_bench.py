"""Time the hash index's write side: framing a Put / Delete batch, compacting the oldest half of a
store, the table rebuild behind it, and the logical size.

  store   --records (10,000,000) records of 16-byte keys and 100-byte values in 4 segments, 4 records per key (the keys
          drawn at random, so a key's records are spread over the segments), 5% of the records deletes.  The pool is
          the device frame of the whole op list; every record must then pass seb_dev_seg_verify.
  frame   the first --batch (1,000,000) ops: seb_dev_seg_frame_plan (with its one synchronisation) and _emit (the
          records and the seal), rotation at 64 MiB
  compact the oldest 2 of the 4 segments: seb_dev_seg_compact_plan (scratch table, marks, scan, one synchronisation)
          and _emit (offsets, the copy by output bytes, the seal)
  rebuild what seb_hidx_compact does behind the emit, timed on its own: the copy of the segments that stay, the
          shift of their offsets (a torch add here), seb_dev_hidx_clear and the two inserts
  logical seb_dev_hidx_logical_size over the rebuilt table (with its synchronisation)
  host    the host half once each, by wall clock: seb_seg_frame, seb_seg_compact, seb_hidx_logical_size

Before any timing the device's image, offsets, cuts, every size counter and the logical size must equal the host
half's.  3 warm-up and 10 timed rounds, medians of seb.Timer events.

Model, written before the first run (DESIGN.md 5.7's terms: streams / 4.4 TB/s + gathers / 249 G/s; 5.19's measured
10 G records/s insert, 22 G keys/s Get without verify and 0.63 ms per 1.36 GB of segment CRC):
  frame   plan: 17 bytes of offsets and flags per op and 8 written, 25 MB, 0.006 ms; four launches and one
          synchronisation, so tens of microseconds of latency decide it.  emit: 116 MB in, 131 MB out, 0.056 ms as
          streams; but every 16-byte chunk bisects rec_off (8 MB, L2-resident) in 20 dependent steps: 8.2M chunks x
          20 = 164M gathers, 0.66 ms at the ceiling.  The seal: 131 MB at the measured CRC rate, 0.06 ms.  Expect
          0.7-0.8 ms, bound by the bisection, not by HBM.
  compact 5M records over 2.5M keys; 2.34M distinct in the older half, about 2.2M survivors, a 300 MB image.
          plan: clearing 128 MiB of slots 0.03 ms, the insert 0.5 ms at the measured rate, the mark is a Get without
          verify per record plus 12 bytes written: 5M / 22 G/s = 0.23 ms; expect 0.8-0.9 ms.  emit: 300 MB out and
          (survivors are 44% of the records, so at line granularity) most of the 680 MB in: 1 GB, 0.22 ms; the
          bisection of out_rec_off (18 MB) is 19M chunks x 22 steps = 410M gathers, 1.65 ms; the seal 0.14 ms.
          Expect about 2 ms, again the bisection.
  rebuild the copy of 680 MB (1.36 GB of traffic) 0.31 ms, clearing 256 MiB 0.06 ms, 7.2M records inserted 0.75 ms:
          about 1.1 ms.
  logical 256 MiB of slots streamed, 0.06 ms, and 2.5M header gathers, 0.01 ms at the ceiling: 0.1 ms with the
          synchronisation.
  host    frame: 131 MB through a byte-wise CRC and memcpy, 0.2-0.3 s.  compact: a std::unordered_map over 5M
          records, 2-3 s (5.19 measured 6.6 s for 10M inserts and 10M lookups).
One JSON line; no pass/fail threshold.

    python tools/hashwrite_bench.py [--records N] [--batch N] [--out profiles/hashwrite_bench.jsonl]
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

SEGMENTS, PER_KEY, VALUE, LIMIT = 4, 4, 100, 64 << 20
TS0, TS1 = 1_700_000_000, 1_800_000_000


def note(msg):
    print(f"hashwrite_bench: {msg}", file=sys.stderr, flush=True)


def med(xs):
    return round(float(np.median(xs)), 4)


def timed(seb, torch, fns, steps, warmup):
    """Medians of the spans between consecutive fns, each round synchronised at its end."""
    t = [seb.Timer() for _ in range(len(fns) + 1)]
    spans = [[] for _ in fns]
    for step in range(warmup + steps):
        t[0].record()
        for i, fn in enumerate(fns):
            fn()
            t[i + 1].record()
        torch.cuda.synchronize()
        if step >= warmup:
            for i in range(len(fns)):
                spans[i].append(t[i].elapsed_ms(t[i + 1]))
    return [med(s) for s in spans], [[round(min(s), 4), round(max(s), 4)] for s in spans]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()

    import torch

    import seb_bloom as seb

    seb.device_check(0)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(23)
    n, nb = a.records, min(a.batch, a.records)
    note(f"building {n} ops")
    keys = kg.key16(rng.permutation(n) % (n // PER_KEY))
    deleted = (rng.random(n) < 0.05).astype(np.uint8)
    val_off = np.arange(n + 1, dtype=np.uint64) * VALUE
    d_keys = torch.from_numpy(keys.reshape(-1)).to(dev)
    d_vals = torch.randint(0, 256, (n * VALUE,), dtype=torch.uint8, device=dev)
    d_voff = torch.from_numpy(val_off.view(np.int64)).to(dev)
    d_del = torch.from_numpy(deleted).to(dev)
    dk = seb.dev_keys(d_keys, n=n, stride=16)
    d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    P, _ = seb.dev_seg_frame_plan(dk, d_voff, d_del, d_off, 0, seb.SEG_NO_LIMIT)
    d_pool = torch.empty(P, dtype=torch.uint8, device=dev)
    seb.dev_seg_frame_emit(dk, d_vals, d_voff, d_del, TS0, d_off, d_pool, P)
    first = np.array([n * s // SEGMENTS for s in range(SEGMENTS + 1)], np.int64)
    d_first = torch.from_numpy(first).to(dev)
    ok = torch.empty(n, dtype=torch.uint8, device=dev)
    valid = torch.empty(SEGMENTS, dtype=torch.int64, device=dev)
    seb.dev_seg_verify(d_pool, P, d_off, n, d_first, SEGMENTS, ok, valid, None)
    assert valid.cpu().numpy().tolist() == np.diff(first).tolist(), "a framed record fails the segment verify"
    rec_off = d_off.cpu().numpy().view(np.uint64)
    pool = d_pool.cpu().numpy()
    del ok

    # ---- frame
    note(f"frame of {nb} ops: the host half, then the comparison")
    vals_b = d_vals[: nb * VALUE].cpu().numpy()
    t0 = time.perf_counter()
    h_image, h_off, h_cuts = seb.seg_frame(keys[:nb], vals_b, val_off[: nb + 1], deleted[:nb], TS1, 0, LIMIT)
    host_frame = time.perf_counter() - t0
    dkb = seb.dev_keys(d_keys, n=nb, stride=16)
    b_off = torch.empty(nb + 1, dtype=torch.int64, device=dev)
    total, cuts = seb.dev_seg_frame_plan(dkb, d_voff, d_del, b_off, 0, LIMIT)
    b_image = torch.empty(total, dtype=torch.uint8, device=dev)
    seb.dev_seg_frame_emit(dkb, d_vals, d_voff, d_del, TS1, b_off, b_image, total)
    assert total == h_image.size and cuts.tolist() == h_cuts.tolist(), "frame: sizes or cuts differ from the host half's"
    assert np.array_equal(b_off.cpu().numpy().view(np.uint64), h_off), "frame: rec_off differs from the host half's"
    assert np.array_equal(b_image.cpu().numpy(), h_image), "frame: the image differs from the host half's"
    frame_ms, frame_mm = timed(seb, torch, [lambda: seb.dev_seg_frame_plan(dkb, d_voff, d_del, b_off, 0, LIMIT),
                                            lambda: seb.dev_seg_frame_emit(dkb, d_vals, d_voff, d_del, TS1, b_off, b_image, total)],
                               a.steps, a.warmup)
    del h_image, b_image, vals_b

    # ---- compaction of the oldest two segments
    c = SEGMENTS // 2
    n_c, edge = int(first[c]), int(rec_off[first[c]])
    note(f"compaction of {n_c} records: the host half, then the comparison")
    t0 = time.perf_counter()
    h_image, h_out, h_sizes = seb.seg_compact(pool[:edge], rec_off[:n_c], None, TS1)
    host_compact = time.perf_counter() - t0
    ws = torch.empty(seb.dev_seg_compact_workspace_size(n_c), dtype=torch.uint8, device=dev)
    sz = seb.dev_seg_compact_plan(d_pool, P, d_off, None, n_c, ws)
    assert sz.as_dict() == h_sizes, ("compaction: the sizes differ from the host half's", sz.as_dict(), h_sizes)
    rest = P - edge
    new_pool = torch.empty(sz.image_bytes + rest, dtype=torch.uint8, device=dev)
    new_off = torch.empty(sz.survivors + (n - n_c) + 1, dtype=torch.int64, device=dev)
    seb.dev_seg_compact_emit(d_pool, P, d_off, n_c, TS1, sz, ws, new_pool, new_off)
    assert np.array_equal(new_off[: sz.survivors + 1].cpu().numpy().view(np.uint64), h_out), "compaction: out_rec_off differs"
    assert np.array_equal(new_pool[: sz.image_bytes].cpu().numpy(), h_image), "compaction: the image differs from the host half's"
    compact_ms, compact_mm = timed(seb, torch, [lambda: seb.dev_seg_compact_plan(d_pool, P, d_off, None, n_c, ws),
                                                lambda: seb.dev_seg_compact_emit(d_pool, P, d_off, n_c, TS1, sz, ws, new_pool, new_off)],
                                   a.steps, a.warmup)

    # ---- the rebuild, then the logical size
    capacity = n
    table = torch.empty(seb.dev_hidx_table_bytes(capacity), dtype=torch.uint8, device=dev)
    total_new = sz.image_bytes + rest
    tail = new_off[sz.survivors: sz.survivors + (n - n_c)]

    def copy_rest():
        new_pool[sz.image_bytes:] = d_pool[edge:]
        torch.add(d_off[n_c:n], sz.image_bytes - edge, out=tail)

    def inserts():
        seb.dev_hidx_insert(table, capacity, new_pool, total_new, new_off, None, sz.survivors)
        seb.dev_hidx_insert(table, capacity, new_pool, total_new, tail, None, n - n_c)

    copy_rest(), seb.dev_hidx_clear(table, capacity), inserts()
    distinct, bad = seb.dev_hidx_count(table, capacity)
    note("the logical size on the host")
    after = np.concatenate([h_image, pool[edge:]])
    after_off = np.concatenate([h_out[:-1], rec_off[n_c:n] - np.uint64(edge) + np.uint64(sz.image_bytes)])
    t0 = time.perf_counter()
    h_logical = seb.hidx_logical_size(after, after_off)
    host_logical = time.perf_counter() - t0
    got_logical = seb.dev_hidx_logical_size(table, capacity, new_pool, total_new)
    assert bad == 0 and got_logical == h_logical, ("the logical size differs from the host half's", got_logical, h_logical, bad)
    assert np.array_equal(new_pool.cpu().numpy(), after), "the rebuilt pool differs from the host's"
    rebuild_ms, rebuild_mm = timed(seb, torch, [copy_rest, lambda: seb.dev_hidx_clear(table, capacity), inserts], a.steps, a.warmup)
    logical_ms, logical_mm = timed(seb, torch, [lambda: seb.dev_hidx_logical_size(table, capacity, new_pool, total_new)], a.steps,
                                   a.warmup)

    line = {"bench": "hashwrite", "records": n, "per_key": PER_KEY, "segments": SEGMENTS, "pool_bytes": int(P), "deletes": int(deleted.sum()),
            "steps": a.steps, "warmup": a.warmup, "small": bool(n != 10_000_000 or nb != 1_000_000),
            "frame": {"ops": nb, "image_bytes": int(total), "cuts": int(cuts.size), "plan_ms": frame_ms[0], "emit_ms": frame_ms[1],
                      "min_max": frame_mm, "ops_per_s_g": round(nb / ((frame_ms[0] + frame_ms[1]) * 1e-3) / 1e9, 3),
                      "host_ms": round(host_frame * 1e3, 1)},
            "compact": {**h_sizes, "plan_ms": compact_ms[0], "emit_ms": compact_ms[1], "min_max": compact_mm,
                        "emit_out_gb_per_s": round(sz.image_bytes / (compact_ms[1] * 1e-3) / 1e9, 1),
                        "host_ms": round(host_compact * 1e3, 1)},
            "rebuild": {"records": sz.survivors + n - n_c, "distinct": distinct, "capacity": capacity, "copy_and_shift_ms": rebuild_ms[0],
                        "clear_ms": rebuild_ms[1], "insert_ms": rebuild_ms[2], "total_ms": round(sum(rebuild_ms), 4), "min_max": rebuild_mm},
            "logical_size": {"value": int(got_logical), "ms": logical_ms[0], "min_max": logical_mm[0], "host_ms": round(host_logical * 1e3, 1)},
            "checked": "the frame's image, rec_off and cuts, the compaction's sizes, offsets and image, the rebuilt pool and the "
                       "logical size equal to the host half's"}
    out = json.dumps(line)
    print(out, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
