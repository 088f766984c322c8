"""Time the hash index's read side: recover() of four segment images and Get of a key batch.

  store   --records (10,000,000) records of 16-byte keys and 100-byte values (136 bytes each, 1.36 GB) in 4 segments,
          at 1 and at 4 records per key (the keys drawn at random, so a key's records are spread over the segments);
          no record is corrupt
  batch   --keys (10,000,000) 16-byte keys, half of them present, shuffled
  device  recover = seb_dev_seg_verify + seb_dev_hidx_clear + seb_dev_hidx_insert on a table of capacity = records
          (what a caller knows before it has counted keys), and without verify: clear + insert alone;
          Get = seb_dev_hidx_get with verify on and off.  seb.Timer events around the calls.
  host    the same answers from the host half: seb_seg_verify + seb_hidx_lookup (which builds its map inside the
          call) on the host images, and the copy of status / vloc / vlen to the device that a caller who goes on to
          seb_dev_get_values needs.  Wall clock.

Before any timing the device's ok / valid / live, its key count and its (status, rec, vloc, vlen) must equal the
host half's for the whole batch, with verify on.

Model, written before the first run (DESIGN.md 5.7's terms: streams / 4.4 TB/s + gathers / 249 G/s):
  Get     streams: 16 bytes of key in and 22 bytes out per key (status 1, rec 8, vloc 8, vlen 4, source 1): 380 MB,
          0.086 ms.  Gathers: one slot per key (at a load of 0.3 a probe rarely goes on to a second slot), and for a
          present key its record's header and then its key, two dependent gathers; 20M for this batch, 0.080 ms at
          the ceiling.  That ceiling was measured on an L2-resident table; this one is 256 MiB of slots and the records
          lie in 1.36 GB, so every gather is an HBM sector read and the chain is two deep: expect a multiple of the
          sum, 0.17 ms, not the sum.  With verify each present key's 136 bytes are read as well: 5M x 3 cache lines
          of 128 bytes = 1.9 GB at line granularity, 0.44 ms at the stream rate if every line were used whole.
  Insert  streams: 8 bytes of rec_off and one of live per record, 0.02 ms.  Per record a gather of header and key
          (36 bytes of a 136-byte record, so in effect the whole pool's lines: 1.36 GB, 0.31 ms), an atomic load of
          the slot, and a compare-and-swap (a new key) or an atomic load + key gather + atomicMax (a key seen
          before).  The only atomic figure the project has is 5.4 G cells/s through the block-id plan (DESIGN.md
          5.17), one workload's; it is quoted as that and no target is fixed from it: at that rate 10M records would
          take 1.9 ms.
  Verify  the pool once, staged through LDS: 1.36 GB, 0.31 ms at the stream rate; the table CRC is a dependent chain
          of four LDS lookups per 4 bytes per lane, which k_wal_crc showed to be the limit, not HBM.
One JSON line per shape; no pass/fail threshold.

    python tools/hashindex_bench.py [--records N] [--keys N] [--per-key 1,4] [--out profiles/hashindex_bench.jsonl]
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

STREAM_BYTES_PER_S = 4.4e12
GATHER_PER_S = 249e9
REC = 136                     # 20 + 16 + 100
SEGMENTS = 4


def note(msg):
    print(f"hashindex_bench: {msg}", file=sys.stderr, flush=True)


def med(xs):
    return round(float(np.median(xs)), 4)


def make_store(torch, seb, rng, records, per_key):
    """The pool on the host and on the device.  The records are laid out by numpy; their CRC fields are filled by
    SEB_WAL_SEAL, which stores ChecksumIEEE(record[4:]) for any record extent (the comparison with the host half,
    whose CRC is separate code, checks them)."""
    nkeys = records // per_key
    ids = rng.permutation(records) % nkeys if per_key > 1 else rng.permutation(records)
    pool = np.zeros((records, REC), np.uint8)
    pool[:, 4:12] = (1_700_000_000 + np.arange(records, dtype=np.uint64)).view(np.uint8).reshape(records, 8)
    pool[:, 12:16] = np.frombuffer(np.uint32(16).tobytes(), np.uint8)
    pool[:, 16:20] = np.frombuffer(np.uint32(100).tobytes(), np.uint8)
    pool[:, 20:36] = kg.key16(ids)
    pool[:, 36:] = rng.integers(0, 256, (records, 100), dtype=np.uint8)
    d_pool = torch.from_numpy(pool.reshape(-1)).cuda()
    rec_off = np.arange(records + 1, dtype=np.uint64) * REC
    d_off = torch.from_numpy(rec_off.view(np.int64)).cuda()
    seb.dev_wal_crc(d_pool, d_off, seb.WAL_SEAL)
    torch.cuda.synchronize()
    pool = d_pool.cpu().numpy()
    first = np.array([records * s // SEGMENTS for s in range(SEGMENTS + 1)], np.uint64)
    base = first[:-1] * np.uint64(REC)
    size = np.diff(first) * np.uint64(REC)
    return pool, d_pool, rec_off[:-1].copy(), d_off[:-1], first, base, size, ids, nkeys


def run_shape(torch, seb, records, nprobe, per_key, steps, warmup, host_steps):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(19 + per_key)
    note(f"{per_key} per key: building {records} records")
    pool, d_pool, rec_off, d_off, first, base, size, ids, nkeys = make_store(torch, seb, rng, records, per_key)
    P = pool.size
    d_first = torch.from_numpy(first.view(np.int64)).to(dev)
    present = ids[rng.integers(0, records, nprobe // 2)]
    probe = kg.key16(np.concatenate([present, np.arange(5 * 10**9, 5 * 10**9 + nprobe - present.size)])[rng.permutation(nprobe)])
    d_probe = torch.from_numpy(probe.reshape(-1)).to(dev)
    dk = seb.dev_keys(d_probe, n=nprobe, stride=16)
    capacity = records
    table = torch.empty(seb.dev_hidx_table_bytes(capacity), dtype=torch.uint8, device=dev)
    ok = torch.empty(records, dtype=torch.uint8, device=dev)
    live = torch.empty(records, dtype=torch.uint8, device=dev)
    valid = torch.empty(SEGMENTS, dtype=torch.int64, device=dev)
    status = torch.empty(nprobe, dtype=torch.uint8, device=dev)
    source = torch.empty(nprobe, dtype=torch.uint8, device=dev)
    rec = torch.empty(nprobe, dtype=torch.int64, device=dev)
    vloc = torch.empty(nprobe, dtype=torch.int64, device=dev)
    vlen = torch.empty(nprobe, dtype=torch.int32, device=dev)
    t = [seb.Timer() for _ in range(4)]

    def recover_round(verify):
        t[0].record()
        if verify:
            seb.dev_seg_verify(d_pool, P, d_off, records, d_first, SEGMENTS, ok, valid, live)
        t[1].record()
        seb.dev_hidx_clear(table, capacity)
        t[2].record()
        seb.dev_hidx_insert(table, capacity, d_pool, P, d_off, live if verify else None, records)
        t[3].record()
        return seb.dev_hidx_count(table, capacity)

    def get_round(verify):
        t[0].record()
        seb.dev_hidx_get(table, capacity, d_pool, P, dk, verify, status, rec, vloc, vlen, source)
        t[1].record()
        torch.cuda.synchronize()

    def host_round(verify):
        t0 = time.perf_counter()
        h_ok, h_valid, h_after, h_live = seb.seg_verify(pool, rec_off, first, base, size) if verify else (None,) * 4
        t1 = time.perf_counter()
        st, rc, vl, vn, distinct = seb.hidx_lookup(pool, rec_off, h_live, probe, verify)
        t2 = time.perf_counter()
        back = [torch.from_numpy(a.view(s)).to(dev) for a, s in ((st, np.uint8), (vl, np.int64), (vn, np.int32))]
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        del back
        return (h_ok, h_valid, h_live, st, rc, vl, vn, distinct), dict(seg_verify=t1 - t0, lookup=t2 - t1, h2d=t3 - t2)

    note(f"{per_key} per key: the host half (verify on), then the comparison")
    want, host_on = host_round(True)
    distinct, bad = recover_round(True)
    get_round(True)
    assert (distinct, bad) == (want[7], 0) and distinct == nkeys, (distinct, bad, want[7], nkeys)
    for name, d, w in (("ok", ok, want[0]), ("valid", valid, want[1]), ("live", live, want[2]), ("status", status, want[3]),
                       ("rec", rec, want[4]), ("vloc", vloc, want[5]), ("vlen", vlen, want[6])):
        assert np.array_equal(d.cpu().numpy().view(w.dtype), w), f"{name} differs from the host half's"
    found = int((want[3] == seb.GET_FOUND).sum())
    del want
    note(f"{per_key} per key: equal ({distinct} keys, {found} found); timing")
    host = {True: [host_on], False: []}
    for v in (True, False):
        while len(host[v]) < host_steps:
            host[v].append(host_round(v)[1])
    line = {"bench": "hashindex", "records": records, "per_key": per_key, "distinct": distinct, "segments": SEGMENTS,
            "pool_bytes": int(P), "keys": nprobe, "found": found, "capacity": capacity,
            "table_slots": (int(table.numel()) - 64) // 8, "steps": steps, "warmup": warmup, "host_steps": host_steps,
            "small": bool(records != 10_000_000 or nprobe != 10_000_000)}
    for v in (True, False):
        tag = "verify" if v else "noverify"
        ver, clr, ins, get = [], [], [], []
        for step in range(warmup + steps):
            recover_round(v)
            if step >= warmup:
                ver.append(t[0].elapsed_ms(t[1])), clr.append(t[1].elapsed_ms(t[2])), ins.append(t[2].elapsed_ms(t[3]))
        recover_round(True)  # the table the Gets read holds the verified records either way
        for step in range(warmup + steps):
            get_round(v)
            if step >= warmup:
                get.append(t[0].elapsed_ms(t[1]))
        hm = {k: round(float(np.median([h[k] for h in host[v]])) * 1e3, 1) for k in host[v][0]}
        line[tag] = {"seg_verify_ms": med(ver) if v else 0.0, "clear_ms": med(clr), "insert_ms": med(ins),
                     "recover_ms": round((med(ver) if v else 0.0) + med(clr) + med(ins), 4),
                     "insert_ms_min_max": [round(min(ins), 4), round(max(ins), 4)],
                     "get_ms": med(get), "get_ms_min_max": [round(min(get), 4), round(max(get), 4)],
                     "insert_records_per_s_g": round(records / (med(ins) * 1e-3) / 1e9, 3),
                     "get_keys_per_s_g": round(nprobe / (med(get) * 1e-3) / 1e9, 3),
                     "host_ms": hm, "host_total_ms": round(sum(hm.values()), 1)}
        line[tag]["host_over_device"] = round(line[tag]["host_total_ms"] / (line[tag]["recover_ms"] + line[tag]["get_ms"]), 1)
    line["model_ms"] = {"get_streams": round(38 * nprobe / STREAM_BYTES_PER_S * 1e3, 4),
                        "get_gathers": round((nprobe + 2 * found) / GATHER_PER_S * 1e3, 4),
                        "pool_stream": round(P / STREAM_BYTES_PER_S * 1e3, 4),
                        "insert_at_5.4_g_cells_per_s_for_comparison_only": round(records / 5.4e9 * 1e3, 3)}
    line["checked"] = "ok, valid, live, the key count and status / rec / vloc / vlen equal to the host half's for the whole batch"
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--keys", type=int, default=10_000_000)
    ap.add_argument("--per-key", default="1,4")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=1)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    import seb_bloom as seb

    seb.device_check(0)
    torch.cuda.set_device(0)
    for per_key in (int(x) for x in a.per_key.split(",")):
        line = json.dumps(run_shape(torch, seb, a.records, a.keys, per_key, a.steps, a.warmup, a.host_steps))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
