"""Time the batched SSTable builder (seb_dev_sst_plan, seb_dev_sst_encode) on the two shapes the engine
produces, with the `lsm` layout's entries: 16-byte keys (keygen.key16, sorted) at a 16-byte stride,
100-byte values, one deleted byte per entry (one in 16 set), 125 bytes per entry image.

  flush       one file of --flush-entries entries (default 250,000: an L0 file of keygen.LSM_LAYOUT)
  compaction  --files x --file-entries entries (default 100 x 100,000, lsm/compaction.go:253):
              1.25 GB in, 1.28 GB of data blocks out

Before any timing the first file's data section, block lengths, index block and metadata must equal the
host half (seb_sst_encode) byte for byte.  Then, with seb.Timer (no L2-flushing fence), --warmup +
--steps steps per shape, plan and encode timed separately (the plan ends in its own synchronise, the
encode is followed by one).  Yardsticks, printed with the times: the byte floor = (bytes read + bytes
written by the encode) / the 4.4 TB/s stream rate of DESIGN.md 5.7, and the host half on one thread
over the same input (every file, once).  One JSON line per shape; no pass/fail threshold.

    python tools/sst_bench.py [--out profiles/sst_bench.jsonl]
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
STREAM_TBS = 4.4  # the 16-B vector stream rate


def sorted_keys(n: int) -> np.ndarray:
    """key16 of n indices, in Go string order within the whole batch (files are consecutive slices)."""
    k = kg.key16(np.arange(n, dtype=np.int64) * 2)
    be = k.view(">u8").reshape(n, 2)
    return k[np.lexsort((be[:, 1], be[:, 0]))]


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def run_shape(torch, seb, name, files, per_file, steps, warmup, host):
    dev = torch.device("cuda", 0)
    n = files * per_file
    fb = [f * per_file for f in range(files + 1)]
    hkeys = sorted_keys(n)
    rng = np.random.default_rng(17)
    hvals = rng.integers(0, 256, n * VAL, dtype=np.uint8)
    hvoff = np.arange(n + 1, dtype=np.uint64) * VAL
    hdel = (np.arange(n) % 16 == 5).astype(np.uint8)
    keys = torch.from_numpy(hkeys.reshape(-1)).to(dev)
    dk = seb.dev_keys(keys, n=n, stride=16)
    vals = torch.from_numpy(hvals).to(dev)
    voff = torch.from_numpy(hvoff.view(np.int64)).to(dev)
    dele = torch.from_numpy(hdel).to(dev)
    ws = torch.empty(seb.dev_sst_workspace_size(n, files), dtype=torch.uint8, device=dev)
    sizes = seb.dev_sst_plan(dk, voff, fb, ws)
    blocks, d, x, m = (sum(s[j] for s in sizes) for j in range(4))
    assert not any(s[4] for s in sizes)
    data = torch.empty(d, dtype=torch.uint8, device=dev)
    index = torch.empty(x, dtype=torch.uint8, device=dev)
    meta = torch.empty(m, dtype=torch.uint8, device=dev)
    blen = torch.empty(blocks, dtype=torch.int16, device=dev)
    data.fill_(0xA5)
    seb.dev_sst_encode(dk, vals, voff, dele, fb, sizes, ws, data, index, meta, blen=blen)
    torch.cuda.synchronize()
    # bit-exact check: the first file against the host half
    h_sizes = seb.sst_plan(hkeys[:per_file], hvoff[:per_file + 1])
    h_data, h_index, h_meta = seb.sst_encode(hkeys[:per_file], hvals, hvoff[:per_file + 1], hdel[:per_file])
    assert sizes[0] == h_sizes, (sizes[0], h_sizes)
    assert data[:len(h_data)].cpu().numpy().tobytes() == h_data, "data section differs from the host half"
    assert index[:len(h_index)].cpu().numpy().tobytes() == h_index, "index block differs from the host half"
    assert meta[:len(h_meta)].cpu().numpy().tobytes() == h_meta, "metadata differs from the host half"
    lens = blen[:h_sizes[0]].cpu().numpy().view(np.uint16)
    assert (lens[:-1] == 4 + 32 * ENTRY).all() and lens[-1] == 4 + ((per_file - 1) % 32 + 1) * ENTRY
    t = [seb.Timer() for _ in range(3)]
    plan_ms, enc_ms = [], []
    for step in range(warmup + steps):
        t[0].record()
        seb.dev_sst_plan(dk, voff, fb, ws)
        t[1].record()
        seb.dev_sst_encode(dk, vals, voff, dele, fb, sizes, ws, data, index, meta, blen=blen)
        t[2].record()
        torch.cuda.synchronize()
        if step >= warmup:
            plan_ms.append(t[0].elapsed_ms(t[1]))
            enc_ms.append(t[1].elapsed_ms(t[2]))
    read = 16 * n + VAL * n + 8 * (n + 1) + n  # keys, values, value offsets, deleted bytes
    written = d + x + m + 2 * blocks
    out = {"bench": "sst_build", "shape": name, "files": files, "entries": n, "blocks": blocks, "bytes_read": read,
           "bytes_written": written, "workspace_bytes": ws.numel(), "steps": steps, "warmup": warmup,
           "plan": stats(plan_ms), "encode": stats(enc_ms),
           "floor_ms": round((read + written) / (STREAM_TBS * 1e12) * 1e3, 4)}
    out["encode_share_of_floor"] = round(out["floor_ms"] / out["encode"]["median_ms"], 4)
    out["encode_tbs"] = round((read + written) / out["encode"]["median_ms"] / 1e9, 3)
    if host:
        t0 = time.perf_counter()
        for f in range(files):
            a, b = fb[f], fb[f + 1]
            seb.sst_encode(hkeys[a:b], hvals[a * VAL:b * VAL], hvoff[:b - a + 1], hdel[a:b])
        out["host_one_thread_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flush-entries", type=int, default=250_000)
    ap.add_argument("--files", type=int, default=100)
    ap.add_argument("--file-entries", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the one-thread host yardstick")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    import seb_bloom as seb

    seb.device_check(0)
    torch.cuda.set_device(0)
    for name, files, per in (("flush", 1, a.flush_entries), ("compaction", a.files, a.file_entries)):
        line = json.dumps(run_shape(torch, seb, name, files, per, a.steps, a.warmup, not a.no_host))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
