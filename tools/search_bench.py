"""Time the batched data-block search (seb_dev_search_blocks, seb_dev_resolve_rows) behind a MultiGet
and the block locator, on keygen.lsm_files' 28-file `lsm` layout.

Every file is laid out as SSTableBuilder would write it for 16-byte keys and 100-byte values: 32
entries of 125 bytes per 4 KiB block (4,004 bytes used, zero padded), the index entry of a block its
first key: the index §5.9 assumed.  The block pool holds EVERY block of the 28 files (531,252 blocks,
2.18 GB of HBM), so a cell's block id is its file's first id + offset / 4096 and no host dedup pass is
in the timed chain; the batch is the first --keys (default 2M) probes of keygen.lsm_probe_indices, half
of them present.  Values are a byte pattern; the walk never reads them.

Before timing, the cells of the first --sample keys (default 100K) must equal the host walk
(seb_block_search on the block bytes copied back).  Then, with seb.Timer (no L2-flushing fence),
--warmup + --steps steps each:
  search alone, twice (the spread of two runs of one form is the bar a difference between forms has
    to clear); with --forms, under block_search_algo 1, 2, 1, 2: that option exists only in a library
    built with tools/diag/search_wave_lds.patch (the wave-cooperative form, measured slower and
    removed; profiles/search_bench_two_forms.jsonl),
  resolve alone,
  the whole chain (multiget_list_dev, locate_dev, the id arithmetic, search, resolve),
  search alone again on a second batch whose keys come from a span of 8,192 keys, so that all its
    cells share ~550 blocks (2.2 MB, L2 resident): the walk without the block bytes' HBM traffic.
Prints one JSON line with the times, the counts the model needs (live cells, entries walked, bytes of
block needed in 128-byte lines and in 1 KiB steps) and the floor they give at the §5.7 stream rate.
No pass/fail threshold.

    python tools/search_bench.py [--out profiles/search_bench.jsonl]
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

EPB = 32            # entries per block
ENTRY = 9 + 16 + 100
STREAM_TBS = 4.4    # the 16-B vector stream rate


def file_blocks(torch, idx: np.ndarray, dev):
    """(pool rows [blocks, 4096] u8 on the device, encoded index block) of a file holding key16(2 * idx)."""
    n = len(idx)
    nblk = -(-n // EPB)
    keys = np.zeros((nblk * EPB, 16), np.uint8)
    keys[:n] = kg.key16(2 * idx)
    ent = torch.zeros((nblk, EPB, ENTRY), dtype=torch.uint8, device=dev)
    ent[:, :, 0] = 16
    ent[:, :, 4] = 100
    ent[:, :, 9:25] = torch.from_numpy(keys).to(dev).view(nblk, EPB, 16)
    ent[:, :, 25:] = (torch.arange(100, device=dev) % 251).to(torch.uint8)
    rows = torch.zeros((nblk, 4096), dtype=torch.uint8, device=dev)
    rows[:, 4:4 + EPB * ENTRY] = ent.view(nblk, EPB * ENTRY)
    rows[:, 0] = EPB
    if n % EPB:  # the last block holds the remainder; the slots after it are padding
        rows[-1, 0] = n % EPB
        rows[-1, 4 + (n % EPB) * ENTRY:] = 0
    first = 2 * idx[::EPB]
    e = np.zeros(len(first), dtype=np.dtype([("ks", "<u4"), ("bo", "<u8"), ("key", "u1", 16)]))
    e["ks"], e["bo"], e["key"] = 16, 4096 * np.arange(len(first), dtype=np.uint64), kg.key16(first)
    return rows, np.uint32(len(first)).tobytes() + e.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=2_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--sample", type=int, default=100_000, help="keys whose cells are checked against the host walk")
    ap.add_argument("--forms", action="store_true", help="time block_search_algo 1 and 2 (a library with the diag patch)")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()

    import torch

    import seb_bloom as seb

    seb.device_check(0)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lay = kg.LSM_LAYOUT
    files = kg.lsm_files(lay)
    reg = seb.Registry(0)
    pools, base_of_slot, at = [], np.zeros(65536, np.int64), 0
    for level, file_num, idx in files:
        m, k = seb.params(len(idx), 0.01)
        keys = torch.from_numpy(kg.key16(2 * idx)).to(dev)
        w = seb.new_words(m, device=dev)
        seb.dev_build(seb.dev_keys(keys, n=len(idx), stride=16), w, m, k)
        block = m.to_bytes(8, "little") + k.to_bytes(4, "little") + seb.words_to_bits(w, m).tobytes()
        slot = reg.put(file_num, level, block, kg.key16_bytes(int(2 * idx[0])), kg.key16_bytes(int(2 * idx[-1])))
        rows, iblock = file_blocks(torch, idx, dev)
        reg.put_index(file_num, iblock)
        pools.append(rows)
        base_of_slot[slot] = at
        at += rows.shape[0]
    pool = torch.cat(pools).view(-1)
    del pools
    nblocks = at
    assert pool.data_ptr() % 16 == 0 and pool.numel() == nblocks * 4096
    blen = torch.full((nblocks,), 4096, dtype=torch.int16, device=dev)
    base_dev = torch.from_numpy(base_of_slot).to(dev)
    cap = reg.max_candidates()

    def batch(pidx):
        """The device arrays of a probe batch: keys, candidate rows, block offsets, block ids."""
        n = len(pidx)
        pk = seb.dev_keys(torch.from_numpy(kg.key16(pidx)).to(dev), n=n, stride=16)
        rows = torch.zeros(n * cap, dtype=torch.int16, device=dev)
        blocks = torch.zeros(n * cap, dtype=torch.int64, device=dev)
        bid = torch.zeros(n * cap, dtype=torch.int32, device=dev)
        return dict(n=n, pk=pk, rows=rows, blocks=blocks, bid=bid, cells=torch.zeros(n * cap, dtype=torch.int32, device=dev),
                    status=torch.zeros(n, dtype=torch.uint8, device=dev), col=torch.zeros(n, dtype=torch.int16, device=dev),
                    vloc=torch.zeros(n, dtype=torch.int64, device=dev), vlen=torch.zeros(n, dtype=torch.int32, device=dev))

    def plan(B):
        reg.multiget_list_dev(B["pk"], B["rows"], cap)
        reg.locate_dev(B["pk"], B["rows"], B["blocks"], cap)
        # id = the file's first block + offset / 4096; -1 (SEB_NO_BLOCK_ID) where there is no read
        live = B["blocks"] >= 0  # SEB_NO_BLOCK is -1 as an int64
        ids = base_dev[B["rows"].to(torch.int64) & 0xFFFF] + (B["blocks"] >> 12)
        B["bid"].copy_(torch.where(live, ids, torch.full_like(ids, -1)).to(torch.int32))

    def search(B):
        seb.dev_search_blocks(B["pk"], B["bid"], cap, pool, blen, B["cells"], num_blocks=nblocks)

    def resolve(B):
        seb.dev_resolve_rows(B["cells"], B["bid"], B["n"], cap, B["status"], B["col"], B["vloc"], B["vlen"])

    def chain(B):
        plan(B)
        search(B)
        resolve(B)

    pidx = kg.lsm_probe_indices(lay)[: a.keys]
    A = batch(pidx)
    chain(A)
    torch.cuda.synchronize()

    # the answers of the first keys against the host walk, under both forms; and the work of the call
    s = min(a.sample, A["n"])
    bid_h = A["bid"][: s * cap].cpu().numpy().view(np.uint32)
    live_s = np.nonzero(bid_h != 0xFFFFFFFF)[0]
    blocks_h = pool.view(-1, 4096)[torch.from_numpy(bid_h[live_s].astype(np.int64)).to(dev)].cpu().numpy()
    keys_h = kg.key16(pidx[:s])
    want = np.zeros(s * cap, np.uint32)
    for j, c in enumerate(live_s.tolist()):
        want[c] = seb.block_search(blocks_h[j].tobytes(), keys_h[c // cap].tobytes())
    import contextlib

    def form(algo):
        return seb.option("block_search_algo", algo) if a.forms else contextlib.nullcontext()

    algos = (1, 2) if a.forms else (1,)
    for algo in algos:
        with form(algo):
            A["cells"].fill_(0x7E57)
            search(A)
            torch.cuda.synchronize()
        got = A["cells"][: s * cap].cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want), f"form {algo}: cells differ from the host walk"
    resolve(A)
    torch.cuda.synchronize()
    status = A["status"].cpu().numpy()
    assert (status[::2] == 1).all() and (status[1::2] == 0).all(), "even probes are present, odd ones absent"

    def work(B):
        """Live cells, entries walked, and the block bytes the walks need (whole 128-B lines; 1 KiB steps)."""
        cells = B["cells"].cpu().numpy().view(np.uint32)
        bid = B["bid"].cpu().numpy().view(np.uint32)
        live = bid != 0xFFFFFFFF
        st, voff = cells >> 28, (cells >> 13) & 0x1FFF
        e = np.where(st == 2, (voff - 29) // ENTRY, 0)  # a found key's entry; a missed one is counted below
        found = live & (st == 2)
        # an absent key stops at the first greater entry: the host does not know which without the walk; take the mean
        need = np.where(found, 4 + e * ENTRY + 25, 4 + (EPB // 2) * ENTRY + 25)[live]
        entries = np.where(found, e + 1, EPB // 2 + 1)[live]
        return dict(cells=int(cells.size), live_cells=int(live.sum()), found_cells=int(found.sum()),
                    distinct_blocks=int(np.unique(bid[live]).size), entries_walked=int(entries.sum()),
                    bytes_lines128=int((-(-need // 128) * 128).sum()), bytes_steps1k=int(np.minimum(-(-need // 1024) * 1024, 4096).sum()))

    def timed(step):
        for _ in range(a.warmup):
            step()
        t = [seb.Timer() for _ in range(a.steps + 1)]
        t[0].record()
        for j in range(a.steps):
            step()
            t[j + 1].record()
        torch.cuda.synchronize()
        ms = [t[j].elapsed_ms(t[j + 1]) for j in range(a.steps)]
        return {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}

    def forms(B, rounds):
        out = {algo: [] for algo in algos}
        for _ in range(rounds):
            for algo in algos:
                with form(algo):
                    out[algo].append(timed(lambda: search(B)))
        return out

    wa = work(A)
    fa = forms(A, 2)
    res = timed(lambda: resolve(A))
    chain_default = timed(lambda: chain(A))
    plan_only = timed(lambda: plan(A))

    # the cache-resident pass: every key from a span of 8,192 keys
    rng = np.random.default_rng(lay["seed"] + 2)
    r = rng.integers(0, 8192, a.keys)
    Bc = batch(np.where(np.arange(a.keys) % 2 == 0, 2 * r, 2 * r + 1))
    chain(Bc)
    torch.cuda.synchronize()
    wc = work(Bc)
    fc = forms(Bc, 1)

    def floor_ms(w, key):
        return round((w[key] + 8 * w["cells"]) / (STREAM_TBS * 1e12) * 1e3, 4)

    line = {
        "tool": "search_bench", "layout": "lsm", "files": len(files), "keys": a.keys, "cap": cap,
        "blocks": "real layout: 32 entries of 16-B key + 100-B value per 4 KiB block, index = each block's first key",
        "pool_blocks": nblocks, "pool_bytes": nblocks * 4096, "steps": a.steps, "warmup": a.warmup,
        "distinct": dict(work=wa, floor_ms_lines128=floor_ms(wa, "bytes_lines128"), floor_ms_steps1k=floor_ms(wa, "bytes_steps1k"),
                         **{f"search_algo{k}_ms": v for k, v in fa.items()}),
        "resident": dict(work=wc, **{f"search_algo{k}_ms": v for k, v in fc.items()}),
        "resolve_ms": res, "plan_ms": plan_only, "chain_ms": chain_default,
        "checked": f"{len(live_s)} live cells of the first {s} keys equal the host walk" + (" under both forms" if a.forms else ""),
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
