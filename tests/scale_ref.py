"""Inputs with a closed-form answer, for shapes too large for the literal restatements (memtable_ref, merge_ref,
sstable_ref): a million records are built and answered by numpy in well under a second, without the library.

    replay_log   a WAL image of n fixed 33-byte records over `distinct` ids -> the replay's six arrays and sizes
    merge_pool   nruns runs of 21-byte entries, 194 to a block -> the merge's five arrays and sizes, both flags
    sst_run      n 21-byte entries with ascending ids; sst_cut gives the builder's sections of any cut into files
    last_wins    the replay of variable-length records by a dict, last record of a key wins (memtable_ref's closed
                 form: one entry per key from its last record, size = the sum of keyLen + 16 + valueLen), where
                 memtable_ref.expected's sorted-slice inserts are quadratic

Keys are big-endian u64 ids, so id order is Go string order.  Every result is cached and read-only: the tests
share it and leave it unchanged.  All comparisons against these are exact.
"""
import functools

import numpy as np

BLOCK = 4096
ENTRY = 21                       # [keySize u32][valueSize u32][deleted u8][key 8][value 4]
PER_BLOCK = (BLOCK - 4) // ENTRY  # 194: a 195th entry would make 4 + 195 * 21 = 4099 bytes

WAL_REC = np.dtype([("crc", "<u4"), ("seq", "<u8"), ("ks", "<u4"), ("vs", "<u4"), ("del", "u1"), ("key", ">u8"), ("val", "<u4")])
SST_ENT = np.dtype([("ks", "<u4"), ("vs", "<u4"), ("del", "u1"), ("key", ">u8"), ("val", "<u4")])
assert WAL_REC.itemsize == 33 and SST_ENT.itemsize == ENTRY


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _crc_table():
    t = np.arange(256, dtype=np.uint32)
    for _ in range(8):
        t = np.where(t & 1, (t >> 1) ^ np.uint32(0xEDB88320), t >> 1).astype(np.uint32)
    return t


def crc32_rows(rows):
    """zlib.crc32 of every row of a (n, width) u8 array."""
    table = _crc_table()
    crc = np.full(rows.shape[0], 0xFFFFFFFF, np.uint32)
    for j in range(rows.shape[1]):
        crc = table[(crc ^ rows[:, j]) & np.uint32(0xFF)] ^ (crc >> np.uint32(8))
    return crc ^ np.uint32(0xFFFFFFFF)


def be_keys(ids):
    """ids -> their 8-byte big-endian keys, flat u8."""
    return np.ascontiguousarray(ids, dtype=np.uint64).astype(">u8").view(np.uint8)


# ------------------------------------------------------------------ WAL replay

@functools.lru_cache(maxsize=None)
def replay_log(n, distinct, seed=0):
    """(image u8, rec_off u64 [n + 1], (keys, key_off, vals, val_off, deleted, seq), sizes): record i holds a random
    id of [0, distinct) as its key, i as its value, a random sequence and a deleted byte of {0, 1, 2}."""
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, WAL_REC)
    ids = rng.integers(0, distinct, n, dtype=np.uint64)
    rec["seq"] = rng.integers(1, 1 << 40, n, dtype=np.uint64)
    rec["ks"], rec["vs"] = 8, 4
    rec["del"] = rng.integers(0, 3, n, dtype=np.uint8)
    rec["key"] = ids
    rec["val"] = np.arange(n, dtype=np.uint32)
    rows = rec.view(np.uint8).reshape(n, 33)
    rec["crc"] = crc32_rows(rows[:, 4:])
    image = rec.view(np.uint8).reshape(-1)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(33)
    index = np.arange(n)
    order = np.lexsort((index, ids))
    sid = ids[order]
    last = np.ones(n, bool)
    last[:-1] = sid[:-1] != sid[1:]
    s = order[last]  # the last record of each id, ids ascending
    n_out = len(s)
    dele = (rec["del"][s] == 1).astype(np.uint8)
    live = dele == 0
    val_off = np.zeros(n_out + 1, np.uint64)
    np.cumsum(4 * live.astype(np.uint64), out=val_off[1:])
    out = (be_keys(ids[s]), np.arange(n_out + 1, dtype=np.uint64) * np.uint64(8), s[live].astype("<u4").view(np.uint8), val_off,
           dele, rec["seq"][s].astype(np.uint64))
    kb, vb = 8 * n_out, 4 * int(live.sum())
    sizes = (n, n_out, kb, vb, n - n_out, int(dele.sum()), int(rec["seq"].max()) if n else 0, kb + 16 * n_out + vb)
    return _frozen(image, off) + (_frozen(*out), sizes)


def last_wins(records):
    """records (key, value, seq, deleted byte) -> ([(key, value bytes, deleted 0/1, seq)] in key order, sizes): a
    record with byte 1 is a Delete, which stores no value whatever the record carried."""
    last = {}
    for key, value, seq, flag in records:
        last[key] = (key, b"" if flag == 1 else value, 1 if flag == 1 else 0, seq)
    ents = [last[k] for k in sorted(last)]
    kb, vb = sum(len(e[0]) for e in ents), sum(len(e[1]) for e in ents)
    sizes = (len(records), len(ents), kb, vb, len(records) - len(ents), sum(e[2] for e in ents),
             max((r[2] for r in records), default=0), kb + 16 * len(ents) + vb)
    return ents, sizes


# ------------------------------------------------------------------ compaction merge

@functools.lru_cache(maxsize=None)
def merge_pool(total, nruns, space, seed=0):
    """(pool u8, blen u16, run_begin list, want): run r is the sorted distinct ids among its share of `total`
    draws from [0, space); want[flags] = ((keys, key_off, vals, val_off, deleted), sizes) for flags 0 and 1
    (MERGE_DROP_TOMBSTONES).  An entry's value names its run and its place in the run."""
    rng = np.random.default_rng(seed)
    runs = [np.unique(rng.integers(0, space, total // nruns + (r < total % nruns), dtype=np.uint64)) for r in range(nruns)]
    lens = np.array([len(x) for x in runs], np.int64)
    n = int(lens.sum())
    ids = np.concatenate(runs) if n else np.zeros(0, np.uint64)
    run = np.repeat(np.arange(nruns), lens)
    pos = np.arange(n) - np.repeat(np.cumsum(lens) - lens, lens)
    ent = np.zeros(n, SST_ENT)
    ent["ks"], ent["vs"] = 8, 4
    ent["del"] = rng.choice(np.array([0, 1, 2], np.uint8), n, p=[0.7, 0.2, 0.1])
    ent["key"] = ids
    ent["val"] = (run * 1_000_003 + pos).astype(np.uint32)
    run_blocks = -(-lens // PER_BLOCK)
    run_begin = [0] + [int(x) for x in np.cumsum(run_blocks)]
    nb = run_begin[-1]
    block = np.repeat(np.array(run_begin[:-1], np.int64), lens) + pos // PER_BLOCK
    slots = np.zeros((nb, PER_BLOCK), SST_ENT)
    slots[block, pos % PER_BLOCK] = ent
    count = np.bincount(block, minlength=nb).astype("<u4")
    pool = np.zeros((nb, BLOCK), np.uint8)
    pool[:, :4] = count.view(np.uint8).reshape(nb, 4)
    pool[:, 4:4 + PER_BLOCK * ENTRY] = slots.view(np.uint8).reshape(nb, PER_BLOCK * ENTRY)
    blen = (4 + ENTRY * count).astype(np.uint16)
    order = np.lexsort((run, ids))
    sid = ids[order]
    first = np.ones(n, bool)
    first[1:] = sid[1:] != sid[:-1]
    s = order[first]  # per distinct id its entry of the lowest-numbered run, ids ascending
    want = {}
    for flags in (0, 1):
        keep = s[ent["del"][s] != 1] if flags else s
        m = len(keep)
        out = (be_keys(ids[keep]), np.arange(m + 1, dtype=np.uint64) * np.uint64(8), ent["val"][keep].astype("<u4").view(np.uint8),
               np.arange(m + 1, dtype=np.uint64) * np.uint64(4), (ent["del"][keep] == 1).astype(np.uint8))
        want[flags] = (_frozen(*out), (n, m, 8 * m, 4 * m, n - len(s), len(s) - m))
    return _frozen(pool.reshape(-1), blen) + (run_begin, want)


def key8(i):
    return b"%08d" % i


GROUP = 256  # blocks per group of the device's first[] scan (k_merge_groups / k_merge_spread)
NO_ENTRIES = (b"", b"\x07\x00\x00")  # block images that hold no entries: 0 bytes, and 3 bytes (no count)
# (blocks, the three runs' bounds): one group short of full, full, and one block over; three groups with the
# second run boundary just before, at and just after the first group edge
GROUP_POOLS = [(255, (0, 100, 200, 255)), (256, (0, 100, 200, 256)), (257, (0, 100, 256, 257)), (513, (0, 130, 255, 513)),
               (513, (0, 130, 256, 513)), (513, (0, 130, 257, 513))]


@functools.lru_cache(maxsize=None)
def group_runs(nb, bounds):
    """Three runs over a pool of nb blocks, run r = blocks [bounds[r], bounds[r + 1]): values of some 1,300 bytes,
    so a block holds three entries; blocks 255 and 256 and the pool's last block hold no entries.  The runs
    hold the multiples of 2, 3 and 5, so every two of them share keys.  Per run its block images."""
    import merge_ref as mr

    assert len(bounds) == 4 and bounds[0] == 0 and bounds[3] == nb
    rng = np.random.default_rng(1000 * nb + bounds[2])
    empty = {b: NO_ENTRIES[j % 2] for j, b in enumerate((GROUP - 1, GROUP, nb - 1)) if b < nb}
    runs = []
    for r in range(3):
        slots = range(bounds[r], bounds[r + 1])
        m = 3 * sum(b not in empty for b in slots)
        items = [(key8((2, 3, 5)[r] * j), bytes([r]) + bytes(rng.integers(0, 256, int(rng.integers(1290, 1311)), dtype=np.uint8)),
                  int(rng.random() < 0.2)) for j in range(m)]
        blocks = mr.run_blocks(items)
        assert len(blocks) == m // 3
        blocks = iter(blocks)
        runs.append([empty[b] if b in empty else next(blocks) for b in slots])
    return runs


@functools.lru_cache(maxsize=None)
def many_runs(nruns):
    """nruns runs of 0 to 20 small entries over a key space of 3 * nruns ids, so keys are shared between runs;
    every tenth run (9, 19, ...) is empty.  Per run its sorted items."""
    rng = np.random.default_rng(nruns)
    runs = []
    for r in range(nruns):
        m = 0 if r % 10 == 9 else int(rng.integers(0, 21))
        ids = sorted(int(i) for i in rng.choice(max(3 * nruns, 60), m, replace=False))
        runs.append([(key8(i), b"r%d:" % r + bytes(rng.integers(0, 256, int(rng.integers(0, 12)), dtype=np.uint8)),
                      int(rng.random() < 0.2)) for i in ids])
    return runs


# ------------------------------------------------------------------ SSTable builder

@functools.lru_cache(maxsize=None)
def sst_run(n):
    """n entries with ascending ids as the flat arrays the library takes: (key data, key offsets, value data,
    value offsets, deleted).  Every fifth deleted byte is non-zero (1, 2 or 255 in turn)."""
    i = np.arange(n, dtype=np.uint64)
    dl = np.where(i % 5 == 0, np.array([1, 2, 255], np.uint8)[(i // 5) % 3], 0).astype(np.uint8)
    vals = (i * np.uint64(2654435761) >> np.uint64(7)).astype("<u4").view(np.uint8)
    return _frozen(be_keys(3 * i + 1), _offsets(n, 8), vals, _offsets(n, 4), dl)


def _offsets(n, width):
    return np.arange(n + 1, dtype=np.uint64) * np.uint64(width)


def sst_cut(run, file_begin):
    """The builder's output for the files [file_begin[f], file_begin[f + 1]) of an sst_run, laid out back to back:
    (sizes per file, data bytes, true block lengths, index bytes, metadata bytes).  A file's block holds
    (4096 - 4) // 21 entries behind its count and is zero padded; its index entry is [8 u32][offset u64][first
    key]; the metadata is [8 u32][8 u32][min key][max key], or 8 zero bytes for a file without entries."""
    kd, _, vd, _, dl = run
    keys, vals = kd.view(">u8"), vd.view("<u4")
    sizes, data, blens, index, meta = [], [], [], [], []
    for lo, hi in zip(file_begin[:-1], file_begin[1:]):
        m = hi - lo
        nb = -(-m // PER_BLOCK)
        ent = np.zeros(nb * PER_BLOCK, SST_ENT)
        ent["ks"][:m], ent["vs"][:m] = 8, 4
        ent["del"][:m] = dl[lo:hi] != 0
        ent["key"][:m], ent["val"][:m] = keys[lo:hi], vals[lo:hi]
        count = np.minimum(PER_BLOCK, m - PER_BLOCK * np.arange(nb)).astype("<u4")
        blocks = np.zeros((nb, BLOCK), np.uint8)
        blocks[:, :4] = count.view(np.uint8).reshape(nb, 4)
        blocks[:, 4:4 + PER_BLOCK * ENTRY] = ent.view(np.uint8).reshape(nb, PER_BLOCK * ENTRY)
        idx = np.zeros(nb, np.dtype([("ks", "<u4"), ("off", "<u8"), ("key", ">u8")]))
        idx["ks"], idx["off"], idx["key"] = 8, BLOCK * np.arange(nb), keys[lo:hi:PER_BLOCK]
        x = np.array([nb], "<u4").tobytes() + idx.tobytes()
        mt = np.array([8, 8], "<u4").tobytes() + keys[lo:lo + 1].tobytes() + keys[hi - 1:hi].tobytes() if m else bytes(8)
        sizes.append((nb, BLOCK * nb, len(x), len(mt), 0))
        data.append(blocks.tobytes())
        blens += (4 + ENTRY * count).tolist()
        index.append(x)
        meta.append(mt)
    return sizes, b"".join(data), blens, b"".join(index), b"".join(meta)


def sst_slice(run, lo, hi):
    """Entries [lo, hi) of an sst_run as a run of their own (offsets from 0)."""
    kd, koff, vd, voff, dl = run
    return kd[8 * lo:8 * hi], koff[lo:hi + 1] - koff[lo], vd[4 * lo:4 * hi], voff[lo:hi + 1] - voff[lo], dl[lo:hi]


# ------------------------------------------------------------------ variable-length logs, many tiles

@functools.lru_cache(maxsize=None)
def deep_log(n, distinct):
    """memtable_ref.random_log at n records: few distinct keys and long equal-key groups (its 3-letter alphabet),
    or with `distinct` mostly distinct keys (a 256-letter alphabet, key lengths 0 to 24).  (records, wal image,
    rec_off, last_wins' entries, sizes)."""
    import memtable_ref as mref

    rng = np.random.default_rng(n + distinct)
    recs = mref.random_log(rng, n, max_key=24, max_val=120, alphabet=bytes(range(256))) if distinct else \
        mref.random_log(rng, n, max_key=60, max_val=120)
    image, off = mref.wal_image(recs)
    return (recs, image, off) + last_wins(recs)
