"""Python restatements of the reference's compaction merge (lsm/compaction.go), shared by test_merge.py and
test_gpu_merge.py.  Python `bytes` order is Go string order.

    load_block   SSTableIterator.loadBlock (:69-124): the entries of one block image, (key, value, deleted)
                 with deleted = (byte == 1); a cut header or payload ends the block silently
    go_merge     mergeFiles' loop (:226-333) on an emulation of container/heap (Init / Push / Pop with up and
                 down as in Go); Less orders by key alone, every Sequence being 0
    rule_merge   the library's stated rule: per distinct key the entry of the lowest-numbered run, ascending;
                 drop = a surviving tombstone is removed (targetLevel == 4)
    pool_of      runs of block images -> (pool u8, blen u16, run_begin)
    run_blocks   sorted items -> the block images SSTableBuilder cuts (sstable_ref.Builder)
    unpack       the library's five output arrays -> [(key, value, deleted)]
"""
import struct

import numpy as np

import sstable_ref as sr

BLOCK = 4096


def load_block(image: bytes):
    out = []
    L = len(image)
    if L < 4:
        return out
    num = struct.unpack_from("<I", image, 0)[0]
    off = 4
    for _ in range(num):
        if off + 9 > L:
            break
        ks, vs, d = struct.unpack_from("<IIB", image, off)
        off += 9
        if off + ks + vs > L:  # Python ints: no wrap, as Go's 64-bit int
            break
        out.append((bytes(image[off:off + ks]), bytes(image[off + ks:off + ks + vs]), d == 1))
        off += ks + vs
    return out


def load_offsets(image: bytes):
    """The offsets of the 9-byte headers load_block's entries start at."""
    out, L = [], len(image)
    if L < 4:
        return out
    num = struct.unpack_from("<I", image, 0)[0]
    off = 4
    for _ in range(num):
        if off + 9 > L:
            break
        ks, vs = struct.unpack_from("<II", image, off)
        if off + 9 + ks + vs > L:
            break
        out.append(off)
        off += 9 + ks + vs
    return out


class _Heap:
    """container/heap over a Go slice of (key, value, deleted, run); Less by key (Sequence is always 0, so
    for equal keys `h[i].Sequence > h[j].Sequence` is false)."""

    def __init__(self):
        self.h = []

    def less(self, i, j):
        return self.h[i][0] < self.h[j][0]

    def swap(self, i, j):
        self.h[i], self.h[j] = self.h[j], self.h[i]

    def up(self, j):
        while True:
            i = (j - 1) // 2 if j > 0 else 0  # Go's (j - 1) / 2 truncates towards zero
            if i == j or not self.less(j, i):
                break
            self.swap(i, j)
            j = i

    def down(self, i0, n):
        i = i0
        while True:
            j1 = 2 * i + 1
            if j1 >= n:
                break
            j = j1
            if j1 + 1 < n and self.less(j1 + 1, j1):
                j = j1 + 1
            if not self.less(j, i):
                break
            self.swap(i, j)
            i = j

    def push(self, x):
        self.h.append(x)
        self.up(len(self.h) - 1)

    def pop(self):
        n = len(self.h) - 1
        self.swap(0, n)
        self.down(0, n)
        return self.h.pop()


def go_merge(runs, level):
    """runs: per input file its entries [(key, value, deleted)] in iterator order.  The entries mergeFiles
    hands its builders, in order."""
    pos = [0] * len(runs)
    hp = _Heap()

    def nxt(r):
        if pos[r] < len(runs[r]):
            e = runs[r][pos[r]]
            pos[r] += 1
            return (e[0], e[1], e[2], r)
        return None

    for r in range(len(runs)):
        e = nxt(r)
        if e is not None:
            hp.push(e)
    out = []
    while hp.h:
        entry = hp.pop()
        e = nxt(entry[3])
        if e is not None:
            hp.push(e)
        if hp.h and hp.h[0][0] == entry[0]:
            continue
        if level == 4 and entry[2]:
            continue
        out.append(entry[:3])
    return out


def rule_merge(runs, drop=False):
    best = {}
    for run in runs:
        for k, v, d in run:
            best.setdefault(k, (k, v, d))
    return [best[k] for k in sorted(best) if not (drop and best[k][2])]


def run_blocks(items):
    """Sorted (key, value, deleted) items -> the block images of the file SSTableBuilder writes, true lengths."""
    data, _, _, blens, over = sr.sections(items)
    assert over == 0
    return [data[b * BLOCK:b * BLOCK + blens[b]] for b in range(len(blens))]


def pool_of(runs, full_blen=False, fill=0):
    """runs: per run its block images (each at most 4096 bytes).  (pool u8, blen u16, run_begin list): a block's
    slot is padded with `fill` bytes past its image; full_blen: blen = 4096 for every block, which needs zero
    padding to read the same."""
    slots, blen, run_begin = [], [], [0]
    for blocks in runs:
        for img in blocks:
            assert len(img) <= BLOCK
            slots.append(bytes(img) + bytes([0 if full_blen else fill]) * (BLOCK - len(img)))
            blen.append(BLOCK if full_blen else len(img))
        run_begin.append(len(slots))
    pool = np.frombuffer(b"".join(slots), np.uint8).copy() if slots else np.zeros(0, np.uint8)
    return pool, np.array(blen, np.uint16), run_begin


def decoded(runs):
    """Per run of block images the entries the reference's iterator yields."""
    return [[e for img in blocks for e in load_block(img)] for blocks in runs]


def unpack(keys, key_off, vals, val_off, deleted):
    kb, vb = bytes(np.asarray(keys, np.uint8)), bytes(np.asarray(vals, np.uint8))
    ko, vo = [int(x) for x in key_off], [int(x) for x in val_off]
    return [(kb[ko[i]:ko[i + 1]], vb[vo[i]:vo[i + 1]], int(deleted[i])) for i in range(len(ko) - 1)]


def as_bytes(entries):
    """[(key, value, deleted bool)] with the flag as the 1 / 0 byte the library writes."""
    return [(k, v, 1 if d else 0) for k, v, d in entries]


def random_runs(rng, nruns, nkeys, share=0.0, max_key=24, max_val=40):
    """nruns sorted runs of items over a common key space; `share` = the chance a key goes to a second and a
    third run as well.  Values carry the run number."""
    keys = sorted({bytes(rng.integers(0, 256, int(rng.integers(0, max_key + 1)), dtype=np.uint8)) for _ in range(nkeys)})
    runs = [[] for _ in range(nruns)]
    for k in keys:
        owners = {int(rng.integers(0, nruns))}
        while rng.random() < share and len(owners) < nruns:
            owners.add(int(rng.integers(0, nruns)))
        for r in owners:
            v = b"r%d:" % r + bytes(rng.integers(0, 256, int(rng.integers(0, max_val + 1)), dtype=np.uint8))
            runs[r].append((k, v, int(rng.random() < 0.2)))
    return runs
