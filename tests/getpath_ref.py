"""The Get path restated in plain Python for the tests of the compaction of undecided keys and of the row-mapped
join, and LSM.Get over memtables plus SSTables for the end-to-end case.

    LSM.Get   lsm/lsm.go:139-201: the active memtable, the immutable one, then the SSTables; whichever memtable
              holds the key ends the Get (a tombstone with "not found") and no file is read for it

Statuses are the C ABI's: seb_mem_status for the memtables, SEB_GET_* for the answer."""
import bisect
import struct

import numpy as np

import block_ref as br
import memget_ref as gref
import sstable_ref as sref

NONE, FOUND, TOMBSTONE = gref.NONE, gref.FOUND, gref.TOMBSTONE
GET_MISS, GET_FOUND, GET_ERROR = 0, 1, 2
NO_COL = 0xFFFF


def undecided(m: int) -> bool:
    """k_get_join's rule: the SSTables' answer stands unless the memtables said found or tombstone."""
    return m != FOUND and m != TOMBSTONE


def compact(keys, mem_status):
    """keys: a list of bytes.  (the undecided keys in batch order, row = their batch indexes)."""
    row = [i for i, m in enumerate(mem_status) if undecided(int(m))]
    return [keys[i] for i in row], np.array(row, np.uint32)


def compact_arrays(keys, mem_status, stride=None):
    """What the library must write: (sizes (n, undecided, key_bytes), out_keys u8, out_off u64 or None for a
    fixed-stride batch, row u32)."""
    out, row = compact(keys, mem_status)
    data = np.frombuffer(b"".join(out), np.uint8)
    off = None
    if stride is None:
        off = np.zeros(len(out) + 1, np.uint64)
        np.cumsum([len(k) for k in out], out=off[1:])
    return (len(keys), len(out), data.size), data, off, row


def join_rows(mem_status, row, sst_status, mem_vloc=None, mem_vlen=None, sst_col=None, sst_vloc=None, sst_vlen=None):
    """(status u8, source u8, col u16, vloc u64, vlen u32) per batch key.  A key no row names reads as a miss
    from the SSTables; a row outside the batch or naming a decided key is ignored.  Rows must be distinct."""
    n, m = len(mem_status), len(row)
    assert len(set(int(r) for r in row)) == m, "with duplicate rows the winner is unspecified"
    st, src, col = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.full(n, NO_COL, np.uint16)
    vloc, vlen = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    for i, ms in enumerate(mem_status):
        ms = int(ms)
        if ms == FOUND:
            st[i] = GET_FOUND
            vloc[i] = 0 if mem_vloc is None else mem_vloc[i]
            vlen[i] = 0 if mem_vlen is None else mem_vlen[i]
        elif ms == TOMBSTONE:
            st[i] = GET_MISS
        else:
            st[i], src[i] = GET_MISS, 1
    for j, i in enumerate(row):
        i = int(i)
        if i >= n or not undecided(int(mem_status[i])):
            continue
        st[i] = sst_status[j]
        col[i] = NO_COL if sst_col is None else sst_col[j]
        vloc[i] = 0 if sst_vloc is None else sst_vloc[j]
        vlen[i] = 0 if sst_vlen is None else sst_vlen[j]
    return st, src, col, vloc, vlen


NAMES = ("status", "source", "col", "vloc", "vlen")


def assert_same(got, want, name="", names=NAMES):
    for g, w, what in zip(got, want, names):
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape:
            raise AssertionError(f"{name}: {what} has shape {g.shape}, not {w.shape}")
        if not np.array_equal(g, w):
            at = int(np.nonzero(g != w)[0][0])
            raise AssertionError(f"{name}: {what} differs first at {at}: {g[at]} != {w[at]}")


# ------------------------------------------------------------------ LSM.Get over memtables and SSTables

class File:
    """One SSTable as the reference holds it open: level, key range, the builder's index and data section."""

    def __init__(self, file_num, level, items):
        self.file_num, self.level, self.items = file_num, level, items
        self.data, index, _, self.blens, over = sref.sections(items)
        assert over == 0
        self.min, self.max = items[0][0], items[-1][0]
        # the index block's entries: (first key, block offset) per block, as decodeIndex returns them
        self.firsts, self.offs = [], []
        (count,) = struct.unpack_from("<I", index, 0)
        at = 4
        for _ in range(count):
            ks, bo = struct.unpack_from("<IQ", index, at)
            self.firsts.append(index[at + 12: at + 12 + ks])
            self.offs.append(bo)
            at += 12 + ks

    def get(self, key):
        """SSTable.Get without the filter (a filter has no false negatives): the cell of searchBlock, and the
        block it read (None where the key sorts before the first index key)."""
        e = bisect.bisect_right(self.firsts, key) - 1
        if e < 0:
            return br.cell(br.NONE), None
        blk = self.offs[e]
        return br.search_block_ref(self.data[blk: blk + sref.BLOCK], key), blk


def lsm_get(tables, files, key):
    """LSM.Get: (status, source, value or None).  tables: memget_ref memtables, the active one first; files: in
    registration order.  L0 files are visited in that order, then per level 1..4 the first file by MinKey whose
    range covers the key; the first file that finds a live value ends the walk, and a tombstone inside an SSTable
    does not (sst.Get reports it as not found)."""
    s, _, _, value, _ = gref.lsm_get_memtables(tables, key)
    if s == FOUND:
        return GET_FOUND, 0, value
    if s == TOMBSTONE:
        return GET_MISS, 0, None
    visit = [f for f in files if f.level == 0]
    for lvl in range(1, 5):
        for f in sorted((f for f in files if f.level == lvl), key=lambda f: f.min):
            if f.min <= key <= f.max:
                visit.append(f)
                break
    for f in visit:
        c, blk = f.get(key)
        if c >> 28 == br.FOUND:
            voff, vlen = (c >> 13) & 0x1FFF, c & 0x1FFF
            return GET_FOUND, 1, f.data[blk + voff: blk + voff + vlen]
    return GET_MISS, 1, None
