"""The reference's MemTable.Get and LSM.Get's memtable steps restated literally in Python, on top of
memtable_ref.MemTable, for the tests of the batched memtable lookup.

    MemTable.Get           lsm/memtable.go:95-112
    LSM.Get, first steps   lsm/lsm.go:144-166

A Go string compares bytewise, as Python's bytes do.  Statuses and the "no run" / "no entry" values are the C
ABI's (seb_mem_status, 0xFF, SEB_MEM_NO_ENTRY)."""
import bisect

import numpy as np

import memtable_ref as mref

NONE, FOUND, TOMBSTONE = 0, 1, 2
NO_RUN, NO_ENTRY = 0xFF, 2**32 - 1


def memtable_get(mt, key):
    """MemTable.Get: (value, sequence, deleted, found), and idx, which Get does not return, for the tests."""
    idx = bisect.bisect_left(mt.keys, key)                          # sort.Search(... entries[i].Key >= key)
    if idx < len(mt.entries) and mt.entries[idx][0] == key:
        _, value, seq, deleted = mt.entries[idx]                     # entry := m.entries[idx]
        return value, seq, deleted, True, idx
    return None, 0, False, False, None


def lsm_get_memtables(tables, key):
    """LSM.Get before any SSTable: the memtables in order (the active one first); whichever holds the key ends
    the Get, a tombstone with (nil, false).  (status, run, entry, value, seq); a tombstone and a miss carry no
    value (Delete stores Value nil)."""
    for r, mt in enumerate(tables):
        value, seq, deleted, found, idx = memtable_get(mt, key)
        if found:
            if deleted:
                return TOMBSTONE, r, idx, None, seq                  # return nil, false, nil
            return FOUND, r, idx, value, seq                         # return value, true, nil
    return NONE, NO_RUN, NO_ENTRY, None, 0


# ------------------------------------------------------------------ the cases the tests share

def table_from_ops(ops):
    """ops: (key, value, seq, deleted flag byte) in order -> MemTable (a non-zero flag is a Delete here: the
    tests drive the memtable directly, not through the WAL's byte == 1 rule)."""
    mt = mref.MemTable()
    for key, value, seq, flag in ops:
        if flag:
            mt.delete(key, seq)
        else:
            mt.put(key, value, seq)
    return mt


def random_table(rng, n, max_key=60, max_val=40):
    """A memtable from n random put / delete operations with memtable_ref.random_log's key distribution."""
    return table_from_ops(mref.random_log(rng, n, max_key=max_key, max_val=max_val))


def run_arrays(mt, key_lead=0, val_lead=0, deleted_byte=1):
    """GetAllEntries() in the builder's input layout: (keys u8, key_off u64, vals u8, val_off u64, deleted u8,
    seq u64); key_lead / val_lead bytes of 0xEE in front make key_off[0] / val_off[0] non-zero."""
    ents = mt.get_all_entries()
    ko, vo = [key_lead], [val_lead]
    for k, v, _, _ in ents:
        ko.append(ko[-1] + len(k))
        vo.append(vo[-1] + len(v or b""))
    keys = np.frombuffer(b"\xee" * key_lead + b"".join(e[0] for e in ents), np.uint8)
    vals = np.frombuffer(b"\xee" * val_lead + b"".join(e[1] or b"" for e in ents), np.uint8)
    dele = np.array([deleted_byte if e[3] else 0 for e in ents], np.uint8)
    seq = np.array([e[2] for e in ents], np.uint64)
    return keys, np.array(ko, np.uint64), vals, np.array(vo, np.uint64), dele, seq


def neighbours(key):
    """Byte strings right below and above a key in Go string order, and near misses."""
    out = [key + b"\x00", key + b"\xff"]
    if key:
        out += [key[:-1], key[:-1] + bytes([key[-1] ^ 1])]
        if key[-1] > 0:
            out.append(key[:-1] + bytes([key[-1] - 1]) + b"\xff")
    return out


def probes_for(tables, extra=()):
    """Every key of every run, its neighbours, and keys below the first and above the last."""
    ks = set(extra) | {b"", b"\x00", b"\xff" * 70}
    for mt in tables:
        for k in mt.keys:
            ks.add(k)
            ks.update(neighbours(k))
    return sorted(ks)


def expected(tables, probes, val_leads=None):
    """The six output arrays the library must give for `probes` over `tables`: vloc is an offset into the
    run's value bytes as run_arrays lays them out (val_leads[r] bytes in front)."""
    n = len(probes)
    st, run, ent = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    vloc, vlen, seq = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
    starts = []
    for r, mt in enumerate(tables):
        at, s = (val_leads[r] if val_leads else 0), []
        for e in mt.entries:
            s.append(at)
            at += len(e[1] or b"")
        starts.append(s)
    for i, key in enumerate(probes):
        s, r, e, value, sq = lsm_get_memtables(tables, key)
        st[i], run[i], ent[i], seq[i] = s, r, e, sq
        if s == FOUND:
            vloc[i], vlen[i] = starts[r][e], len(value)
    return st, run, ent, vloc, vlen, seq


NAMES = ("status", "run", "entry", "vloc", "vlen", "seq")


def assert_same(got, want, name=""):
    for j, what in enumerate(NAMES):
        g, w = np.asarray(got[j]), np.asarray(want[j])
        if not np.array_equal(g, w):
            at = int(np.nonzero(g != w)[0][0]) if g.shape == w.shape else -1
            raise AssertionError(f"{name}: {what} differs first at key {at}: {g[at] if at >= 0 else g.shape} != "
                                 f"{w[at] if at >= 0 else w.shape}")
