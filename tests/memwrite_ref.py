"""The reference's write side restated literally in Python on top of memtable_ref, for the tests of the memtable
write side.

    LSM.Put / LSM.Delete    lsm/lsm.go:97-137     seq = atomic.AddUint64(&lsm.sequence, 1); WAL.Append; MemTable op
    WAL.Append              lsm/wal.go:31-62      through memtable_ref.wal_record
    MemTable.Put / Delete   lsm/memtable.go:34-93 through memtable_ref.MemTable

An op is (key, value, flag): flag != 0 is a Delete, whose value bytes the reference never sees (LSM.Delete takes a
key alone and appends value nil).  The closed forms the library states (fold = the lowest-numbered holder per key,
the size delta per entry) are held to this, not assumed by it."""
import numpy as np

import memtable_ref as mref


class LSM:
    """lsm.sequence, the log image and the active memtable of one writer."""

    def __init__(self, sequence=0):
        self.sequence = sequence
        self.records = []  # what WAL.Append was called with
        self.mt = mref.MemTable()

    def put(self, key, value):
        self.sequence += 1                                   # seq := atomic.AddUint64(&lsm.sequence, 1)
        self.records.append((key, value, self.sequence, False))
        self.mt.put(key, value, self.sequence)

    def delete(self, key):
        self.sequence += 1
        self.records.append((key, b"", self.sequence, True))  # lsm.wal.Append(key, nil, seq, true)
        self.mt.delete(key, self.sequence)

    def apply(self, ops):
        """A batch in order: (the image of its records, their boundaries, MemTable.size's change)."""
        first, before = len(self.records), self.mt.size
        for key, value, flag in ops:
            if flag:
                self.delete(key)
            else:
                self.put(key, value)
        image, off = mref.wal_image(self.records[first:])
        return image, off, self.mt.size - before


def batch_records(ops, first_seq):
    """WAL.Append's arguments for a batch whose first op gets first_seq."""
    return [(k, b"" if f else v, first_seq + i, bool(f)) for i, (k, v, f) in enumerate(ops)]


def fold(tables):
    """tables: MemTables, newest first -> a MemTable with, per distinct key, the entry of the first table that holds
    it (a plain dict walk); its size by the reference's closed form."""
    seen = {}
    for mt in tables:
        for e in mt.entries:
            seen.setdefault(e[0], e)
    out = mref.MemTable()
    for k in sorted(seen):
        out.keys.append(k)
        out.entries.append(seen[k])
        out.size += len(k) + 16 + len(seen[k][1] or b"")
    return out


def entries_of(mt):
    """[(key, value bytes, deleted 0/1, seq)] as memtable_ref.unpack gives them."""
    return [(k, v or b"", 1 if d else 0, s) for k, v, s, d in mt.entries]


def fold_sizes(tables):
    f = fold(tables)
    n_in = sum(len(t.entries) for t in tables)
    ents = entries_of(f)
    return (n_in, len(ents), sum(len(e[0]) for e in ents), sum(len(e[1]) for e in ents), n_in - len(ents),
            sum(e[2] for e in ents), max([e[2] for t in tables for e in t.entries], default=0), f.size)


# ------------------------------------------------------------------ the cases the tests share

def op_arrays(ops, key_lead=0, val_lead=0, deleted_byte=1):
    """ops -> (keys u8, key_off u64, vals u8, val_off u64, deleted u8): the batch's arrays, key_lead / val_lead
    bytes of 0xEE in front; a Delete keeps whatever value bytes the op carries."""
    ko, vo = [key_lead], [val_lead]
    for k, v, _ in ops:
        ko.append(ko[-1] + len(k))
        vo.append(vo[-1] + len(v))
    keys = np.frombuffer(b"\xee" * key_lead + b"".join(o[0] for o in ops), np.uint8)
    vals = np.frombuffer(b"\xee" * val_lead + b"".join(o[1] for o in ops), np.uint8)
    dele = np.array([(f if f > 1 else deleted_byte) if f else 0 for _, _, f in ops], np.uint8)
    return keys, np.array(ko, np.uint64), vals, np.array(vo, np.uint64), dele


def random_ops(rng, n, max_key=60, max_val=80, dels=0.2, alphabet=b"ab\x00"):
    """n ops over few distinct keys (memtable_ref.random_log's key distribution); a Delete carries value bytes."""
    return [(k, v, 1 if f == 1 else 0) for k, v, _, f in
            mref.random_log(rng, n, max_key=max_key, max_val=max_val, alphabet=alphabet, dels=dels)]


def edge_ops():
    """The empty key, empty values, a Delete that carries value bytes, deleted bytes 2 and 255, ORDER_KEYS."""
    ops = [(b"", b"empty-key", 0), (b"k", b"", 0), (b"d", b"carried-but-never-written", 1), (b"", b"", 1),
           (b"two", b"xx", 2), (b"ff", b"yyy", 255), (b"k", b"again", 0)]
    return ops + [(k, b"v%d" % i, 1 if i % 5 == 0 else 0) for i, k in enumerate(mref.ORDER_KEYS)]
