"""The reference's memtable and WAL recovery restated literally in Python, for the tests of the WAL replay.

    MemTable.Put / Delete / GetAllEntries   lsm/memtable.go:34-93,129-137
    WAL.Append                              lsm/wal.go:31-62
    WAL.ReadAll's record parse              lsm/wal.go:98-146
    recoverFromWAL                          lsm/lsm.go:273-298

A Go string compares bytewise, as Python's bytes do.  The closed forms the library states (one entry per key
from its last record, size = the sum over the survivors of keyLen + 16 + valueLen) are held to this, not
assumed by it.
"""
import bisect
import struct
import zlib


class MemTable:
    """A sorted slice with binary search; `size` follows the reference's arithmetic line by line."""

    def __init__(self):
        self.keys = []     # the entries' keys, kept apart so that bisect can search them
        self.entries = []  # (key, value or None, sequence, deleted)
        self.size = 0

    def put(self, key, value, seq):
        idx = bisect.bisect_left(self.keys, key)                      # sort.Search(... entries[i].Key >= key)
        entry = (key, value, seq, False)
        if idx < len(self.entries) and self.entries[idx][0] == key:
            old_size = len(self.entries[idx][1] or b"")              # oldSize := len(m.entries[idx].Value)
            self.entries[idx] = entry
            self.size += len(value) - old_size
        else:
            self.keys.insert(idx, key)
            self.entries.insert(idx, entry)
            self.size += len(key) + len(value) + 16

    def delete(self, key, seq):
        idx = bisect.bisect_left(self.keys, key)
        entry = (key, None, seq, True)                                # Value: nil
        if idx < len(self.entries) and self.entries[idx][0] == key:
            old_size = len(self.entries[idx][1] or b"")
            self.entries[idx] = entry
            self.size -= old_size
        else:
            self.keys.insert(idx, key)
            self.entries.insert(idx, entry)
            self.size += len(key) + 16

    def get_all_entries(self):
        return list(self.entries)


def wal_record(key, value, seq, deleted):
    """WAL.Append's record; `deleted` True / False as Append takes it, or an int to write that byte."""
    flag = deleted if isinstance(deleted, int) and not isinstance(deleted, bool) else (1 if deleted else 0)
    body = struct.pack("<QIIB", seq, len(key), len(value), flag) + key + value
    return struct.pack("<I", zlib.crc32(body)) + body


def wal_image(records):
    """records: (key, value, seq, deleted) -> (image bytes, the n + 1 record boundaries)."""
    off, parts = [0], []
    for r in records:
        parts.append(wal_record(*r))
        off.append(off[-1] + len(parts[-1]))
    return b"".join(parts), off


def read_all(image):
    """ReadAll's parse of a well-formed image: [(key, value, seq, deleted)]; deleted = (byte == 1)."""
    out, at = [], 0
    while at < len(image):
        crc, seq, ks, vs, flag = struct.unpack_from("<IQIIB", image, at)
        data = image[at + 21:at + 21 + ks + vs]
        assert len(data) == ks + vs and crc == zlib.crc32(image[at + 4:at + 21 + ks + vs])
        out.append((data[:ks], data[ks:], seq, flag == 1))
        at += 21 + ks + vs
    return out


def recover(entries):
    """recoverFromWAL over ReadAll's entries: (the memtable, lsm.sequence)."""
    mt, sequence = MemTable(), 0
    for key, value, seq, deleted in entries:
        if seq > sequence:
            sequence = seq
        if deleted:
            mt.delete(key, seq)
        else:
            mt.put(key, value, seq)
    return mt, sequence


def expected(records):
    """What the replay must return for these records: ([(key, value bytes, deleted 0/1, seq)], sizes)."""
    image, _ = wal_image(records)
    mt, sequence = recover(read_all(image))
    ents = [(k, v or b"", 1 if d else 0, s) for k, v, s, d in mt.get_all_entries()]
    n_out = len(ents)
    sizes = (len(records), n_out, sum(len(e[0]) for e in ents), sum(len(e[1]) for e in ents), len(records) - n_out,
             sum(e[2] for e in ents), sequence, mt.size)
    return ents, sizes


def unpack(keys, key_off, vals, val_off, deleted, seq):
    keys, vals = bytes(keys), bytes(vals)
    return [(keys[int(key_off[i]):int(key_off[i + 1])], vals[int(val_off[i]):int(val_off[i + 1])], int(deleted[i]), int(seq[i]))
            for i in range(len(deleted))]


# ------------------------------------------------------------------ the cases the tests share

P16 = b"0123456789abcdef"
P40 = P16 * 2 + b"01234567"
ORDER_KEYS = [b"", b"a", b"a\x00", b"a\x00\x00", b"a\x00\x01", b"a\x01", b"b", b"\x00", b"\x00\x00", b"\xff", b"\xff\xff",
              P16, P16 + b"\x00", P16 + b"a", P16 + b"\x80", P16[:15], P16[:15] + b"\xff", P16 + b"ab", P16 + b"ac",
              P40, P40 + b"\x00", P40 + b"a", P40 + b"\x80", P40 + b"\xff\x01", P40[:39], P40[:39] + b"\x7f"]


def random_log(rng, n, max_key=300, max_val=5000, alphabet=b"ab\x00", dels=0.2):
    """n records over few distinct keys (a small alphabet, short lengths favoured), every deleted byte of
    {0, 1, 2, 255}, deleted records that carry value bytes, and sequences out of order."""
    recs = []
    for _ in range(n):
        klen = int(rng.integers(0, 4)) if rng.random() < 0.7 else int(rng.integers(0, max_key + 1))
        key = bytes(alphabet[int(x)] for x in rng.integers(0, len(alphabet), klen))
        vlen = int(rng.integers(0, 40)) if rng.random() < 0.9 else int(rng.integers(0, max_val + 1))
        val = bytes(rng.integers(0, 256, vlen, dtype="uint8"))
        flag = int(rng.choice([0, 1, 2, 255], p=[1 - dels - 0.1, dels, 0.05, 0.05]))
        recs.append((key, val, int(rng.integers(0, 1 << 40)), flag))
    return recs


def order_log():
    """Every ORDER_KEYS key three times, in descending then ascending then descending order."""
    ks = sorted(ORDER_KEYS)
    recs = []
    for rnd, seq in ((0, reversed(ks)), (1, ks), (2, reversed(ks))):
        for i, k in enumerate(seq):
            recs.append((k, b"round%d-%d" % (rnd, i), 1000 * rnd + i, 1 if (rnd == 1 and i % 3 == 0) else 0))
    return recs
