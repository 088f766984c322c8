"""The hash index's read side restated in plain Python (hashindex/segment.go, recovery.go, hashindex.go:217-260):
a segment writer, recover() and Get over a dict, and the cases the CPU and GPU tests share.

A record is [crc u32][timestamp u64][keySize u32][valueSize u32][key][value], little-endian, crc =
ChecksumIEEE(record[4:]); valueSize == 0 is a tombstone.  recover() walks the segments oldest first, each from offset
0: fewer than 20 bytes left, or a payload that runs past the end of the file, is io.EOF: it breaks WITHOUT truncating;
a complete record whose CRC does not match cuts the segment at its offset and ends that segment's walk; every record
before that sets latestValues[key].  Tombstones stay in the index (the `entry.size == 0` test is on the whole record's
size).  Get looks the key up, re-verifies the record's CRC (mismatch: an error) and only then returns the value; an
empty one is ErrKeyNotFound.  The one departure (include/seb_bloom.h): keySize + valueSize >= 2^32 counts as a CRC
failure.

Corruptions are single-bit flips, which CRC-32 always detects, so this file alone decides every case."""
import struct
import zlib

import numpy as np

HEADER = 20
MISS, FOUND, ERROR = 0, 1, 2
NO_RECORD = 2**64 - 1


def record(key: bytes, value: bytes, ts: int = 1_700_000_000) -> bytes:
    """segment.append's bytes."""
    body = struct.pack("<QII", ts, len(key), len(value)) + key + value
    return struct.pack("<I", zlib.crc32(body)) + body


class Writer:
    """A segment being appended to: put / delete, the file's bytes, and where each record went."""

    def __init__(self, ts: int = 1_700_000_000):
        self.buf, self.ts, self.offsets = bytearray(), ts, []

    def put(self, key: bytes, value: bytes):
        self.offsets.append(len(self.buf))
        self.buf += record(key, value, self.ts)
        self.ts += 1
        return self

    def delete(self, key: bytes):
        return self.put(key, b"")

    def bytes(self) -> bytes:
        return bytes(self.buf)


def flip(seg: bytes, byte: int, bit: int = 0) -> bytes:
    b = bytearray(seg)
    b[byte] ^= 1 << bit
    return bytes(b)


def read_record(seg: bytes, offset: int):
    """readRecord: ("eof",), ("bad",) or ("ok", key, value, next offset)."""
    if len(seg) - offset < HEADER:
        return ("eof",)
    crc, _, ks, vs = struct.unpack_from("<IQII", seg, offset)
    if ks + vs >= 2**32:  # the stated departure
        return ("bad",)
    if len(seg) - offset - HEADER < ks + vs:
        return ("eof",)
    if zlib.crc32(seg[offset + 4: offset + HEADER + ks + vs]) != crc:
        return ("bad",)
    key = seg[offset + HEADER: offset + HEADER + ks]
    return ("ok", key, seg[offset + HEADER + ks: offset + HEADER + ks + vs], offset + HEADER + ks + vs)


def recover(segments):
    """recover(): a dict with index (key -> (segment, offset)), valid / size_after / short_tail / cut per segment,
    records (the walk's, the cutting one included) and live_records."""
    index = {}
    valid, size_after, short_tail, cut = [], [], [], []
    for s, seg in enumerate(segments):
        offset, n, size, tail, was_cut = 0, 0, len(seg), 0, 0
        while offset < len(seg):
            r = read_record(seg, offset)
            if r[0] == "eof":
                tail = 1
                break
            if r[0] == "bad":
                size, was_cut = offset, 1
                break
            index[r[1]] = (s, offset)
            offset = r[3]
            n += 1
        valid.append(n), size_after.append(size), short_tail.append(tail), cut.append(was_cut)
    return dict(index=index, valid=valid, size_after=size_after, short_tail=short_tail, cut=cut, live_records=sum(valid))


def get(segments, index, key: bytes, verify: bool = True):
    """HashIndex.Get -> segment.read: (status, pool offset of the record or NO_RECORD, vloc, vlen, value)."""
    if key not in index:
        return MISS, NO_RECORD, 0, 0, b""
    s, offset = index[key]
    seg = segments[s]
    crc, _, ks, vs = struct.unpack_from("<IQII", seg, offset)
    if verify and zlib.crc32(seg[offset + 4: offset + HEADER + ks + vs]) != crc:
        return ERROR, NO_RECORD, 0, 0, b""
    if vs == 0:
        return MISS, NO_RECORD, 0, 0, b""
    base = sum(len(x) for x in segments[:s])
    return FOUND, base + offset, base + offset + HEADER + ks, vs, seg[offset + HEADER + ks: offset + HEADER + ks + vs]


def get_batch(segments, index, keys, verify: bool = True):
    rows = [get(segments, index, k, verify) for k in keys]
    return (np.array([r[0] for r in rows], np.uint8), np.array([r[1] for r in rows], np.uint64),
            np.array([r[2] for r in rows], np.uint64), np.array([r[3] for r in rows], np.uint32), [r[4] for r in rows])


def key_lists(keys):
    """A key list as (data u8, offsets u64): the variable-length seb_keys layout."""
    off = np.zeros(len(keys) + 1, np.uint64)
    np.cumsum([len(k) for k in keys], out=off[1:])
    data = np.frombuffer(b"".join(keys), np.uint8) if off[-1] else np.zeros(0, np.uint8)
    return data, off


def probes(rec, rng, extra=()):
    """Case h's batch for a recovered store: every indexed key (deleted ones included), absent keys, the zero-length
    key, and repeats, shuffled."""
    present = sorted(rec["index"])
    absent = [b"absent-%d" % i for i in range(7)] + [k + b"\x00" for k in present[:5]] + [k[:-1] for k in present[:5] if len(k) > 1]
    keys = present + absent + [b""] + present[:9] * 2 + list(extra)
    order = rng.permutation(len(keys))
    return [keys[i] for i in order]


# ------------------------------------------------------------------ the shared cases

def _counted(n, ts=1):
    w = Writer(ts)
    for i in range(n):
        if i % 7 == 3:
            w.delete(b"key-%04d" % (i // 2))
        else:
            w.put(b"key-%04d" % (i % max(n * 2 // 3, 1)), bytes([i & 255]) * (i % 40 + 1))
    return w


def cases(rng=None):
    """name -> list of segment images (bytes), oldest first."""
    rng = np.random.default_rng(5) if rng is None else rng
    out = {}
    # a: an empty segment; one record; 63 / 64 / 65 / 257 records
    out["a_empty"] = [b""]
    out["a_empty_between"] = [_counted(5).bytes(), b"", _counted(3, 50).bytes()]
    for n in (1, 63, 64, 65, 257):
        out[f"a_{n}"] = [_counted(n).bytes()]
    # b: key lengths 0-300, prefixes of one another, equal-length keys that differ in the last byte; values 0-5000
    w1, w2 = Writer(), Writer(10_000)
    stem = bytes(rng.integers(0, 256, 300, dtype=np.uint8))
    for ln in range(301):
        w = w1 if ln % 2 else w2
        w.put(stem[:ln], bytes(rng.integers(0, 256, int(rng.integers(0, 5001)), dtype=np.uint8)))
    for ln in (1, 8, 15, 16, 17, 31, 32, 33, 200):
        for last in (0, 1, 255):
            w2.put(b"\x07" * (ln - 1) + bytes([last]), b"same-length-%d-%d" % (ln, last))
    w2.put(b"", b"the empty key, again")
    out["b_lengths"] = [w1.bytes(), w2.bytes()]
    # c: one key written 3,001 times
    w = Writer()
    for i in range(3001):
        w.put(b"the-one-key", b"value-%d" % i)
    out["c_one_key"] = [w.bytes()]
    # d: Put, Delete, Put of one key across three segments; the same with the Delete last
    filler = lambda t: Writer(t).put(b"other-%d" % t, b"x" * 30)  # noqa: E731
    out["d_put_delete_put"] = [filler(1).put(b"k", b"first").bytes(), filler(2).delete(b"k").bytes(),
                               filler(3).put(b"k", b"third").bytes()]
    out["d_put_put_delete"] = [filler(1).put(b"k", b"first").bytes(), filler(2).put(b"k", b"second").bytes(),
                               filler(3).delete(b"k").bytes()]
    # e: three segments, a flipped bit in a middle record of the middle one
    segs = []
    for s in range(3):
        w = Writer(1000 * s)
        for i in range(40):
            w.put(b"e-%02d" % ((i * 3 + s) % 50), b"seg%d-rec%d" % (s, i) * (i % 4 + 1))
        segs.append(w)
    mid = segs[1]
    for where, name in ((mid.offsets[17] + HEADER + 2, "key"), (mid.offsets[17] + 1, "crc"), (mid.offsets[17] + 9, "timestamp"),
                        (mid.offsets[18] - 1, "value"), (mid.offsets[0] + 5, "first_record")):
        out[f"e_flip_{name}"] = [segs[0].bytes(), flip(mid.bytes(), where, 3), segs[2].bytes()]
    # a flipped size bit: the payload then runs past the end of the file (io.EOF: no cut, the records behind it are
    # never seen), or the record is read at another length and fails its CRC (a cut)
    out["e_flip_size_eof"] = [segs[0].bytes(), flip(mid.bytes(), mid.offsets[17] + 18, 6), segs[2].bytes()]
    out["e_flip_size_cut"] = [segs[0].bytes(), flip(mid.bytes(), mid.offsets[17] + 16, 0), segs[2].bytes()]
    # f: a last segment ending inside a header, and inside a payload; no cut, sizes unchanged
    last = segs[2].bytes()
    out["f_short_header"] = [segs[0].bytes(), segs[1].bytes(), last[: segs[2].offsets[30] + 11]]
    out["f_short_payload"] = [segs[0].bytes(), segs[1].bytes(), last[: segs[2].offsets[30] + HEADER + 3]]
    out["f_short_then_more"] = [segs[0].bytes(), last[: segs[2].offsets[30] + 19], segs[1].bytes()]
    out["f_only_a_tail"] = [last[:7]]
    # g: a header with keySize + valueSize >= 2^32 (its CRC field is whatever the bytes hold)
    for ks, vs, name in ((0xFFFFFFF0, 0x20, "g_wrap_small"), (0xFFFFFFFF, 1, "g_wrap_one"), (0x80000000, 0x80000000, "g_wrap_zero")):
        bad = struct.pack("<IQII", 0x12345678, 77, ks, vs) + b"payload-bytes-behind-the-header" * 3
        head = mid.bytes()[: mid.offsets[20]]
        out[name] = [segs[0].bytes(), head + bad + record(b"after", b"never seen"), segs[2].bytes()]
    return out


def big_store(rng, records=300_000, keys=100_000, segments=4):
    """About `records` records over `keys` keys of 16 bytes with 20-60 byte values and some deletes, in `segments`
    segments."""
    import keygen as kg
    ids = rng.integers(0, keys, records)
    table = kg.key16(np.arange(keys))
    lens = rng.integers(20, 61, records)
    dele = rng.random(records) < 0.05
    per = (records + segments - 1) // segments
    out = []
    for s in range(segments):
        w = Writer(s * per)
        for i in range(s * per, min((s + 1) * per, records)):
            k = table[ids[i]].tobytes()
            w.put(k, b"" if dele[i] else ((b"%08d" % i) * 8)[: lens[i]])
        out.append(w.bytes())
    return out, table
