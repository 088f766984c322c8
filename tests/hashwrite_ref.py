"""The hash index's write side restated in plain Python on top of hashindex_ref (hashindex/segment.go:61-125,
hashindex.go:92-215 and 360-385, compaction.go:12-132): a Put / Delete batch as segment.append's records, the
rotation's cuts, compactSegments + applyCompaction, getLogicalSize, and the cases the CPU and GPU tests share.

append: the record of hashindex_ref.record; Delete is Put(key, nil); one timestamp per call.  Rotation: a record goes
to the active segment iff that segment's size is below the limit BEFORE the append, otherwise the engine rotates once
and the record opens the new segment.  compactSegments walks the chosen segments in list order, each from offset 0:
io.EOF (a short header or a payload past the end) ends that segment's walk silently, a CRC mismatch aborts the whole
compaction; the last record of a key wins among the chosen segments only; a winner with an empty value is dropped;
the others are written with a fresh timestamp.  The reference writes them in a Go map's order: the set is fully
determined, and log order (ascending position of each surviving record) is the one fixed here."""
import numpy as np

import hashindex_ref as href

HEADER = href.HEADER


def frame(ops, ts):
    """ops: (key, value) pairs, value None for a Delete -> (image bytes, offsets of len(ops) + 1 boundaries)."""
    recs = [href.record(k, b"" if v is None else v, ts) for k, v in ops]
    off = np.zeros(len(recs) + 1, np.uint64)
    np.cumsum([len(r) for r in recs], out=off[1:])
    return b"".join(recs), off


def cuts(lens, active_size, limit):
    """The first op of each new segment."""
    out, size = [], active_size
    for j, ln in enumerate(lens):
        if size >= limit:
            out.append(j)
            size = 0
        size += ln
    return out


def compact(segments, num_segments, ts):
    """compactSegments of the oldest num_segments segments: None where it aborts, else a dict: image, rec_off (the
    survivors' offsets and the image's size), and every size counter."""
    latest, n = {}, 0
    for s, seg in enumerate(segments[:num_segments]):
        offset = 0
        while offset < len(seg):
            r = href.read_record(seg, offset)
            if r[0] == "eof":
                break
            if r[0] == "bad":
                return None
            latest[r[1]] = (s, offset, r[2])
            offset = r[3]
            n += 1
    winners = sorted((s, offset, key, value) for key, (s, offset, value) in latest.items())
    recs = [href.record(key, value, ts) for _, _, key, value in winners if value]
    off = np.zeros(len(recs) + 1, np.uint64)
    np.cumsum([len(r) for r in recs], out=off[1:])
    return dict(image=b"".join(recs), rec_off=off, records_in=n, live_in=n, distinct=len(latest), survivors=len(recs),
                tombstoned=len(latest) - len(recs), shadowed=n - len(latest), image_bytes=int(off[-1]))


def count_drop(segments, num_segments):
    """applyCompaction: the index entries deleted = the keys whose latest record overall is a tombstone in a compacted
    segment."""
    rec = href.recover(segments)
    return sum(1 for key, (s, offset) in rec["index"].items()
               if s < num_segments and href.read_record(segments[s], offset)[2] == b"")


def logical_size(segments, index):
    """getLogicalSize: keySize + valueSize over the index entries, tombstoned ones included."""
    total = 0
    for key, (s, offset) in index.items():
        r = href.read_record(segments[s], offset)
        total += len(r[1]) + len(r[2])
    return total


def answers(segments, keys):
    """What Get answers for each key after recover(): (status, value)."""
    rec = href.recover(segments)
    return [(g[0], g[4]) for g in (href.get(segments, rec["index"], k) for k in keys)]


def all_deleted():
    """A store where every key ends deleted: two segments of puts, the deletes in the second."""
    w1, w2 = href.Writer(), href.Writer(500)
    for i in range(40):
        w1.put(b"gone-%02d" % i, b"v" * (i + 1))
    for i in range(0, 40, 3):
        w2.put(b"gone-%02d" % i, b"again")
    for i in range(40):
        w2.delete(b"gone-%02d" % i)
    return [w1.bytes(), w2.bytes()]


# ------------------------------------------------------------------ the shared frame cases

def ops_arrays(ops, lead=0, stride=None):
    """(keys for as_keys, vals u8, val_off u64, deleted u8) for a list of (key, value or None); `lead` bytes sit in
    front of the first value (val_off[0] != 0); stride: the fixed-length layout (every key has that length).  A
    Delete carries value bytes that must not appear."""
    vals = [b"ignored-for-a-delete" if v is None else v for _, v in ops]
    val_off = np.zeros(len(ops) + 1, np.uint64)
    val_off[0] = lead
    np.cumsum([len(v) for v in vals], out=val_off[1:])
    val_off[1:] += np.uint64(lead)
    blob = np.frombuffer(b"\xEE" * lead + b"".join(vals), np.uint8)
    deleted = np.array([v is None for _, v in ops], np.uint8)
    if stride is not None:
        keys = np.frombuffer(b"".join(k for k, _ in ops), np.uint8).reshape(len(ops), stride)
    else:
        keys = href.key_lists([k for k, _ in ops])
    return keys, blob, val_off, deleted


def frame_cases(rng=None):
    """name -> (ops, lead, stride): batches of 0, 1, 63, 64, 65 and 257 ops, key lengths 1-300 and values 0-5,000
    bytes with deletes in the offsets layout, 16-byte keys in the stride layout, val_off[0] != 0."""
    rng = np.random.default_rng(11) if rng is None else rng
    out = {}

    def batch(n, stride=None, vmax=5001):
        ops = []
        for i in range(n):
            kl = stride if stride is not None else (i % 300 + 1 if n > 64 else int(rng.integers(1, 301)))
            key = bytes(rng.integers(0, 256, kl, dtype=np.uint8))
            if rng.random() < 0.2:
                ops.append((key, None))
            else:
                ops.append((key, bytes(rng.integers(0, 256, int(rng.integers(0, vmax)), dtype=np.uint8))))
        return ops

    for n in (0, 1, 63, 64, 65, 257):
        out[f"offsets_{n}"] = (batch(n), 0, None)
        out[f"stride_{n}"] = (batch(n, 16, 120), 0, 16)
    out["lead_65"] = (batch(65), 37, None)
    out["lead_stride_64"] = (batch(64, 16, 90), 5, 16)
    out["only_deletes"] = ([(b"d-%d" % i, None) for i in range(70)], 3, None)
    return out
