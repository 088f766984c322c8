"""Record checksums at the edges of the kernels that compute them, in plain Python and numpy: WAL images for
k_wal_crc (seb_codec.hip) and hash-index segment pools for k_seg_crc / k_hidx_get (seb_hashindex.hip), each with the
expected answers from zlib.crc32 and a literal restatement of the framing rule, and `coverage`, the kernels' geometry
restated, with which every test first shows by arithmetic that its input reaches the edge it is named after.

A WAL record is [crc u32][seq u64][keySize u32][valueSize u32][deleted u8][key][value], record i = image[off[i],
off[i + 1]); crc = ChecksumIEEE(record[4:]) where the record has 4 bytes, else 0; ok = the record has 21 bytes, 21 +
keySize + valueSize is its length and the stored crc is the computed one.  A record of 4 to 20 bytes carries its right
crc here, so only the framing decides its ok = 0, and a seal restores it.

A segment record is [crc u32][timestamp u64][keySize u32][valueSize u32][key][value] at pool offset off[i]; its length
comes from its own header.  ok = the header and keySize + valueSize (< 2^32) bytes lie inside the pool and the stored
crc is ChecksumIEEE(record[4:]); valid[s] = the records of segment s before its first bad one; live = those records.
Offsets are the records' true starts; bytes between records (gaps that set an alignment) belong to no record.

The geometry (`coverage`): a workgroup owns 256 consecutive records; base = the device address of its first record
rounded down to 16; the span is staged in LDS iff end - base <= 36,864, where end is off[r1] for the WAL form and the end
of the workgroup's last record for the segment form.  A staged record is checksummed by crc_lds, any other by
crc_range; in the segment form a record of a staged workgroup that claims bytes past the window goes through
crc_range too, and one that claims bytes past the pool is refused unread."""
import struct
import zlib

import numpy as np

RECS = 256
WINDOW = 36 * 1024
WAL_HEADER, SEG_HEADER = 21, 20
REFUSED, DIRECT, STAGED = -1, 0, 1
LONG = 40_000           # a record that no window holds
LEADS = (0, 1, 15)      # device leads: the rounding down to 16 is part of a span
SPANS = (WINDOW - 1, WINDOW, WINDOW + 1)


# ------------------------------------------------------------------ the kernels' geometry

def coverage(offsets, dev_lead, ends=None, pool_bytes=None):
    """offsets: the WAL form's n + 1 boundaries, or with `ends` (each record's claimed end, from its header) and
    pool_bytes the segment form's n starts.  The image sits dev_lead bytes into a 16-aligned allocation.  Returns
    path (STAGED / DIRECT / REFUSED: not checksummed) and start4, start16, len4 (the checksummed bytes' address mod 4
    and mod 16, their count mod 4) per record, span (end - base, -1 where the segment form has none) and staged per
    workgroup."""
    off = np.asarray(offsets).astype(np.int64)
    wal = ends is None
    start, end = (off[:-1], off[1:]) if wal else (off, np.asarray(ends).astype(np.int64))
    n = start.size
    path = np.full(n, REFUSED, np.int8)
    span, staged = [], []
    for r0 in range(0, n, RECS):
        r1 = min(r0 + RECS, n)
        base = (dev_lead + int(start[r0])) & ~15
        if wal:
            span.append(dev_lead + int(off[r1]) - base)
            staged.append(span[-1] <= WINDOW)
            for i in range(r0, r1):
                if end[i] - start[i] >= 4:
                    path[i] = STAGED if staged[-1] else DIRECT
            continue
        s0, sl, el = int(start[r0]), int(start[r1 - 1]), int(end[r1 - 1])
        whole = s0 <= sl and el <= pool_bytes
        span.append(dev_lead + el - base if whole else -1)
        staged.append(whole and span[-1] <= WINDOW)
        for i in range(r0, r1):
            s, e = int(start[i]), int(end[i])
            if e > pool_bytes:
                continue
            in_window = staged[-1] and s0 <= s <= el and el - s >= SEG_HEADER
            path[i] = STAGED if in_window and e <= el else DIRECT
    body = dev_lead + start + 4
    return dict(path=path, start4=body & 3, start16=body & 15, len4=(end - start - 4) & 3, span=span, staged=staged)


def pairs(cov, path):
    """The (start mod 4, length mod 4) pairs met on `path`."""
    at = cov["path"] == path
    return set(zip(cov["start4"][at].tolist(), cov["len4"][at].tolist()))


ALL_PAIRS = {(s, l) for s in range(4) for l in range(4)}


def assert_all_pairs(cov, path, what=""):
    missing = ALL_PAIRS - pairs(cov, path)
    assert not missing, f"{what}: (start mod 4, length mod 4) pairs {sorted(missing)} never met on path {path}"


def assert_all_starts(cov, what=""):
    met = set(cov["start16"][cov["path"] != REFUSED].tolist())
    assert met == set(range(16)), f"{what}: start alignments {sorted(set(range(16)) - met)} mod 16 never met"


# ------------------------------------------------------------------ records and the rule

def _bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def wal_record(rng, seq, length):
    """A WAL record of `length` bytes: a whole one from 21 bytes on, else bytes that carry their crc where 4 exist."""
    if length < 4:
        return _bytes(rng, length)
    if length < WAL_HEADER:
        body = _bytes(rng, length - 4)
    else:
        ks = min(length - WAL_HEADER, 16)
        body = struct.pack("<QIIB", seq, ks, length - WAL_HEADER - ks, 0) + _bytes(rng, length - WAL_HEADER)
    return struct.pack("<I", zlib.crc32(body)) + body


def seg_record(key, value, ts=1_700_000_000):
    body = struct.pack("<QII", ts, len(key), len(value)) + key + value
    return struct.pack("<I", zlib.crc32(body)) + body


def _seg_sized(rng, uid, payload):
    """A segment record of 20 + payload bytes whose key is its own: the uid's bytes, as many as fit, then a value."""
    if payload < 4:
        return seg_record(struct.pack("<I", uid)[:payload], b"")
    ks = min(payload, 4 + uid % 5)
    return seg_record(struct.pack("<I", uid) + _bytes(rng, ks - 4), _bytes(rng, payload - ks))


def wal_expect(image, off):
    """(crc u32, ok u8) by the rule."""
    img = bytes(image)
    n = len(off) - 1
    crc, ok = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    for i in range(n):
        rec = img[int(off[i]):int(off[i + 1])]
        if len(rec) < 4:
            continue
        crc[i] = zlib.crc32(rec[4:])
        if len(rec) >= WAL_HEADER:
            stored, _, ks, vs = struct.unpack_from("<IQII", rec)
            ok[i] = WAL_HEADER + ks + vs == len(rec) and stored == crc[i]
    return crc, ok


def seg_ends(pool, off):
    """Each record's claimed end: off + 20 + keySize + valueSize as its header states them."""
    img = bytes(pool)
    return np.array([int(o) + SEG_HEADER + sum(struct.unpack_from("<II", img, int(o) + 12)) for o in off], np.int64)


def seg_expect(pool, off, first):
    """(ok u8 per record, valid u64 per segment, live u8 per record) by the rule."""
    img = bytes(pool)
    ok = np.zeros(len(off), np.uint8)
    for i, o in enumerate(int(x) for x in off):
        if len(img) - o < SEG_HEADER:
            continue
        stored, _, ks, vs = struct.unpack_from("<IQII", img, o)
        if ks + vs >= 2**32 or ks + vs > len(img) - o - SEG_HEADER:
            continue
        ok[i] = zlib.crc32(img[o + 4: o + SEG_HEADER + ks + vs]) == stored
    valid, live = np.zeros(len(first) - 1, np.uint64), np.zeros(len(off), np.uint8)
    for s in range(len(first) - 1):
        a, b = int(first[s]), int(first[s + 1])
        bad = np.nonzero(ok[a:b] == 0)[0]
        valid[s] = int(bad[0]) if bad.size else b - a
        live[a: a + int(valid[s])] = 1
    return ok, valid, live


def seg_keys(pool, off):
    """The distinct keys of the records that lie inside the pool, as their headers state them, in first-seen order."""
    img, seen = bytes(pool), {}
    for o, e in zip((int(x) for x in off), seg_ends(pool, off)):
        if e <= len(img):
            ks = struct.unpack_from("<I", img, o + 12)[0]
            seen.setdefault(img[o + SEG_HEADER: o + SEG_HEADER + ks], None)
    return list(seen)


def _wal_case(name, recs, lead=0, **more):
    off = np.zeros(len(recs) + 1, np.uint64)
    np.cumsum([len(r) for r in recs], out=off[1:])
    image = np.frombuffer(b"".join(recs), np.uint8).copy()
    crc, ok = wal_expect(image, off)
    return dict(name=name, form="wal", image=image, off=off, crc=crc, ok=ok, lead=lead, **more)


def _segments(n):
    """Segment boundaries inside a workgroup (100, 333) and on a workgroup's edge (256), where the records reach."""
    return np.array(sorted({0, n} | {b for b in (100, RECS, RECS + 77) if b < n}), np.uint64)


def _seg_case(name, pool, off, lead=0, **more):
    pool = np.frombuffer(bytes(pool), np.uint8).copy()
    off = np.asarray(off, np.uint64)
    first = _segments(len(off))
    base = np.array([0] + [int(off[int(f)]) for f in first[1:-1]], np.uint64)
    size = np.diff(np.concatenate([base, [pool.size]]).astype(np.uint64))
    ok, valid, live = seg_expect(pool, off, first)
    return dict(name=name, form="seg", image=pool, off=off, first=first, base=base, size=size.astype(np.uint64), ok=ok, valid=valid,
                live=live, ends=seg_ends(pool, off), lead=lead, **more)


def _seg_pack(recs, gaps=None):
    """Records back to back (gaps[i] junk bytes in front of record i): (pool bytes, offsets)."""
    buf, off = bytearray(), []
    for i, r in enumerate(recs):
        buf += b"\xEE" * (gaps[i] if gaps else 0)
        off.append(len(buf))
        buf += r
    return bytes(buf), off


# ------------------------------------------------------------------ sweep

def sweep(form, with_long=False, seed=31):
    """Checksummed lengths 0..70 (the WAL form: records of 4..74 bytes; the segment form: 16 + payloads of 0..70)
    at every start alignment mod 16.  The WAL form reaches an alignment with a filler record of 1..15 bytes, the
    segment form with a gap.  Every workgroup is staged; with_long, record 100 of every workgroup (and the last
    record, where the last workgroup has fewer) is LONG bytes long, so that every other record of the set is read
    straight from memory."""
    rng = np.random.default_rng(seed)
    recs, gaps, at = [], [], 0

    def long():
        nonlocal at
        recs.append(wal_record(rng, len(recs), LONG) if form == "wal" else _seg_sized(rng, 10**6 + len(recs), LONG - SEG_HEADER))
        gaps.append(0)
        at += LONG

    def emit(rec, gap=0):
        nonlocal at
        if with_long and len(recs) % RECS == 100:
            long()
        recs.append(rec), gaps.append(gap)
        at += gap + len(rec)

    for length in range(71):
        for align in range(16):
            fill = (align - at) % 16
            if form == "wal":
                if fill:
                    emit(wal_record(rng, len(recs), fill))
                emit(wal_record(rng, len(recs), length + 4))
            else:
                emit(_seg_sized(rng, length * 16 + align, length), fill)
    if with_long and 0 < len(recs) % RECS <= 100:
        long()
    name = f"sweep_{'direct' if with_long else 'staged'}"
    if form == "wal":
        return _wal_case(name, recs)
    return _seg_case(name, *_seg_pack(recs, gaps))


# ------------------------------------------------------------------ window

def window_lengths(span, lead, shape, two):
    """The record lengths of a `window` image, the same for both forms (a minimal record has 21 bytes in either: the
    WAL header alone, or the segment header and a 1-byte key, since a framed batch has no empty key): 256 records whose span, counted from the 16-aligned base below a
    device lead of `lead`, is exactly `span`, and whose last record ends there with start mod 4 and checksummed
    length mod 4 both in {1, 2, 3}.  shape "long": 255 minimal records (21 bytes; the first up to 3 more, which sets
    the last one's alignment) and one long record; "equal": 255 records of one size near 144 and a last one that
    lands on the edge.  two: 100 records of 21..120 bytes follow, a second workgroup whose window begins inside the
    first's last 16 bytes."""
    total = span - lead % 16
    # end = start + 4 + length and end = base + span, base = 0 mod 4: start = span - length (mod 4)
    tails = [t for t in (1, 2, 3) if (span - t) % 4 in (1, 2, 3)]
    tail = tails[lead % len(tails)]
    if shape == "long":
        extra = (total - 4 - 255 * 21 - tail) % 4
        lens = [21 + extra] + [21] * 254
    else:
        each = next(q for q in (141, 142, 143, 144) if (total - 255 * q - 4) % 4 == tail)
        lens = [each] * 255
    lens.append(total - sum(lens))
    assert (lens[-1] - 4) % 4 == tail and (lead + sum(lens[:-1])) % 4 == (span - tail) % 4 and lens[-1] >= 21
    if two:
        lens += [21 + (i * 37) % 100 for i in range(100)]
    return lens


def kv_lengths(form, lens):
    """(key length, value length) per record length: a Put / Delete batch that frames to these records.  Keys of up to
    16 bytes (the segment form: at least 1), the rest is value."""
    hdr = WAL_HEADER if form == "wal" else SEG_HEADER
    return [(min(n - hdr, 16), n - hdr - min(n - hdr, 16)) for n in lens]


def window(form, span, lead, shape, two, seed=32):
    rng = np.random.default_rng(seed + span + lead)
    lens = window_lengths(span, lead, shape, two)
    name = f"window_{span}_lead{lead}_{shape}_{'two' if two else 'one'}"
    if form == "wal":
        return _wal_case(name, [wal_record(rng, i + 1, n) for i, n in enumerate(lens)], lead, kv=kv_lengths(form, lens))
    recs = [seg_record(_bytes(rng, k), _bytes(rng, v)) for k, v in kv_lengths(form, lens)]
    return _seg_case(name, *_seg_pack(recs), lead, kv=kv_lengths(form, lens))


WINDOW_PARAMS = [(span, lead, shape) for span in SPANS for lead in LEADS for shape in ("long", "equal")]


def windows(form):
    return [window(form, span, lead, shape, two) for span, lead, shape in WINDOW_PARAMS for two in (False, True)]


def assert_window(case, cov):
    """The first workgroup spans exactly what the case's name says, is staged iff that fits, and its last record ends
    on the span's last byte at an odd alignment and an odd length."""
    span = int(case["name"].split("_")[1])
    assert cov["span"][0] == span and cov["staged"][0] == (span <= WINDOW), (case["name"], cov["span"][0])
    last = RECS - 1
    assert cov["start4"][last] in (1, 2, 3) and cov["len4"][last] in (1, 2, 3), case["name"]
    assert cov["path"][last] == (STAGED if span <= WINDOW else DIRECT)
    if len(cov["span"]) > 1:
        assert cov["staged"][1]


# ------------------------------------------------------------------ sweep geometry for a Put / Delete batch

def frame_sweep_lengths(form, with_long):
    """Record lengths for a framed batch (records back to back, whole records only): payloads 1..70, 16 times over;
    each round shifts the starts by 3 mod 16.  with_long: a LONG record as record 100 of every workgroup."""
    hdr = WAL_HEADER if form == "wal" else SEG_HEADER
    lens = []
    for _ in range(16):
        for payload in range(1, 71):
            if with_long and len(lens) % RECS == 100:
                lens.append(LONG + len(lens) // RECS)
            lens.append(hdr + payload)
    if with_long and 0 < len(lens) % RECS <= 100:
        lens.append(LONG)
    return lens


# ------------------------------------------------------------------ mixed

def mixed(form, tail, seed=33):
    """Five workgroups: the even ones staged (records of 21..100 bytes), the odd ones not (150..260 bytes), the last
    one with `tail` records; a flipped bit in records 40, 300, 600, 900 and the last."""
    rng = np.random.default_rng(seed + tail)
    n = 4 * RECS + tail
    lens = [int(rng.integers(21, 101)) if (i // RECS) % 2 == 0 else int(rng.integers(150, 261)) for i in range(n)]
    if form == "wal":
        recs = [wal_record(rng, i + 1, ln) for i, ln in enumerate(lens)]
    else:
        recs = [_seg_sized(rng, i, ln - SEG_HEADER) for i, ln in enumerate(lens)]
    for r in sorted({40, 300, 600, 900, n - 1}):
        b = bytearray(recs[r])
        b[10] ^= 0x04  # a byte of the sequence number / the timestamp
        recs[r] = bytes(b)
    name = f"mixed_{tail}"
    return _wal_case(name, recs) if form == "wal" else _seg_case(name, *_seg_pack(recs))


def assert_mixed(case, cov):
    assert cov["staged"] == [True, False, True, False, True], (case["name"], cov["span"])
    assert len(case["off"]) - (case["form"] == "wal") - 4 * RECS == int(case["name"].split("_")[1])
    ok = case["ok"]
    assert (ok[cov["path"] == STAGED] == 0).any() and (ok[cov["path"] == DIRECT] == 0).any() and ok.sum() > ok.size - 6


# ------------------------------------------------------------------ lying sizes (segment form)

LIE_AT = 128


def lying_sizes(seed=34):
    """456 records of 40..80 bytes: the first workgroup's window holds 256 of them and the pool goes on behind it.
    Record 128's keySize (or valueSize) is raised so that the record ends 1,000 bytes past the window but inside the
    pool ("inside"), exactly at pool_bytes ("edge"), or one byte past it ("past").  "sealed": the crc field is that of
    the bytes the record now claims, so the record is good and only a checksum over exactly those bytes says so."""
    out = []
    for field in ("key", "value"):
        for where in ("inside", "edge", "past"):
            for sealed in ((False, True) if where != "past" else (False,)):
                rng = np.random.default_rng(seed)
                recs = [_seg_sized(rng, i, int(rng.integers(20, 61))) for i in range(RECS + 200)]
                pool, off = _seg_pack(recs)
                pool = bytearray(pool)
                el = off[RECS]  # the first workgroup's last record ends where the next one starts
                at = off[LIE_AT]
                target = {"inside": el + 1000, "edge": len(pool), "past": len(pool) + 1}[where]
                pos = at + (12 if field == "key" else 16)
                size = struct.unpack_from("<I", pool, pos)[0] + target - off[LIE_AT + 1]
                struct.pack_into("<I", pool, pos, size)
                if sealed:
                    struct.pack_into("<I", pool, at, zlib.crc32(bytes(pool[at + 4: target])))
                case = _seg_case(f"lying_{field}_{where}{'_sealed' if sealed else ''}", pool, off, window_end=el, target=target)
                out.append(case)
    return out


def assert_lying(case, cov):
    name, r = case["name"], LIE_AT
    pool_bytes = case["image"].size
    assert cov["staged"][0] and case["ends"][r] == case["target"] and case["window_end"] < case["target"]
    assert pool_bytes + SEG_HEADER < WINDOW, "a checksum over the claimed bytes stays inside the staging array"
    if "past" in name:
        assert case["target"] == pool_bytes + 1 and cov["path"][r] == REFUSED and case["ok"][r] == 0
    else:
        assert case["target"] == (pool_bytes if "edge" in name else case["window_end"] + 1000) <= pool_bytes
        assert cov["path"][r] == DIRECT and case["ok"][r] == ("sealed" in name)
    others = np.arange(RECS) != r
    assert (cov["path"][:RECS][others] == STAGED).all() and case["ok"][np.arange(len(case["ok"])) != r].all()
    assert case["first"][1] == 100 and case["first"][2] == RECS  # the record's segment: records 100..255
    assert case["valid"][1] == (RECS - 100 if case["ok"][r] else r - 100) and case["live"][r + 1] == case["ok"][r]


# ------------------------------------------------------------------ the cases

def wal_cases():
    """name -> case: image u8, off u64 (n + 1 boundaries), crc u32, ok u8, lead (the device lead the case is built
    for), kv where a batch frames to it."""
    cases = [sweep("wal"), sweep("wal", True)] + windows("wal") + [mixed("wal", t) for t in (1, 255, 256)]
    return {c["name"]: c for c in cases}


def seg_cases():
    """name -> case: image u8 (the pool), off u64 (n starts), first / base / size (the segments), ok u8, valid u64,
    live u8, ends (the claimed ends), lead."""
    cases = [sweep("seg"), sweep("seg", True)] + windows("seg") + [mixed("seg", t) for t in (1, 255, 256)] + lying_sizes()
    return {c["name"]: c for c in cases}


def case_coverage(case, lead=None):
    lead = case["lead"] if lead is None else lead
    if case["form"] == "wal":
        return coverage(case["off"], lead)
    return coverage(case["off"], lead, case["ends"], case["image"].size)


def assert_case(case, lead=None):
    """What the case's name promises, by arithmetic; returns the coverage."""
    cov = case_coverage(case, lead)
    name = case["name"]
    if name.startswith("sweep"):
        assert_all_pairs(cov, DIRECT if name == "sweep_direct" else STAGED, name)
        assert_all_starts(cov, name)
        short = cov["path"] != REFUSED
        lens = np.diff(case["off"].astype(np.int64)) if case["form"] == "wal" else case["ends"] - case["off"].astype(np.int64)
        body = (lens - 4)[short & (lens < LONG)]
        want = set(range(71)) if case["form"] == "wal" else set(range(16, 87))
        on = (STAGED,) if name == "sweep_staged" else (DIRECT,)
        for length in sorted(want):  # every length at every alignment, on the path the case is about
            at = short & (lens - 4 == length) & np.isin(cov["path"], on)
            assert set(cov["start16"][at].tolist()) == set(range(16)), (name, length)
        assert want <= set(body.tolist())
        if name == "sweep_direct":
            assert not any(cov["staged"]) and (lens >= LONG).sum() == len(cov["staged"])
        else:
            assert all(cov["staged"])
    elif name.startswith("window"):
        assert lead is None or lead == case["lead"]
        assert_window(case, cov)
    elif name.startswith("mixed"):
        assert_mixed(case, cov)
    elif name.startswith("lying"):
        assert_lying(case, cov)
    else:
        raise AssertionError(name)
    return cov
