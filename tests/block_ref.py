"""Python restatements of the reference's data-block code, shared by test_block_search.py and
test_gpu_block_search.py.  Python `bytes` order is Go string order.

    encode_block      the block image SSTableBuilder.Add / flushBlock write (sstable_builder.go:40-135)
    search_block_ref  searchBlock (sstable.go:242-290) as a u32 cell result
    build_sstable     the builder's block cutting: flush when len + entrySize > 4096, index key = the
                      block's first key, blocks padded to 4096
    lsm_get_ref       LSM.Get over a key's SSTables in visiting order (lsm.go:174-197)
    hand_blocks       the hand-built malformed and edge-case blocks with their probe keys
"""
import struct

import numpy as np

BLOCK = 4096
NONE, MISS, FOUND, TOMBSTONE, TRUNC = range(5)
GET_MISS, GET_FOUND, GET_ERROR = range(3)


def cell(status, voff=0, vlen=0):
    return status << 28 | voff << 13 | vlen


def encode_entry(key: bytes, value: bytes, deleted=0, ks=None, vs=None) -> bytes:
    """One entry; `deleted` is the raw byte, ks / vs override the stored sizes."""
    return struct.pack("<IIB", len(key) if ks is None else ks, len(value) if vs is None else vs, int(deleted)) + key + value


def encode_block(entries, num=None, pad=False) -> bytes:
    """entries: (key, value[, deleted byte]) tuples.  num overrides numEntries."""
    body = b"".join(encode_entry(*e) for e in entries)
    out = struct.pack("<I", len(entries) if num is None else num) + body
    assert len(out) <= BLOCK
    return out + b"\x00" * (BLOCK - len(out)) if pad else out


def search_block_ref(block: bytes, key: bytes) -> int:
    L = len(block)
    if L < 4:
        return cell(MISS)
    num = struct.unpack_from("<I", block, 0)[0]
    off = 4
    for _ in range(num):
        if off + 9 > L:
            return cell(TRUNC)
        ks, vs, d = struct.unpack_from("<IIB", block, off)
        off += 9
        if off + ks + vs > L:  # Python ints: no wrap, as Go's 64-bit int
            return cell(TRUNC)
        ek = block[off:off + ks]
        if ek == key:
            return cell(TOMBSTONE) if d == 1 else cell(FOUND, off + ks, vs)
        if ek > key:
            return cell(MISS)
        off += ks + vs
    return cell(MISS)


def build_sstable(items):
    """items: (key, value, deleted) in key order.  Returns (the data blocks' image, a multiple of
    4096 bytes, and the index entries [(first key, block offset)])."""
    image, index = bytearray(), []
    cur, count, first = bytearray(4), 0, None

    def flush():
        nonlocal cur, count, first
        if len(cur) <= 4:
            return
        struct.pack_into("<I", cur, 0, count)
        index.append((first, len(image)))
        image.extend(cur + b"\x00" * (BLOCK - len(cur)))
        cur, count, first = bytearray(4), 0, None

    for key, value, deleted in items:
        e = encode_entry(key, value, 1 if deleted else 0)
        if len(cur) + len(e) > BLOCK:
            flush()
        if first is None:
            first = key
        cur += e
        count += 1
    flush()
    return bytes(image), index


def lsm_get_ref(cells_in_order):
    """LSM.Get over the SSTables a key visits: cells_in_order = each visited file's searchBlock cell
    (NONE where no block is read).  (status, column, cell): the first FOUND ends the walk, TRUNC is
    the error, a tombstone comes back as found == false and the walk continues."""
    for j, c in enumerate(cells_in_order):
        if c >> 28 == FOUND:
            return GET_FOUND, j, c
        if c >> 28 == TRUNC:
            return GET_ERROR, j, c
    return GET_MISS, 0xFFFF, 0


def neighbours(key: bytes):
    out = [key + b"\x00", key + b"\xff", key[:-1]]
    if key:
        out += [key[:-1] + bytes([(key[-1] + 1) & 0xFF]), key[:-1] + bytes([(key[-1] - 1) & 0xFF])]
    return out


P16 = b"0123456789abcdef"
# the key family of test_gpu_locate.py::test_compare_order: ties on the first 16 bytes, prefixes both ways
FAMILY = [P16, P16 + b"\x00", P16 + b"a", P16 + b"a\x00", P16 + b"ab", P16 + b"b", P16 + b"\x7f", P16 + b"\x80",
          P16 + b"\xff" * 3, P16[:15], P16[:15] + b"\x00", P16[:8], P16[:8] + b"\x00" * 8]
ORDER_KEYS = sorted(set([b"q" * n for n in range(41)] + FAMILY + [
    b"ab", b"ab\x00", b"ab\x00\x00", b"a", b"a\x00", b"a\x7f", b"a\x80", b"a\xff", b"\x00", b"\x7f", b"\x80", b"\xff",
    b"\xff\xff", b"dup", P16 + b"dup", b""]))


def hand_blocks():
    """[(name, block image, probe keys)]: every hand-built case of the block walk."""
    abc = [(b"bb", b"v-bb"), (b"dd", b"value-dd"), (b"ff", b"")]
    base = encode_block(abc)
    out = [(f"L{n}", base[:n], [b"bb", b""]) for n in (0, 3, 4)]
    out.append(("num0", encode_block([]), [b"", b"a"]))
    out.append(("num0_padded", encode_block([], pad=True), [b"", b"a"]))
    out.append(("found_first_mid_last_below_between_above", base, [b"bb", b"dd", b"ff", b"a", b"cc", b"ee", b"zz", b"b", b"bbb"]))
    out.append(("tombstone", encode_block([(b"bb", b"x", 1), (b"dd", b"y")]), [b"bb", b"dd"]))
    out.append(("deleted2", encode_block([(b"bb", b"x", 2), (b"dd", b"y", 255)]), [b"bb", b"dd"]))
    out.append(("empty_key_entry", encode_block([(b"", b"empty"), (b"a", b"1")]), [b"", b"a", b"\x00"]))
    out.append(("empty_probe", base, [b""]))
    # zero-length values; the last value ends the block: voff = 4096
    fill = (b"k", b"v" * (BLOCK - 4 - 9 - 1 - 9 - 2))
    full = encode_block([fill, (b"zz", b"")])
    assert len(full) == BLOCK
    out.append(("voff4096", full, [b"zz", b"k"]))
    out.append(("zero_values", encode_block([(b"a", b""), (b"b", b""), (b"c", b"")]), [b"a", b"b", b"c", b"d"]))
    out.append(("header_cut_8of9", base[:len(encode_block(abc[:1])) + 8], [b"bb", b"dd", b"a"]))
    two = encode_block(abc[:2])
    out.append(("value_cut", two[:-1], [b"bb", b"dd", b"a", b"zz"]))
    out.append(("key_cut", encode_block([(b"bb", b"v"), (b"dddd", b"")])[:-1], [b"bb", b"dddd", b"dd", b"zz"]))
    wrap = struct.pack("<I", 1) + struct.pack("<IIB", 0xFFFFFFF0, 0x20, 0) + b"x" * 64
    out.append(("wrap32", wrap, [b"x", b"", b"x" * 16]))
    out.append(("wrap32_vs", struct.pack("<I", 1) + struct.pack("<IIB", 1, 0xFFFFFFFF, 0) + b"x" * 64, [b"x"]))
    out.append(("overstated", encode_block(abc, num=7, pad=True), [b"bb", b"ff", b"zz", b"", b"a"]))
    out.append(("overstated_short", encode_block(abc, num=4), [b"zz", b"ff", b""]))
    out.append(("understated", encode_block(abc, num=2), [b"bb", b"dd", b"ff", b"zz"]))
    out.append(("dup_tomb_then_value", encode_block([(b"aa", b"1"), (b"dd", b"", 1), (b"dd", b"live")]), [b"dd"]))
    out.append(("dup_value_then_tomb", encode_block([(b"aa", b"1"), (b"dd", b"live"), (b"dd", b"", 1)]), [b"dd"]))
    out.append(("unsorted", encode_block([(b"bb", b"1"), (b"ff", b"2"), (b"dd", b"3"), (b"zz", b"4")]),
                [b"dd", b"ff", b"zz", b"bb", b"cc"]))
    out.append(("empty454", struct.pack("<I", 454) + encode_entry(b"", b"") * 454, [b"", b"a"]))
    out.append(("empty454_of_455", struct.pack("<I", 455) + encode_entry(b"", b"") * 454 + b"\x00" * 6, [b"", b"a"]))
    out.append(("empty_tombs_then_key", struct.pack("<I", 41) + encode_entry(b"", b"", 1) * 40 + encode_entry(b"k", b"vv"),
                [b"", b"k", b"j"]))
    # Go string order inside a block: every key of the compare family, probed with itself and its neighbours
    fam = [(k, b"v%d" % i, 1 if i % 7 == 3 else 0) for i, k in enumerate(ORDER_KEYS)]
    img = encode_block(fam)
    probes = sorted(set(ORDER_KEYS) | {q for k in ORDER_KEYS for q in neighbours(k)})
    out.append(("order_family", img, probes))
    out.append(("order_family_padded", encode_block(fam, pad=True), probes[::3]))
    # 18 entries: past one 16-entry batch of the wave form; 70 entries: past a wave
    for n in (16, 17, 18, 33, 70):
        ents = [(b"key%03d" % i, b"val%d" % i) for i in range(n)]
        out.append((f"n{n}", encode_block(ents), [b"key%03d" % i for i in (0, 14, 15, 16, 17, 31, 32, 33, 63, 64, 69, 70) if i <= n]
                    + [b"key015x", b"key", b"kez"]))
    # long entries: a block whose walk crosses every 1 KiB staging step
    big = [(b"long-key-%02d" % i + b"." * 40, bytes([65 + i]) * 180) for i in range(16)]
    out.append(("steps_1k", encode_block(big, pad=True), [k for k, _ in big] + [b"long-key-07", b"m"]))
    out.append(("steps_1k_cut", encode_block(big)[:3000], [k for k, _ in big[9:]] + [b"zz"]))
    return out


def random_block(rng):
    """A seeded random block, possibly damaged: (image, probe keys)."""
    n = int(rng.integers(0, 40))
    keys = sorted({bytes(rng.integers(0, 256, int(rng.integers(0, 24)), dtype=np.uint8)) if rng.random() < 0.5 else
                   b"k%04d" % int(rng.integers(0, 3000)) for _ in range(n)})
    ents = [(k, bytes(rng.integers(0, 256, int(rng.integers(0, 60)), dtype=np.uint8)), int(rng.choice([0, 0, 0, 1, 2])))
            for k in keys]
    img = bytearray(encode_block(ents, pad=rng.random() < 0.3))
    mode = rng.random()
    if mode < 0.3 and len(img):  # byte flips, the header included
        for _ in range(int(rng.integers(1, 4))):
            img[int(rng.integers(0, min(len(img), 4 + 40 * 9)))] ^= 1 << int(rng.integers(0, 8))
    elif mode < 0.5:  # truncation
        img = img[: int(rng.integers(0, len(img) + 1))]
    elif mode < 0.6:  # a wrong count
        struct.pack_into("<I", img, 0, int(rng.integers(0, 60)))
    probes = list(keys[:: max(1, len(keys) // 6)])
    probes += [q for k in probes[:3] for q in neighbours(k)] + [b"", b"\xff" * 30]
    return bytes(img[:BLOCK]), probes
