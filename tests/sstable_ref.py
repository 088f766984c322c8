"""Python restatement of the reference's SSTableBuilder (lsm/sstable_builder.go:42-135,185-290 and the
constants of lsm/sstable.go:11-12,47-48), shared by test_sst_build.py and test_gpu_sst_build.py.

    Builder.add / flush_block / finish   Add / flushBlock / Finish, statement for statement: the current
                                         block is a bytearray that starts as the 4-byte numEntries header
    encode_index / encode_metadata       encodeIndex / encodeMetadata
    footer                               [indexOffset u64][bloomOffset u64][metadataOffset u64][magic u32]
    build_file                           a whole file image from (key, value, deleted byte) items; the
                                         filter bytes come through oracle/bloom_np.py
    pack                                 items -> the flat arrays the library takes

Unlike block_ref.build_sstable (written earlier and independently, blocks padded to 4096 only) this one
writes oversized blocks as the reference does: unpadded, with every later offset shifted.
"""
import struct

import numpy as np

from oracle import bloom_np as bn

BLOCK = 4096
FOOTER = 28
MAGIC = 0x5354424C


class Builder:
    def __init__(self):
        self.data = bytearray()       # what file.Write has received before Finish
        self.cur = bytearray(4)       # currentBlock: make([]byte, 4)
        self.block_offset = 0
        self.index = []               # (first key, block offset)
        self.blens = []               # each written block's true length (before padding)
        self.min_key = self.max_key = b""
        self.num_entries = 0
        self.keys = []

    def add(self, key: bytes, value: bytes, deleted) -> None:
        if self.num_entries == 0:
            self.min_key = key
        self.max_key = key
        self.num_entries += 1
        self.keys.append(key)                                  # bloomFilter.Add(key)
        entry = struct.pack("<IIB", len(key), len(value), 1 if deleted else 0) + key + value
        if len(self.cur) + len(entry) > BLOCK:
            self.flush_block()
        self.cur += entry

    def flush_block(self) -> None:
        if len(self.cur) <= 4:
            return
        ks = struct.unpack_from("<I", self.cur, 4)[0]          # getFirstKeyFromBlock
        first = bytes(self.cur[13:13 + ks])
        count, off = 0, 4                                      # getNumEntriesInBlock
        while off < len(self.cur):
            if off + 9 > len(self.cur):
                break
            k, v = struct.unpack_from("<II", self.cur, off)
            off += 9
            if off + k + v > len(self.cur):
                break
            off += k + v
            count += 1
        struct.pack_into("<I", self.cur, 0, count)
        self.data += self.cur
        self.index.append((first, self.block_offset))
        self.blens.append(len(self.cur))
        self.block_offset += len(self.cur)
        if len(self.cur) < BLOCK:
            pad = BLOCK - len(self.cur)
            self.data += b"\x00" * pad
            self.block_offset += pad
        self.cur = bytearray(4)

    def encode_index(self) -> bytes:
        return struct.pack("<I", len(self.index)) + b"".join(struct.pack("<IQ", len(k), o) + k for k, o in self.index)

    def encode_metadata(self) -> bytes:
        return struct.pack("<II", len(self.min_key), len(self.max_key)) + self.min_key + self.max_key

    def bloom(self, expected_keys: int) -> bytes:
        m, k = bn.params(expected_keys, 0.01)
        if not self.keys:
            return bn.encode(np.zeros(bn.num_bytes(m), np.uint8), m, k)
        lens = np.array([len(x) for x in self.keys], np.uint64)
        off = np.zeros(len(self.keys) + 1, np.uint64)
        np.cumsum(lens, out=off[1:])
        data = np.frombuffer(b"".join(self.keys), np.uint8) if off[-1] else np.zeros(0, np.uint8)
        h1, h2 = bn.fnv_varlen(data, off)
        return bn.encode(bn.build(h1, h2, m, k), m, k)

    def finish(self, expected_keys: int):
        """(file image, data section, index block, metadata, filter bytes)."""
        if len(self.cur) > 4:
            self.flush_block()
        index_offset = self.block_offset
        index = self.encode_index()
        metadata_offset = self.block_offset + len(index)
        meta = self.encode_metadata()
        bloom_offset = metadata_offset + len(meta)
        bloom = self.bloom(expected_keys)
        data = bytes(self.data)
        return data + index + meta + bloom + footer(index_offset, bloom_offset, metadata_offset), data, index, meta, bloom


def footer(index_offset: int, bloom_offset: int, metadata_offset: int) -> bytes:
    return struct.pack("<QQQI", index_offset, bloom_offset, metadata_offset, MAGIC)


def sections(items):
    """(data, index, metadata, per-block true lengths, oversized entry count) without the filter."""
    b = Builder()
    for key, value, deleted in items:
        b.add(key, value, deleted)
    if len(b.cur) > 4:
        b.flush_block()
    over = sum(1 for k, v, _ in items if 4 + 9 + len(k) + len(v) > BLOCK)
    return bytes(b.data), b.encode_index(), b.encode_metadata(), list(b.blens), over


def build_file(items, expected_keys=None) -> bytes:
    b = Builder()
    for key, value, deleted in items:
        b.add(key, value, deleted)
    return b.finish(len(items) if expected_keys is None else expected_keys)[0]


def parse_footer(image: bytes):
    """(index offset, bloom offset, metadata offset) of a file image; the magic is checked."""
    io, bo, mo, magic = struct.unpack("<QQQI", image[-FOOTER:])
    assert magic == MAGIC
    return io, bo, mo


def pack(items, key_pad=0, val_pad=0):
    """items -> (key data u8, key offsets u64, value data u8, value offsets u64, deleted u8).
    key_pad / val_pad bytes of filler come first in the data arrays, so offsets[0] != 0."""
    keys = [k for k, _, _ in items]
    vals = [v for _, v, _ in items]
    koff = np.zeros(len(items) + 1, np.uint64)
    voff = np.zeros(len(items) + 1, np.uint64)
    np.cumsum([len(k) for k in keys], out=koff[1:])
    np.cumsum([len(v) for v in vals], out=voff[1:])
    kd = np.frombuffer(b"\xEE" * key_pad + b"".join(keys), np.uint8).copy()
    vd = np.frombuffer(b"\xDD" * val_pad + b"".join(vals), np.uint8).copy()
    dl = np.array([int(d) for _, _, d in items], np.uint8)
    return kd, koff + np.uint64(key_pad), vd, voff + np.uint64(val_pad), dl


def random_items(rng, n, max_key=40, max_val=300, sort=True):
    keys = {bytes(rng.integers(0, 256, int(rng.integers(0, max_key + 1)), dtype=np.uint8)) for _ in range(n)}
    keys = sorted(keys) if sort else list(keys)
    return [(k, bytes(rng.integers(0, 256, int(rng.integers(0, max_val + 1)), dtype=np.uint8)),
             int(rng.choice([0, 0, 0, 1, 2, 255]))) for k in keys]


def shapes():
    """[(name, items)]: the hand-built runs of the builder tests.  Names ending in _over hold an
    oversized entry."""
    e124 = lambda i: (b"k%07d" % i, b"v" * (124 - 9 - 8), 0)  # noqa: E731  9 + 8 + 107 = 124 bytes
    out = [("fill33", [e124(i) for i in range(33)]), ("fill34", [e124(i) for i in range(34)])]
    for n in (454, 455, 909):
        out.append((f"empty{n}", [(b"", b"", 0)] * n))
    out.append(("full4092", [(b"key", b"x" * (4092 - 9 - 3), 0)]))
    out.append(("full4092_then", [(b"key", b"x" * (4092 - 9 - 3), 0), (b"kez", b"y", 1)]))
    ov = lambda key, d=0: (key, b"B" * (4093 - 9 - len(key)), d)  # noqa: E731  an entry of 4,093 bytes
    small = [(b"s%03d" % i, b"val%d" % i, i % 3 == 0) for i in range(70)]
    out.append(("start_over", [ov(b"abig")] + small))
    out.append(("middle_over", small[:35] + [ov(b"s034x")] + small[35:]))
    out.append(("end_over", small + [ov(b"t", 2)]))
    out.append(("alone_over", [ov(b"big")]))
    out.append(("bigkey_over", [(b"K" * 5000, b"", 0), (b"L", b"l", 0)]))
    out.append(("empty_keys_values", [(b"", b"", 0), (b"", b"v", 1), (b"a", b"", 0), (b"b", b"", 255)]))
    out.append(("deleted_bytes", [(b"d%d" % i, b"x" * i, d) for i, d in enumerate((0, 1, 2, 255, 0, 1))]))
    out.append(("none", []))
    out.append(("one", [(b"only", b"value", 0)]))
    out.append(("one_empty", [(b"", b"", 1)]))
    out.append(("unsorted_dups", [(b"zz", b"1", 0), (b"aa", b"2", 0), (b"zz", b"3", 1), (b"zz", b"3", 0), (b"mm", b"", 0)] * 90))
    out.append(("long_keys", [(b"p" * 30 + b"%05d" % i, b"w" * (i % 50), 0) for i in range(300)]))
    return out
