"""CPU: seb_index_scan, the host-only walk of an SSTable's encoded index block as decodeIndex does
it (lsm/sstable.go:168-201), plus the order check the device layout relies on.  Python `bytes`
ordering is Go string ordering, so "sorted" here is the reference's notion."""
import struct

import pytest

SHORT, INVALID = -5, -1


def encode_index(entries, count=None) -> bytes:
    """[numEntries u32] then per entry [keySize u32][blockOffset u64][key], little-endian."""
    out = [struct.pack("<I", len(entries) if count is None else count)]
    for key, off in entries:
        out.append(struct.pack("<IQ", len(key), off) + key)
    return b"".join(out)


def fails(seb, block, code):
    with pytest.raises(seb.SebError) as e:
        seb.index_scan(block)
    assert e.value.code == code, (block, e.value)


def test_counts_entries(seb):
    assert seb.index_scan(encode_index([])) == 0
    assert seb.index_scan(encode_index([(b"k", 0)])) == 1
    assert seb.index_scan(encode_index([(b"a", 0), (b"b", 4096), (b"c" * 40, 8192)])) == 3
    assert seb.index_scan(encode_index([(b"", 0), (b"", 7), (b"\x00", 9)])) == 3  # the empty key sorts first


def test_trailing_bytes_are_ignored(seb):
    block = encode_index([(b"a", 0), (b"b", 4096)])
    assert seb.index_scan(block + b"\xff" * 13) == 2
    assert seb.index_scan(encode_index([]) + b"garbage") == 0
    # an unsorted key after the last counted entry is not part of the index
    assert seb.index_scan(encode_index([(b"b", 0), (b"a", 1)], count=1)) == 1


def test_short_blocks(seb):
    fails(seb, b"", SHORT)  # decodeIndex: "index too small"
    fails(seb, b"\x00\x00\x00", SHORT)
    block = encode_index([(b"abc", 5)])
    fails(seb, block[:4 + 11], SHORT)  # the 12-byte entry header cut at 11 bytes: "index truncated"
    fails(seb, block[:-1], SHORT)  # the key cut by one byte
    fails(seb, encode_index([(b"abc", 5)], count=2), SHORT)  # a counted entry that is not there
    two = encode_index([(b"a", 0), (b"bcd", 4096)])
    fails(seb, two[:-1], SHORT)
    assert seb.index_scan(block[:4 + 12 + 3]) == 1


def test_order(seb):
    fails(seb, encode_index([(b"b", 0), (b"a", 4096)]), INVALID)
    fails(seb, encode_index([(b"a", 0), (b"c", 1), (b"b", 2)]), INVALID)
    assert seb.index_scan(encode_index([(b"ab", 0), (b"ab\x00", 4096)])) == 2  # a proper prefix sorts first
    fails(seb, encode_index([(b"ab\x00", 0), (b"ab", 4096)]), INVALID)
    assert seb.index_scan(encode_index([(b"k", 0), (b"k", 4096), (b"k", 8192)])) == 3  # equal neighbours
    # bytewise, unsigned: 0x80 and 0xff sort after every ASCII byte
    assert seb.index_scan(encode_index([(b"a\x7f", 0), (b"a\x80", 1), (b"a\xff", 2), (b"b", 3)])) == 4
    fails(seb, encode_index([(b"a\x80", 0), (b"a\x7f", 1)]), INVALID)
    fails(seb, encode_index([(b"\xff", 0), (b"z", 1)]), INVALID)
    # keys that tie on their first 16 bytes: the tails decide
    p = b"0123456789abcdef"
    assert seb.index_scan(encode_index([(p, 0), (p + b"a", 1), (p + b"b", 2)])) == 3
    fails(seb, encode_index([(p + b"b", 0), (p + b"a", 1)]), INVALID)


def test_truncation_is_reported_where_the_walk_meets_it(seb):
    """The walk is sequential, as decodeIndex's: an unsorted pair before the cut is INVALID, a cut
    before the unsorted pair is SHORT."""
    block = encode_index([(b"b", 0), (b"a", 1), (b"c", 2)])
    fails(seb, block[:-1], INVALID)
    fails(seb, block[:4 + 13 + 5], SHORT)
