"""CPU: the host half of the block-id step (seb_block_ids) against blockids_ref's restatement of
the rules and, with no residency table and file numbers put in for slots, against seb_blocks_dedup element for
element.  Every rule, the SEB_ERR_RANGE retry, the sizes-only call, cells == 0 and each refusal."""
import ctypes as C

import numpy as np
import pytest

import blockids_ref as bref

NO_BLOCK, NO_ID, PAD = bref.NO_BLOCK, bref.NO_ID, bref.PAD
SIZES = (0, 1, 63, 64, 65, 255, 257, 2049)


def check(seb, cand, blocks, first=None, count=None, id_base=0):
    want = bref.block_ids(cand, blocks, first, count, id_base)
    got = seb.block_ids(cand, blocks, first, count, id_base)
    assert got[0] == want[0], "sizes"
    bref.assert_same(got[1:], want[1:])
    return want


@pytest.mark.parametrize("name", [p for p in bref.PATTERNS if p != "mixed"])
def test_no_table_equals_the_rules_and_blocks_dedup(seb, name):
    """With no residency table every live cell is a miss; with the slots' file numbers in `files`, bid and the read
    list are seb_blocks_dedup's wherever no offset reaches 2^48 and no cell is padding with a real offset."""
    slot_file = np.array([900, 17, 5, 2**40, 33, 1, 77, 8, 250, 64], np.uint64)
    for cells in SIZES[1:]:
        cand, blocks = bref.pattern(name, cells)
        sizes, bid, us, ub = check(seb, cand, blocks)
        assert sizes[1] == 0 and sizes[4] == 0
        live = cand != PAD
        files = slot_file[np.where(live, cand, 0)]
        dbid, uf, dub = seb.blocks_dedup(files, np.where(live, blocks, NO_BLOCK).astype(np.uint64))
        assert np.array_equal(dbid, bid) and np.array_equal(uf, slot_file[us]) and np.array_equal(dub, ub), (name, cells)


def test_every_rule_with_a_mixed_table(seb):
    first, count = bref.table_mixed()
    for cells in SIZES:
        cand, blocks = bref.pattern("mixed", max(cells, 1))
        cand, blocks = cand[:cells], blocks[:cells]
        for id_base in (0, 1000):
            sizes, *_ = check(seb, cand, blocks, first, count, id_base)
        if cells >= 255:
            assert all(s > 0 for s in sizes), sizes  # resident, misses, uniq and bad all occur
    # one cell per rule, by hand
    cand = np.array([PAD, 1, 0, 0, 0, 0, 3, 3, 5, 2, 8, 2, 8], np.uint16)
    blocks = np.array([4096, NO_BLOCK, 2**48, 9 * 4096, 10 * 4096, 4097, 2 * 4096, 3 * 4096, 0, 4096, 4096, 4096, 0],
                      np.uint64)
    sizes, bid, us, ub = seb.block_ids(cand, blocks, first, count, id_base=50)
    assert bid.tolist() == [NO_ID, NO_ID, NO_ID, 109, NO_ID, NO_ID, NO_ID - 1, NO_ID, NO_ID, 50, 51, 50, 52]
    assert us.tolist() == [2, 8, 8] and ub.tolist() == [4096, 4096, 0]
    assert sizes == (13, 2, 4, 3, 5)
    # a table shorter than the slots in use: the slots past it are misses
    sizes, bid, us, ub = seb.block_ids(cand, blocks, first[:1], count[:1])
    assert sizes == bref.block_ids(cand, blocks, first[:1], count[:1])[0] and sizes[1] == 1


def test_range_retry_sizes_only_and_empty(seb):
    cand, blocks = bref.pattern("7x3", 257)
    want = bref.block_ids(cand, blocks)
    uniq = want[0][3]
    assert uniq == 21
    with pytest.raises(seb.SebError) as e:
        seb.block_ids(cand, blocks, uniq_cap=uniq - 1)
    assert e.value.code == -4 and e.value.sizes == want[0]
    got = seb.block_ids(cand, blocks, uniq_cap=e.value.sizes[3])
    assert got[0] == want[0]
    bref.assert_same(got[1:], want[1:])
    got = seb.block_ids(cand, blocks, uniq_cap=uniq + 9)  # a larger capacity: nothing past uniq is part of the answer
    bref.assert_same(got[1:], want[1:])
    # the sizes alone: every output NULL, the capacity and id_base not looked at
    sz = seb.seb_blockids_sizes()
    L = seb.lib()
    assert L.seb_block_ids(cand.ctypes.data, blocks.ctypes.data, 257, None, None, 0, NO_ID, None, None, None, 0, C.byref(sz)) == 0
    assert sz.as_tuple() == want[0] and sz.reserved == 0
    # cells == 0, with and without pointers
    assert L.seb_block_ids(None, None, 0, None, None, 0, 0, None, None, None, 0, C.byref(sz)) == 0
    assert sz.as_tuple() == (0, 0, 0, 0, 0)
    got = seb.block_ids(np.zeros((0, 3), np.uint16), np.zeros((0, 3), np.uint64))
    assert got[0] == (0, 0, 0, 0, 0) and got[1].shape == (0, 3) and got[2].size == 0 and got[3].size == 0


def test_refusals(seb):
    L = seb.lib()
    cand, blocks = bref.pattern("7x3", 65)
    first, count = bref.table_mixed()
    bid, us, ub = np.zeros(65, np.uint32), np.zeros(65, np.uint16), np.zeros(65, np.uint64)
    sz = seb.seb_blockids_sizes()
    p = lambda a: a.ctypes.data  # noqa: E731

    def call(cand_=p(cand), blocks_=p(blocks), cells=65, first_=None, count_=None, slots=0, id_base=0, bid_=p(bid),
             us_=p(us), ub_=p(ub), cap=65, sz_=C.byref(sz)):
        return L.seb_block_ids(cand_, blocks_, cells, first_, count_, slots, id_base, bid_, us_, ub_, cap, sz_)

    assert call() == 0
    uniq = sz.uniq
    assert call(sz_=None) == -1
    assert call(cand_=None) == -1 and call(blocks_=None) == -1
    assert call(first_=None, count_=p(count), slots=6) == -1 and call(first_=p(first), count_=None, slots=6) == -1
    assert call(bid_=None) == -1 and call(us_=None) == -1 and call(ub_=None) == -1
    assert call(cells=2**32) == -1 and b"2^32" in L.seb_last_error()
    assert call(cells=2**32 - 1, cand_=None) == -1
    # ids are u32 and SEB_NO_BLOCK_ID is none: id_base + uniq may reach 2^32 - 1 and not pass it
    assert call(id_base=NO_ID - uniq) == 0 and int(bid.max()) == NO_ID - 1
    assert call(id_base=NO_ID - uniq + 1) == -1 and b"id_base" in L.seb_last_error()
    assert call(cap=uniq - 1) == -4 and sz.uniq == uniq
