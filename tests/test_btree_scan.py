"""CPU: the host half of the B-tree's range scans (include/seb_bloom.h, "B-tree, range scans").

seb_bt_dir_build equals btree_scan_ref's restatement byte for byte on every accepted case and refuses, with the same
page in its message, every image the restatement refuses: every corrupt image of btree_ref, the two literal deep
trees, hand edits of the chain, a leaf listed twice, keys out of order across a leaf boundary.  seb_bt_scan equals the
scan by directory in every array, and on every non-empty start the LITERAL iterator entry for entry, except across
the emptied leaf of h_updates_deletes, where the literal iterator must stop and the library go on.  With an empty start
the library equals the sorted Put dictionary; on e_root_split the literal empty-start seek must skip keys (the finding
stays visible).  limit, the caps' retry convention, R = 0."""
import bisect
import struct

import numpy as np
import pytest

import btree_ref as bref
import btree_scan_ref as sref

CASES = bref.cases()
CORRUPT = bref.corrupt_cases()
ACCEPTED = sorted(n for n in CASES if sref.accepted(n))


def host_dir(seb, image):
    meta = seb.bt_open(image)
    kind, level, _ = seb.bt_check(image, meta)
    return meta, kind, level


def built(seb, image):
    meta, kind, level = host_dir(seb, image)
    d, info = seb.bt_dir_build(image, meta, kind, level)
    return meta, d, info


def refused(seb, image, rule=None):
    """The library refuses with the page the restatement names; returns (rule, page)."""
    meta, kind, level = host_dir(seb, image)
    with pytest.raises(sref.Refused) as want:
        sref.build_dir(image, bref.open_image(image), kind, level)
    with pytest.raises(seb.SebError) as e:
        seb.bt_dir_build(image, meta, kind, level)
    assert e.value.code == -1 and f"page {want.value.page}:" in str(e.value), (str(e.value), str(want.value))
    if rule:
        assert want.value.rule == rule, str(want.value)
    return want.value.rule, want.value.page


@pytest.mark.parametrize("name", ACCEPTED)
def test_directory_equals_the_restatement(seb, name):
    case = CASES[name]
    meta, d, info = built(seb, case.image)
    kind, level, st = bref.check(case.image, case.meta)
    want, w_info = sref.build_dir(case.image, case.meta, kind, level)
    assert d.size == want.size == seb.bt_dir_bytes(meta.num_pages)
    assert info == w_info and info["keys"] == st["keys"] and info["leaves"] == st["reach_leaves"] and info["depth"] == st["depth"]
    assert d.tobytes() == want.tobytes(), name


@pytest.mark.parametrize("name", ACCEPTED)
def test_scan_equals_the_restatement_and_the_literal_iterator(seb, name):
    case = CASES[name]
    meta, d, info = built(seb, case.image)
    starts, ends = sref.ranges(case, np.random.default_rng(3), d)
    got = seb.bt_scan(case.image, meta, d, starts, ends)
    want = sref.scan_by_dir(case.image, case.meta, d, starts, ends)
    for k in sref.ARRAYS:
        assert np.array_equal(got[k], want[k]), (name, k)
    assert not got["range_status"].any() and (got["status"] == bref.FOUND).all() and (got["source"] == 1).all()
    stopped = 0
    ordered = sorted(case.puts.items()) if case.puts is not None else None
    for r, (s, e) in enumerate(zip(starts, ends)):
        mine = sref.pairs_of(got, r)
        assert [k for k, _ in mine] == sorted(k for k, _ in mine) and all((not s or k >= s) and (not e or k < e) for k, _ in mine)
        if ordered is not None:
            lo = bisect.bisect_left(ordered, (s,))
            hi = bisect.bisect_left(ordered, (e,)) if e else len(ordered)
            assert mine == ordered[lo: max(lo, hi)], (name, r)
        if not s:
            continue
        lit, end = sref.literal_scan(case.image, case.meta, s, e or None)
        if end == "done":
            assert lit == mine, (name, r, s, e)
        else:  # an empty leaf inside the chain: the literal iterator stops there, the library goes on
            assert name == "h_updates_deletes" and end in ("error", "nil-key") and mine[: len(lit)] == lit, (name, r, s, e)
            stopped += len(mine) > len(lit)  # not where the range itself ends at the empty leaf
    assert (stopped > 0) == (name == "h_updates_deletes")
    if case.keys:
        assert int(got["range_off"][-1]) > len(case.keys)  # the ranges overlap: more entries than keys


def test_the_literal_empty_start_skips_keys():
    """iterator.go's seek descends by CellAt(0).Child: the subtree under RightPtr is never visited."""
    case = CASES["e_root_split"]
    lit, end = sref.literal_scan(case.image, case.meta, b"", None)
    assert end == "done" and 0 < len(lit) < len(case.puts)
    assert [k for k, _ in lit] == sorted(case.puts)[len(case.puts) - len(lit):]


def test_empty_start_on_a_root_leaf_agrees(seb):
    for name in ("a_empty", "b_one_key", "c_lengths"):
        case = CASES[name]
        if bref.page_of(case.image, case.meta["root"]).is_leaf:
            meta, d, _ = built(seb, case.image)
            got = seb.bt_scan(case.image, meta, d, [b""], [b""])
            assert sref.pairs_of(got, 0) == sref.literal_scan(case.image, case.meta, b"", None)[0]


# ------------------------------------------------------------------ refusals

@pytest.mark.parametrize("name", sorted(CORRUPT))
def test_corrupt_images_are_refused(seb, name):
    image = CORRUPT[name][0]
    rule, page = refused(seb, image)
    want = {"chain_32": "deep", "chain_33": "deep", "two_levels": "mixed", "two_parents": "mixed", "last_page_other_level": "mixed",
            "self_pointer": "level"}.get(name, "bad")
    assert rule == want, (name, rule, page)


@pytest.mark.parametrize("name", ["f_depth3_literal", "g_depth4_literal"])
def test_literal_deep_trees_are_refused(seb, name):
    """splitInternal's exchanged pointers: the chain no longer follows the key order, and the keys do not increase."""
    case = CASES[name]
    assert refused(seb, case.image)[0] == "chain"
    # the order rule fails too: with every RightPtr rewritten to follow the listed order, the keys still do not increase
    kind, level, _ = bref.check(case.image, case.meta)
    lst = [case.meta["root"]]
    while not bref.page_of(case.image, lst[0]).is_leaf:
        lst = [c for p in lst for c in [bref.page_of(case.image, p).right_ptr] + [x.child for x in bref.page_of(case.image, p).cells()]]
    b = bytearray(case.image)
    for p, nxt in zip(lst, lst[1:] + [0]):
        bref.page_of(b, p).right_ptr = nxt
    assert refused(seb, bytes(b))[0] == "order"


def edited(image, fn):
    b = bytearray(image)
    fn(lambda p: bref.page_of(b, p))
    return bytes(b)


def leaves_of(seb, image):
    meta, d, info = built(seb, image)
    return [int(p) for p in sref.dir_arrays(d, meta.num_pages)[0]]


def test_hand_edits(seb):
    case = CASES["f_depth3_fixed"]
    lv = leaves_of(seb, case.image)
    assert len(lv) > 8
    # one leaf's RightPtr swapped for another leaf's; the last leaf's non-zero
    rule, page = refused(seb, edited(case.image, lambda pg: setattr(pg(lv[3]), "right_ptr", lv[6])), "chain")
    assert page == lv[3]
    rule, page = refused(seb, edited(case.image, lambda pg: setattr(pg(lv[-1]), "right_ptr", lv[0])), "chain")
    assert page == lv[-1]

    # a leaf listed twice: a parent's cell re-pointed at its neighbour's leaf (same level, both good)
    root = bref.page_of(case.image, case.meta["root"])
    parent = root.right_ptr
    pp = bref.page_of(case.image, parent)

    def repoint(pg):
        p = pg(parent)
        off = p.cell_offset(1)
        struct.pack_into(">I", p.d, off + bref.uvarint16(p.d, off)[1], p.cell_at(0, leaf=False).child)
    rule, page = refused(seb, edited(case.image, repoint), "twice")
    assert page == pp.cell_at(0, leaf=False).child

    # the order broken across a leaf boundary, both leaves individually good: the first key of leaf 5 rewritten (same
    # length) to sort below the last key of leaf 4 and still below its own second key
    def lower(pg):
        p = pg(lv[5])
        c = p.cell_at(0)
        p.d[c.koff: c.koff + len(c.key)] = b"\x01" * len(c.key)
    img = edited(case.image, lower)
    assert bref.page_kind(bref.page_of(img, lv[5]), case.meta["num_pages"]) == bref.LEAF
    rule, page = refused(seb, img, "order")
    assert page == lv[4]


def test_root_outside(seb):
    case = CASES["e_root_split"]
    b = bytearray(case.image)
    struct.pack_into(">I", b, 4, case.meta["num_pages"] + 3)
    assert refused(seb, bytes(b), "root")[1] == case.meta["num_pages"] + 3


def test_scan_refuses_a_foreign_directory(seb):
    a, b = CASES["e_root_split"], CASES["c_lengths"]
    meta_a, d_a, _ = built(seb, a.image)
    meta_b, d_b, _ = built(seb, b.image)
    with pytest.raises(seb.SebError) as e:
        seb.bt_scan(a.image, meta_a, np.zeros(d_a.size, np.uint8), [b"k"], [b""])
    assert e.value.code == -1 and "directory" in str(e.value)
    if meta_a.num_pages != meta_b.num_pages:
        with pytest.raises(seb.SebError):
            seb.bt_scan(a.image, meta_a, np.concatenate([d_b, np.zeros(d_a.size, np.uint8)])[: d_a.size], [b"k"], [b""])


# ------------------------------------------------------------------ limit, caps, R = 0

def test_limit(seb):
    case = CASES["e_root_split"]
    meta, d, info = built(seb, case.image)
    leaf, first, _ = sref.dir_arrays(d, meta.num_pages)
    n0 = int(first[1])
    assert info["leaves"] >= 2 and n0 >= 3
    keys = sorted(case.puts)
    starts, ends = [b"", keys[1], keys[0], b""], [b"", b"", keys[-1], keys[2]]
    for limit in (1, n0 - 1, n0, 0, 10**9):  # 1; a cut inside the first leaf; exactly its last cell; none
        got = seb.bt_scan(case.image, meta, d, starts, ends, limit)
        want = sref.scan_by_dir(case.image, case.meta, d, starts, ends, limit)
        for k in sref.ARRAYS:
            assert np.array_equal(got[k], want[k]), (limit, k)
        full = [keys, keys[1:], keys[:-1], keys[:2]]
        for r, f in enumerate(full):
            assert [k for k, _ in sref.pairs_of(got, r)] == (f[:limit] if limit else f), (limit, r)


def test_caps_retry(seb):
    case = CASES["c_lengths"]
    meta, d, _ = built(seb, case.image)
    starts, ends = [b"", case.keys[2]], [b"", b""]
    full = seb.bt_scan(case.image, meta, d, starts, ends)
    ne, nk, nv = full["sizes"][1:]
    assert ne == 2 * len(case.keys) - 2 and nk > 0 and nv > 0
    for caps in ((ne - 1, nk, nv), (ne, nk - 1, nv), (ne, nk, nv - 1), (0, 0, 0)):
        with pytest.raises(seb.SebError) as e:
            seb.bt_scan(case.image, meta, d, starts, ends, caps=caps)
        assert e.value.code == -4 and e.value.sizes == (2, ne, nk, nv), (caps, str(e.value))
        again = seb.bt_scan(case.image, meta, d, starts, ends, caps=e.value.sizes[1:])
        assert all(np.array_equal(again[k], full[k]) for k in sref.ARRAYS)
    roomy = seb.bt_scan(case.image, meta, d, starts, ends, caps=(ne + 5, nk + 9, nv + 1))
    assert all(np.array_equal(roomy[k], full[k]) for k in sref.ARRAYS)


def test_no_ranges_and_no_entries(seb):
    case = CASES["e_root_split"]
    meta, d, _ = built(seb, case.image)
    got = seb.bt_scan(case.image, meta, d, [], [])
    assert got["sizes"] == (0, 0, 0, 0) and list(got["range_off"]) == [0] and got["status"].size == 0
    got = seb.bt_scan(case.image, meta, d, [b"zzz", b"key-0003"], [b"", b"key-0003"])
    assert got["sizes"] == (2, 0, 0, 0) and list(got["range_off"]) == [0, 0, 0] and list(got["key_off"]) == [0]
    empty = CASES["a_empty"]
    meta, d, info = built(seb, empty.image)
    assert info == dict(leaves=1, keys=0, depth=1)
    assert seb.bt_scan(empty.image, meta, d, [b"", b"a"], [b"", b"b"])["sizes"] == (2, 0, 0, 0)
    with pytest.raises(seb.SebError):
        seb.bt_scan(case.image, meta, d, [b"a", b"b"], [b""])
