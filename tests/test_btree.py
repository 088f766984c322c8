"""CPU: the host half of the B-tree's read side (include/seb_bloom.h, "B-tree, read side") against
btree_ref's restatement, on every shared case: seb_bt_open gives readMetadata's fields, seb_bt_check the reference
rules' kind, level and counts per image, seb_bt_get the walk's (status, leaf, pos, vloc, vlen) per probe key, and
seb_get_values turns those arrays into the value bytes with the image as its pool.  Where the tree is sound (depth
<= 2 or built with the fixed split, no cell touched by hand) Get also equals the Put dictionary; the literal depth-3
tree must LOSE Put keys, so that the reference's splitInternal bug stays visible.  Corrupt images are answered by a
status, never by an exception.  Then each refusal."""
import ctypes as C

import numpy as np
import pytest

import btree_ref as bref

CASES = bref.cases()
CORRUPT = bref.corrupt_cases()
COLS = ("status", "leaf", "pos", "vloc", "vlen")


def host_all(seb, image, keys):
    meta = seb.bt_open(image)
    kind, level, stats = seb.bt_check(image, meta)
    return meta, kind, level, stats, seb.bt_get(image, meta, keys)


def against_ref(seb, image, keys, what):
    want_meta = bref.open_image(image)
    meta, kind, level, stats, got = host_all(seb, image, keys)
    assert meta.as_dict() == want_meta, what
    w_kind, w_level, w_stats = bref.check(image, want_meta)
    assert np.array_equal(kind, w_kind) and np.array_equal(level, w_level), what
    assert stats == w_stats, (what, stats, w_stats)
    want = bref.get_batch(image, want_meta, keys, w_kind)
    for name, g, w in zip(COLS, got, want):
        assert np.array_equal(g, w), (what, name)
    _, off, vals = seb.get_values(got[0], np.ones(len(keys), np.uint8), None, got[3], got[4], pool=np.frombuffer(image, np.uint8))
    w_vals = iter(bref.values(image, want))
    for i, st in enumerate(got[0]):
        chunk = vals[int(off[i]): int(off[i + 1])].tobytes()
        assert chunk == (next(w_vals) if st == bref.FOUND else b""), (what, i)
    return got, stats, w_kind


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_matches_the_reference(seb, name):
    case = CASES[name]
    keys = bref.probes(case, np.random.default_rng(5))
    got, stats, _ = against_ref(seb, case.image, keys, name)
    assert stats["bad"] == 0 and stats["uniform"] == 1 and stats["keys"] == len(case.keys), name
    assert got[0][keys.index(b"")] == bref.ERROR and got[1][keys.index(b"")] == bref.NO_PAGE
    if case.puts is not None:  # a sound tree: Get is the Put dictionary
        st, _, _, vloc, vlen = seb.bt_get(case.image, seb.bt_open(case.image), case.keys)
        assert (st == bref.FOUND).all(), name
        for k, o, n in zip(case.keys, vloc, vlen):
            assert case.image[int(o): int(o) + int(n)] == case.puts[k], (name, k)
        absent = [k for k in keys if k and k not in case.puts]
        assert (seb.bt_get(case.image, seb.bt_open(case.image), absent)[0] == bref.MISS).all(), name


def test_the_cases_hold_what_they_claim(seb):
    assert CASES["a_empty"].meta["num_pages"] == 2 and bref.page_of(CASES["a_empty"].image, 1).num_cells == 0
    for name, depth in (("e_root_split", 2), ("f_depth3_literal", 3), ("f_depth3_fixed", 3), ("g_depth4_literal", 4),
                        ("g_depth4_fixed", 4)):
        assert seb.bt_check(CASES[name].image, seb.bt_open(CASES[name].image))[2]["depth"] == depth, name
    # the reference's splitInternal hands the leftmost children to the wrong pages: keys that were Put read MISS
    for name in ("f_depth3_literal", "g_depth4_literal"):
        case = CASES[name]
        st = seb.bt_get(case.image, seb.bt_open(case.image), case.keys)[0]
        assert 0 < int((st == bref.MISS).sum()) < len(case.keys) and not (st == bref.ERROR).any(), name
    # updates and deletes: some leaf's directory order is not its physical order; one leaf of the chain is empty
    img, meta = CASES["h_updates_deletes"].image, CASES["h_updates_deletes"].meta
    pages = [bref.page_of(img, p) for p in range(1, meta["num_pages"])]
    offs = [[pg.cell_offset(i) for i in range(pg.num_cells)] for pg in pages if pg.is_leaf]
    assert any(o != sorted(o, reverse=True) for o in offs)
    assert any(pg.is_leaf and pg.num_cells == 0 and pg.right_ptr != 0 for pg in pages)
    img, meta = CASES["i_v1_mixed"].image, CASES["i_v1_mixed"].meta
    assert {bref.page_of(img, p).d[9] for p in range(1, meta["num_pages"])} == {0, 1, 2}
    # pages wider than a wave: leaves of 300 cells under a root of more than 128; several internal pages of 129
    leaf_w, int_w = bref.widths(CASES["j_wide_300"].image)
    assert leaf_w[-1] == 300 and leaf_w.count(300) > 100 and int_w == [133]
    leaf_w, int_w = bref.widths(CASES["k_wide_3level"].image)
    assert leaf_w[-1] == 100 and int_w.count(129) >= 3 and len(int_w) >= 5
    assert seb.bt_check(CASES["k_wide_3level"].image, seb.bt_open(CASES["k_wide_3level"].image))[2]["depth"] == 3
    # the boundary family: internal pages of exactly 63, 64, 65 and 128 cells, leaves one narrower
    for lc, fo in bref.BOUNDARY:
        leaf_w, int_w = bref.widths(CASES["l_boundary_%d" % (fo - 1)].image)
        assert int_w == [1, fo - 1, fo - 1] and set(leaf_w) == {lc} and fo - 1 in (63, 64, 65, 128)
    # the chains: depth 31 and 32, the key found behind 30 and 31 internal pages without a cell
    for d in (30, 31):
        case = CASES["m_chain_%d" % d]
        st = seb.bt_check(case.image, seb.bt_open(case.image))[2]
        assert st["depth"] == d + 1 and st["reach_internals"] == d and bref.widths(case.image) == ([1], [0] * d)
    # every wide edit sits on a page of 300 cells (the root: more than 128)
    for name, claim in bref.corrupt_claims().items():
        if name.startswith("wide_"):
            assert bref.page_of(CASES["j_wide_300"].image, claim["bad"][0]).num_cells in (300, 133), name


@pytest.mark.parametrize("name", sorted(CORRUPT))
def test_corrupt_image_is_answered_by_a_status(seb, name):
    image, keys = CORRUPT[name]
    got, stats, kind = against_ref(seb, image, keys, name)
    claim = bref.corrupt_claims()[name]
    if name == "unsorted":
        assert stats["bad"] == 1 and stats["reach_bad"] == 1
    if claim["errors"]:
        assert (got[0] == bref.ERROR).sum() > 1, name  # more than the empty key's
    else:
        assert (got[0] == bref.ERROR).sum() == 1 and (got[0] == bref.FOUND).any() and (got[0] == bref.MISS).any(), name
    if "bad" in claim:  # exactly these pages are bad
        assert list(np.nonzero(kind == bref.BAD)[0]) == [0] + sorted(claim["bad"]), name
    for k, v in claim.get("stats", {}).items():
        assert stats[k] == v, (name, k, stats)
    level = seb.bt_check(image, seb.bt_open(image))[1]
    for p, lv in claim.get("level", {}).items():
        assert level[p] == lv, (name, p)
    if name.startswith("chain_"):  # every key, the present one too, ends at the 32nd page of the walk
        assert (got[0] == bref.ERROR).all() and (got[1][:-1] == bref.MAX_DEPTH).all(), name
    if name == "self_pointer":  # the cycle ends at the 32nd page
        i = keys.index(b"a")
        assert got[0][i] == bref.ERROR and got[1][i] == bref.open_image(image)["root"]
    if name == "num_pages_past_image":
        meta = seb.bt_open(image)
        assert meta.header_pages == 1000 and meta.num_pages == len(image) // bref.PAGE


def test_long_and_fixed_width_keys(seb):
    """A batch key longer than any stored key, and the fixed-stride layout."""
    case = CASES["e_root_split"]
    meta = seb.bt_open(case.image)
    long = bref.long_keys(case)
    got = seb.bt_get(case.image, meta, long)
    want = bref.get_batch(case.image, case.meta, long)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    fixed = np.frombuffer(b"".join(case.keys), np.uint8).reshape(len(case.keys), 8)
    assert (seb.bt_get(case.image, meta, fixed)[0] == bref.FOUND).all()


def test_refusals(seb):
    L = seb.lib()
    case = CASES["e_root_split"]
    img = np.frombuffer(case.image, np.uint8)
    meta = seb.seb_bt_meta()
    for bad in (case.image[:4095], b"", b"XTRE" + case.image[4:]):
        with pytest.raises(seb.SebError) as e:
            seb.bt_open(bad)
        assert e.value.code == -1 and "seb_bt_open" in str(e.value)
    assert L.seb_bt_open(img.ctypes.data, img.size, None) == -1
    meta = seb.bt_open(case.image)
    st = np.zeros(2, np.uint8)
    kb = seb.as_keys([b"a", b"b"])
    assert L.seb_bt_get(img.ctypes.data, img.size, None, kb.ref, st.ctypes.data, None, None, None, None) == -1
    assert L.seb_bt_get(img.ctypes.data, img.size, C.byref(meta), kb.ref, None, None, None, None, None) == -1
    assert L.seb_bt_get(None, img.size, C.byref(meta), kb.ref, st.ctypes.data, None, None, None, None) == -1
    assert L.seb_bt_check(img.ctypes.data, img.size, None, None, None, None) == -1
    short = seb.seb_bt_meta(meta.root, meta.header_pages, meta.free_list, meta.num_pages + 1)  # pages the image lacks
    assert L.seb_bt_check(img.ctypes.data, img.size, C.byref(short), None, None, None) == -1
    assert "do not fit" in seb.last_error()
    assert L.seb_bt_get(img.ctypes.data, img.size, C.byref(short), kb.ref, st.ctypes.data, None, None, None, None) == -1
    down = seb.HostKeys(np.frombuffer(b"abcd", np.uint8), np.array([0, 3, 2], np.uint64))  # offsets that decrease
    assert L.seb_bt_get(img.ctypes.data, img.size, C.byref(meta), down.ref, st.ctypes.data, None, None, None, None) == -1
    # nullable outputs, and an empty batch
    assert L.seb_bt_check(img.ctypes.data, img.size, C.byref(meta), None, None, None) == 0
    assert L.seb_bt_get(img.ctypes.data, img.size, C.byref(meta), kb.ref, st.ctypes.data, None, None, None, None) == 0
    assert all(a.size == 0 for a in seb.bt_get(case.image, meta, []))
