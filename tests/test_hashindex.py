"""CPU: the host half of the hash index's read side (include/seb_bloom.h, "hash index, read side")
against hashindex_ref's restatement of recover() and Get, on every shared case: seb_seg_scan + seb_seg_verify give
the reference's valid / size_after / short_tail / cut per segment, seb_hidx_lookup its (status, rec, vloc, vlen) per
key with verify on and off and its key count, and seb_get_values turns those arrays into the reference's value bytes
with the segment pool as its pool.  Records corrupted after the index was built turn ERROR under verify only, a
corrupted tombstone included.  Then each refusal."""
import ctypes as C

import numpy as np
import pytest

import hashindex_ref as href

CASES = href.cases()


def host_recover(seb, segments):
    pool, rec_off, first, base, size, tails = seb.segs_scan(segments)
    ok, valid, after, live = seb.seg_verify(pool, rec_off, first, base, size)
    return dict(pool=pool, rec_off=rec_off, first=first, base=base, size=size, short_tail=tails, ok=ok, valid=valid,
                size_after=after, live=live)


def check_recover(h, want, what):
    assert list(h["valid"]) == want["valid"], what
    assert list(h["size_after"]) == want["size_after"], what
    counts = np.diff(h["first"].astype(np.int64))
    cut = [int(v < c) for v, c in zip(h["valid"], counts)]
    assert cut == want["cut"], what
    # the scan looks at no CRC: what it says of the bytes behind a cut, recover never reads
    assert [int(t and not c) for t, c in zip(h["short_tail"], cut)] == want["short_tail"], what
    for s, (f, v, c) in enumerate(zip(h["first"][:-1], h["valid"], counts)):
        f, v = int(f), int(v)
        assert h["ok"][f: f + v].all() and h["live"][f: f + v].all(), (what, s)
        assert not h["live"][f + v: f + int(c)].any(), (what, s)
        if v < c:
            assert h["ok"][f + v] == 0, (what, s)


def check_get(seb, h, segments, index, keys, verify, what):
    st, rec, vloc, vlen, distinct = seb.hidx_lookup(h["pool"], h["rec_off"], h["live"], href.key_lists(keys), verify)
    w_st, w_rec, w_vloc, w_vlen, w_vals = href.get_batch(segments, index, keys, verify)
    for name, g, w in (("status", st, w_st), ("rec", rec, w_rec), ("vloc", vloc, w_vloc), ("vlen", vlen, w_vlen)):
        assert np.array_equal(g, w), (what, name, verify)
    assert distinct == len(index), what
    _, off, vals = seb.get_values(st, np.ones(len(keys), np.uint8), None, vloc, vlen, pool=h["pool"])
    for i, w in enumerate(w_vals):
        assert vals[int(off[i]): int(off[i + 1])].tobytes() == w, (what, i)
    return st


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_matches_the_reference(seb, name):
    segments = CASES[name]
    want = href.recover(segments)
    h = host_recover(seb, segments)
    check_recover(h, want, name)
    keys = href.probes(want, np.random.default_rng(3))
    for verify in (True, False):
        check_get(seb, h, segments, want["index"], keys, verify, name)


def test_the_cases_hold_what_they_claim():
    """Tombstones stay in the index, the cut drops the records behind it, the third segment still applies."""
    r = href.recover(CASES["d_put_put_delete"])
    assert b"k" in r["index"] and href.get(CASES["d_put_put_delete"], r["index"], b"k")[0] == href.MISS
    r = href.recover(CASES["d_put_delete_put"])
    assert href.get(CASES["d_put_delete_put"], r["index"], b"k")[4] == b"third"
    r = href.recover(CASES["e_flip_key"])
    assert r["cut"] == [0, 1, 0] and r["valid"] == [40, 17, 40] and 0 < r["size_after"][1] < len(CASES["e_flip_key"][1])
    assert any(s == 2 for s, _ in r["index"].values())
    r = href.recover(CASES["e_flip_size_eof"])
    assert r["cut"] == [0, 0, 0] and r["short_tail"] == [0, 1, 0] and r["valid"][1] == 17
    for name in ("f_short_header", "f_short_payload"):
        r = href.recover(CASES[name])
        assert r["cut"] == [0, 0, 0] and r["short_tail"] == [0, 0, 1] and r["size_after"][2] == len(CASES[name][2])
    for name in ("g_wrap_small", "g_wrap_one", "g_wrap_zero"):
        r = href.recover(CASES[name])
        assert r["cut"] == [0, 1, 0] and r["valid"][1] == 20 and b"after" not in r["index"]
    assert len(href.recover(CASES["c_one_key"])["index"]) == 1
    assert b"" in href.recover(CASES["b_lengths"])["index"]


def test_records_corrupted_after_the_build(seb):
    """One live record and one tombstone get a flipped bit after recover: exactly those keys turn ERROR with verify,
    and without it the live one is still FOUND (with the flipped byte) and the tombstone a MISS."""
    w = href.Writer()
    for i in range(50):
        w.put(b"c-%02d" % i, b"value-%d" % i)
    w.delete(b"c-07").delete(b"c-31")
    good = [w.bytes()]
    want = href.recover(good)
    h = host_recover(seb, good)
    hit = want["index"][b"c-20"][1] + href.HEADER + 4 + 2   # inside c-20's value
    tomb = want["index"][b"c-31"][1] + 6                    # inside the tombstone's timestamp
    bad = [href.flip(href.flip(good[0], hit, 5), tomb, 1)]
    h["pool"] = np.frombuffer(bad[0], np.uint8)
    keys = href.probes(want, np.random.default_rng(4))
    st = check_get(seb, h, bad, want["index"], keys, True, "corrupted")
    assert {keys[i] for i in np.nonzero(st == href.ERROR)[0]} == {b"c-20", b"c-31"}
    st = check_get(seb, h, bad, want["index"], keys, False, "corrupted")
    assert not (st == href.ERROR).any() and st[keys.index(b"c-20")] == href.FOUND and st[keys.index(b"c-31")] == href.MISS


def test_fixed_stride_keys_and_no_live_array(seb):
    """The fixed-stride seb_keys layout, and live == NULL meaning every record."""
    w = href.Writer()
    keys = [b"%016d" % i for i in range(100)]
    for k in keys[:80]:
        w.put(k, k[::-1])
    segs = [w.bytes()]
    want = href.recover(segs)
    pool, rec_off, *_ = seb.segs_scan(segs)
    st, rec, vloc, vlen, distinct = seb.hidx_lookup(pool, rec_off, None, np.frombuffer(b"".join(keys), np.uint8).reshape(100, 16))
    w_st, w_rec, w_vloc, w_vlen, _ = href.get_batch(segs, want["index"], keys)
    assert np.array_equal(st, w_st) and np.array_equal(rec, w_rec) and np.array_equal(vloc, w_vloc) and np.array_equal(vlen, w_vlen)
    assert distinct == 80


def test_refusals(seb):
    L = seb.lib()
    seg = np.frombuffer(CASES["a_65"][0], np.uint8)
    with pytest.raises(seb.SebError) as e:
        seb.seg_scan(seg, cap=64)
    assert e.value.code == -1 and "more than 64 records" in str(e.value)
    assert seb.seg_scan(seg, cap=65)[0].size == 65
    off = np.zeros(8, np.uint64)
    n, tail = C.c_uint64(0), C.c_int(0)
    assert L.seb_seg_scan(seg.ctypes.data, seg.size, 0, off.ctypes.data, 8, None, C.byref(tail)) == -1
    assert L.seb_seg_scan(seg.ctypes.data, seg.size, 0, off.ctypes.data, 8, C.byref(n), None) == -1
    assert L.seb_seg_scan(None, 5, 0, off.ctypes.data, 8, C.byref(n), C.byref(tail)) == -1
    pool, rec_off, first, base, size, _ = seb.segs_scan(CASES["e_flip_key"])
    for bad_first in ([1, 40, 80, 120], [0, 50, 40, int(first[-1])], [0, 40, 80, int(first[-1]) - 1]):
        with pytest.raises(seb.SebError) as e:
            seb.seg_verify(pool, rec_off, np.array(bad_first, np.uint64), base, size)
        assert e.value.code == -1 and "seg_first" in str(e.value)
    valid, after = np.zeros(3, np.uint64), np.zeros(3, np.uint64)
    args = (rec_off.ctypes.data, rec_off.size, first.ctypes.data, base.ctypes.data, size.ctypes.data, 3, None, valid.ctypes.data,
            after.ctypes.data, None)
    assert L.seb_seg_verify(pool.ctypes.data, 1 << 47, *args) == -1 and "2^47" in seb.last_error()
    assert L.seb_seg_verify(None, pool.size, *args) == -1
    assert L.seb_seg_verify(pool.ctypes.data, pool.size, *args[:7], None, *args[8:]) == -1
    assert L.seb_seg_verify(pool.ctypes.data, pool.size, *args) == 0  # ok and live are optional
    data, koff = href.key_lists([b"ab", b"c"])
    with pytest.raises(seb.SebError) as e:
        seb.hidx_lookup(pool, rec_off, None, (data, np.array([0, 3, 2], np.uint64)))
    assert e.value.code == -1 and "offsets decrease" in str(e.value)
    kb = seb.as_keys((data, koff))
    st = np.zeros(2, np.uint8)
    assert L.seb_hidx_lookup(pool.ctypes.data, pool.size, rec_off.ctypes.data, None, rec_off.size, kb.ref, 1, None, None, None,
                             None, None) == -1
    assert L.seb_hidx_lookup(pool.ctypes.data, 1 << 47, rec_off.ctypes.data, None, rec_off.size, kb.ref, 1, st.ctypes.data, None,
                             None, None, None) == -1
    assert L.seb_hidx_lookup(pool.ctypes.data, pool.size, rec_off.ctypes.data, None, rec_off.size, kb.ref, 1, st.ctypes.data, None,
                             None, None, None) == 0
    assert seb.dev_hidx_table_bytes(0) == 64 + 8 and seb.dev_hidx_table_bytes(2) == 64 + 8 * 4
    assert seb.dev_hidx_table_bytes(1000) == 64 + 8 * 2048 and seb.dev_hidx_table_bytes((1 << 40) + 1) == 0


def test_option_round_trip(seb):
    assert seb.get_option("hidx_hash_mask") == 0
    with seb.option("hidx_hash_mask", 3):
        assert seb.get_option("hidx_hash_mask") == 3
    assert seb.get_option("hidx_hash_mask") == 0
    with pytest.raises(seb.SebError):
        seb.set_option("hidx_hash_mask", -1)
