"""CPU: the host half of the hash index's write side (include/seb_bloom.h, "hash index, write side")
against hashwrite_ref's restatement: seb_seg_frame_plan / _emit give segment.append's bytes and the rotation's cuts,
seb_seg_compact gives compactSegments' image in log order with every size counter, recover() of the compacted store
answers every Get as before, seb_hidx_logical_size gives getLogicalSize.  Then each refusal, with guard bytes."""
import ctypes as C

import numpy as np
import pytest

import hashindex_ref as href
import hashwrite_ref as wref

CASES = href.cases()
FRAMES = wref.frame_cases()
TS = 1_777_000_123
CLEAN = sorted(n for n in CASES if n[0] in "abcd")
SHORT = sorted(n for n in CASES if n.startswith("f_short"))
BAD = sorted(n for n in CASES if n.startswith(("e_flip", "g_wrap")))


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_frame_matches_the_reference(seb, name):
    ops, lead, stride = FRAMES[name]
    keys, vals, val_off, deleted = wref.ops_arrays(ops, lead, stride)
    want, want_off = wref.frame(ops, TS)
    assert want == b"".join(href.record(k, b"" if v is None else v, TS) for k, v in ops)
    image, off, cuts = seb.seg_frame(keys, vals, val_off, deleted, TS)
    assert image.tobytes() == want and np.array_equal(off, want_off) and cuts.size == 0
    if not any(v is None for _, v in ops):
        image2, _, _ = seb.seg_frame(keys, vals, val_off, None, TS)
        assert image2.tobytes() == want
    lens = np.diff(want_off.astype(np.int64)).tolist()
    for limit in (1, 100, 4096):
        for active in (0, limit - 1, limit, limit + 1):
            w = wref.cuts(lens, active, limit)
            off, cuts, total = seb.seg_frame_plan(keys, val_off, deleted, active, limit)
            assert cuts.tolist() == w and total == len(want), (limit, active)
            if w:
                with pytest.raises(seb.SebError) as e:
                    seb.seg_frame_plan(keys, val_off, deleted, active, limit, cut_cap=len(w) - 1)
                assert e.value.code == -4 and str(len(w)) in str(e.value)


def test_cut_cap_too_small_reports_the_need_and_writes_nothing(seb):
    ops, lead, stride = FRAMES["offsets_65"]
    keys, _, val_off, deleted = wref.ops_arrays(ops, lead, stride)
    kb = seb.as_keys(keys)
    off = np.full(67, 0xA5A5A5A5A5A5A5A5, np.uint64)
    cut = np.full(66, 0xA5A5A5A5A5A5A5A5, np.uint64)
    total, ncuts = C.c_uint64(7), C.c_uint64(0)
    rc = seb.lib().seb_seg_frame_plan(kb.ref, val_off.ctypes.data, deleted.ctypes.data, 1, 1, off.ctypes.data, cut.ctypes.data, 64,
                                      C.byref(total), C.byref(ncuts))
    assert rc == -4 and ncuts.value == 65 and total.value == 7
    assert (off == 0xA5A5A5A5A5A5A5A5).all() and (cut == 0xA5A5A5A5A5A5A5A5).all()
    # cut == NULL only counts
    rc = seb.lib().seb_seg_frame_plan(kb.ref, val_off.ctypes.data, deleted.ctypes.data, 1, 1, None, None, 0, None, C.byref(ncuts))
    assert rc == 0 and ncuts.value == 65


def frame_raw(seb, kb, vals, val_off, deleted, guard=64):
    """plan then emit through the raw ABI with guard bytes round every output: (rc of the plan, rc of the emit)."""
    n = kb.n
    off = np.full(n + 1 + 2, 0x5C5C5C5C5C5C5C5C, np.uint64)
    cut = np.full(n + 2, 0x5C5C5C5C5C5C5C5C, np.uint64)
    image = np.full(4096 + 2 * guard, 0x5C, np.uint8)
    total, ncuts = C.c_uint64(0), C.c_uint64(0)
    L = seb.lib()
    rc1 = L.seb_seg_frame_plan(kb.ref, val_off.ctypes.data, None if deleted is None else deleted.ctypes.data, 0, 50,
                               off[1:].ctypes.data, cut[1:].ctypes.data, n, C.byref(total), C.byref(ncuts))
    msg1 = seb.last_error()
    rc2 = L.seb_seg_frame_emit(kb.ref, vals.ctypes.data, val_off.ctypes.data, None if deleted is None else deleted.ctypes.data, TS,
                               image[guard:].ctypes.data, 4096)
    assert (off == 0x5C5C5C5C5C5C5C5C).all() and (cut == 0x5C5C5C5C5C5C5C5C).all() and (image == 0x5C).all()
    return rc1, rc2, msg1


def test_frame_refusals_write_nothing(seb):
    vals = np.frombuffer(b"v" * 64, np.uint8)
    good_keys = [b"a", b"bb", b"ccc", b"dddd"]
    data, koff = href.key_lists(good_keys)
    voff = np.array([0, 4, 8, 12, 16], np.uint64)
    # an empty key: op 2 (Put refuses it)
    k2 = seb.as_keys((data, np.array([0, 1, 3, 3, 7], np.uint64)))
    rc1, rc2, msg = frame_raw(seb, k2, vals, voff, None)
    assert rc1 == -1 and rc2 == -1 and "op 2" in msg and "empty key" in msg
    # decreasing key offsets at op 1, and an empty key before it is named first
    k3 = seb.as_keys((data, np.array([0, 3, 2, 6, 10], np.uint64)))
    rc1, rc2, msg = frame_raw(seb, k3, vals, voff, None)
    assert rc1 == -1 and rc2 == -1 and "op 1" in msg
    k4 = seb.as_keys((data, np.array([0, 0, 2, 1, 10], np.uint64)))
    rc1, rc2, msg = frame_raw(seb, k4, vals, voff, None)
    assert rc1 == -1 and "op 0" in msg and "empty key" in msg
    # decreasing value offsets at op 3
    kb = seb.as_keys((data, koff))
    rc1, rc2, msg = frame_raw(seb, kb, vals, np.array([0, 4, 8, 12, 11], np.uint64), None)
    assert rc1 == -1 and rc2 == -1 and "op 3" in msg and "value" in msg
    # a key of 2^32 bytes, a value of 2^32 bytes (offsets only: no byte is read before the check)
    big = 1 << 32
    kbig = seb.as_keys((data, np.array([0, 1, 3, 3 + big, 7 + big], np.uint64)))
    rc1, rc2, msg = frame_raw(seb, kbig, vals, voff, None)
    assert rc1 == -1 and rc2 == -1 and "op 2" in msg and "key" in msg
    rc1, rc2, msg = frame_raw(seb, kb, vals, np.array([0, 4, 4 + big, 12 + big, 16 + big], np.uint64), None)
    assert rc1 == -1 and rc2 == -1 and "op 1" in msg and "value" in msg
    # keySize + valueSize >= 2^32 with each below it; a Delete of the same op counts no value and passes the plan
    half = 1 << 31
    khalf = seb.as_keys((data, np.array([0, 1, 1 + half, 2 + half, 3 + half], np.uint64)))
    vhalf = np.array([0, 4, 4 + half, 8 + half, 12 + half], np.uint64)
    rc1, rc2, msg = frame_raw(seb, khalf, vals, vhalf, None)
    assert rc1 == -1 and rc2 == -1 and "op 1" in msg and "keySize + valueSize" in msg
    total = C.c_uint64(0)
    assert seb.lib().seb_seg_frame_plan(khalf.ref, vhalf.ctypes.data, np.array([0, 1, 0, 0], np.uint8).ctypes.data, 0, 50, None,
                                        None, 0, C.byref(total), None) == 0
    assert total.value == 4 * 20 + (3 + half) + 12
    # limit 0, a null val_off, an image_bytes that is not the plan's
    assert seb.lib().seb_seg_frame_plan(kb.ref, voff.ctypes.data, None, 0, 0, None, None, 0, None, None) == -1
    assert "limit" in seb.last_error()
    assert seb.lib().seb_seg_frame_plan(kb.ref, None, None, 0, 5, None, None, 0, None, None) == -1
    image = np.zeros(200, np.uint8)
    assert seb.lib().seb_seg_frame_emit(kb.ref, vals.ctypes.data, voff.ctypes.data, None, TS, image.ctypes.data, 105) == -1
    assert "image_bytes" in seb.last_error() and not image.any()
    assert seb.lib().seb_seg_frame_emit(kb.ref, vals.ctypes.data, voff.ctypes.data, None, TS, image.ctypes.data, 106) == 0


def check_compaction(seb, segments, c, what):
    want = wref.compact(segments, c, TS)
    assert want is not None, what
    image, out_off, sizes = seb.segs_compact(segments, c, TS)
    assert image.tobytes() == want["image"], what
    assert np.array_equal(out_off, want["rec_off"]), what
    assert sizes == {k: want[k] for k in sizes}, what
    assert set(sizes) == {"records_in", "live_in", "distinct", "survivors", "tombstoned", "shadowed", "image_bytes"}
    # every Get answers the same before and after, and the count drops by applyCompaction's deletions
    before = href.recover(segments)
    keys = href.probes(before, np.random.default_rng(3))
    after_segments = [image.tobytes()] + list(segments[c:])
    assert wref.answers(after_segments, keys) == wref.answers(segments, keys), what
    after = href.recover(after_segments)
    assert len(before["index"]) - len(after["index"]) == wref.count_drop(segments, c), what
    # the library's own read side on the compacted store
    pool, rec_off, first, base, size, _ = seb.segs_scan(after_segments)
    live = seb.seg_verify(pool, rec_off, first, base, size)[3]
    st, _, vloc, vlen, distinct = seb.hidx_lookup(pool, rec_off, live, href.key_lists(keys))
    w_st = href.get_batch(after_segments, after["index"], keys)[0]
    assert np.array_equal(st, w_st) and distinct == len(after["index"]), what
    assert seb.hidx_logical_size(pool, rec_off, live) == wref.logical_size(after_segments, after["index"]), what
    return sizes


@pytest.mark.parametrize("name", CLEAN + SHORT)
def test_compaction_of_every_prefix(seb, name):
    segments = CASES[name]
    for c in range(1, len(segments) + 1):
        check_compaction(seb, segments, c, (name, c))


def test_the_short_tail_is_dropped_silently(seb):
    for name in SHORT:
        segments = CASES[name]
        c = len(segments)
        image, _, sizes = seb.segs_compact(segments, c, TS)
        rec = href.recover(segments)
        assert sizes["records_in"] == sum(rec["valid"]) and not any(rec["cut"]), name
    image, out_off, sizes = seb.segs_compact(CASES["f_only_a_tail"], 1, TS)
    assert image.size == 0 and out_off.tolist() == [0] and sizes["records_in"] == 0


@pytest.mark.parametrize("name", BAD)
def test_a_bad_record_aborts_only_where_its_segment_is_compacted(seb, name):
    segments = CASES[name]
    rec = href.recover(segments)
    check_compaction(seb, segments, 1, (name, 1))  # the bad segment is the middle one
    if any(rec["cut"]):
        for c in (2, 3):
            assert wref.compact(segments, c, TS) is None
            with pytest.raises(seb.SebError) as e:
                seb.segs_compact(segments, c, TS)
            assert e.value.code == -1 and "segment 1" in str(e.value) and f"record {rec['valid'][1]}" in str(e.value)
    else:  # e_flip_size_eof: the payload runs past the end of the file: io.EOF, silently
        for c in (2, 3):
            check_compaction(seb, segments, c, (name, c))


def test_every_key_deleted_gives_an_empty_image(seb):
    segments = wref.all_deleted()
    sizes = check_compaction(seb, segments, 2, "all deleted")
    assert sizes["survivors"] == 0 and sizes["image_bytes"] == 0 and sizes["tombstoned"] == 40 == sizes["distinct"]
    sizes = check_compaction(seb, segments, 1, "all deleted, first segment")
    assert sizes["survivors"] == 40  # the deletes are in the segment that stays


def test_winners_are_chosen_among_the_compacted_segments_only(seb):
    """d_put_delete_put: compacting the first segment alone still writes k = first, which the later Delete hides."""
    segments = CASES["d_put_delete_put"]
    image, _, sizes = seb.segs_compact(segments, 1, TS)
    assert href.record(b"k", b"first", TS) in image.tobytes() and sizes["survivors"] == 2
    image, _, sizes = seb.segs_compact(segments, 2, TS)
    assert b"first" not in image.tobytes() and sizes["tombstoned"] == 1 and sizes["shadowed"] == 1


def test_logical_size_against_the_dict(seb):
    for name in CLEAN + BAD:
        segments = CASES[name]
        rec = href.recover(segments)
        pool, rec_off, first, base, size, _ = seb.segs_scan(segments)
        live = seb.seg_verify(pool, rec_off, first, base, size)[3]
        assert seb.hidx_logical_size(pool, rec_off, live) == wref.logical_size(segments, rec["index"]), name


def test_compact_refusals_and_the_range_retry(seb):
    L = seb.lib()
    segments = CASES["a_65"]
    pool, rec_off, *_ = seb.segs_scan(segments)
    want = wref.compact(segments, 1, TS)
    for caps in ((want["image_bytes"] - 1, want["survivors"] + 1), (want["image_bytes"], want["survivors"])):
        with pytest.raises(seb.SebError) as e:
            seb.seg_compact(pool, rec_off, None, TS, caps=caps)
        assert e.value.code == -4 and e.value.sizes["image_bytes"] == want["image_bytes"]
        assert e.value.sizes["survivors"] == want["survivors"]
    image, out_off, _ = seb.seg_compact(pool, rec_off, None, TS, caps=(want["image_bytes"], want["survivors"] + 1))
    assert image.tobytes() == want["image"]
    # guard bytes: nothing outside the image and the offsets
    img = np.full(want["image_bytes"] + 32, 0x7E, np.uint8)
    out = np.full(want["survivors"] + 1 + 4, 0x7E7E7E7E7E7E7E7E, np.uint64)
    sz = seb.seb_segcompact_sizes()
    assert L.seb_seg_compact(pool.ctypes.data, pool.size, rec_off.ctypes.data, None, rec_off.size, TS, img[16:].ctypes.data,
                             want["image_bytes"], out[2:].ctypes.data, want["survivors"] + 1, C.byref(sz)) == 0
    assert (img[:16] == 0x7E).all() and (img[-16:] == 0x7E).all() and img[16:-16].tobytes() == want["image"]
    assert (out[:2] == 0x7E7E7E7E7E7E7E7E).all() and (out[-2:] == 0x7E7E7E7E7E7E7E7E).all()
    # a live record that does not lie inside the pool is named; one that is not live is not looked at
    off2 = rec_off.copy()
    off2[9] = pool.size - 5
    with pytest.raises(seb.SebError) as e:
        seb.seg_compact(pool, off2, None, TS)
    assert e.value.code == -1 and "record 9" in str(e.value)
    live = np.ones(rec_off.size, np.uint8)
    live[9] = 0
    assert seb.seg_compact(pool, off2, live, TS)[2]["live_in"] == rec_off.size - 1
    assert L.seb_seg_compact(pool.ctypes.data, pool.size, rec_off.ctypes.data, None, rec_off.size, TS, None, 0, None, 0, None) == -1
    assert L.seb_seg_compact(pool.ctypes.data, 1 << 47, rec_off.ctypes.data, None, rec_off.size, TS, None, 0, None, 0,
                             C.byref(sz)) == -1 and "2^47" in seb.last_error()
    assert L.seb_hidx_logical_size(pool.ctypes.data, pool.size, rec_off.ctypes.data, None, rec_off.size, None) == -1
    assert seb.dev_seg_compact_workspace_size(1 << 38) == 0 and seb.dev_seg_compact_workspace_size(1000) > 0
