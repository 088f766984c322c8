"""CPU: the host half of the WAL replay (seb_wal_replay_plan / seb_wal_replay_emit) against
memtable_ref's literal restatement of MemTable.Put / Delete / GetAllEntries and recoverFromWAL: the six arrays
and all eight sizes, the closed forms (one entry per key from its last record, memtable_size) held to the
restated arithmetic."""
import numpy as np
import pytest

import memtable_ref as mref
import scale_ref as sc


def replay(seb, records, image=None, off=None):
    if image is None:
        image, off = mref.wal_image(records)
    sizes = seb.wal_replay_plan(image, off)
    out = seb.wal_replay_emit(image, off)
    assert out[6] == sizes
    assert out[1][0] == 0 and out[3][0] == 0 and len(out[1]) == len(out[3]) == sizes[1] + 1
    return mref.unpack(*out[:6]), sizes


def check(seb, records, name=""):
    got, sizes = replay(seb, records)
    want, want_sizes = mref.expected(records)
    assert sizes == want_sizes, name
    assert got == want, name
    return got, sizes


@pytest.mark.parametrize("n", [0, 1, 2, 17, 300, 3000])
def test_random_logs(seb, n):
    rng = np.random.default_rng(n)
    recs = mref.random_log(rng, n)
    got, sizes = check(seb, recs, f"n={n}")
    if n >= 300:
        assert sizes[4] > n // 3 and sizes[5] > 0  # duplicates are common, tombstones survive
        assert any(f == 1 and v for _, v, _, f in recs)  # deleted records that carry value bytes
        assert len({k for k, _, _, _ in recs}) == sizes[1]
        ks = [k for k, _, _, _ in got]
        assert ks == sorted(ks)


def test_deleted_byte_and_value_of_a_delete(seb):
    recs = [(b"k0", b"v", 1, 0), (b"k1", b"carried", 2, 1), (b"k2", b"v2", 3, 2), (b"k3", b"v3", 4, 255)]
    got, sizes = check(seb, recs)
    assert got == [(b"k0", b"v", 0, 1), (b"k1", b"", 1, 2), (b"k2", b"v2", 0, 3), (b"k3", b"v3", 0, 4)]
    assert sizes == (4, 4, 8, 5, 0, 1, 4, 8 + 5 + 64)


def test_last_record_wins_whatever_its_sequence(seb):
    recs = [(b"a", b"first", 9000, 0), (b"b", b"x", 5, 0), (b"a", b"second", 7, 0), (b"b", b"", 6, 1), (b"c", b"", 1, 1),
            (b"c", b"back", 2, 0), (b"a", b"3", 3, 0)]
    got, sizes = check(seb, recs)
    assert got == [(b"a", b"3", 0, 3), (b"b", b"", 1, 6), (b"c", b"back", 0, 2)]
    assert sizes[6] == 9000 and sizes[4] == 4  # the largest seq is on an overwritten record


def test_empty_and_single(seb):
    assert check(seb, [])[1] == (0,) * 8
    assert check(seb, [(b"", b"", 0, 0)])[0] == [(b"", b"", 0, 0)]
    assert check(seb, [(b"", b"gone", 3, 1)])[1] == (1, 1, 0, 0, 0, 1, 3, 16)
    out = seb.wal_replay_emit(b"", [0])
    assert out[1].tolist() == [0] and out[6] == (0,) * 8


def test_go_string_order_and_prefix_ties(seb):
    got, sizes = check(seb, mref.order_log())
    ks = [k for k, _, _, _ in got]
    assert ks == sorted(mref.ORDER_KEYS) and ks[0] == b""
    at = ks.index(b"a")
    assert ks[at:at + 3] == [b"a", b"a\x00", b"a\x00\x00"]
    assert all(v.startswith(b"round2-") for _, v, _, _ in got) and sizes[4] == 2 * len(ks)


def test_one_large_key_and_value(seb):
    big = b"K" * 69_999
    recs = [(b"m", b"1", 1, 0), (big + b"b", b"x", 2, 0), (b"v", b"V" * 70_000, 3, 0), (big + b"a", b"y", 4, 0),
            (big + b"b", b"z", 5, 0), (b"v", b"", 6, 1), (b"w", b"W" * 70_000, 7, 0)]
    got, sizes = check(seb, recs)
    assert [k for k, _, _, _ in got] == [big + b"a", big + b"b", b"m", b"v", b"w"]
    assert got[1][1] == b"z" and got[3][1:3] == (b"", 1) and len(got[4][1]) == 70_000


def test_image_at_a_nonzero_first_offset(seb):
    recs = mref.random_log(np.random.default_rng(3), 200)
    image, off = mref.wal_image(recs)
    pad = b"\xEE" * 13
    out = seb.wal_replay_emit(pad + image + pad, [o + 13 for o in off])
    assert mref.unpack(*out[:6]) == mref.expected(recs)[0]


# ------------------------------------------------------------------ errors

def test_bad_framing_names_the_lowest_record(seb):
    recs = mref.random_log(np.random.default_rng(11), 50, max_val=60)
    image, off = mref.wal_image(recs)
    for bad in ([0], [17], [49], [30, 12, 44]):
        img = bytearray(image)
        for r in bad:
            img[off[r] + 12] ^= 1  # keySize off by one: 21 + keySize + valueSize != the record's length
        for call in (lambda: seb.wal_replay_plan(bytes(img), off), lambda: seb.wal_replay_emit(bytes(img), off, sizes=(50,) + (0,) * 7)):
            with pytest.raises(seb.SebError) as ei:
                call()
            assert ei.value.code == -1 and f"record {min(bad)} " in str(ei.value), str(ei.value)
    # a record shorter than a header, and one whose sizes overflow 32 bits when added
    short_off = off[:20] + [off[20] - 5] + [o for o in off[21:]]
    with pytest.raises(seb.SebError) as ei:
        seb.wal_replay_plan(image, short_off)
    assert ei.value.code == -1 and "record 19 " in str(ei.value)
    tiny = [0, 20]
    with pytest.raises(seb.SebError) as ei:
        seb.wal_replay_plan(bytes(20), tiny)
    assert ei.value.code == -1 and "record 0 " in str(ei.value)
    wrap = bytearray(mref.wal_record(b"abc", b"", 1, 0))
    wrap[12:16] = (0xFFFFFFFF).to_bytes(4, "little")
    wrap[16:20] = (4).to_bytes(4, "little")  # 21 + 0xFFFFFFFF + 4 wraps to 24 in 32 bits
    with pytest.raises(seb.SebError) as ei:
        seb.wal_replay_plan(bytes(wrap), [0, len(wrap)])
    assert ei.value.code == -1 and "record 0 " in str(ei.value)


def test_decreasing_offsets_are_refused(seb):
    recs = mref.random_log(np.random.default_rng(12), 30, max_val=60)
    image, off = mref.wal_image(recs)
    swapped = list(off)
    swapped[10], swapped[11] = swapped[11], swapped[10]
    with pytest.raises(seb.SebError) as ei:
        seb.wal_replay_plan(image, swapped)
    # record 9 now runs to record 11's start: its framing fails first, before record 10's offsets are met
    assert ei.value.code == -1 and "record 9 " in str(ei.value)
    first = [off[1] + 40] + list(off[1:])
    with pytest.raises(seb.SebError) as ei:
        seb.wal_replay_plan(image, first)
    assert ei.value.code == -1 and "record 0:" in str(ei.value) and "decreases" in str(ei.value)
    beyond = list(off)
    beyond[5] = off[-1] + 100  # leaves the image
    with pytest.raises(seb.SebError) as ei:
        seb.wal_replay_plan(image, beyond)
    assert ei.value.code == -1 and "record 4:" in str(ei.value)


def test_emit_refuses_other_sizes_and_writes_nothing_past_them(seb):
    recs = mref.random_log(np.random.default_rng(13), 120, max_val=80)
    image, off = mref.wal_image(recs)
    sizes = seb.wal_replay_plan(image, off)
    for j in (1, 2, 3, 5, 6, 7):
        bad = list(sizes)
        bad[j] -= 1
        with pytest.raises(seb.SebError) as ei:
            seb.wal_replay_emit(image, off, sizes=tuple(bad))
        assert ei.value.code == -1 and "plan" in str(ei.value)


# ------------------------------------------------------------------ the shapes of test_gpu_replay.py's scale tests

T = 1024


def check_arrays(out, want, sizes, name):
    assert out[6] == sizes, (name, out[6], sizes)
    for j, what in enumerate(("keys", "key_off", "vals", "val_off", "deleted", "seq")):
        assert np.array_equal(out[j], want[j]), (name, what)


@pytest.mark.parametrize("n,distinct", [(129 * T + 3, 50_000), (1024 * T + 1025, 400_000)])
def test_scale_logs_equal_the_closed_form(seb, n, distinct):
    """The host half on scale_ref.replay_log: the reference of the device's many-tile tests, held to numpy's lexsort."""
    image, off, want, sizes = sc.replay_log(n, distinct)
    assert sizes[0] == n and distinct // 2 < sizes[1] <= distinct and 0 < sizes[5] < sizes[1]
    assert seb.wal_replay_plan(image, off) == sizes
    check_arrays(seb.wal_replay_emit(image, off), want, sizes, f"n={n}")


def test_scale_log_is_a_wal_and_last_wins_is_the_memtable(seb):
    """The generators themselves at a size the literal restatement takes: replay_log's image parses as ReadAll
    parses it (CRCs included) and replays as recoverFromWAL does; last_wins equals memtable_ref.expected."""
    image, off, want, sizes = sc.replay_log(3 * T + 5, 700)
    recs = [(k, v, s, 1 if d else 0) for k, v, s, d in mref.read_all(image.tobytes())]
    assert len(recs) == 3 * T + 5
    assert (mref.unpack(*want), sizes) == mref.expected(recs) == sc.last_wins(recs)
    recs = mref.random_log(np.random.default_rng(5), 2000)
    assert sc.last_wins(recs) == mref.expected(recs)


@pytest.mark.parametrize("distinct", [0, 1], ids=["few_keys", "distinct_keys"])
@pytest.mark.parametrize("n", [8 * T + 1, 16 * T, 17 * T - 5, 33 * T + 1])
def test_deep_logs_equal_last_wins(seb, n, distinct):
    recs, image, off, want, sizes = sc.deep_log(n, distinct)
    out = seb.wal_replay_emit(image, off)
    assert out[6] == sizes and mref.unpack(*out[:6]) == want
    assert (sizes[1] > n // 2) == bool(distinct)
