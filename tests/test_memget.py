"""CPU: the host half of the batched memtable lookup (include/seb_bloom.h, the memtable lookup group; DESIGN.md
5.14).  seb_runs_search equals memget_ref's restatement of MemTable.Get and of LSM.Get's memtable steps for
every key, in all six outputs: 1, 2 and 8 runs that share keys, a tombstone in run 0 over a value in run 1, an
empty run 0, no runs; Go string order on ORDER_KEYS; every key of a run with its neighbouring byte strings; a
replay's arrays as they are; the deleted-byte rule and non-zero first offsets; the refusals with their entry.

The library has a host form of the join (seb_get_join), so its truth table is tested here; the device form is
held to the same table in test_gpu_memget.py."""
import numpy as np
import pytest

import memget_ref as gref
import memtable_ref as mref


def host_runs(seb, arrays):
    return [seb.host_run(a[0], a[1], a[3], a[4], a[5]) for a in arrays]


def compare(seb, tables, probes, name="", leads=None):
    leads = leads or [(0, 0)] * len(tables)
    arrays = [gref.run_arrays(mt, kl, vl) for mt, (kl, vl) in zip(tables, leads)]
    got = seb.runs_search(probes, host_runs(seb, arrays))
    gref.assert_same(got, gref.expected(tables, probes, [vl for _, vl in leads]), name)
    return got


@pytest.mark.parametrize("sizes", [(1,), (40,), (300,), (200, 250), (1, 1), (0, 120), (50, 0)])
def test_random_runs(seb, sizes):
    rng = np.random.default_rng(sum(sizes) + len(sizes))
    tables = [gref.random_table(rng, n) for n in sizes]
    got = compare(seb, tables, gref.probes_for(tables), f"sizes={sizes}")
    if sizes == (200, 250):  # the runs share keys, and both kinds of answer come from both runs
        shared = set(tables[0].keys) & set(tables[1].keys)
        assert len(shared) > 5
        for r in (0, 1):
            assert {gref.FOUND, gref.TOMBSTONE} <= set(got[0][got[1] == r].tolist())
        assert (got[0] == gref.NONE).any()
    if sizes == (0, 120):  # an empty active memtable in front of a non-empty one
        assert set(got[1].tolist()) == {1, gref.NO_RUN}


def test_tombstone_in_run_0_hides_a_value_in_run_1(seb):
    active = gref.table_from_ops([(b"a", b"new", 9, 0), (b"k", b"", 11, 1), (b"z", b"", 12, 1)])
    frozen = gref.table_from_ops([(b"k", b"old-value", 3, 0), (b"m", b"only-here", 4, 0), (b"z", b"", 5, 1)])
    probes = [b"k", b"m", b"a", b"z", b"b", b""]
    got = compare(seb, [active, frozen], probes, "tombstone over value")
    assert got[0].tolist() == [gref.TOMBSTONE, gref.FOUND, gref.FOUND, gref.TOMBSTONE, gref.NONE, gref.NONE]
    assert got[1].tolist() == [0, 1, 0, 0, 0xFF, 0xFF] and got[2].tolist()[:4] == [1, 1, 0, 2]
    assert got[4].tolist() == [0, 9, 3, 0, 0, 0] and got[5].tolist() == [11, 4, 9, 12, 0, 0]
    # the other way round the value is returned
    got = compare(seb, [frozen, active], [b"k"], "value over tombstone")
    assert (got[0][0], got[1][0], got[4][0]) == (gref.FOUND, 0, 9)


def test_no_runs_and_eight_runs(seb):
    probes = [b"", b"a", b"ab"]
    got = seb.runs_search(probes, [])
    assert got[0].tolist() == [0, 0, 0] and got[1].tolist() == [0xFF] * 3 and got[2].tolist() == [gref.NO_ENTRY] * 3
    assert not got[3].any() and not got[4].any() and not got[5].any()
    rng = np.random.default_rng(8)
    tables = [gref.random_table(rng, 60) for _ in range(7)] + [gref.table_from_ops([(b"only-in-the-last", b"v", 1, 0)])]
    got = compare(seb, tables, gref.probes_for(tables), "8 runs")
    assert set(got[1].tolist()) == set(range(8)) | {gref.NO_RUN}
    with pytest.raises(seb.SebError) as ei:
        seb.runs_search(probes, host_runs(seb, [gref.run_arrays(t) for t in tables + tables[:1]]))
    assert ei.value.code == -1 and "runs" in str(ei.value)
    assert all(a.size == 0 for a in seb.runs_search([], host_runs(seb, [gref.run_arrays(tables[0])])))


def test_go_string_order(seb):
    """Ties in the first 16 and 40 bytes, the empty key, extensions: every ORDER_KEYS key against runs made of them."""
    ks = sorted(mref.ORDER_KEYS)
    even = gref.table_from_ops([(k, b"e%d" % i, i, i % 4 == 0) for i, k in enumerate(ks) if i % 2 == 0])
    every = gref.table_from_ops([(k, b"a%d" % i, 100 + i, i % 3 == 0) for i, k in enumerate(ks)])
    probes = gref.probes_for([every], extra=ks)
    got = compare(seb, [every], probes, "ORDER_KEYS")
    assert (got[0] != gref.NONE).sum() == len(ks) and got[0][probes.index(b"")] == gref.TOMBSTONE
    got = compare(seb, [even, every], probes, "ORDER_KEYS, two runs")
    assert sorted(probes[i] for i in np.nonzero(got[1] == 0)[0]) == ks[::2]
    assert sorted(probes[i] for i in np.nonzero(got[1] == 1)[0]) == ks[1::2]


def test_straight_from_a_replay(seb):
    """wal_replay_emit's six arrays wrapped as a seb_run, without any copy, give MemTable.Get for every key of the log."""
    recs = mref.random_log(np.random.default_rng(3), 900, max_key=60, max_val=80) + mref.order_log()
    image, off = mref.wal_image(recs)
    keys, koff, vals, voff, dele, seq, _ = seb.wal_replay_emit(image, off)
    run = seb.host_run(keys, koff, voff, dele, seq)
    assert run.keys == keys.ctypes.data and run.key_off == koff.ctypes.data and run.seq == seq.ctypes.data  # no copy
    mt, _ = mref.recover(mref.read_all(image))
    probes = sorted({r[0] for r in recs}) + [b"not-in-the-log", b"a\x00\x00\x00"]
    got = seb.runs_search(probes, [run])
    gref.assert_same(got, gref.expected([mt], probes), "replay")
    assert (got[0] == gref.TOMBSTONE).any() and (got[0] == gref.FOUND).sum() > 20
    for i in np.nonzero(got[0] == gref.FOUND)[0][:50]:  # the location is the value
        assert vals[int(got[3][i]):int(got[3][i]) + int(got[4][i])].tobytes() == mt.entries[int(got[2][i])][1]


def test_deleted_bytes_and_first_offsets(seb):
    """Any non-zero deleted byte counts as deleted: this is the builder's input rule (seb_sst_encode writes the
    flag of every non-zero byte), not the WAL's byte == 1 rule, which the replay has applied before it emits 1 or 0.
    key_off[0] and val_off[0] may be non-zero."""
    mt = gref.random_table(np.random.default_rng(5), 150)
    probes = gref.probes_for([mt])
    want = gref.expected([mt], probes, [9])
    assert (want[0] == gref.TOMBSTONE).sum() > 10
    for byte in (1, 2, 255):
        a = gref.run_arrays(mt, key_lead=5, val_lead=9, deleted_byte=byte)
        assert a[1][0] == 5 and a[3][0] == 9
        gref.assert_same(seb.runs_search(probes, host_runs(seb, [a])), want, f"deleted byte {byte}")
    a = gref.run_arrays(mt, key_lead=5, val_lead=9)
    got = seb.runs_search(probes, [seb.host_run(a[0], a[1], a[3], None, None)])  # no deleted array: none is; no seq: 0
    assert not (got[0] == gref.TOMBSTONE).any() and not got[5].any()
    assert np.array_equal(got[0] != gref.NONE, want[0] != gref.NONE) and np.array_equal(got[2], want[2])


def refused(seb, arrays, probes=(b"x",)):
    with pytest.raises(seb.SebError) as ei:
        seb.runs_search(list(probes), host_runs(seb, arrays))
    assert ei.value.code == -1
    return str(ei.value)


def test_refusals_name_the_entry(seb):
    good = gref.run_arrays(gref.random_table(np.random.default_rng(6), 300))
    assert len(good[4]) > 45
    tie = mref.P40 + b"tail"
    ks = [b"!", b"#", tie, tie, tie + b"x"]  # equal neighbours that tie beyond 40 bytes: entry 3
    mt = gref.table_from_ops([(k + bytes([i]), b"v", i, 0) for i, k in enumerate(ks)])
    a = list(gref.run_arrays(mt))
    a[0] = np.frombuffer(b"".join(ks), np.uint8)
    a[1] = np.cumsum([0] + [len(k) for k in ks]).astype(np.uint64)
    msg = refused(seb, [good, a])
    assert "run 1: entry 3 " in msg and "strictly" in msg
    ks = [b"a", b"c", b"b", b"a"]  # a decreasing pair: entry 2 (entry 3 decreases too; the first is named)
    b = list(gref.run_arrays(gref.table_from_ops([(k, b"v", 1, 0) for k in (b"1", b"2", b"3", b"4")])))
    b[0] = np.frombuffer(b"".join(ks), np.uint8)
    msg = refused(seb, [b])
    assert "run 0: entry 2 " in msg and "strictly" in msg
    c = [x.copy() for x in good]  # a key_off past key_bytes: the entry whose end it is
    c[1][41:] += np.uint64(c[0].size)
    msg = refused(seb, [good, good, c])
    assert "run 2: entry 40:" in msg and "key_off" in msg
    d = [x.copy() for x in good]  # key_off that decreases, and val_off that decreases
    d[1][7] = d[1][6] - 1
    msg = refused(seb, [d])
    assert "run 0: entry 6:" in msg and "key_off" in msg
    e = [x.copy() for x in good]
    e[3][30:] += 50
    e[3][33] = e[3][32] - 1
    msg = refused(seb, [e])
    assert "run 0: entry 32:" in msg and "val_off" in msg
    # a bad run is refused before any key is looked up, also for an empty batch
    with pytest.raises(seb.SebError):
        seb.runs_search([], host_runs(seb, [c]))


def test_join_truth_table(seb):
    mem, sst = np.meshgrid(np.arange(3, dtype=np.uint8), np.arange(3, dtype=np.uint8), indexing="ij")
    mem, sst = mem.reshape(-1), sst.reshape(-1)
    st, src = seb.get_join(mem, sst)
    for m, s, got, source in zip(mem.tolist(), sst.tolist(), st.tolist(), src.tolist()):
        if m == seb.MEM_FOUND:
            want = (seb.GET_FOUND, 0)
        elif m == seb.MEM_TOMBSTONE:  # also over GET_ERROR: the reference has returned before it reads any file
            want = (seb.GET_MISS, 0)
        else:
            want = (s, 1)
        assert (got, source) == want, (m, s)
    assert seb.get_join(np.zeros(0, np.uint8), np.zeros(0, np.uint8))[0].size == 0
