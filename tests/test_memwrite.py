"""CPU: the host half of the memtable write side (include/seb_bloom.h, the memtable write side group; DESIGN.md
5.15) against memwrite_ref's restatement of LSM.Put / LSM.Delete.

The framed image is byte-identical to memtable_ref.wal_image of the records WAL.Append was called with; the image
read back (seb_wal_scan, the CRCs, seb_wal_replay_*) is the batch's run; fold([replay(Bk) .. replay(B1), old])
equals the MemTable after all ops in entries, values, flags, sequences and size, for 1, 2 and 8 runs; the size
deltas summed over the batches equal MemTable.size; every refusal names its op, run or entry."""
import numpy as np
import pytest

import memtable_ref as mref
import memwrite_ref as wref


def frame(seb, ops, first_seq=1, layout="varlen", deleted_byte=1):
    if layout == "fixed":
        keys, _, vals, voff, dele = wref.op_arrays(ops, 0, 7, deleted_byte)
        stride = len(ops[0][0])
        return seb.wal_frame(keys.reshape(-1, stride), vals, voff, dele, first_seq)
    keys, koff, vals, voff, dele = wref.op_arrays(ops, 5, 9, deleted_byte)
    return seb.wal_frame((keys, koff), vals, voff, dele, first_seq)


def replay(seb, image, off):
    """The batch's run through the host replay: (keys, key_off, vals, val_off, deleted, seq, sizes)."""
    return seb.wal_replay_emit(image, off)


def host_run(seb, a):
    return seb.host_run(a[0], a[1], a[3], a[4], a[5])


BATCHES = [("empty", []), ("one", [(b"k", b"v", 0)]), ("one delete", [(b"k", b"carried", 1)]), ("edge", wref.edge_ops())]


@pytest.mark.parametrize("first_seq", [1, (1 << 32) + 5, (1 << 63) + 11])
def test_image_is_wal_image(seb, first_seq):
    rng = np.random.default_rng(3)
    cases = BATCHES + [(f"random {n}", wref.random_ops(rng, n)) for n in (63, 300, 1025)]
    for name, ops in cases:
        want, want_off = mref.wal_image(wref.batch_records(ops, first_seq))
        for byte in (1, 2, 255):
            image, off = frame(seb, ops, first_seq, deleted_byte=byte)
            assert image.tobytes() == want, (name, byte)
            assert off.tolist() == want_off, (name, byte)
        plan_off, total = seb.wal_frame_plan((wref.op_arrays(ops)[0], wref.op_arrays(ops)[1]), wref.op_arrays(ops)[3],
                                             wref.op_arrays(ops)[4])
        assert total == len(want) and plan_off.tolist() == want_off
    # the writer itself: sequences continue from lsm.sequence
    lsm = wref.LSM(sequence=first_seq - 1)
    for ops in (wref.random_ops(rng, 40), wref.edge_ops()):
        seq0 = lsm.sequence + 1
        want, want_off, _ = lsm.apply(ops)
        image, off = frame(seb, ops, seq0)
        assert image.tobytes() == want and off.tolist() == want_off
    assert lsm.sequence == first_seq - 1 + 40 + len(wref.edge_ops())


def test_fixed_stride_keys_and_no_deleted_array(seb):
    rng = np.random.default_rng(4)
    for stride in (1, 16, 24):
        ops = [(bytes(rng.integers(97, 100, stride, dtype=np.uint8)), bytes(rng.integers(0, 256, int(rng.integers(0, 30)), dtype=np.uint8)),
                int(rng.random() < 0.2)) for _ in range(200)]
        image, off = frame(seb, ops, 77, layout="fixed")
        want, want_off = mref.wal_image(wref.batch_records(ops, 77))
        assert image.tobytes() == want and off.tolist() == want_off
        keys, koff, vals, voff, _ = wref.op_arrays(ops)
        image, _ = seb.wal_frame((keys, koff), vals, voff, None, 77)  # deleted == NULL: every op is a Put
        assert image.tobytes() == mref.wal_image(wref.batch_records([(k, v, 0) for k, v, _ in ops], 77))[0]


def test_the_image_reads_back_as_the_batchs_run(seb):
    rng = np.random.default_rng(5)
    for ops in (wref.edge_ops(), wref.random_ops(rng, 700), []):
        image, off = frame(seb, ops, 1000)
        scan_off, rc = seb.wal_scan(image.tobytes())
        assert rc == 0 and scan_off.tolist() == off.tolist()
        entries = mref.read_all(image.tobytes())  # asserts every record's CRC
        assert len(entries) == len(ops)
        got = replay(seb, image, off)
        lsm = wref.LSM(sequence=999)
        lsm.apply(ops)
        assert mref.unpack(*got[:6]) == wref.entries_of(lsm.mt)
        assert got[6][6] == (lsm.sequence if ops else 0) and got[6][7] == lsm.mt.size


def write_history(seb, rng, batches, per_batch=250, old_ops=400):
    """An old run and `batches` write batches on top of it: (the runs newest first, their tables newest first, the
    writer).  Each run is the host replay of its batch's framed image."""
    lsm = wref.LSM(sequence=50)
    runs, tables = [], []
    for b in range(batches + 1):
        ops = wref.random_ops(rng, old_ops if b == 0 else per_batch) + (wref.edge_ops() if b % 3 == 1 else [])
        seq0 = lsm.sequence + 1
        lsm.apply(ops)
        image, off = frame(seb, ops, seq0)
        runs.insert(0, replay(seb, image, off))
        tables.insert(0, mref.recover(mref.read_all(image.tobytes()))[0])
    return runs, tables, lsm


@pytest.mark.parametrize("num_runs", [1, 2, 8])
def test_fold_is_the_memtable_after_all_ops(seb, num_runs):
    rng = np.random.default_rng(num_runs)
    runs, tables, lsm = write_history(seb, rng, num_runs - 1)
    assert len(runs) == num_runs
    hruns, vals = [host_run(seb, a) for a in runs], [a[2] for a in runs]
    got = seb.runs_fold(hruns, vals)
    assert mref.unpack(*got[:6]) == wref.entries_of(lsm.mt)  # entries, values, flags, sequences
    want = wref.fold_sizes(tables)
    assert got[6] == want and got[6] == seb.runs_fold_plan(hruns, vals)
    assert got[6][7] == lsm.mt.size and got[6][6] == lsm.sequence
    assert mref.unpack(*got[:6]) == wref.entries_of(wref.fold(tables))  # the identity itself
    if num_runs > 1:
        assert got[6][4] > 0 and got[6][5] > 0  # something was shadowed, and tombstones stay
    assert got[1][0] == 0 and got[3][0] == 0


def test_fold_shapes(seb):
    rng = np.random.default_rng(9)
    assert seb.runs_fold([], [])[6] == (0,) * 8
    empty = replay(seb, *frame(seb, []))
    one = replay(seb, *frame(seb, [(b"", b"value-of-the-empty-key", 0)], 7))
    for arrays in ([empty], [empty, empty], [empty, one, empty], [one, one]):
        got = seb.runs_fold([host_run(seb, a) for a in arrays], [a[2] for a in arrays])
        n = 1 if any(a is one for a in arrays) else 0
        assert got[6][1] == n and got[6][0] == sum(a is one for a in arrays)
        if n:
            assert mref.unpack(*got[:6]) == [(b"", b"value-of-the-empty-key", 0, 7)]
    # identical runs: everything but run 0 is shadowed; a run without seq gives 0; a tombstone with value bytes
    # behind it comes out with no value
    a = list(replay(seb, *frame(seb, wref.random_ops(rng, 300), 1)))
    n = len(a[4])
    got = seb.runs_fold([host_run(seb, a)] * 3, [a[2]] * 3)
    assert got[6][:2] == (3 * n, n) and got[6][4] == 2 * n
    assert all(np.array_equal(x, y) for x, y in zip(got[:6], a[:6]))
    vlen = np.diff(a[3].astype(np.int64)) + 3  # every entry, tombstones included, carries 3 more value bytes
    voff = np.concatenate([[11], 11 + np.cumsum(vlen)]).astype(np.uint64)
    vals = np.full(int(voff[-1]), 0x77, np.uint8)
    for e in range(n):
        vals[int(voff[e]):int(voff[e]) + int(vlen[e]) - 3] = a[2][int(a[3][e]):int(a[3][e + 1])]
    got = seb.runs_fold([seb.host_run(a[0], a[1], voff, a[4], None)], [vals])
    dele = a[4].astype(bool)
    assert dele.any() and (np.diff(got[3].astype(np.int64))[dele] == 0).all()
    assert (np.diff(got[3].astype(np.int64))[~dele] == vlen[~dele]).all() and not got[5].any()
    assert got[6][6] == 0  # no run has sequences


def test_deltas_sum_to_the_memtable_size(seb):
    rng = np.random.default_rng(11)
    lsm = wref.LSM(sequence=1 << 33)
    active, total = [], 0  # the active memtable's runs, newest first
    for b in range(8):
        ops = wref.random_ops(rng, 200, dels=0.35) + (wref.edge_ops() if b in (2, 5) else [])
        seq0 = lsm.sequence + 1
        _, _, want = lsm.apply(ops)
        fresh = replay(seb, *frame(seb, ops, seq0))
        got = seb.run_size_delta(host_run(seb, fresh), [host_run(seb, a) for a in active])
        assert got == want, (b, got, want)
        total += got
        active.insert(0, fresh)
        assert total == lsm.mt.size
    assert len(active) == 8
    # the cases by name: a value over a tombstone, a tombstone over a value, a key only the last run holds, and a
    # negative total
    old = [replay(seb, *frame(seb, [(b"t", b"", 1), (b"v", b"0123456789", 0)], 1)),
           replay(seb, *frame(seb, [(b"t", b"hidden", 0)], 3)),
           replay(seb, *frame(seb, [(b"last", b"abcdefgh", 0)], 4))]
    fresh = replay(seb, *frame(seb, [(b"t", b"xyz", 0), (b"v", b"", 1), (b"last", b"", 0), (b"new", b"12", 0)], 5))
    assert seb.run_size_delta(host_run(seb, fresh), [host_run(seb, a) for a in old]) == 3 - 10 - 8 + (3 + 16 + 2)
    fresh = replay(seb, *frame(seb, [(b"v", b"", 1), (b"last", b"", 1)], 9))
    assert seb.run_size_delta(host_run(seb, fresh), [host_run(seb, a) for a in old]) == -18
    assert seb.run_size_delta(host_run(seb, fresh), []) == 1 + 16 + 4 + 16  # no runs: the run's own size


def test_frame_refusals_name_the_op(seb):
    n = 40
    koff = (np.arange(n + 1, dtype=np.uint64) * np.uint64(3))
    voff = (np.arange(n + 1, dtype=np.uint64) * np.uint64(5))
    keys, vals = np.zeros(3 * n, np.uint8), np.zeros(5 * n, np.uint8)
    seb.wal_frame_plan((keys, koff), voff)
    for what, op, word in (("key", 17, "key"), ("val", 9, "value")):
        for kind in ("decrease", "huge"):
            k, v = koff.copy(), voff.copy()
            a = k if what == "key" else v
            if kind == "decrease":
                a[op + 1] = a[op] - np.uint64(1)
            else:
                a[op + 1:] += np.uint64(1 << 32)
            a[36] = a[35] - np.uint64(1)  # a later offender: not the one named
            with pytest.raises(seb.SebError) as ei:
                seb.wal_frame_plan((keys, k), v)  # the plan reads offsets alone
            assert ei.value.code == -1 and f"op {op}:" in str(ei.value) and word in str(ei.value), str(ei.value)
    k, v = koff.copy(), voff.copy()
    k[31], v[12] = k[30] - np.uint64(1), v[11] - np.uint64(1)  # both kinds: the lower op is named
    with pytest.raises(seb.SebError) as ei:
        seb.wal_frame_plan((keys, k), v)
    assert "op 11:" in str(ei.value) and "value" in str(ei.value)
    k = koff.copy()
    k[6] = k[5] - np.uint64(1)
    with pytest.raises(seb.SebError) as ei:
        seb.wal_frame((keys, k), vals, voff, None, 1)
    assert "op 5:" in str(ei.value)
    kb = seb.as_keys((keys, koff))
    image = np.zeros(21 * n + 8 * n, np.uint8)
    rc = seb.lib().seb_wal_frame_emit(kb.ref, vals.ctypes.data, voff.ctypes.data, None, 1, image.ctypes.data, image.size - 1)
    assert rc == -1 and "plan" in seb.last_error()
    assert seb.lib().seb_wal_frame_emit(kb.ref, vals.ctypes.data, voff.ctypes.data, None, 1, image.ctypes.data, image.size) == 0
    assert seb.lib().seb_wal_frame_plan(kb.ref, None, None, None, None) == -1


def test_run_refusals_name_the_run_and_entry(seb):
    rng = np.random.default_rng(13)
    good = list(replay(seb, *frame(seb, wref.random_ops(rng, 300), 1)))
    assert len(good[4]) > 45
    bad = (np.frombuffer(b"acba", np.uint8), np.arange(5, dtype=np.uint64), None, np.zeros(5, np.uint64), np.zeros(4, np.uint8), None)
    hg, hb = host_run(seb, good), host_run(seb, bad)
    with pytest.raises(seb.SebError) as ei:
        seb.run_size_delta(hg, [hg, hb])
    assert ei.value.code == -1 and "run 1: entry 2 " in str(ei.value)
    with pytest.raises(seb.SebError) as ei:
        seb.run_size_delta(hb, [hg, hg])
    assert ei.value.code == -1 and "the new run: entry 2 " in str(ei.value)
    with pytest.raises(seb.SebError) as ei:
        seb.run_size_delta(hg, [hg] * 8)  # the new run is the eighth
    assert ei.value.code == -1
    with pytest.raises(seb.SebError) as ei:
        seb.runs_fold_plan([hg, hg, hb], [good[2]] * 3)
    assert ei.value.code == -1 and "run 2: entry 2 " in str(ei.value)
    with pytest.raises(seb.SebError) as ei:
        seb.runs_fold_plan([hg, hg], [good[2], good[2][:-1]])
    assert ei.value.code == -1 and "run 1: val_off[n]" in str(ei.value)
    with pytest.raises(seb.SebError) as ei:
        seb.runs_fold_plan([hg] * 9, [good[2]] * 9)
    assert ei.value.code == -1
    sizes = list(seb.runs_fold_plan([hg], [good[2]]))
    sizes[2] += 1
    with pytest.raises(seb.SebError) as ei:
        seb.runs_fold([hg], [good[2]], sizes=tuple(sizes))
    assert ei.value.code == -1 and "plan" in str(ei.value)
