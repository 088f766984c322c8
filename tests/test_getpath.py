"""CPU: the host half of the Get path (seb_get_compact, seb_get_join_rows) against getpath_ref's restatement:
every key layout, decided fractions 0, all and mixed, status bytes 3 and 255 (undecided), empty keys, n == 0, the
SEB_ERR_RANGE retry, each refusal, the join's full truth table and its three bad-row rules."""
import ctypes as C

import numpy as np
import pytest

import getpath_ref as pref

RNG = np.random.default_rng(16)


def fixed_batch(n, stride):
    return [bytes(RNG.integers(0, 256, stride, dtype=np.uint8)) for _ in range(n)]


def varlen_batch(n, max_len=40):
    return [bytes(RNG.integers(0, 256, int(RNG.integers(0, max_len + 1)), dtype=np.uint8)) for _ in range(n)]


def as_fixed(keys, stride):
    return np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), stride).copy()


def as_varlen(keys, lead=0):
    off = np.zeros(len(keys) + 1, np.uint64)
    np.cumsum([len(k) for k in keys], out=off[1:])
    data = np.frombuffer(b"\xee" * lead + b"".join(keys) + b"\xee" * 3, np.uint8).copy()
    return data, off + np.uint64(lead)


def statuses(n):
    """[(name, mem_status)]: decided fractions 0, all and mixed, and the bytes that are no seb_mem_status."""
    out = [("none", np.zeros(n, np.uint8)), ("all", np.where(np.arange(n) % 2, 1, 2).astype(np.uint8)),
           ("alternating", (np.arange(n) % 2).astype(np.uint8)),
           ("mixed", RNG.choice(np.array([0, 1, 2], np.uint8), n)),
           ("odd bytes", RNG.choice(np.array([0, 1, 2, 3, 255], np.uint8), n))]
    return out


def check_compact(seb, keys, batch, mem, stride, name):
    want = pref.compact_arrays(keys, mem, stride)
    got = seb.get_compact(batch, mem)
    assert got[0] == want[0], name
    assert np.array_equal(got[1], want[1]), name
    assert (got[2] is None) == (want[2] is None), name
    if want[2] is not None:
        assert np.array_equal(got[2], want[2]) and got[2][0] == 0, name
    assert np.array_equal(got[3], want[3]) and got[3].dtype == np.uint32, name
    assert np.all(np.diff(got[3].astype(np.int64)) > 0), name


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257, 1025])
def test_compact_every_layout(seb, n):
    for stride in (16, 5, 24, 1):
        keys = fixed_batch(n, stride)
        for name, mem in statuses(n):
            if n:
                check_compact(seb, keys, as_fixed(keys, stride), mem, stride, f"stride {stride}, {name}")
    for lead in (0, 7):
        keys = varlen_batch(n)
        for name, mem in statuses(n):
            check_compact(seb, keys, as_varlen(keys, lead), mem, None, f"offsets, lead {lead}, {name}")


def test_status_bytes_3_and_255_are_undecided(seb):
    keys = fixed_batch(6, 16)
    mem = np.array([3, 1, 255, 2, 0, 128], np.uint8)
    sizes, _, off, row = seb.get_compact(as_fixed(keys, 16), mem)
    assert sizes == (6, 4, 64) and off is None and row.tolist() == [0, 2, 4, 5]


def test_empty_keys(seb):
    """A batch of empty keys only, and empty keys among others: an empty key is a key like any other."""
    keys = [b""] * 5
    mem = np.array([0, 1, 0, 2, 0], np.uint8)
    sizes, data, off, row = seb.get_compact(as_varlen(keys), mem)
    assert sizes == (5, 3, 0) and data.size == 0 and off.tolist() == [0, 0, 0, 0] and row.tolist() == [0, 2, 4]
    keys = [b"", b"ab", b"", b"", b"c", b""]
    for name, mem in statuses(len(keys)):
        check_compact(seb, keys, as_varlen(keys, 3), mem, None, name)
    # fixed stride 0: n keys of no bytes and no data pointer
    kb = seb.HostKeys(np.zeros((4, 0), np.uint8))
    sizes, data, off, row = seb.get_compact(kb, np.array([0, 1, 0, 0], np.uint8))
    assert sizes == (4, 3, 0) and off is None and row.tolist() == [0, 2, 3]


def test_n_zero(seb):
    sizes, data, off, row = seb.get_compact(np.zeros((0, 16), np.uint8), np.zeros(0, np.uint8))
    assert sizes == (0, 0, 0) and data.size == 0 and off is None and row.size == 0
    sizes, data, off, row = seb.get_compact((np.zeros(0, np.uint8), np.zeros(1, np.uint64)), np.zeros(0, np.uint8))
    assert sizes == (0, 0, 0) and off.tolist() == [0] and row.size == 0
    st, src, col, vloc, vlen = seb.get_join_rows(np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint8))
    assert st.size == src.size == col.size == vloc.size == vlen.size == 0


def test_range_retry(seb):
    """A cap below its size: SEB_ERR_RANGE, *sizes filled for the retry, and nothing written."""
    keys = varlen_batch(50)
    data, off = as_varlen(keys, 2)
    mem = (np.arange(50) % 3 == 0).astype(np.uint8)
    want = pref.compact_arrays(keys, mem)
    (_, m, kbytes) = want[0]
    for caps in ((kbytes - 1, m), (kbytes, m - 1), (0, 0)):
        with pytest.raises(seb.SebError) as e:
            seb.get_compact((data, off), mem, caps=caps)
        assert e.value.code == -4 and e.value.sizes == want[0]
    got = seb.get_compact((data, off), mem, caps=(kbytes, m))
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])
    # nothing is written by the refused call: the raw ABI on guarded buffers
    kb = seb.as_keys((data, off))
    out_keys, out_off, row = np.full(kbytes, 0xA5, np.uint8), np.full(m + 1, 7, np.uint64), np.full(m, 9, np.uint32)
    sz = seb.seb_compact_sizes()
    rc = seb.lib().seb_get_compact(kb.ref, mem.ctypes.data, C.byref(sz), out_keys.ctypes.data, kbytes, out_off.ctypes.data,
                                   row.ctypes.data, m - 1)
    assert rc == -4 and sz.as_tuple() == want[0]
    assert np.all(out_keys == 0xA5) and np.all(out_off == 7) and np.all(row == 9)
    # larger caps than needed are fine and write no more than the sizes say
    big = seb.get_compact((data, off), mem, caps=(kbytes + 9, m + 3))
    assert big[0] == want[0] and np.array_equal(big[3], want[3])


def test_refusals(seb):
    L = seb.lib()
    keys = fixed_batch(4, 16)
    kb = seb.as_keys(as_fixed(keys, 16))
    mem = np.zeros(4, np.uint8)
    sz = seb.seb_compact_sizes()
    row, out = np.zeros(4, np.uint32), np.zeros(64, np.uint8)
    args = (out.ctypes.data, 64, None, row.ctypes.data, 4)
    assert L.seb_get_compact(kb.ref, mem.ctypes.data, C.byref(sz), *args) == 0
    assert L.seb_get_compact(None, mem.ctypes.data, C.byref(sz), *args) == -1               # null keys
    assert L.seb_get_compact(kb.ref, None, C.byref(sz), *args) == -1                        # null mem_status
    assert L.seb_get_compact(kb.ref, mem.ctypes.data, None, *args) == -1                    # null sizes
    assert L.seb_get_compact(kb.ref, mem.ctypes.data, C.byref(sz), out.ctypes.data, 64, None, None, 4) == -1  # null row
    assert L.seb_get_compact(kb.ref, mem.ctypes.data, C.byref(sz), None, 64, None, row.ctypes.data, 4) == -1  # null out_keys
    big = seb.seb_keys(kb._s.data, None, 2**32, 16, 0)
    assert L.seb_get_compact(C.byref(big), mem.ctypes.data, C.byref(sz), None, 0, None, None, 0) == -1  # n >= 2^32
    assert "2^32" in seb.last_error()
    bad = seb.seb_keys(kb._s.data, None, 4, 16, 1)
    assert L.seb_get_compact(C.byref(bad), mem.ctypes.data, C.byref(sz), *args) == -1       # reserved != 0
    # a batch with offsets needs out_off; offsets that decrease are refused and name the key
    data, off = as_varlen([b"ab", b"c", b"def"])
    vk = seb.as_keys((data, off))
    mem3 = np.zeros(3, np.uint8)
    assert L.seb_get_compact(vk.ref, mem3.ctypes.data, C.byref(sz), out.ctypes.data, 64, None, row.ctypes.data, 4) == -1
    off2 = off.copy()
    off2[2] = off2[1] - 1
    dk = seb.as_keys((data, off2))
    assert L.seb_get_compact(dk.ref, mem3.ctypes.data, C.byref(sz), None, 0, None, None, 0) == -1
    assert "offsets decrease at 1" in seb.last_error()
    # the join: required pointers, n >= 2^32
    st = np.zeros(4, np.uint8)
    r2, ss = np.zeros(2, np.uint32), np.zeros(2, np.uint8)
    j = lambda mem_p, row_p, ss_p, st_p, n=4, m=2: L.seb_get_join_rows(mem_p, None, None, n, row_p, m, ss_p, None, None, None,  # noqa: E731
                                                                       st_p, None, None, None, None)
    assert j(mem.ctypes.data, r2.ctypes.data, ss.ctypes.data, st.ctypes.data) == 0
    assert j(None, r2.ctypes.data, ss.ctypes.data, st.ctypes.data) == -1
    assert j(mem.ctypes.data, None, ss.ctypes.data, st.ctypes.data) == -1
    assert j(mem.ctypes.data, r2.ctypes.data, None, st.ctypes.data) == -1
    assert j(mem.ctypes.data, r2.ctypes.data, ss.ctypes.data, None) == -1
    assert j(mem.ctypes.data, r2.ctypes.data, ss.ctypes.data, st.ctypes.data, n=2**32) == -1
    assert j(mem.ctypes.data, None, None, st.ctypes.data, m=0) == 0                         # m == 0 needs no row


def test_join_truth_table(seb):
    """3 memtable statuses x 3 SSTable statuses, every output, with and without the nullable inputs."""
    mem, sst = (x.reshape(-1).astype(np.uint8) for x in np.meshgrid(np.arange(3), np.arange(3), indexing="ij"))
    n = mem.size
    _, row = pref.compact([b""] * n, mem)
    m = row.size
    assert m == 3
    sst_m = sst[row]
    mem_vloc, mem_vlen = np.arange(1000, 1000 + n, dtype=np.uint64), np.arange(10, 10 + n, dtype=np.uint32)
    sst_col = np.arange(m, dtype=np.uint16)
    sst_vloc, sst_vlen = np.arange(5000, 5000 + m, dtype=np.uint64), np.arange(70, 70 + m, dtype=np.uint32)
    full = dict(mem_vloc=mem_vloc, mem_vlen=mem_vlen, sst_col=sst_col, sst_vloc=sst_vloc, sst_vlen=sst_vlen)
    got = seb.get_join_rows(mem, row, sst_m, **full)
    pref.assert_same(got, pref.join_rows(mem, row, sst_m, **full), "truth table")
    for i in range(n):
        ms, ss = int(mem[i]), int(sst[i])
        want = (1, 0) if ms == 1 else (0, 0) if ms == 2 else (ss, 1)
        assert (got[0][i], got[1][i]) == want, (ms, ss)
    # on status and source it is seb_get_join over the whole batch's sst_status
    st, src = seb.get_join(mem, sst)
    assert np.array_equal(got[0], st) and np.array_equal(got[1], src)
    for drop in full:
        part = {k: v for k, v in full.items() if k != drop}
        pref.assert_same(seb.get_join_rows(mem, row, sst_m, **part), pref.join_rows(mem, row, sst_m, **part), f"without {drop}")
    pref.assert_same(seb.get_join_rows(mem, row, sst_m), pref.join_rows(mem, row, sst_m), "status alone")


def test_join_bad_rows(seb):
    mem = np.array([0, 1, 0, 2, 3, 0], np.uint8)
    mem_vloc, mem_vlen = np.arange(6, dtype=np.uint64) + 100, np.arange(6, dtype=np.uint32) + 7
    # an undecided key that no row names: a miss from the SSTables
    row = np.array([0, 5], np.uint32)
    args = dict(mem_vloc=mem_vloc, mem_vlen=mem_vlen, sst_col=np.array([1, 2], np.uint16),
                sst_vloc=np.array([11, 12], np.uint64), sst_vlen=np.array([3, 4], np.uint32))
    got = seb.get_join_rows(mem, row, np.array([1, 2], np.uint8), **args)
    pref.assert_same(got, pref.join_rows(mem, row, np.array([1, 2], np.uint8), **args), "unnamed keys")
    for i in (2, 4):
        assert [int(g[i]) for g in got] == [0, 1, 0xFFFF, 0, 0]
    # a row outside the batch and rows naming decided keys are ignored
    row = np.array([1, 3, 6, 2**32 - 1, 2], np.uint32)
    sst = np.array([2, 1, 1, 1, 1], np.uint8)
    args = dict(mem_vloc=mem_vloc, mem_vlen=mem_vlen, sst_col=np.arange(5, dtype=np.uint16),
                sst_vloc=np.arange(5, dtype=np.uint64) + 50, sst_vlen=np.arange(5, dtype=np.uint32) + 60)
    got = seb.get_join_rows(mem, row, sst, **args)
    pref.assert_same(got, pref.join_rows(mem, row, sst, **args), "ignored rows")
    assert [int(g[1]) for g in got] == [1, 0, 0xFFFF, 101, 8]       # the memtable's found stands
    assert [int(g[3]) for g in got] == [0, 0, 0xFFFF, 0, 0]          # and so does its tombstone
    assert [int(g[2]) for g in got] == [1, 1, 4, 54, 64]
    # duplicate rows: one of them wins, nothing else is touched
    row = np.array([2, 2], np.uint32)
    got = seb.get_join_rows(mem, row, np.array([1, 2], np.uint8), sst_col=np.array([8, 9], np.uint16))
    assert (int(got[0][2]), int(got[2][2])) in ((1, 8), (2, 9))
    assert [int(got[0][i]) for i in (0, 1, 3, 4, 5)] == [0, 1, 0, 0, 0]
