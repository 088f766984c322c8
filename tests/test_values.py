"""CPU: seb_get_values, the host half of the Get path's last step (the found values gathered into one dense
buffer), held to values_ref's restatement of the semantics: sizes, out_off, out_vals and the lowest invalid key."""
import ctypes as C

import numpy as np
import pytest

import values_ref as vref

INVALID, RANGE = -1, -4


def check_batch(seb, b, what=""):
    args = vref.batch_args(b)
    vref.assert_same(seb.get_values(*args), vref.values(*args), what)


@pytest.mark.parametrize("kind", ["memtable", "pool", "mixed", "runs8"])
@pytest.mark.parametrize("n", [1, 2, 63, 300])
def test_sources(seb, kind, n):
    rng = np.random.default_rng(100 + n)
    kw = dict(memtable=dict(num_runs=1, runs_only=True), pool=dict(num_runs=0, pool_only=True), mixed=dict(num_runs=2),
              runs8=dict(num_runs=8))[kind]
    b = vref.make_batch(rng, n, lengths=(0, 1, 15, 16, 17, 4083), **kw)
    check_batch(seb, b, f"{kind} n={n}")
    if kind == "runs8" and n == 300:
        assert set(b["run"][(b["status"] == 1) & (b["source"] == 0)]) == set(range(8))


def test_only_found_carries_whatever_the_other_keys_hold(seb):
    """Status bytes 0, 2, 3 and 255 with garbage vloc / vlen / source / run contribute nothing."""
    rng = np.random.default_rng(5)
    b = vref.make_batch(rng, 200, found=np.zeros(200, bool))
    for k, st in enumerate((0, 2, 3, 255)):
        b["status"][k::4] = st
    sizes, out_off, out_vals = seb.get_values(*vref.batch_args(b))
    assert sizes == (200, 0, 0) and not out_off.any() and out_vals.size == 0
    b["status"][[3, 77, 199]] = 1  # three carrying keys among them
    for i, (src, ln) in zip((3, 77, 199), ((0, 5), (1, 0), (1, 17))):
        b["source"][i], b["run"][i], b["vloc"][i], b["vlen"][i] = src, 1, 40 + i, ln
    check_batch(seb, b)
    assert seb.get_values(*vref.batch_args(b))[0] == (200, 3, 22)


def test_every_length_and_the_exact_ends(seb):
    rng = np.random.default_rng(6)
    vals = [rng.integers(0, 256, 5000, dtype=np.uint8), rng.integers(0, 256, 4083, dtype=np.uint8)]
    pool = rng.integers(0, 256, 2 * 4096, dtype=np.uint8)
    lens = [0, 1, 15, 16, 17, 4083]
    rows = []  # (source, run, vloc, vlen)
    for ln in lens:
        rows.append((0, 0, 5000 - ln, ln))      # ends exactly at val_bytes[0]
        rows.append((0, 1, 4083 - ln, ln))      # the whole of run 1 for 4083
        rows.append((1, 7, 8192 - ln, ln))      # ends exactly at pool_bytes
        rows.append((1, 0, 4090, ln))           # a pool value across a block boundary is not re-checked
        rows.append((0, 0, 0, ln))
    rows += [(0, 0, 5000, 0), (1, 0, 8192, 0)]  # an empty value at the very end of its source
    n = len(rows)
    src, run, vloc, vlen = (np.array(c, t) for c, t in zip(zip(*rows), (np.uint8, np.uint8, np.uint64, np.uint32)))
    status = np.ones(n, np.uint8)
    args = (status, src, run, vloc, vlen, vals, pool)
    vref.assert_same(seb.get_values(*args), vref.values(*args))


def test_empty_batch_and_no_sources(seb):
    e8, e32, e64 = np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint64)
    sizes, out_off, out_vals = seb.get_values(e8, e8, e8, e64, e32)
    assert sizes == (0, 0, 0) and list(out_off) == [0] and out_vals.size == 0
    # num_runs == 0 and no pool, with no carrying key: valid
    st = np.array([0, 2, 0], np.uint8)
    sizes, out_off, _ = seb.get_values(st, st, None, np.zeros(3, np.uint64), np.zeros(3, np.uint32))
    assert sizes == (3, 0, 0) and list(out_off) == [0, 0, 0, 0]
    # a found key of no bytes in an empty pool: valid (0 <= 0 and 0 <= 0 - 0)
    one = np.ones(1, np.uint8)
    assert seb.get_values(one, one, None, np.zeros(1, np.uint64), np.zeros(1, np.uint32))[0] == (1, 1, 0)


def test_sizes_only_and_the_range_retry(seb):
    rng = np.random.default_rng(8)
    b = vref.make_batch(rng, 120, num_runs=3)
    args = vref.batch_args(b)
    want = vref.values(*args)
    n, found, total = want[0]
    assert total > 16
    L = seb.lib()
    st, so, rn, vl, vn = (np.ascontiguousarray(a) for a in args[:5])
    vp = (C.c_void_p * 3)(*[v.ctypes.data for v in b["vals"]])
    vb = (C.c_uint64 * 3)(*[v.size for v in b["vals"]])
    common = (st.ctypes.data, so.ctypes.data, rn.ctypes.data, vl.ctypes.data, vn.ctypes.data, n, vp, vb, 3,
              b["pool"].ctypes.data, b["pool"].size)
    sz = seb.seb_values_sizes()
    assert L.seb_get_values(*common, C.byref(sz), None, None, 0) == 0  # both outputs null: sizes only
    assert sz.as_tuple() == (n, found, total) and sz.reserved == 0
    out_off = np.full(n + 1, 0xA5A5A5A5A5A5A5A5, np.uint64)
    out_vals = np.full(total, 0xA5, np.uint8)
    for cap in (total - 1, 0):
        sz = seb.seb_values_sizes()
        assert L.seb_get_values(*common, C.byref(sz), out_off.ctypes.data, out_vals.ctypes.data, cap) == RANGE
        assert sz.as_tuple() == (n, found, total)  # filled for the retry
        assert (out_off == 0xA5A5A5A5A5A5A5A5).all() and (out_vals == 0xA5).all()  # nothing written
    assert L.seb_get_values(*common, C.byref(sz), out_off.ctypes.data, out_vals.ctypes.data, total) == 0
    vref.assert_same((sz.as_tuple(), out_off, out_vals), want)
    with pytest.raises(seb.SebError) as e:
        seb.get_values(*args, val_cap=total - 1)
    assert e.value.code == RANGE and e.value.sizes == (n, found, total)
    vref.assert_same(seb.get_values(*args, val_cap=total + 9), want)
    # out_off alone null with a cap: a required pointer is missing
    assert L.seb_get_values(*common, C.byref(sz), None, out_vals.ctypes.data, total) == INVALID


def test_run_null_with_one_run(seb):
    rng = np.random.default_rng(9)
    b = vref.make_batch(rng, 90, num_runs=1)
    b["run"][:] = 0
    args = list(vref.batch_args(b))
    want = vref.values(*args)
    args[2] = None
    vref.assert_same(seb.get_values(*args), want)
    # with two runs a null run array is a missing argument
    b2 = vref.make_batch(rng, 10, num_runs=2)
    a2 = list(vref.batch_args(b2))
    a2[2] = None
    with pytest.raises(seb.SebError) as e:
        seb.get_values(*a2)
    assert e.value.code == INVALID and "null" in str(e.value)


def refusal_batch(rng, kind, lo, hi):
    """A valid batch of 400 keys, then keys lo < hi made invalid in the way `kind` names."""
    b = vref.make_batch(rng, 400, num_runs=3)
    val_bytes = None
    for i in (lo, hi):
        b["status"][i] = 1
        if kind == "run":            # a run id >= num_runs
            b["source"][i], b["run"][i], b["vloc"][i], b["vlen"][i] = 0, 3, 0, 0
        elif kind == "past_run":     # vloc + vlen one byte past the end of its run
            b["source"][i], b["run"][i], b["vloc"][i], b["vlen"][i] = 0, 2, len(b["vals"][2]) - 9, 10
        elif kind == "past_pool":
            b["source"][i], b["vloc"][i], b["vlen"][i] = 1, len(b["pool"]) - 9, 10
        elif kind == "wrap":         # vloc + vlen wraps to 1
            b["source"][i], b["vloc"][i], b["vlen"][i] = 1, 2**64 - 1, 2
        elif kind == "source":
            b["source"][i] = 2
        elif kind == "null_vals":    # a null vals[r] with val_bytes[r] != 0
            b["source"][i], b["run"][i], b["vloc"][i], b["vlen"][i] = 0, 1, 0, 0
    if kind == "null_vals":
        keep = (b["status"] != 1) | (b["source"] != 0) | (b["run"] != 1)
        keep[[lo, hi]] = True
        b["status"][~keep] = 0       # no other key names run 1
        val_bytes = [len(b["vals"][0]), 64, len(b["vals"][2])]
        b["vals"][1] = None
    return b, val_bytes


@pytest.mark.parametrize("kind", ["run", "past_run", "past_pool", "wrap", "source", "null_vals"])
def test_refusal_names_the_lowest_invalid_key(seb, kind):
    rng = np.random.default_rng(10)
    for lo, hi in ((37, 311), (0, 399)):
        b, val_bytes = refusal_batch(rng, kind, lo, hi)
        args = vref.batch_args(b)
        assert vref.lowest_invalid(*args, val_bytes=val_bytes) == lo
        with pytest.raises(seb.SebError) as e:
            seb.get_values(*args, val_bytes=val_bytes)
        assert e.value.code == INVALID and f"key {lo} " in str(e.value), str(e.value)
        # the same key with a status that carries nothing is no refusal
        b["status"][lo] = 2
        assert vref.lowest_invalid(*vref.batch_args(b), val_bytes=val_bytes) == hi
        b["status"][hi] = 255
        args = vref.batch_args(b)
        vref.assert_same(seb.get_values(*args, val_bytes=val_bytes), vref.values(*args, val_bytes=val_bytes))


def test_argument_refusals(seb):
    one = np.ones(1, np.uint8)
    z64, z32 = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
    vals9 = [np.zeros(4, np.uint8)] * 9
    with pytest.raises(seb.SebError) as e:  # more than SEB_MEM_MAX_RUNS runs
        seb.get_values(one, 0 * one, 0 * one, z64, z32, vals9)
    assert e.value.code == INVALID
    L = seb.lib()
    sz = seb.seb_values_sizes()
    assert L.seb_get_values(None, None, None, None, None, 2**32, None, None, 0, None, 0, C.byref(sz), None, None, 0) == INVALID
    assert L.seb_get_values(None, None, None, None, None, 0, None, None, 0, None, 8, C.byref(sz), None, None, 0) == INVALID
    assert L.seb_get_values(None, None, None, None, None, 0, None, None, 0, None, 0, None, None, None, 0) == INVALID
    assert L.seb_dev_get_values_workspace_size(2**32) == 0
    assert L.seb_dev_get_values_workspace_size(1) >= 128 + 16 + 13
