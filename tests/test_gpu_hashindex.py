"""GPU: the hash index's read side on the device (include/seb_bloom.h, "hash index, read side").

seb_dev_seg_verify, seb_dev_hidx_insert / _count and seb_dev_hidx_get equal the host half (seb_seg_verify,
seb_hidx_lookup, themselves held to hashindex_ref's restatement in test_hashindex.py) in ok, valid, live, the key
count and (status, rec, vloc, vlen, source).  Every shared case at two table sizes (capacity = the distinct keys, and
four times that), and again with the test-only option hidx_hash_mask = 3, under which every key shares one tag and
four home slots, so the key compare and long probe chains decide every answer; the results must be identical.  One
store of about 300,000 records over 100,000 keys in four segments.  A table of 4 slots for 1,000 keys is
SEB_ERR_RANGE and the retry succeeds; two inserts equal one; bits flipped in the pool after the build turn exactly
the flipped records' keys ERROR under verify and none without it.  With the option grid_cap at 1 and 2, 1,354
records and 1,300 keys take the loops of k_seg_live, k_hidx_insert and k_hidx_get through three trips, the last one
partial, at hash masks 0 and 3; the outputs equal the default grid's byte for byte.  Every output starts as 0xA5 between 64 guard
bytes.  The entry points' refusals, one case on a busy side stream with late inputs, and recover -> get_batch ->
values end to end against the reference dict, byte for byte.  The corrupted inputs are data errors that the kernels
answer with a status; nothing here provokes a fault."""
import numpy as np
import pytest

import crc_ref as cr
import hashindex_ref as href
import stream_late as sl

pytestmark = pytest.mark.gpu

CASES = href.cases()
SEG_CASES = cr.seg_cases()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


lead_view = sl.lead_view  # the bytes of an array on the device, `lead` bytes into an aligned allocation


class Store:
    """Segment images laid out for the calls, on the host (with the host half's answers) and on the device."""

    def __init__(self, torch, seb, segments, lead=1):
        self.pool, self.rec_off, self.first, self.base, self.size, self.tails = seb.segs_scan(segments)
        self.ok, self.valid, self.size_after, self.live = seb.seg_verify(self.pool, self.rec_off, self.first, self.base, self.size)
        self.n, self.nseg, self.pool_bytes = self.rec_off.size, len(segments), self.pool.size
        self.d_pool = lead_view(torch, self.pool, lead)
        self.d_off = sl.to_dev(torch, self.rec_off)
        self.d_first = sl.to_dev(torch, self.first)


def dev_verify(torch, seb, s, stream=None):
    """seb_dev_seg_verify into guarded outputs: (ok, valid, live, the live tensor)."""
    ok, live, valid = sl.Out(torch, s.n, np.uint8), sl.Out(torch, s.n, np.uint8), sl.Out(torch, s.nseg, np.uint64)
    seb.dev_seg_verify(s.d_pool, s.pool_bytes, s.d_off, s.n, s.d_first, s.nseg, ok.t, valid.t, live.t, stream=stream)
    return ok, valid, live


def new_table(torch, seb, capacity):
    """A cleared table between guard bytes: (the whole buffer, the table's view)."""
    nbytes = seb.dev_hidx_table_bytes(capacity)
    buf = torch.full((sl.GUARD + nbytes + sl.GUARD,), sl.FILL, dtype=torch.uint8, device="cuda")
    table = buf[sl.GUARD: sl.GUARD + nbytes]
    assert table.data_ptr() % 16 == 0
    seb.dev_hidx_clear(table, capacity)
    return buf, table


def table_guards(buf):
    h = buf.cpu().numpy()
    assert (h[: sl.GUARD] == sl.FILL).all() and (h[-sl.GUARD:] == sl.FILL).all(), "bytes outside the table were written"


def dev_keys_of(torch, seb, keys, lead=3):
    data, off = href.key_lists(keys)
    return seb.dev_keys(lead_view(torch, data, lead), sl.to_dev(torch, off))


def dev_get(torch, seb, s, table, capacity, keys, verify, dk=None, stream=None):
    n = len(keys)
    outs = [sl.Out(torch, n, t) for t in (np.uint8, np.uint64, np.uint64, np.uint32, np.uint8)]
    seb.dev_hidx_get(table, capacity, s.d_pool, s.pool_bytes, dev_keys_of(torch, seb, keys) if dk is None else dk, verify,
                     *[o.t for o in outs], stream=stream)
    return outs


def same_get(seb, s, live, keys, verify, outs, what):
    st, rec, vloc, vlen, distinct = seb.hidx_lookup(s.pool, s.rec_off, live, href.key_lists(keys), verify)
    for name, o, w in zip(("status", "rec", "vloc", "vlen"), outs, (st, rec, vloc, vlen)):
        sl.same(o.get(name), w, f"{what}: {name}")
    sl.same(outs[4].get("source"), (st == href.FOUND).astype(np.uint8), f"{what}: source")
    return st, distinct


def build_and_check(torch, seb, segments, what, factor=1, keys=None):
    """verify + insert + count + get (verify on and off) against the host half; returns the statuses."""
    s = Store(torch, seb, segments)
    ok, valid, live = dev_verify(torch, seb, s)
    torch.cuda.synchronize()
    sl.same(ok.get("ok")[: s.n], s.ok, f"{what}: ok")
    sl.same(valid.get("valid"), s.valid, f"{what}: valid")
    sl.same(live.get("live")[: s.n], s.live, f"{what}: live")
    rec = href.recover(segments)
    capacity = factor * len(rec["index"])
    buf, table = new_table(torch, seb, capacity)
    seb.dev_hidx_insert(table, capacity, s.d_pool, s.pool_bytes, s.d_off, live.t, s.n)
    distinct, bad = seb.dev_hidx_count(table, capacity)
    assert (distinct, bad) == (len(rec["index"]), 0), what
    keys = href.probes(rec, np.random.default_rng(3)) if keys is None else keys
    sts = []
    for verify in (True, False):
        outs = dev_get(torch, seb, s, table, capacity, keys, verify)
        torch.cuda.synchronize()
        st, d = same_get(seb, s, s.live, keys, verify, outs, what)
        assert d == distinct
        sts.append(st)
    table_guards(buf)
    return sts


# ------------------------------------------------------------------ the shared cases

@pytest.mark.parametrize("factor", [1, 4])
@pytest.mark.parametrize("name", sorted(CASES))
def test_cases(seb, torch_cuda, name, factor):
    build_and_check(torch_cuda, seb, CASES[name], name, factor)


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_with_colliding_hashes(seb, torch_cuda, name):
    """hidx_hash_mask = 3: one tag, four home slots; the answers are those of the full hash."""
    want = build_and_check(torch_cuda, seb, CASES[name], name)
    assert len(href.recover(CASES[name])["index"]) <= 2000
    with seb.option("hidx_hash_mask", 3):
        got = build_and_check(torch_cuda, seb, CASES[name], name + " (mask 3)")
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


# ------------------------------------------------------------------ a large store

@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(11)
    segments, table = href.big_store(rng)
    return segments, table, rng


def test_large_store(seb, torch_cuda, big):
    """About 300,000 records over 100,000 keys in four segments, a flipped bit in the second segment; the batch is
    the fixed-stride layout: 16-byte aligned keys, half of them present."""
    torch = torch_cuda
    segments, keytab, rng = big
    segments = list(segments)
    mid = seb.seg_scan(segments[1])[0]
    segments[1] = href.flip(segments[1], int(mid[len(mid) // 2]) + 5, 2)  # a timestamp byte of a middle record
    s = Store(torch, seb, segments, lead=0)
    assert s.n > 250_000 and s.valid[1] < s.first[2] - s.first[1]
    ok, valid, live = dev_verify(torch, seb, s)
    torch.cuda.synchronize()
    sl.same(ok.get("ok"), s.ok, "ok")
    sl.same(valid.get("valid"), s.valid, "valid")
    sl.same(live.get("live"), s.live, "live")
    import keygen as kg
    probe = np.concatenate([keytab[rng.integers(0, len(keytab), 100_000)], kg.key16(np.arange(10**7, 10**7 + 100_000))])
    probe = probe[rng.permutation(len(probe))]
    st, rec, vloc, vlen, distinct = seb.hidx_lookup(s.pool, s.rec_off, s.live, probe, True)
    assert 90_000 < distinct <= 100_000 and 60_000 < int((st == href.FOUND).sum()) < 100_000
    capacity = distinct
    buf, table = new_table(torch, seb, capacity)
    seb.dev_hidx_insert(table, capacity, s.d_pool, s.pool_bytes, s.d_off, live.t, s.n)
    assert seb.dev_hidx_count(table, capacity) == (distinct, 0)
    d_probe = torch.from_numpy(probe.copy()).cuda()
    assert d_probe.data_ptr() % 16 == 0
    dk = seb.dev_keys(d_probe, n=len(probe), stride=16)
    for verify in (True, False):
        outs = [sl.Out(torch, len(probe), t) for t in (np.uint8, np.uint64, np.uint64, np.uint32, np.uint8)]
        seb.dev_hidx_get(table, capacity, s.d_pool, s.pool_bytes, dk, verify, *[o.t for o in outs])
        torch.cuda.synchronize()
        for name, o, w in zip(("status", "rec", "vloc", "vlen"), outs, (st, rec, vloc, vlen)):
            sl.same(o.get(name), w, name)
    table_guards(buf)


# ------------------------------------------------------------------ a table that fills; two inserts

def thousand_keys():
    w1, w2 = href.Writer(), href.Writer(5000)
    for i in range(1000):
        (w1 if i < 600 else w2).put(b"key-%05d" % i, b"v-%d" % i)
    for i in range(0, 1000, 3):
        w2.put(b"key-%05d" % i, b"second-%d" % i)
    for i in range(0, 1000, 50):
        w2.delete(b"key-%05d" % i)
    return [w1.bytes(), w2.bytes()]


def test_a_table_that_fills_is_range_and_the_retry_succeeds(seb, torch_cuda):
    torch = torch_cuda
    segments = thousand_keys()
    s = Store(torch, seb, segments)
    ok, valid, live = dev_verify(torch, seb, s)
    buf, table = new_table(torch, seb, 2)
    assert seb.dev_hidx_table_bytes(2) == 64 + 4 * 8
    seb.dev_hidx_insert(table, 2, s.d_pool, s.pool_bytes, s.d_off, live.t, s.n)
    with pytest.raises(seb.SebError) as e:
        seb.dev_hidx_count(table, 2)
    assert e.value.code == -4 and "filled" in str(e.value)
    table_guards(buf)
    keys = href.probes(href.recover(segments), np.random.default_rng(8))
    outs = dev_get(torch, seb, s, table, 2, keys, True)  # a full table still answers inside its bounds
    torch.cuda.synchronize()
    assert set(outs[0].get("status")) <= {0, 1, 2}
    capacity = int(s.live.sum())
    buf, table = new_table(torch, seb, capacity)
    seb.dev_hidx_insert(table, capacity, s.d_pool, s.pool_bytes, s.d_off, live.t, s.n)
    assert seb.dev_hidx_count(table, capacity) == (1000, 0)
    outs = dev_get(torch, seb, s, table, capacity, keys, True)
    torch.cuda.synchronize()
    same_get(seb, s, s.live, keys, True, outs, "retry")


@pytest.mark.parametrize("mask", [0, 3])
def test_two_inserts_equal_one(seb, torch_cuda, mask):
    """The records up to a boundary, then those behind it (greater offsets), into one table; also the same records
    inserted twice."""
    torch = torch_cuda
    segments = thousand_keys()
    s = Store(torch, seb, segments)
    keys = href.probes(href.recover(segments), np.random.default_rng(9))
    with seb.option("hidx_hash_mask", mask):
        for cut in (1, 600, 1100):
            buf, table = new_table(torch, seb, 1000)
            seb.dev_hidx_insert(table, 1000, s.d_pool, s.pool_bytes, s.d_off[:cut], None, cut)
            seb.dev_hidx_insert(table, 1000, s.d_pool, s.pool_bytes, s.d_off[cut:], None, s.n - cut)
            seb.dev_hidx_insert(table, 1000, s.d_pool, s.pool_bytes, s.d_off, None, s.n)
            assert seb.dev_hidx_count(table, 1000) == (1000, 0)
            outs = dev_get(torch, seb, s, table, 1000, keys, True)
            torch.cuda.synchronize()
            same_get(seb, s, None, keys, True, outs, f"cut {cut}")
            table_guards(buf)


# ------------------------------------------------------------------ capped grids: the grid-stride loops iterate

def capped_store(torch, seb):
    """thousand_keys() with a flipped bit in the first segment (live is 0 behind it), and a batch of 1,300 keys: at
    most 2 workgroups take both in three trips, the last one partial."""
    segments = thousand_keys()
    off = seb.seg_scan(segments[0])[0]
    segments[0] = href.flip(segments[0], int(off[400]) + 5, 2)
    s = Store(torch, seb, segments)
    rec = href.recover(segments)
    keys = href.probes(rec, np.random.default_rng(21))
    keys = (keys + sorted(rec["index"]))[:1300]
    assert 2 * 256 * 2 < s.n < 2 * 256 * 3 and 2 * 256 * 2 < len(keys) < 2 * 256 * 3
    assert 0 < int(s.live[:1024].sum()) < 1024 and s.live[1024:].any(), "every trip writes both values of live"
    return s, rec, keys


@pytest.mark.parametrize("mask", [0, 3])
def test_verify_with_live_under_a_grid_cap(seb, torch_cuda, mask):
    """seb_dev_seg_verify with live (k_seg_live) at 1 and 2 workgroups."""
    torch = torch_cuda
    s, _, _ = capped_store(torch, seb)
    runs = {}
    with seb.option("hidx_hash_mask", mask):
        for cap in sl.CAPS:
            with sl.grid_cap(seb, cap):
                ok, valid, live = dev_verify(torch, seb, s)
                torch.cuda.synchronize()
            runs[cap] = [o.get(name) for o, name in ((ok, "ok"), (valid, "valid"), (live, "live"))]
            for got, want, name in zip(runs[cap], (s.ok, s.valid, s.live), ("ok", "valid", "live")):
                sl.same(got, want, f"cap {cap}: {name}")
    assert all(a.tobytes() == b.tobytes() for cap in (1, 2) for a, b in zip(runs[cap], runs[None]))


@pytest.mark.parametrize("mask", [0, 3])
def test_insert_and_count_under_a_grid_cap(seb, torch_cuda, mask):
    """seb_dev_hidx_insert / _count at 1 and 2 workgroups: the key count, and the table's answers to a default-grid
    Get, equal the host half's and the default grid's.  (Which slot a key takes depends on the order of arrival, so
    tables are compared through what they answer.)"""
    torch = torch_cuda
    s, rec, keys = capped_store(torch, seb)
    capacity = len(rec["index"])
    d_live = sl.to_dev(torch, s.live)
    runs = {}
    with seb.option("hidx_hash_mask", mask):
        for cap in sl.CAPS:
            buf, table = new_table(torch, seb, capacity)
            with sl.grid_cap(seb, cap):
                seb.dev_hidx_insert(table, capacity, s.d_pool, s.pool_bytes, s.d_off, d_live, s.n)
                assert seb.dev_hidx_count(table, capacity) == (capacity, 0), cap
            outs = dev_get(torch, seb, s, table, capacity, keys, True)
            torch.cuda.synchronize()
            st, distinct = same_get(seb, s, s.live, keys, True, outs, f"cap {cap}")
            assert distinct == capacity and (st == href.FOUND).sum() > 500 and (st == href.MISS).any()
            runs[cap] = [o.get().tobytes() for o in outs]
            table_guards(buf)
    assert runs[1] == runs[None] and runs[2] == runs[None]


@pytest.mark.parametrize("verify", [True, False])
@pytest.mark.parametrize("mask", [0, 3])
def test_get_under_a_grid_cap(seb, torch_cuda, mask, verify):
    """seb_dev_hidx_get at 1 and 2 workgroups, with the CRC check and without it."""
    torch = torch_cuda
    s, rec, keys = capped_store(torch, seb)
    capacity = len(rec["index"])
    runs = {}
    with seb.option("hidx_hash_mask", mask):
        buf, table = new_table(torch, seb, capacity)
        seb.dev_hidx_insert(table, capacity, s.d_pool, s.pool_bytes, s.d_off, sl.to_dev(torch, s.live), s.n)
        for cap in sl.CAPS:
            with sl.grid_cap(seb, cap):
                outs = dev_get(torch, seb, s, table, capacity, keys, verify)
                torch.cuda.synchronize()
            st, _ = same_get(seb, s, s.live, keys, verify, outs, f"cap {cap}")
            assert (st[1024:] == href.FOUND).any() and (st[:1024] == href.FOUND).any()
            runs[cap] = [o.get().tobytes() for o in outs]
        table_guards(buf)
    assert runs[1] == runs[None] and runs[2] == runs[None]


# ------------------------------------------------------------------ crc_ref's cases: windows, alignments, lying sizes

class CaseStore:
    """A crc_ref segment case laid out like Store, its pool `lead` bytes off a 16-byte boundary."""

    def __init__(self, torch, seb, case, lead):
        self.pool, self.rec_off, self.first = case["image"], case["off"], case["first"]
        self.ok, self.valid, _, self.live = seb.seg_verify(self.pool, self.rec_off, self.first, case["base"], case["size"])
        self.n, self.nseg, self.pool_bytes = self.rec_off.size, self.first.size - 1, self.pool.size
        self.d_pool = lead_view(torch, self.pool, lead)
        assert self.d_pool.data_ptr() % 16 == lead % 16
        self.d_off = sl.to_dev(torch, self.rec_off)
        self.d_first = sl.to_dev(torch, self.first)


def case_leads(case):
    return cr.LEADS if not case["name"].startswith("window") else (case["lead"],)


@pytest.mark.parametrize("name", sorted(SEG_CASES))
def test_seg_verify_edge_cases(seb, torch_cuda, name):
    """seb_dev_seg_verify on a crc_ref case (three or four segments, a boundary on a workgroup's edge and one inside
    a workgroup): ok, valid and live equal the host half's and the restated rule's.

    The lying_*_sealed cases are the ones that tell the two checksum paths apart: record 128 of a staged workgroup
    claims bytes past the window, and its crc field matches exactly those bytes, so ok = 1 only if the checksum went
    through crc_range over the pool (a walk of the window's LDS copy gives ok = 0).  In the unsealed ones a wrong path
    and the right one both answer ok = 0.  Keep them."""
    torch = torch_cuda
    case = SEG_CASES[name]
    for lead in case_leads(case):
        cr.assert_case(case, lead)  # the input does what its name says, at this lead
        s = CaseStore(torch, seb, case, lead)
        inner = s.first[1:-1].tolist()
        assert any(f % 256 for f in inner) and (256 in inner or s.n == 256)
        ok, valid, live = dev_verify(torch, seb, s)
        torch.cuda.synchronize()
        for got, host, rule, what in ((ok, s.ok, case["ok"], "ok"), (valid, s.valid, case["valid"], "valid"),
                                      (live, s.live, case["live"], "live")):
            sl.same(got.get(what), host, f"{name} lead {lead}: {what}")
            sl.same(host, rule, f"{name}: the host half's {what}")


@pytest.mark.parametrize("name", sorted(n for n in SEG_CASES if n.startswith(("sweep", "lying"))))
def test_get_with_verify_edge_cases(seb, torch_cuda, name):
    """seb_dev_hidx_get with the CRC check over a crc_ref pool, every key its records state looked up and some absent
    ones: over the live records, and over all records (then a record whose size field lies without a matching
    checksum is found and answers ERROR; one that claims bytes past the pool never enters the table)."""
    torch = torch_cuda
    case = SEG_CASES[name]
    keys = cr.seg_keys(case["image"], case["off"])
    keys = keys + [b"absent-%d" % i for i in range(9)] + [k + b"\x00" for k in keys[:9]]
    inside = case["ends"] <= case["image"].size
    for lead in case_leads(case):
        s = CaseStore(torch, seb, case, lead)
        for live in (s.live, None):
            st, _, _, _, distinct = seb.hidx_lookup(s.pool, s.rec_off, live, href.key_lists(keys), True)
            assert (st == href.FOUND).sum() > 200 and (st == href.MISS).sum() >= 18
            buf, table = new_table(torch, seb, len(keys))
            seb.dev_hidx_insert(table, len(keys), s.d_pool, s.pool_bytes, s.d_off, None if live is None else sl.to_dev(torch, live), s.n)
            skipped = int((~inside & (np.ones(s.n, bool) if live is None else live.astype(bool))).sum())
            assert seb.dev_hidx_count(table, len(keys)) == (distinct, skipped), (name, lead)
            for verify in (True, False):
                outs = dev_get(torch, seb, s, table, len(keys), keys, verify)
                torch.cuda.synchronize()
                got, _ = same_get(seb, s, live, keys, verify, outs, f"{name} lead {lead} verify {verify}")
                assert (got == href.ERROR).any() == (verify and live is None and name.startswith("lying") and
                                                     "sealed" not in name and "past" not in name)
            table_guards(buf)


# ------------------------------------------------------------------ verify

def test_bits_flipped_after_the_build(seb, torch_cuda):
    torch = torch_cuda
    segments = thousand_keys()
    rec = href.recover(segments)
    s = Store(torch, seb, segments)
    ok, valid, live = dev_verify(torch, seb, s)
    buf, table = new_table(torch, seb, 1000)
    seb.dev_hidx_insert(table, 1000, s.d_pool, s.pool_bytes, s.d_off, live.t, s.n)
    assert seb.dev_hidx_count(table, 1000) == (1000, 0)
    base = [0, len(segments[0])]
    at = {k: base[rec["index"][k][0]] + rec["index"][k][1] for k in (b"key-00007", b"key-00100")}
    assert href.get(segments, rec["index"], b"key-00007")[0] == href.FOUND
    assert href.get(segments, rec["index"], b"key-00100")[0] == href.MISS  # a tombstone
    flips = {at[b"key-00007"] + href.HEADER + 9 + 1: 4, at[b"key-00100"] + 5: 0}  # a value byte; the tombstone's timestamp
    bad = s.pool.copy()
    for where, bit in flips.items():
        bad[where] ^= 1 << bit
        s.d_pool[where] = int(bad[where])
    s.pool = bad
    keys = href.probes(rec, np.random.default_rng(10))
    outs = dev_get(torch, seb, s, table, 1000, keys, True)
    torch.cuda.synchronize()
    st, _ = same_get(seb, s, s.live, keys, True, outs, "verify on")
    assert {keys[i] for i in np.nonzero(st == href.ERROR)[0]} == {b"key-00007", b"key-00100"}
    outs = dev_get(torch, seb, s, table, 1000, keys, False)
    torch.cuda.synchronize()
    st, _ = same_get(seb, s, s.live, keys, False, outs, "verify off")
    assert not (st == href.ERROR).any() and st[keys.index(b"key-00007")] == href.FOUND


# ------------------------------------------------------------------ refusals

def test_refusals(seb, torch_cuda):
    torch = torch_cuda
    s = Store(torch, seb, CASES["a_65"], lead=0)
    buf, table = new_table(torch, seb, 100)
    keys = [b"key-0001", b"nope"]
    dk = dev_keys_of(torch, seb, keys)
    st = torch.zeros(2, dtype=torch.uint8, device="cuda")
    u64 = torch.zeros(4, dtype=torch.int64, device="cuda")
    u32 = torch.zeros(4, dtype=torch.int32, device="cuda")
    ok = torch.zeros(s.n, dtype=torch.uint8, device="cuda")
    valid = torch.zeros(2, dtype=torch.int64, device="cuda")
    odd8 = u64.view(torch.uint8)[4:]
    odd4 = u32.view(torch.uint8)[2:]

    def refused(fn, *a, words=None, **kw):
        with pytest.raises(seb.SebError) as e:
            fn(*a, **kw)
        assert e.value.code == -1, e.value
        if words:
            assert words in str(e.value), e.value

    P = s.pool_bytes
    refused(seb.dev_hidx_clear, None, 100, words="null")
    refused(seb.dev_hidx_clear, table[8:], 100, words="16-byte")
    refused(seb.dev_hidx_clear, table, (1 << 40) + 1, words="capacity")
    refused(seb.dev_seg_verify, None, P, s.d_off, s.n, s.d_first, 1, ok, valid, words="null pool")
    refused(seb.dev_seg_verify, s.d_pool, 1 << 47, s.d_off, s.n, s.d_first, 1, ok, valid, words="2^47")
    refused(seb.dev_seg_verify, s.d_pool, P, None, s.n, s.d_first, 1, ok, valid)
    refused(seb.dev_seg_verify, s.d_pool, P, s.d_off, s.n, None, 1, ok, valid)
    refused(seb.dev_seg_verify, s.d_pool, P, s.d_off, s.n, s.d_first, 1, None, valid)
    refused(seb.dev_seg_verify, s.d_pool, P, s.d_off, s.n, s.d_first, 1, ok, None)
    refused(seb.dev_seg_verify, s.d_pool, P, s.d_off, s.n, s.d_first, 0, ok, valid, words="without a segment")
    refused(seb.dev_seg_verify, s.d_pool, P, s.d_off.view(torch.uint8)[4:], 3, s.d_first, 1, ok, valid, words="aligned")
    refused(seb.dev_seg_verify, s.d_pool, P, s.d_off, s.n, s.d_first, 1, ok, odd8, words="aligned")
    refused(seb.dev_hidx_insert, None, 100, s.d_pool, P, s.d_off, None, s.n)
    refused(seb.dev_hidx_insert, table[16 + 8:], 100, s.d_pool, P, s.d_off, None, s.n, words="16-byte")
    refused(seb.dev_hidx_insert, table, 100, None, P, s.d_off, None, s.n, words="null pool")
    refused(seb.dev_hidx_insert, table, 100, s.d_pool, 1 << 47, s.d_off, None, s.n, words="2^47")
    refused(seb.dev_hidx_insert, table, 100, s.d_pool, P, None, None, s.n, words="rec_off")
    refused(seb.dev_hidx_insert, table, 100, s.d_pool, P, s.d_off.view(torch.uint8)[4:], None, 3, words="aligned")
    refused(seb.dev_hidx_count, None, 100)
    refused(seb.dev_hidx_get, None, 100, s.d_pool, P, dk, True, st)
    refused(seb.dev_hidx_get, table, 100, None, P, dk, True, st, words="null pool")
    refused(seb.dev_hidx_get, table, 100, s.d_pool, 1 << 47, dk, True, st, words="2^47")
    refused(seb.dev_hidx_get, table, 100, s.d_pool, P, dk, True, None, words="status")
    refused(seb.dev_hidx_get, table, 100, s.d_pool, P, dk, True, st, odd8, words="aligned")
    refused(seb.dev_hidx_get, table, 100, s.d_pool, P, dk, True, st, None, odd8, words="aligned")
    refused(seb.dev_hidx_get, table, 100, s.d_pool, P, dk, True, st, None, None, odd4, words="aligned")
    bad_keys = seb.dev_keys(dk._keep[0], dk._keep[1].view(torch.uint8)[4:])
    bad_keys.n = 1
    refused(seb.dev_hidx_get, table, 100, s.d_pool, P, bad_keys, True, st, words="aligned")
    torch.cuda.synchronize()
    assert (table.cpu().numpy() == 0).all(), "a refused call wrote the table"
    # nothing to do is no refusal
    seb.dev_hidx_insert(table, 100, s.d_pool, P, None, None, 0)
    seb.dev_hidx_get(table, 100, s.d_pool, P, seb.dev_keys(dk._keep[0], n=0, stride=4), True, None)
    seb.dev_seg_verify(None, 0, None, 0, None, 0, None, None)
    assert seb.dev_hidx_count(table, 100) == (0, 0)
    table_guards(buf)


# ------------------------------------------------------------------ a busy side stream, late inputs

@pytest.fixture(scope="module")
def rig(seb, torch_cuda):
    try:
        r = sl.Rig(torch_cuda, seb)
    except AssertionError as e:
        pytest.fail(f"stream control: {e}")
    return r


def test_on_a_busy_side_stream(seb, torch_cuda, rig):
    """The pool and the offsets arrive late before verify + clear + insert; the keys late before the Get."""
    torch = torch_cuda
    good_segs = thousand_keys()
    s = Store(torch, seb, good_segs, lead=0)
    rng = np.random.default_rng(12)
    poison_pool = s.pool.copy()
    poison_pool[rng.integers(0, s.pool_bytes, 4000)] ^= 0x10  # many records fail their CRC
    poison_off = s.rec_off[::-1].copy()
    p_ok, p_valid, _, p_live = seb.seg_verify(poison_pool, s.rec_off, s.first, s.base, s.size)
    sl.differ([s.ok, s.valid], [p_ok, p_valid], ["ok", "valid"])
    keys = href.probes(href.recover(good_segs), rng)
    poison_keys = [k[::-1] if len(k) > 1 else k for k in keys]
    kdata, koff = href.key_lists(keys)
    pdata, _ = href.key_lists(poison_keys)
    want = seb.hidx_lookup(s.pool, s.rec_off, s.live, (kdata, koff), True)
    sl.differ(want[:4], seb.hidx_lookup(s.pool, s.rec_off, s.live, (pdata, koff), True)[:4])
    L = rig.session()
    d_pool = L.inp(s.pool, poison_pool)
    d_off = L.inp(s.rec_off, poison_off)
    d_first = sl.to_dev(torch, s.first)
    nbytes = seb.dev_hidx_table_bytes(1000)
    table = torch.full((nbytes,), 0x33, dtype=torch.uint8, device="cuda")  # not cleared yet
    ok, valid, live = sl.Out(torch, s.n, np.uint8), sl.Out(torch, 2, np.uint64), sl.Out(torch, s.n, np.uint8)
    L.arm()
    L.call(seb.dev_seg_verify, d_pool, s.pool_bytes, d_off, s.n, d_first, 2, ok.t, valid.t, live.t)
    L.call(seb.dev_hidx_clear, table, 1000)
    L.call(seb.dev_hidx_insert, table, 1000, d_pool, s.pool_bytes, d_off, live.t, s.n)
    assert L.plan(seb.dev_hidx_count, table, 1000) == (1000, 0)
    sl.same(ok.get("ok"), s.ok, "ok")
    sl.same(valid.get("valid"), s.valid, "valid")
    sl.same(live.get("live"), s.live, "live")
    d_kdata = L.inp(kdata, pdata)
    dk = seb.dev_keys(d_kdata, sl.to_dev(torch, koff))
    outs = [L.out(len(keys), t) for t in (np.uint8, np.uint64, np.uint64, np.uint32, np.uint8)]
    L.arm()
    L.call(seb.dev_hidx_get, table, 1000, d_pool, s.pool_bytes, dk, True, *[o.t for o in outs])
    L.finish()
    for name, o, w in zip(("status", "rec", "vloc", "vlen"), outs, want[:4]):
        sl.same(o.get(name), w, name)


# ------------------------------------------------------------------ end to end

@pytest.mark.parametrize("name", ["b_lengths", "d_put_delete_put", "e_flip_value", "f_short_payload", "g_wrap_small", "a_empty"])
def test_end_to_end(seb, torch_cuda, name):
    """HashIndex.recover -> get_batch (Get, then the values gather over the segment pool) against the reference dict."""
    segments = CASES[name]
    rec = href.recover(segments)
    hx = seb.HashIndex()
    try:
        got = hx.recover(segments)
        for k in ("valid", "size_after", "short_tail", "cut"):
            assert list(got[k]) == rec[k], (name, k)
        assert got["live_records"] == rec["live_records"] and got["distinct"] == len(rec["index"]) == hx.count
        assert list(hx.segment_sizes) == rec["size_after"]
        keys = href.probes(rec, np.random.default_rng(14))
        status, off, vals = hx.get_batch(keys)
        w_st, _, _, _, w_vals = href.get_batch(segments, rec["index"], keys)
        assert np.array_equal(status, w_st), name
        for i, w in enumerate(w_vals):
            assert vals[int(off[i]): int(off[i + 1])].tobytes() == w, (name, i)
    finally:
        hx.close()


def test_end_to_end_recover_retries_and_insert_appends(seb, torch_cuda):
    """A first capacity that is too small (the retry inside recover), then records appended to the active segment,
    one of them corrupt: the index equals a recover of the whole."""
    segments = thousand_keys()
    tail = href.Writer(9000)
    for i in range(990, 1030):
        tail.put(b"key-%05d" % i, b"appended-%d" % i)
    tail.delete(b"key-00001")
    good_tail = tail.bytes()
    bad_tail = href.flip(good_tail, tail.offsets[35] + 3, 1)
    hx = seb.HashIndex()
    try:
        got = hx.recover(segments, slack_bytes=len(good_tail), capacity=8)
        assert got["distinct"] == 1000 and hx.capacity == got["live_records"]
        assert hx.insert(bad_tail) == 35
        whole = [segments[0], segments[1] + bad_tail]
        rec = href.recover(whole)
        assert hx.count == len(rec["index"]) and list(hx.segment_sizes) == rec["size_after"]
        keys = href.probes(rec, np.random.default_rng(15))
        status, off, vals = hx.get_batch(keys)
        w_st, _, _, _, w_vals = href.get_batch(whole, rec["index"], keys)
        assert np.array_equal(status, w_st)
        for i, w in enumerate(w_vals):
            assert vals[int(off[i]): int(off[i + 1])].tobytes() == w, i
    finally:
        hx.close()


def test_end_to_end_insert_grows_a_table_that_fills(seb, torch_cuda):
    """recover with capacity = the keys (2,048 slots for 1,000 keys), then 1,200 new keys appended: the insert fills
    the table, and HashIndex rebuilds a larger one from the recovered segments and every insert so far."""
    segments = thousand_keys()
    first, second = href.Writer(9000), href.Writer(20000)
    for i in range(2000, 2100):
        first.put(b"key-%05d" % i, b"first-tail-%d" % i)
    for i in range(2100, 3200):
        second.put(b"key-%05d" % i, b"second-tail-%d" % i)
    second.put(b"key-00002", b"rewritten")
    hx = seb.HashIndex()
    try:
        got = hx.recover(segments, slack_bytes=len(first.buf) + len(second.buf), capacity=1000)
        assert got["distinct"] == 1000 and hx.capacity == 1000
        assert hx.insert(first.bytes()) == 100 and hx.capacity == 1000
        assert hx.insert(second.bytes()) == 1101 and hx.capacity > 1000
        whole = [segments[0], segments[1] + first.bytes() + second.bytes()]
        rec = href.recover(whole)
        assert hx.count == len(rec["index"]) == 2200 and list(hx.segment_sizes) == rec["size_after"]
        keys = href.probes(rec, np.random.default_rng(16))
        status, off, vals = hx.get_batch(keys)
        w_st, _, _, _, w_vals = href.get_batch(whole, rec["index"], keys)
        assert np.array_equal(status, w_st)
        for i, w in enumerate(w_vals):
            assert vals[int(off[i]): int(off[i + 1])].tobytes() == w, i
    finally:
        hx.close()
