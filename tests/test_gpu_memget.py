"""GPU: the batched memtable lookup (include/seb_bloom.h, the memtable lookup group).

seb_dev_run_index + seb_dev_runs_search equal the host half (seb_runs_search, itself held to memget_ref's
restatement in test_memget.py) in all six outputs: run sizes 0..1025 and 50,000, batch sizes 0..257, a grid-stride
boundary and 200,000, every key layout (aligned stride 16, strides 5 and 24, offsets with offsets[0] != 0, keys at
an odd address), a run's keys at an odd address, Go string order on ORDER_KEYS, 2 and 8 runs with shared keys, a
tombstone in run 0 over a value in run 1, a key held only by the last run.  Outputs start as 0xA5 between guard
bytes and each nullable output is left out in turn.  seb_dev_run_index names the same entry as the host half in
its three refusals and leaves the 0x5A guard behind the index alone.  A log image goes from seb_dev_wal_replay_*
through the index into the search without leaving the device.  seb_dev_get_join over every status pair, and a
small LSM.Get over memtable runs and an SSTable block pool."""
import numpy as np
import pytest

import block_ref as br
import memget_ref as gref
import memtable_ref as mref

pytestmark = pytest.mark.gpu

GUARD = 64
ELEM = (1, 1, 4, 8, 4, 8)  # bytes per key of status, run, entry, vloc, vlen, seq
DTYPE = (np.uint8, np.uint8, np.uint32, np.uint64, np.uint32, np.uint64)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def odd_view(torch, a, lead=1):
    """The bytes of `a` at an odd device address (lead bytes into an allocation)."""
    buf = torch.from_numpy(np.concatenate([np.full(lead, 0xEE, np.uint8), np.asarray(a, np.uint8)])).cuda()
    return buf[lead:]


def u64_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def upload_run(torch, seb, a, with_seq=True, with_deleted=True):
    """arrays (keys, key_off, vals, val_off, deleted, seq) -> a dev_run whose keys and deleted sit at odd addresses."""
    keys, koff, _, voff, dele, seq = a
    dk = odd_view(torch, keys)
    assert keys.size == 0 or dk.data_ptr() % 2 == 1
    return seb.dev_run(dk, u64_dev(torch, koff), u64_dev(torch, voff), odd_view(torch, dele, 3) if with_deleted else None,
                       u64_dev(torch, seq) if with_seq else None, n=len(koff) - 1, key_bytes=keys.size)


def build_index(torch, seb, run):
    """The run's index with a 0x5A guard behind it, which the build must leave alone, accepted or refused."""
    size = seb.dev_run_index_size(run.n)
    assert size == (16 + 16 * run.n if run.n else 0)
    ix = torch.full((size + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    try:
        seb.dev_run_index(run, ix, index_bytes=size)
    finally:
        torch.cuda.synchronize()
        assert (ix[size:].cpu().numpy() == 0x5A).all(), "the index build wrote past its index"
    return ix


def dev_probes(torch, seb, probes, layout):
    """layout: 'varlen' (odd data pointer, offsets[0] != 0), 'fixed' (aligned) or 'fixed_odd' (stride = the key length)."""
    if layout == "varlen":
        off = np.cumsum([0] + [len(p) for p in probes]).astype(np.uint64) + np.uint64(3)
        buf = np.concatenate([np.full(4, 0xEE, np.uint8), np.frombuffer(b"".join(probes), np.uint8), np.full(4, 0xEE, np.uint8)])
        d = torch.from_numpy(buf).cuda()[1:]
        assert d.data_ptr() % 2 == 1
        return seb.dev_keys(d, u64_dev(torch, off))
    stride = len(probes[0])
    assert all(len(p) == stride for p in probes)
    data = np.frombuffer(b"".join(probes), np.uint8)
    d = odd_view(torch, data) if layout == "fixed_odd" else torch.from_numpy(data.copy()).cuda()
    assert d.data_ptr() % 16 == (0 if layout == "fixed" else d.data_ptr() % 16)
    return seb.dev_keys(d, n=len(probes), stride=stride)


def device_search(torch, seb, dk, runs, indexes, omit=()):
    """The search into 0xA5 buffers between guards: six numpy arrays (None for an output left out)."""
    n = dk.n
    bufs = [torch.full((GUARD + e * n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for e in ELEM]
    views = [None if j in omit else b[GUARD:GUARD + e * n] for j, (b, e) in enumerate(zip(bufs, ELEM))]
    seb.dev_runs_search(dk, runs, indexes, *views)
    torch.cuda.synchronize()
    out = []
    for j, (b, e) in enumerate(zip(bufs, ELEM)):
        h = b.cpu().numpy()
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + e * n:] == 0xA5).all(), "bytes outside an output were written"
        if j in omit:
            assert (h == 0xA5).all(), "an output that was left out was written"
            out.append(None)
        else:
            out.append(np.frombuffer(h[GUARD:GUARD + e * n].tobytes(), DTYPE[j]))
    return out


def host_search(seb, arrays, probes):
    return seb.runs_search(probes, [seb.host_run(a[0], a[1], a[3], a[4], a[5]) for a in arrays])


def compare(torch, seb, arrays, probes, layout="varlen", name="", want=None):
    runs = [upload_run(torch, seb, a) for a in arrays]
    indexes = [build_index(torch, seb, r) if r.n else None for r in runs]
    got = device_search(torch, seb, dev_probes(torch, seb, probes, layout) if probes else seb.dev_keys(
        torch.zeros(16, dtype=torch.uint8, device="cuda"), n=0), runs, indexes)
    want = host_search(seb, arrays, probes) if want is None else want
    gref.assert_same(got, want, name)
    return got


def key_of(i, klen=16):
    return (b"%0*d" % (klen, i))[:klen]


def sized_run(n, seed=0, klen=16, step=3):
    """n entries with keys key_of(step * i): value sizes 0..40, every 7th entry deleted, sequences out of order."""
    rng = np.random.default_rng(seed)
    keys = np.frombuffer(b"".join(key_of(step * i, klen) for i in range(n)), np.uint8)
    koff = (np.arange(n + 1, dtype=np.uint64) * np.uint64(klen))
    dele = (np.arange(n) % 7 == 3).astype(np.uint8)
    vlen = np.where(dele == 1, 0, rng.integers(0, 41, n))
    voff = np.concatenate([[0], np.cumsum(vlen)]).astype(np.uint64)
    return keys, koff, np.zeros(int(voff[-1]), np.uint8), voff, dele, rng.integers(1, 1 << 50, n).astype(np.uint64)


def sized_probes(n_run, count, seed=1, klen=16, step=3):
    """One in `step` present: draws over [0, step * n_run + 2), so some lie above the last key."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, max(step * n_run, 4) + 2, count)
    return [key_of(int(i), klen) for i in ids]


# ------------------------------------------------------------------ shapes

@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 8, 9, 1023, 1024, 1025, 50_000])
def test_run_sizes(seb, torch_cuda, n):
    a = sized_run(n, seed=n)
    probes = sized_probes(n, 600, seed=n) + [key_of(0), key_of(3 * max(n - 1, 0)), key_of(3 * n), b"", b"\xff" * 20]
    got = compare(torch_cuda, seb, [a], probes, name=f"n={n}")
    if n >= 7:
        assert {gref.NONE, gref.FOUND} <= set(got[0].tolist())
    if n == 0:
        assert not got[0].any() and (got[1] == 0xFF).all() and (got[2] == gref.NO_ENTRY).all()


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257, 200_000])
def test_batch_sizes(seb, torch_cuda, count):
    a = sized_run(3000, seed=2)
    probes = sized_probes(3000, count, seed=count)
    got = compare(torch_cuda, seb, [a], probes, layout="fixed", name=f"batch {count}")
    assert all(g.size == count for g in got)
    if count >= 63:
        assert 0.2 < (got[0] != gref.NONE).mean() < 0.5


def test_grid_stride_boundary(seb, torch_cuda):
    """Two workgroups of 256 lanes walk 1,300 keys: three rounds, the last one partial."""
    a = sized_run(900, seed=4)
    probes = sized_probes(900, 1300, seed=5)
    want = host_search(seb, [a], probes)
    with seb.option("grid_cap", 2):
        assert 2 * 256 * 2 < len(probes) < 2 * 256 * 3
        compare(torch_cuda, seb, [a], probes, layout="fixed", name="grid_cap 2", want=want)


@pytest.mark.parametrize("layout,klen", [("fixed", 16), ("fixed_odd", 16), ("fixed", 5), ("fixed_odd", 5), ("fixed", 24),
                                         ("varlen", 16), ("varlen", 24)])
def test_key_layouts(seb, torch_cuda, layout, klen):
    """Aligned stride 16 is key_prefix's fast path; every other layout takes its byte loads: stride 5 (shorter than a
    prefix word), stride 24 (bytes past the prefix decide), the offsets form, keys at an odd address."""
    a = sized_run(700, seed=klen, klen=klen)
    probes = sized_probes(700, 500, seed=klen + 1, klen=klen)
    if klen == 24:  # keys that tie with an entry in their first 16 bytes and differ behind them
        probes += [key_of(3 * i, 24)[:23] + b"x" for i in range(0, 700, 50)]
    got = compare(torch_cuda, seb, [a], probes, layout=layout, name=f"{layout} {klen}")
    assert {gref.NONE, gref.FOUND, gref.TOMBSTONE} <= set(got[0].tolist())


def test_go_string_order(seb, torch_cuda):
    """Ties in the first 16 and 40 bytes, the empty key, extensions; against memget_ref directly as well."""
    ks = sorted(mref.ORDER_KEYS)
    every = gref.table_from_ops([(k, b"a%d" % i, 100 + i, i % 3 == 0) for i, k in enumerate(ks)])
    even = gref.table_from_ops([(k, b"e%d" % i, i, i % 4 == 0) for i, k in enumerate(ks) if i % 2 == 0])
    probes = gref.probes_for([every], extra=ks)
    for tables in ([every], [even, every]):
        got = compare(torch_cuda, seb, [gref.run_arrays(t, 5, 9) for t in tables], probes, name="ORDER_KEYS")
        gref.assert_same(got, gref.expected(tables, probes, [9] * len(tables)), "ORDER_KEYS vs the restatement")
    assert (got[0] != gref.NONE).sum() == len(ks)


def test_two_and_eight_runs(seb, torch_cuda):
    rng = np.random.default_rng(31)
    active = gref.table_from_ops([(b"a", b"new", 9, 0), (b"k", b"", 11, 1), (b"z", b"", 12, 1)])
    frozen = gref.table_from_ops([(b"k", b"old-value", 3, 0), (b"m", b"only-here", 4, 0), (b"z", b"", 5, 1)])
    probes = [b"k", b"m", b"a", b"z", b"b", b""]
    got = compare(torch_cuda, seb, [gref.run_arrays(active), gref.run_arrays(frozen)], probes, name="tombstone over value")
    assert got[0].tolist() == [gref.TOMBSTONE, gref.FOUND, gref.FOUND, gref.TOMBSTONE, gref.NONE, gref.NONE]
    assert got[1].tolist() == [0, 1, 0, 0, 0xFF, 0xFF] and got[4].tolist() == [0, 9, 3, 0, 0, 0]
    two = [gref.random_table(rng, 400), gref.random_table(rng, 500)]
    assert len(set(two[0].keys) & set(two[1].keys)) > 5
    got = compare(torch_cuda, seb, [gref.run_arrays(t) for t in two], gref.probes_for(two), name="2 runs")
    gref.assert_same(got, gref.expected(two, gref.probes_for(two)), "2 runs vs the restatement")
    eight = [gref.random_table(rng, 80) for _ in range(3)] + [mref.MemTable()] + [gref.random_table(rng, 80) for _ in range(3)]
    eight.append(gref.table_from_ops([(b"only-in-the-last", b"v", 1, 0)]))
    got = compare(torch_cuda, seb, [gref.run_arrays(t) for t in eight], gref.probes_for(eight), name="8 runs")
    assert set(got[1].tolist()) == {0, 1, 2, 4, 5, 6, 7, gref.NO_RUN}
    # nine runs, and a null status
    runs = [upload_run(torch_cuda, seb, gref.run_arrays(eight[0]))] * 9
    ix = [build_index(torch_cuda, seb, runs[0])] * 9
    dk = dev_probes(torch_cuda, seb, probes[:4], "varlen")
    st = torch_cuda.zeros(8, dtype=torch_cuda.uint8, device="cuda")
    for bad_runs, bad_ix, bad_st in ((runs, ix, st), (runs[:1], ix[:1], None)):
        with pytest.raises(seb.SebError) as ei:
            seb.dev_runs_search(dk, bad_runs, bad_ix, bad_st)
        assert ei.value.code == -1
    # no runs at all: everything is NONE
    got = device_search(torch_cuda, seb, dk, [], [])
    assert not got[0].any() and (got[1] == 0xFF).all() and (got[2] == gref.NO_ENTRY).all() and not got[5].any()


@pytest.mark.parametrize("omit", [1, 2, 3, 4, 5])
def test_nullable_outputs(seb, torch_cuda, omit):
    a = [sized_run(300, seed=1), sized_run(500, seed=2, step=2)]
    probes = sized_probes(500, 700, seed=omit)
    runs = [upload_run(torch_cuda, seb, x, with_seq=(r == 0)) for r, x in enumerate(a)]  # run 1 has no seq: 0
    indexes = [build_index(torch_cuda, seb, r) for r in runs]
    want = list(seb.runs_search(probes, [seb.host_run(a[0][0], a[0][1], a[0][3], a[0][4], a[0][5]),
                                         seb.host_run(a[1][0], a[1][1], a[1][3], a[1][4], None)]))
    assert (want[5][want[1] == 1] == 0).all() and (want[5][want[1] == 0] != 0).all()
    got = device_search(torch_cuda, seb, dev_probes(torch_cuda, seb, probes, "fixed"), runs, indexes, omit=(omit,))
    assert got[omit] is None
    for j in range(6):
        if j != omit:
            assert np.array_equal(got[j], want[j]), gref.NAMES[j]


def test_no_deleted_array_and_deleted_bytes(seb, torch_cuda):
    """deleted == NULL: no entry is; bytes 2 and 255 count as deleted (the builder's input rule)."""
    mt = gref.random_table(np.random.default_rng(5), 200)
    probes = gref.probes_for([mt])
    for byte in (2, 255):
        got = compare(torch_cuda, seb, [gref.run_arrays(mt, 5, 9, deleted_byte=byte)], probes, name=f"deleted byte {byte}")
        gref.assert_same(got, gref.expected([mt], probes, [9]), f"deleted byte {byte} vs the restatement")
    a = gref.run_arrays(mt)
    run = upload_run(torch_cuda, seb, a, with_deleted=False)
    got = device_search(torch_cuda, seb, dev_probes(torch_cuda, seb, probes, "varlen"), [run], [build_index(torch_cuda, seb, run)])
    want = seb.runs_search(probes, [seb.host_run(a[0], a[1], a[3], None, a[5])])
    gref.assert_same(got, want, "no deleted array")
    assert not (got[0] == gref.TOMBSTONE).any()


# ------------------------------------------------------------------ the index

def test_index_refusals_name_the_host_halfs_entry(seb, torch_cuda):
    good = list(gref.run_arrays(gref.random_table(np.random.default_rng(6), 300)))
    assert len(good[4]) > 45
    tie = mref.P40 + b"tail"
    tks = [b"!", b"#", tie, tie, tie + b"x"]  # equal neighbours that tie beyond 40 bytes
    a = list(gref.run_arrays(gref.table_from_ops([(k + bytes([i]), b"v", i, 0) for i, k in enumerate(tks)])))
    a[0], a[1] = np.frombuffer(b"".join(tks), np.uint8), np.cumsum([0] + [len(k) for k in tks]).astype(np.uint64)
    b = list(gref.run_arrays(gref.table_from_ops([(k, b"v", 1, 0) for k in (b"1", b"2", b"3", b"4")])))
    b[0] = np.frombuffer(b"acba", np.uint8)  # a decreasing pair (and a second one behind it)
    c = [x.copy() for x in good]
    c[1][41:] += np.uint64(c[0].size)  # a key_off past key_bytes (and every later one)
    d = [x.copy() for x in good]
    d[3][30:] += 50
    d[3][33] = d[3][32] - 1  # val_off decreases
    far = list(sized_run(2000, seed=3))  # an offender far from entry 0, in another workgroup, and a later one
    far[0] = far[0].copy()
    far[0][16 * 1500:16 * 1501] = far[0][16 * 1499:16 * 1500]
    far[0][16 * 1900:16 * 1901] = far[0][16 * 10:16 * 11]
    for arrays, entry, word in ((a, 3, "strictly"), (b, 2, "strictly"), (c, 40, "key_off"), (d, 32, "val_off"),
                                (far, 1500, "strictly")):
        with pytest.raises(seb.SebError) as host:
            host_search(seb, [arrays], [b"x"])
        with pytest.raises(seb.SebError) as dev:
            build_index(torch_cuda, seb, upload_run(torch_cuda, seb, arrays))  # checks the guard behind the index
        assert dev.value.code == -1 and f"entry {entry}" in str(dev.value) and word in str(dev.value), str(dev.value)
        assert str(host.value).split("entry ", 1)[1] == str(dev.value).split("entry ", 1)[1]
    run = upload_run(torch_cuda, seb, good)
    ix = torch_cuda.zeros(seb.dev_run_index_size(run.n), dtype=torch_cuda.uint8, device="cuda")
    with pytest.raises(seb.SebError) as ei:
        seb.dev_run_index(run, ix, index_bytes=ix.numel() - 1)
    assert ei.value.code == -1 and "index" in str(ei.value)
    assert seb.dev_run_index_size(0) == 0
    seb.dev_run_index(upload_run(torch_cuda, seb, gref.run_arrays(mref.MemTable())), None)  # n == 0: nothing launched


def test_a_stale_index_reads_nothing_out_of_bounds(seb, torch_cuda):
    """Another run's index, an all-ones and an all-zero index: answers are wrong at most, and every output stays
    inside its n elements (entry below n or NO_ENTRY, values inside the run's value bytes)."""
    a = sized_run(1000, seed=8, klen=24)
    run = upload_run(torch_cuda, seb, a)
    size = seb.dev_run_index_size(run.n)
    other = build_index(torch_cuda, seb, upload_run(torch_cuda, seb, sized_run(1000, seed=9, klen=24, step=5)))
    probes = sized_probes(1000, 800, seed=3, klen=24)
    dk = dev_probes(torch_cuda, seb, probes, "fixed")
    for ix in (other, torch_cuda.full((size,), 0xFF, dtype=torch_cuda.uint8, device="cuda"),
               torch_cuda.zeros(size, dtype=torch_cuda.uint8, device="cuda")):
        got = device_search(torch_cuda, seb, dk, [run], [ix])
        hit = got[0] != gref.NONE
        assert (got[2][hit] < 1000).all() and (got[2][~hit] == gref.NO_ENTRY).all()
        assert (got[3] + got[4] <= a[3][-1]).all()


# ------------------------------------------------------------------ end to end

def test_replay_to_lookup_without_leaving_the_device(seb, torch_cuda):
    torch = torch_cuda
    recs = mref.random_log(np.random.default_rng(41), 2500, max_key=60, max_val=80) + mref.order_log()
    image, off = mref.wal_image(recs)
    dimg = odd_view(torch, np.frombuffer(image, np.uint8), 7)
    doff = u64_dev(torch, off)
    ws = torch.zeros(seb.dev_wal_replay_workspace_size(len(recs)), dtype=torch.uint8, device="cuda")
    sizes = seb.dev_wal_replay_plan(dimg, doff, ws)
    _, n_out, kb, vb = sizes[:4]
    keys = torch.zeros(kb, dtype=torch.uint8, device="cuda")
    vals = torch.zeros(max(vb, 1), dtype=torch.uint8, device="cuda")
    koff, voff = (torch.zeros(n_out + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    dele = torch.zeros(n_out, dtype=torch.uint8, device="cuda")
    seq = torch.zeros(n_out, dtype=torch.int64, device="cuda")
    seb.dev_wal_replay_emit(dimg, doff, sizes, ws, keys, koff, vals, voff, dele, seq)
    run = seb.dev_run(keys, koff, voff, dele, seq)  # the replay's arrays as they are
    assert run.n == n_out and run.key_bytes == kb
    ix = build_index(torch, seb, run)
    mt, _ = mref.recover(mref.read_all(image))
    probes = sorted({r[0] for r in recs}) + [b"not-in-the-log", b"a\x00\x00\x00"]
    got = device_search(torch, seb, dev_probes(torch, seb, probes, "varlen"), [run], [ix])
    gref.assert_same(got, gref.expected([mt], probes), "replay -> lookup")
    hv = vals.cpu().numpy()
    for i in np.nonzero(got[0] == gref.FOUND)[0][:50]:  # the location is the value
        assert hv[int(got[3][i]):int(got[3][i]) + int(got[4][i])].tobytes() == mt.entries[int(got[2][i])][1]


def test_join_truth_table(seb, torch_cuda):
    torch = torch_cuda
    mem, sst = (x.reshape(-1).astype(np.uint8) for x in np.meshgrid(np.arange(3), np.arange(3), indexing="ij"))
    want_st, want_src = seb.get_join(mem, sst)  # the host form, held to the table in test_memget.py
    assert want_st.tolist() == [0, 1, 2, 1, 1, 1, 0, 0, 0] and want_src.tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 0]
    dmem, dsst = torch.from_numpy(mem).cuda(), torch.from_numpy(sst).cuda()
    st = torch.full((GUARD + 9 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    src = torch.full((GUARD + 9 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    seb.dev_get_join(dmem, dsst, 9, st[GUARD:GUARD + 9], src[GUARD:GUARD + 9])
    torch.cuda.synchronize()
    for buf, want in ((st, want_st), (src, want_src)):
        h = buf.cpu().numpy()
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + 9:] == 0xA5).all() and np.array_equal(h[GUARD:GUARD + 9], want)
    seb.dev_get_join(dmem, dsst, 9, dsst, None)  # status aliasing sst_status, source null
    torch.cuda.synchronize()
    assert np.array_equal(dsst.cpu().numpy(), want_st)
    seb.dev_get_join(dmem, dsst, 0, dsst, None)  # n == 0: nothing launched


def test_lsm_get_over_memtables_and_an_sstable_pool(seb, torch_cuda):
    torch = torch_cuda
    active = gref.table_from_ops([(b"hidden", b"", 20, 1), (b"mem-val", b"from-the-memtable", 21, 0)])
    frozen = gref.table_from_ops([(b"m-trunc", b"", 10, 1), (b"hidden", b"older-memtable-value", 11, 0)])
    images = [br.encode_block([(b"hidden", b"old"), (b"mem-val", b"sstv"), (b"sst-tomb", b"", 1)]),
              br.encode_block([(b"sst-tomb", b"older-value")]),
              br.encode_block([(b"a", b"x")], num=2)]  # the second entry's header is past the image: TRUNC
    probes = [b"hidden", b"m-trunc", b"sst-tomb", b"mem-val", b"nowhere", b"err-only"]
    none = seb.NO_BLOCK_ID
    bid = np.array([[0, none], [2, none], [0, 1], [0, none], [0, 1], [2, none]], np.uint32)
    pool = np.full((3, br.BLOCK), 0xA5, np.uint8)
    for b, img in enumerate(images):
        pool[b, :len(img)] = np.frombuffer(img, np.uint8)
    dpool = torch.from_numpy(pool.reshape(-1)).cuda()
    dblen = torch.from_numpy(np.array([len(i) for i in images], np.uint16).view(np.int16)).cuda()
    dk = dev_probes(torch, seb, probes, "varlen")
    n = len(probes)
    cells = torch.zeros(n * 2, dtype=torch.int32, device="cuda")
    dbid = torch.from_numpy(bid.reshape(-1).view(np.int32).copy()).cuda()
    seb.dev_search_blocks(dk, dbid, 2, dpool, dblen, cells)
    sst = torch.zeros(n, dtype=torch.uint8, device="cuda")
    seb.dev_resolve_rows(cells, dbid, n, 2, sst)
    runs = [upload_run(torch, seb, gref.run_arrays(t)) for t in (active, frozen)]
    mem = device_search(torch, seb, dk, runs, [build_index(torch, seb, r) for r in runs])
    dmem = torch.from_numpy(mem[0].copy()).cuda()
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    source = torch.zeros(n, dtype=torch.uint8, device="cuda")
    seb.dev_get_join(dmem, sst, n, status, source)
    torch.cuda.synchronize()
    assert sst.cpu().numpy().tolist() == [br.GET_FOUND, br.GET_ERROR, br.GET_FOUND, br.GET_FOUND, br.GET_MISS, br.GET_ERROR]
    assert mem[0].tolist() == [gref.TOMBSTONE, gref.TOMBSTONE, gref.NONE, gref.FOUND, gref.NONE, gref.NONE]
    # a memtable tombstone hides an SSTable value and an SSTable TRUNC error; an SSTable tombstone falls through
    assert status.cpu().numpy().tolist() == [br.GET_MISS, br.GET_MISS, br.GET_FOUND, br.GET_FOUND, br.GET_MISS, br.GET_ERROR]
    assert source.cpu().numpy().tolist() == [0, 0, 1, 0, 1, 1]
    assert mem[1].tolist()[:2] == [0, 1] and mem[4][3] == len(b"from-the-memtable")


def test_context_form(seb, torch_cuda):
    a = [sized_run(5000, seed=1), sized_run(9000, seed=2, step=2), sized_run(0)]
    probes = sized_probes(9000, 3000, seed=6)
    hruns = [seb.host_run(x[0], x[1], x[3], x[4], x[5]) for x in a]
    want = compare(torch_cuda, seb, a, probes, layout="fixed", name="device form")
    keys = np.frombuffer(b"".join(probes), np.uint8).reshape(-1, 16)
    gref.assert_same(seb.memtable_get(keys, hruns), want, "context form")
    ctx = seb.Ctx()
    try:
        gref.assert_same(ctx.memtable_get(probes, hruns[:1]), host_search(seb, a[:1], probes), "context form, lists")
        bad = list(a[0])
        bad[0] = bad[0].copy()
        bad[0][16 * 77:16 * 78] = bad[0][16 * 76:16 * 77]
        with pytest.raises(seb.SebError) as ei:
            ctx.memtable_get(probes, [hruns[1], seb.host_run(bad[0], bad[1], bad[3], bad[4], bad[5])])
        assert ei.value.code == -1 and "run 1: entry 77 " in str(ei.value)
    finally:
        ctx.close()
