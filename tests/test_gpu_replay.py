"""GPU: the WAL replay (include/seb_bloom.h, the WAL replay group).

seb_dev_wal_replay_plan / seb_dev_wal_replay_emit equal the host half (seb_wal_replay_plan / seb_wal_replay_emit,
itself held to memtable_ref's restatement in test_replay.py) byte for byte in all six arrays and the sizes: record
counts around the tile T (an odd tile count makes the pass tree lopsided), one key throughout, distinct keys in
descending and random order, a key's records in tiles 0, 2 and 4, an equal-key group across a tile edge of the
sorted result, Go string order on keys that tie in their first 16 and 40 bytes, Delete then Put and the reverse,
and large keys and values.  Outputs start as 0xA5 between guard bytes; keys, values and deleted sit at odd
addresses, the image sits at an odd address, and a 0x5A guard follows the workspace.  The replayed run goes
straight into the device builder, whose file equals the restatement's.

Beyond six tiles (each test asserts by arithmetic that its shape crosses its threshold, and compares the device
with the host half and with a reference of its own: last-record-wins by a dict, or scale_ref's lexsort):
  8 T + 1, 16 T, 17 T - 5, 33 T + 1 records    merge widths of 8 T and more, lopsided trees at depth; long
                                               equal-key groups, then mostly distinct keys
  17 T, one key's 2 T + 5 records in all tiles  a group over more than two whole tiles, ended by a Delete with a value
  129 T + 3 records                             130 tiles: a second workgroup of k_replay_cuts; bad framing of
                                               records 129 T + 1 and 129 T + 2 names the first, in the host's words
  1024 T + 1025 records                         1026 tiles, 11 passes: the carry of k_replay_scan"""
import numpy as np
import pytest

import memtable_ref as mref
import scale_ref as sc
import sstable_ref as sr

pytestmark = pytest.mark.gpu

GUARD = 64
T = 1024  # the tile of the sort, of the merge passes, of the survivor scan and of the emit (seb.MERGE_TILE)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def guarded(torch, size, lead=GUARD):
    buf = torch.full((lead + size + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[lead:lead + size]


def check_guards(buf, size, lead=GUARD):
    h = buf.cpu().numpy()
    assert (h[:lead] == 0xA5).all() and (h[lead + size:] == 0xA5).all(), "bytes outside the stated sizes were written"
    return h[lead:lead + size]


def dev_image(torch, image, off, lead=7):
    """The image at an odd device address (lead bytes into an allocation) and its offsets."""
    img = np.frombuffer(bytes(image), np.uint8)
    buf = torch.from_numpy(np.concatenate([np.full(lead, 0xEE, np.uint8), img])).cuda()
    view = buf[lead:]
    assert len(img) == 0 or view.data_ptr() % 2 == 1
    doff = torch.from_numpy(np.array(off, np.uint64).view(np.int64)).cuda()
    return view, doff


def device_plan(torch, seb, image, off):
    """plan on the device: (dimg, doff, ws, sizes); the 16 bytes behind the workspace stay 0x5A, accepted or refused."""
    dimg, doff = dev_image(torch, image, off)
    n = len(off) - 1
    ws = torch.full((seb.dev_wal_replay_workspace_size(n) + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    try:
        sizes = seb.dev_wal_replay_plan(dimg, doff, ws, ws_bytes=ws.numel() - 16)
    finally:
        torch.cuda.synchronize()
        assert (ws[-16:].cpu().numpy() == 0x5A).all(), "the plan wrote past its workspace"
    return dimg, doff, ws, sizes


def device_emit(torch, seb, dimg, doff, ws, sizes):
    """emit into guarded 0xA5 buffers, keys, values and deleted at odd addresses: the six arrays as numpy."""
    _, n_out, kb, vb = sizes[:4]
    bk, keys = guarded(torch, kb, GUARD + 1)
    bv, vals = guarded(torch, vb, GUARD + 3)
    bko, koff = guarded(torch, 8 * (n_out + 1))
    bvo, voff = guarded(torch, 8 * (n_out + 1))
    bd, dele = guarded(torch, n_out, GUARD + 5)
    bs, seq = guarded(torch, 8 * n_out)
    seb.dev_wal_replay_emit(dimg, doff, sizes, ws, keys, koff, vals, voff, dele, seq)
    torch.cuda.synchronize()
    u64 = lambda a: np.frombuffer(a.tobytes(), np.uint64)  # noqa: E731
    return (check_guards(bk, kb, GUARD + 1), u64(check_guards(bko, 8 * (n_out + 1))), check_guards(bv, vb, GUARD + 3),
            u64(check_guards(bvo, 8 * (n_out + 1))), check_guards(bd, n_out, GUARD + 5), u64(check_guards(bs, 8 * n_out)))


def compare_image(torch, seb, image, off, name=""):
    """Device against host half over a log image: the device's six arrays, read back once, and the sizes."""
    want = seb.wal_replay_emit(image, off)
    dimg, doff, ws, sizes = device_plan(torch, seb, image, off)
    assert sizes == want[6], (name, "sizes", sizes, want[6])
    got = device_emit(torch, seb, dimg, doff, ws, sizes)
    for j, what in enumerate(("keys", "key_off", "vals", "val_off", "deleted", "seq")):
        if not np.array_equal(got[j], want[j]):
            at = int(np.nonzero(got[j][:len(want[j])] != want[j][:len(got[j])])[0][0])
            raise AssertionError(f"{name}: {what} differs first at {at}: {got[j][at:at + 8]} != {want[j][at:at + 8]}")
    return got, sizes


def compare(torch, seb, recs, name="", ref=True):
    """Device against host half over a log of records; returns the replayed entries and the sizes."""
    image, off = mref.wal_image(recs)
    got, sizes = compare_image(torch, seb, image, off, name)
    ents = mref.unpack(*got)
    if ref:  # the restatement itself, where its sorted-slice inserts stay quick
        assert (ents, sizes) == mref.expected(recs), name
    return ents, sizes


def key8(i):
    return b"%08d" % i


# ------------------------------------------------------------------ shapes

@pytest.mark.parametrize("n", [0, 1, 2, T - 1, T, T + 1, 2 * T + 1, 3 * T, 5 * T + 7])
def test_record_counts(seb, torch_cuda, n):
    rng = np.random.default_rng(n)
    recs = mref.random_log(rng, n, max_key=60, max_val=120)
    got, sizes = compare(torch_cuda, seb, recs, f"n={n}")
    assert sizes[0] == n and sizes[1] == len({k for k, _, _, _ in recs})
    if n > T:
        assert sizes[4] > n // 3 and sizes[5] > 0


def test_one_key_throughout(seb, torch_cuda):
    recs = [(b"the-key-of-this-log", b"v%d" % i, 7 * i % 1000, 1 if i % 5 == 1 else 0) for i in range(2 * T + 3)]
    got, sizes = compare(torch_cuda, seb, recs, "one key")
    assert got == [(b"the-key-of-this-log", b"v%d" % (2 * T + 2), 0, 7 * (2 * T + 2) % 1000)]
    assert sizes[:2] == (2 * T + 3, 1) and sizes[4] == 2 * T + 2 and sizes[6] == 999


@pytest.mark.parametrize("order", ["descending", "random"])
def test_all_keys_distinct(seb, torch_cuda, order):
    n = 4 * T + 5
    ids = list(range(n - 1, -1, -1)) if order == "descending" else [int(i) for i in np.random.default_rng(1).permutation(n)]
    recs = [(key8(3 * i), b"val%d" % i, s, 1 if i % 11 == 0 else 0) for s, i in enumerate(ids)]
    got, sizes = compare(torch_cuda, seb, recs, order)
    assert [k for k, _, _, _ in got] == [key8(3 * i) for i in range(n)] and sizes[4] == 0


def test_a_keys_records_in_tiles_0_2_and_4(seb, torch_cuda):
    """The key's last record is in tile 4, so the winner crosses the boundary of every pass of a 5-tile tree."""
    n = 5 * T
    recs = [(key8(2 * i + 1), b"filler", i, 0) for i in range(n)]
    hot = key8(4000)  # sorts into the middle
    for j, at in enumerate((5, T - 1, 2 * T, 2 * T + 700, 4 * T + 1, 5 * T - 1)):
        recs[at] = (hot, b"hot%d" % j, 10 ** 6 - j, 1 if j == 3 else 0)
    got, sizes = compare(torch_cuda, seb, recs, "tiles 0, 2, 4")
    assert (hot, b"hot5", 0, 10 ** 6 - 5) in got and sizes[4] == 5 and sizes[6] == 10 ** 6
    # the same with the last record a Delete that carries value bytes
    recs[5 * T - 1] = (hot, b"carried", 1, 1)
    got, sizes = compare(torch_cuda, seb, recs, "tiles 0, 2, 4, deleted last")
    assert (hot, b"", 1, 1) in got and sizes[5] == 1


@pytest.mark.parametrize("below", [T - 4, T - 9, T])
def test_equal_keys_across_a_tile_edge_of_the_sorted_result(seb, torch_cuda, below):
    """`below` keys sort below the tie key, so its 9 records take places below .. below + 8 of the sorted records:
    across the first tile's edge (the survivor, the last of them, is the next tile's record and mark looks across
    the edge), ending exactly at it, and starting at it."""
    tie = key8(500000)
    rng = np.random.default_rng(below)
    recs = [(key8(i), b"b", i, 0) for i in range(below)] + [(key8(600000 + i), b"a", i, 0) for i in range(T + 300)]
    recs = [recs[int(i)] for i in rng.permutation(len(recs))]
    for j, at in enumerate(sorted(int(x) for x in rng.choice(len(recs), 9, replace=False))):
        recs.insert(at + j, (tie, b"tie%d" % j, 50 - j, 0))
    got, sizes = compare(torch_cuda, seb, recs, f"tie group after {below}")
    assert got[below] == (tie, b"tie8", 0, 42) and sizes[4] == 8 and sizes[1] == below + 1 + T + 300


# ------------------------------------------------------------------ key order

def test_go_string_order_and_prefix_ties(seb, torch_cuda):
    recs = mref.order_log()
    # with fillers so that the ties meet inside LDS sorts and across merge passes
    fill = [(b"f%07d" % i, b"", 5000 + i, 0) for i in range(2 * T)]
    mixed = []
    for i, r in enumerate(recs):
        mixed += fill[26 * i:26 * (i + 1)] + [r]
    mixed += fill[26 * len(recs):]
    got, sizes = compare(torch_cuda, seb, mixed, "go string order")
    ks = [k for k, _, _, _ in got if not k.startswith(b"f0")]
    assert ks == sorted(mref.ORDER_KEYS) and ks[0] == b""
    at = ks.index(b"a")
    assert ks[at:at + 3] == [b"a", b"a\x00", b"a\x00\x00"]
    assert all(v.startswith(b"round2-") for k, v, _, _ in got if not k.startswith(b"f0"))


def test_delete_then_put_and_put_then_delete(seb, torch_cuda):
    recs = [(b"dp", b"", 1, 1), (b"pd", b"put", 2, 0), (b"dp", b"put-after-delete", 3, 0), (b"pd", b"ignored", 4, 1),
            (b"dd", b"", 5, 1), (b"dd", b"x", 6, 1), (b"two", b"2", 7, 2), (b"ff", b"255", 8, 255)]
    got, sizes = compare(torch_cuda, seb, recs, "delete / put")
    assert got == [(b"dd", b"", 1, 6), (b"dp", b"put-after-delete", 0, 3), (b"ff", b"255", 0, 8), (b"pd", b"", 1, 4),
                   (b"two", b"2", 0, 7)]
    assert sizes == (8, 5, 11, 20, 3, 2, 8, 11 + 20 + 80)


def test_value_sizes_and_one_large_key_and_value(seb, torch_cuda):
    rng = np.random.default_rng(9)
    recs = mref.random_log(rng, 600, max_key=300, max_val=5000)
    recs = [(k, v if i % 3 else bytes(rng.integers(0, 256, int(rng.integers(0, 5001)), dtype=np.uint8)), s, f)
            for i, (k, v, s, f) in enumerate(recs)]
    big = bytes(rng.integers(0, 256, 69_999, dtype=np.uint8))
    recs[100:100] = [(big + b"b", b"first", 1, 0)]
    recs[300:300] = [(b"large-value", bytes(rng.integers(0, 256, 70_000, dtype=np.uint8)), 2, 0), (big + b"a", b"y", 3, 0)]
    recs[500:500] = [(big + b"b", b"second", 4, 0), (big + b"c", b"dead" * 20_000, 5, 1)]
    got, sizes = compare(torch_cuda, seb, recs, "sizes")
    by_key = {k: (v, d, s) for k, v, d, s in got}
    assert by_key[big + b"b"] == (b"second", 0, 4) and by_key[big + b"c"] == (b"", 1, 5)
    assert len(by_key[b"large-value"][0]) == 70_000
    ks = [k for k, _, _, _ in got]
    at = ks.index(big + b"a")
    assert ks[at:at + 3] == [big + b"a", big + b"b", big + b"c"]


# ------------------------------------------------------------------ many tiles

def passes_of(n):
    """The levels of the pairwise merge tree over the tiles of n records."""
    tiles, p = -(-n // T), 0
    while (1 << p) < tiles:
        p += 1
    return tiles, p


def check_closed_form(got, sizes, want, want_sizes, name):
    assert sizes == want_sizes, (name, sizes, want_sizes)
    for j, what in enumerate(("keys", "key_off", "vals", "val_off", "deleted", "seq")):
        assert np.array_equal(got[j], want[j]), (name, what, "differs from the closed form")


@pytest.mark.parametrize("distinct", [0, 1], ids=["few_keys", "distinct_keys"])
@pytest.mark.parametrize("n", [8 * T + 1, 16 * T, 17 * T - 5, 33 * T + 1])
def test_pass_tree_depth(seb, torch_cuda, n, distinct):
    """9, 16, 17 and 34 tiles: merge widths of 8 T and more, and trees whose last pair is one short tile (8 T + 1,
    33 T + 1) or a lopsided subtree (17 T - 5) against a full power of two.  Variable-length records: long
    equal-key groups, then mostly distinct keys.  Against the host half and against last-record-wins by a dict."""
    tiles, passes = passes_of(n)
    assert tiles in (9, 16, 17, 34) and passes >= 4 and (T << (passes - 1)) >= 8 * T  # a pass of width >= 8 T runs
    recs, image, off, want, want_sizes = sc.deep_log(n, distinct)
    got, sizes = compare_image(torch_cuda, seb, image, off, f"n={n}")
    assert sizes == want_sizes and mref.unpack(*got) == want
    assert (sizes[1] > n // 2) == bool(distinct) and sizes[5] > 0


def test_one_keys_group_over_more_than_two_tiles_at_depth(seb, torch_cuda):
    """17 tiles; one key holds 2 T + 5 records, some in every tile, so its group spans more than two whole tiles of
    the sorted records and every pass merges parts of it.  Its last record is a Delete that carries value bytes."""
    n, m = 17 * T, 2 * T + 5
    tiles, passes = passes_of(n)
    assert tiles == 17 and passes == 5 and m > 2 * T
    rng = np.random.default_rng(17)
    hot = key8(500000)  # sorts into the middle of the fillers
    recs = [(key8(2 * int(i) + 1), b"f%d" % i, 3 * s, int(s % 9 == 0)) for s, i in enumerate(rng.permutation(n))]
    per = [m // 17 + (t < m % 17) for t in range(17)]
    at = sorted(t * T + int(x) for t in range(17) for x in rng.choice(T, per[t], replace=False))
    assert len(at) == m and {a // T for a in at} == set(range(17))
    for j, a in enumerate(at):
        recs[a] = (hot, b"hot%d" % j, 10 ** 7 + 5 * j, 1 if j % 7 == 3 else 0)
    recs[at[-1]] = (hot, b"carried-by-the-delete", 77, 1)
    want, want_sizes = sc.last_wins(recs)
    got, sizes = compare(torch_cuda, seb, recs, "one key over 17 tiles", ref=False)
    assert (got, sizes) == (want, want_sizes)
    assert [e for e in got if e[0] == hot] == [(hot, b"", 1, 77)]
    assert sizes[1] == n - m + 1 and sizes[4] == m - 1 and sizes[6] == 10 ** 7 + 5 * (m - 2)


def test_cuts_second_workgroup(seb, torch_cuda):
    """130 tiles: 260 diagonal searches a pass, a lane each, 256 lanes to a workgroup of k_replay_cuts."""
    n = 129 * T + 3
    tiles, passes = passes_of(n)
    assert 2 * tiles > 256 and passes == 8
    image, off, want, want_sizes = sc.replay_log(n, 50_000)
    got, sizes = compare_image(torch_cuda, seb, image, off, "130 tiles")
    check_closed_form(got, sizes, want, want_sizes, "130 tiles")


def test_scan_carry_over_more_than_1024_tiles(seb, torch_cuda):
    """1026 tiles, 11 passes: k_replay_scan's second chunk takes the first chunk's sum as its carry, for the
    survivors' counts, key bytes and value bytes."""
    n = 1024 * T + 1025
    tiles, passes = passes_of(n)
    assert tiles > 1024 and -(-n // T) == 1026 and passes == 11
    image, off, want, want_sizes = sc.replay_log(n, 400_000)
    got, sizes = compare_image(torch_cuda, seb, image, off, "1026 tiles")
    check_closed_form(got, sizes, want, want_sizes, "1026 tiles")


# ------------------------------------------------------------------ errors

def test_bad_framing_far_from_tile_0(seb, torch_cuda):
    """Records 129 T + 1 and 129 T + 2, in the last of 130 tiles, are not framed: the lowest is named, in the host's words."""
    n = 129 * T + 3
    bad = 129 * T + 1
    assert bad // T >= 128 and bad + 1 < n
    image, off, _, _ = sc.replay_log(n, 50_000)
    img = image.copy()
    img[int(off[bad]) + 16] ^= 2  # valueSize: 21 + keySize + valueSize != the record's length
    img[int(off[bad + 1]) + 12] ^= 1  # and the next record's keySize
    with pytest.raises(seb.SebError) as host:
        seb.wal_replay_plan(img, off)
    with pytest.raises(seb.SebError) as ei:
        device_plan(torch_cuda, seb, img, off)  # checks the guard behind the workspace
    assert ei.value.code == -1 and f"record {bad} " in str(ei.value), str(ei.value)
    assert str(ei.value).split(": ", 2)[2] == str(host.value).split(": ", 2)[2]


@pytest.mark.parametrize("bad", [0, 1500, 2 * T + 99])
def test_bad_framing(seb, torch_cuda, bad):
    torch = torch_cuda
    recs = mref.random_log(np.random.default_rng(4), 2 * T + 100, max_key=40, max_val=60)
    image, off = mref.wal_image(recs)
    img = bytearray(image)
    img[off[bad] + 16] ^= 2  # valueSize: 21 + keySize + valueSize != the record's length
    if bad == 1500:  # a later bad record too: the lowest is named
        img[off[1900] + 12] ^= 1
    with pytest.raises(seb.SebError) as host:
        seb.wal_replay_plan(bytes(img), off)
    with pytest.raises(seb.SebError) as ei:
        device_plan(torch, seb, bytes(img), off)  # checks the guard behind the workspace
    assert ei.value.code == -1 and f"record {bad} " in str(ei.value), str(ei.value)
    assert str(ei.value).split(": ", 2)[2] == str(host.value).split(": ", 2)[2]
    # decreasing offsets at the first record
    with pytest.raises(seb.SebError) as ei:
        device_plan(torch, seb, image, [off[1] + 40] + off[1:])
    assert ei.value.code == -1 and "record 0:" in str(ei.value) and "decreases" in str(ei.value)


def test_stale_workspace_and_capacities(seb, torch_cuda):
    torch = torch_cuda
    recs = mref.random_log(np.random.default_rng(6), T + 300, max_key=40, max_val=60)
    image, off = mref.wal_image(recs)
    dimg, doff = dev_image(torch, image, off)
    need = seb.dev_wal_replay_workspace_size(len(recs))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    with pytest.raises(seb.SebError) as ei:
        seb.dev_wal_replay_plan(dimg, doff, ws, ws_bytes=need - 1)
    assert ei.value.code == -1 and "workspace" in str(ei.value)
    sizes = seb.dev_wal_replay_plan(dimg, doff, ws)
    assert sizes == seb.wal_replay_plan(image, off)
    n_in, n_out, kb, vb, ow, tomb, mseq, msize = sizes
    lens = (kb, 8 * (n_out + 1), vb, 8 * (n_out + 1), n_out, 8 * n_out)
    outs = [guarded(torch, size) for size in lens]
    blank = torch.zeros(need, dtype=torch.uint8, device="cuda")
    other = torch.zeros(need, dtype=torch.uint8, device="cuda")  # another log's plan
    image2, off2 = mref.wal_image(recs[:-1] + [(b"zzz", b"", 0, 0)])
    dimg2, doff2 = dev_image(torch, image2, off2)
    seb.dev_wal_replay_plan(dimg2, doff2, other)
    for bad_sizes, bad_ws in (((n_in, n_out - 1, kb, vb, ow + 1, tomb, mseq, msize - 16), ws),
                              ((n_in, n_out, kb - 1, vb, ow, tomb, mseq, msize - 1), ws), (sizes, blank), (sizes, other)):
        with pytest.raises(seb.SebError) as ei:
            seb.dev_wal_replay_emit(dimg, doff, bad_sizes, bad_ws, *[view for _, view in outs])
        assert ei.value.code == -1 and "plan" in str(ei.value)
    torch.cuda.synchronize()
    for (buf, _), size in zip(outs, lens):
        assert (buf.cpu().numpy() == 0xA5).all(), "a refused emit wrote an output"
    # the host-buffer form: each capacity one short is SEB_ERR_RANGE with the sizes filled
    for caps in ((kb - 1, vb, n_out), (kb, vb - 1, n_out), (kb, vb, n_out - 1)):
        with pytest.raises(seb.SebError) as ei:
            seb.wal_recover(image, caps=caps)
        assert ei.value.code == -4 and ei.value.sizes == sizes


def test_wal_recover(seb, torch_cuda):
    recs = mref.random_log(np.random.default_rng(7), 2 * T + 50, max_key=40, max_val=200)
    image, off = mref.wal_image(recs)
    want = seb.wal_replay_emit(image, off)
    for got in (seb.wal_recover(image), seb.wal_recover(image, caps=(want[6][2], want[6][3], want[6][1]))):
        assert got[6] == want[6] and all(np.array_equal(g, w) for g, w in zip(got[:6], want[:6]))
    assert (mref.unpack(*want[:6]), want[6]) == mref.expected(recs)
    empty = seb.wal_recover(b"")
    assert empty[6] == (0,) * 8 and empty[1].tolist() == [0]
    flipped = bytearray(image)
    for r in (1800, 700):  # payload bits of two records: the lowest is named
        flipped[off[r + 1] - 1] ^= 0x10
    with pytest.raises(seb.SebError) as ei:
        seb.wal_recover(bytes(flipped))
    assert ei.value.code == -1 and "WAL corruption detected: CRC mismatch (record 700)" in str(ei.value)
    for cut in (off[-1] - 1, off[-2] + 20, off[-2] + 3):  # inside the last record's payload and inside its header
        with pytest.raises(seb.SebError) as ei:
            seb.wal_recover(image[:cut])
        assert ei.value.code == -5, str(ei.value)
        with pytest.raises(seb.SebError) as ei:  # both at once: ReadAll meets the bad record first
            seb.wal_recover(bytes(flipped[:cut]))
        assert ei.value.code == -1 and "CRC mismatch (record 700)" in str(ei.value)


# ------------------------------------------------------------------ end to end

def test_replay_into_the_builder(seb, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(21)
    recs = [(key8(int(rng.integers(0, 2500))), b"val-%d" % i + b"." * int(rng.integers(0, 90)), i + 1,
             int(rng.random() < 0.15)) for i in range(3 * T + 11)]
    image, off = mref.wal_image(recs)
    dimg, doff, ws, sizes = device_plan(torch, seb, image, off)
    want, want_sizes = mref.expected(recs)
    assert sizes == want_sizes and 1500 < sizes[1] < 2500
    _, n_out, kb, vb = sizes[:4]
    keys = torch.zeros(kb + 16, dtype=torch.uint8, device="cuda")
    vals = torch.zeros(vb + 16, dtype=torch.uint8, device="cuda")
    koff = torch.zeros(n_out + 1, dtype=torch.int64, device="cuda")
    voff = torch.zeros(n_out + 1, dtype=torch.int64, device="cuda")
    dele = torch.zeros(n_out + 1, dtype=torch.uint8, device="cuda")
    seb.dev_wal_replay_emit(dimg, doff, sizes, ws, keys, koff, vals, voff, dele)  # no seq: the builder takes none
    fb = [0, n_out]
    dk = seb.dev_keys(keys, koff)
    sws = torch.zeros(seb.dev_sst_workspace_size(n_out, 1), dtype=torch.uint8, device="cuda")
    fs = seb.dev_sst_plan(dk, voff, fb, sws)
    data, index, meta = (torch.zeros(fs[0][j] + 16, dtype=torch.uint8, device="cuda") for j in (1, 2, 3))
    seb.dev_sst_encode(dk, vals, voff, dele, fb, fs, sws, data, index, meta)
    torch.cuda.synchronize()
    wd, wx, wm, _, _ = sr.sections([(k, v, d) for k, v, d, _ in want])
    assert data.cpu().numpy().tobytes()[:fs[0][1]] == wd
    assert index.cpu().numpy().tobytes()[:fs[0][2]] == wx and meta.cpu().numpy().tobytes()[:fs[0][3]] == wm
