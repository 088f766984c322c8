"""GPU: the batched compaction merge (include/seb_bloom.h, the compaction merge group).

seb_dev_merge_count / seb_dev_merge_plan / seb_dev_merge_emit equal the host half (seb_merge_plan /
seb_merge_emit, itself held to the restatements in test_merge.py) byte for byte: 1 to 9 runs (an odd number
makes the merge tree lopsided), run lengths around the merge tile T, ties in every run and across a tile
boundary of the last pass, Go string order on keys that tie in their first 16 and 40 bytes, tombstones, and
the pool's layouts.  Outputs start as 0xA5 between guard bytes and sit at odd addresses.  The merged run goes
straight into the device builder, whose files equal the restatement's.

Beyond six tiles, 135 blocks and 9 runs (each test asserts by arithmetic that its shape crosses its threshold,
and compares the device with the host half and with rule_merge or scale_ref's lexsort):
  pools of 255, 256, 257, 513 blocks     a non-zero group base in k_merge_spread; a run boundary at blocks 255,
                                         256 and 257; blocks without entries at 255, 256 and the pool's end
  16, 17, 33, 257, 1025 runs             pairs of 8 to 1024 runs, lopsided trees, every tenth run empty, a second
                                         workgroup of k_merge_runs; an unsorted run 600 behind two empty runs
  17 runs, some 139 tiles                a second workgroup of k_merge_cuts
  5 runs, more than 1024 tiles           the carry of k_merge_scan over the tiles' sums
The carry of the same k_merge_scan over the group sums needs more than 262,144 blocks, a pool of 1 GiB: it is
not run here."""
import numpy as np
import pytest

import block_ref as br
import merge_ref as mr
import scale_ref as sc
import sstable_ref as sr

pytestmark = pytest.mark.gpu

GUARD = 64
T = 1024  # the merge tile, the survivor-scan tile and the emit tile (seb.MERGE_TILE)


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


def dev_pool(torch, pool, blen):
    dpool = torch.from_numpy(np.concatenate([pool, np.zeros(16, np.uint8)])).cuda()
    dblen = torch.from_numpy(np.concatenate([blen, np.zeros(1, np.uint16)]).view(np.int16)).cuda()
    assert dpool.data_ptr() % 16 == 0
    return dpool, dblen


def device_plan(torch, seb, pool, blen, rb, flags=0, block_counts=None):
    """count + plan on the device: (dpool, ws, sizes); the counts are checked against loadBlock's, or against
    block_counts where a generator states them."""
    nb = len(blen)
    dpool, dblen = dev_pool(torch, pool, blen)
    bc, dcnt = guarded(torch, 2 * nb)
    run_entries = seb.dev_merge_count(dpool, dblen, rb, dcnt.view(torch.int16))
    counts = np.frombuffer(check_guards(bc, 2 * nb).tobytes(), np.uint16).tolist()
    want = block_counts if block_counts is not None else \
        [len(mr.load_block(bytes(pool[b * 4096:b * 4096 + min(int(blen[b]), 4096)]))) for b in range(nb)]
    assert counts == want
    assert run_entries == [sum(want[rb[r]:rb[r + 1]]) for r in range(len(rb) - 1)]
    n = sum(run_entries)
    ws = torch.full((seb.dev_merge_workspace_size(n, nb, len(rb) - 1) + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    try:
        sizes = seb.dev_merge_plan(dpool, dblen, rb, dcnt.view(torch.int16), ws, flags, ws_bytes=ws.numel() - 16)
    finally:  # accepted or refused, the plan writes its workspace alone: not past it, not the counts it reads
        torch.cuda.synchronize()
        assert (ws[-16:].cpu().numpy() == 0x5A).all(), "the plan wrote past its workspace"
        assert np.frombuffer(check_guards(bc, 2 * nb).tobytes(), np.uint16).tolist() == counts
    return dpool, ws, sizes


def device_emit(torch, seb, dpool, ws, sizes):
    """emit into guarded 0xA5 buffers, keys and values at odd addresses: the five arrays as numpy."""
    _, n_out, kb, vb, _, _ = sizes
    bk, keys = guarded(torch, kb, GUARD + 1)
    bv, vals = guarded(torch, vb, GUARD + 3)
    bko, koff = guarded(torch, 8 * (n_out + 1))
    bvo, voff = guarded(torch, 8 * (n_out + 1))
    bd, dele = guarded(torch, n_out, GUARD + 5)
    seb.dev_merge_emit(dpool, sizes, ws, keys, koff, vals, voff, dele)
    torch.cuda.synchronize()
    return (check_guards(bk, kb, GUARD + 1), np.frombuffer(check_guards(bko, 8 * (n_out + 1)).tobytes(), np.uint64),
            check_guards(bv, vb, GUARD + 3), np.frombuffer(check_guards(bvo, 8 * (n_out + 1)).tobytes(), np.uint64),
            check_guards(bd, n_out, GUARD + 5))


def compare(torch, seb, runs, flags=0, name="", **kw):
    """Device against host half over runs of block images; returns the merged items and the sizes."""
    got, sizes = compare_pool(torch, seb, *mr.pool_of(runs, **kw), flags, name)
    return mr.unpack(*got), sizes


def compare_pool(torch, seb, pool, blen, rb, flags=0, name="", block_counts=None):
    """Device against host half over a pool: the device's five arrays, read back once, and the sizes."""
    want = seb.merge_emit(pool, blen, rb, flags)
    dpool, ws, sizes = device_plan(torch, seb, pool, blen, rb, flags, block_counts)
    assert sizes == want[5], (name, "sizes")
    got = device_emit(torch, seb, dpool, ws, sizes)
    for j, what in enumerate(("keys", "key_off", "vals", "val_off", "deleted")):
        if not np.array_equal(got[j], want[j]):
            at = int(np.nonzero(got[j][:len(want[j])] != want[j][:len(got[j])])[0][0])
            raise AssertionError(f"{name}: {what} differs first at {at}: {got[j][at:at + 8]} != {want[j][at:at + 8]}")
    return got, sizes


def items_of(keys, r, rng=None, dels=0.0):
    return [(k, b"r%d:" % r + (bytes(rng.integers(0, 256, int(rng.integers(0, 30)), dtype=np.uint8)) if rng else b""),
             int(rng.random() < dels) if rng else 0) for k in keys]


def key8(i):
    return b"%08d" % i


# ------------------------------------------------------------------ shapes

@pytest.mark.parametrize("nruns", [1, 2, 3, 5, 8, 9])
def test_run_counts(seb, torch_cuda, nruns):
    rng = np.random.default_rng(nruns)
    runs = mr.random_runs(rng, nruns, 4000, share=0.25)
    blocks = [mr.run_blocks(run) for run in runs]
    got, sizes = compare(torch_cuda, seb, blocks, 0, f"R={nruns}", fill=0xCC)
    ents = mr.decoded(blocks)
    assert got == mr.as_bytes(mr.rule_merge(ents))
    assert [k for k, _, _ in got] == [e[0] for e in mr.go_merge(ents, 1)]
    assert (sizes[4] > 0) == (nruns > 1)
    if nruns == 1:  # the identity: the decode alone
        assert got == [(k, v, d) for k, v, d in runs[0]]
    compare(torch_cuda, seb, blocks, seb.MERGE_DROP_TOMBSTONES, f"R={nruns} drop", full_blen=True)


@pytest.mark.parametrize("length", [T - 1, T, T + 1, 2 * T + 1])
def test_tile_edges(seb, torch_cuda, length):
    rng = np.random.default_rng(length)
    one = [mr.run_blocks(items_of([key8(i) for i in range(length)], 0, rng, 0.1))]
    got, sizes = compare(torch_cuda, seb, one, 0, f"one run of {length}")
    assert sizes[:2] == (length, length)
    # two runs of this length perfectly interleaved, then a third of another length over the same range
    a = mr.run_blocks(items_of([key8(2 * i) for i in range(length)], 0, rng))
    b = mr.run_blocks(items_of([key8(2 * i + 1) for i in range(length)], 1, rng))
    c = mr.run_blocks(items_of([key8(3 * i) for i in range(T + 7)], 2, rng))
    got, sizes = compare(torch_cuda, seb, [a, b], 0, f"interleaved {length}")
    assert [k for k, _, _ in got] == [key8(i) for i in range(2 * length)]
    compare(torch_cuda, seb, [a, b, c], 0, f"three runs {length}")
    compare(torch_cuda, seb, [c, b, a], seb.MERGE_DROP_TOMBSTONES, f"three runs reversed {length}")


def test_below_and_empty_runs(seb, torch_cuda):
    rng = np.random.default_rng(5)
    low = mr.run_blocks(items_of([key8(i) for i in range(1500)], 0, rng))
    high = mr.run_blocks(items_of([key8(5000 + i) for i in range(1300)], 1, rng))
    got, _ = compare(torch_cuda, seb, [high, low], 0, "one run below another")
    assert [k for k, _, _ in got] == [key8(i) for i in range(1500)] + [key8(5000 + i) for i in range(1300)]
    compare(torch_cuda, seb, [low, high], 0, "one run above another")
    nothing = [br.encode_block([]), b"", b"\x07\x00\x00"]  # blocks without entries: count 0, 0 bytes, 3 bytes
    for runs, entries in (([[], low, high], 2800), ([low, [], high], 2800), ([low, high, []], 2800),
                          ([nothing, low, [], nothing, high, nothing], 2800), ([[], [], []], 0), ([nothing, [], nothing], 0)):
        got, sizes = compare(torch_cuda, seb, runs, 0, "empty runs", fill=0xCC)
        assert sizes[:2] == (entries, entries)


def test_nothing_to_merge(seb, torch_cuda):
    torch = torch_cuda
    assert seb.dev_merge_count(None, None, [0, 0], None) == [0]
    assert seb.dev_merge_plan(None, None, [], None, None) == (0,) * 6
    sizes = seb.dev_merge_plan(None, None, [0, 0, 0], None, None)
    assert sizes == (0,) * 6
    bko, koff = guarded(torch, 8)
    bvo, voff = guarded(torch, 8)
    seb.dev_merge_emit(None, sizes, None, None, koff, None, voff, None)  # entries_in == 0: nothing is launched
    torch.cuda.synchronize()
    assert not check_guards(bko, 8).any() and not check_guards(bvo, 8).any()
    out = seb.merge(np.zeros(0, np.uint8), np.zeros(0, np.uint16), [0, 0])
    assert out[1].tolist() == [0] and out[5] == (0,) * 6


# ------------------------------------------------------------------ ties

def test_one_key_in_every_run(seb, torch_cuda):
    runs = [[br.encode_block([(b"the-key", b"run%d" % r, 1 if r == 4 else 0)])] for r in range(9)]
    got, sizes = compare(torch_cuda, seb, runs, 0, "one key, 9 runs")
    assert got == [(b"the-key", b"run0", 0)] and sizes == (9, 1, 7, 4, 8, 0)


def test_tie_group_across_a_tile_boundary(seb, torch_cuda):
    """T - 4 keys below the tie key, all in run 0: the 9 equal keys take outputs T - 4 .. T + 4 of the last
    pass (runs 0-7 against run 8), of the survivor scan and of the emit."""
    tie = key8(500000)
    runs = [mr.run_blocks(items_of([key8(i) for i in range(T - 4)] + [tie] + [key8(600000 + i) for i in range(300)], 0))]
    for r in range(1, 9):
        runs.append(mr.run_blocks(items_of([tie] + [key8(700000 + 1000 * r + i) for i in range(200)], r)))
    got, sizes = compare(torch_cuda, seb, runs, 0, "tie group across a tile")
    assert got[T - 4] == (tie, b"r0:", 0) and sizes[4] == 8
    assert len({k for k, _, _ in got}) == len(got)


def test_every_key_in_every_run(seb, torch_cuda):
    keys = [key8(7 * i) for i in range(1300)]
    runs = [mr.run_blocks(items_of(keys, r)) for r in range(5)]
    got, sizes = compare(torch_cuda, seb, runs, 0, "every key in every run")
    assert got == items_of(keys, 0) and sizes[4] == 4 * len(keys)


# ------------------------------------------------------------------ key order

def test_go_string_order(seb, torch_cuda):
    p40 = b"0123456789abcdef" * 2 + b"01234567"
    long = b"L" * 4082
    keys = set(br.ORDER_KEYS) | {p40, p40 + b"\x00", p40 + b"a", p40 + b"\x80", p40 + b"\xff\x01", p40[:39], p40[:39] + b"\x7f"}
    keys = sorted(keys)
    runs = [[], [], []]
    for i, k in enumerate(keys):
        runs[i % 3].append((k, b"r%d" % (i % 3), 0))
        if i % 5 == 0 and i % 3 != 2:  # shared with run 2, as a tombstone that must lose
            runs[2].append((k, b"dup", 1))
    # keys of 4,083 bytes (one entry fills a block), equal up to their last byte, in three runs, one of them twice
    runs[0] += [(long + b"b", b"", 0), (long + b"\x80", b"", 0)]
    runs[1] += [(long + b"a", b"", 0), (long + b"b", b"", 1)]
    runs[2] += [(long + b"\x7f", b"", 0)]
    blocks = [mr.run_blocks(sorted(run)) for run in runs]
    got, sizes = compare(torch_cuda, seb, blocks, 0, "go string order")
    ents = mr.decoded(blocks)
    assert got == mr.as_bytes(mr.rule_merge(ents))
    ks = [k for k, _, _ in got]
    assert ks == sorted(ks) and ks[0] == b"" and ks.index(b"ab") + 2 == ks.index(b"ab\x00\x00")
    at = ks.index(long + b"a")
    assert ks[at:at + 4] == [long + b"a", long + b"b", long + b"\x7f", long + b"\x80"] and got[at + 1][2] == 0
    assert all(d == 0 for _, _, d in got) and sizes[4] > 5


# ------------------------------------------------------------------ tombstones

def test_tombstones(seb, torch_cuda):
    r0 = [br.encode_block([(b"a", b"0a", 1), (b"b", b"0b", 0), (b"c", b"0c", 2), (b"d", b"0d", 255)])]
    r1 = [br.encode_block([(b"b", b"1b", 1), (b"e", b"1e", 1)])]
    r2 = [br.encode_block([(b"a", b"2a", 0), (b"e", b"2e", 0)])]
    got, sizes = compare(torch_cuda, seb, [r0, r1, r2], 0, "tombstones kept")
    assert got == [(b"a", b"0a", 1), (b"b", b"0b", 0), (b"c", b"0c", 0), (b"d", b"0d", 0), (b"e", b"1e", 1)]
    got, sizes = compare(torch_cuda, seb, [r0, r1, r2], seb.MERGE_DROP_TOMBSTONES, "tombstones dropped")
    assert got == [(b"b", b"0b", 0), (b"c", b"0c", 0), (b"d", b"0d", 0)] and sizes == (8, 3, 3, 6, 3, 2)
    dead = mr.run_blocks([(key8(i), b"x", 1) for i in range(T + 50)])
    got, sizes = compare(torch_cuda, seb, [dead], seb.MERGE_DROP_TOMBSTONES, "all tombstones")
    assert got == [] and sizes == (T + 50, 0, 0, 0, 0, T + 50)
    live = mr.run_blocks([(key8(2 * i), b"live", 0) for i in range(T)])
    got, sizes = compare(torch_cuda, seb, [dead, live], seb.MERGE_DROP_TOMBSTONES, "tombstones over live values")
    assert [k for k, _, _ in got] == [key8(2 * i) for i in range((T + 50 + 1) // 2, T)]


# ------------------------------------------------------------------ layout

@pytest.mark.parametrize("full_blen", [False, True])
def test_value_sizes_and_pool_layout(seb, torch_cuda, full_blen):
    rng = np.random.default_rng(9)
    big = [(b"big%03d" % i, bytes(rng.integers(0, 256, 4083 - 6, dtype=np.uint8)), 0) for i in range(40)]  # 4092-byte entries
    none = [(b"none%04d" % i, b"", i % 3 == 0) for i in range(1500)]
    mixed = sr.random_items(rng, 1200, max_key=30, max_val=500)
    mixed = [(k, v, 1 if d == 1 else 0) for k, v, d in mixed]
    a, b, c = mr.run_blocks(big), mr.run_blocks(none), mr.run_blocks(mixed)
    # slots that hold no entries inside and between the runs: with a true blen (0) their 0xEE bytes are never
    # read, with blen = 4096 they are zero and read as a block of no entries
    hole = [b""]
    runs = [hole + a[:20] + hole + a[20:], hole, b + hole, c]
    got, sizes = compare(torch_cuda, seb, runs, 0, f"layout full_blen={full_blen}", full_blen=full_blen, fill=0xEE)
    assert sizes[0] == len(big) + len(none) + len(mixed)
    assert got == mr.as_bytes(mr.rule_merge(mr.decoded(runs)))


# ------------------------------------------------------------------ many blocks, many runs, many tiles

def passes_of(nruns):
    p = 0
    while (1 << p) < nruns:
        p += 1
    return p


def check_closed_form(got, sizes, want, name):
    arrays, want_sizes = want
    assert sizes == want_sizes, (name, sizes, want_sizes)
    for j, what in enumerate(("keys", "key_off", "vals", "val_off", "deleted")):
        assert np.array_equal(got[j], arrays[j]), (name, what, "differs from the closed form")


@pytest.mark.parametrize("nb,bounds", sc.GROUP_POOLS, ids=[f"{nb}-{b[2]}" for nb, b in sc.GROUP_POOLS])
def test_block_groups(seb, torch_cuda, nb, bounds):
    """Pools of 255, 256, 257 and 513 blocks, a group of the first[] scan being 256: k_merge_spread adds a
    non-zero group base from block 256 on; a run boundary at blocks 255, 256 and 257 makes rf[] read first[] just
    before, at and just after a group edge; blocks 255, 256 and the last hold no entries."""
    groups = -(-nb // 256)
    assert groups == {255: 1, 256: 1, 257: 2, 513: 3}[nb] and (nb <= 256 or nb > 256 and groups >= 2)
    if nb == 513:
        assert nb // 256 >= 2 and bounds[2] in (255, 256, 257)
    runs = sc.group_runs(nb, bounds)
    flat = [img for run in runs for img in run]
    assert len(flat) == nb and all(len(mr.load_block(flat[b])) == (0 if b in (255, 256, nb - 1) else 3) for b in range(nb))
    ents = mr.decoded(runs)
    for flags in (0, seb.MERGE_DROP_TOMBSTONES):
        got, sizes = compare(torch_cuda, seb, runs, flags, f"{nb} blocks, flags {flags}", fill=0xCC)  # counts against load_block
        assert got == mr.as_bytes(mr.rule_merge(ents, bool(flags))) and sizes[4] > 0


@pytest.mark.parametrize("nruns", [16, 17, 33, 257, 1025])
def test_many_runs(seb, torch_cuda, nruns):
    """16 to 1025 runs of 0 to 20 entries, every tenth run empty: pairs of 8, 16, ... 1024 runs (merge_tile and the
    host's tile table), a lopsided tree (17, 33, 257, 1025), rf[] with equal neighbours, and from 256 runs on a
    second workgroup of k_merge_runs."""
    passes = passes_of(nruns)
    assert passes >= 4 and (1 << (passes - 1)) >= (16 if nruns > 16 else 8)  # the widest pair's side, in runs
    if nruns > 256:
        assert (nruns + 1 + 255) // 256 >= 2  # k_merge_runs: a lane per rf[0 .. nruns]
    blocks = [mr.run_blocks(run) for run in sc.many_runs(nruns)]
    assert sum(not run for run in blocks) >= nruns // 10 and not blocks[9]
    ents = mr.decoded(blocks)
    for flags in (0, seb.MERGE_DROP_TOMBSTONES):
        got, sizes = compare(torch_cuda, seb, blocks, flags, f"{nruns} runs, flags {flags}")
        assert got == mr.as_bytes(mr.rule_merge(ents, bool(flags))) and sizes[4] > 0
        assert (sizes[5] > 0) == bool(flags)


def test_unsorted_run_above_256_is_refused(seb, torch_cuda):
    """Run 600 of 1025 is not increasing at its entry 5 and runs 598 and 599 are empty: k_merge_check's bisection
    over rf[] must land on run 600, not on an empty run with the same first record.  Run 900 is bad as well."""
    bad = 600
    assert bad > 256
    runs = [list(run) for run in sc.many_runs(1025)]
    runs[bad - 2] = []
    assert not runs[bad - 1] and not runs[bad - 2]
    for r, at in ((bad, 5), (900, 3)):
        run = [(key8(7 * i), b"bad%d" % r, 0) for i in range(12)]
        run[at - 1], run[at] = run[at], run[at - 1]
        runs[r] = run
    pool, blen, rb = mr.pool_of([mr.run_blocks(run) for run in runs])
    with pytest.raises(seb.SebError) as host:
        seb.merge_plan(pool, blen, rb)
    with pytest.raises(seb.SebError) as ei:
        device_plan(torch_cuda, seb, pool, blen, rb)
    assert ei.value.code == -1 and f"run {bad} entry 5 " in str(ei.value), str(ei.value)
    assert str(ei.value).split(": ", 2)[2] == str(host.value).split(": ", 2)[2]


@pytest.mark.parametrize("flags", [0, 1], ids=["keep", "drop_tombstones"])
def test_cuts_second_workgroup(seb, torch_cuda, flags):
    """17 runs over some 139 tiles: the last passes have more than 128 tiles, so k_merge_cuts' searches, a lane
    each, fill more than one workgroup of 256."""
    pool, blen, rb, want = sc.merge_pool(140 * T, 17, 400_000)
    n = want[flags][1][0]
    assert 2 * (-(-n // T)) > 256 and passes_of(17) == 5 and len(blen) // 256 >= 2
    got, sizes = compare_pool(torch_cuda, seb, pool, blen, rb, flags, "139 tiles", ((blen.astype(np.int64) - 4) // 21).tolist())
    check_closed_form(got, sizes, want[flags], "139 tiles")


@pytest.mark.parametrize("flags", [0, 1], ids=["keep", "drop_tombstones"])
def test_scan_carry_over_more_than_1024_tiles(seb, torch_cuda, flags):
    """5 runs of some 210,000 entries: more than 1024 tiles go into the survivor scan, so k_merge_scan's second
    chunk takes the first chunk's sum as its carry (counts, key bytes, value bytes); 21 groups of blocks."""
    pool, blen, rb, want = sc.merge_pool(1024 * T + 40_000, 5, 3_000_000)
    n = want[flags][1][0]  # entries in, after each run's draws lost their duplicates
    assert -(-n // T) > 1024 and len(blen) // 256 >= 2
    got, sizes = compare_pool(torch_cuda, seb, pool, blen, rb, flags, "1026 tiles", ((blen.astype(np.int64) - 4) // 21).tolist())
    assert sizes[0] == n
    check_closed_form(got, sizes, want[flags], "more than 1024 tiles")


# ------------------------------------------------------------------ errors

def test_unsorted_run_is_refused(seb, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(4)
    good = [mr.run_blocks(items_of([key8(3 * i + r) for i in range(1200)], r, rng)) for r in range(3)]
    swapped = [(key8(i), b"v", 0) for i in range(900)]
    swapped[700], swapped[701] = swapped[701], swapped[700]
    dup = [(key8(40 if i == 41 else i), b"v", 0) for i in range(300)]  # two equal neighbours
    bad = [br.encode_block(swapped[j:j + 100]) for j in range(0, 900, 100)]
    bad2 = [br.encode_block(dup[j:j + 100]) for j in range(0, 300, 100)]
    pool, blen, rb = mr.pool_of([good[0], good[1], bad, good[2], bad2])
    for call in (lambda: seb.merge_plan(pool, blen, rb), lambda: device_plan(torch, seb, pool, blen, rb),
                 lambda: seb.merge(pool, blen, rb)):
        with pytest.raises(seb.SebError) as ei:
            call()
        assert ei.value.code == -1 and "run 2 entry 701" in str(ei.value), str(ei.value)
    pool, blen, rb = mr.pool_of([good[0], bad2])
    with pytest.raises(seb.SebError) as ei:
        device_plan(torch, seb, pool, blen, rb)
    assert ei.value.code == -1 and "run 1 entry 41" in str(ei.value), str(ei.value)
    # the plan takes no output array: what a refused plan may have touched is its workspace, and device_plan
    # checks the 16 bytes behind the workspace and the count buffer's guards after every plan, refused or not


def test_short_workspace_and_capacities(seb, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(6)
    runs = [mr.run_blocks(items_of([key8(2 * i + r) for i in range(700)], r, rng)) for r in range(2)]
    pool, blen, rb = mr.pool_of(runs)
    nb = len(blen)
    dpool, dblen = dev_pool(torch, pool, blen)
    dcnt = torch.zeros(nb, dtype=torch.int16, device="cuda")
    n = sum(seb.dev_merge_count(dpool, dblen, rb, dcnt))
    need = seb.dev_merge_workspace_size(n, nb, 2)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    with pytest.raises(seb.SebError) as ei:
        seb.dev_merge_plan(dpool, dblen, rb, dcnt, ws, ws_bytes=need - 1)
    assert ei.value.code == -1 and "workspace" in str(ei.value)
    sizes = seb.dev_merge_plan(dpool, dblen, rb, dcnt, ws)
    assert sizes == seb.merge_plan(pool, blen, rb)
    # emit with sizes that are not this plan's, or with a workspace that holds no plan: refused, nothing written
    n_in, n_out, kb, vb, sh, dr = sizes
    outs = [guarded(torch, size) for size in (kb, 8 * (n_out + 1), vb, 8 * (n_out + 1), n_out)]
    blank = torch.zeros(need, dtype=torch.uint8, device="cuda")
    for bad_sizes, bad_ws in (((n_in, n_out - 1, kb, vb, sh + 1, dr), ws), ((n_in, n_out, kb - 1, vb, sh, dr), ws), (sizes, blank)):
        with pytest.raises(seb.SebError) as ei:
            seb.dev_merge_emit(dpool, bad_sizes, bad_ws, *[view for _, view in outs])
        assert ei.value.code == -1 and "plan" in str(ei.value)
    torch.cuda.synchronize()
    for (buf, _), size in zip(outs, (kb, 8 * (n_out + 1), vb, 8 * (n_out + 1), n_out)):
        assert (buf.cpu().numpy() == 0xA5).all(), "a refused emit wrote an output"
    # the host-buffer form: each capacity one short is SEB_ERR_RANGE with the sizes filled
    _, n_out, kb, vb, _, _ = sizes
    for caps in ((kb - 1, vb, n_out), (kb, vb - 1, n_out), (kb, vb, n_out - 1)):
        with pytest.raises(seb.SebError) as ei:
            seb.merge(pool, blen, rb, caps=caps)
        assert ei.value.code == -4 and ei.value.sizes == sizes
    want = seb.merge_emit(pool, blen, rb)
    for got in (seb.merge(pool, blen, rb, caps=(kb, vb, n_out)), seb.merge(pool, blen, rb)):
        assert got[5] == want[5] and all(np.array_equal(g, w) for g, w in zip(got[:5], want[:5]))


# ------------------------------------------------------------------ end to end

def sst_files(torch, seb, dpool, ws, sizes, per_file):
    """The merged run on the device straight into the device builder: per output file (data, index, metadata)."""
    _, n_out, kb, vb, _, _ = sizes
    keys = torch.zeros(kb + 16, dtype=torch.uint8, device="cuda")
    vals = torch.zeros(vb + 16, dtype=torch.uint8, device="cuda")
    koff = torch.zeros(n_out + 1, dtype=torch.int64, device="cuda")
    voff = torch.zeros(n_out + 1, dtype=torch.int64, device="cuda")
    dele = torch.zeros(n_out + 1, dtype=torch.uint8, device="cuda")
    seb.dev_merge_emit(dpool, sizes, ws, keys, koff, vals, voff, dele)
    fb = [min(f * per_file, n_out) for f in range(-(-n_out // per_file) + 1)]
    dk = seb.dev_keys(keys, koff)
    sws = torch.zeros(seb.dev_sst_workspace_size(n_out, len(fb) - 1), dtype=torch.uint8, device="cuda")
    fs = seb.dev_sst_plan(dk, voff, fb, sws)
    d, x, m = (sum(s[j] for s in fs) for j in (1, 2, 3))
    data, index, meta = (torch.zeros(v + 16, dtype=torch.uint8, device="cuda") for v in (d, x, m))
    seb.dev_sst_encode(dk, vals, voff, dele, fb, fs, sws, data, index, meta)
    torch.cuda.synchronize()
    data, index, meta = (t.cpu().numpy().tobytes() for t in (data, index, meta))
    out, at = [], [0, 0, 0]
    for s in fs:
        out.append((data[at[0]:at[0] + s[1]], index[at[1]:at[1] + s[2]], meta[at[2]:at[2] + s[3]]))
        at = [at[0] + s[1], at[1] + s[2], at[2] + s[3]]
    return out


@pytest.mark.parametrize("shared", [True, False])
def test_merge_into_the_builder(seb, torch_cuda, shared):
    torch = torch_cuda
    rng = np.random.default_rng(21 + shared)
    files = []
    for r in range(5):  # overlapping key ranges; with `shared` every 9th key of a file is also the next file's
        ids = sorted(set(int(i) for i in rng.integers(400 * r, 400 * r + 1500, 1100)))
        ids = [5 * i + (0 if shared and i % 9 == 0 else r) for i in ids]
        files.append([(key8(i), b"file%d-%d" % (r, i) + b"." * int(rng.integers(0, 90)), int(rng.random() < 0.15))
                      for i in sorted(set(ids))])
    blocks = [mr.run_blocks(f) for f in files]  # each file's data section as sstable_ref writes it
    ents = mr.decoded(blocks)
    common = sum(len({k for k, _, _ in a} & {k for k, _, _ in b}) for i, a in enumerate(files) for b in files[i + 1:])
    assert (common > 0) == shared
    for level in (1, 4):
        flags = seb.MERGE_DROP_TOMBSTONES if level == 4 else 0
        want = mr.rule_merge(ents, level == 4) if shared else mr.go_merge(ents, level)
        pool, blen, rb = mr.pool_of(blocks, full_blen=True)
        dpool, ws, sizes = device_plan(torch, seb, pool, blen, rb, flags)
        assert sizes[1] == len(want) > 3000
        got = sst_files(torch, seb, dpool, ws, sizes, 1000)
        assert len(got) == -(-len(want) // 1000)
        for f, (data, index, meta) in enumerate(got):
            wd, wx, wm, _, _ = sr.sections(mr.as_bytes(want[1000 * f:1000 * (f + 1)]))
            assert data == wd and index == wx and meta == wm, f"level {level}, output file {f}"
        host = seb.merge(pool, blen, rb, flags)
        assert mr.unpack(*host[:5]) == mr.as_bytes(want) and host[5] == sizes
