"""GPU: the Get path (include/seb_bloom.h, the Get path group).

seb_dev_get_compact_plan + seb_dev_get_compact_emit equal the host half (seb_get_compact, itself held to
getpath_ref's restatement in test_getpath.py) in sizes, out_keys, out_off and row: batch sizes around a wave, around
1, 2 and 4 tiles of 1024 keys and one that needs two stretches of the tile-sum scan; decided patterns none, all,
alternating, one undecided key first or last, decided runs covering whole waves and whole tiles, random fractions;
every key layout (aligned stride 16: the fast path; stride 16 at an odd source or an odd destination; strides 5 and
24; offsets with offsets[0] != 0 at an odd address, key lengths 0..300, long keys across a tile boundary).  Outputs
start as 0xA5 between guard bytes.  A workspace that is not the plan of the sizes it is used with makes the emit
write nothing, and statuses rewritten between plan and emit leave every guard intact.  seb_dev_get_join_rows: the
truth table, the bad-row rules, each nullable argument left out in turn, n == 0 and m == 0.  End to end: LSM.Get over
two memtable runs and four SSTables on two levels, the whole batch through the SSTable steps against the compacted
batch, both against getpath_ref."""
import ctypes as C

import numpy as np
import pytest

import getpath_ref as pref
import keygen as kg
import memget_ref as gref
from oracle import bloom_np as bn
from oracle import oracle_c as oc

pytestmark = pytest.mark.gpu

GUARD = 64
TILE = 1024  # kGetTile
NO_ID = 2**32 - 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def u64_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def odd_view(torch, a, lead=1):
    buf = torch.from_numpy(np.concatenate([np.full(lead, 0xEE, np.uint8), np.asarray(a, np.uint8).reshape(-1)])).cuda()
    return buf[lead:]


class Batch:
    """A key batch on the host (what seb.get_compact takes) and how to put it on the device."""

    def __init__(self, host, n, stride=None, odd=False):
        self.host, self.n, self.stride, self.odd = host, n, stride, odd

    def dev(self, torch, seb):
        if self.stride is None:
            data, off = self.host
            d = odd_view(torch, data)
            assert d.data_ptr() % 2 == 1 and (self.n == 0 or off[0] != 0)
            return seb.dev_keys(d, u64_dev(torch, off))
        flat = self.host.reshape(-1)
        d = odd_view(torch, flat) if self.odd else torch.from_numpy(flat.copy() if flat.size else np.zeros(16, np.uint8)).cuda()
        assert self.n == 0 or d.data_ptr() % 16 == (1 if self.odd else 0)
        return seb.dev_keys(d, n=self.n, stride=self.stride)


def fixed_batch(rng, n, stride, odd=False):
    return Batch(rng.integers(0, 256, (n, stride), dtype=np.uint8), n, stride, odd)


def varlen_batch(rng, n, max_len=300, long_at=()):
    lens = rng.integers(0, max_len + 1, n)
    lens[rng.random(n) < 0.2] = 0
    for i in long_at:
        if i < n:
            lens[i] = max_len
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64) + np.uint64(5)
    data = rng.integers(0, 256, int(off[-1]) + 3, dtype=np.uint8)
    return Batch((data, off), n)


def decided(rng, n, k=None):
    """k (a mask, or None for all) decided: FOUND or TOMBSTONE; the others a mix of the undecided bytes 0, 3, 255."""
    mem = rng.choice(np.array([0, 0, 0, 3, 255], np.uint8), n)
    dec = rng.choice(np.array([1, 2], np.uint8), n)
    return dec if k is None else np.where(k, dec, mem).astype(np.uint8)


def patterns(rng, n):
    i = np.arange(n)
    out = [("none", decided(rng, n, np.zeros(n, bool))), ("all", decided(rng, n)), ("alternating", decided(rng, n, i % 2 == 0)),
           ("first", decided(rng, n, i != 0)), ("last", decided(rng, n, i != n - 1)),
           ("runs", decided(rng, n, ((i >= 64) & (i < 128)) | ((i >= 256) & (i < 512)) | ((i >= 1024) & (i < 2048)) |
                            ((i >= 3072) & (i < 3072 + 256))))]
    for f in (0.1, 0.5, 0.9):
        out.append((f"random {f}", decided(rng, n, rng.random(n) < f)))
    return out


def device_compact(torch, seb, batch, mem, out_odd=False, emit_mem=None, sizes=None, ws=None, check_ws=True):
    """plan + emit into 0xA5 buffers between guards.  Returns (sizes tuple, out_keys, out_off or None, row) as
    numpy arrays, sized by the plan.  emit_mem: other statuses for the emit; sizes / ws: another plan's."""
    dk = batch.dev(torch, seb)
    n = dk.n
    dmem = odd_view(torch, mem, 3)
    need = seb.dev_get_compact_workspace_size(n)
    assert need == 128 + (2 * 8 * ((n + TILE - 1) // TILE) + 15) // 16 * 16
    own_ws = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    plan = seb.dev_get_compact_plan(dk, dmem, own_ws, ws_bytes=need)
    torch.cuda.synchronize()
    assert (own_ws[need:].cpu().numpy() == 0x5A).all(), "the plan wrote past its workspace"
    sz = plan if sizes is None else sizes
    m, kbytes = sz.undecided, sz.key_bytes
    lead = 1 if out_odd else 0
    kbuf = torch.full((GUARD + lead + kbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    obuf = torch.full((GUARD + 8 * (m + 1) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    rbuf = torch.full((GUARD + 4 * m + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out_keys = kbuf[GUARD + lead: GUARD + lead + kbytes]
    assert out_keys.data_ptr() % 16 == lead or kbytes == 0
    varlen = batch.stride is None
    demit = dmem if emit_mem is None else odd_view(torch, emit_mem, 3)
    ck, _ = seb.dev_get_compact_emit(dk, demit, sz, own_ws if ws is None else ws, out_keys,
                                     obuf[GUARD: GUARD + 8 * (m + 1)] if varlen else None, rbuf[GUARD: GUARD + 4 * m])
    torch.cuda.synchronize()
    assert ck.n == m and ck.stride == (0 if varlen else batch.stride)
    hk, ho, hr = kbuf.cpu().numpy(), obuf.cpu().numpy(), rbuf.cpu().numpy()
    assert (hk[:GUARD + lead] == 0xA5).all() and (hk[GUARD + lead + kbytes:] == 0xA5).all(), "bytes outside out_keys were written"
    assert (ho[:GUARD] == 0xA5).all() and (ho[GUARD + 8 * (m + 1):] == 0xA5).all(), "bytes outside out_off were written"
    assert (hr[:GUARD] == 0xA5).all() and (hr[GUARD + 4 * m:] == 0xA5).all(), "bytes outside row were written"
    if not varlen:
        assert (ho == 0xA5).all(), "out_off of a fixed-stride batch was written"
    if check_ws and ws is None:
        assert (own_ws[need:].cpu().numpy() == 0x5A).all()
    return (plan.as_tuple(), hk[GUARD + lead: GUARD + lead + kbytes],
            np.frombuffer(ho[GUARD: GUARD + 8 * (m + 1)].tobytes(), np.uint64) if varlen else None,
            np.frombuffer(hr[GUARD: GUARD + 4 * m].tobytes(), np.uint32), kbuf, obuf, rbuf, own_ws, plan)


def compare(torch, seb, batch, mem, name, out_odd=False):
    got = device_compact(torch, seb, batch, mem, out_odd)
    want = seb.get_compact(batch.host, mem)
    assert got[0] == want[0], f"{name}: sizes {got[0]} != {want[0]}"
    assert np.array_equal(got[3], want[3]), f"{name}: row"
    if want[2] is not None and want[0][1]:  # with no undecided key the emit launches nothing: out_off[0] is not written
        assert np.array_equal(got[2], want[2]), f"{name}: out_off"
    if not np.array_equal(got[1], want[1]):
        at = int(np.nonzero(got[1] != want[1])[0][0])
        raise AssertionError(f"{name}: out_keys differs first at byte {at} of {want[1].size}")
    return got


SIZES = [0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 4 * TILE - 1,
         4 * TILE, 4 * TILE + 1]


@pytest.mark.parametrize("n", SIZES)
def test_aligned_16_byte_keys(seb, torch_cuda, n):
    """The fast path: one 16-byte load and one 16-byte store per surviving key."""
    rng = np.random.default_rng(100 + n)
    batch = fixed_batch(rng, n, 16)
    for name, mem in patterns(rng, n):
        got = compare(torch_cuda, seb, batch, mem, f"n={n}, {name}")
        if name == "all" or n == 0:
            assert got[0][1:] == (0, 0)
        if name == "none":
            assert got[0] == (n, n, 16 * n)


def test_two_stretches_of_the_tile_scan(seb, torch_cuda):
    """200,000 16-byte keys are 196 tiles: more than the 128 the scan takes in one stretch, so the carry counts."""
    n = 200_000
    rng = np.random.default_rng(7)
    batch = fixed_batch(rng, n, 16)
    assert (n + TILE - 1) // TILE > 128
    for f in (0.1, 0.5, 0.9):
        compare(torch_cuda, seb, batch, decided(rng, n, rng.random(n) < f), f"fraction {f}")
    compare(torch_cuda, seb, batch, decided(rng, n, np.arange(n) < 140 * TILE), "the first stretch decided")


LAYOUTS = ["fixed16_odd_src", "fixed16_odd_dst", "stride5", "stride24", "offsets"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", [0, 1, 65, 257, TILE - 1, TILE + 1, 2 * TILE + 1, 4 * TILE + 1])
def test_every_other_layout(seb, torch_cuda, layout, n):
    rng = np.random.default_rng(200 + n)
    if layout == "offsets":
        # keys of 300 bytes on both sides of every tile boundary: longer than a 16-byte chunk, at any alignment
        batch = varlen_batch(rng, n, long_at=(TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, 4 * TILE - 1, 4 * TILE))
    else:
        batch = fixed_batch(rng, n, {"stride5": 5, "stride24": 24}.get(layout, 16), odd=layout == "fixed16_odd_src")
    for name, mem in patterns(rng, n):
        if name in ("first", "last", "random 0.1", "random 0.9") and n > 300:
            continue  # the rank logic is the aligned test's; here the byte copy is what differs
        compare(torch_cuda, seb, batch, mem, f"{layout}, n={n}, {name}", out_odd=layout == "fixed16_odd_dst")


def test_empty_keys_and_long_keys(seb, torch_cuda):
    """A batch of empty keys only; and undecided 300-byte keys right at a tile boundary between decided ones."""
    rng = np.random.default_rng(3)
    n = 1500
    empty = Batch((np.full(8, 0xEE, np.uint8), np.full(n + 1, 5, np.uint64)), n)
    got = compare(torch_cuda, seb, empty, decided(rng, n, np.arange(n) % 3 == 0), "empty keys")
    assert got[0] == (n, n - n // 3, 0) and not got[2].any()
    batch = varlen_batch(rng, 2500, long_at=(1022, 1023, 1024, 1025))
    keep = np.ones(2500, bool)
    keep[[1023, 1024]] = False
    got = compare(torch_cuda, seb, batch, decided(rng, 2500, keep), "two long keys across a tile boundary")
    assert got[0][1:] == (2, 600) and got[3].tolist() == [1023, 1024]


def test_another_plans_workspace_writes_nothing(seb, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(4)
    n = 3000
    for make in (lambda k: fixed_batch(rng, k, 16), lambda k: varlen_batch(rng, k, 60)):
        a, b = make(n), make(n)
        mem_a, mem_b = decided(rng, n, rng.random(n) < 0.5), decided(rng, n, rng.random(n) < 0.2)
        ra = device_compact(torch, seb, a, mem_a)
        rb = device_compact(torch, seb, b, mem_b)
        assert ra[0] != rb[0]
        # batch B's keys, statuses and sizes with the workspace that holds batch A's plan
        got = device_compact(torch, seb, b, mem_b, ws=ra[7])
        for buf in got[4:7]:
            assert (buf.cpu().numpy() == 0xA5).all(), "an emit with another plan's workspace wrote"
        # batch A's own sizes on a workspace that holds no plan at all
        blank = torch.zeros_like(ra[7])
        got = device_compact(torch, seb, a, mem_a, ws=blank)
        for buf in got[4:7]:
            assert (buf.cpu().numpy() == 0xA5).all(), "an emit with a blank workspace wrote"
        # sizes of another n are refused on the host
        c = make(n + 1)
        sz_c = device_compact(torch, seb, c, decided(rng, n + 1, rng.random(n + 1) < 0.5))[8]
        with pytest.raises(seb.SebError):
            device_compact(torch, seb, a, mem_a, sizes=sz_c)


@pytest.mark.parametrize("layout", ["fixed16", "fixed16_odd_src", "stride5", "offsets"])
def test_stale_statuses_stay_inside_the_outputs(seb, torch_cuda, layout):
    """mem_status rewritten to all-undecided between plan and emit: the outputs may be wrong, but every store is
    clamped to the plan's sizes.  device_compact checks the guards on both sides of each output and behind the
    workspace; the content is not looked at.  All memory involved is valid."""
    rng = np.random.default_rng(5)
    for n in (1000, 2 * TILE + 77, 5000):
        batch = varlen_batch(rng, n, 60) if layout == "offsets" else fixed_batch(
            rng, n, 5 if layout == "stride5" else 16, odd=layout == "fixed16_odd_src")
        for f in (0.5, 0.95, 1.0):
            mem = decided(rng, n, rng.random(n) < f)
            got = device_compact(torch_cuda, seb, batch, mem, emit_mem=np.zeros(n, np.uint8))
            assert got[0][1] == int(np.count_nonzero((mem != 1) & (mem != 2)))
        # and the other way round: fewer undecided keys at the emit than at the plan
        device_compact(torch_cuda, seb, batch, np.zeros(n, np.uint8), emit_mem=decided(rng, n, rng.random(n) < 0.5))


def test_refusals(seb, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(6)
    batch = fixed_batch(rng, 100, 16)
    dk = batch.dev(torch, seb)
    mem = torch.zeros(100, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(seb.dev_get_compact_workspace_size(100), dtype=torch.uint8, device="cuda")
    sz = seb.dev_get_compact_plan(dk, mem, ws)
    assert sz.as_tuple() == (100, 100, 1600)
    out, row = torch.zeros(1600, dtype=torch.uint8, device="cuda"), torch.zeros(100, dtype=torch.int32, device="cuda")
    with pytest.raises(seb.SebError):
        seb.dev_get_compact_plan(dk, mem, ws, ws_bytes=ws.numel() - 1)      # a workspace that is too small
    with pytest.raises(seb.SebError):
        seb.dev_get_compact_plan(dk, None, ws)                              # null mem_status
    with pytest.raises(seb.SebError):
        seb.dev_get_compact_plan(dk, mem, None, ws_bytes=1 << 20)           # null workspace
    with pytest.raises(seb.SebError):
        seb.dev_get_compact_plan(dk, mem, ws[1:], ws_bytes=ws.numel())      # a misaligned workspace
    big = seb.seb_keys(dk.data, None, 2**32, 16, 0)
    L, raw = seb.lib(), seb.seb_compact_sizes()
    assert L.seb_dev_get_compact_plan(C.byref(big), mem.data_ptr(), ws.data_ptr(), 1 << 40, C.byref(raw), None) == -1  # n >= 2^32
    assert L.seb_dev_get_compact_emit(C.byref(big), mem.data_ptr(), C.byref(raw), ws.data_ptr(), out.data_ptr(), None,
                                      row.data_ptr(), None) == -1
    assert L.seb_dev_get_compact_plan(C.byref(dk), mem.data_ptr(), ws.data_ptr(), ws.numel(), None, None) == -1  # null sizes
    assert L.seb_dev_get_compact_plan(None, mem.data_ptr(), ws.data_ptr(), ws.numel(), C.byref(raw), None) == -1  # null keys
    assert seb.dev_get_compact_workspace_size(2**32) == 0
    with pytest.raises(seb.SebError):
        seb.dev_get_compact_emit(dk, mem, sz, ws, out, None, None)          # null row
    with pytest.raises(seb.SebError):
        seb.dev_get_compact_emit(dk, mem, sz, ws, None, None, row)          # null out_keys
    with pytest.raises(seb.SebError):
        seb.dev_get_compact_emit(dk, None, sz, ws, out, None, row)          # null mem_status
    vb = varlen_batch(rng, 50, 20)
    vk = vb.dev(torch, seb)
    vws = torch.zeros(seb.dev_get_compact_workspace_size(50), dtype=torch.uint8, device="cuda")
    vsz = seb.dev_get_compact_plan(vk, mem, vws)
    with pytest.raises(seb.SebError):
        seb.dev_get_compact_emit(vk, mem, vsz, vws, torch.zeros(max(vsz.key_bytes, 1), dtype=torch.uint8, device="cuda"),
                                 None, row)                                  # offsets without out_off
    bad = seb.seb_compact_sizes(100, 100, 1599, 0)
    with pytest.raises(seb.SebError):
        seb.dev_get_compact_emit(dk, mem, bad, ws, out, None, row)          # key_bytes is not undecided * stride
    # n == 0 and undecided == 0 launch nothing and need no buffers
    zero = seb.dev_keys(out, n=0, stride=16)
    assert seb.dev_get_compact_plan(zero, None, None, ws_bytes=0).as_tuple() == (0, 0, 0)
    seb.dev_get_compact_emit(zero, None, seb.seb_compact_sizes(0, 0, 0, 0), None, None, None, None)
    allm = torch.ones(100, dtype=torch.uint8, device="cuda")
    sz0 = seb.dev_get_compact_plan(dk, allm, ws)
    assert sz0.as_tuple() == (100, 0, 0)
    seb.dev_get_compact_emit(dk, allm, sz0, ws, None, None, None)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the row-mapped join

J_ELEM = (1, 1, 2, 8, 4)  # status, source, col, vloc, vlen
J_DTYPE = (np.uint8, np.uint8, np.uint16, np.uint64, np.uint32)
J_IN = ("mem_vloc", "mem_vlen", "sst_col", "sst_vloc", "sst_vlen")


def device_join(torch, seb, mem, row, sst, omit_out=(), **inputs):
    """seb_dev_get_join_rows into 0xA5 buffers between guards: five numpy arrays (None for an output left out)."""
    n, m = len(mem), len(row)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(  # noqa: E731
        {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[np.asarray(a).dtype.itemsize]).copy()).cuda() if len(a) else \
        torch.zeros(1, dtype=torch.uint8, device="cuda")
    bufs = [torch.full((GUARD + e * n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for e in J_ELEM]
    views = [None if j in omit_out else b[GUARD: GUARD + e * n] for j, (b, e) in enumerate(zip(bufs, J_ELEM))]
    dev_in = {k: up(inputs.get(k)) for k in J_IN}
    seb.dev_get_join_rows(up(np.asarray(mem, np.uint8)), n, up(np.asarray(row, np.uint32)), m, up(np.asarray(sst, np.uint8)),
                          views[0], views[1], views[2], views[3], views[4], **dev_in)
    torch.cuda.synchronize()
    out = []
    for j, (b, e) in enumerate(zip(bufs, J_ELEM)):
        h = b.cpu().numpy()
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + e * n:] == 0xA5).all(), "bytes outside an output were written"
        if j in omit_out:
            assert (h == 0xA5).all(), "an output that was left out was written"
            out.append(None)
        else:
            out.append(np.frombuffer(h[GUARD: GUARD + e * n].tobytes(), J_DTYPE[j]))
    return out


def check_join(torch, seb, mem, row, sst, name, omit_out=(), **inputs):
    got = device_join(torch, seb, mem, row, sst, omit_out, **inputs)
    want = seb.get_join_rows(mem, row, sst, **inputs)
    ref = pref.join_rows(mem, row, sst, **inputs)
    pref.assert_same(want, ref, name + " (host half against the restatement)")
    keep = [j for j in range(5) if j not in omit_out]
    pref.assert_same([got[j] for j in keep], [want[j] for j in keep], name, [pref.NAMES[j] for j in keep])
    return got


def join_inputs(rng, n, m):
    return dict(mem_vloc=rng.integers(0, 1 << 40, n).astype(np.uint64), mem_vlen=rng.integers(0, 1 << 20, n).astype(np.uint32),
                sst_col=rng.integers(0, 7, m).astype(np.uint16), sst_vloc=rng.integers(0, 1 << 40, m).astype(np.uint64),
                sst_vlen=rng.integers(0, 4096, m).astype(np.uint32))


def test_join_truth_table_and_nullable_arguments(seb, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(8)
    mem, sst = (x.reshape(-1).astype(np.uint8) for x in np.meshgrid(np.arange(3), np.arange(3), indexing="ij"))
    _, row = pref.compact([b""] * 9, mem)
    full = join_inputs(rng, 9, 3)
    got = check_join(torch, seb, mem, row, sst[row], "truth table", **full)
    for i in range(9):
        ms, ss = int(mem[i]), int(sst[i])
        assert (got[0][i], got[1][i]) == ((1, 0) if ms == 1 else (0, 0) if ms == 2 else (ss, 1)), (ms, ss)
    # status and source are seb_dev_get_join's over the whole batch's sst_status
    st, src = seb.get_join(mem, sst)
    assert np.array_equal(got[0], st) and np.array_equal(got[1], src)
    for drop in J_IN:
        check_join(torch, seb, mem, row, sst[row], f"without {drop}", **{k: v for k, v in full.items() if k != drop})
    for j in range(1, 5):
        check_join(torch, seb, mem, row, sst[row], f"without output {pref.NAMES[j]}", omit_out=(j,), **full)
    check_join(torch, seb, mem, row, sst[row], "status alone", omit_out=(1, 2, 3, 4))


@pytest.mark.parametrize("n", [1, 255, 257, 5000])
def test_join_sizes(seb, torch_cuda, n):
    rng = np.random.default_rng(n)
    mem = decided(rng, n, rng.random(n) < 0.5)
    _, row = pref.compact([b""] * n, mem)
    sst = rng.integers(0, 3, row.size).astype(np.uint8)
    check_join(torch_cuda, seb, mem, row, sst, f"n={n}", **join_inputs(rng, n, row.size))


def test_join_bad_rows_and_empty_batches(seb, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(9)
    n = 700
    mem = decided(rng, n, rng.random(n) < 0.5)
    _, row = pref.compact([b""] * n, mem)
    # every third undecided key is named by no row
    part = np.delete(row, np.arange(0, row.size, 3))
    sst = rng.integers(1, 3, part.size).astype(np.uint8)
    got = check_join(torch, seb, mem, part, sst, "unnamed keys", **join_inputs(rng, n, part.size))
    for i in row[::3]:
        assert [int(g[i]) for g in got] == [0, 1, 0xFFFF, 0, 0]
    # rows outside the batch and rows naming decided keys are ignored; the guards show nothing else was written
    dec = np.nonzero((mem == 1) | (mem == 2))[0].astype(np.uint32)
    rows = np.concatenate([part, dec[:50], np.array([n, n + 1, 2**31, 2**32 - 1], np.uint32)])
    rows = rows[rng.permutation(rows.size)]
    sst = rng.integers(0, 3, rows.size).astype(np.uint8)
    check_join(torch, seb, mem, rows, sst, "ignored rows", **join_inputs(rng, n, rows.size))
    # m == 0: the memtables' answers and the "no row" default; n == 0: nothing at all
    e8, e32 = np.zeros(0, np.uint8), np.zeros(0, np.uint32)
    check_join(torch, seb, mem, e32, e8, "m == 0", **join_inputs(rng, n, 0))
    check_join(torch, seb, e8, e32, e8, "n == 0 and m == 0")
    L = seb.lib()
    assert L.seb_dev_get_join_rows(None, None, None, 0, None, 0, None, None, None, None, None, None, None, None, None, None) == 0
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    assert L.seb_dev_get_join_rows(None, None, None, 4, p, 2, p, None, None, None, p, None, None, None, None, None) == -1
    assert L.seb_dev_get_join_rows(p, None, None, 4, p, 2, p, None, None, None, None, None, None, None, None, None) == -1
    assert L.seb_dev_get_join_rows(p, None, None, 4, None, 2, p, None, None, None, p, None, None, None, None, None) == -1
    assert L.seb_dev_get_join_rows(p, None, None, 4, p, 2, None, None, None, None, p, None, None, None, None, None) == -1
    assert L.seb_dev_get_join_rows(p, None, None, 2**32, p, 2, p, None, None, None, p, None, None, None, None, None) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------ end to end

def sst_steps(torch, seb, reg, dk, cap, first_block, dpool, dblen):
    """MultiGet list -> locate -> block ids in the pool of data sections -> block search -> resolve, on dk's keys."""
    n = dk.n
    cand = torch.zeros(max(n * cap, 1), dtype=torch.int16, device="cuda")
    blocks = torch.zeros(max(n * cap, 1), dtype=torch.int64, device="cuda")
    reg.multiget_list_dev(dk, cand, cap)
    reg.locate_dev(dk, cand, blocks, cap)
    first = first_block[cand.to(torch.int64) & 0xFFFF]
    bid = torch.where((blocks == -1) | (first < 0), torch.full_like(blocks, -1), first + blocks // 4096).to(torch.int32)
    cells = torch.zeros(max(n * cap, 1), dtype=torch.int32, device="cuda")
    seb.dev_search_blocks(dk, bid, cap, dpool, dblen, cells)
    status = torch.full((max(n, 1),), 0x7E, dtype=torch.uint8, device="cuda")
    col = torch.zeros(max(n, 1), dtype=torch.int16, device="cuda")
    vloc = torch.zeros(max(n, 1), dtype=torch.int64, device="cuda")
    vlen = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
    seb.dev_resolve_rows(cells, bid, n, cap, status, col, vloc, vlen)
    return dict(cand=cand, blocks=blocks, bid=bid, cells=cells, status=status, col=col, vloc=vloc, vlen=vlen)


def test_end_to_end(seb, torch_cuda):
    """LSM.Get over two memtable runs and four SSTables (two overlapping L0 files, two disjoint L1 files) built by
    the library's device builder, their data sections as the block pool.  Pipeline A: the whole batch through
    list, locate, search, resolve and seb_dev_get_join.  Pipeline B: compact, the same steps on the m undecided
    keys, seb_dev_get_join_rows.  A, B and getpath_ref's LSM.Get agree."""
    torch = torch_cuda
    rng = np.random.default_rng(31)
    key = kg.key16_bytes
    val = lambda tag, i: tag + b"%d" % i + bytes(rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8))  # noqa: E731
    # key index ranges: [0, 4000) in L1 (two files), some of them again in L0; memtables above and across
    l1 = [[(key(i), val(b"l1-", i), 0) for i in range(0, 2000, 2)], [(key(i), val(b"l1-", i), 0) for i in range(2000, 4000, 2)]]
    l0a = [(key(i), val(b"l0a-", i), 1 if i % 12 == 0 else 0) for i in range(0, 4000, 6)]     # tombstones over L1 values
    l0b = [(key(i), val(b"l0b-", i), 0) for i in range(1, 4200, 14)]                           # odd keys: only here
    file_items = [(100, 0, l0a), (101, 0, l0b), (200, 1, l1[0]), (201, 1, l1[1])]
    active = gref.table_from_ops(
        [(key(i), val(b"act-", i), 5000 + i, 0) for i in range(4, 4000, 40)] +          # values over SSTable keys
        [(key(i), b"", 6000 + i, 1) for i in range(8, 4000, 40)] +                       # tombstones over SSTable values
        [(key(i), val(b"act-", i), 7000 + i, 0) for i in range(5001, 5200, 2)])          # only in the active run
    frozen = gref.table_from_ops(
        [(key(i), val(b"imm-", i), 100 + i, 0) for i in range(4, 4000, 80)] +            # hidden by the active run
        [(key(i), val(b"imm-", i), 200 + i, 0) for i in range(16, 4000, 40)] +           # only in the immutable run
        [(key(i), b"", 300 + i, 1) for i in range(24, 4000, 40)] +
        [(key(i), val(b"imm-", i), 400 + i, 0) for i in range(6001, 6100, 2)])
    tables = [active, frozen]
    files = [pref.File(num, level, items) for num, level, items in file_items]

    # the SSTables: one call of the device builder, data sections back to back = the block pool
    items = [it for _, _, its in file_items for it in its]
    file_begin = np.concatenate([[0], np.cumsum([len(its) for _, _, its in file_items])]).tolist()
    kd = torch.from_numpy(np.frombuffer(b"".join(k for k, _, _ in items), np.uint8).copy()).cuda()
    bk = seb.dev_keys(kd, n=len(items), stride=16)
    voff = np.concatenate([[0], np.cumsum([len(v) for _, v, _ in items])]).astype(np.uint64)
    dvals = torch.from_numpy(np.frombuffer(b"".join(v for _, v, _ in items), np.uint8).copy()).cuda()
    dvoff = u64_dev(torch, voff)
    ddel = torch.from_numpy(np.array([d for _, _, d in items], np.uint8)).cuda()
    bws = torch.zeros(seb.dev_sst_workspace_size(len(items), 4), dtype=torch.uint8, device="cuda")
    sizes = seb.dev_sst_plan(bk, dvoff, file_begin, bws)
    assert all(s[4] == 0 for s in sizes)
    nblocks = sum(s[0] for s in sizes)
    dpool = torch.zeros(sum(s[1] for s in sizes), dtype=torch.uint8, device="cuda")
    dindex = torch.zeros(sum(s[2] for s in sizes), dtype=torch.uint8, device="cuda")
    dmeta = torch.zeros(sum(s[3] for s in sizes), dtype=torch.uint8, device="cuda")
    dblen = torch.zeros(nblocks, dtype=torch.int16, device="cuda")
    seb.dev_sst_encode(bk, dvals, dvoff, ddel, file_begin, sizes, bws, dpool, dindex, dmeta, dblen)
    torch.cuda.synchronize()
    pool, index = dpool.cpu().numpy(), dindex.cpu().numpy().tobytes()
    assert pool.tobytes() == b"".join(f.data for f in files) and nblocks >= 40
    reg = seb.Registry(0)
    first_block = torch.full((65536,), -1, dtype=torch.int64, device="cuda")
    at_index = at_block = 0
    for (num, level, its), s in zip(file_items, sizes):
        keys = [k for k, _, _ in its]
        m_bits, k_hash = oc.params(len(keys), 0.01)
        bits = oc.build(m_bits, k_hash, np.frombuffer(b"".join(keys), np.uint8), len(keys), stride=16)
        slot = reg.put(num, level, bn.encode(bits, m_bits, k_hash), keys[0], keys[-1])
        reg.put_index(num, index[at_index: at_index + s[2]])
        first_block[slot] = at_block
        at_index += s[2]
        at_block += s[0]
    cap = reg.max_candidates()
    assert cap == 3  # two L0 files and one L1 file

    # the batch: every kind of key, in random order
    ids = np.concatenate([np.arange(0, 4300), np.arange(5000, 5200), np.arange(6000, 6100), np.arange(9000, 9050)])
    ids = ids[rng.permutation(ids.size)]
    probes = [key(int(i)) for i in ids]
    n = len(probes)
    want = [pref.lsm_get(tables, files, p) for p in probes]
    kinds = dict(active=0, frozen=0, mem_tomb_over_sst=0, sst_only=0, sst_tomb_over_older=0, nowhere=0)
    in_sst = {}  # key -> the deleted flags of its entries, over all files
    for f in files:
        for k, _, d in f.items:
            in_sst.setdefault(k, []).append(d)
    l0a_tombs = {k for k, _, d in l0a if d}
    for p, (st, source, value) in zip(probes, want):
        ms, r = gref.lsm_get_memtables(tables, p)[:2]
        flags = in_sst.get(p, [])
        kinds["active"] += ms == gref.FOUND and r == 0 and not flags
        kinds["frozen"] += ms == gref.FOUND and r == 1 and not flags
        kinds["mem_tomb_over_sst"] += ms == gref.TOMBSTONE and any(not d for d in flags)
        kinds["sst_only"] += ms == gref.NONE and st == pref.GET_FOUND
        kinds["sst_tomb_over_older"] += ms == gref.NONE and st == pref.GET_FOUND and value.startswith(b"l1-") and p in l0a_tombs
        kinds["nowhere"] += ms == gref.NONE and not flags
    assert all(v >= 10 for v in kinds.values()), kinds

    dk = seb.dev_keys(torch.from_numpy(np.frombuffer(b"".join(probes), np.uint8).copy()).cuda(), n=n, stride=16)
    arrays = [gref.run_arrays(t) for t in tables]
    runs, indexes = [], []
    for a in arrays:
        run = seb.dev_run(torch.from_numpy(a[0].copy()).cuda(), u64_dev(torch, a[1]), u64_dev(torch, a[3]),
                          torch.from_numpy(a[4]).cuda(), u64_dev(torch, a[5]))
        ix = torch.zeros(seb.dev_run_index_size(run.n), dtype=torch.uint8, device="cuda")
        seb.dev_run_index(run, ix)
        runs.append(run), indexes.append(ix)
    mem_status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    mem_run = torch.zeros(n, dtype=torch.uint8, device="cuda")
    mem_vloc = torch.zeros(n, dtype=torch.int64, device="cuda")
    mem_vlen = torch.zeros(n, dtype=torch.int32, device="cuda")
    seb.dev_runs_search(dk, runs, indexes, mem_status, run=mem_run, vloc=mem_vloc, vlen=mem_vlen)

    # pipeline A: the whole batch through the SSTable steps, then seb_dev_get_join
    A = sst_steps(torch, seb, reg, dk, cap, first_block, dpool, dblen)
    a_status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    a_source = torch.zeros(n, dtype=torch.uint8, device="cuda")
    seb.dev_get_join(mem_status, A["status"], n, a_status, a_source)

    # pipeline B: only the undecided keys go on
    ws = torch.zeros(seb.dev_get_compact_workspace_size(n), dtype=torch.uint8, device="cuda")
    plan = seb.dev_get_compact_plan(dk, mem_status, ws)
    m = plan.undecided
    assert 0 < m < n and plan.key_bytes == 16 * m
    ck, row = seb.dev_get_compact_emit(dk, mem_status, plan, ws, torch.zeros(16 * m, dtype=torch.uint8, device="cuda"), None,
                                       torch.zeros(m, dtype=torch.int32, device="cuda"))
    B = sst_steps(torch, seb, reg, ck, cap, first_block, dpool, dblen)
    b_out = [torch.full((n,), 0x7E, dtype=d, device="cuda") for d in (torch.uint8, torch.uint8, torch.int16, torch.int64, torch.int32)]
    seb.dev_get_join_rows(mem_status, n, row, m, B["status"], *b_out, mem_vloc=mem_vloc, mem_vlen=mem_vlen, sst_col=B["col"],
                          sst_vloc=B["vloc"], sst_vlen=B["vlen"])
    torch.cuda.synchronize()

    host = lambda t, v: np.frombuffer(t.cpu().numpy().tobytes(), v)  # noqa: E731
    ms = host(mem_status, np.uint8)
    und = (ms != 1) & (ms != 2)
    hrow = host(row, np.uint32)
    assert np.array_equal(hrow, np.nonzero(und)[0])
    b_status, b_source, b_col, b_vloc, b_vlen = (host(t, v) for t, v in zip(b_out, (np.uint8, np.uint8, np.uint16, np.uint64, np.uint32)))
    # A and B agree: status and source everywhere; col, vloc and vlen on the undecided keys
    assert np.array_equal(b_status, host(a_status, np.uint8)) and np.array_equal(b_source, host(a_source, np.uint8))
    assert np.array_equal(b_col[und], host(A["col"], np.uint16)[:n][und])
    assert np.array_equal(b_vloc[und], host(A["vloc"], np.uint64)[:n][und])
    assert np.array_equal(b_vlen[und], host(A["vlen"], np.uint32)[:n][und])
    # B's m-key arrays are A's rows gathered by row
    for name, v, per in (("cand", np.uint16, cap), ("blocks", np.uint64, cap), ("bid", np.uint32, cap), ("cells", np.uint32, cap),
                         ("status", np.uint8, 1), ("col", np.uint16, 1), ("vloc", np.uint64, 1), ("vlen", np.uint32, 1)):
        a, b = host(A[name], v)[: n * per].reshape(n, per), host(B[name], v)[: m * per].reshape(m, per)
        assert np.array_equal(b, a[hrow]), name
    # both agree with LSM.Get, value bytes included
    vals = [a[2] for a in arrays]
    hrun = host(mem_run, np.uint8)
    for i, (st, source, value) in enumerate(want):
        assert (int(b_status[i]), int(b_source[i])) == (st, source), (i, probes[i])
        if st == pref.GET_FOUND:
            src_bytes = pool if source == 1 else vals[hrun[i]]
            assert src_bytes[int(b_vloc[i]): int(b_vloc[i]) + int(b_vlen[i])].tobytes() == value, i
            assert (b_col[i] == 0xFFFF) == (source == 0)
        else:
            assert (int(b_col[i]), int(b_vloc[i]), int(b_vlen[i])) == (0xFFFF, 0, 0), i
    reg.close()
