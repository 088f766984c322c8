"""GPU: the block-id step's device forms (seb_dev_block_ids_resident, seb_dev_block_ids_plan / _emit, DESIGN.md
5.17) held to the host half seb_block_ids, which test_blockids.py holds to blockids_ref's restatement of the rules
(checked here again for the sizes Python walks quickly).  Every output lies between guard bytes.

Sizes: 0, 1, 63, 64, 65, 255, 257, 2049 (two tiles of 1024 and one cell) and 300,001 (several workgroups of the
grid-stride kernels, 293 tiles, a ragged last one).  Patterns: blockids_ref.PATTERNS.  max_uniq is the exact count of
distinct miss pairs, so the table runs at the fullest load it can have (for a power of two of pairs exactly one
half), and `cells`, which gives another table size and so other probe chains: no output may depend on either.
With the option grid_cap at 1 and 2, 1,300 cells take the loops of k_bid_resident, k_bid_insert and k_bid_emit through
three trips, the last one partial; the outputs equal the default grid's byte for byte.

The busy-stream case goes through tests/stream_late.py, the end-to-end case through the device builder and the
restated LSM.Get of getpath_ref."""
import ctypes as C

import numpy as np
import pytest

import blockids_ref as bref
import getpath_ref as pref
import keygen as kg
import stream_late as sl
from oracle import bloom_np as bn
from oracle import oracle_c as oc

pytestmark = pytest.mark.gpu

NO_BLOCK, NO_ID, PAD = bref.NO_BLOCK, bref.NO_ID, bref.PAD
SIZES = (0, 1, 63, 64, 65, 255, 257, 2049, 300_001)
FILL = sl.FILL


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


class Cells:
    """The cells and the residency table on the device, with the host half's answer."""

    def __init__(self, torch, seb, cand, blocks, first=None, count=None, id_base=0):
        self.cand, self.blocks, self.first, self.count, self.id_base = cand, blocks, first, count, id_base
        self.cells, self.slots = int(cand.size), 0 if first is None else int(first.size)
        self.dcand, self.dblocks = sl.to_dev(torch, cand), sl.to_dev(torch, blocks)
        self.dfirst = None if first is None else sl.to_dev(torch, first)
        self.dcount = None if count is None else sl.to_dev(torch, count)
        self.sizes, self.bid, self.us, self.ub = seb.block_ids(cand, blocks, first, count, id_base)
        if self.cells <= 2049:
            want = bref.block_ids(cand, blocks, first, count, id_base)
            assert want[0] == self.sizes
            bref.assert_same((self.bid, self.us, self.ub), want[1:], "host half")

    def args(self):
        return (self.dcand, self.dblocks, self.cells, self.dfirst, self.dcount, self.slots)


def workspace(torch, seb, cells, max_uniq):
    return torch.full((max(seb.dev_block_ids_workspace_size(cells, max_uniq), 16),), 0x5A, dtype=torch.uint8, device="cuda")


def plan_emit(torch, seb, d, max_uniq, what):
    """plan + emit between guards == the host half."""
    ws = workspace(torch, seb, d.cells, max_uniq)
    sz = seb.dev_block_ids_plan(*d.args(), max_uniq, ws)
    assert sz.as_tuple() == d.sizes and sz.reserved == 0, f"{what}: the plan's sizes"
    bid, us, ub = sl.Out(torch, d.cells, np.uint32), sl.Out(torch, sz.uniq, np.uint16), sl.Out(torch, sz.uniq, np.uint64)
    seb.dev_block_ids_emit(*d.args(), max_uniq, d.id_base, sz, ws, bid.t, us.t, ub.t)
    torch.cuda.synchronize()
    bref.assert_same((bid.get("bid"), us.get("uniq_slot"), ub.get("uniq_block")), (d.bid.reshape(-1), d.us, d.ub), what)
    return sz, ws


def resident_want(seb, d):
    """What the resident call writes, from the host half: the miss cells, told apart by an id_base no resident id
    comes near, lose their ids."""
    if d.cells <= 2049:
        want, cnt = bref.resident_only(d.cand, d.blocks, d.first, d.count)
        assert cnt == (d.sizes[1], d.sizes[2], d.sizes[4])
        return want
    far = seb.block_ids(d.cand, d.blocks, d.first, d.count, 2**31)[1].reshape(-1)
    return np.where((far >= 2**31) & (far < 2**31 + d.sizes[3]), NO_ID, far).astype(np.uint32)


def resident(torch, seb, d, what):
    """the resident call between guards == the rules with the miss cells left without an id; its counts == the sizes."""
    bid, counts = sl.Out(torch, d.cells, np.uint32), sl.Out(torch, 3, np.uint64)
    seb.dev_block_ids_resident(*d.args(), bid.t, counts.t)
    torch.cuda.synchronize()
    sl.same(bid.get("bid"), resident_want(seb, d), f"{what}: resident bid")
    if d.cells:
        assert tuple(int(x) for x in counts.get("counts")) == (d.sizes[1], d.sizes[2], d.sizes[4]), f"{what}: counts"
    else:
        assert (counts.get("counts").view(np.uint8) == FILL).all()  # nothing is launched, nothing written


@pytest.mark.parametrize("cells", SIZES)
def test_patterns_without_a_table(seb, torch_cuda, cells):
    torch = torch_cuda
    if cells == 0:
        d = Cells(torch, seb, np.zeros(0, np.uint16), np.zeros(0, np.uint64))
        plan_emit(torch, seb, d, 0, "empty")
        resident(torch, seb, d, "empty")
        return
    for name in bref.PATTERNS:
        if name == "mixed":
            continue
        cand, blocks = bref.pattern(name, cells)
        d = Cells(torch, seb, cand, blocks, id_base=7 if name == "7x3" else 0)
        uniq = d.sizes[3]
        if name == "distinct":
            assert uniq == cells
        if name == "one_pair":
            assert uniq == 1
        if name == "ends" and cells > 2:
            assert d.us[0] == 9 and (d.bid.reshape(-1) == d.bid.reshape(-1)[0]).sum() == 2
        plan_emit(torch, seb, d, uniq, f"{name} {cells} exact")
        if name in ("distinct", "7x3", "high_bits"):
            plan_emit(torch, seb, d, cells, f"{name} {cells} max_uniq=cells")
            plan_emit(torch, seb, d, 2**40, f"{name} {cells} max_uniq above cells")
    cand, blocks = bref.pattern("padding", cells)
    resident(torch, seb, Cells(torch, seb, cand, blocks), f"padding {cells}")


@pytest.mark.parametrize("cells", SIZES[1:])
def test_mixed_residency_table(seb, torch_cuda, cells):
    """res_slots below the largest slot, offsets past res_count, unaligned offsets, offsets >= 2^48, a res_first near
    2^32 whose sum overflows, padding of both kinds; the resident call's counts are the host's sizes."""
    torch = torch_cuda
    first, count = bref.table_mixed()
    cand, blocks = bref.pattern("mixed", cells)
    assert int(cand[cand != PAD].max(initial=0)) >= first.size or cells < 63
    for id_base, table in ((0, (first, count)), (5000, (first, count)), (3, (first[:1], count[:1])), (0, (None, None))):
        d = Cells(torch, seb, cand, blocks, *table, id_base=id_base)
        what = f"mixed {cells} slots {d.slots}"
        plan_emit(torch, seb, d, d.sizes[3], what)
        resident(torch, seb, d, what)
        if cells >= 255 and d.slots == first.size:
            assert all(s > 0 for s in d.sizes), d.sizes
    # bid alone, without counts
    d = Cells(torch, seb, cand, blocks, first, count)
    bid = sl.Out(torch, cells, np.uint32)
    seb.dev_block_ids_resident(*d.args(), bid.t, None)
    torch.cuda.synchronize()
    sl.same(bid.get("bid"), resident_want(seb, d), "bid without counts")


def capped_cells(torch, seb, name):
    """1,300 cells: at most 2 workgroups take them in three trips, the last one partial."""
    cand, blocks = bref.pattern(name, 1300)
    table = bref.table_mixed() if name == "mixed" else (None, None)
    d = Cells(torch, seb, cand, blocks, *table, id_base=11)
    assert 2 * 256 * 2 < d.cells < 2 * 256 * 3
    flat = d.bid.reshape(-1)
    assert (flat[1024:] != NO_ID).any() and (flat[:1024] != NO_ID).any()
    return d


@pytest.mark.parametrize("name", ["mixed"])
def test_resident_map_under_a_grid_cap(seb, torch_cuda, name):
    """seb_dev_block_ids_resident (k_bid_resident) at 1 and 2 workgroups: ids and counts equal the host half's and
    the default grid's."""
    torch = torch_cuda
    d = capped_cells(torch, seb, name)
    want = resident_want(seb, d)
    assert (want[1024:] != NO_ID).any()
    runs = []
    for cap in sl.CAPS:
        bid, counts = sl.Out(torch, d.cells, np.uint32), sl.Out(torch, 3, np.uint64)
        with sl.grid_cap(seb, cap):
            seb.dev_block_ids_resident(*d.args(), bid.t, counts.t)
            torch.cuda.synchronize()
        sl.same(bid.get("bid"), want, f"{name} cap {cap}: resident bid")
        assert tuple(int(x) for x in counts.get("counts")) == (d.sizes[1], d.sizes[2], d.sizes[4]), (name, cap)
        runs.append((bid.get().tobytes(), counts.get().tobytes()))
    assert runs[1] == runs[0] and runs[2] == runs[0]


@pytest.mark.parametrize("name", ["mixed", "distinct", "7x3"])
def test_plan_and_emit_under_a_grid_cap(seb, torch_cuda, name):
    """The insert (k_bid_insert, inside the plan) and the emit (k_bid_emit) at 1 and 2 workgroups; the plan's tile
    kernels keep their one workgroup per tile.  Sizes, ids and the unique blocks equal the host half's and the
    default grid's."""
    torch = torch_cuda
    d = capped_cells(torch, seb, name)
    uniq = d.sizes[3]
    assert uniq > (1024 if name == "distinct" else 2) and d.sizes[2] > 512
    runs = []
    for cap in sl.CAPS:
        ws = workspace(torch, seb, d.cells, uniq)
        bid, us, ub = sl.Out(torch, d.cells, np.uint32), sl.Out(torch, uniq, np.uint16), sl.Out(torch, uniq, np.uint64)
        with sl.grid_cap(seb, cap):
            sz = seb.dev_block_ids_plan(*d.args(), uniq, ws)
            assert sz.as_tuple() == d.sizes, (name, cap)
            seb.dev_block_ids_emit(*d.args(), uniq, d.id_base, sz, ws, bid.t, us.t, ub.t)
            torch.cuda.synchronize()
        got = (bid.get("bid"), us.get("uniq_slot"), ub.get("uniq_block"))
        bref.assert_same(got, (d.bid.reshape(-1), d.us, d.ub), f"{name} cap {cap}")
        runs.append([g.tobytes() for g in got])
    assert runs[1] == runs[0] and runs[2] == runs[0]


def test_range_and_the_retry(seb, torch_cuda):
    torch = torch_cuda
    first, count = bref.table_mixed()
    for cand, blocks, table, max_uniq in (
            (*bref.pattern("distinct", 2049), (None, None), None),           # max_uniq = uniq - 1
            (*bref.pattern("mixed", 2049), (first, count), None),
            (*bref.pattern("distinct", 1000), (None, None), 1),              # a table of 4 slots for 1000 pairs: it fills
            (*bref.pattern("distinct", 300_001), (None, None), 1),
            (*bref.pattern("distinct", 300_001), (None, None), 1000),        # a table of 2048 slots fills as well
            (*bref.pattern("7x3", 2049), (None, None), 0)):
        d = Cells(torch, seb, cand, blocks, *table)
        uniq = d.sizes[3]
        bound = uniq - 1 if max_uniq is None else max_uniq
        ws = workspace(torch, seb, d.cells, bound)
        with pytest.raises(seb.SebError) as e:
            seb.dev_block_ids_plan(*d.args(), bound, ws)
        sz = e.value.sizes
        assert e.value.code == -4
        assert (sz.cells, sz.resident, sz.misses, sz.bad) == (d.sizes[0], d.sizes[1], d.sizes[2], d.sizes[4]), "exact counts"
        assert bound < sz.uniq <= sz.misses
        # the emit refuses the failed plan's sizes, and a plan that failed leaves nothing an emit would accept
        bid, us, ub = sl.Out(torch, d.cells, np.uint32), sl.Out(torch, uniq, np.uint16), sl.Out(torch, uniq, np.uint64)
        with pytest.raises(seb.SebError):
            seb.dev_block_ids_emit(*d.args(), bound, 0, sz, ws, bid.t, us.t, ub.t)
        forged = seb.seb_blockids_sizes(sz.cells, sz.resident, sz.misses, min(bound, sz.misses), sz.bad, 0)
        seb.dev_block_ids_emit(*d.args(), bound, 0, forged, ws, bid.t, us.t, ub.t)
        torch.cuda.synchronize()
        for o in (bid, us, ub):
            assert (o.get().view(np.uint8) == FILL).all(), "an emit after a failed plan wrote"
        sz2, _ = plan_emit(torch, seb, d, sz.misses, "the retry with max_uniq = misses")
        assert sz2.uniq == uniq


def test_emit_with_other_sizes_or_another_workspace_writes_nothing(seb, torch_cuda):
    torch = torch_cuda
    first, count = bref.table_mixed()
    cand, blocks = bref.pattern("mixed", 2049)
    d = Cells(torch, seb, cand, blocks, first, count)
    uniq = d.sizes[3]
    sz, ws = plan_emit(torch, seb, d, uniq + 40, "the plan")
    outs = lambda: (sl.Out(torch, d.cells, np.uint32), sl.Out(torch, uniq, np.uint16), sl.Out(torch, uniq, np.uint64))  # noqa: E731

    def untouched(o):
        torch.cuda.synchronize()
        for x in o:
            assert (x.get().view(np.uint8) == FILL).all()

    for field, delta in (("resident", 1), ("resident", -1), ("misses", 1), ("bad", -1), ("uniq", -1)):
        other = seb.seb_blockids_sizes(*sz.as_tuple(), 0)
        setattr(other, field, getattr(other, field) + delta)
        o = outs()
        seb.dev_block_ids_emit(*d.args(), uniq + 40, 0, other, ws, *[x.t for x in o])
        untouched(o)
    # another max_uniq, another table size (the header in front of a larger workspace), a workspace no plan wrote
    big = 4 * (uniq + 40)
    grown = torch.cat([ws, workspace(torch, seb, d.cells, big)])
    for max_uniq, w in ((uniq + 41, ws), (big, grown), (uniq + 40, workspace(torch, seb, d.cells, uniq + 40))):
        o = outs()
        seb.dev_block_ids_emit(*d.args(), max_uniq, 0, sz, w, *[x.t for x in o])
        untouched(o)
    d2 = Cells(torch, seb, cand[:2048], blocks[:2048], first, count)
    sz2 = seb.dev_block_ids_plan(*d2.args(), uniq + 40, ws)
    o = outs()
    seb.dev_block_ids_emit(*d.args(), uniq + 40, 0, sz, ws, *[x.t for x in o])
    untouched(o)
    assert sz2.cells == 2048


def test_inputs_changed_since_the_plan_stay_inside_the_outputs(seb, torch_cuda):
    """The emit reads cells that are no longer the plan's: the outputs may be wrong, the guards may not."""
    torch = torch_cuda
    rng = np.random.default_rng(5)
    first, count = bref.table_mixed()
    cand, blocks = bref.pattern("mixed", 2049)
    d = Cells(torch, seb, cand, blocks, first, count)
    ws = workspace(torch, seb, d.cells, d.sizes[3])
    sz = seb.dev_block_ids_plan(*d.args(), d.sizes[3], ws)
    perm = rng.permutation(d.cells)
    for c2, b2 in ((cand[perm], blocks[perm]), (cand, (blocks + 4096).astype(np.uint64)), (cand[::-1].copy(), blocks)):
        e = Cells(torch, seb, c2, b2, first, count)
        bid, us, ub = sl.Out(torch, d.cells, np.uint32), sl.Out(torch, sz.uniq, np.uint16), sl.Out(torch, sz.uniq, np.uint64)
        seb.dev_block_ids_emit(*e.args(), d.sizes[3], 0, sz, ws, bid.t, us.t, ub.t)
        torch.cuda.synchronize()
        got = bid.get("bid"), us.get("uniq_slot"), ub.get("uniq_block")
        ok = got[0]
        assert ((ok == NO_ID) | (ok < sz.uniq) | ((ok >= 100) & (ok < 110)) | (ok >= NO_ID - 3)).all()


def test_refusals(seb, torch_cuda):
    torch = torch_cuda
    L = seb.lib()
    first, count = bref.table_mixed()
    cand, blocks = bref.pattern("mixed", 257)
    d = Cells(torch, seb, cand, blocks, first, count)
    uniq = d.sizes[3]
    ws = workspace(torch, seb, 257, uniq)
    need = seb.dev_block_ids_workspace_size(257, uniq)
    assert need % 16 == 0 and seb.dev_block_ids_workspace_size(2**32, 1) == 0
    assert seb.dev_block_ids_workspace_size(257, 2**50) == seb.dev_block_ids_workspace_size(257, 257)
    sz = seb.seb_blockids_sizes()
    bid, us, ub, counts = (sl.Out(torch, 257, np.uint32), sl.Out(torch, uniq, np.uint16), sl.Out(torch, uniq, np.uint64),
                           sl.Out(torch, 3, np.uint64))
    p = lambda t: t.data_ptr()  # noqa: E731
    base = dict(cand=p(d.dcand), blocks=p(d.dblocks), cells=257, first=p(d.dfirst), count=p(d.dcount), slots=6)

    def res(bid_=p(bid.t), counts_=p(counts.t), **kw):
        a = dict(base, **kw)
        return L.seb_dev_block_ids_resident(a["cand"], a["blocks"], a["cells"], a["first"], a["count"], a["slots"], bid_, counts_, None)

    def plan(ws_=p(ws), ws_bytes=need, sz_=C.byref(sz), max_uniq=uniq, **kw):
        a = dict(base, **kw)
        return L.seb_dev_block_ids_plan(a["cand"], a["blocks"], a["cells"], a["first"], a["count"], a["slots"], max_uniq, ws_,
                                        ws_bytes, sz_, None)

    def emit(sizes=None, ws_=p(ws), bid_=p(bid.t), us_=p(us.t), ub_=p(ub.t), max_uniq=uniq, id_base=0, **kw):
        a = dict(base, **kw)
        return L.seb_dev_block_ids_emit(a["cand"], a["blocks"], a["cells"], a["first"], a["count"], a["slots"], max_uniq, id_base,
                                        C.byref(sz) if sizes is None else sizes, ws_, bid_, us_, ub_, None)

    assert plan() == 0 and sz.as_tuple() == d.sizes
    common = [dict(cand=None), dict(blocks=None), dict(first=None), dict(count=None), dict(cells=2**32),
              dict(cand=base["cand"] + 1), dict(blocks=base["blocks"] + 4), dict(first=base["first"] + 2),
              dict(count=base["count"] + 1)]
    for kw in common:
        assert res(**kw) == -1 and plan(**kw) == -1 and emit(**kw) == -1, kw
    assert res(bid_=None) == -1 and res(bid_=p(bid.t) + 2) == -1 and res(counts_=p(counts.t) + 4) == -1
    assert plan(ws_=None) == -1 and plan(ws_=p(ws) + 8) == -1 and plan(sz_=None) == -1 and plan(ws_bytes=need - 1) == -1
    assert b"workspace" in L.seb_last_error()
    assert plan() == 0  # the refused plans above changed nothing the emit needs; sz was reset by them
    for kw in (dict(sizes=None, ws_=None), dict(ws_=p(ws) + 8), dict(bid_=None), dict(us_=None), dict(ub_=None),
               dict(bid_=p(bid.t) + 2), dict(us_=p(us.t) + 1), dict(ub_=p(ub.t) + 4), dict(id_base=NO_ID - uniq + 1)):
        assert emit(**kw) == -1, kw
    for field, value in (("cells", 256), ("uniq", uniq + 1), ("uniq", sz.misses + 1), ("resident", 258), ("bad", 2**63)):
        other = seb.seb_blockids_sizes(*sz.as_tuple(), 0)
        setattr(other, field, value)
        assert emit(sizes=C.byref(other)) == -1, field
    # cells == 0: nothing launched, nothing written, no pointer needed
    assert L.seb_dev_block_ids_resident(None, None, 0, None, None, 0, None, p(counts.t), None) == 0
    assert L.seb_dev_block_ids_plan(None, None, 0, None, None, 0, 5, None, 0, C.byref(sz), None) == 0
    assert sz.as_tuple() == (0, 0, 0, 0, 0)
    assert L.seb_dev_block_ids_emit(None, None, 0, None, None, 0, 5, 0, C.byref(sz), None, None, None, None, None) == 0
    torch.cuda.synchronize()
    for o in (bid, us, ub, counts):
        assert (o.get().view(np.uint8) == FILL).all(), "a refused call wrote"


@pytest.fixture(scope="module")
def rig(seb, torch_cuda):
    try:
        return sl.Rig(torch_cuda, seb)
    except AssertionError as e:
        pytest.fail(f"stream control: {e}")


def test_on_a_busy_side_stream_with_late_inputs(seb, torch_cuda, rig):
    """The cells arrive late on the side stream, a valid poison in their place until then: the plan (which blocks
    through the delay), the emit and the resident call are enqueued while the stream is busy and must read the good
    cells, which only stream order gives them."""
    torch = torch_cuda
    first, count = bref.table_mixed()
    cells = 2049
    cand, blocks = bref.pattern("mixed", cells, seed=1)
    cand_p, blocks_p = bref.pattern("mixed", cells, seed=2)
    good, poison = seb.block_ids(cand, blocks, first, count, 11), seb.block_ids(cand_p, blocks_p, first, count, 11)
    res_good, res_poison = bref.resident_only(cand, blocks, first, count), bref.resident_only(cand_p, blocks_p, first, count)
    sl.differ([good[1], res_good[0]], [poison[1], res_poison[0]], ["bid", "resident bid"])
    assert good[0] != poison[0]
    L = rig.session()
    dcand, dblocks = L.inp(cand, cand_p), L.inp(blocks, blocks_p)
    dfirst, dcount = sl.to_dev(torch, first), sl.to_dev(torch, count)
    max_uniq = max(good[0][3], poison[0][3]) + 3
    ws = workspace(torch, seb, cells, max_uniq)
    # warm: every kernel of the three calls has run once, on other data, before a delay is armed
    warm = Cells(torch, seb, cand_p[:300], blocks_p[:300], first, count)
    plan_emit(torch, seb, warm, 300, "warm")
    resident(torch, seb, warm, "warm")
    L.arm()
    sz = L.plan(seb.dev_block_ids_plan, dcand, dblocks, cells, dfirst, dcount, first.size, max_uniq, ws)
    assert sz.as_tuple() == good[0], "the plan's sizes"
    cand2, blocks2 = L.inp(cand, cand_p), L.inp(blocks, blocks_p)  # the resident call's own late cells
    bid, us, ub = L.out(cells, np.uint32), L.out(sz.uniq, np.uint16), L.out(sz.uniq, np.uint64)
    rbid, counts = L.out(cells, np.uint32), L.out(3, np.uint64)
    L.arm()
    L.call(seb.dev_block_ids_resident, cand2, blocks2, cells, dfirst, dcount, first.size, rbid.t, counts.t)
    L.call(seb.dev_block_ids_emit, dcand, dblocks, cells, dfirst, dcount, first.size, max_uniq, 11, sz, ws, bid.t, us.t, ub.t)
    L.finish()
    bref.assert_same((bid.get("bid"), us.get("uniq_slot"), ub.get("uniq_block")), good[1:], "late emit")
    sl.same(rbid.get("resident bid"), res_good[0], "late resident bid")
    assert tuple(int(x) for x in counts.get("counts")) == res_good[1]


def test_end_to_end(seb, torch_cuda):
    """Four SSTables on two levels from the device builder, two resident in the pool and two not: list -> locate ->
    plan / emit -> the read list's blocks copied from the files' images into the pool at id_base + r -> search ->
    resolve equals the restated LSM.Get for present, absent and shadowed keys."""
    torch = torch_cuda
    rng = np.random.default_rng(41)
    key = kg.key16_bytes
    val = lambda tag, i: tag + b"%d" % i + bytes(rng.integers(0, 256, int(rng.integers(0, 120)), dtype=np.uint8))  # noqa: E731
    l1 = [[(key(i), val(b"l1-", i), 0) for i in range(0, 1000, 2)], [(key(i), val(b"l1-", i), 0) for i in range(1000, 2000, 2)]]
    l0a = [(key(i), val(b"l0a-", i), 1 if i % 12 == 0 else 0) for i in range(0, 2000, 6)]   # shadows L1, tombstones too
    l0b = [(key(i), val(b"l0b-", i), 0) for i in range(1, 2100, 14)]
    file_items = [(100, 0, l0a), (101, 0, l0b), (200, 1, l1[0]), (201, 1, l1[1])]
    resident_files = {100, 201}
    files = [pref.File(num, level, items) for num, level, items in file_items]
    items = [it for _, _, its in file_items for it in its]
    file_begin = np.concatenate([[0], np.cumsum([len(its) for _, _, its in file_items])]).tolist()
    kd = torch.from_numpy(np.frombuffer(b"".join(k for k, _, _ in items), np.uint8).copy()).cuda()
    bk = seb.dev_keys(kd, n=len(items), stride=16)
    voff = np.concatenate([[0], np.cumsum([len(v) for _, v, _ in items])]).astype(np.uint64)
    dvals = torch.from_numpy(np.frombuffer(b"".join(v for _, v, _ in items), np.uint8).copy()).cuda()
    dvoff = sl.to_dev(torch, voff)
    ddel = torch.from_numpy(np.array([d for _, _, d in items], np.uint8)).cuda()
    bws = torch.zeros(seb.dev_sst_workspace_size(len(items), 4), dtype=torch.uint8, device="cuda")
    sizes = seb.dev_sst_plan(bk, dvoff, file_begin, bws)
    assert all(s[4] == 0 for s in sizes)
    nblocks = sum(s[0] for s in sizes)
    dimg = torch.zeros(sum(s[1] for s in sizes), dtype=torch.uint8, device="cuda")  # the four data sections, back to back
    dindex = torch.zeros(sum(s[2] for s in sizes), dtype=torch.uint8, device="cuda")
    dmeta = torch.zeros(sum(s[3] for s in sizes), dtype=torch.uint8, device="cuda")
    dlen = torch.zeros(nblocks, dtype=torch.int16, device="cuda")
    seb.dev_sst_encode(bk, dvals, dvoff, ddel, file_begin, sizes, bws, dimg, dindex, dmeta, dlen)
    torch.cuda.synchronize()
    index = dindex.cpu().numpy().tobytes()
    assert dimg.cpu().numpy().tobytes() == b"".join(f.data for f in files) and nblocks >= 16

    # the pool: the resident files' sections first, then room for the read list
    reg = seb.Registry(0)
    res_first = np.full(8, NO_ID, np.uint32)
    res_count = np.zeros(8, np.uint32)
    image_at = {}  # slot -> the file's first block in dimg
    pool_parts, blen_parts, id_base, at_index, at_block = [], [], 0, 0, 0
    for (num, level, its), s in zip(file_items, sizes):
        keys = [k for k, _, _ in its]
        m_bits, k_hash = oc.params(len(keys), 0.01)
        bits = oc.build(m_bits, k_hash, np.frombuffer(b"".join(keys), np.uint8), len(keys), stride=16)
        slot = reg.put(num, level, bn.encode(bits, m_bits, k_hash), keys[0], keys[-1])
        reg.put_index(num, index[at_index: at_index + s[2]])
        image_at[slot] = at_block
        if num in resident_files:
            res_first[slot], res_count[slot] = id_base, s[0]
            pool_parts.append(dimg[at_block * 4096: (at_block + s[0]) * 4096])
            blen_parts.append(dlen[at_block: at_block + s[0]])
            id_base += s[0]
        at_index += s[2]
        at_block += s[0]
    cap = reg.max_candidates()
    assert cap == 3

    ids = np.concatenate([np.arange(0, 2150), np.arange(9000, 9050)])
    ids = ids[rng.permutation(ids.size)]
    probes = [key(int(i)) for i in ids]
    n = len(probes)
    want = [pref.lsm_get([], files, p) for p in probes]
    dk = seb.dev_keys(torch.from_numpy(np.frombuffer(b"".join(probes), np.uint8).copy()).cuda(), n=n, stride=16)
    cells = n * cap
    cand = torch.zeros(cells, dtype=torch.int16, device="cuda")
    blocks = torch.zeros(cells, dtype=torch.int64, device="cuda")
    reg.multiget_list_dev(dk, cand, cap)
    reg.locate_dev(dk, cand, blocks, cap)
    dfirst, dcount = sl.to_dev(torch, res_first), sl.to_dev(torch, res_count)
    max_uniq = nblocks - id_base  # the blocks of the files that are not resident
    ws = workspace(torch, seb, cells, max_uniq)
    sz = seb.dev_block_ids_plan(cand, blocks, cells, dfirst, dcount, 8, max_uniq, ws)
    assert sz.resident > 0 and sz.misses > sz.uniq > 0 and sz.bad == 0
    bid = torch.zeros(cells, dtype=torch.int32, device="cuda")
    us = torch.zeros(sz.uniq, dtype=torch.int16, device="cuda")
    ub = torch.zeros(sz.uniq, dtype=torch.int64, device="cuda")
    seb.dev_block_ids_emit(cand, blocks, cells, dfirst, dcount, 8, max_uniq, id_base, sz, ws, bid, us, ub)
    torch.cuda.synchronize()
    host = lambda t, v: np.frombuffer(t.cpu().numpy().tobytes(), v)  # noqa: E731
    hs = seb.block_ids(host(cand, np.uint16), host(blocks, np.uint64), res_first, res_count, id_base)
    assert hs[0] == sz.as_tuple()
    bref.assert_same((host(bid, np.uint32), host(us, np.uint16), host(ub, np.uint64)), hs[1:], "end to end")
    # the caller's reads: block r of the list from its file's image into pool block id_base + r
    src = np.array([image_at[int(s)] for s in hs[2]], np.int64) + (hs[3] // 4096).astype(np.int64)
    assert (hs[3] % 4096 == 0).all() and len(set(src.tolist())) == sz.uniq
    dsrc = torch.from_numpy(src).cuda()
    pool = torch.cat(pool_parts + [dimg.view(-1, 4096)[dsrc].reshape(-1)])
    blen = torch.cat(blen_parts + [dlen[dsrc]])
    assert pool.numel() == (id_base + sz.uniq) * 4096 and sz.uniq <= max_uniq

    out_cells = torch.zeros(cells, dtype=torch.int32, device="cuda")
    seb.dev_search_blocks(dk, bid, cap, pool, blen, out_cells)
    status = torch.full((n,), 0x7E, dtype=torch.uint8, device="cuda")
    vloc = torch.zeros(n, dtype=torch.int64, device="cuda")
    vlen = torch.zeros(n, dtype=torch.int32, device="cuda")
    seb.dev_resolve_rows(out_cells, bid, n, cap, status, None, vloc, vlen)
    torch.cuda.synchronize()
    hpool, st, hvloc, hvlen = pool.cpu().numpy(), host(status, np.uint8), host(vloc, np.uint64), host(vlen, np.uint32)
    kinds = dict(found=0, absent=0, shadowed=0, tomb_over_older=0)
    l0a_keys = {k: d for k, _, d in l0a}
    for i, (s, _, value) in enumerate(want):
        assert int(st[i]) == s, (i, probes[i])
        if s == pref.GET_FOUND:
            assert hpool[int(hvloc[i]): int(hvloc[i]) + int(hvlen[i])].tobytes() == value, i
            kinds["found"] += 1
            kinds["shadowed"] += value.startswith(b"l0a-") and int(ids[i]) % 2 == 0     # an L1 value lies under it
            kinds["tomb_over_older"] += value.startswith(b"l1-") and l0a_keys.get(probes[i]) == 1
        else:
            kinds["absent"] += 1
    assert all(v >= 10 for v in kinds.values()), kinds
    reg.close()
