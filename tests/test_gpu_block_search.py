"""GPU: the batched data-block search (seb_dev_search_blocks / seb_dev_resolve_rows /
seb_search_blocks) against searchBlock (lsm/sstable.go:242-290) and LSM.Get's walk over a key's
SSTables (lsm/lsm.go:174-197).

The per-cell reference is the host walker seb_block_search, which test_block_search.py holds to the
Python restatement of the reference; the end-to-end test goes back to the restatement itself.
Pool slots are filled with 0xA5 past each block's length, so a read past `blen` changes an answer."""
import bisect
import ctypes as C
import itertools
import struct

import numpy as np
import pytest

import block_ref as br
import keygen as kg
from oracle import bloom_np as bn
from oracle import oracle_c as oc

pytestmark = pytest.mark.gpu

NO_BLOCK = 2**64 - 1
NO_ID = 2**32 - 1
PAD = 0xFFFF


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def pack(keys):
    off = np.zeros(len(keys) + 1, np.uint64)
    np.cumsum(np.array([len(k) for k in keys], np.uint64), out=off[1:])
    return np.frombuffer(b"".join(keys), np.uint8), off


def dev_varlen(torch, seb, keys, shift=3):
    """A device variable-length batch whose data pointer is odd and whose offsets[0] != 0."""
    data, off = pack(keys)
    buf = np.concatenate([np.full(1 + shift, 0xEE, np.uint8), data, np.full(4, 0xEE, np.uint8)])
    d = torch.from_numpy(buf).cuda()[1:]
    assert d.data_ptr() % 2 == 1
    o = torch.from_numpy((off + np.uint64(shift)).view(np.int64)).cuda()
    return seb.dev_keys(d, o)


def dev_fixed16(torch, seb, keys):
    d = torch.from_numpy(np.frombuffer(b"".join(keys), np.uint8).copy()).cuda()
    assert d.data_ptr() % 16 == 0 and all(len(k) == 16 for k in keys)
    return seb.dev_keys(d, n=len(keys), stride=16)


def make_pool(images):
    """(pool bytes in 4096-byte slots, u16 lengths): the slot past each image is 0xA5."""
    pool = np.full((max(len(images), 1), br.BLOCK), 0xA5, np.uint8)
    for b, img in enumerate(images):
        pool[b, :len(img)] = np.frombuffer(img, np.uint8)
    return pool, np.array([len(i) for i in images], np.uint16)


def dev_pool(torch, pool, blen):
    p = torch.from_numpy(pool.reshape(-1)).cuda()
    assert p.data_ptr() % 16 == 0
    return p, torch.from_numpy(blen.view(np.int16)).cuda()


def host_cells(seb, images, keys, bid):
    """seb_block_search per cell of bid (n, cap); ids that name no block give CELL_NONE."""
    memo = {}
    out = np.zeros(bid.shape, np.uint32)
    for i, key in enumerate(keys):
        for j, b in enumerate(bid[i].tolist()):
            if b < len(images):
                if (b, key) not in memo:
                    memo[(b, key)] = seb.block_search(images[b], key)
                out[i, j] = memo[(b, key)]
    return out


def run_search(torch, seb, dk, bid, dpool, dblen, guard=False):
    n, cap = bid.shape
    flat = np.append(bid.reshape(-1), np.uint32(0)) if guard else bid.reshape(-1)  # a live id past the end
    db = torch.from_numpy(flat.view(np.int32).copy()).cuda() if flat.size else torch.zeros(1, dtype=torch.int32, device="cuda")
    cells = torch.full((n * cap + 1,), 0x7E57, dtype=torch.int32, device="cuda")
    seb.dev_search_blocks(dk, db, cap, dpool, dblen, cells)
    torch.cuda.synchronize()
    got = cells.cpu().numpy().view(np.uint32)
    assert got[n * cap] == 0x7E57, "a cell past n * cap was written"
    return got[: n * cap].reshape(n, cap), db, cells


@pytest.fixture(scope="module")
def parity(seb):
    """The hand-built blocks plus random ones as one pool, every probe against every block: the
    host walker's cells, once, for a variable-length batch and for 16-byte keys."""
    rng = np.random.default_rng(11)
    hand = br.hand_blocks()
    images = [img for _, img, _ in hand]
    probes = sorted({k for _, _, keys in hand for k in keys})
    while len(images) < 60:
        img, keys = br.random_block(rng)
        images.append(img)
        probes = sorted(set(probes) | set(keys[:4]))
    lens = {len(i) for i in images}
    assert 0 in lens and 4096 in lens and len(probes) > 300
    fixed = sorted({(q + b"\x00" * 16)[:16] for q in probes[::2]} | {(q + b"\xff" * 16)[:16] for q in probes[1::4]})
    fixed += [b"key%03d" % i + b"\x00" * 10 for i in range(4)]
    # entries that are exactly 16 bytes long, so that aligned 16-byte keys are found too
    ents = sorted(set(fixed[::5]))
    images.append(br.encode_block([(k, b"val-" + k[:3], 1 if i % 5 == 2 else 0) for i, k in enumerate(ents)]))
    pool, blen = make_pool(images)
    bid_v = np.tile(np.arange(len(images), dtype=np.uint32), (len(probes), 1))
    bid_f = np.tile(np.arange(len(images), dtype=np.uint32), (len(fixed), 1))
    want_v, want_f = host_cells(seb, images, probes, bid_v), host_cells(seb, images, fixed, bid_f)
    for want in (want_v, want_f):
        assert set(np.unique(want >> 28).tolist()) == {br.MISS, br.FOUND, br.TOMBSTONE, br.TRUNC}
    return dict(images=images, pool=pool, blen=blen, probes=probes, fixed=fixed, bid_v=bid_v, bid_f=bid_f, want_v=want_v,
                want_f=want_f)


@pytest.mark.parametrize("grid_cap", [None, 2])
def test_cell_parity(seb, torch_cuda, parity, grid_cap):
    """Every probe against every block (cap = the number of blocks), cell for cell equal to the
    host walker; grid_cap 2 makes two workgroups take the tiles in turns.  (One kernel: the
    wave-cooperative form was measured slower and removed)"""
    torch = torch_cuda
    p = parity
    dpool, dblen = dev_pool(torch, p["pool"], p["blen"])
    with seb.option("grid_cap", grid_cap or seb.get_option("grid_cap")):
        got, _, _ = run_search(torch, seb, dev_varlen(torch, seb, p["probes"]), p["bid_v"], dpool, dblen)
        bad = np.argwhere(got != p["want_v"])
        assert bad.size == 0, [(p["probes"][i], j, hex(got[i, j]), hex(p["want_v"][i, j])) for i, j in bad[:5]]
        got, _, _ = run_search(torch, seb, dev_fixed16(torch, seb, p["fixed"]), p["bid_f"], dpool, dblen)
        bad = np.argwhere(got != p["want_f"])
        assert bad.size == 0, [(p["fixed"][i], j, hex(got[i, j]), hex(p["want_f"][i, j])) for i, j in bad[:5]]


@pytest.fixture(scope="module")
def table(seb):
    """A small SSTable image of 16-byte keys as the pool of the row tests."""
    rng = np.random.default_rng(5)
    items = [(kg.key16_bytes(int(i)), bytes(rng.integers(0, 256, int(rng.integers(0, 120)), dtype=np.uint8)), i % 9 == 4)
             for i in range(0, 900, 3)]
    image, index = br.build_sstable(items)
    images = [image[o:o + 4096] for _, o in index] + [image[:1000], b""]
    assert 6 <= len(images) <= 16
    return images


def test_row_shapes(seb, torch_cuda, table):
    """cap 1 / 3 / 16 / 17 and n around the 64-lane and 256-thread boundaries; rows mix live ids,
    SEB_NO_BLOCK_ID, ids >= num_blocks and many cells on one block; a wave with 64, 0 and 1 live
    lanes; the element past n * cap stays untouched."""
    torch = torch_cuda
    rng = np.random.default_rng(9)
    images = table
    nb = len(images)
    pool, blen = make_pool(images)
    dpool, dblen = dev_pool(torch, pool, blen)
    ids = np.array(list(range(nb)) + [2] * 8 + [NO_ID] * 10 + [nb, nb + 1, 2**31, NO_ID - 1], np.uint32)
    for cap in (1, 3, 16, 17):
        for n in (0, 1, 63, 64, 65, 257):
            probes = [kg.key16_bytes(int(i)) for i in rng.integers(0, 920, n)]
            bid = ids[rng.integers(0, len(ids), (n, cap))]
            flat = bid.reshape(-1)
            if flat.size >= 192:
                flat[0:64] = rng.integers(0, nb, 64)  # a wave with 64 live lanes,
                flat[64:192] = NO_ID                 # one with none,
                flat[150] = 1                        # one with a single live lane
            data = np.frombuffer(b"".join(probes), np.uint8).copy() if n else np.zeros(16, np.uint8)
            dk = seb.dev_keys(torch.from_numpy(data).cuda(), n=n, stride=16)
            got, db, cells = run_search(torch, seb, dk, bid, dpool, dblen, guard=True)
            want = host_cells(seb, images, probes, bid)
            assert np.array_equal(got, want), (cap, n)
            if n == 257:
                assert (want >> 28 == br.FOUND).any() and (want >> 28 == br.NONE).any(), (cap, n)
            if n and cap == 3:  # the host form on the same rows
                st, col, vloc, vlen, hc = seb.search_blocks(data.reshape(n, 16), bid, pool, blen, want_cells=True)
                assert np.array_equal(hc, want), (cap, n)
    # argument errors: nothing is launched
    lib = seb.lib()
    args = lambda **kw: [kw.get("keys", C.byref(dk)), kw.get("bid", db.data_ptr()), kw.get("cap", 17),  # noqa: E731
                         kw.get("pool", dpool.data_ptr()), kw.get("blen", dblen.data_ptr()), nb,
                         kw.get("cells", cells.data_ptr()), None]
    assert lib.seb_dev_search_blocks(*args(cap=0)) == -1 and "cap 0" in seb.last_error()
    for name in ("bid", "pool", "blen", "cells"):
        assert lib.seb_dev_search_blocks(*args(**{name: None})) == -1 and "null" in seb.last_error(), name
    assert lib.seb_dev_search_blocks(*args(keys=None)) == -1
    assert lib.seb_dev_search_blocks(*args(pool=dpool.data_ptr() + 8)) == -1 and "aligned" in seb.last_error()
    torch.cuda.synchronize()
    zero = seb.dev_keys(torch.zeros(16, dtype=torch.uint8, device="cuda"), n=0, stride=16)
    assert lib.seb_dev_search_blocks(C.byref(zero), db.data_ptr(), 3, dpool.data_ptr(), dblen.data_ptr(), nb,
                                     cells.data_ptr(), None) == 0


def test_host_form_chunked(seb, torch_cuda, table, monkeypatch):
    """seb_search_blocks past its first chunk of keys: with SEB_CHUNK_BYTES = 4096 a chunk is 256
    16-byte keys, so the batches are no chunk, one key, one full chunk, a one-key second chunk, and
    four chunks with a one-key tail.  Cells against search_block_ref, rows against lsm_get_ref."""
    monkeypatch.setenv("SEB_CHUNK_BYTES", "4096")
    ctx = seb.Ctx(0)
    rng = np.random.default_rng(17)
    images = table
    nb, cap, top = len(images), 3, 769
    pool, blen = make_pool(images)
    ids = np.array(list(range(nb)) * 3 + [NO_ID] * 4 + [nb, 2**31], np.uint32)
    probes = [kg.key16_bytes(int(i)) for i in rng.integers(0, 920, top)]
    bid = ids[rng.integers(0, len(ids), (top, cap))]
    memo = {}
    want = np.zeros((top, cap), np.uint32)
    rows = []
    for i, key in enumerate(probes):
        for j, b in enumerate(bid[i].tolist()):
            if b < nb:
                if (b, key) not in memo:
                    memo[(b, key)] = br.search_block_ref(images[b], key)
                want[i, j] = memo[(b, key)]
        st, wc, c = br.lsm_get_ref(want[i].tolist())
        found = st == br.GET_FOUND
        rows.append((st, wc, int(bid[i, wc]) * 4096 + ((c >> 13) & 0x1FFF) if found else 0, c & 0x1FFF if found else 0))
    rows = np.array(rows, np.uint64)
    assert {br.GET_MISS, br.GET_FOUND} <= set(rows[:, 0].tolist()) and (want >> 28 == br.NONE).any()
    data = np.frombuffer(b"".join(probes), np.uint8).reshape(top, 16)
    for n in (0, 1, 256, 257, top):
        st, col, vloc, vlen, cells = ctx.search_blocks(data[:n], bid[:n], pool, blen, want_cells=True)
        assert np.array_equal(cells, want[:n]), n
        for got, ref in zip((st, col, vloc, vlen), rows[:n].T.reshape(4, n)):
            assert np.array_equal(got.astype(np.uint64), ref), n
    ctx.close()


def test_resolve(seb, torch_cuda):
    """Rows of every ordering of MISS / TOMBSTONE / FOUND / TRUNC / NONE over cap 1..5 against
    lsm_get_ref; null optional outputs; the orderings the issue names."""
    torch = torch_cuda
    rng = np.random.default_rng(13)
    kinds = (br.MISS, br.TOMBSTONE, br.FOUND, br.TRUNC, br.NONE)
    for cap in range(1, 6):
        rows = list(itertools.product(kinds, repeat=cap))
        n = len(rows)
        cells = np.zeros((n, cap), np.uint32)
        bid = rng.integers(0, 2**32 - 2, (n, cap)).astype(np.uint32)
        for i, row in enumerate(rows):
            for j, st in enumerate(row):
                if st == br.FOUND:
                    cells[i, j] = br.cell(st, int(rng.integers(13, 4097)), int(rng.integers(0, 4084)))
                else:
                    cells[i, j] = br.cell(st)
                    if st == br.NONE:
                        bid[i, j] = NO_ID
        want = [br.lsm_get_ref(cells[i].tolist()) for i in range(n)]
        dc = torch.from_numpy(np.append(cells.reshape(-1), np.uint32(br.cell(br.FOUND, 1, 1))).view(np.int32)).cuda()
        db = torch.from_numpy(np.append(bid.reshape(-1), np.uint32(0)).view(np.int32)).cuda()
        status = torch.full((n + 1,), 9, dtype=torch.uint8, device="cuda")
        col = torch.full((n + 1,), 9, dtype=torch.int16, device="cuda")
        vloc = torch.full((n + 1,), 9, dtype=torch.int64, device="cuda")
        vlen = torch.full((n + 1,), 9, dtype=torch.int32, device="cuda")
        seb.dev_resolve_rows(dc, db, n, cap, status, col, vloc, vlen)
        only = torch.full((n + 1,), 9, dtype=torch.uint8, device="cuda")
        seb.dev_resolve_rows(dc, db, n, cap, only)  # col, vloc and vlen null
        torch.cuda.synchronize()
        st, co = status.cpu().numpy(), col.cpu().numpy().view(np.uint16)
        lo, le = vloc.cpu().numpy().view(np.uint64), vlen.cpu().numpy().view(np.uint32)
        assert st[n] == 9 and co[n] == 9 and lo[n] == 9 and le[n] == 9  # nothing past n keys
        assert np.array_equal(only.cpu().numpy(), st)
        for i, (ws, wc, wcell) in enumerate(want):
            assert (st[i], co[i]) == (ws, wc), (rows[i], st[i], co[i])
            if ws == br.GET_FOUND:
                assert lo[i] == int(bid[i, wc]) * 4096 + ((wcell >> 13) & 0x1FFF) and le[i] == wcell & 0x1FFF, rows[i]
            else:
                assert lo[i] == 0 and le[i] == 0, rows[i]
        named = {(br.TOMBSTONE, br.FOUND): (br.GET_FOUND, 1),  # the older value under a tombstone: the reference's answer
                 (br.TRUNC, br.FOUND): (br.GET_ERROR, 0), (br.FOUND, br.TRUNC): (br.GET_FOUND, 0),
                 (br.MISS, br.NONE): (br.GET_MISS, 0xFFFF), (br.TOMBSTONE, br.TOMBSTONE): (br.GET_MISS, 0xFFFF)}
        if cap == 2:
            for row, (ws, wc) in named.items():
                i = rows.index(row)
                assert (st[i], co[i]) == (ws, wc), row
    lib = seb.lib()
    assert lib.seb_dev_resolve_rows(dc.data_ptr(), db.data_ptr(), 5, 0, status.data_ptr(), None, None, None, None) == -1
    assert lib.seb_dev_resolve_rows(None, db.data_ptr(), 5, 2, status.data_ptr(), None, None, None, None) == -1
    assert lib.seb_dev_resolve_rows(dc.data_ptr(), db.data_ptr(), 5, 2, None, None, None, None, None) == -1
    assert lib.seb_dev_resolve_rows(dc.data_ptr(), db.data_ptr(), 0, 2, status.data_ptr(), None, None, None, None) == 0


def encode_index(entries) -> bytes:
    return struct.pack("<I", len(entries)) + b"".join(struct.pack("<IQ", len(k), o) + k for k, o in entries)


def lsm_walk(files, key: bytes):
    """lsm/lsm.go:168-198: every L0 file in insertion order, then per level 1..4 the first file by
    MinKey whose range covers the key; of those, the files whose filter may contain the key."""
    visit = [f for f in files if f["level"] == 0]
    for lvl in range(1, 5):
        for f in sorted((f for f in files if f["level"] == lvl), key=lambda f: f["min"]):
            if f["min"] <= key <= f["max"]:
                visit.append(f)
                break
    kb = np.frombuffer(key, np.uint8).reshape(1, -1)
    return [f for f in visit if oc.probe(f["bits"], f["m"], f["k"], kb, 1, stride=len(key))[0]]


def test_end_to_end(seb, torch_cuda):
    """The registry of test_gpu_locate.py::test_end_to_end_read_plan (3 overlapping L0 files, 4 L1
    files, 3 L2 files) with every file a real image from build_sstable: MultiGet -> locate ->
    dedup -> pool -> search -> resolve equals LSM.Get's walk with searchBlock per file, value bytes
    included.  Keys deleted in L0 and live below answer with the older value, as the reference does."""
    torch = torch_cuda
    rng = np.random.default_rng(21)
    universe = np.arange(0, 6000, 2)
    reg = seb.Registry(0)
    files = []

    def add(file_num, level, idx):
        keys = [kg.key16_bytes(int(i)) for i in idx]
        vals = [bytes([file_num & 0xFF]) + k[-6:] + bytes(rng.integers(0, 256, int(rng.integers(0, 294)), dtype=np.uint8))
                if rng.random() > 0.1 else b"" for k in keys]
        dele = [level == 0 and rng.random() < 0.3 for _ in keys]
        image, index = br.build_sstable(list(zip(keys, vals, dele)))
        m, k = oc.params(len(keys), 0.01)
        data, off = pack(keys)
        bits = oc.build(m, k, data, len(keys), offsets=off)
        slot = reg.put(file_num, level, bn.encode(bits, m, k), keys[0], keys[-1])
        reg.put_index(file_num, encode_index(index))
        files.append(dict(file=file_num, level=level, min=keys[0], max=keys[-1], bits=bits, m=m, k=k, slot=slot,
                          image=image, firsts=[k for k, _ in index], offs=[o for _, o in index],
                          value=dict(zip(keys, vals)), deleted={k for k, d in zip(keys, dele) if d}))

    for f in range(3):
        add(100 + f, 0, np.sort(rng.choice(universe, 400, replace=False)))
    for j, part in enumerate(np.array_split(universe[50:], 4)):
        add(1000 + j, 1, part)
    for j, part in reversed(list(enumerate(np.array_split(universe, 3)))):
        add(2000 + j, 2, part)
    by_file = {f["file"]: f for f in files}
    probes = [kg.key16_bytes(int(i)) for i in rng.integers(0, 6100, 1500)] + [files[0]["min"], files[-1]["max"]]
    n, cap = len(probes), reg.max_candidates()
    assert cap == 5
    # the reference: LSM.Get's walk, SSTable.Get's index step and searchBlock per visited file
    want = []
    under_tomb = 0
    for p in probes:
        cells, where = [], []
        for f in lsm_walk(files, p):
            e = bisect.bisect_right(f["firsts"], p) - 1
            blk = None if e < 0 else f["offs"][e]
            cells.append(br.cell(br.NONE) if blk is None else br.search_block_ref(f["image"][blk:blk + 4096], p))
            where.append((f, blk))
        st, col, c = br.lsm_get_ref(cells)
        val = None
        if st == br.GET_FOUND:
            f, blk = where[col]
            val = f["image"][blk + ((c >> 13) & 0x1FFF): blk + ((c >> 13) & 0x1FFF) + (c & 0x1FFF)]
            assert val == f["value"][p]
            under_tomb += any(x >> 28 == br.TOMBSTONE for x in cells[:col])
        want.append((st, col, val))
    found = sum(w[0] == br.GET_FOUND for w in want)
    assert n // 3 < found < 2 * n // 3 and under_tomb > 10 and not any(w[0] == br.GET_ERROR for w in want)

    dk = dev_fixed16(torch, seb, probes)
    rows = torch.zeros(n * cap, dtype=torch.int16, device="cuda")
    blocks = torch.zeros(n * cap, dtype=torch.int64, device="cuda")
    reg.multiget_list_dev(dk, rows, cap)
    reg.locate_dev(dk, rows, blocks, cap)
    torch.cuda.synchronize()
    slots = rows.cpu().numpy().view(np.uint16).reshape(n, cap)
    slot_file = np.full(65536, NO_BLOCK, np.uint64)
    for f in files:
        slot_file[f["slot"]] = f["file"]
    bid, uf, ub = seb.blocks_dedup(slot_file[slots], blocks.cpu().numpy().view(np.uint64).reshape(n, cap))
    images = [by_file[int(f)]["image"][int(o):int(o) + 4096] for f, o in zip(uf, ub)]
    assert len(images) > 100 and all(len(i) == 4096 for i in images)
    pool, blen = make_pool(images)
    dpool, dblen = dev_pool(torch, pool, blen)
    _, db, cells = run_search(torch, seb, dk, bid, dpool, dblen)
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    col = torch.zeros(n, dtype=torch.int16, device="cuda")
    vloc = torch.zeros(n, dtype=torch.int64, device="cuda")
    vlen = torch.zeros(n, dtype=torch.int32, device="cuda")
    seb.dev_resolve_rows(cells, db, n, cap, status, col, vloc, vlen)
    torch.cuda.synchronize()
    got = (status.cpu().numpy(), col.cpu().numpy().view(np.uint16), vloc.cpu().numpy().view(np.uint64),
           vlen.cpu().numpy().view(np.uint32))
    flat = pool.reshape(-1)
    for i, (st, wc, val) in enumerate(want):
        assert (got[0][i], got[1][i]) == (st, wc), i
        if st == br.GET_FOUND:
            assert flat[int(got[2][i]):int(got[2][i]) + int(got[3][i])].tobytes() == val, i
        else:
            assert got[2][i] == 0 and got[3][i] == 0, i
    # the host-buffer form gives the same answers
    hk = np.frombuffer(b"".join(probes), np.uint8).reshape(n, 16)
    hs, hc, hl, hv = seb.search_blocks(hk, bid, pool, blen)
    for a, b in zip((hs, hc, hl, hv), got):
        assert np.array_equal(a, b)
    # and so does the read plan of one registry call
    pf, pb = reg.multiget_blocks(seb.as_keys(hk))
    bid2, uf2, ub2 = seb.blocks_dedup(pf, pb)
    assert np.array_equal(bid2, bid) and np.array_equal(uf2, uf) and np.array_equal(ub2, ub)
    reg.close()


def test_binding_guards(seb, torch_cuda):
    """Short cells, bid, blen and pool tensors raise ValueError before any launch."""
    torch = torch_cuda
    n, cap, nb = 65, 3, 4
    dk = seb.dev_keys(torch.zeros(16 * n, dtype=torch.uint8, device="cuda"), n=n, stride=16)
    i32 = lambda k: torch.zeros(k, dtype=torch.int32, device="cuda")  # noqa: E731
    pool = torch.zeros(nb * 4096, dtype=torch.uint8, device="cuda")
    blen = torch.zeros(nb, dtype=torch.int16, device="cuda")
    with pytest.raises(ValueError):
        seb.dev_search_blocks(dk, i32(n * cap), cap, pool, blen, i32(n * cap - 1))
    with pytest.raises(ValueError):
        seb.dev_search_blocks(dk, i32(n * cap - 1), cap, pool, blen, i32(n * cap))
    with pytest.raises(ValueError):
        seb.dev_search_blocks(dk, i32(n * cap), cap, pool, blen[:-1], i32(n * cap), num_blocks=nb)
    with pytest.raises(ValueError):
        seb.dev_search_blocks(dk, i32(n * cap), cap, pool, i32(nb), i32(n * cap))  # 32-bit lengths
    with pytest.raises(ValueError):
        seb.dev_search_blocks(dk, i32(n * cap), cap, pool[:-1], blen, i32(n * cap))
    seb.dev_search_blocks(dk, i32(n * cap), cap, pool, blen, i32(n * cap))
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8, device="cuda")  # noqa: E731
    for kw in (dict(cells=i32(n * cap - 1)), dict(bid=i32(n * cap - 1)), dict(status=u8(n - 1)),
               dict(col=torch.zeros(n - 1, dtype=torch.int16, device="cuda")),
               dict(vloc=torch.zeros(n - 1, dtype=torch.int64, device="cuda")), dict(vlen=i32(n - 1))):
        a = dict(cells=i32(n * cap), bid=i32(n * cap), status=u8(n), col=None, vloc=None, vlen=None)
        a.update(kw)
        with pytest.raises(ValueError):
            seb.dev_resolve_rows(a["cells"], a["bid"], n, cap, a["status"], a["col"], a["vloc"], a["vlen"])
    seb.dev_resolve_rows(i32(n * cap), i32(n * cap), n, cap, u8(n))
    torch.cuda.synchronize()
    with pytest.raises(ValueError):  # the host form: a pool shorter than its blocks
        seb.search_blocks(np.zeros((2, 16), np.uint8), np.zeros((2, 1), np.uint32), np.zeros(4096, np.uint8),
                          np.zeros(2, np.uint16))
