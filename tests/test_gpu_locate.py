"""GPU: the registry's batched block locator (seb_registry_put_index / seb_registry_locate* /
seb_registry_multiget_blocks) against SSTable.Get's index step (lsm/sstable.go:210-222):

    blockIdx := sort.Search(len(index), func(i) { return index[i].Key > key })
    blockIdx == 0 -> not found, else index[blockIdx-1].BlockOffset

Python `bytes` ordering is Go string ordering, so the reference is bisect_right(index_keys, key) - 1.
The filters are tiny (a few hundred bits): the locator never reads them, the end-to-end test does."""
import bisect
import ctypes as C
import struct

import numpy as np
import pytest

import keygen as kg
from oracle import bloom_np as bn
from oracle import oracle_c as oc

pytestmark = pytest.mark.gpu

NO_BLOCK = 2**64 - 1
PAD = 0xFFFF


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def encode_index(entries) -> bytes:
    """[numEntries u32] then per entry [keySize u32][blockOffset u64][key], little-endian."""
    return struct.pack("<I", len(entries)) + b"".join(struct.pack("<IQ", len(k), o) + k for k, o in entries)


def pack(keys):
    """(bytes, u64 offsets[n+1]) of a list of byte strings."""
    off = np.zeros(len(keys) + 1, np.uint64)
    np.cumsum(np.array([len(k) for k in keys], np.uint64), out=off[1:])
    return np.frombuffer(b"".join(keys), np.uint8), off


def bloom_of(keys):
    """(encoded bloom block, bits, m, k) of a tiny filter over `keys` (at least one)."""
    m, k = oc.params(max(len(keys), 1), 0.01)
    data, off = pack(keys)
    bits = oc.build(m, k, data, len(keys), offsets=off)
    return bn.encode(bits, m, k), bits, m, k


def ref_block(entries, key: bytes) -> int:
    j = bisect.bisect_right([k for k, _ in entries], key) - 1
    return NO_BLOCK if j < 0 else entries[j][1]


def ref_rows(by_slot, probes, cand):
    """The reference for whole candidate rows: by_slot maps a live slot to its index entries."""
    want = np.full(cand.shape, NO_BLOCK, np.uint64)
    keys = {s: [k for k, _ in entries] for s, entries in by_slot.items()}
    for i, p in enumerate(probes):
        for j, s in enumerate(cand[i]):
            if int(s) in by_slot:
                e = bisect.bisect_right(keys[int(s)], p) - 1
                want[i, j] = NO_BLOCK if e < 0 else by_slot[int(s)][e][1]
    return want


def neighbours(key: bytes):
    """The key's predecessors and successors in string order that a bisection can mistake for it."""
    out = [key + b"\x00", key + b"\xff", key[:-1]]
    if key:
        out += [key[:-1] + bytes([(key[-1] + 1) & 0xFF]), key[:-1] + bytes([(key[-1] - 1) & 0xFF])]
    return out


def dev_varlen(torch, seb, keys, shift=3):
    """A device variable-length batch whose data pointer is odd and whose offsets[0] != 0."""
    data, off = pack(keys)
    buf = np.concatenate([np.full(1 + shift, 0xEE, np.uint8), data, np.full(4, 0xEE, np.uint8)])
    d = torch.from_numpy(buf).cuda()[1:]
    assert d.data_ptr() % 2 == 1
    o = torch.from_numpy((off + np.uint64(shift)).view(np.int64)).cuda()
    return seb.dev_keys(d, o)


def locate_dev(torch, seb, reg, dk, cand: np.ndarray) -> np.ndarray:
    n, cap = cand.shape
    dc = torch.from_numpy(np.ascontiguousarray(cand).view(np.int16).reshape(-1)).cuda() if cand.size else \
        torch.zeros(1, dtype=torch.int16, device="cuda")
    out = torch.full((max(n * cap, 1),), 5, dtype=torch.int64, device="cuda")
    reg.locate_dev(dk, dc, out, cap)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)[: n * cap].reshape(n, cap)


def test_bisection_edges(seb, torch_cuda):
    """One file per index size around every boundary a bisection (or a multi-way node of 8) has:
    each index key, its neighbours, a key below the first, above the last, and the empty key, in
    every file."""
    rng = np.random.default_rng(5)
    sizes = [0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 513]
    reg = seb.Registry(0)
    by_slot, probes = {}, [b"", b"\x00", b"\xff" * 24]
    for f, size in enumerate(sizes):
        keys = set()
        while len(keys) < size:
            keys.add(b"k" + bytes(rng.integers(1, 255, int(rng.integers(1, 20)), dtype=np.uint8)))
        entries = [(k, 4096 * j + f) for j, k in enumerate(sorted(keys))]
        slot = reg.put(10 + f, 0, bloom_of([b"x"])[0], b"a", b"z")
        reg.put_index(10 + f, encode_index(entries))
        assert reg.index_entries(10 + f) == size
        by_slot[slot] = entries
        for k, _ in entries:
            probes += [k] + neighbours(k)
    cand = np.tile(np.array(sorted(by_slot), np.uint16), (len(probes), 1))
    got = reg.locate(probes, cand)
    want = ref_rows(by_slot, probes, cand)
    assert got.shape == want.shape and np.array_equal(got, want)
    with seb.option("grid_cap", 2):  # two workgroups walk the cells' tiles in turns
        assert np.array_equal(reg.locate(probes, cand), want)
    assert (want[:, 0] == NO_BLOCK).all() and (want != NO_BLOCK).any()  # the empty index answers nothing
    reg.close()


def test_compare_order(seb, torch_cuda):
    """Go string order on the device: lengths 0..40, keys that tie on their first 16 bytes and
    differ in the tail, proper prefixes both ways, "ab" against "ab\\0", the bytes 0x00 / 0x7f /
    0x80 / 0xff, duplicate index keys (the last one answers); as a variable-length batch on an odd
    pointer with offsets[0] != 0 and as aligned 16-byte keys."""
    torch = torch_cuda
    p16 = b"0123456789abcdef"
    fam = [p16, p16 + b"\x00", p16 + b"a", p16 + b"a\x00", p16 + b"ab", p16 + b"b", p16 + b"\x7f", p16 + b"\x80",
           p16 + b"\xff" * 3, p16[:15], p16[:15] + b"\x00", p16[:8], p16[:8] + b"\x00" * 8]
    keys = [b"q" * n for n in range(41)] + fam
    keys += [b"ab", b"ab\x00", b"ab\x00\x00", b"a", b"a\x00", b"a\x7f", b"a\x80", b"a\xff", b"\x00", b"\x7f", b"\x80",
             b"\xff", b"\xff\xff"]
    keys += [b"dup", b"dup", b"dup", p16 + b"dup", p16 + b"dup", b"", b""]
    full = [(k, 1000 + j) for j, k in enumerate(sorted(keys))]
    tails = [(k, 7 * j) for j, k in enumerate(sorted(fam + [p16 + b"a", p16 + b"a"]))]  # every key past one prefix
    reg = seb.Registry(0)
    by_slot = {}
    for f, entries in enumerate((full, tails)):
        slot = reg.put(f, 0, bloom_of([b"x"])[0], b"a", b"z")
        reg.put_index(f, encode_index(entries))
        by_slot[slot] = entries
    probes = sorted(set(keys))
    probes += [q for k in probes for q in neighbours(k)]
    cand = np.tile(np.array(sorted(by_slot), np.uint16), (len(probes), 1))
    want = ref_rows(by_slot, probes, cand)
    assert np.array_equal(locate_dev(torch, seb, reg, dev_varlen(torch, seb, probes), cand), want)
    assert np.array_equal(reg.locate(probes, cand), want)
    # aligned fixed 16-byte keys (one 16-B load per key): every probe cut or zero-padded to 16 bytes
    fixed = sorted({(q + b"\x00" * 16)[:16] for q in probes} | {(q + b"\xff" * 16)[:16] for q in probes})
    d = torch.from_numpy(np.frombuffer(b"".join(fixed), np.uint8).copy()).cuda()
    assert d.data_ptr() % 16 == 0
    cand = np.tile(np.array(sorted(by_slot), np.uint16), (len(fixed), 1))
    got = locate_dev(torch, seb, reg, seb.dev_keys(d, n=len(fixed), stride=16), cand)
    assert np.array_equal(got, ref_rows(by_slot, fixed, cand))
    reg.close()


def test_rows(seb, torch_cuda):
    """Row shapes: cap 1 / 3 / 16 / 17 and n around the 64-lane and 256-thread boundaries, rows
    mixing live slots with padding, a freed slot id, ids past the table and 0xFFFE.  Padded and bad
    cells give NO_BLOCK, and nothing past the n * cap cells is written."""
    torch = torch_cuda
    rng = np.random.default_rng(9)
    reg = seb.Registry(0)
    by_slot = {}
    for f in range(5):
        entries = [(kg.key16_bytes(int(i)), 4096 * j + f) for j, i in enumerate(range(3 * f, 3000, 37 + f))]
        slot = reg.put(f, 0, bloom_of([b"x"])[0], b"a", b"z")
        reg.put_index(f, encode_index(entries))
        by_slot[slot] = entries
    reg.remove(1)  # slot 1 stays inside the table, free
    free = [s for s in by_slot if s not in reg.slots()]
    assert free == [1]
    del by_slot[1]
    ids = np.array(sorted(by_slot) + [PAD, PAD, PAD, 1, 5, 4095, 0xFFFE], np.uint16)
    for cap in (1, 3, 16, 17):
        for n in (0, 1, 63, 64, 65, 257):
            probes = [kg.key16_bytes(int(i)) for i in rng.integers(0, 3100, n)]
            cand = ids[rng.integers(0, len(ids), (n, cap))]
            data = np.frombuffer(b"".join(probes), np.uint8).copy() if n else np.zeros(16, np.uint8)
            dk = seb.dev_keys(torch.from_numpy(data).cuda(), n=n, stride=16)
            dc = torch.from_numpy(np.append(cand.reshape(-1), np.uint16(0)).view(np.int16)).cuda()  # a live id past the end
            out = torch.full((n * cap + 1,), 5, dtype=torch.int64, device="cuda")
            reg.locate_dev(dk, dc, out, cap)
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint64)
            assert got[n * cap] == 5, (cap, n)
            want = ref_rows(by_slot, probes, cand)
            assert np.array_equal(got[: n * cap].reshape(n, cap), want), (cap, n)
            if n:
                assert np.array_equal(reg.locate(np.frombuffer(data, np.uint8).reshape(n, 16), cand), want), (cap, n)
    with pytest.raises(seb.SebError) as e:  # cap == 0
        reg.locate_dev(dk, dc, out, 0)
    assert e.value.code == -1
    rc = seb.lib().seb_registry_locate_dev(reg._h, C.byref(dk), None, 3, out.data_ptr(), None)
    assert rc == -1 and "null" in seb.last_error()
    reg.close()


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


def three_level_registry(seb, rng):
    """(registry, files): 3 overlapping L0 files, a disjoint L1 of 4, an L2 of 3 put out of order;
    each file's index is every 8th key."""
    universe = np.arange(0, 6000, 2)
    reg = seb.Registry(0)
    files = []

    def add(file_num, level, idx):
        keys = [kg.key16_bytes(int(i)) for i in idx]
        block, bits, m, k = bloom_of(keys)
        entries = [(keys[j], 4096 * (j // 8) + 64) for j in range(0, len(keys), 8)]
        slot = reg.put(file_num, level, block, keys[0], keys[-1])
        reg.put_index(file_num, encode_index(entries))
        files.append(dict(file=file_num, level=level, min=keys[0], max=keys[-1], bits=bits, m=m, k=k, slot=slot,
                          entries=entries))

    for f in range(3):
        add(100 + f, 0, np.sort(rng.choice(universe, 400, replace=False)))
    for j, part in enumerate(np.array_split(universe[50:], 4)):  # the first keys are below every L1 file
        add(1000 + j, 1, part)
    for j, part in reversed(list(enumerate(np.array_split(universe, 3)))):
        add(2000 + j, 2, part)
    return reg, files


def read_plan_ref(files, probes, cap):
    """(file numbers, slots, block offsets), each (n, cap): LSM.Get's walk, then SSTable.Get's index step."""
    n = len(probes)
    want_files = np.full((n, cap), NO_BLOCK, np.uint64)
    want_slots = np.full((n, cap), PAD, np.uint16)
    want_blocks = np.full((n, cap), NO_BLOCK, np.uint64)
    for i, p in enumerate(probes):
        for j, f in enumerate(lsm_walk(files, p)):
            want_files[i, j], want_slots[i, j], want_blocks[i, j] = f["file"], f["slot"], ref_block(f["entries"], p)
    return want_files, want_slots, want_blocks


def test_end_to_end_read_plan(seb, torch_cuda):
    """A 3-level registry (overlapping L0 files, a disjoint L1, an L2) with each file's index being
    every 8th key: multiget_list_dev then locate_dev equals LSM.Get's walk followed by
    SSTable.Get's index step, and multiget_blocks returns the same pairs as file numbers."""
    torch = torch_cuda
    rng = np.random.default_rng(21)
    reg, files = three_level_registry(seb, rng)
    probes = [kg.key16_bytes(int(i)) for i in rng.integers(0, 6100, 1500)] + [files[0]["min"], files[-1]["max"]]
    n, cap = len(probes), reg.max_candidates()
    assert cap == 5
    want_files, want_slots, want_blocks = read_plan_ref(files, probes, cap)
    assert (want_blocks != NO_BLOCK).sum() > n // 2  # about every second probe is present in two levels
    dk = seb.dev_keys(torch.from_numpy(np.frombuffer(b"".join(probes), np.uint8).copy()).cuda(), n=n, stride=16)
    rows = torch.zeros(n * cap, dtype=torch.int16, device="cuda")
    blocks = torch.zeros(n * cap, dtype=torch.int64, device="cuda")
    reg.multiget_list_dev(dk, rows, cap)
    reg.locate_dev(dk, rows, blocks, cap)
    torch.cuda.synchronize()
    assert np.array_equal(rows.cpu().numpy().view(np.uint16).reshape(n, cap), want_slots)
    assert np.array_equal(blocks.cpu().numpy().view(np.uint64).reshape(n, cap), want_blocks)
    # the read plan from one call: cap = 1 is too narrow, the call says so and names the width
    hk = seb.as_keys(np.frombuffer(b"".join(probes), np.uint8).reshape(n, 16))
    need = C.c_uint32()
    small = np.zeros((n, 1), np.uint64)
    rc = seb.lib().seb_registry_multiget_blocks(reg._h, hk.ref, small.ctypes.data, small.ctypes.data, 1, C.byref(need))
    assert rc == -4 and need.value == cap
    got_files, got_blocks = reg.multiget_blocks(hk)  # retries from cap = 1
    assert got_files.shape == (n, cap)
    assert np.array_equal(got_files, want_files) and np.array_equal(got_blocks, want_blocks)
    assert np.array_equal(got_files, reg.multiget_files(hk))
    reg.close()


def test_host_forms_chunked(seb, torch_cuda, monkeypatch):
    """The host-pointer forms past their first chunk.  The registry's context reads SEB_CHUNK_BYTES
    when the first host call creates it: 4096 bytes are 256 16-byte keys, so the batches are no
    chunk, one key, one full chunk, a one-key second chunk, and four chunks with a one-key tail."""
    monkeypatch.setenv("SEB_CHUNK_BYTES", "4096")
    rng = np.random.default_rng(23)
    reg, files = three_level_registry(seb, rng)
    cap = reg.max_candidates()
    assert cap == 5
    probes = [kg.key16_bytes(int(i)) for i in rng.integers(0, 6100, 767)] + [files[0]["min"], files[-1]["max"]]
    want_files, want_slots, want_blocks = read_plan_ref(files, probes, cap)
    want_mask = np.zeros(len(probes), np.uint64)
    for j in range(cap):
        live = want_slots[:, j] != PAD
        want_mask[live] |= np.uint64(1) << want_slots[live, j].astype(np.uint64)
    by_slot = {f["slot"]: f["entries"] for f in files}
    mixed = want_slots.copy()  # locate's own rows: every slot, padding and a free id, whatever the filters say
    mixed[::3] = np.array(sorted(by_slot)[:cap], np.uint16)
    mixed[1::7, 1] = 4095
    want_mixed = ref_rows(by_slot, probes, mixed)
    assert (want_blocks != NO_BLOCK).sum() > len(probes) // 2
    for n in (0, 1, 256, 257, 769):
        hk = seb.as_keys(np.frombuffer(b"".join(probes[:n]), np.uint8).reshape(n, 16))
        assert np.array_equal(reg.multiget(hk), want_mask[:n]), n
        assert np.array_equal(reg.multiget_list(hk), want_slots[:n]), n
        wide = reg.multiget_list(hk, cap=cap + 2)  # an odd row width
        assert wide.shape == (n, cap + 2), n
        assert np.array_equal(wide[:, :cap], want_slots[:n]) and (wide[:, cap:] == PAD).all(), n
        got = reg.multiget_files(hk)
        assert got.shape == (n, cap) and np.array_equal(got, want_files[:n]), n
        assert np.array_equal(reg.locate(hk, want_slots[:n]), want_blocks[:n]), n
        assert np.array_equal(reg.locate(hk, mixed[:n]), want_mixed[:n]), n
        got_files, got_blocks = reg.multiget_blocks(hk)
        assert got_files.shape == (n, cap), n
        assert np.array_equal(got_files, want_files[:n]) and np.array_equal(got_blocks, want_blocks[:n]), n
    reg.close()


def test_lifecycle(seb, torch_cuda):
    """Indexes follow their files: counts, a reused slot answers from its new file's index, a
    missing index fails the call by name, bad blocks are refused and leave the file usable."""
    reg = seb.Registry(0)
    block = bloom_of([b"b", b"m"])[0]
    a = [(b"b", 10), (b"m", 20)]
    b = [(b"c", 111), (b"h", 222), (b"p", 333)]
    s1 = reg.put(1, 0, block, b"b", b"m")
    s2 = reg.put(2, 0, block, b"b", b"m")
    reg.put_index(1, encode_index(a))
    probes = [b"a", b"b", b"d", b"j", b"m", b"z"]
    cand = np.tile(np.array([s1, s2], np.uint16), (len(probes), 1))
    with pytest.raises(seb.SebError) as e:  # file 2 has no index yet
        reg.locate(probes, cand)
    assert e.value.code == -1 and "file 2 " in seb.last_error()
    with pytest.raises(seb.SebError) as e:
        reg.multiget_blocks(probes, cap=2)
    assert e.value.code == -1 and "file 2 " in seb.last_error()
    with pytest.raises(seb.SebError) as e:
        reg.index_entries(2)
    assert e.value.code == -1
    # refused blocks: truncated, unsorted; the file keeps no index and still answers multiget
    for bad, code in ((encode_index(b)[:-1], -5), (b"\x01\x00", -5), (encode_index(b[::-1]), -1)):
        with pytest.raises(seb.SebError) as e:
            reg.put_index(2, bad)
        assert e.value.code == code
    assert int(reg.multiget([b"b", b"m"])[0]) == (1 << s1) | (1 << s2)
    reg.put_index(2, encode_index([]))
    assert (reg.index_entries(1), reg.index_entries(2)) == (2, 0)
    want = ref_rows({s1: a, s2: []}, probes, cand)
    assert np.array_equal(reg.locate(probes, cand), want) and (want[:, 1] == NO_BLOCK).all()
    for file_num in (1, 99):  # a second index; an unknown file
        with pytest.raises(seb.SebError) as e:
            reg.put_index(file_num, encode_index(a))
        assert e.value.code == -1
    # compaction: file 1 goes, file 3 takes its slot with another index
    reg.remove(1)
    with pytest.raises(seb.SebError):
        reg.index_entries(1)
    assert np.array_equal(reg.locate(probes, cand), ref_rows({s2: []}, probes, cand))  # the freed slot answers nothing
    assert reg.put(3, 0, block, b"b", b"m") == s1
    reg.put_index(3, encode_index(b))
    assert reg.index_entries(3) == 3
    assert np.array_equal(reg.locate(probes, cand), ref_rows({s1: b, s2: []}, probes, cand))
    files, blocks = reg.multiget_blocks([b"m"], cap=2)
    assert files.tolist() == [[2, 3]] and blocks.tolist() == [[NO_BLOCK, 222]]  # L0 in insertion order
    reg.close()


def test_binding_guards(seb, torch_cuda):
    """The device wrappers check buffer sizes before the call: a short buffer is a ValueError, not
    an out-of-bounds write."""
    torch = torch_cuda
    reg = seb.Registry(0)
    reg.put(1, 0, bloom_of([b"x"])[0], b"a", b"z")
    reg.put_index(1, encode_index([(b"a", 0)]))
    n, cap = 65, 3
    dk = seb.dev_keys(torch.zeros(16 * n, dtype=torch.uint8, device="cuda"), n=n, stride=16)
    cand = torch.zeros(n * cap, dtype=torch.int16, device="cuda")
    with pytest.raises(ValueError):
        reg.locate_dev(dk, cand, torch.zeros(n * cap - 1, dtype=torch.int64, device="cuda"), cap)
    with pytest.raises(ValueError):
        reg.locate_dev(dk, cand[:-1], torch.zeros(n * cap, dtype=torch.int64, device="cuda"), cap)
    reg.locate_dev(dk, cand, torch.zeros(n * cap, dtype=torch.int64, device="cuda"), cap)
    torch.cuda.synchronize()
    reg.close()
    m, k = seb.params(1000, 0.01)
    assert seb.pack6_supported(m, k) and seb.packed6_bytes(n) == 768 > 6 * n
    with pytest.raises(ValueError):
        seb.dev_pack_residues6(dk, m, k, torch.zeros(6 * n, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        seb.dev_probe_multi_packed6(torch.zeros(6 * n, dtype=torch.uint8, device="cuda"), n, [(seb.new_words(m), m, k)],
                                    torch.zeros(n, dtype=torch.uint8, device="cuda"))
    buf = torch.zeros(seb.packed6_bytes(n), dtype=torch.uint8, device="cuda")
    seb.dev_pack_residues6(dk, m, k, buf)
    torch.cuda.synchronize()
