"""GPU: the batched SSTable builder (include/seb_bloom.h, the SSTable builder group).

seb_dev_sst_plan / seb_dev_sst_encode equal the host half (seb_sst_plan / seb_sst_encode, itself held to
the restatement of SSTableBuilder in test_sst_build.py) byte for byte: one file and many files per call,
file boundaries at 0-entry and 1-entry files and inside a block's worth of entries, runs of T - 1, T and
T + 1 entries for the cut's tile size T, odd data pointers, offsets[0] != 0 and the fixed 16-byte-stride
layout.  Outputs start as 0xA5 between guard bytes: the padding must come out zero and the guards
untouched.  seb_sst_build gives the restatement's whole file image, and the files it writes serve the
read side (registry, locate, block search, resolve) end to end.

Beyond four tiles and 45 files (each test asserts by arithmetic that its shape crosses its threshold):
  65, 257, 1025, 1500 files over four tiles   a second workgroup of k_sst_walk and k_sst_filemeta (64 files each),
                                              of k_sst_files and k_sst_sizes (256), the carry of the meta_len scan
  40 tiles cut into 300 files                 files over several tiles, tiles with several files: k_sst_walk's hops
  1024 T + 1025 entries, one and three files  1026 tiles: the carry of k_sst_scan; against the host half and
                                              against scale_ref's closed form
The 16 bytes behind the workspace stay 0x5A through plan and encode."""
import ctypes as C
import struct

import numpy as np
import pytest

import block_ref as br
import keygen as kg
import scale_ref as sc
import sstable_ref as sr

pytestmark = pytest.mark.gpu

GUARD = 64
NO_BLOCK = 2**64 - 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def dev_run(torch, seb, items, layout):
    """The run on the device.  "odd": variable-length keys and values behind odd data pointers with
    offsets[0] != 0; "even": the same, 16-byte aligned from offset 0; "fixed16": 16-byte keys at a
    16-byte stride without an offset array."""
    if layout == "fixed16":
        assert all(len(k) == 16 for k, _, _ in items)
        return dev_packed(torch, seb, sr.pack(items), layout)
    kp, vp = (3, 5) if layout == "odd" else (0, 0)
    return dev_packed(torch, seb, sr.pack(items, key_pad=kp, val_pad=vp), layout)


def dev_packed(torch, seb, packed, layout):
    """dev_run over sstable_ref.pack's five arrays (the pads already in them)."""
    kd, koff, vd, voff, dl = packed
    if layout == "fixed16":
        dk = seb.dev_keys(torch.from_numpy(np.concatenate([kd, np.zeros(16, np.uint8)])).cuda(), n=len(dl), stride=16)
        dv = torch.from_numpy(np.concatenate([vd, np.zeros(1, np.uint8)])).cuda()
    else:
        lead = 1 if layout == "odd" else 0
        k = torch.from_numpy(np.concatenate([np.full(lead, 0xEE, np.uint8), kd, np.full(3, 0xEE, np.uint8)])).cuda()[lead:]
        dv = torch.from_numpy(np.concatenate([np.full(lead, 0xDD, np.uint8), vd, np.full(3, 0xDD, np.uint8)])).cuda()[lead:]
        assert k.data_ptr() % 2 == lead and dv.data_ptr() % 2 == lead
        dk = seb.dev_keys(k, torch.from_numpy(koff.view(np.int64)).cuda())
    dvoff = torch.from_numpy(voff.view(np.int64)).cuda()
    ddel = torch.from_numpy(np.concatenate([dl, np.zeros(1, np.uint8)])).cuda()
    return dk, dv, dvoff, ddel


def guarded(torch, size, lead=GUARD):
    buf = torch.full((lead + size + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[lead:lead + size]


def check_guards(buf, size, lead=GUARD):
    h = buf.cpu().numpy()
    assert (h[:lead] == 0xA5).all() and (h[lead + size:] == 0xA5).all(), "bytes outside the stated sizes were written"
    return h[lead:lead + size].tobytes()


def device_sections(torch, seb, items, file_begin, layout, packed=None):
    """Plan + encode on the device: (sizes per file, data, blen, index, metadata); the run as items, or as
    sstable_ref.pack's arrays."""
    dk, dv, dvoff, ddel = dev_run(torch, seb, items, layout) if packed is None else dev_packed(torch, seb, packed, layout)
    nf = len(file_begin) - 1
    ws = torch.full((seb.dev_sst_workspace_size(dk.n, nf) + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    sizes = seb.dev_sst_plan(dk, dvoff, file_begin, ws[:-16])
    blocks, d, x, m = (sum(s[j] for s in sizes) for j in range(4))
    bd, data = guarded(torch, d)
    assert data.data_ptr() % 16 == 0
    bx, index = guarded(torch, x, lead=GUARD + 1)  # the index and the metadata at odd addresses
    bm, meta = guarded(torch, m, lead=GUARD + 3)
    bl, blen = guarded(torch, 2 * blocks)
    seb.dev_sst_encode(dk, dv, dvoff, ddel, file_begin, sizes, ws[:-16], data, index, meta, blen=blen.view(torch.int16))
    torch.cuda.synchronize()
    assert (ws[-16:].cpu().numpy() == 0x5A).all(), "the plan or the encode wrote past the workspace"
    return (sizes, check_guards(bd, d), np.frombuffer(check_guards(bl, 2 * blocks), np.uint16).tolist(),
            check_guards(bx, x, GUARD + 1), check_guards(bm, m, GUARD + 3))


def host_sections(seb, items, file_begin):
    """The host half per file, concatenated the way the device lays the files out."""
    sizes, data, index, meta, blens = [], [], [], [], []
    for f in range(len(file_begin) - 1):
        part = items[file_begin[f]:file_begin[f + 1]]
        kd, koff, vd, voff, dl = sr.pack(part)
        sizes.append(seb.sst_plan((kd, koff), voff))
        d, x, m = seb.sst_encode((kd, koff), vd, voff, dl)
        data.append(d), index.append(x), meta.append(m)
        blens += sr.sections(part)[3]
    return sizes, b"".join(data), blens, b"".join(index), b"".join(meta)


def host_sections_packed(seb, run, file_begin):
    """host_sections over a scale_ref.sst_run; the true block lengths are not the host half's to give."""
    sizes, data, index, meta = [], [], [], []
    for lo, hi in zip(file_begin[:-1], file_begin[1:]):
        kd, koff, vd, voff, dl = sc.sst_slice(run, lo, hi)
        sizes.append(seb.sst_plan((kd, koff), voff))
        d, x, m = seb.sst_encode((kd, koff), vd, voff, dl)
        data.append(d), index.append(x), meta.append(m)
    return sizes, b"".join(data), None, b"".join(index), b"".join(meta)


def compare(torch, seb, items, file_begin, layout, name=""):
    want = host_sections(seb, items, file_begin)
    got = device_sections(torch, seb, items, file_begin, layout)
    check_sections(got, want, layout, name)
    return want[0]


def check_sections(got, want, layout, name):
    assert got[0] == want[0], (name, "sizes")
    assert want[2] is None or got[2] == want[2], (name, "blen")
    for j, what in ((1, "data"), (3, "index"), (4, "metadata")):
        if got[j] != want[j]:
            at = next(i for i, (a, b) in enumerate(zip(got[j], want[j])) if a != b)
            raise AssertionError(f"{name} {layout}: {what} differs first at byte {at} (block {at // 4096}, +{at % 4096}): "
                                 f"{got[j][at:at + 8].hex()} != {want[j][at:at + 8].hex()}")


DEVICE_SHAPES = [(n, it) for n, it in sr.shapes() if not n.endswith("_over") and n != "none"]


@pytest.mark.parametrize("name,items", DEVICE_SHAPES, ids=[n for n, _ in DEVICE_SHAPES])
def test_shapes_one_file(seb, torch_cuda, name, items):
    compare(torch_cuda, seb, items, [0, len(items)], "odd", name)
    compare(torch_cuda, seb, items, [0, len(items)], "even", name)
    if len(items) > 2:  # the same run as files: an empty one first, a cut after one entry, a cut in mid block
        compare(torch_cuda, seb, items, [0, 0, 1, len(items) // 2, len(items) // 2, len(items), len(items)], "odd", name)


def small_items(rng, n):
    """Entries of about 20 bytes (some 200 per block), sorted distinct keys."""
    return [(b"%08d" % i, bytes(rng.integers(0, 256, int(rng.integers(0, 8)), dtype=np.uint8)), int(i % 7 == 0))
            for i in range(n)]


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_tile_edges(seb, torch_cuda, delta):
    """Runs of T - 1, T and T + 1 entries for the cut's tile size T, as one file and as files that end
    and begin at the tile boundary and next to it; blocks of some 200 entries straddle the boundary."""
    T = seb.SST_TILE
    rng = np.random.default_rng(100 + delta)
    n = T + delta
    items = small_items(rng, n)
    sizes = compare(torch_cuda, seb, items, [0, n], "odd", f"T{delta:+d}")
    assert sizes[0][0] > 4
    items = small_items(rng, 2 * T + 300)
    compare(torch_cuda, seb, items, [0, n, 2 * T, 2 * T, len(items)], "even", f"files at T{delta:+d}")
    compare(torch_cuda, seb, items, [0, 1, n - 1, n, n + 1, len(items)], "odd", f"one-entry files at T{delta:+d}")


def test_many_files_random(seb, torch_cuda):
    """Random runs over several tiles cut into many files, empty and one-entry files among them, and a
    run of large entries (a block per entry or two, so block starts are dense in a tile)."""
    torch = torch_cuda
    rng = np.random.default_rng(7)
    items = sr.random_items(rng, 3600)
    n = len(items)
    cuts = sorted(set(int(c) for c in rng.integers(0, n, 40)) | {0, n})
    fb = [0] + cuts + [cuts[5], cuts[5] + 1] + [n]  # duplicates make empty files
    fb = sorted(fb)
    sizes = compare(torch, seb, items, fb, "odd", "random")
    assert any(s[0] == 0 for s in sizes) and sum(s[0] for s in sizes) > 100
    big = [(b"big%05d" % i, bytes(rng.integers(0, 256, int(rng.integers(1500, 4070)), dtype=np.uint8)), 0) for i in range(1300)]
    compare(torch, seb, big, [0, 700, 1300], "even", "big entries")
    tiny = [(b"", b"", i % 2) for i in range(3000)]  # 454 entries per block: the longest hops between block starts
    compare(torch, seb, tiny, [0, 455, 3000], "odd", "empty entries")


@pytest.mark.parametrize("nf", [65, 257, 1025, 1500])
def test_file_counts(seb, torch_cuda, nf):
    """More files than a workgroup of the per-file kernels has lanes: 64 for k_sst_walk and k_sst_filemeta, 256 for
    k_sst_files and k_sst_sizes, and more than 1024 for the carry of the meta_len scan.  Some 4,000 entries over
    four tiles; files that end before, at and after a tile edge, empty and one-entry files among them."""
    T = seb.SST_TILE
    assert (nf + 63) // 64 >= 2  # every nf: k_sst_walk, k_sst_filemeta
    assert (nf + 255) // 256 >= 2 or nf == 65  # k_sst_files, k_sst_sizes
    assert nf > 1024 or nf in (65, 257)  # the meta_len scan's second chunk
    rng = np.random.default_rng(nf)
    items = sr.random_items(rng, 4000)
    n = len(items)
    assert 3 * T + 1 < n <= 4000
    cuts = [T - 1, T, T + 1, 2 * T, 2 * T, 2 * T + 1, 3 * T - 1, 3 * T - 1, 3 * T + 1, n]
    cuts += [int(c) for c in rng.integers(0, n + 1, nf - 1 - len(cuts))]
    fb = [0] + sorted(cuts) + [n]
    lens = [b - a for a, b in zip(fb[:-1], fb[1:])]
    assert len(fb) == nf + 1 and 0 in lens and 1 in lens and lens[-1] == 0
    want = host_sections(seb, items, fb)
    ref = [sr.sections(items[a:b]) for a, b in zip(fb[:-1], fb[1:])]
    assert want[1] == b"".join(r[0] for r in ref) and want[3] == b"".join(r[1] for r in ref)
    assert want[4] == b"".join(r[2] for r in ref) and want[0] == [(len(r[3]), len(r[0]), len(r[1]), len(r[2]), 0) for r in ref]
    for layout in ("odd", "even"):
        check_sections(device_sections(torch_cuda, seb, items, fb, layout), want, layout, f"{nf} files")


def test_many_tiles_and_many_files(seb, torch_cuda):
    """40 tiles cut into 300 files at random places: files that span several tiles (k_sst_walk's lane hops from
    exit to exit) and tiles that hold several files (their lanes write the same entry point)."""
    T = seb.SST_TILE
    rng = np.random.default_rng(40)
    n = 40 * T
    items = small_items(rng, n)
    # 40 cuts anywhere, 259 crowded into six of the tiles: long files between the crowds, many files to a tile in them
    crowd = np.concatenate([rng.integers(10 * T, 12 * T, 100), rng.integers(25 * T, 29 * T, 159)])
    fb = [0] + sorted(int(c) for c in np.concatenate([rng.integers(0, n + 1, 40), crowd])) + [n]
    lens = [b - a for a, b in zip(fb[:-1], fb[1:])]
    tiles_of = [(b - 1) // T - a // T + 1 for a, b in zip(fb[:-1], fb[1:]) if b > a]
    assert len(lens) == 300 and (300 + 63) // 64 >= 2 and max(tiles_of) >= 3 and max(lens) > 2 * T
    assert max(np.bincount([c // T for c in fb[1:-1]], minlength=40)) >= 3 and n // T == 40
    want = host_sections(seb, items, fb)
    check_sections(device_sections(torch_cuda, seb, items, fb, "odd"), want, "odd", "40 tiles, 300 files")


@pytest.mark.parametrize("files", [1, 3])
def test_scan_carry_over_more_than_1024_tiles(seb, torch_cuda, files):
    """1026 tiles: k_sst_scan's second chunk takes the first chunk's sum as its carry, for the tiles' block counts
    and index bytes.  One file, and three files cut at entries that are no multiple of the tile."""
    T = seb.SST_TILE
    n = 1024 * T + 1025
    assert -(-n // T) > 1024
    fb = [0, n] if files == 1 else [0, 300 * T + 77, 301 * T - 5, n]
    assert all(c % T for c in fb[1:])
    run = sc.sst_run(n)
    got = device_sections(torch_cuda, seb, None, fb, "even", packed=tuple(a.copy() for a in run))  # run is read-only
    check_sections(got, host_sections_packed(seb, run, fb), "even", f"1026 tiles, {files} files: host half")
    check_sections(got, sc.sst_cut(run, fb), "even", f"1026 tiles, {files} files: closed form")


def test_fixed_stride_layout(seb, torch_cuda):
    rng = np.random.default_rng(3)
    n = 2500
    keys = sorted({kg.key16_bytes(int(i)) for i in rng.integers(0, 10**6, n)})
    items = [(k, bytes(rng.integers(0, 256, 100, dtype=np.uint8)), int(rng.random() < 0.1)) for k in keys]
    sizes = compare(torch_cuda, seb, items, [0, len(items)], "fixed16", "lsm entries")
    assert sizes[0][0] == -(-len(items) // 32)  # 125-byte entries: 32 per block
    compare(torch_cuda, seb, items, [0, 1000, 1001, len(items)], "fixed16", "lsm entries, 3 files")


def test_no_entries(seb, torch_cuda):
    torch = torch_cuda
    dk = seb.dev_keys(torch.zeros(16, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
    voff = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.zeros(16, dtype=torch.uint8, device="cuda")
    assert seb.dev_sst_workspace_size(0, 2) == 0
    sizes = seb.dev_sst_plan(dk, voff, [0, 0, 0], ws)
    assert sizes == [(0, 0, 4, 8, 0)] * 2
    out = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
    seb.dev_sst_encode(dk, None, voff, None, [0, 0, 0], sizes, ws, out, out, out)  # n == 0: nothing is launched
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all()


def test_oversized_entries(seb, torch_cuda):
    """A file with an oversized entry: the plan reports it, encode refuses with SEB_ERR_RANGE naming the
    file, and sst_build still returns the reference's exact image (through the host half)."""
    torch = torch_cuda
    by = dict(sr.shapes())
    ctx = seb.Ctx(0)
    for name in ("start_over", "middle_over", "end_over", "alone_over", "bigkey_over"):
        items = by[name]
        first = by["fill34"]
        run = first + items
        dk, dv, dvoff, ddel = dev_run(torch, seb, run, "odd")
        fb = [0, len(first), len(run)]
        ws = torch.zeros(seb.dev_sst_workspace_size(len(run), 2), dtype=torch.uint8, device="cuda")
        sizes = seb.dev_sst_plan(dk, dvoff, fb, ws)
        kd, koff, vd, voff, dl = sr.pack(items)
        assert sizes[1] == seb.sst_plan((kd, koff), voff) and sizes[1][4] >= 1 and sizes[0][4] == 0, name
        d, x, m = (sum(s[j] for s in sizes) for j in (1, 2, 3))
        bufs = [torch.full((v + 16,), 0xA5, dtype=torch.uint8, device="cuda") for v in (d, x, m)]
        with pytest.raises(seb.SebError) as e:
            seb.dev_sst_encode(dk, dv, dvoff, ddel, fb, sizes, ws, *bufs)
        assert e.value.code == -4 and "file 1" in str(e.value), name
        torch.cuda.synchronize()
        assert all((b.cpu().numpy() == 0xA5).all() for b in bufs)
        assert ctx.sst_build((kd, koff), vd, voff, dl) == sr.build_file(items), name
    ctx.close()


@pytest.mark.parametrize("expected", ["n", 100000])
def test_sst_build_file_image(seb, torch_cuda, expected):
    rng = np.random.default_rng(12)
    ctx = seb.Ctx(0)
    runs = [(n, it) for n, it in sr.shapes() if n in ("none", "one", "fill34", "empty455", "deleted_bytes", "long_keys")]
    runs.append(("random", sr.random_items(rng, 1500)))
    for name, items in runs:
        exp = len(items) if expected == "n" else expected
        kd, koff, vd, voff, dl = sr.pack(items, key_pad=1, val_pad=2)
        got = ctx.sst_build((kd, koff), vd, voff, dl, expected_keys=exp)
        want = sr.build_file(items, expected_keys=exp)
        assert len(got) == len(want) and got == want, name
    # fixed-stride keys, no deleted array, the module-level form
    keys = np.frombuffer(b"".join(kg.key16_bytes(i) for i in range(0, 900, 3)), np.uint8).reshape(-1, 16)
    items = [(keys[i].tobytes(), b"v%d" % i, 0) for i in range(len(keys))]
    _, _, vd, voff, _ = sr.pack(items)
    assert seb.sst_build(keys, vd, voff, expected_keys=len(items) if expected == "n" else expected) == \
        sr.build_file(items, expected_keys=len(items) if expected == "n" else expected)
    # expected_keys == 0 with entries: the reference's Add would take a remainder by zero
    with pytest.raises(seb.SebError) as e:
        ctx.sst_build(keys, vd, voff, expected_keys=0)
    assert e.value.code == -1
    # the retry contract: a capacity below *need names the size
    kb = seb.as_keys(keys)
    need = C.c_uint64()
    small = np.zeros(100, np.uint8)
    rc = seb.lib().seb_sst_build(ctx._p, kb.ref, vd.ctypes.data, voff.ctypes.data, None, len(items), small.ctypes.data, 100,
                                 C.byref(need))
    assert rc == -4 and need.value == len(sr.build_file(items)) and not small.any()
    ctx.close()


def test_end_to_end_files_serve_the_read_side(seb, torch_cuda):
    """Three overlapping L0 files of a few thousand keys, with tombstones and overwritten keys, built by
    sst_build; their footers are parsed here, the filter and index sections go into a registry, the
    device-written data sections are the block pool (blen from the encoder), and
    multiget_blocks -> blocks_dedup -> dev_search_blocks -> dev_resolve_rows answers every present and
    absent key as LSM.Get does over the restatement's files."""
    torch = torch_cuda
    rng = np.random.default_rng(31)
    universe = np.arange(0, 9000, 2)
    reg = seb.Registry(0)
    ctx = seb.Ctx(0)
    files, all_items, fb = [], [], [0]
    for f in range(3):
        idx = np.sort(rng.choice(universe, 2500, replace=False))
        keys = [kg.key16_bytes(int(i)) for i in idx]
        items = [(k, bytes([f]) + bytes(rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8)), int(rng.random() < 0.25))
                 for k in keys]
        kd, koff, vd, voff, dl = sr.pack(items)
        image = ctx.sst_build((kd, koff), vd, voff, dl)
        assert image == sr.build_file(items)
        io, bo, mo = sr.parse_footer(image)
        index, meta, bloom = image[io:mo], image[mo:bo], image[bo:-sr.FOOTER]
        kmin, kmax = struct.unpack_from("<II", meta)
        assert meta[8:8 + kmin] == keys[0] and meta[8 + kmin:8 + kmin + kmax] == keys[-1]
        reg.put(100 + f, 0, bloom, keys[0], keys[-1])
        reg.put_index(100 + f, index)
        files.append(dict(file=100 + f, items={k: (v, d) for k, v, d in items}, blocks=io // 4096))
        all_items += items
        fb.append(len(all_items))
    # the pool: the three data sections written back to back by the device encoder
    dk, dv, dvoff, ddel = dev_run(torch, seb, all_items, "fixed16")
    ws = torch.zeros(seb.dev_sst_workspace_size(len(all_items), 3), dtype=torch.uint8, device="cuda")
    sizes = seb.dev_sst_plan(dk, dvoff, fb, ws)
    assert [s[0] for s in sizes] == [f["blocks"] for f in files]
    nblocks = sum(s[0] for s in sizes)
    pool = torch.full((nblocks * 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    blen = torch.zeros(nblocks, dtype=torch.int16, device="cuda")
    index = torch.zeros(sum(s[2] for s in sizes), dtype=torch.uint8, device="cuda")
    meta = torch.zeros(sum(s[3] for s in sizes), dtype=torch.uint8, device="cuda")
    seb.dev_sst_encode(dk, dv, dvoff, ddel, fb, sizes, ws, pool, index, meta, blen=blen)
    first_block = {100 + f: sum(s[0] for s in sizes[:f]) for f in range(3)}
    probes = [kg.key16_bytes(int(i)) for i in rng.integers(0, 9100, 3000)]
    hk = np.frombuffer(b"".join(probes), np.uint8).reshape(-1, 16)
    n = len(probes)
    pf, pb = reg.multiget_blocks(seb.as_keys(hk))
    cap = pf.shape[1]
    # the read list names (file, offset) pairs; the pool holds file f's block at first_block[f] + offset / 4096
    bid = np.full(pf.shape, seb.NO_BLOCK_ID, np.uint32)
    has = pb != NO_BLOCK
    bid[has] = [first_block[int(f)] + int(o) // 4096 for f, o in zip(pf[has], pb[has])]
    _, uf, ub = seb.blocks_dedup(pf, pb)
    assert len(uf) > 100
    dprobe = seb.dev_keys(torch.from_numpy(hk.reshape(-1).copy()).cuda(), n=n, stride=16)
    dbid = torch.from_numpy(bid.view(np.int32).reshape(-1)).cuda()
    cells = torch.zeros(n * cap, dtype=torch.int32, device="cuda")
    seb.dev_search_blocks(dprobe, dbid, cap, pool, blen, cells)
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    vloc = torch.zeros(n, dtype=torch.int64, device="cuda")
    vlen = torch.zeros(n, dtype=torch.int32, device="cuda")
    seb.dev_resolve_rows(cells, dbid, n, cap, status, None, vloc, vlen)
    torch.cuda.synchronize()
    flat = pool.cpu().numpy()
    st, loc, ln = status.cpu().numpy(), vloc.cpu().numpy(), vlen.cpu().numpy()
    found = under_tomb = 0
    for i, p in enumerate(probes):
        # LSM.Get over the L0 files in the registry's visiting order (insertion order): the first file that holds
        # a live entry answers; a tombstone is "not found" in that file and the walk goes on (block_ref.lsm_get_ref)
        walk = [f["items"].get(p) for f in files]
        ref_cells = [br.cell(br.NONE) if e is None else br.cell(br.TOMBSTONE) if e[1] else br.cell(br.FOUND, 0, len(e[0]))
                     for e in walk]
        want_st, col, _ = br.lsm_get_ref(ref_cells)
        assert st[i] == want_st, (i, p)
        if want_st == br.GET_FOUND:
            assert flat[int(loc[i]):int(loc[i]) + int(ln[i])].tobytes() == walk[col][0], i
            found += 1
            under_tomb += any(c >> 28 == br.TOMBSTONE for c in ref_cells[:col])
    assert n // 4 < found < n and under_tomb > 20
    reg.close()
    ctx.close()


def test_binding_guards(seb, torch_cuda):
    """Short workspace, offsets and output tensors raise ValueError before any launch."""
    torch = torch_cuda
    rng = np.random.default_rng(1)
    items = small_items(rng, 500)
    dk, dv, dvoff, ddel = dev_run(torch, seb, items, "even")
    fb = [0, 500]
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8, device="cuda")  # noqa: E731
    need = seb.dev_sst_workspace_size(500, 1)
    assert need > 0
    with pytest.raises(ValueError):
        seb.dev_sst_plan(dk, dvoff, fb, u8(need - 1))
    with pytest.raises(ValueError):
        seb.dev_sst_plan(dk, dvoff[:-1], fb, u8(need))
    ws = u8(need)
    sizes = seb.dev_sst_plan(dk, dvoff, fb, ws)
    b, d, x, m, _ = sizes[0]
    for short in ("data", "index", "meta", "blen"):
        t = dict(data=u8(d), index=u8(x), meta=u8(m), blen=torch.zeros(b, dtype=torch.int16, device="cuda"))
        t[short] = t[short][:-1]
        with pytest.raises(ValueError):
            seb.dev_sst_encode(dk, dv, dvoff, ddel, fb, sizes, ws, t["data"], t["index"], t["meta"], blen=t["blen"])
    with pytest.raises(ValueError):
        seb.dev_sst_encode(dk, dv, dvoff, ddel, fb, sizes, ws, u8(d), u8(x), u8(m), blen=torch.zeros(b, dtype=torch.int32, device="cuda"))
    with pytest.raises(seb.SebError):  # file_begin must run from 0 to n
        seb.dev_sst_plan(dk, dvoff, [0, 499], ws)
    with pytest.raises(seb.SebError):  # a data section that is not 16-byte aligned
        seb.dev_sst_encode(dk, dv, dvoff, ddel, fb, sizes, ws, u8(d + 1)[1:], u8(x), u8(m))
    torch.cuda.synchronize()
