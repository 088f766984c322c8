"""GPU: the B-tree's range scans on the device (include/seb_bloom.h, "B-tree, range scans").

seb_dev_bt_dir_build writes the bytes of the host half's directory (itself held to btree_scan_ref's restatement in
test_btree_scan.py and run under ASan + UBSan in test_btree_scan_sanitize.py), whole, on every accepted case with the
image at leads 0, 1 and 3, and refuses every image the host half refuses with the same page.  seb_dev_bt_scan_plan,
seb_dev_bt_scan_cells and the two values gathers equal seb_bt_scan in every array: at R = 0, 1, 63, 65 and 257, with no
entries at all, with every output 0xA5-filled between guards, with grid_cap at 1 and 2 for every grid-stride kernel, on
a busy side stream with late inputs.  Widths: btree_ref's pages of 64, 65, 66 and 129 children (where the right
pointer changes lane and pass of the scatter), leaves of 300 cells, the chain of 31 rounds, and one bulk-loaded image
with one leaf more than a stretch of the tile scan covers (128 tiles of 64 pages, + 1), scanned by as many ranges, so
that the scan's carry is crossed in the directory build and in the plan.  BTreeImage.open -> scan_batch end to end.
The refused images are data errors answered by a status; nothing here provokes a fault."""
import struct

import numpy as np
import pytest

import btree_ref as bref
import btree_scan_ref as sref
import stream_late as sl

pytestmark = pytest.mark.gpu

CASES = bref.cases()
CORRUPT = bref.corrupt_cases()
ACCEPTED = sorted(n for n in CASES if sref.accepted(n))
TILE, STRETCH = 64, 128  # pages (ranges) per tile of the scans in seb_btscan.hip, tiles per stretch of scan_tile_sums
ENTRY = (("status", np.uint8), ("source", np.uint8), ("kloc", np.uint64), ("klen", np.uint32), ("vloc", np.uint64), ("vlen", np.uint32))
_HOST = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def host(seb, name, image=None):
    """The host half's answers for an image, computed once: meta, kind, level, and the directory or the refusal."""
    if name not in _HOST:
        image = CASES[name].image if image is None else image
        meta = seb.bt_open(image)
        kind, level, _ = seb.bt_check(image, meta)
        try:
            d, info = seb.bt_dir_build(image, meta, kind, level)
            err = None
        except seb.SebError as e:
            d, info, err = None, None, str(e)
        _HOST[name] = dict(image=image, meta=meta, kind=kind, level=level, dir=d, info=info, err=err)
    return _HOST[name]


def host_scan(seb, name, starts, ends, limit=0, tag=""):
    key = (name, "scan", tag, limit)
    if key not in _HOST:
        h = host(seb, name)
        _HOST[key] = seb.bt_scan(h["image"], h["meta"], h["dir"], starts, ends, limit)
    return _HOST[key]


def key_lists(keys):
    off = np.zeros(len(keys) + 1, np.uint64)
    np.cumsum([len(k) for k in keys], out=off[1:])
    data = np.frombuffer(b"".join(keys), np.uint8) if off[-1] else np.zeros(0, np.uint8)
    return data, off


def dev_keys_of(torch, seb, keys, lead=3):
    data, off = key_lists(keys)
    return seb.dev_keys(sl.lead_view(torch, np.concatenate([data, np.zeros(1, np.uint8)]), lead), sl.to_dev(torch, off))


class Dev:
    """An image on the device `lead` bytes into its allocation, checked; dir_build() builds into a guarded output."""

    def __init__(self, torch, seb, h, lead=0, stream=None):
        self.torch, self.seb, self.meta = torch, seb, h["meta"]
        self.nbytes = self.meta.num_pages * bref.PAGE
        self.image = sl.lead_view(torch, np.frombuffer(h["image"], np.uint8)[: self.nbytes], lead)
        n = self.meta.num_pages
        self.kind, self.level = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda"), torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")
        seb.dev_bt_check(self.image, self.nbytes, self.meta, self.kind, self.level)
        self.dir = sl.Out(torch, seb.bt_dir_bytes(n), np.uint8)
        self.ws = torch.empty(seb.dev_bt_dir_workspace_size(n), dtype=torch.uint8, device="cuda")

    def dir_build(self, stream=None):
        return self.seb.dev_bt_dir_build(self.image, self.nbytes, self.meta, self.kind, self.level, self.dir.t, self.ws, stream=stream)

    def scan(self, starts, ends, limit=0, stream=None, dk=None):
        """plan + cells + the two gathers: a dict of the arrays seb_bt_scan returns, read back through their guards."""
        torch, seb = self.torch, self.seb
        R = len(starts)
        ks, ke = dk if dk else (dev_keys_of(torch, seb, starts), dev_keys_of(torch, seb, ends, 5))
        rs = sl.Out(torch, R, np.uint8)
        ws = torch.empty(max(seb.dev_bt_scan_workspace_size(R), 8), dtype=torch.uint8, device="cuda")
        sz = seb.dev_bt_scan_plan(self.image, self.nbytes, self.meta, self.dir.t, ks, ke, limit, rs.t, ws, stream=stream)
        n = sz.entries
        ro = sl.Out(torch, R + 1, np.uint64)
        outs = {k: sl.Out(torch, n, t) for k, t in ENTRY}
        seb.dev_bt_scan_cells(self.image, self.nbytes, self.meta, self.dir.t, sz, ws, ro.t, *[outs[k].t for k, _ in ENTRY], stream=stream)
        got = dict(sizes=(sz.ranges, sz.entries))
        for name, loc, length in (("key", "kloc", "klen"), ("val", "vloc", "vlen")):
            off = sl.Out(torch, n + 1, np.uint64)
            if n:
                gws = torch.empty(seb.dev_get_values_workspace_size(n), dtype=torch.uint8, device="cuda")
                args = (outs["status"].t, outs["source"].t, None, outs[loc].t, outs[length].t, n, [], self.image)
                gsz = seb.dev_get_values_plan(*args, gws, pool_bytes=self.nbytes, stream=stream)
                dense = sl.Out(torch, gsz.val_bytes, np.uint8)
                seb.dev_get_values_emit(*args, gsz, gws, off.t, dense.t if gsz.val_bytes else None, pool_bytes=self.nbytes, stream=stream)
                torch.cuda.synchronize()
                got[name + "_off"], got[name + "s"] = off.get(name + "_off"), dense.get(name + "s")
            else:
                got[name + "_off"], got[name + "s"] = np.zeros(1, np.uint64), np.zeros(0, np.uint8)
        torch.cuda.synchronize()
        got.update(range_status=rs.get("range_status"), range_off=ro.get("range_off"))
        got.update({k: outs[k].get(k) for k, _ in ENTRY})
        return got


def same_scan(got, want, what):
    for k in sref.ARRAYS:
        sl.same(got[k], want[k], f"{what}: {k}")


def page_in(msg):
    return int(msg.split("page ")[1].split(":")[0])


# ------------------------------------------------------------------ the directory

@pytest.mark.parametrize("lead", [0, 1, 3])
@pytest.mark.parametrize("name", ACCEPTED)
def test_directory_bytes(seb, torch_cuda, name, lead):
    h = host(seb, name)
    dv = Dev(torch_cuda, seb, h, lead)
    info = dv.dir_build()
    assert info == h["info"], (name, info, h["info"])
    sl.same(dv.dir.get("dir"), h["dir"], f"{name} lead {lead}: dir")


def hand_edits(seb):
    """name -> image: a RightPtr swapped, the last leaf's non-zero, a leaf listed twice, the order broken, the root
    outside (the edits of test_btree_scan.py)."""
    case = CASES["f_depth3_fixed"]
    lv = [int(p) for p in sref.dir_arrays(host(seb, "f_depth3_fixed")["dir"], case.meta["num_pages"])[0]]
    out = {}

    def edit(name, fn):
        b = bytearray(case.image)
        fn(lambda p: bref.page_of(b, p), b)
        out[name] = bytes(b)
    edit("edit_chain_swapped", lambda pg, b: setattr(pg(lv[3]), "right_ptr", lv[6]))
    edit("edit_chain_last", lambda pg, b: setattr(pg(lv[-1]), "right_ptr", lv[0]))
    parent = bref.page_of(case.image, case.meta["root"]).right_ptr

    def repoint(pg, b):
        p = pg(parent)
        off = p.cell_offset(1)
        struct.pack_into(">I", p.d, off + bref.uvarint16(p.d, off)[1], p.cell_at(0, leaf=False).child)
    edit("edit_twice", repoint)

    def lower(pg, b):
        c = pg(lv[5]).cell_at(0)
        pg(lv[5]).d[c.koff: c.koff + len(c.key)] = b"\x01" * len(c.key)
    edit("edit_order", lower)
    edit("edit_root_outside", lambda pg, b: struct.pack_into(">I", b, 4, case.meta["num_pages"] + 3))
    return out


REFUSED = sorted(CORRUPT) + ["f_depth3_literal", "g_depth4_literal", "edit_chain_swapped", "edit_chain_last", "edit_twice", "edit_order",
                             "edit_root_outside"]


@pytest.mark.parametrize("name", REFUSED)
def test_refused_images(seb, torch_cuda, name):
    """Every image the host half refuses is refused on the device with the same page and the same words."""
    image = CORRUPT[name][0] if name in CORRUPT else CASES[name].image if name in CASES else hand_edits(seb)[name]
    h = host(seb, "refused:" + name, image)
    assert h["err"] is not None and "page " in h["err"], name
    dv = Dev(torch_cuda, seb, h, 1)
    with pytest.raises(seb.SebError) as e:
        dv.dir_build()
    assert e.value.code == -1 and page_in(str(e.value)) == page_in(h["err"]), (str(e.value), h["err"])
    assert str(e.value).split("page ")[1] == h["err"].split("page ")[1]
    assert not dv.dir.get("dir")[:32].any(), "a refused directory keeps a header"
    # and a scan against it is refused before anything is launched
    rs = torch_cuda.full((1,), 0x5A, dtype=torch_cuda.uint8, device="cuda")
    ws = torch_cuda.empty(seb.dev_bt_scan_workspace_size(1), dtype=torch_cuda.uint8, device="cuda")
    with pytest.raises(seb.SebError) as e:
        seb.dev_bt_scan_plan(dv.image, dv.nbytes, dv.meta, dv.dir.t, dev_keys_of(torch_cuda, seb, [b"a"]), dev_keys_of(torch_cuda, seb, [b""]),
                             0, rs, ws)
    assert e.value.code == -1 and "directory" in str(e.value) and int(rs.cpu()[0]) == 0x5A


# ------------------------------------------------------------------ the scan

@pytest.mark.parametrize("name", ACCEPTED)
def test_scan_equals_the_host_half(seb, torch_cuda, name):
    case, h = CASES[name], host(seb, name)
    starts, ends = sref.ranges(case, np.random.default_rng(3), h["dir"])
    want = host_scan(seb, name, starts, ends)
    dv = Dev(torch_cuda, seb, h, 1)
    dv.dir_build()
    got = dv.scan(starts, ends)
    same_scan(got, want, name)
    assert got["sizes"] == want["sizes"][:2]


@pytest.mark.parametrize("R", [0, 1, 63, 65, 257])
def test_batch_sizes_and_limits(seb, torch_cuda, R):
    case, h = CASES["f_depth3_fixed"], host(seb, "f_depth3_fixed")
    rng = np.random.default_rng(R)
    pick = rng.integers(0, len(case.keys), (R, 2))
    starts = [case.keys[min(a, b)] if i % 5 else b"" for i, (a, b) in enumerate(pick)]
    ends = [case.keys[max(a, b)] + (b"\0" if i % 2 else b"") if i % 7 else b"" for i, (a, b) in enumerate(pick)]
    dv = Dev(torch_cuda, seb, h)
    dv.dir_build()
    for limit in (0, 1, 3):
        want = host_scan(seb, "f_depth3_fixed", starts, ends, limit, tag=f"R{R}")
        same_scan(dv.scan(starts, ends, limit), want, f"R={R} limit={limit}")
    if R:  # the fixed-stride layout: the starts as keys of one length (every key of this case has the same)
        width = len(case.keys[0])
        fs = [s or case.keys[0] for s in starts]
        fixed = np.frombuffer(b"".join(fs), np.uint8).reshape(R, width)
        dk = (seb.dev_keys(sl.lead_view(torch_cuda, fixed.reshape(-1), 0), n=R, stride=width), dev_keys_of(torch_cuda, seb, ends))
        same_scan(dv.scan(fs, ends, 2, dk=dk), host_scan(seb, "f_depth3_fixed", fs, ends, 2, tag=f"R{R}fixed"), f"R={R} fixed stride")


def test_no_entries(seb, torch_cuda):
    case, h = CASES["e_root_split"], host(seb, "e_root_split")
    starts, ends = [b"zzz", case.keys[3], case.keys[9], b"\xff"], [b"", case.keys[3], case.keys[2], b"\0"]
    want = host_scan(seb, "e_root_split", starts, ends, tag="none")
    assert want["sizes"][1] == 0
    dv = Dev(torch_cuda, seb, h)
    dv.dir_build()
    same_scan(dv.scan(starts, ends), want, "no entries")
    e = host(seb, "a_empty")
    dv = Dev(torch_cuda, seb, e)
    assert dv.dir_build() == dict(leaves=1, keys=0, depth=1)
    same_scan(dv.scan([b"", b"a"], [b"", b"b"]), host_scan(seb, "a_empty", [b"", b"a"], [b"", b"b"], tag="none"), "empty tree")


def test_error_ranges(seb, torch_cuda):
    """A bound whose walk ends in ERROR: the directory of the good image, the image then damaged on the device exactly as
    on the host (a leaf's type byte): range_status says so, the other ranges are answered."""
    case, h = CASES["f_depth3_fixed"], host(seb, "f_depth3_fixed")
    lv = [int(p) for p in sref.dir_arrays(h["dir"], h["meta"].num_pages)[0]]
    b = bytearray(case.image)
    b[lv[1] * bref.PAGE] = 7
    hurt = dict(h, image=bytes(b))
    first_of = lambda p: bref.page_of(case.image, p).cell_at(0).key  # noqa: E731
    starts, ends = [b"", first_of(lv[1]), first_of(lv[0]), first_of(lv[2])], [first_of(lv[0]) + b"\0", b"", first_of(lv[1]), b""]
    want = seb.bt_scan(hurt["image"], h["meta"], h["dir"], starts, ends)
    assert list(want["range_status"]) == [0, bref.ERROR, bref.ERROR, 0] and want["sizes"][1] > 2
    dv = Dev(torch_cuda, seb, h)
    dv.dir_build()
    dv.image[lv[1] * bref.PAGE] = 7
    same_scan(dv.scan(starts, ends), want, "a damaged leaf")
    # entries through the damaged leaf no longer parse: ERROR entries with zero lengths, skipped by the gathers
    want = seb.bt_scan(hurt["image"], h["meta"], h["dir"], [b""], [b""])
    assert (want["status"] == bref.ERROR).sum() == bref.page_of(case.image, lv[1]).num_cells
    same_scan(dv.scan([b""], [b""]), want, "entries of a damaged leaf")


# ------------------------------------------------------------------ capped grids

def many_ranges(case, n, seed, span=3):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, len(case.keys) - span - 1, n)
    return [case.keys[i] for i in a], [case.keys[i + int(rng.integers(0, span + 1))] for i in a]


@pytest.mark.parametrize("name", ["k_wide_3level", "f_depth3_fixed"])
def test_under_a_grid_cap(seb, torch_cuda, name):
    """At most 1 and 2 workgroups per grid-stride launch: k_dir_count, k_dir_leaves and k_dir_verify take several trips
    over more than 256 leaves, k_dir_scatter's waves several pages, k_scan_plan / k_scan_offsets several trips over 1,300
    ranges and k_scan_cells over their entries; every byte equals the default grid's and the host half's."""
    case, h = CASES[name], host(seb, name)
    R = 1300
    starts, ends = many_ranges(case, R, 11)
    want = host_scan(seb, name, starts, ends, tag="cap")
    if name == "k_wide_3level":
        assert h["info"]["leaves"] > 256 and h["info"]["leaves"] % 256 and want["sizes"][1] > 2 * 256 * 2
    runs = {}
    for cap in sl.CAPS:
        dv = Dev(torch_cuda, seb, h, 1)
        with sl.grid_cap(seb, cap):
            assert dv.dir_build() == h["info"]
            got = dv.scan(starts, ends)
        sl.same(dv.dir.get("dir"), h["dir"], f"{name} cap {cap}: dir")
        same_scan(got, want, f"{name} cap {cap}")
        runs[cap] = [got[k].tobytes() for k in sref.ARRAYS]
    assert runs[1] == runs[None] and runs[2] == runs[None]


# ------------------------------------------------------------------ across the scan's carry

@pytest.fixture(scope="module")
def carry_image():
    """Leaves of 2 cells, one leaf more than a stretch of the tile scan covers."""
    leaves = STRETCH * TILE + 1
    keys = [int(i).to_bytes(3, "big") for i in range(7, 7 + 5 * 2 * leaves, 5)]
    image = bref.bulk_load(keys, [k[1:] for k in keys], leaf_cells=2, fanout=32)
    return image, keys, leaves


def test_across_the_carry(seb, torch_cuda, carry_image):
    image, keys, leaves = carry_image
    h = host(seb, "carry", image)
    assert h["info"]["leaves"] == leaves == STRETCH * TILE + 1 and h["info"]["keys"] == 2 * leaves
    dv = Dev(torch_cuda, seb, h)
    assert dv.dir_build() == h["info"]
    sl.same(dv.dir.get("dir"), h["dir"], "carry: dir")
    first = sref.dir_arrays(h["dir"], h["meta"].num_pages)[1]
    assert int(first[STRETCH * TILE]) == 2 * STRETCH * TILE  # the entry behind the carry
    # as many ranges, a few entries each: range_off crosses the carry in the plan; the last ranges lie behind it
    R = STRETCH * TILE + 1
    at = np.linspace(0, len(keys) - 4, R).astype(np.int64)
    starts, ends = [keys[i] for i in at], [keys[i + 1 + (j % 3)] for j, i in enumerate(at)]
    want = seb.bt_scan(image, h["meta"], h["dir"], starts, ends)
    assert want["sizes"][1] > R and int(want["range_off"][STRETCH * TILE]) > 0
    same_scan(dv.scan(starts, ends), want, "carry: scan")


# ------------------------------------------------------------------ a busy side stream, late inputs

@pytest.fixture(scope="module")
def rig(seb, torch_cuda):
    try:
        r = sl.Rig(torch_cuda, seb)
    except AssertionError as e:
        pytest.fail(f"stream control: {e}")
    return r


def test_on_a_busy_side_stream(seb, torch_cuda, rig):
    """The image arrives late before the directory build; the bounds late before the plan; the cells and the gathers
    follow on the busy stream."""
    torch = torch_cuda
    case, other = CASES["f_depth3_fixed"], CASES["e_root_split"]
    h = host(seb, "f_depth3_fixed")
    meta, n = h["meta"], h["meta"].num_pages
    nbytes = n * bref.PAGE
    good = np.frombuffer(case.image, np.uint8)[:nbytes]
    poison = np.zeros(nbytes, np.uint8)
    src = np.frombuffer(other.image, np.uint8)
    poison[: min(nbytes, src.size)] = src[: min(nbytes, src.size)]  # another tree's pages: a valid image, another directory
    starts, ends = many_ranges(case, 300, 5, span=6)
    sdata, soff = key_lists(starts)
    edata, eoff = key_lists(ends)
    want = host_scan(seb, "f_depth3_fixed", starts, ends, tag="late")
    sl.differ([want["range_off"]], [seb.bt_scan(case.image, meta, h["dir"], (sdata[::-1].copy(), soff), (edata, eoff))["range_off"]])
    L = rig.session()
    d_image = L.inp(good, poison)
    L.arm()
    kind, level = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    L.plan(seb.dev_bt_check, d_image, nbytes, meta, kind, level)
    d_dir = L.out(seb.bt_dir_bytes(n), np.uint8)
    ws = torch.empty(seb.dev_bt_dir_workspace_size(n), dtype=torch.uint8, device="cuda")
    info = seb.dev_bt_dir_build(d_image, nbytes, meta, kind, level, d_dir.t, ws, stream=L.S)
    assert info == h["info"]
    sl.same(d_dir.get("dir"), h["dir"], "late: dir")
    R = len(starts)
    d_s = L.inp(np.concatenate([sdata, np.zeros(1, np.uint8)]), np.concatenate([sdata[::-1], np.zeros(1, np.uint8)]))
    ks, ke = seb.dev_keys(d_s, sl.to_dev(torch, soff)), seb.dev_keys(sl.to_dev(torch, np.concatenate([edata, np.zeros(1, np.uint8)])), sl.to_dev(torch, eoff))
    rs = L.out(R, np.uint8)
    sws = torch.empty(seb.dev_bt_scan_workspace_size(R), dtype=torch.uint8, device="cuda")
    L.arm()
    sz = L.plan(seb.dev_bt_scan_plan, d_image, nbytes, meta, d_dir.t, ks, ke, 0, rs.t, sws)
    assert sz.entries == want["sizes"][1]
    ro = L.out(R + 1, np.uint64)
    outs = {k: L.out(sz.entries, t) for k, t in ENTRY}
    L.arm()
    L.call(seb.dev_bt_scan_cells, d_image, nbytes, meta, d_dir.t, sz, sws, ro.t, *[outs[k].t for k, _ in ENTRY])
    L.finish()
    sl.same(rs.get("range_status"), want["range_status"], "late: range_status")
    sl.same(ro.get("range_off"), want["range_off"], "late: range_off")
    for k, _ in ENTRY:
        sl.same(outs[k].get(k), want[k], f"late: {k}")


# ------------------------------------------------------------------ refusals of the entry points

def test_entry_point_refusals(seb, torch_cuda):
    torch, h = torch_cuda, host(seb, "e_root_split")
    dv = Dev(torch, seb, h)
    meta, n = dv.meta, dv.meta.num_pages
    small = torch.empty(16, dtype=torch.uint8, device="cuda")

    def refused(fn, *a, words=None, code=-1, **kw):
        with pytest.raises(seb.SebError) as e:
            fn(*a, **kw)
        assert e.value.code == code and (not words or words in str(e.value)), e.value

    refused(seb.dev_bt_dir_build, dv.image, dv.nbytes, meta, dv.kind, dv.level, dv.dir.t, small, words="workspace")
    refused(seb.dev_bt_dir_build, dv.image, dv.nbytes, meta, None, dv.level, dv.dir.t, dv.ws, words="null")
    refused(seb.dev_bt_dir_build, dv.image, dv.nbytes - 1, meta, dv.kind, dv.level, dv.dir.t, dv.ws, words="do not fit")
    refused(seb.dev_bt_dir_build, dv.image, dv.nbytes, meta, dv.kind, dv.level, dv.dir.buf[sl.GUARD + 4:], dv.ws, ws_bytes=1 << 30,
            words="aligned")
    assert (dv.dir.get("dir") == sl.FILL).all(), "a refused call wrote the directory"
    dv.dir_build()
    ks, ke = dev_keys_of(torch, seb, [b"a", b"b"]), dev_keys_of(torch, seb, [b""])
    rs = torch.full((2,), 0x5A, dtype=torch.uint8, device="cuda")
    ws = torch.empty(seb.dev_bt_scan_workspace_size(2), dtype=torch.uint8, device="cuda")
    refused(seb.dev_bt_scan_plan, dv.image, dv.nbytes, meta, dv.dir.t, ks, ke, 0, rs, ws, words="starts")
    ke = dev_keys_of(torch, seb, [b"", b""])
    refused(seb.dev_bt_scan_plan, dv.image, dv.nbytes, meta, dv.dir.t, ks, ke, 0, rs, small, words="workspace")
    refused(seb.dev_bt_scan_plan, dv.image, dv.nbytes, meta, None, ks, ke, 0, rs, ws, words="null")
    torch.cuda.synchronize()
    assert (rs.cpu().numpy() == 0x5A).all()
    # another plan's workspace: the cells write nothing
    sz = seb.dev_bt_scan_plan(dv.image, dv.nbytes, meta, dv.dir.t, ks, ke, 0, rs, ws)
    assert sz.entries > 0
    lie = seb.seb_bt_scan_sizes(sz.ranges, sz.entries + 1, 0, 0)
    ro = sl.Out(torch, 3, np.uint64)
    outs = [sl.Out(torch, sz.entries + 1, t) for _, t in ENTRY]
    seb.dev_bt_scan_cells(dv.image, dv.nbytes, meta, dv.dir.t, lie, ws, ro.t, *[o.t for o in outs])
    torch.cuda.synchronize()
    assert (ro.get().view(np.uint8) == sl.FILL).all() and all((o.get().view(np.uint8) == sl.FILL).all() for o in outs)


# ------------------------------------------------------------------ end to end

@pytest.mark.parametrize("name", ["a_empty", "c_lengths", "g_depth4_fixed", "h_updates_deletes", "i_v1_mixed"])
def test_end_to_end(seb, torch_cuda, name):
    """BTreeImage.open -> scan_batch against the restatement's scan by directory, entry for entry."""
    case, h = CASES[name], host(seb, name)
    starts, ends = sref.ranges(case, np.random.default_rng(21), h["dir"], cap=8)
    want = sref.scan_by_dir(case.image, case.meta, sref.build_dir(case.image, case.meta, *bref.check(case.image, case.meta)[:2])[0], starts, ends, 5)
    bt = seb.BTreeImage()
    try:
        bt.open(case.image)
        assert bt.dir is not None and bt.dir_error is None and bt.dir_info == h["info"]
        rs, ro, ko, kb, vo, vb = bt.scan_batch(starts, ends, limit=5)
        for got, k in ((rs, "range_status"), (ro, "range_off"), (ko, "key_off"), (kb, "keys"), (vo, "val_off"), (vb, "vals")):
            sl.same(got, want[k], f"{name}: {k}")
        assert bt.scan_batch([], [])[1].tolist() == [0]
        if case.puts:
            got = sref.pairs_of(dict(range_off=ro, key_off=ko, keys=kb, val_off=vo, vals=vb), 0)
            assert starts[0] == b"" and ends[0] == b"" and got == sorted(case.puts.items())[:5]
    finally:
        bt.close()


def test_open_keeps_working_without_a_directory(seb, torch_cuda):
    case = CASES["g_depth4_literal"]
    bt = seb.BTreeImage()
    try:
        bt.open(case.image)
        assert bt.dir is None and "page " in bt.dir_error and "chain" in bt.dir_error
        keys = bref.probes(case, np.random.default_rng(15))
        status, off, vals = bt.get_batch(keys)
        want = bref.get_batch(case.image, case.meta, keys)
        assert np.array_equal(status, want[0]) and (status == bref.FOUND).any()
        with pytest.raises(seb.SebError) as e:
            bt.scan_batch([b""], [b""])
        assert "page " in str(e.value)
    finally:
        bt.close()
