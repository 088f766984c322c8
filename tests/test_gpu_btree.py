"""GPU: the B-tree's read side on the device (include/seb_bloom.h, "B-tree, read side").

seb_dev_bt_check and seb_dev_bt_get equal the host half (seb_bt_check, seb_bt_get, themselves held to btree_ref's
restatement in test_btree.py and run under ASan + UBSan on the same bytes in test_btree_sanitize.py) in kind, level,
the counts and (status, leaf, pos, vloc, vlen, source): on every shared case and every corrupt image, with the image
at leads 0, 1 and 3 into its allocation, at batch sizes 0, 1, 63, 65 and 257, in the offsets layout and the fixed-
stride one.  One bulk-loaded image of about 100,000 16-byte keys at depth 4 takes 300,000 probes, half of them
absent.  btree_ref's wide images (leaves of 300 cells, internal pages of 63, 64, 65, 128, 129 and 133) take a wave's
lanes through several trips over a directory, its chains reach the depth limit from both sides, and three edited
images hold leaves at two levels.  With the option grid_cap at 1 and 2 the grid-stride loops of all four kernels take
several trips, the last one partial, and every output equals the default grid's byte for byte.  Batch keys of 65,535,
65,536 and 65,537 bytes.  Every output starts as 0xA5 between 64 guard bytes.  The entry points' refusals, one case on a busy side
stream with late inputs, and load -> get_batch -> values end to end against the reference, byte for byte.  The
corrupt images are data errors that the kernels answer with a status through the bounds rules the header states;
nothing here provokes a fault."""
import numpy as np
import pytest

import btree_ref as bref
import stream_late as sl

pytestmark = pytest.mark.gpu

CASES = bref.cases()
CORRUPT = bref.corrupt_cases()
COLS = ("status", "leaf", "pos", "vloc", "vlen")
TYPES = (np.uint8, np.uint32, np.uint32, np.uint64, np.uint32, np.uint8)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def lead_view(torch, a, lead):
    """The bytes of `a` on the device, `lead` bytes into an aligned allocation that ends with them."""
    a = np.frombuffer(a, np.uint8) if isinstance(a, bytes) else np.asarray(a, np.uint8).reshape(-1)
    buf = torch.from_numpy(np.concatenate([np.full(lead, 0xEE, np.uint8), a])).cuda()
    return buf[lead: lead + a.size]


def key_lists(keys):
    off = np.zeros(len(keys) + 1, np.uint64)
    np.cumsum([len(k) for k in keys], out=off[1:])
    data = np.frombuffer(b"".join(keys), np.uint8) if off[-1] else np.zeros(0, np.uint8)
    return data, off


def dev_keys_of(torch, seb, keys, lead=3):
    data, off = key_lists(keys)
    return seb.dev_keys(lead_view(torch, np.concatenate([data, np.zeros(1, np.uint8)]), lead), sl.to_dev(torch, off))


def dev_check(torch, seb, d_image, nbytes, meta, stream=None):
    kind, level = sl.Out(torch, meta.num_pages, np.uint8), sl.Out(torch, meta.num_pages, np.uint8)
    stats = seb.dev_bt_check(d_image, nbytes, meta, kind.t, level.t, stream=stream)
    return kind, level, stats


def dev_get(torch, seb, d_image, nbytes, meta, dk, n, stream=None):
    outs = [sl.Out(torch, n, t) for t in TYPES]
    seb.dev_bt_get(d_image, nbytes, meta, dk, *[o.t for o in outs], stream=stream)
    return outs


def same_get(outs, want, what):
    for name, o, w in zip(COLS, outs, want):
        sl.same(o.get(name), w, f"{what}: {name}")
    sl.same(outs[5].get("source"), (want[0] == bref.FOUND).astype(np.uint8), f"{what}: source")


def check_and_get(torch, seb, image, keys, what, lead):
    meta = seb.bt_open(image)
    nbytes = meta.num_pages * bref.PAGE
    d_image = lead_view(torch, image[:nbytes], lead)
    kind, level, stats = dev_check(torch, seb, d_image, nbytes, meta)
    w_kind, w_level, w_stats = seb.bt_check(image, meta)
    sl.same(kind.get("kind"), w_kind, f"{what}: kind")
    sl.same(level.get("level"), w_level, f"{what}: level")
    assert stats == w_stats, (what, stats, w_stats)
    want = seb.bt_get(image, meta, keys)
    outs = dev_get(torch, seb, d_image, nbytes, meta, dev_keys_of(torch, seb, keys), len(keys))
    torch.cuda.synchronize()
    same_get(outs, want, what)
    return want


# ------------------------------------------------------------------ the shared cases, the corrupt images

@pytest.mark.parametrize("lead", [0, 1, 3])
@pytest.mark.parametrize("name", sorted(CASES))
def test_cases(seb, torch_cuda, name, lead):
    case = CASES[name]
    want = check_and_get(torch_cuda, seb, case.image, bref.probes(case, np.random.default_rng(5)), name, lead)
    if case.keys:
        assert (want[0] == bref.FOUND).any() and (want[0] == bref.MISS).any()


@pytest.mark.parametrize("name", sorted(CORRUPT))
def test_corrupt_images(seb, torch_cuda, name):
    """Data errors answered by a status, through the bounds rules that the sanitizer run exercised on these bytes."""
    image, keys = CORRUPT[name]
    want = check_and_get(torch_cuda, seb, image, keys, name, 1)
    claim = bref.corrupt_claims()[name]
    if claim["errors"]:
        assert (want[0] == bref.ERROR).sum() > 1, name
    else:
        assert (want[0] == bref.FOUND).any() and (want[0] == bref.MISS).any(), name
    # what the image was made for, stated on the host half's answer that the device just equalled
    meta = seb.bt_open(image)
    w_kind, w_level, w_stats = seb.bt_check(image, meta)
    if "bad" in claim:
        assert list(np.nonzero(w_kind == bref.BAD)[0]) == [0] + sorted(claim["bad"]), name
    assert all(w_stats[k] == v for k, v in claim.get("stats", {}).items()), (name, w_stats)
    assert all(w_level[p] == lv for p, lv in claim.get("level", {}).items()), name


def test_long_batch_keys(seb, torch_cuda):
    """Batch keys of 65,535, 65,536 and 65,537 bytes and more: the compare looks at the first 65,536."""
    torch, case = torch_cuda, CASES["e_root_split"]
    meta = seb.bt_open(case.image)
    nbytes = meta.num_pages * bref.PAGE
    keys = bref.long_keys(case)
    assert sorted(len(k) for k in keys)[1:4] == [65535, 65536, 65537]
    want = seb.bt_get(case.image, meta, keys)
    assert list(want[0]) == [bref.MISS] * 2 + [bref.FOUND] + [bref.MISS] * 3
    d_image = lead_view(torch, case.image, 0)
    for lead in (0, 3):
        outs = dev_get(torch, seb, d_image, nbytes, meta, dev_keys_of(torch, seb, keys, lead), len(keys))
        torch.cuda.synchronize()
        same_get(outs, want, f"long keys, lead {lead}")


# ------------------------------------------------------------------ capped grids: the grid-stride loops iterate

def padded_probes(case, n, seed):
    """n probe keys of a case: probes(), then present keys over again."""
    keys = bref.probes(case, np.random.default_rng(seed))
    return (keys + case.keys * (n // max(len(case.keys), 1) + 1))[:n]


@pytest.mark.parametrize("name", ["f_depth3_fixed", "k_wide_3level", "two_parents"])
def test_check_under_a_grid_cap(seb, torch_cuda, name):
    """seb_dev_bt_check with at most 1 and 2 workgroups: a wave takes many pages in turn (k_bt_check, k_bt_level), on
    the wide image its lanes many cells in turn as well, and k_bt_stats's lanes several pages.  Kind, level and every
    count equal the host half's and the default grid's."""
    torch = torch_cuda
    image = CASES[name].image if name in CASES else CORRUPT[name][0]
    meta = seb.bt_open(image)
    np_ = meta.num_pages
    # cap 2 = 8 waves: more than two trips of the page loop, the last one partial
    assert np_ > 16 and np_ % 8 != 0 and np_ % 4 != 0, np_
    if name == "k_wide_3level":  # k_bt_stats, a lane per page: a second, partial trip at cap 1
        assert 256 < np_ < 512 and bref.widths(image)[1].count(129) >= 3
    nbytes = np_ * bref.PAGE
    d_image = lead_view(torch, image, 1)
    w_kind, w_level, w_stats = seb.bt_check(image, meta)
    runs = {}
    for cap in sl.CAPS:
        with sl.grid_cap(seb, cap):
            kind, level, stats = dev_check(torch, seb, d_image, nbytes, meta)
        runs[cap] = (kind.get("kind"), level.get("level"), stats)
        sl.same(runs[cap][0], w_kind, f"{name} cap {cap}: kind")
        sl.same(runs[cap][1], w_level, f"{name} cap {cap}: level")
        assert stats == w_stats, (name, cap, stats, w_stats)
    for cap in (1, 2):
        assert runs[cap][0].tobytes() == runs[None][0].tobytes() and runs[cap][1].tobytes() == runs[None][1].tobytes()
        assert runs[cap][2] == runs[None][2]


def test_large_check_under_a_grid_cap(seb, torch_cuda, big):
    """k_bt_stats's lane-per-page loop and its per-wave atomics over several trips: the large image's check."""
    torch = torch_cuda
    image = big[0]
    meta = seb.bt_open(image)
    np_ = meta.num_pages
    assert np_ > 2 * 256 * 2 and np_ % 512 != 0 and np_ % 256 != 0, np_  # a lane per page: the last trip partial
    nbytes = np_ * bref.PAGE
    d_image = lead_view(torch, image, 0)
    w_kind, w_level, w_stats = seb.bt_check(image, meta)
    for cap in (1, 2):
        with sl.grid_cap(seb, cap):
            kind, level, stats = dev_check(torch, seb, d_image, nbytes, meta)
        sl.same(kind.get("kind"), w_kind, f"cap {cap}: kind")
        sl.same(level.get("level"), w_level, f"cap {cap}: level")
        assert stats == w_stats, (cap, stats, w_stats)


@pytest.mark.parametrize("layout", ["offsets", "stride16"])
def test_get_under_a_grid_cap(seb, torch_cuda, big, layout):
    """seb_dev_bt_get with at most 1 and 2 workgroups: a lane takes several keys in turn, the last trip partial."""
    torch = torch_cuda
    n = 1300
    assert 2 * 256 * 2 < n < 2 * 256 * 3
    if layout == "offsets":
        case = CASES["k_wide_3level"]
        image, keys = case.image, padded_probes(case, n, 31)
        make = lambda: dev_keys_of(torch, seb, keys)  # noqa: E731
    else:
        image, keys = big[0], np.ascontiguousarray(big[2][:n])
        make = lambda: seb.dev_keys(lead_view(torch, np.concatenate([keys.reshape(-1), np.zeros(1, np.uint8)]), 7), n=n, stride=16)  # noqa: E731
    assert len(keys) == n
    meta = seb.bt_open(image)
    nbytes = meta.num_pages * bref.PAGE
    d_image = lead_view(torch, image, 0)
    want = seb.bt_get(image, meta, keys)
    assert (want[0] == bref.FOUND).sum() > 100 and (want[0] == bref.MISS).sum() > 100
    assert (want[0][1024:] == bref.FOUND).any()  # the third trip answers something that 0xA5 is not
    runs = {}
    for cap in sl.CAPS:
        with sl.grid_cap(seb, cap):
            outs = dev_get(torch, seb, d_image, nbytes, meta, make(), n)
            torch.cuda.synchronize()
        same_get(outs, want, f"{layout} cap {cap}")
        runs[cap] = [o.get().tobytes() for o in outs]
    assert runs[1] == runs[None] and runs[2] == runs[None]


@pytest.mark.parametrize("n", [0, 1, 63, 65, 257])
def test_batch_sizes(seb, torch_cuda, n):
    """Batches around a wave and a workgroup, in the offsets layout and in the fixed-stride one (8-byte keys)."""
    torch, case = torch_cuda, CASES["e_root_split"]
    meta = seb.bt_open(case.image)
    nbytes = meta.num_pages * bref.PAGE
    d_image = lead_view(torch, case.image, 0)
    rng = np.random.default_rng(n)
    keys = [case.keys[i] if j % 3 else b"key-9%03d" % j for j, i in enumerate(rng.integers(0, len(case.keys), n))]
    want = seb.bt_get(case.image, meta, keys)
    outs = dev_get(torch, seb, d_image, nbytes, meta, dev_keys_of(torch, seb, keys), n)
    torch.cuda.synchronize()
    same_get(outs, want, f"offsets n={n}")
    fixed = np.frombuffer(b"".join(keys), np.uint8).reshape(n, 8)
    for lead in (0, 5):
        dk = seb.dev_keys(lead_view(torch, np.concatenate([fixed.reshape(-1), np.zeros(1, np.uint8)]), lead), n=n, stride=8)
        outs = dev_get(torch, seb, d_image, nbytes, meta, dk, n)
        torch.cuda.synchronize()
        same_get(outs, want, f"stride 8 n={n} lead={lead}")


# ------------------------------------------------------------------ one large image

@pytest.fixture(scope="module")
def big():
    """About 100,000 16-byte keys (half of them under one 12-byte prefix) bulk-loaded at depth 4, and 300,000 probes,
    half of them absent."""
    rng = np.random.default_rng(77)
    rows = rng.integers(0, 256, (100_000, 16), dtype=np.uint8)
    rows[:50_000, :12] = np.frombuffer(b"shared-pref-", np.uint8)
    rows = np.unique(rows, axis=0)
    keys = [r.tobytes() for r in rows]
    image = bref.bulk_load(keys, [k[:3] + b"-val" for k in keys], leaf_cells=64, fanout=32)
    probe = rows[rng.integers(0, len(rows), 300_000)].copy()
    probe[150_000:, 15] ^= 0x41
    return image, len(keys), probe[rng.permutation(300_000)]


def test_large_image(seb, torch_cuda, big):
    torch = torch_cuda
    image, nkeys, probe = big
    meta = seb.bt_open(image)
    nbytes = meta.num_pages * bref.PAGE
    d_image = lead_view(torch, image, 0)
    kind, level, stats = dev_check(torch, seb, d_image, nbytes, meta)
    w_kind, w_level, w_stats = seb.bt_check(image, meta)
    sl.same(kind.get("kind"), w_kind, "kind")
    sl.same(level.get("level"), w_level, "level")
    assert stats == w_stats and stats["keys"] == nkeys and stats["depth"] >= 3 and stats["bad"] == 0 and stats["uniform"] == 1
    want = seb.bt_get(image, meta, probe)
    found = int((want[0] == bref.FOUND).sum())
    assert 140_000 < found < 160_000 and not (want[0] == bref.ERROR).any()
    for lead in (0, 7):  # the aligned 16-byte key load, and the bytewise one
        dk = seb.dev_keys(lead_view(torch, np.concatenate([probe.reshape(-1), np.zeros(1, np.uint8)]), lead), n=len(probe), stride=16)
        outs = dev_get(torch, seb, d_image, nbytes, meta, dk, len(probe))
        torch.cuda.synchronize()
        same_get(outs, want, f"lead {lead}")


# ------------------------------------------------------------------ refusals

def test_refusals(seb, torch_cuda):
    torch, case = torch_cuda, CASES["e_root_split"]
    meta = seb.bt_open(case.image)
    nbytes = meta.num_pages * bref.PAGE
    d_image = lead_view(torch, case.image, 0)
    dk = dev_keys_of(torch, seb, [b"key-0001", b"nope"])
    st = torch.full((2,), 0x5A, dtype=torch.uint8, device="cuda")
    u64 = torch.zeros(4, dtype=torch.int64, device="cuda")
    u32 = torch.zeros(4, dtype=torch.int32, device="cuda")
    odd8, odd4 = u64.view(torch.uint8)[4:], u32.view(torch.uint8)[2:]
    kind = torch.full((meta.num_pages,), 0x5A, dtype=torch.uint8, device="cuda")

    def refused(fn, *a, words=None, **kw):
        with pytest.raises(seb.SebError) as e:
            fn(*a, **kw)
        assert e.value.code == -1, e.value
        if words:
            assert words in str(e.value), e.value

    refused(seb.dev_bt_check, None, nbytes, meta, kind, words="null image")
    refused(seb.dev_bt_check, d_image, nbytes - 1, meta, kind, words="do not fit")
    refused(seb.dev_bt_get, None, nbytes, meta, dk, st, words="null image")
    refused(seb.dev_bt_get, d_image, nbytes - 4096, meta, dk, st, words="do not fit")
    refused(seb.dev_bt_get, d_image, nbytes, meta, dk, None, words="status")
    refused(seb.dev_bt_get, d_image, nbytes, meta, dk, st, odd4, words="aligned")
    refused(seb.dev_bt_get, d_image, nbytes, meta, dk, st, None, odd4, words="aligned")
    refused(seb.dev_bt_get, d_image, nbytes, meta, dk, st, None, None, odd8, words="aligned")
    refused(seb.dev_bt_get, d_image, nbytes, meta, dk, st, None, None, None, odd4, words="aligned")
    bad_keys = seb.dev_keys(dk._keep[0], dk._keep[1].view(torch.uint8)[4:])
    bad_keys.n = 1
    refused(seb.dev_bt_get, d_image, nbytes, meta, bad_keys, st, words="aligned")
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0x5A).all() and (kind.cpu().numpy() == 0x5A).all(), "a refused call wrote an output"
    ctx = seb.Ctx(0)
    try:
        room = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        with pytest.raises(seb.SebError) as e:
            ctx.bt_load(case.image[:100], room)
        assert e.value.code == -1
        with pytest.raises(seb.SebError) as e:
            ctx.bt_load(case.image, room, cap=nbytes - 1)
        assert e.value.code == -4 and "cap" in str(e.value)
        assert (room.cpu().numpy() == 0).all(), "a refused load uploaded"
    finally:
        ctx.close()
    # nothing to do is no refusal; every output but status is nullable
    seb.dev_bt_get(d_image, nbytes, meta, seb.dev_keys(dk._keep[0], n=0, stride=4), None)
    seb.dev_bt_get(d_image, nbytes, meta, dk, st)
    assert seb.dev_bt_check(d_image, nbytes, meta) == seb.bt_check(case.image, meta)[2]
    torch.cuda.synchronize()
    assert list(st.cpu().numpy()) == [bref.FOUND, bref.MISS]


# ------------------------------------------------------------------ a busy side stream, late inputs

@pytest.fixture(scope="module")
def rig(seb, torch_cuda):
    try:
        r = sl.Rig(torch_cuda, seb)
    except AssertionError as e:
        pytest.fail(f"stream control: {e}")
    return r


def test_on_a_busy_side_stream(seb, torch_cuda, rig):
    """The image arrives late before the check; the keys late before the Get."""
    torch = torch_cuda
    case, other = CASES["f_depth3_fixed"], CASES["f_depth3_literal"]
    meta = seb.bt_open(case.image)
    assert seb.bt_open(other.image).as_dict() == meta.as_dict()  # the poison: the literal build of the same Puts
    good, poison = np.frombuffer(case.image, np.uint8), np.frombuffer(other.image, np.uint8)
    nbytes = meta.num_pages * bref.PAGE
    keys = bref.probes(case, np.random.default_rng(8))
    poison_keys = [k[::-1] if len(k) > 1 else k for k in keys]
    kdata, koff = key_lists(keys)
    pdata, _ = key_lists(poison_keys)
    w_kind, w_level, w_stats = seb.bt_check(case.image, meta)
    want = seb.bt_get(case.image, meta, (kdata, koff))
    sl.differ([w_stats["reach_leaves"]], [seb.bt_check(other.image, meta)[2]["reach_leaves"]], ["stats"])
    sl.differ(want, seb.bt_get(case.image, meta, (pdata, koff)))
    sl.differ(want, seb.bt_get(other.image, meta, (kdata, koff)))
    L = rig.session()
    d_image = L.inp(good, poison)
    kind, level = L.out(meta.num_pages, np.uint8), L.out(meta.num_pages, np.uint8)
    L.arm()
    stats = L.plan(seb.dev_bt_check, d_image, nbytes, meta, kind.t, level.t)
    assert stats == w_stats
    sl.same(kind.get("kind"), w_kind, "kind")
    sl.same(level.get("level"), w_level, "level")
    d_kdata = L.inp(kdata, pdata)
    dk = seb.dev_keys(d_kdata, sl.to_dev(torch, koff))
    outs = [L.out(len(keys), t) for t in TYPES]
    L.arm()
    L.call(seb.dev_bt_get, d_image, nbytes, meta, dk, *[o.t for o in outs])
    L.finish()
    same_get(outs, want, "late")


# ------------------------------------------------------------------ end to end

@pytest.mark.parametrize("name", ["a_empty", "c_lengths", "g_depth4_fixed", "h_updates_deletes", "i_v1_mixed"])
def test_end_to_end(seb, torch_cuda, name):
    """BTreeImage.open -> get_batch (Get, then the values gather over the image) against the reference's walk."""
    case = CASES[name]
    bt = seb.BTreeImage()
    try:
        stats = bt.open(case.image)
        w_kind, w_level, w_stats = bref.check(case.image, case.meta)
        assert stats == w_stats and bt.meta.as_dict() == case.meta, name
        assert np.array_equal(bt.kind.cpu().numpy()[: len(w_kind)], w_kind) and np.array_equal(bt.level.cpu().numpy()[: len(w_level)], w_level)
        assert bt.check() == w_stats
        keys = bref.probes(case, np.random.default_rng(15))
        status, off, vals = bt.get_batch(keys)
        want = bref.get_batch(case.image, case.meta, keys)
        assert np.array_equal(status, want[0]), name
        w_vals = iter(bref.values(case.image, want))
        for i, st in enumerate(status):
            assert vals[int(off[i]): int(off[i + 1])].tobytes() == (next(w_vals) if st == bref.FOUND else b""), (name, i)
        if case.puts is not None:
            status, off, vals = bt.get_batch(case.keys)
            assert (status == bref.FOUND).all()
            assert all(vals[int(off[i]): int(off[i + 1])].tobytes() == case.puts[k] for i, k in enumerate(case.keys))
    finally:
        bt.close()
