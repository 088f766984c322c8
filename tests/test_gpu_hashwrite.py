"""GPU: the hash index's write side on the device (include/seb_bloom.h, "hash index, write side").

seb_dev_seg_frame_plan / _emit, seb_dev_seg_compact_plan / _emit and seb_dev_hidx_logical_size equal the host half
(seb_seg_frame_*, seb_seg_compact, seb_hidx_logical_size, themselves held to hashwrite_ref's restatement in
test_hashwrite.py) byte for byte: the frame cases with cuts, the compaction of every prefix of every shared case with
the test-only option hidx_hash_mask 0 and 3, c_one_key (3,001 records, one survivor), b_lengths (record sizes that
straddle 16-byte output boundaries), a store where every key ends deleted (an empty image), more than 256 survivors
(two CRC workgroups), and one 1 MiB value among 20-byte ones (the copy is split by output bytes).  Every output and
the workspace start as 0xA5 between 64 guard bytes, images sit at odd byte alignments.  seb_hidx_compact against the
host's compaction and read side.  HashIndex end to end: put_batch -> get_batch, then compact of the oldest 2 of 4
segments of a 300,000-record store.  With the option grid_cap at 1 and 2 the loops of k_sc_place, k_sc_copy,
k_hidx_logical and k_off_shift take several trips, and the outputs equal the default grid's byte for byte.  One case on a busy side stream with late inputs.  The refused inputs are data
errors answered with a status; nothing here provokes a fault."""
import numpy as np
import pytest

import crc_ref as cr
import hashindex_ref as href
import hashwrite_ref as wref
import stream_late as sl

pytestmark = pytest.mark.gpu

CASES = href.cases()
FRAMES = wref.frame_cases()
TS = 1_777_000_123
SIZE_KEYS = ("records_in", "live_in", "distinct", "survivors", "tombstoned", "shadowed", "image_bytes")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


@pytest.fixture(scope="module", autouse=True)
def no_fallback(seb):
    before = seb.fallback_count()
    yield
    assert seb.fallback_count() == before == 0


lead_view = sl.lead_view  # the bytes of an array on the device, `lead` bytes into an aligned allocation


# ------------------------------------------------------------------ frame

def dev_ops(torch, seb, keys, vals, val_off, deleted):
    """The ops of wref.ops_arrays on the device: keys 3 and values 5 bytes into their allocations."""
    if isinstance(keys, tuple):
        dk = seb.dev_keys(lead_view(torch, keys[0], 3), sl.to_dev(torch, keys[1]))
    else:
        dk = seb.dev_keys(lead_view(torch, keys, 3), n=keys.shape[0], stride=keys.shape[1])
    return dk, lead_view(torch, vals, 5), sl.to_dev(torch, val_off), lead_view(torch, deleted, 1)


def dev_frame(torch, seb, arrays, active, limit, what, image_lead=7):
    keys, vals, val_off, deleted = arrays
    n = val_off.size - 1
    want_image, want_off, want_cuts = seb.seg_frame(keys, vals, val_off, deleted, TS, active, limit)
    dk, d_vals, d_voff, d_del = dev_ops(torch, seb, keys, vals, val_off, deleted)
    rec_off = sl.Out(torch, n + 1, np.uint64)
    total, cuts = seb.dev_seg_frame_plan(dk, d_voff, d_del, rec_off.t, active, limit)
    assert total == want_image.size and cuts.tolist() == want_cuts.tolist(), what
    image = sl.Out(torch, total, np.uint8, lead=image_lead)
    assert total == 0 or image.t.data_ptr() % 16 == image_lead % 16
    seb.dev_seg_frame_emit(dk, d_vals, d_voff, d_del, TS, rec_off.t, image.t, total)
    torch.cuda.synchronize()
    if n:
        sl.same(rec_off.get("rec_off"), want_off, f"{what}: rec_off")
    sl.same(image.get("image"), want_image, f"{what}: image")
    return want_image, want_off


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_frame_cases(seb, torch_cuda, name):
    ops, lead, stride = FRAMES[name]
    arrays = wref.ops_arrays(ops, lead, stride)
    image, _ = dev_frame(torch_cuda, seb, arrays, 0, seb.SEG_NO_LIMIT, name)
    assert image.tobytes() == wref.frame(ops, TS)[0]
    for limit in (1, 100, 4096):
        for active in (0, limit - 1, limit, limit + 1):
            dev_frame(torch_cuda, seb, arrays, active, limit, (name, active, limit), image_lead=1 + (active & 7))


def kv_ops(kv, seed):
    """A Put batch with the given (key length, value length) per op."""
    rng = np.random.default_rng(seed)
    return [(bytes(rng.integers(0, 256, k, dtype=np.uint8)), bytes(rng.integers(0, 256, v, dtype=np.uint8))) for k, v in kv]


@pytest.mark.parametrize("span,lead,shape", cr.WINDOW_PARAMS)
def test_frame_seals_at_the_window_edges(seb, torch_cuda, span, lead, shape):
    """The frame's seal (k_seg_crc in seal mode) where the first 256 records span exactly 36,863 / 36,864 / 36,865
    bytes from the 16-aligned base below the image, a second workgroup behind them: the sealed image is the host
    half's."""
    ops = kv_ops(cr.kv_lengths("seg", cr.window_lengths(span, lead, shape, True)), seed=span + lead)
    off = wref.frame(ops, TS)[1].astype(np.int64)
    cov = cr.coverage(off[:-1], lead, off[1:], int(off[-1]))
    cr.assert_window(dict(name=f"window_{span}"), cov)
    assert len(cov["span"]) == 2
    image, _ = dev_frame(torch_cuda, seb, wref.ops_arrays(ops), 0, seb.SEG_NO_LIMIT, (span, lead, shape), image_lead=lead)
    assert image.tobytes() == wref.frame(ops, TS)[0]


@pytest.mark.parametrize("with_long", [False, True])
def test_frame_seals_every_alignment(seb, torch_cuda, with_long):
    """Payloads of 1..70 bytes at every start alignment, all staged; and again with one 40,000-byte record in every
    workgroup, so that the seal reads every short record straight from memory."""
    ops = kv_ops(cr.kv_lengths("seg", cr.frame_sweep_lengths("seg", with_long)), seed=42)
    off = wref.frame(ops, TS)[1].astype(np.int64)
    for lead in (0, 7):
        cov = cr.coverage(off[:-1], lead, off[1:], int(off[-1]))
        cr.assert_all_pairs(cov, cr.DIRECT if with_long else cr.STAGED)
        cr.assert_all_starts(cov)
        assert not any(cov["staged"]) if with_long else all(cov["staged"])
        dev_frame(torch_cuda, seb, wref.ops_arrays(ops), 0, seb.SEG_NO_LIMIT, ("sweep", with_long, lead), image_lead=lead)


def test_frame_cut_capacity_and_refusals(seb, torch_cuda):
    torch = torch_cuda
    ops, lead, stride = FRAMES["offsets_65"]
    keys, vals, val_off, deleted = wref.ops_arrays(ops, lead, stride)
    dk, d_vals, d_voff, d_del = dev_ops(torch, seb, keys, vals, val_off, deleted)
    rec_off = sl.Out(torch, 66, np.uint64)
    with pytest.raises(seb.SebError) as e:
        seb.dev_seg_frame_plan(dk, d_voff, d_del, rec_off.t, 1, 1, cut_cap=64)
    assert e.value.code == -4 and "65" in str(e.value)
    assert seb.dev_seg_frame_plan(dk, d_voff, d_del, rec_off.t, 1, 1, cut_cap=65)[1].tolist() == list(range(65))
    rec_off.get("rec_off")
    # more cuts than come back with the plan's synchronisation (1,024): 1,300 ops that each open a segment, more than
    # one tile of the scan
    many = [(b"k%04d" % i, b"v" * (i % 7)) for i in range(1300)]
    dev_frame(torch, seb, wref.ops_arrays(many), 1, 1, "1,300 cuts")
    assert seb.seg_frame_plan(*[wref.ops_arrays(many)[i] for i in (0, 2, 3)], 1, 1)[1].tolist() == list(range(1300))

    def refused(words, fn, *a, **kw):
        with pytest.raises(seb.SebError) as e:
            fn(*a, **kw)
        assert e.value.code == -1 and words in str(e.value), e.value

    # the offsets alone decide: the key and value bytes these offsets describe do not exist and are never read
    data, koff = href.key_lists([b"a", b"bb", b"ccc", b"dddd"])
    d_data = lead_view(torch, data, 3)
    voff = np.array([0, 4, 8, 12, 16], np.uint64)
    d_v = lead_view(torch, np.frombuffer(b"v" * 16, np.uint8), 5)
    big, half = 1 << 32, 1 << 31
    off5 = sl.Out(torch, 5, np.uint64)
    for bad_koff, bad_voff, dele, words in (
            ([0, 1, 3, 3, 7], voff, None, "op 2: an empty key"),
            ([0, 3, 2, 6, 10], voff, None, "op 1: its key offsets"),
            ([0, 0, 2, 1, 10], voff, None, "op 0: an empty key"),
            (koff, [0, 4, 8, 12, 11], None, "op 3: its value offsets"),
            ([0, 1, 3, 3 + big, 7 + big], voff, None, "op 2: its key offsets"),
            (koff, [0, 4, 4 + big, 12 + big, 16 + big], None, "op 1: its value offsets"),
            ([0, 1, 1 + half, 2 + half, 3 + half], [0, 4, 4 + half, 8 + half, 12 + half], None, "op 1: keySize + valueSize")):
        kb = seb.dev_keys(d_data, sl.to_dev(torch, np.array(bad_koff, np.uint64)))
        refused(words, seb.dev_seg_frame_plan, kb, sl.to_dev(torch, np.array(bad_voff, np.uint64)), dele, off5.t, 0, 50)
        off5.get("rec_off")
    good = seb.dev_keys(d_data, sl.to_dev(torch, koff))
    d_voff4 = sl.to_dev(torch, voff)
    refused("limit is 0", seb.dev_seg_frame_plan, good, d_voff4, None, off5.t, 0, 0)
    refused("rec_off", seb.dev_seg_frame_plan, good, d_voff4, None, rec_off.t.view(torch.uint8)[4:44], 0, 50)
    refused("8-byte aligned", seb.dev_seg_frame_plan, good, d_voff4.view(torch.uint8)[4:], None, off5.t, 0, 50)
    assert seb.dev_seg_frame_plan(good, d_voff4, None, off5.t, 0, 50)[0] == 106
    image = sl.Out(torch, 106, np.uint8, lead=3)
    refused("image_bytes", seb.dev_seg_frame_emit, good, d_v, d_voff4, None, TS, off5.t, image.t, 50)
    refused("null image", seb.dev_seg_frame_emit, good, d_v, d_voff4, None, TS, off5.t, None, 106)
    refused("rec_off", seb.dev_seg_frame_emit, good, d_v, d_voff4, None, TS, None, image.t, 106)
    torch.cuda.synchronize()
    assert (image.get("image") == sl.FILL).all(), "a refused emit wrote the image"
    # nothing to do is no refusal
    empty = seb.dev_keys(d_data, sl.to_dev(torch, np.zeros(1, np.uint64)))
    empty.n = 0
    assert seb.dev_seg_frame_plan(empty, None, None, None, 0, 50)[0] == 0
    seb.dev_seg_frame_emit(empty, None, None, None, TS, None, None, 0)


# ------------------------------------------------------------------ compaction

def dev_compact(torch, seb, pool, rec_off, live, what, pool_lead=1, image_lead=5, keep=None):
    """plan + emit on the device into guarded outputs against seb_seg_compact; returns the host's triple.  keep: a
    list that receives the device's (out_rec_off, image) bytes."""
    want_image, want_off, want = seb.seg_compact(pool, rec_off, live, TS)
    n = rec_off.size
    d_pool = lead_view(torch, pool, pool_lead)
    d_off, d_live = sl.to_dev(torch, rec_off), None if live is None else lead_view(torch, live, 1)
    ws = sl.Out(torch, max(seb.dev_seg_compact_workspace_size(n), 16), np.uint8)
    assert ws.t.data_ptr() % 16 == 0
    sz = seb.dev_seg_compact_plan(d_pool, pool.size, d_off if n else None, d_live if n else None, n, ws.t)
    assert sz.as_dict() == want, what
    image = sl.Out(torch, sz.image_bytes, np.uint8, lead=image_lead)
    out_off = sl.Out(torch, sz.survivors + 1, np.uint64)
    seb.dev_seg_compact_emit(d_pool, pool.size, d_off if n else None, n, TS, sz, ws.t, image.t if sz.image_bytes else None,
                             out_off.t)
    torch.cuda.synchronize()
    sl.same(out_off.get("out_rec_off"), want_off, f"{what}: out_rec_off")
    sl.same(image.get("image"), want_image, f"{what}: image")
    ws.get("workspace")
    if keep is not None:
        keep.append((out_off.get().tobytes(), image.get().tobytes()))
    return want_image, want_off, want


def prefix_arrays(seb, segments, c):
    pool, rec_off, first, base, size, _ = seb.segs_scan(list(segments)[:c])
    live = seb.seg_verify(pool, rec_off, first, base, size)[3]
    return pool, rec_off, live


@pytest.mark.parametrize("mask", [0, 3])
@pytest.mark.parametrize("name", sorted(CASES))
def test_compaction_of_every_prefix(seb, torch_cuda, name, mask):
    """The live records of every prefix (a segment cut by a bad record gives its records before the cut, as recover
    leaves the file); with mask 3 every key shares one tag and four home slots."""
    segments = CASES[name]
    assert len(href.recover(segments)["index"]) <= 2000
    with seb.option("hidx_hash_mask", mask):
        for c in range(1, len(segments) + 1):
            pool, rec_off, live = prefix_arrays(seb, segments, c)
            image, _, sizes = dev_compact(torch_cuda, seb, pool, rec_off, live, (name, c, mask), image_lead=1 + 2 * c)
            want = wref.compact(segments, c, TS)
            if want is not None:  # no bad record in the prefix: the reference's own image
                assert image.tobytes() == want["image"] and sizes == {k: want[k] for k in SIZE_KEYS}, (name, c)
    if name == "c_one_key":
        assert sizes["survivors"] == 1 and sizes["records_in"] == 3001 and sizes["shadowed"] == 3000


def many_keys(tag=b"v", keys=1100):
    """1,100 keys in two segments with rewrites and deletes: more than 256 survivors."""
    w1, w2 = href.Writer(), href.Writer(5000)
    for i in range(keys):
        (w1 if i < 600 else w2).put(b"key-%05d" % i, tag + b"-%d" % i)
    for i in range(0, keys, 3):
        w2.put(b"key-%05d" % i, tag + b"-second-%d" % i)
    for i in range(0, keys, 50):
        w2.delete(b"key-%05d" % i)
    return [w1.bytes(), w2.bytes()]


@pytest.mark.parametrize("mask", [0, 3])
def test_compaction_special_stores(seb, torch_cuda, mask):
    torch = torch_cuda
    with seb.option("hidx_hash_mask", mask):
        # every key ends deleted: an empty image, only out_rec_off[0] is written
        pool, rec_off, live = prefix_arrays(seb, wref.all_deleted(), 2)
        image, out_off, sizes = dev_compact(torch, seb, pool, rec_off, live, "all deleted")
        assert image.size == 0 and out_off.tolist() == [0] and sizes["tombstoned"] == 40
        # more than 256 survivors: two workgroups of the seal, more than one tile is not needed for that
        pool, rec_off, live = prefix_arrays(seb, many_keys(), 2)
        _, _, sizes = dev_compact(torch, seb, pool, rec_off, None, "many keys", pool_lead=0, image_lead=0)
        assert sizes["survivors"] == 1100 - 22 > 1024 and sizes["records_in"] == rec_off.size > 1024
        # one 1 MiB value among 20-byte ones, rewritten keys around it
        rng = np.random.default_rng(21)
        w = href.Writer()
        for i in range(60):
            w.put(b"small-%02d" % (i % 45), bytes(rng.integers(0, 256, 20, dtype=np.uint8)))
            if i == 30:
                w.put(b"the-long-one", bytes(rng.integers(0, 256, 1 << 20, dtype=np.uint8)))
        w.delete(b"small-03")
        pool, rec_off, live = prefix_arrays(seb, [w.bytes()], 1)
        image, _, sizes = dev_compact(torch, seb, pool, rec_off, live, "one long value", pool_lead=3, image_lead=9)
        assert sizes["survivors"] == 45 and image.size > 1 << 20


def test_compaction_refusals(seb, torch_cuda):
    torch = torch_cuda
    pool, rec_off, live = prefix_arrays(seb, CASES["a_65"], 1)
    n = rec_off.size
    d_pool, d_off = lead_view(torch, pool, 1), sl.to_dev(torch, rec_off)
    ws = sl.Out(torch, seb.dev_seg_compact_workspace_size(n), np.uint8)

    def refused(words, fn, *a, **kw):
        with pytest.raises(seb.SebError) as e:
            fn(*a, **kw)
        assert e.value.code == -1 and words in str(e.value), e.value

    refused("null pool", seb.dev_seg_compact_plan, None, pool.size, d_off, None, n, ws.t)
    refused("2^47", seb.dev_seg_compact_plan, d_pool, 1 << 47, d_off, None, n, ws.t)
    refused("rec_off", seb.dev_seg_compact_plan, d_pool, pool.size, None, None, n, ws.t)
    refused("rec_off", seb.dev_seg_compact_plan, d_pool, pool.size, d_off.view(torch.uint8)[4:], None, 3, ws.t)
    refused("workspace", seb.dev_seg_compact_plan, d_pool, pool.size, d_off, None, n, None)
    refused("workspace", seb.dev_seg_compact_plan, d_pool, pool.size, d_off, None, n, ws.t[8:])
    refused("workspace", seb.dev_seg_compact_plan, d_pool, pool.size, d_off, None, n, ws.t, ws_bytes=ws.nbytes - 1)
    torch.cuda.synchronize()
    assert (ws.get("workspace") == sl.FILL).all(), "a refused plan wrote the workspace"
    # a live record that does not lie inside the pool is named; the same record not live is not looked at
    off2 = rec_off.copy()
    off2[9] = pool.size - 5
    off2[40] = pool.size + 100
    refused("record 9", seb.dev_seg_compact_plan, d_pool, pool.size, sl.to_dev(torch, off2), None, n, ws.t)
    live2 = np.ones(n, np.uint8)
    live2[[9, 40]] = 0
    want = seb.seg_compact(pool, off2, live2, TS)[2]
    assert seb.dev_seg_compact_plan(d_pool, pool.size, sl.to_dev(torch, off2), sl.to_dev(torch, live2), n, ws.t).as_dict() == want
    # the emit: sizes that are not a plan's, null outputs; then a workspace that holds another plan writes nothing
    sz = seb.dev_seg_compact_plan(d_pool, pool.size, d_off, None, n, ws.t)
    image, out_off = sl.Out(torch, sz.image_bytes, np.uint8, lead=3), sl.Out(torch, sz.survivors + 1, np.uint64)
    wrong = seb.seb_segcompact_sizes.from_buffer_copy(sz)
    wrong.records_in += 1
    refused("sizes", seb.dev_seg_compact_emit, d_pool, pool.size, d_off, n, TS, wrong, ws.t, image.t, out_off.t)
    with pytest.raises(ValueError):
        seb.dev_seg_compact_emit(d_pool, pool.size, d_off, n, TS, sz, ws.t, image.t, None)
    other_pool, other_off, _ = prefix_arrays(seb, CASES["a_64"], 1)
    seb.dev_seg_compact_plan(lead_view(torch, other_pool, 1), other_pool.size, sl.to_dev(torch, other_off), None, other_off.size, ws.t)
    seb.dev_seg_compact_emit(d_pool, pool.size, d_off, n, TS, sz, ws.t, image.t, out_off.t)
    torch.cuda.synchronize()
    assert (out_off.get("out_rec_off") == np.uint64(0xA5A5A5A5A5A5A5A5)).all(), "an emit on another plan's workspace wrote offsets"
    assert seb.dev_seg_compact_plan(None, 0, None, None, 0, None).as_dict()["survivors"] == 0  # nothing to do


# ------------------------------------------------------------------ logical size, seb_hidx_compact

def upload_store(torch, seb, segments):
    pool, rec_off, first, base, size, _ = seb.segs_scan(segments)
    live = seb.seg_verify(pool, rec_off, first, base, size)[3]
    return dict(pool=pool, rec_off=rec_off, first=first, base=base, size=size, live=live, d_pool=lead_view(torch, pool, 0),
                d_off=sl.to_dev(torch, rec_off), d_live=sl.to_dev(torch, live))


@pytest.mark.parametrize("name", ["b_lengths", "d_put_put_delete", "e_flip_value", "a_empty", "c_one_key"])
def test_logical_size(seb, torch_cuda, name):
    torch = torch_cuda
    s = upload_store(torch, seb, CASES[name])
    rec = href.recover(CASES[name])
    capacity = max(len(rec["index"]), 1)
    table = torch.zeros(seb.dev_hidx_table_bytes(capacity), dtype=torch.uint8, device="cuda")
    seb.dev_hidx_insert(table, capacity, s["d_pool"], s["pool"].size, s["d_off"], s["d_live"], s["rec_off"].size)
    got = seb.dev_hidx_logical_size(table, capacity, s["d_pool"], s["pool"].size)
    assert got == seb.hidx_logical_size(s["pool"], s["rec_off"], s["live"]) == wref.logical_size(CASES[name], rec["index"])


@pytest.mark.parametrize("name,c", [("b_lengths", 1), ("d_put_delete_put", 2), ("d_put_put_delete", 3), ("f_short_then_more", 2),
                                    ("e_flip_size_eof", 2), ("e_flip_key", 1), ("a_empty_between", 2)])
def test_hidx_compact_on_a_context(seb, torch_cuda, name, c):
    """The oldest c segments compacted through seb_hidx_compact: the new pool is the host's image followed by the
    segments that stay, the offsets and the table answer every Get as the store did before."""
    hidx_compact_check(torch_cuda, seb, CASES[name], c)


def hidx_compact_check(torch, seb, segments, c):
    """Returns the bytes of the new pool, of the new offsets and of the Get's outputs."""
    s = upload_store(torch, seb, segments)
    want_image, want_off, want_sizes = seb.segs_compact(segments, c, TS)
    after = [want_image.tobytes()] + list(segments[c:])
    h = upload_store(torch, seb, after)  # the host's view of the compacted store
    n_head = int(s["first"][c])
    rest_n = s["rec_off"].size - n_head
    capacity = max(int(s["live"].sum()), 1)
    table = sl.Out(torch, seb.dev_hidx_table_bytes(capacity), np.uint8)
    dst = sl.Out(torch, h["pool"].size, np.uint8)
    new_off = sl.Out(torch, want_sizes["survivors"] + rest_n + 1, np.uint64)
    ctx = seb.Ctx(0)
    try:
        got = ctx.hidx_compact(s["d_pool"], s["pool"].size, s["base"], s["size"], c, s["d_off"][n_head:] if rest_n else None,
                               s["d_live"][n_head:] if rest_n else None, rest_n, TS, dst.t if h["pool"].size else None, table.t,
                               capacity, new_off.t)
    finally:
        ctx.close()
    assert got["sizes"] == want_sizes and got["pool_bytes"] == h["pool"].size
    assert got["seg_base"].tolist() == h["base"].tolist() and got["seg_bytes"].tolist() == h["size"].tolist()
    sl.same(dst.get("the new pool"), h["pool"], "the new pool")
    offs = new_off.get("new_rec_off")
    # the segments that stay keep records a cut has killed: their offsets move with them, dead or live
    rest_want = s["rec_off"][n_head:].astype(np.int64) - int(s["base"][c] if c < len(segments) else s["pool"].size) + want_image.size
    sl.same(offs, np.concatenate([want_off[:-1].astype(np.int64), rest_want, [h["pool"].size]]).astype(np.uint64), "new_rec_off")
    before = href.recover(segments)
    keys = href.probes(before, np.random.default_rng(5))
    assert got["distinct"] == len(before["index"]) - wref.count_drop(segments, c) == len(href.recover(after)["index"])
    outs = [sl.Out(torch, len(keys), t) for t in (np.uint8, np.uint64, np.uint64, np.uint32, np.uint8)]
    data, koff = href.key_lists(keys)
    dk = seb.dev_keys(lead_view(torch, data, 3), sl.to_dev(torch, koff))
    seb.dev_hidx_get(table.t, capacity, dst.t if h["pool"].size else s["d_pool"], h["pool"].size, dk, True, *[o.t for o in outs])
    torch.cuda.synchronize()
    st, rec, vloc, vlen, _ = seb.hidx_lookup(h["pool"], h["rec_off"], h["live"], (data, koff), True)
    for nm, o, w in zip(("status", "rec", "vloc", "vlen"), outs, (st, rec, vloc, vlen)):
        sl.same(o.get(nm), w, nm)
    assert [int(x) for x in st] == [a[0] for a in wref.answers(segments, keys)]
    table.get("table")
    return [dst.get().tobytes(), offs.tobytes()] + [o.get().tobytes() for o in outs]


# ------------------------------------------------------------------ capped grids: the grid-stride loops iterate

@pytest.mark.parametrize("mask", [0, 3])
def test_compaction_under_a_grid_cap(seb, torch_cuda, mask):
    """The compaction's plan (k_hidx_insert) and emit (k_sc_place, a lane per record; k_sc_copy, a lane per 16 output
    bytes on four times the capped grid) at 1 and 2 workgroups: three trips over the records, two over the image's
    chunks, the last ones partial.  Sizes, offsets and image equal the host's and the default grid's byte for byte."""
    pool, rec_off, live = prefix_arrays(seb, many_keys(), 2)
    assert 2 * 256 * 2 < rec_off.size < 2 * 256 * 3
    keep = []
    with seb.option("hidx_hash_mask", mask):
        for cap in sl.CAPS:
            with sl.grid_cap(seb, cap):
                image, _, sizes = dev_compact(torch_cuda, seb, pool, rec_off, live, ("many keys", mask, cap), image_lead=3, keep=keep)
    chunks = (3 + image.size + 15) // 16
    assert 2 * 4 * 256 < chunks < 2 * 2 * 4 * 256 and sizes["survivors"] > 1024
    assert keep[1] == keep[0] and keep[2] == keep[0]


def test_logical_size_under_a_grid_cap(seb, torch_cuda):
    """seb_dev_hidx_logical_size (k_hidx_logical, a lane per slot) at 1 and 2 workgroups: 16 and 8 trips over 4,096
    slots, a wave's sum added once per wave."""
    torch = torch_cuda
    segments = many_keys()
    s = upload_store(torch, seb, segments)
    rec = href.recover(segments)
    capacity = len(rec["index"])
    assert seb.dev_hidx_table_bytes(capacity) == 64 + 8 * 4096
    table = torch.zeros(seb.dev_hidx_table_bytes(capacity), dtype=torch.uint8, device="cuda")
    seb.dev_hidx_insert(table, capacity, s["d_pool"], s["pool"].size, s["d_off"], s["d_live"], s["rec_off"].size)
    want = seb.hidx_logical_size(s["pool"], s["rec_off"], s["live"])
    assert want == wref.logical_size(segments, rec["index"]) > 10_000
    for cap in sl.CAPS:
        with sl.grid_cap(seb, cap):
            assert seb.dev_hidx_logical_size(table, capacity, s["d_pool"], s["pool"].size) == want, cap


def test_hidx_compact_under_a_grid_cap(seb, torch_cuda):
    """seb_hidx_compact whole at 1 and 2 workgroups; the offset shift (k_off_shift) moves the 1,489 offsets of the
    segments that stay, and the end offset, in three trips."""
    w0 = href.Writer(100)
    for i in range(100):
        w0.put(b"old-%03d" % i, b"o" * (i % 9))
    w0.put(b"key-00007", b"shadowed by the segments that stay")
    segments = [w0.bytes()] + many_keys()
    first = seb.segs_scan(segments)[2]
    rest = int(first[3] - first[1])
    assert 2 * 256 * 2 < rest + 1 < 2 * 256 * 3
    runs = []
    for cap in sl.CAPS:
        with sl.grid_cap(seb, cap):
            runs.append(hidx_compact_check(torch_cuda, seb, segments, 1))
    assert runs[1] == runs[0] and runs[2] == runs[0]


def test_hidx_compact_aborts_on_a_bad_record_and_reports_small_capacities(seb, torch_cuda):
    torch = torch_cuda
    segments = CASES["e_flip_value"]
    s = upload_store(torch, seb, segments)
    rec = href.recover(segments)
    capacity = 200
    table = torch.zeros(seb.dev_hidx_table_bytes(capacity), dtype=torch.uint8, device="cuda")
    dst = sl.Out(torch, s["pool"].size, np.uint8)
    new_off = sl.Out(torch, s["rec_off"].size + 1, np.uint64)
    n2 = int(s["first"][2])
    ctx = seb.Ctx(0)
    try:
        with pytest.raises(seb.SebError) as e:
            ctx.hidx_compact(s["d_pool"], s["pool"].size, s["base"], s["size"], 2, s["d_off"][n2:], s["d_live"][n2:],
                             s["rec_off"].size - n2, TS, dst.t, table, capacity, new_off.t)
        assert e.value.code == -1 and "segment 1" in str(e.value) and f"record {rec['valid'][1]}" in str(e.value)
        n1 = int(s["first"][1])
        with pytest.raises(seb.SebError) as e:
            ctx.hidx_compact(s["d_pool"], s["pool"].size, s["base"], s["size"], 1, s["d_off"][n1:], s["d_live"][n1:],
                             s["rec_off"].size - n1, TS, dst.t, table, capacity, new_off.t, dst_cap=100)
        assert e.value.code == -4 and e.value.compacted["sizes"] == seb.segs_compact(segments, 1, TS)[2]
        with pytest.raises(seb.SebError) as e:
            ctx.hidx_compact(s["d_pool"], s["pool"].size, s["base"][::-1].copy(), s["size"], 1, s["d_off"][n1:], s["d_live"][n1:],
                             s["rec_off"].size - n1, TS, dst.t, table, capacity, new_off.t)
        assert e.value.code == -1 and "segment" in str(e.value)
    finally:
        ctx.close()
    torch.cuda.synchronize()
    assert (dst.get("dst") == sl.FILL).all() and (new_off.get("new_rec_off") == np.uint64(0xA5A5A5A5A5A5A5A5)).all()


# ------------------------------------------------------------------ HashIndex end to end

def test_put_batch_then_get_batch(seb, torch_cuda):
    """Batches with rewrites and deletes, rotation at 4 KiB: the images are segment.append's, the cuts the rotation's,
    and every Get (verify on) answers as recover() of the written files does."""
    rng = np.random.default_rng(31)
    hx = seb.HashIndex()
    hx.segment_limit = 4096
    files, live_keys = [b""], []
    try:
        for b in range(4):
            ops = []
            for i in range(120):
                k = b"put-%04d" % int(rng.integers(0, 300))
                ops.append((k, None if rng.random() < 0.15 else bytes(rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8))))
                live_keys.append(k)
            keys, vals, val_off, deleted = wref.ops_arrays(ops, lead=b)
            image, rec_off, cuts = hx.put_batch(keys, vals, val_off, deleted, timestamp=TS + b)
            want, want_off = wref.frame(ops, TS + b)
            assert image.tobytes() == want and np.array_equal(rec_off, want_off)
            assert cuts.tolist() == wref.cuts(np.diff(want_off.astype(np.int64)).tolist(), len(files[-1]), 4096)
            edges = [0] + [int(rec_off[int(c)]) for c in cuts] + [len(want)]
            files[-1] += want[edges[0]: edges[1]]
            files += [want[edges[i]: edges[i + 1]] for i in range(1, len(edges) - 1)]
        assert len(files) > 4 and [len(f) for f in files] == [int(x) for x in hx._seg_bytes]
        rec = href.recover(files)
        assert hx.count == len(rec["index"]) and not any(rec["cut"])
        keys = sorted(set(live_keys)) + [b"absent", b"put-"]
        status, off, vals = hx.get_batch(keys, verify=True)
        w_st, _, _, _, w_vals = href.get_batch(files, rec["index"], keys)
        assert np.array_equal(status, w_st) and (w_st == href.FOUND).sum() > 100
        for i, w in enumerate(w_vals):
            assert vals[int(off[i]): int(off[i + 1])].tobytes() == w, i
        assert hx.logical_size() == wref.logical_size(files, rec["index"])
    finally:
        hx.close()


@pytest.fixture(scope="module")
def big(seb):
    rng = np.random.default_rng(11)
    segments, keytab = href.big_store(rng, records=300_000)
    return segments, keytab, wref.count_drop(segments, 2)


def test_compact_the_oldest_two_of_four_segments(seb, torch_cuda, big):
    segments, keytab, drop = big
    import keygen as kg
    probe = np.concatenate([keytab, kg.key16(np.arange(10**7, 10**7 + 20_000))])
    image, _, want_sizes = seb.segs_compact(segments, 2, TS)
    after = [image.tobytes()] + list(segments[2:])
    pool, rec_off, first, base, size, _ = seb.segs_scan(after)
    live = seb.seg_verify(pool, rec_off, first, base, size)[3]
    hx = seb.HashIndex()
    try:
        hx.recover(segments)
        count = hx.count
        before = hx.get_batch(probe, verify=True)
        logical = hx.logical_size()
        sizes = hx.compact(2, TS)
        assert sizes == want_sizes and drop > 0
        assert count - hx.count == drop
        assert hx.pool_bytes == pool.size and [int(x) for x in hx._seg_bytes] == [int(x) for x in size]
        got = hx.get_batch(probe, verify=True)
        for g, w, nm in zip(got, before, ("status", "out_off", "values")):
            sl.same(g, w, nm)
        assert 60_000 < int((got[0] == href.FOUND).sum()) < 100_000
        assert hx.logical_size() == seb.hidx_logical_size(pool, rec_off, live) < logical
        sl.same(hx.pool[: hx.pool_bytes].cpu().numpy(), pool, "the compacted pool")
    finally:
        hx.close()


# ------------------------------------------------------------------ a busy side stream, late inputs

@pytest.fixture(scope="module")
def rig(seb, torch_cuda):
    try:
        r = sl.Rig(torch_cuda, seb)
    except AssertionError as e:
        pytest.fail(f"stream control: {e}")
    return r


def test_on_a_busy_side_stream(seb, torch_cuda, rig):
    """Frame: the value offsets arrive late before the plan, the values late before the emit.  Compaction: the live
    flags arrive late before the plan, the pool late before the emit."""
    torch = torch_cuda
    ops, lead, stride = FRAMES["offsets_257"]
    keys, vals, val_off, deleted = wref.ops_arrays(ops, lead, stride)
    poison_voff = np.arange(val_off.size, dtype=np.uint64)  # every value one byte
    poison_vals = vals ^ np.uint8(0x5A)
    want_image, want_off, want_cuts = seb.seg_frame(keys, vals, val_off, deleted, TS, 10, 9000)
    p_image, p_off, p_cuts = seb.seg_frame(keys, vals, poison_voff, deleted, TS, 10, 9000)
    sl.differ([want_off, want_cuts], [p_off, p_cuts], ["rec_off", "cuts"])
    L = rig.session()
    dk = seb.dev_keys(lead_view(torch, keys[0], 3), sl.to_dev(torch, keys[1]))
    d_del = lead_view(torch, deleted, 1)
    d_voff = L.inp(val_off, poison_voff)
    rec_off = L.out(val_off.size, np.uint64)
    L.arm()
    total, cuts = L.plan(seb.dev_seg_frame_plan, dk, d_voff, d_del, rec_off.t, 10, 9000)
    assert total == want_image.size and cuts.tolist() == want_cuts.tolist()
    d_vals = L.inp(vals, poison_vals)
    image = L.out(total, np.uint8, lead=3)
    L.arm()
    L.call(seb.dev_seg_frame_emit, dk, d_vals, d_voff, d_del, TS, rec_off.t, image.t, total)
    L.finish()
    sl.same(rec_off.get("rec_off"), want_off, "rec_off")
    sl.same(image.get("image"), want_image, "image")

    good, poison = many_keys(b"v"), many_keys(b"w")
    pool, off, live = prefix_arrays(seb, good, 2)
    poison_pool = seb.segs_scan(poison)[0]
    assert poison_pool.size == pool.size
    want = seb.seg_compact(pool, off, live, TS)
    sl.differ([want[0]], [seb.seg_compact(poison_pool, off, live, TS)[0]], ["image"])
    sl.differ([want[2]["survivors"]], [seb.seg_compact(pool, off, np.zeros_like(live), TS)[2]["survivors"]], ["survivors"])
    n = off.size
    L = rig.session()
    d_off = sl.to_dev(torch, off)
    d_live = L.inp(live, np.zeros_like(live))
    d_pool = sl.to_dev(torch, pool)
    ws = L.out(seb.dev_seg_compact_workspace_size(n), np.uint8)
    L.arm()
    sz = L.plan(seb.dev_seg_compact_plan, d_pool, pool.size, d_off, d_live, n, ws.t)
    assert sz.as_dict() == want[2]
    late_pool = L.inp(pool, poison_pool)
    out_image, out_off = L.out(sz.image_bytes, np.uint8, lead=1), L.out(sz.survivors + 1, np.uint64)
    L.arm()
    L.call(seb.dev_seg_compact_emit, late_pool, pool.size, d_off, n, TS, sz, ws.t, out_image.t, out_off.t)
    L.finish()
    sl.same(out_off.get("out_rec_off"), want[1], "out_rec_off")
    sl.same(out_image.get("image"), want[0], "image")
