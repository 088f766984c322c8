"""GPU: the memtable write side (include/seb_bloom.h, the memtable write side group), the device
form against the host half byte for byte (the host half is held to memwrite_ref's restatement in test_memwrite.py).

Outputs start as 0xA5 between guard bytes; keys, values and deleted sit at odd device addresses and key_off[0] /
val_off[0] are non-zero.

Frame: n = 0, 1, 63, 64, 65, 1023, 1024, 1025, 50,000 and 140,000 (the scan's carry), every seb_keys layout, the
empty key, empty values, a Delete that carries value bytes, deleted bytes 2 and 255, no deleted array, a first_seq
above 2^32; SEB_WAL_VERIFY passes on every record and the image goes into seb_dev_wal_replay_* on the device.
Delta: 0, 1 and 7 existing runs, a key over a tombstone, a tombstone over a value, a key only the last run holds, a
negative total.  Fold: run sizes from {0, 1, 1023, 1024, 1025} in 1, 2 and 8 runs, identical runs, disjoint
interleaved runs, ORDER_KEYS, ties on the first 16 and 40 bytes, a run without seq, seq left out, a tombstone with
value bytes behind it, the shapes at which the structure changes (a tile's boundary, the scan's carry at 200,000
entries), a stale index.  End to end: three batches -> frame -> replay -> three runs -> lookup -> fold -> builder."""
import numpy as np
import pytest

import crc_ref as cr
import memget_ref as gref
import memtable_ref as mref
import memwrite_ref as wref

pytestmark = pytest.mark.gpu

GUARD = 64
A5_64 = int(np.array([0xA5A5A5A5A5A5A5A5], np.uint64).view(np.int64)[0])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def odd_view(torch, a, lead=1):
    """The bytes of `a` at an odd device address (lead bytes into an allocation)."""
    buf = torch.from_numpy(np.concatenate([np.full(lead, 0xEE, np.uint8), np.asarray(a, np.uint8)])).cuda()
    return buf[lead:]


def u64_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


class Guarded:
    """A device array of `count` elements of `dtype`, 0xA5 all over, between guards; `lead` bytes make a u8 array's
    address odd."""

    def __init__(self, torch, count, dtype=np.uint8, lead=0):
        self.torch, self.count, self.dtype = torch, count, np.dtype(dtype)
        if self.dtype == np.uint8:
            self.buf = torch.full((GUARD + lead + count + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            self.view = self.buf[GUARD + lead:GUARD + lead + count]
            assert lead % 2 == 0 or count == 0 or self.view.data_ptr() % 2 == 1
        else:
            assert self.dtype.itemsize == 8 and lead == 0
            self.buf = torch.full((GUARD + count + GUARD,), A5_64, dtype=torch.int64, device="cuda")
            self.view = self.buf[GUARD:GUARD + count]
        self.lead = lead

    def host(self, written=True):
        """The array on the host; the guards, and the array itself where it must not have been written, are checked."""
        self.torch.cuda.synchronize()
        h = self.buf.cpu().numpy().view(np.uint8)
        k = self.dtype.itemsize
        a, b = (GUARD + self.lead) * (1 if k == 1 else 8), (GUARD + self.lead) * (1 if k == 1 else 8) + self.count * k
        assert (h[:a] == 0xA5).all() and (h[b:] == 0xA5).all(), "bytes outside an output were written"
        if not written:
            assert (h == 0xA5).all(), "an output that was left out was written"
        return np.frombuffer(h[a:b].tobytes(), self.dtype)


# ------------------------------------------------------------------ frame

def big_ops(n, seed, klen=None):
    """The arrays of n ops made with numpy: key lengths 0..24 (or klen), value lengths 0..120, every 16th op a
    Delete that carries its value bytes, deleted bytes of {1, 2, 255}; 5 and 9 bytes in front of the keys and values."""
    rng = np.random.default_rng(seed)
    kl = rng.integers(0, 25, n) if klen is None else np.full(n, klen)
    vl = rng.integers(0, 121, n)
    if n > 2:
        kl[0], vl[1] = (0 if klen is None else klen), 0  # the empty key, an empty value
    koff = (5 + np.concatenate([[0], np.cumsum(kl)])).astype(np.uint64)
    voff = (9 + np.concatenate([[0], np.cumsum(vl)])).astype(np.uint64)
    keys = rng.integers(97, 101, int(koff[-1]), dtype=np.uint8)
    vals = rng.integers(0, 256, int(voff[-1]), dtype=np.uint8)
    dele = np.where(np.arange(n) % 16 == 3, rng.choice(np.array([1, 2, 255], np.uint8), n), 0).astype(np.uint8)
    return keys, koff, vals, voff, dele


def upload_ops(torch, seb, arrays, layout="varlen", with_deleted=True):
    """(the device seb_keys, vals, val_off, deleted) and the host keys argument of the same ops."""
    keys, koff, vals, voff, dele = arrays
    n = len(voff) - 1
    if layout == "varlen":
        dk = seb.dev_keys(odd_view(torch, keys), u64_dev(torch, koff))
        hk = (keys, koff)
    else:
        stride = int(koff[1] - koff[0]) if n else 16
        body = keys[int(koff[0]):]
        d = odd_view(torch, body) if layout == "fixed_odd" else torch.from_numpy(body.copy()).cuda()
        assert n == 0 or d.data_ptr() % 16 == 0 or layout == "fixed_odd"
        dk = seb.dev_keys(d, n=n, stride=stride)
        hk = body.reshape(n, stride)
    return dk, hk, odd_view(torch, vals, 3), u64_dev(torch, voff), (odd_view(torch, dele, 5) if with_deleted else None)


def device_frame(torch, seb, arrays, first_seq, layout="varlen", with_deleted=True, replay=True, image_lead=7):
    keys, koff, vals, voff, dele = arrays
    n = len(voff) - 1
    dk, hk, dvals, dvoff, ddel = upload_ops(torch, seb, arrays, layout, with_deleted)
    want_img, want_off = seb.wal_frame(hk, vals, voff, dele if with_deleted else None, first_seq)
    rec = Guarded(torch, n + 1, np.uint64)
    total = seb.dev_wal_frame_plan(dk, dvoff, ddel, rec.view)
    assert total == want_img.size
    img = Guarded(torch, total, lead=image_lead)
    assert total == 0 or img.view.data_ptr() % 16 == image_lead % 16
    seb.dev_wal_frame_emit(dk, dvals, dvoff, ddel, first_seq, rec.view, img.view, image_bytes=total)
    got_off = rec.host(written=n > 0)
    if n:
        assert np.array_equal(got_off, want_off), "rec_off differs"
    got = img.host()
    if not np.array_equal(got, want_img):
        at = int(np.nonzero(got != want_img)[0][0])
        raise AssertionError(f"the image differs first at byte {at} of {total} (record {int(np.searchsorted(want_off, at, 'right')) - 1})")
    if n == 0:
        return got
    ok = Guarded(torch, n)
    seb.dev_wal_crc(img.view, rec.view, seb.WAL_VERIFY, ok=ok.view)
    assert (ok.host() == 1).all(), "a record fails SEB_WAL_VERIFY"
    if replay:  # the image goes straight into the replay, on the device
        ws = torch.zeros(seb.dev_wal_replay_workspace_size(n), dtype=torch.uint8, device="cuda")
        sizes = seb.dev_wal_replay_plan(img.view, rec.view, ws)
        want = seb.wal_replay_emit(want_img, want_off)
        assert sizes == want[6]
        _, n_out, kb, vb = sizes[:4]
        out = [Guarded(torch, kb, lead=1), Guarded(torch, n_out + 1, np.uint64), Guarded(torch, vb, lead=3),
               Guarded(torch, n_out + 1, np.uint64), Guarded(torch, n_out, lead=1), Guarded(torch, n_out, np.uint64)]
        seb.dev_wal_replay_emit(img.view, rec.view, sizes, ws, *[o.view for o in out])
        for name, o, w in zip(("keys", "key_off", "vals", "val_off", "deleted", "seq"), out, want):
            assert np.array_equal(o.host(), w), f"the replayed run's {name} differs"
    return got


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 50_000, 140_000])
def test_frame_sizes(seb, torch_cuda, n):
    """1024 ops are a tile of the plan; 140,000 ops are 137 tiles, past the scan's first stretch of 128."""
    device_frame(torch_cuda, seb, big_ops(n, seed=n), first_seq=(1 << 32) + 17, replay=n <= 50_000)


@pytest.mark.parametrize("layout,klen", [("fixed", 16), ("fixed_odd", 16), ("fixed", 5), ("fixed_odd", 5), ("fixed", 24),
                                         ("fixed", 40), ("varlen", 16), ("varlen", None)])
def test_frame_key_layouts(seb, torch_cuda, layout, klen):
    device_frame(torch_cuda, seb, big_ops(1500, seed=7, klen=klen), first_seq=9, layout=layout)


def test_frame_edges(seb, torch_cuda):
    """The empty key, empty values, a Delete that carries value bytes, deleted bytes 2 and 255, no deleted array,
    long keys and values (whole 16-byte chunks inside one key or value), against the restatement as well."""
    torch = torch_cuda
    for byte in (1, 2, 255):
        ops = wref.edge_ops()
        got = device_frame(torch, seb, wref.op_arrays(ops, 5, 9, byte), first_seq=(1 << 40) + 1)
        assert got.tobytes() == mref.wal_image(wref.batch_records(ops, (1 << 40) + 1))[0]
    rng = np.random.default_rng(2)
    ops = [(bytes(rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8)),
            bytes(rng.integers(0, 256, int(rng.integers(0, 5000)), dtype=np.uint8)), int(rng.random() < 0.2)) for _ in range(120)]
    got = device_frame(torch, seb, wref.op_arrays(ops, 5, 9), first_seq=3)
    assert got.tobytes() == mref.wal_image(wref.batch_records(ops, 3))[0]
    got = device_frame(torch, seb, wref.op_arrays(ops, 5, 9), first_seq=3, with_deleted=False)  # every op is a Put
    assert got.tobytes() == mref.wal_image(wref.batch_records([(k, v, 0) for k, v, _ in ops], 3))[0]
    only_deletes = [(b"k%d" % i, b"carried", 1) for i in range(70)]
    device_frame(torch, seb, wref.op_arrays(only_deletes, 1, 1), first_seq=1)
    device_frame(torch, seb, wref.op_arrays([(b"", b"", 0)] * 70, 1, 1), first_seq=1)  # 21-byte records only


def kv_ops(kv, seed):
    """The arrays of a Put batch with the given (key length, value length) per op."""
    rng = np.random.default_rng(seed)
    koff = (5 + np.concatenate([[0], np.cumsum([k for k, _ in kv])])).astype(np.uint64)
    voff = (9 + np.concatenate([[0], np.cumsum([v for _, v in kv])])).astype(np.uint64)
    return (rng.integers(0, 256, int(koff[-1]), dtype=np.uint8), koff, rng.integers(0, 256, int(voff[-1]), dtype=np.uint8), voff,
            np.zeros(len(kv), np.uint8))


@pytest.mark.parametrize("span,lead,shape", cr.WINDOW_PARAMS)
def test_frame_seals_at_the_window_edges(seb, torch_cuda, span, lead, shape):
    """The frame's seal (k_wal_crc in seal mode) where the first 256 records span exactly 36,863 / 36,864 / 36,865
    bytes from the 16-aligned base below the image, a second workgroup behind them: the sealed image is the host
    half's, and every record passes SEB_WAL_VERIFY."""
    arrays = kv_ops(cr.kv_lengths("wal", cr.window_lengths(span, lead, shape, True)), seed=span + lead)
    want_off = seb.wal_frame_plan((arrays[0], arrays[1]), arrays[3], arrays[4])[0]
    cov = cr.coverage(want_off, lead)
    cr.assert_window(dict(name=f"window_{span}"), cov)
    assert len(cov["span"]) == 2
    device_frame(torch_cuda, seb, arrays, first_seq=5, replay=False, image_lead=lead)


@pytest.mark.parametrize("with_long", [False, True])
def test_frame_seals_every_alignment(seb, torch_cuda, with_long):
    """Payloads of 1..70 bytes at every start alignment, all staged; and again with one 40,000-byte record in every
    workgroup, so that the seal reads every short record straight from memory."""
    arrays = kv_ops(cr.kv_lengths("wal", cr.frame_sweep_lengths("wal", with_long)), seed=41)
    want_off = seb.wal_frame_plan((arrays[0], arrays[1]), arrays[3], arrays[4])[0]
    for lead in (0, 7):
        cov = cr.coverage(want_off, lead)
        cr.assert_all_pairs(cov, cr.DIRECT if with_long else cr.STAGED)
        cr.assert_all_starts(cov)
        assert not any(cov["staged"]) if with_long else all(cov["staged"])
        device_frame(torch_cuda, seb, arrays, first_seq=1 << 33, replay=False, image_lead=lead)


def test_frame_refusals_name_the_host_halfs_op(seb, torch_cuda):
    torch = torch_cuda
    n = 3000
    keys, koff, vals, voff, dele = big_ops(n, seed=5)
    for which, op in ((1, 2500), (3, 1200)):
        for huge in (False, True):
            a = [keys, koff.copy(), vals, voff.copy(), dele]
            if huge:
                a[which][op + 1:] += np.uint64(1 << 32)
            else:
                a[which][op + 1] = a[which][op] - np.uint64(1)
            a[which][2901] = a[which][2900] - np.uint64(1)  # a later offender, in another tile
            with pytest.raises(seb.SebError) as host:
                seb.wal_frame_plan((a[0], a[1]), a[3], a[4])
            rec = Guarded(torch, n + 1, np.uint64)
            with pytest.raises(seb.SebError) as dev:
                seb.dev_wal_frame_plan(seb.dev_keys(odd_view(torch, keys), u64_dev(torch, a[1])), u64_dev(torch, a[3]),
                                       odd_view(torch, dele), rec.view)
            rec.host()  # the guards
            assert dev.value.code == -1 and f"op {op}:" in str(dev.value), str(dev.value)
            assert str(host.value).split("op ", 1)[1] == str(dev.value).split("op ", 1)[1]
    dk, _, dvals, dvoff, ddel = upload_ops(torch, seb, (keys, koff, vals, voff, dele))
    rec = Guarded(torch, n + 1, np.uint64)
    total = seb.dev_wal_frame_plan(dk, dvoff, ddel, rec.view)
    img = Guarded(torch, total, lead=1)
    with pytest.raises(seb.SebError) as ei:  # fewer bytes than n headers
        seb.dev_wal_frame_emit(dk, dvals, dvoff, ddel, 1, rec.view, img.view, image_bytes=21 * n - 1)
    assert ei.value.code == -1
    img.host(written=False)


# ------------------------------------------------------------------ runs

def key_of(i, klen=16):
    return (b"%0*d" % (klen, i))[:klen]


def sized_run(n, seed=0, klen=16, step=3, shift=0, carried=0):
    """n entries with keys key_of(step * i + shift): value sizes 0..40, every 7th entry deleted (with `carried`
    value bytes behind it), sequences out of order; 5 and 9 bytes in front of the keys and the values."""
    rng = np.random.default_rng(seed)
    keys = np.frombuffer(b"\xee" * 5 + b"".join(key_of(step * i + shift, klen) for i in range(n)), np.uint8)
    koff = 5 + np.arange(n + 1, dtype=np.uint64) * np.uint64(klen)
    dele = (np.arange(n) % 7 == 3).astype(np.uint8) * np.uint8(255)
    vlen = np.where(dele != 0, carried, rng.integers(0, 41, n))
    voff = (9 + np.concatenate([[0], np.cumsum(vlen)])).astype(np.uint64)
    return (keys, koff, rng.integers(0, 256, int(voff[-1]), dtype=np.uint8), voff, dele,
            rng.integers(1, 1 << 50, n).astype(np.uint64))


def upload_run(torch, seb, a, with_seq=True):
    """arrays (keys, key_off, vals, val_off, deleted, seq) -> (a dev_run whose keys and deleted sit at odd addresses,
    its values at an odd address)."""
    keys, koff, vals, voff, dele, seq = a
    run = seb.dev_run(odd_view(torch, keys), u64_dev(torch, koff), u64_dev(torch, voff), odd_view(torch, dele, 3),
                      u64_dev(torch, seq) if with_seq and seq is not None else None, n=len(koff) - 1, key_bytes=keys.size)
    return run, odd_view(torch, vals, 1)


def build_index(torch, seb, run):
    if not run.n:
        return None
    ix = torch.zeros(seb.dev_run_index_size(run.n), dtype=torch.uint8, device="cuda")
    seb.dev_run_index(run, ix)
    return ix


def host_run(seb, a, with_seq=True):
    return seb.host_run(a[0], a[1], a[3], a[4], a[5] if with_seq else None)


# ------------------------------------------------------------------ delta

def device_delta(torch, seb, fresh, existing):
    drun = [upload_run(torch, seb, a)[0] for a in existing]
    out = Guarded(torch, 1, np.uint64)
    seb.dev_run_size_delta(upload_run(torch, seb, fresh)[0], drun, [build_index(torch, seb, r) for r in drun], out.view)
    got = int(out.host().view(np.int64)[0])
    want = seb.run_size_delta(host_run(seb, fresh), [host_run(seb, a) for a in existing])
    assert got == want, (got, want)
    return got


@pytest.mark.parametrize("num_runs", [0, 1, 7])
def test_delta_over_runs(seb, torch_cuda, num_runs):
    rng = np.random.default_rng(num_runs)
    tables = [gref.random_table(rng, 300) for _ in range(num_runs)]
    if num_runs == 7:
        tables[3] = mref.MemTable()  # an empty run among them
    fresh = gref.random_table(rng, 400)
    got = device_delta(torch_cuda, seb, gref.run_arrays(fresh, 5, 9), [gref.run_arrays(t, 3, 7) for t in tables])
    before = wref.fold(tables)
    assert got == wref.fold([fresh] + tables).size - before.size  # the restatement's own sizes
    if num_runs == 0:
        assert got == fresh.size
    for n in (1, 63, 64, 65, 1025):  # a wave's and a workgroup's boundaries
        device_delta(torch_cuda, seb, sized_run(n, seed=n, step=2), [sized_run(700, seed=1)][:min(num_runs, 1)])
    device_delta(torch_cuda, seb, sized_run(0), [sized_run(50)][:min(num_runs, 1)])


def test_delta_cases_by_name(seb, torch_cuda):
    def run(ops):
        return gref.run_arrays(gref.table_from_ops(ops), 5, 9)
    old = [run([(b"t", b"", 1, 1), (b"v", b"0123456789", 2, 0)]), run([(b"t", b"hidden", 3, 0)]),
           run([(b"last", b"abcdefgh", 4, 0), (mref.P40 + b"x", b"tie-40", 5, 0), (mref.P16 + b"y", b"tie-16", 6, 0)])]
    fresh = run([(b"t", b"xyz", 7, 0), (b"v", b"", 8, 1), (b"last", b"", 9, 0), (b"new", b"12", 10, 0)])
    assert device_delta(torch_cuda, seb, fresh, old) == 3 - 10 - 8 + (3 + 16 + 2)
    fresh = run([(b"v", b"", 8, 1), (b"last", b"", 9, 1), (mref.P40 + b"x", b"", 10, 1), (mref.P16 + b"y", b"1", 11, 0),
                 (mref.P40 + b"z", b"", 12, 1)])
    assert device_delta(torch_cuda, seb, fresh, old) == -10 - 8 - 6 - 5 + (41 + 16)  # ties on 16 and 40 bytes
    assert device_delta(torch_cuda, seb, run([(b"v", b"", 8, 1), (b"last", b"", 9, 1)]), old) == -18  # a negative total
    big = [sized_run(50_000, seed=r, step=3, shift=r) for r in range(3)]
    assert device_delta(torch_cuda, seb, sized_run(50_000, seed=9, step=2), big) != 0


# ------------------------------------------------------------------ fold

NAMES = ("keys", "key_off", "vals", "val_off", "deleted", "seq")


def device_fold(torch, seb, arrays, with_seq=None, omit_seq=False, indexes=None, check=True):
    """The fold of `arrays` (newest first) on the device into guarded outputs; compared with the host half unless
    check is False (a stale index).  with_seq[r] False: run r has no seq array."""
    with_seq = with_seq or [True] * len(arrays)
    up = [upload_run(torch, seb, a, w) for a, w in zip(arrays, with_seq)]
    runs, vals = [u[0] for u in up], [u[1] for u in up]
    val_bytes = [a[2].size for a in arrays]
    indexes = [build_index(torch, seb, r) for r in runs] if indexes is None else indexes
    total = sum(r.n for r in runs)
    size = seb.dev_runs_fold_workspace_size(total)
    ws = Guarded(torch, size)
    assert ws.view.data_ptr() % 16 == 0
    sizes = seb.dev_runs_fold_plan(runs, indexes, val_bytes, ws.view, ws_bytes=size)
    _, n_out, kb, vb = sizes[:4]
    out = [Guarded(torch, kb, lead=1), Guarded(torch, n_out + 1, np.uint64), Guarded(torch, vb, lead=3),
           Guarded(torch, n_out + 1, np.uint64), Guarded(torch, n_out, lead=1), Guarded(torch, n_out, np.uint64)]
    views = [o.view for o in out]
    if omit_seq:
        views[5] = None
    seb.dev_runs_fold_emit(runs, indexes, vals, sizes, ws.view, *views, val_bytes=val_bytes)
    got = [o.host(written=not (omit_seq and j == 5) and (o.count > 0)) for j, o in enumerate(out)]
    ws.host()
    if check:
        want = seb.runs_fold([host_run(seb, a, w) for a, w in zip(arrays, with_seq)], [a[2] for a in arrays])
        assert sizes == want[6], (sizes, want[6])
        for j, name in enumerate(NAMES):
            if not (omit_seq and j == 5):
                assert np.array_equal(got[j], want[j]), f"the folded run's {name} differs"
    return got, sizes


@pytest.mark.parametrize("sizes", [(0,), (1,), (1023,), (1024,), (1025,), (1024, 0), (1, 1023), (1023, 1025), (1025, 1024),
                                   (0, 1, 1023, 1024, 1025, 1, 0, 1024), (1025,) * 8])
def test_fold_run_sizes(seb, torch_cuda, sizes):
    """1024 entries are a tile of the sums and of the emit: totals of 1023, 1024 and 1025, and a second and a ninth
    tile.  Steps 2 and 3 share every sixth key; the shifts make later runs hold keys of their own."""
    arrays = [sized_run(n, seed=r, step=2 + r % 2, shift=(r // 2) * 6, carried=r % 3) for r, n in enumerate(sizes)]
    _, sz = device_fold(torch_cuda, seb, arrays)
    assert sz[0] == sum(sizes)
    if len(sizes) > 1 and min(sizes) > 1000:
        assert sz[4] > 0 and sz[5] > 0


def test_fold_identical_and_disjoint_runs(seb, torch_cuda):
    a = sized_run(1500, seed=3, carried=2)
    got, sz = device_fold(torch_cuda, seb, [a] * 8)
    assert sz[:2] == (8 * 1500, 1500) and sz[4] == 7 * 1500  # everything but run 0 is shadowed
    assert np.array_equal(got[0], a[0][5:]) and np.array_equal(got[5], a[5])
    arrays = [sized_run(700, seed=r, step=8, shift=r) for r in range(8)]  # interleaved, no key twice
    _, sz = device_fold(torch_cuda, seb, arrays)
    assert sz[:2] == (5600, 5600) and sz[4] == 0


def test_fold_go_string_order_and_ties(seb, torch_cuda):
    ks = sorted(mref.ORDER_KEYS)
    every = gref.table_from_ops([(k, b"a%d" % i, 100 + i, i % 3 == 0) for i, k in enumerate(ks)])
    even = gref.table_from_ops([(k, b"e%d" % i, i, i % 4 == 0) for i, k in enumerate(ks) if i % 2 == 0])
    tie = gref.table_from_ops([(mref.P40 + bytes([i]), b"t%d" % i, 300 + i, i % 2) for i in range(0, 200, 3)] +
                              [(mref.P16 + bytes([i]), b"s%d" % i, 600 + i, 0) for i in range(0, 200, 5)])
    tie2 = gref.table_from_ops([(mref.P40 + bytes([i]), b"u%d" % i, 900 + i, 0) for i in range(0, 200, 2)] +
                               [(mref.P16 + bytes([i]) + b"x", b"w", 1, 0) for i in range(0, 200, 5)])
    for tables in ([every], [even, every], [every, even], [tie, tie2, every], [tie2, even, tie, mref.MemTable(), every]):
        got, sz = device_fold(torch_cuda, seb, [gref.run_arrays(t, 5, 9) for t in tables])
        assert mref.unpack(*got) == wref.entries_of(wref.fold(tables))  # the restatement directly
        assert sz == wref.fold_sizes(tables)


def test_fold_nullable_seq_and_runs_without_seq(seb, torch_cuda):
    arrays = [sized_run(900, seed=1), sized_run(1100, seed=2, step=2), sized_run(300, seed=3, step=5)]
    got, sz = device_fold(torch_cuda, seb, arrays, with_seq=[True, False, True])
    assert (got[5] == 0).any() and (got[5] != 0).any()
    device_fold(torch_cuda, seb, arrays, omit_seq=True)
    _, sz = device_fold(torch_cuda, seb, arrays, with_seq=[False] * 3)
    assert sz[6] == 0


def test_fold_scan_carry(seb, torch_cuda):
    """8 runs of 25,000: 200,000 entries are 196 tiles, past the scan's first stretch of 128 tiles."""
    arrays = [sized_run(25_000, seed=r, step=2 + r % 3, shift=r) for r in range(8)]
    _, sz = device_fold(torch_cuda, seb, arrays)
    assert sz[0] == 200_000 and sz[4] > 10_000


def test_fold_refusals(seb, torch_cuda):
    torch = torch_cuda
    a, b = sized_run(600, seed=1), sized_run(500, seed=2, step=2)
    up = [upload_run(torch, seb, x) for x in (a, b)]
    runs, vals = [u[0] for u in up], [u[1] for u in up]
    ix = [build_index(torch, seb, r) for r in runs]
    vb = [a[2].size, b[2].size]
    size = seb.dev_runs_fold_workspace_size(1100)
    ws = torch.zeros(size, dtype=torch.uint8, device="cuda")
    with pytest.raises(seb.SebError) as ei:
        seb.dev_runs_fold_plan(runs, ix, [vb[0], vb[1] - 1], ws)
    assert ei.value.code == -1 and "run 1: val_off[n]" in str(ei.value)
    with pytest.raises(seb.SebError) as ei:
        seb.dev_runs_fold_plan(runs, ix, vb, ws, ws_bytes=size - 1)
    assert ei.value.code == -1 and "workspace" in str(ei.value)
    with pytest.raises(seb.SebError) as ei:
        seb.dev_runs_fold_plan(runs * 5, ix * 5, vb * 5, ws)  # ten runs
    assert ei.value.code == -1
    sizes = seb.dev_runs_fold_plan(runs, ix, vb, ws)
    out = [Guarded(torch, sizes[2]), Guarded(torch, sizes[1] + 1, np.uint64), Guarded(torch, sizes[3]),
           Guarded(torch, sizes[1] + 1, np.uint64), Guarded(torch, sizes[1]), Guarded(torch, sizes[1], np.uint64)]
    views = [o.view for o in out]
    with pytest.raises(seb.SebError) as ei:  # a workspace that does not hold the plan
        seb.dev_runs_fold_emit(runs, ix, vals, sizes, torch.zeros_like(ws), *views, val_bytes=vb)
    assert ei.value.code == -1 and "plan" in str(ei.value)
    wrong = list(sizes)
    wrong[1], wrong[4] = wrong[1] - 1, wrong[4] + 1
    with pytest.raises(seb.SebError) as ei:  # sizes another plan could have returned, not this one
        seb.dev_runs_fold_emit(runs, ix, vals, tuple(wrong), ws, *views, val_bytes=vb)
    assert ei.value.code == -1
    for o in out:
        o.host(written=False)
    # nothing at all: no launch, the two first offsets alone
    assert seb.dev_runs_fold_workspace_size(0) == 128
    assert seb.dev_runs_fold_plan([], [], [], None) == (0,) * 8
    ko, vo = Guarded(torch, 1, np.uint64), Guarded(torch, 1, np.uint64)
    seb.dev_runs_fold_emit([], [], [], (0,) * 8, None, None, ko.view, None, vo.view, None)
    assert ko.host()[0] == 0 and vo.host()[0] == 0


def test_fold_with_a_stale_index_stays_in_bounds(seb, torch_cuda):
    """Another run's index, an all-ones and an all-zero index: the fold is wrong at most; every output stays inside
    the sizes its plan returned (the guards), and nothing faults."""
    torch = torch_cuda
    arrays = [sized_run(1000, seed=8, klen=24), sized_run(1300, seed=9, klen=24, step=2), sized_run(400, seed=10, klen=24, step=7)]
    runs = [upload_run(torch, seb, a)[0] for a in arrays]
    good = [build_index(torch, seb, r) for r in runs]
    other = build_index(torch, seb, upload_run(torch, seb, sized_run(1300, seed=11, klen=24, step=5))[0])
    for ix1 in (other, torch.full_like(good[1], 0xFF), torch.zeros_like(good[1])):
        device_fold(torch, seb, arrays, indexes=[good[0], ix1, good[2]], check=False)
    device_fold(torch, seb, arrays, indexes=[torch.zeros_like(g) for g in good], check=False)


# ------------------------------------------------------------------ end to end

def test_three_batches_to_a_file_image_on_the_device(seb, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(77)
    lsm = wref.LSM(sequence=(1 << 32) + 100)
    runs, vals, indexes, tables = [], [], [], []
    for b in range(3):
        ops = wref.random_ops(rng, 1200, max_key=40, max_val=60) + (wref.edge_ops() if b == 1 else [])
        seq0 = lsm.sequence + 1
        lsm.apply(ops)
        n = len(ops)
        dk, _, dvals, dvoff, ddel = upload_ops(torch, seb, wref.op_arrays(ops, 5, 9))
        rec = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        total = seb.dev_wal_frame_plan(dk, dvoff, ddel, rec)
        img = torch.zeros(total + 1, dtype=torch.uint8, device="cuda")[1:]
        seb.dev_wal_frame_emit(dk, dvals, dvoff, ddel, seq0, rec, img)
        ws = torch.zeros(seb.dev_wal_replay_workspace_size(n), dtype=torch.uint8, device="cuda")
        sizes = seb.dev_wal_replay_plan(img, rec, ws)
        _, n_out, kb, vb = sizes[:4]
        keys = torch.zeros(max(kb, 1), dtype=torch.uint8, device="cuda")
        v = torch.zeros(max(vb, 1), dtype=torch.uint8, device="cuda")
        koff, voff = (torch.zeros(n_out + 1, dtype=torch.int64, device="cuda") for _ in range(2))
        dele = torch.zeros(n_out, dtype=torch.uint8, device="cuda")
        seq = torch.zeros(n_out, dtype=torch.int64, device="cuda")
        seb.dev_wal_replay_emit(img, rec, sizes, ws, keys, koff, v, voff, dele, seq)
        run = seb.dev_run(keys, koff, voff, dele, seq, key_bytes=kb)  # the replay's arrays as they are
        runs.insert(0, run), vals.insert(0, v), indexes.insert(0, build_index(torch, seb, run))
        tables.insert(0, mref.recover(mref.read_all(bytes(img.cpu().numpy())))[0])
    # the batched Get sees the latest write of each key
    probes = sorted(lsm.mt.keys) + [b"never-written"]
    off = np.cumsum([0] + [len(p) for p in probes]).astype(np.uint64)
    dk = seb.dev_keys(odd_view(torch, np.frombuffer(b"".join(probes), np.uint8)), u64_dev(torch, off))
    st = torch.zeros(len(probes), dtype=torch.uint8, device="cuda")
    rr = torch.zeros(len(probes), dtype=torch.uint8, device="cuda")
    sq = torch.zeros(len(probes), dtype=torch.int64, device="cuda")
    seb.dev_runs_search(dk, runs, indexes, st, run=rr, seq=sq)
    torch.cuda.synchronize()
    want = gref.expected(tables, probes)
    assert np.array_equal(st.cpu().numpy(), want[0]) and np.array_equal(rr.cpu().numpy(), want[1])
    assert np.array_equal(sq.cpu().numpy().view(np.uint64), want[5])
    assert [int(s) for s in want[5][:-1]] == [e[2] for e in lsm.mt.entries]  # the memtable's own sequences
    # fold, then the builder
    total = sum(r.n for r in runs)
    fws = torch.zeros(seb.dev_runs_fold_workspace_size(total), dtype=torch.uint8, device="cuda")
    vb_in = [int(v.numel()) for v in vals]
    fs = seb.dev_runs_fold_plan(runs, indexes, vb_in, fws)
    assert fs == wref.fold_sizes(tables) and fs[7] == lsm.mt.size and fs[6] == lsm.sequence
    _, n_out, kb, vb = fs[:4]
    fkeys = torch.zeros(kb, dtype=torch.uint8, device="cuda")
    fvals = torch.zeros(max(vb, 1), dtype=torch.uint8, device="cuda")
    fkoff, fvoff = (torch.zeros(n_out + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    fdel = torch.zeros(n_out, dtype=torch.uint8, device="cuda")
    fseq = torch.zeros(n_out, dtype=torch.int64, device="cuda")
    seb.dev_runs_fold_emit(runs, indexes, vals, fs, fws, fkeys, fkoff, fvals, fvoff, fdel, fseq, val_bytes=vb_in)
    torch.cuda.synchronize()
    got = mref.unpack(fkeys.cpu().numpy(), fkoff.cpu().numpy(), fvals.cpu().numpy(), fvoff.cpu().numpy(), fdel.cpu().numpy(),
                      fseq.cpu().numpy().view(np.uint64))
    assert got == wref.entries_of(lsm.mt)  # GetAllEntries()
    fk = seb.dev_keys(fkeys, fkoff)
    sws = torch.zeros(seb.dev_sst_workspace_size(n_out, 1), dtype=torch.uint8, device="cuda")
    ss = seb.dev_sst_plan(fk, fvoff, [0, n_out], sws)
    data = torch.zeros(ss[0][1], dtype=torch.uint8, device="cuda")
    index = torch.zeros(ss[0][2], dtype=torch.uint8, device="cuda")
    meta = torch.zeros(ss[0][3], dtype=torch.uint8, device="cuda")
    seb.dev_sst_encode(fk, fvals, fvoff, fdel, [0, n_out], ss, sws, data, index, meta)
    torch.cuda.synchronize()
    h = gref.run_arrays(lsm.mt)  # the host path for the MemTable's GetAllEntries()
    hd, hi, hm = seb.sst_encode((h[0], h[1]), h[2], h[3], h[4])
    assert data.cpu().numpy().tobytes() == hd and index.cpu().numpy().tobytes() == hi and meta.cpu().numpy().tobytes() == hm


def test_context_forms(seb, torch_cuda):
    rng = np.random.default_rng(88)
    lsm = wref.LSM(sequence=40)
    ctx = seb.Ctx()
    try:
        active, total = [], 0  # the batches' runs, newest first
        for b in range(3):
            ops = wref.random_ops(rng, 800) + (wref.edge_ops() if b == 1 else [])
            keys, koff, vals, voff, dele = wref.op_arrays(ops, 5, 9, 255)
            seq0 = lsm.sequence + 1
            want_img, _, want_delta = lsm.apply(ops)
            hruns = [seb.host_run(a[0], a[1], a[3], a[4], a[5]) for a in active]
            image, run, delta, seq_after = ctx.memtable_apply((keys, koff), vals, voff, dele, seq0, hruns)
            assert image.tobytes() == want_img and delta == want_delta and seq_after == lsm.sequence
            want_run = seb.wal_replay_emit(*seb.wal_frame((keys, koff), vals, voff, dele, seq0))
            assert run[6] == want_run[6] and all(np.array_equal(x, y) for x, y in zip(run[:6], want_run[:6]))
            total += delta
            active.insert(0, run)
        assert total == lsm.mt.size
        got = ctx.memtable_fold([seb.host_run(a[0], a[1], a[3], a[4], a[5]) for a in active], [a[2] for a in active])
        assert mref.unpack(*got[:6]) == wref.entries_of(lsm.mt) and got[6][7] == lsm.mt.size
        # fixed-stride keys and no deleted array, onto the three runs
        fk = np.frombuffer(b"".join(key_of(i * 7 % 500) for i in range(600)), np.uint8).reshape(-1, 16)
        fv, fvo = rng.integers(0, 256, 9 + 600 * 4, dtype=np.uint8), 9 + np.arange(601, dtype=np.uint64) * np.uint64(4)
        hruns = [seb.host_run(a[0], a[1], a[3], a[4], a[5]) for a in active]
        image, run, delta, seq_after = ctx.memtable_apply(fk, fv, fvo, None, 1 << 40, hruns)
        want_fimg, want_foff = seb.wal_frame(fk, fv, fvo, None, 1 << 40)
        want_frun = seb.wal_replay_emit(want_fimg, want_foff)
        assert np.array_equal(image, want_fimg) and run[6] == want_frun[6] and seq_after == (1 << 40) + 599
        assert all(np.array_equal(x, y) for x, y in zip(run[:6], want_frun[:6]))
        assert delta == seb.run_size_delta(seb.host_run(*[want_frun[j] for j in (0, 1, 3, 4, 5)]), hruns)
        # an empty batch, fixed capacities that are too small, and a bad existing run
        image, run, delta, seq_after = ctx.memtable_apply([], b"", [0], None, 7, [])
        assert image.size == 0 and run[6] == (0,) * 8 and delta == 0 and seq_after == 6
        with pytest.raises(seb.SebError) as ei:
            ctx.memtable_apply((keys, koff), vals, voff, dele, 1, [], caps=(10, 10, 10, 10))
        assert ei.value.code == -4 and ei.value.image_bytes == len(want_img) and ei.value.sizes[:6] == want_run[6][:6]
        with pytest.raises(seb.SebError) as ei:
            ctx.memtable_fold([seb.host_run(a[0], a[1], a[3], a[4], a[5]) for a in active], [a[2] for a in active], caps=(1, 1, 1))
        assert ei.value.code == -4 and ei.value.sizes == got[6]
        bad = seb.host_run(np.frombuffer(b"acba", np.uint8), np.arange(5, dtype=np.uint64), np.zeros(5, np.uint64),
                           np.zeros(4, np.uint8), None)
        with pytest.raises(seb.SebError) as ei:
            ctx.memtable_apply((keys, koff), vals, voff, dele, 1, [seb.host_run(*[active[0][j] for j in (0, 1, 3, 4, 5)]), bad])
        assert ei.value.code == -1 and "run 1: entry 2 " in str(ei.value)
    finally:
        ctx.close()
