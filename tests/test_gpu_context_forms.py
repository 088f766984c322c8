"""GPU: the nine host-buffer forms on a context (seb_search_blocks, seb_sst_build, seb_merge, seb_wal_recover,
seb_memtable_get, seb_memtable_apply, seb_memtable_fold, seb_hidx_recover, seb_hidx_compact), which stage their
arrays through one carver over the context's grow-only buffers (csrc/seb_stage.h).

Buffer reuse: one context, every form called large / one entry / empty / large again, each answer against the host
half.  A size or an offset of the large call that survived in a buffer would show in the small calls behind it, a
buffer that shrank in the last one.  The large shapes have about 3000 entries (more than one tile of every kernel
involved), an odd entry count and key and value byte totals that are no multiples of 16, so every section ends off
an alignment boundary; key and value offsets start above 0.

Optional outputs: each nullable output left out in turn and all at once, through the C ABI; the return code is
SEB_OK, the outputs that were passed equal the full call's, and every host array sits in a larger buffer of 0xA5
whose bytes outside the stated capacity stay untouched.  300 keys, two runs or blocks' worth of two chunks
(SEB_CHUNK_BYTES = 4096: 256 16-byte keys a chunk)."""
import ctypes as C

import numpy as np
import pytest

import block_ref as br
import hashindex_ref as href
import hashwrite_ref as hwref
import keygen as kg
import memtable_ref as mref
import memwrite_ref as wref
import merge_ref as mr
import sstable_ref as sr
import stream_late as sl

pytestmark = pytest.mark.gpu

TS = 1_777_000_123
NO_ID = 2**32 - 1
ORDER = (0, 1, 2, 0)  # large, one entry, empty, large again
RUN_NAMES = ("keys", "key_off", "vals", "val_off", "deleted", "seq")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def same_arrays(got, want, names, what):
    assert len(got) == len(want), what
    for g, w, name in zip(got, want, names):
        assert np.array_equal(np.asarray(g), np.asarray(w)), f"{what}: {name} differs"


def off_alignment(n, key_bytes, val_bytes):
    return n % 2 == 1 and key_bytes % 16 != 0 and val_bytes % 16 != 0


def first_off_alignment(make, sizes_of, seed):
    """make(seed) for the first seed from `seed` on whose answer has an odd entry count and byte totals off 16."""
    while True:
        case = make(seed)
        if off_alignment(*sizes_of(case)[1:4]):
            return case
        seed += 1


def host_run_of(seb, run):
    """host_run over a run's (keys, key_off, vals, val_off, deleted, seq, ...)."""
    return seb.host_run(run[0], run[1], run[3], run[4], run[5])


# ------------------------------------------------------------------ the shapes and the host half's answers

def block_table(n_items, seed):
    """The blocks of a file of 16-byte keys 3 * i, and two slots that hold no whole block."""
    rng = np.random.default_rng(seed)
    items = [(kg.key16_bytes(3 * i), bytes(rng.integers(0, 256, int(rng.integers(0, 120)), dtype=np.uint8)), i % 9 == 4)
             for i in range(n_items)]
    image, index = br.build_sstable(items)
    return [image[o:o + 4096] for _, o in index] + [image[:1000], b""]


def search_shape(seb, images, n, cap, seed, top=3 * 1500 + 20):
    """n probes (one in five of another length than 16) against (n, cap) block ids: the arguments and the rows."""
    rng = np.random.default_rng(seed)
    nb = len(images)
    ids = np.array(list(range(nb)) * 3 + [NO_ID] * 4 + [nb, 2**31], np.uint32)
    probes = [kg.key16_bytes(int(i)) if j % 5 else bytes(rng.integers(0, 256, int(rng.integers(0, 25)), dtype=np.uint8))
              for j, i in enumerate(rng.integers(0, top, n))]
    bid = ids[rng.integers(0, len(ids), (n, cap))].reshape(n, cap)
    off = np.cumsum([3] + [len(p) for p in probes]).astype(np.uint64)
    data = np.frombuffer(b"\xee" * 3 + b"".join(probes), np.uint8)
    memo, cells, rows = {}, np.zeros((n, cap), np.uint32), []
    for i, key in enumerate(probes):
        for j, b in enumerate(bid[i].tolist()):
            if b < nb:
                if (b, key) not in memo:
                    memo[(b, key)] = seb.block_search(images[b], key)
                cells[i, j] = memo[(b, key)]
        st, wc, c = br.lsm_get_ref(cells[i].tolist())
        found = st == br.GET_FOUND
        rows.append((st, wc, int(bid[i, wc]) * 4096 + ((c >> 13) & 0x1FFF) if found else 0, c & 0x1FFF if found else 0))
    rows = np.array(rows, np.uint64).reshape(n, 4)
    want = (rows[:, 0].astype(np.uint8), rows[:, 1].astype(np.uint16), rows[:, 2], rows[:, 3].astype(np.uint32), cells)
    return dict(keys=(data, off), bid=bid, want=want)


def sst_items(seed):
    """About 3000 sorted items, cut back until the count is odd and both byte totals are off a multiple of 16."""
    items = sr.random_items(np.random.default_rng(seed), 3050)
    while not off_alignment(len(items), sum(len(k) for k, _, _ in items), sum(len(v) for _, v, _ in items)):
        items.pop()
    return items


def key15(i):
    return b"%015d" % i


def lookup_run(n, seed, step):
    """n entries with the 15-byte keys step * i: values of 0..40 bytes, every 7th entry deleted, sequences out of order;
    3 and 5 bytes in front of the keys and the values."""
    rng = np.random.default_rng(seed)
    keys = np.frombuffer(b"\xee" * 3 + b"".join(key15(step * i) for i in range(n)), np.uint8)
    koff = 3 + np.arange(n + 1, dtype=np.uint64) * np.uint64(15)
    dele = (np.arange(n) % 7 == 3).astype(np.uint8)
    voff = (5 + np.concatenate([[0], np.cumsum(np.where(dele == 1, 0, rng.integers(0, 41, n)))])).astype(np.uint64)
    return keys, koff, np.zeros(int(voff[-1]), np.uint8), voff, dele, rng.integers(1, 1 << 50, n).astype(np.uint64)


def lookup_shape(seb, sizes, count, seed):
    runs = [lookup_run(n, seed + r, 2 + r) for r, n in enumerate(sizes)]
    rng = np.random.default_rng(seed + 100)
    probes = [key15(int(i)) for i in rng.integers(0, 2 * max(sizes + [2]) + 2, count)]
    off = 3 + np.arange(count + 1, dtype=np.uint64) * np.uint64(15)
    keys = (np.frombuffer(b"\xee" * 3 + b"".join(probes), np.uint8), off)
    hruns = [host_run_of(seb, a) for a in runs]
    return dict(keys=keys, runs=runs, want=seb.runs_search(keys, hruns))


def store_of(records, segments, seed, flip_last=True):
    """`records` Put / Delete records over fewer keys in `segments` segment images; a flipped bit in the last one."""
    rng = np.random.default_rng(seed)
    per, out = (records + segments - 1) // segments, []
    for s in range(segments):
        w = href.Writer(1000 * s + 1)
        for i in range(s * per, min((s + 1) * per, records)):
            key = b"key-%05d" % int(rng.integers(0, max(records // 2, 1))) + b"x" * int(rng.integers(0, 9))
            w.put(key, b"" if rng.random() < 0.1 else bytes(rng.integers(0, 256, int(rng.integers(1, 90)), dtype=np.uint8)))
        out.append(href.flip(w.bytes(), w.offsets[len(w.offsets) // 2] + 3, 2) if flip_last and s == segments - 1 else w.bytes())
    return out


@pytest.fixture(scope="module")
def shapes(seb):
    """Per form its three shapes (large, one entry, empty) with the host half's answer, computed once."""
    out = {}
    images = block_table(1500, 3)
    assert 24 <= len(images) <= 60
    pool = np.full((len(images), br.BLOCK), 0xA5, np.uint8)
    for b, img in enumerate(images):
        pool[b, :len(img)] = np.frombuffer(img, np.uint8)
    out["search"] = dict(pool=pool, blen=np.array([len(i) for i in images], np.uint16),
                         cases=[search_shape(seb, images, n, 3, 7 + n) for n in (3001, 1, 0)])

    out["sst"] = []
    for items in (sst_items(12), [(b"k", b"v", 0)], []):
        kd, koff, vd, voff, dl = sr.pack(items, key_pad=1, val_pad=2)
        out["sst"].append(dict(args=((kd, koff), vd, voff, dl), want=sr.build_file(items)))

    def merge_case(runs):
        pool_m, blen_m, rb = mr.pool_of([mr.run_blocks(r) for r in runs], fill=0xCC)
        return dict(args=(pool_m, blen_m, rb), want=seb.merge_emit(pool_m, blen_m, rb))

    def replay_case(n, seed):
        image, off = mref.wal_image(mref.random_log(np.random.default_rng(seed), n, max_key=40, max_val=60))
        return dict(image=bytes(image), want=seb.wal_replay_emit(image, off))

    out["merge"] = [first_off_alignment(lambda seed: merge_case(mr.random_runs(np.random.default_rng(seed), 3, 3000, share=0.25)),
                                        lambda case: case["want"][5], 21), merge_case([[(b"k", b"v", 0)]]), merge_case([])]
    assert len(out["merge"][0]["args"][1]) >= 24
    out["replay"] = [first_off_alignment(lambda seed: replay_case(3001, seed), lambda case: case["want"][6], 30), replay_case(1, 31),
                     replay_case(0, 32)]

    out["memget"] = [lookup_shape(seb, [2001, 1000, 0], 3001, 40), lookup_shape(seb, [1], 1, 41), lookup_shape(seb, [], 0, 42)]
    assert 2001 % 2 and (2001 * 15) % 16 and 3001 % 2

    # the write side: four batches in turn, each onto the runs of the batches before it, newest first
    def big_batch(seed):
        return wref.op_arrays(wref.random_ops(np.random.default_rng(seed), 3000) + wref.edge_ops(), 5, 9, 255)

    def batch_sizes(arrays):
        return None, len(arrays[4]), int(arrays[1][-1]) - 5, int(arrays[3][-1]) - 9

    batches = [first_off_alignment(big_batch, batch_sizes, 50), wref.op_arrays([(b"one", b"entry", 0)], 5, 9, 255),
               wref.op_arrays([], 5, 9, 255), first_off_alignment(big_batch, batch_sizes, 150)]
    out["apply"], active, seq0 = [], [], 41
    for keys, koff, vals, voff, dele in batches:
        ops = dele
        image, rec_off = seb.wal_frame((keys, koff), vals, voff, dele, seq0)
        run = seb.wal_replay_emit(image, rec_off)
        hruns = [host_run_of(seb, a) for a in active]
        delta = seb.run_size_delta(host_run_of(seb, run), hruns) if len(ops) else 0
        out["apply"].append(dict(args=((keys, koff), vals, voff, dele, seq0), prior=list(active), image=image, run=run,
                                 delta=delta, seq_after=seq0 - 1 + len(ops)))
        seq0 += len(ops)
        if len(ops):
            active.insert(0, run)
    big2, one, big1 = active
    out["fold"] = []
    for runs in ([big2, one, big1], [one], []):
        hruns, vals = [host_run_of(seb, a) for a in runs], [a[2] for a in runs]
        out["fold"].append(dict(runs=runs, want=seb.runs_fold(hruns, vals)))
    _, n_out, kb, vb = out["fold"][0]["want"][6][:4]
    assert n_out > 1024 and (n_out % 2 or kb % 16 or vb % 16)

    out["hidx"] = []
    for segments, c in ((store_of(3001, 3, 60), 2), (store_of(1, 1, 61, flip_last=False), 1), ([b""], 1)):
        image, rec_off, sizes = seb.segs_compact(segments, c, TS)
        out["hidx"].append(dict(segments=segments, c=c, rec=href.recover(segments), image=image, rec_off=rec_off, sizes=sizes,
                                drop=hwref.count_drop(segments, c)))
    assert sum(len(s) for s in out["hidx"][0]["segments"]) % 16 and out["hidx"][0]["rec"]["cut"][2]
    return out


# ------------------------------------------------------------------ A1: buffer reuse

def test_forms_reuse_their_buffers(seb, torch_cuda, shapes):
    ctx = seb.Ctx(0)
    try:
        for turn, j in enumerate(ORDER):
            what = f"call {turn} (shape {j})"
            s = shapes["search"]
            case = s["cases"][j]
            got = ctx.search_blocks(case["keys"], case["bid"], s["pool"], s["blen"], want_cells=True)
            same_arrays(got, case["want"], ("status", "col", "vloc", "vlen", "cells"), f"search_blocks, {what}")

            case = shapes["sst"][j]
            got = ctx.sst_build(*case["args"])
            assert len(got) == len(case["want"]) and got == case["want"], f"sst_build, {what}"

            case = shapes["merge"][j]
            got = ctx.merge(*case["args"])
            assert got[5] == case["want"][5], f"merge, {what}: sizes"
            same_arrays(got[:5], case["want"][:5], RUN_NAMES, f"merge, {what}")

            case = shapes["replay"][j]
            got = ctx.wal_recover(case["image"])
            assert got[6] == case["want"][6], f"wal_recover, {what}: sizes"
            same_arrays(got[:6], case["want"][:6], RUN_NAMES, f"wal_recover, {what}")

            case = shapes["memget"][j]
            got = ctx.memtable_get(case["keys"], [host_run_of(seb, a) for a in case["runs"]])
            same_arrays(got, case["want"], ("status", "run", "entry", "vloc", "vlen", "seq"), f"memtable_get, {what}")

            case = shapes["fold"][j]
            got = ctx.memtable_fold([host_run_of(seb, a) for a in case["runs"]], [a[2] for a in case["runs"]])
            assert got[6] == case["want"][6], f"memtable_fold, {what}: sizes"
            same_arrays(got[:6], case["want"][:6], RUN_NAMES, f"memtable_fold, {what}")
        # the write batches are large, one entry, empty, large again by themselves: each onto the runs before it
        for turn, case in enumerate(shapes["apply"]):
            what = f"memtable_apply, batch {turn}"
            image, run, delta, seq_after = ctx.memtable_apply(*case["args"], [host_run_of(seb, a) for a in case["prior"]])
            assert np.array_equal(image, case["image"]), f"{what}: image"
            assert run[6] == case["run"][6] and (delta, seq_after) == (case["delta"], case["seq_after"]), what
            same_arrays(run[:6], case["run"][:6], RUN_NAMES, what)
        assert seb.fallback_count() == 0
    finally:
        ctx.close()


def test_hash_index_forms_reuse_their_buffer(seb, torch_cuda, shapes):
    """HashIndex.recover (seb_hidx_recover on the index's context), seb_hidx_compact on the same context and
    HashIndex.compact, over one index: large, one record, an empty segment, large again."""
    torch = torch_cuda
    hx = seb.HashIndex()
    try:
        for turn, j in enumerate(ORDER):
            case = shapes["hidx"][j]
            segments, c, rec, what = case["segments"], case["c"], case["rec"], f"call {turn} (shape {j})"
            got = hx.recover(segments)
            for k in ("valid", "size_after", "short_tail", "cut"):
                assert list(got[k]) == rec[k], (what, k)
            assert got["live_records"] == rec["live_records"] and got["distinct"] == len(rec["index"]) == hx.count, what
            # seb_hidx_compact: the pool recover filled, the host half's offsets and live bytes of the segments that stay
            pool, rec_off, first, base, size, _ = seb.segs_scan(segments)
            live = seb.seg_verify(pool, rec_off, first, base, size)[3]
            after = seb.segs_scan([case["image"].tobytes()] + list(segments[c:]))[0]
            n_head = int(first[c])
            rest_n = rec_off.size - n_head
            capacity = max(int(live.sum()), 1)
            table = sl.Out(torch, seb.dev_hidx_table_bytes(capacity), np.uint8)
            dst = sl.Out(torch, after.size, np.uint8)
            new_off = sl.Out(torch, case["sizes"]["survivors"] + rest_n + 1, np.uint64)
            done = hx._ctx.hidx_compact(hx.pool, pool.size, base, size, c, sl.to_dev(torch, rec_off[n_head:]) if rest_n else None,
                                        sl.to_dev(torch, live[n_head:]) if rest_n else None, rest_n, TS,
                                        dst.t if after.size else None, table.t, capacity, new_off.t)
            torch.cuda.synchronize()
            assert done["sizes"] == case["sizes"] and done["pool_bytes"] == after.size, what
            assert done["distinct"] == len(rec["index"]) - case["drop"], what
            sl.same(dst.get("the new pool"), after, f"{what}: the new pool")
            edge = int(base[c]) if c < len(segments) else pool.size
            rest_want = rec_off[n_head:].astype(np.int64) - edge + case["image"].size
            sl.same(new_off.get("new_rec_off"),
                    np.concatenate([case["rec_off"][:-1].astype(np.int64), rest_want, [after.size]]).astype(np.uint64), f"{what}: new_rec_off")
            table.get("table")
            count = hx.count
            assert hx.compact(c, TS) == case["sizes"] and count - hx.count == case["drop"], what
            sl.same(hx.pool[: hx.pool_bytes].cpu().numpy(), after, f"{what}: HashIndex.compact's pool")
        assert seb.fallback_count() == 0
    finally:
        hx.close()


# ------------------------------------------------------------------ A2: optional outputs left out

class Framed:
    """A host output of `count` elements inside a larger buffer of 0xA5: the bytes around it must stay."""

    def __init__(self, count, dtype, slack=64):
        self.nbytes, self.slack = count * np.dtype(dtype).itemsize, slack
        self.buf = np.full(slack + self.nbytes + slack, 0xA5, np.uint8)
        self.a = self.buf[slack:slack + self.nbytes].view(dtype)
        self.ptr = self.a.ctypes.data

    def get(self, what):
        assert (self.buf[:self.slack] == 0xA5).all() and (self.buf[self.slack + self.nbytes:] == 0xA5).all(), \
            f"{what}: bytes outside the stated capacity were written"
        return self.a


def run_frames(sizes, with_seq):
    """Exact-capacity frames for a sorted run of these sizes: (frames, the C arguments from keys to entry_cap)."""
    n_out, kb, vb = sizes[1:4]
    f = [Framed(kb, np.uint8), Framed(n_out + 1, np.uint64), Framed(vb, np.uint8), Framed(n_out + 1, np.uint64),
         Framed(n_out, np.uint8), Framed(n_out, np.uint64)]
    args = [f[0].ptr, kb, f[1].ptr, f[2].ptr, vb, f[3].ptr, f[4].ptr, f[5].ptr if with_seq else None, n_out]
    return f, args


def check_run(frames, want, with_seq, what):
    for j, name in enumerate(RUN_NAMES):
        if j == 5 and not with_seq:
            assert (frames[5].buf == 0xA5).all(), f"{what}: seq was left out and written"
        else:
            assert np.array_equal(frames[j].get(f"{what}: {name}"), want[j]), f"{what}: {name}"


@pytest.fixture()
def chunked_ctx(seb, monkeypatch):
    monkeypatch.setenv("SEB_CHUNK_BYTES", "4096")  # 256 16-byte keys a chunk: the 300 keys below take two
    ctx = seb.Ctx(0)
    yield ctx
    ctx.close()


def test_a_sorted_run_without_seq(seb, torch_cuda, chunked_ctx):
    recs = mref.random_log(np.random.default_rng(70), 300, max_key=40, max_val=60)
    image, off = mref.wal_image(recs)
    img = np.frombuffer(bytes(image), np.uint8)
    want = seb.wal_replay_emit(image, off)
    # the fold of that run under a newer one
    newer = seb.wal_replay_emit(*mref.wal_image(mref.random_log(np.random.default_rng(71), 200, max_key=40, max_val=60)))
    hruns, vals = [host_run_of(seb, a) for a in (newer, want)], [newer[2], want[2]]
    folded = seb.runs_fold(hruns, vals)
    arr, vp, vb, keep = seb._fold_host_args(hruns, vals)
    full = {}
    for with_seq in (True, False):
        frames, args = run_frames(want[6], with_seq)
        sz = seb.seb_replay_sizes()
        assert seb.lib().seb_wal_recover(chunked_ctx._p, img.ctypes.data, img.size, *args, C.byref(sz)) == 0, seb.last_error()
        assert sz.as_tuple() == want[6]
        check_run(frames, want, with_seq, "seb_wal_recover")
        full.setdefault("recover", [f.a.copy() for f in frames])
        assert all(np.array_equal(f.a, w) for f, w in zip(frames[:5], full["recover"])), "seq left out: not the full call's outputs"
        frames, args = run_frames(folded[6], with_seq)
        fz = seb.seb_fold_sizes()
        assert seb.lib().seb_memtable_fold(chunked_ctx._p, arr, vp, vb, 2, *args, C.byref(fz)) == 0, seb.last_error()
        assert fz.as_tuple() == folded[6]
        check_run(frames, folded, with_seq, "seb_memtable_fold")
        full.setdefault("fold", [f.a.copy() for f in frames])
        assert all(np.array_equal(f.a, w) for f, w in zip(frames[:5], full["fold"])), "seq left out: not the full call's outputs"


def left_out(call, outputs, omits, want):
    """call(pointer or None per output) once with every output, then with each of `omits` left out: SEB_OK, the
    outputs passed equal the full call's (and the host half's), nothing outside a capacity or in an output left out."""
    full = None
    for omit in ((),) + tuple(omits):
        frames = [Framed(count, t) for _, t, count in outputs]
        call([None if j in omit else f.ptr for j, f in enumerate(frames)])
        got = [None if j in omit else f.get(name) for j, (f, (name, _, _)) in enumerate(zip(frames, outputs))]
        full = got if full is None else full
        for j, (name, _, _) in enumerate(outputs):
            if j in omit:
                assert (frames[j].buf == 0xA5).all(), f"{name} was left out and written (without {omit})"
            else:
                assert np.array_equal(got[j], full[j]) and np.array_equal(got[j], np.asarray(want[j]).reshape(-1)), (name, omit)


def test_memtable_get_with_outputs_left_out(seb, torch_cuda, chunked_ctx):
    n = 300
    runs = [lookup_run(150, 80, 2), lookup_run(151, 81, 3)]
    keys = np.frombuffer(b"".join(key15(int(i)) for i in np.random.default_rng(82).integers(0, 460, n)), np.uint8).reshape(n, 15)
    hruns = [host_run_of(seb, a) for a in runs]
    want = seb.runs_search(keys, hruns)
    assert {0, 1} <= set(want[1].tolist()) and (want[0] == 0).any()
    kb = seb.as_keys(keys)

    def call(ptrs):
        assert seb.lib().seb_memtable_get(chunked_ctx._p, kb.ref, seb._run_array(hruns), 2, *ptrs) == 0, seb.last_error()

    outputs = [("status", np.uint8, n), ("run", np.uint8, n), ("entry", np.uint32, n), ("vloc", np.uint64, n), ("vlen", np.uint32, n),
               ("seq", np.uint64, n)]
    left_out(call, outputs, [(1,), (2,), (3,), (4,), (5,), (1, 2, 3, 4, 5)], want)


def test_search_blocks_with_outputs_left_out(seb, torch_cuda, chunked_ctx):
    n, cap = 300, 2
    images = block_table(60, 90)[:2]  # two blocks
    pool = np.full((2, br.BLOCK), 0xA5, np.uint8)
    for b, img in enumerate(images):
        pool[b, :len(img)] = np.frombuffer(img, np.uint8)
    blen = np.array([len(i) for i in images], np.uint16)
    case = search_shape(seb, images, n, cap, 91, top=200)
    keys = case["keys"]
    assert (case["want"][0] == br.GET_FOUND).any() and (case["want"][0] == br.GET_MISS).any()
    kb = seb.as_keys(keys)
    bid = np.ascontiguousarray(case["bid"])

    def call(ptrs):
        rc = seb.lib().seb_search_blocks(chunked_ctx._p, kb.ref, bid.ctypes.data, cap, pool.ctypes.data, blen.ctypes.data, 2, *ptrs)
        assert rc == 0, seb.last_error()

    outputs = [("status", np.uint8, n), ("col", np.uint16, n), ("vloc", np.uint64, n), ("vlen", np.uint32, n),
               ("cells", np.uint32, n * cap)]
    left_out(call, outputs, [(1,), (2,), (3,), (4,), (1, 2, 3, 4)], case["want"])
