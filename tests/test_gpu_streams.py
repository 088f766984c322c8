"""GPU: the device entry points on a side stream that is busy when they are called (include/seb_bloom.h: "work is
enqueued on `stream` and NOT synchronised"; the plan calls "SYNCHRONISE the stream").

Method (tests/stream_late.py): the inputs the library is pointed at hold a valid *poison* of the same sizes; on the
side stream S a delay is enqueued, then device-to-device copies that bring the good data, then the library calls.
After every non-synchronising call the test asserts that S has not left the delay yet.  Whatever the library issued
on another stream, read back too early or still needed from a caller's host array after returning sees the poison,
an unwritten output or a dead ctypes temporary, and the answer is wrong every time, not by chance.  Answers are
compared with the oracle, the Python restatements (*_ref.py) or the host half, never with a default-stream run, and
each case first checks on the CPU that the poison's answers differ from the good data's in every compared output.
A synchronising call must not return before S passed the delay (it would have synchronised another stream).

Three kinds of call whose results are not synchronised still wait for the stream by design and are checked like
plan calls: seb_dev_merge_emit, seb_dev_wal_replay_emit and seb_dev_runs_fold_emit (they read the workspace's header
back before they launch, as the header file says), the first registry call after put / remove (the rebuild is a
hipDeviceSynchronize), and a call that grows its stream's library scratch (the old buffer is freed after a
hipStreamSynchronize of that stream).

The positive control (fixture `rig`) accepts a stream only if a default-stream read made during S's delay sees the
poison; it tries up to 8 fresh streams and fails the module, never skips it, if none runs apart from the null stream.

Figures, on an MI355X with four hardware queues per process, this module run alone (so every kernel loads on its
first launch here):
  delay          50 ms per arm(), by torch.cuda._sleep (calibrated against events; it scales with its argument)
  enqueue time   at most 1.7 ms from arm() to the return of a chain's last call, over 52 checked calls, once the
                 library's code object is loaded.  With 20 ms the check failed twice: the first library launch of
                 the process took 43 ms (the fixture now makes one launch before the control) and a six-call chain
                 whose kernels each loaded on first launch took 20.1 ms.
  control        accepted the first stream tried (index 0)
  mutation       k_gjr_rows of launch_get_join_rows moved to stream 0 in a scratch build: both cases of
                 test_compact_plan_emit_and_join_rows fail with a wrong join status (only they and the control were
                 run against it)."""
import bisect
import struct

import numpy as np
import pytest

import block_ref as br
import getpath_ref as pref
import keygen as kg
import memget_ref as gref
import memtable_ref as tref
import memwrite_ref as wref
import merge_ref as mref
import sstable_ref as sref
import stream_late as sl
from oracle import bloom_np as bn
from oracle import codec_c as cc
from oracle import oracle_c as oc

pytestmark = pytest.mark.gpu

GUARD, FILL = sl.GUARD, sl.FILL
N = 2049  # two tiles of 1024 and one entry


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


@pytest.fixture(scope="module")
def rig(seb, torch_cuda):
    """The positive control, before any case: a side stream that demonstrably runs apart from the null stream."""
    try:
        r = sl.Rig(torch_cuda, seb)
    except AssertionError as e:
        pytest.fail(f"stream control: {e}")
    yield r
    print(f"\nstream_late: delay {sl.DELAY_MS} ms by {r.delay_kind}; control accepted stream index {r.stream_index}; "
          f"largest enqueue time {r.max_enqueue_ms:.3f} ms over {r.calls} calls")


def test_control_figures(rig):
    """The control ran (the fixture fails otherwise); the delay is within the bound the issue sets."""
    assert rig.stream_index < 8 and sl.DELAY_MS <= sl.MAX_DELAY_MS
    assert rig.stream.cuda_stream != 0, "the side stream is the null stream"


# ------------------------------------------------------------------ helpers

def words_of(seb, bits, m):
    """The oracle's bit array padded to the library's word array (seb_words_bytes), as int32."""
    w = np.zeros(max(seb.words_bytes(m), 16), np.uint8)
    w[: bits.size] = bits
    return w.view(np.int32)


def guarded(L, good, poison):
    """A late in/out buffer between guards: (whole tensor, the body's view in the arrays' own width)."""
    good, poison = np.ascontiguousarray(good), np.ascontiguousarray(poison)
    g = np.full(GUARD, FILL, np.uint8)
    t = L.inp(np.concatenate([g, good.view(np.uint8).reshape(-1), g]), np.concatenate([g, poison.view(np.uint8).reshape(-1), g]))
    body = t[GUARD: GUARD + good.nbytes]
    return t, body if good.dtype.itemsize == 1 else body.view(getattr(L.torch, sl._TORCH_OF[good.dtype.itemsize]))


def read_guarded(t, nbytes, dtype, name):
    h = t.cpu().numpy()
    assert (h[:GUARD] == FILL).all() and (h[GUARD + nbytes:] == FILL).all(), f"bytes outside {name} were written"
    return np.frombuffer(h[GUARD: GUARD + nbytes].tobytes(), dtype)


def key_sets(seed, n, n_build=None):
    """(build keys, good probes, poison probes): 16-byte keys; about half of either probe batch is in the build set,
    at different places."""
    rng = np.random.default_rng(seed)
    nb = n if n_build is None else n_build
    build = rng.integers(0, 256, (nb, 16), dtype=np.uint8)
    def probes():
        p = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        hit = rng.random(n) < 0.5
        p[hit] = build[rng.integers(0, nb, int(hit.sum()))]
        return p
    return build, probes(), probes()


def varlen_sets(seed, n):
    """Variable-length keys (0..40 bytes) over one offsets array: (offsets, build data, good probe data, poison)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 41, n)
    off = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    total = int(off[-1])
    build = rng.integers(0, 256, total, dtype=np.uint8)
    def probes():
        p = rng.integers(0, 256, total, dtype=np.uint8)
        for i in np.nonzero(rng.random(n) < 0.5)[0]:
            p[int(off[i]): int(off[i + 1])] = build[int(off[i]): int(off[i + 1])]
        return p
    return off, build, probes(), probes()


def packed_ref(keys, m):
    """seb_dev_pack_residues' word per key: r0 | b << 29 | carries << 58 (include/seb_bloom.h), in Python integers."""
    h1, h2 = bn.fnv_fixed(keys)
    out = np.zeros(len(keys), np.uint64)
    r0 = np.zeros(len(keys), np.uint64)
    b = np.zeros(len(keys), np.uint64)
    car = np.zeros(len(keys), np.uint64)
    for i, (a, d) in enumerate(zip((int(x) for x in h1), (int(x) for x in h2))):
        acc, c = a, 0
        for q in range(1, 7):
            acc += d
            if acc >= 1 << 64:
                acc -= 1 << 64
                c |= 1 << (q - 1)
        r0[i], b[i], car[i] = a % m, d % m, c
        out[i] = (a % m) | (d % m) << 29 | c << 58
    return out, r0, b, car


def unpack6(buf, n):
    blocks = buf[: -(-n // 64) * 384].reshape(-1, 384)
    lo = blocks[:, :256].copy().view("<u4").astype(np.uint64)
    hi = blocks[:, 256:].copy().view("<u2").astype(np.uint64)
    return (lo | (hi << np.uint64(32))).ravel()[:n]


# ------------------------------------------------------------------ 1. filter kernels, small filter

N1 = 5000


@pytest.fixture(scope="module")
def small(seb):
    m, k = seb.params(N1, 0.01)
    assert k == 7 and m < (1 << 21)
    build, good, poison = key_sets(11, N1)
    bits = oc.build(m, k, build, N1, stride=16)
    want = oc.probe(bits, m, k, good, N1, stride=16)
    want_p = oc.probe(bits, m, k, poison, N1, stride=16)
    sl.differ([want], [want_p])
    return dict(m=m, k=k, build=build, good=good, poison=poison, bits=bits, want=want)


def test_clear_and_build(seb, torch_cuda, rig, small):
    """seb_dev_clear alone, before seb_dev_build and before seb_dev_build_ws (both OR into the words), and
    seb_dev_build_fresh: the word arrays receive garbage by the late copy, so a clear issued elsewhere leaves it
    standing and a build issued elsewhere is wiped."""
    m, k = small["m"], small["k"]
    rng = np.random.default_rng(12)
    other = rng.integers(0, 256, (N1, 16), dtype=np.uint8)
    want = words_of(seb, oc.build(m, k, small["build"], N1, stride=16), m)
    sl.differ([want], [words_of(seb, oc.build(m, k, other, N1, stride=16), m)])
    nw = want.size
    L = rig.session()
    garbage, garbage2 = rng.integers(1, 2**31, nw).astype(np.int32), rng.integers(1, 2**31, nw).astype(np.int32)
    bufs = [guarded(L, garbage, garbage2) for _ in range(4)]
    dk = seb.dev_keys(L.inp(small["build"], other), n=N1, stride=16)
    need = seb.dev_build_workspace_size(N1, m, k)
    ws = torch_cuda.empty(max(need, 16), dtype=torch_cuda.uint8, device="cuda")
    L.arm()
    L.call(seb.dev_clear, bufs[0][1], m)
    L.call(seb.dev_clear, bufs[1][1], m)
    L.call(seb.dev_build, dk, bufs[1][1], m, k)
    L.call(seb.dev_build_fresh, dk, bufs[2][1], m, k)
    L.call(seb.dev_clear, bufs[3][1], m)
    L.call(seb.dev_build_ws, dk, bufs[3][1], m, k, ws if need else None)
    L.finish()
    sl.same(read_guarded(bufs[0][0], 4 * nw, np.int32, "words"), np.zeros(nw, np.int32), "dev_clear")
    sl.same(read_guarded(bufs[1][0], 4 * nw, np.int32, "words"), want, "dev_clear + dev_build")
    sl.same(read_guarded(bufs[2][0], 4 * nw, np.int32, "words"), want, "dev_build_fresh")
    sl.same(read_guarded(bufs[3][0], 4 * nw, np.int32, "words"), want, "dev_clear + dev_build_ws")


def test_probe_and_packed_forms(seb, torch_cuda, rig, small):
    """seb_dev_probe; seb_dev_pack_residues -> seb_dev_probe_packed; seb_dev_probe_emit_packed."""
    m, k, want = small["m"], small["k"], small["want"]
    wp, _, _, _ = packed_ref(small["good"], m)
    sl.differ([wp], [packed_ref(small["poison"], m)[0]])
    L = rig.session()
    words = sl.to_dev(torch_cuda, words_of(seb, small["bits"], m))
    dk = seb.dev_keys(L.inp(small["good"], small["poison"]), n=N1, stride=16)
    out, packed, out2, out3, packed3 = L.out(N1, np.uint8), L.out(N1, np.uint64), L.out(N1, np.uint8), L.out(N1, np.uint8), L.out(N1, np.uint64)
    L.arm()
    L.call(seb.dev_probe, dk, words, m, k, out.t)
    L.call(seb.dev_pack_residues, dk, m, k, packed.t)
    L.call(seb.dev_probe_packed, packed.t, N1, words, m, k, out2.t)
    L.call(seb.dev_probe_emit_packed, dk, words, m, k, out3.t, packed3.t)
    L.finish()
    sl.same(out.get(), want, "dev_probe")
    sl.same(packed.get(), wp, "dev_pack_residues")
    sl.same(out2.get(), want, "dev_probe_packed")
    sl.same(out3.get(), want, "dev_probe_emit_packed: answers")
    sl.same(packed3.get(), wp, "dev_probe_emit_packed: packed")


def test_variable_length_build_and_probe(seb, torch_cuda, rig):
    """A variable-length batch through the pre-hash path (varlen_prehash_min_keys 0): build and probe."""
    off, build, good, poison = varlen_sets(13, N1)
    m, k = oc.params(N1, 0.01)
    bits = oc.build(m, k, build, N1, offsets=off)
    rng = np.random.default_rng(14)
    other = rng.integers(0, 256, build.size, dtype=np.uint8)
    want = oc.probe(bits, m, k, good, N1, offsets=off)
    sl.differ([want, bits], [oc.probe(bits, m, k, poison, N1, offsets=off), oc.build(m, k, other, N1, offsets=off)])
    L = rig.session()
    doff = sl.to_dev(torch_cuda, off)
    words = sl.to_dev(torch_cuda, words_of(seb, bits, m))
    bk = seb.dev_keys(L.inp(build, other), doff)
    pk = seb.dev_keys(L.inp(good, poison), doff)
    nw = words.numel()
    built, built_view = guarded(L, np.zeros(nw, np.int32), np.full(nw, 0x01010101, np.int32))
    out = L.out(N1, np.uint8)
    with seb.option("varlen_prehash_min_keys", 0):
        L.arm()
        L.call(seb.dev_build, bk, built_view, m, k)
        L.call(seb.dev_probe, pk, words, m, k, out.t)
        L.finish()
    sl.same(read_guarded(built, 4 * nw, np.int32, "words"), words_of(seb, bits, m), "dev_build (offsets)")
    sl.same(out.get(), want, "dev_probe (offsets)")


def test_multi_filter_forms(seb, torch_cuda, rig):
    """seb_dev_build_many, seb_dev_probe_multi, seb_dev_probe_multi_packed and seb_dev_pack_residues6 ->
    seb_dev_probe_multi_packed6 over three filters of one (m, k).  The filter lists and key_begin are host arrays
    that die with the wrapper's frame."""
    nf, per = 3, 1700
    m, k = oc.params(per, 0.01)
    assert k == 7 and m < (1 << 21)
    build, good, poison = key_sets(15, N1, nf * per)
    rng = np.random.default_rng(16)
    other = rng.integers(0, 256, (nf * per, 16), dtype=np.uint8)
    begin = [0, 1500, 3300, nf * per]  # uneven files
    fbits = [oc.build(m, k, build[begin[f]: begin[f + 1]], begin[f + 1] - begin[f], stride=16) for f in range(nf)]
    obits = [oc.build(m, k, other[begin[f]: begin[f + 1]], begin[f + 1] - begin[f], stride=16) for f in range(nf)]
    host = [(b, m, k) for b in fbits]
    want = oc.probe_multi(host, good, N1, stride=16)
    sl.differ([want] + fbits, [oc.probe_multi(host, poison, N1, stride=16)] + obits)
    wp, r0, b, car = packed_ref(good, m)
    w6 = r0 | b << np.uint64(21) | car << np.uint64(42)
    L = rig.session()
    filters = [(sl.to_dev(torch_cuda, words_of(seb, fb, m)), m, k) for fb in fbits]
    nw = filters[0][0].numel()
    built = [guarded(L, np.zeros(nw, np.int32), np.full(nw, 0x01010101, np.int32)) for _ in range(nf)]
    bk = seb.dev_keys(L.inp(build, other), n=nf * per, stride=16)
    pk = seb.dev_keys(L.inp(good, poison), n=N1, stride=16)
    mask8, mask16, mask64 = L.out(N1, np.uint8), L.out(N1, np.uint16), L.out(N1, np.uint64)
    packed, packed6 = L.out(N1, np.uint64), L.out(seb.packed6_bytes(N1), np.uint8)
    L.arm()
    L.call(seb.dev_build_many, bk, begin, [(v, m, k) for _, v in built])
    # the widest masks first: the interleaved table in the stream's scratch never has to grow (a grow synchronises)
    L.call(seb.dev_pack_residues6, pk, m, k, packed6.t)
    L.call(seb.dev_probe_multi_packed6, packed6.t, N1, filters, mask64.t)
    L.call(seb.dev_pack_residues, pk, m, k, packed.t)
    L.call(seb.dev_probe_multi_packed, packed.t, N1, filters, mask16.t)
    L.call(seb.dev_probe_multi, pk, filters, mask8.t)
    L.finish()
    for f in range(nf):
        sl.same(read_guarded(built[f][0], 4 * nw, np.int32, "words"), words_of(seb, fbits[f], m), f"dev_build_many: filter {f}")
    sl.same(mask8.get().astype(np.uint64), want, "dev_probe_multi")
    sl.same(packed.get(), wp, "dev_pack_residues")
    sl.same(mask16.get().astype(np.uint64), want, "dev_probe_multi_packed")
    sl.same(unpack6(packed6.get(), N1), w6, "dev_pack_residues6")
    sl.same(mask64.get(), want, "dev_probe_multi_packed6")


def test_or_slices_route_partition_crc(seb, torch_cuda, rig):
    """seb_dev_or_slices, seb_dev_shard_route, seb_dev_shard_partition and seb_dev_wal_crc (verify and seal)."""
    torch = torch_cuda
    rng = np.random.default_rng(17)
    ns, sw = 3, 4099
    sg, sp = (rng.integers(-2**31, 2**31, ns * sw, dtype=np.int64).astype(np.int32) for _ in range(2))
    want_or = np.bitwise_or.reduce(sg.reshape(ns, sw), axis=0)
    kgood, kpoison = (rng.integers(0, 256, (N1, 16), dtype=np.uint8) for _ in range(2))
    bits = 8
    h, hp = cc.fnv32a_batch(kgood, N1, stride=16), cc.fnv32a_batch(kpoison, N1, stride=16)
    shard, shard_p = ((x & ((1 << bits) - 1)).astype(np.uint16) for x in (h, hp))
    perm, begin = cc.partition(shard, bits)
    perm_p, begin_p = cc.partition(shard_p, bits)
    img, off = kg.wal_image(N, value_size=100, delete_every=0)
    img_p = img.copy()
    # the poison: other value bytes inside the same framing, so other CRCs, and records that fail their stored CRC
    img_p[(off[1:].astype(np.int64)[:, None] - 1 - np.arange(50)[None, :]).reshape(-1)] ^= 0x55
    crc, ok = cc.wal_crc(img, off)
    crc_p, ok_p = cc.wal_crc(img_p, off)
    blank, blank_p, sealed_p = img.copy(), img_p.copy(), img_p.copy()
    st = off[:-1].astype(np.int64)
    for bb in range(4):
        blank[st + bb] = 0
        blank_p[st + bb] = 0
        sealed_p[st + bb] = ((crc_p >> np.uint32(8 * bb)) & np.uint32(0xFF)).astype(np.uint8)
    sl.differ([want_or, h, shard, perm, begin, crc, ok, img],
              [np.bitwise_or.reduce(sp.reshape(ns, sw), axis=0), hp, shard_p, perm_p, begin_p, crc_p, ok_p, sealed_p])
    L = rig.session()
    slices = L.inp(sg, sp)
    dk = seb.dev_keys(L.inp(kgood, kpoison), n=N1, stride=16)
    d_img, d_off = L.inp(img, img_p), sl.to_dev(torch, off)
    d_blank, d_blank_view = guarded(L, blank, blank_p)
    o_or, o_shard, o_hash = L.out(sw, np.int32), L.out(N1, np.uint16), L.out(N1, np.uint32)
    o_perm, o_begin, o_pshard = L.out(N1, np.uint32), L.out((1 << bits) + 1, np.uint64), L.out(N1, np.uint16)
    o_crc, o_ok = L.out(N, np.uint32), L.out(N, np.uint8)
    ws = torch.empty(max(seb.dev_shard_partition_workspace_size(N1, bits), 16), dtype=torch.uint8, device="cuda")
    L.arm()
    L.call(seb.dev_or_slices, slices, ns, o_or.t)
    L.call(seb.dev_shard_route, dk, bits, o_shard.t, o_hash.t)
    L.call(seb.dev_shard_partition, dk, bits, o_perm.t, o_begin.t, o_pshard.t, ws)
    L.call(seb.dev_wal_crc, d_img, d_off, seb.WAL_VERIFY, o_crc.t, o_ok.t)
    L.call(seb.dev_wal_crc, d_blank_view, d_off, seb.WAL_SEAL)
    L.finish()
    sl.same(o_or.get(), want_or, "dev_or_slices")
    sl.same(o_hash.get(), h, "dev_shard_route: hash")
    sl.same(o_shard.get(), shard, "dev_shard_route: shard")
    sl.same(o_perm.get(), perm, "dev_shard_partition: perm")
    sl.same(o_begin.get(), begin, "dev_shard_partition: shard_begin")
    sl.same(o_pshard.get(), shard, "dev_shard_partition: shard")
    sl.same(o_crc.get(), crc, "dev_wal_crc: crc")
    sl.same(o_ok.get(), ok, "dev_wal_crc: ok")
    sl.same(read_guarded(d_blank, img.size, np.uint8, "the sealed image"), img, "dev_wal_crc: seal")


# ------------------------------------------------------------------ 2. filter kernels that keep per-stream scratch

M_PHASED = 33_554_433          # one bit over a 4 MiB range: the phased probe, two ranges
M_BUCKETED = 512 * 65536 - 17  # the first filter the bin scatter takes


@pytest.fixture(scope="module")
def phased(seb):
    """The phased probe's filter and three probe batches of growing size, each with a poison."""
    k = 7
    rng = np.random.default_rng(21)
    build = rng.integers(0, 256, (60_000, 16), dtype=np.uint8)
    bits = oc.build(M_PHASED, k, build, 60_000, stride=16)
    batches = []
    for n in (60_000, 90_000, 120_000):
        good, poison = (rng.integers(0, 256, (n, 16), dtype=np.uint8) for _ in range(2))
        for p in (good, poison):
            hit = rng.random(n) < 0.5
            p[hit] = build[rng.integers(0, 60_000, int(hit.sum()))]
        want = oc.probe(bits, M_PHASED, k, good, n, stride=16)
        sl.differ([want], [oc.probe(bits, M_PHASED, k, poison, n, stride=16)])
        batches.append((n, good, poison, want))
    return dict(k=k, bits=bits, batches=batches)


def test_phased_probe_scratch_grows_on_a_busy_stream(seb, torch_cuda, rig, phased):
    """Two probes on busy S, the second with a larger batch: S's scratch grows while S is busy (the grow
    synchronises S, so that call is checked like a plan call); then the first batch again on busy S, served from the
    grown scratch with no synchronisation."""
    k = phased["k"]
    L = rig.session()
    words = sl.to_dev(torch_cuda, words_of(seb, phased["bits"], M_PHASED))
    (n0, g0, p0, w0), (n1, g1, p1, w1) = phased["batches"][:2]
    dk0, dk1 = seb.dev_keys(L.inp(g0, p0), n=n0, stride=16), seb.dev_keys(L.inp(g1, p1), n=n1, stride=16)
    out0, out1, out2 = L.out(n0, np.uint8), L.out(n1, np.uint8), L.out(n0, np.uint8)
    L.arm()
    L.call(seb.dev_probe, dk0, words, M_PHASED, k, out0.t)
    held = seb.workspace_bytes()
    assert held > 0, "the phased probe took no library scratch: another probe path ran"
    L.plan(seb.dev_probe, dk1, words, M_PHASED, k, out1.t)
    assert seb.workspace_bytes() > held, "the larger batch did not grow the scratch"
    dk2 = seb.dev_keys(L.inp(g0, p0), n=n0, stride=16)
    L.arm()
    L.call(seb.dev_probe, dk2, words, M_PHASED, k, out2.t)
    L.finish()
    sl.same(out0.get(), w0, "first probe")
    sl.same(out1.get(), w1, "larger probe")
    sl.same(out2.get(), w0, "probe from the grown scratch")


def test_bucketed_build_scratch_grows_on_a_busy_stream(seb, torch_cuda, rig):
    """build_algo 2 at the first bin-scatter filter, 300,000 keys and then 450,000."""
    k = 7
    rng = np.random.default_rng(22)
    sets = []
    for n in (300_000, 450_000):
        good, poison = (rng.integers(0, 256, (n, 16), dtype=np.uint8) for _ in range(2))
        want = words_of(seb, oc.build(M_BUCKETED, k, good, n, stride=16), M_BUCKETED)
        sl.differ([want], [words_of(seb, oc.build(M_BUCKETED, k, poison, n, stride=16), M_BUCKETED)])
        sets.append((n, good, poison, want))
    L = rig.session()
    nw = sets[0][3].size
    dks = [seb.dev_keys(L.inp(g, p), n=n, stride=16) for n, g, p, _ in sets]
    bufs = [guarded(L, np.zeros(nw, np.int32), np.full(nw, 0x01010101, np.int32)) for _ in sets]
    with seb.option("build_algo", 2):
        L.arm()
        L.call(seb.dev_build, dks[0], bufs[0][1], M_BUCKETED, k)
        held = seb.workspace_bytes()
        assert held > 0, "the bucketed build took no library scratch: another build ran"
        L.plan(seb.dev_build, dks[1], bufs[1][1], M_BUCKETED, k)
        assert seb.workspace_bytes() > held, "the larger batch did not grow the scratch"
        L.finish()
    for (n, _, _, want), (t, _) in zip(sets, bufs):
        sl.same(read_guarded(t, 4 * nw, np.int32, "words"), want, f"bucketed build of {n} keys")


# ------------------------------------------------------------------ 13. release with work pending

def test_release_with_work_pending(seb, torch_cuda, rig, phased):
    """seb_workspace_release while S still sits in its delay with a phased probe behind it: on return the probe is
    done (release synchronises the streams that hold scratch), nothing is held, the answers are right, and the
    next probe on S allocates again."""
    torch = torch_cuda
    k = phased["k"]
    n, good, poison, want = phased["batches"][0]
    L = rig.session()
    words = sl.to_dev(torch, words_of(seb, phased["bits"], M_PHASED))
    dk = seb.dev_keys(L.inp(good, poison), n=n, stride=16)
    out, out2 = L.out(n, np.uint8), L.out(n, np.uint8)
    L.arm()
    L.call(seb.dev_probe, dk, words, M_PHASED, k, out.t)
    done = torch.cuda.Event()
    done.record(L.S)
    assert done.query() is False
    seb.workspace_release()
    assert done.query() is True, "seb_workspace_release returned with the stream's work still pending"
    assert seb.workspace_bytes() == 0
    sl.same(out.get(), want, "the probe that was pending")
    dk2 = seb.dev_keys(L.inp(good, poison), n=n, stride=16)
    L.arm()
    L.call(seb.dev_probe, dk2, words, M_PHASED, k, out2.t)
    assert seb.workspace_bytes() > 0
    L.finish()
    sl.same(out2.get(), want, "the probe after the release")


# ------------------------------------------------------------------ data of the LSM-side cases

SHIFT = 17 * 1000


def kb(i):
    """The key of id i: six digits and i % 17 bytes more, so 6..22 bytes in the ids' order.  An id shifted by a
    multiple of SHIFT has another key of the same length: a poison made by shifting keeps every array size."""
    return b"%06d" % i + b"x" * (i % 17)


def vb(tag, i, length):
    return (tag + b"%d." % i).ljust(length, b"~")[:length]


def pack(keys):
    off = np.zeros(len(keys) + 1, np.uint64)
    np.cumsum([len(k) for k in keys], out=off[1:])
    return np.frombuffer(b"".join(keys) or b"\0", np.uint8).copy(), off


def late_keys(L, seb, good, poison):
    """A variable-length device batch whose bytes arrive late; the poison keys have the good keys' lengths."""
    (gd, off), (pd, poff) = pack(good), pack(poison)
    assert np.array_equal(off, poff)
    return seb.dev_keys(L.inp(gd, pd), sl.to_dev(L.torch, off))


def sorted_items(ids, tag, rng, vlen=lambda pos: 30 + pos % 41, dels=0.15):
    """(key, value, deleted) in key order; the value lengths follow the position, not the id."""
    return [(kb(int(i)), vb(tag, int(i), vlen(pos)), int(rng.random() < dels)) for pos, i in enumerate(sorted(ids))]


# ------------------------------------------------------------------ 4. block search

def test_block_search_and_resolve(seb, torch_cuda, rig):
    """seb_dev_search_blocks -> seb_dev_resolve_rows, cap 3, over three files' blocks in one pool: the keys and the
    block ids arrive late; cells, status, col, vloc and vlen against block_ref."""
    rng = np.random.default_rng(41)
    cap = 3
    files = [sorted_items(rng.choice(6000, 1400, replace=False), b"f%d-" % f, rng) for f in range(cap)]
    runs = [mref.run_blocks(items) for items in files]
    pool, blen, rb = mref.pool_of(runs, fill=0xA5)
    images = [img for blocks in runs for img in blocks]
    assert len(images) >= 40
    firsts = [[mref.load_block(img)[0][0] for img in blocks] for blocks in runs]

    def bid_of(keys):
        """Per key and file, the block SSTable.Get would read: the last one whose first key is <= the key."""
        bid = np.full((len(keys), cap), seb.NO_BLOCK_ID, np.uint32)
        for i, key in enumerate(keys):
            for f in range(cap):
                e = bisect.bisect_right(firsts[f], key) - 1
                if e >= 0:
                    bid[i, f] = rb[f] + e
        return bid

    def answers(keys, bid):
        cells = np.zeros((len(keys), cap), np.uint32)
        st, col = np.zeros(len(keys), np.uint8), np.zeros(len(keys), np.uint16)
        vloc, vlen = np.zeros(len(keys), np.uint64), np.zeros(len(keys), np.uint32)
        for i, key in enumerate(keys):
            for f in range(cap):
                b = int(bid[i, f])
                cells[i, f] = br.search_block_ref(images[b], key) if b != seb.NO_BLOCK_ID else br.cell(br.NONE)
            s, c, cell = br.lsm_get_ref(cells[i].tolist())
            st[i], col[i] = s, c
            if s == br.GET_FOUND:
                vloc[i], vlen[i] = int(bid[i, c]) * 4096 + ((cell >> 13) & 0x1FFF), cell & 0x1FFF
        return cells.reshape(-1), st, col, vloc, vlen

    ids = rng.integers(0, 6400, N)
    keys = [kb(int(i)) for i in ids]
    bid = bid_of(keys)
    want = answers(keys, bid)
    # the poison: keys shifted out of every file (same lengths), and the rows of block ids in another order
    pkeys, pbid = [kb(int(i) + SHIFT) for i in ids], bid[rng.permutation(N)]
    want_p = answers(pkeys, pbid)
    assert {br.FOUND, br.MISS, br.TOMBSTONE} <= set((want[0] >> 28).tolist()) and (want[1] == br.GET_FOUND).sum() > N // 4
    sl.differ(want, want_p, ("cells", "status", "col", "vloc", "vlen"))
    L = rig.session()
    dpool, dblen = sl.to_dev(torch_cuda, pool), sl.to_dev(torch_cuda, blen)
    dk = late_keys(L, seb, keys, pkeys)
    dbid = L.inp(bid.reshape(-1), pbid.reshape(-1))
    cells, st, col = L.out(N * cap, np.uint32), L.out(N, np.uint8), L.out(N, np.uint16)
    vloc, vlen = L.out(N, np.uint64), L.out(N, np.uint32)
    L.arm()
    L.call(seb.dev_search_blocks, dk, dbid, cap, dpool, dblen, cells.t)
    L.call(seb.dev_resolve_rows, cells.t, dbid, N, cap, st.t, col.t, vloc.t, vlen.t)
    L.finish()
    for o, w, name in zip((cells, st, col, vloc, vlen), want, ("cells", "status", "col", "vloc", "vlen")):
        sl.same(o.get(name), w, name)


# ------------------------------------------------------------------ 5. builder

def test_builder_plan_and_encode(seb, torch_cuda, rig):
    """seb_dev_sst_plan -> seb_dev_sst_encode, two files in one call, against sstable_ref: the keys and val_off
    arrive late before the plan; the values and the deleted bytes, which only the encode reads, before the encode."""
    rng = np.random.default_rng(51)
    ids = np.sort(rng.choice(9000, N, replace=False))
    file_begin = [0, 1000, N]
    vl = 20 + rng.integers(0, 120, N)
    good = [(kb(int(i)), vb(b"g", int(i), int(vl[p])), int(rng.random() < 0.2)) for p, i in enumerate(ids)]
    vl_p = np.roll(vl, 700)  # the same lengths at other entries: the same bytes in all, other block cuts
    poison = [(kb(int(i) + SHIFT), vb(b"p", int(i), int(vl_p[p])), int(rng.random() < 0.2)) for p, i in enumerate(ids)]

    def want_of(items):
        parts = [sref.sections(items[a:b]) for a, b in zip(file_begin[:-1], file_begin[1:])]
        assert all(p[4] == 0 for p in parts)
        sizes = [(len(p[3]), len(p[0]), len(p[1]), len(p[2]), 0) for p in parts]
        return sizes, (np.frombuffer(b"".join(p[0] for p in parts), np.uint8), np.frombuffer(b"".join(p[1] for p in parts), np.uint8),
                       np.frombuffer(b"".join(p[2] for p in parts), np.uint8), np.array([x for p in parts for x in p[3]], np.uint16))

    sizes_w, want = want_of(good)
    sizes_p, want_p = want_of(poison)
    sl.differ(want, want_p, ("data", "index", "meta", "blen"))
    g, p = sref.pack(good), sref.pack(poison)
    assert np.array_equal(g[1], p[1]) and g[2].size == p[2].size
    L = rig.session()
    torch = torch_cuda
    dk = seb.dev_keys(L.inp(g[0], p[0]), sl.to_dev(torch, g[1]))
    dvoff = L.inp(g[3], p[3])
    ws = torch.zeros(seb.dev_sst_workspace_size(N, 2), dtype=torch.uint8, device="cuda")
    L.arm()
    sizes = L.plan(seb.dev_sst_plan, dk, dvoff, file_begin, ws)
    assert sizes == sizes_w, "the plan's sizes"
    dvals, ddel = L.inp(g[2], p[2]), L.inp(g[4], p[4])
    data, index, meta, oblen = (L.out(w.size, w.dtype) for w in want)
    L.arm()
    L.call(seb.dev_sst_encode, dk, dvals, dvoff, ddel, file_begin, sizes, ws, data.t, index.t, meta.t, blen=oblen.t)
    L.finish()
    for o, w, name in zip((data, index, meta, oblen), want, ("data", "index", "meta", "blen")):
        sl.same(o.get(name), w, name)


# ------------------------------------------------------------------ 6. merge

def same_blocks(items, target):
    """The longest prefix of the sorted items that the builder cuts into `target` blocks."""
    while len(mref.run_blocks(items)) > target:
        items = items[:-1]
    assert len(mref.run_blocks(items)) == target
    return items


def test_merge_count_plan_emit(seb, torch_cuda, rig):
    """seb_dev_merge_count -> seb_dev_merge_plan -> seb_dev_merge_emit over three runs that share keys, against
    merge_ref.rule_merge (and, byte for byte, the host half).  The poison has the good pool's blocks per run, but
    longer values (so other entries per block), other keys and no key in two runs."""
    rng = np.random.default_rng(61)
    counts = (1025, 700, 324)
    space = rng.choice(3000, 1500, replace=False)
    ids = [rng.choice(space, c, replace=False) for c in counts]
    good = [sorted_items(x, b"r%d:" % r, rng) for r, x in enumerate(ids)]
    runs = [mref.run_blocks(items) for items in good]
    poison = [same_blocks(sorted_items(x + SHIFT * (r + 1), b"p%d:" % r, rng, vlen=lambda pos: 36 + pos % 41), len(runs[r]))
              for r, x in enumerate(ids)]
    pool, blen, rb = mref.pool_of(runs)
    pool_p, blen_p, rb_p = mref.pool_of([mref.run_blocks(items) for items in poison])
    assert rb == rb_p and pool.size == pool_p.size

    def want_of(items_runs, pl, bl):
        merged = mref.as_bytes(mref.rule_merge(items_runs))
        n_in = sum(len(r) for r in items_runs)
        sizes = (n_in, len(merged), sum(len(k) for k, _, _ in merged), sum(len(v) for _, v, _ in merged), n_in - len(merged), 0)
        host = seb.merge_emit(pl, bl, rb)
        assert host[5] == sizes and mref.unpack(*host[:5]) == merged, "the host half against rule_merge"
        block_entries = np.array([len(mref.load_block(bytes(pl[b * 4096: b * 4096 + int(bl[b])]))) for b in range(len(bl))], np.uint16)
        return sizes, merged, (block_entries,) + tuple(host[:5])

    sizes_w, merged, want = want_of(good, pool, blen)
    assert sizes_w[4] > 100, "the runs share keys"
    _, _, want_p = want_of(poison, pool_p, blen_p)
    names = ("block_entries", "keys", "key_off", "vals", "val_off", "deleted")
    sl.differ(want, want_p, names)
    L = rig.session()
    torch = torch_cuda
    dpool, dblen = L.inp(pool, pool_p), L.inp(blen, blen_p)
    dcnt = L.out(len(blen), np.uint16)
    L.arm()
    run_entries = L.plan(seb.dev_merge_count, dpool, dblen, rb, dcnt.t)
    assert run_entries == [len(r) for r in good]
    ws = torch.zeros(seb.dev_merge_workspace_size(sizes_w[0], len(blen), 3), dtype=torch.uint8, device="cuda")
    sizes = L.plan(seb.dev_merge_plan, dpool, dblen, rb, dcnt.t, ws)
    assert sizes == sizes_w, "the plan's sizes"
    outs = [L.out(w.size, w.dtype) for w in want[1:]]
    L.arm()  # the emit reads the workspace's header back before it launches: it waits for the stream, like a plan call
    L.plan(seb.dev_merge_emit, dpool, sizes, ws, *[o.t for o in outs])
    L.finish()
    got = [dcnt.get()] + [o.get(n) for o, n in zip(outs, names[1:])]
    for g, w, name in zip(got, want, names):
        sl.same(g, w, name)
    assert mref.unpack(*got[1:]) == merged


# ------------------------------------------------------------------ 7. replay

def test_replay_plan_and_emit(seb, torch_cuda, rig):
    """seb_dev_wal_replay_plan -> seb_dev_wal_replay_emit against memtable_ref: 2049 records over about 700 keys.
    The poison's records have the same lengths, other keys (twice as many distinct ones), flags and sequences."""
    rng = np.random.default_rng(71)
    ids = rng.choice(rng.choice(5000, 700, replace=False), N)
    seqs, seqs_p = rng.permutation(N) + 1, rng.permutation(N) + 5000
    recs = [(kb(int(i)), vb(b"g", p, 10 + p % 50), int(seqs[p]), bool(rng.random() < 0.2)) for p, i in enumerate(ids)]
    recs_p = [(kb(int(i) + SHIFT * (1 + p % 2)), vb(b"p", p, 10 + p % 50), int(seqs_p[p]), bool(rng.random() < 0.2))
              for p, i in enumerate(ids)]

    def want_of(records):
        image, off = tref.wal_image(records)
        ents, sizes = tref.expected(records)
        host = seb.wal_replay_emit(image, off)
        assert host[6] == sizes and tref.unpack(*host[:6]) == ents, "the host half against memtable_ref"
        return np.frombuffer(image, np.uint8), np.array(off, np.uint64), sizes, ents, tuple(host[:6])

    img, off, sizes_w, ents, want = want_of(recs)
    img_p, off_p, _, _, want_p = want_of(recs_p)
    assert np.array_equal(off, off_p) and sizes_w[4] > 1000
    names = ("keys", "key_off", "vals", "val_off", "deleted", "seq")
    sl.differ(want, want_p, names)
    L = rig.session()
    torch = torch_cuda
    dimg, doff = L.inp(img, img_p), sl.to_dev(torch, off)
    ws = torch.zeros(seb.dev_wal_replay_workspace_size(N), dtype=torch.uint8, device="cuda")
    L.arm()
    sizes = L.plan(seb.dev_wal_replay_plan, dimg, doff, ws)
    assert sizes == sizes_w, "the plan's sizes"
    outs = [L.out(w.size, w.dtype) for w in want]
    L.arm()  # the emit reads the workspace's header back before it launches: it waits for the stream, like a plan call
    L.plan(seb.dev_wal_replay_emit, dimg, doff, sizes, ws, *[o.t for o in outs])
    L.finish()
    got = [o.get(n) for o, n in zip(outs, names)]
    for g, w, name in zip(got, want, names):
        sl.same(g, w, name)
    assert tref.unpack(*got) == ents


# ------------------------------------------------------------------ 8. memtable read side

def table(ids, tag, rng, seq0, flags=None, vlen=20):
    """A memtable of distinct ids (so one entry per op); flags: the deleted flag per op, default random."""
    flags = (rng.random(len(ids)) < 0.25) if flags is None else flags
    seqs = rng.permutation(len(ids)) + seq0
    return gref.table_from_ops([(kb(int(i)), vb(tag, int(i), vlen), int(s), int(f)) for i, s, f in zip(ids, seqs, flags)])


def late_run(L, seb, good, poison):
    """A dev_run whose arrays (memget_ref.run_arrays: keys, key_off, vals, val_off, deleted, seq) arrive late."""
    for j in (0, 1, 2, 3):
        assert good[j].shape == poison[j].shape, "the poison run has other array sizes"
    keys, koff, voff = L.inp(good[0], poison[0]), L.inp(good[1], poison[1], differ=False), L.inp(good[3], poison[3], differ=False)
    return seb.dev_run(keys, koff, voff, L.inp(good[4], poison[4]), L.inp(good[5], poison[5]), n=len(good[1]) - 1,
                       key_bytes=good[0].size)


def index_for(L, seb, run):
    """The run's index, built by a synchronising call on S; its bytes are the library's own format, so the cases
    check it through the calls that read it, and here only the guards."""
    ix = L.out(seb.dev_run_index_size(run.n), np.uint8)
    L.plan(seb.dev_run_index, run, ix.t)
    return ix


def memget_data(seed, n_probe=N):
    """Two memtables (the active one first), good and poison, and good and poison probe keys with what
    memget_ref expects for each."""
    rng = np.random.default_rng(seed)
    space = rng.choice(6000, 3000, replace=False)
    ids = [rng.choice(space, c, replace=False) for c in (N, 1500)]
    good = [table(x, b"a%d-" % r, rng, 1000 * r) for r, x in enumerate(ids)]
    poison = []
    for r, x in enumerate(ids):  # other keys of the same lengths, the same number of tombstones at other entries
        flags = np.array([e[3] for e in good[r].entries])
        poison.append(table(x + SHIFT * (r + 1), b"b%d-" % r, rng, 7000 + 1000 * r, flags=rng.permutation(flags)))
    pids = rng.choice(np.concatenate([space, np.arange(6000, 6400)]), n_probe)
    probes, probes_p = [kb(int(i)) for i in pids], [kb(int(i) + SHIFT * (1 + p % 2)) for p, i in enumerate(pids)]
    return dict(good=good, poison=poison, probes=probes, probes_p=probes_p, want=gref.expected(good, probes),
                want_p=gref.expected(good, probes_p))


def test_run_index_runs_search_get_join(seb, torch_cuda, rig):
    """seb_dev_run_index (two runs, late arrays) -> seb_dev_runs_search (late probe keys) -> seb_dev_get_join (late
    sst_status) against memget_ref."""
    d = memget_data(81)
    rng = np.random.default_rng(82)
    want = d["want"]
    assert {gref.NONE, gref.FOUND, gref.TOMBSTONE} <= set(want[0].tolist()) and {0, 1} <= set(want[1].tolist())
    sst, sst_p = (rng.integers(0, 3, N).astype(np.uint8) for _ in range(2))

    def join(ms, ss):
        dec = (ms == gref.FOUND) | (ms == gref.TOMBSTONE)
        return np.where(ms == gref.FOUND, 1, np.where(ms == gref.TOMBSTONE, 0, ss)).astype(np.uint8), (~dec).astype(np.uint8)

    want_join, want_join_p = join(want[0], sst), join(d["want_p"][0], sst_p)
    host_join = seb.get_join(want[0], sst)
    assert np.array_equal(host_join[0], want_join[0]) and np.array_equal(host_join[1], want_join[1])
    sl.differ(want + want_join, d["want_p"] + want_join_p, gref.NAMES + ("join status", "join source"))
    L = rig.session()
    runs = [late_run(L, seb, gref.run_arrays(g), gref.run_arrays(p)) for g, p in zip(d["good"], d["poison"])]
    L.arm()
    indexes = [index_for(L, seb, r) for r in runs]
    dk = late_keys(L, seb, d["probes"], d["probes_p"])
    dsst = L.inp(sst, sst_p)
    outs = [L.out(N, t) for t in (np.uint8, np.uint8, np.uint32, np.uint64, np.uint32, np.uint64)]
    jst, jsrc = L.out(N, np.uint8), L.out(N, np.uint8)
    L.arm()
    L.call(seb.dev_runs_search, dk, runs, [ix.t for ix in indexes], *[o.t for o in outs])
    L.call(seb.dev_get_join, outs[0].t, dsst, N, jst.t, jsrc.t)
    L.finish()
    gref.assert_same([o.get(n) for o, n in zip(outs, gref.NAMES)], want, "runs_search")
    sl.same(jst.get(), want_join[0], "get_join: status")
    sl.same(jsrc.get(), want_join[1], "get_join: source")
    for ix in indexes:
        ix.get("a run index")


# ------------------------------------------------------------------ 9. memtable write side

def test_wal_frame_plan_and_emit(seb, torch_cuda, rig):
    """seb_dev_wal_frame_plan -> seb_dev_wal_frame_emit against memwrite_ref / memtable_ref's records: keys, val_off
    and deleted arrive late before the plan, the value bytes before the emit."""
    rng = np.random.default_rng(91)
    ids = rng.choice(5000, N)
    vl = 5 + rng.integers(0, 60, N)
    vl_p = np.roll(vl, 900)
    ops = [(kb(int(i)), vb(b"g", p, int(vl[p])), int(rng.random() < 0.2)) for p, i in enumerate(ids)]
    ops_p = [(kb(int(i) + SHIFT), vb(b"p", p, int(vl_p[p])), int(rng.random() < 0.2)) for p, i in enumerate(ids)]
    first_seq = (1 << 33) + 5

    def want_of(o):
        image, off = tref.wal_image(wref.batch_records(o, first_seq))
        return np.array(off, np.uint64), np.frombuffer(image, np.uint8)

    want, want_p = want_of(ops), want_of(ops_p)
    sl.differ(want, want_p, ("rec_off", "image"))
    g, p = wref.op_arrays(ops), wref.op_arrays(ops_p)
    assert np.array_equal(g[1], p[1]) and g[2].size == p[2].size
    L = rig.session()
    dk = seb.dev_keys(L.inp(g[0], p[0]), sl.to_dev(torch_cuda, g[1]))
    dvoff, ddel = L.inp(g[3], p[3]), L.inp(g[4], p[4])
    rec = L.out(N + 1, np.uint64)
    L.arm()
    total = L.plan(seb.dev_wal_frame_plan, dk, dvoff, ddel, rec.t)
    assert total == want[1].size, "the plan's image size"
    dvals = L.inp(g[2], p[2])
    image = L.out(total, np.uint8)
    L.arm()
    L.call(seb.dev_wal_frame_emit, dk, dvals, dvoff, ddel, first_seq, rec.t, image.t, image_bytes=total)
    L.finish()
    sl.same(rec.get("rec_off"), want[0], "rec_off")
    sl.same(image.get("image"), want[1], "image")


def test_run_size_delta(seb, torch_cuda, rig):
    """seb_dev_run_size_delta of a fresh run that arrives late over two existing runs, against memwrite_ref.fold."""
    torch = torch_cuda
    rng = np.random.default_rng(92)
    space = rng.choice(6000, 3000, replace=False)
    old = [table(rng.choice(space, 1200, replace=False), b"o%d-" % r, rng, 100 + 2000 * r) for r in range(2)]
    fresh_ids = rng.choice(space, N, replace=False)
    fresh = table(fresh_ids, b"new-", rng, 9000, vlen=27)
    flags = np.array([e[3] for e in fresh.entries])
    fresh_p = table(fresh_ids + SHIFT, b"bad-", rng, 20000, flags=rng.permutation(flags), vlen=27)
    before = wref.fold(old).size
    want, want_p = wref.fold([fresh] + old).size - before, wref.fold([fresh_p] + old).size - before
    assert want != want_p and want_p == fresh_p.size
    existing, indexes = [], []
    for t in old:  # set up beforehand, on the default stream
        a = gref.run_arrays(t)
        run = seb.dev_run(sl.to_dev(torch, a[0]), sl.to_dev(torch, a[1]), sl.to_dev(torch, a[3]), sl.to_dev(torch, a[4]),
                          sl.to_dev(torch, a[5]), n=len(a[1]) - 1, key_bytes=a[0].size)
        ix = torch.zeros(seb.dev_run_index_size(run.n), dtype=torch.uint8, device="cuda")
        seb.dev_run_index(run, ix)
        existing.append(run), indexes.append(ix)
    L = rig.session()
    run = late_run(L, seb, gref.run_arrays(fresh), gref.run_arrays(fresh_p))
    delta = L.out(1, np.int64)
    L.arm()
    L.call(seb.dev_run_size_delta, run, existing, indexes, delta.t)
    L.finish()
    assert int(delta.get("delta")[0]) == want


def test_runs_fold_plan_and_emit(seb, torch_cuda, rig):
    """seb_dev_run_index x 3 -> seb_dev_runs_fold_plan -> seb_dev_runs_fold_emit over three runs that share keys,
    against memwrite_ref.fold (and, byte for byte, the host half): the runs arrive late before the first index is
    built, the value bytes before the emit."""
    rng = np.random.default_rng(93)
    space = rng.choice(6000, 1800, replace=False)
    ids = [rng.choice(space, c, replace=False) for c in (1025, 700, 324)]
    good = [table(x, b"r%d-" % r, rng, 1 + 3000 * r) for r, x in enumerate(ids)]
    poison = []
    for r, x in enumerate(ids):
        flags = np.array([e[3] for e in good[r].entries])
        poison.append(table(x + SHIFT * (r + 1), b"p%d-" % r, rng, 50000 + 3000 * r, flags=rng.permutation(flags)))

    def want_of(tables):
        arrays = [gref.run_arrays(t) for t in tables]
        host = seb.runs_fold([seb.host_run(a[0], a[1], a[3], a[4], a[5]) for a in arrays], [a[2] for a in arrays])
        sizes = wref.fold_sizes(tables)
        assert host[6] == sizes and tref.unpack(*host[:6]) == wref.entries_of(wref.fold(tables)), "the host half against fold"
        return arrays, sizes, tuple(host[:6])

    arrays, sizes_w, want = want_of(good)
    arrays_p, _, want_p = want_of(poison)
    assert sizes_w[4] > 100, "the runs share keys"
    names = ("keys", "key_off", "vals", "val_off", "deleted", "seq")
    sl.differ(want, want_p, names)
    L = rig.session()
    torch = torch_cuda
    runs = [late_run(L, seb, g, p) for g, p in zip(arrays, arrays_p)]
    val_bytes = [a[2].size for a in arrays]
    ws = torch.zeros(seb.dev_runs_fold_workspace_size(sizes_w[0]), dtype=torch.uint8, device="cuda")
    L.arm()
    indexes = [index_for(L, seb, r) for r in runs]
    sizes = L.plan(seb.dev_runs_fold_plan, runs, [ix.t for ix in indexes], val_bytes, ws)
    assert sizes == sizes_w, "the plan's sizes"
    outs = [L.out(w.size, w.dtype) for w in want]
    vals = [L.inp(g[2], p[2]) for g, p in zip(arrays, arrays_p)]
    L.arm()  # the emit reads the workspace's header back before it launches: it waits for the stream, like a plan call
    L.plan(seb.dev_runs_fold_emit, runs, [ix.t for ix in indexes], vals, sizes, ws, *[o.t for o in outs], val_bytes=val_bytes)
    L.finish()
    got = [o.get(n) for o, n in zip(outs, names)]
    for g, w, name in zip(got, want, names):
        sl.same(g, w, name)


# ------------------------------------------------------------------ 10. Get path

def getpath_data(seed, layout, n=N):
    """A probe batch (fixed 16-byte keys or variable-length ones), memtable statuses and the SSTable steps' results
    for the undecided keys, good and poison, with getpath_ref's answers."""
    rng = np.random.default_rng(seed)
    ids = rng.choice(50_000, n, replace=False)
    if layout == "fixed16":
        keys, keys_p = [kg.key16_bytes(int(i)) for i in ids], [kg.key16_bytes(int(i) + 60_000) for i in ids]
    else:
        keys, keys_p = [kb(int(i)) for i in ids], [kb(int(i) + SHIFT) for i in ids]
    mem = rng.choice(np.array([0, 0, 3, 255, 1, 1, 2], np.uint8), n)
    mem_p = rng.permutation(mem)  # the same number of undecided keys, at other places
    stride = 16 if layout == "fixed16" else None
    out = dict(layout=layout, n=n, keys=keys, keys_p=keys_p, mem=mem, mem_p=mem_p, stride=stride)
    for tag, k, ms in (("", keys, mem), ("_p", keys_p, mem_p)):
        sizes, okeys, ooff, row = pref.compact_arrays(k, ms, stride)
        m = sizes[1]
        inputs = dict(mem_vloc=rng.integers(0, 1 << 40, n).astype(np.uint64), mem_vlen=rng.integers(1, 1 << 20, n).astype(np.uint32),
                      sst_col=rng.integers(0, 7, m).astype(np.uint16), sst_vloc=rng.integers(1, 1 << 40, m).astype(np.uint64),
                      sst_vlen=rng.integers(1, 4096, m).astype(np.uint32))
        sst = rng.integers(0, 3, m).astype(np.uint8)
        compact = (okeys, row) if ooff is None else (okeys, ooff, row)
        out.update({"sizes" + tag: sizes, "compact" + tag: compact, "sst" + tag: sst, "inputs" + tag: inputs,
                    "join" + tag: pref.join_rows(ms, row, sst, **inputs)})
    assert out["sizes"][1] == out["sizes_p"][1] and 0 < out["sizes"][1] < n
    sl.differ(out["compact"] + out["join"], out["compact_p"] + out["join_p"])
    return out


def late_batch(L, seb, d):
    if d["layout"] == "fixed16":
        t = L.inp(np.frombuffer(b"".join(d["keys"]), np.uint8), np.frombuffer(b"".join(d["keys_p"]), np.uint8))
        assert t.data_ptr() % 16 == 0
        return seb.dev_keys(t, n=d["n"], stride=16)
    return late_keys(L, seb, d["keys"], d["keys_p"])


def compact_outs(L, d):
    sizes = d["sizes"]
    return L.out(sizes[2], np.uint8), (L.out(sizes[1] + 1, np.uint64) if d["stride"] is None else None), L.out(sizes[1], np.uint32)


def check_compact(d, okeys, ooff, row):
    want = d["compact"]
    sl.same(okeys.get("out_keys"), want[0], "out_keys")
    if ooff is not None:
        sl.same(ooff.get("out_off"), want[1], "out_off")
    sl.same(row.get("row"), want[-1], "row")


@pytest.mark.parametrize("layout", ["fixed16", "offsets"])
def test_compact_plan_emit_and_join_rows(seb, torch_cuda, rig, layout):
    """seb_dev_get_compact_plan -> seb_dev_get_compact_emit -> seb_dev_get_join_rows against getpath_ref: the keys
    and mem_status arrive late before the plan; the SSTable steps' results and the memtables' value places, which
    only the join reads, before the emit.  fixed16: aligned 16-byte keys, the fast path."""
    d = getpath_data(101 if layout == "fixed16" else 102, layout)
    n, m = d["n"], d["sizes"][1]
    L = rig.session()
    torch = torch_cuda
    dk = late_batch(L, seb, d)
    dmem = L.inp(d["mem"], d["mem_p"])
    ws = torch.zeros(seb.dev_get_compact_workspace_size(n), dtype=torch.uint8, device="cuda")
    L.arm()
    plan = L.plan(seb.dev_get_compact_plan, dk, dmem, ws)
    assert plan.as_tuple() == d["sizes"], "the plan's sizes"
    okeys, ooff, row = compact_outs(L, d)
    dsst = L.inp(d["sst"], d["sst_p"])
    din = {k: L.inp(v, d["inputs_p"][k]) for k, v in d["inputs"].items()}
    jo = [L.out(n, t) for t in (np.uint8, np.uint8, np.uint16, np.uint64, np.uint32)]
    L.arm()
    ck, _ = L.call(seb.dev_get_compact_emit, dk, dmem, plan, ws, okeys.t, None if ooff is None else ooff.t, row.t)
    assert ck.n == m
    L.call(seb.dev_get_join_rows, dmem, n, row.t, m, dsst, *[o.t for o in jo], **din)
    L.finish()
    check_compact(d, okeys, ooff, row)
    pref.assert_same([o.get(nm) for o, nm in zip(jo, pref.NAMES)], d["join"], "join_rows")


# ------------------------------------------------------------------ 3. registry

NO_BLOCK = 2**64 - 1
PAD = 0xFFFF


def encode_index(entries) -> bytes:
    """[numEntries u32] then per entry [keySize u32][blockOffset u64][key], little-endian."""
    return struct.pack("<I", len(entries)) + b"".join(struct.pack("<IQ", len(k), o) + k for k, o in entries)


def reg_add(reg, files, file_num, level, idx):
    """Put a file of the 16-byte keys of the sorted ids `idx` with its filter and its index (every 8th key)."""
    keys = [kg.key16_bytes(int(i)) for i in idx]
    m, k = oc.params(len(keys), 0.01)
    bits = oc.build(m, k, np.frombuffer(b"".join(keys), np.uint8), len(keys), stride=16)
    entries = [(keys[j], 4096 * (j // 8) + 64 + file_num) for j in range(0, len(keys), 8)]
    slot = reg.put(file_num, level, bn.encode(bits, m, k), keys[0], keys[-1])
    reg.put_index(file_num, encode_index(entries))
    files.append(dict(file=file_num, level=level, min=keys[0], max=keys[-1], bits=bits, m=m, k=k, slot=slot, entries=entries,
                      ekeys=[e[0] for e in entries]))


def read_plan(files, probes, cap):
    """LSM.Get's walk (lsm/lsm.go:168-198: every L0 file in insertion order, then the first L1 file by MinKey whose
    range covers the key), the files of it whose filter may contain the key, and SSTable.Get's index step in each:
    (mask u64, slots (n, cap) u16, block offsets (n, cap) u64)."""
    n = len(probes)
    arr = np.frombuffer(b"".join(probes), np.uint8)
    maybe = {f["file"]: oc.probe(f["bits"], f["m"], f["k"], arr, n, stride=16) for f in files}
    l0 = [f for f in files if f["level"] == 0]
    l1 = sorted((f for f in files if f["level"] == 1), key=lambda f: f["min"])
    mask = np.zeros(n, np.uint64)
    slots, blocks = np.full((n, cap), PAD, np.uint16), np.full((n, cap), NO_BLOCK, np.uint64)
    for i, p in enumerate(probes):
        j = 0
        for f in l0 + [f for f in l1 if f["min"] <= p <= f["max"]][:1]:
            if maybe[f["file"]][i]:
                e = bisect.bisect_right(f["ekeys"], p) - 1
                slots[i, j], blocks[i, j] = f["slot"], (NO_BLOCK if e < 0 else f["entries"][e][1])
                mask[i] |= np.uint64(1 << f["slot"])
                j += 1
    return mask, slots.reshape(-1), blocks.reshape(-1)


def test_registry_first_call_after_put_and_remove(seb, torch_cuda, rig):
    """Four L0 files of one (m, k), so the interleaved L0 table is built, and three disjoint L1 files with indexes.
    After the puts, and again after a remove and a put, the first device call is made on busy S: the rebuild and
    launch_l0_table happen inside it (it synchronises the device, so it is checked like a plan call).  Then
    seb_registry_multiget_dev, _multiget_list_dev and _locate_dev on busy S with fresh late keys."""
    rng = np.random.default_rng(31)
    universe = np.arange(0, 6000, 2)
    reg, files = seb.Registry(0), []
    try:
        for f in range(4):
            reg_add(reg, files, 100 + f, 0, np.sort(rng.choice(universe, 400, replace=False)))
        assert len({(f["m"], f["k"]) for f in files}) == 1
        for j, part in enumerate(np.array_split(universe[50:], 3)):
            reg_add(reg, files, 1000 + j, 1, part)
        cap = 5

        def batch():
            ids, ids_p = rng.integers(0, 6100, N), rng.integers(0, 6100, N)
            good, poison = [kg.key16_bytes(int(i)) for i in ids], [kg.key16_bytes(int(i)) for i in ids_p]
            want, want_p = read_plan(files, good, cap), read_plan(files, poison, cap)
            sl.differ(want, want_p, ("mask", "slots", "blocks"))
            assert (want[2] != NO_BLOCK).sum() > N // 2
            return np.frombuffer(b"".join(good), np.uint8), np.frombuffer(b"".join(poison), np.uint8), want

        def first_call(L):
            """The call that finds the registry dirty."""
            good, poison, want = batch()
            dk = seb.dev_keys(L.inp(good, poison), n=N, stride=16)
            rows = L.out(N * cap, np.uint16)
            L.arm()
            L.plan(reg.multiget_list_dev, dk, rows.t, cap)
            L.finish()
            sl.same(rows.get("rows"), want[1], "multiget_list_dev, the first call")

        def busy_calls(L):
            good, poison, want = batch()
            dk = seb.dev_keys(L.inp(good, poison), n=N, stride=16)
            mask, rows, blocks = L.out(N, np.uint64), L.out(N * cap, np.uint16), L.out(N * cap, np.uint64)
            L.arm()
            L.call(reg.multiget_dev, dk, mask.t)
            L.call(reg.multiget_list_dev, dk, rows.t, cap)
            L.call(reg.locate_dev, dk, rows.t, blocks.t, cap)
            L.finish()
            sl.same(mask.get("mask"), want[0], "multiget_dev")
            sl.same(rows.get("rows"), want[1], "multiget_list_dev")
            sl.same(blocks.get("blocks"), want[2], "locate_dev")

        L = rig.session()
        first_call(L)
        assert reg.max_candidates() == cap
        busy_calls(L)
        # compaction, while nothing is pending: an L0 file goes, another takes its slot at the end of the L0 order
        gone = files.pop(1)
        reg.remove(gone["file"])
        reg_add(reg, files, 104, 0, np.sort(rng.choice(universe, 400, replace=False)))
        assert files[-1]["slot"] == gone["slot"]
        first_call(L)
        busy_calls(L)
    finally:
        torch_cuda.cuda.synchronize()
        reg.close()


# ------------------------------------------------------------------ 11. one whole Get on S

def test_whole_get_on_the_ambient_stream(seb, torch_cuda, rig):
    """LSM.Get over two memtable runs and four SSTables (test_gpu_getpath.py::test_end_to_end, the compacted
    pipeline) for 2049 keys that arrive late, every library call made under `with torch.cuda.stream(S)` with
    stream=None: runs search -> compact -> list -> locate -> search -> resolve -> join rows, and no host
    synchronisation but the plan's own.  Status, source, vlen and the value bytes behind vloc against getpath_ref's
    LSM.Get; col as that test checks it."""
    torch = torch_cuda
    rng = np.random.default_rng(111)
    key = kg.key16_bytes
    val = lambda tag, i: tag + b"%d" % i + bytes(rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8))  # noqa: E731
    l1 = [[(key(i), val(b"l1-", i), 0) for i in range(0, 2000, 2)], [(key(i), val(b"l1-", i), 0) for i in range(2000, 4000, 2)]]
    l0a = [(key(i), val(b"l0a-", i), 1 if i % 12 == 0 else 0) for i in range(0, 4000, 6)]
    l0b = [(key(i), val(b"l0b-", i), 0) for i in range(1, 4200, 14)]
    file_items = [(100, 0, l0a), (101, 0, l0b), (200, 1, l1[0]), (201, 1, l1[1])]
    active = gref.table_from_ops(
        [(key(i), val(b"act-", i), 5000 + i, 0) for i in range(4, 4000, 40)] +
        [(key(i), b"", 6000 + i, 1) for i in range(8, 4000, 40)] +
        [(key(i), val(b"act-", i), 7000 + i, 0) for i in range(5001, 5200, 2)])
    frozen = gref.table_from_ops(
        [(key(i), val(b"imm-", i), 100 + i, 0) for i in range(4, 4000, 80)] +
        [(key(i), val(b"imm-", i), 200 + i, 0) for i in range(16, 4000, 40)] +
        [(key(i), b"", 300 + i, 1) for i in range(24, 4000, 40)] +
        [(key(i), val(b"imm-", i), 400 + i, 0) for i in range(6001, 6100, 2)])
    tables = [active, frozen]
    files = [pref.File(num, level, items) for num, level, items in file_items]
    # set up beforehand, on the default stream: the block pool (the files' data sections), the registry, the runs
    pool = np.frombuffer(b"".join(f.data for f in files), np.uint8)
    blens = np.array([x for f in files for x in f.blens], np.uint16)
    dpool, dblen = sl.to_dev(torch, pool), sl.to_dev(torch, blens)
    reg = seb.Registry(0)
    try:
        first_block = torch.full((65536,), -1, dtype=torch.int64, device="cuda")
        at_block = 0
        for (num, level, its), f in zip(file_items, files):
            keys = [k for k, _, _ in its]
            m_bits, k_hash = oc.params(len(keys), 0.01)
            bits = oc.build(m_bits, k_hash, np.frombuffer(b"".join(keys), np.uint8), len(keys), stride=16)
            slot = reg.put(num, level, bn.encode(bits, m_bits, k_hash), keys[0], keys[-1])
            reg.put_index(num, encode_index(list(zip(f.firsts, f.offs))))
            first_block[slot] = at_block
            at_block += len(f.blens)
        cap = reg.max_candidates()  # the registry is rebuilt here, not under the delay
        assert cap == 3
        arrays = [gref.run_arrays(t) for t in tables]
        runs, indexes = [], []
        for a in arrays:
            run = seb.dev_run(sl.to_dev(torch, a[0]), sl.to_dev(torch, a[1]), sl.to_dev(torch, a[3]), sl.to_dev(torch, a[4]),
                              sl.to_dev(torch, a[5]))
            ix = torch.zeros(seb.dev_run_index_size(run.n), dtype=torch.uint8, device="cuda")
            seb.dev_run_index(run, ix)
            runs.append(run), indexes.append(ix)
        # the batch: every kind of key; the poison is another draw of the same size
        universe = np.concatenate([np.arange(0, 4300), np.arange(5000, 5200), np.arange(6000, 6100), np.arange(9000, 9050)])

        def batch():
            probes = [key(int(i)) for i in rng.choice(universe, N, replace=False)]
            got = [pref.lsm_get(tables, files, p) for p in probes]
            return probes, got, (np.array([g[0] for g in got], np.uint8), np.array([g[1] for g in got], np.uint8),
                                 np.array([len(g[2]) if g[0] == pref.GET_FOUND else 0 for g in got], np.uint32))

        probes, want, want_arr = batch()
        probes_p, _, want_arr_p = batch()
        sl.differ(want_arr, want_arr_p, ("status", "source", "vlen"))
        assert {(1, 0), (0, 0), (1, 1), (0, 1)} <= {(w[0], w[1]) for w in want}
        n = N
        want_m = sum(1 for p in probes if gref.lsm_get_memtables(tables, p)[0] == gref.NONE)

        def block_ids(cand, blocks):
            """The torch glue between locate and search: block ids in the pool of data sections."""
            first = first_block[cand.to(torch.int64) & 0xFFFF]
            return torch.where((blocks == -1) | (first < 0), torch.full_like(blocks, -1), first + blocks // 4096).to(torch.int32)

        # torch loads each of its kernels on first use, which takes longer than any delay: the glue and the fills run once here
        block_ids(torch.zeros(cap, dtype=torch.int16, device="cuda"), torch.zeros(cap, dtype=torch.int64, device="cuda"))
        for dt in (torch.uint8, torch.int16, torch.int32, torch.int64):
            torch.zeros(4, dtype=dt, device="cuda"), torch.full((4,), 0x7E, dtype=dt, device="cuda")
        L = rig.session()
        dk = seb.dev_keys(L.inp(np.frombuffer(b"".join(probes), np.uint8), np.frombuffer(b"".join(probes_p), np.uint8)), n=n, stride=16)
        mem_status, mem_run, mem_vloc, mem_vlen = L.out(n, np.uint8), L.out(n, np.uint8), L.out(n, np.uint64), L.out(n, np.uint32)
        b_out = [L.out(n, t) for t in (np.uint8, np.uint8, np.uint16, np.uint64, np.uint32)]
        ws = torch.zeros(seb.dev_get_compact_workspace_size(n), dtype=torch.uint8, device="cuda")
        L.arm()
        with torch.cuda.stream(L.S):
            assert torch.cuda.current_stream().cuda_stream == L.S.cuda_stream
            seb.dev_runs_search(dk, runs, indexes, mem_status.t, run=mem_run.t, vloc=mem_vloc.t, vlen=mem_vlen.t)
            L.busy("dev_runs_search")
            plan = seb.dev_get_compact_plan(dk, mem_status.t, ws)  # blocks through the delay and the late copy
            assert L.gate.query() is True
            m = plan.undecided
            assert plan.as_tuple() == (n, want_m, 16 * want_m), "the plan's sizes"
            # everything sized by the plan is made on S; a second delay keeps S busy for the calls that follow
            ckeys, row = torch.zeros(16 * m, dtype=torch.uint8, device="cuda"), torch.zeros(m, dtype=torch.int32, device="cuda")
            cand = torch.zeros(m * cap, dtype=torch.int16, device="cuda")
            blocks = torch.zeros(m * cap, dtype=torch.int64, device="cuda")
            cells = torch.zeros(m * cap, dtype=torch.int32, device="cuda")
            status = torch.full((m,), 0x7E, dtype=torch.uint8, device="cuda")
            col = torch.zeros(m, dtype=torch.int16, device="cuda")
            vloc, vlen = torch.zeros(m, dtype=torch.int64, device="cuda"), torch.zeros(m, dtype=torch.int32, device="cuda")
            L.arm(sync=False)
            ck, _ = seb.dev_get_compact_emit(dk, mem_status.t, plan, ws, ckeys, None, row)
            L.busy("dev_get_compact_emit")
            reg.multiget_list_dev(ck, cand, cap)
            L.busy("multiget_list_dev")
            reg.locate_dev(ck, cand, blocks, cap)
            L.busy("locate_dev")
            bid = block_ids(cand, blocks)
            seb.dev_search_blocks(ck, bid, cap, dpool, dblen, cells)
            L.busy("dev_search_blocks")
            seb.dev_resolve_rows(cells, bid, m, cap, status, col, vloc, vlen)
            L.busy("dev_resolve_rows")
            seb.dev_get_join_rows(mem_status.t, n, row, m, status, *[o.t for o in b_out], mem_vloc=mem_vloc.t,
                                  mem_vlen=mem_vlen.t, sst_col=col, sst_vloc=vloc, sst_vlen=vlen)
            L.busy("dev_get_join_rows")
        L.finish()
        b_status, b_source, b_col, b_vloc, b_vlen = (o.get(nm) for o, nm in zip(b_out, pref.NAMES))
        sl.same(b_status, want_arr[0], "status")
        sl.same(b_source, want_arr[1], "source")
        sl.same(b_vlen, want_arr[2], "vlen")
        hrun = mem_run.get("mem_run")
        vals = [a[2] for a in arrays]
        for i, (st, source, value) in enumerate(want):
            if st == pref.GET_FOUND:
                src_bytes = pool if source == 1 else vals[hrun[i]]
                assert src_bytes[int(b_vloc[i]): int(b_vloc[i]) + int(b_vlen[i])].tobytes() == value, i
                assert (b_col[i] == 0xFFFF) == (source == 0), i
            else:
                assert (int(b_col[i]), int(b_vloc[i])) == (0xFFFF, 0), i
    finally:
        torch.cuda.synchronize()
        reg.close()


# ------------------------------------------------------------------ 12. two side streams at once

def test_two_side_streams_interleaved(seb, torch_cuda, rig, phased):
    """A smoke check for state shared between streams: from one host thread, the phased probe on S1 and the
    compaction and the runs search on S2, call by call, three rounds, the probe batch larger each round so that S1's
    scratch grows.  No delay and no late input here: how the two streams' work interleaves on the GPU is not
    controlled, so a pass shows only that nothing obvious is shared.  All answers against the references."""
    torch = torch_cuda
    k = phased["k"]
    g = getpath_data(121, "fixed16")
    d = memget_data(122)
    L = rig.session()
    S1, S2 = rig.stream, torch.cuda.Stream()
    words = sl.to_dev(torch, words_of(seb, phased["bits"], M_PHASED))
    n, m = g["n"], g["sizes"][1]
    gk = seb.dev_keys(sl.to_dev(torch, np.frombuffer(b"".join(g["keys"]), np.uint8)), n=n, stride=16)
    gmem = sl.to_dev(torch, g["mem"])
    runs, indexes = [], []
    for t in d["good"]:
        a = gref.run_arrays(t)
        run = seb.dev_run(sl.to_dev(torch, a[0]), sl.to_dev(torch, a[1]), sl.to_dev(torch, a[3]), sl.to_dev(torch, a[4]),
                          sl.to_dev(torch, a[5]), n=len(a[1]) - 1, key_bytes=a[0].size)
        ix = torch.zeros(seb.dev_run_index_size(run.n), dtype=torch.uint8, device="cuda")
        seb.dev_run_index(run, ix)
        runs.append(run), indexes.append(ix)
    pdata, poff = pack(d["probes"])
    mk = seb.dev_keys(sl.to_dev(torch, pdata), sl.to_dev(torch, poff))
    rounds = []
    for nb, good, _, want in phased["batches"]:
        rounds.append(dict(pk=seb.dev_keys(sl.to_dev(torch, good), n=nb, stride=16), nb=nb, want=want,
                           probe=[L.out(nb, np.uint8), L.out(nb, np.uint8)], compact=compact_outs(L, g),
                           ws=torch.zeros(seb.dev_get_compact_workspace_size(n), dtype=torch.uint8, device="cuda"),
                           search=[L.out(N, t) for t in (np.uint8, np.uint8, np.uint32, np.uint64, np.uint32, np.uint64)]))
    torch.cuda.synchronize()
    held = []
    for r in rounds:
        seb.dev_probe(r["pk"], words, M_PHASED, k, r["probe"][0].t, stream=S1)
        plan = seb.dev_get_compact_plan(gk, gmem, r["ws"], stream=S2)
        assert plan.as_tuple() == g["sizes"]
        seb.dev_probe(r["pk"], words, M_PHASED, k, r["probe"][1].t, stream=S1)
        okeys, ooff, row = r["compact"]
        seb.dev_get_compact_emit(gk, gmem, plan, r["ws"], okeys.t, None, row.t, stream=S2)
        seb.dev_runs_search(mk, runs, indexes, *[o.t for o in r["search"]], stream=S2)
        held.append(seb.workspace_bytes())
    S1.synchronize()
    S2.synchronize()
    assert held[0] < held[1] < held[2], "the probe's scratch did not grow from round to round"
    for j, r in enumerate(rounds):
        for o in r["probe"]:
            sl.same(o.get(), r["want"], f"round {j}: probe")
        check_compact(g, *r["compact"])
        gref.assert_same([o.get(nm) for o, nm in zip(r["search"], gref.NAMES)], d["want"], f"round {j}: runs_search")
