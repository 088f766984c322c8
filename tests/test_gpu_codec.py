"""GPU parity for SURVEY.md §8(f) row 4 through the C ABI: shard routing (FNV-1a 32,
hashindex/shard.go:47-52), the stable shard partition (UpdateBatch's distribution,
hashindex/shard.go:104-122) and WAL record CRC32-IEEE compute / seal / verify (lsm/wal.go:31-62,
98-133), each against oracle/codec_oracle.c element for element.

Routing: every key layout, the fixed-16 one also at device leads of 1, 4 and 8 bytes (the form that does not take the
uint4 load), and k_route's grid-stride loop under the option grid_cap at 1 and 2.  Partition: tile boundaries at one
and two tiles, 4,096 bins (16 per lane of the scatter), a wave whose 1,024 keys share one shard, a last tile of
exactly 64 keys, and 4096 * 1024 + 4097 keys: 1,026 tiles, the one shape at which k_route_scan_rows carries from a
stretch of 1,024 tiles into the next.  WAL checksums: crc_ref's cases (every length 0..70 at every alignment on the
staged and on the direct path, spans of 36,863 / 36,864 / 36,865 bytes at device leads 0, 1 and 15, staged and
unstaged workgroups in turn) in all three modes, inputs and outputs between guard bytes."""
import zlib

import numpy as np
import pytest

from oracle import codec_c as cc
import crc_ref as cr
import keygen as kg
import stream_late as sl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def to_dev(torch, arr):
    return torch.from_numpy(np.array(arr, copy=True)).cuda()


def _varlen(rng, n, maxlen=90):
    keys = [bytes(rng.integers(0, 256, int(rng.integers(0, maxlen)), dtype=np.uint8)) for _ in range(n)]
    off = np.zeros(n + 1, np.uint64)
    np.cumsum([len(k) for k in keys], out=off[1:])
    return np.frombuffer(b"".join(keys) or b"\0", np.uint8), off


def _route_layout(torch, seb, layout, n, rng):
    """(seb_keys, the oracle's hashes) of n keys in `layout`.  fixed16_leadL: the stride-16 batch L bytes off a
    16-byte boundary, which goes through fnv32a_range and not through one uint4 load per key."""
    if layout.startswith("fixed16"):
        lead = int(layout[len("fixed16_lead"):] or 0)
        data = kg.key16(np.arange(n))
        view = sl.lead_view(torch, data, lead)
        assert view.data_ptr() % 16 == lead
        return seb.dev_keys(view, n=n, stride=16), cc.fnv32a_batch(data, n, stride=16)
    if layout == "stride13":
        data = rng.integers(0, 256, (n, 13), dtype=np.uint8)
        return seb.dev_keys(to_dev(torch, data.ravel()), n=n, stride=13), cc.fnv32a_batch(data, n, stride=13)
    if layout == "varlen":
        data, off = _varlen(rng, n)
        return seb.dev_keys(to_dev(torch, data), to_dev(torch, off.view(np.int64))), cc.fnv32a_batch(data, n, offsets=off)
    assert layout == "empty_keys"
    off = np.zeros(n + 1, np.uint64)
    return seb.dev_keys(to_dev(torch, np.zeros(1, np.uint8)), to_dev(torch, off.view(np.int64))), np.full(n, 0x811C9DC5, np.uint32)


@pytest.mark.parametrize("layout", ["fixed16", "fixed16_lead1", "fixed16_lead4", "fixed16_lead8", "stride13", "varlen",
                                    "empty_keys"])
@pytest.mark.parametrize("bits", [0, 8, 16])
def test_shard_route_matches_oracle(seb, torch_cuda, layout, bits):
    torch = torch_cuda
    n = 5003
    kd, want = _route_layout(torch, seb, layout, n, np.random.default_rng(11))
    shard = torch.zeros(n, dtype=torch.int16, device="cuda")
    h = torch.zeros(n, dtype=torch.int32, device="cuda")
    seb.dev_shard_route(kd, bits, shard, h)
    torch.cuda.synchronize()
    assert np.array_equal(h.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(shard.cpu().numpy().view(np.uint16), (want & ((1 << bits) - 1)).astype(np.uint16))


@pytest.mark.parametrize("layout", ["fixed16", "fixed16_lead1", "fixed16_lead4", "fixed16_lead8", "stride13", "varlen"])
def test_route_under_a_grid_cap(seb, torch_cuda, layout):
    """k_route at 1 and 2 workgroups: 1,300 keys take its grid-stride loop through six and three trips, the last one
    partial; shard and hash equal the oracle's and the default grid's, and nothing outside them is written."""
    torch = torch_cuda
    n, bits = 1300, 8
    assert 1024 < n < 1536
    kd, want = _route_layout(torch, seb, layout, n, np.random.default_rng(17))
    assert (want[1024:] != 0x811C9DC5).any() and len(set(want[1024:].tolist())) > 200, "the later trips hash real keys"
    runs = {}
    for cap in sl.CAPS:
        shard, h = sl.Out(torch, n, np.uint16), sl.Out(torch, n, np.uint32)
        with sl.grid_cap(seb, cap):
            seb.dev_shard_route(kd, bits, shard.t, h.t)
            torch.cuda.synchronize()
        runs[cap] = (shard.get("shard"), h.get("hash"))
        sl.same(runs[cap][1], want, f"cap {cap}: hash")
        sl.same(runs[cap][0], (want & 255).astype(np.uint16), f"cap {cap}: shard")
    assert all(a.tobytes() == b.tobytes() for cap in (1, 2) for a, b in zip(runs[cap], runs[None]))


@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097, 8191, 8193, 100_003])
@pytest.mark.parametrize("bits", [0, 1, 8, 12])
def test_shard_partition_matches_oracle(seb, torch_cuda, n, bits):
    torch = torch_cuda
    data = kg.key16(np.arange(n)) if n else np.zeros((1, 16), np.uint8)
    kd = seb.dev_keys(to_dev(torch, data), n=n, stride=16)
    perm = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
    begin = torch.zeros((1 << bits) + 1, dtype=torch.int64, device="cuda")
    shard = torch.zeros(max(n, 1), dtype=torch.int16, device="cuda")
    seb.dev_shard_partition(kd, bits, perm, begin, shard)
    torch.cuda.synchronize()
    want_shard = (cc.fnv32a_batch(data, n, stride=16) & ((1 << bits) - 1)).astype(np.uint16)
    want_perm, want_begin = cc.partition(want_shard, bits)
    assert np.array_equal(begin.cpu().numpy().view(np.uint64), want_begin)
    if n:
        assert np.array_equal(perm.cpu().numpy().view(np.uint32)[:n], want_perm)
        assert np.array_equal(shard.cpu().numpy().view(np.uint16)[:n], want_shard)


def test_shard_partition_skewed_and_varlen(seb, torch_cuda):
    """One shard holding almost every key (identical keys) and variable-length keys."""
    torch = torch_cuda
    rng = np.random.default_rng(12)
    keys = [b"same-key"] * 9000 + [bytes(rng.integers(0, 256, 20, dtype=np.uint8)) for _ in range(1000)]
    rng.shuffle(keys)
    off = np.zeros(len(keys) + 1, np.uint64)
    np.cumsum([len(k) for k in keys], out=off[1:])
    data = np.frombuffer(b"".join(keys), np.uint8)
    kd = seb.dev_keys(to_dev(torch, data), to_dev(torch, off.view(np.int64)))
    n = len(keys)
    perm = torch.zeros(n, dtype=torch.int32, device="cuda")
    begin = torch.zeros(257, dtype=torch.int64, device="cuda")
    seb.dev_shard_partition(kd, 8, perm, begin)
    torch.cuda.synchronize()
    want_perm, want_begin = cc.partition((cc.fnv32a_batch(data, n, offsets=off) & 255).astype(np.uint16), 8)
    assert np.array_equal(perm.cpu().numpy().view(np.uint32), want_perm)
    assert np.array_equal(begin.cpu().numpy().view(np.uint64), want_begin)


def _partition_check(torch, seb, data, n, bits, want_hash=None):
    """seb_dev_shard_partition of n stride-16 keys into guarded outputs against fnv32a_batch + partition."""
    d = to_dev(torch, data)
    assert d.data_ptr() % 16 == 0
    kd = seb.dev_keys(d, n=n, stride=16)
    perm, begin, shard = sl.Out(torch, n, np.uint32), sl.Out(torch, (1 << bits) + 1, np.uint64), sl.Out(torch, n, np.uint16)
    seb.dev_shard_partition(kd, bits, perm.t, begin.t, shard.t)
    torch.cuda.synchronize()
    want_hash = cc.fnv32a_batch(data, n, stride=16) if want_hash is None else want_hash
    want_shard = (want_hash & ((1 << bits) - 1)).astype(np.uint16)
    want_perm, want_begin = cc.partition(want_shard, bits)
    sl.same(begin.get("shard_begin"), want_begin, "shard_begin")
    sl.same(perm.get("perm"), want_perm, "perm")
    sl.same(shard.get("shard"), want_shard, "shard")


def _keys_by_shard(rng, bits, candidates=400_000):
    """Random 16-byte keys and their shard, to pick keys of a chosen shard from."""
    pool = rng.integers(0, 256, (candidates, 16), dtype=np.uint8)
    return pool, cc.fnv32a_batch(pool, candidates, stride=16) & ((1 << bits) - 1)


def test_shard_partition_one_wave_in_one_shard(seb, torch_cuda):
    """Two tiles at 256 bins; in the second, all 1,024 keys of wave 2 fall in shard 7 (every row of the wave is one
    peer group of 64) while the other three waves are spread."""
    rng = np.random.default_rng(18)
    pool, sh = _keys_by_shard(rng, 8)
    n, a = 2 * 4096, 4096 + 2 * 1024
    data = pool[:n].copy()
    data[a: a + 1024] = pool[n:][sh[n:] == 7][:1024]
    want = cc.fnv32a_batch(data, n, stride=16) & 255
    assert (want[a: a + 1024] == 7).all()
    for w in (0, 1, 3):
        assert len(set(want[4096 + w * 1024: 4096 + (w + 1) * 1024].tolist())) > 200
    _partition_check(torch_cuda, seb, data, n, 8)


@pytest.mark.parametrize("bits", [8, 12])
def test_shard_partition_last_tile_of_64_keys(seb, torch_cuda, bits):
    """4096 + 64 keys: in the last tile one row of one wave is live and nothing else."""
    n = 4096 + 64
    assert n % 4096 == 64
    _partition_check(torch_cuda, seb, kg.key16(np.arange(n)), n, bits)


CARRY_N = 4096 * 1024 + 4097


@pytest.fixture(scope="module")
def carry_keys():
    """CARRY_N stride-16 keys, made once: the bench's keys for the first 1,024 tiles; tile 1,024 holds one key of
    every one of the 4,096 shards (chosen by hash from later keys of the same generator), tile 1,025 one key."""
    tail0 = 4096 * 1024
    data = kg.key16(np.arange(CARRY_N))
    pool = kg.key16(np.arange(CARRY_N, CARRY_N + 200_000))
    sh = cc.fnv32a_batch(pool, len(pool), stride=16) & 4095
    firsts = np.unique(sh, return_index=True)[1]
    assert firsts.size == 4096
    data[tail0: tail0 + 4096] = pool[np.random.default_rng(19).permutation(firsts)]
    return data, cc.fnv32a_batch(data, CARRY_N, stride=16)


@pytest.mark.parametrize("bits", [1, 8, 12])
def test_shard_partition_scan_carry(seb, torch_cuda, carry_keys, bits):
    """1,026 tiles: k_route_scan_rows scans every bin's row in two stretches, and the prefixes of tiles 1,024 and
    1,025 are the first stretch's total (the carry) plus their own.  Every bin has keys in those tiles, so a lost
    carry would misplace keys of every bin."""
    data, want_hash = carry_keys
    ntiles = (CARRY_N + 4095) // 4096
    assert ntiles == 1026 > 1024
    tail = (want_hash[1024 * 4096:] & ((1 << bits) - 1)).astype(np.int64)
    assert np.bincount(tail, minlength=1 << bits).all(), "a bin without a key in tiles 1024 and up"
    _partition_check(torch_cuda, seb, data, CARRY_N, bits, want_hash)


def _wal_varied(rng, n):
    """Records with value sizes 0..5000 (small, unaligned, large) in Append's layout."""
    recs = []
    for i in range(n):
        key = bytes(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8))
        vs = int(rng.choice([0, 1, 3, 7, 100, 1000, 5000]))
        val = bytes(rng.integers(0, 256, vs, dtype=np.uint8))
        body = (i + 1).to_bytes(8, "little") + len(key).to_bytes(4, "little") + vs.to_bytes(4, "little") + \
            bytes([i % 3 == 0]) + key + val
        recs.append(zlib.crc32(body).to_bytes(4, "little") + body)
    off = np.zeros(n + 1, np.uint64)
    np.cumsum([len(r) for r in recs], out=off[1:])
    return np.frombuffer(b"".join(recs), np.uint8).copy(), off


@pytest.mark.parametrize("kind", ["bench_layout", "varied"])
def test_wal_crc_seal_verify(seb, torch_cuda, kind):
    torch = torch_cuda
    rng = np.random.default_rng(13)
    img, off = kg.wal_image(20000, value_size=100) if kind == "bench_layout" else _wal_varied(rng, 3000)
    n = off.size - 1
    want_crc, want_ok = cc.wal_crc(img, off)
    assert want_ok.all()
    d_img, d_off = to_dev(torch, img), to_dev(torch, off.view(np.int64))
    crc = torch.zeros(n, dtype=torch.int32, device="cuda")
    ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    seb.dev_wal_crc(d_img, d_off, seb.WAL_VERIFY, crc, ok)
    torch.cuda.synchronize()
    assert np.array_equal(crc.cpu().numpy().view(np.uint32), want_crc)
    assert ok.cpu().numpy().all()
    # seal: clear every CRC field, seal on the device, get the original image back
    blank = img.copy()
    st = off[:-1].astype(np.int64)
    for b in range(4):
        blank[st + b] = 0
    d_blank = to_dev(torch, blank)
    seb.dev_wal_crc(d_blank, d_off, seb.WAL_SEAL)
    torch.cuda.synchronize()
    assert np.array_equal(d_blank.cpu().numpy(), img)


def test_wal_verify_flags_exactly_the_corrupt_records(seb, torch_cuda):
    torch = torch_cuda
    img, off = kg.wal_image(5000, value_size=100)
    img = img.copy()
    st = off.astype(np.int64)
    bad = {17: 40, 999: 0, 2500: 12, 4999: 136}  # payload, crc field, keySize, last byte of the image
    for r, o in bad.items():
        img[st[r] + o] ^= 0x21
    short = off.copy()
    want_crc, want_ok = cc.wal_crc(img, short)
    assert sorted(np.nonzero(want_ok == 0)[0].tolist()) == sorted(bad)
    crc = torch.zeros(5000, dtype=torch.int32, device="cuda")
    ok = torch.zeros(5000, dtype=torch.uint8, device="cuda")
    seb.dev_wal_crc(to_dev(torch, img), to_dev(torch, short.view(np.int64)), seb.WAL_VERIFY, crc, ok)
    torch.cuda.synchronize()
    assert np.array_equal(ok.cpu().numpy(), want_ok)
    assert np.array_equal(crc.cpu().numpy().view(np.uint32), want_crc)
    # framing violations: a record shorter than its header, and one of 0..3 bytes
    odd = np.array([0, 20, 20, 23, 160], np.uint64)
    ok2 = torch.zeros(4, dtype=torch.uint8, device="cuda")
    crc2 = torch.zeros(4, dtype=torch.int32, device="cuda")
    seb.dev_wal_crc(to_dev(torch, img[:200]), to_dev(torch, odd.view(np.int64)), seb.WAL_VERIFY, crc2, ok2)
    torch.cuda.synchronize()
    w_crc, w_ok = cc.wal_crc(img[:200], odd)
    assert np.array_equal(ok2.cpu().numpy(), w_ok) and not w_ok.any()
    assert np.array_equal(crc2.cpu().numpy().view(np.uint32), w_crc)


# ------------------------------------------------------------------ crc_ref's cases: windows, alignments, short records

WAL_CASES = cr.wal_cases()


def image_at(torch, image, lead):
    """The image on the device between guard bytes, `lead` bytes (mod 16) off a 16-byte boundary."""
    o = sl.Out(torch, image.size, np.uint8, lead=lead)
    assert o.t.data_ptr() % 16 == lead % 16
    o.t.copy_(torch.from_numpy(image.copy()))
    return o


@pytest.mark.parametrize("name", sorted(WAL_CASES))
def test_wal_crc_edge_cases(seb, torch_cuda, name):
    """seb_dev_wal_crc in its three modes on a crc_ref case, at the case's device lead (the sweep and the mixed cases:
    at 0, 1 and 15).  CRC: crc = zlib's.  VERIFY: crc and ok = the rule's, ok = 0 for every record of fewer than 21
    bytes; the image is not written.  SEAL: the CRC field of every record that has one is blanked, and the sealed
    image is the original byte for byte (mixed's flipped records get the checksum of what they now hold), records of
    0..3 bytes and the guards included."""
    torch = torch_cuda
    case = WAL_CASES[name]
    img, off = case["image"], case["off"]
    n = off.size - 1
    lens = np.diff(off.astype(np.int64))
    st = off[:-1].astype(np.int64)
    d_off = sl.to_dev(torch, off)
    for lead in (cr.LEADS if name.startswith(("sweep", "mixed")) else (case["lead"],)):
        cr.assert_case(case, lead)  # the input does what its name says, at this lead
        d_img = image_at(torch, img, lead)
        crc = sl.Out(torch, n, np.uint32)
        seb.dev_wal_crc(d_img.t, d_off, seb.WAL_CRC, crc.t)
        crc2, ok = sl.Out(torch, n, np.uint32), sl.Out(torch, n, np.uint8)
        seb.dev_wal_crc(d_img.t, d_off, seb.WAL_VERIFY, crc2.t, ok.t)
        torch.cuda.synchronize()
        sl.same(crc.get("crc"), case["crc"], f"{name} lead {lead}: crc")
        sl.same(crc2.get("crc"), case["crc"], f"{name} lead {lead}: crc (verify)")
        got_ok = ok.get("ok")
        sl.same(got_ok, case["ok"], f"{name} lead {lead}: ok")
        assert not got_ok[lens < 21].any()
        sl.same(d_img.get("image"), img, f"{name} lead {lead}: the image after CRC and VERIFY")
        blank = img.copy()
        for b in range(4):
            blank[st[lens >= 4] + b] = 0
        assert (blank != img).sum() > n
        # the seal writes the checksum of what the record holds: the original field, but for mixed's flipped records
        sealed = blank.copy()
        for b in range(4):
            sealed[st[lens >= 4] + b] = (case["crc"][lens >= 4] >> (8 * b)) & 0xFF
        changed = np.nonzero(sealed != img)[0]
        assert changed.size == 0 or name.startswith("mixed")
        assert set(np.searchsorted(off, changed, "right") - 1) <= set(np.nonzero((case["ok"] == 0) & (lens >= 21))[0])
        d_blank = image_at(torch, blank, lead)
        seb.dev_wal_crc(d_blank.t, d_off, seb.WAL_SEAL)
        torch.cuda.synchronize()
        sl.same(d_blank.get("sealed image"), sealed, f"{name} lead {lead}: sealed image")
