"""GPU: the Get path's last step (include/seb_bloom.h, "Get values").

seb_dev_get_values_plan + seb_dev_get_values_emit equal the host half (seb_get_values, itself held to values_ref's
restatement in test_values.py) in sizes, out_off and out_vals.  Batch sizes around a wave, around 1, 2 and 4 tiles
of 1024 keys and one that needs two stretches of the tile-sum scan; value lengths around one and two 16-byte
chunks, 4083, one value of 70,000 bytes and one of 3 MiB among 1-byte values (the copy is balanced by output
bytes); out_vals 16-byte aligned and at an odd address, sources at odd addresses, values at byte 0 and at the last
byte of their source; the found patterns of test_gpu_getpath.patterns; pool only, one run only with a null run
array, 8 runs and the pool, a run of no bytes behind a null pointer.  With the option grid_cap at 1 and 2 the copy's
workgroups take 23 groups of 4 KiB in turns.  Outputs start as 0xA5 between 64 guard bytes.
The plan names the lower of two invalid keys in different tiles.  A workspace that is another plan's makes the emit
write nothing, and inputs rewritten between plan and emit leave every guard intact.  One case on a busy side stream
with late inputs, and LSM.Get end to end: the values of every key of a batch over two memtable runs and four
SSTables equal getpath_ref's."""
import numpy as np
import pytest

import getpath_ref as pref
import keygen as kg
import memget_ref as gref
import stream_late as sl
import test_gpu_getpath as tg
import values_ref as vref
from oracle import bloom_np as bn
from oracle import oracle_c as oc

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5
TILE = 1024  # kValTile
INVALID = -1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def lead_view(torch, a, lead):
    """The bytes of `a` on the device, `lead` bytes into a 256-byte aligned allocation (lead 0: 16-byte aligned)."""
    a = np.asarray(a, np.uint8).reshape(-1)
    buf = torch.from_numpy(np.concatenate([np.full(lead, 0xEE, np.uint8), a, np.zeros(1, np.uint8)])).cuda()
    return buf[lead: lead + a.size]


class Dev:
    """A batch (values_ref.make_batch's dict) on the device: the byte arrays and the sources `lead` bytes off."""

    def __init__(self, torch, b, lead=1, run_none=False, val_bytes=None):
        self.n = len(b["status"])
        self.status, self.source = lead_view(torch, b["status"], 3), lead_view(torch, b["source"], 1)
        self.run = None if run_none else lead_view(torch, b["run"], 5)
        self.vloc = torch.from_numpy(np.ascontiguousarray(b["vloc"], np.uint64).view(np.int64).copy()).cuda() if self.n else None
        self.vlen = torch.from_numpy(np.ascontiguousarray(b["vlen"], np.uint32).view(np.int32).copy()).cuda() if self.n else None
        self.vals = [None if v is None else lead_view(torch, v, lead) for v in b["vals"]]
        self.val_bytes = val_bytes if val_bytes is not None else [0 if v is None else len(v) for v in b["vals"]]
        self.pool = None if b["pool"] is None else lead_view(torch, b["pool"], lead)
        self.pool_bytes = 0 if b["pool"] is None else len(b["pool"])
        for t in self.vals + [self.pool]:
            assert t is None or t.numel() == 0 or t.data_ptr() % 16 == lead % 16

    def arrays(self):
        return (self.status, self.source, self.run, self.vloc, self.vlen, self.n, self.vals, self.pool)

    def kw(self):
        return dict(val_bytes=self.val_bytes, pool_bytes=self.pool_bytes)


def guarded(torch, nbytes, lead=0):
    buf = torch.full((GUARD + lead + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD + lead: GUARD + lead + nbytes]


def read_guarded(buf, nbytes, lead, name):
    h = buf.cpu().numpy()
    a, b = GUARD + lead, GUARD + lead + nbytes
    assert (h[:a] == FILL).all() and (h[b:] == FILL).all(), f"bytes outside {name} were written"
    return h[a:b]


def device_values(torch, seb, plan_dev, emit_dev=None, out_lead=0, sizes=None, ws=None):
    """plan on plan_dev, emit on emit_dev (default: the same) into 0xA5 buffers between guards, sized by the plan.
    sizes / ws: another plan's, for the emit.  Returns (sizes tuple, out_off, out_vals) as numpy arrays."""
    d = plan_dev
    n = d.n
    need = seb.dev_get_values_workspace_size(n)
    tiles = (n + TILE - 1) // TILE
    up16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
    assert need == 128 + up16(16 * tiles) + up16(8 * n) + up16(4 * n) + up16(n)
    own_ws = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    plan = seb.dev_get_values_plan(*d.arrays(), own_ws, ws_bytes=need, **d.kw())
    sz = plan if sizes is None else sizes
    obuf, out_off = guarded(torch, 8 * (n + 1))
    vbuf, out_vals = guarded(torch, sz.val_bytes, out_lead)
    assert sz.val_bytes == 0 or out_vals.data_ptr() % 16 == out_lead
    e = d if emit_dev is None else emit_dev
    seb.dev_get_values_emit(*e.arrays(), sz, own_ws if ws is None else ws, out_off, out_vals if sz.val_bytes else None, **e.kw())
    torch.cuda.synchronize()
    assert (own_ws[need:].cpu().numpy() == 0x5A).all(), "the plan or the emit wrote past the workspace"
    off = np.frombuffer(read_guarded(obuf, 8 * (n + 1), 0, "out_off").tobytes(), np.uint64)
    return plan.as_tuple(), off, read_guarded(vbuf, sz.val_bytes, out_lead, "out_vals")


def check(torch, seb, b, what, out_lead=0, lead=1, run_none=False, val_bytes=None):
    args = list(vref.batch_args(b))
    if run_none:
        args[2] = None
    want = seb.get_values(*args, val_bytes=val_bytes)
    got = device_values(torch, seb, Dev(torch, b, lead, run_none, val_bytes), out_lead=out_lead)
    vref.assert_same(got, want, what)
    return want[0]


# ------------------------------------------------------------------ sizes, lengths, alignments

@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049, 4097])
def test_batch_sizes(seb, torch_cuda, n):
    """Mixed sources (two runs and the pool, all at odd addresses), lengths around one and two chunks and 4083;
    out_vals 16-byte aligned and at an odd address."""
    rng = np.random.default_rng(n)
    b = vref.make_batch(rng, n, found=rng.random(n) < 0.7)
    for out_lead in (0, 1):
        sizes = check(torch_cuda, seb, b, f"n={n} out_lead={out_lead}", out_lead)
    assert sizes[1] > 0 or n == 1


@pytest.mark.parametrize("out_lead", [0, 1])
def test_copy_under_a_grid_cap(seb, torch_cuda, out_lead):
    """The copy (k_gv_copy, a workgroup per 4 KiB of output) at 1 and 2 workgroups: each takes several groups in
    turn, restaging its offsets every time; at 2 the last trip is one group.  Sizes, offsets and values equal the
    host half's and the default grid's."""
    torch = torch_cuda
    rng = np.random.default_rng(2)
    b = vref.make_batch(rng, 300, found=rng.random(300) < 0.7)  # 93,649 bytes: 23 groups
    want = seb.get_values(*vref.batch_args(b))
    groups = (out_lead + int(want[0][2]) + 4095) // 4096
    assert groups > 2 * 2 and groups % 2 == 1, groups
    runs = []
    for cap in sl.CAPS:
        with sl.grid_cap(seb, cap):
            got = device_values(torch, seb, Dev(torch, b), out_lead=out_lead)
        vref.assert_same(got, want, f"cap {cap} out_lead={out_lead}")
        runs.append((got[0], got[1].tobytes(), got[2].tobytes()))
    assert runs[1] == runs[0] and runs[2] == runs[0]


def test_two_stretches_of_the_scan(seb, torch_cuda):
    """131,073 keys: 128 tiles + 1.  Values of 0-3 bytes."""
    n = 128 * TILE + 1
    rng = np.random.default_rng(2)
    vals = [rng.integers(0, 256, 5000, dtype=np.uint8), rng.integers(0, 256, 777, dtype=np.uint8)]
    pool = rng.integers(0, 256, 8192, dtype=np.uint8)
    found = rng.random(n) < 0.6
    found[[0, n - 1]] = True
    source = rng.integers(0, 2, n).astype(np.uint8)
    run = rng.integers(0, 2, n).astype(np.uint8)
    size = np.where(source == 1, 8192, np.where(run == 0, 5000, 777))
    vlen = rng.integers(0, 4, n).astype(np.uint32)
    vlen[[0, n - 1]] = 3
    vloc = (rng.integers(0, 2**40, n) % (size - 3)).astype(np.uint64)
    status = np.where(found, 1, rng.choice(np.array([0, 2, 3, 255], np.uint8), n)).astype(np.uint8)
    b = dict(status=status, source=source, run=run, vloc=vloc, vlen=vlen, vals=vals, pool=pool)
    sizes = check(torch_cuda, seb, b, "131073 keys", out_lead=1)
    assert sizes[1] == int(found.sum())


@pytest.mark.parametrize("big", [70_000, 3 << 20])
def test_one_long_value_among_short_ones(seb, torch_cuda, big):
    """The copy is balanced by output bytes: a memtable value of 70,000 bytes, and one of 3 MiB, among 1-byte values.
    No time is asserted; a workgroup that walked the long value alone would run into the test's time limit."""
    rng = np.random.default_rng(big)
    n = 300
    b = vref.make_batch(rng, n, num_runs=2, run_bytes=big + 100, found=np.ones(n, bool), lengths=(1,))
    at = 137
    b["source"][at], b["run"][at], b["vloc"][at], b["vlen"][at] = 0, 1, 33, big
    for out_lead in (0, 1):
        sizes = check(torch_cuda, seb, b, f"one value of {big}", out_lead)
    assert sizes == (n, n, n - 1 + big)


@pytest.mark.parametrize("lead", [0, 1, 9])
def test_first_and_last_bytes_of_a_source(seb, torch_cuda, lead):
    """Values that start at byte 0 of their source and values that end at its last byte (where the aligned word
    that covers a chunk would pass the end), sources 16-byte aligned and at odd addresses."""
    rng = np.random.default_rng(40 + lead)
    vals = [rng.integers(0, 256, 100, dtype=np.uint8), rng.integers(0, 256, 4083, dtype=np.uint8)]
    pool = rng.integers(0, 256, 4096 + 5, dtype=np.uint8)
    rows = []
    for ln in (1, 15, 16, 17, 31, 32, 33, 40):
        rows += [(0, 0, 0, ln), (0, 0, 100 - ln, ln), (1, 0, 0, ln), (1, 0, 4101 - ln, ln), (0, 1, 4083 - ln, ln)]
    rows += [(0, 1, 0, 4083), (0, 0, 0, 100), (1, 0, 0, 4101), (0, 0, 100, 0), (1, 3, 4101, 0)]
    src, run, vloc, vlen = (np.array(c, t) for c, t in zip(zip(*rows), (np.uint8, np.uint8, np.uint64, np.uint32)))
    b = dict(status=np.ones(len(rows), np.uint8), source=src, run=run, vloc=vloc, vlen=vlen, vals=vals, pool=pool)
    for out_lead in (0, 1, 15):
        check(torch_cuda, seb, b, f"lead={lead} out_lead={out_lead}", out_lead, lead)


def test_found_patterns(seb, torch_cuda):
    """None found, all, alternating, only the first, only the last, found runs covering whole waves and whole
    tiles, random fractions: the masks of test_gpu_getpath.patterns."""
    rng = np.random.default_rng(4)
    n = 4097
    for name, mem in tg.patterns(rng, n):
        found = (mem == 1) | (mem == 2)
        b = vref.make_batch(rng, n, found=found, lengths=(0, 1, 15, 16, 17, 33))
        sizes = check(torch_cuda, seb, b, name, out_lead=1)
        assert sizes[1] == int(found.sum())
        if name == "none":
            assert sizes == (n, 0, 0)


def test_sources(seb, torch_cuda):
    rng = np.random.default_rng(5)
    n = 1500
    check(torch_cuda, seb, vref.make_batch(rng, n, num_runs=0, pool_only=True), "pool only")
    b = vref.make_batch(rng, n, num_runs=1, runs_only=True)
    b["pool"] = None
    check(torch_cuda, seb, b, "one run only, run == NULL, no pool", run_none=True)
    b = vref.make_batch(rng, n, num_runs=8)
    assert set(b["run"][(b["status"] == 1) & (b["source"] == 0)]) == set(range(8))
    check(torch_cuda, seb, b, "8 runs and the pool", out_lead=1)
    # run 1 holds no bytes and is a null pointer: only empty values may name it
    b = vref.make_batch(rng, n, num_runs=3)
    named = (b["status"] == 1) & (b["source"] == 0) & (b["run"] == 1)
    assert named.sum() > 20
    b["vloc"][named], b["vlen"][named] = 0, 0
    b["vals"][1] = None
    check(torch_cuda, seb, b, "a run of no bytes behind a null pointer")
    # no key found and no source at all
    b = vref.make_batch(rng, 70, num_runs=0, found=np.zeros(70, bool))
    b["pool"] = None
    assert check(torch_cuda, seb, b, "nothing found, no sources", run_none=True) == (70, 0, 0)


def test_empty_batch_and_argument_refusals(seb, torch_cuda):
    torch = torch_cuda
    L = seb.lib()
    import ctypes as C
    sz = seb.seb_values_sizes(9, 9, 9, 9)
    assert L.seb_dev_get_values_plan(None, None, None, None, None, 0, None, None, 0, None, 0, None, 0, C.byref(sz), None) == 0
    assert (sz.n, sz.found, sz.val_bytes, sz.reserved) == (0, 0, 0, 0)
    assert L.seb_dev_get_values_emit(None, None, None, None, None, 0, None, None, 0, None, 0, C.byref(sz), None, None, None, None) == 0
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    common = (p, p, None, p, p, 4, None, None, 0, None, 0)
    w = p + 1024  # the workspace: the bytes behind the (all zero) input arrays
    assert L.seb_dev_get_values_plan(*common, w, 3072, C.byref(sz), None) == 0 and sz.as_tuple() == (4, 0, 0)
    assert L.seb_dev_get_values_plan(*common, w, 64, C.byref(sz), None) == INVALID          # workspace too small
    assert L.seb_dev_get_values_plan(*common, w + 8, 3000, C.byref(sz), None) == INVALID    # misaligned workspace
    assert L.seb_dev_get_values_plan(*common, None, 3072, C.byref(sz), None) == INVALID
    assert L.seb_dev_get_values_plan(p, p, None, p + 4, p, 4, None, None, 0, None, 0, w, 3072, C.byref(sz), None) == INVALID
    assert L.seb_dev_get_values_plan(p, p, None, p, p, 4, None, None, 0, None, 8, w, 3072, C.byref(sz), None) == INVALID
    assert L.seb_dev_get_values_plan(p, p, None, p, p, 2**32, None, None, 0, None, 0, w, 3072, C.byref(sz), None) == INVALID
    assert L.seb_dev_get_values_plan(p, p, None, p, p, 4, None, None, 9, None, 0, w, 3072, C.byref(sz), None) == INVALID
    ok = seb.seb_values_sizes(4, 0, 0, 0)
    assert L.seb_dev_get_values_emit(*common, C.byref(ok), w, None, None, None) == INVALID  # out_off is required
    assert L.seb_dev_get_values_emit(*common, C.byref(seb.seb_values_sizes(5, 0, 0, 0)), w, p + 512, None, None) == INVALID
    assert L.seb_dev_get_values_emit(*common, C.byref(ok), w, p + 512 + 4, None, None) == INVALID
    torch.cuda.synchronize()


# ------------------------------------------------------------------ refusals and bounds

@pytest.mark.parametrize("kind", ["source", "wrap", "past_pool", "run", "null_vals"])
def test_plan_names_the_lower_of_two_invalid_keys_in_different_tiles(seb, torch_cuda, kind):
    torch = torch_cuda
    rng = np.random.default_rng(6)
    n, lo, hi = 4097, 1500, 3500
    b = vref.make_batch(rng, n, num_runs=3, lengths=(0, 1, 17))
    val_bytes = None
    for i in (lo, hi):
        b["status"][i] = 1
        if kind == "source":
            b["source"][i] = 2
        elif kind == "wrap":
            b["source"][i], b["vloc"][i], b["vlen"][i] = 1, 2**64 - 1, 2
        elif kind == "past_pool":
            b["source"][i], b["vloc"][i], b["vlen"][i] = 1, len(b["pool"]) - 9, 10
        elif kind == "run":
            b["source"][i], b["run"][i], b["vloc"][i], b["vlen"][i] = 0, 3, 0, 0
        else:
            b["source"][i], b["run"][i], b["vloc"][i], b["vlen"][i] = 0, 1, 0, 0
    if kind == "null_vals":
        named = (b["status"] == 1) & (b["source"] == 0) & (b["run"] == 1)
        named[[lo, hi]] = False
        b["status"][named] = 0
        val_bytes = [len(b["vals"][0]), 64, len(b["vals"][2])]
        b["vals"][1] = None
    assert vref.lowest_invalid(*vref.batch_args(b), val_bytes=val_bytes) == lo
    d = Dev(torch, b, val_bytes=val_bytes)
    ws = torch.zeros(seb.dev_get_values_workspace_size(n), dtype=torch.uint8, device="cuda")
    with pytest.raises(seb.SebError) as e:
        seb.dev_get_values_plan(*d.arrays(), ws, **d.kw())
    assert e.value.code == INVALID and f"key {lo} " in str(e.value), str(e.value)
    # no emit may follow: one made all the same, with sizes that would fit, writes nothing
    obuf, out_off = guarded(torch, 8 * (n + 1))
    seb.dev_get_values_emit(*d.arrays(), seb.seb_values_sizes(n, 0, 0, 0), ws, out_off, None, **d.kw())
    torch.cuda.synchronize()
    assert (obuf.cpu().numpy() == FILL).all()
    # with the lower key carrying nothing, the plan names the other
    b["status"][lo] = 0
    d = Dev(torch, b, val_bytes=val_bytes)
    with pytest.raises(seb.SebError) as e:
        seb.dev_get_values_plan(*d.arrays(), ws, **d.kw())
    assert f"key {hi} " in str(e.value)


def test_another_plans_workspace_writes_nothing(seb, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(7)
    n = 2049
    b1 = vref.make_batch(rng, n, lengths=(1, 16, 33))
    b2 = vref.make_batch(rng, n, lengths=(0, 15, 40))
    d1, d2 = Dev(torch, b1), Dev(torch, b2)
    ws2 = torch.zeros(seb.dev_get_values_workspace_size(n), dtype=torch.uint8, device="cuda")
    plan2 = seb.dev_get_values_plan(*d2.arrays(), ws2, **d2.kw())
    want1 = seb.get_values(*vref.batch_args(b1))
    assert plan2.as_tuple() != want1[0]
    # b1's plan and sizes with b2's workspace: every output byte keeps its fill
    _, off, vals = device_values(torch, seb, d1, ws=ws2)
    assert (off.view(np.uint8) == FILL).all() and (vals == FILL).all()
    # b2's sizes with b1's own workspace: the same
    _, off, vals = device_values(torch, seb, d1, sizes=plan2)
    assert (off.view(np.uint8) == FILL).all() and (vals == FILL).all()
    # a workspace of zeros (no plan at all)
    _, off, vals = device_values(torch, seb, d1, ws=torch.zeros_like(ws2))
    assert (off.view(np.uint8) == FILL).all() and (vals == FILL).all()


def test_inputs_rewritten_between_plan_and_emit_stay_inside_the_outputs(seb, torch_cuda):
    """vlen raised and status flipped to FOUND after the plan: the output may be wrong, every guard is intact
    (device_values checks them) and out_off stays inside [0, val_bytes].  The keys that carry nothing hold zeros
    here, and the raised lengths pass their source's end by at most 40 bytes: only writes are under test."""
    torch = torch_cuda
    rng = np.random.default_rng(8)
    for n in (700, 4097):
        b = vref.make_batch(rng, n, garbage=False, lengths=(0, 1, 16, 33, 200))
        e = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()}
        was_found = b["status"] == 1
        e["vlen"][was_found] += rng.integers(1, 41, int(was_found.sum())).astype(np.uint32)
        flip = ~was_found & (rng.random(n) < 0.5)
        e["status"][flip] = 1
        e["source"][flip], e["run"][flip], e["vloc"][flip] = 1, 0, rng.integers(0, 4096, int(flip.sum()))
        e["vlen"][flip] = rng.integers(0, 300, int(flip.sum()))
        for out_lead in (0, 1):
            sizes, off, vals = device_values(torch, seb, Dev(torch, b), Dev(torch, e), out_lead)
            assert off[0] == 0 and off[-1] == sizes[2] and (off <= sizes[2]).all()
        # and shrunk: fewer bytes than the plan counted
        e2 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()}
        e2["status"][was_found & (rng.random(n) < 0.5)] = 0
        sizes, off, vals = device_values(torch, seb, Dev(torch, b), Dev(torch, e2), 1)
        assert (off <= sizes[2]).all()


# ------------------------------------------------------------------ a busy side stream, late inputs

@pytest.fixture(scope="module")
def rig(seb, torch_cuda):
    try:
        r = sl.Rig(torch_cuda, seb)
    except AssertionError as e:
        pytest.fail(f"stream control: {e}")
    return r


def test_plan_and_emit_on_a_busy_side_stream(seb, torch_cuda, rig):
    """The five input arrays arrive late before the plan, the source bytes late before the emit."""
    torch = torch_cuda
    rng = np.random.default_rng(9)
    n = 2049
    good = vref.make_batch(rng, n, num_runs=2, lengths=(0, 1, 16, 33, 100))
    poison = vref.make_batch(rng, n, num_runs=2, lengths=(0, 5, 40))   # valid over sources of the same sizes
    pvals = [rng.integers(0, 256, len(v), dtype=np.uint8) for v in good["vals"]]
    ppool = rng.integers(0, 256, len(good["pool"]), dtype=np.uint8)
    want = seb.get_values(*vref.batch_args(good))
    wrong = seb.get_values(*vref.batch_args(dict(good, vals=pvals, pool=ppool)))
    sl.differ(want[1:], seb.get_values(*vref.batch_args(poison))[1:], ["out_off", "out_vals"])
    sl.differ(want[2:], wrong[2:], ["out_vals"])
    L = rig.session()
    five = [L.inp(good[k], poison[k]) for k in ("status", "source", "run", "vloc", "vlen")]
    dvals = [sl.to_dev(torch, p) for p in pvals]
    dpool = sl.to_dev(torch, ppool)
    ws = torch.zeros(seb.dev_get_values_workspace_size(n), dtype=torch.uint8, device="cuda")
    L.arm()
    plan = L.plan(seb.dev_get_values_plan, *five, n, dvals, dpool, ws)
    assert plan.as_tuple() == want[0], "the plan's sizes"
    out_off, out_vals = L.out(n + 1, np.uint64), L.out(want[0][2], np.uint8, lead=1)
    for live, g in zip(dvals + [dpool], good["vals"] + [good["pool"]]):
        L.pairs.append((sl.to_dev(torch, g), live))
    L.arm()
    L.call(seb.dev_get_values_emit, *five, n, dvals, dpool, plan, ws, out_off.t, out_vals.t)
    L.finish()
    sl.same(out_off.get("out_off"), want[1], "out_off")
    sl.same(out_vals.get("out_vals"), want[2], "out_vals")


# ------------------------------------------------------------------ end to end

def test_end_to_end_values(seb, torch_cuda):
    """LSM.Get, value bytes included, over two memtable runs and four SSTables (two overlapping L0 files with
    tombstones over L1 values, two disjoint L1 files) built by the library's device builder, their data sections
    as the block pool: runs search, compact, list, locate, search, resolve, join rows (pipeline B of
    test_gpu_getpath.test_end_to_end), then plan + emit.  Every key's span of out_vals equals getpath_ref's value
    and is empty where LSM.Get returns none."""
    torch = torch_cuda
    rng = np.random.default_rng(32)
    key = kg.key16_bytes
    val = lambda tag, i: tag + b"%d" % i + bytes(rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8))  # noqa: E731
    l1 = [[(key(i), val(b"l1-", i), 0) for i in range(0, 1000, 2)], [(key(i), val(b"l1-", i), 0) for i in range(1000, 2000, 2)]]
    l0a = [(key(i), val(b"l0a-", i), 1 if i % 12 == 0 else 0) for i in range(0, 2000, 6)]     # tombstones over L1 values
    l0b = [(key(i), val(b"l0b-", i), 0) for i in range(1, 2100, 14)]                           # odd keys: only here
    file_items = [(100, 0, l0a), (101, 0, l0b), (200, 1, l1[0]), (201, 1, l1[1])]
    active = gref.table_from_ops(
        [(key(i), val(b"act-", i), 5000 + i, 0) for i in range(4, 2000, 40)] +          # values over SSTable keys
        [(key(i), b"", 6000 + i, 1) for i in range(8, 2000, 40)] +                       # tombstones over SSTable values
        [(key(i), b"", 6500 + i, 0) for i in range(12, 2000, 120)] +                     # empty values: found, no bytes
        [(key(i), val(b"act-", i), 7000 + i, 0) for i in range(5001, 5100, 2)])          # only in the active run
    frozen = gref.table_from_ops(
        [(key(i), val(b"imm-", i), 100 + i, 0) for i in range(4, 2000, 80)] +            # hidden by the active run
        [(key(i), val(b"imm-", i), 200 + i, 0) for i in range(16, 2000, 40)] +           # only in the immutable run
        [(key(i), b"", 300 + i, 1) for i in range(24, 2000, 40)] +
        [(key(i), val(b"imm-", i), 400 + i, 0) for i in range(6001, 6050, 2)])
    tables = [active, frozen]
    files = [pref.File(num, level, items) for num, level, items in file_items]

    items = [it for _, _, its in file_items for it in its]
    file_begin = np.concatenate([[0], np.cumsum([len(its) for _, _, its in file_items])]).tolist()
    kd = torch.from_numpy(np.frombuffer(b"".join(k for k, _, _ in items), np.uint8).copy()).cuda()
    bk = seb.dev_keys(kd, n=len(items), stride=16)
    voff = np.concatenate([[0], np.cumsum([len(v) for _, v, _ in items])]).astype(np.uint64)
    dvals = torch.from_numpy(np.frombuffer(b"".join(v for _, v, _ in items), np.uint8).copy()).cuda()
    dvoff = tg.u64_dev(torch, voff)
    ddel = torch.from_numpy(np.array([d for _, _, d in items], np.uint8)).cuda()
    bws = torch.zeros(seb.dev_sst_workspace_size(len(items), 4), dtype=torch.uint8, device="cuda")
    sizes = seb.dev_sst_plan(bk, dvoff, file_begin, bws)
    nblocks = sum(s[0] for s in sizes)
    dpool = torch.zeros(sum(s[1] for s in sizes), dtype=torch.uint8, device="cuda")
    dindex = torch.zeros(sum(s[2] for s in sizes), dtype=torch.uint8, device="cuda")
    dmeta = torch.zeros(sum(s[3] for s in sizes), dtype=torch.uint8, device="cuda")
    dblen = torch.zeros(nblocks, dtype=torch.int16, device="cuda")
    seb.dev_sst_encode(bk, dvals, dvoff, ddel, file_begin, sizes, bws, dpool, dindex, dmeta, dblen)
    torch.cuda.synchronize()
    index = dindex.cpu().numpy().tobytes()
    assert dpool.cpu().numpy().tobytes() == b"".join(f.data for f in files)
    reg = seb.Registry(0)
    first_block = torch.full((65536,), -1, dtype=torch.int64, device="cuda")
    at_index = at_block = 0
    for (num, level, its), s in zip(file_items, sizes):
        keys = [k for k, _, _ in its]
        m_bits, k_hash = oc.params(len(keys), 0.01)
        bits = oc.build(m_bits, k_hash, np.frombuffer(b"".join(keys), np.uint8), len(keys), stride=16)
        slot = reg.put(num, level, bn.encode(bits, m_bits, k_hash), keys[0], keys[-1])
        reg.put_index(num, index[at_index: at_index + s[2]])
        first_block[slot] = at_block
        at_index += s[2]
        at_block += s[0]
    cap = reg.max_candidates()

    ids = np.concatenate([np.arange(0, 2150), np.arange(5000, 5100), np.arange(6000, 6050), np.arange(9000, 9050)])
    ids = ids[rng.permutation(ids.size)]
    probes = [key(int(i)) for i in ids]
    n = len(probes)
    want = [pref.lsm_get(tables, files, p) for p in probes]
    n_found = sum(st == pref.GET_FOUND for st, _, _ in want)
    assert sum(st == pref.GET_FOUND and src == 0 for st, src, _ in want) >= 50
    assert sum(st == pref.GET_FOUND and src == 1 for st, src, _ in want) >= 500
    assert sum(st == pref.GET_FOUND and not v for st, _, v in want) >= 5 and n - n_found >= 100

    dk = seb.dev_keys(torch.from_numpy(np.frombuffer(b"".join(probes), np.uint8).copy()).cuda(), n=n, stride=16)
    arrays = [gref.run_arrays(t) for t in tables]
    runs, indexes = [], []
    for a in arrays:
        run = seb.dev_run(torch.from_numpy(a[0].copy()).cuda(), tg.u64_dev(torch, a[1]), tg.u64_dev(torch, a[3]),
                          torch.from_numpy(a[4]).cuda(), tg.u64_dev(torch, a[5]))
        ix = torch.zeros(seb.dev_run_index_size(run.n), dtype=torch.uint8, device="cuda")
        seb.dev_run_index(run, ix)
        runs.append(run), indexes.append(ix)
    mem_status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    mem_run = torch.zeros(n, dtype=torch.uint8, device="cuda")
    mem_vloc = torch.zeros(n, dtype=torch.int64, device="cuda")
    mem_vlen = torch.zeros(n, dtype=torch.int32, device="cuda")
    seb.dev_runs_search(dk, runs, indexes, mem_status, run=mem_run, vloc=mem_vloc, vlen=mem_vlen)
    ws = torch.zeros(seb.dev_get_compact_workspace_size(n), dtype=torch.uint8, device="cuda")
    plan = seb.dev_get_compact_plan(dk, mem_status, ws)
    m = plan.undecided
    ck, row = seb.dev_get_compact_emit(dk, mem_status, plan, ws, torch.zeros(16 * m, dtype=torch.uint8, device="cuda"), None,
                                       torch.zeros(m, dtype=torch.int32, device="cuda"))
    B = tg.sst_steps(torch, seb, reg, ck, cap, first_block, dpool, dblen)
    status, source = (torch.full((n,), 0x7E, dtype=torch.uint8, device="cuda") for _ in range(2))
    vloc = torch.zeros(n, dtype=torch.int64, device="cuda")
    vlen = torch.zeros(n, dtype=torch.int32, device="cuda")
    seb.dev_get_join_rows(mem_status, n, row, m, B["status"], status, source, vloc=vloc, vlen=vlen, mem_vloc=mem_vloc,
                          mem_vlen=mem_vlen, sst_vloc=B["vloc"], sst_vlen=B["vlen"])

    # the last step: the values themselves
    run_vals = [torch.from_numpy(a[2].copy() if a[2].size else np.zeros(1, np.uint8)).cuda() for a in arrays]
    run_bytes = [int(a[2].size) for a in arrays]
    vws = torch.zeros(seb.dev_get_values_workspace_size(n), dtype=torch.uint8, device="cuda")
    vplan = seb.dev_get_values_plan(status, source, mem_run, vloc, vlen, n, run_vals, dpool, vws, val_bytes=run_bytes)
    assert vplan.n == n and vplan.found == n_found
    assert vplan.val_bytes == sum(len(v) for st, _, v in want if st == pref.GET_FOUND)
    obuf, out_off = guarded(torch, 8 * (n + 1))
    vbuf, out_vals = guarded(torch, vplan.val_bytes, 1)
    seb.dev_get_values_emit(status, source, mem_run, vloc, vlen, n, run_vals, dpool, vplan, vws, out_off, out_vals,
                            val_bytes=run_bytes)
    torch.cuda.synchronize()
    off = np.frombuffer(read_guarded(obuf, 8 * (n + 1), 0, "out_off").tobytes(), np.uint64)
    got = read_guarded(vbuf, vplan.val_bytes, 1, "out_vals")
    hstatus = status.cpu().numpy()
    for i, (st, _, value) in enumerate(want):
        assert int(hstatus[i]) == st, i
        span = got[int(off[i]): int(off[i + 1])].tobytes()
        assert span == (value if st == pref.GET_FOUND else b""), (i, probes[i])
    reg.close()
