"""A pure-Python restatement of the Get path's last step (include/seb_bloom.h, "Get values"): the
values of the found keys of a batch, back to back in batch order, with an offset array.  It is what
seb_get_values is held to, and seb_get_values is what the device form is held to.

A batch is five arrays of n elements (status, source, run, vloc, vlen; run may be None and is then read as 0), the
runs' value bytes `vals` (a list of bytes-like objects; None for a null pointer, whose size val_bytes[r] then gives)
and the block pool (bytes-like or None)."""
import numpy as np

GET_FOUND = 1
MAX_RUNS = 8


def _sizes(vals, val_bytes):
    return list(val_bytes) if val_bytes is not None else [0 if v is None else len(v) for v in vals]


def lowest_invalid(status, source, run, vloc, vlen, vals=(), pool=None, val_bytes=None):
    """The lowest key that carries a value (status == GET_FOUND exactly) which does not lie inside the source it
    names, or None.  Arithmetic is on Python integers, so nothing wraps."""
    vb = _sizes(vals, val_bytes)
    pool_bytes = 0 if pool is None else len(pool)
    for i in range(len(status)):
        if int(status[i]) != GET_FOUND:
            continue
        s = int(source[i])
        if s == 0:
            r = 0 if run is None else int(run[i])
            if r >= len(vals) or (vals[r] is None and vb[r] != 0):
                return i
            size = vb[r]
        elif s == 1:
            size = pool_bytes
        else:
            return i
        if int(vloc[i]) + int(vlen[i]) > size:
            return i
    return None


def values(status, source, run, vloc, vlen, vals=(), pool=None, val_bytes=None):
    """((n, found, val_bytes), out_off u64 n + 1, out_vals u8) of a batch without an invalid carrying key."""
    assert lowest_invalid(status, source, run, vloc, vlen, vals, pool, val_bytes) is None
    n = len(status)
    out_off = np.zeros(n + 1, np.uint64)
    parts, found, at = [], 0, 0
    for i in range(n):
        if int(status[i]) == GET_FOUND:
            found += 1
            a, ln = int(vloc[i]), int(vlen[i])
            if ln:
                src = pool if int(source[i]) == 1 else vals[0 if run is None else int(run[i])]
                parts.append(bytes(memoryview(src)[a:a + ln]))
                assert len(parts[-1]) == ln
                at += ln
        out_off[i + 1] = at
    return (n, found, at), out_off, np.frombuffer(b"".join(parts), np.uint8)


def assert_same(got, want, what=""):
    (gs, go, gv), (ws, wo, wv) = got, want
    assert tuple(int(x) for x in gs) == tuple(ws), (what, gs, ws)
    assert np.array_equal(np.asarray(go, np.uint64), wo), f"{what}: out_off differs"
    assert np.array_equal(np.asarray(gv, np.uint8), wv), f"{what}: out_vals differs"


# ---------------------------------------------------------------- batches the CPU and the GPU tests share

LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 4083)


def make_batch(rng, n, num_runs=2, pool_bytes=3 * 4096, run_bytes=6000, found=None, lengths=LENGTHS, pool_only=False,
               runs_only=False, garbage=True):
    """A valid batch of n keys over num_runs runs and a pool of random bytes.  found: a bool mask (default: random
    halves).  The keys that carry nothing hold the status bytes 0, 2, 3 and 255 and, with `garbage`, arbitrary
    source / run / vloc / vlen.  Returns a dict of the arrays, vals (list of u8 arrays) and pool (u8 array)."""
    vals = [rng.integers(0, 256, run_bytes + 17 * r, dtype=np.uint8) for r in range(num_runs)]
    pool = rng.integers(0, 256, pool_bytes, dtype=np.uint8)
    if found is None:
        found = rng.random(n) < 0.5
    found = np.asarray(found, bool)
    status = np.where(found, GET_FOUND, rng.choice(np.array([0, 2, 3, 255], np.uint8), n)).astype(np.uint8)
    source = np.zeros(n, np.uint8)
    run = np.zeros(n, np.uint8)
    vloc = np.zeros(n, np.uint64)
    vlen = np.zeros(n, np.uint32)
    for i in range(n):
        if not found[i]:
            if garbage:
                source[i] = rng.integers(0, 256)
                run[i] = rng.integers(0, 256)
                vloc[i] = rng.integers(0, 2**64, dtype=np.uint64)
                vlen[i] = rng.integers(0, 2**32, dtype=np.uint32)
            continue
        if num_runs == 0 or pool_only:
            in_pool = True
        else:
            in_pool = not runs_only and rng.random() < 0.5
        if in_pool:
            source[i] = 1
            run[i] = rng.integers(0, 256)  # never looked at for a pool value
            size = pool_bytes
        else:
            run[i] = rng.integers(0, num_runs)
            size = len(vals[run[i]])
        ln = min(int(rng.choice(lengths)), size)
        vlen[i] = ln
        vloc[i] = rng.integers(0, size - ln + 1)
    return dict(status=status, source=source, run=run, vloc=vloc, vlen=vlen, vals=vals, pool=pool)


def batch_args(b):
    return (b["status"], b["source"], b["run"], b["vloc"], b["vlen"], b["vals"], b["pool"])
