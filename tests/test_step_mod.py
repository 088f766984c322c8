"""The 3-instruction modular step of the position recurrence (seb_device.h step_mod):

    step_mod(x, na, m) = min(x - na, x - na + m)   in u32 arithmetic, na = m - a

equals (x + a) mod m for m < 2^31, x < m, 1 <= na <= m.  Checked here with numpy's wrapping
uint32 arithmetic: every (x, na) for small m, and 10^6 random triples (edges included) for the large
moduli the kernels meet (just under the packed-residue width, 2^29, and the M32 limit)."""
import numpy as np
import pytest


def step_mod(x, na, m):
    x = np.asarray(x, np.uint32)
    na = np.asarray(na, np.uint32)
    t = x - na                      # wraps mod 2^32
    u = t + np.uint32(m)            # wraps mod 2^32
    return np.minimum(t, u)


def want(x, na, m):
    a = np.uint64(m) - np.asarray(na, np.uint64)   # the addend, in [0, m - 1]
    return ((np.asarray(x, np.uint64) + a) % np.uint64(m)).astype(np.uint32)


@pytest.mark.parametrize("m", [1, 2, 3, 64, 255, 257])
def test_step_mod_exhaustive_small(m):
    x, na = np.meshgrid(np.arange(m, dtype=np.uint32), np.arange(1, m + 1, dtype=np.uint32), indexing="ij")
    with np.errstate(over="ignore"):
        got = step_mod(x, na, m)
    assert np.array_equal(got, want(x, na, m))
    assert (got < m).all()


@pytest.mark.parametrize("m", [(1 << 29) - 3, 1 << 29, (1 << 31) - 1])
def test_step_mod_random_large(m):
    rng = np.random.default_rng(m & 0xffff)
    n = 1_000_000
    x = rng.integers(0, m, n, dtype=np.uint64).astype(np.uint32)
    na = rng.integers(1, m + 1, n, dtype=np.uint64).astype(np.uint32)
    # the edges: na = m (addend 0), na = 1, x = 0, x = m - 1, in every combination
    ex = np.array([0, 0, m - 1, m - 1, 0, m - 1, 1, m - 2], np.uint32)
    ena = np.array([m, 1, m, 1, m - 1, 2, m, m], np.uint32)
    x[: ex.size] = ex
    na[: ena.size] = ena
    x[ex.size: ex.size + 1000] = 0
    x[ex.size + 1000: ex.size + 2000] = m - 1
    na[ex.size + 2000: ex.size + 3000] = m
    with np.errstate(over="ignore"):
        got = step_mod(x, na, m)
    assert np.array_equal(got, want(x, na, m))
    assert (got < m).all()


def test_wrapped_addend_is_a_max():
    """step_addends: -nd = max(b - c, b - c - m) in u32 arithmetic equals ((b - c) mod m) - m, so
    nd = m - ((b - c) mod m), for b, c < m < 2^31 (c = 2^64 mod m; c = 0 for a power of two)."""
    for m in (1, 2, 3, 64, 255, 257):
        b, c = np.meshgrid(np.arange(m, dtype=np.uint32), np.arange(m, dtype=np.uint32), indexing="ij")
        with np.errstate(over="ignore"):
            t = b - c
            nd = np.uint32(0) - np.maximum(t, t - np.uint32(m))
        bc = (b.astype(np.int64) - c.astype(np.int64)) % m
        assert np.array_equal(nd.astype(np.int64), m - bc)
    rng = np.random.default_rng(7)
    for m in ((1 << 29) - 3, 1 << 28, 95_850_584, (1 << 31) - 1):
        b = rng.integers(0, m, 1_000_000, dtype=np.uint64).astype(np.uint32)
        c = np.uint32((1 << 64) % m)
        b[:4] = [0, m - 1, c, max(int(c), 1) - 1]
        with np.errstate(over="ignore"):
            t = b - c
            nd = np.uint32(0) - np.maximum(t, t - np.uint32(m))
        bc = (b.astype(np.int64) - int(c)) % m
        assert np.array_equal(nd.astype(np.int64), m - bc)
