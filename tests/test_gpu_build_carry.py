"""The bin scatter's carried partial chunks and apply's flat walk over the written chunks
(csrc/seb_bucket.hip): whole filters, padding bytes included, byte for byte against the oracle
under build_algo 2, each batch both as a fresh build over words full of 0xA5 and OR-ed onto a
half-built filter.

A carry needs a tile with at least two rounds, so more than 256 x round_keys keys: 3 rounds per
tile at 513 buckets (round_keys 1829) with 1,000,003 keys, 4 at 1463 buckets (5120) and at 2274
buckets (32-slot bins) with 4,000,003."""
import functools

import numpy as np
import pytest

from oracle import oracle_c as oc
import keygen as kg

pytestmark = pytest.mark.gpu

K = 7
M513, M1463, M2274 = 33_580_000, 95_850_584, 149_000_000


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def to_dev(torch, arr):
    return torch.from_numpy(np.array(arr, copy=True)).cuda()


@functools.lru_cache(maxsize=None)
def indices(name, n):
    rng = np.random.default_rng(23)
    if name == "ordinary":
        return rng.permutation(3 * n)[:n]
    if name == "identical":
        return np.full(n, 42, np.int64)
    if name == "distinct50":
        return rng.integers(0, 50, n)
    if name == "uneven":  # first half 3 distinct keys repeated, second half ordinary keys
        return np.concatenate([rng.integers(0, 3, n // 2), 1000 + rng.permutation(3 * n)[: n - n // 2]])
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def batch(name, n):
    """The batch's keys; computed once and shared, never modified."""
    keys = kg.key16(indices(name, n))
    keys.setflags(write=False)
    return keys


@functools.lru_cache(maxsize=None)
def reference(name, n, m):
    """The oracle's filter of the batch (of its distinct keys: OR is idempotent)."""
    uniq = np.unique(indices(name, n))
    ref = oc.build(m, K, kg.key16(uniq), len(uniq), stride=16)
    ref.setflags(write=False)
    return ref


def whole(words, m):
    """The filter's bytes and its padding bytes."""
    raw = words.cpu().numpy().view(np.uint8)
    return raw[: (m + 7) // 8], raw[(m + 7) // 8:]


def check_fresh(seb, torch, kd, words, m, ref, what):
    words.view(torch.uint8).fill_(0xA5)
    seb.dev_build_fresh(kd, words, m, K)
    torch.cuda.synchronize()
    bits, pad = whole(words, m)
    assert np.array_equal(bits, ref), what
    assert not pad.any(), what


def check_fresh_and_ored(seb, torch, keys, m, ref, what):
    n = len(keys)
    kd = seb.dev_keys(to_dev(torch, keys), n=n, stride=16)
    words = seb.new_words(m)
    check_fresh(seb, torch, kd, words, m, ref, (what, "fresh"))
    w2 = seb.new_words(m)
    seb.dev_build(seb.dev_keys(to_dev(torch, keys[: n // 2]), n=n // 2, stride=16), w2, m, K)
    seb.dev_build(kd, w2, m, K)
    torch.cuda.synchronize()
    bits, pad = whole(w2, m)
    assert np.array_equal(bits, ref), (what, "ored")
    assert not pad.any(), (what, "ored")
    return words


@pytest.mark.parametrize("bins", [1, 0], ids=["bins", "counting"])
@pytest.mark.parametrize("m,n", [(M513, 1_000_003), (M1463, 4_000_003), (M2274, 4_000_003)],
                         ids=["nb513_3rounds", "nb1463_4rounds", "nb2274_4rounds"])
def test_carry_across_rounds(seb, torch_cuda, m, n, bins):
    """3 rounds per tile with a ragged last round and a short last tile (513 buckets), 4 rounds per
    tile at 48-slot (1463 buckets) and 32-slot bins (2274); the counting sort through the same
    apply in its unpadded form."""
    with seb.option("build_algo", 2), seb.option("scatter_bins", bins):
        check_fresh_and_ored(seb, torch_cuda, batch("ordinary", n), m, reference("ordinary", n, m), (m, n, bins))


def test_single_round_tile(seb, torch_cuda):
    """300,000 keys at 1463 buckets: every tile has exactly one round, the padded write-out."""
    n, m = 300_000, M1463
    with seb.option("build_algo", 2):
        check_fresh_and_ored(seb, torch_cuda, batch("ordinary", n), m, reference("ordinary", n, m), "single")


@pytest.mark.parametrize("name", ["identical", "distinct50"])
def test_overflow_while_carrying(seb, torch_cuda, name):
    """Runs that pass their bins and then their regions while remainders are carried; then a fresh
    build of ordinary keys on the same stream: the overflow bitmap went back to zero."""
    torch = torch_cuda
    n, m = 1_500_000, M513
    with seb.option("build_algo", 2):
        words = check_fresh_and_ored(seb, torch, batch(name, n), m, reference(name, n, m), name)
        n2 = 1_000_003
        kd = seb.dev_keys(to_dev(torch, batch("ordinary", n2)), n=n2, stride=16)
        check_fresh(seb, torch, kd, words, m, reference("ordinary", n2, m), (name, "ordinary after"))


def test_uneven_and_empty_regions(seb, torch_cuda):
    """The flat walk over regions of very unequal length: the tiles of the batch's first half fill a
    few buckets to the cap and leave every other region empty."""
    n, m = 1_000_003, M513
    with seb.option("build_algo", 2):
        check_fresh_and_ored(seb, torch_cuda, batch("uneven", n), m, reference("uneven", n, m), "uneven")


def test_packed_source(seb, torch_cuda):
    """A variable-length batch pre-hashed to packed residues goes through the same scatter (1.2M
    keys >= varlen_prehash_min_keys, k = 7, m < 2^29), 3 rounds per tile at 513 buckets."""
    torch = torch_cuda
    n, m = 1_200_000, M513
    idx = np.random.default_rng(29).permutation(4 * n)[:n]
    data, off = kg.varlen_keys(idx)
    ref = oc.build(m, K, data, n, offsets=off)
    hd, ho = kg.varlen_keys(idx[: n // 2])
    with seb.option("build_algo", 2):
        kd = seb.dev_keys(to_dev(torch, data), to_dev(torch, off.astype(np.int64)))
        words = seb.new_words(m)
        check_fresh(seb, torch, kd, words, m, ref, "varlen fresh")
        w2 = seb.new_words(m)
        seb.dev_build(seb.dev_keys(to_dev(torch, hd), to_dev(torch, ho.astype(np.int64))), w2, m, K)
        seb.dev_build(kd, w2, m, K)
        torch.cuda.synchronize()
        bits, pad = whole(w2, m)
        assert np.array_equal(bits, ref)
        assert not pad.any()
