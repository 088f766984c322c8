"""The kernels whose arithmetic around the hash was trimmed (the 3-instruction modular step, phase 0
without the pack/unpack round trip, the bin scatter's out-of-line rare path) against the oracle:
the bin scatter at the bucket counts where it switches bins or hands over to the counting sort, with
its bins and regions overflowing, and over never-cleared words; the phased probes, compacted and
dense, at the moduli where the step's edge cases live (just under the packed width, c = 0, C2's m
and an odd one).  Every expectation comes from oracle/, none from the library."""
import numpy as np
import pytest

from oracle import oracle_c as oc

pytestmark = pytest.mark.gpu

K = 7
N_BUILD = 300_000
N_PROBE = 70_001                     # 1093 groups of 64 and a ragged one of 49
M_C2 = 95_850_584


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


@pytest.fixture(scope="module")
def keys():
    k = np.random.default_rng(20240607).integers(0, 256, (N_BUILD, 16), dtype=np.uint8)
    k.setflags(write=False)
    return k


@pytest.fixture(scope="module")
def keys_dev(torch_cuda, keys):
    return torch_cuda.from_numpy(np.array(keys, copy=True)).cuda()


@pytest.fixture(scope="module")
def probe_keys(keys):
    """Half present (every 8th build key, so they spread over the tiles), half random."""
    half = N_PROBE // 2
    absent = np.random.default_rng(99).integers(0, 256, (N_PROBE - half, 16), dtype=np.uint8)
    p = np.concatenate([keys[: half * 8: 8], absent])
    p = p[np.random.default_rng(5).permutation(N_PROBE)]  # present and absent mixed within each wave
    p.setflags(write=False)
    return p


# ---------------------------------------------------------------- scatter -------------------

@pytest.mark.parametrize("m", [512 * 65536 - 17,     # 512 buckets: the first filter the bin scatter takes
                               1575 * 65536,          # the last with 48-slot bins
                               1575 * 65536 + 1,      # 1576 buckets: 32-slot bins
                               2275 * 65536 - 1,      # the last the bin scatter takes
                               M_C2])
def test_bin_scatter_boundaries(seb, torch_cuda, keys, keys_dev, m):
    torch = torch_cuda
    want = oc.build(m, K, keys, N_BUILD, stride=16)
    words = seb.new_words(m)
    with seb.option("build_algo", 2):
        seb.dev_build(seb.dev_keys(keys_dev, n=N_BUILD, stride=16), words, m, K)
        torch.cuda.synchronize()
    assert np.array_equal(seb.words_to_bits(words, m), want)


def test_bin_scatter_three_distinct_keys(seb, torch_cuda, keys):
    """300,000 copies of 3 keys: 21 positions take 100,000 claims each, so every round overflows
    its bins and every tile its regions (the path that leaves the bin write's straight line)."""
    rep = np.ascontiguousarray(keys[np.arange(N_BUILD) % 3])
    with seb.option("build_algo", 2):
        f = seb.BloomFilter(10_000_000, 0.01)
        try:
            assert (f.num_bits, f.num_hashes) == (M_C2, K)
            f.add_batch(rep)
            enc = f.encode()
        finally:
            f.close()
    want = oc.build(M_C2, K, rep, N_BUILD, stride=16)
    assert int(np.unpackbits(want).sum()) <= 21
    assert enc[12:] == want.tobytes()


def test_bin_scatter_fresh_over_prefilled_words(seb, torch_cuda, keys, keys_dev):
    """A fresh build writes every word of the filter: nothing of the 0xA5 fill survives.  The same
    keys through the handle (whose first build is a fresh one) encode to the oracle's bits."""
    torch = torch_cuda
    want = oc.build(M_C2, K, keys, N_BUILD, stride=16)
    words = seb.new_words(M_C2)
    words.view(torch.uint8).fill_(0xA5)
    with seb.option("build_algo", 2):
        seb.dev_build_fresh(seb.dev_keys(keys_dev, n=N_BUILD, stride=16), words, M_C2, K)
        torch.cuda.synchronize()
        f = seb.BloomFilter(10_000_000, 0.01)
        try:
            f.add_batch(keys)
            enc = f.encode()
        finally:
            f.close()
    assert np.array_equal(seb.words_to_bits(words, M_C2), want)
    assert enc[12:] == want.tobytes()


# ---------------------------------------------------------------- probe ---------------------

PROBE_MS = [(1 << 29) - 3, 1 << 28, M_C2, 12_345_677]


@pytest.fixture(scope="module")
def _filters():
    cache = {}
    yield cache
    cache.clear()


@pytest.fixture
def probe_case(request, seb, torch_cuda, keys, keys_dev, probe_keys, _filters):
    """(m, device words holding the ORACLE's bits, oracle answers), built once per m."""
    m = request.param
    if m not in _filters:
        bits = oc.build(m, K, keys, N_BUILD, stride=16)
        want = oc.probe(bits, m, K, probe_keys, N_PROBE, stride=16)
        assert want.sum() >= N_PROBE // 2 and not want.all()
        words = seb.new_words(m)
        seb.dev_build(seb.dev_keys(keys_dev, n=N_BUILD, stride=16), words, m, K)
        torch_cuda.cuda.synchronize()
        assert np.array_equal(seb.words_to_bits(words, m), bits)  # the probes below read the oracle's filter
        _filters[m] = (words, want)
    return (m,) + _filters[m]


@pytest.fixture(scope="module")
def probe_dev(torch_cuda, probe_keys):
    return torch_cuda.from_numpy(np.array(probe_keys, copy=True)).cuda()


@pytest.mark.parametrize("compact", [1, 0], ids=["compact", "dense"])
@pytest.mark.parametrize("phases", [1, 3, 7])
@pytest.mark.parametrize("probe_case", PROBE_MS, indirect=True)
def test_phased_probe_answers(seb, torch_cuda, probe_dev, probe_case, phases, compact):
    torch = torch_cuda
    m, words, want = probe_case
    out = torch.full((N_PROBE + 7,), 7, dtype=torch.uint8, device="cuda")
    with seb.option("probe_phases", phases), seb.option("probe_compact", compact):
        seb.dev_probe(seb.dev_keys(probe_dev, n=N_PROBE, stride=16), words, m, K, out[:N_PROBE])
        torch.cuda.synchronize()
    got = out.cpu().numpy()
    bad = np.flatnonzero(got[:N_PROBE] != want)
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    assert (got[N_PROBE:] == 7).all()


@pytest.mark.parametrize("probe_case", PROBE_MS, indirect=True)
def test_probe_packed_answers(seb, torch_cuda, probe_dev, probe_case):
    torch = torch_cuda
    m, words, want = probe_case
    packed = torch.zeros(N_PROBE, dtype=torch.int64, device="cuda")
    seb.dev_pack_residues(seb.dev_keys(probe_dev, n=N_PROBE, stride=16), m, K, packed)
    out = torch.full((N_PROBE + 7,), 7, dtype=torch.uint8, device="cuda")
    seb.dev_probe_packed(packed, N_PROBE, words, m, K, out[:N_PROBE])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    bad = np.flatnonzero(got[:N_PROBE] != want)
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    assert (got[N_PROBE:] == 7).all()
