"""The block-id rules restated in plain Python, independent of the library: a located cell
(slot, block offset) into an id of the block pool.  test_blockids.py holds the host half to it, test_gpu_blockids.py
the device forms, test_blockids_sanitize.py the stand-alone program."""
import numpy as np

NO_BLOCK = 2**64 - 1
NO_ID = 2**32 - 1
PAD = 0xFFFF
NAMES = ("bid", "uniq_slot", "uniq_block")


def classify(slot, off, res_first=None, res_count=None):
    """("none" | "bad" | "resident" | "miss", id or None) for one cell, rules 1-3 in their order."""
    slot, off = int(slot), int(off)
    if slot == PAD or off == NO_BLOCK:
        return "none", None
    if off >= 2**48:
        return "bad", None
    if res_first is not None and slot < len(res_first) and int(res_first[slot]) != NO_ID:
        q, rem = divmod(off, 4096)
        if rem == 0 and q < int(res_count[slot]) and int(res_first[slot]) + q < NO_ID:
            return "resident", int(res_first[slot]) + q
        return "bad", None
    return "miss", None


def block_ids(cand, blocks, res_first=None, res_count=None, id_base=0):
    """(sizes, bid, uniq_slot, uniq_block); sizes = (cells, resident, misses, uniq, bad).  bid has cand's shape."""
    cand, blocks = np.asarray(cand, np.uint16), np.asarray(blocks, np.uint64)
    assert cand.shape == blocks.shape
    fc, fb = cand.reshape(-1), blocks.reshape(-1)
    bid = np.full(fc.size, NO_ID, np.uint32)
    rank, us, ub = {}, [], []
    resident = misses = bad = 0
    for c in range(fc.size):
        kind, rid = classify(fc[c], fb[c], res_first, res_count)
        if kind == "bad":
            bad += 1
        elif kind == "resident":
            resident += 1
            bid[c] = rid
        elif kind == "miss":
            misses += 1
            pair = (int(fc[c]), int(fb[c]))
            if pair not in rank:
                rank[pair] = len(us)
                us.append(pair[0])
                ub.append(pair[1])
            bid[c] = id_base + rank[pair]
    assert id_base + len(us) <= NO_ID
    return ((fc.size, resident, misses, len(us), bad), bid.reshape(cand.shape), np.array(us, np.uint16),
            np.array(ub, np.uint64))


def resident_only(cand, blocks, res_first=None, res_count=None):
    """What seb_dev_block_ids_resident writes: (bid with NO_ID for the miss cells, (resident, misses, bad))."""
    cand, blocks = np.asarray(cand, np.uint16).reshape(-1), np.asarray(blocks, np.uint64).reshape(-1)
    bid = np.full(cand.size, NO_ID, np.uint32)
    n = {"none": 0, "bad": 0, "resident": 0, "miss": 0}
    for c in range(cand.size):
        kind, rid = classify(cand[c], blocks[c], res_first, res_count)
        n[kind] += 1
        if kind == "resident":
            bid[c] = rid
    return bid, (n["resident"], n["miss"], n["bad"])


def assert_same(got, want, what=""):
    for g, w, name in zip(got, want, NAMES):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what} {name}: shape {g.shape}, not {w.shape}"
        if not np.array_equal(g, w):
            at = int(np.nonzero(g.reshape(-1) != w.reshape(-1))[0][0])
            raise AssertionError(f"{what} {name}: differs first at {at}: {g.reshape(-1)[at]} != {w.reshape(-1)[at]}")


# ------------------------------------------------------------------ the cases the CPU and the GPU tests share

def table_mixed():
    """A residency table over 6 slots: 0 and 3 resident, 3's ids close to 2^32 so that the sum overflows; slots 6 and
    up lie past res_slots."""
    first = np.array([100, NO_ID, NO_ID, NO_ID - 3, NO_ID, 7], np.uint32)
    count = np.array([10, 0, 5, 8, 0, 0], np.uint32)  # slot 5: resident with no block; slot 2: a count without a first
    return first, count


def pattern(name, cells, seed=0):
    """(cand, blocks) of `cells` cells for one named pattern."""
    rng = np.random.default_rng(seed + cells)
    c = np.arange(cells, dtype=np.uint64)
    if name == "distinct":       # every pair once: the table at its fullest, chains that wrap its end
        return (c % 7).astype(np.uint16), (c // 7) * 4096
    if name == "one_pair":       # the greatest contention
        return np.full(cells, 3, np.uint16), np.full(cells, 8192, np.uint64)
    if name == "7x3":
        return rng.integers(0, 7, cells).astype(np.uint16), rng.integers(0, 3, cells).astype(np.uint64) * 4096
    if name == "cross":          # the same offset in two slots, two offsets in one slot
        return (c % 2).astype(np.uint16) + 1, np.where(c % 3 == 0, 4096, np.where(c % 2 == 1, 8192, 4096)).astype(np.uint64)
    if name == "high_bits":      # offsets that differ only in bit 32 or only in bit 40
        k = rng.integers(0, 4, cells)
        return np.full(cells, 2, np.uint16), (4096 + (k & 1) * 2**32 + (k >> 1) * 2**40).astype(np.uint64)
    if name == "unaligned":      # not multiples of 4096, in files that are not resident
        return rng.integers(0, 5, cells).astype(np.uint16), rng.integers(1, 40, cells).astype(np.uint64) * 1001
    if name == "ends":           # a pair whose only two cells are the first and the last of the batch
        cand, blocks = (c % 5).astype(np.uint16), (c % 11) * 4096
        cand[0] = cand[-1] = 9
        blocks[0] = blocks[-1] = 12345
        return cand, blocks
    if name == "padding":        # 0xFFFF with a real offset, a real slot with NO_BLOCK
        cand, blocks = rng.integers(0, 4, cells).astype(np.uint16), rng.integers(0, 6, cells).astype(np.uint64) * 4096
        cand[c % 3 == 0] = PAD
        blocks[c % 4 == 1] = NO_BLOCK
        return cand, blocks
    if name == "mixed":          # for table_mixed(): every rule
        cand = rng.integers(0, 9, cells).astype(np.uint16)  # slots 6..8 lie past the table
        blocks = rng.integers(0, 12, cells).astype(np.uint64) * 4096  # past slot 0's 10 and slot 3's 8 blocks
        k = rng.integers(0, 16, cells)
        blocks[k == 0] += 17                       # unaligned
        blocks[k == 1] = 2**48 + 4096              # refused by rule 2
        blocks[k == 2] = 2**63
        blocks[k == 3] = NO_BLOCK
        cand[k == 4] = PAD
        return cand, blocks
    raise KeyError(name)


PATTERNS = ("distinct", "one_pair", "7x3", "cross", "high_bits", "unaligned", "ends", "padding", "mixed")
