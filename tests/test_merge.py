"""CPU: the host half of the batched compaction merge (include/seb_bloom.h, the compaction merge group;
DESIGN.md 5.12) against the restatements of merge_ref.py.

seb_block_entries is loadBlock's walk; seb_merge_plan / seb_merge_emit give, byte for byte, what the
reference's mergeFiles hands its builders when no key occurs in two runs, and the stated rule (the entry of
the lowest-numbered run survives) otherwise, where the key sequence still equals the reference's.  All
comparisons are exact."""
import struct

import numpy as np
import pytest

import block_ref as br
import merge_ref as mr
import scale_ref as sc


def host_merge(seb, runs_blocks, flags=0, **kw):
    pool, blen, rb = mr.pool_of(runs_blocks, **kw)
    plan = seb.merge_plan(pool, blen, rb, flags)
    out = seb.merge_emit(pool, blen, rb, flags)
    assert out[5] == plan
    got = mr.unpack(*out[:5])
    n_in, n_out, kb, vb, shadowed, dropped = plan
    assert n_out == len(got) and kb == sum(len(k) for k, _, _ in got) and vb == sum(len(v) for _, v, _ in got)
    assert n_in == n_out + shadowed + dropped
    assert int(out[1][0]) == 0 and int(out[3][0]) == 0
    return got, plan


# ------------------------------------------------------------------ the restatements themselves

def test_ref_heap_is_go_heap():
    """merge([[a],[a]]) keeps input 1, as the Go heap does; Pop order is sorted."""
    a = (b"a", b"0", False)
    assert mr.go_merge([[a], [(b"a", b"1", False)]], 1) == [(b"a", b"1", False)]
    hp = mr._Heap()
    for k in [b"d", b"b", b"e", b"a", b"c", b"b"]:
        hp.push((k, b"", False, 0))
    assert [hp.pop()[0] for _ in range(6)] == [b"a", b"b", b"b", b"c", b"d", b"e"]


@pytest.mark.parametrize("seed", range(6))
def test_ref_rule_and_go_agree_on_keys(seed):
    rng = np.random.default_rng(seed)
    runs = mr.random_runs(rng, int(rng.integers(1, 10)), 300, share=0.3)
    ents = [[(k, v, d == 1) for k, v, d in run] for run in runs]
    assert [e[0] for e in mr.go_merge(ents, 1)] == [e[0] for e in mr.rule_merge(ents)]
    assert len({e[0] for e in mr.go_merge(ents, 4)}) == len(mr.go_merge(ents, 4))


# ------------------------------------------------------------------ seb_block_entries

def check_block(seb, img):
    assert seb.block_entries(img).tolist() == mr.load_offsets(img)
    assert len(mr.load_offsets(img)) == len(mr.load_block(img))


def test_block_entries_hand_blocks(seb):
    for name, img, _ in br.hand_blocks():
        check_block(seb, img)


def test_block_entries_random(seb):
    rng = np.random.default_rng(11)
    for _ in range(300):
        check_block(seb, br.random_block(rng)[0])


def test_block_entries_edges(seb):
    abc = [(b"bb", b"v-bb"), (b"dd", b"value-dd", 1), (b"ff", b"")]
    base = br.encode_block(abc)
    for n in range(4):
        assert seb.block_entries(base[:n]).size == 0
    over = br.encode_block(abc, num=7, pad=True)  # walks into the padding: empty-key entries up to the end
    assert len(seb.block_entries(over)) == 7 and mr.load_block(over)[3:] == [(b"", b"", False)] * 4
    check_block(seb, over)
    check_block(seb, br.encode_block(abc, num=4))  # overstated, unpadded: the cut header ends the block
    assert len(seb.block_entries(br.encode_block(abc, num=2))) == 2
    one = len(br.encode_block(abc[:1]))
    assert len(seb.block_entries(base[:one + 8])) == 1  # a header cut at 8 of 9 bytes
    assert len(seb.block_entries(base[:one + 9])) == 1  # the header whole, the payload missing
    assert len(seb.block_entries(base[:-1])) == 2  # b"ff" has an empty value: the cut takes the key's last byte
    assert len(seb.block_entries(br.encode_block(abc[:2])[:-1])) == 1  # a payload cut by one byte
    e454 = struct.pack("<I", 454) + br.encode_entry(b"", b"") * 454
    assert seb.block_entries(e454).tolist() == [4 + 9 * i for i in range(454)]
    e455 = struct.pack("<I", 455) + br.encode_entry(b"", b"") * 454 + b"\x00" * 6
    assert len(e455) == 4096 and len(seb.block_entries(e455)) == 454
    with pytest.raises(seb.SebError) as ei:
        seb.block_entries(e454, cap=453)
    assert ei.value.code == -4 and ei.value.count == 454
    with pytest.raises(seb.SebError) as ei:
        seb.block_entries(b"\x00" * 4097)
    assert ei.value.code == -1


# ------------------------------------------------------------------ the merge

def disjoint_runs(rng, nruns, n):
    keys = sorted({b"%s%05d" % (bytes(rng.integers(97, 123, int(rng.integers(0, 20)), dtype=np.uint8)), i) for i in range(n)})
    runs = [[] for _ in range(nruns)]
    for k in keys:
        r = int(rng.integers(0, nruns))
        runs[r].append((k, b"run%d-" % r + bytes(rng.integers(0, 256, int(rng.integers(0, 60)), dtype=np.uint8)),
                        int(rng.random() < 0.25)))
    return runs


@pytest.mark.parametrize("level", [1, 4])
@pytest.mark.parametrize("nruns", [1, 2, 3, 7])
def test_disjoint_runs_equal_the_reference(seb, level, nruns):
    rng = np.random.default_rng(100 * level + nruns)
    runs = disjoint_runs(rng, nruns, 1500)
    sets = [{k for k, _, _ in run} for run in runs]
    assert all(not (sets[a] & sets[b]) for a in range(nruns) for b in range(a + 1, nruns)), "the runs share a key"
    blocks = [mr.run_blocks(run) for run in runs]
    want = mr.as_bytes(mr.go_merge(mr.decoded(blocks), level))
    got, plan = host_merge(seb, blocks, seb.MERGE_DROP_TOMBSTONES if level == 4 else 0)
    assert got == want
    assert plan[4] == 0 and (plan[5] > 0) == (level == 4)


@pytest.mark.parametrize("level", [1, 4])
@pytest.mark.parametrize("seed", range(4))
def test_shared_keys_follow_the_rule(seb, level, seed):
    rng = np.random.default_rng(seed)
    nruns = (2, 3, 5, 9)[seed]
    runs = mr.random_runs(rng, nruns, 1200, share=0.35)
    blocks = [mr.run_blocks(run) for run in runs]
    ents = mr.decoded(blocks)
    drop = level == 4
    got, plan = host_merge(seb, blocks, seb.MERGE_DROP_TOMBSTONES if drop else 0, full_blen=seed % 2 == 1)
    assert got == mr.as_bytes(mr.rule_merge(ents, drop))
    assert plan[4] > 0
    if not drop:
        assert [k for k, _, _ in got] == [e[0] for e in mr.go_merge(ents, level)]


def test_tombstones_shadow_and_deleted_bytes(seb):
    r0 = [br.encode_block([(b"a", b"0a", 1), (b"b", b"0b", 0), (b"c", b"0c", 2), (b"d", b"0d", 255)])]
    r1 = [br.encode_block([(b"b", b"1b", 1), (b"e", b"1e", 1)])]
    r2 = [br.encode_block([(b"a", b"2a", 0), (b"e", b"2e", 0)])]
    got, plan = host_merge(seb, [r0, r1, r2])
    assert got == [(b"a", b"0a", 1), (b"b", b"0b", 0), (b"c", b"0c", 0), (b"d", b"0d", 0), (b"e", b"1e", 1)]
    assert plan == (8, 5, 5, 10, 3, 0)
    got, plan = host_merge(seb, [r0, r1, r2], seb.MERGE_DROP_TOMBSTONES)
    assert got == [(b"b", b"0b", 0), (b"c", b"0c", 0), (b"d", b"0d", 0)]  # a and e do not resurface
    assert plan == (8, 3, 3, 6, 3, 2)


def test_empty_inputs(seb):
    assert seb.merge_plan(np.zeros(0, np.uint8), np.zeros(0, np.uint16), []) == (0,) * 6
    assert seb.merge_plan(np.zeros(0, np.uint8), np.zeros(0, np.uint16), [0, 0, 0]) == (0,) * 6
    out = seb.merge_emit(np.zeros(0, np.uint8), np.zeros(0, np.uint16), [0, 0])
    assert out[1].tolist() == [0] and out[3].tolist() == [0] and out[4].size == 0
    items = [(b"k%03d" % i, b"v", 0) for i in range(40)]
    empty = [br.encode_block([]), b"", b"\x01\x00"]  # blocks of no entries: a zero count, 0 and 2 bytes
    got, plan = host_merge(seb, [[], empty[:1] + mr.run_blocks(items[:20]) + empty[1:], [], mr.run_blocks(items[20:]), empty])
    assert got == items and plan[0] == 40


def test_unsorted_and_equal_neighbours_are_refused(seb):
    good = mr.run_blocks([(b"k%03d" % i, b"v", 0) for i in range(30)])
    bad = [br.encode_block([(b"a", b"1"), (b"c", b"2"), (b"b", b"3")])]
    dup = [br.encode_block([(b"a", b"1"), (b"b", b"2")]), br.encode_block([(b"b", b"3"), (b"c", b"4")])]
    for runs, where in (([good, bad, dup], "run 1 entry 2"), ([good, good, dup, bad], "run 2 entry 2"),
                        ([bad], "run 0 entry 2")):
        pool, blen, rb = mr.pool_of(runs)
        for call in (seb.merge_plan, seb.merge_emit):
            with pytest.raises(seb.SebError) as ei:
                call(pool, blen, rb)
            assert ei.value.code == -1 and where in str(ei.value), str(ei.value)
    # an overstated count that reaches the padding: empty keys after a key, so the run is not increasing;
    # a run whose only key is the empty key passes
    abc = [(b"bb", b"1"), (b"dd", b"2")]
    pool, blen, rb = mr.pool_of([[br.encode_block(abc, num=5, pad=True)]])
    with pytest.raises(seb.SebError) as ei:
        seb.merge_plan(pool, blen, rb)
    assert ei.value.code == -1 and "run 0 entry 2" in str(ei.value)
    got, _ = host_merge(seb, [[br.encode_block([], num=1, pad=True)]], full_blen=True)
    assert got == [(b"", b"", 0)]


def test_emit_refuses_sizes_that_are_not_the_plans(seb):
    pool, blen, rb = mr.pool_of([mr.run_blocks([(b"k%03d" % i, b"val", 0) for i in range(50)])])
    n_in, n_out, kb, vb, sh, dr = seb.merge_plan(pool, blen, rb)
    for sizes in ((n_in, n_out - 1, kb, vb, sh, dr), (n_in, n_out, kb - 1, vb, sh, dr), (n_in, n_out, kb, vb - 1, sh, dr),
                  (n_in, n_out + 1, kb, vb, sh, dr)):
        with pytest.raises(seb.SebError) as ei:
            seb.merge_emit(pool, blen, rb, 0, sizes=sizes)
        assert ei.value.code == -1


# ------------------------------------------------------------------ the shapes of test_gpu_merge.py's scale tests

T = 1024


def check_arrays(out, want, name):
    arrays, sizes = want
    assert out[5] == sizes, (name, out[5], sizes)
    for j, what in enumerate(("keys", "key_off", "vals", "val_off", "deleted")):
        assert np.array_equal(out[j], arrays[j]), (name, what)


def test_scale_pool_is_the_rule(seb):
    """scale_ref.merge_pool itself at a size the restatement takes: its blocks decode as loadBlock decodes them,
    and its closed form is rule_merge's answer; an empty run among them."""
    for total, nruns, space in ((3000, 7, 2000), (40, 9, 30), (5, 8, 100)):
        pool, blen, rb, want = sc.merge_pool(total, nruns, space)
        runs = [[bytes(pool[b * 4096:b * 4096 + int(blen[b])]) for b in range(rb[r], rb[r + 1])] for r in range(nruns)]
        ents = mr.decoded(runs)
        assert all(len(mr.load_block(img)) == (len(img) - 4) // 21 <= sc.PER_BLOCK for run in runs for img in run)
        for flags in (0, 1):
            arrays, sizes = want[flags]
            assert mr.unpack(*arrays) == mr.as_bytes(mr.rule_merge(ents, bool(flags)))
            assert sizes[0] == sum(len(e) for e in ents) == sizes[1] + sizes[4] + sizes[5]
            check_arrays(seb.merge_emit(pool, blen, rb, flags), want[flags], f"{nruns} runs")


@pytest.mark.parametrize("total,nruns,space", [(140 * T, 17, 400_000), (1024 * T + 40_000, 5, 3_000_000), (12_000, 1025, 100_000)])
def test_scale_pools_equal_the_closed_form(seb, total, nruns, space):
    pool, blen, rb, want = sc.merge_pool(total, nruns, space)
    for flags in (0, seb.MERGE_DROP_TOMBSTONES):
        arrays, sizes = want[flags]
        assert total * 0.9 < sizes[0] <= total and sizes[4] > 0 and (sizes[5] > 0) == bool(flags)
        assert seb.merge_plan(pool, blen, rb, flags) == sizes
        check_arrays(seb.merge_emit(pool, blen, rb, flags), want[flags], f"{nruns} runs, flags {flags}")


@pytest.mark.parametrize("nb,bounds", sc.GROUP_POOLS, ids=[f"{nb}-{b[2]}" for nb, b in sc.GROUP_POOLS])
def test_block_group_pools_follow_the_rule(seb, nb, bounds):
    runs = sc.group_runs(nb, bounds)
    ents = mr.decoded(runs)
    assert sum(len(run) for run in runs) == nb and sum(len(e) for e in ents) == 3 * (nb - sum(b < nb for b in {255, 256, nb - 1}))
    for flags in (0, seb.MERGE_DROP_TOMBSTONES):
        got, plan = host_merge(seb, runs, flags, fill=0xCC)
        assert got == mr.as_bytes(mr.rule_merge(ents, bool(flags))) and plan[4] > 0


@pytest.mark.parametrize("nruns", [16, 17, 33, 257, 1025])
def test_many_runs_follow_the_rule(seb, nruns):
    blocks = [mr.run_blocks(run) for run in sc.many_runs(nruns)]
    ents = mr.decoded(blocks)
    assert sum(not run for run in blocks) >= nruns // 10
    for flags in (0, seb.MERGE_DROP_TOMBSTONES):
        got, plan = host_merge(seb, blocks, flags)
        assert got == mr.as_bytes(mr.rule_merge(ents, bool(flags))) and plan[4] > 0


def test_emit_refuses_sizes_that_are_not_the_plans(seb):
    pool, blen, rb = mr.pool_of([mr.run_blocks([(b"k%03d" % i, b"val", 0) for i in range(50)])])
    n_in, n_out, kb, vb, sh, dr = seb.merge_plan(pool, blen, rb)
    for sizes in ((n_in, n_out - 1, kb, vb, sh, dr), (n_in, n_out, kb - 1, vb, sh, dr), (n_in, n_out, kb, vb - 1, sh, dr),
                  (n_in, n_out + 1, kb, vb, sh, dr)):
        with pytest.raises(seb.SebError) as ei:
            seb.merge_emit(pool, blen, rb, 0, sizes=sizes)
        assert ei.value.code == -1
