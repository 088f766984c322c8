"""A Python restatement of the reference's range scan (btree/iterator.go), written fresh for the tests of the
B-tree's range scans, beside the library's own design restated: the leaf directory with every
refusal, and the scan by directory.  The pages, the cases and the walk are btree_ref's.

literal_scan is Iterator LITERALLY: seek (the empty-start descent by CellAt(0).Child included, which skips the subtree
under RightPtr), Next, the chain followed along RightPtr, with a step cap so that a test cannot spin.  It returns
(entries, end): end is "done", "error" (CellAt failed: the first cell of an empty leaf with an end key), "nil-key"
(an empty leaf with a nil end hands out a nil key) or "cap".

build_dir / scan_by_dir state what include/seb_bloom.h ("B-tree, range scans") states."""
import struct

import numpy as np

import btree_ref as bref

DIR_MAGIC, DIR_HEADER = 0x42544452, 32
STEP_CAP = 200_000


# ---------------------------------------------------------------- the literal iterator

def literal_seek(image, meta, start):
    """(page id, cell index) or None (an internal page without cells on the empty-start descent)."""
    pid = meta["root"]
    pg = bref.page_of(image, pid)
    if len(start) == 0:
        for _ in range(bref.MAX_DEPTH + 2):
            if pg.is_leaf:
                return pid, 0
            if pg.num_cells == 0:
                return None
            pid = pg.cell_at(0, leaf=False).child  # NOT the right pointer: the leftmost subtree is skipped
            pg = bref.page_of(image, pid)
        raise AssertionError("the literal seek does not end")
    for _ in range(bref.MAX_DEPTH + 2):
        pg = bref.page_of(image, pid)
        if pg.is_leaf:
            i = pg.search_cell(start)
            return pid, (-i - 1 if i < 0 else i)
        pid = bref.find_child_linear(pg, start)
    raise AssertionError("the literal seek does not end")


def literal_scan(image, meta, start, end, limit=0):
    """end None: the reference's nil endKey."""
    at = literal_seek(image, meta, start)
    out = []
    if at is None:
        return out, "done"
    pid, idx = at
    first = True
    for _ in range(STEP_CAP):
        if limit and len(out) == limit:
            return out, "done"
        pg = bref.page_of(image, pid)
        if not first:
            idx += 1
        first = False
        if idx >= pg.num_cells:
            if pg.right_ptr == 0:
                return out, "done"
            pid, idx = pg.right_ptr, 0
            pg = bref.page_of(image, pid)
        c = pg.cell_at(idx)
        if end is not None:
            if c is None:
                return out, "error"
            if c.key >= end:
                return out, "done"
        if c is None:
            return out, "nil-key"
        out.append((c.key, c.value))
    return out, "cap"


# ---------------------------------------------------------------- the directory

class Refused(Exception):
    def __init__(self, rule, page):
        super().__init__(f"page {page}: {rule}")
        self.rule, self.page = rule, page


def dir_offsets(num_pages):
    first_at = (DIR_HEADER + 4 * num_pages + 7) & ~7
    ord_at = first_at + 8 * num_pages + 8
    return first_at, ord_at, (ord_at + 4 * num_pages + 15) & ~15


def build_dir(image, meta, kind, level):
    """(bytes of the directory, dict(leaves, keys, depth)); Refused(rule, page) by the rules of seb_bt_dir_build, in
    their order."""
    n, root = meta["num_pages"], meta["root"]
    ok = lambda p: 1 <= p < n  # noqa: E731
    if not ok(root):
        raise Refused("root", root)
    lst, depth = [root], 0
    for r in range(bref.MAX_DEPTH):
        kind0 = kind[lst[0]] if ok(lst[0]) else bref.BAD
        for p in lst:
            if not ok(p) or kind[p] == bref.BAD:
                raise Refused("bad", p)
            if level[p] != r:
                raise Refused("level", p)
            if kind[p] != kind0:
                raise Refused("mixed", p)
        depth = r + 1
        if kind0 == bref.LEAF:
            break
        if r + 1 == bref.MAX_DEPTH:
            raise Refused("deep", lst[0])
        if sum(bref.page_of(image, p).num_cells + 1 for p in lst) > n:
            raise Refused("wide", lst[0])
        nxt = []
        for p in lst:
            pg = bref.page_of(image, p)
            nxt.append(pg.right_ptr)  # the LEFTMOST child
            nxt += [c.child for c in pg.cells()]
        lst = nxt
    L = len(lst)
    twice = sorted({p for p in lst if lst.count(p) > 1}) if len(set(lst)) != L else []
    if twice:
        raise Refused("twice", twice[0])
    cells = [bref.page_of(image, p).num_cells for p in lst]
    first = np.zeros(L + 1, np.uint64)
    np.cumsum(cells, out=first[1:])
    for i, p in enumerate(lst):
        if bref.page_of(image, p).right_ptr != (lst[i + 1] if i + 1 < L else 0):
            raise Refused("chain", p)
    for i, p in enumerate(lst):
        if not cells[i]:
            continue
        j = next((j for j in range(i + 1, L) if cells[j]), None)
        if j is None:
            continue
        a, b = bref.page_of(image, p).cell_at(cells[i] - 1), bref.page_of(image, lst[j]).cell_at(0)
        if a is None or b is None or not a.key < b.key:
            raise Refused("order", p)
    first_at, ord_at, total = dir_offsets(n)
    d = np.zeros(total, np.uint8)
    d[:DIR_HEADER] = np.frombuffer(struct.pack("<IIIIQII", DIR_MAGIC, n, root, L, int(first[L]), depth, 0), np.uint8)
    d[DIR_HEADER: DIR_HEADER + 4 * L] = np.array(lst, np.uint32).view(np.uint8)
    d[first_at: first_at + 8 * (L + 1)] = first.view(np.uint8)
    ordv = np.full(n, bref.NO_PAGE, np.uint32)
    ordv[lst] = np.arange(L, dtype=np.uint32)
    d[ord_at: ord_at + 4 * n] = ordv.view(np.uint8)
    return d, dict(leaves=L, keys=int(first[L]), depth=depth)


def dir_arrays(d, num_pages):
    first_at, ord_at, _ = dir_offsets(num_pages)
    L = int(d[12:16].view(np.uint32)[0])
    return (d[DIR_HEADER: DIR_HEADER + 4 * L].view(np.uint32), d[first_at: first_at + 8 * (L + 1)].view(np.uint64),
            d[ord_at: ord_at + 4 * num_pages].view(np.uint32))


def scan_by_dir(image, meta, d, starts, ends, limit=0):
    """dict of the arrays seb_bt_scan returns, over lists of start and end keys (b"": from the first key / unbounded)."""
    n = meta["num_pages"]
    leaf, first, ordv = dir_arrays(d, n)
    L, keys = len(leaf), int(first[-1])

    def position(key, empty):
        if len(key) == 0:
            return empty
        st, lf, pos, _, _ = bref.get(image, meta, key)
        if st == bref.ERROR or lf >= n or ordv[lf] >= L or pos > int(first[ordv[lf] + 1] - first[ordv[lf]]):
            return None
        return int(first[ordv[lf]]) + pos

    rs, ro, rows, kk, vv = [], [0], [], [], []
    for s, e in zip(starts, ends):
        a, b = position(s, 0), position(e, keys)
        bad = a is None or b is None
        cnt = 0 if bad else max(0, b - a)
        cnt = min(cnt, limit) if limit else cnt
        rs.append(bref.ERROR if bad else 0)
        for g in range(a or 0, (a or 0) + cnt):
            o = int(np.searchsorted(first, g, side="right")) - 1
            c = bref.page_of(image, int(leaf[o])).cell_at(g - int(first[o]))
            rows.append((bref.FOUND, 1, int(leaf[o]) * bref.PAGE + c.koff, len(c.key), int(leaf[o]) * bref.PAGE + c.voff, len(c.value)))
            kk.append(c.key), vv.append(c.value)
        ro.append(len(rows))
    cols = list(zip(*rows)) if rows else [[]] * 6
    names = ("status", "source", "kloc", "klen", "vloc", "vlen")
    types = (np.uint8, np.uint8, np.uint64, np.uint32, np.uint64, np.uint32)
    out = {k: np.array(c, t) for k, c, t in zip(names, cols, types)}
    out.update(range_status=np.array(rs, np.uint8), range_off=np.array(ro, np.uint64),
               key_off=np.cumsum([0] + [len(k) for k in kk]).astype(np.uint64), keys=np.frombuffer(b"".join(kk), np.uint8),
               val_off=np.cumsum([0] + [len(v) for v in vv]).astype(np.uint64), vals=np.frombuffer(b"".join(vv), np.uint8),
               pairs=list(zip(kk, vv)))
    return out


ARRAYS = ("range_status", "range_off", "status", "source", "kloc", "klen", "vloc", "vlen", "key_off", "keys", "val_off", "vals")


def pairs_of(got, r):
    """Range r's (key, value) list out of a scan's arrays."""
    ko, vo, kb, vb = got["key_off"], got["val_off"], got["keys"], got["vals"]
    return [(bytes(kb[int(ko[e]): int(ko[e + 1])]), bytes(vb[int(vo[e]): int(vo[e + 1])]))
            for e in range(int(got["range_off"][r]), int(got["range_off"][r + 1]))]


# ---------------------------------------------------------------- the ranges of a case

def leaf_boundaries(image, meta, d):
    """(last key of a non-empty leaf, first key of the next listed non-empty leaf) pairs."""
    leaf, first, _ = dir_arrays(d, meta["num_pages"])
    full = [int(p) for i, p in enumerate(leaf) if first[i + 1] > first[i]]
    out = []
    for a, b in zip(full, full[1:]):
        pa, pb = bref.page_of(image, a), bref.page_of(image, b)
        out.append((pa.cell_at(pa.num_cells - 1).key, pb.cell_at(0).key))
    return out


def ranges(case, rng, d=None, cap=24):
    """(starts, ends): for a sample of stored keys k and k's successor, bounds at k, k + b"\\0" and k[:-1]; below the
    minimum and above the maximum; start == end, start > end; empty start, empty end, both; bounds between the last key
    of a leaf and the first of the next (pos == numCells); the separators; long keys."""
    keys = case.keys
    out = [(b"", b""), (b"\0", b""), (b"", b"\xff" * 40), (b"\xff" * 40, b""), (b"\xff" * 40, b"\0")]
    if not keys:
        return [s for s, _ in out], [e for _, e in out]
    idx = sorted(set(rng.choice(len(keys), min(cap, len(keys)), replace=False).tolist()) | {0, len(keys) - 1})
    var = lambda k: [k, k + b"\0", k[:-1]]  # noqa: E731
    small = len(keys) <= 400  # on a large case only ranges near an end of the key space are unbounded
    for i in idx:
        k, nx = keys[i], keys[min(i + 1, len(keys) - 1)]
        far = keys[min(i + 1 + int(rng.integers(0, 40)), len(keys) - 1)]
        for s in var(k):
            out += [(s, e) for e in var(nx) if e] + [(s, far)] + ([(s, b"")] if small or i >= len(keys) - 300 else [])
        if small or i < 300:
            out += [(b"", e) for e in var(k) if e]
        out += [(k, k), (nx, k), (k + b"\0", k)]
    out += [(keys[0][:-1] or b"\0", keys[0]), (b"\0", keys[-1] + b"\xff"), (keys[-1], keys[-1] + b"\0"), (keys[-1] + b"\0", b"")]
    seps = case.seps[:60]
    out += [(s, b"") for s in seps[: 20 if small else 0]] + [(b"", s) for s in seps[: 20 if small else 0]]
    out += [(a, b) for a, b in zip(case.seps, case.seps[1:])][: 60 if small else 400: 1 if small else 7]
    out += [(s, s + b"\0") for s in case.seps]  # every separator as a bound
    out += [(s[:-1] or b"\0", s + b"\0") for s in seps[:10]]
    if d is not None:
        for last, nxt in leaf_boundaries(case.image, case.meta, d)[:30]:
            between = last + b"\0"
            out += [(between, nxt + b"\0"), (last, between), (between, nxt)] + ([(between, b""), (b"", between)] if small else [])
    if len(keys) > 4:
        lk = bref.long_keys(case)
        out += [(lk[0], lk[0] + b"\1"), (keys[-2], lk[1]), (lk[3], lk[5]), (lk[2], lk[4])]
    return [s for s, _ in out], [e for _, e in out]


def accepted(name):
    """The shared cases whose directory is built (the literal deep trees are refused)."""
    return not name.endswith("_literal")
