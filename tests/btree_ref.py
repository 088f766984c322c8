"""A Python restatement of the reference's page-based B-tree (btree/), written fresh for the tests of the B-tree's
read side: the page, cell and varint codec (btree/page.go, btree/varint.go), Put with both splits,
the root split and the update path (btree/split.go, page.go InsertCell / updateCell), LITERAL, bugs included, the
literal Get walk (linear findChild, searchCell), the page rules of the check, a bulk loader and the shared cases.

The literal splitInternal (split.go:141-164) gives the LEFT page the middle cell's child as its RightPtr and hands
the left page's old leftmost child to the NEW page: from the first internal split on, keys that were Put are no
longer reachable by Get.  Tree(fixed_split=True) assigns the two pointers the other way round, for sound deep trees.
A reader follows the image, so the tests compare with a walk of the image (get) and with the Put dictionary only
where the tree has depth <= 2 or was built fixed.

get() answers what the library answers: the reference's walk with the bisection and the departures that
include/seb_bloom.h states (a page type that is neither 1 nor 2, a touched cell that does not parse, a page id
outside [1, num_pages) and a walk of more than MAX_DEPTH pages are ERROR).  On every internal page the check calls
good it also runs findChild's linear scan and asserts that both agree.

Beside the trees that Put builds, cases() holds bulk-loaded images with pages wider than the 64 lanes a wave strides
a directory with (leaves of 300 cells; internal pages of 63, 64, 65, 128, 129 and 133 cells) and chains of internal
pages without a cell up to the depth limit; corrupt_cases() holds edits of the widest image behind cell 63, chains
past the depth limit, and leaves at two levels.  corrupt_claims() states what each damaged image must give."""
import struct

import numpy as np

PAGE, HEADER, MAGIC, MAX_DEPTH = 4096, 10, 0x42545245, 32
NO_PAGE, NO_LEVEL = 0xFFFFFFFF, 0xFF
BAD, INTERNAL, LEAF = 0, 1, 2
MISS, FOUND, ERROR = 0, 1, 2


class PageFull(Exception):
    pass


# ---------------------------------------------------------------- varint (btree/varint.go)

def put_uvarint(x: int) -> bytes:
    out = bytearray()
    while x >= 0x80:
        out.append((x & 0x7F) | 0x80)
        x >>= 7
    out.append(x)
    return bytes(out)


def uvarint16(buf, at: int):
    """uvarint16 of buf[at: PAGE]: (value, length), or None where the reference returns n <= 0."""
    x = s = 0
    for i in range(PAGE - at if at < PAGE else 0):
        b = buf[at + i]
        if i == 9:
            return None
        if b < 0x80:
            if i == 8 and b > 1:
                return None
            x |= b << s
            return None if x > 0xFFFF else (x, i + 1)
        x |= (b & 0x7F) << s
        s += 7
    return None


def varint_size16(x: int) -> int:
    return 1 if x < 128 else 2 if x < 16384 else 3


# ---------------------------------------------------------------- a page (btree/page.go)

class Cell:
    __slots__ = ("key", "value", "child", "koff", "voff")

    def __init__(self, key, value=b"", child=0, koff=0, voff=0):
        self.key, self.value, self.child, self.koff, self.voff = bytes(key), bytes(value), child, koff, voff


class Page:
    def __init__(self, data=None, kind=LEAF, version=2):
        if data is None:
            self.d = bytearray(PAGE)
            self.d[0] = kind
            struct.pack_into(">HIHB", self.d, 1, 0, 0, PAGE, version)
        else:
            self.d = data  # a bytearray or a memoryview of one: edits go through

    type = property(lambda s: s.d[0])
    num_cells = property(lambda s: struct.unpack_from(">H", s.d, 1)[0], lambda s, n: struct.pack_into(">H", s.d, 1, n))
    right_ptr = property(lambda s: struct.unpack_from(">I", s.d, 3)[0], lambda s, v: struct.pack_into(">I", s.d, 3, v))
    free_ptr = property(lambda s: struct.unpack_from(">H", s.d, 7)[0], lambda s, v: struct.pack_into(">H", s.d, 7, v))
    is_leaf = property(lambda s: s.d[0] == LEAF)
    v1 = property(lambda s: s.d[9] <= 1)  # Version(): 0 reads as V1

    def cell_offset(self, i):
        return struct.unpack_from(">H", self.d, HEADER + 2 * i)[0]

    def set_cell_offset(self, i, off):
        struct.pack_into(">H", self.d, HEADER + 2 * i, off)

    def parse(self, off, leaf=None):
        """parseLeafCell / parseInternalCell at `off`; None for every error, and (the stated departure) where a V2
        internal cell's child id would be read past the page end."""
        d, leaf = self.d, self.is_leaf if leaf is None else leaf
        child = vs = 0
        if self.v1:
            head = 4 if leaf else 6
            if off + head > PAGE:
                return None
            ks = struct.unpack_from(">H", d, off)[0]
            if leaf:
                vs = struct.unpack_from(">H", d, off + 2)[0]
            else:
                child = struct.unpack_from(">I", d, off + 2)[0]
        else:
            if off + (2 if leaf else 5) > PAGE:
                return None
            a = uvarint16(d, off)
            if a is None:
                return None
            ks, n1 = a
            if leaf:
                b = uvarint16(d, off + n1)
                if b is None:
                    return None
                vs, n2 = b
            else:
                n2 = 4
                if off + n1 + 4 > PAGE:
                    return None
                child = struct.unpack_from(">I", d, off + n1)[0]
            head = n1 + n2
        if off + head + ks + vs > PAGE:
            return None
        k0 = off + head
        return Cell(d[k0: k0 + ks], d[k0 + ks: k0 + ks + vs], child, k0, k0 + ks)

    def cell_at(self, i, leaf=None):
        """CellAt; None also where the directory entry lies past the page end (the reference panics there)."""
        if i >= self.num_cells or HEADER + 2 * i + 2 > PAGE:
            return None
        return self.parse(self.cell_offset(i), leaf)

    def cell_size(self, ks, vs):
        if self.is_leaf:
            return 4 + ks + vs if self.v1 else varint_size16(ks) + varint_size16(vs) + ks + vs
        return 6 + ks if self.v1 else varint_size16(ks) + 4 + ks

    def is_full(self, ks, vs):
        return self.free_ptr - (HEADER + 2 * (self.num_cells + 1)) < self.cell_size(ks, vs)

    def search_cell(self, key):
        """searchCell: the insertion point, or -(index + 1) on a match; a cell that fails to parse ends it at `left`."""
        left, right = 0, self.num_cells
        while left < right:
            mid = (left + right) // 2
            c = self.cell_at(mid)
            if c is None:
                return left
            if key == c.key:
                return -(mid + 1)
            if key < c.key:
                right = mid
            else:
                left = mid + 1
        return left

    def write_cell(self, off, cell):
        leaf = self.is_leaf
        if self.v1:
            head = struct.pack(">HH", len(cell.key), len(cell.value)) if leaf else struct.pack(">HI", len(cell.key), cell.child)
        else:
            head = put_uvarint(len(cell.key)) + (put_uvarint(len(cell.value)) if leaf else struct.pack(">I", cell.child))
        body = head + cell.key + (cell.value if leaf else b"")
        self.d[off: off + len(body)] = body

    def insert_cell(self, cell):
        ks, vs = len(cell.key), len(cell.value) if self.is_leaf else 0
        if self.is_full(ks, vs):  # tested BEFORE the key is looked for: an update on a full page splits
            raise PageFull
        n, pos = self.num_cells, self.search_cell(cell.key)
        if pos < 0:  # updateCell: delete + insert
            self.delete_cell(-pos - 1)
            return self.insert_cell(cell)
        free = self.free_ptr - self.cell_size(ks, vs)
        self.write_cell(free, cell)
        for i in range(n, pos, -1):
            self.set_cell_offset(i, self.cell_offset(i - 1))
        self.set_cell_offset(pos, free)
        self.num_cells, self.free_ptr = n + 1, free

    def delete_cell(self, i):
        """DeleteCell: only the directory shifts; the cell's bytes stay behind as dead space."""
        n = self.num_cells
        assert i < n
        for j in range(i, n - 1):
            self.set_cell_offset(j, self.cell_offset(j + 1))
        self.num_cells = n - 1

    def cells(self):
        return [self.cell_at(i) for i in range(self.num_cells)]


# ---------------------------------------------------------------- the tree (btree/btree.go, split.go, pager.go)

class Tree:
    """Put / Delete / image().  fixed_split: splitInternal's two pointers assigned correctly.  version: the byte new
    pages carry (2 = V2 as the reference writes; 0 or 1 = V1)."""

    def __init__(self, fixed_split=False, version=2):
        self.fixed, self.version = fixed_split, version
        self.pages = [None, Page(kind=LEAF, version=version)]  # createPager: metadata + an empty root leaf
        self.root, self.free_list = 1, 0
        self.puts = {}
        self.internal_splits = 0

    def new_page(self, kind):
        self.pages.append(Page(kind=kind, version=self.version))
        return len(self.pages) - 1

    def find_child(self, page, key):
        return find_child_linear(page, key)

    def get_child_page_id(self, page, key):  # node.go:19-57: as findChild, but a bad cell is an error
        n = page.num_cells
        for i in range(n):
            c = page.cell_at(i)
            assert c is not None
            if key >= c.key:
                if i + 1 < n:
                    nx = page.cell_at(i + 1)
                    if nx is not None and key >= nx.key:
                        continue
                return c.child
        assert page.right_ptr != 0
        return page.right_ptr

    def put(self, key, value):
        assert len(key) > 0
        split = self._insert_and_split(self.root, key, value)
        if split:  # handleRootSplit
            new_root = self.new_page(INTERNAL)
            self.pages[new_root].insert_cell(Cell(split[0], child=split[1]))
            self.pages[new_root].right_ptr = self.root
            self.root = new_root
        self.puts[bytes(key)] = bytes(value)
        return self

    def _insert_and_split(self, pid, key, value):
        page = self.pages[pid]
        if page.is_leaf:
            try:
                page.insert_cell(Cell(key, value))
                return None
            except PageFull:
                return self._split(page, Cell(key, value), True)
        child = self.get_child_page_id(page, key)
        split = self._insert_and_split(child, key, value)
        if not split:
            return None
        cell = Cell(split[0], child=split[1])
        try:
            page.insert_cell(cell)
            return None
        except PageFull:
            return self._split(page, cell, False)

    def _split(self, page, new_cell, leaf):
        """splitLeaf / splitInternal: returns (separator key, new page id)."""
        cells = page.cells()
        assert all(c is not None for c in cells)
        pos = 0
        for i, c in enumerate(cells):
            if new_cell.key < c.key:
                pos = i
                break
            pos = i + 1
        cells.insert(pos, new_cell)
        mid = len(cells) // 2
        new_id = self.new_page(LEAF if leaf else INTERNAL)
        new = self.pages[new_id]
        old_right = page.right_ptr
        page.num_cells, page.free_ptr = 0, PAGE
        for c in cells[:mid]:
            page.insert_cell(c)
        if leaf:
            for c in cells[mid:]:
                new.insert_cell(c)
            page.right_ptr, new.right_ptr = new_id, old_right  # the leaf chain
            return new.cell_at(0).key, new_id
        self.internal_splits += 1
        for c in cells[mid + 1:]:
            new.insert_cell(c)
        if self.fixed:
            page.right_ptr, new.right_ptr = old_right, cells[mid].child
        else:  # literal, split.go:153-164: the two leftmost children change places
            page.right_ptr, new.right_ptr = cells[mid].child, old_right
        return cells[mid].key, new_id

    def delete(self, key):
        """Delete as DeleteCell on the leaf, WITHOUT the rebalancing (mergeOrRedistribute) that follows it in the
        reference: such images are valid (an underfull or empty leaf is a page like any other) and test-made."""
        pid = self.root
        while not self.pages[pid].is_leaf:
            pid = self.find_child(self.pages[pid], key)
        i = self.pages[pid].search_cell(key)
        if i < 0:
            self.pages[pid].delete_cell(-i - 1)
            self.puts.pop(bytes(key), None)
        return self

    def depth(self):
        d, pid = 1, self.root
        while not self.pages[pid].is_leaf:
            d, pid = d + 1, self.pages[pid].right_ptr
        return d

    def image(self, header_pages=None) -> bytes:
        n = len(self.pages)
        meta = bytearray(PAGE)
        struct.pack_into(">IIII", meta, 0, MAGIC, self.root, n if header_pages is None else header_pages, self.free_list)
        return bytes(meta) + b"".join(bytes(p.d) for p in self.pages[1:])


def find_child_linear(page, key):
    """findChild (btree.go:200-229), literal: the last cell with key >= cell.Key, bad cells skipped with `continue`."""
    n = page.num_cells
    for i in range(n):
        c = page.cell_at(i, leaf=False)
        if c is None:
            continue
        if key >= c.key:
            if i + 1 < n:
                nx = page.cell_at(i + 1, leaf=False)
                if nx is not None and key >= nx.key:
                    continue
            return c.child
    return page.right_ptr


# ---------------------------------------------------------------- open, check, get on an image

def open_image(image):
    """readMetadata: dict(root, header_pages, free_list, num_pages), or None for ErrInvalidDatabase."""
    if len(image) < PAGE:
        return None
    magic, root, pages, free = struct.unpack_from(">IIII", image, 0)
    if magic != MAGIC:
        return None
    return dict(root=root, header_pages=pages, free_list=free, num_pages=min(pages, len(image) // PAGE))


def page_of(image, p):
    return Page(memoryview(image)[p * PAGE: (p + 1) * PAGE])


def page_kind(page, num_pages):
    ok_id = lambda c: 1 <= c < num_pages  # noqa: E731
    if page.type not in (INTERNAL, LEAF):
        return BAD
    n = page.num_cells
    if HEADER + 2 * n > PAGE:
        return BAD
    if not (ok_id(page.right_ptr) or (page.is_leaf and page.right_ptr == 0)):
        return BAD
    prev = None
    for i in range(n):
        c = page.cell_at(i)
        if c is None or (not page.is_leaf and not ok_id(c.child)) or (prev is not None and not prev < c.key):
            return BAD
        prev = c.key
    return page.type


def check(image, meta):
    """(kind u8[num_pages], level u8[num_pages], stats dict) by the rules of seb_bt_check."""
    n = meta["num_pages"]
    kind, level = np.zeros(n, np.uint8), np.full(n, NO_LEVEL, np.uint8)
    for p in range(1, n):
        kind[p] = page_kind(page_of(image, p), n)
    front = []
    if 1 <= meta["root"] < n:
        level[meta["root"]] = 0
        front = [meta["root"]]
    for r in range(MAX_DEPTH - 1):
        nxt = []
        for p in front:
            if kind[p] != INTERNAL:
                continue
            pg = page_of(image, p)
            for c in [pg.right_ptr] + [x.child for x in pg.cells()]:
                if 1 <= c < n and level[c] == NO_LEVEL:
                    level[c] = r + 1
                    nxt.append(c)
        front = nxt
    reach = level != NO_LEVEL
    body = np.arange(n) >= 1
    leaves = [p for p in range(1, n) if reach[p] and kind[p] == LEAF]
    st = dict(leaves=int(((kind == LEAF) & body).sum()), internals=int(((kind == INTERNAL) & body).sum()),
              bad=int(((kind == BAD) & body).sum()), reach_leaves=len(leaves),
              reach_internals=int(((kind == INTERNAL) & reach).sum()), reach_bad=int(((kind == BAD) & reach & body).sum()),
              keys=sum(page_of(image, p).num_cells for p in leaves), depth=int(level[reach].max()) + 1 if reach.any() else 0,
              uniform=int(len({int(level[p]) for p in leaves}) <= 1))
    return kind, level, st


def get(image, meta, key, kind=None):
    """(status, leaf, pos, vloc, vlen) for one key, as seb_bt_get answers.  kind (check's): where given, every good
    internal page also runs the literal linear findChild, which must pick the same child."""
    if len(key) == 0:
        return ERROR, NO_PAGE, 0, 0, 0
    n, pid = meta["num_pages"], meta["root"]
    for _ in range(MAX_DEPTH):
        if not 1 <= pid < n:
            return ERROR, pid, 0, 0, 0
        pg, last = page_of(image, pid), pid
        if pg.type not in (INTERNAL, LEAF):
            return ERROR, pid, 0, 0, 0
        lo, hi, child = 0, pg.num_cells, pg.right_ptr
        while lo < hi:
            mid = (lo + hi) // 2
            c = pg.cell_at(mid)
            if c is None:
                return ERROR, pid, 0, 0, 0
            if pg.is_leaf and key == c.key:
                return FOUND, pid, mid, pid * PAGE + c.voff, len(c.value)
            if key < c.key:
                hi = mid
            else:
                lo, child = mid + 1, c.child
        if pg.is_leaf:
            return MISS, pid, lo, 0, 0
        if kind is not None and kind[pid] == INTERNAL:
            assert find_child_linear(pg, key) == child, "the bisection and findChild's scan differ on a good page"
        pid = child
    return ERROR, last, 0, 0, 0


def get_batch(image, meta, keys, kind=None):
    """Arrays (status u8, leaf u32, pos u32, vloc u64, vlen u32) over a key list."""
    rows = [get(image, meta, k, kind) for k in keys]
    cols = list(zip(*rows)) if rows else [[]] * 5
    return tuple(np.array(c, t) for c, t in zip(cols, (np.uint8, np.uint32, np.uint32, np.uint64, np.uint32)))


def values(image, answers):
    """The found keys' value bytes, in batch order."""
    st, _, _, vloc, vlen = answers
    return [bytes(image[int(o): int(o) + int(n)]) for s, o, n in zip(st, vloc, vlen) if s == FOUND]


# ---------------------------------------------------------------- bulk loader

def bulk_load(keys, vals, leaf_cells=64, fanout=32):
    """A page-at-a-time loader for large images: sorted distinct keys, leaf_cells cells per leaf (fewer where the
    page fills), fanout children per internal page; V2 pages.  Returns the image."""
    assert all(a < b for a, b in zip(keys, keys[1:]))
    pages = []  # bytearrays, page ids from 1

    def build(kind, cells, right):
        pg = Page(kind=kind)
        free = PAGE
        for i, c in enumerate(cells):
            free -= pg.cell_size(len(c.key), len(c.value))
            assert free >= HEADER + 2 * (i + 1), "the page overflows: lower leaf_cells / fanout"
            pg.write_cell(free, c)
            pg.set_cell_offset(i, free)
        pg.num_cells, pg.free_ptr, pg.right_ptr = len(cells), free, right
        pages.append(pg.d)
        return len(pages)

    level = []  # (min key, page id)
    groups = [list(range(i, min(i + leaf_cells, len(keys)))) for i in range(0, len(keys), leaf_cells)] or [[]]
    for g, idx in enumerate(groups):
        nxt = len(pages) + 2 if g + 1 < len(groups) else 0
        pid = build(LEAF, [Cell(keys[i], vals[i]) for i in idx], nxt)
        level.append((keys[idx[0]] if idx else b"", pid))
    while len(level) > 1:
        up = []
        for i in range(0, len(level), fanout):
            grp = level[i: i + fanout]
            pid = build(INTERNAL, [Cell(k, child=p) for k, p in grp[1:]], grp[0][1])
            up.append((grp[0][0], pid))
        level = up
    meta = bytearray(PAGE)
    struct.pack_into(">IIII", meta, 0, MAGIC, level[0][1], len(pages) + 1, 0)
    return bytes(meta) + b"".join(bytes(p) for p in pages)


# ---------------------------------------------------------------- the shared cases

class Case:
    """image; puts: the Put dictionary where Get must equal it (depth <= 2 or a fixed build, no cell touched by
    hand), else None; keys: the keys that were Put (for probes); seps: every separator key of the image."""

    def __init__(self, image, keys, puts=None, random3=0):
        self.image, self.keys, self.puts, self.random3 = image, sorted(keys), puts, random3
        self.meta = open_image(image)
        self.seps = []
        for p in range(1, self.meta["num_pages"]):
            pg = page_of(image, p)
            if pg.type == INTERNAL and page_kind(pg, self.meta["num_pages"]) == INTERNAL:
                self.seps += [c.key for c in pg.cells()]


def _tree_case(tree, sound):
    return Case(tree.image(), list(tree.puts), dict(tree.puts) if sound else None)


def _wide(i):
    return (b"wide-%05d-" % i) + bytes([65 + i % 26]) * 188  # 200-byte keys


def _deep(n, fixed):
    t = Tree(fixed_split=fixed)
    order = np.random.default_rng(n).permutation(n)
    for i in order:
        t.put(_wide(int(i)), bytes([i % 251]) * 700)
    return t


def _keys3(n, seed):
    """n sorted distinct 3-byte keys."""
    ids = np.sort(np.random.default_rng(seed).choice(1 << 24, n, replace=False))
    return [int(i).to_bytes(3, "big") for i in ids]


def _wide_case(n, leaf_cells, fanout, seed, random3=2000):
    """Pages wider than a wave: n 3-byte keys with values b"" and b"v", bulk-loaded."""
    keys = _keys3(n, seed)
    vals = [b"v" if k[2] & 1 else b"" for k in keys]
    return Case(bulk_load(keys, vals, leaf_cells=leaf_cells, fanout=fanout), keys, dict(zip(keys, vals)), random3)


# (leaf_cells, fanout): internal pages of 63, 64, 65 and 128 cells, i.e. 64, 65, 66 and 129 children with the right
# pointer: the widths at which the right pointer changes lane and pass of a 64-lane loop over i <= n
BOUNDARY = ((63, 64), (64, 65), (65, 66), (128, 129))


def widths(image):
    """(the cell counts of the good leaves, of the good internal pages) of an image, as two sorted lists."""
    n = open_image(image)["num_pages"]
    out = {LEAF: [], INTERNAL: []}
    for p in range(1, n):
        pg = page_of(image, p)
        if page_kind(pg, n) != BAD:
            out[pg.type].append(pg.num_cells)
    return sorted(out[LEAF]), sorted(out[INTERNAL])


CHAIN_KEY, CHAIN_VALUE = b"end-of-chain", b"found"


def chain_image(d):
    """d internal pages without a cell, page i pointing right to page i + 1, then a one-key leaf: a tree of depth
    d + 1 whose root is page 1.  MAX_DEPTH - 1 internal pages is the deepest tree that Get walks to its leaf."""
    pages = []
    for i in range(1, d + 1):
        pg = Page(kind=INTERNAL)
        pg.right_ptr = i + 1
        pages.append(pg)
    leaf = Page(kind=LEAF)
    leaf.insert_cell(Cell(CHAIN_KEY, CHAIN_VALUE))
    pages.append(leaf)
    meta = bytearray(PAGE)
    struct.pack_into(">IIII", meta, 0, MAGIC, 1, d + 2, 0)
    return bytes(meta) + b"".join(bytes(p.d) for p in pages)


_CACHE = {}


def cases():
    """name -> Case; built once per process."""
    if _CACHE:
        return _CACHE
    c = _CACHE
    c["a_empty"] = _tree_case(Tree(), True)
    c["b_one_key"] = _tree_case(Tree().put(b"only", b"value"), True)
    t = Tree()
    for kl in (1, 127, 128):
        for vl in (0, 127, 128, 1500):
            t.put(bytes([0x40 + len(t.puts)]) * kl, bytes([vl % 256 or 7]) * vl)
    c["c_lengths"] = _tree_case(t, True)
    t = Tree()
    base = b"0123456789abcdefXYZ"
    for k in (b"k", b"k\0", b"k\0\0", base[:8] + b"A", base[:8] + b"B", base[:16] + b"A", base[:16] + b"B", base[:17] + b"A",
              base[:17] + b"B", base[:16], base[:8], base, base + b"\0", b"\0", b"\0\0", b"\xff" * 16, b"\xff" * 17):
        t.put(k, b"v:" + k)
    c["d_prefixes"] = _tree_case(t, True)
    t = Tree()
    for i in range(60):
        t.put(b"key-%04d" % (i * 7 % 60), b"val-%d-" % i + b"x" * 100)
    assert t.depth() == 2
    c["e_root_split"] = _tree_case(t, True)
    for name, n, depth in (("f_depth3", 400, 3), ("g_depth4", 3000, 4)):
        for fixed in (False, True):
            t = _deep(n, fixed)
            assert t.depth() == depth and t.internal_splits > 0, (name, t.depth())
            c[name + ("_fixed" if fixed else "_literal")] = _tree_case(t, fixed)
    # updates and deletes: directory order differs from physical order; one leaf of the chain is emptied
    t = Tree()
    for i in range(200):
        t.put(b"u-%04d" % i, b"first-%d" % i + b"." * 40)
    for i in range(0, 200, 3):
        t.put(b"u-%04d" % i, b"second-%d" % i + b"!" * (i % 60))
    for i in range(5, 200, 11):
        t.delete(b"u-%04d" % i)
    mid_leaf = t.pages[t.root].cell_at(0).child
    for cell in t.pages[mid_leaf].cells():
        t.delete(cell.key)
    assert t.pages[mid_leaf].num_cells == 0 and t.pages[mid_leaf].right_ptr != 0 and t.depth() == 2
    c["h_updates_deletes"] = _tree_case(t, True)
    # hand-made V1 pages (version byte 0 and 1) among V2 pages: two leaves and the root re-encoded
    t = Tree()
    for i in range(300):
        t.put(b"mix-%04d" % i, b"v" * (i % 90))
    leaves = [t.pages[t.root].right_ptr] + [x.child for x in t.pages[t.root].cells()]
    for pid, ver in ((leaves[0], 0), (leaves[2], 1), (t.root, 1)):
        old = t.pages[pid]
        new = Page(kind=old.type, version=ver)
        for cell in old.cells():
            new.insert_cell(cell)
        new.right_ptr = old.right_ptr
        t.pages[pid] = new
    assert len(leaves) >= 4
    c["i_v1_mixed"] = Case(t.image(), list(t.puts), None)
    # pages wider than a wave (a wave per page, the lanes striding the directory by 64)
    c["j_wide_300"] = _wide_case(40_000, 300, 200, 300)      # leaves of 300 cells under a root of 133
    c["k_wide_3level"] = _wide_case(40_000, 100, 130, 100)   # 400 leaves under internal pages of 129 cells
    for lc, fo in BOUNDARY:
        c["l_boundary_%d" % (fo - 1)] = _wide_case(2 * lc * fo, lc, fo, fo, random3=500)
    # the deepest trees that Get still walks to the leaf: depth 31 and 32
    for d in (30, 31):
        c["m_chain_%d" % d] = Case(chain_image(d), [CHAIN_KEY], {CHAIN_KEY: CHAIN_VALUE})
    return c


def probes(case, rng, cap=120, random3=None):
    """Present keys, absent keys between neighbours, keys below the minimum and above the maximum, every separator,
    a present key with one byte appended and with its last byte dropped, the empty key; then random3 (default: the
    case's) 3-byte keys, half of them present."""
    keys = case.keys
    pick = keys if len(keys) <= cap else [keys[i] for i in sorted(rng.choice(len(keys), cap, replace=False))]
    out = list(pick)
    for k in pick[: cap // 2]:
        out += [k + b"\0", k + b"\x7f", k[:-1]]
    out += [b"\0", b"\x01", b"\xff" * 3, b"\xff" * 40, b""]
    if keys:
        out += [keys[0][:-1], keys[0][:1], keys[-1] + b"\xff", keys[-1] + b"\0"]
    out += case.seps + [s + b"\0" for s in case.seps[:40]] + [s[:-1] for s in case.seps[:40]]
    random3 = case.random3 if random3 is None else random3
    if random3:
        out += [keys[i] for i in rng.integers(0, len(keys), random3 // 2)]
        out += [r.tobytes() for r in rng.integers(0, 256, (random3 - random3 // 2, 3), dtype=np.uint8)]
    return out


def long_keys(case):
    """Batch keys longer than any stored key, three of them a present key followed by zeros to around the 65,536
    bytes that a compare looks at."""
    k = case.keys[3]
    return [k + b"\0" * 70000, b"\xff" * 66000, case.keys[0]] + [k + b"\0" * (n - len(k)) for n in (65535, 65536, 65537)]


def _base_tree():
    t = Tree()
    for i in range(150):
        t.put(b"c-%04d" % i, b"value-%d-" % i + b"z" * 60)
    assert t.depth() == 2 and t.pages[t.root].num_cells >= 3
    return t


_CORRUPT, _CLAIMS = {}, {}


def corrupt_claims():
    """name -> what a damaged image of corrupt_cases() must give beyond equality with the restatement: "bad": the
    pages that the check calls bad (exactly these); "errors": whether more than the empty key's ERROR is answered;
    "stats": counts of the check; "level": page -> level."""
    corrupt_cases()
    return _CLAIMS


def corrupt_cases():
    """name -> (image, probe keys): data errors that a status answers, built once per process.  corrupt_claims()
    says which of them must give an ERROR and which pages the check must call bad."""
    if _CORRUPT:
        return _CORRUPT
    out = {}
    t = _base_tree()
    good = t.image()
    keys = sorted(t.puts) + [b"a", b"zzz", b"c-0075x", b""]
    root = t.root
    leaves = [t.pages[root].right_ptr] + [c.child for c in t.pages[root].cells()]
    n = len(t.pages)

    def edit(fn, image=good):  # fn(bytes, the base tree's root page, page id -> page)
        b = bytearray(image)
        fn(b, Page(memoryview(b)[root * PAGE: (root + 1) * PAGE]), lambda p: Page(memoryview(b)[p * PAGE: (p + 1) * PAGE]))
        return bytes(b)

    def child_field(rp, i):  # the offset of cell i's child id in a V2 internal page
        off = rp.cell_offset(i)
        return off + uvarint16(rp.d, off)[1]

    out["child_past_end"] = edit(lambda b, rp, pg: struct.pack_into(">I", rp.d, child_field(rp, 0), n + 5))
    out["child_zero"] = edit(lambda b, rp, pg: struct.pack_into(">I", rp.d, child_field(rp, 1), 0))
    out["cell_offset_past_page"] = edit(lambda b, rp, pg: pg(leaves[1]).set_cell_offset(3, 4095))
    out["num_cells_3000"] = edit(lambda b, rp, pg: setattr(pg(leaves[0]), "num_cells", 3000))

    def long_varint(b, rp, pg):
        p = pg(leaves[1])
        at = HEADER + 2 * p.num_cells + 4
        assert at + 11 < p.free_ptr
        p.d[at: at + 11] = b"\x80" * 10 + b"\x00"
        p.set_cell_offset(2, at)
    out["varint_too_long"] = edit(long_varint)

    def key_past_end(b, rp, pg):
        p = pg(leaves[2])
        p.d[4090: 4092] = bytes([100, 1])  # keySize 100, valueSize 1 at offset 4090
        p.set_cell_offset(p.num_cells // 2, 4090)
    out["key_past_page_end"] = edit(key_past_end)
    out["type_7"] = edit(lambda b, rp, pg: pg(leaves[1]).d.__setitem__(0, 7))
    out["self_pointer"] = edit(lambda b, rp, pg: setattr(rp, "right_ptr", root))
    big = bytearray(good)
    struct.pack_into(">I", big, 8, 1000)  # NumPages above the file's pages, and the file cut short
    out["num_pages_past_image"] = bytes(big[: (n - 1) * PAGE])

    def unsorted(b, rp, pg):
        p = pg(leaves[1])
        a, c = p.cell_offset(1), p.cell_offset(2)
        p.set_cell_offset(1, c), p.set_cell_offset(2, a)
    out["unsorted"] = edit(unsorted)
    _CORRUPT.update({k: (v, keys) for k, v in out.items()})
    _CLAIMS.update({k: dict(errors=k != "unsorted") for k in out})
    _CLAIMS["unsorted"]["bad"] = [leaves[1]]

    # ---- wide pages, each edit on the 300-cell image: exactly the edited page turns bad
    wide = cases()["j_wide_300"]
    wkeys = probes(wide, np.random.default_rng(23), random3=300)
    wn, wroot = wide.meta["num_pages"], wide.meta["root"]
    wleaf = page_of(wide.image, wroot).cell_at(70).child  # a leaf of 300 cells in the middle of the key space
    assert page_of(wide.image, wleaf).num_cells == 300 and page_of(wide.image, wroot).num_cells > 128
    # every key of the edited leaf and of the leaf under the root's edited cell: the bisections touch every cell
    wkeys = wkeys + [c.key for p in (wleaf, page_of(wide.image, wroot).cell_at(100).child) for c in page_of(wide.image, p).cells()]

    def swap(i, j):
        def fn(b, rp, pg):
            p = pg(wleaf)
            a, c = p.cell_offset(i), p.cell_offset(j)
            p.set_cell_offset(i, c), p.set_cell_offset(j, a)
        return fn

    def wide_case(name, fn, bad, errors):
        _CORRUPT[name] = (edit(fn, wide.image), wkeys)
        _CLAIMS[name] = dict(errors=errors, bad=[bad])

    wide_case("wide_swap_63_64", swap(63, 64), wleaf, False)
    wide_case("wide_swap_64_65", swap(64, 65), wleaf, False)
    wide_case("wide_swap_last_pair", swap(298, 299), wleaf, False)
    wide_case("wide_child_past_end_100", lambda b, rp, pg: struct.pack_into(">I", pg(wroot).d, child_field(pg(wroot), 100), wn + 5),
              wroot, True)
    wide_case("wide_cell_offset_4095_at_200", lambda b, rp, pg: pg(wleaf).set_cell_offset(200, 4095), wleaf, True)
    wide_case("wide_duplicate_127_128", lambda b, rp, pg: pg(wleaf).set_cell_offset(128, pg(wleaf).cell_offset(127)), wleaf, False)

    # ---- chains too deep for Get: the levels stop at MAX_DEPTH - 1, the leaf is never reached
    for d in (32, 33):
        _CORRUPT["chain_%d" % d] = (chain_image(d), [CHAIN_KEY, b"a", b"zzz", b""])
        _CLAIMS["chain_%d" % d] = dict(errors=True, bad=[], stats=dict(depth=MAX_DEPTH, reach_leaves=0, reach_internals=MAX_DEPTH,
                                                                        leaves=1, internals=d, keys=0, uniform=1))

    # ---- leaves at two levels, a page with two parents (the depth-3 fixed build edited)
    deep = cases()["f_depth3_fixed"]
    dkeys = probes(deep, np.random.default_rng(29))
    droot, dn = deep.meta["root"], deep.meta["num_pages"]
    drp = page_of(deep.image, droot)
    first, second = drp.right_ptr, drp.cell_at(0).child  # the root's two leftmost subtrees
    leaf_a = page_of(deep.image, first).right_ptr
    # the root points right at a level-2 leaf of its own first subtree: that subtree's page and other leaves are lost
    _CORRUPT["two_levels"] = (edit(lambda b, rp, pg: setattr(pg(droot), "right_ptr", leaf_a), deep.image), dkeys)
    _CLAIMS["two_levels"] = dict(errors=False, bad=[], level={leaf_a: 1}, stats=dict(uniform=0, reach_leaves=119, keys=345, leaves=138,
                                                                                      internals=11, reach_internals=10, depth=3))
    # the root's first cell points at that leaf, whose parent stays reachable: level 1 from the root, 2 from the parent
    _CORRUPT["two_parents"] = (edit(lambda b, rp, pg: struct.pack_into(">I", pg(droot).d, child_field(pg(droot), 0), leaf_a), deep.image),
                               dkeys)
    lost = page_of(deep.image, second).num_cells + 1
    _CLAIMS["two_parents"] = dict(errors=False, bad=[], level={leaf_a: 1, first: 1}, stats=dict(uniform=0, reach_leaves=138 - lost,
                                                                                                 reach_internals=10, depth=3))
    # the one leaf at another level is the image's last page: a copy of leaf_a appended, the root pointing right at it
    b = bytearray(deep.image) + deep.image[leaf_a * PAGE: (leaf_a + 1) * PAGE]
    struct.pack_into(">I", b, 8, dn + 1)
    page_of(b, droot).right_ptr = dn
    _CORRUPT["last_page_other_level"] = (bytes(b), dkeys)
    _CLAIMS["last_page_other_level"] = dict(errors=False, bad=[], level={dn: 1}, stats=dict(uniform=0, leaves=139, depth=3,
                                            reach_leaves=139 - (page_of(deep.image, first).num_cells + 1)))
    return _CORRUPT
