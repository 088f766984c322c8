// seb_btree.h — the B-tree's read side: what its host half (seb_btree.cpp, no HIP dependency) and
// its kernels (seb_btree.hip) share.  The page codec, the page rules of the check and the walk of Get are written
// ONCE here and compiled for both sides, so the device form cannot drift from its reference; only the key compare
// differs (memcmp on the host, seb_keycmp.h's prefix words on the device) and is passed in.
//
// The image (btree/pager.go, btree/page.go): page p at byte p * 4096, page 0 the metadata, every integer big-endian.
// A page: [type u8][numCells u16][rightPtr u32][freePtr u16][version u8], a directory of u16 cell offsets in key
// order, cells growing down from the page end.  Version 0 or 1 is V1 (fixed u16 sizes), anything else V2 (varints).
//
// Bounds, whatever the image holds: no function here reads a byte outside the 4096 of the page it is given; every
// offset is tested before it is used; every loop is counted.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SEB_BT_HD __host__ __device__ __forceinline__
#else
#define SEB_BT_HD inline
#endif

namespace seb {

constexpr uint32_t kBtPage = 4096;
constexpr uint32_t kBtHeader = 10;  // the page header; the directory follows
constexpr uint32_t kBtMagic = 0x42545245u;
constexpr uint32_t kBtMaxDepth = 32;
constexpr uint32_t kBtNoPage = 0xFFFFFFFFu;
constexpr uint32_t kBtNoLevel = 0xFF;
constexpr uint32_t kBtMaxKey = 0x10000;  // a batch key is compared as its first 65,536 bytes: no stored key is longer
enum : uint8_t { kBtBad = 0, kBtInternal = 1, kBtLeaf = 2 };
enum : uint8_t { kBtMiss = 0, kBtFound = 1, kBtError = 2 };  // SEB_GET_*

struct BtMeta {  // seb_bt_meta
    uint32_t root, header_pages, free_list, num_pages;
};

struct BtStats {  // seb_bt_stats
    uint64_t leaves, internals, bad;                    // pages [1, num_pages)
    uint64_t reach_leaves, reach_internals, reach_bad;  // those with a level
    uint64_t keys;                                      // the cells on reachable good leaves
    uint32_t depth, uniform;  // levels that hold a reachable page; 1 iff every reachable good leaf sits at one level
};

struct BtCell {  // offsets within the page
    uint32_t koff, klen;
    uint32_t voff, vlen;  // leaf
    uint32_t child;       // internal
};

struct BtAnswer {
    uint8_t status;
    uint32_t leaf, pos, vlen;
    uint64_t vloc;
};

SEB_BT_HD uint32_t bt_be16(const uint8_t *p) { return (uint32_t)p[0] << 8 | p[1]; }
SEB_BT_HD uint32_t bt_be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// uvarint16 (btree/varint.go:34-85) of page[at, 4096): the value and its length, or false where the reference gives
// n <= 0: the bytes end inside it, a tenth byte, a ninth byte above 1, a value above 0xFFFF.
SEB_BT_HD bool bt_varint(const uint8_t *page, uint32_t at, uint32_t *val, uint32_t *len) {
    uint64_t x = 0;
    for (uint32_t i = 0; i < 9; ++i) {
        if (at + i >= kBtPage) return false;
        const uint32_t b = page[at + i];
        if (b < 0x80) {
            if (i == 8 && b > 1) return false;
            x |= (uint64_t)b << (7 * i);
            if (x > 0xFFFF) return false;
            *val = (uint32_t)x, *len = i + 1;
            return true;
        }
        x |= (uint64_t)(b & 0x7f) << (7 * i);
    }
    return false;
}

// parseLeafCell / parseInternalCell (btree/page.go:198-316) at offset `off` (any u16).  ONE DEPARTURE: a V2 internal
// cell whose child id would be read past the page end is an error here; the reference panics on that slice.
SEB_BT_HD bool bt_parse(const uint8_t *page, bool leaf, bool v1, uint32_t off, BtCell *c) {
    uint32_t ks, vs = 0, head;
    c->child = 0;
    if (v1) {
        head = leaf ? 4 : 6;
        if (off + head > kBtPage) return false;
        ks = bt_be16(page + off);
        if (leaf) vs = bt_be16(page + off + 2);
        else c->child = bt_be32(page + off + 2);
    } else {
        uint32_t n1, n2 = 4;
        if (off + (leaf ? 2 : 5) > kBtPage || !bt_varint(page, off, &ks, &n1)) return false;
        if (leaf) {
            if (!bt_varint(page, off + n1, &vs, &n2)) return false;
        } else {
            if (off + n1 + 4 > kBtPage) return false;
            c->child = bt_be32(page + off + n1);
        }
        head = n1 + n2;
    }
    if (off + head + ks + vs > kBtPage) return false;
    c->koff = off + head, c->klen = ks, c->voff = off + head + ks, c->vlen = vs;
    return true;
}

// cell i of a page with n cells: its directory entry must lie inside the page (the reference's getCellOffset panics
// beyond it: the second departure), then bt_parse
SEB_BT_HD bool bt_cell(const uint8_t *page, bool leaf, bool v1, uint32_t i, BtCell *c) {
    if (kBtHeader + 2 * i + 2 > kBtPage) return false;
    return bt_parse(page, leaf, v1, bt_be16(page + kBtHeader + 2 * i), c);
}

SEB_BT_HD int bt_bytes_cmp(const uint8_t *a, uint32_t alen, const uint8_t *b, uint32_t blen) {  // bytes.Compare
    const uint32_t n = alen < blen ? alen : blen;
    for (uint32_t i = 0; i < n; ++i)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return alen == blen ? 0 : alen < blen ? -1 : 1;
}

SEB_BT_HD bool bt_page_id_ok(uint32_t id, uint32_t num_pages) { return id >= 1 && id < num_pages; }

// The check's rules for cell i of a page whose type is 1 or 2 and whose directory fits: it parses, it is strictly
// below cell i + 1 (which parses too), and an internal cell's child lies in [1, num_pages).
SEB_BT_HD bool bt_cell_good(const uint8_t *page, bool leaf, bool v1, uint32_t n, uint32_t i, uint32_t num_pages) {
    BtCell a, b;
    if (!bt_cell(page, leaf, v1, i, &a)) return false;
    if (!leaf && !bt_page_id_ok(a.child, num_pages)) return false;
    if (i + 1 < n) {
        if (!bt_cell(page, leaf, v1, i + 1, &b)) return false;
        if (bt_bytes_cmp(page + a.koff, a.klen, page + b.koff, b.klen) >= 0) return false;
    }
    return true;
}

// what the check tests before the cells: the type, the directory, the right pointer; *n = numCells
SEB_BT_HD uint8_t bt_page_head(const uint8_t *page, uint32_t num_pages, uint32_t *n) {
    const uint8_t type = page[0];
    *n = bt_be16(page + 1);
    if (type != kBtInternal && type != kBtLeaf) return kBtBad;
    if (kBtHeader + 2 * *n > kBtPage) return kBtBad;
    const uint32_t right = bt_be32(page + 3);
    if (!(bt_page_id_ok(right, num_pages) || (type == kBtLeaf && right == 0))) return kBtBad;
    return type;
}

// One page of Get's walk.  cmp(stored, len) = the sign of bytes.Compare(key, stored key).  Returns true when the
// walk goes on to *next; false when `a` holds the answer.  A leaf is searchCell (btree/page.go:451-473) literally;
// an internal page bisects for the last cell with key >= cell.Key, which on every page the check calls good is
// findChild's linear scan (btree/btree.go:200-229).  A cell that fails to parse is SEB_GET_ERROR here, where
// searchCell would answer "not found" and findChild would skip the cell: the third departure.
template <class Cmp>
SEB_BT_HD bool bt_page_step(const uint8_t *page, uint32_t id, const Cmp &cmp, BtAnswer *a, uint32_t *next) {
    a->leaf = id, a->pos = 0;
    const uint8_t type = page[0];
    if (type != kBtInternal && type != kBtLeaf) return false;
    const bool leaf = type == kBtLeaf, v1 = page[9] <= 1;
    uint32_t lo = 0, hi = bt_be16(page + 1), child = bt_be32(page + 3);
    for (uint32_t step = 0; step < 17 && lo < hi; ++step) {  // hi < 2^16
        const uint32_t mid = (lo + hi) / 2;
        BtCell c;
        if (!bt_cell(page, leaf, v1, mid, &c)) return false;
        const int r = cmp(page + c.koff, c.klen);
        if (leaf && r == 0) {
            a->status = kBtFound, a->pos = mid, a->vloc = (uint64_t)id * kBtPage + c.voff, a->vlen = c.vlen;
            return false;
        }
        if (r < 0) hi = mid;
        else lo = mid + 1, child = c.child;
    }
    if (leaf) {
        a->status = kBtMiss, a->pos = lo;
        return false;
    }
    *next = child;
    return true;
}

// Get (btree/btree.go:232-280) for one non-empty key.  root_page: the root's 4096 bytes where the caller holds a
// copy (the kernel's LDS), else nullptr.  SEB_GET_ERROR with leaf = the page it arose at: an id outside
// [1, num_pages) (leaf = that id), a type that is neither 1 nor 2, a touched cell that does not parse, or an
// internal page as the kBtMaxDepth-th page of the walk (how a cycle ends).
template <class Cmp>
SEB_BT_HD void bt_walk(const uint8_t *image, uint32_t num_pages, uint32_t root, const uint8_t *root_page, const Cmp &cmp,
                       BtAnswer *a) {
    a->status = kBtError, a->leaf = root, a->pos = 0, a->vloc = 0, a->vlen = 0;
    uint32_t id = root, next = 0;
    if (!bt_page_id_ok(id, num_pages)) return;
    if (!bt_page_step(root_page ? root_page : image + (uint64_t)id * kBtPage, id, cmp, a, &next)) return;
    for (uint32_t depth = 1; depth < kBtMaxDepth; ++depth) {
        id = next;
        if (!bt_page_id_ok(id, num_pages)) {
            a->leaf = id;
            return;
        }
        if (!bt_page_step(image + (uint64_t)id * kBtPage, id, cmp, a, &next)) return;
    }
}

// ---- range scans: the leaf directory and what a scan computes from it.
//
// The directory of an image of num_pages pages is one flat buffer of bt_dir_bytes(num_pages) bytes, little-endian, whose
// array offsets depend on num_pages alone (every array has room for num_pages leaves):
//   [0, 32)            the header: u32 magic "BTDR", u32 num_pages, u32 root, u32 leaves L, u64 keys, u32 depth, u32 0
//   32                 leaf[num_pages] u32: the reachable leaves' page ids in key order, 0 from entry L on
//   bt_dir_first_at    first[num_pages + 1] u64: the exclusive prefix sum of the leaves' numCells, first[L] = keys, 0 behind
//   bt_dir_ord_at      ord[num_pages] u32: a page's position in leaf[], kBtNoPage for a page that is no listed leaf
// A refused image leaves a zeroed header, and nothing else in the buffer means anything.
constexpr uint32_t kBtDirMagic = 0x42544452u;
constexpr uint32_t kBtDirHeader = 32;

struct BtDirInfo {  // seb_bt_dir_info
    uint64_t leaves, keys;
    uint32_t depth, reserved;
};

SEB_BT_HD uint64_t bt_dir_first_at(uint32_t num_pages) { return (kBtDirHeader + 4ull * num_pages + 7) & ~7ull; }
SEB_BT_HD uint64_t bt_dir_ord_at(uint32_t num_pages) { return bt_dir_first_at(num_pages) + 8ull * num_pages + 8; }
SEB_BT_HD uint64_t bt_dir_bytes(uint32_t num_pages) { return (bt_dir_ord_at(num_pages) + 4ull * num_pages + 15) & ~15ull; }

struct BtDir {  // a directory's arrays; L and keys from its header, already held to L <= num_pages by who made this
    const uint32_t *leaf;
    const uint64_t *first;
    const uint32_t *ord;
    uint32_t num_pages, leaves;
    uint64_t keys;
};

SEB_BT_HD BtDir bt_dir_view(const uint8_t *dir, uint32_t num_pages, uint32_t leaves, uint64_t keys) {
    return BtDir{(const uint32_t *)(dir + kBtDirHeader), (const uint64_t *)(dir + bt_dir_first_at(num_pages)),
                 (const uint32_t *)(dir + bt_dir_ord_at(num_pages)), num_pages, leaves, keys};
}

// The global position of a seek's answer (leaf, pos): first[ord[leaf]] + pos.  False where the seek ended in ERROR, at a
// page the directory does not list, or past the leaf's cells.
SEB_BT_HD bool bt_dir_position(const BtDir &d, const BtAnswer &a, uint64_t *g) {
    if (a.status == kBtError || a.leaf >= d.num_pages) return false;
    const uint32_t o = d.ord[a.leaf];
    if (o >= d.leaves) return false;
    const uint64_t lo = d.first[o], hi = d.first[o + 1];
    if (hi < lo || a.pos > hi - lo) return false;
    *g = lo + a.pos;
    return true;
}

// One range's first position and count: start / end are the seeks' positions (0 and keys for an empty bound)
SEB_BT_HD uint64_t bt_range_count(uint64_t first, uint64_t last, uint64_t limit) {
    const uint64_t c = last > first ? last - first : 0;
    return limit && c > limit ? limit : c;
}

// the last index of the non-decreasing x[0, n] (n + 1 entries, x[0] <= v) with x[index] <= v, held below n: a counted
// bisection.  With x = first[] it is the leaf ordinal of global position v, with x = range_off[] the range of entry v.
SEB_BT_HD uint64_t bt_upper_index(const uint64_t *x, uint64_t n, uint64_t v) {
    uint64_t lo = 0, hi = n;  // the answer lies in [lo, hi)
    for (uint32_t step = 0; step < 64 && lo + 1 < hi; ++step) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (x[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct BtEntry {  // one output entry of a scan
    uint8_t status;
    uint64_t kloc, vloc;
    uint32_t klen, vlen;
};

// The cell at global position g: SEB_GET_FOUND with the key's and the value's place in the image, or SEB_GET_ERROR
// with zero lengths where the directory's arrays or the page no longer give a cell.
SEB_BT_HD BtEntry bt_scan_entry(const uint8_t *image, const BtDir &d, uint64_t g) {
    BtEntry e{kBtError, 0, 0, 0, 0};
    if (d.leaves == 0 || g >= d.keys) return e;
    const uint64_t o = bt_upper_index(d.first, d.leaves, g);
    const uint64_t lo = d.first[o];
    const uint32_t p = d.leaf[o];
    if (g < lo || g - lo > 0xFFFF || !bt_page_id_ok(p, d.num_pages)) return e;
    const uint8_t *page = image + (uint64_t)p * kBtPage;
    const uint32_t i = (uint32_t)(g - lo);
    BtCell c;
    if (page[0] != kBtLeaf || i >= bt_be16(page + 1) || !bt_cell(page, true, page[9] <= 1, i, &c)) return e;
    e.status = kBtFound;
    e.kloc = (uint64_t)p * kBtPage + c.koff, e.klen = c.klen;
    e.vloc = (uint64_t)p * kBtPage + c.voff, e.vlen = c.vlen;
    return e;
}

// The chain and order rules for listed leaf i (the directory's leaf[] and first[] already written): 0 good, 1 the
// chain (RightPtr(leaf[i]) is not leaf[i + 1], or not 0 on the last leaf), 2 the order (the last key of this non-empty
// leaf is not strictly below the first key of the next non-empty leaf, or one of the two does not parse).
SEB_BT_HD uint32_t bt_leaf_link(const uint8_t *image, const BtDir &d, uint32_t i) {
    const uint32_t p = d.leaf[i];
    if (!bt_page_id_ok(p, d.num_pages)) return 1;
    const uint8_t *page = image + (uint64_t)p * kBtPage;
    if (bt_be32(page + 3) != (i + 1 < d.leaves ? d.leaf[i + 1] : 0)) return 1;
    const uint64_t n = d.first[i + 1] - d.first[i];
    if (n == 0) return 0;
    uint32_t j = i + 1;
    for (; j < d.leaves && d.first[j + 1] == d.first[j]; ++j) {}
    if (j >= d.leaves) return 0;
    const uint32_t q = d.leaf[j];
    if (!bt_page_id_ok(q, d.num_pages)) return 2;
    const uint8_t *next = image + (uint64_t)q * kBtPage;
    BtCell a, b;
    if (n > 0xFFFF || !bt_cell(page, true, page[9] <= 1, (uint32_t)n - 1, &a) || !bt_cell(next, true, next[9] <= 1, 0, &b)) return 2;
    return bt_bytes_cmp(page + a.koff, a.klen, next + b.koff, b.klen) < 0 ? 0 : 2;
}

// ---- the host half (seb_btree.cpp, seb_btscan.cpp).  0; -1 a null argument; -2 fewer than 4096 bytes or a wrong magic (bt_open);
// -3 meta.num_pages pages do not fit the image; -4 out of memory
struct BtKeys {  // host memory, validated by the caller
    const uint8_t *data;
    const uint64_t *offsets;
    uint64_t n;
    uint32_t stride;
};
int bt_open(const uint8_t *image, uint64_t image_bytes, BtMeta *meta);
// kind / level: num_pages bytes each (nullable); stats nullable
int bt_check(const uint8_t *image, uint64_t image_bytes, const BtMeta &meta, uint8_t *kind, uint8_t *level, BtStats *stats);
int bt_get(const uint8_t *image, uint64_t image_bytes, const BtMeta &meta, const BtKeys &keys, uint8_t *status, uint32_t *leaf,
           uint32_t *pos, uint64_t *vloc, uint32_t *vlen);

// ---- seb_btscan.cpp.  The directory's refusals, in the order they are tested; each names a page.
enum : int {
    kDirRoot = 1,   // the root lies outside [1, num_pages)
    kDirBad,        // a listed page that the check calls bad (or whose id lies outside the image)
    kDirLevel,      // a page listed in round r whose level is not r
    kDirMixed,      // a round lists leaves and internal pages: leaves at two levels
    kDirDeep,       // internal pages in the last round the walk reaches
    kDirWide,       // a level whose children number more than num_pages
    kDirTwice,      // a leaf listed twice
    kDirChain,      // RightPtr(leaf[i]) != leaf[i + 1], or the last leaf's is not 0
    kDirOrder,      // the keys do not increase across a leaf boundary
};
const char *bt_dir_rule_text(int rule);
// -5: refused, *rule and *page say why; dir: bt_dir_bytes(num_pages) bytes, 8-byte aligned; kind / level: bt_check's
int bt_dir_build(const uint8_t *image, uint64_t image_bytes, const BtMeta &meta, const uint8_t *kind, const uint8_t *level,
                 uint8_t *dir, BtDirInfo *info, int *rule, uint32_t *page);
// the header of `dir` against meta: false where it is no directory of this image
bool bt_dir_header_ok(const uint8_t *hdr32, const BtMeta &meta, uint32_t *leaves, uint64_t *keys);

struct BtScanSizes {  // seb_bt_scan_sizes
    uint64_t ranges, entries, key_bytes, val_bytes;
};
struct BtScanOut {  // host memory; entry arrays of entry_cap elements, offsets of entry_cap + 1, all nullable with cap 0
    uint8_t *range_status;  // ranges
    uint64_t *range_off;    // ranges + 1
    uint8_t *status, *source;
    uint64_t *kloc, *vloc;
    uint32_t *klen, *vlen;
    uint64_t entry_cap;
    uint64_t *key_off, *val_off;
    uint8_t *keys, *vals;
    uint64_t key_cap, val_cap;
};
// -6: dir is no directory of this image; -7: a cap is below the need (*sizes filled for the retry; range_status and
// range_off are written all the same); -8: 2^32 entries or more
int bt_scan(const uint8_t *image, uint64_t image_bytes, const BtMeta &meta, const uint8_t *dir, const BtKeys &starts,
            const BtKeys &ends, uint64_t limit, const BtScanOut &out, BtScanSizes *sizes);

}  // namespace seb
