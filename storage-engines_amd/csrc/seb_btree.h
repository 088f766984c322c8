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

// ---- the host half (seb_btree.cpp).  0; -1 a null argument; -2 fewer than 4096 bytes or a wrong magic (bt_open);
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

}  // namespace seb
