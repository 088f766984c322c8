// seb_btree.cpp — the host half of the B-tree's read side (no HIP dependency): readMetadata, the
// structural check of a page-file image and Get for a key batch.  The page rules and the walk are seb_btree.h's, the
// same text the kernels compile; this file adds the loops over pages and keys, the levels and the counts.  It is the
// reference for the device forms and what a caller without a GPU uses.
#include "seb_btree.h"

#include <cstring>
#include <new>
#include <vector>

namespace seb {

int bt_open(const uint8_t *image, uint64_t image_bytes, BtMeta *meta) {
    if (!meta || (image_bytes && !image)) return -1;
    *meta = BtMeta{0, 0, 0, 0};
    if (image_bytes < kBtPage || bt_be32(image) != kBtMagic) return -2;
    meta->root = bt_be32(image + 4), meta->header_pages = bt_be32(image + 8), meta->free_list = bt_be32(image + 12);
    const uint64_t held = image_bytes / kBtPage;
    meta->num_pages = meta->header_pages < held ? meta->header_pages : (uint32_t)held;
    return 0;
}

static uint8_t page_kind(const uint8_t *page, uint32_t num_pages, uint32_t *cells) {
    const uint8_t kind = bt_page_head(page, num_pages, cells);
    if (kind == kBtBad) return kBtBad;
    const bool leaf = kind == kBtLeaf, v1 = page[9] <= 1;
    for (uint32_t i = 0; i < *cells; ++i)
        if (!bt_cell_good(page, leaf, v1, *cells, i, num_pages)) return kBtBad;
    return kind;
}

int bt_check(const uint8_t *image, uint64_t image_bytes, const BtMeta &meta, uint8_t *kind, uint8_t *level, BtStats *stats) {
    const uint32_t np = meta.num_pages;
    if (np && !image) return -1;
    if ((uint64_t)np * kBtPage > image_bytes) return -3;
    std::vector<uint8_t> k, lv;
    std::vector<uint32_t> cells, front, next;
    try {
        k.assign(np, kBtBad), lv.assign(np, (uint8_t)kBtNoLevel), cells.assign(np, 0);
        for (uint32_t p = 1; p < np; ++p) k[p] = page_kind(image + (uint64_t)p * kBtPage, np, &cells[p]);
        // the levels: rounds from the root; only a good internal page hands a level on
        if (bt_page_id_ok(meta.root, np)) lv[meta.root] = 0, front.push_back(meta.root);
        for (uint32_t r = 0; r + 1 < kBtMaxDepth && !front.empty(); ++r) {
            next.clear();
            for (uint32_t p : front) {
                if (k[p] != kBtInternal) continue;
                const uint8_t *page = image + (uint64_t)p * kBtPage;
                const bool v1 = page[9] <= 1;
                auto reach = [&](uint32_t c) {
                    if (bt_page_id_ok(c, np) && lv[c] == kBtNoLevel) lv[c] = (uint8_t)(r + 1), next.push_back(c);
                };
                reach(bt_be32(page + 3));
                for (uint32_t i = 0; i < cells[p]; ++i) {
                    BtCell c;
                    if (bt_cell(page, false, v1, i, &c)) reach(c.child);
                }
            }
            front.swap(next);
        }
    } catch (const std::bad_alloc &) {
        return -4;
    }
    if (kind && np) memcpy(kind, k.data(), np);
    if (level && np) memcpy(level, lv.data(), np);
    if (stats) {
        BtStats s{};
        uint32_t top = 0, leaf_lo = kBtNoLevel, leaf_hi = 0;
        bool any = false;
        for (uint32_t p = 1; p < np; ++p) {
            const bool reached = lv[p] != kBtNoLevel;
            ++(k[p] == kBtLeaf ? s.leaves : k[p] == kBtInternal ? s.internals : s.bad);
            if (!reached) continue;
            ++(k[p] == kBtLeaf ? s.reach_leaves : k[p] == kBtInternal ? s.reach_internals : s.reach_bad);
            any = true;
            if (lv[p] > top) top = lv[p];
            if (k[p] == kBtLeaf) {
                s.keys += cells[p];
                if (lv[p] < leaf_lo) leaf_lo = lv[p];
                if (lv[p] > leaf_hi) leaf_hi = lv[p];
            }
        }
        s.depth = any ? top + 1 : 0;
        s.uniform = s.reach_leaves == 0 || leaf_lo == leaf_hi;
        *stats = s;
    }
    return 0;
}

namespace {
struct HostCmp {
    const uint8_t *key;
    uint32_t klen;
    int operator()(const uint8_t *stored, uint32_t slen) const { return bt_bytes_cmp(key, klen, stored, slen); }
};
}  // namespace

int bt_get(const uint8_t *image, uint64_t image_bytes, const BtMeta &meta, const BtKeys &keys, uint8_t *status, uint32_t *leaf,
           uint32_t *pos, uint64_t *vloc, uint32_t *vlen) {
    if (keys.n && !status) return -1;
    if (meta.num_pages && !image) return -1;
    if ((uint64_t)meta.num_pages * kBtPage > image_bytes) return -3;
    for (uint64_t i = 0; i < keys.n; ++i) {
        uint64_t beg = i * keys.stride, len = keys.stride;
        if (keys.offsets) beg = keys.offsets[i], len = keys.offsets[i + 1] > beg ? keys.offsets[i + 1] - beg : 0;
        BtAnswer a{kBtError, kBtNoPage, 0, 0, 0};  // an empty key: ErrKeyEmpty
        if (len) bt_walk(image, meta.num_pages, meta.root, nullptr, HostCmp{keys.data + beg, (uint32_t)(len < kBtMaxKey ? len : kBtMaxKey)}, &a);
        status[i] = a.status;
        if (leaf) leaf[i] = a.leaf;
        if (pos) pos[i] = a.pos;
        if (vloc) vloc[i] = a.vloc;
        if (vlen) vlen[i] = a.vlen;
    }
    return 0;
}

}  // namespace seb
