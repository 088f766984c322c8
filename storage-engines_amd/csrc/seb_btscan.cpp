// seb_btscan.cpp — the host half of the B-tree's range scans (no HIP dependency): the leaf directory
// of a checked image and Scan for a batch of ranges.  The directory's layout, the position arithmetic, the cell
// locate and the chain / order rule are seb_btree.h's, the same text the kernels compile; this file adds the loops.
// It is the reference for the device forms and what a caller without a GPU uses.
#include "seb_btree.h"

#include <cstring>
#include <new>
#include <vector>

namespace seb {

const char *bt_dir_rule_text(int rule) {
    switch (rule) {
    case kDirRoot:
        return "the root lies outside the image";
    case kDirBad:
        return "a reachable page that the check calls bad";
    case kDirLevel:
        return "a page listed at a level that is not its own";
    case kDirMixed:
        return "leaves at two levels";
    case kDirDeep:
        return "an internal page at the depth limit";
    case kDirWide:
        return "a level with more children than the image has pages";
    case kDirTwice:
        return "a leaf listed twice";
    case kDirChain:
        return "the leaf chain does not follow the key order";
    case kDirOrder:
        return "the keys do not increase across a leaf boundary";
    default:
        return "refused";
    }
}

static void put32(uint8_t *p, uint32_t v) { memcpy(p, &v, 4); }
static void put64(uint8_t *p, uint64_t v) { memcpy(p, &v, 8); }

bool bt_dir_header_ok(const uint8_t *h, const BtMeta &meta, uint32_t *leaves, uint64_t *keys) {
    uint32_t w[4];
    memcpy(w, h, 16);
    memcpy(keys, h + 16, 8);
    *leaves = w[3];
    return w[0] == kBtDirMagic && w[1] == meta.num_pages && w[2] == meta.root && w[3] <= meta.num_pages;
}

int bt_dir_build(const uint8_t *image, uint64_t image_bytes, const BtMeta &meta, const uint8_t *kind, const uint8_t *level,
                 uint8_t *dir, BtDirInfo *info, int *rule, uint32_t *bad_page) {
    const uint32_t np = meta.num_pages;
    if (!dir || !info || !rule || !bad_page || (np && (!image || !kind || !level))) return -1;
    if ((uint64_t)np * kBtPage > image_bytes) return -3;
    *info = BtDirInfo{0, 0, 0, 0}, *rule = 0, *bad_page = 0;
    memset(dir, 0, bt_dir_bytes(np));
    auto refuse = [&](int r, uint32_t p) {
        *rule = r, *bad_page = p;
        memset(dir, 0, kBtDirHeader);
        return -5;
    };
    if (!bt_page_id_ok(meta.root, np)) return refuse(kDirRoot, meta.root);
    std::vector<uint32_t> list, next;
    uint32_t depth = 0;
    try {
        list.push_back(meta.root);
        for (uint32_t r = 0; r < kBtMaxDepth; ++r) {
            const uint8_t kind0 = bt_page_id_ok(list[0], np) ? kind[list[0]] : (uint8_t)kBtBad;
            for (uint32_t p : list) {
                if (!bt_page_id_ok(p, np) || kind[p] == kBtBad) return refuse(kDirBad, p);
                if (level[p] != r) return refuse(kDirLevel, p);
                if (kind[p] != kind0) return refuse(kDirMixed, p);
            }
            depth = r + 1;
            if (kind0 == kBtLeaf) break;
            if (r + 1 == kBtMaxDepth) return refuse(kDirDeep, list[0]);
            uint64_t total = 0;
            for (uint32_t p : list) total += bt_be16(image + (uint64_t)p * kBtPage + 1) + 1u;
            if (total > np) return refuse(kDirWide, list[0]);
            next.clear();
            for (uint32_t p : list) {
                const uint8_t *page = image + (uint64_t)p * kBtPage;
                const uint32_t n = bt_be16(page + 1);
                next.push_back(bt_be32(page + 3));  // the right pointer: the LEFTMOST child
                for (uint32_t i = 0; i < n; ++i) {
                    BtCell c;
                    next.push_back(bt_cell(page, false, page[9] <= 1, i, &c) ? c.child : kBtNoPage);
                }
            }
            list.swap(next);
        }
    } catch (const std::bad_alloc &) {
        return -4;
    }
    const uint32_t L = (uint32_t)list.size();
    uint32_t *leaf = (uint32_t *)(dir + kBtDirHeader), *ord = (uint32_t *)(dir + bt_dir_ord_at(np));
    uint64_t *first = (uint64_t *)(dir + bt_dir_first_at(np));
    memset(ord, 0xFF, 4ull * np);
    uint64_t keys = 0;
    uint32_t twice = kBtNoPage;
    for (uint32_t i = 0; i < L; ++i) {
        const uint32_t p = list[i];
        leaf[i] = p, first[i] = keys;
        keys += bt_be16(image + (uint64_t)p * kBtPage + 1);
        if (ord[p] != kBtNoPage && p < twice) twice = p;
        ord[p] = i;
    }
    first[L] = keys;
    if (twice != kBtNoPage) return refuse(kDirTwice, twice);
    const BtDir d = bt_dir_view(dir, np, L, keys);
    for (uint32_t want = 1; want <= 2; ++want)  // every chain fault comes before any order fault
        for (uint32_t i = 0; i < L; ++i)
            if (bt_leaf_link(image, d, i) == want) return refuse(want == 1 ? kDirChain : kDirOrder, list[i]);
    put32(dir, kBtDirMagic), put32(dir + 4, np), put32(dir + 8, meta.root), put32(dir + 12, L);
    put64(dir + 16, keys), put32(dir + 24, depth), put32(dir + 28, 0);
    *info = BtDirInfo{L, keys, depth, 0};
    return 0;
}

namespace {
struct HostCmp {
    const uint8_t *key;
    uint32_t klen;
    int operator()(const uint8_t *stored, uint32_t slen) const { return bt_bytes_cmp(key, klen, stored, slen); }
};

// the global position a bound seeks to: `empty` for an empty bound; false where the seek fails
bool seek(const uint8_t *image, const BtMeta &meta, const BtDir &d, const BtKeys &k, uint64_t i, uint64_t empty, uint64_t *g) {
    uint64_t beg = i * k.stride, len = k.stride;
    if (k.offsets) beg = k.offsets[i], len = k.offsets[i + 1] > beg ? k.offsets[i + 1] - beg : 0;
    if (!len) {
        *g = empty;
        return true;
    }
    BtAnswer a;
    bt_walk(image, meta.num_pages, meta.root, nullptr, HostCmp{k.data + beg, (uint32_t)(len < kBtMaxKey ? len : kBtMaxKey)}, &a);
    return bt_dir_position(d, a, g);
}
}  // namespace

int bt_scan(const uint8_t *image, uint64_t image_bytes, const BtMeta &meta, const uint8_t *dir, const BtKeys &starts,
            const BtKeys &ends, uint64_t limit, const BtScanOut &out, BtScanSizes *sizes) {
    const uint64_t R = starts.n;
    if (!sizes || !dir || ends.n != R || (meta.num_pages && !image) || !out.range_off || (R && !out.range_status)) return -1;
    if ((uint64_t)meta.num_pages * kBtPage > image_bytes) return -3;
    *sizes = BtScanSizes{R, 0, 0, 0};
    uint32_t L;
    uint64_t keys;
    if (!bt_dir_header_ok(dir, meta, &L, &keys)) return -6;
    const BtDir d = bt_dir_view(dir, meta.num_pages, L, keys);
    std::vector<uint64_t> first_r;
    try {
        first_r.assign(R, 0);
    } catch (const std::bad_alloc &) {
        return -4;
    }
    uint64_t entries = 0;
    for (uint64_t r = 0; r < R; ++r) {
        uint64_t a = 0, b = 0;
        const bool ok = seek(image, meta, d, starts, r, 0, &a) && seek(image, meta, d, ends, r, keys, &b);
        out.range_status[r] = ok ? 0 : kBtError;
        out.range_off[r] = entries, first_r[r] = a;
        entries += ok ? bt_range_count(a, b, limit) : 0;
    }
    out.range_off[R] = entries;
    sizes->entries = entries;
    if (entries >> 32) return -8;
    // the sizes first: a cap below the need leaves the entry arrays untouched
    for (uint64_t r = 0; r < R; ++r)
        for (uint64_t e = out.range_off[r]; e < out.range_off[r + 1]; ++e) {
            const BtEntry c = bt_scan_entry(image, d, first_r[r] + (e - out.range_off[r]));
            sizes->key_bytes += c.klen, sizes->val_bytes += c.vlen;
        }
    if (entries > out.entry_cap || sizes->key_bytes > out.key_cap || sizes->val_bytes > out.val_cap) return -7;
    if ((entries && (!out.key_off || !out.val_off || !out.status || !out.source || !out.kloc || !out.klen || !out.vloc || !out.vlen)) ||
        (sizes->key_bytes && !out.keys) || (sizes->val_bytes && !out.vals))
        return -1;
    uint64_t kb = 0, vb = 0;
    for (uint64_t r = 0; r < R; ++r)
        for (uint64_t e = out.range_off[r]; e < out.range_off[r + 1]; ++e) {
            const BtEntry c = bt_scan_entry(image, d, first_r[r] + (e - out.range_off[r]));
            out.status[e] = c.status, out.source[e] = 1;
            out.kloc[e] = c.kloc, out.klen[e] = c.klen, out.vloc[e] = c.vloc, out.vlen[e] = c.vlen;
            out.key_off[e] = kb, out.val_off[e] = vb;
            if (c.klen) memcpy(out.keys + kb, image + c.kloc, c.klen);
            if (c.vlen) memcpy(out.vals + vb, image + c.vloc, c.vlen);
            kb += c.klen, vb += c.vlen;
        }
    if (out.key_off) out.key_off[entries] = kb;
    if (out.val_off) out.val_off[entries] = vb;
    return 0;
}

}  // namespace seb
