// seb_hashwrite.cpp — the host half of the hash index's write side.  No HIP dependency, so it
// compiles alone (tools/sanitize/hashwrite_check.cpp, with seb_hashindex.cpp, seb_memwrite.cpp and seb_memtable.cpp);
// the C ABI wrappers that set seb_last_error are in seb_hidx.cpp.
//
//   frame    HashIndex.Put / Delete -> segment.append (hashindex/segment.go:61-125): [crc u32][timestamp u64][keySize
//            u32][valueSize u32][key][value], crc = ChecksumIEEE(record[4:]); Delete is Put(key, nil).  Put refuses an
//            empty key (hashindex.go:92-95).  One timestamp per call.
//   cuts     a record goes to the active segment iff its size is below the limit BEFORE the append; otherwise the
//            engine rotates once and appends to the new, empty segment (hashindex.go:92-215).
//   compact  compactSegments (hashindex/compaction.go:12-76) for the records of the chosen segments: the last record
//            of a key wins among these records only, a winner with an empty value is dropped, every other winner is
//            written with a fresh timestamp.  The reference writes them in a Go map's order; log order (the survivors
//            in ascending position) is one of the orders it can produce and the one fixed here.
//   logical  getLogicalSize (hashindex.go:360-385): keySize + valueSize over the index entries.
#include "seb_hashwrite.h"

#include <cstring>
#include <new>
#include <string_view>
#include <unordered_map>

#include "seb_memwrite.h"

namespace seb {

namespace {

inline void put32(uint8_t *p, uint32_t v) { memcpy(p, &v, 4); }
inline void put64(uint8_t *p, uint64_t v) { memcpy(p, &v, 8); }

// op i's key and value lengths from the offsets alone
inline int op_lens(const KeysView &kb, const uint64_t *val_off, uint64_t i, uint64_t *klen, uint64_t *vlen) {
    if (kb.offsets) {
        const uint64_t a = kb.offsets[i], b = kb.offsets[i + 1];
        if (b < a || b - a >= (1ull << 32)) return -2;
        *klen = b - a;
    } else {
        *klen = kb.stride;
    }
    const uint64_t a = val_off[i], b = val_off[i + 1];
    if (b < a || b - a >= (1ull << 32)) return -3;
    *vlen = b - a;
    return *klen == 0 ? -6 : 0;
}

using Index = std::unordered_map<std::string_view, uint64_t>;  // key -> its latest record's offset

// the index over the live records; -4 with *bad where one does not lie inside the pool and strict is set
int build_index(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, const uint8_t *live, uint64_t n,
                bool strict, Index &index, uint64_t *live_in, uint64_t *bad) {
    for (uint64_t r = 0; r < n; ++r) {
        if (live && !live[r]) continue;
        if (live_in) ++*live_in;
        uint32_t ks, vs;
        if (!seg_record(pool, pool_bytes, rec_off[r], &ks, &vs)) {
            if (!strict) continue;
            if (bad) *bad = r;
            return -4;
        }
        const std::string_view key(ks ? (const char *)pool + rec_off[r] + kSegHeader : "", ks);
        auto it = index.try_emplace(key, rec_off[r]).first;
        if (it->second < rec_off[r]) it->second = rec_off[r];
    }
    return 0;
}

}  // namespace

int seg_frame_plan(const KeysView &kb, const uint64_t *val_off, const uint8_t *deleted, uint64_t active_size,
                   uint64_t limit, uint64_t *rec_off, uint64_t *cut, uint64_t cut_cap, uint64_t *image_bytes,
                   uint64_t *ncuts, uint64_t *bad_op) {
    if (kb.n >= (1ull << 32)) return -4;
    if (kb.n && !val_off) return -1;
    if (limit == 0) return -9;
    uint64_t cuts = 0;
    {  // every op, before anything is written or a key or value byte is read; the sum rule reads deleted[i]: a
       // Delete's value is nil whatever bytes the op carries
        uint64_t size = active_size;
        for (uint64_t i = 0; i < kb.n; ++i) {
            uint64_t klen, vlen;
            int rc = op_lens(kb, val_off, i, &klen, &vlen);
            if (!rc && klen + (deleted && deleted[i] ? 0 : vlen) >= (1ull << 32)) rc = -7;
            if (rc) {
                if (bad_op) *bad_op = i;
                return rc;
            }
            if (deleted && deleted[i]) vlen = 0;
            if (size >= limit) ++cuts, size = 0;
            size += kSegHeader + klen + vlen;
        }
    }
    if (ncuts) *ncuts = cuts;
    if (cut && cuts > cut_cap) return -8;
    uint64_t at = 0, size = active_size, c = 0;
    if (rec_off) rec_off[0] = 0;
    for (uint64_t i = 0; i < kb.n; ++i) {
        uint64_t klen, vlen;
        op_lens(kb, val_off, i, &klen, &vlen);
        if (deleted && deleted[i]) vlen = 0;
        if (size >= limit) {
            if (cut) cut[c] = i;
            ++c, size = 0;
        }
        size += kSegHeader + klen + vlen;
        at += kSegHeader + klen + vlen;
        if (rec_off) rec_off[i + 1] = at;
    }
    if (image_bytes) *image_bytes = at;
    return 0;
}

int seg_frame_emit(const KeysView &kb, const uint8_t *vals, const uint64_t *val_off, const uint8_t *deleted,
                   uint64_t timestamp, uint8_t *image, uint64_t image_bytes, uint64_t *bad_op) {
    uint64_t total = 0;
    const int rc = seg_frame_plan(kb, val_off, deleted, 0, 1, nullptr, nullptr, 0, &total, nullptr, bad_op);
    if (rc) return rc;
    if (total != image_bytes) return -5;
    if (kb.n && (!image || !kb.data)) return -1;
    uint8_t *p = image;
    for (uint64_t i = 0; i < kb.n; ++i) {
        const uint64_t ko = kb.offsets ? kb.offsets[i] : i * (uint64_t)kb.stride;
        const uint32_t klen = kb.offsets ? (uint32_t)(kb.offsets[i + 1] - ko) : kb.stride;
        const uint32_t vlen = deleted && deleted[i] ? 0 : (uint32_t)(val_off[i + 1] - val_off[i]);
        if (vlen && !vals) return -1;
        put64(p + 4, timestamp);
        put32(p + 12, klen);
        put32(p + 16, vlen);
        memcpy(p + kSegHeader, kb.data + ko, klen);
        if (vlen) memcpy(p + kSegHeader + klen, vals + val_off[i], vlen);
        const uint64_t len = (uint64_t)kSegHeader + klen + vlen;
        put32(p, crc32_ieee(p + 4, len - 4));
        p += len;
    }
    return 0;
}

int seg_compact(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, const uint8_t *live, uint64_t n,
                uint64_t timestamp, uint8_t *image, uint64_t image_cap, uint64_t *out_rec_off, uint64_t rec_cap,
                SegCompactSizes *sizes, uint64_t *bad) {
    if (!sizes || (pool_bytes && !pool) || (n && !rec_off)) return -1;
    *sizes = SegCompactSizes{n, 0, 0, 0, 0, 0, 0, 0};
    if (pool_bytes >= kHidxPoolLimit) return -2;
    SegCompactSizes s{n, 0, 0, 0, 0, 0, 0, 0};
    try {
        Index index;
        const int rc = build_index(pool, pool_bytes, rec_off, live, n, true, index, &s.live_in, bad);
        if (rc) return rc;
        s.distinct = index.size();
        s.shadowed = s.live_in - s.distinct;
        const auto wins = [&](uint64_t r, uint32_t *ks, uint32_t *vs) {
            if (live && !live[r]) return false;
            seg_record(pool, pool_bytes, rec_off[r], ks, vs);  // it passed in build_index
            const std::string_view key(*ks ? (const char *)pool + rec_off[r] + kSegHeader : "", *ks);
            return index.find(key)->second == rec_off[r];
        };
        for (uint64_t r = 0; r < n; ++r) {
            uint32_t ks, vs;
            if (!wins(r, &ks, &vs)) continue;
            if (vs == 0)
                ++s.tombstoned;
            else
                ++s.survivors, s.image_bytes += (uint64_t)kSegHeader + ks + vs;
        }
        *sizes = s;
        if (!image && !out_rec_off) return 0;
        if (image_cap < s.image_bytes || rec_cap < s.survivors + 1) return -5;
        if (!out_rec_off || (s.image_bytes && !image)) return -1;
        uint64_t at = 0, k = 0;
        for (uint64_t r = 0; r < n; ++r) {
            uint32_t ks, vs;
            if (!wins(r, &ks, &vs) || vs == 0) continue;
            const uint64_t len = (uint64_t)kSegHeader + ks + vs;
            uint8_t *p = image + at;
            put64(p + 4, timestamp);
            memcpy(p + 12, pool + rec_off[r] + 12, len - 12);
            put32(p, crc32_ieee(p + 4, len - 4));
            out_rec_off[k++] = at;
            at += len;
        }
        out_rec_off[k] = at;
    } catch (const std::bad_alloc &) {
        return -3;
    }
    return 0;
}

int hidx_logical_size(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, const uint8_t *live, uint64_t n,
                      uint64_t *logical) {
    if (!logical || (pool_bytes && !pool) || (n && !rec_off)) return -1;
    *logical = 0;
    if (pool_bytes >= kHidxPoolLimit) return -2;
    try {
        Index index;
        build_index(pool, pool_bytes, rec_off, live, n, false, index, nullptr, nullptr);
        uint64_t sum = 0;
        for (const auto &kv : index) {
            uint32_t ks, vs;
            seg_record(pool, pool_bytes, kv.second, &ks, &vs);
            sum += (uint64_t)ks + vs;
        }
        *logical = sum;
    } catch (const std::bad_alloc &) {
        return -3;
    }
    return 0;
}

}  // namespace seb
