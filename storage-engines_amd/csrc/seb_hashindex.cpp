// seb_hashindex.cpp — the host half of the hash index's read side: what hashindex/recovery.go's
// recover() and hashindex/hashindex.go's Get do for a set of segment images held back to back, oldest first, in
// one byte pool.  A record is [crc u32][timestamp u64][keySize u32][valueSize u32][key][value], little-endian, crc =
// ChecksumIEEE(record[4:]) (hashindex/segment.go:14-18, 61-125); a record is named by its pool offset, and the
// later record of a key is the one at the greater offset.  No HIP dependency, so it compiles alone
// (tools/sanitize/hashindex_check.cpp, with seb_memwrite.cpp for crc32_ieee); the C ABI wrappers that set
// seb_last_error are in seb_hidx.cpp.
#include "seb_hashindex.h"

#include <new>
#include <string_view>
#include <unordered_map>

#include "seb_memwrite.h"

namespace seb {

namespace {

inline uint32_t le32(const uint8_t *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

inline bool record_crc_ok(const uint8_t *pool, uint64_t off, uint32_t ks, uint32_t vs) {
    return crc32_ieee(pool + off + 4, (uint64_t)kSegHeader - 4 + ks + vs) == le32(pool + off);
}

}  // namespace

int seg_scan(const uint8_t *data, uint64_t bytes, uint64_t base, uint64_t *rec_off, uint64_t cap, uint64_t *n,
             int *short_tail) {
    if (!n || !short_tail || (bytes && !data)) return -1;
    *n = 0, *short_tail = 0;
    uint64_t at = 0;
    while (at < bytes) {
        if (bytes - at < kSegHeader) {  // ReadAt of the header: io.EOF, recover breaks (recovery.go:88-92)
            *short_tail = 1;
            break;
        }
        const uint64_t payload = (uint64_t)le32(data + at + 12) + le32(data + at + 16);
        const bool wraps = payload >= (1ull << 32);
        if (!wraps && payload > bytes - at - kSegHeader) {  // ReadAt of key + value: io.EOF
            *short_tail = 1;
            break;
        }
        if (*n == cap || !rec_off) return *n = cap, -2;
        rec_off[(*n)++] = base + at;
        if (wraps) break;  // the stated departure: this record fails, the segment is cut here
        at += kSegHeader + payload;
    }
    return 0;
}

bool seg_record(const uint8_t *pool, uint64_t pool_bytes, uint64_t off, uint32_t *ks, uint32_t *vs) {
    if (off > pool_bytes || pool_bytes - off < kSegHeader) return false;
    *ks = le32(pool + off + 12), *vs = le32(pool + off + 16);
    const uint64_t payload = (uint64_t)*ks + *vs;
    return payload < (1ull << 32) && payload <= pool_bytes - off - kSegHeader;
}

int seg_verify(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, uint64_t num_records,
               const uint64_t *seg_first, const uint64_t *seg_base, const uint64_t *seg_bytes, uint64_t num_segments,
               uint8_t *ok, uint64_t *valid, uint64_t *size_after, uint8_t *live) {
    if ((pool_bytes && !pool) || (num_records && !rec_off) || !seg_first) return -1;
    if (num_segments && (!seg_base || !seg_bytes || !valid || !size_after)) return -1;
    if (pool_bytes >= kHidxPoolLimit) return -2;
    if (seg_first[0] != 0 || seg_first[num_segments] != num_records) return -3;
    for (uint64_t s = 0; s < num_segments; ++s)
        if (seg_first[s + 1] < seg_first[s] || seg_first[s + 1] > num_records) return -3;
    for (uint64_t s = 0; s < num_segments; ++s) {
        bool cut = false;
        valid[s] = seg_first[s + 1] - seg_first[s];
        size_after[s] = seg_bytes[s];
        for (uint64_t r = seg_first[s]; r < seg_first[s + 1]; ++r) {
            uint32_t ks, vs;
            const bool good = seg_record(pool, pool_bytes, rec_off[r], &ks, &vs) && record_crc_ok(pool, rec_off[r], ks, vs);
            if (ok) ok[r] = good;
            if (!good && !cut) {  // Truncate(offset), size = offset (recovery.go:93-99)
                cut = true;
                valid[s] = r - seg_first[s];
                size_after[s] = rec_off[r] - seg_base[s];
            }
            if (live) live[r] = !cut;
        }
    }
    return 0;
}

int hidx_lookup(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, const uint8_t *live,
                uint64_t num_records, const KeysView &keys, int verify, uint8_t *status, uint64_t *rec, uint64_t *vloc,
                uint32_t *vlen, uint64_t *distinct) {
    if ((pool_bytes && !pool) || (num_records && !rec_off)) return -1;
    if (keys.n && (!status || (!keys.offsets && keys.stride && !keys.data))) return -1;
    if (pool_bytes >= kHidxPoolLimit) return -2;
    try {
        std::unordered_map<std::string_view, uint64_t> index;  // key -> its latest record's offset
        for (uint64_t r = 0; r < num_records; ++r) {
            uint32_t ks, vs;
            if ((live && !live[r]) || !seg_record(pool, pool_bytes, rec_off[r], &ks, &vs)) continue;
            const std::string_view key(ks ? (const char *)pool + rec_off[r] + kSegHeader : "", ks);
            auto it = index.try_emplace(key, rec_off[r]).first;
            if (it->second < rec_off[r]) it->second = rec_off[r];
        }
        if (distinct) *distinct = index.size();
        for (uint64_t i = 0; i < keys.n; ++i) {
            const uint64_t b = keys.offsets ? keys.offsets[i] : i * keys.stride;
            const uint64_t len = keys.offsets ? keys.offsets[i + 1] - b : keys.stride;
            const auto it = index.find(std::string_view(len ? (const char *)keys.data + b : "", len));
            uint8_t st = 0;  // SEB_GET_MISS
            uint64_t at = kHidxNoRec, loc = 0;
            uint32_t vl = 0;
            if (it != index.end()) {
                uint32_t ks, vs;
                seg_record(pool, pool_bytes, it->second, &ks, &vs);  // it passed when it was inserted
                // segment.read: the CRC first, then the value; an empty value is ErrKeyNotFound
                if (verify && !record_crc_ok(pool, it->second, ks, vs))
                    st = 2;  // SEB_GET_ERROR
                else if (vs)
                    st = 1, at = it->second, loc = it->second + kSegHeader + ks, vl = vs;
            }
            status[i] = st;
            if (rec) rec[i] = at;
            if (vloc) vloc[i] = loc;
            if (vlen) vlen[i] = vl;
        }
    } catch (const std::bad_alloc &) {
        return -3;
    }
    return 0;
}

}  // namespace seb
