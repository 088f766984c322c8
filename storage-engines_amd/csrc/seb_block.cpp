// seb_block.cpp — the host side of the batched data-block search: searchBlock's walk
// (lsm/sstable.go:242-290) for one block image and one key, and the read-list builder; and the host
// half of the batched SSTable builder and of the batched compaction merge (below).  No HIP dependency, so it compiles alone
// (tools/sanitize/block_check.cpp, sst_check.cpp, merge_check.cpp); the C ABI wrappers that set seb_last_error are in
// seb_sstable.cpp.
//
//   numEntries := u32(block[0:4]); off := 4                              sstable.go:243-248
//   for i := 0; i < numEntries; i++ {
//       if off+9 > len(block) { return error "block truncated" }         :251-253
//       keySize, valueSize, deleted := u32, u32, block[off+8] == 1; off += 9
//       if off+keySize+valueSize > len(block) { return error }           :261-263 (Go int: 64 bits)
//       if entryKey == key { deleted ? (nil, false) : (value, true) }    :268-281
//       if entryKey > key { return not found }                           :284-286
//       off += keySize + valueSize
//   }
//   return not found
#include <cstdint>
#include <cstring>
#include <new>
#include <algorithm>
#include <unordered_map>
#include <vector>

#include "seb_block.h"

namespace seb {

constexpr uint64_t kBlockBytes = 4096;
enum : uint32_t { kCellNone = 0, kCellMiss = 1, kCellFound = 2, kCellTombstone = 3, kCellTrunc = 4 };
static inline uint32_t cell_pack(uint32_t status, uint32_t voff, uint32_t vlen) {
    return status << 28 | voff << 13 | vlen;
}

static inline uint32_t le32(const uint8_t *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// 0, or -1 for a bad argument (len > 4096, a null pointer with a non-zero length, null cell).
int block_search(const uint8_t *block, uint64_t len, const uint8_t *key, uint64_t key_len, uint32_t *cell) {
    if (!cell || len > kBlockBytes || (len && !block) || (key_len && !key)) return -1;
    *cell = cell_pack(kCellMiss, 0, 0);
    if (len < 4) return 0;
    const uint32_t num = le32(block);
    uint64_t off = 4;
    for (uint32_t i = 0; i < num; ++i) {
        if (off + 9 > len) {
            *cell = cell_pack(kCellTrunc, 0, 0);
            return 0;
        }
        const uint64_t ks = le32(block + off), vs = le32(block + off + 4);
        const bool deleted = block[off + 8] == 1;
        off += 9;
        if (off + ks + vs > len) {  // 64-bit sums: 0xFFFFFFF0 + 0x20 does not wrap
            *cell = cell_pack(kCellTrunc, 0, 0);
            return 0;
        }
        const uint64_t common = ks < key_len ? ks : key_len;
        int c = common ? memcmp(block + off, key, common) : 0;
        if (c == 0) c = ks < key_len ? -1 : ks > key_len ? 1 : 0;  // a proper prefix sorts first
        if (c == 0) {
            *cell = deleted ? cell_pack(kCellTombstone, 0, 0) : cell_pack(kCellFound, (uint32_t)(off + ks), (uint32_t)vs);
            return 0;
        }
        if (c > 0) return 0;  // entryKey > key: not found
        off += ks + vs;
    }
    return 0;
}

struct PairHash {
    size_t operator()(const std::pair<uint64_t, uint64_t> &p) const {
        uint64_t h = p.first * 0x9E3779B97F4A7C15ull ^ (p.second + 0x7F4A7C15ull + (p.first << 6));
        h ^= h >> 29;
        return (size_t)(h * 0xBF58476D1CE4E5B9ull);
    }
};

// 0; -1 bad argument; -2 uniq_cap too small (*num_uniq = the count needed); -3 out of memory;
// -4 more than 2^32 - 1 distinct blocks (ids are u32).
int blocks_dedup(const uint64_t *files, const uint64_t *blocks, uint64_t cells, uint32_t *bid, uint64_t *uniq_files,
                 uint64_t *uniq_blocks, uint64_t uniq_cap, uint64_t *num_uniq) {
    if (!num_uniq || (cells && (!files || !blocks || !bid)) || (uniq_cap && (!uniq_files || !uniq_blocks))) return -1;
    *num_uniq = 0;
    try {
        std::unordered_map<std::pair<uint64_t, uint64_t>, uint32_t, PairHash> ids;
        uint64_t count = 0;
        for (uint64_t c = 0; c < cells; ++c) {
            if (blocks[c] == UINT64_MAX) {  // SEB_NO_BLOCK
                bid[c] = UINT32_MAX;
                continue;
            }
            auto it = ids.find({files[c], blocks[c]});
            if (it != ids.end()) {
                bid[c] = it->second;
                continue;
            }
            if (count >= UINT32_MAX) return -4;
            ids.emplace(std::make_pair(files[c], blocks[c]), (uint32_t)count);
            if (count < uniq_cap) {
                uniq_files[count] = files[c];
                uniq_blocks[count] = blocks[c];
            }
            bid[c] = (uint32_t)count++;
        }
        *num_uniq = count;
        return count > uniq_cap ? -2 : 0;
    } catch (const std::bad_alloc &) {
        return -3;
    }
}

// ------------------------------------------------------------------------------------------------
// The host half of the batched SSTable builder: SSTableBuilder.Add / flushBlock / Finish /
// encodeIndex / encodeMetadata (lsm/sstable_builder.go:42-135,185-290) for one sorted run in memory.
//
//   Add:   entry = [keySize u32][valueSize u32][deleted u8][key][value]              :55-74
//          if len(cur)+len(entry) > 4096 { flushBlock() }   (a no-op while len(cur) <= 4)  :77-82,92
//          cur = append(cur, entry...)
//   flush: cur[0:4] = numEntries; write cur; index += (first key, blockOffset);       :104-120
//          blockOffset += len(cur); a block shorter than 4096 is zero padded to it     :123-130
// One walk serves both entry points: out == nullptr only sizes.

static inline void put32(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24);
}
static inline void put64(uint8_t *p, uint64_t v) {
    put32(p, (uint32_t)v);
    put32(p + 4, (uint32_t)(v >> 32));
}

// 0; -1 a null argument; -2 a key or value of 2^32 bytes or more, or decreasing offsets; -3 a capacity
// below its section (sizes are still filled).
int sst_walk(const SstKeys &k, const uint8_t *vals, const uint64_t *voff, const uint8_t *deleted, const SstOut *out,
             SstSizes *sz) {
    if (!sz || (k.n && !voff)) return -1;
    SstSizes s{0, 0, 4, 8, 0};
    const uint64_t n = k.n;
    for (uint64_t i = 0; i < n; ++i) {
        if (k.off(i + 1) < k.off(i) || voff[i + 1] < voff[i]) return -2;
        if (k.off(i + 1) - k.off(i) > UINT32_MAX || voff[i + 1] - voff[i] > UINT32_MAX) return -2;
    }
    if (n && !k.data && k.off(n) != k.off(0)) return -1;
    // pass 1: the cut alone (sizes), pass 2: the bytes; the same loop with and without stores
    for (int pass = 0; pass < (out ? 2 : 1); ++pass) {
        const bool wr = pass == 1;
        if (wr && (s.data_bytes > out->data_cap || s.index_bytes > out->index_cap || s.meta_bytes > out->meta_cap)) {
            *sz = s;
            return -3;
        }
        if (wr && ((s.data_bytes && (!out->data || (!vals && voff[n] != voff[0]))) || !out->index || !out->meta)) return -1;
        uint64_t at = 0, iat = 4, blocks = 0, oversize = 0;  // data offset, index offset
        uint64_t i = 0;
        while (i < n) {
            // the block that starts at entry i: entries [i, j)
            uint64_t len = 4, j = i;
            while (j < n) {
                const uint64_t e = 9 + (k.off(j + 1) - k.off(j)) + (voff[j + 1] - voff[j]);
                if (len + e > kBlockBytes && len > 4) break;
                len += e;
                ++j;
                if (e + 4 > kBlockBytes) ++oversize;
            }
            const uint64_t klen0 = k.off(i + 1) - k.off(i);
            if (wr) {
                uint8_t *b = out->data + at;
                put32(b, (uint32_t)(j - i));
                uint64_t o = 4;
                for (uint64_t t = i; t < j; ++t) {
                    const uint64_t ks = k.off(t + 1) - k.off(t), vs = voff[t + 1] - voff[t];
                    put32(b + o, (uint32_t)ks);
                    put32(b + o + 4, (uint32_t)vs);
                    b[o + 8] = deleted && deleted[t] ? 1 : 0;
                    if (ks) memcpy(b + o + 9, k.data + k.off(t), ks);
                    if (vs) memcpy(b + o + 9 + ks, vals + voff[t], vs);
                    o += 9 + ks + vs;
                }
                if (len < kBlockBytes) memset(b + len, 0, kBlockBytes - len);
                uint8_t *x = out->index + iat;
                put32(x, (uint32_t)klen0);
                put64(x + 4, at);
                if (klen0) memcpy(x + 12, k.data + k.off(i), klen0);
            }
            at += len < kBlockBytes ? kBlockBytes : len;
            iat += 12 + klen0;
            ++blocks;
            i = j;
        }
        const uint64_t kmin = n ? k.off(1) - k.off(0) : 0, kmax = n ? k.off(n) - k.off(n - 1) : 0;
        if (wr) {
            put32(out->index, (uint32_t)blocks);
            put32(out->meta, (uint32_t)kmin);
            put32(out->meta + 4, (uint32_t)kmax);
            if (kmin) memcpy(out->meta + 8, k.data + k.off(0), kmin);
            if (kmax) memcpy(out->meta + 8 + kmin, k.data + k.off(n - 1), kmax);
        }
        s = SstSizes{blocks, at, iat, 8 + kmin + kmax, oversize};
    }
    *sz = s;
    return 0;
}

// [indexOffset u64][bloomOffset u64][metadataOffset u64][magic u32]      sstable_builder.go:223-228
void sst_footer(uint64_t index_offset, uint64_t bloom_offset, uint64_t metadata_offset, uint8_t *out28) {
    put64(out28, index_offset);
    put64(out28 + 8, bloom_offset);
    put64(out28 + 16, metadata_offset);
    put32(out28 + 24, 0x5354424Cu);
}

// ------------------------------------------------------------------------------------------------
// The host half of the batched compaction merge: SSTableIterator.loadBlock (lsm/compaction.go:69-124)
// for one block image, and mergeFiles' loop (:226-333) over k sorted runs of a block pool.
//
//   loadBlock: len < 4: no entries.  off = 4; for i < numEntries { off+9 > len: break;
//              keySize, valueSize, deleted = (byte == 1); off += 9; off+keySize+valueSize > len: break
//              (64-bit sums); yield; off += keySize + valueSize }
//   merge:     Less is by key alone (every Sequence is 0, :119), so one entry per distinct key comes out in
//              ascending key order; which of several equal-key entries it is depends on container/heap's
//              array order.  Here it is the entry of the lowest-numbered run (the one departure, see
//              seb_bloom.h).  targetLevel == 4 drops a surviving tombstone (:276).
// One walk serves plan and emit: out == nullptr only sizes.

uint32_t block_entries(const uint8_t *block, uint64_t len, uint16_t *entry_off, uint32_t cap) {
    if (len < 4) return 0;
    const uint32_t num = le32(block);
    uint64_t off = 4;
    uint32_t c = 0;
    for (uint32_t i = 0; i < num; ++i) {
        if (off + 9 > len) break;
        const uint64_t ks = le32(block + off), vs = le32(block + off + 4);
        if (off + 9 + ks + vs > len) break;
        if (c < cap) entry_off[c] = (uint16_t)off;
        ++c;
        off += 9 + ks + vs;
    }
    return c;
}

namespace {
struct MergeEnt {
    const uint8_t *p;  // the entry's 9-byte header; the key follows it, the value follows the key
    uint32_t ks, vs;
};
inline int ent_cmp(const MergeEnt &a, const MergeEnt &b) {
    const uint32_t n = a.ks < b.ks ? a.ks : b.ks;
    const int c = n ? memcmp(a.p + 9, b.p + 9, n) : 0;
    return c ? c : a.ks < b.ks ? -1 : a.ks > b.ks ? 1 : 0;
}
}  // namespace

// 0; -1 a null argument or a run_begin that decreases; -2 a run that is not strictly increasing (*err_run,
// *err_entry: the lowest-numbered such run and its first entry that is not above its predecessor); -3 out of
// memory; -4 2^32 entries or more; -5 (out != nullptr) the walk does not fit `want`.
int merge_walk(const uint8_t *pool, const uint16_t *blen, const uint64_t *run_begin, uint32_t num_runs, uint32_t flags,
               const MergeOut *out, const MergeSizes *want, MergeSizes *sz, uint32_t *err_run, uint64_t *err_entry) {
    if (!sz || (num_runs && !run_begin)) return -1;
    *sz = MergeSizes{0, 0, 0, 0, 0, 0};
    for (uint32_t r = 0; r < num_runs; ++r)
        if (run_begin[r + 1] < run_begin[r]) return -1;
    const uint64_t nblocks = num_runs ? run_begin[num_runs] : 0;
    if (num_runs && nblocks > run_begin[0] && (!pool || !blen)) return -1;  // num_runs == 0: run_begin may be null
    if (out && (!out->key_off || !out->val_off || !want)) return -1;
    try {
        std::vector<MergeEnt> ents;
        std::vector<uint64_t> first(num_runs + 1, 0);
        uint16_t offs[kMaxBlockEntries];
        for (uint32_t r = 0; r < num_runs; ++r) {
            first[r] = ents.size();
            for (uint64_t b = run_begin[r]; b < run_begin[r + 1]; ++b) {
                const uint8_t *blk = pool + b * kBlockBytes;
                const uint64_t len = blen[b] < kBlockBytes ? blen[b] : kBlockBytes;
                const uint32_t c = block_entries(blk, len, offs, kMaxBlockEntries);
                for (uint32_t i = 0; i < c; ++i) ents.push_back(MergeEnt{blk + offs[i], le32(blk + offs[i]), le32(blk + offs[i] + 4)});
            }
            if (ents.size() >= (1ull << 32)) return -4;
        }
        first[num_runs] = ents.size();
        MergeSizes s{ents.size(), 0, 0, 0, 0, 0};
        for (uint32_t r = 0; r < num_runs; ++r)
            for (uint64_t e = first[r] + 1; e < first[r + 1]; ++e)
                if (ent_cmp(ents[e - 1], ents[e]) >= 0) {
                    if (err_run) *err_run = r;
                    if (err_entry) *err_entry = e - first[r];
                    *sz = s;
                    return -2;
                }
        // a binary heap of run cursors, least key first, the lower-numbered run first among equal keys: the
        // first entry popped of each key is the survivor
        std::vector<uint64_t> cur(first.begin(), first.end() - 1);
        auto after = [&](uint32_t a, uint32_t b) {  // a comes out after b
            const int c = ent_cmp(ents[cur[a]], ents[cur[b]]);
            return c ? c > 0 : a > b;
        };
        std::vector<uint32_t> heap;
        for (uint32_t r = 0; r < num_runs; ++r)
            if (cur[r] < first[r + 1]) heap.push_back(r);
        std::make_heap(heap.begin(), heap.end(), after);
        const MergeEnt *last = nullptr;
        if (out) out->key_off[0] = out->val_off[0] = 0;
        while (!heap.empty()) {
            std::pop_heap(heap.begin(), heap.end(), after);
            const uint32_t r = heap.back();
            const MergeEnt &e = ents[cur[r]];
            if (++cur[r] < first[r + 1])
                std::push_heap(heap.begin(), heap.end(), after);
            else
                heap.pop_back();
            if (last && ent_cmp(*last, e) == 0) {
                ++s.shadowed;
                continue;
            }
            last = &e;
            const bool del = e.p[8] == 1;
            if (del && (flags & 1u)) {
                ++s.dropped;
                continue;
            }
            if (out) {
                if (s.entries_out >= want->entries_out || s.key_bytes + e.ks > want->key_bytes ||
                    s.val_bytes + e.vs > want->val_bytes || (e.ks && !out->keys) || (e.vs && !out->vals) || !out->deleted)
                    return -5;
                if (e.ks) memcpy(out->keys + s.key_bytes, e.p + 9, e.ks);
                if (e.vs) memcpy(out->vals + s.val_bytes, e.p + 9 + e.ks, e.vs);
                out->deleted[s.entries_out] = del ? 1 : 0;
                out->key_off[s.entries_out + 1] = s.key_bytes + e.ks;
                out->val_off[s.entries_out + 1] = s.val_bytes + e.vs;
            }
            ++s.entries_out;
            s.key_bytes += e.ks;
            s.val_bytes += e.vs;
        }
        *sz = s;
        return 0;
    } catch (const std::bad_alloc &) {
        return -3;
    }
}

}  // namespace seb
