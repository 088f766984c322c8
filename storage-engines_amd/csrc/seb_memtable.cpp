// seb_memtable.cpp — the host half of the WAL replay: recoverFromWAL (lsm/lsm.go:273-298) feeding
// MemTable.Put / MemTable.Delete (lsm/memtable.go:34-93) and GetAllEntries (:129-137), for a whole log image at
// once.  No HIP dependency, so it compiles alone (tools/sanitize/replay_check.cpp); the C ABI wrappers that set
// seb_last_error are in seb_recover.cpp.
//
//   record   [crc u32][seq u64][keySize u32][valueSize u32][deleted u8][key][value], little-endian
//            (lsm/wal.go:31-62); deleted = (byte == 1) (:114)
//   replay   Put and Delete replace the whole entry of a key that is there (memtable.go:51-54, 82-85), so one
//            entry per distinct key survives: the one of the key's last record in log order, whatever its seq.
//            Delete stores Value nil whatever the record carried.  Entries are in ascending Go string order.
//   sequence the maximum over all records, overwritten ones included (lsm.go:286-288)
//   size     path independent: the sum over the survivors of keyLen + 16 + valueLen (memtable.go:54,60,85,91)
//
// That is a sort by (key, record index) with the last record of each key winning.  One walk serves plan and
// emit: out == nullptr only sizes.
//
// Below it, the host half of the batched memtable lookup over such runs (run_check, runs_search, get_join;
// tools/sanitize/memget_check.cpp compiles this file alone as well).
#include "seb_memtable.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

namespace seb {

namespace {
inline uint32_t le32(const uint8_t *p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}
inline uint64_t le64(const uint8_t *p) {
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
}
struct WalRec {
    const uint8_t *p;  // the record's 21-byte header; the key follows it, the value follows the key
    uint32_t ks, vs;
};
inline int key_cmp(const WalRec &a, const WalRec &b) {
    const uint32_t n = a.ks < b.ks ? a.ks : b.ks;
    const int c = n ? memcmp(a.p + kWalHeaderBytes, b.p + kWalHeaderBytes, n) : 0;
    return c ? c : a.ks < b.ks ? -1 : a.ks > b.ks ? 1 : 0;
}
}  // namespace

int replay_walk(const uint8_t *data, const uint64_t *rec_off, uint64_t n, const ReplayOut *out, const ReplaySizes *want,
                ReplaySizes *sz, uint64_t *err_rec) {
    if (!sz) return -1;
    *sz = ReplaySizes{0, 0, 0, 0, 0, 0, 0, 0};
    if (n && (!data || !rec_off)) return -1;
    if (out && (!out->key_off || !out->val_off || !want)) return -1;
    if (n >= (1ull << 32)) return -4;
    try {
        std::vector<WalRec> recs((size_t)n);
        ReplaySizes s{n, 0, 0, 0, 0, 0, 0, 0};
        const uint64_t lo = n ? rec_off[0] : 0, hi = n ? rec_off[n] : 0;
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t a = rec_off[i], b = rec_off[i + 1];
            if (a < lo || b < a || b > hi) {
                if (err_rec) *err_rec = i;
                *sz = ReplaySizes{n, 0, 0, 0, 0, 0, 0, 0};
                return -6;
            }
            const uint64_t len = b - a;
            bool framed = len >= kWalHeaderBytes;
            uint32_t ks = 0, vs = 0;
            if (framed) {
                ks = le32(data + a + 12), vs = le32(data + a + 16);
                framed = (uint64_t)kWalHeaderBytes + ks + vs == len;
            }
            if (!framed) {
                if (err_rec) *err_rec = i;
                *sz = ReplaySizes{n, 0, 0, 0, 0, 0, 0, 0};
                return -2;
            }
            recs[i] = WalRec{data + a, ks, vs};
            const uint64_t seq = le64(data + a + 4);
            if (seq > s.max_sequence) s.max_sequence = seq;
        }
        std::vector<uint32_t> order((size_t)n);
        for (uint64_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
            const int c = key_cmp(recs[x], recs[y]);
            return c ? c < 0 : x < y;
        });
        if (out) out->key_off[0] = out->val_off[0] = 0;
        for (uint64_t j = 0; j < n; ++j) {
            const WalRec &e = recs[order[j]];
            if (j + 1 < n && key_cmp(e, recs[order[j + 1]]) == 0) {  // a later record of this key replaces it
                ++s.overwritten;
                continue;
            }
            const bool del = e.p[20] == 1;
            const uint32_t vs = del ? 0 : e.vs;
            if (out) {
                if (s.entries_out >= want->entries_out || s.key_bytes + e.ks > want->key_bytes ||
                    s.val_bytes + vs > want->val_bytes || (e.ks && !out->keys) || (vs && !out->vals) || !out->deleted)
                    return -5;
                if (e.ks) memcpy(out->keys + s.key_bytes, e.p + kWalHeaderBytes, e.ks);
                if (vs) memcpy(out->vals + s.val_bytes, e.p + kWalHeaderBytes + e.ks, vs);
                out->deleted[s.entries_out] = del ? 1 : 0;
                if (out->seq) out->seq[s.entries_out] = le64(e.p + 4);
                out->key_off[s.entries_out + 1] = s.key_bytes + e.ks;
                out->val_off[s.entries_out + 1] = s.val_bytes + vs;
            }
            ++s.entries_out;
            s.key_bytes += e.ks;
            s.val_bytes += vs;
            s.tombstones += del ? 1 : 0;
            s.memtable_size += (uint64_t)e.ks + 16 + vs;
        }
        *sz = s;
        return 0;
    } catch (const std::bad_alloc &) {
        return -3;
    }
}

// ------------------------------------------------ batched memtable lookup (lsm/memtable.go:95-112, lsm/lsm.go:144-166)
//
//   MemTable.Get  idx := sort.Search(len(entries), entries[i].Key >= key); idx < len && entries[idx].Key == key
//                 -> (value, found = !deleted); LSM.Get returns on `found || value == nil && ...`: whichever
//                 memtable holds the key ends the Get, the active one first (lsm.go:148-166)
//   a run         GetAllEntries() in the builder's input layout, which the WAL replay and the merge emit

namespace {
inline int bytes_cmp(const uint8_t *a, uint64_t an, const uint8_t *b, uint64_t bn) {
    const uint64_t n = an < bn ? an : bn;
    const int c = n ? memcmp(a, b, n) : 0;
    return c ? c : an < bn ? -1 : an > bn ? 1 : 0;
}
}  // namespace

int run_check(const Run &r, uint64_t *entry) {
    if (r.n >= (1ull << 32)) return -5;
    if (r.n && (!r.key_off || !r.val_off || (!r.keys && r.key_bytes))) return -1;
    for (uint64_t e = 0; e < r.n; ++e) {
        if (entry) *entry = e;
        const uint64_t k0 = r.key_off[e], k1 = r.key_off[e + 1];
        if (k1 < k0 || k1 > r.key_bytes || k1 - k0 >= (1ull << 32)) return -2;
        const uint64_t v0 = r.val_off[e], v1 = r.val_off[e + 1];
        if (v1 < v0 || v1 - v0 >= (1ull << 32)) return -3;
        if (e) {  // entry e - 1 has passed, so its bytes may be read
            const uint64_t p0 = r.key_off[e - 1];
            if (bytes_cmp(r.keys + p0, k0 - p0, r.keys + k0, k1 - k0) >= 0) return -4;
        }
    }
    return 0;
}

int runs_search(const KeysView &kb, const Run *runs, uint32_t num_runs, uint8_t *status, uint8_t *run, uint32_t *entry,
                uint64_t *vloc, uint32_t *vlen, uint64_t *seq, uint32_t *bad_run, uint64_t *bad_entry) {
    if (num_runs > kMemMaxRuns || (num_runs && !runs)) return -1;
    if (kb.n >= (1ull << 32)) return -6;
    if (kb.n && (!status || (!kb.data && (kb.offsets || kb.stride)))) return -1;
    for (uint32_t r = 0; r < num_runs; ++r) {
        if (bad_run) *bad_run = r;
        const int rc = run_check(runs[r], bad_entry);
        if (rc) return rc;
    }
    for (uint64_t i = 0; i < kb.n; ++i) {
        const uint64_t o = kb.offsets ? kb.offsets[i] : i * (uint64_t)kb.stride;
        const uint64_t klen = kb.offsets ? kb.offsets[i + 1] - o : kb.stride;
        const uint8_t *key = kb.data + o;
        uint8_t st = kMemNone, rr = 0xFF;
        uint32_t ee = kMemNoEntry, vn = 0;
        uint64_t vl = 0, sq = 0;
        for (uint32_t r = 0; r < num_runs && st == kMemNone; ++r) {
            const Run &t = runs[r];
            uint64_t a = 0, b = t.n;  // sort.Search: the least index whose key is >= key
            while (a < b) {
                const uint64_t h = (a + b) >> 1;
                if (bytes_cmp(t.keys + t.key_off[h], t.key_off[h + 1] - t.key_off[h], key, klen) < 0)
                    a = h + 1;
                else
                    b = h;
            }
            if (a >= t.n || bytes_cmp(t.keys + t.key_off[a], t.key_off[a + 1] - t.key_off[a], key, klen) != 0) continue;
            const bool del = t.deleted && t.deleted[a] != 0;
            st = del ? kMemTombstone : kMemFound;
            rr = (uint8_t)r;
            ee = (uint32_t)a;
            if (!del) vl = t.val_off[a], vn = (uint32_t)(t.val_off[a + 1] - t.val_off[a]);  // Delete stores Value nil
            sq = t.seq ? t.seq[a] : 0;
        }
        status[i] = st;
        if (run) run[i] = rr;
        if (entry) entry[i] = ee;
        if (vloc) vloc[i] = vl;
        if (vlen) vlen[i] = vn;
        if (seq) seq[i] = sq;
    }
    return 0;
}

int get_join(const uint8_t *mem_status, const uint8_t *sst_status, uint64_t n, uint8_t *status, uint8_t *source) {
    if (n && (!mem_status || !sst_status || !status)) return -1;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t m = mem_status[i];
        const uint8_t s = m == kMemFound ? 1 /* SEB_GET_FOUND */ : m == kMemTombstone ? 0 /* SEB_GET_MISS */ : sst_status[i];
        if (source) source[i] = m == kMemNone ? 1 : 0;
        status[i] = s;
    }
    return 0;
}

}  // namespace seb
