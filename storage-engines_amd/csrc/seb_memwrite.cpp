// seb_memwrite.cpp — the host half of the memtable's write side.  No HIP dependency, so it
// compiles alone with seb_memtable.cpp (tools/sanitize/memwrite_check.cpp); the C ABI wrappers that set
// seb_last_error are in seb_write.cpp.
//
//   frame   LSM.Put / LSM.Delete take seq = atomic.AddUint64(&lsm.sequence, 1) and call WAL.Append(key, value,
//           seq, deleted) (lsm/lsm.go:97-137): [crc u32][seq u64][keySize u32][valueSize u32][deleted u8][key]
//           [value], little-endian, crc = ChecksumIEEE(record[4:]) (lsm/wal.go:31-62).  Delete appends value nil:
//           valueSize 0 and deleted 1, whatever value bytes the op arrays carry for it.
//   delta   MemTable.size is path independent, the sum over the entries of keyLen + 16 + valueLen with valueLen
//           0 for a tombstone (memtable.go:54,60,85,91).  A new run in front of the memtable's runs changes it
//           by: keyLen + 16 + valueLen for a key no run holds, valueLen - v_old where the first run that holds
//           the key has it with value length v_old (0 for a tombstone on either side).
//   fold    Put and Delete replace the whole entry of a key that is there (memtable.go:51-54, 82-85), so the
//           memtable after batches B1..Bk on top of `old` is fold([replay(Bk), .., replay(B1), old]): per
//           distinct key the entry of the lowest-numbered run that holds it, tombstones kept, in Go string order.
#include "seb_memwrite.h"

#include <cstring>
#include <new>
#include <vector>

namespace seb {

namespace {
inline int bytes_cmp(const uint8_t *a, uint64_t an, const uint8_t *b, uint64_t bn) {
    const uint64_t n = an < bn ? an : bn;
    const int c = n ? memcmp(a, b, n) : 0;
    return c ? c : an < bn ? -1 : an > bn ? 1 : 0;
}
inline void put32(uint8_t *p, uint32_t v) { memcpy(p, &v, 4); }
inline void put64(uint8_t *p, uint64_t v) { memcpy(p, &v, 8); }

struct CrcTable {
    uint32_t t[256];
    CrcTable() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = c & 1 ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[i] = c;
        }
    }
};

// op i's key and value lengths from the offsets alone: 0, -2 (key) or -3 (value)
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
    return 0;
}
}  // namespace

uint32_t crc32_ieee(const uint8_t *p, uint64_t n) {
    static const CrcTable tab;
    uint32_t c = ~0u;
    for (uint64_t i = 0; i < n; ++i) c = tab.t[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return ~c;
}

int frame_plan(const KeysView &kb, const uint64_t *val_off, const uint8_t *deleted, uint64_t *rec_off,
               uint64_t *image_bytes, uint64_t *bad_op) {
    if (kb.n >= (1ull << 32)) return -4;
    if (kb.n && !val_off) return -1;
    uint64_t at = 0;
    if (rec_off) rec_off[0] = 0;
    for (uint64_t i = 0; i < kb.n; ++i) {
        uint64_t klen, vlen;
        const int rc = op_lens(kb, val_off, i, &klen, &vlen);
        if (rc) {
            if (bad_op) *bad_op = i;
            return rc;
        }
        at += kWalHeaderBytes + klen + (deleted && deleted[i] ? 0 : vlen);
        if (rec_off) rec_off[i + 1] = at;
    }
    if (image_bytes) *image_bytes = at;
    return 0;
}

int frame_emit(const KeysView &kb, const uint8_t *vals, const uint64_t *val_off, const uint8_t *deleted,
               uint64_t first_seq, uint8_t *image, uint64_t image_bytes, uint64_t *bad_op) {
    uint64_t total = 0;
    const int rc = frame_plan(kb, val_off, deleted, nullptr, &total, bad_op);
    if (rc) return rc;
    if (total != image_bytes) return -5;
    if (kb.n && (!image || (!kb.data && (kb.offsets || kb.stride)))) return -1;
    uint8_t *p = image;
    for (uint64_t i = 0; i < kb.n; ++i) {
        const uint64_t ko = kb.offsets ? kb.offsets[i] : i * (uint64_t)kb.stride;
        const uint32_t klen = kb.offsets ? (uint32_t)(kb.offsets[i + 1] - ko) : kb.stride;
        const bool del = deleted && deleted[i];
        const uint32_t vlen = del ? 0 : (uint32_t)(val_off[i + 1] - val_off[i]);
        if (vlen && !vals) return -1;
        put64(p + 4, first_seq + i);
        put32(p + 12, klen);
        put32(p + 16, vlen);
        p[20] = del ? 1 : 0;
        if (klen) memcpy(p + kWalHeaderBytes, kb.data + ko, klen);
        if (vlen) memcpy(p + kWalHeaderBytes + klen, vals + val_off[i], vlen);
        const uint64_t len = (uint64_t)kWalHeaderBytes + klen + vlen;
        put32(p, crc32_ieee(p + 4, len - 4));
        p += len;
    }
    return 0;
}

// ------------------------------------------------ size delta

namespace {
// the least entry of t that is >= key; *eq = it is the key
inline uint64_t lower_bound(const Run &t, const uint8_t *key, uint64_t klen, bool *eq) {
    uint64_t a = 0, b = t.n;
    while (a < b) {
        const uint64_t h = (a + b) >> 1;
        if (bytes_cmp(t.keys + t.key_off[h], t.key_off[h + 1] - t.key_off[h], key, klen) < 0)
            a = h + 1;
        else
            b = h;
    }
    *eq = a < t.n && bytes_cmp(t.keys + t.key_off[a], t.key_off[a + 1] - t.key_off[a], key, klen) == 0;
    return a;
}
inline uint64_t live_vlen(const Run &t, uint64_t e) {
    return t.deleted && t.deleted[e] ? 0 : t.val_off[e + 1] - t.val_off[e];
}
}  // namespace

int run_size_delta(const Run &fresh, const Run *runs, uint32_t num_runs, int64_t *delta, uint32_t *bad_run,
                   uint64_t *bad_entry) {
    if (!delta || num_runs > kMemMaxRuns - 1 || (num_runs && !runs)) return -1;
    *delta = 0;
    for (uint32_t r = 0; r <= num_runs; ++r) {
        if (bad_run) *bad_run = r;
        const int rc = run_check(r < num_runs ? runs[r] : fresh, bad_entry);
        if (rc) return rc;
    }
    int64_t d = 0;
    for (uint64_t e = 0; e < fresh.n; ++e) {
        const uint8_t *key = fresh.keys + fresh.key_off[e];
        const uint64_t klen = fresh.key_off[e + 1] - fresh.key_off[e], vlen = live_vlen(fresh, e);
        bool held = false;
        for (uint32_t r = 0; r < num_runs && !held; ++r) {
            const uint64_t a = lower_bound(runs[r], key, klen, &held);
            if (held) d += (int64_t)vlen - (int64_t)live_vlen(runs[r], a);
        }
        if (!held) d += (int64_t)(klen + 16 + vlen);
    }
    *delta = d;
    return 0;
}

// ------------------------------------------------ fold

int runs_fold(const Run *runs, const uint8_t *const *vals, const uint64_t *val_bytes, uint32_t num_runs,
              const ReplayOut *out, const FoldSizes *want, FoldSizes *sz, uint32_t *bad_run, uint64_t *bad_entry) {
    if (!sz) return -1;
    *sz = FoldSizes{0, 0, 0, 0, 0, 0, 0, 0};
    if (num_runs > kMemMaxRuns || (num_runs && (!runs || !val_bytes))) return -1;
    if (out && (!out->key_off || !out->val_off || !want || (num_runs && !vals))) return -1;
    FoldSizes s{0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t r = 0; r < num_runs; ++r) {
        if (bad_run) *bad_run = r;
        const int rc = run_check(runs[r], bad_entry);
        if (rc) return rc;
        if (runs[r].n && runs[r].val_off[runs[r].n] > val_bytes[r]) return -7;
        s.entries_in += runs[r].n;
        if (runs[r].seq)
            for (uint64_t e = 0; e < runs[r].n; ++e)
                if (runs[r].seq[e] > s.max_sequence) s.max_sequence = runs[r].seq[e];
    }
    if (s.entries_in >= (1ull << 32)) return -5;
    // every run is sorted: a walk with one cursor per run, the least key first, the lowest run on a tie
    uint64_t at[kMemMaxRuns] = {0};
    if (out) out->key_off[0] = out->val_off[0] = 0;
    for (;;) {
        int w = -1;
        const uint8_t *wk = nullptr;
        uint64_t wl = 0;
        for (uint32_t r = 0; r < num_runs; ++r) {
            const Run &t = runs[r];
            if (at[r] >= t.n) continue;
            const uint8_t *k = t.keys + t.key_off[at[r]];
            const uint64_t kl = t.key_off[at[r] + 1] - t.key_off[at[r]];
            if (w < 0 || bytes_cmp(k, kl, wk, wl) < 0) w = (int)r, wk = k, wl = kl;
        }
        if (w < 0) break;
        const Run &t = runs[w];
        const uint64_t e = at[w];
        for (uint32_t r = 0; r < num_runs; ++r) {  // the key's other holders are shadowed
            const Run &u = runs[r];
            if (at[r] >= u.n) continue;
            if (bytes_cmp(u.keys + u.key_off[at[r]], u.key_off[at[r] + 1] - u.key_off[at[r]], wk, wl) == 0) {
                ++at[r];
                if ((int)r != w) ++s.shadowed;
            }
        }
        const bool del = t.deleted && t.deleted[e];
        const uint64_t vl = del ? 0 : t.val_off[e + 1] - t.val_off[e];  // Delete stores Value nil
        if (out) {
            if (s.entries_out >= want->entries_out || s.key_bytes + wl > want->key_bytes ||
                s.val_bytes + vl > want->val_bytes || (wl && !out->keys) || (vl && (!out->vals || !vals[w])) ||
                !out->deleted)
                return -6;
            if (wl) memcpy(out->keys + s.key_bytes, wk, wl);
            if (vl) memcpy(out->vals + s.val_bytes, vals[w] + t.val_off[e], vl);
            out->deleted[s.entries_out] = del ? 1 : 0;
            if (out->seq) out->seq[s.entries_out] = t.seq ? t.seq[e] : 0;
            out->key_off[s.entries_out + 1] = s.key_bytes + wl;
            out->val_off[s.entries_out + 1] = s.val_bytes + vl;
        }
        ++s.entries_out;
        s.key_bytes += wl;
        s.val_bytes += vl;
        s.tombstones += del ? 1 : 0;
        s.memtable_size += wl + 16 + vl;
    }
    *sz = s;
    return 0;
}

}  // namespace seb
