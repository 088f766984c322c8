// seb_getpath.cpp — the host half of the Get path: LSM.Get returns at the first memtable that
// holds the key, value or tombstone, and reads no filter, index or block for it (lsm/lsm.go:144-166).  For a key
// batch that is a stream compaction between the memtable lookup and the SSTable steps, and a join that puts the
// SSTables' answers for the m compacted keys back on their batch rows.  No HIP dependency, so it compiles alone
// (tools/sanitize/getpath_check.cpp); the C ABI wrappers that set seb_last_error are in seb_recover.cpp.
#include "seb_getpath.h"

#include <cstring>

namespace seb {

int get_compact(const KeysView &kb, const uint8_t *mem, CompactSizes *sz, uint8_t *out_keys, uint64_t key_cap,
                uint64_t *out_off, uint32_t *row, uint64_t row_cap, uint64_t *bad) {
    if (!sz) return -1;
    *sz = CompactSizes{kb.n, 0, 0, 0};
    if (kb.n >= (1ull << 32)) return -2;
    if (kb.n && (!mem || (!kb.data && (kb.offsets || kb.stride)))) return -1;
    uint64_t und = 0, bytes = 0;
    for (uint64_t i = 0; i < kb.n; ++i) {
        if (kb.offsets && kb.offsets[i + 1] < kb.offsets[i]) {
            if (bad) *bad = i;
            return -3;
        }
        if (!mem_undecided(mem[i])) continue;
        ++und;
        bytes += kb.offsets ? kb.offsets[i + 1] - kb.offsets[i] : kb.stride;
    }
    sz->undecided = und;
    sz->key_bytes = bytes;
    if (!out_keys && !out_off && !row) return 0;  // the plan
    if (row_cap < und || key_cap < bytes) return -4;
    if ((und && !row) || (bytes && !out_keys) || (kb.offsets && !out_off)) return -1;
    uint64_t j = 0, at = 0;
    if (kb.offsets) out_off[0] = 0;
    for (uint64_t i = 0; i < kb.n; ++i) {
        if (!mem_undecided(mem[i])) continue;
        const uint64_t o = kb.offsets ? kb.offsets[i] : i * (uint64_t)kb.stride;
        const uint64_t len = kb.offsets ? kb.offsets[i + 1] - o : kb.stride;
        if (len) memcpy(out_keys + at, kb.data + o, len);
        at += len;
        row[j++] = (uint32_t)i;
        if (kb.offsets) out_off[j] = at;
    }
    return 0;
}

int get_join_rows(const uint8_t *mem, const uint64_t *mem_vloc, const uint32_t *mem_vlen, uint64_t n, const uint32_t *row,
                  uint64_t m, const uint8_t *sst_status, const uint16_t *sst_col, const uint64_t *sst_vloc,
                  const uint32_t *sst_vlen, uint8_t *status, uint8_t *source, uint16_t *col, uint64_t *vloc, uint32_t *vlen) {
    if (n >= (1ull << 32)) return -2;
    if ((n && (!mem || !status)) || (m && (!row || !sst_status))) return -1;
    for (uint64_t i = 0; i < n; ++i) {  // the memtables' answer, or "no row names this key"
        const uint8_t ms = mem[i];
        const bool found = ms == kMemFound;
        status[i] = found ? 1 /* SEB_GET_FOUND */ : 0 /* SEB_GET_MISS */;
        if (source) source[i] = mem_undecided(ms) ? 1 : 0;
        if (col) col[i] = 0xFFFF;
        if (vloc) vloc[i] = found && mem_vloc ? mem_vloc[i] : 0;
        if (vlen) vlen[i] = found && mem_vlen ? mem_vlen[i] : 0;
    }
    for (uint64_t j = 0; j < m; ++j) {  // a row outside the batch, or one naming a decided key, is ignored
        const uint64_t i = row[j];
        if (i >= n || !mem_undecided(mem[i])) continue;
        status[i] = sst_status[j];
        if (col) col[i] = sst_col ? sst_col[j] : 0xFFFF;
        if (vloc) vloc[i] = sst_vloc ? sst_vloc[j] : 0;
        if (vlen) vlen[i] = sst_vlen ? sst_vlen[j] : 0;
    }
    return 0;
}

}  // namespace seb
