// seb_values.cpp — the host half of the Get path's last step: LSM.Get returns the value, a copy
// of the block's bytes (lsm/sstable.go:276-278) or the memtable entry's Value (lsm/lsm.go:146-152, 157-163,
// 175-180).  For a key batch that is a gather: the found keys' values, which the join left as (source, run, vloc,
// vlen), back to back in batch order with an offset array.  No HIP dependency, so it compiles alone
// (tools/sanitize/values_check.cpp); the C ABI wrappers that set seb_last_error are in seb_recover.cpp.
#include "seb_values.h"

#include <cstring>

namespace seb {

namespace {

// *valid = carrying key i's value lies inside the source it names; then its address (null only for a value of no
// bytes in a source of none)
const uint8_t *value_at(const uint8_t *source, const uint8_t *run, const uint64_t *vloc, const uint32_t *vlen, uint64_t i,
                        const ValueSources &s, bool *valid) {
    const uint8_t *base;
    uint64_t bytes;
    if (source[i] == 0) {
        const uint32_t r = run ? run[i] : 0;
        if (r >= s.num_runs) return *valid = false, nullptr;
        base = s.vals[r], bytes = s.val_bytes[r];
        if (!base && bytes) return *valid = false, nullptr;
    } else if (source[i] == 1) {
        base = s.pool, bytes = s.pool_bytes;
    } else {
        return *valid = false, nullptr;
    }
    *valid = value_inside(vloc[i], vlen[i], bytes);
    return *valid && base ? base + vloc[i] : nullptr;
}

}  // namespace

int get_values(const uint8_t *status, const uint8_t *source, const uint8_t *run, const uint64_t *vloc, const uint32_t *vlen,
               uint64_t n, const ValueSources &src, ValuesSizes *sz, uint64_t *out_off, uint8_t *out_vals, uint64_t val_cap,
               uint64_t *bad) {
    if (!sz) return -1;
    *sz = ValuesSizes{n, 0, 0, 0};
    if (n >= (1ull << 32)) return -2;
    if (src.num_runs > kValuesMaxRuns) return -5;
    if (n && (!status || !source || !vloc || !vlen)) return -1;
    if ((src.num_runs && (!src.vals || !src.val_bytes)) || (src.num_runs > 1 && n && !run) || (src.pool_bytes && !src.pool))
        return -1;
    uint64_t found = 0, bytes = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (status[i] != 1 /* SEB_GET_FOUND */) continue;
        bool valid;
        value_at(source, run, vloc, vlen, i, src, &valid);
        if (!valid) {
            if (bad) *bad = i;
            return -3;
        }
        ++found;
        bytes += vlen[i];
    }
    sz->found = found;
    sz->val_bytes = bytes;
    if (!out_off && !out_vals) return 0;  // the plan
    if (val_cap < bytes) return -4;
    if (!out_off || (bytes && !out_vals)) return -1;
    uint64_t at = 0;
    out_off[0] = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (status[i] == 1 && vlen[i]) {
            bool valid;
            memcpy(out_vals + at, value_at(source, run, vloc, vlen, i, src, &valid), vlen[i]);
            at += vlen[i];
        }
        out_off[i + 1] = at;
    }
    return 0;
}

}  // namespace seb
