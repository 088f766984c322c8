// seb_values.h — the host-only code of seb_values.cpp (no HIP dependency): the host half of the Get path's last
// step, the found values gathered into one dense buffer.
#pragma once
#include <cstdint>

namespace seb {

struct ValuesSizes {  // seb_values_sizes
    uint64_t n, found, val_bytes, reserved;
};

constexpr uint32_t kValuesMaxRuns = 8;  // SEB_MEM_MAX_RUNS

// Where the values lie: the runs' value bytes (vals[r][0, val_bytes[r]), r < num_runs) and the block pool.
struct ValueSources {
    const uint8_t *const *vals;
    const uint64_t *val_bytes;
    uint32_t num_runs;
    const uint8_t *pool;
    uint64_t pool_bytes;
};

// The one rule both halves apply to a carrying key (status == SEB_GET_FOUND): true where its value lies inside
// the source it names.  The comparisons are made this way round so that nothing wraps.
inline bool value_inside(uint64_t vloc, uint32_t vlen, uint64_t bytes) { return vloc <= bytes && vlen <= bytes - vloc; }

// Key i carries a value iff status[i] == SEB_GET_FOUND; out_off[0..n] and the values back to back in batch order.
// sz always; out_off and out_vals both null: sizes only.  run may be null where num_runs <= 1 (read as 0).
// 0; -1 a null required pointer (or a null pool with pool_bytes != 0); -2 n >= 2^32; -3 the carrying key *bad is
// invalid (the lowest one; sz holds n alone); -4 val_cap < val_bytes: sz is filled and nothing is written; -5
// num_runs > kValuesMaxRuns.
int get_values(const uint8_t *status, const uint8_t *source, const uint8_t *run, const uint64_t *vloc, const uint32_t *vlen,
               uint64_t n, const ValueSources &src, ValuesSizes *sz, uint64_t *out_off, uint8_t *out_vals, uint64_t val_cap,
               uint64_t *bad);

}  // namespace seb
