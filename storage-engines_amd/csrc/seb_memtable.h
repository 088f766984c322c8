// seb_memtable.h — the host-only code of seb_memtable.cpp (no HIP dependency): the host half of the WAL
// replay, a log image into the memtable's sorted run.
#pragma once
#include <cstdint>

namespace seb {

constexpr uint32_t kWalHeaderBytes = 21;  // [crc u32][seq u64][keySize u32][valueSize u32][deleted u8]

struct ReplaySizes {  // seb_replay_sizes
    uint64_t records_in, entries_out, key_bytes, val_bytes, overwritten, tombstones, max_sequence, memtable_size;
};
struct ReplayOut {  // the run in the builder's layout (entries_out + 1 offsets each) and the survivors' sequences
    uint8_t *keys;
    uint64_t *key_off;
    uint8_t *vals;
    uint64_t *val_off;
    uint8_t *deleted;
    uint64_t *seq;  // nullable
};
// recoverFromWAL + GetAllEntries over records [rec_off[i], rec_off[i+1]) of data: out == nullptr sizes only;
// with out, nothing past `want` (a plan's sizes) is written.  0; -1 a null argument; -2 record *err_rec is not
// framed (length < 21, or 21 + keySize + valueSize != length); -3 out of memory; -4 2^32 records or more; -5 the
// walk does not fit `want`; -6 record *err_rec's offsets decrease or leave [rec_off[0], rec_off[n]].  The first
// record that fails either check is the one named.  No byte outside [rec_off[0], rec_off[n]) is read, and none
// of a record before its framing has been checked.
int replay_walk(const uint8_t *data, const uint64_t *rec_off, uint64_t n, const ReplayOut *out, const ReplaySizes *want,
                ReplaySizes *sz, uint64_t *err_rec);

}  // namespace seb
