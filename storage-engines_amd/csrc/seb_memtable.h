// seb_memtable.h — the host-only code of seb_memtable.cpp (no HIP dependency): the host half of the WAL
// replay, a log image into the memtable's sorted run, and of the batched memtable lookup over such runs.
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

// ---- batched memtable lookup: MemTable.Get (lsm/memtable.go:95-112) over LSM.Get's runs (lsm/lsm.go:144-166)

struct Run {  // seb_run: a sorted run in the builder's input layout
    const uint8_t *keys;
    uint64_t key_bytes;
    const uint64_t *key_off, *val_off;
    const uint8_t *deleted;  // nullable; any non-zero byte = deleted (the builder's input rule)
    const uint64_t *seq;     // nullable
    uint64_t n;
};
struct KeysView {  // seb_keys without its reserved word
    const uint8_t *data;
    const uint64_t *offsets;
    uint64_t n;
    uint32_t stride;
};
constexpr uint32_t kMemMaxRuns = 8;  // SEB_MEM_MAX_RUNS
enum : uint8_t { kMemNone = 0, kMemFound = 1, kMemTombstone = 2 };
constexpr uint32_t kMemNoEntry = 0xFFFFFFFFu;  // SEB_MEM_NO_ENTRY

// What seb_dev_run_index checks, entry by entry in this order: key_off[e] <= key_off[e+1] <= key_bytes and a key
// below 2^32 bytes (-2), val_off[e] <= val_off[e+1] and a value below 2^32 bytes (-3), key e-1 < key e in Go
// string order (-4).  0; -1 a null array with n != 0; -5 n >= 2^32; otherwise *entry = the first entry that
// fails.  No key byte of an entry is read before its offsets and its predecessor's have passed.
int run_check(const Run &run, uint64_t *entry);
// status (required), run, entry, vloc, vlen, seq: n elements each, nullable.  Every run is checked first
// (run_check's code, *bad_run and *bad_entry naming the run and entry); -1 also for num_runs > kMemMaxRuns or
// a null required pointer; -6 keys.n >= 2^32.
int runs_search(const KeysView &keys, const Run *runs, uint32_t num_runs, uint8_t *status, uint8_t *run, uint32_t *entry,
                uint64_t *vloc, uint32_t *vlen, uint64_t *seq, uint32_t *bad_run, uint64_t *bad_entry);
// LSM.Get's decision over both halves: a memtable answer ends the Get (a tombstone as "not found", before any
// file is read); otherwise the SSTables' answer stands.  source (nullable): 0 the memtables, 1 the SSTables.
// status may alias sst_status.  -1: a null required pointer.
int get_join(const uint8_t *mem_status, const uint8_t *sst_status, uint64_t n, uint8_t *status, uint8_t *source);

}  // namespace seb
