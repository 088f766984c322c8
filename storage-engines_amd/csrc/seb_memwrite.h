// seb_memwrite.h — the host-only code of seb_memwrite.cpp (no HIP dependency): the host half of the memtable's
// write side.  A Put / Delete batch framed as WAL.Append's records, MemTable.size's change for a new run in
// front of the active memtable's runs, and several runs folded into the one run GetAllEntries() returns.
#pragma once
#include <cstdint>

#include "seb_memtable.h"

namespace seb {

// ---- frame: LSM.Put / LSM.Delete -> WAL.Append (lsm/lsm.go:97-137, lsm/wal.go:31-65)

// rec_off[0..n] (nullable) and *image_bytes (nullable) for the batch: record i is 21 + keyLen + (deleted ? 0 :
// valueLen) bytes.  0; -1 a null argument; -2 op *bad_op's key offsets decrease or its key has 2^32 bytes or
// more; -3 the same of its value; -4 n >= 2^32.  An op's checks run before any later op's, and nothing but the
// offsets and the deleted bytes is read.
int frame_plan(const KeysView &keys, const uint64_t *val_off, const uint8_t *deleted, uint64_t *rec_off,
               uint64_t *image_bytes, uint64_t *bad_op);
// The sealed image into image[0, image_bytes): op i gets sequence first_seq + i.  frame_plan's codes; -5
// image_bytes is not the plan's.  Nothing outside the image is written.
int frame_emit(const KeysView &keys, const uint8_t *vals, const uint64_t *val_off, const uint8_t *deleted,
               uint64_t first_seq, uint8_t *image, uint64_t image_bytes, uint64_t *bad_op);
uint32_t crc32_ieee(const uint8_t *p, uint64_t n);  // hash/crc32.ChecksumIEEE

// ---- size delta: MemTable.size's change when `fresh` goes in front of `runs` (lsm/memtable.go:34-93)

// Every run is checked as runs_search checks it (run_check's codes; *bad_run = num_runs names `fresh`).  -1
// also for num_runs > kMemMaxRuns - 1 or a null required pointer.
int run_size_delta(const Run &fresh, const Run *runs, uint32_t num_runs, int64_t *delta, uint32_t *bad_run,
                   uint64_t *bad_entry);

// ---- fold: up to kMemMaxRuns runs, newest first, into one (GetAllEntries() of the memtable they add up to)

struct FoldSizes {  // seb_fold_sizes
    uint64_t entries_in, entries_out, key_bytes, val_bytes, shadowed, tombstones, max_sequence, memtable_size;
};
// out == nullptr sizes only (vals may then be null); with out, nothing past `want` (a plan's sizes) is written.
// 0; run_check's codes with *bad_run / *bad_entry; -1 a null argument or too many runs; -5 also for 2^32
// entries or more in total; -6 the walk does not fit `want`; -7 run *bad_run's val_off[n] passes its val_bytes.
int runs_fold(const Run *runs, const uint8_t *const *vals, const uint64_t *val_bytes, uint32_t num_runs,
              const ReplayOut *out, const FoldSizes *want, FoldSizes *sz, uint32_t *bad_run, uint64_t *bad_entry);

}  // namespace seb
