// seb_kernels.h — internal interface between the C-ABI host layer and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace seb {

// Reduction constants for one filter, computed on the host (seb_host.h: mod_arg()).
struct ModArg {
    uint64_t m;   // numBits (>= 1)
    uint64_t mu;  // floor((2^64 - 1) / m)
    uint64_t c;   // 2^64 mod m
    uint32_t k;   // numHashes
    uint32_t pad;
};
// Filters with m below this take the u32-residue kernels (template flag M32): the Barrett
// quotient (mod_m31) is at most one low, so x - q*m < 2m fits in 32 bits.
constexpr uint64_t kM32Limit = 1ull << 31;

struct KeyBatch {  // device pointers
    const uint8_t *data;
    const uint64_t *offsets;  // n+1 or nullptr
    uint64_t n;
    uint32_t stride;
    const uint4 *hashes = nullptr;   // pre-hashed batch: (h1 lo, h1 hi, h2 lo, h2 hi) per key
};

constexpr int kMaxMulti = 64;
struct MultiFilter {
    const uint32_t *words;
    ModArg md;
};
struct MultiArg {  // passed by value (kernel arguments), <= 64 filters
    MultiFilter f[kMaxMulti];
    uint32_t nf;
    uint32_t pad;
};

constexpr int kMaxMany = 32;
constexpr uint64_t kLdsFilterBytes = 160 * 1024;  // a filter whose word array fits one CU's LDS
struct ManyFilter {
    uint32_t *words;
    uint64_t nwords;
    uint64_t key_begin, key_end;
    ModArg md;
};
struct ManyArg {
    ManyFilter f[kMaxMany];
    uint32_t nf;
    uint32_t pad;
};

// One registered SSTable filter, in LSM lookup order (k_multiget).
struct RegSlot {
    const uint32_t *words;
    ModArg md;
    uint32_t min_off, min_len, max_off, max_len;  // key range bytes in the registry's range buffer
    int32_t level;
    uint32_t slot;          // bit of the output mask
    int32_t gbit;           // L0 group member: its bit in the group table's entries, else -1
    uint32_t pad;
    uint64_t min_be[2];     // first 16 bytes of MinKey / MaxKey as big-endian words (zero padded)
    uint64_t max_be[2];
};
struct RegLayout {          // slot index ranges per level (lookup order) + shape flags
    uint32_t lo[5], hi[5];
    uint32_t nonoverlap;    // bit L: level L's files are disjoint and in MinKey order (bisection exact)
    uint32_t all_k7_m32;    // every filter has k == 7 and m < kM32Limit (2^31)
    // L0 group: the L0 files sharing one (m, k), every key tests all of them, as one bit-interleaved
    // table (entry p = bit p of each member, l0b bits per entry): one gather per position for the
    // whole group.  l0g == 0: none.
    const uint32_t *l0tab;
    ModArg l0md;
    uint32_t l0g, l0b;
};
constexpr uint32_t kL0GroupMax = 32;
struct L0Members {          // builder argument: the group's word arrays, in bit order
    const uint32_t *w[kL0GroupMax];
};
uint64_t l0_table_words(uint64_t m, uint32_t bits);
hipError_t launch_l0_table(const L0Members &mem, uint32_t g, uint32_t bits, uint64_t m, uint32_t *table,
                           hipStream_t s);
// seb_codec.hip: shard routing (FNV-1a32) and WAL CRC32
hipError_t launch_route(const KeyBatch &kb, uint32_t bits, uint16_t *shard, uint32_t *hash, hipStream_t s);
uint64_t route_workspace_bytes(uint64_t n, uint32_t bits);
hipError_t launch_route_partition(const KeyBatch &kb, uint32_t bits, uint32_t *perm, uint64_t *shard_begin,
                                  uint16_t *shard_out, void *ws, uint64_t ws_bytes, hipStream_t s);
hipError_t launch_wal_crc(uint8_t *data, const uint64_t *off, uint64_t n, int mode, uint32_t *crc, uint8_t *ok,
                          hipStream_t s);
// The scatter-free order's segment tables (multiget_order 1): segment s = b * C + sc is bucket b's
// run of 4096-key super-chunk sc; seg[s] = its first sorted row (low 32 bits, non-decreasing in s)
// | (sc << 12 | the run's offset in the super-chunk's bucket-sorted keys) << 32; half[s] = its keys
// in the super-chunk's first 2048-key chunk; wstart[w] = the segment of row 64 w.
struct MgSeg {
    const uint64_t *seg = nullptr;  // null: rows are read linearly (or through key_order)
    const uint32_t *wstart = nullptr;
    const uint32_t *half = nullptr;
    uint32_t nseg = 0, C = 0, nb = 0, pad = 0;
    uint32_t part_lo = 0;  // the partition level's first lookup-ordered slot: bucket b >= 1's file is part_lo + b - 1
    // per bucket b and level L = 1..4, brange[4 b + L - 1] = A | B << 16: a disjoint level's bisection for a
    // key of bucket b ends in [lo + A, lo + B] (the files whose MinKey can bound the bucket's keys); null: none
    const uint32_t *brange = nullptr;
};
// cand != null: the list form (cap u16 slots per key, any nslots) instead of masks.
constexpr uint32_t kRegMaxFiles = 4096;  // registry capacity (u16 slot ids, 0xFFFF = none)
// Answer j goes to row j of maybe / cand; key_order != null: key j is read as key key_order[j] of kb.
hipError_t launch_multiget(const KeyBatch &kb, const RegSlot *slots, uint32_t nslots, const RegLayout &lay,
                           const uint8_t *ranges, uint64_t *maybe, uint16_t *cand, uint32_t cap, hipStream_t s,
                           const uint32_t *key_order, const MgSeg &seg = MgSeg{}, bool narrow = false);
// Key-range order for MultiGet: buckets = files of slots [lo, hi) (a disjoint, MinKey-ordered
// level) with MinKey <= key.  The MultiGet then answers into mo.answers (sorted rows) and
// launch_multiget_unpermute writes them to the caller's output in batch order.
constexpr uint32_t kMgMaxBuckets = 1025;
struct MgOrder {
    bool active = false;          // false: the level does not apply; answer in batch order directly
    uint64_t n = 0;
    uint32_t nb = 0, bits = 0;            // buckets of the partition level, bits of a bucket id
    const void *bucket = nullptr;         // each key's bucket, in batch order (u8 when bucket8, else u16)
    bool bucket8 = false;
    const uint32_t *runs = nullptr;       // per chunk and bucket: the first sorted row of its run
    const uint32_t *key_order = nullptr;  // batches that are not moved: key index of each sorted row
    const uint8_t *keys = nullptr;        // aligned fixed 16-B batches: the keys moved into that order
    void *answers = nullptr;              // n * answer_bytes: the MultiGet's answers in sorted rows
    MgSeg seg;                            // the scatter-free order: keys read through segments
    int narrow = 0;  // sorted rows held narrow: 1 u32 masks (slots all < 32), 2 u8 list rows (slots all < 255)
};
// Aligned fixed 16-B batches are sorted by bucket inside each chunk and read through the segment
// tables (multiget_order 1) or moved into that order (multiget_order 2; 16 B more per key), others
// get an index.  nb: the partition level's bucket count (its files + 1).
bool multiget_order_moves(const KeyBatch &kb);
uint64_t multiget_order_bytes(const KeyBatch &kb, uint64_t answer_bytes, uint32_t nb);
hipError_t launch_multiget_order(const KeyBatch &kb, const RegSlot *slots, uint32_t lo, uint32_t hi,
                                 const uint8_t *ranges, void *ws, MgOrder *mo, hipStream_t s);
hipError_t launch_multiget_unpermute(const MgOrder &mo, void *out, uint64_t answer_bytes, hipStream_t s);

// seb_locate.hip: a registered file's sparse index (lsm/sstable.go:168-201) in HBM as a structure of
// arrays, one table entry per registry slot id (a free slot, or a file without an index yet: all zero).
struct LocSlot {
    const uint64_t *pre;   // entry e: pre[2e], pre[2e+1] = its key's first 16 bytes, zero padded, big-endian (16-B aligned)
    const uint64_t *koff;  // n + 1 offsets into bytes: key e = bytes[koff[e], koff[e+1]), so its length too
    const uint64_t *boff;  // entry e's BlockOffset
    const uint8_t *bytes;  // the keys' bytes, read only where 16-byte prefixes tie
    uint32_t n;            // entries
    uint32_t pad;
};
constexpr uint64_t kNoBlock = ~0ull;  // SEB_NO_BLOCK
// blocks[i * cap + j] = the block offset SSTable.Get would read for key i in the file of slot
// cand[i * cap + j] (lsm/sstable.go:210-222), kNoBlock for none; slots >= ntab have no index.
hipError_t launch_locate(const KeyBatch &kb, const uint16_t *cand, uint32_t cap, const LocSlot *tab, uint32_t ntab,
                         uint64_t *blocks, hipStream_t s);

// seb_search.hip: searchBlock (lsm/sstable.go:242-290) for every cell of a MultiGet's rows, and
// LSM.Get's decision over each row (lsm/lsm.go:174-197).  Block b of the caller's pool is
// pool[b * kBlockBytes, b * kBlockBytes + min(blen[b], kBlockBytes)).
constexpr uint32_t kBlockBytes = 4096;        // SEB_BLOCK_BYTES
constexpr uint32_t kNoBlockId = 0xFFFFFFFFu;  // SEB_NO_BLOCK_ID
enum : uint32_t { kCellNone = 0, kCellMiss = 1, kCellFound = 2, kCellTombstone = 3, kCellTrunc = 4 };
enum : uint8_t { kGetMiss = 0, kGetFound = 1, kGetError = 2 };
// cells[c] = status << 28 | voff << 13 | vlen for key c / cap in block bid[c]; kCellNone for an id >= nblocks.
hipError_t launch_search_blocks(const KeyBatch &kb, const uint32_t *bid, uint32_t cap, const uint8_t *pool,
                                const uint16_t *blen, uint32_t nblocks, uint32_t *cells, hipStream_t s);
// Per key, the first FOUND or TRUNC cell of its row decides; col / vloc / vlen may be null.
hipError_t launch_resolve_rows(const uint32_t *cells, const uint32_t *bid, uint64_t n, uint32_t cap, uint8_t *status,
                               uint16_t *col, uint64_t *vloc, uint32_t *vlen, hipStream_t s);

// seb_sst.hip: the batched SSTable builder (lsm/sstable_builder.go:42-135,185-290): the block cut of many
// files (entries [file_begin[f], file_begin[f+1]) of one batch), then their data blocks, index blocks and
// metadata.  The plan lives in a caller-provided workspace: offsets of its arrays, all 16-byte aligned.
constexpr uint32_t kSstTile = 1024;  // entries per tile of the cut; > 454, the most a block holds
struct SstWs {
    uint64_t bytes, tiles;
    uint64_t fbeg, ovs_cnt, ovs_exc, fbk, fix, sizes, meta_len;      // per file
    uint64_t entry, tile_cnt, tile_base, tile_ix, tile_ixbase;       // per tile
    uint64_t nxt, ex, tix, blk_first;                                // per entry / per block
};
SstWs sst_ws_layout(uint64_t n, uint32_t num_files);
// n >= 1, num_files >= 1, n < 2^32.  Synchronises the stream; sizes_host: num_files x seb_sst_sizes.
hipError_t launch_sst_plan(const KeyBatch &kb, const uint64_t *voff, const uint64_t *file_begin_host, uint32_t num_files,
                           void *ws, void *sizes_host, hipStream_t s);
// A plan without oversized entries; nblocks / index_total / meta_total: the sums of the plan's sizes, past
// which nothing is written.
hipError_t launch_sst_encode(const KeyBatch &kb, const uint8_t *vals, const uint64_t *voff, const uint8_t *deleted,
                             uint32_t num_files, const void *ws, uint64_t nblocks, uint64_t index_total,
                             uint64_t meta_total, uint8_t *data, uint16_t *blen, uint8_t *index, uint8_t *meta,
                             hipStream_t s);

// seb_merge.hip: the batched compaction merge (lsm/compaction.go:69-124,226-333): k sorted runs of a block
// pool into one sorted, de-duplicated run in the builder's input layout.  The plan lives in a caller-provided
// workspace: a 128-byte header, then arrays at these offsets, all 16-byte aligned.
constexpr uint32_t kMergeTile = 1024;  // records per tile of a merge pass, of the survivor scan and of the emit
constexpr uint32_t kMergeMaxRuns = 1u << 20;  // SEB_MERGE_MAX_RUNS
struct MergeWs {
    uint64_t bytes, head_bytes, tiles;
    // per run, per block, per 256 blocks: placed before anything that depends on n
    uint64_t run_begin, run_first, block_first, groups;
    // per tile x 3, per entry x 2, the passes' tile tables, one pass's cuts
    uint64_t sums, rec_a, rec_b, tab, tab_cap, cuts;
    uint32_t passes;
};
MergeWs merge_ws_layout(uint64_t n, uint32_t num_blocks, uint32_t num_runs);
uint64_t merge_emit_min_bytes(uint64_t n);  // the least workspace a plan of n entries can have
hipError_t launch_merge_count(const uint8_t *pool, const uint16_t *blen, uint32_t num_blocks, uint16_t *block_entries,
                              hipStream_t s);
// The plan in three steps, each of which synchronises the stream (num_runs >= 1, num_blocks >= 1):
// head: the blocks' first records; *n_host = the entry count, run_first_host[num_runs + 1] = the runs' first
// records (needs head_bytes of workspace); decode (n >= 1, n < 2^32, the whole workspace): the records and the
// order check, *err_host = run << 32 | entry of the least offender, all ones for none; tree: the merge
// passes and the survivors, sizes_host = one seb_merge_sizes.
hipError_t launch_merge_head(const uint64_t *run_begin_host, uint32_t num_runs, const uint16_t *block_entries,
                             uint32_t num_blocks, void *ws, uint64_t *n_host, uint64_t *run_first_host, hipStream_t s);
hipError_t launch_merge_decode(const uint8_t *pool, const uint16_t *blen, uint32_t num_blocks, uint32_t num_runs,
                               uint64_t n, void *ws, uint64_t *err_host, hipStream_t s);
hipError_t launch_merge_tree(const uint8_t *pool, uint32_t num_blocks, uint32_t num_runs, uint64_t n,
                             const uint64_t *run_first_host, uint32_t flags, void *ws, void *sizes_host, hipStream_t s);
// *ok = the workspace's header is the plan's that returned `sizes` (one seb_merge_sizes) and its arrays lie inside
// ws_bytes; reads the header back, so it waits for what the stream holds.
hipError_t merge_ws_check(const void *sizes, const void *ws, uint64_t ws_bytes, bool *ok, hipStream_t s);
// sizes: one seb_merge_sizes with entries_in >= 1; nothing past its entries_out / key_bytes / val_bytes is written.
hipError_t launch_merge_emit(const uint8_t *pool, const void *sizes, const void *ws, uint8_t *keys, uint64_t *key_off,
                             uint8_t *vals, uint64_t *val_off, uint8_t *deleted, hipStream_t s);

// seb_replay.hip: the WAL replay (lsm/lsm.go:273-298 over lsm/memtable.go:34-93,129-137): the records of a log
// image into one sorted run, the last record of each key surviving, in the builder's input layout.  The plan
// lives in a caller-provided workspace: a 128-byte header, then arrays at these offsets, all 16-byte aligned.
// Tiles are kMergeTile records.
struct ReplayWs {
    uint64_t bytes, tiles;
    uint64_t sums, rec_a, rec_b, cuts;  // per tile x 3, per record x 2, two per tile
    uint32_t passes;
};
ReplayWs replay_ws_layout(uint64_t n);
uint64_t replay_emit_min_bytes(uint64_t n);  // the least workspace a plan of n records can have
// n >= 1, n < 2^32, the whole workspace.  Synchronises the stream; sizes_host = one seb_replay_sizes; *err_host =
// record << 1 | (1: not framed, 0: its offsets decrease) of the least bad record, all ones for none.
hipError_t launch_replay_plan(const uint8_t *data, const uint64_t *rec_off, uint64_t n, void *ws, void *sizes_host,
                              uint64_t *err_host, hipStream_t s);
// *ok = the workspace's header is the plan's that returned `sizes` (one seb_replay_sizes) and its arrays lie
// inside ws_bytes; reads the header back, so it waits for what the stream holds.
hipError_t replay_ws_check(const void *sizes, const void *ws, uint64_t ws_bytes, bool *ok, hipStream_t s);
// sizes: one seb_replay_sizes with records_in >= 1; nothing past its entries_out / key_bytes / val_bytes is
// written; seq may be null.
hipError_t launch_replay_emit(const uint8_t *data, const uint64_t *rec_off, const void *sizes, const void *ws, uint8_t *keys,
                              uint64_t *key_off, uint8_t *vals, uint64_t *val_off, uint8_t *deleted, uint64_t *seq,
                              hipStream_t s);

// seb_memget.hip: the batched memtable lookup (lsm/lsm.go:144-166 over lsm/memtable.go:95-112): a key batch
// against up to kMemRuns sorted runs in the builder's input layout, the first run that holds a key deciding.
constexpr uint32_t kMemRuns = 8;  // SEB_MEM_MAX_RUNS
enum : uint32_t { kMemStatusNone = 0, kMemStatusFound = 1, kMemStatusTombstone = 2 };
struct MemRun {  // device pointers; pre = run_index_prefixes(the run's index)
    const uint64_t *pre;   // entry e: pre[2e], pre[2e+1] = its key's first 16 bytes, zero padded, big-endian (16-B aligned)
    const uint64_t *koff;  // n + 1 offsets into bytes
    const uint64_t *voff;  // n + 1 value offsets
    const uint8_t *bytes;  // the keys' bytes, read only where 16-byte prefixes tie
    const uint8_t *deleted;  // nullable
    const uint64_t *seq;     // nullable
    uint64_t key_bytes;
    uint32_t n;
    uint32_t pad;
};
struct MemRunTab {  // passed by value (kernel arguments)
    MemRun r[kMemRuns];
    uint32_t nruns;
    uint32_t pad;
};
struct MemOut {  // n elements each; all but status nullable
    uint8_t *status, *run;
    uint32_t *entry;
    uint64_t *vloc;
    uint32_t *vlen;
    uint64_t *seq;
};
uint64_t run_index_bytes(uint64_t n);  // 0 for n == 0
const uint64_t *run_index_prefixes(const void *index);
// n >= 1; the index is 16-byte aligned device memory of run_index_bytes(n).  Synchronises the stream; *err_host =
// entry << 2 | (0: its key offsets, 1: its value offsets, 2: not above its predecessor) of the least offender,
// all ones for none.
hipError_t launch_run_index(const uint8_t *bytes, uint64_t key_bytes, const uint64_t *koff, const uint64_t *voff,
                            uint32_t n, void *index, uint64_t *err_host, hipStream_t s);
hipError_t launch_runs_search(const KeyBatch &kb, const MemRunTab &tab, const MemOut &out, hipStream_t s);
// status may be sst itself; source may be null.
hipError_t launch_get_join(const uint8_t *mem, const uint8_t *sst, uint64_t n, uint8_t *status, uint8_t *source,
                           hipStream_t s);

// seb_memwrite.hip: the memtable's write side (lsm/lsm.go:97-137, lsm/wal.go:31-65, lsm/memtable.go:34-93): a Put /
// Delete batch framed as WAL records, MemTable.size's change for a new run, and up to kMemRuns runs folded into one.
constexpr uint32_t kWriteTile = 1024;  // ops per tile of the frame's scan, slots per tile of the fold's sums and emit
constexpr uint32_t kScanWidth = 128;   // tiles per stretch of the scan over the tiles' sums (a carry between stretches)
uint64_t frame_scratch_bytes(uint64_t n);  // device scratch of launch_frame_plan
// n >= 1.  rec_off: n + 1 device u64.  Synchronises the stream; *image_bytes_host = the image's size; *err_host =
// op << 1 | (0: its key offsets, 1: its value offsets) of the least bad op, all ones for none.
hipError_t launch_frame_plan(const KeyBatch &kb, const uint64_t *val_off, const uint8_t *deleted, uint64_t *rec_off,
                             void *scratch, uint64_t *image_bytes_host, uint64_t *err_host, hipStream_t s);
// n >= 1, image_bytes >= 1.  Writes image[0, image_bytes) with every CRC field 0; nothing else is written.
hipError_t launch_frame_emit(const KeyBatch &kb, const uint8_t *vals, const uint64_t *val_off, const uint8_t *deleted,
                             uint64_t first_seq, const uint64_t *rec_off, uint8_t *image, uint64_t image_bytes,
                             hipStream_t s);
// *delta (device) = MemTable.size's change when `fresh` (pre unused) goes in front of tab's runs.
hipError_t launch_size_delta(const MemRun &fresh, const MemRunTab &tab, int64_t *delta, hipStream_t s);
struct FoldTab {  // passed by value (kernel arguments)
    MemRunTab tab;
    const uint8_t *vals[kMemRuns];  // run r's value bytes
    uint64_t val_bytes[kMemRuns];
    uint64_t begin[kMemRuns + 1];   // run r's entries are [begin[r], begin[r+1]) of the union
};
// The fold's plan lives in a caller-provided workspace: a 128-byte header, the tiles' three sums, a 16-byte slot
// per entry of the union.
struct FoldWs {
    uint64_t bytes, tiles, sums, slots;
};
FoldWs fold_ws_layout(uint64_t entries);
// entries >= 1, < 2^32.  Synchronises; sizes_host = one seb_fold_sizes; *err_host = the least run whose val_off[n]
// passes its val_bytes, all ones for none.
hipError_t launch_fold_plan(const FoldTab &tab, uint64_t entries, void *ws, void *sizes_host, uint64_t *err_host,
                            hipStream_t s);
// *ok = the workspace's header is the plan's that returned `sizes`; reads the header back.
hipError_t fold_ws_check(const void *sizes, const void *ws, bool *ok, hipStream_t s);
hipError_t launch_fold_emit(const FoldTab &tab, const void *sizes, const void *ws, uint8_t *keys, uint64_t *key_off,
                            uint8_t *vals, uint64_t *val_off, uint8_t *deleted, uint64_t *seq, hipStream_t s);

// seb_getpath.hip: the Get path (lsm/lsm.go:144-166): the keys the memtables leave undecided compacted into a dense
// batch with a row map, and the SSTables' answers for those keys joined back onto their batch rows.  The plan lives
// in a caller-provided workspace: a 128-byte header, then the tiles' two sums.
constexpr uint32_t kGetTile = 1024;  // keys per tile of the compaction's sums and emit
uint64_t compact_ws_bytes(uint64_t n);
// n >= 1, n < 2^32.  Synchronises the stream; sizes_host = one seb_compact_sizes.
hipError_t launch_compact_plan(const KeyBatch &kb, const uint8_t *mem_status, void *ws, void *sizes_host, hipStream_t s);
// sizes: one seb_compact_sizes with n == kb.n >= 1; nothing is written unless ws holds the plan that returned it, and
// nothing past row[undecided), out_off[undecided] and out_keys[key_bytes) in any case.  out_off is used only where
// kb has offsets.
hipError_t launch_compact_emit(const KeyBatch &kb, const uint8_t *mem_status, const void *sizes, const void *ws,
                               uint8_t *out_keys, uint64_t *out_off, uint32_t *row, hipStream_t s);
// Two launches in stream order: a lane per batch key, then a lane per row.  Nullable: mem_vloc, mem_vlen, sst_col,
// sst_vloc, sst_vlen, source, col, vloc, vlen.
hipError_t launch_get_join_rows(const uint8_t *mem_status, const uint64_t *mem_vloc, const uint32_t *mem_vlen, uint64_t n,
                                const uint32_t *row, uint64_t m, const uint8_t *sst_status, const uint16_t *sst_col,
                                const uint64_t *sst_vloc, const uint32_t *sst_vlen, uint8_t *status, uint8_t *source,
                                uint16_t *col, uint64_t *vloc, uint32_t *vlen, hipStream_t s);

// seb_values.hip: the Get path's last step (lsm/sstable.go:276-278, lsm/lsm.go:146-180): the found keys' values
// gathered back to back in batch order, with an offset array.  The plan lives in a caller-provided workspace: a
// 128-byte header, the tiles' two sums, then 13 bytes per key that the emit's first kernel leaves for its second.
constexpr uint32_t kValTile = 1024;       // keys per tile of the sums and of the offsets
constexpr uint32_t kValCopyGrid = 8192;   // the copy's workgroups (4 KiB of output each) before they stride
struct ValuesArg {  // device pointers; vals[r] / val_bytes[r] for r < num_runs <= kMemRuns; run nullable (read as 0)
    const uint8_t *status, *source, *run;
    const uint64_t *vloc;
    const uint32_t *vlen;
    uint64_t n;
    const uint8_t *vals[kMemRuns];
    uint64_t val_bytes[kMemRuns];
    uint32_t num_runs;
    const uint8_t *pool;
    uint64_t pool_bytes;
};
uint64_t values_ws_bytes(uint64_t n);
// n >= 1, n < 2^32.  Synchronises the stream; sizes_host = one seb_values_sizes; *bad_host = the lowest invalid
// carrying key, or ~0 where there is none (with one, the sizes hold n alone).
hipError_t launch_values_plan(const ValuesArg &a, void *ws, void *sizes_host, uint64_t *bad_host, hipStream_t s);
// sizes: one seb_values_sizes with n == a.n >= 1; nothing is written unless ws holds the plan that returned it, and
// nothing past out_off[n] and out_vals[val_bytes) in any case.  No copy is launched where val_bytes == 0.
hipError_t launch_values_emit(const ValuesArg &a, const void *sizes, void *ws, uint64_t *out_off, uint8_t *out_vals,
                              hipStream_t s);

// seb_blockids.hip: the block-id step between the locate and the block search (the rules: seb_blockids.h).  The
// miss path's plan lives in a caller-provided workspace: a 128-byte header, an open-addressing table of the smallest
// power of two >= 2 * max_uniq slots (pair u64, least cell index u32, rank u32), then the tiles' sums.
constexpr uint32_t kBidTile = 1024;  // cells per tile of the first-appearance sums and ranks
// the bound the table is sized by: max_uniq, or cells where that is less
uint64_t blockids_max_uniq(uint64_t cells, uint64_t max_uniq);
uint64_t blockids_ws_bytes(uint64_t cells, uint64_t max_uniq);
// cells >= 1, < 2^32.  One kernel; counts (nullable, three device u64: resident, misses, bad) is cleared on the
// stream first.
hipError_t launch_blockids_resident(const uint16_t *cand, const uint64_t *blocks, uint64_t cells, const uint32_t *res_first,
                                    const uint32_t *res_count, uint32_t res_slots, uint32_t *bid, uint64_t *counts,
                                    hipStream_t s);
// cells >= 1, < 2^32.  Synchronises the stream; sizes_host = one seb_blockids_sizes; *overflow = the table filled
// (sizes' uniq is then max_uniq + 1, not a count).
hipError_t launch_blockids_plan(const uint16_t *cand, const uint64_t *blocks, uint64_t cells, const uint32_t *res_first,
                                const uint32_t *res_count, uint32_t res_slots, uint64_t max_uniq, void *ws,
                                void *sizes_host, bool *overflow, hipStream_t s);
// sizes: one seb_blockids_sizes; nothing is written unless ws holds the plan that returned it, and nothing outside
// bid[cells), uniq_slot[uniq) and uniq_block[uniq) in any case.
hipError_t launch_blockids_emit(const uint16_t *cand, const uint64_t *blocks, uint64_t cells, const uint32_t *res_first,
                                const uint32_t *res_count, uint32_t res_slots, uint64_t max_uniq, uint32_t id_base,
                                const void *sizes, const void *ws, uint32_t *bid, uint16_t *uniq_slot, uint64_t *uniq_block,
                                hipStream_t s);

// seb_hashindex.hip: the hash index's read side (the semantics: seb_hashindex.h).  The table: a 64-byte header
// [overflow][occupied slots][bad records] and hidx_slots(capacity) slots of one u64 (0 empty, else a hash tag in the
// high 16 bits and record offset + 1 in the low 48).  hash_mask: the test-only option (0 = off).
uint64_t hidx_slots(uint64_t capacity);  // the smallest power of two >= 2 * capacity
uint64_t hidx_table_bytes(uint64_t capacity);
hipError_t launch_hidx_clear(void *table, uint64_t capacity, hipStream_t s);
// ok[n], valid[nseg] (device) and live[n] (nullable) from rec_off[n] and seg_first[nseg + 1] (device).
hipError_t launch_seg_verify(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, uint64_t n,
                             const uint64_t *seg_first, uint64_t nseg, uint8_t *ok, uint64_t *valid, uint8_t *live,
                             hipStream_t s);
hipError_t launch_hidx_insert(void *table, uint64_t capacity, const uint8_t *pool, uint64_t pool_bytes,
                              const uint64_t *rec_off, const uint8_t *live, uint64_t n, uint64_t hash_mask, hipStream_t s);
// Synchronises the stream; state_host = the header's three words.
hipError_t launch_hidx_state(const void *table, uint64_t state_host[3], hipStream_t s);
// rec, vloc, vlen and source are nullable; nothing outside the kb.n elements of each is written.
hipError_t launch_hidx_get(const void *table, uint64_t capacity, const uint8_t *pool, uint64_t pool_bytes, const KeyBatch &kb,
                           bool verify, uint64_t hash_mask, uint8_t *status, uint64_t *rec, uint64_t *vloc, uint32_t *vlen,
                           uint8_t *source, hipStream_t s);

// k_seg_crc's seal mode: the checksum of every record rec_off names that lies inside pool[0, pool_bytes) goes into
// its CRC field.
hipError_t launch_seg_seal(uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, uint64_t n, hipStream_t s);

// seb_hashwrite.hip: the hash index's write side (the semantics: seb_hashwrite.h).
uint64_t segframe_scratch_bytes(uint64_t n, uint64_t cut_cap);  // device scratch of launch_segframe_plan
// n >= 1, limit >= 1.  rec_off: n + 1 device u64.  Synchronises the stream; out_host = [the least bad op << 2 | (0 key
// offsets, 1 value offsets, 2 empty key, 3 keySize + valueSize), all ones for none][the image's size][the cuts'
// count]; cut_host (HOST memory of min(cut_cap, n) entries, nullable) receives the first min(cut_cap, n, count) cuts
// (entries behind them may be written too).
hipError_t launch_segframe_plan(const KeyBatch &kb, const uint64_t *val_off, const uint8_t *deleted, uint64_t active_size,
                                uint64_t limit, uint64_t *rec_off, uint64_t *cut_host, uint64_t cut_cap, void *scratch,
                                uint64_t out_host[3], hipStream_t s);
// n >= 1, image_bytes >= 1.  Writes the sealed image[0, image_bytes); nothing else is written.
hipError_t launch_segframe_emit(const KeyBatch &kb, const uint8_t *vals, const uint64_t *val_off, const uint8_t *deleted,
                                uint64_t timestamp, const uint64_t *rec_off, uint8_t *image, uint64_t image_bytes,
                                hipStream_t s);
// The compaction's plan lives in a caller-provided workspace: a 64-byte header, a scratch key table of capacity n,
// the tiles' two sums, then per record its output offset, a survivor's source offset and its mark.
struct SegCompactWs {
    uint64_t bytes, tiles, table, sums, pos, src, mark;
};
SegCompactWs segcompact_ws_layout(uint64_t n);
// n >= 1, < 2^38.  Synchronises; out_host = [the least live record outside the pool, all ones for none][live records]
// [distinct keys][survivors][tombstoned keys][image bytes][the scratch table overflowed][winning records].
hipError_t launch_segcompact_plan(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, const uint8_t *live,
                                  uint64_t n, uint64_t hash_mask, void *ws, uint64_t out_host[8], hipStream_t s);
// Nothing is written unless ws holds the plan that returned (survivors, image_bytes), and nothing outside
// image[0, image_bytes) and out_rec_off[0, survivors] in any case.  survivors == 0: only out_rec_off[0].
hipError_t launch_segcompact_emit(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, uint64_t n,
                                  uint64_t timestamp, uint64_t survivors, uint64_t image_bytes, void *ws, uint8_t *image,
                                  uint64_t *out_rec_off, hipStream_t s);
// dst[0, n) = src[i] - sub + add (all ones where src[i] < sub), dst[n] = end
hipError_t launch_offsets_shift(const uint64_t *src, uint64_t n, uint64_t sub, uint64_t add, uint64_t *dst, uint64_t end,
                                hipStream_t s);
// Synchronises; *sum_host = keySize + valueSize over the records the table names; sum_dev: 8 bytes of device scratch.
hipError_t launch_hidx_logical(const void *table, uint64_t capacity, const uint8_t *pool, uint64_t pool_bytes,
                               uint64_t *sum_dev, uint64_t *sum_host, hipStream_t s);

// The B-tree's read side (seb_btree.hip).  The check's workspace: bt_check_ws_bytes(num_pages) bytes,
// 16-byte aligned.  launch_bt_check synchronises the stream (a read-back per level round, one for the counts) and
// fills *stats_host; kind and level are nullable.  launch_bt_get: leaf, pos, vloc, vlen and source are nullable;
// nothing outside the kb.n elements of each is written.
struct BtStats;
uint64_t bt_check_ws_bytes(uint32_t num_pages);
hipError_t launch_bt_check(const uint8_t *image, uint32_t num_pages, uint32_t root, uint8_t *kind, uint8_t *level, void *ws,
                           BtStats *stats_host, hipStream_t s);
hipError_t launch_bt_get(const uint8_t *image, uint32_t num_pages, uint32_t root, const KeyBatch &kb, uint8_t *status,
                         uint32_t *leaf, uint32_t *pos, uint64_t *vloc, uint32_t *vlen, uint8_t *source, hipStream_t s);

// The B-tree's range scans (seb_btscan.hip).  The directory's workspace: bt_dir_ws_bytes(num_pages)
// bytes, 16-byte aligned; launch_bt_dir_build synchronises (a read-back per level) and fills *info_host, or *rule_host
// (seb_btree.h's kDir*, 0 for none) and *page_host where it refuses; dir: bt_dir_bytes(num_pages) bytes, 8-byte aligned.
// The scan's plan lives in a workspace of bt_scan_ws_bytes(ranges) bytes, 8-byte aligned: a 256-byte header, first_r,
// range_off, the tiles' sums.  launch_bt_scan_plan (ranges >= 1) synchronises; launch_bt_scan_cells writes nothing
// unless ws holds the plan of (ranges, entries), and nothing outside range_off[ranges + 1] and the entries' elements.
struct BtDirInfo;
uint32_t bt_dir_tile();
uint64_t bt_dir_ws_bytes(uint32_t num_pages);
hipError_t launch_bt_dir_build(const uint8_t *image, uint32_t num_pages, uint32_t root, const uint8_t *kind, const uint8_t *level,
                               uint8_t *dir, void *ws, BtDirInfo *info_host, int *rule_host, uint32_t *page_host, hipStream_t s);
uint64_t bt_scan_ws_bytes(uint64_t ranges);
hipError_t bt_scan_read_dir(const uint8_t *dir, uint8_t head_host[32], hipStream_t s);
hipError_t launch_bt_scan_plan(const uint8_t *image, uint32_t num_pages, uint32_t root, const uint8_t *dir, const KeyBatch &starts,
                               const KeyBatch &ends, uint64_t limit, void *ws, uint8_t *range_status, uint64_t *entries_host,
                               hipStream_t s);
hipError_t launch_bt_scan_cells(const uint8_t *image, uint32_t num_pages, uint32_t root, const uint8_t *dir, uint64_t ranges,
                                uint64_t entries, const void *ws, uint64_t *range_off, uint8_t *status, uint8_t *source,
                                uint64_t *kloc, uint32_t *klen, uint64_t *vloc, uint32_t *vlen, hipStream_t s);

// Process-wide tuning knobs (seb_set_option): the auto-dispatch thresholds, the build algorithm,
// and the few shape choices tests force to cover both paths.  Variants measured slower were
// removed from the kernels (DESIGN.md 8 keeps their numbers).
struct Options {
    int build_algo = 0;           // 0 auto, 1 device-scope atomics, 2 radix-partitioned (bucketed), 3 LDS-resident
                                  // filter (atomic merge), 4 LDS images + OR kernel
    int multi_interleave = 1;     // multi-filter probe: interleaved table when filters share (m, k)
    int multiget_order = 1;       // MultiGet: probe batches of >= 64K keys in key-range order (1: aligned 16-B keys
                                  // sorted within chunks and read through segment tables; 2: moved across the
                                  // batch by a scatter pass, round 5's form) or in batch order (0)
    int multiget_l0_group = 1;    // MultiGet: L0 files of one (m, k) tested through one interleaved table
    int multiget_xcd = 1;         // MultiGet: the blocks sharing an XCD walk one contiguous eighth of the batch
                                  // (1, default: 575 vs 596 us per 10M-key k_multiget on 28 files), or not (0)
    int probe_compact = 1;        // phased probe from keys: later phases read only the live keys' words
    int scatter_bins = 1;         // bucketed build, k == 7: scatter through fixed LDS bins, pipelined against the
                                  // hashing (1), or the counting sort (0)
    uint64_t varlen_prehash_min_keys = 1u << 16;  // LDS-staged pre-hash from this many var-length keys
    uint64_t bucket_min_keys = 100000;  // auto: bucketed build from this many keys on
    uint64_t lds_min_keys = 75000;      // auto: LDS-resident build (filter <= 160 KiB) from this many keys on
    uint32_t many_splits = 0;     // batched small-filter build: workgroups per filter (0 = auto, one per CU)
    int probe_phases = 0;         // phased probe: number of filter ranges (0 = one per 4 MiB of filter)
    unsigned grid_cap = 1u << 20; // grid-stride kernels: most workgroups per launch
    uint64_t workspace_limit_mib = 0;  // library scratch cap (0 = none); a larger request fails SEB_ERR_NOMEM
    uint64_t multiget_piece_mib = 1024;  // registry MultiGet: a key-range ordered walk's scratch per piece of the batch
    int varlen_tail = 1;          // pre-hash: the 64 * v longest keys of a workgroup of 512 - 64 * v keys on
                                  // 2 * v waves of 32 keys, a lane per chain (v = 1, 2, 3), or one key per
                                  // lane throughout (0, measured slower: DESIGN.md 5.5)
    int cpu_fallback = 1;         // Go API mirror: a build/probe whose device path fails (SEB_ERR_DEVICE/NOMEM)
                                  // is done on the filter's host copy instead (seb_fallback_count)
    int fault_inject = 0;         // test only: the Go API mirror's device path fails with SEB_ERR_DEVICE
    uint64_t hidx_hash_mask = 0;  // test only: the hash index's key hash is AND-ed with it (0 = off), so that many
                                  // keys share a home slot and a tag
};
Options &options();

// The grid of a 256-lane grid-stride launch over `items` >= 1: a workgroup per 256 items, at most `most` of them and
// at most options().grid_cap (seb_blockids.hip, seb_hashindex.hip, seb_hashwrite.hip, seb_btree.hip, seb_btscan.hip, seb_values.hip's
// copy and seb_codec.hip's k_route, whose ceiling is 65,536).  The default grid_cap lies above every ceiling, so a
// default launch has min(ceil(items / 256), most) workgroups; a test sets grid_cap to 1 or 2 and the kernels' loops
// take many trips on a small input.  Only for kernels whose workgroups never wait for one another.
constexpr unsigned kStreamBlocks = 4096;  // most workgroups of a grid-stride launch
inline unsigned stream_grid(uint64_t items, unsigned most = kStreamBlocks) {
    const uint64_t b = (items + 255) / 256;
    const unsigned cap = most < options().grid_cap ? most : options().grid_cap;
    return (unsigned)(b < cap ? (b ? b : 1) : cap);
}

hipError_t launch_build(const KeyBatch &kb, uint32_t *words, const ModArg &md, hipStream_t s);
// Copy `bytes` of filter words to host-pinned memory (both 16-B aligned) with a kernel.
hipError_t launch_copy_out(const uint32_t *words, uint8_t *host, uint64_t bytes, hipStream_t s);
// Zero `bytes` (a multiple of 16) of filter words.
hipError_t launch_clear_words(uint32_t *words, uint64_t bytes, hipStream_t s);
bool bucketed_supported(uint64_t m, uint32_t k);
uint64_t bucketed_workspace_bytes(uint64_t n, uint64_t m, uint32_t k);
// Build from packed residues (k == 7, m < 2^kPackBits); same workspace as launch_build_bucketed.
// ovf != null: a fresh build: `words` (seb_words_bytes) need no clear and are written whole;
// `ovf` is an all-zero bitmap of the same size, left all zero again.
hipError_t launch_build_bucketed_packed(const uint64_t *packed, uint64_t n, uint32_t *words, const ModArg &md,
                                        void *ws, uint64_t ws_bytes, hipStream_t s, uint32_t *ovf = nullptr);
hipError_t launch_build_bucketed(const KeyBatch &kb, uint32_t *words, const ModArg &md, void *ws, uint64_t ws_bytes,
                                 hipStream_t s, uint32_t *ovf = nullptr);
// 1 = atomic, 2 = bucketed, 3 = LDS-resident (atomic merge), 4 = LDS images + OR kernel, for a
// batch of n keys into an m-bit filter.
int choose_build_algo(uint64_t n, uint64_t m, uint32_t k);
// The image build (algo 4): scratch bytes, and the launch.  fresh: the filter words hold nothing
// yet, so they are written rather than OR-ed (and need no clear beforehand).
uint64_t image_workspace_bytes(uint64_t n, uint64_t m);
hipError_t launch_build_images(const KeyBatch &kb, uint32_t *words, const ModArg &md, void *ws, uint64_t ws_bytes,
                               bool fresh, hipStream_t s);
hipError_t launch_probe(const KeyBatch &kb, const uint32_t *words, const ModArg &md, uint8_t *out, hipStream_t s);
hipError_t launch_probe_multi(const KeyBatch &kb, const MultiArg &ma, void *mask, uint32_t mask_bytes,
                              hipStream_t s);
// Pre-hash a variable-length batch into one uint4 (h1, h2) per key (LDS-staged byte walk).
hipError_t launch_hash_varlen(const KeyBatch &kb, uint4 *hashes, hipStream_t s);
// The same pre-hash writing packed residues for filter md (k == 7, m < 2^kPackBits) instead.
hipError_t launch_hash_varlen_packed(const KeyBatch &kb, const ModArg &md, uint64_t *packed, hipStream_t s);

// Interleaved multi-filter probe (all filters share (m, k), k == 7, m < 2^31): scratch bytes
// needed for the per-call table (0 = not applicable), and the launch (table in `ws`).
uint64_t interleaved_bytes(const MultiArg &ma, uint32_t mask_bytes);
hipError_t launch_probe_interleaved(const KeyBatch &kb, const MultiArg &ma, void *mask, uint32_t mask_bytes, void *ws,
                                    hipStream_t s);
// The same over packed residues (all filters share (m, k), k == 7, m < 2^kPackBits); `ws` holds
// the table (interleaved_table_bytes).
hipError_t launch_probe_interleaved_packed(const uint64_t *packed, uint64_t n, const MultiArg &ma, void *mask,
                                           uint32_t mask_bytes, void *ws, hipStream_t s);
hipError_t launch_build_many_lds(const KeyBatch &kb, const ManyArg &ma, uint32_t lds_bytes, hipStream_t s);

// Packed residues (k == 7, m < 2^kPackBits): 8 bytes per key instead of the key itself.
constexpr uint32_t kPackBits = 29;
hipError_t launch_pack_residues(const KeyBatch &kb, const ModArg &md, uint64_t *packed, hipStream_t s);
// Narrow packed residues (k == 7, m < 2^kPack6Bits, e.g. the 958,506-bit compaction filters): the
// same three fields in 48 bits (21-bit r0, 21-bit b, 6 carries), 6 bytes per key, stored in blocks
// of 64 keys (64 u32 low words, then 64 u16 high words: kPack6Block bytes), so a wave moves a block
// with two coalesced loads and a slice starting at a multiple of 64 keys is one contiguous range.
constexpr uint32_t kPack6Bits = 21;
constexpr uint32_t kPack6Block = 384;
constexpr uint64_t packed6_bytes(uint64_t n) { return ((n + 63) / 64) * kPack6Block; }
hipError_t launch_pack_residues6(const KeyBatch &kb, const ModArg &md, uint8_t *packed6, hipStream_t s);
hipError_t launch_probe_interleaved_packed6(const uint8_t *packed6, uint64_t n, const MultiArg &ma, void *mask,
                                            uint32_t mask_bytes, void *ws, hipStream_t s);
// out[w] = OR over s < nslices of in[s * slice_words + w] (the sharded build's reduction step)
hipError_t launch_or_slices(const uint32_t *in, uint32_t nslices, uint64_t slice_words, uint32_t *out, hipStream_t s);
hipError_t launch_probe_packed(const uint64_t *packed, uint64_t n, const uint32_t *words, const ModArg &md,
                               uint8_t *out, hipStream_t s);
// Phased probe (the default for k == 7, m < 2^kPackBits, 4-byte aligned out): one launch per word
// range of the filter (probe_phase_count of them); `packed` is 8*n bytes of scratch.
uint64_t probe_phase_count(uint64_t m);
// kb == nullptr: probe the packed words themselves (no phase 0 hashing).
hipError_t launch_probe_phased(const KeyBatch *kb, uint64_t n, const uint32_t *words, const ModArg &md, uint8_t *out,
                               uint64_t *packed, hipStream_t s);
// The phased probe from keys with compacted later phases (probe_compact_bytes of 16-B aligned
// scratch in `ws`; needs probe_phase_count(m) >= 2).
uint64_t probe_compact_bytes(uint64_t n);
hipError_t launch_probe_compact(const KeyBatch &kb, const uint32_t *words, const ModArg &md, uint8_t *out, void *ws,
                                hipStream_t s);
// The same from a variable-length batch, phase 0 fused into the LDS-staged pre-hash.
hipError_t launch_probe_compact_varlen(const KeyBatch &kb, const uint32_t *words, const ModArg &md, uint8_t *out,
                                       void *ws, hipStream_t s);
hipError_t launch_hash_varlen_phase0(const KeyBatch &kb, const ModArg &md, const uint32_t *words, uint64_t *rows,
                                     ulonglong2 *recs, uint32_t hi, hipStream_t s);
// The same from a batch of packed residues (the pre-hashed variable-length batch, a broadcast batch).
hipError_t launch_probe_compact_packed(const uint64_t *packed, uint64_t n, const uint32_t *words, const ModArg &md,
                                       uint8_t *out, void *ws, hipStream_t s);
// Probe from keys that also writes the batch's packed residues.
hipError_t launch_probe_emit(const KeyBatch &kb, const uint32_t *words, const ModArg &md, uint8_t *out,
                             uint64_t *packed, hipStream_t s);

}  // namespace seb
