/*
 * seb_bloom.h — C ABI of the MI355X-native bloom-filter build + probe path.
 *
 * Drop-in boundary for intellect4all/storage-engines lsm/bloom.go.  The reference is Go; its
 * callers are lsm/sstable_builder.go:30,53,217 (build at flush/compaction) and
 * lsm/sstable.go:129,206 (decode at open, probe on Get).  A cgo shim
 * (storage-engines_amd/go/lsm/bloom.go) binds the "Go API mirror" group
 * below one-for-one, so those callers compile unchanged.  Every entry point takes plain C types
 * (pointers and sizes); no torch or HIP types appear in a signature (streams are `void*`
 * holding a hipStream_t, NULL = the library's own stream / the null stream).
 *
 * Results are bit-exact with the reference: identical bit array (byte h>>3, bit h&7 — on the
 * little-endian device this is u32 word h>>5, bit h&31) and identical MayContain answers.
 *
 * Errors: every int-returning function returns SEB_OK (0) or a negative SEB_ERR_* code, and
 * seb_last_error() gives a thread-local message.  The reference has no error returns (bad input
 * panics or yields nil); the Go shim turns a negative code into the same panic.  The Go API
 * mirror (seb_filter_*) does not fail for want of a device: a build or batched probe whose device
 * path returns SEB_ERR_DEVICE / SEB_ERR_NOMEM is done on the filter's host copy instead (option
 * "cpu_fallback", default on), counted by seb_fallback_count(), the first one per process also
 * logged to stderr.  SEB_ERR_INTERNAL (a failed launch, a kernel fault) is never absorbed.  The
 * fallback needs the filter's host copy to be current: a filter over 64 MiB of bits whose device
 * copy is ahead of it (built on the device with the host mirror off) reports the error instead.
 * Every other entry point (device-resident, host-buffer, registry) reports the error.
 */
#ifndef SEB_BLOOM_H
#define SEB_BLOOM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEB_ABI_VERSION 1

enum seb_status {
    SEB_OK = 0,
    SEB_ERR_INVALID = -1, /* bad argument; the reference would panic (e.g. % 0, index out of range) */
    SEB_ERR_DEVICE = -2,  /* no usable gfx950 device: none, no driver, no code object, runtime down */
    SEB_ERR_NOMEM = -3,   /* host or device allocation failed (or over workspace_limit_mib) */
    SEB_ERR_RANGE = -4,   /* sizing outside the reference's defined float->int range */
    SEB_ERR_SHORT = -5,   /* a decoded filter's bits are shorter than ceil(numBits/8) */
    SEB_ERR_INTERNAL = -6, /* any other HIP error: a rejected launch, a kernel fault, a library bug */
};

/* A batch of keys.  Fixed-length keys: offsets == NULL, key i = data[i*stride, (i+1)*stride).
 * Variable-length keys: offsets holds n+1 non-decreasing byte offsets (offsets[0] may be != 0),
 * key i = data[offsets[i], offsets[i+1]).  Host or device memory per the entry point. */
typedef struct seb_keys {
    const uint8_t *data;
    const uint64_t *offsets;
    uint64_t n;
    uint32_t stride;
    uint32_t reserved; /* must be 0 */
} seb_keys;

/* One filter for the multi-filter probe.  `bits` is host bytes (ceil(num_bits/8)) for
 * seb_probe_multi and device u32 words (seb_words_bytes(num_bits) bytes) for
 * seb_dev_probe_multi. */
typedef struct seb_filter_ref {
    const void *bits;
    uint64_t num_bits;
    uint32_t num_hashes;
    uint32_t reserved; /* must be 0 */
} seb_filter_ref;

/* ---------------------------------------------------------------- sizing (host only) ---- */

/* m and k exactly as NewBloomFilter computes them (lsm/bloom.go:19-31): float64 Go math.Log,
 * const-folded Ln2*Ln2, Ceil, k forced to >= 1.  n == 0 gives m = 0, k = 1 (as in Go). */
int seb_params(int64_t expected_keys, double false_positive_rate, uint64_t *num_bits,
               uint32_t *num_hashes);
/* ceil(m/8): the reference's len(bits) (lsm/bloom.go:34). */
uint64_t seb_num_bytes(uint64_t num_bits);
/* Bytes of the device word array for m bits: ceil(m/128)*16 (u32 words, 16-B padded, pad = 0). */
uint64_t seb_words_bytes(uint64_t num_bits);

int seb_abi_version(void);
/* Process-wide tuning knobs (results never change, only speed):
 *   "build_algo"      0 auto, 1 device-scope atomic OR, 2 radix-partitioned LDS build, 3 the whole
 *                     filter in one CU's LDS (word array <= 160 KiB), keys split over workgroups
 *                     (atomic merge), 4 LDS images of the whole filter + an OR kernel (<= 160 KiB)
 *                     Auto: 4 from lds_min_keys keys while the word array fits 160 KiB (3 when
 *                     the words are not 16-B aligned), 2 from bucket_min_keys keys for larger
 *                     filters, 1 below those
 *   "bucket_min_keys" auto build_algo: radix-partitioned from this many keys on
 *   "lds_min_keys"    auto build_algo: LDS-resident filter (<= 160 KiB) from this many keys on
 *   "many_splits"     batched small-filter build: workgroups per filter (0 = auto)
 *   "probe_phases"    k == 7, m < 2^29 probes: filter ranges of the phased probe, one launch each
 *                     (0 = one per 4 MiB of filter; 1 = the single-launch sliced probe)
 *   "probe_compact"   phased probe: later phases read only the live keys' packed words, kept
 *                     compacted per 64-key group (1, default), or every key's (0)
 *   "scatter_bins"    radix-partitioned build, k == 7, 512-2275 buckets (m ~ 33.5M-149M bits):
 *                     positions placed through fixed per-bucket LDS bins, the claims pipelined
 *                     against the hashing (1, default), or by a counting sort (0)
 *   "multi_interleave" multi-filter probes with shared (m, k): bit-transposed table (0/1)
 *   "multiget_order"  registry MultiGet walks batches of >= 64K keys in key-range order (1, default:
 *                     aligned 16-B keys sorted by bucket within 4096-key super-chunks and read
 *                     through segment tables; 2: moved across the batch by a scatter pass) or batch order (0)
 *   "multiget_piece_mib" registry MultiGet: a batch whose key-range order would need more scratch
 *                     than this (MiB, default 1024) is walked in pieces of whole 2048-key chunks
 *   "multiget_l0_group" registry MultiGet tests the L0 files that share (m, k) through one
 *                     bit-interleaved table, one gather per position for all of them (1, default)
 *   "multiget_xcd"    registry MultiGet: the workgroups that share an XCD walk one contiguous eighth of
 *                     the (key-range ordered) batch, so each XCD's L2 holds its own stretch's filters
 *                     (1, default), or blocks walk the batch in launch order (0)
 *   "varlen_prehash_min_keys"  variable-length batches of this many keys are pre-hashed in LDS
 *   "varlen_tail"     pre-hash: v = 1 (default), 2, 3: workgroups of 512 - 64 v keys whose 64 v longest
 *                     keys run on 2 v waves of 32 keys, one lane per FNV chain; 0: 448 keys, one key per
 *                     lane throughout
 *   "grid_cap"        maximum workgroups of the grid-stride kernels
 *   "workspace_limit_mib"  cap on library scratch and a context's build scratch (0 = none); a
 *                     request above it fails with SEB_ERR_NOMEM (MultiGet's key-range order then
 *                     falls back to batch order; the Go API mirror's build to its CPU fallback)
 *   "cpu_fallback"    Go API mirror: on a device failure build / probe on the host copy (1, default)
 *                     or return the error (0)
 *   "fault_inject"    test only: the Go API mirror's device path fails with SEB_ERR_DEVICE (1) or
 *                     SEB_ERR_INTERNAL (2), or not (0)
 *   "hidx_hash_mask"  test only: the hash index's key hash is AND-ed with it before the home slot and the tag are
 *                     taken (0, default: off), so that many keys share both and the key compare and long probe
 *                     chains are reached; set it before the table's first insert and keep it for its Gets
 * Environment variables SEB_<NAME> (upper case) set the initial values. */
int seb_set_option(const char *name, int64_t value);
int seb_get_option(const char *name, int64_t *value);
const char *seb_last_error(void);
/* 0 if a gfx950 device is usable, else SEB_ERR_DEVICE (message in seb_last_error). */
int seb_device_check(int device);

/* ------------------------------------------------- device-resident entry points ---------- */
/* All pointers are device memory; work is enqueued on `stream` and NOT synchronised.
 * seb_dev_build ORs the keys into `words` (clear first with seb_dev_clear for a fresh filter),
 * the device form of the reference's Add loop (sstable_builder.go:53 -> bloom.go:70-77). */
int seb_dev_clear(uint32_t *words, uint64_t num_bits, void *stream);
int seb_dev_build(const seb_keys *keys, uint32_t *words, uint64_t num_bits, uint32_t num_hashes,
                  void *stream);
/* A new filter from `keys` (NewBloomFilter + Add per key): `words` (seb_words_bytes) need not be
 * cleared; every word is written.  The radix-partitioned build and the LDS image build write them
 * whole instead of clearing and OR-ing; other build paths clear first.  Device builds take word
 * arrays aligned to 4 B; 16-B aligned ones (any hipMalloc / torch allocation) take the 16-B
 * clear and the image build, others hipMemsetAsync and the LDS-filter build. */
int seb_dev_build_fresh(const seb_keys *keys, uint32_t *words, uint64_t num_bits, uint32_t num_hashes,
                        void *stream);
/* Same, with caller-owned scratch (graph-capture friendly: no allocation inside the call).
 * seb_dev_build_workspace_size gives the bytes needed for n keys (0: this build needs none). */
uint64_t seb_dev_build_workspace_size(uint64_t n, uint64_t num_bits, uint32_t num_hashes);
int seb_dev_build_ws(const seb_keys *keys, uint32_t *words, uint64_t num_bits, uint32_t num_hashes,
                     void *workspace, uint64_t workspace_bytes, void *stream);
/* out[i] = MayContain(key i) as 0/1 bytes (bloom.go:82-92; Go []bool layout). */
int seb_dev_probe(const seb_keys *keys, const uint32_t *words, uint64_t num_bits, uint32_t num_hashes,
                  uint8_t *out, void *stream);
/* Packed residues, for one probe batch shared by several filters of the same (num_bits, num_hashes)
 * (multi-GPU: hash once on the root, broadcast 8 bytes per key instead of the key).  Requires
 * num_hashes == 7 and num_bits < 2^29.  packed[i] = r0 | b << 29 | carries << 58 with
 * r0 = hash1 mod m, b = hash2 mod m and bit q-1 of carries set when hash1 + q*hash2 wraps 2^64 at
 * step q (q = 1..6); seb_dev_probe_packed gives the answers seb_dev_probe gives for the keys
 * (MayContain of lsm/bloom.go:82-92). */
int seb_dev_pack_residues(const seb_keys *keys, uint64_t num_bits, uint32_t num_hashes, uint64_t *packed,
                          void *stream);
int seb_dev_probe_packed(const uint64_t *packed, uint64_t n, const uint32_t *words, uint64_t num_bits,
                         uint32_t num_hashes, uint8_t *out, void *stream);
/* Multi-filter probe of packed residues (seb_dev_probe_multi's mask layout); every filter must
 * have the packed batch's (num_bits, num_hashes). */
int seb_dev_probe_multi_packed(const uint64_t *packed, uint64_t n, const seb_filter_ref *filters, uint32_t num_filters,
                               void *mask, uint32_t mask_bytes, void *stream);
/* Narrow packed residues (6 bytes per key) for num_hashes == 7 and num_bits < 2^21, e.g. the
 * compaction-sized filters of lsm/compaction.go:253,286 (m = 958,506): the same three fields as
 * seb_dev_pack_residues at 21 / 21 / 6 bits, v = r0 | b << 21 | carries << 42, stored in blocks of
 * 64 keys (key i in block i / 64): 64 little-endian u32 low words, then 64 u16 high halves, 384
 * bytes per block; the buffer holds seb_packed6_bytes(n) bytes and must be 4-byte aligned.  A slice
 * of the batch that starts at a multiple of 64 keys is the contiguous byte range from its first
 * block, so a batch split in 64-key multiples travels as plain byte ranges (a quarter fewer bytes
 * over xGMI than the 8-byte form).  seb_dev_probe_multi_packed6 gives the masks
 * seb_dev_probe_multi gives for the keys. */
uint64_t seb_packed6_bytes(uint64_t n);
int seb_dev_pack_residues6(const seb_keys *keys, uint64_t num_bits, uint32_t num_hashes, void *packed6, void *stream);
int seb_dev_probe_multi_packed6(const void *packed6, uint64_t n, const seb_filter_ref *filters, uint32_t num_filters,
                                void *mask, uint32_t mask_bytes, void *stream);
/* seb_dev_probe plus the batch's packed residues in one pass (the broadcast root's probe). */
int seb_dev_probe_emit_packed(const seb_keys *keys, const uint32_t *words, uint64_t num_bits, uint32_t num_hashes,
                              uint8_t *out, uint64_t *packed, void *stream);
/* Multi-filter probe: bit f of mask[i] = MayContain of filters[f] on key i.  mask_bytes is the
 * width of one mask element (1, 2, 4 or 8) and must cover num_filters bits (<= 64). `filters`
 * is a HOST array whose .bits are device word arrays. */
int seb_dev_probe_multi(const seb_keys *keys, const seb_filter_ref *filters, uint32_t num_filters,
                        void *mask, uint32_t mask_bytes, void *stream);
/* Batched build of many independent filters in one launch (compaction output files,
 * lsm/compaction.go:286): keys [key_begin[f], key_begin[f+1]) of `keys` go into filter f.
 * `filters` is a HOST array whose .bits are device word arrays (cleared by the caller);
 * key_begin is a HOST array of num_filters+1 entries. */
int seb_dev_build_many(const seb_keys *keys, const uint64_t *key_begin, const seb_filter_ref *filters,
                       uint32_t num_filters, void *stream);

/* Sharded build of one filter: every rank ORs its key shard into a partial filter,
 * an all-to-all hands rank g the G partials of word slice g (slice after slice), and this call
 * ORs them: out[w] = OR_s slices[s * slice_words + w].  RCCL has no bitwise-OR reduction, so the
 * reduce step of the exchange runs here.  Device pointers; out may not overlap slices. */
int seb_dev_or_slices(const uint32_t *slices, uint32_t num_slices, uint64_t slice_words, uint32_t *out, void *stream);

/* Small device/stream helpers for hosts without their own HIP binding (ctypes, cgo). */
int seb_dev_alloc(void **ptr, uint64_t bytes);
int seb_dev_free(void *ptr);
int seb_host_alloc(void **ptr, uint64_t bytes); /* pinned host memory */
int seb_host_free(void *ptr);
int seb_memcpy_h2d(void *dst, const void *src, uint64_t bytes, void *stream);
int seb_memcpy_d2h(void *dst, const void *src, uint64_t bytes, void *stream);
int seb_stream_sync(void *stream);
/* Timing events created with hipEventDisableSystemFence: a default event's completion fence
 * writes back and invalidates L2 (~15 us between two kernels on gfx950).  elapsed waits for
 * `end`; use only for timing, not to order host reads after device writes. */
int seb_timer_create(void **event);
int seb_timer_record(void *event, void *stream);
int seb_timer_elapsed_ms(void *start, void *end, float *ms);
int seb_timer_destroy(void *event);

/* Library-owned scratch.  Entry points that need scratch and take no workspace argument use
 * grow-only buffers kept per (device, stream); a call holds its stream's buffers until it returns,
 * so calls from several threads on one stream are safe (their launches do not interleave).
 * seb_workspace_bytes: bytes currently held; seb_workspace_release: synchronise the streams that
 * own scratch and free all of it (the next call re-allocates).  A phased probe holds ≈8.3 bytes per
 * key (its compacted packed words and group records); a key-range ordered registry MultiGet
 * 20 bytes per key of aligned 16-B keys (bucket ids, run starts, the moved keys) or 8 for keys it
 * reads through an index, plus its answers in sorted rows (8 bytes per key for masks, 2 per slot for
 * candidate rows); the scratch of a context's (or a registry's) own streams is freed by
 * seb_ctx_destroy (seb_registry_free). */
uint64_t seb_workspace_bytes(void);
int seb_workspace_release(void);

/* ------------------------------------------- host-buffer batched entry points ------------ */
/* Keys and bits in host memory: H2D, kernels and D2H on the context's streams, synchronous.
 * A context owns a device, streams and grow-only scratch buffers; one context per thread
 * (contexts are cheap; calls on one context are serialised by a lock). */
typedef struct seb_ctx seb_ctx;
int seb_ctx_create(int device, seb_ctx **out);
void seb_ctx_destroy(seb_ctx *ctx);

#define SEB_BUILD_FRESH 1u /* `bits` is output only: start from an all-zero filter */
/* bits: ceil(num_bits/8) host bytes, OR-accumulated (or written fresh with SEB_BUILD_FRESH). */
int seb_build(seb_ctx *ctx, const seb_keys *keys, uint8_t *bits, uint64_t num_bits, uint32_t num_hashes,
              uint32_t flags);
int seb_probe(seb_ctx *ctx, const seb_keys *keys, const uint8_t *bits, uint64_t num_bits,
              uint32_t num_hashes, uint8_t *out);
int seb_probe_multi(seb_ctx *ctx, const seb_keys *keys, const seb_filter_ref *filters, uint32_t num_filters,
                    uint64_t *mask);

/* ----------------------------------- Go API mirror (lsm/bloom.go, one call per Go method) ---- */
/* A filter handle.  Its bit array lives in HBM (device-resident filter registry); a host copy is
 * materialised on Encode.  Add() defers: keys are appended to a host arena and built in one
 * batched launch at the next Encode / MayContain / flush (or when the arena passes a size cap).
 * All functions are thread-safe; MayContain may be called concurrently on one filter. */
typedef struct seb_filter seb_filter;

/* NewBloomFilter(expectedKeys, falsePositiveRate)          lsm/bloom.go:19   (NULL + last_error
 * when the sizing leaves the defined range, where Go's behaviour is implementation-defined) */
seb_filter *seb_filter_new(int64_t expected_keys, double false_positive_rate);
void seb_filter_free(seb_filter *f);
/* (*BloomFilter).Add(key)                                    lsm/bloom.go:70 */
int seb_filter_add(seb_filter *f, const uint8_t *key, uint64_t len);
int seb_filter_add_batch(seb_filter *f, const seb_keys *keys);
/* (*BloomFilter).MayContain(key) -> 1 / 0, or < 0 on error  lsm/bloom.go:82 */
int seb_filter_may_contain(seb_filter *f, const uint8_t *key, uint64_t len);
int seb_filter_may_contain_batch(seb_filter *f, const seb_keys *keys, uint8_t *out);
/* (*BloomFilter).Encode() -> 12 + len(bits) bytes           lsm/bloom.go:96 */
uint64_t seb_filter_encoded_size(seb_filter *f);
int seb_filter_encode(seb_filter *f, uint8_t *out, uint64_t cap);
/* DecodeBloomFilter(data) -> NULL when len < 12 (Go: nil)   lsm/bloom.go:105 */
seb_filter *seb_filter_decode(const uint8_t *data, uint64_t len);
/* Accessors and an explicit flush of deferred Adds. */
uint64_t seb_filter_num_bits(const seb_filter *f);
uint32_t seb_filter_num_hashes(const seb_filter *f);
uint64_t seb_filter_pending(seb_filter *f);
int seb_filter_flush(seb_filter *f);
/* How many Go-API-mirror builds / batched probes ran on the host copy because the device path
 * failed (the "cpu_fallback" option); 0 on a healthy GPU. */
uint64_t seb_fallback_count(void);
/* Registry MultiGets (seb_registry_multiget*) that ran in batch order because the key-range
 * order's scratch could not be had (SEB_ERR_NOMEM under "workspace_limit_mib" or the device): the
 * answers are the same, only slower; a benchmark reports it to show which path it measured. */
uint64_t seb_multiget_order_fallbacks(void);

/* ------------------ device-resident filter registry + batched LSM lookup ---- */
/* One registry per LSM instance.  seb_registry_put decodes an SSTable's bloom block (the bytes
 * OpenSSTable reads, lsm/sstable.go:121-129) straight into HBM, with the file's level and
 * [MinKey, MaxKey]; level 0 keeps insertion order, levels 1..4 are ordered by MinKey, as
 * lsm/levels.go:45-63 keeps them.  seb_registry_remove frees it (compaction, lsm/compaction.go).
 * seb_registry_multiget: for each key, bit s of maybe[i] is set when registry slot s is a file
 * LSM.Get would consult for the key (every L0 file; per level 1..4 the first file whose range
 * covers it, lsm/lsm.go:168-198) AND its filter may contain the key; the mask form needs every slot
 * < 64 (a registry that never held more than 64 files).  The list form takes any registry (up to
 * 4096 files, u16 slot ids): row i of cand (cap u16 per key) lists the slots of those files in the
 * order Get visits them (L0 in insertion order, then levels 1..4), padded with 0xFFFF; cap must be
 * >= seb_registry_max_candidates (the L0 file count + the number of non-empty levels 1..4). */
typedef struct seb_registry seb_registry;
seb_registry *seb_registry_new(int device);
void seb_registry_free(seb_registry *reg);
/* returns the slot (>= 0) or < 0 */
int seb_registry_put(seb_registry *reg, uint64_t file_num, int level, const uint8_t *bloom, uint64_t bloom_len,
                     const uint8_t *min_key, uint64_t min_len, const uint8_t *max_key, uint64_t max_len);
int seb_registry_remove(seb_registry *reg, uint64_t file_num);
/* file number and level of every slot (UINT64_MAX / -1 for free slots); returns the file count */
int seb_registry_slots(seb_registry *reg, uint64_t *file_nums, int32_t *levels, uint32_t cap);
int seb_registry_multiget(seb_registry *reg, const seb_keys *keys, uint64_t *maybe);          /* host keys */
int seb_registry_multiget_dev(seb_registry *reg, const seb_keys *keys, uint64_t *maybe, void *stream);
int seb_registry_max_candidates(seb_registry *reg); /* >= 0, or < 0 on error */
int seb_registry_multiget_list(seb_registry *reg, const seb_keys *keys, uint16_t *cand, uint32_t cap); /* host */
int seb_registry_multiget_list_dev(seb_registry *reg, const seb_keys *keys, uint16_t *cand, uint32_t cap,
                                   void *stream);
/* The list form with file numbers instead of slots (host keys): files[i*cap + j] is the file_num of
 * the j-th file Get would read for key i, padded with UINT64_MAX.  Sizing, lookup and slot->file
 * mapping happen under one hold of the registry lock, so a concurrent put/remove (flush,
 * compaction) cannot make rows overflow or a reused slot name the wrong file.  *need (nullable)
 * receives the row width the registry needs now; cap < *need returns SEB_ERR_RANGE (retry). */
int seb_registry_multiget_files(seb_registry *reg, const seb_keys *keys, uint64_t *files, uint32_t cap,
                                uint32_t *need);

/* ------------- sparse indexes + batched block locator (SSTable.Get's index step, lsm/sstable.go:210-222) ---- */
/* Once a file's filter says "maybe", SSTable.Get bisects the file's sparse index (one entry per 4 KiB
 * data block, lsm/sstable_builder.go:113-117) for the key and reads the block of the last entry whose
 * key is <= the key; a key below the first entry is "not found" without a read.  The registry keeps
 * each file's index in HBM next to its filter and answers that for every cell of a MultiGet's
 * candidate rows, so a key batch becomes (file, block offset) pairs: all readBlock needs. */
#define SEB_NO_BLOCK UINT64_MAX

/* Host only.  Walk an encoded index block ([numEntries u32] then per entry [keySize u32][blockOffset u64]
 * [key], little-endian) as decodeIndex does (lsm/sstable.go:168-201); *entries (nullable) = numEntries.
 * SEB_ERR_SHORT where decodeIndex fails ("index too small": len < 4; "index truncated": an entry's
 * 12-byte header or its key runs past the end); bytes after the last entry are ignored, as there.
 * ONE DEPARTURE from the reference: SEB_ERR_INVALID when the keys are not non-decreasing in Go string
 * order.  decodeIndex accepts such a block, but sort.Search's answer on it depends on its probe
 * sequence, and SSTableBuilder never writes one; refusing it leaves the device layout free.  Equal
 * neighbours are accepted: the answer is then the last of them, as an upper bound gives. */
int seb_index_scan(const uint8_t *index, uint64_t index_len, uint64_t *entries);
/* Attach the index block OpenSSTable reads (lsm/sstable.go:105-119) to a registered file; validated
 * by the same walk (its errors), SEB_ERR_INVALID for an unknown file or a file that has one already.
 * numEntries == 0 is a valid index: every key gets SEB_NO_BLOCK.  Released with the file's filter by
 * seb_registry_remove / seb_registry_free. */
int seb_registry_put_index(seb_registry *reg, uint64_t file_num, const uint8_t *index, uint64_t index_len);
int seb_registry_index_entries(seb_registry *reg, uint64_t file_num, uint64_t *entries);
/* cand: n x cap u16 rows exactly as seb_registry_multiget_list* writes them (slots in visiting order,
 * 0xFFFF padding).  blocks[i*cap + j] = the BlockOffset of the last index entry of slot cand[i*cap + j]
 * whose key is <= key i, or SEB_NO_BLOCK when there is none (blockIdx == 0), the cell is padding, or it
 * names a free or out-of-range slot (never read out of bounds).  Every registered file must have its
 * index: else SEB_ERR_INVALID naming the file.  cap == 0 or a null argument: SEB_ERR_INVALID; n == 0:
 * SEB_OK, nothing launched.  The _dev form takes device pointers and is not synchronised. */
int seb_registry_locate_dev(seb_registry *reg, const seb_keys *keys, const uint16_t *cand, uint32_t cap,
                            uint64_t *blocks, void *stream);
int seb_registry_locate(seb_registry *reg, const seb_keys *keys, const uint16_t *cand, uint32_t cap,
                        uint64_t *blocks);
/* The read plan (host keys): seb_registry_multiget_files plus blocks[i*cap + j], the block offset to
 * read in files[i*cap + j] (SEB_NO_BLOCK: no read, and for the UINT64_MAX padding).  Same cap / *need /
 * SEB_ERR_RANGE retry contract; lookup, locate and the slot->file mapping under one hold of the lock. */
int seb_registry_multiget_blocks(seb_registry *reg, const seb_keys *keys, uint64_t *files, uint64_t *blocks,
                                 uint32_t cap, uint32_t *need);

/* ------------- batched data-block search: SSTable.Get's last step + LSM.Get's decision over a key's files ---- */
/* With the block to read known per cell, SSTable.Get reads it and walks it for the key (searchBlock,
 * lsm/sstable.go:242-290); LSM.Get takes the first file, in visiting order, that answers "found" or fails
 * (lsm/lsm.go:174-197).  The caller reads the blocks (the library reads no file) into a block pool; this
 * group searches every cell's block for its key and resolves each key's row of cells.
 *
 * A block image is [numEntries u32] then per entry [keySize u32][valueSize u32][deleted u8][key][value],
 * little-endian, at most SEB_BLOCK_BYTES bytes (readBlock returns block[:n], n <= 4096).  The walk, bit-exact:
 * fewer than 4 bytes: not found.  For each of numEntries entries: a 9-byte header or a key + value that runs
 * past the image is the error "block truncated" (sizes added in 64 bits, as Go's int does; nothing wraps); an
 * entry equal to the key answers (deleted == 1 exactly: a tombstone; any other byte: the value); an entry
 * greater than the key in Go string order ends the walk with "not found".  The first entry in walk order that
 * does one of the three decides; nothing checks that the block is sorted, so an unsorted block, duplicate
 * keys and a wrong numEntries are answered by the walk (an equal entry behind a greater one is never reached,
 * the first duplicate wins, an overstated count walks into the zero padding as empty-key entries).
 *
 * A TOMBSTONE INSIDE AN SSTABLE DOES NOT END LSM.Get: sst.Get returns found == false for it
 * (sstable.go:273-275), so lsm.go:175-181,187-196 go on to the next, older file, and a value there is
 * returned.  seb_dev_resolve_rows does the same; the cell status tells a caller that wants otherwise.
 *
 * Block pool: caller-owned memory of num_blocks slots of SEB_BLOCK_BYTES bytes; block b is
 * pool[b * 4096, b * 4096 + blen[b]) with blen[b] <= 4096 (a larger blen is read as 4096); the base must be
 * 16-byte aligned.  The pool may persist across calls (a device block cache); the library never allocates or
 * copies it.  A cell names its block by id: bid[i * cap + j], or SEB_NO_BLOCK_ID for "no read".
 * A cell's result is one u32, status << 28 | voff << 13 | vlen: voff = the value's byte offset inside the
 * block (0..4096), vlen its size (<= 4083), both 0 unless the status is SEB_CELL_FOUND. */
#define SEB_BLOCK_BYTES 4096u
#define SEB_NO_BLOCK_ID UINT32_MAX
enum seb_cell_status {
    SEB_CELL_NONE = 0,      /* the id is SEB_NO_BLOCK_ID or >= num_blocks: nothing was read */
    SEB_CELL_MISS = 1,      /* not found */
    SEB_CELL_FOUND = 2,     /* the value is block[voff, voff + vlen) */
    SEB_CELL_TOMBSTONE = 3, /* the key's entry is deleted */
    SEB_CELL_TRUNC = 4,     /* searchBlock's error "block truncated" */
};
#define SEB_CELL(status, voff, vlen) ((uint32_t)(status) << 28 | (uint32_t)(voff) << 13 | (uint32_t)(vlen))
#define SEB_CELL_STATUS(cell) ((uint32_t)(cell) >> 28)
#define SEB_CELL_VOFF(cell) (((uint32_t)(cell) >> 13) & 0x1FFFu)
#define SEB_CELL_VLEN(cell) ((uint32_t)(cell) & 0x1FFFu)
enum seb_get_status { SEB_GET_MISS = 0, SEB_GET_FOUND = 1, SEB_GET_ERROR = 2 };

/* Host only: the walk above for one block image and one key.  len > 4096 or a null pointer with a non-zero
 * length: SEB_ERR_INVALID.  "block truncated" is a cell status, not an error code. */
int seb_block_search(const uint8_t *block, uint64_t len, const uint8_t *key, uint64_t key_len, uint32_t *cell);
/* Device pointers, not synchronised.  cells[c] for each of the n * cap cells = seb_block_search of pool block
 * bid[c] and key c / cap (SEB_CELL_NONE for an id that names no block; nothing is read for it).  Keys in every
 * seb_keys layout.  n == 0: SEB_OK, nothing launched; cap == 0, a null argument or a pool that is not 16-byte
 * aligned: SEB_ERR_INVALID.  Nothing past the n * cap cells is written. */
int seb_dev_search_blocks(const seb_keys *keys, const uint32_t *bid, uint32_t cap, const uint8_t *pool,
                          const uint16_t *blen, uint32_t num_blocks, uint32_t *cells, void *stream);
/* Device pointers, not synchronised.  Per key, the deciding cell is the first of its row's cap cells whose
 * status is SEB_CELL_FOUND or SEB_CELL_TRUNC: status[i] = SEB_GET_FOUND / SEB_GET_ERROR, or SEB_GET_MISS when
 * there is none (tombstones do not decide, see above); col[i] = its column, 0xFFFF for none;
 * vloc[i] = bid * 4096 + voff, the value's byte offset in the pool, and vlen[i] its size, both 0 unless
 * found.  col, vloc and vlen may be null. */
int seb_dev_resolve_rows(const uint32_t *cells, const uint32_t *bid, uint64_t n, uint32_t cap, uint8_t *status,
                         uint16_t *col, uint64_t *vloc, uint32_t *vlen, void *stream);
/* The host-buffer form on a context: keys, bid (n * cap), pool (num_blocks * 4096 bytes) and blen in host
 * memory; H2D, both kernels, D2H; synchronous.  status is required; col, vloc, vlen and cells (the n * cap cell
 * results) may be null. */
int seb_search_blocks(seb_ctx *ctx, const seb_keys *keys, const uint32_t *bid, uint32_t cap, const uint8_t *pool,
                      const uint16_t *blen, uint32_t num_blocks, uint8_t *status, uint16_t *col, uint64_t *vloc,
                      uint32_t *vlen, uint32_t *cells);
/* Host only: seb_registry_multiget_blocks' parallel (file, block offset) arrays into the read list.  Each
 * distinct pair once, in first-appearance order, in uniq_files / uniq_blocks (uniq_cap entries each), and
 * bid[c] = its position for every cell; a cell whose block is SEB_NO_BLOCK gets SEB_NO_BLOCK_ID.  The same
 * offset in two files is two blocks.  *num_uniq = the number of distinct pairs; uniq_cap below it:
 * SEB_ERR_RANGE (nothing in bid or uniq_* is then meaningful; retry with *num_uniq). */
int seb_blocks_dedup(const uint64_t *files, const uint64_t *blocks, uint64_t cells, uint32_t *bid,
                     uint64_t *uniq_files, uint64_t *uniq_blocks, uint64_t uniq_cap, uint64_t *num_uniq);

/* ------------- block ids: a located cell (slot, block offset) into an id of the block pool ---- */
/* The step between seb_registry_locate_dev and seb_dev_search_blocks, on the cells as the list and the locate
 * write them: cand[c] (u16 slot, 0xFFFF padding) and blocks[c] (u64, SEB_NO_BLOCK for none), c < cells = n * cap;
 * a cell does not depend on its row.  cells >= 2^32 is SEB_ERR_INVALID.
 *
 * Residency table (nullable; res_slots == 0 without one): slot s is RESIDENT when s < res_slots and res_first[s]
 * != SEB_NO_BLOCK_ID; its data section then lies in the pool as blocks res_first[s] .. res_first[s] +
 * res_count[s] - 1 (what the device builder and the merge leave behind).
 *
 * Per cell, in this order:
 *   1. cand == 0xFFFF or blocks == SEB_NO_BLOCK (either one): bid = SEB_NO_BLOCK_ID.
 *   2. an offset >= 2^48: bid = SEB_NO_BLOCK_ID, counted in `bad` (no file is 256 TiB; the device packs
 *      (slot, offset) into one 64-bit word).
 *   3. a resident slot: with q = offset / 4096, bid = res_first[s] + q where offset % 4096 == 0, q < res_count[s]
 *      and the sum is below 2^32 - 1; otherwise SEB_NO_BLOCK_ID, counted in `bad`: nothing is ever read for it.
 *   4. otherwise a MISS: bid = id_base + r, r = the rank of the cell's (slot, offset) pair among the distinct miss
 *      pairs in order of first appearance by cell index.  uniq_slot[r] (u16) and uniq_block[r] (u64) are the read
 *      list: the caller reads block r into pool block id_base + r.  id_base + uniq > 2^32 - 1: SEB_ERR_INVALID.
 * The same offset in two slots is two blocks.  With no residency table and file numbers for slots, bid and the
 * read list are seb_blocks_dedup's, element for element.  The caller owns the pool and chooses id_base. */
typedef struct seb_blockids_sizes {
    uint64_t cells;
    uint64_t resident; /* cells that rule 3 gave an id */
    uint64_t misses;   /* cells of rule 4 */
    uint64_t uniq;     /* distinct miss pairs: the read list's length */
    uint64_t bad;      /* cells refused by rule 2 or 3 */
    uint64_t reserved; /* 0 */
} seb_blockids_sizes;

/* Host only, and the reference for the device forms.  *sizes is filled whenever the arguments are valid.  bid,
 * uniq_slot and uniq_block all NULL: the sizes only (uniq_cap and id_base are not looked at).  Otherwise uniq_cap <
 * uniq is SEB_ERR_RANGE with *sizes filled for the retry and nothing else meaningful; then bid (where cells != 0)
 * and uniq_slot / uniq_block (where uniq != 0) are required.  Writes bid[0, cells), uniq_slot[0, uniq) and
 * uniq_block[0, uniq) and nothing else.  SEB_ERR_INVALID: a NULL required pointer (sizes; cand and blocks where
 * cells != 0; res_first and res_count where res_slots != 0), cells >= 2^32, id_base + uniq > 2^32 - 1.
 * cells == 0 is valid. */
int seb_block_ids(const uint16_t *cand, const uint64_t *blocks, uint64_t cells, const uint32_t *res_first,
                  const uint32_t *res_count, uint32_t res_slots, uint32_t id_base, uint32_t *bid, uint16_t *uniq_slot,
                  uint64_t *uniq_block, uint64_t uniq_cap, seb_blockids_sizes *sizes);

/* Device pointers (blocks, uniq_block and counts 8-byte aligned, res_first, res_count and bid 4-byte aligned, cand
 * and uniq_slot 2-byte aligned; else SEB_ERR_INVALID).  Not synchronised.  One kernel that applies rules 1-3 to
 * every cell; a miss cell gets SEB_NO_BLOCK_ID.  counts (nullable): three u64 of device memory, set by the call
 * to resident, misses and bad as in seb_blockids_sizes (cleared on the stream, then one add per wave).  This is the
 * whole step for a tree whose files are all resident (misses == 0).  cells == 0: nothing is launched, counts is
 * not written, SEB_OK.  Writes bid[0, cells) and counts[0, 3) and nothing else. */
int seb_dev_block_ids_resident(const uint16_t *cand, const uint64_t *blocks, uint64_t cells, const uint32_t *res_first,
                               const uint32_t *res_count, uint32_t res_slots, uint32_t *bid, uint64_t *counts,
                               void *stream);

/* Every rule on device pointers (aligned as above), as the Get path's plan / emit pair; `sizes` is HOST memory.
 * max_uniq is the caller's bound on the distinct miss pairs: the number of blocks in the files that are not
 * resident is a good one, and `cells` always suffices (a larger value counts as `cells`).  The workspace
 * (seb_dev_block_ids_workspace_size(cells, max_uniq) bytes of device memory, 16-byte aligned, opaque; 0 for cells
 * >= 2^32) holds a table of the smallest power of two >= 2 * max_uniq slots; it carries the plan to the emit and
 * must not be touched in between.
 * seb_dev_block_ids_plan SYNCHRONISES and fills *sizes.  More than max_uniq distinct miss pairs: SEB_ERR_RANGE;
 * sizes->misses (with resident and bad) is exact, sizes->uniq is some value above max_uniq (exact unless the table
 * filled), and a retry with max_uniq = sizes->misses cannot fail this way.  A table that fills ends the probes; no
 * lane ever waits for another.
 * seb_dev_block_ids_emit (not synchronised; the same inputs, max_uniq and workspace) writes bid[0, cells),
 * uniq_slot[0, uniq) and uniq_block[0, uniq) and nothing else.  No output depends on the hash or on scheduling.
 * SEB_ERR_INVALID and nothing launched: a NULL required pointer (sizes; cand, blocks and the workspace where cells
 * != 0; res_first and res_count where res_slots != 0; for the emit bid, and uniq_slot / uniq_block where uniq != 0),
 * cells >= 2^32, a misaligned pointer, a workspace below seb_dev_block_ids_workspace_size (plan); for the emit
 * sizes->cells != cells, sizes->uniq above max_uniq or above sizes->misses, resident + misses + bad > cells, or
 * id_base + uniq > 2^32 - 1.  cells == 0: nothing is launched or written, SEB_OK (the plan sets *sizes to zeros and
 * needs no workspace).
 * Write bounds, whatever the inputs hold: the workspace's header carries a magic word, cells, the table size,
 * max_uniq and the plan's totals; where they do not match `sizes` the emit writes nothing.  Where the inputs changed
 * between plan and emit the outputs may be wrong, but every store stays inside the three ranges above. */
uint64_t seb_dev_block_ids_workspace_size(uint64_t cells, uint64_t max_uniq);
int seb_dev_block_ids_plan(const uint16_t *cand, const uint64_t *blocks, uint64_t cells, const uint32_t *res_first,
                           const uint32_t *res_count, uint32_t res_slots, uint64_t max_uniq, void *workspace,
                           uint64_t workspace_bytes, seb_blockids_sizes *sizes, void *stream);
int seb_dev_block_ids_emit(const uint16_t *cand, const uint64_t *blocks, uint64_t cells, const uint32_t *res_first,
                           const uint32_t *res_count, uint32_t res_slots, uint64_t max_uniq, uint32_t id_base,
                           const seb_blockids_sizes *sizes, const void *workspace, uint32_t *bid, uint16_t *uniq_slot,
                           uint64_t *uniq_block, void *stream);

/* ------------- batched SSTable builder: data blocks, index block, metadata and the file image ---- */
/* What SSTableBuilder computes between its Write calls (lsm/sstable_builder.go:42-135,185-290), for a sorted
 * run that is already in memory: entry i has key i of `keys`, value vals[val_off[i], val_off[i+1]) (n + 1
 * non-decreasing offsets, val_off[0] may be != 0) and the flag deleted[i] (any non-zero byte is "deleted";
 * deleted == NULL: none).  The library writes no file; the order of the entries is never checked.
 *
 * Entry image: [keySize u32][valueSize u32][deleted u8 = 1 or 0][key][value], little-endian,
 * e = 9 + keySize + valueSize bytes.  A block is [numEntries u32] then its entries.  The cut is greedy: before
 * an entry is appended, a block of more than 4 bytes that the entry would take past 4096 is flushed.  With P
 * the 64-bit prefix sum of e, the block that starts at entry s ends before the smallest t > s with
 * 4 + (P[t+1] - P[s]) > 4096; entry s always belongs to it.  A flushed block shorter than 4096 bytes is zero
 * padded to 4096; its index entry is (its first key, the offset it was written at).  An entry with
 * 4 + e > 4096 ("oversized") is a block of its own, longer than 4096 bytes and written unpadded, and every
 * later block offset of the file stops being a multiple of 4096 (the reference cannot read such a block back,
 * but the bytes it writes are defined, and the host half writes them).
 *
 * Finish: the index block [numEntries u32] then per block [keySize u32][blockOffset u64][key]; the metadata
 * [minKeySize u32][maxKeySize u32][minKey][maxKey] with min / max = the first and the last key added (8 zero
 * bytes for an empty file); the filter's Encode(); the 28-byte footer [indexOffset u64][bloomOffset u64]
 * [metadataOffset u64][0x5354424C u32].  A file without entries is a 4-byte index, 8 bytes of metadata, the
 * empty filter and the footer.
 *
 * With no oversized entry the data section is the block pool of the block search above: block b at
 * b * 4096, its true length in a u16 array, so a block is searchable the moment it is written. */
typedef struct seb_sst_sizes {
    uint64_t num_blocks;       /* data blocks = index entries */
    uint64_t data_bytes;       /* the data section: 4096 per block, more for an oversized one */
    uint64_t index_bytes;      /* 4 + per block 12 + its first key's length */
    uint64_t meta_bytes;       /* 8 + the first and the last key's lengths */
    uint64_t oversize_entries; /* entries with 4 + e > 4096 */
} seb_sst_sizes;
#define SEB_SST_FOOTER_BYTES 28u
#define SEB_SST_MAGIC 0x5354424Cu

/* Host only: one file.  seb_sst_plan sizes the three sections; seb_sst_encode writes them (a capacity below
 * the section's size: SEB_ERR_RANGE, nothing meaningful written; *sizes, nullable, is filled either way) and
 * is the reference for the device form, the path for files the device refuses and what a caller without a GPU
 * uses.  A key or a value of 2^32 bytes or more, or decreasing offsets: SEB_ERR_INVALID. */
int seb_sst_plan(const seb_keys *keys, const uint64_t *val_off, seb_sst_sizes *sizes);
int seb_sst_encode(const seb_keys *keys, const uint8_t *vals, const uint64_t *val_off, const uint8_t *deleted,
                   uint8_t *data, uint64_t data_cap, uint8_t *index, uint64_t index_cap, uint8_t *meta,
                   uint64_t meta_cap, seb_sst_sizes *sizes);
int seb_sst_footer(uint64_t index_offset, uint64_t bloom_offset, uint64_t metadata_offset, uint8_t *out28);

/* Device pointers, many files in one call (a compaction's output files, lsm/compaction.go:253): file f holds
 * entries [file_begin[f], file_begin[f+1]) of the batch; file_begin is a HOST array of num_files + 1
 * non-decreasing entries from 0 to keys->n.  Keys in every seb_keys layout, any byte alignment; n < 2^32.
 * The workspace (seb_dev_sst_workspace_size bytes of device memory, 16-byte aligned, opaque) carries the plan
 * from the first call to the second and must not be touched in between.
 * seb_dev_sst_plan runs the cut for every file, SYNCHRONISES the stream and fills the host array
 * sizes[num_files], so the caller can allocate the outputs.
 * seb_dev_sst_encode (not synchronised; `sizes` as the plan returned them) writes every file's data section
 * back to back (file f at the sum of the earlier data_bytes, so block b of the call at b * 4096), blen
 * (nullable): each block's true length as the pool's u16, the index blocks back to back and the metadata back
 * to back.  Outputs need not be cleared (the zero padding is written) and nothing is written outside the
 * stated sizes; `data` must be 16-byte aligned.  The device never writes a block longer than 4096 bytes: a
 * file with oversize_entries > 0 makes encode return SEB_ERR_RANGE naming the file (use the host half).
 * Files of 0 entries (0 blocks, a 4-byte index) and of 1 entry are valid; n == 0 launches nothing. */
uint64_t seb_dev_sst_workspace_size(uint64_t n, uint32_t num_files);
int seb_dev_sst_plan(const seb_keys *keys, const uint64_t *val_off, const uint64_t *file_begin, uint32_t num_files,
                     void *workspace, uint64_t workspace_bytes, seb_sst_sizes *sizes, void *stream);
int seb_dev_sst_encode(const seb_keys *keys, const uint8_t *vals, const uint64_t *val_off, const uint8_t *deleted,
                       const uint64_t *file_begin, uint32_t num_files, const seb_sst_sizes *sizes,
                       const void *workspace, uint64_t workspace_bytes, uint8_t *data, uint16_t *blen,
                       uint8_t *index, uint8_t *meta, void *stream);
/* The host-buffer form on a context: one file, host memory, synchronous.  `out` receives the complete file
 * image, byte-identical to what SSTableBuilder leaves on disk: data, index, metadata, the Encode() of
 * NewBloomFilter(expected_keys, 0.01) with every key added, the footer.  *need (nullable) = its size; cap
 * below it: SEB_ERR_RANGE (retry with *need, as seb_registry_multiget_blocks).  A file with an oversized entry
 * goes through the host half, the filter still through the device.  expected_keys == 0 with n > 0:
 * SEB_ERR_INVALID (the reference's Add would take a remainder by zero). */
int seb_sst_build(seb_ctx *ctx, const seb_keys *keys, const uint8_t *vals, const uint64_t *val_off,
                  const uint8_t *deleted, int64_t expected_keys, uint8_t *out, uint64_t cap, uint64_t *need);

/* ------------- batched compaction merge: k sorted runs of a block pool into one run for the builder ---- */
/* What mergeFiles computes before its builder (lsm/compaction.go:226-333): every input file's data blocks are
 * parsed (SSTableIterator.loadBlock, :69-124), the entries go through a k-way merge by key, duplicates are
 * skipped, and at targetLevel == 4 tombstones are dropped.  Input: the data sections of the input files as
 * runs of a block pool in the block search's layout (block b at pool + b * 4096, blen[b] bytes, a larger blen
 * read as 4096, base 16-byte aligned); run r is blocks [run_begin[r], run_begin[r+1]), run_begin a HOST array
 * of num_runs + 1 non-decreasing entries from 0 to num_blocks; a run's entries are its blocks' entries in
 * block order.  Output: one sorted run in the builder's input layout above.
 *
 * The decode is loadBlock's walk, bit-exact: fewer than 4 bytes: no entries.  From off = 4, for i < numEntries:
 * off + 9 > len ends the block; keySize, valueSize, deleted = (byte == 1) are read; off + 9 + keySize +
 * valueSize > len (64-bit sums) ends the block; both ends are silent (a break, not searchBlock's error).  An
 * overstated numEntries therefore walks into the zero padding as empty-key entries; a deleted byte of 2 or 255
 * is "not deleted".  A block yields at most 454 entries.
 *
 * The merge orders by key alone (every entry's Sequence is 0, :119): one entry per distinct key comes out, in
 * ascending Go string order; with SEB_MERGE_DROP_TOMBSTONES a surviving tombstone is then dropped (it still
 * shadows the older entries of its key: they do not resurface).
 *
 * ONE DEPARTURE FROM THE REFERENCE.  Of several entries with one key, the reference keeps whichever
 * container/heap's array order leaves for last (merge([[a],[a]]) keeps input 1; over random inputs the lowest,
 * the highest and a middle holder all occur): an accident of the heap, not a rule.  Here the entry of the
 * LOWEST-NUMBERED RUN survives; the caller orders the runs.  In mergeFiles' allFiles order (the L0 files, then
 * the overlapping files of the next level, :180,216) that is the file LSM.Get visits first (lsm.go:168-198).
 * The key sequence and the decode are bit-exact, and when no key occurs in two runs so is the whole output.
 *
 * Every run must be STRICTLY INCREASING in Go string order (true of anything a memtable flush or an earlier
 * merge wrote; the reference does not check it, and its output on such input is again heap-dependent).  Both
 * halves check it: the plan returns SEB_ERR_INVALID and seb_last_error names the lowest-numbered offending run
 * and its first entry that is not above its predecessor ("run R entry E", E counted inside the run).  Nothing
 * is read out of bounds on any input.  An overstated numEntries that reaches the padding ends as this error
 * unless the run's only key is the empty key.
 *
 * Output entry o: key keys[key_off[o], key_off[o+1]), value vals[val_off[o], val_off[o+1]), deleted[o] = 1
 * or 0; key_off[0] = val_off[0] = 0, entries_out + 1 offsets each: the seb_keys offset form + vals / val_off /
 * deleted that seb_dev_sst_plan, seb_dev_sst_encode and seb_dev_build_many take (file_begin[f] =
 * min(f * 100000, entries_out) is mergeFiles' file split, :253,301).  Nothing outside the sizes the plan
 * returned is written.  Limits: entries_in < 2^32, num_blocks < 2^32, num_runs <= SEB_MERGE_MAX_RUNS.
 * num_runs == 0, an empty pool, runs of 0 blocks and blocks of 0 entries are valid. */
#define SEB_MERGE_DROP_TOMBSTONES 1u /* targetLevel == 4 */
#define SEB_MERGE_MAX_RUNS 1048576u
typedef struct seb_merge_sizes {
    uint64_t entries_in, entries_out; /* decoded / surviving */
    uint64_t key_bytes, val_bytes;    /* of the survivors */
    uint64_t shadowed, dropped;       /* lost to a lower-numbered run / tombstones dropped */
} seb_merge_sizes;

/* Host only.  seb_block_entries: the decode above for one block image; entry_off[i] = the offset of entry i's
 * 9-byte header, *count = the entries found.  len > 4096: SEB_ERR_INVALID; cap < *count: SEB_ERR_RANGE with
 * *count filled (the first cap offsets are written).  seb_merge_plan sizes the output; seb_merge_emit (`sizes`
 * as the plan returned them; anything else: SEB_ERR_INVALID) writes it.  They are the reference for the device
 * form and what a caller without a GPU uses. */
int seb_block_entries(const uint8_t *block, uint64_t len, uint16_t *entry_off, uint32_t cap, uint32_t *count);
int seb_merge_plan(const uint8_t *pool, const uint16_t *blen, const uint64_t *run_begin, uint32_t num_runs,
                   uint32_t flags, seb_merge_sizes *sizes);
int seb_merge_emit(const uint8_t *pool, const uint16_t *blen, const uint64_t *run_begin, uint32_t num_runs,
                   uint32_t flags, uint8_t *keys, uint64_t *key_off, uint8_t *vals, uint64_t *val_off,
                   uint8_t *deleted, const seb_merge_sizes *sizes);

/* Device pointers (run_begin, run_entries and sizes are HOST memory).
 * seb_dev_merge_count: block_entries[b] (device, num_blocks u16) = block b's entry count; SYNCHRONISES and
 * fills run_entries[num_runs] (nullable), whose sum is the `entries` of the workspace size.
 * seb_dev_merge_plan (block_entries as count left them; workspace: seb_dev_merge_workspace_size bytes of device
 * memory, 16-byte aligned, opaque, too small: SEB_ERR_INVALID) decodes, checks the runs' order, merges, marks
 * the survivors, SYNCHRONISES and fills *sizes, so the caller can allocate the outputs.
 * seb_dev_merge_emit (not synchronised; the same pool and workspace, untouched in between; `sizes` as the plan
 * returned them) writes the five output arrays; keys and vals may have any byte alignment.  Before it launches
 * it reads the workspace's 128-byte header back (so it waits for what the stream already holds; nothing, right
 * after the plan): a workspace that does not hold the plan that returned `sizes` is SEB_ERR_INVALID and nothing
 * is written.  Nothing is launched when entries_in == 0. */
int seb_dev_merge_count(const uint8_t *pool, const uint16_t *blen, uint32_t num_blocks, const uint64_t *run_begin,
                        uint32_t num_runs, uint16_t *block_entries, uint64_t *run_entries, void *stream);
uint64_t seb_dev_merge_workspace_size(uint64_t entries, uint32_t num_blocks, uint32_t num_runs);
int seb_dev_merge_plan(const uint8_t *pool, const uint16_t *blen, uint32_t num_blocks, const uint64_t *run_begin,
                       uint32_t num_runs, const uint16_t *block_entries, uint32_t flags, void *workspace,
                       uint64_t workspace_bytes, seb_merge_sizes *sizes, void *stream);
int seb_dev_merge_emit(const uint8_t *pool, const seb_merge_sizes *sizes, const void *workspace,
                       uint64_t workspace_bytes, uint8_t *keys, uint64_t *key_off, uint8_t *vals, uint64_t *val_off,
                       uint8_t *deleted, void *stream);
/* The host-buffer form on a context: pool (num_blocks * 4096 bytes), blen and the outputs in host memory;
 * H2D, count, plan, emit, D2H; synchronous.  key_cap / val_cap bytes and entry_cap entries (key_off and val_off
 * hold entry_cap + 1 offsets); a capacity below a size: SEB_ERR_RANGE with *sizes filled, so the caller can
 * retry (the seb_sst_build convention). */
int seb_merge(seb_ctx *ctx, const uint8_t *pool, const uint16_t *blen, uint32_t num_blocks, const uint64_t *run_begin,
              uint32_t num_runs, uint32_t flags, uint8_t *keys, uint64_t key_cap, uint64_t *key_off, uint8_t *vals,
              uint64_t val_cap, uint64_t *val_off, uint8_t *deleted, uint64_t entry_cap, seb_merge_sizes *sizes);

/* ------------- WAL replay: a log image into the memtable's sorted run for the builder ---- */
/* What recoverFromWAL leaves in the memtable (lsm/lsm.go:273-298) and what flushMemtable then hands to the
 * builder, GetAllEntries() (lsm/memtable.go:129-137, lsm/lsm.go:343-370), for a whole log image at once.
 * Input: a WAL image and its record boundaries as seb_wal_scan yields them: record i = data[rec_off[i],
 * rec_off[i+1]) = [crc u32][seq u64][keySize u32][valueSize u32][deleted u8][key][value], little-endian
 * (lsm/wal.go:31-62); the image may sit at any byte alignment.
 *
 * Every record goes through MemTable.Put or MemTable.Delete (lsm/memtable.go:34-93) in log order:
 *   - deleted = (byte == 1) (wal.go:114): a byte of 2 or 255 is a Put.
 *   - a Put makes the entry (key, value, seq, not deleted); a deleted record makes (key, NO VALUE, seq,
 *     deleted): Delete stores Value nil, so a deleted record's valueSize bytes do not come out.
 *   - a record of a key that is there replaces the whole entry (memtable.go:51-54, 82-85).  One entry per
 *     distinct key survives: that of the key's LAST RECORD IN LOG ORDER, even where an earlier record has the
 *     higher seq.  Tombstones stay, as entries with deleted = 1.
 *   - entries come out in ascending Go string order (bytewise, a key before its extensions); the empty key is
 *     a key like any other.
 *   - max_sequence = the maximum seq over ALL records, overwritten ones included (lsm.go:286-288); 0 for none.
 *   - memtable_size = MemTable.size after the replay = the sum over the survivors of keyLen + 16 + valueLen
 *     (valueLen 0 for a tombstone): Put and Delete keep it path independent (memtable.go:54,60,85,91).
 *   - recovery never flushes: a whole log is one run.
 * There is no departure from the reference: (key, record index) is a total order, so every output byte is
 * determined.
 *
 * Output: the builder's input layout exactly as seb_dev_merge_emit writes it (keys / key_off, vals / val_off,
 * entries_out + 1 offsets each starting at 0, deleted = 1 or 0) plus seq (nullable): seq[o] = the surviving
 * record's sequence, which MemTable.Get returns.  Nothing outside the sizes the plan returned is written.
 *
 * Safety: before anything else of a record is read its framing is checked (length >= 21 and 21 + keySize +
 * valueSize == length, 64-bit sums), and before that its offsets (rec_off[0] <= rec_off[i] <= rec_off[i+1] <=
 * rec_off[n]).  The first record that fails either check: SEB_ERR_INVALID, and seb_last_error names it
 * ("record R").  No byte outside [rec_off[0], rec_off[n]) is read on any input.  The CRC is NOT rechecked:
 * that is SEB_WAL_VERIFY's job, which the caller runs first (seb_wal_recover does).  Limits: n < 2^32; key and
 * value sizes take the full u32.  n == 0 is valid and gives an empty run. */
typedef struct seb_replay_sizes {
    uint64_t records_in, entries_out; /* records / surviving entries */
    uint64_t key_bytes, val_bytes;    /* of the survivors */
    uint64_t overwritten, tombstones; /* records lost to a later record of their key / surviving tombstones */
    uint64_t max_sequence;            /* lsm.sequence after the recovery */
    uint64_t memtable_size;           /* MemTable.size after the recovery */
} seb_replay_sizes;

/* Host only.  seb_wal_replay_plan sizes the output; seb_wal_replay_emit (`sizes` as the plan returned them;
 * anything else: SEB_ERR_INVALID) writes it.  They are the reference for the device form and what a caller
 * without a GPU uses. */
int seb_wal_replay_plan(const uint8_t *data, const uint64_t *rec_off, uint64_t n, seb_replay_sizes *sizes);
int seb_wal_replay_emit(const uint8_t *data, const uint64_t *rec_off, uint64_t n, uint8_t *keys, uint64_t *key_off,
                        uint8_t *vals, uint64_t *val_off, uint8_t *deleted, uint64_t *seq,
                        const seb_replay_sizes *sizes);

/* Device pointers, rec_off included (n + 1 u64, 8-byte aligned); sizes is HOST memory.
 * seb_dev_wal_replay_plan (workspace: seb_dev_wal_replay_workspace_size(n) bytes of device memory, 16-byte
 * aligned, opaque; too small: SEB_ERR_INVALID) checks and decodes the records, sorts them, marks the survivors,
 * SYNCHRONISES and fills *sizes, so the caller can allocate the outputs.
 * seb_dev_wal_replay_emit (not synchronised; the same image, offsets and workspace, untouched in between;
 * `sizes` as the plan returned them) writes the six output arrays; keys, vals and deleted may have any byte
 * alignment.  Before it launches it reads the workspace's 128-byte header back (so it waits for what the
 * stream already holds; nothing, right after the plan): a workspace that does not hold the plan that returned
 * `sizes` is SEB_ERR_INVALID and nothing is written.  Nothing is launched when records_in == 0. */
uint64_t seb_dev_wal_replay_workspace_size(uint64_t n);
int seb_dev_wal_replay_plan(const uint8_t *data, const uint64_t *rec_off, uint64_t n, void *workspace,
                            uint64_t workspace_bytes, seb_replay_sizes *sizes, void *stream);
int seb_dev_wal_replay_emit(const uint8_t *data, const uint64_t *rec_off, const seb_replay_sizes *sizes,
                            const void *workspace, uint64_t workspace_bytes, uint8_t *keys, uint64_t *key_off,
                            uint8_t *vals, uint64_t *val_off, uint8_t *deleted, uint64_t *seq, void *stream);
/* The host-buffer form on a context: WAL.ReadAll + recoverFromWAL in one synchronous call.  image (bytes) and
 * the outputs are host memory: seb_wal_scan on the host, H2D, SEB_WAL_VERIFY, plan, emit, D2H.  key_cap /
 * val_cap bytes and entry_cap entries (key_off and val_off hold entry_cap + 1 offsets, seq is nullable); a
 * capacity below a size: SEB_ERR_RANGE with *sizes filled, so the caller can retry (the seb_merge convention).
 * Errors come in ReadAll's order: a complete record that fails verification is SEB_ERR_INVALID and
 * seb_last_error reads "WAL corruption detected: CRC mismatch (record R)" with the lowest R, also when the tail
 * is truncated as well (ReadAll meets the bad record first); otherwise a truncated tail is SEB_ERR_SHORT.  An
 * empty image is valid and gives an empty run. */
int seb_wal_recover(seb_ctx *ctx, const uint8_t *image, uint64_t bytes, uint8_t *keys, uint64_t key_cap,
                    uint64_t *key_off, uint8_t *vals, uint64_t val_cap, uint64_t *val_off, uint8_t *deleted,
                    uint64_t *seq, uint64_t entry_cap, seb_replay_sizes *sizes);

/* ------------- batched memtable lookup: LSM.Get's first two steps, and the join with the SSTables' answer ---- */
/* Before it looks at any file, LSM.Get asks the active memtable and then the immutable one (lsm/lsm.go:144-166),
 * and whichever holds the key ends the Get.  MemTable.Get (lsm/memtable.go:95-112) is
 *   idx := sort.Search(len(entries), entries[i].Key >= key);  idx < len && entries[idx].Key == key
 * over the sorted slice that GetAllEntries() returns (memtable.go:129-137): a sorted run in the builder's input
 * layout, keys / key_off / vals / val_off / deleted / seq, exactly what seb_dev_wal_replay_emit and
 * seb_dev_merge_emit write.  This group looks a key batch up in up to SEB_MEM_MAX_RUNS such runs.
 *
 * Semantics, bit-exact with the reference:
 *   - runs are visited in array order: run 0 is the active memtable, run 1 the immutable one.
 *   - the first run that holds the key decides: SEB_MEM_FOUND, or SEB_MEM_TOMBSTONE where deleted[e] != 0 (ANY
 *     non-zero byte, the builder's input rule).  Later runs are not consulted: a tombstone in run 0 hides a
 *     value in run 1.  A key held by no run: SEB_MEM_NONE.
 *   - A TOMBSTONE IN A MEMTABLE ENDS LSM.Get with "not found" and no SSTable is read (lsm.go:150-153,160-163),
 *     unlike a tombstone inside an SSTable, which falls through to older files (seb_dev_resolve_rows).  So the
 *     memtable step has a status of its own, and seb_dev_get_join makes LSM.Get's decision over both halves.
 *   - order is Go string order: bytewise, a key before its extensions; the empty key is a key like any other.
 * Outputs per key (status required, the others nullable): status u8; run u8 = the deciding run, 0xFF for none;
 * entry u32 = the deciding entry, SEB_MEM_NO_ENTRY for none; vloc u64 = val_off[e] and vlen u32 = val_off[e+1] -
 * val_off[e], both 0 unless the status is SEB_MEM_FOUND (Delete stores Value nil: a tombstone reports no value);
 * seq u64 = the entry's sequence, 0 for none and where the deciding run has no seq array.
 *
 * The one stated refusal: a run whose keys do not increase STRICTLY is SEB_ERR_INVALID.  sort.Search on an
 * unsorted slice answers by its probe sequence, and no memtable produces one (Put and Delete keep one entry
 * per key in order); the block locator refuses unsorted indexes for the same reason.  Also refused: key_off
 * that decreases or passes key_bytes, val_off that decreases, a key or a value of 2^32 bytes or more.  The
 * checks run entry by entry (an entry's key offsets, its value offsets, then its key against its
 * predecessor's) and seb_last_error names the first entry that fails ("entry E").  Limits: n < 2^32 entries
 * per run, keys->n < 2^32. */
#define SEB_MEM_MAX_RUNS 8u
enum seb_mem_status { SEB_MEM_NONE = 0, SEB_MEM_FOUND = 1, SEB_MEM_TOMBSTONE = 2 };
#define SEB_MEM_NO_ENTRY UINT32_MAX
typedef struct seb_run {            /* a sorted run in the builder's input layout */
    const uint8_t *keys;  uint64_t key_bytes;   /* bytes addressable from keys */
    const uint64_t *key_off;                    /* n + 1, key_off[0] may be != 0 */
    const uint64_t *val_off;                    /* n + 1, val_off[0] may be != 0 */
    const uint8_t *deleted;                     /* n; any non-zero byte = deleted (the builder's rule); NULL: none */
    const uint64_t *seq;                        /* n; nullable */
    uint64_t n;                                 /* < 2^32 */
} seb_run;

/* Host only: the run pointers and the keys are host memory.  Every run is checked first, as seb_dev_run_index
 * checks it (SEB_ERR_INVALID, "run R: entry E"); then every key is looked up.  num_runs == 0, or runs of 0
 * entries: everything is SEB_MEM_NONE.  num_runs > SEB_MEM_MAX_RUNS or a null required pointer:
 * SEB_ERR_INVALID.  It is the reference for the device form and what a caller without a GPU uses. */
int seb_runs_search(const seb_keys *keys, const seb_run *runs, uint32_t num_runs, uint8_t *status, uint8_t *run,
                    uint32_t *entry, uint64_t *vloc, uint32_t *vlen, uint64_t *seq);
/* Host only: seb_dev_get_join on host arrays. */
int seb_get_join(const uint8_t *mem_status, const uint8_t *sst_status, uint64_t n, uint8_t *status, uint8_t *source);

/* A run's device index: opaque device memory of seb_dev_run_index_size(n) bytes (0 for n == 0 and for
 * n >= 2^32), 16-byte aligned; it holds the zero-padded big-endian 16-byte prefix of every key (two u64 per
 * entry, the layout seb_registry_put_index uses) behind a 16-byte header.  seb_dev_run_index (`run`: a HOST
 * struct of device pointers, key_off / val_off / seq 8-byte aligned, keys and deleted at any byte alignment)
 * builds it and runs the checks above on the device; it SYNCHRONISES and returns SEB_ERR_INVALID naming the
 * first offending entry, SEB_OK otherwise.  No key byte of an entry is read before its offsets and its
 * predecessor's have passed.  n == 0 is valid: nothing is launched and index may be null.  A run that changes
 * needs its index built again. */
uint64_t seb_dev_run_index_size(uint64_t n);
int seb_dev_run_index(const seb_run *run, void *index, uint64_t index_bytes, void *stream);
/* Device pointers, not synchronised; `runs` and `index` are HOST arrays of num_runs elements (index[r] may be
 * null where runs[r].n == 0).  Keys in every seb_keys layout at any byte alignment.  num_runs == 0, or runs of
 * 0 entries: everything is SEB_MEM_NONE.  num_runs > SEB_MEM_MAX_RUNS, a null required pointer or
 * keys->n >= 2^32: SEB_ERR_INVALID.  keys->n == 0: nothing is launched.  Nothing outside the n elements of each
 * output is written.  On any index content nothing is read outside the runs' arrays as seb_dev_run_index
 * checked them and the first seb_dev_run_index_size(n) bytes of each index: a stale index gives wrong answers,
 * never an out-of-bounds read. */
int seb_dev_runs_search(const seb_keys *keys, const seb_run *runs, const void *const *index, uint32_t num_runs,
                        uint8_t *status, uint8_t *run, uint32_t *entry, uint64_t *vloc, uint32_t *vlen, uint64_t *seq,
                        void *stream);
/* LSM.Get's decision over both halves; device pointers, not synchronised.  sst_status is the array
 * seb_dev_resolve_rows writes.  SEB_MEM_FOUND gives SEB_GET_FOUND; SEB_MEM_TOMBSTONE gives SEB_GET_MISS, also
 * where sst_status[i] is SEB_GET_ERROR: the reference has returned before it reads any file; SEB_MEM_NONE gives
 * sst_status[i].  source[i] (nullable) = 0 where the memtables decided, 1 where the SSTables' answer stands.
 * status may alias sst_status. */
int seb_dev_get_join(const uint8_t *mem_status, const uint8_t *sst_status, uint64_t n, uint8_t *status,
                     uint8_t *source, void *stream);
/* The host-buffer form on a context: keys, the runs' arrays and the six outputs in host memory; H2D of each
 * run's keys, offsets, deleted bytes and sequences (not its values: the answer is a location), the indexes,
 * the search, D2H; synchronous.  A run that fails its checks: SEB_ERR_INVALID, "run R: entry E". */
int seb_memtable_get(seb_ctx *ctx, const seb_keys *keys, const seb_run *runs, uint32_t num_runs, uint8_t *status,
                     uint8_t *run, uint32_t *entry, uint64_t *vloc, uint32_t *vlen, uint64_t *seq);

/* ------------- Get path: only the keys the memtables leave undecided go on to the SSTable steps ---- */
/* LSM.Get returns at the first memtable that holds the key, value or tombstone, and reads no filter, no index and
 * no block for it (lsm/lsm.go:144-166).  For a batch that is a stream compaction between seb_dev_runs_search and
 * the SSTable steps (seb_registry_multiget_list_dev, seb_registry_locate_dev, seb_dev_search_blocks,
 * seb_dev_resolve_rows), which then run on m <= n keys, and a join that puts their answers back on the batch rows.
 *
 * Undecided keys: key i is undecided iff mem_status[i] is neither SEB_MEM_FOUND nor SEB_MEM_TOMBSTONE, whatever
 * else the byte holds (3 and 255 count as undecided).  That is the rule by which seb_dev_get_join takes
 * sst_status[i], so both pipelines give every status byte the same status.
 *
 * Compaction: the undecided keys in batch order (stable) become a dense batch of m = sizes->undecided keys, and
 * row[j] (u32) = the batch index of compacted key j; row increases strictly.  A fixed-stride batch gives a
 * fixed-stride batch of the same stride (key j at out_keys + j * stride; out_off is neither required nor
 * written); a batch with offsets gives out_off[0..m], out_off[0] == 0 (whatever offsets[0] was), and
 * sizes->key_bytes = the sum of the undecided keys' lengths = out_off[m].
 *
 * Row-mapped join, per batch key i:
 *   SEB_MEM_FOUND      status SEB_GET_FOUND, source 0, vloc = mem_vloc[i], vlen = mem_vlen[i], col 0xFFFF
 *   SEB_MEM_TOMBSTONE  status SEB_GET_MISS, source 0, vloc 0, vlen 0, col 0xFFFF
 *   undecided          the j with row[j] == i: status = sst_status[j], source 1, vloc / vlen / col = sst_vloc[j] /
 *                      sst_vlen[j] / sst_col[j], as seb_dev_resolve_rows wrote them for compacted key j
 * and on bad input: an undecided key that no row names reads SEB_GET_MISS, source 1, 0, 0, 0xFFFF; a row[j] >= n
 * or one naming a decided key is ignored (never an out-of-bounds or an overriding write); rows are expected to be
 * distinct, and with duplicates which of them wins is unspecified.  mem_vloc, mem_vlen, sst_col, sst_vloc and
 * sst_vlen are nullable and read as 0 (0xFFFF for sst_col); source, col, vloc and vlen are nullable.  status
 * must not alias sst_status (they differ in length).  On status the result equals seb_dev_get_join over the
 * whole batch's sst_status, and on source too for the three seb_mem_status values (seb_dev_get_join reports
 * source 0 for a status byte above 2, this group 1: the SSTables' answer stands there). */
typedef struct seb_compact_sizes {
    uint64_t n;         /* keys->n */
    uint64_t undecided; /* m: rows of the compacted batch */
    uint64_t key_bytes; /* of the compacted batch: m * stride, or the sum of the undecided keys' lengths */
    uint64_t reserved;  /* 0 */
} seb_compact_sizes;

/* Host only: keys in every seb_keys layout, everything in host memory.  *sizes is always filled.  out_keys,
 * out_off and row all NULL: sizes only (the host's plan), and key_cap / row_cap are not looked at.  Otherwise
 * row_cap < undecided or key_cap < key_bytes is SEB_ERR_RANGE with *sizes filled for the retry and nothing
 * written; then row (where undecided != 0), out_keys (where key_bytes != 0) and out_off (iff keys->offsets is
 * non-NULL) are required.  Writes row[0, undecided), out_off[0, undecided] and out_keys[0, key_bytes) and
 * nothing else.  SEB_ERR_INVALID: a NULL required pointer (keys, sizes, mem_status where n != 0), offsets that
 * decrease, keys->n >= 2^32.  n == 0 is valid.  It is the reference for the device form. */
int seb_get_compact(const seb_keys *keys, const uint8_t *mem_status, seb_compact_sizes *sizes, uint8_t *out_keys,
                    uint64_t key_cap, uint64_t *out_off, uint32_t *row, uint64_t row_cap);
/* Host only: the row-mapped join above on host arrays.  Required: mem_status and status where n != 0, row and
 * sst_status where m != 0 (else SEB_ERR_INVALID, nothing written); n >= 2^32: SEB_ERR_INVALID.  Writes the n
 * elements of each non-NULL output and nothing else. */
int seb_get_join_rows(const uint8_t *mem_status, const uint64_t *mem_vloc, const uint32_t *mem_vlen, uint64_t n,
                      const uint32_t *row, uint64_t m, const uint8_t *sst_status, const uint16_t *sst_col,
                      const uint64_t *sst_vloc, const uint32_t *sst_vlen, uint8_t *status, uint8_t *source, uint16_t *col,
                      uint64_t *vloc, uint32_t *vlen);

/* Device pointers (offsets and out_off 8-byte aligned, row 4-byte aligned; keys in every seb_keys layout at any
 * byte alignment, mem_status and out_keys at any byte alignment); `sizes` is HOST memory.  The workspace
 * (seb_dev_get_compact_workspace_size(n) bytes of device memory, 16-byte aligned, opaque; 0 for n >= 2^32)
 * carries the plan to the emit and must not be touched in between.
 * seb_dev_get_compact_plan SYNCHRONISES and fills *sizes, so the caller can allocate (or check) the outputs.
 * seb_dev_get_compact_emit (not synchronised; the same keys, mem_status and workspace) writes row[0, undecided),
 * out_off[0, undecided] (required iff keys->offsets is non-NULL, else ignored) and out_keys[0, key_bytes).
 * SEB_ERR_INVALID and nothing launched: a NULL required pointer (keys, sizes; mem_status and workspace where
 * n != 0; for the emit row, out_off as above and out_keys where key_bytes != 0), keys->n >= 2^32, a misaligned
 * pointer, a workspace below seb_dev_get_compact_workspace_size(n) (plan), sizes->n != keys->n, undecided > n or
 * a key_bytes that is not undecided * stride for a fixed-stride batch (emit).  keys->n == 0, and for the emit
 * sizes->undecided == 0: nothing is launched and nothing is written, out_off[0] included, SEB_OK (for n == 0 the
 * plan sets *sizes to zeros and needs no workspace).
 * Write bounds, whatever the inputs hold: the workspace's header carries a magic word, n, the tile count and the
 * plan's two totals; where they do not match `sizes` the emit writes nothing.  Where mem_status changed between
 * plan and emit the outputs may be wrong, but every store is clamped to the three ranges above.  Nothing is read
 * outside the batch's keys as its offsets describe them, mem_status[0, n) and the workspace. */
uint64_t seb_dev_get_compact_workspace_size(uint64_t n);
int seb_dev_get_compact_plan(const seb_keys *keys, const uint8_t *mem_status, void *workspace, uint64_t workspace_bytes,
                             seb_compact_sizes *sizes, void *stream);
int seb_dev_get_compact_emit(const seb_keys *keys, const uint8_t *mem_status, const seb_compact_sizes *sizes,
                             const void *workspace, uint8_t *out_keys, uint64_t *out_off, uint32_t *row, void *stream);
/* The row-mapped join on device pointers, not synchronised: two launches in stream order, a lane per batch key
 * (the memtables' answer or the "no row" default), then a lane per row.  Required pointers and refusals as the
 * host form, also m >= 2^32.  n == 0: nothing is launched; m == 0: the first launch alone.  Nothing outside the n
 * elements of each output is written, whatever row holds. */
int seb_dev_get_join_rows(const uint8_t *mem_status, const uint64_t *mem_vloc, const uint32_t *mem_vlen, uint64_t n,
                          const uint32_t *row, uint64_t m, const uint8_t *sst_status, const uint16_t *sst_col,
                          const uint64_t *sst_vloc, const uint32_t *sst_vlen, uint8_t *status, uint8_t *source,
                          uint16_t *col, uint64_t *vloc, uint32_t *vlen, void *stream);

/* ------------- Get values: a batch's found values gathered into one dense buffer ---- */
/* LSM.Get returns the value: searchBlock's make([]byte, valueSize) + copy (lsm/sstable.go:276-278), or the memtable
 * entry's Value (lsm/lsm.go:146-152, 157-163, 175-180).  The Get path above ends with a location per key; this
 * group does the copy for a batch: the found keys' values back to back in batch order, with an offset array, so a
 * GetBatch is one D2H copy away from its answer.
 *
 * Inputs per batch key i: status[i] (seb_get_status), source[i] (0: the memtables decided; 1: the block pool holds
 * the value), vloc[i] (u64), vlen[i] (u32), as seb_dev_get_join_rows writes them, and run[i] (u8), the deciding
 * run as seb_dev_runs_search writes it; run is looked at only where source[i] == 0, may be NULL iff num_runs <= 1
 * and is then read as 0.  (Pipeline A's seb_dev_get_join + seb_dev_resolve_rows arrays also work, with the
 * memtables' vloc / vlen merged in by the caller.)
 * Sources: vals[r][0, val_bytes[r]) for r < num_runs <= SEB_MEM_MAX_RUNS, the runs' value bytes as
 * seb_dev_runs_fold_emit takes them (vloc is the entry's val_off, an offset from vals[r]; vals[r] may be NULL only
 * where val_bytes[r] == 0), and pool[0, pool_bytes), the block pool (vloc = bid * 4096 + voff; pool may be NULL iff
 * pool_bytes == 0).  num_runs == 0 is valid.
 *
 * Key i carries a value iff status[i] == SEB_GET_FOUND exactly.  Every other status byte (MISS, ERROR, 3, 255)
 * contributes 0 bytes, and its source, run, vloc and vlen are never used to form an address, whatever they hold.
 * A carrying key is valid iff
 *   source == 0, run[i] < num_runs, vloc <= val_bytes[r] and vlen <= val_bytes[r] - vloc (compared this way round,
 *                so nothing wraps), and vals[r] is not a NULL with val_bytes[r] != 0; or
 *   source == 1, vloc <= pool_bytes and vlen <= pool_bytes - vloc (a pool value is NOT required to lie inside one
 *                4 KiB block: the resolve guarantees that, this step does not re-check it).
 * Any other source byte is invalid.  INVALID CARRYING KEYS ARE REFUSED, NOT SKIPPED: SEB_ERR_INVALID, and
 * seb_last_error names the lowest such key ("key K"); *sizes then holds n alone and no emit may follow.  (The
 * rule seb_dev_run_index applies to runs; a skipped value would be a Get that silently returns the wrong bytes.)
 *
 * Outputs: out_off[0..n] (u64), out_off[0] = 0 and out_off[i + 1] - out_off[i] = vlen[i] for a carrying key, else
 * 0; out_vals[0, out_off[n]) = the values back to back.  A found empty value and a miss both have an empty span;
 * status tells them apart. */
typedef struct seb_values_sizes {
    uint64_t n;         /* batch keys */
    uint64_t found;     /* carrying keys */
    uint64_t val_bytes; /* the sum of their vlen = out_off[n] */
    uint64_t reserved;  /* 0 */
} seb_values_sizes;

/* Host only: everything in host memory.  *sizes is always filled.  out_off and out_vals both NULL: sizes only (the
 * host's plan), and val_cap is not looked at.  Otherwise val_cap < val_bytes is SEB_ERR_RANGE with *sizes filled
 * for the retry and nothing written (seb_get_compact's convention); then out_off is required, and out_vals where
 * val_bytes != 0.  Writes out_off[0, n] and out_vals[0, val_bytes) and nothing else.  SEB_ERR_INVALID: the refusal
 * above, a NULL required pointer (sizes; status, source, vloc and vlen where n != 0; run where num_runs > 1; vals and
 * val_bytes where num_runs != 0; pool where pool_bytes != 0), num_runs > SEB_MEM_MAX_RUNS, n >= 2^32.  n == 0 is
 * valid.  It is the reference for the device form and what a caller without a GPU uses.
 * There is no host-buffer form on a seb_ctx: it would upload the whole pool for one gather. */
int seb_get_values(const uint8_t *status, const uint8_t *source, const uint8_t *run, const uint64_t *vloc,
                   const uint32_t *vlen, uint64_t n, const uint8_t *const *vals, const uint64_t *val_bytes,
                   uint32_t num_runs, const uint8_t *pool, uint64_t pool_bytes, seb_values_sizes *sizes,
                   uint64_t *out_off, uint8_t *out_vals, uint64_t val_cap);

/* Device pointers (vloc and out_off 8-byte aligned, vlen 4-byte aligned; status, source, run, the sources and
 * out_vals at any byte alignment); `vals` and `val_bytes` are HOST arrays of num_runs elements holding device
 * pointers and sizes, like `runs` / `index` in seb_dev_runs_search; `sizes` is HOST memory.  The workspace
 * (seb_dev_get_values_workspace_size(n) bytes of device memory, 16-byte aligned, opaque; 0 for n >= 2^32) carries
 * the plan to the emit and must not be touched in between; the emit writes to it too.
 * seb_dev_get_values_plan SYNCHRONISES, fills *sizes, and returns the refusal above.
 * seb_dev_get_values_emit (not synchronised; the same inputs and workspace) writes out_off[0, n] and
 * out_vals[0, val_bytes).  Where val_bytes == 0 out_off is still written (all zeros), out_vals may be NULL and no
 * copy kernel is launched.  n == 0: nothing is launched and nothing is written, SEB_OK (the plan sets *sizes to
 * zeros and needs no workspace).
 * SEB_ERR_INVALID and nothing launched: a NULL required pointer (as the host form; the workspace where n != 0; for
 * the emit out_off, and out_vals where val_bytes != 0), n >= 2^32, num_runs > SEB_MEM_MAX_RUNS, a misaligned
 * pointer, a workspace below seb_dev_get_values_workspace_size(n) (plan), sizes->n != n or found > n (emit).
 * Bounds, whatever the inputs hold: the workspace's header carries a magic word, n, the tile count, the plan's two
 * totals and its refusal; where they do not match `sizes` the emit writes nothing.  The emit re-derives every
 * source address from the inputs and checks it against its source, so where the inputs changed between plan and
 * emit the outputs may be wrong, but nothing is read outside vals[r][0, val_bytes[r]), pool[0, pool_bytes), the five
 * input arrays and the workspace, and nothing is written outside out_off[0, n] and out_vals[0, val_bytes). */
uint64_t seb_dev_get_values_workspace_size(uint64_t n);
int seb_dev_get_values_plan(const uint8_t *status, const uint8_t *source, const uint8_t *run, const uint64_t *vloc,
                            const uint32_t *vlen, uint64_t n, const uint8_t *const *vals, const uint64_t *val_bytes,
                            uint32_t num_runs, const uint8_t *pool, uint64_t pool_bytes, void *workspace,
                            uint64_t workspace_bytes, seb_values_sizes *sizes, void *stream);
int seb_dev_get_values_emit(const uint8_t *status, const uint8_t *source, const uint8_t *run, const uint64_t *vloc,
                            const uint32_t *vlen, uint64_t n, const uint8_t *const *vals, const uint64_t *val_bytes,
                            uint32_t num_runs, const uint8_t *pool, uint64_t pool_bytes, const seb_values_sizes *sizes,
                            void *workspace, uint64_t *out_off, uint8_t *out_vals, void *stream);

/* ------------- memtable write side: Put / Delete batches into WAL records, the memtable's runs and the flush input ---- */
/* What LSM.Put / LSM.Delete do to the log and to the active memtable (lsm/lsm.go:97-137, 203-235, lsm/wal.go:31-65,
 * lsm/memtable.go:34-93), for a batch of n ops applied in order by one writer, with lsm.sequence == S before it.
 *
 * Sequences: op i gets seq = S + 1 + i (atomic.AddUint64 returns the new value); afterwards lsm.sequence = S + n.
 * The callers pass first_seq = S + 1.
 *
 * The record: WAL.Append(key, value, seq, deleted) writes [crc u32][seq u64][keySize u32][valueSize u32][deleted u8]
 * [key][value], little-endian, crc = ChecksumIEEE(record[4:]).  LSM.Delete appends value = nil: a Delete op's record
 * has valueSize = 0 and deleted = 1, WHATEVER VALUE BYTES THE OP ARRAYS CARRY FOR IT; a Put has deleted = 0.  An op is
 * a Delete where deleted[i] is any non-zero byte (deleted == NULL: none is).  The image of the batch is the
 * concatenation of its records, rec_off[i+1] - rec_off[i] = 21 + keyLen + (deleted ? 0 : valueLen), rec_off[0] = 0:
 * what the caller hands to one Write of the log, and what seb_wal_scan / SEB_WAL_VERIFY / seb_wal_replay_* read back.
 *
 * The memtable: MemTable.Put / Delete keep one entry per key; a later op of a key replaces the whole entry; tombstones
 * stay, with a nil value.  So after batches B1..Bk on a memtable that held the run `old`, the memtable equals
 *   fold([replay(Bk), ..., replay(B1), old])
 * where replay is the replay group's run of one batch's records and fold keeps, for each distinct key, the entry of
 * the LOWEST-NUMBERED RUN that holds it (the caller passes the runs newest first, the order seb_dev_runs_search
 * visits them in).  There is no departure from the reference: (key, run number) is a total order, so every output
 * byte of the fold is determined.  Tombstones are never dropped: a flush keeps them.
 *
 * MemTable.size is path independent: the sum over the entries of keyLen + 16 + valueLen, valueLen 0 for a tombstone.
 * For a new run put in front of the ACTIVE memtable's runs (the immutable memtable is a separate MemTable and takes
 * no part) its change is a sum over the new run's entries: an entry whose key no existing run holds adds keyLen + 16
 * + valueLen; an entry whose key the first existing run that holds it has with value length v_old adds valueLen -
 * v_old (0 for either length where that entry is a tombstone).
 *
 * WHEN TO FREEZE IS THE CALLER'S DECISION.  The reference tests IsFull() after every single op and freezes only when
 * immutableMemtable == nil, so the size at which a memtable freezes is no invariant of the reference: it runs past
 * maxSize whenever a flush is pending.  This group reports the size after the batch; the caller decides once per
 * batch.  There is no per-op cut.  Concurrent writers, file I/O (Write, Sync) and LSM.Scan are out of scope.
 *
 * The one refusal of the frame: a key or a value of 2^32 bytes or more (the reference would truncate uint32(len) and
 * corrupt its log), and offsets that decrease: SEB_ERR_INVALID, and seb_last_error names the lowest offender
 * ("op I").  The check runs on every op's offsets, a Delete's value offsets included, before any byte of the op is
 * read.  Limit: n < 2^32.  n == 0 is valid: nothing is launched and the image is empty. */
typedef struct seb_fold_sizes {
    uint64_t entries_in, entries_out; /* over all runs / distinct keys */
    uint64_t key_bytes, val_bytes;    /* of the output run */
    uint64_t shadowed, tombstones;    /* entries lost to a lower-numbered run / tombstones in the output */
    uint64_t max_sequence;            /* over ALL input entries, shadowed ones included; 0 where no run has seq */
    uint64_t memtable_size;           /* MemTable.size of the folded memtable */
} seb_fold_sizes;

/* Host only.  keys in every seb_keys layout; val_off: n + 1 non-decreasing offsets into vals (val_off[0] may be != 0);
 * deleted nullable.  seb_wal_frame_plan writes rec_off[0..n] (nullable) and *image_bytes (nullable);
 * seb_wal_frame_emit writes the sealed image into image[0, image_bytes) (image_bytes not the plan's:
 * SEB_ERR_INVALID) and nothing outside it.  They are the reference for the device form and what a caller without a
 * GPU uses. */
int seb_wal_frame_plan(const seb_keys *keys, const uint64_t *val_off, const uint8_t *deleted, uint64_t *rec_off,
                       uint64_t *image_bytes);
int seb_wal_frame_emit(const seb_keys *keys, const uint8_t *vals, const uint64_t *val_off, const uint8_t *deleted,
                       uint64_t first_seq, uint8_t *image, uint64_t image_bytes);
/* Device pointers (offsets 8-byte aligned; keys, vals, deleted and the image at any byte alignment); image_bytes of
 * the plan is HOST memory.  seb_dev_wal_frame_plan writes rec_off[0..n] (required), SYNCHRONISES and fills
 * *image_bytes, so the caller can allocate the image.  seb_dev_wal_frame_emit (not synchronised; rec_off and
 * image_bytes as the plan left them) writes the sealed image: the records, then SEB_WAL_SEAL's CRCs.  Nothing is
 * written outside [image, image + image_bytes) or the n + 1 offsets, and nothing is read outside the ops' arrays as
 * their offsets describe them.  rec_off is trusted as seb_dev_wal_crc trusts it: offsets that are not this batch's
 * plan are the caller's error. */
int seb_dev_wal_frame_plan(const seb_keys *keys, const uint64_t *val_off, const uint8_t *deleted, uint64_t *rec_off,
                           uint64_t *image_bytes, void *stream);
int seb_dev_wal_frame_emit(const seb_keys *keys, const uint8_t *vals, const uint64_t *val_off, const uint8_t *deleted,
                           uint64_t first_seq, const uint64_t *rec_off, uint8_t *image, uint64_t image_bytes,
                           void *stream);

/* MemTable.size's change when `fresh` goes in front of the active memtable's `runs` (num_runs <=
 * SEB_MEM_MAX_RUNS - 1, newest first).  Host: every run and `fresh` are checked as seb_runs_search checks a run
 * ("run R: entry E"; `fresh` is named "the new run").  Device: `fresh` and `runs` are HOST structs of device
 * pointers, index[r] is run r's index from seb_dev_run_index (`fresh` needs none); *delta is DEVICE memory (8-byte
 * aligned) and the call is not synchronised.  num_runs == 0 gives the run's own size.  On any index content nothing
 * is read outside the runs' arrays as seb_dev_run_index checked them. */
int seb_run_size_delta(const seb_run *fresh, const seb_run *runs, uint32_t num_runs, int64_t *delta);
int seb_dev_run_size_delta(const seb_run *fresh, const seb_run *runs, const void *const *index, uint32_t num_runs,
                           int64_t *delta, void *stream);

/* Fold up to SEB_MEM_MAX_RUNS runs, newest first, into the one run GetAllEntries() hands to the builder.  vals[r] /
 * val_bytes[r] are run r's value bytes (seb_run carries no value pointer); val_off[n] > val_bytes[r] is
 * SEB_ERR_INVALID naming "run R".  Output: the builder's input layout exactly as seb_dev_wal_replay_emit writes it:
 * keys / key_off / vals / val_off (entries_out + 1 offsets each, starting at 0), deleted = 1 or 0, seq (nullable): the
 * distinct keys in Go string order, the empty key included, each entry from the lowest-numbered run that holds it; a
 * tombstone comes out with no value, even where its run carries value bytes; seq from the winning entry, 0 where that
 * run has no seq array.  Limit: fewer than 2^32 entries in total.  num_runs == 0 and runs of 0 entries are valid.
 *
 * Host only: every run is checked as seb_runs_search checks it ("run R: entry E").  seb_runs_fold_emit takes `sizes`
 * as the plan returned them (anything else: SEB_ERR_INVALID). */
int seb_runs_fold_plan(const seb_run *runs, const uint64_t *val_bytes, uint32_t num_runs, seb_fold_sizes *sizes);
int seb_runs_fold_emit(const seb_run *runs, const uint8_t *const *vals, const uint64_t *val_bytes, uint32_t num_runs,
                       uint8_t *keys, uint64_t *key_off, uint8_t *out_vals, uint64_t *val_off, uint8_t *deleted,
                       uint64_t *seq, const seb_fold_sizes *sizes);
/* Device: `runs`, `index`, `vals` and `val_bytes` are HOST arrays; the runs' pointers, the indexes (from
 * seb_dev_run_index, which has refused unsorted runs and bad offsets) and vals[r] are device memory.  The workspace
 * (seb_dev_runs_fold_workspace_size(total entries) bytes of device memory, 16-byte aligned, opaque; too small:
 * SEB_ERR_INVALID) carries the plan to the emit and must not be touched in between.  seb_dev_runs_fold_plan
 * SYNCHRONISES and fills *sizes.  seb_dev_runs_fold_emit (not synchronised; the same runs, indexes and workspace)
 * reads the workspace's 128-byte header back before it launches: a workspace that does not hold the plan that
 * returned `sizes` is SEB_ERR_INVALID and nothing is written.  Nothing is launched when entries_in == 0.  Nothing
 * outside the sizes the plan returned is written, and on any index or workspace content nothing is read outside
 * the runs' arrays (key_bytes, val_bytes[r], n entries): a stale index gives a wrong run, never an out-of-bounds
 * access. */
uint64_t seb_dev_runs_fold_workspace_size(uint64_t entries);
int seb_dev_runs_fold_plan(const seb_run *runs, const void *const *index, const uint64_t *val_bytes, uint32_t num_runs,
                           void *workspace, uint64_t workspace_bytes, seb_fold_sizes *sizes, void *stream);
int seb_dev_runs_fold_emit(const seb_run *runs, const void *const *index, const uint8_t *const *vals,
                           const uint64_t *val_bytes, uint32_t num_runs, const seb_fold_sizes *sizes,
                           const void *workspace, uint64_t workspace_bytes, uint8_t *keys, uint64_t *key_off,
                           uint8_t *out_vals, uint64_t *val_off, uint8_t *deleted, uint64_t *seq, void *stream);

/* The host-buffer forms on a context; synchronous.
 * seb_memtable_apply: one write batch.  Ops (keys / vals / val_off / deleted), first_seq and the active memtable's
 * existing runs (num_runs <= SEB_MEM_MAX_RUNS - 1, newest first; their values are not needed) in host memory.  H2D,
 * frame, seal, replay plan + emit of the image, index of the new run's keys, size delta, D2H.  Outputs: the sealed
 * image (image_cap bytes; the caller's one Write to the log), the batch's run in six arrays (key_cap / val_cap bytes,
 * entry_cap entries, key_off and val_off entry_cap + 1 offsets; seq nullable), *sizes = the replay's sizes of the
 * batch, *size_delta = MemTable.size's change, *sequence = lsm.sequence after the batch (first_seq - 1 + n).  A
 * capacity below a size: SEB_ERR_RANGE with *image_bytes and *sizes filled, so the caller can retry (the
 * seb_wal_recover convention).  An existing run that fails its checks: SEB_ERR_INVALID, "run R: entry E".
 * seb_memtable_fold: runs (with vals / val_bytes) in host memory into one run in host memory; same convention. */
int seb_memtable_apply(seb_ctx *ctx, const seb_keys *keys, const uint8_t *vals, const uint64_t *val_off,
                       const uint8_t *deleted, uint64_t first_seq, const seb_run *runs, uint32_t num_runs,
                       uint8_t *image, uint64_t image_cap, uint64_t *image_bytes, uint8_t *run_keys, uint64_t key_cap,
                       uint64_t *run_key_off, uint8_t *run_vals, uint64_t val_cap, uint64_t *run_val_off,
                       uint8_t *run_deleted, uint64_t *run_seq, uint64_t entry_cap, seb_replay_sizes *sizes,
                       int64_t *size_delta, uint64_t *sequence);
int seb_memtable_fold(seb_ctx *ctx, const seb_run *runs, const uint8_t *const *vals, const uint64_t *val_bytes,
                      uint32_t num_runs, uint8_t *keys, uint64_t key_cap, uint64_t *key_off, uint8_t *out_vals,
                      uint64_t val_cap, uint64_t *val_off, uint8_t *deleted, uint64_t *seq, uint64_t entry_cap,
                      seb_fold_sizes *sizes);

/* ---------- hash-index shard routing + WAL record checksums (off the bloom path) ---- */
/* shard[i] = FNV-1a32(key i) & ((1 << shard_bits) - 1), the reference's getShard
 * (hashindex/shard.go:47-52; 256 shards = shard_bits 8).  hash[i] (nullable) = the full FNV-1a32.
 * shard (nullable) is one u16 per key; shard_bits <= 16.  Device pointers. */
int seb_dev_shard_route(const seb_keys *keys, uint32_t shard_bits, uint16_t *shard, uint32_t *hash, void *stream);
/* Stable partition of a key batch by shard: UpdateBatch's distribution step (hashindex/shard.go:104-122).
 * perm = key indices grouped by shard ascending, input order inside a shard; shard s owns
 * perm[shard_begin[s], shard_begin[s+1]) (shard_begin nullable, 2^shard_bits + 1 entries); shard
 * (nullable) as above.  shard_bits <= 12, n < 2^32; workspace of
 * seb_dev_shard_partition_workspace_size bytes.  The reference distributes a Go map, whose order
 * is random: it defines only the set per shard, which this order refines. */
uint64_t seb_dev_shard_partition_workspace_size(uint64_t n, uint32_t shard_bits);
int seb_dev_shard_partition(const seb_keys *keys, uint32_t shard_bits, uint32_t *perm, uint64_t *shard_begin,
                            uint16_t *shard, void *workspace, uint64_t workspace_bytes, void *stream);
/* WAL records (lsm/wal.go:31-62): record i = data[rec_off[i], rec_off[i+1]) =
 * [crc32 u32][seq u64][keySize u32][valueSize u32][deleted u8][key][value], all little-endian,
 * crc = crc32.ChecksumIEEE(record[4:]).  SEB_WAL_CRC: crc[i] only; SEB_WAL_SEAL: also store it in
 * the record (Append, :59-60); SEB_WAL_VERIFY: ok[i] = 1 iff the record is framed (length >= 21
 * and 21 + keySize + valueSize == length) and its stored CRC matches (ReadAll, :98-133).  crc and
 * ok are nullable except ok for VERIFY.  Device pointers. */
enum seb_wal_mode { SEB_WAL_CRC = 0, SEB_WAL_SEAL = 1, SEB_WAL_VERIFY = 2 };
int seb_dev_wal_crc(uint8_t *data, const uint64_t *rec_off, uint64_t n, int mode, uint32_t *crc, uint8_t *ok,
                    void *stream);
/* Host: walk a WAL image's framing as ReadAll does (21-byte header, then keySize + valueSize bytes)
 * into rec_off (cap entries).  *n = complete records; rec_off[0..*n] are their boundaries.
 * SEB_OK if the image ends on a record boundary, SEB_ERR_SHORT if the tail is a truncated header or
 * payload (ReadAll's "failed to read WAL header/data" error), SEB_ERR_INVALID if cap < records + 1. */
int seb_wal_scan(const uint8_t *data, uint64_t bytes, uint64_t *rec_off, uint64_t cap, uint64_t *n);

/* ------------- hash index, read side: recover() for a set of segment images, Get for a key batch ---- */
/* The reference's second engine (hashindex/) is a Bitcask-style store: append-only segment files and an in-memory map
 * from key to (segment, offset, size).  This group is its read side: what recover() (hashindex/recovery.go:14-141)
 * makes of the segment files, and what Get (hashindex/hashindex.go:217-260 -> segment.read, hashindex/segment.go:
 * 127-183) answers from them, for a key batch.  The write side (append's framing, segment rotation) and
 * compactSegments are the next group.
 *
 * Layout: the caller holds the segment images back to back, OLDEST FIRST (ascending segment id), in one byte pool of
 * pool_bytes < 2^47, with per-segment host arrays seg_base[s] (the image's first byte in the pool) and seg_bytes[s].
 * A record is named by its POOL OFFSET; because the segments lie in id order, the later record of a key is the one
 * at the greater pool offset, the only order the device needs.
 *
 * The record (segment.go:14-18, 61-125): [crc u32][timestamp u64][keySize u32][valueSize u32][key][value], little-
 * endian, a SEB_SEG_HEADER_BYTES header, crc = ChecksumIEEE(record[4:]).  valueSize == 0 is a tombstone.
 *
 * recover(): the segments in ascending id, each from offset 0.  Where fewer than 20 bytes remain, or the payload
 * runs past the end of the file, ReadAt returns io.EOF and recover BREAKS WITHOUT TRUNCATING: the segment keeps its
 * size (short_tail).  A complete record whose CRC does not match CUTS the segment at that record's offset (Truncate,
 * size = offset): it and everything behind it in this segment is dropped; later segments are still read.  Every
 * record before that sets latestValues[key]; the last one in (segment, offset) order wins.  A key of length 0 is
 * accepted here (only Put refuses it).  TOMBSTONES STAY IN THE INDEX: recover's `entry.size == 0` test is never true,
 * size being the whole record's, so the key count after recovery is the number of distinct keys, deleted ones
 * included.
 *
 * Get: the index lookup, then segment.read, which re-verifies the record's CRC on every read (a mismatch is an
 * error) and only then looks at the value (an empty one is ErrKeyNotFound).  Per key: SEB_GET_MISS where the key is
 * absent or its latest record is a tombstone; SEB_GET_ERROR on a CRC mismatch (a corrupted tombstone included: the
 * CRC comes first); SEB_GET_FOUND with rec = the record's pool offset, vloc = rec + 20 + keySize and vlen =
 * valueSize.  MISS and ERROR rows get rec = SEB_HIDX_NO_RECORD, vloc = 0, vlen = 0.  With verify == 0 the CRC is not
 * looked at.  The (status, vloc, vlen) arrays are the ones the LSM Get path ends in, so seb_dev_get_values gathers
 * the values from them unchanged, with the segment pool as its `pool`, source = 1 and num_runs = 0.
 *
 * ONE DEPARTURE from the reference: a header with keySize + valueSize >= 2^32 is treated as a CRC failure: the
 * segment is cut there.  The reference adds the two as uint32, reads the wrapped length, and then fails the CRC
 * (with probability 1 - 2^-32) or panics on the slice.  seb_seg_scan lists such a record as its segment's last, and
 * every verify fails it. */
#define SEB_SEG_HEADER_BYTES 20u
#define SEB_HIDX_NO_RECORD UINT64_MAX

/* Host only.  seb_seg_scan: one segment image's sequential header walk, as seb_wal_scan but with the 20-byte header:
 * rec_off[0, *n) = the records' POOL offsets (base + file offset), *short_tail = 1 iff the image ends inside a header
 * or a payload (that tail is no record).  The walk trusts every header's sizes and looks at no CRC, so behind a
 * record that seb_seg_verify fails the offsets and *short_tail describe bytes that recover never reads: they mean
 * something only for a segment that is not cut (seb_hidx_recover reports short_tail = 0 for a cut one).
 * SEB_ERR_INVALID: more than cap records (bytes / 20 + 1 always suffice), a
 * NULL n or short_tail, NULL data with bytes != 0.
 * seb_seg_verify: records [seg_first[s], seg_first[s + 1]) belong to segment s (seg_first[0] = 0, seg_first[
 * num_segments] = num_records).  ok[r] (nullable) = record r lies whole inside the pool, passes the 2^32 rule and
 * its CRC matches; valid[s] = the records of segment s before its first bad one; size_after[s] = the segment's size
 * after recover: the cut offset, or its unchanged seg_bytes[s]; live[r] (nullable) = 1 iff r < seg_first[s] +
 * valid[s], the records the index is built from.
 * seb_hidx_lookup: the whole answer on the host, through a hash map built inside the call from the live records
 * (live nullable: all of them; one that does not lie inside the pool takes no part); no table layout is exposed.
 * keys in every seb_keys layout, host memory; rec, vloc, vlen and distinct are nullable; *distinct = the index's key
 * count.  It is the reference for the device form and what a caller without a GPU uses. */
int seb_seg_scan(const uint8_t *data, uint64_t bytes, uint64_t base, uint64_t *rec_off, uint64_t cap, uint64_t *n,
                 int *short_tail);
int seb_seg_verify(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, uint64_t num_records,
                   const uint64_t *seg_first, const uint64_t *seg_base, const uint64_t *seg_bytes, uint64_t num_segments,
                   uint8_t *ok, uint64_t *valid, uint64_t *size_after, uint8_t *live);
int seb_hidx_lookup(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, const uint8_t *live,
                    uint64_t num_records, const seb_keys *keys, int verify, uint8_t *status, uint64_t *rec, uint64_t *vloc,
                    uint32_t *vlen, uint64_t *distinct);

/* Device pointers (table 16-byte aligned; rec_off, seg_first, valid, rec, vloc and key offsets 8-byte aligned; vlen
 * 4-byte aligned; the pool, keys, ok, live, status and source at any byte alignment).  Not synchronised unless
 * stated.  SEB_ERR_INVALID and nothing launched: a NULL required pointer, a misaligned one, pool_bytes >= 2^47,
 * capacity > 2^40.
 *
 * The table is opaque: seb_dev_hidx_table_bytes(capacity) bytes (0 for capacity > 2^40), open addressing with linear
 * probing over the smallest power of two >= 2 * capacity slots.  seb_dev_hidx_clear empties it.
 * seb_dev_seg_verify: ok, valid (DEVICE memory here) and live (nullable) as seb_seg_verify gives them; size_after
 * follows on the host from valid, rec_off and the segments' bases.  Limits: fewer than 2^38 records, 2^32 segments.
 * seb_dev_hidx_insert: every record with live[r] != 0 (live nullable: all) goes into the table.  A record that does
 * not lie whole inside the pool is counted as bad and skipped.  The call may be repeated on the same table with
 * records at greater offsets (the active segment grew and the caller appended to the pool); the result equals one
 * insert of everything.  The pool must not change while an insert runs.
 * seb_dev_hidx_count SYNCHRONISES: *distinct = the occupied slots = the index's key count, *bad_records = the
 * skipped ones (both nullable).  SEB_ERR_RANGE: the table filled during an insert since the last clear (more than
 * capacity distinct keys); clear and insert again: a capacity of the live records cannot fail that way.
 * seb_dev_hidx_get: keys in the layouts seb_dev_shard_route takes; status required, rec / vloc / vlen / source
 * nullable; source[i] = 1 for a FOUND key (the pool holds its value), else 0.  NO INSERT MAY RUN CONCURRENTLY: the
 * probe reads the table with plain loads.  Bounds, whatever the table or the pool hold: every slot index is masked,
 * every record is re-checked against pool_bytes before a byte of it is read, the probe is a counted loop of at most
 * table-size steps, and nothing is written outside the keys->n elements of the five output arrays. */
uint64_t seb_dev_hidx_table_bytes(uint64_t capacity);
int seb_dev_hidx_clear(void *table, uint64_t capacity, void *stream);
int seb_dev_seg_verify(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, uint64_t num_records,
                       const uint64_t *seg_first, uint64_t num_segments, uint8_t *ok, uint64_t *valid, uint8_t *live,
                       void *stream);
int seb_dev_hidx_insert(void *table, uint64_t capacity, const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off,
                        const uint8_t *live, uint64_t num_records, void *stream);
int seb_dev_hidx_count(const void *table, uint64_t capacity, uint64_t *distinct, uint64_t *bad_records, void *stream);
int seb_dev_hidx_get(const void *table, uint64_t capacity, const uint8_t *pool, uint64_t pool_bytes, const seb_keys *keys,
                     int verify, uint8_t *status, uint64_t *rec, uint64_t *vloc, uint32_t *vlen, uint8_t *source,
                     void *stream);

/* recover() on a context; synchronous.  images[s] / image_bytes[s]: the segment files in HOST memory, oldest first.
 * dev_pool (DEVICE memory of pool_cap >= the images' total bytes) receives them back to back; dev_table (DEVICE
 * memory of seb_dev_hidx_table_bytes(capacity) bytes) is cleared and receives the index: scan on the host, upload,
 * verify, insert.  Host outputs per segment: valid, size_after, short_tail and cut (u8; both nullable); *records
 * (all scanned), *live_records (the sum of valid) and *distinct (the key count), each nullable.  SEB_ERR_RANGE: pool_cap
 * below the images' bytes (nothing is done), or the table filled: the per-segment outputs, *records and
 * *live_records are then filled, and a retry with capacity = *live_records cannot fail that way. */
int seb_hidx_recover(seb_ctx *ctx, const uint8_t *const *images, const uint64_t *image_bytes, uint64_t num_segments,
                     uint8_t *dev_pool, uint64_t pool_cap, void *dev_table, uint64_t capacity, uint64_t *valid,
                     uint64_t *size_after, uint8_t *short_tail, uint8_t *cut, uint64_t *records, uint64_t *live_records,
                     uint64_t *distinct);

/* ------------- hash index, write side: Put / Delete batches framed, segments compacted, the logical size ---- */
/* FRAME.  HashIndex.Put / Delete -> segment.append (hashindex/segment.go:61-125): op i becomes the record above
 * with `timestamp` (the reference's time.Now().Unix(); one per call: a caller that wants seconds to differ splits the
 * batch); Delete is Put(key, nil): valueSize 0, whatever value bytes the op carries.  Inputs as seb_wal_frame_* takes
 * them: keys in every seb_keys layout, vals + val_off (n + 1 non-decreasing offsets, val_off[0] may be != 0), deleted
 * nullable.  ROTATION (hashindex.go:92-215): a record goes to the active segment iff that segment's size is below
 * `limit` (SegmentSizeBytes, >= 1) BEFORE the append; otherwise the engine rotates once and the record opens the new
 * segment.  With active_size = the active segment's size before the batch: cut[k] = the first op of the k-th new
 * segment, ops [0, cut[0]) stay in the active one, and the image is the concatenation the engine splits at
 * rec_off[cut[k]].
 *
 * Refusals, SEB_ERR_INVALID with seb_last_error naming the lowest offender ("op I"), checked for every op before a
 * key or value byte is read and before anything is written: offsets that decrease; a key or a value of 2^32 bytes
 * or more; an EMPTY KEY (Put refuses it, hashindex.go:92-95); keySize + valueSize >= 2^32 (the read side's stated
 * departure; a Delete counts valueSize 0).  limit == 0: SEB_ERR_INVALID.  n < 2^32; n == 0 is valid and launches
 * nothing.
 *
 * Host: seb_seg_frame_plan writes rec_off[0..n] (nullable), cut[0..*ncuts) (nullable: the cuts are only counted),
 * *image_bytes and *ncuts (nullable).  cut_cap below the count: SEB_ERR_RANGE, *ncuts holds the need and nothing else
 * is written.  seb_seg_frame_emit writes the sealed image into image[0, image_bytes) (image_bytes not the plan's:
 * SEB_ERR_INVALID) and nothing outside it.
 * Device: device pointers (offsets 8-byte aligned; keys, vals, deleted and the image at any byte alignment) except
 * cut, image_bytes and ncuts, which are HOST memory.  seb_dev_seg_frame_plan writes rec_off[0..n] (required),
 * SYNCHRONISES once and fills cut, *image_bytes and *ncuts (both required).  The cuts are a chain of bisections over
 * rec_off in one lane, one link per new segment: a batch makes about image_bytes / limit of them.
 * seb_dev_seg_frame_emit (not synchronised) writes the records and seals them (the segment CRC kernel's seal mode).
 * Nothing is written outside the image and the n + 1 offsets, nothing is read outside the ops' arrays as their
 * offsets describe them; rec_off is trusted as seb_dev_wal_frame_emit trusts it. */
int seb_seg_frame_plan(const seb_keys *keys, const uint64_t *val_off, const uint8_t *deleted, uint64_t active_size,
                       uint64_t limit, uint64_t *rec_off, uint64_t *cut, uint64_t cut_cap, uint64_t *image_bytes,
                       uint64_t *ncuts);
int seb_seg_frame_emit(const seb_keys *keys, const uint8_t *vals, const uint64_t *val_off, const uint8_t *deleted,
                       uint64_t timestamp, uint8_t *image, uint64_t image_bytes);
int seb_dev_seg_frame_plan(const seb_keys *keys, const uint64_t *val_off, const uint8_t *deleted, uint64_t active_size,
                           uint64_t limit, uint64_t *rec_off, uint64_t *cut, uint64_t cut_cap, uint64_t *image_bytes,
                           uint64_t *ncuts, void *stream);
int seb_dev_seg_frame_emit(const seb_keys *keys, const uint8_t *vals, const uint64_t *val_off, const uint8_t *deleted,
                           uint64_t timestamp, const uint64_t *rec_off, uint8_t *image, uint64_t image_bytes,
                           void *stream);

/* COMPACTION.  compactSegments (hashindex/compaction.go:12-76) walks the chosen segments in list order, each from
 * offset 0; io.EOF (a short header, a payload past the end) ends that segment's walk silently, a CRC mismatch aborts
 * the whole compaction.  Each clean record sets latestValues[key]: the last one wins AMONG THE CHOSEN SEGMENTS ONLY (a
 * key with a newer record in an uncompacted segment is still written); keys whose winning value is empty are
 * dropped; every other key is appended to a new segment with a fresh timestamp.  An empty key found in a segment is
 * kept.  The reference writes the winners in a Go map's order; the SET is fully determined, and log order (the
 * winners in ascending position) is one of the orders it can produce: that order is fixed here, so the compacted
 * image is byte-exact.
 *
 * Input: the pool, and rec_off / live (nullable: all) for the records of the segments being compacted, in scan order
 * (seb_seg_scan + seb_seg_verify; choosing the segments is the caller's job, and so is refusing a compaction whose
 * verify found a bad record: these calls look at no CRC).  A live record that does not lie inside the pool:
 * SEB_ERR_INVALID naming it ("record R").  Output: the survivors in record order, each with `timestamp` and a fresh
 * CRC, and out_rec_off[0..survivors] = their offsets within the new image, ready for seb_dev_hidx_insert with the
 * image as (part of) a pool.  Zero survivors: image_bytes == 0 and only out_rec_off[0] is written.
 *
 * Host: seb_seg_compact with image == NULL and out_rec_off == NULL only sizes; image_cap below image_bytes or rec_cap
 * below survivors + 1 is SEB_ERR_RANGE with *sizes filled for a retry.
 * Device: the workspace (seb_dev_seg_compact_workspace_size(num_records) bytes of device memory, 16-byte aligned,
 * opaque; 0 for 2^38 records or more) carries the plan to the emit and must not be touched in between.  The plan builds
 * a scratch key table in it from these records alone (seb_dev_hidx_insert's kernel; the test-only hidx_hash_mask
 * applies), marks the survivors, scans their sizes, SYNCHRONISES and fills *sizes.  The emit (not synchronised; the
 * same pool, rec_off and workspace) places the offsets, copies by OUTPUT BYTES (16 per lane, whatever record they
 * belong to, so one long value does not hold a workgroup) and seals.  Its kernels check the workspace's header
 * against `sizes` and write nothing where it is another plan's; every source record is re-checked against pool_bytes
 * before a byte of it is read, and nothing is written outside image[0, image_bytes) and out_rec_off[0, survivors]. */
typedef struct seb_segcompact_sizes {
    uint64_t records_in, live_in;   /* the records given / those with live[r] != 0 */
    uint64_t distinct, survivors;   /* keys among the live records / records written */
    uint64_t tombstoned, shadowed;  /* keys dropped because their winning value is empty / live records that lost */
    uint64_t image_bytes, reserved;
} seb_segcompact_sizes;
int seb_seg_compact(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, const uint8_t *live,
                    uint64_t num_records, uint64_t timestamp, uint8_t *image, uint64_t image_cap, uint64_t *out_rec_off,
                    uint64_t rec_cap, seb_segcompact_sizes *sizes);
uint64_t seb_dev_seg_compact_workspace_size(uint64_t num_records);
int seb_dev_seg_compact_plan(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, const uint8_t *live,
                             uint64_t num_records, void *workspace, uint64_t workspace_bytes, seb_segcompact_sizes *sizes,
                             void *stream);
int seb_dev_seg_compact_emit(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, uint64_t num_records,
                             uint64_t timestamp, const seb_segcompact_sizes *sizes, void *workspace,
                             uint64_t workspace_bytes, uint8_t *image, uint64_t *out_rec_off, void *stream);

/* getLogicalSize (hashindex.go:360-385): the sum over the index entries, tombstoned keys included, of keySize +
 * valueSize: the denominator of the "space amplification > 3.0" compaction trigger.  Host: over the live records'
 * map, as seb_hidx_lookup builds it.  Device: a lane per slot of the table; SYNCHRONISES; *logical is HOST memory. */
int seb_hidx_logical_size(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, const uint8_t *live,
                          uint64_t num_records, uint64_t *logical);
int seb_dev_hidx_logical_size(const void *table, uint64_t capacity, const uint8_t *pool, uint64_t pool_bytes,
                              uint64_t *logical, void *stream);

/* compactSegments + applyCompaction on a context; synchronous.  dev_pool (DEVICE) holds the segments back to back,
 * oldest first, as seg_base / seg_bytes (HOST, num_segments each) describe them; the oldest compact_segments >= 1 of
 * them are compacted (choosing how many is the caller's job: doCompact's "oldest half").  Their bytes are scanned and
 * verified; ANY BAD RECORD in them is SEB_ERR_INVALID naming "segment S: record R", as the reference aborts, and
 * nothing is compacted; a short tail is not an error and its bytes are not copied.  Plan and emit go to the front of
 * dst_pool (DEVICE, dst_cap bytes, not overlapping dev_pool); the segments that stay are copied behind the new
 * image, and their live records' offsets rest_rec_off / rest_live (DEVICE; live nullable) are shifted:
 * new_rec_off (DEVICE, new_rec_cap >= survivors + rest_records + 1 entries) = the survivors' offsets, the shifted
 * ones, then the new pool's size.  dev_table is cleared and receives everything; the new image lies at the lowest
 * offsets, so newer segments still win: the table equals the live index after applyCompaction (compaction.go:78-132),
 * every Get answers as before, and *distinct drops by the keys whose latest record was a tombstone in a compacted
 * segment.  Rebuilding rather than editing the table in place is deliberate: linear probing has no delete.  Host
 * outputs: *sizes, new_seg_base / new_seg_bytes (num_segments - compact_segments + 1 each), *distinct (nullable).
 * SEB_ERR_RANGE: dst_cap or new_rec_cap is below the need (*sizes and the new segment arrays are filled; nothing is
 * written to the device outputs), or the table filled (seb_dev_hidx_count's rule). */
int seb_hidx_compact(seb_ctx *ctx, const uint8_t *dev_pool, uint64_t pool_bytes, const uint64_t *seg_base,
                     const uint64_t *seg_bytes, uint64_t num_segments, uint64_t compact_segments,
                     const uint64_t *rest_rec_off, const uint8_t *rest_live, uint64_t rest_records, uint64_t timestamp,
                     uint8_t *dst_pool, uint64_t dst_cap, void *dev_table, uint64_t capacity, uint64_t *new_rec_off,
                     uint64_t new_rec_cap, seb_segcompact_sizes *sizes, uint64_t *new_seg_base, uint64_t *new_seg_bytes,
                     uint64_t *distinct);

/* ------------- B-tree, read side: a page-file image checked, Get for a key batch ---- */
/* The reference's third engine (btree/) is a page-based B+-tree in one file.  This group is its read side: what
 * readMetadata (btree/pager.go:142-164) makes of the file, a structural check of every page, and what Get
 * (btree/btree.go:232-280) answers from the pages, for a key batch.  Range scans are the next group; the write side (Put,
 * splits, Delete, merges), the WAL's replay and the pager's cache stay with the caller, who hands over the image that Sync wrote, with
 * any WAL already applied.
 *
 * Layout (btree/page.go:9-44): page p at byte p * SEB_BT_PAGE_BYTES; every integer big-endian.  Page 0: magic,
 * RootPageID, NumPages, FreeListPtr at bytes 0, 4, 8, 12.  A page: [type u8: 1 internal, 2 leaf][numCells u16]
 * [rightPtr u32][freePtr u16][version u8], then a directory of u16 cell offsets IN KEY ORDER; the cells grow down from
 * the page end and deleted or updated ones leave dead bytes behind, so only the directory is sorted.  Version 0 or 1
 * is V1 (leaf cell: ks u16, vs u16, key, value; internal cell: ks u16, child u32, key); any other version byte is V2
 * (the sizes are varints of btree/varint.go:34-85; a value above 0xFFFF is an error).  An internal page's rightPtr is
 * its LEFTMOST child (keys below every cell); a leaf's is the next leaf, or 0.
 *
 * seb_bt_open is readMetadata: SEB_ERR_INVALID where the reference gives ErrInvalidDatabase (fewer than 4096 bytes, a
 * wrong magic).  meta->num_pages = min(NumPages, image_bytes / 4096) is the bound EVERY later page access is held to:
 * readPage's "out of bounds" and a file shorter than its header claims.
 *
 * seb_bt_check, the pass an open should be followed by.  kind[p] for p >= 1 (page 0 is SEB_BT_PAGE_BAD and is not
 * counted): a page is good, and kind[p] its type, when the type is 1 or 2; the directory fits (10 + 2 * numCells <=
 * 4096); every cell parses by CellAt's rules without a byte read outside the page; the directory's keys increase
 * strictly; an internal page's children and rightPtr lie in [1, num_pages); a leaf's rightPtr is 0 or in that range.
 * level[p] = the page's distance from the root over good internal pages, SEB_BT_NO_LEVEL where it has none within
 * SEB_BT_MAX_DEPTH pages (the root itself has level 0 whatever it holds, if its id lies in [1, num_pages)).  stats:
 * see the struct.  kind, level and stats are nullable.
 *
 * seb_bt_get.  Per key: SEB_GET_FOUND with leaf = the leaf reached, pos = the matched directory index, vloc = the
 * value's byte offset within the image (page * 4096 + cell offset + header + keySize), vlen = valueSize (0 is still
 * found); SEB_GET_MISS with leaf and pos = searchCell's insertion point (what Iterator.seek computes), vloc = vlen =
 * 0; SEB_GET_ERROR with leaf = the page it arose at, pos = vloc = vlen = 0.  The (status, vloc, vlen) arrays are the
 * ones seb_dev_get_values_* takes, with the image as its `pool`, source = 1 and num_runs = 0.
 * The bisection is fixed so that host and device agree on any bytes: a leaf is searchCell (btree/page.go:451-473)
 * literally; an internal page takes lo = 0, hi = n, mid = (lo + hi) / 2, key >= cell[mid].key ? lo = mid + 1 : hi =
 * mid, and descends to rightPtr when lo == 0, else to cell[lo - 1].child; on every page the check calls good that is
 * findChild's linear scan (btree/btree.go:200-229).
 * SEB_GET_ERROR: an empty key (ErrKeyEmpty; leaf = SEB_BT_NO_PAGE); a page id outside [1, num_pages) (leaf = that id);
 * and the DEPARTURES from the reference, which there walk garbage, panic or skip: a page whose type is neither 1 nor
 * 2 (the reference treats it as internal); a touched cell that fails to parse, or whose directory entry or V2 child id
 * lies past the page end (searchCell answers "not found", findChild skips the cell with `continue`, getCellOffset and
 * the child read panic); an internal page as the SEB_BT_MAX_DEPTH-th page of the walk (leaf = that page), which is
 * how a cycle ends (the reference loops for ever).
 * A key longer than 65,535 bytes is no stored key: it is compared by its first 65,536 bytes, which orders it exactly.
 *
 * Host forms: host memory, keys in every seb_keys layout; they are the reference for the device forms and what a
 * caller without a GPU uses.  SEB_ERR_INVALID: a NULL required pointer, meta->num_pages pages that do not fit
 * image_bytes, key offsets that decrease.
 * Device forms: device pointers (key offsets and vloc 8-byte aligned; leaf, pos and vlen 4-byte aligned; the IMAGE,
 * keys, kind, level, status and source at any byte alignment); meta and stats are HOST memory.  SEB_ERR_INVALID and
 * nothing launched: a NULL required pointer, a misaligned one, num_pages pages that do not fit image_bytes, more than
 * 2^31 pages (8 TiB).
 * seb_dev_bt_check SYNCHRONISES (one read-back per level round and one for the counts); seb_dev_bt_get does not;
 * source[i] (nullable) = 1 for a FOUND key, else 0.  Bounds, whatever the image holds: every page id is tested against
 * num_pages before a byte of the page is read, every offset against 4096 before it is used, both loops of the walk
 * are counted, and nothing is written outside the keys->n elements of the outputs (num_pages of kind and level). */
#define SEB_BT_PAGE_BYTES 4096u
#define SEB_BT_MAGIC 0x42545245u
#define SEB_BT_MAX_DEPTH 32u
#define SEB_BT_NO_PAGE UINT32_MAX
#define SEB_BT_NO_LEVEL 0xFFu
enum seb_bt_page_kind { SEB_BT_PAGE_BAD = 0, SEB_BT_PAGE_INTERNAL = 1, SEB_BT_PAGE_LEAF = 2 };
typedef struct seb_bt_meta {
    uint32_t root, header_pages; /* RootPageID, the header's NumPages */
    uint32_t free_list, num_pages; /* FreeListPtr, min(NumPages, image_bytes / 4096) */
} seb_bt_meta;
typedef struct seb_bt_stats {
    uint64_t leaves, internals, bad;                   /* pages [1, num_pages) by kind */
    uint64_t reach_leaves, reach_internals, reach_bad; /* those that have a level */
    uint64_t keys;           /* the cells on reachable good leaves: the key count Stats cannot give after a reopen */
    uint32_t depth, uniform; /* the levels that hold a page (0: the root lies outside); 1 iff every reachable good leaf
                              * sits at one level */
} seb_bt_stats;
int seb_bt_open(const uint8_t *image, uint64_t image_bytes, seb_bt_meta *meta);
int seb_bt_check(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, uint8_t *kind, uint8_t *level,
                 seb_bt_stats *stats);
int seb_bt_get(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, const seb_keys *keys, uint8_t *status,
               uint32_t *leaf, uint32_t *pos, uint64_t *vloc, uint32_t *vlen);
int seb_dev_bt_check(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, uint8_t *kind, uint8_t *level,
                     seb_bt_stats *stats, void *stream);
int seb_dev_bt_get(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, const seb_keys *keys, uint8_t *status,
                   uint32_t *leaf, uint32_t *pos, uint64_t *vloc, uint32_t *vlen, uint8_t *source, void *stream);
/* open, upload, check on a context; synchronous.  image: the file in HOST memory; dev_image (DEVICE memory of cap >=
 * meta->num_pages * 4096 bytes) receives its pages, dev_kind / dev_level (DEVICE, num_pages bytes each, nullable) the
 * check's arrays; *meta and *stats (nullable) are filled on the host.  SEB_ERR_INVALID as seb_bt_open; SEB_ERR_RANGE:
 * cap is below the pages' bytes (*meta is filled, nothing is uploaded). */
int seb_bt_load(seb_ctx *ctx, const uint8_t *image, uint64_t image_bytes, uint8_t *dev_image, uint64_t cap, uint8_t *dev_kind,
                uint8_t *dev_level, seb_bt_meta *meta, seb_bt_stats *stats);

/* ------------- B-tree, range scans: a leaf directory per image, Scan for a batch of ranges ---- */
/* BTree.Scan(startKey, endKey) (btree/btree.go, btree/iterator.go) for a batch of ranges [start, end).  The reference's
 * Iterator is serial: seek, then cell by cell and leaf by leaf along RightPtr.  Here the leaves' key order is derived
 * from the tree top-down, ONCE PER IMAGE after the check, into a LEAF DIRECTORY; the chain is only checked against that
 * order and never followed.  A range then costs two seeks (seb_bt_get's walk) and arithmetic on global key positions,
 * and every output entry is located on its own, so the work balances by entries and not by ranges.
 *
 * THE DIRECTORY: one flat buffer of seb_bt_dir_bytes(num_pages) bytes, 8-byte aligned, little-endian; the host form and
 * the device form write the same bytes.  Its arrays' offsets depend on num_pages alone (each has room for num_pages
 * leaves):
 *   [0, 32)                           u32 SEB_BT_DIR_MAGIC, u32 num_pages, u32 root, u32 leaves L, u64 keys, u32 depth, u32 0
 *   32                                leaf[num_pages] u32: the reachable leaves' page ids in key order; 0 from entry L on
 *   F = (32 + 4 num_pages + 7) & ~7   first[num_pages + 1] u64: the exclusive prefix sum of the leaves' numCells, first[L]
 *                                     = keys; 0 behind it
 *   F + 8 num_pages + 8               ord[num_pages] u32: a page's position in leaf[], SEB_BT_NO_PAGE for a page that is no
 *                                     listed leaf
 * It is built level by level from the root: level 0 is [root]; a level's pages hand on their children, the right
 * pointer FIRST (it is the leftmost child), then the cells' children in directory order; the first level that holds
 * leaves is leaf[].  kind and level are seb_bt_check's arrays, both required.
 * REFUSALS, each SEB_ERR_INVALID with "page P" in seb_last_error, tested in this order; the header is then zero and
 * nothing in the buffer means anything:
 *   the root lies outside [1, num_pages);
 *   per level r, the listed page at the least position that is bad by the check (or outside the image), else whose
 *     level is not r (a self-pointer, a page with parents at two levels), else whose kind differs from the kind of the
 *     level's first page (leaves at two levels);
 *   level SEB_BT_MAX_DEPTH - 1 holds internal pages (deeper than Get walks): names the level's first page;
 *   a level's children number more than num_pages (not a tree; it bounds the lists on a DAG): the level's first page;
 *   a leaf listed twice: the least such page id;
 *   the chain: the leaf at the least position i with RightPtr(leaf[i]) != leaf[i + 1], or != 0 on the last leaf;
 *   the order: the leaf at the least position whose last key is not strictly below the first key of the next
 *     NON-EMPTY leaf.
 * Chain and order make the position arithmetic below equal to a chain-following iterator on every accepted image.
 * seb_dev_bt_dir_build: device pointers (image, kind, level at any alignment); the workspace is
 * seb_dev_bt_dir_workspace_size(num_pages) bytes of device memory, 16-byte aligned, opaque; SYNCHRONISES (a read-back
 * per level, as the check); *info is HOST memory.
 *
 * SCAN.  starts / ends: two seb_keys of equal n; range r is [start_r, end_r).  An empty start means from the first key,
 * an empty end means unbounded (the reference's nil endKey; a caller with a non-nil empty endKey, for which the
 * reference yields nothing, answers that itself).  limit (0: none) caps each range's entries.  A bound is sought as
 * seb_bt_get walks; (leaf, pos) becomes the global position first[ord[leaf]] + pos; count = min(limit, max(0, last -
 * first)).  range_status[r] = 0, or SEB_GET_ERROR with no entries where a seek ended in ERROR or at a page the
 * directory does not list.  range_off[0..n] = the exclusive scan of the counts.  Per output entry e of range r, global
 * position g = first_r + (e - range_off[r]): status[e] = SEB_GET_FOUND, source[e] = 1, kloc / klen and vloc / vlen = the
 * key's and the value's place in the image; SEB_GET_ERROR with zero lengths where the cell no longer parses (the image
 * changed after the directory was built).  These arrays are what seb_dev_get_values_plan / _emit take with the image
 * as `pool` and num_runs = 0: one gather over (kloc, klen) gives key_off + keys, one over (vloc, vlen) val_off + values,
 * and range r's entries are a sorted run in the builder's input layout.
 * SEB_ERR_RANGE: 2^32 entries or more (the gather's limit; sizes->entries says how many).  SEB_ERR_INVALID: dir's
 * header is not this image's (magic, num_pages, root), a NULL or misaligned pointer, starts->n != ends->n.
 * Host form seb_bt_scan: all host memory; also the dense keys and values.  entry_cap / key_cap / val_cap below the
 * need: SEB_ERR_RANGE with *sizes filled for a retry (range_status and range_off are written all the same); NULL entry
 * outputs with caps of 0 only size.  It is the reference for the device form.
 * Device: seb_dev_bt_scan_plan (SYNCHRONISES; fills *sizes: ranges, entries; key_bytes and val_bytes stay 0, the
 * gathers size them) keeps range_off and first_r in the workspace (seb_dev_bt_scan_workspace_size(ranges) bytes, 8-byte
 * aligned, opaque; 0 for 2^32 ranges or more).  seb_dev_bt_scan_cells (not synchronised; the same image, dir and
 * workspace) writes range_off[0..ranges] and the six entry arrays, one lane per ENTRY; it writes nothing where the
 * workspace holds another plan.  Bounds, whatever the image or the directory holds: every ord / leaf / first index is
 * tested against L <= num_pages, every page id against num_pages, both bisections are counted, and nothing is written
 * outside ranges / ranges + 1 / entries elements.
 *
 * DEPARTURES from btree/iterator.go.  (1) Empty start: the reference's seek descends by CellAt(0).Child, which skips
 * the subtree under RightPtr (the leftmost, by findChild and GetChildPageID's own comment) at every level, and returns
 * an empty scan on an internal page without cells; here an empty start begins at the first key of the tree (on a
 * root-leaf tree both agree).  (2) An empty leaf inside the chain: the reference's Next moves to it and fails in
 * CellAt(0), or with a nil end hands out a nil key; here it contributes no entry and the scan goes on.  (3) Images the
 * directory refuses are still iterated by the reference; among them are the images its own splitInternal produces from
 * depth 3 on (the two leftmost children change places), which fail both the chain and the order rule. */
#define SEB_BT_DIR_MAGIC 0x42544452u
typedef struct seb_bt_dir_info {
    uint64_t leaves, keys;    /* L, first[L] */
    uint32_t depth, reserved; /* levels, the leaves' included */
} seb_bt_dir_info;
typedef struct seb_bt_scan_sizes {
    uint64_t ranges, entries;
    uint64_t key_bytes, val_bytes; /* host form only */
} seb_bt_scan_sizes;
uint64_t seb_bt_dir_bytes(uint32_t num_pages);
int seb_bt_dir_build(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, const uint8_t *kind,
                     const uint8_t *level, uint8_t *dir, seb_bt_dir_info *info);
int seb_bt_scan(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, const uint8_t *dir,
                const seb_keys *starts, const seb_keys *ends, uint64_t limit, uint8_t *range_status, uint64_t *range_off,
                uint8_t *status, uint8_t *source, uint64_t *kloc, uint32_t *klen, uint64_t *vloc, uint32_t *vlen,
                uint64_t entry_cap, uint64_t *key_off, uint8_t *keys, uint64_t key_cap, uint64_t *val_off, uint8_t *vals,
                uint64_t val_cap, seb_bt_scan_sizes *sizes);
uint64_t seb_dev_bt_dir_workspace_size(uint32_t num_pages);
int seb_dev_bt_dir_build(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, const uint8_t *kind,
                         const uint8_t *level, uint8_t *dir, void *workspace, uint64_t workspace_bytes,
                         seb_bt_dir_info *info, void *stream);
uint64_t seb_dev_bt_scan_workspace_size(uint64_t ranges);
int seb_dev_bt_scan_plan(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, const uint8_t *dir,
                         const seb_keys *starts, const seb_keys *ends, uint64_t limit, uint8_t *range_status,
                         void *workspace, uint64_t workspace_bytes, seb_bt_scan_sizes *sizes, void *stream);
int seb_dev_bt_scan_cells(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, const uint8_t *dir,
                          const seb_bt_scan_sizes *sizes, const void *workspace, uint64_t workspace_bytes,
                          uint64_t *range_off, uint8_t *status, uint8_t *source, uint64_t *kloc, uint32_t *klen,
                          uint64_t *vloc, uint32_t *vlen, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SEB_BLOOM_H */
