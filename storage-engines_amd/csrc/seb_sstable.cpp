// seb_sstable.cpp — the entry points of the batched data-block search, of the batched SSTable
// builder and of the batched compaction merge: the C ABI over their host halves (seb_block.cpp) and
// their kernels (seb_search.hip, seb_sst.hip, seb_merge.hip), and the host-buffer forms through a context.
// Also the block-id step that feeds the search (seb_blockids.cpp, seb_blockids.hip).
#include <new>

#include "seb_block.h"
#include "seb_blockids.h"
#include "seb_host.h"
#include "seb_stage.h"

using namespace seb;

// ------------------------------------------------ batched data-block search (SSTable.Get's last step)

extern "C" int seb_block_search(const uint8_t *block, uint64_t len, const uint8_t *key, uint64_t key_len,
                                uint32_t *cell) {
    if (len > SEB_BLOCK_BYTES)
        return fail(SEB_ERR_INVALID, "seb_block_search: %llu bytes > the 4096 readBlock returns", (unsigned long long)len);
    if (seb::block_search(block, len, key, key_len, cell) != 0)
        return fail(SEB_ERR_INVALID, "seb_block_search: null argument");
    return SEB_OK;
}

extern "C" int seb_blocks_dedup(const uint64_t *files, const uint64_t *blocks, uint64_t cells, uint32_t *bid,
                                uint64_t *uniq_files, uint64_t *uniq_blocks, uint64_t uniq_cap, uint64_t *num_uniq) {
    switch (seb::blocks_dedup(files, blocks, cells, bid, uniq_files, uniq_blocks, uniq_cap, num_uniq)) {
    case 0:
        return SEB_OK;
    case -2:
        return fail(SEB_ERR_RANGE, "seb_blocks_dedup: %llu distinct blocks > uniq_cap %llu; retry with *num_uniq",
                    (unsigned long long)*num_uniq, (unsigned long long)uniq_cap);
    case -3:
        return fail(SEB_ERR_NOMEM, "seb_blocks_dedup: out of host memory");
    case -4:
        return fail(SEB_ERR_INVALID, "seb_blocks_dedup: more than 2^32 - 1 distinct blocks");
    default:
        return fail(SEB_ERR_INVALID, "seb_blocks_dedup: null argument");
    }
}

// ------------------------------------------------ block ids: (slot, block offset) cells into ids of the block pool

static_assert(sizeof(seb_blockids_sizes) == sizeof(seb::BlockIdSizes) && sizeof(seb_blockids_sizes) == 48, "seb_blockids_sizes layout");

static int blockids_rc(int rc, const seb_blockids_sizes *sz, uint64_t cap, const char *who) {
    switch (rc) {
    case 0:
        return SEB_OK;
    case -2:
        return fail(SEB_ERR_INVALID, "%s: 2^32 cells or more", who);
    case -3:
        return fail(SEB_ERR_NOMEM, "%s: out of host memory", who);
    case -4:
        return fail(SEB_ERR_RANGE, "%s: %llu distinct miss pairs > %llu; retry with *sizes", who,
                    (unsigned long long)sz->uniq, (unsigned long long)cap);
    case -5:
        return fail(SEB_ERR_INVALID, "%s: id_base + %llu ids pass 2^32 - 1", who, (unsigned long long)sz->uniq);
    default:
        return fail(SEB_ERR_INVALID, "%s: a null argument", who);
    }
}

extern "C" int seb_block_ids(const uint16_t *cand, const uint64_t *blocks, uint64_t cells, const uint32_t *res_first,
                             const uint32_t *res_count, uint32_t res_slots, uint32_t id_base, uint32_t *bid,
                             uint16_t *uniq_slot, uint64_t *uniq_block, uint64_t uniq_cap, seb_blockids_sizes *sizes) {
    const int rc = seb::block_ids(cand, blocks, cells, res_first, res_count, res_slots, id_base, bid, uniq_slot, uniq_block,
                                  uniq_cap, (seb::BlockIdSizes *)sizes);
    return blockids_rc(rc, sizes, uniq_cap, "seb_block_ids");
}

// the device forms' common refusals; SEB_OK with cells == 0 is the caller's to return early on
static int check_blockids_args(const uint16_t *cand, const uint64_t *blocks, uint64_t cells, const uint32_t *res_first,
                               const uint32_t *res_count, uint32_t res_slots, const char *who) {
    if (cells >= (1ull << 32)) return blockids_rc(-2, nullptr, 0, who);
    if ((cells && (!cand || !blocks)) || (res_slots && (!res_first || !res_count))) return blockids_rc(-1, nullptr, 0, who);
    if (((uintptr_t)cand & 1) || ((uintptr_t)blocks & 7) || ((uintptr_t)res_first & 3) || ((uintptr_t)res_count & 3))
        return fail(SEB_ERR_INVALID, "%s: cand is not 2-byte aligned, blocks not 8-byte or the residency table not 4-byte", who);
    return SEB_OK;
}

extern "C" int seb_dev_block_ids_resident(const uint16_t *cand, const uint64_t *blocks, uint64_t cells,
                                          const uint32_t *res_first, const uint32_t *res_count, uint32_t res_slots,
                                          uint32_t *bid, uint64_t *counts, void *stream) {
    const char *who = "seb_dev_block_ids_resident";
    enter();
    int rc;
    if ((rc = check_blockids_args(cand, blocks, cells, res_first, res_count, res_slots, who))) return rc;
    if (cells == 0) return SEB_OK;
    if (!bid) return blockids_rc(-1, nullptr, 0, who);
    if (((uintptr_t)bid & 3) || ((uintptr_t)counts & 7))
        return fail(SEB_ERR_INVALID, "%s: bid is not 4-byte aligned, or counts not 8-byte aligned", who);
    HIP_OR_FAIL(launch_blockids_resident(cand, blocks, cells, res_first, res_count, res_slots, bid, counts, (hipStream_t)stream));
    return SEB_OK;
}

extern "C" uint64_t seb_dev_block_ids_workspace_size(uint64_t cells, uint64_t max_uniq) {
    return cells >= (1ull << 32) ? 0 : blockids_ws_bytes(cells, max_uniq);
}

extern "C" int seb_dev_block_ids_plan(const uint16_t *cand, const uint64_t *blocks, uint64_t cells, const uint32_t *res_first,
                                      const uint32_t *res_count, uint32_t res_slots, uint64_t max_uniq, void *workspace,
                                      uint64_t workspace_bytes, seb_blockids_sizes *sizes, void *stream) {
    const char *who = "seb_dev_block_ids_plan";
    enter();
    int rc;
    if (!sizes) return blockids_rc(-1, nullptr, 0, who);
    *sizes = seb_blockids_sizes{cells, 0, 0, 0, 0, 0};
    if ((rc = check_blockids_args(cand, blocks, cells, res_first, res_count, res_slots, who))) return rc;
    if (cells == 0) return SEB_OK;
    if (!workspace) return blockids_rc(-1, nullptr, 0, who);
    if ((uintptr_t)workspace & 15) return fail(SEB_ERR_INVALID, "%s: the workspace is not 16-byte aligned", who);
    const uint64_t want = blockids_ws_bytes(cells, max_uniq);
    if (workspace_bytes < want)
        return fail(SEB_ERR_INVALID, "%s: workspace %llu < %llu bytes for %llu cells, max_uniq %llu", who,
                    (unsigned long long)workspace_bytes, (unsigned long long)want, (unsigned long long)cells,
                    (unsigned long long)max_uniq);
    bool overflow = false;
    HIP_OR_FAIL(launch_blockids_plan(cand, blocks, cells, res_first, res_count, res_slots, max_uniq, workspace, sizes, &overflow,
                                     (hipStream_t)stream));
    const uint64_t bound = blockids_max_uniq(cells, max_uniq);
    if (overflow || sizes->uniq > bound) return blockids_rc(-4, sizes, bound, who);
    return SEB_OK;
}

extern "C" int seb_dev_block_ids_emit(const uint16_t *cand, const uint64_t *blocks, uint64_t cells, const uint32_t *res_first,
                                      const uint32_t *res_count, uint32_t res_slots, uint64_t max_uniq, uint32_t id_base,
                                      const seb_blockids_sizes *sizes, const void *workspace, uint32_t *bid,
                                      uint16_t *uniq_slot, uint64_t *uniq_block, void *stream) {
    const char *who = "seb_dev_block_ids_emit";
    enter();
    int rc;
    if (!sizes) return blockids_rc(-1, nullptr, 0, who);
    if ((rc = check_blockids_args(cand, blocks, cells, res_first, res_count, res_slots, who))) return rc;
    if (sizes->cells != cells || sizes->uniq > blockids_max_uniq(cells, max_uniq) || sizes->uniq > sizes->misses ||
        sizes->resident > cells || sizes->misses > cells || sizes->bad > cells ||
        sizes->resident + sizes->misses + sizes->bad > cells)
        return fail(SEB_ERR_INVALID, "%s: sizes are not these cells' plan", who);
    if ((uint64_t)id_base + sizes->uniq > SEB_NO_BLOCK_ID) return blockids_rc(-5, sizes, 0, who);
    if (cells == 0) return SEB_OK;
    if (!workspace || !bid || (sizes->uniq && (!uniq_slot || !uniq_block))) return blockids_rc(-1, nullptr, 0, who);
    if (((uintptr_t)workspace & 15) || ((uintptr_t)bid & 3) || ((uintptr_t)uniq_slot & 1) || ((uintptr_t)uniq_block & 7))
        return fail(SEB_ERR_INVALID, "%s: the workspace is not 16-byte aligned, bid not 4-byte, uniq_slot not 2-byte or "
                    "uniq_block not 8-byte", who);
    HIP_OR_FAIL(launch_blockids_emit(cand, blocks, cells, res_first, res_count, res_slots, max_uniq, id_base, sizes, workspace,
                                     bid, uniq_slot, uniq_block, (hipStream_t)stream));
    return SEB_OK;
}

static int check_search_args(const seb_keys *keys, const void *bid, uint32_t cap, const uint8_t *pool, const void *blen,
                             uint32_t num_blocks, const char *who) {
    int rc;
    if ((rc = check_keys(keys, who))) return rc;
    if (cap == 0) return fail(SEB_ERR_INVALID, "%s: cap 0", who);
    if (!bid || (num_blocks && (!pool || !blen))) return fail(SEB_ERR_INVALID, "%s: null argument", who);
    return SEB_OK;
}

extern "C" int seb_dev_search_blocks(const seb_keys *keys, const uint32_t *bid, uint32_t cap, const uint8_t *pool,
                                     const uint16_t *blen, uint32_t num_blocks, uint32_t *cells, void *stream) {
    const char *who = "seb_dev_search_blocks";
    enter();
    int rc;
    if (!pool || !blen || !cells) return fail(SEB_ERR_INVALID, "%s: null argument", who);
    if ((rc = check_search_args(keys, bid, cap, pool, blen, num_blocks, who))) return rc;
    if ((uintptr_t)pool & 15) return fail(SEB_ERR_INVALID, "%s: the block pool is not 16-byte aligned", who);
    if (keys->n == 0) return SEB_OK;
    HIP_OR_FAIL(launch_search_blocks(key_batch(keys), bid, cap, pool, blen, num_blocks, cells, (hipStream_t)stream));
    return SEB_OK;
}

extern "C" int seb_dev_resolve_rows(const uint32_t *cells, const uint32_t *bid, uint64_t n, uint32_t cap,
                                    uint8_t *status, uint16_t *col, uint64_t *vloc, uint32_t *vlen, void *stream) {
    const char *who = "seb_dev_resolve_rows";
    enter();
    if (!cells || !bid || !status) return fail(SEB_ERR_INVALID, "%s: null argument", who);
    if (cap == 0) return fail(SEB_ERR_INVALID, "%s: cap 0", who);
    if (n == 0) return SEB_OK;
    HIP_OR_FAIL(launch_resolve_rows(cells, bid, n, cap, status, col, vloc, vlen, (hipStream_t)stream));
    return SEB_OK;
}

// Host buffers through the context: the pool and blen go up once, then a chunk of keys at a time on the
// compute stream (copy in, search, resolve, copy out), as seb_registry_locate does.
extern "C" int seb_search_blocks(seb_ctx *c, const seb_keys *kb, const uint32_t *bid, uint32_t cap,
                                 const uint8_t *pool, const uint16_t *blen, uint32_t num_blocks, uint8_t *status,
                                 uint16_t *col, uint64_t *vloc, uint32_t *vlen, uint32_t *cells) {
    const char *who = "seb_search_blocks";
    WsCall ws_call;
    int rc;
    if (!c) return fail(SEB_ERR_INVALID, "%s: null ctx", who);
    if ((rc = check_search_args(kb, bid, cap, pool, blen, num_blocks, who)) || (rc = validate_offsets(kb, who))) return rc;
    if (!status && kb->n) return fail(SEB_ERR_INVALID, "%s: null status", who);
    if (kb->n == 0) return SEB_OK;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OR_FAIL(hipSetDevice(c->device));
    const uint64_t pool_bytes = (uint64_t)num_blocks * SEB_BLOCK_BYTES;
    if ((rc = c->sb_pool.reserve(std::max<uint64_t>(pool_bytes, 16))) ||
        (rc = c->sb_blen.reserve(std::max<uint64_t>(2ull * num_blocks, 16))))
        return rc;
    if (num_blocks) {
        HIP_OR_FAIL(hipMemcpyAsync(c->sb_pool.p, pool, pool_bytes, hipMemcpyHostToDevice, c->s_comp));
        HIP_OR_FAIL(hipMemcpyAsync(c->sb_blen.p, blen, 2ull * num_blocks, hipMemcpyHostToDevice, c->s_comp));
    }
    return chunks_serial(c, kb, [&](const KeyBatch &dk, const Chunk &ch) -> int {
        const uint64_t n = dk.n, ncell = n * (uint64_t)cap;
        Carver out;  // per key: vloc u64, vlen u32, col u16, status u8
        const uint64_t o_vloc = out.take(8 * n), o_vlen = out.take(4 * n), o_col = out.take(2 * n), o_st = out.take(n);
        if ((rc = c->sb_bid.reserve(ncell * 4)) || (rc = c->sb_cells.reserve(ncell * 4)) ||
            (rc = c->sb_out.reserve(out.bytes())))
            return rc;
        uint8_t *o = (uint8_t *)c->sb_out.p;
        HIP_OR_FAIL(hipMemcpyAsync(c->sb_bid.p, bid + ch.i0 * cap, ncell * 4, hipMemcpyHostToDevice, c->s_comp));
        HIP_OR_FAIL(launch_search_blocks(dk, (const uint32_t *)c->sb_bid.p, cap, (const uint8_t *)c->sb_pool.p,
                                         (const uint16_t *)c->sb_blen.p, num_blocks, (uint32_t *)c->sb_cells.p,
                                         c->s_comp));
        HIP_OR_FAIL(launch_resolve_rows((const uint32_t *)c->sb_cells.p, (const uint32_t *)c->sb_bid.p, n, cap, o + o_st,
                                        (uint16_t *)(o + o_col), (uint64_t *)(o + o_vloc), (uint32_t *)(o + o_vlen), c->s_comp));
        if ((rc = download(status + ch.i0, o + o_st, n, c->s_comp)) ||
            (rc = download(col ? col + ch.i0 : nullptr, o + o_col, 2 * n, c->s_comp)) ||
            (rc = download(vloc ? vloc + ch.i0 : nullptr, o + o_vloc, 8 * n, c->s_comp)) ||
            (rc = download(vlen ? vlen + ch.i0 : nullptr, o + o_vlen, 4 * n, c->s_comp)) ||
            (rc = download(cells ? cells + ch.i0 * cap : nullptr, c->sb_cells.p, ncell * 4, c->s_comp)))
            return rc;
        return SEB_OK;
    });
}

// ------------------------------------------------ batched SSTable builder (lsm/sstable_builder.go)

static_assert(sizeof(seb_sst_sizes) == sizeof(seb::SstSizes) && sizeof(seb_sst_sizes) == 40, "seb_sst_sizes layout");

static int sst_host_rc(int rc, const seb_sst_sizes *sz, const char *who) {
    switch (rc) {
    case 0:
        return SEB_OK;
    case -2:
        return fail(SEB_ERR_INVALID, "%s: a key or a value of 2^32 bytes or more, or offsets that decrease", who);
    case -3:
        return fail(SEB_ERR_RANGE, "%s: a capacity is below its section (data %llu, index %llu, metadata %llu bytes)", who,
                    (unsigned long long)sz->data_bytes, (unsigned long long)sz->index_bytes,
                    (unsigned long long)sz->meta_bytes);
    default:
        return fail(SEB_ERR_INVALID, "%s: null argument", who);
    }
}

static seb::SstKeys sst_keys(const seb_keys *kb) { return seb::SstKeys{kb->data, kb->offsets, kb->n, kb->stride}; }

extern "C" int seb_sst_plan(const seb_keys *keys, const uint64_t *val_off, seb_sst_sizes *sizes) {
    int rc;
    if ((rc = check_keys(keys, "seb_sst_plan"))) return rc;
    return sst_host_rc(seb::sst_walk(sst_keys(keys), nullptr, val_off, nullptr, nullptr, (seb::SstSizes *)sizes), sizes,
                       "seb_sst_plan");
}

extern "C" int seb_sst_encode(const seb_keys *keys, const uint8_t *vals, const uint64_t *val_off, const uint8_t *deleted,
                              uint8_t *data, uint64_t data_cap, uint8_t *index, uint64_t index_cap, uint8_t *meta,
                              uint64_t meta_cap, seb_sst_sizes *sizes) {
    int rc;
    if ((rc = check_keys(keys, "seb_sst_encode"))) return rc;
    seb_sst_sizes local;
    if (!sizes) sizes = &local;
    const seb::SstOut out{data, index, meta, data_cap, index_cap, meta_cap};
    return sst_host_rc(seb::sst_walk(sst_keys(keys), vals, val_off, deleted, &out, (seb::SstSizes *)sizes), sizes,
                       "seb_sst_encode");
}

extern "C" int seb_sst_footer(uint64_t index_offset, uint64_t bloom_offset, uint64_t metadata_offset, uint8_t *out28) {
    if (!out28) return fail(SEB_ERR_INVALID, "seb_sst_footer: null output");
    seb::sst_footer(index_offset, bloom_offset, metadata_offset, out28);
    return SEB_OK;
}

extern "C" uint64_t seb_dev_sst_workspace_size(uint64_t n, uint32_t num_files) {
    return n == 0 || n >= (1ull << 32) ? 0 : sst_ws_layout(n, num_files).bytes;
}

static int check_sst_dev_args(const seb_keys *keys, const uint64_t *val_off, const uint64_t *file_begin,
                              uint32_t num_files, const void *ws, uint64_t ws_bytes, const char *who) {
    int rc;
    if ((rc = check_keys(keys, who))) return rc;
    if (!file_begin || num_files == 0) return fail(SEB_ERR_INVALID, "%s: no files", who);
    if (file_begin[0] != 0 || file_begin[num_files] != keys->n)
        return fail(SEB_ERR_INVALID, "%s: file_begin must run from 0 to n = %llu", who, (unsigned long long)keys->n);
    for (uint32_t f = 0; f < num_files; ++f)
        if (file_begin[f + 1] < file_begin[f]) return fail(SEB_ERR_INVALID, "%s: file_begin decreases at %u", who, f);
    if (keys->n == 0) return SEB_OK;
    if (keys->n >= (1ull << 32)) return fail(SEB_ERR_INVALID, "%s: n >= 2^32", who);
    if (!val_off) return fail(SEB_ERR_INVALID, "%s: null val_off", who);
    if (!ws || ((uintptr_t)ws & 15)) return fail(SEB_ERR_INVALID, "%s: the workspace is null or not 16-byte aligned", who);
    const uint64_t want = sst_ws_layout(keys->n, num_files).bytes;
    if (ws_bytes < want)
        return fail(SEB_ERR_INVALID, "%s: workspace %llu < %llu bytes", who, (unsigned long long)ws_bytes,
                    (unsigned long long)want);
    return SEB_OK;
}

extern "C" int seb_dev_sst_plan(const seb_keys *keys, const uint64_t *val_off, const uint64_t *file_begin,
                                uint32_t num_files, void *ws, uint64_t ws_bytes, seb_sst_sizes *sizes, void *stream) {
    const char *who = "seb_dev_sst_plan";
    enter();
    int rc;
    if ((rc = check_sst_dev_args(keys, val_off, file_begin, num_files, ws, ws_bytes, who))) return rc;
    if (!sizes) return fail(SEB_ERR_INVALID, "%s: null sizes", who);
    if (keys->n == 0) {  // every file is empty: a 4-byte index and 8 bytes of metadata each
        for (uint32_t f = 0; f < num_files; ++f) sizes[f] = seb_sst_sizes{0, 0, 4, 8, 0};
        return SEB_OK;
    }
    HIP_OR_FAIL(launch_sst_plan(key_batch(keys), val_off, file_begin, num_files, ws, sizes, (hipStream_t)stream));
    return SEB_OK;
}

extern "C" int seb_dev_sst_encode(const seb_keys *keys, const uint8_t *vals, const uint64_t *val_off,
                                  const uint8_t *deleted, const uint64_t *file_begin, uint32_t num_files,
                                  const seb_sst_sizes *sizes, const void *ws, uint64_t ws_bytes, uint8_t *data,
                                  uint16_t *blen, uint8_t *index, uint8_t *meta, void *stream) {
    const char *who = "seb_dev_sst_encode";
    enter();
    int rc;
    if ((rc = check_sst_dev_args(keys, val_off, file_begin, num_files, ws, ws_bytes, who))) return rc;
    if (!sizes) return fail(SEB_ERR_INVALID, "%s: null sizes", who);
    if (keys->n == 0) return SEB_OK;
    uint64_t blocks = 0, index_total = 0, meta_total = 0;
    for (uint32_t f = 0; f < num_files; ++f) {
        if (sizes[f].oversize_entries)
            return fail(SEB_ERR_RANGE, "%s: file %u has %llu oversized entries (a block longer than 4096 bytes): use "
                        "seb_sst_encode for it", who, f, (unsigned long long)sizes[f].oversize_entries);
        if (sizes[f].data_bytes != sizes[f].num_blocks * SEB_BLOCK_BYTES)
            return fail(SEB_ERR_INVALID, "%s: file %u: sizes are not a plan's", who, f);
        blocks += sizes[f].num_blocks;
        index_total += sizes[f].index_bytes;
        meta_total += sizes[f].meta_bytes;
    }
    if (blocks > keys->n) return fail(SEB_ERR_INVALID, "%s: sizes are not a plan's: more blocks than entries", who);
    if (!index || !meta || (blocks && !data)) return fail(SEB_ERR_INVALID, "%s: null output", who);
    if ((uintptr_t)data & 15) return fail(SEB_ERR_INVALID, "%s: the data section is not 16-byte aligned", who);
    HIP_OR_FAIL(launch_sst_encode(key_batch(keys), vals, val_off, deleted, num_files, ws, blocks, index_total, meta_total,
                                  data, blen, index, meta, (hipStream_t)stream));
    return SEB_OK;
}

// One file from host memory: the run goes up in one piece, the plan and the encode run on the compute
// stream, the filter is built from the keys already on the device, and the sections come back into
// `out` at their places.  A file with an oversized entry (or no entry) is encoded by the host half.
extern "C" int seb_sst_build(seb_ctx *c, const seb_keys *kb, const uint8_t *vals, const uint64_t *val_off,
                             const uint8_t *deleted, int64_t expected_keys, uint8_t *out, uint64_t cap, uint64_t *need) {
    const char *who = "seb_sst_build";
    int rc;
    if (!c) return fail(SEB_ERR_INVALID, "%s: null ctx", who);
    if ((rc = check_keys(kb, who))) return rc;
    const uint64_t n = kb->n;
    if (n && expected_keys == 0)
        return fail(SEB_ERR_INVALID, "%s: expected_keys == 0 with %llu entries (the reference's Add panics: integer "
                    "divide by zero)", who, (unsigned long long)n);
    uint64_t m = 0;
    uint32_t k = 0;
    if ((rc = seb_params(expected_keys, 0.01, &m, &k))) return rc;
    seb_sst_sizes sz;
    if ((rc = seb_sst_plan(kb, val_off, &sz))) return rc;
    const uint64_t nb = seb_num_bytes(m);
    const uint64_t o_index = sz.data_bytes, o_meta = o_index + sz.index_bytes, o_bloom = o_meta + sz.meta_bytes,
                   o_foot = o_bloom + 12 + nb, total = o_foot + SEB_SST_FOOTER_BYTES;
    if (need) *need = total;
    if (cap < total)
        return fail(SEB_ERR_RANGE, "%s: cap %llu < the file image's %llu bytes; retry with *need", who,
                    (unsigned long long)cap, (unsigned long long)total);
    if (!out) return fail(SEB_ERR_INVALID, "%s: null out", who);
    memcpy(out + o_bloom, &m, 8);  // Encode(): [numBits u64][numHashes u32][bits]
    memcpy(out + o_bloom + 8, &k, 4);
    seb::sst_footer(o_index, o_bloom, o_meta, out + o_foot);
    const bool on_host = n == 0 || sz.oversize_entries || n >= (1ull << 32);
    if (on_host) {
        rc = seb_sst_encode(kb, vals, val_off, deleted, out, sz.data_bytes, out + o_index, sz.index_bytes, out + o_meta,
                            sz.meta_bytes, nullptr);
        if (rc) return rc;
        if (n == 0) {
            memset(out + o_bloom + 12, 0, nb);
            return SEB_OK;
        }
    }
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OR_FAIL(hipSetDevice(c->device));
    hipStream_t s = c->s_comp;
    Drain drain{s};
    // the filter: NewBloomFilter(expected_keys, 0.01) + Add per key
    const uint64_t wb = seb_words_bytes(m);
    if ((rc = c->words.reserve(wb))) return rc;
    uint32_t *dw = (uint32_t *)c->words.p;
    HIP_OR_FAIL(hipMemsetAsync(dw, 0, wb, s));
    if ((rc = build_device_from_host(c, kb, dw, mod_arg(m, k)))) return rc;
    HIP_OR_FAIL(hipMemcpyAsync(out + o_bloom + 12, dw, nb, hipMemcpyDeviceToHost, s));
    if (on_host) {
        HIP_OR_FAIL(hipStreamSynchronize(s));
        return SEB_OK;
    }
    // the run on the device, and the three sections
    OpsOnDevice ops(kb, val_off);
    if ((ops.v1 - ops.v0) && !vals) return fail(SEB_ERR_INVALID, "%s: null vals", who);
    Carver in, outc;
    ops.carve(in, kb, deleted != nullptr);
    const uint64_t ws_bytes = sst_ws_layout(n, 1).bytes;
    const uint64_t a_data = outc.take(sz.data_bytes), a_index = outc.take(sz.index_bytes), a_metao = outc.take(sz.meta_bytes);
    if ((rc = c->sst_in.reserve(in.bytes())) || (rc = c->sst_ws.reserve(ws_bytes, true)) ||
        (rc = c->sst_out.reserve(outc.bytes())))
        return rc;
    uint8_t *dout = (uint8_t *)c->sst_out.p;
    if ((rc = ops.upload(section(c->sst_in, 0), kb, vals, val_off, deleted, s))) return rc;
    const KeyBatch dk = key_batch(&ops.keys);
    const uint64_t fbeg[2] = {0, n};
    seb_sst_sizes dsz;
    HIP_OR_FAIL(launch_sst_plan(dk, ops.val_off, fbeg, 1, c->sst_ws.p, &dsz, s));
    if (memcmp(&dsz, &sz, sizeof sz) != 0)
        return fail(SEB_ERR_INTERNAL, "%s: the device plan (%llu blocks, %llu index bytes) differs from the host's (%llu, %llu)",
                    who, (unsigned long long)dsz.num_blocks, (unsigned long long)dsz.index_bytes,
                    (unsigned long long)sz.num_blocks, (unsigned long long)sz.index_bytes);
    HIP_OR_FAIL(launch_sst_encode(dk, ops.vals, ops.val_off, ops.deleted, 1, c->sst_ws.p, sz.num_blocks, sz.index_bytes,
                                  sz.meta_bytes, dout + a_data, nullptr, dout + a_index, dout + a_metao, s));
    if ((rc = download(out, dout + a_data, sz.data_bytes, s)) || (rc = download(out + o_index, dout + a_index, sz.index_bytes, s)) ||
        (rc = download(out + o_meta, dout + a_metao, sz.meta_bytes, s)))
        return rc;
    HIP_OR_FAIL(hipStreamSynchronize(s));
    return SEB_OK;
}

// ------------------------------------------------ batched compaction merge (lsm/compaction.go:69-124,226-333)

static_assert(sizeof(seb_merge_sizes) == sizeof(seb::MergeSizes) && sizeof(seb_merge_sizes) == 48, "seb_merge_sizes layout");

extern "C" int seb_block_entries(const uint8_t *block, uint64_t len, uint16_t *entry_off, uint32_t cap, uint32_t *count) {
    const char *who = "seb_block_entries";
    if (len > SEB_BLOCK_BYTES)
        return fail(SEB_ERR_INVALID, "%s: %llu bytes > the 4096 readBlock returns", who, (unsigned long long)len);
    if (!count || (len && !block) || (cap && !entry_off)) return fail(SEB_ERR_INVALID, "%s: null argument", who);
    *count = seb::block_entries(block, len, entry_off, cap);
    if (*count > cap)
        return fail(SEB_ERR_RANGE, "%s: %u entries > cap %u; retry with *count", who, *count, cap);
    return SEB_OK;
}

static int merge_host_rc(int rc, uint32_t run, uint64_t entry, const char *who) {
    switch (rc) {
    case 0:
        return SEB_OK;
    case -2:
        return fail(SEB_ERR_INVALID, "%s: run %u entry %llu is not above its predecessor (every run must be strictly "
                    "increasing)", who, run, (unsigned long long)entry);
    case -3:
        return fail(SEB_ERR_NOMEM, "%s: out of host memory", who);
    case -4:
        return fail(SEB_ERR_INVALID, "%s: 2^32 entries or more", who);
    case -5:
        return fail(SEB_ERR_INVALID, "%s: sizes are not this input's plan", who);
    default:
        return fail(SEB_ERR_INVALID, "%s: null argument, or run_begin decreases", who);
    }
}

static int check_merge_runs(const uint64_t *run_begin, uint32_t num_runs, const char *who) {
    if (num_runs > SEB_MERGE_MAX_RUNS)
        return fail(SEB_ERR_INVALID, "%s: %u runs > SEB_MERGE_MAX_RUNS", who, num_runs);
    if (num_runs && !run_begin) return fail(SEB_ERR_INVALID, "%s: null run_begin", who);
    return SEB_OK;
}

extern "C" int seb_merge_plan(const uint8_t *pool, const uint16_t *blen, const uint64_t *run_begin, uint32_t num_runs,
                              uint32_t flags, seb_merge_sizes *sizes) {
    const char *who = "seb_merge_plan";
    int rc;
    if ((rc = check_merge_runs(run_begin, num_runs, who))) return rc;
    uint32_t run = 0;
    uint64_t entry = 0;
    rc = seb::merge_walk(pool, blen, run_begin, num_runs, flags, nullptr, nullptr, (seb::MergeSizes *)sizes, &run, &entry);
    return merge_host_rc(rc, run, entry, who);
}

extern "C" int seb_merge_emit(const uint8_t *pool, const uint16_t *blen, const uint64_t *run_begin, uint32_t num_runs,
                              uint32_t flags, uint8_t *keys, uint64_t *key_off, uint8_t *vals, uint64_t *val_off,
                              uint8_t *deleted, const seb_merge_sizes *sizes) {
    const char *who = "seb_merge_emit";
    int rc;
    if ((rc = check_merge_runs(run_begin, num_runs, who))) return rc;
    if (!sizes) return fail(SEB_ERR_INVALID, "%s: null sizes", who);
    uint32_t run = 0;
    uint64_t entry = 0;
    const seb::MergeOut out{keys, key_off, vals, val_off, deleted};
    seb::MergeSizes got;
    rc = seb::merge_walk(pool, blen, run_begin, num_runs, flags, &out, (const seb::MergeSizes *)sizes, &got, &run, &entry);
    if (rc == 0 && memcmp(&got, sizes, sizeof got) != 0) rc = -5;
    return merge_host_rc(rc, run, entry, who);
}

static int check_merge_dev_args(const uint8_t *pool, const uint16_t *blen, uint32_t num_blocks, const uint64_t *run_begin,
                                uint32_t num_runs, const void *block_entries, const char *who, bool aligned = true) {
    int rc;
    if ((rc = check_merge_runs(run_begin, num_runs, who))) return rc;
    if (num_runs == 0) {
        if (num_blocks) return fail(SEB_ERR_INVALID, "%s: %u blocks in no run", who, num_blocks);
        return SEB_OK;
    }
    if (run_begin[0] != 0 || run_begin[num_runs] != num_blocks)
        return fail(SEB_ERR_INVALID, "%s: run_begin must run from 0 to num_blocks = %u", who, num_blocks);
    for (uint32_t r = 0; r < num_runs; ++r)
        if (run_begin[r + 1] < run_begin[r]) return fail(SEB_ERR_INVALID, "%s: run_begin decreases at %u", who, r);
    if (num_blocks && (!pool || !blen || !block_entries)) return fail(SEB_ERR_INVALID, "%s: null argument", who);
    if (aligned && ((uintptr_t)pool & 15)) return fail(SEB_ERR_INVALID, "%s: the block pool is not 16-byte aligned", who);
    return SEB_OK;
}

extern "C" int seb_dev_merge_count(const uint8_t *pool, const uint16_t *blen, uint32_t num_blocks,
                                   const uint64_t *run_begin, uint32_t num_runs, uint16_t *block_entries,
                                   uint64_t *run_entries, void *stream) {
    const char *who = "seb_dev_merge_count";
    enter();
    int rc;
    if ((rc = check_merge_dev_args(pool, blen, num_blocks, run_begin, num_runs, block_entries, who))) return rc;
    if (run_entries)
        for (uint32_t r = 0; r < num_runs; ++r) run_entries[r] = 0;
    if (num_blocks == 0) return SEB_OK;
    hipStream_t s = (hipStream_t)stream;
    HIP_OR_FAIL(launch_merge_count(pool, blen, num_blocks, block_entries, s));
    std::vector<uint16_t> cnt;
    try {
        cnt.resize(run_entries ? num_blocks : 0);
    } catch (const std::bad_alloc &) {
        return fail(SEB_ERR_NOMEM, "%s: out of host memory", who);
    }
    if (run_entries) HIP_OR_FAIL(hipMemcpyAsync(cnt.data(), block_entries, 2ull * num_blocks, hipMemcpyDeviceToHost, s));
    HIP_OR_FAIL(hipStreamSynchronize(s));
    if (run_entries)
        for (uint32_t r = 0; r < num_runs; ++r)
            for (uint64_t b = run_begin[r]; b < run_begin[r + 1]; ++b) run_entries[r] += cnt[b];
    return SEB_OK;
}

extern "C" uint64_t seb_dev_merge_workspace_size(uint64_t entries, uint32_t num_blocks, uint32_t num_runs) {
    if (entries >= (1ull << 32) || num_runs > SEB_MERGE_MAX_RUNS) return 0;
    return merge_ws_layout(entries, num_blocks, num_runs).bytes;
}

extern "C" int seb_dev_merge_plan(const uint8_t *pool, const uint16_t *blen, uint32_t num_blocks,
                                  const uint64_t *run_begin, uint32_t num_runs, const uint16_t *block_entries,
                                  uint32_t flags, void *ws, uint64_t ws_bytes, seb_merge_sizes *sizes, void *stream) {
    const char *who = "seb_dev_merge_plan";
    enter();
    int rc;
    if ((rc = check_merge_dev_args(pool, blen, num_blocks, run_begin, num_runs, block_entries, who))) return rc;
    if (!sizes) return fail(SEB_ERR_INVALID, "%s: null sizes", who);
    *sizes = seb_merge_sizes{0, 0, 0, 0, 0, 0};
    if (num_blocks == 0) return SEB_OK;
    if (!ws || ((uintptr_t)ws & 15)) return fail(SEB_ERR_INVALID, "%s: the workspace is null or not 16-byte aligned", who);
    const uint64_t head = merge_ws_layout(0, num_blocks, num_runs).head_bytes;
    if (ws_bytes < head)
        return fail(SEB_ERR_INVALID, "%s: workspace %llu < %llu bytes", who, (unsigned long long)ws_bytes,
                    (unsigned long long)head);
    hipStream_t s = (hipStream_t)stream;
    try {
        std::vector<uint64_t> run_first((size_t)num_runs + 1);
        uint64_t n = 0;
        HIP_OR_FAIL(launch_merge_head(run_begin, num_runs, block_entries, num_blocks, ws, &n, run_first.data(), s));
        if (n >= (1ull << 32)) return fail(SEB_ERR_INVALID, "%s: 2^32 entries or more", who);
        sizes->entries_in = n;
        if (n == 0) return SEB_OK;
        const uint64_t want = merge_ws_layout(n, num_blocks, num_runs).bytes;
        if (ws_bytes < want)
            return fail(SEB_ERR_INVALID, "%s: workspace %llu < %llu bytes for %llu entries", who,
                        (unsigned long long)ws_bytes, (unsigned long long)want, (unsigned long long)n);
        uint64_t err = 0;
        HIP_OR_FAIL(launch_merge_decode(pool, blen, num_blocks, num_runs, n, ws, &err, s));
        if (err != UINT64_MAX)
            return merge_host_rc(-2, (uint32_t)(err >> 32), err & 0xFFFFFFFFull, who);
        HIP_OR_FAIL(launch_merge_tree(pool, num_blocks, num_runs, n, run_first.data(), flags, ws, sizes, s));
    } catch (const std::bad_alloc &) {
        return fail(SEB_ERR_NOMEM, "%s: out of host memory", who);
    }
    return SEB_OK;
}

extern "C" int seb_dev_merge_emit(const uint8_t *pool, const seb_merge_sizes *sizes, const void *ws, uint64_t ws_bytes,
                                  uint8_t *keys, uint64_t *key_off, uint8_t *vals, uint64_t *val_off, uint8_t *deleted,
                                  void *stream) {
    const char *who = "seb_dev_merge_emit";
    enter();
    if (!sizes || !key_off || !val_off) return fail(SEB_ERR_INVALID, "%s: null argument", who);
    if (sizes->entries_out > sizes->entries_in || sizes->entries_in >= (1ull << 32) ||
        sizes->entries_in - sizes->entries_out != sizes->shadowed + sizes->dropped ||
        sizes->key_bytes > 4096 * sizes->entries_out || sizes->val_bytes > 4096 * sizes->entries_out)
        return fail(SEB_ERR_INVALID, "%s: sizes are not a plan's", who);
    hipStream_t s = (hipStream_t)stream;
    if (sizes->entries_in == 0) {  // nothing to launch: the two first offsets alone
        HIP_OR_FAIL(hipMemsetAsync(key_off, 0, 8, s));
        HIP_OR_FAIL(hipMemsetAsync(val_off, 0, 8, s));
        return SEB_OK;
    }
    if (!pool || !ws || ((uintptr_t)ws & 15) || ((uintptr_t)pool & 15))
        return fail(SEB_ERR_INVALID, "%s: the pool or the workspace is null or not 16-byte aligned", who);
    if (ws_bytes < merge_emit_min_bytes(sizes->entries_in))
        return fail(SEB_ERR_INVALID, "%s: workspace %llu bytes is not a plan's of %llu entries", who,
                    (unsigned long long)ws_bytes, (unsigned long long)sizes->entries_in);
    if ((sizes->entries_out && !deleted) || (sizes->key_bytes && !keys) || (sizes->val_bytes && !vals))
        return fail(SEB_ERR_INVALID, "%s: null output", who);
    bool ok = false;  // the plan synchronised, so reading the header back waits only for what the caller enqueued since
    HIP_OR_FAIL(merge_ws_check(sizes, ws, ws_bytes, &ok, s));
    if (!ok) return fail(SEB_ERR_INVALID, "%s: the workspace does not hold the plan that returned these sizes", who);
    HIP_OR_FAIL(launch_merge_emit(pool, sizes, ws, keys, key_off, vals, val_off, deleted, s));
    return SEB_OK;
}

// Host buffers through the context: the pool and blen go up in one piece, count, plan and emit run on the
// compute stream, and the five arrays come back.
extern "C" int seb_merge(seb_ctx *c, const uint8_t *pool, const uint16_t *blen, uint32_t num_blocks,
                         const uint64_t *run_begin, uint32_t num_runs, uint32_t flags, uint8_t *keys, uint64_t key_cap,
                         uint64_t *key_off, uint8_t *vals, uint64_t val_cap, uint64_t *val_off, uint8_t *deleted,
                         uint64_t entry_cap, seb_merge_sizes *sizes) {
    const char *who = "seb_merge";
    int rc;
    if (!c) return fail(SEB_ERR_INVALID, "%s: null ctx", who);
    if (!sizes || !key_off || !val_off) return fail(SEB_ERR_INVALID, "%s: null argument", who);
    if ((rc = check_merge_dev_args(pool, blen, num_blocks, run_begin, num_runs, blen, who, false))) return rc;
    *sizes = seb_merge_sizes{0, 0, 0, 0, 0, 0};
    key_off[0] = val_off[0] = 0;
    if (num_blocks == 0) return SEB_OK;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OR_FAIL(hipSetDevice(c->device));
    hipStream_t s = c->s_comp;
    Drain drain{s};
    Carver inc;  // the pool, blen, each block's entry count
    const uint64_t pool_bytes = (uint64_t)num_blocks * SEB_BLOCK_BYTES, a_pool = inc.take(pool_bytes),
                   a_blen = inc.take(2ull * num_blocks), a_cnt = inc.take(2ull * num_blocks);
    if ((rc = c->mrg_in.reserve(inc.bytes()))) return rc;
    uint8_t *in = section(c->mrg_in, a_pool);
    uint16_t *dblen = (uint16_t *)section(c->mrg_in, a_blen), *dcnt = (uint16_t *)section(c->mrg_in, a_cnt);
    if ((rc = upload(in, pool, pool_bytes, s)) || (rc = upload((uint8_t *)dblen, blen, 2ull * num_blocks, s))) return rc;
    std::vector<uint64_t> run_entries;
    try {
        run_entries.resize(num_runs);
    } catch (const std::bad_alloc &) {
        return fail(SEB_ERR_NOMEM, "%s: out of host memory", who);
    }
    if ((rc = seb_dev_merge_count(in, dblen, num_blocks, run_begin, num_runs, dcnt, run_entries.data(), s))) return rc;
    uint64_t n = 0;
    for (uint64_t e : run_entries) n += e;
    if (n >= (1ull << 32)) return fail(SEB_ERR_INVALID, "%s: 2^32 entries or more", who);
    const uint64_t ws_bytes = merge_ws_layout(n, num_blocks, num_runs).bytes;
    if ((rc = c->mrg_ws.reserve(ws_bytes, true))) return rc;
    if ((rc = seb_dev_merge_plan(in, dblen, num_blocks, run_begin, num_runs, dcnt, flags, c->mrg_ws.p, ws_bytes, sizes, s)))
        return rc;
    const RunDst dst{keys, key_cap, key_off, vals, val_cap, val_off, deleted, nullptr, entry_cap};
    if ((rc = check_run_dst(who, dst, sizes->entries_out, sizes->key_bytes, sizes->val_bytes))) return rc;
    if (sizes->entries_in == 0) return SEB_OK;
    const RunOut at(sizes->key_bytes, sizes->val_bytes, sizes->entries_out, false);
    if ((rc = c->mrg_out.reserve(at.bytes))) return rc;
    uint8_t *o = (uint8_t *)c->mrg_out.p;
    if ((rc = seb_dev_merge_emit(in, sizes, c->mrg_ws.p, ws_bytes, o, (uint64_t *)(o + at.koff), o + at.vals,
                                 (uint64_t *)(o + at.voff), o + at.del, s)))
        return rc;
    if ((rc = run_download(o, at, dst, s))) return rc;
    HIP_OR_FAIL(hipStreamSynchronize(s));
    return SEB_OK;
}
