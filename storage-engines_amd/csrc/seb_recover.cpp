// seb_recover.cpp — the WAL replay's entry points: the C ABI over its host half (seb_memtable.cpp) and its
// kernels (seb_replay.hip), and seb_wal_recover, ReadAll + recoverFromWAL on host buffers through a context.
// Below them the batched memtable lookup's, over the same host file and seb_memget.hip, and seb_memtable_get;
// beside those the Get path's (seb_getpath.cpp, seb_getpath.hip): the compaction of undecided keys and the row join,
// and its last step's (seb_values.cpp, seb_values.hip): the found values gathered into one buffer.
#include <new>

#include "seb_getpath.h"
#include "seb_host.h"
#include "seb_memtable.h"
#include "seb_stage.h"
#include "seb_values.h"

using namespace seb;

// ------------------------------------------------ WAL replay (lsm/lsm.go:273-298, lsm/memtable.go:34-93,129-137)

static_assert(sizeof(seb_replay_sizes) == sizeof(seb::ReplaySizes) && sizeof(seb_replay_sizes) == 64, "seb_replay_sizes layout");

static const seb_replay_sizes kNoReplay = {0, 0, 0, 0, 0, 0, 0, 0};

static int replay_host_rc(int rc, uint64_t record, const char *who) {
    switch (rc) {
    case 0:
        return SEB_OK;
    case -2:
        return fail(SEB_ERR_INVALID, "%s: record %llu is not framed (its length is below 21 or is not 21 + keySize + "
                    "valueSize)", who, (unsigned long long)record);
    case -3:
        return fail(SEB_ERR_NOMEM, "%s: out of host memory", who);
    case -4:
        return fail(SEB_ERR_INVALID, "%s: 2^32 records or more", who);
    case -5:
        return fail(SEB_ERR_INVALID, "%s: sizes are not this input's plan", who);
    case -6:
        return fail(SEB_ERR_INVALID, "%s: record %llu: rec_off decreases or leaves [rec_off[0], rec_off[n]]", who,
                    (unsigned long long)record);
    default:
        return fail(SEB_ERR_INVALID, "%s: null argument", who);
    }
}

extern "C" int seb_wal_replay_plan(const uint8_t *data, const uint64_t *rec_off, uint64_t n, seb_replay_sizes *sizes) {
    uint64_t record = 0;
    const int rc = seb::replay_walk(data, rec_off, n, nullptr, nullptr, (seb::ReplaySizes *)sizes, &record);
    return replay_host_rc(rc, record, "seb_wal_replay_plan");
}

extern "C" int seb_wal_replay_emit(const uint8_t *data, const uint64_t *rec_off, uint64_t n, uint8_t *keys, uint64_t *key_off,
                                   uint8_t *vals, uint64_t *val_off, uint8_t *deleted, uint64_t *seq,
                                   const seb_replay_sizes *sizes) {
    const char *who = "seb_wal_replay_emit";
    if (!sizes) return fail(SEB_ERR_INVALID, "%s: null sizes", who);
    uint64_t record = 0;
    const seb::ReplayOut out{keys, key_off, vals, val_off, deleted, seq};
    seb::ReplaySizes got;
    int rc = seb::replay_walk(data, rec_off, n, &out, (const seb::ReplaySizes *)sizes, &got, &record);
    if (rc == 0 && memcmp(&got, sizes, sizeof got) != 0) rc = -5;
    return replay_host_rc(rc, record, who);
}

extern "C" uint64_t seb_dev_wal_replay_workspace_size(uint64_t n) {
    if (n >= (1ull << 32)) return 0;
    return replay_ws_layout(n).bytes;
}

extern "C" int seb_dev_wal_replay_plan(const uint8_t *data, const uint64_t *rec_off, uint64_t n, void *ws, uint64_t ws_bytes,
                                       seb_replay_sizes *sizes, void *stream) {
    const char *who = "seb_dev_wal_replay_plan";
    enter();
    if (!sizes) return fail(SEB_ERR_INVALID, "%s: null sizes", who);
    *sizes = kNoReplay;
    if (n >= (1ull << 32)) return replay_host_rc(-4, 0, who);
    if (n == 0) return SEB_OK;
    if (!data || !rec_off || ((uintptr_t)rec_off & 7)) return fail(SEB_ERR_INVALID, "%s: null data, or rec_off null or not 8-byte aligned", who);
    if (!ws || ((uintptr_t)ws & 15)) return fail(SEB_ERR_INVALID, "%s: the workspace is null or not 16-byte aligned", who);
    const uint64_t want = replay_ws_layout(n).bytes;
    if (ws_bytes < want)
        return fail(SEB_ERR_INVALID, "%s: workspace %llu < %llu bytes for %llu records", who, (unsigned long long)ws_bytes,
                    (unsigned long long)want, (unsigned long long)n);
    uint64_t err = 0;
    seb_replay_sizes got = kNoReplay;
    HIP_OR_FAIL(launch_replay_plan(data, rec_off, n, ws, &got, &err, (hipStream_t)stream));
    sizes->records_in = n;
    if (err != UINT64_MAX) return replay_host_rc(err & 1 ? -2 : -6, err >> 1, who);
    *sizes = got;
    return SEB_OK;
}

extern "C" int seb_dev_wal_replay_emit(const uint8_t *data, const uint64_t *rec_off, const seb_replay_sizes *sizes,
                                       const void *ws, uint64_t ws_bytes, uint8_t *keys, uint64_t *key_off, uint8_t *vals,
                                       uint64_t *val_off, uint8_t *deleted, uint64_t *seq, void *stream) {
    const char *who = "seb_dev_wal_replay_emit";
    enter();
    if (!sizes || !key_off || !val_off) return fail(SEB_ERR_INVALID, "%s: null argument", who);
    if (sizes->entries_out > sizes->records_in || sizes->records_in >= (1ull << 32) ||
        sizes->records_in - sizes->entries_out != sizes->overwritten || sizes->tombstones > sizes->entries_out ||
        sizes->key_bytes > (sizes->entries_out << 32) || sizes->val_bytes > (sizes->entries_out << 32) ||
        sizes->memtable_size != sizes->key_bytes + 16 * sizes->entries_out + sizes->val_bytes)
        return fail(SEB_ERR_INVALID, "%s: sizes are not a plan's", who);
    hipStream_t s = (hipStream_t)stream;
    if (sizes->records_in == 0) {  // nothing to launch: the two first offsets alone
        HIP_OR_FAIL(hipMemsetAsync(key_off, 0, 8, s));
        HIP_OR_FAIL(hipMemsetAsync(val_off, 0, 8, s));
        return SEB_OK;
    }
    if (!data || !rec_off || ((uintptr_t)rec_off & 7) || !ws || ((uintptr_t)ws & 15))
        return fail(SEB_ERR_INVALID, "%s: null data, rec_off or workspace, or one that is not aligned", who);
    if (ws_bytes < replay_emit_min_bytes(sizes->records_in))
        return fail(SEB_ERR_INVALID, "%s: workspace %llu bytes is not a plan's of %llu records", who,
                    (unsigned long long)ws_bytes, (unsigned long long)sizes->records_in);
    if ((sizes->entries_out && !deleted) || (sizes->key_bytes && !keys) || (sizes->val_bytes && !vals))
        return fail(SEB_ERR_INVALID, "%s: null output", who);
    bool ok = false;  // the plan synchronised, so reading the header back waits only for what the caller enqueued since
    HIP_OR_FAIL(replay_ws_check(sizes, ws, ws_bytes, &ok, s));
    if (!ok) return fail(SEB_ERR_INVALID, "%s: the workspace does not hold the plan that returned these sizes", who);
    HIP_OR_FAIL(launch_replay_emit(data, rec_off, sizes, ws, keys, key_off, vals, val_off, deleted, seq, s));
    return SEB_OK;
}

// Host buffers through the context: ReadAll's framing walk on the host, the image and its offsets up in one
// piece each, verify, plan and emit on the compute stream, and the six arrays back.
extern "C" int seb_wal_recover(seb_ctx *c, const uint8_t *image, uint64_t bytes, uint8_t *keys, uint64_t key_cap,
                               uint64_t *key_off, uint8_t *vals, uint64_t val_cap, uint64_t *val_off, uint8_t *deleted,
                               uint64_t *seq, uint64_t entry_cap, seb_replay_sizes *sizes) {
    const char *who = "seb_wal_recover";
    int rc;
    if (!c) return fail(SEB_ERR_INVALID, "%s: null ctx", who);
    if (!sizes || !key_off || !val_off || (bytes && !image)) return fail(SEB_ERR_INVALID, "%s: null argument", who);
    *sizes = kNoReplay;
    key_off[0] = val_off[0] = 0;
    if (bytes == 0) return SEB_OK;
    std::vector<uint64_t> off;
    std::vector<uint8_t> ok;
    uint64_t n = 0;
    try {
        off.resize(bytes / 21 + 2);
    } catch (const std::bad_alloc &) {
        return fail(SEB_ERR_NOMEM, "%s: out of host memory", who);
    }
    const int scan = seb_wal_scan(image, bytes, off.data(), off.size(), &n);
    if (scan != SEB_OK && scan != SEB_ERR_SHORT) return scan;
    const std::string tail = scan == SEB_ERR_SHORT ? last_error() : std::string();
    if (n >= (1ull << 32)) return replay_host_rc(-4, 0, who);
    if (n == 0) return scan == SEB_OK ? SEB_OK : fail(SEB_ERR_SHORT, "%s: %s", who, tail.c_str());
    try {
        ok.resize(n);
    } catch (const std::bad_alloc &) {
        return fail(SEB_ERR_NOMEM, "%s: out of host memory", who);
    }
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OR_FAIL(hipSetDevice(c->device));
    hipStream_t s = c->s_comp;
    Drain drain{s};
    Carver inc;  // the image, its records' offsets, a byte per record
    const uint64_t img_bytes = off[n], a_img = inc.take(img_bytes), a_off = inc.take(8 * (n + 1)), a_ok = inc.take(n);
    if ((rc = c->rpl_in.reserve(inc.bytes()))) return rc;
    uint8_t *in = section(c->rpl_in, a_img), *dok = section(c->rpl_in, a_ok);
    const uint64_t *doff = nullptr;
    if ((rc = upload(in, image, img_bytes, s)) || (rc = upload(&doff, section(c->rpl_in, a_off), off.data(), 8 * (n + 1), s)))
        return rc;
    if ((rc = seb_dev_wal_crc(in, doff, n, SEB_WAL_VERIFY, nullptr, dok, s))) return rc;
    if ((rc = download(ok.data(), dok, n, s))) return rc;
    HIP_OR_FAIL(hipStreamSynchronize(s));
    // ReadAll's order: it meets a complete record that fails its CRC before it meets the truncated tail
    for (uint64_t i = 0; i < n; ++i)
        if (!ok[i])
            return fail(SEB_ERR_INVALID, "%s: WAL corruption detected: CRC mismatch (record %llu)", who, (unsigned long long)i);
    if (scan == SEB_ERR_SHORT) return fail(SEB_ERR_SHORT, "%s: %s", who, tail.c_str());
    const uint64_t ws_bytes = replay_ws_layout(n).bytes;
    if ((rc = c->rpl_ws.reserve(ws_bytes, true))) return rc;
    if ((rc = seb_dev_wal_replay_plan(in, doff, n, c->rpl_ws.p, ws_bytes, sizes, s))) return rc;
    const RunDst dst{keys, key_cap, key_off, vals, val_cap, val_off, deleted, seq, entry_cap};
    if ((rc = check_run_dst(who, dst, sizes->entries_out, sizes->key_bytes, sizes->val_bytes))) return rc;
    const RunOut at(sizes->key_bytes, sizes->val_bytes, sizes->entries_out);
    if ((rc = c->rpl_out.reserve(at.bytes))) return rc;
    uint8_t *o = (uint8_t *)c->rpl_out.p;
    if ((rc = seb_dev_wal_replay_emit(in, doff, sizes, c->rpl_ws.p, ws_bytes, o, (uint64_t *)(o + at.koff), o + at.vals,
                                      (uint64_t *)(o + at.voff), o + at.del, seq ? (uint64_t *)(o + at.seq) : nullptr, s)))
        return rc;
    if ((rc = run_download(o, at, dst, s))) return rc;
    HIP_OR_FAIL(hipStreamSynchronize(s));
    return SEB_OK;
}

// ------------------------------------------------ batched memtable lookup (lsm/lsm.go:144-166, lsm/memtable.go:95-112)

static_assert(sizeof(seb_run) == sizeof(seb::Run) && sizeof(seb_run) == 56, "seb_run layout");
static_assert(SEB_MEM_MAX_RUNS == seb::kMemMaxRuns && SEB_MEM_MAX_RUNS == seb::kMemRuns, "SEB_MEM_MAX_RUNS");

// run < 0: the call has one run and does not number it
static int memget_rc(int rc, int run, uint64_t entry, const char *who) {
    char where[48] = "";
    if (run >= 0) snprintf(where, sizeof where, "run %d: ", run);
    const unsigned long long e = (unsigned long long)entry;
    switch (rc) {
    case 0:
        return SEB_OK;
    case -2:
        return fail(SEB_ERR_INVALID, "%s: %sentry %llu: key_off decreases, passes key_bytes or spans 2^32 bytes or more", who,
                    where, e);
    case -3:
        return fail(SEB_ERR_INVALID, "%s: %sentry %llu: val_off decreases or spans 2^32 bytes or more", who, where, e);
    case -4:
        return fail(SEB_ERR_INVALID, "%s: %sentry %llu is not above its predecessor (a run's keys increase strictly)", who,
                    where, e);
    case -5:
        return fail(SEB_ERR_INVALID, "%s: %s2^32 entries or more", who, where);
    case -6:
        return fail(SEB_ERR_INVALID, "%s: 2^32 keys or more", who);
    default:
        return fail(SEB_ERR_INVALID, "%s: a null argument, or more than %u runs", who, SEB_MEM_MAX_RUNS);
    }
}

extern "C" int seb_runs_search(const seb_keys *keys, const seb_run *runs, uint32_t num_runs, uint8_t *status, uint8_t *run,
                               uint32_t *entry, uint64_t *vloc, uint32_t *vlen, uint64_t *seq) {
    const char *who = "seb_runs_search";
    int rc;
    if ((rc = check_keys(keys, who)) || (rc = validate_offsets(keys, who))) return rc;
    uint32_t bad_run = 0;
    uint64_t bad_entry = 0;
    rc = seb::runs_search(seb::KeysView{keys->data, keys->offsets, keys->n, keys->stride}, (const seb::Run *)runs, num_runs,
                          status, run, entry, vloc, vlen, seq, &bad_run, &bad_entry);
    return memget_rc(rc, (int)bad_run, bad_entry, who);
}

extern "C" int seb_get_join(const uint8_t *mem_status, const uint8_t *sst_status, uint64_t n, uint8_t *status,
                            uint8_t *source) {
    if (seb::get_join(mem_status, sst_status, n, status, source) != 0)
        return fail(SEB_ERR_INVALID, "seb_get_join: null argument");
    return SEB_OK;
}

extern "C" uint64_t seb_dev_run_index_size(uint64_t n) { return n >= (1ull << 32) ? 0 : run_index_bytes(n); }

static int check_dev_run(const seb_run *r, const char *who) {
    if (r->n >= (1ull << 32)) return memget_rc(-5, -1, 0, who);
    if (r->n && (!r->key_off || !r->val_off || (!r->keys && r->key_bytes) || ((uintptr_t)r->key_off & 7) ||
                 ((uintptr_t)r->val_off & 7) || ((uintptr_t)r->seq & 7)))
        return fail(SEB_ERR_INVALID, "%s: a run's null key_off, val_off or keys, or offsets or seq that are not 8-byte aligned", who);
    return SEB_OK;
}

extern "C" int seb_dev_run_index(const seb_run *run, void *index, uint64_t index_bytes, void *stream) {
    const char *who = "seb_dev_run_index";
    enter();
    int rc;
    if (!run) return fail(SEB_ERR_INVALID, "%s: null run", who);
    if ((rc = check_dev_run(run, who))) return rc;
    if (run->n == 0) return SEB_OK;
    if (!index || ((uintptr_t)index & 15)) return fail(SEB_ERR_INVALID, "%s: the index is null or not 16-byte aligned", who);
    const uint64_t want = run_index_bytes(run->n);
    if (index_bytes < want)
        return fail(SEB_ERR_INVALID, "%s: index %llu < %llu bytes for %llu entries", who, (unsigned long long)index_bytes,
                    (unsigned long long)want, (unsigned long long)run->n);
    uint64_t err = 0;
    HIP_OR_FAIL(launch_run_index(run->keys, run->key_bytes, run->key_off, run->val_off, (uint32_t)run->n, index, &err,
                                 (hipStream_t)stream));
    if (err != UINT64_MAX) return memget_rc(-2 - (int)(err & 3), -1, err >> 2, who);
    return SEB_OK;
}

extern "C" int seb_dev_runs_search(const seb_keys *keys, const seb_run *runs, const void *const *index, uint32_t num_runs,
                                   uint8_t *status, uint8_t *run, uint32_t *entry, uint64_t *vloc, uint32_t *vlen,
                                   uint64_t *seq, void *stream) {
    const char *who = "seb_dev_runs_search";
    enter();
    int rc;
    if ((rc = check_keys(keys, who))) return rc;
    if (num_runs > SEB_MEM_MAX_RUNS || (num_runs && (!runs || !index))) return memget_rc(-1, -1, 0, who);
    if (keys->n >= (1ull << 32)) return memget_rc(-6, -1, 0, who);
    MemRunTab tab{};
    for (uint32_t r = 0; r < num_runs; ++r) {
        const seb_run &u = runs[r];
        if ((rc = check_dev_run(&u, who))) return rc;
        if (!u.n) continue;
        if (!index[r] || ((uintptr_t)index[r] & 15))
            return fail(SEB_ERR_INVALID, "%s: run %u: the index is null or not 16-byte aligned", who, r);
    }
    tab.nruns = num_runs;
    for (uint32_t r = 0; r < num_runs; ++r) {
        const seb_run &u = runs[r];
        MemRun &t = tab.r[r];
        if (!u.n) continue;  // n == 0: the bisection has no step and nothing of the run is read
        t = MemRun{run_index_prefixes(index[r]), u.key_off, u.val_off, u.keys, u.deleted, u.seq, u.key_bytes, (uint32_t)u.n,
                   0};
    }
    if (keys->n == 0) return SEB_OK;
    if (!status) return memget_rc(-1, -1, 0, who);
    HIP_OR_FAIL(launch_runs_search(key_batch(keys), tab, MemOut{status, run, entry, vloc, vlen, seq}, (hipStream_t)stream));
    return SEB_OK;
}

extern "C" int seb_dev_get_join(const uint8_t *mem_status, const uint8_t *sst_status, uint64_t n, uint8_t *status,
                                uint8_t *source, void *stream) {
    const char *who = "seb_dev_get_join";
    enter();
    if (n && (!mem_status || !sst_status || !status)) return fail(SEB_ERR_INVALID, "%s: null argument", who);
    HIP_OR_FAIL(launch_get_join(mem_status, sst_status, n, status, source, (hipStream_t)stream));
    return SEB_OK;
}

// ------------------------------------------------ Get path: undecided keys on to the SSTable steps (lsm/lsm.go:144-166)

static_assert(sizeof(seb_compact_sizes) == sizeof(seb::CompactSizes) && sizeof(seb_compact_sizes) == 32, "seb_compact_sizes layout");

static int compact_rc(int rc, uint64_t bad, const seb_compact_sizes *sz, const char *who) {
    switch (rc) {
    case 0:
        return SEB_OK;
    case -2:
        return fail(SEB_ERR_INVALID, "%s: 2^32 keys or more", who);
    case -3:
        return fail(SEB_ERR_INVALID, "%s: offsets decrease at %llu", who, (unsigned long long)bad);
    case -4:
        return fail(SEB_ERR_RANGE, "%s: a capacity is below its size (%llu rows, %llu key bytes); retry with *sizes", who,
                    (unsigned long long)sz->undecided, (unsigned long long)sz->key_bytes);
    default:
        return fail(SEB_ERR_INVALID, "%s: a null argument", who);
    }
}

extern "C" int seb_get_compact(const seb_keys *keys, const uint8_t *mem_status, seb_compact_sizes *sizes, uint8_t *out_keys,
                               uint64_t key_cap, uint64_t *out_off, uint32_t *row, uint64_t row_cap) {
    const char *who = "seb_get_compact";
    int rc;
    if ((rc = check_keys(keys, who))) return rc;
    uint64_t bad = 0;
    rc = seb::get_compact(seb::KeysView{keys->data, keys->offsets, keys->n, keys->stride}, mem_status,
                          (seb::CompactSizes *)sizes, out_keys, key_cap, out_off, row, row_cap, &bad);
    return compact_rc(rc, bad, sizes, who);
}

extern "C" int seb_get_join_rows(const uint8_t *mem_status, const uint64_t *mem_vloc, const uint32_t *mem_vlen, uint64_t n,
                                 const uint32_t *row, uint64_t m, const uint8_t *sst_status, const uint16_t *sst_col,
                                 const uint64_t *sst_vloc, const uint32_t *sst_vlen, uint8_t *status, uint8_t *source,
                                 uint16_t *col, uint64_t *vloc, uint32_t *vlen) {
    const int rc = seb::get_join_rows(mem_status, mem_vloc, mem_vlen, n, row, m, sst_status, sst_col, sst_vloc, sst_vlen,
                                      status, source, col, vloc, vlen);
    return compact_rc(rc, 0, nullptr, "seb_get_join_rows");
}

extern "C" uint64_t seb_dev_get_compact_workspace_size(uint64_t n) { return n >= (1ull << 32) ? 0 : compact_ws_bytes(n); }

extern "C" int seb_dev_get_compact_plan(const seb_keys *keys, const uint8_t *mem_status, void *workspace,
                                        uint64_t workspace_bytes, seb_compact_sizes *sizes, void *stream) {
    const char *who = "seb_dev_get_compact_plan";
    enter();
    int rc;
    if ((rc = check_keys(keys, who))) return rc;
    if (!sizes) return compact_rc(-1, 0, nullptr, who);
    *sizes = seb_compact_sizes{keys->n, 0, 0, 0};
    if (keys->n >= (1ull << 32)) return compact_rc(-2, 0, nullptr, who);
    if (keys->n == 0) return SEB_OK;
    if (!mem_status || !workspace) return compact_rc(-1, 0, nullptr, who);
    if (((uintptr_t)workspace & 15) || ((uintptr_t)keys->offsets & 7))
        return fail(SEB_ERR_INVALID, "%s: the workspace is not 16-byte aligned, or the offsets are not 8-byte aligned", who);
    const uint64_t want = compact_ws_bytes(keys->n);
    if (workspace_bytes < want)
        return fail(SEB_ERR_INVALID, "%s: workspace %llu < %llu bytes for %llu keys", who, (unsigned long long)workspace_bytes,
                    (unsigned long long)want, (unsigned long long)keys->n);
    HIP_OR_FAIL(launch_compact_plan(key_batch(keys), mem_status, workspace, sizes, (hipStream_t)stream));
    return SEB_OK;
}

extern "C" int seb_dev_get_compact_emit(const seb_keys *keys, const uint8_t *mem_status, const seb_compact_sizes *sizes,
                                        const void *workspace, uint8_t *out_keys, uint64_t *out_off, uint32_t *row,
                                        void *stream) {
    const char *who = "seb_dev_get_compact_emit";
    enter();
    int rc;
    if ((rc = check_keys(keys, who))) return rc;
    if (!sizes) return compact_rc(-1, 0, nullptr, who);
    if (keys->n >= (1ull << 32)) return compact_rc(-2, 0, nullptr, who);
    if (sizes->n != keys->n || sizes->undecided > sizes->n || (!keys->offsets && sizes->key_bytes != sizes->undecided * keys->stride))
        return fail(SEB_ERR_INVALID, "%s: sizes are not this batch's plan", who);
    if (keys->n == 0 || sizes->undecided == 0) return SEB_OK;
    if (!mem_status || !workspace || !row || (keys->offsets && !out_off) || (sizes->key_bytes && !out_keys))
        return compact_rc(-1, 0, nullptr, who);
    if (((uintptr_t)workspace & 15) || ((uintptr_t)keys->offsets & 7) || ((uintptr_t)out_off & 7) || ((uintptr_t)row & 3))
        return fail(SEB_ERR_INVALID, "%s: the workspace is not 16-byte aligned, offsets or out_off not 8-byte aligned, or row "
                    "not 4-byte aligned", who);
    HIP_OR_FAIL(launch_compact_emit(key_batch(keys), mem_status, sizes, workspace, out_keys, out_off, row, (hipStream_t)stream));
    return SEB_OK;
}

extern "C" int seb_dev_get_join_rows(const uint8_t *mem_status, const uint64_t *mem_vloc, const uint32_t *mem_vlen, uint64_t n,
                                     const uint32_t *row, uint64_t m, const uint8_t *sst_status, const uint16_t *sst_col,
                                     const uint64_t *sst_vloc, const uint32_t *sst_vlen, uint8_t *status, uint8_t *source,
                                     uint16_t *col, uint64_t *vloc, uint32_t *vlen, void *stream) {
    const char *who = "seb_dev_get_join_rows";
    enter();
    if (n >= (1ull << 32) || m >= (1ull << 32)) return compact_rc(-2, 0, nullptr, who);
    if ((n && (!mem_status || !status)) || (m && (!row || !sst_status))) return compact_rc(-1, 0, nullptr, who);
    HIP_OR_FAIL(launch_get_join_rows(mem_status, mem_vloc, mem_vlen, n, row, m, sst_status, sst_col, sst_vloc, sst_vlen, status,
                                     source, col, vloc, vlen, (hipStream_t)stream));
    return SEB_OK;
}

// ------------------------------------------------ Get values: the found values into one dense buffer (lsm/sstable.go:276-278)

static_assert(sizeof(seb_values_sizes) == sizeof(seb::ValuesSizes) && sizeof(seb_values_sizes) == 32, "seb_values_sizes layout");
static_assert(SEB_MEM_MAX_RUNS == seb::kValuesMaxRuns && SEB_MEM_MAX_RUNS == kMemRuns, "the runs a key may name");

static int values_rc(int rc, uint64_t bad, const seb_values_sizes *sz, const char *who) {
    switch (rc) {
    case 0:
        return SEB_OK;
    case -2:
        return fail(SEB_ERR_INVALID, "%s: 2^32 keys or more", who);
    case -3:
        return fail(SEB_ERR_INVALID, "%s: key %llu is found but its value does not lie inside the source it names", who,
                    (unsigned long long)bad);
    case -4:
        return fail(SEB_ERR_RANGE, "%s: val_cap is below the values' %llu bytes; retry with *sizes", who,
                    (unsigned long long)sz->val_bytes);
    case -5:
        return fail(SEB_ERR_INVALID, "%s: more than %u runs", who, SEB_MEM_MAX_RUNS);
    default:
        return fail(SEB_ERR_INVALID, "%s: a null argument", who);
    }
}

extern "C" int seb_get_values(const uint8_t *status, const uint8_t *source, const uint8_t *run, const uint64_t *vloc,
                              const uint32_t *vlen, uint64_t n, const uint8_t *const *vals, const uint64_t *val_bytes,
                              uint32_t num_runs, const uint8_t *pool, uint64_t pool_bytes, seb_values_sizes *sizes,
                              uint64_t *out_off, uint8_t *out_vals, uint64_t val_cap) {
    uint64_t bad = 0;
    const int rc = seb::get_values(status, source, run, vloc, vlen, n, ValueSources{vals, val_bytes, num_runs, pool, pool_bytes},
                                   (seb::ValuesSizes *)sizes, out_off, out_vals, val_cap, &bad);
    return values_rc(rc, bad, sizes, "seb_get_values");
}

extern "C" uint64_t seb_dev_get_values_workspace_size(uint64_t n) { return n >= (1ull << 32) ? 0 : values_ws_bytes(n); }

// The argument checks the plan and the emit share; *a is filled where they pass and n != 0.
static int values_args(const uint8_t *status, const uint8_t *source, const uint8_t *run, const uint64_t *vloc,
                       const uint32_t *vlen, uint64_t n, const uint8_t *const *vals, const uint64_t *val_bytes, uint32_t num_runs,
                       const uint8_t *pool, uint64_t pool_bytes, const void *workspace, ValuesArg *a, const char *who) {
    if (n >= (1ull << 32)) return values_rc(-2, 0, nullptr, who);
    if (num_runs > SEB_MEM_MAX_RUNS) return values_rc(-5, 0, nullptr, who);
    if ((num_runs && (!vals || !val_bytes)) || (pool_bytes && !pool)) return values_rc(-1, 0, nullptr, who);
    if (n == 0) return SEB_OK;
    if (!status || !source || !vloc || !vlen || !workspace || (num_runs > 1 && !run)) return values_rc(-1, 0, nullptr, who);
    if (((uintptr_t)workspace & 15) || ((uintptr_t)vloc & 7) || ((uintptr_t)vlen & 3))
        return fail(SEB_ERR_INVALID, "%s: the workspace is not 16-byte aligned, vloc not 8-byte aligned, or vlen not 4-byte "
                    "aligned", who);
    *a = ValuesArg{};
    a->status = status, a->source = source, a->run = run, a->vloc = vloc, a->vlen = vlen, a->n = n;
    for (uint32_t r = 0; r < num_runs; ++r) a->vals[r] = vals[r], a->val_bytes[r] = val_bytes[r];
    a->num_runs = num_runs, a->pool = pool, a->pool_bytes = pool_bytes;
    return SEB_OK;
}

extern "C" int seb_dev_get_values_plan(const uint8_t *status, const uint8_t *source, const uint8_t *run, const uint64_t *vloc,
                                       const uint32_t *vlen, uint64_t n, const uint8_t *const *vals, const uint64_t *val_bytes,
                                       uint32_t num_runs, const uint8_t *pool, uint64_t pool_bytes, void *workspace,
                                       uint64_t workspace_bytes, seb_values_sizes *sizes, void *stream) {
    const char *who = "seb_dev_get_values_plan";
    enter();
    if (!sizes) return values_rc(-1, 0, nullptr, who);
    *sizes = seb_values_sizes{n, 0, 0, 0};
    ValuesArg a;
    int rc;
    if ((rc = values_args(status, source, run, vloc, vlen, n, vals, val_bytes, num_runs, pool, pool_bytes, workspace, &a, who)))
        return rc;
    if (n == 0) return SEB_OK;
    const uint64_t want = values_ws_bytes(n);
    if (workspace_bytes < want)
        return fail(SEB_ERR_INVALID, "%s: workspace %llu < %llu bytes for %llu keys", who, (unsigned long long)workspace_bytes,
                    (unsigned long long)want, (unsigned long long)n);
    uint64_t bad = ~0ull;
    HIP_OR_FAIL(launch_values_plan(a, workspace, sizes, &bad, (hipStream_t)stream));
    return bad == ~0ull ? SEB_OK : values_rc(-3, bad, nullptr, who);
}

extern "C" int seb_dev_get_values_emit(const uint8_t *status, const uint8_t *source, const uint8_t *run, const uint64_t *vloc,
                                       const uint32_t *vlen, uint64_t n, const uint8_t *const *vals, const uint64_t *val_bytes,
                                       uint32_t num_runs, const uint8_t *pool, uint64_t pool_bytes, const seb_values_sizes *sizes,
                                       void *workspace, uint64_t *out_off, uint8_t *out_vals, void *stream) {
    const char *who = "seb_dev_get_values_emit";
    enter();
    if (!sizes) return values_rc(-1, 0, nullptr, who);
    ValuesArg a;
    int rc;
    if ((rc = values_args(status, source, run, vloc, vlen, n, vals, val_bytes, num_runs, pool, pool_bytes, workspace, &a, who)))
        return rc;
    if (sizes->n != n || sizes->found > sizes->n) return fail(SEB_ERR_INVALID, "%s: sizes are not this batch's plan", who);
    if (n == 0) return SEB_OK;
    if (!out_off || (sizes->val_bytes && !out_vals)) return values_rc(-1, 0, nullptr, who);
    if ((uintptr_t)out_off & 7) return fail(SEB_ERR_INVALID, "%s: out_off is not 8-byte aligned", who);
    HIP_OR_FAIL(launch_values_emit(a, sizes, workspace, out_off, out_vals, (hipStream_t)stream));
    return SEB_OK;
}

// Host buffers through the context: each run's key bytes, offsets, deleted bytes and sequences go up once
// (its values stay where they are: the answer is a location), its index is built, then a chunk of keys at a
// time on the compute stream (copy in, search, copy out), as seb_search_blocks does.
extern "C" int seb_memtable_get(seb_ctx *c, const seb_keys *kb, const seb_run *runs, uint32_t num_runs, uint8_t *status,
                                uint8_t *run, uint32_t *entry, uint64_t *vloc, uint32_t *vlen, uint64_t *seq) {
    const char *who = "seb_memtable_get";
    WsCall ws_call;
    int rc;
    if (!c) return fail(SEB_ERR_INVALID, "%s: null ctx", who);
    if ((rc = check_keys(kb, who)) || (rc = validate_offsets(kb, who))) return rc;
    if (num_runs > SEB_MEM_MAX_RUNS || (num_runs && !runs) || (kb->n && !status)) return memget_rc(-1, -1, 0, who);
    if (kb->n >= (1ull << 32)) return memget_rc(-6, -1, 0, who);
    uint32_t bad_run = 0;
    if ((rc = memget_rc(check_host_runs(runs, num_runs, SEB_MEM_MAX_RUNS, &bad_run), (int)bad_run, 0, who))) return rc;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OR_FAIL(hipSetDevice(c->device));
    hipStream_t s = c->s_comp;
    if ((rc = c->mg_runs.reserve(runs_upload_bytes(runs, nullptr, num_runs)))) return rc;
    Drain drain{s};
    RunUpload up;  // the values stay where they are: the answer is a location
    if ((rc = runs_upload(runs, nullptr, nullptr, num_runs, (uint8_t *)c->mg_runs.p, &up, s, who))) return rc;
    if (kb->n == 0) return SEB_OK;
    return chunks_serial(c, kb, [&](const KeyBatch &dk, const Chunk &ch) -> int {
        const uint64_t n = dk.n;
        Carver out;  // per key: vloc u64, seq u64, entry u32, vlen u32, status u8, run u8
        const uint64_t o_vloc = out.take(8 * n), o_seq = out.take(8 * n), o_ent = out.take(4 * n), o_vlen = out.take(4 * n),
                       o_st = out.take(n), o_run = out.take(n);
        if ((rc = c->mg_out.reserve(out.bytes()))) return rc;
        uint8_t *o = (uint8_t *)c->mg_out.p;
        const seb_keys dkeys{dk.data, dk.offsets, dk.n, dk.stride, 0};
        if ((rc = seb_dev_runs_search(&dkeys, up.drun, up.dindex, num_runs, o + o_st, o + o_run, (uint32_t *)(o + o_ent),
                                      (uint64_t *)(o + o_vloc), (uint32_t *)(o + o_vlen), (uint64_t *)(o + o_seq), s)))
            return rc;
        if ((rc = download(status + ch.i0, o + o_st, n, s)) || (rc = download(run ? run + ch.i0 : nullptr, o + o_run, n, s)) ||
            (rc = download(entry ? entry + ch.i0 : nullptr, o + o_ent, 4 * n, s)) ||
            (rc = download(vloc ? vloc + ch.i0 : nullptr, o + o_vloc, 8 * n, s)) ||
            (rc = download(vlen ? vlen + ch.i0 : nullptr, o + o_vlen, 4 * n, s)) ||
            (rc = download(seq ? seq + ch.i0 : nullptr, o + o_seq, 8 * n, s)))
            return rc;
        return SEB_OK;
    });
}
