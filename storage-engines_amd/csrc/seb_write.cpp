// seb_write.cpp — the memtable write side's entry points: the C ABI over its host half (seb_memwrite.cpp) and its
// kernels (seb_memwrite.hip), and the host-buffer forms seb_memtable_apply and seb_memtable_fold on a context.
#include <new>

#include "seb_host.h"
#include "seb_memwrite.h"
#include "seb_stage.h"

using namespace seb;

static_assert(sizeof(seb_fold_sizes) == sizeof(seb::FoldSizes) && sizeof(seb_fold_sizes) == 64, "seb_fold_sizes layout");
static_assert(sizeof(seb_run) == sizeof(seb::Run), "seb_run layout");

static const seb_fold_sizes kNoFold = {0, 0, 0, 0, 0, 0, 0, 0};

// ------------------------------------------------ frame (lsm/lsm.go:97-137, lsm/wal.go:31-65)

static int frame_rc(int rc, uint64_t op, const char *who) {
    const unsigned long long i = (unsigned long long)op;
    switch (rc) {
    case 0:
        return SEB_OK;
    case -2:
        return fail(SEB_ERR_INVALID, "%s: op %llu: its key offsets decrease or its key has 2^32 bytes or more", who, i);
    case -3:
        return fail(SEB_ERR_INVALID, "%s: op %llu: its value offsets decrease or its value has 2^32 bytes or more", who, i);
    case -4:
        return fail(SEB_ERR_INVALID, "%s: 2^32 ops or more", who);
    case -5:
        return fail(SEB_ERR_INVALID, "%s: image_bytes is not this batch's plan", who);
    default:
        return fail(SEB_ERR_INVALID, "%s: null argument", who);
    }
}

static int check_ops(const seb_keys *keys, const uint64_t *val_off, const char *who) {
    int rc;
    if ((rc = check_keys(keys, who))) return rc;
    if (keys->n >= (1ull << 32)) return frame_rc(-4, 0, who);
    if (keys->n && !val_off) return frame_rc(-1, 0, who);
    return SEB_OK;
}

extern "C" int seb_wal_frame_plan(const seb_keys *keys, const uint64_t *val_off, const uint8_t *deleted, uint64_t *rec_off,
                                  uint64_t *image_bytes) {
    const char *who = "seb_wal_frame_plan";
    int rc;
    if ((rc = check_ops(keys, val_off, who))) return rc;
    uint64_t op = 0;
    rc = seb::frame_plan(KeysView{keys->data, keys->offsets, keys->n, keys->stride}, val_off, deleted, rec_off, image_bytes, &op);
    return frame_rc(rc, op, who);
}

extern "C" int seb_wal_frame_emit(const seb_keys *keys, const uint8_t *vals, const uint64_t *val_off, const uint8_t *deleted,
                                  uint64_t first_seq, uint8_t *image, uint64_t image_bytes) {
    const char *who = "seb_wal_frame_emit";
    int rc;
    if ((rc = check_ops(keys, val_off, who))) return rc;
    uint64_t op = 0;
    rc = seb::frame_emit(KeysView{keys->data, keys->offsets, keys->n, keys->stride}, vals, val_off, deleted, first_seq, image,
                         image_bytes, &op);
    return frame_rc(rc, op, who);
}

static int check_dev_ops(const seb_keys *keys, const uint64_t *val_off, const char *who) {
    int rc;
    if ((rc = check_ops(keys, val_off, who))) return rc;
    if (keys->n && (((uintptr_t)keys->offsets & 7) || ((uintptr_t)val_off & 7)))
        return fail(SEB_ERR_INVALID, "%s: offsets that are not 8-byte aligned", who);
    return SEB_OK;
}

extern "C" int seb_dev_wal_frame_plan(const seb_keys *keys, const uint64_t *val_off, const uint8_t *deleted,
                                      uint64_t *rec_off, uint64_t *image_bytes, void *stream) {
    const char *who = "seb_dev_wal_frame_plan";
    WsCall ws_call;
    enter();
    int rc;
    if ((rc = check_dev_ops(keys, val_off, who))) return rc;
    if (!image_bytes) return frame_rc(-1, 0, who);
    *image_bytes = 0;
    if (keys->n == 0) return SEB_OK;
    if (!rec_off || ((uintptr_t)rec_off & 7)) return fail(SEB_ERR_INVALID, "%s: rec_off is null or not 8-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    void *scratch = nullptr;
    if ((rc = cached_workspace(s, frame_scratch_bytes(keys->n), &scratch, 5))) return rc;
    uint64_t err = 0, bytes = 0;
    HIP_OR_FAIL(launch_frame_plan(key_batch(keys), val_off, deleted, rec_off, scratch, &bytes, &err, s));
    if (err != UINT64_MAX) return frame_rc(err & 1 ? -3 : -2, err >> 1, who);
    *image_bytes = bytes;
    return SEB_OK;
}

extern "C" int seb_dev_wal_frame_emit(const seb_keys *keys, const uint8_t *vals, const uint64_t *val_off,
                                      const uint8_t *deleted, uint64_t first_seq, const uint64_t *rec_off, uint8_t *image,
                                      uint64_t image_bytes, void *stream) {
    const char *who = "seb_dev_wal_frame_emit";
    enter();
    int rc;
    if ((rc = check_dev_ops(keys, val_off, who))) return rc;
    const uint64_t n = keys->n;
    if (n == 0) return image_bytes ? frame_rc(-5, 0, who) : SEB_OK;
    if (!rec_off || ((uintptr_t)rec_off & 7) || !image) return fail(SEB_ERR_INVALID, "%s: null image, or rec_off null or not 8-byte aligned", who);
    // a record has 21 bytes at least and 21 + 2 (2^32 - 1) at most
    if (image_bytes < 21 * n || image_bytes > n * (21 + 2 * 0xFFFFFFFFull)) return frame_rc(-5, 0, who);
    hipStream_t s = (hipStream_t)stream;
    HIP_OR_FAIL(launch_frame_emit(key_batch(keys), vals, val_off, deleted, first_seq, rec_off, image, image_bytes, s));
    return seb_dev_wal_crc(image, rec_off, n, SEB_WAL_SEAL, nullptr, nullptr, stream);
}

// ------------------------------------------------ runs: the shared checks

// run < 0: the call does not number the run; fresh: it is the new run
static int run_rc(int rc, int run, bool fresh, uint64_t entry, const char *who) {
    char where[48] = "";
    if (fresh)
        snprintf(where, sizeof where, "the new run: ");
    else if (run >= 0)
        snprintf(where, sizeof where, "run %d: ", run);
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
        return fail(SEB_ERR_INVALID, "%s: sizes are not these runs' plan", who);
    case -7:
        return fail(SEB_ERR_INVALID, "%s: run %d: val_off[n] passes the run's val_bytes", who, run);
    default:
        return fail(SEB_ERR_INVALID, "%s: a null argument, or too many runs", who);
    }
}

static int check_dev_run(const seb_run *r, int run, bool fresh, const char *who) {
    if (r->n >= (1ull << 32)) return run_rc(-5, run, fresh, 0, who);
    if (r->n && (!r->key_off || !r->val_off || (!r->keys && r->key_bytes) || ((uintptr_t)r->key_off & 7) ||
                 ((uintptr_t)r->val_off & 7) || ((uintptr_t)r->seq & 7)))
        return fail(SEB_ERR_INVALID, "%s: a run's null key_off, val_off or keys, or offsets or seq that are not 8-byte aligned", who);
    return SEB_OK;
}

static int fill_run_tab(const seb_run *runs, const void *const *index, uint32_t num_runs, MemRunTab *tab, const char *who) {
    int rc;
    *tab = MemRunTab{};
    tab->nruns = num_runs;
    for (uint32_t r = 0; r < num_runs; ++r) {
        const seb_run &u = runs[r];
        if ((rc = check_dev_run(&u, (int)r, false, who))) return rc;
        if (!u.n) continue;  // the bisection has no step and nothing of the run is read
        if (!index[r] || ((uintptr_t)index[r] & 15))
            return fail(SEB_ERR_INVALID, "%s: run %u: the index is null or not 16-byte aligned", who, r);
        tab->r[r] = MemRun{run_index_prefixes(index[r]), u.key_off, u.val_off, u.keys, u.deleted, u.seq, u.key_bytes, (uint32_t)u.n, 0};
    }
    return SEB_OK;
}

// ------------------------------------------------ size delta (lsm/memtable.go:34-93)

extern "C" int seb_run_size_delta(const seb_run *fresh, const seb_run *runs, uint32_t num_runs, int64_t *delta) {
    const char *who = "seb_run_size_delta";
    if (!fresh) return run_rc(-1, -1, false, 0, who);
    uint32_t bad_run = 0;
    uint64_t bad_entry = 0;
    const int rc = seb::run_size_delta(*(const seb::Run *)fresh, (const seb::Run *)runs, num_runs, delta, &bad_run, &bad_entry);
    return run_rc(rc, (int)bad_run, rc && rc != -1 && bad_run == num_runs, bad_entry, who);
}

extern "C" int seb_dev_run_size_delta(const seb_run *fresh, const seb_run *runs, const void *const *index, uint32_t num_runs,
                                      int64_t *delta, void *stream) {
    const char *who = "seb_dev_run_size_delta";
    enter();
    int rc;
    if (!fresh || !delta || ((uintptr_t)delta & 7) || num_runs > SEB_MEM_MAX_RUNS - 1 || (num_runs && (!runs || !index)))
        return run_rc(-1, -1, false, 0, who);
    if ((rc = check_dev_run(fresh, -1, true, who))) return rc;
    MemRunTab tab;
    if ((rc = fill_run_tab(runs, index, num_runs, &tab, who))) return rc;
    const MemRun f{nullptr, fresh->key_off, fresh->val_off, fresh->keys, fresh->deleted, fresh->seq, fresh->key_bytes,
                   (uint32_t)fresh->n, 0};
    HIP_OR_FAIL(launch_size_delta(f, tab, delta, (hipStream_t)stream));
    return SEB_OK;
}

// ------------------------------------------------ fold

extern "C" int seb_runs_fold_plan(const seb_run *runs, const uint64_t *val_bytes, uint32_t num_runs, seb_fold_sizes *sizes) {
    uint32_t bad_run = 0;
    uint64_t bad_entry = 0;
    const int rc = seb::runs_fold((const seb::Run *)runs, nullptr, val_bytes, num_runs, nullptr, nullptr, (seb::FoldSizes *)sizes,
                                  &bad_run, &bad_entry);
    return run_rc(rc, (int)bad_run, false, bad_entry, "seb_runs_fold_plan");
}

extern "C" int seb_runs_fold_emit(const seb_run *runs, const uint8_t *const *vals, const uint64_t *val_bytes, uint32_t num_runs,
                                  uint8_t *keys, uint64_t *key_off, uint8_t *out_vals, uint64_t *val_off, uint8_t *deleted,
                                  uint64_t *seq, const seb_fold_sizes *sizes) {
    const char *who = "seb_runs_fold_emit";
    if (!sizes) return run_rc(-1, -1, false, 0, who);
    uint32_t bad_run = 0;
    uint64_t bad_entry = 0;
    const seb::ReplayOut out{keys, key_off, out_vals, val_off, deleted, seq};
    seb::FoldSizes got;
    int rc = seb::runs_fold((const seb::Run *)runs, vals, val_bytes, num_runs, &out, (const seb::FoldSizes *)sizes, &got,
                            &bad_run, &bad_entry);
    if (rc == 0 && memcmp(&got, sizes, sizeof got) != 0) rc = -6;
    return run_rc(rc, (int)bad_run, false, bad_entry, who);
}

extern "C" uint64_t seb_dev_runs_fold_workspace_size(uint64_t entries) {
    return entries >= (1ull << 32) ? 0 : fold_ws_layout(entries).bytes;
}

static int fill_fold_tab(const seb_run *runs, const void *const *index, const uint8_t *const *vals, const uint64_t *val_bytes,
                         uint32_t num_runs, FoldTab *tab, uint64_t *entries, const char *who) {
    int rc;
    if (num_runs > SEB_MEM_MAX_RUNS || (num_runs && (!runs || !index || !val_bytes))) return run_rc(-1, -1, false, 0, who);
    *tab = FoldTab{};
    if ((rc = fill_run_tab(runs, index, num_runs, &tab->tab, who))) return rc;
    uint64_t total = 0;
    for (uint32_t r = 0; r < num_runs; ++r) {
        tab->begin[r] = total;
        total += runs[r].n;
        tab->val_bytes[r] = runs[r].n ? val_bytes[r] : 0;
        tab->vals[r] = vals && runs[r].n ? vals[r] : nullptr;
    }
    for (uint32_t r = num_runs; r <= SEB_MEM_MAX_RUNS; ++r) tab->begin[r] = total;
    if (total >= (1ull << 32)) return run_rc(-5, -1, false, 0, who);
    *entries = total;
    return SEB_OK;
}

extern "C" int seb_dev_runs_fold_plan(const seb_run *runs, const void *const *index, const uint64_t *val_bytes,
                                      uint32_t num_runs, void *ws, uint64_t ws_bytes, seb_fold_sizes *sizes, void *stream) {
    const char *who = "seb_dev_runs_fold_plan";
    enter();
    int rc;
    if (!sizes) return run_rc(-1, -1, false, 0, who);
    *sizes = kNoFold;
    FoldTab tab;
    uint64_t entries = 0;
    if ((rc = fill_fold_tab(runs, index, nullptr, val_bytes, num_runs, &tab, &entries, who))) return rc;
    if (entries == 0) return SEB_OK;
    if (!ws || ((uintptr_t)ws & 15)) return fail(SEB_ERR_INVALID, "%s: the workspace is null or not 16-byte aligned", who);
    const uint64_t want = fold_ws_layout(entries).bytes;
    if (ws_bytes < want)
        return fail(SEB_ERR_INVALID, "%s: workspace %llu < %llu bytes for %llu entries", who, (unsigned long long)ws_bytes,
                    (unsigned long long)want, (unsigned long long)entries);
    uint64_t err = 0;
    seb_fold_sizes got = kNoFold;
    HIP_OR_FAIL(launch_fold_plan(tab, entries, ws, &got, &err, (hipStream_t)stream));
    sizes->entries_in = entries;
    if (err != UINT64_MAX) return run_rc(-7, (int)err, false, 0, who);
    *sizes = got;
    return SEB_OK;
}

extern "C" int seb_dev_runs_fold_emit(const seb_run *runs, const void *const *index, const uint8_t *const *vals,
                                      const uint64_t *val_bytes, uint32_t num_runs, const seb_fold_sizes *sizes, const void *ws,
                                      uint64_t ws_bytes, uint8_t *keys, uint64_t *key_off, uint8_t *out_vals, uint64_t *val_off,
                                      uint8_t *deleted, uint64_t *seq, void *stream) {
    const char *who = "seb_dev_runs_fold_emit";
    enter();
    int rc;
    if (!sizes || !key_off || !val_off) return run_rc(-1, -1, false, 0, who);
    FoldTab tab;
    uint64_t entries = 0;
    if ((rc = fill_fold_tab(runs, index, vals, val_bytes, num_runs, &tab, &entries, who))) return rc;
    if (sizes->entries_in != entries || sizes->entries_out > entries || entries - sizes->entries_out != sizes->shadowed ||
        sizes->tombstones > sizes->entries_out || sizes->key_bytes > (sizes->entries_out << 32) ||
        sizes->val_bytes > (sizes->entries_out << 32) ||
        sizes->memtable_size != sizes->key_bytes + 16 * sizes->entries_out + sizes->val_bytes)
        return run_rc(-6, -1, false, 0, who);
    hipStream_t s = (hipStream_t)stream;
    if (entries == 0) {  // nothing to launch: the two first offsets alone
        HIP_OR_FAIL(hipMemsetAsync(key_off, 0, 8, s));
        HIP_OR_FAIL(hipMemsetAsync(val_off, 0, 8, s));
        return SEB_OK;
    }
    if (!ws || ((uintptr_t)ws & 15) || ws_bytes < fold_ws_layout(entries).bytes)
        return fail(SEB_ERR_INVALID, "%s: the workspace is null, not 16-byte aligned or not a plan's of %llu entries", who,
                    (unsigned long long)entries);
    if ((sizes->entries_out && !deleted) || (sizes->key_bytes && !keys) || (sizes->val_bytes && !out_vals))
        return fail(SEB_ERR_INVALID, "%s: null output", who);
    for (uint32_t r = 0; r < num_runs; ++r)
        if (runs[r].n && val_bytes[r] && (!vals || !vals[r])) return fail(SEB_ERR_INVALID, "%s: run %u: null vals", who, r);
    bool ok = false;  // the plan synchronised, so reading the header back waits only for what the caller enqueued since
    HIP_OR_FAIL(fold_ws_check(sizes, ws, &ok, s));
    if (!ok) return fail(SEB_ERR_INVALID, "%s: the workspace does not hold the plan that returned these sizes", who);
    HIP_OR_FAIL(launch_fold_emit(tab, sizes, ws, keys, key_off, out_vals, val_off, deleted, seq, s));
    return SEB_OK;
}

// ------------------------------------------------ the host-buffer forms


extern "C" int seb_memtable_apply(seb_ctx *c, const seb_keys *kb, const uint8_t *vals, const uint64_t *val_off,
                                  const uint8_t *deleted, uint64_t first_seq, const seb_run *runs, uint32_t num_runs,
                                  uint8_t *image, uint64_t image_cap, uint64_t *image_bytes, uint8_t *run_keys, uint64_t key_cap,
                                  uint64_t *run_key_off, uint8_t *run_vals, uint64_t val_cap, uint64_t *run_val_off,
                                  uint8_t *run_deleted, uint64_t *run_seq, uint64_t entry_cap, seb_replay_sizes *sizes,
                                  int64_t *size_delta, uint64_t *sequence) {
    const char *who = "seb_memtable_apply";
    WsCall ws_call;
    int rc;
    if (!c) return fail(SEB_ERR_INVALID, "%s: null ctx", who);
    if (!image_bytes || !sizes || !size_delta || !sequence || !run_key_off || !run_val_off) return frame_rc(-1, 0, who);
    if ((rc = check_ops(kb, val_off, who)) || (rc = validate_offsets(kb, who))) return rc;
    uint32_t bad_run = 0;
    if ((rc = run_rc(check_host_runs(runs, num_runs, SEB_MEM_MAX_RUNS - 1, &bad_run), (int)bad_run, false, 0, who))) return rc;
    const uint64_t n = kb->n;
    *image_bytes = 0;
    *sizes = seb_replay_sizes{0, 0, 0, 0, 0, 0, 0, 0};
    *size_delta = 0;
    *sequence = first_seq - 1 + n;
    run_key_off[0] = run_val_off[0] = 0;
    if (n == 0) return SEB_OK;
    if (val_off[n] < val_off[0]) return frame_rc(-3, 0, who);
    if (!kb->data && (kb->offsets || kb->stride)) return frame_rc(-1, 0, who);
    OpsOnDevice ops(kb, val_off);
    if (ops.v1 > ops.v0 && !vals) return frame_rc(-1, 0, who);
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OR_FAIL(hipSetDevice(c->device));
    hipStream_t s = c->s_comp;
    Carver in;  // the ops, their records' offsets, the size delta
    ops.carve(in, kb, deleted != nullptr);
    const uint64_t i_rec = in.take(8 * (n + 1)), i_delta = in.take(8);
    if ((rc = c->mw_in.reserve(in.bytes()))) return rc;
    Drain drain{s};
    if ((rc = ops.upload(section(c->mw_in, 0), kb, vals, val_off, deleted, s))) return rc;
    uint64_t *drec = (uint64_t *)section(c->mw_in, i_rec);
    // frame and seal
    if ((rc = seb_dev_wal_frame_plan(&ops.keys, ops.val_off, ops.deleted, drec, image_bytes, s))) return rc;
    const uint64_t img = *image_bytes;
    if ((rc = c->mw_img.reserve(img))) return rc;
    uint8_t *dimg = (uint8_t *)c->mw_img.p;
    if ((rc = seb_dev_wal_frame_emit(&ops.keys, ops.vals, ops.val_off, ops.deleted, first_seq, drec, dimg, img, s))) return rc;
    // replay: the batch's run
    const uint64_t ws_bytes = replay_ws_layout(n).bytes;
    if ((rc = c->mw_ws.reserve(ws_bytes, true))) return rc;
    if ((rc = seb_dev_wal_replay_plan(dimg, drec, n, c->mw_ws.p, ws_bytes, sizes, s))) return rc;
    const RunDst dst{run_keys, key_cap, run_key_off, run_vals, val_cap, run_val_off, run_deleted, run_seq, entry_cap};
    if ((rc = check_run_dst(who, dst, sizes->entries_out, sizes->key_bytes, sizes->val_bytes, &img, image_cap, image))) return rc;
    if ((rc = download(image, dimg, img, s))) return rc;
    const RunOut at(sizes->key_bytes, sizes->val_bytes, sizes->entries_out);
    if ((rc = c->mw_out.reserve(at.bytes))) return rc;
    uint8_t *o = (uint8_t *)c->mw_out.p;
    if ((rc = seb_dev_wal_replay_emit(dimg, drec, sizes, c->mw_ws.p, ws_bytes, o, (uint64_t *)(o + at.koff), o + at.vals,
                                      (uint64_t *)(o + at.voff), o + at.del, (uint64_t *)(o + at.seq), s)))
        return rc;
    if ((rc = run_download(o, at, dst, s))) return rc;
    // the existing runs and their indexes, then the size delta
    if ((rc = c->mw_runs.reserve(runs_upload_bytes(runs, nullptr, num_runs)))) return rc;
    RunUpload up;
    if ((rc = runs_upload(runs, nullptr, nullptr, num_runs, (uint8_t *)c->mw_runs.p, &up, s, who))) return rc;
    const seb_run fresh{o, sizes->key_bytes, (const uint64_t *)(o + at.koff), (const uint64_t *)(o + at.voff), o + at.del,
                        (const uint64_t *)(o + at.seq), sizes->entries_out};
    int64_t *ddelta = (int64_t *)section(c->mw_in, i_delta);
    if ((rc = seb_dev_run_size_delta(&fresh, up.drun, up.dindex, num_runs, ddelta, s))) return rc;
    if ((rc = download(size_delta, ddelta, 8, s))) return rc;
    HIP_OR_FAIL(hipStreamSynchronize(s));
    return SEB_OK;
}

extern "C" int seb_memtable_fold(seb_ctx *c, const seb_run *runs, const uint8_t *const *vals, const uint64_t *val_bytes,
                                 uint32_t num_runs, uint8_t *keys, uint64_t key_cap, uint64_t *key_off, uint8_t *out_vals,
                                 uint64_t val_cap, uint64_t *val_off, uint8_t *deleted, uint64_t *seq, uint64_t entry_cap,
                                 seb_fold_sizes *sizes) {
    const char *who = "seb_memtable_fold";
    int rc;
    if (!c) return fail(SEB_ERR_INVALID, "%s: null ctx", who);
    if (!sizes || !key_off || !val_off || (num_runs && !val_bytes)) return run_rc(-1, -1, false, 0, who);
    *sizes = kNoFold;
    key_off[0] = val_off[0] = 0;
    uint32_t bad_run = 0;
    if ((rc = run_rc(check_host_runs(runs, num_runs, SEB_MEM_MAX_RUNS, &bad_run), (int)bad_run, false, 0, who))) return rc;
    uint64_t entries = 0;
    for (uint32_t r = 0; r < num_runs; ++r) entries += runs[r].n;
    if (entries >= (1ull << 32)) return run_rc(-5, -1, false, 0, who);
    if (entries == 0) return SEB_OK;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OR_FAIL(hipSetDevice(c->device));
    hipStream_t s = c->s_comp;
    if ((rc = c->mw_runs.reserve(runs_upload_bytes(runs, val_bytes, num_runs)))) return rc;
    Drain drain{s};
    RunUpload up;
    if ((rc = runs_upload(runs, vals, val_bytes, num_runs, (uint8_t *)c->mw_runs.p, &up, s, who))) return rc;
    const uint64_t ws_bytes = fold_ws_layout(entries).bytes;
    if ((rc = c->mw_ws.reserve(ws_bytes, true))) return rc;
    if ((rc = seb_dev_runs_fold_plan(up.drun, up.dindex, val_bytes, num_runs, c->mw_ws.p, ws_bytes, sizes, s))) return rc;
    const RunDst dst{keys, key_cap, key_off, out_vals, val_cap, val_off, deleted, seq, entry_cap};
    if ((rc = check_run_dst(who, dst, sizes->entries_out, sizes->key_bytes, sizes->val_bytes))) return rc;
    const RunOut at(sizes->key_bytes, sizes->val_bytes, sizes->entries_out);
    if ((rc = c->mw_out.reserve(at.bytes))) return rc;
    uint8_t *o = (uint8_t *)c->mw_out.p;
    if ((rc = seb_dev_runs_fold_emit(up.drun, up.dindex, up.dvals, val_bytes, num_runs, sizes, c->mw_ws.p, ws_bytes, o,
                                     (uint64_t *)(o + at.koff), o + at.vals, (uint64_t *)(o + at.voff), o + at.del,
                                     seq ? (uint64_t *)(o + at.seq) : nullptr, s)))
        return rc;
    if ((rc = run_download(o, at, dst, s))) return rc;
    HIP_OR_FAIL(hipStreamSynchronize(s));
    return SEB_OK;
}
