// seb_recover.cpp — the WAL replay's entry points: the C ABI over its host half (seb_memtable.cpp) and its
// kernels (seb_replay.hip), and seb_wal_recover, ReadAll + recoverFromWAL on host buffers through a context.
#include <new>

#include "seb_host.h"
#include "seb_memtable.h"

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
    auto up = [](uint64_t x) { return (x + 15) & ~15ull; };
    const uint64_t img_bytes = off[n], a_off = up(img_bytes), a_ok = a_off + up(8 * (n + 1));
    if ((rc = c->rpl_in.reserve(a_ok + up(n)))) return rc;
    uint8_t *in = (uint8_t *)c->rpl_in.p;
    const uint64_t *doff = (const uint64_t *)(in + a_off);
    // off and ok die with this frame: whichever way it is left, what the stream holds is waited for first
    struct Drain {
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{s};
    HIP_OR_FAIL(hipMemcpyAsync(in, image, img_bytes, hipMemcpyHostToDevice, s));
    HIP_OR_FAIL(hipMemcpyAsync(in + a_off, off.data(), 8 * (n + 1), hipMemcpyHostToDevice, s));
    if ((rc = seb_dev_wal_crc(in, doff, n, SEB_WAL_VERIFY, nullptr, in + a_ok, s))) return rc;
    HIP_OR_FAIL(hipMemcpyAsync(ok.data(), in + a_ok, n, hipMemcpyDeviceToHost, s));
    HIP_OR_FAIL(hipStreamSynchronize(s));
    // ReadAll's order: it meets a complete record that fails its CRC before it meets the truncated tail
    for (uint64_t i = 0; i < n; ++i)
        if (!ok[i])
            return fail(SEB_ERR_INVALID, "%s: WAL corruption detected: CRC mismatch (record %llu)", who, (unsigned long long)i);
    if (scan == SEB_ERR_SHORT) return fail(SEB_ERR_SHORT, "%s: %s", who, tail.c_str());
    const uint64_t ws_bytes = replay_ws_layout(n).bytes;
    if ((rc = c->rpl_ws.reserve(ws_bytes, true))) return rc;
    if ((rc = seb_dev_wal_replay_plan(in, doff, n, c->rpl_ws.p, ws_bytes, sizes, s))) return rc;
    if (sizes->entries_out > entry_cap || sizes->key_bytes > key_cap || sizes->val_bytes > val_cap)
        return fail(SEB_ERR_RANGE, "%s: a capacity is below its size (%llu entries, %llu key bytes, %llu value bytes); "
                    "retry with *sizes", who, (unsigned long long)sizes->entries_out, (unsigned long long)sizes->key_bytes,
                    (unsigned long long)sizes->val_bytes);
    const uint64_t no = sizes->entries_out;
    if ((no && !deleted) || (sizes->key_bytes && !keys) || (sizes->val_bytes && !vals))
        return fail(SEB_ERR_INVALID, "%s: null output", who);
    const uint64_t o_koff = up(sizes->key_bytes), o_vals = o_koff + up(8 * (no + 1)), o_voff = o_vals + up(sizes->val_bytes),
                   o_del = o_voff + up(8 * (no + 1)), o_seq = o_del + up(no), out_bytes = o_seq + up(8 * no);
    if ((rc = c->rpl_out.reserve(std::max<uint64_t>(out_bytes, 16)))) return rc;
    uint8_t *o = (uint8_t *)c->rpl_out.p;
    if ((rc = seb_dev_wal_replay_emit(in, doff, sizes, c->rpl_ws.p, ws_bytes, o, (uint64_t *)(o + o_koff), o + o_vals,
                                      (uint64_t *)(o + o_voff), o + o_del, seq ? (uint64_t *)(o + o_seq) : nullptr, s)))
        return rc;
    if (sizes->key_bytes) HIP_OR_FAIL(hipMemcpyAsync(keys, o, sizes->key_bytes, hipMemcpyDeviceToHost, s));
    HIP_OR_FAIL(hipMemcpyAsync(key_off, o + o_koff, 8 * (no + 1), hipMemcpyDeviceToHost, s));
    if (sizes->val_bytes) HIP_OR_FAIL(hipMemcpyAsync(vals, o + o_vals, sizes->val_bytes, hipMemcpyDeviceToHost, s));
    HIP_OR_FAIL(hipMemcpyAsync(val_off, o + o_voff, 8 * (no + 1), hipMemcpyDeviceToHost, s));
    if (no) HIP_OR_FAIL(hipMemcpyAsync(deleted, o + o_del, no, hipMemcpyDeviceToHost, s));
    if (no && seq) HIP_OR_FAIL(hipMemcpyAsync(seq, o + o_seq, 8 * no, hipMemcpyDeviceToHost, s));
    HIP_OR_FAIL(hipStreamSynchronize(s));
    return SEB_OK;
}
