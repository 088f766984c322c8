// seb_stage.cpp — the longer functions of seb_stage.h
#include "seb_stage.h"

namespace seb {

int OpsOnDevice::upload(uint8_t *base, const seb_keys *kb, const uint8_t *hvals, const uint64_t *hval_off,
                        const uint8_t *hdeleted, hipStream_t s) {
    int rc;
    const uint64_t n = kb->n;
    keys = seb_keys{base + a_keys - k0, nullptr, n, kb->stride, 0};
    vals = base + a_vals - v0;
    if ((rc = seb::upload(base + a_keys, kb->data ? kb->data + k0 : nullptr, k1 - k0, s)) ||
        (rc = seb::upload(&keys.offsets, base + a_koff, kb->offsets, 8 * (n + 1), s)) ||
        (rc = seb::upload(base + a_vals, hvals ? hvals + v0 : nullptr, v1 - v0, s)) ||
        (rc = seb::upload(&val_off, base + a_voff, hval_off, 8 * (n + 1), s)) ||
        (rc = seb::upload(&deleted, base + a_del, hdeleted, n, s)))
        return rc;
    return SEB_OK;
}

int runs_upload(const seb_run *runs, const uint8_t *const *vals, const uint64_t *val_bytes, uint32_t num_runs, uint8_t *base,
                RunUpload *up, hipStream_t s, const char *who) {
    int rc;
    Carver c;
    for (uint32_t r = 0; r < num_runs; ++r) {
        const seb_run &u = runs[r];
        if (!u.n) continue;
        const uint64_t vb = val_bytes ? val_bytes[r] : 0;
        const uint8_t *hvals = vb && vals ? vals[r] : nullptr;
        const RunSections at = run_sections(c, u, vb);
        seb_run &d = up->drun[r];
        d.n = u.n;
        d.key_bytes = u.key_bytes;
        if ((vb && !hvals) || upload(&d.keys, base + at.keys, u.keys, u.key_bytes, s) ||
            upload(&d.key_off, base + at.key_off, u.key_off, 8 * (u.n + 1), s) ||
            upload(&d.val_off, base + at.val_off, u.val_off, 8 * (u.n + 1), s) ||
            upload(&d.deleted, base + at.deleted, u.deleted, u.n, s) || upload(&d.seq, base + at.seq, u.seq, 8 * u.n, s) ||
            upload(&up->dvals[r], base + at.vals, hvals, vb, s))
            return fail(SEB_ERR_INTERNAL, "%s: run %u: a null array, or a copy to the device failed", who, r);
        if (!u.key_bytes) d.keys = nullptr;
        up->dindex[r] = base + at.index;
        if ((rc = seb_dev_run_index(&d, base + at.index, run_index_bytes(u.n), s))) {
            if (rc == SEB_ERR_INVALID) {  // the same words with the run's number
                const std::string msg = last_error();
                const size_t colon = msg.find(": ");
                return fail(rc, "%s: run %u: %s", who, r, colon == std::string::npos ? msg.c_str() : msg.c_str() + colon + 2);
            }
            return rc;
        }
    }
    return SEB_OK;
}

int check_host_runs(const seb_run *runs, uint32_t num_runs, uint32_t max_runs, uint32_t *bad_run) {
    if (num_runs > max_runs || (num_runs && !runs)) return -1;
    for (uint32_t r = 0; r < num_runs; ++r) {
        const seb_run &u = runs[r];
        *bad_run = r;
        if (u.n >= (1ull << 32)) return -5;
        if (u.n && (!u.key_off || !u.val_off || (!u.keys && u.key_bytes))) return -1;
    }
    return 0;
}

int check_run_dst(const char *who, const RunDst &d, uint64_t entries, uint64_t key_bytes, uint64_t val_bytes,
                  const uint64_t *image_bytes, uint64_t image_cap, const uint8_t *image) {
    const unsigned long long e = (unsigned long long)entries, k = (unsigned long long)key_bytes, v = (unsigned long long)val_bytes;
    const bool fits = entries <= d.entry_cap && key_bytes <= d.key_cap && val_bytes <= d.val_cap;
    if (image_bytes && (*image_bytes > image_cap || !fits))
        return fail(SEB_ERR_RANGE, "%s: a capacity is below its size (%llu image bytes, %llu entries, %llu key bytes, %llu value "
                    "bytes); retry with *image_bytes and *sizes", who, (unsigned long long)*image_bytes, e, k, v);
    if (!fits)
        return fail(SEB_ERR_RANGE, "%s: a capacity is below its size (%llu entries, %llu key bytes, %llu value bytes); "
                    "retry with *sizes", who, e, k, v);
    if ((image_bytes && !image) || (entries && !d.deleted) || (key_bytes && !d.keys) || (val_bytes && !d.vals))
        return fail(SEB_ERR_INVALID, "%s: null output", who);
    return SEB_OK;
}

int run_download(const uint8_t *o, const RunOut &at, const RunDst &d, hipStream_t s) {
    int rc;
    if ((rc = download(d.keys, o + at.keys, at.key_bytes, s)) || (rc = download(d.key_off, o + at.koff, 8 * (at.n + 1), s)) ||
        (rc = download(d.vals, o + at.vals, at.val_bytes, s)) || (rc = download(d.val_off, o + at.voff, 8 * (at.n + 1), s)) ||
        (rc = download(d.deleted, o + at.del, at.n, s)) || (rc = download(d.seq, o + at.seq, 8 * at.n, s)))
        return rc;
    return SEB_OK;
}

}  // namespace seb
