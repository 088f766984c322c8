// seb_hidx.cpp — the hash index's entry points: the C ABI over its host half (seb_hashindex.cpp)
// and its kernels (seb_hashindex.hip), and seb_hidx_recover, recover() on host images through a context.
#include <new>

#include "seb_hashindex.h"
#include "seb_host.h"

using namespace seb;

static_assert(SEB_SEG_HEADER_BYTES == seb::kSegHeader, "SEB_SEG_HEADER_BYTES");
static_assert(SEB_HIDX_NO_RECORD == seb::kHidxNoRec, "SEB_HIDX_NO_RECORD");

constexpr uint64_t kMaxCapacity = 1ull << 40;

static int hidx_rc(int rc, const char *who) {
    switch (rc) {
    case 0:
        return SEB_OK;
    case -2:
        return fail(SEB_ERR_INVALID, "%s: pool_bytes is 2^47 or more", who);
    case -3:
        return fail(SEB_ERR_NOMEM, "%s: out of host memory", who);
    default:
        return fail(SEB_ERR_INVALID, "%s: a null argument", who);
    }
}

// ------------------------------------------------ host only

extern "C" int seb_seg_scan(const uint8_t *data, uint64_t bytes, uint64_t base, uint64_t *rec_off, uint64_t cap, uint64_t *n,
                            int *short_tail) {
    const char *who = "seb_seg_scan";
    const int rc = seb::seg_scan(data, bytes, base, rec_off, cap, n, short_tail);
    if (rc == -2) return fail(SEB_ERR_INVALID, "%s: more than %llu records", who, (unsigned long long)cap);
    return hidx_rc(rc, who);
}

extern "C" int seb_seg_verify(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, uint64_t num_records,
                              const uint64_t *seg_first, const uint64_t *seg_base, const uint64_t *seg_bytes,
                              uint64_t num_segments, uint8_t *ok, uint64_t *valid, uint64_t *size_after, uint8_t *live) {
    const char *who = "seb_seg_verify";
    const int rc = seb::seg_verify(pool, pool_bytes, rec_off, num_records, seg_first, seg_base, seg_bytes, num_segments, ok, valid,
                                   size_after, live);
    if (rc == -3)
        return fail(SEB_ERR_INVALID, "%s: seg_first does not start at 0, decreases or does not end at num_records", who);
    return hidx_rc(rc, who);
}

extern "C" int seb_hidx_lookup(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, const uint8_t *live,
                               uint64_t num_records, const seb_keys *keys, int verify, uint8_t *status, uint64_t *rec,
                               uint64_t *vloc, uint32_t *vlen, uint64_t *distinct) {
    const char *who = "seb_hidx_lookup";
    int rc;
    if ((rc = check_keys(keys, who)) || (rc = validate_offsets(keys, who))) return rc;
    return hidx_rc(seb::hidx_lookup(pool, pool_bytes, rec_off, live, num_records,
                                    seb::KeysView{keys->data, keys->offsets, keys->n, keys->stride}, verify, status, rec, vloc, vlen,
                                    distinct),
                   who);
}

// ------------------------------------------------ device

extern "C" uint64_t seb_dev_hidx_table_bytes(uint64_t capacity) { return capacity > kMaxCapacity ? 0 : hidx_table_bytes(capacity); }

static int check_table(const void *table, uint64_t capacity, const char *who) {
    if (capacity > kMaxCapacity) return fail(SEB_ERR_INVALID, "%s: capacity above 2^40", who);
    if (!table || ((uintptr_t)table & 15)) return fail(SEB_ERR_INVALID, "%s: the table is null or not 16-byte aligned", who);
    return SEB_OK;
}

static int check_pool(const uint8_t *pool, uint64_t pool_bytes, const char *who) {
    if (pool_bytes >= seb::kHidxPoolLimit) return hidx_rc(-2, who);
    if (pool_bytes && !pool) return fail(SEB_ERR_INVALID, "%s: null pool", who);
    return SEB_OK;
}

extern "C" int seb_dev_hidx_clear(void *table, uint64_t capacity, void *stream) {
    const char *who = "seb_dev_hidx_clear";
    enter();
    int rc;
    if ((rc = check_table(table, capacity, who))) return rc;
    HIP_OR_FAIL(launch_hidx_clear(table, capacity, (hipStream_t)stream));
    return SEB_OK;
}

extern "C" int seb_dev_seg_verify(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, uint64_t num_records,
                                  const uint64_t *seg_first, uint64_t num_segments, uint8_t *ok, uint64_t *valid, uint8_t *live,
                                  void *stream) {
    const char *who = "seb_dev_seg_verify";
    enter();
    int rc;
    if ((rc = check_pool(pool, pool_bytes, who))) return rc;
    if (num_records >= (1ull << 38) || num_segments >= (1ull << 32))
        return fail(SEB_ERR_INVALID, "%s: 2^38 records or 2^32 segments, or more", who);
    if ((num_records && (!rec_off || !ok)) || (num_segments && (!seg_first || !valid)) || (num_records && !num_segments))
        return fail(SEB_ERR_INVALID, "%s: a null argument, or records without a segment", who);
    if (((uintptr_t)rec_off & 7) || ((uintptr_t)seg_first & 7) || ((uintptr_t)valid & 7))
        return fail(SEB_ERR_INVALID, "%s: rec_off, seg_first or valid is not 8-byte aligned", who);
    HIP_OR_FAIL(launch_seg_verify(pool, pool_bytes, rec_off, num_records, seg_first, num_segments, ok, valid, live,
                                  (hipStream_t)stream));
    return SEB_OK;
}

extern "C" int seb_dev_hidx_insert(void *table, uint64_t capacity, const uint8_t *pool, uint64_t pool_bytes,
                                   const uint64_t *rec_off, const uint8_t *live, uint64_t num_records, void *stream) {
    const char *who = "seb_dev_hidx_insert";
    enter();
    int rc;
    if ((rc = check_table(table, capacity, who)) || (rc = check_pool(pool, pool_bytes, who))) return rc;
    if (num_records && !rec_off) return fail(SEB_ERR_INVALID, "%s: null rec_off", who);
    if ((uintptr_t)rec_off & 7) return fail(SEB_ERR_INVALID, "%s: rec_off is not 8-byte aligned", who);
    HIP_OR_FAIL(launch_hidx_insert(table, capacity, pool, pool_bytes, rec_off, live, num_records, options().hidx_hash_mask,
                                   (hipStream_t)stream));
    return SEB_OK;
}

extern "C" int seb_dev_hidx_count(const void *table, uint64_t capacity, uint64_t *distinct, uint64_t *bad_records,
                                  void *stream) {
    const char *who = "seb_dev_hidx_count";
    enter();
    int rc;
    if ((rc = check_table(table, capacity, who))) return rc;
    uint64_t st[3] = {0, 0, 0};
    HIP_OR_FAIL(launch_hidx_state(table, st, (hipStream_t)stream));
    if (distinct) *distinct = st[1];
    if (bad_records) *bad_records = st[2];
    if (st[0])
        return fail(SEB_ERR_RANGE, "%s: the table of %llu slots filled: more than %llu distinct keys; clear it and insert "
                    "again with a capacity of the live records at most", who, (unsigned long long)hidx_slots(capacity),
                    (unsigned long long)capacity);
    return SEB_OK;
}

extern "C" int seb_dev_hidx_get(const void *table, uint64_t capacity, const uint8_t *pool, uint64_t pool_bytes,
                                const seb_keys *keys, int verify, uint8_t *status, uint64_t *rec, uint64_t *vloc, uint32_t *vlen,
                                uint8_t *source, void *stream) {
    const char *who = "seb_dev_hidx_get";
    enter();
    int rc;
    if ((rc = check_keys(keys, who)) || (rc = check_table(table, capacity, who)) || (rc = check_pool(pool, pool_bytes, who)))
        return rc;
    if (keys->n == 0) return SEB_OK;
    if (!status) return fail(SEB_ERR_INVALID, "%s: null status", who);
    if (((uintptr_t)keys->offsets & 7) || ((uintptr_t)rec & 7) || ((uintptr_t)vloc & 7) || ((uintptr_t)vlen & 3))
        return fail(SEB_ERR_INVALID, "%s: offsets, rec or vloc not 8-byte aligned, or vlen not 4-byte aligned", who);
    HIP_OR_FAIL(launch_hidx_get(table, capacity, pool, pool_bytes, key_batch(keys), verify != 0, options().hidx_hash_mask, status,
                                rec, vloc, vlen, source, (hipStream_t)stream));
    return SEB_OK;
}

// Host images through the context: the framing walk on the host, the images and the offsets up, verify, clear and
// insert on the compute stream, the per-segment counts and the table's state back.
extern "C" int seb_hidx_recover(seb_ctx *c, const uint8_t *const *images, const uint64_t *image_bytes, uint64_t num_segments,
                                uint8_t *dev_pool, uint64_t pool_cap, void *dev_table, uint64_t capacity, uint64_t *valid,
                                uint64_t *size_after, uint8_t *short_tail, uint8_t *cut, uint64_t *records,
                                uint64_t *live_records, uint64_t *distinct) {
    const char *who = "seb_hidx_recover";
    int rc;
    if (!c) return fail(SEB_ERR_INVALID, "%s: null ctx", who);
    if (num_segments >= (1ull << 32)) return fail(SEB_ERR_INVALID, "%s: 2^32 segments or more", who);
    if (num_segments && (!images || !image_bytes || !valid || !size_after)) return hidx_rc(-1, who);
    if ((rc = check_table(dev_table, capacity, who))) return rc;
    if (records) *records = 0;
    if (live_records) *live_records = 0;
    if (distinct) *distinct = 0;
    uint64_t total = 0;
    for (uint64_t s = 0; s < num_segments; ++s) {
        if (image_bytes[s] && !images[s]) return hidx_rc(-1, who);
        if (image_bytes[s] >= seb::kHidxPoolLimit || (total += image_bytes[s]) >= seb::kHidxPoolLimit) return hidx_rc(-2, who);
    }
    if (total > pool_cap)
        return fail(SEB_ERR_RANGE, "%s: pool_cap %llu is below the images' %llu bytes", who, (unsigned long long)pool_cap,
                    (unsigned long long)total);
    if (total && !dev_pool) return fail(SEB_ERR_INVALID, "%s: null pool", who);
    std::vector<uint64_t> off, first, base, dvalid;
    try {
        first.resize(num_segments + 1);
        base.resize(num_segments + 1);
        dvalid.resize(num_segments);
        uint64_t at = 0, n = 0;
        for (uint64_t s = 0; s < num_segments; ++s) {
            first[s] = n, base[s] = at;
            off.resize(n + image_bytes[s] / seb::kSegHeader + 1);
            uint64_t got = 0;
            int tail = 0;
            if (seb::seg_scan(images[s], image_bytes[s], at, off.data() + n, off.size() - n, &got, &tail) != 0)
                return fail(SEB_ERR_INTERNAL, "%s: segment %llu: the scan ran past its bound", who, (unsigned long long)s);
            if (short_tail) short_tail[s] = (uint8_t)tail;
            n += got, at += image_bytes[s];
        }
        first[num_segments] = n, base[num_segments] = at;
        off.resize(n);
    } catch (const std::bad_alloc &) {
        return hidx_rc(-3, who);
    }
    const uint64_t n = off.size();
    if (n >= (1ull << 38)) return fail(SEB_ERR_INVALID, "%s: 2^38 records or more", who);
    if (records) *records = n;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OR_FAIL(hipSetDevice(c->device));
    hipStream_t st = c->s_comp;
    auto up = [](uint64_t x) { return (x + 15) & ~15ull; };
    const uint64_t a_first = up(8 * n), a_valid = a_first + up(8 * (num_segments + 1)), a_ok = a_valid + up(8 * num_segments),
                   a_live = a_ok + up(n);
    if ((rc = c->hx_ws.reserve(a_live + up(n) + 16))) return rc;
    uint8_t *w = (uint8_t *)c->hx_ws.p;
    // the vectors die with this frame: whichever way it is left, what the stream holds is waited for first
    struct Drain {
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{st};
    for (uint64_t s = 0; s < num_segments; ++s)
        if (image_bytes[s]) HIP_OR_FAIL(hipMemcpyAsync(dev_pool + base[s], images[s], image_bytes[s], hipMemcpyHostToDevice, st));
    if (n) HIP_OR_FAIL(hipMemcpyAsync(w, off.data(), 8 * n, hipMemcpyHostToDevice, st));
    HIP_OR_FAIL(hipMemcpyAsync(w + a_first, first.data(), 8 * (num_segments + 1), hipMemcpyHostToDevice, st));
    if (num_segments &&
        (rc = seb_dev_seg_verify(dev_pool, total, (const uint64_t *)w, n, (const uint64_t *)(w + a_first), num_segments, w + a_ok,
                                 (uint64_t *)(w + a_valid), w + a_live, st)))
        return rc;
    if ((rc = seb_dev_hidx_clear(dev_table, capacity, st))) return rc;
    if ((rc = seb_dev_hidx_insert(dev_table, capacity, dev_pool, total, (const uint64_t *)w, w + a_live, n, st))) return rc;
    if (num_segments) HIP_OR_FAIL(hipMemcpyAsync(dvalid.data(), w + a_valid, 8 * num_segments, hipMemcpyDeviceToHost, st));
    uint64_t keys = 0;
    const int count_rc = seb_dev_hidx_count(dev_table, capacity, &keys, nullptr, st);  // synchronises
    if (count_rc != SEB_OK && count_rc != SEB_ERR_RANGE) return count_rc;
    uint64_t alive = 0;
    for (uint64_t s = 0; s < num_segments; ++s) {
        const uint64_t cnt = first[s + 1] - first[s];
        const bool was_cut = dvalid[s] < cnt;
        valid[s] = was_cut ? dvalid[s] : cnt;
        size_after[s] = was_cut ? off[first[s] + dvalid[s]] - base[s] : image_bytes[s];
        if (cut) cut[s] = was_cut;
        if (short_tail && was_cut) short_tail[s] = 0;  // recover never reached the tail: the walk ended at the cut
        alive += valid[s];
    }
    if (live_records) *live_records = alive;
    if (count_rc == SEB_ERR_RANGE)
        return fail(SEB_ERR_RANGE, "%s: the table filled: more than %llu distinct keys; retry with a capacity of the %llu live "
                    "records at most", who, (unsigned long long)capacity, (unsigned long long)alive);
    if (distinct) *distinct = keys;
    return SEB_OK;
}
