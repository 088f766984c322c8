// seb_hidx.cpp — the hash index's entry points: the C ABI over its host halves
// (seb_hashindex.cpp, seb_hashwrite.cpp) and its kernels (seb_hashindex.hip, seb_hashwrite.hip), and seb_hidx_recover,
// recover() on host images through a context.
#include <new>

#include "seb_hashindex.h"
#include "seb_hashwrite.h"
#include "seb_host.h"
#include "seb_stage.h"

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

// The framing walk over `ns` segments of seg_bytes[s] bytes at pool offsets seg_base[s]: off = every record's pool offset,
// first[s] = segment s's first record (ns + 1 entries); valid gets its ns entries.  images: each segment's own host bytes
// (seb_hidx_recover); null: the segments lie back to back in `head` from seg_base[0] on (seb_hidx_compact).
static int seg_walk(const uint8_t *const *images, const uint8_t *head, const uint64_t *seg_base, const uint64_t *seg_bytes,
                    uint64_t ns, std::vector<uint64_t> &off, std::vector<uint64_t> &first, std::vector<uint64_t> &valid,
                    uint8_t *short_tail, const char *who) {
    try {
        first.resize(ns + 1);
        valid.resize(ns);
        uint64_t n = 0;
        for (uint64_t s = 0; s < ns; ++s) {
            first[s] = n;
            off.resize(n + seg_bytes[s] / seb::kSegHeader + 1);
            uint64_t got = 0;
            int tail = 0;
            const uint8_t *image = images ? images[s] : head + (seg_base[s] - seg_base[0]);
            if (seb::seg_scan(image, seg_bytes[s], seg_base[s], off.data() + n, off.size() - n, &got, &tail) != 0)
                return fail(SEB_ERR_INTERNAL, "%s: segment %llu: the scan ran past its bound", who, (unsigned long long)s);
            if (short_tail) short_tail[s] = (uint8_t)tail;
            n += got;  // a short tail is no record
        }
        first[ns] = n;
        off.resize(n);
    } catch (const std::bad_alloc &) {
        return hidx_rc(-3, who);
    }
    if (off.size() >= (1ull << 38)) return fail(SEB_ERR_INVALID, "%s: 2^38 records or more", who);
    return SEB_OK;
}

// Both forms' first sections: the records' offsets, each segment's first record and valid count, a CRC and a live byte per record
struct SegSections {
    uint64_t off, first, valid, ok, live;
    SegSections(Carver &c, uint64_t n, uint64_t ns)
        : off(c.take(8 * n)), first(c.take(8 * (ns + 1))), valid(c.take(8 * ns)), ok(c.take(n)), live(c.take(n)) {}
};

// The walk's offsets up, the segments verified (w: the buffer the sections were carved from)
static int seg_stage_verify(uint8_t *w, const SegSections &at, const std::vector<uint64_t> &off, const std::vector<uint64_t> &first,
                            uint64_t ns, const uint8_t *pool, uint64_t pool_bytes, hipStream_t st) {
    int rc;
    if ((rc = upload(w + at.off, off.data(), 8 * off.size(), st)) || (rc = upload(w + at.first, first.data(), 8 * (ns + 1), st)))
        return rc;
    if (!ns) return SEB_OK;
    return seb_dev_seg_verify(pool, pool_bytes, (const uint64_t *)(w + at.off), off.size(), (const uint64_t *)(w + at.first), ns,
                              w + at.ok, (uint64_t *)(w + at.valid), w + at.live, st);
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
        base.resize(num_segments + 1);
    } catch (const std::bad_alloc &) {
        return hidx_rc(-3, who);
    }
    for (uint64_t s = 0; s < num_segments; ++s) base[s + 1] = base[s] + image_bytes[s];
    if ((rc = seg_walk(images, nullptr, base.data(), image_bytes, num_segments, off, first, dvalid, short_tail, who))) return rc;
    const uint64_t n = off.size();
    if (records) *records = n;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OR_FAIL(hipSetDevice(c->device));
    hipStream_t st = c->s_comp;
    Drain drain{st};
    Carver ws;
    const SegSections at(ws, n, num_segments);
    if ((rc = c->hx_ws.reserve(ws.bytes()))) return rc;
    uint8_t *w = (uint8_t *)c->hx_ws.p;
    for (uint64_t s = 0; s < num_segments; ++s)
        if (image_bytes[s]) HIP_OR_FAIL(hipMemcpyAsync(dev_pool + base[s], images[s], image_bytes[s], hipMemcpyHostToDevice, st));
    if ((rc = seg_stage_verify(w, at, off, first, num_segments, dev_pool, total, st))) return rc;
    if ((rc = seb_dev_hidx_clear(dev_table, capacity, st))) return rc;
    if ((rc = seb_dev_hidx_insert(dev_table, capacity, dev_pool, total, (const uint64_t *)(w + at.off), w + at.live, n, st)))
        return rc;
    if ((rc = download(dvalid.data(), w + at.valid, 8 * num_segments, st))) return rc;
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

// ------------------------------------------------ write side

static_assert(sizeof(seb_segcompact_sizes) == sizeof(seb::SegCompactSizes) && sizeof(seb_segcompact_sizes) == 64,
              "seb_segcompact_sizes layout");

static int segframe_rc(int rc, uint64_t op, uint64_t need, const char *who) {
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
    case -6:
        return fail(SEB_ERR_INVALID, "%s: op %llu: an empty key (Put refuses it)", who, i);
    case -7:
        return fail(SEB_ERR_INVALID, "%s: op %llu: keySize + valueSize is 2^32 or more", who, i);
    case -8:
        return fail(SEB_ERR_RANGE, "%s: cut_cap is below the batch's %llu cuts", who, (unsigned long long)need);
    case -9:
        return fail(SEB_ERR_INVALID, "%s: limit is 0", who);
    default:
        return fail(SEB_ERR_INVALID, "%s: null argument", who);
    }
}

static int check_seg_ops(const seb_keys *keys, const uint64_t *val_off, const char *who) {
    int rc;
    if ((rc = check_keys(keys, who))) return rc;
    if (keys->n >= (1ull << 32)) return segframe_rc(-4, 0, 0, who);
    if (keys->n && !val_off) return segframe_rc(-1, 0, 0, who);
    return SEB_OK;
}

extern "C" int seb_seg_frame_plan(const seb_keys *keys, const uint64_t *val_off, const uint8_t *deleted, uint64_t active_size,
                                  uint64_t limit, uint64_t *rec_off, uint64_t *cut, uint64_t cut_cap, uint64_t *image_bytes,
                                  uint64_t *ncuts) {
    const char *who = "seb_seg_frame_plan";
    int rc;
    if ((rc = check_seg_ops(keys, val_off, who))) return rc;
    uint64_t op = 0, cuts = 0;
    rc = seb::seg_frame_plan(KeysView{keys->data, keys->offsets, keys->n, keys->stride}, val_off, deleted, active_size, limit,
                             rec_off, cut, cut_cap, image_bytes, &cuts, &op);
    if (ncuts && (rc == 0 || rc == -8)) *ncuts = cuts;
    return segframe_rc(rc, op, cuts, who);
}

extern "C" int seb_seg_frame_emit(const seb_keys *keys, const uint8_t *vals, const uint64_t *val_off, const uint8_t *deleted,
                                  uint64_t timestamp, uint8_t *image, uint64_t image_bytes) {
    const char *who = "seb_seg_frame_emit";
    int rc;
    if ((rc = check_seg_ops(keys, val_off, who))) return rc;
    uint64_t op = 0;
    rc = seb::seg_frame_emit(KeysView{keys->data, keys->offsets, keys->n, keys->stride}, vals, val_off, deleted, timestamp,
                             image, image_bytes, &op);
    return segframe_rc(rc, op, 0, who);
}

static int check_dev_seg_ops(const seb_keys *keys, const uint64_t *val_off, const char *who) {
    int rc;
    if ((rc = check_seg_ops(keys, val_off, who))) return rc;
    if (keys->n && (((uintptr_t)keys->offsets & 7) || ((uintptr_t)val_off & 7)))
        return fail(SEB_ERR_INVALID, "%s: offsets that are not 8-byte aligned", who);
    return SEB_OK;
}

extern "C" int seb_dev_seg_frame_plan(const seb_keys *keys, const uint64_t *val_off, const uint8_t *deleted,
                                      uint64_t active_size, uint64_t limit, uint64_t *rec_off, uint64_t *cut, uint64_t cut_cap,
                                      uint64_t *image_bytes, uint64_t *ncuts, void *stream) {
    const char *who = "seb_dev_seg_frame_plan";
    WsCall ws_call;
    enter();
    int rc;
    if ((rc = check_dev_seg_ops(keys, val_off, who))) return rc;
    if (!image_bytes || !ncuts) return segframe_rc(-1, 0, 0, who);
    if (limit == 0) return segframe_rc(-9, 0, 0, who);
    *image_bytes = *ncuts = 0;
    if (keys->n == 0) return SEB_OK;
    if (!rec_off || ((uintptr_t)rec_off & 7)) return fail(SEB_ERR_INVALID, "%s: rec_off is null or not 8-byte aligned", who);
    if (!cut) cut_cap = 0;
    hipStream_t s = (hipStream_t)stream;
    void *scratch = nullptr;
    if ((rc = cached_workspace(s, segframe_scratch_bytes(keys->n, cut_cap), &scratch, 5))) return rc;
    const uint64_t slots = cut_cap < keys->n ? cut_cap : keys->n;
    std::vector<uint64_t> got;
    try {
        got.resize(slots);
    } catch (const std::bad_alloc &) {
        return hidx_rc(-3, who);
    }
    uint64_t h[3] = {0, 0, 0};
    HIP_OR_FAIL(launch_segframe_plan(key_batch(keys), val_off, deleted, active_size, limit, rec_off, got.data(), cut_cap, scratch, h,
                                     s));
    if (h[0] != UINT64_MAX) {
        static const int why[4] = {-2, -3, -6, -7};
        return segframe_rc(why[h[0] & 3], h[0] >> 2, 0, who);
    }
    *image_bytes = h[1];
    *ncuts = h[2];
    if (cut && h[2] > cut_cap) return segframe_rc(-8, 0, h[2], who);
    if (cut && h[2]) memcpy(cut, got.data(), 8 * h[2]);
    return SEB_OK;
}

extern "C" int seb_dev_seg_frame_emit(const seb_keys *keys, const uint8_t *vals, const uint64_t *val_off,
                                      const uint8_t *deleted, uint64_t timestamp, const uint64_t *rec_off, uint8_t *image,
                                      uint64_t image_bytes, void *stream) {
    const char *who = "seb_dev_seg_frame_emit";
    enter();
    int rc;
    if ((rc = check_dev_seg_ops(keys, val_off, who))) return rc;
    const uint64_t n = keys->n;
    if (n == 0) return image_bytes ? segframe_rc(-5, 0, 0, who) : SEB_OK;
    if (!rec_off || ((uintptr_t)rec_off & 7) || !image)
        return fail(SEB_ERR_INVALID, "%s: null image, or rec_off null or not 8-byte aligned", who);
    // a record has 21 bytes at least (the header and a key byte) and 20 + 2^32 - 1 at most
    if (image_bytes < 21 * n || image_bytes > n * (20 + 0xFFFFFFFFull) || image_bytes >= seb::kHidxPoolLimit)
        return segframe_rc(-5, 0, 0, who);
    HIP_OR_FAIL(launch_segframe_emit(key_batch(keys), vals, val_off, deleted, timestamp, rec_off, image, image_bytes,
                                     (hipStream_t)stream));
    return SEB_OK;
}

static int compact_rc(int rc, uint64_t bad, const seb_segcompact_sizes *sz, const char *who) {
    switch (rc) {
    case -4:
        return fail(SEB_ERR_INVALID, "%s: record %llu does not lie inside the pool, or its keySize + valueSize is 2^32 or more",
                    who, (unsigned long long)bad);
    case -5:
        return fail(SEB_ERR_RANGE, "%s: a capacity is below the compaction's sizes: %llu image bytes, %llu + 1 offsets", who,
                    (unsigned long long)sz->image_bytes, (unsigned long long)sz->survivors);
    default:
        return hidx_rc(rc, who);
    }
}

extern "C" int seb_seg_compact(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, const uint8_t *live,
                               uint64_t num_records, uint64_t timestamp, uint8_t *image, uint64_t image_cap,
                               uint64_t *out_rec_off, uint64_t rec_cap, seb_segcompact_sizes *sizes) {
    const char *who = "seb_seg_compact";
    uint64_t bad = 0;
    const int rc = seb::seg_compact(pool, pool_bytes, rec_off, live, num_records, timestamp, image, image_cap, out_rec_off, rec_cap,
                                    (seb::SegCompactSizes *)sizes, &bad);
    return compact_rc(rc, bad, sizes, who);
}

extern "C" int seb_hidx_logical_size(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, const uint8_t *live,
                                     uint64_t num_records, uint64_t *logical) {
    return hidx_rc(seb::hidx_logical_size(pool, pool_bytes, rec_off, live, num_records, logical), "seb_hidx_logical_size");
}

extern "C" uint64_t seb_dev_seg_compact_workspace_size(uint64_t num_records) {
    return num_records >= (1ull << 38) ? 0 : segcompact_ws_layout(num_records ? num_records : 1).bytes;
}

static int check_compact(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, uint64_t n, const void *ws,
                         uint64_t ws_bytes, const char *who) {
    int rc;
    if ((rc = check_pool(pool, pool_bytes, who))) return rc;
    if (n >= (1ull << 38)) return fail(SEB_ERR_INVALID, "%s: 2^38 records or more", who);
    if (n && (!rec_off || ((uintptr_t)rec_off & 7))) return fail(SEB_ERR_INVALID, "%s: rec_off is null or not 8-byte aligned", who);
    if (n && (!ws || ((uintptr_t)ws & 15) || ws_bytes < segcompact_ws_layout(n).bytes))
        return fail(SEB_ERR_INVALID, "%s: the workspace is null, not 16-byte aligned or below %llu bytes", who,
                    (unsigned long long)segcompact_ws_layout(n).bytes);
    return SEB_OK;
}

extern "C" int seb_dev_seg_compact_plan(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, const uint8_t *live,
                                        uint64_t num_records, void *workspace, uint64_t workspace_bytes,
                                        seb_segcompact_sizes *sizes, void *stream) {
    const char *who = "seb_dev_seg_compact_plan";
    enter();
    int rc;
    if (!sizes) return hidx_rc(-1, who);
    *sizes = seb_segcompact_sizes{num_records, 0, 0, 0, 0, 0, 0, 0};
    if ((rc = check_compact(pool, pool_bytes, rec_off, num_records, workspace, workspace_bytes, who))) return rc;
    if (num_records == 0) return SEB_OK;
    uint64_t h[8];
    HIP_OR_FAIL(launch_segcompact_plan(pool, pool_bytes, rec_off, live, num_records, options().hidx_hash_mask, workspace, h,
                                       (hipStream_t)stream));
    if (h[0] != UINT64_MAX) return compact_rc(-4, h[0], sizes, who);
    if (h[6]) return fail(SEB_ERR_INTERNAL, "%s: the scratch table filled", who);
    *sizes = seb_segcompact_sizes{num_records, h[1], h[2], h[3], h[4], h[1] - h[2], h[5], 0};
    return SEB_OK;
}

extern "C" int seb_dev_seg_compact_emit(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, uint64_t num_records,
                                        uint64_t timestamp, const seb_segcompact_sizes *sizes, void *workspace,
                                        uint64_t workspace_bytes, uint8_t *image, uint64_t *out_rec_off, void *stream) {
    const char *who = "seb_dev_seg_compact_emit";
    enter();
    int rc;
    if (!sizes) return hidx_rc(-1, who);
    if ((rc = check_compact(pool, pool_bytes, rec_off, num_records, workspace, workspace_bytes, who))) return rc;
    if (sizes->records_in != num_records || sizes->survivors > num_records || sizes->image_bytes < 21 * sizes->survivors ||
        (sizes->survivors == 0 && sizes->image_bytes) || sizes->image_bytes >= seb::kHidxPoolLimit)
        return fail(SEB_ERR_INVALID, "%s: sizes are not these records' plan", who);
    if (!out_rec_off || ((uintptr_t)out_rec_off & 7) || (sizes->image_bytes && !image))
        return fail(SEB_ERR_INVALID, "%s: null image, or out_rec_off null or not 8-byte aligned", who);
    HIP_OR_FAIL(launch_segcompact_emit(pool, pool_bytes, rec_off, num_records, timestamp, sizes->survivors, sizes->image_bytes,
                                       workspace, image, out_rec_off, (hipStream_t)stream));
    return SEB_OK;
}

extern "C" int seb_dev_hidx_logical_size(const void *table, uint64_t capacity, const uint8_t *pool, uint64_t pool_bytes,
                                         uint64_t *logical, void *stream) {
    const char *who = "seb_dev_hidx_logical_size";
    WsCall ws_call;
    enter();
    int rc;
    if ((rc = check_table(table, capacity, who)) || (rc = check_pool(pool, pool_bytes, who))) return rc;
    if (!logical) return hidx_rc(-1, who);
    *logical = 0;
    hipStream_t s = (hipStream_t)stream;
    void *scratch = nullptr;
    if ((rc = cached_workspace(s, 16, &scratch, 5))) return rc;
    HIP_OR_FAIL(launch_hidx_logical(table, capacity, pool, pool_bytes, (uint64_t *)scratch, logical, s));
    return SEB_OK;
}

// compactSegments + applyCompaction on a pool in device memory: the compacted segments' bytes come down for the
// framing walk alone (the walk is sequential); verify, plan, emit, the copy of the segments that stay, the shift of
// their offsets, clear and insert run on the compute stream.
extern "C" int seb_hidx_compact(seb_ctx *c, const uint8_t *dev_pool, uint64_t pool_bytes, const uint64_t *seg_base,
                                const uint64_t *seg_bytes, uint64_t num_segments, uint64_t compact_segments,
                                const uint64_t *rest_rec_off, const uint8_t *rest_live, uint64_t rest_records, uint64_t timestamp,
                                uint8_t *dst_pool, uint64_t dst_cap, void *dev_table, uint64_t capacity, uint64_t *new_rec_off,
                                uint64_t new_rec_cap, seb_segcompact_sizes *sizes, uint64_t *new_seg_base,
                                uint64_t *new_seg_bytes, uint64_t *distinct) {
    const char *who = "seb_hidx_compact";
    int rc;
    if (!c) return fail(SEB_ERR_INVALID, "%s: null ctx", who);
    if (!sizes || !seg_base || !seg_bytes || !new_seg_base || !new_seg_bytes) return hidx_rc(-1, who);
    *sizes = seb_segcompact_sizes{0, 0, 0, 0, 0, 0, 0, 0};
    if (distinct) *distinct = 0;
    const uint64_t cs = compact_segments;
    if (cs == 0 || cs > num_segments || num_segments >= (1ull << 32))
        return fail(SEB_ERR_INVALID, "%s: %llu of %llu segments", who, (unsigned long long)cs, (unsigned long long)num_segments);
    if ((rc = check_table(dev_table, capacity, who)) || (rc = check_pool(dev_pool, pool_bytes, who))) return rc;
    uint64_t at = seg_base[0];
    for (uint64_t s = 0; s < num_segments; ++s) {  // back to back, oldest first, inside the pool
        if (seg_base[s] != at || seg_bytes[s] > pool_bytes - at)
            return fail(SEB_ERR_INVALID, "%s: segment %llu does not lie behind its predecessor inside the pool", who,
                        (unsigned long long)s);
        at += seg_bytes[s];
    }
    const uint64_t head_at = seg_base[0], rest_at = seg_base[cs - 1] + seg_bytes[cs - 1], head_bytes = rest_at - head_at,
                   rest_bytes = at - rest_at;
    if (rest_records >= (1ull << 38)) return fail(SEB_ERR_INVALID, "%s: 2^38 records or more", who);
    if (rest_records && (!rest_rec_off || ((uintptr_t)rest_rec_off & 7)))
        return fail(SEB_ERR_INVALID, "%s: rest_rec_off is null or not 8-byte aligned", who);
    if (!new_rec_off || ((uintptr_t)new_rec_off & 7)) return fail(SEB_ERR_INVALID, "%s: new_rec_off is null or not 8-byte aligned", who);
    std::vector<uint8_t> head;
    std::vector<uint64_t> off, first, dvalid;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OR_FAIL(hipSetDevice(c->device));
    hipStream_t st = c->s_comp;
    Drain drain{st};
    try {
        head.resize(head_bytes);
    } catch (const std::bad_alloc &) {
        return hidx_rc(-3, who);
    }
    if ((rc = download(head.data(), dev_pool + head_at, head_bytes, st))) return rc;
    if (head_bytes) HIP_OR_FAIL(hipStreamSynchronize(st));
    if ((rc = seg_walk(nullptr, head.data(), seg_base, seg_bytes, cs, off, first, dvalid, nullptr, who))) return rc;
    std::vector<uint8_t>().swap(head);
    const uint64_t n = off.size();
    Carver ws;
    const SegSections sec(ws, n, cs);
    const uint64_t plan_bytes = n ? segcompact_ws_layout(n).bytes : 0, a_plan = ws.take(plan_bytes);
    if ((rc = c->hx_ws.reserve(ws.bytes()))) return rc;
    uint8_t *w = (uint8_t *)c->hx_ws.p;
    if ((rc = seg_stage_verify(w, sec, off, first, cs, dev_pool, pool_bytes, st))) return rc;
    if ((rc = download(dvalid.data(), w + sec.valid, 8 * cs, st))) return rc;
    HIP_OR_FAIL(hipStreamSynchronize(st));
    for (uint64_t s = 0; s < cs; ++s)  // compactSegments returns the error: nothing is compacted
        if (dvalid[s] < first[s + 1] - first[s])
            return fail(SEB_ERR_INVALID, "%s: segment %llu: record %llu fails its CRC: the compaction is aborted", who,
                        (unsigned long long)s, (unsigned long long)dvalid[s]);
    const uint64_t *doff = (const uint64_t *)(w + sec.off);
    if ((rc = seb_dev_seg_compact_plan(dev_pool, pool_bytes, doff, nullptr, n, w + a_plan, plan_bytes, sizes, st))) return rc;
    const uint64_t image = sizes->image_bytes, surv = sizes->survivors, total = image + rest_bytes;
    new_seg_base[0] = 0, new_seg_bytes[0] = image;
    for (uint64_t s = cs; s < num_segments; ++s)
        new_seg_base[s - cs + 1] = seg_base[s] - rest_at + image, new_seg_bytes[s - cs + 1] = seg_bytes[s];
    if (total > dst_cap || surv + rest_records + 1 > new_rec_cap)
        return fail(SEB_ERR_RANGE, "%s: the new pool needs %llu bytes and %llu offsets", who, (unsigned long long)total,
                    (unsigned long long)(surv + rest_records + 1));
    if (total >= seb::kHidxPoolLimit) return hidx_rc(-2, who);
    if (total && !dst_pool) return fail(SEB_ERR_INVALID, "%s: null destination pool", who);
    if ((rc = seb_dev_seg_compact_emit(dev_pool, pool_bytes, doff, n, timestamp, sizes, w + a_plan, plan_bytes, dst_pool,
                                       new_rec_off, st)))
        return rc;
    if (rest_bytes) HIP_OR_FAIL(hipMemcpyAsync(dst_pool + image, dev_pool + rest_at, rest_bytes, hipMemcpyDeviceToDevice, st));
    HIP_OR_FAIL(launch_offsets_shift(rest_rec_off, rest_records, rest_at, image, new_rec_off + surv, total, st));
    if ((rc = seb_dev_hidx_clear(dev_table, capacity, st))) return rc;
    // the new image lies at the lowest offsets, so the segments that stay still win
    if ((rc = seb_dev_hidx_insert(dev_table, capacity, dst_pool, total, new_rec_off, nullptr, surv, st))) return rc;
    if ((rc = seb_dev_hidx_insert(dev_table, capacity, dst_pool, total, new_rec_off + surv, rest_live, rest_records, st))) return rc;
    uint64_t keys = 0;
    if ((rc = seb_dev_hidx_count(dev_table, capacity, &keys, nullptr, st))) return rc;  // synchronises
    if (distinct) *distinct = keys;
    return SEB_OK;
}
