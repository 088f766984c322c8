// seb_bt.cpp — the B-tree read side's entry points: the C ABI over its host half (seb_btree.cpp) and
// its kernels (seb_btree.hip), and seb_bt_load, open + upload + check of a host image through a context.
#include "seb_btree.h"
#include "seb_host.h"

using namespace seb;

static_assert(SEB_BT_PAGE_BYTES == seb::kBtPage && SEB_BT_MAGIC == seb::kBtMagic && SEB_BT_MAX_DEPTH == seb::kBtMaxDepth &&
                  SEB_BT_NO_PAGE == seb::kBtNoPage && SEB_BT_NO_LEVEL == seb::kBtNoLevel,
              "the B-tree's constants");
static_assert(SEB_BT_PAGE_BAD == seb::kBtBad && SEB_BT_PAGE_INTERNAL == seb::kBtInternal && SEB_BT_PAGE_LEAF == seb::kBtLeaf &&
                  SEB_GET_MISS == seb::kBtMiss && SEB_GET_FOUND == seb::kBtFound && SEB_GET_ERROR == seb::kBtError,
              "the B-tree's page kinds and statuses");
static_assert(sizeof(seb_bt_meta) == sizeof(seb::BtMeta) && sizeof(seb_bt_meta) == 16, "seb_bt_meta layout");
static_assert(sizeof(seb_bt_stats) == sizeof(seb::BtStats) && sizeof(seb_bt_stats) == 64, "seb_bt_stats layout");

static int bt_rc(int rc, const char *who) {
    switch (rc) {
    case 0:
        return SEB_OK;
    case -2:
        return fail(SEB_ERR_INVALID, "%s: the image has fewer than 4096 bytes or a wrong magic (ErrInvalidDatabase)", who);
    case -3:
        return fail(SEB_ERR_INVALID, "%s: meta->num_pages pages do not fit image_bytes", who);
    case -4:
        return fail(SEB_ERR_NOMEM, "%s: out of host memory", who);
    default:
        return fail(SEB_ERR_INVALID, "%s: a null argument", who);
    }
}

static const BtMeta &meta_of(const seb_bt_meta *m) { return *reinterpret_cast<const BtMeta *>(m); }

// ------------------------------------------------ host only

extern "C" int seb_bt_open(const uint8_t *image, uint64_t image_bytes, seb_bt_meta *meta) {
    return bt_rc(seb::bt_open(image, image_bytes, reinterpret_cast<BtMeta *>(meta)), "seb_bt_open");
}

extern "C" int seb_bt_check(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, uint8_t *kind, uint8_t *level,
                            seb_bt_stats *stats) {
    const char *who = "seb_bt_check";
    if (!meta) return bt_rc(-1, who);
    return bt_rc(seb::bt_check(image, image_bytes, meta_of(meta), kind, level, reinterpret_cast<BtStats *>(stats)), who);
}

extern "C" int seb_bt_get(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, const seb_keys *keys,
                          uint8_t *status, uint32_t *leaf, uint32_t *pos, uint64_t *vloc, uint32_t *vlen) {
    const char *who = "seb_bt_get";
    int rc;
    if (!meta) return bt_rc(-1, who);
    if ((rc = check_keys(keys, who)) || (rc = validate_offsets(keys, who))) return rc;
    return bt_rc(seb::bt_get(image, image_bytes, meta_of(meta), BtKeys{keys->data, keys->offsets, keys->n, keys->stride}, status, leaf,
                             pos, vloc, vlen),
                 who);
}

// ------------------------------------------------ device

static int check_image(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, const char *who) {
    if (!meta) return bt_rc(-1, who);
    if (meta->num_pages && !image) return fail(SEB_ERR_INVALID, "%s: null image", who);
    if (meta->num_pages > (1u << 31)) return fail(SEB_ERR_INVALID, "%s: more than 2^31 pages", who);  // the kernels' page loops
    if ((uint64_t)meta->num_pages * kBtPage > image_bytes) return bt_rc(-3, who);
    return SEB_OK;
}

extern "C" int seb_dev_bt_check(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, uint8_t *kind, uint8_t *level,
                                seb_bt_stats *stats, void *stream) {
    const char *who = "seb_dev_bt_check";
    WsCall ws_call;
    enter();
    int rc;
    if ((rc = check_image(image, image_bytes, meta, who))) return rc;
    hipStream_t s = (hipStream_t)stream;
    void *ws = nullptr;
    if (meta->num_pages && (rc = cached_workspace(s, bt_check_ws_bytes(meta->num_pages), &ws, 5))) return rc;
    BtStats got;
    HIP_OR_FAIL(launch_bt_check(image, meta->num_pages, meta->root, kind, level, ws, &got, s));
    if (stats) *reinterpret_cast<BtStats *>(stats) = got;
    return SEB_OK;
}

extern "C" int seb_dev_bt_get(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, const seb_keys *keys,
                              uint8_t *status, uint32_t *leaf, uint32_t *pos, uint64_t *vloc, uint32_t *vlen, uint8_t *source,
                              void *stream) {
    const char *who = "seb_dev_bt_get";
    enter();
    int rc;
    if ((rc = check_keys(keys, who)) || (rc = check_image(image, image_bytes, meta, who))) return rc;
    if (keys->n == 0) return SEB_OK;
    if (!status) return fail(SEB_ERR_INVALID, "%s: null status", who);
    if (((uintptr_t)keys->offsets & 7) || ((uintptr_t)vloc & 7) || ((uintptr_t)leaf & 3) || ((uintptr_t)pos & 3) || ((uintptr_t)vlen & 3))
        return fail(SEB_ERR_INVALID, "%s: offsets or vloc not 8-byte aligned, or leaf, pos or vlen not 4-byte aligned", who);
    HIP_OR_FAIL(launch_bt_get(image, meta->num_pages, meta->root, key_batch(keys), status, leaf, pos, vloc, vlen, source,
                              (hipStream_t)stream));
    return SEB_OK;
}

// A host image through the context: readMetadata on the host, the pages up and the check on the compute stream.
extern "C" int seb_bt_load(seb_ctx *c, const uint8_t *image, uint64_t image_bytes, uint8_t *dev_image, uint64_t cap,
                           uint8_t *dev_kind, uint8_t *dev_level, seb_bt_meta *meta, seb_bt_stats *stats) {
    const char *who = "seb_bt_load";
    int rc;
    if (!c) return fail(SEB_ERR_INVALID, "%s: null ctx", who);
    if (!meta) return bt_rc(-1, who);
    if (stats) *stats = seb_bt_stats{};
    if ((rc = seb_bt_open(image, image_bytes, meta))) return rc;
    const uint64_t bytes = (uint64_t)meta->num_pages * kBtPage;
    if (bytes > cap)
        return fail(SEB_ERR_RANGE, "%s: cap %llu is below the pages' %llu bytes", who, (unsigned long long)cap,
                    (unsigned long long)bytes);
    if (!dev_image) return fail(SEB_ERR_INVALID, "%s: null device image", who);
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OR_FAIL(hipSetDevice(c->device));
    hipStream_t st = c->s_comp;
    HIP_OR_FAIL(hipMemcpyAsync(dev_image, image, bytes, hipMemcpyHostToDevice, st));
    rc = seb_dev_bt_check(dev_image, bytes, meta, dev_kind, dev_level, stats, st);  // synchronises
    if (rc) (void)hipStreamSynchronize(st);  // the caller's image is not read after the return
    return rc;
}
