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

// ------------------------------------------------ range scans: the leaf directory, batched Scan

static_assert(sizeof(seb_bt_dir_info) == sizeof(seb::BtDirInfo) && sizeof(seb_bt_dir_info) == 24, "seb_bt_dir_info layout");
static_assert(sizeof(seb_bt_scan_sizes) == sizeof(seb::BtScanSizes) && sizeof(seb_bt_scan_sizes) == 32, "seb_bt_scan_sizes layout");
static_assert(SEB_BT_DIR_MAGIC == seb::kBtDirMagic, "the directory's magic");

static int dir_refused(int rule, uint32_t page, const char *who) {
    return fail(SEB_ERR_INVALID, "%s: page %u: %s", who, page, bt_dir_rule_text(rule));
}

static int scan_rc(int rc, const seb_bt_scan_sizes *sz, const char *who) {
    switch (rc) {
    case -6:
        return fail(SEB_ERR_INVALID, "%s: dir is not the directory of this image", who);
    case -7:
        return fail(SEB_ERR_RANGE, "%s: a cap is below the scan's %llu entries, %llu key bytes, %llu value bytes; retry with *sizes",
                    who, (unsigned long long)sz->entries, (unsigned long long)sz->key_bytes, (unsigned long long)sz->val_bytes);
    case -8:
        return fail(SEB_ERR_RANGE, "%s: the ranges hold 2^32 entries or more (%llu)", who, (unsigned long long)sz->entries);
    default:
        return bt_rc(rc, who);
    }
}

extern "C" uint64_t seb_bt_dir_bytes(uint32_t num_pages) { return seb::bt_dir_bytes(num_pages); }

extern "C" int seb_bt_dir_build(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, const uint8_t *kind,
                                const uint8_t *level, uint8_t *dir, seb_bt_dir_info *info) {
    const char *who = "seb_bt_dir_build";
    if (!meta) return bt_rc(-1, who);
    if ((uintptr_t)dir & 7) return fail(SEB_ERR_INVALID, "%s: dir is not 8-byte aligned", who);
    int rule = 0;
    uint32_t page = 0;
    const int rc = seb::bt_dir_build(image, image_bytes, meta_of(meta), kind, level, dir, reinterpret_cast<BtDirInfo *>(info), &rule, &page);
    return rc == -5 ? dir_refused(rule, page, who) : bt_rc(rc, who);
}

static BtKeys host_keys(const seb_keys *k) { return BtKeys{k->data, k->offsets, k->n, k->stride}; }

extern "C" int seb_bt_scan(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, const uint8_t *dir,
                           const seb_keys *starts, const seb_keys *ends, uint64_t limit, uint8_t *range_status, uint64_t *range_off,
                           uint8_t *status, uint8_t *source, uint64_t *kloc, uint32_t *klen, uint64_t *vloc, uint32_t *vlen,
                           uint64_t entry_cap, uint64_t *key_off, uint8_t *keys, uint64_t key_cap, uint64_t *val_off, uint8_t *vals,
                           uint64_t val_cap, seb_bt_scan_sizes *sizes) {
    const char *who = "seb_bt_scan";
    int rc;
    if (!meta || !sizes) return bt_rc(-1, who);
    if ((rc = check_keys(starts, who)) || (rc = validate_offsets(starts, who)) || (rc = check_keys(ends, who)) ||
        (rc = validate_offsets(ends, who)))
        return rc;
    if (starts->n != ends->n) return fail(SEB_ERR_INVALID, "%s: %llu starts, %llu ends", who, (unsigned long long)starts->n,
                                          (unsigned long long)ends->n);
    if ((uintptr_t)dir & 7) return fail(SEB_ERR_INVALID, "%s: dir is not 8-byte aligned", who);
    const BtScanOut out{range_status, range_off, status, source, kloc, vloc, klen, vlen, entry_cap, key_off, val_off, keys, vals, key_cap, val_cap};
    rc = seb::bt_scan(image, image_bytes, meta_of(meta), dir, host_keys(starts), host_keys(ends), limit, out,
                      reinterpret_cast<BtScanSizes *>(sizes));
    return scan_rc(rc, sizes, who);
}

extern "C" uint64_t seb_dev_bt_dir_workspace_size(uint32_t num_pages) { return bt_dir_ws_bytes(num_pages); }

extern "C" int seb_dev_bt_dir_build(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, const uint8_t *kind,
                                    const uint8_t *level, uint8_t *dir, void *workspace, uint64_t workspace_bytes,
                                    seb_bt_dir_info *info, void *stream) {
    const char *who = "seb_dev_bt_dir_build";
    enter();
    int rc;
    if ((rc = check_image(image, image_bytes, meta, who))) return rc;
    if (!dir || !info || !workspace || (meta->num_pages && (!kind || !level))) return bt_rc(-1, who);
    if (((uintptr_t)dir & 7) || ((uintptr_t)workspace & 15))
        return fail(SEB_ERR_INVALID, "%s: dir is not 8-byte aligned or the workspace not 16-byte aligned", who);
    if (workspace_bytes < bt_dir_ws_bytes(meta->num_pages))
        return fail(SEB_ERR_INVALID, "%s: workspace %llu < %llu bytes for %u pages", who, (unsigned long long)workspace_bytes,
                    (unsigned long long)bt_dir_ws_bytes(meta->num_pages), meta->num_pages);
    int rule = 0;
    uint32_t page = 0;
    HIP_OR_FAIL(launch_bt_dir_build(image, meta->num_pages, meta->root, kind, level, dir, workspace, reinterpret_cast<BtDirInfo *>(info),
                                    &rule, &page, (hipStream_t)stream));
    return rule ? dir_refused(rule, page, who) : SEB_OK;
}

extern "C" uint64_t seb_dev_bt_scan_workspace_size(uint64_t ranges) { return ranges >= (1ull << 32) ? 0 : bt_scan_ws_bytes(ranges); }

// what the plan and the cells test alike
static int scan_args(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, const uint8_t *dir, uint64_t ranges,
                     const void *workspace, uint64_t workspace_bytes, const char *who) {
    int rc;
    if ((rc = check_image(image, image_bytes, meta, who))) return rc;
    if (ranges >= (1ull << 32)) return fail(SEB_ERR_INVALID, "%s: 2^32 ranges or more", who);
    if (!dir) return bt_rc(-1, who);
    if ((uintptr_t)dir & 7) return fail(SEB_ERR_INVALID, "%s: dir is not 8-byte aligned", who);
    if (ranges == 0) return SEB_OK;
    if (!workspace) return bt_rc(-1, who);
    if ((uintptr_t)workspace & 7) return fail(SEB_ERR_INVALID, "%s: the workspace is not 8-byte aligned", who);
    if (workspace_bytes < bt_scan_ws_bytes(ranges))
        return fail(SEB_ERR_INVALID, "%s: workspace %llu < %llu bytes for %llu ranges", who, (unsigned long long)workspace_bytes,
                    (unsigned long long)bt_scan_ws_bytes(ranges), (unsigned long long)ranges);
    return SEB_OK;
}

extern "C" int seb_dev_bt_scan_plan(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, const uint8_t *dir,
                                    const seb_keys *starts, const seb_keys *ends, uint64_t limit, uint8_t *range_status,
                                    void *workspace, uint64_t workspace_bytes, seb_bt_scan_sizes *sizes, void *stream) {
    const char *who = "seb_dev_bt_scan_plan";
    enter();
    int rc;
    if (!sizes) return bt_rc(-1, who);
    *sizes = seb_bt_scan_sizes{0, 0, 0, 0};
    if ((rc = check_keys(starts, who)) || (rc = check_keys(ends, who))) return rc;
    if (starts->n != ends->n) return fail(SEB_ERR_INVALID, "%s: %llu starts, %llu ends", who, (unsigned long long)starts->n,
                                          (unsigned long long)ends->n);
    sizes->ranges = starts->n;
    if ((rc = scan_args(image, image_bytes, meta, dir, starts->n, workspace, workspace_bytes, who))) return rc;
    if (((uintptr_t)starts->offsets & 7) || ((uintptr_t)ends->offsets & 7)) return fail(SEB_ERR_INVALID, "%s: offsets not 8-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    uint8_t head[32];
    uint32_t leaves;
    uint64_t keys;
    HIP_OR_FAIL(bt_scan_read_dir(dir, head, s));
    if (!bt_dir_header_ok(head, meta_of(meta), &leaves, &keys)) return scan_rc(-6, sizes, who);
    if (starts->n == 0) return SEB_OK;
    if (!range_status) return fail(SEB_ERR_INVALID, "%s: null range_status", who);
    HIP_OR_FAIL(launch_bt_scan_plan(image, meta->num_pages, meta->root, dir, key_batch(starts), key_batch(ends), limit, workspace,
                                    range_status, &sizes->entries, s));
    return sizes->entries >> 32 ? scan_rc(-8, sizes, who) : SEB_OK;
}

extern "C" int seb_dev_bt_scan_cells(const uint8_t *image, uint64_t image_bytes, const seb_bt_meta *meta, const uint8_t *dir,
                                     const seb_bt_scan_sizes *sizes, const void *workspace, uint64_t workspace_bytes,
                                     uint64_t *range_off, uint8_t *status, uint8_t *source, uint64_t *kloc, uint32_t *klen,
                                     uint64_t *vloc, uint32_t *vlen, void *stream) {
    const char *who = "seb_dev_bt_scan_cells";
    enter();
    int rc;
    if (!sizes) return bt_rc(-1, who);
    if ((rc = scan_args(image, image_bytes, meta, dir, sizes->ranges, workspace, workspace_bytes, who))) return rc;
    if (sizes->entries >> 32) return scan_rc(-8, sizes, who);
    if (!range_off || (sizes->entries && (!status || !source || !kloc || !klen || !vloc || !vlen))) return bt_rc(-1, who);
    if (((uintptr_t)range_off & 7) || ((uintptr_t)kloc & 7) || ((uintptr_t)vloc & 7) || ((uintptr_t)klen & 3) || ((uintptr_t)vlen & 3))
        return fail(SEB_ERR_INVALID, "%s: range_off, kloc or vloc not 8-byte aligned, or klen or vlen not 4-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    if (sizes->ranges == 0) {
        HIP_OR_FAIL(hipMemsetAsync(range_off, 0, 8, s));
        return SEB_OK;
    }
    HIP_OR_FAIL(launch_bt_scan_cells(image, meta->num_pages, meta->root, dir, sizes->ranges, sizes->entries, workspace, range_off, status,
                                     source, kloc, klen, vloc, vlen, s));
    return SEB_OK;
}
