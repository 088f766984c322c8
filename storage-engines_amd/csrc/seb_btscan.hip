// seb_btscan.hip — the B-tree's range scans on the device: the leaf directory of a checked image and
// Scan for a batch of ranges.  The directory's layout, the position arithmetic, the cell locate and the chain / order
// rule are seb_btree.h's, the text the host half (seb_btscan.cpp) compiles too; this file adds how the work is spread.
//
// The directory is derived top-down, a round per level, and never follows the leaf chain:
//   k_dir_count     a lane per page of the level's list: the page must be good, at this level and of the kind of the
//                   list's first page (the least offender per rule through an atomicMin of position << 32 | page); its
//                   children (numCells + 1) or, on a leaf, its cells are scanned within the wave (kDirTile = 64 pages
//                   per tile), the tile's sum goes to sums[].
//   k_bt_tile_scan  the exclusive scan of the tiles' sums (scan_tile_sums, seb_scan.h: one workgroup, a carry between
//                   stretches of kScanWidth tiles) and the total; the scan plan uses it too.
//   k_dir_scatter   a wave per listed page, lanes striding i <= n as k_bt_level does: the right pointer (the LEFTMOST
//                   child) first, then the cells' children in directory order, into the next level's list.
//   k_dir_leaves    the last list is leaf[]: first[] from the same scan, ord[] scattered.
//   k_dir_verify    a lane per leaf: a leaf listed twice (leaf[ord[p]] != p), then bt_leaf_link's chain and order rule.
// The host reads 64 bytes back per round (the check does the same) and once after the verify.
//
//   k_scan_plan     a lane per range: bt_walk for the start and for the end, each (leaf, pos) turned into a global
//                   position through the directory; the counts scanned within the wave, tile sums as above.
//   k_scan_offsets  range_off[] completed from the scanned tile sums, the plan's header written.
//   k_scan_cells    a lane per OUTPUT ENTRY: a counted bisection of range_off gives its range, one of first[] its leaf,
//                   bt_cell its key's and value's place.  The bytes are then gathered by seb_values.hip's kernels.
//
// Bounds, whatever the image, the directory or the workspace hold: every page id is tested against num_pages before a
// byte of the page is read, every ord / leaf / first index against L <= num_pages, every list index against the list's
// length, both bisections and the walk are counted, and nothing is written outside R / R + 1 / entries elements.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seb_btree.h"
#include "seb_btree_dev.h"
#include "seb_kernels.h"
#include "seb_scan.h"

namespace seb {

namespace {

constexpr uint32_t kDirTile = 64;  // pages (ranges) per tile of the scans: a wave
constexpr uint64_t kWsHead = 256;
constexpr uint64_t kNone = ~0ull;
// the workspace header's u64 words
enum : uint32_t { wTotal = 0, wBad, wLevel, wMixed, wTwice, wChain, wOrder, wKind0, wMagic, wRanges, wWords };
constexpr uint64_t kPlanMagic = 0x42545343414E504Cull;

__device__ __forceinline__ uint64_t wave_excl(uint64_t c, uint32_t lane, uint64_t *incl_out) {
    uint64_t incl = c;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up((unsigned long long)incl, d, 64);
        if (lane >= d) incl += t;
    }
    *incl_out = incl;
    return incl - c;
}

__device__ __forceinline__ void least(u64a *slot, uint64_t pos, uint32_t page) {
    __hip_atomic_fetch_min(slot, (u64a)(pos << 32 | page), HIDX_RLX_AGENT);
}

__global__ __launch_bounds__(256) void k_dir_count(const uint8_t *__restrict__ image, uint32_t np, const uint8_t *__restrict__ kind,
                                                   const uint8_t *__restrict__ level, const uint32_t *__restrict__ list, uint32_t m,
                                                   uint32_t r, uint32_t *__restrict__ excl, uint64_t *__restrict__ sums, u64a *hdr) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256, m64 = ((uint64_t)m + 63) & ~63ull;
    const uint32_t p0 = list[0];
    const uint8_t kind0 = bt_page_id_ok(p0, np) ? kind[p0] : (uint8_t)kBtBad;
    if (blockIdx.x == 0 && threadIdx.x == 0) hdr[wKind0] = kind0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m64; i += stride) {
        uint64_t c = 0;
        if (i < m) {
            const uint32_t p = list[i];
            if (!bt_page_id_ok(p, np) || kind[p] == kBtBad) least(hdr + wBad, i, p);
            else if (level[p] != r) least(hdr + wLevel, i, p);
            else if (kind[p] != kind0) least(hdr + wMixed, i, p);
            else c = bt_be16(image + (uint64_t)p * kBtPage + 1) + (kind0 == kBtInternal ? 1u : 0u);
        }
        uint64_t incl;
        const uint64_t ex = wave_excl(c, lane, &incl);
        if (i < m) excl[i] = (uint32_t)ex;  // at most 64 * 65,536
        if (lane == 63) sums[i / kDirTile] = incl;
    }
}

__global__ __launch_bounds__(kScanWidth) void k_bt_tile_scan(uint64_t *sums, uint64_t tiles, uint64_t *total) {
    scan_tile_sums(sums, tiles, total);
}

__global__ __launch_bounds__(256) void k_dir_scatter(const uint8_t *__restrict__ image, uint32_t np, const uint32_t *__restrict__ list,
                                                     uint32_t m, const uint32_t *__restrict__ excl, const uint64_t *__restrict__ sums,
                                                     uint32_t *__restrict__ next, uint64_t total) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t i = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6; i < m; i += nwaves) {
        const uint32_t p = list[i];
        if (!bt_page_id_ok(p, np)) continue;
        const uint8_t *page = image + (uint64_t)p * kBtPage;
        const uint32_t n = bt_be16(page + 1);
        const bool v1 = page[9] <= 1;
        const uint64_t base = sums[i / kDirTile] + excl[i];
        for (uint32_t j = lane; j <= n; j += 64) {  // j == 0: the right pointer, the LEFTMOST child
            uint32_t child = bt_be32(page + 3);
            if (j) {
                BtCell c;
                child = bt_cell(page, false, v1, j - 1, &c) ? c.child : kBtNoPage;
            }
            if (base + j < total) next[base + j] = child;  // total <= num_pages, the list's room
        }
    }
}

__global__ __launch_bounds__(256) void k_dir_leaves(uint32_t np, const uint32_t *__restrict__ list, uint32_t L,
                                                    const uint32_t *__restrict__ excl, const uint64_t *__restrict__ sums,
                                                    uint64_t total, uint8_t *dir) {
    uint32_t *leaf = (uint32_t *)(dir + kBtDirHeader), *ord = (uint32_t *)(dir + bt_dir_ord_at(np));
    uint64_t *first = (uint64_t *)(dir + bt_dir_first_at(np));
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i <= L; i += stride) {
        if (i == L) {
            first[L] = total;
            continue;
        }
        const uint32_t p = list[i];
        leaf[i] = p, first[i] = sums[i / kDirTile] + excl[i];
        if (p < np) ord[p] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(256) void k_dir_verify(const uint8_t *__restrict__ image, uint32_t np, uint32_t L, uint64_t keys,
                                                    const uint8_t *__restrict__ dir, u64a *hdr) {
    const BtDir d = bt_dir_view(dir, np, L, keys);
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < L; i += stride) {
        const uint32_t p = d.leaf[i];
        if (p >= np || d.ord[p] != i) {
            __hip_atomic_fetch_min(hdr + wTwice, (u64a)p, HIDX_RLX_AGENT);
            continue;
        }
        const uint32_t link = bt_leaf_link(image, d, (uint32_t)i);
        if (link) least(hdr + (link == 1 ? wChain : wOrder), i, p);
    }
}

// the directory as a kernel reads it: its header must be this image's, and L is held to num_pages
__device__ __forceinline__ bool dev_dir(const uint8_t *dir, uint32_t np, uint32_t root, BtDir *d) {
    const uint32_t *h = (const uint32_t *)dir;
    if (h[0] != kBtDirMagic || h[1] != np || h[2] != root || h[3] > np) return false;
    *d = bt_dir_view(dir, np, h[3], *(const uint64_t *)(dir + 16));
    return true;
}

__device__ __forceinline__ bool dev_seek(const uint8_t *image, uint32_t np, uint32_t root, const BtDir &d, const KeyBatch &kb,
                                         uint64_t i, uint64_t empty, uint64_t *g) {
    uint64_t kbeg = i * kb.stride, klen64 = kb.stride;
    if (kb.offsets) {
        kbeg = kb.offsets[i];
        const uint64_t kend = kb.offsets[i + 1];
        klen64 = kend > kbeg ? kend - kbeg : 0;
    }
    if (!klen64) {
        *g = empty;
        return true;
    }
    DevCmp cmp{kb.data + kbeg, (uint32_t)(klen64 < kBtMaxKey ? klen64 : kBtMaxKey), 0, 0};
    key_prefix(kb, cmp.key, cmp.klen, cmp.k0, cmp.k1);
    BtAnswer a;
    bt_walk(image, np, root, nullptr, cmp, &a);
    return bt_dir_position(d, a, g);
}

__global__ __launch_bounds__(256) void k_scan_plan(const uint8_t *__restrict__ image, uint32_t np, uint32_t root,
                                                   const uint8_t *__restrict__ dir, KeyBatch starts, KeyBatch ends, uint64_t limit,
                                                   uint64_t *__restrict__ first_r, uint64_t *__restrict__ range_off,
                                                   uint64_t *__restrict__ sums, uint8_t *__restrict__ range_status) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t R = starts.n, stride = (uint64_t)gridDim.x * 256, r64 = (R + 63) & ~63ull;
    BtDir d;
    const bool have = dev_dir(dir, np, root, &d);
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < r64; r += stride) {
        uint64_t c = 0;
        if (r < R) {
            uint64_t a = 0, b = 0;
            const bool ok = have && dev_seek(image, np, root, d, starts, r, 0, &a) && dev_seek(image, np, root, d, ends, r, d.keys, &b);
            range_status[r] = ok ? 0 : kBtError;
            first_r[r] = a;
            c = ok ? bt_range_count(a, b, limit) : 0;
        }
        uint64_t incl;
        const uint64_t ex = wave_excl(c, lane, &incl);
        if (r < R) range_off[r] = ex;
        if (lane == 63) sums[r / kDirTile] = incl;
    }
}

__global__ __launch_bounds__(256) void k_scan_offsets(uint64_t R, uint64_t *__restrict__ range_off, const uint64_t *__restrict__ sums,
                                                      uint64_t *hdr) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r <= R; r += stride) {
        if (r == R) range_off[R] = hdr[wTotal], hdr[wMagic] = kPlanMagic, hdr[wRanges] = R;
        else range_off[r] += sums[r / kDirTile];
    }
}

struct ScanOut {
    uint64_t *range_off;
    uint8_t *status, *source;
    uint64_t *kloc;
    uint32_t *klen;
    uint64_t *vloc;
    uint32_t *vlen;
};

__global__ __launch_bounds__(256) void k_scan_cells(const uint8_t *__restrict__ image, uint32_t np, uint32_t root,
                                                    const uint8_t *__restrict__ dir, const uint64_t *__restrict__ hdr, uint64_t R,
                                                    uint64_t entries, const uint64_t *__restrict__ first_r,
                                                    const uint64_t *__restrict__ range_off, ScanOut out) {
    if (hdr[wMagic] != kPlanMagic || hdr[wRanges] != R || hdr[wTotal] != entries) return;  // another plan's workspace
    BtDir d;
    const bool have = dev_dir(dir, np, root, &d);
    const uint64_t stride = (uint64_t)gridDim.x * 256, items = entries > R + 1 ? entries : R + 1;
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < items; e += stride) {
        if (e <= R) out.range_off[e] = range_off[e];
        if (e >= entries) continue;
        const uint64_t r = bt_upper_index(range_off, R, e);
        const uint64_t begin = range_off[r];
        BtEntry c{kBtError, 0, 0, 0, 0};
        if (have && begin <= e) c = bt_scan_entry(image, d, first_r[r] + (e - begin));
        out.status[e] = c.status, out.source[e] = 1;
        out.kloc[e] = c.kloc, out.klen[e] = c.klen, out.vloc[e] = c.vloc, out.vlen[e] = c.vlen;
    }
}

inline hipError_t drained(hipStream_t s, hipError_t e) {
    (void)hipStreamSynchronize(s);
    return e;
}

inline uint64_t tiles_of(uint64_t n) { return (n + kDirTile - 1) / kDirTile; }

}  // namespace

uint32_t bt_dir_tile() { return kDirTile; }

uint64_t bt_dir_ws_bytes(uint32_t np) { return kWsHead + ((12ull * np + 15) & ~15ull) + 8 * (tiles_of(np) + 1); }

hipError_t launch_bt_dir_build(const uint8_t *image, uint32_t np, uint32_t root, const uint8_t *kind, const uint8_t *level,
                               uint8_t *dir, void *ws, BtDirInfo *info_host, int *rule_host, uint32_t *page_host, hipStream_t s) {
    *info_host = BtDirInfo{0, 0, 0, 0}, *rule_host = 0, *page_host = 0;
    hipError_t e;
    if ((e = hipMemsetAsync(dir, 0, bt_dir_bytes(np), s)) != hipSuccess) return e;
    if (!bt_page_id_ok(root, np)) {
        *rule_host = kDirRoot, *page_host = root;
        return hipStreamSynchronize(s);
    }
    if ((e = hipMemsetAsync(dir + bt_dir_ord_at(np), 0xFF, 4ull * np, s)) != hipSuccess) return e;
    u64a *hdr = (u64a *)ws;
    uint32_t *list = (uint32_t *)((uint8_t *)ws + kWsHead), *next = list + np, *excl = next + np;
    uint64_t *sums = (uint64_t *)((uint8_t *)ws + kWsHead + ((12ull * np + 15) & ~15ull));
    if ((e = hipMemcpyAsync(list, &root, 4, hipMemcpyHostToDevice, s)) != hipSuccess) return drained(s, e);
    uint64_t h[wWords];
    uint32_t m = 1;
    auto refused = [&](int rule, uint64_t word) {
        *rule_host = rule, *page_host = (uint32_t)word;
        return hipSuccess;
    };
    for (uint32_t r = 0; r < kBtMaxDepth; ++r) {
        if ((e = hipMemsetAsync(hdr, 0xFF, kWsHead, s)) != hipSuccess) return drained(s, e);
        hipLaunchKernelGGL(k_dir_count, dim3(stream_grid(((uint64_t)m + 63) & ~63ull)), dim3(256), 0, s, image, np, kind, level,
                           (const uint32_t *)list, m, r, excl, sums, hdr);
        if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
        hipLaunchKernelGGL(k_bt_tile_scan, dim3(1), dim3(kScanWidth), 0, s, sums, tiles_of(m), (uint64_t *)hdr + wTotal);
        if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
        if ((e = hipMemcpyAsync(h, hdr, sizeof h, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        // the least position over the three page rules; a position reports one rule only
        uint64_t worst = kNone;
        int rule = 0;
        for (uint32_t w = wBad; w <= wMixed; ++w)
            if (h[w] < worst) worst = h[w], rule = kDirBad + (int)(w - wBad);
        if (rule) return refused(rule, worst);
        const uint64_t total = h[wTotal];
        if (h[wKind0] == kBtLeaf) {
            const uint32_t L = m;
            hipLaunchKernelGGL(k_dir_leaves, dim3(stream_grid((uint64_t)L + 1)), dim3(256), 0, s, np, (const uint32_t *)list, L,
                               (const uint32_t *)excl, (const uint64_t *)sums, total, dir);
            if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
            hipLaunchKernelGGL(k_dir_verify, dim3(stream_grid(L)), dim3(256), 0, s, image, np, L, total, (const uint8_t *)dir, hdr);
            if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
            if ((e = hipMemcpyAsync(h, hdr, sizeof h, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
            if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
            if (h[wTwice] != kNone) return refused(kDirTwice, h[wTwice]);
            if (h[wChain] != kNone) return refused(kDirChain, h[wChain]);
            if (h[wOrder] != kNone) return refused(kDirOrder, h[wOrder]);
            struct {
                uint32_t magic, np, root, leaves;
                uint64_t keys;
                uint32_t depth, zero;
            } head{kBtDirMagic, np, root, L, total, r + 1, 0};
            static_assert(sizeof head == kBtDirHeader, "the directory's header");
            if ((e = hipMemcpyAsync(dir, &head, sizeof head, hipMemcpyHostToDevice, s)) != hipSuccess) return drained(s, e);
            if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
            *info_host = BtDirInfo{L, total, r + 1, 0};
            return hipSuccess;
        }
        uint32_t first_page = 0;
        if (r + 1 == kBtMaxDepth || total > np) {
            if ((e = hipMemcpyAsync(&first_page, list, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
            if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
            return refused(r + 1 == kBtMaxDepth ? kDirDeep : kDirWide, first_page);
        }
        hipLaunchKernelGGL(k_dir_scatter, dim3(stream_grid(64ull * m)), dim3(256), 0, s, image, np, (const uint32_t *)list, m,
                           (const uint32_t *)excl, (const uint64_t *)sums, next, total);
        if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
        uint32_t *t = list;
        list = next, next = t, m = (uint32_t)total;
    }
    return hipSuccess;  // not reached: the last round returns
}

uint64_t bt_scan_ws_bytes(uint64_t R) { return kWsHead + 8 * R + 8 * (R + 1) + 8 * (tiles_of(R) + 1); }

hipError_t bt_scan_read_dir(const uint8_t *dir, uint8_t head_host[32], hipStream_t s) {
    hipError_t e;
    if ((e = hipMemcpyAsync(head_host, dir, kBtDirHeader, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    return hipStreamSynchronize(s);
}

hipError_t launch_bt_scan_plan(const uint8_t *image, uint32_t np, uint32_t root, const uint8_t *dir, const KeyBatch &starts,
                               const KeyBatch &ends, uint64_t limit, void *ws, uint8_t *range_status, uint64_t *entries_host,
                               hipStream_t s) {
    const uint64_t R = starts.n;
    uint64_t *hdr = (uint64_t *)ws, *first_r = (uint64_t *)((uint8_t *)ws + kWsHead), *range_off = first_r + R, *sums = range_off + R + 1;
    hipError_t e;
    if ((e = hipMemsetAsync(hdr, 0, kWsHead, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_scan_plan, dim3(stream_grid((R + 63) & ~63ull)), dim3(256), 0, s, image, np, root, dir, starts, ends, limit,
                       first_r, range_off, sums, range_status);
    if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
    hipLaunchKernelGGL(k_bt_tile_scan, dim3(1), dim3(kScanWidth), 0, s, sums, tiles_of(R), hdr + wTotal);
    if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
    hipLaunchKernelGGL(k_scan_offsets, dim3(stream_grid(R + 1)), dim3(256), 0, s, R, range_off, (const uint64_t *)sums, hdr);
    if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
    if ((e = hipMemcpyAsync(entries_host, hdr + wTotal, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    return hipStreamSynchronize(s);
}

hipError_t launch_bt_scan_cells(const uint8_t *image, uint32_t np, uint32_t root, const uint8_t *dir, uint64_t R, uint64_t entries,
                                const void *ws, uint64_t *range_off, uint8_t *status, uint8_t *source, uint64_t *kloc, uint32_t *klen,
                                uint64_t *vloc, uint32_t *vlen, hipStream_t s) {
    const uint64_t *hdr = (const uint64_t *)ws, *first_r = (const uint64_t *)((const uint8_t *)ws + kWsHead), *ws_off = first_r + R;
    const ScanOut out{range_off, status, source, kloc, klen, vloc, vlen};
    const uint64_t items = entries > R + 1 ? entries : R + 1;
    hipLaunchKernelGGL(k_scan_cells, dim3(stream_grid(items)), dim3(256), 0, s, image, np, root, dir, hdr, R, entries, first_r, ws_off, out);
    return hipGetLastError();
}

}  // namespace seb
