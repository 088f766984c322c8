// seb_btree.hip — the B-tree's read side on the device: the structural check of a page-file image
// and Get for a key batch.  The page codec, the page rules and the walk are seb_btree.h's, the text the host half
// compiles too; this file adds how the work is spread and how a key is compared.
//
//   k_bt_check   a wave per page, lanes striding the directory: each lane parses cell i and cell i + 1 and compares
//                them (strictly increasing keys; an internal cell's child inside the image); kind[p] by lane 0.
//   k_bt_level   one round of the levels: a wave per page of level r that is a good internal page hands r + 1 to its
//                children with an agent-scope atomicMin; a round that lowered nothing ends the rounds (the host reads
//                the round's counter back: the check synchronises anyway).
//   k_bt_stats   a lane per page: level[p] as a byte, and the counts, summed per wave and added with one atomic per
//                wave and counter.
//   k_bt_get     a lane per key.  The key's 16-byte big-endian prefix is built once (seb_keycmp.h); every page is
//                bisected with dependent loads: a directory entry, the cell's header, the key bytes.  Every key's
//                first page is the root: with kLdsRoot the workgroup copies it into LDS once (4 KiB) and the first
//                log2(n_root) steps read LDS.  SEB_BT_LDS_ROOT is the build switch, OFF by default: measured on a
//                10M-key tree it gains 5% on a sorted batch and loses 2% on a shuffled one (DESIGN.md 5.21 has both
//                figures); the root's few lines are cache-resident either way.
//
// Bounds, whatever the image holds: a page id is tested against num_pages before a byte of the page is read, every
// offset inside a page against 4096 before it is used (seb_btree.h), both loops of the walk are counted, and nothing is
// written outside the n elements of the outputs.  The image may lie at any byte alignment: pages are read bytewise,
// key prefixes through the aligned dwords that cover them (ld_u64_le), and the LDS copy of the root through the
// aligned 16-byte chunks that cover it, each of which holds at least one byte of the page.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seb_btree.h"
#include "seb_btree_dev.h"  // DevCmp; seb_hidx_dev.h's ld_u64_le, prefix_words, u64a and the agent-scope atomics' spelling
#include "seb_kernels.h"

#ifndef SEB_BT_LDS_ROOT
#define SEB_BT_LDS_ROOT 0
#endif

namespace seb {

namespace {

enum : uint32_t { bLeaves = 0, bInternals, bBad, bReachLeaves, bReachInternals, bReachBad, bKeys, bDepth, bLeafLoInv, bLeafHi1, bWords };
constexpr uint64_t kBtWsHead = 256;  // u64 counts[16], u32 changed[32]

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(256) void k_bt_check(const uint8_t *__restrict__ image, uint32_t np, uint8_t *__restrict__ kind) {
    const uint32_t lane = threadIdx.x & 63, nwaves = gridDim.x * 4;
    for (uint32_t p = (blockIdx.x * 256 + threadIdx.x) >> 6; p < np; p += nwaves) {
        uint8_t k = kBtBad;
        if (p) {
            const uint8_t *page = image + (uint64_t)p * kBtPage;
            uint32_t n;
            k = bt_page_head(page, np, &n);
            if (k != kBtBad) {
                const bool leaf = k == kBtLeaf, v1 = page[9] <= 1;
                bool ok = true;
                for (uint32_t i = lane; i < n && ok; i += 64) ok = bt_cell_good(page, leaf, v1, n, i, np);
                if (__ballot(!ok)) k = kBtBad;
            }
        }
        if (lane == 0) kind[p] = k;
    }
}

__global__ __launch_bounds__(256) void k_bt_level(const uint8_t *__restrict__ image, uint32_t np, const uint8_t *__restrict__ kind,
                                                  uint32_t *lev, uint32_t r, uint32_t *changed) {
    const uint32_t lane = threadIdx.x & 63, nwaves = gridDim.x * 4;
    for (uint32_t p = ((blockIdx.x * 256 + threadIdx.x) >> 6) + 1; p < np; p += nwaves) {
        if (__hip_atomic_load(lev + p, HIDX_RLX_AGENT) != r || kind[p] != kBtInternal) continue;
        const uint8_t *page = image + (uint64_t)p * kBtPage;
        const uint32_t n = bt_be16(page + 1);
        const bool v1 = page[9] <= 1;
        bool lowered = false;
        for (uint32_t i = lane; i <= n; i += 64) {  // i == n: the right pointer
            BtCell c;
            uint32_t child = bt_be32(page + 3);
            if (i < n) {
                if (!bt_cell(page, false, v1, i, &c)) continue;
                child = c.child;
            }
            if (bt_page_id_ok(child, np)) lowered |= __hip_atomic_fetch_min(lev + child, r + 1, HIDX_RLX_AGENT) > r + 1;
        }
        if (__ballot(lowered) && lane == 0) __hip_atomic_fetch_add(changed, 1u, HIDX_RLX_AGENT);
    }
}

__global__ __launch_bounds__(256) void k_bt_stats(const uint8_t *__restrict__ image, uint32_t np, const uint8_t *__restrict__ kind,
                                                  const uint32_t *__restrict__ lev, uint8_t *__restrict__ level, u64a *counts) {
    const uint32_t stride = gridDim.x * 256;
    u64a sum[bDepth] = {0, 0, 0, 0, 0, 0, 0};
    uint32_t depth = 0, leaf_lo_inv = 0, leaf_hi1 = 0;
    for (uint32_t p = blockIdx.x * 256 + threadIdx.x; p < np; p += stride) {
        const uint32_t l = lev[p] < kBtNoLevel ? lev[p] : kBtNoLevel;
        if (level) level[p] = (uint8_t)l;
        if (p == 0) continue;
        const uint8_t k = kind[p];
        const uint32_t slot = k == kBtLeaf ? bLeaves : k == kBtInternal ? bInternals : bBad;
        ++sum[slot];
        if (l == kBtNoLevel) continue;
        ++sum[slot + bReachLeaves];
        depth = l + 1 > depth ? l + 1 : depth;
        if (k == kBtLeaf) {
            sum[bKeys] += bt_be16(image + (uint64_t)p * kBtPage + 1);
            leaf_hi1 = l + 1 > leaf_hi1 ? l + 1 : leaf_hi1;
            leaf_lo_inv = 256 - l > leaf_lo_inv ? 256 - l : leaf_lo_inv;
        }
    }
    for (uint32_t j = 0; j < bDepth; ++j) sum[j] = wave_sum(sum[j]);
    depth = wave_max(depth), leaf_hi1 = wave_max(leaf_hi1), leaf_lo_inv = wave_max(leaf_lo_inv);
    if ((threadIdx.x & 63) == 0) {
        for (uint32_t j = 0; j < bDepth; ++j)
            if (sum[j]) __hip_atomic_fetch_add(counts + j, sum[j], HIDX_RLX_AGENT);
        if (depth) __hip_atomic_fetch_max(counts + bDepth, (u64a)depth, HIDX_RLX_AGENT);
        if (leaf_hi1) __hip_atomic_fetch_max(counts + bLeafHi1, (u64a)leaf_hi1, HIDX_RLX_AGENT);
        if (leaf_lo_inv) __hip_atomic_fetch_max(counts + bLeafLoInv, (u64a)leaf_lo_inv, HIDX_RLX_AGENT);
    }
}

struct BtOut {
    uint8_t *status;
    uint32_t *leaf, *pos;
    uint64_t *vloc;
    uint32_t *vlen;
    uint8_t *source;
};

template <bool kLdsRoot>
__global__ __launch_bounds__(256) void k_bt_get(const uint8_t *__restrict__ image, uint32_t np, uint32_t root, KeyBatch kb, BtOut out) {
    __shared__ uint4 stage[kLdsRoot ? kBtPage / 16 + 1 : 1];
    const uint8_t *root_page = nullptr;
    if constexpr (kLdsRoot) {
        if (bt_page_id_ok(root, np)) {
            const uint8_t *g = image + (uint64_t)root * kBtPage;
            const uintptr_t base = (uintptr_t)g & ~(uintptr_t)15, end = (uintptr_t)g + kBtPage;
            for (uint32_t c = threadIdx.x; c < kBtPage / 16 + 1; c += 256)
                if (base + 16 * (uintptr_t)c < end) stage[c] = ((const uint4 *)base)[c];
            root_page = (const uint8_t *)stage + ((uintptr_t)g - base);
        }
        __syncthreads();
    }
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < kb.n; i += stride) {
        uint64_t kbeg = i * kb.stride, klen64 = kb.stride;
        if (kb.offsets) {
            kbeg = kb.offsets[i];
            const uint64_t kend = kb.offsets[i + 1];
            klen64 = kend > kbeg ? kend - kbeg : 0;
        }
        BtAnswer a{kBtError, kBtNoPage, 0, 0, 0};  // an empty key: ErrKeyEmpty
        if (klen64) {
            DevCmp cmp{kb.data + kbeg, (uint32_t)(klen64 < kBtMaxKey ? klen64 : kBtMaxKey), 0, 0};
            key_prefix(kb, cmp.key, cmp.klen, cmp.k0, cmp.k1);
            bt_walk(image, np, root, root_page, cmp, &a);
        }
        out.status[i] = a.status;
        if (out.leaf) out.leaf[i] = a.leaf;
        if (out.pos) out.pos[i] = a.pos;
        if (out.vloc) out.vloc[i] = a.vloc;
        if (out.vlen) out.vlen[i] = a.vlen;
        if (out.source) out.source[i] = a.status == kBtFound ? 1 : 0;
    }
}

inline hipError_t drained(hipStream_t s, hipError_t e) {
    (void)hipStreamSynchronize(s);
    return e;
}

}  // namespace

uint64_t bt_check_ws_bytes(uint32_t num_pages) { return kBtWsHead + 4 * (uint64_t)num_pages + ((num_pages + 15ull) & ~15ull); }

hipError_t launch_bt_check(const uint8_t *image, uint32_t np, uint32_t root, uint8_t *kind, uint8_t *level, void *ws,
                           BtStats *stats_host, hipStream_t s) {
    *stats_host = BtStats{};
    stats_host->uniform = 1;
    if (np == 0) return hipSuccess;
    u64a *counts = (u64a *)ws;
    uint32_t *changed = (uint32_t *)((uint8_t *)ws + 8 * 16), *lev = (uint32_t *)((uint8_t *)ws + kBtWsHead);
    if (!kind) kind = (uint8_t *)(lev + np);
    hipError_t e;
    if ((e = hipMemsetAsync(ws, 0, kBtWsHead, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(lev, 0xFF, 4 * (uint64_t)np, s)) != hipSuccess) return e;
    if (bt_page_id_ok(root, np) && (e = hipMemsetAsync(lev + root, 0, 4, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_bt_check, dim3(stream_grid(64ull * np)), dim3(256), 0, s, image, np, kind);
    if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
    for (uint32_t r = 0; r + 1 < kBtMaxDepth && bt_page_id_ok(root, np); ++r) {
        uint32_t moved = 0;
        hipLaunchKernelGGL(k_bt_level, dim3(stream_grid(64ull * np)), dim3(256), 0, s, image, np, (const uint8_t *)kind, lev, r, changed + r);
        if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
        if ((e = hipMemcpyAsync(&moved, changed + r, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        if (!moved) break;
    }
    hipLaunchKernelGGL(k_bt_stats, dim3(stream_grid(np)), dim3(256), 0, s, image, np, (const uint8_t *)kind, (const uint32_t *)lev, level,
                       counts);
    if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
    uint64_t h[bWords];
    if ((e = hipMemcpyAsync(h, counts, sizeof h, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    *stats_host = BtStats{h[bLeaves], h[bInternals], h[bBad], h[bReachLeaves], h[bReachInternals], h[bReachBad], h[bKeys],
                          (uint32_t)h[bDepth], (uint32_t)(h[bReachLeaves] == 0 || h[bLeafHi1] - 1 == 256 - h[bLeafLoInv])};
    return hipSuccess;
}

hipError_t launch_bt_get(const uint8_t *image, uint32_t np, uint32_t root, const KeyBatch &kb, uint8_t *status, uint32_t *leaf,
                         uint32_t *pos, uint64_t *vloc, uint32_t *vlen, uint8_t *source, hipStream_t s) {
    if (kb.n == 0) return hipSuccess;
    const BtOut out{status, leaf, pos, vloc, vlen, source};
    hipLaunchKernelGGL(k_bt_get<SEB_BT_LDS_ROOT != 0>, dim3(stream_grid(kb.n)), dim3(256), 0, s, image, np, root, kb, out);
    return hipGetLastError();
}

}  // namespace seb
