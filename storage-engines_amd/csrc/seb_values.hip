// seb_values.hip — the Get path's last step on the device: the found keys' values, which the
// join left as (source, run, vloc, vlen), gathered back to back into one buffer with an offset array.  The host
// half and the semantics are in seb_values.cpp.
//
//   k_gv_sums      a workgroup per tile of kValTile keys: each key classified (not carrying / valid / invalid), the
//                  tile's count of carrying keys and their value bytes (one wave-level sum and one LDS add per
//                  wave), the lowest invalid key by atomicMin into the header
//   k_gv_scan      exclusive scan of the two arrays of tile sums (seb_scan.h), the totals into the header
//   k_gv_offsets   a workgroup per tile, four consecutive keys per lane: the keys classified again, out_off by a
//                  scan in the workgroup on top of the tile's base, and each key's checked source address and
//                  length into the workspace (13 bytes per key), so the copy reads no input array
//   k_gv_copy      balanced by output bytes: a lane per 16 aligned bytes of out_vals, a workgroup per 4 KiB.  Two
//                  waves find the first and the last key of the workgroup's span by a 64-way search over out_off
//                  (4 rounds at 10M keys); where the span holds at most kValStage keys their offsets are staged
//                  in LDS and each lane's bisection runs there.  A chunk inside one value whose covering aligned
//                  source words lie inside the source array is two 16-byte loads, a shift and one 16-byte store;
//                  a whole chunk that spans values fetches each value's piece the same way, cuts it to its bytes
//                  and shifts it into place, one 16-byte store; the output's first and last chunk go byte by byte
//
// Workspace: [magic][n][tiles][found][val_bytes][lowest invalid key] in a 128-byte header, the tiles' two sums,
// then src[n] (u64), len[n] (u32) and pad[n] (u8: how many bytes of the value's source array, up to 15 each way, lie
// in front of it and behind it, which is what an aligned 16-byte load may touch).  The emit stores nothing unless
// the header is the plan's that returned its `sizes`.  Every source address is re-derived from the inputs and
// checked against its source array by k_gv_offsets; the copy reads [src[i] - pad, src[i] + len[i] + pad) alone, all
// inside that array, and stores to out_vals[0, val_bytes) alone, so inputs that changed since the plan give wrong
// output, never an access outside those.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "seb_kernels.h"
#include "seb_scan.h"

namespace seb {

namespace {

typedef const __attribute__((address_space(1))) uint8_t *gbytes;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) u32x4 *gquads;

constexpr uint32_t VT = kValTile;
constexpr uint32_t kValStage = 1024;                        // offsets of a copy workgroup's span staged in LDS
constexpr uint64_t kValuesMagic = 0x5345554C41565447ull;  // "GTVALUES"
enum : uint32_t { hMagic = 0, hTotal = 1, hTiles = 2, hFound = 3, hBytes = 4, hBad = 5 };  // the header's u64 words
constexpr uint64_t kHeadBytes = 128;

inline __host__ __device__ uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Key i: 0 it carries no value, 1 a valid value of *len bytes at address *addr, 2 an invalid carrying key.  *pad =
// min(15, the source array's bytes in front of the value) | min(15, those behind it) << 4.  The source table is in
// kernel arguments, so the run is picked by selects, not by an indexed read.
__device__ __forceinline__ uint32_t classify(const ValuesArg &a, uint64_t i, uint32_t *len, uint64_t *addr, uint32_t *pad) {
    *len = 0, *addr = 0, *pad = 0;
    if (((gbytes)a.status)[i] != kGetFound) return 0;
    const uint32_t src = ((gbytes)a.source)[i];
    uint64_t base, bytes;
    if (src == 0) {
        const uint32_t r = a.run ? ((gbytes)a.run)[i] : 0;
        if (r >= a.num_runs) return 2;
        base = 0, bytes = 0;
#pragma unroll
        for (uint32_t q = 0; q < kMemRuns; ++q)
            if (r == q) base = (uint64_t)a.vals[q], bytes = a.val_bytes[q];
        if (!base && bytes) return 2;
    } else if (src == 1) {
        base = (uint64_t)a.pool, bytes = a.pool_bytes;
    } else {
        return 2;
    }
    const uint64_t vloc = a.vloc[i];
    const uint32_t vlen = a.vlen[i];
    if (vloc > bytes || vlen > bytes - vloc) return 2;
    const uint64_t behind = bytes - vloc - vlen;
    *len = vlen, *addr = base + vloc;
    *pad = (uint32_t)(vloc < 15 ? vloc : 15) | (uint32_t)(behind < 15 ? behind : 15) << 4;
    return 1;
}

__global__ __launch_bounds__(256) void k_gv_sums(ValuesArg a, uint64_t *__restrict__ sums, uint64_t tiles,
                                                 uint64_t *__restrict__ hdr) {
    __shared__ unsigned long long acc[2];
    const uint32_t tid = threadIdx.x;
    if (tid < 2) acc[tid] = 0;
    __syncthreads();
    const uint64_t ts = (uint64_t)blockIdx.x * VT;
    unsigned long long cnt = 0, bytes = 0, bad = ~0ull;
    for (uint32_t q = 0; q < VT / 256; ++q) {
        const uint64_t i = ts + q * 256 + tid;
        if (i >= a.n) break;
        uint32_t len, pad;
        uint64_t addr;
        const uint32_t c = classify(a, i, &len, &addr, &pad);
        if (c == 1) ++cnt, bytes += len;
        if (c == 2 && i < bad) bad = i;
    }
    cnt = wave_sum(cnt), bytes = wave_sum(bytes);
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(bad, d, 64);
        bad = o < bad ? o : bad;
    }
    if ((tid & 63) == 0) {
        atomicAdd(&acc[0], cnt), atomicAdd(&acc[1], bytes);
        if (bad != ~0ull) atomicMin((unsigned long long *)&hdr[hBad], bad);
    }
    __syncthreads();
    if (tid == 0) {
        sums[blockIdx.x] = acc[0];
        sums[tiles + blockIdx.x] = acc[1];
        if (blockIdx.x == 0) hdr[hMagic] = kValuesMagic, hdr[hTotal] = a.n, hdr[hTiles] = tiles;
    }
}

__global__ __launch_bounds__(kScanWidth) void k_gv_scan(uint64_t *x, uint64_t count, uint64_t *total) {
    scan_tile_sums(x + (uint64_t)blockIdx.x * count, count, total + blockIdx.x);
}

struct ValuesSz {  // seb_values_sizes
    uint64_t n, found, val_bytes, reserved;
};

__device__ __forceinline__ bool plan_matches(const uint64_t *ws, const ValuesSz &sz, uint64_t n) {
    return ws[hMagic] == kValuesMagic && ws[hTotal] == sz.n && ws[hTiles] == (sz.n + VT - 1) / VT && ws[hFound] == sz.found &&
           ws[hBytes] == sz.val_bytes && ws[hBad] == ~0ull && n == sz.n;
}

__global__ __launch_bounds__(256) void k_gv_offsets(ValuesArg a, const uint64_t *__restrict__ ws, ValuesSz sz,
                                                    uint64_t *__restrict__ out_off, uint64_t *__restrict__ wsrc,
                                                    uint32_t *__restrict__ wlen, uint8_t *__restrict__ wpad) {
    __shared__ uint64_t wbytes[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint64_t n = sz.n, tiles = (n + VT - 1) / VT;
    if (!plan_matches(ws, sz, a.n)) return;  // not the plan that returned these sizes
    const uint64_t base = ws[kHeadBytes / 8 + tiles + blockIdx.x];
    const uint64_t first = (uint64_t)blockIdx.x * VT + 4 * tid;
    uint32_t len[4], pad[4];
    uint64_t src[4];
    uint64_t ks = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {  // a key that is invalid by now carries nothing
        const uint64_t i = first + q;
        len[q] = 0, src[q] = 0, pad[q] = 0;
        if (i < n) classify(a, i, &len[q], &src[q], &pad[q]);
        ks += len[q];
    }
    unsigned long long ik = ks;  // inclusive scan inside the wave, then the four waves' totals through LDS
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const unsigned long long tk = __shfl_up(ik, d, 64);
        if (lane >= d) ik += tk;
    }
    if (lane == 63) wbytes[w] = ik;
    __syncthreads();
    uint64_t at = base + ik - ks;
#pragma unroll
    for (uint32_t v = 0; v < 4; ++v)
        if (v < w) at += wbytes[v];
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint64_t i = first + q;
        if (i < n) {
            out_off[i] = at < sz.val_bytes ? at : sz.val_bytes;
            wsrc[i] = src[q];
            wlen[i] = len[q];
            wpad[i] = (uint8_t)pad[q];
        }
        at += len[q];
    }
    if (blockIdx.x == 0 && tid == 0) out_off[n] = sz.val_bytes;
}

// The 16 bytes at address s, when the aligned 16-byte words that cover them lie inside [lo, hi): two loads
// and a shift.  false: nothing was read.  (seb_getpath.hip's load16.)
__device__ __forceinline__ bool load16(uint64_t s, uint64_t lo, uint64_t hi, uint64_t &w0, uint64_t &w1) {
    const uint64_t s0 = s & ~15ull;
    uint32_t sh = (uint32_t)(s - s0);
    if (s0 < lo || s0 + (sh ? 32 : 16) > hi) return false;
    const u32x4 u = *(gquads)s0;
    w0 = (uint64_t)u.x | (uint64_t)u.y << 32, w1 = (uint64_t)u.z | (uint64_t)u.w << 32;
    if (sh) {
        const u32x4 v = *(gquads)(s0 + 16);
        uint64_t w2 = (uint64_t)v.x | (uint64_t)v.y << 32, w3 = (uint64_t)v.z | (uint64_t)v.w << 32;
        if (sh >= 8) w0 = w1, w1 = w2, w2 = w3, sh -= 8;
        if (sh) {
            const uint32_t bits = 8 * sh;
            w0 = w0 >> bits | w1 << (64 - bits);
            w1 = w1 >> bits | w2 << (64 - bits);
        }
    }
    return true;
}

// The last i in [lo, hi] with off[i] <= pos, given off[lo] <= pos, by every lane of one wave: each round the 64
// lanes probe 64 evenly spaced keys, so the range shrinks 64-fold.  Offsets that do not increase still end on
// an index inside [lo, hi].
__device__ __forceinline__ uint64_t wave_find(const uint64_t *__restrict__ off, uint64_t lo, uint64_t hi, uint64_t pos,
                                              uint32_t lane) {
    while (hi > lo) {
        const uint64_t step = (hi - lo + 63) >> 6;
        const uint64_t p = lo + 1 + lane * step;
        const bool ok = p <= hi && off[p] <= pos;
        const uint64_t mask = __ballot(ok);
        const uint32_t k = mask == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~mask);  // the lanes up to the first that fails
        if (k == 0) return lo;
        lo = lo + 1 + (k - 1) * step;
        hi = lo + step - 1 < hi ? lo + step - 1 : hi;
    }
    return lo;
}

// The last i in [lo, hi] with q[i - qb] <= pos, given q[lo - qb] <= pos: one lane's bisection.
__device__ __forceinline__ uint64_t bisect(const uint64_t *q, uint64_t qb, uint64_t lo, uint64_t hi, uint64_t pos) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo + 1) >> 1);
        if (q[mid - qb] <= pos) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// An aligned 16-byte load is made only inside [src - pad's low nibble, src + len + pad's high nibble), which
// k_gv_offsets derived from the value's own source array.
__global__ __launch_bounds__(256) void k_gv_copy(const uint64_t *__restrict__ ws, ValuesSz sz, uint64_t n,
                                                 const uint64_t *__restrict__ out_off, const uint64_t *__restrict__ wsrc,
                                                 const uint32_t *__restrict__ wlen, const uint8_t *__restrict__ wpad,
                                                 uint8_t *__restrict__ out_vals) {
    __shared__ uint64_t stage[kValStage];
    __shared__ uint64_t span[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (!plan_matches(ws, sz, n)) return;
    const uint64_t total = sz.val_bytes;
    const uint64_t a = (uint64_t)out_vals, a0 = a & ~15ull;
    const uint64_t lead = a - a0, chunks = (lead + total + 15) >> 4, groups = (chunks + 255) >> 8;
    for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        // the workgroup's span of output bytes [glo, ghi) and the keys that hold its first and its last byte
        const uint64_t glo = (g << 12) > lead ? (g << 12) - lead : 0;
        const uint64_t gend = ((g + 1) << 12) - lead, ghi = gend < total ? gend : total;
        if (w < 2) {
            const uint64_t k = wave_find(out_off, 0, n - 1, w == 0 ? glo : ghi - 1, lane);
            if (lane == 0) span[w] = k;
        }
        __syncthreads();
        const uint64_t kf = span[0], kl = span[1] < span[0] ? span[0] : span[1];
        const bool staged = kl - kf < kValStage;
        if (staged)
            for (uint64_t j = tid; j <= kl - kf; j += 256) stage[j] = out_off[kf + j];
        __syncthreads();
        const uint64_t *q = staged ? stage : out_off;
        const uint64_t qb = staged ? kf : 0;
        const uint64_t c = (g << 8) + tid;
        if (c < chunks) {
            const bool head = (c << 4) < lead;
            const uint64_t lo = head ? 0 : (c << 4) - lead;
            const uint64_t end16 = (c << 4) + 16 - lead, hi = end16 < total ? end16 : total;
            uint64_t i = bisect(q, qb, kf, kl, lo);
            uint64_t beg = q[i - qb], s = wsrc[i], len = wlen[i];
            uint32_t pad = wpad[i];
            uint64_t w0, w1;
            if (!head && end16 <= total && lo >= beg && lo - beg + 16 <= len && load16(s + (lo - beg), s - (pad & 15), s + len + (pad >> 4), w0, w1)) {
                *(u32x4 *)(a0 + (c << 4)) = u32x4{(uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32)};
            } else if (!head && end16 <= total) {
                // a whole chunk that spans values (or lies at its source's edge): each value's piece is fetched
                // like a chunk, cut to its bytes and shifted into place; one 16-byte store
                w0 = w1 = 0;
                for (uint64_t j = lo; j < end16;) {
                    if (j < beg || j - beg >= len) {  // past key i's value: the key that holds byte j
                        i = bisect(q, qb, i, kl, j);
                        beg = q[i - qb], s = wsrc[i], len = wlen[i], pad = wpad[i];
                        if (j < beg || j - beg >= len) {  // offsets that are not the plan's: the byte stays 0
                            ++j;
                            continue;
                        }
                    }
                    const uint64_t piece_end = beg + len < end16 ? beg + len : end16;
                    const uint32_t cnt = (uint32_t)(piece_end - j), at = (uint32_t)(j - lo);  // 1..16 bytes at byte `at`
                    const uint64_t p = s + (j - beg);
                    uint64_t v0, v1;
                    if (!load16(p, s - (pad & 15), s + len + (pad >> 4), v0, v1)) {
                        v0 = v1 = 0;
                        for (uint32_t k = 0; k < cnt; ++k) {
                            const uint64_t byte = ((gbytes)p)[k];
                            if (k < 8) v0 |= byte << (8 * k); else v1 |= byte << (8 * (k - 8));
                        }
                    }
                    if (cnt < 8) v1 = 0, v0 &= (1ull << (8 * cnt)) - 1;
                    else if (cnt == 8) v1 = 0;
                    else if (cnt < 16) v1 &= (1ull << (8 * (cnt - 8))) - 1;
                    if (at >= 8) v1 = v0 << (8 * (at - 8)), v0 = 0;
                    else if (at) v1 = v1 << (8 * at) | v0 >> (64 - 8 * at), v0 <<= 8 * at;
                    w0 |= v0, w1 |= v1;
                    j = piece_end;
                }
                *(u32x4 *)(a0 + (c << 4)) = u32x4{(uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32)};
            } else {
                for (uint64_t j = lo; j < hi; ++j) {
                    if (j < beg || j - beg >= len) {  // past key i's value: the key that holds byte j
                        i = bisect(q, qb, i, kl, j);
                        beg = q[i - qb], s = wsrc[i], len = wlen[i];
                        if (j < beg || j - beg >= len) continue;  // offsets that are not the plan's: nothing to copy
                    }
                    out_vals[j] = ((gbytes)s)[j - beg];
                }
            }
        }
        __syncthreads();  // the next round restages
    }
}

hipError_t drained(hipStream_t s, hipError_t e) {
    (void)hipStreamSynchronize(s);
    return e;
}

struct WsLayout {
    uint64_t tiles, sums, src, len, pad, bytes;
};
WsLayout ws_layout(uint64_t n) {
    WsLayout l;
    l.tiles = (n + VT - 1) / VT;
    l.sums = kHeadBytes;
    l.src = l.sums + up16(8 * 2 * l.tiles);
    l.len = l.src + up16(8 * n);
    l.pad = l.len + up16(4 * n);
    l.bytes = l.pad + up16(n);
    return l;
}

}  // namespace

uint64_t values_ws_bytes(uint64_t n) { return ws_layout(n).bytes; }

hipError_t launch_values_plan(const ValuesArg &a, void *ws, void *sizes_host, uint64_t *bad_host, hipStream_t s) {
    const WsLayout l = ws_layout(a.n);
    uint64_t *hdr = (uint64_t *)ws, *sums = (uint64_t *)((uint8_t *)ws + l.sums);
    hipError_t e;
    if ((e = hipMemsetAsync(hdr, 0xFF, kHeadBytes, s)) != hipSuccess) return drained(s, e);  // hBad = none
    hipLaunchKernelGGL(k_gv_sums, dim3((unsigned)l.tiles), dim3(256), 0, s, a, sums, l.tiles, hdr);
    hipLaunchKernelGGL(k_gv_scan, dim3(2), dim3(kScanWidth), 0, s, sums, l.tiles, hdr + hFound);
    if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
    uint64_t h[8];
    if ((e = hipMemcpyAsync(h, hdr, sizeof h, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    *bad_host = h[hBad];
    const bool ok = h[hBad] == ~0ull;
    const uint64_t out[4] = {a.n, ok ? h[hFound] : 0, ok ? h[hBytes] : 0, 0};
    memcpy(sizes_host, out, sizeof out);
    return hipSuccess;
}

hipError_t launch_values_emit(const ValuesArg &a, const void *sizes, void *ws, uint64_t *out_off, uint8_t *out_vals,
                              hipStream_t s) {
    ValuesSz sz;
    memcpy(&sz, sizes, sizeof sz);
    const WsLayout l = ws_layout(sz.n);
    const uint64_t *hdr = (const uint64_t *)ws;
    uint64_t *wsrc = (uint64_t *)((uint8_t *)ws + l.src);
    uint32_t *wlen = (uint32_t *)((uint8_t *)ws + l.len);
    uint8_t *wpad = (uint8_t *)ws + l.pad;
    hipLaunchKernelGGL(k_gv_offsets, dim3((unsigned)l.tiles), dim3(256), 0, s, a, hdr, sz, out_off, wsrc, wlen, wpad);
    if (sz.val_bytes) {
        const uint64_t groups = ((((uint64_t)out_vals & 15) + sz.val_bytes + 15) / 16 + 255) / 256;
        hipLaunchKernelGGL(k_gv_copy, dim3(stream_grid(256 * groups, kValCopyGrid)), dim3(256), 0, s, hdr, sz, sz.n, out_off, wsrc, wlen, wpad, out_vals);
    }
    return hipGetLastError();
}

}  // namespace seb
