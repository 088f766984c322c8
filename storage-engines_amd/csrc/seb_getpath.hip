// seb_getpath.hip — the Get path on the device: the keys the memtables leave undecided are
// compacted into a dense batch before the SSTable steps, and the SSTables' answers for those m keys are joined
// back onto their batch rows.  The host half and the semantics are in seb_getpath.cpp.
//
//   k_gc_sums      a workgroup per tile of kGetTile keys: the tile's count of undecided keys and their key bytes
//                  (count * stride for a fixed-stride batch); one wave-level sum and one LDS add per wave
//   k_gc_scan      exclusive scan of the two arrays of tile sums (seb_scan.h), the totals into the header
//   k_gc_emit      a workgroup per tile, four consecutive keys per lane: the flags again, each undecided key's
//                  rank in the tile by a scan in the workgroup; (batch index, local offset, source address) go
//                  to LDS at that rank, then row and out_off are stored coalesced.  Key bytes: 16-byte keys
//                  with source and destination 16-byte aligned are one 16-byte load and one 16-byte store per
//                  surviving key; every other layout copies the tile's contiguous output span 16 aligned bytes
//                  at a time, a bisection over the local offsets in LDS finding each chunk's source key
//   k_gjr_base     a lane per batch key: the memtables' answer, or "no row names this key"
//   k_gjr_rows     a lane per row: the SSTables' answer to batch key row[j], where that key is undecided
//
// Workspace: [magic][n][tiles][undecided][key_bytes] in a 128-byte header, then the tiles' two sums.  The emit
// stores nothing unless the header is the plan's that returned its `sizes`, and every store is clamped to
// row[0, undecided), out_off[0, undecided] and out_keys[0, key_bytes): a status array that changed since the
// plan gives wrong output, never a store outside those.
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

constexpr uint32_t GT = kGetTile;
constexpr uint64_t kCompactMagic = 0x5443504D4F435447ull;  // "GTCOMPCT"
enum : uint32_t { hMagic = 0, hTotal = 1, hTiles = 2, hUnd = 3, hBytes = 4 };  // the header's u64 words
constexpr uint64_t kHeadBytes = 128;

__device__ __forceinline__ bool undecided(uint32_t m) { return m != kMemStatusFound && m != kMemStatusTombstone; }

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// key i's length; offsets that decrease read as an empty key
__device__ __forceinline__ uint64_t key_len(const KeyBatch &kb, uint64_t i) {
    if (!kb.offsets) return kb.stride;
    const uint64_t a = kb.offsets[i], b = kb.offsets[i + 1];
    return b > a ? b - a : 0;
}

__global__ __launch_bounds__(256) void k_gc_sums(KeyBatch kb, const uint8_t *__restrict__ mem, uint64_t *__restrict__ sums,
                                                 uint64_t tiles, uint64_t *__restrict__ hdr) {
    __shared__ unsigned long long acc[2];
    const uint32_t tid = threadIdx.x;
    if (tid < 2) acc[tid] = 0;
    __syncthreads();
    const uint64_t ts = (uint64_t)blockIdx.x * GT;
    unsigned long long cnt = 0, bytes = 0;
    for (uint32_t q = 0; q < GT / 256; ++q) {
        const uint64_t i = ts + q * 256 + tid;
        if (i >= kb.n) break;
        if (undecided(((gbytes)mem)[i])) ++cnt, bytes += key_len(kb, i);
    }
    cnt = wave_sum(cnt), bytes = wave_sum(bytes);
    if ((tid & 63) == 0) atomicAdd(&acc[0], cnt), atomicAdd(&acc[1], bytes);
    __syncthreads();
    if (tid == 0) {
        sums[blockIdx.x] = acc[0];
        sums[tiles + blockIdx.x] = acc[1];
        if (blockIdx.x == 0) hdr[hMagic] = kCompactMagic, hdr[hTotal] = kb.n, hdr[hTiles] = tiles;
    }
}

__global__ __launch_bounds__(kScanWidth) void k_gc_scan(uint64_t *x, uint64_t count, uint64_t *total) {
    scan_tile_sums(x + (uint64_t)blockIdx.x * count, count, total + blockIdx.x);
}

// The 16 bytes at address s, when the aligned 16-byte words that cover them lie inside [lo, hi): two loads
// and a shift.  false: nothing was read.  (seb_memwrite.hip's load16, through global loads.)
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

// dst[0, total) is the concatenation of the tile's cnt undecided keys: q[i] = key i's offset in it (q[cnt] =
// total), its bytes are at address sp[i] inside the batch's key bytes [lo, hi), inside which alone an aligned
// 16-byte load is made.  room = the bytes the caller's array still holds from dst.  (The fold's copy_stream with
// one source array.)
__device__ __forceinline__ void copy_span(uint8_t *__restrict__ dst, uint64_t total, uint64_t room, const uint64_t *q,
                                          const uint64_t *sp, uint32_t cnt, uint64_t lo8, uint64_t hi8) {
    if (total == 0 || cnt == 0) return;
    if (room < total) total = room;
    const uint64_t a = (uint64_t)dst, a0 = a & ~15ull;
    const uint64_t lead = a - a0, chunks = (lead + total + 15) >> 4;
    for (uint64_t c = threadIdx.x; c < chunks; c += blockDim.x) {
        const bool head = (c << 4) < lead;
        const uint64_t lo = head ? 0 : (c << 4) - lead;
        const uint64_t end16 = (c << 4) + 16 - lead, hi = end16 < total ? end16 : total;
        uint32_t i = 0, ih = cnt - 1;  // the last key with q[i] <= lo: the one that holds byte lo
        while (i < ih) {
            const uint32_t mid = (i + ih + 1) >> 1;
            if (q[mid] <= lo) i = mid; else ih = mid - 1;
        }
        uint64_t end = q[i + 1];
        uint64_t w0, w1;
        if (!head && end16 <= total && lo + 16 <= end && load16(sp[i] + (lo - q[i]), lo8, hi8, w0, w1)) {
            *(u32x4 *)(a0 + (c << 4)) = u32x4{(uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32)};
            continue;
        }
        gbytes src = (gbytes)sp[i];
        uint64_t beg = q[i];
        for (uint64_t j = lo; j < hi; ++j) {
            while (j >= end && i + 1 < cnt) {  // j < total <= q[cnt]; the guard holds i below cnt whatever q holds
                ++i;
                beg = end;
                end = q[i + 1];
                src = (gbytes)sp[i];
            }
            if (j >= end) break;
            dst[j] = src[j - beg];
        }
    }
}

struct CompactArg {  // seb_compact_sizes
    uint64_t n, undecided, key_bytes, reserved;
};

// fast: 16-byte keys, kb.data and out_keys 16-byte aligned, sz.key_bytes == 16 * sz.undecided
__global__ __launch_bounds__(256) void k_gc_emit(KeyBatch kb, const uint8_t *__restrict__ mem,
                                                 const uint64_t *__restrict__ ws, CompactArg sz,
                                                 uint8_t *__restrict__ out_keys, uint64_t *__restrict__ out_off,
                                                 uint32_t *__restrict__ row, int fast) {
    __shared__ uint64_t loff[GT + 1], lsrc[GT];
    __shared__ uint32_t lrow[GT];
    __shared__ uint32_t wcnt[4];
    __shared__ uint64_t wbytes[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint64_t n = sz.n, tiles = (n + GT - 1) / GT;
    if (ws[hMagic] != kCompactMagic || ws[hTotal] != n || ws[hTiles] != tiles || ws[hUnd] != sz.undecided ||
        ws[hBytes] != sz.key_bytes || kb.n != n)
        return;  // not the plan that returned these sizes
    const uint64_t *sums = ws + kHeadBytes / 8;
    const uint64_t obase = sums[blockIdx.x], kbase = sums[tiles + blockIdx.x];
    const uint64_t first = (uint64_t)blockIdx.x * GT + 4 * tid;
    bool und[4];
    uint64_t len[4], src[4];
    uint32_t c = 0;
    uint64_t ks = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint64_t i = first + q;
        und[q] = i < n && undecided(((gbytes)mem)[i]);
        len[q] = 0, src[q] = 0;
        if (und[q]) {
            len[q] = key_len(kb, i);
            src[q] = (uint64_t)kb.data + (kb.offsets ? kb.offsets[i] : i * (uint64_t)kb.stride);
            ++c, ks += len[q];
        }
    }
    // inclusive scan inside the wave, then the four waves' totals through LDS
    uint32_t ic = c;
    unsigned long long ik = ks;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t tc = __shfl_up(ic, d, 64);
        const unsigned long long tk = __shfl_up(ik, d, 64);
        if (lane >= d) ic += tc, ik += tk;
    }
    if (lane == 63) wcnt[w] = ic, wbytes[w] = ik;
    __syncthreads();
    uint32_t cnt = 0, ci = ic - c;
    uint64_t ktot = 0, ko = ik - ks;
#pragma unroll
    for (uint32_t v = 0; v < 4; ++v) {
        if (v < w) ci += wcnt[v], ko += wbytes[v];
        cnt += wcnt[v], ktot += wbytes[v];
    }
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        if (!und[q]) continue;
        lrow[ci] = (uint32_t)(first + q);
        loff[ci] = ko;
        lsrc[ci] = src[q];
        ++ci, ko += len[q];
    }
    if (tid == 0) loff[cnt] = ktot;
    __syncthreads();
    for (uint32_t j = tid; j < cnt; j += 256) {
        const uint64_t o = obase + j;
        if (o >= sz.undecided) continue;
        row[o] = lrow[j];
        if (out_off) {
            const uint64_t at = kbase + loff[j];
            out_off[o] = at < sz.key_bytes ? at : sz.key_bytes;
        }
        if (fast) *(u32x4 *)(out_keys + 16 * o) = ((gquads)kb.data)[lrow[j]];
    }
    if (out_off && blockIdx.x == 0 && tid == 0) out_off[sz.undecided] = sz.key_bytes;
    if (!fast && kbase < sz.key_bytes) {
        const uint64_t lo8 = (uint64_t)kb.data + (kb.offsets ? kb.offsets[0] : 0);
        const uint64_t hi8 = (uint64_t)kb.data + (kb.offsets ? kb.offsets[n] : n * (uint64_t)kb.stride);
        copy_span(out_keys + kbase, ktot, sz.key_bytes - kbase, loff, lsrc, cnt, lo8, hi8);
    }
}

struct JoinArg {
    const uint8_t *mem;
    const uint64_t *mem_vloc;
    const uint32_t *mem_vlen;
    const uint32_t *row;
    const uint8_t *sst_status;
    const uint16_t *sst_col;
    const uint64_t *sst_vloc;
    const uint32_t *sst_vlen;
    uint8_t *status, *source;
    uint16_t *col;
    uint64_t *vloc;
    uint32_t *vlen;
    uint64_t n, m;
};

__global__ __launch_bounds__(256) void k_gjr_base(JoinArg a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t ms = a.mem[i];
    const bool found = ms == kMemStatusFound;
    a.status[i] = found ? kGetFound : kGetMiss;
    if (a.source) a.source[i] = undecided(ms) ? 1 : 0;
    if (a.col) a.col[i] = 0xFFFF;
    if (a.vloc) a.vloc[i] = found && a.mem_vloc ? a.mem_vloc[i] : 0;
    if (a.vlen) a.vlen[i] = found && a.mem_vlen ? a.mem_vlen[i] : 0;
}

__global__ __launch_bounds__(256) void k_gjr_rows(JoinArg a) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.m) return;
    const uint64_t i = a.row[j];
    if (i >= a.n || !undecided(a.mem[i])) return;  // a row outside the batch or naming a decided key
    a.status[i] = a.sst_status[j];
    if (a.col) a.col[i] = a.sst_col ? a.sst_col[j] : 0xFFFF;
    if (a.vloc) a.vloc[i] = a.sst_vloc ? a.sst_vloc[j] : 0;
    if (a.vlen) a.vlen[i] = a.sst_vlen ? a.sst_vlen[j] : 0;
}

inline uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

hipError_t drained(hipStream_t s, hipError_t e) {
    (void)hipStreamSynchronize(s);
    return e;
}

}  // namespace

uint64_t compact_ws_bytes(uint64_t n) { return kHeadBytes + up16(8 * 2 * ((n + GT - 1) / GT)); }

hipError_t launch_compact_plan(const KeyBatch &kb, const uint8_t *mem, void *ws, void *sizes_host, hipStream_t s) {
    const uint64_t tiles = (kb.n + GT - 1) / GT;
    uint64_t *hdr = (uint64_t *)ws, *sums = hdr + kHeadBytes / 8;
    hipLaunchKernelGGL(k_gc_sums, dim3((unsigned)tiles), dim3(256), 0, s, kb, mem, sums, tiles, hdr);
    hipLaunchKernelGGL(k_gc_scan, dim3(2), dim3(kScanWidth), 0, s, sums, tiles, hdr + hUnd);
    hipError_t e;
    if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
    uint64_t h[8];
    if ((e = hipMemcpyAsync(h, hdr, sizeof h, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    const uint64_t out[4] = {kb.n, h[hUnd], h[hBytes], 0};
    memcpy(sizes_host, out, sizeof out);
    return hipSuccess;
}

hipError_t launch_compact_emit(const KeyBatch &kb, const uint8_t *mem, const void *sizes, const void *ws,
                               uint8_t *out_keys, uint64_t *out_off, uint32_t *row, hipStream_t s) {
    CompactArg sz;
    memcpy(&sz, sizes, sizeof sz);
    const uint64_t tiles = (sz.n + GT - 1) / GT;
    const int fast = !kb.offsets && kb.stride == 16 && (((uint64_t)kb.data | (uint64_t)out_keys) & 15) == 0 &&
                     sz.key_bytes == 16 * sz.undecided;
    hipLaunchKernelGGL(k_gc_emit, dim3((unsigned)tiles), dim3(256), 0, s, kb, mem, (const uint64_t *)ws, sz, out_keys,
                       kb.offsets ? out_off : nullptr, row, fast);
    return hipGetLastError();
}

hipError_t launch_get_join_rows(const uint8_t *mem, const uint64_t *mem_vloc, const uint32_t *mem_vlen, uint64_t n,
                                const uint32_t *row, uint64_t m, const uint8_t *sst_status, const uint16_t *sst_col,
                                const uint64_t *sst_vloc, const uint32_t *sst_vlen, uint8_t *status, uint8_t *source,
                                uint16_t *col, uint64_t *vloc, uint32_t *vlen, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const JoinArg a{mem, mem_vloc, mem_vlen, row, sst_status, sst_col, sst_vloc, sst_vlen, status, source, col, vloc, vlen, n, m};
    hipLaunchKernelGGL(k_gjr_base, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    if (m) hipLaunchKernelGGL(k_gjr_rows, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace seb
