// seb_memget.hip — batched memtable lookup: LSM.Get's first two steps (lsm/lsm.go:144-166) for a key batch.
//
// Before it looks at any SSTable, LSM.Get asks the active memtable and then the immutable one
// (MemTable.Get, lsm/memtable.go:95-112):
//   idx := sort.Search(len(m.entries), func(i) { return m.entries[i].Key >= key })
//   idx < len && m.entries[idx].Key == key -> the entry decides: its value, or "deleted"
// Whichever memtable holds the key ends the Get; a tombstone there ends it with "not found".  A memtable is a
// sorted run in the builder's input layout (keys / key_off / vals / val_off / deleted / seq), as the WAL replay
// and the compaction merge emit it.
//
//   k_run_prefix   one lane per entry: its offsets are checked and its key's zero-padded big-endian 16-byte
//                  prefix goes into the run's index (key_prefix's two words)
//   k_run_order    one lane per entry: it must be greater than its predecessor; prefix words first, key bytes
//                  (cmp_key) only on a 16-byte tie.  Both kernels reduce the least offender into the index's
//                  header word (entry << 2 | kind), as k_merge_check does
//   k_runs_search  one lane per key, keys in batch order: per run, while the key is undecided, a lower-bound
//                  bisection over the prefix array (16-B global loads), key bytes only where prefixes tie
//   k_get_join     LSM.Get's decision over the memtables' status and the SSTables'
//
// Index: [err u64, all ones = none][pad u64][n x (p0 u64, p1 u64)]; 0 bytes for n == 0.  The search reads only
// the prefixes, at indexes below n, and the run's arrays at entries below n with key offsets clamped to
// key_bytes, so an index that does not belong to its run gives wrong answers and never an out-of-bounds read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seb_kernels.h"
#include "seb_keycmp.h"

namespace seb {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint64_t kRunIndexHead = 16;  // the header in front of the prefixes
enum : uint32_t { kBadKeyOff = 0, kBadValOff = 1, kBadOrder = 2 };

uint64_t run_index_bytes(uint64_t n) { return n ? kRunIndexHead + 16 * n : 0; }

__global__ __launch_bounds__(256) void k_run_prefix(const uint8_t *__restrict__ bytes, uint64_t key_bytes,
                                                    const uint64_t *__restrict__ koff, const uint64_t *__restrict__ voff,
                                                    uint32_t n, uint64_t *__restrict__ hdr, u32x4 *__restrict__ pre) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const uint64_t k0 = koff[e], k1 = koff[e + 1], v0 = voff[e], v1 = voff[e + 1];
    const bool key_ok = k0 <= k1 && k1 <= key_bytes && k1 - k0 < (1ull << 32);
    const bool val_ok = v0 <= v1 && v1 - v0 < (1ull << 32);
    uint64_t p0 = 0, p1 = 0;
    if (key_ok) {  // the key may sit at any byte address: byte loads
        const uint32_t len = (uint32_t)(k1 - k0);
        p0 = be64(bytes + k0, len);
        p1 = len > 8 ? be64(bytes + k0 + 8, len - 8) : 0ull;
    }
    pre[e] = u32x4{(uint32_t)p0, (uint32_t)(p0 >> 32), (uint32_t)p1, (uint32_t)(p1 >> 32)};
    if (!key_ok || !val_ok)
        atomicMin((unsigned long long *)hdr, (unsigned long long)e << 2 | (key_ok ? kBadValOff : kBadKeyOff));
}

__global__ __launch_bounds__(256) void k_run_order(const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ koff,
                                                   uint32_t n, uint64_t *__restrict__ hdr, const u32x4 *__restrict__ pre) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x + 1;
    if (e >= n) return;
    // an entry at or before e with bad offsets: neither e - 1's bytes nor e's may be read, and e is not the least
    if ((*(volatile uint64_t *)hdr >> 2) <= e) return;
    const u32x4 a = pre[e - 1], b = pre[e];
    const uint64_t a0 = (uint64_t)a.x | ((uint64_t)a.y << 32), a1 = (uint64_t)a.z | ((uint64_t)a.w << 32);
    const uint64_t be[2] = {(uint64_t)b.x | ((uint64_t)b.y << 32), (uint64_t)b.z | ((uint64_t)b.w << 32)};
    bool less;
    if (a0 != be[0]) {
        less = a0 < be[0];
    } else if (a1 != be[1]) {
        less = a1 < be[1];
    } else {  // equal 16-byte prefixes: lengths, and past 16 bytes the tails, decide
        const uint64_t o0 = koff[e - 1], o1 = koff[e], o2 = koff[e + 1];
        less = cmp_key(bytes + o0, (uint32_t)(o1 - o0), a0, a1, be, bytes + o1, (uint32_t)(o2 - o1)) < 0;
    }
    if (!less) atomicMin((unsigned long long *)hdr, (unsigned long long)e << 2 | kBadOrder);
}

// n >= 1.  Synchronises the stream; *err_host = entry << 2 | kind of the least offender, all ones for none.
hipError_t launch_run_index(const uint8_t *bytes, uint64_t key_bytes, const uint64_t *koff, const uint64_t *voff,
                            uint32_t n, void *index, uint64_t *err_host, hipStream_t s) {
    uint64_t *hdr = (uint64_t *)index;
    u32x4 *pre = (u32x4 *)((uint8_t *)index + kRunIndexHead);
    hipError_t e;
    if ((e = hipMemsetAsync(hdr, 0xFF, kRunIndexHead, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_run_prefix, dim3((n + 255) / 256), dim3(256), 0, s, bytes, key_bytes, koff, voff, n, hdr, pre);
    if (n > 1) hipLaunchKernelGGL(k_run_order, dim3((n - 1 + 255) / 256), dim3(256), 0, s, bytes, koff, n, hdr, pre);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(err_host, hdr, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) {
        (void)hipStreamSynchronize(s);  // err_host dies with the caller's frame
        return e;
    }
    return hipStreamSynchronize(s);
}

const uint64_t *run_index_prefixes(const void *index) { return (const uint64_t *)((const uint8_t *)index + kRunIndexHead); }

// key (k0, k1 = its prefix words) against entry e of run t, whose prefix is p: < 0, 0, > 0 in Go string order
__device__ __forceinline__ int cmp_entry(const MemRun &t, uint32_t e, const u32x4 p, const uint8_t *key, uint32_t klen,
                                         uint64_t k0, uint64_t k1) {
    const uint64_t be[2] = {(uint64_t)p.x | ((uint64_t)p.y << 32), (uint64_t)p.z | ((uint64_t)p.w << 32)};
    if (k0 != be[0]) return k0 < be[0] ? -1 : 1;
    if (k1 != be[1]) return k1 < be[1] ? -1 : 1;
    // equal 16-byte prefixes: lengths, and past 16 bytes the tails, decide.  The offsets are clamped to the
    // bytes seb_dev_run_index checked, so a run that changed since reads nothing outside them.
    uint64_t o0 = gload(t.koff, e), o1 = gload(t.koff, (uint64_t)e + 1);
    o0 = o0 < t.key_bytes ? o0 : t.key_bytes;
    o1 = o1 < o0 ? o0 : o1 < t.key_bytes ? o1 : t.key_bytes;
    return cmp_key(key, klen, k0, k1, be, t.bytes + o0, (uint32_t)(o1 - o0));
}

constexpr int kMemThreads = 256;

__global__ __launch_bounds__(kMemThreads) void k_runs_search(KeyBatch kb, MemRunTab tab, MemOut out) {
    const uint64_t stride = (uint64_t)gridDim.x * kMemThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kMemThreads + threadIdx.x; i < kb.n; i += stride) {
        const uint8_t *key;
        uint32_t klen;
        if (kb.offsets) {
            key = kb.data + kb.offsets[i];
            klen = (uint32_t)(kb.offsets[i + 1] - kb.offsets[i]);
        } else {
            key = kb.data + i * (uint64_t)kb.stride;
            klen = kb.stride;
        }
        uint64_t k0, k1;
        key_prefix(kb, key, klen, k0, k1);
        uint32_t st = kMemStatusNone, rr = 0xFF, ee = 0xFFFFFFFFu, vn = 0;
        uint64_t vl = 0, sq = 0;
        for (uint32_t r = 0; r < tab.nruns && st == kMemStatusNone; ++r) {
            const MemRun &t = tab.r[r];
            // sort.Search: a = the least entry >= key; eq = the probe that last lowered b found it equal, and
            // that entry is the one a ends on
            uint32_t a = 0, b = t.n;
            bool eq = false;
            while (a < b) {
                const uint32_t mid = a + ((b - a) >> 1);
                const int cmp = cmp_entry(t, mid, gload((const u32x4 *)t.pre, mid), key, klen, k0, k1);
                if (cmp > 0) {
                    a = mid + 1;
                } else {
                    b = mid;
                    eq = cmp == 0;
                }
            }
            if (eq && a < t.n) {
                const bool del = t.deleted && gload(t.deleted, a) != 0;
                st = del ? kMemStatusTombstone : kMemStatusFound;
                rr = r;
                ee = a;
                if (!del) {  // Delete stores Value nil: a tombstone reports no value
                    vl = gload(t.voff, a);
                    vn = (uint32_t)(gload(t.voff, (uint64_t)a + 1) - vl);
                }
                if (t.seq) sq = gload(t.seq, a);
            }
        }
        out.status[i] = (uint8_t)st;
        if (out.run) out.run[i] = (uint8_t)rr;
        if (out.entry) out.entry[i] = ee;
        if (out.vloc) out.vloc[i] = vl;
        if (out.vlen) out.vlen[i] = vn;
        if (out.seq) out.seq[i] = sq;
    }
}

hipError_t launch_runs_search(const KeyBatch &kb, const MemRunTab &tab, const MemOut &out, hipStream_t s) {
    if (kb.n == 0) return hipSuccess;
    uint64_t g = (kb.n + kMemThreads - 1) / kMemThreads;
    if (g > options().grid_cap) g = options().grid_cap;
    hipLaunchKernelGGL(k_runs_search, dim3((unsigned)g), dim3(kMemThreads), 0, s, kb, tab, out);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_get_join(const uint8_t *mem, const uint8_t *sst, uint64_t n, uint8_t *status,
                                                  uint8_t *source) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint8_t m = mem[i];
    const uint8_t s = m == kMemStatusFound ? kGetFound : m == kMemStatusTombstone ? kGetMiss : sst[i];
    status[i] = s;  // may be sst itself: each lane reads its element before it writes it
    if (source) source[i] = m == kMemStatusNone ? 1 : 0;
}

hipError_t launch_get_join(const uint8_t *mem, const uint8_t *sst, uint64_t n, uint8_t *status, uint8_t *source,
                           hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_get_join, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, mem, sst, n, status, source);
    return hipGetLastError();
}

}  // namespace seb
