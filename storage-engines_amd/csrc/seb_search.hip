// seb_search.hip — batched data-block search: the last step of SSTable.Get and LSM.Get's decision
// over a key's candidate files.
//
// After the registry has named, per cell of a MultiGet's candidate rows, the 4 KiB data block to
// read (seb_locate.hip), the reference reads the block and walks it (searchBlock,
// lsm/sstable.go:242-290):
//   numEntries := u32(block[0:4]); off := 4
//   for i < numEntries { off+9 > len -> error "block truncated"
//                        keySize, valueSize, deleted = block[off+8] == 1; off += 9
//                        off+keySize+valueSize > len -> error (Go int: 64-bit sums, nothing wraps)
//                        entryKey == key -> deleted ? not found (tombstone) : the value
//                        entryKey >  key -> not found (Go string order)
//                        off += keySize + valueSize }
//   not found
// The first entry in walk order that truncates, equals or exceeds the key decides; nothing checks
// that the block is sorted.  k_search_lane answers that for every cell: cells[c] = status << 28 |
// voff << 13 | vlen for key c / cap in pool block bid[c] (the caller read the blocks into the pool).
// Cells are visited in linear order, as in k_locate: the bid reads and cells writes are coalesced,
// and a cell that names no block (the majority: padding) stores kCellNone and leaves.
//
// k_resolve_rows is LSM.Get over the row (lsm/lsm.go:174-197): the first cell whose file answers
// "found" or fails decides.  A TOMBSTONE DOES NOT: sst.Get returns found == false for a deleted
// entry (sstable.go:273-275), so the reference goes on to the next, older file and returns a value
// it finds there; parity means this kernel does the same.
//
// k_search_lane: a lane per cell walks its block in global memory, the reference's loop as it
// stands.  A wave-cooperative form that staged each block in LDS was measured 4x slower and removed
// (tools/diag/search_wave_lds.patch).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seb_kernels.h"
#include "seb_keycmp.h"

namespace seb {

__device__ __forceinline__ uint32_t cell_pack(uint32_t status, uint32_t voff, uint32_t vlen) {
    return status << 28 | voff << 13 | vlen;
}

struct CellKey {  // a batch key as the compares need it
    const uint8_t *p;
    uint32_t len;
    uint64_t k0, k1;  // its first 16 bytes, zero padded, big-endian
};

__device__ __forceinline__ CellKey cell_key(const KeyBatch &kb, uint64_t c, uint32_t cap) {
    const uint64_t i = (c >> 32) ? c / cap : (uint64_t)((uint32_t)c / cap);
    CellKey k;
    if (kb.offsets) {
        k.p = kb.data + kb.offsets[i];
        k.len = (uint32_t)(kb.offsets[i + 1] - kb.offsets[i]);
    } else {
        k.p = kb.data + i * (uint64_t)kb.stride;
        k.len = kb.stride;
    }
    key_prefix(kb, k.p, k.len, k.k0, k.k1);
    return k;
}

typedef const __attribute__((address_space(1))) uint8_t *gbytes;

__device__ __forceinline__ uint32_t gle32(gbytes p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// searchBlock over blk[0, L), L <= kBlockBytes.  Every read is below L.
__device__ uint32_t walk_global(const uint8_t *blk, uint32_t L, const CellKey &k) {
    if (L < 4) return cell_pack(kCellMiss, 0, 0);
    gbytes g = (gbytes)blk;
    const uint32_t num = gle32(g);
    uint32_t off = 4;
    // at most (L - 4) / 9 <= 454 entries fit: a header past L ends the walk whatever num says
    for (uint32_t i = 0; i < num; ++i) {
        if (off + 9 > L) return cell_pack(kCellTrunc, 0, 0);
        const uint32_t ks = gle32(g + off), vs = gle32(g + off + 4);
        const bool deleted = g[off + 8] == 1;
        off += 9;
        if ((uint64_t)off + ks + vs > L) return cell_pack(kCellTrunc, 0, 0);
        uint64_t be[2];
        if (off + 16 <= L) {  // two 8-byte loads, the bytes past the key masked off
            uint64_t a, b;
            __builtin_memcpy(&a, g + off, 8);
            __builtin_memcpy(&b, g + off + 8, 8);
            be[0] = be64_of_le(a, ks);
            be[1] = ks > 8 ? be64_of_le(b, ks - 8) : 0ull;
        } else {  // the block's last bytes: ks <= L - off < 16 byte loads
            be[0] = be64(blk + off, ks);
            be[1] = ks > 8 ? be64(blk + off + 8, ks - 8) : 0ull;
        }
        const int cmp = cmp_key(k.p, k.len, k.k0, k.k1, be, blk + off, ks);  // key vs entryKey
        if (cmp == 0) return deleted ? cell_pack(kCellTombstone, 0, 0) : cell_pack(kCellFound, off + ks, vs);
        if (cmp < 0) return cell_pack(kCellMiss, 0, 0);
        off += ks + vs;
    }
    return cell_pack(kCellMiss, 0, 0);
}

__global__ __launch_bounds__(256) void k_search_lane(KeyBatch kb, const uint32_t *__restrict__ bid, uint32_t cap,
                                                     uint64_t cells, const uint8_t *__restrict__ pool,
                                                     const uint16_t *__restrict__ blen, uint32_t nblocks,
                                                     uint32_t *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += stride) {
        const uint32_t b = bid[c];
        uint32_t res = cell_pack(kCellNone, 0, 0);
        if (b < nblocks) {  // kNoBlockId fails this for every nblocks
            uint32_t L = blen[b];
            if (L > kBlockBytes) L = kBlockBytes;
            res = walk_global(pool + (uint64_t)b * kBlockBytes, L, cell_key(kb, c, cap));
        }
        out[c] = res;
    }
}

// ------------------------------------------------------------ LSM.Get over a row of cells ----

__global__ __launch_bounds__(256) void k_resolve_rows(const uint32_t *__restrict__ cells,
                                                      const uint32_t *__restrict__ bid, uint64_t n, uint32_t cap,
                                                      uint8_t *__restrict__ status, uint16_t *__restrict__ col,
                                                      uint64_t *__restrict__ vloc, uint32_t *__restrict__ vlen) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint8_t st = kGetMiss;
        uint16_t at = 0xFFFF;
        uint64_t loc = 0;
        uint32_t len = 0;
        for (uint32_t j = 0; j < cap; ++j) {
            const uint32_t cell = cells[i * cap + j], cs = cell >> 28;
            if (cs == kCellFound || cs == kCellTrunc) {  // a tombstone does not decide: the walk goes on
                at = (uint16_t)(j < 0xFFFF ? j : 0xFFFF);
                if (cs == kCellFound) {
                    st = kGetFound;
                    loc = (uint64_t)bid[i * cap + j] * kBlockBytes + ((cell >> 13) & 0x1FFFu);
                    len = cell & 0x1FFFu;
                } else {
                    st = kGetError;
                }
                break;
            }
        }
        status[i] = st;
        if (col) col[i] = at;
        if (vloc) vloc[i] = loc;
        if (vlen) vlen[i] = len;
    }
}

hipError_t launch_search_blocks(const KeyBatch &kb, const uint32_t *bid, uint32_t cap, const uint8_t *pool,
                                const uint16_t *blen, uint32_t nblocks, uint32_t *cells_out, hipStream_t s) {
    const uint64_t cells = kb.n * (uint64_t)cap;
    if (cells == 0) return hipSuccess;
    uint64_t g = (cells + 255) / 256;
    if (g > options().grid_cap) g = options().grid_cap;
    hipLaunchKernelGGL(k_search_lane, dim3((unsigned)g), dim3(256), 0, s, kb, bid, cap, cells, pool, blen, nblocks,
                       cells_out);
    return hipGetLastError();
}

hipError_t launch_resolve_rows(const uint32_t *cells, const uint32_t *bid, uint64_t n, uint32_t cap, uint8_t *status,
                               uint16_t *col, uint64_t *vloc, uint32_t *vlen, hipStream_t s) {
    if (n == 0) return hipSuccess;
    uint64_t g = (n + 255) / 256;
    if (g > options().grid_cap) g = options().grid_cap;
    hipLaunchKernelGGL(k_resolve_rows, dim3((unsigned)g), dim3(256), 0, s, cells, bid, n, cap, status, col, vloc, vlen);
    return hipGetLastError();
}

}  // namespace seb
