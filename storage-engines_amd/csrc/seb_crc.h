// seb_crc.h — CRC-32 (IEEE) on the device, shared by the kernels that checksum records: k_wal_crc
// (seb_codec.hip: WAL records) and k_seg_crc / k_hidx_get (seb_hashindex.hip: hash-index segment records; k_seg_crc's
// seal mode writes the checksums of the records that seb_hashwrite.hip frames and compacts).
// crc32.ChecksumIEEE: reflected polynomial 0xEDB88320, init ~0, final ~ (Go hash/crc32).
// Slicing-by-4 tables, generated at compile time, staged in LDS per workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace seb {

struct CrcTables {
    uint32_t t[4][256];
};
constexpr CrcTables make_crc_tables() {
    CrcTables c{};
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t v = i;
        for (int b = 0; b < 8; ++b) v = (v & 1u) ? (v >> 1) ^ 0xEDB88320u : v >> 1;
        c.t[0][i] = v;
    }
    for (uint32_t i = 0; i < 256; ++i)
        for (int k = 1; k < 4; ++k) c.t[k][i] = (c.t[k - 1][i] >> 8) ^ c.t[0][c.t[k - 1][i] & 0xffu];
    return c;
}
static __device__ const CrcTables kCrcTab = make_crc_tables();

// the tables into a workgroup's LDS; the caller's barrier follows
__device__ __forceinline__ void crc_stage_tables(uint32_t (*tab)[256]) {
    for (uint32_t j = threadIdx.x; j < 1024; j += blockDim.x) (&tab[0][0])[j] = (&kCrcTab.t[0][0])[j];
}

__device__ __forceinline__ uint32_t crc_word(uint32_t crc, uint32_t w, const uint32_t (*t)[256]) {
    const uint32_t x = crc ^ w;
    return t[3][x & 0xffu] ^ t[2][(x >> 8) & 0xffu] ^ t[1][(x >> 16) & 0xffu] ^ t[0][x >> 24];
}
__device__ __forceinline__ uint32_t crc_byte(uint32_t crc, uint32_t b, const uint32_t (*t)[256]) {
    return (crc >> 8) ^ t[0][(crc ^ b) & 0xffu];
}

// CRC state over bytes [s, e) of p (raw state in/out: caller applies the ~ at both ends).
__device__ __forceinline__ uint32_t crc_range(uint32_t crc, const uint8_t *p, uint64_t s, uint64_t e,
                                              const uint32_t (*t)[256]) {
    uint64_t a = s;
    while (a < e && (((uintptr_t)(p + a)) & 3u)) crc = crc_byte(crc, p[a++], t);  // to a dword boundary
    const uint32_t *w = (const uint32_t *)(p + a);
    uint64_t nw = (e - a) >> 2;
    for (uint64_t j = 0; j < nw; ++j) crc = crc_word(crc, w[j], t);
    for (a += nw << 2; a < e; ++a) crc = crc_byte(crc, p[a], t);
    return crc;
}

// ChecksumIEEE of the L bytes at byte p of an LDS staging area (lw: its dwords), four bytes per step through a
// funnel shift of two aligned LDS dwords.  Reads up to one dword past the last byte's.
__device__ __forceinline__ uint32_t crc_lds(const uint32_t *lw, uint32_t p, uint32_t L, const uint32_t (*tab)[256]) {
    const uint32_t sh = p & 3u;
    uint32_t wi = p >> 2, cur = lw[wi], c = ~0u;
    for (uint32_t j = 0; j + 4 <= L; j += 4) {
        const uint32_t nxt = lw[++wi];
        c = crc_word(c, __builtin_amdgcn_alignbyte(nxt, cur, sh), tab);
        cur = nxt;
    }
    const uint32_t r = L & 3u;
    if (r) {
        const uint32_t w = __builtin_amdgcn_alignbyte(lw[wi + 1], cur, sh);
        for (uint32_t j = 0; j < r; ++j) c = crc_byte(c, (w >> (8 * j)) & 0xffu, tab);
    }
    return ~c;
}

__device__ __forceinline__ uint32_t ld_u32_le(const uint8_t *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

}  // namespace seb
