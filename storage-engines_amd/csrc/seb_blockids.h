// seb_blockids.h — the rules that turn a located cell (slot, block offset) into a block id of the pool
// (DESIGN.md 5.17), shared by the host half (seb_blockids.cpp, no HIP dependency) and the kernels
// (seb_blockids.hip), and the host half's interface.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SEB_BID_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define SEB_BID_HD inline
#endif

namespace seb {

constexpr uint64_t kBidNoBlock = UINT64_MAX;    // SEB_NO_BLOCK
constexpr uint32_t kBidNoId = UINT32_MAX;  // SEB_NO_BLOCK_ID
constexpr uint32_t kBidPad = 0xFFFF;        // the candidate rows' padding

enum BidKind : uint32_t {
    kBidNone = 0,      // rule 1: padding or no block; bid = SEB_NO_BLOCK_ID
    kBidBad = 1,       // rules 2 and 3's refusals; bid = SEB_NO_BLOCK_ID, counted in `bad`
    kBidResident = 2,  // rule 3: *id = res_first[slot] + offset / 4096
    kBidMiss = 3,      // rule 4: *pair = slot << 48 | offset, never all ones (slot <= 0xFFFE)
};

// Rules 1-3 for one cell, in their order; nothing of the residency table is read for a cell of rule 1 or 2.
SEB_BID_HD BidKind bid_classify(uint32_t slot, uint64_t off, const uint32_t *res_first, const uint32_t *res_count,
                                uint32_t res_slots, uint32_t *id, uint64_t *pair) {
    if (slot == kBidPad || off == kBidNoBlock) return kBidNone;
    if (off >> 48) return kBidBad;
    if (slot < res_slots) {
        const uint32_t first = res_first[slot];
        if (first != kBidNoId) {
            const uint64_t q = off >> 12, sum = (uint64_t)first + q;
            if ((off & 4095) || q >= res_count[slot] || sum >= kBidNoId) return kBidBad;
            *id = (uint32_t)sum;
            return kBidResident;
        }
    }
    *pair = (uint64_t)slot << 48 | off;
    return kBidMiss;
}

struct BlockIdSizes {  // seb_blockids_sizes
    uint64_t cells, resident, misses, uniq, bad, reserved;
};

// The host half: every rule, the miss pairs ranked in order of first appearance.  *sz is filled whenever the
// arguments are valid.  bid, uniq_slot and uniq_block all null: sizes only.  0; -1 a null required pointer;
// -2 cells >= 2^32; -3 out of memory; -4 uniq_cap < uniq (nothing written is meaningful); -5 id_base + uniq
// > 2^32 - 1.
int block_ids(const uint16_t *cand, const uint64_t *blocks, uint64_t cells, const uint32_t *res_first,
              const uint32_t *res_count, uint32_t res_slots, uint32_t id_base, uint32_t *bid, uint16_t *uniq_slot,
              uint64_t *uniq_block, uint64_t uniq_cap, BlockIdSizes *sz);

}  // namespace seb
