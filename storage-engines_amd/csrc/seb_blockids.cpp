// seb_blockids.cpp — the host half of the block-id step: between the locate, which leaves a
// (slot, block offset) per cell, and the block search, which wants an id of the block pool per cell.  A cell of
// a file whose data section is resident in the pool is mapped by arithmetic; the other cells' distinct
// (slot, offset) pairs are numbered in order of first appearance, which is the caller's read list.  It is the
// reference for the kernels of seb_blockids.hip.  No HIP dependency, so it compiles alone
// (tools/sanitize/blockids_check.cpp); the C ABI wrappers that set seb_last_error are in seb_sstable.cpp.
#include "seb_blockids.h"

#include <cstddef>
#include <new>
#include <unordered_map>
#include <vector>

namespace seb {

namespace {

struct MixHash {
    size_t operator()(uint64_t x) const {
        x ^= x >> 30;
        x *= 0xBF58476D1CE4E5B9ull;
        x ^= x >> 27;
        x *= 0x94D049BB133111EBull;
        return (size_t)(x ^ x >> 31);
    }
};

}  // namespace

int block_ids(const uint16_t *cand, const uint64_t *blocks, uint64_t cells, const uint32_t *res_first,
              const uint32_t *res_count, uint32_t res_slots, uint32_t id_base, uint32_t *bid, uint16_t *uniq_slot,
              uint64_t *uniq_block, uint64_t uniq_cap, BlockIdSizes *sz) {
    if (!sz) return -1;
    *sz = BlockIdSizes{cells, 0, 0, 0, 0, 0};
    if (cells >= (1ull << 32)) return -2;
    if ((cells && (!cand || !blocks)) || (res_slots && (!res_first || !res_count))) return -1;
    try {
        std::unordered_map<uint64_t, uint32_t, MixHash> rank;
        std::vector<uint64_t> order;  // the distinct miss pairs by first appearance
        for (uint64_t c = 0; c < cells; ++c) {
            uint32_t id = 0;
            uint64_t pair = 0;
            switch (bid_classify(cand[c], blocks[c], res_first, res_count, res_slots, &id, &pair)) {
            case kBidNone:
                break;
            case kBidBad:
                ++sz->bad;
                break;
            case kBidResident:
                ++sz->resident;
                break;
            case kBidMiss:
                ++sz->misses;
                if (rank.emplace(pair, (uint32_t)order.size()).second) order.push_back(pair);
                break;
            }
        }
        const uint64_t uniq = sz->uniq = order.size();
        if (!bid && !uniq_slot && !uniq_block) return 0;  // the sizes alone
        if (uniq_cap < uniq) return -4;
        if ((uint64_t)id_base + uniq > kBidNoId) return -5;
        if ((cells && !bid) || (uniq && (!uniq_slot || !uniq_block))) return -1;
        for (uint64_t c = 0; c < cells; ++c) {
            uint32_t id = kBidNoId;
            uint64_t pair = 0;
            if (bid_classify(cand[c], blocks[c], res_first, res_count, res_slots, &id, &pair) == kBidMiss)
                id = id_base + rank.find(pair)->second;
            bid[c] = id;
        }
        for (uint64_t r = 0; r < uniq; ++r) {
            uniq_slot[r] = (uint16_t)(order[r] >> 48);
            uniq_block[r] = order[r] & ((1ull << 48) - 1);
        }
        return 0;
    } catch (const std::bad_alloc &) {
        return -3;
    }
}

}  // namespace seb
