// blockids_check.cpp — the host half of the block-id step (storage-engines_amd/csrc/seb_blockids.cpp: block_ids)
// under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/sanitize/blockids_check.cpp storage-engines_amd/csrc/seb_blockids.cpp -o blockids_check
//   blockids_check < cases.txt
//
// Each input line is one case, fields separated by blanks ("-": an empty array, "null": a null pointer), number
// lists comma separated:
//   <cand | null> <blocks | null> <cells> <res_first | null> <res_count | null> <res_slots> <id_base> <uniq_cap | plan | sizes>
// Every array is a heap buffer of exactly its bytes (bid of exactly `cells` ids, the read list of exactly uniq_cap
// entries, or for "plan" of exactly the sizes a call with null outputs returned), so one element read past an
// input, or written past an output, is a report.  "sizes": the call with null outputs alone.  Per case one line:
//   0 <cells> <resident> <misses> <uniq> <bad> <bid> <uniq_slot> <uniq_block>      ("sizes": without the arrays)
//   or, refused:  <rc> <cells> <resident> <misses> <uniq> <bad>
// A refused call must leave its outputs (filled with 0xA5 beforehand) untouched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../storage-engines_amd/csrc/seb_blockids.h"

template <typename T>
static T *nums_of(const std::string &c, uint64_t *n) {
    *n = 0;
    if (c == "null") return nullptr;
    std::vector<T> v;
    if (c != "-") {
        std::stringstream ss(c);
        std::string tok;
        while (std::getline(ss, tok, ',')) v.push_back((T)strtoull(tok.c_str(), nullptr, 10));
    }
    *n = v.size();
    T *p = (T *)malloc(sizeof(T) * v.size());
    if (!v.empty()) memcpy(p, v.data(), sizeof(T) * v.size());
    return p;
}
template <typename T>
static void csv(const T *p, uint64_t n) {
    printf(n ? " " : " -");
    for (uint64_t i = 0; i < n; ++i) printf(i ? ",%llu" : "%llu", (unsigned long long)p[i]);
}
static void sizes_out(int rc, const seb::BlockIdSizes &sz) {
    printf("%d %llu %llu %llu %llu %llu", rc, (unsigned long long)sz.cells, (unsigned long long)sz.resident,
           (unsigned long long)sz.misses, (unsigned long long)sz.uniq, (unsigned long long)sz.bad);
}
static bool untouched(const void *p, uint64_t bytes) {
    for (uint64_t i = 0; i < bytes; ++i)
        if (((const uint8_t *)p)[i] != 0xA5) return false;
    return true;
}

int main() {
    std::string line;
    uint64_t cases = 0;
    while (std::getline(std::cin, line)) {
        std::stringstream ss(line);
        std::string f[8];
        for (auto &x : f) ss >> x;
        if (f[7].empty()) {
            fprintf(stderr, "case %llu: 8 fields expected\n", (unsigned long long)cases);
            return 2;
        }
        uint64_t n_cand, n_blocks, n_first, n_count;
        uint16_t *cand = nums_of<uint16_t>(f[0], &n_cand);
        uint64_t *blocks = nums_of<uint64_t>(f[1], &n_blocks);
        const uint64_t cells = strtoull(f[2].c_str(), nullptr, 10);
        uint32_t *first = nums_of<uint32_t>(f[3], &n_first), *count = nums_of<uint32_t>(f[4], &n_count);
        const uint32_t slots = (uint32_t)strtoull(f[5].c_str(), nullptr, 10);
        const uint32_t id_base = (uint32_t)strtoull(f[6].c_str(), nullptr, 10);
        seb::BlockIdSizes sz{};
        int rc = 0;
        uint64_t cap = 0;
        if (f[7] == "plan" || f[7] == "sizes") {
            rc = seb::block_ids(cand, blocks, cells, first, count, slots, id_base, nullptr, nullptr, nullptr, 0, &sz);
            cap = sz.uniq;
        } else {
            cap = strtoull(f[7].c_str(), nullptr, 10);
        }
        if (rc != 0 || f[7] == "sizes") {
            sizes_out(rc, sz);
        } else {
            const uint64_t nb = cells < (1ull << 32) ? cells : 0;  // a refused cell count allocates nothing
            uint32_t *bid = (uint32_t *)malloc(4 * nb);
            uint16_t *us = (uint16_t *)malloc(2 * cap);
            uint64_t *ub = (uint64_t *)malloc(8 * cap);
            memset(bid, 0xA5, 4 * nb), memset(us, 0xA5, 2 * cap), memset(ub, 0xA5, 8 * cap);
            rc = seb::block_ids(cand, blocks, cells, first, count, slots, id_base, bid, us, ub, cap, &sz);
            sizes_out(rc, sz);
            if (rc == 0) {
                csv(bid, cells), csv(us, sz.uniq), csv(ub, sz.uniq);
                if (!untouched(us + sz.uniq, 2 * (cap - sz.uniq)) || !untouched(ub + sz.uniq, 8 * (cap - sz.uniq))) {
                    fprintf(stderr, "case %llu: the read list was written past uniq\n", (unsigned long long)cases);
                    return 1;
                }
            } else if (!untouched(bid, 4 * nb) || !untouched(us, 2 * cap) || !untouched(ub, 8 * cap)) {
                fprintf(stderr, "case %llu: a refused call wrote to its outputs\n", (unsigned long long)cases);
                return 1;
            }
            free(bid), free(us), free(ub);
        }
        printf("\n");
        free(cand), free(blocks), free(first), free(count);
        ++cases;
    }
    printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
