// block_check.cpp — the host block walker (storage-engines_amd/csrc/seb_block.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/sanitize/block_check.cpp storage-engines_amd/csrc/seb_block.cpp -o block_check
//   block_check < cases.txt
//
// Each input line is "<block hex or -> <key hex or -> <expected cell, hex>".  The block and the key
// are copied into heap buffers of exactly their sizes (zero length: no buffer at all), so a read
// past `len` is a heap-buffer-overflow report.  Prints "ok <cases>" and exits 0 when every cell
// matches; 1 on a mismatch.  tests/test_block_search.py feeds it the hand-built malformed blocks.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

namespace seb {
int block_search(const uint8_t *block, uint64_t len, const uint8_t *key, uint64_t key_len, uint32_t *cell);
int blocks_dedup(const uint64_t *files, const uint64_t *blocks, uint64_t cells, uint32_t *bid, uint64_t *uniq_files,
                 uint64_t *uniq_blocks, uint64_t uniq_cap, uint64_t *num_uniq);
}  // namespace seb

static uint8_t *exact(const std::string &hex, uint64_t *len) {
    *len = hex == "-" ? 0 : hex.size() / 2;
    if (*len == 0) return nullptr;
    uint8_t *p = (uint8_t *)malloc(*len);
    for (uint64_t i = 0; i < *len; ++i) p[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
    return p;
}

int main() {
    std::string bh, kh, want;
    uint64_t cases = 0;
    while (std::cin >> bh >> kh >> want) {
        uint64_t blen, klen;
        uint8_t *b = exact(bh, &blen), *k = exact(kh, &klen);
        uint32_t cell = 0xDEADBEEF;
        const int rc = seb::block_search(b, blen, k, klen, &cell);
        const uint32_t w = (uint32_t)strtoul(want.c_str(), nullptr, 16);
        free(b);
        free(k);
        if (rc != 0 || cell != w) {
            fprintf(stderr, "case %llu: rc %d cell %08x, expected %08x\n", (unsigned long long)cases, rc, cell, w);
            return 1;
        }
        ++cases;
    }
    // the read-list builder on exact-size buffers: a retry after a capacity that is too small
    const uint64_t n = 7;
    uint64_t *files = (uint64_t *)malloc(n * 8), *blocks = (uint64_t *)malloc(n * 8);
    const uint64_t f[n] = {5, 5, 9, 5, 9, 7, 5}, o[n] = {4096, 0, 4096, 4096, UINT64_MAX, 0, 0};
    memcpy(files, f, sizeof f);
    memcpy(blocks, o, sizeof o);
    uint32_t *bid = (uint32_t *)malloc(n * 4);
    uint64_t need = 0;
    uint64_t *uf = (uint64_t *)malloc(2 * 8), *ub = (uint64_t *)malloc(2 * 8);
    if (seb::blocks_dedup(files, blocks, n, bid, uf, ub, 2, &need) != -2 || need != 4) return 1;
    free(uf);
    free(ub);
    uf = (uint64_t *)malloc(need * 8);
    ub = (uint64_t *)malloc(need * 8);
    if (seb::blocks_dedup(files, blocks, n, bid, uf, ub, need, &need) != 0 || need != 4) return 1;
    const uint32_t want_bid[n] = {0, 1, 2, 0, UINT32_MAX, 3, 1};
    if (memcmp(bid, want_bid, sizeof want_bid) || uf[2] != 9 || ub[2] != 4096 || uf[3] != 7) return 1;
    if (seb::blocks_dedup(nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, &need) != 0 || need != 0) return 1;
    free(files);
    free(blocks);
    free(bid);
    free(uf);
    free(ub);
    printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
