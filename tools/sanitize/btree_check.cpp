// btree_check.cpp — the host half of the B-tree's read side (storage-engines_amd/csrc/seb_btree.cpp: bt_open,
// bt_check, bt_get, and through them the page codec and the walk of seb_btree.h, the text the kernels compile too)
// under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/sanitize/btree_check.cpp \
//       storage-engines_amd/csrc/seb_btree.cpp -o btree_check
//   btree_check < cases.txt
//
// Each input line is one case, fields separated by blanks ("-": no bytes):
//   B <image file> <K> <key 0 hex> ...
// The file is read into a heap buffer of exactly its bytes; the K keys are packed in a buffer of exactly their
// bytes; kind and level have exactly num_pages bytes and every Get output exactly K elements, so one byte read past
// the image or written past an output is a report.  Per case one output line ("invalid" where bt_open refuses):
//   <root,header_pages,free_list,num_pages> <kind,...> <level,...> <the nine stats> <status,...> <leaf,...> <pos,...>
//   <vloc,...> <vlen,...>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../storage-engines_amd/csrc/seb_btree.h"

static int nibble(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

static uint8_t *bytes_of(const std::string &h, uint64_t *n) {  // an exact-size heap copy
    *n = h == "-" ? 0 : h.size() / 2;
    uint8_t *p = (uint8_t *)malloc(*n);
    for (uint64_t i = 0; i < *n; ++i) p[i] = (uint8_t)(nibble(h[2 * i]) << 4 | nibble(h[2 * i + 1]));
    return p;
}

template <typename T>
static void list(const T *v, uint64_t n) {
    printf(n ? " " : " -");
    for (uint64_t i = 0; i < n; ++i) printf(i ? ",%llu" : "%llu", (unsigned long long)v[i]);
}

int main() {
    std::string line;
    uint64_t cases = 0;
    while (std::getline(std::cin, line)) {
        std::stringstream ss(line);
        std::string kind_of_case, path;
        uint64_t K = 0;
        ss >> kind_of_case >> path >> K;
        const unsigned long long cn = (unsigned long long)cases;
        if (kind_of_case != "B") return fprintf(stderr, "case %llu: unknown kind\n", cn), 1;
        FILE *f = fopen(path.c_str(), "rb");
        if (!f) return fprintf(stderr, "case %llu: cannot open %s\n", cn, path.c_str()), 1;
        fseek(f, 0, SEEK_END);
        const uint64_t bytes = (uint64_t)ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t *image = (uint8_t *)malloc(bytes);
        if (bytes && fread(image, 1, bytes, f) != bytes) return fprintf(stderr, "case %llu: short read\n", cn), 1;
        fclose(f);
        std::vector<uint8_t> kbytes;
        uint64_t *koff = (uint64_t *)malloc(8 * (K + 1));
        koff[0] = 0;
        for (uint64_t k = 0; k < K; ++k) {
            std::string h;
            ss >> h;
            uint64_t n = 0;
            uint8_t *b = bytes_of(h, &n);
            kbytes.insert(kbytes.end(), b, b + n);
            koff[k + 1] = kbytes.size();
            free(b);
        }
        uint8_t *kdata = (uint8_t *)malloc(kbytes.size());
        if (!kbytes.empty()) memcpy(kdata, kbytes.data(), kbytes.size());
        seb::BtMeta meta;
        const int rc = seb::bt_open(image, bytes, &meta);
        if (rc == -2) {
            printf("invalid\n");
        } else if (rc != 0) {
            return fprintf(stderr, "case %llu: bt_open failed\n", cn), 1;
        } else {
            const uint64_t np = meta.num_pages;
            uint8_t *kind = (uint8_t *)malloc(np), *level = (uint8_t *)malloc(np);
            seb::BtStats st;
            if (seb::bt_check(image, bytes, meta, kind, level, &st) != 0) return fprintf(stderr, "case %llu: bt_check failed\n", cn), 1;
            uint8_t *status = (uint8_t *)malloc(K);
            uint32_t *leaf = (uint32_t *)malloc(4 * K), *pos = (uint32_t *)malloc(4 * K), *vlen = (uint32_t *)malloc(4 * K);
            uint64_t *vloc = (uint64_t *)malloc(8 * K);
            if (seb::bt_get(image, bytes, meta, seb::BtKeys{kdata, koff, K, 0}, status, leaf, pos, vloc, vlen) != 0)
                return fprintf(stderr, "case %llu: bt_get failed\n", cn), 1;
            const uint32_t m[4] = {meta.root, meta.header_pages, meta.free_list, meta.num_pages};
            const uint64_t s[9] = {st.leaves, st.internals, st.bad, st.reach_leaves, st.reach_internals, st.reach_bad, st.keys, st.depth,
                                   st.uniform};
            list(m, 4), list(kind, np), list(level, np), list(s, 9);
            list(status, K), list(leaf, K), list(pos, K), list(vloc, K), list(vlen, K);
            printf("\n");
            free(kind), free(level), free(status), free(leaf), free(pos), free(vlen), free(vloc);
        }
        free(image), free(koff), free(kdata);
        ++cases;
    }
    printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
