// merge_check.cpp — the host half of the compaction merge (storage-engines_amd/csrc/seb_block.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/sanitize/merge_check.cpp storage-engines_amd/csrc/seb_block.cpp -o merge_check
//   merge_check < cases.txt
//
// Each input line is one merge: <flags> <run_begin, comma separated; "-": no runs, a null pointer> <block image in
// hex ("-" for none)>...
// The pool is a heap buffer of exactly blocks * 4096 bytes in which every slot's bytes past its image are
// poisoned, so a read past a block's length is a report; the outputs are heap buffers of exactly the plan's
// sizes.  Every case is planned, emitted, and emitted again with each size one short (which must be
// refused and write nothing past the short buffers).  Per case one output line:
//   <rc> <run> <entry> <entries_in> <entries_out> <shadowed> <dropped> <keys hex> <key offsets> <values hex>
//   <value offsets> <deleted hex>
#include <sanitizer/asan_interface.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../storage-engines_amd/csrc/seb_block.h"

static void hex(const uint8_t *p, uint64_t n) {
    if (!n) printf(" -");
    else printf(" ");
    for (uint64_t i = 0; i < n; ++i) printf("%02x", p[i]);
}
static void csv(const uint64_t *p, uint64_t n) {
    printf(" ");
    for (uint64_t i = 0; i < n; ++i) printf(i ? ",%llu" : "%llu", (unsigned long long)p[i]);
}

struct Out {
    uint8_t *keys, *vals, *del;
    uint64_t *koff, *voff;
    explicit Out(const seb::MergeSizes &s)
        : keys((uint8_t *)malloc(s.key_bytes)), vals((uint8_t *)malloc(s.val_bytes)), del((uint8_t *)malloc(s.entries_out)),
          koff((uint64_t *)malloc(8 * (s.entries_out + 1))), voff((uint64_t *)malloc(8 * (s.entries_out + 1))) {}
    ~Out() {
        free(keys), free(vals), free(del), free(koff), free(voff);
    }
    seb::MergeOut ref() const { return seb::MergeOut{keys, koff, vals, voff, del}; }
};

int main() {
    std::string line;
    uint64_t cases = 0;
    while (std::getline(std::cin, line)) {
        std::stringstream ss(line);
        uint32_t flags;
        std::string rbs, tok;
        ss >> flags >> rbs;
        std::vector<uint64_t> rb;
        std::stringstream rs(rbs);
        if (rbs != "-")  // "-": no runs and a null run_begin
            while (std::getline(rs, tok, ',')) rb.push_back(strtoull(tok.c_str(), nullptr, 10));
        std::vector<std::string> blocks;
        while (ss >> tok) blocks.push_back(tok == "-" ? "" : tok);
        const uint64_t nb = blocks.size();
        uint8_t *pool = (uint8_t *)malloc(nb * 4096 + 1);
        std::vector<uint16_t> blen(nb + 1);
        for (uint64_t b = 0; b < nb; ++b) {
            const uint64_t len = blocks[b].size() / 2;
            blen[b] = (uint16_t)len;
            for (uint64_t i = 0; i < len; ++i) pool[b * 4096 + i] = (uint8_t)strtoul(blocks[b].substr(2 * i, 2).c_str(), nullptr, 16);
            ASAN_POISON_MEMORY_REGION(pool + b * 4096 + len, 4096 - len);
        }
        const uint32_t nr = rb.empty() ? 0 : (uint32_t)rb.size() - 1;
        seb::MergeSizes sz{}, got{};
        uint32_t run = 0;
        uint64_t entry = 0;
        const uint64_t *rbp = rb.empty() ? nullptr : rb.data();
        int rc = seb::merge_walk(nb ? pool : nullptr, nb ? blen.data() : nullptr, rbp, nr, flags, nullptr, nullptr, &sz, &run, &entry);
        if (rc != 0) {
            printf("%d %u %llu\n", rc, run, (unsigned long long)entry);
        } else {
            Out o(sz);
            const seb::MergeOut ref = o.ref();
            rc = seb::merge_walk(nb ? pool : nullptr, nb ? blen.data() : nullptr, rbp, nr, flags, &ref, &sz, &got, &run, &entry);
            if (rc != 0 || memcmp(&sz, &got, sizeof sz)) return fprintf(stderr, "case %llu: emit differs from plan\n", (unsigned long long)cases), 1;
            printf("0 0 0 %llu %llu %llu %llu", (unsigned long long)sz.entries_in, (unsigned long long)sz.entries_out,
                   (unsigned long long)sz.shadowed, (unsigned long long)sz.dropped);
            hex(o.keys, sz.key_bytes), csv(o.koff, sz.entries_out + 1), hex(o.vals, sz.val_bytes);
            csv(o.voff, sz.entries_out + 1), hex(o.del, sz.entries_out);
            printf("\n");
            for (int shorten = 0; shorten < 3; ++shorten) {  // sizes one short: refused, nothing past the short buffers
                seb::MergeSizes want = sz;
                uint64_t *field = shorten == 0 ? &want.entries_out : shorten == 1 ? &want.key_bytes : &want.val_bytes;
                if (*field == 0) continue;
                --*field;
                Out small(want);
                const seb::MergeOut sref = small.ref();
                if (seb::merge_walk(nb ? pool : nullptr, nb ? blen.data() : nullptr, rbp, nr, flags, &sref, &want, &got, &run, &entry) != -5)
                    return fprintf(stderr, "case %llu: sizes one short were accepted\n", (unsigned long long)cases), 1;
            }
        }
        ASAN_UNPOISON_MEMORY_REGION(pool, nb * 4096 + 1);
        free(pool);
        ++cases;
    }
    printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
