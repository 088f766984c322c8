// stage_check.cpp — the arithmetic of the context forms' staging layer (storage-engines_amd/csrc/seb_stage.h, its
// part without HIP: Carver, RunOut, run_sections / runs_upload_bytes) under AddressSanitizer +
// UndefinedBehaviorSanitizer, as a stand-alone program:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/sanitize/stage_check.cpp -o stage_check
//   stage_check
//
// Byte counts and entry counts come from {0, 1, 15, 16, 17, 4096}.  Every layout is also lived in: a heap buffer of
// exactly the layout's total is allocated, each section's bytes are filled with the section's number, and every
// section is read back, so a section past the total is a report and two sections that overlap are an error.  One
// output line per case:
//   C <bytes of 4 sections> : <their offsets> <total>
//   R <key_bytes> <val_bytes> <n> <with_seq> : <keys koff vals voff del seq> <bytes>
//   U <n> <key_bytes> <val_bytes> <deleted seq values: 0/1 each> : <runs_upload_bytes> <where the walk over the runs ends>
// U is two runs, the first of n entries and the second of 17, as runs_upload walks them.  The index's size is
// a stand-in here (the real one belongs to the kernels): 13 n + 5 bytes, 0 for no entries.
#define SEB_STAGE_NO_HIP
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../storage-engines_amd/csrc/seb_stage.h"

uint64_t seb::run_index_bytes(uint64_t n) { return n ? 13 * n + 5 : 0; }

struct Section {
    uint64_t off, bytes;
};

// a buffer of exactly `total` bytes holds every section, and no two sections share a byte
static bool live_in(const std::vector<Section> &sections, uint64_t total) {
    uint8_t *buf = (uint8_t *)malloc(total);
    for (size_t i = 0; i < sections.size(); ++i)
        if (sections[i].bytes) memset(buf + sections[i].off, (int)(i + 1), sections[i].bytes);
    bool ok = true;
    for (size_t i = 0; i < sections.size(); ++i)
        for (uint64_t b = 0; b < sections[i].bytes; ++b) ok = ok && buf[sections[i].off + b] == (uint8_t)(i + 1);
    free(buf);
    return ok;
}

int main() {
    static const uint64_t kSizes[6] = {0, 1, 15, 16, 17, 4096};
    typedef unsigned long long ull;
    uint64_t cases = 0;
    for (uint64_t a : kSizes)
        for (uint64_t b : kSizes)
            for (uint64_t c : kSizes)
                for (uint64_t d : kSizes) {
                    seb::Carver cv;
                    const uint64_t bytes[4] = {a, b, c, d};
                    std::vector<Section> s;
                    for (uint64_t x : bytes) s.push_back({cv.take(x), x});
                    if (!live_in(s, cv.bytes())) return fprintf(stderr, "C case %llu: sections overlap\n", (ull)cases), 1;
                    printf("C %llu %llu %llu %llu : %llu %llu %llu %llu %llu\n", (ull)a, (ull)b, (ull)c, (ull)d, (ull)s[0].off,
                           (ull)s[1].off, (ull)s[2].off, (ull)s[3].off, (ull)cv.bytes());
                    ++cases;
                }
    for (uint64_t kb : kSizes)
        for (uint64_t vb : kSizes)
            for (uint64_t n : kSizes)
                for (int seq = 0; seq < 2; ++seq) {
                    const seb::RunOut at(kb, vb, n, seq != 0);
                    const std::vector<Section> s = {{at.keys, kb},          {at.koff, 8 * (n + 1)}, {at.vals, vb},
                                                    {at.voff, 8 * (n + 1)}, {at.del, n},            {at.seq, seq ? 8 * n : 0}};
                    if (!live_in(s, at.bytes)) return fprintf(stderr, "R case %llu: sections overlap\n", (ull)cases), 1;
                    printf("R %llu %llu %llu %d : %llu %llu %llu %llu %llu %llu %llu\n", (ull)kb, (ull)vb, (ull)n, seq, (ull)at.keys,
                           (ull)at.koff, (ull)at.vals, (ull)at.voff, (ull)at.del, (ull)at.seq, (ull)at.bytes);
                    ++cases;
                }
    static const uint8_t some_bytes[8] = {};
    static const uint64_t some_words[1] = {};
    for (uint64_t n : kSizes)
        for (uint64_t kb : kSizes)
            for (uint64_t vb : kSizes)
                for (int flags = 0; flags < 8; ++flags) {
                    const bool del = flags & 1, seq = flags & 2, vals = flags & 4;
                    seb_run runs[2] = {};
                    const uint64_t ns[2] = {n, 17}, val_bytes[2] = {vb, 33};
                    for (int r = 0; r < 2; ++r) {
                        runs[r].n = ns[r];
                        runs[r].key_bytes = kb;
                        runs[r].keys = kb ? some_bytes : nullptr;
                        runs[r].key_off = runs[r].val_off = some_words;
                        runs[r].deleted = del ? some_bytes : nullptr;
                        runs[r].seq = seq ? some_words : nullptr;
                    }
                    const uint64_t total = seb::runs_upload_bytes(runs, vals ? val_bytes : nullptr, 2);
                    seb::Carver cv;  // as runs_upload walks: a run of no entries is skipped
                    std::vector<Section> s;
                    for (int r = 0; r < 2; ++r) {
                        if (!ns[r]) continue;
                        const uint64_t v = vals ? val_bytes[r] : 0;
                        const seb::RunSections at = seb::run_sections(cv, runs[r], v);
                        s.push_back({at.keys, kb});
                        s.push_back({at.key_off, 8 * (ns[r] + 1)});
                        s.push_back({at.val_off, 8 * (ns[r] + 1)});
                        s.push_back({at.deleted, del ? ns[r] : 0});
                        s.push_back({at.seq, seq ? 8 * ns[r] : 0});
                        s.push_back({at.vals, v});
                        s.push_back({at.index, seb::run_index_bytes(ns[r])});
                    }
                    if (!live_in(s, total)) return fprintf(stderr, "U case %llu: sections overlap\n", (ull)cases), 1;
                    printf("U %llu %llu %llu %d %d %d : %llu %llu\n", (ull)n, (ull)kb, (ull)vb, del, seq, vals, (ull)total,
                           (ull)cv.bytes());
                    ++cases;
                }
    printf("ok %llu\n", (ull)cases);
    return 0;
}
