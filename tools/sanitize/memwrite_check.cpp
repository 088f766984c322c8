// memwrite_check.cpp — the host half of the memtable write side (storage-engines_amd/csrc/seb_memwrite.cpp:
// frame_plan, frame_emit, run_size_delta, runs_fold) under AddressSanitizer + UndefinedBehaviorSanitizer, as a
// stand-alone program:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/sanitize/memwrite_check.cpp \
//       storage-engines_amd/csrc/seb_memwrite.cpp storage-engines_amd/csrc/seb_memtable.cpp -o memwrite_check
//   memwrite_check < cases.txt
//
// Each input line is one case, fields separated by blanks ("-": an empty array, "null": a null pointer):
//   F <first_seq> <stride> <key offsets | null> <keys hex> <val_off> <vals hex> <deleted hex | null>
//   D <num_runs> { run } x num_runs { run }             the existing runs, then the new one
//   M <num_runs> { run <vals hex> } x num_runs
// with run = <keys hex> <key_off> <val_off> <deleted hex | null> <seq | null>.  Number lists are comma separated.
// Every array is a heap buffer of exactly its bytes, so one byte read past the ops' or a run's arrays, or written
// past the image or an output array, is a report.  Per case one output line:
//   F: 0 <image hex> <rec_off>                                      or, refused:  <rc> <op>
//   D: 0 <delta>                                                    or, refused:  <rc> <run> <entry>
//   M: 0 <keys hex> <key_off> <vals hex> <val_off> <deleted hex> <seq> <the eight sizes>    or:  <rc> <run> <entry>
// A frame is also planned without rec_off, and a fold emitted without seq; both must agree with the full call.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../storage-engines_amd/csrc/seb_memwrite.h"

static int nibble(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

// exact-size heap copies; "null" and (for bytes) nothing at all give a null pointer
static uint8_t *bytes_of(const std::string &h, uint64_t *n) {
    *n = 0;
    if (h == "null" || h == "-") return nullptr;
    *n = h.size() / 2;
    uint8_t *p = (uint8_t *)malloc(*n);
    for (uint64_t i = 0; i < *n; ++i) p[i] = (uint8_t)(nibble(h[2 * i]) << 4 | nibble(h[2 * i + 1]));
    return p;
}
static uint64_t *nums_of(const std::string &c, uint64_t *n) {
    *n = 0;
    if (c == "null" || c == "-") return nullptr;
    std::vector<uint64_t> v;
    std::stringstream ss(c);
    std::string tok;
    while (std::getline(ss, tok, ',')) v.push_back(strtoull(tok.c_str(), nullptr, 10));
    *n = v.size();
    uint64_t *p = (uint64_t *)malloc(8 * v.size());
    memcpy(p, v.data(), 8 * v.size());
    return p;
}
static void hex(const uint8_t *p, uint64_t n) {
    printf(n ? " " : " -");
    for (uint64_t i = 0; i < n; ++i) printf("%02x", p[i]);
}
static void csv(const uint64_t *p, uint64_t n) {
    printf(n ? " " : " -");
    for (uint64_t i = 0; i < n; ++i) printf(i ? ",%llu" : "%llu", (unsigned long long)p[i]);
}

static seb::Run read_run(std::stringstream &ss, std::vector<void *> &held) {
    std::string a, b, c, d, e;
    ss >> a >> b >> c >> d >> e;
    uint64_t kb = 0, nk = 0, nv = 0, nd = 0, ns = 0;
    uint8_t *keys = bytes_of(a, &kb);
    uint64_t *koff = nums_of(b, &nk), *voff = nums_of(c, &nv);
    uint8_t *del = bytes_of(d, &nd);
    uint64_t *seq = nums_of(e, &ns);
    held.insert(held.end(), {(void *)keys, (void *)koff, (void *)voff, (void *)del, (void *)seq});
    return seb::Run{keys, kb, koff, voff, del, seq, nk ? nk - 1 : 0};
}

int main() {
    std::string line;
    unsigned long long cases = 0;
    while (std::getline(std::cin, line)) {
        std::stringstream ss(line);
        std::string kind, a, b, c, d, e;
        ss >> kind;
        std::vector<void *> held;
        if (kind == "F") {
            unsigned long long first_seq = 0;
            uint32_t stride = 0;
            ss >> first_seq >> stride >> a >> b >> c >> d >> e;
            uint64_t nk = 0, kb = 0, nv = 0, vb = 0, nd = 0;
            uint64_t *koff = nums_of(a, &nk);
            uint8_t *keys = bytes_of(b, &kb);
            uint64_t *voff = nums_of(c, &nv);
            uint8_t *vals = bytes_of(d, &vb), *del = bytes_of(e, &nd);
            if (!keys) keys = (uint8_t *)malloc(0);  // a batch of empty keys: a pointer to no bytes, not a null one
            if (!vals) vals = (uint8_t *)malloc(0);
            held = {koff, keys, voff, vals, del};
            const uint64_t n = nv ? nv - 1 : 0;
            const seb::KeysView kv{keys, koff, n, stride};
            uint64_t *rec_off = (uint64_t *)malloc(8 * (n + 1));
            uint64_t total = 0, total2 = 0, op = 0;
            int rc = seb::frame_plan(kv, voff, del, rec_off, &total, &op);
            if (rc == 0) {
                if (seb::frame_plan(kv, voff, del, nullptr, &total2, nullptr) != 0 || total2 != total || rec_off[n] != total)
                    return fprintf(stderr, "case %llu: the plans differ\n", cases), 1;
                uint8_t *image = (uint8_t *)malloc(total);
                rc = seb::frame_emit(kv, vals, voff, del, first_seq, image, total, &op);
                if (rc == 0) printf("0"), hex(image, total), csv(rec_off, n + 1), printf("\n");
                if (rc == 0 && seb::frame_emit(kv, vals, voff, del, first_seq, image, total + 1, &op) != -5)
                    return fprintf(stderr, "case %llu: a wrong image size was accepted\n", cases), 1;
                free(image);
            }
            if (rc != 0) printf("%d %llu\n", rc, (unsigned long long)op);
            free(rec_off);
        } else if (kind == "D") {
            uint32_t num_runs = 0;
            ss >> num_runs;
            std::vector<seb::Run> runs;
            for (uint32_t r = 0; r < num_runs; ++r) runs.push_back(read_run(ss, held));
            const seb::Run fresh = read_run(ss, held);
            int64_t *delta = (int64_t *)malloc(8);
            uint32_t bad_run = 0;
            uint64_t bad_entry = 0;
            const int rc = seb::run_size_delta(fresh, runs.data(), num_runs, delta, &bad_run, &bad_entry);
            if (rc != 0)
                printf("%d %u %llu\n", rc, bad_run, (unsigned long long)bad_entry);
            else
                printf("0 %lld\n", (long long)*delta);
            free(delta);
        } else if (kind == "M") {
            uint32_t num_runs = 0;
            ss >> num_runs;
            std::vector<seb::Run> runs;
            std::vector<const uint8_t *> vals;
            std::vector<uint64_t> val_bytes;
            for (uint32_t r = 0; r < num_runs; ++r) {
                runs.push_back(read_run(ss, held));
                ss >> a;
                uint64_t vb = 0;
                uint8_t *v = bytes_of(a, &vb);
                held.push_back(v);
                vals.push_back(v);
                val_bytes.push_back(vb);
            }
            seb::FoldSizes sz, got, got2;
            uint32_t bad_run = 0;
            uint64_t bad_entry = 0;
            int rc = seb::runs_fold(runs.data(), nullptr, val_bytes.data(), num_runs, nullptr, nullptr, &sz, &bad_run, &bad_entry);
            if (rc == 0) {
                const uint64_t n = sz.entries_out;
                uint8_t *keys = (uint8_t *)malloc(sz.key_bytes), *ov = (uint8_t *)malloc(sz.val_bytes), *del = (uint8_t *)malloc(n);
                uint64_t *koff = (uint64_t *)malloc(8 * (n + 1)), *voff = (uint64_t *)malloc(8 * (n + 1)), *seq = (uint64_t *)malloc(8 * n);
                const seb::ReplayOut out{keys, koff, ov, voff, del, seq};
                rc = seb::runs_fold(runs.data(), vals.data(), val_bytes.data(), num_runs, &out, &sz, &got, &bad_run, &bad_entry);
                if (rc != 0 || memcmp(&got, &sz, sizeof sz)) return fprintf(stderr, "case %llu: the emit differs from its plan\n", cases), 1;
                printf("0"), hex(keys, sz.key_bytes), csv(koff, n + 1), hex(ov, sz.val_bytes), csv(voff, n + 1), hex(del, n), csv(seq, n);
                csv(&sz.entries_in, 8), printf("\n");
                uint8_t *keys2 = (uint8_t *)malloc(sz.key_bytes);
                const seb::ReplayOut out2{keys2, koff, ov, voff, del, nullptr};  // without seq
                if (seb::runs_fold(runs.data(), vals.data(), val_bytes.data(), num_runs, &out2, &sz, &got2, nullptr, nullptr) != 0 ||
                    (sz.key_bytes && memcmp(keys, keys2, sz.key_bytes)))
                    return fprintf(stderr, "case %llu: the emit without seq differs\n", cases), 1;
                if (n) {  // sizes below the plan's: refused, and nothing past them is written
                    seb::FoldSizes less = sz;
                    --less.entries_out;
                    uint64_t *koff3 = (uint64_t *)malloc(8 * n), *voff3 = (uint64_t *)malloc(8 * n);
                    const seb::ReplayOut out3{keys2, koff3, ov, voff3, del, nullptr};
                    if (seb::runs_fold(runs.data(), vals.data(), val_bytes.data(), num_runs, &out3, &less, &got2, nullptr, nullptr) != -6)
                        return fprintf(stderr, "case %llu: sizes below the plan's were accepted\n", cases), 1;
                    free(koff3), free(voff3);
                }
                free(keys), free(keys2), free(ov), free(del), free(koff), free(voff), free(seq);
            } else {
                printf("%d %u %llu\n", rc, bad_run, (unsigned long long)bad_entry);
            }
        } else {
            return fprintf(stderr, "case %llu: unknown kind\n", cases), 1;
        }
        for (void *p : held) free(p);
        ++cases;
    }
    printf("ok %llu\n", cases);
    return 0;
}
