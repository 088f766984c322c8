// values_check.cpp — the host half of the Get path's last step (storage-engines_amd/csrc/seb_values.cpp:
// get_values) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/sanitize/values_check.cpp storage-engines_amd/csrc/seb_values.cpp -o values_check
//   values_check < cases.txt
//
// Each input line is one case, fields separated by blanks ("-": an empty array, "null": a null pointer):
//   V <status hex> <source hex> <run hex | null> <vloc> <vlen> <num_runs> <run 0's value bytes> ... <pool> <val_cap | plan | sizes>
// A run's value bytes and the pool are hex, "-", "null" or "null:<size>" (a null pointer with that size).  Number
// lists are comma separated.  Every array is a heap buffer of exactly its bytes (out_vals of exactly val_cap, or for
// "plan" of exactly the plan's val_bytes), so one byte read past an input or a source, or written past an output, is
// a report.  Per case one output line:
//   0 <n> <found> <val_bytes> <out_off> <out_vals hex>        or, refused:  <rc> <n> <found> <val_bytes> <bad key>
// "plan": the sizes come from a call with null outputs, the outputs are then exactly that large; "sizes": that call
// alone.  A refused call must leave its outputs (filled with 0xA5 beforehand) untouched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../storage-engines_amd/csrc/seb_values.h"

static int nibble(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

// exact-size heap copies; "null" gives a null pointer, "-" a pointer to no bytes
static uint8_t *bytes_of(const std::string &h, uint64_t *n) {
    *n = 0;
    if (h == "null") return nullptr;
    if (h.rfind("null:", 0) == 0) return *n = strtoull(h.c_str() + 5, nullptr, 10), nullptr;
    if (h == "-") return (uint8_t *)malloc(0);
    *n = h.size() / 2;
    uint8_t *p = (uint8_t *)malloc(*n);
    for (uint64_t i = 0; i < *n; ++i) p[i] = (uint8_t)(nibble(h[2 * i]) << 4 | nibble(h[2 * i + 1]));
    return p;
}
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
static void hex(const uint8_t *p, uint64_t n) {
    printf(n ? " " : " -");
    for (uint64_t i = 0; i < n; ++i) printf("%02x", p[i]);
}

int main() {
    std::string line;
    uint64_t cases = 0;
    while (std::getline(std::cin, line)) {
        std::stringstream ss(line);
        std::string kind, sh, oh, rh, vl, vn, ph, mode;
        uint32_t num_runs = 0;
        ss >> kind >> sh >> oh >> rh >> vl >> vn >> num_runs;
        const unsigned long long cn = (unsigned long long)cases;
        if (kind != "V") return fprintf(stderr, "case %llu: unknown kind\n", cn), 1;
        uint64_t n = 0, t = 0;
        uint8_t *status = bytes_of(sh, &n);
        uint8_t *source = bytes_of(oh, &t);
        if (source && t != n) return fprintf(stderr, "case %llu: source and status differ in length\n", cn), 1;
        uint8_t *run = bytes_of(rh, &t);
        if (run && t != n) return fprintf(stderr, "case %llu: run and status differ in length\n", cn), 1;
        uint64_t *vloc = nums_of<uint64_t>(vl, &t);
        if (vloc && t != n) return fprintf(stderr, "case %llu: vloc and status differ in length\n", cn), 1;
        uint32_t *vlen = nums_of<uint32_t>(vn, &t);
        if (vlen && t != n) return fprintf(stderr, "case %llu: vlen and status differ in length\n", cn), 1;
        const uint8_t **vals = (const uint8_t **)malloc(sizeof(uint8_t *) * num_runs);
        uint64_t *val_bytes = (uint64_t *)malloc(8 * num_runs);
        for (uint32_t r = 0; r < num_runs; ++r) {
            std::string h;
            ss >> h;
            vals[r] = bytes_of(h, &val_bytes[r]);
        }
        ss >> ph >> mode;
        uint64_t pool_bytes = 0;
        uint8_t *pool = bytes_of(ph, &pool_bytes);
        const seb::ValueSources src{vals, val_bytes, num_runs, pool, pool_bytes};
        seb::ValuesSizes sz{}, plan{};
        uint64_t bad = 0, cap = 0;
        int rc = 0;
        if (mode == "plan" || mode == "sizes") {
            rc = seb::get_values(status, source, run, vloc, vlen, n, src, &plan, nullptr, nullptr, 0, &bad);
            cap = plan.val_bytes;
            sz = plan;
        } else {
            cap = strtoull(mode.c_str(), nullptr, 10);
        }
        if (rc == 0 && mode == "sizes") {
            printf("0 %llu %llu %llu - -\n", (unsigned long long)sz.n, (unsigned long long)sz.found, (unsigned long long)sz.val_bytes);
        } else if (rc == 0) {
            uint64_t *out_off = (uint64_t *)malloc(8 * (n + 1));
            uint8_t *out_vals = (uint8_t *)malloc(cap);
            memset(out_off, 0xA5, 8 * (n + 1));
            memset(out_vals, 0xA5, cap);
            rc = seb::get_values(status, source, run, vloc, vlen, n, src, &sz, out_off, out_vals, cap, &bad);
            if (rc == 0) {
                if (mode == "plan" && memcmp(&sz, &plan, sizeof sz)) return fprintf(stderr, "case %llu: plan and emit sizes differ\n", cn), 1;
                printf("0 %llu %llu %llu", (unsigned long long)sz.n, (unsigned long long)sz.found, (unsigned long long)sz.val_bytes);
                printf(" ");
                for (uint64_t i = 0; i <= n; ++i) printf(i ? ",%llu" : "%llu", (unsigned long long)out_off[i]);
                hex(out_vals, sz.val_bytes), printf("\n");
            } else {
                for (uint64_t i = 0; i < 8 * (n + 1); ++i)
                    if (((uint8_t *)out_off)[i] != 0xA5) return fprintf(stderr, "case %llu: a refused call wrote out_off\n", cn), 1;
                for (uint64_t i = 0; i < cap; ++i)
                    if (out_vals[i] != 0xA5) return fprintf(stderr, "case %llu: a refused call wrote out_vals\n", cn), 1;
            }
            free(out_off), free(out_vals);
        }
        if (rc != 0)
            printf("%d %llu %llu %llu %llu\n", rc, (unsigned long long)sz.n, (unsigned long long)sz.found,
                   (unsigned long long)sz.val_bytes, (unsigned long long)bad);
        for (uint32_t r = 0; r < num_runs; ++r) free((void *)vals[r]);
        free(vals), free(val_bytes), free(status), free(source), free(run), free(vloc), free(vlen), free(pool);
        ++cases;
    }
    printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
