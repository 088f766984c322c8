// seb_filter.cpp — the handle API that mirrors lsm/bloom.go method for method: deferred Adds, the
// device and host copies of a filter, the lock-free host MayContain, and the boundary's CPU fallback.
#include <atomic>
#include <cstdio>
#include <memory>
#include <thread>

#include "seb_host.h"

using namespace seb;

// ------------------------------------------------ Go API mirror (lsm/bloom.go handles) -------

static std::mutex g_pool_mu;
static std::vector<seb_ctx *> g_pool;

static int default_device() {
    long d;
    return env_flag("SEB_DEVICE", &d) ? (int)d : 0;
}

struct CtxLease {  // borrow a context from the process pool (concurrent filters do not serialise)
    seb_ctx *c = nullptr;
    int rc = SEB_OK;
    explicit CtxLease(int device) {
        {
            std::lock_guard<std::mutex> g(g_pool_mu);
            for (size_t i = 0; i < g_pool.size(); ++i)
                if (g_pool[i]->device == device) {
                    c = g_pool[i];
                    g_pool.erase(g_pool.begin() + i);
                    break;
                }
        }
        if (!c) rc = seb_ctx_create(device, &c);
    }
    ~CtxLease() {
        if (c) {
            std::lock_guard<std::mutex> g(g_pool_mu);
            g_pool.push_back(c);
        }
    }
};

static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#endif
}

// A lock for the filter handle: one atomic exchange to take it uncontended (Add takes it once per
// key, so a pthread mutex's call + fence pair showed in the per-key cost), a bounded spin, then
// yields (a waiter may be waiting on a GPU build that takes milliseconds).
struct FilterLock {
    std::atomic<bool> held{false};
    void lock() {
        for (int spin = 0; held.exchange(true, std::memory_order_acquire); ++spin) {
            while (held.load(std::memory_order_relaxed)) {
                if (++spin > 64) std::this_thread::yield();
                else cpu_relax();
            }
        }
    }
    void unlock() { held.store(false, std::memory_order_release); }
};
using FilterGuard = std::lock_guard<FilterLock>;

// Freed filters' device word arrays, kept per device for the next filter of a similar size
// (flushes and compactions create filters of a few sizes over and over); at most 256 MiB.
struct DevWordsPool {
    std::mutex mu;
    struct Buf {
        int device;
        void *p;
        uint64_t bytes;
    };
    std::vector<Buf> free;
    uint64_t total = 0;
    static constexpr uint64_t kCap = 256ull << 20;
    void *take(int device, uint64_t bytes, uint64_t *got) {
        std::lock_guard<std::mutex> g(mu);
        size_t best = free.size();
        for (size_t i = 0; i < free.size(); ++i)
            if (free[i].device == device && free[i].bytes >= bytes && free[i].bytes <= 2 * bytes &&
                (best == free.size() || free[i].bytes < free[best].bytes))
                best = i;
        if (best == free.size()) return nullptr;
        void *p = free[best].p;
        *got = free[best].bytes;
        total -= free[best].bytes;
        free.erase(free.begin() + best);
        return p;
    }
    bool give(int device, void *p, uint64_t bytes) {
        std::lock_guard<std::mutex> g(mu);
        if (total + bytes > kCap) return false;
        free.push_back({device, p, bytes});
        total += bytes;
        return true;
    }
};
static DevWordsPool g_words_pool;

// A filter handle.  Writers (Add, flush, Encode's host sync) hold `mu`.  A single-key MayContain
// does not: once the host copy reflects every Add (no pending keys, host_ok) and the filter is
// usable, `readable` is published (release) and MayContain answers from `host` with no lock, as
// the reference's MayContain runs lock-free from many goroutines (lsm/lsm.go:166 drops the RLock
// before the SSTable loop).  `host` is sized once, at New/Decode, and never reallocated, so a
// reader can never see freed memory; a reader racing an Add on the same filter sees bits of
// either state, which is the reference's own contract (an unsynchronised Go Add/MayContain pair
// is a data race there).
//
// Deferred Adds go to a host arena.  While every key has one length (the reference's SSTable keys
// usually do) the arena is a fixed-stride batch and no offsets are kept: the build reads it as
// such (16-B keys take the vector path), and the H2D copy carries the key bytes only.  The first
// key of another length materialises the offsets.
constexpr uint64_t kNoLen = UINT64_MAX, kMixedLen = UINT64_MAX - 1;
struct seb_filter {
    FilterLock mu;
    uint64_t m = 0;
    uint32_t k = 0;
    uint64_t mu_m = 0, c_m = 0;  // floor((2^64-1)/m), 2^64 mod m: the host MayContain's reductions
    uint64_t nbytes = 0;  // len(bits): ceil(m/8) for New, len(data)-12 for Decode
    int device = 0;
    uint32_t *dwords = nullptr;  // HBM copy, authoritative once allocated
    uint64_t dbytes = 0;
    std::vector<uint8_t> host;  // host copy (valid when host_ok); nbytes long for the handle's life
    bool host_ok = true;
    bool host_zero = false;     // New, nothing built yet: the device copy starts as a memset
    std::atomic<bool> readable{false};  // host_ok, nothing pending, usable: lock-free MayContain
    std::unique_ptr<uint8_t[]> pend; // deferred Add arena: pend_bytes of pend_capb used
    uint64_t pend_bytes = 0, pend_capb = 0;
    std::vector<uint64_t> pend_off;  // n+1 offsets into pend, only once lengths differ
    uint64_t pend_n = 0;
    uint64_t pend_len = kNoLen;      // the common key length, or kMixedLen
    uint64_t pend_cap = 64ull << 20;
};

static void set_moduli(seb_filter *f) {
    if (f->m) {
        f->mu_m = UINT64_MAX / f->m;
        f->c_m = (0 - f->m) % f->m;
    }
}

static bool usable_quiet(const seb_filter *f) {
    return f->m != 0 && f->k <= 4096 && f->nbytes >= seb_num_bytes(f->m);
}

static void publish_locked(seb_filter *f) {
    f->readable.store(f->host_ok && f->pend_n == 0 && usable_quiet(f), std::memory_order_release);
}

// x mod m with mu = floor((2^64-1)/m): the Barrett estimate is at most 2 low.
static inline uint64_t host_mod(uint64_t x, uint64_t m, uint64_t mu) {
    const uint64_t q = (uint64_t)(((unsigned __int128)x * mu) >> 64);
    uint64_t r = x - q * m;
    if (r >= m) r -= m;
    if (r >= m) r -= m;
    return r;
}

// lsm/bloom.go:82-92 for one key on the host copy: hash1 = FNV-1a 64, hash2 = FNV-1 64
// (:44-54), positions (h1 + i*h2) mod m with u64 wraparound (:58-67), LSB-first bit test
// (:87), false at the first clear bit.  The positions are stepped incrementally: with
// r = (h1 + i*h2) mod m and b = h2 mod m, the next residue is r + b mod m, less 2^64 mod m when
// the u64 sum h1 + (i+1)*h2 wrapped: two Barrett reductions per key instead of k divisions.
static int host_may_contain(const seb_filter *f, const uint8_t *key, uint64_t len) {
    const uint8_t *bits = f->host.data();
    const uint64_t m = f->m, c = f->c_m;
    const uint32_t k = f->k;
    uint64_t h1 = 0xcbf29ce484222325ull, h2 = 0xcbf29ce484222325ull;
    const uint64_t P = 0x100000001b3ull;
    for (uint64_t i = 0; i < len; ++i) {
        h1 = (h1 ^ key[i]) * P;
        h2 = (h2 * P) ^ key[i];
    }
    if (k == 0) return 1;  // no positions: the reference's loop never returns false
    uint64_t r = host_mod(h1, m, f->mu_m);
    const uint64_t b = host_mod(h2, m, f->mu_m);
    uint64_t s = h1;
    for (uint32_t i = 0;;) {
        if (!(bits[r >> 3] & (1u << (r & 7)))) return 0;
        if (++i >= k) return 1;
        const uint64_t s2 = s + h2;
        const bool wrap = s2 < s;
        s = s2;
        uint64_t t = r + b;
        if (t < r || t >= m) t -= m;  // r, b < m: one subtract, also when r + b overflowed
        if (wrap) t = t >= c ? t - c : t + (m - c);
        r = t;
    }
}

// The device word array, on `s`: a pooled or new buffer, zeroed, then the host bits unless the
// filter is a fresh New (all zero).
static int ensure_device_copy(seb_filter *f, hipStream_t s, bool clear = true) {
    if (f->dwords) return SEB_OK;
    HIP_OR_FAIL(hipSetDevice(f->device));
    uint64_t want = std::max<uint64_t>(seb_words_bytes(f->m), (f->nbytes + 15) / 16 * 16);
    if (want == 0) want = 16;
    uint64_t got = 0;
    void *p = g_words_pool.take(f->device, want, &got);
    if (!p) {
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(SEB_ERR_NOMEM, "filter: hipMalloc(%llu): %s", (unsigned long long)want, hipGetErrorString(e));
        }
        got = want;
    }
    f->dwords = (uint32_t *)p;
    f->dbytes = got;
    if (f->host_zero) {
        if (clear) HIP_OR_FAIL(hipMemsetAsync(f->dwords, 0, f->dbytes, s));
    } else {
        const uint64_t tail = f->nbytes & ~15ull;  // zero the padding past the copied bytes
        HIP_OR_FAIL(hipMemsetAsync((uint8_t *)f->dwords + tail, 0, f->dbytes - tail, s));
        if (f->nbytes) HIP_OR_FAIL(hipMemcpyAsync(f->dwords, f->host.data(), f->nbytes, hipMemcpyHostToDevice, s));
    }
    return SEB_OK;
}

static int usable(seb_filter *f, const char *who) {
    int rc = check_filter_args(f->m, f->k, who);
    if (rc) return rc;
    if (f->nbytes < seb_num_bytes(f->m))
        return fail(SEB_ERR_SHORT, "%s: decoded bits (%llu B) shorter than ceil(numBits/8) (%llu B); the reference "
                    "panics (index out of range)", who, (unsigned long long)f->nbytes,
                    (unsigned long long)seb_num_bytes(f->m));
    return SEB_OK;
}

// OR host keys into the filter's device words on a pooled context; returns when the build is done.
// `fresh`: the filter is a New with nothing built, and its device words are taken without a clear
// (the build writes them whole or clears them itself); host_zero stays set until the build
// succeeded (build_into_filter drops such a device copy on failure, so a retry starts clean).
static int build_into_filter_device_on(seb_ctx *c, seb_filter *f, const seb_keys *kb, bool fresh);

// On failure the context's stream is drained before the lease goes back, so nothing queued by this
// build can still write the filter's device words when drop_device_copy hands them to the pool;
// only this stream is waited for (no device-wide synchronisation, which would stall other threads'
// work and break their stream captures).
static int build_into_filter_device(seb_filter *f, const seb_keys *kb, bool fresh) {
    if (options().fault_inject)
        return fail(options().fault_inject == 2 ? SEB_ERR_INTERNAL : SEB_ERR_DEVICE,
                    "BloomFilter build: injected %s (fault_inject)",
                    options().fault_inject == 2 ? "internal error" : "device fault");
    CtxLease L(f->device);
    if (L.rc) return L.rc;
    std::lock_guard<std::mutex> g(L.c->mu);
    HIP_OR_FAIL(hipSetDevice(f->device));
    const int rc = build_into_filter_device_on(L.c, f, kb, fresh);
    if (rc != SEB_OK) {
        (void)hipStreamSynchronize(L.c->s_comp);
        (void)hipGetLastError();
    }
    return rc;
}

static int build_into_filter_device_on(seb_ctx *c, seb_filter *f, const seb_keys *kb, bool fresh) {
    int rc;
    // a new filter's first build writes its words whole (image build) or clears them first: no
    // separate memset of the device copy
    if ((rc = ensure_device_copy(f, c->s_comp, !fresh))) return rc;
    f->host_ok = false;  // the device copy is about to move ahead of the host copy
    f->readable.store(false, std::memory_order_relaxed);
    // Small builds skip the DMA engine, whose copies started ~8 us (keys in) and ~16 us (bits out)
    // after the work before them ended (profiles/r03_flush_trace.txt).  Keys: a device-scope-atomic
    // build (flush sizes, one thread per key, hundreds of workgroups) reads them straight from
    // host-pinned staging over PCIe; the LDS builds (a dozen workgroups) read too few at a time for
    // that and get a DMA copy.  Bits: a kernel writes filters up to 16 MiB into pinned memory.
    const ModArg md = mod_arg(f->m, f->k);
    const uint64_t kbytes = kb->offsets ? kb->offsets[kb->n] - kb->offsets[0] : kb->n * (uint64_t)kb->stride;
    const uint64_t obytes = kb->offsets ? (kb->n + 1) * 8 : 0;
    const bool zc_keys = choose_build_algo(kb->n, f->m, f->k) == 1 && kbytes <= (16ull << 20) &&
                         obytes <= (8ull << 20) && !(kb->offsets && kb->n >= options().varlen_prehash_min_keys);
    const bool zc_bits = f->nbytes <= (16ull << 20);
    const bool mirror = f->nbytes <= (64ull << 20);
    if (zc_keys) {
        const uint64_t kpad = (kbytes + 15) & ~15ull;
        if ((rc = c->hkeys.reserve(kpad + obytes + 16))) return rc;
        uint8_t *hk = (uint8_t *)c->hkeys.p;
        if (kbytes) memcpy(hk, kb->data + (kb->offsets ? kb->offsets[0] : 0), kbytes);
        KeyBatch dk{(const uint8_t *)c->hkeys.dev, nullptr, kb->n, kb->stride};
        if (kb->offsets) {
            uint64_t *ho = (uint64_t *)(hk + kpad);
            const uint64_t o0 = kb->offsets[0];
            for (uint64_t i = 0; i <= kb->n; ++i) ho[i] = kb->offsets[i] - o0;
            dk.offsets = (const uint64_t *)((uint8_t *)c->hkeys.dev + kpad);
        }
        if ((rc = ctx_build_dispatch(c, dk, f->dwords, md, fresh))) return rc;
    } else if ((rc = build_device_from_host(c, kb, f->dwords, md, fresh))) {
        return rc;
    }
    // the host copy follows in the same stream (Encode or a first MayContain comes next on the
    // flush path): one synchronisation for build and copy
    if (zc_bits) {
        if ((rc = c->hbits.reserve(f->nbytes + 16))) return rc;
        HIP_OR_FAIL(launch_copy_out(f->dwords, (uint8_t *)c->hbits.dev, f->nbytes, c->s_comp));
    } else if (mirror && f->nbytes) {
        HIP_OR_FAIL(hipMemcpyAsync(f->host.data(), f->dwords, f->nbytes, hipMemcpyDeviceToHost, c->s_comp));
    }
    HIP_OR_FAIL(hipStreamSynchronize(c->s_comp));
    if (zc_bits && f->nbytes) memcpy(f->host.data(), c->hbits.p, f->nbytes);
    f->host_ok = mirror;
    f->host_zero = false;
    return SEB_OK;
}

// The boundary's CPU fallback (SURVEY.md 8(b) error row): the Go API has no error returns
// (lsm/bloom.go:19-41,70-77,96-102 never fail on valid input), so a build or batched probe whose
// device path fails for want of a device or of memory is done on the filter's host copy instead,
// with the same arithmetic as host_may_contain.  Every use is counted (seb_fallback_count); the
// GPU tests and smoke() assert that the count stays 0, so the parity they show is the HIP path's.
static std::atomic<uint64_t> g_fallbacks{0};

extern "C" uint64_t seb_fallback_count(void) { return g_fallbacks.load(std::memory_order_relaxed); }

static bool device_failure(int rc) { return rc == SEB_ERR_DEVICE || rc == SEB_ERR_NOMEM; }

// Counts a fallback; the first one in the process is also written to stderr with its cause (the
// failing call's seb_last_error), so a deployment sees it without reading the counter.
static void note_fallback(const char *who) {
    if (g_fallbacks.fetch_add(1, std::memory_order_relaxed) == 0)
        fprintf(stderr, "seb_bloom: %s fell back to the host copy (CPU) after a device failure: %s\n", who,
                last_error().c_str());
}

// lsm/bloom.go:70-77 for one key on the host copy: positions stepped as in host_may_contain
// ((h1 + i*h2) mod m with u64 wraparound, :58-67), LSB-first byte ORs (:73-75).
static void host_add_key(seb_filter *f, const uint8_t *key, uint64_t len) {
    uint8_t *bits = f->host.data();
    const uint64_t m = f->m, c = f->c_m;
    const uint32_t k = f->k;
    uint64_t h1 = 0xcbf29ce484222325ull, h2 = 0xcbf29ce484222325ull;
    const uint64_t P = 0x100000001b3ull;
    for (uint64_t i = 0; i < len; ++i) {
        h1 = (h1 ^ key[i]) * P;
        h2 = (h2 * P) ^ key[i];
    }
    uint64_t r = host_mod(h1, m, f->mu_m);
    const uint64_t b = host_mod(h2, m, f->mu_m);
    uint64_t s = h1;
    for (uint32_t i = 0; i < k; ++i) {
        bits[r >> 3] |= (uint8_t)(1u << (r & 7));
        const uint64_t s2 = s + h2;
        const bool wrap = s2 < s;
        s = s2;
        uint64_t t = r + b;
        if (t < r || t >= m) t -= m;
        if (wrap) t = t >= c ? t - c : t + (m - c);
        r = t;
    }
}

static const uint8_t *host_key(const seb_keys *kb, uint64_t i, uint64_t *len) {
    if (kb->offsets) {
        *len = kb->offsets[i + 1] - kb->offsets[i];
        return kb->data + kb->offsets[i];
    }
    *len = kb->stride;
    return kb->data + i * (uint64_t)kb->stride;
}

// Give the device word array back: a copy that is garbage (a fresh build that failed) or stale
// (the host copy moved ahead in a fallback).  Its only writer, the failed build's stream, was
// drained before that build's lease ended (build_into_filter_device).  The next device use
// uploads the host copy again (ensure_device_copy).
static void drop_device_copy(seb_filter *f) {
    if (!f->dwords) return;
    (void)hipSetDevice(f->device);
    if (!g_words_pool.give(f->device, f->dwords, f->dbytes)) (void)hipFree(f->dwords);
    (void)hipGetLastError();
    f->dwords = nullptr;
    f->dbytes = 0;
}

static int build_into_filter(seb_filter *f, const seb_keys *kb) {
    const bool fresh = f->host_zero && !f->dwords;
    const bool host_was_ok = f->host_ok;
    int rc = build_into_filter_device(f, kb, fresh);
    if (rc == SEB_OK) return SEB_OK;
    if (fresh) {  // its device words were never cleared: back to a New's state, so a retry starts from zeros
        drop_device_copy(f);
        if (f->nbytes) memset(f->host.data(), 0, f->nbytes);
        f->host_ok = true;
    }
    // Otherwise the device copy (authoritative while host_ok is false) holds the old bits ORed with
    // part of this batch at most, and the batch stays pending: a retry ORs it whole.
    if (!device_failure(rc) || !options().cpu_fallback || !(fresh || host_was_ok) || f->nbytes < seb_num_bytes(f->m))
        return rc;  // no usable host copy to fall back on (a large filter whose device copy is ahead)
    // The host copy holds the bits before this build, or (a D2H that ran before the failure) those
    // ORed with some of this batch's: OR-ing the whole batch into it gives the right filter.
    for (uint64_t i = 0; i < kb->n; ++i) {
        uint64_t len;
        const uint8_t *key = host_key(kb, i, &len);
        host_add_key(f, key, len);
    }
    drop_device_copy(f);
    f->host_ok = true;
    f->host_zero = false;
    note_fallback("BloomFilter build");
    (void)hipGetLastError();
    return SEB_OK;
}

static int flush_locked(seb_filter *f) {
    if (f->pend_n == 0) return SEB_OK;
    int rc = usable(f, "BloomFilter.Add");
    if (rc) return rc;
    const bool uniform = f->pend_len != kMixedLen;
    seb_keys kb{f->pend.get(), uniform ? nullptr : f->pend_off.data(), f->pend_n,
                uniform ? (uint32_t)f->pend_len : 0u, 0};
    if ((rc = build_into_filter(f, &kb))) return rc;
    f->pend_bytes = 0;
    f->pend_off.clear();
    f->pend_n = 0;
    f->pend_len = kNoLen;
    publish_locked(f);
    return SEB_OK;
}

// Room for `more` bytes in the Add arena (doubling); false when memory runs out.
static bool arena_reserve(seb_filter *f, uint64_t more) {
    if (f->pend_bytes + more <= f->pend_capb) return true;
    uint64_t cap = std::max<uint64_t>({f->pend_bytes + more, 2 * f->pend_capb, 4096});
    uint8_t *p = new (std::nothrow) uint8_t[cap];
    if (!p) return false;
    if (f->pend_bytes) memcpy(p, f->pend.get(), f->pend_bytes);
    f->pend.reset(p);
    f->pend_capb = cap;
    return true;
}

extern "C" seb_filter *seb_filter_new(int64_t n, double p) {
    uint64_t m;
    uint32_t k;
    if (seb_params(n, p, &m, &k) != SEB_OK) return nullptr;
    seb_filter *f = new (std::nothrow) seb_filter();
    if (!f) return nullptr;
    f->m = m;
    f->k = k;
    set_moduli(f);
    f->nbytes = seb_num_bytes(m);
    f->device = default_device();
    f->host.assign(f->nbytes, 0);
    f->host_zero = true;
    long cap;
    if (env_flag("SEB_PENDING_CAP", &cap) && cap > 0) f->pend_cap = (uint64_t)cap;
    // the caller's expectedKeys: room for that many 16-B keys (the arena still grows past it)
    if (n > 0) (void)arena_reserve(f, std::min<uint64_t>((uint64_t)n * 16, f->pend_cap));
    publish_locked(f);  // an empty filter answers false everywhere
    return f;
}

extern "C" void seb_filter_free(seb_filter *f) {
    if (!f) return;
    if (f->dwords && !g_words_pool.give(f->device, f->dwords, f->dbytes)) {
        (void)hipSetDevice(f->device);
        (void)hipFree(f->dwords);
    }
    delete f;
}

extern "C" int seb_filter_add(seb_filter *f, const uint8_t *key, uint64_t len) {
    if (!f || (!key && len)) return fail(SEB_ERR_INVALID, "BloomFilter.Add: null argument");
    FilterGuard g(f->mu);
    if (__builtin_expect(!usable_quiet(f), 0)) return usable(f, "BloomFilter.Add");
    f->readable.store(false, std::memory_order_relaxed);  // pending keys: MayContain must flush first
    if (len != f->pend_len) {
        if (f->pend_len == kNoLen && len <= 0xffffffffull) {
            f->pend_len = len;
        } else if (f->pend_len != kMixedLen) {  // the first key of another length: keep offsets from here
            f->pend_off.resize(f->pend_n + 1);
            for (uint64_t i = 0; i <= f->pend_n; ++i) f->pend_off[i] = i * f->pend_len;
            f->pend_len = kMixedLen;
        }
    }
    if (!arena_reserve(f, len)) return fail(SEB_ERR_NOMEM, "BloomFilter.Add: arena of %llu B", (unsigned long long)len);
    uint8_t *dst = f->pend.get() + f->pend_bytes;
    if (len == 16)
        memcpy(dst, key, 16);  // the reference's fixed-size keys: one 16-B move
    else if (len)
        memcpy(dst, key, len);
    f->pend_bytes += len;
    ++f->pend_n;
    if (f->pend_len == kMixedLen) f->pend_off.push_back(f->pend_bytes);
    if (f->pend_bytes >= f->pend_cap || f->pend_n >= (1ull << 32)) return flush_locked(f);
    return SEB_OK;
}

extern "C" int seb_filter_add_batch(seb_filter *f, const seb_keys *kb) {
    if (!f) return fail(SEB_ERR_INVALID, "BloomFilter.Add: null filter");
    int rc;
    if ((rc = check_keys(kb, "BloomFilter.Add")) || (rc = validate_offsets(kb, "BloomFilter.Add"))) return rc;
    FilterGuard g(f->mu);
    if ((rc = usable(f, "BloomFilter.Add"))) return rc;
    if ((rc = flush_locked(f))) return rc;  // keep Add order: earlier single Adds first
    if (kb->n == 0) return SEB_OK;
    if ((rc = build_into_filter(f, kb))) return rc;
    publish_locked(f);
    return SEB_OK;
}

static int probe_filter_device(seb_filter *f, const seb_keys *kb, uint8_t *out) {
    if (options().fault_inject)
        return fail(options().fault_inject == 2 ? SEB_ERR_INTERNAL : SEB_ERR_DEVICE,
                    "BloomFilter probe: injected %s (fault_inject)",
                    options().fault_inject == 2 ? "internal error" : "device fault");
    CtxLease L(f->device);
    if (L.rc) return L.rc;
    std::lock_guard<std::mutex> g2(L.c->mu);
    HIP_OR_FAIL(hipSetDevice(f->device));
    int rc;
    if ((rc = ensure_device_copy(f, L.c->s_comp))) return rc;
    return probe_device_to_host(L.c, kb, f->dwords, mod_arg(f->m, f->k), out);
}

extern "C" int seb_filter_may_contain_batch(seb_filter *f, const seb_keys *kb, uint8_t *out) {
    WsCall ws_call;
    if (!f) return fail(SEB_ERR_INVALID, "BloomFilter.MayContain: null filter");
    int rc;
    if ((rc = check_keys(kb, "BloomFilter.MayContain")) || (rc = validate_offsets(kb, "BloomFilter.MayContain")))
        return rc;
    if (!out && kb->n) return fail(SEB_ERR_INVALID, "BloomFilter.MayContain: null out");
    FilterGuard g(f->mu);
    if ((rc = usable(f, "BloomFilter.MayContain"))) return rc;
    if ((rc = flush_locked(f))) return rc;
    rc = probe_filter_device(f, kb, out);
    if (rc == SEB_OK || !device_failure(rc) || !options().cpu_fallback || !f->host_ok) return rc;
    for (uint64_t i = 0; i < kb->n; ++i) {  // the boundary's CPU fallback (see build_into_filter)
        uint64_t len;
        const uint8_t *key = host_key(kb, i, &len);
        out[i] = (uint8_t)host_may_contain(f, key, len);
    }
    note_fallback("BloomFilter.MayContain batch");
    (void)hipGetLastError();
    return SEB_OK;
}

static int sync_host_locked(seb_filter *f);

// MayContain(key) (lsm/bloom.go:82-92), called once per Get per candidate SSTable
// (lsm/sstable.go:206): answered on the host copy, lock-free once the filter is readable.  A GPU
// launch costs microseconds against ~100 ns for this; batches go to the GPU
// (seb_filter_may_contain_batch).
extern "C" int seb_filter_may_contain(seb_filter *f, const uint8_t *key, uint64_t len) {
    if (!f) return fail(SEB_ERR_INVALID, "BloomFilter.MayContain: null filter");
    if (!key && len) return fail(SEB_ERR_INVALID, "BloomFilter.MayContain: null key");
    if (!f->readable.load(std::memory_order_acquire)) {
        FilterGuard g(f->mu);
        int rc;
        if ((rc = usable(f, "BloomFilter.MayContain")) || (rc = flush_locked(f)) || (rc = sync_host_locked(f)))
            return rc;
        publish_locked(f);
    }
    return host_may_contain(f, key, len);
}

static int sync_host_locked(seb_filter *f) {
    if (f->host_ok) return SEB_OK;
    HIP_OR_FAIL(hipSetDevice(f->device));
    if (f->nbytes) HIP_OR_FAIL(hipMemcpy(f->host.data(), f->dwords, f->nbytes, hipMemcpyDeviceToHost));
    f->host_ok = true;
    publish_locked(f);
    return SEB_OK;
}

extern "C" uint64_t seb_filter_encoded_size(seb_filter *f) { return f ? 12 + f->nbytes : 0; }

extern "C" int seb_filter_encode(seb_filter *f, uint8_t *out, uint64_t cap) {
    if (!f || !out) return fail(SEB_ERR_INVALID, "BloomFilter.Encode: null argument");
    FilterGuard g(f->mu);
    if (cap < 12 + f->nbytes) return fail(SEB_ERR_INVALID, "BloomFilter.Encode: buffer too small");
    int rc;
    if ((rc = flush_locked(f)) || (rc = sync_host_locked(f))) return rc;
    for (int b = 0; b < 8; ++b) out[b] = (uint8_t)(f->m >> (8 * b));  // binary.LittleEndian
    for (int b = 0; b < 4; ++b) out[8 + b] = (uint8_t)(f->k >> (8 * b));
    if (f->nbytes) memcpy(out + 12, f->host.data(), f->nbytes);
    return SEB_OK;
}

extern "C" seb_filter *seb_filter_decode(const uint8_t *data, uint64_t len) {
    if (!data || len < 12) {
        fail(SEB_ERR_INVALID, "DecodeBloomFilter: %llu bytes < 12 (Go returns nil)", (unsigned long long)len);
        return nullptr;
    }
    seb_filter *f = new (std::nothrow) seb_filter();
    if (!f) return nullptr;
    for (int b = 0; b < 8; ++b) f->m |= (uint64_t)data[b] << (8 * b);
    for (int b = 0; b < 4; ++b) f->k |= (uint32_t)data[8 + b] << (8 * b);
    f->nbytes = len - 12;
    set_moduli(f);
    f->device = default_device();
    f->host.assign(data + 12, data + len);
    publish_locked(f);  // immutable from here unless Add is called on it
    return f;
}

extern "C" uint64_t seb_filter_num_bits(const seb_filter *f) { return f ? f->m : 0; }
extern "C" uint32_t seb_filter_num_hashes(const seb_filter *f) { return f ? f->k : 0; }
extern "C" uint64_t seb_filter_pending(seb_filter *f) {
    if (!f) return 0;
    FilterGuard g(f->mu);
    return f->pend_n;
}
extern "C" int seb_filter_flush(seb_filter *f) {
    if (!f) return fail(SEB_ERR_INVALID, "flush: null filter");
    FilterGuard g(f->mu);
    return flush_locked(f);
}
