// seb_host.cpp — the C ABI (include/seb_bloom.h), its base: errors, options, the stream workspace,
// the build and probe dispatchers, the device-resident bloom entry points, memory and timers, shard
// routing and WAL checksums.  The host-buffer entry points (a chunked H2D -> kernel -> D2H pipeline
// through a context) are in seb_ctx.cpp, the handle API that mirrors lsm/bloom.go method for method
// in seb_filter.cpp, the registry in seb_registry.cpp, the SSTable halves in seb_sstable.cpp.
#include <cctype>
#include <cstdarg>
#include <cstdio>
#include <memory>

#include "seb_host.h"

using namespace seb;

// ------------------------------------------------------------------ errors ------------------

static thread_local std::string t_err;

std::string &seb::last_error() { return t_err; }

int seb::fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    t_err = buf;
    return code;
}

extern "C" const char *seb_last_error(void) { return t_err.c_str(); }
extern "C" int seb_abi_version(void) { return SEB_ABI_VERSION; }

// ------------------------------------------------------------------ helpers -----------------

extern "C" uint64_t seb_num_bytes(uint64_t m) { return m / 8 + (m % 8 != 0); }
extern "C" uint64_t seb_words_bytes(uint64_t m) { return (m / 128 + (m % 128 != 0)) * 16; }

extern "C" int seb_params(int64_t n, double p, uint64_t *m, uint32_t *k) {
    if (!m || !k) return fail(SEB_ERR_INVALID, "seb_params: null output");
    if (seb::params(n, p, m, k) != 0)
        return fail(SEB_ERR_RANGE, "seb_params: n=%lld p=%g outside the reference's defined range", (long long)n, p);
    return SEB_OK;
}

int seb::check_filter_args(uint64_t m, uint32_t k, const char *who) {
    if (m == 0) return fail(SEB_ERR_INVALID, "%s: numBits == 0 (the reference panics: integer divide by zero)", who);
    if (k > 4096) return fail(SEB_ERR_INVALID, "%s: numHashes %u > 4096", who, k);
    return SEB_OK;
}

int seb::check_keys(const seb_keys *kb, const char *who) {
    if (!kb) return fail(SEB_ERR_INVALID, "%s: null keys", who);
    if (kb->reserved != 0) return fail(SEB_ERR_INVALID, "%s: keys.reserved must be 0", who);
    if (kb->n > 0 && !kb->data && (kb->offsets || kb->stride != 0))
        return fail(SEB_ERR_INVALID, "%s: null key data", who);
    return SEB_OK;
}

int seb::validate_offsets(const seb_keys *kb, const char *who) {
    if (!kb->offsets) return SEB_OK;
    for (uint64_t i = 0; i < kb->n; ++i)
        if (kb->offsets[i + 1] < kb->offsets[i]) return fail(SEB_ERR_INVALID, "%s: offsets decrease at %llu", who, (unsigned long long)i);
    return SEB_OK;
}

// Every knob of seb_set_option: name, field, accepted range.  SEB_<NAME> in the environment sets
// its initial value.
struct OptionDesc {
    const char *name;
    int64_t lo, hi;
    int64_t (*get)(const Options &);
    void (*set)(Options &, int64_t);
};
#define SEB_OPT(field, lo, hi)                                                              \
    OptionDesc {                                                                            \
        #field, lo, hi, [](const Options &o) { return (int64_t)o.field; },                   \
            [](Options &o, int64_t v) { o.field = (decltype(o.field))v; }                    \
    }
static const OptionDesc kOptions[] = {
    SEB_OPT(build_algo, 0, 4),
    SEB_OPT(multi_interleave, 0, 1),
    SEB_OPT(multiget_order, 0, 2),
    SEB_OPT(multiget_l0_group, 0, 1),
    SEB_OPT(multiget_xcd, 0, 1),
    SEB_OPT(varlen_prehash_min_keys, 0, INT64_MAX),
    SEB_OPT(bucket_min_keys, 0, INT64_MAX),
    SEB_OPT(lds_min_keys, 0, INT64_MAX),
    SEB_OPT(many_splits, 0, 64),
    SEB_OPT(probe_phases, 0, 64),
    SEB_OPT(probe_compact, 0, 1),
    SEB_OPT(scatter_bins, 0, 1),
    SEB_OPT(grid_cap, 1, 1 << 30),
    SEB_OPT(workspace_limit_mib, 0, 1 << 30),
    SEB_OPT(multiget_piece_mib, 1, 1 << 20),
    SEB_OPT(varlen_tail, 0, 3),
    SEB_OPT(cpu_fallback, 0, 1),
    SEB_OPT(fault_inject, 0, 2),
    SEB_OPT(hidx_hash_mask, 0, INT64_MAX),
};
#undef SEB_OPT

static const OptionDesc *find_option(const char *name) {
    for (const OptionDesc &d : kOptions)
        if (!strcmp(d.name, name)) return &d;
    return nullptr;
}

static std::once_flag g_env_once;
static void load_env() {
    Options &o = options();
    for (const OptionDesc &d : kOptions) {
        char var[64] = "SEB_";
        size_t j = 4;
        for (const char *c = d.name; *c && j + 1 < sizeof var; ++c) var[j++] = (char)toupper((unsigned char)*c);
        var[j] = 0;
        long v;
        if (env_flag(var, &v) && v >= d.lo && v <= d.hi) d.set(o, v);
    }
}

void seb::enter() {
    std::call_once(g_env_once, load_env);
    (void)hipGetLastError();
}

extern "C" int seb_set_option(const char *name, int64_t value) {
    std::call_once(g_env_once, load_env);
    if (!name) return fail(SEB_ERR_INVALID, "seb_set_option: null name");
    const OptionDesc *d = find_option(name);
    if (!d || value < d->lo || value > d->hi)
        return fail(SEB_ERR_INVALID, "seb_set_option: bad option %s=%lld", name, (long long)value);
    d->set(options(), value);
    return SEB_OK;
}

extern "C" int seb_get_option(const char *name, int64_t *value) {
    std::call_once(g_env_once, load_env);
    if (!name || !value) return fail(SEB_ERR_INVALID, "seb_get_option: null argument");
    const OptionDesc *d = find_option(name);
    if (!d) return fail(SEB_ERR_INVALID, "seb_get_option: unknown option %s", name);
    *value = d->get(options());
    return SEB_OK;
}

extern "C" int seb_device_check(int device) {
    std::call_once(g_env_once, load_env);
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0)
        return fail(SEB_ERR_DEVICE, "no HIP device (%s)", e != hipSuccess ? hipGetErrorString(e) : "count 0");
    if (device < 0 || device >= count) return fail(SEB_ERR_DEVICE, "device %d out of range (count %d)", device, count);
    hipDeviceProp_t prop;
    HIP_OR_FAIL(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SEB_ERR_DEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    return SEB_OK;
}

// ------------------------------------------------------- device-resident entry points --------

extern "C" int seb_dev_clear(uint32_t *words, uint64_t m, void *stream) {
    enter();
    if (!words && m) return fail(SEB_ERR_INVALID, "seb_dev_clear: null words");
    if (m == 0) return SEB_OK;
    if (((uintptr_t)words & 15) == 0)
        HIP_OR_FAIL(launch_clear_words(words, seb_words_bytes(m), (hipStream_t)stream));
    else
        HIP_OR_FAIL(hipMemsetAsync(words, 0, seb_words_bytes(m), (hipStream_t)stream));
    return SEB_OK;
}

// Library-owned scratch: grow-only buffers, one set per (device, stream), so concurrent streams
// never share one.  Calls on ONE stream are ordered by the stream, but their enqueue phases can
// overlap across host threads; so an ABI call holds its stream's slot (a recursive lock) from its
// first workspace request until it returns (WsCall at the entry point).  A second thread's call
// on the same stream therefore enqueues after the first call's launches, and a grow (stream sync
// + free) can never free a buffer that another thread has been handed but not yet launched on.
struct WsEntry {
    int tag;  // 0: build / key preparation; 1: packed residues; 2: compacted probe rows; 3: MultiGet key-range order;
              // 4: the fresh build's overflow bitmap (kept all zero)
    void *p;
    uint64_t bytes;
};
struct WsSlot {
    int device;
    hipStream_t stream;
    bool dead = false;  // its stream was destroyed (ws_drop_stream); reusable for a new one
    std::recursive_mutex mu;  // held by the call enqueueing against this slot's buffers
    std::vector<WsEntry> bufs;
};
static std::mutex g_ws_mu;  // guards the slot list; each slot's buffers are guarded by slot->mu
static std::vector<std::unique_ptr<WsSlot>> g_ws;
static thread_local int t_ws_depth = 0;
static thread_local std::vector<std::unique_lock<std::recursive_mutex>> t_ws_held;

WsCall::WsCall() : mark(t_ws_held.size()) {
    if (t_ws_depth++ == 0) (void)hipGetLastError();  // as enter(): no stale error from before this call
}
WsCall::~WsCall() {
    while (t_ws_held.size() > mark) t_ws_held.pop_back();
    --t_ws_depth;
}

static WsSlot *ws_slot(int dev, hipStream_t s) {
    std::lock_guard<std::mutex> g(g_ws_mu);
    for (auto &sl : g_ws)
        if (!sl->dead && sl->device == dev && sl->stream == s) return sl.get();
    for (auto &sl : g_ws)
        if (sl->dead) {  // buffers already freed; nobody holds a dead slot's lock
            sl->dead = false;
            sl->device = dev;
            sl->stream = s;
            return sl.get();
        }
    g_ws.emplace_back(new WsSlot());
    g_ws.back()->device = dev;
    g_ws.back()->stream = s;
    return g_ws.back().get();
}

// A failed hipMalloc is answered with SEB_ERR_NOMEM and HIP's error state is cleared, so a caller
// that falls back (MultiGet's batch order) does not find it again in a later hipGetLastError.
static int ws_alloc(void **p, uint64_t bytes) {
    const uint64_t lim = options().workspace_limit_mib;
    if (lim && bytes > (lim << 20))
        return fail(SEB_ERR_NOMEM, "workspace %llu B > workspace_limit_mib %llu", (unsigned long long)bytes,
                    (unsigned long long)lim);
    hipError_t a = hipMalloc(p, bytes);
    if (a != hipSuccess) {
        *p = nullptr;
        (void)hipGetLastError();
        return fail(SEB_ERR_NOMEM, "workspace hipMalloc(%llu): %s", (unsigned long long)bytes, hipGetErrorString(a));
    }
    return SEB_OK;
}

int seb::cached_workspace(hipStream_t s, uint64_t bytes, void **out, int tag, bool zero) {
    if (t_ws_depth == 0) return fail(SEB_ERR_INVALID, "internal: library scratch requested outside a WsCall scope");
    int dev = 0;
    HIP_OR_FAIL(hipGetDevice(&dev));
    WsSlot *sl = ws_slot(dev, s);
    t_ws_held.emplace_back(sl->mu);  // released when the outermost WsCall of this thread returns
    for (auto &e : sl->bufs)
        if (e.tag == tag) {
            if (e.bytes >= bytes) {
                *out = e.p;
                return SEB_OK;
            }
            HIP_OR_FAIL(hipStreamSynchronize(s));  // earlier launches on this stream may still read it
            HIP_OR_FAIL(hipFree(e.p));
            e.p = nullptr;
            e.bytes = 0;
            int rc = ws_alloc(&e.p, bytes);
            if (rc) return rc;
            e.bytes = bytes;
            if (zero) HIP_OR_FAIL(hipMemsetAsync(e.p, 0, bytes, s));
            *out = e.p;
            return SEB_OK;
        }
    void *p = nullptr;
    int rc = ws_alloc(&p, bytes);
    if (rc) return rc;
    sl->bufs.push_back({tag, p, bytes});
    if (zero) HIP_OR_FAIL(hipMemsetAsync(p, 0, bytes, s));
    *out = p;
    return SEB_OK;
}

void seb::ws_drop_stream(int dev, hipStream_t s) {
    WsSlot *sl = nullptr;
    {
        std::lock_guard<std::mutex> g(g_ws_mu);
        for (auto &x : g_ws)
            if (!x->dead && x->device == dev && x->stream == s) sl = x.get();
    }
    if (!sl) return;
    std::lock_guard<std::recursive_mutex> g2(sl->mu);  // a call still enqueueing on it finishes first
    if (!sl->bufs.empty()) {
        (void)hipStreamSynchronize(s);
        for (auto &b : sl->bufs) (void)hipFree(b.p);
        sl->bufs.clear();
    }
    (void)hipGetLastError();
    std::lock_guard<std::mutex> g(g_ws_mu);
    sl->dead = true;
}

// Drop this stream's scratch buffer `tag` (after a failed call that may have left it dirty, such as
// the fresh build's overflow bitmap); the next request allocates (and zeroes) a new one.
static void ws_discard(hipStream_t s, int tag) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return (void)hipGetLastError();
    WsSlot *sl = ws_slot(dev, s);
    std::lock_guard<std::recursive_mutex> g(sl->mu);
    for (auto &e : sl->bufs)
        if (e.tag == tag && e.p) {
            (void)hipStreamSynchronize(s);
            (void)hipFree(e.p);
            e.p = nullptr;
            e.bytes = 0;
        }
    (void)hipGetLastError();
}

// Slots are never deleted, so the pointers stay valid after g_ws_mu is dropped (a call holding a
// slot's lock may take g_ws_mu for another request, so the two are never held in that order here).
static std::vector<WsSlot *> ws_slots_snapshot() {
    std::lock_guard<std::mutex> g(g_ws_mu);
    std::vector<WsSlot *> v;
    for (auto &sl : g_ws) v.push_back(sl.get());
    return v;
}

extern "C" uint64_t seb_workspace_bytes(void) {
    uint64_t total = 0;
    for (WsSlot *sl : ws_slots_snapshot()) {
        std::lock_guard<std::recursive_mutex> g(sl->mu);
        for (auto &e : sl->bufs) total += e.bytes;
    }
    return total;
}

extern "C" int seb_workspace_release(void) {
    int saved = 0;
    HIP_OR_FAIL(hipGetDevice(&saved));
    int rc = SEB_OK;
    for (WsSlot *sl : ws_slots_snapshot()) {
        std::lock_guard<std::recursive_mutex> g2(sl->mu);  // waits for a call still enqueueing on it
        if (sl->bufs.empty()) continue;
        hipError_t e = hipSetDevice(sl->device);
        if (e == hipSuccess) e = hipStreamSynchronize(sl->stream);
        for (auto &b : sl->bufs)
            if (e == hipSuccess) e = hipFree(b.p);
        if (e != hipSuccess) {
            rc = fail(hip_status(e), "seb_workspace_release: %s", hipGetErrorString(e));
            break;
        }
        sl->bufs.clear();
    }
    (void)hipSetDevice(saved);
    return rc;
}

static bool want_prehash(const KeyBatch &kb) {
    return kb.offsets && !kb.hashes && kb.n >= options().varlen_prehash_min_keys;
}
static uint64_t prehash_bytes(const KeyBatch &kb) { return want_prehash(kb) ? ((kb.n * 16 + 255) & ~255ull) : 0; }
// Pre-hash straight to packed residues (8 B per key) when the filter allows them (k == 7,
// m < 2^29): the bucketed build and the phased probe then read half the bytes per key and skip
// re-deriving the residues.
static bool want_prehash_packed(const KeyBatch &kb, const ModArg &md) {
    return want_prehash(kb) && md.k == 7 && md.m < (1ull << kPackBits);
}

// The build dispatcher (seb_host.h).
int seb::build_dispatch(KeyBatch kb, uint32_t *words, const ModArg &md, hipStream_t s, void *ws, uint64_t ws_bytes,
                        const GrowFn &grow, bool fresh, uint32_t *ovf) {
    // The clear kernel and the image build's OR kernel store 16 B per lane: word arrays that are
    // only 4-B aligned are cleared by hipMemsetAsync and built by the LDS-filter build instead.
    const bool a16 = ((uintptr_t)words & 15) == 0;
    auto clear = [&]() -> hipError_t {
        return a16 ? launch_clear_words(words, seb_words_bytes(md.m), s)
                   : hipMemsetAsync(words, 0, seb_words_bytes(md.m), s);
    };
    if (kb.n == 0 || md.k == 0) {
        if (fresh) HIP_OR_FAIL(clear());
        return SEB_OK;
    }
    int algo = choose_build_algo(kb.n, md.m, md.k);
    if (algo == 4 && !a16) algo = 3;
    const bool bucketed = algo == 2;
    if (!(fresh && bucketed)) ovf = nullptr;
    if (fresh && algo != 4 && !ovf) HIP_OR_FAIL(clear());
    if (bucketed && want_prehash_packed(kb, md)) {  // scratch: [packed residues | bucketed]
        const uint64_t pack_b = (kb.n * 8 + 255) & ~255ull;
        const uint64_t need = pack_b + bucketed_workspace_bytes(kb.n, md.m, md.k);
        if (need > ws_bytes) {
            int rc = grow(need, &ws);
            if (rc) return rc;
            ws_bytes = need;
        }
        HIP_OR_FAIL(launch_hash_varlen_packed(kb, md, (uint64_t *)ws, s));
        HIP_OR_FAIL(launch_build_bucketed_packed((const uint64_t *)ws, kb.n, words, md, (uint8_t *)ws + pack_b,
                                                 ws_bytes - pack_b, s, ovf));
        return SEB_OK;
    }
    const uint64_t head = prehash_bytes(kb);
    const uint64_t need = head + (bucketed ? bucketed_workspace_bytes(kb.n, md.m, md.k)
                                  : algo == 4 ? image_workspace_bytes(kb.n, md.m) : 0);
    if (need > ws_bytes) {
        int rc = grow(need, &ws);
        if (rc) return rc;
        ws_bytes = need;
    }
    if (head) {
        HIP_OR_FAIL(launch_hash_varlen(kb, (uint4 *)ws, s));
        kb.hashes = (const uint4 *)ws;
    }
    if (bucketed) {
        HIP_OR_FAIL(launch_build_bucketed(kb, words, md, (uint8_t *)ws + head, ws_bytes - head, s, ovf));
        return SEB_OK;
    }
    if (algo == 4) {
        HIP_OR_FAIL(launch_build_images(kb, words, md, (uint8_t *)ws + head, ws_bytes - head, fresh, s));
        return SEB_OK;
    }
    if (algo == 3) {  // the whole filter in one CU's LDS, the keys split over workgroups (build_many's kernel)
        ManyArg ma;
        memset(&ma, 0, sizeof ma);
        ma.nf = 1;
        ma.f[0].words = words;
        ma.f[0].nwords = seb_words_bytes(md.m) / 4;
        ma.f[0].key_begin = 0;
        ma.f[0].key_end = kb.n;
        ma.f[0].md = md;
        HIP_OR_FAIL(launch_build_many_lds(kb, ma, (uint32_t)seb_words_bytes(md.m), s));
        return SEB_OK;
    }
    HIP_OR_FAIL(launch_build(kb, words, md, s));
    return SEB_OK;
}

// Variable-length probe batches: pre-hash into the per-(device, stream) scratch cache first.
// `extra` bytes at the front of the scratch are the caller's.
static int prepare_probe_keys(KeyBatch &kb, hipStream_t s, uint64_t extra, void **ws_out) {
    const uint64_t pre_b = prehash_bytes(kb);
    *ws_out = nullptr;
    if (extra + pre_b == 0) return SEB_OK;
    void *ws = nullptr;
    int rc = cached_workspace(s, extra + pre_b, &ws);
    if (rc) return rc;
    *ws_out = ws;
    if (pre_b) {
        HIP_OR_FAIL(launch_hash_varlen(kb, (uint4 *)((uint8_t *)ws + extra), s));
        kb.hashes = (const uint4 *)((uint8_t *)ws + extra);
    }
    return SEB_OK;
}

// The phased probe applies to k == 7, m < 2^29 filters spanning more than one phase, with a
// 4-byte aligned answer array.
static bool want_phased(uint64_t n, const ModArg &md, const uint8_t *out) {
    if (md.k != 7 || md.m >= (1ull << kPackBits)) return false;
    return probe_phase_count(md.m) > 1 && ((uintptr_t)out & 3) == 0 && n > 0;
}

int seb::probe_dispatch(KeyBatch kb, const uint32_t *words, const ModArg &md, uint8_t *out, hipStream_t s) {
    void *ws;
    int rc;
    if (want_phased(kb.n, md, out) && want_prehash_packed(kb, md) && options().probe_compact) {
        // the pre-hash with phase 0 fused in: compacted rows (tag 2) only, no dense packed batch
        void *rows;
        if ((rc = cached_workspace(s, probe_compact_bytes(kb.n), &rows, 2))) return rc;
        HIP_OR_FAIL(launch_probe_compact_varlen(kb, words, md, out, rows, s));
        return SEB_OK;
    }
    if (want_phased(kb.n, md, out) && want_prehash_packed(kb, md)) {  // pre-hash to packed, all phases from it
        void *packed;
        if ((rc = cached_workspace(s, kb.n * 8, &packed, 1))) return rc;
        HIP_OR_FAIL(launch_hash_varlen_packed(kb, md, (uint64_t *)packed, s));
        if (options().probe_compact) {  // compacted rows (tag 2) from the packed words
            void *rows;
            if ((rc = cached_workspace(s, probe_compact_bytes(kb.n), &rows, 2))) return rc;
            HIP_OR_FAIL(launch_probe_compact_packed((const uint64_t *)packed, kb.n, words, md, out, rows, s));
        } else {
            HIP_OR_FAIL(launch_probe_phased(nullptr, kb.n, words, md, out, (uint64_t *)packed, s));
        }
        return SEB_OK;
    }
    if ((rc = prepare_probe_keys(kb, s, 0, &ws))) return rc;
    if (want_phased(kb.n, md, out) && options().probe_compact) {  // compacted rows in their own scratch (tag 1)
        void *rows;
        if ((rc = cached_workspace(s, probe_compact_bytes(kb.n), &rows, 1))) return rc;
        HIP_OR_FAIL(launch_probe_compact(kb, words, md, out, rows, s));
        return SEB_OK;
    }
    if (want_phased(kb.n, md, out)) {  // packed residues in their own scratch (tag 1)
        void *packed;
        if ((rc = cached_workspace(s, kb.n * 8, &packed, 1))) return rc;
        HIP_OR_FAIL(launch_probe_phased(&kb, kb.n, words, md, out, (uint64_t *)packed, s));
        return SEB_OK;
    }
    HIP_OR_FAIL(launch_probe(kb, words, md, out, s));
    return SEB_OK;
}

extern "C" uint64_t seb_dev_build_workspace_size(uint64_t n, uint64_t m, uint32_t k) {
    enter();
    if (m == 0 || n == 0) return 0;
    // conservative: assumes a variable-length batch (pre-hashed) as well
    const uint64_t pre_b = n >= options().varlen_prehash_min_keys ? ((n * 16 + 255) & ~255ull) : 0;
    const int algo = choose_build_algo(n, m, k);
    return pre_b + (algo == 2 ? bucketed_workspace_bytes(n, m, k) : algo == 4 ? image_workspace_bytes(n, m) : 0);
}

extern "C" int seb_dev_build_ws(const seb_keys *keys, uint32_t *words, uint64_t m, uint32_t k, void *ws,
                                uint64_t ws_bytes, void *stream) {
    enter();
    int rc;
    if ((rc = check_keys(keys, "seb_dev_build_ws")) || (rc = check_filter_args(m, k, "seb_dev_build_ws"))) return rc;
    if (!words) return fail(SEB_ERR_INVALID, "seb_dev_build_ws: null words");
    return build_dispatch(key_batch(keys), words, mod_arg(m, k), (hipStream_t)stream, ws, ws_bytes,
                          [&](uint64_t need, void **) -> int {
                              return fail(SEB_ERR_INVALID, "seb_dev_build_ws: workspace %llu B < %llu B",
                                          (unsigned long long)ws_bytes, (unsigned long long)need);
                          });
}

extern "C" int seb_dev_build(const seb_keys *keys, uint32_t *words, uint64_t m, uint32_t k, void *stream) {
    WsCall ws_call;
    enter();
    int rc;
    if ((rc = check_keys(keys, "seb_dev_build")) || (rc = check_filter_args(m, k, "seb_dev_build"))) return rc;
    if (!words) return fail(SEB_ERR_INVALID, "seb_dev_build: null words");
    hipStream_t s = (hipStream_t)stream;
    return build_dispatch(key_batch(keys), words, mod_arg(m, k), s, nullptr, 0,
                          [&](uint64_t need, void **out) { return cached_workspace(s, need, out); });
}

extern "C" int seb_dev_build_fresh(const seb_keys *keys, uint32_t *words, uint64_t m, uint32_t k, void *stream) {
    WsCall ws_call;
    enter();
    int rc;
    if ((rc = check_keys(keys, "seb_dev_build_fresh")) || (rc = check_filter_args(m, k, "seb_dev_build_fresh")))
        return rc;
    if (!words) return fail(SEB_ERR_INVALID, "seb_dev_build_fresh: null words");
    hipStream_t s = (hipStream_t)stream;
    const KeyBatch kb = key_batch(keys);
    const ModArg md = mod_arg(m, k);
    void *ovf = nullptr;
    if (kb.n && choose_build_algo(kb.n, md.m, md.k) == 2 &&
        (rc = cached_workspace(s, seb_words_bytes(m), &ovf, 4, true)))
        return rc;
    rc = build_dispatch(kb, words, md, s, nullptr, 0,
                        [&](uint64_t need, void **out) { return cached_workspace(s, need, out); }, true,
                        (uint32_t *)ovf);
    if (rc && ovf) ws_discard(s, 4);  // the bitmap may no longer be all zero
    return rc;
}

extern "C" int seb_dev_probe(const seb_keys *keys, const uint32_t *words, uint64_t m, uint32_t k, uint8_t *out,
                             void *stream) {
    WsCall ws_call;
    enter();
    int rc;
    if ((rc = check_keys(keys, "seb_dev_probe")) || (rc = check_filter_args(m, k, "seb_dev_probe"))) return rc;
    if (!words || (!out && keys->n)) return fail(SEB_ERR_INVALID, "seb_dev_probe: null words/out");
    return probe_dispatch(key_batch(keys), words, mod_arg(m, k), out, (hipStream_t)stream);
}

// Packed residues: one 8-byte word per key (r0, b, carry flags) for k == 7 and m < 2^29.
static int check_packed_args(uint64_t m, uint32_t k, const char *who) {
    int rc = check_filter_args(m, k, who);
    if (rc) return rc;
    if (k != 7 || m >= (1ull << kPackBits))
        return fail(SEB_ERR_INVALID, "%s: packed residues need k == 7 and m < 2^%u (k=%u m=%llu)", who, kPackBits, k,
                    (unsigned long long)m);
    return SEB_OK;
}

extern "C" int seb_dev_pack_residues(const seb_keys *keys, uint64_t m, uint32_t k, uint64_t *packed, void *stream) {
    WsCall ws_call;
    enter();
    int rc;
    if ((rc = check_keys(keys, "seb_dev_pack_residues")) || (rc = check_packed_args(m, k, "seb_dev_pack_residues")))
        return rc;
    if (!packed && keys->n) return fail(SEB_ERR_INVALID, "seb_dev_pack_residues: null packed");
    KeyBatch kb = key_batch(keys);
    if (want_prehash_packed(kb, mod_arg(m, k))) {
        HIP_OR_FAIL(launch_hash_varlen_packed(kb, mod_arg(m, k), packed, (hipStream_t)stream));
        return SEB_OK;
    }
    void *ws;
    if ((rc = prepare_probe_keys(kb, (hipStream_t)stream, 0, &ws))) return rc;
    HIP_OR_FAIL(launch_pack_residues(kb, mod_arg(m, k), packed, (hipStream_t)stream));
    return SEB_OK;
}

extern "C" int seb_dev_probe_packed(const uint64_t *packed, uint64_t n, const uint32_t *words, uint64_t m, uint32_t k,
                                    uint8_t *out, void *stream) {
    WsCall ws_call;
    enter();
    int rc = check_packed_args(m, k, "seb_dev_probe_packed");
    if (rc) return rc;
    if (n && (!packed || !words || !out)) return fail(SEB_ERR_INVALID, "seb_dev_probe_packed: null pointer");
    const ModArg md = mod_arg(m, k);
    if (want_phased(n, md, out) && options().probe_compact) {
        void *rows;
        if ((rc = cached_workspace((hipStream_t)stream, probe_compact_bytes(n), &rows, 2))) return rc;
        HIP_OR_FAIL(launch_probe_compact_packed(packed, n, words, md, out, rows, (hipStream_t)stream));
    } else if (want_phased(n, md, out))
        HIP_OR_FAIL(launch_probe_phased(nullptr, n, words, md, out, const_cast<uint64_t *>(packed), (hipStream_t)stream));
    else
        HIP_OR_FAIL(launch_probe_packed(packed, n, words, md, out, (hipStream_t)stream));
    return SEB_OK;
}

// Narrow packed residues: 6 bytes per key in 64-key blocks, for k == 7 and m < 2^21.
static int check_packed6_args(uint64_t m, uint32_t k, const char *who) {
    int rc = check_filter_args(m, k, who);
    if (rc) return rc;
    if (k != 7 || m >= (1ull << kPack6Bits))
        return fail(SEB_ERR_INVALID, "%s: 6-byte packed residues need k == 7 and m < 2^%u (k=%u m=%llu)", who,
                    kPack6Bits, k, (unsigned long long)m);
    return SEB_OK;
}

extern "C" uint64_t seb_packed6_bytes(uint64_t n) { return packed6_bytes(n); }

extern "C" int seb_dev_pack_residues6(const seb_keys *keys, uint64_t m, uint32_t k, void *packed6, void *stream) {
    WsCall ws_call;
    enter();
    int rc;
    if ((rc = check_keys(keys, "seb_dev_pack_residues6")) || (rc = check_packed6_args(m, k, "seb_dev_pack_residues6")))
        return rc;
    if (!packed6 && keys->n) return fail(SEB_ERR_INVALID, "seb_dev_pack_residues6: null packed6");
    if (((uintptr_t)packed6 & 3) != 0) return fail(SEB_ERR_INVALID, "seb_dev_pack_residues6: packed6 not 4-byte aligned");
    KeyBatch kb = key_batch(keys);
    void *ws;
    if ((rc = prepare_probe_keys(kb, (hipStream_t)stream, 0, &ws))) return rc;
    HIP_OR_FAIL(launch_pack_residues6(kb, mod_arg(m, k), (uint8_t *)packed6, (hipStream_t)stream));
    return SEB_OK;
}

extern "C" int seb_dev_probe_emit_packed(const seb_keys *keys, const uint32_t *words, uint64_t m, uint32_t k,
                                         uint8_t *out, uint64_t *packed, void *stream) {
    WsCall ws_call;
    enter();
    int rc;
    if ((rc = check_keys(keys, "seb_dev_probe_emit_packed")) ||
        (rc = check_packed_args(m, k, "seb_dev_probe_emit_packed")))
        return rc;
    if (keys->n && (!words || !out || !packed)) return fail(SEB_ERR_INVALID, "seb_dev_probe_emit_packed: null pointer");
    KeyBatch kb = key_batch(keys);
    const ModArg md = mod_arg(m, k);
    if (want_phased(kb.n, md, out) && want_prehash_packed(kb, md)) {
        HIP_OR_FAIL(launch_hash_varlen_packed(kb, md, packed, (hipStream_t)stream));
        HIP_OR_FAIL(launch_probe_phased(nullptr, kb.n, words, md, out, packed, (hipStream_t)stream));
        return SEB_OK;
    }
    void *ws;
    if ((rc = prepare_probe_keys(kb, (hipStream_t)stream, 0, &ws))) return rc;
    if (want_phased(kb.n, md, out))  // phase 0 writes the packed residues anyway
        HIP_OR_FAIL(launch_probe_phased(&kb, kb.n, words, md, out, packed, (hipStream_t)stream));
    else
        HIP_OR_FAIL(launch_probe_emit(kb, words, md, out, packed, (hipStream_t)stream));
    return SEB_OK;
}

int seb::fill_multi(const seb_filter_ref *filters, uint32_t nf, uint32_t mask_bytes, MultiArg *ma, const char *who) {
    if (!filters || nf == 0) return fail(SEB_ERR_INVALID, "%s: no filters", who);
    if (nf > (uint32_t)kMaxMulti) return fail(SEB_ERR_INVALID, "%s: %u filters > %d", who, nf, kMaxMulti);
    if (!(mask_bytes == 1 || mask_bytes == 2 || mask_bytes == 4 || mask_bytes == 8) || nf > 8 * mask_bytes)
        return fail(SEB_ERR_INVALID, "%s: mask_bytes %u cannot hold %u filters", who, mask_bytes, nf);
    memset(ma, 0, sizeof *ma);
    ma->nf = nf;
    for (uint32_t f = 0; f < nf; ++f) {
        int rc = check_filter_args(filters[f].num_bits, filters[f].num_hashes, who);
        if (rc) return rc;
        if (!filters[f].bits || filters[f].reserved) return fail(SEB_ERR_INVALID, "%s: bad filter %u", who, f);
        ma->f[f].words = (const uint32_t *)filters[f].bits;
        ma->f[f].md = mod_arg(filters[f].num_bits, filters[f].num_hashes);
    }
    return SEB_OK;
}

extern "C" int seb_dev_probe_multi(const seb_keys *keys, const seb_filter_ref *filters, uint32_t nf, void *mask,
                                   uint32_t mask_bytes, void *stream) {
    WsCall ws_call;
    enter();
    int rc;
    MultiArg ma;
    if ((rc = check_keys(keys, "seb_dev_probe_multi")) ||
        (rc = fill_multi(filters, nf, mask_bytes, &ma, "seb_dev_probe_multi")))
        return rc;
    if (!mask && keys->n) return fail(SEB_ERR_INVALID, "seb_dev_probe_multi: null mask");
    hipStream_t s = (hipStream_t)stream;
    KeyBatch kb = key_batch(keys);
    const uint64_t tb = options().multi_interleave && keys->n >= 65536 ? interleaved_bytes(ma, mask_bytes) : 0;
    void *ws = nullptr;
    if ((rc = prepare_probe_keys(kb, s, (tb + 255) & ~255ull, &ws))) return rc;
    if (tb) {
        HIP_OR_FAIL(launch_probe_interleaved(kb, ma, mask, mask_bytes, ws, s));
        return SEB_OK;
    }
    HIP_OR_FAIL(launch_probe_multi(kb, ma, mask, mask_bytes, s));
    return SEB_OK;
}

extern "C" int seb_dev_probe_multi_packed(const uint64_t *packed, uint64_t n, const seb_filter_ref *filters,
                                          uint32_t nf, void *mask, uint32_t mask_bytes, void *stream) {
    WsCall ws_call;
    enter();
    int rc;
    MultiArg ma;
    if ((rc = fill_multi(filters, nf, mask_bytes, &ma, "seb_dev_probe_multi_packed"))) return rc;
    for (uint32_t f = 0; f < nf; ++f)
        if (ma.f[f].md.m != ma.f[0].md.m || ma.f[f].md.k != ma.f[0].md.k)
            return fail(SEB_ERR_INVALID, "seb_dev_probe_multi_packed: filters must share (num_bits, num_hashes)");
    if ((rc = check_packed_args(ma.f[0].md.m, ma.f[0].md.k, "seb_dev_probe_multi_packed"))) return rc;
    if (n && (!packed || !mask)) return fail(SEB_ERR_INVALID, "seb_dev_probe_multi_packed: null pointer");
    if (n == 0) return SEB_OK;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t tb = ((ma.f[0].md.m + 31) / 32) * 32 * mask_bytes;
    void *ws = nullptr;
    if ((rc = cached_workspace(s, (tb + 255) & ~255ull, &ws))) return rc;
    HIP_OR_FAIL(launch_probe_interleaved_packed(packed, n, ma, mask, mask_bytes, ws, s));
    return SEB_OK;
}

extern "C" int seb_dev_probe_multi_packed6(const void *packed6, uint64_t n, const seb_filter_ref *filters,
                                           uint32_t nf, void *mask, uint32_t mask_bytes, void *stream) {
    WsCall ws_call;
    enter();
    int rc;
    MultiArg ma;
    if ((rc = fill_multi(filters, nf, mask_bytes, &ma, "seb_dev_probe_multi_packed6"))) return rc;
    for (uint32_t f = 0; f < nf; ++f)
        if (ma.f[f].md.m != ma.f[0].md.m || ma.f[f].md.k != ma.f[0].md.k)
            return fail(SEB_ERR_INVALID, "seb_dev_probe_multi_packed6: filters must share (num_bits, num_hashes)");
    if ((rc = check_packed6_args(ma.f[0].md.m, ma.f[0].md.k, "seb_dev_probe_multi_packed6"))) return rc;
    if (n && (!packed6 || !mask)) return fail(SEB_ERR_INVALID, "seb_dev_probe_multi_packed6: null pointer");
    if (((uintptr_t)packed6 & 3) != 0)
        return fail(SEB_ERR_INVALID, "seb_dev_probe_multi_packed6: packed6 not 4-byte aligned");
    if (n == 0) return SEB_OK;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t tb = ((ma.f[0].md.m + 31) / 32) * 32 * mask_bytes;
    void *ws = nullptr;
    if ((rc = cached_workspace(s, (tb + 255) & ~255ull, &ws))) return rc;
    HIP_OR_FAIL(launch_probe_interleaved_packed6((const uint8_t *)packed6, n, ma, mask, mask_bytes, ws, s));
    return SEB_OK;
}

extern "C" int seb_dev_or_slices(const uint32_t *slices, uint32_t num_slices, uint64_t slice_words, uint32_t *out,
                                 void *stream) {
    enter();
    if (slice_words && num_slices && (!slices || !out)) return fail(SEB_ERR_INVALID, "seb_dev_or_slices: null pointer");
    HIP_OR_FAIL(launch_or_slices(slices, num_slices, slice_words, out, (hipStream_t)stream));
    return SEB_OK;
}

static const uint32_t kLdsMax = 160 * 1024;

extern "C" int seb_dev_build_many(const seb_keys *keys, const uint64_t *key_begin, const seb_filter_ref *filters,
                                  uint32_t nf, void *stream) {
    enter();
    int rc;
    if ((rc = check_keys(keys, "seb_dev_build_many"))) return rc;
    if (!key_begin || (!filters && nf)) return fail(SEB_ERR_INVALID, "seb_dev_build_many: null arrays");
    hipStream_t s = (hipStream_t)stream;
    KeyBatch kb = key_batch(keys);
    ManyArg ma;
    memset(&ma, 0, sizeof ma);
    uint32_t lds = 0;
    auto flush = [&]() -> int {
        if (ma.nf == 0) return SEB_OK;
        HIP_OR_FAIL(launch_build_many_lds(kb, ma, lds, s));
        memset(&ma, 0, sizeof ma);
        lds = 0;
        return SEB_OK;
    };
    for (uint32_t f = 0; f < nf; ++f) {
        const uint64_t m = filters[f].num_bits;
        const uint32_t k = filters[f].num_hashes;
        if ((rc = check_filter_args(m, k, "seb_dev_build_many"))) return rc;
        if (!filters[f].bits || key_begin[f + 1] < key_begin[f] || key_begin[f + 1] > keys->n)
            return fail(SEB_ERR_INVALID, "seb_dev_build_many: bad filter %u", f);
        const uint64_t wb = seb_words_bytes(m);
        if (wb <= kLdsMax) {
            ManyFilter &F = ma.f[ma.nf++];
            F.words = (uint32_t *)filters[f].bits;
            F.nwords = wb / 4;
            F.key_begin = key_begin[f];
            F.key_end = key_begin[f + 1];
            F.md = mod_arg(m, k);
            lds = std::max<uint32_t>(lds, (uint32_t)wb);
            if (ma.nf == (uint32_t)kMaxMany && (rc = flush())) return rc;
        } else {  // too large for one CU's LDS: grid-wide atomics over this filter's key range
            KeyBatch sub = kb;
            sub.n = key_begin[f + 1] - key_begin[f];
            if (kb.offsets)
                sub.offsets = kb.offsets + key_begin[f];
            else
                sub.data = kb.data + key_begin[f] * (uint64_t)kb.stride;
            HIP_OR_FAIL(launch_build(sub, (uint32_t *)filters[f].bits, mod_arg(m, k), s));
        }
    }
    return flush();
}

extern "C" int seb_dev_alloc(void **ptr, uint64_t bytes) {
    if (!ptr) return fail(SEB_ERR_INVALID, "seb_dev_alloc: null");
    hipError_t e = hipMalloc(ptr, bytes ? bytes : 16);
    if (e != hipSuccess) return (void)hipGetLastError(), fail(SEB_ERR_NOMEM, "hipMalloc(%llu): %s", (unsigned long long)bytes, hipGetErrorString(e));
    return SEB_OK;
}
extern "C" int seb_dev_free(void *ptr) {
    HIP_OR_FAIL(hipFree(ptr));
    return SEB_OK;
}
extern "C" int seb_host_alloc(void **ptr, uint64_t bytes) {
    if (!ptr) return fail(SEB_ERR_INVALID, "seb_host_alloc: null");
    hipError_t e = hipHostMalloc(ptr, bytes ? bytes : 16, hipHostMallocDefault);
    if (e != hipSuccess) return (void)hipGetLastError(), fail(SEB_ERR_NOMEM, "hipHostMalloc(%llu): %s", (unsigned long long)bytes, hipGetErrorString(e));
    return SEB_OK;
}
extern "C" int seb_host_free(void *ptr) {
    HIP_OR_FAIL(hipHostFree(ptr));
    return SEB_OK;
}
extern "C" int seb_memcpy_h2d(void *dst, const void *src, uint64_t bytes, void *stream) {
    HIP_OR_FAIL(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return SEB_OK;
}
extern "C" int seb_memcpy_d2h(void *dst, const void *src, uint64_t bytes, void *stream) {
    HIP_OR_FAIL(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return SEB_OK;
}
extern "C" int seb_stream_sync(void *stream) {
    HIP_OR_FAIL(hipStreamSynchronize((hipStream_t)stream));
    return SEB_OK;
}

// Timing events without the system-scope fence a default HIP event performs when it completes:
// that fence writes back and invalidates L2 and costs ~15 us between two kernels on gfx950
// (profiles/r02_event_gaps), which would inflate the very step it measures.
extern "C" int seb_timer_create(void **ev) {
    if (!ev) return fail(SEB_ERR_INVALID, "seb_timer_create: null");
    hipEvent_t e;
    HIP_OR_FAIL(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
    *ev = (void *)e;
    return SEB_OK;
}

extern "C" int seb_timer_record(void *ev, void *stream) {
    HIP_OR_FAIL(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
    return SEB_OK;
}

extern "C" int seb_timer_elapsed_ms(void *start, void *end, float *ms) {
    if (!ms) return fail(SEB_ERR_INVALID, "seb_timer_elapsed_ms: null");
    HIP_OR_FAIL(hipEventSynchronize((hipEvent_t)end));
    HIP_OR_FAIL(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)end));
    return SEB_OK;
}

extern "C" int seb_timer_destroy(void *ev) {
    if (ev) HIP_OR_FAIL(hipEventDestroy((hipEvent_t)ev));
    return SEB_OK;
}

// ------------------------------------------------ shard routing + WAL checksums (§8(f) row 4)

extern "C" int seb_dev_shard_route(const seb_keys *keys, uint32_t bits, uint16_t *shard, uint32_t *hash,
                                   void *stream) {
    enter();
    int rc;
    if ((rc = check_keys(keys, "seb_dev_shard_route"))) return rc;
    if (bits > 16) return fail(SEB_ERR_INVALID, "seb_dev_shard_route: shard_bits %u > 16", bits);
    HIP_OR_FAIL(launch_route(key_batch(keys), bits, shard, hash, (hipStream_t)stream));
    return SEB_OK;
}

extern "C" uint64_t seb_dev_shard_partition_workspace_size(uint64_t n, uint32_t bits) {
    return bits > 12 ? 0 : route_workspace_bytes(n, bits);
}

extern "C" int seb_dev_shard_partition(const seb_keys *keys, uint32_t bits, uint32_t *perm, uint64_t *shard_begin,
                                       uint16_t *shard, void *ws, uint64_t ws_bytes, void *stream) {
    enter();
    int rc;
    if ((rc = check_keys(keys, "seb_dev_shard_partition"))) return rc;
    if (bits > 12) return fail(SEB_ERR_INVALID, "seb_dev_shard_partition: shard_bits %u > 12", bits);
    if (keys->n >= (1ull << 32)) return fail(SEB_ERR_INVALID, "seb_dev_shard_partition: n >= 2^32");
    if (keys->n && (!perm || !ws)) return fail(SEB_ERR_INVALID, "seb_dev_shard_partition: null perm/workspace");
    if (ws_bytes < route_workspace_bytes(keys->n, bits))
        return fail(SEB_ERR_INVALID, "seb_dev_shard_partition: workspace %llu < %llu bytes",
                    (unsigned long long)ws_bytes, (unsigned long long)route_workspace_bytes(keys->n, bits));
    HIP_OR_FAIL(launch_route_partition(key_batch(keys), bits, perm, shard_begin, shard, ws, ws_bytes,
                                       (hipStream_t)stream));
    return SEB_OK;
}

extern "C" int seb_dev_wal_crc(uint8_t *data, const uint64_t *rec_off, uint64_t n, int mode, uint32_t *crc,
                               uint8_t *ok, void *stream) {
    enter();
    if (mode < SEB_WAL_CRC || mode > SEB_WAL_VERIFY) return fail(SEB_ERR_INVALID, "seb_dev_wal_crc: bad mode %d", mode);
    if (n && (!data || !rec_off)) return fail(SEB_ERR_INVALID, "seb_dev_wal_crc: null data/offsets");
    if (n && mode == SEB_WAL_VERIFY && !ok) return fail(SEB_ERR_INVALID, "seb_dev_wal_crc: VERIFY needs ok[]");
    HIP_OR_FAIL(launch_wal_crc(data, rec_off, n, mode, crc, ok, (hipStream_t)stream));
    return SEB_OK;
}

// ReadAll's framing walk (lsm/wal.go:98-121): a 21-byte header, then keySize + valueSize bytes.
extern "C" int seb_wal_scan(const uint8_t *data, uint64_t bytes, uint64_t *rec_off, uint64_t cap, uint64_t *n) {
    if (!n || (bytes && !data)) return fail(SEB_ERR_INVALID, "seb_wal_scan: null argument");
    *n = 0;
    if (cap < 1 || !rec_off) return fail(SEB_ERR_INVALID, "seb_wal_scan: offsets capacity 0");
    uint64_t at = 0, cnt = 0;
    rec_off[0] = 0;
    while (at < bytes) {
        if (bytes - at < 21) {
            *n = cnt;
            return fail(SEB_ERR_SHORT, "seb_wal_scan: truncated header at byte %llu", (unsigned long long)at);
        }
        uint32_t ks, vs;
        memcpy(&ks, data + at + 12, 4);
        memcpy(&vs, data + at + 16, 4);
        const uint64_t len = 21ull + ks + vs;
        if (bytes - at < len) {
            *n = cnt;
            return fail(SEB_ERR_SHORT, "seb_wal_scan: truncated record at byte %llu", (unsigned long long)at);
        }
        if (cnt + 2 > cap) {
            *n = cnt;
            return fail(SEB_ERR_INVALID, "seb_wal_scan: more than %llu records", (unsigned long long)(cap - 1));
        }
        at += len;
        rec_off[++cnt] = at;
    }
    *n = cnt;
    return SEB_OK;
}
