// seb_host.h — what the host files of the C ABI share (internal, not installed): error reporting,
// the argument checks, the stream workspace, the context with its buffers and chunk loops, and the
// build / probe dispatchers.
//   seb_host.cpp      errors, options, workspace, dispatch, the seb_dev_* bloom entry points, shard + WAL
//   seb_ctx.cpp       contexts, the chunk loops, seb_build / seb_probe / seb_probe_multi
//   seb_stage.h       what the host-buffer forms on a context share (only .cpp files include it): up16, Drain, the section
//                     carver over a DevBuf, the two copy helpers, an op batch, the runs and a sorted run's outputs on the
//                     device (the longer functions: seb_stage.cpp); its first part compiles without HIP
//   seb_filter.cpp    the Go-API filter handle and its CPU fallback
//   seb_registry.cpp  the registry, MultiGet, the index walk and the block locator
//   seb_sstable.cpp   the block-search, SSTable-builder and compaction-merge entry points
//   seb_recover.cpp   the WAL replay's entry points and seb_wal_recover; the memtable lookup's and seb_memtable_get
//   seb_memtable.cpp  the host half of the WAL replay and of the memtable lookup (no HIP dependency; seb_memtable.h)
//   seb_write.cpp     the memtable write side's entry points, seb_memtable_apply and seb_memtable_fold
//   seb_memwrite.cpp  the host half of the memtable write side (no HIP dependency; seb_memwrite.h)
//   seb_memwrite.hip  its kernels: frame, size delta, fold
//   seb_getpath.cpp   the host half of the Get path: compacting undecided keys, the row join (no HIP dependency;
//                     seb_getpath.h); its entry points are in seb_recover.cpp beside the memtable lookup's
//   seb_getpath.hip   its kernels: tile sums, scan, emit, the two join passes (the scan itself: seb_scan.h)
//   seb_blockids.cpp  the host half of the block-id step: located cells into ids of the block pool (no HIP
//                     dependency; seb_blockids.h); its entry points are in seb_sstable.cpp beside seb_blocks_dedup
//   seb_blockids.hip  its kernels: the resident map, the miss pairs' table, flags, scan, rank, emit
//   seb_values.cpp    the host half of the Get path's last step: the found values gathered into one buffer (no HIP
//                     dependency; seb_values.h); its entry points are in seb_recover.cpp beside the Get path's
//   seb_values.hip    its kernels: tile sums, scan, offsets, the copy balanced by output bytes
//   seb_hashindex.cpp the host half of the hash index's read side: segment scan, verify and cuts, Get (no HIP
//                     dependency; seb_hashindex.h)
//   seb_hashindex.hip its kernels: segment CRC, live flags, table insert, Get (the CRC itself: seb_crc.h)
//   seb_hashwrite.cpp the host half of the hash index's write side: frame and cuts, compaction, logical size (no HIP
//                     dependency; seb_hashwrite.h)
//   seb_hashwrite.hip its kernels (the seal: k_seg_crc's seal mode in seb_hashindex.hip; what both share: seb_hidx_dev.h)
//   seb_hidx.cpp      the hash index's entry points, seb_hidx_recover and seb_hidx_compact (their segment walk and sections)
//   seb_btree.h      the B-tree's page codec, page rules and walk: one text for the host half and the kernels
//   seb_btree.cpp    the host half of the B-tree's read side: open, check, Get (no HIP dependency)
//   seb_btree.hip    its kernels: the page check, the level rounds, the counts, Get
//   seb_bt.cpp       the B-tree's entry points and seb_bt_load
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/seb_bloom.h"
#include "seb_kernels.h"

namespace seb {

int params(int64_t n, double p, uint64_t *m_out, uint32_t *k_out);

// ------------------------------------------------------------------ errors ------------------

// The calling thread's last error text (seb_last_error); fail() sets it and returns `code`.
std::string &last_error();
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// The status a failed HIP call maps to.  Only genuine unavailability is SEB_ERR_DEVICE (no device,
// no driver, no code object for it, a runtime that is not up) and only an allocation failure is
// SEB_ERR_NOMEM: those two are what the Go API mirror's CPU fallback absorbs.  Everything else (a
// rejected launch, parameters the library computed wrong, a kernel fault) is SEB_ERR_INTERNAL,
// which is reported and never absorbed, so a library bug cannot hide behind the fallback.
inline int hip_status(hipError_t e) {
    switch (e) {
    case hipErrorOutOfMemory:
        return SEB_ERR_NOMEM;
    case hipErrorNoDevice:
    case hipErrorInvalidDevice:
    case hipErrorInsufficientDriver:
    case hipErrorNoBinaryForGpu:
    case hipErrorNotInitialized:
    case hipErrorDeinitialized:
        return SEB_ERR_DEVICE;
    default:
        return SEB_ERR_INTERNAL;
    }
}

// A failed HIP call is reported through the return code, and HIP's last-error state is cleared so
// it does not surface again in the caller's own later checks (torch's hipGetLastError, say).
#define HIP_OR_FAIL(expr)                                                                              \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            (void)hipGetLastError();                                                                   \
            return seb::fail(seb::hip_status(e_), "%s: %s", #expr, hipGetErrorString(e_));             \
        }                                                                                              \
    } while (0)

// Makes `device` current for one call and restores the caller's device when it returns.
struct DeviceGuard {
    int saved = -1;
    int set(int device) {
        HIP_OR_FAIL(hipGetDevice(&saved));
        if (saved != device) HIP_OR_FAIL(hipSetDevice(device));
        return SEB_OK;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (saved >= 0 && hipGetDevice(&cur) == hipSuccess && cur != saved) (void)hipSetDevice(saved);
    }
};

// ------------------------------------------------------------------ helpers -----------------

// Entry of a call that launches kernels: the knobs are loaded, and HIP's last-error state is
// cleared, so a failed HIP call made earlier on this thread (the caller's, or an allocation the
// library recovered from) is not reported by this call's post-launch hipGetLastError.
void enter();

int check_filter_args(uint64_t m, uint32_t k, const char *who);
int check_keys(const seb_keys *kb, const char *who);
int validate_offsets(const seb_keys *kb, const char *who);
int fill_multi(const seb_filter_ref *filters, uint32_t nf, uint32_t mask_bytes, MultiArg *ma, const char *who);

inline ModArg mod_arg(uint64_t m, uint32_t k) {
    ModArg a{};
    a.m = m;
    a.k = k;
    a.mu = UINT64_MAX / m;
    a.c = (UINT64_MAX % m + 1) % m;  // 2^64 mod m
    return a;
}

inline KeyBatch key_batch(const seb_keys *kb) { return KeyBatch{kb->data, kb->offsets, kb->n, kb->stride}; }

inline bool env_flag(const char *name, long *out) {
    const char *v = getenv(name);
    if (!v || !*v) return false;
    *out = strtol(v, nullptr, 0);
    return true;
}

// ------------------------------------------------------------------ stream workspace --------

// Scope of one ABI call that may use library scratch: slots locked inside it stay locked until
// the call returns (its last launch is enqueued by then).
struct WsCall {
    size_t mark;
    WsCall();
    ~WsCall();
    WsCall(const WsCall &) = delete;
    WsCall &operator=(const WsCall &) = delete;
};

// zero: a new (or regrown) buffer is cleared on the stream before first use (the fresh build's
// overflow bitmap, which its users leave all zero).
int cached_workspace(hipStream_t s, uint64_t bytes, void **out, int tag = 0, bool zero = false);

// A stream about to be destroyed (a context's) gives its scratch back first: otherwise its slot
// would keep a dead handle that a later seb_workspace_release would synchronise on.
void ws_drop_stream(int dev, hipStream_t s);

// ------------------------------------------------------------------ dispatch ----------------

// Build dispatcher: bucketed (LDS, no global atomics), LDS-resident or device-scope atomics;
// large variable-length batches are pre-hashed first.  `ws` / `ws_bytes` may be null/0, in which
// case `grow` supplies scratch.
// fresh: `words` holds nothing yet (a new filter); the image build then writes it without a clear,
// and so does the bucketed build given `ovf` (an all-zero overflow bitmap of seb_words_bytes(m));
// every other path clears it first.
using GrowFn = std::function<int(uint64_t need, void **out)>;
int build_dispatch(KeyBatch kb, uint32_t *words, const ModArg &md, hipStream_t s, void *ws, uint64_t ws_bytes,
                   const GrowFn &grow, bool fresh = false, uint32_t *ovf = nullptr);

int probe_dispatch(KeyBatch kb, const uint32_t *words, const ModArg &md, uint8_t *out, hipStream_t s);

// ------------------------------------------------------- contexts (host-buffer API) ----------

// Grow-only device buffer, freed with its owner (whose device must be current then).
struct DevBuf {
    void *p = nullptr;
    uint64_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    // limited: scratch that workspace_limit_mib caps (a context's build scratch)
    int reserve(uint64_t bytes, bool limited = false) {
        if (bytes <= cap) return SEB_OK;
        const uint64_t lim = options().workspace_limit_mib;
        if (limited && lim && bytes > (lim << 20))
            return fail(SEB_ERR_NOMEM, "workspace %llu B > workspace_limit_mib %llu", (unsigned long long)bytes,
                        (unsigned long long)lim);
        release();
        uint64_t want = std::max<uint64_t>(bytes, 4096);
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) return (void)hipGetLastError(), fail(SEB_ERR_NOMEM, "hipMalloc(%llu): %s", (unsigned long long)want, hipGetErrorString(e));
        cap = want;
        return SEB_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// Grow-only host-pinned buffer (device-accessible), for the small builds' zero-copy path.
struct PinBuf {
    void *p = nullptr;
    void *dev = nullptr;  // the device's address of p
    uint64_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() { release(); }
    int reserve(uint64_t bytes) {
        if (bytes <= cap) return SEB_OK;
        release();
        uint64_t want = std::max<uint64_t>(bytes, 1 << 20);
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e != hipSuccess) {
            p = nullptr;
            return (void)hipGetLastError(), fail(SEB_ERR_NOMEM, "hipHostMalloc(%llu): %s", (unsigned long long)want,
                                                 hipGetErrorString(e));
        }
        if ((e = hipHostGetDevicePointer(&dev, p, 0)) != hipSuccess) {
            release();
            return (void)hipGetLastError(), fail(hip_status(e), "hipHostGetDevicePointer: %s", hipGetErrorString(e));
        }
        cap = want;
        return SEB_OK;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = dev = nullptr;
        cap = 0;
    }
};

}  // namespace seb

struct seb_ctx {
    int device = 0;
    std::mutex mu;
    hipStream_t s_h2d = nullptr, s_comp = nullptr, s_d2h = nullptr;
    hipEvent_t ev_h2d[2] = {}, ev_comp[2] = {}, ev_d2h[2] = {};
    seb::DevBuf keys[2], offs[2], out[2], words, filt, ws;
    seb::DevBuf sb_bid, sb_pool, sb_blen, sb_cells, sb_out;  // seb_search_blocks: its inputs and outputs on the device
    seb::DevBuf sst_in, sst_ws, sst_out;  // seb_sst_build: the run, the plan's workspace, the three sections
    seb::DevBuf mrg_in, mrg_ws, mrg_out;  // seb_merge: pool + blen + counts, the plan's workspace, the five output arrays
    seb::DevBuf rpl_in, rpl_ws, rpl_out;  // seb_wal_recover: image + offsets + ok, the plan's workspace, the six output arrays
    seb::DevBuf mg_runs, mg_out;  // seb_memtable_get: the runs' arrays and indexes, a chunk's six output arrays
    seb::DevBuf mw_in, mw_img, mw_ws, mw_out, mw_runs;  // seb_memtable_apply / _fold: the ops + rec_off + delta, the image,
                                                         // the plan's workspace, the run's six arrays, the runs + indexes
    seb::DevBuf hx_ws;  // seb_hidx_recover: rec_off + seg_first + valid + ok + live; seb_hidx_compact: the same and the plan's
                        // workspace
    seb::PinBuf hkeys, hbits;  // small filter builds: keys in, bits out, read and written by the kernels
    uint64_t chunk_bytes = 64ull << 20;
    std::vector<uint64_t> off_tmp[2];
};

namespace seb {

// Host key batch -> sequence of chunks [i0, i1) whose key bytes fit the chunk budget.
struct Chunk {
    uint64_t i0, i1, byte0, byte1;
};

// The three ways host keys go through a context (c->mu held, c->device current).
//
// Double buffered: chunk j is staged on s_h2d into buffer j & 1, `launch` enqueues on s_comp what
// turns the chunk's device keys into out_per_key bytes per key in `dout`, and s_d2h copies them to
// host_out + i0 * out_per_key; returns with every answer on the host.  single_ok: a batch of one
// chunk runs on s_comp alone (nothing to overlap).
using ChunkLaunch = std::function<int(const KeyBatch &dk, void *dout)>;
int chunks_pipelined(seb_ctx *c, const seb_keys *kb, uint64_t out_per_key, void *host_out, bool single_ok,
                     const ChunkLaunch &launch);

// Serial: a chunk is staged on s_comp, `body` enqueues its copies and launches there, and s_comp is
// synchronised before the next chunk reuses the staging buffers.
using ChunkBody = std::function<int(const KeyBatch &dk, const Chunk &ch)>;
int chunks_serial(seb_ctx *c, const seb_keys *kb, const ChunkBody &body);

// Input only: OR host keys into device words (all on c->s_comp ordering), chunked + double buffered.
int build_device_from_host(seb_ctx *c, const seb_keys *kb, uint32_t *dwords, const ModArg &md, bool fresh = false);

// build_dispatch on s_comp with the context's own build scratch, which grows between launches.
int ctx_build_dispatch(seb_ctx *c, KeyBatch dk, uint32_t *dwords, const ModArg &md, bool fresh);

int probe_device_to_host(seb_ctx *c, const seb_keys *kb, const uint32_t *dwords, const ModArg &md, uint8_t *out);

}  // namespace seb
