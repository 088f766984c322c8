// seb_stage.h — the staging the host-buffer forms on a seb_ctx share (internal; only .cpp files include it): the 16-byte
// sections a DevBuf is carved into, the copies in and out of them, an op batch, the runs and a sorted run's outputs on the
// device.  The first part is arithmetic alone and compiles without HIP (SEB_STAGE_NO_HIP: tools/sanitize/stage_check.cpp).
#pragma once
#include <cstdint>

#include "../../include/seb_bloom.h"

namespace seb {

inline uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

uint64_t run_index_bytes(uint64_t n);  // seb_kernels.h

// Sections of one device buffer, taken in order, each 16-byte aligned.  A section of no bytes (an absent array) is
// legal and takes no room; bytes() is what the buffer must hold for the sections taken so far.
struct Carver {
    uint64_t at = 0;
    uint64_t take(uint64_t bytes) { return (at += up16(bytes)) - up16(bytes); }
    uint64_t bytes() const { return at; }
};

// The six arrays of a sorted run on the device, in one buffer (with_seq: the run has sequences)
struct RunOut {
    uint64_t key_bytes, val_bytes, n;
    uint64_t keys, koff, vals, voff, del, seq, bytes;
    RunOut(uint64_t key_bytes_, uint64_t val_bytes_, uint64_t n_, bool with_seq = true)
        : key_bytes(key_bytes_), val_bytes(val_bytes_), n(n_) {
        Carver c;
        keys = c.take(key_bytes), koff = c.take(8 * (n + 1)), vals = c.take(val_bytes), voff = c.take(8 * (n + 1));
        del = c.take(n), seq = c.take(with_seq ? 8 * n : 0), bytes = c.bytes();
    }
};

// A host run's sections, in this order; `val_bytes` of values (0: they stay on the host).  An absent array takes no room.
struct RunSections { uint64_t keys, key_off, val_off, deleted, seq, vals, index; };
inline RunSections run_sections(Carver &c, const seb_run &u, uint64_t val_bytes) {
    return {c.take(u.keys ? u.key_bytes : 0), c.take(u.key_off ? 8 * (u.n + 1) : 0), c.take(u.val_off ? 8 * (u.n + 1) : 0),
            c.take(u.deleted ? u.n : 0),      c.take(u.seq ? 8 * u.n : 0),           c.take(val_bytes),
            c.take(run_index_bytes(u.n))};
}

// What runs_upload carves (val_bytes null: no values go up); an empty run takes nothing
inline uint64_t runs_upload_bytes(const seb_run *runs, const uint64_t *val_bytes, uint32_t num_runs) {
    Carver c;
    for (uint32_t r = 0; r < num_runs; ++r)
        if (runs[r].n) run_sections(c, runs[r], val_bytes ? val_bytes[r] : 0);
    return c.bytes() < 16 ? 16 : c.bytes();
}

}  // namespace seb

#ifndef SEB_STAGE_NO_HIP
#include "seb_host.h"

namespace seb {

// The caller's arrays and the frame's vectors are read and written by asynchronous copies: whichever way a frame is left,
// they are waited for.  Declared after the context's lock (the stream drains first) and after the vectors the copies use.
struct Drain {
    hipStream_t s;
    ~Drain() { (void)hipStreamSynchronize(s); }
};

inline uint8_t *section(const DevBuf &b, uint64_t off) { return (uint8_t *)b.p + off; }

// A host array into a section: a null source or no bytes, no copy; with dev, *dev = the section, null for a null source
inline int upload(uint8_t *at, const void *src, uint64_t bytes, hipStream_t s) {
    if (src && bytes) HIP_OR_FAIL(hipMemcpyAsync(at, src, bytes, hipMemcpyHostToDevice, s));
    return SEB_OK;
}
template <typename T>
int upload(const T **dev, uint8_t *at, const void *src, uint64_t bytes, hipStream_t s) {
    *dev = src ? (const T *)at : nullptr;
    return upload(at, src, bytes, s);
}
// A section into a host array: a null destination or no bytes, no copy
inline int download(void *dst, const void *at, uint64_t bytes, hipStream_t s) {
    if (dst && bytes) HIP_OR_FAIL(hipMemcpyAsync(dst, at, bytes, hipMemcpyDeviceToHost, s));
    return SEB_OK;
}

// An op batch (n != 0) on the device: key bytes, key offsets, value bytes, value offsets, deleted bytes.  The ops' byte
// ranges [k0, k1) and [v0, v1) go up as they are and the device pointers are set back by the first offset, so the
// offsets stay absolute.  carve() takes the sections, upload() copies and sets keys / vals / val_off / deleted.
struct OpsOnDevice {
    uint64_t k0, k1, v0, v1;
    uint64_t a_keys = 0, a_koff = 0, a_vals = 0, a_voff = 0, a_del = 0;
    seb_keys keys = {};
    const uint8_t *vals = nullptr, *deleted = nullptr;
    const uint64_t *val_off = nullptr;
    OpsOnDevice(const seb_keys *kb, const uint64_t *hval_off)
        : k0(kb->offsets ? kb->offsets[0] : 0), k1(kb->offsets ? kb->offsets[kb->n] : kb->n * (uint64_t)kb->stride),
          v0(hval_off[0]), v1(hval_off[kb->n]) {}
    void carve(Carver &c, const seb_keys *kb, bool has_deleted) {
        a_keys = c.take(k1 - k0), a_koff = c.take(kb->offsets ? 8 * (kb->n + 1) : 0), a_vals = c.take(v1 - v0);
        a_voff = c.take(8 * (kb->n + 1)), a_del = c.take(has_deleted ? kb->n : 0);
    }
    int upload(uint8_t *base, const seb_keys *kb, const uint8_t *hvals, const uint64_t *hval_off, const uint8_t *hdeleted,
               hipStream_t s);
};

// Host runs in one device buffer of runs_upload_bytes, each run's index built and checked on the device; vals and
// val_bytes given: the values too.  drun / dindex / dvals: num_runs each.
struct RunUpload {
    seb_run drun[SEB_MEM_MAX_RUNS] = {};
    const void *dindex[SEB_MEM_MAX_RUNS] = {};
    const uint8_t *dvals[SEB_MEM_MAX_RUNS] = {};
};
int runs_upload(const seb_run *runs, const uint8_t *const *vals, const uint64_t *val_bytes, uint32_t num_runs, uint8_t *base,
                RunUpload *up, hipStream_t s, const char *who);

// 0, -1 (a null argument, or more than max_runs runs) or -5 (*bad_run has 2^32 entries or more): the caller's words
int check_host_runs(const seb_run *runs, uint32_t num_runs, uint32_t max_runs, uint32_t *bad_run);

// The caller's arrays for a sorted run and their capacities, in the forms' argument order (seq null: none wanted)
struct RunDst {
    uint8_t *keys;
    uint64_t key_cap, *key_off;
    uint8_t *vals;
    uint64_t val_cap, *val_off;
    uint8_t *deleted;
    uint64_t *seq, entry_cap;
};

// A plan's sizes against the capacities (SEB_ERR_RANGE: the caller retries with the sizes), then the arrays the
// sizes need.  image_bytes given: the call also returns an image of that many bytes.
int check_run_dst(const char *who, const RunDst &d, uint64_t entries, uint64_t key_bytes, uint64_t val_bytes,
                  const uint64_t *image_bytes = nullptr, uint64_t image_cap = 0, const uint8_t *image = nullptr);

int run_download(const uint8_t *o, const RunOut &at, const RunDst &d, hipStream_t s);

}  // namespace seb
#endif
