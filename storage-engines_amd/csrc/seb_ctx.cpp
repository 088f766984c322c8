// seb_ctx.cpp — contexts (the host-buffer API): three streams and grow-only staging buffers on one
// device, the loops that take a host key batch through them a chunk at a time, and the host-buffer
// bloom entry points seb_build / seb_probe / seb_probe_multi.
#include "seb_host.h"

using namespace seb;

// ------------------------------------------------------- contexts (host-buffer API) ----------

extern "C" int seb_ctx_create(int device, seb_ctx **out) {
    if (!out) return fail(SEB_ERR_INVALID, "seb_ctx_create: null out");
    int rc = seb_device_check(device);
    if (rc) return rc;
    HIP_OR_FAIL(hipSetDevice(device));
    seb_ctx *c = new seb_ctx();
    c->device = device;
    long cb;
    if (env_flag("SEB_CHUNK_BYTES", &cb) && cb > 0) c->chunk_bytes = (uint64_t)cb;
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->s_h2d, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->s_comp, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->s_d2h, hipStreamNonBlocking);
    for (int b = 0; b < 2 && e == hipSuccess; ++b) {
        e = hipEventCreateWithFlags(&c->ev_h2d[b], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_comp[b], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_d2h[b], hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        seb_ctx_destroy(c);
        return fail(hip_status(e), "seb_ctx_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return SEB_OK;
}

// What must be ordered is done here; the buffers go with the context (DevBuf, PinBuf).
extern "C" void seb_ctx_destroy(seb_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->s_comp) (void)hipStreamSynchronize(c->s_comp);
    for (int b = 0; b < 2; ++b) {
        if (c->ev_h2d[b]) (void)hipEventDestroy(c->ev_h2d[b]);
        if (c->ev_comp[b]) (void)hipEventDestroy(c->ev_comp[b]);
        if (c->ev_d2h[b]) (void)hipEventDestroy(c->ev_d2h[b]);
    }
    for (hipStream_t st : {c->s_h2d, c->s_comp, c->s_d2h})
        if (st) ws_drop_stream(c->device, st);
    if (c->s_h2d) (void)hipStreamDestroy(c->s_h2d);
    if (c->s_comp) (void)hipStreamDestroy(c->s_comp);
    if (c->s_d2h) (void)hipStreamDestroy(c->s_d2h);
    delete c;
}

static void plan_chunks(const seb_keys *kb, uint64_t budget, std::vector<Chunk> &out) {
    out.clear();
    const uint64_t n = kb->n;
    if (n == 0) return;
    if (!kb->offsets) {
        uint64_t per = kb->stride ? std::max<uint64_t>(1, budget / kb->stride) : n;
        for (uint64_t i = 0; i < n; i += per) {
            uint64_t j = std::min(n, i + per);
            out.push_back({i, j, i * kb->stride, j * kb->stride});
        }
        return;
    }
    const uint64_t *o = kb->offsets;
    uint64_t i = 0;
    while (i < n) {
        // largest j with o[j] - o[i] <= budget (at least one key)
        uint64_t lo = i + 1, hi = n;
        while (lo < hi) {
            uint64_t mid = lo + (hi - lo + 1) / 2;
            if (o[mid] - o[i] <= budget) lo = mid; else hi = mid - 1;
        }
        out.push_back({i, lo, o[i], o[lo]});
        i = lo;
    }
}

// Stage one chunk of host keys into buffer b on s_h2d; returns the device KeyBatch for it.  A batch
// of one chunk is copied on s_comp itself: nothing to overlap, and a cross-stream event wait
// costs ~17 us before the kernel may start (profiles/r03_flush_trace.txt).
static int stage_chunk(seb_ctx *c, const seb_keys *kb, const Chunk &ch, int b, KeyBatch *dk, bool single) {
    int rc;
    const uint64_t bytes = ch.byte1 - ch.byte0;
    if ((rc = c->keys[b].reserve(bytes + 16))) return rc;
    hipStream_t cs = single ? c->s_comp : c->s_h2d;
    if (!single) HIP_OR_FAIL(hipStreamWaitEvent(c->s_h2d, c->ev_comp[b], 0));  // buffer b no longer read
    if (bytes) HIP_OR_FAIL(hipMemcpyAsync(c->keys[b].p, kb->data + ch.byte0, bytes, hipMemcpyHostToDevice, cs));
    dk->n = ch.i1 - ch.i0;
    dk->stride = kb->stride;
    if (kb->offsets) {
        const uint64_t cnt = dk->n + 1;
        if ((rc = c->offs[b].reserve(cnt * 8))) return rc;
        HIP_OR_FAIL(hipMemcpyAsync(c->offs[b].p, kb->offsets + ch.i0, cnt * 8, hipMemcpyHostToDevice, cs));
        dk->offsets = (const uint64_t *)c->offs[b].p;
        dk->data = (const uint8_t *)c->keys[b].p - ch.byte0;  // offsets are absolute
    } else {
        dk->offsets = nullptr;
        dk->data = (const uint8_t *)c->keys[b].p;
    }
    if (single) return SEB_OK;
    HIP_OR_FAIL(hipEventRecord(c->ev_h2d[b], c->s_h2d));
    HIP_OR_FAIL(hipStreamWaitEvent(c->s_comp, c->ev_h2d[b], 0));
    return SEB_OK;
}

int seb::ctx_build_dispatch(seb_ctx *c, KeyBatch dk, uint32_t *dwords, const ModArg &md, bool fresh) {
    return build_dispatch(dk, dwords, md, c->s_comp, c->ws.p, c->ws.cap, [c](uint64_t need, void **out) -> int {
        HIP_OR_FAIL(hipStreamSynchronize(c->s_comp));  // previous chunks may still use it
        int r = c->ws.reserve(need, true);
        *out = c->ws.p;
        return r;
    }, fresh);
}

int seb::build_device_from_host(seb_ctx *c, const seb_keys *kb, uint32_t *dwords, const ModArg &md, bool fresh) {
    std::vector<Chunk> chunks;
    plan_chunks(kb, c->chunk_bytes, chunks);
    for (size_t j = 0; j < chunks.size(); ++j) {
        const int b = (int)(j & 1);
        KeyBatch dk{};
        int rc = stage_chunk(c, kb, chunks[j], b, &dk, chunks.size() == 1);
        if (rc) return rc;
        if ((rc = ctx_build_dispatch(c, dk, dwords, md, fresh && j == 0))) return rc;
        HIP_OR_FAIL(hipEventRecord(c->ev_comp[b], c->s_comp));
    }
    return SEB_OK;
}

int seb::chunks_pipelined(seb_ctx *c, const seb_keys *kb, uint64_t out_per_key, void *host_out, bool single_ok,
                          const ChunkLaunch &launch) {
    std::vector<Chunk> chunks;
    plan_chunks(kb, c->chunk_bytes, chunks);
    const bool single = single_ok && chunks.size() == 1;  // copy in, launch, copy out on s_comp alone
    for (size_t j = 0; j < chunks.size(); ++j) {
        const int b = (int)(j & 1);
        KeyBatch dk{};
        int rc = stage_chunk(c, kb, chunks[j], b, &dk, single);
        if (rc) return rc;
        const uint64_t bytes = dk.n * out_per_key;
        uint8_t *dst = (uint8_t *)host_out + chunks[j].i0 * out_per_key;
        if ((rc = c->out[b].reserve(bytes))) return rc;
        if (!single) HIP_OR_FAIL(hipStreamWaitEvent(c->s_comp, c->ev_d2h[b], 0));  // out[b] drained
        if ((rc = launch(dk, c->out[b].p))) return rc;
        if (single) {
            HIP_OR_FAIL(hipMemcpyAsync(dst, c->out[b].p, bytes, hipMemcpyDeviceToHost, c->s_comp));
            HIP_OR_FAIL(hipStreamSynchronize(c->s_comp));
            return SEB_OK;
        }
        HIP_OR_FAIL(hipEventRecord(c->ev_comp[b], c->s_comp));
        HIP_OR_FAIL(hipStreamWaitEvent(c->s_d2h, c->ev_comp[b], 0));
        HIP_OR_FAIL(hipMemcpyAsync(dst, c->out[b].p, bytes, hipMemcpyDeviceToHost, c->s_d2h));
        HIP_OR_FAIL(hipEventRecord(c->ev_d2h[b], c->s_d2h));
    }
    HIP_OR_FAIL(hipStreamSynchronize(c->s_d2h));
    return SEB_OK;
}

int seb::chunks_serial(seb_ctx *c, const seb_keys *kb, const ChunkBody &body) {
    std::vector<Chunk> chunks;
    plan_chunks(kb, c->chunk_bytes, chunks);
    for (const Chunk &ch : chunks) {
        KeyBatch dk{};
        int rc;
        if ((rc = stage_chunk(c, kb, ch, 0, &dk, true)) || (rc = body(dk, ch))) return rc;
        HIP_OR_FAIL(hipStreamSynchronize(c->s_comp));  // the staging buffers are reused by the next chunk
    }
    return SEB_OK;
}

int seb::probe_device_to_host(seb_ctx *c, const seb_keys *kb, const uint32_t *dwords, const ModArg &md, uint8_t *out) {
    return chunks_pipelined(c, kb, 1, out, true, [&](const KeyBatch &dk, void *dout) {
        return probe_dispatch(dk, dwords, md, (uint8_t *)dout, c->s_comp);
    });
}

extern "C" int seb_build(seb_ctx *c, const seb_keys *kb, uint8_t *bits, uint64_t m, uint32_t k, uint32_t flags) {
    int rc;
    if (!c) return fail(SEB_ERR_INVALID, "seb_build: null ctx");
    if ((rc = check_keys(kb, "seb_build")) || (rc = check_filter_args(m, k, "seb_build")) ||
        (rc = validate_offsets(kb, "seb_build")))
        return rc;
    if (!bits) return fail(SEB_ERR_INVALID, "seb_build: null bits");
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OR_FAIL(hipSetDevice(c->device));
    const uint64_t wb = seb_words_bytes(m), nb = seb_num_bytes(m);
    if ((rc = c->words.reserve(wb))) return rc;
    uint32_t *dw = (uint32_t *)c->words.p;
    HIP_OR_FAIL(hipMemsetAsync(dw, 0, wb, c->s_comp));
    if (!(flags & SEB_BUILD_FRESH)) HIP_OR_FAIL(hipMemcpyAsync(dw, bits, nb, hipMemcpyHostToDevice, c->s_comp));
    if ((rc = build_device_from_host(c, kb, dw, mod_arg(m, k)))) return rc;
    HIP_OR_FAIL(hipMemcpyAsync(bits, dw, nb, hipMemcpyDeviceToHost, c->s_comp));
    HIP_OR_FAIL(hipStreamSynchronize(c->s_comp));
    return SEB_OK;
}

extern "C" int seb_probe(seb_ctx *c, const seb_keys *kb, const uint8_t *bits, uint64_t m, uint32_t k, uint8_t *out) {
    WsCall ws_call;
    int rc;
    if (!c) return fail(SEB_ERR_INVALID, "seb_probe: null ctx");
    if ((rc = check_keys(kb, "seb_probe")) || (rc = check_filter_args(m, k, "seb_probe")) ||
        (rc = validate_offsets(kb, "seb_probe")))
        return rc;
    if (!bits || (!out && kb->n)) return fail(SEB_ERR_INVALID, "seb_probe: null bits/out");
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OR_FAIL(hipSetDevice(c->device));
    const uint64_t wb = seb_words_bytes(m), nb = seb_num_bytes(m);
    if ((rc = c->words.reserve(wb))) return rc;
    uint32_t *dw = (uint32_t *)c->words.p;
    HIP_OR_FAIL(hipMemsetAsync(dw, 0, wb, c->s_comp));
    HIP_OR_FAIL(hipMemcpyAsync(dw, bits, nb, hipMemcpyHostToDevice, c->s_comp));
    return probe_device_to_host(c, kb, dw, mod_arg(m, k), out);
}

extern "C" int seb_probe_multi(seb_ctx *c, const seb_keys *kb, const seb_filter_ref *filters, uint32_t nf,
                               uint64_t *mask) {
    int rc;
    if (!c) return fail(SEB_ERR_INVALID, "seb_probe_multi: null ctx");
    if ((rc = check_keys(kb, "seb_probe_multi")) || (rc = validate_offsets(kb, "seb_probe_multi"))) return rc;
    if (!mask && kb->n) return fail(SEB_ERR_INVALID, "seb_probe_multi: null mask");
    if (!filters || nf == 0 || nf > (uint32_t)kMaxMulti) return fail(SEB_ERR_INVALID, "seb_probe_multi: bad filter count");
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OR_FAIL(hipSetDevice(c->device));
    uint64_t total = 0;
    std::vector<uint64_t> at(nf);
    for (uint32_t f = 0; f < nf; ++f) {
        if ((rc = check_filter_args(filters[f].num_bits, filters[f].num_hashes, "seb_probe_multi"))) return rc;
        if (!filters[f].bits) return fail(SEB_ERR_INVALID, "seb_probe_multi: null bits %u", f);
        at[f] = total;
        total += seb_words_bytes(filters[f].num_bits);
    }
    if ((rc = c->filt.reserve(total))) return rc;
    HIP_OR_FAIL(hipMemsetAsync(c->filt.p, 0, total, c->s_comp));
    std::vector<seb_filter_ref> dref(filters, filters + nf);
    for (uint32_t f = 0; f < nf; ++f) {
        uint8_t *d = (uint8_t *)c->filt.p + at[f];
        HIP_OR_FAIL(hipMemcpyAsync(d, filters[f].bits, seb_num_bytes(filters[f].num_bits), hipMemcpyHostToDevice, c->s_comp));
        dref[f].bits = d;
    }
    MultiArg ma;
    if ((rc = fill_multi(dref.data(), nf, 8, &ma, "seb_probe_multi"))) return rc;
    return chunks_pipelined(c, kb, 8, mask, false, [&](const KeyBatch &dk, void *dout) -> int {
        HIP_OR_FAIL(launch_probe_multi(dk, ma, dout, 8, c->s_comp));
        return SEB_OK;
    });
}
