// seb_registry.cpp — the device-resident filter registry: Put / Remove, the batched MultiGet in its
// device and host-pointer forms, the files' sparse indexes and the batched block locator.
#include <atomic>

#include "seb_host.h"

using namespace seb;

// --------------------------------- device-resident filter registry + batched MultiGet --------
// SURVEY.md §8(f) rows 1-2.  Each SSTable's bloom block (its Encode() bytes, read at
// lsm/sstable.go:121-129) is decoded straight into HBM once; the level layout mirrors
// lsm/levels.go: level 0 in insertion order (AddSSTable appends, :53), levels 1..4 sorted by
// MinKey (:56-60; ties keep insertion order).  seb_registry_multiget answers, for a whole key
// batch, which registered files LSM.Get would consult and which of their filters may contain the
// key (lsm/lsm.go:168-198).

struct RegEntry {
    uint64_t file_num = 0, seq = 0;
    int level = 0;
    uint32_t slot = 0;
    uint64_t m = 0;
    uint32_t k = 0;
    uint32_t *dwords = nullptr;
    std::string min_key, max_key;
    // the file's sparse index (seb_registry_put_index): one device block holding the LocSlot arrays
    bool has_index = false;
    void *dindex = nullptr;
    LocSlot loc{};
};

struct seb_registry {
    std::mutex mu;
    int device = 0;
    std::vector<RegEntry> entries;
    uint64_t seq = 0;
    bool dirty = true;
    DevBuf dslots, dranges;
    DevBuf dl0;                    // the L0 group's interleaved table (RegLayout::l0tab)
    DevBuf dbrange;                // per partition bucket, each disjoint level's bisection range (MgSeg::brange)
    DevBuf dloc;                   // the locator's table: one LocSlot per slot id below max_slot
    DevBuf dcand, dblocks;         // the host-pointer locator's candidate rows and block offsets
    bool has_brange = false;
    uint32_t nslots = 0;
    uint32_t max_cand = 0;         // longest Get walk: every L0 file + one file per non-empty level 1..4
    uint32_t max_slot = 0;         // 1 + the largest slot id in use (the mask form needs <= 64)
    uint32_t part_lo = 0, part_hi = 0;  // multiget_order's partition level: lookup-ordered slots [lo, hi)
    RegLayout layout{};
    seb_ctx *ctx = nullptr;
};

static void be_prefix(const std::string &s, uint64_t out[2]) {  // first 16 bytes, big-endian, zero padded
    for (int w = 0; w < 2; ++w) {
        uint64_t v = 0;
        for (int i = 0; i < 8; ++i) {
            const size_t at = (size_t)w * 8 + i;
            v = (v << 8) | (at < s.size() ? (uint8_t)s[at] : 0u);
        }
        out[w] = v;
    }
}

extern "C" seb_registry *seb_registry_new(int device) {
    seb_registry *r = new (std::nothrow) seb_registry();
    if (!r) return nullptr;
    r->device = device;
    return r;
}

extern "C" void seb_registry_free(seb_registry *r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    for (auto &e : r->entries) {
        (void)hipFree(e.dwords);
        if (e.dindex) (void)hipFree(e.dindex);
    }
    if (r->ctx) seb_ctx_destroy(r->ctx);
    delete r;
}

// r->mu held.
static RegEntry *find_entry(seb_registry *r, uint64_t file_num) {
    for (auto &e : r->entries)
        if (e.file_num == file_num) return &e;
    return nullptr;
}

extern "C" int seb_registry_put(seb_registry *r, uint64_t file_num, int level, const uint8_t *bloom, uint64_t bloom_len,
                                const uint8_t *min_key, uint64_t min_len, const uint8_t *max_key, uint64_t max_len) {
    if (!r || !bloom || (!min_key && min_len) || (!max_key && max_len))
        return fail(SEB_ERR_INVALID, "seb_registry_put: null argument");
    if (level < 0 || level > 4) return fail(SEB_ERR_INVALID, "seb_registry_put: level %d outside 0..4", level);
    if (bloom_len < 12) return fail(SEB_ERR_INVALID, "seb_registry_put: bloom block < 12 bytes (DecodeBloomFilter: nil)");
    uint64_t m = 0;
    uint32_t k = 0;
    for (int b = 0; b < 8; ++b) m |= (uint64_t)bloom[b] << (8 * b);
    for (int b = 0; b < 4; ++b) k |= (uint32_t)bloom[8 + b] << (8 * b);
    int rc = check_filter_args(m, k, "seb_registry_put");
    if (rc) return rc;
    if (bloom_len - 12 < seb_num_bytes(m)) return fail(SEB_ERR_SHORT, "seb_registry_put: bits shorter than ceil(m/8)");
    std::lock_guard<std::mutex> g(r->mu);
    if (find_entry(r, file_num))
        return fail(SEB_ERR_INVALID, "seb_registry_put: file %llu already registered", (unsigned long long)file_num);
    if (r->entries.size() >= kRegMaxFiles)
        return fail(SEB_ERR_INVALID, "seb_registry_put: registry holds at most %u files", kRegMaxFiles);
    std::vector<char> used(kRegMaxFiles, 0);
    for (auto &e : r->entries) used[e.slot] = 1;
    uint32_t slot = 0;  // lowest free slot: a registry of <= 64 files keeps every slot < 64 (mask form)
    while (used[slot]) ++slot;
    HIP_OR_FAIL(hipSetDevice(r->device));
    RegEntry e;
    e.file_num = file_num;
    e.seq = r->seq++;
    e.level = level;
    e.slot = slot;
    e.m = m;
    e.k = k;
    e.min_key.assign((const char *)min_key, min_len);
    e.max_key.assign((const char *)max_key, max_len);
    const uint64_t wb = seb_words_bytes(m);
    hipError_t a = hipMalloc((void **)&e.dwords, wb);
    if (a != hipSuccess) return (void)hipGetLastError(), fail(SEB_ERR_NOMEM, "seb_registry_put: hipMalloc: %s", hipGetErrorString(a));
    HIP_OR_FAIL(hipMemset(e.dwords, 0, wb));
    HIP_OR_FAIL(hipMemcpy(e.dwords, bloom + 12, seb_num_bytes(m), hipMemcpyHostToDevice));
    r->entries.push_back(std::move(e));
    r->dirty = true;
    return (int)slot;
}

extern "C" int seb_registry_remove(seb_registry *r, uint64_t file_num) {
    if (!r) return fail(SEB_ERR_INVALID, "seb_registry_remove: null registry");
    std::lock_guard<std::mutex> g(r->mu);
    RegEntry *e = find_entry(r, file_num);
    if (!e) return fail(SEB_ERR_INVALID, "seb_registry_remove: file %llu not registered", (unsigned long long)file_num);
    HIP_OR_FAIL(hipSetDevice(r->device));
    HIP_OR_FAIL(hipDeviceSynchronize());  // no multiget may still read it
    HIP_OR_FAIL(hipFree(e->dwords));
    if (e->dindex) HIP_OR_FAIL(hipFree(e->dindex));
    r->entries.erase(r->entries.begin() + (e - r->entries.data()));
    r->dirty = true;
    return SEB_OK;
}

// Lookup order: level 0 by insertion, then each level 1..4 by (MinKey, insertion).
static std::vector<const RegEntry *> lookup_order(const seb_registry *r) {
    std::vector<const RegEntry *> v;
    for (auto &e : r->entries) v.push_back(&e);
    std::stable_sort(v.begin(), v.end(), [](const RegEntry *a, const RegEntry *b) {
        if (a->level != b->level) return a->level < b->level;
        if (a->level > 0 && a->min_key != b->min_key) return a->min_key < b->min_key;
        return a->seq < b->seq;
    });
    return v;
}

static int sync_registry_locked(seb_registry *r) {
    if (!r->dirty) return SEB_OK;
    HIP_OR_FAIL(hipSetDevice(r->device));
    auto order = lookup_order(r);
    std::vector<RegSlot> slots;
    std::string ranges;
    RegLayout lay{};
    lay.all_k7_m32 = 1;
    for (int L = 0; L < 5; ++L) lay.lo[L] = lay.hi[L] = 0;
    for (size_t i = 0; i < order.size(); ++i) {
        const int L = order[i]->level;
        if (i == 0 || order[i - 1]->level != L) lay.lo[L] = (uint32_t)i;
        lay.hi[L] = (uint32_t)i + 1;
        if (order[i]->k != 7 || order[i]->m >= kM32Limit) lay.all_k7_m32 = 0;
    }
    for (int L = 0; L < 5; ++L)
        if (lay.hi[L] == 0) lay.lo[L] = lay.hi[L] = (uint32_t)order.size();  // empty level
    for (int L = 1; L < 5; ++L) {  // disjoint, MinKey-ordered level: bisection finds the first cover
        bool ok = true;
        for (uint32_t i = lay.lo[L]; i + 1 < lay.hi[L]; ++i)
            ok &= order[i]->min_key <= order[i]->max_key && order[i]->max_key < order[i + 1]->min_key;
        if (lay.hi[L] > lay.lo[L]) ok &= order[lay.hi[L] - 1]->min_key <= order[lay.hi[L] - 1]->max_key;
        if (ok) lay.nonoverlap |= 1u << L;
    }
    for (const RegEntry *e : order) {
        RegSlot s{};
        s.words = e->dwords;
        s.md = mod_arg(e->m, e->k);
        s.min_off = (uint32_t)ranges.size();
        s.min_len = (uint32_t)e->min_key.size();
        ranges += e->min_key;
        s.max_off = (uint32_t)ranges.size();
        s.max_len = (uint32_t)e->max_key.size();
        ranges += e->max_key;
        s.level = e->level;
        s.slot = e->slot;
        s.gbit = -1;
        be_prefix(e->min_key, s.min_be);
        be_prefix(e->max_key, s.max_be);
        slots.push_back(s);
    }
    // L0 group: the largest set of L0 files sharing (m, k) (flushes of equal-sized memtables do;
    // MaxL0Files = 4, lsm/levels.go:9), at most kL0GroupMax, tested through one interleaved table
    std::vector<uint32_t> grp;
    for (uint32_t i = lay.lo[0]; i < lay.hi[0]; ++i) {
        std::vector<uint32_t> same;
        for (uint32_t j = lay.lo[0]; j < lay.hi[0] && same.size() < kL0GroupMax; ++j)
            if (order[j]->m == order[i]->m && order[j]->k == order[i]->k) same.push_back(j);
        if (same.size() > grp.size()) grp = same;
    }
    if (grp.size() < 2) grp.clear();
    uint32_t gbits = 2;
    while (gbits < grp.size()) gbits *= 2;
    int rc;
    uint32_t max_slot = 0;
    for (const RegEntry *e : order) max_slot = std::max(max_slot, e->slot + 1);
    std::vector<LocSlot> loc(max_slot);  // by slot id; free slots and files without an index stay all zero
    for (const RegEntry *e : order)
        if (e->has_index) loc[e->slot] = e->loc;
    if ((rc = r->dloc.reserve(sizeof(LocSlot) * (loc.size() + 1)))) return rc;
    if ((rc = r->dslots.reserve(sizeof(RegSlot) * (slots.size() + 1))) ||
        (rc = r->dranges.reserve(ranges.size() + 16)) ||
        (!grp.empty() && (rc = r->dl0.reserve(4 * l0_table_words(order[grp[0]]->m, gbits) + 16))))
        return rc;
    HIP_OR_FAIL(hipDeviceSynchronize());  // previous multigets may still read the tables
    lay.l0g = 0;
    if (!grp.empty()) {
        L0Members mem{};
        for (uint32_t f = 0; f < grp.size(); ++f) {
            mem.w[f] = order[grp[f]]->dwords;
            slots[grp[f]].gbit = (int32_t)f;
        }
        const RegEntry *g0 = order[grp[0]];
        HIP_OR_FAIL(launch_l0_table(mem, (uint32_t)grp.size(), gbits, g0->m, (uint32_t *)r->dl0.p, nullptr));
        HIP_OR_FAIL(hipStreamSynchronize(nullptr));  // MultiGets run on other (non-blocking) streams
        lay.l0tab = (const uint32_t *)r->dl0.p;
        lay.l0md = mod_arg(g0->m, g0->k);
        lay.l0g = (uint32_t)grp.size();
        lay.l0b = gbits;
    }
    if (!slots.empty()) HIP_OR_FAIL(hipMemcpy(r->dslots.p, slots.data(), sizeof(RegSlot) * slots.size(), hipMemcpyHostToDevice));
    if (!ranges.empty()) HIP_OR_FAIL(hipMemcpy(r->dranges.p, ranges.data(), ranges.size(), hipMemcpyHostToDevice));
    if (!loc.empty()) HIP_OR_FAIL(hipMemcpy(r->dloc.p, loc.data(), sizeof(LocSlot) * loc.size(), hipMemcpyHostToDevice));
    r->nslots = (uint32_t)slots.size();
    r->layout = lay;
    r->max_cand = lay.hi[0] - lay.lo[0];
    for (int L = 1; L < 5; ++L) r->max_cand += lay.hi[L] > lay.lo[L] ? 1u : 0u;
    r->max_slot = 0;
    for (const RegEntry *e : order) r->max_slot = std::max(r->max_slot, e->slot + 1);
    r->part_lo = r->part_hi = 0;  // the disjoint level with the most files orders MultiGet batches
    for (int L = 1; L < 5; ++L)
        if ((lay.nonoverlap >> L & 1u) && lay.hi[L] - lay.lo[L] >= 2 && lay.hi[L] - lay.lo[L] < kMgMaxBuckets &&
            lay.hi[L] - lay.lo[L] > r->part_hi - r->part_lo) {
            r->part_lo = lay.lo[L];
            r->part_hi = lay.hi[L];
        }
    // Per bucket b (keys K with MinKey_P[b-1] <= K < MinKey_P[b] of the partition files P) and
    // disjoint level L: A = its files with MinKey <= MinKey_P[b-1], B = those with MinKey <
    // MinKey_P[b]; K's bisection result lies in [A, B].
    r->has_brange = false;
    if (r->part_hi > r->part_lo) {
        const uint32_t nb = r->part_hi - r->part_lo + 1;
        std::vector<uint32_t> br((size_t)nb * 4, 0u);
        for (uint32_t b = 0; b < nb; ++b) {
            const std::string *low = b ? &order[r->part_lo + b - 1]->min_key : nullptr;
            const std::string *high = b + 1 < nb ? &order[r->part_lo + b]->min_key : nullptr;
            for (int L = 1; L < 5; ++L) {
                uint32_t A = 0, B = lay.hi[L] - lay.lo[L];
                if ((lay.nonoverlap >> L & 1u) && lay.hi[L] > lay.lo[L]) {  // MinKey-ordered files
                    const auto f0 = order.begin() + lay.lo[L], f1 = order.begin() + lay.hi[L];
                    if (low)
                        A = (uint32_t)(std::partition_point(f0, f1, [&](const RegEntry *e) { return e->min_key <= *low; }) - f0);
                    if (high)
                        B = (uint32_t)(std::partition_point(f0, f1, [&](const RegEntry *e) { return e->min_key < *high; }) - f0);
                }
                br[(size_t)b * 4 + L - 1] = A | B << 16;
            }
        }
        int brc;
        if ((brc = r->dbrange.reserve(br.size() * 4))) return brc;
        HIP_OR_FAIL(hipMemcpy(r->dbrange.p, br.data(), br.size() * 4, hipMemcpyHostToDevice));
        r->has_brange = true;
    }
    r->dirty = false;
    return SEB_OK;
}

extern "C" int seb_registry_slots(seb_registry *r, uint64_t *file_nums, int32_t *levels, uint32_t cap) {
    if (!r) return fail(SEB_ERR_INVALID, "seb_registry_slots: null registry");
    std::lock_guard<std::mutex> g(r->mu);
    for (uint32_t s = 0; s < cap; ++s) {
        if (file_nums) file_nums[s] = UINT64_MAX;
        if (levels) levels[s] = -1;
    }
    for (auto &e : r->entries)
        if (e.slot < cap) {
            if (file_nums) file_nums[e.slot] = e.file_num;
            if (levels) levels[e.slot] = e.level;
        }
    return (int)r->entries.size();
}

// The layout a MultiGet launches with: the L0 group table only while multiget_l0_group is on.
static RegLayout mg_layout(const seb_registry *r) {
    RegLayout l = r->layout;
    if (!options().multiget_l0_group) l.l0g = 0;
    return l;
}

// multiget_order: the batch's key-range order over the registry's partition level, in the
// stream's scratch (tag 3); mo->active false when off, too small a batch or no disjoint level of
// >= 2 files.  On success kb reads the moved keys, if they were moved.
static std::atomic<uint64_t> g_mg_batch_order{0};
extern "C" uint64_t seb_multiget_order_fallbacks(void) { return g_mg_batch_order.load(std::memory_order_relaxed); }

static bool multiget_ordered(const seb_registry *r, uint64_t n) {
    return options().multiget_order && r->part_hi > r->part_lo && n >= 65536 && n <= 0xffffffffull;
}

static int multiget_order(seb_registry *r, KeyBatch &kb, uint64_t answer_bytes, hipStream_t s, MgOrder *mo) {
    *mo = MgOrder{};
    if (!multiget_ordered(r, kb.n)) return SEB_OK;
    void *ws = nullptr;
    int rc = cached_workspace(s, multiget_order_bytes(kb, answer_bytes, r->part_hi - r->part_lo + 1), &ws, 3);
    if (rc == SEB_ERR_NOMEM) {  // the order is only a speed-up: batch order needs no scratch
        last_error().clear();
        g_mg_batch_order.fetch_add(1, std::memory_order_relaxed);  // seb_multiget_order_fallbacks
        return SEB_OK;
    }
    if (rc) return rc;
    HIP_OR_FAIL(launch_multiget_order(kb, (const RegSlot *)r->dslots.p, r->part_lo, r->part_hi,
                                      (const uint8_t *)r->dranges.p, ws, mo, s));
    if (mo->keys) kb.data = mo->keys;  // the MultiGet streams the moved keys
    return SEB_OK;
}

// One MultiGet launch (mask form: maybe; list form: cand rows of cap u16) over kb, in key-range
// order when the registry has a partition level (answers in sorted rows, then unpermuted into the
// output), else in batch order.
// Largest ordered piece: the order's scratch (bucket ids, tables, sorted keys, sorted-row answers)
// stays near multiget_piece_mib (1 GiB) however large the batch or its rows; a larger batch is
// walked in pieces of whole 2048-key chunks, each in key-range order.

static int multiget_piece(seb_registry *r, KeyBatch kb, uint64_t *maybe, uint16_t *cand, uint32_t cap, hipStream_t s);

static int multiget_launch(seb_registry *r, KeyBatch kb, uint64_t *maybe, uint16_t *cand, uint32_t cap,
                           hipStream_t s) {
    const uint64_t answer_bytes = maybe ? 8 : 2ull * cap;
    const uint64_t scratch = (uint64_t)options().multiget_piece_mib << 20;
    const uint64_t piece = std::max<uint64_t>(65536, (scratch / (answer_bytes + 40)) & ~2047ull);
    if (!multiget_ordered(r, kb.n) || kb.n <= piece) return multiget_piece(r, kb, maybe, cand, cap, s);
    for (uint64_t off = 0; off < kb.n; off += piece) {
        KeyBatch p = kb;
        p.n = std::min(piece, kb.n - off);
        if (kb.offsets)
            p.offsets = kb.offsets + off;  // absolute offsets into the same data
        else
            p.data = kb.data + off * kb.stride;
        if (kb.hashes) p.hashes = kb.hashes + off;
        const int rc = multiget_piece(r, p, maybe ? maybe + off : nullptr, cand ? cand + off * cap : nullptr, cap, s);
        if (rc) return rc;
    }
    return SEB_OK;
}

static int multiget_piece(seb_registry *r, KeyBatch kb, uint64_t *maybe, uint16_t *cand, uint32_t cap,
                          hipStream_t s) {
    const uint64_t answer_bytes = maybe ? 8 : 2ull * cap;
    MgOrder mo;
    int rc;
    if ((rc = multiget_order(r, kb, answer_bytes, s, &mo))) return rc;
    // masks of a registry whose slots are all < 32 travel through the sorted rows as u32 (40 MB
    // less written and read per 10M keys), list rows of 2/4/6/8 slots all < 255 as u8 (6-slot rows:
    // 60 MB); the caller's output keeps its u64 masks / u16 rows
    if (mo.active && maybe && r->max_slot <= 32 && ((uintptr_t)maybe & 7) == 0) mo.narrow = 1;
    if (mo.seg.seg && r->has_brange) mo.seg.brange = (const uint32_t *)r->dbrange.p;
    if (mo.active && !maybe && r->max_slot <= 255 && cap <= 8 && cap % 2 == 0 &&
        ((uintptr_t)cand & (cap == 6 ? 3 : 2 * cap - 1)) == 0)
        mo.narrow = 2;
    HIP_OR_FAIL(launch_multiget(kb, (const RegSlot *)r->dslots.p, r->nslots, mg_layout(r), (const uint8_t *)r->dranges.p,
                                mo.active ? (maybe ? (uint64_t *)mo.answers : nullptr) : maybe,
                                mo.active ? (maybe ? nullptr : (uint16_t *)mo.answers) : cand, cap, s, mo.key_order,
                                mo.seg, mo.narrow != 0));
    if (mo.active)
        HIP_OR_FAIL(launch_multiget_unpermute(mo, maybe ? (void *)maybe : (void *)cand, answer_bytes, s));
    return SEB_OK;
}

// Mask form (maybe != null) or list form (cand, cap u16 per key); called with r->mu held and the
// registry synced.
static int check_multiget_out(seb_registry *r, uint64_t *maybe, uint16_t *cand, uint32_t cap, uint64_t n,
                              const char *who) {
    if (!maybe && !cand && n) return fail(SEB_ERR_INVALID, "%s: null output", who);
    if (maybe && r->max_slot > 64)
        return fail(SEB_ERR_INVALID, "%s: slot %u >= 64 does not fit a u64 mask; use seb_registry_multiget_list",
                    who, r->max_slot - 1);
    if (cand && cap < r->max_cand)
        return fail(SEB_ERR_INVALID, "%s: cap %u < %u candidates a key can have", who, cap, r->max_cand);
    return SEB_OK;
}

static int registry_multiget_dev(seb_registry *r, const seb_keys *keys, uint64_t *maybe, uint16_t *cand, uint32_t cap,
                                 void *stream, const char *who) {
    enter();
    int rc;
    if (!r) return fail(SEB_ERR_INVALID, "%s: null registry", who);
    if ((rc = check_keys(keys, who))) return rc;
    DeviceGuard dg;  // the registry's tables, and so the stream and its scratch, are on r->device
    if ((rc = dg.set(r->device))) return rc;
    WsCall ws_call;
    std::lock_guard<std::mutex> g(r->mu);
    if ((rc = sync_registry_locked(r)) || (rc = check_multiget_out(r, maybe, cand, cap, keys->n, who))) return rc;
    return multiget_launch(r, key_batch(keys), maybe, cand, cap, (hipStream_t)stream);
}

static int registry_multiget_host_locked(seb_registry *r, const seb_keys *kb, uint64_t *maybe, uint16_t *cand,
                                         uint32_t cap);

static int registry_multiget_host(seb_registry *r, const seb_keys *kb, uint64_t *maybe, uint16_t *cand, uint32_t cap,
                                  const char *who) {
    int rc;
    if (!r) return fail(SEB_ERR_INVALID, "%s: null registry", who);
    if ((rc = check_keys(kb, who)) || (rc = validate_offsets(kb, who))) return rc;
    std::lock_guard<std::mutex> g(r->mu);
    if ((rc = sync_registry_locked(r)) || (rc = check_multiget_out(r, maybe, cand, cap, kb->n, who))) return rc;
    return registry_multiget_host_locked(r, kb, maybe, cand, cap);
}

// Host keys through the registry's own context; r->mu held, registry synced, outputs checked.
static int registry_multiget_host_locked(seb_registry *r, const seb_keys *kb, uint64_t *maybe, uint16_t *cand,
                                         uint32_t cap) {
    WsCall ws_call;
    int rc;
    if (!r->ctx && (rc = seb_ctx_create(r->device, &r->ctx))) return rc;
    seb_ctx *c = r->ctx;
    std::lock_guard<std::mutex> g2(c->mu);
    HIP_OR_FAIL(hipSetDevice(c->device));
    return chunks_pipelined(c, kb, maybe ? 8 : 2ull * cap, maybe ? (void *)maybe : (void *)cand, false,
                            [&](const KeyBatch &dk, void *dout) {
                                return multiget_launch(r, dk, maybe ? (uint64_t *)dout : nullptr,
                                                       maybe ? nullptr : (uint16_t *)dout, cap, c->s_comp);
                            });
}

extern "C" int seb_registry_multiget_dev(seb_registry *r, const seb_keys *keys, uint64_t *maybe, void *stream) {
    if (!maybe && keys && keys->n) return fail(SEB_ERR_INVALID, "seb_registry_multiget: null output");
    return registry_multiget_dev(r, keys, maybe, nullptr, 0, stream, "seb_registry_multiget");
}

extern "C" int seb_registry_multiget(seb_registry *r, const seb_keys *kb, uint64_t *maybe) {
    if (!maybe && kb && kb->n) return fail(SEB_ERR_INVALID, "seb_registry_multiget: null output");
    return registry_multiget_host(r, kb, maybe, nullptr, 0, "seb_registry_multiget");
}

extern "C" int seb_registry_max_candidates(seb_registry *r) {
    if (!r) return fail(SEB_ERR_INVALID, "seb_registry_max_candidates: null registry");
    std::lock_guard<std::mutex> g(r->mu);
    int rc = sync_registry_locked(r);
    return rc ? rc : (int)r->max_cand;
}

extern "C" int seb_registry_multiget_list(seb_registry *r, const seb_keys *kb, uint16_t *cand, uint32_t cap) {
    if (!cand && kb && kb->n) return fail(SEB_ERR_INVALID, "seb_registry_multiget_list: null output");
    return registry_multiget_host(r, kb, nullptr, cand, cap, "seb_registry_multiget_list");
}

// The file-number forms (r->mu held, registry synced): rows of `cap` cells must hold the longest
// walk a key can have now, which *need names; then the rows' slot ids become file numbers.
static int check_files_cap(const seb_registry *r, uint32_t cap, uint32_t *need, const char *who) {
    const uint32_t want = std::max<uint32_t>(r->max_cand, 1);
    if (need) *need = want;
    if (cap < want)
        return fail(SEB_ERR_RANGE, "%s: cap %u < %u candidates a key can have now; retry with *need", who, cap, want);
    return SEB_OK;
}

static void slots_to_files(const seb_registry *r, const std::vector<uint16_t> &cand, uint64_t *files) {
    std::vector<uint64_t> by_slot(kRegMaxFiles, UINT64_MAX);
    for (auto &e : r->entries) by_slot[e.slot] = e.file_num;
    for (uint64_t i = 0; i < cand.size(); ++i) files[i] = cand[i] == 0xFFFF ? UINT64_MAX : by_slot[cand[i]];
}

// The list form translated to file numbers under ONE hold of the registry lock, so a Put or
// Remove between sizing the rows, running the lookup and mapping slots to files cannot make the
// rows overflow or a freed-and-reused slot name the wrong file (the three-call sequence
// max_candidates / multiget_list / slots is not atomic).
extern "C" int seb_registry_multiget_files(seb_registry *r, const seb_keys *kb, uint64_t *files, uint32_t cap,
                                           uint32_t *need) {
    const char *who = "seb_registry_multiget_files";
    int rc;
    if (!r) return fail(SEB_ERR_INVALID, "%s: null registry", who);
    if ((rc = check_keys(kb, who)) || (rc = validate_offsets(kb, who))) return rc;
    if (!files && kb->n) return fail(SEB_ERR_INVALID, "%s: null output", who);
    std::lock_guard<std::mutex> g(r->mu);
    if ((rc = sync_registry_locked(r)) || (rc = check_files_cap(r, cap, need, who))) return rc;
    if (kb->n == 0) return SEB_OK;
    std::vector<uint16_t> cand(kb->n * (uint64_t)cap);
    if ((rc = registry_multiget_host_locked(r, kb, nullptr, cand.data(), cap))) return rc;
    slots_to_files(r, cand, files);
    return SEB_OK;
}

extern "C" int seb_registry_multiget_list_dev(seb_registry *r, const seb_keys *keys, uint16_t *cand, uint32_t cap,
                                              void *stream) {
    if (!cand && keys && keys->n) return fail(SEB_ERR_INVALID, "seb_registry_multiget_list: null output");
    return registry_multiget_dev(r, keys, nullptr, cand, cap, stream, "seb_registry_multiget_list");
}

// ---------------------------------------- sparse indexes + the batched block locator ----------
// What SSTable.Get does with a file that passed its filter (lsm/sstable.go:210-222): bisect the
// file's sparse index for the key and take the entry before the first greater one.  The index
// block (decodeIndex, lsm/sstable.go:168-201: [numEntries u32] then per entry [keySize u32]
// [blockOffset u64][key]) is parsed once into device arrays next to the file's filter words.

struct IndexView {  // one walk of an encoded index block
    std::vector<uint64_t> pre, koff, boff;
    std::string bytes;
};

// decodeIndex's walk plus the order check; view == nullptr only validates and counts.
static int index_walk(const uint8_t *index, uint64_t len, uint64_t *entries, IndexView *view, const char *who) {
    if (len && !index) return fail(SEB_ERR_INVALID, "%s: null index", who);
    if (len < 4) return fail(SEB_ERR_SHORT, "%s: index too small (%llu bytes)", who, (unsigned long long)len);
    uint32_t num;
    memcpy(&num, index, 4);
    uint64_t at = 4;
    const uint8_t *prev = nullptr;
    uint64_t prev_len = 0;
    if (view) view->koff.push_back(0);
    for (uint32_t e = 0; e < num; ++e) {
        if (len - at < 12) return fail(SEB_ERR_SHORT, "%s: index truncated in the header of entry %u", who, e);
        uint32_t ks;
        uint64_t bo;
        memcpy(&ks, index + at, 4);
        memcpy(&bo, index + at + 4, 8);
        at += 12;
        if (len - at < ks) return fail(SEB_ERR_SHORT, "%s: index truncated in the key of entry %u", who, e);
        const uint8_t *key = index + at;
        if (prev) {  // Go string order: bytewise, a proper prefix first
            const int c = memcmp(prev, key, (size_t)std::min<uint64_t>(prev_len, ks));
            if (c > 0 || (c == 0 && prev_len > ks))
                return fail(SEB_ERR_INVALID, "%s: index keys decrease at entry %u", who, e);
        }
        if (view) {
            uint64_t be[2];
            be_prefix(std::string((const char *)key, std::min<uint32_t>(ks, 16)), be);
            view->pre.push_back(be[0]);
            view->pre.push_back(be[1]);
            view->boff.push_back(bo);
            view->bytes.append((const char *)key, ks);
            view->koff.push_back(view->bytes.size());
        }
        prev = key;
        prev_len = ks;
        at += ks;
    }
    if (entries) *entries = num;
    return SEB_OK;
}

extern "C" int seb_index_scan(const uint8_t *index, uint64_t index_len, uint64_t *entries) {
    if (entries) *entries = 0;
    return index_walk(index, index_len, entries, nullptr, "seb_index_scan");
}

extern "C" int seb_registry_put_index(seb_registry *r, uint64_t file_num, const uint8_t *index, uint64_t index_len) {
    const char *who = "seb_registry_put_index";
    if (!r) return fail(SEB_ERR_INVALID, "%s: null registry", who);
    IndexView v;
    uint64_t n = 0;
    int rc;
    if ((rc = index_walk(index, index_len, &n, &v, who))) return rc;
    std::lock_guard<std::mutex> g(r->mu);
    RegEntry *e = find_entry(r, file_num);
    if (!e) return fail(SEB_ERR_INVALID, "%s: file %llu not registered", who, (unsigned long long)file_num);
    if (e->has_index) return fail(SEB_ERR_INVALID, "%s: file %llu already has an index", who, (unsigned long long)file_num);
    LocSlot loc{};
    void *d = nullptr;
    if (n) {  // one block: pre (16 B per entry) | boff | koff (n + 1) | bytes
        DeviceGuard dg;
        if ((rc = dg.set(r->device))) return rc;
        const uint64_t pre_b = 16 * n, boff_b = 8 * n, koff_b = 8 * (n + 1);
        hipError_t a = hipMalloc(&d, pre_b + boff_b + koff_b + v.bytes.size() + 16);
        if (a != hipSuccess) return (void)hipGetLastError(), fail(SEB_ERR_NOMEM, "%s: hipMalloc: %s", who, hipGetErrorString(a));
        uint8_t *p = (uint8_t *)d;
        hipError_t c = hipMemcpy(p, v.pre.data(), pre_b, hipMemcpyHostToDevice);
        if (c == hipSuccess) c = hipMemcpy(p + pre_b, v.boff.data(), boff_b, hipMemcpyHostToDevice);
        if (c == hipSuccess) c = hipMemcpy(p + pre_b + boff_b, v.koff.data(), koff_b, hipMemcpyHostToDevice);
        if (c == hipSuccess && !v.bytes.empty())
            c = hipMemcpy(p + pre_b + boff_b + koff_b, v.bytes.data(), v.bytes.size(), hipMemcpyHostToDevice);
        if (c != hipSuccess) {
            (void)hipFree(d);
            (void)hipGetLastError();
            return fail(hip_status(c), "%s: hipMemcpy: %s", who, hipGetErrorString(c));
        }
        loc.pre = (const uint64_t *)p;
        loc.boff = (const uint64_t *)(p + pre_b);
        loc.koff = (const uint64_t *)(p + pre_b + boff_b);
        loc.bytes = p + pre_b + boff_b + koff_b;
        loc.n = (uint32_t)n;
    }
    e->has_index = true;
    e->dindex = d;
    e->loc = loc;
    r->dirty = true;
    return SEB_OK;
}

extern "C" int seb_registry_index_entries(seb_registry *r, uint64_t file_num, uint64_t *entries) {
    const char *who = "seb_registry_index_entries";
    if (!r || !entries) return fail(SEB_ERR_INVALID, "%s: null argument", who);
    std::lock_guard<std::mutex> g(r->mu);
    const RegEntry *e = find_entry(r, file_num);
    if (!e) return fail(SEB_ERR_INVALID, "%s: file %llu not registered", who, (unsigned long long)file_num);
    if (!e->has_index) return fail(SEB_ERR_INVALID, "%s: file %llu has no index", who, (unsigned long long)file_num);
    *entries = e->loc.n;
    return SEB_OK;
}

// r->mu held: every registered file must have its index before cells may name it.
static int check_indexes_locked(const seb_registry *r, const char *who) {
    for (auto &e : r->entries)
        if (!e.has_index)
            return fail(SEB_ERR_INVALID, "%s: file %llu has no index (seb_registry_put_index)", who,
                        (unsigned long long)e.file_num);
    return SEB_OK;
}

extern "C" int seb_registry_locate_dev(seb_registry *r, const seb_keys *keys, const uint16_t *cand, uint32_t cap,
                                       uint64_t *blocks, void *stream) {
    const char *who = "seb_registry_locate";
    enter();
    int rc;
    if (!r || !cand || !blocks) return fail(SEB_ERR_INVALID, "%s: null argument", who);
    if (cap == 0) return fail(SEB_ERR_INVALID, "%s: cap 0", who);
    if ((rc = check_keys(keys, who))) return rc;
    DeviceGuard dg;
    if ((rc = dg.set(r->device))) return rc;
    std::lock_guard<std::mutex> g(r->mu);
    if ((rc = sync_registry_locked(r)) || (rc = check_indexes_locked(r, who))) return rc;
    if (keys->n == 0) return SEB_OK;
    HIP_OR_FAIL(launch_locate(key_batch(keys), cand, cap, (const LocSlot *)r->dloc.p, r->max_slot, blocks,
                              (hipStream_t)stream));
    return SEB_OK;
}

// Host keys through the registry's own context, a chunk at a time on its compute stream; r->mu held,
// registry synced, indexes checked.  cand_in != null: locate those rows.  Else the MultiGet's own rows
// are located and copied to cand_out.
static int registry_locate_host_locked(seb_registry *r, const seb_keys *kb, const uint16_t *cand_in, uint16_t *cand_out,
                                       uint32_t cap, uint64_t *blocks) {
    WsCall ws_call;
    int rc;
    if (!r->ctx && (rc = seb_ctx_create(r->device, &r->ctx))) return rc;
    seb_ctx *c = r->ctx;
    std::lock_guard<std::mutex> g2(c->mu);
    HIP_OR_FAIL(hipSetDevice(c->device));
    return chunks_serial(c, kb, [&](const KeyBatch &dk, const Chunk &ch) -> int {
        const uint64_t cells = dk.n * (uint64_t)cap;
        if ((rc = r->dcand.reserve(cells * 2)) || (rc = r->dblocks.reserve(cells * 8))) return rc;
        uint16_t *dc = (uint16_t *)r->dcand.p;
        if (cand_in) {
            HIP_OR_FAIL(hipMemcpyAsync(dc, cand_in + ch.i0 * cap, cells * 2, hipMemcpyHostToDevice, c->s_comp));
        } else {
            if ((rc = multiget_launch(r, dk, nullptr, dc, cap, c->s_comp))) return rc;
            HIP_OR_FAIL(hipMemcpyAsync(cand_out + ch.i0 * cap, dc, cells * 2, hipMemcpyDeviceToHost, c->s_comp));
        }
        HIP_OR_FAIL(launch_locate(dk, dc, cap, (const LocSlot *)r->dloc.p, r->max_slot, (uint64_t *)r->dblocks.p,
                                  c->s_comp));
        HIP_OR_FAIL(hipMemcpyAsync(blocks + ch.i0 * cap, r->dblocks.p, cells * 8, hipMemcpyDeviceToHost, c->s_comp));
        return SEB_OK;
    });
}

extern "C" int seb_registry_locate(seb_registry *r, const seb_keys *kb, const uint16_t *cand, uint32_t cap,
                                   uint64_t *blocks) {
    const char *who = "seb_registry_locate";
    int rc;
    if (!r || !cand || !blocks) return fail(SEB_ERR_INVALID, "%s: null argument", who);
    if (cap == 0) return fail(SEB_ERR_INVALID, "%s: cap 0", who);
    if ((rc = check_keys(kb, who)) || (rc = validate_offsets(kb, who))) return rc;
    std::lock_guard<std::mutex> g(r->mu);
    if ((rc = sync_registry_locked(r)) || (rc = check_indexes_locked(r, who))) return rc;
    if (kb->n == 0) return SEB_OK;
    return registry_locate_host_locked(r, kb, cand, nullptr, cap, blocks);
}

// seb_registry_multiget_files plus each candidate's block offset: lookup, locate and the slot->file
// mapping under ONE hold of the registry lock.
extern "C" int seb_registry_multiget_blocks(seb_registry *r, const seb_keys *kb, uint64_t *files, uint64_t *blocks,
                                            uint32_t cap, uint32_t *need) {
    const char *who = "seb_registry_multiget_blocks";
    int rc;
    if (!r) return fail(SEB_ERR_INVALID, "%s: null registry", who);
    if ((rc = check_keys(kb, who)) || (rc = validate_offsets(kb, who))) return rc;
    if ((!files || !blocks) && kb->n) return fail(SEB_ERR_INVALID, "%s: null output", who);
    std::lock_guard<std::mutex> g(r->mu);
    if ((rc = sync_registry_locked(r)) || (rc = check_files_cap(r, cap, need, who)) ||
        (rc = check_indexes_locked(r, who)))
        return rc;
    if (kb->n == 0) return SEB_OK;
    std::vector<uint16_t> cand(kb->n * (uint64_t)cap);
    if ((rc = registry_locate_host_locked(r, kb, nullptr, cand.data(), cap, blocks))) return rc;
    slots_to_files(r, cand, files);
    return SEB_OK;
}
