// zpq_api.hip -- the GPU half of the C ABI in include/zpaq_hip.h: per-device
// context, state-slot management, kernel selection and launch.
//
// Data layout in HBM (DESIGN.md has the full picture):
//   * read-only tables (squash/stretch/dt/dt2k/ns, ~80 KiB) uploaded once per ctx;
//   * one DModel + init image per (ctx, model);
//   * a pool of per-block STATE SLOTS, each DModel::slot_bytes (12.07 MiB at level 2):
//     [VM regs | R[256] | MATCH scalars | H | M | per-component cm/ht/a16 tables].
//     A slot is owned by one resident workgroup (generic kernel) or one lane group
//     (chain kernel) and re-initialised in-kernel between blocks;
//   * caller-provided in/out slabs addressed by in_off/out_off.
// There is no CPU fallback anywhere in this file: if HIP is unusable every
// compute entry point returns ZPQ_E_NODEVICE.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <exception>
#include <map>
#include <mutex>
#include <thread>
#include <unordered_set>
#include <vector>

#include "../../include/zpaq_hip.h"
#include "zpq_common.h"
#include "zpq_host.h"
#include "zpq_dev.h"

#define ZPQ_SET_ALL (ZPQ_SET_LANES | ZPQ_SET_PIPE | ZPQ_SET_WAVES | ZPQ_SET_VMWAVES | ZPQ_SET_CHUNKS)

#define HIPCK(x)                                                              \
    do {                                                                      \
        hipError_t e_ = (x);                                                  \
        if (e_ != hipSuccess) {                                               \
            fprintf(stderr, "[zpaq_hip] %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return (e_ == hipErrorOutOfMemory) ? ZPQ_E_NOMEM : ZPQ_E_NODEVICE; \
        }                                                                     \
    } while (0)

struct DevModel {
    DModel *d_model = nullptr;
    uint32_t *d_img = nullptr;
};

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t n)
    {
        if (n <= cap) return ZPQ_OK;
        // Grow: take the new buffer first so that a failed regrow keeps the old one usable.  Pools of ~100 GiB
        // cannot coexist with their successor; only then is the old one given up before the second attempt.
        size_t want = n + n / 8 + 4096;
        void *q = nullptr;
        if (hipMalloc(&q, want) != hipSuccess) {
            (void)hipGetLastError();
            q = nullptr;
            if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
            if (hipMalloc(&q, want) != hipSuccess) {
                (void)hipGetLastError();
                want = n + 4096;
                if (hipMalloc(&q, want) != hipSuccess) { (void)hipGetLastError(); return ZPQ_E_NOMEM; }
            }
        }
        if (p) (void)hipFree(p);
        p = q;
        cap = want;
        return ZPQ_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }                                // (the owner has selected the device: zpq_ctx_destroy)
};

// The caller's arrays of a batch call, as include/zpaq_hip.h passes them: host pointers at the host entry points, device
// pointers below run_batch.  consumed / final_code / first_byte are the decoder's and may be null.
struct BlockArrays {
    int n = 0;
    const uint8_t *in = nullptr; const uint64_t *in_off = nullptr;
    uint32_t flags = 0;
    uint8_t *out = nullptr; const uint64_t *out_off = nullptr;
    uint32_t *out_len = nullptr, *consumed = nullptr, *final_code = nullptr, *first_byte = nullptr;
    int32_t *status = nullptr;
    // blocks [b0, b1): the offsets stay absolute, so in / out do not move
    BlockArrays window(int b0, int b1) const
    {
        BlockArrays w = *this;
        w.n = b1 - b0; w.in_off = in_off + b0; w.out_off = out_off + b0; w.out_len = out_len + b0; w.status = status + b0;
        w.consumed = consumed ? consumed + b0 : nullptr;
        w.final_code = final_code ? final_code + b0 : nullptr;
        w.first_byte = first_byte ? first_byte + b0 : nullptr;
        return w;
    }
    uint64_t in_bytes() const { return in_off[n] - in_off[0]; }
    uint64_t out_bytes() const { return out_off[n] - out_off[0]; }
};
// the ABI's parameter order, once (encoders have no consumed / final_code / first_byte)
static BlockArrays block_arrays(int n, const uint8_t *in, const uint64_t *in_off, uint32_t flags, uint8_t *out, const uint64_t *out_off,
                                uint32_t *out_len, int32_t *status, uint32_t *consumed = nullptr, uint32_t *final_code = nullptr,
                                uint32_t *first_byte = nullptr)
{
    BlockArrays h;
    h.n = n; h.in = in; h.in_off = in_off; h.flags = flags; h.out = out; h.out_off = out_off;
    h.out_len = out_len; h.status = status; h.consumed = consumed; h.final_code = final_code; h.first_byte = first_byte;
    return h;
}
// ... and what only the debug hooks and zpq_block pass
struct BatchExtras {
    uint8_t *own_slot = nullptr;   // zpq_block: use this slot instead of the pool
    int32_t *trace = nullptr; uint32_t ntrace = 0;
    uint32_t *ctx_out = nullptr; size_t ctx_words = 0;
};

// Slab check of a host-pointer call: offsets monotone, no block beyond what a 32-bit length holds, and bytes behind
// every non-empty window.  `out` = false: the input half alone, without the length bound (zpq_sha1_blocks).
static bool slabs_valid(const BlockArrays &h, bool out = true)
{
    for (int b = 0; b < h.n; b++) {
        if (h.in_off[b + 1] < h.in_off[b]) return false;
        if (out && (h.out_off[b + 1] < h.out_off[b] || h.in_off[b + 1] - h.in_off[b] > 0xFFFFFFF0ull ||
                    h.out_off[b + 1] - h.out_off[b] > 0xFFFFFFF0ull))
            return false;
    }
    return !(h.in_bytes() && !h.in) && !(out && h.out_bytes() && !h.out);
}

// One staging set for a window of host blocks: the device side of the bytes, the offsets and the small results, the
// pinned host side of the small arrays, and the events that order a round's upload, kernel and download.  The ctx has
// three: one for the one-shot calls, two for host_pipeline's rounds.
struct StageSet {
    DevBuf in, out, inoff, outoff, dstoff, meta, status, misc;   // misc: trace / ctx_out, or a block set's slot map
    hipEvent_t ev_in = nullptr, ev_k = nullptr, ev_out = nullptr;
    // pinned host side of the small arrays: a copy to or from PAGEABLE memory blocks the calling thread until it
    // has run, i.e. until the round's kernel is done -- which would keep the next round's upload from being queued
    uint64_t *h_off = nullptr;         // [3][n + 1]: relative in / out offsets, absolute destination offsets
    uint32_t *h_meta = nullptr;        // [4][n] out_len, consumed, final_code, first_byte  + [n] status
    size_t h_cap = 0;                  // blocks the pinned arrays are sized for
    int b0 = 0, n = 0;                 // the window whose results sit in h_meta (not yet handed to the caller)
    StageSet() = default;
    StageSet(const StageSet &) = delete;
    StageSet &operator=(const StageSet &) = delete;
    ~StageSet()
    {
        if (h_off) (void)hipHostFree(h_off);
        if (h_meta) (void)hipHostFree(h_meta);
        for (hipEvent_t e : {ev_in, ev_k, ev_out}) if (e) (void)hipEventDestroy(e);
    }
    int create_events()
    {
        for (hipEvent_t *e : {&ev_in, &ev_k, &ev_out}) HIPCK(hipEventCreateWithFlags(e, hipEventDisableTiming));
        return ZPQ_OK;
    }
    int ensure_host(size_t nblk)
    {
        if (nblk <= h_cap) return ZPQ_OK;
        if (h_off) (void)hipHostFree(h_off);
        if (h_meta) (void)hipHostFree(h_meta);
        h_off = nullptr; h_meta = nullptr; h_cap = 0;
        const size_t want = nblk + nblk / 8 + 16;
        if (hipHostMalloc((void **)&h_off, 3 * (want + 1) * 8, hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc((void **)&h_meta, 5 * want * 4, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return ZPQ_E_NOMEM; }
        h_cap = want;
        return ZPQ_OK;
    }
    uint64_t *h_in() const { return h_off; }
    uint64_t *h_out(int nb) const { return h_off + (nb + 1); }
    uint64_t *h_dst(int nb) const { return h_off + 2 * (size_t)(nb + 1); }
    // what a kernel sees of a staged window of nb blocks
    BlockArrays device_view(int nb, uint32_t flags, int decode) const
    {
        uint32_t *m = (uint32_t *)meta.p;
        return block_arrays(nb, (const uint8_t *)in.p, (const uint64_t *)inoff.p, flags, (uint8_t *)out.p, (const uint64_t *)outoff.p, m,
                            (int32_t *)status.p, decode ? m + nb : nullptr, decode ? m + 2 * (size_t)nb : nullptr, decode ? m + 3 * (size_t)nb : nullptr);
    }
};

struct zpq_ctx {
    int device = 0;
    int cus = 256;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool ev_valid = false;
    int16_t *d_squash = nullptr, *d_stretch = nullptr, *d_dt2k = nullptr;
    uint32_t *d_dt = nullptr, *d_stretch_c = nullptr;
    uint8_t *d_ns = nullptr;
    std::map<uint64_t, DevModel> models;   // key = model id << 32 | compact-store capacity (0 = dense layout)
    uint32_t sparse_cap = 0;               // line-store capacity (lines) for the largest block the caller submits
    uint32_t sparse_pct = 112;             // capacity = this percentage of the lines a largest block can touch (125: measured 4-7 % slower at levels 4-5, fewer blocks fit)
    DevBuf slots;
    // The pool's dirty-line logs (DBatch::dlog, zpq_dev.h), beside the pool.  Slots [0, dlog_valid) hold what a launch of a
    // log-keeping kernel left, for the device model dlog_model at dlog_cap entries per table, and their logs name every line
    // of theirs that is not zero: the next such launch clears those lines alone.  Any other launch on the pool, a launch that
    // failed, a pool or log buffer that was reallocated or released, and a new state budget make it 0 (dlog_drop).
    DevBuf dlog;
    const DModel *dlog_model = nullptr;    // (the device copy: one per model and layout)
    DModel dlog_layout;                    // ... and the layout it holds (zpq_debug_pool_residue)
    uint32_t dlog_cap = 0;
    int dlog_valid = 0;
    void dlog_drop() { dlog_valid = 0; dlog_model = nullptr; }
    uint64_t budget = 0;
    int last_slots = 0;
    unsigned last_host = 0;                // what host_pipeline did with the last host-pointer batch (zpq_ctx_last_host_transfer)
    uint32_t last_sp = 0;                  // line-store capacity the last launch ran with (0 = dense)
    const char *last_name = "";
    // staging for the host-pointer entry points: the one-shot calls' set, and for pipelined host batches (host_pipeline)
    // two more with a copy-in and a copy-out stream beside the compute stream
    StageSet one, pipe[2];
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    uint32_t *h_gate = nullptr;            // pinned, device-visible: "the rest of the striped upload has arrived"
    std::mutex mu;
    std::vector<zpq_block *> children;     // blocks created on this ctx and not yet destroyed (guarded by g_reg_mu)
    std::vector<zpq_blockset *> sets;      // block sets likewise
    uint64_t set_bytes = 0;                // state slots held by block sets: they count against `budget`
    uint64_t pool_budget() const { return budget > set_bytes ? budget - set_bytes : 0; }   // what is left for the slot pool
};

// ------------------------------------------------------------------ handle lifetime
// A front end may drop its handles in any order (a garbage-collected host language does): a zpq_block may outlive its
// zpq_ctx and its zpq_model.  The ctx keeps the list of its blocks and, when destroyed, releases their device state and
// ORPHANS them (b->ctx = nullptr: every later call on the block returns ZPQ_E_CLOSED, zpq_block_destroy only frees the
// host struct); a block holds a reference on its model.  A zpq_ctx* is checked against the set of living contexts at
// every entry point, so that a call on a destroyed ctx is an error code, not a read of freed memory.
static std::mutex g_reg_mu;
static std::unordered_set<const zpq_ctx *> &live_set()
{
    static std::unordered_set<const zpq_ctx *> *s = new std::unordered_set<const zpq_ctx *>();   // never destroyed: handles may be dropped from atexit handlers
    return *s;
}
static bool ctx_live(const zpq_ctx *c)
{
    if (!c) return false;
    std::lock_guard<std::mutex> lk(g_reg_mu);
    return live_set().count(c) != 0;
}

void zpq_note_exception(const char *where) noexcept
{
    try {
        try { throw; }
        catch (const std::exception &e) { fprintf(stderr, "[zpaq_hip] %s: C++ exception stopped at the C boundary: %s\n", where, e.what()); }
        catch (...) { fprintf(stderr, "[zpaq_hip] %s: unknown C++ exception stopped at the C boundary\n", where); }
    } catch (...) {
    }
}

struct zpq_block {
    zpq_ctx *ctx;              // nullptr once the ctx has been destroyed (orphaned block)
    const zpq_model *model;    // the block holds a reference (zpq_model_retain)
    uint8_t *slot;
    bool fresh;
    // A block's FIRST segment runs on the fast batch kernels (their state lives in LDS / the shared pool and is
    // gone afterwards).  Most blocks have exactly one segment; if a second one arrives, the persistent state in
    // `slot` is materialised first by replaying segment 1's symbols through the generic kernel (the model state
    // depends only on the symbol sequence, not on which direction coded it).
    bool lazy = false;
    std::vector<uint8_t> lazy_in;
    uint32_t lazy_flags = 0;
};

// N blocks whose model state persists across segments, coded a segment of each per launch (zpq_blockset_*).  The state
// lives in the set's own slots, in the layout chosen when the set is made: chain models on k_chain<..., KEEP> (dense tables
// or the line store, sized by max_member_bytes), every other model on k_generic with ZB_KEEP_STATE, a launch per member --
// or, on request (ZPQ_SET_LANES) and with at most 64 components, on the KEEP forms of k_rows / k_lanes, a launch per round;
// with ZPQ_SET_WAVES on top, and a model both wave-per-component kernels take, on k_wset / k_wsetd (zpq_gpipe.hip), call by call;
// with ZPQ_SET_VMWAVES on top, and a model the interpreter-wave pair takes, on k_vset / k_vsetd, call by call.
struct zpq_blockset {
    zpq_ctx *ctx = nullptr;        // nullptr once the ctx has been destroyed (orphaned set)
    const zpq_model *model = nullptr;   // the set holds a reference
    int nmembers = 0;
    bool chain = false;
    uint32_t flags = 0;            // ZPQ_SET_* in force (a request that decides nothing is not among them)
    uint32_t sp = 0;               // line-store capacity (lines), 0 = dense tables
    DModel layout;                 // what the kernels see
    uint8_t *slots = nullptr;
    uint64_t bytes = 0;
    std::vector<int32_t> failed;   // per member: ZPQ_OK, or the status its first failing segment ended with (sticky)
    std::vector<uint8_t> fresh;    // per member: no segment coded yet (the generic route initialises in-kernel)
    std::vector<uint8_t> open;     // per member: a chunk call left its segment unfinished (1 = the encoder did, 2 = the decoder; 0 = no)
};

// ------------------------------------------------------------------ ctx
static int ctx_init(zpq_ctx *c, const zpq::Tables &T);
static int set_max_block_bytes(zpq_ctx *c, uint64_t bytes);
extern "C" int zpq_ctx_create(int device, zpq_ctx **out) try
{
    if (!out) return ZPQ_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ZPQ_E_NODEVICE;
    if (device < 0 || device >= ndev) return ZPQ_E_ARG;
    int tst = ZPQ_OK;
    const zpq::Tables &T = zpq::tables(&tst);
    if (tst != ZPQ_OK) return tst;
    HIPCK(hipSetDevice(device));
    zpq_ctx *c = new (std::nothrow) zpq_ctx();
    if (!c) return ZPQ_E_NOMEM;
    c->device = device;
    const int rc = ctx_init(c, T);
    { std::lock_guard<std::mutex> lk(g_reg_mu); live_set().insert(c); }
    if (rc != ZPQ_OK) { zpq_ctx_destroy(c); return rc; }   // releases whatever the failed step left behind
    *out = c;
    return ZPQ_OK;
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

static int ctx_init(zpq_ctx *c, const zpq::Tables &T)
{
    const int device = c->device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->cus = prop.multiProcessorCount;
    HIPCK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPCK(hipEventCreate(&c->ev0));
    HIPCK(hipEventCreate(&c->ev1));
    HIPCK(hipStreamCreateWithFlags(&c->s_h2d, hipStreamNonBlocking));
    HIPCK(hipStreamCreateWithFlags(&c->s_d2h, hipStreamNonBlocking));
    HIPCK(hipHostMalloc((void **)&c->h_gate, 64, hipHostMallocPortable | hipHostMallocMapped));
    *c->h_gate = 1;
    for (auto &ps : c->pipe) if (int rc = ps.create_events()) return rc;   // (the one-shot set runs on one stream: no events)
    // device tables: squash/stretch/dt2k narrowed to i16 (all values fit)
    std::vector<int16_t> sq(4096), st(32768), d2(256);
    for (int i = 0; i < 4096; i++) sq[i] = (int16_t)T.squash[i];
    for (int i = 0; i < 32768; i++) st[i] = (int16_t)T.stretch[i];
    for (int i = 0; i < 256; i++) d2[i] = (int16_t)T.dt2k[i];
    HIPCK(hipMalloc((void **)&c->d_squash, 4096 * 2));
    HIPCK(hipMalloc((void **)&c->d_stretch, 32768 * 2));
    HIPCK(hipMalloc((void **)&c->d_dt2k, 256 * 2));
    HIPCK(hipMalloc((void **)&c->d_dt, 1024 * 4));
    HIPCK(hipMalloc((void **)&c->d_ns, 1024));
    HIPCK(hipMalloc((void **)&c->d_stretch_c, sizeof T.stretch_c));
    HIPCK(hipMemcpy(c->d_squash, sq.data(), 4096 * 2, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(c->d_stretch, st.data(), 32768 * 2, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(c->d_dt2k, d2.data(), 256 * 2, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(c->d_dt, T.dt, 1024 * 4, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(c->d_ns, T.ns, 1024, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(c->d_stretch_c, T.stretch_c, sizeof T.stretch_c, hipMemcpyHostToDevice));
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) c->budget = (uint64_t)fr / 100 * 85;
    else c->budget = 64ull << 30;
    {
        const char *ev = getenv("ZPQ_SPARSE_PCT");             // tuning knob: store capacity as % of the touched-line bound
        const int pct = ev ? atoi(ev) : 0;
        if (pct >= 101 && pct <= 400) c->sparse_pct = (uint32_t)pct;
    }
    set_max_block_bytes(c, 65536);
    return ZPQ_OK;
}

extern "C" void zpq_ctx_destroy(zpq_ctx *c) try
{
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        if (!c || !live_set().erase(c)) return;            // null, destroyed already, or never a ctx of this library
    }
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    {
        // blocks that outlive their ctx: their device state goes with it, the host structs stay for zpq_block_destroy
        std::lock_guard<std::mutex> lk(g_reg_mu);
        for (zpq_block *b : c->children) {
            if (b->slot) (void)hipFree(b->slot);
            b->slot = nullptr;
            b->ctx = nullptr;
        }
        c->children.clear();
        for (zpq_blockset *bs : c->sets) {
            if (bs->slots) (void)hipFree(bs->slots);
            bs->slots = nullptr;
            bs->ctx = nullptr;
        }
        c->sets.clear();
        c->set_bytes = 0;
    }
    for (auto &kv : c->models) { (void)hipFree(kv.second.d_model); (void)hipFree(kv.second.d_img); }
    if (c->h_gate) (void)hipHostFree(c->h_gate);
    if (c->s_h2d) { (void)hipStreamSynchronize(c->s_h2d); (void)hipStreamDestroy(c->s_h2d); }
    if (c->s_d2h) { (void)hipStreamSynchronize(c->s_d2h); (void)hipStreamDestroy(c->s_d2h); }
    (void)hipFree(c->d_squash); (void)hipFree(c->d_stretch); (void)hipFree(c->d_dt2k);
    (void)hipFree(c->d_dt); (void)hipFree(c->d_ns); (void)hipFree(c->d_stretch_c);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;                                               // (the slot pool and the staging sets release themselves: the device is selected above)
} ZPQ_CATCH(return)

extern "C" int zpq_ctx_sync(zpq_ctx *c) try
{
    if (!ctx_live(c)) return ZPQ_E_ARG;
    HIPCK(hipStreamSynchronize(c->stream));
    return ZPQ_OK;
} ZPQ_CATCH(return ZPQ_E_INTERNAL)
extern "C" int zpq_ctx_device(const zpq_ctx *c) { return ctx_live(c) ? c->device : -1; }
extern "C" void *zpq_ctx_stream(zpq_ctx *c) { return ctx_live(c) ? (void *)c->stream : nullptr; }
extern "C" int zpq_ctx_set_state_budget(zpq_ctx *c, uint64_t bytes) try
{
    if (!ctx_live(c)) return ZPQ_E_ARG;
    c->budget = bytes;
    c->dlog_drop();
    return ZPQ_OK;
} ZPQ_CATCH(return ZPQ_E_INTERNAL)
extern "C" int zpq_ctx_set_max_block_bytes(zpq_ctx *c, uint64_t bytes) try
{
    if (!ctx_live(c)) return ZPQ_E_ARG;
    return set_max_block_bytes(c, bytes);
} ZPQ_CATCH(return ZPQ_E_INTERNAL)
static uint32_t line_store_cap(const zpq_ctx *c, uint64_t bytes)
{
    // A block of N bytes (+ PP byte) probes each hash table 2(N+1) times (predictor.v:558-560: once per nibble),
    // so it touches at most that many 64-byte lines.  The store holds sparse_pct % of that bound: probing is
    // linear over 4-slot groups, a worst-case block (every probe a new line) ends at 89 % load.
    const uint64_t probes = 2 * (bytes + 2);
    uint64_t cap = (probes * c->sparse_pct + 99) / 100 + 16;
    cap = (cap + 3) & ~3ull;
    if (cap > (1ull << 25)) cap = 1ull << 25;               // line offsets are 32-bit in the kernel
    return (uint32_t)cap;
}
static int set_max_block_bytes(zpq_ctx *c, uint64_t bytes)
{
    c->sparse_cap = line_store_cap(c, bytes);
    return ZPQ_OK;
}
extern "C" int zpq_ctx_last_slots(const zpq_ctx *c) { return ctx_live(c) ? c->last_slots : 0; }
extern "C" unsigned zpq_ctx_last_host_transfer(const zpq_ctx *c) { return ctx_live(c) ? c->last_host : 0u; }
extern "C" unsigned zpq_ctx_last_line_store(const zpq_ctx *c) { return ctx_live(c) ? c->last_sp : 0u; }
extern "C" const char *zpq_ctx_last_kernel_name(const zpq_ctx *c) { return ctx_live(c) ? c->last_name : ""; }
extern "C" float zpq_ctx_last_kernel_ms(const zpq_ctx *c) try
{
    if (!ctx_live(c) || !c->ev_valid) return -1.f;
    if (hipEventSynchronize(c->ev1) != hipSuccess) return -1.f;
    float ms = -1.f;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) return -1.f;
    return ms;
} ZPQ_CATCH(return -1.f)

static int get_dev_model(zpq_ctx *c, const zpq_model *m, const DModel &layout, uint32_t sparse_cap, DevModel *out)
{
    const uint64_t key = (m->id << 32) | (uint64_t)sparse_cap;
    auto it = c->models.find(key);
    if (it != c->models.end()) { *out = it->second; return ZPQ_OK; }
    DevModel dm;
    HIPCK(hipMalloc((void **)&dm.d_model, sizeof(DModel)));
    HIPCK(hipMalloc((void **)&dm.d_img, m->img.size() * 4 + 4));
    HIPCK(hipMemcpy(dm.d_model, &layout, sizeof(DModel), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(dm.d_img, m->img.data(), m->img.size() * 4, hipMemcpyHostToDevice));
    c->models[key] = dm;
    *out = dm;
    return ZPQ_OK;
}

// ------------------------------------------------------------------ batch core (device pointers)
struct BatchArgs {
    BlockArrays io;                        // device pointers
    BatchExtras x;                         // (trace and ctx_out device pointers too; ctx_words is the host's business)
    const uint32_t *gate_flag = nullptr;   // striped upload (chain encode only): see DBatch
    uint32_t gate_pos = 0;
    uint32_t *prog_counter = nullptr;      // early download (chain decode only): see DBatch
    uint32_t prog_pos = 0;
};

// ---- knobs: each parsed in one place, and read when the call is made
// A request flag and its environment variable: NAME=1 sets the request for every call of the process, NAME=0 clears it,
// anything but a leading '0' or '1' decides nothing (ZPQ_VM_PIPE, ZPQ_SET_LANES / _PIPE / _WAVES / _VMWAVES).
static bool request(const char *var, uint32_t flags, uint32_t bit)
{
    const char *ev = getenv(var);
    const bool env = ev && (ev[0] == '0' || ev[0] == '1');
    return env ? ev[0] == '1' : (flags & bit) != 0;
}
// ZPQ_DIRTY_LOG_CAP: entries per table of the dirty-line log (default 16384; 0 = no log, the kernels as they were)
static uint32_t dirty_log_cap()
{
    const char *ev = getenv("ZPQ_DIRTY_LOG_CAP");
    if (!ev || !*ev) return 16384u;
    const long v = atol(ev);
    return v <= 0 ? 0u : (v > (1l << 20) ? (1u << 20) : (uint32_t)v);
}
struct SparseKnobs {
    uint32_t forced_cap = 0;               // ZPQ_SPARSE_FORCE_LOG2 = 8 .. 25 (tests: exercise the store on small models), else 0
    bool never = false, always = false;    // ZPQ_SPARSE_MODE, a tuning knob: "never" / "always" (a forced capacity is "always")
};
static SparseKnobs sparse_knobs()
{
    SparseKnobs k;
    const char *ev = getenv("ZPQ_SPARSE_FORCE_LOG2");
    const int lg = ev ? atoi(ev) : 0;
    if (lg >= 8 && lg <= 25) k.forced_cap = 1u << lg;
    const char *mode = getenv("ZPQ_SPARSE_MODE");
    k.never = mode && !strcmp(mode, "never");
    k.always = k.forced_cap || (mode && !strcmp(mode, "always"));
    return k;
}
// ZPQ_FLAG_LINESTORE / ZPQ_LANES_STORE, a request: k_rows / k_lanes with the model's large hashed tables on the compact line
// store.  The layout it would run on at `cap` lines, from the model's shape alone: the lane kernels take the model, at least
// one ICM / ISSE table is larger than the store, and the compact slot stays below 4 GiB (the kernels hold a store's tags
// as a 32-bit distance from its lines).
static bool lanes_store_layout(const zpq_model *m, uint32_t cap, DModel *layout)
{
    return zpq_lanes_supported(&m->d) && zpq_sparse_layout(m->d, cap, layout) && layout->slot_bytes < (1ull << 32);
}
extern "C" int zpq_lanes_store_applies(const zpq_model *m, uint32_t cap_lines) try
{
    DModel layout;
    return m && lanes_store_layout(m, cap_lines, &layout) ? 1 : 0;
} ZPQ_CATCH(return 0)
extern "C" uint64_t zpq_lanes_store_slot_bytes(const zpq_model *m, uint32_t cap_lines) try
{
    DModel layout;
    return m && lanes_store_layout(m, cap_lines, &layout) ? layout.slot_bytes : 0;
} ZPQ_CATCH(return 0)
// a model the chain kernels take
static bool is_chain_model(const zpq_model *m) { return m->d.fast_kind && zpq_chain_blocks_per_wg(&m->d) > 0; }

// ---- the kernel families of a batch call
enum Family {
    F_CHAIN,                     // zpq_chain.hip (which chooses k_chain, k_pipe, k_dpipe ... itself)
    F_GENERIC,                   // lane 0 runs every component: any model, own slots, traces
    F_LANES,                     // up to 64 components: one block per wave, lane i = component i (k_rows / k_lanes)
    F_GPIPE, F_GDEC,             // lanes family, encode / decode: the wave-per-component pipeline and its decoder (zpq_gpipe.hip)
    F_VPIPE, F_VDEC,             // the same pair with an interpreter wave (k_vpipe / k_vdec), when asked for
    F_COUNT
};

// What a batch call will launch: kernel family, slot layout, resident slots and grid.
struct Plan {
    Family fam = F_GENERIC;
    uint32_t sp = 0;             // compact line store capacity (lines), 0 = dense tables
    DModel M;                    // layout the kernels see (dense or compact): the plan's own copy
    int nslots = 0, grid = 0, bpw = 0;
};

// One row per family: the name zpq_ctx_last_kernel_name reports per direction (null: the launcher says), the resident
// blocks per CU (null: the chain family plans its own grid, plan_chain) and the launcher behind one signature.
struct FamilyRow {
    const char *name[2];
    int (*blocks_per_cu)(const DModel *M);
    int (*launch)(const DBatch *B, const Plan &P, int decode, hipStream_t s, const char **name);
};
static const FamilyRow FAMILY[F_COUNT] = {
    /* F_CHAIN   */ {{nullptr, nullptr}, nullptr,
                     [](const DBatch *B, const Plan &P, int d, hipStream_t s, const char **n) { return zpq_launch_chain(B, &P.M, d, P.grid, P.bpw, s, n); }},
    /* F_GENERIC */ {{"k_generic<encode>", "k_generic<decode>"}, zpq_generic_blocks_per_cu,
                     [](const DBatch *B, const Plan &P, int d, hipStream_t s, const char **) { zpq_launch_generic(B, &P.M, d, P.grid, s); return (int)ZPQ_OK; }},
    /* F_LANES   */ {{nullptr, nullptr}, zpq_lanes_blocks_per_cu,
                     [](const DBatch *B, const Plan &P, int d, hipStream_t s, const char **n) { *n = zpq_lanes_kernel_name(&P.M, d); return zpq_launch_lanes(B, &P.M, d, P.nslots, s); }},
    /* F_GPIPE   */ {{"k_gpipe<encode>", nullptr}, zpq_gpipe_blocks_per_cu,
                     [](const DBatch *B, const Plan &P, int, hipStream_t s, const char **) { return zpq_launch_gpipe(B, &P.M, P.nslots, s); }},
    /* F_GDEC    */ {{nullptr, "k_gdec<decode>"}, zpq_gdec_blocks_per_cu,
                     [](const DBatch *B, const Plan &P, int, hipStream_t s, const char **) { return zpq_launch_gdec(B, &P.M, P.nslots, s); }},
    /* F_VPIPE   */ {{"k_vpipe<encode>", nullptr}, zpq_vpipe_blocks_per_cu,
                     [](const DBatch *B, const Plan &P, int, hipStream_t s, const char **) { return zpq_launch_vpipe(B, &P.M, P.nslots, s); }},
    /* F_VDEC    */ {{nullptr, "k_vdec<decode>"}, zpq_vdec_blocks_per_cu,
                     [](const DBatch *B, const Plan &P, int, hipStream_t s, const char **) { return zpq_launch_vdec(B, &P.M, P.nslots, s); }},
};

// resident slots / grid of the chain kernel for one slot layout
static int plan_chain(zpq_ctx *c, const DModel &M, int nblocks, int *nslots_out, int *grid_out, int *bpw_out)
{
    const uint64_t max_by_mem = M.slot_bytes ? (c->pool_budget() / M.slot_bytes) : (uint64_t)nblocks;
    if (max_by_mem == 0) return ZPQ_E_NOMEM;
    int bpw = 0;
    const uint64_t can_hold = max_by_mem < (uint64_t)nblocks ? max_by_mem : (uint64_t)nblocks;
    if (!zpq_chain_plan(&M, (int)can_hold, c->cus, &bpw)) return ZPQ_E_INTERNAL;
    int nwg = (nblocks + bpw - 1) / bpw;
    const int cap_wg = zpq_chain_max_wgs(&M, c->cus);
    if (nwg > cap_wg) nwg = cap_wg;
    int nslots = nwg * bpw;
    if ((uint64_t)nslots > max_by_mem) nslots = (int)max_by_mem;      // last workgroup partly idle
    if (nslots > nblocks) nslots = nblocks;
    *nslots_out = nslots;
    *grid_out = (nslots + bpw - 1) / bpw;
    *bpw_out = bpw;
    return ZPQ_OK;
}

static int plan_batch(zpq_ctx *c, const zpq_model *m, uint32_t flags, int nblocks, bool trace, bool own_slot, Plan *P, int decode = 0) try
{
    const bool pooled = !trace && !own_slot;
    const bool chain = pooled && !(flags & (ZPQ_FLAG_GENERIC | ZPQ_FLAG_LANES | ZPQ_FLAG_NOEOF | ZB_CTX_ONLY)) && is_chain_model(m);
    // everything else with up to 64 components: one block per wave, lane i = component i
    const bool lanes = !chain && pooled && !(flags & (ZPQ_FLAG_GENERIC | ZPQ_FLAG_NOEOF | ZB_CTX_ONLY | ZB_KEEP_STATE)) &&
                       zpq_lanes_supported(&m->d);
    P->sp = 0;
    P->M = m->d;
    int nslots, grid, bpw = 0;
    if (chain) {
        // Dense tables or the compact line store?  The store costs ~120 instructions per nibble and hashed
        // component, so it is used where it pays: when it lets the batch finish in fewer rounds of resident
        // blocks (levels 3-5 at scale, level 1 beyond ~6900 blocks), or when a dense slot is so large
        // (levels 4-5: 385 MiB / 2 GiB) that clearing it per block costs more than the store does.
        P->fam = F_CHAIN;
        int dn = 0, dg = 0, db = 0;
        const int rcd = plan_chain(c, m->d, nblocks, &dn, &dg, &db);
        const SparseKnobs K = sparse_knobs();
        const uint32_t cap = K.forced_cap ? K.forced_cap : c->sparse_cap;
        DModel sparse_layout;
        int sn = 0, sg = 0, sb = 0;
        bool use_sparse = false;
        if (!K.never && zpq_sparse_layout(m->d, cap, &sparse_layout) && plan_chain(c, sparse_layout, nblocks, &sn, &sg, &sb) == ZPQ_OK) {
            if (rcd != ZPQ_OK || K.always || m->d.slot_bytes > (256ull << 20)) use_sparse = true;
            else {
                const int rounds_d = (nblocks + dn - 1) / dn, rounds_s = (nblocks + sn - 1) / sn;
                use_sparse = rounds_s < rounds_d;
            }
        }
        if (use_sparse) { P->sp = cap; P->M = sparse_layout; nslots = sn; grid = sg; bpw = sb; }
        else {
            if (rcd != ZPQ_OK) return rcd;
            nslots = dn; grid = dg; bpw = db;
        }
    } else {
        // the line store on request (never by itself: EXPERIMENTS.md R20).  ZPQ_SPARSE_FORCE_LOG2 counts only under the request
        // here; a request that is not honoured decides nothing.  (zpq_block calls, ZB_NO_VMPIPE, make no requests.)
        if (lanes && !(flags & ZB_NO_VMPIPE) && request("ZPQ_LANES_STORE", flags, ZPQ_FLAG_LINESTORE)) {
            const SparseKnobs K = sparse_knobs();
            const uint32_t cap = K.forced_cap ? K.forced_cap : c->sparse_cap;
            DModel layout;
            if (!K.never && lanes_store_layout(m, cap, &layout)) { P->sp = cap; P->M = layout; }
        }
        const DModel &M = P->M;
        const uint64_t max_by_mem = M.slot_bytes ? (c->pool_budget() / M.slot_bytes) : (uint64_t)nblocks;
        if (max_by_mem == 0 && !own_slot) return ZPQ_E_NOMEM;
        nslots = nblocks;
        P->fam = F_GENERIC;
        if (lanes) {
            // the wave pipelines where the model is in their envelope; the pair with an interpreter wave only on request
            // (ZPQ_FLAG_VMPIPE / ZPQ_VM_PIPE; a zpq_block's first segment keeps its kernel: ZB_NO_VMPIPE)
            const bool vm_pipe = !(flags & ZB_NO_VMPIPE) && request("ZPQ_VM_PIPE", flags, ZPQ_FLAG_VMPIPE);
            if (P->sp) P->fam = F_LANES;                           // (the wave pipelines have no store)
            else if ((decode ? zpq_gdec_applies(&M) : zpq_gpipe_applies(&M)) != 0) P->fam = decode ? F_GDEC : F_GPIPE;
            else if (vm_pipe && (decode ? zpq_vdec_applies(&M) : zpq_vpipe_applies(&M)) != 0) P->fam = decode ? F_VDEC : F_VPIPE;
            else P->fam = F_LANES;
        }
        const int cap_res = c->cus * FAMILY[P->fam].blocks_per_cu(&M);
        if (nslots > cap_res) nslots = cap_res;
        if (!own_slot && (uint64_t)nslots > max_by_mem) nslots = (int)max_by_mem;
        grid = nslots;
    }
    if (own_slot) { nslots = 1; grid = 1; }
    P->nslots = nslots; P->grid = grid; P->bpw = bpw;
    return ZPQ_OK;
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

extern "C" int zpq_ctx_resident_capacity(zpq_ctx *c, const zpq_model *m, uint32_t flags) try
{
    if (!ctx_live(c) || !m) return ZPQ_E_ARG;
    // the largest batch that both directions code in ONE round (a general model's encoder -- a wave per component -- holds more
    // blocks per CU than its decoder)
    Plan P, Q;
    int rc = plan_batch(c, m, flags & 0xffu, 1 << 30, false, false, &P, 0);
    if (rc == ZPQ_OK) rc = plan_batch(c, m, flags & 0xffu, 1 << 30, false, false, &Q, 1);
    return rc != ZPQ_OK ? rc : (P.nslots < Q.nslots ? P.nslots : Q.nslots);
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

// a DBatch with the model, its image, the ctx's tables and the (device) arrays of the call
static DBatch batch_base(const zpq_ctx *c, const DevModel &dm, const BlockArrays &io)
{
    DBatch B;
    memset(&B, 0, sizeof B);
    B.model = dm.d_model; B.img = dm.d_img;
    B.squash = c->d_squash; B.stretch = c->d_stretch; B.dt = c->d_dt; B.dt2k = c->d_dt2k;
    B.ns = c->d_ns; B.stretch_c = c->d_stretch_c;
    B.nblocks = io.n; B.flags = io.flags;
    B.in = io.in; B.in_off = io.in_off; B.out = io.out; B.out_off = io.out_off;
    B.out_len = io.out_len; B.consumed = io.consumed; B.final_code = io.final_code;
    B.first_byte = io.first_byte; B.status = io.status;
    return B;
}

// a launch on stream s between the ctx's two timing events, with the last_* bookkeeping; launch(&name) queues it
template <class F> static int timed_launch(zpq_ctx *c, hipStream_t s, F &&launch)
{
    HIPCK(hipEventRecord(c->ev0, s));
    const char *name = nullptr;
    const int rc = launch(&name);
    if (rc != ZPQ_OK) return rc;
    c->last_name = name;
    HIPCK(hipGetLastError());
    HIPCK(hipEventRecord(c->ev1, s));
    c->ev_valid = true;
    return ZPQ_OK;
}
static int launch_family(zpq_ctx *c, const DBatch &B, const Plan &P, int decode, hipStream_t s)
{
    return timed_launch(c, s, [&](const char **name) {
        *name = FAMILY[P.fam].name[decode];
        return FAMILY[P.fam].launch(&B, P, decode, s, name);
    });
}

static int run_batch(zpq_ctx *c, const zpq_model *m, int decode, const BatchArgs &a)
{
    const BlockArrays &io = a.io;
    if (!ctx_live(c)) return c ? ZPQ_E_CLOSED : ZPQ_E_ARG;
    if (!m) return ZPQ_E_ARG;
    if (io.n < 0) return ZPQ_E_ARG;
    if (io.n == 0) return ZPQ_OK;
    if (!io.in_off || !io.out_off || !io.out_len || !io.status) return ZPQ_E_ARG;
    if (a.x.own_slot && io.n != 1) return ZPQ_E_ARG;
    HIPCK(hipSetDevice(c->device));
    Plan P;
    int rc = plan_batch(c, m, io.flags, io.n, a.x.trace != nullptr, a.x.own_slot != nullptr, &P, decode);
    if (rc != ZPQ_OK) return rc;
    DevModel dm;
    rc = get_dev_model(c, m, P.M, P.sp, &dm);
    if (rc != ZPQ_OK) return rc;

    DBatch B = batch_base(c, dm, io);
    B.trace = a.x.trace; B.ntrace = a.x.ntrace; B.ctx_out = a.x.ctx_out;
    B.gate_flag = (P.fam == F_CHAIN && !decode) ? a.gate_flag : nullptr;
    B.gate_pos = a.gate_pos;
    if (a.gate_flag && !B.gate_flag) return ZPQ_E_INTERNAL;      // (a gated upload must meet a kernel that honours the gate)
    B.prog_counter = (P.fam == F_CHAIN && decode) ? a.prog_counter : nullptr;   // (other kernels do not report: the host then copies after the kernel)
    B.prog_pos = a.prog_pos;

    B.nslots = P.nslots;
    if (a.x.own_slot) {
        B.slots = a.x.own_slot;
    } else {
        const size_t had = c->slots.cap;
        rc = c->slots.ensure((size_t)P.nslots * P.M.slot_bytes + 256);   // (the slack a MIX row read needs is part of slot_bytes: zpq_model.cpp mix_row_pad)
        if (c->slots.cap != had) c->dlog_drop();                 // (a new pool: nobody knows what is in it)
        if (rc != ZPQ_OK) return rc;
        B.slots = (uint8_t *)c->slots.p;
    }
    // The dirty-line log: offered to a launch that keeps it (the dense level-2 pair), whose slots then enter with a valid log
    // where the last launches on the pool kept it too, for this model, at this capacity.  Without room for the log the launch
    // runs as it always did.
    bool logged = false;
    if (!a.x.own_slot) {
        const uint32_t cap = dirty_log_cap();
        if (cap && P.fam == F_CHAIN && !P.sp && zpq_chain_keeps_dlog(&B, &P.M, decode, P.bpw)) {
            const size_t had = c->dlog.cap;
            const int lrc = c->dlog.ensure((size_t)P.nslots * 3 * zpqdev::dlog_stride(cap) * 4);
            if (c->dlog.cap != had || cap != c->dlog_cap || dm.d_model != c->dlog_model) c->dlog_drop();
            if (lrc == ZPQ_OK) {
                logged = true;
                B.dlog = (uint32_t *)c->dlog.p; B.dlog_cap = cap; B.dlog_valid = c->dlog_valid;
            }
        }
    }
    c->last_slots = P.nslots;
    c->last_sp = P.sp;
    c->last_host = 0;                                            // (host_pipeline sets it when its batch is through)
    rc = launch_family(c, B, P, decode, c->stream);
    if (!a.x.own_slot) {
        if (rc != ZPQ_OK || !logged) c->dlog_drop();             // (a launch on fewer slots than are valid keeps the others valid)
        else {
            if (c->dlog_model != dm.d_model) c->dlog_layout = P.M;
            c->dlog_model = dm.d_model; c->dlog_cap = B.dlog_cap;
            c->dlog_valid = std::max(c->dlog_valid, P.nslots);
        }
    }
    return rc;
}

// debug (tests): apply the log-clear to the pool's first nslots slots and count the non-zero 16-byte words left in their
// zero_bytes -- 0 if the logs name every dirty line.  ZPQ_E_ARG unless that many slots hold valid logs.
extern "C" int zpq_debug_pool_residue(zpq_ctx *c, int nslots, uint64_t *count) try
{
    if (!ctx_live(c) || !count || nslots < 1) return ZPQ_E_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (nslots > c->dlog_valid || !c->dlog_model || !c->dlog.p || !c->slots.p) return ZPQ_E_ARG;
    HIPCK(hipSetDevice(c->device));
    unsigned long long *d_count = nullptr;
    HIPCK(hipMalloc((void **)&d_count, 8));
    DBatch B;
    memset(&B, 0, sizeof B);
    B.model = c->dlog_model; B.slots = (uint8_t *)c->slots.p; B.nslots = nslots;
    B.dlog = (uint32_t *)c->dlog.p; B.dlog_cap = c->dlog_cap; B.dlog_valid = c->dlog_valid;
    int rc = ZPQ_OK;
    unsigned long long h = 0;
    if (hipMemsetAsync(d_count, 0, 8, c->stream) != hipSuccess) rc = ZPQ_E_NODEVICE;
    if (rc == ZPQ_OK) rc = zpq_launch_dlog_residue(&B, &c->dlog_layout, nslots, d_count, c->stream);
    if (rc == ZPQ_OK && (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h, d_count, 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                         hipStreamSynchronize(c->stream) != hipSuccess)) rc = ZPQ_E_NODEVICE;
    (void)hipFree(d_count);
    if (rc != ZPQ_OK) { c->dlog_drop(); return rc; }
    *count = h;
    return ZPQ_OK;
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

// debug (tests): the counts (word 0) of the logs of the pool's first nslots slots, three per slot, as the last launch left
// them: a strided copy and nothing else -- no kernel, nothing cleared, dlog_valid as it was.  ZPQ_E_ARG unless that many
// slots hold valid logs.
extern "C" int zpq_debug_dlog_counts(zpq_ctx *c, int nslots, uint32_t *counts) try
{
    if (!ctx_live(c) || !counts || nslots < 1) return ZPQ_E_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (nslots > c->dlog_valid || !c->dlog_model || !c->dlog.p) return ZPQ_E_ARG;
    HIPCK(hipSetDevice(c->device));
    const size_t pitch = (size_t)zpqdev::dlog_stride(c->dlog_cap) * 4;
    HIPCK(hipMemcpy2DAsync(counts, 4, c->dlog.p, pitch, 4, (size_t)nslots * 3, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return ZPQ_OK;
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

extern "C" int zpq_encode_blocks_dev(zpq_ctx *c, const zpq_model *m, int nblocks, const uint8_t *in,
                                     const uint64_t *in_off, uint32_t flags, uint8_t *out,
                                     const uint64_t *out_off, uint32_t *out_len, int32_t *status) try
{
    BatchArgs a;
    a.io = block_arrays(nblocks, in, in_off, flags & 0xffu, out, out_off, out_len, status);
    return run_batch(c, m, 0, a);
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

extern "C" int zpq_decode_blocks_dev(zpq_ctx *c, const zpq_model *m, int nblocks, const uint8_t *in,
                                     const uint64_t *in_off, uint32_t flags, uint8_t *out,
                                     const uint64_t *out_off, uint32_t *out_len, uint32_t *consumed,
                                     uint32_t *final_code, uint32_t *first_byte, int32_t *status) try
{
    BatchArgs a;
    a.io = block_arrays(nblocks, in, in_off, flags & 0xffu, out, out_off, out_len, status, consumed, final_code, first_byte);
    return run_batch(c, m, 1, a);
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

// ------------------------------------------------------------------ host-pointer forms
// Staging a window of nb blocks in a set, in three steps with the caller's upload of the bytes between the last two:
// room on both sides; the offsets relative to the window (stage_offsets, or the caller's own packing); then the
// offsets go up, status := -1 and the results := 0.
static int stage_room(StageSet &S, int nb, size_t in_bytes, size_t out_bytes, size_t misc_bytes)
{
    int rc;
    const size_t offb = (size_t)(nb + 1) * 8, u32b = (size_t)nb * 4;
    if ((rc = S.in.ensure(in_bytes + 16)) || (rc = S.out.ensure(out_bytes + 16)) || (rc = S.inoff.ensure(offb)) ||
        (rc = S.outoff.ensure(offb)) || (rc = S.dstoff.ensure(offb)) || (rc = S.meta.ensure(u32b * 4)) || (rc = S.status.ensure(u32b)) ||
        (rc = S.misc.ensure(misc_bytes)) || (rc = S.ensure_host((size_t)nb)))
        return rc;
    return ZPQ_OK;
}
static void stage_offsets(StageSet &S, const BlockArrays &h)
{
    uint64_t *h_in = S.h_in(), *h_out = S.h_out(h.n), *h_dst = S.h_dst(h.n);
    for (int k = 0; k <= h.n; k++) { h_in[k] = h.in_off[k] - h.in_off[0]; h_out[k] = h.out_off[k] - h.out_off[0]; h_dst[k] = h.out_off[k]; }
}
// dst: the absolute destination offsets as well (k_gather packs into the caller's slabs)
static int stage_upload(StageSet &S, int nb, hipStream_t s, bool dst)
{
    const size_t offb = (size_t)(nb + 1) * 8, u32b = (size_t)nb * 4;
    HIPCK(hipMemcpyAsync(S.inoff.p, S.h_in(), offb, hipMemcpyHostToDevice, s));
    HIPCK(hipMemcpyAsync(S.outoff.p, S.h_out(nb), offb, hipMemcpyHostToDevice, s));
    if (dst) HIPCK(hipMemcpyAsync(S.dstoff.p, S.h_dst(nb), offb, hipMemcpyHostToDevice, s));
    HIPCK(hipMemsetAsync(S.status.p, 0xff, u32b, s));          // -1: "kernel never reported"
    HIPCK(hipMemsetAsync(S.meta.p, 0, u32b * 4, s));
    return ZPQ_OK;
}
// Handing the small results back: queue their download into the set's pinned arrays ...
static int fetch_results(StageSet &S, int b0, int nb, hipStream_t s)
{
    HIPCK(hipMemcpyAsync(S.h_meta, S.meta.p, (size_t)nb * 16, hipMemcpyDeviceToHost, s));
    HIPCK(hipMemcpyAsync(S.h_meta + 4 * (size_t)nb, S.status.p, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
    S.b0 = b0; S.n = nb;
    return ZPQ_OK;
}
// ... and, once that has run, give them to the caller's arrays: the window's block j is the caller's at[j] (null: b0 + j)
static void deliver(StageSet &S, const BlockArrays &h, int decode, const int *at = nullptr)
{
    const size_t nn = (size_t)S.n;
    for (size_t j = 0; j < nn; j++) {
        const size_t i = at ? (size_t)at[j] : (size_t)S.b0 + j;
        h.out_len[i] = S.h_meta[j];
        if (decode && h.consumed) h.consumed[i] = S.h_meta[nn + j];
        if (decode && h.final_code) h.final_code[i] = S.h_meta[2 * nn + j];
        if (decode && h.first_byte) h.first_byte[i] = S.h_meta[3 * nn + j];
        h.status[i] = (int32_t)S.h_meta[4 * nn + j];
    }
    S.n = 0;
}

static int host_pipeline(zpq_ctx *c, const zpq_model *m, int decode, const BlockArrays &h);
static int host_batch(zpq_ctx *c, const zpq_model *m, int decode, const BlockArrays &h, const BatchExtras &x = BatchExtras())
{
    if (!ctx_live(c)) return c ? ZPQ_E_CLOSED : ZPQ_E_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    c->last_host = 0;                                            // (whatever becomes of this call: host_pipeline sets it at its end)
    if (!m || h.n < 0) return ZPQ_E_ARG;
    if (h.n == 0) return ZPQ_OK;
    if (!h.in_off || !h.out_off || !h.out_len || !h.status) return ZPQ_E_ARG;
    if (!slabs_valid(h)) return ZPQ_E_ARG;
    HIPCK(hipSetDevice(c->device));
    if (h.n >= 2 && !x.own_slot && !x.trace && !x.ctx_out) return host_pipeline(c, m, decode, h);
    // One block (and the own_slot / trace / ctx_out forms): the window in[in_off[0] .. in_off[n]) alone goes up, the kernel
    // sees offsets relative to it, and what it produced comes back to out + out_off[0] -- as host_pipeline does per round.
    StageSet &S = c->one;
    hipStream_t s = c->stream;
    const size_t win_in = (size_t)h.in_bytes(), win_out = (size_t)h.out_bytes();
    const size_t misc_bytes = (x.trace ? (size_t)x.ntrace * 4 : 0) + x.ctx_words * 4 + 16;
    int rc = stage_room(S, h.n, win_in, win_out, misc_bytes);
    if (rc != ZPQ_OK) return rc;
    stage_offsets(S, h);
    if (win_in) HIPCK(hipMemcpyAsync(S.in.p, h.in + h.in_off[0], win_in, hipMemcpyHostToDevice, s));
    if ((rc = stage_upload(S, h.n, s, false)) != ZPQ_OK) return rc;
    if (misc_bytes > 16) HIPCK(hipMemsetAsync(S.misc.p, 0, misc_bytes, s));
    BatchArgs a;
    a.io = S.device_view(h.n, h.flags, decode);
    a.x.own_slot = x.own_slot;
    if (x.trace) { a.x.trace = (int32_t *)S.misc.p; a.x.ntrace = x.ntrace; }
    if (x.ctx_out) a.x.ctx_out = (uint32_t *)S.misc.p;
    rc = run_batch(c, m, decode, a);
    if (rc != ZPQ_OK) return rc;
    if ((rc = fetch_results(S, 0, h.n, s)) != ZPQ_OK) return rc;
    uint8_t *const dst = win_out ? h.out + h.out_off[0] : nullptr;
    if (win_out && h.n == 1) {
        // one segment (zpq_block_*): its slab is sized for the worst case; move only what was produced
        HIPCK(hipStreamSynchronize(s));
        const size_t got = S.h_meta[0] < win_out ? S.h_meta[0] : win_out;
        if (got) HIPCK(hipMemcpyAsync(dst, S.out.p, got, hipMemcpyDeviceToHost, s));
    } else if (win_out) HIPCK(hipMemcpyAsync(dst, S.out.p, win_out, hipMemcpyDeviceToHost, s));
    if (x.trace) HIPCK(hipMemcpyAsync(x.trace, S.misc.p, (size_t)x.ntrace * 4, hipMemcpyDeviceToHost, s));
    if (x.ctx_out) HIPCK(hipMemcpyAsync(x.ctx_out, S.misc.p, x.ctx_words * 4, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    deliver(S, h, decode);
    return ZPQ_OK;
}

// ------------------------------------------------------------------ pinned host memory + pipelined host batches
extern "C" void *zpq_host_alloc(size_t bytes) try
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
} ZPQ_CATCH(return nullptr)
extern "C" void zpq_host_free(void *p) try
{
    if (p) (void)hipHostFree(p);
} ZPQ_CATCH(return)

// device-visible address of a host buffer if it is pinned (zpq_host_alloc / hipHostMalloc / hipHostRegister), else null
static void *pinned_device_ptr(const void *p)
{
    if (!p) return nullptr;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (at.type != hipMemoryTypeHost) return nullptr;
    void *d = nullptr;
    if (hipHostGetDevicePointer(&d, const_cast<void *>(p), 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return d;
}

__global__ void __launch_bounds__(256) k_gather(const uint8_t *src, const uint64_t *src_off, const uint32_t *len,
                                                uint8_t *dst, const uint64_t *dst_off, int n, uint32_t skip, int slabs);

// Batches of two or more blocks through host pointers, in ROUNDS of at most the resident capacity: round r+1 is
// uploaded and round r-1 downloaded while round r is coded (three streams, two staging sets).  What replaces the
// reference's sequential loop over files (cmd/main.v:283-311: read, compress, write, next file) keeps that order per
// block but moves the three phases of different rounds in parallel.  With PINNED caller buffers (zpq_host_alloc)
// uploads are plain DMA and the output is packed by the GPU straight into the caller's slabs -- only bytes that
// were produced cross PCIe; with pageable buffers the runtime's staged copies are used and whole slabs come back.
static int host_pipeline(zpq_ctx *c, const zpq_model *m, int decode, const BlockArrays &h)
{
    const int nblocks = h.n;
    const uint8_t *const in = h.in;
    uint8_t *const out = h.out;
    HIPCK(hipSetDevice(c->device));
    c->last_host = 0;
    Plan P0;
    int rc = plan_batch(c, m, h.flags, nblocks, false, false, &P0, decode);
    if (rc != ZPQ_OK) return rc;
    // striped upload / early download: a single round of the dense short chains (the kernels that honour the gate)
    const bool hio = P0.fam == F_CHAIN && !P0.sp && zpq_chain_has_hio(&m->d) && !getenv("ZPQ_NO_STRIPE");
    // Rounds only where overlapping transfers with coding can pay: a batch that exceeds the resident capacity AND
    // moves a sizeable amount of data.  Smaller batches go as one launch (blocks beyond the capacity are worked off
    // by the resident groups in turn, inside the kernel).
    uint64_t min_bytes = 64ull << 20;
    if (const char *ev = getenv("ZPQ_PIPE_MIN_BYTES")) min_bytes = strtoull(ev, nullptr, 0);   // tests: force rounds on small data
    const bool big = h.in_bytes() + h.out_bytes() >= min_bytes;
    const int per_round = (big && P0.nslots > 0) ? P0.nslots : nblocks;
    uint8_t *const out_dev_view = (uint8_t *)pinned_device_ptr(out);           // non-null: the GPU can write the caller's slabs
    const bool in_pinned = pinned_device_ptr(in) != nullptr;                    // (hipMemcpyAsync takes either kind; pinned = true DMA)
    const int nrounds = (nblocks + per_round - 1) / per_round;
    c->pipe[0].n = c->pipe[1].n = 0;
    const uint32_t *gate_flag_dev = nullptr;
    uint64_t stripe_L = 0, early_L = 0;
    unsigned did = 0;                                                           // bit 0: striped upload, bit 1: early download
    uint32_t stripe_delay_us = 0;
    if (const char *ev = getenv("ZPQ_STRIPE_DELAY_US")) {                       // tests: lanes reach the gate before the second stripe is sent
        const unsigned long long v = strtoull(ev, nullptr, 0);
        stripe_delay_us = v > 500000ull ? 500000u : (uint32_t)v;
    }
    for (int r = 0; r < nrounds; r++) {
        StageSet &S = c->pipe[r & 1];
        const int b0 = r * per_round, b1 = (b0 + per_round < nblocks) ? b0 + per_round : nblocks, n = b1 - b0;
        if (r >= 2) { HIPCK(hipEventSynchronize(S.ev_out)); deliver(S, h, decode); }   // the set's previous round has left the device
        const BlockArrays w = h.window(b0, b1);
        const uint64_t in_base = w.in_off[0], in_bytes = w.in_bytes(), out_base = w.out_off[0], out_bytes = w.out_bytes();
        if ((rc = stage_room(S, n, in_bytes, out_bytes, 0)) != ZPQ_OK) return rc;
        stage_offsets(S, w);
        const uint64_t *h_in = S.h_in(), *h_out = S.h_out(n);
        // ---- upload on the copy-in stream
        // One round cannot overlap its upload with its own coding by rounds -- every block starts at once.  But an
        // encoder needs a block's bytes only as it gets to them (64 KiB take ~200 ms), so for a single round of equally
        // long blocks from pinned memory the upload is STRIPED: the first 8 KiB of every block go first, the kernel
        // starts, the rest follows while it runs; a lane that reaches the end of the first stripe waits for *h_gate.
        bool striped = false;
        const uint64_t stripe = 8192;
        if (!decode && nrounds == 1 && in_pinned && hio && n >= 64) {
            const uint64_t L = h_in[1] - h_in[0];
            striped = L >= 4 * stripe && (L & 3u) == 0;
            for (int k = 1; k < n && striped; k++) striped = h_in[k + 1] - h_in[k] == L;
            if (striped) {
                void *gate_dev = nullptr;
                if (hipHostGetDevicePointer(&gate_dev, c->h_gate, 0) != hipSuccess) { (void)hipGetLastError(); striped = false; }
                else {
                    __atomic_store_n(c->h_gate, 0u, __ATOMIC_RELEASE);
                    HIPCK(hipMemcpy2DAsync(S.in.p, L, in + in_base, L, stripe, (size_t)n, hipMemcpyHostToDevice, c->s_h2d));
                    gate_flag_dev = (const uint32_t *)gate_dev;
                    stripe_L = L;
                }
            }
        }
        if (!striped && in_bytes) HIPCK(hipMemcpyAsync(S.in.p, in + in_base, in_bytes, hipMemcpyHostToDevice, c->s_h2d));
        if ((rc = stage_upload(S, n, c->s_h2d, true)) != ZPQ_OK) return rc;
        HIPCK(hipEventRecord(S.ev_in, c->s_h2d));
        // ---- code on the compute stream
        HIPCK(hipStreamWaitEvent(c->stream, S.ev_in, 0));
        BatchArgs a;
        a.io = S.device_view(n, h.flags, decode);
        if (striped) { a.gate_flag = gate_flag_dev; a.gate_pos = (uint32_t)stripe; }
        // The mirror image for a decoder's output: every block reports when its first `early` bytes are stored (and
        // visible to the copy engines); once all have, that stripe is copied out beside the kernel, which still has
        // the last quarter of every block to decode.  Single round, pinned slabs of equal length and stride.
        uint32_t early = 0;
        uint32_t *prog_dev = nullptr;
        if (decode && nrounds == 1 && out_dev_view && hio && n >= 64) {
            const uint64_t L = h_out[1] - h_out[0];
            bool uni = L >= 16384 && L <= 0x7FFFFFFFull;
            for (int k = 1; k < n && uni; k++) uni = h_out[k + 1] - h_out[k] == L;
            void *pd = nullptr;
            if (uni && hipHostGetDevicePointer(&pd, c->h_gate + 8, 0) == hipSuccess) {
                early = (uint32_t)(L / 4 * 3) & ~255u;
                prog_dev = (uint32_t *)pd;
                __atomic_store_n(c->h_gate + 8, 0u, __ATOMIC_RELEASE);
                a.prog_counter = prog_dev; a.prog_pos = early;
                early_L = L;
            } else (void)hipGetLastError();
        }
        rc = run_batch(c, m, decode, a);
        if (striped) {
            // the rest of every block, beside the running kernel; then the signal (whatever happened: a kernel left
            // waiting for it would only end at its spin limit)
            if (rc == ZPQ_OK && stripe_delay_us) {
                struct timespec ts = {(time_t)(stripe_delay_us / 1000000u), (long)(stripe_delay_us % 1000000u) * 1000L};
                nanosleep(&ts, nullptr);
            }
            hipError_t e2 = rc == ZPQ_OK ? hipMemcpy2DAsync((uint8_t *)S.in.p + stripe, stripe_L, in + in_base + stripe, stripe_L, stripe_L - stripe,
                                                            (size_t)n, hipMemcpyHostToDevice, c->s_h2d) : hipSuccess;
            if (e2 == hipSuccess) e2 = hipStreamSynchronize(c->s_h2d);
            __atomic_store_n(c->h_gate, 1u, __ATOMIC_RELEASE);
            if (e2 != hipSuccess && rc == ZPQ_OK) { (void)hipDeviceSynchronize(); return ZPQ_E_NODEVICE; }
        }
        if (rc != ZPQ_OK) { (void)hipDeviceSynchronize(); return rc; }
        if (striped) did |= 1u;
        HIPCK(hipEventRecord(S.ev_k, c->stream));
        uint32_t skip = 0;
        if (prog_dev) {
            // wait (politely) until every block has reported, or the kernel has ended without all reports (a kernel
            // family that does not report, an error): then nothing was copied early and everything goes the usual way
            for (;;) {
                if (__atomic_load_n(c->h_gate + 8, __ATOMIC_ACQUIRE) >= (uint32_t)n) { skip = early; break; }
                if (hipEventQuery(S.ev_k) == hipSuccess) { skip = __atomic_load_n(c->h_gate + 8, __ATOMIC_ACQUIRE) >= (uint32_t)n ? early : 0; break; }
                (void)hipGetLastError();
                struct timespec ts = {0, 50000};
                nanosleep(&ts, nullptr);
            }
            if (skip) did |= 2u;
            if (skip) HIPCK(hipMemcpy2DAsync(out + out_base, early_L, S.out.p, early_L, skip, (size_t)n, hipMemcpyDeviceToHost, c->s_d2h));
        }
        // ---- download on the copy-out stream
        HIPCK(hipStreamWaitEvent(c->s_d2h, S.ev_k, 0));
        if ((rc = fetch_results(S, b0, n, c->s_d2h)) != ZPQ_OK) return rc;
        if (out_bytes) {
            if (out_dev_view) {
                // the GPU packs each block's produced bytes straight into the caller's (pinned) slab
                hipLaunchKernelGGL(k_gather, dim3(n), dim3(256), 0, c->s_d2h, (const uint8_t *)S.out.p, (const uint64_t *)S.outoff.p,
                                   (const uint32_t *)S.meta.p, out_dev_view, (const uint64_t *)S.dstoff.p, n, skip, 1);
                HIPCK(hipGetLastError());
            } else {
                // pageable destination: the runtime stages this copy and the call returns only when it has run, so
                // with pageable slabs rounds do not overlap (use zpq_host_alloc)
                HIPCK(hipMemcpyAsync(out + out_base, S.out.p, out_bytes, hipMemcpyDeviceToHost, c->s_d2h));
            }
        }
        HIPCK(hipEventRecord(S.ev_out, c->s_d2h));
    }
    HIPCK(hipStreamSynchronize(c->s_d2h));
    HIPCK(hipStreamSynchronize(c->stream));
    deliver(c->pipe[nrounds & 1], h, decode);                                  // (older round first)
    deliver(c->pipe[(nrounds + 1) & 1], h, decode);
    c->last_host = did | ((unsigned)nrounds << 8);
    return ZPQ_OK;
}

extern "C" int zpq_encode_blocks(zpq_ctx *c, const zpq_model *m, int nblocks, const uint8_t *in,
                                 const uint64_t *in_off, uint32_t flags, uint8_t *out,
                                 const uint64_t *out_off, uint32_t *out_len, int32_t *status) try
{
    return host_batch(c, m, 0, block_arrays(nblocks, in, in_off, flags & 0xffu, out, out_off, out_len, status));
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

extern "C" int zpq_decode_blocks(zpq_ctx *c, const zpq_model *m, int nblocks, const uint8_t *in,
                                 const uint64_t *in_off, uint32_t flags, uint8_t *out,
                                 const uint64_t *out_off, uint32_t *out_len, uint32_t *consumed,
                                 uint32_t *final_code, uint32_t *first_byte, int32_t *status) try
{
    return host_batch(c, m, 1, block_arrays(nblocks, in, in_off, flags & 0xffu, out, out_off, out_len, status, consumed, final_code, first_byte));
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

// ------------------------------------------------------------------ several GPUs behind one call
// Blocks are independent (compressor.v:90,147-148: fresh Predictor/ZPAQL per block), so any static deal gives the same
// bytes.  Context g takes the g-th contiguous share -- contiguous so that its PCIe transfers are -- on its own host
// thread (one host thread per device, no cross-device step but the caller's own buffers).
static int multi_batch(zpq_ctx *const *ctxs, int nctx, const zpq_model *m, int decode, const BlockArrays &h)
{
    const int nblocks = h.n;
    if (!ctxs || nctx <= 0 || !m || nblocks < 0) return ZPQ_E_ARG;
    for (int g = 0; g < nctx; g++) if (!ctxs[g]) return ZPQ_E_ARG;
    if (nblocks == 0) return ZPQ_OK;
    if (!h.in_off || !h.out_off || !h.out_len || !h.status) return ZPQ_E_ARG;
    const int G = nctx < nblocks ? nctx : nblocks;
    std::vector<int> rcs((size_t)G, ZPQ_OK);
    std::vector<std::thread> th;
    for (int g = 0; g < G; g++) {
        const int b0 = (int)((int64_t)nblocks * g / G), b1 = (int)((int64_t)nblocks * (g + 1) / G);
        th.emplace_back([=, &rcs]() {
            rcs[(size_t)g] = host_batch(ctxs[g], m, decode, h.window(b0, b1));
        });
    }
    for (std::thread &t : th) t.join();
    for (int r : rcs) if (r != ZPQ_OK) return r;
    return ZPQ_OK;
}

extern "C" int zpq_encode_blocks_multi(zpq_ctx *const *ctxs, int nctx, const zpq_model *m, int nblocks, const uint8_t *in,
                                       const uint64_t *in_off, uint32_t flags, uint8_t *out, const uint64_t *out_off,
                                       uint32_t *out_len, int32_t *status) try
{
    return multi_batch(ctxs, nctx, m, 0, block_arrays(nblocks, in, in_off, flags & 0xffu, out, out_off, out_len, status));
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

extern "C" int zpq_decode_blocks_multi(zpq_ctx *const *ctxs, int nctx, const zpq_model *m, int nblocks, const uint8_t *in,
                                       const uint64_t *in_off, uint32_t flags, uint8_t *out, const uint64_t *out_off,
                                       uint32_t *out_len, uint32_t *consumed, uint32_t *final_code, uint32_t *first_byte,
                                       int32_t *status) try
{
    return multi_batch(ctxs, nctx, m, 1, block_arrays(nblocks, in, in_off, flags & 0xffu, out, out_off, out_len, status, consumed, final_code, first_byte));
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

// ------------------------------------------------------------------ slab compaction
// out_len[b] bytes of each capacity-strided output slab -> one dense buffer, so that only real
// payload bytes cross PCIe.  One workgroup per block: bytes up to the destination's first 16-byte
// boundary, then 16-byte stores fed by two aligned 16-byte loads funnel-shifted to the source's
// misalignment, then the tail.
// skip: leave out the first `skip` bytes of every block (they have been copied already)
// slabs: src_off has n + 1 entries and block b holds at most src_off[b + 1] - src_off[b] bytes, whatever len[b] says
// (host_pipeline: a block whose slab was too small reports the length it needed, or cap + 1)
__global__ void __launch_bounds__(256) k_gather(const uint8_t *src, const uint64_t *src_off, const uint32_t *len,
                                                uint8_t *dst, const uint64_t *dst_off, int n, uint32_t skip, int slabs)
{
    const int b = blockIdx.x;
    if (b >= n) return;
    uint32_t have = len[b];
    if (slabs) {
        const uint64_t cap = src_off[b + 1] - src_off[b];
        if (have > cap) have = (uint32_t)cap;
    }
    if (have <= skip) return;
    const uint8_t *s = src + src_off[b] + skip;
    uint8_t *d = dst + dst_off[b] + skip;
    const uint32_t L = have - skip;
    uint32_t head = (uint32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(d) & 15u)) & 15u);
    if (head > L) head = L;
    for (uint32_t i = threadIdx.x; i < head; i += 256) d[i] = s[i];
    const uint32_t nvec = (L - head) / 16u;
    const uint8_t *sv = s + head;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(sv) & 3u);      // source byte offset inside its dword
    const uint32_t *s4 = reinterpret_cast<const uint32_t *>(sv - mis);
    uint4 *d16 = reinterpret_cast<uint4 *>(d + head);
    const uint32_t sh = mis * 8u;
    for (uint32_t v = threadIdx.x; v < nvec; v += 256) {
        const uint32_t *q = s4 + 4u * v;
        const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
        uint4 o;
        if (mis == 0) { o = make_uint4(w0, w1, w2, w3); }
        else {
            const uint32_t w4 = q[4];                       // in bounds: mis > 0 means bytes of the 5th dword belong to this vector
            o.x = (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh);
            o.y = (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh);
            o.z = (uint32_t)((((uint64_t)w3 << 32) | w2) >> sh);
            o.w = (uint32_t)((((uint64_t)w4 << 32) | w3) >> sh);
        }
        d16[v] = o;
    }
    for (uint32_t i = head + nvec * 16u + threadIdx.x; i < L; i += 256) d[i] = s[i];
}

extern "C" int zpq_gather_dev(zpq_ctx *c, int nblocks, const uint8_t *src, const uint64_t *src_off, const uint32_t *len,
                              uint8_t *dst, const uint64_t *dst_off) try
{
    if (!ctx_live(c)) return c ? ZPQ_E_CLOSED : ZPQ_E_ARG;
    if (nblocks < 0) return ZPQ_E_ARG;
    if (nblocks == 0) return ZPQ_OK;
    if (!src_off || !len || !dst_off) return ZPQ_E_ARG;
    HIPCK(hipSetDevice(c->device));
    hipLaunchKernelGGL(k_gather, dim3(nblocks), dim3(256), 0, c->stream, src, src_off, len, dst, dst_off, nblocks, 0u, 0);
    return hipGetLastError() == hipSuccess ? ZPQ_OK : ZPQ_E_INTERNAL;
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

// ------------------------------------------------------------------ SHA-1 side kernel (sha1.v:6-146)
extern "C" int zpq_sha1_blocks_dev(zpq_ctx *c, int nblocks, const uint8_t *in, const uint64_t *in_off, uint8_t *out20) try
{
    if (!ctx_live(c)) return c ? ZPQ_E_CLOSED : ZPQ_E_ARG;
    if (nblocks < 0) return ZPQ_E_ARG;
    if (nblocks == 0) return ZPQ_OK;
    if (!in_off || !out20) return ZPQ_E_ARG;
    HIPCK(hipSetDevice(c->device));
    return zpq_launch_sha1(in, in_off, in_off + 1, nblocks, out20, c->stream);
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

extern "C" int zpq_sha1_ranges_dev(zpq_ctx *c, int nranges, const uint8_t *in, const uint64_t *begin, const uint64_t *end, uint8_t *out20) try
{
    if (!ctx_live(c)) return c ? ZPQ_E_CLOSED : ZPQ_E_ARG;
    if (nranges < 0) return ZPQ_E_ARG;
    if (nranges == 0) return ZPQ_OK;
    if (!begin || !end || !out20) return ZPQ_E_ARG;
    HIPCK(hipSetDevice(c->device));
    return zpq_launch_sha1(in, begin, end, nranges, out20, c->stream);
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

extern "C" int zpq_sha1_blocks(zpq_ctx *c, int nblocks, const uint8_t *in, const uint64_t *in_off, uint8_t *out20) try
{
    if (!ctx_live(c)) return c ? ZPQ_E_CLOSED : ZPQ_E_ARG;
    if (nblocks < 0) return ZPQ_E_ARG;
    if (nblocks == 0) return ZPQ_OK;
    if (!in_off || !out20) return ZPQ_E_ARG;
    BlockArrays h;
    h.n = nblocks; h.in = in; h.in_off = in_off;
    if (!slabs_valid(h, false)) return ZPQ_E_ARG;
    const size_t base = (size_t)in_off[0], in_bytes = (size_t)h.in_bytes();
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCK(hipSetDevice(c->device));
    // (no results but the digests: the one-shot set lends its in / inoff / out buffers, nothing of stage_upload applies)
    StageSet &S = c->one;
    int rc;
    const size_t offb = (size_t)(nblocks + 1) * 8;
    if ((rc = S.in.ensure(in_bytes + 16)) || (rc = S.inoff.ensure(offb)) || (rc = S.out.ensure((size_t)nblocks * 20)))
        return rc;
    std::vector<uint64_t> rel((size_t)nblocks + 1);
    for (int b = 0; b <= nblocks; b++) rel[b] = in_off[b] - base;
    hipStream_t s = c->stream;
    if (in_bytes) HIPCK(hipMemcpyAsync(S.in.p, in + base, in_bytes, hipMemcpyHostToDevice, s));
    HIPCK(hipMemcpyAsync(S.inoff.p, rel.data(), offb, hipMemcpyHostToDevice, s));
    rc = zpq_launch_sha1((const uint8_t *)S.in.p, (const uint64_t *)S.inoff.p, (const uint64_t *)S.inoff.p + 1, nblocks, (uint8_t *)S.out.p, s);
    if (rc != ZPQ_OK) return rc;
    HIPCK(hipMemcpyAsync(out20, S.out.p, (size_t)nblocks * 20, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    return ZPQ_OK;
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

// ------------------------------------------------------------------ one block, many segments
extern "C" int zpq_block_create(zpq_ctx *c, const zpq_model *m, zpq_block **out) try
{
    if (!out) return ZPQ_E_ARG;
    *out = nullptr;
    if (!ctx_live(c)) return c ? ZPQ_E_CLOSED : ZPQ_E_ARG;
    if (!m) return ZPQ_E_ARG;
    HIPCK(hipSetDevice(c->device));
    zpq_block *b = new (std::nothrow) zpq_block();
    if (!b) return ZPQ_E_NOMEM;
    b->ctx = c; b->model = m; b->fresh = true; b->slot = nullptr;
    if (hipMalloc((void **)&b->slot, m->d.slot_bytes) != hipSuccess) { (void)hipGetLastError(); delete b; return ZPQ_E_NOMEM; }
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        if (!live_set().count(c)) { (void)hipFree(b->slot); delete b; return ZPQ_E_CLOSED; }
        c->children.push_back(b);
    }
    zpq_model_retain(m);
    *out = b;
    return ZPQ_OK;
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

extern "C" void zpq_block_destroy(zpq_block *b) try
{
    if (!b) return;
    zpq_ctx *c = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        c = b->ctx;                                         // nullptr: the ctx went first and took the slot with it
        if (c) c->children.erase(std::remove(c->children.begin(), c->children.end(), b), c->children.end());
        b->ctx = nullptr;
    }
    if (c) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        if (b->slot) (void)hipFree(b->slot);
    }
    zpq_model_release(b->model);
    delete b;
} ZPQ_CATCH(return)

// replay the first segment into b->slot (see zpq_block): encode with no output room -- the coder only counts
static int block_materialise(zpq_block *b)
{
    if (!b->ctx) return ZPQ_E_CLOSED;
    if (!b->lazy) return ZPQ_OK;
    const uint64_t in_off[2] = {0, b->lazy_in.size()}, out_off[2] = {0, 0};
    uint32_t olen = 0;
    int32_t st = 0;
    uint8_t dummy = 0;
    BatchExtras x;
    x.own_slot = b->slot;
    const int rc = host_batch(b->ctx, b->model, 0, block_arrays(1, b->lazy_in.data(), in_off, b->lazy_flags | ZPQ_FLAG_GENERIC, &dummy, out_off, &olen, &st), x);
    if (rc != ZPQ_OK) return rc;
    if (st != ZPQ_OK && st != ZPQ_E_OVERFLOW) return st;
    b->lazy = false;
    b->lazy_in.clear();
    b->lazy_in.shrink_to_fit();
    return ZPQ_OK;
}

// One segment of a block, either direction.  `ran`: the call reached the device and r holds what it answered (the caller
// then fills its out parameters, whatever the status).
struct SegResult { uint32_t len = 0, consumed = 0, code = 0, first = 0xFFFFFFFFu; bool ran = false; };
static int block_segment(zpq_block *b, int decode, const uint8_t *in, size_t n, uint32_t flags, uint8_t *out, size_t cap, SegResult *r)
{
    if (!b->ctx) return ZPQ_E_CLOSED;                   // the block's ctx has been destroyed
    const uint64_t in_off[2] = {0, n}, out_off[2] = {0, cap};
    int32_t st = 0;
    BlockArrays h = block_arrays(1, in, in_off, flags & 0xffu & ~ZPQ_FLAG_LINESTORE, out, out_off, &r->len, &st);
    if (decode) { h.consumed = &r->consumed; h.final_code = &r->code; h.first_byte = &r->first; }
    if (!(b->fresh && !(flags & ZPQ_FLAG_GENERIC))) {
        // a later segment (or the generic kernel asked for): on the block's own slot
        if (int rcm = block_materialise(b)) return rcm;
        h.flags |= ZPQ_FLAG_GENERIC | (b->fresh ? 0u : ZB_KEEP_STATE);
        BatchExtras x;
        x.own_slot = b->slot;
        const int rc = host_batch(b->ctx, b->model, decode, h, x);
        if (rc != ZPQ_OK) return rc;
        r->ran = true;
        b->fresh = false;
        return st;
    }
    h.flags |= ZB_NO_VMPIPE;
    const int rc = host_batch(b->ctx, b->model, decode, h);
    if (rc != ZPQ_OK) return rc;
    r->ran = true;
    if (st != ZPQ_OK) return st;                        // nothing persisted: the block is still fresh, the caller may retry
    b->fresh = false;
    b->lazy = true;
    b->lazy_flags = flags & 0xffu & ~ZPQ_FLAG_LINESTORE;
    if (!decode) { b->lazy_in.assign(in, in + n); return ZPQ_OK; }
    // the symbols this segment coded: [PP byte] + output.  With ZPQ_FLAG_PP the first symbol came back in `first`
    // (0xFFFFFFFF = the stream ended before it); a later encode replays 0 as the PP byte, anything else literally.
    b->lazy_in.clear();
    if (flags & ZPQ_FLAG_PP) {
        if (r->first == 0xFFFFFFFFu) b->lazy_flags &= ~(uint32_t)ZPQ_FLAG_PP;
        else if (r->first != 0) { b->lazy_flags &= ~(uint32_t)ZPQ_FLAG_PP; b->lazy_in.push_back((uint8_t)r->first); }
    }
    b->lazy_in.insert(b->lazy_in.end(), out, out + r->len);
    return ZPQ_OK;
}

extern "C" int zpq_block_encode_segment(zpq_block *b, const uint8_t *in, size_t n, uint32_t flags,
                                        uint8_t *out, size_t cap, size_t *out_len) try
{
    if (!b || !out_len || (n && !in) || (cap && !out)) return ZPQ_E_ARG;
    SegResult r;
    const int rc = block_segment(b, 0, in, n, flags, out, cap, &r);
    if (r.ran) *out_len = r.len;
    return rc;
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

extern "C" int zpq_block_decode_segment(zpq_block *b, const uint8_t *in, size_t n, uint32_t flags,
                                        uint8_t *out, size_t cap, size_t *out_len, size_t *consumed,
                                        uint32_t *final_code, uint32_t *first_byte) try
{
    if (!b || !out_len || (n && !in) || (cap && !out)) return ZPQ_E_ARG;
    SegResult r;
    const int rc = block_segment(b, 1, in, n, flags, out, cap, &r);
    if (r.ran) {
        *out_len = r.len;
        if (consumed) *consumed = r.consumed;
        if (final_code) *final_code = r.code;
        if (first_byte) *first_byte = r.first;
    }
    return rc;
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

// ------------------------------------------------------------------ N blocks, many segments
// the layout a set of this model gets: the line store wherever a table is larger than a store sized for max_member_bytes
// (the slots are the set's for its whole life, so the smaller slot always pays), unless ZPQ_SPARSE_MODE=never
static bool set_layout(const zpq_ctx *c, const zpq_model *m, uint64_t max_member_bytes, DModel *layout, uint32_t *sp)
{
    *sp = 0;
    if (!is_chain_model(m)) { *layout = m->d; return false; }
    const SparseKnobs K = sparse_knobs();
    const uint32_t cap = K.forced_cap ? K.forced_cap : (max_member_bytes ? line_store_cap(c, max_member_bytes) : c->sparse_cap);
    if (!K.never && zpq_sparse_layout(m->d, cap, layout) && zpq_chain_blocks_per_wg(layout) > 0) *sp = cap;
    else *layout = m->d;
    return true;
}

// ZPQ_SET_LANES, a request: honoured where no chain kernel takes the model and the lane-per-component kernels do.  The
// environment variable ZPQ_SET_LANES=1 sets it for every set of the process, ZPQ_SET_LANES=0 clears it (anything but a
// leading '0' or '1' decides nothing, as with ZPQ_VM_PIPE).  Host logic only: no device is needed.
extern "C" int zpq_blockset_lanes_applies(const zpq_model *m) try
{
    return m && !is_chain_model(m) && zpq_lanes_supported(&m->d) ? 1 : 0;
} ZPQ_CATCH(return 0)
// ZPQ_SET_PIPE, a request of the same kind: honoured where the wave-pipelined encoder codes the model's chain (its five
// shapes); ZPQ_SET_PIPE=1 / =0 in the environment by the same rule.  No model can have both.
extern "C" int zpq_blockset_pipe_applies(const zpq_model *m) try
{
    return m && is_chain_model(m) && zpq_pipe_shape_applies(&m->d) ? 1 : 0;
} ZPQ_CATCH(return 0)
// ZPQ_SET_WAVES, a request on top of ZPQ_SET_LANES: honoured where that one is in force for the set and both wave-per-component
// kernels take the model (gpipe_cfg: the shape alone; ZPQ_ENC_GPIPE / ZPQ_DEC_GPIPE choose the kernel per call, not here).
// ZPQ_SET_WAVES=1 / =0 in the environment by the same rule, resolved on its own and then combined.
extern "C" int zpq_blockset_waves_applies(const zpq_model *m) try
{
    return zpq_blockset_lanes_applies(m) && zpq_gpipe_shape_applies(&m->d) && zpq_gdec_shape_applies(&m->d) ? 1 : 0;
} ZPQ_CATCH(return 0)
// ZPQ_SET_VMWAVES, the same request for the models whose HCOMP program is not the shipped hash chain: honoured where
// ZPQ_SET_LANES is in force and k_vpipe / k_vdec take the model (vpipe_cfg: the shape alone, one envelope for both directions).
// ZPQ_SET_VMWAVES=1 / =0 in the environment by the same rule.  No model can have both this and ZPQ_SET_WAVES: the hash chain
// decides between them.
extern "C" int zpq_blockset_vmwaves_applies(const zpq_model *m) try
{
    return zpq_blockset_lanes_applies(m) && zpq_vpipe_applies(&m->d) ? 1 : 0;
} ZPQ_CATCH(return 0)
extern "C" int zpq_blockset_resolve_flags(const zpq_model *m, uint32_t flags) try
{
    if (!m || (flags & ~(uint32_t)ZPQ_SET_ALL)) return ZPQ_E_ARG;
    const bool lanes = request("ZPQ_SET_LANES", flags, ZPQ_SET_LANES) && zpq_blockset_lanes_applies(m);
    const bool pipe = request("ZPQ_SET_PIPE", flags, ZPQ_SET_PIPE) && zpq_blockset_pipe_applies(m);
    const bool waves = lanes && request("ZPQ_SET_WAVES", flags, ZPQ_SET_WAVES) && zpq_blockset_waves_applies(m);
    const bool vmwaves = lanes && request("ZPQ_SET_VMWAVES", flags, ZPQ_SET_VMWAVES) && zpq_blockset_vmwaves_applies(m);
    // ZPQ_SET_CHUNKS, a request on top of ZPQ_SET_LANES with no environment variable (only a caller of the chunk calls can use
    // it): honoured wherever that one is in force, it decides nothing anywhere else
    const bool chunks = lanes && (flags & ZPQ_SET_CHUNKS) != 0;
    return (int)((lanes ? ZPQ_SET_LANES : 0u) | (pipe ? ZPQ_SET_PIPE : 0u) | (waves ? ZPQ_SET_WAVES : 0u) | (vmwaves ? ZPQ_SET_VMWAVES : 0u)
                 | (chunks ? ZPQ_SET_CHUNKS : 0u));
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

static int set_capacity(zpq_ctx *c, const DModel &layout, bool chain, bool lanes)
{
    const uint64_t by_mem = layout.slot_bytes ? c->pool_budget() / layout.slot_bytes : (1u << 20);
    // (the lane kernels have no dependency between workgroups: a launch may hold any number of members)
    if (lanes) return by_mem > (1u << 20) ? (1 << 20) : (int)by_mem;
    const uint64_t resident = chain ? (uint64_t)zpq_chain_max_wgs(&layout, c->cus) * (uint64_t)zpq_chain_blocks_per_wg(&layout)
                                    : (uint64_t)c->cus * (uint64_t)zpq_generic_blocks_per_cu(&layout);
    const uint64_t n = by_mem < resident ? by_mem : resident;
    return n > (1u << 20) ? (1 << 20) : (int)n;
}

extern "C" int zpq_blockset_capacity_ex(zpq_ctx *c, const zpq_model *m, uint64_t max_member_bytes, uint32_t flags) try
{
    if (flags & ~(uint32_t)ZPQ_SET_ALL) return ZPQ_E_ARG;
    if (!ctx_live(c)) return c ? ZPQ_E_CLOSED : ZPQ_E_ARG;
    if (!m) return ZPQ_E_ARG;
    HIPCK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mu);
    DModel layout;
    uint32_t sp = 0;
    const bool chain = set_layout(c, m, max_member_bytes, &layout, &sp);
    // (ZPQ_SET_PIPE changes nothing here: any round of such a set may fall back to the chain encoder; nor do ZPQ_SET_WAVES / _VMWAVES:
    // workgroups of the wave kernels do not wait for one another either, memory alone bounds the set)
    const int rf = zpq_blockset_resolve_flags(m, flags);
    return set_capacity(c, layout, chain, rf > 0 && ((uint32_t)rf & ZPQ_SET_LANES) != 0);
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

extern "C" int zpq_blockset_capacity(zpq_ctx *c, const zpq_model *m, uint64_t max_member_bytes) try
{
    return zpq_blockset_capacity_ex(c, m, max_member_bytes, 0);
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

extern "C" int zpq_blockset_create_ex(zpq_ctx *c, const zpq_model *m, int nmembers, uint64_t max_member_bytes, uint32_t flags, zpq_blockset **out) try
{
    if (!out) return ZPQ_E_ARG;
    *out = nullptr;
    if (flags & ~(uint32_t)ZPQ_SET_ALL) return ZPQ_E_ARG;
    if (!ctx_live(c)) return c ? ZPQ_E_CLOSED : ZPQ_E_ARG;
    if (!m || nmembers < 1) return ZPQ_E_ARG;
    HIPCK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mu);
    zpq_blockset *s = new (std::nothrow) zpq_blockset();
    if (!s) return ZPQ_E_NOMEM;
    s->chain = set_layout(c, m, max_member_bytes, &s->layout, &s->sp);
    s->flags = (uint32_t)zpq_blockset_resolve_flags(m, flags);
    const bool lanes = (s->flags & ZPQ_SET_LANES) != 0;
    s->nmembers = nmembers;
    s->bytes = (uint64_t)nmembers * s->layout.slot_bytes + 256;
    if (nmembers > set_capacity(c, s->layout, s->chain, lanes) || s->bytes > c->pool_budget()) { delete s; return ZPQ_E_NOMEM; }
    if (hipMalloc((void **)&s->slots, s->bytes) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(c->stream);
        c->slots.release();                                 // the idle slot pool makes room; it grows back on demand
        c->dlog.release();
        c->dlog_drop();
        if (hipMalloc((void **)&s->slots, s->bytes) != hipSuccess) { (void)hipGetLastError(); delete s; return ZPQ_E_NOMEM; }
    }
    int rc = ZPQ_OK;
    if (s->chain || lanes) {
        // Predictor.init + ZPAQL.clear of every member now: each launch on the set is KEEP, the first segment's included.
        // (A chain model -- ICM, ISSE, MIX2 -- has its zeroed part, ICM cm[] = cminit, ISSE weight pairs and MIX2 weights
        // 32768 to set, predictor.v:366-368,396,443-445: k_set_init's fill, whose ZF_CONST and MATCH cases find nothing.)
        DevModel dm;
        rc = get_dev_model(c, m, s->layout, s->sp, &dm);
        if (rc == ZPQ_OK) rc = zpq_launch_lanes_set_init(dm.d_model, dm.d_img, s->slots, nmembers, c->stream);
        if (rc == ZPQ_OK && (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)) rc = ZPQ_E_NODEVICE;
    }
    if (rc != ZPQ_OK) { (void)hipGetLastError(); (void)hipFree(s->slots); delete s; return rc; }
    s->failed.assign((size_t)nmembers, ZPQ_OK);
    s->fresh.assign((size_t)nmembers, 1);
    s->open.assign((size_t)nmembers, 0);
    s->ctx = c; s->model = m;
    {
        std::lock_guard<std::mutex> lk2(g_reg_mu);
        if (!live_set().count(c)) { (void)hipFree(s->slots); delete s; return ZPQ_E_CLOSED; }
        c->sets.push_back(s);
        c->set_bytes += s->bytes;
    }
    zpq_model_retain(m);
    *out = s;
    return ZPQ_OK;
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

extern "C" int zpq_blockset_create(zpq_ctx *c, const zpq_model *m, int nmembers, uint64_t max_member_bytes, zpq_blockset **out) try
{
    return zpq_blockset_create_ex(c, m, nmembers, max_member_bytes, 0, out);
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

extern "C" unsigned zpq_blockset_flags(const zpq_blockset *s) try
{
    return s ? s->flags : 0u;
} ZPQ_CATCH(return 0u)

extern "C" void zpq_blockset_destroy(zpq_blockset *s) try
{
    if (!s) return;
    zpq_ctx *c = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        c = s->ctx;                                         // nullptr: the ctx went first and took the slots with it
        if (c) {
            c->sets.erase(std::remove(c->sets.begin(), c->sets.end(), s), c->sets.end());
            c->set_bytes -= s->bytes;
        }
        s->ctx = nullptr;
    }
    if (c) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        if (s->slots) (void)hipFree(s->slots);
    }
    zpq_model_release(s->model);
    delete s;
} ZPQ_CATCH(return)

// chunk = a zpq_blockset_*_chunks call: members may stop in the middle of their segment (encode: more[i] != 0, NULL = none;
// decode: the slab is full) and are then OPEN, which the set remembers and reports in open_out[]; an open member goes on
// from there in the next chunk call.  Without chunk an open member is refused.
static int set_segments(zpq_blockset *s, int decode, const int32_t *member, const BlockArrays &h, bool chunk = false,
                        const uint8_t *more = nullptr, uint8_t *open_out = nullptr)
{
    const int n = h.n;
    if (!s) return ZPQ_E_ARG;
    zpq_ctx *c = s->ctx;
    if (!c) return ZPQ_E_CLOSED;
    if (!ctx_live(c)) return ZPQ_E_CLOSED;
    if (n < 0 || n > s->nmembers || (h.flags & ZPQ_FLAG_NOEOF)) return ZPQ_E_ARG;
    if (n == 0) return ZPQ_OK;
    if (!h.in_off || !h.out_off || !h.out_len || !h.status) return ZPQ_E_ARG;
    if (!slabs_valid(h)) return ZPQ_E_ARG;
    std::vector<int32_t> mem((size_t)n);
    {
        std::vector<uint8_t> seen((size_t)s->nmembers, 0);
        for (int i = 0; i < n; i++) {
            const int32_t k = member ? member[i] : i;
            if (k < 0 || k >= s->nmembers || seen[(size_t)k]) return ZPQ_E_ARG;
            seen[(size_t)k] = 1;
            mem[(size_t)i] = k;
        }
    }
    // (a ZPQ_SET_LANES set takes chunk calls only where ZPQ_SET_CHUNKS was asked for at its creation)
    const bool lane_chunks = chunk && (s->flags & ZPQ_SET_CHUNKS) != 0;
    if (chunk && (((s->flags & ZPQ_SET_LANES) && !lane_chunks) || s->layout.n < 1 || (decode && !open_out))) return ZPQ_E_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    // an open segment belongs to the chunk calls of the direction that opened it
    for (int i = 0; i < n; i++) {
        const uint8_t o = s->open[(size_t)mem[(size_t)i]];
        if (o && (!chunk || o != (decode ? 2 : 1))) return ZPQ_E_ARG;
    }
    HIPCK(hipSetDevice(c->device));
    // failed members report their status and take no part; the rest are packed into one batch
    std::vector<int> live;
    uint64_t in_bytes = 0, out_bytes = 0;
    for (int i = 0; i < n; i++) {
        const int32_t f = s->failed[(size_t)mem[(size_t)i]];
        if (f != ZPQ_OK) {
            h.status[i] = f; h.out_len[i] = 0;
            if (h.consumed) h.consumed[i] = 0;
            if (h.final_code) h.final_code[i] = 0;
            if (h.first_byte) h.first_byte[i] = 0xFFFFFFFFu;
            if (open_out) open_out[i] = 0;
        } else {
            live.push_back(i);
            in_bytes += h.in_off[i + 1] - h.in_off[i];
            out_bytes += h.out_off[i + 1] - h.out_off[i];
        }
    }
    const int k = (int)live.size();
    if (k == 0) return ZPQ_OK;
    const bool all = k == n;
    StageSet &S = c->one;
    hipStream_t st = c->stream;
    const size_t u32b = (size_t)k * 4;
    int rc = stage_room(S, k, (size_t)in_bytes, (size_t)out_bytes, u32b + 16);
    if (rc != ZPQ_OK) return rc;
    // the live members' slabs one behind the other (with all of them live that is the caller's window as it stands)
    uint64_t *const h_in = S.h_in(), *const h_out = S.h_out(k);
    std::vector<int32_t> h_map((size_t)k);
    h_in[0] = 0; h_out[0] = 0;
    for (int j = 0; j < k; j++) {
        const int i = live[(size_t)j];
        // (16-byte aligned slabs: the kernels read and write them by dwords)
        h_in[j + 1] = h_in[j] + (h.in_off[i + 1] - h.in_off[i]);
        h_out[j + 1] = h_out[j] + (h.out_off[i + 1] - h.out_off[i]);
        h_map[(size_t)j] = mem[(size_t)i];
        if (chunk && (s->chain || lane_chunks))   // (k_chain / k_rows / k_lanes<..., KEEP> alone read these marks: chunk calls never run on k_pipe, k_wset, k_vset)
            h_map[(size_t)j] |= (s->open[(size_t)mem[(size_t)i]] ? ZB_MAP_CONT : 0) | (!decode && more && more[i] ? ZB_MAP_MORE : 0);
    }
    if (all) { if (in_bytes) HIPCK(hipMemcpyAsync(S.in.p, h.in + h.in_off[0], (size_t)in_bytes, hipMemcpyHostToDevice, st)); }
    else for (int j = 0; j < k; j++) {
        const int i = live[(size_t)j];
        const size_t len = (size_t)(h.in_off[i + 1] - h.in_off[i]);
        if (len) HIPCK(hipMemcpyAsync((uint8_t *)S.in.p + h_in[j], h.in + h.in_off[i], len, hipMemcpyHostToDevice, st));
    }
    HIPCK(hipMemcpyAsync(S.misc.p, h_map.data(), u32b, hipMemcpyHostToDevice, st));
    if ((rc = stage_upload(S, k, st, false)) != ZPQ_OK) return rc;
    BlockArrays dv = S.device_view(k, h.flags & 0xffu & ~ZPQ_FLAG_LINESTORE, decode);   // (a set's layout is its own: no request here)
    if (s->chain || (s->flags & ZPQ_SET_LANES)) {
        DevModel dm;
        if ((rc = get_dev_model(c, s->model, s->layout, s->sp, &dm)) != ZPQ_OK) return rc;
        dv.flags = (dv.flags & ~(uint32_t)(ZPQ_FLAG_GENERIC | ZPQ_FLAG_LANES)) | ZB_KEEP_STATE;
        if (chunk) dv.flags |= ZB_CHUNK;   // (always k_chain<..., KEEP>, ZPQ_SET_PIPE or not; always k_rows / k_lanes<..., KEEP>, ZPQ_SET_WAVES / _VMWAVES or not)
        else if (!decode && (s->flags & ZPQ_SET_PIPE)) dv.flags |= ZB_SET_PIPE;   // this call may run on k_pipe<..., KEEP> (zpq_launch_chain)
        DBatch B = batch_base(c, dm, dv);
        B.slots = s->slots; B.nslots = k;
        B.slot_map = (const int32_t *)S.misc.p;
        c->last_slots = k;
        c->last_sp = s->sp;
        if (s->chain) {
            Plan P;
            P.fam = F_CHAIN; P.sp = s->sp; P.M = s->layout; P.nslots = k;
            if (!zpq_chain_plan(&s->layout, k, c->cus, &P.bpw)) return ZPQ_E_INTERNAL;
            P.grid = (k + P.bpw - 1) / P.bpw;
            if (P.grid > zpq_chain_max_wgs(&s->layout, c->cus)) return ZPQ_E_INTERNAL;   // (nmembers <= capacity rules this out)
            if ((rc = launch_family(c, B, P, decode, st)) != ZPQ_OK) return rc;
        } else {
            // the round in one launch of k_rows / k_lanes<..., KEEP>: any number of members, no workgroup waits for another
            // ZPQ_SET_WAVES: this call runs on k_wset / k_wsetd unless ZPQ_ENC_GPIPE=0 / ZPQ_DEC_GPIPE=0 says otherwise right now;
            // the slot format is one, so calls on a set may alternate.  No floor on k.  ZPQ_SET_VMWAVES: the same with k_vset / k_vsetd.
            // (the KEEP launchers are not a batch call's families: they have no row in FAMILY)
            const char *ev = getenv(decode ? "ZPQ_DEC_GPIPE" : "ZPQ_ENC_GPIPE");
            const bool on = !(ev && atoi(ev) == 0);
            // A chunk call (ZPQ_SET_CHUNKS) always runs on k_rows / k_lanes: the pause is theirs alone.
            const bool waves = (s->flags & ZPQ_SET_WAVES) != 0 && on && !chunk, vmwaves = (s->flags & ZPQ_SET_VMWAVES) != 0 && on && !chunk;
            rc = timed_launch(c, st, [&](const char **name) {
                if (waves || vmwaves) return (waves ? zpq_launch_wset : zpq_launch_vset)(&B, &s->layout, decode, st, name);
                *name = zpq_lanes_kernel_name(&s->layout, decode);
                return zpq_launch_lanes_keep(&B, &s->layout, decode, st);
            });
            if (rc != ZPQ_OK) return rc;
        }
    } else {
        // other models: the lane-0 kernel on the member's slot, one launch each (ZB_KEEP_STATE from the second segment on)
        for (int j = 0; j < k; j++) {
            const int32_t mb = h_map[(size_t)j];
            BatchArgs a;
            a.io = dv.window(j, j + 1);
            a.io.flags = dv.flags | ZPQ_FLAG_GENERIC | (s->fresh[(size_t)mb] ? 0u : ZB_KEEP_STATE);
            if (chunk) {
                const int i = live[(size_t)j];
                a.io.flags |= ZB_CHUNK | (s->open[(size_t)mb] ? ZB_CHUNK_CONT : 0u) | (!decode && more && more[i] ? ZB_CHUNK_MORE : 0u);
            }
            a.x.own_slot = s->slots + (uint64_t)mb * s->layout.slot_bytes;
            if ((rc = run_batch(c, s->model, decode, a)) != ZPQ_OK) { (void)hipStreamSynchronize(st); return rc; }
        }
    }
    if ((rc = fetch_results(S, 0, k, st)) != ZPQ_OK) return rc;
    if (all && out_bytes) HIPCK(hipMemcpyAsync(h.out + h.out_off[0], S.out.p, (size_t)out_bytes, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    deliver(S, h, decode, live.data());
    for (int j = 0; j < k; j++) {
        const int i = live[(size_t)j];
        const int32_t mb = h_map[(size_t)j] & ZB_MAP_SLOT;              // (a chunk call on a chain or ZPQ_SET_CHUNKS set: the entry carries ZB_MAP_* as well)
        s->fresh[(size_t)mb] = 0;
        // still open: an encoder that was told so; a decoder that says it paused, its slab full, in front of the next EOF flag
        // (ZB_ST_PAUSED, which stays in here).  A failed member is never open.
        const bool paused = chunk && decode && h.status[i] == ZB_ST_PAUSED;
        if (paused) h.status[i] = ZPQ_OK;
        if (h.status[i] != ZPQ_OK) s->failed[(size_t)mb] = h.status[i];
        const bool op = chunk && h.status[i] == ZPQ_OK && (decode ? paused : (more && more[i]));
        s->open[(size_t)mb] = op ? (decode ? 2 : 1) : 0;
        if (open_out) open_out[i] = op ? 1 : 0;
        if (!all) {
            // a set with failed members: each live member's slab on its own, only what was produced
            const uint64_t cap = h.out_off[i + 1] - h.out_off[i];
            const size_t got = (size_t)(h.out_len[i] < cap ? h.out_len[i] : cap);
            if (got) HIPCK(hipMemcpyAsync(h.out + h.out_off[i], (uint8_t *)S.out.p + h_out[j], got, hipMemcpyDeviceToHost, st));
        }
    }
    if (!all) HIPCK(hipStreamSynchronize(st));
    return ZPQ_OK;
}

extern "C" int zpq_blockset_encode_segments(zpq_blockset *s, int n, const int32_t *member, const uint8_t *in, const uint64_t *in_off,
                                            uint32_t flags, uint8_t *out, const uint64_t *out_off, uint32_t *out_len, int32_t *status) try
{
    return set_segments(s, 0, member, block_arrays(n, in, in_off, flags, out, out_off, out_len, status));
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

extern "C" int zpq_blockset_decode_segments(zpq_blockset *s, int n, const int32_t *member, const uint8_t *in, const uint64_t *in_off,
                                            uint32_t flags, uint8_t *out, const uint64_t *out_off, uint32_t *out_len, uint32_t *consumed,
                                            uint32_t *final_code, uint32_t *first_byte, int32_t *status) try
{
    return set_segments(s, 1, member, block_arrays(n, in, in_off, flags, out, out_off, out_len, status, consumed, final_code, first_byte));
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

extern "C" int zpq_blockset_encode_chunks(zpq_blockset *s, int n, const int32_t *member, const uint8_t *in, const uint64_t *in_off,
                                          uint32_t flags, const uint8_t *more, uint8_t *out, const uint64_t *out_off,
                                          uint32_t *out_len, int32_t *status) try
{
    return set_segments(s, 0, member, block_arrays(n, in, in_off, flags, out, out_off, out_len, status), true, more);
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

extern "C" int zpq_blockset_decode_chunks(zpq_blockset *s, int n, const int32_t *member, const uint8_t *in, const uint64_t *in_off,
                                          uint32_t flags, uint8_t *out, const uint64_t *out_off, uint32_t *out_len, uint32_t *consumed,
                                          uint32_t *final_code, uint32_t *first_byte, uint8_t *open, int32_t *status) try
{
    return set_segments(s, 1, member, block_arrays(n, in, in_off, flags, out, out_off, out_len, status, consumed, final_code, first_byte),
                        true, nullptr, open);
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

extern "C" int zpq_blockset_member_open(const zpq_blockset *s, int member) try
{
    if (!s) return ZPQ_E_ARG;
    zpq_ctx *c = s->ctx;
    if (!c || !ctx_live(c)) return ZPQ_E_CLOSED;
    if (member < 0 || member >= s->nmembers) return ZPQ_E_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    return s->open[(size_t)member] ? 1 : 0;
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

// ------------------------------------------------------------------ test hooks
extern "C" int zpq_debug_contexts(zpq_ctx *c, const zpq_model *m, const uint8_t *in, size_t n, uint32_t *h_out) try
{
    if (!ctx_live(c) || !m || !h_out || (n && !in)) return ZPQ_E_ARG;
    if (m->d.n == 0 || n == 0) return ZPQ_OK;
    const uint64_t in_off[2] = {0, n}, out_off[2] = {0, 0};
    uint32_t olen = 0;
    int32_t st = 0;
    uint8_t dummy = 0;
    BatchExtras x;
    x.ctx_out = h_out; x.ctx_words = n * (size_t)m->d.n;
    int rc = host_batch(c, m, 0, block_arrays(1, in, in_off, ZPQ_FLAG_GENERIC | ZB_CTX_ONLY, &dummy, out_off, &olen, &st), x);
    return rc != ZPQ_OK ? rc : st;
} ZPQ_CATCH(return ZPQ_E_INTERNAL)

extern "C" int zpq_debug_encode_trace(zpq_ctx *c, const zpq_model *m, const uint8_t *in, size_t n,
                                      uint32_t flags, uint8_t *out, size_t cap, size_t *out_len,
                                      int32_t *p_trace, size_t ntrace) try
{
    if (!ctx_live(c) || !m || !out_len || !p_trace || (n && !in) || (cap && !out)) return ZPQ_E_ARG;
    const uint64_t in_off[2] = {0, n}, out_off[2] = {0, cap};
    uint32_t olen = 0;
    int32_t st = 0;
    BatchExtras x;
    x.trace = p_trace; x.ntrace = (uint32_t)ntrace;
    int rc = host_batch(c, m, 0, block_arrays(1, in, in_off, (flags & 0xffu) | ZPQ_FLAG_GENERIC, out, out_off, &olen, &st), x);
    if (rc != ZPQ_OK) return rc;
    *out_len = olen;
    return st;
} ZPQ_CATCH(return ZPQ_E_INTERNAL)
