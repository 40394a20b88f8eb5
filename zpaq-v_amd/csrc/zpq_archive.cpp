// zpq_archive.cpp -- batch form of the reference CLI's add / extract / list loops
// (cmd/main.v:239-470) on top of the C ABI.
//
// The reference CLI writes one block with one segment per file and runs a fresh Compressor
// state machine per block (cmd/main.v:283-311); extraction walks find_block / find_filename /
// decompress / read_segment_end block after block (cmd/main.v:342-380).  Blocks are independent
// coding problems, so here a set of files is ONE GPU batch:
//   add:     upload all files once -> zpq_encode_blocks_dev + zpq_sha1_blocks_dev on the same
//            device buffer -> download coded payloads + digests -> host writes the framing.
//            Byte-identical to the per-file Compressor loop.
//   extract: host finds every block by the reference's rolling-hash locator
//            (decompressor.v:227-241) and reads headers + first segment names; all modelled
//            blocks with the same header are decoded by one zpq_decode_blocks_dev call, digests
//            by one zpq_sha1_blocks_dev call; the host then walks each trailer the way
//            Decoder.skip / read_segment_end do.  A block that turns out to hold more than one
//            segment, a store-mode block, or anything unusual is replayed through the sequential
//            Decompresser (state must persist across its segments).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <thread>

#include "../../include/zpaq_frontend.hpp"
#include "zpq_host.h"

namespace zpaq {

namespace {

struct DevMem {
    void *p = nullptr;
    ~DevMem() { if (p) (void)hipFree(p); }
    int alloc(size_t n) { return hipMalloc(&p, n ? n : 16) == hipSuccess ? ZPQ_OK : ZPQ_E_NOMEM; }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

#define HK(x) do { if ((x) != hipSuccess) return ZPQ_E_NODEVICE; } while (0)

// One message per GPU lane hashes ~18 MB/s, a host core ~400 MB/s: the side kernel wins once
// the batch holds a few dozen messages' worth of its longest one.
bool gpu_sha1_pays(uint64_t total, uint64_t longest) { return longest > 0 && total >= 24 * longest; }

void host_sha1(const uint8_t *p, size_t n, uint8_t out[20])
{
    SHA1 s;
    s.write_bytes(p, n);
    const std::vector<uint8_t> h = s.result();
    memcpy(out, h.data(), 20);
}

// Page-locked staging buffers, kept for the life of the process (pinning hundreds of MiB costs more than the
// transfer it speeds up, so a buffer is pinned once and handed out again).
struct PinnedPool {
    struct Buf { void *p; size_t cap; bool busy; };
    std::mutex mu;
    std::vector<Buf> bufs;
    void *acquire(size_t n)
    {
        std::lock_guard<std::mutex> lk(mu);
        for (Buf &b : bufs) if (!b.busy && b.cap >= n) { b.busy = true; return b.p; }
        for (Buf &b : bufs) if (!b.busy) { (void)hipHostFree(b.p); b.p = nullptr; b.cap = 0; b.busy = true;      // regrow a free one
            const size_t want = n + n / 8 + 4096;
            if (hipHostMalloc(&b.p, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); b.p = nullptr; b.busy = false; return nullptr; }
            b.cap = want; return b.p; }
        Buf nb{nullptr, 0, true};
        const size_t want = n + n / 8 + 4096;
        if (hipHostMalloc(&nb.p, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        nb.cap = want;
        bufs.push_back(nb);
        return nb.p;
    }
    void release(void *p)
    {
        std::lock_guard<std::mutex> lk(mu);
        for (Buf &b : bufs) if (b.p == p) b.busy = false;
    }
};
PinnedPool &pinned_pool() { static PinnedPool *pool = new PinnedPool(); return *pool; }   // (never destroyed: HIP may be gone at exit)
struct PinnedLease {
    void *p = nullptr;
    ~PinnedLease() { if (p) pinned_pool().release(p); }
    bool get(size_t n) { p = pinned_pool().acquire(n ? n : 16); return p != nullptr; }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

// fn(i) for i in [0, n) on a few host threads (memcpy-bound work: 4 threads saturate a socket's copy bandwidth here)
template <class F> void parallel_for(int n, uint64_t bytes, F fn)
{
    int T = (int)std::min<uint64_t>(4, std::max<uint64_t>(1, bytes >> 23));
    if (T > n) T = n > 0 ? n : 1;
    if (T <= 1) { for (int i = 0; i < n; i++) fn(i); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++)
        th.emplace_back([=, &fn]() { for (int i = (int)((int64_t)n * t / T); i < (int)((int64_t)n * (t + 1) / T); i++) fn(i); });
    for (std::thread &x : th) x.join();
}

struct VecWriter : Writer {
    std::vector<uint8_t> *v;
    explicit VecWriter(std::vector<uint8_t> *vv) : v(vv) {}
    void put(int c) override { v->push_back((uint8_t)c); }
    void write(const uint8_t *buf, int n) override { v->insert(v->end(), buf, buf + n); }
};

}  // namespace

// ------------------------------------------------------------------ add
namespace {
// one ZPAQ block to write: a whole file, or one fragment of it (continuations carry no name: libzpaq's
// convention for "more of the previous file")
struct Piece {
    std::string name, comment;
    const uint8_t *p;
    size_t n;
};
}  // namespace

static int add_pieces(zpq_ctx *ctx, int level, const std::vector<Piece> &files, std::vector<uint8_t> *archive, std::vector<size_t> *ends);

int archive_add(zpq_ctx *ctx, int level, const std::vector<ArchiveFile> &files, std::vector<uint8_t> *archive, size_t fragment_bytes,
                int solid_files)
{
    return archive_add(std::vector<zpq_ctx *>{ctx}, level, files, archive, fragment_bytes, solid_files);
}

// Several GPUs: block b -> context b mod G, one host thread per context, no collective; the
// blocks are written out in their original order, so the archive does not depend on G.
static void cut_pieces(std::vector<Piece> &pieces, const std::string &name, const std::string &comment, const uint8_t *p, size_t n, size_t fragment_bytes)
{
    if (fragment_bytes == 0 || n <= fragment_bytes) { pieces.push_back(Piece{name, comment, p, n}); return; }
    for (size_t off = 0; off < n; off += fragment_bytes) {
        const size_t k = std::min(fragment_bytes, n - off);
        pieces.push_back(off == 0 ? Piece{name, comment, p, k} : Piece{"", "", p + off, k});
    }
}
static int add_all(const std::vector<zpq_ctx *> &ctxs, int level, const std::vector<Piece> &pieces, std::vector<uint8_t> *archive);
static int add_solid(const std::vector<zpq_ctx *> &ctxs, int level, const std::vector<Piece> &pieces, int solid, std::vector<uint8_t> *archive);

int archive_add(const std::vector<zpq_ctx *> &ctxs, int level, const std::vector<ArchiveFile> &files, std::vector<uint8_t> *archive,
                size_t fragment_bytes, int solid_files)
{
    if (!archive || level < 0 || level > 5 || ctxs.empty() || solid_files < 0) return ZPQ_E_ARG;
    std::vector<Piece> pieces;
    for (const ArchiveFile &f : files) cut_pieces(pieces, f.name, f.comment, f.data.data(), f.data.size(), fragment_bytes);
    return solid_files > 1 ? add_solid(ctxs, level, pieces, solid_files, archive) : add_all(ctxs, level, pieces, archive);
}

// the same over caller-owned bytes (no copy of the file contents is made on the way to the GPU)
int archive_add_views(const std::vector<zpq_ctx *> &ctxs, int level, int nfiles, const char *const *names, const char *const *comments,
                      const uint8_t *const *data, const uint64_t *lens, std::vector<uint8_t> *archive, size_t fragment_bytes, int solid_files)
{
    if (!archive || level < 0 || level > 5 || ctxs.empty() || nfiles < 0 || solid_files < 0) return ZPQ_E_ARG;
    std::vector<Piece> pieces;
    for (int i = 0; i < nfiles; i++) cut_pieces(pieces, names[i], comments[i], data[i], (size_t)lens[i], fragment_bytes);
    return solid_files > 1 ? add_solid(ctxs, level, pieces, solid_files, archive) : add_all(ctxs, level, pieces, archive);
}

static int add_all(const std::vector<zpq_ctx *> &ctxs, int level, const std::vector<Piece> &pieces, std::vector<uint8_t> *archive)
{
    const size_t G = (level == 0 || pieces.size() < 2) ? 1 : std::min(ctxs.size(), pieces.size());
    if (G <= 1) return add_pieces(ctxs[0], level, pieces, archive, nullptr);
    std::vector<std::vector<Piece>> shard(G);
    for (size_t i = 0; i < pieces.size(); i++) shard[i % G].push_back(pieces[i]);
    std::vector<std::vector<uint8_t>> outs(G);
    std::vector<std::vector<size_t>> ends(G);
    std::vector<int> rcs(G, ZPQ_OK);
    std::vector<std::thread> th;
    for (size_t g = 0; g < G; g++)
        th.emplace_back([&, g]() { rcs[g] = add_pieces(ctxs[g], level, shard[g], &outs[g], &ends[g]); });
    for (std::thread &t : th) t.join();
    for (int r : rcs) if (r != ZPQ_OK) return r;
    for (size_t i = 0; i < pieces.size(); i++) {
        const size_t g = i % G, k = i / G;
        const size_t from = k ? ends[g][k - 1] : 0;
        archive->insert(archive->end(), outs[g].begin() + (ptrdiff_t)from, outs[g].begin() + (ptrdiff_t)ends[g][k]);
    }
    return ZPQ_OK;
}

static int add_pieces(zpq_ctx *ctx, int level, const std::vector<Piece> &files, std::vector<uint8_t> *archive, std::vector<size_t> *ends)
{
    VecWriter w(archive);
    const int n = (int)files.size();
    {
        size_t guess = archive->size();
        for (const Piece &f : files) guess += f.n / 2 + f.name.size() + f.comment.size() + 128;
        archive->reserve(guess);
    }
    if (n == 0) return ZPQ_OK;
    if (level == 0) {                                   // store mode has no coder: host only (compressor.v:297-354)
        for (const Piece &f : files) {
            Compressor c(nullptr);
            FileReader r(std::vector<uint8_t>(f.p, f.p + f.n));
            c.set_output(&w);
            c.start_block(0);
            c.start_segment(f.name, f.comment);
            c.set_input(&r);
            while (c.compress(65536)) {}
            c.end_segment();
            c.end_block();
            if (ends) ends->push_back(archive->size());
        }
        return ZPQ_OK;
    }
    if (!ctx) return ZPQ_E_NODEVICE;
    uint8_t hdr[256];
    int hlen = 0, cend = 0, hbegin = 0, hend = 0;
    int rc = zpq_level_header(level, hdr, (int)sizeof hdr, &hlen, &cend, &hbegin, &hend);
    if (rc != ZPQ_OK) return rc;
    zpq_model *model = nullptr;
    if ((rc = zpq_model_create(hdr, hlen, cend, hbegin, hend, &model)) != ZPQ_OK) return rc;
    struct ModelGuard { zpq_model *m; ~ModelGuard() { zpq_model_destroy(m); } } guard{model};

    std::vector<uint64_t> in_off((size_t)n + 1, 0), out_off((size_t)n + 1, 0);
    uint64_t longest = 0;
    for (int i = 0; i < n; i++) {
        const uint64_t len = files[i].n;
        if (len > 0xFFFFFF00ull) return ZPQ_E_TOOBIG;
        in_off[i + 1] = in_off[i] + len;
        out_off[i + 1] = out_off[i] + len + len / 4 + 1024;      // overflowing blocks are redone below
        longest = std::max(longest, len);
    }
    const uint64_t total = in_off[n], out_total = out_off[n];
    const bool gpu_sha = gpu_sha1_pays(total, longest);

    HK(hipSetDevice(zpq_ctx_device(ctx)));
    hipStream_t s = (hipStream_t)zpq_ctx_stream(ctx);
    DevMem d_in, d_inoff, d_out, d_outoff, d_len, d_st, d_sha;
    if ((rc = d_in.alloc(total + 64)) || (rc = d_inoff.alloc(((size_t)n + 1) * 8)) || (rc = d_out.alloc(out_total + 64)) ||
        (rc = d_outoff.alloc(((size_t)n + 1) * 8)) || (rc = d_len.alloc((size_t)n * 4)) || (rc = d_st.alloc((size_t)n * 4)) ||
        (rc = d_sha.alloc((size_t)n * 20)))
        return rc;
    {
        // the files lie scattered in pageable memory: gather them into one pinned buffer on a few host threads, then
        // one DMA (a hipMemcpyAsync per file is a staged, synchronous copy each: ~100 ms for 8192 files)
        PinnedLease stage;
        if (!stage.get(total)) return ZPQ_E_NOMEM;
        uint8_t *h = stage.as<uint8_t>();
        // in chunks of ~32 MiB: the DMA of one chunk runs while the next is being gathered
        for (int i0 = 0; i0 < n;) {
            int i1 = i0;
            while (i1 < n && in_off[i1] - in_off[i0] < (32ull << 20)) i1++;
            const uint64_t c0 = in_off[i0], cbytes = in_off[i1] - c0;
            parallel_for(i1 - i0, cbytes, [&](int k) { const int i = i0 + k; if (files[i].n) memcpy(h + in_off[i], files[i].p, files[i].n); });
            if (cbytes) HK(hipMemcpyAsync(d_in.as<uint8_t>() + c0, h + c0, cbytes, hipMemcpyHostToDevice, s));
            i0 = i1;
        }
        HK(hipStreamSynchronize(s));                       // (the lease goes back to the pool here)
    }
    HK(hipMemcpyAsync(d_inoff.p, in_off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
    HK(hipMemcpyAsync(d_outoff.p, out_off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
    HK(hipMemsetAsync(d_st.p, 0xff, (size_t)n * 4, s));
    // compress() is always entered by the CLI loop, so the PP byte is coded first (compressor.v:271-274)
    if ((rc = zpq_encode_blocks_dev(ctx, model, n, d_in.as<uint8_t>(), d_inoff.as<uint64_t>(), ZPQ_FLAG_PP, d_out.as<uint8_t>(),
                                    d_outoff.as<uint64_t>(), d_len.as<uint32_t>(), d_st.as<int32_t>())) != ZPQ_OK)
        return rc;
    if (gpu_sha && (rc = zpq_sha1_blocks_dev(ctx, n, d_in.as<uint8_t>(), d_inoff.as<uint64_t>(), d_sha.as<uint8_t>())) != ZPQ_OK)
        return rc;
    std::vector<uint32_t> lens((size_t)n);
    std::vector<int32_t> st((size_t)n);
    std::vector<uint8_t> sha((size_t)n * 20);
    HK(hipMemcpyAsync(lens.data(), d_len.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HK(hipMemcpyAsync(st.data(), d_st.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (gpu_sha) HK(hipMemcpyAsync(sha.data(), d_sha.p, (size_t)n * 20, hipMemcpyDeviceToHost, s));
    HK(hipStreamSynchronize(s));
    // the slabs are capacity-strided: pack the real payload bytes on the device, download only those
    std::vector<uint64_t> pk_off((size_t)n + 1, 0);
    for (int i = 0; i < n; i++) {
        if (st[i] != ZPQ_OK) { lens[i] = 0; }
        pk_off[i + 1] = pk_off[i] + lens[i];
    }
    PinnedLease coded_lease;
    if (!coded_lease.get((size_t)pk_off[n])) return ZPQ_E_NOMEM;
    const uint8_t *const coded = coded_lease.as<uint8_t>();
    {
        DevMem d_pk, d_pkoff, d_len2;
        if ((rc = d_pk.alloc(pk_off[n] + 64)) || (rc = d_pkoff.alloc(((size_t)n + 1) * 8)) || (rc = d_len2.alloc((size_t)n * 4))) return rc;
        HK(hipMemcpyAsync(d_pkoff.p, pk_off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
        HK(hipMemcpyAsync(d_len2.p, lens.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
        if ((rc = zpq_gather_dev(ctx, n, d_out.as<uint8_t>(), d_outoff.as<uint64_t>(), d_len2.as<uint32_t>(), d_pk.as<uint8_t>(),
                                 d_pkoff.as<uint64_t>())) != ZPQ_OK)
            return rc;
        if (pk_off[n]) HK(hipMemcpyAsync(coded_lease.p, d_pk.p, (size_t)pk_off[n], hipMemcpyDeviceToHost, s));
        HK(hipStreamSynchronize(s));
    }
    if (!gpu_sha) for (int i = 0; i < n; i++) host_sha1(files[i].p, files[i].n, &sha[(size_t)i * 20]);

    // a payload that outgrew its slab (possible: worst case ~16x) is coded again alone
    std::map<int, std::vector<uint8_t>> redo;
    for (int i = 0; i < n; i++) {
        if (st[i] == ZPQ_OK) continue;
        if (st[i] != ZPQ_E_OVERFLOW) return st[i];
        std::vector<uint8_t> big(files[i].n * 17 + 4096);
        const uint64_t io[2] = {0, files[i].n}, oo[2] = {0, big.size()};
        uint32_t bl = 0;
        int32_t bs = 0;
        if ((rc = zpq_encode_blocks(ctx, model, 1, files[i].p, io, ZPQ_FLAG_PP, big.data(), oo, &bl, &bs)) != ZPQ_OK) return rc;
        if (bs != ZPQ_OK) return bs;
        big.resize(bl);
        redo[i] = std::move(big);
    }
    // every block's bytes: [locator + header | segment header | payload | trailer | end of block].  All sizes are known
    // now, so the archive is sized once and the blocks are written into place on a few host threads.
    std::vector<uint8_t> head;                              // identical for every block of this level
    { VecWriter hw(&head); framing::block_header(hw, hdr, hlen, cend, hbegin, hend); }
    const size_t base = archive->size();
    std::vector<size_t> at((size_t)n + 1, base);
    for (int i = 0; i < n; i++) {
        auto it = redo.find(i);
        const size_t payload = it != redo.end() ? it->second.size() : lens[i];
        at[i + 1] = at[i] + head.size() + (1 + files[i].name.size() + 1 + files[i].comment.size() + 1 + 1) + payload + (4 + 1 + 20) + 1;
    }
    archive->resize(at[n]);
    uint8_t *const A = archive->data();
    parallel_for(n, at[n] - base, [&](int i) {
        uint8_t *q = A + at[i];
        memcpy(q, head.data(), head.size()); q += head.size();
        *q++ = 1;                                                           // framing::segment_header
        memcpy(q, files[i].name.data(), files[i].name.size()); q += files[i].name.size();
        *q++ = 0;
        memcpy(q, files[i].comment.data(), files[i].comment.size()); q += files[i].comment.size();
        *q++ = 0; *q++ = 0;
        auto it = redo.find(i);
        if (it != redo.end()) { memcpy(q, it->second.data(), it->second.size()); q += it->second.size(); }
        else { memcpy(q, coded + pk_off[i], lens[i]); q += lens[i]; }
        *q++ = 0; *q++ = 0; *q++ = 0; *q++ = 0; *q++ = 253;                  // framing::segment_trailer
        memcpy(q, &sha[(size_t)i * 20], 20); q += 20;
        *q++ = 0xFF;                                                        // framing::block_end
    });
    if (ends) for (int i = 0; i < n; i++) ends->push_back(at[i + 1]);
    (void)w;
    return ZPQ_OK;
}

// ------------------------------------------------------------------ add, several files per block (NOT reference behaviour)
// solid = N > 1: N consecutive pieces share one block, a segment each with its own name, comment and SHA-1 -- the
// layout the reference's extractor reads (it loops find_filename inside a block, cmd/main.v:349-380) and its writer
// never makes.  The model carries over from file to file (compressor.v:238-245), so small files stop paying for a fresh
// model, a block header and a slot clear each.  Blocks are independent: they go through block sets (zpq_blockset_*),
// round r of a set coding the r-th piece of every block of the set in one launch.
namespace {
typedef std::vector<Piece> SolidBlock;

// one block through the sequential front end (level 0: no coder; or a block whose set member failed)
int solid_block_sequential(zpq_ctx *ctx, int level, const SolidBlock &blk, std::vector<uint8_t> *out)
{
    VecWriter w(out);
    Compressor c(level == 0 ? nullptr : ctx);
    c.set_output(&w);
    c.start_block(level);
    for (const Piece &f : blk) {
        FileReader r(std::vector<uint8_t>(f.p, f.p + f.n));
        c.start_segment(f.name, f.comment);
        c.set_input(&r);
        while (c.compress(65536)) {}
        c.end_segment();
        if (c.last_error() != ZPQ_OK) return c.last_error();
    }
    c.end_block();
    return c.last_error();
}

// this context's blocks, appended to *out in their order; ends[k] = size of *out behind block k
int add_solid_blocks(zpq_ctx *ctx, int level, const std::vector<const SolidBlock *> &blocks, std::vector<uint8_t> *out, std::vector<size_t> *ends)
{
    const int nb = (int)blocks.size();
    if (level == 0) {
        for (const SolidBlock *b : blocks) {
            const int rc = solid_block_sequential(nullptr, 0, *b, out);
            if (rc != ZPQ_OK) return rc;
            ends->push_back(out->size());
        }
        return ZPQ_OK;
    }
    if (!ctx) return ZPQ_E_NODEVICE;
    uint8_t hdr[256];
    int hlen = 0, cend = 0, hbegin = 0, hend = 0;
    int rc = zpq_level_header(level, hdr, (int)sizeof hdr, &hlen, &cend, &hbegin, &hend);
    if (rc != ZPQ_OK) return rc;
    zpq_model *model = nullptr;
    if ((rc = zpq_model_create(hdr, hlen, cend, hbegin, hend, &model)) != ZPQ_OK) return rc;
    struct ModelGuard { zpq_model *m; ~ModelGuard() { zpq_model_destroy(m); } } guard{model};
    std::vector<uint8_t> head;
    { VecWriter hw(&head); framing::block_header(hw, hdr, hlen, cend, hbegin, hend); }

    std::vector<std::vector<std::vector<uint8_t>>> coded((size_t)nb);      // [block][piece] payload
    std::vector<uint8_t> failed((size_t)nb, 0);
    for (int b0 = 0; b0 < nb;) {
        // a set of as many blocks as one may hold, its line store sized for the largest member's real sum (every segment
        // codes a PP byte of its own)
        uint64_t maxsum = 0;
        int b1 = b0;
        int cap_members = 1;
        for (; b1 < nb; b1++) {
            uint64_t sum = blocks[(size_t)b1]->size();
            for (const Piece &f : *blocks[(size_t)b1]) { if (f.n > 0xFFFFFF00ull) return ZPQ_E_TOOBIG; sum += f.n; }
            const uint64_t m2 = std::max(maxsum, sum);
            int capn = cap_members;
            if (b1 == b0 || m2 != maxsum) capn = zpq_blockset_capacity(ctx, model, m2);   // (a larger store: fewer members fit)
            if (capn < 0) return capn;
            if (capn < 1) return ZPQ_E_NOMEM;
            if (b1 - b0 + 1 > capn) break;
            maxsum = m2; cap_members = capn;
        }
        if (b1 == b0) return ZPQ_E_NOMEM;
        const int nm = b1 - b0;
        zpq_blockset *set = nullptr;
        if ((rc = zpq_blockset_create(ctx, model, nm, maxsum, &set)) != ZPQ_OK) return rc;
        struct SetGuard { zpq_blockset *s; ~SetGuard() { zpq_blockset_destroy(s); } } sguard{set};
        size_t rounds = 0;
        for (int b = b0; b < b1; b++) { rounds = std::max(rounds, blocks[(size_t)b]->size()); coded[(size_t)b].resize(blocks[(size_t)b]->size()); }
        std::vector<uint8_t> in, outbuf;
        for (size_t r = 0; r < rounds; r++) {
            std::vector<int32_t> member;
            std::vector<uint64_t> in_off(1, 0), out_off(1, 0);
            for (int b = b0; b < b1; b++) {
                if (blocks[(size_t)b]->size() <= r || failed[(size_t)b]) continue;
                const Piece &f = (*blocks[(size_t)b])[r];
                member.push_back(b - b0);
                in_off.push_back(in_off.back() + f.n);
                out_off.push_back(out_off.back() + ((f.n + f.n / 4 + 1024 + 15) & ~(uint64_t)15));
            }
            const int k = (int)member.size();
            if (!k) continue;
            in.resize((size_t)in_off.back() + 16);
            outbuf.resize((size_t)out_off.back() + 16);
            parallel_for(k, in_off.back(), [&](int j) {
                const Piece &f = (*blocks[(size_t)(b0 + member[(size_t)j])])[r];
                if (f.n) memcpy(in.data() + in_off[(size_t)j], f.p, f.n);
            });
            std::vector<uint32_t> len((size_t)k);
            std::vector<int32_t> st((size_t)k);
            // compress() is always entered, so every segment codes its PP byte first (compressor.v:271-274)
            if ((rc = zpq_blockset_encode_segments(set, k, member.data(), in.data(), in_off.data(), ZPQ_FLAG_PP, outbuf.data(), out_off.data(),
                                                   len.data(), st.data())) != ZPQ_OK)
                return rc;
            for (int j = 0; j < k; j++) {
                const int b = b0 + member[(size_t)j];
                if (st[(size_t)j] != ZPQ_OK) { failed[(size_t)b] = 1; continue; }   // (a payload that outgrew its slab, ...): redone below
                coded[(size_t)b][r].assign(outbuf.data() + out_off[(size_t)j], outbuf.data() + out_off[(size_t)j] + len[(size_t)j]);
            }
        }
        b0 = b1;
    }
    // digests on a few host threads, then the framing: [locator + header | per file: segment header, payload, trailer | FF]
    std::vector<std::pair<int, int>> all;
    uint64_t total = 0;
    for (int b = 0; b < nb; b++) for (size_t r = 0; r < blocks[(size_t)b]->size(); r++) { all.emplace_back(b, (int)r); total += (*blocks[(size_t)b])[r].n; }
    std::vector<uint8_t> sha(all.size() * 20);
    parallel_for((int)all.size(), total, [&](int i) { const Piece &f = (*blocks[(size_t)all[(size_t)i].first])[(size_t)all[(size_t)i].second]; host_sha1(f.p, f.n, &sha[(size_t)i * 20]); });
    size_t si = 0;
    for (int b = 0; b < nb; b++) {
        const SolidBlock &blk = *blocks[(size_t)b];
        if (failed[(size_t)b]) {
            if ((rc = solid_block_sequential(ctx, level, blk, out)) != ZPQ_OK) return rc;
            si += blk.size();
        } else {
            out->insert(out->end(), head.begin(), head.end());
            for (size_t r = 0; r < blk.size(); r++, si++) {
                out->push_back(1);                                                  // framing::segment_header
                out->insert(out->end(), blk[r].name.begin(), blk[r].name.end());
                out->push_back(0);
                out->insert(out->end(), blk[r].comment.begin(), blk[r].comment.end());
                out->push_back(0); out->push_back(0);
                out->insert(out->end(), coded[(size_t)b][r].begin(), coded[(size_t)b][r].end());
                const uint8_t tr[5] = {0, 0, 0, 0, 253};                           // framing::segment_trailer
                out->insert(out->end(), tr, tr + 5);
                out->insert(out->end(), sha.begin() + (ptrdiff_t)(si * 20), sha.begin() + (ptrdiff_t)(si * 20 + 20));
            }
            out->push_back(0xFF);                                                   // framing::block_end
        }
        ends->push_back(out->size());
    }
    return ZPQ_OK;
}
}  // namespace

static int add_solid(const std::vector<zpq_ctx *> &ctxs, int level, const std::vector<Piece> &pieces, int solid, std::vector<uint8_t> *archive)
{
    std::vector<SolidBlock> blocks;
    for (size_t i = 0; i < pieces.size(); i += (size_t)solid)
        blocks.emplace_back(pieces.begin() + (ptrdiff_t)i, pieces.begin() + (ptrdiff_t)std::min(pieces.size(), i + (size_t)solid));
    if (blocks.empty()) return ZPQ_OK;
    // block g -> context g mod G, one host thread per context; written out in their original order
    const size_t G = level == 0 ? 1 : std::min(ctxs.size(), blocks.size());
    std::vector<std::vector<const SolidBlock *>> shard(G);
    for (size_t g = 0; g < blocks.size(); g++) shard[g % G].push_back(&blocks[g]);
    std::vector<std::vector<uint8_t>> outs(G);
    std::vector<std::vector<size_t>> ends(G);
    std::vector<int> rcs(G, ZPQ_OK);
    if (G == 1) rcs[0] = add_solid_blocks(ctxs[0], level, shard[0], &outs[0], &ends[0]);
    else {
        std::vector<std::thread> th;
        for (size_t g = 0; g < G; g++) th.emplace_back([&, g]() { rcs[g] = add_solid_blocks(ctxs[g], level, shard[g], &outs[g], &ends[g]); });
        for (std::thread &t : th) t.join();
    }
    for (int r : rcs) if (r != ZPQ_OK) return r;
    for (size_t i = 0; i < blocks.size(); i++) {
        const size_t g = i % G, k = i / G;
        const size_t from = k ? ends[g][k - 1] : 0;
        archive->insert(archive->end(), outs[g].begin() + (ptrdiff_t)from, outs[g].begin() + (ptrdiff_t)ends[g][k]);
    }
    return ZPQ_OK;
}

// ------------------------------------------------------------------ extract / list
namespace {

const int kCompSize[10] = {0, 2, 3, 2, 3, 4, 6, 6, 3, 5};

struct BlockRec {
    size_t tag_pos = 0;          // where a Decompresser must start reading to find this block again
    std::vector<uint8_t> hdr;
    int cend = 0, hbegin = 0, hend = 0, ncomp = 0;
    bool has_segment = false;
    std::string name, comment;
    size_t payload = 0;          // first byte of the coded data of the first segment
    size_t next_tag = 0;         // start of the next block's locator window (or archive end)
    size_t end = 0;              // store-mode blocks: where the sequential reader stands after the block (0 = not known yet)
};

// Walks a store-mode block (no components) from its first segment marker to the byte after its end-of-block
// marker, exactly as the sequential loop consumes it: per segment `01 name 00 comment 00 00`, length-prefixed
// chunks up to a zero length (decompressor.v:518-587), the trailer byte (+ 20 digest bytes behind 253, :590-635),
// then the next marker; 0xFF ends the block (:350-368).  A stream that ends inside the block leaves the reader at n.
size_t walk_store_block(const uint8_t *a, size_t n, size_t q)
{
    auto get = [&]() -> int { return q < n ? a[q++] : -1; };
    for (;;) {
        const int marker = get();                          // find_filename
        if (marker < 0) return n;
        if (marker == 0xFF) return q;
        for (;;) { const int c = get(); if (c < 0) return n; if (c == 0) break; if (c == 0xFF) return q; }
        for (;;) { const int c = get(); if (c < 0) return n; if (c == 0) break; }
        if (get() < 0) return n;
        for (;;) {                                         // decompress_store
            if (n - q < 4) return n;
            const uint32_t len = ((uint32_t)a[q] << 24) | ((uint32_t)a[q + 1] << 16) | ((uint32_t)a[q + 2] << 8) | (uint32_t)a[q + 3];
            q += 4;
            if (len == 0) break;
            if (n - q < len) return n;
            q += len;
        }
        const int trailer = get();                         // read_segment_end
        if (trailer < 0) return n;
        if (trailer == 253) { if (n - q < 20) return n; q += 20; }
    }
}

// find_block (decompressor.v:219-346) on a flat buffer: false = the reference's loop would stop here.
// `at_reader` says that `pos` is a position the sequential reader really stands at (stream start, or right
// behind a block whose end is known): only there may a bare "zPQ" start a block.
bool next_block(const uint8_t *a, size_t n, size_t &pos, BlockRec &b, bool at_reader)
{
    // The reference rolls four 32-bit hashes h = h*{12,20,28,44} + c over the stream and stops when all
    // four hit their targets (decompressor.v:227-241).  12^16 = 20^16 = 28^16 = 44^16 = 0 (mod 2^32), so the
    // hashes are a function of the last 16 bytes only, and the targets are the hashes of the 13-byte
    // locator + "zPQ"; the initial constants are the state after the 13 locator bytes, so a stream that
    // starts with "zPQ" WHERE find_block BEGINS READING matches too.  Searching for those bytes is the same
    // test (up to a 128-bit hash collision) at memmem speed instead of 16 multiplies per archive byte.
    static const uint8_t tag16[16] = {0x37, 0x6b, 0x53, 0x74, 0xa0, 0x31, 0x83, 0xd3, 0x8c, 0xb2, 0x28, 0xb0, 0xd3, 0x7a, 0x50, 0x51};
    if (pos >= n) return false;
    if (at_reader && pos + 3 <= n && memcmp(a + pos, tag16 + 13, 3) == 0) { b.tag_pos = pos; pos += 3; }
    else {
        const void *m = memmem(a + pos, n - pos, tag16, sizeof tag16);
        if (!m) { pos = n; return false; }
        b.tag_pos = (size_t)(static_cast<const uint8_t *>(m) - a);
        pos = b.tag_pos + 16;
    }
    b.end = 0;
    auto get = [&]() -> int { return pos < n ? a[pos++] : -1; };
    const int level = get();
    if (level != 1 && level != 2) return false;
    if (get() != 1) return false;
    const int lo = get(), hi = get();
    if (lo < 0 || hi < 0) return false;
    const int hsize = lo + hi * 256;
    b.hdr.clear();
    for (int i = 0; i < 5; i++) { const int v = get(); if (v < 0) return false; b.hdr.push_back((uint8_t)v); }
    b.ncomp = b.hdr[4];
    for (int i = 0; i < b.ncomp; i++) {
        const int t = get();
        if (t < 0 || t >= 10) return false;
        b.hdr.push_back((uint8_t)t);
        for (int j = 1; j < kCompSize[t]; j++) { const int v = get(); if (v < 0) return false; b.hdr.push_back((uint8_t)v); }
    }
    if (get() != 0) return false;
    b.hdr.push_back(0);
    b.cend = (int)b.hdr.size() - 1;
    b.hbegin = (int)b.hdr.size();
    const int hcomp_len = hsize - (int)b.hdr.size();
    for (int i = 0; i < hcomp_len; i++) { const int v = get(); if (v < 0) return false; b.hdr.push_back((uint8_t)v); }
    b.hend = (int)b.hdr.size() - 1;
    const size_t body = pos;
    // find_filename (decompressor.v:350-429) for the first segment
    b.has_segment = false;
    b.name.clear(); b.comment.clear();
    size_t q = pos;
    auto get2 = [&]() -> int { return q < n ? a[q++] : -1; };
    auto parse_first = [&]() {
        const int marker = get2();
        if (marker < 0 || marker == 0xFF) { pos = q; return; }
        for (;;) { const int c = get2(); if (c < 0) return; if (c == 0) break; if (c == 0xFF) { pos = q; return; } b.name.push_back((char)c); }
        for (;;) { const int c = get2(); if (c < 0) return; if (c == 0) break; b.comment.push_back((char)c); }
        if (get2() < 0) return;
        b.has_segment = true;
        b.payload = q;
        pos = q;
    };
    parse_first();
    if (b.ncomp == 0) {
        // Store mode: the payload is raw bytes and may itself hold locators (an archive stored inside an
        // archive).  The sequential reader consumes the block before it looks for the next one
        // (cmd/main.v:342-380), so the search resumes behind it, never inside it.
        b.end = walk_store_block(a, n, body);
        pos = b.end;
    }
    return true;
}

// every segment of one block through the sequential front end; returns how far into [from, to) the reader got.
// *clean = the block decoded without a complaint and ended in its end-of-block marker, i.e. the returned position
// is where an undamaged stream continues (a damaged block's reader position means nothing).
size_t replay_block(zpq_ctx *ctx, const uint8_t *a, size_t from, size_t to, bool want_data, std::vector<ArchiveFile> *out, bool *clean)
{
    *clean = false;
    FileReader r(std::vector<uint8_t>(a + from, a + to));
    Decompresser d(ctx);
    d.set_input(&r);
    if (!d.find_block()) {
        if (d.last_error() != ZPQ_OK) { ArchiveFile f; f.status = d.last_error(); out->push_back(std::move(f)); }
        return from + d.position();
    }
    bool ok = true;
    while (d.find_filename()) {
        ArchiveFile f;
        f.name = d.get_filename();
        f.comment = d.get_comment();
        FileWriter fw;
        d.set_output(&fw);
        while (d.decompress(65536)) {}
        const std::vector<uint8_t> digest = d.get_sha1();
        d.read_segment_end();
        f.status = d.last_error();
        uint8_t stored[20];
        if (d.stored_sha1(stored)) f.sha1_ok = memcmp(stored, digest.data(), 20) == 0;
        f.size = fw.bytes().size();
        if (want_data) f.data = fw.bytes();
        const int fst = f.status;
        ok = ok && fst == ZPQ_OK && f.sha1_ok;
        out->push_back(std::move(f));
        if (fst != ZPQ_OK) break;
    }
    *clean = ok && d.block_ended();
    return from + d.position();
}

uint64_t size_hint(const std::string &comment)            // the CLI's "<n> bytes" comment (cmd/main.v:300-302); only a capacity hint
{
    uint64_t v = 0;
    size_t i = 0;
    while (i < comment.size() && comment[i] >= '0' && comment[i] <= '9' && v < (1ull << 40)) v = v * 10 + (uint64_t)(comment[i++] - '0');
    return (i > 0 && comment.compare(i, std::string::npos, " bytes") == 0) ? v : ~0ull;
}

}  // namespace

static int extract_segments(const std::vector<zpq_ctx *> &ctxs, const uint8_t *arc, size_t n, bool want_data, std::vector<ArchiveFile> *files);

int archive_extract(zpq_ctx *ctx, const uint8_t *arc, size_t n, bool want_data, std::vector<ArchiveFile> *files, bool join_unnamed)
{
    return archive_extract(std::vector<zpq_ctx *>{ctx}, arc, n, want_data, files, join_unnamed);
}

int archive_extract(const std::vector<zpq_ctx *> &ctxs, const uint8_t *arc, size_t n, bool want_data, std::vector<ArchiveFile> *files,
                    bool join_unnamed)
{
    if (!files || (n && !arc) || ctxs.empty()) return ZPQ_E_ARG;
    if (!join_unnamed) return extract_segments(ctxs, arc, n, want_data, files);
    std::vector<ArchiveFile> segs;
    const int rc = extract_segments(ctxs, arc, n, want_data, &segs);
    for (ArchiveFile &sg : segs) {
        if (sg.name.empty() && !files->empty()) {              // a fragment: more of the previous file
            ArchiveFile &f = files->back();
            f.size += sg.size;
            f.sha1_ok = f.sha1_ok && sg.sha1_ok;
            if (f.status == ZPQ_OK) f.status = sg.status;
            f.data.insert(f.data.end(), sg.data.begin(), sg.data.end());
        } else files->push_back(std::move(sg));
    }
    return rc;
}

namespace {
struct Decoded {
    bool done = false; size_t end = 0; ArchiveFile f;
    bool multi = false;                  // the first segment decoded cleanly and another segment follows it: a candidate for the sets
    std::vector<ArchiveFile> more;       // segments 2.. of a block that went through a set
};
typedef std::map<std::vector<uint8_t>, std::vector<int>> Groups;
}  // namespace
static int decode_groups(zpq_ctx *ctx, const uint8_t *arc, size_t n, bool want_data, const std::vector<BlockRec> &blocks,
                         const Groups &groups, std::vector<Decoded> &dec);
static int decode_multi(zpq_ctx *ctx, const uint8_t *arc, size_t n, bool want_data, const std::vector<BlockRec> &blocks,
                        const Groups &groups, std::vector<Decoded> &dec);

static int extract_segments(const std::vector<zpq_ctx *> &ctxs, const uint8_t *arc, size_t n, bool want_data, std::vector<ArchiveFile> *files)
{
    zpq_ctx *ctx = ctxs[0];
    // ---- pass 1: every block the sequential loop could visit.  Store-mode blocks are walked to their end, so
    //      nothing inside their raw payload is mistaken for a block; modelled blocks end where their decoder
    //      stops, which only pass 3 knows: records that turn out to lie inside one are dropped there.
    std::vector<BlockRec> blocks;
    {
        size_t pos = 0;
        bool at_reader = true;
        for (;;) {
            BlockRec b;
            if (!next_block(arc, n, pos, b, at_reader)) break;
            at_reader = b.end != 0;
            blocks.push_back(std::move(b));
        }
        for (size_t i = 0; i < blocks.size(); i++) {
            blocks[i].next_tag = i + 1 < blocks.size() ? blocks[i + 1].tag_pos : n;
            if (blocks[i].end && blocks[i].end < blocks[i].next_tag) blocks[i].next_tag = blocks[i].end;   // replay exactly the block
        }
    }
    // ---- pass 2: one batch per distinct header over the single-segment candidates
    std::vector<Decoded> dec(blocks.size());
    // candidates dealt round-robin over the contexts (block b -> context b mod G), one host thread each
    size_t G = 0;
    for (zpq_ctx *c : ctxs) if (c) G++; else break;
    std::vector<Groups> groups(G ? G : 1);
    size_t ncand = 0;
    for (size_t i = 0; i < blocks.size(); i++)
        if (blocks[i].ncomp > 0 && blocks[i].has_segment && G && n < 0xFFFFFF00ull) groups[ncand++ % G][blocks[i].hdr].push_back((int)i);
    if (ncand) {
        std::vector<int> rcs(G, ZPQ_OK);
        if (G == 1 || ncand < 2) rcs[0] = decode_groups(ctxs[0], arc, n, want_data, blocks, groups[0], dec);
        else {
            std::vector<std::thread> th;
            for (size_t g = 0; g < G; g++)
                th.emplace_back([&, g]() { rcs[g] = decode_groups(ctxs[g], arc, n, want_data, blocks, groups[g], dec); });
            for (std::thread &t : th) t.join();
        }
        for (int r : rcs) if (r != ZPQ_OK) return r;
        // ---- pass 2b: blocks that hold several segments, all blocks of one header through block sets, round r decoding the
        //      r-th segment of every block in one launch (the first segment again: the set's state must see it).  A block
        //      that is unusual in any way is left to the sequential replay below, with the result it always had.
        std::vector<Groups> multi(G);
        size_t nmulti = 0;
        for (size_t i = 0; i < blocks.size(); i++) if (dec[i].multi && !dec[i].done) multi[nmulti++ % G][blocks[i].hdr].push_back((int)i);
        if (nmulti) {
            std::fill(rcs.begin(), rcs.end(), ZPQ_OK);
            if (G == 1 || nmulti < 2) rcs[0] = decode_multi(ctxs[0], arc, n, want_data, blocks, multi[0], dec);
            else {
                std::vector<std::thread> th;
                for (size_t g = 0; g < G; g++)
                    th.emplace_back([&, g]() { rcs[g] = decode_multi(ctxs[g], arc, n, want_data, blocks, multi[g], dec); });
                for (std::thread &t : th) t.join();
            }
            for (int r : rcs) if (r != ZPQ_OK) return r;
        }
    }
    // ---- everything else, in archive order, following the sequential reader: `seq` is where it stands.
    //      A record that begins before `seq` lies inside the block just consumed (the reference never sees it);
    //      a bare "zPQ" exactly at `seq` starts a block the locator search could not see.  Behind a DAMAGED block
    //      the reader's position means nothing: the walk then resumes at the next locator (more forgiving than
    //      the reference, whose reader would plough on through whatever follows).
    static const uint8_t zpq3[3] = {0x7a, 0x50, 0x51};
    size_t seq = 0;
    for (size_t i = 0; i <= blocks.size(); i++) {
        const size_t tag = i < blocks.size() ? blocks[i].tag_pos : n;
        if (tag < seq) continue;
        while (seq + 3 <= tag && memcmp(arc + seq, zpq3, 3) == 0 && !(i < blocks.size() && tag == seq)) {
            bool clean = false;
            const size_t stop = replay_block(ctx, arc, seq, tag, want_data, files, &clean);
            if (!clean || stop <= seq) { seq = tag; break; }
            seq = stop;
        }
        if (i == blocks.size()) break;
        if (tag < seq) continue;                               // swallowed by a bare block just replayed
        if (dec[i].done) {
            const bool clean = dec[i].f.sha1_ok && dec[i].f.status == ZPQ_OK;
            files->push_back(std::move(dec[i].f));
            for (ArchiveFile &f : dec[i].more) files->push_back(std::move(f));     // (a block from a set: every segment was clean)
            seq = clean ? dec[i].end : tag + 1;
            continue;
        }
        bool clean = false;
        const size_t stop = replay_block(ctx, arc, blocks[i].tag_pos, blocks[i].next_tag, want_data, files, &clean);
        seq = clean ? stop : tag + 1;
    }
    return ZPQ_OK;
}

// one context's share: a batch per distinct header (writes only the dec[] entries of its own blocks)
static int decode_groups(zpq_ctx *ctx, const uint8_t *arc, size_t n, bool want_data, const std::vector<BlockRec> &blocks,
                         const Groups &groups, std::vector<Decoded> &dec)
{
    if (groups.empty()) return ZPQ_OK;
    {
        HK(hipSetDevice(zpq_ctx_device(ctx)));
        hipStream_t s = (hipStream_t)zpq_ctx_stream(ctx);
        DevMem d_arc;
        int rc;
        if ((rc = d_arc.alloc(n + 64))) return rc;
        HK(hipMemcpyAsync(d_arc.p, arc, n, hipMemcpyHostToDevice, s));
        for (const auto &g : groups) {
            const BlockRec &b0 = blocks[(size_t)g.second[0]];
            zpq_model *model = nullptr;
            if (zpq_model_create(b0.hdr.data(), (int)b0.hdr.size(), b0.cend, b0.hbegin, b0.hend, &model) != ZPQ_OK) continue;   // replayed below
            struct ModelGuard { zpq_model *m; ~ModelGuard() { zpq_model_destroy(m); } } guard{model};
            std::vector<int> todo = g.second;
            std::vector<uint64_t> capmul(blocks.size(), 1);
            for (int attempt = 0; attempt < 4 && !todo.empty(); attempt++) {
                const int m = (int)todo.size();
                // input ranges: the decoder stops at the EOF symbol, so a range may run on to the next
                // candidate's payload (in_off must be contiguous); bytes after the payload are never coded
                std::vector<uint64_t> in_off((size_t)m + 1), out_off((size_t)m + 1, 0);
                for (int k = 0; k < m; k++) in_off[k] = blocks[(size_t)todo[k]].payload;
                in_off[m] = n;
                for (int k = 0; k < m; k++) {
                    const BlockRec &b = blocks[(size_t)todo[k]];
                    const uint64_t hint = size_hint(b.comment);
                    const uint64_t paylen = b.next_tag - b.payload;
                    // first try: the size the comment promises, but never absurdly more than the payload could
                    // plausibly expand to (the first fragment of a split file carries the WHOLE file's size)
                    uint64_t cap = paylen * 8 + 65536;
                    if (hint != ~0ull && attempt == 0) cap = std::min<uint64_t>(hint + 64, paylen * 4096 + 65536);
                    cap *= capmul[(size_t)todo[k]];
                    cap = std::min<uint64_t>(cap, 0xFFFFFF00ull);
                    out_off[k + 1] = out_off[k] + ((cap + 15) & ~15ull);
                }
                DevMem d_inoff, d_out, d_outoff, d_u32, d_st, d_sha;
                const size_t u = (size_t)m * 4;
                if ((rc = d_inoff.alloc(((size_t)m + 1) * 8)) || (rc = d_outoff.alloc(((size_t)m + 1) * 8)) || (rc = d_out.alloc(out_off[m] + 64)) ||
                    (rc = d_u32.alloc(u * 4)) || (rc = d_st.alloc(u)) || (rc = d_sha.alloc((size_t)m * 20)))
                    return rc;
                HK(hipMemcpyAsync(d_inoff.p, in_off.data(), ((size_t)m + 1) * 8, hipMemcpyHostToDevice, s));
                HK(hipMemcpyAsync(d_outoff.p, out_off.data(), ((size_t)m + 1) * 8, hipMemcpyHostToDevice, s));
                HK(hipMemsetAsync(d_st.p, 0xff, u, s));
                uint32_t *d_len = d_u32.as<uint32_t>(), *d_cons = d_len + m, *d_code = d_cons + m, *d_first = d_code + m;
                if ((rc = zpq_decode_blocks_dev(ctx, model, m, d_arc.as<uint8_t>(), d_inoff.as<uint64_t>(), ZPQ_FLAG_PP, d_out.as<uint8_t>(),
                                                d_outoff.as<uint64_t>(), d_len, d_cons, d_code, d_first, d_st.as<int32_t>())) != ZPQ_OK)
                    return rc;
                std::vector<uint32_t> meta((size_t)m * 4);
                std::vector<int32_t> st((size_t)m);
                HK(hipMemcpyAsync(meta.data(), d_u32.p, u * 4, hipMemcpyDeviceToHost, s));
                HK(hipMemcpyAsync(st.data(), d_st.p, u, hipMemcpyDeviceToHost, s));
                HK(hipStreamSynchronize(s));
                const uint32_t *len = meta.data(), *cons = len + m, *code = cons + m, *first = code + m;
                // digests of the decoded bytes (capacity-strided slabs: explicit ranges)
                uint64_t tot = 0, longest = 0;
                for (int k = 0; k < m; k++) if (st[k] == ZPQ_OK) { tot += len[k]; longest = std::max<uint64_t>(longest, len[k]); }
                const bool gpu_sha = gpu_sha1_pays(tot, longest);
                std::vector<uint8_t> sha((size_t)m * 20, 0);
                PinnedLease slab_lease;
                const uint8_t *slab = nullptr;
                if (gpu_sha) {
                    std::vector<uint64_t> rng((size_t)m * 2);      // begin[0..m) then end[0..m)
                    for (int k = 0; k < m; k++) { rng[(size_t)k] = out_off[k]; rng[(size_t)m + k] = out_off[k] + (st[k] == ZPQ_OK ? len[k] : 0); }
                    DevMem d_rng;
                    if ((rc = d_rng.alloc((size_t)m * 16))) return rc;
                    HK(hipMemcpyAsync(d_rng.p, rng.data(), (size_t)m * 16, hipMemcpyHostToDevice, s));
                    if ((rc = zpq_sha1_ranges_dev(ctx, m, d_out.as<uint8_t>(), d_rng.as<uint64_t>(), d_rng.as<uint64_t>() + m, d_sha.as<uint8_t>())) != ZPQ_OK)
                        return rc;
                    HK(hipMemcpyAsync(sha.data(), d_sha.p, (size_t)m * 20, hipMemcpyDeviceToHost, s));
                    HK(hipStreamSynchronize(s));
                }
                // decoded blocks sit in capacity-strided slabs: pack them on the device, download only real bytes
                std::vector<uint64_t> pk_off((size_t)m + 1, 0);
                for (int k = 0; k < m; k++) pk_off[k + 1] = pk_off[k] + (st[k] == ZPQ_OK ? len[k] : 0);
                if (want_data || !gpu_sha) {
                    std::vector<uint32_t> plen((size_t)m);
                    for (int k = 0; k < m; k++) plen[k] = st[k] == ZPQ_OK ? len[k] : 0;
                    DevMem d_pk, d_pkoff, d_plen;
                    if ((rc = d_pk.alloc(pk_off[m] + 64)) || (rc = d_pkoff.alloc(((size_t)m + 1) * 8)) || (rc = d_plen.alloc(u))) return rc;
                    HK(hipMemcpyAsync(d_pkoff.p, pk_off.data(), ((size_t)m + 1) * 8, hipMemcpyHostToDevice, s));
                    HK(hipMemcpyAsync(d_plen.p, plen.data(), u, hipMemcpyHostToDevice, s));
                    if ((rc = zpq_gather_dev(ctx, m, d_out.as<uint8_t>(), d_outoff.as<uint64_t>(), d_plen.as<uint32_t>(), d_pk.as<uint8_t>(),
                                             d_pkoff.as<uint64_t>())) != ZPQ_OK)
                        return rc;
                    if (!slab_lease.get((size_t)pk_off[m])) return ZPQ_E_NOMEM;
                    slab = slab_lease.as<uint8_t>();
                    if (pk_off[m]) HK(hipMemcpyAsync(slab_lease.p, d_pk.p, (size_t)pk_off[m], hipMemcpyDeviceToHost, s));
                    HK(hipStreamSynchronize(s));
                    if (!gpu_sha) for (int k = 0; k < m; k++) if (st[k] == ZPQ_OK) host_sha1(slab + pk_off[k], len[k], &sha[(size_t)k * 20]);
                }
                // ---- pass 3: trailer walk per block (Decoder.skip decoder.v:151-196, read_segment_end decompressor.v:590-635)
                std::vector<int> again, fill;
                for (int k = 0; k < m; k++) {
                    const size_t bi = (size_t)todo[k];
                    const BlockRec &b = blocks[bi];
                    if (st[k] == ZPQ_E_OVERFLOW) { capmul[bi] *= 8; again.push_back(todo[k]); continue; }
                    if (st[k] != ZPQ_OK || first[k] == 1u) continue;               // replayed (reports the error there)
                    size_t p = b.payload + cons[k];
                    auto get = [&]() -> int { return p < n ? arc[p++] : -1; };
                    uint32_t curr = code[k];
                    bool ok = true;
                    int marker = -1;
                    if (curr == 0) { const int c = get(); if (c < 0) ok = false; else curr = (uint32_t)c; }
                    while (ok && curr != 0) { const int c = get(); if (c < 0) { ok = false; break; } curr = (curr << 8) | (uint32_t)c; }
                    while (ok) { const int c = get(); if (c < 0) break; if (c != 0) { marker = c; break; } }
                    bool sha_ok = true;
                    if (marker == 253) {
                        if (p + 20 > n) continue;
                        sha_ok = memcmp(arc + p, &sha[(size_t)k * 20], 20) == 0;
                        p += 20;
                    }
                    const int after = get();
                    if (after != 0xFF) {
                        // more segments (or damage): through a block set if all is as a writer leaves it, else replayed sequentially
                        if (after == 1 && sha_ok && first[k] == 0u) dec[bi].multi = true;
                        continue;
                    }
                    Decoded &d = dec[bi];
                    d.done = true;
                    d.end = p;
                    d.f.name = b.name;
                    d.f.comment = b.comment;
                    d.f.sha1_ok = sha_ok;
                    d.f.size = first[k] == 0xFFFFFFFFu ? 0 : len[k];
                    if (want_data && d.f.size) fill.push_back(k);
                }
                // the files' bytes out of the pinned slab, on a few host threads
                if (!fill.empty())
                    parallel_for((int)fill.size(), pk_off[m], [&](int j) {
                        const int k = fill[(size_t)j];
                        dec[(size_t)todo[k]].f.data.assign(slab + pk_off[k], slab + pk_off[k] + len[k]);
                    });
                todo.swap(again);
            }
        }
    }
    return ZPQ_OK;
}

// one context's share of the multi-segment blocks: per distinct header sets of as many blocks as one may hold
static int decode_multi(zpq_ctx *ctx, const uint8_t *arc, size_t n, bool want_data, const std::vector<BlockRec> &blocks,
                        const Groups &groups, std::vector<Decoded> &dec)
{
    struct Member {
        int bi; size_t pos; std::string name, comment; std::vector<ArchiveFile> files; bool alive = true, finished = false; size_t end = 0;
    };
    for (const auto &g : groups) {
        const BlockRec &b0 = blocks[(size_t)g.second[0]];
        zpq_model *model = nullptr;
        if (zpq_model_create(b0.hdr.data(), (int)b0.hdr.size(), b0.cend, b0.hbegin, b0.hend, &model) != ZPQ_OK) continue;
        struct ModelGuard { zpq_model *m; ~ModelGuard() { zpq_model_destroy(m); } } guard{model};
        for (size_t c0 = 0; c0 < g.second.size();) {
            // the decoded sizes are not known: the line store is sized for eight times the coded bytes (a member that needs
            // more gets ZPQ_E_TOOBIG and is replayed sequentially)
            uint64_t mmb = 0;
            size_t c1 = c0;
            int capn = 0;
            for (; c1 < g.second.size(); c1++) {
                const BlockRec &b = blocks[(size_t)g.second[c1]];
                const uint64_t m2 = std::max<uint64_t>(mmb, (uint64_t)(b.next_tag - b.payload) * 8 + 65536);
                if (c1 == c0 || m2 != mmb) capn = zpq_blockset_capacity(ctx, model, m2);
                if (capn < 1 || (int)(c1 - c0) + 1 > capn) break;
                mmb = m2;
            }
            if (c1 == c0) { c0++; continue; }                                   // does not fit at all: replayed
            std::vector<Member> mem;
            for (size_t c = c0; c < c1; c++) {
                const BlockRec &b = blocks[(size_t)g.second[c]];
                Member m;
                m.bi = g.second[c]; m.pos = b.payload; m.name = b.name; m.comment = b.comment;
                mem.push_back(std::move(m));
            }
            c0 = c1;
            zpq_blockset *set = nullptr;
            if (zpq_blockset_create(ctx, model, (int)mem.size(), mmb, &set) != ZPQ_OK) continue;   // replayed
            struct SetGuard { zpq_blockset *s; ~SetGuard() { zpq_blockset_destroy(s); } } sguard{set};
            std::vector<uint8_t> out;
            for (;;) {
                // the members still going, in archive order: a range may run on to the next member's segment (the decoder
                // stops at the EOF symbol), so the ranges are contiguous
                std::vector<int32_t> member;
                for (size_t j = 0; j < mem.size(); j++) if (mem[j].alive && !mem[j].finished) member.push_back((int32_t)j);
                const int k = (int)member.size();
                if (!k) break;
                std::vector<uint64_t> in_off((size_t)k + 1), out_off((size_t)k + 1, 0);
                for (int j = 0; j < k; j++) {
                    const Member &m = mem[(size_t)member[(size_t)j]];
                    const BlockRec &b = blocks[(size_t)m.bi];
                    in_off[(size_t)j] = m.pos;
                    const uint64_t hint = size_hint(m.comment), paylen = b.next_tag - m.pos;
                    uint64_t cap = paylen * 8 + 65536;
                    if (hint != ~0ull) cap = std::min<uint64_t>(hint + 64, paylen * 4096 + 65536);
                    out_off[(size_t)j + 1] = out_off[(size_t)j] + ((cap + 15) & ~15ull);
                }
                in_off[(size_t)k] = blocks[(size_t)mem[(size_t)member[(size_t)k - 1]].bi].next_tag;
                out.resize((size_t)out_off[(size_t)k] + 16);
                std::vector<uint32_t> meta((size_t)k * 4);
                std::vector<int32_t> st((size_t)k);
                uint32_t *len = meta.data(), *cons = len + k, *code = cons + k, *first = code + k;
                const int rc = zpq_blockset_decode_segments(set, k, member.data(), arc, in_off.data(), ZPQ_FLAG_PP, out.data(), out_off.data(),
                                                            len, cons, code, first, st.data());
                if (rc != ZPQ_OK) return rc;
                std::vector<uint8_t> sha((size_t)k * 20);
                uint64_t tot = 0;
                for (int j = 0; j < k; j++) if (st[(size_t)j] == ZPQ_OK) tot += len[j];
                parallel_for(k, tot, [&](int j) { if (st[(size_t)j] == ZPQ_OK) host_sha1(out.data() + out_off[(size_t)j], len[j], &sha[(size_t)j * 20]); });
                for (int j = 0; j < k; j++) {
                    Member &m = mem[(size_t)member[(size_t)j]];
                    m.alive = false;                                              // until the segment proves clean
                    if (st[(size_t)j] != ZPQ_OK || first[j] != 0u) continue;      // overflow, store full, PP byte != 0: replayed
                    // Decoder.skip (decoder.v:151-196) and read_segment_end (decompressor.v:590-635), as in pass 3
                    size_t p = m.pos + cons[j];
                    auto get = [&]() -> int { return p < n ? arc[p++] : -1; };
                    uint32_t curr = code[j];
                    bool ok = true;
                    int marker = -1;
                    if (curr == 0) { const int c = get(); if (c < 0) ok = false; else curr = (uint32_t)c; }
                    while (ok && curr != 0) { const int c = get(); if (c < 0) { ok = false; break; } curr = (curr << 8) | (uint32_t)c; }
                    while (ok) { const int c = get(); if (c < 0) break; if (c != 0) { marker = c; break; } }
                    if (marker == 253) {
                        if (p + 20 > n || memcmp(arc + p, &sha[(size_t)j * 20], 20) != 0) continue;
                        p += 20;
                    } else if (marker != 254) continue;
                    if (p >= blocks[(size_t)m.bi].next_tag) continue;            // ran out of its block: damage
                    ArchiveFile f;
                    f.name = m.name; f.comment = m.comment; f.size = len[j];
                    if (want_data) f.data.assign(out.data() + out_off[(size_t)j], out.data() + out_off[(size_t)j] + len[j]);
                    m.files.push_back(std::move(f));
                    // find_filename for the next segment (decompressor.v:350-429)
                    const int after = get();
                    if (after == 0xFF) { m.alive = true; m.finished = true; m.end = p; continue; }
                    if (after != 1) continue;
                    m.name.clear(); m.comment.clear();
                    bool good = true;
                    for (;;) { const int c = get(); if (c < 0 || c == 0xFF) { good = false; break; } if (c == 0) break; m.name.push_back((char)c); }
                    for (; good;) { const int c = get(); if (c < 0) { good = false; break; } if (c == 0) break; m.comment.push_back((char)c); }
                    if (!good || get() < 0 || p >= blocks[(size_t)m.bi].next_tag) continue;
                    m.pos = p;
                    m.alive = true;
                }
            }
            for (Member &m : mem) {
                if (!m.finished || m.files.empty()) continue;
                Decoded &d = dec[(size_t)m.bi];
                d.done = true;
                d.end = m.end;
                d.f = std::move(m.files[0]);
                d.more.assign(std::make_move_iterator(m.files.begin() + 1), std::make_move_iterator(m.files.end()));
            }
        }
    }
    return ZPQ_OK;
}

}  // namespace zpaq

// ------------------------------------------------------------------ flat C surface for ctypes
// (C++ exceptions stop here: *rc = ZPQ_E_INTERNAL / ZPQ_E_NOMEM and an empty handle, never an abort)
struct zpqf_archive {
    std::vector<uint8_t> bytes;
    std::vector<zpaq::ArchiveFile> files;
};

namespace {
template <class F> zpqf_archive *archive_call(int *rc, const char *where, F &&f) noexcept
{
    zpqf_archive *h = nullptr;
    int r = ZPQ_E_INTERNAL;
    try {
        h = new zpqf_archive();
        r = f(h);
    } catch (const std::bad_alloc &) {
        zpq_note_exception(where);
        r = ZPQ_E_NOMEM;
    } catch (...) {
        zpq_note_exception(where);
        r = ZPQ_E_INTERNAL;
    }
    if (rc) *rc = r;
    return h;
}
const zpaq::ArchiveFile *file_at(zpqf_archive *h, int i) { return (h && i >= 0 && (size_t)i < h->files.size()) ? &h->files[(size_t)i] : nullptr; }
}  // namespace

extern "C" {
zpqf_archive *zpqf_archive_add_fragmented(zpq_ctx *ctx, int level, int nfiles, const char *const *names, const char *const *comments,
                                          const uint8_t *const *data, const uint64_t *lens, uint64_t fragment_bytes, int *rc)
{
    return archive_call(rc, __func__, [&](zpqf_archive *h) {
        return zpaq::archive_add_views(std::vector<zpq_ctx *>{ctx}, level, nfiles, names, comments, data, lens, &h->bytes, (size_t)fragment_bytes);
    });
}
zpqf_archive *zpqf_archive_add_multi(zpq_ctx *const *ctxs, int nctx, int level, int nfiles, const char *const *names,
                                     const char *const *comments, const uint8_t *const *data, const uint64_t *lens,
                                     uint64_t fragment_bytes, int *rc)
{
    return archive_call(rc, __func__, [&](zpqf_archive *h) {
        if (!ctxs || nctx <= 0) return (int)ZPQ_E_ARG;
        return zpaq::archive_add_views(std::vector<zpq_ctx *>(ctxs, ctxs + nctx), level, nfiles, names, comments, data, lens, &h->bytes,
                                       (size_t)fragment_bytes);
    });
}
zpqf_archive *zpqf_archive_add_solid(zpq_ctx *const *ctxs, int nctx, int level, int nfiles, const char *const *names,
                                     const char *const *comments, const uint8_t *const *data, const uint64_t *lens,
                                     uint64_t fragment_bytes, int solid_files, int *rc)
{
    return archive_call(rc, __func__, [&](zpqf_archive *h) {
        if (!ctxs || nctx <= 0) return (int)ZPQ_E_ARG;
        return zpaq::archive_add_views(std::vector<zpq_ctx *>(ctxs, ctxs + nctx), level, nfiles, names, comments, data, lens, &h->bytes,
                                       (size_t)fragment_bytes, solid_files);
    });
}
zpqf_archive *zpqf_archive_extract_multi(zpq_ctx *const *ctxs, int nctx, const uint8_t *arc, size_t n, int want_data, int *rc)
{
    return archive_call(rc, __func__, [&](zpqf_archive *h) {
        if (!ctxs || nctx <= 0) return (int)ZPQ_E_ARG;
        return zpaq::archive_extract(std::vector<zpq_ctx *>(ctxs, ctxs + nctx), arc, n, (want_data & 1) != 0, &h->files, (want_data & 2) != 0);
    });
}
zpqf_archive *zpqf_archive_add(zpq_ctx *ctx, int level, int nfiles, const char *const *names, const char *const *comments,
                               const uint8_t *const *data, const uint64_t *lens, int *rc)
{
    return zpqf_archive_add_fragmented(ctx, level, nfiles, names, comments, data, lens, 0, rc);
}
size_t zpqf_archive_bytes(zpqf_archive *h, const uint8_t **p)
{
    if (!h || !p) return 0;
    *p = h->bytes.data();
    return h->bytes.size();
}
zpqf_archive *zpqf_archive_extract(zpq_ctx *ctx, const uint8_t *arc, size_t n, int want_data, int *rc)
{
    return archive_call(rc, __func__, [&](zpqf_archive *h) {
        return zpaq::archive_extract(ctx, arc, n, (want_data & 1) != 0, &h->files, (want_data & 2) != 0);
    });
}
int zpqf_archive_nfiles(zpqf_archive *h) { return h ? (int)h->files.size() : 0; }
const char *zpqf_archive_name(zpqf_archive *h, int i) { const zpaq::ArchiveFile *f = file_at(h, i); return f ? f->name.c_str() : ""; }
const char *zpqf_archive_comment(zpqf_archive *h, int i) { const zpaq::ArchiveFile *f = file_at(h, i); return f ? f->comment.c_str() : ""; }
uint64_t zpqf_archive_size(zpqf_archive *h, int i) { const zpaq::ArchiveFile *f = file_at(h, i); return f ? f->size : 0; }
int zpqf_archive_sha1_ok(zpqf_archive *h, int i) { const zpaq::ArchiveFile *f = file_at(h, i); return (f && f->sha1_ok) ? 1 : 0; }
int zpqf_archive_status(zpqf_archive *h, int i) { const zpaq::ArchiveFile *f = file_at(h, i); return f ? f->status : ZPQ_E_ARG; }
const uint8_t *zpqf_archive_data(zpqf_archive *h, int i) { const zpaq::ArchiveFile *f = file_at(h, i); return f ? f->data.data() : nullptr; }
void zpqf_archive_free(zpqf_archive *h) { zpq_guard_v(__func__, [&] { delete h; }); }
}
