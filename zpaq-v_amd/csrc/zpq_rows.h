// zpq_rows.h -- what every kernel that keeps bit histories states the same way: find_ht's lookup of a nibble's row among
// three candidates, the compact line store's probe, and the two shipped context programs evaluated in registers.  What a
// kernel does around them (when a request goes out, what it forwards from registers, when a store is issued) stays in
// the kernel.  Brought in like zpq_dev.h (`using namespace zpqdev;`).
// Plain functions of values that return small structs where that leaves the shipped levels' kernels (k_chain, k_pipe,
// k_pipe2, k_dpipe) the code they had; macros (ZPQ_...) where it does not: those kernels are scheduled to the
// instruction, and the compiler lays a function that is simplified on its own before it is inlined out differently from
// the same lines written in place (tools/isa_identity.py is the check; EXPERIMENTS.md R21 has what was tried).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace zpqdev {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ---- find_ht (predictor.v:495-532).  A context's three candidate rows h0, h0 ^ 16, h0 ^ 32 share one 64-byte line.
struct RowReq { uint32_t chk, h0; };              // the check byte a row must carry, candidate A's offset in the dense table
__device__ __forceinline__ RowReq row_request(const uint32_t hc, const uint32_t c8v, const int sizebits, const uint32_t ht_mask)
{
    const uint32_t cx = hc + 16u * c8v;
    return RowReq{(cx >> sizebits) & 255u, (cx * 16u) & ht_mask};
}
struct Cands { u32x4 A, B, C; };
// NO_ROWS: a kernel file's *_DEBUG_NO_ROWS timing switch (wrong output): no hash-row traffic at all
template <bool NO_ROWS = false>
__device__ __forceinline__ Cands load_cands(const uint8_t *tbase, const uint32_t po)
{
    Cands c;
    if (NO_ROWS) { c.A = u32x4{po, 0, 0, 0}; c.B = c.A; c.C = c.A; return c; }
    c.A = *reinterpret_cast<const u32x4 *>(tbase + po);
    c.B = *reinterpret_cast<const u32x4 *>(tbase + (po ^ 16u));
    c.C = *reinterpret_cast<const u32x4 *>(tbase + (po ^ 32u));
    return c;
}
// Hit / victim with selects only, in two steps.  ZPQ_ROW_PICK decides on the candidates' FIRST dwords (check byte and
// priority live there) and declares hit (a candidate carries the check byte), ua (the row is A) and ub (it is B, else C)
// in the caller's scope; pick3 then takes whatever belongs to the chosen candidate -- the whole row at once (find_row),
// dword by dword, or (zpq_pipe.hip ZPP_FWD_FIND) the rest of it from wherever its newest copy is.
// (A macro, not a function returning the three flags: handed on in a struct they reach the selects as bytes, and every
//  kernel came out with branches where it had selects.)
#define ZPQ_ROW_PICK(ax_, bx_, cx_, chk_)                                                                               \
    const bool ma_ = ((ax_) & 255u) == (chk_), mb_ = ((bx_) & 255u) == (chk_), mc_ = ((cx_) & 255u) == (chk_);         \
    const uint32_t qa_ = ((ax_) >> 8) & 255u, qb_ = ((bx_) >> 8) & 255u, qc_ = ((cx_) >> 8) & 255u;                     \
    const bool va_ = qa_ <= qb_ && qa_ <= qc_, vb_ = qb_ < qc_;             /* victim order (predictor.v:513-531) */    \
    const bool hit = ma_ || mb_ || mc_;                                                                                 \
    const bool ua = ma_ || (!hit && va_);                                                                               \
    const bool ub = !ua && (mb_ || (!hit && vb_))
template <class T>
__device__ __forceinline__ T pick3(const bool ua, const bool ub, const T a, const T b, const T c) { return ua ? a : (ub ? b : c); }
// a nibble's bit-history row (byte 0 = check) and its offset from the table's base; a miss starts the victim over
struct Row { uint32_t x, y, z, w, off; };
__device__ __forceinline__ Row row_new(const bool hit, const uint32_t x, const uint32_t y, const uint32_t z, const uint32_t w, const uint32_t chk, const uint32_t off)
{
    Row R;
    R.off = off;
    R.x = hit ? x : chk; R.y = hit ? y : 0u; R.z = hit ? z : 0u; R.w = hit ? w : 0u;
    return R;
}
// pa, pb = pa ^ 16, pc = pa ^ 32: the candidates' offsets (the caller's values: most callers compare them as well)
__device__ __forceinline__ Row find_row(const Cands c, const uint32_t chk, const uint32_t pa, const uint32_t pb, const uint32_t pc)
{
    ZPQ_ROW_PICK(c.A.x, c.B.x, c.C.x, chk);
    const uint32_t off = pick3(ua, ub, pa, pb, pc);
    const u32x4 R = pick3(ua, ub, c.A, c.B, c.C);
    return row_new(hit, R.x, R.y, R.z, R.w, chk, off);
}

// ---- The compact line store (zpq_model.cpp zpq_sparse_layout): dense line index -> slot.  Open addressing over GROUPS
// of four slots: a line's key is its dense index + 1 (0 = free), its home slot mulhi(key * 0x9E3779B1, cap) (capacity
// need not be a power of two); probing visits the home group's slots cyclically from the home slot, then the following
// groups the same way.  One 16-byte load brings the home group's four tags, and the HOME slot's rows are fetched with
// them: a line that sits in its home slot, or a new line (it takes the first free slot it meets, and a new line is all
// zero -- nothing to load), costs one memory round trip; only a line that was displaced when it was claimed needs a
// second one for its rows, and only a full group is walked past.  A block that needs more than 15/16 of the store is
// refused before probes get long.  The kernels differ in when a claim's stores are issued, who may walk and how a
// refusal is recorded; that stays with them.
__device__ __forceinline__ uint32_t sp_key(const uint32_t h0) { return (h0 >> 6) + 1u; }
__device__ __forceinline__ uint32_t sp_home(const uint32_t key, const uint32_t cap) { return __umulhi(key * 0x9E3779B1u, cap); }
#define ZPQ_SP_LIMIT(cap_) ((cap_) - ((cap_) >> 4))                     /* claims a store takes before it refuses its block */
// The walk: T0_ = the home group's tags (fetched with the home slot's rows).  Declares in the caller's scope r (0: the
// probe did not end: every slot taken, or may_walk_ said no), si (the slot where it ended) and t (what that slot holds:
// the key, or 0 = free).  may_walk_ goes into the condition as written (no parentheses): whoever may not walk -- a
// store that has refused its block, the copy that resolves for a context that never came -- stays in the home group.
// (Macros like ZPQ_ROW_PICK, and for the same reason: as functions, even the limit alone, they moved instructions in the
// shipped levels' kernels.)
#define ZPQ_SP_WALK(tags_, groups_, key_, home_, T0_, may_walk_)                                                        \
    const uint32_t o_ = (home_) & 3u;                                                                                   \
    /* slots of a group that end the probe -- the line's own tag, or a free slot -- as a 4-bit mask rotated so that */  \
    /* bit j stands for slot (o_ + j) & 3: the lowest set bit is the first such slot met */                             \
    auto probe_group_ = [&](const zpqdev::u32x4 T) -> uint32_t {                                                        \
        const uint32_t mm = (min(T.x ^ (key_), T.x) == 0u ? 1u : 0u) | (min(T.y ^ (key_), T.y) == 0u ? 2u : 0u) |       \
                            (min(T.z ^ (key_), T.z) == 0u ? 4u : 0u) | (min(T.w ^ (key_), T.w) == 0u ? 8u : 0u);        \
        return ((mm * 17u) >> o_) & 15u;                                                                                \
    };                                                                                                                  \
    zpqdev::u32x4 T_ = (T0_);                                                                                           \
    uint32_t g_ = (home_) >> 2;                                                                                         \
    uint32_t r = probe_group_(T_);                                                                                      \
    if (r == 0u && may_walk_) {                                        /* home group full of other lines: walk on */    \
        for (uint32_t tries_ = 1; tries_ < (groups_); tries_++) {                                                       \
            g_ = (g_ + 1u == (groups_)) ? 0u : g_ + 1u;                                                                 \
            T_ = *reinterpret_cast<const zpqdev::u32x4 *>((tags_) + 4u * g_);                                           \
            r = probe_group_(T_);                                                                                       \
            if (r) break;                                                                                               \
        }                                                                                                               \
    }                                                                                                                   \
    const uint32_t idx_ = (o_ + (uint32_t)__builtin_ctz(r | 16u)) & 3u;                                                 \
    const uint32_t t = (idx_ & 2u) ? ((idx_ & 1u) ? T_.w : T_.z) : ((idx_ & 1u) ? T_.y : T_.x);                         \
    const uint32_t si = 4u * g_ + idx_
// a claim: the slot's tag, and the line all zero, like an untouched dense line
#define ZPQ_SP_CLAIM(tags_, si_, key_, line_)                                                                           \
    do {                                                                                                                \
        const zpqdev::u32x4 z4_ = {0, 0, 0, 0};                                                                         \
        uint8_t *l_ = (line_);                                                                                          \
        (tags_)[(si_)] = (key_);                                                                                        \
        *reinterpret_cast<zpqdev::u32x4 *>(l_) = z4_;                                                                   \
        *reinterpret_cast<zpqdev::u32x4 *>(l_ + 16) = z4_;                                                              \
        *reinterpret_cast<zpqdev::u32x4 *>(l_ + 32) = z4_;                                                              \
        *reinterpret_cast<zpqdev::u32x4 *>(l_ + 48) = z4_;                                                              \
    } while (0)

// ---- The shipped levels' context programs (ZPAQL.run(byte) + h[] copy, predictor.v:809-816) in registers.
__device__ __forceinline__ uint32_t hash_step(const uint32_t a, const uint32_t x) { return (a + x + 512u) * 773u; }   // HASH (zpaql.v)
// levels 2-5: b=c c-- *c=a d=0 (hash *d=a d++)* hash *d=a halt: H[k] = hash^(k+1) of (byte, prev), i.e. k + 1 steps
// `a = hash_step(a, prev)` from a = byte; the caller keeps prev = byte.  (The loop stays with the callers: some keep the
// link that is their lane's on the way, and as a function of the depth it moved instructions in k_pipe.)
// level 1: *b=a a=0 d=0 hash b-- hash *d=a d++ b-- hash b-- hash *d=a halt, M = 4 bytes (m4), B = b4, which ends 3 lower.
// level1_put is the program's first step (M as the byte leaves it), level1_hashes the rest: H[0], H[1].
__device__ __forceinline__ uint32_t level1_put(const uint32_t m4, const uint32_t b4, const uint32_t byte)
{
    return (m4 & ~(255u << ((b4 & 3) * 8))) | (byte << ((b4 & 3) * 8));
}
struct Level1 { uint32_t h0, h1; };
__device__ __forceinline__ Level1 level1_hashes(const uint32_t mm, const uint32_t b4)
{
    uint32_t bb = b4;
    uint32_t a = 0;
    a = hash_step(a, (mm >> ((bb & 3) * 8)) & 255u); bb--;
    a = hash_step(a, (mm >> ((bb & 3) * 8)) & 255u);
    const uint32_t h0v = a; bb--;
    a = hash_step(a, (mm >> ((bb & 3) * 8)) & 255u); bb--;
    a = hash_step(a, (mm >> ((bb & 3) * 8)) & 255u);
    return Level1{h0v, a};
}

}  // namespace zpqdev
