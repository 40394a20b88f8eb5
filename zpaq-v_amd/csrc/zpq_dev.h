// zpq_dev.h -- device primitives every kernel file states the same way: the reference's wrapping arithmetic and clamps,
// the coder's range multiply, the LDS barrier, and Predictor.init's fill of one state slot.  A kernel file brings them
// into its own namespace (`using namespace zpqdev;`), so call sites read as before.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zpq_common.h"

namespace zpqdev {

// V's int arithmetic wraps (predictor.v); C++'s signed overflow is undefined, so: through unsigned
__device__ __forceinline__ int32_t wadd(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
__device__ __forceinline__ int32_t wsub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
__device__ __forceinline__ int32_t wmul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }
__device__ __forceinline__ int32_t clamp2k(int32_t x) { return min(max(x, -2048), 2047); }
__device__ __forceinline__ int32_t clamp512k(int32_t x) { return min(max(x, -262144), 262143); }
// (u64(range) * p16) >> 16 for p16 < 2^16 (encoder.v:60-61, decoder.v:86-87) without the 64-bit multiply:
// range = hi * 2^16 + lo  =>  hi * p16 + ((lo * p16) >> 16), both products of 16-bit operands (two full-rate v_mul_u32_u24)
__device__ __forceinline__ uint32_t mul_shr16(uint32_t range, uint32_t p16)
{
    return (uint32_t)__umul24(range >> 16, p16) + ((uint32_t)__umul24(range & 0xFFFFu, p16) >> 16);   // (__umul24 returns int)
}
// LDS traffic of this wave done, then the workgroup barrier (no wait for global memory: loads and stores stay in flight)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- Predictor.init + ZPAQL.clear of one state slot (predictor.v:325-470, zpaql.v:54-95), in three steps.  The calling
// thread takes elements first, first + stride, ...; what orders the zeroing before the fills (a workgroup barrier, or a
// wave barrier between fences) is the caller's, as is who calls: a wave, a row of lanes, a workgroup.
__device__ __forceinline__ void slot_zero(const DModel &M, uint8_t *slot, const uint32_t first, const uint32_t stride)
{
    uint4 *z4 = reinterpret_cast<uint4 *>(slot);
    const uint64_t n16 = M.zero_bytes / 16;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    for (uint64_t i = first; i < n16; i += stride) z4[i] = zero;
}
// the tables that do not start as zeroes: ZF_CONST, ZF_PATTERN from the init image, the a16 tables
__device__ __forceinline__ void slot_fill(const DModel &M, const uint32_t *img, uint8_t *slot, const uint32_t first, const uint32_t stride)
{
    for (int32_t ci = 0; ci < M.n; ci++) {
        const DComp &c = M.comp[ci];
        if (c.cm_len && c.cm_fill != ZF_ZERO) {
            uint32_t *t = reinterpret_cast<uint32_t *>(slot + c.cm_off);
            if (c.cm_fill == ZF_CONST) { for (uint32_t i = first; i < c.cm_len; i += stride) t[i] = c.cm_fill_val; }
            else { const uint32_t *im = img + c.cm_fill_val; for (uint32_t i = first; i < c.cm_len; i += stride) t[i] = im[i % c.cm_pat_len]; }
        }
        if (c.a16_len && c.a16_fill) {
            uint16_t *t = reinterpret_cast<uint16_t *>(slot + c.a16_off);
            for (uint32_t i = first; i < c.a16_len; i += stride) t[i] = (uint16_t)c.a16_fill;
        }
    }
}
// Quirk Q17: Predictor.init leaves sizebits / bufbits in a MATCH's cr.a / cr.b (predictor.v:372-373), which predict / update
// then read as the initial match length and offset (:566-572).  For the kernels that keep MATCH's scalars in the slot.
__device__ __forceinline__ void slot_match_init(const DModel &M, uint8_t *slot, const uint32_t first, const uint32_t stride)
{
    DCompScal *gs = reinterpret_cast<DCompScal *>(slot + M.scal_off);
    for (uint32_t ci = first; ci < (uint32_t)M.n; ci += stride)
        if (M.comp[ci].type == ZT_MATCH) { gs[ci].a = M.comp[ci].a; gs[ci].b = M.comp[ci].b; }
}


// ---- The dirty-line log (DBatch::dlog).  Invariant: after a launch that keeps the log, every byte of a slot's zero_bytes
// is zero except in the 64-byte lines of hashed table c whose offsets are entries [0, count) of the slot's log for c;
// count == dlog_cap says the log overflowed and the whole table may be dirty.  Per slot and table: DLOG_HDR words (word 0 =
// count), then the entries (room rounded up to four: a thread reads four entries with one load).  The tables are the
// model's components [0, nt), all hashed (a chain without a MIX2).
constexpr uint32_t DLOG_HDR = 16;
__host__ __device__ __forceinline__ uint64_t dlog_stride(const uint32_t cap) { return DLOG_HDR + (((uint64_t)cap + 3u) & ~3ull); }
__device__ __forceinline__ uint32_t *dlog_table(const DBatch &B, const int slot_id, const int c, const int nt)
{
    return B.dlog + ((uint64_t)slot_id * (uint32_t)nt + (uint32_t)c) * dlog_stride(B.dlog_cap);
}
// zero the logged lines of one table: a thread takes four entries per load and whole lines, two loads in flight (the
// entry is a dependent load in front of its stores: one at a time the loop would run at one memory round trip per line)
__device__ __forceinline__ void dlog_zero_lines(uint8_t *tb, const uint32_t ht_len, const uint32_t *lg, const uint32_t cnt,
                                                const uint32_t first, const uint32_t stride)
{
    const uint4 zero = make_uint4(0, 0, 0, 0);
    const uint32_t mask = ht_len - 64u;                    // (a table is a power of two of at least one line: no entry leaves it)
    const uint4 *e4 = reinterpret_cast<const uint4 *>(lg + DLOG_HDR);
    const uint32_t nq = (cnt + 3u) >> 2;
    auto z = [&](const uint32_t idx, const uint32_t off) {
        if (idx < cnt) {
            uint4 *l = reinterpret_cast<uint4 *>(tb + (off & mask));
            l[0] = zero; l[1] = zero; l[2] = zero; l[3] = zero;
        }
    };
    for (uint32_t q = first; q < nq; q += 2u * stride) {
        const uint32_t q1 = q + stride;
        const uint4 a = e4[q];
        const uint4 b = e4[min(q1, nq - 1u)];
        z(4u * q, a.x); z(4u * q + 1u, a.y); z(4u * q + 2u, a.z); z(4u * q + 3u, a.w);
        if (q1 < nq) { z(4u * q1, b.x); z(4u * q1 + 1u, b.y); z(4u * q1 + 2u, b.z); z(4u * q1 + 3u, b.w); }
    }
}
__device__ __forceinline__ void dlog_zero_range(uint8_t *slot, const uint64_t from, const uint64_t to, const uint32_t first, const uint32_t stride)
{
    uint4 *z4 = reinterpret_cast<uint4 *>(slot + from);
    const uint64_t n16 = to > from ? (to - from) / 16 : 0;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    for (uint64_t i = first; i < n16; i += stride) z4[i] = zero;
}
// what of a slot no table holds: in front of, between and behind the tables (components lie in the slot in their order)
__device__ __forceinline__ void dlog_zero_rest(const DModel &M, uint8_t *slot, const int nt, const uint32_t first, const uint32_t stride)
{
    uint64_t from = 0;
    for (int c = 0; c < nt; c++) {
        dlog_zero_range(slot, from, M.comp[c].ht_off, first, stride);
        from = M.comp[c].ht_off + M.comp[c].ht_len;
    }
    dlog_zero_range(slot, from, M.zero_bytes, first, stride);
}
// one table of a slot whose log is valid: its logged lines, or all of it after an overflow
__device__ __forceinline__ void dlog_clear_table(const DBatch &B, const DModel &M, uint8_t *slot, const int slot_id, const int c, const int nt,
                                                 const uint32_t first, const uint32_t stride)
{
    const uint32_t *lg = dlog_table(B, slot_id, c, nt);
    const uint32_t cnt = lg[0];
    if (cnt >= B.dlog_cap) dlog_zero_range(slot, M.comp[c].ht_off, M.comp[c].ht_off + M.comp[c].ht_len, first, stride);
    else dlog_zero_lines(slot + M.comp[c].ht_off, M.comp[c].ht_len, lg, cnt, first, stride);
}

}  // namespace zpqdev
