/*
 * zpaq_hip.h -- C ABI of libzpaq_hip.so: the MI355X (gfx950) ZPAQ block codec.
 *
 * This is the drop-in boundary for ONE hot path of dy-tea/zpaq-v: the bit-serial
 * context-mixing coder.  Each entry point cites the reference interface it
 * replaces (file:line under the reference's zpaq/ directory).  The reference's
 * front end (compressor.v / decompressor.v) keeps its API; its per-byte calls
 *     c.enc.compress(ch)            compressor.v:272,287,375-378
 *     d.dec.decompress()            decompressor.v:470,485
 * are lifted to one call per SEGMENT (zpq_block_*) or per BATCH of independent
 * blocks (zpq_encode_blocks / zpq_decode_blocks).  INTEGRATION.md shows the V
 * `fn C.…` binding a maintainer would add.
 *
 * Conventions: extern "C", plain pointers and sizes, caller-owned buffers that
 * must stay valid for the duration of the call, int return = ZPQ_OK or a
 * negative ZPQ_E_* code, never aborts, no exceptions.  All results are
 * bit-identical to the reference's V CPU path (as restated by oracle/).
 * There is NO CPU fallback: without a HIP device every compute entry point
 * returns ZPQ_E_NODEVICE.
 */
#ifndef ZPAQ_HIP_H
#define ZPAQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (library-level returns and per-block status[]) ---- */
#define ZPQ_OK 0
#define ZPQ_E_NODEVICE (-1)  /* no HIP device / HIP runtime failure */
#define ZPQ_E_ARG (-2)       /* NULL pointer, negative count, bad offsets */
#define ZPQ_E_HEADER (-3)    /* malformed COMP/HCOMP header (V would panic on an index) */
#define ZPQ_E_TOOBIG (-4)    /* a table the header asks for exceeds the supported size */
#define ZPQ_E_MIX_M0 (-5)    /* MIX with m==0: the reference divides by m (predictor.v:426) */
#define ZPQ_E_NOMEM (-6)     /* host or device allocation failed */
#define ZPQ_E_OVERFLOW (-7)  /* per block: output slab too small (out_len holds the needed size if known) */
#define ZPQ_E_VMSTEPS (-8)   /* per block: HCOMP exceeded ZPQ_VM_STEP_CAP steps in one run (reference would hang) */
#define ZPQ_E_INTERNAL (-9)  /* self-check failed, or a C++ exception (host allocation, the HIP runtime) was stopped at this boundary */
#define ZPQ_E_CLOSED (-10)   /* the zpq_ctx this handle (a ctx pointer, a zpq_block) belongs to has been destroyed */

#define ZPQ_VM_STEP_CAP (1u << 20)

/* ---- flags ---- */
#define ZPQ_FLAG_PP 1u        /* encode: code a leading PP-mode byte 0 first (compressor.v:271-274).
                                 decode: drop the first decoded byte (the PP byte) from the output
                                 and report it in first_byte[] (decompressor.v:469-475). */
#define ZPQ_FLAG_GENERIC 2u   /* force the generic all-component interpreter kernel */
#define ZPQ_FLAG_LANES 8u     /* force the lane-per-component kernel (any model with <= 64 components) */
#define ZPQ_FLAG_NOEOF 4u     /* encode: stop after the last data byte, no compress(-1)/flush().  Only the
                                 reference's component-less end_segment path needs it (compressor.v:364). */
#define ZPQ_FLAG_VMPIPE 16u   /* a request: code a general model whose HCOMP program is NOT the shipped hash chain on the
                                 wave-per-component kernels with an interpreter wave (k_vpipe / k_vdec) instead of
                                 k_rows.  Honoured when no chain kernel takes the model, neither ZPQ_FLAG_GENERIC nor
                                 ZPQ_FLAG_NOEOF is set and the model is in those kernels' envelope (the nine component
                                 types, inputs earlier than their consumer, a MIX of 1-8 inputs, at most 14
                                 components, rings and header within the LDS); otherwise the call runs exactly as
                                 without it.  The coded bytes are the same either way; zpq_ctx_last_kernel_name tells
                                 which kernel ran ("k_vpipe<encode>" / "k_vdec<decode>").  All batch entry points
                                 (host, _dev, _multi) honour it, and zpq_ctx_resident_capacity answers for the pair
                                 it selects.  zpq_block_* and zpq_blockset_* ignore both the flag and the variable: a
                                 block's first segment runs on the batch kernel it ran on before (k_rows for such a
                                 model), later segments on k_generic; a block set runs on k_generic, or on k_rows /
                                 k_lanes under ZPQ_SET_LANES.  The way onto these kernels' state hand-over forms for a
                                 block set is the set's own flag, ZPQ_SET_VMWAVES (below).  The environment decides first:
                                 ZPQ_VM_PIPE=1 sets it for every call, ZPQ_VM_PIPE=0 clears it (a value that starts
                                 with neither digit decides nothing). */
#define ZPQ_FLAG_LINESTORE 32u /* a request: code a general model on k_rows / k_lanes with every ICM / ISSE table that is
                                 larger than the compact line store (68 bytes per line of zpq_ctx_set_max_block_bytes'
                                 capacity) kept on such a store instead of a dense table, as the chain kernels keep
                                 the tables of levels 3-5.  A slot then holds a few MiB where the dense one holds up to
                                 1 GiB per table: more resident blocks, nothing but the tags to clear per block, and
                                 batches that otherwise end in ZPQ_E_NOMEM.  Honoured when the call reaches the
                                 lane-per-component kernels (no chain kernel takes it, or ZPQ_FLAG_LANES; neither
                                 ZPQ_FLAG_GENERIC nor ZPQ_FLAG_NOEOF; at most 64 components), ZPQ_SPARSE_MODE is not
                                 "never" and zpq_lanes_store_applies(model, capacity) holds; otherwise the call runs
                                 exactly as without it.  A honoured request runs k_rows / k_lanes also where the wave
                                 pipelines (k_gpipe / k_gdec, k_vpipe / k_vdec) would apply: those have no store.  The
                                 coded bytes are the same either way; the kernel names stay "k_rows<...>" /
                                 "k_lanes<...>" and zpq_ctx_last_line_store reports the capacity (0 = dense).  A block
                                 that touches more than 15/16 of the capacity in lines of one table -- larger than
                                 zpq_ctx_set_max_block_bytes promised -- ends with ZPQ_E_TOOBIG in status[] (behind
                                 ZPQ_E_VMSTEPS, ahead of ZPQ_E_OVERFLOW), its output unspecified, other blocks
                                 untouched.  All batch entry points honour it and zpq_ctx_resident_capacity follows it;
                                 zpq_block_* and zpq_blockset_* ignore the flag and the variable.  The environment
                                 decides first: ZPQ_LANES_STORE=1 / =0 by the rule of ZPQ_VM_PIPE.  Measured (MI355X,
                                 C4b with ICM and ISSE at 22 bits, 64 KiB blocks, EXPERIMENTS.md R20): it pays from the
                                 batch size at which the dense slots no longer hold the batch in one round -- 487
                                 blocks of that model's 513 MiB slot --: 3.1x / 5.8x (encode / decode) at 2048 blocks,
                                 9.1x / 16.5x at 8192; at 256 blocks, one round either way, it loses 1.47x on encode
                                 against k_gpipe and gains 1.24x on decode against k_gdec (against dense k_rows: 8 % and
                                 3 % slower, the probe).  It stays a request. */

/* ---- header helpers: levels.v:26-375 (get_compression_level) and the scan
 *      that defines cend/hbegin/hend, compressor.v:96-145 ---- */
int zpq_level_header(int level, uint8_t *buf, int cap, int *len, int *cend, int *hbegin, int *hend);
int zpq_scan_header(const uint8_t *hdr, int len, int *cend, int *hbegin, int *hend);

/* ---- model: what Predictor.init(&z) + ZPAQL.inith/initp derive from a header
 *      (predictor.v:292-470, zpaql.v:74-95).  Device independent. ---- */
typedef struct zpq_model zpq_model;
int zpq_model_create(const uint8_t *hdr, int len, int cend, int hbegin, int hend, zpq_model **out);
int zpq_model_create_level(int level, zpq_model **out);
void zpq_model_destroy(zpq_model *);
int zpq_model_ncomp(const zpq_model *);
uint64_t zpq_model_state_bytes(const zpq_model *); /* device bytes of one block's tables */
int zpq_model_has_fast_path(const zpq_model *);    /* 1 if the LDS-resident chain kernel applies */
/* ZPQ_FLAG_LINESTORE's envelope, host logic only (no device): would the request be honoured for this model on a line
 * store of cap_lines lines (what zpq_ctx_set_max_block_bytes derives from the block size), from the model's shape alone?
 * 1 when the lane-per-component kernels take the model (1-64 components), cap_lines is a multiple of 4 and at least 16,
 * at least one ICM / ISSE table is larger than the store (68 * cap_lines bytes) and the slot on the store is below 4 GiB;
 * else 0.  zpq_lanes_store_slot_bytes: the size of one block's slot under the store (compare zpq_model_state_bytes, the
 * dense slot), 0 where the store does not apply. */
int zpq_lanes_store_applies(const zpq_model *, uint32_t cap_lines);
uint64_t zpq_lanes_store_slot_bytes(const zpq_model *, uint32_t cap_lines);

/* ---- per-device context: stream, read-only tables, per-block state slots ---- */
/* Handle lifetime: handles may be destroyed in ANY order (a garbage-collected host language will).  zpq_ctx_destroy
 * releases the device state of every zpq_block still alive on the ctx and orphans it: later calls on such a block
 * return ZPQ_E_CLOSED, zpq_block_destroy still has to be called and frees the host struct only.  A zpq_block keeps
 * its zpq_model alive (zpq_model_destroy drops the creator's reference).  Calls on a destroyed zpq_ctx* return
 * ZPQ_E_CLOSED / ZPQ_E_ARG (the pointer is checked against the set of living contexts), zpq_ctx_destroy twice is a
 * no-op.  What stays the caller's duty: no call may be RUNNING on a ctx while another thread destroys it. */
typedef struct zpq_ctx zpq_ctx;
int zpq_ctx_create(int device, zpq_ctx **out);
void zpq_ctx_destroy(zpq_ctx *);
int zpq_ctx_sync(zpq_ctx *);
void *zpq_ctx_stream(zpq_ctx *); /* the hipStream_t all launches of this ctx go to */
int zpq_ctx_device(const zpq_ctx *); /* HIP device index the ctx was created on */
/* Upper bound on state-slot memory this ctx may hold (default: 85% of the HBM free at zpq_ctx_create). */
int zpq_ctx_set_state_budget(zpq_ctx *, uint64_t bytes);
/* Largest block (bytes) the caller will submit to the chain kernel: sizes the compact line store
 * that stands in for every hash table larger than it (a block of N bytes touches at most 2(N+2)
 * lines per table, predictor.v:495-532,558-560; the store holds 1.12x that).  Default 65536: level 1's
 * ISSE and all tables of levels 3-5 use the store, level 2's 4 MiB tables stay dense.  A bigger block gets
 * ZPQ_E_TOOBIG in status[] instead of wrong output. */
int zpq_ctx_set_max_block_bytes(zpq_ctx *, uint64_t bytes);
/* Resident blocks (state slots) the last batch call used; for reporting. */
int zpq_ctx_last_slots(const zpq_ctx *);
/* What the host pipeline did with the last host-pointer batch call (zpq_encode_blocks / zpq_decode_blocks of two or
 * more blocks): bit 0 = the input was uploaded in two stripes, the second one beside the running encoder; bit 1 = the
 * first stripe of the output was copied out beside the running decoder; bits 8 and up = the number of rounds.
 * 0 for a NULL or closed ctx, before any call, and after a batch call that did not go through that pipeline (a _dev
 * call, a single block or segment, a call that failed or was refused for its arguments).  Calls that code nothing
 * (zpq_gather_dev, zpq_sha1_*) leave it as it is.  For reporting and for tests that must know which transfer path
 * they exercised. */
unsigned zpq_ctx_last_host_transfer(const zpq_ctx *);
/* Capacity (64-byte lines per hash table) of the compact line store the last batch call's kernel ran with;
 * 0 = dense tables.  For reporting and for tests that must know which instantiation they exercised. */
unsigned zpq_ctx_last_line_store(const zpq_ctx *);
/* How many blocks of this model a single launch keeps resident on this ctx (the smaller of what
 * the CUs' LDS/wave slots hold and what the state budget holds); a larger batch is worked off by
 * the resident groups in turn.  Where the encoder and the decoder of a model hold different numbers
 * (general models: a wave per component either way, different register budgets) the smaller one is
 * reported: a batch of this size is one round in both directions.  flags as for the batch calls
 * (kernel choice).  < 0 = ZPQ_E_*. */
int zpq_ctx_resident_capacity(zpq_ctx *, const zpq_model *, uint32_t flags);
/* Time of the last batch's coding kernel alone, from HIP events on the ctx stream (ms). */
float zpq_ctx_last_kernel_ms(const zpq_ctx *);
const char *zpq_ctx_last_kernel_name(const zpq_ctx *);

/*
 * Batch of independent ZPAQ blocks, one segment per block, a FRESH
 * Predictor/ZPAQL per block (compressor.v:90,147-148,184-185).  Replaces, per
 * block b, the loop
 *     enc := Encoder.new(); pr.reset()                compressor.v:238-245
 *     [enc.compress(0)]  if ZPQ_FLAG_PP               compressor.v:271-274
 *     for ch in in[in_off[b] .. in_off[b+1]): enc.compress(ch)   compressor.v:277-290, encoder.v:93-120
 *     enc.compress(-1); enc.flush()                   compressor.v:375-378, encoder.v:130-139
 * and writes exactly the bytes the Encoder would have put() to
 * out[out_off[b] ...], at most out_off[b+1]-out_off[b] of them; out_len[b] =
 * byte count.  status[b] = ZPQ_OK / ZPQ_E_OVERFLOW / ZPQ_E_VMSTEPS.
 * Host-pointer form: copies in/out over PCIe around the kernel.
 * The window contract: in_off[] / out_off[] are windows into the caller's buffers.
 * For any nblocks >= 1 the host-pointer forms (these two, their _multi forms,
 * zpq_sha1_blocks, zpq_blockset_*_segments) read only in[in_off[0] .. in_off[nblocks])
 * and write only inside out[out_off[0] .. out_off[nblocks]).  Neither first offset
 * need be 0, and an offset beyond 2^32 is an offset like any other: the one bound is
 * on a single slab, out_off[b+1] - out_off[b] <= 4 GiB - 16 (and the same for in_off).
 */
int zpq_encode_blocks(zpq_ctx *, const zpq_model *, int nblocks, const uint8_t *in,
                      const uint64_t *in_off, uint32_t flags, uint8_t *out,
                      const uint64_t *out_off, uint32_t *out_len, int32_t *status);
/*
 * Mirror: per block  pr.reset(); dec := Decoder.new(); dec.init()  decompressor.v:413-418, decoder.v:29-47
 *                    loop c := dec.decompress() until -1           decompressor.v:470,485, decoder.v:122-145
 * out_len[b] = decoded bytes stored; consumed[b] = bytes the Decoder pulled from
 * its Reader (clipped to the segment length) so the caller can run
 * Decoder.skip() (decoder.v:151-196) from there; final_code[b] = Decoder.code at
 * EOF (skip() starts from it); first_byte[b] = the PP byte when ZPQ_FLAG_PP
 * (else 0xFFFFFFFF).  consumed/final_code/first_byte may be NULL.
 * The input window may be longer than the stream (junk behind it: consumed stays at the stream's end) or shorter (a
 * stream without its tail): bytes at or past in_off[b+1] read as 0, the way the reference's Decoder shifts in nothing
 * when its Reader returns -1 (decoder.v:57-62), whatever lies behind the block in `in`.
 * A slab too small: with cap = out_off[b+1] - out_off[b], a decoder stops right after it has decoded byte cap + 1 (the
 * PP byte of ZPQ_FLAG_PP not counted); out_len[b] is then cap + 1 and status[b] ZPQ_E_OVERFLOW, consumed[b] and
 * final_code[b] are those of that point, and the cap bytes in the slab are the decoded prefix.  A stream that ends with
 * byte cap is ZPQ_OK.  The encoders keep counting instead: out_len[b] is the full coded length, the slab holds its first
 * cap bytes.  The device-pointer forms write no byte from min(out_len[b], cap) on, in either direction.
 */
int zpq_decode_blocks(zpq_ctx *, const zpq_model *, int nblocks, const uint8_t *in,
                      const uint64_t *in_off, uint32_t flags, uint8_t *out,
                      const uint64_t *out_off, uint32_t *out_len, uint32_t *consumed,
                      uint32_t *final_code, uint32_t *first_byte, int32_t *status);

/*
 * Host-pointer batches are worked off in rounds of at most the resident capacity; the upload of round
 * r+1 and the download of round r-1 run beside the coding of round r (three streams).  Buffers from
 * zpq_host_alloc (pinned, device-visible) make the transfers plain DMA and let the GPU pack each block's
 * produced bytes straight into the caller's slab -- only bytes that exist cross PCIe.  Pageable buffers
 * work too (staged copies by the runtime, whole slabs come back).  One slab may be at most 4 GiB - 16.
 * A decoder's batch of 64 or more equal pinned slabs of at least 16 KiB MAY leave in two stripes (it does for a
 * dense short chain model coded in a single round; bit 1 of zpq_ctx_last_host_transfer says so): the first
 * E = (3/4 of the slab, rounded down to 256) bytes of EVERY slab are then copied beside the running kernel, whatever
 * the block produced.  Bytes in [out_len[b], E) of such a slab are unspecified; bytes from max(out_len[b], E) on are
 * not written.
 */
void *zpq_host_alloc(size_t bytes);
void zpq_host_free(void *);

/*
 * The same batch dealt over several contexts (one per GPU; several on one GPU also work): context g
 * codes the g-th contiguous share of the blocks on its own host thread.  Replaces the reference's
 * single-threaded loop over files (cmd/main.v:283-311; its -threads option is parsed and dropped,
 * cmd/main.v:35,97,156).  Blocks are independent, so the result is bit-identical for any nctx.
 */
int zpq_encode_blocks_multi(zpq_ctx *const *ctxs, int nctx, const zpq_model *, int nblocks, const uint8_t *in,
                            const uint64_t *in_off, uint32_t flags, uint8_t *out, const uint64_t *out_off,
                            uint32_t *out_len, int32_t *status);
int zpq_decode_blocks_multi(zpq_ctx *const *ctxs, int nctx, const zpq_model *, int nblocks, const uint8_t *in,
                            const uint64_t *in_off, uint32_t flags, uint8_t *out, const uint64_t *out_off,
                            uint32_t *out_len, uint32_t *consumed, uint32_t *final_code, uint32_t *first_byte,
                            int32_t *status);

/* Same, but every pointer is a DEVICE pointer and the call only enqueues work on
 * the ctx stream (no host sync, no PCIe).  This is the form bench.py times.
 * Ordering contract: the ctx stream is created hipStreamNonBlocking, so it does NOT
 * synchronise with the legacy default stream (or with torch's current stream).  The caller
 * must make sure the producers of in/in_off/out_off have finished (device or stream
 * synchronize, or an event the ctx stream waits on) before calling, and must zpq_ctx_sync()
 * (or wait on zpq_ctx_stream()) before consuming the results on another stream.
 * Threading contract: the host-pointer entry points (zpq_encode_blocks, zpq_decode_blocks,
 * zpq_sha1_blocks, zpq_block_*, zpq_blockset_*, and zpq_*_blocks_multi on each ctx it is
 * given) serialise on a per-ctx mutex and may be called from several threads; the _dev
 * forms take no lock -- one thread per ctx at a time (they share the ctx's slot pool and
 * stream), which is how the one-thread-per-device design of SURVEY 8(e) uses them. */
int zpq_encode_blocks_dev(zpq_ctx *, const zpq_model *, int nblocks, const uint8_t *in,
                          const uint64_t *in_off, uint32_t flags, uint8_t *out,
                          const uint64_t *out_off, uint32_t *out_len, int32_t *status);
int zpq_decode_blocks_dev(zpq_ctx *, const zpq_model *, int nblocks, const uint8_t *in,
                          const uint64_t *in_off, uint32_t flags, uint8_t *out,
                          const uint64_t *out_off, uint32_t *out_len, uint32_t *consumed,
                          uint32_t *final_code, uint32_t *first_byte, int32_t *status);

/*
 * Compaction of capacity-strided output slabs: dst[dst_off[b] ..] = src[src_off[b] .. + len[b]).
 * Device pointers, enqueue only.  Lets a front end download exactly the coded bytes that
 * Writer.put() would have received (encoder.v:76-83) instead of whole slabs.
 */
int zpq_gather_dev(zpq_ctx *, int nblocks, const uint8_t *src, const uint64_t *src_off, const uint32_t *len,
                   uint8_t *dst, const uint64_t *dst_off);

/*
 * SHA-1 of nblocks independent byte ranges in[in_off[b] .. in_off[b+1]) -> out20[20*b ..]:
 * the digest Compressor/Decompresser accumulate with sha1.put() per uncompressed byte
 * (compressor.v:284, decompressor.v:493,505; sha1.v:6-146) and store behind marker 253 in the
 * segment trailer (compressor.v:389-395).  One message per GPU lane, so it pays for batches
 * (hundreds of ranges); a front end handling a single large segment should hash on the host.
 * _dev: device pointers, enqueue only on the ctx stream.  zpq_sha1_ranges_dev takes explicit
 * [begin[b], end[b]) pairs (decoded blocks sit in capacity-strided slabs).
 */
int zpq_sha1_ranges_dev(zpq_ctx *, int nranges, const uint8_t *in, const uint64_t *begin, const uint64_t *end, uint8_t *out20);
int zpq_sha1_blocks(zpq_ctx *, int nblocks, const uint8_t *in, const uint64_t *in_off, uint8_t *out20);
int zpq_sha1_blocks_dev(zpq_ctx *, int nblocks, const uint8_t *in, const uint64_t *in_off, uint8_t *out20);

/*
 * One ZPAQ block whose model state persists across segments -- what
 * Compressor{z,pr} / Decompresser{z,pr} hold between start_block and end_block
 * (compressor.v:79-188, decompressor.v:219-346).  zpq_block_create ==
 * "z.clear(); inith(); initp(); pr = Predictor.new(); pr.init(&z)".
 * Each segment call == new coder + pr.reset() + the per-byte loop above.
 */
typedef struct zpq_block zpq_block;
int zpq_block_create(zpq_ctx *, const zpq_model *, zpq_block **out);
void zpq_block_destroy(zpq_block *);
int zpq_block_encode_segment(zpq_block *, const uint8_t *in, size_t n, uint32_t flags,
                             uint8_t *out, size_t cap, size_t *out_len);
int zpq_block_decode_segment(zpq_block *, const uint8_t *in, size_t n, uint32_t flags,
                             uint8_t *out, size_t cap, size_t *out_len, size_t *consumed,
                             uint32_t *final_code, uint32_t *first_byte);

/*
 * A SET of such blocks, coded a segment of each per call: what a front end that puts several segments into every block
 * needs (the reference's extractor loops find_filename inside each block, cmd/main.v:349-380; a writer may put several
 * files into one block the same way).  Per member a call is exactly zpq_block_{encode,decode}_segment -- model tables,
 * z.h, z.m and the VM registers carry over from the member's previous segment, the coder and c8 / hmap4 / h[] start
 * again (compressor.v:238-245, decompressor.v:413-418, predictor.v:827-833) -- but all listed members go through ONE
 * launch, their state handed from launch to launch through the set's own state slots.
 *   zpq_blockset_create   nmembers x "z.clear(); inith(); initp(); pr.init(&z)" (compressor.v:147-185).  max_member_bytes is
 *                         the promise for a member's bytes over ALL its segments: it sizes the compact line store the way
 *                         zpq_ctx_set_max_block_bytes does for a block (lines accumulate across segments); 0 = the ctx's
 *                         setting.  The slots count against the ctx's state budget: ZPQ_E_NOMEM if the set does not fit.
 *   zpq_blockset_capacity members one set of this model may hold on this ctx (< 0 = ZPQ_E_*).
 *   zpq_blockset_{encode,decode}_segments   one segment for each of the n listed members.  member[] = n distinct indices in
 *                         any order (NULL = 0 .. n-1); the other arguments as for zpq_encode_blocks / zpq_decode_blocks,
 *                         entry i belonging to member[i].  Host pointers, synchronous on the ctx stream.
 * A member whose segment ends with a status other than ZPQ_OK (ZPQ_E_OVERFLOW, ZPQ_E_TOOBIG, ZPQ_E_VMSTEPS) has FAILED:
 * later calls report that status for it without coding (out_len, consumed and final_code 0, first_byte 0xFFFFFFFF), the other
 * members are untouched.  ZPQ_FLAG_NOEOF: ZPQ_E_ARG.
 * The rest of a slab: a call in which every listed member is live copies the whole of out[out_off[0] .. out_off[n]) back, as
 * the batch calls do for pageable buffers -- the bytes of a slab from min(out_len[i], cap) on are unspecified, nothing at or
 * past out_off[n] is written.  A call in which a listed member has failed before copies only the stored bytes of each live
 * member, min(out_len[i], cap) of them: every other byte of `out`, the failed members' slabs included, stays as it was.
 * Lifetime as for zpq_block: the ctx orphans its sets (calls then return ZPQ_E_CLOSED), a set keeps its model alive.
 *
 * Models no chain kernel takes are coded by the lane-0 kernel, ONE LAUNCH PER MEMBER.  zpq_blockset_create_ex /
 * zpq_blockset_capacity_ex take flags (unknown bits: ZPQ_E_ARG); the plain forms are the _ex forms with flags = 0.
 *   ZPQ_SET_LANES         a request: code such a model on the lane-per-component kernels (k_rows / k_lanes, a state
 *                         hand-over form of each), one launch per round whatever the number of members.  Honoured when
 *                         zpq_blockset_lanes_applies(model): no chain kernel takes it and it has at most 64 components.
 *                         Otherwise it decides nothing.  The capacity of such a set is bounded by memory alone.  It keeps
 *                         p[], the last bit's predictions, across segments as the reference does (a component whose
 *                         input index is not below its own reads them at a segment's first bit), and so does the lane-0
 *                         kernel: the same bytes on either route.  ZPQ_SET_LANES=1 in the environment makes the request for every set the
 *                         process creates, ZPQ_SET_LANES=0 withdraws it (anything but a leading 0 / 1 decides nothing).
 *   ZPQ_SET_PIPE          a request: run the ENCODE calls of a chain-model set on the wave-pipelined encoder (k_pipe, a state
 *                         hand-over form of it) instead of the lane-per-component one (k_chain).  Honoured when
 *                         zpq_blockset_pipe_applies(model): a chain model of one of the five shapes that encoder codes (an
 *                         ICM and 1, 2 or 4 ISSEs, or 5 or 7 ISSEs and a MIX2, with the shipped context programs: levels
 *                         1-5).  Otherwise it decides nothing.  The choice is made per call, as both encoders keep the same
 *                         state in the set's slots: a call with fewer than 12 live members, or under ZPQ_ENC_PIPE=0, runs
 *                         on the chain encoder, the next one may run on the pipeline again.  Decode calls and the set's
 *                         capacity are those of the chain kernel.  The coded bytes are identical either way;
 *                         zpq_ctx_last_kernel_name tells which ran ("k_pipe<encode>" / "k_chain<encode>").  The value is
 *                         4: bit 1 is not a flag and stays refused.  ZPQ_SET_PIPE=1 in the environment makes the request
 *                         for every set the process creates, ZPQ_SET_PIPE=0 withdraws it (same rule as ZPQ_SET_LANES).
 *                         The two requests are resolved independently; no model can have both.
 *   ZPQ_SET_WAVES         a request on top of ZPQ_SET_LANES: run the calls of such a set on the wave-per-component kernels
 *                         (k_gpipe / k_gdec's state hand-over forms, k_wset / k_wsetd: a wave is a component, a lane a
 *                         member).  Honoured where ZPQ_SET_LANES is in force for the set (flag or environment, and honoured)
 *                         and zpq_blockset_waves_applies(model): the lanes predicate, and the model is one both wave kernels
 *                         take -- every input an earlier component, a MIX of at most 8 inputs, the shipped hash chain as
 *                         HCOMP, the rings and the decoder's LDS within 160 KiB (its shape alone; ZPQ_ENC_GPIPE /
 *                         ZPQ_DEC_GPIPE do not enter it).  Otherwise it decides nothing: alone on a general model it resolves
 *                         to 0, on a chain model to what the other bits give.  A honoured set reports ZPQ_SET_LANES |
 *                         ZPQ_SET_WAVES (17).  The choice is made per call, the slots hold one format for both families: an
 *                         encode call under ZPQ_ENC_GPIPE=0, a decode call under ZPQ_DEC_GPIPE=0 (read at the call) runs on
 *                         k_rows / k_lanes as without the request (ZPQ_LANES_ROWS chooses between those), the next call may
 *                         run on the wave kernels again.  No floor on the number of members.  ZPQ_GPIPE_BATCH=0 selects the
 *                         bit-serial encoder stages as for plain batches; ZPQ_GDEC_BPW is ignored (always 64 lanes per
 *                         workgroup).  Same coded bytes whichever kernel ran; zpq_ctx_last_kernel_name tells which
 *                         ("k_wset<encode>" / "k_wsetd<decode>").  The capacity stays that of ZPQ_SET_LANES: memory alone.
 *                         ZPQ_SET_WAVES=1 / =0 in the environment by the rule of ZPQ_SET_LANES, resolved on its own and then
 *                         combined: a process that wants it from the environment sets both variables.
 *   ZPQ_SET_VMWAVES       the same request for a model whose HCOMP program is NOT the shipped hash chain: run the calls of the
 *                         set on the state hand-over forms of k_vpipe / k_vdec (k_vset / k_vsetd: a wave per component, one
 *                         for the coder and one that runs the ZPAQL interpreter, a lane per member).  Honoured where
 *                         ZPQ_SET_LANES is in force for the set (flag or environment, and honoured) and
 *                         zpq_blockset_vmwaves_applies(model): the lanes predicate, and the model is in the envelope of
 *                         ZPQ_FLAG_VMPIPE -- not the hash chain, at most 14 components, every input an earlier component, a
 *                         MIX of 1-8 inputs, both directions' LDS (rings, contexts, header) within 160 KiB; its shape alone,
 *                         no environment variable and no batch size enter it.  Otherwise it decides nothing.  A honoured set
 *                         reports ZPQ_SET_LANES | ZPQ_SET_VMWAVES (65).  No model can have both this and ZPQ_SET_WAVES (the
 *                         HCOMP program decides): a caller who wants the wave kernels wherever they apply passes
 *                         ZPQ_SET_LANES | ZPQ_SET_WAVES | ZPQ_SET_VMWAVES (81), which resolves to 17 or to 65.  Everything
 *                         else is as for ZPQ_SET_WAVES: the choice per call (an encode call under ZPQ_ENC_GPIPE=0, a decode
 *                         call under ZPQ_DEC_GPIPE=0 runs on k_rows / k_lanes, the slots hold one format), no floor on the
 *                         number of members, ZPQ_GPIPE_BATCH=0, ZPQ_GDEC_BPW ignored, the same coded bytes, ZPQ_E_VMSTEPS
 *                         ahead of ZPQ_E_OVERFLOW as in plain batches, the capacity of ZPQ_SET_LANES, and the names
 *                         "k_vset<encode>" / "k_vsetd<decode>".  ZPQ_SET_VMWAVES=1 / =0 in the environment by the rule of
 *                         ZPQ_SET_LANES, resolved on its own and then combined.
 *                         Whether the request pays depends on the PROGRAM, not on the number of members (measured at 16, 512
 *                         and 4096 members, 4 KiB segments, tools/set_vmwaves_bench.py): behind a program as light as the hash
 *                         chain (C4b's components, `a=a` in front of it) a round takes 2.3-2.8x less kernel time to encode
 *                         and 1.35-1.55x less to decode than on k_rows, from 16 members on; behind a program that loops
 *                         1-16 times per byte (zpaql_programs "loop_count") it LOSES at every member count measured, 16
 *                         included (encode 7-37 %, decode 16-51 % slower): one wave runs the 64 members' interpreters in
 *                         lockstep, k_rows one interpreter per row of lanes.  Leave such sets on ZPQ_SET_LANES alone.
 *   ZPQ_SET_CHUNKS        a request on top of ZPQ_SET_LANES: let zpq_blockset_{encode,decode}_chunks (below) code such a set, on
 *                         k_rows / k_lanes -- without it they return ZPQ_E_ARG for a ZPQ_SET_LANES set, as they always have.
 *                         Honoured where ZPQ_SET_LANES is in force for the set (flag or environment, and honoured); anywhere
 *                         else it decides nothing: a chain-model set or a plain set resolves as without it and chunks as
 *                         without it.  A honoured set reports 129, 145 (| ZPQ_SET_WAVES) or 193 (| ZPQ_SET_VMWAVES).  It has no
 *                         environment variable -- nothing in a process but a caller of the chunk calls can use it -- and
 *                         changes neither the capacity nor the whole-segment calls of the set.  The value is 128.
 *   zpq_blockset_flags    the ZPQ_SET_* in force for a set (0 for a request that decided nothing).  Like every call on a
 *                         set it must not race with zpq_blockset_destroy of the same handle.
 *   zpq_blockset_lanes_applies / _pipe_applies / _waves_applies / _vmwaves_applies / zpq_blockset_resolve_flags   host logic only, no device
 *                         needed: would the request be honoured for this model (its shape alone, neither a batch size nor
 *                         the environment); the flags a set created with `flags` would get (environment applied).
 */
#define ZPQ_SET_LANES 1u
#define ZPQ_SET_PIPE 4u
#define ZPQ_SET_WAVES 16u
#define ZPQ_SET_VMWAVES 64u
#define ZPQ_SET_CHUNKS 128u
typedef struct zpq_blockset zpq_blockset;
int zpq_blockset_create(zpq_ctx *, const zpq_model *, int nmembers, uint64_t max_member_bytes, zpq_blockset **out);
int zpq_blockset_create_ex(zpq_ctx *, const zpq_model *, int nmembers, uint64_t max_member_bytes, uint32_t flags, zpq_blockset **out);
void zpq_blockset_destroy(zpq_blockset *);
int zpq_blockset_capacity(zpq_ctx *, const zpq_model *, uint64_t max_member_bytes);
int zpq_blockset_capacity_ex(zpq_ctx *, const zpq_model *, uint64_t max_member_bytes, uint32_t flags);
unsigned zpq_blockset_flags(const zpq_blockset *);
int zpq_blockset_lanes_applies(const zpq_model *);
int zpq_blockset_pipe_applies(const zpq_model *);
int zpq_blockset_waves_applies(const zpq_model *);
int zpq_blockset_vmwaves_applies(const zpq_model *);
int zpq_blockset_resolve_flags(const zpq_model *, uint32_t flags);
int zpq_blockset_encode_segments(zpq_blockset *, int n, const int32_t *member, const uint8_t *in, const uint64_t *in_off,
                                 uint32_t flags, uint8_t *out, const uint64_t *out_off, uint32_t *out_len, int32_t *status);
int zpq_blockset_decode_segments(zpq_blockset *, int n, const int32_t *member, const uint8_t *in, const uint64_t *in_off,
                                 uint32_t flags, uint8_t *out, const uint64_t *out_off, uint32_t *out_len, uint32_t *consumed,
                                 uint32_t *final_code, uint32_t *first_byte, int32_t *status);
/*
 * CHUNKED coding: a member's segment a piece at a time -- what Compressor.compress(n) (compressor.v:259-293) and
 * Decompresser.decompress(n) (decompressor.v:443-515) do n bytes at a time, the coder and the predictor carrying on between
 * calls.  A member is OPEN after a chunk call that left its segment unfinished; the set remembers it
 * (zpq_blockset_member_open: 1 / 0, < 0 = ZPQ_E_*), and the next chunk call on that member goes on where the last one
 * stopped -- no new coder, no Predictor.reset(), no PP byte, whatever `flags` says.  One call may mix members that start,
 * go on and end.  Arguments, windows (above, "The window contract") and the copy-back of slabs ("The rest of a slab") are
 * those of zpq_blockset_{encode,decode}_segments.
 *   encode   member i not open: a segment starts as in zpq_blockset_encode_segments (new coder, reset(), the PP byte under
 *            ZPQ_FLAG_PP).  more[i] != 0: the call stops behind the last input byte -- no compress(-1), no flush() --, stores
 *            what the Encoder has put() so far and leaves the member open; more[i] == 0 (more == NULL: all 0) ends the
 *            segment.  Zero input bytes are legal both to open a segment (the PP byte is then all that is coded) and to end
 *            one.  The bytes of a segment's chunks, one behind the other, are exactly what ONE zpq_blockset_encode_segments
 *            call writes for the whole segment; with more == NULL and no member open the call IS that call.  A slab too small
 *            for its chunk fails the member (ZPQ_E_OVERFLOW, sticky), as do ZPQ_E_TOOBIG / ZPQ_E_VMSTEPS: max_member_bytes
 *            covers all chunks of all segments.
 *   decode   a decoder PAUSES instead of overflowing: once it has stored cap = out_off[i+1] - out_off[i] bytes it stops in
 *            front of the next byte's EOF flag -- nothing more is decoded, the model is not touched -- and reports out_len[i]
 *            = cap, open[i] = 1, status[i] = ZPQ_OK, consumed[i] and final_code[i] as of that point.  (A segment that starts
 *            under ZPQ_FLAG_PP decodes the PP byte first and reports it in first_byte[i]; a call that goes on reports
 *            0xFFFFFFFF.)  The next call reads on from where the decoder stands: its window starts consumed[i] bytes behind
 *            the previous window's start; consumed[] counts per call.  Reaching the EOF symbol closes the member, open[i] = 0;
 *            a stream that ends exactly with a full slab takes one more call (out_len 0, open 0) to find that out, and so cap
 *            = 0 decodes nothing.  ZPQ_E_OVERFLOW is never reported.  open[] (n entries) is required.  A window that ends
 *            before the chunk's data does reads zeros past its end, as in zpq_decode_blocks: enough input for the bytes a
 *            call is to decode is the CALLER'S duty (a decoder runs four bytes, its code register, ahead of the bits it has
 *            decoded; passing the whole rest of the stream is the simple choice).
 * An open member listed in zpq_blockset_{encode,decode}_segments, or in a chunk call of the other direction, makes the call
 * return ZPQ_E_ARG with nothing coded; ZPQ_FLAG_NOEOF stays ZPQ_E_ARG; a failed member is never open.
 * Kernels: chain models on k_chain<..., KEEP> in both directions -- on a ZPQ_SET_PIPE set too, every encode_chunks call runs on
 * "k_chain<encode>" (same slot format, as for that flag's per-call choice) --, every other model on the lane-0 kernel, a launch
 * per member.  A set on which ZPQ_SET_LANES is in force returns ZPQ_E_ARG from both chunk calls (flags 1, 17, 65) unless it was
 * created with ZPQ_SET_CHUNKS (129, 145, 193): then every chunk call is ONE launch of k_rows / k_lanes<..., KEEP>
 * ("k_rows<encode>" ..., ZPQ_LANES_ROWS choosing between the two per call: they read each other's pauses), on a 145 or 193 set
 * too -- its chunk calls never run on k_wset / k_vset, as a ZPQ_SET_PIPE set's never run on k_pipe, while its whole-segment
 * calls go on choosing per call (one slot format).  Measured on C4b (profiles/r22_set_lanes_chunks.txt): a chunk call of 256 bytes
 * takes 42x (16 members) to 630x (256 members) less wall-clock time than on a plain set's lane-0 kernel, 16 chunk calls cost 1.00-1.01x
 * the kernel time of one call, and a set that never chunks pays nothing for the pause.  Carrying the pause to k_wset / k_wsetd / k_vset / k_vsetd and to KEEP forms on the
 * line store is later work, as are zpq_block_* and the archive layer / front end (which still re-decode with a larger slab).
 */
int zpq_blockset_encode_chunks(zpq_blockset *, int n, const int32_t *member, const uint8_t *in, const uint64_t *in_off,
                               uint32_t flags, const uint8_t *more /* n entries, NULL = all 0 */,
                               uint8_t *out, const uint64_t *out_off, uint32_t *out_len, int32_t *status);
int zpq_blockset_decode_chunks(zpq_blockset *, int n, const int32_t *member, const uint8_t *in, const uint64_t *in_off,
                               uint32_t flags, uint8_t *out, const uint64_t *out_off, uint32_t *out_len,
                               uint32_t *consumed, uint32_t *final_code, uint32_t *first_byte,
                               uint8_t *open /* n entries, out, required */, int32_t *status);
int zpq_blockset_member_open(const zpq_blockset *, int member);   /* 1 = its segment is open, 0 = not, < 0 = ZPQ_E_* */

/* ---- inspection / test hooks ---- */
/* squash_table / stretch_table as built at start-up (predictor.v:11-15,21-96). */
int zpq_tables(int32_t *squash4096, int32_t *stretch32768);
/* dt_table (predictor.v:111-166), dt2k (predictor.v:99-106), StateTable.ns (statetable.v:15-57); any pointer may be NULL. */
int zpq_tables_ex(int32_t *dt1024, int32_t *dt2k256, uint8_t *ns1024);
/* Run the device ZPAQL VM over `in` on a fresh block and return, for every input
 * byte, the n context hashes Predictor.update copies out (predictor.v:809-816):
 * h_out[i*ncomp + k].  Exercises zpaql.v:167-954 alone. */
int zpq_debug_contexts(zpq_ctx *, const zpq_model *, const uint8_t *in, size_t n, uint32_t *h_out);
/* The pool's dirty-line logs (ZPQ_DIRTY_LOG_CAP, default 16384 entries per table, 0 = off): the dense level-2 kernels
 * note which 64-byte table lines a launch made non-zero, and the next launch of theirs on the pool zeroes those lines
 * instead of every slot.  This hook applies that clear to the pool's first nslots slots and counts the non-zero 16-byte
 * words left in the part of them a launch expects zeroed: 0 when the logs name every dirty line.  ZPQ_E_ARG unless the
 * last launches on the pool left valid logs for at least nslots slots. */
int zpq_debug_pool_residue(zpq_ctx *, int nslots, uint64_t *count);
/* The logs' counts as the last launch left them: counts[3 * slot + table] for the pool's first nslots slots (a count equal
 * to the capacity = the log overflowed).  A copy and nothing else: no kernel, nothing cleared.  ZPQ_E_ARG as above. */
int zpq_debug_dlog_counts(zpq_ctx *, int nslots, uint32_t *counts /* nslots * 3 */);
/* Encode one fresh block with the generic kernel and record predict()'s return
 * value for the first ntrace modelled bits (predictor.v:536-668). */
int zpq_debug_encode_trace(zpq_ctx *, const zpq_model *, const uint8_t *in, size_t n,
                           uint32_t flags, uint8_t *out, size_t cap, size_t *out_len,
                           int32_t *p_trace, size_t ntrace);
const char *zpq_status_string(int code);
const char *zpq_version(void);

#ifdef __cplusplus
}
#endif
#endif
