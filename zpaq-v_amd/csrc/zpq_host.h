// zpq_host.h -- host-only internals of libzpaq_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <vector>

#include "zpq_common.h"

namespace zpq {

// Start-up tables exactly as the reference builds them (predictor.v:7-18).
struct Tables {
    int32_t squash[4096];
    int32_t stretch[32768];
    int32_t dt[1024];
    int32_t dt2k[256];
    uint8_t ns[1024];
    uint32_t stretch_c[2048 + 128];  // LDS-sized packing of stretch (see zpq_model.cpp)
};
const Tables &tables(int *status);
uint64_t tables_fnv(int which);

}  // namespace zpq

// Re-lay a model's state slot with a compact line store (capacity `cap` lines, a multiple of 4) for every
// ICM/ISSE hash table that is larger than the store; false if none qualifies.  The zeroed prefix of the slot
// (zero_bytes) then ends before the stores' line arrays: a line is cleared when it is claimed.
bool zpq_sparse_layout(const DModel &dense, uint32_t cap, DModel *out);

// The HCOMP shape every shipped level >= 2 uses (levels.v:126-141 and on):
//   b=c c-- *c=a d=0 (hash *d=a d++) x K  hash *d=a halt
// leaves H[k] = hash^(k+1)(byte, previous byte) for k <= K and never touches H beyond.  Returns the
// number of hashes K+1 when the model's program is exactly that (and M, H are large enough), else 0.
int zpq_vm_hashchain(const DModel *M);

struct zpq_model {
    DModel d;
    std::vector<uint32_t> img;  // initial table contents (ICM/ISSE/SSE), uploaded per ctx
    uint64_t id;                // unique, for the per-ctx device cache
    mutable std::atomic<int> refs{1};   // the creator's handle + one per zpq_block built on it: zpq_model_destroy only drops the creator's
};
void zpq_model_retain(const zpq_model *m);
void zpq_model_release(const zpq_model *m);   // deletes the model with its last reference

// ---- what the kernel files offer zpq_api.hip (and one another): each file that defines one of these includes this header,
// so that a declaration and its definition meet in one translation unit.  blocks_per_cu / blocks_per_wg: resident blocks;
// *_applies: the model (or plan) is in the kernels' envelope; zpq_launch_*: ZPQ_OK or an error code, the launch is queued.
extern "C" {
// zpq_generic.hip
void zpq_launch_generic(const DBatch *B, const DModel *hostM, int decode, int grid, hipStream_t stream);
int zpq_generic_blocks_per_cu(const DModel *M);
// zpq_chain.hip
int zpq_chain_blocks_per_wg(const DModel *M);   // 0 = model not supported by the chain kernel
int zpq_chain_max_wgs(const DModel *M, int cus);
int zpq_chain_plan(const DModel *M, int nblocks, int cus, int *blocks_per_wg);
int zpq_launch_chain(const DBatch *B, const DModel *hostM, int decode, int nwg, int blocks_per_wg, hipStream_t stream, const char **name_out);
int zpq_chain_has_hio(const DModel *M);   // kernels that take part in striped host transfers exist for this model
// zpq_pipe.hip / zpq_dpipe.hip: the wave-pipelined encoder / decoder of chain plans (zpq_launch_chain chooses them)
int zpq_pipe_shape_applies(const DModel *M);   // the chain is one of the shapes k_pipe codes
int zpq_pipe_applies(const DModel *M, int blocks_per_wg, int nslots);
int zpq_launch_pipe(const DBatch *B, const DModel *hostM, int nwg, int blocks_per_wg, hipStream_t stream, const char **name_out);
// the dirty-line log (DBatch::dlog): would the launch keep it?  (B->dlog itself is not looked at: the host asks before it offers one)
int zpq_pipe_keeps_dlog(const DBatch *B, const DModel *hostM, int blocks_per_wg);
int zpq_chain_keeps_dlog(const DBatch *B, const DModel *hostM, int decode, int blocks_per_wg);
// debug: log-clear slots [0, nslots) of a pool whose logs are valid for d_model (a chain of nt hashed tables), reset their
// counts, and count the non-zero 16-byte words left in their zero_bytes into *d_count
int zpq_launch_dlog_residue(const DBatch *B, const DModel *hostM, int nslots, unsigned long long *d_count, hipStream_t stream);
int zpq_dpipe_applies(const DModel *M, int blocks_per_wg, int nslots);
int zpq_launch_dpipe(const DBatch *B, const DModel *hostM, int nwg, int blocks_per_wg, hipStream_t stream);
// zpq_lanes.hip: lane i = component i (k_rows: four blocks per wave, k_lanes), and the KEEP forms for block sets
int zpq_lanes_supported(const DModel *M);
int zpq_lanes_blocks_per_cu(const DModel *M);
const char *zpq_lanes_kernel_name(const DModel *M, int decode);
int zpq_launch_lanes(const DBatch *B, const DModel *hostM, int decode, int nslots, hipStream_t stream);
int zpq_launch_lanes_set_init(const DModel *d_model, const uint32_t *d_img, uint8_t *slots, int nmembers, hipStream_t stream);
int zpq_launch_lanes_keep(const DBatch *B, const DModel *hostM, int decode, hipStream_t stream);
// zpq_gpipe.hip: general models as a pipeline of waves (wave = component, lane = block): the encoder, its bit-synchronous
// decoder, the same pair with an interpreter wave for any other HCOMP program (ZPQ_FLAG_VMPIPE / ZPQ_VM_PIPE), and the
// block-set forms of both pairs (ZPQ_SET_WAVES: k_wset / k_wsetd, ZPQ_SET_VMWAVES: k_vset / k_vsetd)
int zpq_gpipe_shape_applies(const DModel *M);   // the envelopes from the model's shape alone
int zpq_gdec_shape_applies(const DModel *M);
int zpq_gpipe_applies(const DModel *M);
int zpq_gpipe_blocks_per_cu(const DModel *M);
int zpq_launch_gpipe(const DBatch *B, const DModel *hostM, int nslots, hipStream_t stream);
int zpq_gdec_applies(const DModel *M);
int zpq_gdec_blocks_per_cu(const DModel *M);
int zpq_launch_gdec(const DBatch *B, const DModel *hostM, int nslots, hipStream_t stream);
int zpq_vpipe_applies(const DModel *M);
int zpq_vpipe_blocks_per_cu(const DModel *M);
int zpq_launch_vpipe(const DBatch *B, const DModel *hostM, int nslots, hipStream_t stream);
int zpq_vdec_applies(const DModel *M);
int zpq_vdec_blocks_per_cu(const DModel *M);
int zpq_launch_vdec(const DBatch *B, const DModel *hostM, int nslots, hipStream_t stream);
int zpq_launch_wset(const DBatch *B, const DModel *hostM, int decode, hipStream_t stream, const char **name);
int zpq_launch_vset(const DBatch *B, const DModel *hostM, int decode, hipStream_t stream, const char **name);
// zpq_sha1.hip
int zpq_launch_sha1(const uint8_t *in, const uint64_t *beg, const uint64_t *end, int n, uint8_t *out20, hipStream_t stream);
}

// ---- the C boundary never lets a C++ exception out (include/zpaq_hip.h: "never aborts, no exceptions").  Every
// extern "C" definition is a function-try-block:   extern "C" int f(...) try { ... } ZPQ_CATCH(return ZPQ_E_INTERNAL)
// std::bad_alloc and std::system_error can come from the containers and threads of the host code; the HIP runtime itself
// has been seen to throw (std::bad_variant_access out of a call on a stream whose owner was gone).
void zpq_note_exception(const char *where) noexcept;
#define ZPQ_CATCH(on_error) catch (...) { zpq_note_exception(__func__); on_error; }

// the same for one-line entry points:  return zpq_guard<int>(0, __func__, [&] { ... });
template <class R, class F> static inline R zpq_guard(R on_error, const char *where, F &&f) noexcept
{
    try { return f(); } catch (...) { zpq_note_exception(where); return on_error; }
}
template <class F> static inline void zpq_guard_v(const char *where, F &&f) noexcept
{
    try { f(); } catch (...) { zpq_note_exception(where); }
}
