// Micro-benchmark: zeroing N random 64-byte lines per 4-MiB table from a u32 list of their offsets -- the dirty-line log's
// clear (zpq_dev.h, dlog_zero_lines: the kernels' own code) -- against streaming zeroes over the whole table, which is what
// the level-2 kernels' slot clear did for every table.  The footprint is FOOT_GIB of tables (default 96, the level-2 pool of
// 8192 slots); a workgroup owns its share of them as a workgroup of k_pipe owns its slots' tables.  Two shapes of the
// scattered clear: a WAVE per table (k_pipe, 256 threads) and EIGHT LANES per table (k_chain<decode>: a block's group of
// lanes clears its own slot, 32 groups per workgroup).  Dirty fractions 1/64 .. 1/2 of a table's 65536 lines.
// Reported per fraction: ms for the scattered clear in both shapes, ms for streaming, lines per second, and the ratio.
//   hipcc --offload-arch=gfx950 -O3 -o tools/micro/bin/lineclear tools/micro/lineclear.hip && tools/micro/bin/lineclear [FOOT_GIB]
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../zpaq-v_amd/csrc/zpq_dev.h"

using namespace zpqdev;

constexpr unsigned TABLE = 4u << 20, TLINES = TABLE / 64;

// the lists: n pseudo-random line offsets per table (duplicates as they fall, as in a log)
__global__ void k_lists(uint32_t *lists, unsigned long long stride, unsigned n, unsigned ntab)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (unsigned long long)n * ntab) return;
    const unsigned t = (unsigned)(i / n), k = (unsigned)(i % n);
    unsigned long long r = (i + 1) * 0x9E3779B97F4A7C15ull;
    r ^= r >> 29; r *= 0xBF58476D1CE4E5B9ull; r ^= r >> 32;
    lists[t * stride + DLOG_HDR + k] = (uint32_t)(r % TLINES) * 64u;
    if (k == 0) lists[t * stride] = n;
}
// a wave per table, the workgroup's tables in turn (k_pipe's clear phase)
__global__ void __launch_bounds__(256) k_clear_wave(uint8_t *tabs, const uint32_t *lists, unsigned long long stride, unsigned ntab)
{
    const unsigned per = (ntab + gridDim.x - 1) / gridDim.x, t0 = blockIdx.x * per, t1 = min(t0 + per, ntab);
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (unsigned t = t0 + wave; t < t1; t += 4) {
        const uint32_t *lg = lists + t * stride;
        dlog_zero_lines(tabs + (unsigned long long)t * TABLE, TABLE, lg, lg[0], lane, 64);
    }
}
// eight lanes per table: a workgroup's 32 groups work on 32 tables side by side (k_chain<decode>'s clear)
__global__ void __launch_bounds__(256) k_clear_group(uint8_t *tabs, const uint32_t *lists, unsigned long long stride, unsigned ntab)
{
    const unsigned per = (ntab + gridDim.x - 1) / gridDim.x, t0 = blockIdx.x * per, t1 = min(t0 + per, ntab);
    const unsigned grp = threadIdx.x >> 3, li = threadIdx.x & 7;
    for (unsigned t = t0 + grp; t < t1; t += 32) {
        const uint32_t *lg = lists + t * stride;
        dlog_zero_lines(tabs + (unsigned long long)t * TABLE, TABLE, lg, lg[0], li, 8);
    }
}
// streaming: the whole workgroup over each of its tables (the slot clear as it was)
__global__ void __launch_bounds__(256) k_stream(uint8_t *tabs, unsigned ntab)
{
    const unsigned per = (ntab + gridDim.x - 1) / gridDim.x, t0 = blockIdx.x * per, t1 = min(t0 + per, ntab);
    const uint4 zero = make_uint4(0, 0, 0, 0);
    for (unsigned t = t0; t < t1; t++) {
        uint4 *z4 = reinterpret_cast<uint4 *>(tabs + (unsigned long long)t * TABLE);
        for (unsigned i = threadIdx.x; i < TABLE / 16; i += 256) z4[i] = zero;
    }
}

int main(int argc, char **argv)
{
    const unsigned long long gib = argc > 1 ? strtoull(argv[1], 0, 0) : 96;
    const unsigned ntab = (unsigned)((gib << 30) / TABLE);
    const unsigned nmax = TLINES / 2;
    const unsigned long long stride = dlog_stride(nmax);
    uint8_t *tabs; uint32_t *lists;
    if (hipMalloc((void **)&tabs, (unsigned long long)ntab * TABLE) != hipSuccess || hipMalloc((void **)&lists, (unsigned long long)ntab * stride * 4) != hipSuccess) {
        printf("alloc of %llu GiB failed\n", gib); return 1;
    }
    hipMemset(tabs, 1, (unsigned long long)ntab * TABLE);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    auto timed = [&](auto &&launch) {
        float best = 1e30f;
        for (int rep = 0; rep < 3; rep++) {
            hipEventRecord(e0); launch(); hipEventRecord(e1); hipEventSynchronize(e1);
            float ms; hipEventElapsedTime(&ms, e0, e1);
            if (ms < best) best = ms;
        }
        return best;
    };
    const int grid = 256;
    const float ms_stream = timed([&] { hipLaunchKernelGGL(k_stream, dim3(grid), dim3(256), 0, 0, tabs, ntab); });
    printf("%u tables of 4 MiB (%llu GiB), %d workgroups of 256 threads\n", ntab, gib, grid);
    printf("streaming clear of every table: %7.2f ms = %5.2f TB/s (%.3f us per table and workgroup)\n", ms_stream,
           (double)ntab * TABLE / (ms_stream * 1e-3) / 1e12, ms_stream * 1e3 / ((ntab + grid - 1) / grid));
    for (unsigned den = 64; den >= 2; den /= 2) {
        if (den == 32) continue;
        const unsigned n = TLINES / den;
        const unsigned long long total = (unsigned long long)n * ntab;
        hipLaunchKernelGGL(k_lists, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, lists, stride, n, ntab);
        const float ms_w = timed([&] { hipLaunchKernelGGL(k_clear_wave, dim3(grid), dim3(256), 0, 0, tabs, lists, stride, ntab); });
        const float ms_g = timed([&] { hipLaunchKernelGGL(k_clear_group, dim3(grid), dim3(256), 0, 0, tabs, lists, stride, ntab); });
        printf("dirty 1/%-2u (%5u lines per table): wave per table %7.2f ms = %6.2f G lines/s, %.2f of streaming | eight lanes per table %7.2f ms = %6.2f G lines/s, %.2f of streaming\n",
               den, n, ms_w, total / (ms_w * 1e-3) / 1e9, ms_w / ms_stream, ms_g, total / (ms_g * 1e-3) / 1e9, ms_g / ms_stream);
        fflush(stdout);
    }
    if (hipGetLastError() != hipSuccess) { printf("HIP error\n"); return 1; }
    return 0;
}
