// Scans and reductions over a wavefront (wave64) and over a workgroup: the one place for them.  Every kernel header takes its sums,
// minima, maxima and prefix scans from here; a __shfl_up / __shfl_xor elsewhere fetches a neighbour's value and nothing more.
//   tk_wave_min_u32 / _min_u64 / _max_u32 / _max_u64 / _sum_u32   the reduction, in every lane
//   tk_wave_scan_u32                                               inclusive prefix sum over the wavefront
//   tk_block_exscan_256 / tk_block_exmax32_256 / tk_block_exmax64_256   exclusive scan over a workgroup of 256 threads
//   tk_block_sum_256                                               sum over a workgroup of 256 threads
//   tk_scan1024 / tk_scan_blocks                                   the one workgroup of 1024 threads that scans per-workgroup values
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint32_t tk_wave_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        uint32_t w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ uint64_t tk_wave_min_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        uint64_t w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t tk_wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long tk_wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t tk_wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// inclusive prefix sum across the wave
// inclusive prefix sum over the wavefront: four DPP row shifts inside the rows of sixteen lanes, then the last lane of a row to the rows
// behind it (row_bcast:15 to rows 1 and 3, row_bcast:31 to rows 2 and 3) -- six full-rate instructions (round 4: six __shfl_up, each a
// ds_bpermute through the LDS crossbar plus a compare and a select)
// (row_bcast:15 / row_bcast:31 are DPP controls of the GFX9 / CDNA encodings only -- the library is built for gfx950; a wave64 target without
// them takes the shuffle form by itself instead of failing in the assembler)
#if !defined(TK_SCAN_SHFL) && defined(__HIP_DEVICE_COMPILE__) && !defined(__GFX9__)
#define TK_SCAN_SHFL 1
#endif
#ifndef TK_SCAN_SHFL
__device__ __forceinline__ uint32_t tk_wave_scan_u32(uint32_t v, int /*lane*/) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);   // row_shr:1 (a lane without a source adds nothing)
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
    return v;
}
#else
__device__ __forceinline__ uint32_t tk_wave_scan_u32(uint32_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        uint32_t w = __shfl_up(v, o, 64);
        if (lane >= o) v += w;
    }
    return v;
}
#endif
// block-wide (256 threads) exclusive scan; returns the exclusive prefix, *total gets the block sum
__device__ __forceinline__ uint32_t tk_block_exscan_256(uint32_t v, uint32_t* total, uint32_t* sh /*[8]*/) {
    int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t inc = tk_wave_scan_u32(v, lane);
    if (lane == 63) sh[wid] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        uint32_t s = sh[w];
        if (w < wid) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}
// sum over the 256 threads of a workgroup, 64-bit, in every thread (sh is the caller's again after the workgroup's next barrier)
__device__ __forceinline__ unsigned long long tk_block_sum_256(uint32_t v, uint32_t* sh /*[4]*/) {
    v = tk_wave_sum_u32(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (unsigned long long)sh[0] + sh[1] + sh[2] + sh[3];
}

__device__ __forceinline__ unsigned long long tk_max64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
// exclusive max-scan over the 256 threads of a workgroup (0 = nothing before); *total = the workgroup's maximum
__device__ __forceinline__ unsigned long long tk_block_exmax64_256(unsigned long long v, unsigned long long* total, unsigned long long* sh /*[4]*/) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long w = __shfl_up(inc, o, 64);
        if (lane >= o) inc = tk_max64(inc, w);
    }
    const unsigned long long before = __shfl_up(inc, 1, 64);
    if (lane == 63) sh[wid] = inc;
    __syncthreads();
    unsigned long long base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const unsigned long long s = sh[w];
        if (w < wid) base = tk_max64(base, s);
        tot = tk_max64(tot, s);
    }
    __syncthreads();
    *total = tot;
    return lane ? tk_max64(base, before) : base;
}
// ... its 32-bit sibling
__device__ __forceinline__ uint32_t tk_block_exmax32_256(uint32_t v, uint32_t* total, uint32_t* sh /*[4]*/) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t w = __shfl_up(inc, o, 64);
        if (lane >= o) inc = max(inc, w);
    }
    const uint32_t before = __shfl_up(inc, 1, 64);
    if (lane == 63) sh[wid] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t s = sh[w];
        if (w < wid) base = max(base, s);
        tot = max(tot, s);
    }
    __syncthreads();
    *total = tot;
    return lane ? max(base, before) : base;
}

// exclusive scan over the 1024 threads of the one workgroup: sums, or maxima with 0 = nothing
template <bool MAX>
__device__ __forceinline__ unsigned long long tk_scan1024(unsigned long long v, unsigned long long* total, unsigned long long* wsum /*[16]*/) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long w = __shfl_up(inc, o, 64);
        if (lane >= o) inc = MAX ? tk_max64(inc, w) : inc + w;
    }
    const unsigned long long before = __shfl_up(inc, 1, 64);
    if (lane == 63) wsum[wid] = inc;
    __syncthreads();
    unsigned long long base = 0, tot = 0;
    for (int w = 0; w < 16; ++w) {
        const unsigned long long s = wsum[w];
        if (w < wid) base = MAX ? tk_max64(base, s) : base + s;
        tot = MAX ? tk_max64(tot, s) : tot + s;
    }
    __syncthreads();
    *total = tot;
    if (!lane) return base;
    return MAX ? tk_max64(base, before) : base + before;
}
// The one workgroup of 1024 threads over the values of nb workgroups, in place: a[i] -> `carry` combined with everything before a[i] (sums,
// or maxima with 0 = nothing), 1024 values at a time.  Returns, in every thread, the carry behind a[nb - 1].
template <bool MAX, class T>
__device__ __forceinline__ unsigned long long tk_scan_blocks(T* __restrict__ a, uint64_t nb, unsigned long long carry, unsigned long long* wsum /*[16]*/) {
    for (uint64_t base = 0; base < nb; base += 1024) {
        const uint64_t i = base + threadIdx.x;
        unsigned long long tot;
        const unsigned long long ex = tk_scan1024<MAX>(i < nb ? (unsigned long long)a[i] : 0ull, &tot, wsum);
        if (i < nb) a[i] = (T)(MAX ? tk_max64(carry, ex) : carry + ex);
        carry = MAX ? tk_max64(carry, tot) : carry + tot;
    }
    return carry;
}
