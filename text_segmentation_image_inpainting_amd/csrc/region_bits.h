// What regions.hip (K10) and blocks.hip (K15) share: the 64 x 32 rectangle a block of 256 threads owns, its rows as 64-bit words, the
// run helpers on those words and the block scan of the table kernels.  Device helpers only: every kernel stays in its own file.
#pragma once
#include "emu_atomics.h"
#include "page_grid.h"

#include <limits.h>

namespace tsii {

constexpr int RG_W = 64, RG_H = 32, RG_PIX = RG_W * RG_H, RG_THREADS = 256, RG_PER = RG_PIX / RG_THREADS;
constexpr int RG_SCAN = 8;                       // segment counts per thread of the scan kernels
constexpr int RG_STATS = 5;                      // area, y0, x0, y1, x1 per root, at ws[root * 5]
typedef unsigned long long u64;

// parent links are read while other threads lower them: relaxed device-scope atomic accesses, never kept in a register across a loop
#ifndef __HIP_MEMORY_SCOPE_AGENT
#define __HIP_MEMORY_SCOPE_AGENT 4
#endif
__device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ u64 bit_span(int first, int len) { return (len >= 64 ? ~0ull : ((1ull << len) - 1ull)) << first; }
// first column of the run of set bits that contains column c
__device__ __forceinline__ int run_start(u64 bits, int c) {
    const u64 z = ~bits & ((1ull << c) - 1ull);
    return z ? 64 - __builtin_clzll(z) : 0;
}
// number of set bits from column c on (bit c is set)
__device__ __forceinline__ int run_len(u64 bits, int c) {
    const u64 v = ~(bits >> c);
    return v ? __builtin_ctzll(v) : 64;
}
// 64 bytes of 0 / 1 per row -> one word per row (8 bytes -> 8 bits with one multiply, as the K8 mask kernel does)
__device__ __forceinline__ void pack_rows(const u64 (*bytes)[8], u64* bits, int tid) {
    if (tid < RG_H) {
        u64 v = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) v |= ((bytes[tid][k] * 0x0102040810204080ull) >> 56) << (8 * k);
        bits[tid] = v;
    }
}

// thread tid owns column tid & 63 of rows (tid >> 6) + 4 k, k = 0..7: a wave reads 64 consecutive pixels of one row
#define RG_FOR_PIXELS(k, r, c) \
    const int c = tid & 63;    \
    _Pragma("unroll") for (int k = 0, r = tid >> 6; k < RG_PER; ++k, r += 4)

// exclusive scan of one int per thread over the block; sh holds 2 * RG_THREADS ints; *total = the block's sum
__device__ __forceinline__ int block_excl_scan(int v, int* sh, int tid, int* total) {
    int cur = 0;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < RG_THREADS; d <<= 1) {
        const int t = sh[cur + tid] + (tid >= d ? sh[cur + tid - d] : 0);
        cur ^= RG_THREADS;
        sh[cur + tid] = t;
        __syncthreads();
    }
    const int incl = sh[cur + tid];
    *total = sh[cur + RG_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// the segments of the table scan: one per (page row, rectangle column), in raster order
struct RegionsWs {
    int64_t npix, nseg, nb;
    int nbx, nby;
};
static inline bool regions_ws(int h, int w, RegionsWs* r) {
    if (h < 1 || w < 1 || (int64_t)h * w > (1ll << 31) - 2) return false;
    r->npix = (int64_t)h * w;
    r->nbx = cdiv(w, RG_W); r->nby = cdiv(h, RG_H);
    r->nseg = (int64_t)h * r->nbx;
    r->nb = cdiv64(r->nseg, RG_THREADS * RG_SCAN);
    return true;
}

}  // namespace tsii
