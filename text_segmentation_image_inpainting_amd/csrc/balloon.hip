// K25: region balloons (include/tsii_hip.h, "region balloons"): for every table row the speech balloon around its lettering -- the flood
// fill from the row's own text over the colour of its ring --, the balloon's area and box, whether it is closed, and the largest upright
// rectangle inside it around the block's centre.  All integer: one defined answer, the same bits on every run.  The header has the
// semantics; this file has one kernel.
//
// A workgroup of 1024 threads owns one table row at a time (a grid of at most BL_SLOTS workgroups walks the rows).  The working set is
// bit planes of the row's window, one uint32 word per 32 window pixels, bit 0 the leftmost: a window of 1024 x 1024 pixels is 128 KiB a
// plane.  The growing plane B always lives in LDS.  The passable plane P lives in LDS behind it while both fit (BL_BOTH words each: up to
// 768 x 768 pixels, 2 x 72 KiB) and in the workgroup's slot of the workspace above that; the fill reads it through one generic pointer.
//
//   1. classify: a thread per word: the text bytes and, for text inside the row's box, the labels -> C (own text, kept in B's place) and T
//                (any text, kept in P's place);
//   2. ring:     over the words around the box only: dilate(C) & ~T from row words (the construction of the K8 mask kernel and of
//                near_bits in region_ring.h, here on 32-bit words with their two neighbours); the ring's page bytes -> n, lo, hi, sum per
//                thread, then LDS atomics by the few threads that met ring pixels (64-bit sums); the anchor is a packed-key minimum over
//                the bits of C in the same walk;
//   3. passable: a thread per word: P = C | (~T & |page - colour| <= tol), over T in place;
//   4. fill:     B = C, then sweeps until none changes a word.  A thread owns a segment of BL_SEG = 33 window rows of one word column and
//                walks it down and then up; at every word the seeds are B itself, the word above (below), bit 31 of the left and bit 0 of
//                the right neighbour; the runs of P that hold a seed are filled with one addition each way (p + s carries through a run of
//                ones; the other direction on the bit-reversed word), which is what the shift-doubling steps compute in 2 x 5 rounds.  A
//                sweep so moves the front 33 pixels up or down and at least one word sideways.  Words are only ever grown and each has one
//                writer, so a neighbour's word read while its owner updates it is a subset of the fixed point: the order of the threads
//                changes the number of sweeps, never the result.  33 rows, not 32: lane t of a sweep reads bank t mod 32 whatever the
//                window's width (the segments lie 33 * WW == WW words apart modulo 32), so a sweep has no LDS bank conflict.
//                Termination is an LDS flag (three of them in rotation: one barrier per sweep); behind it stands a hard stop at the
//                window's pixel count, which a correct fill never reaches;
//   5. measure:  area, box and the open flag by LDS atomics from the threads whose words are not empty; the plane's bytes;
//   6. rectangle: a thread per window row takes L(y) and Rr(y) from B with clz / ctz across words; a thread per ya walks up to the anchor's
//                row and then yb downwards with running max L / min Rr; the winner is the maximum of the key
//                area << 20 | (1023 - ya) << 10 | (1023 - yb), a 64-bit LDS atomic.
// No floating point, no grid-wide barrier, no global atomics; a workgroup writes its rows' outputs, its workspace slot and 255s into plane.
// Every count and box read from the device is clamped: a foreign table gives wrong numbers, never an access outside the buffers.
#include "region_ring.h"

namespace tsii {

constexpr int BL_THREADS = 1024, BL_SIDE = 1024, BL_WORDS = BL_SIDE * BL_SIDE / 32;   // the largest window and its plane
constexpr int BL_BOTH = 768 * 24, BL_LDS = 2 * BL_BOTH;       // words per plane while B and P share the LDS; the LDS array (>= BL_WORDS)
constexpr int BL_SEG = 33, BL_SLOTS = 256, BL_OUT = 16;
constexpr int BL_RING_MAX = 8, BL_REACH_MAX = 512;
// A measurement knob, never set in the product build (tools/variants/build_variant.py -DBL_STOP_AFTER=k): a row ends, with an all-zero
// answer, behind step k (1 classify, 2 ring, 3 passable, 4 fill, 5 measure and the runs' ends), so that the stage's time splits by steps.
#ifndef BL_STOP_AFTER
#define BL_STOP_AFTER 0
#endif
#define BL_STOP(k)                                   \
    if (BL_STOP_AFTER == (k)) {                      \
        if (tid < BL_OUT) out[tid] = 0;              \
        if (tid < 8) rc[tid] = 0;                    \
        continue;                                    \
    }
static_assert(BL_LDS >= BL_WORDS, "B alone must fit");

static inline bool balloon_geometry(int h, int w, int max_regions) {
    return h >= 1 && h <= 32767 && w >= 1 && w <= 32767 && (int64_t)h * w <= (1ll << 31) - 2 && max_regions >= 1;
}
// a slot holds P of the largest window the page allows
static inline size_t balloon_slot_words(int h, int w) {
    const int sh = h < BL_SIDE ? h : BL_SIDE, sw = w < BL_SIDE ? w : BL_SIDE;
    return (size_t)sh * (size_t)((sw + 31) / 32);
}
static inline int balloon_slots(int max_regions) { return max_regions < BL_SLOTS ? max_regions : BL_SLOTS; }
// ws: uint32 P[slots][slot_words] | int sweeps[max_regions] (the sweeps the fill of each served row took: a debug word)
static inline size_t balloon_ws_bytes(int h, int w, int max_regions) {
    return ((size_t)balloon_slots(max_regions) * balloon_slot_words(h, w) + (size_t)max_regions) * 4;
}

__device__ __forceinline__ int bl_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int bl_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int bl_max(int a, int b) { return a > b ? a : b; }
// A word of B that another thread may be growing in the same sweep (its one writer stores with st_own): relaxed workgroup-scope atomic
// accesses, so that the compiler neither keeps such a word in a register across the walk nor tears the access.  Any value read is a
// subset of the fixed point (words only grow), which is all the fill needs.
#ifndef __HIP_MEMORY_SCOPE_WORKGROUP
#define __HIP_MEMORY_SCOPE_WORKGROUP 3
#endif
__device__ __forceinline__ uint32_t ld_shared(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void st_own(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ uint32_t low_bits(int n) { return n >= 32 ? ~0u : ((1u << n) - 1u); }
// the runs of ones of p that hold a bit of s (s within p), whole
__device__ __forceinline__ uint32_t fill_runs(uint32_t p, uint32_t s) {
    const uint32_t up = (p & ~(p + s)) | s;
    const uint32_t pr = __builtin_bitreverse32(p), sr = __builtin_bitreverse32(s);
    return up | __builtin_bitreverse32((pr & ~(pr + sr)) | sr);
}

__global__ __launch_bounds__(BL_THREADS) void balloon_kernel(const uint8_t* __restrict__ page, const uint8_t* __restrict__ text,
                                                             const int* __restrict__ labels, int h, int w, const int* __restrict__ table,
                                                             const int* __restrict__ n_regions, int max_regions, int ring, int tol, int reach,
                                                             uint32_t* slots, size_t slot_words, int* __restrict__ sweeps,
                                                             int* __restrict__ balloon, int64_t* __restrict__ rect, uint8_t* plane) {
    __shared__ uint32_t bits[BL_LDS];
    __shared__ int Ls[BL_SIDE], Rs[BL_SIDE];
    __shared__ u64 s_sum[3], s_best;
    __shared__ int s_n, s_lo[3], s_hi[3], s_area, s_box[4], s_open, s_flag[3];
    __shared__ unsigned s_anchor;
    const int tid = threadIdx.x;
    const int R = clamp_count(n_regions[1], max_regions);
    for (int r = blockIdx.x; r < R; r += gridDim.x) {                    // everything below is uniform over the workgroup
        const int* t = table + (int64_t)r * 6;
        const int lab = t[0];
        const int y0 = bl_clamp(t[2], 0, h), x0 = bl_clamp(t[3], 0, w), y1 = bl_clamp(t[4], 0, h), x1 = bl_clamp(t[5], 0, w);
        const int wy0 = bl_max(y0 - reach, 0), wy1 = bl_min(y1 + reach, h), wx0 = bl_max(x0 - reach, 0), wx1 = bl_min(x1 + reach, w);
        const int wh = wy1 - wy0, ww = wx1 - wx0;
        int* out = balloon + (int64_t)r * BL_OUT;
        int64_t* rc = rect + (int64_t)r * 8;
        int status = (wh > BL_SIDE || ww > BL_SIDE) ? 8 : ((y0 >= y1 || x0 >= x1) ? 16 : 0);
        if (status != 0) {
            if (tid < BL_OUT) out[tid] = tid == 0 ? status : 0;
            if (tid < 8) rc[tid] = 0;
            if (tid == 0) sweeps[r] = 0;
            continue;
        }
        const int WW = (ww + 31) >> 5, nwords = wh * WW;
        uint32_t* B = bits;
        uint32_t* P = nwords <= BL_BOTH ? bits + BL_BOTH : slots + (size_t)blockIdx.x * slot_words;
        __syncthreads();                                                 // the row before is done with the LDS
        if (tid == 0) {
            s_n = 0; s_area = 0; s_open = 0; s_anchor = ~0u; s_best = 0;
            s_flag[0] = s_flag[1] = s_flag[2] = 0;
            s_box[0] = s_box[1] = INT_MAX; s_box[2] = s_box[3] = -1;
            for (int c = 0; c < 3; ++c) { s_lo[c] = 255; s_hi[c] = 0; s_sum[c] = 0; }
        }
        // ---- 1. classify: C -> B, T -> P
        for (int i = tid; i < nwords; i += BL_THREADS) {
            const int ry = i / WW, wc = i - ry * WW, y = wy0 + ry, xb = wx0 + 32 * wc, nb = bl_min(32, wx1 - xb);
            const int64_t base = (int64_t)y * w + xb;
            const bool row_in = y >= y0 && y < y1;
            uint32_t tb = 0, cb = 0;
            for (int k = 0; k < nb; ++k) {
                if (text[base + k] == 0) continue;
                tb |= 1u << k;
                if (row_in && xb + k >= x0 && xb + k < x1 && labels[base + k] == lab) cb |= 1u << k;
            }
            B[i] = cb; P[i] = tb;
        }
        __syncthreads();
        BL_STOP(1)
        // ---- 2. the ring's statistics and the anchor, over the words around the box
        {
            const int ra = bl_max(y0 - ring, wy0) - wy0, rb = bl_min(y1 + ring, wy1) - wy0;
            const int ca = (bl_max(x0 - ring, wx0) - wx0) >> 5, cb = ((bl_min(x1 + ring, wx1) - wx0 - 1) >> 5) + 1;
            const int cn = cb - ca, nsub = (rb - ra) * cn;
            const int cy = y0 + y1 - 1, cx = x0 + x1 - 1;
            int n = 0, lo[3] = {255, 255, 255}, hi[3] = {0, 0, 0};
            unsigned sum[3] = {0u, 0u, 0u}, akey = ~0u;                  // a window's sum stays below 2^20 * 255
            for (int j = tid; j < nsub; j += BL_THREADS) {
                const int ry = ra + j / cn, wc = ca + j % cn, y = wy0 + ry, xb = wx0 + 32 * wc, nb = bl_min(32, wx1 - xb);
                uint32_t acc = 0;
                for (int dy = -ring; dy <= ring; ++dy) {
                    const int yy = ry + dy;
                    if (yy < 0 || yy >= wh) continue;
                    const uint32_t* row = B + yy * WW;
                    const uint32_t a = wc > 0 ? row[wc - 1] : 0u, b = row[wc], c = wc + 1 < WW ? row[wc + 1] : 0u;
                    if ((a | b | c) == 0u) continue;
                    const u64 ab = ((u64)b << 32) | a, bc = ((u64)c << 32) | b;
                    acc |= b;
                    for (int k = 1; k <= ring; ++k) acc |= (uint32_t)(ab >> (32 - k)) | (uint32_t)(bc >> k);
                }
                uint32_t rg = acc & ~P[ry * WW + wc] & low_bits(nb);
                while (rg != 0u) {
                    const int k = __builtin_ctz(rg);
                    rg &= rg - 1u;
                    const uint8_t* px = page + ((int64_t)y * w + xb + k) * 3;
                    ++n;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int v = px[c];
                        lo[c] = v < lo[c] ? v : lo[c]; hi[c] = v > hi[c] ? v : hi[c]; sum[c] += (unsigned)v;
                    }
                }
                uint32_t own = B[ry * WW + wc];
                const int dyc = 2 * y - cy, ady = dyc < 0 ? -dyc : dyc;
                while (own != 0u) {
                    const int k = __builtin_ctz(own);
                    own &= own - 1u;
                    const int dxc = 2 * (xb + k) - cx, adx = dxc < 0 ? -dxc : dxc;
                    const unsigned key = ((unsigned)(ady + adx) << 20) | ((unsigned)ry << 10) | (unsigned)(32 * wc + k);
                    akey = key < akey ? key : akey;
                }
            }
            if (n > 0) {
                atomicAdd(&s_n, n);
                for (int c = 0; c < 3; ++c) { atomicMin(&s_lo[c], lo[c]); atomicMax(&s_hi[c], hi[c]); atomicAdd(&s_sum[c], (u64)sum[c]); }
            }
            if (akey != ~0u) atomicMin(&s_anchor, akey);
        }
        __syncthreads();
        const unsigned anchor = s_anchor;
        if (anchor == ~0u) {                                             // no pixel of the row's own
            if (tid < BL_OUT) out[tid] = tid == 0 ? 16 : 0;
            if (tid < 8) rc[tid] = 0;
            if (tid == 0) sweeps[r] = 0;
            continue;
        }
        BL_STOP(2)
        const int ary = (int)((anchor >> 10) & 1023u), arx = (int)(anchor & 1023u);
        const int n = s_n;
        int col[3];
        status = n == 0 ? 1 : 0;
        for (int c = 0; c < 3; ++c) {
            col[c] = n >= 1 ? (int)((2 * s_sum[c] + (u64)n) / (2 * (u64)n)) : 0;
            if (s_hi[c] - s_lo[c] > tol) status |= 2;
        }
        if (status != 0) {                                               // no colour to follow: no balloon
            if (tid == 0) {
                out[0] = status; out[1] = n; out[2] = col[0]; out[3] = col[1]; out[4] = col[2];
                for (int k = 5; k < BL_OUT; ++k) out[k] = 0;
                out[10] = wy0 + ary; out[11] = wx0 + arx;
                sweeps[r] = 0;
            }
            if (tid < 8) rc[tid] = 0;
            continue;
        }
        // ---- 3. passable: P = C | (~T & the colour within tol)
        for (int i = tid; i < nwords; i += BL_THREADS) {
            const int ry = i / WW, wc = i - ry * WW, y = wy0 + ry, xb = wx0 + 32 * wc, nb = bl_min(32, wx1 - xb);
            const uint8_t* px = page + ((int64_t)y * w + xb) * 3;
            const uint32_t tb = P[i];
            uint32_t pb = B[i];
            for (int k = 0; k < nb; ++k) {
                if ((tb >> k) & 1u) continue;
                const int d0 = (int)px[3 * k] - col[0], d1 = (int)px[3 * k + 1] - col[1], d2 = (int)px[3 * k + 2] - col[2];
                if ((d0 < 0 ? -d0 : d0) <= tol && (d1 < 0 ? -d1 : d1) <= tol && (d2 < 0 ? -d2 : d2) <= tol) pb |= 1u << k;
            }
            P[i] = pb;
        }
        __syncthreads();
        BL_STOP(3)
        // ---- 4. fill
        const int ntasks = ((wh + BL_SEG - 1) / BL_SEG) * WW;
        const int64_t limit = (int64_t)wh * ww;
        int nsweeps = 0;
        for (int64_t it = 0; it < limit; ++it) {
            const int f = (int)(it % 3);
            if (tid == 0) s_flag[(f + 1) % 3] = 0;                        // the flag of the sweep after this one: nobody reads or sets it now
            bool changed = false;
            for (int task = tid; task < ntasks; task += BL_THREADS) {
                const int seg = task / WW, wc = task - seg * WW, ra = seg * BL_SEG, rb = bl_min(ra + BL_SEG, wh);
                const bool left = wc > 0, right = wc + 1 < WW;
                uint32_t prev = ra > 0 ? ld_shared(B + (ra - 1) * WW + wc) : 0u;
                for (int ry = ra; ry < rb; ++ry) {
                    const int i = ry * WW + wc;
                    const uint32_t p = P[i];
                    if (p == 0u) { prev = 0u; continue; }
                    const uint32_t b = B[i];
                    uint32_t s = b | prev;
                    if (left) s |= ld_shared(B + i - 1) >> 31;
                    if (right) s |= ld_shared(B + i + 1) << 31;
                    prev = fill_runs(p, s & p);
                    if (prev != b) { st_own(B + i, prev); changed = true; }
                }
                prev = rb < wh ? ld_shared(B + rb * WW + wc) : 0u;
                for (int ry = rb - 1; ry >= ra; --ry) {
                    const int i = ry * WW + wc;
                    const uint32_t p = P[i];
                    if (p == 0u) { prev = 0u; continue; }
                    const uint32_t b = B[i];
                    uint32_t s = b | prev;
                    if (left) s |= ld_shared(B + i - 1) >> 31;
                    if (right) s |= ld_shared(B + i + 1) << 31;
                    prev = fill_runs(p, s & p);
                    if (prev != b) { st_own(B + i, prev); changed = true; }
                }
            }
            if (changed) s_flag[f] = 1;
            __syncthreads();
            ++nsweeps;
            if (s_flag[f] == 0) break;
        }
        BL_STOP(4)
        // ---- 5. area, box, open; the plane's bytes
        {
            int area = 0, ya = INT_MAX, xa = INT_MAX, yb = -1, xb_ = -1, open = 0;
            for (int i = tid; i < nwords; i += BL_THREADS) {
                const uint32_t b = B[i];
                if (b == 0u) continue;
                const int ry = i / WW, wc = i - ry * WW;
                area += __builtin_popcount(b);
                ya = ry < ya ? ry : ya; yb = ry > yb ? ry : yb;
                const int xl = 32 * wc + __builtin_ctz(b), xr = 32 * wc + 31 - __builtin_clz(b);
                xa = xl < xa ? xl : xa; xb_ = xr > xb_ ? xr : xb_;
                if ((ry == 0 && wy0 > 0) || (ry == wh - 1 && wy1 < h) || (xl == 0 && wx0 > 0) || (xr == ww - 1 && wx1 < w)) open = 1;
                if (plane != nullptr) {
                    uint8_t* dst = plane + (int64_t)(wy0 + ry) * w + wx0 + 32 * wc;
                    uint32_t v = b;
                    while (v != 0u) {
                        dst[__builtin_ctz(v)] = 255;
                        v &= v - 1u;
                    }
                }
            }
            if (area > 0) {
                atomicAdd(&s_area, area);
                atomicMin(&s_box[0], ya); atomicMin(&s_box[1], xa); atomicMax(&s_box[2], yb); atomicMax(&s_box[3], xb_);
                if (open) atomicMax(&s_open, 1);
            }
        }
        // ---- 6. the rectangle: L(y) and Rr(y) of the run through the anchor's column, then the candidates
        for (int ry = tid; ry < wh; ry += BL_THREADS) {
            const uint32_t* row = B + ry * WW;
            const int wc = arx >> 5, bx = arx & 31;
            const uint32_t here = row[wc];
            if (((here >> bx) & 1u) == 0u) { Ls[ry] = -1; Rs[ry] = -1; continue; }
            uint32_t z = ~here & ((1u << bx) - 1u);
            int c = wc;
            while (z == 0u && c > 0) { --c; z = ~row[c]; }
            Ls[ry] = z != 0u ? 32 * c + 32 - __builtin_clz(z) : 0;
            z = ~here & ~((2u << bx) - 1u);
            c = wc;
            while (z == 0u && c + 1 < WW) { ++c; z = ~row[c]; }
            Rs[ry] = z != 0u ? 32 * c + __builtin_ctz(z) - 1 : 32 * WW - 1;
        }
        __syncthreads();
        BL_STOP(5)
        {
            u64 best = 0;
            for (int ya = tid; ya <= ary; ya += BL_THREADS) {
                int mL = 0, mR = INT_MAX;
                bool ok = true;
                for (int y = ya; y <= ary; ++y) {
                    const int l = Ls[y];
                    if (l < 0) { ok = false; break; }
                    mL = l > mL ? l : mL; mR = Rs[y] < mR ? Rs[y] : mR;
                }
                if (!ok) continue;
                for (int yb = ary;;) {
                    const u64 key = ((u64)((yb - ya + 1) * (mR - mL + 1)) << 20) | ((u64)(1023 - ya) << 10) | (u64)(1023 - yb);
                    best = key > best ? key : best;
                    ++yb;
                    if (yb >= wh || Ls[yb] < 0) break;
                    mL = Ls[yb] > mL ? Ls[yb] : mL; mR = Rs[yb] < mR ? Rs[yb] : mR;
                }
            }
            if (best != 0) atomicMax(&s_best, best);
        }
        __syncthreads();
        if (tid == 0) {
            const u64 best = s_best;
            const int ya = 1023 - (int)((best >> 10) & 1023u), yb = 1023 - (int)(best & 1023u);
            int mL = 0, mR = INT_MAX;
            for (int y = ya; y <= yb; ++y) { mL = Ls[y] > mL ? Ls[y] : mL; mR = Rs[y] < mR ? Rs[y] : mR; }
            const int ry0 = wy0 + ya, ry1 = wy0 + yb + 1, rx0 = wx0 + mL, rx1 = wx0 + mR + 1;
            out[0] = s_open ? 4 : 0; out[1] = n; out[2] = col[0]; out[3] = col[1]; out[4] = col[2];
            out[5] = s_area; out[6] = wy0 + s_box[0]; out[7] = wx0 + s_box[1]; out[8] = wy0 + s_box[2] + 1; out[9] = wx0 + s_box[3] + 1;
            out[10] = wy0 + ary; out[11] = wx0 + arx; out[12] = ry0; out[13] = rx0; out[14] = ry1; out[15] = rx1;
            rc[0] = -1; rc[1] = 0; rc[2] = 1; rc[3] = rx0; rc[4] = rx1 - 1; rc[5] = -(int64_t)(ry1 - 1); rc[6] = -(int64_t)ry0; rc[7] = 1;
            sweeps[r] = nsweeps;
        }
    }
}

}  // namespace tsii

using namespace tsii;

extern "C" size_t tsii_region_balloons_ws_bytes(int h, int w, int max_regions, int reach) {
    if (!balloon_geometry(h, w, max_regions) || reach < 1 || reach > BL_REACH_MAX) return 0;
    return balloon_ws_bytes(h, w, max_regions);
}

extern "C" int tsii_region_balloons(const uint8_t* page, const uint8_t* text, const int* labels, int h, int w, const int* table,
                                    const int* n_regions, int max_regions, int ring, int tol, int reach, int* balloon, int64_t* rect,
                                    uint8_t* plane, void* ws, void* stream) {
    TSII_REQUIRE(page && text && labels && table && n_regions && balloon && rect && ws, "region_balloons: null pointer");
    TSII_REQUIRE(balloon_geometry(h, w, max_regions),
                 "region_balloons: page of %d x %d pixels, max_regions %d (sides 1..32767, h * w <= 2^31 - 2, max_regions >= 1)", h, w, max_regions);
    TSII_REQUIRE(ring >= 1 && ring <= BL_RING_MAX, "region_balloons: ring %d (1..%d)", ring, BL_RING_MAX);
    TSII_REQUIRE(tol >= 0 && tol <= 255, "region_balloons: tol %d (0..255)", tol);
    TSII_REQUIRE(reach >= ring && reach <= BL_REACH_MAX, "region_balloons: reach %d (ring %d .. %d)", reach, ring, BL_REACH_MAX);
    TSII_REQUIRE((reinterpret_cast<uintptr_t>(rect) & 7u) == 0, "region_balloons: rect must be 8-byte aligned");
    TSII_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3u) == 0 && (reinterpret_cast<uintptr_t>(balloon) & 3u) == 0,
                 "region_balloons: ws and balloon must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (plane != nullptr && hipMemsetAsync(plane, 0, (size_t)h * w, st) != hipSuccess) return check_launch("region_balloons (memset)");
    const int nslots = balloon_slots(max_regions);
    const size_t slot_words = balloon_slot_words(h, w);
    uint32_t* slots = static_cast<uint32_t*>(ws);
    int* sweeps = reinterpret_cast<int*>(slots + (size_t)nslots * slot_words);
    hipLaunchKernelGGL(balloon_kernel, dim3((unsigned)nslots), dim3(BL_THREADS), 0, st, page, text, labels, h, w, table, n_regions, max_regions,
                       ring, tol, reach, slots, slot_words, sweeps, balloon, rect, plane);
    return check_launch("region_balloons");
}
