// K12: region hulls (include/tsii_hip.h, "region hulls"): the convex hull of every region in the table tsii_text_regions left is filled
// into the uint8 text plane, in place; its pixel count goes to hull_area and the per-tile core counts are taken again of the final
// plane.  All integer, cross products in int64: one defined answer, the same bits on every run.
//
// A region meets every row of its box, so its hull is, row by row, the interval between the lower convex envelope of the rows'
// leftmost pixels and the upper concave envelope of their rightmost ones.  A PAIR is one (region, row of its box); the pairs of all
// table rows lie one region after the other in the workspace and a thread of the middle kernels owns one pair.
//   1. offsets:  one block scans the box heights of the table rows (int64) -> every region's first pair; clears its hull_area;
//   2. init:     xmin = INT_MAX, xmax = -1 for every pair in use (nothing in ws has to be cleared by the caller);
//   3. extents:  one thread per pixel of the label plane; the first / last pixel of a row run finds its table row by binary search
//                (the table ascends in label) and lowers xmin / raises xmax of its pair with one atomic;
//   4. vertices: pair i of a region is a vertex of the lower envelope iff the largest slope from any earlier row to it is smaller than
//                the smallest slope from it to any later row (cross-multiplied); the upper envelope likewise.  O(rows) per pair, all
//                pairs in parallel: a page-tall region is spread over rows / 256 blocks instead of one dependent chain;
//   5. fill:     max-scans over the vertex flags give every pair its neighbouring vertices on both envelopes (a region's first and last
//                rows are vertices, so the scans never leave the region), the row formula gives [xl, xr], a wave per row stores the 1s;
//   6. finish:   one pass over the plane: bytes to 0 / 1, text pixels per tile core.
// No grid-wide barrier, no waiting on another block: each step is its own launch.  Everything read from the table or n_regions is
// clamped before use: a table that does not belong to the labels gives wrong bytes, never an access outside the buffers.
// K22, region geometry, stands behind the hull's kernels in this file: it shares steps 1 to 4 with them.
#include "emu_atomics.h"
#include "page_grid.h"

#include <limits.h>

namespace tsii {

constexpr int HL_THREADS = 256;
constexpr int HL_W = 64, HL_H = 32;              // rectangle of the finish kernel: a wave reads 64 consecutive bytes of a row
constexpr int HL_HDR = 2;                        // ws[0] = pairs in use, ws[1] = R

struct HullWs {
    int64_t npairs;                              // the bound on the pairs, from (h, w, max_regions) alone
    int* hdr;
    int* roff;                                   // [max_regions] first pair of a region
    int* rht;                                    // [max_regions] its rows (0: the region is skipped)
    int* ext;                                    // [npairs][2] xmin, xmax
    uint8_t* vflag;                              // [npairs] bit 0: vertex of the lower envelope, bit 1: of the upper one
};
static inline bool hull_geometry(int h, int w, int max_regions, int64_t* npairs) {
    if (h < 1 || w < 1 || (int64_t)h * w > (1ll << 31) - 2 || max_regions < 1) return false;
    const int64_t a = (int64_t)max_regions * h, b = (int64_t)h * cdiv(w, 2);
    *npairs = a < b ? a : b;
    return true;
}
static inline HullWs hull_ws(void* ws, int max_regions, int64_t npairs) {
    HullWs r;
    r.npairs = npairs;
    r.hdr = static_cast<int*>(ws);
    r.roff = r.hdr + HL_HDR;
    r.rht = r.roff + max_regions;
    r.ext = r.rht + max_regions;
    r.vflag = reinterpret_cast<uint8_t*>(r.ext + 2 * npairs);
    return r;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// inclusive max-scan of one int per thread over the block; sh holds 2 * HL_THREADS ints
__device__ __forceinline__ int block_max_scan(int v, int* sh, int tid) {
    int cur = 0;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < HL_THREADS; d <<= 1) {
        const int a = sh[cur + tid], b = tid >= d ? sh[cur + tid - d] : INT_MIN;
        cur ^= HL_THREADS;
        sh[cur + tid] = a > b ? a : b;
        __syncthreads();
    }
    const int r = sh[cur + tid];
    __syncthreads();
    return r;
}

// ---- 1. offsets ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HL_THREADS) void hull_offsets_kernel(const int* __restrict__ table, const int* __restrict__ n_regions, int max_regions,
                                                                  int h, int64_t npairs, int* __restrict__ hdr, int* __restrict__ roff,
                                                                  int* __restrict__ rht, int* __restrict__ hull_area) {
    __shared__ long long sh[2 * HL_THREADS];
    const int tid = threadIdx.x;
    const int R = clampi(n_regions[1], 0, max_regions);
    long long carry = 0;
    for (int r0 = 0; r0 < R; r0 += HL_THREADS) {
        const int r = r0 + tid;
        int ht = 0;
        if (r < R) {
            const int y0 = clampi(table[(int64_t)r * 6 + 2], 0, h);
            ht = clampi(table[(int64_t)r * 6 + 4], y0, h) - y0;
        }
        int cur = 0;
        sh[tid] = ht;
        __syncthreads();
        for (int d = 1; d < HL_THREADS; d <<= 1) {
            const long long t = sh[cur + tid] + (tid >= d ? sh[cur + tid - d] : 0);
            cur ^= HL_THREADS;
            sh[cur + tid] = t;
            __syncthreads();
        }
        const long long first = carry + sh[cur + tid] - ht;
        carry += sh[cur + HL_THREADS - 1];
        __syncthreads();
        if (r < R) {
            roff[r] = (int)(first < npairs ? first : npairs);
            rht[r] = first + ht <= npairs ? ht : 0;          // only a table that does not belong to the labels gets here with more
            if (hull_area != nullptr) hull_area[r] = 0;     // NULL: the geometry call, which has no such column
        }
    }
    if (tid == 0) {
        hdr[0] = (int)(carry < npairs ? carry : npairs);
        hdr[1] = R;
    }
}

// ---- 2. init ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HL_THREADS) void hull_init_kernel(const int* __restrict__ hdr, int* __restrict__ ext) {
    const int64_t q = (int64_t)blockIdx.x * HL_THREADS + threadIdx.x;
    if (q >= hdr[0]) return;
    ext[2 * q] = INT_MAX;
    ext[2 * q + 1] = -1;
}

// ---- 3. extents ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HL_THREADS) void hull_extents_kernel(const int* __restrict__ labels, int h, int w, const int* __restrict__ table,
                                                                  const int* __restrict__ hdr, const int* __restrict__ roff,
                                                                  const int* __restrict__ rht, int* ext) {
    const int64_t p = (int64_t)blockIdx.x * HL_THREADS + threadIdx.x;
    if (p >= (int64_t)h * w) return;
    const int lab = labels[p];
    if (lab == 0) return;
    const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
    const bool first = x == 0 || labels[p - 1] != lab, last = x == w - 1 || labels[p + 1] != lab;
    if (!first && !last) return;
    const int R = hdr[1];
    int lo = 0, hi = R;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (table[(int64_t)mid * 6] < lab) lo = mid + 1; else hi = mid;
    }
    if (lo >= R || table[(int64_t)lo * 6] != lab) return;      // a kept region beyond the table: no hull
    const int i = y - clampi(table[(int64_t)lo * 6 + 2], 0, h);
    if (i < 0 || i >= rht[lo]) return;
    int* e = ext + 2 * ((int64_t)roff[lo] + i);
    if (first) atomicMin(e, x);
    if (last) atomicMax(e + 1, x);
}

// the region and the row of pair q; false: q belongs to no region
__device__ __forceinline__ bool pair_region(int q, int R, const int* __restrict__ roff, const int* __restrict__ rht, int* r, int* i, int* n) {
    int lo = 0, hi = R;                                       // the last region that starts at or before q
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (roff[mid] <= q) lo = mid + 1; else hi = mid;
    }
    if (lo == 0) return false;
    *r = lo - 1;
    *i = q - roff[lo - 1];
    *n = rht[lo - 1];
    return *i < *n;
}

// ---- 4. vertices -----------------------------------------------------------------------------------------------------------------
// slopes are fractions dx / dy with dy > 0, compared by cross-multiplication in int64
__global__ __launch_bounds__(HL_THREADS) void hull_vertices_kernel(int w, const int* __restrict__ hdr, const int* __restrict__ roff,
                                                                   const int* __restrict__ rht, const int* __restrict__ ext,
                                                                   uint8_t* __restrict__ vflag) {
    const int64_t q64 = (int64_t)blockIdx.x * HL_THREADS + threadIdx.x;
    if (q64 >= hdr[0]) return;
    const int q = (int)q64;
    int r, i, n;
    if (!pair_region(q, hdr[1], roff, rht, &r, &i, &n)) return;
    int flags = 3;
    if (i > 0 && i < n - 1) {
        const int* e = ext + 2 * (int64_t)(q - i);
        const int xl = clampi(e[2 * i], 0, w - 1), xr = clampi(e[2 * i + 1], 0, w - 1);
        // over the earlier rows: the largest slope to xl, the smallest to xr; row i - 1 starts them
        int64_t an = xl - clampi(e[2 * (i - 1)], 0, w - 1), ad = 1, bn = xr - clampi(e[2 * (i - 1) + 1], 0, w - 1), bd = 1;
        for (int j = i - 2; j >= 0; --j) {
            const int64_t d = i - j, nl = xl - clampi(e[2 * j], 0, w - 1), nr = xr - clampi(e[2 * j + 1], 0, w - 1);
            if (nl * ad > an * d) { an = nl; ad = d; }
            if (nr * bd < bn * d) { bn = nr; bd = d; }
        }
        // over the later rows: the smallest slope from xl, the largest from xr
        int64_t cn = clampi(e[2 * (i + 1)], 0, w - 1) - xl, cd = 1, dn = clampi(e[2 * (i + 1) + 1], 0, w - 1) - xr, dd = 1;
        for (int k = i + 2; k < n; ++k) {
            const int64_t d = k - i, nl = clampi(e[2 * k], 0, w - 1) - xl, nr = clampi(e[2 * k + 1], 0, w - 1) - xr;
            if (nl * cd < cn * d) { cn = nl; cd = d; }
            if (nr * dd > dn * d) { dn = nr; dd = d; }
        }
        flags = (an * cd < cn * ad ? 1 : 0) | (bn * dd > dn * bd ? 2 : 0);
    }
    vflag[q] = (uint8_t)flags;
}

// ---- 5. intervals and fill -------------------------------------------------------------------------------------------------------
// the envelope through (ya, xa), (yb, xb) at row y, ya < y < yb, all values >= 0: exact ceiling (up) or floor
__device__ __forceinline__ int envelope_at(int64_t ya, int64_t xa, int64_t yb, int64_t xb, int64_t y, bool up) {
    const int64_t den = yb - ya, num = xa * (yb - y) + xb * (y - ya) + (up ? den - 1 : 0);
    if (((num | den) >> 32) == 0) return (int)((unsigned)num / (unsigned)den);     // every page tsii_text_regions accepts
    return (int)(num / den);
}

__global__ __launch_bounds__(HL_THREADS) void hull_fill_kernel(uint8_t* text, int h, int w, const int* __restrict__ table,
                                                               const int* __restrict__ hdr, const int* __restrict__ roff,
                                                               const int* __restrict__ rht, const int* __restrict__ ext,
                                                               const uint8_t* __restrict__ vflag, int* __restrict__ hull_area) {
    __shared__ int sh[2 * HL_THREADS];
    __shared__ int carry[4];                     // nearest vertex outside the block: lower / upper envelope, before / (negated) behind
    __shared__ int row_y[HL_THREADS], row_x[HL_THREADS], row_len[HL_THREADS];     // first the flags and the mirrored scans' results
    const int tid = threadIdx.x, total = hdr[0];
    const int64_t q0 = (int64_t)blockIdx.x * HL_THREADS;
    if (q0 >= total) return;                     // the whole block
    const int q = (int)q0 + tid;
    int r = 0, i = 0, n = 0;
    const bool valid = q < total && pair_region(q, hdr[1], roff, rht, &r, &i, &n);
    const int f = valid ? vflag[q] : 3;          // a pair of no region ends every scan
    // nearest vertex at or before / at or behind the pair, inside the block (the scans towards the right run on the mirrored block)
    const int pl = block_max_scan((f & 1) ? q : -1, sh, tid), pu = block_max_scan((f & 2) ? q : -1, sh, tid);
    row_y[tid] = f;
    __syncthreads();
    const int m = HL_THREADS - 1 - tid, qm = (int)q0 + m, fm = row_y[m];       // thread tid scans for pair 255 - tid ...
    const int sl = block_max_scan((fm & 1) ? -qm : INT_MIN, sh, tid), su = block_max_scan((fm & 2) ? -qm : INT_MIN, sh, tid);
    row_x[m] = sl; row_len[m] = su;                                           // ... and hands the result over
    __syncthreads();
    const int nl = row_x[tid], nu = row_len[tid];
    __syncthreads();
    // ... and outside it: the block looks 256 pairs at a time until both envelopes have one
    if (tid < 4) carry[tid] = tid < 2 ? -1 : INT_MIN;
    __syncthreads();
    for (int64_t c = q0 - HL_THREADS; c >= 0; c -= HL_THREADS) {
        const int fc = vflag[c + tid];
        if (fc & 1) atomicMax(carry + 0, (int)c + tid);
        if (fc & 2) atomicMax(carry + 1, (int)c + tid);
        __syncthreads();
        const bool done = carry[0] >= 0 && carry[1] >= 0;
        __syncthreads();
        if (done) break;
    }
    for (int64_t c = q0 + HL_THREADS; c < total; c += HL_THREADS) {
        const int fc = c + tid < total ? vflag[c + tid] : 3;
        if (fc & 1) atomicMax(carry + 2, -((int)c + tid));
        if (fc & 2) atomicMax(carry + 3, -((int)c + tid));
        __syncthreads();
        const bool done = carry[2] > INT_MIN && carry[3] > INT_MIN;
        __syncthreads();
        if (done) break;
    }
    int len = 0, xl = 0, y = 0;
    if (valid) {
        const int base = q - i, end = base + n - 1;           // the region's first and last pairs: vertices of both envelopes
        const int* e = ext;
        y = clampi(table[(int64_t)r * 6 + 2], 0, h) + i;      // < h: rht was cut to the page
        int xr;
        if (f & 1) xl = clampi(e[2 * (int64_t)q], 0, w - 1);
        else {
            const int a = clampi(pl >= 0 ? pl : carry[0], base, q - 1);
            const int b = clampi(nl > INT_MIN ? -nl : (carry[2] > INT_MIN ? -carry[2] : end), q + 1, end);
            xl = envelope_at(a, clampi(e[2 * (int64_t)a], 0, w - 1), b, clampi(e[2 * (int64_t)b], 0, w - 1), q, true);
        }
        if (f & 2) xr = clampi(e[2 * (int64_t)q + 1], 0, w - 1);
        else {
            const int a = clampi(pu >= 0 ? pu : carry[1], base, q - 1);
            const int b = clampi(nu > INT_MIN ? -nu : (carry[3] > INT_MIN ? -carry[3] : end), q + 1, end);
            xr = envelope_at(a, clampi(e[2 * (int64_t)a + 1], 0, w - 1), b, clampi(e[2 * (int64_t)b + 1], 0, w - 1), q, false);
        }
        xl = clampi(xl, 0, w - 1);
        xr = clampi(xr, 0, w - 1);
        len = xr >= xl ? xr - xl + 1 : 0;
        if (len > 0) atomicAdd(hull_area + r, len);
    }
    row_y[tid] = y; row_x[tid] = xl; row_len[tid] = len;
    __syncthreads();
    // a wave per row: bytes up to the first 16-byte boundary, 16-byte stores, the last bytes.  Overlapping hulls store the same value.
    const int lane = tid & 63;
    for (int t = tid >> 6; t < HL_THREADS; t += HL_THREADS / 64) {
        const int n1 = row_len[t];
        if (n1 == 0) continue;
        uint8_t* p = text + (int64_t)row_y[t] * w + row_x[t];
        int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u);
        if (head > n1) head = n1;
        if (lane < head) p[lane] = 1;
        const int chunks = (n1 - head) >> 4, tail = (n1 - head) & 15;
        uint4 ones;
        ones.x = ones.y = ones.z = ones.w = 0x01010101u;
        for (int c = lane; c < chunks; c += 64) *reinterpret_cast<uint4*>(p + head + 16 * c) = ones;
        if (lane < tail) p[head + 16 * chunks + lane] = 1;
    }
}

// ---- 6. finish -------------------------------------------------------------------------------------------------------------------
// a block owns a 64 x 32 rectangle of one tile core (the geometry of the plane_up kernel): one atomic per block
__global__ __launch_bounds__(HL_THREADS) void hull_finish_kernel(uint8_t* __restrict__ text, PageGrid g, int nbx, int nby, int* __restrict__ core_count) {
    __shared__ int wave_count[HL_THREADS / 64];
    const int tid = threadIdx.x, c = tid & 63;
    const int t = blockIdx.x / (nbx * nby), sub = blockIdx.x % (nbx * nby);
    const int ci = t / g.tx, cj = t % g.tx;
    const int64_t y0 = (int64_t)ci * g.s + (sub / nbx) * HL_H, x0 = (int64_t)cj * g.s + (sub % nbx) * HL_W;
    const int64_t yend = (int64_t)(ci + 1) * g.s < g.h ? (int64_t)(ci + 1) * g.s : g.h, xend = (int64_t)(cj + 1) * g.s < g.w ? (int64_t)(cj + 1) * g.s : g.w;
    if (y0 >= yend || x0 >= xend) return;               // the whole block
    int cnt = 0;
    if (x0 + c < xend) {
        for (int row = tid >> 6; row < HL_H && y0 + row < yend; row += HL_THREADS / 64) {
            uint8_t* p = text + (y0 + row) * g.w + x0 + c;
            const uint8_t v = *p;
            if (v > 1) *p = 1;
            cnt += v != 0;
        }
    }
    if (core_count == nullptr) return;                  // the whole grid
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_down(cnt, d);
    if (c == 0) wave_count[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int k = 0; k < HL_THREADS / 64; ++k) total += wave_count[k];
        if (total > 0) atomicAdd(core_count + t, total);
    }
}

// ==== K22: region geometry (include/tsii_hip.h, "region geometry") ====================================================================
// The hull's vertices in order and the minimum-area enclosing rectangle of every table row.  Kernels 1-4 above run unchanged (the
// offsets kernel without a hull_area column); behind them a wave owns a region:
//   5g. polygon: the flagged pairs become the ordered polygon -- the first row's leftmost pixel, the right chain downwards, the left
//                chain upwards; the two ends of the first and the last row each once.  Two passes over the region's pairs: the chains'
//                lengths (a wave sum), then a wave scan per 64 pairs gives every vertex its place.  The full list goes to the workspace
//                (one word per vertex: y << 16 | x, both below 2^15), the first max_vertices of it to the caller;
//   6g. rect:    a lane per edge (lane, lane + 64, ...) walks the region's vertex list -- every lane reads the same word, the list is
//                short and comes from L2 -- for the extreme dot products along the edge and its normal; the lanes' best edges meet in a
//                butterfly of shuffles.  Areas are the fractions A / D with A < 2^62 and D < 2^31: compared by cross-multiplication
//                in 128 bits made of 64-bit halves, ties to the smaller edge, so every lane ends with the same winner and its owner
//                stores the row.
// No atomics, no LDS, no block barrier.
constexpr int GM_WAVES = HL_THREADS / 64;        // regions per block
constexpr int GM_MAX_SIDE = 32767;               // every dot product fits int32, every area product int64

struct GeometryWs {
    HullWs hull;
    int* nvert;                                  // [max_regions] vertices of a region's hull
    int* vlist;                                  // [2 * npairs] region r's vertices from 2 * roff[r] on
};
static inline bool geometry_args_ok(int h, int w, int max_regions, int max_vertices, int64_t* npairs) {
    return h <= GM_MAX_SIDE && w <= GM_MAX_SIDE && max_vertices >= 3 && max_vertices <= 1024 && hull_geometry(h, w, max_regions, npairs);
}
static inline size_t hull_ws_bytes(int max_regions, int64_t npairs) {
    return (sizeof(int) * (size_t)(HL_HDR + 2 * (int64_t)max_regions + 2 * npairs) + (size_t)npairs + 3) / 4 * 4;
}
static inline GeometryWs geometry_ws(void* ws, int max_regions, int64_t npairs) {
    GeometryWs r;
    r.hull = hull_ws(ws, max_regions, npairs);
    r.nvert = reinterpret_cast<int*>(static_cast<char*>(ws) + hull_ws_bytes(max_regions, npairs));
    r.vlist = r.nvert + max_regions;
    return r;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ long long shfl_xor_i64(long long v, int d) {
    const unsigned lo = __shfl_xor((unsigned)((unsigned long long)v & 0xffffffffull), d), hi = __shfl_xor((unsigned)((unsigned long long)v >> 32), d);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// ---- 5g. polygon -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void put_vertex(int* __restrict__ vl, int* __restrict__ vo, int max_vertices, int pos, int y, int x) {
    vl[pos] = (y << 16) | x;
    if (pos < max_vertices) {
        vo[2 * pos] = y;
        vo[2 * pos + 1] = x;
    }
}

__global__ __launch_bounds__(HL_THREADS) void geometry_polygon_kernel(int h, int w, const int* __restrict__ table, const int* __restrict__ hdr,
                                                                      const int* __restrict__ roff, const int* __restrict__ rht,
                                                                      const int* __restrict__ ext, const uint8_t* __restrict__ vflag,
                                                                      int max_vertices, int* __restrict__ nvert, int* __restrict__ vlist,
                                                                      int* __restrict__ n_vertices, int* __restrict__ vertices) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * GM_WAVES + (threadIdx.x >> 6);
    if (r >= hdr[1]) return;                     // the whole wave, here and below
    const int n = rht[r];
    if (n <= 0) {                                // only a table that does not belong to the labels
        if (lane == 0) nvert[r] = n_vertices[r] = 0;
        return;
    }
    const int64_t base = roff[r];                // base + n <= npairs (offsets kernel)
    const int y0 = clampi(table[(int64_t)r * 6 + 2], 0, h);      // y0 + n <= h
    const int* e = ext + 2 * base;
    const uint8_t* f = vflag + base;
    const bool one_top = clampi(e[0], 0, w - 1) == clampi(e[1], 0, w - 1);
    // a pair's right end is listed unless it is the first row's and that row is one pixel; its left end unless it is the first row's
    // (the start of the list) or the last row's and that row is one pixel
    int cr = 0, cl = 0;
    for (int i = lane; i < n; i += 64) {
        const int fl = f[i];
        cr += (fl & 2) && !(i == 0 && one_top);
        cl += (fl & 1) && i > 0 && !(i == n - 1 && clampi(e[2 * i], 0, w - 1) == clampi(e[2 * i + 1], 0, w - 1));
    }
    const int nr = wave_sum(cr), nl = wave_sum(cl), total = 1 + nr + nl;     // <= 2 n
    int* vl = vlist + 2 * base;
    int* vo = vertices + (int64_t)r * max_vertices * 2;
    if (lane == 0) {
        put_vertex(vl, vo, max_vertices, 0, y0, clampi(e[0], 0, w - 1));
        nvert[r] = n_vertices[r] = total;
    }
    int before_r = 0, before_l = 0;              // listed ends in the rows above this chunk
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        int er = 0, el = 0, xl = 0, xr = 0;
        if (i < n) {
            const int fl = f[i];
            xl = clampi(e[2 * i], 0, w - 1);
            xr = clampi(e[2 * i + 1], 0, w - 1);
            er = (fl & 2) && !(i == 0 && one_top);
            el = (fl & 1) && i > 0 && !(i == n - 1 && xl == xr);
        }
        const int sr = wave_inclusive_scan(er, lane), sl = wave_inclusive_scan(el, lane);
        if (er) put_vertex(vl, vo, max_vertices, before_r + sr, y0 + i, xr);                        // 1 + the ends above it
        if (el) put_vertex(vl, vo, max_vertices, 1 + nr + nl - (before_l + sl), y0 + i, xl);      // 1 + nr + the ends below it
        before_r += __shfl(sr, 63);
        before_l += __shfl(sl, 63);
    }
}

// ---- 6g. rect --------------------------------------------------------------------------------------------------------------------
struct U128 { unsigned long long hi, lo; };
__device__ __forceinline__ U128 mul_64x64(unsigned long long a, unsigned long long b) {
    const unsigned long long a0 = a & 0xffffffffull, a1 = a >> 32, b0 = b & 0xffffffffull, b1 = b >> 32;
    const unsigned long long p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const unsigned long long mid = (p00 >> 32) + (p01 & 0xffffffffull) + (p10 & 0xffffffffull);
    U128 r;
    r.lo = (p00 & 0xffffffffull) | (mid << 32);
    r.hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
    return r;
}
// the rectangle of edge k1, area a1 / d1, comes before that of k2: the smaller area, then the smaller edge; k < 0: no edge yet
__device__ __forceinline__ bool rect_before(long long a1, int d1, int k1, long long a2, int d2, int k2) {
    if (k1 < 0) return false;
    if (k2 < 0) return true;
    const U128 p = mul_64x64((unsigned long long)a1, (unsigned long long)d2), q = mul_64x64((unsigned long long)a2, (unsigned long long)d1);
    if (p.hi != q.hi) return p.hi < q.hi;
    if (p.lo != q.lo) return p.lo < q.lo;
    return k1 < k2;
}

__global__ __launch_bounds__(HL_THREADS) void geometry_rect_kernel(const int* __restrict__ hdr, const int* __restrict__ roff,
                                                                   const int* __restrict__ nvert, const int* __restrict__ vlist,
                                                                   long long* __restrict__ rect) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * GM_WAVES + (threadIdx.x >> 6);
    if (r >= hdr[1]) return;                     // the whole wave, here and below
    const int n = nvert[r];
    long long* out = rect + 8 * (int64_t)r;
    if (n <= 0) {
        if (lane < 8) out[lane] = lane == 0 ? -1 : 0;
        return;
    }
    const int* vl = vlist + 2 * (int64_t)roff[r];
    if (n == 1) {                                // d = (0, 1), n = (-1, 0): d . V = x, n . V = -y
        if (lane == 0) {
            const long long y = vl[0] >> 16, x = vl[0] & 0xffff;
            out[0] = -1; out[1] = 0; out[2] = 1; out[3] = x; out[4] = x; out[5] = -y; out[6] = -y; out[7] = 1;
        }
        return;
    }
    int k_best = -1, dy_best = 0, dx_best = 0, d_best = 1, lo_d_best = 0, hi_d_best = 0, lo_n_best = 0, hi_n_best = 0;
    long long a_best = 0;
    for (int k = lane; k < n; k += 64) {
        const int p = vl[k], q = vl[k + 1 == n ? 0 : k + 1];
        const int dy = (q >> 16) - (p >> 16), dx = (q & 0xffff) - (p & 0xffff);
        int lo_d = INT_MAX, hi_d = INT_MIN, lo_n = INT_MAX, hi_n = INT_MIN;
        for (int j = 0; j < n; ++j) {
            const int v = vl[j], y = v >> 16, x = v & 0xffff;
            const int pd = dy * y + dx * x, pn = dy * x - dx * y;        // |.| <= 2 * 32766^2 < 2^31
            lo_d = pd < lo_d ? pd : lo_d; hi_d = pd > hi_d ? pd : hi_d;
            lo_n = pn < lo_n ? pn : lo_n; hi_n = pn > hi_n ? pn : hi_n;
        }
        const long long a = ((long long)hi_d - lo_d) * ((long long)hi_n - lo_n);
        const int d = dy * dy + dx * dx;
        if (rect_before(a, d, k, a_best, d_best, k_best)) {
            k_best = k; a_best = a; d_best = d; dy_best = dy; dx_best = dx;
            lo_d_best = lo_d; hi_d_best = hi_d; lo_n_best = lo_n; hi_n_best = hi_n;
        }
    }
    int k_win = k_best, d_win = d_best;
    long long a_win = a_best;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const int k2 = __shfl_xor(k_win, s), d2 = __shfl_xor(d_win, s);
        const long long a2 = shfl_xor_i64(a_win, s);
        if (rect_before(a2, d2, k2, a_win, d_win, k_win)) { k_win = k2; d_win = d2; a_win = a2; }
    }
    if (k_best >= 0 && k_best == k_win) {        // one lane: an edge belongs to one lane
        out[0] = k_best; out[1] = dy_best; out[2] = dx_best; out[3] = lo_d_best; out[4] = hi_d_best; out[5] = lo_n_best; out[6] = hi_n_best;
        out[7] = d_best;
    }
}

}  // namespace tsii

using namespace tsii;

extern "C" size_t tsii_region_hulls_ws_bytes(int h, int w, int max_regions) {
    int64_t npairs;
    if (!hull_geometry(h, w, max_regions, &npairs)) return 0;
    return hull_ws_bytes(max_regions, npairs);
}

extern "C" int tsii_region_hulls(uint8_t* text, const int* labels, int h, int w, const int* table, const int* n_regions, int max_regions,
                                 int tile, int halo, int* core_count, int* hull_area, void* ws, void* stream) {
    TSII_REQUIRE(text && labels && table && n_regions && hull_area && ws, "region_hulls: null pointer");
    int64_t npairs;
    TSII_REQUIRE(hull_geometry(h, w, max_regions, &npairs), "region_hulls: page of %d x %d pixels, max_regions %d (h, w >= 1, h * w <= 2^31 - 2, max_regions >= 1)",
                 h, w, max_regions);
    TSII_REQUIRE(core_count == nullptr || grid_ok(h, w, tile, halo), "region_hulls: bad geometry h %d w %d tile %d halo %d", h, w, tile, halo);
    TSII_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3u) == 0, "region_hulls: ws must be 4-byte aligned");
    const ApplyGrid a = make_apply_grid(h, w, tile, halo, core_count, HL_W, HL_H);
    TSII_REQUIRE(a.napply < (1ll << 31), "region_hulls: bad geometry h %d w %d tile %d halo %d (too many tile cores)", h, w, tile, halo);
    hipStream_t st = (hipStream_t)stream;
    if (!clear_core_count(core_count, a.g, st)) return check_launch("region_hulls (memset)");
    const HullWs s = hull_ws(ws, max_regions, npairs);
    const unsigned pair_blocks = flat_grid(npairs, HL_THREADS);
    hipLaunchKernelGGL(hull_offsets_kernel, dim3(1), dim3(HL_THREADS), 0, st, table, n_regions, max_regions, h, npairs, s.hdr, s.roff, s.rht, hull_area);
    hipLaunchKernelGGL(hull_init_kernel, dim3(pair_blocks), dim3(HL_THREADS), 0, st, s.hdr, s.ext);
    hipLaunchKernelGGL(hull_extents_kernel, dim3(flat_grid((int64_t)h * w, HL_THREADS)), dim3(HL_THREADS), 0, st, labels, h, w, table, s.hdr, s.roff,
                       s.rht, s.ext);
    hipLaunchKernelGGL(hull_vertices_kernel, dim3(pair_blocks), dim3(HL_THREADS), 0, st, w, s.hdr, s.roff, s.rht, s.ext, s.vflag);
    hipLaunchKernelGGL(hull_fill_kernel, dim3(pair_blocks), dim3(HL_THREADS), 0, st, text, h, w, table, s.hdr, s.roff, s.rht, s.ext, s.vflag, hull_area);
    hipLaunchKernelGGL(hull_finish_kernel, dim3((unsigned)a.napply), dim3(HL_THREADS), 0, st, text, a.g, a.nbx, a.nby, core_count);
    return check_launch("region_hulls");
}

extern "C" size_t tsii_region_geometry_ws_bytes(int h, int w, int max_regions, int max_vertices) {
    int64_t npairs;
    if (!geometry_args_ok(h, w, max_regions, max_vertices, &npairs)) return 0;
    return hull_ws_bytes(max_regions, npairs) + sizeof(int) * (size_t)(max_regions + 2 * npairs);
}

extern "C" int tsii_region_geometry(const int* labels, const int* table, const int* n_regions, int max_regions, int h, int w, int max_vertices,
                                    int* n_vertices, int* vertices, int64_t* rect, void* ws, size_t ws_bytes, void* stream) {
    TSII_REQUIRE(labels && table && n_regions && n_vertices && vertices && rect && ws, "region_geometry: null pointer");
    int64_t npairs;
    TSII_REQUIRE(geometry_args_ok(h, w, max_regions, max_vertices, &npairs),
                 "region_geometry: page of %d x %d pixels, max_regions %d, max_vertices %d (h, w 1..32767, max_regions >= 1, max_vertices 3..1024)",
                 h, w, max_regions, max_vertices);
    TSII_REQUIRE(ws_bytes >= tsii_region_geometry_ws_bytes(h, w, max_regions, max_vertices), "region_geometry: workspace of %zu bytes, %zu needed",
                 ws_bytes, tsii_region_geometry_ws_bytes(h, w, max_regions, max_vertices));
    TSII_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3u) == 0 && (reinterpret_cast<uintptr_t>(rect) & 7u) == 0,
                 "region_geometry: ws must be 4-byte aligned, rect 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const GeometryWs s = geometry_ws(ws, max_regions, npairs);
    const unsigned pair_blocks = flat_grid(npairs, HL_THREADS), region_blocks = flat_grid(max_regions, GM_WAVES);
    hipLaunchKernelGGL(hull_offsets_kernel, dim3(1), dim3(HL_THREADS), 0, st, table, n_regions, max_regions, h, npairs, s.hull.hdr, s.hull.roff,
                       s.hull.rht, (int*)nullptr);
    hipLaunchKernelGGL(hull_init_kernel, dim3(pair_blocks), dim3(HL_THREADS), 0, st, s.hull.hdr, s.hull.ext);
    hipLaunchKernelGGL(hull_extents_kernel, dim3(flat_grid((int64_t)h * w, HL_THREADS)), dim3(HL_THREADS), 0, st, labels, h, w, table, s.hull.hdr,
                       s.hull.roff, s.hull.rht, s.hull.ext);
    hipLaunchKernelGGL(hull_vertices_kernel, dim3(pair_blocks), dim3(HL_THREADS), 0, st, w, s.hull.hdr, s.hull.roff, s.hull.rht, s.hull.ext,
                       s.hull.vflag);
    hipLaunchKernelGGL(geometry_polygon_kernel, dim3(region_blocks), dim3(HL_THREADS), 0, st, h, w, table, s.hull.hdr, s.hull.roff, s.hull.rht,
                       s.hull.ext, s.hull.vflag, max_vertices, s.nvert, s.vlist, n_vertices, vertices);
    hipLaunchKernelGGL(geometry_rect_kernel, dim3(region_blocks), dim3(HL_THREADS), 0, st, s.hull.hdr, s.hull.roff, s.nvert, s.vlist,
                       reinterpret_cast<long long*>(rect));
    return check_launch("region_geometry");
}
