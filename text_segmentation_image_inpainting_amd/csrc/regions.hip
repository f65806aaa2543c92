// K10: text regions (include/tsii_hip.h, "text regions"): connected-component labelling of the uint8 text plane of the page pipeline,
// area and box of every component, a minimum-area filter applied in place, per-tile core counts of what is left, and a table of the
// kept components in raster order of their first pixels.  All integer; the label of a component is 1 + its smallest pixel index, so
// the result does not depend on the order in which blocks or atomics happen to run.
//
// Union-find over the int32 label plane itself: labels[p] = 1 + parent(p) for a text pixel (a root points at itself), 0 for
// background; links only ever go to a smaller index.  A block owns RG_W x RG_H page pixels; a row of the rectangle is one 64-bit word,
// so a row RUN (maximal stretch of set bits) is found with bit operations and stands in for its pixels everywhere below.
//   1. local:   runs of neighbouring rows are united in LDS; every pixel gets the global index of its local root (4 B / pixel written,
//               1 B read) and the local roots' statistics are initialised (nothing in ws has to be cleared by the caller);
//   2. seam:    one thread per pixel of a rectangle's first column / first row unites it with its neighbours across the seam
//               (atomicMin find / union on the label plane);
//   3. measure: one thread per run resolves the run's root once (and leaves it in the run's first pixel); area and box meet per root
//               in an LDS hash table and leave the block as one set of atomics per (block, root);
//   4. filter:  labels and text are rewritten from the runs' roots and the roots' areas, kept pixels are counted per (block, tile
//               core), found / kept roots per block, kept roots per (row, rectangle column) segment -- segments are in raster order;
//   5. table:   two-level exclusive scan of the segment counts, then every segment writes the rows of its kept roots.
// No grid-wide barrier, no waiting on another block: each step is its own launch.
#include "region_bits.h"

namespace tsii {

// a[x] = OFF + parent of x; OFF = 0 in LDS (local indices), 1 on the label plane (0 = background)
template <int OFF>
__device__ __forceinline__ int uf_find(const int* a, int x) {
    for (;;) {
        const int p = ld(a + x) - OFF;
        if (p == x) return x;
        x = p;
    }
}
template <int OFF>
__device__ __forceinline__ void uf_unite(int* a, int x, int y) {
    for (;;) {
        x = uf_find<OFF>(a, x);
        y = uf_find<OFF>(a, y);
        if (x == y) return;
        if (x < y) { const int t = x; x = y; y = t; }
        const int old = atomicMin(a + x, y + OFF) - OFF;      // the larger root now points at the smaller one ...
        if (old == x) return;
        x = old;                                             // ... unless it had a parent by then: unite that one with y as well
    }
}

// ---- 1. local labelling ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_THREADS) void regions_local_kernel(const uint8_t* __restrict__ text, int h, int w, int nbx, int conn8,
                                                                   int* __restrict__ labels, int* __restrict__ stats) {
    __shared__ u64 bytes[RG_H][8];
    __shared__ u64 bits[RG_H];
    __shared__ int parent[RG_PIX];
    const int tid = threadIdx.x;
    const int x0 = (blockIdx.x % nbx) * RG_W, y0 = (blockIdx.x / nbx) * RG_H;
    {
        uint8_t* bt = reinterpret_cast<uint8_t*>(&bytes[0][0]);
        RG_FOR_PIXELS(k, r, c) {
            const int x = x0 + c, y = y0 + r;
            bt[r * RG_W + c] = (x < w && y < h && text[(int64_t)y * w + x] != 0) ? 1 : 0;
        }
    }
    __syncthreads();
    pack_rows(bytes, bits, tid);
    __syncthreads();
    {
        RG_FOR_PIXELS(k, r, c) {
            const u64 b = bits[r];
            if (((b >> c) & 1ull) && (c == 0 || !((b >> (c - 1)) & 1ull))) parent[r * RG_W + c] = r * RG_W + c;
        }
    }
    __syncthreads();
    {   // every run below the first row: unite with the runs of the row above that touch it (8: diagonally as well)
        RG_FOR_PIXELS(k, r, c) {
            const u64 b = bits[r];
            if (r > 0 && ((b >> c) & 1ull) && (c == 0 || !((b >> (c - 1)) & 1ull))) {
                u64 span = bit_span(c, run_len(b, c));
                if (conn8) span |= (span << 1) | (span >> 1);
                const u64 up = bits[r - 1];
                u64 m = up & span;
                while (m) {
                    const int cb = __builtin_ctzll(m);
                    uf_unite<0>(parent, r * RG_W + c, (r - 1) * RG_W + run_start(up, cb));
                    m &= ~bit_span(cb, run_len(up, cb));
                }
            }
        }
    }
    __syncthreads();
    {   // flatten the runs' links (a link replaced while another thread walks it still leads to the same root)
        RG_FOR_PIXELS(k, r, c) {
            const u64 b = bits[r];
            if (((b >> c) & 1ull) && (c == 0 || !((b >> (c - 1)) & 1ull))) st(parent + r * RG_W + c, uf_find<0>(parent, r * RG_W + c));
        }
    }
    __syncthreads();
    {
        RG_FOR_PIXELS(k, r, c) {
            const int x = x0 + c, y = y0 + r;
            if (x < w && y < h) {
                const u64 b = bits[r];
                int out = 0;
                if ((b >> c) & 1ull) {
                    const int lr = parent[r * RG_W + run_start(b, c)];
                    const int64_t gi = (int64_t)(y0 + (lr >> 6)) * w + x0 + (lr & 63);
                    out = (int)gi + 1;
                    if (lr == r * RG_W + c) {           // a local root: the only pixels that can end up as a component's root
                        int* s = stats + gi * RG_STATS;
                        s[0] = 0; s[1] = INT_MAX; s[2] = INT_MAX; s[3] = 0; s[4] = 0;
                    }
                }
                labels[(int64_t)y * w + x] = out;
            }
        }
    }
}

// ---- 2. seams ----------------------------------------------------------------------------------------------------------------------
// Two pixels of different rectangles that touch: either they differ in the rectangle ROW, then the lower one is in a first row and the
// other is at (y - 1, x - 1 .. x + 1); or only in the rectangle COLUMN, then the right one is in a first column and the other is at
// (y - 1 .. y + 1, x - 1).  (A corner pair met by both rules is united twice, which changes nothing.)
__device__ __forceinline__ void seam_unite(int* labels, int p, int64_t q) {
    if (ld(labels + q) != 0) uf_unite<1>(labels, p, (int)q);
}
__global__ __launch_bounds__(RG_THREADS) void regions_seam_kernel(int* labels, int h, int w, int conn8, int64_t n_vertical, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    if (i < n_vertical) {
        const int x = (int)(i / h + 1) * RG_W, y = (int)(i % h);
        const int64_t p = (int64_t)y * w + x;
        if (ld(labels + p) == 0) return;
        seam_unite(labels, (int)p, p - 1);
        if (conn8) {
            if (y > 0) seam_unite(labels, (int)p, p - w - 1);
            if (y + 1 < h) seam_unite(labels, (int)p, p + w - 1);
        }
    } else {
        const int64_t j = i - n_vertical;
        const int y = (int)(j / w + 1) * RG_H, x = (int)(j % w);
        const int64_t p = (int64_t)y * w + x;
        if (ld(labels + p) == 0) return;
        seam_unite(labels, (int)p, p - w);
        if (conn8) {
            if (x > 0) seam_unite(labels, (int)p, p - w - 1);
            if (x + 1 < w) seam_unite(labels, (int)p, p - w + 1);
        }
    }
}

// ---- 3. flatten and measure --------------------------------------------------------------------------------------------------------
// at most 32 runs per row, 1024 per rectangle: the table is never more than half full
constexpr int RG_HASH = 2048;
__global__ __launch_bounds__(RG_THREADS) void regions_measure_kernel(int* labels, int h, int w, int nbx, int* stats) {
    __shared__ u64 bytes[RG_H][8];
    __shared__ u64 bits[RG_H];
    __shared__ int hkey[RG_HASH], harea[RG_HASH], hy0[RG_HASH], hx0[RG_HASH], hy1[RG_HASH], hx1[RG_HASH];
    const int tid = threadIdx.x;
    const int x0 = (blockIdx.x % nbx) * RG_W, y0 = (blockIdx.x / nbx) * RG_H;
    for (int j = tid; j < RG_HASH; j += RG_THREADS) {
        hkey[j] = -1; harea[j] = 0; hy0[j] = INT_MAX; hx0[j] = INT_MAX; hy1[j] = 0; hx1[j] = 0;
    }
    int v[RG_PER];
    {
        uint8_t* bt = reinterpret_cast<uint8_t*>(&bytes[0][0]);
        RG_FOR_PIXELS(k, r, c) {
            const int x = x0 + c, y = y0 + r;
            v[k] = (x < w && y < h) ? ld(labels + (int64_t)y * w + x) : 0;
            bt[r * RG_W + c] = v[k] != 0 ? 1 : 0;
        }
    }
    __syncthreads();
    pack_rows(bytes, bits, tid);
    __syncthreads();
    {
        RG_FOR_PIXELS(k, r, c) {
            const u64 b = bits[r];
            if (((b >> c) & 1ull) && (c == 0 || !((b >> (c - 1)) & 1ull))) {
                const int x = x0 + c, y = y0 + r, len = run_len(b, c);
                const int gi = (int)((int64_t)y * w + x);
                const int root = uf_find<1>(labels, v[k] - 1);
                if (root != gi) st(labels + gi, root + 1);           // the filter reads the run's root here
                unsigned slot = ((unsigned)root * 2654435761u) >> 21;  // 11 bits
                for (;;) {
                    const int was = atomicCAS(hkey + slot, -1, root);
                    if (was == -1 || was == root) break;
                    slot = (slot + 1) & (RG_HASH - 1);
                }
                atomicAdd(harea + slot, len);
                atomicMin(hy0 + slot, y); atomicMin(hx0 + slot, x);
                atomicMax(hy1 + slot, y + 1); atomicMax(hx1 + slot, x + len);
            }
        }
    }
    __syncthreads();
    for (int j = tid; j < RG_HASH; j += RG_THREADS) {
        if (hkey[j] >= 0) {
            int* s = stats + (int64_t)hkey[j] * RG_STATS;
            atomicAdd(s, harea[j]);
            atomicMin(s + 1, hy0[j]); atomicMin(s + 2, hx0[j]);
            atomicMax(s + 3, hy1[j]); atomicMax(s + 4, hx1[j]);
        }
    }
}

// ---- 4. filter and count -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_THREADS) void regions_filter_kernel(int* __restrict__ labels, uint8_t* __restrict__ text, int h, int w, int nbx,
                                                                    const int* __restrict__ stats, int min_area, PageGrid g,
                                                                    int* __restrict__ core_count, int* __restrict__ n_regions,
                                                                    int* __restrict__ segcnt) {
    __shared__ u64 bytes[RG_H][8];
    __shared__ u64 bits[RG_H];
    __shared__ int fin[RG_PIX];          // final label of the run that starts here
    __shared__ int cnt[RG_PIX];          // kept pixels per tile core that meets the rectangle (at most one core per pixel)
    __shared__ int rowkept[RG_H];
    __shared__ int nroots[2];
    const int tid = threadIdx.x;
    const int bx = blockIdx.x % nbx, x0 = bx * RG_W, y0 = (blockIdx.x / nbx) * RG_H;
    if (tid < RG_H) rowkept[tid] = 0;
    if (tid < 2) nroots[tid] = 0;
    int v[RG_PER];
    uint8_t* bt = reinterpret_cast<uint8_t*>(&bytes[0][0]);
    {
        RG_FOR_PIXELS(k, r, c) {
            const int x = x0 + c, y = y0 + r;
            v[k] = (x < w && y < h) ? labels[(int64_t)y * w + x] : 0;
            bt[r * RG_W + c] = v[k] != 0 ? 1 : 0;
        }
    }
    __syncthreads();
    pack_rows(bytes, bits, tid);
    __syncthreads();
    {
        RG_FOR_PIXELS(k, r, c) {
            const u64 b = bits[r];
            if (((b >> c) & 1ull) && (c == 0 || !((b >> (c - 1)) & 1ull))) {
                const int gi = (int)((int64_t)(y0 + r) * w + x0 + c);
                const bool keep = stats[(int64_t)(v[k] - 1) * RG_STATS] >= min_area;
                fin[r * RG_W + c] = keep ? v[k] : 0;
                if (v[k] - 1 == gi) {
                    atomicAdd(nroots, 1);
                    if (keep) { atomicAdd(nroots + 1, 1); atomicAdd(rowkept + r, 1); }
                }
            }
        }
    }
    __syncthreads();
    {
        RG_FOR_PIXELS(k, r, c) {
            const int x = x0 + c, y = y0 + r;
            const u64 b = bits[r];
            const int out = ((b >> c) & 1ull) ? fin[r * RG_W + run_start(b, c)] : 0;
            if (x < w && y < h) {
                labels[(int64_t)y * w + x] = out;
                text[(int64_t)y * w + x] = out != 0 ? 1 : 0;
            }
            bt[r * RG_W + c] = out != 0 ? 1 : 0;
        }
    }
    if (tid < RG_H && y0 + tid < h) segcnt[(int64_t)(y0 + tid) * nbx + bx] = rowkept[tid];
    if (tid == 0) {
        if (nroots[0]) atomicAdd(n_regions, nroots[0]);
        if (nroots[1]) atomicAdd(n_regions + 1, nroots[1]);
    }
    if (core_count == nullptr) return;                  // the whole grid
    __syncthreads();
    pack_rows(bytes, bits, tid);                        // the kept pixels now
    const int xe = (x0 + RG_W < w ? x0 + RG_W : w), ye = (y0 + RG_H < h ? y0 + RG_H : h);
    const int tj0 = x0 / g.s, ntj = (xe - 1) / g.s - tj0 + 1, ti0 = y0 / g.s, nti = (ye - 1) / g.s - ti0 + 1;
    for (int j = tid; j < nti * ntj; j += RG_THREADS) cnt[j] = 0;
    __syncthreads();
    if (tid < RG_H && y0 + tid < h && bits[tid] != 0) {
        const u64 kb = bits[tid];
        const int ti = (y0 + tid) / g.s - ti0;
        for (int tj = 0; tj < ntj; ++tj) {
            const int xa = ((tj0 + tj) * g.s > x0 ? (tj0 + tj) * g.s : x0) - x0;
            const int xb = ((tj0 + tj + 1) * g.s < x0 + RG_W ? (tj0 + tj + 1) * g.s : x0 + RG_W) - x0;
            const int n = __builtin_popcountll(kb & bit_span(xa, xb - xa));
            if (n) atomicAdd(cnt + ti * ntj + tj, n);
        }
    }
    __syncthreads();
    for (int j = tid; j < nti * ntj; j += RG_THREADS)
        if (cnt[j]) atomicAdd(core_count + (ti0 + j / ntj) * g.tx + tj0 + j % ntj, cnt[j]);
}

// ---- 5. scan of the segment counts and the table -----------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_THREADS) void regions_scan_sums_kernel(const int* __restrict__ segcnt, int64_t nseg, int* __restrict__ bsum) {
    __shared__ int sh[2 * RG_THREADS];
    const int tid = threadIdx.x;
    const int64_t s0 = ((int64_t)blockIdx.x * RG_THREADS + tid) * RG_SCAN;
    int sum = 0;
    for (int k = 0; k < RG_SCAN; ++k) sum += s0 + k < nseg ? segcnt[s0 + k] : 0;
    int total;
    block_excl_scan(sum, sh, tid, &total);
    if (tid == 0) bsum[blockIdx.x] = total;
}
// one block: bsum -> its exclusive scan, in place
__global__ __launch_bounds__(RG_THREADS) void regions_scan_top_kernel(int* bsum, int nb) {
    __shared__ int sh[2 * RG_THREADS];
    const int tid = threadIdx.x;
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += RG_THREADS) {
        const int v = b0 + tid < nb ? bsum[b0 + tid] : 0;
        int total;
        const int ex = block_excl_scan(v, sh, tid, &total);
        if (b0 + tid < nb) bsum[b0 + tid] = carry + ex;
        carry += total;
    }
}
__global__ __launch_bounds__(RG_THREADS) void regions_table_kernel(const int* __restrict__ labels, int w, int nbx, const int* __restrict__ segcnt,
                                                                   int64_t nseg, const int* __restrict__ bsum, const int* __restrict__ stats,
                                                                   int max_regions, int* __restrict__ table) {
    __shared__ int sh[2 * RG_THREADS];
    const int tid = threadIdx.x;
    const int64_t s0 = ((int64_t)blockIdx.x * RG_THREADS + tid) * RG_SCAN;
    int n[RG_SCAN], sum = 0;
    for (int k = 0; k < RG_SCAN; ++k) { n[k] = s0 + k < nseg ? segcnt[s0 + k] : 0; sum += n[k]; }
    int total;
    int row = bsum[blockIdx.x] + block_excl_scan(sum, sh, tid, &total);
    for (int k = 0; k < RG_SCAN && row < max_regions; ++k) {
        if (n[k] == 0) continue;
        const int y = (int)((s0 + k) / nbx), x0 = (int)((s0 + k) % nbx) * RG_W;
        const int xe = x0 + RG_W < w ? x0 + RG_W : w;
        for (int x = x0; x < xe && row < max_regions; ++x) {
            const int64_t p = (int64_t)y * w + x;
            if (labels[p] != (int)p + 1) continue;      // after the filter: exactly the kept roots
            const int* s = stats + p * RG_STATS;
            int* t = table + (int64_t)row * 6;
            t[0] = (int)p + 1; t[1] = s[0]; t[2] = s[1]; t[3] = s[2]; t[4] = s[3]; t[5] = s[4];
            ++row;
        }
    }
}

}  // namespace tsii

using namespace tsii;

extern "C" size_t tsii_text_regions_ws_bytes(int h, int w, int max_regions) {
    RegionsWs r;
    if (max_regions < 0 || !regions_ws(h, w, &r)) return 0;
    return sizeof(int) * (size_t)(r.npix * RG_STATS + r.nseg + r.nb);
}

extern "C" int tsii_text_regions(uint8_t* text, int h, int w, int connectivity, int min_area, int max_regions,
                                 int tile, int halo, int* core_count, int* labels, int* table, int* n_regions, void* ws, void* stream) {
    TSII_REQUIRE(text && labels && n_regions && ws, "text_regions: null pointer");
    TSII_REQUIRE(connectivity == 4 || connectivity == 8, "text_regions: connectivity %d (4 or 8)", connectivity);
    RegionsWs r;
    TSII_REQUIRE(regions_ws(h, w, &r), "text_regions: page of %d x %d pixels (h, w >= 1, h * w <= 2^31 - 2)", h, w);
    TSII_REQUIRE(max_regions >= 0 && (max_regions == 0 || table != nullptr), "text_regions: max_regions %d (>= 0, with a table unless 0)", max_regions);
    TSII_REQUIRE(core_count == nullptr || grid_ok(h, w, tile, halo), "text_regions: bad geometry h %d w %d tile %d halo %d", h, w, tile, halo);
    TSII_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3u) == 0, "text_regions: ws must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    PageGrid g = make_grid(h, w, 32, 0);                // not used without core_count
    if (core_count != nullptr) {
        g = make_grid(h, w, tile, halo);
        if (hipMemsetAsync(core_count, 0, sizeof(int) * (size_t)g.ty * g.tx, st) != hipSuccess) return check_launch("text_regions (memset)");
    }
    if (hipMemsetAsync(n_regions, 0, 2 * sizeof(int), st) != hipSuccess) return check_launch("text_regions (memset)");
    int* stats = static_cast<int*>(ws);
    int* segcnt = stats + r.npix * RG_STATS;
    int* bsum = segcnt + r.nseg;
    const int conn8 = connectivity == 8;
    const unsigned nblocks = (unsigned)(r.nbx * r.nby);
    hipLaunchKernelGGL(regions_local_kernel, dim3(nblocks), dim3(RG_THREADS), 0, st, text, h, w, r.nbx, conn8, labels, stats);
    const int64_t n_vertical = (int64_t)(r.nbx - 1) * h, n_seam = n_vertical + (int64_t)(r.nby - 1) * w;
    if (n_seam > 0)
        hipLaunchKernelGGL(regions_seam_kernel, dim3(flat_grid(n_seam, RG_THREADS)), dim3(RG_THREADS), 0, st, labels, h, w, conn8, n_vertical, n_seam);
    hipLaunchKernelGGL(regions_measure_kernel, dim3(nblocks), dim3(RG_THREADS), 0, st, labels, h, w, r.nbx, stats);
    hipLaunchKernelGGL(regions_filter_kernel, dim3(nblocks), dim3(RG_THREADS), 0, st, labels, text, h, w, r.nbx, stats, min_area, g,
                       core_count, n_regions, segcnt);
    if (max_regions > 0) {
        hipLaunchKernelGGL(regions_scan_sums_kernel, dim3((unsigned)r.nb), dim3(RG_THREADS), 0, st, segcnt, r.nseg, bsum);
        hipLaunchKernelGGL(regions_scan_top_kernel, dim3(1), dim3(RG_THREADS), 0, st, bsum, (int)r.nb);
        hipLaunchKernelGGL(regions_table_kernel, dim3((unsigned)r.nb), dim3(RG_THREADS), 0, st, labels, w, r.nbx, segcnt, r.nseg, bsum, stats,
                           max_regions, table);
    }
    return check_launch("text_regions");
}
