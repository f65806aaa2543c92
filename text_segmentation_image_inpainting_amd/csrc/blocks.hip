// K15: text blocks (include/tsii_hip.h, "text blocks"): single-linkage grouping of the components of a label plane at Chebyshev distance
// `gap`.  The label of a block is 1 + its smallest pixel index, area, box and member count go with it; the area filter, the per-tile core
// counts and the table are those of K10, taken per block.  All integer, nothing depends on the order of blocks or atomics.
//
// F = the labelled pixels.  F dilated by the square window [-b, +a]^2 (a = (gap - 1) / 2, b = gap - 1 - a: `gap` cells a side) puts a
// square around every pixel of F; two squares overlap or touch, corners included, iff their pixels are at most `gap` apart, so the
// 8-connected components of the dilated plane D are the blocks -- and K10 labels D.
//   1. pack:    F as one bit per pixel, 64 pixels a word: a wave reads 64 consecutive labels of a row (the one pass over the int32 plane),
//               the flags become words in LDS the way K10 packs its rectangles (no ballot: the same code runs on the test emulator);
//   2. dilate:  a block owns 256 x 32 pixels of D.  Row words of F, each OR-ed with its shifted self over the window (a word and its
//               two neighbours, doubling: O(log gap) shifts), go to LDS; the rows are OR-ed over the window by doubling in LDS; the
//               bits leave as bytes, 16 to a store wherever the address allows;
//   3. label:   tsii_text_regions on D, 8-connected, no filter, no table, on the same stream (its workspace is a piece of ours);
//   4. min:     the first pixel of every row run of F lowers the cell of its D-component to its own index + 1: the block's label;
//   5. name:    block_labels = that cell on F, 0 elsewhere; a block's first pixel initialises the block's statistics;
//   6. measure: area and box per run, members per component first pixel, met in an LDS hash table per 64 x 32 rectangle (as K10 does)
//               and added to the block's statistics with one set of atomics per (rectangle, block);
//   7. filter, scan, table: block_labels and text are rewritten by the area filter; counts and the table as in K10.
// No grid-wide barrier, no waiting on another block: each step is its own launch.
#include "emu_atomics.h"
#include "region_bits.h"

namespace tsii {

constexpr int BK_GAP_MAX = 64;
constexpr int DL_WORDS = 4, DL_ROWS = 32;                    // the dilate kernel's rectangle: 256 x 32 pixels
constexpr int DL_IN = DL_ROWS + BK_GAP_MAX - 1;              // the rows of F it depends on
constexpr int DL_CHUNKS = DL_WORDS * 4 + 1;                  // 16-byte pieces of one row of the rectangle, the unaligned head included

// ---- 1. pack ---------------------------------------------------------------------------------------------------------------------
// a block packs 32 words: its waves read 64 consecutive labels of a row each, the flags meet in LDS as bytes, 32 threads make the words
__global__ __launch_bounds__(RG_THREADS) void blocks_pack_kernel(const int* __restrict__ labels, int w, int wpr, int64_t nwords,
                                                                 u64* __restrict__ fbits) {
    __shared__ u64 bytes[RG_H][8];
    __shared__ u64 bits[RG_H];
    const int tid = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * RG_H;
    {
        uint8_t* bt = reinterpret_cast<uint8_t*>(&bytes[0][0]);
        RG_FOR_PIXELS(k, r, c) {
            const int64_t i = first + r, y = i / wpr;
            const int x = (int)(i - y * wpr) * 64 + c;
            bt[r * RG_W + c] = (i < nwords && x < w && labels[y * w + x] != 0) ? 1 : 0;
        }
    }
    __syncthreads();
    pack_rows(bytes, bits, tid);
    if (tid < RG_H && first + tid < nwords) fbits[first + tid] = bits[tid];
}

// ---- 2. dilate -------------------------------------------------------------------------------------------------------------------
// OR of the 128-bit value hi:lo shifted by 0 .. n-1 (n <= 33) towards bit 0 (DOWN) or away from it, by doubling
template <bool DOWN>
__device__ __forceinline__ void or_window(u64& hi, u64& lo, int n) {
    int cov = 1;
    for (;;) {
        const int s = 2 * cov <= n ? cov : n - cov;
        if (s == 0) return;
        if (DOWN) { lo |= (lo >> s) | (hi << (64 - s)); hi |= hi >> s; }
        else { hi |= (hi << s) | (lo >> (64 - s)); lo |= lo << s; }
        cov += s;
    }
}
// 8 bits -> 8 bytes of 0 / 1, bit 0 in the lowest byte
__device__ __forceinline__ u64 spread8(u64 b) {
    return ((((b & 0xffull) * 0x0101010101010101ull) & 0x8040201008040201ull) + 0x7f7f7f7f7f7f7f7full) >> 7 & 0x0101010101010101ull;
}

__global__ __launch_bounds__(RG_THREADS) void blocks_dilate_kernel(const u64* __restrict__ fbits, int h, int w, int wpr, int nbx, int a, int b,
                                                                   uint8_t* __restrict__ dplane) {
    __shared__ u64 rows[2][DL_IN][DL_WORDS];
    const int tid = threadIdx.x, gap = a + b + 1;
    const int wx0 = (blockIdx.x % nbx) * DL_WORDS, y0 = (blockIdx.x / nbx) * DL_ROWS;
    const int nin = DL_ROWS + gap - 1;                       // row r of the staging is page row y0 - a + r: D(y) = OR of rows y - a .. y + b
    // along the rows: D(x) = OR of F(x - a .. x + b)
    for (int j = tid; j < nin * DL_WORDS; j += RG_THREADS) {
        const int r = j / DL_WORDS, c = j % DL_WORDS, y = y0 - a + r, wx = wx0 + c;
        u64 acc = 0;
        if (y >= 0 && y < h && wx < wpr) {
            const u64* row = fbits + (int64_t)y * wpr;
            const u64 mid = row[wx];
            u64 hi = wx + 1 < wpr ? row[wx + 1] : 0ull, lo = mid;
            or_window<true>(hi, lo, b + 1);                  // the pixels to the right come down
            acc = lo;
            hi = mid; lo = wx > 0 ? row[wx - 1] : 0ull;
            or_window<false>(hi, lo, a + 1);                 // the pixels to the left go up
            acc |= hi;
        }
        rows[0][r][c] = acc;
    }
    __syncthreads();
    // down the columns: out(j) = OR of staging rows j .. j + gap - 1
    int cur = 0, cov = 1;
    for (;;) {
        const int s = 2 * cov <= gap ? cov : gap - cov;
        if (s == 0) break;
        for (int j = tid; j < nin * DL_WORDS; j += RG_THREADS) {
            const int r = j / DL_WORDS, c = j % DL_WORDS;
            rows[cur ^ 1][r][c] = rows[cur][r][c] | (r + s < nin ? rows[cur][r + s][c] : 0ull);
        }
        __syncthreads();
        cur ^= 1;
        cov += s;
    }
    // bits to bytes
    const int x0 = wx0 * 64, ncols = w - x0 < DL_WORDS * 64 ? w - x0 : DL_WORDS * 64;
    for (int j = tid; j < DL_ROWS * DL_CHUNKS; j += RG_THREADS) {
        const int r = j / DL_CHUNKS, k = j % DL_CHUNKS, y = y0 + r;
        if (y >= h) break;
        uint8_t* p = dplane + (int64_t)y * w + x0;
        const int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u);
        const int first = k == 0 ? 0 : head + 16 * (k - 1);
        int end = k == 0 ? head : first + 16;
        if (end > ncols) end = ncols;
        if (first >= end) continue;
        const int wi = first >> 6, sh = first & 63;
        u64 bits = rows[cur][r][wi] >> sh;
        if (sh > 48 && wi + 1 < DL_WORDS) bits |= rows[cur][r][wi + 1] << (64 - sh);
        if (end - first == 16 && k > 0) {
            const u64 s0 = spread8(bits), s1 = spread8(bits >> 8);
            uint4 v;
            v.x = (unsigned)s0; v.y = (unsigned)(s0 >> 32); v.z = (unsigned)s1; v.w = (unsigned)(s1 >> 32);
            *reinterpret_cast<uint4*>(p + first) = v;
        } else {
            for (int i = first; i < end; ++i) p[i] = (uint8_t)((bits >> (i - first)) & 1ull);
        }
    }
}

// ---- 4. min ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_THREADS) void blocks_min_kernel(const int* __restrict__ labels, const int* __restrict__ dlabels, int w, int64_t npix,
                                                                unsigned* __restrict__ bmin) {
    const int64_t p = (int64_t)blockIdx.x * RG_THREADS + threadIdx.x;
    if (p >= npix || labels[p] == 0) return;
    if (p % w != 0 && labels[p - 1] != 0) return;            // not the first pixel of its row run
    const int d = dlabels[p];
    if (d > 0) atomicMin(bmin + (d - 1), (unsigned)p + 1u);
}

// ---- 5. name ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_THREADS) void blocks_name_kernel(const int* __restrict__ labels, const int* __restrict__ dlabels, int64_t npix,
                                                                 const unsigned* __restrict__ bmin, int* __restrict__ block_labels,
                                                                 int* __restrict__ stats, int* __restrict__ members) {
    const int64_t p = (int64_t)blockIdx.x * RG_THREADS + threadIdx.x;
    if (p >= npix) return;
    int out = 0;
    if (labels[p] != 0) {
        const int d = dlabels[p];
        const unsigned m = d > 0 ? bmin[d - 1] : 0u;
        out = (m >= 1u && m <= (unsigned)p + 1u) ? (int)m : (int)p + 1;     // always so behind steps 2 to 4: an index into this page
        if (out == (int)p + 1) {
            int* s = stats + p * RG_STATS;
            s[0] = 0; s[1] = INT_MAX; s[2] = INT_MAX; s[3] = 0; s[4] = 0;
            members[p] = 0;
        }
    }
    block_labels[p] = out;
}

// ---- 6. measure ------------------------------------------------------------------------------------------------------------------
// at most 32 runs per row, 1024 per rectangle: the table is never more than half full
constexpr int BK_HASH = 2048;
__global__ __launch_bounds__(RG_THREADS) void blocks_measure_kernel(const int* __restrict__ block_labels, const int* __restrict__ labels, int h, int w,
                                                                    int nbx, int64_t npix, int* stats, int* members) {
    __shared__ u64 bytes[RG_H][8];
    __shared__ u64 bits[RG_H];
    __shared__ int hkey[BK_HASH], harea[BK_HASH], hy0[BK_HASH], hx0[BK_HASH], hy1[BK_HASH], hx1[BK_HASH], hmem[BK_HASH];
    const int tid = threadIdx.x;
    const int x0 = (blockIdx.x % nbx) * RG_W, y0 = (blockIdx.x / nbx) * RG_H;
    for (int j = tid; j < BK_HASH; j += RG_THREADS) {
        hkey[j] = -1; harea[j] = 0; hy0[j] = INT_MAX; hx0[j] = INT_MAX; hy1[j] = 0; hx1[j] = 0; hmem[j] = 0;
    }
    int v[RG_PER];
    {
        uint8_t* bt = reinterpret_cast<uint8_t*>(&bytes[0][0]);
        RG_FOR_PIXELS(k, r, c) {
            const int x = x0 + c, y = y0 + r;
            v[k] = (x < w && y < h) ? block_labels[(int64_t)y * w + x] : 0;
            bt[r * RG_W + c] = v[k] != 0 ? 1 : 0;
        }
    }
    __syncthreads();
    pack_rows(bytes, bits, tid);
    __syncthreads();
    {
        RG_FOR_PIXELS(k, r, c) {
            const u64 bw = bits[r];
            if (((bw >> c) & 1ull) && (c == 0 || !((bw >> (c - 1)) & 1ull))) {       // the first pixel of a run: one block
                const int x = x0 + c, y = y0 + r, len = run_len(bw, c);
                const int gi = (int)((int64_t)y * w + x);
                const int root = v[k] - 1;
                if (root < 0 || root >= npix) continue;
                unsigned slot = ((unsigned)root * 2654435761u) >> 21;                // 11 bits
                for (;;) {
                    const int was = atomicCAS(hkey + slot, -1, root);
                    if (was == -1 || was == root) break;
                    slot = (slot + 1) & (BK_HASH - 1);
                }
                atomicAdd(harea + slot, len);
                atomicMin(hy0 + slot, y); atomicMin(hx0 + slot, x);
                atomicMax(hy1 + slot, y + 1); atomicMax(hx1 + slot, x + len);
                if (labels[gi] == gi + 1) atomicAdd(hmem + slot, 1);                 // a component's first pixel starts a run
            }
        }
    }
    __syncthreads();
    for (int j = tid; j < BK_HASH; j += RG_THREADS) {
        if (hkey[j] >= 0) {
            int* s = stats + (int64_t)hkey[j] * RG_STATS;
            atomicAdd(s, harea[j]);
            atomicMin(s + 1, hy0[j]); atomicMin(s + 2, hx0[j]);
            atomicMax(s + 3, hy1[j]); atomicMax(s + 4, hx1[j]);
            if (hmem[j]) atomicAdd(members + hkey[j], hmem[j]);
        }
    }
}

// ---- 7. filter, scan, table ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_THREADS) void blocks_filter_kernel(int* __restrict__ block_labels, uint8_t* __restrict__ text, int h, int w, int nbx,
                                                                   int64_t npix, const int* __restrict__ stats, int min_area, PageGrid g,
                                                                   int* __restrict__ core_count, int* __restrict__ n_blocks,
                                                                   int* __restrict__ segcnt) {
    __shared__ u64 bytes[RG_H][8];
    __shared__ u64 bits[RG_H];
    __shared__ int cnt[RG_PIX];          // kept pixels per tile core that meets the rectangle (at most one core per pixel)
    __shared__ int rowkept[RG_H];
    __shared__ int nroots[2];
    const int tid = threadIdx.x;
    const int bx = blockIdx.x % nbx, x0 = bx * RG_W, y0 = (blockIdx.x / nbx) * RG_H;
    if (tid < RG_H) rowkept[tid] = 0;
    if (tid < 2) nroots[tid] = 0;
    __syncthreads();
    uint8_t* bt = reinterpret_cast<uint8_t*>(&bytes[0][0]);
    {
        RG_FOR_PIXELS(k, r, c) {
            const int x = x0 + c, y = y0 + r;
            int out = 0;
            if (x < w && y < h) {
                const int64_t p = (int64_t)y * w + x;
                const int v = block_labels[p];
                if (v >= 1 && v <= npix) {
                    const bool keep = stats[(int64_t)(v - 1) * RG_STATS] >= min_area;
                    out = keep ? v : 0;
                    if (v - 1 == p) {
                        atomicAdd(nroots, 1);
                        if (keep) { atomicAdd(nroots + 1, 1); atomicAdd(rowkept + r, 1); }
                    }
                }
                block_labels[p] = out;
                text[p] = out != 0 ? 1 : 0;
            }
            bt[r * RG_W + c] = out != 0 ? 1 : 0;
        }
    }
    __syncthreads();
    if (tid < RG_H && y0 + tid < h) segcnt[(int64_t)(y0 + tid) * nbx + bx] = rowkept[tid];
    if (tid == 0) {
        if (nroots[0]) atomicAdd(n_blocks, nroots[0]);
        if (nroots[1]) atomicAdd(n_blocks + 1, nroots[1]);
    }
    if (core_count == nullptr) return;                  // the whole grid
    pack_rows(bytes, bits, tid);                        // the kept pixels
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

__global__ __launch_bounds__(RG_THREADS) void blocks_scan_sums_kernel(const int* __restrict__ segcnt, int64_t nseg, int* __restrict__ bsum) {
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
__global__ __launch_bounds__(RG_THREADS) void blocks_scan_top_kernel(int* bsum, int nb) {
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
__global__ __launch_bounds__(RG_THREADS) void blocks_table_kernel(const int* __restrict__ block_labels, int w, int nbx, const int* __restrict__ segcnt,
                                                                  int64_t nseg, const int* __restrict__ bsum, const int* __restrict__ stats,
                                                                  const int* __restrict__ members_in, int max_regions, int* __restrict__ table,
                                                                  int* __restrict__ members) {
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
            if (block_labels[p] != (int)p + 1) continue;    // after the filter: exactly the kept blocks' first pixels
            const int* s = stats + p * RG_STATS;
            int* t = table + (int64_t)row * 6;
            t[0] = (int)p + 1; t[1] = s[0]; t[2] = s[1]; t[3] = s[2]; t[4] = s[3]; t[5] = s[4];
            members[row] = members_in[p];
            ++row;
        }
    }
}

// the workspace, every piece on a 16-byte boundary of it
struct BlocksWs {
    RegionsWs r;
    int wpr;
    int64_t nwords;
    size_t counts, fbits, dplane, dlabels, bmin, members, segcnt, bsum, shared, total;      // byte offsets
};
static inline size_t up16(size_t v) { return (v + 15) / 16 * 16; }
static inline bool blocks_ws(int h, int w, int max_regions, int gap, BlocksWs* s) {
    if (max_regions < 0 || gap < 1 || gap > BK_GAP_MAX || !regions_ws(h, w, &s->r)) return false;
    const size_t labelling = tsii_text_regions_ws_bytes(h, w, 0);
    if (labelling == 0) return false;
    const size_t npix = (size_t)s->r.npix;
    s->wpr = cdiv(w, 64);
    s->nwords = (int64_t)h * s->wpr;
    size_t at = 0;
    s->counts = at;  at += 16;                                              // the labelling's {found, kept}
    s->fbits = at;   at += up16(sizeof(u64) * (size_t)s->nwords);
    s->dplane = at;  at += up16(npix);
    s->dlabels = at; at += up16(sizeof(int) * npix);
    s->bmin = at;    at += up16(sizeof(int) * npix);
    s->members = at; at += up16(sizeof(int) * npix);
    s->segcnt = at;  at += up16(sizeof(int) * (size_t)s->r.nseg);
    s->bsum = at;    at += up16(sizeof(int) * (size_t)s->r.nb);
    s->shared = at;  at += up16(labelling);     // first the labelling's workspace, then -- that call is over -- the blocks' statistics
    s->total = at;
    return labelling >= sizeof(int) * npix * RG_STATS;
}

}  // namespace tsii

using namespace tsii;

extern "C" size_t tsii_text_blocks_ws_bytes(int h, int w, int max_regions, int gap) {
    BlocksWs s;
    return blocks_ws(h, w, max_regions, gap, &s) ? s.total : 0;
}

extern "C" int tsii_text_blocks(uint8_t* text, const int* labels, int h, int w, int gap, int min_area, int max_regions,
                                int tile, int halo, int* core_count, int* block_labels, int* table, int* members,
                                int* n_blocks, void* ws, void* stream) {
    TSII_REQUIRE(text && labels && block_labels && n_blocks && ws, "text_blocks: null pointer");
    TSII_REQUIRE(block_labels != labels, "text_blocks: block_labels must not be the label plane itself");
    TSII_REQUIRE(gap >= 1 && gap <= BK_GAP_MAX, "text_blocks: gap %d (1..%d)", gap, BK_GAP_MAX);
    TSII_REQUIRE(max_regions >= 0 && (max_regions == 0 || (table != nullptr && members != nullptr)),
                 "text_blocks: max_regions %d (>= 0, with a table and members unless 0)", max_regions);
    BlocksWs s;
    TSII_REQUIRE(blocks_ws(h, w, max_regions, gap, &s), "text_blocks: page of %d x %d pixels (h, w >= 1, h * w <= 2^31 - 2)", h, w);
    TSII_REQUIRE(core_count == nullptr || grid_ok(h, w, tile, halo), "text_blocks: bad geometry h %d w %d tile %d halo %d", h, w, tile, halo);
    TSII_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, "text_blocks: ws must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* base = static_cast<char*>(ws);
    int* counts = reinterpret_cast<int*>(base + s.counts);
    u64* fbits = reinterpret_cast<u64*>(base + s.fbits);
    uint8_t* dplane = reinterpret_cast<uint8_t*>(base + s.dplane);
    int* dlabels = reinterpret_cast<int*>(base + s.dlabels);
    unsigned* bmin = reinterpret_cast<unsigned*>(base + s.bmin);
    int* nmemb = reinterpret_cast<int*>(base + s.members);
    int* segcnt = reinterpret_cast<int*>(base + s.segcnt);
    int* bsum = reinterpret_cast<int*>(base + s.bsum);
    int* stats = reinterpret_cast<int*>(base + s.shared);
    const RegionsWs& r = s.r;
    const int a = (gap - 1) / 2, b = gap - 1 - a;
    PageGrid g = make_grid(h, w, 32, 0);                // not used without core_count
    if (core_count != nullptr) {
        g = make_grid(h, w, tile, halo);
        if (hipMemsetAsync(core_count, 0, sizeof(int) * (size_t)g.ty * g.tx, st) != hipSuccess) return check_launch("text_blocks (memset)");
    }
    if (hipMemsetAsync(n_blocks, 0, 2 * sizeof(int), st) != hipSuccess) return check_launch("text_blocks (memset)");
    if (hipMemsetAsync(bmin, 0xff, sizeof(int) * (size_t)r.npix, st) != hipSuccess) return check_launch("text_blocks (memset)");
    hipLaunchKernelGGL(blocks_pack_kernel, dim3(flat_grid(s.nwords, RG_H)), dim3(RG_THREADS), 0, st, labels, w, s.wpr, s.nwords,
                       fbits);
    const int dbx = cdiv(s.wpr, DL_WORDS), dby = cdiv(h, DL_ROWS);
    hipLaunchKernelGGL(blocks_dilate_kernel, dim3((unsigned)(dbx * dby)), dim3(RG_THREADS), 0, st, fbits, h, w, s.wpr, dbx, a, b, dplane);
    const int rc = tsii_text_regions(dplane, h, w, 8, 0, 0, 0, 0, nullptr, dlabels, nullptr, counts, stats, stream);
    if (rc != 0) return rc;
    const unsigned pix_blocks = flat_grid(r.npix, RG_THREADS), nblocks = (unsigned)(r.nbx * r.nby);
    hipLaunchKernelGGL(blocks_min_kernel, dim3(pix_blocks), dim3(RG_THREADS), 0, st, labels, dlabels, w, r.npix, bmin);
    hipLaunchKernelGGL(blocks_name_kernel, dim3(pix_blocks), dim3(RG_THREADS), 0, st, labels, dlabels, r.npix, bmin, block_labels, stats, nmemb);
    hipLaunchKernelGGL(blocks_measure_kernel, dim3(nblocks), dim3(RG_THREADS), 0, st, block_labels, labels, h, w, r.nbx, r.npix, stats, nmemb);
    hipLaunchKernelGGL(blocks_filter_kernel, dim3(nblocks), dim3(RG_THREADS), 0, st, block_labels, text, h, w, r.nbx, r.npix, stats, min_area, g,
                       core_count, n_blocks, segcnt);
    if (max_regions > 0) {
        hipLaunchKernelGGL(blocks_scan_sums_kernel, dim3((unsigned)r.nb), dim3(RG_THREADS), 0, st, segcnt, r.nseg, bsum);
        hipLaunchKernelGGL(blocks_scan_top_kernel, dim3(1), dim3(RG_THREADS), 0, st, bsum, (int)r.nb);
        hipLaunchKernelGGL(blocks_table_kernel, dim3((unsigned)r.nb), dim3(RG_THREADS), 0, st, block_labels, w, r.nbx, segcnt, r.nseg, bsum, stats,
                           nmemb, max_regions, table, members);
    }
    return check_launch("text_blocks");
}
