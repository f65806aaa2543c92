// K18: page scores (include/tsii_hip.h, "page scores"): what TextEraser did to a page, measured against the same page cleaned by hand.
// Two entry points, all in integers: one defined answer, the same bits on every run.
//
//   tsii_pair_text_mask: the text mask the reference's Dataloader derives from a (raw, clean) pair -- |L(raw) - L(clean)| > thr, grown by a
//       k x k square whose anchor is k / 2 (even k: the square reaches one pixel further up and left than down and right).  One kernel: a
//       block of 256 threads owns RING_W x RING_H pixels and stages the thresholded bit of them and of an apron of k - 1 pixels in LDS (the
//       plane exists nowhere else); one thread per staged row packs it into bits and ORs k shifts of them (the row maximum), one thread
//       per owned row ORs k of those (the column maximum): the construction of near_bits in region_ring.h.
//   tsii_page_scores: one pass over out, clean, mask, truth and labels.  A block owns RING_W x RING_H pixels, a thread 4 consecutive pixels
//       of two rows (12 page bytes per load, as the apply kernels of K13 / K16 / K17 read them).
//       page sums: a block's sums fit 32 bits (2048 pixels x 3 x 255^2 < 2^29): reduced in the wave by shuffles, across the waves in LDS, and
//           left as 12 words per block in ws; a second launch of one block adds them up in 64 bits.  No atomics, no contended address: a
//           page of 1170 x 1654 pixels would otherwise send 962 blocks to the same 12 words.
//       row sums: a thread merges the run of equal labels it walks through in registers, finds the table row of a run by the binary search
//           of region_ring.h, and adds the run to the block's table in LDS: SC_SLOTS rows, open addressing by atomicCAS.  At its end a
//           block leaves three 64-bit atomicAdd and one 32-bit atomicMax per row it met -- one set per (block, row), spread over the rows.
//           A row that finds no slot (a block with more than SC_SLOTS distinct rows) sends its runs to memory directly.
// A row found by the search lies below n_rows and nothing is indexed by a label: a table that does not belong to the labels gives wrong
// numbers, never an access outside the buffers.
#include "region_ring.h"

namespace tsii {

// ---- the pair's text mask ------------------------------------------------------------------------------------------------------------
constexpr int PM_KMAX = 31, PM_SW = RING_W + PM_KMAX - 1, PM_SH = RING_H + PM_KMAX - 1;

// Pillow's convert("L"): ITU-R 601-2 in 16-bit fixed point, rounded
__device__ __forceinline__ int luma(const uint8_t* __restrict__ page, int64_t p) {
    return (19595 * (int)page[p * 3] + 38470 * (int)page[p * 3 + 1] + 7471 * (int)page[p * 3 + 2] + 32768) >> 16;
}

__global__ __launch_bounds__(RING_THREADS) void pair_text_mask_kernel(const uint8_t* __restrict__ raw, const uint8_t* __restrict__ clean, int h,
                                                                      int w, int nbx, int thr, int k, uint8_t* __restrict__ truth) {
    __shared__ uint8_t bit[PM_SH * PM_SW];           // t of the block's pixels and their apron: sh rows of sw
    __shared__ u64 hrow[PM_SH], vany[RING_H];
    const int tid = threadIdx.x;
    const int64_t x0 = (int64_t)(blockIdx.x % nbx) * RING_W, y0 = (int64_t)(blockIdx.x / nbx) * RING_H;      // 64 bits: a page of one row may be 2^31 - 2 wide
    const int before = k / 2, span = k - 1, sw = RING_W + span, sh = RING_H + span;
    for (int j = tid; j < sh * sw; j += RING_THREADS) {
        const int sr = j / sw, sc = j - sr * sw;
        const int64_t y = y0 - before + sr, x = x0 - before + sc;
        uint8_t v = 0;
        if (y >= 0 && y < h && x >= 0 && x < w) {
            const int64_t p = y * w + x;
            const int d = luma(raw, p) - luma(clean, p);
            v = (d < 0 ? -d : d) > thr ? 1 : 0;
        }
        bit[j] = v;
    }
    __syncthreads();
    if (tid < sh) {                                  // one staged row per thread: bit c = some t in staged columns c .. c + span
        u64 lo = 0, hi = 0;
        const uint8_t* s = bit + tid * sw;
        for (int c = 0; c < sw; ++c) {
            const u64 b = s[c];
            if (c < 64) lo |= b << c; else hi |= b << (c - 64);
        }
        u64 acc = lo;
        for (int d = 1; d <= span; ++d) acc |= (lo >> d) | (hi << (64 - d));
        hrow[tid] = acc;
    }
    __syncthreads();
    if (tid < RING_H) {
        u64 acc = 0;
        for (int d = 0; d <= span; ++d) acc |= hrow[tid + d];
        vany[tid] = acc;
    }
    __syncthreads();
    const int c = tid & 63;
    const int64_t x = x0 + c;
    if (x >= w) return;
    for (int r = tid >> 6; r < RING_H && y0 + r < h; r += RING_THREADS / 64)
        truth[(y0 + r) * w + x] = ((vany[r] >> c) & 1ull) ? 255 : 0;
}

// ---- the scores --------------------------------------------------------------------------------------------------------------------
constexpr int SC_PAGE = 12;                          // the words of `page`
constexpr int SC_SLOTS = 32;                         // table rows a block keeps in LDS (tests/test_score_kernels.py holds a block with more)
constexpr int SC_WAVES = RING_THREADS / 64;

static inline bool score_geometry(int h, int w) { return h >= 1 && w >= 1 && (int64_t)h * w <= (1ll << 31) - 2; }
static inline int64_t score_blocks(int h, int w) { return cdiv64(w, RING_W) * cdiv64(h, RING_H); }
// ws: int part[blocks][SC_PAGE]
static inline size_t score_ws_bytes(int h, int w) { return (size_t)score_blocks(h, w) * SC_PAGE * sizeof(int); }

// pixels, sum a, sum s, max m of a set of pixels
struct Err4 {
    int n, a, s, m;
};
__device__ __forceinline__ void err_add(Err4& e, int a, int s, int m) { e.n += 1; e.a += a; e.s += s; e.m = m > e.m ? m : e.m; }

// the LDS slot of a table row (open addressing from row % SC_SLOTS), -1 when the block's table is full
__device__ __forceinline__ int sc_slot(int* key, int row) {
    for (int i = 0, s = row & (SC_SLOTS - 1); i < SC_SLOTS; ++i, s = (s + 1) & (SC_SLOTS - 1)) {
        const int was = atomicCAS(key + s, -1, row);
        if (was == -1 || was == row) return s;
    }
    return -1;
}

__device__ __forceinline__ void row_to_memory(int64_t* rows, int row, const Err4& e) {
    u64* g = reinterpret_cast<u64*>(rows + (int64_t)row * 4);
    atomicAdd(g, (u64)e.n); atomicAdd(g + 1, (u64)e.a); atomicAdd(g + 2, (u64)e.s);
    if (e.m > 0) atomicMax(reinterpret_cast<int*>(g + 3), e.m);          // the low word of a little-endian int64 whose high word is 0
}

// a finished run of one table row: into the block's table, or to memory where that is full
__device__ __forceinline__ void flush_run(int* key, int* acc, int64_t* rows, int row, int& slot_row, int& slot, const Err4& e) {
    if (row < 0 || e.n == 0) return;
    if (row != slot_row) { slot_row = row; slot = sc_slot(key, row); }
    if (slot < 0) { row_to_memory(rows, row, e); return; }
    int* a = acc + slot * 4;
    atomicAdd(a, e.n); atomicAdd(a + 1, e.a); atomicAdd(a + 2, e.s);
    if (e.m > 0) atomicMax(a + 3, e.m);
}

// thread tid owns pixels 4 (tid & 15) .. + 3 of rows (tid >> 4) and (tid >> 4) + 16 of the block's rectangle
__global__ __launch_bounds__(RING_THREADS) void page_scores_kernel(const uint8_t* __restrict__ out, const uint8_t* __restrict__ clean,
                                                                   const uint8_t* __restrict__ mask, const uint8_t* __restrict__ truth,
                                                                   const int* __restrict__ labels, const int* __restrict__ table, int n_rows, int h,
                                                                   int w, int nbx, int* __restrict__ part, int64_t* rows) {
    __shared__ int wave_part[SC_WAVES][SC_PAGE];
    __shared__ int key[SC_SLOTS], acc[SC_SLOTS * 4];
    const int tid = threadIdx.x;
    const int64_t x0 = (int64_t)(blockIdx.x % nbx) * RING_W, y0 = (int64_t)(blockIdx.x / nbx) * RING_H;
    const bool by_row = labels != nullptr && n_rows > 0;
    if (by_row) {
        if (tid < SC_SLOTS) key[tid] = -1;
        if (tid < SC_SLOTS * 4) acc[tid] = 0;
        __syncthreads();
    }
    int tp = 0, fp = 0, fn = 0, tn = 0;
    Err4 fill = {0, 0, 0, 0}, left = {0, 0, 0, 0}, run = {0, 0, 0, 0};
    int run_lab = 0, run_row = NOROW, slot_row = NOROW, slot = -1;
    const int64_t xa = x0 + 4 * (tid & 15);
    if (xa < w) {
        const int npx = w - xa < 4 ? (int)(w - xa) : 4;
        for (int r = tid >> 4; r < RING_H && y0 + r < h; r += RING_THREADS / 16) {
            const int64_t p = (y0 + r) * w + xa;
            uint8_t o[12], c[12], m4[4], t4[4];
            int l4[4] = {0, 0, 0, 0};
            if (npx == 4) {
                memcpy(o, out + p * 3, 12);
                memcpy(c, clean + p * 3, 12);
                memcpy(m4, mask + p, 4);
                memcpy(t4, truth + p, 4);
                if (by_row) memcpy(l4, labels + p, 16);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int64_t q = k < npx ? p + k : p;
                    m4[k] = mask[q]; t4[k] = truth[q];
                    if (by_row) l4[k] = labels[q];
                    o[3 * k] = out[q * 3]; o[3 * k + 1] = out[q * 3 + 1]; o[3 * k + 2] = out[q * 3 + 2];
                    c[3 * k] = clean[q * 3]; c[3 * k + 1] = clean[q * 3 + 1]; c[3 * k + 2] = clean[q * 3 + 2];
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k >= npx) continue;
                int d0 = (int)o[3 * k] - (int)c[3 * k], d1 = (int)o[3 * k + 1] - (int)c[3 * k + 1], d2 = (int)o[3 * k + 2] - (int)c[3 * k + 2];
                d0 = d0 < 0 ? -d0 : d0; d1 = d1 < 0 ? -d1 : d1; d2 = d2 < 0 ? -d2 : d2;
                const int a = d0 + d1 + d2, s = d0 * d0 + d1 * d1 + d2 * d2, m01 = d0 > d1 ? d0 : d1, m = m01 > d2 ? m01 : d2;
                const bool is_mask = m4[k] != 0, is_truth = t4[k] != 0;
                tp += is_mask && is_truth; fp += is_mask && !is_truth; fn += !is_mask && is_truth; tn += !is_mask && !is_truth;
                if (is_mask) err_add(fill, a, s, m); else err_add(left, a, s, m);
                if (!by_row) continue;
                const int lab = l4[k];
                if (lab != run_lab) {                // the run ends: labels of one region are mostly neighbours
                    flush_run(key, acc, rows, run_row, slot_row, slot, run);
                    run = {0, 0, 0, 0};
                    run_lab = lab;
                    run_row = lab != 0 ? find_row(table, n_rows, lab) : NOROW;
                }
                if (run_row >= 0) err_add(run, a, s, m);
            }
        }
    }
    if (by_row) flush_run(key, acc, rows, run_row, slot_row, slot, run);
    // the page sums of the block: in the wave, then across the waves
    int v[SC_PAGE] = {tp, fp, fn, tn, fill.n, fill.a, fill.s, fill.m, left.n, left.a, left.s, left.m};
#pragma unroll
    for (int i = 0; i < SC_PAGE; ++i) {
        const bool is_max = (i == 7 || i == 11);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const int other = __shfl_down(v[i], d);
            v[i] = is_max ? (other > v[i] ? other : v[i]) : v[i] + other;
        }
        if ((tid & 63) == 0) wave_part[tid >> 6][i] = v[i];
    }
    __syncthreads();
    if (tid < SC_PAGE) {
        const bool is_max = (tid == 7 || tid == 11);
        int total = wave_part[0][tid];
        for (int k = 1; k < SC_WAVES; ++k) total = is_max ? (wave_part[k][tid] > total ? wave_part[k][tid] : total) : total + wave_part[k][tid];
        part[(int64_t)blockIdx.x * SC_PAGE + tid] = total;
    }
    if (by_row && tid < SC_SLOTS && key[tid] >= 0) { // after the barrier above: every run of the block is in the table
        const Err4 e = {acc[tid * 4], acc[tid * 4 + 1], acc[tid * 4 + 2], acc[tid * 4 + 3]};
        row_to_memory(rows, key[tid], e);
    }
}

// one block: page[i] = the sum (i = 7, 11: the maximum) of part[b][i] over the blocks, in 64 bits
__global__ __launch_bounds__(RING_THREADS) void page_scores_finish_kernel(const int* __restrict__ part, int64_t nblocks, int64_t* __restrict__ page) {
    __shared__ int64_t wave_sum64[SC_WAVES][SC_PAGE];
    const int tid = threadIdx.x;
    int64_t v[SC_PAGE];
#pragma unroll
    for (int i = 0; i < SC_PAGE; ++i) v[i] = 0;
    for (int64_t b = tid; b < nblocks; b += RING_THREADS) {
#pragma unroll
        for (int i = 0; i < SC_PAGE; ++i) {
            const int64_t x = part[b * SC_PAGE + i];
            v[i] = (i == 7 || i == 11) ? (x > v[i] ? x : v[i]) : v[i] + x;
        }
    }
#pragma unroll
    for (int i = 0; i < SC_PAGE; ++i) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {           // 64 bits as two 32-bit shuffles
            const unsigned lo = __shfl_down((unsigned)(v[i] & 0xffffffffll), d), hi = __shfl_down((unsigned)((u64)v[i] >> 32), d);
            const int64_t other = (int64_t)(((u64)hi << 32) | lo);
            v[i] = (i == 7 || i == 11) ? (other > v[i] ? other : v[i]) : v[i] + other;
        }
        if ((tid & 63) == 0) wave_sum64[tid >> 6][i] = v[i];
    }
    __syncthreads();
    if (tid < SC_PAGE) {
        int64_t total = wave_sum64[0][tid];
        for (int k = 1; k < SC_WAVES; ++k) total = (tid == 7 || tid == 11) ? (wave_sum64[k][tid] > total ? wave_sum64[k][tid] : total) : total + wave_sum64[k][tid];
        page[tid] = total;
    }
}

}  // namespace tsii

using namespace tsii;

extern "C" int tsii_pair_text_mask(const uint8_t* raw, const uint8_t* clean, int h, int w, int thr, int k, uint8_t* truth, void* stream) {
    TSII_REQUIRE(raw && clean && truth, "pair_text_mask: null pointer");
    TSII_REQUIRE(score_geometry(h, w), "pair_text_mask: page of %d x %d pixels (h, w >= 1, h * w <= 2^31 - 2)", h, w);
    TSII_REQUIRE(thr >= 0 && thr <= 255, "pair_text_mask: thr %d (0..255)", thr);
    TSII_REQUIRE(k >= 1 && k <= PM_KMAX, "pair_text_mask: k %d (1..%d)", k, PM_KMAX);
    TSII_REQUIRE(truth != raw && truth != clean, "pair_text_mask: truth must not be one of the pages");
    const int64_t nb = score_blocks(h, w);
    hipLaunchKernelGGL(pair_text_mask_kernel, dim3((unsigned)nb), dim3(RING_THREADS), 0, (hipStream_t)stream, raw, clean, h, w,
                       (int)cdiv64(w, RING_W), thr, k, truth);
    return check_launch("pair_text_mask");
}

extern "C" size_t tsii_page_scores_ws_bytes(int h, int w, int max_rows) {
    if (!score_geometry(h, w) || max_rows < 0) return 0;
    return score_ws_bytes(h, w);
}

extern "C" int tsii_page_scores(const uint8_t* out, const uint8_t* clean, const uint8_t* mask, const uint8_t* truth, const int* labels,
                                const int* table, int n_rows, int h, int w, int64_t* page, int64_t* rows, void* ws, size_t ws_bytes,
                                void* stream) {
    TSII_REQUIRE(out && clean && mask && truth && page && ws, "page_scores: null pointer");
    TSII_REQUIRE(score_geometry(h, w), "page_scores: page of %d x %d pixels (h, w >= 1, h * w <= 2^31 - 2)", h, w);
    TSII_REQUIRE(n_rows >= 0, "page_scores: n_rows %d", n_rows);
    const bool by_row = labels != nullptr && n_rows > 0;
    TSII_REQUIRE(!by_row || (table && rows), "page_scores: labels and n_rows %d without table or rows", n_rows);
    TSII_REQUIRE(ws_bytes >= score_ws_bytes(h, w), "page_scores: workspace too small");
    TSII_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3u) == 0 && (reinterpret_cast<uintptr_t>(page) & 7u) == 0 &&
                 (!by_row || (reinterpret_cast<uintptr_t>(rows) & 7u) == 0), "page_scores: ws must be 4-byte, page and rows 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (by_row && hipMemsetAsync(rows, 0, sizeof(int64_t) * 4 * (size_t)n_rows, st) != hipSuccess) return check_launch("page_scores (memset)");
    const int64_t nb = score_blocks(h, w);
    int* part = static_cast<int*>(ws);
    hipLaunchKernelGGL(page_scores_kernel, dim3((unsigned)nb), dim3(RING_THREADS), 0, st, out, clean, mask, truth, labels, table, n_rows, h, w,
                       (int)cdiv64(w, RING_W), part, rows);
    hipLaunchKernelGGL(page_scores_finish_kernel, dim3(1), dim3(RING_THREADS), 0, st, part, nb, page);
    return check_launch("page_scores");
}
