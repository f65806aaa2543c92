// K19: seeded regions (include/tsii_hip.h, "seeded regions"): the second half of a hysteresis threshold.  Behind tsii_text_regions or
// tsii_text_blocks, which cut the plane at the low probability, a table row is kept only if at least min_seeds of its pixels are set in a
// second plane, cut at the high one; the rows that are not leave the text plane, the label plane, the table and the core counts before
// anything else sees them.  All integer: one defined answer, the same bits on every run.
//
//   1. count:   a block of 256 threads owns RING_W x RING_H page pixels, a thread 4 consecutive pixels of two rows (16 label bytes and 4
//               seed bytes per load).  A thread merges the run of equal labels it walks through in registers and looks a run up -- the
//               binary search of region_ring.h -- only when it holds a seed; the run's seeds meet per block in SD_SLOTS rows of LDS (open
//               addressing by atomicCAS) and leave the block as one atomicAdd per (block, row).  A row that finds no slot (a block with
//               more than SD_SLOTS seeded rows) sends its runs to memory directly.
//   2. decide:  one block walks the table 256 rows at a time: a row is read into registers, judged, its old label and its verdict are left
//               in ws for the filter, and an exclusive scan of the verdicts gives the kept rows their new place.  A row only ever moves
//               towards the front, into places whose rows were read before the scan's first barrier: the move is safe in place.  The same
//               pass compacts members and seeds, counts what was dropped and lowers n_regions[1].  Where the table was cut (kept >
//               max_regions) the count that is left may still reach behind the rows that stay: the freed rows become EMPTY rows (label
//               INT_MAX: no pixel has it, and the column still ascends), which every later call finds nothing for and which this call
//               never judges, so that a second call changes nothing.
//   3. filter:  a block owns a RING_W x RING_H rectangle of one tile core, a thread 4 consecutive pixels of two rows: labels and text in,
//               the old row of a labelled pixel by binary search over the labels of ws, a store only where a quad lost a pixel, one
//               atomicAdd per block for the core count.
// No grid-wide barrier, no waiting on another block: each step is its own launch.  The count read from n_regions is clamped to
// max_regions and a row found by a search lies below it; nothing is indexed by a label: a table that does not belong to the labels gives
// wrong numbers, never an access outside the buffers.  The boxes of the table are not read.
#include "region_bits.h"
#include "region_ring.h"

namespace tsii {

constexpr int SD_SLOTS = 32;                         // seeded table rows a block keeps in LDS (tests/test_seeds_kernels.py holds a block with more)
constexpr int SD_META = 4;                           // ws behind the three columns: rows judged, rows dropped, two spare words

static inline bool seeds_geometry(int h, int w, int max_regions) {
    return h >= 1 && w >= 1 && (int64_t)h * w <= (1ll << 31) - 2 && max_regions >= 1;
}
// ws: int count[max_regions] | int old_label[max_regions] | int keep[max_regions] | int meta[SD_META]
static inline size_t seeds_ws_bytes(int max_regions) { return sizeof(int) * (3 * (size_t)max_regions + SD_META); }

// the index of lab in the ascending labels[0 .. R), NOROW without one: find_row of region_ring.h on a column of its own
__device__ __forceinline__ int find_label(const int* __restrict__ labels, int R, int lab) {
    int lo = 0, hi = R;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (labels[mid] < lab) lo = mid + 1; else hi = mid;
    }
    return (lo < R && labels[lo] == lab) ? lo : NOROW;
}

// ---- 1. count ----------------------------------------------------------------------------------------------------------------------
// the LDS slot of a table row (open addressing from row % SD_SLOTS), -1 when the block's table is full
__device__ __forceinline__ int sd_slot(int* key, int row) {
    for (int i = 0, s = row & (SD_SLOTS - 1); i < SD_SLOTS; ++i, s = (s + 1) & (SD_SLOTS - 1)) {
        const int was = atomicCAS(key + s, -1, row);
        if (was == -1 || was == row) return s;
    }
    return -1;
}
// a finished run of `n` seeds under one label: into the block's table, or to memory where that is full
__device__ __forceinline__ void flush_seeds(int* key, int* acc, int* count, const int* __restrict__ table, int R, int lab, int n) {
    if (n == 0 || lab == 0) return;
    const int row = find_row(table, R, lab);
    if (row < 0) return;
    const int slot = sd_slot(key, row);
    if (slot < 0) atomicAdd(count + row, n); else atomicAdd(acc + slot, n);
}

// thread tid owns pixels 4 (tid & 15) .. + 3 of rows (tid >> 4) and (tid >> 4) + 16 of the block's rectangle
__global__ __launch_bounds__(RING_THREADS) void seeds_count_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ seed, int h, int w, int nbx,
                                                                   const int* __restrict__ table, const int* __restrict__ n_regions, int max_regions,
                                                                   int* count) {
    __shared__ int key[SD_SLOTS], acc[SD_SLOTS];
    const int tid = threadIdx.x;
    const int64_t x0 = (int64_t)(blockIdx.x % nbx) * RING_W, y0 = (int64_t)(blockIdx.x / nbx) * RING_H;      // 64 bits: a page of one row may be 2^31 - 2 wide
    const int R = clamp_count(n_regions[1], max_regions);
    if (tid < SD_SLOTS) { key[tid] = -1; acc[tid] = 0; }
    __syncthreads();
    int run_lab = 0, run_n = 0;
    const int64_t xa = x0 + 4 * (tid & 15);
    if (xa < w && R > 0) {
        const int npx = w - xa < 4 ? (int)(w - xa) : 4;
        for (int r = tid >> 4; r < RING_H && y0 + r < h; r += RING_THREADS / 16) {
            const int64_t p = (y0 + r) * w + xa;
            uint8_t s4[4] = {0, 0, 0, 0};
            int l4[4] = {0, 0, 0, 0};
            if (npx == 4) {
                memcpy(s4, seed + p, 4);
                if (s4[0] | s4[1] | s4[2] | s4[3]) memcpy(l4, labels + p, 16);       // the great majority of quads holds no seed
            } else {
                for (int k = 0; k < npx; ++k) { s4[k] = seed[p + k]; l4[k] = labels[p + k]; }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (s4[k] == 0) continue;                // a pixel without a seed neither counts nor ends a run: only seeds are summed
                if (l4[k] != run_lab) {
                    flush_seeds(key, acc, count, table, R, run_lab, run_n);
                    run_lab = l4[k];
                    run_n = 0;
                }
                ++run_n;
            }
        }
    }
    flush_seeds(key, acc, count, table, R, run_lab, run_n);
    __syncthreads();
    if (tid < SD_SLOTS && key[tid] >= 0 && acc[tid] != 0) atomicAdd(count + key[tid], acc[tid]);
}

// ---- 2. decide, scan and compact ---------------------------------------------------------------------------------------------------
// one block.  Rows [k, R) of table, members and seeds are not written and keep what they held on entry -- unless the table was cut: then
// those rows of table and members become empty rows.
__global__ __launch_bounds__(RG_THREADS) void seeds_decide_kernel(int* table, int* members, int* n_regions, int max_regions, int min_seeds,
                                                                  const int* __restrict__ count, int* __restrict__ old_label, int* __restrict__ keep,
                                                                  int* __restrict__ meta, int* __restrict__ seeds, int* __restrict__ dropped) {
    __shared__ int sh[2 * RG_THREADS];
    __shared__ unsigned gone[2];                     // rows dropped, their summed area (unsigned: a foreign table may wrap it)
    const int tid = threadIdx.x;
    const int kept_in = n_regions[1];
    const int R = clamp_count(kept_in, max_regions);
    if (tid < 2) gone[tid] = 0;
    __syncthreads();                                 // every thread has read n_regions before thread 0 rewrites it
    int carry = 0;
    unsigned my_rows = 0, my_area = 0;
    for (int b0 = 0; b0 < R; b0 += RG_THREADS) {
        const int r = b0 + tid;
        const bool valid = r < R;
        int row[6] = {0, 0, 0, 0, 0, 0}, mem = 0, s = 0;
        if (valid) {
#pragma unroll
            for (int k = 0; k < 6; ++k) row[k] = table[(int64_t)r * 6 + k];
            if (members != nullptr) mem = members[r];
            s = count[r];
        }
        const bool stays = valid && (s >= min_seeds || row[0] == INT_MAX);       // an empty row is no region: never judged
        if (valid) {
            old_label[r] = row[0];
            keep[r] = stays ? 1 : 0;
            if (!stays) { ++my_rows; my_area += (unsigned)row[1]; }
        }
        int total;
        const int at = carry + block_excl_scan(stays ? 1 : 0, sh, tid, &total);     // its first barrier: every row of this stretch is in registers
        if (stays) {
#pragma unroll
            for (int k = 0; k < 6; ++k) table[(int64_t)at * 6 + k] = row[k];
            if (members != nullptr) members[at] = mem;
            if (row[0] != INT_MAX) seeds[at] = s;       // an empty row has no seeds entry
        }
        carry += total;
    }
    if (kept_in > max_regions) {                     // after the scan's last barrier: every row has been read and moved
        for (int r = carry + tid; r < R; r += RG_THREADS) {
            table[(int64_t)r * 6] = INT_MAX;
#pragma unroll
            for (int k = 1; k < 6; ++k) table[(int64_t)r * 6 + k] = 0;
            if (members != nullptr) members[r] = 0;
        }
    }
    if (my_rows) { atomicAdd(gone, my_rows); atomicAdd(gone + 1, my_area); }
    __syncthreads();
    if (tid == 0) {
        dropped[0] = (int)gone[0]; dropped[1] = (int)gone[1];
        n_regions[1] = kept_in - (int)gone[0];
        meta[0] = R; meta[1] = (int)gone[0]; meta[2] = 0; meta[3] = 0;
    }
}

// ---- 3. filter and count ---------------------------------------------------------------------------------------------------------
// thread tid owns pixels 4 (tid & 15) .. + 3 of rows (tid >> 4) and (tid >> 4) + 16 of the rectangle
__global__ __launch_bounds__(RING_THREADS) void seeds_filter_kernel(uint8_t* text, int* labels, const int* __restrict__ old_label,
                                                                    const int* __restrict__ keep, const int* __restrict__ meta, int max_regions,
                                                                    PageGrid g, int nbx, int nby, int* __restrict__ core_count) {
    __shared__ int wave_count[RING_THREADS / 64];
    const int tid = threadIdx.x;
    const int t = blockIdx.x / (nbx * nby), sub = blockIdx.x % (nbx * nby);
    const int ci = t / g.tx, cj = t % g.tx;
    const int64_t y0 = (int64_t)ci * g.s + (sub / nbx) * RING_H, x0 = (int64_t)cj * g.s + (sub % nbx) * RING_W;
    const int64_t yend = (int64_t)(ci + 1) * g.s < g.h ? (int64_t)(ci + 1) * g.s : g.h, xend = (int64_t)(cj + 1) * g.s < g.w ? (int64_t)(cj + 1) * g.s : g.w;
    if (y0 >= yend || x0 >= xend) return;               // the whole block
    const int R = clamp_count(meta[0], max_regions);
    const bool any_gone = meta[1] != 0;
    if (!any_gone && core_count == nullptr) return;     // nothing to rewrite and nothing to count: the whole grid
    const int64_t xa = x0 + 4 * (tid & 15);
    int cnt = 0;
    if (xa < xend) {
        const int npx = xend - xa < 4 ? (int)(xend - xa) : 4;
        for (int row = tid >> 4; row < RING_H && y0 + row < yend; row += RING_THREADS / 16) {
            const int64_t p = (y0 + row) * g.w + xa;
            uint8_t t4[4] = {0, 0, 0, 0};
            int l4[4] = {0, 0, 0, 0};
            if (npx == 4) {
                memcpy(t4, text + p, 4);
                if (any_gone) memcpy(l4, labels + p, 16);
            } else {
                for (int k = 0; k < npx; ++k) { t4[k] = text[p + k]; if (any_gone) l4[k] = labels[p + k]; }
            }
            int last_lab = 0;
            bool last_gone = false, changed = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k >= npx) continue;
                const int lab = l4[k];
                if (lab != 0) {
                    if (lab != last_lab) {
                        last_lab = lab;
                        const int r = find_label(old_label, R, lab);
                        last_gone = r >= 0 && keep[r] == 0;
                    }
                    if (last_gone) { l4[k] = 0; t4[k] = 0; changed = true; }
                }
                cnt += t4[k] != 0;
            }
            if (!changed) continue;
            if (npx == 4) {
                memcpy(labels + p, l4, 16);
                memcpy(text + p, t4, 4);
            } else {
                for (int k = 0; k < npx; ++k) { labels[p + k] = l4[k]; text[p + k] = t4[k]; }
            }
        }
    }
    if (core_count == nullptr) return;                  // the whole grid
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_down(cnt, d);
    if ((tid & 63) == 0) wave_count[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int k = 0; k < RING_THREADS / 64; ++k) total += wave_count[k];
        if (total > 0) atomicAdd(core_count + t, total);
    }
}

}  // namespace tsii

using namespace tsii;

extern "C" size_t tsii_region_seeds_ws_bytes(int h, int w, int max_regions) {
    if (!seeds_geometry(h, w, max_regions)) return 0;
    return seeds_ws_bytes(max_regions);
}

extern "C" int tsii_region_seeds(uint8_t* text, int* labels, const uint8_t* seed, int h, int w, int* table, int* n_regions, int max_regions,
                                 int min_seeds, int tile, int halo, int* core_count, int* seeds, int* members, int* dropped, void* ws,
                                 void* stream) {
    TSII_REQUIRE(text && labels && seed && table && n_regions && seeds && dropped && ws, "region_seeds: null pointer");
    TSII_REQUIRE(seeds_geometry(h, w, max_regions), "region_seeds: page of %d x %d pixels, max_regions %d (h, w >= 1, h * w <= 2^31 - 2, max_regions >= 1)",
                 h, w, max_regions);
    TSII_REQUIRE(min_seeds >= 1, "region_seeds: min_seeds %d (>= 1)", min_seeds);
    TSII_REQUIRE(core_count == nullptr || grid_ok(h, w, tile, halo), "region_seeds: bad geometry h %d w %d tile %d halo %d", h, w, tile, halo);
    TSII_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3u) == 0, "region_seeds: ws must be 4-byte aligned");
    TSII_REQUIRE(seed != text, "region_seeds: seed must not be the text plane");
    const ApplyGrid a = make_apply_grid(h, w, tile, halo, core_count, RING_W, RING_H);
    const int rbx = (int)cdiv64(w, RING_W);
    const int64_t ncount = (int64_t)rbx * cdiv64(h, RING_H);
    TSII_REQUIRE(a.napply < (1ll << 31) && ncount < (1ll << 31), "region_seeds: bad geometry h %d w %d tile %d halo %d (too many blocks)", h, w, tile, halo);
    hipStream_t st = (hipStream_t)stream;
    int* count = static_cast<int*>(ws);
    int* old_label = count + max_regions;
    int* keep = old_label + max_regions;
    int* meta = keep + max_regions;
    if (hipMemsetAsync(count, 0, sizeof(int) * (size_t)max_regions, st) != hipSuccess) return check_launch("region_seeds (memset)");
    if (!clear_core_count(core_count, a.g, st)) return check_launch("region_seeds (memset)");
    hipLaunchKernelGGL(seeds_count_kernel, dim3((unsigned)ncount), dim3(RING_THREADS), 0, st, labels, seed, h, w, rbx, table, n_regions, max_regions, count);
    hipLaunchKernelGGL(seeds_decide_kernel, dim3(1), dim3(RG_THREADS), 0, st, table, members, n_regions, max_regions, min_seeds, count, old_label, keep,
                       meta, seeds, dropped);
    hipLaunchKernelGGL(seeds_filter_kernel, dim3((unsigned)a.napply), dim3(RING_THREADS), 0, st, text, labels, old_label, keep, meta, max_regions, a.g,
                       a.nbx, a.nby, core_count);
    return check_launch("region_seeds");
}
