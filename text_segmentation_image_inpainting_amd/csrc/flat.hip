// K13: flat regions (include/tsii_hip.h, "flat regions"): a text region whose surrounding ring of page pixels is of one colour within a
// tolerance is painted with the ring's mean colour and leaves the text plane; what is left of the plane, the 0 / 255 mask of the whole
// plane and the per-tile core counts come out of the same pass.  All integer (the channel sums in 64 bits): one defined answer, the same
// bits on every run.
//
//   1. init:   the statistics of all max_regions table rows (nothing in ws has to be cleared by the caller);
//   2. ring:   the ring walk of region_ring.h: a block owns RING_W x RING_H page pixels and stages, for them and an apron of `ring`
//              pixels, the table row of every text pixel (stage_rows); the dilated bit mask sends the great majority of non-text pixels
//              away after one test (near_bits); a non-text pixel next to text meets the rows of its (2 ring + 1)^2 window lowest first
//              (for_rows_in_window).  A thread keeps the statistics of the row it met last in registers, rows meet per block in a small
//              LDS hash table (a full table sends a thread's statistics to memory directly) and leave the block as one set of integer
//              atomics per (block, row);
//   3. decide: one thread per table row: flat or not, the rounded mean colour, the ring's pixel count -> `flat`;
//   4. apply:  a block owns a RING_W x RING_H rectangle of one tile core, a thread 4 consecutive pixels of a row: 12 page bytes and 4 text
//              bytes in, labels only where there is text; painted, text, mask out, one atomicAdd per block for the core count.
// No grid-wide barrier, no waiting on another block: each step is its own launch.  The count read from n_regions is clamped to
// max_regions and a row found by the search lies below it: a table that does not belong to the labels gives wrong bytes, never an
// access outside the buffers.  The boxes of the table are not read.
#include "region_ring.h"

namespace tsii {

constexpr int FL_RMAX = 8, FL_SW = RING_W + 2 * FL_RMAX, FL_SH = RING_H + 2 * FL_RMAX;      // the staged rectangle at the widest ring
constexpr int FL_HASH = 256, FL_PROBES = 8;      // rows per block in LDS; a thread that finds no slot in FL_PROBES steps goes to memory
constexpr int FL_STAT = 7;                       // n, lo r g b, hi r g b per table row

static inline bool flat_geometry(int h, int w, int max_regions) {
    return h >= 1 && w >= 1 && (int64_t)h * w <= (1ll << 31) - 2 && max_regions >= 1;
}
// ws: u64 sum[max_regions][3] | int stat[max_regions][FL_STAT]
static inline size_t flat_ws_bytes(int max_regions) { return (size_t)max_regions * (3 * sizeof(u64) + FL_STAT * sizeof(int)); }

// ---- 1. init ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RING_THREADS) void flat_init_kernel(int max_regions, u64* __restrict__ sum, int* __restrict__ stat) {
    const int r = blockIdx.x * RING_THREADS + threadIdx.x;
    if (r >= max_regions) return;
    sum[(int64_t)r * 3] = sum[(int64_t)r * 3 + 1] = sum[(int64_t)r * 3 + 2] = 0;
    int* s = stat + (int64_t)r * FL_STAT;
    s[0] = 0; s[1] = s[2] = s[3] = 255; s[4] = s[5] = s[6] = 0;
}

// ---- 2. ring statistics ------------------------------------------------------------------------------------------------------------
// what a thread knows of the table row it met last: the pixels of its column that lie in that row's ring
struct RingAcc {
    int row, n, lo[3], hi[3], sum[3];
};
__device__ __forceinline__ void acc_reset(RingAcc& a, int row) {
    a.row = row; a.n = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) { a.lo[c] = 255; a.hi[c] = 0; a.sum[c] = 0; }
}
__device__ __forceinline__ void stats_to_memory(int row, int n, int lo0, int lo1, int lo2, int hi0, int hi1, int hi2, int s0, int s1, int s2,
                                                u64* sum, int* stat) {
    int* s = stat + (int64_t)row * FL_STAT;
    atomicAdd(s, n);
    atomicMin(s + 1, lo0); atomicMin(s + 2, lo1); atomicMin(s + 3, lo2);
    atomicMax(s + 4, hi0); atomicMax(s + 5, hi1); atomicMax(s + 6, hi2);
    atomicAdd(sum + (int64_t)row * 3, (u64)s0); atomicAdd(sum + (int64_t)row * 3 + 1, (u64)s1); atomicAdd(sum + (int64_t)row * 3 + 2, (u64)s2);
}
// a block's sums stay below RING_W * RING_H * 255 < 2^31
__device__ __forceinline__ void acc_flush(const RingAcc& a, int* hkey, int* hn, int (*hlo)[FL_HASH], int (*hhi)[FL_HASH], int (*hsum)[FL_HASH],
                                          u64* sum, int* stat) {
    if (a.n == 0) return;
    unsigned slot = ((unsigned)a.row * 2654435761u) >> 24;        // 8 bits
    for (int probe = 0; probe < FL_PROBES; ++probe) {
        const int was = atomicCAS(hkey + slot, -1, a.row);
        if (was == -1 || was == a.row) {
            atomicAdd(hn + slot, a.n);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                atomicMin(&hlo[c][slot], a.lo[c]); atomicMax(&hhi[c][slot], a.hi[c]); atomicAdd(&hsum[c][slot], a.sum[c]);
            }
            return;
        }
        slot = (slot + 1) & (FL_HASH - 1);
    }
    stats_to_memory(a.row, a.n, a.lo[0], a.lo[1], a.lo[2], a.hi[0], a.hi[1], a.hi[2], a.sum[0], a.sum[1], a.sum[2], sum, stat);
}

__global__ __launch_bounds__(RING_THREADS) void flat_ring_kernel(const uint8_t* __restrict__ page, const uint8_t* __restrict__ text,
                                                                 const int* __restrict__ labels, int h, int w, int nbx,
                                                                 const int* __restrict__ table, const int* __restrict__ n_regions, int max_regions,
                                                                 int ring, u64* sum, int* stat) {
    __shared__ int idx[FL_SH * FL_SW];               // region_ring.h, stage_rows
    __shared__ u64 hrow[FL_SH], vnear[RING_H];       // region_ring.h, near_bits
    __shared__ int hkey[FL_HASH], hn[FL_HASH], hlo[3][FL_HASH], hhi[3][FL_HASH], hsum[3][FL_HASH];
    const int tid = threadIdx.x;
    const int x0 = (blockIdx.x % nbx) * RING_W, y0 = (blockIdx.x / nbx) * RING_H;
    const int R = clamp_count(n_regions[1], max_regions);
    const int sw = RING_W + 2 * ring, sh = RING_H + 2 * ring, span = 2 * ring;
    {
        hkey[tid] = -1; hn[tid] = 0;                 // FL_HASH == RING_THREADS
#pragma unroll
        for (int c = 0; c < 3; ++c) { hlo[c][tid] = 255; hhi[c][tid] = 0; hsum[c][tid] = 0; }
    }
    stage_rows(idx, sw, sh, x0, y0, ring, text, labels, h, w, table, R, tid);
    near_bits(idx, sw, sh, span, hrow, vnear, tid);
    RingAcc a;
    acc_reset(a, -1);
    const int c = tid & 63, x = x0 + c;
    if (x < w) {
        for (int k = 0, r = tid >> 6; k < RING_PER; ++k, r += 4) {
            const int y = y0 + r;                    // no page bytes are staged: a pixel is text when its own entry says so
            if (y >= h || !((vnear[r] >> c) & 1ull) || idx[(r + ring) * sw + c + ring] != NOTEXT) continue;
            const uint8_t* px = page + ((int64_t)y * w + x) * 3;
            const int v0 = px[0], v1 = px[1], v2 = px[2];
            for_rows_in_window(idx, sw, r, c, span, [&](int row) {
                if (row != a.row) {
                    acc_flush(a, hkey, hn, hlo, hhi, hsum, sum, stat);
                    acc_reset(a, row);
                }
                ++a.n;
                a.lo[0] = v0 < a.lo[0] ? v0 : a.lo[0]; a.lo[1] = v1 < a.lo[1] ? v1 : a.lo[1]; a.lo[2] = v2 < a.lo[2] ? v2 : a.lo[2];
                a.hi[0] = v0 > a.hi[0] ? v0 : a.hi[0]; a.hi[1] = v1 > a.hi[1] ? v1 : a.hi[1]; a.hi[2] = v2 > a.hi[2] ? v2 : a.hi[2];
                a.sum[0] += v0; a.sum[1] += v1; a.sum[2] += v2;
            });
        }
    }
    acc_flush(a, hkey, hn, hlo, hhi, hsum, sum, stat);
    __syncthreads();
    if (hkey[tid] >= 0)
        stats_to_memory(hkey[tid], hn[tid], hlo[0][tid], hlo[1][tid], hlo[2][tid], hhi[0][tid], hhi[1][tid], hhi[2][tid],
                        hsum[0][tid], hsum[1][tid], hsum[2][tid], sum, stat);
}

// ---- 3. decide -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RING_THREADS) void flat_decide_kernel(const int* __restrict__ n_regions, int max_regions, int tol,
                                                                   const u64* __restrict__ sum, const int* __restrict__ stat, int* __restrict__ flat) {
    const int r = blockIdx.x * RING_THREADS + threadIdx.x;
    if (r >= clamp_count(n_regions[1], max_regions)) return;
    const int* s = stat + (int64_t)r * FL_STAT;
    const int n = s[0];
    int* f = flat + (int64_t)r * 5;
    f[0] = (n >= 1 && s[4] - s[1] <= tol && s[5] - s[2] <= tol && s[6] - s[3] <= tol) ? 1 : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) f[1 + c] = n >= 1 ? (int)((2 * sum[(int64_t)r * 3 + c] + (u64)n) / (2 * (u64)n)) : 0;
    f[4] = n;
}

// ---- 4. apply ------------------------------------------------------------------------------------------------------------------
// thread tid owns pixels 4 (tid & 15) .. + 3 of rows (tid >> 4) and (tid >> 4) + 16 of the rectangle
__global__ __launch_bounds__(RING_THREADS) void flat_apply_kernel(const uint8_t* __restrict__ page, uint8_t* text, const int* __restrict__ labels,
                                                                  const int* __restrict__ table, const int* __restrict__ n_regions, int max_regions,
                                                                  const int* __restrict__ flat, PageGrid g, int nbx, int nby,
                                                                  uint8_t* __restrict__ painted, uint8_t* __restrict__ mask, int* __restrict__ core_count) {
    __shared__ int wave_count[RING_THREADS / 64];
    const int tid = threadIdx.x;
    const int t = blockIdx.x / (nbx * nby), sub = blockIdx.x % (nbx * nby);
    const int ci = t / g.tx, cj = t % g.tx;
    const int64_t y0 = (int64_t)ci * g.s + (sub / nbx) * RING_H, x0 = (int64_t)cj * g.s + (sub % nbx) * RING_W;
    const int64_t yend = (int64_t)(ci + 1) * g.s < g.h ? (int64_t)(ci + 1) * g.s : g.h, xend = (int64_t)(cj + 1) * g.s < g.w ? (int64_t)(cj + 1) * g.s : g.w;
    if (y0 >= yend || x0 >= xend) return;               // the whole block
    const int R = clamp_count(n_regions[1], max_regions);
    const int64_t xa = x0 + 4 * (tid & 15);
    int cnt = 0;
    if (xa < xend) {
        const int npx = xend - xa < 4 ? (int)(xend - xa) : 4;
        for (int row = tid >> 4; row < RING_H && y0 + row < yend; row += RING_THREADS / 16) {
            const int64_t p = (y0 + row) * g.w + xa;
            uint8_t b[12], t4[4], m4[4];
            if (npx == 4) {
                memcpy(b, page + p * 3, 12);
                memcpy(t4, text + p, 4);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int64_t q = k < npx ? p + k : p;
                    t4[k] = k < npx ? text[q] : 0;
                    b[3 * k] = page[q * 3]; b[3 * k + 1] = page[q * 3 + 1]; b[3 * k + 2] = page[q * 3 + 2];
                }
            }
            int last_lab = 0, last_row = NOROW;
            bool last_flat = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                m4[k] = t4[k] ? 255 : 0;
                if (t4[k] == 0) continue;
                const int lab = labels[p + k];
                if (lab != last_lab) {
                    last_lab = lab;
                    last_row = find_row(table, R, lab);
                    last_flat = last_row >= 0 && flat[(int64_t)last_row * 5] != 0;
                }
                if (last_flat) {
                    const int* f = flat + (int64_t)last_row * 5;
                    b[3 * k] = (uint8_t)f[1]; b[3 * k + 1] = (uint8_t)f[2]; b[3 * k + 2] = (uint8_t)f[3];
                    t4[k] = 0;
                } else {
                    t4[k] = 1;
                    ++cnt;
                }
            }
            if (npx == 4) {
                memcpy(painted + p * 3, b, 12);
                memcpy(text + p, t4, 4);
                if (mask != nullptr) memcpy(mask + p, m4, 4);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k < npx) {
                        painted[(p + k) * 3] = b[3 * k]; painted[(p + k) * 3 + 1] = b[3 * k + 1]; painted[(p + k) * 3 + 2] = b[3 * k + 2];
                        text[p + k] = t4[k];
                        if (mask != nullptr) mask[p + k] = m4[k];
                    }
                }
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

extern "C" size_t tsii_flat_regions_ws_bytes(int h, int w, int max_regions) {
    if (!flat_geometry(h, w, max_regions)) return 0;
    return flat_ws_bytes(max_regions);
}

extern "C" int tsii_flat_regions(const uint8_t* page, uint8_t* text, const int* labels, int h, int w, const int* table, const int* n_regions,
                                 int max_regions, int ring, int tol, int tile, int halo, int* core_count, uint8_t* painted, uint8_t* mask,
                                 int* flat, void* ws, void* stream) {
    TSII_REQUIRE(page && text && labels && table && n_regions && painted && flat && ws, "flat_regions: null pointer");
    TSII_REQUIRE(flat_geometry(h, w, max_regions), "flat_regions: page of %d x %d pixels, max_regions %d (h, w >= 1, h * w <= 2^31 - 2, max_regions >= 1)",
                 h, w, max_regions);
    TSII_REQUIRE(ring >= 1 && ring <= FL_RMAX, "flat_regions: ring %d (1..%d)", ring, FL_RMAX);
    TSII_REQUIRE(tol >= 0 && tol <= 255, "flat_regions: tol %d (0..255)", tol);
    TSII_REQUIRE(core_count == nullptr || grid_ok(h, w, tile, halo), "flat_regions: bad geometry h %d w %d tile %d halo %d", h, w, tile, halo);
    TSII_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, "flat_regions: ws must be 8-byte aligned");
    TSII_REQUIRE(painted != page, "flat_regions: painted must not be the page");
    const ApplyGrid a = make_apply_grid(h, w, tile, halo, core_count, RING_W, RING_H);
    const int rbx = cdiv(w, RING_W);
    const int64_t nring = (int64_t)rbx * cdiv(h, RING_H);
    TSII_REQUIRE(a.napply < (1ll << 31) && nring < (1ll << 31), "flat_regions: bad geometry h %d w %d tile %d halo %d (too many blocks)", h, w, tile, halo);
    hipStream_t st = (hipStream_t)stream;
    if (!clear_core_count(core_count, a.g, st)) return check_launch("flat_regions (memset)");
    u64* sum = static_cast<u64*>(ws);
    int* stat = reinterpret_cast<int*>(sum + 3 * (size_t)max_regions);
    const unsigned row_blocks = flat_grid(max_regions, RING_THREADS);
    hipLaunchKernelGGL(flat_init_kernel, dim3(row_blocks), dim3(RING_THREADS), 0, st, max_regions, sum, stat);
    hipLaunchKernelGGL(flat_ring_kernel, dim3((unsigned)nring), dim3(RING_THREADS), 0, st, page, text, labels, h, w, rbx, table, n_regions, max_regions,
                       ring, sum, stat);
    hipLaunchKernelGGL(flat_decide_kernel, dim3(row_blocks), dim3(RING_THREADS), 0, st, n_regions, max_regions, tol, sum, stat, flat);
    hipLaunchKernelGGL(flat_apply_kernel, dim3((unsigned)a.napply), dim3(RING_THREADS), 0, st, page, text, labels, table, n_regions, max_regions, flat,
                       a.g, a.nbx, a.nby, painted, mask, core_count);
    return check_launch("flat_regions");
}
