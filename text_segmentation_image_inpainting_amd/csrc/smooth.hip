// K16: smooth regions (include/tsii_hip.h, "smooth regions"): a text region whose surrounding ring of page pixels is locally smooth -- no
// non-text pixel of the ring differs from a non-text 4-neighbour by more than a tolerance -- is filled with the harmonic continuation of
// its surroundings at page level and leaves the text plane.  Two entry points on either side of tsii_harmonic_fill (K14), which runs
// unchanged between them: `classify` decides every table row and stages the solver's operands, `apply` writes the filled pixels of the
// smooth rows.  The decision is all integer: one defined answer, the same bits on every run.
//
//   classify 1. init:   the statistics of all max_regions table rows (nothing in ws has to be cleared by the caller);
//            2. stage:  x = byte / 255 and valid = (text == 0) over the whole page, 4 pixels and four 16-byte stores per thread;
//            3. ring:   the ring walk of region_ring.h with another statistic than K13's.  A block owns RING_W x RING_H page pixels and
//                       stages, for them and an apron of `ring` pixels, the table row of every text pixel (stage_rows), and, for them and
//                       an apron of ONE pixel, the page bytes of the non-text pixels (stage_pixels): the local step d of a pixel needs
//                       its 4-neighbours only, so what the block reads lies within ring + 1 of its rectangle.  d is computed once per
//                       pixel from LDS and goes to every row of the pixel's window (for_rows_in_window); rows meet per block in an LDS
//                       hash table and leave it as one set of integer atomics per (block, row) -- atomicAdd on n, atomicMax on the
//                       three steps, 32 bits all;
//            4. decide: one thread per table row -> `smooth`;
//   apply:   K13's apply kernel (csrc/flat.hip) with another paint: a block owns a RING_W x RING_H rectangle of one tile core, a thread 4
//            consecutive pixels of a row; `filled` is read on the text pixels of smooth rows only.
// No grid-wide barrier, no waiting on another block: each step is its own launch.  The count read from n_regions is clamped to max_regions
// and a row found by the search lies below it: a table that does not belong to the labels gives wrong bytes, never an access outside the
// buffers.  The boxes of the table are not read.
#include "region_ring.h"

namespace tsii {

constexpr int SM_RMAX = 8, SM_SW = RING_W + 2 * SM_RMAX, SM_SH = RING_H + 2 * SM_RMAX;   // the staged rectangle at the widest ring
constexpr int SM_PW = RING_W + 2, SM_PH = RING_H + 2;                                    // the staged page bytes: an apron of one pixel
constexpr int SM_HASH = 256, SM_PROBES = 8;      // rows per block in LDS; a thread that finds no slot in SM_PROBES steps goes to memory
constexpr int SM_STAT = 4;                       // n, step r g b per table row

static inline bool smooth_geometry(int h, int w, int max_regions) {
    return h >= 1 && w >= 1 && (int64_t)h * w * 3 <= (1ll << 31) && max_regions >= 1;
}

// ---- 1. init ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RING_THREADS) void smooth_init_kernel(int max_regions, int* __restrict__ stat) {
    const int64_t i = (int64_t)blockIdx.x * RING_THREADS + threadIdx.x;
    if (i < (int64_t)max_regions * SM_STAT) stat[i] = 0;
}

// ---- 2. the solver's operands --------------------------------------------------------------------------------------------------------
// thread i owns pixels 4 i .. 4 i + 3 of the page taken as one row of n pixels; vec: every pointer has the alignment of its vector
__global__ __launch_bounds__(RING_THREADS) void smooth_stage_kernel(const uint8_t* __restrict__ page, const uint8_t* __restrict__ text, int64_t n,
                                                                    int vec, float* __restrict__ x, float* __restrict__ valid) {
    const int64_t p = ((int64_t)blockIdx.x * RING_THREADS + threadIdx.x) * 4;
    if (p >= n) return;
    if (vec && p + 4 <= n) {
        uint8_t b[12], t4[4];
        memcpy(b, page + p * 3, 12);
        memcpy(t4, text + p, 4);
        float v[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) v[k] = (float)b[k] / 255.0f;
        float4* xo = reinterpret_cast<float4*>(x + p * 3);
        xo[0] = make_float4(v[0], v[1], v[2], v[3]);
        xo[1] = make_float4(v[4], v[5], v[6], v[7]);
        xo[2] = make_float4(v[8], v[9], v[10], v[11]);
        *reinterpret_cast<float4*>(valid + p) = make_float4(t4[0] ? 0.f : 1.f, t4[1] ? 0.f : 1.f, t4[2] ? 0.f : 1.f, t4[3] ? 0.f : 1.f);
        return;
    }
    for (int64_t q = p; q < p + 4 && q < n; ++q) {
        x[q * 3] = (float)page[q * 3] / 255.0f; x[q * 3 + 1] = (float)page[q * 3 + 1] / 255.0f; x[q * 3 + 2] = (float)page[q * 3 + 2] / 255.0f;
        valid[q] = text[q] ? 0.f : 1.f;
    }
}

// ---- 3. ring statistics ------------------------------------------------------------------------------------------------------------
// what a thread knows of the table row it met last: the pixels of its column that lie in that row's ring
struct StepAcc {
    int row, n, step[3];
};
__device__ __forceinline__ void sm_reset(StepAcc& a, int row) { a.row = row; a.n = 0; a.step[0] = a.step[1] = a.step[2] = 0; }
__device__ __forceinline__ void sm_to_memory(int row, int n, int s0, int s1, int s2, int* stat) {
    int* s = stat + (int64_t)row * SM_STAT;
    atomicAdd(s, n);
    atomicMax(s + 1, s0); atomicMax(s + 2, s1); atomicMax(s + 3, s2);
}
__device__ __forceinline__ void sm_flush(const StepAcc& a, int* hkey, int* hn, int (*hstep)[SM_HASH], int* stat) {
    if (a.n == 0) return;
    unsigned slot = ((unsigned)a.row * 2654435761u) >> 24;        // 8 bits
    for (int probe = 0; probe < SM_PROBES; ++probe) {
        const int was = atomicCAS(hkey + slot, -1, a.row);
        if (was == -1 || was == a.row) {
            atomicAdd(hn + slot, a.n);
#pragma unroll
            for (int c = 0; c < 3; ++c) atomicMax(&hstep[c][slot], a.step[c]);
            return;
        }
        slot = (slot + 1) & (SM_HASH - 1);
    }
    sm_to_memory(a.row, a.n, a.step[0], a.step[1], a.step[2], stat);
}

// |a - b| per byte of two staged pixels, the maximum with d so far
__device__ __forceinline__ void sm_step(int a, int b, int& d0, int& d1, int& d2) {
    if (b == NOPIX) return;
    int f0, f1, f2;
    abs_diff3(a, b, f0, f1, f2);
    d0 = f0 > d0 ? f0 : d0; d1 = f1 > d1 ? f1 : d1; d2 = f2 > d2 ? f2 : d2;
}

__global__ __launch_bounds__(RING_THREADS) void smooth_ring_kernel(const uint8_t* __restrict__ page, const uint8_t* __restrict__ text,
                                                                   const int* __restrict__ labels, int h, int w, int nbx,
                                                                   const int* __restrict__ table, const int* __restrict__ n_regions, int max_regions,
                                                                   int ring, int* stat) {
    __shared__ int idx[SM_SH * SM_SW];               // region_ring.h, stage_rows
    __shared__ int pix[SM_PH * SM_PW];               // region_ring.h, stage_pixels
    __shared__ u64 hrow[SM_SH], vnear[RING_H];       // region_ring.h, near_bits
    __shared__ int hkey[SM_HASH], hn[SM_HASH], hstep[3][SM_HASH];
    const int tid = threadIdx.x;
    const int x0 = (blockIdx.x % nbx) * RING_W, y0 = (blockIdx.x / nbx) * RING_H;
    const int R = clamp_count(n_regions[1], max_regions);
    const int sw = RING_W + 2 * ring, sh = RING_H + 2 * ring, span = 2 * ring;
    {
        hkey[tid] = -1; hn[tid] = 0;                 // SM_HASH == RING_THREADS
        hstep[0][tid] = hstep[1][tid] = hstep[2][tid] = 0;
    }
    stage_rows(idx, sw, sh, x0, y0, ring, text, labels, h, w, table, R, tid);
    stage_pixels(pix, SM_PW, SM_PH, x0 - 1, y0 - 1, page, text, h, w, tid);
    near_bits(idx, sw, sh, span, hrow, vnear, tid);
    StepAcc a;
    sm_reset(a, -1);
    const int c = tid & 63, x = x0 + c;
    if (x < w) {
        for (int k = 0, r = tid >> 6; k < RING_PER; ++k, r += 4) {
            const int y = y0 + r;
            if (y >= h || !((vnear[r] >> c) & 1ull)) continue;
            const int* pc = pix + (r + 1) * SM_PW + c + 1;
            const int me = pc[0];
            if (me == NOPIX) continue;               // text
            int d0 = 0, d1 = 0, d2 = 0;              // the local step: against the non-text 4-neighbours on the page
            sm_step(me, pc[-SM_PW], d0, d1, d2); sm_step(me, pc[SM_PW], d0, d1, d2);
            sm_step(me, pc[-1], d0, d1, d2); sm_step(me, pc[1], d0, d1, d2);
            for_rows_in_window(idx, sw, r, c, span, [&](int row) {
                if (row != a.row) {
                    sm_flush(a, hkey, hn, hstep, stat);
                    sm_reset(a, row);
                }
                ++a.n;
                a.step[0] = d0 > a.step[0] ? d0 : a.step[0]; a.step[1] = d1 > a.step[1] ? d1 : a.step[1];
                a.step[2] = d2 > a.step[2] ? d2 : a.step[2];
            });
        }
    }
    sm_flush(a, hkey, hn, hstep, stat);
    __syncthreads();
    if (hkey[tid] >= 0) sm_to_memory(hkey[tid], hn[tid], hstep[0][tid], hstep[1][tid], hstep[2][tid], stat);
}

// ---- 4. decide -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RING_THREADS) void smooth_decide_kernel(const int* __restrict__ n_regions, int max_regions, int tol,
                                                                     const int* __restrict__ stat, int* __restrict__ smooth) {
    const int r = blockIdx.x * RING_THREADS + threadIdx.x;
    if (r >= clamp_count(n_regions[1], max_regions)) return;
    const int* s = stat + (int64_t)r * SM_STAT;
    int* f = smooth + (int64_t)r * 5;
    f[0] = (s[0] >= 1 && s[1] <= tol && s[2] <= tol && s[3] <= tol) ? 1 : 0;
    f[1] = s[1]; f[2] = s[2]; f[3] = s[3];
    f[4] = s[0];
}

// ---- apply ---------------------------------------------------------------------------------------------------------------------
// floor(clamp(v, 0, 1) * 255 + 0.5) with the product and the sum rounded one after the other, as the host restatement computes it
__device__ __forceinline__ uint8_t sm_byte(float v) {
#pragma clang fp contract(off)
    const float cl = fminf(fmaxf(v, 0.f), 1.f);
    const float scaled = cl * 255.f;
    return (uint8_t)floorf(scaled + 0.5f);
}

// thread tid owns pixels 4 (tid & 15) .. + 3 of rows (tid >> 4) and (tid >> 4) + 16 of the rectangle
__global__ __launch_bounds__(RING_THREADS) void smooth_apply_kernel(const uint8_t* __restrict__ page, uint8_t* text, const int* __restrict__ labels,
                                                                    const int* __restrict__ table, const int* __restrict__ n_regions, int max_regions,
                                                                    const int* __restrict__ smooth, const float* __restrict__ filled, PageGrid g,
                                                                    int nbx, int nby, uint8_t* __restrict__ painted, uint8_t* __restrict__ mask,
                                                                    int* __restrict__ core_count) {
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
            int last_lab = 0;
            bool last_smooth = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                m4[k] = t4[k] ? 255 : 0;
                if (t4[k] == 0) continue;
                const int lab = labels[p + k];
                if (lab != last_lab) {
                    last_lab = lab;
                    const int found = find_row(table, R, lab);
                    last_smooth = found >= 0 && smooth[(int64_t)found * 5] != 0;
                }
                if (last_smooth) {
                    const float* f = filled + (p + k) * 3;
                    b[3 * k] = sm_byte(f[0]); b[3 * k + 1] = sm_byte(f[1]); b[3 * k + 2] = sm_byte(f[2]);
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

extern "C" size_t tsii_smooth_regions_ws_bytes(int h, int w, int max_regions) {
    if (!smooth_geometry(h, w, max_regions)) return 0;
    return (size_t)max_regions * SM_STAT * sizeof(int);
}

extern "C" int tsii_smooth_regions_classify(const uint8_t* page, const uint8_t* text, const int* labels, int h, int w, const int* table,
                                            const int* n_regions, int max_regions, int ring, int tol, int* smooth, float* x, float* valid,
                                            void* ws, void* stream) {
    TSII_REQUIRE(page && text && labels && table && n_regions && smooth && x && valid && ws, "smooth_regions_classify: null pointer");
    TSII_REQUIRE(smooth_geometry(h, w, max_regions),
                 "smooth_regions_classify: page of %d x %d pixels, max_regions %d (h, w >= 1, h * w * 3 <= 2^31, max_regions >= 1)", h, w, max_regions);
    TSII_REQUIRE(ring >= 1 && ring <= SM_RMAX, "smooth_regions_classify: ring %d (1..%d)", ring, SM_RMAX);
    TSII_REQUIRE(tol >= 0 && tol <= 255, "smooth_regions_classify: tol %d (0..255)", tol);
    TSII_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3u) == 0, "smooth_regions_classify: ws must be 4-byte aligned");
    const int rbx = cdiv(w, RING_W);
    const int64_t nring = (int64_t)rbx * cdiv(h, RING_H), n = (int64_t)h * w;
    TSII_REQUIRE(nring < (1ll << 31), "smooth_regions_classify: page of %d x %d pixels (too many blocks)", h, w);
    hipStream_t st = (hipStream_t)stream;
    int* stat = static_cast<int*>(ws);
    const int vec = aligned16(x) && aligned16(valid) && (reinterpret_cast<uintptr_t>(page) & 3u) == 0 && (reinterpret_cast<uintptr_t>(text) & 3u) == 0;
    hipLaunchKernelGGL(smooth_init_kernel, dim3(flat_grid((int64_t)max_regions * SM_STAT, RING_THREADS)), dim3(RING_THREADS), 0, st, max_regions, stat);
    hipLaunchKernelGGL(smooth_stage_kernel, dim3(flat_grid(cdiv64(n, 4), RING_THREADS)), dim3(RING_THREADS), 0, st, page, text, n, vec, x, valid);
    hipLaunchKernelGGL(smooth_ring_kernel, dim3((unsigned)nring), dim3(RING_THREADS), 0, st, page, text, labels, h, w, rbx, table, n_regions, max_regions,
                       ring, stat);
    hipLaunchKernelGGL(smooth_decide_kernel, dim3(flat_grid(max_regions, RING_THREADS)), dim3(RING_THREADS), 0, st, n_regions, max_regions, tol, stat, smooth);
    return check_launch("smooth_regions_classify");
}

extern "C" int tsii_smooth_regions_apply(const uint8_t* page, uint8_t* text, const int* labels, int h, int w, const int* table,
                                         const int* n_regions, int max_regions, const int* smooth, const float* filled, int tile, int halo,
                                         int* core_count, uint8_t* painted, uint8_t* mask, void* stream) {
    TSII_REQUIRE(page && text && labels && table && n_regions && smooth && filled && painted, "smooth_regions_apply: null pointer");
    TSII_REQUIRE(smooth_geometry(h, w, max_regions),
                 "smooth_regions_apply: page of %d x %d pixels, max_regions %d (h, w >= 1, h * w * 3 <= 2^31, max_regions >= 1)", h, w, max_regions);
    TSII_REQUIRE(core_count == nullptr || grid_ok(h, w, tile, halo), "smooth_regions_apply: bad geometry h %d w %d tile %d halo %d", h, w, tile, halo);
    TSII_REQUIRE(painted != page, "smooth_regions_apply: painted must not be the page");
    const ApplyGrid a = make_apply_grid(h, w, tile, halo, core_count, RING_W, RING_H);
    TSII_REQUIRE(a.napply < (1ll << 31), "smooth_regions_apply: bad geometry h %d w %d tile %d halo %d (too many blocks)", h, w, tile, halo);
    hipStream_t st = (hipStream_t)stream;
    if (!clear_core_count(core_count, a.g, st)) return check_launch("smooth_regions_apply (memset)");
    hipLaunchKernelGGL(smooth_apply_kernel, dim3((unsigned)a.napply), dim3(RING_THREADS), 0, st, page, text, labels, table, n_regions, max_regions, smooth,
                       filled, a.g, a.nbx, a.nby, painted, mask, core_count);
    return check_launch("smooth_regions_apply");
}
