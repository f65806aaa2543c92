// K17: tone regions (include/tsii_hip.h, "tone regions"): a text region whose surrounding ring of page pixels is a periodic pattern --
// screentone, stripes, a dot lattice -- is filled by copying, for every text pixel, the nearest non-text pixel a whole number of periods
// away, and leaves the text plane.  The period is one integer shift per region, measured on the ring: the shift under which the ring
// matches the page best.  All in 32-bit integers with atomicAdd and atomicMax: one defined answer, the same bits on every run.
//
//   1. init:   the statistics of the table rows in use (nothing in ws has to be cleared by the caller);
//   2. ring:   the ring walk of region_ring.h with another statistic than K13's.  A block owns RING_W x RING_H page pixels and stages, for
//              them and an apron of `ring` pixels, the table row of every text pixel (stage_rows); a block with no text within `ring`
//              (near_bits) leaves there.  The others stage, for their pixels and an apron of `period` pixels to the left, to the right
//              and below, the page bytes of the non-text pixels (stage_pixels).  The shifts (dy 0..period, dx -period..period) are cut
//              into chunks of TN_CHUNK over blockIdx.z; a block keeps cnt and err of (row, shift) for up to TN_SLOTS rows in LDS and
//              leaves one pair of atomics per (block, row, shift) with a pair; rows beyond TN_SLOTS go to memory directly.  The lanes of
//              a wave walk the chunk rotated by their lane number, so that 64 pixels of one row do not meet at one LDS word;
//   3. decide: one thread per table row: step, the best shift by the key (err, dy^2 + dx^2, dy, dx) -> `tone` (the flag still without the
//              source check);
//   4. source: one thread per page pixel; a text pixel of a row with a flag walks p + s, p - s, p + 2 s, ... to its first non-text pixel
//              and notes it in ws; without one within TN_WALK steps each way the row's flag is taken back (the first such pixel of a row,
//              by atomicMax on a word of ws, takes it back with one atomicAdd);
//   5. apply:  K13's apply kernel (csrc/flat.hip) with another paint: a block owns a RING_W x RING_H rectangle of one tile core, a thread 4
//              consecutive pixels of a row; the noted source is read on the text pixels of tone rows only.
// No grid-wide barrier, no waiting on another block: each step is its own launch.  The count read from n_regions is clamped to max_regions
// and a row found by the search lies below it; a noted source is always a pixel of the page: a table that does not belong to the labels
// gives wrong bytes, never an access outside the buffers.  The boxes of the table are not read.
#include "region_ring.h"

namespace tsii {

constexpr int TN_RMAX = 16, TN_SW = RING_W + 2 * TN_RMAX, TN_SH = RING_H + 2 * TN_RMAX;  // the staged rows at the widest ring
constexpr int TN_PMAX = 16, TN_PW = RING_W + 2 * TN_PMAX, TN_PH = RING_H + TN_PMAX;      // the staged page bytes at the longest period
constexpr int TN_SLOTS = 16, TN_CHUNK = 128;     // table rows per block in LDS (a row that finds no slot goes to memory); shifts per block
constexpr int TN_WALK = 256;                     // steps each way of the source walk
constexpr int TN_NOSHIFT = INT_MIN;              // staged shift offsets: not a shift of S (or behind its end)

static inline int tone_shifts(int period) { return (period + 1) * (2 * period + 1); }    // dy 0..period, dx -period..period, row-major
static inline bool tone_geometry(int h, int w, int max_regions, int period) {
    return h >= 1 && w >= 1 && (int64_t)h * w * 3 <= (1ll << 31) && max_regions >= 1 && period >= 2 && period <= TN_PMAX &&
           (int64_t)max_regions * tone_shifts(period) * 2 < (1ll << 31);
}
// ws: int stat[max_regions][shifts][2] (cnt, err) | ringn[max_regions] | cand[max_regions] | nosrc[max_regions] | src[h * w]
static inline size_t tone_ws_bytes(int h, int w, int max_regions, int period) {
    return ((size_t)max_regions * ((size_t)tone_shifts(period) * 2 + 3) + (size_t)h * w) * sizeof(int);
}

// ---- 1. init ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RING_THREADS) void tone_init_kernel(const int* __restrict__ n_regions, int max_regions, int shifts,
                                                                 int* __restrict__ stat, int* __restrict__ small) {
    const int64_t i = (int64_t)blockIdx.x * RING_THREADS + threadIdx.x;
    const int R = clamp_count(n_regions[1], max_regions);
    if (i < (int64_t)R * shifts * 2) stat[i] = 0;
    if (i < (int64_t)R) small[i] = small[i + max_regions] = small[i + 2 * (int64_t)max_regions] = 0;
}

// ---- 2. ring statistics ------------------------------------------------------------------------------------------------------------
// the LDS slot of a table row, -1 when the block's table is full
__device__ __forceinline__ int tn_slot(int* hkey, int row) {
    for (int s = 0; s < TN_SLOTS; ++s) {
        const int was = atomicCAS(hkey + s, -1, row);
        if (was == -1 || was == row) return s;
    }
    return -1;
}

// the largest |a - b| over the three bytes of two staged pixels
__device__ __forceinline__ int tn_diff(int a, int b) {
    int f0, f1, f2;
    abs_diff3(a, b, f0, f1, f2);
    const int m = f0 > f1 ? f0 : f1;
    return m > f2 ? m : f2;
}

__global__ __launch_bounds__(RING_THREADS) void tone_ring_kernel(const uint8_t* __restrict__ page, const uint8_t* __restrict__ text,
                                                                 const int* __restrict__ labels, int h, int w, int nbx,
                                                                 const int* __restrict__ table, const int* __restrict__ n_regions, int max_regions,
                                                                 int ring, int period, int shifts, int* stat, int* ringn) {
    __shared__ int idx[TN_SH * TN_SW];               // region_ring.h, stage_rows
    __shared__ int pix[TN_PH * TN_PW];               // region_ring.h, stage_pixels: rows of pw = RING_W + 2 period entries
    __shared__ u64 hrow[TN_SH], vnear[RING_H];       // region_ring.h, near_bits
    __shared__ int hkey[TN_SLOTS], hn[TN_SLOTS];
    __shared__ int acnt[TN_SLOTS * TN_CHUNK], aerr[TN_SLOTS * TN_CHUNK];
    __shared__ int soff[TN_CHUNK];                   // the chunk's shifts as offsets into pix
    const int tid = threadIdx.x;
    const int x0 = (blockIdx.x % nbx) * RING_W, y0 = (blockIdx.x / nbx) * RING_H;
    const int k0 = blockIdx.z * TN_CHUNK;            // the first shift of this block's chunk
    const int R = clamp_count(n_regions[1], max_regions);
    const int sw = RING_W + 2 * ring, sh = RING_H + 2 * ring, span = 2 * ring;
    const int pw = RING_W + 2 * period, ph = RING_H + period, dxs = 2 * period + 1;
    stage_rows(idx, sw, sh, x0, y0, ring, text, labels, h, w, table, R, tid);
    near_bits(idx, sw, sh, span, hrow, vnear, tid);
    u64 any = 0;
    for (int r = 0; r < RING_H; ++r) any |= vnear[r];
    if (any == 0) return;                            // the whole block: no table row within `ring` of its pixels
    stage_pixels(pix, pw, ph, x0 - period, y0, page, text, h, w, tid);
    for (int j = tid; j < TN_SLOTS * TN_CHUNK; j += RING_THREADS) acnt[j] = aerr[j] = 0;
    if (tid < TN_SLOTS) { hkey[tid] = -1; hn[tid] = 0; }
    if (tid < TN_CHUNK) {
        const int k = k0 + tid, dy = k / dxs, dx = k - dy * dxs - period;
        soff[tid] = (k < shifts && (dy > 0 || dx > 0)) ? dy * pw + dx : TN_NOSHIFT;
    }
    __syncthreads();
    const int c = tid & 63, x = x0 + c;
    int last_row = -1, last_slot = -1;
    if (x < w) {
        for (int k = 0, r = tid >> 6; k < RING_PER; ++k, r += 4) {
            const int y = y0 + r;
            if (y >= h || !((vnear[r] >> c) & 1ull)) continue;
            const int* pc = pix + r * pw + c + period;
            const int me = pc[0];
            if (me == NOPIX) continue;               // text
            for_rows_in_window(idx, sw, r, c, span, [&](int row) {
                if (row != last_row) { last_row = row; last_slot = tn_slot(hkey, row); }
                if (blockIdx.z == 0) {               // n_r: by the blocks of the first chunk
                    if (last_slot >= 0) atomicAdd(hn + last_slot, 1);
                    else atomicAdd(ringn + row, 1);
                }
                int* gs = stat + ((int64_t)row * shifts + k0) * 2;
                for (int i = 0; i < TN_CHUNK; ++i) {
                    const int j = (i + c) & (TN_CHUNK - 1);
                    const int off = soff[j];
                    if (off == TN_NOSHIFT) continue;
                    const int other = pc[off];
                    if (other == NOPIX) continue;
                    const int e = tn_diff(me, other);
                    if (last_slot >= 0) {
                        atomicAdd(acnt + last_slot * TN_CHUNK + j, 1);
                        if (e > 0) atomicMax(aerr + last_slot * TN_CHUNK + j, e);
                    } else {
                        atomicAdd(gs + 2 * j, 1);
                        if (e > 0) atomicMax(gs + 2 * j + 1, e);
                    }
                }
            });
        }
    }
    __syncthreads();
    if (tid < TN_SLOTS && hn[tid] > 0) atomicAdd(ringn + hkey[tid], hn[tid]);
    for (int j = tid; j < TN_SLOTS * TN_CHUNK; j += RING_THREADS) {
        const int n = acnt[j];
        if (n == 0) continue;                        // a slot without a row has no pair
        int* gs = stat + ((int64_t)hkey[j / TN_CHUNK] * shifts + k0 + (j & (TN_CHUNK - 1))) * 2;
        atomicAdd(gs, n);
        if (aerr[j] > 0) atomicMax(gs + 1, aerr[j]);
    }
}

// ---- 3. decide -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RING_THREADS) void tone_decide_kernel(const int* __restrict__ n_regions, int max_regions, int period, int shifts,
                                                                   int tol, const int* __restrict__ stat, const int* __restrict__ ringn,
                                                                   int* __restrict__ cand, int* __restrict__ tone) {
    const int r = blockIdx.x * RING_THREADS + threadIdx.x;
    if (r >= clamp_count(n_regions[1], max_regions)) return;
    const int* s = stat + (int64_t)r * shifts * 2;
    const int n = ringn[r], dxs = 2 * period + 1;
    const int e01 = s[(period + 1) * 2 + 1], e10 = s[(dxs + period) * 2 + 1];      // the unit shifts (0, 1) and (1, 0)
    const int step = e01 > e10 ? e01 : e10;
    int best_err = INT_MAX, best_d2 = 0, best_dy = 0, best_dx = 0;
    if (n >= 1) {
        for (int k = 0; k < shifts; ++k) {           // ascending (dy, dx): the first of equal (err, length) stays
            const int dy = k / dxs, dx = k - dy * dxs - period, ax = dx < 0 ? -dx : dx;
            if ((dy < 2 && ax < 2) || (dy == 0 && dx <= 0)) continue;
            const int cnt = s[2 * k], err = s[2 * k + 1], d2 = dy * dy + dx * dx;
            if (2 * cnt < n || err > tol) continue;
            if (err < best_err || (err == best_err && d2 < best_d2)) { best_err = err; best_d2 = d2; best_dy = dy; best_dx = dx; }
        }
    }
    const bool found = best_err != INT_MAX;
    const int flag = (found && step > tol) ? 1 : 0;
    int* f = tone + (int64_t)r * 6;
    f[0] = flag; f[1] = best_dy; f[2] = best_dx; f[3] = found ? best_err : 0; f[4] = n; f[5] = step;
    cand[r] = flag;
}

// ---- 4. sources ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RING_THREADS) void tone_source_kernel(const uint8_t* __restrict__ text, const int* __restrict__ labels, int h, int w,
                                                                   const int* __restrict__ table, const int* __restrict__ n_regions, int max_regions,
                                                                   const int* __restrict__ cand, int* nosrc, int* tone, int* __restrict__ src) {
    const int64_t p = (int64_t)blockIdx.x * RING_THREADS + threadIdx.x;
    if (p >= (int64_t)h * w || text[p] == 0) return;
    const int row = find_row(table, clamp_count(n_regions[1], max_regions), labels[p]);
    if (row < 0 || cand[row] == 0) return;
    const int dy = tone[(int64_t)row * 6 + 1], dx = tone[(int64_t)row * 6 + 2];      // written by the decide kernel, not touched here
    const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
    int ya = y, xa = x, yb = y, xb = x;
    bool ona = true, onb = true;
    for (int k = 1; k <= TN_WALK && (ona || onb); ++k) {
        ya += dy; xa += dx; yb -= dy; xb -= dx;
        ona = ona && ya < h && xa >= 0 && xa < w;    // dy >= 0: once off the page, off for good
        if (ona) {
            const int64_t q = (int64_t)ya * w + xa;
            if (text[q] == 0) { src[p] = (int)q; return; }
        }
        onb = onb && yb >= 0 && xb >= 0 && xb < w;
        if (onb) {
            const int64_t q = (int64_t)yb * w + xb;
            if (text[q] == 0) { src[p] = (int)q; return; }
        }
    }
    if (atomicMax(nosrc + row, 1) == 0) atomicAdd(tone + (int64_t)row * 6, -1);       // the first pixel without a source takes the flag back
}

// ---- 5. apply ------------------------------------------------------------------------------------------------------------------
// thread tid owns pixels 4 (tid & 15) .. + 3 of rows (tid >> 4) and (tid >> 4) + 16 of the rectangle
__global__ __launch_bounds__(RING_THREADS) void tone_apply_kernel(const uint8_t* __restrict__ page, uint8_t* text, const int* __restrict__ labels,
                                                                  const int* __restrict__ table, const int* __restrict__ n_regions, int max_regions,
                                                                  const int* __restrict__ tone, const int* __restrict__ src, PageGrid g,
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
    const int64_t npage = (int64_t)g.h * g.w;
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
            bool last_tone = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                m4[k] = t4[k] ? 255 : 0;
                if (t4[k] == 0) continue;
                const int lab = labels[p + k];
                if (lab != last_lab) {
                    last_lab = lab;
                    const int found = find_row(table, R, lab);
                    last_tone = found >= 0 && tone[(int64_t)found * 6] == 1;
                }
                if (last_tone) {
                    int64_t q = src[p + k];
                    q = q < 0 ? 0 : (q >= npage ? npage - 1 : q);      // as the source kernel noted it: a pixel of the page
                    b[3 * k] = page[q * 3]; b[3 * k + 1] = page[q * 3 + 1]; b[3 * k + 2] = page[q * 3 + 2];
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

extern "C" size_t tsii_tone_regions_ws_bytes(int h, int w, int max_regions, int period) {
    if (!tone_geometry(h, w, max_regions, period)) return 0;
    return tone_ws_bytes(h, w, max_regions, period);
}

extern "C" int tsii_tone_regions(const uint8_t* page, uint8_t* text, const int* labels, int h, int w, const int* table, const int* n_regions,
                                 int max_regions, int ring, int period, int tol, int tile, int halo, int* core_count, uint8_t* painted,
                                 uint8_t* mask, int* tone, void* ws, void* stream) {
    TSII_REQUIRE(page && text && labels && table && n_regions && painted && tone && ws, "tone_regions: null pointer");
    TSII_REQUIRE(period >= 2 && period <= TN_PMAX, "tone_regions: period %d (2..%d)", period, TN_PMAX);
    TSII_REQUIRE(tone_geometry(h, w, max_regions, period),
                 "tone_regions: page of %d x %d pixels, max_regions %d (h, w >= 1, h * w * 3 <= 2^31, max_regions >= 1, max_regions * shifts < 2^30)",
                 h, w, max_regions);
    TSII_REQUIRE(ring >= 1 && ring <= TN_RMAX, "tone_regions: ring %d (1..%d)", ring, TN_RMAX);
    TSII_REQUIRE(tol >= 0 && tol <= 255, "tone_regions: tol %d (0..255)", tol);
    TSII_REQUIRE(core_count == nullptr || grid_ok(h, w, tile, halo), "tone_regions: bad geometry h %d w %d tile %d halo %d", h, w, tile, halo);
    TSII_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3u) == 0, "tone_regions: ws must be 4-byte aligned");
    TSII_REQUIRE(painted != page, "tone_regions: painted must not be the page");
    const ApplyGrid a = make_apply_grid(h, w, tile, halo, core_count, RING_W, RING_H);
    const int rbx = cdiv(w, RING_W);
    const int64_t nring = (int64_t)rbx * cdiv(h, RING_H);
    TSII_REQUIRE(a.napply < (1ll << 31) && nring < (1ll << 31), "tone_regions: bad geometry h %d w %d tile %d halo %d (too many blocks)", h, w, tile, halo);
    hipStream_t st = (hipStream_t)stream;
    if (!clear_core_count(core_count, a.g, st)) return check_launch("tone_regions (memset)");
    const int shifts = tone_shifts(period);
    int* stat = static_cast<int*>(ws);
    int* ringn = stat + (size_t)max_regions * shifts * 2;
    int* cand = ringn + max_regions;
    int* nosrc = cand + max_regions;
    int* src = nosrc + max_regions;
    hipLaunchKernelGGL(tone_init_kernel, dim3(flat_grid((int64_t)max_regions * shifts * 2, RING_THREADS)), dim3(RING_THREADS), 0, st, n_regions,
                       max_regions, shifts, stat, ringn);
    hipLaunchKernelGGL(tone_ring_kernel, dim3((unsigned)nring, 1, (unsigned)cdiv(shifts, TN_CHUNK)), dim3(RING_THREADS), 0, st, page, text, labels,
                       h, w, rbx, table, n_regions, max_regions, ring, period, shifts, stat, ringn);
    hipLaunchKernelGGL(tone_decide_kernel, dim3(flat_grid(max_regions, RING_THREADS)), dim3(RING_THREADS), 0, st, n_regions, max_regions, period, shifts,
                       tol, stat, ringn, cand, tone);
    hipLaunchKernelGGL(tone_source_kernel, dim3(flat_grid((int64_t)h * w, RING_THREADS)), dim3(RING_THREADS), 0, st, text, labels, h, w, table, n_regions,
                       max_regions, cand, nosrc, tone, src);
    hipLaunchKernelGGL(tone_apply_kernel, dim3((unsigned)a.napply), dim3(RING_THREADS), 0, st, page, text, labels, table, n_regions, max_regions, tone,
                       src, a.g, a.nbx, a.nby, painted, mask, core_count);
    return check_launch("tone_regions");
}
