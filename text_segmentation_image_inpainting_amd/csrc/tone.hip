// K17: tone regions (include/tsii_hip.h, "tone regions"): a text region whose surrounding ring of page pixels is a periodic pattern --
// screentone, stripes, a dot lattice -- is filled by copying, for every text pixel, the nearest non-text pixel a whole number of periods
// away, and leaves the text plane.  The period is one integer shift per region, measured on the ring: the shift under which the ring
// matches the page best.  All in 32-bit integers with atomicAdd and atomicMax: one defined answer, the same bits on every run.
//
//   1. init:   the statistics of the table rows in use (nothing in ws has to be cleared by the caller);
//   2. ring:   K13's ring kernel (csrc/flat.hip) with another statistic.  A block owns TN_W x TN_H page pixels and stages, for them and an
//              apron of `ring` pixels, the table row of every text pixel, and, for them and an apron of `period` pixels to the left, to
//              the right and below, the page bytes of the non-text pixels.  The shifts (dy 0..period, dx -period..period) are cut into
//              chunks of TN_CHUNK over blockIdx.z; a block keeps cnt and err of (row, shift) for up to TN_SLOTS rows in LDS and leaves
//              one pair of atomics per (block, row, shift) with a pair; rows beyond TN_SLOTS go to memory directly.  The lanes of a wave
//              walk the chunk rotated by their lane number, so that 64 pixels of one row do not meet at one LDS word.  A block with no
//              text within `ring` leaves after the first staging;
//   3. decide: one thread per table row: step, the best shift by the key (err, dy^2 + dx^2, dy, dx) -> `tone` (the flag still without the
//              source check);
//   4. source: one thread per page pixel; a text pixel of a row with a flag walks p + s, p - s, p + 2 s, ... to its first non-text pixel
//              and notes it in ws; without one within TN_WALK steps each way the row's flag is taken back (the first such pixel of a row,
//              by atomicMax on a word of ws, takes it back with one atomicAdd);
//   5. apply:  K13's apply geometry: a block owns a TN_W x TN_H rectangle of one tile core, a thread 4 consecutive pixels of a row; the
//              noted source is read on the text pixels of tone rows only.
// No grid-wide barrier, no waiting on another block: each step is its own launch.  The count read from n_regions is clamped to max_regions
// and a row found by the search lies below it; a noted source is always a pixel of the page: a table that does not belong to the labels
// gives wrong bytes, never an access outside the buffers.  The boxes of the table are not read.  The ring walk is a copy of K13's and not
// a shared header: flat.hip and smooth.hip stay as they are.
#include "page_grid.h"

#include <limits.h>
#include <string.h>

namespace tsii {

typedef unsigned long long u64;

#ifdef TSII_HIP_EMU
// the test emulator runs one thread at a time and supplies the 32-bit atomicAdd only
static inline int atomicMax(int* p, int v) { const int o = *p; if (v > o) *p = v; return o; }
static inline int atomicCAS(int* p, int expect, int v) { const int o = *p; if (o == expect) *p = v; return o; }
#endif

constexpr int TN_W = 64, TN_H = 32, TN_THREADS = 256, TN_PER = TN_W * TN_H / TN_THREADS;
constexpr int TN_RMAX = 16, TN_SW = TN_W + 2 * TN_RMAX, TN_SH = TN_H + 2 * TN_RMAX;      // the staged rows at the widest ring
constexpr int TN_PMAX = 16, TN_PW = TN_W + 2 * TN_PMAX, TN_PH = TN_H + TN_PMAX;          // the staged page bytes at the longest period
constexpr int TN_SLOTS = 16, TN_CHUNK = 128;     // table rows per block in LDS (a row that finds no slot goes to memory); shifts per block
constexpr int TN_WALK = 256;                     // steps each way of the source walk
constexpr int TN_NOTEXT = -2, TN_NOROW = -1;     // staged values below the table rows: not text (or off the page); text of no table row
constexpr int TN_NOPIX = -1;                     // staged page bytes: text, or off the page
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

__device__ __forceinline__ int tn_clamp_count(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the table row whose label is lab, TN_NOROW without one (the table ascends in label)
__device__ __forceinline__ int tn_find_row(const int* __restrict__ table, int R, int lab) {
    int lo = 0, hi = R;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (table[(int64_t)mid * 6] < lab) lo = mid + 1; else hi = mid;
    }
    return (lo < R && table[(int64_t)lo * 6] == lab) ? lo : TN_NOROW;
}

// ---- 1. init ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TN_THREADS) void tone_init_kernel(const int* __restrict__ n_regions, int max_regions, int shifts,
                                                               int* __restrict__ stat, int* __restrict__ small) {
    const int64_t i = (int64_t)blockIdx.x * TN_THREADS + threadIdx.x;
    const int R = tn_clamp_count(n_regions[1], max_regions);
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
    const int e0 = (a & 255) - (b & 255), e1 = ((a >> 8) & 255) - ((b >> 8) & 255), e2 = ((a >> 16) & 255) - ((b >> 16) & 255);
    const int f0 = e0 < 0 ? -e0 : e0, f1 = e1 < 0 ? -e1 : e1, f2 = e2 < 0 ? -e2 : e2;
    const int m = f0 > f1 ? f0 : f1;
    return m > f2 ? m : f2;
}

__global__ __launch_bounds__(TN_THREADS) void tone_ring_kernel(const uint8_t* __restrict__ page, const uint8_t* __restrict__ text,
                                                               const int* __restrict__ labels, int h, int w, int nbx,
                                                               const int* __restrict__ table, const int* __restrict__ n_regions, int max_regions,
                                                               int ring, int period, int shifts, int* stat, int* ringn) {
    __shared__ int idx[TN_SH * TN_SW];               // rows of sw = TN_W + 2 ring entries: table row, TN_NOROW or TN_NOTEXT
    __shared__ int pix[TN_PH * TN_PW];               // rows of pw = TN_W + 2 period entries: r | g << 8 | b << 16 of the non-text pixels, else TN_NOPIX
    __shared__ u64 hrow[TN_SH];                      // bit c: a pixel with a table row in staged columns c .. c + 2 ring of this staged row
    __shared__ u64 vnear[TN_H];                      // bit c: ... within `ring` of the block's pixel (row, c)
    __shared__ int hkey[TN_SLOTS], hn[TN_SLOTS];
    __shared__ int acnt[TN_SLOTS * TN_CHUNK], aerr[TN_SLOTS * TN_CHUNK];
    __shared__ int soff[TN_CHUNK];                   // the chunk's shifts as offsets into pix
    const int tid = threadIdx.x;
    const int x0 = (blockIdx.x % nbx) * TN_W, y0 = (blockIdx.x / nbx) * TN_H;
    const int k0 = blockIdx.z * TN_CHUNK;            // the first shift of this block's chunk
    const int R = tn_clamp_count(n_regions[1], max_regions);
    const int sw = TN_W + 2 * ring, sh = TN_H + 2 * ring, span = 2 * ring;
    const int pw = TN_W + 2 * period, ph = TN_H + period, dxs = 2 * period + 1;
    for (int j = tid; j < sh * sw; j += TN_THREADS) {
        const int sr = j / sw, sc = j - sr * sw;
        const int y = y0 - ring + sr, x = x0 - ring + sc;
        int v = TN_NOTEXT;
        if (y >= 0 && y < h && x >= 0 && x < w) {
            const int64_t p = (int64_t)y * w + x;
            if (text[p] != 0) v = tn_find_row(table, R, labels[p]);
        }
        idx[j] = v;
    }
    __syncthreads();
    if (tid < sh) {                                  // one staged row per thread: its "has a row" bits, dilated to the right by 2 ring
        u64 lo = 0, hi = 0;
        const int* s = idx + tid * sw;
        for (int c = 0; c < sw; ++c) {
            const u64 b = s[c] >= 0 ? 1ull : 0ull;
            if (c < 64) lo |= b << c; else hi |= b << (c - 64);
        }
        u64 acc = lo;
        for (int k = 1; k <= span; ++k) acc |= (lo >> k) | (hi << (64 - k));
        hrow[tid] = acc;
    }
    __syncthreads();
    if (tid < TN_H) {
        u64 acc = 0;
        for (int k = 0; k <= span; ++k) acc |= hrow[tid + k];
        vnear[tid] = acc;
    }
    __syncthreads();
    u64 any = 0;
    for (int r = 0; r < TN_H; ++r) any |= vnear[r];
    if (any == 0) return;                            // the whole block: no table row within `ring` of its pixels
    for (int j = tid; j < ph * pw; j += TN_THREADS) {
        const int sr = j / pw, sc = j - sr * pw;
        const int y = y0 + sr, x = x0 - period + sc;
        int v = TN_NOPIX;
        if (y < h && x >= 0 && x < w) {
            const int64_t p = (int64_t)y * w + x;
            if (text[p] == 0) v = (int)page[p * 3] | ((int)page[p * 3 + 1] << 8) | ((int)page[p * 3 + 2] << 16);
        }
        pix[j] = v;
    }
    for (int j = tid; j < TN_SLOTS * TN_CHUNK; j += TN_THREADS) acnt[j] = aerr[j] = 0;
    if (tid < TN_SLOTS) { hkey[tid] = -1; hn[tid] = 0; }
    if (tid < TN_CHUNK) {
        const int k = k0 + tid, dy = k / dxs, dx = k - dy * dxs - period;
        soff[tid] = (k < shifts && (dy > 0 || dx > 0)) ? dy * pw + dx : TN_NOSHIFT;
    }
    __syncthreads();
    const int c = tid & 63, x = x0 + c;
    int last_row = -1, last_slot = -1;
    if (x < w) {
        for (int k = 0, r = tid >> 6; k < TN_PER; ++k, r += 4) {
            const int y = y0 + r;
            if (y >= h || !((vnear[r] >> c) & 1ull)) continue;
            const int* pc = pix + r * pw + c + period;
            const int me = pc[0];
            if (me == TN_NOPIX) continue;            // text
            int cur = -1;                            // the rows of the window in ascending order, two per walk
            for (;;) {
                int m1 = INT_MAX, m2 = INT_MAX;
                for (int dy = 0; dy <= span; ++dy) {
                    const int* s = idx + (r + dy) * sw + c;
                    for (int dx = 0; dx <= span; ++dx) {
                        const int v = s[dx];
                        if (v > cur && v != m1) {
                            if (v < m1) { m2 = m1; m1 = v; }
                            else if (v < m2) m2 = v;
                        }
                    }
                }
                if (m1 == INT_MAX) break;
                for (int t = 0; t < 2; ++t) {
                    const int row = t == 0 ? m1 : m2;
                    if (row == INT_MAX) break;
                    if (row != last_row) { last_row = row; last_slot = tn_slot(hkey, row); }
                    if (blockIdx.z == 0) {           // n_r: by the blocks of the first chunk
                        if (last_slot >= 0) atomicAdd(hn + last_slot, 1);
                        else atomicAdd(ringn + row, 1);
                    }
                    int* gs = stat + ((int64_t)row * shifts + k0) * 2;
                    for (int i = 0; i < TN_CHUNK; ++i) {
                        const int j = (i + c) & (TN_CHUNK - 1);
                        const int off = soff[j];
                        if (off == TN_NOSHIFT) continue;
                        const int other = pc[off];
                        if (other == TN_NOPIX) continue;
                        const int e = tn_diff(me, other);
                        if (last_slot >= 0) {
                            atomicAdd(acnt + last_slot * TN_CHUNK + j, 1);
                            if (e > 0) atomicMax(aerr + last_slot * TN_CHUNK + j, e);
                        } else {
                            atomicAdd(gs + 2 * j, 1);
                            if (e > 0) atomicMax(gs + 2 * j + 1, e);
                        }
                    }
                }
                if (m2 == INT_MAX) break;
                cur = m2;
            }
        }
    }
    __syncthreads();
    if (tid < TN_SLOTS && hn[tid] > 0) atomicAdd(ringn + hkey[tid], hn[tid]);
    for (int j = tid; j < TN_SLOTS * TN_CHUNK; j += TN_THREADS) {
        const int n = acnt[j];
        if (n == 0) continue;                        // a slot without a row has no pair
        int* gs = stat + ((int64_t)hkey[j / TN_CHUNK] * shifts + k0 + (j & (TN_CHUNK - 1))) * 2;
        atomicAdd(gs, n);
        if (aerr[j] > 0) atomicMax(gs + 1, aerr[j]);
    }
}

// ---- 3. decide -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TN_THREADS) void tone_decide_kernel(const int* __restrict__ n_regions, int max_regions, int period, int shifts,
                                                                 int tol, const int* __restrict__ stat, const int* __restrict__ ringn,
                                                                 int* __restrict__ cand, int* __restrict__ tone) {
    const int r = blockIdx.x * TN_THREADS + threadIdx.x;
    if (r >= tn_clamp_count(n_regions[1], max_regions)) return;
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
__global__ __launch_bounds__(TN_THREADS) void tone_source_kernel(const uint8_t* __restrict__ text, const int* __restrict__ labels, int h, int w,
                                                                 const int* __restrict__ table, const int* __restrict__ n_regions, int max_regions,
                                                                 const int* __restrict__ cand, int* nosrc, int* tone, int* __restrict__ src) {
    const int64_t p = (int64_t)blockIdx.x * TN_THREADS + threadIdx.x;
    if (p >= (int64_t)h * w || text[p] == 0) return;
    const int row = tn_find_row(table, tn_clamp_count(n_regions[1], max_regions), labels[p]);
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
__global__ __launch_bounds__(TN_THREADS) void tone_apply_kernel(const uint8_t* __restrict__ page, uint8_t* text, const int* __restrict__ labels,
                                                                const int* __restrict__ table, const int* __restrict__ n_regions, int max_regions,
                                                                const int* __restrict__ tone, const int* __restrict__ src, PageGrid g,
                                                                int nbx, int nby, uint8_t* __restrict__ painted, uint8_t* __restrict__ mask,
                                                                int* __restrict__ core_count) {
    __shared__ int wave_count[TN_THREADS / 64];
    const int tid = threadIdx.x;
    const int t = blockIdx.x / (nbx * nby), sub = blockIdx.x % (nbx * nby);
    const int ci = t / g.tx, cj = t % g.tx;
    const int64_t y0 = (int64_t)ci * g.s + (sub / nbx) * TN_H, x0 = (int64_t)cj * g.s + (sub % nbx) * TN_W;
    const int64_t yend = (int64_t)(ci + 1) * g.s < g.h ? (int64_t)(ci + 1) * g.s : g.h, xend = (int64_t)(cj + 1) * g.s < g.w ? (int64_t)(cj + 1) * g.s : g.w;
    if (y0 >= yend || x0 >= xend) return;               // the whole block
    const int R = tn_clamp_count(n_regions[1], max_regions);
    const int64_t npage = (int64_t)g.h * g.w;
    const int64_t xa = x0 + 4 * (tid & 15);
    int cnt = 0;
    if (xa < xend) {
        const int npx = xend - xa < 4 ? (int)(xend - xa) : 4;
        for (int row = tid >> 4; row < TN_H && y0 + row < yend; row += TN_THREADS / 16) {
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
                    const int found = tn_find_row(table, R, lab);
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
        for (int k = 0; k < TN_THREADS / 64; ++k) total += wave_count[k];
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
    PageGrid g;
    if (core_count != nullptr) g = make_grid(h, w, tile, halo);
    else {                                              // without counts: cores of 2^20 pixels a side, no tile behind them
        g.h = h; g.w = w; g.tile = g.s = 1 << 20; g.halo = 0;
        g.ty = (int)cdiv64(h, g.s); g.tx = (int)cdiv64(w, g.s);
    }
    const int nbx = cdiv(g.s < w ? g.s : w, TN_W), nby = cdiv(g.s < h ? g.s : h, TN_H);
    const int64_t napply = (int64_t)g.ty * g.tx * nbx * nby;
    const int rbx = cdiv(w, TN_W);
    const int64_t nring = (int64_t)rbx * cdiv(h, TN_H);
    TSII_REQUIRE(napply < (1ll << 31) && nring < (1ll << 31), "tone_regions: bad geometry h %d w %d tile %d halo %d (too many blocks)", h, w, tile, halo);
    hipStream_t st = (hipStream_t)stream;
    if (core_count != nullptr && hipMemsetAsync(core_count, 0, sizeof(int) * (size_t)g.ty * g.tx, st) != hipSuccess)
        return check_launch("tone_regions (memset)");
    const int shifts = tone_shifts(period);
    int* stat = static_cast<int*>(ws);
    int* ringn = stat + (size_t)max_regions * shifts * 2;
    int* cand = ringn + max_regions;
    int* nosrc = cand + max_regions;
    int* src = nosrc + max_regions;
    hipLaunchKernelGGL(tone_init_kernel, dim3(flat_grid((int64_t)max_regions * shifts * 2, TN_THREADS)), dim3(TN_THREADS), 0, st, n_regions,
                       max_regions, shifts, stat, ringn);
    hipLaunchKernelGGL(tone_ring_kernel, dim3((unsigned)nring, 1, (unsigned)cdiv(shifts, TN_CHUNK)), dim3(TN_THREADS), 0, st, page, text, labels,
                       h, w, rbx, table, n_regions, max_regions, ring, period, shifts, stat, ringn);
    hipLaunchKernelGGL(tone_decide_kernel, dim3(flat_grid(max_regions, TN_THREADS)), dim3(TN_THREADS), 0, st, n_regions, max_regions, period, shifts,
                       tol, stat, ringn, cand, tone);
    hipLaunchKernelGGL(tone_source_kernel, dim3(flat_grid((int64_t)h * w, TN_THREADS)), dim3(TN_THREADS), 0, st, text, labels, h, w, table, n_regions,
                       max_regions, cand, nosrc, tone, src);
    hipLaunchKernelGGL(tone_apply_kernel, dim3((unsigned)napply), dim3(TN_THREADS), 0, st, page, text, labels, table, n_regions, max_regions, tone,
                       src, g, nbx, nby, painted, mask, core_count);
    return check_launch("tone_regions");
}
