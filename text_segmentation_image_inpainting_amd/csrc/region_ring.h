// What flat.hip (K13), smooth.hip (K16) and tone.hip (K17) share: the ring walk -- a block of 256 threads owns 64 x 32 page pixels,
// stages the table row of every text pixel around them, and every non-text pixel next to text meets each table row of its window once
// -- with clamp_count and find_row, which the apply kernels use too.  Device helpers only: every kernel stays in its own file, with its
// own statistic and its own LDS table of rows.  The apply kernels are three near-copies on purpose: their body moved into a device
// function no longer compiles to the one 12-byte store per full quad, and tsii_smooth_regions_apply measured 3.7 % slower.
#pragma once
#include "emu_atomics.h"
#include "page_grid.h"

#include <limits.h>
#include <string.h>

namespace tsii {

typedef unsigned long long u64;

constexpr int RING_W = 64, RING_H = 32, RING_THREADS = 256, RING_PER = RING_W * RING_H / RING_THREADS;
constexpr int NOTEXT = -2, NOROW = -1;           // staged values below the table rows: not text (or off the page); text of no table row
constexpr int NOPIX = -1;                        // staged page bytes: text, or off the page

__device__ __forceinline__ int clamp_count(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the table row whose label is lab, NOROW without one (the table ascends in label)
__device__ __forceinline__ int find_row(const int* __restrict__ table, int R, int lab) {
    int lo = 0, hi = R;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (table[(int64_t)mid * 6] < lab) lo = mid + 1; else hi = mid;
    }
    return (lo < R && table[(int64_t)lo * 6] == lab) ? lo : NOROW;
}

// ---- the ring walk -------------------------------------------------------------------------------------------------------------------
// idx: sh rows of sw = RING_W + 2 ring entries for the block's rectangle at (x0, y0) and an apron of `ring` pixels: the table row of a
// text pixel (binary search over the ascending label column; labels are read for text pixels only), NOROW or NOTEXT
__device__ __forceinline__ void stage_rows(int* idx, int sw, int sh, int x0, int y0, int ring, const uint8_t* __restrict__ text,
                                           const int* __restrict__ labels, int h, int w, const int* __restrict__ table, int R, int tid) {
    for (int j = tid; j < sh * sw; j += RING_THREADS) {
        const int sr = j / sw, sc = j - sr * sw;
        const int y = y0 - ring + sr, x = x0 - ring + sc;
        int v = NOTEXT;
        if (y >= 0 && y < h && x >= 0 && x < w) {
            const int64_t p = (int64_t)y * w + x;
            if (text[p] != 0) v = find_row(table, R, labels[p]);
        }
        idx[j] = v;
    }
}

// The dilated bit mask of "has a row" (the construction of the K8 mask kernel), which sends the great majority of non-text pixels away
// after one test.  hrow[sh], bit c: a pixel with a table row in staged columns c .. c + span of this staged row; vnear[RING_H], bit c:
// ... within span / 2 of the block's pixel (row, c).  Waits for the staging before it and for its own result.
__device__ __forceinline__ void near_bits(const int* idx, int sw, int sh, int span, u64* hrow, u64* vnear, int tid) {
    __syncthreads();
    if (tid < sh) {                                  // one staged row per thread: its "has a row" bits, dilated to the right by span
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
    if (tid < RING_H) {
        u64 acc = 0;
        for (int k = 0; k <= span; ++k) acc |= hrow[tid + k];
        vnear[tid] = acc;
    }
    __syncthreads();
}

// f(row) once per distinct table row in the (span + 1)^2 window of the block's pixel (r, c), in ascending order: two rows per walk of
// the window
template <class F>
__device__ __forceinline__ void for_rows_in_window(const int* idx, int sw, int r, int c, int span, F f) {
    int cur = -1;
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
            f(row);
        }
        if (m2 == INT_MAX) break;
        cur = m2;
    }
}

// ---- staged page bytes ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int pack_pixel(const uint8_t* __restrict__ page, int64_t p) {
    return (int)page[p * 3] | ((int)page[p * 3 + 1] << 8) | ((int)page[p * 3 + 2] << 16);
}
// pix: ph rows of pw entries for the page pixels from (xs, ys) on: r | g << 8 | b << 16 of a non-text pixel, NOPIX elsewhere
__device__ __forceinline__ void stage_pixels(int* pix, int pw, int ph, int xs, int ys, const uint8_t* __restrict__ page,
                                             const uint8_t* __restrict__ text, int h, int w, int tid) {
    for (int j = tid; j < ph * pw; j += RING_THREADS) {
        const int sr = j / pw, sc = j - sr * pw;
        const int y = ys + sr, x = xs + sc;
        int v = NOPIX;
        if (y >= 0 && y < h && x >= 0 && x < w) {
            const int64_t p = (int64_t)y * w + x;
            if (text[p] == 0) v = pack_pixel(page, p);
        }
        pix[j] = v;
    }
}
// |a - b| per byte of two staged pixels
__device__ __forceinline__ void abs_diff3(int a, int b, int& d0, int& d1, int& d2) {
    const int e0 = (a & 255) - (b & 255), e1 = ((a >> 8) & 255) - ((b >> 8) & 255), e2 = ((a >> 16) & 255) - ((b >> 16) & 255);
    d0 = e0 < 0 ? -e0 : e0; d1 = e1 < 0 ? -e1 : e1; d2 = e2 < 0 ? -e2 : e2;
}

}  // namespace tsii
