// K11: the page pipeline's two resamplings (include/tsii_hip.h, "working resolution"): a uint8 page to the segmenter's working size
// with Pillow's 8-bit bicubic filter, byte for byte, and the working-resolution text plane back onto the page's tile grid with the
// reference's "bilinear, then > 0" stated in integers.  Both are integer arithmetic from end to end: the only floating point is the
// double-precision coefficient table, computed on the host (tsii_resize_coeffs_u8) exactly as Pillow computes its own.
#include "page_grid.h"

#include <math.h>

namespace tsii {

constexpr int RS_PRECISION = 22;                          // Pillow's PRECISION_BITS for 8-bit channels: 32 - 8 - 2
constexpr int RS_MAX_RATIO = 8;                           // in / out and out / in per axis
constexpr int RS_MAX_TAPS = 2 * 2 * RS_MAX_RATIO + 1;     // 2 * ceil(support) + 1 at support = 2 * 8
constexpr int RS_BW = 64, RS_BH = 16;                     // output patch of a block
constexpr int RS_ROWS = RS_BH * RS_MAX_RATIO + RS_MAX_TAPS;   // input rows the patch's RS_BH output rows can need (161)

static inline bool resize_axis_ok(int in, int out) {
    return in >= 1 && out >= 1 && in < (1 << 20) && out < (1 << 20) && in <= RS_MAX_RATIO * out && out <= RS_MAX_RATIO * in;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ uint8_t clip8(unsigned acc) {
    return (uint8_t)clampi((int)acc >> RS_PRECISION, 0, 255);
}

// ---- bicubic resize ----------------------------------------------------------------------------------------------------------
// A block owns RS_BW x RS_BH output pixels:
//   0. its RS_BW rows of the horizontal table go to LDS (a row has an odd number of taps: lane-per-column reads are conflict free);
//   1. the input rows its output rows need are filtered horizontally to bytes in LDS, one thread per (row, column), 3 channels;
//   2. those bytes are filtered vertically, one thread per output pixel; a wave is one output row, so the vertical taps are uniform.
// A pass whose sizes agree copies.  Every bound read from a table is clamped to the buffers before it is used: a table that does not
// belong to these sizes gives wrong bytes, never an access outside the page, the output or LDS.
__global__ __launch_bounds__(256) void page_resize_u8_kernel(const uint8_t* __restrict__ page, int H, int W, int hs, int ws,
                                                             const int* __restrict__ by, const int* __restrict__ ky,
                                                             const int* __restrict__ bx, const int* __restrict__ kx,
                                                             int taps_y, int taps_x, uint8_t* __restrict__ out) {
    __shared__ uint8_t mid[RS_ROWS][RS_BW * 3];
    __shared__ int cx[RS_BW * RS_MAX_TAPS];
    __shared__ int xb[RS_BW][2];
    const int tid = threadIdx.x, c = tid & 63;
    const int ox0 = blockIdx.x * RS_BW, oy0 = blockIdx.y * RS_BH;
    const int ncols = ws - ox0 < RS_BW ? ws - ox0 : RS_BW, nrows = hs - oy0 < RS_BH ? hs - oy0 : RS_BH;
    const bool hpass = W != ws, vpass = H != hs;
    int y_lo = oy0, y_hi = oy0 + nrows;
    if (vpass) {
        const int last = oy0 + nrows - 1;
        y_lo = clampi(by[2 * oy0], 0, H);
        y_hi = clampi(by[2 * last] + by[2 * last + 1], y_lo, H);
        if (y_hi - y_lo > RS_ROWS) y_hi = y_lo + RS_ROWS;
    }
    if (hpass) {   // 0.
        for (int i = tid; i < ncols * taps_x; i += 256) cx[i] = kx[(int64_t)ox0 * taps_x + i];
        if (tid < ncols) {
            const int xmin = clampi(bx[2 * (ox0 + tid)], 0, W);
            xb[tid][0] = xmin;
            xb[tid][1] = clampi(bx[2 * (ox0 + tid) + 1], 0, taps_x < W - xmin ? taps_x : W - xmin);
        }
        __syncthreads();
    }
    if (c < ncols) {   // 1.
        for (int r = tid >> 6; r < y_hi - y_lo; r += 4) {
            const uint8_t* row = page + (int64_t)(y_lo + r) * W * 3;
            uint8_t* m = &mid[r][3 * c];
            if (hpass) {
                const uint8_t* p = row + xb[c][0] * 3;
                const int n = xb[c][1];
                const int* k = cx + c * taps_x;
                unsigned s0 = 1u << (RS_PRECISION - 1), s1 = s0, s2 = s0;
                for (int x = 0; x < n; ++x) {
                    const unsigned kk = (unsigned)k[x];
                    s0 += kk * p[3 * x]; s1 += kk * p[3 * x + 1]; s2 += kk * p[3 * x + 2];
                }
                m[0] = clip8(s0); m[1] = clip8(s1); m[2] = clip8(s2);
            } else {
                const uint8_t* p = row + (ox0 + c) * 3;
                m[0] = p[0]; m[1] = p[1]; m[2] = p[2];
            }
        }
    }
    __syncthreads();
    if (c < ncols) {   // 2.
        for (int r = tid >> 6; r < nrows; r += 4) {
            const int oy = oy0 + r;
            uint8_t* o = out + ((int64_t)oy * ws + ox0 + c) * 3;
            if (vpass) {
                const int ymin = clampi(by[2 * oy], y_lo, y_hi);
                const int n = clampi(by[2 * oy + 1], 0, taps_y < y_hi - ymin ? taps_y : y_hi - ymin);
                const int* k = ky + (int64_t)oy * taps_y;
                unsigned s0 = 1u << (RS_PRECISION - 1), s1 = s0, s2 = s0;
                for (int x = 0; x < n; ++x) {
                    const unsigned kk = (unsigned)k[x];
                    const uint8_t* m = &mid[ymin - y_lo + x][3 * c];
                    s0 += kk * m[0]; s1 += kk * m[1]; s2 += kk * m[2];
                }
                o[0] = clip8(s0); o[1] = clip8(s1); o[2] = clip8(s2);
            } else {
                const uint8_t* m = &mid[r][3 * c];
                o[0] = m[0]; o[1] = m[1]; o[2] = m[2];
            }
        }
    }
}

// ---- text plane up --------------------------------------------------------------------------------------------------------------
// source taps of destination index d (align_corners = false, in integers): i0, and i1 = i0 unless the position has a fraction
__device__ __forceinline__ void up_taps(int d, int in, int out, int& i0, int& i1) {
    const int v = (2 * d + 1) * in - out;
    const unsigned num = v > 0 ? (unsigned)v : 0u, den = 2u * (unsigned)out;
    i0 = (int)(num / den);
    i0 = i0 < in - 1 ? i0 : in - 1;
    i1 = (num % den) != 0 && i0 + 1 < in ? i0 + 1 : i0;
}

// The block shape of the K8 mask kernel: MB_W x MB_H page pixels inside ONE tile core, so that a block's count goes to one tile.
// One lane per column (its two source columns are fixed), 8 rows per thread; the counts meet through __shfl_down and LDS and leave
// with one atomicAdd per block.
constexpr int UP_W = 64, UP_H = 32;

__global__ __launch_bounds__(256) void text_plane_up_kernel(const uint8_t* __restrict__ text_s, int hs, int ws, PageGrid g, int nbx, int nby,
                                                            uint8_t* __restrict__ text, int* __restrict__ core_count) {
    __shared__ int wave_count[4];
    const int tid = threadIdx.x, c = tid & 63;
    const int t = blockIdx.x / (nbx * nby), sub = blockIdx.x % (nbx * nby);
    const int ci = t / g.tx, cj = t % g.tx;
    const int y0 = ci * g.s + (sub / nbx) * UP_H, x0 = cj * g.s + (sub % nbx) * UP_W;
    const int yend = (ci + 1) * g.s < g.h ? (ci + 1) * g.s : g.h, xend = (cj + 1) * g.s < g.w ? (cj + 1) * g.s : g.w;
    if (y0 >= yend || x0 >= xend) return;               // the whole block: this part of the core is off the page / past the core
    int cnt = 0;
    if (x0 + c < xend) {
        int sx0, sx1;
        up_taps(x0 + c, ws, g.w, sx0, sx1);
        for (int row = tid >> 6; row < UP_H && y0 + row < yend; row += 4) {
            int sy0, sy1;
            up_taps(y0 + row, hs, g.h, sy0, sy1);
            const uint8_t* r0 = text_s + (int64_t)sy0 * ws;
            const uint8_t* r1 = text_s + (int64_t)sy1 * ws;
            const uint8_t v = (r0[sx0] | r0[sx1] | r1[sx0] | r1[sx1]) ? 1 : 0;
            text[(int64_t)(y0 + row) * g.w + x0 + c] = v;
            cnt += v;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_down(cnt, d);
    if (c == 0) wave_count[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        const int total = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
        if (total > 0) atomicAdd(core_count + t, total);
    }
}

}  // namespace tsii

using namespace tsii;

extern "C" int tsii_resize_taps(int in, int out) {
    if (!resize_axis_ok(in, out)) return 0;
    const double scale = (double)in / (double)out;
    const double support = 2.0 * (scale < 1.0 ? 1.0 : scale);
    return (int)ceil(support) * 2 + 1;
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter.  Contraction is off: a fused multiply-add in the filter
// polynomial or in w * 2^22 + 0.5 can move a coefficient by one unit, and the result would no longer be Pillow's.
extern "C" int tsii_resize_coeffs_u8(int in, int out, int* bounds, int* kk) {
#pragma clang fp contract(off)
    TSII_REQUIRE(bounds && kk, "resize_coeffs_u8: null pointer");
    TSII_REQUIRE(resize_axis_ok(in, out), "resize_coeffs_u8: sizes %d -> %d (both >= 1, the ratio within [1/%d, %d])", in, out, RS_MAX_RATIO, RS_MAX_RATIO);
    const int taps = tsii_resize_taps(in, out);
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs;
    const double a = -0.5;
    double w[RS_MAX_TAPS];
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        const int n = xmax - xmin < taps ? xmax - xmin : taps;
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            double t = (x + xmin - center + 0.5) / fs;
            if (t < 0.0) t = -t;
            double v = 0.0;
            if (t < 1.0) v = ((a + 2.0) * t - (a + 3.0)) * t * t + 1;
            else if (t < 2.0) v = (((t - 5) * t + 8) * t - 4) * a;
            w[x] = v;
            ww += v;
        }
        int* k = kk + (size_t)xx * taps;
        for (int x = 0; x < taps; ++x) {
            int q = 0;
            if (x < n) {
                const double v = ww != 0.0 ? w[x] / ww : w[x];
                q = v < 0 ? (int)(-0.5 + v * (double)(1 << RS_PRECISION)) : (int)(0.5 + v * (double)(1 << RS_PRECISION));
            }
            k[x] = q;
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = n;
    }
    return 0;
}

extern "C" int tsii_page_resize_u8(const uint8_t* page, int h, int w, int hs, int ws, const int* bounds_y, const int* kk_y,
                                   const int* bounds_x, const int* kk_x, int taps_y, int taps_x, uint8_t* out, void* stream) {
    TSII_REQUIRE(page && out, "page_resize_u8: null pointer");
    TSII_REQUIRE(resize_axis_ok(h, hs) && resize_axis_ok(w, ws), "page_resize_u8: %d x %d -> %d x %d (sides >= 1, each ratio within [1/%d, %d])",
                 h, w, hs, ws, RS_MAX_RATIO, RS_MAX_RATIO);
    TSII_REQUIRE(h == hs || (bounds_y && kk_y && taps_y == tsii_resize_taps(h, hs)), "page_resize_u8: vertical tables (taps %d) do not belong to %d -> %d", taps_y, h, hs);
    TSII_REQUIRE(w == ws || (bounds_x && kk_x && taps_x == tsii_resize_taps(w, ws)), "page_resize_u8: horizontal tables (taps %d) do not belong to %d -> %d", taps_x, w, ws);
    hipLaunchKernelGGL(page_resize_u8_kernel, dim3((unsigned)cdiv(ws, RS_BW), (unsigned)cdiv(hs, RS_BH)), dim3(256), 0, (hipStream_t)stream,
                       page, h, w, hs, ws, bounds_y, kk_y, bounds_x, kk_x, taps_y, taps_x, out);
    return check_launch("page_resize_u8");
}

extern "C" int tsii_text_plane_up(const uint8_t* text_s, int hs, int ws, int h, int w, int tile, int halo,
                                  uint8_t* text, int* core_count, void* stream) {
    TSII_REQUIRE(text_s && text && core_count, "text_plane_up: null pointer");
    TSII_REQUIRE(grid_ok(h, w, tile, halo), "text_plane_up: bad geometry h %d w %d tile %d halo %d", h, w, tile, halo);
    TSII_REQUIRE(hs >= 1 && ws >= 1 && (2ll * h + 1) * hs < (1ll << 31) && (2ll * w + 1) * ws < (1ll << 31),
                 "text_plane_up: working plane %d x %d for a page of %d x %d is out of range", hs, ws, h, w);
    const PageGrid g = make_grid(h, w, tile, halo);
    const int nt = g.ty * g.tx, nbx = cdiv(g.s, UP_W), nby = cdiv(g.s, UP_H);
    TSII_REQUIRE((int64_t)nt * nbx * nby < (1ll << 31), "text_plane_up: page too large");
    if (hipMemsetAsync(core_count, 0, sizeof(int) * (size_t)nt, (hipStream_t)stream) != hipSuccess) return check_launch("text_plane_up (memset)");
    hipLaunchKernelGGL(text_plane_up_kernel, dim3((unsigned)(nt * nbx * nby)), dim3(256), 0, (hipStream_t)stream,
                       text_s, hs, ws, g, nbx, nby, text, core_count);
    return check_launch("text_plane_up");
}
