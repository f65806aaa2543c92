// K23: region crops (include/tsii_hip.h, "region crops"): every table row's minimum-area rectangle, as tsii_region_geometry left it, is
// cut out of the raw page, deskewed, scaled into a fixed slot of ch x cw pixels and left on the device in the shape an OCR net takes.
// All integer: one defined answer, the same bits on every run.  The header has the semantics; this file has two kernels.
//
//   1. header:  a lane per table row.  The padded rectangle, the frame, the fit, the supersampling factor and the fixed-point origin and
//               sides (the row's ~12 int64 divisions) are taken once per row and left in info[r], which is also all the second kernel
//               reads of the row: what the host gets is what the pixels were made from.
//   2. sample:  a block of 256 threads owns a 16 x 16 tile of one slot, a thread one slot pixel.  The sample position is separable:
//               P = O + C(m) + W(l), C a function of the sub-column and W of the sub-row.  The tile has 16 s sub-columns and 16 s
//               sub-rows of two components each, at most 256 terms at s = 4: a thread takes one of them, through LDS.  The term itself is
//               floor(S (2m + 1) / den) with S an int32 and den = 2 uw s <= 32768: with q = floor(S / den) and rem = S - q den it is
//               q (2m + 1) + (rem (2m + 1)) / den, whose product stays below 2^30: two 32-bit divisions and no 64-bit one.  A thread then
//               walks its s x s sub-samples: 4 neighbours x 3 bytes each, clamped to the page.  Pixels outside uh x uw get `fill`; a tile
//               wholly outside skips the terms.
// No workspace, no atomics, no floating point, no waiting on another block.  The count read from n_regions is clamped to max_regions and
// max_crops; a row of rect is validated (VALIDATION in the header) before anything is derived from it and is served as a row without
// pixels where it fails; every page index is clamped to the page: a foreign table gives wrong pictures, never an access outside the
// buffers.
#include "region_ring.h"

namespace tsii {

constexpr int CR_THREADS = 256, CR_TILE = 16, CR_INFO = 10, CR_MAX_SS = 4, CR_TERMS = CR_TILE * CR_MAX_SS;
constexpr int64_t CR_MAX_DOT = (1ll << 31) - 65536;      // |lo|, |hi|: Eu / 2 = (hi - lo) + pad then stays below 2^32

// floor(a / b) for b > 0
__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) {
    const int64_t q = a / b;
    return (a % b < 0) ? q - 1 : q;
}
__device__ __forceinline__ int floor_div32(int a, int b) {
    const int q = a / b;
    return (a % b < 0) ? q - 1 : q;
}
__device__ __forceinline__ bool fits_i32(int64_t v) { return v >= -(1ll << 31) && v < (1ll << 31); }
__device__ __forceinline__ int clampi(int64_t v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

// ---- 1. header ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CR_THREADS) void crops_header_kernel(const int64_t* __restrict__ rect, const int* __restrict__ n_regions, int max_rows,
                                                                  int ch, int cw, int orient, int max_ss, int* __restrict__ info) {
    const int r = blockIdx.x * CR_THREADS + threadIdx.x;
    const int R = clamp_count(n_regions[1], max_rows);
    if (r >= R) return;
    int out[CR_INFO] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t* row = rect + (int64_t)r * 8;
    const int64_t dy = row[1], dx = row[2], lo_d = row[3], hi_d = row[4], lo_n = row[5], hi_n = row[6], D = row[7];
    bool ok = D >= 1 && D <= (1ll << 31) && dy >= -32767 && dy <= 32767 && dx >= -32767 && dx <= 32767 &&
              lo_d >= -CR_MAX_DOT && hi_d <= CR_MAX_DOT && lo_d <= hi_d && lo_n >= -CR_MAX_DOT && hi_n <= CR_MAX_DOT && lo_n <= hi_n;
    if (ok) {
        const int64_t pad = (dy < 0 ? -dy : dy) + (dx < 0 ? -dx : dx);
        const int64_t A0 = 2 * lo_d - pad, A1 = 2 * hi_d + pad, B0 = 2 * lo_n - pad, B1 = 2 * hi_n + pad;
        const int64_t EA = A1 - A0, EB = B1 - B0;
        // the frames: u and v as (y part, x part), the ranges' lower ends; Eu is EA for f = 0, 2 and EB for f = 1, 3
        const int64_t uy[4] = {dy, dx, -dy, -dx}, ux[4] = {dx, -dy, -dx, dy};
        const int64_t vy[4] = {dx, -dy, -dx, dy}, vx[4] = {-dy, -dx, dy, dx};
        const int64_t U0s[4] = {A0, -B1, -A1, B0}, V0s[4] = {-B1, -A1, B0, A0};
        int f = -1;
        int64_t fuy = 0, fux = 0, fvy = 0, fvx = 0, U0 = 0, V0 = 0;     // the chosen frame, in scalars: the tables above are indexed by constants only
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t eu = (k & 1) ? EB : EA, ev = (k & 1) ? EA : EB;
            if (orient == 1 && eu < ev) continue;
            if (f < 0 || ux[k] > fux || (orient == 1 && ux[k] == fux && uy[k] > fuy)) {
                f = k; fuy = uy[k]; fux = ux[k]; fvy = vy[k]; fvx = vx[k]; U0 = U0s[k]; V0 = V0s[k];
            }
        }
        const int64_t Eu = (f & 1) ? EB : EA, Ev = (f & 1) ? EA : EB;
        ok = Eu >= 1 && Ev >= 1;                        // a foreign row only: pad >= 1 wherever d is not (0, 0)
        if (ok) {
            int uh, uw;
            if (Eu * ch >= Ev * cw) { uw = cw; uh = clampi((2 * (int64_t)cw * Ev + Eu) / (2 * Eu), 1, ch); }
            else                    { uh = ch; uw = clampi((2 * (int64_t)ch * Eu + Ev) / (2 * Ev), 1, cw); }
            const u64 hu = (u64)(Eu / 2), hv = (u64)(Ev / 2);
            int s = max_ss;
            for (int k = max_ss - 1; k >= 1; --k) {
                const u64 su = (u64)k * uw, sv = (u64)k * uh;
                if (su * su * (u64)D >= hu * hu && sv * sv * (u64)D >= hv * hv) s = k;
            }
            const int64_t v[6] = {floor_div((U0 * fuy + V0 * fvy) * 2048, D), floor_div((U0 * fux + V0 * fvx) * 2048, D),
                                  floor_div(Eu * fuy * 2048, D), floor_div(Eu * fux * 2048, D),
                                  floor_div(Ev * fvy * 2048, D), floor_div(Ev * fvx * 2048, D)};
#pragma unroll
            for (int k = 0; k < 6; ++k) ok = ok && fits_i32(v[k]);
            if (ok) {
                out[0] = uh; out[1] = uw; out[2] = f; out[3] = s;
#pragma unroll
                for (int k = 0; k < 6; ++k) out[4 + k] = (int)v[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < CR_INFO; ++k) info[(int64_t)r * CR_INFO + k] = out[k];
}

// ---- 2. sample ---------------------------------------------------------------------------------------------------------------------
// block b: tile b % tiles of slot b / tiles; thread tid: slot pixel (16 ty + (tid >> 4), 16 tx + (tid & 15))
__global__ __launch_bounds__(CR_THREADS) void crops_sample_kernel(const uint8_t* __restrict__ page, int h, int w, const int* __restrict__ n_regions,
                                                                  int max_rows, int ch, int cw, int fill, int max_ss, int tiles_x, int tiles,
                                                                  const int* __restrict__ info, uint8_t* __restrict__ crops) {
    __shared__ int term[4][CR_TERMS];                    // C_y, C_x over the tile's sub-columns, W_y, W_x over its sub-rows
    const int tid = threadIdx.x;
    const int r = blockIdx.x / tiles, t = blockIdx.x % tiles;
    if (r >= clamp_count(n_regions[1], max_rows)) return;   // the whole block
    const int i0 = (t / tiles_x) * CR_TILE, j0 = (t % tiles_x) * CR_TILE;
    const int* my = info + (int64_t)r * CR_INFO;
    const int uh = clamp_count(my[0], ch), uw = clamp_count(my[1], cw), s = clamp_count(my[3], max_ss);
    const bool inside = i0 < uh && j0 < uw && s >= 1;       // the whole block
    if (inside) {
        const int which = tid >> 6, e = tid & 63;           // which: 0, 1 the columns' y and x parts, 2, 3 the rows'
        const int first = (which < 2 ? j0 : i0) * s, count = (which < 2 ? uw : uh) * s;
        if (e < CR_TILE * s && first + e < count) {
            const int S = my[6 + which], den = 2 * count, odd = 2 * (first + e) + 1;
            const int q = floor_div32(S, den), rem = S - q * den;                    // 0 <= rem < den <= 32768, odd < den
            term[which][e] = (int)((int64_t)q * odd + (int64_t)((unsigned)(rem * odd) / (unsigned)den));
        }
        __syncthreads();
    }
    const int ii = tid >> 4, jj = tid & 15, i = i0 + ii, j = j0 + jj;
    if (i >= ch || j >= cw) return;
    uint8_t* dst = crops + (((int64_t)r * ch + i) * cw + j) * 3;
    if (!inside || i >= uh || j >= uw) {
        dst[0] = dst[1] = dst[2] = (uint8_t)fill;
        return;
    }
    const int64_t oy = my[4], ox = my[5];
    unsigned acc[3] = {0u, 0u, 0u};
    for (int a = 0; a < s; ++a) {
        const int64_t py0 = oy + term[2][ii * s + a], px0 = ox + term[3][ii * s + a];
        for (int b = 0; b < s; ++b) {
            const int64_t py = py0 + term[0][jj * s + b], px = px0 + term[1][jj * s + b];
            const int64_t iy = py >> 12, ix = px >> 12;
            const unsigned fy = (unsigned)(py & 4095) >> 4, fx = (unsigned)(px & 4095) >> 4;
            const int ya = clampi(iy, 0, h - 1), yb = clampi(iy + 1, 0, h - 1), xa = clampi(ix, 0, w - 1), xb = clampi(ix + 1, 0, w - 1);
            const uint8_t* p00 = page + ((int64_t)ya * w + xa) * 3;
            const uint8_t* p01 = page + ((int64_t)ya * w + xb) * 3;
            const uint8_t* p10 = page + ((int64_t)yb * w + xa) * 3;
            const uint8_t* p11 = page + ((int64_t)yb * w + xb) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                acc[c] += (256u - fy) * ((256u - fx) * p00[c] + fx * p01[c]) + fy * ((256u - fx) * p10[c] + fx * p11[c]);
        }
    }
    const unsigned ss = (unsigned)(s * s);
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c] = (uint8_t)((acc[c] + 32768u * ss) / (65536u * ss));
}

}  // namespace tsii

using namespace tsii;

extern "C" int tsii_region_crops(const uint8_t* page, int h, int w, const int64_t* rect, const int* n_regions, int max_regions, int max_crops,
                                 int ch, int cw, int orient, int fill, int max_ss, int* info, uint8_t* crops, void* stream) {
    TSII_REQUIRE(page && rect && n_regions && info && crops, "region_crops: null pointer");
    TSII_REQUIRE(h >= 1 && h <= 32767 && w >= 1 && w <= 32767, "region_crops: page of %d x %d pixels (sides 1..32767)", h, w);
    TSII_REQUIRE(max_regions >= 1 && max_crops >= 1, "region_crops: max_regions %d, max_crops %d (>= 1)", max_regions, max_crops);
    TSII_REQUIRE(ch >= 1 && ch <= 4096 && cw >= 1 && cw <= 4096, "region_crops: slots of %d x %d pixels (sides 1..4096)", ch, cw);
    TSII_REQUIRE((int64_t)max_crops * ch * cw * 3 <= (1ll << 31) - 1, "region_crops: %d slots of %d x %d x 3 bytes (up to 2^31 - 1 bytes)", max_crops, ch, cw);
    TSII_REQUIRE(orient == 0 || orient == 1, "region_crops: orient %d (0: upright, 1: long)", orient);
    TSII_REQUIRE(fill >= 0 && fill <= 255, "region_crops: fill %d (0..255)", fill);
    TSII_REQUIRE(max_ss >= 1 && max_ss <= CR_MAX_SS, "region_crops: max_ss %d (1..%d)", max_ss, CR_MAX_SS);
    TSII_REQUIRE((reinterpret_cast<uintptr_t>(rect) & 7u) == 0, "region_crops: rect must be 8-byte aligned");
    TSII_REQUIRE((reinterpret_cast<uintptr_t>(info) & 3u) == 0, "region_crops: info must be 4-byte aligned");
    const int max_rows = max_regions < max_crops ? max_regions : max_crops;
    const int tiles_x = cdiv(cw, CR_TILE), tiles = tiles_x * cdiv(ch, CR_TILE);
    const int64_t nblocks = (int64_t)max_rows * tiles;      // <= max_crops * ch * cw: below 2^31
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(crops_header_kernel, dim3((unsigned)cdiv(max_rows, CR_THREADS)), dim3(CR_THREADS), 0, st, rect, n_regions, max_rows, ch, cw,
                       orient, max_ss, info);
    hipLaunchKernelGGL(crops_sample_kernel, dim3((unsigned)nblocks), dim3(CR_THREADS), 0, st, page, h, w, n_regions, max_rows, ch, cw, fill, max_ss,
                       tiles_x, tiles, info, crops);
    return check_launch("region_crops");
}
