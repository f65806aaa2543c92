// K24: region paste (include/tsii_hip.h, "region paste"): the return trip of K23.  Every slot of a batch of straight-alpha RGBA pictures is
// laid back onto the page along the rectangle its info row names, antialiased, in ascending row order, in place.  All integer: one defined
// answer, the same bits on every run.  The header has the semantics; this file has two kernels.
//
//   1. plan:   a lane per row.  The row's validation, the steps Gu and Gv (crop pixels per 2^-12 page pixel, times 2^24), the supersampling
//              factor and the bounding box are taken once per row and left in plan[r]: the only place with 64-bit divisions.  The quotient
//              floor(S_c n 2^24 / (S.S)) does not fit int64 on the way (2^28 * 2^12 * 2^24), so it is taken as a long division, six bits at
//              a time, from a first quotient that the validation has already bounded by 128.
//   2. apply:  a block of 256 threads owns a 16 x 16 tile of the page, a thread one page pixel.  The rows are staged 256 at a time: thread k
//              tests row base + k (live, its box meets the tile) and leaves the row's box in LDS, an empty one where the test fails; a
//              chunk none of whose rows meets the tile is left at once (a word in LDS says whether a thread staged a hit).  Every thread
//              then walks the boxes in ascending order and composites the rows that hold its pixel into it; the pixel lives in registers
//              and is stored once, after the last row.
//              Per sub-sample the position is two v_mad_i64_i32 per axis (dP and G both fit int32, PLAN VALIDATION in the header); the
//              weights and sums are 32-bit.  The sub-sample offsets ((2l + 1) 2048) / s and the final division by 255 s^2 have s in 1..4:
//              a shift or a multiplication by a constant, no division instruction in the pixel loop.
// No workspace beyond plan, no atomics, no floating point, no waiting on another block: a page pixel belongs to one thread, which meets
// the rows in their order.  The count read from n_rows is clamped to max_rows; a row of info is validated before anything is derived from
// it and pastes nothing where it fails; every slot index is tested against uh x uw <= ch x cw and every box is clamped to the page: a
// foreign info gives wrong pictures, never an access outside the buffers.
#include "region_ring.h"

namespace tsii {

constexpr int PA_THREADS = 256, PA_TILE = 16, PA_INFO = 10, PA_PLAN = 12, PA_MAX_SS = 4, PA_CHUNK = PA_THREADS;
constexpr int64_t PA_MAX_O = 1ll << 29, PA_MAX_S = (1ll << 28) - 1;      // |O_c|; |SU_c|, |SV_c|: S.S stays below 2^57, |dP_c| below 2^30
constexpr int PA_G_BITS = 24, PA_STEP = 6;                          // the scale of G; the bits one step of the long division takes

__device__ __forceinline__ int64_t abs64(int64_t v) { return v < 0 ? -v : v; }

// floor(a 2^24 / d) for 1 <= d < 2^57 and |a| < 128 d: the floor quotient of a first (|q| <= 128, 0 <= rem < d), then 24 more bits,
// six at a time (rem << 6 < 2^63).  |result| <= 2^31.
__device__ __forceinline__ int64_t scaled_quotient(int64_t a, int64_t d) {
    int64_t q = a / d, rem = a % d;
    if (rem < 0) { q -= 1; rem += d; }
#pragma unroll
    for (int k = 0; k < PA_G_BITS / PA_STEP; ++k) {
        const u64 t = (u64)rem << PA_STEP, digit = t / (u64)d;
        rem = (int64_t)(t - digit * (u64)d);
        q = q * (1 << PA_STEP) + (int64_t)digit;
    }
    return q;
}

// ---- 1. plan -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PA_THREADS) void paste_plan_kernel(const int* __restrict__ info, const int* __restrict__ n_rows, int max_rows, int h, int w,
                                                                int ch, int cw, int max_ss, int64_t* __restrict__ plan) {
    const int r = blockIdx.x * PA_THREADS + threadIdx.x;
    if (r >= clamp_count(n_rows[0], max_rows)) return;
    int64_t out[PA_PLAN] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int* my = info + (int64_t)r * PA_INFO;
    const int uh = my[0], uw = my[1];
    const int64_t oy = my[4], ox = my[5], suy = my[6], sux = my[7], svy = my[8], svx = my[9];
    bool ok = uh >= 1 && uh <= ch && uw >= 1 && uw <= cw && abs64(oy) <= PA_MAX_O && abs64(ox) <= PA_MAX_O && abs64(suy) <= PA_MAX_S &&
              abs64(sux) <= PA_MAX_S && abs64(svy) <= PA_MAX_S && abs64(svx) <= PA_MAX_S;
    const int64_t uu = ok ? suy * suy + sux * sux : 0, vv = ok ? svy * svy + svx * svx : 0;      // below 2^57
    ok = ok && uu >= 1 && vv >= 1;
    // |G_c| < 2^31: |S_c| n < 128 (S.S), both sides below 2^64
    ok = ok && (u64)abs64(suy) * (u64)uw < 128ull * (u64)uu && (u64)abs64(sux) * (u64)uw < 128ull * (u64)uu &&
         (u64)abs64(svy) * (u64)uh < 128ull * (u64)vv && (u64)abs64(svx) * (u64)uh < 128ull * (u64)vv;
    if (ok) {
        const int64_t cy[4] = {oy, oy + suy, oy + suy + svy, oy + svy}, cx[4] = {ox, ox + sux, ox + sux + svx, ox + svx};
        int64_t ylo = cy[0], yhi = cy[0], xlo = cx[0], xhi = cx[0];
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            ylo = cy[k] < ylo ? cy[k] : ylo; yhi = cy[k] > yhi ? cy[k] : yhi;
            xlo = cx[k] < xlo ? cx[k] : xlo; xhi = cx[k] > xhi ? cx[k] : xhi;
        }
        int64_t y0 = (ylo >> 12) - 1, y1 = (yhi >> 12) + 1, x0 = (xlo >> 12) - 1, x1 = (xhi >> 12) + 1;
        y0 = y0 < 0 ? 0 : y0; x0 = x0 < 0 ? 0 : x0; y1 = y1 > h - 1 ? h - 1 : y1; x1 = x1 > w - 1 ? w - 1 : x1;
        if (y0 <= y1 && x0 <= x1) {
            const u64 eu = 4096ull * (u64)uw, ev = 4096ull * (u64)uh;
            int s = max_ss;
            for (int k = max_ss - 1; k >= 1; --k)
                if ((u64)(k * k) * (u64)uu >= eu * eu && (u64)(k * k) * (u64)vv >= ev * ev) s = k;
            out[0] = 1; out[1] = y0; out[2] = x0; out[3] = y1; out[4] = x1; out[5] = s;
            out[6] = scaled_quotient(suy * uw, uu); out[7] = scaled_quotient(sux * uw, uu);
            out[8] = scaled_quotient(svy * uh, vv); out[9] = scaled_quotient(svx * uh, vv);
        }
    }
#pragma unroll
    for (int k = 0; k < PA_PLAN; ++k) plan[(int64_t)r * PA_PLAN + k] = out[k];
}

// ---- 2. apply ----------------------------------------------------------------------------------------------------------------------
// ((2l + 1) 2048) / s - 2048 for s in 1..4, l < s: the numerator stays below 2^14, where (n * 43691) >> 17 is n / 3
__device__ __forceinline__ int sub_offset(int l, int s) {
    const unsigned n = (unsigned)(2 * l + 1) * 2048u;
    return (int)(s == 3 ? (n * 43691u) >> 17 : n >> (s >> 1)) - 2048;
}
// v / (255 s^2) for s in 1..4: constant divisors, which compile to a multiplication
__device__ __forceinline__ unsigned div_255ss(unsigned v, int s) {
    switch (s) {
        case 1: return v / 255u;
        case 2: return v / (255u * 4u);
        case 3: return v / (255u * 9u);
        default: return v / (255u * 16u);
    }
}

// block b: tile (b / tiles_x, b % tiles_x); thread tid: page pixel (16 ty + (tid >> 4), 16 tx + (tid & 15))
__global__ __launch_bounds__(PA_THREADS) void paste_apply_kernel(uint8_t* __restrict__ page, int h, int w, const int* __restrict__ info,
                                                                 const int* __restrict__ n_rows, int max_rows, const uint8_t* __restrict__ slots,
                                                                 int ch, int cw, int tiles_x, const int64_t* __restrict__ plan) {
    __shared__ int4 box[PA_CHUNK];                       // y0, x0, y1, x1 of row base + k where it is live and meets this tile, else (1, 1, 0, 0)
    __shared__ int seen;                                 // 1 + the latest chunk in which some row met this tile
    const int tid = threadIdx.x;
    const int R = clamp_count(n_rows[0], max_rows);
    const int ty0 = (int)(blockIdx.x / tiles_x) * PA_TILE, tx0 = (int)(blockIdx.x % tiles_x) * PA_TILE;
    const int y = ty0 + (tid >> 4), x = tx0 + (tid & 15);
    unsigned pix[3] = {0u, 0u, 0u};
    bool have = false, dirty = false;
    if (tid == 0) seen = 0;
    for (int base = 0, chunk = 1; base < R; base += PA_CHUNK, ++chunk) {
        __syncthreads();                                 // `seen` is cleared; the walk of the chunk before is over
        int4 mine = make_int4(1, 1, 0, 0);
        if (base + tid < R) {
            const int64_t* p = plan + (int64_t)(base + tid) * PA_PLAN;
            if (p[0] != 0 && p[1] < ty0 + PA_TILE && p[3] >= ty0 && p[2] < tx0 + PA_TILE && p[4] >= tx0) {
                mine = make_int4((int)p[1], (int)p[2], (int)p[3], (int)p[4]);
                seen = chunk;                            // every writer of this chunk writes the same value
            }
        }
        box[tid] = mine;
        __syncthreads();
        if (seen != chunk) continue;                     // the whole block: no row of the chunk meets the tile
        const int count = R - base < PA_CHUNK ? R - base : PA_CHUNK;
        for (int k = 0; k < count; ++k) {
            const int4 b = box[k];
            if (y < b.x || y > b.z || x < b.y || x > b.w) continue;
            const int r = base + k;
            const int64_t* p = plan + (int64_t)r * PA_PLAN;
            const int s = (int)p[5], guy = (int)p[6], gux = (int)p[7], gvy = (int)p[8], gvx = (int)p[9];
            const int* my = info + (int64_t)r * PA_INFO;
            const int uh = my[0], uw = my[1], oy = my[4], ox = my[5];
            const uint8_t* slot = slots + (int64_t)r * ch * cw * 4;
            unsigned sum[3] = {0u, 0u, 0u}, sum_a = 0u;
            for (int l = 0; l < s; ++l) {
                const int dpy = 4096 * y + sub_offset(l, s) - oy;
                const int64_t au = (int64_t)dpy * guy, av = (int64_t)dpy * gvy;
                for (int m = 0; m < s; ++m) {
                    const int dpx = 4096 * x + sub_offset(m, s) - ox;
                    const int64_t qx = ((au + (int64_t)dpx * gux) >> 16) - 128, qy = ((av + (int64_t)dpx * gvx) >> 16) - 128;
                    if (qx < -256 || qx >= 256ll * uw || qy < -256 || qy >= 256ll * uh) continue;      // all four neighbours outside
                    const int j0 = (int)qx >> 8, i0 = (int)qy >> 8;
                    const unsigned fx = (unsigned)((int)qx & 255), fy = (unsigned)((int)qy & 255);
                    unsigned tc[3] = {0u, 0u, 0u}, ta = 0u;
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int i = i0 + e;
                        if (i < 0 || i >= uh) continue;
#pragma unroll
                        for (int g = 0; g < 2; ++g) {
                            const int j = j0 + g;
                            if (j < 0 || j >= uw) continue;
                            uint32_t rgba;
                            memcpy(&rgba, slot + ((int64_t)i * cw + j) * 4, 4);
                            const unsigned wa = (e ? fy : 256u - fy) * (g ? fx : 256u - fx) * (rgba >> 24);
                            ta += wa;
                            tc[0] += wa * (rgba & 255u); tc[1] += wa * ((rgba >> 8) & 255u); tc[2] += wa * ((rgba >> 16) & 255u);
                        }
                    }
                    sum_a += (ta + 32768u) >> 16;
#pragma unroll
                    for (int c = 0; c < 3; ++c) sum[c] += (tc[c] + 32768u) >> 16;
                }
            }
            if (sum_a == 0u) continue;
            if (!have) {
                const uint8_t* src = page + ((int64_t)y * w + x) * 3;
                pix[0] = src[0]; pix[1] = src[1]; pix[2] = src[2];
                have = true;
            }
            const unsigned den = 255u * (unsigned)(s * s);
#pragma unroll
            for (int c = 0; c < 3; ++c) pix[c] = div_255ss(sum[c] + pix[c] * (den - sum_a) + den / 2u, s);
            dirty = true;
        }
    }
    if (dirty) {
        uint8_t* dst = page + ((int64_t)y * w + x) * 3;
        dst[0] = (uint8_t)pix[0]; dst[1] = (uint8_t)pix[1]; dst[2] = (uint8_t)pix[2];
    }
}

}  // namespace tsii

using namespace tsii;

extern "C" int tsii_region_paste(uint8_t* page, int h, int w, const int* info, const int* n_rows, int max_rows, const uint8_t* slots, int ch,
                                 int cw, int max_ss, int64_t* plan, void* stream) {
    TSII_REQUIRE(page && info && n_rows && slots && plan, "region_paste: null pointer");
    TSII_REQUIRE(h >= 1 && h <= 32767 && w >= 1 && w <= 32767, "region_paste: page of %d x %d pixels (sides 1..32767)", h, w);
    TSII_REQUIRE(max_rows >= 1, "region_paste: max_rows %d (>= 1)", max_rows);
    TSII_REQUIRE(ch >= 1 && ch <= 4096 && cw >= 1 && cw <= 4096, "region_paste: slots of %d x %d pixels (sides 1..4096)", ch, cw);
    TSII_REQUIRE(max_ss >= 1 && max_ss <= PA_MAX_SS, "region_paste: max_ss %d (1..%d)", max_ss, PA_MAX_SS);
    TSII_REQUIRE((reinterpret_cast<uintptr_t>(plan) & 7u) == 0, "region_paste: plan must be 8-byte aligned");
    TSII_REQUIRE((reinterpret_cast<uintptr_t>(info) & 3u) == 0 && (reinterpret_cast<uintptr_t>(n_rows) & 3u) == 0,
                 "region_paste: info and n_rows must be 4-byte aligned");
    const int tiles_x = cdiv(w, PA_TILE), tiles = tiles_x * cdiv(h, PA_TILE);      // at most 2048 x 2048
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(paste_plan_kernel, dim3((unsigned)cdiv64(max_rows, PA_THREADS)), dim3(PA_THREADS), 0, st, info, n_rows, max_rows, h, w, ch, cw,
                       max_ss, plan);
    hipLaunchKernelGGL(paste_apply_kernel, dim3((unsigned)tiles), dim3(PA_THREADS), 0, st, page, h, w, info, n_rows, max_rows, slots, ch, cw, tiles_x,
                       plan);
    return check_launch("region_paste");
}
