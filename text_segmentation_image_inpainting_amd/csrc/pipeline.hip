// K8: page-level text removal around the two networks (include/tsii_hip.h, "page pipeline"): cut a uint8 HWC page into overlapping
// square tiles for the segmenter, turn the tiles' logits into a dilated text plane with per-tile counts, cut the filler's tiles
// (image * mask and the mask plane) for the tiles that have text -- or for windows placed on the text regions by the host -- and
// compose the filler's output back into the page bytes.
// Six streaming kernels: nothing here is arithmetic bound, every choice below is about bytes and the shape of the accesses.
//
// Stores are plain (default cache policy), not non-temporal: every output is read next by another kernel (the nets' first layers,
// the mask kernel, compose), and a whole page's tiles (63 MB at 1170 x 1654, tile 512 / halo 64) fit the 256 MB MALL -- a
// non-temporal store would send the hand-off through HBM.
#include "page_grid.h"

#include <string.h>

namespace tsii {

// mirror reflection without repeating the edge (period 2 (n - 1)); n == 1 -> 0
__device__ __forceinline__ int reflect(int v, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    v %= p;
    if (v < 0) v += p;
    return v < n ? v : p - v;
}

// three 16-byte stores of the 12 floats of 4 NHWC pixels; dst is 16-byte aligned (48-byte pitch from an aligned base)
__device__ __forceinline__ void store12(float* dst, const float (&v)[12]) {
    float4* d = reinterpret_cast<float4*>(dst);
    d[0] = make_float4(v[0], v[1], v[2], v[3]);
    d[1] = make_float4(v[4], v[5], v[6], v[7]);
    d[2] = make_float4(v[8], v[9], v[10], v[11]);
}

// ---- segmenter tiles -------------------------------------------------------------------------------------------------------
// one thread = 4 consecutive pixels of a tile row.  Inside the page (row reflected or not, columns unreflected) the 12 page bytes
// are one span (byte-aligned: read as three unaligned dwords); spans that touch a page edge take the per-pixel path.
__global__ __launch_bounds__(256) void page_tiles_norm_kernel(const uint8_t* __restrict__ page, PageGrid g, int total,
                                                              float sc0, float sc1, float sc2, float sh0, float sh1, float sh2,
                                                              float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int qn = g.tile >> 2;
    const int q = i % qn, r = (i / qn) % g.tile, t = i / (qn * g.tile);
    const int y = (t / g.tx) * g.s - g.halo + r, x0 = (t % g.tx) * g.s - g.halo + 4 * q;
    const uint8_t* row = page + (int64_t)reflect(y, g.h) * g.w * 3;
    uint8_t b[12];
    if (x0 >= 0 && x0 + 3 < g.w) {
        memcpy(b, row + x0 * 3, 12);
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const uint8_t* s = row + reflect(x0 + p, g.w) * 3;
            b[3 * p] = s[0]; b[3 * p + 1] = s[1]; b[3 * p + 2] = s[2];
        }
    }
    float v[12];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        v[3 * p] = fmaf((float)b[3 * p], sc0, sh0);
        v[3 * p + 1] = fmaf((float)b[3 * p + 1], sc1, sh1);
        v[3 * p + 2] = fmaf((float)b[3 * p + 2], sc2, sh2);
    }
    store12(out + (int64_t)i * 12, v);
}

// ---- text mask ---------------------------------------------------------------------------------------------------------------
// A block owns MB_W x MB_H page pixels inside ONE tile core (so its count goes to one tile) plus a ring of r = dilate / 2:
//   1. coalesced logit loads (each pixel from the tile that owns it), thresholded to a byte tile in LDS;
//   2. one thread per row packs the row into 128 bits (8 bytes -> 8 bits with one multiply) and dilates it horizontally:
//      bit c of the result = OR of bits c .. c + 2r, 64 result bits per row;
//   3. one thread per output row ORs 2r + 1 row words, counts the set bits inside the core and the page;
//   4. every lane writes one byte of a 64-byte row segment; the counts meet in wave 0 (__shfl_down) and leave with one atomicAdd.
constexpr int MB_W = 64, MB_H = 32, MB_RMAX = 15, MB_ROWS = MB_H + 2 * MB_RMAX;

__global__ __launch_bounds__(256) void tiles_text_mask_kernel(const float* __restrict__ logits, PageGrid g, float thr, int r,
                                                              int nbx, int nby, uint8_t* __restrict__ text, int* __restrict__ core_count) {
    __shared__ unsigned long long bytes[MB_ROWS][16];   // 128 thresholded pixels per row, one per byte
    __shared__ unsigned long long hrow[MB_ROWS];
    __shared__ unsigned long long vrow[MB_H];
    const int tid = threadIdx.x;
    const int t = blockIdx.x / (nbx * nby), sub = blockIdx.x % (nbx * nby);
    const int ci = t / g.tx, cj = t % g.tx;
    const int y0 = ci * g.s + (sub / nbx) * MB_H, x0 = cj * g.s + (sub % nbx) * MB_W;
    const int yend = (ci + 1) * g.s < g.h ? (ci + 1) * g.s : g.h, xend = (cj + 1) * g.s < g.w ? (cj + 1) * g.s : g.w;
    if (y0 >= yend || x0 >= xend) return;               // the whole block: this part of the core is off the page / past the core
    const int rows = MB_H + 2 * r, cols = MB_W + 2 * r;

    {   // 1. column c of the region is page column x0 - r + c: its owning tile and the column inside that tile are fixed per thread
        const int c = tid & 127, px = x0 - r + c;
        const bool col_ok = c < cols && px >= 0 && px < g.w;
        const int tj = col_ok ? px / g.s : 0;
        const int lx = px - tj * g.s + g.halo;
        uint8_t* bt = reinterpret_cast<uint8_t*>(&bytes[0][0]);
        for (int row = tid >> 7; row < rows; row += 2) {
            const int py = y0 - r + row;
            uint8_t v = 0;
            if (col_ok && py >= 0 && py < g.h) {
                const int ti = py / g.s;
                v = logits[((int64_t)(ti * g.tx + tj) * g.tile + (py - ti * g.s + g.halo)) * g.tile + lx] > thr ? 1 : 0;
            }
            bt[row * 128 + c] = v;
        }
    }
    __syncthreads();
    if (tid < rows) {   // 2.
        unsigned long long lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            lo |= ((bytes[tid][k] * 0x0102040810204080ull) >> 56) << (8 * k);
            hi |= ((bytes[tid][8 + k] * 0x0102040810204080ull) >> 56) << (8 * k);
        }
        unsigned long long acc = lo;
        for (int k = 1; k <= 2 * r; ++k) acc |= (lo >> k) | (hi << (64 - k));
        hrow[tid] = acc;
    }
    __syncthreads();
    int cnt = 0;
    if (tid < MB_H) {   // 3.
        unsigned long long acc = 0;
        for (int k = 0; k <= 2 * r; ++k) acc |= hrow[tid + k];
        vrow[tid] = acc;
        const int nvalid = xend - x0;                   // 1 .. MB_W or more
        const unsigned long long colmask = nvalid >= 64 ? ~0ull : ((1ull << nvalid) - 1ull);
        if (y0 + tid < yend) cnt = __builtin_popcountll(acc & colmask);
    }
    __syncthreads();
    {   // 4.
        const int c = tid & 63;
        if (x0 + c < xend) {
            for (int row = tid >> 6; row < MB_H && y0 + row < yend; row += 4)
                text[(int64_t)(y0 + row) * g.w + x0 + c] = (uint8_t)((vrow[row] >> c) & 1ull);
        }
    }
    if (tid < 64) {     // wave 0 holds every row's count (lanes >= MB_H hold 0)
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) cnt += __shfl_down(cnt, d);
        if (tid == 0 && cnt > 0) atomicAdd(core_count + t, cnt);
    }
}

// ---- filler tiles ------------------------------------------------------------------------------------------------------------
// the same thread shape as the segmenter tiles; outside the page is a hole (mask 0, image 0).  fill_span is thread i's work once it
// knows where its 4 pixels lie on the page: row y, columns x0 .. x0 + 3 (any of them may be off the page)
__device__ __forceinline__ void fill_span(const uint8_t* __restrict__ page, const uint8_t* __restrict__ text, int h, int w, int y, int x0,
                                          int i, float* __restrict__ img, float* __restrict__ mask) {
    uint8_t b[12], tx4[4];
    bool in[4];
    const bool row_in = y >= 0 && y < h;
    if (row_in && x0 >= 0 && x0 + 3 < w) {
        memcpy(b, page + ((int64_t)y * w + x0) * 3, 12);
        memcpy(tx4, text + (int64_t)y * w + x0, 4);
        in[0] = in[1] = in[2] = in[3] = true;
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            in[p] = row_in && x0 + p >= 0 && x0 + p < w;
            const int64_t o = in[p] ? (int64_t)y * w + x0 + p : 0;
            tx4[p] = text[o];
            b[3 * p] = page[o * 3]; b[3 * p + 1] = page[o * 3 + 1]; b[3 * p + 2] = page[o * 3 + 2];
        }
    }
    float v[12], m[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        m[p] = (in[p] && tx4[p] == 0) ? 1.f : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[3 * p + c] = ((float)b[3 * p + c] / 255.0f) * m[p];
    }
    store12(img + (int64_t)i * 12, v);
    reinterpret_cast<float4*>(mask)[i] = make_float4(m[0], m[1], m[2], m[3]);
}

// the listed tiles of the grid
__global__ __launch_bounds__(256) void page_tiles_fill_kernel(const uint8_t* __restrict__ page, const uint8_t* __restrict__ text, PageGrid g,
                                                              const int* __restrict__ tile_ids, int nt, int total,
                                                              float* __restrict__ img, float* __restrict__ mask) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int qn = g.tile >> 2;
    const int q = i % qn, r = (i / qn) % g.tile;
    int t = tile_ids[i / (qn * g.tile)];
    t = t < 0 ? 0 : (t >= nt ? nt - 1 : t);           // a bad id must not become a wild read
    fill_span(page, text, g.h, g.w, (t / g.tx) * g.s - g.halo + r, (t % g.tx) * g.s - g.halo + 4 * q, i, img, mask);
}

// windows whose first pixel comes from a table: any int32 origin, on or off the page.  A coordinate far off the page is brought to
// the nearest one that is still off it for all 4 pixels (-1 / h for the row, -4 / w for the first column), so nothing overflows.
__global__ __launch_bounds__(256) void page_windows_fill_kernel(const uint8_t* __restrict__ page, const uint8_t* __restrict__ text, int h, int w,
                                                                int tile, const int* __restrict__ origin, int total,
                                                                float* __restrict__ img, float* __restrict__ mask) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int qn = tile >> 2;
    const int q = i % qn, r = (i / qn) % tile, k = i / (qn * tile);
    const int64_t y = (int64_t)origin[2 * k] + r, x0 = (int64_t)origin[2 * k + 1] + 4 * q;
    fill_span(page, text, h, w, y < -1 ? -1 : (y > h ? h : (int)y), x0 < -4 ? -4 : (x0 > w ? w : (int)x0), i, img, mask);
}

// ---- compose -----------------------------------------------------------------------------------------------------------------
// one thread = 4 consecutive page pixels in flat order (12 page bytes and 4 text bytes, both dword aligned); the filler's floats
// are touched for text pixels only
__device__ __forceinline__ uint8_t to_u8(float o) {
    return (uint8_t)floorf(fmaf(fminf(fmaxf(o, 0.f), 1.f), 255.f, 0.5f));
}
__device__ __forceinline__ void compose_pixel(const float* __restrict__ out, const int* __restrict__ slot, int n_sel, const PageGrid& g, int pix, uint8_t* rgb) {
    const int y = pix / g.w, x = pix - y * g.w;
    const int ti = y / g.s, tj = x / g.s;
    const int sl = slot[ti * g.tx + tj];
    if (sl < 0 || sl >= n_sel) return;                                 // a tile that was not filled keeps its page bytes
    const float* o = out + (((int64_t)sl * g.tile + (y - ti * g.s + g.halo)) * g.tile + (x - tj * g.s + g.halo)) * 3;
    rgb[0] = to_u8(o[0]); rgb[1] = to_u8(o[1]); rgb[2] = to_u8(o[2]);
}
__global__ __launch_bounds__(256) void compose_page_u8_kernel(const uint8_t* __restrict__ page, const uint8_t* __restrict__ text,
                                                              const float* __restrict__ out, const int* __restrict__ slot, int n_sel, PageGrid g,
                                                              int npix, uint8_t* __restrict__ clean, uint8_t* __restrict__ mask_u8) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int p0 = 4 * i;
    if (p0 >= npix) return;
    if (p0 + 3 < npix) {
        uint8_t b[12], t4[4];
        memcpy(b, __builtin_assume_aligned(page + (int64_t)p0 * 3, 4), 12);
        memcpy(t4, __builtin_assume_aligned(text + p0, 4), 4);
        if (out != nullptr) {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (t4[p]) compose_pixel(out, slot, n_sel, g, p0 + p, b + 3 * p);
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) t4[p] = t4[p] ? 255 : 0;
        memcpy(__builtin_assume_aligned(clean + (int64_t)p0 * 3, 4), b, 12);
        memcpy(__builtin_assume_aligned(mask_u8 + p0, 4), t4, 4);
    } else {
        for (int pix = p0; pix < npix; ++pix) {
            uint8_t b[3] = {page[(int64_t)pix * 3], page[(int64_t)pix * 3 + 1], page[(int64_t)pix * 3 + 2]};
            const uint8_t tv = text[pix];
            if (tv && out != nullptr) compose_pixel(out, slot, n_sel, g, pix, b);
            clean[(int64_t)pix * 3] = b[0]; clean[(int64_t)pix * 3 + 1] = b[1]; clean[(int64_t)pix * 3 + 2] = b[2];
            mask_u8[pix] = tv ? 255 : 0;
        }
    }
}

// the same walk with an ownership table instead of the grid: window k owns the page rectangle rect[k] and the owner of a text pixel
// is the LOWEST k whose rectangle holds it.  The table (6 ints a window) is staged in LDS once per block; it is searched only by
// threads whose 4 text bytes are not all zero.
constexpr int WIN_MAX = 1024;

__device__ __forceinline__ void compose_window_pixel(const float* __restrict__ out, const int* s_rect, const int* s_org, int n, int w, int tile,
                                                     int pix, uint8_t* rgb) {
    const int y = pix / w, x = pix - y * w;
    for (int k = 0; k < n; ++k) {
        if (y < s_rect[4 * k] || x < s_rect[4 * k + 1] || y >= s_rect[4 * k + 2] || x >= s_rect[4 * k + 3]) continue;
        const int64_t ly = (int64_t)y - s_org[2 * k], lx = (int64_t)x - s_org[2 * k + 1];
        if (ly < 0 || ly >= tile || lx < 0 || lx >= tile) return;      // a rectangle that leaves its window must not become a wild read
        const float* o = out + (((int64_t)k * tile + ly) * tile + lx) * 3;
        rgb[0] = to_u8(o[0]); rgb[1] = to_u8(o[1]); rgb[2] = to_u8(o[2]);
        return;
    }
}
__global__ __launch_bounds__(256) void compose_page_windows_u8_kernel(const uint8_t* __restrict__ page, const uint8_t* __restrict__ text,
                                                                      const float* __restrict__ out, const int* __restrict__ origin,
                                                                      const int* __restrict__ rect, int n, int w, int tile, int npix,
                                                                      uint8_t* __restrict__ clean, uint8_t* __restrict__ mask_u8) {
    __shared__ int s_rect[4 * WIN_MAX];
    __shared__ int s_org[2 * WIN_MAX];
    for (int k = threadIdx.x; k < 4 * n; k += blockDim.x) s_rect[k] = rect[k];
    for (int k = threadIdx.x; k < 2 * n; k += blockDim.x) s_org[k] = origin[k];
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int p0 = 4 * i;
    if (p0 >= npix) return;
    if (p0 + 3 < npix) {
        uint8_t b[12], t4[4];
        memcpy(b, __builtin_assume_aligned(page + (int64_t)p0 * 3, 4), 12);
        memcpy(t4, __builtin_assume_aligned(text + p0, 4), 4);
        if (n > 0 && (t4[0] | t4[1] | t4[2] | t4[3])) {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (t4[p]) compose_window_pixel(out, s_rect, s_org, n, w, tile, p0 + p, b + 3 * p);
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) t4[p] = t4[p] ? 255 : 0;
        memcpy(__builtin_assume_aligned(clean + (int64_t)p0 * 3, 4), b, 12);
        memcpy(__builtin_assume_aligned(mask_u8 + p0, 4), t4, 4);
    } else {
        for (int pix = p0; pix < npix; ++pix) {
            uint8_t b[3] = {page[(int64_t)pix * 3], page[(int64_t)pix * 3 + 1], page[(int64_t)pix * 3 + 2]};
            const uint8_t tv = text[pix];
            if (tv && n > 0) compose_window_pixel(out, s_rect, s_org, n, w, tile, pix, b);
            clean[(int64_t)pix * 3] = b[0]; clean[(int64_t)pix * 3 + 1] = b[1]; clean[(int64_t)pix * 3 + 2] = b[2];
            mask_u8[pix] = tv ? 255 : 0;
        }
    }
}

}  // namespace tsii

using namespace tsii;

static inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

extern "C" int tsii_page_tile_count(int h, int w, int tile, int halo) {
    if (!grid_ok(h, w, tile, halo)) return 0;
    const PageGrid g = make_grid(h, w, tile, halo);
    return g.ty * g.tx;
}

extern "C" int tsii_page_tiles_norm(const uint8_t* page, int h, int w, int tile, int halo,
                                    float scale0, float scale1, float scale2, float shift0, float shift1, float shift2,
                                    float* tiles, void* stream) {
    TSII_REQUIRE(page && tiles, "page_tiles_norm: null pointer");
    TSII_REQUIRE(grid_ok(h, w, tile, halo), "page_tiles_norm: bad geometry h %d w %d tile %d halo %d (tile %% 32 == 0, tile > 2 halo)", h, w, tile, halo);
    TSII_REQUIRE(aligned16(tiles), "page_tiles_norm: tiles must be 16-byte aligned");
    const PageGrid g = make_grid(h, w, tile, halo);
    const int total = g.ty * g.tx * tile * (tile / 4);
    hipLaunchKernelGGL(page_tiles_norm_kernel, dim3(flat_grid(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       page, g, total, scale0, scale1, scale2, shift0, shift1, shift2, tiles);
    return check_launch("page_tiles_norm");
}

extern "C" int tsii_tiles_text_mask(const float* logits, int h, int w, int tile, int halo, float logit_threshold, int dilate,
                                    uint8_t* text, int* core_count, void* stream) {
    TSII_REQUIRE(logits && text && core_count, "tiles_text_mask: null pointer");
    TSII_REQUIRE(grid_ok(h, w, tile, halo), "tiles_text_mask: bad geometry h %d w %d tile %d halo %d", h, w, tile, halo);
    TSII_REQUIRE(dilate >= 1 && dilate <= 2 * MB_RMAX + 1 && dilate % 2 == 1, "tiles_text_mask: dilate %d (odd, 1..31)", dilate);
    const PageGrid g = make_grid(h, w, tile, halo);
    const int nt = g.ty * g.tx, nbx = cdiv(g.s, MB_W), nby = cdiv(g.s, MB_H);
    TSII_REQUIRE((int64_t)nt * nbx * nby < (1ll << 31), "tiles_text_mask: page too large");
    if (hipMemsetAsync(core_count, 0, sizeof(int) * (size_t)nt, (hipStream_t)stream) != hipSuccess) return check_launch("tiles_text_mask (memset)");
    hipLaunchKernelGGL(tiles_text_mask_kernel, dim3((unsigned)(nt * nbx * nby)), dim3(256), 0, (hipStream_t)stream,
                       logits, g, logit_threshold, dilate / 2, nbx, nby, text, core_count);
    return check_launch("tiles_text_mask");
}

extern "C" int tsii_page_tiles_fill(const uint8_t* page, const uint8_t* text, int h, int w, int tile, int halo,
                                    const int* tile_ids, int n_sel, float* img, float* mask, void* stream) {
    TSII_REQUIRE(page && text && tile_ids && img && mask, "page_tiles_fill: null pointer");
    TSII_REQUIRE(grid_ok(h, w, tile, halo), "page_tiles_fill: bad geometry h %d w %d tile %d halo %d", h, w, tile, halo);
    const PageGrid g = make_grid(h, w, tile, halo);
    TSII_REQUIRE(n_sel > 0 && n_sel <= g.ty * g.tx, "page_tiles_fill: %d selected tiles of %d", n_sel, g.ty * g.tx);
    TSII_REQUIRE(aligned16(img) && aligned16(mask), "page_tiles_fill: outputs must be 16-byte aligned");
    const int total = n_sel * tile * (tile / 4);
    hipLaunchKernelGGL(page_tiles_fill_kernel, dim3(flat_grid(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       page, text, g, tile_ids, g.ty * g.tx, total, img, mask);
    return check_launch("page_tiles_fill");
}

extern "C" int tsii_compose_page_u8(const uint8_t* page, const uint8_t* text, const float* out, const int* slot, int n_sel,
                                    int h, int w, int tile, int halo, uint8_t* clean, uint8_t* mask_u8, void* stream) {
    TSII_REQUIRE(page && text && clean && mask_u8, "compose_page_u8: null pointer");
    TSII_REQUIRE((out == nullptr) == (slot == nullptr) && (out == nullptr) == (n_sel == 0) && n_sel >= 0, "compose_page_u8: out, slot and n_sel > 0 come together");
    TSII_REQUIRE(grid_ok(h, w, tile, halo), "compose_page_u8: bad geometry h %d w %d tile %d halo %d", h, w, tile, halo);
    TSII_REQUIRE(aligned4(page) && aligned4(text) && aligned4(clean) && aligned4(mask_u8), "compose_page_u8: byte planes must be 4-byte aligned");
    const PageGrid g = make_grid(h, w, tile, halo);
    const int npix = h * w;
    hipLaunchKernelGGL(compose_page_u8_kernel, dim3(flat_grid(cdiv(npix, 4), 256)), dim3(256), 0, (hipStream_t)stream,
                       page, text, out, slot, n_sel, g, npix, clean, mask_u8);
    return check_launch("compose_page_u8");
}

// the page, the tile side and the windows' volume as the grid entry points bound them; halo plays no part
static inline bool windows_ok(int h, int w, int tile) {
    return h > 0 && w > 0 && tile > 0 && tile % 32 == 0 && (int64_t)h * w < (1ll << 31) - 4;
}

extern "C" int tsii_page_windows_fill(const uint8_t* page, const uint8_t* text, int h, int w, int tile, const int* origin, int n,
                                      float* img, float* mask, void* stream) {
    TSII_REQUIRE(page && text && origin && img && mask, "page_windows_fill: null pointer");
    TSII_REQUIRE(windows_ok(h, w, tile), "page_windows_fill: bad geometry h %d w %d tile %d (tile %% 32 == 0)", h, w, tile);
    TSII_REQUIRE(n > 0 && (int64_t)n * tile * (tile / 4) < (1ll << 31), "page_windows_fill: %d windows of %d", n, tile);
    TSII_REQUIRE(aligned16(img) && aligned16(mask), "page_windows_fill: outputs must be 16-byte aligned");
    const int total = n * tile * (tile / 4);
    hipLaunchKernelGGL(page_windows_fill_kernel, dim3(flat_grid(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       page, text, h, w, tile, origin, total, img, mask);
    return check_launch("page_windows_fill");
}

extern "C" int tsii_compose_page_windows_u8(const uint8_t* page, const uint8_t* text, const float* out, const int* origin, const int* rect,
                                            int n, int h, int w, int tile, uint8_t* clean, uint8_t* mask_u8, void* stream) {
    TSII_REQUIRE(page && text && clean && mask_u8, "compose_page_windows_u8: null pointer");
    TSII_REQUIRE(n >= 0 && n <= WIN_MAX, "compose_page_windows_u8: %d windows (at most %d)", n, WIN_MAX);
    TSII_REQUIRE((out == nullptr) == (n == 0) && (origin == nullptr) == (n == 0) && (rect == nullptr) == (n == 0),
                 "compose_page_windows_u8: out, origin, rect and n > 0 come together");
    TSII_REQUIRE(windows_ok(h, w, tile), "compose_page_windows_u8: bad geometry h %d w %d tile %d (tile %% 32 == 0)", h, w, tile);
    TSII_REQUIRE(aligned4(page) && aligned4(text) && aligned4(clean) && aligned4(mask_u8), "compose_page_windows_u8: byte planes must be 4-byte aligned");
    const int npix = h * w;
    hipLaunchKernelGGL(compose_page_windows_u8_kernel, dim3(flat_grid(cdiv(npix, 4), 256)), dim3(256), 0, (hipStream_t)stream,
                       page, text, out, origin, rect, n, w, tile, npix, clean, mask_u8);
    return check_launch("compose_page_windows_u8");
}
