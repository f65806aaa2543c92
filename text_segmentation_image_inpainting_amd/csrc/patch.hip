// K21: patch fill (include/tsii_hip.h, "patch fill"): every hole pixel becomes a copy of a page pixel whose (2r+1)^2 neighbourhood matches
// the hole pixel's own -- a PatchMatch-style search of a nearest-neighbour field, coarse to fine, all in integers.  The header's block is
// the definition; this file is one way to compute it:
//
//   pf_pack        W_0: the page (init under the holes) as packed RGBX words, four pixels = one 16-byte store per thread
//   pf_pull        level l -> l+1: rounded means of the children and "some child is a hole"
//   pf_admissible  the erosion of the non-hole plane by 2r+1, separably through an LDS tile
//   pf_init        the field of a level from its parent's (none at the coarsest level)
//   pf_search<R>   one Jacobi iteration: a block owns a 32 x 16 tile, returns if the tile has no hole, stages T (the work image with the
//                  sourced hole pixels replaced by their sources) for the tile and an apron of r in LDS, compacts the tile's hole pixels
//                  into a list (wave scan + wave totals) and gives every lane one hole pixel; a lane walks its candidates, reading the
//                  source windows as rows of 2r+1 words from the packed level, one v_sad_u8 per pixel pair, and drops a candidate after
//                  the first row at which its partial cost exceeds the best so far.  T never goes to memory: there is no apply launch
//   pf_finish      out, nnf and stats at level 0; chunks without a hole copy with 16-byte vectors
//
// The field is stored as the LINEAR index sy * w_l + sx of the source in its image (-1: none): the order of the linear index is the
// lexicographic order of (sy, sx) the definition breaks ties by.  Field words of pixels that are not holes are never read.
#include "tsii_common.h"

namespace tsii {

constexpr int PF_THREADS = 256;
constexpr int PF_TW = 32, PF_TH = 16;                   // the tile of a search / admissible block
constexpr int PF_MAX_RADIUS = 4, PF_MAX_LEVELS = 6, PF_MAX_ITERS = 8;
constexpr int PF_CHUNK = 1024;                          // pixels of a finish block
constexpr uint32_t PF_ABSENT = 0xff000000u;             // a staged cell off the level: the X byte of a pixel word is 0

struct PfLevels {
    int count;
    int h[PF_MAX_LEVELS], w[PF_MAX_LEVELS];
    size_t img[PF_MAX_LEVELS], hole[PF_MAX_LEVELS], adm[PF_MAX_LEVELS], fa[PF_MAX_LEVELS], fb[PF_MAX_LEVELS];
    size_t bytes;
};

static inline bool pf_geometry(int n, int h, int w) {
    return n >= 1 && h >= 1 && w >= 1 && (int64_t)n * h * w * 3 < (1ll << 31);
}
static inline bool pf_params(int radius, int levels) {
    return radius >= 1 && radius <= PF_MAX_RADIUS && levels >= 1 && levels <= PF_MAX_LEVELS;
}
static inline PfLevels pf_levels(int n, int h, int w, int radius, int levels) {
    PfLevels lv;
    lv.count = 0;
    size_t off = 0;
    auto take = [&](size_t nbytes) { const size_t at = off; off += (nbytes + 15) & ~(size_t)15; return at; };
    for (int l = 0, hl = h, wl = w; l < levels; ++l, hl = (hl + 1) / 2, wl = (wl + 1) / 2) {
        if (l > 0 && (hl < wl ? hl : wl) < 2 * radius + 1) break;
        const size_t px = (size_t)n * hl * wl;
        lv.h[l] = hl; lv.w[l] = wl;
        lv.img[l] = take(px * 4);
        lv.hole[l] = l > 0 ? take(px) : 0;              // level 0 reads the caller's plane
        lv.adm[l] = take(px);
        lv.fa[l] = take(px * 4);
        lv.fb[l] = take(px * 4);
        lv.count = l + 1;
    }
    lv.bytes = off;
    return lv;
}

// |a - b| summed over the four bytes of a word, on top of acc
__device__ __forceinline__ unsigned sad4(unsigned a, unsigned b, unsigned acc) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(a, b, acc);
#else
    for (int i = 0; i < 4; ++i) {
        const int d = (int)((a >> (8 * i)) & 0xffu) - (int)((b >> (8 * i)) & 0xffu);
        acc += (unsigned)(d < 0 ? -d : d);
    }
    return acc;
#endif
}

__host__ __device__ __forceinline__ uint32_t pf_mix(uint32_t v) {
    v ^= v >> 16; v *= 0x7feb352du; v ^= v >> 15; v *= 0x846ca68bu; v ^= v >> 16;
    return v;
}

__device__ __forceinline__ bool pf_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__device__ __forceinline__ uint32_t pf_rgbx(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16); }

// ---- W_0: thread = pixels 4 t .. 4 t + 3 of the flat run (vec: every pointer 4-byte aligned, img 16) or pixel t ------------------------
__global__ __launch_bounds__(PF_THREADS) void pf_pack_kernel(const uint8_t* __restrict__ page, const uint8_t* __restrict__ hole,
                                                             const uint8_t* __restrict__ init, int64_t pixels, uint32_t* __restrict__ img, int vec) {
    const int px = vec ? 4 : 1;
    const int64_t items = (pixels + px - 1) / px;
    for (int64_t t = (int64_t)blockIdx.x * PF_THREADS + threadIdx.x; t < items; t += (int64_t)gridDim.x * PF_THREADS) {
        const int64_t p0 = t * px;
        if (vec && p0 + 4 <= pixels) {
            const uint32_t hw = *reinterpret_cast<const uint32_t*>(hole + p0);
            const uint32_t* a = reinterpret_cast<const uint32_t*>(page + p0 * 3);
            uint32_t w0 = a[0], w1 = a[1], w2 = a[2];
            uint32_t v[4] = {w0 & 0xffffffu, (w0 >> 24) | ((w1 & 0xffffu) << 8), (w1 >> 16) | ((w2 & 0xffu) << 16), w2 >> 8};
            if (hw != 0) {                              // init is read under holes only
                const uint32_t* b = reinterpret_cast<const uint32_t*>(init + p0 * 3);
                w0 = b[0]; w1 = b[1]; w2 = b[2];
                const uint32_t u[4] = {w0 & 0xffffffu, (w0 >> 24) | ((w1 & 0xffffu) << 8), (w1 >> 16) | ((w2 & 0xffu) << 16), w2 >> 8};
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if ((hw >> (8 * i)) & 0xffu) v[i] = u[i];
            }
            uint4 o;
            o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
            *reinterpret_cast<uint4*>(img + p0) = o;
        } else {
            for (int64_t p = p0; p < pixels && p < p0 + px; ++p) img[p] = pf_rgbx((hole[p] != 0 ? init : page) + p * 3);
        }
    }
}

// ---- level l -> l + 1: thread = one coarse pixel; vec: w even and src 8-byte aligned, a row pair of children is one 8-byte load -----------
__global__ __launch_bounds__(PF_THREADS) void pf_pull_kernel(const uint32_t* __restrict__ src, const uint8_t* __restrict__ hsrc, int n, int h, int w,
                                                             int hc, int wc, uint32_t* __restrict__ dst, uint8_t* __restrict__ hdst, int vec) {
    const int64_t items = (int64_t)n * hc * wc;
    for (int64_t i = (int64_t)blockIdx.x * PF_THREADS + threadIdx.x; i < items; i += (int64_t)gridDim.x * PF_THREADS) {
        const int X = (int)(i % wc), Y = (int)((i / wc) % hc);
        const int64_t base = (i / ((int64_t)wc * hc)) * h * w;
        unsigned r = 0, g = 0, b = 0, cnt = 0, any = 0;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int y = 2 * Y + dy;
            if (y >= h) continue;
            const int64_t q = base + (int64_t)y * w + 2 * X;
            uint32_t v0, v1 = 0;
            const bool two = 2 * X + 1 < w;
            if (vec) {
                const int2 t = *reinterpret_cast<const int2*>(src + q);
                v0 = (uint32_t)t.x; v1 = (uint32_t)t.y;
            } else {
                v0 = src[q];
                if (two) v1 = src[q + 1];
            }
            r += v0 & 0xffu; g += (v0 >> 8) & 0xffu; b += (v0 >> 16) & 0xffu;
            any |= hsrc[q];
            ++cnt;
            if (two) {
                r += v1 & 0xffu; g += (v1 >> 8) & 0xffu; b += (v1 >> 16) & 0xffu;
                any |= hsrc[q + 1];
                ++cnt;
            }
        }
        const unsigned sh = cnt >> 1, half = cnt >> 1;       // cnt is 1, 2 or 4: (sum + cnt / 2) / cnt is a shift by 0, 1 or 2
        dst[i] = ((r + half) >> sh) | (((g + half) >> sh) << 8) | (((b + half) >> sh) << 16);
        hdst[i] = any != 0 ? 1 : 0;
    }
}

// ---- admissible sources: a block per 32 x 16 tile, the "bad" plane (hole or off the level) with an apron of r, rows then columns --------
__global__ __launch_bounds__(PF_THREADS) void pf_admissible_kernel(const uint8_t* __restrict__ hole, int h, int w, int nbx, int nby, int r,
                                                                   uint8_t* __restrict__ adm) {
    constexpr int MW = PF_TW + 2 * PF_MAX_RADIUS, MH = PF_TH + 2 * PF_MAX_RADIUS;
    __shared__ uint8_t bad[MH * MW];
    __shared__ uint8_t rowbad[MH * PF_TW];
    const int tid = threadIdx.x;
    const int bx = blockIdx.x % nbx, by = (blockIdx.x / nbx) % nby;
    const int64_t base = (int64_t)(blockIdx.x / (nbx * nby)) * h * w;
    const int y0 = by * PF_TH, x0 = bx * PF_TW;
    const int sh = PF_TH + 2 * r, sw = PF_TW + 2 * r;
    for (int j = tid; j < sh * sw; j += PF_THREADS) {
        const int y = y0 - r + j / sw, x = x0 - r + j % sw;
        bad[j] = (y < 0 || y >= h || x < 0 || x >= w || hole[base + (int64_t)y * w + x] != 0) ? 1 : 0;
    }
    __syncthreads();
    for (int j = tid; j < sh * PF_TW; j += PF_THREADS) {
        const int row = j / PF_TW, c = j % PF_TW;
        unsigned b = 0;
        for (int d = 0; d <= 2 * r; ++d) b |= bad[row * sw + c + d];
        rowbad[j] = (uint8_t)b;
    }
    __syncthreads();
    for (int j = tid; j < PF_TH * PF_TW; j += PF_THREADS) {
        const int row = j / PF_TW, c = j % PF_TW, y = y0 + row, x = x0 + c;
        if (y >= h || x >= w) continue;
        unsigned b = 0;
        for (int d = 0; d <= 2 * r; ++d) b |= rowbad[(row + d) * PF_TW + c];
        adm[base + (int64_t)y * w + x] = b ? 0 : 1;
    }
}

// ---- the field a level starts with: thread = one pixel; par == nullptr at the coarsest level --------------------------------------------
__global__ __launch_bounds__(PF_THREADS) void pf_init_kernel(const uint8_t* __restrict__ hole, const uint8_t* __restrict__ adm,
                                                             const int* __restrict__ par, int n, int h, int w, int hp, int wp, int* __restrict__ field) {
    const int64_t items = (int64_t)n * h * w;
    for (int64_t i = (int64_t)blockIdx.x * PF_THREADS + threadIdx.x; i < items; i += (int64_t)gridDim.x * PF_THREADS) {
        int v = -1;
        if (par != nullptr && hole[i] != 0) {
            const int x = (int)(i % w), y = (int)((i / w) % h);
            const int64_t im = i / ((int64_t)w * h);
            const int ps = par[(im * hp + (y >> 1)) * wp + (x >> 1)];
            if (ps >= 0) {
                const int sy = 2 * (ps / wp) + (y & 1), sx = 2 * (ps % wp) + (x & 1);
                if (sy < h && sx < w && adm[(im * h + sy) * w + sx] != 0) v = sy * w + sx;
            }
        }
        field[i] = v;
    }
}

// ---- one Jacobi iteration of one level ------------------------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(PF_THREADS) void pf_search_kernel(const uint32_t* __restrict__ img, const uint8_t* __restrict__ hole,
                                                               const uint8_t* __restrict__ adm, const int* __restrict__ cur, int* __restrict__ nxt,
                                                               int h, int w, int nbx, int nby, uint32_t key) {
    constexpr int SW = PF_TW + 2 * R, SH = PF_TH + 2 * R, D = 2 * R + 1;
    __shared__ uint32_t T[SH * SW];
    __shared__ uint16_t list[PF_TH * PF_TW];
    __shared__ int wave_cnt[PF_THREADS / 64];
    __shared__ int any_hole;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int bx = blockIdx.x % nbx, by = (blockIdx.x / nbx) % nby;
    const int64_t base = (int64_t)(blockIdx.x / (nbx * nby)) * h * w;
    const int y0 = by * PF_TH, x0 = bx * PF_TW;
    if (tid == 0) any_hole = 0;
    __syncthreads();
    const int j0 = 2 * tid;                             // this thread's two pixels of the tile: one row, two columns
    bool mine[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int y = y0 + (j0 + i) / PF_TW, x = x0 + (j0 + i) % PF_TW;
        mine[i] = y < h && x < w && hole[base + (int64_t)y * w + x] != 0;
    }
    if (mine[0] || mine[1]) any_hole = 1;
    __syncthreads();
    if (any_hole == 0) return;                          // the whole block: most of a page has no text
    for (int j = tid; j < SH * SW; j += PF_THREADS) {   // T for the tile and its apron
        const int y = y0 - R + j / SW, x = x0 - R + j % SW;
        uint32_t v = PF_ABSENT;
        if (y >= 0 && y < h && x >= 0 && x < w) {
            const int64_t q = base + (int64_t)y * w + x;
            v = img[q];
            if (hole[q] != 0) {
                const int s = cur[q];
                if (s >= 0) v = img[base + s];
            }
        }
        T[j] = v;
    }
    const int c = (int)mine[0] + (int)mine[1];
    int incl = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    if (lane == 63) wave_cnt[wv] = incl;
    __syncthreads();
    int at = incl - c, total = 0;
#pragma unroll
    for (int k = 0; k < PF_THREADS / 64; ++k) {
        if (k < wv) at += wave_cnt[k];
        total += wave_cnt[k];
    }
    if (mine[0]) list[at++] = (uint16_t)j0;
    if (mine[1]) list[at] = (uint16_t)(j0 + 1);
    __syncthreads();
    const int big = h > w ? h : w;
    for (int i = tid; i < total; i += PF_THREADS) {
        const int j = list[i], ty = j / PF_TW, tx = j % PF_TW, y = y0 + ty, x = x0 + tx;
        const uint32_t* tp = T + ty * SW + tx;          // the window of p starts at the staged cell (ty, tx)
        unsigned best_cost = 0xffffffffu;
        int best = -1;
        auto consider = [&](int sy, int sx) {
            if ((unsigned)sy >= (unsigned)h || (unsigned)sx >= (unsigned)w) return;
            const int s = sy * w + sx;
            if (s == best || adm[base + s] == 0) return;
            const uint32_t* sp = img + base + (int64_t)(sy - R) * w + (sx - R);
            unsigned cost = 0;
            for (int dy = 0; dy < D; ++dy) {
#pragma unroll
                for (int dx = 0; dx < D; ++dx) {
                    const uint32_t t = tp[dy * SW + dx];
                    if ((t >> 24) == 0) cost = sad4(t, sp[dx], cost);
                }
                if (cost > best_cost) return;           // abandoned: the rest only adds
                sp += w;
            }
            if (cost < best_cost || s < best) { best_cost = cost; best = s; }
        };
        const int s0 = cur[base + (int64_t)y * w + x];
        int cy = y, cx = x;
        if (s0 >= 0) {
            cy = s0 / w; cx = s0 % w;
            consider(cy, cx);
        }
        for (int k = 1; k <= 8; k <<= 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ey = e == 2 ? k : (e == 3 ? -k : 0), ex = e == 0 ? k : (e == 1 ? -k : 0);
                const int qy = y + ey, qx = x + ex;
                if (qy < 0 || qy >= h || qx < 0 || qx >= w) continue;
                const int64_t q = base + (int64_t)qy * w + qx;
                if (hole[q] == 0) continue;
                const int s = cur[q];
                if (s >= 0) consider(s / w - ey, s % w - ex);
            }
        }
        const uint32_t hp = pf_mix(pf_mix(key ^ (uint32_t)y) ^ (uint32_t)x);
        for (int jj = 0, rad = big; rad >= 1; ++jj, rad >>= 1) {
            const uint32_t u = pf_mix(hp ^ (0x9e3779b9u * (uint32_t)(jj + 1)));
            const uint64_t m = 2 * (uint64_t)rad + 1;
            const int oy = (int)(((uint64_t)(u & 0xffffu) * m) >> 16) - rad, ox = (int)(((uint64_t)(u >> 16) * m) >> 16) - rad;
            consider(cy + oy, cx + ox);
        }
        nxt[base + (int64_t)y * w + x] = best;
    }
}

// ---- out, nnf, stats: a block per chunk of PF_CHUNK pixels of one image ---------------------------------------------------------------
// init and out are not restrict: they may be one buffer
__global__ __launch_bounds__(PF_THREADS) void pf_finish_kernel(const uint8_t* __restrict__ page, const uint8_t* __restrict__ hole,
                                                               const uint8_t* init, const int* __restrict__ field, int h, int w,
                                                               int chunks, uint8_t* out, int* __restrict__ nnf, int* __restrict__ stats) {
    __shared__ int any_hole;
    __shared__ int counts[2];
    const int tid = threadIdx.x;
    const int im = blockIdx.x / chunks;
    const int64_t hw = (int64_t)h * w, base = (int64_t)im * hw, p0 = (int64_t)(blockIdx.x % chunks) * PF_CHUNK;
    const int cnt = (int)(hw - p0 < PF_CHUNK ? hw - p0 : PF_CHUNK);
    if (tid == 0) { any_hole = 0; counts[0] = counts[1] = 0; }
    __syncthreads();
    {
        bool found = false;
        for (int j = tid; j < cnt; j += PF_THREADS) found |= hole[base + p0 + j] != 0;
        if (found) any_hole = 1;
    }
    __syncthreads();
    if (any_hole == 0) {
        const uint8_t* src = page + (base + p0) * 3;
        uint8_t* dst = out + (base + p0) * 3;
        const int nbytes = cnt * 3;
        int done = 0;
        if (pf_aligned16(src) && pf_aligned16(dst)) {
            for (int j = tid; j < nbytes / 16; j += PF_THREADS) reinterpret_cast<uint4*>(dst)[j] = reinterpret_cast<const uint4*>(src)[j];
            done = nbytes / 16 * 16;
        }
        for (int j = done + tid; j < nbytes; j += PF_THREADS) dst[j] = src[j];
        int* f = nnf + (base + p0) * 2;
        done = 0;
        if (pf_aligned16(f)) {
            for (int j = tid; j < cnt / 2; j += PF_THREADS) reinterpret_cast<int4*>(f)[j] = make_int4(-1, -1, -1, -1);
            done = cnt / 2 * 4;
        }
        for (int j = done + tid; j < 2 * cnt; j += PF_THREADS) f[j] = -1;
        return;
    }
    for (int j = tid; j < cnt; j += PF_THREADS) {
        const int64_t p = base + p0 + j;
        const uint8_t* from = page + p * 3;
        int sy = -1, sx = -1;
        if (hole[p] != 0) {
            const int s = field[p];
            atomicAdd(&counts[0], 1);
            if (s >= 0) {
                atomicAdd(&counts[1], 1);
                sy = s / w; sx = s % w;
                from = page + (base + s) * 3;
            } else {
                from = init + p * 3;
            }
        }
        const uint8_t b0 = from[0], b1 = from[1], b2 = from[2];     // out may be init: read before the write
        out[p * 3] = b0; out[p * 3 + 1] = b1; out[p * 3 + 2] = b2;
        nnf[p * 2] = sy; nnf[p * 2 + 1] = sx;
    }
    __syncthreads();
    if (tid == 0) {
        atomicAdd(stats + im * 3, counts[0]);
        atomicAdd(stats + im * 3 + 1, counts[1]);
        atomicAdd(stats + im * 3 + 2, counts[0] - counts[1]);
    }
}

template <int R>
static void pf_launch_search(unsigned blocks, hipStream_t st, const uint32_t* img, const uint8_t* hole, const uint8_t* adm, const int* cur, int* nxt,
                             int h, int w, int nbx, int nby, uint32_t key) {
    hipLaunchKernelGGL(pf_search_kernel<R>, dim3(blocks), dim3(PF_THREADS), 0, st, img, hole, adm, cur, nxt, h, w, nbx, nby, key);
}

}  // namespace tsii

using namespace tsii;

extern "C" size_t tsii_patch_fill_ws_bytes(int n, int h, int w, int radius, int levels) {
    if (!pf_geometry(n, h, w) || !pf_params(radius, levels)) return 0;
    return pf_levels(n, h, w, radius, levels).bytes;
}

extern "C" int tsii_patch_fill(const uint8_t* page, const uint8_t* hole, const uint8_t* init, int n, int h, int w, int radius, int levels,
                               int iters, uint32_t seed, uint8_t* out, int32_t* nnf, int32_t* stats, void* ws, void* stream) {
    TSII_REQUIRE(page && hole && init && out && nnf && stats && ws, "patch_fill: null pointer");
    TSII_REQUIRE(pf_geometry(n, h, w), "patch_fill: %d images of %d x %d pixels (n, h, w >= 1, n * h * w * 3 < 2^31)", n, h, w);
    TSII_REQUIRE(radius >= 1 && radius <= PF_MAX_RADIUS, "patch_fill: radius %d (1..%d)", radius, PF_MAX_RADIUS);
    TSII_REQUIRE(levels >= 1 && levels <= PF_MAX_LEVELS, "patch_fill: levels %d (1..%d)", levels, PF_MAX_LEVELS);
    TSII_REQUIRE(iters >= 1 && iters <= PF_MAX_ITERS, "patch_fill: iters %d (1..%d)", iters, PF_MAX_ITERS);
    TSII_REQUIRE(out != page, "patch_fill: out must not be page");
    TSII_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3u) == 0, "patch_fill: ws must be 4-byte aligned");
    const PfLevels lv = pf_levels(n, h, w, radius, levels);
    hipStream_t st = (hipStream_t)stream;
    char* wsb = static_cast<char*>(ws);
    const bool ws16 = aligned16(ws);
    auto image = [&](int l) { return reinterpret_cast<uint32_t*>(wsb + lv.img[l]); };
    auto holes = [&](int l) { return l == 0 ? hole : reinterpret_cast<const uint8_t*>(wsb + lv.hole[l]); };
    auto admis = [&](int l) { return reinterpret_cast<uint8_t*>(wsb + lv.adm[l]); };
    const int64_t pixels = (int64_t)n * h * w;
    {
        const int vec = ws16 && ((reinterpret_cast<uintptr_t>(page) | reinterpret_cast<uintptr_t>(hole) | reinterpret_cast<uintptr_t>(init)) & 3u) == 0;
        hipLaunchKernelGGL(pf_pack_kernel, dim3(flat_grid(vec ? cdiv64(pixels, 4) : pixels, PF_THREADS)), dim3(PF_THREADS), 0, st, page, hole, init,
                           pixels, image(0), vec);
    }
    for (int l = 0; l + 1 < lv.count; ++l) {
        const int64_t items = (int64_t)n * lv.h[l + 1] * lv.w[l + 1];
        const int vec = ws16 && lv.w[l] % 2 == 0;
        hipLaunchKernelGGL(pf_pull_kernel, dim3(flat_grid(items, PF_THREADS)), dim3(PF_THREADS), 0, st, image(l), holes(l), n, lv.h[l], lv.w[l],
                           lv.h[l + 1], lv.w[l + 1], image(l + 1), reinterpret_cast<uint8_t*>(wsb + lv.hole[l + 1]), vec);
    }
    const int* final_field = nullptr;
    for (int l = lv.count - 1; l >= 0; --l) {
        const int hl = lv.h[l], wl = lv.w[l];
        const int nbx = cdiv(wl, PF_TW), nby = cdiv(hl, PF_TH);
        const unsigned blocks = (unsigned)((int64_t)n * nbx * nby);
        const int64_t items = (int64_t)n * hl * wl;
        int* fa = reinterpret_cast<int*>(wsb + lv.fa[l]);
        int* fb = reinterpret_cast<int*>(wsb + lv.fb[l]);
        hipLaunchKernelGGL(pf_admissible_kernel, dim3(blocks), dim3(PF_THREADS), 0, st, holes(l), hl, wl, nbx, nby, radius, admis(l));
        hipLaunchKernelGGL(pf_init_kernel, dim3(flat_grid(items, PF_THREADS)), dim3(PF_THREADS), 0, st, holes(l), admis(l), final_field, n, hl, wl,
                           l + 1 < lv.count ? lv.h[l + 1] : 1, l + 1 < lv.count ? lv.w[l + 1] : 1, fa);
        for (int t = 1; t <= iters; ++t) {
            const uint32_t key = pf_mix(seed + 0x9e3779b9u * (uint32_t)(16 * l + t));
            switch (radius) {
                case 1: pf_launch_search<1>(blocks, st, image(l), holes(l), admis(l), fa, fb, hl, wl, nbx, nby, key); break;
                case 2: pf_launch_search<2>(blocks, st, image(l), holes(l), admis(l), fa, fb, hl, wl, nbx, nby, key); break;
                case 3: pf_launch_search<3>(blocks, st, image(l), holes(l), admis(l), fa, fb, hl, wl, nbx, nby, key); break;
                default: pf_launch_search<4>(blocks, st, image(l), holes(l), admis(l), fa, fb, hl, wl, nbx, nby, key); break;
            }
            int* t2 = fa; fa = fb; fb = t2;
        }
        final_field = fa;
    }
    if (hipMemsetAsync(stats, 0, (size_t)n * 3 * sizeof(int32_t), st) != hipSuccess) {
        set_error("patch_fill: hipMemsetAsync failed");
        return -2;
    }
    const int chunks = (int)cdiv64((int64_t)h * w, PF_CHUNK);
    hipLaunchKernelGGL(pf_finish_kernel, dim3((unsigned)((int64_t)n * chunks)), dim3(PF_THREADS), 0, st, page, hole, init, final_field, h, w, chunks,
                       out, nnf, stats);
    return check_launch("patch_fill");
}
