// K14: harmonic fill (include/tsii_hip.h, "harmonic fill"): the holes of an image are filled with the smooth continuation of the valid
// pixels around them -- Laplace's equation with the valid pixels as the boundary, solved in ONE coarse-to-fine pass: a pyramid of means
// of the valid pixels up to 1 x 1, then, level by level back down, every hole starts from its relaxed parent and takes `sweeps` Jacobi
// sweeps.  No net, no checkpoint, no atomics; every hole value is a convex combination of valid inputs.
//
//   pull:  level l -> l + 1: a thread owns two coarse pixels of a row = 4 x 2 fine pixels, read as 16-byte vectors where the
//          12-byte pixels of the row start on a 16-byte line (w % 4 == 0); values and validity bytes of level l + 1 go to ws.
//   apex:  ONE workgroup per image starts at the first level of at most 64 x 64 pixels and holds that level and everything above it in
//          LDS: the remaining pulls, the 1 x 1 apex and every push and sweep back down to its first level, which it writes once.
//          An image of at most 64 x 64 pixels is finished by this kernel alone.
//   push:  one launch per remaining level down to level 0.  A block owns 32 x 64 pixels and stages them with an apron of `sweeps`
//          pixels (holes take their parent's relaxed value), runs all sweeps on an LDS ping-pong pair and writes its patch.  After s
//          sweeps a pixel depends on pixels within Manhattan distance s only, so the patch is exactly what a sweep over the whole level
//          gives: sweep k is computed on the patch grown by sweeps - k and reads the patch grown by sweeps - k + 1.  A block whose patch
//          has no hole decides so from the validity alone and only copies (level 0) or does nothing (coarser levels).
//
// The relaxed level u_l lives in the buffer of v_l: a push writes HOLE pixels only and every reader takes hole pixels from the parent
// level, never from that buffer, so blocks of one launch do not depend on each other.  All means are taken in one fixed order
// (mean_of) by every kernel: the result does not depend on the blocking, a batch image equals the image run alone, two runs agree.
// Values are SELECTED by validity, never multiplied by it: a NaN under a hole is never read.
#include "tsii_common.h"

#include <string.h>

namespace tsii {

constexpr int HF_THREADS = 256;
constexpr int HF_PH = 32, HF_PW = 64;                   // the patch of a push block
constexpr int HF_MAX_SWEEPS = 16;
constexpr int HF_APEX = 64;                             // the apex kernel starts at the first level of at most HF_APEX x HF_APEX pixels
constexpr int HF_APEX_PIX = 5461;                       // 64^2 + 32^2 + ... + 1: that level and everything above it
constexpr int HF_MAX_LEVELS = 32;

struct HfLevels {
    int L;                                              // level L is 1 x 1
    int h[HF_MAX_LEVELS], w[HF_MAX_LEVELS];
    size_t voff[HF_MAX_LEVELS], moff[HF_MAX_LEVELS];    // byte offsets into ws of levels 1 .. L (values, then validity bytes)
    size_t bytes;
};

static inline bool hf_geometry(int n, int h, int w) {
    return n >= 1 && h >= 1 && w >= 1 && (int64_t)n * h * w * 3 <= (1ll << 31);
}

static inline HfLevels hf_levels(int n, int h, int w) {
    HfLevels lv;
    lv.L = 0; lv.h[0] = h; lv.w[0] = w; lv.voff[0] = lv.moff[0] = 0;
    while (lv.h[lv.L] > 1 || lv.w[lv.L] > 1) {
        lv.h[lv.L + 1] = (lv.h[lv.L] + 1) / 2; lv.w[lv.L + 1] = (lv.w[lv.L] + 1) / 2;
        ++lv.L;
    }
    size_t off = 0;
    for (int l = 1; l <= lv.L; ++l) {                   // every level starts on a 16-byte line
        lv.voff[l] = off;
        off += ((size_t)n * lv.h[l] * lv.w[l] * 3 * sizeof(float) + 15) & ~(size_t)15;
    }
    for (int l = 1; l <= lv.L; ++l) {
        lv.moff[l] = off;
        off += ((size_t)n * lv.h[l] * lv.w[l] + 15) & ~(size_t)15;
    }
    lv.bytes = off > 16 ? off : 16;
    return lv;
}

// validity of a pixel of a level: the fp32 plane of level 0 (valid iff != 0) or the bytes of a coarser level
struct HfValid {
    const float* f;
    const uint8_t* b;
};
__device__ __forceinline__ bool hf_valid(const HfValid& m, int64_t p) { return m.f != nullptr ? m.f[p] != 0.f : m.b[p] != 0; }

// THE mean of the library: up to four terms added in the order given, divided by their count (cnt >= 1)
__device__ __forceinline__ float mean_of(float a, bool ha, float b, bool hb, float c, bool hc, float d, bool hd) {
    float s = 0.f;
    int cnt = 0;
    if (ha) { s = a; cnt = 1; }
    if (hb) { s = cnt ? s + b : b; ++cnt; }
    if (hc) { s = cnt ? s + c : c; ++cnt; }
    if (hd) { s = cnt ? s + d : d; ++cnt; }
    return s / (float)cnt;
}

// ---- pull: level l -> l + 1 -------------------------------------------------------------------------------------------------------
// thread = coarse pixels (i, 2 jp) and (i, 2 jp + 1) of one image
__global__ __launch_bounds__(HF_THREADS) void hf_pull_kernel(const float* __restrict__ v, HfValid m, int n, int h, int w, int hc, int wc,
                                                             float* __restrict__ vc, uint8_t* __restrict__ mc, int vec_ok) {
    const int wp = (wc + 1) >> 1;
    const int64_t total = (int64_t)n * hc * wp;
    for (int64_t t = (int64_t)blockIdx.x * HF_THREADS + threadIdx.x; t < total; t += (int64_t)gridDim.x * HF_THREADS) {
        const int jp = (int)(t % wp);
        const int i = (int)((t / wp) % hc);
        const int64_t img = t / ((int64_t)wp * hc);
        const int y0 = 2 * i, x0 = 4 * jp;
        float px[2][4][3];
        bool ok[2][4];
        if (vec_ok && y0 + 1 < h && x0 + 3 < w && m.f != nullptr) {     // 2 rows of 4 whole pixels: 48 bytes on a 16-byte line each
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int64_t p = (img * h + y0 + r) * w + x0;
                const float4 a = *reinterpret_cast<const float4*>(v + p * 3), b = *reinterpret_cast<const float4*>(v + p * 3 + 4),
                             c = *reinterpret_cast<const float4*>(v + p * 3 + 8), k = *reinterpret_cast<const float4*>(m.f + p);
                px[r][0][0] = a.x; px[r][0][1] = a.y; px[r][0][2] = a.z; px[r][1][0] = a.w; px[r][1][1] = b.x; px[r][1][2] = b.y;
                px[r][2][0] = b.z; px[r][2][1] = b.w; px[r][2][2] = c.x; px[r][3][0] = c.y; px[r][3][1] = c.z; px[r][3][2] = c.w;
                ok[r][0] = k.x != 0.f; ok[r][1] = k.y != 0.f; ok[r][2] = k.z != 0.f; ok[r][3] = k.w != 0.f;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bool in = y0 + r < h && x0 + q < w;
                    const int64_t p = in ? (img * h + y0 + r) * w + x0 + q : 0;
                    ok[r][q] = in && hf_valid(m, p);
#pragma unroll
                    for (int c = 0; c < 3; ++c) px[r][q][c] = ok[r][q] ? v[p * 3 + c] : 0.f;
                }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int j = 2 * jp + q;
            if (j >= wc) continue;
            const bool a = ok[0][2 * q], b = ok[0][2 * q + 1], c = ok[1][2 * q], d = ok[1][2 * q + 1];
            const int64_t pc = (img * hc + i) * wc + j;
            const bool any = a || b || c || d;
            mc[pc] = any ? 1 : 0;
            if (any) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    vc[pc * 3 + ch] = mean_of(px[0][2 * q][ch], a, px[0][2 * q + 1][ch], b, px[1][2 * q][ch], c, px[1][2 * q + 1][ch], d);
            }
        }
    }
}

// ---- apex: one workgroup per image, everything from its first level up in LDS -----------------------------------------------------
__device__ __forceinline__ int hf_dim(int d, int l) { return (d + (1 << l) - 1) >> l; }          // l ceil-halvings of d
__device__ __forceinline__ int hf_off(int h, int w, int l) {                                      // pixels of the levels below l
    int o = 0;
    for (int k = 0; k < l; ++k) o += hf_dim(h, k) * hf_dim(w, k);
    return o;
}

// src / m: the first level [n, h, w, 3] / its validity; dst: where its relaxed values go -- all pixels (write_all: level 0 -> out) or the
// hole pixels only (the level's own buffer in ws)
__global__ __launch_bounds__(HF_THREADS) void hf_apex_kernel(const float* __restrict__ src, HfValid m, int h, int w, int sweeps,
                                                             float* dst, int write_all) {
    __shared__ float pv[HF_APEX_PIX * 3];               // the pyramid's values ...
    __shared__ float nxt[HF_APEX * HF_APEX * 3];        // ... a sweep's new hole values ...
    __shared__ uint8_t pm[HF_APEX_PIX + 3];             // ... and validity
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * h * w;
    int nl = 1;
    while (hf_dim(h, nl - 1) > 1 || hf_dim(w, nl - 1) > 1) ++nl;                                  // levels 0 .. nl - 1 of this kernel
    for (int i = tid; i < h * w; i += HF_THREADS) {
        const bool ok = hf_valid(m, base + i);
        pm[i] = ok ? 1 : 0;
        if (ok) {
#pragma unroll
            for (int c = 0; c < 3; ++c) pv[i * 3 + c] = src[(base + i) * 3 + c];
        }
    }
    __syncthreads();
    for (int l = 0; l + 1 < nl; ++l) {                  // pulls
        const int hl = hf_dim(h, l), wl = hf_dim(w, l), hc = hf_dim(h, l + 1), wc = hf_dim(w, l + 1);
        const int o = hf_off(h, w, l), oc = o + hl * wl;
        for (int i = tid; i < hc * wc; i += HF_THREADS) {
            const int y = 2 * (i / wc), x = 2 * (i % wc);
            const int p = o + y * wl + x;
            const bool right = x + 1 < wl, down = y + 1 < hl;
            const bool a = pm[p] != 0, b = right && pm[p + 1] != 0, c = down && pm[p + wl] != 0, d = right && down && pm[p + wl + 1] != 0;
            const bool any = a || b || c || d;
            pm[oc + i] = any ? 1 : 0;
            if (any) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    pv[(oc + i) * 3 + ch] = mean_of(a ? pv[p * 3 + ch] : 0.f, a, b ? pv[(p + 1) * 3 + ch] : 0.f, b,
                                                    c ? pv[(p + wl) * 3 + ch] : 0.f, c, d ? pv[(p + wl + 1) * 3 + ch] : 0.f, d);
            }
        }
        __syncthreads();
    }
    if (tid < 3 && pm[hf_off(h, w, nl - 1)] == 0) pv[hf_off(h, w, nl - 1) * 3 + tid] = 0.f;       // the apex of an image without a valid pixel
    __syncthreads();
    for (int l = nl - 2; l >= 0; --l) {                 // pushes and sweeps
        const int hl = hf_dim(h, l), wl = hf_dim(w, l), wc = hf_dim(w, l + 1);
        const int o = hf_off(h, w, l), oc = o + hl * wl;
        for (int i = tid; i < hl * wl; i += HF_THREADS) {
            if (pm[o + i] != 0) continue;
            const int pc = oc + (i / wl >> 1) * wc + (i % wl >> 1);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) pv[(o + i) * 3 + ch] = pv[pc * 3 + ch];
        }
        __syncthreads();
        for (int s = 0; s < sweeps; ++s) {
            for (int i = tid; i < hl * wl; i += HF_THREADS) {
                if (pm[o + i] != 0) continue;
                const int y = i / wl, x = i % wl, p = o + i;
                const bool up = y > 0, down = y + 1 < hl, left = x > 0, right = x + 1 < wl;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    nxt[i * 3 + ch] = mean_of(up ? pv[(p - wl) * 3 + ch] : 0.f, up, down ? pv[(p + wl) * 3 + ch] : 0.f, down,
                                              left ? pv[(p - 1) * 3 + ch] : 0.f, left, right ? pv[(p + 1) * 3 + ch] : 0.f, right);
            }
            __syncthreads();
            for (int i = tid; i < hl * wl; i += HF_THREADS) {      // (every level below the apex has 2 pixels or more: a neighbour)
                if (pm[o + i] != 0) continue;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) pv[(o + i) * 3 + ch] = nxt[i * 3 + ch];
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < h * w; i += HF_THREADS) {
        if (!write_all && pm[i] != 0) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[(base + i) * 3 + c] = pv[i * 3 + c];
    }
}

// ---- push and relax: one level, a block per 32 x 64 patch -------------------------------------------------------------------------------
enum { HF_ABSENT = 0, HF_VALID = 1, HF_HOLE = 2 };

// src / m: v_l and its validity; par: u_{l+1} [n, hp, wp, 3]; dst: all pixels of the patch (write_all: level 0 -> out, never src) or
// the hole pixels only (dst == src, the level's own buffer).  S: the widest apron this instance has LDS for.
template <int S>
__global__ __launch_bounds__(HF_THREADS) void hf_push_kernel(const float* src, HfValid m, const float* __restrict__ par, int h, int w, int hp,
                                                             int wp, int nbx, int nby, int sweeps, float* dst, int write_all, int vec_ok) {
    constexpr int CELLS = (HF_PH + 2 * S) * (HF_PW + 2 * S);
    __shared__ float bufa[CELLS * 3], bufb[CELLS * 3];
    __shared__ uint8_t st[CELLS];
    __shared__ int any_hole;
    const int tid = threadIdx.x;
    const int bx = blockIdx.x % nbx, by = (blockIdx.x / nbx) % nby;
    const int64_t img = blockIdx.x / (nbx * nby);
    const int y0 = by * HF_PH, x0 = bx * HF_PW;
    const int64_t base = img * h * w;
    if (tid == 0) any_hole = 0;
    __syncthreads();
    {
        bool hole = false;
        for (int j = tid; j < HF_PH * HF_PW; j += HF_THREADS) {
            const int y = y0 + j / HF_PW, x = x0 + j % HF_PW;
            if (y < h && x < w && !hf_valid(m, base + (int64_t)y * w + x)) hole = true;
        }
        if (hole) any_hole = 1;
    }
    __syncthreads();
    if (any_hole == 0) {                                // the whole block: nothing to relax
        if (!write_all) return;
        if (vec_ok && x0 + HF_PW <= w) {                // rows of 64 pixels = 48 16-byte vectors on a 16-byte line
            for (int j = tid; j < HF_PH * 48; j += HF_THREADS) {
                const int y = y0 + j / 48;
                if (y >= h) break;
                const int64_t e = (base + (int64_t)y * w + x0) * 3 + 4 * (j % 48);
                *reinterpret_cast<float4*>(dst + e) = *reinterpret_cast<const float4*>(src + e);
            }
        } else {
            const int pw = w - x0 < HF_PW ? w - x0 : HF_PW;
            for (int j = tid; j < HF_PH * pw * 3; j += HF_THREADS) {
                const int y = y0 + j / (pw * 3);
                if (y >= h) break;
                const int64_t e = (base + (int64_t)y * w + x0) * 3 + j % (pw * 3);
                dst[e] = src[e];
            }
        }
        return;
    }
    const int a = sweeps, sh = HF_PH + 2 * a, sw = HF_PW + 2 * a;
    for (int j = tid; j < sh * sw; j += HF_THREADS) {   // stage the patch and its apron
        const int y = y0 - a + j / sw, x = x0 - a + j % sw;
        int s = HF_ABSENT;
        if (y >= 0 && y < h && x >= 0 && x < w) {
            const int64_t p = base + (int64_t)y * w + x;
            const bool ok = hf_valid(m, p);
            s = ok ? HF_VALID : HF_HOLE;
            const float* from = ok ? src + p * 3 : par + ((img * hp + (y >> 1)) * wp + (x >> 1)) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) bufa[j * 3 + c] = bufb[j * 3 + c] = from[c];
        }
        st[j] = (uint8_t)s;
    }
    __syncthreads();
    float* cur = bufa;
    float* nxt = bufb;
    for (int k = 1; k <= a; ++k) {                      // sweep k: the patch grown by a - k, from the patch grown by a - k + 1
        const int rh = sh - 2 * k, rw = sw - 2 * k;
        for (int j = tid; j < rh * rw; j += HF_THREADS) {
            const int q = (k + j / rw) * sw + k + j % rw;
            if (st[q] != HF_HOLE) continue;
            const bool up = st[q - sw] != HF_ABSENT, down = st[q + sw] != HF_ABSENT, left = st[q - 1] != HF_ABSENT, right = st[q + 1] != HF_ABSENT;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                nxt[q * 3 + c] = mean_of(up ? cur[(q - sw) * 3 + c] : 0.f, up, down ? cur[(q + sw) * 3 + c] : 0.f, down,
                                         left ? cur[(q - 1) * 3 + c] : 0.f, left, right ? cur[(q + 1) * 3 + c] : 0.f, right);
        }
        __syncthreads();
        float* t = cur; cur = nxt; nxt = t;
    }
    for (int j = tid; j < HF_PH * HF_PW; j += HF_THREADS) {
        const int r = j / HF_PW, c = j % HF_PW, y = y0 + r, x = x0 + c;
        if (y >= h || x >= w) continue;
        const int q = (a + r) * sw + a + c;
        if (!write_all && st[q] != HF_HOLE) continue;
        const int64_t e = (base + (int64_t)y * w + x) * 3;
        dst[e] = cur[q * 3]; dst[e + 1] = cur[q * 3 + 1]; dst[e + 2] = cur[q * 3 + 2];
    }
}

}  // namespace tsii

using namespace tsii;

extern "C" size_t tsii_harmonic_fill_ws_bytes(int n, int h, int w) {
    if (!hf_geometry(n, h, w)) return 0;
    return hf_levels(n, h, w).bytes;
}

extern "C" int tsii_harmonic_fill(const float* x, const float* mask, int n, int h, int w, int sweeps, float* out, void* ws, void* stream) {
    TSII_REQUIRE(x && mask && out && ws, "harmonic_fill: null pointer");
    TSII_REQUIRE(hf_geometry(n, h, w), "harmonic_fill: %d images of %d x %d pixels (n, h, w >= 1, n * h * w * 3 <= 2^31)", n, h, w);
    TSII_REQUIRE(sweeps >= 0 && sweeps <= HF_MAX_SWEEPS, "harmonic_fill: sweeps %d (0..%d)", sweeps, HF_MAX_SWEEPS);
    TSII_REQUIRE(out != x, "harmonic_fill: out must not be x");
    TSII_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3u) == 0, "harmonic_fill: ws must be 4-byte aligned");
    const HfLevels lv = hf_levels(n, h, w);
    hipStream_t st = (hipStream_t)stream;
    char* wsb = static_cast<char*>(ws);
    const bool ws16 = aligned16(ws);
    auto values = [&](int l) { return reinterpret_cast<float*>(wsb + lv.voff[l]); };
    auto valid = [&](int l) { return l == 0 ? HfValid{mask, nullptr} : HfValid{nullptr, reinterpret_cast<const uint8_t*>(wsb + lv.moff[l])}; };
    int k = 0;                                          // the apex kernel's first level
    while (lv.h[k] > HF_APEX || lv.w[k] > HF_APEX) ++k;
    for (int l = 0; l < k; ++l) {                       // pulls above the apex kernel
        const int64_t items = (int64_t)n * lv.h[l + 1] * ((lv.w[l + 1] + 1) / 2);
        const int vec = l == 0 && lv.w[0] % 4 == 0 && aligned16(x) && aligned16(mask);
        hipLaunchKernelGGL(hf_pull_kernel, dim3(flat_grid(items, HF_THREADS)), dim3(HF_THREADS), 0, st, l == 0 ? x : values(l), valid(l), n, lv.h[l],
                           lv.w[l], lv.h[l + 1], lv.w[l + 1], values(l + 1), reinterpret_cast<uint8_t*>(wsb + lv.moff[l + 1]), vec);
    }
    hipLaunchKernelGGL(hf_apex_kernel, dim3((unsigned)n), dim3(HF_THREADS), 0, st, k == 0 ? x : values(k), valid(k), lv.h[k], lv.w[k], sweeps,
                       k == 0 ? out : values(k), k == 0 ? 1 : 0);
    for (int l = k - 1; l >= 0; --l) {
        const int nbx = cdiv(lv.w[l], HF_PW), nby = cdiv(lv.h[l], HF_PH);
        const unsigned blocks = (unsigned)((int64_t)n * nbx * nby);      // below 2^31 / (32 * 64 * 3) + n
        const float* src = l == 0 ? x : values(l);
        float* dst = l == 0 ? out : values(l);
        const int vec = lv.w[l] % 4 == 0 && (l == 0 ? aligned16(x) && aligned16(out) : ws16);
        if (sweeps <= 4)
            hipLaunchKernelGGL(hf_push_kernel<4>, dim3(blocks), dim3(HF_THREADS), 0, st, src, valid(l), values(l + 1), lv.h[l], lv.w[l], lv.h[l + 1],
                               lv.w[l + 1], nbx, nby, sweeps, dst, l == 0 ? 1 : 0, vec);
        else if (sweeps <= 8)
            hipLaunchKernelGGL(hf_push_kernel<8>, dim3(blocks), dim3(HF_THREADS), 0, st, src, valid(l), values(l + 1), lv.h[l], lv.w[l], lv.h[l + 1],
                               lv.w[l + 1], nbx, nby, sweeps, dst, l == 0 ? 1 : 0, vec);
        else
            hipLaunchKernelGGL(hf_push_kernel<HF_MAX_SWEEPS>, dim3(blocks), dim3(HF_THREADS), 0, st, src, valid(l), values(l + 1), lv.h[l], lv.w[l],
                               lv.h[l + 1], lv.w[l + 1], nbx, nby, sweeps, dst, l == 0 ? 1 : 0, vec);
    }
    return check_launch("harmonic_fill");
}
