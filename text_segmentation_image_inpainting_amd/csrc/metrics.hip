// K9: validation metrics on the device (include/tsii_hip.h, "K9: validation metrics"): the confusion histograms of a segmenter at
// up to 32 thresholds, the masked error sums of a filler, and per-image SSIM.  Nothing here feeds a gradient; the point is that a
// validation loop leaves the host out of it: integer histograms and a handful of doubles per image are all that ever gets read back.
//
// Determinism ("same batch, same bits"): no floating-point atomics.  Integer counts meet with integer atomics (exact in any
// order); every floating-point sum leaves its block as ONE double and a last kernel adds the blocks' partials in a fixed order
// (strided per thread, then a fixed tree), so a result depends on the inputs and the launch geometry only -- and the geometry is a
// function of the shape.
//
// The first two kernels stream (16-byte loads where rows allow, a scalar form for everything else); SSIM is a stencil: a block
// stages a tile with its 10-pixel ring in LDS, runs the horizontal 11-tap pass for the five moments into LDS, the vertical pass
// from LDS, and forms the SSIM values in registers.
#include "tsii_common.h"

#include <math.h>
#include <string.h>

namespace tsii {

// ---- reductions ---------------------------------------------------------------------------------------------------------------
// the shuffles move 32 bits: a double travels as its two halves
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unsigned u[2];
        memcpy(u, &v, 8);
        u[0] = __shfl_down(u[0], off, 64);
        u[1] = __shfl_down(u[1], off, 64);
        double o;
        memcpy(&o, u, 8);
        v += o;
    }
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// out[row] = scale * sum_i part[row * nb + i]: thread t adds the partials t, t + 256, ... in that order, then a fixed tree
__global__ __launch_bounds__(256) void metric_final_kernel(const double* __restrict__ part, int nb, double scale, double* __restrict__ out) {
    __shared__ double red[256];
    const double* p = part + (int64_t)blockIdx.x * nb;
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) s += p[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0] * scale;
}

// ---- segmentation: confusion histograms ----------------------------------------------------------------------------------------
// A thread keeps, for every threshold j, how many of its pixels (and how many of its TEXT pixels) have logit > thr[j]: 2 K counters
// in registers (the loops are unrolled, the indices static), no LDS traffic per pixel.  With ascending thresholds "exceeds at
// least b of them" is "logit > thr[b - 1]", so the bins are differences of neighbouring counters -- exact integer algebra.  The
// counters meet per wave (shuffles), per block (LDS, integer atomics), and leave as one integer atomic per non-empty bin.
constexpr int CF_KMAX = 32;
struct Thresholds {
    float v[CF_KMAX];
};

__global__ __launch_bounds__(256) void seg_confusion_kernel(const float* __restrict__ logits, const float* __restrict__ target, int64_t hw,
                                                            int bpi, int vec, Thresholds thr, int k, int* __restrict__ hist) {
    __shared__ int ge_all[CF_KMAX + 2], ge_txt[CF_KMAX + 2];   // [b]: pixels exceeding at least b thresholds; [k + 1] = 0
    const int tid = threadIdx.x;
    const int img = blockIdx.x / bpi, blk = blockIdx.x % bpi;
    const float* lg = logits + (int64_t)img * hw;
    const float* tg = target + (int64_t)img * hw;
    if (tid < CF_KMAX + 2) { ge_all[tid] = 0; ge_txt[tid] = 0; }
    int all[CF_KMAX], txt[CF_KMAX], n_all = 0, n_txt = 0;
#pragma unroll
    for (int j = 0; j < CF_KMAX; ++j) { all[j] = 0; txt[j] = 0; }
    auto take = [&](float l, float t) {
        const int is = t > 0.5f ? 1 : 0;
        n_all += 1; n_txt += is;
#pragma unroll
        for (int j = 0; j < CF_KMAX; ++j) {
            if (j < k) {
                const int g = l > thr.v[j] ? 1 : 0;
                all[j] += g; txt[j] += g & is;
            }
        }
    };
    const int64_t stride = (int64_t)bpi * 256;
    if (vec) {      // hw % 4 == 0 and both bases 16-byte aligned: every image starts aligned
        const float4* l4 = reinterpret_cast<const float4*>(lg);
        const float4* t4 = reinterpret_cast<const float4*>(tg);
        for (int64_t i = (int64_t)blk * 256 + tid; i < (hw >> 2); i += stride) {
            const float4 l = l4[i], t = t4[i];
            take(l.x, t.x); take(l.y, t.y); take(l.z, t.z); take(l.w, t.w);
        }
    } else {
        for (int64_t i = (int64_t)blk * 256 + tid; i < hw; i += stride) take(lg[i], tg[i]);
    }
    __syncthreads();                                            // the zeros above
    n_all = wave_sum_i(n_all); n_txt = wave_sum_i(n_txt);
    const bool lead = (tid & 63) == 0;
    if (lead && n_all) { atomicAdd(&ge_all[0], n_all); atomicAdd(&ge_txt[0], n_txt); }
#pragma unroll
    for (int j = 0; j < CF_KMAX; ++j) {
        if (j < k) {
            const int a = wave_sum_i(all[j]), t = wave_sum_i(txt[j]);
            if (lead && a) { atomicAdd(&ge_all[j + 1], a); atomicAdd(&ge_txt[j + 1], t); }
        }
    }
    __syncthreads();
    if (tid < 2 * (k + 1)) {
        const int c = tid / (k + 1), b = tid % (k + 1);
        const int t = ge_txt[b] - ge_txt[b + 1], a = ge_all[b] - ge_all[b + 1];
        const int v = c ? t : a - t;
        if (v) atomicAdd(hist + ((int64_t)img * 2 + c) * (k + 1) + b, v);
    }
}

// ---- inpainting: masked error sums ---------------------------------------------------------------------------------------------
struct ErrAcc {
    int cnt = 0;
    double h1 = 0.0, h2 = 0.0, v1 = 0.0, v2 = 0.0;
    __device__ __forceinline__ void take(float o, float c, float m, int clamp01) {
        if (clamp01) o = fminf(fmaxf(o, 0.f), 1.f);
        const float d = o - c;                                   // the one fp32 rounding; everything after it is double
        const double ad = fabs((double)d), d2 = (double)d * (double)d;
        const bool hole = !(m > 0.5f);
        cnt += hole ? 1 : 0;
        h1 += hole ? ad : 0.0; h2 += hole ? d2 : 0.0;
        v1 += hole ? 0.0 : ad; v2 += hole ? 0.0 : d2;
    }
};

// part[(img * 5 + q) * bpi + blk]; q: hole count, sum |d| holes, sum d^2 holes, sum |d| valid, sum d^2 valid
__device__ __forceinline__ void err_block_out(ErrAcc& a, int img, int bpi, int blk, double* __restrict__ part) {
    __shared__ double wred[4][5];
    const double q[5] = {(double)wave_sum_i(a.cnt), wave_sum_d(a.h1), wave_sum_d(a.h2), wave_sum_d(a.v1), wave_sum_d(a.v2)};
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) wred[threadIdx.x >> 6][i] = q[i];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int i = threadIdx.x;
        part[((int64_t)img * 5 + i) * bpi + blk] = (wred[0][i] + wred[1][i]) + (wred[2][i] + wred[3][i]);
    }
}

// one thread = 4 consecutive pixels = C float4 of each tensor (hw % 4 == 0, 16-byte aligned bases)
template <int C, bool PLANE>
__global__ __launch_bounds__(256) void inpaint_errors_vec_kernel(const float* __restrict__ out, const float* __restrict__ clean,
                                                                 const float* __restrict__ mask, int64_t hw, int bpi, int clamp01,
                                                                 double* __restrict__ part) {
    const int img = blockIdx.x / bpi, blk = blockIdx.x % bpi;
    const float* o = out + (int64_t)img * hw * C;
    const float* c = clean + (int64_t)img * hw * C;
    const float* m = mask + (int64_t)img * hw * (PLANE ? 1 : C);
    ErrAcc acc;
    for (int64_t u = (int64_t)blk * 256 + threadIdx.x; u < (hw >> 2); u += (int64_t)bpi * 256) {
        float ov[4 * C], cv[4 * C], mv[4 * C];
#pragma unroll
        for (int v = 0; v < C; ++v) {
            const VecF<4> a = vload<4>(o + u * 4 * C + 4 * v), b = vload<4>(c + u * 4 * C + 4 * v);
#pragma unroll
            for (int j = 0; j < 4; ++j) { ov[4 * v + j] = a.v[j]; cv[4 * v + j] = b.v[j]; }
        }
        if constexpr (PLANE) {
            const VecF<4> p = vload<4>(m + u * 4);
#pragma unroll
            for (int e = 0; e < 4 * C; ++e) mv[e] = p.v[e / C];
        } else {
#pragma unroll
            for (int v = 0; v < C; ++v) {
                const VecF<4> p = vload<4>(m + u * 4 * C + 4 * v);
#pragma unroll
                for (int j = 0; j < 4; ++j) mv[4 * v + j] = p.v[j];
            }
        }
#pragma unroll
        for (int e = 0; e < 4 * C; ++e) acc.take(ov[e], cv[e], mv[e], clamp01);
    }
    err_block_out(acc, img, bpi, blk, part);
}

// any C, any hw, any alignment: one element per thread and turn
__global__ __launch_bounds__(256) void inpaint_errors_elem_kernel(const float* __restrict__ out, const float* __restrict__ clean,
                                                                  const float* __restrict__ mask, int64_t hw, int ch, int plane, int bpi,
                                                                  int clamp01, double* __restrict__ part) {
    const int img = blockIdx.x / bpi, blk = blockIdx.x % bpi;
    const int64_t ne = hw * ch;
    const float* o = out + (int64_t)img * ne;
    const float* c = clean + (int64_t)img * ne;
    const float* m = mask + (int64_t)img * (plane ? hw : ne);
    ErrAcc acc;
    for (int64_t e = (int64_t)blk * 256 + threadIdx.x; e < ne; e += (int64_t)bpi * 256)
        acc.take(o[e], c[e], m[plane ? e / ch : e], clamp01);
    err_block_out(acc, img, bpi, blk, part);
}

// ---- SSIM ----------------------------------------------------------------------------------------------------------------------
// A block owns SS_W x SS_H window positions (a window is named by its top-left pixel) of one image, all channels:
//   1. the (SS_H + 10) x (SS_W + 10) pixels x C channels of both images go to LDS as they lie in memory (interleaved channels,
//      16-byte loads where the rows allow; zeros beyond the image), each channel MINUS the tile's first pixel of that channel;
//   2. per channel: horizontal pass, one thread = two neighbouring columns of one row (12 LDS reads of each image for 2 x 5 sums);
//   3. vertical pass, one thread = two neighbouring rows of one column (12 LDS reads per moment for two outputs), the SSIM
//      values in double from the fp32 moments, summed per thread in double.
// The shift of step 1 is the shifted-data form of the variance: var and cov do not change when a constant is subtracted, the
// means get it back (mu = shift + mu'), and the cancellation in E[x^2] - mu^2 happens at the size of the tile's VARIATION rather
// than of its values -- on a flat tile every moment is exactly 0.  The shift depends on the tile grid only (same bits each run),
// and it is symmetric in the two images.
constexpr int SS_W = 32, SS_H = 16, SS_R = 10, SS_IW = SS_W + SS_R, SS_IH = SS_H + SS_R;
struct Gauss11 {
    float w[11];
};

template <int C>
__global__ __launch_bounds__(256) void ssim_kernel(const float* __restrict__ a, const float* __restrict__ b, int h, int w, int ntx, int nty,
                                                   int vec, Gauss11 g, double c1, double c2, double* __restrict__ part) {
    constexpr int NV = (SS_IW * C + 3) / 4, RS = 4 * NV + 4;     // floats per staged row (a multiple of 4: 16-byte LDS stores)
    __shared__ float sa[SS_IH * RS], sb[SS_IH * RS];
    __shared__ float mom[5][SS_IH][SS_W + 1];
    __shared__ double wred[4];
    const int tid = threadIdx.x;
    const int tiles = ntx * nty;
    const int img = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int y0 = (tile / ntx) * SS_H, x0 = (tile % ntx) * SS_W;   // < h - 10, < w - 10: the tile's first pixel is in the image
    const int rowlen = w * C;
    const float* ai = a + (int64_t)img * h * rowlen;
    const float* bi = b + (int64_t)img * h * rowlen;
    __shared__ float shift[2][4];
    if (tid < C) {
        shift[0][tid] = ai[(int64_t)y0 * rowlen + x0 * C + tid];
        shift[1][tid] = bi[(int64_t)y0 * rowlen + x0 * C + tid];
    }
    __syncthreads();
    // 1. element e0 + j of a staged row has channel (e0 + j) % C (x0 * C is a multiple of C)
    for (int it = tid; it < SS_IH * NV; it += 256) {
        const int r = it / NV, v = it % NV;
        const int gy = y0 + r, e0 = x0 * C + 4 * v;
        float va[4] = {0.f, 0.f, 0.f, 0.f}, vb[4] = {0.f, 0.f, 0.f, 0.f};
        if (gy < h) {
            const float* ra = ai + (int64_t)gy * rowlen;
            const float* rb = bi + (int64_t)gy * rowlen;
            if (vec && e0 + 3 < rowlen) {
                const VecF<4> pa = vload<4>(ra + e0), pb = vload<4>(rb + e0);
#pragma unroll
                for (int j = 0; j < 4; ++j) { va[j] = pa.v[j]; vb[j] = pb.v[j]; }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (e0 + j < rowlen) { va[j] = ra[e0 + j]; vb[j] = rb[e0 + j]; }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ch = (4 * v + j) % C;
            va[j] -= shift[0][ch]; vb[j] -= shift[1][ch];
        }
        *reinterpret_cast<float4*>(&sa[r * RS + 4 * v]) = make_float4(va[0], va[1], va[2], va[3]);
        *reinterpret_cast<float4*>(&sb[r * RS + 4 * v]) = make_float4(vb[0], vb[1], vb[2], vb[3]);
    }
    __syncthreads();
    const int vq = tid >> 5, vx = tid & 31;                       // vertical pass: rows 2 vq, 2 vq + 1 of column vx
    const bool col_ok = x0 + vx < w - SS_R;
    const bool ok0 = col_ok && y0 + 2 * vq < h - SS_R, ok1 = col_ok && y0 + 2 * vq + 1 < h - SS_R;
    double sum = 0.0;
#pragma unroll 1
    for (int ch = 0; ch < C; ++ch) {
        // 2.
        for (int it = tid; it < SS_IH * (SS_W / 2); it += 256) {
            const int r = it / (SS_W / 2), p = it % (SS_W / 2);
            const float* pa = &sa[r * RS + 2 * p * C + ch];
            const float* pb = &sb[r * RS + 2 * p * C + ch];
            float xa[12], xb[12];
#pragma unroll
            for (int t = 0; t < 12; ++t) { xa[t] = pa[t * C]; xb[t] = pb[t * C]; }
            float m0[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, m1[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 12; ++t) {
                const float aa = xa[t] * xa[t], bb = xb[t] * xb[t], ab = xa[t] * xb[t];
                if (t < 11) {
                    const float wt = g.w[t];
                    m0[0] = fmaf(wt, xa[t], m0[0]); m0[1] = fmaf(wt, xb[t], m0[1]);
                    m0[2] = fmaf(wt, aa, m0[2]); m0[3] = fmaf(wt, bb, m0[3]); m0[4] = fmaf(wt, ab, m0[4]);
                }
                if (t > 0) {
                    const float wt = g.w[t - 1];
                    m1[0] = fmaf(wt, xa[t], m1[0]); m1[1] = fmaf(wt, xb[t], m1[1]);
                    m1[2] = fmaf(wt, aa, m1[2]); m1[3] = fmaf(wt, bb, m1[3]); m1[4] = fmaf(wt, ab, m1[4]);
                }
            }
#pragma unroll
            for (int m = 0; m < 5; ++m) { mom[m][r][2 * p] = m0[m]; mom[m][r][2 * p + 1] = m1[m]; }
        }
        __syncthreads();
        // 3.
        float o0[5], o1[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int t = 0; t < 12; ++t) {
                const float x = mom[m][2 * vq + t][vx];
                if (t < 11) s0 = fmaf(g.w[t], x, s0);
                if (t > 0) s1 = fmaf(g.w[t - 1], x, s1);
            }
            o0[m] = s0; o1[m] = s1;
        }
        auto ssim_of = [&](const float (&o)[5]) {
            const double da = o[0], db = o[1];                   // shifted means
            const double va = (double)o[2] - da * da, vb = (double)o[3] - db * db, cab = (double)o[4] - da * db;
            const double ma = (double)shift[0][ch] + da, mb = (double)shift[1][ch] + db;
            return ((2.0 * ma * mb + c1) * (2.0 * cab + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2));
        };
        if (ok0) sum += ssim_of(o0);
        if (ok1) sum += ssim_of(o1);
        __syncthreads();                                          // mom is rewritten by the next channel
    }
    sum = wave_sum_d(sum);
    if ((tid & 63) == 0) wred[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) part[(int64_t)img * tiles + tile] = (wred[0] + wred[1]) + (wred[2] + wred[3]);
}

static inline int errors_bpi(int64_t hw, int c, bool vec) {
    const int64_t units = vec ? hw / 4 : hw * c;                  // thread turns per image
    int64_t b = cdiv64(units, 256 * (vec ? 4 : 16));
    return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}
static inline bool errors_vec(const void* o, const void* c, const void* m, int64_t hw, int ch) {
    return ch >= 1 && ch <= 4 && hw % 4 == 0 && aligned16(o) && aligned16(c) && aligned16(m);
}
static inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace tsii

using namespace tsii;

extern "C" int tsii_seg_confusion(const float* logits, const float* target, int n, int64_t hw, const float* thresholds, int k,
                                  int* hist, void* stream) {
    TSII_REQUIRE(logits && target && thresholds && hist, "seg_confusion: null pointer");
    TSII_REQUIRE(n > 0 && hw > 0 && hw < (1ll << 31), "seg_confusion: n %d, h*w %lld (1 .. 2^31 - 1 pixels per image)", n, (long long)hw);
    TSII_REQUIRE(k >= 1 && k <= CF_KMAX, "seg_confusion: %d thresholds (1..32)", k);
    Thresholds thr;
    for (int j = 0; j < CF_KMAX; ++j) thr.v[j] = j < k ? thresholds[j] : 0.f;
    for (int j = 0; j < k; ++j)
        TSII_REQUIRE(thr.v[j] == thr.v[j] && (j == 0 || thr.v[j - 1] <= thr.v[j]), "seg_confusion: thresholds must ascend (no NaN)");
    const bool vec = hw % 4 == 0 && aligned16(logits) && aligned16(target);
    const int64_t units = vec ? hw / 4 : hw;
    int64_t bpi = cdiv64(units, 256 * 8);
    bpi = bpi < 1 ? 1 : (bpi > 1024 ? 1024 : bpi);
    TSII_REQUIRE((int64_t)n * bpi < (1ll << 31), "seg_confusion: batch too large");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, sizeof(int) * (size_t)n * 2 * (size_t)(k + 1), st) != hipSuccess) return check_launch("seg_confusion (memset)");
    hipLaunchKernelGGL(seg_confusion_kernel, dim3((unsigned)(n * bpi)), dim3(256), 0, st, logits, target, hw, (int)bpi, vec ? 1 : 0, thr, k, hist);
    return check_launch("seg_confusion");
}

extern "C" size_t tsii_inpaint_errors_ws_bytes(int n, int h, int w, int c) {
    if (n <= 0 || h <= 0 || w <= 0 || c <= 0) return 0;
    return sizeof(double) * 5 * (size_t)n * 256;                  // 5 partials per block, at most 256 blocks per image
}

template <int C>
static void launch_errors_vec(const float* out, const float* clean, const float* mask, int plane, int clamp01, int n, int64_t hw, int bpi,
                              double* part, hipStream_t st) {
    if (plane) hipLaunchKernelGGL(HIP_KERNEL_NAME(inpaint_errors_vec_kernel<C, true>), dim3((unsigned)(n * bpi)), dim3(256), 0, st, out, clean, mask, hw, bpi, clamp01, part);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(inpaint_errors_vec_kernel<C, false>), dim3((unsigned)(n * bpi)), dim3(256), 0, st, out, clean, mask, hw, bpi, clamp01, part);
}

extern "C" int tsii_inpaint_errors(const float* out, const float* clean, const float* mask, int mask_is_plane, int clamp01,
                                   int n, int h, int w, int c, double* sums, void* ws, size_t ws_bytes, void* stream) {
    TSII_REQUIRE(out && clean && mask && sums && ws, "inpaint_errors: null pointer");
    TSII_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0, "inpaint_errors: n %d h %d w %d c %d", n, h, w, c);
    const int64_t hw = (int64_t)h * w;
    TSII_REQUIRE(hw * c < (1ll << 31) && (int64_t)n * 256 < (1ll << 31), "inpaint_errors: image of %lld elements (below 2^31)", (long long)(hw * c));
    TSII_REQUIRE(ws_bytes >= tsii_inpaint_errors_ws_bytes(n, h, w, c) && aligned8(ws) && aligned8(sums), "inpaint_errors: workspace too small or not 8-byte aligned");
    const bool vec = errors_vec(out, clean, mask, hw, c);
    const int bpi = errors_bpi(hw, c, vec);
    double* part = (double*)ws;
    hipStream_t st = (hipStream_t)stream;
    const int pl = mask_is_plane ? 1 : 0, cl = clamp01 ? 1 : 0;
    if (!vec) {
        hipLaunchKernelGGL(inpaint_errors_elem_kernel, dim3((unsigned)(n * bpi)), dim3(256), 0, st, out, clean, mask, hw, c, pl, bpi, cl, part);
    } else if (c == 1) launch_errors_vec<1>(out, clean, mask, pl, cl, n, hw, bpi, part, st);
    else if (c == 2) launch_errors_vec<2>(out, clean, mask, pl, cl, n, hw, bpi, part, st);
    else if (c == 3) launch_errors_vec<3>(out, clean, mask, pl, cl, n, hw, bpi, part, st);
    else launch_errors_vec<4>(out, clean, mask, pl, cl, n, hw, bpi, part, st);
    int rc = check_launch("inpaint_errors");
    if (rc) return rc;
    hipLaunchKernelGGL(metric_final_kernel, dim3((unsigned)(n * 5)), dim3(256), 0, st, (const double*)part, bpi, 1.0, sums);
    return check_launch("inpaint_errors (final)");
}

static inline bool ssim_shape_ok(int n, int h, int w, int c) {
    return n > 0 && h >= 11 && w >= 11 && c >= 1 && c <= 4 && (int64_t)h * w * c < (1ll << 31) &&
           (int64_t)n * cdiv(w - SS_R, SS_W) * cdiv(h - SS_R, SS_H) < (1ll << 31);
}

extern "C" size_t tsii_ssim_ws_bytes(int n, int h, int w, int c) {
    if (!ssim_shape_ok(n, h, w, c)) return 0;
    return sizeof(double) * (size_t)n * cdiv(w - SS_R, SS_W) * cdiv(h - SS_R, SS_H);
}

extern "C" int tsii_ssim(const float* a, const float* b, int n, int h, int w, int c, float data_range, double* ssim, void* ws,
                         size_t ws_bytes, void* stream) {
    TSII_REQUIRE(a && b && ssim && ws, "ssim: null pointer");
    TSII_REQUIRE(ssim_shape_ok(n, h, w, c), "ssim: n %d h %d w %d c %d (h, w >= 11, 1 <= c <= 4)", n, h, w, c);
    TSII_REQUIRE(data_range > 0.f && data_range < __builtin_huge_valf(), "ssim: data_range must be positive and finite");
    TSII_REQUIRE(ws_bytes >= tsii_ssim_ws_bytes(n, h, w, c) && aligned8(ws) && aligned8(ssim), "ssim: workspace too small or not 8-byte aligned");
    Gauss11 g;
    double gw[11], gs = 0.0;
    for (int i = 0; i < 11; ++i) { gw[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); gs += gw[i]; }
    for (int i = 0; i < 11; ++i) g.w[i] = (float)(gw[i] / gs);
    const double L = (double)data_range, c1 = (0.01 * L) * (0.01 * L), c2 = (0.03 * L) * (0.03 * L);
    const int ntx = cdiv(w - SS_R, SS_W), nty = cdiv(h - SS_R, SS_H), tiles = ntx * nty;
    const int vec = ((int64_t)w * c) % 4 == 0 && aligned16(a) && aligned16(b) ? 1 : 0;
    double* part = (double*)ws;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(n * tiles));
    if (c == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(ssim_kernel<1>), grid, dim3(256), 0, st, a, b, h, w, ntx, nty, vec, g, c1, c2, part);
    else if (c == 2) hipLaunchKernelGGL(HIP_KERNEL_NAME(ssim_kernel<2>), grid, dim3(256), 0, st, a, b, h, w, ntx, nty, vec, g, c1, c2, part);
    else if (c == 3) hipLaunchKernelGGL(HIP_KERNEL_NAME(ssim_kernel<3>), grid, dim3(256), 0, st, a, b, h, w, ntx, nty, vec, g, c1, c2, part);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(ssim_kernel<4>), grid, dim3(256), 0, st, a, b, h, w, ntx, nty, vec, g, c1, c2, part);
    int rc = check_launch("ssim");
    if (rc) return rc;
    const double scale = 1.0 / ((double)(h - SS_R) * (double)(w - SS_R) * (double)c);
    hipLaunchKernelGGL(metric_final_kernel, dim3((unsigned)n), dim3(256), 0, st, (const double*)part, tiles, scale, ssim);
    return check_launch("ssim (final)");
}
