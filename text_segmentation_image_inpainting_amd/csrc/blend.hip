// K20: seamless fill (include/tsii_hip.h, "seamless fill"): the output of an inpainting filler is taken into the image in the gradient
// domain -- its gradients inside the holes, its level from the valid pixels around them.  For a hole that is the filler's (clamped) output
// plus the harmonic continuation of its own error on the valid pixels, the membrane correction of Poisson cloning:
//
//   residual:  d = x - clamp(out, 0, 1) on the valid pixels (0 under the holes, where nothing reads it)
//   K14:       c = tsii_harmonic_fill(d, mask, sweeps), the entry point of csrc/harmonic.hip itself, untouched: its bits are K14's
//   apply:     dst = out on the valid pixels, clamp(out, 0, 1) + c under the holes
//
// The two kernels of this file are element-wise streams over the n * h * w pixels of the batch as ONE flat run: four 12-byte pixels are
// three 16-byte vectors on a 16-byte line wherever the pointers are, whatever w is, so a thread owns four pixels (one vector of the
// plane, three of every value tensor) and the last n * h * w % 4 pixels take the scalar path, as everything does behind a pointer that is
// not 16-byte aligned.  Values are SELECTED by validity, never multiplied by it: what x holds under a hole (NaN) reaches nothing.  One
// subtraction and one addition per value, no products: nothing for the compiler to contract.  dst may be out: a thread reads what it
// writes before it writes it and nothing else.
#include "tsii_common.h"

namespace tsii {

constexpr int SF_THREADS = 256;
constexpr int SF_MAX_SWEEPS = 16;

static inline bool sf_geometry(int n, int h, int w) {
    return n >= 1 && h >= 1 && w >= 1 && (int64_t)n * h * w * 3 <= (1ll << 31);
}
static inline size_t sf_plane_bytes(int n, int h, int w) {                      // one [n, h, w, 3] fp32 tensor, up to a 16-byte line
    return ((size_t)n * h * w * 3 * sizeof(float) + 15) & ~(size_t)15;
}

// compose's clamp (NaN passes, as it does through torch.clamp)
__device__ __forceinline__ float sf_clamp(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

__device__ __forceinline__ float sf_residual(float x, float out, bool valid) { return valid ? x - sf_clamp(out) : 0.f; }
__device__ __forceinline__ float sf_apply(float out, float c, bool valid) { return valid ? out : sf_clamp(out) + c; }

// thread = pixels 4 t .. 4 t + 3 of the flat run (VEC) or pixel t
template <bool VEC>
__global__ __launch_bounds__(SF_THREADS) void sf_residual_kernel(const float* __restrict__ x, const float* __restrict__ out,
                                                                 const float* __restrict__ mask, int64_t pixels, float* __restrict__ d) {
    constexpr int PX = VEC ? 4 : 1;
    const int64_t items = (pixels + PX - 1) / PX;
    for (int64_t t = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x; t < items; t += (int64_t)gridDim.x * SF_THREADS) {
        const int64_t p0 = t * PX;
        if (VEC && p0 + 4 <= pixels) {
            const VecF<4> m = vload<4>(mask + p0);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const VecF<4> a = vload<4>(x + p0 * 3 + 4 * q), b = vload<4>(out + p0 * 3 + 4 * q);
                VecF<4> r;
#pragma unroll
                for (int i = 0; i < 4; ++i) r.v[i] = sf_residual(a.v[i], b.v[i], m.v[(4 * q + i) / 3] != 0.f);
                vstore<4>(d + p0 * 3 + 4 * q, r);
            }
        } else {
            for (int64_t p = p0; p < pixels && p < p0 + PX; ++p) {
                const bool valid = mask[p] != 0.f;
#pragma unroll
                for (int c = 0; c < 3; ++c) d[p * 3 + c] = sf_residual(x[p * 3 + c], out[p * 3 + c], valid);
            }
        }
    }
}

// out and dst are not restrict: they may be one buffer
template <bool VEC>
__global__ __launch_bounds__(SF_THREADS) void sf_apply_kernel(const float* out, const float* __restrict__ c, const float* __restrict__ mask,
                                                              int64_t pixels, float* dst) {
    constexpr int PX = VEC ? 4 : 1;
    const int64_t items = (pixels + PX - 1) / PX;
    for (int64_t t = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x; t < items; t += (int64_t)gridDim.x * SF_THREADS) {
        const int64_t p0 = t * PX;
        if (VEC && p0 + 4 <= pixels) {
            const VecF<4> m = vload<4>(mask + p0);
            VecF<4> r[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const VecF<4> a = vload<4>(out + p0 * 3 + 4 * q), b = vload<4>(c + p0 * 3 + 4 * q);
#pragma unroll
                for (int i = 0; i < 4; ++i) r[q].v[i] = sf_apply(a.v[i], b.v[i], m.v[(4 * q + i) / 3] != 0.f);
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) vstore<4>(dst + p0 * 3 + 4 * q, r[q]);
        } else {
            for (int64_t p = p0; p < pixels && p < p0 + PX; ++p) {
                const bool valid = mask[p] != 0.f;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) dst[p * 3 + ch] = sf_apply(out[p * 3 + ch], c[p * 3 + ch], valid);
            }
        }
    }
}

}  // namespace tsii

using namespace tsii;

extern "C" size_t tsii_seamless_fill_ws_bytes(int n, int h, int w) {
    if (!sf_geometry(n, h, w)) return 0;
    return 2 * sf_plane_bytes(n, h, w) + tsii_harmonic_fill_ws_bytes(n, h, w);      // d, c, K14's own
}

extern "C" int tsii_seamless_fill(const float* x, const float* out, const float* mask, int n, int h, int w, int sweeps, float* dst, void* ws,
                                  void* stream) {
    TSII_REQUIRE(x && out && mask && dst && ws, "seamless_fill: null pointer");
    TSII_REQUIRE(sf_geometry(n, h, w), "seamless_fill: %d images of %d x %d pixels (n, h, w >= 1, n * h * w * 3 <= 2^31)", n, h, w);
    TSII_REQUIRE(sweeps >= 0 && sweeps <= SF_MAX_SWEEPS, "seamless_fill: sweeps %d (0..%d)", sweeps, SF_MAX_SWEEPS);
    TSII_REQUIRE(dst != x, "seamless_fill: dst must not be x");
    TSII_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3u) == 0, "seamless_fill: ws must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int64_t pixels = (int64_t)n * h * w;
    const size_t plane = sf_plane_bytes(n, h, w);
    char* wsb = static_cast<char*>(ws);
    float* d = reinterpret_cast<float*>(wsb);
    float* c = reinterpret_cast<float*>(wsb + plane);
    void* hws = wsb + 2 * plane;
    const bool vec = aligned16(x) && aligned16(out) && aligned16(mask) && aligned16(dst) && aligned16(ws);
    const unsigned grid = flat_grid(vec ? cdiv64(pixels, 4) : pixels, SF_THREADS);
    if (vec)
        hipLaunchKernelGGL(sf_residual_kernel<true>, dim3(grid), dim3(SF_THREADS), 0, st, x, out, mask, pixels, d);
    else
        hipLaunchKernelGGL(sf_residual_kernel<false>, dim3(grid), dim3(SF_THREADS), 0, st, x, out, mask, pixels, d);
    const int rc = tsii_harmonic_fill(d, mask, n, h, w, sweeps, c, hws, stream);
    if (rc != 0) return rc;
    if (vec)
        hipLaunchKernelGGL(sf_apply_kernel<true>, dim3(grid), dim3(SF_THREADS), 0, st, out, c, mask, pixels, dst);
    else
        hipLaunchKernelGGL(sf_apply_kernel<false>, dim3(grid), dim3(SF_THREADS), 0, st, out, c, mask, pixels, dst);
    return check_launch("seamless_fill");
}
