// Pieces shared by the split-bf16 GEMM kernels (gemm_split.hip: 4-wave tiles; gemm_pc.hip: producer / consumer form).
#pragma once
#include "gemm_tiles.h"

namespace tsii {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

static constexpr int SPLIT_BK = 32;          // K elements per tile; one LDS row = 32 bf16 = 64 bytes = 4 chunks of 8

// a - b as ONE v_sub_f32 the vectorizer cannot pair into a packed-fp32 instruction
__device__ __forceinline__ float scalar_sub(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    float r;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
#else
    return a - b;
#endif
}

// 8 consecutive fp32 values -> P planes of 8 bf16 (element i of a plane in bits [16*(i&1), +16) of dword i >> 1)
template <int P>
__device__ __forceinline__ void split8(const float (&v)[8], u32x4 (&pl)[P]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f32x2 x = {v[2 * j], v[2 * j + 1]};
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const bf16x2 h = __builtin_convertvector(x, bf16x2);      // v_cvt_pk_bf16_f32 (RNE)
            const unsigned u = __builtin_bit_cast(unsigned, h);
            pl[p][j] = u;
            if (p + 1 < P) {
                // exact: the low significand bits.  Two scalar v_sub_f32 ON PURPOSE: the packed form (v_pk_add_f32) issues at
                // ~1/15 of the scalar rate while the SIMD's matrix pipe is busy (tools/probes/valu_rates.hip, measured on MI355X:
                // 9 vs 100-180 cycles per instruction next to a v_mfma_f32_32x32x16_bf16 stream)
                x[0] = scalar_sub(x[0], __builtin_bit_cast(float, u << 16));
                x[1] = scalar_sub(x[1], __builtin_bit_cast(float, u & 0xffff0000u));
            }
        }
    }
}

// byte offset of (row, chunk) inside one plane of an operand tile
__device__ __forceinline__ int split_off(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4); }

// PRODUCTS = 8 / 6 -> 3 planes, 3 -> 2 planes.  Order of the partial products (smallest first):
//   8: (2,1) (1,2) (2,0) (1,1) (0,2) (1,0) (0,1) (0,0)   6: the last six of those   3: (1,0) (0,1) (0,0)   1: (0,0) = plain bf16 operands
template <int PRODUCTS>
struct SplitTerm {
    static __device__ __forceinline__ constexpr int pa(int q) {
        if (PRODUCTS == 1) return 0;
        if (PRODUCTS == 3) return q == 0 ? 1 : 0;
        const int qq = q + (8 - PRODUCTS);      // index into the 8-term order
        return qq == 0 ? 2 : qq == 1 ? 1 : qq == 2 ? 2 : qq == 3 ? 1 : qq == 4 ? 0 : qq == 5 ? 1 : 0;
    }
    static __device__ __forceinline__ constexpr int pb(int q) {
        if (PRODUCTS == 1) return 0;
        if (PRODUCTS == 3) return q == 1 ? 1 : 0;
        const int qq = q + (8 - PRODUCTS);
        return qq == 0 ? 1 : qq == 1 ? 2 : qq == 2 ? 0 : qq == 3 ? 1 : qq == 4 ? 2 : qq == 5 ? 0 : qq == 6 ? 1 : 0;
    }
};
template <int PRODUCTS>
struct SplitPlanes { static constexpr int value = PRODUCTS == 1 ? 1 : PRODUCTS == 3 ? 2 : 3; };

// ---- staging of a ROWS x 32 fp32 tile by a 256-thread block (gemm_split.hip, gemm_dxdw.hip) ---------------------------------
// chunks of a ROWS x 32 tile handled per thread: f = tid + 256*i -> row f >> 2, chunk f & 3 (= tid & 3 for every i)
template <int ROWS>
struct SplitChunks { static constexpr int value = (ROWS * 4 + 255) / 256; };

// raw loads of this thread's chunks: 8 consecutive k of a row-major [rows, K] fp32 matrix as 2 float4.  BRANCH-FREE:
// out-of-range rows / k are clamped to valid addresses and zeroed by the store pass (a branch around each load made
// hipcc wait vmcnt(0) after every single load -- the loads must issue back to back and stay in flight over the MFMAs).
template <int ROWS>
__device__ __forceinline__ void split_load(const float* __restrict__ Pm, int64_t ld, int64_t row0, int64_t nrows, int k0, int K,
                                           float4 (&regs)[SplitChunks<ROWS>::value][2]) {
    // wave-uniform 64-bit base (SGPRs) + 32-bit per-thread BYTE offsets (saddr + voffset addressing)
    const int tid = threadIdx.x;
    const char* __restrict__ base = reinterpret_cast<const char*>(Pm + row0 * ld);
    const int last = (int)((nrows - row0 < ROWS) ? (nrows - row0) : ROWS) - 1;      // >= 0: the block has at least one row
#pragma unroll
    for (int i = 0; i < SplitChunks<ROWS>::value; ++i) {
        const int f = tid + 256 * i;
        int r = f >> 2;
        r = r < last ? r : last;
        int k = k0 + (f & 3) * 8;
        k = k < K - 8 ? k : K - 8;                                                 // K % 8 == 0, K >= 8
        const float* p = reinterpret_cast<const float*>(base + (unsigned)((r * (int)ld + k) * 4));
        regs[i][0] = *reinterpret_cast<const float4*>(p);
        regs[i][1] = *reinterpret_cast<const float4*>(p + 4);
    }
}

template <int ROWS>
__device__ __forceinline__ void split_row_scales(const RowScale& rs, int64_t row0, int64_t nrows,
                                                 float (&s0)[SplitChunks<ROWS>::value], float (&s1)[SplitChunks<ROWS>::value]) {
#pragma unroll
    for (int i = 0; i < SplitChunks<ROWS>::value; ++i) {
        const int64_t row = row0 + ((threadIdx.x + 256 * i) >> 2);
        s0[i] = 1.f; s1[i] = 1.f;
        if (rs.r0 != nullptr && row < nrows) {
            s0[i] = rs.r0[row];
            s1[i] = rs.r1 != nullptr ? rs.r1[row] : 1.f;
        }
    }
}

// registers -> (BatchNorm + activation of the producer) -> x*mask row scale -> bf16 planes -> LDS
template <int ROWS, int P, bool SCALED, bool BNIN>
__device__ __forceinline__ void split_store(unsigned char* __restrict__ S, const float4 (&regs)[SplitChunks<ROWS>::value][2], int k0, int split,
                                            const float (&s0)[SplitChunks<ROWS>::value], const float (&s1)[SplitChunks<ROWS>::value],
                                            const float4 (&psc)[2], const float4 (&psh)[2], float neg, float hi, int nvalid, int K) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < SplitChunks<ROWS>::value; ++i) {
        const int f = tid + 256 * i;
        if (ROWS * 4 % 256 != 0 && f >= ROWS * 4) continue;
        const int r = f >> 2, c = f & 3;
        float v[8] = {regs[i][0].x, regs[i][0].y, regs[i][0].z, regs[i][0].w, regs[i][1].x, regs[i][1].y, regs[i][1].z, regs[i][1].w};
        const bool valid = r < nvalid && k0 + c * 8 < K;      // clamped loads (split_load): rows / k outside the matrix are zeros
        if constexpr (BNIN) {
            const float sc[8] = {psc[0].x, psc[0].y, psc[0].z, psc[0].w, psc[1].x, psc[1].y, psc[1].z, psc[1].w};
            const float sh[8] = {psh[0].x, psh[0].y, psh[0].z, psh[0].w, psh[1].x, psh[1].y, psh[1].z, psh[1].w};
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = bn_act_load(v[e], sc[e], sh[e], neg, hi);
        }
        if constexpr (SCALED) {
            const int k = k0 + c * 8;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] *= (k + e < split) ? s0[i] : s1[i];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = valid ? v[e] : 0.f;
        u32x4 pl[P];
        split8<P>(v, pl);
        const int off = split_off(r, c);
#pragma unroll
        for (int p = 0; p < P; ++p) *reinterpret_cast<u32x4*>(S + p * (ROWS * 64) + off) = pl[p];
    }
}

// ---- weights pre-split (B operand of the NT kernel) --------------------------------------------------------
// One tiny kernel per call splits the [N,K] weight matrix (or its transpose, for dX) into P bf16 planes
// planes[p][row][col] in a caller workspace; the GEMM blocks then stage B as plain 16-byte copies -- no VALU work for B,
// which every one of the M/128 row blocks would otherwise repeat (half of the staging VALU of a 128x128 tile).
template <int P>
__global__ void split_w_kernel(const float* __restrict__ w, int rows_in, int cols_in, int transpose, unsigned short* __restrict__ planes) {
    const int64_t total = (int64_t)rows_in * cols_in;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        // i indexes the OUTPUT [rows_out, cols_out]; transpose: out[r][c] = w[c][r]
        const int cols_out = transpose ? rows_in : cols_in;
        const int r = (int)(i / cols_out), c = (int)(i % cols_out);
        float x = transpose ? w[(int64_t)c * cols_in + r] : w[i];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const __bf16 h = (__bf16)x;                               // RNE
            const unsigned short u = __builtin_bit_cast(unsigned short, h);
            planes[(int64_t)p * total + i] = u;
            x -= __builtin_bit_cast(float, (unsigned)u << 16);
        }
    }
}

}  // namespace tsii
