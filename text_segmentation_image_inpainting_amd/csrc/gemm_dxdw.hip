// K3x: dX and dW of a thin 1x1 layer from ONE pass over the wide gradient (split-bf16 arithmetic, 6 products, gemm_split.hip).
//
//   dx[m,k] = rs(m,k) * sum_n dy[m,n]*inv[m] * w[n,k]          dw[n,k] = sum_m dy[m,n]*inv[m] * x[m,k]*rs(m,k)
// with n = the WIDE side (cout) and k = the THIN side (cin <= 128).  Both products have g = dy * inv as an operand; the two
// stand-alone kernels (tsii_pw_bwd_dx, tsii_pw_bwd_dw) each stream the [m, n] gradient from HBM, and on the first two resolution
// levels that read is what they take their time for.  Here a block walks a contiguous range of 64-row tiles (split-M, one full wave
// of blocks); per tile it stages x*rs once, marches over dy in stages of 64 columns, and every stage feeds both products:
//   staging   g (64 rows x 64 columns), the matching [k][64 n] piece of the pre-split W^T planes (split_w_kernel layout) and, once
//             per tile, x*rs: all ROW-MAJOR as sub-tiles [plane][64 rows][32 bf16] with the swizzle of split_bf16.h (split_off)
//   dX        A = g rows (ds_read_b128 fragments as in gemm_nt_split_kernel), B = the W^T piece; accumulators [64 x thin] per tile
//   dW        contracts over the tile's rows: BOTH operands (g columns, x columns) come out of the row-major images through the
//             transposing LDS read (bf16_common.h: lds_read8_tr), four consecutive rows of one column per instruction.  The
//             [wide x thin] accumulators of the block stay in registers over all its row tiles (stage loop unrolled: NST stages).
//   end       one partial [wide x thin] slab per block -> launch_reduce_rows; the bias gradient takes the column-sum route
// Waves (4): dX tile rows 32 (w >> 1), thin tiles TT2 (w & 1) ..;  dW columns 32 (w >> 1) of the stage, the same thin tiles.
// Registers (TT2 = 1, NST = 6: thin <= 64, wide <= 384): 96 dW + 16 dX accumulators, 16 (32 with x) in flight across the MFMA phase.
//
// K3xb (BN = true; TT2 = 1, NST = 4: thin <= 64, wide <= 256): the gradient operand is da, the gradient w.r.t. the OUTPUT of the
// BatchNorm(+activation) that follows the layer, next to that BatchNorm's raw input y (= this layer's output).  Both stream in side
// by side (16 more registers in flight, paid for by the 32 accumulators two stages fewer free) and the staging step forms
// g = bn_bwd_elem(da, y, coef) * inv in the registers it splits anyway -- the stand-alone apply pass (bn.hip: bn_bwd_apply_kernel,
// the same helper, the same bits) and its dy tensor are gone.  The constants' table coef[6][wide] sits in LDS, filled once per block.
#include "bf16_common.h"
#include "gemm_tiles.h"
#include "split_bf16.h"

namespace tsii {

static constexpr int XW_ROWS = 64;                      // rows of a tile = the m extent of one dW contraction step
static constexpr int XW_SUB = 3 * XW_ROWS * 64;         // bytes of a 64-row sub-tile: 3 planes x 64 rows x 32 bf16

#if defined(TSII_HIP_EMU)
template <class... T> static inline void xw_lds_wait(T&...) {}
#else
// the transposing reads are inline assembly: the consumers must not move above the wait (the operands are tied to it)
__device__ __forceinline__ void xw_lds_wait(hu32x2& a, hu32x2& b, hu32x2& c, hu32x2& d, hu32x2& e, hu32x2& f) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f) : : "memory");
}
#endif

// g, x: one chunk (row tid >> 2, 8 columns from 8 (tid & 3)) of a 64 x 32 fp32 sub-tile per thread, loaded and split into the
// [plane][64 rows][32 bf16] image by the staging helpers of the NT kernel (split_bf16.h: split_load / split_store with ROWS = 64)
__device__ __forceinline__ void xw_load(const float* __restrict__ base, int ld, int col0, int ncols, float4 (&regs)[1][2]) {
    split_load<XW_ROWS>(base, ld, 0, XW_ROWS, col0, ncols, regs);
}
__device__ __forceinline__ void xw_store(unsigned char* __restrict__ S, const float4 (&regs)[1][2], int col0, int ncols, int split, float f0, float f1) {
    const float s0[1] = {f0}, s1[1] = {f1};
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 none[2] = {z, z};
    split_store<XW_ROWS, 3, true, false>(S, regs, col0, split, s0, s1, none, none, 1.f, 0.f, XW_ROWS, ncols);
}

// K3xb operands: nothing in the plain forms (their code is what it was), the BatchNorm's side of the hand-over in the BN form
template <bool BN>
struct XwBn {};
template <>
struct XwBn<true> {
    const float* y;      // [m, wide] raw BatchNorm input
    const float* coef;   // [6][wide]: mean, 1/std, gamma, beta, sum dz / m, sum dz*xhat / m (tsii_bn_bwd_reduce)
    float neg, hi;       // the activation in its load-time form (make_in_bn)
};

// g = BatchNorm-backward(da, y) of this thread's 8 columns (from `col` of the LDS table, CW columns per constant), in place
template <int CW>
__device__ __forceinline__ void xw_bn_apply(float4 (&da)[1][2], const float4 (&y)[1][2], const float* __restrict__ Cs, int col, float neg, float hi) {
    // inbn_grad's values (bf16_common.h) as two selects: its `&&` became a branch per element here
    auto grad = [&](float z) { const float in = z < hi ? 1.f : 0.f; return z > 0.f ? in : neg; };
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const float* c = Cs + col + 4 * q;
        const float4 mu = *reinterpret_cast<const float4*>(c), is = *reinterpret_cast<const float4*>(c + CW);
        const float4 ga = *reinterpret_cast<const float4*>(c + 2 * CW), be = *reinterpret_cast<const float4*>(c + 3 * CW);
        const float4 k1 = *reinterpret_cast<const float4*>(c + 4 * CW), k2 = *reinterpret_cast<const float4*>(c + 5 * CW);
        float4& d = da[0][q];
        const float4& v = y[0][q];
        d.x = bn_bwd_elem(d.x, v.x, mu.x, is.x, ga.x, be.x, k1.x, k2.x, grad);
        d.y = bn_bwd_elem(d.y, v.y, mu.y, is.y, ga.y, be.y, k1.y, k2.y, grad);
        d.z = bn_bwd_elem(d.z, v.z, mu.z, is.z, ga.z, be.z, k1.z, k2.z, grad);
        d.w = bn_bwd_elem(d.w, v.w, mu.w, is.w, ga.w, be.w, k1.w, k2.w, grad);
    }
}

template <int TT2, int NST, bool BN = false>
__global__ __launch_bounds__(256, TT2 == 1 ? 2 : 1) void pw_dxdw_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                        const unsigned short* __restrict__ wt, const float* __restrict__ inv,
                                                                        RowScale rs, float* __restrict__ dx, float* __restrict__ part,
                                                                        int ntiles, int tiles_per_block, int wide, int thin, XwBn<BN> bn) {
    constexpr int CW = 64 * NST;                         // columns of the constants' table (BN)
    constexpr int KP = 64 * TT2;                         // thin side as staged (2 TT2 tiles of 32)
    constexpr int WSUB = 3 * KP * 64;                    // bytes of a W^T sub-tile: 3 planes x KP rows x 32 bf16
    constexpr int WCH = KP / 64;                         // W^T chunks per thread, plane and sub-tile
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * XW_SUB + 2 * TT2 * XW_SUB + 2 * WSUB + 2 * XW_ROWS * 4 + (BN ? 6 * CW * 4 : 0)];
    unsigned char* Gs = smem;                            // [2 column halves] sub-tiles of g
    unsigned char* Xs = Gs + 2 * XW_SUB;                 // [2 TT2 thin tiles] sub-tiles of x * rs
    unsigned char* Ws = Xs + 2 * TT2 * XW_SUB;           // [2 column halves][plane][KP rows k][32 n]
    float* Rs = reinterpret_cast<float*>(Ws + 2 * WSUB); // r0 | r1 of the tile's rows (dX epilogue)
    float* Cs = Rs + 2 * XW_ROWS;                        // BN: coef[6][CW], zeros past `wide` (read behind the first stage's barrier)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, hi = lane >> 5;
    const int wr = wave >> 1, wu = wave & 1;
    const int nst = (wide + 63) >> 6;
    const int tile_beg = (int)blockIdx.x * tiles_per_block;
    const int tile_end = tile_beg + tiles_per_block < ntiles ? tile_beg + tiles_per_block : ntiles;
    const int64_t wplane = (int64_t)wide * thin;

    if constexpr (BN) {
        for (int i = threadIdx.x; i < 6 * CW; i += 256) {
            const int j = i / CW, c = i - j * CW;
            Cs[i] = c < wide ? bn.coef[j * wide + c] : 0.f;
        }
    }

    f32x16 adw[NST][TT2];
#pragma unroll
    for (int s = 0; s < NST; ++s)
#pragma unroll
        for (int t = 0; t < TT2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) adw[s][t][r] = 0.f;

    // ---- what is in flight for the next stage: g (two sub-tiles), the W^T piece; at a tile's first stage x, inv and the mask rows
    float4 rg[2][1][2], rx[2 * TT2][1][2], ry[2][1][2];
    u32x4 rw[2][WCH][3];
    float finv = 1.f, fx0 = 1.f, fx1 = 1.f;
    auto prefetch = [&](int tile, int s, bool first, int wide, int thin) {
        const int64_t row0 = (int64_t)tile * XW_ROWS;
        const float* gb = dy + row0 * wide;
#pragma unroll
        for (int h = 0; h < 2; ++h) xw_load(gb, wide, 64 * s + 32 * h, wide, rg[h]);
        if constexpr (BN) {
            const float* yb = bn.y + row0 * wide;
#pragma unroll
            for (int h = 0; h < 2; ++h) xw_load(yb, wide, 64 * s + 32 * h, wide, ry[h]);
        }

        if (first) {
            const float* xb = x + row0 * thin;
#pragma unroll
            for (int u = 0; u < 2 * TT2; ++u) xw_load(xb, thin, 32 * u, thin, rx[u]);
            const int64_t row = row0 + (tid >> 2);
            finv = inv != nullptr ? inv[row] : 1.f;
            fx0 = 1.f; fx1 = 1.f;
            if (rs.r0 != nullptr) {
                fx0 = rs.r0[row];
                fx1 = rs.r1 != nullptr ? rs.r1[row] : 1.f;
            }
        }
    };
    // the W^T piece comes from L2 (every block re-reads the same planes): fetched BEHIND the MFMA phase, so its 24 registers are
    // not held across it (they made the kernel spill); the barrier wait and the split of g cover most of the latency
    auto fetch_w = [&](int s, int wide, int thin) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < WCH; ++i) {
                const int f = tid + 256 * i;
                int k = f >> 2, n = 64 * s + 32 * h + (f & 3) * 8;
                k = k < thin - 1 ? k : thin - 1;
                n = n < wide - 8 ? n : wide - 8;
                const unsigned off = (unsigned)((k * wide + n) * 2);
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    rw[h][i][p] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(wt + p * wplane) + off);
            }
    };

    // ---- fragment addresses.  ds_read_b128 (dX): row li of the wave's tile, chunk 2 kk + hi of the 32-column sub-tile
    const int swz = (li >> 2) & 3;
    const int fo[2] = {li * 64 + (((0 + hi) ^ swz) << 4), li * 64 + (((2 + hi) ^ swz) << 4)};
    // transposing read (dW): lane (q = lane & 15, g1 = (lane >> 4) & 1, hi) points at row 16 ks + 8 hi + (q >> 2) + 4 j, columns
    // 16 g1 + 4 (q & 3) ..; (row >> 2) & 3 = (2 hi + j) & 3 there, so a K step is a constant offset of 16 rows
    const int q = lane & 15, g1 = (lane >> 4) & 1;
    int tro[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = 8 * hi + (q >> 2) + 4 * j, chunk = 2 * g1 + ((q & 3) >> 1);
        tro[j] = row * 64 + ((chunk ^ ((2 * hi + j) & 3)) << 4) + (q & 1) * 8;
    }

    if (tile_beg < tile_end) { prefetch(tile_beg, 0, true, wide, thin); fetch_w(0, wide, thin); }
    const int wide_arg = wide, thin_arg = thin;
    for (int tile = tile_beg; tile < tile_end; ++tile) {
        // the stage loop below is unrolled: left alone, the compiler hoists every stage's clamped offsets out of this loop and holds
        // them in registers for the whole kernel (it spilled over a hundred); opaque copies keep them inside
        unsigned wide_o = (unsigned)wide_arg, thin_o = (unsigned)thin_arg;
        TSII_OPAQUE_U32(wide_o); TSII_OPAQUE_U32(thin_o);
        const int wide = (int)wide_o, thin = (int)thin_o;
        f32x16 adx[TT2];
#pragma unroll
        for (int t = 0; t < TT2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) adx[t][r] = 0.f;

#pragma unroll
        for (int s = 0; s < NST; ++s) {
            if (s < nst) {
                __syncthreads();                         // the fragment reads of the previous stage (and its epilogue's Rs) are done
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    // (columns past `wide` meet zero constants and are zeroed by the store; the table has a slot for every staged column)
                    if constexpr (BN) xw_bn_apply<CW>(rg[h], ry[h], Cs, 64 * s + 32 * h + 8 * (tid & 3), bn.neg, bn.hi);
                    xw_store(Gs + h * XW_SUB, rg[h], 64 * s + 32 * h, wide, 0x7fffffff, finv, finv);
#pragma unroll
                    for (int i = 0; i < WCH; ++i) {
                        const int f = tid + 256 * i;
                        const int k = f >> 2, c = f & 3;
                        const bool valid = k < thin && 64 * s + 32 * h + c * 8 < wide;
                        const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
                        for (int p = 0; p < 3; ++p)
                            *reinterpret_cast<u32x4*>(Ws + h * WSUB + p * (KP * 64) + split_off(k, c)) = valid ? rw[h][i][p] : z;
                    }
                }
                if (s == 0) {
#pragma unroll
                    for (int u = 0; u < 2 * TT2; ++u) xw_store(Xs + u * XW_SUB, rx[u], 32 * u, thin, rs.split, fx0, fx1);
                    if ((tid & 3) == 0) { Rs[tid >> 2] = fx0; Rs[XW_ROWS + (tid >> 2)] = fx1; }
                }
                __syncthreads();
                {   // the next stage's loads fly during the MFMA phase (after the block's last stage: a harmless reload)
                    const bool last = s + 1 >= nst;
                    const int nt = last ? (tile + 1 < tile_end ? tile + 1 : tile) : tile;
                    prefetch(nt, last ? 0 : s + 1, last, wide, thin);
                }
                __builtin_amdgcn_s_setprio(2);
                // ---- dX: [32 rows] x [TT2 thin tiles] of this wave, K = the stage's 64 columns
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const int h = ks >> 1, kk = ks & 1;
                    bf16x8 a[3];
#pragma unroll
                    for (int p = 0; p < 3; ++p)
                        a[p] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(Gs + h * XW_SUB + p * (XW_ROWS * 64) + wr * (32 * 64) + fo[kk]));
#pragma unroll
                    for (int t = 0; t < TT2; ++t) {
                        bf16x8 b[3];
#pragma unroll
                        for (int p = 0; p < 3; ++p)
                            b[p] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(Ws + h * WSUB + p * (KP * 64) + (TT2 * wu + t) * (32 * 64) + fo[kk]));
#pragma unroll
                        for (int pq = 0; pq < 6; ++pq)
                            adx[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[SplitTerm<6>::pa(pq)], b[SplitTerm<6>::pb(pq)], adx[t], 0, 0, 0);
                    }
                }
                // ---- dW: [32 columns of g] x [TT2 thin tiles], K = the tile's 64 rows
                const unsigned char* Ga = Gs + wr * XW_SUB;
#define TSII_XW_TR(KS)                                                                                                              \
                {                                                                                                                   \
                    hu32x2 al[3], ah[3];                                                                                            \
                    _Pragma("unroll") for (int p = 0; p < 3; ++p) {                                                                 \
                        lds_read8_tr<(KS) * 1024>(al[p], Ga + p * (XW_ROWS * 64) + tro[0]);                                         \
                        lds_read8_tr<(KS) * 1024>(ah[p], Ga + p * (XW_ROWS * 64) + tro[1]);                                         \
                    }                                                                                                               \
                    xw_lds_wait(al[0], ah[0], al[1], ah[1], al[2], ah[2]);                                                          \
                    bf16x8 a[3];                                                                                                    \
                    _Pragma("unroll") for (int p = 0; p < 3; ++p) {                                                                 \
                        const u32x4 av = {al[p][0], al[p][1], ah[p][0], ah[p][1]};                                                  \
                        a[p] = __builtin_bit_cast(bf16x8, av);                                                                      \
                    }                                                                                                               \
                    _Pragma("unroll") for (int t = 0; t < TT2; ++t) {                                                               \
                        const unsigned char* Xb = Xs + (TT2 * wu + t) * XW_SUB;                                                     \
                        hu32x2 bl[3], bh[3];                                                                                        \
                        _Pragma("unroll") for (int p = 0; p < 3; ++p) {                                                             \
                            lds_read8_tr<(KS) * 1024>(bl[p], Xb + p * (XW_ROWS * 64) + tro[0]);                                     \
                            lds_read8_tr<(KS) * 1024>(bh[p], Xb + p * (XW_ROWS * 64) + tro[1]);                                     \
                        }                                                                                                           \
                        xw_lds_wait(bl[0], bh[0], bl[1], bh[1], bl[2], bh[2]);                                                      \
                        bf16x8 b[3];                                                                                                \
                        _Pragma("unroll") for (int p = 0; p < 3; ++p) {                                                             \
                            const u32x4 bv = {bl[p][0], bl[p][1], bh[p][0], bh[p][1]};                                              \
                            b[p] = __builtin_bit_cast(bf16x8, bv);                                                                  \
                        }                                                                                                           \
                        _Pragma("unroll") for (int pq = 0; pq < 6; ++pq)                                                            \
                            adw[s][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[SplitTerm<6>::pa(pq)], b[SplitTerm<6>::pb(pq)], adw[s][t], 0, 0, 0); \
                    }                                                                                                               \
                }
                TSII_XW_TR(0) TSII_XW_TR(1) TSII_XW_TR(2) TSII_XW_TR(3)
#undef TSII_XW_TR
                __builtin_amdgcn_s_setprio(0);
                fetch_w(s + 1 < nst ? s + 1 : 0, wide, thin);
            }
        }

        // ---- dX epilogue: rs(m, k) on the way out; a lane holds column k = 32 u + li of 16 rows (128-byte runs per row)
        float* dxt = dx + (int64_t)tile * XW_ROWS * thin;
#pragma unroll
        for (int t = 0; t < TT2; ++t) {
            const int k = (TT2 * wu + t) * 32 + li;
            if (k < thin) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    const float f = rs.r0 == nullptr ? 1.f : (k < rs.split ? Rs[row] : Rs[XW_ROWS + row]);
                    dxt[row * thin + k] = adx[t][r] * f;
                }
            }
        }
    }

    // ---- the block's partial dw[n][k]: n = 64 s + 32 (w >> 1) + accumulator row, k = 32 u + li
    float* pz = part + (int64_t)blockIdx.x * wplane;
    int li_e = li, hi_e = hi, wr_e = wr, wu_e = wu;
    if constexpr (BN) {      // re-derived behind the loop: carried across it these indices were the form's only two spilled registers
        unsigned t = threadIdx.x;
        TSII_OPAQUE_U32(t);
        li_e = (int)(t & 31u); hi_e = (int)((t >> 5) & 1u); wr_e = (int)(t >> 7); wu_e = (int)((t >> 6) & 1u);
    }
#pragma unroll
    for (int s = 0; s < NST; ++s)
#pragma unroll
        for (int t = 0; t < TT2; ++t) {
            const int k = (TT2 * wu_e + t) * 32 + li_e;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = 64 * s + 32 * wr_e + (r & 3) + 8 * (r >> 2) + 4 * hi_e;
                if (n < wide && k < thin) pz[n * thin + k] = adw[s][t][r];
            }
        }
}

// eligible shapes by registers: thin <= 64 with up to 6 stages of 64 columns, thin <= 128 with up to 3 (96 dW accumulators either way)
static bool xw_shape_ok(int64_t m, int wide, int thin) {
    if (m <= 0 || m % XW_ROWS != 0 || m / XW_ROWS >= (1ll << 31) || wide < 32 || wide % 32 != 0 || thin < 32 || thin % 32 != 0) return false;
    if (thin <= 64) return wide <= 384;
    return thin <= 128 && wide <= 192;
}
// K3xb: the one-thin-tile form with four column stages
static bool xw_bn_shape_ok(int64_t m, int wide, int thin) { return xw_shape_ok(m, wide, thin) && thin <= 64 && wide <= 256; }

// split-M plan: one full wave of blocks (2 per CU at thin <= 64, else 1), contiguous tile ranges
static void xw_plan(int64_t m, int thin, int* nblocks, int* tiles_per_block) {
    const int64_t ntiles = m / XW_ROWS;
    int64_t want = (int64_t)device_cus() * (thin <= 64 ? 2 : 1);
    if (want > ntiles) want = ntiles;
    const int64_t tpb = cdiv64(ntiles, want);
    *tiles_per_block = (int)tpb;
    *nblocks = (int)cdiv64(ntiles, tpb);
}

}  // namespace tsii

using namespace tsii;

// Below this many rows the two stand-alone kernels stay: the 64^2 and 32^2 levels are matrix-bound, one read of dy buys nothing there
static constexpr int64_t TSII_DXDW_MIN_M = 524288;

extern "C" int tsii_pw_bwd_dxdw_ok(int64_t m, int n, int k, int64_t min_m) {
    if (gemm_products() != 6) return 0;                  // the 6-product split-bf16 arithmetic only
    if (!xw_shape_ok(m, n, k)) return 0;
    if (min_m >= 0) return m >= min_m ? 1 : 0;          // tests: every shape the kernel can run
    // the library's own choice: only the class that was timed against the two calls -- thin side 64,
    // wide side 256 .. 384.  Thin 32 pads half of every staged tile, thin 96 / 128 runs one block per CU: not measured, not taken
    return (k == 64 && n >= 256 && m >= TSII_DXDW_MIN_M) ? 1 : 0;
}

// tiles (64 rows) a block of the kernel walks for this shape on this device; 0: not eligible
extern "C" int tsii_pw_bwd_dxdw_tiles_per_block(int64_t m, int n, int k) {
    if (!xw_shape_ok(m, n, k)) return 0;
    int nb = 0, tpb = 0;
    xw_plan(m, k, &nb, &tpb);
    return tpb;
}

extern "C" size_t tsii_pw_bwd_dxdw_ws_bytes(int64_t m, int n, int k) {
    if (!xw_shape_ok(m, n, k)) return 0;
    int nb = 0, tpb = 0;
    xw_plan(m, k, &nb, &tpb);
    return ((size_t)nb * n * k + colsum_ws_floats(m, n)) * sizeof(float) + (size_t)3 * n * k * sizeof(unsigned short) + 16;
}

extern "C" int tsii_pw_bwd_dxdw(const float* dy, const float* x, int64_t m, int n, const float* w, int k, const float* inv,
                                const float* keep, const float* r0, int split, const float* r1, float* dx, float* dw, float* dbias,
                                void* ws, size_t ws_bytes, void* stream) {
    TSII_REQUIRE(dy && x && w && dx && dw && ws, "pw_bwd_dxdw: null pointer");
    TSII_REQUIRE(gemm_products() == 6, "pw_bwd_dxdw: the 6-product split-bf16 arithmetic only (tsii_set_gemm_products)");
    TSII_REQUIRE(xw_shape_ok(m, n, k), "pw_bwd_dxdw: shape m=%lld n=%d k=%d is not eligible (tsii_pw_bwd_dxdw_ok)", (long long)m, n, k);
    TSII_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(ws), "pw_bwd_dxdw: 16-byte aligned operands are required");
    TSII_REQUIRE(ws_bytes >= tsii_pw_bwd_dxdw_ws_bytes(m, n, k), "pw_bwd_dxdw: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    int nb = 0, tpb = 0;
    xw_plan(m, k, &nb, &tpb);
    float* part = (float*)ws;
    float* cpart = part + (size_t)nb * n * k;
    unsigned short* planes = reinterpret_cast<unsigned short*>((reinterpret_cast<uintptr_t>(cpart + colsum_ws_floats(m, n)) + 15) & ~(uintptr_t)15);
    // W [n,k] -> bf16 planes of W^T [k][n] (the B operand of dX, as launch_nt_split lays it out)
    hipLaunchKernelGGL(split_w_kernel<3>, dim3(stream_grid((int64_t)n * k, 256)), dim3(256), 0, st, w, n, k, 1, planes);
    int rc = check_launch("split_w");
    if (rc) return rc;
    const RowScale rs = {r0, r1, r0 != nullptr ? split : 0};
    const int ntiles = (int)(m / XW_ROWS);
    if (k <= 64) hipLaunchKernelGGL((pw_dxdw_kernel<1, 6>), dim3(nb), dim3(256), 0, st, dy, x, planes, inv, rs, dx, part, ntiles, tpb, n, k, XwBn<false>{});
    else hipLaunchKernelGGL((pw_dxdw_kernel<2, 3>), dim3(nb), dim3(256), 0, st, dy, x, planes, inv, rs, dx, part, ntiles, tpb, n, k, XwBn<false>{});
    rc = check_launch("pw_dxdw");
    if (rc) return rc;
    rc = launch_reduce_rows(part, nb, (int64_t)n * k, dw, st);
    if (rc) return rc;
    if (dbias != nullptr) rc = launch_colsum_scaled(dy, keep, m, n, dbias, cpart, st);
    return rc;
}

// ---- K3xb: the same with the backward APPLY pass of the BatchNorm(+activation) that follows the layer folded into the staging step
extern "C" int tsii_pw_bwd_dxdw_bn_ok(int64_t m, int n, int k, int64_t min_m) {
    if (gemm_products() != 6) return 0;
    if (!xw_bn_shape_ok(m, n, k)) return 0;
    if (min_m >= 0) return m >= min_m ? 1 : 0;
    // the library's own choice: the class that was timed against apply pass + K3x
    return (k == 64 && n == 256 && m >= TSII_DXDW_MIN_M) ? 1 : 0;
}

extern "C" int tsii_pw_bwd_dxdw_bn_tiles_per_block(int64_t m, int n, int k) {
    if (!xw_bn_shape_ok(m, n, k)) return 0;
    int nb = 0, tpb = 0;
    xw_plan(m, k, &nb, &tpb);
    return tpb;
}

extern "C" size_t tsii_pw_bwd_dxdw_bn_ws_bytes(int64_t m, int n, int k) {
    if (!xw_bn_shape_ok(m, n, k)) return 0;
    int nb = 0, tpb = 0;
    xw_plan(m, k, &nb, &tpb);
    return (size_t)nb * n * k * sizeof(float) + (size_t)3 * n * k * sizeof(unsigned short) + 16;
}

extern "C" int tsii_pw_bwd_dxdw_bn(const float* da, const float* y, const float* coef, int act, float slope, const float* x, int64_t m,
                                   int n, const float* w, int k, const float* inv, const float* keep, const float* r0, int split,
                                   const float* r1, float* dx, float* dw, float* dbias, void* ws, size_t ws_bytes, void* stream) {
    TSII_REQUIRE(da && y && coef && x && w && dx && dw && ws, "pw_bwd_dxdw_bn: null pointer");
    // dy is never written, so there is nothing to take a bias gradient from in a pass of its own; the layers this serves (a 1x1
    // layer in front of a BatchNorm) have no bias.  keep only enters the bias gradient.
    (void)keep;
    TSII_REQUIRE(dbias == nullptr, "pw_bwd_dxdw_bn: layers with a bias keep tsii_bn_bwd_apply + tsii_pw_bwd_dxdw");
    TSII_REQUIRE(gemm_products() == 6, "pw_bwd_dxdw_bn: the 6-product split-bf16 arithmetic only (tsii_set_gemm_products)");
    TSII_REQUIRE(xw_bn_shape_ok(m, n, k), "pw_bwd_dxdw_bn: shape m=%lld n=%d k=%d is not eligible (tsii_pw_bwd_dxdw_bn_ok)", (long long)m, n, k);
    InBN ib;
    TSII_REQUIRE(make_in_bn(nullptr, nullptr, act, slope, &ib) == 0, "pw_bwd_dxdw_bn: activation %d (slope %g) has no load-time form", act, (double)slope);
    TSII_REQUIRE(aligned16(da) && aligned16(y) && aligned16(x) && aligned16(ws), "pw_bwd_dxdw_bn: 16-byte aligned operands are required");
    TSII_REQUIRE(ws_bytes >= tsii_pw_bwd_dxdw_bn_ws_bytes(m, n, k), "pw_bwd_dxdw_bn: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    int nb = 0, tpb = 0;
    xw_plan(m, k, &nb, &tpb);
    float* part = (float*)ws;
    unsigned short* planes = reinterpret_cast<unsigned short*>((reinterpret_cast<uintptr_t>(part + (size_t)nb * n * k) + 15) & ~(uintptr_t)15);
    hipLaunchKernelGGL(split_w_kernel<3>, dim3(stream_grid((int64_t)n * k, 256)), dim3(256), 0, st, w, n, k, 1, planes);
    int rc = check_launch("split_w");
    if (rc) return rc;
    const RowScale rs = {r0, r1, r0 != nullptr ? split : 0};
    XwBn<true> bn;
    bn.y = y; bn.coef = coef; bn.neg = ib.neg; bn.hi = ib.hi;
    hipLaunchKernelGGL((pw_dxdw_kernel<1, 4, true>), dim3(nb), dim3(256), 0, st, da, x, planes, inv, rs, dx, part, (int)(m / XW_ROWS), tpb, n, k, bn);
    rc = check_launch("pw_dxdw_bn");
    if (rc) return rc;
    return launch_reduce_rows(part, nb, (int64_t)n * k, dw, st);
}
