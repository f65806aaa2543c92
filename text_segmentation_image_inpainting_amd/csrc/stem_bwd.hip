// K4s: backward of the 7x7 / stride-2 stem (a 4x4 valid convolution over the space-to-depth image x2 [n, h2, w2, 12], 64 output
// channels) in ONE pass: weight gradient, bias gradient and, optionally, the gradient of the LeakyReLU behind the stem.
//
//   dy[r, co]           = gy[r, co] * (y[r, co] > 0 ? 1 : slope)                      (y given; else dy = gy)
//   dwk[co][c][ay][ax]  = sum_r dy[r, co] * inv[r] * x2[n, oy + ay, ox + ax, c]       r = (n, oy, ox), m = n ho wo rows
//   db[co]              = sum_r dy[r, co] * keep[r]
// 6-product split-bf16 arithmetic (gemm_split.hip), the dW half of gemm_dxdw.hip with the roles renamed: the thin operand is
// dy * inv (64 columns), the wide one the 192 gathered columns of x2, both contracted over a tile's 64 rows through the transposing
// LDS read, the [192 x 64] accumulators held in registers over all of a block's tiles (split-M, two blocks per CU).
//
// Loader.  A tile is 64 consecutive output pixels of one output row (wo % 64 == 0).  Its receptive field is 4 image rows of
// 67 pixels x 12 channels = 804 contiguous floats each.  That window is fetched once with 16-byte loads, split into three bf16
// planes (split8 of split_bf16.h) and kept as it lies in memory: win[plane][ay][808 bf16].  With k' = 48 ay + 12 ax + c the operand
// element (row r, column k') is win[ay][12 r + (k' - 48 ay)]: a row-major matrix with a row stride of 12 elements (24 bytes).  The
// transposing read takes four consecutive rows of one column from any 8-byte aligned row-major image, so it reads the [64 x 192]
// operand straight out of the window -- the im2col matrix is never built, every x2 element is split once, and no address is decoded
// per (tap, channel).  A 32-column MFMA tile is two 16-lane groups with an address each: 16-column blocks b = k' / 16, ay = b / 3.
// dy * inv goes through split_load / split_store into the swizzled [plane][64 rows][32 bf16] sub-tiles of gemm_dxdw.hip.
//
// Waves (4): wr = wave >> 1 picks the 32 columns 64 s + 32 wr of k' (s = 0 .. 2), wu = wave & 1 the 32 output channels.
// A block leaves one slab [192 k'][64 co] | [64 db]; launch_reduce_rows adds the slabs, a small kernel permutes k' -> (c, ay, ax).
// LDS: 2 x 12288 (dy) + 3 x 6464 (window) = 43968 bytes.  Registers: 48 dW accumulators + 16 bias sums + <= 50 in flight.
#include "bf16_common.h"
#include "gemm_tiles.h"
#include "split_bf16.h"

namespace tsii {

static constexpr int SB_ROWS = 64;                            // rows of a tile = output pixels = the contraction extent of one step
static constexpr int SB_SUB = 3 * SB_ROWS * 64;               // bytes of a dy sub-tile: 3 planes x 64 rows x 32 bf16
static constexpr int SB_C4 = 12, SB_KA = 4, SB_COUT = 64;
static constexpr int SB_K = SB_C4 * SB_KA * SB_KA;            // 192
static constexpr int SB_WIN_FLOATS = (SB_ROWS + SB_KA - 1) * SB_C4;   // 804 floats of one window row
static constexpr int SB_WIN_CHUNKS = (SB_WIN_FLOATS + 7) / 8;         // 101 chunks of 8 (the last one half used)
static constexpr int SB_WIN_ROW = SB_WIN_CHUNKS * 16;                 // 1616 bytes of one window row in one plane
static constexpr int SB_WIN_PLANE = SB_KA * SB_WIN_ROW;               // 6464
static constexpr int SB_ROW_STEP = SB_C4 * 2;                         // 24 bytes: one output pixel further in the window
static constexpr int SB_SLAB = SB_K * SB_COUT + SB_COUT;              // floats a block leaves: dW partial | db partial

#if defined(TSII_HIP_EMU)
template <class... T> static inline void sb_lds_wait(T&...) {}
#else
// the transposing reads are inline assembly: the consumers must not move above the wait (the operands are tied to it)
__device__ __forceinline__ void sb_lds_wait(hu32x2& a, hu32x2& b, hu32x2& c, hu32x2& d, hu32x2& e, hu32x2& f) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f) : : "memory");
}
#endif

// one MFMA operand (three planes, 8 k each) from two transposing reads per plane
__device__ __forceinline__ void sb_operand(hu32x2 (&lo)[3], hu32x2 (&hi)[3], bf16x8 (&o)[3]) {
    sb_lds_wait(lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const u32x4 v = {lo[p][0], lo[p][1], hi[p][0], hi[p][1]};
        o[p] = __builtin_bit_cast(bf16x8, v);
    }
}

// contraction step KS (rows 16 KS .. 16 KS + 15 of the tile): the dy fragment once, then the wave's three k' tiles
template <int KS>
__device__ __forceinline__ void sb_step(const unsigned char* __restrict__ Gb, int tro0, int tro1, const unsigned char* (&Wa)[3], f32x16 (&acc)[3]) {
    hu32x2 bl[3], bh[3];
    bf16x8 b[3];
    lds_read8_tr<KS * 1024>(bl[0], Gb + tro0);
    lds_read8_tr<KS * 1024>(bh[0], Gb + tro1);
    lds_read8_tr<KS * 1024 + SB_ROWS * 64>(bl[1], Gb + tro0);
    lds_read8_tr<KS * 1024 + SB_ROWS * 64>(bh[1], Gb + tro1);
    lds_read8_tr<KS * 1024 + 2 * SB_ROWS * 64>(bl[2], Gb + tro0);
    lds_read8_tr<KS * 1024 + 2 * SB_ROWS * 64>(bh[2], Gb + tro1);
    sb_operand(bl, bh, b);
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        constexpr int O = KS * 16 * SB_ROW_STEP;             // 16 rows further; the second read of a pair: 4 rows further
        hu32x2 al[3], ah[3];
        bf16x8 a[3];
        lds_read8_tr<O>(al[0], Wa[s]);
        lds_read8_tr<O + 4 * SB_ROW_STEP>(ah[0], Wa[s]);
        lds_read8_tr<O + SB_WIN_PLANE>(al[1], Wa[s]);
        lds_read8_tr<O + SB_WIN_PLANE + 4 * SB_ROW_STEP>(ah[1], Wa[s]);
        lds_read8_tr<O + 2 * SB_WIN_PLANE>(al[2], Wa[s]);
        lds_read8_tr<O + 2 * SB_WIN_PLANE + 4 * SB_ROW_STEP>(ah[2], Wa[s]);
        sb_operand(al, ah, a);
#pragma unroll
        for (int pq = 0; pq < 6; ++pq)
            acc[s] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[SplitTerm<6>::pa(pq)], b[SplitTerm<6>::pb(pq)], acc[s], 0, 0, 0);
    }
}

__device__ __forceinline__ void sb_unpack(const float4 (&r)[2], float (&v)[8]) {
    v[0] = r[0].x; v[1] = r[0].y; v[2] = r[0].z; v[3] = r[0].w; v[4] = r[1].x; v[5] = r[1].y; v[6] = r[1].z; v[7] = r[1].w;
}

template <bool ACT>
__global__ __launch_bounds__(256, 2) void stem_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ y, float slope,
                                                          const float* __restrict__ inv, const float* __restrict__ keep,
                                                          const float* __restrict__ x2, int ho, int wo, float* __restrict__ part,
                                                          int ntiles, int tiles_per_block) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * SB_SUB + 3 * SB_WIN_PLANE];
    unsigned char* Gs = smem;                            // [2 column halves] sub-tiles of dy * inv
    unsigned char* Wn = smem + 2 * SB_SUB;               // [plane][4 window rows][808 bf16]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, hi = lane >> 5;
    const int wr = wave >> 1, wu = wave & 1;
    const int tile_beg = (int)blockIdx.x * tiles_per_block;
    const int tile_end = tile_beg + tiles_per_block < ntiles ? tile_beg + tiles_per_block : ntiles;
    const int h2 = ho + SB_KA - 1, w2 = wo + SB_KA - 1, tiles_per_row = wo >> 6;

    f32x16 acc[3];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
    float dbacc[2][8];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 8; ++e) dbacc[h][e] = 0.f;

    // ---- the window: chunk f = tid + 256 i of 4 x 101 -> row ay = f / 101, floats 8 ch .. of that row.  Branch-free loads: a chunk
    // past the end repeats the last one (and is not stored); the half chunk at the end of a row repeats its first half (never read)
    unsigned woff[2][2];
    int wlds[2];
    bool wvalid[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int f = tid + 256 * i;
        wvalid[i] = f < SB_KA * SB_WIN_CHUNKS;
        const int fc = wvalid[i] ? f : SB_KA * SB_WIN_CHUNKS - 1;
        const int ay = fc / SB_WIN_CHUNKS, ch = fc - ay * SB_WIN_CHUNKS;
        woff[i][0] = (unsigned)((ay * w2 * SB_C4 + 8 * ch) * 4);
        woff[i][1] = woff[i][0] + (8 * ch + 4 < SB_WIN_FLOATS ? 16u : 0u);
        wlds[i] = ay * SB_WIN_ROW + ch * 16;
    }

    // ---- what is in flight for the next tile
    float4 rg[2][1][2], ry[2][1][2], rw[2][2];
    float finv = 1.f, fkeep = 1.f;
    auto prefetch = [&](int tile) {
        const int64_t row0 = (int64_t)tile * SB_ROWS;
        const int orow = tile / tiles_per_row, ox0 = (tile - orow * tiles_per_row) * SB_ROWS;
        const int img = orow / ho, oy = orow - img * ho;
        const char* xb = reinterpret_cast<const char*>(x2 + (((int64_t)img * h2 + oy) * w2 + ox0) * SB_C4);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            rw[i][0] = *reinterpret_cast<const float4*>(xb + woff[i][0]);
            rw[i][1] = *reinterpret_cast<const float4*>(xb + woff[i][1]);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            split_load<SB_ROWS>(gy + row0 * SB_COUT, SB_COUT, 0, SB_ROWS, 32 * h, SB_COUT, rg[h]);
            if constexpr (ACT) split_load<SB_ROWS>(y + row0 * SB_COUT, SB_COUT, 0, SB_ROWS, 32 * h, SB_COUT, ry[h]);
        }
        const int64_t row = row0 + (tid >> 2);
        finv = inv != nullptr ? inv[row] : 1.f;
        fkeep = keep != nullptr ? keep[row] : 1.f;
    };

    // ---- fragment addresses.  Transposing read: lane (q = lane & 15, g1 = (lane >> 4) & 1, hi) points at row 8 hi + (q >> 2) + 4 j of
    // the contraction step, columns 16 g1 + 4 (q & 3) .. of the wave's 32
    const int q = lane & 15, g1 = (lane >> 4) & 1;
    int tro[2];                                           // dy sub-tile (swizzled, gemm_dxdw.hip)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = 8 * hi + (q >> 2) + 4 * j, chunk = 2 * g1 + ((q & 3) >> 1);
        tro[j] = row * 64 + ((chunk ^ ((2 * hi + j) & 3)) << 4) + (q & 1) * 8;
    }
    const unsigned char* Gb = Gs + wu * SB_SUB;
    const unsigned char* Wa[3];                           // window: 16-column block b = 2 (2 s + wr) + g1 -> row ay = b / 3, columns 16 (b % 3) ..
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int b = 2 * (2 * s + wr) + g1, ay = b / 3, jb = b - 3 * ay;
        Wa[s] = Wn + ay * SB_WIN_ROW + (8 * hi + (q >> 2)) * SB_ROW_STEP + (16 * jb + 4 * (q & 3)) * 2;
    }

    if (tile_beg < tile_end) prefetch(tile_beg);
    for (int tile = tile_beg; tile < tile_end; ++tile) {
        __syncthreads();                                  // the fragment reads of the previous tile are done
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (wvalid[i]) {
                float v[8];
                sb_unpack(rw[i], v);
                u32x4 pl[3];
                split8<3>(v, pl);
#pragma unroll
                for (int p = 0; p < 3; ++p) *reinterpret_cast<u32x4*>(Wn + p * SB_WIN_PLANE + wlds[i]) = pl[p];
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float v[8];
            sb_unpack(rg[h][0], v);
            if constexpr (ACT) {                          // act_bwd_kernel's own product (act_grad, LeakyReLU): the same dy
                float a[8];
                sb_unpack(ry[h][0], a);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = v[e] * (a[e] > 0.f ? 1.f : slope);
                rg[h][0][0] = make_float4(v[0], v[1], v[2], v[3]);
                rg[h][0][1] = make_float4(v[4], v[5], v[6], v[7]);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) dbacc[h][e] += v[e] * fkeep;
            const float s0[1] = {finv}, s1[1] = {finv};
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 none[2] = {z, z};
            split_store<SB_ROWS, 3, true, false>(Gs + h * SB_SUB, rg[h], 32 * h, 0x7fffffff, s0, s1, none, none, 1.f, 0.f, SB_ROWS, SB_COUT);
        }
        __syncthreads();
        prefetch(tile + 1 < tile_end ? tile + 1 : tile);  // flies during the MFMA phase (after the last tile: a harmless reload)
        __builtin_amdgcn_s_setprio(2);
        sb_step<0>(Gb, tro[0], tro[1], Wa, acc);
        sb_step<1>(Gb, tro[0], tro[1], Wa, acc);
        sb_step<2>(Gb, tro[0], tro[1], Wa, acc);
        sb_step<3>(Gb, tro[0], tro[1], Wa, acc);
        __builtin_amdgcn_s_setprio(0);
    }

    // ---- the block's slab: dw[k'][co], k' = 32 (2 s + wr) + accumulator row, co = 32 wu + li; then the bias sums
    float* pz = part + (int64_t)blockIdx.x * SB_SLAB;
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = 32 * (2 * s + wr) + (r & 3) + 8 * (r >> 2) + 4 * hi;
            pz[k * SB_COUT + 32 * wu + li] = acc[s][r];
        }
    __syncthreads();
    float* Ds = reinterpret_cast<float*>(Gs);             // [64 rows][64 columns] of per-thread sums (16 KB of the dy image)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 8; ++e) Ds[(tid >> 2) * SB_COUT + 32 * h + 8 * (tid & 3) + e] = dbacc[h][e];
    __syncthreads();
    if (tid < SB_COUT) {
        float t = 0.f;
        for (int r = 0; r < SB_ROWS; ++r) t += Ds[r * SB_COUT + tid];
        pz[SB_K * SB_COUT + tid] = t;
    }
}

// reduced slab [192 k'][64 co] | [64] -> dwk [co][c][ay][ax] (k' = 48 ay + 12 ax + c) and db
__global__ void stem_bwd_finish_kernel(const float* __restrict__ red, float* __restrict__ dwk, float* __restrict__ db) {
    const int o = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (o < SB_K * SB_COUT) {
        const int co = o / SB_K, rem = o - co * SB_K;
        const int c = rem >> 4, ay = (rem >> 2) & 3, ax = rem & 3;
        dwk[o] = red[(48 * ay + 12 * ax + c) * SB_COUT + co];
    } else if (o < SB_SLAB && db != nullptr) {
        db[o - SB_K * SB_COUT] = red[o];
    }
}

static bool sb_geom_ok(int n, int h2, int w2, int c4, int cout, int kh, int kw, int stride, int ho, int wo) {
    if (n <= 0 || ho <= 0 || wo <= 0 || c4 != SB_C4 || cout != SB_COUT || kh != SB_KA || kw != SB_KA || stride != 1) return false;
    if (wo % SB_ROWS != 0 || wo > (1 << 20) || h2 != ho + SB_KA - 1 || w2 != wo + SB_KA - 1) return false;
    return (int64_t)n * ho * (wo / SB_ROWS) < (1ll << 31);
}

// split-M plan: one full wave of blocks (2 per CU), contiguous tile ranges
static void sb_plan(int n, int ho, int wo, int* nblocks, int* tiles_per_block) {
    const int64_t ntiles = (int64_t)n * ho * (wo / SB_ROWS);
    int64_t want = (int64_t)device_cus() * 2;
    if (want > ntiles) want = ntiles;
    const int64_t tpb = cdiv64(ntiles, want);
    *tiles_per_block = (int)tpb;
    *nblocks = (int)cdiv64(ntiles, tpb);
}

}  // namespace tsii

using namespace tsii;

extern "C" int tsii_stem_bwd_ok(const float* gy, const float* y, const float* x2, int n, int h2, int w2, int c4, int cout,
                                int kh, int kw, int stride, int ho, int wo) {
    if (gemm_products() != 6) return 0;                  // the 6-product split-bf16 arithmetic only
    if (!sb_geom_ok(n, h2, w2, c4, cout, kh, kw, stride, ho, wo)) return 0;
    return (gy != nullptr && x2 != nullptr && aligned16(gy) && aligned16(x2) && aligned16(y)) ? 1 : 0;
}

// tiles (64 output pixels) a block of the kernel walks for this shape on this device; 0: not eligible
extern "C" int tsii_stem_bwd_tiles_per_block(int n, int ho, int wo) {
    if (!sb_geom_ok(n, ho + SB_KA - 1, wo + SB_KA - 1, SB_C4, SB_COUT, SB_KA, SB_KA, 1, ho, wo)) return 0;
    int nb = 0, tpb = 0;
    sb_plan(n, ho, wo, &nb, &tpb);
    return tpb;
}

extern "C" size_t tsii_stem_bwd_ws_bytes(int n, int ho, int wo) {
    if (!sb_geom_ok(n, ho + SB_KA - 1, wo + SB_KA - 1, SB_C4, SB_COUT, SB_KA, SB_KA, 1, ho, wo)) return 0;
    int nb = 0, tpb = 0;
    sb_plan(n, ho, wo, &nb, &tpb);
    return ((size_t)nb + 1) * SB_SLAB * sizeof(float);
}

extern "C" int tsii_stem_bwd(const float* gy, const float* y, float slope, const float* inv, const float* keep, const float* x2,
                             int n, int h2, int w2, int c4, int cout, int kh, int kw, int stride, int ho, int wo,
                             float* dwk, float* db, void* ws, size_t ws_bytes, void* stream) {
    TSII_REQUIRE(gy && x2 && dwk && ws, "stem_bwd: null pointer");
    TSII_REQUIRE(gemm_products() == 6, "stem_bwd: the 6-product split-bf16 arithmetic only (tsii_set_gemm_products)");
    TSII_REQUIRE(sb_geom_ok(n, h2, w2, c4, cout, kh, kw, stride, ho, wo),
                 "stem_bwd: n=%d x2 %dx%dx%d cout=%d taps %dx%d stride %d out %dx%d is not eligible (tsii_stem_bwd_ok)", n, h2, w2, c4, cout, kh,
                 kw, stride, ho, wo);
    TSII_REQUIRE(aligned16(gy) && aligned16(y) && aligned16(x2) && aligned16(ws), "stem_bwd: 16-byte aligned operands are required");
    TSII_REQUIRE(ws_bytes >= tsii_stem_bwd_ws_bytes(n, ho, wo), "stem_bwd: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    int nb = 0, tpb = 0;
    sb_plan(n, ho, wo, &nb, &tpb);
    const int ntiles = (int)((int64_t)n * ho * (wo / SB_ROWS));
    float* part = (float*)ws;
    float* red = part + (size_t)nb * SB_SLAB;
    if (y != nullptr) hipLaunchKernelGGL((stem_bwd_kernel<true>), dim3(nb), dim3(256), 0, st, gy, y, slope, inv, keep, x2, ho, wo, part, ntiles, tpb);
    else hipLaunchKernelGGL((stem_bwd_kernel<false>), dim3(nb), dim3(256), 0, st, gy, y, slope, inv, keep, x2, ho, wo, part, ntiles, tpb);
    int rc = check_launch("stem_bwd");
    if (rc) return rc;
    rc = launch_reduce_rows(part, nb, SB_SLAB, red, st);
    if (rc) return rc;
    hipLaunchKernelGGL(stem_bwd_finish_kernel, dim3(cdiv(SB_SLAB, 256)), dim3(256), 0, st, red, dwk, db);
    return check_launch("stem_bwd_finish");
}
