/*
 * tsii_hip.h -- C ABI of libtsii_hip.so, the MI355X (gfx950) kernels behind the
 * partial-convolution inpainting hot path of yu45020/Text_Segmentation_Image_Inpainting.
 *
 * The reference has no FFI/plugin seam (pure Python nn.Modules calling aten ops), so this
 * ABI is the seam a replacement .so provides underneath the reference's nn.Module surface;
 * each entry point names the reference lines whose aten ops it replaces (paths relative to
 * the reference repo root).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *  - fp32 everywhere.  Activations are NHWC-contiguous ([N,H,W,C]; a 1x1 conv sees them as
 *    a row-major [M=N*H*W, C] matrix).  Mask "planes" are [N,H,W] fp32 holding exactly 0/1
 *    (or small integer counts); a channel-constant mask [N,C,H,W] is represented by its plane.
 *  - The caller owns every buffer (outputs, workspaces); nothing is allocated, freed or
 *    retained by the library.  All calls are asynchronous on `stream` (a hipStream_t).
 *  - Return value: 0 = enqueued; negative = invalid argument / unsupported shape / HIP
 *    launch error, message via tsii_last_error() (thread-local).  Never throws.
 *  - "row scale" (r0, split, r1): element (row m, channel k) of the operand is multiplied by
 *    r0[m] if k < split else r1[m]; r0 == NULL disables it; r1 == NULL means 1.0 for k >= split.
 *    This is how x*mask (partial_convolution.py:51,123) is fused for masks made of one or
 *    two channel-constant planes (decoder concat of up-sampled + skip masks,
 *    image_inpainting.py:83-84).
 */
#ifndef TSII_HIP_H
#define TSII_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSII_ABI_VERSION 27

/* activation kinds for the BN/activation kernels */
#define TSII_ACT_NONE 0
#define TSII_ACT_RELU 1
#define TSII_ACT_LEAKY 2 /* slope argument */
#define TSII_ACT_RELU6 3
#define TSII_ACT_SIGMOID 4

int tsii_version(void);
const char* tsii_last_error(void);

/* Arithmetic of the point-wise / implicit-GEMM matrix products.  The switch is THREAD-LOCAL: it applies to the entry points
 * the calling thread calls afterwards and nothing another thread does can change it (the only other state the library keeps is
 * the thread-local error string and a read-only device-properties cache).  A host that runs forward and backward on
 * different threads (PyTorch autograd does) sets it on each of them -- the package's `_lib.call` does so before every call.
 *   6 (default) split-bf16: each fp32 operand is split exactly into 3 bf16 pieces while it is staged, the 6 partial
 *               products of weight >= 2^-16 go through v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- dropped terms
 *               <= 2^-23 |a*b|, i.e. fp32-class results at 2.7x the matrix-core rate of the f32-input MFMA;
 *   8           the same with the two 2^-24 cross terms as well (only the 2^-32 term is dropped): 2x the f32 MFMA rate;
 *   3           2 pieces / 3 partial products (error <= 2^-15 |a*b|): inference-grade, opt-in;
 *   1           operands rounded to bf16, one product (fp32 accumulation, fp32 storage everywhere else): the "mixed bf16"
 *               arithmetic of BASELINE config 5, tolerance 1e-2 class, opt-in;
 *   0           v_mfma_f32_32x32x2_f32 (bit-exact fp32 FMA chain).
 * The environment variable TSII_GEMM_PRODUCTS sets every thread's initial value; -1 puts the calling thread back to it.
 * inputs/outputs are fp32 in every mode.
 * Range caveat of the split modes: an operand that is inf, or finite but beyond the largest bf16 (3.39e38), splits into
 * (inf, NaN, NaN) -- where the f32 MFMA mode gives +-inf for that row, these give NaN; both rows are lost either way. */
int tsii_set_gemm_products(int products);
int tsii_get_gemm_products(void);

/* ---- K1: mask bookkeeping (partial_convolution.py:57-66,74-77,129-135) --------------- */

/* plane[n,h,w] = sum_c mask[n,c,h,w]; mask given with element strides (any layout).
 * With c == 1 this extracts channel 0 (the `mask[:, :1]` of :59 / :104). */
int tsii_mask_channel_sum(const float* mask, int n, int h, int w, int c,
                          int64_t sn, int64_t sh, int64_t sw, int64_t sc,
                          float* plane, void* stream);

/* S = a0*p0 + a1*p1 (p1 may be NULL); cnt = box_{kh x kw, stride, pad, dilation}(S) with zero
 * padding (padding counts as hole); hole = (cnt == 0).
 *   fill_holes != 0 (PartialConv :60-66,74-75): denom = hole ? 1 : cnt*post_scale,
 *                                               new_mask = hole ? 0 : 1, inv = hole ? 0 : 1/denom
 *   fill_holes == 0 (PartialConvNoHoles :130-135): denom = cnt*post_scale, new_mask = 1, inv = 1/denom
 * post_scale = Cin for same_holes (:61), 1 otherwise.  All values are small integers: bit-exact.
 * Any of denom / new_mask / inv may be NULL. */
int tsii_mask_update(const float* p0, float a0, const float* p1, float a1,
                     int n, int h, int w,
                     int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                     int ho, int wo, float post_scale, int fill_holes,
                     float* denom, float* new_mask, float* inv, void* stream);

/* nearest x2 up-sampling of a plane (DoubleUpSample on the mask, partial_convolution.py:231) */
int tsii_plane_upsample2x(const float* in, int n, int h, int w, float* out, void* stream);

/* out = x * mask, both NHWC with identical shape (general per-channel masks, :51) */
int tsii_mul_mask(const float* x, const float* mask, int64_t numel, float* out, void* stream);
/* dx = dy * mask */
/* (same entry point: multiplication is its own adjoint) */

/* ---- K3: point-wise (1x1) convolution as an MFMA GEMM ---- ------------------------------
 * PartialConv1x1 (:101-105), PartialConvNoHoles k=1 (:121-137), PartialConv k=1.
 *   y[m,n] = keep[m] ? (sum_k x[m,k]*rs(m,k)*w[n,k]) / denom[m] + bias[n] : 0
 * denom/keep/bias/r0 may be NULL (plain conv). */
/* ws: weight workspace of tsii_pw_ws_bytes(n, k) bytes -- in the split-bf16 arithmetic modes (tsii_set_gemm_products)
 * the weights are split into bf16 planes there once per call (otherwise every block splits its weight tile again while
 * staging it); NULL is allowed. */
size_t tsii_pw_ws_bytes(int n, int k);
int tsii_pw_fwd(const float* x, int64_t m, int k, const float* w, int n, const float* bias,
                const float* r0, int split, const float* r1,
                const float* denom, const float* keep, float* y, void* ws, size_t ws_bytes, void* stream);
/* dx[m,k] = rs(m,k) * sum_n dy[m,n]*inv[m]*w[n,k];  wt_ws: tsii_pw_ws_bytes(n, k) bytes of scratch (required) */
int tsii_pw_bwd_dx(const float* dy, int64_t m, int n, const float* w, int k, const float* inv,
                   const float* r0, int split, const float* r1, float* dx, float* wt_ws, void* stream);
/* dw[n,k] = sum_m dy[m,n]*inv[m] * x[m,k]*rs(m,k);  dbias[n] = sum_m dy[m,n]*keep[m] (dbias may be
 * NULL; keep NULL = all rows: the bias is added after the division, so its gradient is not scaled) */
size_t tsii_pw_bwd_dw_ws_bytes(int64_t m, int n, int k);
int tsii_pw_bwd_dw(const float* dy, const float* x, int64_t m, int n, int k, const float* inv, const float* keep,
                   const float* r0, int split, const float* r1, float* dw, float* dbias,
                   void* ws, size_t ws_bytes, void* stream);
/* K3x: tsii_pw_bwd_dx and tsii_pw_bwd_dw of one layer from ONE pass over dy (n = the wide side, k <= 128 the thin one): the same
 * dx, dw and dbias, every argument as in those two calls.  6-product split-bf16 arithmetic only; the shape must pass
 * tsii_pw_bwd_dxdw_ok(m, n, k, 0): m % 64 == 0, n % 32 == 0, k % 32 == 0 and (k <= 64, n <= 384) or (k <= 128, n <= 192) -- the
 * [n x k] weight-gradient accumulators stay in registers.  _ok with min_m >= 0 accepts every such shape of at least min_m rows;
 * min_m < 0 is the library's own choice: only the measured class, k == 64 and 256 <= n <= 384 at m >= 524288 (below that the
 * layer is matrix-bound), everything else keeps the two calls.  ws: tsii_pw_bwd_dxdw_ws_bytes(m, n, k) bytes. */
int tsii_pw_bwd_dxdw_ok(int64_t m, int n, int k, int64_t min_m);
int tsii_pw_bwd_dxdw_tiles_per_block(int64_t m, int n, int k);   /* 64-row tiles one block walks on this device (0: not eligible) */
size_t tsii_pw_bwd_dxdw_ws_bytes(int64_t m, int n, int k);
int tsii_pw_bwd_dxdw(const float* dy, const float* x, int64_t m, int n, const float* w, int k, const float* inv,
                     const float* keep, const float* r0, int split, const float* r1, float* dx, float* dw, float* dbias,
                     void* ws, size_t ws_bytes, void* stream);
/* K3xb: tsii_bn_bwd_apply + tsii_pw_bwd_dxdw in one pass, without the dy tensor between them.  da [m, n]: the gradient w.r.t. the
 * output of the BatchNorm(+act) that follows the layer; y [m, n]: that BatchNorm's raw input (the layer's output); coef [6][n]: the
 * table tsii_bn_bwd_reduce leaves; act / slope: a load-time activation (none, ReLU, ReLU6, LeakyReLU with slope in [0, 1]).  The kernel
 * forms g = dy * inv with dy the very bits tsii_bn_bwd_apply would write, and is K3x from there on: dx and dw equal those of the two
 * calls bit for bit.  dbias must be NULL (a 1x1 layer in front of a BatchNorm has no bias; layers with one keep the two calls); keep
 * is accepted for symmetry and not read.  Shapes: tsii_pw_bwd_dxdw_bn_ok(m, n, k, 0): as K3x with k <= 64 and n <= 256; min_m < 0:
 * the measured class only, k == 64, n == 256, m >= 524288.  da, y, x, ws 16-byte aligned; ws: tsii_pw_bwd_dxdw_bn_ws_bytes. */
int tsii_pw_bwd_dxdw_bn_ok(int64_t m, int n, int k, int64_t min_m);
int tsii_pw_bwd_dxdw_bn_tiles_per_block(int64_t m, int n, int k);
size_t tsii_pw_bwd_dxdw_bn_ws_bytes(int64_t m, int n, int k);
int tsii_pw_bwd_dxdw_bn(const float* da, const float* y, const float* coef, int act, float slope, const float* x, int64_t m, int n,
                        const float* w, int k, const float* inv, const float* keep, const float* r0, int split, const float* r1,
                        float* dx, float* dw, float* dbias, void* ws, size_t ws_bytes, void* stream);

/* ---- K2: depth-wise partial convolution (PartialConv groups=C, MobileNetV2.py:174-176) --
 *   y[n,ho,wo,c] = keep ? (sum_taps w[c,t]*x[n,hi,wi,c]*rmask[n,hi,wi]) / denom[n,ho,wo] + b[c] : 0
 * w is the reference layout [C,1,kh,kw]; ws: c*kh*kw floats of scratch. */
int tsii_dw_fwd(const float* x, const float* rmask, const float* w, const float* bias,
                const float* denom, const float* keep,
                int n, int h, int wd, int c, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                int ho, int wo, float* y, float* ws, void* stream);
int tsii_dw_bwd_dx(const float* dy, const float* inv, const float* w, const float* rmask,
                   int n, int h, int wd, int c, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                   int ho, int wo, float* dx, float* ws, void* stream);
size_t tsii_dw_bwd_dw_ws_bytes(int n, int ho, int wo, int c, int kh, int kw);
int tsii_dw_bwd_dw(const float* dy, const float* inv, const float* keep, const float* x, const float* rmask,
                   int n, int h, int wd, int c, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                   int ho, int wo, float* dwgt, float* dbias, void* ws, size_t ws_bytes, void* stream);

/* ---- K4: dense k x k partial convolution, groups == 1 (PartialConv.forward :49-80) ------
 * x*mask is either the two-plane row scale (r0/split/r1 at input resolution) or a full
 * per-channel mask `mfull` (same NHWC shape as x; ImageFill stem, image_inpainting.py:23).
 * w is the reference layout [Cout,Cin,kh,kw]. */
size_t tsii_dense_ws_bytes(int cin, int cout, int kh, int kw);
int tsii_dense_fwd(const float* x, const float* mfull, const float* r0, int split, const float* r1,
                   const float* w, const float* bias, const float* denom, const float* keep,
                   int n, int h, int wd, int cin, int cout,
                   int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int ho, int wo,
                   float* y, void* ws, size_t ws_bytes, void* stream);
int tsii_dense_bwd_dx(const float* dy, const float* inv, const float* w,
                      const float* mfull, const float* r0, int split, const float* r1,
                      int n, int h, int wd, int cin, int cout,
                      int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int ho, int wo,
                      float* dx, void* ws, size_t ws_bytes, void* stream);
size_t tsii_dense_bwd_dw_ws_bytes(int n, int ho, int wo, int cin, int cout, int kh, int kw);
int tsii_dense_bwd_dw(const float* dy, const float* inv, const float* keep, const float* x,
                      const float* mfull, const float* r0, int split, const float* r1,
                      int n, int h, int wd, int cin, int cout,
                      int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int ho, int wo,
                      float* dwgt, float* dbias, void* ws, size_t ws_bytes, void* stream);

/* ---- K4c: the decoder's last level without its concatenated tensor: 3x3 / stride 1 / pad 1 PartialConv with <= 4 output
 * channels over cat(nearest-x2(low [n,h/2,wd/2,c1]), skip [n,h,wd,c2])  (DoubleUpSample + torch.cat + the 35 -> 3 output layer,
 * models/partial_convolution.py:224-231, models/image_inpainting.py:82-86).  r0 / r1: mask planes [n,h,wd] of the two parts
 * (NULL = ones; the x*mask split is the concat boundary c1), denom / keep / inv as for tsii_dense_*.  Equal to
 * tsii_upcat_fwd + tsii_dense_fwd (and tsii_dense_bwd_dx + tsii_upcat_bwd, tsii_dense_bwd_dw) to rounding.
 * tsii_head_cat_ok() != 0: this geometry has the fused kernels (h, wd even, c1 % 4 == 0, 20 < c1 + c2 <= 68, cout <= 4).
 * ws: tsii_dense_ws_bytes(c1 + c2, cout, 3, 3) (fwd, bwd_dx) / tsii_dense_bwd_dw_ws_bytes(n, h, wd, c1 + c2, cout, 3, 3) (bwd_dw).
 * dskip may be NULL (the skip is a data tensor). */
int tsii_head_cat_ok(int n, int h, int wd, int c1, int c2, int cout);
int tsii_head_cat_fwd(const float* low, const float* skip, int c1, int c2, const float* r0, const float* r1,
                      const float* w, const float* bias, const float* denom, const float* keep,
                      int n, int h, int wd, int cout, float* y, void* ws, size_t ws_bytes, void* stream);
int tsii_head_cat_bwd_dx(const float* dy, const float* inv, const float* w, int c1, int c2, const float* r0, const float* r1,
                         int n, int h, int wd, int cout, float* dlow, float* dskip, void* ws, size_t ws_bytes, void* stream);
int tsii_head_cat_bwd_dw(const float* dy, const float* inv, const float* keep, const float* low, const float* skip,
                         int c1, int c2, const float* r0, const float* r1, int n, int h, int wd, int cout,
                         float* dwgt, float* dbias, void* ws, size_t ws_bytes, void* stream);
/* K4d: tsii_head_cat_bwd_dw on the f32 matrix cores (v_mfma_f32_16x16x4_f32, exact fp32), with the low part's mask given where
 * it lives: r0_low [n, h/2, wd/2] is the mask plane of `low` itself (NULL = ones) -- the up-sampled half is then constant over
 * each 2x2 block and its share of the product runs over LOW-resolution pixels against 2x2 box sums of dy*inv.
 * tsii_head_cat_low_ok() != 0: h % 16 == 0, wd % 64 == 0 (whole 16 x 64 tiles), c1 in {32, 64}, 1 <= c2 <= 16, cout <= 3.
 * Same workspace as tsii_head_cat_bwd_dw. */
int tsii_head_cat_low_ok(int n, int h, int wd, int c1, int c2, int cout);
/* ... the weight gradient AND the gradient of `low` in one pass (the box sums the former holds in LDS are the left operand of the
 * latter: dlow[j][ci] = r0_low[j] * sum_m S[j][m] W[m][ci]); tsii_head_cat_bwd_low_ok(): tsii_head_cat_low_ok() and c1 == 32.
 * = tsii_head_cat_bwd_dw_low + the d low half of tsii_head_cat_bwd_dx (no d skip: the skip is a data tensor). */
int tsii_head_cat_bwd_low_ok(int n, int h, int wd, int c1, int c2, int cout);
int tsii_head_cat_bwd_low(const float* dy, const float* inv, const float* keep, const float* low, const float* skip,
                          int c1, int c2, const float* r0_low, const float* r1, const float* w, int n, int h, int wd, int cout,
                          float* dwgt, float* dbias, float* dlow, void* ws, size_t ws_bytes, void* stream);
/* ... and the forward pass: the up-sampled half as Z[low pixel][(tap, cout)] = W_low x low on the matrix cores (kept in LDS per
 * tile), 9 entries of Z per output pixel and channel + the 3-channel skip half on the vector ALU.  tsii_head_cat_fwd_low_ok():
 * tsii_head_cat_low_ok() and c2 == 3.  No workspace. */
int tsii_head_cat_fwd_low_ok(int n, int h, int wd, int c1, int c2, int cout);
int tsii_head_cat_fwd_low(const float* low, const float* skip, int c1, int c2, const float* r0_low, const float* r1,
                          const float* w, const float* bias, const float* denom, const float* keep,
                          int n, int h, int wd, int cout, float* y, void* stream);
int tsii_head_cat_bwd_dw_low(const float* dy, const float* inv, const float* keep, const float* low, const float* skip,
                             int c1, int c2, const float* r0_low, const float* r1, int n, int h, int wd, int cout,
                             float* dwgt, float* dbias, void* ws, size_t ws_bytes, void* stream);

/* ---- K4b: stems (odd k, stride 2, pad (k-1)/2, very few input channels; models/image_inpainting.py:23) as a stride-1
 * valid convolution over the space-to-depth image, so they run on the vector-gather implicit GEMM:
 *   tsii_stem_s2d:   x [n,h,w,c] * mask (mfull, or the r0/split/r1 planes, or none) zero-padded by `pad`
 *                    -> out [n,(h+2pad)/2,(w+2pad)/2,4c], channel order (row phase, column phase, c)
 *   tsii_stem_w_fwd: w [cout,cin,k,k] -> w2 [cout,4cin,ka,ka], ka = (k+1)/2 (reference layout of that conv)
 *   tsii_stem_w_bwd: dw2 [cout,4cin,ka,ka] -> dw [cout,cin,k,k]
 * then tsii_dense_fwd / tsii_dense_bwd_dw on (out, w2) with kernel ka, stride 1, padding 0. */
int tsii_stem_s2d(const float* x, const float* mfull, const float* r0, int split, const float* r1,
                  int n, int h, int w, int c, int pad, float* out, void* stream);
int tsii_stem_w_fwd(const float* w, int cout, int cin, int k, float* w2, void* stream);
int tsii_stem_w_bwd(const float* dw2, int cout, int cin, int k, float* dw, void* stream);
/* K4s: the stem's backward in one pass over its output gradient gy [m = n ho wo, 64]: dwk [64][12][4][4] (what tsii_dense_bwd_dw
 * leaves for tsii_stem_w_bwd) and db [64] (may be NULL) of the 4x4 valid convolution over x2 [n, h2, w2, 12].  With y (the stem's
 * pre-activation output, [m, 64]) the gradient of the LeakyReLU behind the stem is formed on load: dy = gy * (y > 0 ? 1 : slope),
 * tsii_act_bwd's own product; y NULL: dy = gy.  dwk = sum dy * inv * x2 (inv NULL = ones), db = sum dy * keep (keep NULL = ones).
 * 6-product split-bf16 arithmetic only.  tsii_stem_bwd_ok() != 0: c4 == 12, 4x4 taps, stride 1, cout == 64, wo % 64 == 0,
 * h2 == ho + 3, w2 == wo + 3, arithmetic mode 6, gy / y / x2 16-byte aligned; everything else keeps tsii_act_bwd +
 * tsii_dense_bwd_dw, and the entry point refuses it.  ws: tsii_stem_bwd_ws_bytes(n, ho, wo) bytes, 16-byte aligned. */
int tsii_stem_bwd_ok(const float* gy, const float* y, const float* x2, int n, int h2, int w2, int c4, int cout,
                     int kh, int kw, int stride, int ho, int wo);
int tsii_stem_bwd_tiles_per_block(int n, int ho, int wo);        /* 64-pixel tiles one block walks on this device (0: not eligible) */
size_t tsii_stem_bwd_ws_bytes(int n, int ho, int wo);
int tsii_stem_bwd(const float* gy, const float* y, float slope, const float* inv, const float* keep, const float* x2,
                  int n, int h2, int w2, int c4, int cout, int kh, int kw, int stride, int ho, int wo,
                  float* dwk, float* db, void* ws, size_t ws_bytes, void* stream);

/* ---- K6: BatchNorm2d (+activation, +residual)  (partial_convolution.py:193-197,
 *          residual add MobileNetV2.py:186-187, image_inpainting.py:216) ------------------
 * y is [M,C].  Training: batch mean / biased variance (and running-stat update with
 * momentum, unbiased variance, like nn.BatchNorm2d); eval: pass the running stats to apply. */
size_t tsii_bn_ws_bytes(int64_t m, int c);
int tsii_bn_stats(const float* y, int64_t m, int c, float* mean, float* var,
                  float* running_mean, float* running_var, float momentum,
                  void* ws, size_t ws_bytes, void* stream);
/* out = act(gamma*(y-mean)/sqrt(var+eps)+beta) (+ residual) */
int tsii_bn_act_fwd(const float* y, int64_t m, int c, const float* mean, const float* var,
                    const float* gamma, const float* beta, float eps, int act, float slope,
                    const float* residual, float* out, void* stream);
/* training != 0: full batch-stat backward; else eval backward.  dgamma/dbeta always written. */
int tsii_bn_act_bwd(const float* dout, const float* y, int64_t m, int c,
                    const float* mean, const float* var, const float* gamma, const float* beta,
                    float eps, int act, float slope, int training,
                    float* dy, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);

/* ---- K6b: BatchNorm folded into the neighbouring convolutions (training-time fusion of the reference's
 *           Sequential(conv, BatchNorm2d, act, conv ...) chains, e.g. models/MobileNetV2.py:168-179) -----
 * Producer side ("stat_part"): the conv kernel also writes, per block of output rows and per channel,
 *   (count, p, sum(y - p), sum((y - p)^2)) with the pivot p a value of that block (no cancellation for
 *   near-constant channels), as float [rows][4][c_out]; rows = tsii_pw_stat_rows(m) /
 *   tsii_dw_stat_rows(...).  tsii_bn_finalize() combines them (fp64, parallel-variance formula) into the
 *   batch mean / biased variance, updates the running statistics like nn.BatchNorm2d and emits
 *   scale = gamma/sqrt(var+eps), shift = beta - mean*scale -- no separate pass over y.
 * Consumer side ("in_scale/in_shift"): the next conv applies a = act(in_scale[c]*v + in_shift[c]) to every
 *   element it loads (before the x*mask multiply; zero padding pads a), so the normalised activation is never
 *   written to HBM.  in_scale == NULL: plain input; in_act is NONE, RELU, LEAKY (slope in [0,1]) or RELU6 (the
 *   load-time form is min(max(z, neg*z), hi); anything else is an error).  The *_bwd_dw_bn forms recompute a the same way;
 *   dX is unchanged (it is the gradient w.r.t. a) and feeds tsii_bn_act_bwd together with the raw y. */
int64_t tsii_pw_stat_rows(int64_t m);
int tsii_pw_fwd_bn(const float* x, int64_t m, int k, const float* w, int n, const float* bias,
                   const float* r0, int split, const float* r1, const float* denom, const float* keep,
                   const float* in_scale, const float* in_shift, int in_act, float in_slope,
                   float* stat_part, float* y, void* ws, size_t ws_bytes, void* stream);
int tsii_pw_bwd_dw_bn(const float* dy, const float* x, int64_t m, int n, int k, const float* inv, const float* keep,
                      const float* r0, int split, const float* r1,
                      const float* in_scale, const float* in_shift, int in_act, float in_slope,
                      float* dw, float* dbias, void* ws, size_t ws_bytes, void* stream);
/* 0 when the geometry has no LDS-tiled kernel (then only the unfused entry points apply) */
int64_t tsii_dw_stat_rows(int n, int ho, int wo, int c, int kh, int kw, int sh, int sw, int dh, int dw);
int tsii_dw_fwd_bn(const float* x, const float* rmask, const float* w, const float* bias,
                   const float* denom, const float* keep,
                   int n, int h, int wd, int c, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                   int ho, int wo, const float* in_scale, const float* in_shift, int in_act, float in_slope,
                   float* stat_part, float* y, float* ws, void* stream);
int tsii_dw_bwd_dw_bn(const float* dy, const float* inv, const float* keep, const float* x, const float* rmask,
                      int n, int h, int wd, int c, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                      int ho, int wo, const float* in_scale, const float* in_shift, int in_act, float in_slope,
                      float* dwgt, float* dbias, void* ws, size_t ws_bytes, void* stream);
/* dense k x k forward with the statistics partials ([rows][4][cout]); rows == 0: this geometry is not on the
 * implicit-GEMM path (few-output-channel / generic kernels), use tsii_dense_fwd + tsii_bn_stats */
int64_t tsii_dense_stat_rows(int has_mfull, int n, int h, int wd, int cin, int cout, int kh, int kw, int sh, int sw,
                             int ph, int pw, int dh, int dw, int ho, int wo);
int tsii_dense_fwd_bn(const float* x, const float* mfull, const float* r0, int split, const float* r1,
                      const float* w, const float* bias, const float* denom, const float* keep,
                      int n, int h, int wd, int cin, int cout,
                      int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int ho, int wo,
                      float* stat_part, float* y, void* ws, size_t ws_bytes, void* stream);
size_t tsii_bn_finalize_ws_bytes(int64_t rows, int c);
/* scale/shift may be NULL (then gamma/beta may be too) */
int tsii_bn_finalize(const float* stat_part, int64_t rows, int c, int64_t m,
                     float* mean, float* var, float* running_mean, float* running_var, float momentum,
                     const float* gamma, const float* beta, float eps, float* scale, float* shift,
                     void* ws, size_t ws_bytes, void* stream);
/* ---- K6c: the two reductions of the BatchNorm backward taken by the kernel that PRODUCES its incoming gradient.
 * tsii_dw_bwd_dx_bn: depth-wise dX (3x3; stride 1 / dilation 1, or stride 2 / pad 1 / dilation 1: the marching-strip paths,
 *   rows = tsii_dw_bwd_stat_rows(n,h,wd,c,...) > 0) whose output dx is the gradient w.r.t. a = act(BN(bn_y)), bn_y being the raw [n,h,wd,c] tensor the depth-wise conv consumed
 *   through its load-time BatchNorm; it also writes bwd_part[rows][2][c] = per-strip (sum dz, sum dz*xhat),
 *   dz = dx*act'(z).  tsii_bn_act_bwd_pre is tsii_bn_act_bwd without its reduction pass (ws: tsii_bn_ws_bytes(m, c)). */
int64_t tsii_dw_bwd_stat_rows(int n, int h, int wd, int c, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw);
int tsii_dw_bwd_dx_bn(const float* dy, const float* inv, const float* w, const float* rmask,
                      int n, int h, int wd, int c, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                      int ho, int wo, const float* bn_y, const float* bn_mean, const float* bn_var,
                      const float* bn_gamma, const float* bn_beta, float bn_eps, int bn_act, float bn_slope,
                      float* dx, float* bwd_part, float* ws, void* stream);
/* K6d: tsii_dw_bwd_dx_bn that ALSO returns the layer's weight gradient dwgt[c][1][3][3] (no bias gradient: the layer has no bias) --
 * the dX pass holds dy * inv with its halo in LDS and forms the layer's input act(BN(bn_y)) * rmask at its own pixels for the K6c
 * sums, i.e. both operands of dW; tsii_dw_bwd_dw_bn's second pass over (dy, bn_y) is not run.  3x3; stride 1 at dilation 1 / 2 / 4 / 8 (padding 0..2d; not the row-phase kernel's geometries) or stride 2 / padding 1 / dilation 1:
 * ws_dw of tsii_dw_bwd_dxdw_ws_bytes(...) bytes, 0 = no such form for this geometry (call the two separate entry points).
 * Replaces the autograd of F.conv2d(groups=C) in models/partial_convolution.py:49-51 for dX and dW together. */
size_t tsii_dw_bwd_dxdw_ws_bytes(int n, int h, int wd, int c, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw);
int tsii_dw_bwd_dxdw_bn(const float* dy, const float* inv, const float* w, const float* rmask,
                        int n, int h, int wd, int c, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                        int ho, int wo, const float* bn_y, const float* bn_mean, const float* bn_var,
                        const float* bn_gamma, const float* bn_beta, float bn_eps, int bn_act, float bn_slope,
                        float* dx, float* bwd_part, float* dwgt, float* ws, void* ws_dw, size_t ws_dw_bytes, void* stream);
/* K6e: tsii_dw_bwd_dxdw_bn fed with the gradient w.r.t. the ACTIVATION that follows the layer: da2 = d loss / d act2(BN2(y2)), y2 = the
 * layer's raw output (bn2_y, same [n,ho,wo,c] layout), bn2_coef[6][c] = (mean, 1/std, gamma, beta, dbeta/m, dgamma/m) of BN2 as
 * tsii_bn_bwd_reduce leaves it -- BN2's backward is applied while the kernel stages its slab, so tsii_bn_act_bwd_pre's pass over
 * (da2, y2) -> dy2 and this kernel's read of dy2 become this kernel's reads of da2 and y2.  Stride 1 / dilation 1 and stride 2 / padding 1
 * (tsii_dw_bwd_dxdw_fold_ok() == 1); everything else as tsii_dw_bwd_dxdw_bn.
 * tsii_bn_bwd_reduce / tsii_bn_bwd_apply: the two halves of tsii_bn_act_bwd_pre (reduction of the K6c partial rows to dgamma, dbeta
 * and the table; the stand-alone apply pass over the table: dy = ((dout act'(z) - coef[4]) - xhat coef[5]) gamma / std).
 * Together they replace the autograd of nn.BatchNorm2d + activation in models/partial_convolution.py:176-180 (bn_act). */
int tsii_dw_bwd_dxdw_fold_ok(int n, int h, int wd, int c, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw);
int tsii_dw_bwd_dxdw_bn2(const float* da2, const float* bn2_y, const float* bn2_coef, int bn2_act, float bn2_slope,
                         const float* inv, const float* w, const float* rmask,
                         int n, int h, int wd, int c, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                         int ho, int wo, const float* bn_y, const float* bn_mean, const float* bn_var,
                         const float* bn_gamma, const float* bn_beta, float bn_eps, int bn_act, float bn_slope,
                         float* dx, float* bwd_part, float* dwgt, float* ws, void* ws_dw, size_t ws_dw_bytes, void* stream);
size_t tsii_bn_bwd_reduce_ws_bytes(int64_t rows, int c);
int tsii_bn_bwd_reduce(const float* mean, const float* var, const float* gamma, const float* beta, float eps, int training,
                       const float* bwd_part, int64_t rows, int64_t m, int c, float* dgamma, float* dbeta, float* coef,
                       void* ws, size_t ws_bytes, void* stream);
int tsii_bn_bwd_apply(const float* dout, const float* y, int64_t m, int c, const float* coef, int act, float slope, float* dy,
                      void* stream);
/* same for the point-wise dX (N = k % 4 == 0): dx is the gradient w.r.t. a = act(BN(bn_y)), bn_y raw [m,k];
 * bwd_part[tsii_pw_stat_rows(m)][2][k] */
int tsii_pw_bwd_dx_bn(const float* dy, int64_t m, int n, const float* w, int k, const float* inv,
                      const float* r0, int split, const float* r1,
                      const float* bn_y, const float* bn_mean, const float* bn_var, const float* bn_gamma,
                      const float* bn_beta, float bn_eps, int bn_act, float bn_slope,
                      float* dx, float* bwd_part, float* wt_ws, void* stream);
int tsii_bn_act_bwd_pre(const float* dout, const float* y, int64_t m, int c,
                        const float* mean, const float* var, const float* gamma, const float* beta,
                        float eps, int act, float slope, int training, const float* bwd_part, int64_t rows,
                        float* dy, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);
/* tsii_bn_act_bwd_pre that ALSO leaves pooled[n, y/2, x/2, :] = sum over the 2x2 block of dy[n, y, x, :] * pool_scale[n, y, x]
 * (rows of dy = pixels of [.., up_h, up_w] images, both even; pool_scale NULL = 1): dy is the gradient of a tsii_pw_fwd_up
 * output, pooled the gradient of its up-sampled addend (= tsii_pool2x2_scaled(dy, pool_scale), without the second pass). */
int tsii_bn_act_bwd_pre_pool(const float* dout, const float* y, int64_t m, int c,
                             const float* mean, const float* var, const float* gamma, const float* beta,
                             float eps, int act, float slope, int training, const float* bwd_part, int64_t rows,
                             int up_h, int up_w, const float* pool_scale, float* dy, float* pooled,
                             float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);
/* eval mode: (scale, shift) from the running statistics */
int tsii_bn_scale_shift(const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                        int c, float* scale, float* shift, void* stream);
/* activation only (PartialActivation :204-211): out = act(x); dx = dout*act'(x) */
int tsii_act_fwd(const float* x, int64_t numel, int act, float slope, float* out, void* stream);
int tsii_act_bwd(const float* dout, const float* x, int64_t numel, int act, float slope, float* dx, void* stream);

/* ---- K7: nearest x2 up-sampling + channel concat (DoubleUpSample + torch.cat,
 *          partial_convolution.py:229-231, image_inpainting.py:82-85) --------------------
 * out[n,y,x,0:c1] = low[n,y/2,x/2,:], out[n,y,x,c1:] = skip[n,y,x,:];  low is [n,h,w,c1].
 * c2 == 0 (skip NULL) is the plain DoubleUpSample of x. */
int tsii_upcat_fwd(const float* low, const float* skip, int n, int h, int w, int c1, int c2,
                   float* out, void* stream);
int tsii_upcat_bwd(const float* dout, int n, int h, int w, int c1, int c2,
                   float* dlow, float* dskip, void* stream);

/* ---- K7b (round 4): the same DoubleUpSample + torch.cat in front of a 1x1 partial convolution, never written --------------
 * A 1x1 convolution commutes with nearest up-sampling and distributes over the channel concatenation:
 *   conv1x1(cat(up2(low), skip) * mask) = up2(conv1x1_low(low * mask_low)) + conv1x1_skip(skip * mask_skip)
 * (models/partial_convolution.py:121-137 over image_inpainting.py:82-85), so the decoder's expand convolutions run their
 * low-resolution half at LOW resolution -- a quarter of its multiply-adds, and the concatenated tensor never exists:
 *   z = tsii_pw_fwd(low, ..)                       plain [m/4, n] product at low resolution
 *   y = tsii_pw_fwd_up(skip, .., up_add = z)       y[row] = keep ? (acc[row] + z[low_row(row)]) / denom + bias : 0
 * rows of y are the pixels of [.., up_h, up_w] images (up_h even, up_w % 4 == 0, m % (up_h*up_w) == 0, n % 4 == 0, m < 2^31);
 * stat_part (or NULL) as in tsii_pw_fwd_bn.  Backward: tsii_pw_bwd_dx / tsii_pw_bwd_dw on the skip half as usual, and
 * dz = tsii_pool2x2_scaled(dy, inv) -- dlow[n,y,x,:] = sum of the 2x2 block of dout[n,2y+dy,2x+dx,:] * scale[n,2y+dy,2x+dx]
 * (scale NULL = 1; dout is [n,2h,2w,c]) -- is the gradient of z. */
int tsii_pw_fwd_up(const float* x, int64_t m, int k, const float* w, int n, const float* bias,
                   const float* r0, int split, const float* r1, const float* denom, const float* keep,
                   const float* up_add, int up_h, int up_w, float* stat_part, float* y, void* ws, size_t ws_bytes,
                   void* stream);
int tsii_pool2x2_scaled(const float* dout, const float* scale, int n, int h, int w, int c, float* dlow, void* stream);

/* ---- K11 (first piece): mean-L1 loss (nn.L1Loss, loss.py:190; bench loss of SURVEY 8d) - */
size_t tsii_l1_ws_bytes(int64_t numel);
int tsii_l1_mean_fwd(const float* a, const float* b, int64_t numel, float* loss,
                     void* ws, size_t ws_bytes, void* stream);
/* da = sign(a-b) * (*gscale) / numel;  gscale is a device pointer to the upstream scalar grad */
int tsii_l1_mean_bwd(const float* a, const float* b, int64_t numel, const float* gscale,
                     float* da, void* stream);

/* ---- training-step helpers ---------------------------------------------------------- */
/* fused SGD step (nesterov momentum + weight decay; the optimiser the reference trained with,
 * checkpoints/ReadME.md:4): g += wd*p; buf = mom*buf + g; p -= lr*(g + mom*buf) */
int tsii_sgd_nesterov(float* p, const float* g, float* buf, int64_t numel,
                      float lr, float momentum, float weight_decay, void* stream);

/* ---- segmentation path (models/common.py, models/text_segmentation.py, loss.py) ------- */
/* out = act(a + b): residual adds `x + self.conv(x)` (models/MobileNetV2.py:146-147, models/Xception.py:44)
 * and `act_fn(rfb_pool + resi)` (models/common.py:156).  Backward: tsii_act_bwd(dout, out, ...) twice. */
int tsii_add_act_fwd(const float* a, const float* b, int64_t numel, int act, float slope, float* out, void* stream);
/* channel concat / slice on [M, C] NHWC rows (torch.cat dim=1, models/text_segmentation.py:68,75,80,111;
 * models/common.py:91,151):  to_dst != 0: big[m, coff + c] = small[m, c];  else small[m, c] = big[m, coff + c] */
int tsii_copy_channels(float* big, int64_t m, int cbig, int coff, float* small_, int csmall, int to_dst, void* stream);
/* bilinear up-sampling by an integer factor, align_corners=False (F.interpolate / nn.Upsample,
 * models/text_segmentation.py:54,76,109,113); x is [n,h,w,c], y is [n,h*s,w*s,c] */
int tsii_bilinear_up_fwd(const float* x, int n, int h, int w, int c, int scale, float* y, void* stream);
int tsii_bilinear_up_bwd(const float* dy, int n, int h, int w, int c, int scale, float* dx, void* stream);
/* global average pool (nn.AdaptiveAvgPool2d(1), models/common.py:19,35): gap[n,c] = mean_hw x[n,hw,c] */
size_t tsii_gap_ws_bytes(int n, int hw, int c);
int tsii_gap_fwd(const float* x, int n, int hw, int c, float* gap, void* ws, size_t ws_bytes, void* stream);
int tsii_gap_bwd(const float* dgap, int n, int hw, int c, float* dx, void* stream);
/* scSE combine (models/common.py:38-43): out = x*cse[n,c] + x*sse[n,hw];
 * backward: dx = g*(cse+sse), dcse[n,c] = sum_hw g*x, dsse[n,hw] = sum_c g*x */
int tsii_scse_fwd(const float* x, const float* cse, const float* sse, int n, int hw, int c, float* out, void* stream);
int tsii_scse_bwd(const float* g, const float* x, const float* cse, const float* sse, int n, int hw, int c,
                  float* dx, float* dcse, float* dsse, void* ws, size_t ws_bytes, void* stream);
/* BinaryFocalLoss (loss.py:58-75): mean( exp(gamma*logsigmoid(-x*(2t-1))) * w*BCEwithlogits(x,t) ),
 * w = words_w if t > 0 else background_w.  ws: tsii_l1_ws_bytes(numel). */
int tsii_bce_focal_fwd(const float* x, const float* t, int64_t numel, float gamma, float background_w, float words_w,
                       float* loss, void* ws, size_t ws_bytes, void* stream);
int tsii_bce_focal_bwd(const float* x, const float* t, int64_t numel, float gamma, float background_w, float words_w,
                       const float* gscale, float* dx, void* stream);

/* pixel shuffle by r on NHWC (the reference only mentions it in its README; semantics =
 * torch.nn.PixelShuffle on NCHW): x [n,h,w,c*r*r] -> y [n,h*r,w*r,c], y[n,h*r+i,w*r+j,c] = x[n,h,w,c*r*r+i*r+j].
 * inverse != 0 runs the adjoint / un-shuffle (y -> x). */
int tsii_pixel_shuffle(const float* src, int n, int h, int w, int c, int r, int inverse, float* dst, void* stream);

/* ---- InpaintingLoss pieces (loss.py:195-225,303-307) ------------------------------------ */
/* comp = mask*raw + (1-mask)*out (loss.py:196); backward: dout = dcomp*(1-mask) */
int tsii_compose_fwd(const float* raw, const float* mask, const float* out, int64_t numel, float* comp, void* stream);
int tsii_compose_bwd(const float* dcomp, const float* mask, int64_t numel, float* dout, void* stream);
/* loss = w_valid*mean|m*out - m*gt| + w_hole*mean|(1-m)*out - (1-m)*gt|  (loss.py:199-200,223); ws: tsii_l1_ws_bytes */
int tsii_masked_l1_fwd(const float* out, const float* gt, const float* mask, int64_t numel, float w_valid, float w_hole,
                       float* loss, void* ws, size_t ws_bytes, void* stream);
int tsii_masked_l1_bwd(const float* out, const float* gt, const float* mask, int64_t numel, float w_valid, float w_hole,
                       const float* gscale, float* dout, void* stream);
/* total_variation_loss (loss.py:303-307) on NHWC [n,h,w,c]: mean|x[:,:,:,:-1]-x[:,:,:,1:]| + mean|x[:,:,:-1,:]-x[:,:,1:,:]| */
int tsii_tv_fwd(const float* x, int n, int h, int w, int c, float* loss, void* ws, size_t ws_bytes, void* stream);
int tsii_tv_bwd(const float* x, int n, int h, int w, int c, const float* gscale, float* dx, void* stream);

/* ==== bf16 ACTIVATION STORAGE (BASELINE config 5: "mixed bf16 with fp32 mask renorm"; round 5) ==========================
 * The segmentation nets (models/text_segmentation.py:18-114 and their blocks: models/MobileNetV2.py:114-149,
 * models/Xception.py:13-114, models/common.py:53-156, models/BaseModels.py:91-127) with activations AND activation
 * gradients kept in HBM as bf16 NHWC; parameters, parameter gradients, BatchNorm statistics, every accumulation and every
 * reduction stay fp32.  `uint16_t*` = raw bf16 bits; every channel count is a multiple of 8 (one 16-byte vector; the host
 * pads the 3-channel stem to 4 and a 1-channel head to 8), every tensor base is 16-byte aligned.  A kernel reads bf16,
 * computes in fp32 and rounds once (RNE) when it stores; the BatchNorm partials a kernel emits describe the ROUNDED values.
 * These nets carry no mask planes, so the entry points have none (the partial-convolution family keeps fp32 storage: its
 * count division / hole logic is the "fp32 mask renorm" of the config and no shipped model combines the two).
 * Layouts of the partial rows are those of the fp32 entry points above (stat_part [rows][4][c], bwd_part [rows][2][c]), so
 * tsii_bn_finalize and the fp32 reductions are shared. */

/* ---- matrix products: 1x1 convolutions (bf16 x bf16 -> fp32 on v_mfma_f32_32x32x16_bf16) ---------------------------- */
int64_t tsii_bf16_stat_rows(int64_t m);                 /* partial rows of the NT kernels: one per 128 output rows */
size_t tsii_bf16_pw_ws_bytes(int n, int k);             /* bf16 image of the weights, written once per call */
/* y[m,n] = sum_k a(x[m,k]) w[n,k] + bias[n],  a = act(in_scale*x + in_shift) applied while loading (in_scale NULL: a = x);
 * stat_part (or NULL): BatchNorm partials of y [tsii_bf16_stat_rows(m)][4][n] */
int tsii_bf16_pw_fwd(const uint16_t* x, int64_t m, int k, const float* w, int n, const float* bias,
                     const float* in_scale, const float* in_shift, int in_act, float in_slope,
                     float* stat_part, uint16_t* y, void* ws, size_t ws_bytes, void* stream);
/* dx[m,k] = sum_n dy[m,n] w[n,k]; with bn_y (raw [m,k] input of the BatchNorm the conv consumed on load, K6c) also
 * bwd_part[tsii_bf16_stat_rows(m)][2][k] = (sum dz, sum dz*xhat), dz = dx*act'(z).  ws: tsii_bf16_pw_ws_bytes(n, k). */
int tsii_bf16_pw_bwd_dx(const uint16_t* dy, int64_t m, int n, const float* w, int k,
                        const uint16_t* bn_y, const float* bn_mean, const float* bn_var, const float* bn_gamma,
                        const float* bn_beta, float bn_eps, int bn_act, float bn_slope,
                        uint16_t* dx, float* bwd_part, void* ws, size_t ws_bytes, void* stream);
/* dw[n,k] = sum_m dy[m,n] a(x[m,k]) (fp32);  dbias[n] = sum_m dy[m,n] (or NULL) */
size_t tsii_bf16_pw_bwd_dw_ws_bytes(int64_t m, int n, int k);
int tsii_bf16_pw_bwd_dw(const uint16_t* dy, const uint16_t* x, int64_t m, int n, int k,
                        const float* in_scale, const float* in_shift, int in_act, float in_slope,
                        float* dw, float* dbias, void* ws, size_t ws_bytes, void* stream);
/* ---- dense k x k convolutions, groups == 1, as implicit GEMM (w: reference layout [cout,cin,kh,kw], fp32) ------------- */
size_t tsii_bf16_dense_ws_bytes(int cin, int cout, int kh, int kw);
int tsii_bf16_dense_fwd(const uint16_t* x, const float* w, const float* bias, int n, int h, int wd, int cin, int cout,
                        int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int ho, int wo,
                        float* stat_part /* [tsii_bf16_stat_rows(n*ho*wo)][4][cout] or NULL */, uint16_t* y,
                        void* ws, size_t ws_bytes, void* stream);
int tsii_bf16_dense_bwd_dx(const uint16_t* dy, const float* w, int n, int h, int wd, int cin, int cout,
                           int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int ho, int wo,
                           uint16_t* dx, void* ws, size_t ws_bytes, void* stream);
size_t tsii_bf16_dense_bwd_dw_ws_bytes(int n, int ho, int wo, int cin, int cout, int kh, int kw);
int tsii_bf16_dense_bwd_dw(const uint16_t* dy, const uint16_t* x, int n, int h, int wd, int cin, int cout,
                           int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int ho, int wo,
                           float* dwgt, float* dbias, void* ws, size_t ws_bytes, void* stream);

/* ---- depth-wise 3x3 convolutions (Conv_block(groups = C), models/BaseModels.py:105-127) and stride-1 average pools -------
 * w: reference layout [c,1,3,3] fp32.  Geometry: 3x3, stride 1 with any dilation or stride 2 with dilation 1, square padding.
 * in_scale / in_shift / stat_part: K6b as for the fp32 entry points (the virtual activation a = act(in_scale*x + in_shift) is
 * rounded to bf16 like a stored one; zero padding pads a).  tsii_bf16_dw_stat_rows: rows of stat_part [rows][4][c] (0: geometry
 * not supported).  The forward and the stride-1 dX are one kernel (the adjoint is the same stencil with flipped taps). */
int64_t tsii_bf16_dw_stat_rows(int n, int ho, int wo, int c, int kh, int kw, int sh, int sw, int dh, int dw);
int tsii_bf16_dw_fwd(const uint16_t* x, const float* w, const float* bias, int n, int h, int wd, int c,
                     int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int ho, int wo,
                     const float* in_scale, const float* in_shift, int in_act, float in_slope,
                     float* stat_part, uint16_t* y, void* stream);
/* K6c: with bn_y (the raw [n,h,wd,c] tensor this conv consumed through its load-time BatchNorm) the kernel also leaves
 * bwd_part[tsii_bf16_dw_bwd_stat_rows(..)][2][c]; rows == 0 (stride 2): pass NULL and run tsii_bf16_bn_act_bwd instead */
int64_t tsii_bf16_dw_bwd_stat_rows(int n, int h, int wd, int c, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw);
int tsii_bf16_dw_bwd_dx(const uint16_t* dy, const float* w, int n, int h, int wd, int c,
                        int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int ho, int wo,
                        const uint16_t* bn_y, const float* bn_mean, const float* bn_var, const float* bn_gamma,
                        const float* bn_beta, float bn_eps, int bn_act, float bn_slope,
                        uint16_t* dx, float* bwd_part, void* stream);
size_t tsii_bf16_dw_bwd_dw_ws_bytes(int n, int ho, int wo, int c, int kh, int kw, int sh, int sw, int dh, int dw);
int tsii_bf16_dw_bwd_dw(const uint16_t* dy, const uint16_t* x, int n, int h, int wd, int c,
                        int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int ho, int wo,
                        const float* in_scale, const float* in_shift, int in_act, float in_slope,
                        float* dwgt, float* dbias, void* ws, size_t ws_bytes, void* stream);
/* nn.AvgPool2d(k, stride 1, padding (k-1)/2), count_include_pad (models/common.py:62-68), k in {3, 5, 9}; the operator is
 * its own adjoint: the backward pass is the same call on the gradient */
int tsii_bf16_avgpool(const uint16_t* x, int n, int h, int wd, int c, int k, uint16_t* y, void* stream);

/* ---- streaming kernels ------------------------------------------------------------------------------------------------
 * BatchNorm statistics of a bf16 [m,c] tensor as partial rows in the stat_part layout ([tsii_bf16_bn_stat_rows(m,c)][4][c]);
 * tsii_bn_finalize turns them into mean / var / running statistics / (scale, shift) like the conv-emitted partials. */
int64_t tsii_bf16_bn_stat_rows(int64_t m, int c);
int tsii_bf16_bn_stats(const uint16_t* y, int64_t m, int c, float* stat_part, void* stream);
/* out = act(scale*y + shift) (+ residual): the materialised form of a BatchNorm(+activation) (models/BaseModels.py:95-99)
 * from the (scale, shift) pair of tsii_bn_finalize / tsii_bn_scale_shift, i.e. exactly what a load-time consumer computes */
int tsii_bf16_bn_act_fwd(const uint16_t* y, int64_t m, int c, const float* scale, const float* shift, int act, float slope,
                         const uint16_t* residual, uint16_t* out, void* stream);
/* BatchNorm(+act) backward: dy (bf16), dgamma / dbeta (fp32).  bwd_part NULL: the kernel takes its two reductions itself;
 * else [rows][2][c] partials left by the consumer's dX kernel (K6c).  ws: tsii_bf16_bn_ws_bytes(m, c). */
size_t tsii_bf16_bn_ws_bytes(int64_t m, int c);
int tsii_bf16_bn_act_bwd(const uint16_t* dout, const uint16_t* y, int64_t m, int c, const float* mean, const float* var,
                         const float* gamma, const float* beta, float eps, int act, float slope, int training,
                         const float* bwd_part, int64_t rows, uint16_t* dy, float* dgamma, float* dbeta,
                         void* ws, size_t ws_bytes, void* stream);
/* out = act(a + b); dx = dout * act'(x)   (models/Xception.py:44, models/MobileNetV2.py:146-147, models/common.py:156) */
int tsii_bf16_add_act_fwd(const uint16_t* a, const uint16_t* b, int64_t numel, int act, float slope, uint16_t* out, void* stream);
int tsii_bf16_act_bwd(const uint16_t* dout, const uint16_t* x, int64_t numel, int act, float slope, uint16_t* dx, void* stream);
/* channel concat / slice (tsii_copy_channels), bilinear up-sampling (tsii_bilinear_up_*) on bf16 tensors */
int tsii_bf16_copy_channels(uint16_t* big, int64_t m, int cbig, int coff, uint16_t* small_, int csmall, int to_dst, void* stream);
int tsii_bf16_bilinear_up_fwd(const uint16_t* x, int n, int h, int w, int c, int scale, uint16_t* y, void* stream);
int tsii_bf16_bilinear_up_bwd(const uint16_t* dy, int n, int h, int w, int c, int scale, uint16_t* dx, void* stream);
/* the fp32 <-> bf16 boundary: the 3-channel image enters through the stem's space-to-depth rearrangement (tsii_stem_s2d with
 * the channels of each phase padded to 4: out [n,(h+2pad)/2,(w+2pad)/2,16], channel order (row phase, column phase, c4));
 * the logits leave as channel `ch` of a head padded to 8 channels; plain casts for everything else */
int tsii_bf16_stem_s2d(const float* x, int n, int h, int w, int c, int pad, uint16_t* out, void* stream);
int tsii_bf16_from_f32(const float* src, int64_t numel, uint16_t* dst, void* stream);
int tsii_bf16_to_f32(const uint16_t* src, int64_t numel, float* dst, void* stream);
int tsii_bf16_channel_to_f32(const uint16_t* src, int64_t m, int c, int ch, float* dst, void* stream);
int tsii_bf16_channel_from_f32(const float* src, int64_t m, int c, int ch, uint16_t* dst, void* stream);

/* ---- K8: page pipeline -- text removal on a whole page (the reference README's road: text mask -> white the words out -> inpaint;
 * the only reference semantics used are Examples/demo_segmentation.py:33-35, sigmoid > 0.5 and MaxPool2d(3, 1, 1)) ----------------
 * The exceptions to "fp32 everywhere": the page, the text plane and the results are uint8, counts and tile lists int32.
 * Tiling.  S = tile - 2*halo > 0, tile % 32 == 0.  The page [h,w] is cut into ty*tx = ceil(h/S)*ceil(w/S) square tiles, row-major;
 * tile (i,j) covers page rows [i*S - halo, i*S - halo + tile) and the same for columns; its CORE is rows [i*S, (i+1)*S) x columns
 * [j*S, (j+1)*S) clipped to the page.  The cores partition the page: every page pixel is OWNED by exactly one tile, and whatever is
 * said per page pixel below (its logit, its filler output) is the value at that pixel in its owning tile.
 * tsii_page_tile_count: ty*tx (0: geometry refused -- h, w >= 1, h*w and the tile volume within 2^31). */
int tsii_page_tile_count(int h, int w, int tile, int halo);

/* Segmenter tiles: page uint8 [h,w,3] -> tiles fp32 NHWC [ty*tx, tile, tile, 3] (16-byte aligned),
 *   tiles[t,r,q,c] = fmaf((float)page[ry,rx,c], scale_c, shift_c),   (ry, rx) = the tile coordinate mirrored into the page.
 * Mirror reflection does not repeat the edge (period 2*(h-1), applied until the coordinate is inside; a side of 1 maps to 0).
 * For ImageNet-style normalisation the caller passes scale = 1/(255*std), shift = -mean/std. */
int tsii_page_tiles_norm(const uint8_t* page, int h, int w, int tile, int halo,
                         float scale0, float scale1, float scale2, float shift0, float shift1, float shift2,
                         float* tiles, void* stream);

/* Text mask: logits fp32 [ty*tx, tile, tile] (the segmenter's [N,1,T,T]) -> text uint8 [h,w] (1 = text), core_count int32 [ty*tx].
 *   text0 = logit > logit_threshold                       (log(p/(1-p)) for a probability threshold p; 0 = the demo's sigmoid > 0.5)
 *   text  = binary dilation of text0 by a dilate x dilate square, outside the page = no text   (dilate odd, 1..31; 3 = MaxPool2d(3,1,1))
 *   core_count[t] = number of text pixels in the core of tile t -- integer atomics: independent of block order.
 * core_count is cleared by the call itself. */
int tsii_tiles_text_mask(const float* logits, int h, int w, int tile, int halo, float logit_threshold, int dilate,
                         uint8_t* text, int* core_count, void* stream);

/* Filler tiles for the n_sel tiles listed in tile_ids (device int32, tile numbers in [0, ty*tx)):
 *   mask[k,r,q]  = inside the page ? 1 - text : 0                                     fp32 [n_sel, tile, tile]
 *   img[k,r,q,c] = ((float)page[y,x,c] / 255.0f) * mask[k,r,q]  (0 outside the page)   fp32 NHWC [n_sel, tile, tile, 3]
 * -- an IEEE (correctly rounded) fp32 division, then an exact product with 0 / 1; not normalised (Dataloader.py:103-132).
 * Outside the page is a hole, not a reflection: the partial convolution's own border rule (padding counts as hole, K1). */
int tsii_page_tiles_fill(const uint8_t* page, const uint8_t* text, int h, int w, int tile, int halo,
                         const int* tile_ids, int n_sel, float* img, float* mask, void* stream);

/* Compose: clean uint8 [h,w,3], mask_u8 uint8 [h,w] = text * 255.
 *   clean = text ? (uint8) floorf(fmaf(min(max(out, 0), 1), 255, 0.5)) : page        -- bytes outside text are copied untouched
 * out: the filler's output fp32 NHWC [n_sel, tile, tile, 3]; slot: device int32 [ty*tx], the index of each tile in out or -1 (a text
 * pixel whose owning tile has no slot keeps its page byte).  out == slot == NULL with n_sel == 0: a page without text.
 * The four byte planes are 4-byte aligned. */
int tsii_compose_page_u8(const uint8_t* page, const uint8_t* text, const float* out, const int* slot, int n_sel,
                         int h, int w, int tile, int halo, uint8_t* clean, uint8_t* mask_u8, void* stream);

/* Filler WINDOWS: the two entry points above with the tile grid replaced by a table.  Window k is the square of `tile` pixels a side
 * whose first pixel is page row origin[2k], column origin[2k+1] (device int32 [n,2]; any values: negative, partly or wholly off the
 * page, overlapping one another); tile % 32 == 0, there is no halo argument.
 *   mask[k,r,q], img[k,r,q,c]: as tsii_page_tiles_fill, for the page pixel (origin[2k] + r, origin[2k+1] + q) -- the same element
 * arithmetic, bit for bit: a window with a grid tile's origin equals that tile.  n >= 1, n * tile * tile / 4 < 2^31. */
int tsii_page_windows_fill(const uint8_t* page, const uint8_t* text, int h, int w, int tile,
                           const int* origin /* device int32 [n,2]: oy, ox */, int n,
                           float* img /* fp32 NHWC [n,tile,tile,3] */, float* mask /* fp32 [n,tile,tile] */, void* stream);

/* Compose from windows: clean uint8 [h,w,3], mask_u8 uint8 [h,w] = text * 255, as tsii_compose_page_u8.  rect: device int32 [n,4],
 * (y0, x0, y1, x1) half-open, the page rectangle window k OWNS; rectangles may overlap.  The OWNER of a text pixel (y, x) is the
 * lowest k with y0 <= y < y1 and x0 <= x < x1:
 *   clean = (uint8) floorf(fmaf(min(max(out[k, y - origin[2k], x - origin[2k+1], c], 0), 1), 255, 0.5))
 * A text pixel in no rectangle keeps its page byte, and so does one whose owner's rectangle leaves its window there (the caller keeps
 * every rectangle inside its window; nothing is read outside out).  Bytes outside text are copied untouched.
 * out == origin == rect == NULL with n == 0: a page without text.  n <= 1024: more is refused (-1) and nothing is launched.
 * No workspace; the four byte planes are 4-byte aligned. */
int tsii_compose_page_windows_u8(const uint8_t* page, const uint8_t* text, const float* out /* fp32 NHWC [n,tile,tile,3] */,
                                 const int* origin /* [n,2] */, const int* rect /* [n,4] y0,x0,y1,x1 half-open */, int n,
                                 int h, int w, int tile, uint8_t* clean, uint8_t* mask_u8, void* stream);

/* ---- K9: validation metrics (csrc/metrics.hip).  The reference has none (it prints losses); these are this library's own. ---------
 * Besides fp32 tensors: histograms are int32, sums and SSIM values are double.  No floating-point atomics: for the same inputs and
 * shapes every output has the same bits on every run (integer counts meet with integer atomics, floating-point sums leave a block as
 * one double and are added in a fixed order by a last kernel).
 *
 * Confusion histograms of a binary segmenter at k thresholds.  logits, target: fp32 [n, hw] (hw = H*W pixels per image, 1 <= hw < 2^31).
 * A pixel is TEXT (class 1) where target > 0.5f, background (class 0) otherwise (NaN: background).  thresholds: k floats in HOST memory,
 * 1 <= k <= 32, ascending (equal neighbours allowed, NaN refused); they are read during the call and travel as kernel arguments, the
 * array may be reused as soon as the call returns.  They are LOGIT thresholds: log(p / (1 - p)) for a probability p.
 *   hist[i, c, b], int32 [n, 2, k + 1] = number of pixels of image i and class c whose logit exceeds exactly b of the thresholds,
 * with "exceeds" = the fp32 comparison logit > thresholds[j] -- the test tsii_tiles_text_mask applies; NaN exceeds nothing, +inf every
 * finite threshold.  The k + 1 bins of an image's two classes sum to hw.  hist is CLEARED BY THE CALL ITSELF (the caller accumulates).
 * At threshold j:  TP = sum_{b > j} hist[i,1,b],  FN = sum_{b <= j} hist[i,1,b],  FP = sum_{b > j} hist[i,0,b],  TN = sum_{b <= j} hist[i,0,b]. */
int tsii_seg_confusion(const float* logits, const float* target, int n, int64_t hw, const float* thresholds, int k,
                       int* hist, void* stream);

/* Error sums of an inpainting result.  out, clean: fp32 NHWC [n,h,w,c] (h*w*c < 2^31).  mask: fp32, [n,h,w,c] (mask_is_plane == 0) or
 * one plane [n,h,w] shared by the channels (mask_is_plane != 0); an ELEMENT (pixel, channel) is VALID where its mask value > 0.5f and
 * a HOLE otherwise (the data set's convention: 1 = keep, 0 = hole).  With clamp01 != 0, o = fminf(fmaxf(out, 0), 1), else o = out.
 *   d = o - clean                     one fp32 subtraction; |d| and d*d and all sums below in double
 *   sums[i,0] = number of hole elements of image i (a plane mask counts a hole pixel c times)
 *   sums[i,1] = sum |d| over hole elements     sums[i,2] = sum d*d over hole elements
 *   sums[i,3] = sum |d| over valid elements    sums[i,4] = sum d*d over valid elements            sums: double [n,5], 8-byte aligned
 * ws: tsii_inpaint_errors_ws_bytes(n,h,w,c) bytes, 8-byte aligned.  16-byte loads are used when h*w % 4 == 0, c <= 4 and the three
 * tensors are 16-byte aligned; every other case takes an element-wise form with the same results up to the order of the double sums. */
size_t tsii_inpaint_errors_ws_bytes(int n, int h, int w, int c);
int tsii_inpaint_errors(const float* out, const float* clean, const float* mask, int mask_is_plane, int clamp01,
                        int n, int h, int w, int c, double* sums, void* ws, size_t ws_bytes, void* stream);

/* Mean structural similarity (Wang, Bovik, Sheikh, Simoncelli 2004) per image.  a, b: fp32 NHWC [n,h,w,c], 1 <= c <= 4, h, w >= 11
 * (smaller is refused).  L = data_range > 0, C1 = (0.01 L)^2, C2 = (0.03 L)^2.
 *   g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) / sum_j exp(-(j - 5)^2 / (2 * 1.5^2)),  i = 0..10     (sigma 1.5, the 11 weights sum to 1)
 *   for every window position (y, x), 0 <= y <= h - 11, 0 <= x <= w - 11 (windows wholly inside the image) and every channel k:
 *     E[f]  = sum_{i,j} g[i] g[j] f(y + i, x + j, k)
 *     mu_a = E[a], mu_b = E[b], var_a = E[a a] - mu_a^2, var_b = E[b b] - mu_b^2, cov = E[a b] - mu_a mu_b     (population moments)
 *     S = ((2 mu_a mu_b + C1) (2 cov + C2)) / ((mu_a^2 + mu_b^2 + C1) (var_a + var_b + C2))
 *   ssim[i] = mean of S over the (h - 10) (w - 10) positions and the c channels of image i                    double [n], 8-byte aligned
 * The weighted sums are fp32 (fmaf, horizontal pass then vertical pass, weights rounded to fp32), taken of the pixel values minus one
 * reference pixel per 32 x 16 tile and channel (variance and covariance do not depend on it; the means get it back in double), S and its
 * sum are double.  Exactly symmetric in (a, b); ssim(a, a) = 1 exactly.  ws: tsii_ssim_ws_bytes(n,h,w,c) bytes (0: shape refused),
 * 8-byte aligned.  A masked form is not offered: compose first (tsii_compose_fwd). */
size_t tsii_ssim_ws_bytes(int n, int h, int w, int c);
int tsii_ssim(const float* a, const float* b, int n, int h, int w, int c, float data_range, double* ssim, void* ws,
              size_t ws_bytes, void* stream);

/* ---- K10: text regions (csrc/regions.hip) -- connected components of the K8 text plane, their areas and boxes, and a minimum-area
 * filter applied on the device (the reference's demo does this on the host: Examples/demo_segmentation.py:17-25,43 labels the mask,
 * drops the regions below an area threshold and marks the rest).  All integer: the same inputs give the same bits on every run.
 * text: uint8 [h,w], READ AND THEN REWRITTEN IN PLACE; a pixel is foreground where its byte is non-zero.  A COMPONENT is a maximal set
 * of foreground pixels connected through the 4- or 8-neighbourhood (connectivity = 4 or 8) inside the page.  Its LABEL is
 * 1 + min(y*w + x) over its pixels, its AREA its pixel count, its BOX y0, x0 inclusive and y1, x1 exclusive.  A component is KEPT iff
 * area >= min_area (min_area <= 1 keeps everything).
 *   labels[p], int32 [h,w]   = the label of p's component if that component is kept, else 0
 *   text[p]                  = labels[p] != 0 ? 1 : 0
 *   n_regions, int32 [2]     = {components found, components kept}
 *   table, int32 [max_regions, 6]: row r = {label, area, y0, x0, y1, x1} of the r-th kept component in ascending label order (raster
 *     order of each region's first pixel).  Only the first min(kept, max_regions) rows are written, the rows behind them are not
 *     touched; n_regions[1] is the true count, which is how a caller sees the truncation.  max_regions == 0 with table == NULL is allowed.
 *   core_count: NULL (tile and halo are ignored), or int32 [ty*tx] on the K8 tile geometry: cleared by the call, then the number of
 *     KEPT text pixels in each tile core -- what tsii_tiles_text_mask writes, after the filter.
 * No allocation, no host synchronisation, everything on the caller's stream.  ws: tsii_text_regions_ws_bytes(h, w, max_regions) bytes
 * (0: geometry refused), 4-byte aligned; the call leaves nothing there a later call depends on and needs nothing cleared beforehand.
 * Refused (non-zero return, tsii_last_error, nothing written): connectivity not 4 or 8; h or w < 1; h*w > 2^31 - 2; max_regions < 0
 * (or > 0 without a table); a bad tile geometry while core_count != NULL. */
size_t tsii_text_regions_ws_bytes(int h, int w, int max_regions);
int tsii_text_regions(uint8_t* text, int h, int w, int connectivity, int min_area, int max_regions,
                      int tile, int halo, int* core_count, int* labels, int* table, int* n_regions, void* ws, void* stream);

/* ---- K11: working resolution (csrc/resample.hip) -- the two resamplings around a segmenter that works at its own size, as the
 * reference's only end-to-end program does (Dataloader.py:285-317: the page is brought to a working size with Pillow's bicubic filter,
 * the net's mask goes back to the page through nn.Upsample(bilinear, align_corners=False) and "> 0").  Integer arithmetic on the device;
 * the same inputs give the same bits on every run.
 *
 * Bicubic resize of a uint8 page, byte for byte PIL.Image.resize((ws, hs), Image.BICUBIC) of an RGB image.  Per axis, from the input
 * size `in` and the output size `out` (refused unless in, out >= 1 and in <= 8 out and out <= 8 in: a row then has at most 33 taps):
 *   scale = in / out, fs = max(scale, 1.0), support = 2.0 * fs, taps = 2 * (int)ceil(support) + 1              (double precision)
 *   for the output index xx: center = (xx + 0.5) * scale, xmin = max(0, (int)(center - support + 0.5)),
 *     xmax = min(in, (int)(center + support + 0.5)), n = xmax - xmin
 *   w[x] = bicubic((x + xmin - center + 0.5) / fs), x = 0..n-1, with a = -0.5:
 *     ((a + 2)|t| - (a + 3)) t^2 + 1 for |t| < 1,   (((|t| - 5)|t| + 8)|t| - 4) a for |t| < 2,   0 otherwise
 *   w is divided by its sum (accumulated in index order); k[x] = (int)(w[x] * 2^22 + 0.5), or (int)(w[x] * 2^22 - 0.5) for w[x] < 0
 *   out[xx] = clip8((2^21 + sum_x k[x] * in[xmin + x]) >> 22)            int32 accumulation, arithmetic shift, clip8 = clamp to 0..255
 * The horizontal pass runs first, to a uint8 intermediate, then the vertical pass; a pass with in == out is skipped.
 * tsii_resize_taps: the row length of the table for (in, out); 0 = refused.
 * tsii_resize_coeffs_u8: a plain HOST function (no device work, no stream): fills the host arrays bounds int32 [out, 2] = {xmin, n}
 * and kk int32 [out, taps] (entries behind n are 0), in double precision with floating-point contraction off.
 * tsii_page_resize_u8: page uint8 [h,w,3] -> out uint8 [hs,ws,3]; the four tables are DEVICE copies of what tsii_resize_coeffs_u8
 * made for (h, hs) and (w, ws), taps_y / taps_x their row lengths (checked); the tables of a skipped pass may be NULL.  No
 * workspace, no allocation, the caller's stream.  Bounds read from a table are clamped to the buffers before use. */
int tsii_resize_taps(int in, int out);
int tsii_resize_coeffs_u8(int in, int out, int* bounds, int* kk);
int tsii_page_resize_u8(const uint8_t* page, int h, int w, int hs, int ws, const int* bounds_y, const int* kk_y,
                        const int* bounds_x, const int* kk_x, int taps_y, int taps_x, uint8_t* out, void* stream);

/* Working-resolution text plane onto the page: text_s uint8 [hs,ws] (non-zero = text; what tsii_tiles_text_mask leaves for the working
 * page's own tile grid) -> text uint8 [h,w] of 0 / 1 and core_count int32 [ty*tx] on the PAGE's K8 tile geometry (cleared by the call;
 * integer atomics), the convention of tsii_tiles_text_mask: selection, tsii_text_regions, fill and compose run unchanged behind it.
 * "Bilinear, align_corners = False, then > 0" in integers.  Per axis, for the destination index d, source size in, destination size out:
 *   num = max(0, (2 d + 1) * in - out),  i0 = num / (2 out),  frac = num % (2 out),  i1 = frac ? min(i0 + 1, in - 1) : i0
 * and a page pixel is text iff any of its up to four taps (y0 | y1, x0 | x1) is.  This equals torch's interpolate(...) > 0 wherever no
 * tap has a weight of exactly zero (there the float32 rounding of the weight decides in torch; here the tap does not count).
 * Refused: a bad tile geometry; hs or ws < 1; (2 h + 1) * hs or (2 w + 1) * ws >= 2^31. */
int tsii_text_plane_up(const uint8_t* text_s, int hs, int ws, int h, int w, int tile, int halo,
                       uint8_t* text, int* core_count, void* stream);

/* ---- K12: region hulls (csrc/hull.hip) -- the last step of the reference's demo (Examples/demo_segmentation.py: cv2.convexHull of every
 * region that passed the area filter, drawn filled): the convex hull of every region in the table is filled into the text plane on the
 * device, behind tsii_text_regions.  All integer, every product and cross product in int64: one defined answer, exact for every page
 * tsii_text_regions accepts, the same bits on every run.
 * Inputs as tsii_text_regions leaves them: text uint8 [h,w] (non-zero = text), labels int32 [h,w], table int32 [max_regions,6],
 * n_regions int32 [2] ON THE DEVICE (the call does not read it on the host).  R = min(n_regions[1], max_regions) table rows are in use;
 * for r < R, C_r is the set of pixels whose label is table[r][0], taken as integer points (y, x), and H_r the set of integer points of
 * the page in the CLOSED convex hull of C_r (boundary points are in; collinear and single-pixel components give a segment or a point).
 * Row form: a component meets every row of its box; with xmin_r(y), xmax_r(y) its leftmost and rightmost pixel in row y of [y0, y1),
 * L_r the greatest convex function <= xmin_r and U_r the least concave function >= xmax_r on those rows, row y of H_r is the interval
 * [ceil(L_r(y)), floor(U_r(y))]; between two neighbouring envelope vertices (ya, xa), (yb, xb) the envelope at row y is
 * (xa (yb - y) + xb (y - ya)) / (yb - ya), rounded with exact integer ceiling (left side) or floor (right side).
 *   text[p]                       = 1 iff text[p] != 0 on entry or p lies in some H_r, else 0.  Hulls may overlap one another, cover
 *     background and cover regions the area filter dropped.  Kept regions beyond the table (kept > max_regions) keep their own pixels
 *     and get no hull.
 *   hull_area, int32 [max_regions]: hull_area[r] = |H_r| for r < R; the rows behind R are not touched.
 *   core_count: NULL (tile and halo are ignored), or int32 [ty*tx] on the K8 tile geometry: cleared by the call, then the number of text
 *     pixels of the FINAL plane in each tile core (integer atomics: independent of block order).
 *   labels, table and n_regions are read only.
 * No allocation, no host synchronisation, everything on the caller's stream; no grid-wide barrier and no waiting on another block.
 * ws: tsii_region_hulls_ws_bytes(h, w, max_regions) bytes (0: geometry refused), 4-byte aligned; it depends on (h, w, max_regions)
 * only, needs nothing cleared beforehand and holds nothing a later call depends on.  (Distinct regions share no pixel and each has a
 * run in every row of its box, so the (region, row) extents of all regions number at most min(max_regions * h, h * ceil(w / 2)); a
 * prefix sum of the box heights over the table, on the device, gives every region its offset inside that bound.)
 * Refused (non-zero return, tsii_last_error, nothing written): h or w < 1; h*w > 2^31 - 2; max_regions < 1; a NULL among text, labels,
 * table, n_regions, hull_area, ws; a bad tile geometry while core_count != NULL.
 * Every box or count read from table or n_regions is clamped to the page and to max_regions before use: a table that does not belong to
 * the labels gives wrong bytes, never an access outside the buffers (the rule of tsii_page_resize_u8). */
size_t tsii_region_hulls_ws_bytes(int h, int w, int max_regions);
int tsii_region_hulls(uint8_t* text, const int* labels, int h, int w, const int* table, const int* n_regions, int max_regions,
                      int tile, int halo, int* core_count, int* hull_area, void* ws, void* stream);

/* ---- K13: flat regions (csrc/flat.hip) -- the reference README's middle step, "use the generated mask to white out words", for the text
 * that sits on one flat colour (a speech bubble): a region whose surrounding RING of page pixels is uniform within `tol` grey levels is
 * painted with the ring's mean colour on the device and leaves the text plane; only what is left goes to an inpainting net.  All integer
 * (the channel sums in 64 bits): exact for every page tsii_text_regions accepts, the same bits on every run.
 * Inputs: page uint8 [h,w,3]; text uint8 [h,w] (non-zero = text), REWRITTEN IN PLACE; labels int32 [h,w], table int32 [max_regions,6] and
 * n_regions int32 [2] ON THE DEVICE exactly as tsii_text_regions leaves them FOR THIS VERY PLANE (every text pixel has a non-zero label;
 * a plane changed since, by tsii_region_hulls for one, is labelled again first); ring 1..8; tol 0..255.  Only the label column of the
 * table is read.  R = min(n_regions[1], max_regions); for r < R:
 *   C_r      the pixels whose label is table[r][0]
 *   Ring_r   the page pixels q with text[q] == 0 on entry for which some p in C_r has max(|qy - py|, |qx - px|) <= ring.  A pixel may lie
 *            in several rings; pixels of other regions (in the table or not) lie in none; the page edge clips the ring
 *   n_r = |Ring_r|;  lo_c, hi_c, sum_c per channel c: minimum, maximum and sum of the ORIGINAL page bytes over Ring_r
 *   flat_r   iff n_r >= 1 and hi_c - lo_c <= tol for all three channels
 *   colour_r[c] = (2 sum_c + n_r) / (2 n_r) in integer division (the mean, halves rounded up); 0 where n_r == 0
 * Outputs:
 *   painted, uint8 [h,w,3] (not the page itself): colour_r on C_r where flat_r holds, the page byte everywhere else
 *   text[p]  = 0 on the flat regions, 1 where it was non-zero otherwise, else 0.  Regions beyond the table (kept > max_regions) are never
 *              flat and stay text
 *   mask, uint8 [h,w] or NULL: 255 where text was non-zero ON ENTRY, else 0 -- the mask of everything that is removed, painted or
 *              inpainted.  (tsii_compose_page_u8 and tsii_compose_page_windows_u8 keep their behaviour: behind this call they get
 *              `painted` as their page and the reduced plane, their own mask output -- of the reduced plane -- goes to a scratch buffer
 *              and this one is the page's mask.)
 *   core_count: NULL (tile and halo are ignored), or int32 [ty*tx] on the K8 tile geometry: cleared by the call, then the text pixels of
 *              the FINAL plane in each tile core (integer atomics: independent of block order)
 *   flat, int32 [max_regions,5]: row r < R = {flat_r, colour_r[0], colour_r[1], colour_r[2], n_r}; the rows behind R are not touched
 *   labels, table and n_regions are read only.
 * No allocation, no host synchronisation, everything on the caller's stream; no grid-wide barrier and no waiting on another block.
 * ws: tsii_flat_regions_ws_bytes(h, w, max_regions) bytes (0: geometry refused), 8-BYTE aligned; it depends on (h, w, max_regions) only,
 * needs nothing cleared beforehand and holds nothing a later call depends on.
 * Refused (non-zero return, tsii_last_error, nothing written): h or w < 1; h*w > 2^31 - 2; max_regions < 1; ring outside 1..8; tol outside
 * 0..255; a NULL among page, text, labels, table, n_regions, painted, flat, ws; painted == page; a bad tile geometry while
 * core_count != NULL.  The count read from n_regions is clamped to max_regions and every table row is found by a search below it: a
 * table that does not belong to the labels gives wrong bytes, never an access outside the buffers. */
size_t tsii_flat_regions_ws_bytes(int h, int w, int max_regions);
int tsii_flat_regions(const uint8_t* page, uint8_t* text, const int* labels, int h, int w, const int* table, const int* n_regions,
                      int max_regions, int ring, int tol, int tile, int halo, int* core_count, uint8_t* painted, uint8_t* mask,
                      int* flat, void* ws, void* stream);

/* ---- K14: harmonic fill (csrc/harmonic.hip) -- a filler that is a kernel and not a net: the holes of an image are filled with the smooth
 * continuation of the pixels around them (Laplace's equation over the holes, the valid pixels as the boundary), in ONE coarse-to-fine
 * pass.  Per image; the 3 channels share one validity plane.
 * Inputs: x fp32 NHWC [n,h,w,3]; mask fp32 [n,h,w], a pixel is VALID iff mask != 0 (the plane tsii_page_tiles_fill writes: 1 = keep,
 * 0 = hole); sweeps 0..16.  Output: out fp32 NHWC [n,h,w,3], never x itself.  The value of x at a hole pixel is NEVER USED (it may be NaN
 * or Inf): values are selected by validity, not multiplied by the mask.
 *   1. Levels.  Level 0 is the image: v_0 = x on valid pixels, m_0 = valid.  Level l+1 has ceil(h_l / 2) x ceil(w_l / 2) pixels; the
 *      children of its pixel (i, j) are the level-l pixels (2i..2i+1, 2j..2j+1) that exist (2 or 1 at an odd edge); m_{l+1} = any child
 *      valid, v_{l+1} = the mean of the VALID children.  Level L is the 1 x 1 level.
 *   2. Apex.  u_L = v_L if m_L, else 0: an image without a valid pixel comes back as zeros.
 *   3. Coarse to fine, l = L-1 .. 0: u_l = v_l on the pixels valid at level l and u_{l+1}(i / 2, j / 2) (the relaxed parent, nearest) on
 *      the others; then `sweeps` Jacobi sweeps: in each, every pixel that is a HOLE at level l becomes the mean of its in-bounds
 *      4-neighbours' values from before the sweep (2, 3 or 4 of them on a level of two pixels a side or more, 1 or 2 on a level one
 *      pixel wide; nothing mirrored).  Valid pixels never change.
 *   4. out = u_0; on valid pixels out equals x bit for bit.
 * Every hole value is a convex combination of valid inputs.  Every mean adds its terms in one fixed order (children: row by row; neighbours:
 * up, down, left, right) and divides by their count: the result does not depend on how the work is cut into blocks, an image of a batch
 * equals the same image run alone, two runs give the same bits.  No atomics.
 * No allocation, no host synchronisation, everything on the caller's stream.
 * ws: tsii_harmonic_fill_ws_bytes(n, h, w) bytes (0: geometry refused; the coarse levels' values and validity bytes, about 0.36 of x),
 * 4-byte aligned (16 for the vector paths); needs nothing cleared beforehand and holds nothing a later call depends on.
 * Refused (non-zero return, tsii_last_error, nothing launched): n, h or w < 1; n*h*w*3 > 2^31; sweeps outside 0..16; a NULL among x, mask,
 * out, ws; out == x. */
size_t tsii_harmonic_fill_ws_bytes(int n, int h, int w);
int tsii_harmonic_fill(const float* x, const float* mask, int n, int h, int w, int sweeps, float* out, void* ws, void* stream);

/* ---- K15: text blocks (csrc/blocks.hip) -- the components of a label plane grouped by distance, on the device: what the reference's demo
 * calls "the text" is a block of lettering (a speech bubble's lines), while a component of tsii_text_regions is a glyph or a piece of one.
 * Single linkage at Chebyshev distance `gap`.  All integer: the same inputs give the same bits on every run.
 * Inputs: text uint8 [h,w], REWRITTEN IN PLACE; labels int32 [h,w], read only, as tsii_text_regions leaves it (normally called with
 * min_area = 0, so that every text pixel has a label); gap 1..64.  F = {p : labels[p] != 0}; a pixel with text != 0 and labels == 0 is
 * background.  The COMPONENTS are the label classes of F.  Two components are LINKED iff some pixel p of one and some pixel q of the
 * other have max(|py - qy|, |px - qx|) <= gap; a BLOCK is a class of the transitive closure of LINKED.  Its LABEL is the smallest label
 * of its components, 1 + min(y*w + x) over its pixels, its AREA its pixel count, its BOX y0, x0 inclusive and y1, x1 exclusive over its
 * pixels, its MEMBERS the number of its components.  A block is KEPT iff area >= min_area (min_area <= 1 keeps everything).
 *   block_labels[p], int32 [h,w] (never the plane `labels` itself) = the label of p's block if that block is kept, else 0
 *   text[p]                  = block_labels[p] != 0 ? 1 : 0
 *   n_blocks, int32 [2]      = {blocks found, blocks kept}
 *   table, int32 [max_regions, 6]: row r = {label, area, y0, x0, y1, x1} of the r-th kept block in ascending label order.  Only the first
 *     min(kept, max_regions) rows are written, the rows behind them are not touched; n_blocks[1] is the true count.
 *   members, int32 [max_regions]: members[r] = MEMBERS of the block of table row r; the same rows are written, the others are not touched.
 *     max_regions == 0 with table == NULL and members == NULL is allowed.
 *   core_count: NULL (tile and halo are ignored), or int32 [ty*tx] on the K8 tile geometry: cleared by the call, then the number of KEPT
 *     text pixels in each tile core (integer atomics: independent of block order).
 * The outputs follow tsii_text_regions: tsii_region_hulls, tsii_flat_regions and a window planner run behind this call unchanged, on
 * (block_labels, table, n_blocks), and then work per block ("the pixels whose label is table[r][0]").
 * How: F, one bit per pixel, gets a square of `gap` cells a side around every pixel ((gap-1)/2 cells towards larger y and x, the rest the other way; clipped
 * to the page): two such squares overlap or touch, corners included, iff their pixels are at most `gap` apart, so the 8-connected components
 * of the dilated plane -- labelled by tsii_text_regions itself, inside this call -- are the blocks.
 * No allocation, no host synchronisation, everything on the caller's stream; no grid-wide barrier and no waiting on another block.
 * ws: tsii_text_blocks_ws_bytes(h, w, max_regions, gap) bytes (0: arguments refused), 8-BYTE aligned; it depends on the size arguments
 * only, needs nothing cleared beforehand and holds nothing a later call depends on (about 33 bytes per pixel: the bit plane, the dilated
 * plane, its labels and the labelling's own workspace, which holds the blocks' statistics once the labelling is over).
 * Refused (non-zero return, tsii_last_error, nothing written): h or w < 1; h*w > 2^31 - 2; gap outside 1..64; max_regions < 0 (or > 0
 * without table and members); a NULL among text, labels, block_labels, n_blocks, ws; block_labels == labels; a bad tile geometry while
 * core_count != NULL.  Labels that tsii_text_regions did not write give wrong blocks, never an access outside the buffers. */
size_t tsii_text_blocks_ws_bytes(int h, int w, int max_regions, int gap);
int tsii_text_blocks(uint8_t* text, const int* labels, int h, int w, int gap, int min_area, int max_regions,
                     int tile, int halo, int* core_count, int* block_labels, int* table, int* members,
                     int* n_blocks, void* ws, void* stream);

/* ---- K16: smooth regions (csrc/smooth.hip) -- the middle route between K13 and an inpainting net: a text region whose surrounding RING of
 * page pixels is LOCALLY SMOOTH (a gradient, a soft shadow, a sky: no hard edge crosses it) is filled with the harmonic continuation of
 * its surroundings at page level and leaves the text plane; only what is left goes to a net.  Two entry points on either side of
 * tsii_harmonic_fill (K14), which the caller runs unchanged between them:
 *     tsii_smooth_regions_classify(..., smooth, x, valid, ws, stream);
 *     tsii_harmonic_fill(x, valid, 1, h, w, sweeps, filled, ws', stream);
 *     tsii_smooth_regions_apply(..., smooth, filled, ..., painted, mask, stream);
 * The decision is all integer: exact, the same bits on every run.
 * Inputs as K13 takes them: page uint8 [h,w,3]; text uint8 [h,w] (non-zero = text; classify reads it, apply REWRITES IT IN PLACE); labels
 * int32 [h,w], table int32 [max_regions,6] and n_regions int32 [2] ON THE DEVICE exactly as tsii_text_regions or tsii_text_blocks left
 * them; ring 1..8; tol 0..255.  Only the label column of the table is read.  R = min(n_regions[1], max_regions); for r < R:
 *   C_r      the pixels whose label is table[r][0] AND whose text byte is non-zero on entry.  A region tsii_flat_regions has painted (its
 *            text bytes cleared, its labels left) has an empty C_r: the stage composes behind K13 with the same labels and table
 *   Ring_r   K13's ring: the page pixels q with text[q] == 0 on entry for which some p in C_r has max(|qy - py|, |qx - px|) <= ring.  A
 *            pixel may lie in several rings; text pixels lie in none; the page edge clips the ring.  n_r = |Ring_r|
 *   d_c(q)   for a pixel q with text[q] == 0: the largest |page[q][c] - page[q'][c]| over the 4-neighbours q' of q that are on the page
 *            and have text[q'] == 0; 0 without one.  It depends on the pixel only, not on the region
 *   step_r[c] = max of d_c(q) over Ring_r (0 where n_r == 0)
 *   smooth_r iff n_r >= 1 and step_r[c] <= tol for all three channels.  A hard edge that crosses the region crosses its ring; a gradient
 *            of slope <= tol per pixel does not trip it; a ring that K13 calls flat at `tol` is smooth at `tol`
 * Outputs of classify:
 *   smooth, int32 [max_regions,5]: row r < R = {smooth_r, step_r[0], step_r[1], step_r[2], n_r}; the rows behind R are not touched
 *   x, fp32 [h,w,3] = (float)page byte / 255.0f (the IEEE quotient); valid, fp32 [h,w] = 1.0 where text == 0, else 0.0: the operands of
 *            tsii_harmonic_fill for n = 1.  The solver's holes are ALL the text on entry: the ink of a neighbouring region that is not
 *            smooth is never valid context
 *   page, text, labels, table and n_regions are read only.
 * apply (smooth: as classify left it; filled fp32 [h,w,3]: the solver's output, read on the pixels of C_r of smooth rows ONLY -- it may hold
 * anything elsewhere):
 *   painted, uint8 [h,w,3] (not the page itself): floor(clamp(filled, 0, 1) * 255 + 0.5) -- the product and the sum each rounded to fp32 --
 *            on C_r where smooth_r holds, the page byte everywhere else
 *   text[p]  = 0 on the smooth regions, 1 where it was non-zero otherwise, else 0.  Regions beyond the table are never smooth and stay text
 *   mask, uint8 [h,w] or NULL: 255 where text was non-zero ON ENTRY, else 0
 *   core_count: NULL (tile and halo are ignored), or int32 [ty*tx] on the K8 tile geometry: cleared by the call, then the text pixels of
 *            the FINAL plane in each tile core (integer atomics: independent of block order)
 *   labels, table, n_regions, smooth and filled are read only.
 * No allocation, no host synchronisation, everything on the caller's stream; no grid-wide barrier and no waiting on another block.
 * ws (classify): tsii_smooth_regions_ws_bytes(h, w, max_regions) bytes (0: geometry refused), 4-byte aligned; it depends on (h, w,
 * max_regions) only, needs nothing cleared beforehand and holds nothing a later call depends on.  x and valid take 16-byte stores where
 * they (and page and text, for 4-byte loads) are aligned for them, scalar ones otherwise.
 * Refused (non-zero return, tsii_last_error, nothing written): h or w < 1; h*w*3 > 2^31; max_regions < 1; ring outside 1..8 or tol outside
 * 0..255 (classify); a NULL among page, text, labels, table, n_regions, smooth and x, valid, ws (classify) or filled, painted (apply);
 * painted == page; a bad tile geometry while core_count != NULL.  The count read from n_regions is clamped to max_regions and every table
 * row is found by a search below it: a table that does not belong to the labels gives wrong bytes, never an access outside the buffers. */
size_t tsii_smooth_regions_ws_bytes(int h, int w, int max_regions);
int tsii_smooth_regions_classify(const uint8_t* page, const uint8_t* text, const int* labels, int h, int w, const int* table,
                                 const int* n_regions, int max_regions, int ring, int tol, int* smooth, float* x, float* valid, void* ws,
                                 void* stream);
int tsii_smooth_regions_apply(const uint8_t* page, uint8_t* text, const int* labels, int h, int w, const int* table, const int* n_regions,
                              int max_regions, const int* smooth, const float* filled, int tile, int halo, int* core_count,
                              uint8_t* painted, uint8_t* mask, void* stream);

/* ---- K17: tone regions (csrc/tone.hip) -- the third net-free route, behind K13 and K16: a text region whose surrounding RING of page
 * pixels is a PERIODIC PATTERN (screentone, stripes, a dot lattice) is filled by copying, for each of its pixels, the nearest non-text
 * pixel a whole number of periods away, and leaves the text plane.  One integer shift per region, measured on the ring.  All in 32-bit
 * integers: exact, the same bits on every run.
 * Inputs as K16 takes them: page uint8 [h,w,3]; text uint8 [h,w] (non-zero = text; REWRITTEN IN PLACE); labels int32 [h,w], table int32
 * [max_regions,6] and n_regions int32 [2] ON THE DEVICE exactly as tsii_text_regions or tsii_text_blocks left them; ring 1..16; period
 * 2..16; tol 0..255.  Only the label column of the table is read.  R = min(n_regions[1], max_regions); for r < R:
 *   C_r      K16's: the pixels whose label is table[r][0] AND whose text byte is non-zero on entry (empty for a region K13 or K16 took)
 *   Ring_r   K13's ring of width `ring`: the pixels q with text[q] == 0 on entry within `ring` (Chebyshev) of a pixel of C_r.  n_r = |Ring_r|
 *   S        the shifts (dy, dx) with 0 <= dy <= period, |dx| <= period and (dy > 0 or dx > 0): one of every pair s, -s
 *   Pairs_r(s) the q in Ring_r for which q + s is on the page and has text == 0 on entry (q + s need not lie in the ring)
 *   cnt_r(s) = |Pairs_r(s)|;  err_r(s) = the largest |page[q][c] - page[q + s][c]| over the pairs and the three channels, 0 without a pair
 *   s is SUPPORTED iff 2 cnt_r(s) >= n_r
 *   step_r   = max(err_r((0,1)), err_r((1,0))).  The region is TEXTURED iff step_r > tol: a flat or gently graded ring is no pattern; it
 *            belongs to K13, K16 or a net and is never streak-filled here
 *   s_r      among the CANDIDATES -- the s with max(|dy|, |dx|) >= 2 that are SUPPORTED with err_r(s) <= tol, and none at all where
 *            n_r == 0 -- the one with the smallest key (err, dy*dy + dx*dx, dy, dx): the best match, then the shortest, then a fixed order.
 *            The unit shifts are measured for step_r and never chosen
 *   src(p)   for p in C_r: the first pixel of p + s_r, p - s_r, p + 2 s_r, p - 2 s_r, ... (k = 1..256) that is on the page with
 *            text == 0 on entry; none within 256 steps each way: p has no source
 *   tone_r   iff n_r >= 1, TEXTURED, a candidate exists and every pixel of C_r has a source.  Regions beyond the table are never tone
 * Outputs:
 *   painted, uint8 [h,w,3] (not the page itself): page[src(p)] on C_r where tone_r holds, the page byte everywhere else
 *   text[p]  = 0 on the tone regions, 1 where it was non-zero otherwise, else 0
 *   mask, uint8 [h,w] or NULL: 255 where text was non-zero ON ENTRY, else 0
 *   core_count: NULL (tile and halo are ignored), or int32 [ty*tx] on the K8 tile geometry: cleared by the call, then the text pixels of
 *            the FINAL plane in each tile core
 *   tone, int32 [max_regions,6]: row r < R = {tone_r, dy, dx, err_r(s_r), n_r, step_r}; dy = dx = err = 0 without a candidate; a row with a
 *            shift, step_r > tol and tone_r = 0 is a region with a pixel without a source; the rows behind R are not touched
 *   page, labels, table and n_regions are read only.
 * No allocation, no host synchronisation, everything on the caller's stream; no grid-wide barrier and no waiting on another block; atomicAdd
 * and atomicMax on 32-bit integers only.
 * ws: tsii_tone_regions_ws_bytes(h, w, max_regions, period) bytes (0: refused), 4-byte aligned; it depends on those four only, needs
 * nothing cleared beforehand and holds nothing a later call depends on.
 * Refused (non-zero return, tsii_last_error, nothing written): h or w < 1; h*w*3 > 2^31; max_regions < 1 (or max_regions * (period + 1) *
 * (2 period + 1) >= 2^30); ring outside 1..16, period outside 2..16, tol outside 0..255; a NULL among page, text, labels, table, n_regions,
 * painted, tone, ws; painted == page; a bad tile geometry while core_count != NULL.  The count read from n_regions is clamped to
 * max_regions and every table row is found by a search below it; the boxes of the table are not read: a table that does not belong to the
 * labels gives wrong bytes, never an access outside the buffers. */
size_t tsii_tone_regions_ws_bytes(int h, int w, int max_regions, int period);
int tsii_tone_regions(const uint8_t* page, uint8_t* text, const int* labels, int h, int w, const int* table, const int* n_regions,
                      int max_regions, int ring, int period, int tol, int tile, int halo, int* core_count,
                      uint8_t* painted, uint8_t* mask, int* tone, void* ws, void* stream);

/* ---- K18: page scores (csrc/score.hip) -- what TextEraser did to a page, measured against the same page cleaned by hand: the text mask of
 * a (raw, clean) pair as the reference's training data derives it (Dataloader.py:213-222), and the eraser's errors over the page, over
 * what it filled, over what it left, and per region.  All in integers: exact, the same bits on every run.
 *
 * tsii_pair_text_mask: raw, clean uint8 [h,w,3]; truth uint8 [h,w] (none of the two pages); thr 0..255; k 1..31, even values included.
 *   L(p)   = (19595 R + 38470 G + 7471 B + 32768) >> 16: Pillow's convert("L")
 *   t(p)   = |L_raw(p) - L_clean(p)| > thr
 *   truth(y,x) = 255 iff t(y + oy, x + ox) holds for some oy, ox in [-(k/2), k - 1 - (k/2)] (integer division) with (y + oy, x + ox) on
 *            the page, else 0: cv2.dilate with a k x k kernel of ones, its default anchor and a border that never sets a pixel.  k = 10
 *            is the reference's: offsets -5..+4.
 *   One launch; the thresholded plane lives in LDS only.
 *
 * tsii_page_scores: out (the eraser's page), clean (the hand-cleaned page) uint8 [h,w,3]; mask (the eraser's, non-zero = text), truth
 * uint8 [h,w]; labels int32 [h,w] or NULL; table int32 [n_rows,6] ON THE DEVICE, of which only the label column is read and which ascends
 * in it (as every tsii_*_regions kernel assumes); n_rows >= 0, a HOST count.  With d_c(p) = |out[p][c] - clean[p][c]|:
 *   a(p) = sum_c d_c,  s(p) = sum_c d_c^2,  m(p) = max_c d_c
 *   page, int64 [12] = { tp, fp, fn, tn of (mask != 0) against (truth != 0);
 *                        pixels, sum a, sum s, max m over the pixels with mask != 0 (the FILL);
 *                        the same four over the pixels with mask == 0 (the LEFTOVER: the eraser returns the page there, so this is the
 *                        ink the mask missed) }.  A maximum over no pixel is 0.
 *   rows, int64 [n_rows,4]: row r = { pixels, sum a, sum s, max m } over the pixels whose label is table[r][0], whatever their mask byte.
 *            A label that is 0 or not in the table counts in no row; a row whose label does not occur is all zero.  With labels == NULL or
 *            n_rows == 0 only `page` is written, and table and rows may be NULL.
 *   The call clears what it accumulates into: a second call on the same buffers gives the same bytes.  All inputs are read only.
 * The largest sum, 3 * 255^2 * (2^31 - 2), fits int64.  No allocation, no host synchronisation, everything on the caller's stream; no
 * grid-wide barrier and no waiting on another block; 64-bit atomicAdd and 32-bit atomicMax on `rows` only.
 * ws: tsii_page_scores_ws_bytes(h, w, max_rows) bytes (0: refused), 4-byte aligned; any n_rows <= max_rows may use it; it needs nothing
 * cleared beforehand and holds nothing a later call depends on (12 words per block of 64 x 32 pixels).  page and rows: 8-byte aligned.
 * Refused (non-zero return, tsii_last_error, nothing written): h or w < 1; h*w > 2^31 - 2; thr, k or n_rows (max_rows) out of range; a NULL
 * among raw, clean, truth / out, clean, mask, truth, page, ws (table, rows: only with labels and n_rows > 0); truth == raw or clean;
 * ws_bytes below tsii_page_scores_ws_bytes; a misaligned ws, page or rows.  A row found by the search lies below n_rows and nothing is
 * indexed by a label: a table that does not belong to the labels gives wrong numbers, never an access outside the buffers. */
int tsii_pair_text_mask(const uint8_t* raw, const uint8_t* clean, int h, int w, int thr, int k, uint8_t* truth, void* stream);
size_t tsii_page_scores_ws_bytes(int h, int w, int max_rows);
int tsii_page_scores(const uint8_t* out, const uint8_t* clean, const uint8_t* mask, const uint8_t* truth, const int* labels,
                     const int* table, int n_rows, int h, int w, int64_t* page, int64_t* rows, void* ws, size_t ws_bytes, void* stream);

/* ---- K19: seeded regions (csrc/seeds.hip) -- the second half of a hysteresis threshold: the plane was cut at a low probability and
 * labelled; a region (or block) stays only if at least min_seeds of its pixels are also set in a second plane, cut at a high one.  Runs
 * behind tsii_text_regions or tsii_text_blocks, in front of everything that works on their outputs.  All integer: the same inputs give
 * the same bits on every run.
 * Inputs as those calls leave them: text uint8 [h,w] (non-zero = text) and labels int32 [h,w], BOTH REWRITTEN IN PLACE; table int32
 * [max_regions,6] = {label, area, y0, x0, y1, x1} ascending in label, REWRITTEN IN PLACE; n_regions int32 [2] = {found, kept} ON THE
 * DEVICE (the call does not read it on the host).  seed: uint8 [h,w], read only, never the text plane; a pixel is a SEED where its byte is
 * non-zero.  n = min(max(n_regions[1], 0), max_regions) table rows are in use.
 *   s[r], r < n              = the number of pixels p with labels[p] == table[r][0] and seed[p] != 0.  A seed whose label is 0 or in no row
 *                              counts nowhere.
 *   row r is KEPT iff s[r] >= min_seeds; the others are DROPPED.  Kept regions beyond the table (kept > max_regions) have no row, are not
 *   judged and stay, as they get no hull and no route.  With k = the number of kept rows:
 *   labels[p], text[p]       = 0 for the pixels of dropped rows; every other byte of both planes is unchanged (text keeps its non-zero
 *                              values, whatever they are).
 *   table                    : the kept rows move to rows 0 .. k - 1 in their order.  The rows from n on are not touched.  Rows k .. n - 1
 *                              keep what they held on entry (the rows that stood there) where the table held every region
 *                              (n_regions[1] <= max_regions on entry).  Where it was cut, the count that is left may reach behind row
 *                              k - 1, so these rows become EMPTY rows {INT_MAX, 0, 0, 0, 0, 0}: the label column still ascends, no pixel
 *                              has that label, and every tsii_* call behind this one finds nothing for such a row (no hull, no ring,
 *                              no route).  An empty row on entry is never judged and stays: a caller tells the rows of regions from the
 *                              empty ones by count, min(n_regions[1] + dropped[0], max_regions) - dropped[0] summed over its calls.
 *   members, NULL or int32 [max_regions] (the column of tsii_text_blocks): compacted with the table, the same rule; 0 in an empty row.
 *   seeds, int32 [max_regions]: seeds[j] = s of the row that is now row j, j < k; the entries from k on are not touched.
 *   n_regions[1]             = its value on entry - (n - k); n_regions[0] is unchanged.
 *   dropped, int32 [2]       = {n - k, the summed area column of the dropped rows}.
 *   core_count: NULL (tile and halo are ignored), or int32 [ty*tx] on the K8 tile geometry: cleared by the call, then the number of
 *     pixels with text != 0 of the REDUCED plane in each tile core (integer atomics: independent of block order).
 * A second call on the same buffers with the same seed plane drops nothing and changes nothing but dropped = {0, 0}.
 * No allocation, no host synchronisation, everything on the caller's stream; no grid-wide barrier and no waiting on another block.
 * ws: tsii_region_seeds_ws_bytes(h, w, max_regions) bytes (0: geometry refused), 4-byte aligned; it needs nothing cleared beforehand and
 * holds nothing a later call depends on (three words per table row: the counts, the labels on entry and the verdicts).
 * Refused (non-zero return, tsii_last_error, nothing written): min_seeds < 1; h or w < 1; h*w > 2^31 - 2; max_regions < 1; a NULL among
 * text, labels, seed, table, n_regions, seeds, dropped, ws; seed == text; a bad tile geometry while core_count != NULL.
 * The count read from n_regions is clamped to max_regions, a row found by the binary search over the label column lies below it and
 * nothing is indexed by a label: a table that does not belong to the labels gives wrong numbers, never an access outside the buffers. */
size_t tsii_region_seeds_ws_bytes(int h, int w, int max_regions);
int tsii_region_seeds(uint8_t* text, int* labels, const uint8_t* seed, int h, int w, int* table, int* n_regions, int max_regions,
                      int min_seeds, int tile, int halo, int* core_count, int* seeds, int* members, int* dropped, void* ws, void* stream);

/* ---- K20: seamless fill (csrc/blend.hip) -- the output of an inpainting filler taken into the image in the gradient domain ("seamless",
 * Poisson composition): inside a hole the result keeps the filler's gradients and takes its level from the valid pixels around the hole.
 * That is the filler's output plus the harmonic continuation of its own error on the valid pixels (the membrane correction), and the
 * harmonic continuation is tsii_harmonic_fill (K14).  Per image; the 3 channels share one validity plane.
 * Inputs: x fp32 NHWC [n,h,w,3], the image as the filler saw it (what tsii_page_tiles_fill / tsii_page_windows_fill write); out fp32 NHWC
 * [n,h,w,3], the filler's output; mask fp32 [n,h,w], a pixel is VALID iff mask != 0 (K14's plane); sweeps 0..16.  Output: dst fp32 NHWC
 * [n,h,w,3]; it may be out itself (in place), never x.
 *   1. o = min(max(out, 0), 1) at every pixel: the clamp of tsii_compose_page_u8, so that what is corrected is what the page would show.
 *   2. d = x - o on the VALID pixels (one fp32 subtraction).  d under a hole is never used.
 *   3. c = tsii_harmonic_fill(d, mask, sweeps): K14's semantics exactly as stated above (levels, apex, coarse to fine, the fixed order of
 *      every mean).  An image without a valid pixel gets c = 0.
 *   4. dst = out, bit for bit and not clamped, on the VALID pixels; dst = o + c (one fp32 addition, not clamped: compose clamps) on the
 *      hole pixels.
 *   5. The value of x at a hole pixel is NEVER USED (it may be NaN); out is read everywhere.
 * The same bits on every run; an image of a batch equals the same image run alone.  No atomics, no allocation, no host synchronisation,
 * everything on the caller's stream.
 * ws: tsii_seamless_fill_ws_bytes(n, h, w) bytes (0: geometry refused; d, c and K14's own workspace, about 2.4 of x), 4-byte aligned (16
 * for the vector paths); needs nothing cleared beforehand and holds nothing a later call depends on.
 * Refused (non-zero return, tsii_last_error, nothing launched): n, h or w < 1; n*h*w*3 > 2^31; sweeps outside 0..16; a NULL among x, out,
 * mask, dst, ws; dst == x. */
size_t tsii_seamless_fill_ws_bytes(int n, int h, int w);
int tsii_seamless_fill(const float* x, const float* out, const float* mask, int n, int h, int w, int sweeps, float* dst, void* ws,
                       void* stream);

/* ---- K21: patch fill (csrc/patch.hip) -- exemplar-based fill: every hole pixel becomes a COPY of a page pixel whose (2r+1)^2 neighbourhood
 * matches the hole pixel's own, found by a PatchMatch-style search of a nearest-neighbour field, coarse to fine.  Per image; every operation
 * is an integer operation, so every run gives the same bits and an image of a batch equals the same image run alone.
 * Inputs: page uint8 [n,h,w,3]; hole uint8 [n,h,w], a pixel is a HOLE iff hole != 0; init uint8 [n,h,w,3], a first guess of the hole
 * pixels (a harmonic fill, say; any bytes are legal); radius r 1..4; levels 1..6; iters 1..8; seed, any 32 bits.  Outputs: out uint8
 * [n,h,w,3] (it may be init, never page); nnf int32 [n,h,w,2]; stats int32 [n,3].
 *   Levels.  h_0 = h, w_0 = w, h_{l+1} = (h_l + 1) / 2, w_{l+1} = (w_l + 1) / 2.  L = min(levels, the number of l with min(h_l, w_l) >=
 *     2r+1), at least 1: levels 0 .. L-1 are used.
 *   Work image.  W_0[p] = init[p] where p is a hole, page[p] elsewhere: the value of page under a hole is NEVER USED, init is used under
 *     the holes only.  H_0[p] = (hole[p] != 0).  The children of a pixel (Y, X) of level l+1 are the pixels (2Y + a, 2X + b), a, b in {0, 1},
 *     that lie on level l; cnt is their number (1, 2 or 4).  W_{l+1}[Y,X][c] = (sum of W_l[child][c] + cnt / 2) / cnt (integer division),
 *     holes and valid pixels alike; H_{l+1}[Y,X] = some child is a hole.
 *   Admissible.  A pixel s of level l is an admissible SOURCE iff all (2r+1)^2 pixels s + d, |d|_inf <= r, lie on the level and none of them
 *     is a hole.
 *   Field.  NNF_l[p], for the hole pixels p of level l, is an admissible source or "none"; p is SOURCED iff it is not none.  At level L-1
 *     the field starts as none everywhere.  At a level l < L-1 it starts from the final field of level l+1: with P = (y >> 1, x >> 1) the
 *     parent of p = (y, x), none if P is not sourced, else c = (2 sy + (y & 1), 2 sx + (x & 1)) for (sy, sx) = NNF_{l+1}[P] if c is
 *     admissible at level l, else none.
 *   Cost.  T[q] = W_l[NNF_l[q]] if q is a sourced hole pixel, W_l[q] otherwise.  cost(p, s) = the sum over the d with |d|_inf <= r and p + d
 *     on the level, and over the 3 channels c, of |T[p + d][c] - W_l[s + d][c]|.
 *   Iteration t = 1 .. iters of level l (Jacobi: the field F read -- in T, as the current source and by propagation -- is the one after
 *     iteration t-1, all new values go to a second field).  For every hole pixel p = (y, x), the candidates are
 *       a. F[p], if p is sourced;
 *       b. propagation, jump-flooded: for k in {1, 2, 4, 8} and e in {(0,1), (0,-1), (1,0), (-1,0)}: if q = p + k e lies on the level and is
 *          a sourced hole pixel, F[q] - k e;
 *       c. random search around centre = F[p] if p is sourced, else p: for j = 0, 1, ... with R_j = max(h_l, w_l) >> j while R_j >= 1, the
 *          pixel centre + (oy, ox), m = 2 R_j + 1, u = hash(seed, l, t, y, x, j),
 *          oy = (int)(((uint64)(u & 0xffff) * m) >> 16) - R_j,  ox = (int)(((uint64)(u >> 16) * m) >> 16) - R_j  (both in [-R_j, R_j]).
 *     Candidates that are not admissible (off the level included) are dropped.  The new F[p] is the candidate with the smallest
 *     (cost, sy, sx), lexicographically; none if no candidate is left.
 *   Hash (all uint32, wrapping).  mix(v): v ^= v >> 16; v *= 0x7feb352d; v ^= v >> 15; v *= 0x846ca68b; v ^= v >> 16.
 *     hash = mix(mix(mix(mix(seed + 0x9e3779b9 * (16 l + t)) ^ y) ^ x) ^ (0x9e3779b9 * (j + 1))).  The image index is not hashed.
 *   Result, from NNF_0 after the last iteration.  Valid pixel: out = page byte for byte, nnf = (-1, -1).  Sourced hole pixel: nnf = (sy,
 *     sx), out = page[sy, sx], the bytes of a page pixel that is not a hole.  Hole pixel without a source (no admissible source on the
 *     level, or none was met): out = init, nnf = (-1, -1).  stats[i] = (holes, sourced, holes - sourced) of image i.
 * Integer sums only (the counts of stats are accumulated with integer atomics, whose order changes nothing); no allocation, no host
 * synchronisation, everything on the caller's stream.
 * ws: tsii_patch_fill_ws_bytes(n, h, w, radius, levels) bytes (0: refused; per used level a packed RGBX word, two field words and two flag
 * bytes per pixel: about 17 bytes per page pixel), 4-byte aligned (16 for the vector paths); needs nothing cleared beforehand and holds
 * nothing a later call depends on.
 * Refused (non-zero return, tsii_last_error, nothing launched): n, h or w < 1; n*h*w*3 >= 2^31; radius outside 1..4; levels outside 1..6;
 * iters outside 1..8; a NULL among page, hole, init, out, nnf, stats, ws; out == page. */
size_t tsii_patch_fill_ws_bytes(int n, int h, int w, int radius, int levels);
int tsii_patch_fill(const uint8_t* page, const uint8_t* hole, const uint8_t* init, int n, int h, int w, int radius, int levels, int iters,
                    uint32_t seed, uint8_t* out, int32_t* nnf, int32_t* stats, void* ws, void* stream);

/* ---- K22: region geometry (csrc/hull.hip, behind K12's kernels) -- the polygon of every region's convex hull and its minimum-area
 * enclosing rectangle (cv2.convexHull and cv2.minAreaRect of the reference's demo, per table row), on the device.  All integer: one
 * defined answer, the same bits on every run.
 * Inputs exactly as tsii_text_regions or tsii_text_blocks leave them: labels int32 [h,w], table int32 [max_regions,6], n_regions int32 [2]
 * ON THE DEVICE (the call does not read it on the host); all three are read only.  R = min(n_regions[1], max_regions) table rows are in
 * use; for r < R, P_r is the set of pixels whose label is table[r][0], taken as integer points (y, x).
 *   Vertices.  V_r is the set of vertices of the closed convex hull of P_r, STRICT: no point of V_r lies on a segment between two others
 *     (one pixel: one vertex; collinear pixels: the two ends).  Order: V[0] is the vertex with the smallest y and among those the smallest
 *     x; the list then runs along the top row to the right and on around the hull, clockwise on a screen whose y points down.
 *     n_vertices, int32 [max_regions]: n_vertices[r] = |V_r|, the TRUE count, also above max_vertices.
 *     vertices, int32 [max_regions, max_vertices, 2]: vertices[r][k] = (y, x) of V[k] for k < min(|V_r|, max_vertices).  The slots behind
 *     that and the rows behind R are not touched.
 *   Rectangle.  For every hull edge k, from V[k] to V[(k + 1) mod n], with the direction d = (dy, dx) = V[k+1] - V[k] and the normal
 *     n = (-dx, dy), both written (y part, x part): the dot products are  d . V = dy * y + dx * x  and  n . V = -dx * y + dy * x.  lo_d,
 *     hi_d, lo_n, hi_n are the extreme dot products over ALL of V_r (never the truncated list), D = dy^2 + dx^2.  The rectangle of edge k
 *     has the area (hi_d - lo_d) (hi_n - lo_n) / D, a rational.  The winning edge has the smallest area, compared EXACTLY by
 *     cross-multiplication in 128 bits (no floating point); ties go to the smaller k.
 *     rect, int64 [max_regions, 8]: rect[r] = {k, dy, dx, lo_d, hi_d, lo_n, hi_n, D} of the winning edge; rows behind R are not touched.
 *     Its corners are the points (a d + b n) / D for a in {lo_d, hi_d}, b in {lo_n, hi_n}.
 *     One vertex (y, x): k = -1, d = (0, 1), D = 1, lo_d = hi_d = x and, n being (-1, 0), lo_n = hi_n = n . V = -y: the SIGNED dot product
 *     of the convention above, so that the corner formula gives (y, x) back.  Two vertices: edge 0, lo_n = hi_n.
 * How: steps 1 to 4 of K12 (row extents, strict vertex flags of both envelopes); then a wave per region orders the flagged ends into the
 * polygon with a scan and evaluates a lane per edge.  No allocation, no host synchronisation, everything on the caller's stream; no
 * grid-wide barrier and no waiting on another block; integer atomics only (the row extents).
 * ws: ws_bytes >= tsii_region_geometry_ws_bytes(h, w, max_regions, max_vertices) bytes (0: arguments refused), 4-byte aligned; it depends on
 * the size arguments only, needs nothing cleared beforehand and holds nothing a later call depends on.  rect is 8-byte aligned.
 * Refused (non-zero return, tsii_last_error, nothing written): h or w < 1 or > 32767 (every dot product then fits int32 and every area
 * product int64); h*w > 2^31 - 2; max_regions < 1; max_vertices outside 3..1024; a NULL pointer; a workspace that is too small; a
 * misaligned ws or rect.
 * Every box or count read from table or n_regions is clamped to the page and to max_regions before use: a table that does not belong to
 * the labels gives wrong numbers (a row without pixels: n_vertices 0, rect {-1, 0, ...}), never an access outside the buffers. */
size_t tsii_region_geometry_ws_bytes(int h, int w, int max_regions, int max_vertices);
int tsii_region_geometry(const int* labels, const int* table, const int* n_regions, int max_regions, int h, int w, int max_vertices,
                         int* n_vertices, int* vertices, int64_t* rect, void* ws, size_t ws_bytes, void* stream);

/* ---- K23: region crops (csrc/crops.hip) -- every table row's minimum-area rectangle cut out of the raw page on the device, deskewed, scaled
 * into a fixed slot and batched: the picture an OCR or typesetting step starts from.  All integer: one defined answer, the same bits on
 * every run.
 * page: uint8 [h,w,3], read only.  rect int64 [max_regions,8] and n_regions int32 [2] exactly as tsii_region_geometry leaves them, ON THE
 * DEVICE (the call does not read them on the host), read only.  R = min(n_regions[1], max_regions, max_crops) rows are served; info rows
 * and slots behind R are not touched.  info: int32 [max_crops,10]; crops: uint8 [max_crops,ch,cw,3].
 *   Padded rectangle.  rect[r] = (k, dy, dx, lo_d, hi_d, lo_n, hi_n, D).  D <= 0 (a row without pixels): info[r] = 0 and the whole slot is
 *     `fill`.  Otherwise pad = |dy| + |dx| and, in DOUBLED dot-product units, A0 = 2 lo_d - pad, A1 = 2 hi_d + pad, B0 = 2 lo_n - pad,
 *     B1 = 2 hi_n + pad: the rectangle grown to cover the pixels' unit squares, never degenerate.
 *   Frame.  f in 0..3 gives the crop's x axis u, its y axis v (u turned clockwise on the screen) and the ranges [U0, U1] along u and
 *     [V0, V1] along v; d = (dy, dx) and n = (-dx, dy) are written (y part, x part) as in K22:
 *       f = 0: u =  d, v = -n, [A0, A1], [-B1, -B0]        f = 1: u = -n, v = -d, [-B1, -B0], [-A1, -A0]
 *       f = 2: u = -d, v =  n, [-A1, -A0], [B0, B1]        f = 3: u =  n, v =  d, [B0, B1], [A0, A1]
 *     The x parts of u are dx, -dy, -dx, dy.  Eu = U1 - U0, Ev = V1 - V0.
 *     orient = 0 ("upright"): the smallest f whose u has the largest x part -- deskewed by at most 45 degrees, never laid on its side.
 *     orient = 1 ("long"): only the frames with Eu >= Ev (Eu == Ev: all four); the largest x part of u, ties to the larger y part of u,
 *     then to the smaller f -- a column is turned so that reading downwards becomes reading rightwards.
 *   Fit.  If Eu * ch >= Ev * cw: uw = cw, uh = clamp((2 cw Ev + Eu) / (2 Eu), 1, ch); otherwise uh = ch,
 *     uw = clamp((2 ch Eu + Ev) / (2 Ev), 1, cw).  Small blocks are magnified, large ones reduced.
 *   Supersampling.  s is the smallest number in 1..max_ss with (s uw)^2 D >= (Eu / 2)^2 and (s uh)^2 D >= (Ev / 2)^2, or max_ss where none
 *     has both (Eu / 2 < 2^32: both sides fit unsigned 64 bits): about one source pixel per sub-sample at the most.
 *   Fixed point.  All divisions are floor divisions (towards minus infinity); everything fits int64.  In units of 2^-12 pixel, per
 *     component: O = floor((U0 u + V0 v) * 2048 / D), SU = floor(Eu u * 2048 / D), SV = floor(Ev v * 2048 / D).
 *     info[r] = (uh, uw, f, s, O_y, O_x, SU_y, SU_x, SV_y, SV_x).
 *   Samples.  Sub-sample (l, m), l < uh s, m < uw s: P = O + floor(SU (2m + 1) / (2 uw s)) + floor(SV (2l + 1) / (2 uh s)) per component;
 *     iy = P_y >> 12, fy = (P_y & 4095) >> 4, the same for x; the four neighbours (iy, iy + 1) x (ix, ix + 1), each index clamped to the
 *     page; per channel t = (256 - fy) ((256 - fx) p00 + fx p01) + fy ((256 - fx) p10 + fx p11).  Crop pixel (i, j), i < uh, j < uw, is
 *     (the sum of t over its s x s sub-samples + 32768 s^2) / (65536 s^2).  Slot pixels outside uh x uw are `fill`.
 *   Validation.  A row is served as a row without pixels (info 0, slot `fill`) unless 1 <= D <= 2^31, |dy| and |dx| <= 32767, lo <= hi and
 *     |lo|, |hi| <= 2^31 - 65536 on both axes, Eu and Ev >= 1 and O, SU and SV fit int32: every row tsii_region_geometry writes for a page
 *     of sides up to 32767 passes.  The count is clamped and every page index is clamped to the page: a foreign table gives wrong
 *     pictures, never an access outside the buffers.
 * No workspace, no allocation, no host synchronisation, no atomics, no floating point; everything on the caller's stream.
 * Refused (non-zero return, tsii_last_error, nothing written): h or w outside 1..32767; max_regions < 1; max_crops < 1; ch or cw outside
 * 1..4096; max_crops * ch * cw * 3 > 2^31 - 1; orient not 0 or 1; fill outside 0..255; max_ss outside 1..4; a NULL pointer; a misaligned
 * rect (8 bytes) or info (4 bytes). */
int tsii_region_crops(const uint8_t* page, int h, int w, const int64_t* rect, const int* n_regions, int max_regions, int max_crops, int ch,
                      int cw, int orient, int fill, int max_ss, int* info, uint8_t* crops, void* stream);

/* ---- K24: region paste (csrc/paste.hip) -- the return trip of K23: a batch of pictures, one per slot, is laid back onto the page along the
 * rectangles the info rows name, antialiased and alpha-blended, on the device: what a typesetter does with the translated lettering.  All
 * integer: one defined answer, the same bits on every run.
 * page: uint8 [h,w,3], composited IN PLACE.  info: int32 [max_rows,10] exactly as tsii_region_crops leaves it, n_rows: int32 [1], both ON
 * THE DEVICE (the call does not read them on the host), read only.  R = clamp(n_rows[0], 0, max_rows) rows are served.  slots: uint8
 * [max_rows,ch,cw,4], straight (not premultiplied) RGBA, read only; the picture of row r is the slot's top-left uh x uw pixels, the rest of
 * the slot is not read.  plan: int64 [max_rows,12], written by the call for the rows below R; the rows behind R are not touched.
 *   Coordinates.  K23's: page pixel (y, x) has its centre at (4096 y, 4096 x), in units of 2^-12 pixel; with info[r] = (uh, uw, f, s', O_y,
 *     O_x, SU_y, SU_x, SV_y, SV_x) the picture's area is O + a SU + b SV, a and b in [0, 1], and crop pixel (i, j) has its centre at
 *     a = (2j + 1) / (2 uw), b = (2i + 1) / (2 uh).  f and s' are not used.
 *   Plan, per row, in exact integers with floor divisions.  The row is DEAD -- plan[r] = 0, nothing is pasted -- if it fails the PLAN
 *     VALIDATION below or its box is empty.  With S.T = S_y T_y + S_x T_x:
 *       Gu_c = floor(SU_c uw 2^24 / (SU.SU)),  Gv_c = floor(SV_c uh 2^24 / (SV.SV))  per component c: the steps in crop pixels per 2^-12
 *         page pixel, times 2^24.  SU and SV are treated as orthogonal, which they are up to the floors of K23's O, SU and SV: the
 *         position along u is taken from the projection on SU alone.
 *       s: the smallest number in 1..max_ss with s^2 (SU.SU) >= (4096 uw)^2 and s^2 (SV.SV) >= (4096 uh)^2, or max_ss where none has
 *         both (unsigned 64-bit compares): about one crop pixel per page sub-sample at the most.
 *       Box: per axis the smallest and the largest of the corners O, O + SU, O + SU + SV, O + SV, each >> 12, the lower end less 1 and the
 *         upper end plus 1, clamped to the page: y0..y1, x0..x1 INCLUSIVE; empty if y0 > y1 or x0 > x1.
 *       plan[r] = (1, y0, x0, y1, x1, s, Gu_y, Gu_x, Gv_y, Gv_x, 0, 0).
 *   Pixels.  Page pixel (y, x) inside the box of a live row, sub-samples (l, m), l < s, m < s:
 *       Pp_y = 4096 y + ((2l + 1) 2048) / s - 2048,  Pp_x = 4096 x + ((2m + 1) 2048) / s - 2048;  dP = Pp - O;
 *       Qx = ((dP.Gu) >> 16) - 128,  Qy = ((dP.Gv) >> 16) - 128  (64-bit, arithmetic shifts): the position in 1/256 crop pixel;
 *       j0 = Qx >> 8, fx = Qx & 255, i0 = Qy >> 8, fy = Qy & 255; the four neighbours (i0, i0 + 1) x (j0, j0 + 1) with the weights
 *       w = (256 - fy | fy) (256 - fx | fx).  A neighbour outside uh x uw counts with alpha 0: transparent, not clamped to the edge, so the
 *       picture's rim is antialiased.  With (c, a) the channel and the alpha byte of a neighbour:
 *       Tc = (sum of w a c + 32768) >> 16 per channel,  Ta = (sum of w a + 32768) >> 16  (sum of w a c <= 65536 * 255 * 255 < 2^32 - 32768).
 *     With N = s^2 and the sums over the pixel's sub-samples:  out = (sum Tc + page (255 N - sum Ta) + (255 N) / 2) / (255 N)  per channel,
 *     32-bit unsigned; it never exceeds 255.  A pixel whose sum Ta is 0 is not written.  Pixels outside the box are not touched, also where
 *     the rim of a much reduced picture would reach them.
 *   Order.  The rows are composited in ascending r, `page` above being what the rows before left: a later row lies over an earlier one.
 *     Every page pixel is stored at most once, by the one thread that owns it: no atomics, no race.
 *   PLAN VALIDATION.  A row is dead unless 1 <= uh <= ch and 1 <= uw <= cw; |O_c| <= 2^29 and |SU_c|, |SV_c| <= 2^28 - 1; SU.SU >= 1 and
 *     SV.SV >= 1; |SU_c| uw < 128 (SU.SU) and |SV_c| uh < 128 (SV.SV).  Then SU.SU < 2^57, every |G_c| < 2^31 and, a page coordinate being
 *     below 2^27 + 2^11, every |dP_c| < 2^30: dP.G stays below 2^62 for every pixel of the box and its two products are 32 x 32 bits.
 *     Every row tsii_region_crops writes for a page of sides up to 32767 passes (a side of its rectangle is shorter than 2^28 units and at
 *     least 4094 long, so |S_c| n / (S.S) <= 4096 / 4094).  The numerator SU_c uw 2^24 itself can leave int64 (2^28 * 2^12 * 2^24): the
 *     kernel takes the quotient by long division, the result is the exact floor.  The count is clamped, every slot index is tested against
 *     uh x uw and the box is clamped to the page: a foreign info gives wrong pictures, never an access outside the buffers.
 * No workspace beyond plan, no allocation, no host synchronisation, no atomics, no floating point; everything on the caller's stream.
 * Refused (non-zero return, tsii_last_error, nothing written): h or w outside 1..32767; ch or cw outside 1..4096; max_ss outside 1..4;
 * max_rows < 1; a NULL pointer; a misaligned plan (8 bytes), info or n_rows (4 bytes). */
int tsii_region_paste(uint8_t* page, int h, int w, const int* info, const int* n_rows, int max_rows, const uint8_t* slots, int ch, int cw,
                      int max_ss, int64_t* plan, void* stream);

/* ---- K25: region balloons (csrc/balloon.hip) -- the speech balloon around every table row's lettering: the flood fill from the row's own
 * text over the colour that surrounds it, the balloon's area and box, whether it is closed, and the largest upright rectangle inside it
 * around the block's centre, which is where a translation has room.  All integer: one defined answer, the same bits on every run.
 * page: uint8 [h,w,3], read only.  text: uint8 [h,w], read only; a non-zero byte is text of some region.  labels int32 [h,w], table int32
 * [max_regions,6] and n_regions int32 [2] as tsii_text_regions or tsii_text_blocks leave them, ON THE DEVICE (the call does not read them
 * on the host), read only.  ring 1..8, tol 0..255, ring <= reach <= 512.  R = min(n_regions[1], max_regions) rows are served; for r < R:
 *   Window.  W_r is the table row's box (y0, x0 inclusive, y1, x1 exclusive, each clamped to the page first), grown by `reach` on every
 *     side and clipped to the page.  A side of W_r above 1024 pixels: status bit 8, every other word of the row 0.
 *   Own pixels.  C_r: the pixels inside the clamped box with labels == table[r][0] and text != 0.  C_r empty: status bit 16, every other
 *     word of the row 0.
 *   Ring and colour (K13's).  Ring_r: the pixels with text == 0 within Chebyshev distance `ring` of a pixel of C_r (reach >= ring puts
 *     them inside the window).  n, lo, hi and sum per channel over the ring's page bytes; colour = (2 sum + n) / (2 n), 0 where n == 0.
 *     n == 0: status bit 1.  hi - lo > tol in any channel: status bit 2.  Either bit: there is no balloon -- status, n, the colour and the
 *     anchor are reported, every other word of the row is 0.
 *   Passable.  P_r = C_r + { p in W_r : text[p] == 0 and |page[p][c] - colour[c]| <= tol for c = 0, 1, 2 }.  The text of OTHER rows is an
 *     obstacle: a second block in the same balloon is a hole in this one's.
 *   Balloon.  B_r: the union of the 4-connected components of P_r, inside W_r, that hold a pixel of C_r.  area = |B_r|; (by0, bx0, by1,
 *     bx1) its box, y1 and x1 exclusive.  OPEN, status bit 4: B_r has a pixel on a side of W_r that is not a side of the page -- the fill
 *     ran to the end of its reach.  A balloon cut by the page's edge is closed.
 *   Anchor.  (ay, ax): the pixel of C_r with the smallest |2y - (y0 + y1 - 1)| + |2x - (x0 + x1 - 1)|, ties to the smallest y, then the
 *     smallest x.  It lies in B_r.
 *   Rectangle.  For a row y with (y, ax) in B_r, L(y) and Rr(y) are the ends of the run of B_r through (y, ax).  The candidates are all
 *     ya <= ay <= yb with (y, ax) in B_r for every y in ya..yb; width = min Rr - max L + 1 over those rows, area = (yb - ya + 1) * width.
 *     The largest area wins, ties to the smallest ya, then the smallest yb.  (ry0, rx0, ry1, rx1) = (ya, max L, yb + 1, min Rr + 1).  Every
 *     upright rectangle inside B_r that holds the anchor lies inside a candidate: this is the largest such rectangle.
 *   balloon, int32 [max_regions,16]: balloon[r] = {status, n, colour r, g, b, area, by0, bx0, by1, bx1, ay, ax, ry0, rx0, ry1, rx1}.
 *   rect, int64 [max_regions,8], K22's layout for the upright rectangle: {-1, 0, 1, rx0, rx1 - 1, -(ry1 - 1), -ry0, 1} (d = (0, 1), n =
 *     (-1, 0), signed dot products as K22 writes them for one vertex), so that tsii_region_crops takes it unchanged; all 0 where there is no
 *     rectangle, which K23 serves as a row without pixels.
 *   plane: NULL, or uint8 [h,w]: cleared by the call, then 255 on every pixel of any served B_r.
 *   The rows behind R are not touched.
 * How: one workgroup per row; bit planes of the window (a word per 32 pixels) in LDS, the passable plane in the workspace where the window
 *   is above 768 x 768; the fill sweeps until no word changes, 33 rows and at least a word per sweep.  No allocation, no host
 *   synchronisation, no floating point, no grid-wide barrier, no global atomics; everything on the caller's stream.
 * ws: tsii_region_balloons_ws_bytes(h, w, max_regions, reach) bytes (0: arguments refused), 4-byte aligned; it depends on the size
 *   arguments only, needs nothing cleared beforehand and holds nothing a later call depends on.  Its last max_regions int32 words are a
 *   debug record: the sweeps the fill of each served row took.  rect is 8-byte aligned.
 * Refused (non-zero return, tsii_last_error, nothing written): h or w outside 1..32767 (h*w <= 2^31 - 2 follows); max_regions < 1; ring
 *   outside 1..8; tol outside 0..255; reach < ring or > 512; a NULL pointer other than plane; a misaligned rect (8 bytes), balloon or ws (4 bytes).
 * Every box or count read from table or n_regions is clamped to the page and to max_regions before use: a table that does not belong to
 *   the labels gives wrong numbers, never an access outside the buffers. */
size_t tsii_region_balloons_ws_bytes(int h, int w, int max_regions, int reach);
int tsii_region_balloons(const uint8_t* page, const uint8_t* text, const int* labels, int h, int w, const int* table, const int* n_regions,
                         int max_regions, int ring, int tol, int reach, int* balloon, int64_t* rect, uint8_t* plane, void* ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TSII_HIP_H */
