/* gdrn_hip.h -- C ABI of libgdrn_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for GDR-Net's
 * per-RoI hot path (ResNet-34 backbone + geometric head + Patch-PnP + pose decode + losses, forward
 * and backward).
 *
 * This is the drop-in boundary for the path.  The reference has no native interface here: its hot
 * path is Python dispatching ATen/cuDNN ops.  Each entry point below names the
 * reference call site(s) whose ATen dispatch it replaces; paths are relative to the reference
 * checkout.  Binding stub for a reference maintainer: INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; every buffer is caller-owned device memory (the library never
 *     allocates or frees device memory and keeps no state besides per-kernel launch attributes);
 *   - every call enqueues asynchronously on `stream` (a hipStream_t passed as void*; 0 = null stream)
 *     and returns an int status: 0 ok, <0 error (GDRN_ERR_*); nothing throws across the boundary;
 *   - activations are NHWC with an explicit pixel stride (`*_cs`, in elements); `dtype` selects the
 *     storage/operand type: GDRN_DT_F32 (fp32 MFMA, parity mode), GDRN_DT_BF16 or GDRN_DT_F16 (16-bit MFMA operands,
 *     fp32 accumulate, throughput mode; which of the two: the library build).  Statistics, losses, pose and parameter gradients are fp32.
 *   - re-entrant and thread-compatible: one host thread per stream.
 */
#ifndef GDRN_HIP_H
#define GDRN_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: status / dtype enums renamed (GDRN_E_* -> GDRN_ERR_*, GDRN_F32 / GDRN_BF16 -> GDRN_DT_*; the old names stay as deprecated aliases),
 *    gdrn_conv_params.pad0_ became w_frag (values outside 0..2 are rejected), gdrn_wgrad_params.variant is honoured (GDRN_WGRAD_W128). */
/* 3: gdrn_conv_params grew halo_waves (appended; zero = the behaviour of version 2). */
/* 4: entry points added (nothing changed): gdrn_loss_scale_state + gdrn_ranger_multi_dyn / gdrn_loss_scale_update / gdrn_unscale_or_zero /
 *    gdrn_scaled_loss_weights -- the fp16 mode's dynamic loss scale decided on the device; gdrn_bn_relu_upsample2x_fwd, gdrn_upsample2x_bwd_bnsums; gdrn_block64_eval; gdrn_conv3x3s2 / gdrn_conv3x3s2_dgrad (+ gdrn_s2_params, gdrn_s2d_params).
 *    Removed: gdrn_conv3x3_wgrad_multi_w128 and gdrn_wgrad_params.variant = GDRN_WGRAD_W128 (the 128 x 64 weight-gradient tile of rounds 4-5:
 *    never faster inside the step). */
/* 5: gdrn_s2d_params grew stats / bias / act (appended; NULL / 0 = the data gradient of version 4): gdrn_conv3x3s2_dgrad also runs the forward pass of
 *    the head's ConvTranspose2d.  gdrn_conv3x3s2 / gdrn_conv3x3s2_dgrad accept maps 8 pixels wide (two images per pixel tile: an even image count). */
#define GDRN_ABI_VERSION 5
/* `dtype` arguments.  The 16-bit format is a property of the library build: libgdrn_hip.so computes GDRN_DT_BF16, libgdrn_hip_f16.so (the same
 * sources compiled with -DGDRN_HALF_F16: v_mfma_f32_*_f16, IEEE-half storage -- the arithmetic of the reference's fp16 autocast,
 * core/gdrn_modeling/main_gdrn.py:53-56,141, gdrn_evaluator.py:568) computes GDRN_DT_F16; each rejects the other's code with GDRN_ERR_ARG,
 * both compute GDRN_DT_F32.  gdrn_half_format() tells a host which one it opened. */
enum { GDRN_DT_F32 = 0, GDRN_DT_BF16 = 1, GDRN_DT_F16 = 2 };
/* status codes (0 = GDRN_OK) */
enum { GDRN_OK = 0, GDRN_ERR_ARG = -1, GDRN_ERR_SHAPE = -2, GDRN_ERR_LAUNCH = -3 };
/* deprecated aliases of ABI version 1 */
enum { GDRN_F32 = GDRN_DT_F32, GDRN_BF16 = GDRN_DT_BF16, GDRN_E_ARG = GDRN_ERR_ARG, GDRN_E_SHAPE = GDRN_ERR_SHAPE, GDRN_E_LAUNCH = GDRN_ERR_LAUNCH };
/* gdrn_wgrad_params.variant */
enum { GDRN_WGRAD_T64 = 0, GDRN_WGRAD_W128 = 1 /* removed in ABI 4: rejected by gdrn_conv3x3_wgrad_ok */ };

int gdrn_version(void);
/* Diagnostics: the HIP error code (hipError_t) behind the calling thread's most recent GDRN_ERR_LAUNCH, its name copied into `name` (cap bytes,
 * may be NULL); 0 if no launch of this thread has failed.  (ABI 3)  The call CLEARS the slot (ABI 4: a code is reported once, with the failure it
 * belongs to; every launch starts with a clean slot).  Without a launch error `name` reads "hipSuccess", or "stale:<name>" when a launch of this
 * thread found and dropped an error an earlier HIP call of the process had left behind. */
int gdrn_last_hip_error(char* name, int cap);
int gdrn_half_format(void);   /* GDRN_DT_BF16 or GDRN_DT_F16: the 16-bit dtype code this library build accepts */
/* Bytes of caller-owned scratch an entry point needs for the given call (every workspace of the ABI is caller-allocated device
 * memory, no initialisation needed unless stated): `op` selects the buffer, `params` points at the arguments that determine its
 * size.  < 0: GDRN_ERR_*.  (the Python engine sizes its plan buffers with the same rules.) */
enum {
    GDRN_WS_CONV_STATS = 0,     /* const gdrn_conv_params*  -> p->stats of gdrn_conv_gemm */
    GDRN_WS_CONV3X3_STATS = 1,  /* const gdrn_conv_params*  -> p->stats / p->bnb_rows of gdrn_conv3x3_halo */
    GDRN_WS_CONV3X3_WGRAD = 2,  /* const gdrn_wgrad_params* -> p->ws of gdrn_conv3x3_wgrad / one task of gdrn_conv3x3_wgrad_multi */
    GDRN_WS_STEM_WGRAD = 3,     /* const int* N             -> ws of gdrn_stem_wgrad */
    GDRN_WS_STEM_STATS = 4,     /* const int* N             -> stats of gdrn_stem_conv */
    GDRN_WS_LINEAR_SPLITK = 5,  /* const int[2] {M, N}      -> ws of gdrn_linear_splitk */
    GDRN_WS_BN_BWD_ROWS = 6     /* const long long[3] {npix, C, dtype} -> rows of gdrn_bn_bwd_reduce */
};
long long gdrn_workspace_bytes(int op, const void* params);
/* fills name (<=255 chars), compute units and the gcn arch string of device `dev`. */
int gdrn_device_info(int dev, char* name, int* cus, char* arch);

/* ------------------------------------------------------------------------------------------------
 * Implicit-GEMM gather convolution (forward conv, data gradient, transposed stride-2 conv, linear).
 * Replaces F.conv2d / F.conv_transpose2d / F.linear dispatched from
 *   resnet_backbone.py:23,69-80 + torchvision BasicBlock (twin: pvnet_net/resnet.py:44-74),
 *   cdpn_rot_head_region.py:81-135,183-185, conv_pnp_net.py:76-92,140-156,
 * and their autograd data-gradients (engine.py:279).
 *   mode 0: y[m][co] = sum_{ky,kx,c} x[n][oy*stride-pad+ky][ox*stride-pad+kx][c] * w[co][ky*KW+kx][c]
 *           m = (n*Ho+oy)*Wo+ox, M = N*Ho*Wo
 *   mode 1: transposed stride-2 gather (ConvTranspose2d forward / stride-2 data gradient):
 *           y[n][oy][ox][co] = sum x[n][(oy+pad-ky)/2][(ox+pad-kx)/2][c] * w[co][ky*KW+kx][c] over the
 *           taps where both divisions are exact; M = N*(Ho/2)*(Wo/2) (rows per parity class)
 *   w: packed [w_rows][KH*KW][Cin] of dtype, zero padded to w_rows (multiple of the N tile, see
 *      gdrn_conv_tile).  Cin*sizeof(dtype) must be a multiple of 128.
 *   epilogue: + bias[co] (fp32), + addend[m][co] (dtype), act (0 none, 1 ReLU, 2 LeakyReLU 0.1);
 *   stats != NULL: per-M-tile partial sum / sum of squares of the raw accumulators,
 *      stats[tile][0][co], stats[tile][1][co] (gdrn_conv_stats_rows tiles) for the following BatchNorm.
 *   bnb_x != NULL (gdrn_conv3x3_halo only, data-gradient launches): y is the gradient w.r.t. the OUTPUT of a
 *      BatchNorm(+ReLU) whose raw input was bnb_x[m][co] (channel stride bnb_cs).  The epilogue then also applies the
 *      ReLU mask -- (bnb_mask[m][co] > 0) when bnb_mask is given, else (bnb_x*bnb_scale + bnb_shift > 0) when
 *      bnb_scale/bnb_shift are given, else none -- stores the MASKED gradient and writes the two BatchNorm-backward sums
 *      of its pixel tile to bnb_rows[tile][2][Cout] (gdrn_conv3x3_stats_rows tiles, plain stores); gdrn_bn_bwd_coef
 *      turns the rows into the BatchNorm backward's coefficients: the separate reduction pass over (dy, x, mask) disappears.
 *   xf_mode != 0 (gdrn_conv3x3_halo only): the conv's INPUT is v(x, x2) evaluated per element while the patch is staged
 *      in LDS, rounded to bf16, zero outside the image (the padding applies to v, not to x), with per-input-channel
 *      fp32 vectors [Cin] (NULL a / b = 1, NULL c2 = 0):
 *        1: v = a*x + c                             BatchNorm(+ReLU) forward apply of the producer (a = scale, c = shift)
 *        2: v = (a*x + c) + bf16(b*x2 + c2)         ... with a residual (b = 1, c2 = 0) or a second normalised branch (the
 *                                                   BasicBlock downsample path, rounded as the pass that materialised it did)
 *        3: v = a*x + (b*x2 + c)                    BatchNorm backward apply: x = masked dy, x2 = the BN's raw input,
 *                                                   (a, b, c) from gdrn_bn_bwd_coef
 *        4: v = a*(x2*msc + msh > 0 ? x : 0) + (b*x2 + c)   the same with the ReLU mask recomputed from the forward affine
 *      then v = max(v, 0) when xf_relu.  x2 has the geometry and channel stride of x.  xf_out (nullable, same geometry
 *      and channel stride as x): v of every in-image pixel is also stored there once, so the tensor exists for the
 *      weight-gradient launch / the next residual without a separate pass.  Replaces gdrn_bn_apply /
 *      gdrn_bn_bwd_apply launches between two halo convs (BasicBlock, cdpn_rot_head_region.py:103-123 and backward).
 */
/* w_frag (gdrn_conv3x3_halo only): layout of w -- 0 / 1: gdrn_pack_wfrag (16-row fragments, first halo kernel), 2: gdrn_pack_wfrag32
 * (second-generation kernel, see gdrn_pack_wfrag32 below). */
/* halo_waves (gdrn_conv3x3_halo, w_frag 0 / 1; ABI 3): 0 = the library picks, 4 / 8 = force the four- / eight-wave form of the 128-channel tile
 * (gdrn_conv3x3_halo_waves below); v3_min_wg (w_frag 2): smallest grid the second-generation kernel gives its 16x16x256 tile, 0 = the default 256. */
typedef struct gdrn_conv_params {
    const void* x;
    const void* w;
    void* y;
    const float* bias;
    const void* addend;
    float* stats;
    const void* bnb_x;
    const void* bnb_mask;
    const float* bnb_mean;
    const float* bnb_invstd;
    const float* bnb_scale;
    const float* bnb_shift;
    float* bnb_rows;
    int bnb_cs;
    int w_frag;
    int Hi, Wi, Cin, x_cs;
    int Ho, Wo, Cout, y_cs, add_cs;
    int KH, KW, stride, pad;
    int mode, act, out_f32;
    int M, w_rows, dtype;
    int xf_mode, xf_relu;
    const void* xf_x2;
    const float* xf_a;
    const float* xf_b;
    const float* xf_c;
    const float* xf_c2;
    const float* xf_msc;
    const float* xf_msh;
    void* xf_out;
    int halo_waves;
    int v3_min_wg;
} gdrn_conv_params;
int gdrn_conv_gemm(const gdrn_conv_params* p, void* stream);
int gdrn_conv_tile(const gdrn_conv_params* p, int* bm, int* bn);
/* ResNet stem, bf16: 7x7 stride-2 pad-3 conv 3 -> 64 on the NHWC4 canvas of gdrn_pack_image (256x256 images ->
 * [N][262][272][4]), one kernel row = one 32-deep MFMA k-step, pixel fragments straight from global memory, weights in
 * registers (resnet_backbone.py:23,69).  w32 = gdrn_pack_stem_w32(OIHW fp32 weight) = bf16 [64][7][32];
 * y = [N][128][128][64]; stats (nullable) = [gdrn_stem_stats_rows(N)][2][64] partial sums for gdrn_bn_finalize. */
int gdrn_pack_stem_w32(const float* w, void* dst, int dtype, void* stream);
int gdrn_stem_stats_rows(int N);
int gdrn_stem_conv(const void* canvas, const void* w32, void* y, float* stats, int N, int dtype, void* stream);
/* Eval mode (module.eval(): BatchNorm on its running statistics): the stem conv, bn1 as per-channel scale / shift (gdrn_bn_eval_params), ReLU and
 * the 3x3 stride-2 max-pool of resnet_backbone.py:69-72 in one pass -- y = [N][64][64][64], bit-identical to gdrn_stem_conv followed by
 * gdrn_bn_relu_maxpool_fwd, without the 134 MB round trip of the conv output (ABI 3). */
/* Eval mode, 64 regions: the geometric head's 1x1 output conv (nn.Conv2d(256, 69, 1), cdpn_rot_head_region.py:127-135; w = weight rows
 * [>= 69][256] in the 16-bit format, fp32 bias) and gdrn_head_tail_fwd (GDRN.py:156-169) in one launch: the fp32 logits go to `head` only if it
 * is non-NULL ([N*HW][hs >= 72]; callers that return the maps), pnp_in as gdrn_head_tail_fwd writes it (ABI 3). */
int gdrn_head_conv_tail_fwd(const void* x, int x_cs, const void* w, int w_rows, const float* bias, const float* coord2d, const float* extents,
                            float* head, int hs, void* pnp_in, int pcs, int N, int HW, int nreg, int dtype, void* stream);
/* ... and with do_loss=True (GDRN.py:345-400) the same pass also accumulates the map-loss sums as gdrn_head_tail_loss_fwd does, one partial row per
 * workgroup: acc = 8 + 8 * gdrn_head_conv_tail_loss_rows(N, HW) doubles, finished by gdrn_map_loss_finalize_rows; head is mandatory (the backward
 * pass reads the logits). */
int gdrn_head_conv_tail_loss_rows(int N, int HW);
int gdrn_head_conv_tail_loss_fwd(const void* x, int x_cs, const void* w, int w_rows, const float* bias, const float* coord2d, const float* extents,
                                 float* head, int hs, void* pnp_in, int pcs, const float* gt_xyz, const float* mask_visib, const float* mask_trunc,
                                 const long long* gt_region, double* acc, int N, int HW, int nreg, int dtype, void* stream);
/* Data gradient of that 1x1 output conv (autograd, core/gdrn_modeling/engine.py:279) with the ReLU mask and the two BatchNorm-backward sums of the
 * BatchNorm(+ReLU) in front of it in the epilogue (cdpn_rot_head_region.py:120-135): dy = d_logits [N*HW][dy_cs >= 96] (channels >= 69 zero), wd = operand
 * rows [256][wd_cs >= 96] (row ci = W[:, ci]), raw / mean / invstd / scale / shift = that BatchNorm's raw input, batch statistics and forward affine
 * (mask: scale * raw + shift > 0), dx [N*HW][dx_cs] = the masked gradient, rows = [gdrn_head_out_dgrad_rows(N, HW)][2][256] for gdrn_bn_bwd_coef (ABI 3). */
int gdrn_head_out_dgrad_rows(int N, int HW);
int gdrn_head_out_dgrad(const void* dy, int dy_cs, const void* wd, int wd_cs, const void* raw, int raw_cs, const float* mean, const float* invstd,
                        const float* scale, const float* shift, void* dx, int dx_cs, float* rows, int N, int HW, int dtype, void* stream);
int gdrn_stem_conv_pool(const void* canvas, const void* w32, const float* scale, const float* shift, void* y, int N, int dtype, void* stream);
/* Stem weight gradient (backward-weight of nn.Conv2d(3, 64, 7, 2, 3), resnet_backbone.py:23, implicit in engine.py:279) fused with
 * the BatchNorm-backward apply in front of it: the stem has no data gradient, so dy = a*g + (b*raw + c) per channel
 * (gdrn_bn_bwd_apply's formula, rounded to bf16) is evaluated while the tile is staged instead of being written and re-read.
 *   canvas [N][262][272][4] bf16; g, raw [N][128][128][64] bf16 (masked upstream gradient / the conv output BatchNorm saw);
 *   a, b, c [64] from gdrn_bn_bwd_coef.  a == NULL: plain weight gradient with dy = g (raw, b, c ignored).
 *   ws: gdrn_stem_wgrad_parts(N) * 64 * 224 floats of scratch; grad: fp32 OIHW [64][3][7][7], overwritten.  bf16 only. */
int gdrn_stem_wgrad_parts(int N);
int gdrn_stem_wgrad(const void* canvas, const void* g, const void* raw, const float* a, const float* b, const float* c, int N,
                    float* ws, float* grad, int dtype, void* stream);
/* Skinny-M linear layer (M <= 64 rows, bf16): y[m][n] = act(sum_k x[m][k]*w[n][k] + bias[n]) with the K range split
 * over workgroups (the layer is bound by reading w once).  Replaces F.linear + LeakyReLU of Patch-PnP's fc1
 * (conv_pnp_net.py:85-92,152) where the gather kernel would run 8 workgroups.  x_rs / w_rs / y_rs: row strides in
 * elements; ws: GDRN_LINEAR_MAX_SPLITS*M*N floats (per-split partial slabs, no initialisation needed). */
#define GDRN_LINEAR_MAX_SPLITS 16
#define GDRN_LINEAR_NO_FINISH (-1)   /* (ABI 5) act: leave the gdrn_linear_splits(K, N) partial slabs [split][M][N] in ws, no bias / activation / y */
int gdrn_linear_splits(int K, int N);
int gdrn_linear_splitk(const void* x, const void* w, const float* bias, void* y, int M, int K, int N, int x_rs, int w_rs,
                       int y_rs, int act, float* ws, int dtype, void* stream);
int gdrn_conv_stats_rows(const gdrn_conv_params* p);
/* Halo-tiled variant for KH=KW=3, stride 1, pad 1, mode 0, H and W multiples of 8 (same params / epilogue contract):
 * the input patch of a TH x TW pixel tile is staged in LDS once per 128-byte channel chunk and the nine taps read
 * it at shifted offsets.  gdrn_conv3x3_tile reports (th, tw, bn), th = 0 when the shape is not covered;
 * gdrn_conv3x3_stats_rows the number of per-tile partial-statistics rows it writes. */
/* p->w of gdrn_conv3x3_halo is the FRAGMENT-MAJOR operand: gdrn_pack_wfrag permutes the 16-byte granules of the
 * row-major [rows][9][Cin] operand into one contiguous 1 KiB block per (16 rows, tap, 128-byte chunk, k-step) =
 * exactly the 64 lanes of an MFMA A operand, so the kernel streams weights L2 -> registers without LDS. bf16 only.
 * Row order: for operands of more than 64 rows (128-channel tile) the two 16-row blocks of a 32-row group interleave in units of
 * 4 rows, so that an MFMA result lane holds 8 contiguous output channels and the conv's epilogue moves 16 bytes per access. */
int gdrn_pack_wfrag(const void* src, void* dst, int rows, int Cin, int dtype, void* stream);
/* Second-generation halo kernel (conv3x3_v3.hip; Cin a multiple of 64, Cout of 128, W of 16, H of 8, bf16, act <= 1, bf16 output):
 * v_mfma_f32_32x32x16_bf16, the weights stream global -> LDS by LDS-DMA and are shared by the 8 waves of a workgroup, tiles of
 * 16x16 pixels x 256 channels (large maps) or 8x16 pixels x 128 channels with the K range split over two wave groups (small maps).
 * Selected by p->w_frag = 2; w is then the operand of gdrn_pack_wfrag32: one contiguous 1 KiB block = the 64 lanes of a 32x32x16
 * MFMA A operand per (128-byte chunk kc, tap, 16-deep k-substep ks, 32-row fragment f), block index ((kc*9 + tap)*4 + ks)*(rows/32) + f;
 * lane l of a block holds fragment row l & 31, k = 16*ks + 8*(l >> 5) .. +7.  Fragment f, row r is operand row
 * (f>>1)*64 + ((r>>2)&1)*32 + (f&1)*16 + (r>>3)*4 + (r&3): an MFMA result lane then holds 32 contiguous output channels per fragment
 * pair (64-byte epilogue accesses).  rows must be a multiple of 64.
 * gdrn_conv3x3_wfrag(p): operand layout for the shape in p: 2, 1, or 0 = no halo tiling.  p->w_frag is the caller's policy here: 0 = the
 * library's preference (the second-generation kernel where it measured faster), 1 = never that kernel, 2 = wherever it covers the shape.
 * The library reads no environment variables and keeps no configuration state: every choice it makes is a function of the params. */
int gdrn_pack_wfrag32(const void* src, void* dst, int rows, int Cin, int dtype, void* stream);
int gdrn_conv3x3_wfrag(const gdrn_conv_params* p);
int gdrn_conv3x3_halo(const gdrn_conv_params* p, void* stream);
int gdrn_conv3x3_tile(const gdrn_conv_params* p, int* th, int* tw, int* bn);
int gdrn_conv3x3_stats_rows(const gdrn_conv_params* p);
/* The first halo kernel's 128-channel tile exists in two forms: four waves, each walking the whole reduction of its 32 channels, and (ABI 3)
 * eight waves -- a second copy of the four takes k-step 1 of every tap stage, the first k-step 0, the halves are added through LDS in front
 * of the epilogue: two waves per SIMD for launches that give a CU a single workgroup (the 8x8 - 16x16 maps of resnet_backbone.py:53-80 at
 * 64 RoIs).  p->halo_waves = 0 lets the library pick (eight when the grid has <= 256 workgroups), 4 / 8 force one.
 * gdrn_conv3x3_halo_waves(p): waves per workgroup of the launch gdrn_conv3x3_halo makes for p (4 or 8; 0: w_frag = 2 or shape not covered). */
int gdrn_conv3x3_halo_waves(const gdrn_conv_params* p);

/* Weight gradient: dw[co][tap][ci] (fp32, packed, pre-zeroed by the caller) +=
 *   sum_m dy[m][co] * x[pix(m,tap)][ci]  (mode-0 gather; bf16 fragments through the LDS transpose read).  variant: 0 (only gdrn_conv3x3_wgrad* read it, see GDRN_WGRAD_W128).
 *   splits <= 0: automatic pixel-range split.
 * ws (gdrn_conv3x3_wgrad only, else NULL): per-split partial tiles go here (plain stores) instead of atomics on dw.
 * gdrn_conv_wgrad: Cin a multiple of 64; Cout <= 64 reads dy in 64-column slabs, else in 128-column slabs: dy_cs >= Cout rounded up to the
 *   slab, dy_cs * sizeof(T) a multiple of 16, x_cs * sizeof(T) a multiple of 8; x_cs < Cin is the window form ("channel" c of pixel (iy, ix) =
 *   element c of the flat row that starts there: the caller keeps every window inside its buffer).  Refused with GDRN_ERR_SHAPE: KH, KW, stride,
 *   Hi, Wi, Ho, Wo <= 0, pad < 0, M <= 0 or no multiple of Ho * Wo (whole images), the strides above; GDRN_ERR_ARG: x, dy or dw NULL, a dtype
 *   other than GDRN_DT_F32 / GDRN_DT_H16.  Rows co >= Cout of dw are never written.
 * Replaces the autograd weight-gradients of the same layers (engine.py:279). */
typedef struct gdrn_wgrad_params {
    const void* x;
    const void* dy;
    float* dw;
    float* ws;
    int Hi, Wi, Cin, x_cs;
    int Ho, Wo, Cout, dy_cs;
    int KH, KW, stride, pad;
    int M, dtype, splits, variant;
} gdrn_wgrad_params;
int gdrn_conv_wgrad(const gdrn_wgrad_params* p, void* stream);
/* Halo-tiled variant for KH=KW=3, pad 1, bf16, Cin and Cout multiples of 64; stride 1 (Ho, Wo multiples of 8) or stride 2 (Hi = 2*Ho,
 * Wi = 2*Wo, Ho a multiple of 4, Wo of 8: the ResNet stage-entry convs, Patch-PnP's convs, and ConvTranspose2d(3, 2, 1, 1) with x = the
 * gradient of its output and dy = its input): a workgroup
 * accumulates a 64 x 64 (co x ci) tile of all nine taps from one staged 8x8 pixel patch per stage.  Same dw layout and
 * accumulate-with-atomics contract.  gdrn_conv3x3_wgrad_ok returns 1 when the shape is covered; beyond the above it wants Cin, Cout, Ho,
 * Wo > 0, x_cs >= Cin, dy_cs >= Cout, x_cs and dy_cs multiples of 8, variant 0, and -- the kernel forms its byte offsets into x and dy in 32
 * bits -- M * dy_cs * 2 < 2^32 and (M / (Ho * Wo)) * Hi * Wi * x_cs * 2 < 2^32.  gdrn_conv3x3_wgrad returns GDRN_ERR_SHAPE for a shape that is
 * not covered or an M that is <= 0 or no multiple of Ho * Wo, GDRN_ERR_ARG for x or dy NULL or dw and ws both NULL; nothing is written then.
 * With p->ws != NULL the partial tiles of the gdrn_conv3x3_wgrad_splits(p) pixel-range splits are stored to
 * ws[split][Cout*Cin*9] (fragment order, no atomics, dw unused) and gdrn_wgrad_reduce_multi sums them for a whole
 * table of layers in one launch, writing dst[co*s_co + ci*s_ci + tap*s_t] (e.g. the OIHW .grad: s_co = Cin*9, s_ci = 9,
 * s_t = 1).  blk_start[i] = sum over tasks j < i of Cout_j*Cin_j/256; nblocks = blk_start[ntasks]. */
int gdrn_conv3x3_wgrad(const gdrn_wgrad_params* p, void* stream);
int gdrn_conv3x3_wgrad_ok(const gdrn_wgrad_params* p);
int gdrn_conv3x3_wgrad_splits(const gdrn_wgrad_params* p);
/* Grouped launch: the weight gradients of ntasks layers in one grid.  tasks_dev: device array of gdrn_wgrad_params with
 * ws != NULL and splits = gdrn_conv3x3_wgrad_splits() of an explicit request (no empty split).  The entry point cannot read its device
 * table: every task must have passed gdrn_conv3x3_wgrad_ok and the M check of gdrn_conv3x3_wgrad on the host (the 32-bit offset limits
 * included).  lds_bytes above 160 KiB: GDRN_ERR_ARG;
 * blk_start[i] = sum_{j<i} (Cout_j/64)*(Cin_j/64)*splits_j, nblocks = blk_start[ntasks]. */
int gdrn_conv3x3_wgrad_multi(const gdrn_wgrad_params* tasks_dev, const int* blk_start_dev, int ntasks, int nblocks, void* stream);
/* the same with an LDS request of lds_bytes (> 64 KiB: one workgroup per CU, the rest of the CU stays free for another stream's kernels) */
int gdrn_conv3x3_wgrad_multi_lds(const gdrn_wgrad_params* tasks_dev, const int* blk_start_dev, int ntasks, int nblocks, int lds_bytes, void* stream);
/* cin_valid: input channels the parameter really has (0 = Cin): padded operand channels are skipped */
typedef struct gdrn_wreduce_task {
    const float* ws;
    float* dst;
    int nsplit, Cout, Cin, cin_valid;
    long long s_co, s_ci, s_t;
} gdrn_wreduce_task;
int gdrn_wgrad_reduce_multi(const gdrn_wreduce_task* tasks_dev, const int* blk_start_dev, int ntasks, int nblocks, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Weight / layout packing.
 * gdrn_pack4: dst[a1][a2][t][b] (contiguous, A1 x A2 x T x B, dtype) = src[a1*s1 + a2*s2 + t'*st + b*sb]
 *   (fp32), zero where a1>=A1v, a2>=A2v or b>=Bv; t' = flip ? T-1-t : t.
 * gdrn_unpack4: the inverse scatter for gradients: src_grad[...] = packed[a1][a2][t][b] (fp32 -> fp32),
 *   only valid indices are written.
 * Used to turn the reference's OIHW / (Cin,Cout,kH,kW) / (out,in) parameter tensors
 * (state_dict schema) into the kernels' [rows][tap][Cin] operand layout. */
int gdrn_pack4(const float* src, void* dst, int A1, int A2, int T, int B, int A1v, int A2v, int Bv,
               long long s1, long long s2, long long st, long long sb, int flip, int dtype, void* stream);
int gdrn_unpack4(const float* packed, float* dst, int A1, int A2, int T, int B, int A1v, int A2v, int Bv,
                 long long s1, long long s2, long long st, long long sb, int flip, void* stream);
/* stem: conv1.weight (64,3,7,7) <-> [64][7][16 px * 4 ch]; image NCHW fp32 -> zero-padded NHWC4 */
int gdrn_pack_stem_w(const float* w, void* dst, int dtype, void* stream);
int gdrn_unpack_stem_w(const float* packed, float* dw, void* stream);
int gdrn_pack_image(const float* img, void* dst, int N, int H, int W, int Hp, int Wp, int dtype, void* stream);
/* generic casts between fp32 and dtype (n elements) */
int gdrn_cast_from_f32(const float* src, void* dst, long long n, int dtype, void* stream);
int gdrn_cast_to_f32(const void* src, float* dst, long long n, int dtype, void* stream);
/* NHWC (dtype, pixel stride cs) -> NCHW fp32 for handing maps back to the caller */
int gdrn_nhwc_to_nchw_f32(const void* src, int cs, int c0, int C, float* dst, int N, int HW, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm2d (train / eval), fused with ReLU, residual add and max-pool where the graph has them.
 * Replaces nn.BatchNorm2d + nn.ReLU + `out += identity` + nn.MaxPool2d at resnet_backbone.py:24-26,
 * BasicBlock, cdpn_rot_head_region.py:92-93,113-114 and their backward. */
/* partial: [rows][2][C] per-tile sums / sums of squares from a conv epilogue; one launch of C/4 workgroups whatever the row
 * count (fp64 accumulation).  ws: unused (kept for ABI stability; was a 64*2*C-double workspace of a two-launch scheme). */
int gdrn_bn_finalize(const float* partial, int rows, int C, double count, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, long long* num_batches_tracked, float momentum,
                     float eps, float* mean, float* invstd, float* scale, float* shift, double* ws, void* stream);
int gdrn_bn_eval_params(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                        float eps, int C, float* scale, float* shift, void* stream);
/* y = x*scale + shift (+ residual) (then ReLU), NHWC [npix][C].  C % 8 == 0 and C <= 512 (GDRN_ERR_ARG otherwise: the kernel stages the
 * per-channel constants in a 512-entry LDS array, like gdrn_bn_bwd_reduce / gdrn_bn_bwd_apply); C / V (V = 4 fp32, 8 16-bit) divides 256. */
int gdrn_bn_apply(const void* x, const float* scale, const float* shift, const void* residual, void* y,
                  long long npix, int C, int relu, int dtype, void* stream);
/* BatchNorm backward = (1) per-channel sums of g and g*xhat, g = dy * (ymask > 0) * (x*mask_scale + mask_shift > 0) (each mask
 * optional), as partial rows rows[r][0][c] = sum g, rows[r][1][c] = sum g*xhat: one row per workgroup of gdrn_bn_bwd_reduce
 * (gdrn_bn_bwd_reduce_rows(npix, C, dtype) <= 1024 of them, plain stores: deterministic, nothing to pre-zero), or one per pixel
 * tile straight from the epilogue of the data-gradient conv that produced dy (gdrn_conv_params.bnb_*);
 * (2) gdrn_bn_bwd_coef: rows -> dgamma, dbeta and the coefficients (a, b, c) of dx = a*g + (b*x + c);
 * (3) the apply pass gdrn_bn_bwd_apply (optional g_out = g), or no pass at all when the consumer of dx is a halo conv
 * (xf_mode 3 / 4) or the stem weight gradient (gdrn_stem_wgrad), which evaluate it while staging their operand.
 * mask_scale/mask_shift (both or neither): the ReLU mask recomputed from the forward affine of a BN->ReLU without residual
 * instead of reading the stored activation (one tensor pass less). */
int gdrn_bn_bwd_reduce_rows(long long npix, int C, int dtype);
int gdrn_bn_bwd_reduce(const void* dy, const void* ymask, const void* x, const float* mean, const float* invstd,
                       const float* mask_scale, const float* mask_shift, long long npix, int C, float* rows, int dtype,
                       void* stream);
int gdrn_bn_bwd_apply(const void* dy, const void* ymask, const void* x, const float* a, const float* b, const float* c,
                      const float* mask_scale, const float* mask_shift, long long npix, int C, void* dx, void* g_out,
                      int dtype, void* stream);
/* rows [nrows][2][C] (fp64 accumulation, one launch of C/4 workgroups) -> a = gamma*invstd, b = -a*invstd*sum(g*xhat)/npix,
 * c = -a*sum(g)/npix - b*mean; dgamma = sum g*xhat, dbeta = sum g (both or neither NULL); npix = elements per channel. */
int gdrn_bn_bwd_coef(const float* rows, int nrows, int C, long long npix, const float* gamma, const float* mean,
                     const float* invstd, float* a, float* b, float* c, float* dgamma, float* dbeta, void* stream);
int gdrn_bn_relu_maxpool_fwd(const void* x, const float* scale, const float* shift, void* y, unsigned char* idx,
                             int N, int H, int W, int C, int dtype, void* stream);
/* g = gradient w.r.t. the BatchNorm OUTPUT in front of the ReLU + max-pool (ReLU mask recomputed from x*scale + shift).
 * rows != NULL (then mean, invstd too): also that BatchNorm's backward sums of g, one partial row [2][C] per workgroup
 * (gdrn_maxpool_bwd_rows(N, H, W, C, dtype) rows, for gdrn_bn_bwd_coef) -- the separate gdrn_bn_bwd_reduce pass over g and x
 * disappears. */
int gdrn_maxpool_bwd_rows(int N, int H, int W, int C, int dtype);
int gdrn_maxpool_bwd(const void* dy, const unsigned char* idx, const void* x, const float* scale, const float* shift,
                     void* g, int N, int H, int W, int C, const float* mean, const float* invstd, float* rows, int dtype,
                     void* stream);

/* nn.UpsamplingBilinear2d(scale_factor=2) (align_corners=True), cdpn_rot_head_region.py:102 */
int gdrn_upsample2x_fwd(const void* x, void* y, int N, int H, int W, int C, int dtype, void* stream);
int gdrn_upsample2x_bwd(const void* dy, void* dx, int N, int H, int W, int C, int dtype, void* stream);
/* (ABI 4) BatchNorm + ReLU + 2x bilinear upsampling in one launch: y = upsample2x(relu(scale * x_raw + shift)), every source value rounded to the
 * storage format first (= gdrn_bn_apply followed by gdrn_upsample2x_fwd, bit for bit; cdpn_rot_head_region.py:103-123). */
int gdrn_bn_relu_upsample2x_fwd(const void* x_raw, const float* scale, const float* shift, void* y, int N, int H, int W, int C, int dtype, void* stream);
/* (ABI 4) gdrn_upsample2x_bwd + the reduction pass of the BatchNorm(+ReLU) backward that reads its result (gdrn_bn_bwd_reduce with the affine mask
 * mask_scale * x_raw + mask_shift > 0) in one launch: dx as gdrn_upsample2x_bwd writes it (unmasked), rows [gdrn_bn_bwd_reduce_rows(N*H*W, C,
 * dtype)][2][C] for gdrn_bn_bwd_coef. */
int gdrn_upsample2x_bwd_bnsums(const void* dy, void* dx, const void* x_raw, const float* mean, const float* invstd, const float* mask_scale,
                               const float* mask_shift, int N, int H, int W, int C, float* rows, int dtype, void* stream);

/* nn.GroupNorm(G, C) + ReLU (conv_pnp_net.py:78-80) and backward.  dgamma/dbeta: fp32 [C], accumulated
 * over samples (zeroed inside). */
int gdrn_gn_relu_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean_rstd, int N,
                     int HW, int C, int G, float eps, int dtype, void* stream);
int gdrn_gn_relu_bwd(const void* dy, const void* y, const void* x, const float* gamma, const float* mean_rstd,
                     void* dx, float* dgamma, float* dbeta, int N, int HW, int C, int G, int dtype, void* stream);

/* elementwise LeakyReLU(0.1) backward on [n] elements given the activation output y: dx = dy*(y>0?1:0.1) */
int gdrn_leaky_bwd(const void* dy, const void* y, void* dx, long long n, int dtype, void* stream);
/* bias gradient: db[c] = sum_rows dy[r][c]  (dy of dtype, row stride cs) */
int gdrn_bias_grad(const void* dy, int cs, int rows, int C, float* db, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Head tail: slicing of the 1x1 output conv into mask / xyz / region, channel softmax over
 * region[:,1:], concat with roi_coord_2d, extent de-normalisation -> Patch-PnP input
 * (GDRN.py:156-169, conv_pnp_net.py:121-125).  head: fp32 [N*HW][hs] = (mask, x, y, z, region[nreg+1]);
 * pnp_in: dtype [N*HW][pcs], channels (xyz(3), coord2d(2), softmax(nreg), zero pad).
 * Rows: 1 <= nreg <= 64 and EVERY row stride an entry point takes holds a whole row -- hs >= nreg + 5, pcs >= nreg + 5, dcs >= nreg + 5
 * (gdrn_head_tail_bwd: pcs only when d_pnp_in is given, pnp_in and d_pnp_in are not read otherwise; gdrn_map_loss_fwd: hs) -- else
 * GDRN_ERR_ARG and nothing is written: the kernels read h[4 + nreg] and pnp[4 + nreg], with a shorter stride the next pixel's values and,
 * in the last row, memory behind the buffer.  Columns >= nreg + 5 of head, pnp_in and d_pnp_in are never read; of d_pnp_in neither are
 * channels 3 and 4 used (the 2-D coordinates have no gradient). */
int gdrn_head_tail_fwd(const float* head, int hs, const float* coord2d, const float* extents, void* pnp_in, int pcs,
                       int N, int HW, int nreg, int dtype, void* stream);
/* Train mode: gdrn_head_tail_fwd and gdrn_map_loss_fwd in ONE pass over the logits (acc as below, zeroed inside).
 * dtype | GDRN_PREZEROED (here and in gdrn_head_tail_fwd / gdrn_head_tail_bwd): the pad channels of the pcs / dcs wide rows are
 * already zero and stay the caller's (the engine zero-fills its buffers once instead of re-writing 56 pad channels per pixel and step).
 * The contract, for every region count and row stride: WITHOUT the flag every channel >= nreg + 5 of a row is written as 0; WITH it the
 * channels from the end of the last written group on are not written at all -- >= 72 on the 64-region path (rows of whole 4-element groups:
 * 69..71 are still written as 0), >= nreg + 5 on the generic path. */
int gdrn_head_tail_loss_fwd(const float* head, int hs, const float* coord2d, const float* extents, void* pnp_in, int pcs,
                            const float* gt_xyz, const float* mask_visib, const float* mask_trunc, const long long* gt_region,
                            double* acc, int N, int HW, int nreg, int dtype, void* stream);
/* dtype | GDRN_ACC_ROWS (gdrn_head_tail_loss_fwd): acc is fp64 [8 + 8 * gdrn_head_tail_loss_rows(...)]; every workgroup STORES its partial
 * sums as row acc[8 + 8 r .. 8 + 8 r + 5] (no memset, no atomics: 24 k atomic adds onto one cache line cost the kernel 15 us, and their
 * order made the sums run-to-run different in the last bits); gdrn_map_loss_finalize_rows adds the rows in a fixed order into acc[0..7]
 * (what gdrn_head_tail_bwd reads) and writes the five map losses. */
#define GDRN_ACC_ROWS 0x200
int gdrn_head_tail_loss_rows(int N, int HW, int nreg, int hs, int pcs);
int gdrn_map_loss_finalize_rows(double* acc, int nrows, int N, int HW, float* losses, void* stream);
/* Map losses (GDRN.py:345-400): acc[0..2] = sum|x*m-gt*m| per coordinate, acc[3] = sum|mask-trunc|,
 * acc[4] = CE_sum(region*m, gt_region*m), acc[5] = sum m  (acc: fp64 [8], zeroed inside). */
int gdrn_map_loss_fwd(const float* head, int hs, const float* gt_xyz, const float* mask_visib, const float* mask_trunc,
                      const long long* gt_region, int N, int HW, int nreg, double* acc, void* stream);
/* d_head[m][0..nreg+4] (dtype, stride dcs, rest zero) = grad of sum_k gw[k]*loss_k through the map
 * losses plus the chain through the head tail from d_pnp_in (NULL: none).
 * gw: device fp32 [5] = dL/d(loss_coor_x, loss_coor_y, loss_coor_z, loss_mask, loss_region). */
int gdrn_head_tail_bwd(const float* head, int hs, const void* pnp_in, const void* d_pnp_in, int pcs,
                       const float* extents, const float* gt_xyz, const float* mask_visib, const float* mask_trunc,
                       const long long* gt_region, const double* acc, const float* gw, void* d_head, int dcs, int N,
                       int HW, int nreg, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pose decode + pose losses for one batch, one thread block per RoI:
 *   rot6d -> R_allo (rot_reps.py:34-49); (dcx,dcy,z_rel) -> t (pose_from_pred_centroid_z.py:176-212);
 *   allocentric -> egocentric (train: core/utils/utils.py:208-236 with eps; test: utils.py:39-94, no eps);
 *   point-matching loss (pm_loss.py:82-114, misc.py:930-949, symmetric: pose_utils.py:430-482),
 *   centroid / z L1 (GDRN.py:444-471).
 * fc: fp32 [N][fs] rows = (rot6d[6], t_[3]).  sym: fp32 [N][Kmax][9] + sym_count[N] (NULL: none).
 * outputs: rot [N][9], trans [N][3]; losses[3] = (loss_PM_R, loss_centroid, loss_z) (train mode: zeroed inside; test mode: not touched);
 * dfc: fp32 [3][N][fs] unit gradients d loss_k / d fc (NULL in test mode); vis: fp32 [N][2] per-RoI
 * rotation error (deg) / translation error. */
typedef struct gdrn_pose_params {
    const float* fc;
    int fs;
    const float* cams;
    const float* centers;
    const float* whs;
    const float* ratios;
    const float* extents;
    const float* gt_rot;
    const float* gt_trans;
    const float* gt_trans_ratio;
    const float* points;
    int npts;
    const float* sym;
    const int* sym_count;
    int Kmax;
    int N;
    int train;
    float* rot;
    float* trans;
    float* losses;
    float* dfc;
    float* vis;
    float* loss_rows;
    const float* gw;
    void* dfc_comb;
    const float* fc2_ws;
    const float* fc2_bias;
    void* f2_out;
    const void* w_rt;
    const float* b_rt;
    float* fc_w;
    int fc2_splits;
} gdrn_pose_params;
int gdrn_pose_loss(const gdrn_pose_params* p, void* stream);
/* (ABI 5, all nullable = the version-4 behaviour) loss_rows [N][4]: the three pose losses as one row per RoI instead of atomics onto `losses`
 * (no memset; gdrn_loss_finalize adds them in RoI order).  gw [3] + dfc_comb [N][fs] (16-bit): dL/dfc = sum_k gw[k] * unit gradient k, written
 * directly (train; `dfc` is then not written).  fc2_ws .. fc2_splits: the tail of Patch-PnP's fully connected stack in the same launch
 * (conv_pnp_net.py:152-160) -- fc2_ws = the gdrn_linear_splits(1024, 256) slabs [split][N][256] gdrn_linear_splitk(act = GDRN_LINEAR_NO_FINISH)
 * left, fc2_bias fp32 [256], LeakyReLU(0.1), f2_out [N][256] 16-bit (fc2's activation), w_rt 16-bit [>= 9][256] row-major (fc_r | fc_t),
 * b_rt fp32 [9], fc_w [N][fs] fp32 receives the nine outputs (`fc` is then not read). */
int gdrn_loss_finalize(double* acc, int nrows, int N, int HW, const float* pose_rows, float* losses, const float* w, float* weighted,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * Small fp32 helpers */
/* out[r][c] = sum_k w[k] * in[k][r][c]  (combine the unit gradients with the incoming loss grads) */
int gdrn_combine3(const float* in, const float* w, float* out, int n, void* stream);
/* map-loss finalisation: losses[0..4] from acc (GDRN.py:347-400) */
int gdrn_map_loss_finalize(const double* acc, int N, int HW, float* losses, void* stream);

/* Fused Ranger step (RAdam + gradient centralisation + Lookahead) over one parameter tensor
 * (lib/torch_utils/solver/ranger.py:100-200).  The tensor is viewed as [rows][cols]; gc != 0 subtracts
 * the per-row gradient mean first (ranger.py:144-145).  step_size / adaptive are the RAdam
 * rectification terms of ranger.py:154-186 (host scalars); lookahead != 0 applies
 * slow += alpha*(p - slow); p = slow (ranger.py:192-198). */
int gdrn_ranger_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, float* slow, int rows, int cols,
                     int gc, float lr, float beta1, float beta2, float eps, float weight_decay, float step_size,
                     int adaptive, int lookahead, float alpha, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-tensor variants: ONE launch for all parameter tensors.  Task tables are arrays in DEVICE memory built once by
 * the host; `*_start` are int prefix arrays [ntasks + 1] (workgroups for pack/unpack: ceil(n / gdrn_pack_chunk()) per
 * task; rows for Ranger).
 * gdrn_pack_task: gdrn_pack4 semantics (dst[a1][a2][t][b] = src[a1*s1 + a2*s2 + t'*st + b*sb], zero padded); frag = 1 / 2:
 *   dst is the fragment-major permutation (gdrn_pack_wfrag / gdrn_pack_wfrag32) of that [A1][1][9][B] operand.  For gdrn_unpack_multi the
 *   same struct describes gdrn_unpack4 (src = packed fp32, dst = parameter-layout gradient, n = A1v*A2v*T*Bv). */
/* Workgroups per task (blk_start prefix sums): ceil(n / gdrn_pack_chunk()) for row-major destinations; bf16 fragment-major
 * (frag = 1, T = 9) tasks take (A1/16) * (B/64) workgroups -- one per brick of 16 rows x 64 b x 9 taps. */
/* gdrn_pack_task.scale (pack only, nullable): per-row factor, dst[a1][..] = src[..] * scale[a1] -- eval mode folds the
 * BatchNorm scale gamma/sqrt(var+eps) of the following BN into the conv operand this way. */
/* gdrn_pack_task.pad_ (frag tasks): 1 + log2(B*sizeof(dtype)/128) when that chunk count is a power of two (the kernel
 * then shifts instead of dividing), else 0. */
/* (ABI 5) frag = 3: tiled transpose -- a ROW-MAJOR copy (gdrn_pack4 / gdrn_unpack4 semantics, flip = 0, no scale) whose unit-stride source index
 * is not b: pad_ = 1 / 2 / 3 names it (a1 / a2 / t); a workgroup moves a 64 x 64 tile of (that index, b) through LDS, reading the source along it
 * and writing the destination along b (fc1's operand copies and gradient: 8.4 M elements with b strides of 64 / 8192 floats).  Workgroups per
 * task: gdrn_pack_transpose_blocks (<= 0: the task does not qualify). */
typedef struct gdrn_pack_task {
    const float* src;
    void* dst;
    const float* scale;
    int A1, A2, T, B, A1v, A2v, Bv;
    int flip;
    long long s1, s2, st, sb;
    long long n;
    int frag;
    int pad_;
} gdrn_pack_task;
typedef struct gdrn_ranger_task {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* slow;
    int rows, cols, gc;
    float lr;
} gdrn_ranger_task;
/* gdrn_zero_multi: zero ntasks device regions (p 16-byte aligned, n16 granules of 16 bytes) in one launch; blk_start prefix sums of
 * ceil(n16 / gdrn_zero_chunk()).  With it a backward pass clears all its atomically-accumulated gradients (packed weight gradients
 * of the generic kernel, GroupNorm / bias / stem gradients) once, and the entry points below are called with GDRN_PREZEROED. */
typedef struct gdrn_zero_task {
    void* p;
    long long n16;
} gdrn_zero_task;
int gdrn_zero_chunk(void);
int gdrn_zero_multi(const gdrn_zero_task* tasks_dev, const int* blk_start_dev, int ntasks, int nblocks, void* stream);
/* gdrn_nonfinite_flag: *flag |= 1 if any of the n floats at x (16-byte aligned) is inf or NaN; *flag is never cleared by the library.  The
 * found_inf test of torch.cuda.amp.GradScaler (core/gdrn_modeling/main_gdrn.py:53-56, engine.py:276-283) for the fp16 arithmetic mode: the
 * host skips the optimizer step and backs the loss scale off when it is raised (ABI 3). */
int gdrn_nonfinite_flag(const float* x, long long n, int* flag, void* stream);
/* Dynamic loss scale of the fp16 arithmetic mode kept ON THE DEVICE (ABI 4, round 6): what torch.cuda.amp.GradScaler holds on the host and reads
 * back once per step (core/gdrn_modeling/engine.py:276-283 `scaler.step(optimizer)` / `scaler.update()`).  `flag` is the target of
 * gdrn_nonfinite_flag (first member: a gdrn_loss_scale_state* is a valid `int* flag`).  A step then is: backward pass with
 * gdrn_scaled_loss_weights' dL/dloss -> gdrn_nonfinite_flag over the gradients -> gdrn_ranger_multi_dyn (a no-op when the flag is raised; the RAdam
 * step index = base_step + applied + 1 counts applied steps only; the gradients are divided by `scale` inside the kernel) -> gdrn_loss_scale_update
 * (overflow: scale x 0.5 (>= 1), skipped + 1, flag cleared; clean: applied + applied_step, good + 1, and after `growth` clean steps in a row
 * scale x 2 (<= 65536)).  No host read anywhere; a host reads the struct when it wants to log or checkpoint. */
typedef struct gdrn_loss_scale_state {
    int flag;            /* raised by gdrn_nonfinite_flag, cleared by gdrn_loss_scale_update */
    int applied;         /* optimizer steps applied since the host wrote base_step */
    int skipped;         /* overflowed steps so far */
    int good;            /* clean steps since the scale last changed */
    int growth;          /* growth interval (0: the scale never grows) */
    float scale;         /* the loss scale on dL/dloss */
    float inv_scale;     /* 1 / scale */
    int base_step;       /* the optimizer's step count when `applied` was last zeroed */
    int last_overflowed; /* 1 if the step gdrn_loss_scale_update closed last had overflowed */
    int pad_[7];
} gdrn_loss_scale_state;
int gdrn_loss_scale_update(gdrn_loss_scale_state* state, int applied_step, void* stream);
/* g[i] = flag ? 0 : g[i] * factor / scale  (gradients handed to an external optimizer: unscaled, or zeroed when the step overflowed) */
int gdrn_unscale_or_zero(float* g, long long n, float factor, const gdrn_loss_scale_state* state, void* stream);
/* out[k] = w[k] * (w2 ? w2[k] : 1) * scale, k < n <= 64: dL/dloss of the scaled backward pass */
int gdrn_scaled_loss_weights(const float* w, const float* w2, int n, const gdrn_loss_scale_state* state, float* out, void* stream);
/* OR-ed into the `dtype` argument of gdrn_gn_relu_bwd / gdrn_bias_grad / gdrn_stem_wgrad: the gradient outputs they accumulate
 * into with atomics were zeroed by the caller (gdrn_zero_multi) -- skip the internal hipMemsetAsync (one launch each). */
#define GDRN_PREZEROED 0x100
int gdrn_pack_chunk(void);
int gdrn_pack_transpose_blocks(const gdrn_pack_task* task);
int gdrn_pack_multi(const gdrn_pack_task* tasks_dev, const int* blk_start_dev, int ntasks, int nblocks, int dtype, void* stream);
int gdrn_unpack_multi(const gdrn_pack_task* tasks_dev, const int* blk_start_dev, int ntasks, int nblocks, void* stream);
/* grad_scale: every gradient element is multiplied by it first (1/world_size when g holds the all-reduced SUM of the ranks'
 * gradients: the averaging pass over the 140 MB buffer disappears; 1.0 otherwise). */
int gdrn_ranger_multi(const gdrn_ranger_task* tasks_dev, const int* row_start_dev, int ntasks, int total_rows, float beta1,
                      float beta2, float eps, float weight_decay, float step_size, int adaptive, int lookahead, float alpha,
                      float grad_scale, void* stream);
/* the same update under a device-resident loss-scale state (see gdrn_loss_scale_state): step size / rectification / lookahead phase are
 * evaluated inside the kernel from state->base_step + state->applied + 1, the gradients are additionally divided by state->scale, and a raised
 * state->flag turns the launch into a no-op */
int gdrn_ranger_multi_dyn(const gdrn_ranger_task* tasks_dev, const int* row_start_dev, int ntasks, int total_rows, float beta1,
                          float beta2, float eps, float weight_decay, int n_sma_threshold, int lookahead_k, float alpha,
                          float grad_scale, const gdrn_loss_scale_state* state, void* stream);

/* (ABI 4) 3x3 STRIDE-2 pad-1 conv, forward, on a halo-tiled MFMA kernel (csrc/conv3x3s2.hip): ResNet-34's three stage-entry convs
 * (resnet_backbone.py:69-80, torchvision BasicBlock stride 2) and Patch-PnP's stride-2 convs (conv_pnp_net.py:76-92) -- optionally with the block's
 * 1x1 stride-2 shortcut conv (`downsample.0`) evaluated in the same launch from the same staged input (wd / yd / stats_d / bias_d).
 *   x [N][Hi][Wi][x_cs], y [N][Ho][Wo][y_cs], yd [N][Ho][Wo][yd_cs]: NHWC 16-bit; Hi = 2 Ho, Wi = 2 Wo, Ho % 4 == 0, Wo % 16 == 0 (or Wo % 8 == 0 and N even), Cin % 64 == 0,
 *   Cout % 128 == 0.  w: the FRAGMENT-MAJOR operand gdrn_pack_wfrag makes of the row-major [w_rows][9][Cin] weights; wd: ROW-MAJOR [wd_rows][Cin].
 *   stats / stats_d (nullable): [gdrn_conv3x3s2_stats_rows][2][Cout] partial sums for gdrn_bn_finalize; bias / bias_d (nullable) fp32 [Cout];
 *   act: 0 none, 1 ReLU (main conv only; the shortcut branch has none).
 *   (ABI 5) bnb_* (nullable, not combined with wd / stats / bias / act): the launch is a data gradient -- the ConvTranspose2d backward of the head is
 *   this conv applied to the output gradient -- w.r.t. a BatchNorm(+ReLU)'s output: y is masked where the stored activation bnb_mask <= 0 and rows
 *   [gdrn_conv3x3s2_stats_rows][2][Cout] of (sum g, sum g * (bnb_x - mean) * invstd) go to bnb_rows for gdrn_bn_bwd_coef (bnb_x / bnb_mask:
 *   [N][Ho][Wo][bnb_cs] 16-bit). */
typedef struct gdrn_s2_params {
    const void* x;
    const void* w;
    void* y;
    const float* bias;
    float* stats;
    const void* wd;
    void* yd;
    const float* bias_d;
    float* stats_d;
    int Hi, Wi, Cin, x_cs;
    int Ho, Wo, Cout, y_cs, yd_cs;
    int N, w_rows, wd_rows, act, dtype;
    const void* bnb_x;
    const void* bnb_mask;
    const float* bnb_mean;
    const float* bnb_invstd;
    float* bnb_rows;
    int bnb_cs;
} gdrn_s2_params;
int gdrn_conv3x3s2_ok(const gdrn_s2_params* p);
int gdrn_conv3x3s2_stats_rows(const gdrn_s2_params* p);
int gdrn_conv3x3s2(const gdrn_s2_params* p, void* stream);

/* (ABI 4) ... and its DATA GRADIENT (csrc/conv3x3s2_dgrad.hip; autograd backward of those convs, engine.py:279): dx [N][Hi][Wi][dx_cs] (Cin
 * channels) from dy [N][Ho][Wo][dy_cs] (Cout channels); w = the fragment-major operand gdrn_pack_wfrag makes of the row-major data-gradient
 * operand [w_rows >= Cin][9 taps, NOT flipped][Cout].  Optional: dyd / wdd -- the output gradient of the block's 1x1 stride-2 shortcut and its
 * ROW-MAJOR operand [wdd_rows >= Cin][Cout], whose data gradient is added in the same launch (even / even input pixels); bnb_* -- dx is the gradient
 * w.r.t. a BatchNorm(+ReLU)'s output: masked where the stored activation bnb_mask <= 0, and rows [gdrn_conv3x3s2_dgrad_rows][2][Cin] of
 * (sum g, sum g * (bnb_x - mean) * invstd) for gdrn_bn_bwd_coef.  Ho % 4 == 0, Wo % 16 == 0 (or Wo % 8 == 0 and N even), Cin % 64 == 0, Cout % 64 == 0.
 * (ABI 5) stats / bias / act -- the forward-conv epilogue, for the launch that IS the forward pass of nn.ConvTranspose2d(3, stride 2, pad 1,
 * output_padding 1) (dy = its input, dx = its output, w rows = its output channels): stats [gdrn_conv3x3s2_dgrad_rows][2][Cin] partial BatchNorm
 * sums of dx, bias fp32 [Cin], act 0 / 1 = ReLU.  All three NULL / 0: a data gradient.  Not combined with dyd / bnb_*. */
typedef struct gdrn_s2d_params {
    const void* dy;
    const void* w;
    void* dx;
    const void* dyd;
    const void* wdd;
    const void* bnb_x;
    const void* bnb_mask;
    const float* bnb_mean;
    const float* bnb_invstd;
    float* bnb_rows;
    int bnb_cs;
    int Hi, Wi, Cin, dx_cs;
    int Ho, Wo, Cout, dy_cs, dyd_cs;
    int N, w_rows, wdd_rows, dtype;
    float* stats;
    const float* bias;
    int act;
} gdrn_s2d_params;
int gdrn_conv3x3s2_dgrad_ok(const gdrn_s2d_params* p);
int gdrn_conv3x3s2_dgrad_rows(const gdrn_s2d_params* p);
int gdrn_conv3x3s2_dgrad(const gdrn_s2d_params* p, void* stream);

/* (ABI 4) One 64-channel ResNet BasicBlock in EVAL mode as one launch: y = relu(conv2(relu(conv1(x) + b1)) + b2 + x), both convs 3x3 stride 1
 * pad 1 with the BatchNorms folded into weights / biases (resnet_backbone.py:69-80 under model.eval(): ResNet-34's layer1 at inference).  x, y:
 * [N][H][W][64] NHWC 16-bit, y != x; w1, w2: the fragment-major operands gdrn_pack_wfrag makes of the row-major [64][9][64] weights; b1, b2: fp32
 * [64].  Bit-identical to the two gdrn_conv3x3_halo launches it replaces; the 64-channel intermediate stays in LDS.  gdrn_block64_eval_ok: 1 if
 * the shape is covered (H % 8 == 0, W % 16 == 0). */
int gdrn_block64_eval_ok(int N, int H, int W, int dtype);
int gdrn_block64_eval(const void* x, const void* w1, const float* b1, const void* w2, const float* b2, void* y, int N, int H, int W, int dtype,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * Inference post-processing on the device: get_out_coor + get_out_mask
 * (core/gdrn_modeling/engine_utils.py:92-126, L1 branches) and GDRN_Evaluator.get_img_model_points_with_coords2d
 * (gdrn_evaluator.py:89-126, max_num_points < 4) for the whole batch, one workgroup per RoI.
 *   mask / coor_{x,y,z}: fp32 maps, element (n, pixel) at base[n*roi_stride + pixel*pix_stride]
 *     (NCHW [N,1,H,W] tensors: roi_stride = HW, pix_stride = 1; the engine's NHWC head output: hs*HW, hs)
 *   coord2d [N][2][HW], extents [N][3], im_hw [N][2] = (im_H, im_W), mask_thr = cfg.MODEL.CDPN.ROT_HEAD.MASK_THR_TEST
 *   out_mask [N][HW] = (mask - min)/(max - min) per RoI;  out_xyz [N][3][HW] (either may be NULL)
 *   img_pts [N][HW][2], model_pts [N][HW][3]: the selected pixels of RoI n in row-major order, counts[n] of them
 *     (both NULL: only the maps / counts).  fp32, the reference's operation order: bit-identical results. */
int gdrn_correspondences(const float* mask, const float* coor_x, const float* coor_y, const float* coor_z, long long roi_stride,
                         int pix_stride, const float* coord2d, const float* extents, const float* im_hw, float mask_thr, int N,
                         int HW, float* out_mask, float* out_xyz, float* img_pts, float* model_pts, int* counts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GPU RoI cropper / target builder: what the reference's data loader does per instance on
 * the host with cv2 + numpy, for a whole batch of RoIs cut from frames that are already resident in HBM.
 *   replaces  crop_resize_by_warp_affine / get_affine_transform     core/utils/data_utils.py:80-137
 *             roi_img + normalize_image, roi_coord_2d                core/gdrn_modeling/data_loader.py:425-439, 487-498;
 *                                                                     core/base_data_loader.py:114-118
 *             roi_mask_{trunc,visib,obj}, roi_xyz, xyz_to_region,    data_loader.py:460-545, 617-632;
 *             roi_wh / resize_ratio / trans_ratio                     core/utils/data_utils.py:213-219
 * cv2.getAffineTransform / cv2.warpAffine (INTER_LINEAR on u8 and fp32, INTER_NEAREST, BORDER_CONSTANT 0) are followed
 * operation by operation (double LU + inversion, 10-bit fixed-point walk, 1/32-pixel bilinear table), rot = 0.
 * One gdrn_roi_task per RoI, as a device array.  Train-only members may be NULL / 0 when only gdrn_roi_crop_inputs is
 * used (test mode). */
/*   image     [H][W][3] u8 frame (the reference reads BGR) this RoI is cut from
 *   coord2d   [H][W][2] fp32 get_2d_coord_np(W, H, fmt="HWC") of that frame size
 *   xyz_crop  [y2-y1+1][x2-x1+1][3] fp32 object coordinates (xyz_info["xyz_crop"]); x1..y2 = xyz_info["xyxy"], inclusive (train)
 *   seg       [H][W] u8 0/1 visible-instance mask (anno["segmentation"]) (train)
 *   trunc     [H][W] u8 0/1 mask from background replacement, or NULL: mask_trunc = mask_visib (train)
 *   cx, cy, scale   bbox_center and the (clamped) square crop size in source pixels
 *   bw, bh          max(x2 - x1, 1), max(y2 - y1, 1) of the annotated box
 *   ox, oy, tz      anno["centroid_2d"] and trans[2] (train);  cls = row of fps_points / extents */
typedef struct gdrn_roi_task {
    const unsigned char* image;
    const float* coord2d;
    const float* xyz_crop;
    const unsigned char* seg;
    const unsigned char* trunc;
    double cx, cy, scale, bw, bh, ox, oy, tz;
    int H, W, x1, y1, x2, y2, cls, pad_;
} gdrn_roi_task;
/* minv [B][2][6] doubles: warpAffine's inverted 2x3 matrix (destination pixel -> source position) for the in_res and the
 * out_res crop of every RoI;  roi_wh [B][2], resize_ratio [B], trans_ratio [B][3] fp32 (each may be NULL). */
int gdrn_roi_affine(const gdrn_roi_task* tasks_dev, int B, int in_res, int out_res, double* minv, float* roi_wh, float* resize_ratio,
                    float* trans_ratio, void* stream);
/* roi_img [B][3][in_res][in_res] = (bilinear u8 crop - pixel_mean) / pixel_std (host arrays of 3 doubles, evaluated in
 * double like numpy);  roi_coord_2d [B][2][out_res][out_res] bilinear fp32 crop.  Either output may be NULL. */
int gdrn_roi_crop_inputs(const gdrn_roi_task* tasks_dev, const double* minv, int B, int in_res, int out_res, const double* pixel_mean,
                         const double* pixel_std, float* roi_img, float* roi_coord_2d, void* stream);
/* Train-mode targets at out_res (nearest crops): roi_xyz [B][3][r][r] = xyz / extent + 0.5, roi_mask_* [B][r][r] fp32,
 * roi_region [B][r][r] int32 = 1 + argmin_k |xyz - fps_points[cls][k]| on object pixels, 0 elsewhere (NULL together with
 * fps_points when NUM_REGIONS <= 1).  fps_points [ncls][nfps][3] double, extents [ncls][3] fp32, device arrays. */
int gdrn_roi_targets(const gdrn_roi_task* tasks_dev, const double* minv, int B, int out_res, const double* fps_points, int nfps,
                     const float* extents, float* roi_xyz, float* roi_mask_trunc, float* roi_mask_visib, float* roi_mask_obj,
                     int* roi_region, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pose-error metrics and recall table on the device (added within ABI 5: new entry points, nothing changed): what the reference's
 * evaluator computes on the host per instance right after inference (GDRN_EvaluatorCustom._eval_predictions,
 * core/gdrn_modeling/gdrn_custom_evaluator.py:493-670 with lib/pysixd/pose_error.py:297-444 and get_closest_rot, core/utils/pose_utils.py:430-454).
 * All arithmetic and every output is fp64, like the reference's numpy.  Per row i of N:
 *   R_est, R_gt [N][3][3], t_est, t_gt [N][3], K [N][3][3] fp64;  labels [N] int32 (class of the row) on the device, labels_host the same N
 *   values in host memory: they are checked against [0, C) on the host before anything is launched (GDRN_ERR_ARG).
 * Per-class tables (device): pts [C][n_max][3] fp64 with npts [C] valid rows each (the padding is never read into a sum or a minimum),
 *   is_sym [C] int32 (non-zero: the class is scored with adi and the closest-rotation search), sym [C][Kmax][3][3] fp64 with nsym [C] valid
 *   entries each (Kmax = 0: sym / nsym may be NULL).
 * err [N][4] = (ad, re, te, proj):  te = |t_gt - t_est|;  R_gt' = R_gt, replaced by R_gt S_k for each symmetry of a symmetric class, in table
 *   order, whenever re(R_est, R_gt S_k) is strictly smaller;  re = re(R_est, R_gt') in degrees;  proj = mean reprojection distance of the class's
 *   points under (R_est, t_est) and (R_gt', t_gt), pixels;  ad = add (mean distance of corresponding points) for a non-symmetric class, adi
 *   (mean distance from each ground-truth-posed point to the nearest estimate-posed point, exact, with the plain R_gt) for a symmetric one.
 * workspace: gdrn_pose_metrics_workspace_bytes(N, n_max) bytes of device memory, no initialisation needed.  Sums are reduced in a fixed order
 *   (no floating-point atomics): the same call gives the same bits. */
long long gdrn_pose_metrics_workspace_bytes(int N, int n_max);
int gdrn_pose_errors(const double* R_est, const double* t_est, const double* R_gt, const double* t_gt, const double* K, const int* labels,
                     const int* labels_host, int N, const double* pts, const int* npts, int n_max, const int* is_sym, const double* sym,
                     const int* nsym, int Kmax, int C, double* err, void* workspace, void* stream);
/* Adds the rows of err [N][4] to the caller's per-class running state (device memory, zeroed by the caller before the first call):
 * hits [C][15] = counts of ad < {0.02, 0.05, 0.10} diameter | (re < d and te < d/100), d = 2, 5, 10 | re < {2, 5, 10} | te < {0.02, 0.05, 0.10} |
 * proj < {2, 5, 10} (strict, the order of the evaluator's metric_names);  seen [C] and err_cnt [C] += rows of the class;  re_sum / te_sum [C] +=
 * their re / te (one workgroup per class, fixed order).  diameter [C] fp64.  Calls on one stream follow each other. */
int gdrn_pose_recall_accumulate(const double* err, const int* labels, const int* labels_host, int N, const double* diameter, int C,
                                long long* hits, long long* seen, double* re_sum, double* te_sum, long long* err_cnt, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Batched PnP-RANSAC and iterative PnP (added within ABI 5: new entry points, nothing changed): the step the reference's evaluator runs per RoI
 * on the host with cv2.solvePnPRansac / cv2.solvePnP between the correspondences and the pose metrics --
 *   GDRN_Evaluator.process_pnp_ransac (core/gdrn_modeling/gdrn_evaluator.py:316-392 -> lib/pysixd/misc.py:145-194) and process_net_and_pnp
 *   (:187-307), i.e. cfg.TEST.PNP_TYPE = ransac_pnp | net_ransac_pnp | net_iter_pnp --
 * for a whole batch, one workgroup per RoI.  Inputs are what gdrn_correspondences writes:
 *   img_pts [N][stride][2] pixels, model_pts [N][stride][3], fp32 (the *_f64 twins: the same layout in fp64, as cv2 accepts either);
 *   counts [N] int32 on the device: only the first counts[n] rows of RoI n are valid, the rest is never read into a result;  counts_host: the same
 *   N values in host memory, checked against [0, stride] before anything is launched (GDRN_ERR_ARG);  K [N][3][3] fp64.
 * All pose arithmetic is fp64.  R [N][3][3], t [N][3] fp64 are in/out: a RoI that cannot be solved (counts[n] < 4, no hypothesis with >= 4 inliers, a
 * non-finite result) keeps the caller's values and gets ok[n] = 0 (num_inliers 0, inlier_mask 0, rms NaN), every other one ok[n] = 1.
 * gdrn_pnp_ransac.  Sampling: hypothesis h of RoI n takes draws d = 0, 1, ... of
 *     x = mix64(seed * 0x9E3779B97F4A7C15 + n * 0xBF58476D1CE4E5B9 + h * 0x94D049BB133111EB + d * 0xD6E8FEB86659FD93)   (mod 2^64; mix64 = the
 *     splitmix64 finaliser),  index = ((x >> 32) * counts[n]) >> 32,
 *   keeping the first 4 distinct indices (a collision advances d; after 64 draws the hypothesis is dropped): no RNG state, the same (seed, inputs)
 *   give the same samples whatever the launch shape.  Minimal solve: P3P on the first three samples after normalising with K^-1, the solution with the
 *   smallest reprojection error on the fourth; a degenerate sample scores 0.  Scoring: inliers are the points with z > 0 and a squared pixel
 *   error < reproj_err^2, counted as integers.  Selection: the highest count wins, ties go to the lowest h.  The winner is refined on its inliers
 *   (below), the inliers are re-selected under the refined pose, and it is refined once more: inlier_mask [N][stride] u8 (or NULL), num_inliers [N]
 *   and rms [N] (or NULL; root of the inliers' mean squared pixel distance) are those of the returned pose.
 * Refinement (both calls): minimises the sum of squared pixel distances by Levenberg-Marquardt on (rotation-vector increment applied on the left,
 *   translation increment); stop rule: a step below 1e-10 (rotation in rad, translation relative to |t|) is applied and ends it, as do max_iter
 *   evaluations (the reference's default solver has 20).  Sums are reduced in a fixed order, no floating-point atomics: repeated calls are bit-identical.
 * gdrn_pnp_refine: from the caller's (R, t) over all counts[n] points without a gate (SOLVEPNP_ITERATIVE with useExtrinsicGuess); rms over all of them.
 * workspace: gdrn_pnp_workspace_bytes(N, stride, iters) bytes of device memory, no initialisation needed (gdrn_pnp_refine uses none: may be NULL).
 * Not cv2's algorithm: a fixed hypothesis count instead of the 0.99-confidence early stop, P3P + least squares instead of EPnP. */
long long gdrn_pnp_workspace_bytes(int N, int stride, int iters);
int gdrn_pnp_ransac(const float* img_pts, const float* model_pts, const int* counts, const int* counts_host, const double* K, int N, int stride,
                    double reproj_err, int iters, unsigned long long seed, int max_iter, double* R, double* t, int* ok, int* num_inliers,
                    unsigned char* inlier_mask, double* rms, void* workspace, void* stream);
int gdrn_pnp_refine(const float* img_pts, const float* model_pts, const int* counts, const int* counts_host, const double* K, int N, int stride,
                    int max_iter, double* R, double* t, int* ok, double* rms, void* workspace, void* stream);
int gdrn_pnp_ransac_f64(const double* img_pts, const double* model_pts, const int* counts, const int* counts_host, const double* K, int N,
                        int stride, double reproj_err, int iters, unsigned long long seed, int max_iter, double* R, double* t, int* ok,
                        int* num_inliers, unsigned char* inlier_mask, double* rms, void* workspace, void* stream);
int gdrn_pnp_refine_f64(const double* img_pts, const double* model_pts, const int* counts, const int* counts_host, const double* K, int N,
                        int stride, int max_iter, double* R, double* t, int* ok, double* rms, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Batched depth rasterizer and object-coordinate targets (added within ABI 5: new entry points, nothing changed): what the reference makes in an
 * offline pass per annotated instance (tools/lm/lm_pbr_1_gen_xyz_crop.py) -- an OpenGL depth render of the object under the ground-truth pose,
 * misc.calc_xyz_bp_fast (lib/pysixd/misc.py:288-316) and mask2bbox_xyxy (lib/utils/mask_utils.py:39-44) -- for N instances per call.
 * Mesh table (device, packed without padding): verts [sum nverts][3] fp64 metres and faces [sum nfaces][3] int32 (vertex indices within the class),
 *   class c owning the rows vert_off[c] .. + nverts[c] and face_off[c] .. + nfaces[c];  f_max = the largest nfaces[c] (sizes the launch).
 * Per instance i: labels[i] (device int32; labels_host the same N values in host memory, checked against [0, C) before anything is launched),
 *   R [N][3][3], t [N][3] (model -> camera, metres), K [N][3][3] fp64: upper triangular, read as [[fx, s, cx], [0, fy, cy], [0, 0, 1]].
 * gdrn_render_depth: depth [N][H][W] fp32 = camera-space z in metres of the nearest surface, 0 where nothing is drawn.  The rules:
 *   rays       pixel (x, y), integer coordinates, is sampled on d = K^-1 [x, y, 1] -- the ray calc_xyz_bp_fast back-projects along; no half-pixel offset
 *   coverage   with camera-space vertices a, b, c: covered when d.(a x b), d.(b x c), d.(c x a) are all >= 0 or all <= 0 (ray space, no perspective
 *              divide; edges inclusive, both windings, no culling)
 *   depth      z = (n.a) / (n.d), n = (b - a) x (c - a): exact under perspective
 *   precision  setup and per-pixel arithmetic in fp64, the depth rounded to fp32 once
 *   order      a face's vertex indices are sorted ascending first and every edge's cross product is taken on its vertex pair in ascending index
 *              order: two triangles evaluate the same bits for a shared edge, so a pixel exactly on it is never dropped by both (watertight), and
 *              the result depends neither on the order of the faces nor on their winding
 *   depth test the nearest fragment wins by an unsigned atomic min on the bits of the positive fp32 depth; the buffer is cleared to +inf and
 *              resolved to 0 inside the call: independent of scheduling, repeated calls are bit-identical
 *   dropped    a triangle with any vertex at z < near, WHOLE -- there is NO near-plane clipping (BOP objects are in front of the camera);  a
 *              degenerate triangle (n == 0);  a fragment with n.d == 0, with z > far, or whose fp32 depth is not positive and finite
 *   frame      a triangle's pixel walk is clipped to the frame; an instance entirely outside leaves its slice all zero
 *   0 < near < far is required (the tool's values: 0.01, 6.5).
 * gdrn_xyz_from_depth: depth [N][H][W] fp32 from the call above or from the caller;  xyz [N][H][W][3] fp32 = R^T (depth K^-1 [x, y, 1] - t)
 *   evaluated in fp64, exactly 0 where depth == 0;  mask [N][H][W] u8 = depth != 0;  xyxy [N][4] int32 = the inclusive bounds of the mask
 *   (x1, y1, x2, y2; integer atomic min / max, finished on the device);  visible [N] int32 = the mask is not empty.  An empty mask gives
 *   xyxy = (0, 0, W - 1, H - 1), visible = 0 and an all-zero xyz, the tool's record of an instance that is not visible (:142-150).
 * Neither call needs scratch memory or reads anything back. */
int gdrn_render_depth(const double* verts, const int* faces, const int* vert_off, const int* nverts, const int* face_off, const int* nfaces,
                      int C, int f_max, const int* labels, const int* labels_host, const double* R, const double* t, const double* K, int N,
                      int H, int W, double near, double far, float* depth, void* stream);
int gdrn_xyz_from_depth(const float* depth, const double* R, const double* t, const double* K, int N, int H, int W, float* xyz,
                        unsigned char* mask, int* xyxy, int* visible, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BOP pose errors (VSD, MSSD, MSPD) and their recall counts (added within ABI 5: new entry points, nothing changed): what the reference gets by
 * writing a CSV and running the BOP toolkit on the host (core/gdrn_modeling/gdrn_evaluator.py:437-514 -> lib/pysixd/scripts/eval_calc_errors.py:344-372
 * with lib/pysixd/pose_error.py:84-179, then eval_calc_scores.py) -- for N estimates per call, one estimate per ground-truth target.  Units: metres
 * and pixels.  Every decision and every output is fp64 except the fp32 visibility difference noted below; no floating-point atomics (integer counts;
 * fp64 sums and minima as per-workgroup partials finished in a fixed order): repeated calls give the same bits, and a row's result does not depend
 * on the other rows of the call.  The speed shortcuts of eval_calc_errors.py:328-347,366-367 (VSD = 1 / MSSD = inf for bounding spheres that do
 * not overlap) are NOT applied: the errors are the functions' values.
 *
 * gdrn_vsd (pose_error.py:84-126, visibility.py:27-36,72-73 in "bop19" mode, misc.py:565-588):
 *   depth_est, depth_gt [N][H][W] fp32: the model under the estimated / the ground-truth pose, the output layout of gdrn_render_depth (0 = nothing);
 *   depth_test [F][H][W] fp32: the test images' depth (0 = missing);  frame [N] int32 (device): the test image of row i, several rows may share
 *   one;  frame_host: the same N values in host memory, checked against [0, F) before anything is launched (GDRN_ERR_ARG);  K [N][3][3] fp64, read
 *   as fx = K[0][0], cx = K[0][2], fy = K[1][1], cy = K[1][2] -- K[0][1] (skew) is NOT read, as in misc.py:565-566;  diameter [N] fp64 (per ROW);
 *   taus [T] fp64 (device), T <= GDRN_VSD_MAX_TAUS;  cost_type GDRN_VSD_STEP | GDRN_VSD_TLINEAR.
 *   Per pixel (x, y): dist = sqrt((X d)^2 + (Y d)^2 + d^2) in fp64 of each of the three depths d, X = (x - cx) / fx, Y = (y - cy) / fy;
 *     visib_gt  = ((float)dist_gt - (float)dist_test <= (float)delta  or  dist_test == 0)  and  dist_gt > 0     -- the difference in fp32, as the
 *                 reference takes it; delta rounded to fp32 as numpy compares an fp32 array with a Python float
 *     visib_est = (the same with dist_est)  or  (visib_gt and dist_est > 0)
 *     dists     = |dist_gt - dist_est| on visib_gt and visib_est, divided by diameter when normalized_by_diameter != 0
 *     cost      = dists >= tau (step)  |  min(dists / tau, 1) (tlinear)
 *   err [N][T] = (sum of costs + |union| - |intersection|) / |union|, 1.0 for every tau when the union is empty.
 *   counts [N][2 + T] int64 = |union|, |union| - |intersection|, and per tau the STEP cost count (whatever cost_type); cleared inside the call.
 *   A pixel where both model depths are 0 is in neither mask and is skipped.  The tlinear sum is taken in a fixed order that is not numpy's: it
 *   agrees with it to about (|intersection| + 4) 2^-52 relative; the step error is one division of two exact integers.
 *   workspace: gdrn_vsd_workspace_bytes(N, H, W, T) bytes of device memory, no initialisation needed.
 *
 * gdrn_mssd_mspd (pose_error.py:131-179): poses, K (all of it: misc.project_pts multiplies by the whole matrix), labels and labels_host as in
 *   gdrn_pose_errors;  pts [C][n_max][3] fp64 with npts [C] valid rows each;  sym_R [C][S_max][3][3], sym_t [C][S_max][3] fp64 with nsym [C] >= 1
 *   valid transformations each (the identity included where it belongs: misc.get_symmetry_transformations).  Rows beyond npts[c] and
 *   transformations beyond nsym[c] never enter a result.  err [N][2] = (MSSD in metres, MSPD in pixels): the minimum over the class's
 *   transformations (R_gt S, R_gt t_S + t_gt) of the maximum over its points of the distance to the estimate-posed point, in 3D and in the image.
 *   A NaN in a pose gives NaN (never a hang); nsym[c] = 0 gives NaN.  Work is spread over (row, slab of 8 transformations), the slabs' minima are
 *   finished in slab order.  workspace: gdrn_mssd_mspd_workspace_bytes(N, n_max, S_max) bytes, no initialisation needed.
 *
 * gdrn_bop_recall_accumulate: adds a batch (vsd_err [N][T] from gdrn_vsd, mssd_mspd_err [N][2]) to the caller's per-class state (device memory,
 *   zeroed by the caller before the first call), GDRN_BOP_NTH = 10 thresholds each, passed as fp64 device arrays (eval_pose_results_more.py:58-63:
 *   np.arange(0.05, 0.51, 0.05) twice and np.arange(5, 51, 5)), strict <:
 *     hits_vsd [C][T][10] += vsd < ths_vsd[k];   hits_mssd [C][10] += mssd / diameter[c] < ths_mssd[k]   (diameter [C] fp64, per CLASS);
 *     hits_mspd [C][10] += (640 / im_width) mspd < ths_mspd[k]   (eval_calc_scores.py:239-250);   seen [C] += rows of the class.
 *   One workgroup per class, integer adds; calls on one stream follow each other. */
#define GDRN_VSD_MAX_TAUS 32
#define GDRN_BOP_NTH 10
enum { GDRN_VSD_STEP = 0, GDRN_VSD_TLINEAR = 1 };
long long gdrn_vsd_workspace_bytes(int N, int H, int W, int T);
int gdrn_vsd(const float* depth_est, const float* depth_gt, const float* depth_test, const int* frame, const int* frame_host, int F,
             const double* K, const double* diameter, int N, int H, int W, double delta, const double* taus, int T, int cost_type,
             int normalized_by_diameter, double* err, long long* counts, void* workspace, void* stream);
long long gdrn_mssd_mspd_workspace_bytes(int N, int n_max, int S_max);
int gdrn_mssd_mspd(const double* R_est, const double* t_est, const double* R_gt, const double* t_gt, const double* K, const int* labels,
                   const int* labels_host, int N, const double* pts, const int* npts, int n_max, const double* sym_R, const double* sym_t,
                   const int* nsym, int S_max, int C, double* err, void* workspace, void* stream);
int gdrn_bop_recall_accumulate(const double* vsd_err, int T, const double* mssd_mspd_err, const int* labels, const int* labels_host, int N,
                               const double* diameter, int C, double im_width, const double* ths_vsd, const double* ths_mssd,
                               const double* ths_mspd, long long* hits_vsd, long long* hits_mssd, long long* hits_mspd, long long* seen,
                               void* stream);

/* ------------------------------------------------------------------------------------------------
 * The errors and recall counts of the reference's YCB-V tables (added within ABI 5: new entry points, nothing changed): the error types
 * AUCadd / AUCadi / AUCad, ABSadd / ABSadi / ABSad, add, adi, reS, teS, reteS and projS of lib/pysixd/scripts/eval_pose_results_more.py:64-93, which
 * the reference scores on the host from a CSV (eval_calc_errors.py:395-448, pose_error.py:184-234,297-337, eval_calc_scores.py, pose_matching.py).
 * Everything is fp64, lengths in metres; poses, K, labels / labels_host and the per-class tables pts / npts / sym_R / sym_t / nsym as in
 * gdrn_pose_errors and gdrn_mssd_mspd (labels_host is checked against [0, C) on the host before anything is launched: GDRN_ERR_ARG; rows beyond
 * npts[c] and transformations beyond nsym[c] never enter a result).  No floating-point atomics, sums and minima in a fixed order: the same call
 * gives the same bits, and a row's result does not depend on the other rows of the call.  N <= 65535 per call (GDRN_ERR_SHAPE).
 *
 * gdrn_ad_errors: err [N][2] = (add, adi) of EVERY row whatever its class, both against the plain ground-truth pose: add the mean distance of
 *   corresponding points, adi the mean distance from each ground-truth-posed point to the nearest estimate-posed point (exact, brute force; the
 *   loop of gdrn_pose_errors).  Work is spread over (row, slab of GDRN_SIXD_AD_SLAB points), the estimate-posed points pass through LDS in tiles of
 *   GDRN_SIXD_AD_TILE; the slabs' sums are added in slab order.  workspace: gdrn_ad_errors_workspace_bytes(N, n_max) bytes, no initialisation.
 *
 * gdrn_sym_errors: err [N][3] = (re_sym [deg], te_sym [m], arp_2d_sym [px]), each the minimum over the class's nsym[c] >= 1 transformations
 *   (R_gt S, R_gt t_S + t_gt) of: the rotation error to R_est | pose_error.te_sym AS IT RUNS (below) | the mean over the class's points of the
 *   distance in the image between the point under that pose and under the estimate (K [R | t] [p, 1] divided by its third row).
 *   te_sym: pose_error.py:218 adds the flattened t_gt [3] to the column R_gt t_S [3,1]; numpy broadcasts, and the value returned is the Frobenius
 *   norm of M[i][j] = (R_gt t_S)[i] + t_gt[j] - t_est[j], i.e. sqrt(3 |a|^2 + 3 |d|^2 + 2 sum(a) sum(d)) with a = R_gt t_S, d = t_gt - t_est --
 *   sqrt(3) |d| for a class with the identity only, not |d|.  The toolkit's teS / reteS decisions are taken on it, so this is the value computed;
 *   the plain translation error is err[2] of gdrn_pose_errors.  nsym[c] = 0 gives NaN; a NaN in
 *   t_est, t_gt or K gives NaN in te_sym / arp_2d_sym.  Work is spread over (row, slab of GDRN_SIXD_SYM_SLAB transformations), the slabs' minima
 *   are finished in slab order.  workspace: gdrn_sym_errors_workspace_bytes(N, n_max, S_max) bytes, no initialisation.
 *
 * gdrn_score_recall_accumulate: adds a batch (ad_err [N][2] from gdrn_ad_errors, sym_err [N][3] from gdrn_sym_errors) to the caller's per-class
 *   state (device memory, zeroed by the caller before the first call); diameter [C] fp64, ad_is_adi [C] int32 (non-zero: "ad" is adi for the class,
 *   dp_model["symmetric_obj_ids"]).  hits [C][GDRN_SIXD_NFLAGS] += the strict-< decisions (pose_matching.py:68), cm = 100 m:
 *     [0..9] AUCadd: add cm < 1..10 | [10..19] AUCadi: adi | [20..29] AUCad: ad | [30] ABSadd: add cm < 2 | [31] ABSadi | [32] ABSad |
 *     [33..35] add / diameter < 0.02, 0.05, 0.1 | [36..38] adi / diameter | [39..41] reS: re_sym < 2, 5, 10 | [42..44] teS: te_sym cm < 2, 5, 10 |
 *     [45..47] reteS: both at once | [48..50] projS: arp_2d_sym < 2, 5, 10
 *   (eval_calc_scores.py:238-250 divides add and adi by the diameter and nothing else of these);  seen [C] += rows of the class.  One workgroup
 *   per class, integer adds; calls on one stream follow each other. */
#define GDRN_SIXD_AD_SLAB 1024
#define GDRN_SIXD_AD_TILE 512
#define GDRN_SIXD_SYM_SLAB 8
#define GDRN_SIXD_NFLAGS 51
long long gdrn_ad_errors_workspace_bytes(int N, int n_max);
int gdrn_ad_errors(const double* R_est, const double* t_est, const double* R_gt, const double* t_gt, const int* labels, const int* labels_host,
                   int N, const double* pts, const int* npts, int n_max, int C, double* err, void* workspace, void* stream);
long long gdrn_sym_errors_workspace_bytes(int N, int n_max, int S_max);
int gdrn_sym_errors(const double* R_est, const double* t_est, const double* R_gt, const double* t_gt, const double* K, const int* labels,
                    const int* labels_host, int N, const double* pts, const int* npts, int n_max, const double* sym_R, const double* sym_t,
                    const int* nsym, int S_max, int C, double* err, void* workspace, void* stream);
int gdrn_score_recall_accumulate(const double* ad_err, const double* sym_err, const int* labels, const int* labels_host, int N,
                                 const double* diameter, const int* ad_is_adi, int C, long long* hits, long long* seen, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Background replacement and colour augmentation of whole training frames (added within ABI 5: new entry points, nothing changed): what the
 * reference does per sample on the host between decoding and cropping -- replace_bg / get_bg_image (core/base_data_loader.py:320-403,
 * resize_short_edge core/utils/data_utils.py:161-187) and the imgaug chain of INPUT.COLOR_AUG_CODE (core/gdrn_modeling/data_loader.py:319-343) --
 * for a batch of frames of any sizes per call.  Every random decision is made by the caller and arrives in the task; the kernels are deterministic.
 *
 * One gdrn_aug_task per frame, the same table twice: as a device array for the kernels and as a host array for the argument checks.  Frames are
 * u8 [H][W][3].  The stages, in this order, on the full frame:
 *   background   (mask != NULL) the top-left ch x cw crop of the bank image bg (u8, rows of bg_w pixels) resized by 1 / inv_scale with cv2's 8-bit
 *                bilinear rule, sampled per pixel: f = (float)((x + 0.5) inv_scale - 0.5), s = floor(f), f -= s; s < 0 -> s = 0, f = 0; s >= cw - 1 ->
 *                s = cw - 1, f = 0; second tap clamped to cw - 1; a0 = rint((1.f - f) 2048), a1 = rint(f 2048); the same in y (ch; b0, b1);
 *                S_r = p[r][s] a0 + p[r][s + 1] a1 (int32); value = (((b0 (S_0 >> 4)) >> 16) + ((b1 (S_1 >> 4)) >> 16) + 2) >> 2.  Pixels with
 *                y >= oh or x >= ow are 0 (oh <= H, ow <= W: the caller's rounding of the resized size).
 *   cut          gdrn_aug_mask_cuts finds the inclusive bounds r_min, r_max, c_min, c_max of mask != 0 and with c_h = 0.5 (r_min + r_max),
 *                c_w = 0.5 (c_min + c_max) in fp64 and u = trunc_u clears, by trunc_mode: 0 rows < int(r_min + (c_h - r_min) u);  1 rows >=
 *                int(c_h + (r_max - c_h) u);  2 columns < int(c_min + (c_w - c_min) u);  3 columns >= int(c_w + (c_max - c_w) u);  4 nothing.
 *                cuts [B][4] int32 = the kept half-open ranges (row_lo, row_hi, col_lo, col_hi); an empty mask keeps nothing (0, 0, 0, 0).
 *   composite    mask_trunc = mask != 0 inside the kept ranges (written as 0 / 1 when mask_trunc != NULL);  v = mask_trunc ? frame : background
 *   dropout      (gh > 0) pixel (y, x) belongs to cell (min(floor(y gh / H), gh - 1), min(floor(x gw / W), gw - 1)) (fp64); a cell whose byte in
 *                the keep grid aux[keep_off ...] ([gh][gw] u8) is 0 becomes 0 in all channels.  gh gw <= GDRN_AUG_MAX_CELLS.
 *   blur         (blur_r in 1 .. GDRN_AUG_MAX_RADIUS; H, W > blur_r) separable, weights blur_w[0 .. 2 blur_r] fp32, reflect-101 borders, horizontal
 *                then vertical in fp32, taps accumulated left to right / top to bottom (acc = w0 p0; acc = acc + w1 p1; ... every product and sum
 *                rounded on its own), no rounding between the passes, then rint (half to even) and a clamp to 0 .. 255.
 *   table        (lut_off >= 0) out = aux[lut_off + c 256 + v] per channel c: the frame's point operations composed by the caller.
 * aux: one device byte array of aux_bytes holding every keep grid and table of the batch; keep_off / lut_off are byte offsets into it, -1 = none.
 * gdrn_aug_mask_cuts: one workgroup per frame, frames with mask == NULL are left alone.  gdrn_aug_frames: one workgroup per 32 x 32 output tile,
 *   the grid sized by the largest frame; reads cuts for frames with a mask (so it follows gdrn_aug_mask_cuts on the stream).
 * Status: GDRN_ERR_ARG for a NULL table / B <= 0 / a task with a missing pointer, a non-positive size, a crop outside its bank image, an offset
 *   outside aux, a mode outside 0..4 or a frame side <= blur_r;  GDRN_ERR_SHAPE for a radius above GDRN_AUG_MAX_RADIUS, a grid above
 *   GDRN_AUG_MAX_CELLS or B > 65535.  Checked on the host table before anything is launched; neither call allocates or reads anything back. */
#define GDRN_AUG_MAX_CELLS 4096
#define GDRN_AUG_MAX_RADIUS 4
typedef struct gdrn_aug_task {
    const unsigned char* frame;      /* [H][W][3] u8 */
    const unsigned char* mask;       /* [H][W] u8, any non-zero = foreground; NULL: the background stays */
    const unsigned char* bg;         /* bank image, u8 rows of bg_w pixels x 3 (with mask) */
    unsigned char* out;              /* [H][W][3] u8 */
    unsigned char* mask_trunc;       /* [H][W] u8 0 / 1, or NULL */
    double inv_scale;                /* 1 / s of the background resize */
    double trunc_u;
    int H, W;
    int bg_h, bg_w, ch, cw, oh, ow;  /* bank image size, crop size, resized size clamped to the frame */
    int trunc_mode;                  /* 0 .. 4 */
    int gh, gw, keep_off;            /* dropout grid, 0 / 0 / -1 = none */
    int lut_off;                     /* -1 = none */
    int blur_r;                      /* 0 = none */
    float blur_w[9];
} gdrn_aug_task;
int gdrn_aug_mask_cuts(const gdrn_aug_task* tasks_dev, const gdrn_aug_task* tasks_host, int B, int* cuts, void* stream);
int gdrn_aug_frames(const gdrn_aug_task* tasks_dev, const gdrn_aug_task* tasks_host, int B, const unsigned char* aux, long long aux_bytes,
                    const int* cuts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * COCO run-length masks, decoded and encoded on the device (added within ABI 5: new entry points, nothing changed): what the reference does per
 * sample on the host with pycocotools -- cocosegm2mask / rle2mask (lib/utils/mask_utils.py:93-125; core/gdrn_modeling/data_loader.py:79,326,332),
 * binary_mask_to_rle (mask_utils.py:54-66; gdrn_evaluator.py:695-697) and mask2bbox_xyxy (mask_utils.py:39-44) -- for a batch of masks of any
 * sizes per call.  Everything is integer and exact.
 *
 * The format is maskApi's.  An h x w mask is scanned column-major (p = x h + y); counts are the lengths of the alternating runs, the first a run of
 * zeros (of length 0 when pixel (0, 0) is set; zero-length runs may occur anywhere in an input).  The string stores counts[i] for i <= 2 and
 * counts[i] - counts[i - 2] behind, each value least-significant first in 5-bit groups as the character 48 + group, bit 0x20 = another group
 * follows; the last group is the first at which the remaining value (arithmetic shifts) is 0 with bit 0x10 clear or -1 with bit 0x10 set, and on
 * reading a last group with bit 0x10 set sign-extends the value.  counts are uint32 (sums wrap as maskApi's do); h w < 2^31.
 *
 * One gdrn_rle_task per mask, the same table twice: as a device array for the kernels and as a host array for the argument checks.
 * gdrn_rle_decode: strings (strings_bytes of them; a mask's string is str_len characters at str_off) -> mask [h][w] u8 0 / 1, contiguous (sx = 1,
 *   sy = w).  run_ends: workspace of run_cap int32, a mask's run ends (clamped to h w) at run_off, room for str_len of them;  nruns [N] int32 and
 *   totals [N] int64 (the unclamped sum of a mask's counts: the caller may compare it with h w) are outputs.  Whatever the string says, nothing is
 *   written outside the h w bytes of a mask: pixels behind the last run are 0, runs behind h w are dropped.  Two launches: one workgroup per mask
 *   (parse), one per 64 x 64 tile (fill).
 * gdrn_rle_count: mask (any non-zero = foreground; byte strides sy between rows, sx between pixels) -> the transition count of every (column,
 *   16-row segment) in seg_counts (seg_cap int32; a mask's w ceil(h / 16) counts at seg_off, column-major; NULL: not wanted) and area [N] int32,
 *   bbox [N][4] int32 = x_min, y_min, x_max, y_max inclusive, an empty mask 0, 0, w - 1, h - 1 as gdrn_xyz_from_depth writes it (both NULL: not
 *   wanted).  A transition is a pixel that differs from its predecessor in scan order, pixel (0, 0) from 0.
 * gdrn_rle_positions: follows gdrn_rle_count on the stream: scans seg_counts in place (exclusive, scan order), writes ntrans [N] int32 and the
 *   scan-order index of every transition, ascending, to positions (pos_cap int32; a mask's at run_off, room for h w + 1).
 * gdrn_rle_string: positions -> the canonical string of rleEncode + rleToString (counts[0] = positions[0], which is 0 when pixel (0, 0) is set;
 *   counts[i] = positions[i] - positions[i - 1]; the last run ends at h w).  With str_offsets == NULL it writes lengths [N] int64 only; with
 *   str_offsets [N + 1] int64 (device) it writes mask n's characters at strings + str_offsets[n], never past str_offsets[n + 1] or strings_bytes.
 * Status: GDRN_ERR_ARG for a NULL table / N <= 0 / a missing pointer, a task with mask == NULL, a non-positive size, a range outside its buffer
 *   or (decode) a strided mask;  GDRN_ERR_SHAPE for h w >= 2^31 or N > 65535.  Checked on the host table before anything is launched; no call
 *   allocates or reads anything back. */
typedef struct gdrn_rle_task {
    unsigned char* mask;             /* decode: out [h][w] u8;  encode: in, read only */
    long long sy, sx;                /* byte strides of mask (decode: w, 1) */
    long long str_off;               /* decode: first character in strings */
    long long run_off;               /* decode: first run end in run_ends;  encode: first entry in positions */
    long long seg_off;               /* encode: first entry in seg_counts */
    int str_len;                     /* decode */
    int h, w;
    int pad_;
} gdrn_rle_task;
int gdrn_rle_decode(const gdrn_rle_task* tasks_dev, const gdrn_rle_task* tasks_host, int N, const unsigned char* strings, long long strings_bytes,
                    int* run_ends, long long run_cap, int* nruns, long long* totals, void* stream);
int gdrn_rle_count(const gdrn_rle_task* tasks_dev, const gdrn_rle_task* tasks_host, int N, int* seg_counts, long long seg_cap, int* area, int* bbox,
                   void* stream);
int gdrn_rle_positions(const gdrn_rle_task* tasks_dev, const gdrn_rle_task* tasks_host, int N, int* seg_counts, long long seg_cap, int* ntrans,
                       int* positions, long long pos_cap, void* stream);
int gdrn_rle_string(const gdrn_rle_task* tasks_dev, const gdrn_rle_task* tasks_host, int N, const int* ntrans, const int* positions,
                    long long pos_cap, const long long* str_offsets, unsigned char* strings, long long strings_bytes, long long* lengths,
                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * Model preparation on the device (added within ABI 5: new entry points, nothing changed): the per-object tables the data-side and evaluation-side
 * modules take -- extents and 3D box (core/gdrn_modeling/data_loader.py:243-276, misc.get_bbox3d_and_center, lib/pysixd/misc.py:982-1030),
 * farthest-point-sampling (FPS) points (sample_farthest_points_init_center, core/csrc/fps/src/farthest_point_sampling.cpp:122-160, what
 * fps_points.pkl holds) and diameters (misc.calc_pts_diameter, misc.py:952-966) -- for all C objects per call.
 *   pts [C][n_max][3] fp64 with npts [C] int32 valid rows each (device; the rows behind are never read), npts_host the same C values in host
 *   memory: the arguments are checked on them before anything is launched.
 * gdrn_model_bounds: bounds [C][9] fp64 = per-axis minimum, maximum (both exact) and mean (sum in a fixed order, divided by the count).
 * gdrn_model_fps: idx [C][K] int32 = the reference's index sequence with init_center, bit for bit: the vertices rounded to fp32 (nearest even),
 *   the first index the point farthest from (max + min) * 0.5f of the fp32 box, then K - 1 times the point whose minimum squared distance
 *   (dx dx + dy dy) + dz dz (fp32, every operation rounded) to the indices so far is largest; among equal maxima the lowest index, and index 0
 *   when no distance is above 0 (K beyond the number of distinct points).  The sequence for K is a prefix of the one for any larger K.
 *   xyz [C][K][3] fp64 (may be NULL) = the fp32-rounded vertices at idx.  One workgroup per object, one launch.  workspace:
 *   gdrn_model_prep_workspace_bytes(C, n_max, K) bytes of 16-byte aligned device memory, no initialisation needed (0 bytes: may be NULL).
 * gdrn_model_diameter: max_sq [C] fp64 = the maximum over all pairs of an object's points of (dx dx + dy dy) + dz dz in fp64, every operation
 *   rounded; the diameter is its sqrt.  A maximum: the same bits for any pair order.
 * Status: GDRN_ERR_ARG for a NULL pointer, C < 1, n_max < 1, a point count outside [1, n_max], K < 1 or a missing / misaligned workspace;
 *   GDRN_ERR_SHAPE for n_max * 3 >= 2^31, C > 65535 or (diameter) 2^32 threads and more in the launch.  No call allocates or reads anything back. */
long long gdrn_model_prep_workspace_bytes(int C, int n_max, int K);
int gdrn_model_bounds(const double* pts, const int* npts, const int* npts_host, int C, int n_max, double* bounds, void* stream);
int gdrn_model_fps(const double* pts, const int* npts, const int* npts_host, int C, int n_max, int K, int* idx, double* xyz, void* workspace,
                   void* stream);
int gdrn_model_diameter(const double* pts, const int* npts, const int* npts_host, int C, int n_max, double* max_sq, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Scene ground truth on the device (added within ABI 5: new entry points, nothing changed): the per-instance annotations the BOP toolkit writes in
 * an offline pass and every dataset file reads (core/gdrn_modeling/datasets/lm_pbr.py:143-178) -- mask, mask_visib and the records of
 * scene_gt_info.json -- from depth renders that are already on the device, for N instances in F frames per call.  Units: metres and pixels.
 * Counts are integers, bounds integer minima / maxima: no floating-point atomics, repeated calls give the same bits, and a row's result does not
 * depend on the other rows of the call (composed scene depth apart, which is a minimum over the frame's rows and so independent of their order).
 *
 * gdrn_scene_gt_canvas: canvas [N][H + 2 pad_y][W + 2 pad_x] fp32, the instance rendered with a margin round the image (gdrn_render_depth with
 *   cx + pad_x, cy + pad_y; 0 = nothing); the image is the central H x W window.  depth [N][H][W] = the window, copied;  px_count_all [N] = the
 *   canvas pixels != 0;  bbox_obj [N][4] = the inclusive bounds x1, y1, x2, y2 of those pixels in IMAGE coordinates (negative / beyond W - 1,
 *   H - 1 outside the image), left as a running minimum / maximum for gdrn_scene_gt_visibility to finish.  Counters are cleared inside the call.
 * gdrn_scene_gt_compose: depth_scene [F][H][W] = per frame and pixel the smallest non-zero value of depth [N][H][W] over the frame's instances
 *   inst[inst_off[f] .. inst_off[f + 1]) (a CSR table: inst_off [F + 1], inst [N], int32, device, with host copies that are checked: inst_off_host
 *   starts at 0, does not decrease and ends at N, every inst_host within [0, N)); 0 where none has a value and for a frame without instances.
 * gdrn_scene_gt_visibility: depth [N][H][W] as written by gdrn_scene_gt_canvas;  depth_scene [F][H][W] fp32 (0 = no measurement);  frame [N] and
 *   frame_host as in gdrn_vsd;  K [N][3][3] fp64 of the IMAGE, read as fx, cx, fy, cy (no skew), as in gdrn_vsd.  Per pixel of the window:
 *     mask       = depth != 0
 *     dist       = sqrt((X d)^2 + (Y d)^2 + d^2) in fp64 for d = depth and d = depth_scene[frame] (misc.depth_im_to_dist_im_fast, as in gdrn_vsd)
 *     mask_visib = GDRN_VISIB_BOP19: ((float)dist_gt - (float)dist_scene <= (float)delta  or  dist_scene == 0)  and  dist_gt > 0
 *                  GDRN_VISIB_BOP18: dist_gt > 0  and  dist_scene > 0  and  (float)dist_gt - (float)dist_scene <= (float)delta
 *                  (visibility._estimate_visib_mask, lib/pysixd/visibility.py:29-36)
 *   mask, mask_visib [N][H][W] u8 (0 / 1);  px_count_valid [N] = mask and depth_scene > 0;  px_count_visib [N] = mask_visib;  bbox_visib [N][4] =
 *   the inclusive bounds of mask_visib;  then, per instance, with px_count_all and bbox_obj of gdrn_scene_gt_canvas (same stream): a box without
 *   pixels becomes (0, 0, -1, -1);  visib_fract [N] fp64 = px_count_visib / px_count_all as one fp64 division, 0.0 when px_count_all == 0.
 * Status: GDRN_ERR_ARG for a NULL pointer, N / F / H / W < 1, a negative margin, a side or margin above 2^20, a frame or CSR entry out of range, a
 *   negative or NaN delta or an unknown mode;  GDRN_ERR_SHAPE for a canvas of 2^31 - 2048 pixels and more or N / F > 65535.  Everything is checked
 *   on the host before a stream or a device pointer is touched.  No call allocates or reads anything back. */
enum { GDRN_VISIB_BOP19 = 0, GDRN_VISIB_BOP18 = 1 };
int gdrn_scene_gt_canvas(const float* canvas, int N, int H, int W, int pad_x, int pad_y, float* depth, int* px_count_all, int* bbox_obj,
                         void* stream);
int gdrn_scene_gt_compose(const float* depth, const int* inst_off, const int* inst_off_host, const int* inst, const int* inst_host, int F, int N,
                          int H, int W, float* depth_scene, void* stream);
int gdrn_scene_gt_visibility(const float* depth, const float* depth_scene, const int* frame, const int* frame_host, int F, const double* K, int N,
                             int H, int W, double delta, int visib_mode, unsigned char* mask, unsigned char* mask_visib, const int* px_count_all,
                             int* px_count_valid, int* px_count_visib, int* bbox_obj, int* bbox_visib, double* visib_fract, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Shaded colour frames of posed meshes (added within ABI 5: new entry points, nothing changed): what the reference draws with
 * lib/meshrenderer/meshrenderer_phong.py (render, render_many) and shader/depth_shader_phong.{vs,frag} -- vertex-colour Phong shading and a z-test
 * between several posed objects in one image -- for N instances in F frames per call, in two passes.  Mesh table, labels, R, t, K as for
 * gdrn_render_depth; normals and colors [sum nverts][3] fp64, packed like verts (unit normals in model coordinates, colours in [0, 1]).
 *
 * gdrn_render_visibility: the arguments and EVERY rule of gdrn_render_depth (rays, coverage, fp64 arithmetic, the one rounding to fp32, dropped
 *   geometry, both windings, the frame): the same fragment code with another store.  vis [N][H][W] uint64:
 *     key = (bits of the fp32 depth << 32) | face index within the class;   ~0 where nothing is drawn
 *   The smallest key wins (one 64-bit unsigned atomic min per fragment): the nearest fp32 depth and, among equal depths, the lowest face index.
 *   The upper halves are bit for bit what gdrn_render_depth writes for the same inputs (0xffffffff where it writes 0).
 * gdrn_shade_frames: one thread per frame pixel (x, y) of frame f; the instances of the frame are inst[inst_off[f] .. inst_off[f + 1]), the CSR
 *   table of gdrn_scene_gt_compose with its host copies, checked the same way.  light [F][3] fp64: the light's position in camera coordinates
 *   (OpenCV convention: x right, y down, z forward; metres);  phong [F][3] fp64 = (ambient, diffuse, specular) weights;  background (nullable)
 *   [F][H][W][3] u8.  Everything below is fp64, contraction off:
 *     instance       among the frame's instances the smallest fp32 depth (upper half of the key); equal depths go to the first in input order
 *     geometry       the winning face's camera-space vertices a, b, c (vertex indices sorted ascending) as the rasterizer computes them, the
 *                    pixel's ray d, z = (n.a) / (n.d) in fp64 (NOT the fp32 depth), P = z d
 *     interpolation  perspective-correct, from the rasterizer's own edge values: the weight of a = d.(b x c), of b = d.(c x a), of c = d.(a x b),
 *                    each divided by the sum of the three; colour and normal are interpolated with them
 *     lighting       N = normalize(R n_interp), the zero vector if its length is 0;  L = normalize(light - P);  V = normalize(-P);
 *                    diff = max(N.L, 0);  Rv = 2 (N.L) N - L;  spec = max(Rv.V, 0), not gated on N.L > 0 (depth_shader_phong.frag:20-26);
 *                    rgb_k = min(1, (ambient + diffuse diff + specular spec) c_k)  (:29-35);  q_k = floor(255 rgb_k + 0.5)
 *   rgb [F][H][W][3] u8 in the channel order of the colour table;  depth [F][H][W] fp32, the winning key's upper half, 0 where nothing is drawn;
 *   index [F][H][W] int32 = the winning instance's row in the batch, -1 where nothing is drawn;  face (nullable) [F][H][W] int32, the winning
 *   face, -1 where nothing is drawn;  normal_map (nullable) [F][H][W][3] u8 = floor(255 (0.5 N + 0.5) + 0.5) (depth_shader_phong.frag:36), 0
 *   where nothing is drawn.  Where nothing is drawn rgb is the background's pixel, 0 without one; a frame without instances is its background.
 *   A key whose face lies outside the table (not written by gdrn_render_visibility) counts as nothing drawn.
 *   rgb, normal_map and background are 4-byte aligned: the 3-byte maps move as aligned dwords, three lanes of four one dword each.
 *   N == 0 is allowed (every frame is its background; the per-instance pointers are then not read).
 * Status: GDRN_ERR_ARG for a NULL pointer that is not nullable, F / H / W / C < 1, N < 0, a label or CSR entry out of range, a misaligned byte
 *   map;  GDRN_ERR_SHAPE for H * W or the workgroup count beyond an int.  Everything is checked on the host before the launch.  Neither call
 *   needs scratch memory beyond vis or reads anything back; no floating-point atomics, repeated calls give the same bits. */
int gdrn_render_visibility(const double* verts, const int* faces, const int* vert_off, const int* nverts, const int* face_off, const int* nfaces,
                           int C, int f_max, const int* labels, const int* labels_host, const double* R, const double* t, const double* K, int N,
                           int H, int W, double near, double far, unsigned long long* vis, void* stream);
int gdrn_shade_frames(const unsigned long long* vis, const double* verts, const int* faces, const int* vert_off, const int* nverts,
                      const int* face_off, const int* nfaces, const double* normals, const double* colors, int C, const int* labels,
                      const int* labels_host, const double* R, const double* t, const double* K, const int* inst_off, const int* inst_off_host,
                      const int* inst, const int* inst_host, int F, int N, int H, int W, const double* light, const double* phong,
                      const unsigned char* background, unsigned char* rgb, float* depth, int* index, int* face, unsigned char* normal_map,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * Textured and flat-shaded frames with the BOP renderer's light model (added within ABI 5: a new entry point, nothing changed): what the reference
 * draws with lib/pysixd/renderer_py.py (renderer.create_renderer(..., mode="rgb")) -- a UV texture map instead of vertex colours where the model
 * has one, Phong or flat shading, light_w = min(1, ambient_w + max(L.N, 0)) without a specular term, np.round as the last step.
 *
 * gdrn_shade_frames_tex: the second pass of gdrn_shade_frames with another shading rule: the same arguments, the same launch (one thread per frame
 *   pixel), the same CSR table and host copies, and in addition
 *     uvs [sum nverts][2] fp64, packed like verts: the texture coordinates of every vertex (zeros for a class without a texture);
 *     texels [n_texels] uint32, one texel per dword as c0 | c1 << 8 | c2 << 16 in the channel order given (that of the colour table), the rows of
 *       a texture in FILE order: row 0 = the top of the image.  One texel is one aligned 4-byte load; nullable when n_texels == 0;
 *     tex [C][3] int32 = (offset into texels, h, w) per class, h == 0: the class has no texture;  tex_host: its host copy, checked before the
 *       launch: offset >= 0, offset + h w <= n_texels, h and w both 0 or both in [1, GDRN_TEX_MAX_SIDE];
 *     ambient [F] fp64, the ambient weight per frame;  light [F][3] fp64 as for gdrn_shade_frames (the reference's default: the camera origin);
 *     shading: GDRN_SHADING_PHONG or GDRN_SHADING_FLAT;  filter: GDRN_TEXFILTER_NEAREST or GDRN_TEXFILTER_BILINEAR; both uniform per call.
 *   Per pixel, everything fp64, contraction off, every fused operation an explicit fma():
 *     instance, geometry, weights   exactly those of gdrn_shade_frames (the same device functions): depth, index and face of the two entry points
 *                    are bit-identical on the same vis.  wa, wb, wc: the weights of a, b, c;  n = (b - a) x (c - a) of the sorted vertices, d the ray
 *     uv             u = fma(wa, u_a, fma(wb, u_b, wc u_c)), v likewise: the nesting of the interpolated colour
 *     normal N       GDRN_SHADING_PHONG: normalize(R n_interp), as gdrn_shade_frames.  GDRN_SHADING_FLAT: normalize(n) of the camera-space face
 *                    normal, negated when n.d > 0 so that it faces the camera (N.d <= 0) -- what cross(dFdx(v_eye_pos), dFdy(v_eye_pos)) gives
 *                    for either winding (renderer_py.py:66).  The zero vector if the length is 0.
 *     light          L = normalize(light - P);  diff = max(N.L, 0);  lw = min(1, ambient + diff)   (renderer_py.py:94-96)
 *     base colour    a class with a texture: the sampled texel / 255, vertex colours ignored (renderer_py.py:98-99); otherwise the interpolated
 *                    vertex colour fma(wa, c_a, fma(wb, c_b, wc c_c))
 *     nearest        i = clamp(floor(u w), 0, w - 1), j = clamp(floor(v h), 0, h - 1), the texel of file row h - 1 - j, column i:
 *                    v = 0 is the bottom row (the reference flips the image before the upload) and coordinates outside [0, 1] take the edge
 *                    texel (GL's clamp-to-edge).  The clamp is done in fp64 before the conversion to int: no |u| overflows it
 *     bilinear       x = u w - 0.5 (a product and a difference, not fused), i0 = floor(x), fx = x - i0, columns clamp(i0) and clamp(i0 + 1) in
 *                    [0, w - 1]; y = v h - 0.5, j0, fy and the rows h - 1 - clamp(j0), h - 1 - clamp(j0 + 1) likewise (clamp-to-edge); per channel
 *                    on the byte values  lo = fma(fx, t10 - t00, t00), hi = fma(fx, t11 - t01, t01), c = fma(fy, hi - lo, lo) / 255
 *                    (t00 = row of j0, column i0; t10 = row of j0, column i0 + 1; t01, t11 = the row of j0 + 1): x first, then y.  No mipmaps
 *     output         q_k = rint(255 (lw c_k)), round-half-to-even (np.round, renderer_py.py:506), clamped into the byte -- NOT the
 *                    floor(255 rgb_k + 0.5) of gdrn_shade_frames
 *   normal_map reports the N that was used, quantised as gdrn_shade_frames does: floor(255 (0.5 N + 0.5) + 0.5).  rgb, depth, index, face, the
 *   background, empty pixels and frames, N == 0, the 4-byte alignment of the byte maps: as gdrn_shade_frames.
 * Status: as gdrn_shade_frames, and GDRN_ERR_ARG for uvs, tex or tex_host NULL, texels NULL with n_texels > 0, n_texels < 0, a tex_host row that
 *   breaks the rule above, an unknown shading or filter.  Everything is checked on the host before a stream or a device pointer is touched.  No
 *   scratch memory, no atomics, no read-back: repeated calls give the same bits. */
enum { GDRN_SHADING_PHONG = 0, GDRN_SHADING_FLAT = 1 };
enum { GDRN_TEXFILTER_NEAREST = 0, GDRN_TEXFILTER_BILINEAR = 1 };
enum { GDRN_TEX_MAX_SIDE = 16384 };
int gdrn_shade_frames_tex(const unsigned long long* vis, const double* verts, const int* faces, const int* vert_off, const int* nverts,
                          const int* face_off, const int* nfaces, const double* normals, const double* colors, const double* uvs,
                          const unsigned int* texels, const int* tex, const int* tex_host, int n_texels, int C, const int* labels,
                          const int* labels_host, const double* R, const double* t, const double* K, const int* inst_off, const int* inst_off_host,
                          const int* inst, const int* inst_host, int F, int N, int H, int W, const double* light, const double* ambient, int shading,
                          int filter, const unsigned char* background, unsigned char* rgb, float* depth, int* index, int* face,
                          unsigned char* normal_map, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Complement-over-union pose errors on the device (added within ABI 5: new entry points, nothing changed): the error types cus, cou_mask, cou_bb
 * and cou_bb_proj of lib/pysixd/pose_error.py:466-589 for N estimates per call.  Counts and bounds are integers, reduced with integer atomics
 * only: the result does not depend on the launch shape or on any order, repeated calls give the same bits, and a row's result does not depend on
 * the other rows of the call.
 *
 * gdrn_cou_maps: est, gt [N][H][W], the silhouette under the estimated and the ground-truth pose, both of the element kind `kind`:
 *     GDRN_COU_DEPTH  fp32 (gdrn_render_depth's maps or any other): a pixel is covered iff value > 0 as IEEE compares fp32 -- NaN, -0.0, 0.0 and
 *                     negatives are not covered, +inf and subnormals are.  Decided on the bit pattern (0x00000001 .. 0x7f800000): no denormal
 *                     mode enters.  (pose_error.cus: depth > 0)
 *     GDRN_COU_MASK   one byte per pixel (uint8 or bool storage): covered iff the byte is non-zero.  (pose_error.cou_mask: astype(bool))
 *   Each map is read once; no alignment of the base pointers, of H * W or of W is assumed.  Per row i:
 *     counts [N][2] int32  = |est and gt|, |est or gt|
 *     boxes  [N][2][4] int32 = the inclusive bounds x1, y1, x2, y2 of est, then of gt;  an EMPTY silhouette is (0, 0, -1, -1), as
 *                     gdrn_scene_gt_visibility writes it
 *     err    [N][2] fp64, contraction off:
 *       err[i][0] = union > 0 ? 1.0 - (double)inter / (double)union : 1.0                     (cus / cou_mask, pose_error.py:479-484, :526-531)
 *       err[i][1] = 1.0 - iou(xywh(est box), xywh(gt box)),  xywh = x1, y1, x2 - x1 + 1, y2 - y1 + 1   (cou_bb_proj as it is meant:
 *                   misc.calc_2d_bbox_xywh(clip=False) + misc.iou);  1.0 if either silhouette is empty
 *     iou(a, b) is misc.iou (lib/pysixd/misc.py:809-836) operation for operation in fp64: corners x + w, y + h; w_inter = min of the right corners -
 *       max of the left ones, h_inter likewise; the intersection counts only when w_inter > 0 and h_inter > 0; then
 *       (w_inter h_inter) / ((w_a h_a + w_b h_b) - w_inter h_inter), otherwise 0.  A NaN in either box gives 0.
 *   workspace: gdrn_cou_maps_workspace_bytes(N) bytes of device memory (ten int32 per row), 4-byte aligned, no initialisation needed.
 * gdrn_cou_bb: err [N] fp64 = 1.0 - iou(bb_est[i], bb_gt[i]) of N pairs of fp64 x, y, w, h boxes [N][4] (pose_error.cou_bb), one thread per pair.
 * Status: GDRN_ERR_ARG for an unknown kind, N < 0, H or W < 1, H * W of 2^31 - 2048 and more, or (N > 0) a NULL pointer;  GDRN_ERR_SHAPE for
 *   N * ceil(H W / 2048) beyond an int.  Everything is checked on the host before a stream or a device pointer is touched.  N == 0 launches
 *   nothing and succeeds.  gdrn_cou_maps_workspace_bytes: GDRN_ERR_ARG for N < 0.  No call allocates or reads anything back. */
enum { GDRN_COU_DEPTH = 0, GDRN_COU_MASK = 1 };
long long gdrn_cou_maps_workspace_bytes(int N);
int gdrn_cou_maps(const void* est, const void* gt, int kind, int N, int H, int W, double* err, int* counts, int* boxes, void* workspace,
                  void* stream);
int gdrn_cou_bb(const double* bb_est, const double* bb_gt, int N, double* err, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depth refinement of estimated poses on the device (added within ABI 5: new entry points, nothing changed): projective point-to-plane ICP of N
 * estimates against observed depth frames, the usual last step of an RGB-D entry before scoring.  The reference is RGB-only and has no
 * counterpart; like the PnP entry points these are pinned to geometry and to an fp64 host restatement (tests/icp_host.py).  All arithmetic is
 * fp64, contraction off, on the fp32 depths as stored.  No floating-point atomics: every sum has a fixed order, the same call gives the same
 * bits, and the instances of a batch do not influence each other.
 *
 *   depth_ren   [N][H][W] fp32: the model under the current pose (gdrn_render_depth's map), 0 = nothing drawn
 *   depth_scene [F][H][W] fp32: the observed frames in metres, 0 = no measurement;  frame [N] int32 (device) / frame_host (the same values on
 *               the host, range-checked against F before any launch): the frame of each estimate
 *   K           [N][3][3] fp64, upper triangular, as for gdrn_render_depth
 *
 * rays    d(x, y) = K^-1 [x, y, 1] on integer pixel coordinates, the ray the rasterizer samples (dy = (y - cy) / fy, dx = ((x - sk dy) - cx) / fx,
 *         third component 1);  p = depth_ren[i][y][x] d is the model surface, q = depth_scene[frame[i]][y][x] d the observation.
 * normal  of the observation at (x, y), computed on the fly:  a = q(x+1, y) - q(x-1, y),  b = q(x, y+1) - q(x, y-1),  c = a x b,
 *         n = c / |c|, |c| = sqrt((cx cx + cy cy) + cz cz).  Valid when the pixel is not on the frame's border, all five observed depths
 *         are > 0, each neighbour's depth differs from the centre's by at most normal_gate, and |c| > 0.  The sign of n is immaterial.
 * pair    pixel (x, y) of instance i is a pair when depth_ren > 0, the normal is valid and |depth_scene - depth_ren| <= dist_gate.  (NaN
 *         depths fail every comparison.)
 * system  r = n . (p - q), evaluated as (depth_ren - depth_scene) ((nx dx + ny dy) + nz): the difference of the two fp32 depths is exact in
 *         fp64;  J = [p x n, n] (rotation first);  A = sum J J^T, b = sum J r, sq = sum r^2, pairs = the integer count.
 *         sys [N][28] fp64 = the 21 entries of A's upper triangle row by row (A00 .. A05, A11 .. A15, .., A55), b (6), sq.
 * step    an instance is DEGENERATE when pairs < min_pairs, when a diagonal entry of A is not > 0, or when a pivot of the Cholesky
 *         factorisation of S A S, S = diag(A_ii^-1/2) -- the remainder of a diagonal entry before its square root -- is not >= 1e-9.  It keeps
 *         the pose it had and is frozen.  Otherwise xi = (w, v) solves A xi = -b (through that factorisation) and
 *         R <- exp([w]x) R,  t <- exp([w]x) t + v,  exp by Rodrigues (sin(th) / th and 2 sin^2(th / 2) / th^2), I + [w]x below |w| = 1e-12.
 *         A step with |w| < 1e-10 and |v| < 1e-10 |t| (t before the step) is applied and freezes the instance as CONVERGED.
 *
 * gdrn_icp_accumulate: one accumulation on given renders: sys [N][28] fp64 and pairs [N] int32.  One workgroup per (instance, band of 16
 *   rows) writes its slab into `workspace`; a second launch combines the bands in ascending order.
 * gdrn_icp_step: one solve and update from combined systems.  R [N][3][3], t [N][3] fp64 in/out;  state [N][2] int32 in/out = the status
 *   (GDRN_ICP_RUNNING to start with) and the number of steps applied so far;  an instance that is not RUNNING is left alone.
 * gdrn_icp_refine: the mesh table, labels, near and far exactly as gdrn_render_depth takes them;  R, t in/out.  `iters` times on the one stream:
 *   gdrn_render_depth into depth_ren_scratch [N][H][W] fp32, the accumulate pass, the step -- which combines the slabs in its prologue, with the
 *   operation sequence of gdrn_icp_accumulate's second launch: the same bits.  Nothing is read back.  Outputs, per instance:
 *     ok [N] int32 = 0 iff it was found degenerate;  iters_done [N] int32 = the steps applied;  pairs [N] int32 and rms [N] fp64 =
 *     sqrt(sq / pairs) of the last system accumulated while it was running, i.e. the residual before its last step (NaN when pairs == 0;
 *     iters == 0: ok 1, pairs 0, rms NaN, the pose untouched).
 *   workspace (both calls): gdrn_icp_workspace_bytes(N, H, W) bytes of device memory, 8-byte aligned, no initialisation needed.
 * Status: GDRN_ERR_ARG for N < 0, H or W < 1, H * W of 2^31 - 1024 and more, gates that are not > 0, iters < 0, min_pairs < 6, a label or a frame
 *   out of range, the rasterizer's argument rules, or (N > 0) a NULL pointer or a misaligned workspace;  GDRN_ERR_SHAPE for N > 65535 and the
 *   rasterizer's shape rules.  Everything is checked on the host before a stream or a device pointer is touched;  N == 0 launches nothing. */
enum { GDRN_ICP_RUNNING = 0, GDRN_ICP_CONVERGED = 1, GDRN_ICP_DEGENERATE = 2 };
long long gdrn_icp_workspace_bytes(int N, int H, int W);
int gdrn_icp_accumulate(const float* depth_ren, const float* depth_scene, const int* frame, const int* frame_host, int F, const double* K, int N,
                        int H, int W, double dist_gate, double normal_gate, double* sys, int* pairs, void* workspace, void* stream);
int gdrn_icp_step(const double* sys, const int* pairs, int N, int min_pairs, double* R, double* t, int* state, void* stream);
int gdrn_icp_refine(const double* verts, const int* faces, const int* vert_off, const int* nverts, const int* face_off, const int* nfaces, int C,
                    int f_max, const int* labels, const int* labels_host, double* R, double* t, const double* K, int N, const float* depth_scene,
                    const int* frame, const int* frame_host, int F, int H, int W, double near, double far, int iters, double dist_gate,
                    double normal_gate, int min_pairs, float* depth_ren_scratch, int* ok, int* iters_done, int* pairs, double* rms,
                    void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Coarse depth alignment in front of the refinement above (added within ABI 5: new entry points, nothing changed): every estimate is shifted
 * along its viewing ray by the median difference between the observed and the rendered depth, so that an RGB-only estimate -- centimetres off
 * along the ray -- comes within gdrn_icp_refine's dist_gate.  The reference has no counterpart; the entry points are pinned to geometry and to
 * a host restatement (tests/align_host.py).  The median is an exact order statistic; only integer atomics are used: the same call gives the
 * same bits, and the instances of a batch do not influence each other.
 *
 *   depth_ren, depth_scene, frame, frame_host, F: as above.  For estimate i, ren = depth_ren[i], sc = depth_scene[frame[i]], both [H][W] fp32.
 *
 * pair     pixel p is a pair iff ren[p] > 0, sc[p] > 0 and fabs((double)d) <= gate, d = sc[p] - ren[p] being ONE fp32 subtraction.  (NaN fails
 *          > 0;  +inf gives d = inf, which fails the gate.)
 * counts   covered = the number of pixels with ren > 0;  pairs = n = the number of pairs.
 * few      n < min_pairs:  ok = 0, offset = NaN, the translation is left bit for bit.
 * median   otherwise, with the d of the pairs in ascending order, lo = d[(n - 1) / 2], hi = d[n / 2] (integer division) and
 *          offset = 0.5 * ((double)lo + (double)hi): numpy's median of the widened values, exactly, for odd and even n.  ok = 1.
 * shift    in fp64, no contraction:  s = offset / t_z;  t_x += s * t_x;  t_y += s * t_y;  t_z += offset  (s from t_z before the shift).  The
 *          model origin keeps its image;  R is not touched.
 *
 * gdrn_depth_offset: one evaluation on given maps: offset [N] fp64, pairs, covered, ok [N] int32.  A first launch (one workgroup per instance
 *   and band of 16 rows) appends the order-preserving integer keys of the pairs' differences to a per-instance list in `workspace`, a second
 *   (one workgroup per instance) selects the two ranks by radix selection over integer histograms (11 + 11 + 10 bits), a third writes the outputs.
 * gdrn_depth_align: the mesh table, labels, near and far exactly as gdrn_render_depth takes them;  R read only, t in/out.  `rounds` times on the
 *   one stream (a fixed count, no stop rule): gdrn_render_depth into depth_ren_scratch [N][H][W] fp32 under the current pose, the offset, the
 *   shift.  An instance with ok = 0 in some round is frozen from then on;  ok, pairs, covered, offset are those of the instance's last
 *   evaluated round (rounds == 0: ok 1, pairs 0, covered 0, offset NaN, the translation untouched).  Nothing is read back.
 *   workspace (both calls): gdrn_depth_align_workspace_bytes(N, H, W) bytes of device memory, 8-byte aligned;  every call initialises what it
 *   reads, the caller prepares nothing.
 * Status: GDRN_ERR_ARG for N < 0, H or W < 1, H * W of 2^31 - 1024 and more, a gate that is not > 0, rounds < 0, min_pairs < 1, a label or a
 *   frame out of range, the rasterizer's argument rules, or (N > 0) a NULL pointer or a misaligned workspace;  GDRN_ERR_SHAPE for N > 65535 and
 *   the rasterizer's shape rules.  Everything is checked on the host before a stream or a device pointer is touched;  N == 0 launches nothing. */
long long gdrn_depth_align_workspace_bytes(int N, int H, int W);
int gdrn_depth_offset(const float* depth_ren, const float* depth_scene, const int* frame, const int* frame_host, int F, int N, int H, int W,
                      double gate, int min_pairs, double* offset, int* pairs, int* covered, int* ok, void* workspace, void* stream);
int gdrn_depth_align(const double* verts, const int* faces, const int* vert_off, const int* nverts, const int* face_off, const int* nfaces, int C,
                     int f_max, const int* labels, const int* labels_host, const double* R, double* t, const double* K, int N,
                     const float* depth_scene, const int* frame, const int* frame_host, int F, int H, int W, double near, double far, int rounds,
                     double gate, int min_pairs, float* depth_ren_scratch, int* ok, int* pairs, int* covered, double* offset, void* workspace,
                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * Silhouette term for the depth refinement above (added within ABI 5: new entry points, nothing changed): the contour of the observed instance
 * mask constrains the directions the point-to-plane term cannot see -- a plate slides in its plane, a cube seen on two faces along their
 * common edge, and gdrn_icp_refine marks such rows DEGENERATE.  The reference has no counterpart; the entry points are pinned to geometry, to
 * an exact Euclidean distance transform and to the reference's edge rule (lib/utils/mask_utils.get_edge, bw = 1) through a host restatement
 * (tests/sil_host.py).  The transform is exact in integers; the sums are fp64, contraction off, in the fixed order of the section above; only
 * integer atomics are used: the same call gives the same bits, and the instances of a batch do not influence each other.
 *
 *   mask_obs [N][H][W] uint8: the observed instance mask of each estimate in its frame, nonzero = object.  depth_ren, depth_scene, frame,
 *   frame_host, F, K and the rays d(x, y) as above;  zs = depth_scene[frame[i]], zr = depth_ren[i].
 *
 * observed contour   pixel p with mask_obs[p] != 0 is a contour pixel iff some in-frame 4-neighbour q has mask_obs[q] == 0 (the frame border is
 *           no edge), unless for any such q:  zs[q] > 0 && zs[p] > 0 && zs[q] < zs[p]  (fp32 compares) -- that is an occluder's boundary,
 *           not the object's.
 * transform d2[p] (int32) = the minimum over the contour pixels c of the instance of (cx - px)^2 + (cy - py)^2, exactly;  nearest[p] (int32) =
 *           cy * W + cx of the minimiser with the smallest linear index;  without a contour pixel d2 = INT32_MAX and nearest = -1.
 *           contour [N] int32 = the number of contour pixels.
 * rendered contour   pixel p is on it when zr[p] > 0, some in-frame 4-neighbour has !(zr > 0), and it is not hidden in the observation:
 *           not (zs[p] > 0 && (double)zs[p] < (double)zr[p] - dist_gate).
 * pair      a rendered contour pixel with nearest[p] >= 0 and (double)d2[p] <= sil_gate * sil_gate (sil_gate in pixels, > 0).
 * system    point to ray: the model point must come to lie on the ray of its observed contour pixel c = nearest[p].  z = (double)zr[p], d = d(p),
 *           g = d(c), P = (z dx, z dy, z);  n1 = (1, 0, -gx), n2 = (0, 1, -gy);  r1 = z (dx - gx), r2 = z (dy - gy), in metres;
 *           J_k = [P x n_k, n_k] (rotation first, the cross product written out in full);  A = sum J_1 J_1^T + J_2 J_2^T, b = sum J_1 r1 + J_2 r2,
 *           sq = sum r1^2 + r2^2 (a pixel's k = 1 term before its k = 2 term), pairs = the number of pair pixels;  sys [N][28] as above.
 * combined  entry by entry sys = sys_depth + weight * sys_sil (one multiply, one add), pairs = pairs_depth + pairs_sil;  the DEGENERATE / solve /
 *           update / CONVERGED rules of gdrn_icp_step then apply unchanged.
 *
 * gdrn_sil_contour_transform: d2, nearest [N][H][W] int32 and contour [N] int32 of the masks.  Three launches: the contour bytes, a column
 *   pass (the nearest contour pixel above and below), a row pass (the minimum of (x - x')^2 + g(x')^2 with the row's g in LDS, tiled for any W).
 * gdrn_sil_accumulate: one accumulation on given renders and a given transform: sys [N][28] fp64 and pairs [N] int32.  One workgroup per
 *   (instance, band of 16 rows) writes its slab into `workspace`; a second launch combines the bands in ascending order.
 * gdrn_icp_step_sil: the combined step from combined systems;  R, t, state as for gdrn_icp_step.
 * gdrn_icp_refine_sil: the arguments of gdrn_icp_refine plus mask_obs, sil_weight, sil_gate.  The transform once;  then `iters` times on the
 *   one stream: gdrn_render_depth into depth_ren_scratch, gdrn_icp_accumulate, the silhouette accumulate pass, the combined step -- which
 *   combines the silhouette slabs in its prologue with the operation sequence of gdrn_sil_accumulate's second launch: the same bits.  Nothing
 *   is read back.  Outputs, per instance: ok, iters_done as for gdrn_icp_refine;  pairs and rms = sqrt(sq / pairs) of the depth term,
 *   sil_pairs [N] int32 and sil_rms [N] fp64 = sqrt(sq_sil / pairs_sil) of the silhouette term (metres), all of the last systems accumulated
 *   while the instance was running (NaN without a pair;  iters == 0: ok 1, counts 0, both rms NaN, the pose untouched, nothing but that written).
 *   workspace (all calls): gdrn_sil_workspace_bytes(N, H, W) bytes of device memory, 8-byte aligned, no initialisation needed.
 * Status: the rules of gdrn_icp_refine, and GDRN_ERR_ARG for a sil_gate that is not > 0 or a weight that is not finite and >= 0;
 *   GDRN_ERR_SHAPE for H or W > 16384 (so that d2 fits) and N > 65535.  Everything is checked on the host before a stream or a device pointer
 *   is touched;  N == 0 launches nothing. */
long long gdrn_sil_workspace_bytes(int N, int H, int W);
int gdrn_sil_contour_transform(const unsigned char* mask_obs, const float* depth_scene, const int* frame, const int* frame_host, int F, int N, int H,
                               int W, int* d2, int* nearest, int* contour, void* workspace, void* stream);
int gdrn_sil_accumulate(const float* depth_ren, const float* depth_scene, const int* frame, const int* frame_host, int F, const double* K,
                        const int* d2, const int* nearest, int N, int H, int W, double sil_gate, double dist_gate, double* sys, int* pairs,
                        void* workspace, void* stream);
int gdrn_icp_step_sil(const double* sys_depth, const int* pairs_depth, const double* sys_sil, const int* pairs_sil, double weight, int N,
                      int min_pairs, double* R, double* t, int* state, void* stream);
int gdrn_icp_refine_sil(const double* verts, const int* faces, const int* vert_off, const int* nverts, const int* face_off, const int* nfaces,
                        int C, int f_max, const int* labels, const int* labels_host, double* R, double* t, const double* K, int N,
                        const float* depth_scene, const int* frame, const int* frame_host, int F, const unsigned char* mask_obs, int H, int W,
                        double near, double far, int iters, double dist_gate, double normal_gate, int min_pairs, double sil_weight,
                        double sil_gate, float* depth_ren_scratch, int* ok, int* iters_done, int* pairs, double* rms, int* sil_pairs,
                        double* sil_rms, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pose from depth and object-coordinate maps: batched 3D-3D RANSAC (added within ABI 5: new entry points, nothing changed).  The RGB-D
 * counterpart of gdrn_pnp_ransac: the network's per-pixel model point and the depth frame's camera point of the same pixel are a 3D-3D pair, and
 * the pose follows from such pairs in closed form inside a RANSAC -- no render, no iteration; rotation, lateral position and depth are fixed
 * together, which gives gdrn_depth_align / gdrn_icp_refine a start that is right in all six degrees of freedom.  The reference is RGB-only
 * (WITH_DEPTH = False) and has no counterpart; the entry points are pinned to geometry and to an independent fp64 host restatement
 * (tests/rigid_host.py).  One workgroup per RoI, all pose arithmetic fp64, sums in a fixed order (wave tree, then the waves through LDS), integer
 * atomics on LDS only: the same call gives the same bits, and the RoIs of a batch do not influence each other.  No call allocates or reads
 * anything back.
 *
 * gdrn_backproject_points.  img_pts [N][stride][2] pixels, model_pts [N][stride][3], fp32, and counts [N] int32 on the device: what
 *   gdrn_correspondences writes.  depth [F][H][W] fp32 in metres, 0 = no measurement;  frame [N] int32 (frame_host: the same N values in host
 *   memory, checked against [0, F) before anything is launched);  K [N][3][3] fp64.  Row j < min(max(counts[n], 0), stride) of RoI n, with (u, v)
 *   widened exactly, looks up the NEAREST pixel ix = floor(u + 0.5), iy = floor(v + 0.5) (no bilinear sampling: it would invent depths across
 *   edges) and is VALID iff u, v and its three model coordinates are finite, 0 <= ix < W, 0 <= iy < H, and d = depth[frame[n]][iy][ix] is finite
 *   and > 0.  Its camera point is the point of the ray K^-1 (u, v, 1)^T -- of the correspondence's own (u, v), as PnP uses it, not of the pixel
 *   centre -- whose z is d (a ray without a finite such point is not valid).  A singular or non-finite K[n] makes every row of RoI n invalid.
 *   cam, mod [N][stride][3] fp64: the valid rows of RoI n compacted to the front IN THEIR INPUT ORDER (ballot + prefix scan, no atomics), the
 *   model point widened exactly;  counts_out[n] of them, every row behind them NaN.
 * gdrn_rigid_ransac.  cam, mod as above;  counts [N] int32 ON THE DEVICE ONLY, clamped to [0, stride] on the device: unlike gdrn_pnp_* this call
 *   takes NO host copy of the counts, so that it chains behind gdrn_backproject_points without a read-back.  dist_thr in metres.
 *   Sampling: the draw rule of gdrn_pnp_ransac (the same mix64, the same four multipliers, index = ((x >> 32) * counts[n]) >> 32), keeping the
 *   first 3 distinct indices (a collision advances d; after 64 draws the hypothesis is dropped).
 *   Closed form (the minimal sample and every refit): the proper rotation (det +1, also for a reflected optimum) and the translation minimising
 *   sum |R m + t - c|^2 -- centroids, the cross-covariance S = sum (m - mbar)(c - cbar)^T about them, the rotation as the eigenvector of the
 *   largest eigenvalue of Horn's symmetric 4x4 matrix of S (cyclic Jacobi, a fixed 6 sweeps), t = cbar - R mbar.
 *   Degenerate: with s1 >= s2 >= s3 >= 0 the singular values of S and s = sign(det S), iff s2 + s s3 <= 1e-9 s1 -- evaluated as the gap between
 *   the two largest eigenvalues of the 4x4 being <= 2e-9 s1 (they add up to 2 s1).  Collinear sets and repeated points are degenerate, coplanar
 *   ones (s3 = 0) are not.  1e-9 is a design constant: seven digits above the fp64 rounding of the sums.  A degenerate sample scores 0.
 *   Scoring: inliers are the rows with |R m + t - c|^2 < dist_thr^2, counted as integers.  Selection: the highest count wins, ties go to the
 *   lowest h;  the winner needs >= 3 inliers.  Then, in gdrn_pnp_ransac's order: the closed form on the winner's inliers, the inliers
 *   re-selected under it, the closed form once more.  inlier_mask [N][stride] u8 (or NULL), num_inliers [N] and rms [N] (or NULL; root of the
 *   inliers' mean squared 3D distance, metres) are those of the returned pose.
 *   R [N][3][3], t [N][3] fp64 are in/out: a RoI with fewer than 3 rows, without a non-degenerate hypothesis of >= 3 inliers, with a degenerate
 *   refit, fewer than 3 inliers under a refit or a non-finite result keeps the caller's values bit for bit and gets ok[n] = 0, num_inliers 0, an
 *   all-zero mask and rms NaN;  every other one ok[n] = 1.
 *   workspace: gdrn_rigid_workspace_bytes(N, stride, iters) bytes of device memory, 8-byte aligned, no initialisation needed.
 * gdrn_rigid_fit: the closed form over all counts[n] rows without a gate (the analogue of gdrn_pnp_refine);  rms over all of them.  The same
 *   degeneracy rule;  an unsolved RoI (fewer than 3 rows, degenerate, a non-finite row) keeps the caller's pose, ok 0, rms NaN.  No workspace.
 * Status: GDRN_ERR_ARG for a NULL pointer that is not nullable, N, stride, iters, F, H or W < 1, a dist_thr that is not finite and > 0, a frame
 *   out of range;  GDRN_ERR_SHAPE for H * W or stride * 3 of 2^31 and more.  Checked on the host before anything is launched. */
int gdrn_backproject_points(const float* img_pts, const float* model_pts, const int* counts, const float* depth, const int* frame,
                            const int* frame_host, int F, int H, int W, const double* K, int N, int stride, double* cam, double* mod,
                            int* counts_out, void* stream);
long long gdrn_rigid_workspace_bytes(int N, int stride, int iters);
int gdrn_rigid_ransac(const double* cam, const double* mod, const int* counts, int N, int stride, double dist_thr, int iters,
                      unsigned long long seed, double* R, double* t, int* ok, int* num_inliers, unsigned char* inlier_mask, double* rms,
                      void* workspace, void* stream);
int gdrn_rigid_fit(const double* cam, const double* mod, const int* counts, int N, int stride, double* R, double* t, int* ok, double* rms,
                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * Hypothesis verification behind the refinement above (added within ABI 5: new entry points, nothing changed): how well a candidate pose
 * explains the observed depth frame and the observed instance mask, and which candidate of a detection explains them best.  gdrn_icp_refine's
 * rms covers only the pairs that passed its own gates: a pose that pokes into measured free space, sits off the mask or hides behind a wall
 * can come back with a small one.  The reference is RGB-only and has no counterpart; the entry points are pinned to geometry and to an
 * integer / fp64 host restatement (tests/verify_host.py), bitwise.  The counts are integers and only integer atomics are used: the same call
 * gives the same bits whatever the launch shape, and the candidates of a batch do not influence each other.
 *
 *   depth_ren, depth_scene, frame, frame_host, F: as for gdrn_icp_accumulate.  mask_obs [M][H][W] uint8 (nonzero = object) or NULL: no mask.
 *   mask_index [N] int32 (device) / mask_index_host (the same values on the host, range-checked against M before any launch): the mask of
 *   each candidate, so that the candidates of one detection share one mask;  both NULL: M must equal N and candidate i reads mask i.
 *
 * Per pixel p of candidate i, with zr = depth_ren[i][p], zc = depth_scene[frame[i]][p], m = mask_obs[mask_index[i]][p] != 0 (absent without a mask):
 *   covered   zr > 0 (a NaN is not; +inf is).     usable   zc is finite and zc > 0.     e = (double)zr - (double)zc, exact.
 *   a covered pixel is exactly one of
 *     unknown    not usable                        no measurement
 *     inlier     usable and fabs(e) <= tau         the render agrees with the observation
 *     occluded   usable and e > tau                the observation is nearer: something stands in front
 *     violated   usable and e < -tau               the observation is farther: the model claims a surface in measured free space
 *   visible   covered and not occluded.
 * counts [N][8] int32 = covered, inlier, occluded, violated, unknown, visible, mask_px (pixels with m set, covered or not), inter (pixels that
 *   are visible and have m set);  without a mask mask_px = inter = 0.
 * sum_q  [N] int64 = the sum over the inliers of (long long)floor(fabs(e) * 1048576.0): exact, a power-of-two scaling of an exact difference.
 * score (one thread per candidate, fp64, contraction off, in this order):
 *     tq    = tau * 1048576.0
 *     fit   = (double)inlier - (double)sum_q / tq              truncated-linear: the sum over the inliers of (1 - |e| / tau), quantised
 *     iou   = has_mask ? (uni > 0 ? (double)inter / (double)uni : 0.0) : 1.0,      uni = visible + mask_px - inter (int32)
 *     score = (iou * fit - penalty * (double)violated) / (double)covered
 *     ok    = covered >= min_covered;   ok == 0: score = -inf (nothing above is evaluated)
 *   The score lies in [-penalty, 1].  The denominator is covered, not visible: a candidate hidden behind a surface has no evidence and must
 *   not win.  The mask factor applies to the positive part only: a lower overlap never raises a score.
 * select  per group g in [0, G): among the rows i with group[i] == g, ok[i] != 0 and score[i] == score[i] (not a NaN), the row with the
 *   highest score, -0.0 ranking below +0.0;  ties go to the lowest row index.  best [G] int32 = that row, -1 without one;  best_score [G] fp64 =
 *   its score, -inf without one.
 *
 * gdrn_verify_maps: counts and sum_q of N candidates on given renders.  One workgroup per (candidate, chunk of 2048 pixels): the render and
 *   the mask are streamed over the whole frame, the observed depth is read only where the render is covered;  no alignment of the base
 *   pointers, of H * W or of W is assumed.  workspace: gdrn_verify_workspace_bytes(N, H, W) bytes of device memory, 8-byte aligned;  the call
 *   clears what it needs on the stream, the caller prepares nothing.
 * gdrn_verify_score: score [N] fp64 and ok [N] int32 from counts and sum_q;  has_mask != 0: the counts were taken with a mask.
 * gdrn_verify_select: group [N] int32 (device) / group_host (the same values on the host, range-checked against G before any launch).  Four
 *   small launches: integer atomicMax of the scores' order-preserving 64-bit keys per group (in best_score's own memory), integer atomicMin of
 *   the row index among the rows that hold the maximum.  No workspace.
 * gdrn_verify_poses: the mesh table, labels, near and far exactly as gdrn_render_depth takes them, the leading arguments in the order of
 *   gdrn_icp_refine;  R, t are only read.  On the one stream: gdrn_render_depth into depth_ren_scratch [N][H][W] fp32 (caller-owned), the
 *   counting pass, the score.  Nothing is read back.  The same bits as the three calls one after the other.
 * Status: GDRN_ERR_ARG for N < 0, H or W < 1, H * W of 2^31 - 1024 and more, F or G < 0, tau outside (0, 1] (so that every sum converts to
 *   fp64 exactly), a penalty that is not finite and >= 0, min_covered < 1, a frame, a label, a group or a mask index out of range, a mask with
 *   M < 1, with one copy of its index but not the other, or without an index and M != N, the rasterizer's argument rules, or (N > 0, resp.
 *   G > 0) a NULL pointer or a misaligned workspace;  GDRN_ERR_SHAPE for N > 65535 in gdrn_verify_maps and gdrn_verify_poses, and the
 *   rasterizer's shape rules.  Everything is checked on the host before a stream or a device pointer is touched;  N == 0 launches nothing
 *   (gdrn_verify_select with N == 0 and G > 0 writes -1 and -inf). */
long long gdrn_verify_workspace_bytes(int N, int H, int W);
int gdrn_verify_maps(const float* depth_ren, const float* depth_scene, const int* frame, const int* frame_host, int F,
                     const unsigned char* mask_obs, const int* mask_index, const int* mask_index_host, int M, int N, int H, int W, double tau,
                     int* counts, long long* sum_q, void* workspace, void* stream);
int gdrn_verify_score(const int* counts, const long long* sum_q, int N, int has_mask, double tau, double penalty, int min_covered,
                      double* score, int* ok, void* stream);
int gdrn_verify_select(const double* score, const int* ok, const int* group, const int* group_host, int N, int G, int* best,
                       double* best_score, void* stream);
int gdrn_verify_poses(const double* verts, const int* faces, const int* vert_off, const int* nverts, const int* face_off, const int* nfaces, int C,
                      int f_max, const int* labels, const int* labels_host, const double* R, const double* t, const double* K, int N,
                      const float* depth_scene, const int* frame, const int* frame_host, int F, int H, int W, double near, double far,
                      const unsigned char* mask_obs, const int* mask_index, const int* mask_index_host, int M, double tau, double penalty,
                      int min_covered, float* depth_ren_scratch, int* counts, long long* sum_q, double* score, int* ok, void* workspace,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * Predicted instance masks in the frame (added within ABI 5: new entry points, nothing changed): the link between the mask head's output --
 * gdrn_correspondences ends at a [res][res] probability map in crop coordinates -- and the steps above that take an observed mask in frame
 * coordinates (gdrn_icp_refine_sil, gdrn_verify_maps / _poses, gdrn_cou_maps, gdrn_rle_count).  The reference has no counterpart on the path
 * (its custom evaluator imports another package's paste with another box convention); the entry points are pinned to the arithmetic stated
 * here, to a numpy fp64 restatement (tests/paste_host.py) bitwise, and through it to independent implementations.  Only integer atomics are
 * used: the same call gives the same bits, and the rows of a batch (in the exclusive form: the frames) do not influence each other.
 *
 * gdrn_roi_components: the largest blob of each map.  prob [B][res][res] fp32, 2 <= res <= 64.  A pixel is foreground iff prob > thr (the
 *   strict fp32 comparison of gdrn_correspondences), a non-finite value counting as 0.  Components are 8-connected.  The kept component is the
 *   one with the most pixels; among equals the one that holds the lowest row-major pixel index.
 *     filtered [B][res][res] fp32 = prob where the pixel belongs to the kept component, 0 elsewhere
 *     num_comp [B] int32 = the number of components;  kept_px [B] int32 = the pixels of the kept one (0 for a map without foreground)
 *   One workgroup per map, the labels in LDS: minimum-label propagation with pointer jumping, at most res^2 rounds (an explicit bound: a round
 *   that changes anything retires a root for good, and there are at most res^2 roots).
 *
 * gdrn_roi_paste_masks: B maps into B masks of H x W.  map [B][res][res] fp32;  geom [B][3] fp64 (device) = cx, cy, scale of each row, the
 *   crop's centre in frame pixels and its side;  geom_host: the same values on the host, checked before any launch.  For frame pixel (x, y) of
 *   row n, in fp64 and in this order (contraction off):
 *     k = (double)res / scale
 *     u = ((double)x - cx) * k + 0.5 * res          v = ((double)y - cy) * k + 0.5 * res
 *     the pixel is 0, and nothing is read, unless -1 < u < res and -1 < v < res
 *     u0 = floor(u), fu = u - u0                    v0 = floor(v), fv = v - v0
 *     m00 = map[v0][u0], m01 = map[v0][u0 + 1], m10 = map[v0 + 1][u0], m11 = map[v0 + 1][u0 + 1], widened to fp64;  a tap outside the map,
 *       or a non-finite one, is 0
 *     a = m00 * (1 - fu) + m01 * fu                 b = m10 * (1 - fu) + m11 * fu                 p = a * (1 - fv) + b * fv
 *     mask[n][y][x] = p > (double)thr
 *   This is bilinear sampling of the map with a zero border at the exact inverse of the ideal crop map of get_affine_transform(center, scale,
 *   0, res): crop index res / 2 lies on (cx, cy), integer coordinates are pixel centres.  It is NOT the inverse of the 1 / 1024 fixed-point
 *   walk gdrn_roi_crop_inputs follows for the forward crop (cv2.warpAffine's), which rounds a source position to 1 / 1024 pixel and an interpolation weight to 1 / 32.
 *     mask [B][H][W] uint8, 0 / 1, every byte written
 *     area [B] int32, bbox [B][4] int32 = x1, y1, x2, y2 of the set pixels, bottom-right inclusive;  an empty mask: area 0 and 0, 0, W - 1,
 *       H - 1 -- gdrn_rle_count's convention exactly
 *   Three launches (two of them one thread per row: the clearing and the empty-mask rule of area / bbox).  A lane writes 16-byte vectors where
 *   the mask's first byte is 16-byte aligned, single bytes otherwise.
 *
 * gdrn_roi_paste_exclusive: the same paste, each frame pixel given to at most one row.  frame_host [B] int32: the frame of each row, within
 *   [0, F);  csr [F + 1 + B] int32 (device) / csr_host (the same values on the host): the offsets of the frames followed by the rows of frame
 *   0, of frame 1, ..., each frame's in ascending order -- the call refuses a csr_host that is not exactly that list of frame_host.  Among the
 *   rows of a pixel's frame with p > (double)thr there, the greatest p wins, compared in fp64;  equal p goes to the lowest row.
 *     index [F][H][W] int32 = the winning row, -1 without one
 *     mask [B][H][W] uint8 = 1 where the row won, every byte written;  area, bbox: of these masks, as above
 *   A gather: one lane per 16 frame pixels walks the rows of its frame.  No atomics on values, no workspace.
 *
 * Status: GDRN_ERR_ARG for B < 0, res outside [2, 64], H or W < 1, B * H * W or F * H * W (gdrn_roi_components: B * res * res) of 2^31 and
 *   more, a thr that is not finite and >= 0, a scale that is not finite and > 0, a centre that is not finite, a frame outside [0, F), a
 *   csr_host that does not match frame_host, or (B > 0) a NULL pointer.  Everything is checked on the host before a stream or a device
 *   pointer is touched;  B == 0 succeeds and writes nothing. */
int gdrn_roi_components(const float* prob, int B, int res, float thr, float* filtered, int* num_comp, int* kept_px, void* stream);
int gdrn_roi_paste_masks(const float* map, const double* geom, const double* geom_host, int B, int res, int H, int W, float thr,
                         unsigned char* mask, int* area, int* bbox, void* stream);
int gdrn_roi_paste_exclusive(const float* map, const double* geom, const double* geom_host, const int* frame_host, const int* csr,
                             const int* csr_host, int B, int F, int res, int H, int W, float thr, int* index, unsigned char* mask, int* area,
                             int* bbox, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GDRN_HIP_H */
