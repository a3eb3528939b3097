/* c2m_hip.h -- C ABI of libc2m_hip.so, the MI355X (gfx950) kernel library behind c2m_amd.
 *
 * The reference (PierfrancescoArdino/C2M) has no FFI on this path: its hot path is stock ATen operators called from
 * Python.  Each entry point below therefore names the reference *call site* (file:line under
 * /root/reference/src) whose ATen op chain it replaces; the Python-side binding is the ctypes stub in
 * c2m_amd/_lib.py (shown in INTEGRATION.md).
 *
 * This header is the ONE definition of every signature.  csrc/common.h includes it, so the compiler holds each definition in
 * the .hip files under csrc/ to its prototype, and c2m_amd/_lib.py parses the prototypes below into its ctypes table at import.  Keep them in the
 * form the parser reads -- `int|long c2m_name(type name, ...);`, by-value types int, unsigned, long, float, double (or int32_t,
 * int64_t, uint8_t), anything with a `*` is passed as a pointer -- or the import raises, naming the function.
 *
 * Conventions (every function):
 *   - plain pointers to DEVICE memory, fp32 unless noted, contiguous NCHW / NCTHW; sizes as int / long
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it and never synchronise or allocate;
 *     scratch is caller-provided (`workspace`), sized by the matching *_workspace_* query
 *   - return value: hipError_t as int (0 = success); shape errors return hipErrorInvalidValue
 *   - thread-safe and re-entrant (no global mutable state); callable from the autograd thread
 */
#ifndef C2M_HIP_H
#define C2M_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { C2M_ACT_NONE = 0, C2M_ACT_RELU = 1, C2M_ACT_LRELU = 2, C2M_ACT_SIGMOID = 3 };

/* Names of the geom[] entries of the convolution entry points (enum c2m_geom_index, enum c2m_wino_geom_index) and the ABI version
 * of this header.  A binding checks at load time that the library was built from the same header:
 *   c2m_abi_version() == C2M_ABI_VERSION, c2m_geom_len() == C2M_G_LEN, c2m_wino_geom_len() == C2M_WG_LEN.                      */
#include "c2m_geom.h"
int c2m_abi_version(void);
int c2m_geom_len(void);
int c2m_wino_geom_len(void);

/* ---- convolution: implicit GEMM on v_mfma_f32_32x32x2_f32 (conv_igemm.hip; kernel families behind the same entry points:
 * conv_gather.hip, conv_patch.hip, conv_thin.hip; weight gradient conv_wgrad.hip, reflect fold conv_fold.hip, weight
 * packing conv_pack.hip; NC8 / Winograd / ring forms in conv_nc8.hip, conv_wino.hip, conv_wino4.hip, conv_ring.hip) ----------
 * Replaces nn.Conv2d / nn.Conv3d (+ ReflectionPad2d/3d, bias, LeakyReLU/ReLU/Sigmoid) at:
 *   modules/layers/down_block.py:14-23,35-47   same_block.py:14-23,36-46,55-67   up_block.py:9-13
 *   residual_block.py:13-31,42-71   spade_block.py:47-49   vgg.py:92-137   generator/generator.py:76-78
 *   and their autograd backward (aten::convolution_backward).
 *
 * D[m][pix] = act( sum_k A[m][k] * G(k,pix) + bias[m] ),  G = input gathered through `ktab`.
 * K order: (channel chunk, tap group, tap slot, channel in chunk); one 16-deep K-step = NS taps x CK channels.
 * ktab: nk groups of (1 + NS) int4: header {channel_offset, nvalid_channels (-2: ones row), 0, 0} then NS taps
 *       {dt, dy, dx, valid}; A is the weight matrix packed by the host into the same order ([M][nk*16]).
 * geom[] (int64; 93 entries -- 90 / 91 / 92 are read by every call --, 120 when parity classes are batched):
 *   0 M   1 nk (K-steps; for wgrad: J rows)   2 lda   3 Npix = N*To*Ho*Wo   4 To 5 Ho 6 Wo   7 Ti 8 Hi 9 Wi
 *   10 st 11 sh 12 sw (input coord = o*stride + tap offset)   13 in_sn 14 in_st 15 in_sh (elements; w stride 1)
 *   16 out_sn 17 out_sc 18 out_st 19 out_sh 20 out_sw 21 out_off   22 reflect (0 zeros / 1 reflect) 23 is3d
 *   24 NS (1, 2 or 4)   25 in_sc (channel stride)   26 splits (from c2m_conv_igemm_splits, or 1)
 *   27 slab_stride (elements between split-K slabs)   28 Cin 29 taps 30 tap groups per chunk 31 real groups (wgrad)
 *   32 x_bytes 33 dy_bytes (wgrad; buffer-load bounds, < 2 GiB)
 *   34 operand precision: 0 = fp32 (exact v_mfma_f32_32x32x2_f32), 1 = bf16 operands, fp32 accumulation
 *      (v_mfma_f32_32x32x16_bf16).  Element types in memory (the bf16 data path, BASELINE configs[2-4]): geom[90] X
 *      (wgrad: X and dY), geom[91] Y / Y_interior -- 0 = fp32, 1 = bf16.  The bf16 kernels gather bf16 X ALWAYS (the host
 *      casts an fp32 input once) and write bf16 or fp32 results; split-K slabs are fp32 (c2m_splitk_reduce's `dt` picks the
 *      final type).  The fp32 kernels and the <= 4-output-channel vector-ALU kernels are fp32 in, fp32 out.
 *   36..51 two-target epilogue (reflect-pad dgrad, Y_interior != NULL): padded coordinate = o*ps + po per dim
 *      (36-38 ps, 39-41 po); outputs inside [lo, lo+ext) (42-44 lo, 45-47 ext) are stored to Y_interior with strides
 *      48 sn 49 sc 50 st 51 sh, the pad ring to Y; c2m_reflect_border_add then folds the ring.
 *   52 LDS-patch kernel (3x3, stride 1, fp32): 1 = on; 53 iy0 54 ix0 input origin of an output tile relative to its
 *      first output; 55-57 / 58-60 patch row / column of tap row / column 0,1,2 ((0,1,2) forward, (2,1,0) dgrad)
 *   61 ncls: stride parity classes batched into this launch (blockIdx.z = class*splits + split); 62 floats per class
 *      weight matrix, 63 int4 entries per class tap table, 64+c out_off of class c, 96+3c.. its (po_t, po_y, po_x)
 *      (geom[] holds 120 entries; 90 / 91 / 92 are the element-type and weight-gradient-form flags)
 *   94 NC8 gather form (conv_gather_nc8_kernel, round 4; every bf16 forward / data gradient that is not a 3x3 / 4x4-stride-2 /
 *      3x3x3 patch layer -- down_block.py:14-23 and same_block.py:50-68 in 3-D, the discriminator tails, 1x1 and 7x7 layers, the
 *      reflect data gradients over (W/2 + 1)-wide class planes): 1 = X is the NC8 form ([N][ceil(C/8)][Ti*Hi*Wi][8] bf16, geom[32]
 *      its bytes) of the gathered tensor, A the c2m_pack_weights_bf16_gather image of the launch's first class, ktab a compact
 *      table [ncls][taps] of {dt, dy, dx, 1}, geom[1] = taps * ceil(C/16) K-steps in (tap, chunk) order (C = geom[28], taps =
 *      geom[29] <= 64), geom[24] = 1; classes, splits, the two-target epilogue and the output types as for the NCHW gather kernel.
 *      95: tile variant (0 = by rows: 32 / 64 / 128-row tiles x 256 pixels).
 * With splits > 1, Y must point at a slab of splits*slab_stride floats and c2m_splitk_reduce finishes the op
 * (sum over splits in a fixed order, + bias[(i / chan_stride) % M], activation).                               */
int c2m_conv_igemm_splits(int M, int nk, int Npix);
int c2m_conv_igemm(const float* A, const void* X, void* Y, void* Y_interior, const float* bias, const int* ktab,
                   const int64_t* geom, int act, float slope, void* stream);
int c2m_splitk_reduce(const float* slab, void* out, const float* bias, long total, int splits, long chan_stride,
                      int M, int act, float slope, int dt /* element type of out */, void* stream);

/* dW[m][c][tap] (+ db[m]) = sum_pix dY[m][pix] * G(row,pix): rows in the same (chunk, tap group, slot, channel)
 * order as the forward K, plus one ones-row group (bias gradient), padded to c2m_conv_wgrad_rows(M, groups+1).
 * Deterministic split-K over pixels: slab = c2m_conv_wgrad_splits(M, J, Npix) * M * J floats; the slab reduction
 * writes dW in the native [Cout][Cin][taps] layout.  geom: 0 M, 1 J, 16 dy_sn, 17 dy_sc, 24 NS, 28..31 as above. */
int c2m_conv_wgrad_splits(int M, int J, int Npix);
int c2m_conv_wgrad_rows(int M, int ngroups);
int c2m_conv_wgrad(const void* dY, const void* X, float* slab, float* dW, float* db, const int* jtab,
                   const int64_t* geom, void* stream);

/* Native conv weights ([Cout][Cin][kt][kh][kw]) -> the packed K order above, one launch; also the per-parity-class
 * transposed matrices of the data gradient (rows = input channels), all classes stacked along the rows.
 * g[]: 0 M rows per class, 1 C (K-side channels), 2 CK, 3 KT, 4 KH, 5 KW, 6 st, 7 sh, 8 sw (1,1,1 = forward),
 *      9 row stride, 10 channel stride of the source (elements).  Replaces the reshape/permute/copy chain that
 *      aten::convolution does internally on its weights (no reference line of its own).                          */
int c2m_pack_weights(const float* w, float* packed, const int64_t* g, void* stream);
/* Every pack of a model in ONE launch (after an optimizer step each trainable weight needs each of its layouts rebuilt once:
 * ~195 launches of 5-7 us in a full G + D step).  The host fills one job record per (weight, layout) -- type 0: the arguments of
 * c2m_pack_weights, type 1: those of c2m_pack_weights_bf16_patch, type 2: those of c2m_pack_weights_bf16_gather -- with the index of its first workgroup (ascending, dense),
 * keeps the table (and one (job, workgroup) pair per workgroup of the launch) in device memory and refreshes all packs in place
 * with c2m_pack_multi.  c2m_pack_job_fill returns the number of workgroups of the job (< 0: bad geometry).                                                           */
int c2m_pack_job_bytes(void);
long c2m_pack_job_fill(void* host_job, int type, const void* w, void* packed, const int64_t* g, unsigned first_block);
int c2m_pack_multi(const void* device_jobs, const void* device_blocktab /* int32 (job, workgroup in job) per workgroup */,
                   int njobs, long total_blocks, void* stream);
/* bf16 weight image of the bf16 LDS-patch kernel (3x3 stride-1 layers in bf16 mode, BASELINE configs[2-4]):
 * out[chunk][tap][row padded to a multiple of 128][16 channels] bf16.  g[] = {M, C, s_m, s_c, flip}; flip = 1 for the
 * data gradient (rotated taps).  Pass the result as A to c2m_conv_igemm with geom[2] (lda) = the padded row count. */
long c2m_pack_weights_bf16_patch_bytes(int M, int C);
int c2m_pack_weights_bf16_patch(const float* w, void* out, const int64_t* g, void* stream);
/* bf16 weight images of the NC8 gather form (geom[94] of c2m_conv_igemm): g[] as c2m_pack_weights with g[2] = 16; out = prod(stride)
 * class images ((rt, ry, rx) row-major) of [tap][16-channel chunk][half][row padded to a multiple of 128] 16-byte units (8 bf16,
 * RNE; zero rows / channels past M / C).  Job type 2 of c2m_pack_job_fill / c2m_pack_multi. */
long c2m_pack_weights_bf16_gather_bytes(const int64_t* g);
int c2m_pack_weights_bf16_gather(const float* w, void* out, const int64_t* g, void* stream);

/* Channel-blocked ("NC8") bf16 convolutions (conv_nc8.hip, round 4; the same 3x3 stride-1 call sites -- vgg.py:92-137,
 * residual_block.py:13-31,42-71, spade_block.py:47-49, up_block.py:9-13, same_block.py:14-23 -- in bf16 mode).
 * c2m_nchw_to_nc8: [N][C][HW] bf16 -> [N][ceil(C/8)][HW][8] bf16 (zero channels past C; HW % 8 == 0): the 8 channels one
 * MFMA lane consumes become ONE 16-byte unit.  c2m_conv_patch_nc8: D = act(W * patches(X) + bias) for a 2-D 3x3 stride-1
 * layer with X in NC8, A = the c2m_pack_weights_bf16_patch image, operands fetched global -> LDS by 16-byte LDS-DMA;
 * geom[] as for c2m_conv_igemm's LDS-patch path (0 M, 1 nk = 9 * chunks, 2 padded rows of A, 3 Npix, 5 Ho, 6 Wo, 8 Hi, 9 Wi,
 * 16-21 output strides / offset, 22 reflect, 26 splits, 27 slab stride, 28 Cin, 36-51 two-target block, 52 = 1, 53-60 patch
 * origin and tap order, 91 output type); Y / Y_interior are NCHW (bf16 or fp32), split-K slabs fp32.                        */
int c2m_nchw_to_nc8(const void* x, void* y, long N, int C, long HW, void* stream);
int c2m_conv_patch_nc8(const void* A, const void* X_nc8, void* Y, void* Y_interior, const float* bias, const int64_t* geom,
                       int act, float slope, void* stream);
/* 4x4 stride-2 pad-1 2-D layers (down_block.py:14-23, discriminator.py:59-89) on the parity-plane form of the same kernel: four
 * (16 channels, input parity) chunks with 2x2 taps each -- the stride-2 gather is the LDS-DMA's per-lane address.  A =
 * c2m_pack_weights_bf16_patch(g[4] = 2) (c2m_pack_weights_bf16_s2_bytes bytes); Y contiguous [N][M][Hi/2][Wi/2], bf16 (yh) or fp32. */
long c2m_pack_weights_bf16_s2_bytes(int M, int C);
int c2m_conv_s2_nc8(const void* A, const void* X_nc8, void* Y, const float* bias, int M, int C, long N, int Hi, int Wi, int reflect,
                    int yh, int act, float slope, void* stream);
/* Data gradient of those layers: the four output parity classes as 2x2 stride-1 correlations of dY over one shared patch, one
 * launch.  A = c2m_pack_weights_bf16_patch with g = {M = input channels, C = output channels, s_m = 16, s_c = M * 16, mode 3 (zeros) /
 * 4 (reflect)}; T = dX [N][M][2Ho][2Wo] (zeros) or the padded gradient [N][M][2Ho+2][2Wo+2] (reflect; c2m_reflect_fold finishes). */
int c2m_conv_s2_dgrad_nc8(const void* A, const void* dY_nc8, void* T, int M, int K, long N, int Ho, int Wo, int reflect, int th,
                          void* stream);
/* 3x3x3 stride-1 pad-1 layers (same_block.py:50-68; motion_autoencoder.py:107-149 fuse_convs / final_fuse) on the same patch
 * kernel: the chunk index runs over (time tap, 16 channels), the workgroup's image is a (sample, frame) pair and the input frame of a
 * chunk is t + kt - 1 (reflected / zero).  X NC8 = [N][ceil(C/8)][T][H][W][8] (c2m_nchw_to_nc8 with HW = T*H*W); A = three
 * c2m_pack_weights_bf16_patch images back to back (kt = 0, 1, 2: w + 9 kt, s_m = 27 C, s_c = 27); Y contiguous [N][M][T][H][W].
 * c2m_conv_wgrad3d_nc8: its weight gradient, one transposed-read launch per time tap (slab: c2m_conv_wgrad_nc8_slab_floats with N*T). */
int c2m_conv3d_nc8(const void* A, const void* X_nc8, void* Y, const float* bias, int M, int C, long N, int T, int H, int W, int reflect,
                   int yh, int act, float slope, void* stream);
/* Its data gradient: launched over the T real frames, frame t summing its (dY frame, time tap) pairs from the device table ptab
 * (int32 [T][11] = {npairs, (frame, kt) x 5}: reflect -- the pad frames folded onto the frames they mirror; zeros -- the in-range
 * pairs); target [N][M][T][H+2][W+2] (reflect: spatially padded gradient, c2m_reflect_fold(pt 0, ph 1, pw 1) finishes) or
 * [N][M][T][H][W] (zeros); the target may have Ctot >= M channels (M = the leading input channels that need a gradient).  A: three
 * pack images with rows = input channels (kt: w + 9 kt, s_m = 27, s_c = 27 Ctot).                                                */
int c2m_conv3d_dgrad_nc8(const void* A, const void* dY_nc8, void* target, const int* ptab, int M, int Ctot, int K, long N, int T, int H,
                         int W, int reflect, int th, void* stream);
int c2m_conv_wgrad3d_nc8(const void* dY_nc8, const void* X_nc8, float* slab, float* dW, float* db, int M, int C, long N, int T, int H,
                         int W, int reflect, void* stream);
/* Weight (+ bias) gradient from NC8 operands: s2 = 0: 2-D 3x3 stride-1 pad-1 layer, dW[m][c][ky][kx] = sum dY[n][m][y][x] *
 * X[n][c][y+ky-1][x+kx-1]; s2 = 1: 4x4 stride-2 pad-1 layer, ... * X[n][c][2y+ky-1][2x+kx-1] (X is the [2H][2W] map; one workgroup per
 * input-row parity, 8 taps each).  zeros or reflect padding; fragments by ds_read_b64_tr_b16 out of plain NC8 images in LDS; slab holds
 * c2m_conv_wgrad_nc8_slab_floats(...) floats of scratch (per-split partial sums, reduced in a fixed order); db may be NULL.  */
int c2m_conv_wgrad_nc8_splits(int M, int C, long N, int H, int W, int s2);
long c2m_conv_wgrad_nc8_slab_floats(int M, int C, long N, int H, int W, int s2);
int c2m_conv_wgrad_nc8(const void* dY_nc8, const void* X_nc8, float* slab, float* dW, float* db, int M, int C, long N, int H,
                       int W, int reflect, int s2, void* stream);

/* Winograd F(2x2,3x3) form of the 3x3 stride-1 layers (conv_wino.hip; same reference call sites as above: vgg.py:92-137,
 * spade_block.py:47-49, residual_block.py:13-71, up_block.py:9-13): 2.25x fewer MFMA FLOPs, fp32, bias/activation fused.
 * c2m_wino_filter_transform packs U = G g G^T in the kernel's fragment order (dgrad = 1: transposed + rotated filter of
 * the data gradient); upack holds c2m_wino_upack_floats(M, K) floats.
 * geom[]: 0 M, 1 K, 2 images, 3 Hi, 4 Wi, 5 Ho, 6 Wo, 7 iy0, 8 ix0 (input origin of output (0,0): -pad forward),
 *         9 reflect, 10 in_sn, 11 in_sc, 12 in_sh, 13 out_sn, 14 out_sc, 15 out_sh, 16 out_off, 17 x_bytes;
 *         with Y_interior (two-target data gradient of a reflect-padded conv, as in c2m_conv_igemm): 18 y2_sn, 19 y2_sc,
 *         20 y2_sh, 21 lo_y, 22 lo_x, 23 ext_y, 24 ext_x;
 *         3x3x3 layers (fuse_convs / the 3-D blocks of the motion decoder, modules/layers/common.py Conv3d call sites) run
 *         as a 2-D Winograd over virtual channels (time tap kt, channel ci), image = (sample, frame): 25 To (frames per
 *         sample of the output), 26 in_st, 27 out_st (frame strides), 28 cin, 29 nkt (0 = 2-D layer, else 3: K = nkt*cin),
 *         30 toff (source frame = t + kt + toff), 31 Ti (source frames), 32 treflect (reflect the source frame index;
 *         otherwise frames outside [0, Ti) are zeros);
 *         33 temporal pair table (device pointer as an integer, or 0): the data gradient of a 3x3x3 layer with reflect
 *         padding in time, launched over the UNPADDED frames -- int32 ptab[To][11] = {npairs, (source frame of dY, U block
 *         = flipped time tap) x 5}: output frame t sums the pairs (to, kt) with reflect(to + kt - 1) == t (needs cin % 8
 *         == 0; toff / treflect are ignored).  With the pair table every launched frame is a real one, so Y_interior may be
 *         given for a 3x3x3 layer too (frames of Y_interior are dense [ext_y][y2_sh] planes inside each channel).
 *         geom[] always holds 34 entries.                                                                           */
long c2m_wino_upack_floats(int M, int K);
int c2m_wino_filter_transform(const float* w, float* upack, int Cout, int Cin, int dgrad, void* stream);
/* Regions (workgroup tiles of <= 32 Winograd tiles) per image c2m_conv_wino uses for an Ho x Wo output domain: 8 x 16
 * outputs, or another th x tw tile shape when that covers a badly fitting domain (18 x 34: 9 -> 6) with <= 0.9x as many. */
int c2m_wino_regions(int Ho, int Wo);
int c2m_conv_wino(const float* upack, const float* X, float* Y, float* Y_interior, const float* bias,
                  const int64_t* geom, int act, float slope, void* stream);

/* Winograd F(4x4, 3x3) form of the same 2-D launches (conv_wino4.hip: 36 multiplies per 16 outputs, 4x fewer MFMA FLOPs than
 * the direct form; points 0, +-3/4, +-3/2, inf: fp32 error 2e-6 ... 4e-6 of the tensor scale): one workgroup = 64 rows x a
 * 16 x 32 output region.  upack: c2m_wino4_upack_floats(M, K) floats written by c2m_wino4_filter_transform (same arguments as
 * the F(2x2,3x3) transform); c2m_conv_wino4 takes c2m_conv_wino's geom[] and refuses its 3x3x3 entries (geom[29], geom[33] != 0).
 * Replaces the same call sites as c2m_conv_wino (ATen conv2d forward / data gradient of the 3x3 stride-1 layers,
 * layers/vgg.py:92-137, residual_block.py:13-31, spade_block.py:47-49).                                                 */
long c2m_wino4_upack_floats(int M, int K);
int c2m_wino4_filter_transform(const float* w, float* upack, int Cout, int Cin, int dgrad, void* stream);
int c2m_wino4_regions(int Ho, int Wo);
int c2m_conv_wino4(const float* upack, const float* X, float* Y, float* Y_interior, const float* bias,
                   const int64_t* geom, int act, float slope, void* stream);

/* Winograd weight gradient of the same layers: dg = G^T [ sum_tiles (A dY A^T) (.) (B^T d B) ] G (3x3, stride 1, pad 1,
 * H % 2 == 0, W % 8 == 0).  slab: c2m_wino_wgrad_splits(...) * 16 * M * K floats, dbslab: splits * M floats; dW in the
 * native [Cout][Cin][3][3] layout, db [Cout] (may be NULL).  Deterministic (fixed-order slab reduction).           */
int c2m_wino_wgrad_splits(int M, int K, int nimg, int H, int W);
int c2m_conv_wino_wgrad(const float* dY, const float* X, float* slab, float* dbslab, float* dW, float* db, int M, int K,
                        int nimg, int H, int W, int reflect, void* stream);
/* The same for the 3x3x3 stride-1 pad-1 layers (Conv3d call sites of modules/layers/common.py): image = (sample, frame),
 * virtual input channels (time tap, channel).  dY [N][M][T][H][W], X [N][Cin][T][H][W]; dW is written as [M][3][Cin][3][3]
 * (the caller permutes to the native [M][Cin][3][3][3]); slab / dbslab sized for K = 3*Cin, nimg = N*T
 * (c2m_wino_wgrad_splits(M, 3*Cin, N*T, H, W)). */
int c2m_conv_wino_wgrad3d(const float* dY, const float* X, float* slab, float* dbslab, float* dW, float* db,
                          int M, int Cin, int N, int T, int H, int W, int reflect, void* stream);

/* Pad-ring part of the data gradient of a reflect-padded (pad 1) 3x3 stride-1 convolution, folded straight into dX
 * (conv_ring.hip).  Replaces, together with a c2m_conv_wino / c2m_conv_wino4 launch over the EXACT H x W domain, the ATen chain
 * reflection_pad2d_backward(conv2d_backward_input(..)) of the `nn.Conv2d(.., padding=1, padding_mode='reflect')` call sites
 * (layers/residual_block.py:13-31,42-71, same_block.py:50-68, spade_block.py:47-49): dX [N][M][H][W] must already hold the
 * zero-padded "same" data gradient (the interior of the padded gradient); this launch adds what rows 0, H+1 and columns 0, W+1 of
 * the padded gradient mirror onto rows 1, H-2 and columns 1, W-2 -- four three-tap GEMMs M x 3C x (N * line) on the exact fp32
 * MFMA + one thread per (image, row, corner) for the four targets that receive three ring terms.  Every element of dX has one
 * writer: no atomics, bit-repeatable.  w: native [C][M][3][3] (C = the layer's output channels, M = its input channels);
 * apack: c2m_ring_pack_floats(C, M) floats written by c2m_ring_pack; dY [N][C][H][W]; H, W >= 4; tensors < 2 GiB.            */
/* Split operand mode of the direct fp32 forward / data-gradient kernel (conv_igemm_kernel; knob C2M_DIRECT_MATH = fp32 | split |
 * auto, read at every launch): out[9] (may be NULL) = launches that ran on split-bf16 operands since the last reset, indexed
 * [tile rows: 32, 64, 128][NS: 1, 2, 4] -- one entry per instantiation the launcher can pick; reset != 0 zeroes the counters.
 * Returns 9.                                                                                                                */
int c2m_direct_math_counts(int64_t* out, int reset);

long c2m_ring_pack_floats(int C, int M);
int c2m_ring_pack(const float* w, float* apack, int C, int M, void* stream);
int c2m_reflect_ring_dgrad(const float* apack, const float* w, const float* dY, float* dX, int N, int C, int M, int H, int W,
                           void* stream);
/* Buffer form (the one the product runs): the ring terms are WRITTEN -- coalesced, no read-modify-write of dX, corners carried by
 * the row terms -- into R [N][M][4][r_l] (sides 0 / 1: added to row 1 / H-2 at column x; 2 / 3: to column 1 / W-2 at row y;
 * r_l >= max(H, W), r_l % 4 == 0, 16-byte aligned), and the c2m_conv_wino / c2m_conv_wino4 launch that FOLLOWS on the same stream
 * over the exact domain adds them in its epilogue: geom[C2M_WG_RING] = R, geom[C2M_WG_RING_L] = r_l (2-D, single target,
 * out_off 0).  The in-place form spent 19 of its ~50 us per launch on one-float-per-128-byte-line accesses to dX's two columns. */
int c2m_reflect_ring_buffer(const float* apack, const float* dY, float* R, int N, int C, int M, int H, int W, int r_l,
                            void* stream);

/* Adjoint of reflection padding: folds a gradient over the padded domain back (ReflectionPad2d/3d backward);
 * _border_add is the in-place form used after a two-target dgrad (dX already holds the direct term).          */
int c2m_reflect_border_add(const void* dXpad, void* dX, long NC, int T, int H, int W, int pt, int ph, int pw,
                           int dt, void* stream);
int c2m_reflect_fold(const void* dXpad, void* dX, long NC, int T, int H, int W, int pt, int ph, int pw,
                     int dt, void* stream);

/* ---- normalisation + activation (norm.hip) -----------------------------------------------------------------
 * BatchNorm2d/3d(train) / InstanceNorm2d / SPADE + LeakyReLU/ReLU:
 *   down_block.py:19-22,44-47  same_block.py:19-22,41-44,64-67  up_block.py:11-12  residual_block.py:20-28,56-70
 *   spade_block.py:68-77.   mode 0 = per (n,c) plane, 1 = per channel over N*S.                              */
/* `dt` = element type of the ACTIVATION tensors (x, y, gy, dx, the SPADE maps gb / ggb): 0 fp32, 1 bf16 (csrc/dtype.h);
 * statistics, affine parameters and their gradients are fp32 in either case, all arithmetic is fp32 in registers.      */
long c2m_norm_workspace_floats(int N, int C, long S);
int c2m_norm_stats(const void* x, float* mean, float* invstd, float* running_mean, float* running_var,
                   float* workspace, int N, int C, long S, int mode, float eps, float momentum, int dt, void* stream);
/* c2m_norm_stats followed by c2m_norm_apply (without the NC8 side output) as ONE call: instance-norm planes (mode 0) of 1024 ...
 * 32768 elements run as one launch that keeps the plane in registers between the statistics and the apply pass (same arithmetic and
 * summation order as the three-launch path; bit-identical for planes of <= 8192 elements); everything else runs the three launches.
 * c2m_norm_bwd makes the same choice by itself for mode 0 without affine-parameter gradients and planes of <= 8192 elements.      */
int c2m_norm_set_fused(int on);       /* tests / A/B: 0 = always the three-launch path; returns the previous setting */
int c2m_norm_fwd(const void* x, float* mean, float* invstd, float* running_mean, float* running_var, float* workspace,
                 const float* gamma, const float* beta, const void* gb, void* y, int N, int C, long S, int mode, float eps,
                 float momentum, int act, float slope, int dt, void* stream);
/* The two entries above with a replication count (mode 1 only; rep = 1 is what they call): the batch stands for `rep` identical
 * copies of itself (one encoded source frame shared by `rep` predicted frames).  mean, invstd and y are the batch's own; only the
 * running variance sees the larger count: unbiased = m2 * rep / (n * rep - 1), what the statistics of the copied batch would give. */
int c2m_norm_stats_rep(const void* x, float* mean, float* invstd, float* running_mean, float* running_var,
                       float* workspace, int N, int C, long S, int mode, float eps, float momentum, int rep, int dt, void* stream);
int c2m_norm_fwd_rep(const void* x, float* mean, float* invstd, float* running_mean, float* running_var, float* workspace,
                     const float* gamma, const float* beta, const void* gb, void* y, int N, int C, long S, int mode, float eps,
                     float momentum, int rep, int act, float slope, int dt, void* stream);
/* y_nc8 / dx_nc8 (bf16 tensors with S % 8 == 0): the result in the channel-blocked layout [N][ceil(C/8)][S][8] the NC8 convolutions
 * consume (bit for bit c2m_nchw_to_nc8 of the NCHW result) INSTEAD of y / dx -- the activation feeds only a convolution, the gradient
 * is the dY of the convolution in front.  Exactly one of (y, y_nc8) and of (dx, dx_nc8) is given: both return hipErrorInvalidValue. */
int c2m_norm_apply(const void* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                   const void* gb, void* y, void* y_nc8, int N, int C, long S, int mode, int act, float slope, int dt, void* stream);
int c2m_norm_bwd(const void* x, const void* gy, const float* mean, const float* invstd, const float* gamma,
                 const float* beta, const void* gb, void* ggb, float* dgamma, float* dbeta, void* dx, void* dx_nc8,
                 float* workspace, int N, int C, long S, int mode, int act, float slope, int dt, void* stream);
int c2m_act_bwd(const void* y, const void* gy, void* gx, long total, int act, float slope, int dt, void* stream);
/* The same gradient (mode 0), or the perceptual-loss tap backward of c2m_relu_tap_bwd (mode 1: t, gl, count = the tap's element
 * count, gy may be NULL), written in the NC8 layout of the bf16 convolutions INSTEAD of NCHW ([N][ceil(C/8)][S][8] bf16; y / t / gy
 * bf16 [N][C][S], S % 8 == 0): for gradients whose only readers are NC8 convolution kernels (round 4; the layout pass and the NCHW
 * write disappear).  Same fp32 arithmetic per element as the NCHW kernels. */
int c2m_grad_to_nc8(int mode, const void* y, const void* t, const void* gy, const float* gl, void* g_nc8, long N, int C, long S,
                    long count, int act, float slope, void* stream);

/* ---- optical-flow warping / resampling (warp.hip) -----------------------------------------------------------
 * utils/ops.py:183-202 resample()/get_grid()/grid_sample() and its backward; callers generator.py:86,
 * motion_autoencoder.py:125 (fused "* occlusion"), losses.py:219, model.py:204,208.                          */
/* `dt` = element type of the image-side tensors (img, out, gout, gimg / in, out): 0 fp32, 1 bf16; flow, occlusion and the
 * flow gradient are fp32 (coordinates are never rounded to bf16).                                                  */
int c2m_flow_warp_fwd(const void* img, const float* flow, const float* occ, void* out, int N, int C, int H, int W,
                      int dt, void* stream);
/* backward of the above (ATen grid_sampler_2d_backward: a float-atomic scatter on GPUs).  Deterministic here: d(image) is
 * gathered through an inverted tap list built in `workspace`, d(flow) is summed in a fixed channel order; neither
 * output needs zero-initialisation and either may be NULL.                                                      */
long c2m_flow_warp_bwd_workspace_bytes(int N, int C, int H, int W, int want_gimg, int want_gflow);
int c2m_flow_warp_bwd(const void* img, const float* flow, const float* occ, const void* gout, void* gimg,
                      float* gflow, int N, int C, int H, int W, void* workspace, int dt, void* stream);
/* F.interpolate(bilinear) (utils/utils.py:349 align_corners=True; motion_autoencoder.py:123, up_block.py:10).  */
int c2m_resize_bilinear(const void* in, void* out, long NC, int Hi, int Wi, int Ho, int Wo, int align,
                        double scale_factor, int dt, void* stream);
/* adjoint of the size-given c2m_resize_bilinear (any Hi, Wi, Ho, Wo >= 1, both align modes): gin [NC][Hi][Wi] from
 * gout [NC][Ho][Wo].  Gathers per input pixel in a fixed order (no float atomics, no zero-initialisation of gin).   */
int c2m_resize_bilinear_bwd(const void* gout, void* gin, long NC, int Hi, int Wi, int Ho, int Wo, int align, int dt,
                            void* stream);
int c2m_upsample2x_fwd(const void* in, void* out, long NC, int Hi, int Wi, int dt, void* stream);
/* The same up-sampling (up_block.py:10) from an NC8 tensor to an NC8 tensor ([N*ceil(C/8)][H][W][8] bf16 -> [..][2H][2W][8]), for the
 * up block whose convolution reads the channel-blocked form only (round 4); per channel the arithmetic of c2m_upsample2x_fwd. */
int c2m_upsample2x_nc8(const void* in_nc8, void* out_nc8, long NCB, int Hi, int Wi, void* stream);
int c2m_upsample2x_bwd(const void* gout, void* gin, long NC, int Hi, int Wi, int dt, void* stream);
/* torchvision.ops.roi_align(aligned=False, sampling_ratio=-1), appearance_encoder/appearance_encoder.py:67-69.
 * boxes [K,5] = (batch, x1, y1, x2, y2) stay on the device; the backward gathers per feature pixel in a fixed order (no
 * float atomics, no zero-initialisation of gfeat [N,C,H,W]).                                                       */
int c2m_roi_align_fwd(const float* feat, const float* boxes, float* out, int K, int C, int H, int W, int PH, int PW,
                      float spatial_scale, void* stream);
int c2m_roi_align_bwd(const float* boxes, const float* gout, float* gfeat, int N, int K, int C, int H, int W, int PH,
                      int PW, float spatial_scale, void* stream);
/* VGG-19 max pools (layers/vgg.py, torchvision features 4/9/18/27).                                           */
int c2m_maxpool2x2_fwd(const void* in, void* out, long NC, int Hi, int Wi, int dt, void* stream);
int c2m_maxpool2x2_bwd(const void* in, const void* gout, void* gin, long NC, int Hi, int Wi, int dt, void* stream);
/* The same for a window input that is the output of a ReLU (vgg.py: conv -> ReLU -> MaxPool2d): gin is the gradient of the
 * ReLU's INPUT (pool backward x (in > 0)), which spares the activation-backward pass over the full-resolution tensor. */
int c2m_maxpool2x2_relu_bwd(const void* in, const void* gout, void* gin, long NC, int Hi, int Wi, int dt, void* stream);

/* ---- FlowNet2 operators of the online target-flow path (flownet_ops.hip) -----------------------------
 * Replace the reference's CUDA extensions, forward only (the flow net runs frozen under no_grad, flow_net.py:32,66-67):
 * resample2d/src/resample2d_kernel.cu:16-75 (bilinear warp, pixel-unit flow, border clamp; caller flownet2/models.py:127,
 * 146,166,177), channelnorm/src/channelnorm_kernel.cu:19-62 (L2 norm over channels -> [N,1,H,W]; models.py:130,148,165,
 * 175), correlation/src/correlation_cuda_kernel.cu:47-147 (+ correlation_cuda.cc:25-38 output size; FlowNetC cost volume,
 * networks/flownet_c.py:44-46).  c2m_bias_act: bias + activation in place, the epilogue of the transposed convolutions
 * (networks/submodules.py:75-80), whose matrix part runs on c2m_conv_igemm's data-gradient form.                          */
int c2m_resample2d_fwd(const float* img, const float* flow, float* out, int N, int C, int H, int W, void* stream);
int c2m_channelnorm_fwd(const float* x, float* out, int N, int C, int H, int W, void* stream);
int c2m_correlation_out_size(int H, int pad, int kernel_size, int max_displacement, int stride1);
int c2m_correlation_fwd(const float* in1, const float* in2, float* out, int N, int C, int H, int W, int pad,
                        int kernel_size, int max_displacement, int stride1, int stride2, void* stream);
int c2m_bias_act(float* x, const float* bias, long N, int C, long HW, int act, float slope, void* stream);

/* ---- sparse-motion raster + occlusion splat (motion_raster.hip): bit-exact index/mask path ------------------
 * motion_estimator/dense_motion.py:94-168 generate_sparse_motion/warp/clip_mask;
 * utils/ops.py:205-275 get_occlusion_map/get_corresponding_map.                                              */
int c2m_sparse_raster(const float* instance, const int* obj_id, const int* obj_batch, const float* thetas, float* bw,
                      float* fw, float* bin, int B, int K, int T, int H, int W, void* stream);
long c2m_occlusion_splat_workspace_bytes(long nimg, int H, int W);
int c2m_occlusion_splat(const float* flow, long sb, long sc, long st, int B, int T, int H, int W, float* occ,
                        float* clip, void* workspace, void* stream);

/* ---- label propagation along the generator's flow (label_warp.hip): rollouts of c2m_amd.interactive -----------------------
 * The reference has no counterpart: it gets the label maps of a frame from Panoptic-DeepLab and an offline tracker.  Frame t of
 * `generated` takes pixel p from position s(p) of the last input frame (utils/ops.py:183-202 resample(); c2m_flow_warp_fwd), so
 * the label of p in frame t is the label of the pixel nearest to s(p): a nearest-neighbour gather with the bilinear warp's own
 * coordinates (csrc/warp_coord.h, after the border clamp), rounded half to even as ATen's nearest grid_sample does.
 * flow [B][2][T][H][W] fp32 in pixels, element strides sb / sc / st of sample / channel / frame, rows dense (a [B][2][H][W]
 * flow: T = 1, st = 0); planes_f [B][Cf][H][W] fp32 -> out_f [B][Cf][T][H][W], planes_i [B][Ci][H][W] int32 -> out_i
 * [B][Ci][T][H][W]; words are copied, never blended.  Cf or Ci may be 0 (its pointers are then not read).  occ [B][1][T][H][W]
 * fp32 or NULL: where occ < threshold the INTEGER outputs get fill_id (a disoccluded pixel belongs to no known object); float
 * planes are not touched.  One launch, no atomics, no workspace; 64-bit indexing when a tensor has >= 2^31 elements.        */
int c2m_label_warp(const float* flow, long sb, long sc, long st, const float* occ, float threshold, int fill_id,
                   const float* planes_f, int Cf, const int32_t* planes_i, int Ci, int B, int T, int H, int W, float* out_f,
                   int32_t* out_i, void* stream);

/* ---- nearest-seed fill of label planes (nearest_fill.hip): propagate_maps(fill="nearest") of c2m_amd.interactive ------------
 * The reference has no counterpart.  hole, seed: uint8 [B][T][H][W], dense, nonzero = set; a pixel set in both is a hole and never
 * a seed.  Every hole pixel (y, x) of image (b, t) takes the words planes[b][c][t][y'][x'] of every plane c from the seed pixel
 * (y', x') of the same image with the smallest ((y - y')^2 + (x - x')^2, y', x'), compared as integers (exact; ties go to the
 * smaller row, then the smaller column).  IN PLACE: only holes are written and only seeds are read, and the two are disjoint.
 * planes_f fp32 [B][Cf][T][H][W] with element strides (fsb, fsc, fst) of sample, channel, frame and dense rows; planes_i int32
 * likewise; words are copied, never interpreted.  Cf or Ci may be 0 (its pointer is then not read), not both.
 * unfilled int32 [B][T] (zeroed by the call): the holes of an image WITHOUT a seed, which is left as it is.
 * H, W <= 32768, H * W < 2^31.  workspace: c2m_nearest_fill_workspace_bytes(B, T, H, W) bytes (-1 for sizes out of range), 8-byte
 * aligned, zero-filled by the call: one bit per pixel in 64-bit words per row, and a seed counter per image.  Everything is checked
 * before the first launch; two zero-fills and two kernels on `stream`, no synchronisation, no copy to the host, no loop that waits
 * for another wave (each is bounded by H or by ceil(W / 64)).  Integer atomic adds only: bit-repeatable.                        */
long c2m_nearest_fill_workspace_bytes(int B, int T, int H, int W);
int c2m_nearest_fill(const uint8_t* hole, const uint8_t* seed, float* planes_f, long fsb, long fsc, long fst, int Cf,
                     int32_t* planes_i, long isb, long isc, long ist, int Ci, int B, int T, int H, int W, int32_t* unfilled,
                     void* workspace, long workspace_bytes, void* stream);

/* ---- dense inverse search optical flow (dense_flow.hip): c2m_amd.flow.dense_flow, ClassicFlow -----------------------------
 * The reference has no counterpart: its only flow producer is FlowNet2 (modules/third_party/flow_net/flow_net.py), which needs
 * a checkpoint.  The flow is that of a -> b in pixels, channel 0 = x, a(x) ~ b(x + flow(x)); DESIGN.md 4.2l states every step.
 * Sizes: 8 <= H, W <= 32768, 1 <= levels <= 7, level l + 1 is ((h + 1) / 2, (w + 1) / 2) and every level is >= 8 on both sides;
 * a level has (n - 8) / 4 + 1 patches per axis, one more where n - 8 is no multiple of 4 (origin of patch j: min(4 j, n - 8)).
 * c2m_flow_workspace_bytes: the workspace of one call (-1 for sizes out of range), 4-byte aligned, never zeroed: per level the gray
 *   images a [N][h][w] then b [N][h][w]; the patch records of level 0 [N][npy][npx][3] (reused by the smaller levels); the flows
 *   of the levels >= 1, [N][2][h][w].  c2m_flow_workspace_offset: where `what` of `level` starts, in floats (0 image a, 1 image b,
 *   2 flow, level >= 1; 3 records) or -1.
 * c2m_flow_pyramid: a, b [N][3][H][W] (dt 0 fp32, 1 bf16) -> every level of both, ONE launch.  A value v becomes
 *   (v - lo) * (255 / (hi - lo)); gray = (0.299 R + 0.587 G) + 0.114 B; a coarser pixel is (((p00 + p01) + p10) + p11) * 0.25 of
 *   the 2 x 2 block at (2y, 2x), rows and columns clamped to the last.
 * c2m_flow_patch_search: ia, ib [N][h][w] (image_elems floats each) -> records [N][npy][npx][3] = (u, v, mean(J) - mean(T)), ONE
 *   launch, one wave per patch.  init: NULL (zero flow) or the dense flow [N][2][hc][wc] with hc, wc = ceil(h, w / 2^init_shift),
 *   init_shift 0 or 1, read as 2^init_shift * init[(oy + 3) >> init_shift][(ox + 3) >> init_shift].  iters (<= 1024) steps for
 *   every patch whose det > 40.96, no early exit; a patch that ends more than 8 px from its initial flow returns to it.
 * c2m_flow_densify: flow [N][2][Ho][Wo], pixel (Y, X) = 2^shift * the weighted mean at level pixel (Y >> shift, X >> shift) over
 *   the <= 3 x 3 patches that cover it, ascending (oy, ox), weight 1 / max(1, |(J - T) - record[2]|); ((Ho - 1) >> shift) < h.
 * Every size and extent is checked before the launch; all three run on `stream`; no atomics, no synchronisation, no host copy:
 * bit-repeatable, and the result of a pair does not depend on N.                                                               */
long c2m_flow_workspace_bytes(int N, int H, int W, int levels);
long c2m_flow_workspace_offset(int N, int H, int W, int levels, int what, int level);
int c2m_flow_pyramid(const void* a, const void* b, int dt, float lo, float hi, int N, int H, int W, int levels,
                     void* workspace, long workspace_bytes, void* stream);
int c2m_flow_patch_search(const float* ia, const float* ib, long image_elems, const float* init, long init_elems,
                          int init_shift, float* records, long record_elems, int N, int h, int w, int iters, void* stream);
int c2m_flow_densify(const float* ia, const float* ib, long image_elems, const float* records, long record_elems,
                     float* flow, long flow_elems, int N, int h, int w, int shift, int Ho, int Wo, void* stream);

/* ---- variational refinement of the dense flow (flow_refine.hip): c2m_amd.flow.refine_flow, dense_flow(refine=...) ----------
 * The reference has no counterpart.  On ONE pyramid level: ia, ib [N][h][w] gray on 0..255 (image_elems floats each), flow
 * [N][2][h][w] the level's dense flow (u, v); 8 <= h, w <= 32768.  DESIGN.md 4.2m states every formula and its association order.
 * c2m_flow_refine_workspace_bytes: the workspace of one level (-1 for sizes out of range), 4-byte aligned, never zeroed: the
 *   planes Ix, Iy, Iz, Ixx, Ixy, Iyy, Ixz, Iyz as [8][N][h][w], then (du, dv) [N][2][h][w] twice.
 * c2m_flow_refine_prepare: the eight planes from ia, ib and flow, ONE launch (J = ib sampled at x + flow, the coordinate clamped
 *   to the image before the gather; central differences with clamped indices).
 * c2m_flow_refine_iterate: outer iteration `iteration` (0, 1, ...; < 1024), ONE launch: the weights and the linear system from
 *   (du, dv) of iteration - 1 (zero for iteration 0), then `sor` (1 .. 5) red-black SOR sweeps with relaxation omega (0 .. 2),
 *   colour (x + y) & 1 == 0 first; alpha, delta, gamma > 0.  out NULL: (du, dv) goes to the workspace, to the copy of index
 *   iteration & 1.  out [N][2][Ho][Wo] (the last iteration): pixel (Y, X) = 2^shift * (u + du, v + dv) at level pixel
 *   (Y >> shift, X >> shift), shift 0 .. 6, ((Ho - 1) >> shift) < h; out must not be `flow`.
 * Every size, extent and parameter is checked before the launch; both run on `stream`; no atomics, no synchronisation, no host
 * copy: bit-repeatable, independent of N and of the tiling (equal to the global red-black sweep in fp32).                       */
long c2m_flow_refine_workspace_bytes(int N, int h, int w);
int c2m_flow_refine_prepare(const float* ia, const float* ib, long image_elems, const float* flow, long flow_elems,
                            void* workspace, long workspace_bytes, int N, int h, int w, void* stream);
int c2m_flow_refine_iterate(const float* flow, long flow_elems, void* workspace, long workspace_bytes, int N, int h, int w,
                            int iteration, int sor, float alpha, float delta, float gamma, float omega, float* out,
                            long out_elems, int shift, int Ho, int Wo, void* stream);

/* ---- segment-guided dense flow (dense_flow.hip, flow_refine.hip): c2m_amd.flow.dense_flow(segments=...) ---------------------
 * The reference has no counterpart.  The three launchers above with a guide: segments [N][H][W] int32 (segment_elems of them),
 * the ids of frame a at level 0; any integer is an id and none is special.  A stage on level `level` (0 .. 6) reads the id of
 * its pixel (y, x) at segments[y << level][x << level]; ((h - 1) << level) < H and ((w - 1) << level) < W.  DESIGN.md 4.2p.
 * c2m_flow_patch_search_guided: every patch sum runs over the n >= 1 pixels whose id is that of the patch centre (oy + 3,
 *   ox + 3), means are sum / n, a patch is searched iff det > 40.96 * n^2 / 4096; records [N][npy][npx][4] = (u, v, mean(J) -
 *   mean(T), n): record_elems >= 4 * N * npy * npx.
 * c2m_flow_densify_guided: records of 4 floats; a pixel is averaged over the covering patches whose centre has its id (all of
 *   them if there is none), weight n / max(1, |residual|).
 * c2m_flow_refine_iterate_guided: a forward difference toward a neighbour of another id is 0 in the smoothness weight, and the
 *   weight of an edge between two ids is 0.
 * Everything else, the checks included, is as above; N == 0 returns 0.  With one id everywhere the results are those of the
 * unguided launchers, bit for bit.                                                                                              */
int c2m_flow_patch_search_guided(const float* ia, const float* ib, long image_elems, const float* init, long init_elems,
                                 int init_shift, float* records, long record_elems, int N, int h, int w, int iters,
                                 const int32_t* segments, long segment_elems, int level, int H, int W, void* stream);
int c2m_flow_densify_guided(const float* ia, const float* ib, long image_elems, const float* records, long record_elems,
                            float* flow, long flow_elems, int N, int h, int w, int shift, int Ho, int Wo,
                            const int32_t* segments, long segment_elems, int level, int H, int W, void* stream);
int c2m_flow_refine_iterate_guided(const float* flow, long flow_elems, void* workspace, long workspace_bytes, int N, int h,
                                   int w, int iteration, int sor, float alpha, float delta, float gamma, float omega,
                                   float* out, long out_elems, int shift, int Ho, int Wo, const int32_t* segments,
                                   long segment_elems, int level, int H, int W, void* stream);

/* ---- block-matching seed of the coarsest level (dense_flow.hip): c2m_amd.flow.patch_match, dense_flow(seed=...) ---------------
 * The reference has no counterpart.  On ONE pyramid level, with the patches of c2m_flow_patch_search: ia, ib [N][h][w]
 * (image_elems floats each) -> records [N][npy][npx][3] = (dx, dy, mean(J) - mean(T)), ONE launch, one wave per patch.  A patch
 * tries every integer displacement (dx, dy) in [-radius, radius]^2, 1 <= radius <= 8, whose 8 x 8 window lies wholly inside
 * ib's level (0 <= ox + dx <= w - 8, 0 <= oy + dy <= h - 8; (0, 0) always is; no coordinate is clamped, nothing is interpolated)
 * and takes the smallest key (cost, dx^2 + dy^2, dy, dx), compared lexicographically.  cost = sum(((J - mJ) - Tm)^2), J ib's
 * window at the displacement, mJ = sum(J) / 64, both sums over the 64 pixels in raster order (row by row, one term after the
 * other, from 0); T, mean(T), Tm = T - mean(T) and det are those of the search, and a patch with det <= 40.96 takes (0, 0).
 * DESIGN.md 4.2q.  The records have the layout of the search's and are densified by c2m_flow_densify.
 * c2m_flow_patch_match_guided: segments, segment_elems, level, H, W as above; every sum runs over the n >= 1 pixels whose id is
 *   that of the patch centre, means are sum / n, the threshold is 40.96 * n^2 / 4096, records [N][npy][npx][4] = (.., n).  One
 *   id everywhere gives the bits of the unguided form.
 * Every size, extent, alignment and the radius are checked before the launch; N == 0 returns 0; no atomics, no
 * synchronisation, no host copy: bit-repeatable, and the result of a pair does not depend on N.                                */
int c2m_flow_patch_match(const float* ia, const float* ib, long image_elems, float* records, long record_elems, int N, int h,
                         int w, int radius, void* stream);
int c2m_flow_patch_match_guided(const float* ia, const float* ib, long image_elems, float* records, long record_elems, int N,
                                int h, int w, int radius, const int32_t* segments, long segment_elems, int level, int H, int W,
                                void* stream);

/* ---- chains of frame-to-frame flows (flow_chain.hip): c2m_amd.flow.chain_flows, clip_flows ---------------------------------
 * The reference has no counterpart.  Frames c_0 .. c_K of N clips; steps [N][K][2][H][W] fp32, channel 0 = x, pixels, with the
 * convention above; out [N][K][2][H][W]; valid [N][K][H][W] uint8 or NULL.  DESIGN.md 4.2n states the algorithm.
 * forward 0: steps[j] is the flow c_{j+1} -> c_j and out[k] the flow c_{k+1} -> c_0: from every pixel of c_{k+1}, d = (0, 0),
 *   then for j = k .. 0: d += steps[j] sampled at pixel + d.  forward 1: steps[j] is c_j -> c_{j+1}, out[k] is c_0 -> c_{k+1}:
 *   one walk j = 0 .. K - 1 from every pixel of c_0 that writes d after every hop.  The sample is the bilinear gather of the
 *   flow kernels: its coordinate is clamped to the image first (a NaN goes to 0), so every read is inside the step planes
 *   whatever they hold; pixel + d itself is never clamped.  The first hop reads at integer coordinates with weight 1: out[0]
 *   is steps[0] for finite steps.  valid is 1 iff pixel + d was inside [0, W - 1] x [0, H - 1] after every hop (a NaN: 0).
 * 1 <= K <= 16, H, W >= 1, N * K * 2 * H * W < 2^31; step_elems, out_elems >= N * K * 2 * H * W, valid_elems >= N * K * H * W;
 * out must not be steps.  Everything is checked before the launch; ONE launch on `stream`, no atomics, no synchronisation, no
 * host copy: bit-repeatable, and the result of a clip does not depend on N.                                                    */
int c2m_flow_chain(const float* steps, long step_elems, float* out, long out_elems, uint8_t* valid, long valid_elems,
                   int N, int K, int H, int W, int forward, void* stream);

/* ---- predicted frames at dataset resolution (detail_warp.hip): c2m_amd.fullres ---------------------------------------------
 * The reference has no counterpart.  frame [B][H][W][3] uint8 is the last input frame at the output size; generated, warped
 * [B][3][T][h][w], flow [B][2][T][h][w] (working-size pixels) and occ [B][1][T][h][w] (NULL: 1 everywhere) are dense fp32 at the
 * working size, warped being the working-size frame moved by `flow` without occlusion (c2m_flow_warp_fwd).  With up() the
 * bilinear enlargement (upsample_bilinear2d, align_corners=False) and warpF the bilinear value of `frame` at the position the
 * working-size warp reads, mapped to the large grid and border-clamped (csrc/warp_coord.h, warp_source_at):
 *     out [B][T][H][W][3] uint8 = floor(clip(255 up(generated) + up(occ) (warpF - 255 up(warped)), 0, 255) + 0.5), NaN -> 0.
 * ids [B][H][W] int32 or NULL: out_ids [B][T][H][W] = the id at the nearest pixel of the same position (ties to even), fill_id
 * where up(occ) < threshold (pass -inf for "never").  Needs 2 <= h <= H, 2 <= w <= W, H * W * 3 < 2^31.  One launch, no
 * atomics, no workspace, bit-repeatable; offsets across frames are 64-bit.                                                  */
int c2m_detail_warp(const uint8_t* frame, const float* generated, const float* warped, const float* flow, const float* occ,
                    const int32_t* ids, float threshold, int fill_id, int B, int T, int h, int w, int H, int W, uint8_t* out,
                    int32_t* out_ids, void* stream);

/* ---- frame quality (quality.hip): c2m_amd.evaluate.frame_quality ---------------------------------------------------------------
 * The reference has no counterpart.  Scores B*T predicted frames against the real ones: out [B][T][9][4] float64, row 0 the whole
 * frame and row 1 + k the pixels whose regions byte has bit k, columns (n_pixels, sse, n_windows, ssim_sum): sse the squared
 * error summed over pixels and channels, n_windows the centres whose 11 x 11 window lies inside the frame (and, for a region,
 * whose own pixel has the bit), ssim_sum the sum over those centres of the channel-mean SSIM (Wang et al. as skimage evaluates
 * it with gaussian_weights=True, use_sample_covariance=False, data_range=L; C1 = (0.01 L)^2, C2 = (0.03 L)^2).
 * form 0 / 1: fp32 / bf16 [B][C][T][H][W]; form 2: uint8 [B][T][H][W][C] (integer levels, pass L = 255).  C is 1 or 3, H and W
 * at least 11.  pred_strides / target_strides: HOST arrays of the (B, C, T) strides in elements (C unused for form 2); rows, and
 * for form 2 the channels, are dense.  regions [B][T][H][W] uint8, dense, or NULL (rows 1..8 are then zero).  weights: HOST
 * array of the eleven normalised float64 taps.  workspace: c2m_frame_quality_workspace_bytes(B, T, H, W) bytes.
 * Moments and everything after them are fp64; the uint8 squared error is summed in integers.  Two launches, no atomics,
 * bit-repeatable.                                                                                                             */
long c2m_frame_quality_workspace_bytes(int B, int T, int H, int W);
int c2m_frame_quality(const void* pred, const void* target, const uint8_t* regions, int form, int B, int C, int T, int H, int W,
                      const long* pred_strides, const long* target_strides, const double* weights, double L, void* workspace,
                      long workspace_bytes, double* out, void* stream);

/* ---- flow scores (flow_score.hip): c2m_amd.evaluate.flow_quality, flow_consistency -------------------------------------------
 * The reference has no counterpart.  Flows in pixels, channel 0 = x, a(x) ~ b(x + flow(x)).  B*T pairs, H, W >= 1, H * W < 2^31.
 * Every operand is one or two or C planes of H * W dense elements per pair; its HOST stride triple (B, C, T), in elements,
 * places plane c of pair (b, t) at b * sB + c * sC + t * sT (none negative, sC >= H * W; a zero sB or sT repeats a frame).
 * valid, regions [B][T][H][W] uint8, dense, or NULL.  out [B][T][9][K] float64: row 0 every counted pixel, row 1 + k those whose
 * regions byte has bit k (zero when regions is NULL).  All per-pixel arithmetic is fp64 on exactly converted inputs, in the
 * operation order written at the top of flow_score.hip and in DESIGN.md 4.2r; thresholds compare squared quantities.
 * c2m_flow_quality: pred fp32 (pred_dt 0) or bf16 (1), target fp32, both [..][2][..].  K = 10: (n, n_nonfinite, sum_epe, sum_e2,
 *   sum_mag, sum_ae, n_out, n_gt1, n_gt3, n_gt5).  A pixel is scored when valid != 0 and both target components are finite and
 *   below 1e9 in magnitude; a scored pixel with a non-finite pred component adds nothing to the sums and counts in n,
 *   n_nonfinite and all four threshold counts.
 * c2m_flow_consistency: flow_ab, flow_ba (or NULL) fp32 [..][2][..], a, b fp32 (image_dt 0) or bf16 (1) with C = 1 or 3 planes;
 *   strides: HOST array of the four triples of flow_ab, a, b, flow_ba (the last unused when flow_ba is NULL).  K = 7: (n, n_inside,
 *   sum_photo, sum_photo2, sum_fb, n_incons, sum_photo_cons), the last three NaN when flow_ba is NULL.  alpha1, alpha2 finite and
 *   >= 0.  photo, fb (fp32) and inconsistent (uint8), each [B][T][H][W] dense, all three or all NULL: per-pixel maps written by
 *   the same launch (photo, fb NaN outside the frame).
 * workspace: the matching *_workspace_bytes(B, T, H, W) bytes.  Two launches each (1024-pixel tiles, then one workgroup per
 * pair adds the tiles' partials in a fixed order); no atomics, no synchronisation, no host copy: bit-repeatable, and the sums
 * of a pair do not depend on B or T.  B * T == 0 returns 0.                                                                     */
long c2m_flow_quality_workspace_bytes(int B, int T, int H, int W);
int c2m_flow_quality(const void* pred, const float* target, const uint8_t* valid, const uint8_t* regions, int pred_dt, int B,
                     int T, int H, int W, const long* pred_strides, const long* target_strides, void* workspace,
                     long workspace_bytes, double* out, void* stream);
long c2m_flow_consistency_workspace_bytes(int B, int T, int H, int W);
int c2m_flow_consistency(const float* flow_ab, const void* a, const void* b, const float* flow_ba, const uint8_t* regions,
                         int image_dt, int B, int C, int T, int H, int W, const long* strides, double alpha1, double alpha2,
                         float* photo, float* fb, uint8_t* inconsistent, void* workspace, long workspace_bytes, double* out,
                         void* stream);

/* ---- loss reductions (losses.hip) ---------------------------------------------------------------------------
 * losses/losses.py:180-189 L1MaskedLoss (also :60-65 VGG L1, model.py:118-121 feature matching); :152-177 SSIM. */
int c2m_l1_mean_fwd(const void* a, const void* b, const float* mask, float* out, long total, int C, long inner,
                    void* workspace /* 8 KiB */, int dt /* a, b */, void* stream);
int c2m_l1_mean_bwd(const void* a, const void* b, const float* mask, const float* gscale, void* ga, void* gb,
                    long total, int C, long inner, int dt /* a, b, ga, gb */, void* stream);
/* Backward of a perceptual-loss tap y = relu(conv(x)) that feeds the next VGG conv and mean|y - t| (losses.py:60-65 on the
 * relu{1..5}_1 slices of layers/vgg.py:92-137): out = (gy + gl[0]/total * sign(y - t)) * (y > 0) in one pass; gy may be NULL
 * (last tap), gl is a device scalar (the gradient of the L1 mean).  out is what the conv's data gradient consumes.       */
int c2m_relu_tap_bwd(const void* y, const void* t, const void* gy, const float* gl, void* out, long total,
                     int dt /* y, t, gy, out */, void* stream);
int c2m_ssim_fwd(const float* x, const float* y, float* out, long NC, int H, int W, void* workspace /* 8 KiB */,
                 void* stream);
int c2m_ssim_bwd(const float* x, const float* y, const float* gscale, float* gx, float* coef, long NC, int H, int W,
                 void* stream);

/* ---- object GNN (gnn.hip, round 5): the attention of torch_geometric's GATv2Conv(heads, concat=False, add_self_loops=False)
 * on a dense graph of <= 64 nodes, src/modules/motion_estimator/sparse_motion_estimator.py:104-112 (one layer per predicted frame).
 * xl = lin_l(x), xr = lin_r(x) [N][H][C]; att [H][C]; A [N][N] = number of edges j -> i at A[i][j] (mask and weight of the softmax
 * over the incoming edges); out [N][C] = mean over heads of sum_j alpha[i][j][h] * xl[j][h][:] (the layer's bias is added by the
 * caller); alpha [N][N][H] is kept for the backward.  One launch forward, two backward (per-target partials summed in index
 * order: no atomics).  N <= 64, C <= 1024, fp32.                                                                                */
int c2m_gat_dense_fwd(const float* xl, const float* xr, const float* att, const float* A, float* out, float* alpha, int N, int H,
                      int C, float negative_slope, void* stream);
long c2m_gat_dense_bwd_workspace_floats(int N, int H, int C);
int c2m_gat_dense_bwd(const float* xl, const float* xr, const float* att, const float* alpha, const float* gout, float* dxl,
                      float* dxr, float* datt, float* workspace, int N, int H, int C, float negative_slope, void* stream);

/* ---- input pipeline stage upstream of the path (data_prep.hip): SURVEY §8f-3 -------------------------------------
 * src/datasets/cityscapes.py:30-70 (ToTensor of frames, label-id one-hot split 0..10 / 11..19), :212-265 (occlusion
 * PNG -> clip_mask, .flo HWC -> CHW): decoded uint8 / float arrays in, the batch-dict tensors of model.py:124 out.  */
int c2m_prep_video(const uint8_t* frames_bthwc, float* video_bcthw, int B, int T, int H, int W, void* stream);
int c2m_prep_seg_onehot(const uint8_t* labels_bthw, float* bg_mask, float* fg_mask, int B, int T, int H, int W,
                        void* stream);
int c2m_prep_flow_occ(const uint8_t* occ_bthw, const float* flow_bthwc, float* occ_out, float* flow_out, int B, int T,
                      int H, int W, void* stream);

/* Dataset resolution -> train_params.input_size (resize.hip): src/datasets/cityscapes.py:23-33,211 (PIL Image.resize, BICUBIC for
 * frames, NEAREST for label / instance / occlusion maps) and :220-222 (transforms.Resize on the .flo tensor, * size[0] / h).
 * Every table is built by the caller per axis and passed twice: *_host (read by the entry point: checked, and used to size the
 * tile) and the same values on the device (read by the kernel).  Dense arrays; a launch each; no allocation, no atomics.
 * c2m_resize_u8: [N][Hin][Win][C] uint8, C in {1, 3} -> [N][Hout][Wout][C], Pillow's 8-bit resampler bit for bit: bounds[out][2]
 *   = (first, count) and coef[out][ks] int32 (precompute_coeffs + normalize_coeffs_8bpc: 22 fractional bits), each pass
 *   clip8((2^21 + sum p * k) >> 22), horizontal first, uint8 between the passes.  count in [1, ks], bounds non-decreasing.
 * c2m_resize_nearest: [N][Hin][Win] of 1- or 4-byte elements -> [N][Hout][Wout] through index[out] (source column / row, or -1:
 *   zero), Pillow's NEAREST.
 * c2m_resize_flow: [N][Hin][Win][2] fp32 -> [N][Hout][Wout][2], separable filter with fp32 weights weight[out][ks], fp32
 *   accumulation in a fixed order (row dot products left to right, then top to bottom), then (v * Hout) / Hin on both channels. */
int c2m_resize_u8(const uint8_t* src, uint8_t* dst, int N, int Hin, int Win, int Hout, int Wout, int C,
                  const int32_t* bounds_x_host, const int32_t* bounds_x, const int32_t* coef_x, int ksx,
                  const int32_t* bounds_y_host, const int32_t* bounds_y, const int32_t* coef_y, int ksy, void* stream);
int c2m_resize_nearest(const void* src, void* dst, int elem_bytes, long N, int Hin, int Win, int Hout, int Wout,
                       const int32_t* index_x_host, const int32_t* index_x, const int32_t* index_y_host, const int32_t* index_y,
                       void* stream);
int c2m_resize_flow(const float* src, float* dst, long N, int Hin, int Win, int Hout, int Wout, const int32_t* bounds_x_host,
                    const int32_t* bounds_x, const float* weight_x, int ksx, const int32_t* bounds_y_host,
                    const int32_t* bounds_y, const float* weight_y, int ksy, void* stream);

/* The detector metric (c2m_amd.evaluate; reference: utils/utils_yolov3.py, yolo_v3/models.py YOLOLayer, yolo_v3/utils/utils.py
 * non_max_suppression).  fp32, no atomics, every result bit-repeatable.
 * c2m_detect_input: frame [B][C][H][W] through element strides (the last time index of a video is read in place) -> out
 *   [B][C][S][S]: nearest x scale, zero to the right and below, cropped where the scaled frame is larger than S.
 * c2m_yolo_candidates: heads[h] = device pointer to [N][na[h] * (5 + C)][grid[h]][grid[h]] raw head maps; HOST arrays grid, nanchors,
 *   stride (image size / grid) and anchors [nheads][max_anchors][2] = (w, h) / stride.  Decodes every box, keeps conf >= conf_thres,
 *   and writes them compacted in box order (head, anchor, row, column): cand [N][cap][7] = (x1, y1, x2, y2, conf, class_conf,
 *   class), score [N][cap] = conf * class_conf (slots >= count[n] are not written), count [N].  cap >= boxes per image.
 *   block_count: N * ceil(boxes / 256) ints of workspace.  Two launches (counts; prefix + scatter).
 * c2m_nms_merge: sorted [N][cap][7] = the candidates by descending score; one workgroup per image runs the reference's loop:
 *   head = first alive; invalid = alive, same class, IoU(head's original box, box) > nms_thres (+1 areas, 1e-16); output row =
 *   head's row with box = sum conf * box / sum conf over invalid; invalid and the head are removed.  dets [N][cap][7], kept [N].
 * c2m_match_detections: for object m: node index[m] of the graph (roi [nodes][T][4] = xmin, xmax, ymin, ymax and x
 *   [nodes][tin][F], both read at the last time index; batch [nodes]); detections of image batch (ground truth) and B + batch
 *   (predicted) of dets [2B][cap][7].  flags [M][3] = skipped (-1: index outside the graph), gt_found, pred_found; boxes [M][8] =
 *   the two truncated boxes (y1, x1, y2, x2); err [M][2] = mse, mse_normalized.  skip_area = 0.005 w h, min_area = 0.01 h w.    */
int c2m_detect_input(const float* frame, float* out, int B, int C, int H, int W, long stride_b, long stride_c, long stride_h,
                     long stride_w, int scale, int S, void* stream);
int c2m_yolo_candidates(const void* const* heads, const int* grid, const int* nanchors, const float* stride, const float* anchors,
                        int max_anchors, int nheads, int N, int C, float conf_thres, int cap, int* block_count, float* cand,
                        float* score, int* count, void* stream);
int c2m_nms_merge(const float* sorted, const int* count, int N, int cap, float nms_thres, float* dets, int* kept, void* stream);
int c2m_match_detections(const float* dets, const int* kept, int cap, int B, const long* index, int M, const float* roi, int T,
                         const float* x, int tin, int F, const long* batch, long nodes, int scale, int h, int w,
                         double skip_area, double min_area, int* flags, int* boxes, double* err, void* stream);

/* Per-instance boxes of the input frames, for graphs built from instance maps instead of tracker files (click-to-move;
 * c2m_amd.interactive).  The reference has no counterpart: it reads per-object tracker boxes (cityscapes.py:79-199).
 * c2m_instance_stats: instance [B][T][H][W] int32, planes = (sample, input frame t < t_in); for every id in [id_lo, id_hi)
 *   (id_lo >= 0; other ids are ignored) table[B*t_in][id_hi-id_lo][5] = {count, x_min, x_max, y_min, y_max} (an absent id:
 *   {0, INT_MAX, -1, INT_MAX, -1}).  The table is written in full; integer atomics only, so the result is bit-repeatable.
 * c2m_instance_compact: per sample, the ids with count >= min_pixels (>= 1) in EVERY input frame, ascending:
 *   ids[B][max_nodes], boxes[B][max_nodes][t_in][4] = {x_min, y_min, x_max+1, y_max+1}, count[B] (<= max_nodes),
 *   overflow[B] = 1 when the sample has more than max_nodes such ids.  Slots past count are zero; no atomics.      */
int c2m_instance_stats(const int32_t* instance, int32_t* table, int B, int T, int t_in, int H, int W, int id_lo, int id_hi,
                       void* stream);
int c2m_instance_compact(const int32_t* table, int32_t* ids, int32_t* boxes, int32_t* count, int32_t* overflow, int B,
                         int t_in, int nid, int id_lo, int min_pixels, int max_nodes, void* stream);

/* Linking the objects of two instance maps that do not share ids (instance_link.hip; c2m_amd.tracking).  The reference reads an
 * id column per frame from tracker files instead.  Integer arithmetic after the source coordinate, int32 atomics only:
 * bit-repeatable.  max_nodes <= c2m_instance_link_max_nodes() (64: one lane per slot) in all three.
 * c2m_instance_slots: per plane of a c2m_instance_stats table [planes][nid][5], the ids with count >= min_pixels (>= 1),
 *   ascending; an id's position is its SLOT.  slot_ids[planes][max_nodes] (-1 past count), boxes[planes][max_nodes][4] =
 *   {x_min, y_min, x_max+1, y_max+1} and areas[planes][max_nodes] (zero past count), count[planes] (<= max_nodes),
 *   overflow[planes] = 1 when the plane has more than max_nodes such ids.
 * c2m_instance_overlap: ref, frame [P][H][W] int32; flow [P][2][H][W] fp32 in pixels, defined on the frame's pixels and pointing
 *   into the ref plane, or NULL; the slot lists and counts of both planes as c2m_instance_slots wrote them.
 *   pairs[P][max_nodes+1][max_nodes+1] (written in full) : pairs[p][i][j] = number of frame pixels q whose id has frame slot j
 *   and whose source pixel holds an id with ref slot i; index max_nodes = "no slot".  The source pixel is the one c2m_label_warp
 *   reads for q (same coordinates, border clamp, round half to even); with flow == NULL it is q itself (plain overlap, no
 *   coordinate is computed).  H * W < 2^31.
 * c2m_instance_match: link[P][max_nodes] = the frame slot of every ref slot, or -1.  With r_i / a_j the row / column sums of
 *   pairs (all max_nodes+1 cells) and IoU(i,j) = n_ij / (r_i + a_j - n_ij): j is linked to i iff i has the largest IoU of column j,
 *   j has the largest IoU of row i (cells with n = 0 never count; ties go to the lower slot), IoU * iou_den >= iou_num, and,
 *   with same_class != 0, ref id / 1000 == frame id / 1000.  Fractions are compared by 64-bit cross-multiplication.        */
int c2m_instance_link_max_nodes(void);
int c2m_instance_slots(const int32_t* table, int32_t* slot_ids, int32_t* boxes, int32_t* areas, int32_t* count,
                       int32_t* overflow, int planes, int nid, int id_lo, int min_pixels, int max_nodes, void* stream);
int c2m_instance_overlap(const int32_t* ref, const int32_t* frame, const float* flow, const int32_t* ref_slots,
                         const int32_t* ref_count, const int32_t* frame_slots, const int32_t* frame_count, int32_t* pairs,
                         int P, int H, int W, int max_nodes, void* stream);
int c2m_instance_match(const int32_t* pairs, const int32_t* ref_slots, const int32_t* ref_count, const int32_t* frame_slots,
                       const int32_t* frame_count, int32_t* link, int P, int max_nodes, int iou_num, int iou_den,
                       int same_class, void* stream);

/* ---- Panoptic-DeepLab post-processing (panoptic.hip; c2m_amd.segment) --------------------------------------------------------
 * The label maps and instance maps of N images from the network's three heads, as the reference's get_panoptic_segmentation
 * (post_processing/instance_post_processing.py) and the instance-id image of generate_segmentation.py:299-305 compute them for
 * one image at a time.  Exactly one of logits [N][C][H][W] fp32 (1 <= C <= 256; labels = argmax, first maximum) and labels
 * [N][H][W] uint8 is non-NULL.  center [N][1][H][W], offset [N][2][H][W] (dy, dx) fp32.  class_table: device uint8 [256], 0 for a
 * class that is no thing, else 1 + its position in thing_classes (device int32 [n_things], ascending; n_things <= 255).
 *   centres   score > threshold (>= 0; strict) and equal to the maximum of its nms_kernel x nms_kernel window (odd, 1..15; positions
 *             outside the image do not take part; a plateau keeps all its pixels).  With top_k or more candidates only those
 *             strictly above the top_k-th largest score remain (ties at that score all drop out).  Row-major order:
 *             centers [N][top_k][2] (y, x), zero past center_count [N].  top_k <= c2m_panoptic_max_top_k() (1024).
 *   grouping  a thing pixel belongs to the centre nearest to (y + dy, x + dx), squared distance in fp32, the first of equally
 *             near ones; no centre: no pixel is claimed.
 *   merge     centres ascending: class = the most frequent label among its pixels (ties: the smaller class), value
 *             class * label_divisor + n, n = 1, 2, ... per class; a centre without pixels uses no number.  A class that is no
 *             thing and holds >= stuff_area pixels keeps class * label_divisor; everything else is ignore_label * label_divisor.
 * Outputs [N][H][W]: semantic uint8, panoptic int32, instance int32 (the panoptic value on things, else panoptic / label_divisor).
 * label_divisor > top_k, 256 * label_divisor < 2^31, 0 <= ignore_label <= 255, H * W < 2^31; index arithmetic over N*C*H*W is
 * 64-bit.  workspace: c2m_panoptic_workspace_bytes(N, H, W, top_k, n_things) bytes (-1 for sizes out of range), int32-aligned.
 * Everything is checked before the first launch; five kernels and a zero-fill on `stream`, no synchronisation, no copy to the host.
 * int32 atomics only: bit-repeatable, and the centre order does not depend on scheduling.                                     */
int c2m_panoptic_max_top_k(void);
long c2m_panoptic_workspace_bytes(int N, int H, int W, int top_k, int n_things);
int c2m_panoptic_maps(const float* logits, const uint8_t* labels, int C, const float* center, const float* offset,
                      const uint8_t* class_table, const int32_t* thing_classes, int n_things, uint8_t* semantic,
                      int32_t* instance, int32_t* panoptic, int32_t* centers, int32_t* center_count, void* workspace,
                      long workspace_bytes, int N, int H, int W, float threshold, int nms_kernel, int top_k, int label_divisor,
                      int stuff_area, int ignore_label, void* stream);

/* ---- Connected components and instances from label maps (components.hip; ops.connected_components, c2m_amd.segment) ----------
 * The reference has no counterpart: it reads instance ids a network produced.  keys: N images of H x W, uint8 (key_bytes 1) or
 * int32 (key_bytes 4), rows dense (x stride 1), stride_y and stride_n in elements (>= 0; the keys are only read).  Two pixels
 * belong to one component when they are `connectivity` (4 or 8) neighbours and carry the same key; there is no background.
 * labels int32 [N][H][W]: at every pixel the index y * W + x of its component's first pixel in raster order -- a function of the
 * input alone, and of its own image alone.  H, W >= 1, H * W < 2^31, N * H * W < 2^31.  workspace:
 * c2m_components_workspace_bytes(N, H, W) bytes (-1 for sizes out of range), int32-aligned, nothing in it need be initialised.
 * Three launches on `stream` whatever N is (64 x 16 tiles in LDS, a lock-free union by minimum index across the tile seams,
 * a flatten pass); no kernel waits for another workgroup's write, no synchronisation, no copy to the host, bit-repeatable.
 *
 * c2m_semantic_instances: labels uint8 [N][H][W] dense; class_table device uint8 [256], 0 or 1 + the position of the class in
 * the thing list (n_things <= 32).  components [N][H][W]: the operator's result on the labels.  A component of a thing class
 * with at least min_area (>= 1) pixels qualifies; the qualifying components of a class in an image are numbered n = 1, 2, ... by
 * ascending first raster pixel, and the first label_divisor - 1 of them are kept.  instance [N][H][W]: class * label_divisor + n
 * on a kept component, else the label (stuff, ignore_label, small components, components past the cap).  count, dropped
 * [N][n_things]: kept components, and qualifying ones past the cap.  label_divisor >= 1, 256 * label_divisor < 2^31.
 * workspace: c2m_semantic_instances_workspace_bytes(N, H, W, n_things) bytes (-1 out of range); the call zeroes what it adds into.
 * A zero-fill and eight launches on `stream`; int32 atomics only, so every output is exact and bit-repeatable.                 */
int c2m_components_tile_w(void);
int c2m_components_tile_h(void);
long c2m_components_workspace_bytes(int N, int H, int W);
int c2m_connected_components(const void* keys, int key_bytes, long stride_n, long stride_y, int32_t* labels, void* workspace,
                             long workspace_bytes, int N, int H, int W, int connectivity, void* stream);
long c2m_semantic_instances_workspace_bytes(int N, int H, int W, int n_things);
int c2m_semantic_instances(const uint8_t* labels, const uint8_t* class_table, int n_things, int32_t* instance,
                           int32_t* components, int32_t* count, int32_t* dropped, void* workspace, long workspace_bytes, int N,
                           int H, int W, int connectivity, int min_area, int label_divisor, void* stream);

/* ---- Scoring of label maps (map_quality.hip; c2m_amd.evaluate.map_quality) ------------------------------------------------------
 * Panoptic-quality counts and the confusion matrix of N predicted maps against N ground-truth maps, per image, as the reference's
 * pq_compute_single_core (cityscapesscripts/evaluation/evalPanopticSemanticLabeling.py) and SemanticEvaluator.update compute them
 * for one image at a time.  pred, gt: [N][H][W], both int32 or both uint8 (is_u8).  A value v reads as (cat, n) = (v, 0) below
 * label_divisor, else (v / label_divisor, v % label_divisor); void: v < 0, cat == ignore_label or cat >= num_classes.  A segment
 * is the pixels of one image with the same non-void (cat, n); a ground-truth segment of a thing class (thing_table: device uint8
 * [256], non-zero for a thing) with n == 0 is a crowd region.
 *   pairs     a non-crowd ground-truth segment g and a predicted segment p of the same class match iff 2 * inter > union, union =
 *             area_p + area_g - inter - void_p (void_p: p's pixels on ground-truth void); a match adds 1 to tp[class] and
 *             inter / union (float64) to iou[class], summed per class over g in ascending n.
 *   fn        unmatched non-crowd ground-truth segments; fp: unmatched predicted segments unless 2 * (void_p + crowd_p) > area_p
 *             (crowd_p: p's pixels on the crowd region of its own class).
 *   confusion [N][C+1][C+1] int64, [pred][gt], void last.
 * Outputs: tp, fp, fn int32 [N][C], iou float64 [N][C], confusion, overflow uint8 [N] (1: the image had more distinct pairs of
 * equal class than max_pairs, the hash table's slots; the surplus pairs were dropped).  1 <= num_classes <= 255, label_divisor
 * >= 1, num_classes * label_divisor <= 2^20, max_pairs a power of two <= 2^22, ignore_label >= 0, H * W < 2^31; the image offset
 * is 64-bit.  workspace: c2m_map_quality_workspace_bytes(N, num_classes, label_divisor, max_pairs) bytes (-1 for sizes out of
 * range), 8-byte aligned, zero-filled by the call.  Everything is checked before the first launch; a zero-fill and three kernels on
 * `stream`, no synchronisation, no copy to the host, no loop that waits for another wave (the hash makes at most max_pairs probes).
 * Integer atomics only: every output is bit-repeatable.                                                                        */
long c2m_map_quality_workspace_bytes(int N, int num_classes, int label_divisor, int max_pairs);
int c2m_map_quality(const void* pred, const void* gt, int is_u8, const uint8_t* thing_table, int32_t* tp, int32_t* fp,
                    int32_t* fn, double* iou, int64_t* confusion, uint8_t* overflow, void* workspace, long workspace_bytes,
                    int N, int H, int W, int num_classes, int label_divisor, int ignore_label, int max_pairs, void* stream);

/* ---- Scoring of label maps over time (map_quality.hip; c2m_amd.evaluate.tube_quality) -----------------------------------------
 * Video panoptic quality: the counts above with a TUBE for a segment.  pred, gt: clips [B][T][H][W] with the encodings and
 * parameters of c2m_map_quality.  A window (b, t0, k) is frames t0 .. t0 + k - 1 of clip b (never across a clip); a tube segment
 * is the pixels of the window with one non-void (cat, n); the rules above apply to the window as if it were one image of k * H
 * rows.  windows: HOST int32 [n_windows], distinct k in 1..T.  The outputs hold the results of windows[0], then windows[1], ...:
 * with nw(k) = B * (T - k + 1) windows for k, in the order (b, t0), tp, fp, fn are int32 [sum nw][C], iou float64 [sum nw][C],
 * overflow uint8 [sum nw] (1: a frame of the window had more pairs than max_pairs, or the window's own table of max_pairs slots
 * filled).  k = 1 equals c2m_map_quality bit for bit.
 * ids (optional, with M >= 1): device int32 [B][M] map values, negative = padding.  With g the key of ids[b][m], id_iou float64
 * [sum nw][M] is -1 for padding, a void value, a ground-truth crowd key or a g without ground-truth pixels in the window, else
 * inter / union with inter = the pixels of the window that hold g in BOTH maps and union = area_p[g] + area_g[g] - inter -
 * void_p[g]: the same-id IoU, not thresholded.  id_gt_area, id_pred_area int32 [sum nw][M]: area_g[g], area_p[g] (0 where g is
 * padding, void or a crowd key).  ids == NULL: M must be 0 and the three outputs are not touched.
 * The pixels are read once: the count pass of c2m_map_quality over the B * T frames, then per k a zero-fill of the window tables,
 * a merge of the k per-frame tables of every window (sums; the pair tables re-inserted with the same key and hash), and the pair
 * and class passes of c2m_map_quality on the window tables; k = 1 runs them on the frame tables.  Limits of c2m_map_quality with
 * N = B * T, and T * H * W < 2^31 (a window's counts are int32).  workspace: c2m_tube_quality_workspace_bytes(B, T, num_classes,
 * label_divisor, max_pairs) bytes (-1 for sizes out of range), 8-byte aligned.  Everything is checked before the first launch;
 * all launches on `stream`, no synchronisation, no copy to the host, no loop that waits for another wave.  Integer atomics only:
 * every output is bit-repeatable.                                                                                               */
long c2m_tube_quality_workspace_bytes(int B, int T, int num_classes, int label_divisor, int max_pairs);
int c2m_tube_quality(const void* pred, const void* gt, int is_u8, const uint8_t* thing_table, const int32_t* windows,
                     int n_windows, int32_t* tp, int32_t* fp, int32_t* fn, double* iou, uint8_t* overflow, const int32_t* ids,
                     int M, double* id_iou, int32_t* id_gt_area, int32_t* id_pred_area, void* workspace, long workspace_bytes,
                     int B, int T, int H, int W, int num_classes, int label_divisor, int ignore_label, int max_pairs,
                     void* stream);

/* ---- Relabelling of instance maps (instance_link.hip; c2m_amd.tracking.anchor_maps) --------------------------------------------
 * maps, out: int32 [P][H*W] planes (out may not alias maps).  Plane p has n = count[p] <= 64 pairs (from[p][i], to[p][i]), from
 * strictly ascending over i < n (device int32 [P][64] each).  A value equal to a from becomes its to -- all at once, so two ids
 * may swap --; every other value v >= label_divisor whose class v / label_divisor is a thing (thing_table: device uint8 [256],
 * non-zero for a thing; classes above 255 are no things) becomes (v / label_divisor) * label_divisor, its class's crowd id;
 * everything else (stuff, void, negative values) is copied.  HW < 2^31, label_divisor >= 1.  One launch on `stream`.          */
int c2m_instance_relabel(const int32_t* maps, int32_t* out, const int32_t* from, const int32_t* to, const int32_t* count,
                         const uint8_t* thing_table, int P, long HW, int label_divisor, void* stream);

/* ---- rendering (render.hip): results as uint8 pictures on the device ------------------------------------------------
 * A SHEET is uint8 [T][rows*H][cols*W][C] (HWC); sample b sits in cell (b / cols, b % cols), as the reference's merge
 * (utils/utils.py:26-43) lays samples out; cells without a sample hold zero input.  B <= rows * cols.  Inputs are dense
 * [B][C][T][H][W]; dt = 0 fp32, 1 bf16 (csrc/dtype.h; bf16 is widened to fp32 first, as the reference's .float()).
 * Number formats are numpy's in the reference, operation by operation (see render.hip).  No allocation, no float atomics.
 *
 * c2m_render_frames: utils/utils.py:46-72 (tensor2im, tensor2occ; evaluator/evaluator.py:185-254).  C in {1, 3};
 *   level = trunc(clip(x * 255, 0, 255)), or (x + 1) / 2 * 255 with normalize, in fp32 like numpy.  NaN -> 0 (numpy leaves the
 *   uint8 conversion of NaN undefined).
 * c2m_render_flow: the Middlebury colour code, RGB sheet.  mode 0 = sheet-normalised (utils/utils.py:75-80 tensor2flow ->
 *   utils/ops.py:143-175 compute_flow_img / flow2img): components with |u| or |v| > 1e7 are unknown (zero for the radius,
 *   black in the picture), maxrad = the largest radius over the whole sheet of frame t (a NaN radius makes it -1, Python's
 *   max(-1, nan)), u / maxrad + eps, v / maxrad + eps, all in double; an all-zero sheet is 0 / 0 = NaN = black.  workspace:
 *   c2m_render_flow_workspace_bytes(T) bytes, 8-byte aligned (zeroed by the call; integer max of the radius' bit pattern).
 *   mode 1 = fixed scale (utils/utils.py:287-305 save_flows -> utils/ops.py:84-140 compute_flow_color_map): u * scale,
 *   v * scale (the reference: 3), no normalisation, in double (numpy keeps float32 up to the wheel position there, with an
 *   arctan2 that is not correctly rounded: 2e-5 of a normal flow's pixels differ by one level); workspace may be NULL.
 *   NaN components -> 0 in both modes.
 * c2m_render_instances: ids [B][1][T][H][W] int32 -> RGB sheet on top of `base` (an RGB sheet, NULL = black; may be `out`).
 *   A pixel whose id differs from a 4-neighbour inside its frame (utils/ops.py:278-284 get_edges) and whose largest id m among
 *   itself and those neighbours is in [id_lo, id_hi) gets palette[m % P]; otherwise a pixel whose id is in the range is
 *   tinted (base * (256 - alpha) + palette[id % P] * alpha) >> 8, alpha in 0..256; other pixels keep base.  id_lo >= 0.
 * c2m_draw_overlays: draws onto an RGB sheet in place (utils/utils.py:244-284 draw_bbox / save_images_w_bbox).  Gather form:
 *   every pixel of a cell walks the cell's primitives in order -- boxes by node, then polylines by index -- and keeps the
 *   last that covers it, so nothing is drawn outside the cell.  boxes [B][N][T][4] int32 pixel edges (x0, y0, x1, y1) in
 *   cell coordinates: the 1-pixel outline of [x0, x1-1] x [y0, y1-1] where presence [B][N][T] (bytes) is non-zero, colour
 *   box_rgb [B][N][3]; N <= c2m_draw_overlays_max_boxes() (64, the table kept in LDS).  Polyline d of sample sample[d]:
 *   points [D][P][2] int32 (x, y); frame t shows the first min(count[d][t], P) points and a 3x3 marker on the last shown one,
 *   colour line_rgb [D][3].  A segment a -> b with n = max(|dx|, |dy|) covers, for i = 0..n along the major axis (x when
 *   |dx| >= |dy|), the minor coordinate a_minor + floor((2 * i * d_minor + n) / (2 * n)); n = 0: the single point.      */
int c2m_render_frames(const void* x, int dt, int B, int C, int T, int H, int W, int rows, int cols, int normalize,
                      uint8_t* out, void* stream);
long c2m_render_flow_workspace_bytes(int T);
int c2m_render_flow(const void* flow, int dt, int B, int T, int H, int W, int rows, int cols, int mode, float scale,
                    uint8_t* out, void* workspace, void* stream);
int c2m_render_instances(const int32_t* ids, int B, int T, int H, int W, int rows, int cols, const uint8_t* base,
                         const uint8_t* palette, int P, int id_lo, int id_hi, int alpha, uint8_t* out, void* stream);
int c2m_draw_overlays_max_boxes(void);
int c2m_draw_overlays(uint8_t* sheet, int B, int T, int H, int W, int rows, int cols, const int32_t* boxes,
                      const uint8_t* presence, const uint8_t* box_rgb, int N, const int32_t* points, const int32_t* sample,
                      const int32_t* count, const uint8_t* line_rgb, int D, int P, void* stream);

/* ---- measurement (events.hip): timing events without the system-scope fence of a default hipEventRecord; used by the
 * roofline measurement of bench.py (HIP events on the launch stream), never by the product path.        */
int c2m_event_create(void** event_out);
int c2m_event_record(void* event, void* stream);
int c2m_event_elapsed_ms(void* start, void* stop, float* ms);
int c2m_event_destroy(void* event);
/* For the tests of "a fixed number of launches": the number of nodes the graph capture on `stream` has recorded so far (0 when
 * the stream is not capturing); the difference around a call is what the call put on the stream.                     */
int c2m_capture_node_count(void* stream, long* nodes);

/* ---- optimizer (optim.hip): SURVEY §8f-1 --------------------------------------------------------------------
 * The four torch.optim.Adam(betas=(0.5,0.999), eps=1e-7) of modules/model.py:54-99, stepped at trainer/trainer.py:155-165:
 * one launch per parameter group.  table = device int64 [4][ntensors] {param, grad, exp_avg, exp_avg_sq} pointers,
 * sizes = device int64 [ntensors], blockmap = device int32 [nblocks][2] (tensor, chunk of c2m_adam_chunk() elements).
 * step_size = lr / (1 - beta1^t) and bias_correction2_sqrt = sqrt(1 - beta2^t) are computed by the caller in double,
 * exactly as ATen's single-tensor Adam does; the kernel mirrors its fp32 operation order.                         */
int c2m_adam_chunk(void);
int c2m_adam_step(const int64_t* table, const int64_t* sizes, const int32_t* blockmap, int ntensors, int nblocks,
                  double beta1, double beta2, double eps, double step_size, double bias_correction2_sqrt, void* stream);

#ifdef __cplusplus
}
#endif
#endif
