// What the kernel families behind c2m_conv_igemm / c2m_conv_wgrad share (conv_igemm.hip, conv_gather.hip, conv_patch.hip,
// conv_thin.hip, conv_wgrad.hip): the launch parameter blocks, the tap / pixel arithmetic and the host launchers that cross files.
#pragma once
#include "common.h"
#include "dtype.h"
#include "conv_store.h"
#include "conv_types.h"

struct ConvP {
    const float* A;
    const float* X;
    float* Y;            // output, or the slab base when splits > 1
    const float* bias;   // per-row (may be null); ignored when splits > 1
    const int4* ktab;    // per K-step: header {chan_off, nvalid_chan, 0, 0} + NS x {dt, dy, dx, valid}
    int M, nk, lda;      // nk K-steps of 16
    int Npix, To, Ho, Wo;
    int Ti, Hi, Wi;
    int st, sh, sw;
    int in_sc;           // channel stride of the gathered tensor (elements)
    long in_sn, in_st, in_sh;
    long out_sn, out_sc, out_st, out_sh, out_sw, out_off;
    long slab_stride;    // elements between split slabs
    unsigned x_bytes;    // size of X in bytes (buffer-load bounds: out-of-range lanes read 0)
    // optional second target (reflect-pad dgrad): outputs whose padded coordinate (o*ps + po) lies inside
    // [lo, lo+ext) go straight to the unpadded gradient Y2, only the pad ring is written to Y
    float* Y2;
    int ps_t, ps_y, ps_x, po_t, po_y, po_x, lo_t, lo_y, lo_x, ext_t, ext_y, ext_x;
    long y2_sn, y2_sc, y2_st, y2_sh;
    // LDS-patch variant (3x3, stride 1): input origin of a tile = o + (iy0, ix0); per-tap offsets inside the patch
    int iy0, ix0, pty[3], ptx[3], nchunks, cin;   // cin: input channels of the gathered tensor (LDS-patch kernels)
    int ksteps_per_split;
    int reflect, is3d;
    int act;
    float slope;
    // class batching (stride-s data gradient: the s^d parity classes share every dimension and differ only in
    // weights, tap table and output origin): blockIdx.z = cls * splits + split
    int ncls, splits, ktab_cls;       // ktab_cls: int4 entries per class table
    // bf16 data path (dtype.h): the bf16-operand kernels (BF) gather X as bf16 ALWAYS -- the host casts fp32 inputs once -- and
    // write Y / Y2 as bf16 when yh is set and the launch stores results directly (split-K slabs stay fp32).  The fp32 kernels
    // and the vector-ALU thin kernels read fp32 X, or bf16 X when xh is set (thin kernels only).
    int xh, yh;
    long a_cls;                       // floats per class weight matrix
    long out_off_c[8];
    int po_c[8][3];
    // NC8 gather kernel (conv_gather_nc8_kernel): X = [N][CB][Ti*Hi*Wi][8] bf16, A = c2m_pack_weights_bf16_gather image
    // [class][tap][16-channel chunk][half][Mpad rows] 16-byte units, ktab = [class][ntaps] {dt, dy, dx, 1}
    int g8_nch, g8_ntaps, g8_CB, g8_Mpad;
    unsigned g8_a_bytes, g8_plane_bytes;      // bytes of ONE class image; bytes of one channel-block plane
};

struct WgradP {
    const float* dY;     // [N][M][pix_per_image] contiguous
    const float* X;
    float* slab;         // [S][M][J]
    const int4* jtab;    // per 16-row group (= NS taps x CK channels, same format as the igemm K-step table):
                         // {chan_off, nvalid_chan (-2: ones row, 0: zero rows), 0, 0} + NS x {dt,dy,dx,valid}
    int M, J;            // J = padded (tap, channel) rows incl. the ones-row group
    int Npix, To, Ho, Wo, Ti, Hi, Wi, st, sh, sw;
    int in_sc;
    long in_sn, in_st, in_sh;
    long dy_sn, dy_sc;   // dY strides (pix stride 1)
    int pix_per_split;   // multiple of 64
    int reflect, is3d;
    unsigned x_bytes, dy_bytes;
};

// spatial offset of one tap for this thread's pixel, or -1 when it falls in zero padding
__device__ __forceinline__ int spatial_off(const int4 tp, int ots, int oys, int oxs, int Ti, int Hi, int Wi, int in_st,
                                           int in_sh, int reflect, int is3d) {
    int it = is3d ? ots + tp.x : 0, iy = oys + tp.y, ix = oxs + tp.z;
    bool ok = tp.w != 0;
    if (reflect) {
        if (is3d) { it = it < 0 ? -it : it; it = it >= Ti ? 2 * Ti - 2 - it : it; }
        iy = iy < 0 ? -iy : iy; iy = iy >= Hi ? 2 * Hi - 2 - iy : iy;
        ix = ix < 0 ? -ix : ix; ix = ix >= Wi ? 2 * Wi - 2 - ix : ix;
    } else {
        ok = ok && (unsigned)iy < (unsigned)Hi && (unsigned)ix < (unsigned)Wi;
        if (is3d) ok = ok && (unsigned)it < (unsigned)Ti;
    }
    return ok ? it * in_st + iy * in_sh + ix : -1;
}

// Split operand mode of the direct kernels (conv_igemm_kernel, PREC = 2): an fp32 value as the exact sum of
// three bf16 pieces, v == p0 + p1 + p2 bit for bit, split by TRUNCATION (no piece can overflow; every piece carries v's sign and
// at most 8 significant bits).  Inf and NaN give a NaN piece (Inf - Inf), so non-finite inputs still reach the output.
// Returns the pieces as the high halves of three fp32 bit patterns (c2m_pack_hi pairs them into bf16x2 words).
__device__ __forceinline__ void c2m_split3(float v, unsigned& p0, unsigned& p1, unsigned& p2) {
    p0 = __builtin_bit_cast(unsigned, v) & 0xFFFF0000u;
    const float r = v - __builtin_bit_cast(float, p0);                  // exact: <= 16 significant bits
    p1 = __builtin_bit_cast(unsigned, r) & 0xFFFF0000u;
    p2 = __builtin_bit_cast(unsigned, r - __builtin_bit_cast(float, p1));   // exact: <= 8 significant bits, low half is zero
}
// {hi16(lo), hi16(hi)} as one bf16x2 word (v_perm_b32)
__device__ __forceinline__ unsigned c2m_pack_hi(unsigned lo, unsigned hi) { return __builtin_amdgcn_perm(hi, lo, 0x07060302u); }

// The six products of the split mode in descending weight: (piece of A, piece of B).  The first C2M_SPLIT_NHIGH go to the main
// accumulator, the others to a second one that is added at the end (tools/micro/split_bf16_gemm.hip, form s6/lo4).
#define C2M_SPLIT_NPROD 6
#define C2M_SPLIT_NHIGH 2
__device__ constexpr int C2M_SPLIT_PA[C2M_SPLIT_NPROD] = {0, 0, 1, 0, 1, 2};
__device__ constexpr int C2M_SPLIT_PB[C2M_SPLIT_NPROD] = {0, 1, 0, 2, 1, 0};

template <class P>
__device__ __forceinline__ void decompose_pix(int pix, const P& p, int& n, int& ot, int& oy, int& ox) {
    ox = pix % p.Wo; int r = pix / p.Wo;
    oy = r % p.Ho;   r = r / p.Ho;
    ot = r % p.To;   n = r / p.To;
}

// Host launchers called across files (built with -fvisibility=hidden: not exported).  Each one picks its kernel's tile from
// p.M itself.  The forward launchers return the hipError_t of the launch; the two weight-gradient launchers only launch
// and return the number of slab splits they wrote, c2m_conv_wgrad checks the launch and reduces that many.
int c2m_launch_gather_nc8(const ConvP& p, int variant, int splits, hipStream_t s);                                // conv_gather.hip
int c2m_launch_patch(const ConvP& p, int splits, hipStream_t s);                                                  // conv_patch.hip
int c2m_launch_patch_bf16(const ConvP& p, int splits, hipStream_t s);
int c2m_launch_thin_fwd(const ConvP& p, int ns, hipStream_t s);                                                   // conv_thin.hip
int c2m_launch_thin_rows(const ConvP& p, int kw, int ns, int ntg, int Cin, int xdesc, hipStream_t s);
int c2m_launch_thin_wgrad_rows(const WgradP& p, int kw, int NS, int ntg, int Cin, int ngroups, int S, hipStream_t s);
int c2m_launch_thin_wgrad(WgradP p, int NS, int ngroups, int S, hipStream_t s);
