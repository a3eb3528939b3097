// NC8 gather form of the bf16 implicit-GEMM convolution (round 4); reached through c2m_conv_igemm (conv_igemm.hip) with geom[C2M_G_G8] = 1.
//
// The general bf16 forward / data-gradient kernel over CHANNEL-BLOCKED activations (conv_nc8.hip has the layout and the 3x3 /
// 4x4-stride-2 / 3x3x3 patch forms): any tap set, stride, 2-D or 3-D, stride-parity classes, two-target reflect epilogue, split-K --
// the geometry of conv_igemm_kernel -- for the layers the patch forms do not take ((3,4,4) / (4,4,4) stride-2 blocks, 7x7, 1x1,
// small or ragged maps, the reflect data gradients of the stride-2 layers whose (W/2 + 1)-wide class planes waste half of a
// 32-column tile).  A K-step is (tap, 16 channels); per K-step a wave fetches the two 16-byte units (channel blocks 2c, 2c + 1)
// of ITS 64 pixels with two LDS-DMA instructions whose per-lane address is the pixel's tap offset, computed once per TAP (the
// K loop runs tap-major: chunks inside) -- the NCHW gather kernel issued 16 two-byte loads, 8 packs and 2 ds_write_b128 per lane
// for the same K-step and spent 105 VALU per 8 MFMAs on them.  Weights come pre-packed in bf16
// ([tap][chunk][half][row]) by LDS-DMA as well.  Tile BM rows x 256 pixels, wave w owns pixels 64 w .. 64 w + 63 for all rows;
// U K-steps per stage, NBUF stages, one barrier per stage with counted vmcnt (every wave issues NDMA instructions per stage;
// steps past the split's end and channel blocks past the tensor's last go through zero-record descriptors).
#include "conv_common.h"

template <int BM, int U, int NBUF, int WGS>
__global__ __launch_bounds__(256, WGS) void conv_gather_nc8_kernel(const ConvP p) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    constexpr int MI = BM / 32, NI = 2;
    constexpr int A_ST = U * 2 * BM;                              // weight units per stage: [u][half][row]
    constexpr int NAI = (A_ST + 255) / 256;
    constexpr int A_PAD = NAI * 256;
    constexpr int BUF = A_PAD + U * 512;                          // + [u][half][256 pixels]
    constexpr int NDMA = NAI + 2 * U;
    static_assert(64 % (2 * BM) == 0 || (2 * BM) % 64 == 0, "a 64-unit DMA row belongs to one K-step");
    static_assert(NBUF * BUF * 16 * WGS <= 158 * 1024, "LDS");
    __shared__ uint4 smem[NBUF * BUF];
    __shared__ int4 s_taps[64];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const C2mBlock blk = c2m_xcd_block((unsigned)(p.Npix + 255) / 256, (unsigned)(p.M + BM - 1) / BM, 1);
    const int m0 = blk.y * BM, n0 = blk.x * 256;
    const int cls = p.ncls > 1 ? (int)blk.z / p.splits : 0;
    const int split = p.ncls > 1 ? (int)blk.z - cls * p.splits : (int)blk.z;
    const int k_beg = split * p.ksteps_per_split;
    const int k_end = k_beg + p.ksteps_per_split < p.nk ? k_beg + p.ksteps_per_split : p.nk;
    const int nch = p.g8_nch, ntaps = p.g8_ntaps;

    if (tid < ntaps) s_taps[tid] = p.ktab[cls * ntaps + tid];

    // ---- this lane's pixel (DMA side and MFMA column side agree: wave w holds pixels 64 w ..)
    const int pix = n0 + wave * 64 + lane;
    const bool pvalid = pix < p.Npix;
    int pn, pt, py, px;
    decompose_pix(pvalid ? pix : p.Npix - 1, p, pn, pt, py, px);
    const int ots = pt * p.st, oys = py * p.sh, oxs = px * p.sw;
    const int in_st = (int)p.in_st, in_sh = (int)p.in_sh;
    const unsigned img_byte = (unsigned)pn * (unsigned)p.g8_CB * p.g8_plane_bytes;
    auto tap_voff = [&](int tap) -> unsigned {
        const int4 tp = s_taps[tap < ntaps ? tap : ntaps - 1];
        int it = p.is3d ? ots + tp.x : 0, iy = oys + tp.y, ix = oxs + tp.z;
        bool ok = pvalid;
        if (p.reflect) {
            if (p.is3d) { it = it < 0 ? -it : it; it = it >= p.Ti ? 2 * p.Ti - 2 - it : it; }
            iy = iy < 0 ? -iy : iy; iy = iy >= p.Hi ? 2 * p.Hi - 2 - iy : iy;
            ix = ix < 0 ? -ix : ix; ix = ix >= p.Wi ? 2 * p.Wi - 2 - ix : ix;
        } else {
            ok = ok && (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi && (unsigned)it < (unsigned)p.Ti;
        }
        return ok ? img_byte + (unsigned)(it * in_st + iy * in_sh + ix) * 16u : C2M_OOB;
    };

    const unsigned lds0 = (unsigned)(unsigned long)(__attribute__((address_space(3))) uint4*)&smem[0];
    const unsigned long aaddr = (unsigned long)p.A + (unsigned long)cls * p.g8_a_bytes;
    const u32x4 ars = {(unsigned)aaddr, (unsigned)(aaddr >> 32) & 0xffffu, p.g8_a_bytes, 0x00020000u};
    const unsigned long xaddr = (unsigned long)p.X;
    const u32x4 xrs = {(unsigned)xaddr, (unsigned)(xaddr >> 32) & 0xffffu, p.x_bytes, 0x00020000u};
    const unsigned a_step_bytes = (unsigned)(2 * p.g8_Mpad * 16);
    unsigned avo[NAI];
#pragma unroll
    for (int i = 0; i < NAI; ++i) {
        const int d = (i * 4 + wave) * 64 + lane, within = d % (2 * BM);
        avo[i] = d < A_ST ? (unsigned)(((within / BM) * p.g8_Mpad + m0 + within % BM) * 16) : C2M_OOB;
    }

    // issue-side running state: the K-steps are issued in ascending order, (tap, chunk) advance with them
    int is_tap = __builtin_amdgcn_readfirstlane(k_beg / nch);
    int is_chunk = __builtin_amdgcn_readfirstlane(k_beg - is_tap * nch);
    __syncthreads();                                       // tap table visible
    unsigned is_voff = tap_voff(is_tap);
    auto issue = [&](int k0, int buf) {
        const unsigned base = lds0 + (unsigned)(buf * BUF * 16);
#pragma unroll
        for (int i = 0; i < NAI; ++i) {
            const int d0 = (i * 4 + wave) * 64;
            const int ka = k0 + d0 / (2 * BM);
            const bool live = d0 < A_ST && ka < k_end;
            u32x4 r = ars;
            r[2] = live ? p.g8_a_bytes : 0u;
            const int soff = live ? (int)((unsigned)ka * a_step_bytes) : 0;
            const unsigned dst = base + (unsigned)(d0 * 16);
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                         :: "s"(dst), "v"(avo[i]), "s"(r), "s"(soff) : "memory");
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool live = k0 + u < k_end;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int cb = is_chunk * 2 + h;
                u32x4 r = xrs;
                const bool on = live && cb < p.g8_CB;
                r[2] = on ? p.x_bytes : 0u;
                const int soff = on ? (int)((unsigned)cb * p.g8_plane_bytes) : 0;
                const unsigned dst = base + (unsigned)((A_PAD + (u * 2 + h) * 256 + wave * 64) * 16);
                asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                             :: "s"(dst), "v"(is_voff), "s"(r), "s"(soff) : "memory");
            }
            ++is_chunk;
            if (is_chunk == nch) { is_chunk = 0; ++is_tap; is_voff = tap_voff(is_tap); }
        }
    };

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

#pragma unroll
    for (int s = 0; s < NBUF - 1; ++s) issue(k_beg + s * U, s);
    int cur = 0;
    for (int k = k_beg; k < k_end; k += U) {
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"((NBUF - 2) * NDMA) : "memory");
        __builtin_amdgcn_s_barrier();
        issue(k + (NBUF - 1) * U, cur == 0 ? NBUF - 1 : cur - 1);
        const uint4* __restrict__ sb = smem + cur * BUF;
        bf16x8 a[U][MI], b[U][NI];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int i = 0; i < MI; ++i) a[u][i] = __builtin_bit_cast(bf16x8, sb[(u * 2 + (lane >> 5)) * BM + i * 32 + (lane & 31)]);
#pragma unroll
            for (int j = 0; j < NI; ++j)
                b[u][j] = __builtin_bit_cast(bf16x8, sb[A_PAD + (u * 2 + (lane >> 5)) * 256 + wave * 64 + j * 32 + (lane & 31)]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[u][i], b[u][j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        cur = cur + 1 == NBUF ? 0 : cur + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the zero-record DMAs of the tail still write LDS

    // ---- epilogue: the mappings of conv_igemm_kernel with one row block of BM and the wave's 64 pixel columns; buffer stores with
    // per-pixel offsets for both targets (conv_store.h), rows past M masked per lane in the last row tile
    const bool direct = p.splits == 1;
    const bool yh = p.yh && direct;
    const int yes = yh ? 2 : 4;
    float* __restrict__ Yb = yh ? reinterpret_cast<float*>(reinterpret_cast<bf16_t*>(p.Y) + p.out_off_c[cls])
                                : p.Y + (long)split * p.slab_stride + p.out_off_c[cls];
    const int po_t = p.po_c[cls][0], po_y = p.po_c[cls][1], po_x = p.po_c[cls][2];
    unsigned voff[NI], voff2[NI];
    bool ring = false;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int q = n0 + wave * 64 + j * 32 + (lane & 31);
        int n, ot, oy, ox;
        decompose_pix(q < p.Npix ? q : 0, p, n, ot, oy, ox);
        const long e = (long)n * p.out_sn + (long)ot * p.out_st + (long)oy * p.out_sh + (long)ox * p.out_sw +
                       4L * (lane >> 5) * p.out_sc;
        voff[j] = q < p.Npix ? (unsigned)(e * yes) : 0x80000000u;
        voff2[j] = 0x80000000u;
        if (p.Y2) {
            const int tp = ot * p.ps_t + po_t - p.lo_t, yp = oy * p.ps_y + po_y - p.lo_y, xp = ox * p.ps_x + po_x - p.lo_x;
            if (q < p.Npix && (unsigned)tp < (unsigned)p.ext_t && (unsigned)yp < (unsigned)p.ext_y &&
                (unsigned)xp < (unsigned)p.ext_x) {
                const long e2 = (long)n * p.y2_sn + (long)tp * p.y2_st + (long)yp * p.y2_sh + xp + 4L * (lane >> 5) * p.y2_sc;
                voff2[j] = (unsigned)(e2 * yes);
                voff[j] = 0x80000000u;
            }
        }
        ring = ring || voff[j] != 0x80000000u;
    }
    if (m0 + BM <= p.M) {
        if (p.Y2) c2m_store_tile_fast<MI, NI>(acc, p.Y2, voff2, m0, p.y2_sc, nullptr, false, 0, 0.f, lane, yh);
        if (!p.Y2 || __any(ring))
            c2m_store_tile_fast<MI, NI>(acc, Yb, voff, m0, p.out_sc, p.bias, direct, p.act, p.slope, lane, yh);
    } else {
        if (p.Y2) c2m_store_tile_fast<MI, NI, true>(acc, p.Y2, voff2, m0, p.y2_sc, nullptr, false, 0, 0.f, lane, yh, p.M);
        if (!p.Y2 || __any(ring))
            c2m_store_tile_fast<MI, NI, true>(acc, Yb, voff, m0, p.out_sc, p.bias, direct, p.act, p.slope, lane, yh, p.M);
    }
}

// variant: geom[C2M_G_G8_VARIANT] (0 = the rule below, or one of the rule's choices 1, 3, 5); p.g8_* are filled and validated by c2m_conv_igemm
int c2m_launch_gather_nc8(const ConvP& p, int variant, int splits, hipStream_t s) {
    const unsigned ptiles = (unsigned)c2m_cdiv(p.Npix, 256);
    int v = variant;
    // (kernel trace on one box, seven variants per shape: 64-row tiles 2 stages x 3 workgroups per CU >= 3 stages x 2 everywhere
    // (45-row (4,4,4) data gradient 160 vs 209 us); 128-row tiles: 3 stages of 2 K-steps within 3 % of 4 stages of 1; <= 32 rows:
    // 4 K-steps per stage.  The losers are no longer instantiated; the numbers of the survivors are unchanged.)
    if (v == 0) v = p.M <= 32 ? 1 : ((p.M <= 64 || (p.M % 128 >= 1 && p.M % 128 <= 64)) ? 5 : 3);
#define G8_LAUNCH(BM, UU, NB, WG) do {                                                                                     \
        dim3 grid(ptiles * (unsigned)c2m_cdiv(p.M, BM) * (unsigned)(splits * p.ncls));                                      \
        hipLaunchKernelGGL((conv_gather_nc8_kernel<BM, UU, NB, WG>), grid, dim3(256), 0, s, p); } while (0)
    switch (v) {
        case 1: G8_LAUNCH(32, 4, 2, 2); break;         // (rows, K-steps per stage, stages, workgroups per CU)
        case 3: G8_LAUNCH(128, 2, 3, 2); break;
        case 5: G8_LAUNCH(64, 2, 2, 3); break;
        default: return (int)hipErrorInvalidValue;
    }
#undef G8_LAUNCH
    return (int)hipGetLastError();
}
