// Implicit-GEMM convolution for gfx950 (CDNA4) on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32, exact f32).
//
// Replaces the ATen conv2d/conv3d (+ explicit ReflectionPad2d/3d) calls of the reference blocks:
//   src/modules/layers/down_block.py:14-23,35-47  same_block.py:14-23,36-46,55-67  up_block.py:9-13
//   residual_block.py:13-31,42-71  spade_block.py:47-49  vgg.py (torchvision features)  generator.py:76-78
//
// One kernel serves forward and data-gradient:  D[m][pix] = sum_k A[m][k] * G(k, pix)
//   * K is ordered (channel chunk, tap group, tap, channel-in-chunk): one K-step (16 deep) = NS taps x CK channels
//     (NS*CK = 16).  The spatial part of the gather (o*stride + tap offset, zero / reflect boundary) is therefore
//     computed once per tap per K-step and the CK channel loads only add a channel stride: ~2 VALU per element.
//   * A  : row-major [M][K] weights packed by the host into that K order (zero rows for channel / tap padding).
//   * D  : written with arbitrary output strides (NCHW / NCTHW, or the strided parity classes of a dgrad).
//   * split-K over gridDim.z for layers with few output pixels (deep encoder layers: 2x4 maps, K up to 16384):
//     partial slabs + a fixed-order reduction that also applies bias / activation (no float atomics).
// Orientation: the MFMA column index (lane&31) is the pixel, so every accumulator register is stored as 2 x 128
// contiguous bytes per wave -> coalesced NCHW stores.
//
// Tiling: 256 threads = 4 waves, BK = 16, register-prefetched + double-buffered LDS, one barrier per K-step.
//
// c2m_conv_igemm is also the entry point of the other forward / data-gradient kernel families and routes to their launchers
// (conv_common.h): the NC8 gather form (conv_gather.hip), the LDS-patch 3x3 kernels (conv_patch.hip) and the <= 4-row
// vector-ALU kernels (conv_thin.hip).  The weight gradient is conv_wgrad.hip, the reflect fold conv_fold.hip, the weight
// packing conv_pack.hip.
#include "conv_common.h"
#include <stdlib.h>
#include <string.h>

// PREC = 0: fp32 operands on the fp32 MFMA.  PREC = 1 (BF): bf16 operands (X is a bf16 tensor in HBM -- the bf16 data path --, weights are rounded to bf16, RNE, while they
// are staged into LDS; fp32 accumulation; fp32 or bf16 output, ConvP::yh) on v_mfma_f32_32x32x16_bf16 -- one instruction per 16-deep K-step and 32x32 tile.  LDS
// image [k half h][row][8 bf16] (16 B per lane, conflict-free ds_read_b128).  The K slot order inside a step is
// permuted identically for A and B so that each gathering thread's values are contiguous: slot(k) = (k % BROWS) *
// BPASS + k / BROWS (a sum over k does not care about the order).
//
// PREC = 2: split operands.  X and the weights are fp32 in HBM and are gathered exactly as in the fp32 form (same K order,
// table, buffer gather, split-K, class batching and epilogue); each value is split into three bf16 pieces (c2m_split3) when it
// is stored into LDS -- three images [piece][k half][row][8 bf16] per operand in the bf16 form's slot order -- and a 16-deep
// K-step of a 32x32 tile is the six products a0b0 a0b1 a1b0 a0b2 a1b1 a2b0 on v_mfma_f32_32x32x16_bf16: 6 x 32 cycles against
// 8 x 64 on the fp32 pipe.  The dropped products are below 2^-24 of the result.  The four low-order products have
// an accumulator of their own (s6/lo4 of profiles/split_bf16_numerics.txt), so the 128-row tile holds 128 accumulator registers:
// its launch bound asks for two waves per SIMD (203 VGPRs, no scratch; unbounded it took 261 and one wave).  LDS: 48 KB (128-row
// tile), 36 KB (64-row), 54 KB (32-row).
template <int BM, int BN, int WGM, int WGN, int NS, int U, int PREC = 0>
__global__ __launch_bounds__(256, (PREC == 2 && BM == 128) ? 2 : 1) void conv_igemm_kernel(const ConvP p) {
    constexpr bool BF = PREC == 1, SP = PREC == 2, HALF = BF || SP;     // HALF: bf16 LDS images
    constexpr int NP = SP ? 3 : 1;                                       // pieces per operand
    // U = table K-steps (16 deep each) staged per barrier: U = 2 halves the barriers per MFMA at twice the LDS
    constexpr int BK = 16, CK = BK / NS, BKU = BK * U;
    constexpr int TM = BM / WGM, TN = BN / WGN, MI = TM / 32, NI = TN / 32;
    constexpr int LDA_S = BM + 4, LDB_S = BN;
    constexpr int BROWS = 256 / BN;           // k rows gathered per pass
    constexpr int BPASS = BK / BROWS;         // gathers per thread per K-step
    constexpr int A_F4 = BM * BK / 4;         // float4 loads per K-step (whole block)
    constexpr int APASS = (A_F4 + 255) / 256;
    static_assert(WGM * WGN == 4 && BN >= 64 && CK % BROWS == 0, "tile");
    static_assert(!HALF || BROWS <= 2, "bf16 slot packing is written for BN = 128 / 256");
    __shared__ float sA[HALF ? 1 : 2][HALF ? 1 : BKU][HALF ? 1 : LDA_S];
    __shared__ float sB[HALF ? 1 : 2][HALF ? 1 : BKU][HALF ? 1 : LDB_S];
    __shared__ uint4 hA[HALF ? 2 * U * NP * 2 * BM : 1];      // [buf][u][piece][h][row] x 8 bf16
    __shared__ uint4 hB[HALF ? 2 * U * NP * 2 * BN : 1];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    // XCD-aware order (common.h): the row tiles of one pixel tile gather the same pixels, neighbouring pixel tiles share taps
    const C2mBlock blk = c2m_xcd_block((unsigned)(p.Npix + BN - 1) / BN, (unsigned)(p.M + BM - 1) / BM, 1);
    const int m0 = blk.y * BM, n0 = blk.x * BN;
    const int cls = p.ncls > 1 ? (int)blk.z / p.splits : 0;
    const int split = p.ncls > 1 ? (int)blk.z - cls * p.splits : (int)blk.z;
    const float* __restrict__ Acls = p.A + cls * p.a_cls;
    const int4* __restrict__ ktab = p.ktab + cls * p.ktab_cls;
    const int kt_beg = split * p.ksteps_per_split;
    int kt_end = kt_beg + p.ksteps_per_split; kt_end = kt_end < p.nk ? kt_end : p.nk;

    // ---- gather side: this thread owns one pixel column of the tile
    const int bp = tid % BN;
    const int brow0 = __builtin_amdgcn_readfirstlane(tid / BN);
    int pn, pt, py, px;
    {
        int pix = n0 + bp; pix = pix < p.Npix ? pix : p.Npix - 1;
        decompose_pix(pix, p, pn, pt, py, px);
    }
    const int ots = pt * p.st, oys = py * p.sh, oxs = px * p.sw;
    const int in_st = (int)p.in_st, in_sh = (int)p.in_sh;

    // ---- weight side: float4 along k
    const int akq = (tid & 3) * 4;
    const int arow = tid >> 2;

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // split: the four low-order products accumulate apart and are added once at the end, so the main accumulator is rounded
    // twice per K-step instead of six times (profiles/split_bf16_numerics.txt: 1.7x less error at K = 16384)
    f32x16 lo[SP ? MI : 1][SP ? NI : 1];
    if constexpr (SP) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) lo[i][j][r] = 0.f;
    }

    float4 ra[U][APASS];
    float rb[BF ? 1 : U][BF ? 1 : BPASS];
    unsigned short rh[BF ? U : 1][BF ? BPASS : 1];     // BF: X is bf16 in HBM, gathered as raw 16-bit values
    constexpr int XES = BF ? 2 : 4;                     // bytes per gathered element

    // per-thread weight row pointers (fixed for the whole K loop)
    const float* __restrict__ aptr[APASS];
#pragma unroll
    for (int s = 0; s < APASS; ++s) {
        int row = m0 + arow + s * 64; row = row < p.M ? row : p.M - 1;
        aptr[s] = Acls + (long)row * p.lda + akq;
    }
    // gather table of the NEXT K-step to load, fetched one step ahead (scalar loads: their latency must not sit in
    // front of the address arithmetic)
    int4 t_hdr, t_tap[NS];
    auto fetch_table = [&](int kt) {
        const int4* __restrict__ kd = ktab + (long)kt * (1 + NS);
        t_hdr = kd[0];
#pragma unroll
        for (int q = 0; q < NS; ++q) t_tap[q] = kd[1 + q];
    };

    // B gather through a raw buffer descriptor: per element the VECTOR offset is the per-tap spatial byte offset of
    // this lane (computed once per tap) and the SCALAR offset is the channel offset (SALU only); padding taps and
    // lanes outside the image carry an out-of-range voffset and read 0 -- no per-element VALU at all.
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.X), 0, p.x_bytes, 0x00020000);
    const unsigned img_byte = (unsigned)(pn * (int)p.in_sn) * (unsigned)XES;
    // one 16-deep table step into register set u; kt >= kt_end (odd tail of a U = 2 pair) loads zeros
    auto load_step = [&](int kt, float4 (&fa)[APASS], float (&fb)[BF ? 1 : BPASS], unsigned short (&fh)[BF ? BPASS : 1]) {
        const bool real = kt < kt_end;
#pragma unroll
        for (int s = 0; s < APASS; ++s) {
            if (A_F4 >= 256 || arow + s * 64 < BM)
                fa[s] = real ? *reinterpret_cast<const float4*>(aptr[s] + kt * BK) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const int4 hdr = t_hdr;
        unsigned vo[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            const int so = spatial_off(t_tap[q], ots, oys, oxs, p.Ti, p.Hi, p.Wi, in_st, in_sh, p.reflect, p.is3d);
            vo[q] = (real && so >= 0) ? img_byte + (unsigned)so * (unsigned)XES : C2M_OOB;
        }
#pragma unroll
        for (int s = 0; s < BPASS; ++s) {
            const int slot = (s * BROWS) / CK;                       // compile-time
            const int cc = (s * BROWS) % CK + brow0;                  // wave-uniform
            // channels beyond nvalid only meet zero weights (A is zero-padded); they read in-range data or 0
            const int soff = (hdr.x + cc * p.in_sc) * XES;
            if constexpr (BF) fh[s] = __builtin_amdgcn_raw_buffer_load_b16(xrsrc, vo[slot], soff, 0);
            else fb[s] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, vo[slot], soff, 0));
        }
        fetch_table(kt + 1 < p.nk ? kt + 1 : p.nk - 1);
    };
    auto load_tile = [&](int kt) {
#pragma unroll
        for (int u = 0; u < U; ++u) load_step(kt + u, ra[u], rb[BF ? 0 : u], rh[BF ? u : 0]);
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if constexpr (BF) {
                __bf16* __restrict__ a8 = reinterpret_cast<__bf16*>(hA) + (long)((buf * U + u) * 2) * BM * 8;
#pragma unroll
                for (int s = 0; s < APASS; ++s) {
                    const int r = arow + s * 64;
                    if (A_F4 >= 256 || r < BM) {
                        const float4 v = ra[u][s];
                        if constexpr (BROWS == 1) {        // slot = k: 4 consecutive slots in half akq / 8
                            bf16x4 q = {(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
                            *reinterpret_cast<bf16x4*>(a8 + ((akq >> 3) * BM + r) * 8 + (akq & 7)) = q;
                        } else {                            // slot = (k & 1) * 8 + k / 2: even k -> half 0, odd k -> half 1
                            bf16x2 e = {(__bf16)v.x, (__bf16)v.z}, o = {(__bf16)v.y, (__bf16)v.w};
                            *reinterpret_cast<bf16x2*>(a8 + (0 * BM + r) * 8 + (akq >> 1)) = e;
                            *reinterpret_cast<bf16x2*>(a8 + (1 * BM + r) * 8 + (akq >> 1)) = o;
                        }
                    }
                }
                // this thread's BPASS values are slots brow0*BPASS .. +BPASS-1: whole 8-slot halves
                uint4* __restrict__ b8 = hB + (long)((buf * U + u) * 2) * BN;
#pragma unroll
                for (int hh = 0; hh < BPASS / 8; ++hh) {
                    bf16x8 q;
#pragma unroll
                    for (int e = 0; e < 8; ++e) q[e] = __builtin_bit_cast(__bf16, rh[u][hh * 8 + e]);
                    const int h = BROWS == 1 ? hh : brow0;
                    b8[h * BN + bp] = __builtin_bit_cast(uint4, q);
                }
            } else if constexpr (SP) {
                uint4* __restrict__ a8 = hA + (long)((buf * U + u) * NP * 2) * BM;
#pragma unroll
                for (int s = 0; s < APASS; ++s) {
                    const int r = arow + s * 64;
                    if (A_F4 >= 256 || r < BM) {
                        const float4 v = ra[u][s];
                        unsigned x[3], y[3], z[3], w[3];
                        c2m_split3(v.x, x[0], x[1], x[2]); c2m_split3(v.y, y[0], y[1], y[2]);
                        c2m_split3(v.z, z[0], z[1], z[2]); c2m_split3(v.w, w[0], w[1], w[2]);
#pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            unsigned* __restrict__ aq = reinterpret_cast<unsigned*>(a8 + q * 2 * BM);
                            if constexpr (BROWS == 1) {    // slot = k: 4 consecutive slots in half akq / 8
                                *reinterpret_cast<uint2*>(aq + ((akq >> 3) * BM + r) * 4 + ((akq & 7) >> 1)) =
                                    make_uint2(c2m_pack_hi(x[q], y[q]), c2m_pack_hi(z[q], w[q]));
                            } else {                        // even k -> half 0, odd k -> half 1 (the bf16 form's slots)
                                aq[(0 * BM + r) * 4 + (akq >> 2)] = c2m_pack_hi(x[q], z[q]);
                                aq[(1 * BM + r) * 4 + (akq >> 2)] = c2m_pack_hi(y[q], w[q]);
                            }
                        }
                    }
                }
                uint4* __restrict__ b8 = hB + (long)((buf * U + u) * NP * 2) * BN;
#pragma unroll
                for (int hh = 0; hh < BPASS / 8; ++hh) {
                    unsigned pc[8][3];
#pragma unroll
                    for (int e = 0; e < 8; ++e) c2m_split3(rb[u][hh * 8 + e], pc[e][0], pc[e][1], pc[e][2]);
                    const int h = BROWS == 1 ? hh : brow0;
#pragma unroll
                    for (int q = 0; q < 3; ++q)
                        b8[(q * 2 + h) * BN + bp] = make_uint4(c2m_pack_hi(pc[0][q], pc[1][q]), c2m_pack_hi(pc[2][q], pc[3][q]),
                                                               c2m_pack_hi(pc[4][q], pc[5][q]), c2m_pack_hi(pc[6][q], pc[7][q]));
                }
            } else {
#pragma unroll
                for (int s = 0; s < APASS; ++s) {
                    int r = arow + s * 64;
                    if (A_F4 >= 256 || r < BM) {
                        sA[buf][u * BK + akq + 0][r] = ra[u][s].x; sA[buf][u * BK + akq + 1][r] = ra[u][s].y;
                        sA[buf][u * BK + akq + 2][r] = ra[u][s].z; sA[buf][u * BK + akq + 3][r] = ra[u][s].w;
                    }
                }
#pragma unroll
                for (int s = 0; s < BPASS; ++s) sB[buf][u * BK + brow0 + s * BROWS][bp] = rb[u][s];
            }
        }
    };

    if (kt_beg < kt_end) {
        fetch_table(kt_beg);
        load_tile(kt_beg);
        store_tile(0);
    }
    __syncthreads();
    int cur = 0;
    for (int kt = kt_beg; kt < kt_end; kt += U) {
        const bool more = kt + U < kt_end;
        // interleaved gather issue (below): +9...14 % on the 64-row tile, a few % on the 32-row tile, nothing on the
        // 128-row tile (its 32-MFMA steps already cover the gathers with 3 blocks/CU, and it would pay 8 more VGPRs)
        constexpr bool IL = PREC == 0 && U == 1 && BM < 128;
        if (!IL && more) load_tile(kt + U);
        // all fragment reads of a 16-deep step are issued first (own registers each), so the LDS latency of k-pair
        // kk+1.. hides behind the MFMAs of kk (the compiler otherwise recycles 4 VGPRs and serialises read -> mfma)
        if constexpr (BF) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint4* __restrict__ a8 = hA + (long)((cur * U + u) * 2 + (lane >> 5)) * BM;
                const uint4* __restrict__ b8 = hB + (long)((cur * U + u) * 2 + (lane >> 5)) * BN;
                bf16x8 a[MI], b[NI];
#pragma unroll
                for (int i = 0; i < MI; ++i) a[i] = __builtin_bit_cast(bf16x8, a8[wm * TM + i * 32 + (lane & 31)]);
#pragma unroll
                for (int j = 0; j < NI; ++j) b[j] = __builtin_bit_cast(bf16x8, b8[wn * TN + j * 32 + (lane & 31)]);
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        } else if constexpr (SP) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint4* __restrict__ a8 = hA + (long)((cur * U + u) * NP * 2 + (lane >> 5)) * BM;
                const uint4* __restrict__ b8 = hB + (long)((cur * U + u) * NP * 2 + (lane >> 5)) * BN;
                bf16x8 a[3][MI], b[3][NI];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
#pragma unroll
                    for (int i = 0; i < MI; ++i) a[q][i] = __builtin_bit_cast(bf16x8, a8[q * 2 * BM + wm * TM + i * 32 + (lane & 31)]);
#pragma unroll
                    for (int j = 0; j < NI; ++j) b[q][j] = __builtin_bit_cast(bf16x8, b8[q * 2 * BN + wn * TN + j * 32 + (lane & 31)]);
                }
                // product-major: MI * NI independent accumulators between two MFMAs on the same one
#pragma unroll
                for (int q = 0; q < C2M_SPLIT_NPROD; ++q)
#pragma unroll
                    for (int i = 0; i < MI; ++i)
#pragma unroll
                        for (int j = 0; j < NI; ++j) {
                            f32x16& d = q < C2M_SPLIT_NHIGH ? acc[i][j] : lo[i][j];
                            d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[C2M_SPLIT_PA[q]][i], b[C2M_SPLIT_PB[q]][j], d, 0, 0, 0);
                        }
            }
        } else if constexpr (IL) {
            // One scheduling region per K-step: the gathers (and their address arithmetic) of the NEXT step are issued in
            // the shadow of this step's MFMAs instead of in front of them, and the fragment reads run two k-pairs ahead
            // of the MFMAs that use them.  The last step re-gathers its own (in-range) tile and drops it; the table of
            // the step after next is fetched behind the region (scalar loads share the LDS counter).
            float a[BK / 2][MI], b[BK / 2][NI];
#pragma unroll
            for (int kk = 0; kk < BK / 2; ++kk) {
                const int krow = kk * 2 + (lane >> 5);
#pragma unroll
                for (int i = 0; i < MI; ++i) a[kk][i] = sA[cur][krow][wm * TM + i * 32 + (lane & 31)];
#pragma unroll
                for (int j = 0; j < NI; ++j) b[kk][j] = sB[cur][krow][wn * TN + j * 32 + (lane & 31)];
            }
            {
                const int ktl = more ? kt + 1 : kt;
#pragma unroll
                for (int s2 = 0; s2 < APASS; ++s2)
                    if (A_F4 >= 256 || arow + s2 * 64 < BM) ra[0][s2] = *reinterpret_cast<const float4*>(aptr[s2] + ktl * BK);
                const int4 hdr = t_hdr;
                unsigned vo[NS];
#pragma unroll
                for (int q = 0; q < NS; ++q) {
                    const int so = spatial_off(t_tap[q], ots, oys, oxs, p.Ti, p.Hi, p.Wi, in_st, in_sh, p.reflect, p.is3d);
                    vo[q] = so >= 0 ? img_byte + (unsigned)so * 4u : C2M_OOB;
                }
#pragma unroll
                for (int s2 = 0; s2 < BPASS; ++s2) {
                    const int slot = (s2 * BROWS) / CK;
                    const int cc = (s2 * BROWS) % CK + brow0;
                    rb[0][s2] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                        xrsrc, vo[slot], (hdr.x + cc * p.in_sc) * 4, 0));
                }
            }
#pragma unroll
            for (int kk = 0; kk < BK / 2; ++kk)
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk][i], b[kk][j], acc[i][j], 0, 0, 0);
            constexpr int NMF = (BK / 2) * MI * NI, RPM = (MI + NI + MI * NI - 1) / (MI * NI);
            __builtin_amdgcn_sched_group_barrier(0x100, 2 * (MI + NI), 0);        // two k-pairs of fragment reads
#pragma unroll
            for (int g = 0; g < NMF; ++g) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, RPM, 0);
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
                __builtin_amdgcn_sched_group_barrier(0x004, 2, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            fetch_table(kt + 2 < p.nk ? kt + 2 : p.nk - 1);
        } else
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float a[BK / 2][MI], b[BK / 2][NI];
#pragma unroll
            for (int kk = 0; kk < BK / 2; ++kk) {
                const int krow = u * BK + kk * 2 + (lane >> 5);
#pragma unroll
                for (int i = 0; i < MI; ++i) a[kk][i] = sA[cur][krow][wm * TM + i * 32 + (lane & 31)];
#pragma unroll
                for (int j = 0; j < NI; ++j) b[kk][j] = sB[cur][krow][wn * TN + j * 32 + (lane & 31)];
            }
#ifdef C2M_IGEMM_SERIAL_FRAGS
            __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
            for (int kk = 0; kk < BK / 2; ++kk) {
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk][i], b[kk][j], acc[i][j], 0, 0, 0);
            }
#ifndef C2M_IGEMM_SERIAL_FRAGS
            // fragment reads two k-pairs ahead of the MFMAs that use them: only the first reads of a K-step are waited for
            {
                constexpr int NMF = (BK / 2) * MI * NI, RPM = (MI + NI + MI * NI - 1) / (MI * NI);
                __builtin_amdgcn_sched_group_barrier(0x100, MI + NI, 0);
#pragma unroll
                for (int g = 0; g < NMF; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, RPM, 0);
                }
            }
#endif
            __builtin_amdgcn_sched_barrier(0);
        }
        if (more) store_tile(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

    if constexpr (SP) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j) acc[i][j] += lo[i][j];
    }
    // ---- epilogue: acc[i][j][r] -> row m = ..(r&3)+8*(r>>2)+4*(lane>>5), col pix = ..(lane&31)
    const bool direct = p.splits == 1;
    const bool yh = BF && p.yh && direct;                 // bf16 output elements (slabs are fp32)
    const int yes = yh ? 2 : 4;
    float* __restrict__ Yb = yh ? reinterpret_cast<float*>(reinterpret_cast<bf16_t*>(p.Y) + p.out_off_c[cls])
                                : p.Y + (long)split * p.slab_stride + p.out_off_c[cls];
    const int po_t = p.po_c[cls][0], po_y = p.po_c[cls][1], po_x = p.po_c[cls][2];
    {
        const int row0 = __builtin_amdgcn_readfirstlane(m0 + wm * TM);
        if (row0 + MI * 32 <= p.M) {
            // two targets (reflect data gradient): a pixel goes either to the interior tensor Y2 or, on the pad ring, to Y;
            // each target is one pass of stores with the other target's pixels out of range, and the ring pass is
            // skipped by the waves that hold no ring pixel (most of them)
            unsigned voff[NI], voff2[NI];
            bool ring = false;
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const int pix = n0 + wn * TN + j * 32 + (lane & 31);
                int n, ot, oy, ox;
                decompose_pix(pix < p.Npix ? pix : 0, p, n, ot, oy, ox);
                const long e = (long)n * p.out_sn + (long)ot * p.out_st + (long)oy * p.out_sh + (long)ox * p.out_sw +
                               4L * (lane >> 5) * p.out_sc;
                voff[j] = pix < p.Npix ? (unsigned)(e * yes) : 0x80000000u;
                voff2[j] = 0x80000000u;
                if (p.Y2) {
                    const int tp = ot * p.ps_t + po_t - p.lo_t, yp = oy * p.ps_y + po_y - p.lo_y,
                              xp = ox * p.ps_x + po_x - p.lo_x;
                    if (pix < p.Npix && (unsigned)tp < (unsigned)p.ext_t && (unsigned)yp < (unsigned)p.ext_y &&
                        (unsigned)xp < (unsigned)p.ext_x) {
                        const long e2 = (long)n * p.y2_sn + (long)tp * p.y2_st + (long)yp * p.y2_sh + xp +
                                        4L * (lane >> 5) * p.y2_sc;
                        voff2[j] = (unsigned)(e2 * yes);
                        voff[j] = 0x80000000u;
                    }
                }
                ring = ring || voff[j] != 0x80000000u;
            }
            if (p.Y2) c2m_store_tile_fast<MI, NI>(acc, p.Y2, voff2, row0, p.y2_sc, nullptr, false, 0, 0.f, lane, yh);
            if (!p.Y2 || __any(ring))
                c2m_store_tile_fast<MI, NI>(acc, Yb, voff, row0, p.out_sc, p.bias, direct, p.act, p.slope, lane, yh);
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int pix = n0 + wn * TN + j * 32 + (lane & 31);
        if (pix >= p.Npix) continue;
        int n, ot, oy, ox;
        decompose_pix(pix, p, n, ot, oy, ox);
        float* ybase = Yb;                                     // element type: float, or bf16_t when yh
        long yidx = (long)n * p.out_sn + (long)ot * p.out_st + (long)oy * p.out_sh + (long)ox * p.out_sw;
        long row_stride = p.out_sc;
        if (p.Y2) {
            const int tp = ot * p.ps_t + po_t - p.lo_t, yp = oy * p.ps_y + po_y - p.lo_y,
                      xp = ox * p.ps_x + po_x - p.lo_x;
            if ((unsigned)tp < (unsigned)p.ext_t && (unsigned)yp < (unsigned)p.ext_y && (unsigned)xp < (unsigned)p.ext_x) {
                ybase = p.Y2;
                yidx = (long)n * p.y2_sn + (long)tp * p.y2_st + (long)yp * p.y2_sh + xp;
                row_stride = p.y2_sc;
            }
        }
#pragma unroll
        for (int i = 0; i < MI; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row < p.M) {
                    float v = acc[i][j][r];
                    if (direct) {
                        if (p.bias) v += p.bias[row];
                        v = c2m_act(v, p.act, p.slope);
                    }
                    if (yh) reinterpret_cast<bf16_t*>(ybase)[yidx + (long)row * row_stride] = (bf16_t)v;
                    else ybase[yidx + (long)row * row_stride] = v;
                }
            }
        }
    }
}

// out[i] = act( sum_z slab[z][i] + bias[(i / chan_stride) % M] ), fixed order
template <class T>
__global__ void splitk_reduce_kernel(const float* __restrict__ slab, T* __restrict__ out,
                                     const float* __restrict__ bias, long total, int S, long chan_stride, int M, int act,
                                     float slope) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        float acc = 0.f;
        for (int z = 0; z < S; ++z) acc += slab[(long)z * total + i];
        if (bias) acc += bias[(int)((i / chan_stride) % M)];
        c2m_st(out, i, c2m_act(acc, act, slope));
    }
}

// 16-byte form: 4 consecutive outputs share a channel when chan_stride % 4 == 0.  I = 32-bit indices whenever the slab
// fits (the bias channel needs a division per element; in 64 bits it costs more than the S loads)
template <typename I, class T = float>
__global__ void splitk_reduce_vec_kernel(const float4* __restrict__ slab, T* __restrict__ out,
                                         const float* __restrict__ bias, long total4_, int S, long chan_stride4_, int M,
                                         int act, float slope) {
    const I total4 = (I)total4_, chan_stride4 = (I)chan_stride4_;
    for (I i = blockIdx.x * (I)blockDim.x + threadIdx.x; i < total4; i += (I)gridDim.x * blockDim.x) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int z = 0; z < S; ++z) {
            const float4 v = slab[(long)z * total4_ + i];
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        if (bias) {
            const float b = bias[(int)((i / chan_stride4) % (I)M)];
            acc.x += b; acc.y += b; acc.z += b; acc.w += b;
        }
        c2m_st4(out + 4 * (long)i, make_float4(c2m_act(acc.x, act, slope), c2m_act(acc.y, act, slope), c2m_act(acc.z, act, slope),
                                               c2m_act(acc.w, act, slope)));
    }
}

// C2M_DIRECT_MATH = fp32 | split | auto (default): the matrix instruction of the fp32 launches of conv_igemm_kernel.  Read at
// every launch, as C2M_FOLD_GENERAL is.  0 fp32, 1 split, 2 auto, -1 anything else (the launch is refused).
static int direct_math() {
    const char* e = getenv("C2M_DIRECT_MATH");
    if (!e || !*e || !strcmp(e, "auto")) return 2;
    if (!strcmp(e, "fp32")) return 0;
    if (!strcmp(e, "split")) return 1;
    return -1;
}

// Split launches since the last reset, per [tile rows 32, 64, 128][NS 1, 2, 4]: one entry per PREC = 2 instantiation
constexpr int C2M_DIRECT_COUNTS = 9;
static long direct_counts[C2M_DIRECT_COUNTS];
static void direct_count(int tile, int ns) {
    __atomic_fetch_add(&direct_counts[tile * 3 + (ns == 1 ? 0 : (ns == 2 ? 1 : 2))], 1L, __ATOMIC_RELAXED);
}
C2M_API int c2m_direct_math_counts(int64_t* out, int reset) {
    for (int i = 0; i < C2M_DIRECT_COUNTS; ++i) {
        const long v = reset ? __atomic_exchange_n(&direct_counts[i], 0L, __ATOMIC_RELAXED) : __atomic_load_n(&direct_counts[i], __ATOMIC_RELAXED);
        if (out) out[i] = v;
    }
    return C2M_DIRECT_COUNTS;
}

// Does this forward / data-gradient launch run on split operands?  mode: direct_math().
// auto, from the bench step's launches timed in both modes in one job (profiles/splitbf16_conv_shape_table_{fp32,split}.txt;
// time of the fp32 launches over the time of the same launches split, summed per group):
//   128-row tile (M > 64):   K >= 256: 34 shapes, 3.81 -> 2.84 ms, 1.34x (0.95 ... 1.70);  K < 256: 2 shapes, 1.24x
//   64-row tile (M 33..64):  K >= 256: 10 shapes, 1.61 -> 1.32 ms, 1.23x (0.93 ... 1.44);  K < 256: 3 shapes, 1.01x (0.80, 0.84, 1.06)
//   32-row tile (M <= 32):   14 shapes, 2.27 -> 2.42 ms, 0.94x (0.87 ... 1.00): 12 MFMAs per wave and K-step against 18 staged
//                            elements per thread -- the gather and the split, not the matrix pipe, set its time
static bool igemm_split_pays(int mode, int M, int nk) {
    if (mode != 2) return mode == 1;
    return M > 64 || (M > 32 && nk >= 16);
}

// prec: 0 fp32 MFMA, 1 bf16 operands, 2 split operands (the kernel's PREC)
template <int BM, int BN, int WGM, int WGN>
static int launch_igemm(const ConvP& p, int ns, int splits, hipStream_t s, int prec) {
    dim3 grid((unsigned)c2m_cdiv(p.Npix, BN) * c2m_cdiv(p.M, BM) * splits * p.ncls);
    constexpr int U = 1;
    if (prec == 1) {
        constexpr int UB = 2;      // bf16: 4 MFMAs per 16-deep step and wave, so two steps per barrier
        switch (ns) {
            case 1: hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WGM, WGN, 1, UB, 1>), grid, dim3(256), 0, s, p); break;
            case 2: hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WGM, WGN, 2, UB, 1>), grid, dim3(256), 0, s, p); break;
            case 4: hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WGM, WGN, 4, UB, 1>), grid, dim3(256), 0, s, p); break;
            default: return (int)hipErrorInvalidValue;
        }
        return (int)hipGetLastError();
    }
    if (prec == 2) {               // split: 6 * MI * NI MFMAs per 16-deep step and wave, one step per barrier
        switch (ns) {
            case 1: hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WGM, WGN, 1, U, 2>), grid, dim3(256), 0, s, p); break;
            case 2: hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WGM, WGN, 2, U, 2>), grid, dim3(256), 0, s, p); break;
            case 4: hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WGM, WGN, 4, U, 2>), grid, dim3(256), 0, s, p); break;
            default: return (int)hipErrorInvalidValue;
        }
        direct_count(BM == 32 ? 0 : (BM == 64 ? 1 : 2), ns);
        return (int)hipGetLastError();
    }
    switch (ns) {
        case 1: hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WGM, WGN, 1, U>), grid, dim3(256), 0, s, p); break;
        case 2: hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WGM, WGN, 2, 1>), grid, dim3(256), 0, s, p); break;
        case 4: hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WGM, WGN, 4, 1>), grid, dim3(256), 0, s, p); break;
        default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

static void igemm_tile(int M, int& BM, int& BN) {
    if (M <= 32) { BM = 32; BN = 256; }
    else if (M <= 64) { BM = 64; BN = 128; }
    else { BM = 128; BN = 128; }
}

// Number of K splits the launch will use (the caller sizes the slab = splits * slab_stride floats when > 1).
// Blocks are dispatched dynamically, so a grid only loses time when it is too small to keep every CU busy to the end:
// below ~4 blocks per CU the K loop is split until there are ~5 per CU (e.g. 640 tiles = 2.5/CU would leave the CUs
// that got 2 blocks idle for a third of the launch).
C2M_API int c2m_conv_igemm_splits(int M, int nk, int Npix) {
    int BM, BN;
    igemm_tile(M, BM, BN);
    const long tiles = (long)c2m_cdiv(M, BM) * c2m_cdiv(Npix, BN);
    constexpr long target = 1280;             // ~5 blocks per CU
    if (tiles >= 768 || nk < 8) return 1;
    long S = (target + tiles - 1) / tiles;
    if (S > nk / 4) S = nk / 4;
    if (S > 128) S = 128;
    if (S < 2) return 1;
    const int per = c2m_cdiv(nk, (int)S);
    return c2m_cdiv(nk, per);                 // every split owns >= 1 K-step
}

// geom[] layout (int64): see include/c2m_hip.h
C2M_API int c2m_conv_igemm(const float* A, const void* X, void* Y, void* Y_interior, const float* bias,
                           const int* ktab, const int64_t* g, int act, float slope, void* stream) {
    C2M_ENTER();
    ConvP p;
    p.A = A; p.X = (const float*)X; p.Y = (float*)Y; p.bias = bias; p.ktab = reinterpret_cast<const int4*>(ktab);
    p.Y2 = (float*)Y_interior;
    p.ps_t = (int)g[C2M_G_PS_T]; p.ps_y = (int)g[C2M_G_PS_Y]; p.ps_x = (int)g[C2M_G_PS_X]; p.po_t = (int)g[C2M_G_PO_T]; p.po_y = (int)g[C2M_G_PO_Y];
    p.po_x = (int)g[C2M_G_PO_X]; p.lo_t = (int)g[C2M_G_LO_T]; p.lo_y = (int)g[C2M_G_LO_Y]; p.lo_x = (int)g[C2M_G_LO_X]; p.ext_t = (int)g[C2M_G_EXT_T];
    p.ext_y = (int)g[C2M_G_EXT_Y]; p.ext_x = (int)g[C2M_G_EXT_X]; p.y2_sn = g[C2M_G_Y2_SN]; p.y2_sc = g[C2M_G_Y2_SC]; p.y2_st = g[C2M_G_Y2_ST]; p.y2_sh = g[C2M_G_Y2_SH];
    p.M = (int)g[C2M_G_M]; p.nk = (int)g[C2M_G_NK]; p.lda = (int)g[C2M_G_LDA];
    p.Npix = (int)g[C2M_G_NPIX]; p.To = (int)g[C2M_G_TO]; p.Ho = (int)g[C2M_G_HO]; p.Wo = (int)g[C2M_G_WO];
    p.Ti = (int)g[C2M_G_TI]; p.Hi = (int)g[C2M_G_HI]; p.Wi = (int)g[C2M_G_WI];
    p.st = (int)g[C2M_G_ST]; p.sh = (int)g[C2M_G_SH]; p.sw = (int)g[C2M_G_SW];
    p.in_sn = g[C2M_G_IN_SN]; p.in_st = g[C2M_G_IN_ST]; p.in_sh = g[C2M_G_IN_SH];
    p.out_sn = g[C2M_G_OUT_SN]; p.out_sc = g[C2M_G_OUT_SC]; p.out_st = g[C2M_G_OUT_ST]; p.out_sh = g[C2M_G_OUT_SH]; p.out_sw = g[C2M_G_OUT_SW]; p.out_off = g[C2M_G_OUT_OFF];
    p.reflect = (int)g[C2M_G_REFLECT]; p.is3d = (int)g[C2M_G_IS3D];
    const int ns = (int)g[C2M_G_NS];
    p.in_sc = (int)g[C2M_G_IN_SC];
    const int splits = (int)g[C2M_G_SPLITS];           // 1, or the value returned by c2m_conv_igemm_splits
    p.slab_stride = g[C2M_G_SLAB_STRIDE];
    if (g[C2M_G_X_BYTES] <= 0 || g[C2M_G_X_BYTES] >= 0x80000000LL) return (int)hipErrorInvalidValue;   // X must be < 2 GiB
    p.x_bytes = (unsigned)g[C2M_G_X_BYTES];
    p.act = act; p.slope = slope;
    p.xh = (int)g[C2M_G_X_TYPE]; p.yh = (int)g[C2M_G_Y_TYPE];       // element types of X and of Y / Y_interior: 0 fp32, 1 bf16 (dtype.h)
    if ((p.xh | p.yh) & ~1) return (int)hipErrorInvalidValue;
    if (p.M <= 0 || p.Npix <= 0) return 0;
    if (p.nk <= 0 || (p.lda & 3) || (((uintptr_t)A) & 15) || splits < 1) return (int)hipErrorInvalidValue;
    if (p.Y2 && splits != 1) return (int)hipErrorInvalidValue;   // the two-target epilogue is a direct-store feature
    p.ksteps_per_split = c2m_cdiv(p.nk, splits);
    if (!g[C2M_G_PATCH] && c2m_cdiv(p.nk, p.ksteps_per_split) != splits) return (int)hipErrorInvalidValue;   // empty split
    p.splits = splits;
    p.ncls = g[C2M_G_NCLS] > 1 ? (int)g[C2M_G_NCLS] : 1;
    if (p.ncls > 8) return (int)hipErrorInvalidValue;
    p.a_cls = g[C2M_G_A_CLS]; p.ktab_cls = (int)g[C2M_G_KTAB_CLS];
    p.out_off_c[0] = p.out_off; p.po_c[0][0] = p.po_t; p.po_c[0][1] = p.po_y; p.po_c[0][2] = p.po_x;
    for (int c = 0; c < p.ncls && p.ncls > 1; ++c) {
        p.out_off_c[c] = g[C2M_G_CLS_OUT_OFF + c];
        for (int d = 0; d < 3; ++d) p.po_c[c][d] = (int)g[C2M_G_CLS_PO + 3 * c + d];     // 96 .. 119 (geom[90..92] are the type / form flags)
    }
    if (p.ncls > 1 && (g[C2M_G_PATCH] || (p.a_cls & 3))) return (int)hipErrorInvalidValue;   // gather kernel only
    hipStream_t s = (hipStream_t)stream;
    if (g[C2M_G_G8] == 1) {
        // NC8 gather form (conv_gather_nc8_kernel): X = NC8 of the gathered bf16 tensor ([N][ceil(C/8)][Ti*Hi*Wi][8], geom[32] its bytes),
        // A = c2m_pack_weights_bf16_gather image(s) of this launch's first class, ktab = [ncls][taps] {dt, dy, dx, 1}, nk = taps *
        // ceil(C/16) K-steps in (tap, chunk) order; C = geom[28], taps = geom[29]; geom[C2M_G_G8_VARIANT] = tile variant (0 = rule, or 1 | 3 | 5)
        const int C = (int)g[C2M_G_CIN], taps = (int)g[C2M_G_TAPS];
        if (g[C2M_G_PRECISION] != 1 || !p.xh || g[C2M_G_PATCH] || C <= 0 || taps <= 0 || taps > 64 || (((uintptr_t)A | (uintptr_t)X) & 15))
            return (int)hipErrorInvalidValue;
        p.g8_nch = c2m_cdiv(C, 16); p.g8_ntaps = taps; p.g8_CB = c2m_cdiv(C, 8); p.g8_Mpad = c2m_cdiv(p.M, 128) * 128;
        if (p.nk != taps * p.g8_nch || p.in_st != (long)p.Hi * p.Wi || p.in_sh != p.Wi) return (int)hipErrorInvalidValue;
        const long plane = (long)p.Ti * p.Hi * p.Wi * 16, ab = (long)p.nk * 2 * p.g8_Mpad * 16;
        if (plane * p.g8_CB > (long)p.x_bytes || p.x_bytes % (plane * p.g8_CB) || ab * p.ncls >= 0x80000000LL)
            return (int)hipErrorInvalidValue;
        p.g8_plane_bytes = (unsigned)plane; p.g8_a_bytes = (unsigned)ab;
        if (g[C2M_G_G8_VARIANT] < 0 || g[C2M_G_G8_VARIANT] > 5) return (int)hipErrorInvalidValue;
        return c2m_launch_gather_nc8(p, (int)g[C2M_G_G8_VARIANT], splits, s);
    }
    if (g[C2M_G_PATCH]) {                                           // LDS-patch path (3x3 stride 1, chosen by the host plan)
        if (ns != 1 || p.st != 1 || p.sh != 1 || p.sw != 1) return (int)hipErrorInvalidValue;
        p.iy0 = (int)g[C2M_G_PATCH_IY0]; p.ix0 = (int)g[C2M_G_PATCH_IX0];
        for (int i = 0; i < 3; ++i) { p.pty[i] = (int)g[C2M_G_PATCH_TY + i]; p.ptx[i] = (int)g[C2M_G_PATCH_TX + i]; }
        p.nchunks = p.nk / 9;
        p.cin = (int)g[C2M_G_CIN];
        if (p.nchunks * 9 != p.nk || p.cin <= 0 || p.cin > p.nchunks * 16) return (int)hipErrorInvalidValue;
        p.ksteps_per_split = c2m_cdiv(p.nchunks, splits);           // chunks per split
        if (c2m_cdiv(p.nchunks, p.ksteps_per_split) != splits) return (int)hipErrorInvalidValue;
        if (g[C2M_G_PRECISION] == 1) {
            // bf16: A = c2m_pack_weights_bf16_patch output, lda = its padded row count (a multiple of 128); X is bf16
            if (p.lda % 128 != 0 || p.lda < p.M || !p.xh) return (int)hipErrorInvalidValue;
            return c2m_launch_patch_bf16(p, splits, s);
        }
        if (p.xh || p.yh) return (int)hipErrorInvalidValue;        // the fp32 kernels read and write fp32
        return c2m_launch_patch(p, splits, s);
    }
    if (p.M <= 4 && splits == 1 && p.Npix >= 16384 && !p.Y2 && p.ncls == 1) {      // thin output: vector-ALU kernel
        if (p.xh || p.yh) return (int)hipErrorInvalidValue;        // fp32 in, fp32 out (the host casts bf16 activations)
        // g[C2M_G_SQUARE_KW] = +-KW: 2-D stride-1 square KW x KW tap set in row-major order (dx ascending / descending)
        const int kw = (int)(g[C2M_G_SQUARE_KW] < 0 ? -g[C2M_G_SQUARE_KW] : g[C2M_G_SQUARE_KW]);
        if (p.M <= 3 && (kw == 3 || kw == 7) && !p.is3d && p.To == 1 && p.st == 1 && p.sh == 1 && p.sw == 1 && p.Wo % 4 == 0 &&
            g[C2M_G_TAPS] == kw * kw && g[C2M_G_CIN] > 0 && g[C2M_G_CIN] * kw * kw * 16 <= 48 * 1024) {
            return c2m_launch_thin_rows(p, kw, ns, (int)g[C2M_G_NTG], (int)g[C2M_G_CIN], g[C2M_G_SQUARE_KW] < 0, s);
        }
        return c2m_launch_thin_fwd(p, ns, s);
    }
    const bool bf16 = g[C2M_G_PRECISION] == 1;                          // operand precision: 0 fp32 (exact), 1 bf16 (fp32 accumulate)
    if (bf16 ? !p.xh : (p.xh || p.yh)) return (int)hipErrorInvalidValue;   // bf16 kernels gather bf16 X; fp32 kernels are fp32 only
    // fp32 operands: the exact fp32 MFMA, or the same launch on split-bf16 operands (C2M_DIRECT_MATH)
    const int math = bf16 ? 0 : direct_math();
    if (math < 0) return (int)hipErrorInvalidValue;
    const int prec = bf16 ? 1 : (igemm_split_pays(math, p.M, p.nk) ? 2 : 0);
    if (p.M <= 32)      return launch_igemm<32, 256, 1, 4>(p, ns, splits, s, prec);
    else if (p.M <= 64) return launch_igemm<64, 128, 2, 2>(p, ns, splits, s, prec);
    else                return launch_igemm<128, 128, 2, 2>(p, ns, splits, s, prec);
}

C2M_API int c2m_splitk_reduce(const float* slab, void* out, const float* bias, long total, int splits,
                              long chan_stride, int M, int act, float slope, int dt, void* stream) {
    C2M_ENTER();
    if (total <= 0) return 0;
    const uintptr_t omask = dt == C2M_BF16 ? 7 : 15;
    const bool vec = (total & 3) == 0 && (!bias || (chan_stride & 3) == 0) && (((uintptr_t)slab) & 15) == 0 &&
                     (((uintptr_t)out) & omask) == 0;
    const dim3 grid(c2m_grid(vec ? total / 4 : total, 256));
    hipStream_t s = (hipStream_t)stream;
    C2M_DISPATCH_DT(dt,
        if (vec) {
            if (total / 4 < (1L << 31))
                hipLaunchKernelGGL((splitk_reduce_vec_kernel<unsigned, T>), grid, dim3(256), 0, s, reinterpret_cast<const float4*>(slab),
                                   (T*)out, bias, total / 4, splits, bias ? chan_stride / 4 : 1, M, act, slope);
            else
                hipLaunchKernelGGL((splitk_reduce_vec_kernel<long, T>), grid, dim3(256), 0, s, reinterpret_cast<const float4*>(slab),
                                   (T*)out, bias, total / 4, splits, bias ? chan_stride / 4 : 1, M, act, slope);
        } else {
            hipLaunchKernelGGL(splitk_reduce_kernel<T>, grid, dim3(256), 0, s, slab, (T*)out, bias, total, splits, chan_stride, M,
                               act, slope);
        });
    return (int)hipGetLastError();
}
