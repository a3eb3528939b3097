// Convolution weight gradient for gfx950 (CDNA4) on the matrix pipe: fp32 (v_mfma_f32_32x32x2_f32, exact f32) and bf16 operands.
//
// wgrad:  dW[co][j] = sum_pix dY[co][pix] * G(j, pix), rows j in (tap, channel) order so that 16 consecutive rows
// share a tap; split-K over pixels into deterministic slabs, an all-ones row gives the bias gradient; the slab
// reduction permutes back to the [Cout][Cin][taps] weight layout.
//
// c2m_conv_wgrad also launches the <= 4-row vector-ALU forms (conv_thin.hip), which write the same slab layout.
#include "conv_common.h"

template <int BM, int BN, int WGM, int WGN, int NS, bool BF = false>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const WgradP p) {
    constexpr int CK = 16 / NS;
    constexpr int BK = 64;                 // pixels per K-step (one wave-width: coalesced along pix)
    constexpr int LDS_S = BK + 1;          // odd stride: conflict-free fragment reads
    constexpr int TM = BM / WGM, TN = BN / WGN, MI = TM / 32, NI = TN / 32;
    constexpr int AROWS = BM / 4, BROWSW = BN / 4;   // rows per wave
    constexpr int BGROUPS = BROWSW / 16;              // 16-row (one tap) groups per wave
    static_assert(BROWSW % 16 == 0, "wgrad rows per wave must be whole tap groups");
    // BF: bf16 operands (dY and X rounded RNE while staged), v_mfma_f32_32x32x16_bf16 with 16 pixels per instruction;
    // LDS rows of 64 + 8 bf16 (144 B: conflict-free 16-B fragment reads)
    constexpr int LDH = BK + 8;
    __shared__ float sA[BF ? 1 : BM][BF ? 1 : LDS_S];
    __shared__ float sB[BF ? 1 : BN][BF ? 1 : LDS_S];
    __shared__ __attribute__((aligned(16))) __bf16 hA[BF ? BM : 1][BF ? LDH : 8];
    __shared__ __attribute__((aligned(16))) __bf16 hB[BF ? BN : 1][BF ? LDH : 8];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WGN, wn = wave % WGN;
    // XCD-aware order (common.h): all tiles of a pixel split read the same pixels -> one XCD, back to back
    const C2mBlock blk = c2m_xcd_block((unsigned)p.J / BN, (unsigned)(p.M + BM - 1) / BM, 0);
    const int m0 = blk.y * BM, j0 = blk.x * BN;
    const int split = blk.z;
    const int pbeg = split * p.pix_per_split;
    int pend = pbeg + p.pix_per_split; pend = pend < p.Npix ? pend : p.Npix;
    const int in_st = (int)p.in_st, in_sh = (int)p.in_sh;

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float ra[AROWS], rb[BROWSW];
    // BF: dY and X are bf16 tensors in HBM (the bf16 data path; the host casts fp32 operands once): 2-byte gathers, widened
    // to fp32 registers by a shift (exact), rounded back (exactly) when they are staged into the bf16 LDS image
    constexpr int XES = BF ? 2 : 4;
    auto ldv = [&](const __amdgpu_buffer_rsrc_t& rs, unsigned vo, int soff_elems) -> float {
        if constexpr (BF) return __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b16(rs, vo, soff_elems * 2, 0) << 16);
        else return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, vo, soff_elems * 4, 0));
    };
    // raw buffer descriptors: per-lane byte offset = this lane's pixel (out of range for dead lanes -> reads 0),
    // scalar offset = row / channel offset (SALU): no per-element VALU
    const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.dY), 0, p.dy_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.X), 0, p.x_bytes, 0x00020000);
    auto issue_loads = [&](int pk) {
        const int pix = pk + lane;
        const bool live = pix < pend;
        int n, ot, oy, ox;
        decompose_pix(live ? pix : pend - 1, p, n, ot, oy, ox);
        const int sp = (ot * p.Ho + oy) * p.Wo + ox;
        const unsigned yvo = live ? (unsigned)(n * (int)p.dy_sn + sp) * (unsigned)XES : C2M_OOB;
        const unsigned ximg = (unsigned)(n * (int)p.in_sn) * (unsigned)XES;
        const int ots = ot * p.st, oys = oy * p.sh, oxs = ox * p.sw;
#pragma unroll
        for (int s = 0; s < AROWS; ++s) {
            const int row = m0 + wave * AROWS + s;            // rows >= M give columns that are never stored
            ra[s] = ldv(yrsrc, yvo, row * (int)p.dy_sc);
        }
#pragma unroll
        for (int gq = 0; gq < BGROUPS; ++gq) {
            const int grp = (j0 + wave * BROWSW) / 16 + gq;     // < J/16 by construction of the grid
            const int4* __restrict__ jd = p.jtab + (long)grp * (1 + NS);
            const int4 hdr = jd[0];
            unsigned vo[NS];
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                const int so = spatial_off(jd[1 + q], ots, oys, oxs, p.Ti, p.Hi, p.Wi, in_st, in_sh, p.reflect, p.is3d);
                vo[q] = (live && so >= 0) ? ximg + (unsigned)so * (unsigned)XES : C2M_OOB;
            }
            if (hdr.y == -2) {                                   // ones row (bias gradient); wave-uniform branch
#pragma unroll
                for (int s = 0; s < 16; ++s) rb[gq * 16 + s] = (s == 0) ? 1.f : 0.f;
            } else {
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const int slot = s / CK, cc = s % CK;         // compile-time
                    // channels >= nvalid produce columns the reduction never reads
                    rb[gq * 16 + s] = ldv(xrsrc, vo[slot], hdr.x + cc * p.in_sc);
                }
            }
        }
    };
    // The same loads in four parts (128-row tile): each part is issued between the MFMAs of one k-group of the previous step
    // (no branch: the ones group loads through an out-of-range offset and is patched with a select).
    struct PixCtx { unsigned yvo, ximg; int ots, oys, oxs; bool live; };
    auto load_prep = [&](int pk) {
        const int pix = pk + lane;
        PixCtx c;
        c.live = pix < pend;
        int n, ot, oy, ox;
        decompose_pix(c.live ? pix : pend - 1, p, n, ot, oy, ox);
        const int sp = (ot * p.Ho + oy) * p.Wo + ox;
        c.yvo = c.live ? (unsigned)(n * (int)p.dy_sn + sp) * (unsigned)XES : C2M_OOB;
        c.ximg = (unsigned)(n * (int)p.in_sn) * (unsigned)XES;
        c.ots = ot * p.st; c.oys = oy * p.sh; c.oxs = ox * p.sw;
        return c;
    };
    auto load_a_part = [&](const PixCtx& c, int s0, int s1) {
#pragma unroll
        for (int s = s0; s < s1; ++s) {
            const int row = m0 + wave * AROWS + s;
            ra[s] = ldv(yrsrc, c.yvo, row * (int)p.dy_sc);
        }
    };
    auto load_b_group = [&](const PixCtx& c, int gq) {
        const int grp = (j0 + wave * BROWSW) / 16 + gq;
        const int4* __restrict__ jd = p.jtab + (long)grp * (1 + NS);
        const int4 hdr = jd[0];
        const bool ones = hdr.y == -2;
        unsigned vo[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            const int so = spatial_off(jd[1 + q], c.ots, c.oys, c.oxs, p.Ti, p.Hi, p.Wi, in_st, in_sh, p.reflect, p.is3d);
            vo[q] = (c.live && so >= 0 && !ones) ? c.ximg + (unsigned)so * (unsigned)XES : C2M_OOB;
        }
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int slot = s / CK, cc = s % CK;
            const float v = ldv(xrsrc, vo[slot], hdr.x + cc * p.in_sc);       // ones group: every offset is out of range -> 0
            rb[gq * 16 + s] = (s == 0 && ones) ? 1.f : v;
        }
    };
    // software pipeline (64- and 32-row tiles; +8..15 % measured): the gathers of K-step i+1 are issued in front of the
    // MFMAs of step i and are in flight while they run.  For the 128x128 tile that form is 4 % slower than loading at the
    // top of the step (64 load issues in front of the MFMAs); it interleaves the loads with the MFMAs instead (IL).
    // fp32: the loads of step i+1 (and the fragment reads of k-group g+1) are interleaved with the MFMAs of step i
    // (k-group g) below: +3.5...6 % on the 128-row tile over loading at the top of the step, +6...12 % on the 64- and
    // 32-row tiles over the PIPE form
    constexpr bool IL = !BF && BGROUPS == 2;
    constexpr bool PIPE = BM < 128 && !IL;
    issue_loads(pbeg);
    for (int pk = pbeg; pk < pend; pk += BK) {
        if (!PIPE && !IL && pk > pbeg) issue_loads(pk);
        __syncthreads();   // previous K-step's fragment reads are done
        if constexpr (BF) {
#pragma unroll
            for (int s = 0; s < AROWS; ++s) hA[wave * AROWS + s][lane] = (__bf16)ra[s];
#pragma unroll
            for (int s = 0; s < BROWSW; ++s) hB[wave * BROWSW + s][lane] = (__bf16)rb[s];
        } else {
#pragma unroll
            for (int s = 0; s < AROWS; ++s) sA[wave * AROWS + s][lane] = ra[s];
#pragma unroll
            for (int s = 0; s < BROWSW; ++s) sB[wave * BROWSW + s][lane] = rb[s];
        }
        __syncthreads();
        if (PIPE && pk + BK < pend) issue_loads(pk + BK);
        if constexpr (BF) {
#pragma unroll
            for (int kq = 0; kq < BK / 16; ++kq) {
                const int kc = kq * 16 + 8 * (lane >> 5);
                bf16x8 a[MI], b[NI];
#pragma unroll
                for (int i = 0; i < MI; ++i) a[i] = *reinterpret_cast<const bf16x8*>(&hA[wm * TM + i * 32 + (lane & 31)][kc]);
#pragma unroll
                for (int j = 0; j < NI; ++j) b[j] = *reinterpret_cast<const bf16x8*>(&hB[wn * TN + j * 32 + (lane & 31)][kc]);
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        } else
        if constexpr (IL) {
            // the fragment reads of k-group g + 1 and a part of the NEXT step's loads ride in the shadow of group g's MFMAs
            // (past the split's end every lane is out of range: zeros that are never stored)
            float a[2][8][MI], b[2][8][NI];
            auto read_group = [&](int kg, float (&fa)[8][MI], float (&fb)[8][NI]) {
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    const int kcol = (kg * 8 + kk) * 2 + (lane >> 5);
#pragma unroll
                    for (int i = 0; i < MI; ++i) fa[kk][i] = sA[wm * TM + i * 32 + (lane & 31)][kcol];
#pragma unroll
                    for (int j = 0; j < NI; ++j) fb[kk][j] = sB[wn * TN + j * 32 + (lane & 31)][kcol];
                }
            };
            read_group(0, a[0], b[0]);
            PixCtx nctx;
#pragma unroll
            for (int kg = 0; kg < BK / 16; ++kg) {
                __builtin_amdgcn_sched_barrier(0);
                if (kg + 1 < BK / 16) read_group(kg + 1, a[(kg + 1) & 1], b[(kg + 1) & 1]);
                if constexpr (AROWS == 32) {
                    if (kg == 0) { nctx = load_prep(pk + BK); load_a_part(nctx, 0, 16); }
                    else if (kg == 1) load_a_part(nctx, 16, 32);
                    else load_b_group(nctx, kg - 2);
                } else {                                   // 64- / 32-row tiles: all of dY with the first group
                    if (kg == 0) { nctx = load_prep(pk + BK); load_a_part(nctx, 0, AROWS); }
                    else if (kg <= 2) load_b_group(nctx, kg - 1);
                }
#pragma unroll
                for (int kk = 0; kk < 8; ++kk)
#pragma unroll
                    for (int i = 0; i < MI; ++i)
#pragma unroll
                        for (int j = 0; j < NI; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kg & 1][kk][i], b[kg & 1][kk][j], acc[i][j], 0, 0, 0);
                constexpr int MPG = 8 * MI * NI;           // MFMAs per k-group: 32 / 16 / 8
#pragma unroll
                for (int g = 0; g < 16; ++g) {             // per slot: MFMAs, a fragment read pair, a load (+ its addresses)
                    __builtin_amdgcn_sched_group_barrier(0x008, MPG >= 32 ? 2 : 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, MPG >= 16 ? 2 : 4, 0);
                    __builtin_amdgcn_sched_group_barrier(0x020, MPG >= 16 ? 1 : 2, 0);
                    __builtin_amdgcn_sched_group_barrier(0x006, 4, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        } else
        // fragment reads in groups of 8 k-pairs issued ahead of their MFMAs (see the igemm kernel)
#pragma unroll
        for (int kg = 0; kg < BK / 16; ++kg) {
            float a[8][MI], b[8][NI];
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                const int kcol = (kg * 8 + kk) * 2 + (lane >> 5);
#pragma unroll
                for (int i = 0; i < MI; ++i) a[kk][i] = sA[wm * TM + i * 32 + (lane & 31)][kcol];
#pragma unroll
                for (int j = 0; j < NI; ++j) b[kk][j] = sB[wn * TN + j * 32 + (lane & 31)][kcol];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < 8; ++kk)
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk][i], b[kk][j], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    float* __restrict__ out = p.slab + (long)split * p.M * p.J;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int col = j0 + wn * TN + j * 32 + (lane & 31);
        if (col >= p.J) continue;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row < p.M) out[(long)row * p.J + col] = acc[i][j][r];
            }
    }
}

// ---- bf16 data path: weight gradient with 16-byte loads (round 3) -------------------------------------------------------
// On bf16 NCHW tensors the pixel axis -- the K dimension of this GEMM -- is the contiguous one, so a lane can fetch EIGHT
// consecutive pixels of a row with one 16-byte load and put them into the [row][pixel] LDS image with one ds_write_b128: no
// transposition, no conversion.  conv_wgrad_kernel<BF> (lane = pixel) issues 64 two-byte loads + 64 ds_write_b16 per lane for
// the 16 MFMAs of a 64-pixel step and is bound by exactly that; here the same step costs 8 loads + 8 LDS writes.
// A wave-instruction covers 8 rows x 8 pixel groups (lane = rsub * 8 + grp).  X rows are (tap, channel) pairs read at the
// tap's offset: with unit x stride the 8 input pixels of a group are contiguous, at a 2-byte-granular address (unaligned
// 16-byte buffer loads are exact and full speed on gfx950: tools/micro/unaligned_b128.hip).  Only groups at a row end
// reach into the padding (taps with dx = -1 / +1): those load the aligned neighbour group and shift by one element in
// registers (v_alignbit_b32), the vacated element being 0 (zeros) or the mirrored pixel (reflect).  Rows / frames outside
// the image are whole-group zeros or mirrored by address.  Eligibility (host): sw == 1, Wi == Wo, Wo % 8 == 0, |dx| <= 1.
// Same row order, slab layout and reduction as conv_wgrad_kernel.
// SW = 2 (round 3: the 4x4 stride-2 layers of the discriminators and down blocks, a third of the bf16 weight-gradient time on
// the lane-per-pixel kernel): the 8 input pixels of a group are every second element of a 16-element run starting at
// 2*ox + dx -- two 16-byte loads and four v_perm_b32 (even halves; the odd halves when the run would start at -1 and is loaded
// from 0 instead).  dx = -1 .. 2 (4 taps, pad 1): only the first element of a left-end group (pixel -1) and the last of a
// right-end group (pixel Wi) fall into the padding.  Eligibility: sw == 2, Wi == 2*Wo, Wo % 8 == 0, -1 <= dx <= 2.
template <int BM, int BN, int WGM, int WGN, int SW = 1>
__global__ __launch_bounds__(256) void conv_wgrad_wide_bf16_kernel(const WgradP p, const int ns) {
    constexpr int BK = 64, LDH = BK + 8;
    constexpr int TM = BM / WGM, TN = BN / WGN, MI = TM / 32, NI = TN / 32;
    constexpr int AROWS = BM / 4, BROWSW = BN / 4, AP = AROWS / 8, BP = BROWSW / 8;
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) __bf16 hA[BM][LDH];
    __shared__ __attribute__((aligned(16))) __bf16 hB[BN][LDH];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WGN, wn = wave % WGN;
    const C2mBlock blk = c2m_xcd_block((unsigned)p.J / BN, (unsigned)(p.M + BM - 1) / BM, 0);
    const int m0 = blk.y * BM, j0 = blk.x * BN;
    const int split = blk.z;
    const int pbeg = split * p.pix_per_split;
    int pend = pbeg + p.pix_per_split; pend = pend < p.Npix ? pend : p.Npix;
    const int grp = lane & 7, rsub = lane >> 3;
    const int ck = 16 / ns;

    // per-lane row constants (fixed over the K loop)
    unsigned arow_off[AP];
#pragma unroll
    for (int i = 0; i < AP; ++i) arow_off[i] = (unsigned)((m0 + wave * AROWS + 8 * i + rsub) * (int)p.dy_sc) * 2u;
    unsigned b_off[BP];                                      // channel offset of the row (bytes)
    int b_dt[BP], b_dy[BP], b_dx[BP];
    bool b_on[BP], b_ones[BP];
#pragma unroll
    for (int i = 0; i < BP; ++i) {
        const int j = j0 + wave * BROWSW + 8 * i + rsub;     // < J by construction of the grid
        const int4* __restrict__ jd = p.jtab + (long)(j >> 4) * (1 + ns);
        const int4 hdr = jd[0];
        const int s16 = j & 15, slot = s16 / ck, cc = s16 - slot * ck;
        const int4 tp = jd[1 + slot];
        b_ones[i] = hdr.y == -2 && s16 == 0;
        b_on[i] = hdr.y > 0 && tp.w != 0;                    // a real (tap, channel) row; channels >= nvalid are never read back
        b_off[i] = (unsigned)((hdr.x + cc * p.in_sc)) * 2u;
        b_dt[i] = tp.x; b_dy[i] = tp.y; b_dx[i] = tp.z;
    }

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.dY), 0, p.dy_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.X), 0, p.x_bytes, 0x00020000);
    u32x4 ra[AP], rb[BP], rb2[SW == 2 ? BP : 1];
    int redge[BP];                                           // -1: the group starts one pixel left of the row, +1: ends one past it
    bool rtail[SW == 2 ? BP : 1];                            // SW = 2: the 16th element of the run lies past the row end
    auto issue = [&](int pk) {
        const int pix = pk + 8 * grp;
        const bool live = pix < pend;
        int n, ot, oy, ox;
        decompose_pix(live ? pix : pend - 8, p, n, ot, oy, ox);
        const unsigned yvo = (unsigned)(n * (int)p.dy_sn + (ot * p.Ho + oy) * p.Wo + ox) * 2u;
#pragma unroll
        for (int i = 0; i < AP; ++i)
            ra[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(yrsrc, live ? yvo + arow_off[i] : C2M_OOB, 0, 0));
        const unsigned ximg = (unsigned)(n * (int)p.in_sn) * 2u;
#pragma unroll
        for (int i = 0; i < BP; ++i) {
            int it = p.is3d ? ot * p.st + b_dt[i] : 0, iy = oy * p.sh + b_dy[i];
            const int ix0 = ox * SW + b_dx[i];
            bool ok = live && b_on[i];
            if (p.reflect) {
                if (p.is3d) { it = it < 0 ? -it : it; it = it >= p.Ti ? 2 * p.Ti - 2 - it : it; }
                iy = iy < 0 ? -iy : iy; iy = iy >= p.Hi ? 2 * p.Hi - 2 - iy : iy;
            }
            ok = ok && (unsigned)iy < (unsigned)p.Hi && (!p.is3d || (unsigned)it < (unsigned)p.Ti);
            if constexpr (SW == 1) {
                const int e = ix0 < 0 ? -1 : (ix0 + 8 > p.Wi ? 1 : 0);
                redge[i] = ok ? e : 0;
                const unsigned vo = ximg + b_off[i] + (unsigned)(it * (int)p.in_st + iy * (int)p.in_sh + (ix0 - e)) * 2u;
                rb[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xrsrc, ok ? vo : C2M_OOB, 0, 0));
            } else {
                // 16 elements from ix0 (from 0 when ix0 == -1: the wanted pixels are then the ODD elements 1, 3, .. 13 behind a
                // pad element).  A right-end run reaches up to two elements past its row: in-bounds memory (the next row) except
                // at the very end of the tensor, where the range check returns zeros -- that element is replaced in stash().
                const int e = ix0 < 0 ? -1 : (ix0 + 14 >= p.Wi ? 1 : 0);
                redge[i] = ok ? e : 0;
                // a run whose 16th element is past the row end (dx = 1, 2 in the last group of a row) loads its second half
                // one element EARLIER (elements 7 .. 14, wanted ones in the odd halves): at the end of the tensor the dword
                // (x[Wi-1], x[Wi]) straddles the buffer's range and would come back as zero, x[Wi-1] included
                const bool tail = e >= 0 && ix0 + 15 >= p.Wi;
                rtail[i] = tail;
                const unsigned vo = ximg + b_off[i] + (unsigned)(it * (int)p.in_st + iy * (int)p.in_sh + (e < 0 ? 0 : ix0)) * 2u;
                rb[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xrsrc, ok ? vo : C2M_OOB, 0, 0));
                rb2[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xrsrc, ok ? vo + (tail ? 14u : 16u) : C2M_OOB, 0, 0));
            }
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < AP; ++i)
            *reinterpret_cast<u32x4*>(&hA[wave * AROWS + 8 * i + rsub][8 * grp]) = ra[i];
        if constexpr (SW == 2) {
#pragma unroll
            for (int i = 0; i < BP; ++i) {
                const u32x4 lo = rb[i], hi = rb2[i];
                // even elements (0, 2, .. 14) of the 16-element run / odd elements (1, 3, .. 15) for a left-end group
                const unsigned hsel = rtail[i] ? 0x07060302u : 0x05040100u;      // shifted second half: the odd halves
                const u32x4 ev = {__builtin_amdgcn_perm(lo.y, lo.x, 0x05040100u), __builtin_amdgcn_perm(lo.w, lo.z, 0x05040100u),
                                  __builtin_amdgcn_perm(hi.y, hi.x, hsel), __builtin_amdgcn_perm(hi.w, hi.z, hsel)};
                const u32x4 od = {__builtin_amdgcn_perm(lo.y, lo.x, 0x07060302u), __builtin_amdgcn_perm(lo.w, lo.z, 0x07060302u),
                                  __builtin_amdgcn_perm(hi.y, hi.x, 0x07060302u), __builtin_amdgcn_perm(hi.w, hi.z, 0x07060302u)};
                // left end: (pad, x1, x3, .. x13): pad = x1 (reflect) or 0
                const unsigned padl = p.reflect ? od.x & 0xffffu : 0u;
                const u32x4 L = {(od.x << 16) | padl, __builtin_amdgcn_alignbit(od.y, od.x, 16), __builtin_amdgcn_alignbit(od.z, od.y, 16),
                                 __builtin_amdgcn_alignbit(od.w, od.z, 16)};
                // right end: the last element (pixel Wi) -> x[Wi-2] = the element before it (reflect) or 0
                const u32x4 R = {ev.x, ev.y, ev.z, (ev.w & 0xffffu) | (p.reflect ? ev.w << 16 : 0u)};
                rb[i] = redge[i] < 0 ? L : (redge[i] > 0 ? R : ev);
            }
        }
        bool any_edge = false;
#pragma unroll
        for (int i = 0; i < BP; ++i) any_edge = any_edge || (SW == 1 && redge[i] != 0);
        if (__any(any_edge)) {                               // wave-uniform: most K-steps of a wide map hold no row end
#pragma unroll
            for (int i = 0; i < BP; ++i) {
                const u32x4 v = rb[i];
                // left end: (pad, x0 .. x6) from the aligned load x0 .. x7; pad = x1 (reflect) or 0
                const unsigned padl = p.reflect ? v.x >> 16 : 0u;
                const u32x4 L = {(v.x << 16) | padl, __builtin_amdgcn_alignbit(v.y, v.x, 16), __builtin_amdgcn_alignbit(v.z, v.y, 16),
                                 __builtin_amdgcn_alignbit(v.w, v.z, 16)};
                // right end: (x[W-7] .. x[W-1], pad) from x[W-8] .. x[W-1]; pad = x[W-2] (reflect) or 0
                const unsigned padr = p.reflect ? v.w << 16 : 0u;
                const u32x4 R = {__builtin_amdgcn_alignbit(v.y, v.x, 16), __builtin_amdgcn_alignbit(v.z, v.y, 16),
                                 __builtin_amdgcn_alignbit(v.w, v.z, 16), (v.w >> 16) | padr};
                rb[i] = redge[i] < 0 ? L : (redge[i] > 0 ? R : v);
            }
        }
#pragma unroll
        for (int i = 0; i < BP; ++i) {
            const u32x4 ones = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};       // bf16 1.0 x 8 (bias gradient row)
            *reinterpret_cast<u32x4*>(&hB[wave * BROWSW + 8 * i + rsub][8 * grp]) = b_ones[i] ? ones : rb[i];
        }
    };

    issue(pbeg);
    for (int pk = pbeg; pk < pend; pk += BK) {
        __syncthreads();                                     // the previous step's fragment reads are done
        stash();
        __syncthreads();
        if (pk + BK < pend) issue(pk + BK);                  // in flight during the MFMAs below
#pragma unroll
        for (int kq = 0; kq < BK / 16; ++kq) {
            const int kc = kq * 16 + 8 * (lane >> 5);
            bf16x8 a[MI], b[NI];
#pragma unroll
            for (int i = 0; i < MI; ++i) a[i] = *reinterpret_cast<const bf16x8*>(&hA[wm * TM + i * 32 + (lane & 31)][kc]);
#pragma unroll
            for (int j = 0; j < NI; ++j) b[j] = *reinterpret_cast<const bf16x8*>(&hB[wn * TN + j * 32 + (lane & 31)][kc]);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    float* __restrict__ out = p.slab + (long)split * p.M * p.J;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int col = j0 + wn * TN + j * 32 + (lane & 31);
        if (col >= p.J) continue;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row < p.M) out[(long)row * p.J + col] = acc[i][j][r];
            }
    }
}

// dW[m][c*taps + tap] = sum_s slab[s][m][col(c, tap)] with the (chunk, tap group, slot, channel) row order;
// db[m] = sum_s slab[s][m][ones_col]
// One workgroup = 64 consecutive outputs in the slab's own (m, column) order x G groups of splits (G = 4, or 16 from 64
// splits on; wave g sums the splits s = g, g + G, ...; its 64 lanes read 256 contiguous bytes per split), the four partial sums are combined in a fixed order
// through LDS.  A thread per output with the whole S loop left a 32 x 304 layer with 256 splits on 38 workgroups of
// 256 dependent loads each (177 us for 12 MB).  The single write per output is the scattered one.
template <int G>
__global__ __launch_bounds__(64 * G) void wgrad_reduce_kernel(const float* __restrict__ slab, float* __restrict__ dW,
                                                              float* __restrict__ db, int M, int J, int Cin, int taps, int NS,
                                                              int ntg, int ngroups, int S) {
    __shared__ float part[G][64];
    const int CK = 16 / NS;
    const int used = (ngroups + 1) * 16;                  // real groups + the ones group; pad columns are skipped
    const long total = (long)M * used;
    const long per = (long)M * J;
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    for (long base = (long)blockIdx.x * 64; base < total; base += (long)gridDim.x * 64) {
        const long i = base + lane;
        long dst = -1;                                     // -1: padding / out of range, -2: bias gradient
        long src = 0;
        if (i < total) {
            // (outputs < 2^31 in practice: a 32-bit division instead of a 64-bit one per output)
            const int m = total < (1L << 31) ? (int)((unsigned)i / (unsigned)used) : (int)(i / used);
            const int col = (int)(i - (long)m * used);
            const int g = col >> 4, within = col & 15;
            if (g == ngroups) {
                if (within == 0) dst = -2 - m;
            } else {
                const int c = (g / ntg) * CK + within % CK, tap = (g % ntg) * NS + within / CK;
                if (c < Cin && tap < taps) dst = ((long)m * Cin + c) * taps + tap;
            }
            src = (long)m * J + col;
        }
        float acc = 0.f;
        if (dst != -1) {
            int sp = grp;
            for (; sp + 3 * G < S; sp += 4 * G) {          // four independent loads in flight
                const float v0 = slab[(long)sp * per + src], v1 = slab[(long)(sp + G) * per + src];
                const float v2 = slab[(long)(sp + 2 * G) * per + src], v3 = slab[(long)(sp + 3 * G) * per + src];
                acc += v0; acc += v1; acc += v2; acc += v3;
            }
            for (; sp < S; sp += G) acc += slab[(long)sp * per + src];
        }
        __syncthreads();                                   // the previous round's reads of `part` are done
        part[grp][lane] = acc;
        __syncthreads();
        if (grp == 0 && dst != -1) {
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < G; q += 4) v += (part[q][lane] + part[q + 1][lane]) + (part[q + 2][lane] + part[q + 3][lane]);
            if (dst <= -2) { if (db) db[-2 - dst] = v; }
            else dW[dst] = v;
        }
    }
}

// Few splits, many outputs (the deep layers): one workgroup per (output row m, channel chunk).  The chunk's ntg * 16 slab
// columns are summed over the splits with coalesced reads into LDS, then written as ONE contiguous run of CK * taps floats of
// dW (the per-output form above scatters its 4-byte writes with a stride of `taps` floats: 16x write amplification, 85 us
// on the 512 x 8192 layers).  blockIdx.x == nch handles the bias column.
__global__ __launch_bounds__(256) void wgrad_reduce_rows_kernel(const float* __restrict__ slab, float* __restrict__ dW,
                                                                float* __restrict__ db, int M, int J, int Cin, int taps,
                                                                int lns, int ntg, int ngroups, int S) {
    extern __shared__ float val[];                           // ntg * 16 column sums of this (m, chunk)
    const int NS = 1 << lns, lck = 4 - lns, CK = 16 >> lns;
    const int m = blockIdx.y, chunk = blockIdx.x;
    const int nch = ngroups / ntg;
    const long per = (long)M * J;
    const float* __restrict__ row = slab + (long)m * J;
    if (chunk == nch) {                                       // bias gradient: the ones group's first column
        if (db && threadIdx.x == 0) {
            float acc = 0.f;
            for (int sp = 0; sp < S; ++sp) acc += row[(long)sp * per + ngroups * 16];
            db[m] = acc;
        }
        return;
    }
    const int ncols = ntg * 16, col0 = chunk * ncols;
    for (int c = threadIdx.x; c < ncols; c += 256) {
        float acc = 0.f;
        int sp = 0;
        for (; sp + 3 < S; sp += 4) {
            const float v0 = row[(long)sp * per + col0 + c], v1 = row[(long)(sp + 1) * per + col0 + c];
            const float v2 = row[(long)(sp + 2) * per + col0 + c], v3 = row[(long)(sp + 3) * per + col0 + c];
            acc += v0; acc += v1; acc += v2; acc += v3;
        }
        for (; sp < S; ++sp) acc += row[(long)sp * per + col0 + c];
        val[c] = acc;
    }
    __syncthreads();
    const int cbase = chunk * CK;
    int nc = Cin - cbase; nc = nc < CK ? nc : CK;             // real channels of this chunk
    float* __restrict__ dst = dW + ((long)m * Cin + cbase) * taps;
    for (int o = threadIdx.x; o < nc * taps; o += 256) {
        const int cl = o / taps, tap = o - cl * taps;
        dst[o] = val[((tap >> lns) << 4) + ((tap & (NS - 1)) << lck) + cl];
    }
}

static int launch_wgrad_reduce(long total, hipStream_t s, const float* slab, float* dW, float* db, int M, int J, int Cin,
                               int taps, int NS, int ntg, int ngroups, int S) {
    const int lns = NS == 1 ? 0 : (NS == 2 ? 1 : 2);
    if (S < 64 && ntg > 0 && ngroups % ntg == 0 && (long)ntg * 16 * 4 <= 48 * 1024 && M <= 65535 && total >= (1L << 16)) {
        dim3 grid(ngroups / ntg + 1, M);
        hipLaunchKernelGGL(wgrad_reduce_rows_kernel, grid, dim3(256), (size_t)ntg * 16 * sizeof(float), s, slab, dW, db, M, J,
                           Cin, taps, lns, ntg, ngroups, S);
        return (int)hipGetLastError();
    }
    if (S >= 64)
        hipLaunchKernelGGL(wgrad_reduce_kernel<16>, dim3(c2m_grid(total, 64)), dim3(1024), 0, s, slab, dW, db, M, J, Cin, taps,
                           NS, ntg, ngroups, S);
    else
        hipLaunchKernelGGL(wgrad_reduce_kernel<4>, dim3(c2m_grid(total, 64)), dim3(256), 0, s, slab, dW, db, M, J, Cin, taps,
                           NS, ntg, ngroups, S);
    return (int)hipGetLastError();
}

constexpr int WG64_BN = 128;      // slab rows per workgroup of the 64-row tile (wgrad_tile and the launches below agree)
static void wgrad_tile(int M, int& BM, int& BN) {
    if (M <= 32) { BM = 32; BN = 128; }
    else if (M <= 64) { BM = 64; BN = WG64_BN; }
    else { BM = 128; BN = 128; }
}

// Number of pixel splits the wgrad launch will use for (M, J, Npix): the caller sizes `slab` = S*M*J floats.
C2M_API int c2m_conv_wgrad_splits(int M, int J, int Npix) {
    int BM, BN;
    wgrad_tile(M, BM, BN);
    const long tiles = (long)c2m_cdiv(M, BM) * c2m_cdiv(J, BN);
    // One resident round: blocks <= CUs x blocks/CU (LDS-limited: 2 for the 128x128 tile, 3 otherwise), so no block
    // is left to run alone after the others (a 1026-block grid on 512 slots costs a third round for 2 blocks).
    const long slots = 256L * (BM == 128 ? 2 : 3);
    long S = slots / tiles;
    const long maxS = (Npix + 1023) / 1024;   // at least 1024 pixels (16 K-steps) per split
    if (S > maxS) S = maxS;
    if (S < 1) S = 1;
    return (int)S;
}

// Rows of the slab (a multiple of the tile width) for a conv with `ngroups` 16-row groups (incl. the ones group).
C2M_API int c2m_conv_wgrad_rows(int M, int ngroups) {
    int BM, BN;
    wgrad_tile(M, BM, BN);
    return c2m_cdiv(ngroups * 16, BN) * BN;
}

C2M_API int c2m_conv_wgrad(const void* dY, const void* X, float* slab, float* dW, float* db, const int* jtab,
                           const int64_t* g, void* stream) {
    C2M_ENTER();
    WgradP p;
    p.dY = (const float*)dY; p.X = (const float*)X; p.slab = slab; p.jtab = reinterpret_cast<const int4*>(jtab);
    p.M = (int)g[C2M_G_M]; p.J = (int)g[C2M_G_NK];
    p.Npix = (int)g[C2M_G_NPIX]; p.To = (int)g[C2M_G_TO]; p.Ho = (int)g[C2M_G_HO]; p.Wo = (int)g[C2M_G_WO];
    p.Ti = (int)g[C2M_G_TI]; p.Hi = (int)g[C2M_G_HI]; p.Wi = (int)g[C2M_G_WI];
    p.st = (int)g[C2M_G_ST]; p.sh = (int)g[C2M_G_SH]; p.sw = (int)g[C2M_G_SW];
    p.in_sn = g[C2M_G_IN_SN]; p.in_st = g[C2M_G_IN_ST]; p.in_sh = g[C2M_G_IN_SH];
    p.dy_sn = g[C2M_G_OUT_SN]; p.dy_sc = g[C2M_G_OUT_SC];
    p.reflect = (int)g[C2M_G_REFLECT]; p.is3d = (int)g[C2M_G_IS3D];
    p.in_sc = (int)g[C2M_G_IN_SC];
    const int NS = (int)g[C2M_G_NS], Cin = (int)g[C2M_G_CIN], taps = (int)g[C2M_G_TAPS], ntg = (int)g[C2M_G_NTG], ngroups = (int)g[C2M_G_NGROUPS];
    if (g[C2M_G_X_BYTES] <= 0 || g[C2M_G_X_BYTES] >= 0x80000000LL || g[C2M_G_DY_BYTES] <= 0 || g[C2M_G_DY_BYTES] >= 0x80000000LL) return (int)hipErrorInvalidValue;
    p.x_bytes = (unsigned)g[C2M_G_X_BYTES]; p.dy_bytes = (unsigned)g[C2M_G_DY_BYTES];
    if (p.M <= 0 || p.J <= 0 || p.Npix <= 0) return 0;
    int BM, BN;
    wgrad_tile(p.M, BM, BN);
    if (p.J % BN != 0 || p.J < (ngroups + 1) * 16 || (NS != 1 && NS != 2 && NS != 4)) return (int)hipErrorInvalidValue;
    const int S = c2m_conv_wgrad_splits(p.M, p.J, p.Npix);
    int per = c2m_cdiv(p.Npix, S);
    per = ((per + 63) / 64) * 64;
    p.pix_per_split = per;
    const int Seff = c2m_cdiv(p.Npix, per);   // <= S; unused slabs are never read
    hipStream_t s = (hipStream_t)stream;
    const bool xh = g[C2M_G_X_TYPE] == 1;                           // dY and X are bf16 tensors (bf16 kernels only)
    int Sred = Seff;                                      // splits the launch writes = slabs the reduction sums
    if (p.M <= 4 && p.Npix >= 16384) {                    // thin output: vector-ALU kernels (conv_thin.hip), same slab layout
        if (xh) return (int)hipErrorInvalidValue;         // fp32 operands (the host casts bf16 activations)
        // g[C2M_G_SQUARE_KW] = KW: 2-D stride-1 square KW x KW tap set in row-major order -> row-blocked kernel
        const int kw = (int)g[C2M_G_SQUARE_KW];
        if (p.M <= 3 && (kw == 3 || kw == 7) && !p.is3d && p.To == 1 && p.st == 1 && p.sh == 1 && p.sw == 1 && p.Wo % 4 == 0 &&
            taps == kw * kw && Cin > 0 && (p.dy_sn % 4) == 0 && (p.dy_sc % 4) == 0 && ((uintptr_t)dY & 15) == 0)
            Sred = c2m_launch_thin_wgrad_rows(p, kw, NS, ntg, Cin, ngroups, S, s);
        else
            Sred = c2m_launch_thin_wgrad(p, NS, ngroups, S, s);
    } else {
        const bool bf16 = g[C2M_G_PRECISION] == 1;
        if (bf16 != xh) return (int)hipErrorInvalidValue;  // the bf16 kernel gathers bf16 tensors, the fp32 kernel fp32 ones
        const dim3 grid(p.J / BN, c2m_cdiv(p.M, BM), Seff);
        const dim3 grid1(grid.x * grid.y * grid.z);       // 1-D launch, decoded XCD-aware in the kernel (common.h)
        // g[C2M_G_WGRAD_WIDE] = 1: the layer qualifies for the 16-byte-load form (host: unit x stride, Wi == Wo, Wo % 8 == 0, |tap dx| <= 1)
        if (bf16 && g[C2M_G_WGRAD_WIDE] == 2) {      // the stride-2 form (host: sw == 2, Wi == 2 Wo, Wo % 8 == 0, dx in -1 .. 2)
            if (p.sw != 2 || p.Wi != 2 * p.Wo || (p.Wo & 7) || (p.dy_sc & 7) || (p.pix_per_split & 63)) return (int)hipErrorInvalidValue;
            if (p.M <= 32)      hipLaunchKernelGGL((conv_wgrad_wide_bf16_kernel<32, 128, 1, 4, 2>), grid1, dim3(256), 0, s, p, NS);
            else if (p.M > 64)  hipLaunchKernelGGL((conv_wgrad_wide_bf16_kernel<128, 128, 2, 2, 2>), grid1, dim3(256), 0, s, p, NS);
            else                hipLaunchKernelGGL((conv_wgrad_wide_bf16_kernel<64, WG64_BN, 2, 2, 2>), grid1, dim3(256), 0, s, p, NS);
        } else if (bf16 && g[C2M_G_WGRAD_WIDE] == 1) {
            if (p.sw != 1 || p.Wi != p.Wo || (p.Wo & 7) || p.Wi < 8 || (p.dy_sc & 7) || (p.pix_per_split & 63)) return (int)hipErrorInvalidValue;
            if (p.M <= 32)      hipLaunchKernelGGL((conv_wgrad_wide_bf16_kernel<32, 128, 1, 4>), grid1, dim3(256), 0, s, p, NS);
            else if (p.M > 64)  hipLaunchKernelGGL((conv_wgrad_wide_bf16_kernel<128, 128, 2, 2>), grid1, dim3(256), 0, s, p, NS);
            else                hipLaunchKernelGGL((conv_wgrad_wide_bf16_kernel<64, WG64_BN, 2, 2>), grid1, dim3(256), 0, s, p, NS);
        } else {
#define C2M_WG(BMv, BNv, WGMv, WGNv)                                                                                  \
    do {                                                                                                              \
        if (bf16) {                                                                                                   \
            if (NS == 1)      hipLaunchKernelGGL((conv_wgrad_kernel<BMv, BNv, WGMv, WGNv, 1, true>), grid1, dim3(256), 0, s, p); \
            else if (NS == 2) hipLaunchKernelGGL((conv_wgrad_kernel<BMv, BNv, WGMv, WGNv, 2, true>), grid1, dim3(256), 0, s, p); \
            else              hipLaunchKernelGGL((conv_wgrad_kernel<BMv, BNv, WGMv, WGNv, 4, true>), grid1, dim3(256), 0, s, p); \
        } else {                                                                                                      \
            if (NS == 1)      hipLaunchKernelGGL((conv_wgrad_kernel<BMv, BNv, WGMv, WGNv, 1>), grid1, dim3(256), 0, s, p); \
            else if (NS == 2) hipLaunchKernelGGL((conv_wgrad_kernel<BMv, BNv, WGMv, WGNv, 2>), grid1, dim3(256), 0, s, p); \
            else              hipLaunchKernelGGL((conv_wgrad_kernel<BMv, BNv, WGMv, WGNv, 4>), grid1, dim3(256), 0, s, p); \
        }                                                                                                             \
    } while (0)
            if (p.M <= 32)      C2M_WG(32, 128, 1, 4);
            else if (p.M > 64)  C2M_WG(128, 128, 2, 2);
            else                C2M_WG(64, WG64_BN, 2, 2);
#undef C2M_WG
        }
    }
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    const long total = (long)p.M * (ngroups + 1) * 16;
    return launch_wgrad_reduce(total, s, slab, dW, db, p.M, p.J, Cin, taps, NS, ntg, ngroups, Sred);
}
