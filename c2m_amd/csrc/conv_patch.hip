// LDS-patch kernels for the 3x3 stride-1 convolutions, fp32 (v_mfma_f32_32x32x2_f32) and bf16 (v_mfma_f32_32x32x16_bf16);
// reached through c2m_conv_igemm (conv_igemm.hip) with geom[C2M_G_PATCH] set.  Same packed weights, output strides, split-K slabs and
// two-target reflect epilogue as conv_igemm_kernel.
#include "conv_common.h"

// ------------------------------------------------------------------------------------------------ LDS patch
// 3x3 stride-1 convolutions (forward and data gradient; >80 % of the step's conv FLOPs: VGG, SPADE MLPs, generator,
// decoder): the input patch of a 16-channel chunk ((rows+2) x 34 pixels per channel) is staged in LDS ONCE and serves
// all 9 taps -- the B fragments of every tap are read straight from the patch with a tap offset.  Compared with the
// gather kernel there is no per-tap global gather and no per-tap LDS write of B at all; per 16-deep K-step only the
// weight tile is loaded/stored.  Zero or reflect boundary is resolved while loading the patch.
// Output tile = (BN/32) rows x 32 columns of one image, so each MFMA column block is one contiguous row segment.
template <int BM, int BN, int WGM, int WGN>
__global__ __launch_bounds__(256) void conv_patch3x3_kernel(const ConvP p) {
    constexpr int BK = 16, TR = BN / 32, PH = TR + 2, PW = 34, PCH = PH * PW, PELEMS = BK * PCH;
    constexpr int PLOADS = (PELEMS + 255) / 256;
    constexpr int TM = BM / WGM, TN = BN / WGN, MI = TM / 32, NI = TN / 32;
    constexpr int LDA_S = BM + 4;
    constexpr int A_F4 = BM * BK / 4, APASS = (A_F4 + 255) / 256;
    static_assert(WGM * WGN == 4, "tile");
    __shared__ float sA[2][BK][LDA_S];
    __shared__ float sP[2][PLOADS * 256];      // filled by LDS-DMA: 64 consecutive floats per wave-instruction

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    // tile -> (image, tile row, tile col); XCD-aware order (common.h): row tiles of a pixel tile fastest
    const int tiles_x = (p.Wo + 31) / 32, tiles_y = (p.Ho + TR - 1) / TR;
    const C2mBlock blk = c2m_xcd_block((unsigned)((p.Npix / (p.Ho * p.Wo)) * tiles_y * tiles_x), (unsigned)(p.M + BM - 1) / BM, 1);
    const int m0 = blk.y * BM;
    int tb = blk.x;
    const int tx = tb % tiles_x; tb /= tiles_x;
    const int ty = tb % tiles_y; const int img = tb / tiles_y;        // img = n*To + ot (2-D planes)
    const int oy0 = ty * TR, ox0 = tx * 32;
    const int n_img = img / p.To, t_img = img % p.To;

    // ---- patch loads.  The patch of a chunk is 16 channels x PCH positions, [c][row][col] dense in LDS.  A DMA row is 64
    // consecutive positions of ONE channel: wave w fetches the PROWS rows of channels w, w+4, w+8, w+12, the channel rides in
    // the scalar offset, so a lane owns the PROWS positions wr*64 + lane and the reflect / bounds arithmetic is done PROWS
    // (6 at the 8-row tile) times per thread instead of once per fetched element (22 times: ~550 VALU in the prologue, a third
    // of all VALU of a 288-deep layer; a VALU beside MFMAs costs matrix-pipe cycles, tools/micro/mfma_issue.hip).  The last
    // row of a channel is partial: its lanes beyond PCH are switched off (EXEC), not sent out of range -- an out-of-range
    // lane would write a zero into the next channel's first positions.
    constexpr int PROWS = (PCH + 63) / 64;
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const unsigned long xaddr = (unsigned long)p.X;
    const u32x4 xrs = {(unsigned)xaddr, (unsigned)(xaddr >> 32) & 0xffffu, p.x_bytes, 0x00020000u};
    const unsigned sp_lds = (unsigned)(unsigned long)(__attribute__((address_space(3))) float*)&sP[0][0];
    const unsigned img_byte = (unsigned)(n_img * (int)p.in_sn + t_img * (int)p.in_st) * 4u;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    unsigned pvo[PROWS];
#pragma unroll
    for (int wr = 0; wr < PROWS; ++wr) {
        const int pos = wr * 64 + lane;
        const int r = pos / PW, col = pos % PW;
        int iy = oy0 + p.iy0 + r, ix = ox0 + p.ix0 + col;
        if (p.reflect) {
            iy = iy < 0 ? -iy : iy; iy = iy >= p.Hi ? 2 * p.Hi - 2 - iy : iy;
            ix = ix < 0 ? -ix : ix; ix = ix >= p.Wi ? 2 * p.Wi - 2 - ix : ix;
        }
        const bool ok = pos < PCH && (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;   // (tiles may hang off)
        pvo[wr] = ok ? img_byte + (unsigned)(iy * (int)p.in_sh + ix) * 4u : C2M_OOB;
    }
    auto load_patch = [&](int chunk, int buf) {
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
            const int c = wave_s + 4 * ci, ch = chunk * BK + c;
            u32x4 rsk = xrs;
            rsk[2] = ch < p.cin ? p.x_bytes : 0u;       // channels past K: zero records (the scalar offset is not range-checked)
            const int soff = ch * p.in_sc * 4;
#pragma unroll
            for (int wr = 0; wr < PROWS; ++wr) {
                const unsigned dst = sp_lds + (unsigned)((buf * PLOADS * 256 + c * PCH + wr * 64) * 4);
                if (wr * 64 + 64 <= PCH || wr * 64 + lane < PCH)
                    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, %3 offen lds"
                                 :: "s"(dst), "v"(pvo[wr]), "s"(rsk), "s"(soff) : "memory");
            }
        }
    };

    // ---- weight side (same packed K order as the gather kernel with CK = 16: (chunk, tap, channel))
    const int akq = (tid & 3) * 4, arow = tid >> 2;
    const float* __restrict__ aptr[APASS];
#pragma unroll
    for (int s = 0; s < APASS; ++s) {
        int row = m0 + arow + s * 64; row = row < p.M ? row : p.M - 1;
        aptr[s] = p.A + (long)row * p.lda + akq;
    }
    float4 ra[APASS];
    auto load_a = [&](int kt) {
#pragma unroll
        for (int s = 0; s < APASS; ++s)
            if (A_F4 >= 256 || arow + s * 64 < BM) ra[s] = *reinterpret_cast<const float4*>(aptr[s] + kt * BK);
    };
    auto store_a = [&](int buf) {
#pragma unroll
        for (int s = 0; s < APASS; ++s) {
            const int r = arow + s * 64;
            if (A_F4 >= 256 || r < BM) {
                sA[buf][akq + 0][r] = ra[s].x; sA[buf][akq + 1][r] = ra[s].y;
                sA[buf][akq + 2][r] = ra[s].z; sA[buf][akq + 3][r] = ra[s].w;
            }
        }
    };

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // B fragment base inside the patch: channel (lane>>5), tile row (wn*NI + j), column (lane&31)
    int pbase[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) pbase[j] = (lane >> 5) * PCH + (wn * NI + j) * PW + (lane & 31);

    // split-K over whole channel chunks (gridDim.z); ksteps_per_split holds CHUNKS per split for this kernel
    const int chunk_beg = blk.z * p.ksteps_per_split;
    int chunk_end = chunk_beg + p.ksteps_per_split; chunk_end = chunk_end < p.nchunks ? chunk_end : p.nchunks;
    load_patch(chunk_beg, 0);
    load_a(chunk_beg * 9);
    store_a(0);
    // The patch DMA is inline asm the compiler's s_waitcnt insertion does not see.  It used to be covered only implicitly, by the
    // wait for the A-tile load issued after it (loads return in order) -- but with BM = 32 the threads >= 128 load no A element,
    // so waves 2 and 3 reached the barrier WITHOUT ever waiting for the channels they had fetched, and their part of the patch
    // could still be in flight when the other waves read it.  Alone on the chip the DMA always won the race; next to ANY other
    // kernel that keeps the memory system busy it did not (round 4, tools/concurrency_stress.py: wrong forward values and
    // gradients next to torch.add on another stream).  Every barrier that publishes a freshly fetched patch buffer now has an
    // explicit wait in front of it (free: the waves that load A were waiting there already).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cur = 0, pcur = 0;
    for (int chunk = chunk_beg; chunk < chunk_end; ++chunk) {
        const bool more_chunks = chunk + 1 < chunk_end;
        if (more_chunks) load_patch(chunk + 1, pcur ^ 1);  // the other buffer was last read before the previous barrier
#ifdef C2M_PATCH_ROLLED
#pragma unroll 1
#else
#pragma unroll
#endif
        for (int tap = 0; tap < 9; ++tap) {
            const int kt = chunk * 9 + tap;
            const bool more = tap < 8 || more_chunks;
            if (more) load_a(kt + 1);
            const int toff = p.pty[tap / 3] * PW + p.ptx[tap % 3];
            float a[BK / 2][MI], b[BK / 2][NI];
#pragma unroll
            for (int kk = 0; kk < BK / 2; ++kk) {
                const int krow = kk * 2 + (lane >> 5);
#pragma unroll
                for (int i = 0; i < MI; ++i) a[kk][i] = sA[cur][krow][wm * TM + i * 32 + (lane & 31)];
#pragma unroll
                for (int j = 0; j < NI; ++j) b[kk][j] = sP[pcur][pbase[j] + kk * 2 * PCH + toff];
            }
#pragma unroll
            for (int kk = 0; kk < BK / 2; ++kk)
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk][i], b[kk][j], acc[i][j], 0, 0, 0);
            {   // fragment reads two k-pairs ahead of their MFMAs (only the first reads of a tap are waited for)
                constexpr int NMF = (BK / 2) * MI * NI, RPM = (MI + NI + MI * NI - 1) / (MI * NI);
                __builtin_amdgcn_sched_group_barrier(0x100, 2 * (MI + NI), 0);
#pragma unroll
                for (int g = 0; g < NMF; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, RPM, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (more) store_a(cur ^ 1);
            if (tap == 8 && more_chunks) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // next chunk's patch DMA (see the prologue)
            __syncthreads();
            cur ^= 1;
        }
        pcur ^= 1;
    }

    // ---- epilogue
    const bool direct = blk.nz == 1;
    constexpr bool yh = false;                             // the fp32 kernels write fp32
    constexpr int yes = 4;
    float* __restrict__ Yb = p.Y + (long)blk.z * p.slab_stride;
    {
        const int row0 = __builtin_amdgcn_readfirstlane(m0 + wm * TM);
        if (row0 + MI * 32 <= p.M) {
            unsigned voff[NI], voff2[NI];
            bool ring = false;
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const int oy = oy0 + wn * NI + j, ox = ox0 + (lane & 31);
                const bool in = oy < p.Ho && ox < p.Wo;
                const long e = p.out_off + (long)n_img * p.out_sn + (long)t_img * p.out_st + (long)oy * p.out_sh +
                               (long)ox * p.out_sw + 4L * (lane >> 5) * p.out_sc;
                voff[j] = in ? (unsigned)(e * 4) : 0x80000000u;
                voff2[j] = 0x80000000u;
                if (p.Y2) {
                    const int tp = t_img * p.ps_t + p.po_t - p.lo_t, yp = oy * p.ps_y + p.po_y - p.lo_y,
                              xp = ox * p.ps_x + p.po_x - p.lo_x;
                    if (in && (unsigned)tp < (unsigned)p.ext_t && (unsigned)yp < (unsigned)p.ext_y &&
                        (unsigned)xp < (unsigned)p.ext_x) {
                        const long e2 = (long)n_img * p.y2_sn + (long)tp * p.y2_st + (long)yp * p.y2_sh + xp +
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
        const int oy = oy0 + wn * NI + j, ox = ox0 + (lane & 31);
        if (oy >= p.Ho || ox >= p.Wo) continue;
        float* __restrict__ yb = Yb + p.out_off + (long)n_img * p.out_sn + (long)t_img * p.out_st + (long)oy * p.out_sh +
                                 (long)ox * p.out_sw;
        long row_stride = p.out_sc;
        if (p.Y2) {
            const int tp = t_img * p.ps_t + p.po_t - p.lo_t, yp = oy * p.ps_y + p.po_y - p.lo_y,
                      xp = ox * p.ps_x + p.po_x - p.lo_x;
            if ((unsigned)tp < (unsigned)p.ext_t && (unsigned)yp < (unsigned)p.ext_y && (unsigned)xp < (unsigned)p.ext_x) {
                yb = p.Y2 + (long)n_img * p.y2_sn + (long)tp * p.y2_st + (long)yp * p.y2_sh + xp;
                row_stride = p.y2_sc;
            }
        }
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row < p.M) {
                    float v = acc[i][j][r];
                    if (direct) {
                        if (p.bias) v += p.bias[row];
                        v = c2m_act(v, p.act, p.slope);
                    }
                    yb[(long)row * row_stride] = v;
                }
            }
    }
}

template <int BM, int BN, int WGM, int WGN>
static int launch_patch(const ConvP& p, int splits, hipStream_t s) {
    constexpr int TR = BN / 32;
    const long tiles = (long)(p.Npix / (p.Ho * p.Wo)) * ((p.Ho + TR - 1) / TR) * ((p.Wo + 31) / 32);
    dim3 grid((unsigned)(tiles * c2m_cdiv(p.M, BM) * splits));
    hipLaunchKernelGGL((conv_patch3x3_kernel<BM, BN, WGM, WGN>), grid, dim3(256), 0, s, p);
    return (int)hipGetLastError();
}

int c2m_launch_patch(const ConvP& p, int splits, hipStream_t s) {
    if (p.M <= 32)      return launch_patch<32, 256, 1, 4>(p, splits, s);
    else if (p.M <= 64) return launch_patch<64, 128, 2, 2>(p, splits, s);
    else                return launch_patch<128, 128, 2, 2>(p, splits, s);
}

// ------------------------------------------------------------------------------------------------ LDS patch, bf16
// The bf16 form of the kernel above (BASELINE configs[2-4]): v_mfma_f32_32x32x16_bf16 is 16x the fp32 MFMA rate, so the
// kernel lives or dies by operand delivery.  Per 16-channel chunk
//   * the (8+2) x 34 input patch is gathered ONCE from the bf16 NCHW activations (24 coalesced 2-byte loads per thread: on
//     NCHW the 8 channels a lane needs sit 2*H*W bytes apart; a 16-byte-load + 4x8 register-transpose form of this fetch was
//     measured 5-25 % SLOWER, profiles/r03_ab_bf16_patch_wide_vs_narrow.txt), packed in registers and stored as
//     [pixel][16 channels] (32 B per pixel): the B fragment of ANY of the 9 taps is then one conflict-free ds_read_b128 at a
//     pixel offset -- no per-tap gather, no conversion;
//   * the weights arrive pre-packed in bf16 as [chunk][tap][row][16 channels] (c2m_pack_weights_bf16_patch): one 16-byte
//     load + one ds_write_b128 per 512 MACs of MFMA work, and the A fragment is one ds_read_b128;
//   * one barrier per chunk (72 MFMAs per wave at BM = 128), next chunk's global loads in flight during the MFMAs.
// Tile: BM output channels x (8 rows x 32 columns); wave w owns rows 2w, 2w+1 for all BM channels (MI = BM/32, NI = 2).
template <int BM>
__global__ __launch_bounds__(256) void conv_patch3x3_bf16_kernel(const ConvP p) {
    constexpr int TR = 8, PH = TR + 2, PW = 34, NPIX = PH * PW;           // 340 patch pixels
    constexpr int MI = BM / 32, NI = 2;
    constexpr int A_UNITS = 9 * BM * 2;                                    // 16-byte units per chunk: [tap][half][row]
    constexpr int APT = (A_UNITS + 255) / 256;
    // LDS: double-buffered weight image + patch (73.7 + 21.8 KB at BM = 128: one workgroup per CU, one barrier per chunk;
    // a single-buffered weight image with two workgroups per CU and two barriers per chunk measured 20 % slower).
    // Both images keep the two 8-channel halves in separate planes ([half][pixel], [tap][half][row]): the 32 lanes of a
    // ds_read_b128 half-wave then read 512 contiguous bytes (interleaved halves were a 2-way bank conflict on every read).
    __shared__ uint4 sA[2][A_UNITS];
    __shared__ uint4 sP[2][NPIX * 2];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_x = (p.Wo + 31) / 32, tiles_y = (p.Ho + TR - 1) / TR;
    const C2mBlock blk = c2m_xcd_block((unsigned)((p.Npix / (p.Ho * p.Wo)) * tiles_y * tiles_x), (unsigned)(p.M + BM - 1) / BM, 1);
    const int m0 = blk.y * BM;
    int tb = blk.x;
    const int tx = tb % tiles_x; tb /= tiles_x;
    const int ty = tb % tiles_y; const int img = tb / tiles_y;            // img = n*To + ot (2-D planes)
    const int oy0 = ty * TR, ox0 = tx * 32;
    const int n_img = img / p.To, t_img = img % p.To;

    // ---- patch gather: three rounds of (pixel, 8-channel half); the half is wave-uniform in every round
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.X), 0, p.x_bytes, 0x00020000);
    const unsigned img_byte = (unsigned)(n_img * (int)p.in_sn + t_img * (int)p.in_st) * 2u;     // X is bf16 (2-byte elements)
    const int ppix[3] = {tid, tid, 256 + (tid & 127)};
    const int phalf[3] = {0, 1, wave >> 1};
    unsigned pvo[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int e = ppix[r];
        const int row = e / PW, col = e % PW;
        int iy = oy0 + p.iy0 + row, ix = ox0 + p.ix0 + col;
        bool ok = e < NPIX;
        if (p.reflect) {
            iy = iy < 0 ? -iy : iy; iy = iy >= p.Hi ? 2 * p.Hi - 2 - iy : iy;
            ix = ix < 0 ? -ix : ix; ix = ix >= p.Wi ? 2 * p.Wi - 2 - ix : ix;
        }
        ok = ok && (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
        pvo[r] = ok ? img_byte + (unsigned)(iy * (int)p.in_sh + ix) * 2u : C2M_OOB;
    }
    struct Stage { unsigned short pv[3][8]; };
    auto fetch_patch = [&](int chunk, unsigned short (&pv)[3][8]) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                // channels past Cin (the last chunk of a Cin % 16 != 0 layer): the scalar offset is NOT range-checked by the
                // hardware, so they get a zero-record descriptor (wave-uniform select, SALU only) and read 0 -- never the
                // memory behind X (a NaN there times the zero-padded weight would poison the pixel)
                const int ch = chunk * 16 + phalf[r] * 8 + j;
                const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                    const_cast<float*>(p.X), 0, ch < p.cin ? p.x_bytes : 0, 0x00020000);
                const int soff = ch * p.in_sc * 2;
                pv[r][j] = __builtin_amdgcn_raw_buffer_load_b16(rs, pvo[r], soff, 0);
            }
    };
    auto stash_patch = [&](int buf, const unsigned short (&pv)[3][8]) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            bf16x8 q;
#pragma unroll
            for (int j = 0; j < 8; ++j) q[j] = __builtin_bit_cast(__bf16, pv[r][j]);
            if (r < 2 || ppix[r] < NPIX) sP[buf][phalf[r] * NPIX + ppix[r]] = __builtin_bit_cast(uint4, q);
        }
    };
    // ---- weights: global [chunk][tap][Mpad rows][2 halves] 16-byte units -> LDS [tap][half][row]
    const uint4* __restrict__ Ab = reinterpret_cast<const uint4*>(p.A);
    const long mpad2 = (long)p.lda * 2;                                    // lda = padded row count of the packed matrix
    long aoff[APT];
    int adst[APT];
#pragma unroll
    for (int i = 0; i < APT; ++i) {
        const int u = tid + i * 256;
        const int tap = u / (BM * 2), rem = u % (BM * 2);
        aoff[i] = (long)tap * mpad2 + (long)m0 * 2 + rem;
        adst[i] = (tap * 2 + (rem & 1)) * BM + (rem >> 1);
    }
    auto fetch_a = [&](int chunk, uint4 (&av)[APT]) {
#pragma unroll
        for (int i = 0; i < APT; ++i)
            if (A_UNITS % 256 == 0 || tid + i * 256 < A_UNITS) av[i] = Ab[(long)chunk * 9 * mpad2 + aoff[i]];
    };
    auto stash_a = [&](int buf, const uint4 (&av)[APT]) {
#pragma unroll
        for (int i = 0; i < APT; ++i)
            if (A_UNITS % 256 == 0 || tid + i * 256 < A_UNITS) sA[buf][adst[i]] = av[i];
    };

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    int pbase[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) pbase[j] = (lane >> 5) * NPIX + (wave * NI + j) * PW + (lane & 31);
    const int abase = (lane >> 5) * BM + (lane & 31);

    const int chunk_beg = blk.z * p.ksteps_per_split;
    int chunk_end = chunk_beg + p.ksteps_per_split; chunk_end = chunk_end < p.nchunks ? chunk_end : p.nchunks;
    // The activation gather (HBM / Infinity Cache) runs TWO chunks ahead of its LDS store (two register sets): one chunk of
    // MFMAs (~1.1 us) does not cover its loaded latency (~2.2 us per chunk with every CU fetching at once).  The weight
    // image comes from L2 and runs one chunk ahead (a second set of 36 registers would not fit the 256 VGPRs).
    Stage s0, s1;
    uint4 av[APT];
    const int nck = chunk_end - chunk_beg;
    fetch_a(chunk_beg, av);
    fetch_patch(chunk_beg, s0.pv);
    stash_a(0, av);
    stash_patch(0, s0.pv);
    __syncthreads();
    // vmcnt retires in order: the weight loads of chunk c+1 are issued BEFORE the patch loads of chunk c+2 / c+3, so
    // waiting for them at the end of chunk c leaves the deep patch loads in flight
    if (nck > 1) fetch_patch(chunk_beg + 1, s0.pv);
    if (nck > 1) fetch_a(chunk_beg + 1, av);
    if (nck > 2) fetch_patch(chunk_beg + 2, s1.pv);
    // fragments are read one tap ahead of the MFMAs that use them (two register sets): with one wave per SIMD nothing else
    // hides the LDS latency -- reading them right before use left the matrix pipe idle for most of every tap
    struct Frag { bf16x8 a[MI], b[NI]; };
    auto read_frag = [&](int buf, int tap, Frag& f) {
        const int toff = p.pty[tap / 3] * PW + p.ptx[tap % 3];
#pragma unroll
        for (int i = 0; i < MI; ++i) f.a[i] = __builtin_bit_cast(bf16x8, sA[buf][tap * 2 * BM + i * 32 + abase]);
#pragma unroll
        for (int j = 0; j < NI; ++j) f.b[j] = __builtin_bit_cast(bf16x8, sP[buf][pbase[j] + toff]);
    };
    auto mma = [&](const Frag& f) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[i], f.b[j], acc[i][j], 0, 0, 0);
    };
    constexpr int NPAIR = MI * NI < MI + NI ? MI * NI : MI + NI;
    int cur = 0;
    Frag f0, f1;
    read_frag(0, 0, f0);
#define PB_TAP(T, FC, FN)                                                          \
        read_frag(cur, (T) + 1, FN);                                               \
        mma(FC);                                                                   \
        _Pragma("unroll") for (int g_ = 0; g_ < NPAIR; ++g_) {                     \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                     \
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                     \
        }                                                                          \
        if (MI * NI > NPAIR) __builtin_amdgcn_sched_group_barrier(0x008, MI * NI - NPAIR, 0);   \
        if (MI + NI > NPAIR) __builtin_amdgcn_sched_group_barrier(0x100, MI + NI - NPAIR, 0);   \
        __builtin_amdgcn_sched_barrier(0);
    // one chunk: 9 taps from buffer cur; then the staged next chunk (set SC) goes to buffer cur ^ 1 and SC is refilled
    // with the chunk after next + 1
#define PB_CHUNK(SC)                                                               \
    do {                                                                           \
        PB_TAP(0, f0, f1) PB_TAP(1, f1, f0) PB_TAP(2, f0, f1) PB_TAP(3, f1, f0)    \
        PB_TAP(4, f0, f1) PB_TAP(5, f1, f0) PB_TAP(6, f0, f1) PB_TAP(7, f1, f0)    \
        mma(f0);                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                         \
        if (chunk + 1 < chunk_end) { stash_a(cur ^ 1, av); stash_patch(cur ^ 1, SC.pv); }   \
        __syncthreads();                                                           \
        if (chunk + 2 < chunk_end) fetch_a(chunk + 2, av);                         \
        if (chunk + 3 < chunk_end) fetch_patch(chunk + 3, SC.pv);                  \
        cur ^= 1;                                                                  \
        read_frag(cur, 0, f0);                                                     \
        ++chunk;                                                                   \
    } while (0)
    int chunk = chunk_beg;
    while (chunk < chunk_end) {
        PB_CHUNK(s0);
        if (chunk < chunk_end) PB_CHUNK(s1);
    }
#undef PB_CHUNK
#undef PB_TAP

    // ---- epilogue (same mapping as the fp32 patch kernel)
    const bool direct = blk.nz == 1;
    const bool yh = p.yh && direct;                        // bf16 output elements (split-K slabs are fp32)
    float* __restrict__ Yb = p.Y + (long)blk.z * p.slab_stride;
    // Vector path: a dword store per accumulator register (128 per wave) is store-ISSUE bound (~5 B/clk/CU: 27k cycles for
    // the 128 KB tile against 37k cycles of MFMAs at Cin = 256).  The tile goes through LDS instead (the weight buffers are
    // free now): [channel][64 pixels] per wave, 64 channels at a time, read back as float4 along the pixels and stored with
    // 16-byte stores (32 per wave instead of 128), still full 128-byte row segments per channel.
    if (yh && !p.Y2 && p.out_sw == 1 && (p.Wo & 7) == 0 && (p.out_off & 7) == 0 && (p.out_sc & 7) == 0 && (p.out_sn & 7) == 0 &&
        (p.out_st & 7) == 0 && (p.out_sh & 7) == 0 && ((uintptr_t)p.Y & 15) == 0 && BM >= 64) {
        // bf16 output: the same staging through LDS, read back as 8 pixels per lane -> one 16-byte store of 8 bf16
        float* __restrict__ T = reinterpret_cast<float*>(&sA[0][0]) + wave * (64 * 64);
        bf16_t* __restrict__ yimg = reinterpret_cast<bf16_t*>(p.Y) + p.out_off + (long)n_img * p.out_sn + (long)t_img * p.out_st;
#pragma unroll
        for (int h = 0; h < MI / 2; ++h) {
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int jj = 0; jj < NI; ++jj)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int cl = q * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                        float v = acc[2 * h + q][jj][r];
                        const int row = m0 + h * 64 + cl;
                        if (p.bias && row < p.M) v += p.bias[row];
                        T[cl * 64 + jj * 32 + (lane & 31)] = c2m_act(v, p.act, p.slope);
                    }
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int cl = it * 8 + (lane >> 3), px = (lane & 7) * 8;
                const float4 v0 = *reinterpret_cast<const float4*>(&T[cl * 64 + px]);
                const float4 v1 = *reinterpret_cast<const float4*>(&T[cl * 64 + px + 4]);
                const int row = m0 + h * 64 + cl;
                const int oy = oy0 + wave * NI + (px >> 5), ox = ox0 + (px & 31);
                if (row < p.M && oy < p.Ho && ox < p.Wo) {
                    const bf16x8 o = {(bf16_t)v0.x, (bf16_t)v0.y, (bf16_t)v0.z, (bf16_t)v0.w,
                                      (bf16_t)v1.x, (bf16_t)v1.y, (bf16_t)v1.z, (bf16_t)v1.w};
                    __builtin_nontemporal_store(o, reinterpret_cast<bf16x8*>(yimg + (long)row * p.out_sc + (long)oy * p.out_sh + ox));
                }
            }
        }
        return;
    }
    if (!yh && !p.Y2 && p.out_sw == 1 && (p.Wo & 3) == 0 && (p.out_off & 3) == 0 && (p.out_sc & 3) == 0 && (p.out_sn & 3) == 0 &&
        (p.slab_stride & 3) == 0 && ((uintptr_t)p.Y & 15) == 0 && BM >= 64) {
        float* __restrict__ T = reinterpret_cast<float*>(&sA[0][0]) + wave * (64 * 64);     // 16 KB per wave
        float* __restrict__ yimg = Yb + p.out_off + (long)n_img * p.out_sn + (long)t_img * p.out_st;
#pragma unroll
        for (int h = 0; h < MI / 2; ++h) {
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int jj = 0; jj < NI; ++jj)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int cl = q * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                        float v = acc[2 * h + q][jj][r];
                        if (direct) {
                            const int row = m0 + h * 64 + cl;
                            if (p.bias && row < p.M) v += p.bias[row];
                            v = c2m_act(v, p.act, p.slope);
                        }
                        T[cl * 64 + jj * 32 + (lane & 31)] = v;
                    }
#pragma unroll
            for (int it = 0; it < 16; ++it) {
                const int cl = it * 4 + (lane >> 4), px = (lane & 15) * 4;
                const float4 v = *reinterpret_cast<const float4*>(&T[cl * 64 + px]);
                const int row = m0 + h * 64 + cl;
                const int oy = oy0 + wave * NI + (px >> 5), ox = ox0 + (px & 31);
                if (row < p.M && oy < p.Ho && ox < p.Wo) {
                    // non-temporal: the 100+ MB output would otherwise push the input patches out of L2 / Infinity Cache
                    // while they are still being gathered (+4...12 % on the configs[2] layers)
                    f32x4 vv = {v.x, v.y, v.z, v.w};
                    __builtin_nontemporal_store(vv, reinterpret_cast<f32x4*>(yimg + (long)row * p.out_sc + (long)oy * p.out_sh + ox));
                }
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int oy = oy0 + wave * NI + j, ox = ox0 + (lane & 31);
        if (oy >= p.Ho || ox >= p.Wo) continue;
        float* ybase = Yb;                                     // element type: float, or bf16_t when yh (then blk.z == 0)
        long yidx = p.out_off + (long)n_img * p.out_sn + (long)t_img * p.out_st + (long)oy * p.out_sh + (long)ox * p.out_sw;
        long row_stride = p.out_sc;
        if (p.Y2) {
            const int tp = t_img * p.ps_t + p.po_t - p.lo_t, yp = oy * p.ps_y + p.po_y - p.lo_y,
                      xp = ox * p.ps_x + p.po_x - p.lo_x;
            if ((unsigned)tp < (unsigned)p.ext_t && (unsigned)yp < (unsigned)p.ext_y && (unsigned)xp < (unsigned)p.ext_x) {
                ybase = p.Y2;
                yidx = (long)n_img * p.y2_sn + (long)tp * p.y2_st + (long)yp * p.y2_sh + xp;
                row_stride = p.y2_sc;
            }
        }
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
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

template <int BM>
static int launch_patch_bf16(const ConvP& p, int splits, hipStream_t s) {
    const long tiles = (long)(p.Npix / (p.Ho * p.Wo)) * ((p.Ho + 7) / 8) * ((p.Wo + 31) / 32);
    dim3 grid((unsigned)(tiles * c2m_cdiv(p.M, BM) * splits));
    hipLaunchKernelGGL((conv_patch3x3_bf16_kernel<BM>), grid, dim3(256), 0, s, p);
    return (int)hipGetLastError();
}

int c2m_launch_patch_bf16(const ConvP& p, int splits, hipStream_t s) {
    if (p.M <= 32)      return launch_patch_bf16<32>(p, splits, s);
    // 64-row tiles keep TWO workgroups on a CU (59 KB of LDS each; the 128-row tile's 95 KB leave one wave per SIMD
    // with nothing to hide its stalls): +5...14 % up to 256 input channels, -5 % at 512 (the weight image is
    // streamed twice as often) -- A/B on one box, bf16 tensors
    else if (p.M <= 64 || p.cin <= 256) return launch_patch_bf16<64>(p, splits, s);
    else                return launch_patch_bf16<128>(p, splits, s);
}
