// Vector-ALU kernels for convolutions with <= 4 output channels: forward and weight gradient, per pixel and row-blocked; reached
// through c2m_conv_igemm (conv_igemm.hip) and c2m_conv_wgrad (conv_wgrad.hip).
#include "conv_common.h"

// ------------------------------------------------------------------------------------------------ thin layers
// Convolutions with <= 4 output channels (flow / occlusion heads, the RGB output conv) waste >= 87 % of a 32-row MFMA
// tile; they run on the vector ALU instead: one pixel per lane, the same K-step table and buffer-load gather, weights
// through scalar loads (the k index is wave-uniform).  Forward only needs this; the data gradient of these layers has
// M = Cin >= 32 and stays on the MFMA path.
template <int MT, int NS>
__global__ __launch_bounds__(256) void conv_thin_fwd_kernel(const ConvP p) {
    constexpr int CK = 16 / NS;
    const int in_st = (int)p.in_st, in_sh = (int)p.in_sh;
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.X), 0, p.x_bytes, 0x00020000);
    for (int pix = blockIdx.x * 256 + threadIdx.x; pix < p.Npix; pix += gridDim.x * 256) {
        int n, ot, oy, ox;
        decompose_pix(pix, p, n, ot, oy, ox);
        const unsigned img_byte = (unsigned)(n * (int)p.in_sn) * 4u;
        const int ots = ot * p.st, oys = oy * p.sh, oxs = ox * p.sw;
        float acc[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m] = 0.f;
        for (int kt = 0; kt < p.nk; ++kt) {
            const int4* __restrict__ kd = p.ktab + (long)kt * (1 + NS);
            const int4 hdr = kd[0];
            unsigned vo[NS];
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                const int so = spatial_off(kd[1 + q], ots, oys, oxs, p.Ti, p.Hi, p.Wi, in_st, in_sh, p.reflect, p.is3d);
                vo[q] = so >= 0 ? img_byte + (unsigned)so * 4u : C2M_OOB;
            }
            float xv[16];
#pragma unroll
            for (int e = 0; e < 16; ++e)
                xv[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                    xrsrc, vo[e / CK], (hdr.x + (e % CK) * p.in_sc) * 4, 0));
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const float* __restrict__ wr = p.A + (long)m * p.lda + kt * 16;      // uniform -> scalar loads
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[m] = fmaf(xv[e], wr[e], acc[m]);
            }
        }
        float* __restrict__ yb = p.Y + p.out_off + (long)n * p.out_sn + (long)ot * p.out_st + (long)oy * p.out_sh +
                                 (long)ox * p.out_sw;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < p.M) {
                float v = acc[m];
                if (p.bias) v += p.bias[m];
                yb[(long)m * p.out_sc] = c2m_act(v, p.act, p.slope);
            }
        }
    }
}

// Row-blocked form for 2-D stride-1 square kernels (the 7x7 RGB head, the 3x3 flow / occlusion heads, the data gradient
// of the first VGG conv): each lane computes PX = 4 horizontally adjacent outputs, so one gathered input row segment of
// PX + KW - 1 values feeds PX * KW taps -- 2.8x (7x7) / 2x (3x3) fewer loads per FMA than the per-pixel kernel above,
// which is bound by load issue.  Tap geometry comes from the same K-step table (row-major taps, dx ascending for the
// forward pass, descending for a data gradient), weights from the same packed matrix through scalar loads.
template <int MT, int KW>
__global__ __launch_bounds__(256) void conv_thin_rows_kernel(const ConvP p, int lns, int ntg, int Cin, int xdesc) {
    constexpr int PX = 4, NV = PX + KW - 1;
    extern __shared__ float4 sW[];                        // [c][i][j] -> weights of the (<= 4) output rows
    const int NS = 1 << lns, CK = 16 >> lns, lck = 4 - lns;
    auto tap_entry = [&](int t) { return p.ktab[(t >> lns) * (1 + NS) + 1 + (t & (NS - 1))]; };   // chunk 0's taps
    for (int e = threadIdx.x; e < Cin * KW * KW; e += 256) {
        const int c = e / (KW * KW), t = e - c * (KW * KW);
        const int k = (((c >> lck) * ntg + (t >> lns)) << 4) + ((t & (NS - 1)) << lck) + (c & (CK - 1));
        float w[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < MT; ++m) w[m] = p.A[(long)m * p.lda + k];
        sW[e] = make_float4(w[0], w[1], w[2], w[3]);
    }
    __syncthreads();
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.X), 0, p.x_bytes, 0x00020000);
    const int groups_x = p.Wo / PX;
    const int total = p.Npix / PX;
    const int dx_first = tap_entry(0).z, dx_last = tap_entry(KW - 1).z;
    const int lo = dx_first < dx_last ? dx_first : dx_last;
    // Symmetric tap sets on inputs as wide as the output (every layer this kernel sees): each lane loads its own four input
    // pixels of a row with one 16-byte load and takes the HL halo pixels on each side from the neighbouring lanes, from its
    // own quad at a reflected image border, and from memory only as the first / last lane of a wave.  (Gathering the
    // PX + KW - 1 window per lane fetched every pixel up to KW times through requests that were all in flight together.)
    constexpr int HL = (KW - 1) / 2;
    const bool sym = lo == -HL && p.Wi == p.Wo && (p.in_sh % 4) == 0 && (p.in_sc % 4) == 0 && (p.in_sn % 4) == 0 &&
                     (((uintptr_t)p.X) & 15) == 0;
    const int lane = threadIdx.x & 63;
    const int rounds = (total - (int)blockIdx.x * 256 + (int)gridDim.x * 256 - 1) / ((int)gridDim.x * 256);   // uniform per workgroup
    int g = blockIdx.x * 256 + threadIdx.x;
    for (int it = 0; it < rounds; ++it, g += gridDim.x * 256) {
        const bool live = g < total;
        const int gg = live ? g : total - 1;
        const int xg = gg % groups_x; int r = gg / groups_x;
        const int oy = r % p.Ho; const int n = r / p.Ho;
        const int ox0 = xg * PX;
        const unsigned img_byte = (unsigned)(n * (int)p.in_sn) * 4u;
        float acc[MT][PX];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int q = 0; q < PX; ++q) acc[m][q] = 0.f;
        const bool first = xg == 0, last = xg == groups_x - 1;
        const bool memL = live && !first && lane == 0;
        const bool memR = live && !last && (lane == 63 || g + 1 >= total);
        unsigned cvo[NV];                                  // column byte offsets of this lane's NV inputs (gather form)
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            int ix = ox0 + lo + e;
            bool ok = live;
            if (p.reflect) { ix = ix < 0 ? -ix : ix; ix = ix >= p.Wi ? 2 * p.Wi - 2 - ix : ix; }
            else ok = ok && (unsigned)ix < (unsigned)p.Wi;
            cvo[e] = ok ? (unsigned)ix * 4u : C2M_OOB;
        }
        for (int i = 0; i < KW; ++i) {                    // tap rows (square kernel)
            int iy = oy + tap_entry(i * KW).y;
            bool rok = live;
            if (p.reflect) { iy = iy < 0 ? -iy : iy; iy = iy >= p.Hi ? 2 * p.Hi - 2 - iy : iy; }
            else rok = rok && (unsigned)iy < (unsigned)p.Hi;
            const unsigned rbase = img_byte + (unsigned)(iy * (int)p.in_sh) * 4u;
            unsigned vo[NV];
#pragma unroll
            for (int e = 0; e < NV; ++e) vo[e] = (rok && cvo[e] != C2M_OOB) ? rbase + cvo[e] : C2M_OOB;
            const unsigned own_vo = rok ? rbase + (unsigned)ox0 * 4u : C2M_OOB;
            const float4* __restrict__ wrow = sW + i * KW;
            for (int c = 0; c < Cin; ++c) {
                float v[NV];
                if (sym) {
                    const int soff = c * p.in_sc * 4;
                    const f32x4 own = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrsrc, own_vo, soff, 0));
                    v[HL + 0] = own.x; v[HL + 1] = own.y; v[HL + 2] = own.z; v[HL + 3] = own.w;
#pragma unroll
                    for (int e = 0; e < HL; ++e) {
                        const float ml = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                            xrsrc, (rok && memL) ? own_vo - (unsigned)(HL - e) * 4u : C2M_OOB, soff, 0));
                        const float mr = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                            xrsrc, (rok && memR) ? own_vo + (unsigned)(4 + e) * 4u : C2M_OOB, soff, 0));
                        const float up = __shfl_up(v[4 + e], 1, 64);                   // left neighbour's pixel 4 - HL + e
                        const float dn = __shfl_down(v[HL + e], 1, 64);                // right neighbour's pixel e
                        const float bl = p.reflect ? v[HL + HL - e] : 0.f;             // image border: own pixel HL - e
                        const float br = p.reflect ? v[HL + 2 - e] : 0.f;              //               own pixel 2 - e
                        v[e] = memL ? ml : (first ? bl : up);
                        v[HL + 4 + e] = memR ? mr : (last ? br : dn);
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < NV; ++e)
                        v[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, vo[e], c * p.in_sc * 4, 0));
                }
#pragma unroll
                for (int j = 0; j < KW; ++j) {
                    const float4 w4 = wrow[c * (KW * KW) + j];          // same address in every lane: LDS broadcast
                    const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
                    const int pos = xdesc ? KW - 1 - j : j;
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                        for (int q = 0; q < PX; ++q) acc[m][q] = fmaf(v[q + pos], wv[m], acc[m][q]);
                }
            }
        }
        if (!live) continue;
        float* __restrict__ yb = p.Y + p.out_off + (long)n * p.out_sn + (long)oy * p.out_sh + (long)ox0 * p.out_sw;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < p.M) {
                float o[PX];
#pragma unroll
                for (int q = 0; q < PX; ++q) {
                    float v = acc[m][q];
                    if (p.bias) v += p.bias[m];
                    o[q] = c2m_act(v, p.act, p.slope);
                }
                float* dst = yb + (long)m * p.out_sc;
                if (p.out_sw == 1 && (((uintptr_t)dst) & 15) == 0) {
                    *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
                } else {
#pragma unroll
                    for (int q = 0; q < PX; ++q) dst[(long)q * p.out_sw] = o[q];
                }
            }
        }
    }
}

template <int KW>
static int launch_thin_rows(const ConvP& p, int ns, int ntg, int Cin, int xdesc, hipStream_t s) {
    // few, fat blocks: every block first copies the layer's weights into LDS (Cin * KW * KW float4)
    long blocks = (p.Npix / 4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    dim3 grid((unsigned)blocks);
    const int lns = ns == 1 ? 0 : (ns == 2 ? 1 : 2);
    const size_t lds = (size_t)Cin * KW * KW * sizeof(float4);
    switch (p.M) {
        case 1: hipLaunchKernelGGL((conv_thin_rows_kernel<1, KW>), grid, dim3(256), lds, s, p, lns, ntg, Cin, xdesc); break;
        case 2: hipLaunchKernelGGL((conv_thin_rows_kernel<2, KW>), grid, dim3(256), lds, s, p, lns, ntg, Cin, xdesc); break;
        case 3: hipLaunchKernelGGL((conv_thin_rows_kernel<3, KW>), grid, dim3(256), lds, s, p, lns, ntg, Cin, xdesc); break;
        default: hipLaunchKernelGGL((conv_thin_rows_kernel<4, KW>), grid, dim3(256), lds, s, p, lns, ntg, Cin, xdesc); break;
    }
    return (int)hipGetLastError();
}

template <int NS>
static int launch_thin_fwd(const ConvP& p, hipStream_t s) {
    dim3 grid(c2m_grid(p.Npix, 256));
    switch (p.M) {
        case 1: hipLaunchKernelGGL((conv_thin_fwd_kernel<1, NS>), grid, dim3(256), 0, s, p); break;
        case 2: hipLaunchKernelGGL((conv_thin_fwd_kernel<2, NS>), grid, dim3(256), 0, s, p); break;
        case 3: hipLaunchKernelGGL((conv_thin_fwd_kernel<3, NS>), grid, dim3(256), 0, s, p); break;
        default: hipLaunchKernelGGL((conv_thin_fwd_kernel<4, NS>), grid, dim3(256), 0, s, p); break;
    }
    return (int)hipGetLastError();
}

int c2m_launch_thin_rows(const ConvP& p, int kw, int ns, int ntg, int Cin, int xdesc, hipStream_t s) {      // kw: 3 or 7
    if (kw == 3) return launch_thin_rows<3>(p, ns, ntg, Cin, xdesc, s);
    return launch_thin_rows<7>(p, ns, ntg, Cin, xdesc, s);
}

int c2m_launch_thin_fwd(const ConvP& p, int ns, hipStream_t s) {
    if (ns == 1) return launch_thin_fwd<1>(p, s);
    if (ns == 2) return launch_thin_fwd<2>(p, s);
    return launch_thin_fwd<4>(p, s);
}

// wgrad for <= 4 output channels: lanes = pixels, each thread keeps GPB*16*MT partial sums in registers over its
// pixels of the split, then a block reduction; slab layout identical to the MFMA wgrad so the same reduction finishes.
template <int MT, int NS, int GPB>
__global__ __launch_bounds__(256) void conv_thin_wgrad_kernel(const WgradP p, int ngroups_total) {
    constexpr int CK = 16 / NS;
    __shared__ float red[4][GPB * 16 * MT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g0 = blockIdx.x * GPB;
    const int split = blockIdx.z;
    const int pbeg = split * p.pix_per_split;
    int pend = pbeg + p.pix_per_split; pend = pend < p.Npix ? pend : p.Npix;
    const int in_st = (int)p.in_st, in_sh = (int)p.in_sh;
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.X), 0, p.x_bytes, 0x00020000);
    float acc[GPB][16][MT];
#pragma unroll
    for (int g = 0; g < GPB; ++g)
#pragma unroll
        for (int s = 0; s < 16; ++s)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[g][s][m] = 0.f;
    for (int pix = pbeg + threadIdx.x; pix < pend; pix += 256) {
        int n, ot, oy, ox;
        decompose_pix(pix, p, n, ot, oy, ox);
        const int sp = (ot * p.Ho + oy) * p.Wo + ox;
        float dy[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) dy[m] = m < p.M ? p.dY[(long)n * p.dy_sn + (long)m * p.dy_sc + sp] : 0.f;
        const unsigned ximg = (unsigned)(n * (int)p.in_sn) * 4u;
        const int ots = ot * p.st, oys = oy * p.sh, oxs = ox * p.sw;
#pragma unroll
        for (int g = 0; g < GPB; ++g) {
            const int grp = g0 + g;
            if (grp >= ngroups_total) break;
            const int4* __restrict__ jd = p.jtab + (long)grp * (1 + NS);
            const int4 hdr = jd[0];
            if (hdr.y == -2) {
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[g][0][m] += dy[m];
                continue;
            }
            unsigned vo[NS];
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                const int so = spatial_off(jd[1 + q], ots, oys, oxs, p.Ti, p.Hi, p.Wi, in_st, in_sh, p.reflect, p.is3d);
                vo[q] = so >= 0 ? ximg + (unsigned)so * 4u : C2M_OOB;
            }
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const float x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                    xrsrc, vo[s / CK], (hdr.x + (s % CK) * p.in_sc) * 4, 0));
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[g][s][m] = fmaf(dy[m], x, acc[g][s][m]);
            }
        }
    }
    // block reduction: wave shuffles, then 4 partials through LDS (fixed order)
#pragma unroll
    for (int g = 0; g < GPB; ++g)
#pragma unroll
        for (int s = 0; s < 16; ++s)
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const float v = wave_sum(acc[g][s][m]);
                if (lane == 0) red[wave][(g * 16 + s) * MT + m] = v;
            }
    __syncthreads();
    float* __restrict__ out = p.slab + (long)split * p.M * p.J;
    for (int i = threadIdx.x; i < GPB * 16 * MT; i += 256) {
        const int m = i % MT, gs = i / MT;
        const int col = g0 * 16 + gs;
        if (m < p.M && col < ngroups_total * 16)
            out[(long)m * p.J + col] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    }
}

// Row-blocked weight gradient for <= 4 output channels and a 2-D stride-1 square KW x KW kernel (the 7x7 RGB head, the 3x3
// flow / occlusion heads): a workgroup owns CPB input channels and ALL taps, every lane walks over groups of PX = 4
// horizontally adjacent pixels of the split: per tap row one gathered segment of PX + KW - 1 inputs feeds KW taps x PX pixels
// x MT outputs, i.e. 2.8x (7x7) / 2x (3x3) fewer loads per FMA than the per-pixel kernel above, which is bound by load
// issue (13 TF/s on the 7x7 head).  KW*KW*CPB*MT accumulators per lane (147 for the 7x7 head); block reduction and slab
// layout as above, so the same wgrad_reduce_kernel finishes.  Channel block 0 also sums dY for the bias gradient.
template <int MT, int KW, int CPB, int RI>
__global__ __launch_bounds__(256) void conv_thin_wgrad_rows_kernel(const WgradP p, int lns, int ntg, int Cin, int ngroups,
                                                                   int quads_per_split) {
    constexpr int PX = 4, NV = PX + KW - 1, NACC = CPB * RI * KW * MT;
    __shared__ float red[4][NACC + MT];
    const int NS = 1 << lns, lck = 4 - lns, CK = 16 >> lns;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.x * CPB;
    const int i0 = blockIdx.y * RI;              // first tap row of this workgroup (rows >= KW contribute nothing)
    const int split = blockIdx.z;
    const int groups_x = p.Wo / PX;
    const int total = p.Npix / PX;
    const int qbeg = split * quads_per_split;
    int qend = qbeg + quads_per_split; qend = qend < total ? qend : total;
    auto tap_entry = [&](int t) { return p.jtab[(t >> lns) * (1 + NS) + 1 + (t & (NS - 1))]; };   // chunk 0's taps
    const int dx0 = tap_entry(0).z, dy0 = tap_entry(0).y;        // row-major taps, dy / dx ascending by one
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.X), 0, p.x_bytes, 0x00020000);
    float acc[CPB][RI][KW][MT];
    float accb[MT];
#pragma unroll
    for (int c = 0; c < CPB; ++c)
#pragma unroll
        for (int i = 0; i < RI; ++i)
#pragma unroll
            for (int j = 0; j < KW; ++j)
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[c][i][j][m] = 0.f;
#pragma unroll
    for (int m = 0; m < MT; ++m) accb[m] = 0.f;
    // Two register sets: the loads of pixel group g + 256 (all KW rows x CPB channels: one latency per group instead of one
    // per row) are in flight while group g is accumulated; the kernel runs one wave per SIMD (147 accumulators for the 7x7
    // head), so nothing else would hide them.  Groups past the split's end load through out-of-range offsets (zeros).
    // Input row segments: every lane loads its own four pixels once (one 16-byte load per row; the per-tap gathers of the
    // first version fetched each pixel up to KW times through separate requests that were all in flight together, and the
    // L2 served every one of them).  The HL halo pixels on each side come from the neighbouring lanes (shuffles in
    // accumulate()), from the pixel's own quad at a reflected image border, and from memory only for the first / last live
    // lane of a wave.
    constexpr int HL = (KW - 1) / 2;
    auto load_group = [&](int g, float (&dy)[MT][PX], float (&v)[RI][CPB][NV], int& fl) {
        const bool live = g < qend;
        const int gg = live ? g : qend - 1;
        const int xg = gg % groups_x; const int r = gg / groups_x;
        const int oy = r % p.Ho; const int n = r / p.Ho;
        const int ox0 = xg * PX;
        const bool first = xg == 0, last = xg == groups_x - 1;
        const bool memL = live && !first && lane == 0;
        const bool memR = live && !last && (lane == 63 || g + 1 >= qend);
        fl = (first ? 2 : 0) | (last ? 4 : 0) | (memL ? 8 : 0) | (memR ? 16 : 0);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < p.M && live) {
                const float4 t = *reinterpret_cast<const float4*>(p.dY + (long)n * p.dy_sn + (long)m * p.dy_sc + (long)oy * p.Wo + ox0);
                dy[m][0] = t.x; dy[m][1] = t.y; dy[m][2] = t.z; dy[m][3] = t.w;
            } else {
#pragma unroll
                for (int q = 0; q < PX; ++q) dy[m][q] = 0.f;
            }
        }
        const unsigned img_byte = (unsigned)(n * (int)p.in_sn) * 4u;
#pragma unroll
        for (int i = 0; i < RI; ++i) {
            int iy = oy + dy0 + i0 + i;
            bool rok = live && i0 + i < KW;
            if (p.reflect) { iy = iy < 0 ? -iy : iy; iy = iy >= p.Hi ? 2 * p.Hi - 2 - iy : iy; }
            else rok = rok && (unsigned)iy < (unsigned)p.Hi;
            const unsigned rbase = img_byte + (unsigned)(iy * (int)p.in_sh + ox0) * 4u;
#pragma unroll
            for (int c = 0; c < CPB; ++c) {
                const bool cok = rok && c0 + c < Cin;
                const int soff = (c0 + c) * p.in_sc * 4;
                const f32x4 own = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrsrc, cok ? rbase : C2M_OOB, soff, 0));
                v[i][c][HL + 0] = own.x; v[i][c][HL + 1] = own.y; v[i][c][HL + 2] = own.z; v[i][c][HL + 3] = own.w;
#pragma unroll
                for (int e = 0; e < HL; ++e) {
                    v[i][c][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                        xrsrc, (cok && memL) ? rbase - (unsigned)(HL - e) * 4u : C2M_OOB, soff, 0));
                    v[i][c][HL + 4 + e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                        xrsrc, (cok && memR) ? rbase + (unsigned)(4 + e) * 4u : C2M_OOB, soff, 0));
                }
            }
        }
    };
    auto accumulate = [&](const float (&dy)[MT][PX], float (&v)[RI][CPB][NV], const int fl) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int q = 0; q < PX; ++q) accb[m] += dy[m][q];
#pragma unroll
        for (int i = 0; i < RI; ++i)
#pragma unroll
            for (int c = 0; c < CPB; ++c) {
#pragma unroll
                for (int e = 0; e < HL; ++e) {
#ifdef C2M_THIN_DPP      // bisect build (tools/concurrency_stress.py): whole-wave DPP shifts instead of ds_bpermute_b32 through the LDS crossbar
                    const int su = __builtin_bit_cast(int, v[i][c][4 + e]), sd = __builtin_bit_cast(int, v[i][c][HL + e]);
                    const float up = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(su, su, 0x138, 0xf, 0xf, false));   // wave_shr:1
                    const float dn = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(sd, sd, 0x130, 0xf, 0xf, false));   // wave_shl:1
#else
                    const float up = __shfl_up(v[i][c][4 + e], 1, 64);                 // left neighbour's pixel 4 - HL + e
                    const float dn = __shfl_down(v[i][c][HL + e], 1, 64);              // right neighbour's pixel e
#endif
                    const float bl = p.reflect ? v[i][c][HL + HL - e] : 0.f;           // image border: own pixel HL - e
                    const float br = p.reflect ? v[i][c][HL + 2 - e] : 0.f;            //               own pixel 2 - e
                    v[i][c][e] = (fl & 8) ? v[i][c][e] : ((fl & 2) ? bl : up);
                    v[i][c][HL + 4 + e] = (fl & 16) ? v[i][c][HL + 4 + e] : ((fl & 4) ? br : dn);
                }
#pragma unroll
                for (int j = 0; j < KW; ++j)
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                        for (int q = 0; q < PX; ++q) acc[c][i][j][m] = fmaf(dy[m][q], v[i][c][q + j], acc[c][i][j][m]);
            }
    };
    float dyA[MT][PX], dyB[MT][PX];
    float vA[RI][CPB][NV], vB[RI][CPB][NV];
    int flA = 0, flB = 0;
    int g = qbeg + threadIdx.x;
    if (qbeg < qend) {
        load_group(g, dyA, vA, flA);
        // uniform trip count (whole workgroup): the shuffles in accumulate() need every lane of the wave
        const int rounds = (qend - qbeg + 511) / 512;
        for (int it = 0; it < rounds; ++it, g += 512) {
            load_group(g + 256, dyB, vB, flB);
            accumulate(dyA, vA, flA);
            load_group(g + 512, dyA, vA, flA);
            accumulate(dyB, vB, flB);
        }
    }
    // block reduction: wave shuffles, then 4 partials through LDS (fixed order)
#pragma unroll
    for (int c = 0; c < CPB; ++c)
#pragma unroll
        for (int i = 0; i < RI; ++i)
#pragma unroll
            for (int j = 0; j < KW; ++j)
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const float v = wave_sum(acc[c][i][j][m]);
                    if (lane == 0) red[wave][((c * RI + i) * KW + j) * MT + m] = v;
                }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const float v = wave_sum(accb[m]);
        if (lane == 0) red[wave][NACC + m] = v;
    }
    __syncthreads();
    float* __restrict__ out = p.slab + (long)split * p.M * p.J;
    for (int e = threadIdx.x; e < NACC + MT; e += 256) {
        const float v = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
        if (e >= NACC) {                                          // bias gradient column (ones group), channel block 0 only
            const int m = e - NACC;
            if (blockIdx.x == 0 && blockIdx.y == 0 && m < p.M) out[(long)m * p.J + ngroups * 16] = v;
            continue;
        }
        const int m = e % MT, j = (e / MT) % KW, i = i0 + (e / (MT * KW)) % RI, c = c0 + e / (MT * KW * RI);
        const int t = i * KW + j;
        if (m >= p.M || c >= Cin || i >= KW) continue;
        const int col = (((c >> lck) * ntg + (t >> lns)) << 4) + ((t & (NS - 1)) << lck) + (c & (CK - 1));
        out[(long)m * p.J + col] = v;
    }
}

// The two weight-gradient launchers: S = the splits the caller's slab holds (c2m_conv_wgrad_splits); they return the number of
// splits they wrote, in the slab layout of the MFMA weight gradient, for c2m_conv_wgrad's reduction.
int c2m_launch_thin_wgrad_rows(const WgradP& p, int kw, int NS, int ntg, int Cin, int ngroups, int S, hipStream_t s) {
    const int lns = NS == 1 ? 0 : (NS == 2 ? 1 : 2);
    // tap rows per workgroup: everything must fit the 256 architectural VGPRs (see the kernel)
    const int cpb = kw == 7 ? 1 : 2, ri = kw == 7 ? (p.M == 1 ? 4 : (p.M == 2 ? 3 : 2)) : 3;
    const int cblocks = c2m_cdiv(Cin, cpb);
    const int quads = p.Npix / 4;
    const int units = cblocks * c2m_cdiv(kw, ri);
    int St = (1024 + units - 1) / units;          // ~1024 workgroups, >= 2048 pixel groups each
    if (St > S) St = S;                           // the caller's slab holds S splits
    if (St > c2m_cdiv(quads, 2048)) St = c2m_cdiv(quads, 2048);
    if (St < 1) St = 1;
    const int qps = c2m_cdiv(quads, St);
    const int Srows = c2m_cdiv(quads, qps);
    dim3 rg(cblocks, c2m_cdiv(kw, ri), Srows);
#define C2M_THIN_WR(MT, RI7) \
    if (kw == 7) hipLaunchKernelGGL((conv_thin_wgrad_rows_kernel<MT, 7, 1, RI7>), rg, dim3(256), 0, s, p, lns, ntg, Cin, ngroups, qps); \
    else         hipLaunchKernelGGL((conv_thin_wgrad_rows_kernel<MT, 3, 2, 3>), rg, dim3(256), 0, s, p, lns, ntg, Cin, ngroups, qps);
    if (p.M == 1) { C2M_THIN_WR(1, 4) } else if (p.M == 2) { C2M_THIN_WR(2, 3) } else { C2M_THIN_WR(3, 2) }   // 4 output rows would spill
#undef C2M_THIN_WR
    return Srows;
}

int c2m_launch_thin_wgrad(WgradP p, int NS, int ngroups, int S, hipStream_t s) {
    constexpr int GPB = 2;
    const int ng = ngroups + 1;                       // real groups + the ones group
    // pixel splits sized for ~1024 blocks but >= 16K pixels each (the block reduction is per block)
    int St = (1024 + c2m_cdiv(ng, GPB) - 1) / c2m_cdiv(ng, GPB);
    const int maxS = S;                               // the caller's slab holds S splits
    if (St > maxS) St = maxS;
    if (St < 1) St = 1;
    int per2 = ((c2m_cdiv(p.Npix, St) + 255) / 256) * 256;
    p.pix_per_split = per2;
    const int Sthin = c2m_cdiv(p.Npix, per2);
    dim3 tg(c2m_cdiv(ng, GPB), 1, Sthin);
#define C2M_THIN_W(MT) \
    if (NS == 1)      hipLaunchKernelGGL((conv_thin_wgrad_kernel<MT, 1, GPB>), tg, dim3(256), 0, s, p, ng); \
    else if (NS == 2) hipLaunchKernelGGL((conv_thin_wgrad_kernel<MT, 2, GPB>), tg, dim3(256), 0, s, p, ng); \
    else              hipLaunchKernelGGL((conv_thin_wgrad_kernel<MT, 4, GPB>), tg, dim3(256), 0, s, p, ng);
    if (p.M == 1) { C2M_THIN_W(1) } else if (p.M == 2) { C2M_THIN_W(2) } else if (p.M == 3) { C2M_THIN_W(3) } else { C2M_THIN_W(4) }
#undef C2M_THIN_W
    return Sthin;
}
