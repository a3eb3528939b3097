// Weight packing for the convolution kernels: fp32 K-order matrices (conv_igemm.hip, conv_patch.hip, conv_thin.hip), the bf16
// images of the LDS-patch and NC8 forms (conv_patch.hip, conv_gather.hip, conv_nc8.hip), and one launch for many layers.
//
// Native conv weights -> the kernels' K order in one pass (coalesced writes, gathered reads; weights sit in L2).
//   out[r][((chunk * ntg + tg) * NS + slot) * CK + ch],  r = cls * M + m,  c = chunk*CK + ch,  tap = tg*NS + slot
//   source element: w[m*s_m + c*s_c + ((at*st + rt)*KH + (ay*sh + ry))*KW + (ax*sw + rx)]
//   with tap = (at, ay, ax) over (At, Ay, Ax) = (KT/st, KH/sh, KW/sw) and cls = (rt, ry, rx) over (st, sh, sw).
// Forward: st = sh = sw = 1, s_m = C*taps, s_c = taps.  Data gradient (rows = input channels, K = output channels,
// one class per stride parity): s_m = taps_full, s_c = M*taps_full.  Padding (c >= C or tap >= taps) is written as 0.
#include "common.h"
#include "conv_types.h"
#include <string.h>

struct PackP { int M, C, CK, NS, nch, ntg, At, Ay, Ax, st, sh, sw, KH, KW; long s_m, s_c; };

// one workgroup row per packed row r = cls*M + m (blockIdx.y); the per-tap source offsets of the row's parity class are
// computed once into LDS, CK / NS are powers of two: one integer division (by ntg) per element remains
template <int CK>
__device__ __forceinline__ void pack_weights_row(const float* __restrict__ w, float* __restrict__ out, const PackP& q, int* toff,
                                                 const int r, const int bx, const int nbx) {
    constexpr int NS = 16 / CK, LCK = CK == 16 ? 4 : (CK == 8 ? 3 : 2), LNS = 4 - LCK;
    const int taps = q.At * q.Ay * q.Ax;
    const int lda = q.nch * q.ntg * 16;
    const int m = r % q.M; int cls = r / q.M;
    const int rx = cls % q.sw; cls /= q.sw;
    const int ry = cls % q.sh; const int rt = cls / q.sh;
    for (int tap = threadIdx.x; tap < taps; tap += 256) {
        const int ax = tap % q.Ax; const int ay = (tap / q.Ax) % q.Ay; const int at = tap / (q.Ax * q.Ay);
        toff[tap] = ((at * q.st + rt) * q.KH + (ay * q.sh + ry)) * q.KW + (ax * q.sw + rx);
    }
    __syncthreads();
    const float* __restrict__ wr = w + m * q.s_m;
    float* __restrict__ orow = out + (long)r * lda;
    for (int k = bx * 256 + threadIdx.x; k < lda; k += nbx * 256) {
        const int ch = k & (CK - 1); int t = k >> LCK;
        const int slot = t & (NS - 1); t >>= LNS;
        const int chunk = t / q.ntg, tg = t - chunk * q.ntg;
        const int c = chunk * CK + ch, tap = tg * NS + slot;
        orow[k] = (c < q.C && tap < taps) ? wr[c * q.s_c + toff[tap]] : 0.f;
    }
}

template <int CK>
__global__ __launch_bounds__(256) void pack_weights_kernel(const float* __restrict__ w, float* __restrict__ out,
                                                            const PackP q) {
    __shared__ int toff[128];
    pack_weights_row<CK>(w, out, q, toff, blockIdx.y, blockIdx.x, gridDim.x);
}

// bf16 weights of the bf16 LDS-patch kernel: out[chunk][tap][row (padded to Mpad)][16 channels] in bf16, RNE; rows >= M
// and channels >= C are zero.  3x3 taps only; forward (flip = 0): tap = ky*3+kx of w[m][c][ky][kx] addressed through
// s_m / s_c as in c2m_pack_weights; data gradient (flip = 1): the tap index is reversed (rotated filter).
__device__ __forceinline__ void pack_weights_bf16_patch_body(const float* __restrict__ w, uint4* __restrict__ out, int M, int C,
                                                             int Mpad, long s_m, long s_c, int flip, long units, long b0, long nb) {
    for (long u = b0 * (long)blockDim.x + threadIdx.x; u < units; u += nb * blockDim.x) {
        const int half = (int)(u & 1); long r = u >> 1;
        const int m = (int)(r % Mpad); r /= Mpad;
        int tap, chunk, st;
        if (flip == 2) {
            // 4x4 stride-2 layers on the parity-plane kernel (conv_nc8.hip, S2): out[16-channel chunk][parity py*2+px][tap a*2+b]
            // [row][16 channels] with original tap (ky, kx) = (2a + 1 - py, 2b + 1 - px)
            const int t4 = (int)(r % 4); r /= 4;
            const int par = (int)(r % 4); chunk = (int)(r / 4);
            st = (2 * (t4 >> 1) + 1 - (par >> 1)) * 4 + 2 * (t4 & 1) + 1 - (par & 1);
        } else if (flip == 3 || flip == 4) {
            // data gradient of those layers (conv_s2_dgrad_nc8_kernel): 16 virtual taps vt = class (ri, rj) * 4 + a * 2 + b with
            // ky = zeros: ri ? 2a : 2a + 1, reflect: ri ? 2a + 1 : 2a (same along x); rows = input channels, reduction = output channels
            const int vt = (int)(r % 16); chunk = (int)(r / 16);
            const int ri = vt >> 3, rj = (vt >> 2) & 1, a = (vt >> 1) & 1, b = vt & 1;
            const int ky = flip == 3 ? (ri ? 2 * a : 2 * a + 1) : (ri ? 2 * a + 1 : 2 * a);
            const int kx = flip == 3 ? (rj ? 2 * b : 2 * b + 1) : (rj ? 2 * b + 1 : 2 * b);
            st = ky * 4 + kx;
        } else {
            tap = (int)(r % 9); chunk = (int)(r / 9);
            st = flip ? 8 - tap : tap;
        }
        bf16x8 q;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = chunk * 16 + half * 8 + j;
            q[j] = (__bf16)((m < M && c < C) ? w[m * s_m + c * s_c + st] : 0.f);
        }
        out[u] = __builtin_bit_cast(uint4, q);
    }
}

// bf16 weights of the NC8 gather kernel: out[class][tap][16-channel chunk][half][row (padded to Mpad)] 16-byte units, RNE; the
// source element of (class, tap, m, c) is the one pack_weights_row reads (PackP with CK = 16); rows >= M and channels >= C are zero.
__device__ __forceinline__ void pack_weights_bf16_gather_body(const float* __restrict__ w, uint4* __restrict__ out, const PackP& q,
                                                              int Mpad, long units, long b0, long nb) {
    const int taps = q.At * q.Ay * q.Ax;
    for (long u = b0 * (long)blockDim.x + threadIdx.x; u < units; u += nb * blockDim.x) {
        const int m = (int)(u % Mpad); long r = u / Mpad;
        const int half = (int)(r & 1); r >>= 1;
        const int chunk = (int)(r % q.nch); r /= q.nch;
        const int tap = (int)(r % taps); int cls = (int)(r / taps);
        const int rx = cls % q.sw; cls /= q.sw;
        const int ry = cls % q.sh; const int rt = cls / q.sh;
        const int ax = tap % q.Ax, ay = (tap / q.Ax) % q.Ay, at = tap / (q.Ax * q.Ay);
        const long toff = ((at * q.st + rt) * q.KH + (ay * q.sh + ry)) * q.KW + (ax * q.sw + rx);
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = chunk * 16 + half * 8 + j;
            v[j] = (__bf16)((m < q.M && c < q.C) ? w[m * q.s_m + c * q.s_c + toff] : 0.f);
        }
        out[u] = __builtin_bit_cast(uint4, v);
    }
}

__global__ void pack_weights_bf16_gather_kernel(const float* __restrict__ w, uint4* __restrict__ out, const PackP q, int Mpad,
                                                long units) {
    pack_weights_bf16_gather_body(w, out, q, Mpad, units, blockIdx.x, gridDim.x);
}

__global__ void pack_weights_bf16_patch_kernel(const float* __restrict__ w, uint4* __restrict__ out, int M, int C, int Mpad,
                                               long s_m, long s_c, int flip, long units) {
    pack_weights_bf16_patch_body(w, out, M, C, Mpad, s_m, s_c, flip, units, blockIdx.x, gridDim.x);
}

// out: ceil(C/16) * 9 * Mpad * 32 bytes with Mpad = ceil(M/128)*128.  g[]: 0 M, 1 C, 2 s_m, 3 s_c, 4 flip.
C2M_API long c2m_pack_weights_bf16_patch_bytes(int M, int C) {
    return (long)c2m_cdiv(C, 16) * 9 * (c2m_cdiv(M, 128) * 128) * 32;
}
// (flip = 2: the 4x4 stride-2 parity form, 16 (parity, tap) slots per chunk instead of 9 taps)
C2M_API long c2m_pack_weights_bf16_s2_bytes(int M, int C) {
    return (long)c2m_cdiv(C, 16) * 16 * (c2m_cdiv(M, 128) * 128) * 32;
}

C2M_API int c2m_pack_weights_bf16_patch(const float* w, void* out, const int64_t* g, void* stream) {
    C2M_ENTER();
    const int M = (int)g[0], C = (int)g[1];
    if (M <= 0 || C <= 0) return 0;
    if ((((uintptr_t)out) & 15) != 0) return (int)hipErrorInvalidValue;
    const int Mpad = c2m_cdiv(M, 128) * 128;
    const long units = (long)c2m_cdiv(C, 16) * (g[4] >= 2 ? 16 : 9) * Mpad * 2;
    hipLaunchKernelGGL(pack_weights_bf16_patch_kernel, dim3(c2m_grid(units, 256)), dim3(256), 0, (hipStream_t)stream, w,
                       (uint4*)out, M, C, Mpad, (long)g[2], (long)g[3], (int)g[4], units);
    return (int)hipGetLastError();
}

// g[]: 0 M, 1 C, 2 CK, 3 KT, 4 KH, 5 KW, 6 st, 7 sh, 8 sw, 9 s_m, 10 s_c;  out holds st*sh*sw * M rows of
// ceil(C/CK) * ceil(taps/NS) * 16 floats (NS = 16/CK, taps = (KT/st)*(KH/sh)*(KW/sw)).
static int pack_params(const int64_t* g, PackP& q, long& rows, int& lda) {
    q.M = (int)g[0]; q.C = (int)g[1]; q.CK = (int)g[2];
    const int KT = (int)g[3];
    q.KH = (int)g[4]; q.KW = (int)g[5]; q.st = (int)g[6]; q.sh = (int)g[7]; q.sw = (int)g[8];
    q.s_m = g[9]; q.s_c = g[10];
    rows = 0; lda = 0;
    if (q.M <= 0 || q.C <= 0) return 0;
    if ((q.CK != 4 && q.CK != 8 && q.CK != 16) || q.st < 1 || q.sh < 1 || q.sw < 1 || KT % q.st || q.KH % q.sh ||
        q.KW % q.sw) return (int)hipErrorInvalidValue;
    q.NS = 16 / q.CK;
    q.At = KT / q.st; q.Ay = q.KH / q.sh; q.Ax = q.KW / q.sw;
    q.nch = c2m_cdiv(q.C, q.CK); q.ntg = c2m_cdiv(q.At * q.Ay * q.Ax, q.NS);
    rows = (long)q.st * q.sh * q.sw * q.M;
    lda = q.nch * q.ntg * 16;
    if (q.At * q.Ay * q.Ax > 128 || rows > 65535) return (int)hipErrorInvalidValue;
    return 0;
}

// g[] as c2m_pack_weights (g[2] = CK must be 16).  out: prod(stride) class images of taps * ceil(C/16) * 2 * Mpad 16-byte units
// (taps = (KT/st)(KH/sh)(KW/sw), Mpad = ceil(M/128)*128), classes in (rt, ry, rx) row-major order.
C2M_API long c2m_pack_weights_bf16_gather_bytes(const int64_t* g) {
    PackP q; long rows; int lda;
    if (pack_params(g, q, rows, lda) || rows == 0 || q.CK != 16) return -1;
    return (long)q.st * q.sh * q.sw * q.At * q.Ay * q.Ax * q.nch * 2 * (c2m_cdiv(q.M, 128) * 128) * 16;
}

C2M_API int c2m_pack_weights_bf16_gather(const float* w, void* out, const int64_t* g, void* stream) {
    C2M_ENTER();
    PackP q; long rows; int lda;
    const int rc = pack_params(g, q, rows, lda);
    if (rc || rows == 0) return rc;
    if (q.CK != 16 || (((uintptr_t)out) & 15)) return (int)hipErrorInvalidValue;
    const int Mpad = c2m_cdiv(q.M, 128) * 128;
    const long units = (long)q.st * q.sh * q.sw * q.At * q.Ay * q.Ax * q.nch * 2 * Mpad;
    hipLaunchKernelGGL(pack_weights_bf16_gather_kernel, dim3(c2m_grid(units, 256)), dim3(256), 0, (hipStream_t)stream, w, (uint4*)out,
                       q, Mpad, units);
    return (int)hipGetLastError();
}

C2M_API int c2m_pack_weights(const float* w, float* out, const int64_t* g, void* stream) {
    C2M_ENTER();
    PackP q; long rows; int lda;
    const int rc = pack_params(g, q, rows, lda);
    if (rc || rows == 0) return rc;
    dim3 grid(c2m_cdiv(lda, 1024) < 1 ? 1 : c2m_cdiv(lda, 1024), (unsigned)rows);
    if (q.CK == 16)     hipLaunchKernelGGL((pack_weights_kernel<16>), grid, dim3(256), 0, (hipStream_t)stream, w, out, q);
    else if (q.CK == 8) hipLaunchKernelGGL((pack_weights_kernel<8>), grid, dim3(256), 0, (hipStream_t)stream, w, out, q);
    else                hipLaunchKernelGGL((pack_weights_kernel<4>), grid, dim3(256), 0, (hipStream_t)stream, w, out, q);
    return (int)hipGetLastError();
}

// ---- all packs of a model in ONE launch (round 3).  With an optimizer in the step every trainable weight is re-packed once per
// step and layout -- ~195 launches of 5-7 us in a full G + D step (1.3 ms of GPU time, more host time than that in eager mode).
// The host keeps one PackJob per (weight, layout) it has packed before (c2m_pack_job_fill), the table lives in device memory,
// and after the optimizer step one launch refreshes every pack in place: workgroup b finds its job by bisection over the jobs'
// first workgroup index.  type 0: c2m_pack_weights (g[11]); type 1: c2m_pack_weights_bf16_patch (g[5]); type 2:
// c2m_pack_weights_bf16_gather (g[11]).
struct PackJob {
    const float* w; void* out;
    PackP q;                                                  // type 0
    int M, C, Mpad, flip; long s_m, s_c, units;               // type 1
    int type; unsigned first, xblocks, nblocks;
};

C2M_API int c2m_pack_job_bytes(void) { return (int)sizeof(PackJob); }

// fills *job (host memory, c2m_pack_job_bytes() bytes); returns the number of workgroups the job takes, < 0 on bad geometry
C2M_API long c2m_pack_job_fill(void* job, int type, const void* w, void* out, const int64_t* g, unsigned first_block) {
    PackJob j;
    memset(&j, 0, sizeof(j));
    j.w = (const float*)w; j.out = out; j.type = type; j.first = first_block;
    if (type == 0) {
        long rows; int lda;
        if (pack_params(g, j.q, rows, lda) || rows == 0) return -1;
        j.xblocks = (unsigned)(c2m_cdiv(lda, 1024) < 1 ? 1 : c2m_cdiv(lda, 1024));
        j.nblocks = j.xblocks * (unsigned)rows;
    } else if (type == 1) {
        j.M = (int)g[0]; j.C = (int)g[1]; j.s_m = g[2]; j.s_c = g[3]; j.flip = (int)g[4];
        if (j.M <= 0 || j.C <= 0 || (((uintptr_t)out) & 15) != 0) return -1;
        j.Mpad = c2m_cdiv(j.M, 128) * 128;
        j.units = (long)c2m_cdiv(j.C, 16) * (j.flip >= 2 ? 16 : 9) * j.Mpad * 2;
        j.xblocks = 1;
        j.nblocks = (unsigned)c2m_grid(j.units, 256);
    } else if (type == 2) {                                   // c2m_pack_weights_bf16_gather (g[11])
        long rows; int lda;
        if (pack_params(g, j.q, rows, lda) || rows == 0 || j.q.CK != 16 || (((uintptr_t)out) & 15) != 0) return -1;
        j.Mpad = c2m_cdiv(j.q.M, 128) * 128;
        j.units = (long)j.q.st * j.q.sh * j.q.sw * j.q.At * j.q.Ay * j.q.Ax * j.q.nch * 2 * j.Mpad;
        j.xblocks = 1;
        j.nblocks = (unsigned)c2m_grid(j.units, 256);
    } else {
        return -1;
    }
    memcpy(job, &j, sizeof(j));
    return (long)j.nblocks;
}

__global__ __launch_bounds__(256) void pack_multi_kernel(const PackJob* __restrict__ jobs, const int2* __restrict__ blocktab) {
    __shared__ int toff[128];
    // (job, workgroup within the job) of this workgroup from a host-built table: the first form bisected over the jobs' first
    // workgroup index -- eight dependent global loads (~5 us) in front of ~1 us of copying, 185 us per launch on the G + D set
    const int2 e = blocktab[blockIdx.x];
    const PackJob& j = jobs[e.x];
    const unsigned lb = (unsigned)e.y;
    if (j.type == 0) {
        const int r = (int)(lb / j.xblocks), bx = (int)(lb % j.xblocks);
        const PackP q = j.q;
        if (q.CK == 16)     pack_weights_row<16>(j.w, (float*)j.out, q, toff, r, bx, (int)j.xblocks);
        else if (q.CK == 8) pack_weights_row<8>(j.w, (float*)j.out, q, toff, r, bx, (int)j.xblocks);
        else                pack_weights_row<4>(j.w, (float*)j.out, q, toff, r, bx, (int)j.xblocks);
    } else if (j.type == 2) {
        const PackP q = j.q;
        pack_weights_bf16_gather_body(j.w, (uint4*)j.out, q, j.Mpad, j.units, lb, j.nblocks);
    } else {
        pack_weights_bf16_patch_body(j.w, (uint4*)j.out, j.M, j.C, j.Mpad, j.s_m, j.s_c, j.flip, j.units, lb, j.nblocks);
    }
}

// jobs: device copy of njobs PackJob records; blocktab: device int32 pairs (job index, workgroup index within the job), one per
// workgroup of the launch, in any order (total_blocks = the sum of the jobs' workgroup counts)
C2M_API int c2m_pack_multi(const void* jobs, const void* blocktab, int njobs, long total_blocks, void* stream) {
    C2M_ENTER();
    if (njobs <= 0 || total_blocks <= 0) return 0;
    if (total_blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_multi_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, (const PackJob*)jobs,
                       (const int2*)blocktab);
    return (int)hipGetLastError();
}
