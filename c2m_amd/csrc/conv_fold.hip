// Reflect fold: the gradient of a reflect-padded tensor folded back onto the unpadded one (whole fold, or the pad ring added to
// an interior the conv data gradient already wrote).  Used by every conv route (igemm, NC8, Winograd).
#include "common.h"
#include "dtype.h"
#include "conv_types.h"
#include <stdlib.h>

// dX[n,c,t,y,x] = sum of dXpad over every padded coordinate that reflects onto (t,y,x); fixed order.
struct FoldP { int T, H, W, pt, ph, pw; long total; };

__device__ __forceinline__ int fold_sources(int i, int I, int p, int* src) {
    int n = 0;
    src[n++] = i + p;
    if (p > 0) {
        if (i >= 1 && i <= p) src[n++] = p - i;
        if (i >= I - 1 - p && i <= I - 2) src[n++] = 2 * (I - 1) - i + p;
    }
    return n;
}

template <class T>
__global__ void reflect_fold_kernel(const T* __restrict__ dXp, T* __restrict__ dX, const FoldP f) {
    const int Tp = f.T + 2 * f.pt, Hp = f.H + 2 * f.ph, Wp = f.W + 2 * f.pw;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < f.total; idx += (long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % f.W); long r = idx / f.W;
        const int y = (int)(r % f.H); r /= f.H;
        const int t = (int)(r % f.T); const long nc = r / f.T;
        int st[3], sy[3], sx[3];
        const int nt = fold_sources(t, f.T, f.pt, st), ny = fold_sources(y, f.H, f.ph, sy),
                  nx = fold_sources(x, f.W, f.pw, sx);
        const T* __restrict__ base = dXp + nc * (long)Tp * Hp * Wp;
        float acc = 0.f;
        for (int a = 0; a < nt; ++a)
            for (int b = 0; b < ny; ++b)
                for (int c = 0; c < nx; ++c) acc += c2m_ld(base, ((long)st[a] * Hp + sy[b]) * Wp + sx[c]);
        c2m_st(dX, idx, acc);
    }
}

// W % 4 == 0: a thread owns four consecutive x.  Their direct sources are four consecutive floats of the padded row (one
// 4-byte aligned 16-byte load); mirrored x sources exist only for elements within `pad` of a border and are added per
// element.  Summation order: per (t, y) source pair the direct x term plus its mirrored x terms first, then the pairs in
// (t, y) order -- NOT the scalar kernel's strictly sequential order (the mirrored x terms are added to the direct term
// before the pair joins the running sum), so the two kernels agree to rounding, not bit for bit; either is deterministic.
__device__ __forceinline__ f32x4 fold_ld4u(const float* __restrict__ p) {      // 4-byte aligned 16-byte load
    typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
    return *reinterpret_cast<const f32x4u*>(p);
}
__device__ __forceinline__ f32x4 fold_ld4u(const bf16_t* __restrict__ p) {     // 2-byte aligned 8-byte load (unaligned access mode)
    uint2 r;
    __builtin_memcpy(&r, p, 8);
    const f32x4 v = {__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16),
                     __uint_as_float(r.y & 0xffff0000u)};
    return v;
}

template <class T>
__global__ void reflect_fold_vec_kernel(const T* __restrict__ dXp, T* __restrict__ dX, const FoldP f) {
    typedef float f32x4a __attribute__((ext_vector_type(4)));
    const int Tp = f.T + 2 * f.pt, Hp = f.H + 2 * f.ph, Wp = f.W + 2 * f.pw;
    const int W4 = f.W >> 2;
    const long total4 = f.total >> 2;
    for (long i4 = blockIdx.x * (long)blockDim.x + threadIdx.x; i4 < total4; i4 += (long)gridDim.x * blockDim.x) {
        const int x0 = (int)(i4 % W4) * 4; long r = i4 / W4;
        const int y = (int)(r % f.H); r /= f.H;
        const int t = (int)(r % f.T); const long nc = r / f.T;
        int st[3], sy[3];
        const int nt = fold_sources(t, f.T, f.pt, st), ny = fold_sources(y, f.H, f.ph, sy);
        const T* __restrict__ base = dXp + nc * (long)Tp * Hp * Wp;
        const bool xband = f.pw > 0 && (x0 <= f.pw || x0 + 3 >= f.W - 1 - f.pw);     // some element has mirrored x sources
        f32x4a acc = {0.f, 0.f, 0.f, 0.f};
        for (int a = 0; a < nt; ++a)
            for (int b = 0; b < ny; ++b) {
                const T* __restrict__ row = base + ((long)st[a] * Hp + sy[b]) * Wp;
                f32x4a v = fold_ld4u(row + x0 + f.pw);
                if (xband) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        int sx[3];
                        const int nx = fold_sources(x0 + e, f.W, f.pw, sx);
                        for (int c = 1; c < nx; ++c) v[e] += c2m_ld(row, sx[c]);
                    }
                }
                acc += v;
            }
        c2m_st4(dX + i4 * 4, make_float4(acc[0], acc[1], acc[2], acc[3]));
    }
}

// In-place variant for the two-target dgrad: dX already holds the direct term, add the mirrored pad-ring terms
// (only pixels within `pad` of a border have any).  Generic form: every element looks for extra sources.
template <class T>
__global__ void reflect_border_add_kernel(const T* __restrict__ dXp, T* __restrict__ dX, const FoldP f) {
    const int Tp = f.T + 2 * f.pt, Hp = f.H + 2 * f.ph, Wp = f.W + 2 * f.pw;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < f.total; idx += (long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % f.W); long r = idx / f.W;
        const int y = (int)(r % f.H); r /= f.H;
        const int t = (int)(r % f.T); const long nc = r / f.T;
        int st[3], sy[3], sx[3];
        const int nt = fold_sources(t, f.T, f.pt, st), ny = fold_sources(y, f.H, f.ph, sy),
                  nx = fold_sources(x, f.W, f.pw, sx);
        if (nt * ny * nx == 1) continue;
        const T* __restrict__ base = dXp + nc * (long)Tp * Hp * Wp;
        float acc = 0.f;
        for (int a = 0; a < nt; ++a)
            for (int b = 0; b < ny; ++b)
                for (int c = 0; c < nx; ++c)
                    if (a + b + c > 0) acc += c2m_ld(base, ((long)st[a] * Hp + sy[b]) * Wp + sx[c]);
        c2m_st(dX, idx, c2m_ld(dX, idx) + acc);
    }
}

// Border-only form (every extent >= 2*pad + 2, so the low and high mirror bands are disjoint): enumerates just the
// elements that have a mirrored source, as three disjoint ranges per (n,c) volume:
//   R1  x in band,                      all y, all t        T * H * 2pw
//   R2  x outside band, y in band,      all t               T * 2ph * (W - 2pw)
//   R3  x, y outside their bands,       t in band           2pt * (H - 2ph) * (W - 2pw)
// band(i) = [1, p] U [L-1-p, L-2]; the complement is {0} U [p+1, L-2-p] U {L-1}.
__device__ __forceinline__ int band_index(int j, int L, int p) { return j < p ? 1 + j : L - 1 - 2 * p + j; }
__device__ __forceinline__ int offband_index(int k, int L, int p) {
    return k == 0 ? 0 : (k == L - 2 * p - 1 ? L - 1 : k + p);
}

template <class T>
__global__ void reflect_border_only_kernel(const T* __restrict__ dXp, T* __restrict__ dX, const FoldP f,
                                           const int r1, const int r2, const int r3, const long NC) {
    const int Tp = f.T + 2 * f.pt, Hp = f.H + 2 * f.ph, Wp = f.W + 2 * f.pw;
    const int per = r1 + r2 + r3;
    const long total = NC * per;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long nc = idx / per;
        int e = (int)(idx - nc * per);
        int t, y, x;
        if (e < r1) {
            const int bw = 2 * f.pw;
            x = band_index(e % bw, f.W, f.pw); e /= bw;
            y = e % f.H; t = e / f.H;
        } else if (e < r1 + r2) {
            e -= r1;
            const int ow = f.W - 2 * f.pw, bh = 2 * f.ph;
            x = offband_index(e % ow, f.W, f.pw); e /= ow;
            y = band_index(e % bh, f.H, f.ph); t = e / bh;
        } else {
            e -= r1 + r2;
            const int ow = f.W - 2 * f.pw, oh = f.H - 2 * f.ph;
            x = offband_index(e % ow, f.W, f.pw); e /= ow;
            y = offband_index(e % oh, f.H, f.ph); t = band_index(e / oh, f.T, f.pt);
        }
        int st[3], sy[3], sx[3];
        const int nt = fold_sources(t, f.T, f.pt, st), ny = fold_sources(y, f.H, f.ph, sy),
                  nx = fold_sources(x, f.W, f.pw, sx);
        const T* __restrict__ base = dXp + nc * (long)Tp * Hp * Wp;
        float acc = 0.f;
        for (int a = 0; a < nt; ++a)
            for (int b = 0; b < ny; ++b)
                for (int c = 0; c < nx; ++c)
                    if (a + b + c > 0) acc += c2m_ld(base, ((long)st[a] * Hp + sy[b]) * Wp + sx[c]);
        const long di = (nc * f.T + t) * (long)f.H * f.W + (long)y * f.W + x;
        c2m_st(dX, di, c2m_ld(dX, di) + acc);
    }
}

// The 2-D pad-1 case (every 3x3 / 4x4-stride-2 reflect layer; a 3-D layer folded in the plane only is T independent planes): the
// elements that receive ring contributions are rows 1, H-2 and columns 1, W-2 of each plane.  The general kernel above finds its
// element with ~8 integer divisions by run-time values (20 us per launch on a 40 x 128 x 64 x 128 gradient: ALU bound, 55 launches
// per step); here one division splits (plane, e) and comparisons do the rest.  Same sources in the same order: bit-identical sums.
template <class T>
__global__ void reflect_border_p1_kernel(const T* __restrict__ dXp, T* __restrict__ dX, const int H, const int W, const long planes) {
    const int Hp = H + 2, Wp = W + 2;
    const int per = 2 * W + 2 * (H - 2);
    const long total = planes * per;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long pl = idx / per;
        const int e = (int)(idx - pl * per);
        int y, x;
        if (e < 2 * W) {                               // the two rows: contiguous in x
            y = e < W ? 1 : H - 2;
            x = e < W ? e : e - W;
        } else {                                       // the two columns without the rows above
            const int k2 = e - 2 * W;
            x = k2 < H - 2 ? 1 : W - 2;
            const int k = k2 < H - 2 ? k2 : k2 - (H - 2);
            y = k == 0 ? 0 : (k == H - 3 ? H - 1 : k + 1);
        }
        int sy[3], sx[3];
        const int ny = fold_sources(y, H, 1, sy), nx = fold_sources(x, W, 1, sx);
        const T* __restrict__ base = dXp + pl * (long)Hp * Wp;
        float acc = 0.f;
        for (int b = 0; b < ny; ++b)
            for (int c = 0; c < nx; ++c)
                if (b + c > 0) acc += c2m_ld(base, (long)sy[b] * Wp + sx[c]);
        const long di = pl * (long)H * W + (long)y * W + x;
        c2m_st(dX, di, c2m_ld(dX, di) + acc);
    }
}

C2M_API int c2m_reflect_border_add(const void* dXpad, void* dX, long NC, int T_, int H, int W, int pt, int ph, int pw,
                                   int dt, void* stream) {
    C2M_ENTER();
    FoldP f{T_, H, W, pt, ph, pw, NC * (long)T_ * H * W};
    if (f.total <= 0) return 0;
    const bool roomy = (pt == 0 || T_ >= 2 * pt + 2) && (ph == 0 || H >= 2 * ph + 2) && (pw == 0 || W >= 2 * pw + 2);
    const long per_l = (long)T_ * H * 2 * pw + (long)T_ * 2 * ph * (W - 2 * pw) + 2L * pt * (H - 2 * ph) * (W - 2 * pw);
    if (pt == 0 && ph == 1 && pw == 1 && H >= 4 && W >= 4 && !getenv("C2M_FOLD_GENERAL")) {
        const long planes = NC * T_;
        C2M_DISPATCH_DT(dt,
            hipLaunchKernelGGL(reflect_border_p1_kernel<T>, dim3(c2m_grid(planes * (2L * W + 2L * (H - 2)), 256)), dim3(256), 0,
                               (hipStream_t)stream, (const T*)dXpad, (T*)dX, H, W, planes););
        return (int)hipGetLastError();
    }
    C2M_DISPATCH_DT(dt,
        if (roomy && per_l > 0 && per_l < (1L << 30)) {
            const int r1 = T_ * H * 2 * pw; const int r2 = T_ * 2 * ph * (W - 2 * pw); const int r3 = 2 * pt * (H - 2 * ph) * (W - 2 * pw);
            hipLaunchKernelGGL(reflect_border_only_kernel<T>, dim3(c2m_grid(NC * per_l, 256)), dim3(256), 0,
                               (hipStream_t)stream, (const T*)dXpad, (T*)dX, f, r1, r2, r3, NC);
        } else {
            hipLaunchKernelGGL(reflect_border_add_kernel<T>, dim3(c2m_grid(f.total, 256)), dim3(256), 0, (hipStream_t)stream,
                               (const T*)dXpad, (T*)dX, f);
        });
    return (int)hipGetLastError();
}

C2M_API int c2m_reflect_fold(const void* dXpad, void* dX, long NC, int T_, int H, int W, int pt, int ph, int pw,
                             int dt, void* stream) {
    C2M_ENTER();
    FoldP f{T_, H, W, pt, ph, pw, NC * (long)T_ * H * W};
    if (f.total <= 0) return 0;
    if (dt == C2M_BF16 && (W & 3) == 0 && ((uintptr_t)dX & 7) == 0)
        hipLaunchKernelGGL(reflect_fold_vec_kernel<bf16_t>, dim3(c2m_grid(f.total / 4, 256)), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)dXpad, (bf16_t*)dX, f);
    else if (dt == C2M_BF16)
        hipLaunchKernelGGL(reflect_fold_kernel<bf16_t>, dim3(c2m_grid(f.total, 256)), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)dXpad, (bf16_t*)dX, f);
    else if ((W & 3) == 0 && ((uintptr_t)dX & 15) == 0)
        hipLaunchKernelGGL(reflect_fold_vec_kernel<float>, dim3(c2m_grid(f.total / 4, 256)), dim3(256), 0, (hipStream_t)stream,
                           (const float*)dXpad, (float*)dX, f);
    else
        hipLaunchKernelGGL(reflect_fold_kernel<float>, dim3(c2m_grid(f.total, 256)), dim3(256), 0, (hipStream_t)stream,
                           (const float*)dXpad, (float*)dX, f);
    return (int)hipGetLastError();
}
