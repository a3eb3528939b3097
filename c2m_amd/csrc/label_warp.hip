// Label propagation along a backward flow (gfx950): the nearest-neighbour counterpart of c2m_flow_warp_fwd.
//
//   c2m_label_warp   one launch carries the label planes of the last input frame (one-hot semantic channels as fp32 words,
//                    instance ids as int32 words) to all T predicted frames along flow [B,2,T,H,W].  Output pixel p of frame t
//                    reads the pixel nearest to the position the bilinear warp reads for p (warp_coord.h: the same warp_source
//                    and border clamp), rounded half-to-even like ATen's nearest grid_sample.  Labels are never blended.
//
// This file is compiled with -ffp-contract=off (see warp_coord.h).  The kernel only moves memory: 8 bytes of flow per output
// pixel, then Cf + Ci gathered words.  A thread owns VEC consecutive x of one (sample, frame, row): the source indices are
// computed once and reused for every plane, a wave writes 64 * VEC consecutive words of a row per plane (16-byte stores when
// VEC = 4), nothing is accumulated and there are no atomics.  Planes are copied as 32-bit words, so every bit pattern survives.
#include "common.h"
#include "warp_coord.h"

struct LabelWarpP {
    const float* flow; long sb, sc, st;          // element strides of sample, channel (x / y), frame; rows are dense
    const float* occ; float threshold; uint32_t fill_id;
    const uint32_t* src_f; uint32_t* out_f; int Cf;
    const uint32_t* src_i; uint32_t* out_i; int Ci;
    int B, T, H, W;
};

// out[b][c][t][y][x0..x0+VEC) = src[b][c][idx[0..VEC)] for every plane c; bit e of `fill` (integer planes, disoccluded pixels): fill_id instead
template <typename I, int VEC>
__device__ __forceinline__ void label_gather(const uint32_t* __restrict__ src, uint32_t* __restrict__ out, int C, int T, I HW,
                                             int b, int t, I sp, const unsigned (&idx)[VEC], unsigned fill,
                                             uint32_t fill_id) {
    const uint32_t* __restrict__ pl = src + (long)((I)b * C) * HW;
    uint32_t* __restrict__ o = out + (long)(((I)b * C * T + t) * HW + sp);
    const long ostep = (long)((I)T * HW);
#pragma unroll 4
    for (int c = 0; c < C; ++c, pl += (long)HW, o += ostep) {
        uint32_t v[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = pl[idx[e]];
        if (fill) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[e] = (fill >> e) & 1u ? fill_id : v[e];
        }
        if constexpr (VEC == 4) *reinterpret_cast<uint4*>(o) = make_uint4(v[0], v[1], v[2], v[3]);
        else o[0] = v[0];
    }
}

// I: 32-bit indices when every output has fewer than 2^31 elements.  VEC = 4 needs W % 4 == 0 and 16-byte aligned rows.
template <typename I, int VEC>
__global__ __launch_bounds__(256) void label_warp_kernel(const LabelWarpP p) {
    const int Wv = p.W / VEC;
    const I HW = (I)p.H * (I)p.W;
    const I items = (I)p.B * (I)p.T * (I)p.H * (I)Wv;
    for (I i = blockIdx.x * (I)blockDim.x + threadIdx.x; i < items; i += (I)gridDim.x * blockDim.x) {
        const int x0 = (int)(i % (I)Wv) * VEC; const I r = i / (I)Wv;
        const int y = (int)(r % (I)p.H); const I bt = r / (I)p.H;
        const int t = (int)(bt % (I)p.T); const int b = (int)(bt / (I)p.T);
        const I sp = (I)y * (I)p.W + (I)x0;
        const float* __restrict__ f = p.flow + ((long)b * p.sb + (long)t * p.st + (long)sp);
        float fx[VEC], fy[VEC], oc[VEC];
        if constexpr (VEC == 4) {
            const float4 a = *reinterpret_cast<const float4*>(f), c = *reinterpret_cast<const float4*>(f + p.sc);
            fx[0] = a.x; fx[1] = a.y; fx[2] = a.z; fx[3] = a.w;
            fy[0] = c.x; fy[1] = c.y; fy[2] = c.z; fy[3] = c.w;
            if (p.occ) {
                const float4 q = *reinterpret_cast<const float4*>(p.occ + (long)(((I)b * p.T + t) * HW + sp));
                oc[0] = q.x; oc[1] = q.y; oc[2] = q.z; oc[3] = q.w;
            }
        } else {
            fx[0] = f[0]; fy[0] = f[p.sc];
            if (p.occ) oc[0] = p.occ[(long)(((I)b * p.T + t) * HW + sp)];
        }
        unsigned idx[VEC];
        unsigned fill = 0u;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            float ix, iy;
            warp_source(fx[e], fy[e], x0 + e, y, p.H, p.W, ix, iy);
            // clamped to [0, n - 1] first (NaN -> 0), so the rounded index is in bounds for any flow
            const int sx = (int)rintf(warp_border(ix, p.W)), sy = (int)rintf(warp_border(iy, p.H));
            idx[e] = (unsigned)sy * (unsigned)p.W + (unsigned)sx;
            if (p.occ && oc[e] < p.threshold) fill |= 1u << e;
        }
        if (p.Cf > 0) label_gather<I, VEC>(p.src_f, p.out_f, p.Cf, p.T, HW, b, t, sp, idx, 0u, 0u);
        if (p.Ci > 0) label_gather<I, VEC>(p.src_i, p.out_i, p.Ci, p.T, HW, b, t, sp, idx, fill, p.fill_id);
    }
}


C2M_API int c2m_label_warp(const float* flow, long sb, long sc, long st, const float* occ, float threshold, int fill_id,
                           const float* planes_f, int Cf, const int32_t* planes_i, int Ci, int B, int T, int H, int W,
                           float* out_f, int32_t* out_i, void* stream) {
    C2M_ENTER();
    if (B < 0 || T < 0 || H < 0 || W < 0 || Cf < 0 || Ci < 0) return (int)hipErrorInvalidValue;
    const long HW = (long)H * W, px = (long)B * T * HW;
    if (px == 0 || Cf + Ci == 0) return 0;
    if (HW >= (1L << 31) || !flow || (Cf > 0 && (!planes_f || !out_f)) || (Ci > 0 && (!planes_i || !out_i)))
        return (int)hipErrorInvalidValue;
    const LabelWarpP p{flow, sb, sc, st, occ, threshold, (uint32_t)fill_id,
                       (const uint32_t*)planes_f, (uint32_t*)out_f, Cf, (const uint32_t*)planes_i, (uint32_t*)out_i, Ci,
                       B, T, H, W};
    const bool vec = W % 4 == 0 && sb % 4 == 0 && sc % 4 == 0 && st % 4 == 0 && c2m_aligned(16, flow, occ, out_f, out_i);
    // the largest tensor the kernel indexes with I is an output (the flow and occ offsets are 64-bit in either form)
    const bool small = px * (Cf > Ci ? Cf : Ci) < (1L << 31);
    const dim3 grid(c2m_grid(vec ? px / 4 : px, 256));
    hipStream_t s = (hipStream_t)stream;
    if (vec) {
        if (small) hipLaunchKernelGGL((label_warp_kernel<unsigned, 4>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((label_warp_kernel<long, 4>), grid, dim3(256), 0, s, p);
    } else {
        if (small) hipLaunchKernelGGL((label_warp_kernel<unsigned, 1>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((label_warp_kernel<long, 1>), grid, dim3(256), 0, s, p);
    }
    return (int)hipGetLastError();
}
