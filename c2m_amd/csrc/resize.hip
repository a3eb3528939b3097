// resize.hip -- dataset resolution -> train_params.input_size on the device: the last host step of the input pipeline.
// Reference (CPU, per file): src/datasets/cityscapes.py
//   :23,33        frames            Image.resize(BICUBIC)                      -> c2m_resize_u8      (bit-equal to Pillow)
//   :26-33,211    label / instance / occlusion maps   Image.resize(NEAREST)    -> c2m_resize_nearest (bit-equal to Pillow)
//   :220-222      .flo fields       transforms.Resize(tensor) * size[0] / h    -> c2m_resize_flow
//
// Pillow's 8-bit resampler (src/libImaging/Resample.c) is integer arithmetic: per axis a table of (first, count) source bounds
// and coefficients quantised to 22 bits (precompute_coeffs + normalize_coeffs_8bpc); a pass computes
// clip8((2^21 + sum p * k) >> 22) in int32; the horizontal pass runs first and its result is ROUNDED TO uint8 before the vertical
// pass reads it.  The tables are built by the caller (c2m_amd/ops.py, float64) and arrive twice: on the host, where the entry
// point checks them and sizes the tile, and on the device, where the kernel reads them.
//
// One kernel does both passes.  A workgroup owns a TH x TW output tile.  The source rows its vertical taps reach are streamed
// through LDS R rows at a time (the byte range its horizontal taps reach, fetched as aligned dwords); the horizontal pass turns
// each staged row into TW x C uint8 values of the intermediate image, which stays in LDS; the vertical pass reads that.
// At 8x reduction a tap window is 33 wide, so a 16 x 32 tile reads 161 x 289 source pixels for 128 x 256 it owns (1.42x), and
// holds 15 KB of intermediate + 14 KB of staged rows + 6 KB of coefficients: four workgroups per CU.
#include "common.h"

#define C2M_RS_THREADS 256
#define C2M_RS_LDS_BUDGET (40 * 1024)
#define C2M_RS_STAGE_ROWS 32

__device__ __forceinline__ uint8_t rs_clip8(int v) {          // Pillow's clip8: the lookup table clamps (v >> 22) to [0, 255]
    v >>= 22;
    return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// srcw: the source as dwords, from the 4-byte boundary at or below its first byte; the image bytes are [lo, hi) of it.
template <int C>
__global__ __launch_bounds__(C2M_RS_THREADS) void resize_u8_kernel(
    const uint32_t* __restrict__ srcw, long lo, long hi, uint8_t* __restrict__ dst, int Hin, int Win, int Hout, int Wout,
    const int* __restrict__ bx, const int* __restrict__ kx, int ksx, const int* __restrict__ by, const int* __restrict__ ky,
    int ksy, int TH, int TW, int tiles_x, int tiles_y, int midrows, int stride, int R) {
    extern __shared__ uint32_t rs_lds[];
    int* __restrict__ ckx = (int*)rs_lds;
    int* __restrict__ cky = ckx + TW * ksx;
    uint8_t* __restrict__ mid = (uint8_t*)(cky + TH * ksy);
    const int midpitch = TW * C;
    uint8_t* __restrict__ stage = mid + ((midrows * midpitch + 3) & ~3);
    uint32_t* __restrict__ stage_w = (uint32_t*)stage;

    const int tid = threadIdx.x;
    const unsigned tile = blockIdx.x;
    const int tx = (int)(tile % tiles_x);
    const unsigned tr = tile / tiles_x;
    const int ty = (int)(tr % tiles_y);
    const long n = tr / tiles_y;
    const int x0 = tx * TW, nx = min(TW, Wout - x0);
    const int y0 = ty * TH, ny = min(TH, Hout - y0);

    for (int i = tid; i < nx * ksx; i += C2M_RS_THREADS) ckx[i] = kx[(long)x0 * ksx + i];
    for (int i = tid; i < ny * ksy; i += C2M_RS_THREADS) cky[i] = ky[(long)y0 * ksy + i];

    // bounds are non-decreasing along an axis (checked on the host): the tile's reach is set by its first and last output
    const int colbase = bx[2 * x0], colend = bx[2 * (x0 + nx - 1)] + bx[2 * (x0 + nx - 1) + 1];
    const int rowbase = by[2 * y0], rowend = by[2 * (y0 + ny - 1)] + by[2 * (y0 + ny - 1) + 1];
    const int nrows = min(rowend - rowbase, midrows);
    const int nbytes = min((colend - colbase) * C, stride - 3);
    const int dpr = stride >> 2;

    for (int rc = 0; rc < nrows; rc += R) {
        const int rn = min(R, nrows - rc);
        for (int i = tid; i < rn * dpr; i += C2M_RS_THREADS) {
            const int r = i / dpr, d = i - r * dpr;
            const long b = lo + (((n * Hin + rowbase + rc + r) * (long)Win) + colbase) * C;     // first byte this row needs
            const int sh = (int)(b & 3);
            if (d * 4 < sh + nbytes) {
                const long w = (b >> 2) + d, a = w * 4;
                uint32_t v;
                if (a >= lo && a + 4 <= hi) {
                    v = srcw[w];
                } else {                                           // the dword hangs over an end of the image: bytes
                    v = 0;
                    const uint8_t* __restrict__ sb = (const uint8_t*)srcw;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (a + k >= lo && a + k < hi) v |= (uint32_t)sb[a + k] << (8 * k);
                }
                stage_w[r * dpr + d] = v;
            }
        }
        __syncthreads();                                           // staged rows (and, the first time, the coefficients)
        for (int i = tid; i < rn * nx; i += C2M_RS_THREADS) {
            const int r = i / nx, xl = i - r * nx;
            const long b = lo + (((n * Hin + rowbase + rc + r) * (long)Win) + colbase) * C;
            const int first = bx[2 * (x0 + xl)] - colbase, cnt = bx[2 * (x0 + xl) + 1];
            const uint8_t* __restrict__ p = stage + r * stride + (int)(b & 3) + first * C;
            const int* __restrict__ k = ckx + xl * ksx;
            int s[C];
#pragma unroll
            for (int c = 0; c < C; ++c) s[c] = 1 << 21;
            for (int t = 0; t < cnt; ++t) {
                const int kk = k[t];
#pragma unroll
                for (int c = 0; c < C; ++c) s[c] += (int)p[t * C + c] * kk;
            }
            uint8_t* __restrict__ m = mid + (rc + r) * midpitch + xl * C;
#pragma unroll
            for (int c = 0; c < C; ++c) m[c] = rs_clip8(s[c]);
        }
        __syncthreads();                                           // the staging rows are rewritten by the next chunk
    }

    const int rowlen = nx * C;
    for (int i = tid; i < ny * rowlen; i += C2M_RS_THREADS) {
        const int yl = i / rowlen, j = i - yl * rowlen;
        const int first = by[2 * (y0 + yl)] - rowbase, cnt = by[2 * (y0 + yl) + 1];
        const uint8_t* __restrict__ m = mid + first * midpitch + j;
        const int* __restrict__ k = cky + yl * ksy;
        int s = 1 << 21;
        for (int t = 0; t < cnt; ++t) s += (int)m[t * midpitch] * k[t];
        dst[((n * Hout + y0 + yl) * (long)Wout + x0) * C + j] = rs_clip8(s);
    }
}

// (first, count) per output, count in [1, ks], inside [0, in), both ends non-decreasing.
static bool rs_bounds_ok(const int32_t* b, int out, int in, int ks) {
    int pf = 0, pe = 0;
    for (int i = 0; i < out; ++i) {
        const int f = b[2 * i], c = b[2 * i + 1];
        if (f < 0 || c < 1 || c > ks || f > in - c || f < pf || f + c < pe) return false;
        pf = f;
        pe = f + c;
    }
    return true;
}

// widest source reach of a tile of `tile` outputs
static int rs_span(const int32_t* b, int out, int tile) {
    int span = 0;
    for (int i0 = 0; i0 < out; i0 += tile) {
        const int i1 = (i0 + tile < out ? i0 + tile : out) - 1;
        const int s = b[2 * i1] + b[2 * i1 + 1] - b[2 * i0];
        if (s > span) span = s;
    }
    return span;
}

C2M_API int c2m_resize_u8(const uint8_t* src, uint8_t* dst, int N, int Hin, int Win, int Hout, int Wout, int C,
                          const int32_t* bounds_x_host, const int32_t* bounds_x, const int32_t* coef_x, int ksx,
                          const int32_t* bounds_y_host, const int32_t* bounds_y, const int32_t* coef_y, int ksy, void* stream) {
    C2M_ENTER();
    if (N < 0 || Hin < 1 || Win < 1 || Hout < 1 || Wout < 1 || (C != 1 && C != 3) || ksx < 1 || ksy < 1)
        return (int)hipErrorInvalidValue;
    if (!rs_bounds_ok(bounds_x_host, Wout, Win, ksx) || !rs_bounds_ok(bounds_y_host, Hout, Hin, ksy))
        return (int)hipErrorInvalidValue;
    if (N == 0) return 0;
    int TH = 16, TW = 32, midrows = 0, stride = 0, R = 0;
    long bytes = 0;
    for (;;) {                                                     // the largest tile whose LDS fits the budget
        midrows = rs_span(bounds_y_host, Hout, TH);
        stride = (rs_span(bounds_x_host, Wout, TW) * C + 3 + 3) & ~3;          // + 3: a row may start 3 bytes into a dword
        const long fixed = 4L * (TW * (long)ksx + TH * (long)ksy) + (((long)midrows * TW * C + 3) & ~3L);
        R = (int)((C2M_RS_LDS_BUDGET - fixed) / stride);
        if (R > C2M_RS_STAGE_ROWS) R = C2M_RS_STAGE_ROWS;
        if (R > midrows) R = midrows;
        bytes = fixed + (long)R * stride;
        if (R >= 1 && (R >= 8 || R == midrows || (TH == 1 && TW == 1))) break;
        if (TH > 1 && 2 * TH >= TW) TH /= 2;
        else if (TW > 1) TW /= 2;
        else if (TH > 1) TH /= 2;
        else return (int)hipErrorInvalidValue;                     // one output's taps do not fit: reduction beyond ~3000x
    }
    const int tiles_x = c2m_cdiv(Wout, TW), tiles_y = c2m_cdiv(Hout, TH);
    const long tiles = (long)tiles_x * tiles_y * N;
    if (tiles > 0x7fffffffL) return (int)hipErrorInvalidValue;
    const long mis = (long)((uintptr_t)src & 3);
    const uint32_t* srcw = (const uint32_t*)(src - mis);
    const long total = (long)N * Hin * Win * C;
    if (C == 3)
        hipLaunchKernelGGL(resize_u8_kernel<3>, dim3((unsigned)tiles), dim3(C2M_RS_THREADS), (size_t)bytes, (hipStream_t)stream,
                           srcw, mis, mis + total, dst, Hin, Win, Hout, Wout, bounds_x, coef_x, ksx, bounds_y, coef_y, ksy, TH,
                           TW, tiles_x, tiles_y, midrows, stride, R);
    else
        hipLaunchKernelGGL(resize_u8_kernel<1>, dim3((unsigned)tiles), dim3(C2M_RS_THREADS), (size_t)bytes, (hipStream_t)stream,
                           srcw, mis, mis + total, dst, Hin, Win, Hout, Wout, bounds_x, coef_x, ksx, bounds_y, coef_y, ksy, TH,
                           TW, tiles_x, tiles_y, midrows, stride, R);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------ NEAREST
// Pillow's ImagingScaleAffine: one source index per output column and per output row (the caller's running double sum);
// -1 marks an output whose source falls outside the image, which Pillow leaves zero.
template <typename T>
__global__ void resize_nearest_kernel(const T* __restrict__ src, T* __restrict__ dst, long total, int Hin, int Win, int Hout,
                                      int Wout, const int* __restrict__ xi, const int* __restrict__ yi) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wout);
        const long r = i / Wout;
        const int y = (int)(r % Hout);
        const long n = r / Hout;
        const int sx = xi[x], sy = yi[y];
        dst[i] = (sx < 0 || sy < 0) ? (T)0 : src[(n * Hin + sy) * (long)Win + sx];
    }
}

static bool rs_index_ok(const int32_t* t, int out, int in) {
    for (int i = 0; i < out; ++i)
        if (t[i] < -1 || t[i] >= in) return false;
    return true;
}

C2M_API int c2m_resize_nearest(const void* src, void* dst, int elem_bytes, long N, int Hin, int Win, int Hout, int Wout,
                               const int32_t* index_x_host, const int32_t* index_x, const int32_t* index_y_host,
                               const int32_t* index_y, void* stream) {
    C2M_ENTER();
    if (N < 0 || Hin < 1 || Win < 1 || Hout < 1 || Wout < 1 || (elem_bytes != 1 && elem_bytes != 4))
        return (int)hipErrorInvalidValue;
    if (!rs_index_ok(index_x_host, Wout, Win) || !rs_index_ok(index_y_host, Hout, Hin)) return (int)hipErrorInvalidValue;
    const long total = N * Hout * Wout;
    if (total <= 0) return 0;
    if (elem_bytes == 1)
        hipLaunchKernelGGL(resize_nearest_kernel<uint8_t>, dim3(c2m_grid(total, 256)), dim3(256), 0, (hipStream_t)stream,
                           (const uint8_t*)src, (uint8_t*)dst, total, Hin, Win, Hout, Wout, index_x, index_y);
    else
        hipLaunchKernelGGL(resize_nearest_kernel<uint32_t>, dim3(c2m_grid(total, 256)), dim3(256), 0, (hipStream_t)stream,
                           (const uint32_t*)src, (uint32_t*)dst, total, Hin, Win, Hout, Wout, index_x, index_y);
    return (int)hipGetLastError();
}

// --------------------------------------------------------------------------------------------------------------- flows
// Separable triangle filter on [N][H][W][2] fp32 with per-axis (first, count) bounds and fp32 weights (float64 on the host, then
// cast).  fp32 accumulation in a fixed order: per source row the horizontal dot product left to right, then the vertical one top
// to bottom; then (v * num) / den, the reference's `* size[0] / h` on BOTH channels, as two fp32 operations.
__global__ void resize_flow_kernel(const float* __restrict__ src, float* __restrict__ dst, long total, int Hin, int Win,
                                   int Hout, int Wout, const int* __restrict__ bx, const float* __restrict__ wx, int ksx,
                                   const int* __restrict__ by, const float* __restrict__ wy, int ksy, float num, float den) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wout);
        const long r = i / Wout;
        const int y = (int)(r % Hout);
        const long n = r / Hout;
        const int fx = bx[2 * x], cx = bx[2 * x + 1], fy = by[2 * y], cy = by[2 * y + 1];
        const float* __restrict__ kx = wx + (long)x * ksx;
        const float* __restrict__ kyp = wy + (long)y * ksy;
        float au = 0.f, av = 0.f;
        for (int ty = 0; ty < cy; ++ty) {
            const float* __restrict__ row = src + ((n * Hin + fy + ty) * (long)Win + fx) * 2;
            float ru = 0.f, rv = 0.f;
            for (int t = 0; t < cx; ++t) {
                const float w = kx[t];
                ru += w * row[2 * t];
                rv += w * row[2 * t + 1];
            }
            au += kyp[ty] * ru;
            av += kyp[ty] * rv;
        }
        dst[2 * i] = au * num / den;
        dst[2 * i + 1] = av * num / den;
    }
}

C2M_API int c2m_resize_flow(const float* src, float* dst, long N, int Hin, int Win, int Hout, int Wout,
                            const int32_t* bounds_x_host, const int32_t* bounds_x, const float* weight_x, int ksx,
                            const int32_t* bounds_y_host, const int32_t* bounds_y, const float* weight_y, int ksy,
                            void* stream) {
    C2M_ENTER();
    if (N < 0 || Hin < 1 || Win < 1 || Hout < 1 || Wout < 1 || ksx < 1 || ksy < 1) return (int)hipErrorInvalidValue;
    if (!rs_bounds_ok(bounds_x_host, Wout, Win, ksx) || !rs_bounds_ok(bounds_y_host, Hout, Hin, ksy))
        return (int)hipErrorInvalidValue;
    const long total = N * Hout * Wout;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(resize_flow_kernel, dim3(c2m_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, total, Hin,
                       Win, Hout, Wout, bounds_x, weight_x, ksx, bounds_y, weight_y, ksy, (float)Hout, (float)Hin);
    return (int)hipGetLastError();
}
