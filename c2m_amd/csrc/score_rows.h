// The region-row reduction shared by the score kernels (quality.hip, flow_score.hip).  A score is C2M_SCORE_ROWS rows -- row 0
// everything scored, row 1 + k what lies where bit k of the region byte is set -- of COLS float64 sums per frame (or pair), added
// in one fixed order, so bit-repeatable without atomics:
//   1. a 256-thread kernel masks its terms by C2M_SCORE_ROW_HAS(k, region byte) for each row k, adds them over the wave
//      (wave_sum) and lane 0 writes red[wave][k * COLS + col].  That loop stays with the kernel: which terms are masked and how
//      counts are packed into one int before the shuffle differ;
//   2. after a barrier, score_store_partial adds the four waves in index order into partial[block][9][COLS];
//   3. score_reduce_kernel, one workgroup per frame: slice s of SLICES adds the tiles s, s + SLICES, ... in order, then the slices
//      are added in index order.  SLICES and SLOTS ARE the summation order: frame quality runs <16, 64>, the flow scores <8, 128>
//      (8,192 bytes of LDS either way, 34 VGPRs).
#pragma once
#include "common.h"
#include "dtype.h"

#define C2M_SCORE_ROWS 9                               // everything scored + 8 region bits

// Exact conversions of the scored element types (bf16 -> fp32 -> fp64 loses nothing).
__device__ __forceinline__ double score_val(float v) { return (double)v; }
__device__ __forceinline__ double score_val(bf16_t v) { return (double)(float)v; }
__device__ __forceinline__ double score_val(uint8_t v) { return (double)(int)v; }

// Does row k (0..8) count a pixel with region byte rg (unsigned)?  A macro on purpose: as an inlined function the same expression
// gets the k = 0 iteration of frame_quality_kernel's row loop peeled (+88 instructions; wave_sum(cnt) there does the same).
#define C2M_SCORE_ROW_HAS(k, rg) ((k) == 0 || (((rg) >> ((k) - 1)) & 1u))

// Step 2; rows the caller did not fill (nrows .. 8) are written as zeros.  The caller's barrier stands before this call.
template <int COLS>
__device__ __forceinline__ void score_store_partial(double (*red)[C2M_SCORE_ROWS * COLS], int nrows,
                                                    double* __restrict__ partial) {
    const int tid = threadIdx.x;
    if (tid < C2M_SCORE_ROWS * COLS) {
        double a = 0.0;
        if (tid < nrows * COLS) a = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        partial[(long)blockIdx.x * (C2M_SCORE_ROWS * COLS) + tid] = a;
    }
}

// Step 3: value v = tid % SLOTS (< vals = 9 * cols <= SLOTS), slice s = tid / SLOTS.  Columns nan_from .. cols - 1 are written
// as NaN (nan_from = cols: none).
template <int SLICES, int SLOTS>
__global__ __launch_bounds__(SLICES * SLOTS) void score_reduce_kernel(const double* __restrict__ partial, int tiles, int vals,
                                                                      int cols, int nan_from, double* __restrict__ out) {
    __shared__ double acc[SLICES][SLOTS];
    const int v = threadIdx.x & (SLOTS - 1), s = threadIdx.x / SLOTS;
    const double* __restrict__ p = partial + (long)blockIdx.x * tiles * vals;
    if (v < vals) {
        double a = 0.0;
#pragma unroll 4
        for (int i = s; i < tiles; i += SLICES) a += p[(long)i * vals + v];
        acc[s][v] = a;
    }
    __syncthreads();
    if ((int)threadIdx.x < vals) {
        double a = 0.0;
        for (int i = 0; i < SLICES; ++i) a += acc[i][threadIdx.x];
        if ((int)threadIdx.x % cols >= nan_from) a = __builtin_nan("");
        out[(long)blockIdx.x * vals + threadIdx.x] = a;
    }
}

// The host side the launchers share.  Bytes of partial[frames * tiles][9][cols]; -1 for sizes no launcher takes.
static inline long score_workspace_bytes(int B, int T, int H, int W, long tiles, int cols) {
    if (B < 0 || T < 0 || H < 1 || W < 1) return -1;
    return (long)B * T * tiles * C2M_SCORE_ROWS * cols * (long)sizeof(double);
}

// The kernels index the frames, the elements of one frame and the workgroups of the grid in 32 bits.
static inline bool score_sizes_ok(long frames, long plane, long tiles) {
    return frames <= 0x7fffffffL && plane <= 0x7fffffffL && frames * tiles <= 0x7fffffffL;
}

template <int SLICES, int SLOTS, int COLS>
static inline int score_reduce(const double* partial, long frames, long tiles, int nan_from, double* out, hipStream_t s) {
    static_assert(C2M_SCORE_ROWS * COLS <= SLOTS && (SLOTS & (SLOTS - 1)) == 0, "a slot per value, v = tid & (SLOTS - 1)");
    hipLaunchKernelGGL((score_reduce_kernel<SLICES, SLOTS>), dim3((unsigned)frames), dim3(SLICES * SLOTS), 0, s, partial,
                       (int)tiles, C2M_SCORE_ROWS * COLS, COLS, nan_from, out);
    return (int)hipGetLastError();
}
