// quality.hip -- per-frame PSNR / SSIM sums of predicted frames against the real ones, whole frame and per region bit.
// The reference has no counterpart (its evaluator reports FID / FVD, which need Inception / I3D weights: DESIGN 8).
//
// SSIM is Wang et al.'s as skimage.metrics.structural_similarity(gaussian_weights=True, use_sample_covariance=False,
// data_range=L) evaluates it: a separable 11-tap Gaussian (sigma 1.5, the eleven normalised float64 weights come from the
// caller), the moments ux, uy, E[x^2], E[y^2], E[xy] at every centre whose 11 x 11 window lies inside the frame, per channel
//     S = (2 ux uy + C1)(2 (E[xy] - ux uy) + C2) / ((ux^2 + uy^2 + C1)(E[x^2] - ux^2 + E[y^2] - uy^2 + C2)),
// C1 = (0.01 L)^2, C2 = (0.03 L)^2, then the mean over channels.  Everything from the moments on is fp64: C2 = 9e-4 divides the
// cancellation error of E[x^2] - ux^2, and fp32 moves a frame mean by up to 7e-5.  fp32, bf16 and uint8 inputs
// convert exactly; the uint8 form works on the integer levels with L = 255 and sums its squared error in integers.
//
// One workgroup (256 threads) owns a TH x TW = 16 x 32 tile of the PIXEL space of one frame, on a flat 1-D grid.  Per channel:
//   stage    x and y of the tile plus a 5-pixel halo, (TH + 10) x (TW + 10) = 26 x 42, in their own type (zero outside the frame;
//            the uint8 form stages all C interleaved channels once);
//   rows     the five horizontal 11-tap sums of every staged row at the TW tile columns -> LDS, fp64 [5][26][32];
//   columns  each thread owns two vertically adjacent centres of one column: twelve rows of the five sums from LDS, the eleven
//            weights applied twice, S for both.
// Then nine rows (whole frame, region bits 0..7) of (n_pixels, sse, n_windows, ssim_sum) go through the reduction of
// score_rows.h -- wave shuffles, the four waves in index order into partial[block][9][4], then score_reduce_kernel<16, 64>, one
// workgroup per frame.  No atomics: the result is bit-repeatable.
// LDS per workgroup: 33,280 (row sums) + 8,736 (staging; 6,552 for uint8 x 3) + 1,152 (reduction) = 43,168 bytes at most:
// three workgroups per CU.  The reduce kernel holds 16 x 64 x 8 = 8,192 bytes (36 of the 64 slots are used), one workgroup per
// frame: its occupancy is not limited by it.
#include <initializer_list>
#include "score_rows.h"

#define C2M_Q_TH 16
#define C2M_Q_TW 32
#define C2M_Q_R 5
#define C2M_Q_TAPS 11
#define C2M_Q_SR (C2M_Q_TH + 2 * C2M_Q_R)      // staged rows, 26
#define C2M_Q_SC (C2M_Q_TW + 2 * C2M_Q_R)      // staged columns, 42
#define C2M_Q_THREADS 256
#define C2M_Q_COLS 4                           // n_pixels, sse, n_windows, ssim_sum

struct QualityWeights { double w[C2M_Q_TAPS]; };

template <typename T> struct QIsU8 { static constexpr bool value = false; };
template <> struct QIsU8<uint8_t> { static constexpr bool value = true; };

// float forms: frame (b, t), channel c starts at b * sB + c * sC + t * sT, rows of W elements; uint8: b * sB + t * sT, rows of
// W * C interleaved bytes.  Strides are in elements.
template <typename T, int C>
__global__ __launch_bounds__(C2M_Q_THREADS) void frame_quality_kernel(
    const T* __restrict__ px, const T* __restrict__ py, const uint8_t* __restrict__ regions, int Tn, int H, int W, long sBx,
    long sCx, long sTx, long sBy, long sCy, long sTy, int tiles_x, int tiles_y, QualityWeights wt, double C1, double C2,
    double* __restrict__ partial) {
    constexpr bool U8 = QIsU8<T>::value;
    constexpr int CS = U8 ? C : 1;                                   // channels held by one staging
    __shared__ T stage[2][C2M_Q_SR * C2M_Q_SC * CS];
    __shared__ double mom[5][C2M_Q_SR * C2M_Q_TW];
    __shared__ double red[C2M_Q_THREADS / 64][C2M_SCORE_ROWS * C2M_Q_COLS];

    const int tid = threadIdx.x;
    const unsigned tiles = (unsigned)tiles_x * tiles_y;
    const unsigned frame = blockIdx.x / tiles, tile = blockIdx.x - frame * tiles;
    const int ty = (int)(tile / tiles_x), tx = (int)(tile - (unsigned)ty * tiles_x);
    const int b = (int)(frame / Tn), t = (int)(frame - (unsigned)b * Tn);
    const int y0 = ty * C2M_Q_TH, x0 = tx * C2M_Q_TW;

    const int col = tid & (C2M_Q_TW - 1), rp = tid >> 5;             // this thread's centres: rows 2 rp, 2 rp + 1 of column col
    const int gx = x0 + col, gy = y0 + 2 * rp;
    const bool in0 = gx < W && gy < H, in1 = gx < W && gy + 1 < H;
    const bool okx = gx >= C2M_Q_R && gx < W - C2M_Q_R;
    const bool ok0 = okx && gy >= C2M_Q_R && gy < H - C2M_Q_R, ok1 = okx && gy + 1 >= C2M_Q_R && gy + 1 < H - C2M_Q_R;

    double ssim0 = 0.0, ssim1 = 0.0, sse0 = 0.0, sse1 = 0.0;
    int isse0 = 0, isse1 = 0;                                        // uint8: at most 3 * 255^2 per pixel

    for (int c = 0; c < C; ++c) {
        __syncthreads();                                             // the last channel's reads of mom and stage are done
        if (!U8 || c == 0) {
            const T* __restrict__ fx = px + (b * sBx + (U8 ? 0 : c * sCx) + t * sTx);
            const T* __restrict__ fy = py + (b * sBy + (U8 ? 0 : c * sCy) + t * sTy);
            for (int i = tid; i < C2M_Q_SR * C2M_Q_SC; i += C2M_Q_THREADS) {
                const int r = i / C2M_Q_SC, q = i - r * C2M_Q_SC;
                const int yy = y0 - C2M_Q_R + r, xx = x0 - C2M_Q_R + q;
                const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
                const long o = ((long)yy * W + xx) * CS;
#pragma unroll
                for (int k = 0; k < CS; ++k) {
                    T vx = T(), vy = T();
                    if (in) {
                        vx = fx[o + k];
                        vy = fy[o + k];
                    }
                    stage[0][i * CS + k] = vx;
                    stage[1][i * CS + k] = vy;
                }
            }
            __syncthreads();
        }
        const int ch = U8 ? c : 0;

        // rows: the five 11-tap sums of staged row r at tile column q
        for (int i = tid; i < C2M_Q_SR * C2M_Q_TW; i += C2M_Q_THREADS) {
            const int r = i >> 5, q = i & (C2M_Q_TW - 1);
            const T* __restrict__ sx = &stage[0][(r * C2M_Q_SC + q) * CS + ch];
            const T* __restrict__ sy = &stage[1][(r * C2M_Q_SC + q) * CS + ch];
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
#pragma unroll
            for (int k = 0; k < C2M_Q_TAPS; ++k) {
                const double x = score_val(sx[k * CS]), y = score_val(sy[k * CS]), w = wt.w[k];
                a0 = fma(w, x, a0);
                a1 = fma(w, y, a1);
                a2 = fma(w, x * x, a2);
                a3 = fma(w, y * y, a3);
                a4 = fma(w, x * y, a4);
            }
            mom[0][i] = a0;
            mom[1][i] = a1;
            mom[2][i] = a2;
            mom[3][i] = a3;
            mom[4][i] = a4;
        }

        // squared error of this thread's two pixels (the staged centre is at +R, +R)
        {
            const int i0 = ((2 * rp + C2M_Q_R) * C2M_Q_SC + col + C2M_Q_R) * CS + ch, i1 = i0 + C2M_Q_SC * CS;
            if (U8) {
                const int d0 = (int)score_val(stage[0][i0]) - (int)score_val(stage[1][i0]);
                const int d1 = (int)score_val(stage[0][i1]) - (int)score_val(stage[1][i1]);
                isse0 += d0 * d0;
                isse1 += d1 * d1;
            } else {
                const double d0 = score_val(stage[0][i0]) - score_val(stage[1][i0]);       // exact
                const double d1 = score_val(stage[0][i1]) - score_val(stage[1][i1]);
                sse0 += d0 * d0;
                sse1 += d1 * d1;
            }
        }
        __syncthreads();

        // columns: staged rows 2 rp .. 2 rp + 11 serve the centres at tile rows 2 rp and 2 rp + 1
        double u[5], v[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) u[m] = v[m] = 0.0;
#pragma unroll
        for (int r = 0; r <= C2M_Q_TAPS; ++r) {
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                const double s = mom[m][(2 * rp + r) * C2M_Q_TW + col];
                if (r < C2M_Q_TAPS) u[m] = fma(wt.w[r], s, u[m]);
                if (r >= 1) v[m] = fma(wt.w[r - 1], s, v[m]);
            }
        }
        {
            const double vx = u[2] - u[0] * u[0], vy = u[3] - u[1] * u[1], vxy = u[4] - u[0] * u[1];
            const double s = ((2.0 * u[0] * u[1] + C1) * (2.0 * vxy + C2)) / ((u[0] * u[0] + u[1] * u[1] + C1) * (vx + vy + C2));
            ssim0 += ok0 ? s : 0.0;
        }
        {
            const double vx = v[2] - v[0] * v[0], vy = v[3] - v[1] * v[1], vxy = v[4] - v[0] * v[1];
            const double s = ((2.0 * v[0] * v[1] + C1) * (2.0 * vxy + C2)) / ((v[0] * v[0] + v[1] * v[1] + C1) * (vx + vy + C2));
            ssim1 += ok1 ? s : 0.0;
        }
    }
    if (U8) {
        sse0 = (double)isse0;
        sse1 = (double)isse1;
    }
    ssim0 /= (double)C;
    ssim1 /= (double)C;

    unsigned rg0 = 0, rg1 = 0;
    if (regions != nullptr) {
        const long o = ((long)frame * H + gy) * W + gx;
        if (in0) rg0 = regions[o];
        if (in1) rg1 = regions[o + W];
    }
    const int lane = tid & 63, wave = tid >> 6;
    const int nrows = regions != nullptr ? C2M_SCORE_ROWS : 1;
    for (int k = 0; k < nrows; ++k) {
        const bool m0 = in0 && C2M_SCORE_ROW_HAS(k, rg0), m1 = in1 && C2M_SCORE_ROW_HAS(k, rg1);
        int cnt = (int)m0 + (int)m1 + (((int)(m0 && ok0) + (int)(m1 && ok1)) << 16);      // pixels | windows << 16
        double e = (m0 ? sse0 : 0.0) + (m1 ? sse1 : 0.0);
        double s = (m0 ? ssim0 : 0.0) + (m1 ? ssim1 : 0.0);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);   // (wave_sum(cnt) gets the k loop peeled)
        e = wave_sum(e);
        s = wave_sum(s);
        if (lane == 0) {
            double* r = &red[wave][k * C2M_Q_COLS];
            r[0] = (double)(cnt & 0xffff);
            r[1] = e;
            r[2] = (double)(cnt >> 16);
            r[3] = s;
        }
    }
    __syncthreads();
    score_store_partial<C2M_Q_COLS>(red, nrows, partial);
}

static long q_tiles(int H, int W) { return (long)c2m_cdiv(H, C2M_Q_TH) * c2m_cdiv(W, C2M_Q_TW); }

C2M_API long c2m_frame_quality_workspace_bytes(int B, int T, int H, int W) {
    return score_workspace_bytes(B, T, H, W, q_tiles(H, W), C2M_Q_COLS);
}

template <typename T, int C>
static void q_launch(const void* pred, const void* target, const uint8_t* regions, int Tn, int H, int W, const long* sp,
                     const long* st, int tiles_x, int tiles_y, unsigned blocks, const QualityWeights& wt, double L,
                     double* partial, hipStream_t stream) {
    hipLaunchKernelGGL((frame_quality_kernel<T, C>), dim3(blocks), dim3(C2M_Q_THREADS), 0, stream, (const T*)pred,
                       (const T*)target, regions, Tn, H, W, sp[0], sp[1], sp[2], st[0], st[1], st[2], tiles_x, tiles_y, wt,
                       (0.01 * L) * (0.01 * L), (0.03 * L) * (0.03 * L), partial);
}

C2M_API int c2m_frame_quality(const void* pred, const void* target, const uint8_t* regions, int form, int B, int C, int T,
                              int H, int W, const long* pred_strides, const long* target_strides, const double* weights,
                              double L, void* workspace, long workspace_bytes, double* out, void* stream) {
    C2M_ENTER();
    if (B < 0 || T < 0 || (C != 1 && C != 3) || H < C2M_Q_TAPS || W < C2M_Q_TAPS || form < 0 || form > 2 || !(L > 0.0) ||
        pred_strides == nullptr || target_strides == nullptr || weights == nullptr)
        return (int)hipErrorInvalidValue;
    const long frames = (long)B * T;
    if (frames == 0) return 0;
    if (!score_sizes_ok(frames, (long)H * W * C, q_tiles(H, W))) return (int)hipErrorInvalidValue;
    const long blocks = frames * q_tiles(H, W);
    if (pred == nullptr || target == nullptr || out == nullptr || workspace == nullptr ||
        workspace_bytes < c2m_frame_quality_workspace_bytes(B, T, H, W))
        return (int)hipErrorInvalidValue;
    // a frame's elements must lie inside the strides the caller states: dense inner dims, non-overlapping frames
    const long plane = (long)H * W * (form == 2 ? C : 1);
    for (const long* s : {pred_strides, target_strides}) {
        if (form != 2 && C > 1 && s[1] < plane) return (int)hipErrorInvalidValue;
        if ((T > 1 && s[2] < plane) || (B > 1 && s[0] < plane)) return (int)hipErrorInvalidValue;
    }
    QualityWeights wt;
    for (int k = 0; k < C2M_Q_TAPS; ++k) wt.w[k] = weights[k];
    const int tiles_x = c2m_cdiv(W, C2M_Q_TW), tiles_y = c2m_cdiv(H, C2M_Q_TH);
    double* partial = (double*)workspace;
    hipStream_t s = (hipStream_t)stream;
#define C2M_Q_GO(TYPE)                                                                                                       \
    do {                                                                                                                     \
        if (C == 3) q_launch<TYPE, 3>(pred, target, regions, T, H, W, pred_strides, target_strides, tiles_x, tiles_y,       \
                                      (unsigned)blocks, wt, L, partial, s);                                                  \
        else q_launch<TYPE, 1>(pred, target, regions, T, H, W, pred_strides, target_strides, tiles_x, tiles_y,              \
                               (unsigned)blocks, wt, L, partial, s);                                                         \
    } while (0)
    if (form == 0) C2M_Q_GO(float);
    else if (form == 1) C2M_Q_GO(bf16_t);
    else C2M_Q_GO(uint8_t);
#undef C2M_Q_GO
    C2M_LAUNCH_CHECK();
    return score_reduce<16, 64, C2M_Q_COLS>(partial, frames, q_tiles(H, W), C2M_Q_COLS, out, s);
}
