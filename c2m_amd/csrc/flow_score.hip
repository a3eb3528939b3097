// flow_score.hip -- scores of optical flows, per pair and per region bit: the error of a flow against another one
// (c2m_flow_quality: endpoint error, angular error, KITTI's Fl, bad-pixel counts) and the ground-truth-free consistency of a flow
// with the two frames and with the flow of the reverse pair (c2m_flow_consistency: photometric error of the warp, forward-backward
// distance, UnFlow's occlusion test).  The reference has no counterpart.  DESIGN.md 4.2r; tests/flow_score_np.py restates it.
//
// Flows are in pixels, channel 0 = x: a(x) ~ b(x + flow(x)).  Every input is converted exactly (fp32 / bf16 -> fp64) and ALL
// per-pixel arithmetic is fp64, one rounding per written operation (the file is built with -ffp-contract=off); every threshold
// is decided on squared quantities, so every count is a function of + and x alone.
//
// c2m_flow_quality, per pixel, (pu, pv) the scored flow and (tu, tv) the target:
//     scored    = (valid == NULL || valid != 0) && tu, tv finite && |tu| < 1e9 && |tv| < 1e9
//     nonfinite = scored && !(pu, pv finite)
//     du = pu - tu, dv = pv - tv, e2 = du*du + dv*dv, m2 = tu*tu + tv*tv
//     ae = acos(min(max(c, -1), 1)),  c = ((1 + pu*tu) + pv*tv) / sqrt(((1 + pu*pu) + pv*pv) * (1 + m2))
//     out = e2 > 9 && e2 > 0.0025 * m2;  gt1, gt3, gt5 = e2 > 1, 9, 25
//   columns (n, n_nonfinite, sum sqrt(e2), sum e2, sum sqrt(m2), sum ae, n_out, n_gt1, n_gt3, n_gt5).  A nonfinite pixel adds
//   nothing to the four sums and counts in n, n_nonfinite and ALL FOUR threshold counts: it never poisons a sum and never
//   passes as correct.
//
// c2m_flow_consistency, per pixel x = (px, py) of a, f = flow_ab(x):
//     yx = px + fu, yy = py + fv;  inside = fu, fv finite && 0 <= yx <= W - 1 && 0 <= yy <= H - 1
//   for inside pixels, the bilinear sample S(img) at (yx, yy) in the corner and association order of flow_sample.h:
//     x0 = floor(yx), x1 = min(x0 + 1, W - 1), ax = yx - x0 (rows alike);
//     top = img[y0][x0]*(1 - ax) + img[y0][x1]*ax;  bot = img[y1][x0]*(1 - ax) + img[y1][x1]*ax;  S = top*(1 - ay) + bot*ay
//     p   = (|a_0 - S(b_0)| + |a_1 - S(b_1)| + |a_2 - S(b_2)|) / C                      (added in channel order, from 0)
//     g   = (S(ba_u), S(ba_v));  su = fu + gu, sv = fv + gv;  fb2 = su*su + sv*sv
//     inconsistent = !(fb2 <= alpha1 * ((fu*fu + fv*fv) + (gu*gu + gv*gv)) + alpha2)     (so a NaN in flow_ba is inconsistent)
//   columns (n, n_inside, sum p, sum p*p, sum sqrt(fb2) [finite fb2 only], n_inconsistent, sum p [inside, consistent]).  The
//   last three are NaN when flow_ba is NULL.  Images are taken as finite: a NaN there shows in the photometric sums.
//   Optional maps, written by the same launch: photo, fb fp32 (NaN outside), inconsistent uint8.
//
// Launches: one workgroup (256 threads) owns a tile of 1024 consecutive pixels of one pair, four per thread at a stride of 256
// (coalesced rows; the gathers of the consistency kernel follow the flow from there).  A thread keeps its four pixels' terms
// in registers; then, for the whole pair and for each region bit, the terms are added in a fixed order -- the thread's four in
// index order, then the reduction of score_rows.h: wave shuffles, the four waves in index order into partial[block][9][K] and
// score_reduce_kernel<8, 128>, one workgroup per pair.  No atomics, nothing read back, bit-repeatable; a pair's sums do not
// depend on the batch it is in.
// LDS per workgroup: 4 x 90 x 8 = 2,880 bytes (quality), 4 x 63 x 8 = 2,016 (consistency), 8 x 128 x 8 = 8,192 (reduce); no
// scratch, at most 87 VGPRs: occupancy is not limited by either.
#include "score_rows.h"

#define C2M_FS_THREADS 256
#define C2M_FS_PPT 4                                        // pixels per thread
#define C2M_FS_TILE (C2M_FS_THREADS * C2M_FS_PPT)           // 1024 pixels
#define C2M_FQ_COLS 10
#define C2M_FC_COLS 7

__device__ __forceinline__ bool fs_finite(double v) { return fabs(v) < __builtin_huge_val(); }       // false for NaN

// pair (b, t) = frame / Tn, frame % Tn; channel c of it starts at b * sB + c * sC + t * sT, HW dense elements.
template <typename PT>
__global__ __launch_bounds__(C2M_FS_THREADS) void flow_quality_kernel(
    const PT* __restrict__ pred, const float* __restrict__ target, const uint8_t* __restrict__ valid,
    const uint8_t* __restrict__ regions, int Tn, int HW, long sBp, long sCp, long sTp, long sBt, long sCt, long sTt,
    unsigned tiles, double* __restrict__ partial) {
    __shared__ double red[C2M_FS_THREADS / 64][C2M_SCORE_ROWS * C2M_FQ_COLS];
    const int tid = threadIdx.x;
    const unsigned frame = blockIdx.x / tiles, tile = blockIdx.x - frame * tiles;
    const int b = (int)(frame / (unsigned)Tn), t = (int)(frame - (unsigned)b * Tn);
    const PT* __restrict__ pu_ = pred + (b * sBp + t * sTp);
    const PT* __restrict__ pv_ = pu_ + sCp;
    const float* __restrict__ tu_ = target + (b * sBt + t * sTt);
    const float* __restrict__ tv_ = tu_ + sCt;
    const long mask0 = (long)frame * HW;

    double epe[C2M_FS_PPT], e2s[C2M_FS_PPT], mag[C2M_FS_PPT], ang[C2M_FS_PPT];
    unsigned flag[C2M_FS_PPT];          // 1 scored, 2 nonfinite, 4 out, 8 gt1, 16 gt3, 32 gt5; the region byte << 8
#pragma unroll
    for (int j = 0; j < C2M_FS_PPT; ++j) {
        const long i = (long)tile * C2M_FS_TILE + j * C2M_FS_THREADS + tid;
        epe[j] = e2s[j] = mag[j] = ang[j] = 0.0;
        flag[j] = 0u;
        if (i < HW) {
            const double tu = (double)tu_[i], tv = (double)tv_[i];
            bool scored = fs_finite(tu) && fs_finite(tv) && fabs(tu) < 1e9 && fabs(tv) < 1e9;
            if (valid != nullptr) scored = scored && valid[mask0 + i] != 0;
            if (scored) {
                const double pu = score_val(pu_[i]), pv = score_val(pv_[i]);
                unsigned f = 1u;
                if (fs_finite(pu) && fs_finite(pv)) {
                    const double du = pu - tu, dv = pv - tv;
                    const double e2 = du * du + dv * dv, m2 = tu * tu + tv * tv;
                    const double c = ((1.0 + pu * tu) + pv * tv) / sqrt(((1.0 + pu * pu) + pv * pv) * (1.0 + m2));
                    epe[j] = sqrt(e2);
                    e2s[j] = e2;
                    mag[j] = sqrt(m2);
                    ang[j] = acos(fmin(fmax(c, -1.0), 1.0));
                    f |= (e2 > 9.0 && e2 > 0.0025 * m2 ? 4u : 0u) | (e2 > 1.0 ? 8u : 0u) | (e2 > 9.0 ? 16u : 0u) |
                         (e2 > 25.0 ? 32u : 0u);
                } else {
                    f |= 2u | 4u | 8u | 16u | 32u;
                }
                if (regions != nullptr) f |= (unsigned)regions[mask0 + i] << 8;
                flag[j] = f;
            }
        }
    }

    const int lane = tid & 63, wave = tid >> 6;
    const int nrows = regions != nullptr ? C2M_SCORE_ROWS : 1;
    for (int k = 0; k < nrows; ++k) {
        int c0 = 0, c1 = 0;                                 // three 10-bit counts each: a wave holds at most 256 pixels
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
        for (int j = 0; j < C2M_FS_PPT; ++j) {
            const unsigned f = flag[j];
            const bool m = (f & 1u) && C2M_SCORE_ROW_HAS(k, f >> 8);
            if (m) {
                c0 += 1 + (int)((f >> 1) & 1u) * (1 << 10) + (int)((f >> 2) & 1u) * (1 << 20);
                c1 += (int)((f >> 3) & 1u) + (int)((f >> 4) & 1u) * (1 << 10) + (int)((f >> 5) & 1u) * (1 << 20);
            }
            s0 += m ? epe[j] : 0.0;
            s1 += m ? e2s[j] : 0.0;
            s2 += m ? mag[j] : 0.0;
            s3 += m ? ang[j] : 0.0;
        }
        c0 = wave_sum(c0);
        c1 = wave_sum(c1);
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        s3 = wave_sum(s3);
        if (lane == 0) {
            double* r = &red[wave][k * C2M_FQ_COLS];
            r[0] = (double)(c0 & 1023);
            r[1] = (double)((c0 >> 10) & 1023);
            r[2] = s0;
            r[3] = s1;
            r[4] = s2;
            r[5] = s3;
            r[6] = (double)((c0 >> 20) & 1023);
            r[7] = (double)(c1 & 1023);
            r[8] = (double)((c1 >> 10) & 1023);
            r[9] = (double)((c1 >> 20) & 1023);
        }
    }
    __syncthreads();
    score_store_partial<C2M_FQ_COLS>(red, nrows, partial);
}

// The four corners and the two weights of the bilinear sample at (yx, yy), 0 <= yx <= W - 1 and 0 <= yy <= H - 1.
struct FsTap { int o00, o01, o10, o11; double ax, ay; };

__device__ __forceinline__ FsTap fs_tap(double yx, double yy, int H, int W) {
    const double x0f = floor(yx), y0f = floor(yy);
    const int x0 = (int)x0f, y0 = (int)y0f, x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    FsTap t;
    t.o00 = y0 * W + x0;
    t.o01 = y0 * W + x1;
    t.o10 = y1 * W + x0;
    t.o11 = y1 * W + x1;
    t.ax = yx - x0f;
    t.ay = yy - y0f;
    return t;
}

template <typename T>
__device__ __forceinline__ double fs_sample(const T* __restrict__ img, const FsTap& t) {
    const double top = score_val(img[t.o00]) * (1.0 - t.ax) + score_val(img[t.o01]) * t.ax;
    const double bot = score_val(img[t.o10]) * (1.0 - t.ax) + score_val(img[t.o11]) * t.ax;
    return top * (1.0 - t.ay) + bot * t.ay;
}

// st: the (B, C, T) strides of flow_ab, a, b, flow_ba, in elements.
struct FsStrides { long s[4][3]; };

template <typename T, int C>
__global__ __launch_bounds__(C2M_FS_THREADS) void flow_consistency_kernel(
    const float* __restrict__ fab, const T* __restrict__ ia, const T* __restrict__ ib, const float* __restrict__ fba,
    const uint8_t* __restrict__ regions, int Tn, int H, int W, FsStrides st, double alpha1, double alpha2, unsigned tiles,
    float* __restrict__ photo_map, float* __restrict__ fb_map, uint8_t* __restrict__ incons_map, double* __restrict__ partial) {
    __shared__ double red[C2M_FS_THREADS / 64][C2M_SCORE_ROWS * C2M_FC_COLS];
    const int tid = threadIdx.x;
    const int HW = H * W;
    const unsigned frame = blockIdx.x / tiles, tile = blockIdx.x - frame * tiles;
    const int b = (int)(frame / (unsigned)Tn), t = (int)(frame - (unsigned)b * Tn);
    const float* __restrict__ fu_ = fab + (b * st.s[0][0] + t * st.s[0][2]);
    const float* __restrict__ fv_ = fu_ + st.s[0][1];
    const T* __restrict__ a_ = ia + (b * st.s[1][0] + t * st.s[1][2]);
    const T* __restrict__ b_ = ib + (b * st.s[2][0] + t * st.s[2][2]);
    const float* __restrict__ gu_ = fba != nullptr ? fba + (b * st.s[3][0] + t * st.s[3][2]) : nullptr;
    const float* __restrict__ gv_ = fba != nullptr ? gu_ + st.s[3][1] : nullptr;
    const long mask0 = (long)frame * HW;
    const float nanf_ = __uint_as_float(0x7fc00000u);

    double ph[C2M_FS_PPT], fbd[C2M_FS_PPT];
    unsigned flag[C2M_FS_PPT];          // 1 pixel, 2 inside, 4 inconsistent; the region byte << 8
#pragma unroll
    for (int j = 0; j < C2M_FS_PPT; ++j) {
        const long i = (long)tile * C2M_FS_TILE + j * C2M_FS_THREADS + tid;
        ph[j] = fbd[j] = 0.0;
        flag[j] = 0u;
        if (i < HW) {
            const int py = (int)(i / W), px = (int)(i - (long)py * W);
            const double fu = (double)fu_[i], fv = (double)fv_[i];
            const double yx = (double)px + fu, yy = (double)py + fv;
            const bool inside = fs_finite(fu) && fs_finite(fv) && yx >= 0.0 && yx <= (double)(W - 1) && yy >= 0.0 &&
                                yy <= (double)(H - 1);
            unsigned f = 1u;
            float pm = nanf_, fm = nanf_;
            if (inside) {
                const FsTap tap = fs_tap(yx, yy, H, W);
                double s = 0.0;
#pragma unroll
                for (int c = 0; c < C; ++c) s += fabs(score_val(a_[c * st.s[1][1] + i]) - fs_sample(b_ + c * st.s[2][1], tap));
                const double p = s / (double)C;
                ph[j] = p;
                pm = (float)p;
                f |= 2u;
                if (fba != nullptr) {
                    const double gu = fs_sample(gu_, tap), gv = fs_sample(gv_, tap);
                    const double su = fu + gu, sv = fv + gv;
                    const double fb2 = su * su + sv * sv;
                    const double root = sqrt(fb2);
                    if (!(fb2 <= alpha1 * ((fu * fu + fv * fv) + (gu * gu + gv * gv)) + alpha2)) f |= 4u;
                    if (fs_finite(fb2)) fbd[j] = root;
                    fm = (float)root;
                }
            }
            if (regions != nullptr) f |= (unsigned)regions[mask0 + i] << 8;
            flag[j] = f;
            if (photo_map != nullptr) {
                photo_map[mask0 + i] = pm;
                fb_map[mask0 + i] = fm;
                incons_map[mask0 + i] = (uint8_t)((f >> 2) & 1u);
            }
        }
    }

    const int lane = tid & 63, wave = tid >> 6;
    const int nrows = regions != nullptr ? C2M_SCORE_ROWS : 1;
    for (int k = 0; k < nrows; ++k) {
        int c0 = 0;                                         // three 10-bit counts
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
        for (int j = 0; j < C2M_FS_PPT; ++j) {
            const unsigned f = flag[j];
            const bool m = (f & 1u) && C2M_SCORE_ROW_HAS(k, f >> 8);
            if (m) c0 += 1 + (int)((f >> 1) & 1u) * (1 << 10) + (int)((f >> 2) & 1u) * (1 << 20);
            s0 += m ? ph[j] : 0.0;
            s1 += m ? ph[j] * ph[j] : 0.0;
            s2 += m ? fbd[j] : 0.0;
            s3 += m && !(f & 4u) ? ph[j] : 0.0;
        }
        c0 = wave_sum(c0);
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        s3 = wave_sum(s3);
        if (lane == 0) {
            double* r = &red[wave][k * C2M_FC_COLS];
            r[0] = (double)(c0 & 1023);
            r[1] = (double)((c0 >> 10) & 1023);
            r[2] = s0;
            r[3] = s1;
            r[4] = s2;
            r[5] = (double)((c0 >> 20) & 1023);
            r[6] = s3;
        }
    }
    __syncthreads();
    score_store_partial<C2M_FC_COLS>(red, nrows, partial);
}

static long fs_tiles(int H, int W) { return ((long)H * W + C2M_FS_TILE - 1) / C2M_FS_TILE; }

C2M_API long c2m_flow_quality_workspace_bytes(int B, int T, int H, int W) {
    return score_workspace_bytes(B, T, H, W, fs_tiles(H, W), C2M_FQ_COLS);
}

C2M_API long c2m_flow_consistency_workspace_bytes(int B, int T, int H, int W) {
    return score_workspace_bytes(B, T, H, W, fs_tiles(H, W), C2M_FC_COLS);
}

// (B, C, T) strides of one operand: none negative, and the channels of a pair apart by at least a plane.
static bool fs_strides_ok(const long* s, long plane, int channels) {
    return s[0] >= 0 && s[1] >= 0 && s[2] >= 0 && (channels < 2 || s[1] >= plane);
}

C2M_API int c2m_flow_quality(const void* pred, const float* target, const uint8_t* valid, const uint8_t* regions, int pred_dt,
                             int B, int T, int H, int W, const long* pred_strides, const long* target_strides, void* workspace,
                             long workspace_bytes, double* out, void* stream) {
    C2M_ENTER();
    if (B < 0 || T < 0 || H < 1 || W < 1 || pred_dt < 0 || pred_dt > 1 || pred_strides == nullptr || target_strides == nullptr)
        return (int)hipErrorInvalidValue;
    const long frames = (long)B * T, plane = (long)H * W;
    if (frames == 0) return 0;
    if (!score_sizes_ok(frames, plane, fs_tiles(H, W))) return (int)hipErrorInvalidValue;
    const long blocks = frames * fs_tiles(H, W);
    if (pred == nullptr || target == nullptr || out == nullptr || workspace == nullptr ||
        workspace_bytes < c2m_flow_quality_workspace_bytes(B, T, H, W) || !fs_strides_ok(pred_strides, plane, 2) ||
        !fs_strides_ok(target_strides, plane, 2))
        return (int)hipErrorInvalidValue;
    double* partial = (double*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const long* sp = pred_strides;
    const long* st = target_strides;
    if (pred_dt == 0)
        hipLaunchKernelGGL((flow_quality_kernel<float>), dim3((unsigned)blocks), dim3(C2M_FS_THREADS), 0, s, (const float*)pred,
                           target, valid, regions, T, (int)plane, sp[0], sp[1], sp[2], st[0], st[1], st[2],
                           (unsigned)fs_tiles(H, W), partial);
    else
        hipLaunchKernelGGL((flow_quality_kernel<bf16_t>), dim3((unsigned)blocks), dim3(C2M_FS_THREADS), 0, s,
                           (const bf16_t*)pred, target, valid, regions, T, (int)plane, sp[0], sp[1], sp[2], st[0], st[1], st[2],
                           (unsigned)fs_tiles(H, W), partial);
    C2M_LAUNCH_CHECK();
    return score_reduce<8, 128, C2M_FQ_COLS>(partial, frames, fs_tiles(H, W), C2M_FQ_COLS, out, s);
}

template <typename T, int C>
static void fc_launch(const float* fab, const void* a, const void* b, const float* fba, const uint8_t* regions, int Tn, int H,
                      int W, const FsStrides& st, double alpha1, double alpha2, unsigned tiles, unsigned blocks, float* photo,
                      float* fb, uint8_t* incons, double* partial, hipStream_t stream) {
    hipLaunchKernelGGL((flow_consistency_kernel<T, C>), dim3(blocks), dim3(C2M_FS_THREADS), 0, stream, fab, (const T*)a,
                       (const T*)b, fba, regions, Tn, H, W, st, alpha1, alpha2, tiles, photo, fb, incons, partial);
}

C2M_API int c2m_flow_consistency(const float* flow_ab, const void* a, const void* b, const float* flow_ba,
                                 const uint8_t* regions, int image_dt, int B, int C, int T, int H, int W, const long* strides,
                                 double alpha1, double alpha2, float* photo, float* fb, uint8_t* inconsistent, void* workspace,
                                 long workspace_bytes, double* out, void* stream) {
    C2M_ENTER();
    if (B < 0 || T < 0 || (C != 1 && C != 3) || H < 1 || W < 1 || image_dt < 0 || image_dt > 1 || strides == nullptr ||
        !(alpha1 >= 0.0) || !(alpha2 >= 0.0) || !(alpha1 < __builtin_huge_val()) || !(alpha2 < __builtin_huge_val()))
        return (int)hipErrorInvalidValue;
    const long frames = (long)B * T, plane = (long)H * W;
    if (frames == 0) return 0;
    if (!score_sizes_ok(frames, plane, fs_tiles(H, W))) return (int)hipErrorInvalidValue;
    const long blocks = frames * fs_tiles(H, W);
    const bool maps = photo != nullptr || fb != nullptr || inconsistent != nullptr;
    if (flow_ab == nullptr || a == nullptr || b == nullptr || out == nullptr || workspace == nullptr ||
        workspace_bytes < c2m_flow_consistency_workspace_bytes(B, T, H, W) ||
        (maps && (photo == nullptr || fb == nullptr || inconsistent == nullptr)))
        return (int)hipErrorInvalidValue;
    FsStrides st;
    for (int k = 0; k < 4; ++k) {
        const bool used = k < 3 || flow_ba != nullptr;
        if (used && !fs_strides_ok(strides + 3 * k, plane, k == 0 || k == 3 ? 2 : C)) return (int)hipErrorInvalidValue;
        for (int j = 0; j < 3; ++j) st.s[k][j] = used ? strides[3 * k + j] : 0;
    }
    double* partial = (double*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const unsigned tiles = (unsigned)fs_tiles(H, W);
#define C2M_FC_GO(TYPE)                                                                                                      \
    do {                                                                                                                     \
        if (C == 3) fc_launch<TYPE, 3>(flow_ab, a, b, flow_ba, regions, T, H, W, st, alpha1, alpha2, tiles, (unsigned)blocks,  \
                                       photo, fb, inconsistent, partial, s);                                                 \
        else fc_launch<TYPE, 1>(flow_ab, a, b, flow_ba, regions, T, H, W, st, alpha1, alpha2, tiles, (unsigned)blocks, photo, \
                                fb, inconsistent, partial, s);                                                               \
    } while (0)
    if (image_dt == 0) C2M_FC_GO(float);
    else C2M_FC_GO(bf16_t);
#undef C2M_FC_GO
    C2M_LAUNCH_CHECK();
    return score_reduce<8, 128, C2M_FC_COLS>(partial, frames, tiles, flow_ba != nullptr ? C2M_FC_COLS : 4, out, s);
}
