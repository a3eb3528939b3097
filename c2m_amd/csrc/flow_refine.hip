// Variational refinement of the dense inverse search flow (gfx950): on one pyramid level, the densified patch flow (u, v) is
// improved by `outer` fixed-point iterations of a robust data + gradient-constancy + smoothness energy, each solved by `sor`
// red-black SOR sweeps.  c2m_amd.flow.refine_flow / dense_flow(refine=...) drive it; DESIGN.md 4.2m has every formula with its
// association order (tests/flow_refine_np.py restates them in numpy).  This file is compiled with -ffp-contract=off.
//
//   fr_prepare_kernel   ONE launch per level: the eight planes Ix, Iy, Iz, Ixx, Ixy, Iyy, Ixz, Iyz.  A workgroup owns a 32 x 16 tile
//                       and stages 0.5 (J + Ia) and J - Ia for the tile plus a 2-pixel halo in LDS (J = b's level sampled at
//                       x + flow), positions clamped to the image; first derivatives for the tile plus 1 pixel come from that, the
//                       second ones from those: no second pass over global memory.  LDS: 2 * 36 * 20 + 2 * 34 * 18 floats = 10.7 KB.
//   fr_iterate_kernel   ONE launch per outer iteration.  A workgroup (1024 threads) owns a 32 x 32 tile.  It computes the
//                       coefficients of the linear system for the tile plus a halo of 2 sor pixels, runs all 2 sor half-sweeps on
//                       them in LDS behind workgroup barriers, and writes only its tile.  Half-sweep k updates the tile plus
//                       2 sor - 1 - k pixels: a pixel further out would read a neighbour that another tile's sweep has changed.
//                       Every value is produced by the same operations in the same order whatever tile computes it, so the
//                       result is bit-identical to the global red-black sweep and does not depend on the tiling.
//                       (du, dv) ping-pong between two buffers, since a neighbour tile reads the old values; the last iteration
//                       writes 2^shift (u + du, v + dv)[Y >> shift][X >> shift], the form c2m_flow_densify writes.
//
// LDS of fr_iterate_kernel, sor <= 5 (halo 10): 11 planes (du, dv, u, v, b1, b2, A12, A11 + sw, A22 + sw, wR, wD) of 52 x 52
// floats = 118 976 B, plus the smoothness weight ws on 54 x 54 = 11 664 B: 130 640 B of the CU's 163 840, one workgroup of 16
// waves per CU.  The coefficients are computed on 52^2 / 32^2 = 2.64 x the pixels of the tile, the sweeps on 1.67 x.
// The guided instantiation adds the ids of the 54 x 54 cells as an int plane, 11 664 B: 142 304 B.
#include "common.h"
#include "flow_sample.h"

#define C2M_FR_MAX_SIDE 32768
#define C2M_FR_MIN_SIDE 8
#define C2M_FR_MAX_SOR 5
#define C2M_FR_MAX_OUTER 1024
#define C2M_FR_MAX_SHIFT 6
#define C2M_FR_TILE 32
#define C2M_FR_RS (C2M_FR_TILE + 4 * C2M_FR_MAX_SOR)          // 52: the tile plus the largest halo, 2 sor a side
#define C2M_FR_WS (C2M_FR_RS + 2)                             // 54: one more pixel a side for the smoothness weight
#define C2M_FR_ZETA2 0.01f
#define C2M_FR_EPS2 1e-6f
#define C2M_FR_PT_W 32
#define C2M_FR_PT_H 16

static inline bool fr_level_ok(long N, long h, long w) {
    return N >= 0 && N < (1L << 24) && h >= C2M_FR_MIN_SIDE && w >= C2M_FR_MIN_SIDE && h <= C2M_FR_MAX_SIDE && w <= C2M_FR_MAX_SIDE;
}

// floats: the eight planes [8][N][h][w], then (du, dv) [N][2][h][w] twice (iteration k writes the one of index k & 1)
C2M_API long c2m_flow_refine_workspace_bytes(int N, int h, int w) {
    return fr_level_ok(N, h, w) ? 12L * N * h * w * 4 : -1;
}

// ------------------------------------------------------------------------------------------------ prepare
struct FrPrP {
    const float* ia; const float* ib; const float* flow; float* planes;
    int N, h, w, ty, tx;
};

__global__ __launch_bounds__(256) void fr_prepare_kernel(const FrPrP p) {
    constexpr int TW = C2M_FR_PT_W, TH = C2M_FR_PT_H, S2 = TW + 4, S1 = TW + 2;
    __shared__ float s_avg[(TH + 4) * S2], s_iz[(TH + 4) * S2], s_ix[(TH + 2) * S1], s_iy[(TH + 2) * S1];
    const int tid = threadIdx.x, h = p.h, w = p.w, tiles = p.ty * p.tx;
    const int tile = (int)(blockIdx.x % (unsigned)tiles), n = (int)(blockIdx.x / (unsigned)tiles);
    const int ty0 = (tile / p.tx) * TH, tx0 = (tile % p.tx) * TW;
    const long plane = (long)h * w;
    const float* __restrict__ A = p.ia + n * plane;
    const float* __restrict__ B = p.ib + n * plane;
    const float* __restrict__ U = p.flow + n * 2 * plane;
    // the tile plus 2 pixels, every position clamped to the image: an LDS cell holds the value AT the clamped position, so the
    // cell of a position inside the image holds that position's own value
    for (int idx = tid; idx < (TH + 4) * S2; idx += 256) {
        const int ly = idx / S2, lx = idx - ly * S2;
        const int gy = min(max(ty0 - 2 + ly, 0), h - 1), gx = min(max(tx0 - 2 + lx, 0), w - 1);
        const long q = (long)gy * w + gx;
        const float J = fl_sample(B, h, w, (float)gx + U[q], (float)gy + U[plane + q]);
        const float a = A[q];
        s_avg[idx] = 0.5f * (J + a);
        s_iz[idx] = J - a;
    }
    __syncthreads();
    // the cells of image positions (gy, gx) within 2 (1) pixels of the tile
    auto c2 = [&](int gy, int gx) { return (gy - (ty0 - 2)) * S2 + (gx - (tx0 - 2)); };
    auto c1 = [&](int gy, int gx) { return (gy - (ty0 - 1)) * S1 + (gx - (tx0 - 1)); };
    for (int idx = tid; idx < (TH + 2) * S1; idx += 256) {
        const int ly = idx / S1, lx = idx - ly * S1;
        const int gy = min(max(ty0 - 1 + ly, 0), h - 1), gx = min(max(tx0 - 1 + lx, 0), w - 1);
        s_ix[idx] = 0.5f * (s_avg[c2(gy, min(gx + 1, w - 1))] - s_avg[c2(gy, max(gx - 1, 0))]);
        s_iy[idx] = 0.5f * (s_avg[c2(min(gy + 1, h - 1), gx)] - s_avg[c2(max(gy - 1, 0), gx)]);
    }
    __syncthreads();
    const long P = (long)p.N * plane;
    for (int idx = tid; idx < TH * TW; idx += 256) {
        const int gy = ty0 + idx / TW, gx = tx0 + idx % TW;
        if (gy >= h || gx >= w) continue;
        const int xr = min(gx + 1, w - 1), xl = max(gx - 1, 0), yd = min(gy + 1, h - 1), yu = max(gy - 1, 0);
        float* __restrict__ o = p.planes + n * plane + (long)gy * w + gx;
        o[0] = s_ix[c1(gy, gx)];
        o[P] = s_iy[c1(gy, gx)];
        o[2 * P] = s_iz[c2(gy, gx)];
        o[3 * P] = 0.5f * (s_ix[c1(gy, xr)] - s_ix[c1(gy, xl)]);
        o[4 * P] = 0.5f * (s_ix[c1(yd, gx)] - s_ix[c1(yu, gx)]);
        o[5 * P] = 0.5f * (s_iy[c1(yd, gx)] - s_iy[c1(yu, gx)]);
        o[6 * P] = 0.5f * (s_iz[c2(gy, xr)] - s_iz[c2(gy, xl)]);
        o[7 * P] = 0.5f * (s_iz[c2(yd, gx)] - s_iz[c2(yu, gx)]);
    }
}

C2M_API int c2m_flow_refine_prepare(const float* ia, const float* ib, long image_elems, const float* flow, long flow_elems,
                                    void* workspace, long workspace_bytes, int N, int h, int w, void* stream) {
    C2M_ENTER();
    if (!fr_level_ok(N, h, w)) return (int)hipErrorInvalidValue;
    if (N == 0) return 0;
    FrPrP p;
    p.ia = ia; p.ib = ib; p.flow = flow; p.planes = (float*)workspace;
    p.N = N; p.h = h; p.w = w; p.ty = c2m_cdiv(h, C2M_FR_PT_H); p.tx = c2m_cdiv(w, C2M_FR_PT_W);
    const long blocks = (long)N * p.ty * p.tx;
    if (!ia || !ib || !flow || !workspace || image_elems < (long)N * h * w || flow_elems < 2L * N * h * w ||
        workspace_bytes < 12L * N * h * w * 4 || blocks >= (1L << 31) || !c2m_aligned(4, ia, ib, flow, workspace))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fr_prepare_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ iterate
struct FrItP {
    const float* planes; const float* flow; const float* din; float* dout; float* out;
    int N, h, w, ty, tx, sor, shift, Ho, Wo;
    float alpha, delta, gamma, omega, scale;
};

enum { FR_DU, FR_DV, FR_U, FR_V, FR_B1, FR_B2, FR_A12, FR_D1, FR_D2, FR_WR, FR_WD, FR_PLANES };

// the guide: ids [N][H][W] of level 0; the id of level pixel (y, x) is ids[y << level][x << level], inside the
// map: checked by the launcher.  No smoothness couples two ids: a forward difference toward another id counts as 0 in ws, and
// the weight of an edge between two ids is 0.
struct FrSegP {
    const int32_t* ids;
    int level, W;
    long plane;                                                                 // H * W
};

template <bool G>
__global__ __launch_bounds__(1024) void fr_iterate_kernel(const FrItP p, const FrSegP g) {
    constexpr int T = C2M_FR_TILE, RS = C2M_FR_RS, WS = C2M_FR_WS;
    __shared__ float s_ws[WS * WS];
    __shared__ float s[FR_PLANES][RS * RS];
    __shared__ int s_id[G ? WS * WS : 1];                                       // guided: the ids of the cells of s_ws
    const int tid = threadIdx.x, h = p.h, w = p.w, tiles = p.ty * p.tx;
    const int tile = (int)(blockIdx.x % (unsigned)tiles), n = (int)(blockIdx.x / (unsigned)tiles);
    const int ty0 = (tile / p.tx) * T, tx0 = (tile % p.tx) * T;
    const int halo = 2 * p.sor;                                                 // <= 10: checked by the launcher
    const int ry0 = ty0 - halo, rx0 = tx0 - halo, rn = T + 2 * halo;            // the region: cell (ly, lx) is pixel (ry0 + ly, rx0 + lx)
    const long plane = (long)h * w, P = (long)p.N * plane;
    const float* __restrict__ gu = p.flow + n * 2 * plane;
    const float* __restrict__ gv = gu + plane;
    const float* __restrict__ gdu = p.din ? p.din + n * 2 * plane : nullptr;    // NULL: du = dv = 0 (the first iteration)
    const float* __restrict__ gdv = p.din ? gdu + plane : nullptr;
    const float* __restrict__ pl = p.planes + n * plane;

    // smoothness weight ws on the region plus 1 pixel; cell (ly, lx) of s_ws is pixel (ry0 - 1 + ly, rx0 - 1 + lx)
    for (int idx = tid; idx < (rn + 2) * (rn + 2); idx += 1024) {
        const int ly = idx / (rn + 2), lx = idx - ly * (rn + 2), gy = ry0 - 1 + ly, gx = rx0 - 1 + lx;
        if (gy < 0 || gy >= h || gx < 0 || gx >= w) continue;
        const long q = (long)gy * w + gx, qr = (long)gy * w + min(gx + 1, w - 1), qd = (long)min(gy + 1, h - 1) * w + gx;
        const float U = gu[q] + (gdu ? gdu[q] : 0.f), V = gv[q] + (gdv ? gdv[q] : 0.f);
        float Ux = (gu[qr] + (gdu ? gdu[qr] : 0.f)) - U, Uy = (gu[qd] + (gdu ? gdu[qd] : 0.f)) - U;
        float Vx = (gv[qr] + (gdv ? gdv[qr] : 0.f)) - V, Vy = (gv[qd] + (gdv ? gdv[qd] : 0.f)) - V;
        if constexpr (G) {                                                      // the clamped neighbour of the last column / row is q itself
            const int32_t* __restrict__ S = g.ids + n * g.plane;
            const long row = (long)(gy << g.level) * g.W, rowd = (long)(min(gy + 1, h - 1) << g.level) * g.W;
            const int id = S[row + (gx << g.level)];
            if (S[row + (min(gx + 1, w - 1) << g.level)] != id) Ux = Vx = 0.f;
            if (S[rowd + (gx << g.level)] != id) Uy = Vy = 0.f;
            s_id[ly * WS + lx] = id;
        }
        s_ws[ly * WS + lx] = p.alpha / sqrtf((((Ux * Ux + Uy * Uy) + Vx * Vx) + Vy * Vy) + C2M_FR_EPS2);
    }
    __syncthreads();
    // the linear system on the region
    for (int idx = tid; idx < rn * rn; idx += 1024) {
        const int ly = idx / rn, lx = idx - ly * rn, gy = ry0 + ly, gx = rx0 + lx;
        if (gy < 0 || gy >= h || gx < 0 || gx >= w) continue;
        const long q = (long)gy * w + gx;
        const int c = ly * RS + lx, cw = (ly + 1) * WS + (lx + 1);
        const float ws = s_ws[cw];
        bool eR = gx < w - 1, eD = gy < h - 1, eL = gx > 0, eU = gy > 0;        // the edges of the smoothness graph at this pixel
        if constexpr (G) {                                                      // the cell of a neighbour inside the image holds its id
            const int id = s_id[cw];
            eR = eR && s_id[cw + 1] == id; eD = eD && s_id[cw + WS] == id;
            eL = eL && s_id[cw - 1] == id; eU = eU && s_id[cw - WS] == id;
        }
        const float wR = eR ? 0.5f * (ws + s_ws[cw + 1]) : 0.f, wD = eD ? 0.5f * (ws + s_ws[cw + WS]) : 0.f;
        const float wL = eL ? 0.5f * (s_ws[cw - 1] + ws) : 0.f, wU = eU ? 0.5f * (s_ws[cw - WS] + ws) : 0.f;
        const float sw = ((wL + wR) + wU) + wD;
        const float du = gdu ? gdu[q] : 0.f, dv = gdv ? gdv[q] : 0.f;
        const float Ix = pl[q], Iy = pl[P + q], Iz = pl[2 * P + q], Ixx = pl[3 * P + q], Ixy = pl[4 * P + q], Iyy = pl[5 * P + q],
                    Ixz = pl[6 * P + q], Iyz = pl[7 * P + q];
        const float nI = (Ix * Ix + Iy * Iy) + C2M_FR_ZETA2, nX = (Ixx * Ixx + Ixy * Ixy) + C2M_FR_ZETA2,
                    nY = (Ixy * Ixy + Iyy * Iyy) + C2M_FR_ZETA2;
        const float r = (Iz + Ix * du) + Iy * dv;
        const float wd = (p.delta / sqrtf((r * r) / nI + C2M_FR_EPS2)) / nI;
        const float rx = (Ixz + Ixx * du) + Ixy * dv, ry = (Iyz + Ixy * du) + Iyy * dv;
        const float wg = p.gamma / sqrtf(((rx * rx) / nX + (ry * ry) / nY) + C2M_FR_EPS2);
        const float wgx = wg / nX, wgy = wg / nY;
        const float A11 = ((wd * Ix) * Ix + (wgx * Ixx) * Ixx) + (wgy * Ixy) * Ixy;
        const float A12 = ((wd * Ix) * Iy + (wgx * Ixx) * Ixy) + (wgy * Ixy) * Iyy;
        const float A22 = ((wd * Iy) * Iy + (wgx * Ixy) * Ixy) + (wgy * Iyy) * Iyy;
        s[FR_B1][c] = -(((wd * Iz) * Ix + (wgx * Ixz) * Ixx) + (wgy * Iyz) * Ixy);
        s[FR_B2][c] = -(((wd * Iz) * Iy + (wgx * Ixz) * Ixy) + (wgy * Iyz) * Iyy);
        s[FR_A12][c] = A12; s[FR_D1][c] = A11 + sw; s[FR_D2][c] = A22 + sw;
        s[FR_WR][c] = wR; s[FR_WD][c] = wD;
        s[FR_DU][c] = du; s[FR_DV][c] = dv; s[FR_U][c] = gu[q]; s[FR_V][c] = gv[q];
    }
    // 2 sor half-sweeps, colour (x + y) & 1 == 0 first; half-sweep k updates the tile plus m = halo - 1 - k pixels, whose
    // neighbours (1 <= cell index <= 50 < RS on both axes) still hold the values of the global sweep
    const float om1 = 1.f - p.omega;
    for (int k = 0; k < halo; ++k) {                                            // workgroup-uniform
        __syncthreads();
        const int off = k + 1, m = halo - 1 - k, un = T + 2 * m, half = (un + 1) >> 1, colour = k & 1;
        for (int idx = tid; idx < un * half; idx += 1024) {
            const int r = idx / half, j = idx - r * half, ly = off + r, gy = ry0 + ly;
            const int lx = off + 2 * j + ((colour + rx0 + off + gy) & 1), gx = rx0 + lx;
            if (lx >= off + un || gy < 0 || gy >= h || gx < 0 || gx >= w) continue;
            const int c = ly * RS + lx;
            const int cl = gx > 0 ? c - 1 : c, cr = gx < w - 1 ? c + 1 : c, cu = gy > 0 ? c - RS : c, cd = gy < h - 1 ? c + RS : c;
            const float wL = gx > 0 ? s[FR_WR][c - 1] : 0.f, wR = s[FR_WR][c], wU = gy > 0 ? s[FR_WD][c - RS] : 0.f, wD = s[FR_WD][c];
            const float sw = ((wL + wR) + wU) + wD;
            const float su = (((wL * (s[FR_U][cl] + s[FR_DU][cl]) + wR * (s[FR_U][cr] + s[FR_DU][cr])) +
                               wU * (s[FR_U][cu] + s[FR_DU][cu])) + wD * (s[FR_U][cd] + s[FR_DU][cd])) - sw * s[FR_U][c];
            const float sv = (((wL * (s[FR_V][cl] + s[FR_DV][cl]) + wR * (s[FR_V][cr] + s[FR_DV][cr])) +
                               wU * (s[FR_V][cu] + s[FR_DV][cu])) + wD * (s[FR_V][cd] + s[FR_DV][cd])) - sw * s[FR_V][c];
            const float A12 = s[FR_A12][c];
            float du = om1 * s[FR_DU][c] + p.omega * (((s[FR_B1][c] + su) - A12 * s[FR_DV][c]) / s[FR_D1][c]);
            if constexpr (G) {                                                  // all edges cut and a flat image: D1 = A11 = 0, du stays
                if (!(s[FR_D1][c] > 0.f)) du = s[FR_DU][c];
            }
            float dv = om1 * s[FR_DV][c] + p.omega * (((s[FR_B2][c] + sv) - A12 * du) / s[FR_D2][c]);
            if constexpr (G) {
                if (!(s[FR_D2][c] > 0.f)) dv = s[FR_DV][c];
            }
            s[FR_DU][c] = du; s[FR_DV][c] = dv;
        }
    }
    __syncthreads();
    if (!p.out) {                                                               // (du, dv) of the tile for the next iteration
        float* __restrict__ o = p.dout + n * 2 * plane;
        const int gy = ty0 + (tid >> 5), gx = tx0 + (tid & 31);
        if (gy < h && gx < w) {
            const int c = (halo + (tid >> 5)) * RS + halo + (tid & 31);
            o[(long)gy * w + gx] = s[FR_DU][c];
            o[plane + (long)gy * w + gx] = s[FR_DV][c];
        }
        return;
    }
    // the last iteration: 2^shift (u + du, v + dv)[Y >> shift][X >> shift] for the output pixels whose level pixel is in the tile
    const long oplane = (long)p.Ho * p.Wo;
    float* __restrict__ o = p.out + n * 2 * oplane;
    const int bits = 5 + p.shift, side = T << p.shift;                          // side^2 <= 2^22
    for (int idx = tid; idx < side * side; idx += 1024) {
        const int oy = idx >> bits, ox = idx & (side - 1), Y = (ty0 << p.shift) + oy, X = (tx0 << p.shift) + ox;
        if (Y >= p.Ho || X >= p.Wo) continue;                                   // Y >> shift < h: checked by the launcher
        const int c = (halo + (oy >> p.shift)) * RS + halo + (ox >> p.shift);
        o[(long)Y * p.Wo + X] = p.scale * (s[FR_U][c] + s[FR_DU][c]);
        o[oplane + (long)Y * p.Wo + X] = p.scale * (s[FR_V][c] + s[FR_DV][c]);
    }
}

// ids NULL: the unguided iteration
static int fr_iterate(const float* flow, long flow_elems, void* workspace, long workspace_bytes, int N, int h, int w, int iteration,
                      int sor, float alpha, float delta, float gamma, float omega, float* out, long out_elems, int shift, int Ho,
                      int Wo, const int32_t* ids, int level, int H, int W, void* stream) {
    auto weight = [](float v) { return v > 0.f && v < 3.0e38f; };               // false for a NaN
    if (!fr_level_ok(N, h, w) || iteration < 0 || iteration >= C2M_FR_MAX_OUTER || sor < 1 || sor > C2M_FR_MAX_SOR ||
        !weight(alpha) || !weight(delta) || !weight(gamma) || !(omega > 0.f && omega < 2.f))
        return (int)hipErrorInvalidValue;
    if (out && (shift < 0 || shift > C2M_FR_MAX_SHIFT || Ho < 1 || Wo < 1 || Ho > C2M_FR_MAX_SIDE || Wo > C2M_FR_MAX_SIDE ||
                ((Ho - 1) >> shift) >= h || ((Wo - 1) >> shift) >= w))
        return (int)hipErrorInvalidValue;
    if (N == 0) return 0;
    const long P = (long)N * h * w;
    FrItP p;
    float* ws = (float*)workspace;
    p.planes = ws; p.flow = flow; p.out = out;
    p.din = iteration == 0 ? nullptr : ws + 8 * P + 2 * P * ((iteration - 1) & 1);
    p.dout = ws + 8 * P + 2 * P * (iteration & 1);
    p.N = N; p.h = h; p.w = w; p.ty = c2m_cdiv(h, C2M_FR_TILE); p.tx = c2m_cdiv(w, C2M_FR_TILE);
    p.sor = sor; p.shift = out ? shift : 0; p.Ho = out ? Ho : h; p.Wo = out ? Wo : w;
    p.alpha = alpha; p.delta = delta; p.gamma = gamma; p.omega = omega; p.scale = (float)(1 << p.shift);
    const long blocks = (long)N * p.ty * p.tx;
    if (!flow || !workspace || flow_elems < 2 * P || workspace_bytes < 12 * P * 4 || blocks >= (1L << 31) ||
        (out && out_elems < 2L * N * Ho * Wo) || !c2m_aligned(4, flow, workspace, out))
        return (int)hipErrorInvalidValue;
    const FrSegP g = {ids, level, W, (long)H * W};
    if (ids) hipLaunchKernelGGL(fr_iterate_kernel<true>, dim3((unsigned)blocks), dim3(1024), 0, (hipStream_t)stream, p, g);
    else hipLaunchKernelGGL(fr_iterate_kernel<false>, dim3((unsigned)blocks), dim3(1024), 0, (hipStream_t)stream, p, g);
    return (int)hipGetLastError();
}

C2M_API int c2m_flow_refine_iterate(const float* flow, long flow_elems, void* workspace, long workspace_bytes, int N, int h, int w,
                                    int iteration, int sor, float alpha, float delta, float gamma, float omega, float* out,
                                    long out_elems, int shift, int Ho, int Wo, void* stream) {
    C2M_ENTER();
    return fr_iterate(flow, flow_elems, workspace, workspace_bytes, N, h, w, iteration, sor, alpha, delta, gamma, omega, out,
                      out_elems, shift, Ho, Wo, nullptr, 0, 0, 0, stream);
}

C2M_API int c2m_flow_refine_iterate_guided(const float* flow, long flow_elems, void* workspace, long workspace_bytes, int N, int h,
                                           int w, int iteration, int sor, float alpha, float delta, float gamma, float omega,
                                           float* out, long out_elems, int shift, int Ho, int Wo, const int32_t* segments,
                                           long segment_elems, int level, int H, int W, void* stream) {
    C2M_ENTER();
    if (!fr_level_ok(N, h, w) || level < 0 || level > C2M_FR_MAX_SHIFT || H < 1 || W < 1 || H > C2M_FR_MAX_SIDE ||
        W > C2M_FR_MAX_SIDE || ((long)(h - 1) << level) >= H || ((long)(w - 1) << level) >= W ||
        (N > 0 && (!segments || segment_elems < (long)N * H * W || !c2m_aligned(4, segments))))
        return (int)hipErrorInvalidValue;
    return fr_iterate(flow, flow_elems, workspace, workspace_bytes, N, h, w, iteration, sor, alpha, delta, gamma, omega, out,
                      out_elems, shift, Ho, Wo, segments, level, H, W, stream);
}
