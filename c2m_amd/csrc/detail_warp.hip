// Predicted frames at dataset resolution (gfx950): the sharp last input frame moved along the generator's backward flow, with
// the generator's working-size output supplying what warping cannot.
//
//   c2m_detail_warp   one launch writes all B * T frames.  With up(A) the bilinear enlargement of a working-size plane
//                     (upsample_bilinear2d, align_corners=False) and warpF the bilinear value of the full-size uint8 frame F at
//                     the position the working-size warp reads, mapped to the large grid (warp_coord.h: warp_source_at and the
//                     shared border clamp):
//                         v     = 255 up(G) + up(occ) * (warpF - 255 up(Wl))
//                         level = floor(clip(v, 0, 255) + 0.5), NaN -> 0
//                     Instance ids, when given, are gathered at the nearest pixel of the same position (ties to even) and
//                     become fill_id where up(occ) < threshold; they are never blended.
//
// This file is compiled with -ffp-contract=off (see warp_coord.h).  The kernel is bandwidth-bound by design: per output pixel it
// writes 3 bytes (+ 4 of ids) and gathers 12 bytes of F; the nine working-size planes (G, Wl, flow, occ) are tiny next to that.
// A workgroup owns a TILE_H x TILE_W tile of one output frame and first stages the working-size patch its taps touch in LDS (at
// the workload's factor 8 that is 3 x 34 values per plane for 1024 output pixels), so the 36 working-size taps of a pixel are LDS
// reads.  A thread owns RUN = 4 adjacent pixels of a row: 12 output bytes, three aligned dwords when W % 4 == 0, and a wave
// writes 768 consecutive bytes of one row; other widths fall back to byte stores.  Nothing is accumulated across threads and
// there are no atomics: the result is bit-repeatable.
#include "common.h"
#include "warp_coord.h"

enum { DW_TILE_W = 256, DW_TILE_H = 4, DW_RUN = 4, DW_PLANES = 9 };   // planes: G 0-2, Wl 3-5, flow x 6, flow y 7, occ 8

struct DetailWarpP {
    const uint8_t* frame; const float* gen; const float* warped; const float* flow; const float* occ; const int32_t* ids;
    uint8_t* out; int32_t* out_ids;
    float threshold; int32_t fill_id;
    float rx, ry;                 // w / W, h / H
    int B, T, h, w, H, W;
    int ph, pw;                   // LDS patch: rows, pitch
    unsigned tiles_x, tiles_y;
    int vec;                      // rows of out (and out_ids) take aligned RUN-pixel stores
};

// One axis of upsample_bilinear2d(align_corners=False) at output index X: the un-clamped source position, the two taps, the
// weight of the second.
struct UpTap { float pos, lam; int i0, i1; };
__device__ __forceinline__ UpTap up_tap(int X, float r, int n) {
    UpTap t;
    t.pos = ((float)X + 0.5f) * r - 0.5f;
    const float s = fmaxf(t.pos, 0.0f);
    t.i0 = min((int)s, n - 1);
    t.i1 = min(t.i0 + 1, n - 1);
    t.lam = s - (float)t.i0;
    return t;
}

__global__ __launch_bounds__(256) void detail_warp_kernel(const DetailWarpP p) {
    extern __shared__ __attribute__((aligned(16))) float patch[];            // [DW_PLANES][ph][pw]
    const unsigned tile = blockIdx.x;
    const unsigned tx = tile % p.tiles_x, r0 = tile / p.tiles_x;
    const unsigned ty = r0 % p.tiles_y, bt = r0 / p.tiles_y;
    const int t = (int)(bt % (unsigned)p.T), b = (int)(bt / (unsigned)p.T);
    const int X0 = (int)tx * DW_TILE_W, Y0 = (int)ty * DW_TILE_H;

    // The taps are monotone in the output index, so the tile's first and last pixels bound the patch; the host sized ph x pw
    // to hold it, and the clamps below keep every LDS index inside it whatever the arithmetic does.
    const int px0 = up_tap(X0, p.rx, p.w).i0, py0 = up_tap(Y0, p.ry, p.h).i0;
    const int nw = max(min(up_tap(min(X0 + DW_TILE_W, p.W) - 1, p.rx, p.w).i1 - px0 + 1, p.pw), 1);
    const int nh = max(min(up_tap(min(Y0 + DW_TILE_H, p.H) - 1, p.ry, p.h).i1 - py0 + 1, p.ph), 1);
    const long hw = (long)p.h * p.w;
    const int plane = p.ph * p.pw, cells = nh * nw;
    for (int i = threadIdx.x; i < DW_PLANES * cells; i += blockDim.x) {
        const int c = i / cells, q = i - c * cells;
        const int py = q / nw, px = q - py * nw;
        const long sp = (long)(py0 + py) * p.w + (px0 + px);
        float v;
        if (c < 3) v = p.gen[(((long)b * 3 + c) * p.T + t) * hw + sp];
        else if (c < 6) v = p.warped[(((long)b * 3 + (c - 3)) * p.T + t) * hw + sp];
        else if (c < 8) v = p.flow[(((long)b * 2 + (c - 6)) * p.T + t) * hw + sp];
        else v = p.occ ? p.occ[((long)b * p.T + t) * hw + sp] : 1.0f;
        patch[c * plane + py * p.pw + px] = v;
    }
    __syncthreads();

    const int lx = threadIdx.x % (DW_TILE_W / DW_RUN), ly = threadIdx.x / (DW_TILE_W / DW_RUN);
    const int Y = Y0 + ly, Xr = X0 + lx * DW_RUN;
    if (Y >= p.H || Xr >= p.W) return;
    const UpTap uy = up_tap(Y, p.ry, p.h);
    const int ra = min(max(uy.i0 - py0, 0), nh - 1) * p.pw, rb = min(max(uy.i1 - py0, 0), nh - 1) * p.pw;
    const uint8_t* __restrict__ F = p.frame + (long)b * p.H * p.W * 3;
    const int32_t* __restrict__ ids = p.ids ? p.ids + (long)b * p.H * p.W : nullptr;

    uint8_t lv[DW_RUN * 3];
    int32_t id[DW_RUN];
#pragma unroll
    for (int e = 0; e < DW_RUN; ++e) {
        const int X = min(Xr + e, p.W - 1);             // past the row's end: computed like the last pixel, never stored
        const UpTap ux = up_tap(X, p.rx, p.w);
        const int ca = min(max(ux.i0 - px0, 0), nw - 1), cb = min(max(ux.i1 - px0, 0), nw - 1);
        const float w00 = (1.0f - uy.lam) * (1.0f - ux.lam), w01 = (1.0f - uy.lam) * ux.lam;
        const float w10 = uy.lam * (1.0f - ux.lam), w11 = uy.lam * ux.lam;
        float u[DW_PLANES];
#pragma unroll
        for (int c = 0; c < DW_PLANES; ++c) {
            const float* __restrict__ q = patch + c * plane;
            u[c] = w00 * q[ra + ca] + w01 * q[ra + cb] + w10 * q[rb + ca] + w11 * q[rb + cb];
        }
        float ix, iy;
        warp_source_at(u[6], u[7], ux.pos, uy.pos, p.h, p.w, p.H, p.W, ix, iy);
        // clamped to [0, n - 1] first (NaN -> 0), so every index below is in bounds for any flow
        ix = warp_border(ix, p.W);
        iy = warp_border(iy, p.H);
        const float xw = floorf(ix), yn = floorf(iy);
        const float lx1 = ix - xw, ly1 = iy - yn;
        const int x0 = (int)xw, y0 = (int)yn;
        const int x1 = min(x0 + 1, p.W - 1), y1 = min(y0 + 1, p.H - 1);
        const float nw_ = (1.0f - ly1) * (1.0f - lx1), ne_ = (1.0f - ly1) * lx1, sw_ = ly1 * (1.0f - lx1), se_ = ly1 * lx1;
        const uint8_t* __restrict__ a = F + ((long)y0 * p.W + x0) * 3;
        const uint8_t* __restrict__ bq = F + ((long)y0 * p.W + x1) * 3;
        const uint8_t* __restrict__ cq = F + ((long)y1 * p.W + x0) * 3;
        const uint8_t* __restrict__ dq = F + ((long)y1 * p.W + x1) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float wf = nw_ * (float)a[c] + ne_ * (float)bq[c] + sw_ * (float)cq[c] + se_ * (float)dq[c];
            const float v = 255.0f * u[c] + u[8] * (wf - 255.0f * u[3 + c]);
            lv[e * 3 + c] = (uint8_t)(int)(fminf(fmaxf(v, 0.0f), 255.0f) + 0.5f);      // fmaxf(NaN, 0) = 0
        }
        if (ids) {
            const int32_t s = ids[(long)(int)rintf(iy) * p.W + (int)rintf(ix)];
            id[e] = u[8] < p.threshold ? p.fill_id : s;
        }
    }

    const long row = ((long)b * p.T + t) * p.H + Y;
    uint8_t* __restrict__ o = p.out + (row * p.W + Xr) * 3;
    if (p.vec) {                                            // W % 4 == 0: the whole run is inside the row and dword aligned
        uint32_t d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            d[k] = (uint32_t)lv[4 * k] | (uint32_t)lv[4 * k + 1] << 8 | (uint32_t)lv[4 * k + 2] << 16 | (uint32_t)lv[4 * k + 3] << 24;
        uint32_t* __restrict__ o4 = reinterpret_cast<uint32_t*>(o);
        o4[0] = d[0]; o4[1] = d[1]; o4[2] = d[2];
        if (ids) *reinterpret_cast<int4*>(p.out_ids + row * p.W + Xr) = make_int4(id[0], id[1], id[2], id[3]);
    } else {
#pragma unroll
        for (int e = 0; e < DW_RUN; ++e) {
            if (Xr + e < p.W) {
                o[e * 3] = lv[e * 3]; o[e * 3 + 1] = lv[e * 3 + 1]; o[e * 3 + 2] = lv[e * 3 + 2];
                if (ids) p.out_ids[row * p.W + Xr + e] = id[e];
            }
        }
    }
}

// rows (or columns) of the working-size patch a tile of `tile` output pixels can touch: n_in / n_out <= 1 source pixels per
// output pixel, the second tap, and one more for the rounding of the fp32 source position
static inline int dw_patch(int tile, int n_in, int n_out) {
    const long span = ((long)(tile - 1) * n_in + n_out - 1) / n_out + 3;
    return (int)(span < n_in ? span : n_in);
}

C2M_API int c2m_detail_warp(const uint8_t* frame, const float* generated, const float* warped, const float* flow,
                            const float* occ, const int32_t* ids, float threshold, int fill_id, int B, int T, int h, int w,
                            int H, int W, uint8_t* out, int32_t* out_ids, void* stream) {
    C2M_ENTER();
    if (B < 0 || T < 0 || h < 2 || w < 2 || H < h || W < w) return (int)hipErrorInvalidValue;
    if ((long)B * T == 0) return 0;
    if (!frame || !generated || !warped || !flow || !out || (ids && !out_ids)) return (int)hipErrorInvalidValue;
    if ((long)H * W * 3 >= (1L << 31)) return (int)hipErrorInvalidValue;          // one frame is indexed with 32-bit pixel numbers
    const long tiles_x = c2m_cdiv(W, DW_TILE_W), tiles_y = c2m_cdiv(H, DW_TILE_H);
    const long tiles = tiles_x * tiles_y * B * T;
    if (tiles >= (1L << 31)) return (int)hipErrorInvalidValue;
    DetailWarpP p{frame, generated, warped, flow, occ, ids, out, out_ids, threshold, (int32_t)fill_id,
                  (float)w / (float)W, (float)h / (float)H, B, T, h, w, H, W,
                  dw_patch(DW_TILE_H, h, H), dw_patch(DW_TILE_W, w, W), (unsigned)tiles_x, (unsigned)tiles_y, 0};
    p.vec = W % DW_RUN == 0 && c2m_aligned(4, out) && (!ids || c2m_aligned(16, out_ids));
    const size_t lds = (size_t)DW_PLANES * p.ph * p.pw * sizeof(float);           // <= 9 * 6 * 258 * 4 = 55728 bytes
    hipLaunchKernelGGL(detail_warp_kernel, dim3((unsigned)tiles), dim3(256), lds, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}
