// Source coordinates of the backward warp (utils/ops.py:183-202 resample()), shared by the bilinear warp (warp.hip) and the
// nearest-neighbour label warp (label_warp.hip): one definition, so both read the same source position bit for bit.
// Files that include this are compiled with -ffp-contract=off: the arithmetic follows the fp32 operation order of ATen's
// CPU kernels (oracle/c2m_oracle_index.c documents and pins it), every fused multiply-add is explicit.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float lin_m1_1(int i, int steps) {
    if (steps <= 1) return -1.0f;
    const float step = 2.0f / (float)(steps - 1);
    const int half = steps / 2;
    return i < half ? fmaf(step, (float)i, -1.0f) : fmaf(-step, (float)(steps - 1 - i), 1.0f);
}

// (ix, iy): where output pixel (x, y) reads the input, in input pixels, BEFORE the border clamp: get_grid (align_corners=True
// convention) + pixel flow, un-normalised as grid_sample(align_corners=False) does.
__device__ __forceinline__ void warp_source(float fx, float fy, int x, int y, int H, int W, float& ix, float& iy) {
    const float cx = (float)(((double)W - 1.0) / 2.0), cy = (float)(((double)H - 1.0) / 2.0);
    const float gx = lin_m1_1(x, W) + fx / cx;
    const float gy = lin_m1_1(y, H) + fy / cy;
    ix = fmaf(gx + 1.0f, (float)W / 2.0f, -0.5f);
    iy = fmaf(gy + 1.0f, (float)H / 2.0f, -0.5f);
}

// The same rule at a fractional position, read on a larger grid (detail_warp.hip): (xl, yl) is a position on the h x w grid the
// flow lives on, (fx, fy) the flow there in h x w pixels, and (ix, iy) the position read on an H x W grid covering the same
// image, BEFORE the border clamp.  In real numbers ix = (xl + fx) * W / (w - 1) - 0.5.  At an integer position with H == h and
// W == w every operation below is warp_source's, so the two agree bit for bit (h, w >= 2).
__device__ __forceinline__ float lin_m1_1_at(float p, int steps) {
    const float step = 2.0f / (float)(steps - 1);
    return p < (float)(steps / 2) ? fmaf(step, p, -1.0f) : fmaf(-step, (float)(steps - 1) - p, 1.0f);
}

__device__ __forceinline__ void warp_source_at(float fx, float fy, float xl, float yl, int h, int w, int H, int W, float& ix,
                                               float& iy) {
    const float cx = (float)(((double)w - 1.0) / 2.0), cy = (float)(((double)h - 1.0) / 2.0);
    const float gx = lin_m1_1_at(xl, w) + fx / cx;
    const float gy = lin_m1_1_at(yl, h) + fy / cy;
    ix = fmaf(gx + 1.0f, (float)W / 2.0f, -0.5f);
    iy = fmaf(gy + 1.0f, (float)H / 2.0f, -0.5f);
}

// padding_mode="border" (ATen clip_coordinates): into [0, n - 1]; a NaN coordinate becomes 0
__device__ __forceinline__ float warp_border(float i, int n) { return fminf((float)(n - 1), fmaxf(i, 0.0f)); }

struct WarpCoord {
    int x0, y0, x1, y1;
    float nw, ne, sw, se;   // weights of (y0,x0) (y0,x1) (y1,x0) (y1,x1)
    float w_, e_, n_, s_;
    bool okx1, oky1;
    float gmx, gmy;         // d(ix)/d(flow_x), d(iy)/d(flow_y) incl. the border-clip gate
};

__device__ __forceinline__ WarpCoord warp_coord(float fx, float fy, int x, int y, int H, int W) {
    WarpCoord c;
    const float cx = (float)(((double)W - 1.0) / 2.0), cy = (float)(((double)H - 1.0) / 2.0);
    float ix, iy;
    warp_source(fx, fy, x, y, H, W, ix, iy);
    // clip_coordinates_set_grad (ATen GridSampler.h): gradient gate is 0 on/outside the border
    c.gmx = (ix > 0.0f && ix < (float)(W - 1)) ? ((float)W / 2.0f) / cx : 0.0f;
    c.gmy = (iy > 0.0f && iy < (float)(H - 1)) ? ((float)H / 2.0f) / cy : 0.0f;
    ix = warp_border(ix, W);
    iy = warp_border(iy, H);
    const float xw = floorf(ix), yn = floorf(iy);
    c.w_ = ix - xw; c.e_ = 1.0f - c.w_; c.n_ = iy - yn; c.s_ = 1.0f - c.n_;
    c.nw = c.s_ * c.e_; c.ne = c.s_ * c.w_; c.sw = c.n_ * c.e_; c.se = c.n_ * c.w_;
    c.x0 = (int)xw; c.y0 = (int)yn; c.x1 = c.x0 + 1; c.y1 = c.y0 + 1;
    c.okx1 = c.x1 < W; c.oky1 = c.y1 < H;
    return c;
}
