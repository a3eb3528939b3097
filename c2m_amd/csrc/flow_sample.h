// The bilinear gather of the flow kernels (dense_flow.hip, flow_refine.hip): one definition, so both read b's level alike.
#pragma once

// The coordinate is clamped to the image FIRST, so 0 <= x0 <= x1 <= w - 1 and 0 <= y0 <= y1 <= h - 1 whatever the flow is (a NaN
// goes to 0: fmaxf returns its other operand): every address of the gather is inside the level image.  The bound of step 6 on
// a KEPT flow (|u - u0| <= 8) says how far from the patch the final samples lie (a 25 x 25 window); it is not what keeps the
// reads in bounds, the clamp is.
__device__ __forceinline__ float fl_sample(const float* __restrict__ img, int h, int w, float fx, float fy) {
    fx = fminf(fmaxf(fx, 0.f), (float)(w - 1));
    fy = fminf(fmaxf(fy, 0.f), (float)(h - 1));
    const float x0f = floorf(fx), y0f = floorf(fy);
    const int x0 = (int)x0f, y0 = (int)y0f, x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    const float ax = fx - x0f, ay = fy - y0f;
    const float* __restrict__ r0 = img + (long)y0 * w;
    const float* __restrict__ r1 = img + (long)y1 * w;
    const float top = r0[x0] * (1.f - ax) + r0[x1] * ax;
    const float bot = r1[x0] * (1.f - ax) + r1[x1] * ax;
    return top * (1.f - ay) + bot * ay;
}
