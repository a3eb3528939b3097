// Chains of frame-to-frame flows (gfx950): the flow between two frames of a clip that are K frames apart, from the K flows between
// consecutive frames, by following every pixel through them.  c2m_amd.flow.chain_flows / clip_flows drive it; DESIGN.md 4.2n has
// the algorithm (tests/flow_chain_np.py restates it in numpy).  This file is compiled with -ffp-contract=off.
//
// Frames c_0 .. c_K, flows in pixels, channel 0 = x, a(x) ~ b(x + flow(x)).  A walk starts at a pixel with the displacement
// d = (0, 0); a hop through the step flow s reads s at p = pixel + d (fl_sample: the coordinate is clamped to the image before
// the gather, a NaN goes to 0; p itself is never clamped) and adds it to d.  The DISPLACEMENT is accumulated, not the position,
// so the first hop reads s at integer coordinates with weight exactly 1 and a one-hop chain returns the step's own values.
//
//   fc_backward_kernel  steps[j] = flow c_{j+1} -> c_j, out[k] = flow c_{k+1} -> c_0: the walk j = k, k - 1, ..., 0 from the
//                       pixel of c_{k+1}.  The walks of different k start in different frames and share no hop, so a thread
//                       serves ONE (k, pixel): K times the threads of a thread per pixel, and at most K dependent gathers in a
//                       thread instead of K (K + 1) / 2.  k is a coordinate of the block index, so the trip count is uniform
//                       in a workgroup, and the blocks of the longest walks come first in the grid.
//   fc_forward_kernel   steps[j] = flow c_j -> c_{j+1}, out[k] = flow c_0 -> c_{k+1}: all k are prefixes of ONE walk from the
//                       pixel of c_0, so a thread serves a pixel, walks j = 0 .. K - 1 and writes d after every hop.
//
// Both are gathers from the step planes (a training clip's fit in L2: 8 x 5 x 2 x 128 x 256 floats = 10.5 MB over eight XCDs'
// 4 MiB each) with coalesced stores, 256 threads on 256 consecutive pixels of a plane.  No LDS, no atomics, no barrier.
#include "common.h"
#include "flow_sample.h"

#define C2M_FC_MAX_K 16
#define C2M_FC_BLOCK 256

struct FcP {
    const float* steps; float* out; uint8_t* valid;
    int N, K, H, W, tiles;
};

// One hop of the pixel (x, y) through the step s (two planes): d += s(p), p = pixel + d.  Returns whether pixel + d is inside
// the frame after it (false for a NaN).
__device__ __forceinline__ bool fc_hop(const float* __restrict__ s, long plane, int H, int W, int x, int y, float& dx, float& dy) {
    const float px = (float)x + dx, py = (float)y + dy;
    const float sx = fl_sample(s, H, W, px, py), sy = fl_sample(s + plane, H, W, px, py);
    dx = dx + sx;
    dy = dy + sy;
    const float ex = (float)x + dx, ey = (float)y + dy;
    return ex >= 0.f && ex <= (float)(W - 1) && ey >= 0.f && ey <= (float)(H - 1);
}

__global__ __launch_bounds__(C2M_FC_BLOCK) void fc_backward_kernel(const FcP p) {
    const int tile = (int)(blockIdx.x % (unsigned)p.tiles), rest = (int)(blockIdx.x / (unsigned)p.tiles);
    const int k = p.K - 1 - rest % p.K, n = rest / p.K;
    const long plane = (long)p.H * p.W, q = (long)tile * C2M_FC_BLOCK + threadIdx.x;
    if (q >= plane) return;
    const int y = (int)(q / p.W), x = (int)(q - (long)y * p.W);
    const float* __restrict__ base = p.steps + (long)n * p.K * 2 * plane;
    float dx = 0.f, dy = 0.f;
    bool ok = true;
    for (int j = k; j >= 0; --j) ok = fc_hop(base + (long)j * 2 * plane, plane, p.H, p.W, x, y, dx, dy) && ok;
    const long o = (long)n * p.K + k;
    p.out[o * 2 * plane + q] = dx;
    p.out[(o * 2 + 1) * plane + q] = dy;
    if (p.valid) p.valid[o * plane + q] = ok ? 1 : 0;
}

__global__ __launch_bounds__(C2M_FC_BLOCK) void fc_forward_kernel(const FcP p) {
    const int tile = (int)(blockIdx.x % (unsigned)p.tiles), n = (int)(blockIdx.x / (unsigned)p.tiles);
    const long plane = (long)p.H * p.W, q = (long)tile * C2M_FC_BLOCK + threadIdx.x;
    if (q >= plane) return;
    const int y = (int)(q / p.W), x = (int)(q - (long)y * p.W);
    const float* __restrict__ base = p.steps + (long)n * p.K * 2 * plane;
    float dx = 0.f, dy = 0.f;
    bool ok = true;
    for (int j = 0; j < p.K; ++j) {
        ok = fc_hop(base + (long)j * 2 * plane, plane, p.H, p.W, x, y, dx, dy) && ok;
        const long o = (long)n * p.K + j;
        p.out[o * 2 * plane + q] = dx;
        p.out[(o * 2 + 1) * plane + q] = dy;
        if (p.valid) p.valid[o * plane + q] = ok ? 1 : 0;
    }
}

C2M_API int c2m_flow_chain(const float* steps, long step_elems, float* out, long out_elems, uint8_t* valid, long valid_elems,
                           int N, int K, int H, int W, int forward, void* stream) {
    C2M_ENTER();
    if (N < 0 || K < 1 || K > C2M_FC_MAX_K || H < 1 || W < 1 || (forward != 0 && forward != 1)) return (int)hipErrorInvalidValue;
    const long plane = (long)H * W, limit = 1L << 31;
    if (plane >= limit || 2L * N * K > (limit - 1) / plane) return (int)hipErrorInvalidValue;      // N K 2 H W < 2^31
    if (N == 0) return 0;
    const long total = 2L * N * K * plane;
    if (!steps || !out || step_elems < total || out_elems < total || (valid && valid_elems < total / 2) || (const float*)out == steps ||
        !c2m_aligned(4, steps, out))
        return (int)hipErrorInvalidValue;
    FcP p;
    p.steps = steps; p.out = out; p.valid = valid;
    p.N = N; p.K = K; p.H = H; p.W = W; p.tiles = c2m_cdiv(plane, C2M_FC_BLOCK);
    const long blocks = (long)N * (forward ? 1 : K) * p.tiles;                                      // <= N K H W < 2^30
    if (forward)
        hipLaunchKernelGGL(fc_forward_kernel, dim3((unsigned)blocks), dim3(C2M_FC_BLOCK), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(fc_backward_kernel, dim3((unsigned)blocks), dim3(C2M_FC_BLOCK), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}
