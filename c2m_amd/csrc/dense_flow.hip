// Dense inverse search optical flow (gfx950): a classical, weight-free flow a -> b between two frames, in pixels, channel 0 = x,
// with a(x) ~ b(x + flow(x)) -- the convention of c2m_occlusion_splat and of FlowNet2's output.  c2m_amd.flow.dense_flow drives
// it; DESIGN.md 4.2l has the algorithm, operation by operation (tests/dense_flow_np.py restates it in numpy), and the cost.
//
//   fl_pyramid_kernel       gray (0.299 R + 0.587 G + 0.114 B of the frame mapped to 0..255) and every 2x2-mean level of both frames
//                           of all N pairs in ONE launch: a workgroup owns a 64 x 64 tile of level 0, keeps every level of it in
//                           LDS and halves it level by level.  A tile origin is a multiple of 64 >> l at level l, and the 2 x 2
//                           block of a level-(l+1) pixel, clamped to the last row and column, lies in the same tile: no workgroup
//                           reads what another one wrote.
//   fl_patch_search_kernel  one wave per 8 x 8 patch (stride 4; a last, more overlapping patch where the size is no multiple of 4),
//                           lane = (py, px) = (lane >> 3, lane & 7).  The lane's template pixel and its two gradients stay in
//                           registers; every sum over the patch is a wave_sum_all (fixed shuffle order, so bit-repeatable).  A fixed
//                           number of inverse-compositional steps, no early exit: the result cannot depend on which waves finished
//                           first.  The x2 up-sampling of the coarser level's flow is fused into the read of the initial flow.
//                           One record per patch: u, v, mean(J) - mean(T) at the final flow.
//   fl_densify_kernel       one thread per pixel: the <= 3 x 3 patches that cover it in ascending (oy, ox) order, each weighted by
//                           1 / max(1, |residual of that patch at this pixel|).  No atomics.  With shift > 0 it writes the flow of a
//                           coarser level straight at the size of level 0 (2^shift * f[y >> shift][x >> shift]).
//
//   fl_patch_match_kernel   the optional seed of the coarsest level (at the end of this file): one wave per patch tries
//                           every integer displacement within a radius whose window lies inside b and keeps the cheapest; its
//                           records are densified as the search's are, and the search starts from that flow.
//
// Segment guide: the <true> instantiations of the search and the densify read the level-0 id map of frame a
// (level l reads it at (y << l, x << l)).  A patch sum runs over the lanes whose id is that of the patch centre, a pixel is
// averaged over the covering patches whose centre has its id; a record gains the lane count n as a fourth float.  The <false>
// instantiations are the code above, untouched.
//
// The window of b that a patch samples is read through L1 / L2, not staged in LDS: a level image of the training
// size is <= 128 KB, a patch touches about 9 x 9 floats of it per step, and with no early exit the flow is bounded only at the
// END of the search (step 6), so a staged 25 x 25 window would still need the global path next to it.
#include "common.h"
#include "dtype.h"

#define C2M_FLOW_MAX_LEVELS 7           // 64 >> 6 = 1: the coarsest level a 64 x 64 tile still holds a pixel of
#define C2M_FLOW_MAX_SIDE 32768
#define C2M_FLOW_PATCH 8
#define C2M_FLOW_STRIDE 4
#define C2M_FLOW_MAX_ITERS 1024
#define C2M_FLOW_DET_MIN 40.96f         // 1e-2 * 64^2
#define C2M_FLOW_MAX_STEP2 64.0f        // (8 px)^2

// ------------------------------------------------------------------------------------------------ sizes and the workspace
// floats: per level l the images a[N][h][w] then b[N][h][w]; then the patch records of the largest level [N][npy][npx][3]; then
// the dense flows of the levels 1 .. levels - 1, [N][2][h][w] each (level 0's goes to the caller's tensor).
struct FlLayout {
    int h[C2M_FLOW_MAX_LEVELS], w[C2M_FLOW_MAX_LEVELS];
    long img[C2M_FLOW_MAX_LEVELS], flow[C2M_FLOW_MAX_LEVELS], rec, total;
};

static inline int fl_patches(int n) {                       // origins 0, 4, 8, ... <= n - 8, plus n - 8 if that is not one of them
    return (n - C2M_FLOW_PATCH) / C2M_FLOW_STRIDE + 1 + ((n - C2M_FLOW_PATCH) % C2M_FLOW_STRIDE != 0);
}

static inline bool fl_level_ok(long N, long h, long w) {
    return N >= 0 && N < (1L << 24) && h >= C2M_FLOW_PATCH && w >= C2M_FLOW_PATCH && h <= C2M_FLOW_MAX_SIDE && w <= C2M_FLOW_MAX_SIDE;
}

static bool fl_layout(long N, long H, long W, int levels, FlLayout& L) {
    if (levels < 1 || levels > C2M_FLOW_MAX_LEVELS || !fl_level_ok(N, H, W)) return false;
    long off = 0, h = H, w = W;
    for (int l = 0; l < levels; ++l, h = (h + 1) / 2, w = (w + 1) / 2) {
        if (h < C2M_FLOW_PATCH || w < C2M_FLOW_PATCH) return false;
        L.h[l] = (int)h; L.w[l] = (int)w; L.img[l] = off;
        off += 2 * N * h * w;
    }
    L.rec = off;
    off += N * fl_patches((int)H) * fl_patches((int)W) * 3;
    L.flow[0] = -1;
    for (int l = 1; l < levels; ++l) { L.flow[l] = off; off += 2 * N * L.h[l] * (long)L.w[l]; }
    L.total = off;
    return true;
}

C2M_API long c2m_flow_workspace_bytes(int N, int H, int W, int levels) {
    FlLayout L;
    return fl_layout(N, H, W, levels, L) ? L.total * 4 : -1;
}

C2M_API long c2m_flow_workspace_offset(int N, int H, int W, int levels, int what, int level) {
    FlLayout L;
    if (!fl_layout(N, H, W, levels, L) || level < 0 || level >= levels) return -1;
    switch (what) {
        case 0: return L.img[level];
        case 1: return L.img[level] + (long)N * L.h[level] * L.w[level];
        case 2: return L.flow[level];
        case 3: return L.rec;
        default: return -1;
    }
}

// ------------------------------------------------------------------------------------------------ pyramid
struct FlPyrP {
    const void* src[2]; float* ws;
    int N, H, W, levels, ty, tx;
    int h[C2M_FLOW_MAX_LEVELS], w[C2M_FLOW_MAX_LEVELS];
    long img[C2M_FLOW_MAX_LEVELS];
    float lo, scale;
};

template <class T>
__global__ __launch_bounds__(256) void fl_pyramid_kernel(const FlPyrP p) {
    __shared__ float lds[4096 + 1024 + 256 + 64 + 16 + 4 + 1];
    const int tiles = p.ty * p.tx, tid = threadIdx.x;
    const long items = 2L * p.N * tiles;
    for (long item = blockIdx.x; item < items; item += gridDim.x) {             // workgroup-uniform
        const int tile = (int)(item % tiles), ty = tile / p.tx, tx = tile % p.tx;
        const long im = item / tiles;                                           // a of pair 0 .. N-1, then b of pair 0 .. N-1
        const int which = im >= p.N;
        const T* __restrict__ src = (const T*)p.src[which] + (im - (long)which * p.N) * 3 * p.H * (long)p.W;
        const long plane = (long)p.H * p.W;
        __syncthreads();                                                        // the previous item's last level has been read
        for (int k = 0; k < 16; ++k) {
            const int idx = k * 256 + tid, gy = ty * 64 + (idx >> 6), gx = tx * 64 + (idx & 63);
            if (gy < p.H && gx < p.W) {
                const long q = (long)gy * p.W + gx;
                const float r = (c2m_ld(src, q) - p.lo) * p.scale, g = (c2m_ld(src, plane + q) - p.lo) * p.scale,
                            b = (c2m_ld(src, 2 * plane + q) - p.lo) * p.scale;
                const float v = (0.299f * r + 0.587f * g) + 0.114f * b;
                lds[idx] = v;
                p.ws[p.img[0] + im * plane + q] = v;
            }
        }
        int below = 0;                                                          // LDS offset of level l - 1
        for (int l = 1; l < p.levels; ++l) {                                    // workgroup-uniform
            __syncthreads();
            const int side = 64 >> l, here = below + (4096 >> (2 * (l - 1)));
            const int h = p.h[l], w = p.w[l], hb = p.h[l - 1], wb = p.w[l - 1];
            for (int idx = tid; idx < side * side; idx += 256) {
                const int ly = idx >> (6 - l), lx = idx & (side - 1), gy = ty * side + ly, gx = tx * side + lx;
                if (gy < h && gx < w) {
                    // rows 2 gy, min(2 gy + 1, hb - 1) of the level below, as rows of this tile (origin 2 * side * ty)
                    const int y0 = 2 * ly, y1 = min(2 * gy + 1, hb - 1) - 2 * side * ty;
                    const int x0 = 2 * lx, x1 = min(2 * gx + 1, wb - 1) - 2 * side * tx;
                    const float* b = lds + below;
                    const int s = 2 * side;
                    const float v = (((b[y0 * s + x0] + b[y0 * s + x1]) + b[y1 * s + x0]) + b[y1 * s + x1]) * 0.25f;
                    lds[here + idx] = v;
                    p.ws[p.img[l] + im * ((long)h * w) + (long)gy * w + gx] = v;
                }
            }
            below = here;
        }
    }
}

C2M_API int c2m_flow_pyramid(const void* a, const void* b, int dt, float lo, float hi, int N, int H, int W, int levels,
                             void* workspace, long workspace_bytes, void* stream) {
    C2M_ENTER();
    FlLayout L;
    if (!fl_layout(N, H, W, levels, L) || (dt != C2M_F32 && dt != C2M_BF16) || !(hi > lo) || !(hi - lo < 3.0e38f))
        return (int)hipErrorInvalidValue;
    if (N == 0) return 0;
    if (!a || !b || !workspace || workspace_bytes < L.total * 4 || !c2m_aligned(4, workspace) ||
        !c2m_aligned(dt == C2M_BF16 ? 2 : 4, a, b))
        return (int)hipErrorInvalidValue;
    FlPyrP p;
    p.src[0] = a; p.src[1] = b; p.ws = (float*)workspace;
    p.N = N; p.H = H; p.W = W; p.levels = levels; p.ty = (H + 63) / 64; p.tx = (W + 63) / 64;
    for (int l = 0; l < C2M_FLOW_MAX_LEVELS; ++l) {
        p.h[l] = l < levels ? L.h[l] : 0; p.w[l] = l < levels ? L.w[l] : 0; p.img[l] = l < levels ? L.img[l] : 0;
    }
    p.lo = lo; p.scale = (float)(255.0 / ((double)hi - (double)lo));
    const long items = 2L * N * p.ty * p.tx;
    const dim3 grid((unsigned)(items < 65536 ? items : 65536));
    C2M_DISPATCH_DT(dt, hipLaunchKernelGGL(fl_pyramid_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, p););
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ bilinear sample of b's level
#include "flow_sample.h"                // fl_sample: the coordinate is clamped to the image before the gather

// ------------------------------------------------------------------------------------------------ patch search
struct FlPsP {
    const float* ia; const float* ib; const float* init; float* rec;
    int h, w, npy, npx, hc, wc, shift, iters;
    long waves;                                                                 // N * npy * npx: one wave each
};

// the guide: ids [N][H][W] of level 0; the id of level pixel (y, x) is ids[y << level][x << level], inside the map: checked by
// the launchers
struct FlSegP {
    const int32_t* ids;
    int level, W;
    long plane;                                                                 // H * W
    __device__ __forceinline__ int at(long n, int y, int x) const {
        return ids[n * plane + (long)(y << level) * W + (x << level)];
    }
};

static inline bool fl_seg_ok(const int32_t* ids, long elems, long N, int level, int H, int W, int h, int w) {
    return level >= 0 && level < C2M_FLOW_MAX_LEVELS && H >= 1 && W >= 1 && H <= C2M_FLOW_MAX_SIDE && W <= C2M_FLOW_MAX_SIDE &&
           ((long)(h - 1) << level) < H && ((long)(w - 1) << level) < W && (N == 0 || (ids && elems >= N * (long)H * W &&
           c2m_aligned(4, ids)));
}

template <bool G>
__global__ __launch_bounds__(256) void fl_patch_search_kernel(const FlPsP p, const FlSegP g) {
    const int lane = threadIdx.x & 63, py = lane >> 3, px = lane & 7;
    const int h = p.h, w = p.w;
    const long nwaves = (long)gridDim.x * 4;
    for (long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6); i < p.waves; i += nwaves) {          // wave-uniform
        const int jx = (int)(i % p.npx);
        const long t = i / p.npx;
        const int jy = (int)(t % p.npy);
        const long n = t / p.npy;
        const int ox = min(C2M_FLOW_STRIDE * jx, w - C2M_FLOW_PATCH), oy = min(C2M_FLOW_STRIDE * jy, h - C2M_FLOW_PATCH);
        const int x = ox + px, y = oy + py;                                     // inside the image: ox + 7 <= w - 1
        const float* __restrict__ A = p.ia + n * ((long)h * w);
        const float* __restrict__ B = p.ib + n * ((long)h * w);
        const float* __restrict__ row = A + (long)y * w;
        const float T = row[x];
        const float gx = 0.5f * (row[min(x + 1, w - 1)] - row[max(x - 1, 0)]);
        const float gy = 0.5f * (A[(long)min(y + 1, h - 1) * w + x] - A[(long)max(y - 1, 0) * w + x]);
        float u0 = 0.f, v0 = 0.f;
        if (p.init) {                                                           // 2 * f_coarser[y // 2][x // 2] at the patch centre
            const int cy = (oy + 3) >> p.shift, cx = (ox + 3) >> p.shift;      // < hc, wc = ceil(h, w / 2^shift)
            const float* __restrict__ F = p.init + n * 2 * ((long)p.hc * p.wc) + (long)cy * p.wc + cx;
            const float s = (float)(1 << p.shift);
            u0 = s * F[0];
            v0 = s * F[(long)p.hc * p.wc];
        }
        // guided: the lanes whose id is that of the patch centre (the pixel the initial flow is read at) carry the sums, the
        // others add 0.f in the same shuffle order; cnt >= 1, the centre lane
        bool in = true;
        float cnt = 64.f, det_min = C2M_FLOW_DET_MIN;
        if constexpr (G) {
            in = g.at(n, y, x) == g.at(n, oy + 3, ox + 3);
            const int k = wave_count(in);
            cnt = (float)k;
            det_min = C2M_FLOW_DET_MIN * ((float)(k * k) / 4096.f);
        }
        auto part = [&](float v) { if constexpr (G) return in ? v : 0.f; else return v; };
        auto mean = [&](float s) { if constexpr (G) return s / cnt; else return s * 0.015625f; };
        const float mT = mean(wave_sum_all(part(T))), Tm = T - mT;
        const float a = wave_sum_all(part(gx * gx)), b = wave_sum_all(part(gx * gy)), c = wave_sum_all(part(gy * gy));
        const float det = a * c - b * b;
        float u = u0, v = v0;
        if (det > det_min) {                                                    // wave-uniform: every lane holds lane 0's sums
            for (int it = 0; it < p.iters; ++it) {
                const float J = fl_sample(B, h, w, (float)x + u, (float)y + v);
                const float mJ = mean(wave_sum_all(part(J)));
                const float r = (J - mJ) - Tm;
                const float bx = wave_sum_all(part(r * gx)), by = wave_sum_all(part(r * gy));
                u -= (c * bx - b * by) / det;
                v -= (a * by - b * bx) / det;
            }
            const float du = u - u0, dv = v - v0;
            if (!(du * du + dv * dv <= C2M_FLOW_MAX_STEP2)) { u = u0; v = v0; } // further than 8 px (or NaN): back to the initial flow
        }
        const float J = fl_sample(B, h, w, (float)x + u, (float)y + v);
        const float mJ = mean(wave_sum_all(part(J)));
        if (lane == 0) {
            float* __restrict__ o = p.rec + i * (G ? 4 : 3);
            o[0] = u; o[1] = v; o[2] = mJ - mT;
            if constexpr (G) o[3] = cnt;
        }
    }
}

// ids NULL: the unguided search (records of 3 floats); else the guided one (4 floats)
static int fl_patch_search(const float* ia, const float* ib, long image_elems, const float* init, long init_elems, int init_shift,
                           float* records, long record_elems, int N, int h, int w, int iters, const int32_t* ids, int level,
                           int H, int W, void* stream) {
    if (!fl_level_ok(N, h, w) || iters < 0 || iters > C2M_FLOW_MAX_ITERS || init_shift < 0 || init_shift > 1)
        return (int)hipErrorInvalidValue;
    if (N == 0) return 0;
    FlPsP p;
    p.ia = ia; p.ib = ib; p.init = init; p.rec = records;
    p.h = h; p.w = w; p.npy = fl_patches(h); p.npx = fl_patches(w);
    p.hc = (h + (1 << init_shift) - 1) >> init_shift; p.wc = (w + (1 << init_shift) - 1) >> init_shift;
    p.shift = init_shift; p.iters = iters;
    p.waves = (long)N * p.npy * p.npx;
    if (!ia || !ib || !records || image_elems < (long)N * h * w || record_elems < p.waves * (ids ? 4 : 3) ||
        (init && init_elems < 2L * N * p.hc * p.wc) || !c2m_aligned(4, ia, ib, init, records))
        return (int)hipErrorInvalidValue;
    const FlSegP g = {ids, level, W, (long)H * W};
    const dim3 grid(c2m_grid(p.waves * 64, 256));
    if (ids) hipLaunchKernelGGL(fl_patch_search_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p, g);
    else hipLaunchKernelGGL(fl_patch_search_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p, g);
    return (int)hipGetLastError();
}

C2M_API int c2m_flow_patch_search(const float* ia, const float* ib, long image_elems, const float* init, long init_elems,
                                  int init_shift, float* records, long record_elems, int N, int h, int w, int iters, void* stream) {
    C2M_ENTER();
    return fl_patch_search(ia, ib, image_elems, init, init_elems, init_shift, records, record_elems, N, h, w, iters, nullptr, 0, 0,
                           0, stream);
}

C2M_API int c2m_flow_patch_search_guided(const float* ia, const float* ib, long image_elems, const float* init, long init_elems,
                                         int init_shift, float* records, long record_elems, int N, int h, int w, int iters,
                                         const int32_t* segments, long segment_elems, int level, int H, int W, void* stream) {
    C2M_ENTER();
    if (!fl_level_ok(N, h, w) || !fl_seg_ok(segments, segment_elems, N, level, H, W, h, w)) return (int)hipErrorInvalidValue;
    return fl_patch_search(ia, ib, image_elems, init, init_elems, init_shift, records, record_elems, N, h, w, iters, segments,
                           level, H, W, stream);
}

// ------------------------------------------------------------------------------------------------ densify
struct FlDnP {
    const float* ia; const float* ib; const float* rec; float* out;
    int h, w, npy, npx, shift, Ho, Wo;
    float scale;
    long total;                                                                 // N * Ho * Wo
};

template <bool G>
__global__ __launch_bounds__(256) void fl_densify_kernel(const FlDnP p, const FlSegP g) {
    const int h = p.h, w = p.w;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < p.total; i += (long)gridDim.x * blockDim.x) {
        const int X = (int)(i % p.Wo);
        const long t = i / p.Wo;
        const int Y = (int)(t % p.Ho);
        const long n = t / p.Ho;
        const int x = X >> p.shift, y = Y >> p.shift;                           // < w, h: checked by the launcher
        const float* __restrict__ A = p.ia + n * ((long)h * w);
        const float* __restrict__ B = p.ib + n * ((long)h * w);
        constexpr int RW = G ? 4 : 3;
        const float* __restrict__ R = p.rec + n * RW * ((long)p.npy * p.npx);
        const float T = A[(long)y * w + x];
        int id = 0;
        if constexpr (G) id = g.at(n, y, x);
        // a patch of index j has its origin at min(4 j, n - 8): the indices whose 8 pixels can hold y are ceil((y - 7) / 4) ..
        // y / 4 + 1 (the last, clamped, patch); the test against the origin picks the <= 3 that do
        const int jy0 = y < 4 ? 0 : (y - 4) >> 2, jy1 = min((y >> 2) + 1, p.npy - 1);
        const int jx0 = x < 4 ? 0 : (x - 4) >> 2, jx1 = min((x >> 2) + 1, p.npx - 1);
        float su = 0.f, sv = 0.f, sw = 0.f;
        float au = 0.f, av = 0.f, aw = 0.f;                                     // guided: over ALL covering patches, the fall-back
        bool own = false;                                                       // guided: a covering patch has this pixel's id
        for (int jy = jy0; jy <= jy1; ++jy) {                                   // ascending (oy, ox): the order of the sum is fixed
            const int oy = min(C2M_FLOW_STRIDE * jy, h - C2M_FLOW_PATCH);
            if (y < oy || y > oy + C2M_FLOW_PATCH - 1) continue;
            for (int jx = jx0; jx <= jx1; ++jx) {
                const int ox = min(C2M_FLOW_STRIDE * jx, w - C2M_FLOW_PATCH);
                if (x < ox || x > ox + C2M_FLOW_PATCH - 1) continue;
                const float* __restrict__ q = R + RW * ((long)jy * p.npx + jx);
                const float u = q[0], v = q[1], d = q[2];
                const float r = (fl_sample(B, h, w, (float)x + u, (float)y + v) - T) - d;
                if constexpr (G) {
                    const float wgt = q[3] / fmaxf(1.f, fabsf(r));
                    au += wgt * u; av += wgt * v; aw += wgt;
                    if (g.at(n, oy + 3, ox + 3) == id) { su += wgt * u; sv += wgt * v; sw += wgt; own = true; }
                } else {
                    const float wgt = 1.f / fmaxf(1.f, fabsf(r));
                    su += wgt * u; sv += wgt * v; sw += wgt;
                }
            }
        }
        if constexpr (G) {
            if (!own) { su = au; sv = av; sw = aw; }                            // e.g. a structure thinner than a stride
        }
        float* __restrict__ o = p.out + n * 2 * ((long)p.Ho * p.Wo) + (long)Y * p.Wo + X;
        o[0] = p.scale * (su / sw);                                             // sw > 0: every pixel is covered (h, w >= 8)
        o[(long)p.Ho * p.Wo] = p.scale * (sv / sw);
    }
}

static int fl_densify(const float* ia, const float* ib, long image_elems, const float* records, long record_elems, float* flow,
                      long flow_elems, int N, int h, int w, int shift, int Ho, int Wo, const int32_t* ids, int level, int H, int W,
                      void* stream) {
    if (!fl_level_ok(N, h, w) || shift < 0 || shift >= C2M_FLOW_MAX_LEVELS || Ho < 1 || Wo < 1 || Ho > C2M_FLOW_MAX_SIDE ||
        Wo > C2M_FLOW_MAX_SIDE || ((Ho - 1) >> shift) >= h || ((Wo - 1) >> shift) >= w)
        return (int)hipErrorInvalidValue;
    if (N == 0) return 0;
    FlDnP p;
    p.ia = ia; p.ib = ib; p.rec = records; p.out = flow;
    p.h = h; p.w = w; p.npy = fl_patches(h); p.npx = fl_patches(w); p.shift = shift; p.Ho = Ho; p.Wo = Wo;
    p.scale = (float)(1 << shift);
    p.total = (long)N * Ho * Wo;
    if (!ia || !ib || !records || !flow || image_elems < (long)N * h * w ||
        record_elems < (ids ? 4L : 3L) * N * p.npy * p.npx || flow_elems < 2 * p.total || !c2m_aligned(4, ia, ib, records, flow))
        return (int)hipErrorInvalidValue;
    const FlSegP g = {ids, level, W, (long)H * W};
    const dim3 grid(c2m_grid(p.total, 256));
    if (ids) hipLaunchKernelGGL(fl_densify_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p, g);
    else hipLaunchKernelGGL(fl_densify_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p, g);
    return (int)hipGetLastError();
}

C2M_API int c2m_flow_densify(const float* ia, const float* ib, long image_elems, const float* records, long record_elems,
                             float* flow, long flow_elems, int N, int h, int w, int shift, int Ho, int Wo, void* stream) {
    C2M_ENTER();
    return fl_densify(ia, ib, image_elems, records, record_elems, flow, flow_elems, N, h, w, shift, Ho, Wo, nullptr, 0, 0, 0, stream);
}

C2M_API int c2m_flow_densify_guided(const float* ia, const float* ib, long image_elems, const float* records, long record_elems,
                                    float* flow, long flow_elems, int N, int h, int w, int shift, int Ho, int Wo,
                                    const int32_t* segments, long segment_elems, int level, int H, int W, void* stream) {
    C2M_ENTER();
    if (!fl_level_ok(N, h, w) || !fl_seg_ok(segments, segment_elems, N, level, H, W, h, w)) return (int)hipErrorInvalidValue;
    return fl_densify(ia, ib, image_elems, records, record_elems, flow, flow_elems, N, h, w, shift, Ho, Wo, segments, level, H, W,
                      stream);
}

// ------------------------------------------------------------------------------------------------ block-matching seed
// fl_patch_match_kernel (tests/flow_seed_np.py restates it): the start of the coarsest level's search for fast
// motion.  One wave per patch, the patches and the loop of fl_patch_search_kernel.  A patch tries every integer displacement
// (dx, dy) in [-R, R]^2 whose 8 x 8 window lies wholly inside b's level, 0 <= ox + dx <= w - 8 and 0 <= oy + dy <= h - 8, and
// takes the one with the smallest key (cost, dx^2 + dy^2, dy, dx): a total order, so the choice does not depend on which lane
// held which candidate.  cost = sum(((J - mJ) - Tm)^2) with mJ = sum(J) / 64; BOTH SUMS RUN OVER THE 64 PIXELS IN RASTER ORDER
// (py-major), one term after the other, from 0.f.  T, gx, gy, mean(T), Tm and det are those of the search (the same
// wave_sum_all); a patch with det <= its threshold has the one candidate (0, 0).  Guided: the sums run over the pixels with the
// id of the patch centre (the others add 0.f), means divide by n, the record carries n.  Record: (dx, dy, mJ - mean(T)).
//
// LDS, private to a wave: Tm [64] and the (8 + 2 R)^2 window of b around the patch, row stride 8 + 2 R: (64 + 24 * 24) floats
// = 2560 B a wave, 10 KB a workgroup.  Lane k evaluates the candidates k, k + 64, ... of the (2 R + 1)^2 (dy-major); the lanes
// of a wave read window cells one apart (a 2-way bank conflict where a candidate row wraps: R = 4 reads 9 cells a row of 16),
// Tm[k] is one address for all lanes (a broadcast).  The loop is workgroup-uniform (a wave past the last patch stages and
// computes nothing) so that the two barriers of an item are reached by all four waves.
#define C2M_FLOW_MATCH_MAX_R 8
#define C2M_FLOW_MATCH_SIDE (C2M_FLOW_PATCH + 2 * C2M_FLOW_MATCH_MAX_R)
#define C2M_FLOW_MATCH_LDS (64 + C2M_FLOW_MATCH_SIDE * C2M_FLOW_MATCH_SIDE)

struct FlPmP {
    const float* ia; const float* ib; float* rec;
    int h, w, npy, npx, R;
    long waves;                                                                 // N * npy * npx: one wave each
};

template <bool G>
__global__ __launch_bounds__(256) void fl_patch_match_kernel(const FlPmP p, const FlSegP g) {
    __shared__ float lds[4 * C2M_FLOW_MATCH_LDS];
    const int lane = threadIdx.x & 63, py = lane >> 3, px = lane & 7;
    const int h = p.h, w = p.w, R = p.R, D = 2 * R + 1, S = C2M_FLOW_PATCH + 2 * R;
    float* __restrict__ tm = lds + (threadIdx.x >> 6) * C2M_FLOW_MATCH_LDS;
    float* __restrict__ win = tm + 64;
    const long nwaves = (long)gridDim.x * 4;
    for (long base = (long)blockIdx.x * 4; base < p.waves; base += nwaves) {                      // workgroup-uniform
        const long i = base + (threadIdx.x >> 6);
        const bool live = i < p.waves;                                          // wave-uniform
        int ox = 0, oy = 0;
        long n = 0;
        bool in = true, ok = false;
        float cnt = 64.f, mT = 0.f;
        __syncthreads();                                                        // the previous item's LDS has been read
        if (live) {
            const int jx = (int)(i % p.npx);
            const long t = i / p.npx;
            const int jy = (int)(t % p.npy);
            n = t / p.npy;
            ox = min(C2M_FLOW_STRIDE * jx, w - C2M_FLOW_PATCH); oy = min(C2M_FLOW_STRIDE * jy, h - C2M_FLOW_PATCH);
            const int x = ox + px, y = oy + py;                                 // inside the image: ox + 7 <= w - 1
            const float* __restrict__ A = p.ia + n * ((long)h * w);
            const float* __restrict__ B = p.ib + n * ((long)h * w);
            const float* __restrict__ row = A + (long)y * w;
            const float T = row[x];
            const float gx = 0.5f * (row[min(x + 1, w - 1)] - row[max(x - 1, 0)]);
            const float gy = 0.5f * (A[(long)min(y + 1, h - 1) * w + x] - A[(long)max(y - 1, 0) * w + x]);
            float det_min = C2M_FLOW_DET_MIN;
            if constexpr (G) {
                in = g.at(n, y, x) == g.at(n, oy + 3, ox + 3);
                const int k = wave_count(in);
                cnt = (float)k;
                det_min = C2M_FLOW_DET_MIN * ((float)(k * k) / 4096.f);
            }
            auto part = [&](float v) { if constexpr (G) return in ? v : 0.f; else return v; };
            mT = wave_sum_all(part(T));
            if constexpr (G) mT = mT / cnt; else mT = mT * 0.015625f;
            const float a = wave_sum_all(part(gx * gx)), b = wave_sum_all(part(gx * gy)), c = wave_sum_all(part(gy * gy));
            ok = a * c - b * b > det_min;                                       // wave-uniform: every lane holds lane 0's sums
            tm[lane] = T - mT;
            // the window cell (wy, wx) is b's pixel (oy - R + wy, ox - R + wx).  NO COORDINATE IS CLAMPED: a cell outside the image
            // is neither loaded nor, below, read, because a candidate whose window is not wholly inside the image is skipped
            for (int q = lane; q < S * S; q += 64) {
                const int wy = q / S, wx = q - wy * S, by = oy - R + wy, bx = ox - R + wx;
                if (by >= 0 && by < h && bx >= 0 && bx < w) win[q] = B[(long)by * w + bx];
            }
        }
        __syncthreads();
        if (!live) continue;                                                    // workgroup-uniform loop: the barriers are above
        const unsigned long long members = G ? __ballot(in) : ~0ull;            // wave-uniform: bit k = pixel k carries the sums
        float best = INFINITY, best_mj = 0.f;
        int tie = INT_MAX;                                                      // (dx^2 + dy^2) << 10 | (dy + 8) << 5 | (dx + 8)
        for (int cand = lane; cand < D * D; cand += 64) {
            const int dy = cand / D - R, dx = cand - (dy + R) * D - R;
            if (ox + dx < 0 || ox + dx > w - C2M_FLOW_PATCH || oy + dy < 0 || oy + dy > h - C2M_FLOW_PATCH) continue;
            if (!ok && (dx | dy) != 0) continue;                                // det <= threshold: (0, 0) alone
            // rows dy + R .. dy + R + 7 and columns dx + R .. dx + R + 7 of the window: inside [0, S) since |dx|, |dy| <= R,
            // and cells that were loaded, since the displaced patch is inside the image
            const float* __restrict__ J = win + (dy + R) * S + (dx + R);
            float sj = 0.f;
            for (int k = 0; k < 64; ++k) {                                      // raster order
                const float v = J[(k >> 3) * S + (k & 7)];
                if constexpr (G) sj += ((members >> k) & 1) ? v : 0.f; else sj += v;
            }
            float mj;
            if constexpr (G) mj = sj / cnt; else mj = sj * 0.015625f;
            float cost = 0.f;
            for (int k = 0; k < 64; ++k) {                                      // raster order
                const float d = (J[(k >> 3) * S + (k & 7)] - mj) - tm[k];
                if constexpr (G) cost += ((members >> k) & 1) ? d * d : 0.f; else cost += d * d;
            }
            if (!(cost < INFINITY)) cost = INFINITY;                            // a NaN or an overflow: never below another cost
            const int key = ((dx * dx + dy * dy) << 10) | ((dy + 8) << 5) | (dx + 8);
            if (cost < best || (cost == best && key < tie)) { best = cost; tie = key; best_mj = mj; }
        }
        wave_min_key_all(best, tie, best_mj);                                   // (0, 0) is always a candidate: tie < INT_MAX
        if (lane == 0) {
            float* __restrict__ o = p.rec + i * (G ? 4 : 3);
            o[0] = (float)((tie & 31) - 8); o[1] = (float)(((tie >> 5) & 31) - 8); o[2] = best_mj - mT;
            if constexpr (G) o[3] = cnt;
        }
    }
}

// ids NULL: the unguided match (records of 3 floats); else the guided one (4 floats)
static int fl_patch_match(const float* ia, const float* ib, long image_elems, float* records, long record_elems, int N, int h,
                          int w, int radius, const int32_t* ids, int level, int H, int W, void* stream) {
    if (!fl_level_ok(N, h, w) || radius < 1 || radius > C2M_FLOW_MATCH_MAX_R) return (int)hipErrorInvalidValue;
    if (N == 0) return 0;
    FlPmP p;
    p.ia = ia; p.ib = ib; p.rec = records;
    p.h = h; p.w = w; p.npy = fl_patches(h); p.npx = fl_patches(w); p.R = radius;
    p.waves = (long)N * p.npy * p.npx;
    if (!ia || !ib || !records || image_elems < (long)N * h * w || record_elems < p.waves * (ids ? 4 : 3) ||
        !c2m_aligned(4, ia, ib, records))
        return (int)hipErrorInvalidValue;
    const FlSegP g = {ids, level, W, (long)H * W};
    const dim3 grid(c2m_grid(p.waves * 64, 256));
    if (ids) hipLaunchKernelGGL(fl_patch_match_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p, g);
    else hipLaunchKernelGGL(fl_patch_match_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p, g);
    return (int)hipGetLastError();
}

C2M_API int c2m_flow_patch_match(const float* ia, const float* ib, long image_elems, float* records, long record_elems, int N,
                                 int h, int w, int radius, void* stream) {
    C2M_ENTER();
    return fl_patch_match(ia, ib, image_elems, records, record_elems, N, h, w, radius, nullptr, 0, 0, 0, stream);
}

C2M_API int c2m_flow_patch_match_guided(const float* ia, const float* ib, long image_elems, float* records, long record_elems,
                                        int N, int h, int w, int radius, const int32_t* segments, long segment_elems, int level,
                                        int H, int W, void* stream) {
    C2M_ENTER();
    if (!fl_level_ok(N, h, w) || !fl_seg_ok(segments, segment_elems, N, level, H, W, h, w)) return (int)hipErrorInvalidValue;
    return fl_patch_match(ia, ib, image_elems, records, record_elems, N, h, w, radius, segments, level, H, W, stream);
}
