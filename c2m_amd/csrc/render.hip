// Rendering of results as uint8 sheets (gfx950): frames, occlusion maps, flows in the Middlebury colour code, instance
// overlays, boxes and drag paths.  Replaces the reference's CPU numpy layer (utils/utils.py tensor2im, tensor2occ, tensor2flow,
// save_flows, draw_bbox; utils/ops.py compute_color, flow2img, get_edges).
//
// A sheet is uint8 [T, rows*H, cols*W, C] (HWC); sample b sits in cell (b / cols, b % cols) (the reference's merge).  A thread
// owns VEC consecutive pixels of one row of one cell: it reads 4*VEC*C bytes per plane-aligned vector load and writes VEC*C
// contiguous bytes as 32-bit words (VEC = 4: W % 4 == 0, so the 12 bytes of an RGB group start on a word).  Nothing is
// accumulated except the per-frame radius maximum of the sheet-normalised flow mode (integer max on the bit pattern of a
// non-negative double: exact and order-independent), so every output is bit-repeatable.
//
// Number formats follow numpy's in the reference, operation by operation (this file is compiled with -ffp-contract=off):
//   frames / occlusion   float32 array * Python scalar stays float32 in numpy: x * 255 (or (x + 1) / 2 * 255) in fp32, clipped,
//                        truncated.  (For x * 255 a float64 product truncates to the same level for every float32 x -- checked
//                        exhaustively, tests/test_visual_cpu.py samples it -- so fp32 costs nothing in fidelity here.)
//   flows                float64 throughout.  For the sheet mode that is the reference exactly (merge() copies into a float64
//                        sheet).  compute_flow_color_map gets float32 frames, so numpy keeps u * 3, the radius, arctan2 and the
//                        wheel position in float32 there; its float32 arctan2 is not correctly rounded, so its last bit cannot
//                        be followed by any other implementation, and the double evaluation differs from it on 2e-5 of the
//                        pixels of a normal flow by one level.
#include "common.h"
#include "dtype.h"

struct Sheet { int B, T, H, W, rows, cols; };

// the Middlebury colour wheel: 55 entries in six ramps (15 red->yellow, 6 yellow->green, 4 green->cyan, 11 cyan->blue,
// 13 blue->magenta, 6 magenta->red), the moving channel floor(255 * i / n) up or down; stored as value / 255 in double
struct Wheel { double c[55][3]; };
static constexpr Wheel make_wheel() {
    Wheel w{};
    const int n[6] = {15, 6, 4, 11, 13, 6}, full[6] = {0, 1, 1, 2, 2, 0}, ramp[6] = {1, 0, 2, 1, 0, 2};
    int k = 0;
    for (int s = 0; s < 6; ++s)
        for (int i = 0; i < n[s]; ++i, ++k) {
            const int r = 255 * i / n[s];                     // floor: operands are non-negative
            w.c[k][full[s]] = 1.0;
            w.c[k][ramp[s]] = (s % 2 == 0 ? r : 255 - r) / 255.0;
        }
    return w;
}
__device__ const Wheel c2m_wheel = make_wheel();

__device__ __forceinline__ void load_wheel(double (*lds)[3]) {
    for (int i = threadIdx.x; i < 165; i += blockDim.x) (&lds[0][0])[i] = (&c2m_wheel.c[0][0])[i];
    __syncthreads();
}

// decode work item i -> (t, sheet row Y, cell column cc, first x of the group); returns the sample or -1 for an empty cell
template <int VEC>
__device__ __forceinline__ int sheet_item(const Sheet& s, long i, int& t, int& Y, int& y, int& cc, int& x0) {
    const int Wv = s.W / VEC;
    x0 = (int)(i % Wv) * VEC; i /= Wv;
    cc = (int)(i % s.cols); i /= s.cols;
    const int RH = s.rows * s.H;
    Y = (int)(i % RH); t = (int)(i / RH);
    y = Y % s.H;
    const int b = (Y / s.H) * s.cols + cc;
    return b < s.B ? b : -1;
}

__device__ __forceinline__ long sheet_pixel(const Sheet& s, int t, int Y, int cc, int x0) {
    return ((long)t * s.rows * s.H + Y) * ((long)s.cols * s.W) + (long)cc * s.W + x0;
}

// VEC pixels of C bytes, contiguous; VEC == 4: the group starts on a 32-bit word
template <int VEC, int C>
__device__ __forceinline__ void store_group(uint8_t* __restrict__ out, long pixel, const uint8_t (&v)[VEC * C]) {
    uint8_t* o = out + pixel * C;
    if constexpr (VEC == 4) {
#pragma unroll
        for (int w = 0; w < C; ++w)
            reinterpret_cast<uint32_t*>(o)[w] = (uint32_t)v[4 * w] | (uint32_t)v[4 * w + 1] << 8 | (uint32_t)v[4 * w + 2] << 16 |
                                                (uint32_t)v[4 * w + 3] << 24;
    } else {
#pragma unroll
        for (int e = 0; e < VEC * C; ++e) o[e] = v[e];
    }
}

template <typename T, int VEC>
__device__ __forceinline__ void load_group(const T* __restrict__ p, float (&v)[VEC]) {
    if constexpr (VEC == 4) { const float4 q = c2m_ld4(p); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    else v[0] = c2m_ld(p, 0);
}

// ------------------------------------------------------------------------------------------------ frames / occlusion maps
__device__ __forceinline__ uint8_t frame_level(float x, int normalize) {
    float v = normalize ? (x + 1.0f) / 2.0f * 255.0f : x * 255.0f;
    v = v < 255.0f ? v : 255.0f;                 // NaN -> 255 here, 0 on the next line
    return v > 0.0f && x == x ? (uint8_t)v : (uint8_t)0;
}

template <typename T, int VEC, int C>
__global__ __launch_bounds__(256) void render_frames_kernel(const T* __restrict__ x, uint8_t* __restrict__ out, const Sheet s,
                                                            int normalize, long items) {
    const long HW = (long)s.H * s.W;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < items; i += (long)gridDim.x * blockDim.x) {
        int t, Y, y, cc, x0;
        const int b = sheet_item<VEC>(s, i, t, Y, y, cc, x0);
        uint8_t v[VEC * C];
        if (b < 0) {
#pragma unroll
            for (int e = 0; e < VEC * C; ++e) v[e] = 0;
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float f[VEC];
                load_group<T, VEC>(x + (((long)b * C + c) * s.T + t) * HW + (long)y * s.W + x0, f);
#pragma unroll
                for (int e = 0; e < VEC; ++e) v[e * C + c] = frame_level(f[e], normalize);
            }
        }
        store_group<VEC, C>(out, sheet_pixel(s, t, Y, cc, x0), v);
    }
}

static inline bool sheet_ok(const Sheet& s) {
    return s.B >= 0 && s.T >= 0 && s.H >= 0 && s.W >= 0 && s.rows >= 0 && s.cols >= 0 && (long)s.B <= (long)s.rows * s.cols &&
           (long)s.rows * s.H < (1L << 31) && (long)s.cols * s.W < (1L << 31);
}
static inline long sheet_pixels(const Sheet& s) { return (long)s.T * s.rows * s.H * s.cols * s.W; }

C2M_API int c2m_render_frames(const void* x, int dt, int B, int C, int T, int H, int W, int rows, int cols, int normalize,
                              uint8_t* out, void* stream) {
    C2M_ENTER();
    const Sheet s{B, T, H, W, rows, cols};
    if (!sheet_ok(s) || (C != 1 && C != 3) || (dt != C2M_F32 && dt != C2M_BF16)) return (int)hipErrorInvalidValue;
    const long px = sheet_pixels(s);
    if (px == 0) return 0;
    if (!out || (B > 0 && !x)) return (int)hipErrorInvalidValue;
    const bool vec = W % 4 == 0 && c2m_aligned(4, out) && c2m_aligned(dt == C2M_BF16 ? 8 : 16, x);
    const long items = vec ? px / 4 : px;
    const dim3 grid(c2m_grid(items, 256));
    hipStream_t st = (hipStream_t)stream;
#define C2M_FRAMES(TT, VEC, CC) \
    hipLaunchKernelGGL((render_frames_kernel<TT, VEC, CC>), grid, dim3(256), 0, st, (const TT*)x, out, s, normalize, items)
    C2M_DISPATCH_DT(dt, {
        if (vec) { if (C == 3) C2M_FRAMES(T, 4, 3); else C2M_FRAMES(T, 4, 1); }
        else     { if (C == 3) C2M_FRAMES(T, 1, 3); else C2M_FRAMES(T, 1, 1); }
    });
#undef C2M_FRAMES
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------- flow
#define C2M_UNKNOWN_FLOW 1e7
#define C2M_PI 3.141592653589793

__device__ __forceinline__ double sqrt_rn(double x) { return __dsqrt_rn(x); }      // correctly rounded

// the colour rule on (u, v); NaN components -> black
typedef double F;
__device__ __forceinline__ void flow_colour(F u, F v, const double (*wheel)[3], uint8_t* rgb, int stride) {
    if (u != u || v != v) { rgb[0] = rgb[stride] = rgb[2 * stride] = 0; return; }
    const F rad = sqrt_rn(u * u + v * v);
    const F a = (F)atan2((double)-v, (double)-u) / (F)C2M_PI;
    const F fk = (a + (F)1) / (F)2 * (F)54 + (F)1;
    int k0 = (int)floor(fk);
    k0 = k0 < 1 ? 1 : (k0 > 55 ? 55 : k0);                      // a is in [-1, 1], so this only guards the table
    const int k1 = k0 == 55 ? 1 : k0 + 1;
    const double f = (double)fk - (double)k0;
    const bool inside = rad <= (F)1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double col = (1.0 - f) * wheel[k0 - 1][c] + f * wheel[k1 - 1][c];
        col = inside ? 1.0 - (double)rad * (1.0 - col) : col * 0.75;
        const double lv = floor(255.0 * col);
        rgb[c * stride] = (uint8_t)(lv < 0.0 ? 0.0 : (lv > 255.0 ? 255.0 : lv));
    }
}

__device__ __forceinline__ bool flow_unknown(double u, double v) { return fabs(u) > C2M_UNKNOWN_FLOW || fabs(v) > C2M_UNKNOWN_FLOW; }

// maxrad[t] = bit pattern of the largest radius over all samples of frame t (a NaN radius: the quiet-NaN pattern, which is
// larger than every number's).  Integer atomic max on a non-negative double: exact, any order.
template <typename T>
__global__ __launch_bounds__(256) void flow_maxrad_kernel(const T* __restrict__ x, unsigned long long* __restrict__ maxrad,
                                                          int B, int Tn, long HW) {
    const int t = blockIdx.y;
    double m = 0.0;
    int nan = 0;
    const long n = (long)B * HW;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long b = i / HW, p = i % HW;
        const T* q = x + ((b * 2) * Tn + t) * HW + p;
        double u = (double)c2m_ld(q, 0), v = (double)c2m_ld(q, (long)Tn * HW);
        if (flow_unknown(u, v)) u = v = 0.0;
        const double r = sqrt_rn(u * u + v * v);
        if (r != r) nan = 1; else m = r > m ? r : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double mo = __shfl_down(m, o, 64);
        nan |= __shfl_down(nan, o, 64);
        m = mo > m ? mo : m;
    }
    __shared__ unsigned long long part[4];                     // one atomic per workgroup: T addresses take every update
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = nan ? 0x7ff8000000000000ull : (unsigned long long)__double_as_longlong(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long bits = part[0];
        for (int w = 1; w < 4; ++w) bits = part[w] > bits ? part[w] : bits;
        if (bits) atomicMax(&maxrad[t], bits);
    }
}

// mode 0: sheet-normalised (flow2img), mode 1: fixed scale (compute_flow_color_map)
template <typename T, int VEC, int MODE>
__global__ __launch_bounds__(256) void render_flow_kernel(const T* __restrict__ x, uint8_t* __restrict__ out, const Sheet s,
                                                          const unsigned long long* __restrict__ maxrad_bits, float scale,
                                                          long items) {
    __shared__ double wheel[55][3];
    load_wheel(wheel);
    const long HW = (long)s.H * s.W;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < items; i += (long)gridDim.x * blockDim.x) {
        int t, Y, y, cc, x0;
        const int b = sheet_item<VEC>(s, i, t, Y, y, cc, x0);
        float fu[VEC], fv[VEC];
        if (b < 0) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) fu[e] = fv[e] = 0.0f;             // an empty cell holds zero FLOW
        } else {
            const T* q = x + (((long)b * 2) * s.T + t) * HW + (long)y * s.W + x0;
            load_group<T, VEC>(q, fu);
            load_group<T, VEC>(q + (long)s.T * HW, fv);
        }
        uint8_t v[VEC * 3];
        if constexpr (MODE == 0) {
            double maxrad = __longlong_as_double((long long)maxrad_bits[t]);
            if (maxrad != maxrad) maxrad = -1.0;                            // Python's max(-1, nan) is -1
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                double u = (double)fu[e], w = (double)fv[e];
                const bool unknown = flow_unknown(u, w);
                if (unknown) u = w = 0.0;
                u = u / maxrad + 2.220446049250313e-16;
                w = w / maxrad + 2.220446049250313e-16;
                flow_colour(u, w, wheel, &v[e * 3], 1);
                if (unknown) v[e * 3] = v[e * 3 + 1] = v[e * 3 + 2] = 0;
            }
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) flow_colour((double)fu[e] * (double)scale, (double)fv[e] * (double)scale, wheel, &v[e * 3], 1);
        }
        store_group<VEC, 3>(out, sheet_pixel(s, t, Y, cc, x0), v);
    }
}

C2M_API long c2m_render_flow_workspace_bytes(int T) { return T > 0 ? 8L * T : 0L; }

C2M_API int c2m_render_flow(const void* flow, int dt, int B, int T, int H, int W, int rows, int cols, int mode, float scale,
                            uint8_t* out, void* workspace, void* stream) {
    C2M_ENTER();
    const Sheet s{B, T, H, W, rows, cols};
    if (!sheet_ok(s) || (mode != 0 && mode != 1) || (dt != C2M_F32 && dt != C2M_BF16)) return (int)hipErrorInvalidValue;
    const long px = sheet_pixels(s);
    if (px == 0) return 0;
    if (!out || (B > 0 && !flow) || (mode == 0 && (!workspace || !c2m_aligned(8, workspace)))) return (int)hipErrorInvalidValue;
    const bool vec = W % 4 == 0 && c2m_aligned(4, out) && c2m_aligned(dt == C2M_BF16 ? 8 : 16, flow);
    const long items = vec ? px / 4 : px;
    const dim3 grid(c2m_grid(items, 256));
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* mr = (unsigned long long*)workspace;
    if (mode == 0) {
        hipError_t e = c2m_zero_async(mr, 8L * T, st);
        if (e != hipSuccess) return (int)e;
        const long HW = (long)H * W;
        if (B > 0) {
            long gx = ((long)B * HW + 255) / 256;
            gx = gx > 128 ? 128 : gx;
            const dim3 rg((unsigned)gx, (unsigned)T);
            C2M_DISPATCH_DT(dt, { hipLaunchKernelGGL((flow_maxrad_kernel<T>), rg, dim3(256), 0, st, (const T*)flow, mr, B, s.T, HW); });
            C2M_LAUNCH_CHECK();
        }
    }
#define C2M_FLOW(TT, VEC, MODE) \
    hipLaunchKernelGGL((render_flow_kernel<TT, VEC, MODE>), grid, dim3(256), 0, st, (const TT*)flow, out, s, mr, scale, items)
    C2M_DISPATCH_DT(dt, {
        if (vec) { if (mode == 0) C2M_FLOW(T, 4, 0); else C2M_FLOW(T, 4, 1); }
        else     { if (mode == 0) C2M_FLOW(T, 1, 0); else C2M_FLOW(T, 1, 1); }
    });
#undef C2M_FLOW
    return (int)hipGetLastError();
}

// -------------------------------------------------------------------------------------------------------------- instances
struct InstP {
    const int32_t* ids; const uint8_t* base; uint8_t* out; const uint8_t* palette;
    int P, lo, hi, alpha;
};

__device__ __forceinline__ bool in_range(int id, const InstP& p) { return id >= p.lo && id < p.hi; }

template <int VEC>
__global__ __launch_bounds__(256) void render_instances_kernel(const InstP p, const Sheet s, long items) {
    const long HW = (long)s.H * s.W;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < items; i += (long)gridDim.x * blockDim.x) {
        int t, Y, y, cc, x0;
        const int b = sheet_item<VEC>(s, i, t, Y, y, cc, x0);
        const long pixel = sheet_pixel(s, t, Y, cc, x0);
        uint8_t v[VEC * 3];
        if (VEC == 4 && p.base) {                                           // 12 contiguous bytes on a word boundary
            const uint32_t* q = reinterpret_cast<const uint32_t*>(p.base + pixel * 3);
#pragma unroll
            for (int w = 0; w < 3; ++w) {
                const uint32_t r = q[w];
                v[4 * w] = (uint8_t)r; v[4 * w + 1] = (uint8_t)(r >> 8); v[4 * w + 2] = (uint8_t)(r >> 16); v[4 * w + 3] = (uint8_t)(r >> 24);
            }
        } else {
#pragma unroll
            for (int e = 0; e < VEC * 3; ++e) v[e] = p.base ? p.base[pixel * 3 + e] : (uint8_t)0;
        }
        if (b >= 0) {
            const int32_t* row = p.ids + ((long)b * s.T + t) * HW + (long)y * s.W;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const int x = x0 + e, id = row[x];
                int m = id;                                             // the largest id among the pixel and its 4 neighbours
                if (x > 0) m = max(m, row[x - 1]);
                if (x + 1 < s.W) m = max(m, row[x + 1]);
                if (y > 0) m = max(m, row[x - s.W]);
                if (y + 1 < s.H) m = max(m, row[x + s.W]);
                bool edge = (x > 0 && row[x - 1] != id) || (x + 1 < s.W && row[x + 1] != id) || (y > 0 && row[x - s.W] != id) ||
                            (y + 1 < s.H && row[x + s.W] != id);
                if (edge && in_range(m, p)) {
                    const uint8_t* c = p.palette + (m % p.P) * 3;
                    v[e * 3] = c[0]; v[e * 3 + 1] = c[1]; v[e * 3 + 2] = c[2];
                } else if (in_range(id, p)) {
                    const uint8_t* c = p.palette + (id % p.P) * 3;
#pragma unroll
                    for (int k = 0; k < 3; ++k) v[e * 3 + k] = (uint8_t)(((int)v[e * 3 + k] * (256 - p.alpha) + (int)c[k] * p.alpha) >> 8);
                }
            }
        }
        store_group<VEC, 3>(p.out, pixel, v);
    }
}

C2M_API int c2m_render_instances(const int32_t* ids, int B, int T, int H, int W, int rows, int cols, const uint8_t* base,
                                 const uint8_t* palette, int P, int id_lo, int id_hi, int alpha, uint8_t* out, void* stream) {
    C2M_ENTER();
    const Sheet s{B, T, H, W, rows, cols};
    if (!sheet_ok(s) || P < 1 || alpha < 0 || alpha > 256 || id_lo < 0) return (int)hipErrorInvalidValue;   // ids in range are >= 0: % is plain
    const long px = sheet_pixels(s);
    if (px == 0) return 0;
    if (!out || !palette || (B > 0 && !ids)) return (int)hipErrorInvalidValue;
    const InstP p{ids, base, out, palette, P, id_lo, id_hi, alpha};
    const bool vec = W % 4 == 0 && c2m_aligned(4, out, base);
    const long items = vec ? px / 4 : px;
    const dim3 grid(c2m_grid(items, 256));
    if (vec) hipLaunchKernelGGL((render_instances_kernel<4>), grid, dim3(256), 0, (hipStream_t)stream, p, s, items);
    else hipLaunchKernelGGL((render_instances_kernel<1>), grid, dim3(256), 0, (hipStream_t)stream, p, s, items);
    return (int)hipGetLastError();
}

// --------------------------------------------------------------------------------------------------------------- overlays
#define C2M_OVERLAY_MAX_BOXES 64

struct OverlayP {
    uint8_t* sheet;
    const int32_t* boxes; const uint8_t* presence; const uint8_t* box_rgb; int N;          // [B,N,T,4], [B,N,T], [B,N,3]
    const int32_t* points; const int32_t* sample; const int32_t* count; const uint8_t* line_rgb; int D, P;   // [D,P,2], [D], [D,T], [D,3]
};

__device__ __forceinline__ long long floordiv(long long a, long long b) {      // b > 0
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// does the segment a -> b cover (x, y)?  n = max(|dx|, |dy|); step i = 0..n along the major axis (x when |dx| >= |dy|), the
// minor coordinate is a_minor + floor((2 * i * d_minor + n) / (2 * n)); n = 0: the single point
__device__ __forceinline__ bool segment_covers(int ax, int ay, int bx, int by, int x, int y) {
    const long long dx = (long long)bx - ax, dy = (long long)by - ay;
    const long long adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
    const long long n = adx > ady ? adx : ady;
    if (n == 0) return x == ax && y == ay;
    if (adx >= ady) {
        const long long i = dx > 0 ? (long long)x - ax : (long long)ax - x;
        return i >= 0 && i <= n && (long long)y == ay + floordiv(2 * i * dy + n, 2 * n);
    }
    const long long i = dy > 0 ? (long long)y - ay : (long long)ay - y;
    return i >= 0 && i <= n && (long long)x == ax + floordiv(2 * i * dx + n, 2 * n);
}

// Gather form: one thread per pixel of one cell walks the cell's primitives in order (boxes by node, then polylines by index,
// each line before its marker) and keeps the last one that covers the pixel; pixels nothing covers are not written.
// blockIdx.y = t * B + b.  The present boxes of (b, t) are compacted into LDS once per workgroup.
__global__ __launch_bounds__(256) void draw_overlays_kernel(const OverlayP p, const Sheet s) {
    __shared__ int box[C2M_OVERLAY_MAX_BOXES][4];
    __shared__ uint32_t box_col[C2M_OVERLAY_MAX_BOXES];
    __shared__ int nbox;
    const int t = blockIdx.y / s.B, b = blockIdx.y % s.B;
    if (threadIdx.x < 64) {                                       // wave 0: ordered compaction of the present boxes
        const int n = threadIdx.x;
        const bool present = n < p.N && p.presence[((long)b * p.N + n) * s.T + t] != 0;
        int shown;
        const int k = wave_rank(present, shown);
        if (present) {
            const int32_t* q = p.boxes + (((long)b * p.N + n) * s.T + t) * 4;
            box[k][0] = q[0]; box[k][1] = q[1]; box[k][2] = q[2]; box[k][3] = q[3];
            const uint8_t* c = p.box_rgb + ((long)b * p.N + n) * 3;
            box_col[k] = (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16;
        }
        if (n == 0) nbox = shown;
    }
    __syncthreads();
    const int HW = s.H * s.W;                                     // a cell: below 2^31 pixels (checked by the host)
    const long cell = sheet_pixel(s, t, (b / s.cols) * s.H, b % s.cols, 0);
    const long pitch = (long)s.cols * s.W;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += gridDim.x * blockDim.x) {
        const int y = i / s.W, x = i % s.W;
        uint32_t col = 0;
        bool hit = false;
        for (int k = 0; k < nbox; ++k) {
            const int x0 = box[k][0], y0 = box[k][1], x1 = box[k][2] - 1, y1 = box[k][3] - 1;
            if (x >= x0 && x <= x1 && y >= y0 && y <= y1 && (x == x0 || x == x1 || y == y0 || y == y1)) { col = box_col[k]; hit = true; }
        }
        for (int d = 0; d < p.D; ++d) {
            if (p.sample[d] != b) continue;
            int cnt = p.count[(long)d * s.T + t];
            cnt = cnt > p.P ? p.P : cnt;
            if (cnt <= 0) continue;
            const int32_t* q = p.points + (long)d * p.P * 2;
            bool on = false;
            for (int j = 0; j + 1 < cnt && !on; ++j) on = segment_covers(q[2 * j], q[2 * j + 1], q[2 * j + 2], q[2 * j + 3], x, y);
            const long long mx = (long long)x - q[2 * cnt - 2], my = (long long)y - q[2 * cnt - 1];
            on = on || (mx >= -1 && mx <= 1 && my >= -1 && my <= 1);           // 3x3 marker on the last shown point
            if (on) {
                const uint8_t* c = p.line_rgb + (long)d * 3;
                col = (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16;
                hit = true;
            }
        }
        if (hit) {
            uint8_t* o = p.sheet + (cell + (long)y * pitch + x) * 3;
            o[0] = (uint8_t)col; o[1] = (uint8_t)(col >> 8); o[2] = (uint8_t)(col >> 16);
        }
    }
}

C2M_API int c2m_draw_overlays_max_boxes(void) { return C2M_OVERLAY_MAX_BOXES; }

C2M_API int c2m_draw_overlays(uint8_t* sheet, int B, int T, int H, int W, int rows, int cols, const int32_t* boxes,
                              const uint8_t* presence, const uint8_t* box_rgb, int N, const int32_t* points, const int32_t* sample,
                              const int32_t* count, const uint8_t* line_rgb, int D, int P, void* stream) {
    C2M_ENTER();
    const Sheet s{B, T, H, W, rows, cols};
    if (!sheet_ok(s) || N < 0 || N > C2M_OVERLAY_MAX_BOXES || D < 0 || P < 0 || (long)H * W >= (1L << 31) || (long)B * T >= 65536)
        return (int)hipErrorInvalidValue;
    if (D > 0 && P == 0) D = 0;
    if (sheet_pixels(s) == 0 || B == 0 || (N == 0 && D == 0)) return 0;
    if (!sheet || (N > 0 && (!boxes || !presence || !box_rgb)) || (D > 0 && (!points || !sample || !count || !line_rgb)))
        return (int)hipErrorInvalidValue;
    const OverlayP p{sheet, boxes, presence, box_rgb, N, points, sample, count, line_rgb, D, P};
    long gx = ((long)H * W + 255) / 256;
    gx = gx > 64 ? 64 : gx;
    hipLaunchKernelGGL(draw_overlays_kernel, dim3((unsigned)gx, (unsigned)(B * T)), dim3(256), 0, (hipStream_t)stream, p, s);
    return (int)hipGetLastError();
}
