// Connected components of key maps, and instance ids from semantic label maps (gfx950), for N images per call.
//
// The operator (c2m_connected_components): two pixels belong to one component when they are 4- or 8-neighbours and carry the same
// key; there is no background.  The label of a pixel is the linear index y * W + x of its component's first pixel in raster order,
// so the result is a function of the input alone.  Block-local labelling, then a merge across the tile seams:
//
//   cc_tile_kernel     one workgroup per 64 x 16 tile, keys and one label per pixel in LDS.  Labels start at the pixel's index in
//                      the tile; a pass takes the minimum over the equal-key neighbours inside the tile and lowers the label of the
//                      pixel's current root to it (LDS atomicMin), then every pixel jumps to its root; passes repeat until one
//                      lowers nothing.  parent[p] = the image index of the tile-local root (<= p).
//   cc_seam_kernel     one thread per pixel on the left side of a vertical seam or the upper side of a horizontal one: union with
//                      the equal-key neighbours across (for 8-connectivity the two diagonals as well, which covers both diagonals
//                      of a corner where four tiles meet).  Lock-free union by minimum index on `parent`.
//   cc_flatten_kernel  a launch of its own (the launch boundary is the grid-wide ordering): label[p] = the root reached from p.
//
// Union by minimum keeps parent[i] <= i always, and the root of a finished component is its smallest index whatever order the
// unions took.  NO THREAD EVER WAITS FOR ANOTHER ONE'S WRITE: every loop below walks a value that strictly decreases and states
// its bound.  The seam kernel reads `parent` -- written by other CUs during the same launch -- through agent-scope relaxed atomic
// loads only (a CU's vector L1 is never refreshed by another CU's stores); a stale value is an earlier ancestor of the same
// component, never a wrong one, and progress comes from what atomicMin returns (it executes at the memory side), never from
// reading a location again until it changes.
//
// Instances (c2m_semantic_instances): components of the label map itself, then for the thing classes
//   si_area_kernel     area[root] += 1 per thing pixel (int32 atomics into a zeroed plane: exact, repeatable)
//   si_count_kernel    per chunk of 1024 consecutive raster pixels and per thing class, the number of roots with area >= min_area
//   si_scan_kernel     one workgroup per image: exclusive prefix of those counts along the chunks, per class; count and dropped
//   si_assign_kernel   per chunk: the n-th qualifying root of a class in raster order (block_rank_256 inside the chunk + the
//                      prefix) gets class * label_divisor + n while n < label_divisor, else the class; so do roots below
//                      min_area; pixels of other classes get their label
//   si_paint_kernel    every other thing pixel copies the value of its root
// Integer atomics only; every word of the workspace that is read was written by the same call.
#include "common.h"

#define C2M_CC_TW 64                           // tile: 64 x 16 pixels, 256 threads, 4 pixels each (rows w, w + 4, w + 8, w + 12)
#define C2M_CC_TH 16
#define C2M_CC_TILE (C2M_CC_TW * C2M_CC_TH)
#define C2M_SI_CHUNK 1024                      // consecutive raster pixels ranked by one workgroup
#define C2M_SI_MAX_THINGS 32

C2M_API int c2m_components_tile_w(void) { return C2M_CC_TW; }
C2M_API int c2m_components_tile_h(void) { return C2M_CC_TH; }

static inline bool cc_sizes_ok(int N, int H, int W) {
    return N >= 0 && H >= 1 && W >= 1 && (long)H * W < (1L << 31) && (long)N * H * W < (1L << 31);
}

// Workspace of the operator, in int32 words: parent [N][H*W] (every word written by the tile kernel)
C2M_API long c2m_components_workspace_bytes(int N, int H, int W) {
    if (!cc_sizes_ok(N, H, W)) return -1;
    return (long)N * H * W * 4;
}

__device__ __forceinline__ int cc_lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void cc_lds_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// ------------------------------------------------------------------------------------------------ tile pass
template <class K>
__global__ __launch_bounds__(256) void cc_tile_kernel(const K* __restrict__ keys, long stride_n, long stride_y,
                                                      int* __restrict__ parent, int H, int W, int tiles_x, int tiles_per_img,
                                                      int conn8) {
    __shared__ int s_key[C2M_CC_TILE];
    __shared__ int s_lab[C2M_CC_TILE];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / tiles_per_img, t = blockIdx.x - n * tiles_per_img;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int x0 = tx * C2M_CC_TW, y0 = ty * C2M_CC_TH;
    const int tw = min(C2M_CC_TW, W - x0), th = min(C2M_CC_TH, H - y0);       // the part of the tile inside the image
    const K* __restrict__ src = keys + n * stride_n;
    const int lx = tid & (C2M_CC_TW - 1);
    bool in[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = tid + 256 * j, ly = p / C2M_CC_TW;
        in[j] = lx < tw && ly < th;
        s_key[p] = in[j] ? (int)src[(long)(y0 + ly) * stride_y + x0 + lx] : 0;   // positions outside are never compared
        s_lab[p] = p;
    }
    __syncthreads();
    // Invariant: s_lab[p] <= p and lies in p's component; at the top of a pass every label is a root (s_lab[l] == l).
    // Bound: a pass that sets the flag lowers at least one of the 1024 labels, and a label is lowered at most 1023 times.
    for (;;) {
        bool changed = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (in[j]) {
                const int p = tid + 256 * j, ly = p / C2M_CC_TW;
                const int k = s_key[p], l = cc_lds_load(&s_lab[p]);
                int m = l;
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        if ((dy == 0 && dx == 0) || (!conn8 && dy != 0 && dx != 0)) continue;
                        const int qx = lx + dx, qy = ly + dy;
                        if ((unsigned)qx < (unsigned)tw && (unsigned)qy < (unsigned)th) {
                            const int q = qy * C2M_CC_TW + qx;
                            if (s_key[q] == k) m = min(m, cc_lds_load(&s_lab[q]));
                        }
                    }
                if (m < l) { atomicMin(&s_lab[l], m); changed = true; }        // l was a root when the pass began
            }
        }
        if (!__syncthreads_or(changed)) break;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (in[j]) {
                const int p = tid + 256 * j;
                int r = cc_lds_load(&s_lab[p]);
                for (;;) {                                                    // bound: r strictly decreases, at most p steps
                    const int q = cc_lds_load(&s_lab[r]);
                    if (q >= r) break;
                    r = q;
                }
                cc_lds_store(&s_lab[p], r);                                   // only the owner stores here: a root stays a root
            }
        }
        __syncthreads();
    }
    int* __restrict__ par = parent + (long)n * H * W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (in[j]) {
            const int p = tid + 256 * j, ly = p / C2M_CC_TW;
            const int r = s_lab[p];
            par[(long)(y0 + ly) * W + x0 + lx] = (y0 + r / C2M_CC_TW) * W + x0 + (r & (C2M_CC_TW - 1));
        }
    }
}

// ------------------------------------------------------------------------------------------------ seam pass
__device__ __forceinline__ int cc_parent_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Some ancestor of i that looked like a root when it was read.  Bound: i strictly decreases, at most i steps.
__device__ __forceinline__ int cc_find(int* par, int i) {
    for (;;) {
        const int q = cc_parent_load(par + i);
        if (q >= i) return i;
        i = q;
    }
}

// Union by minimum index.  Bound: max(a, b) strictly decreases from one round to the next (the new pair is {old, b} with
// old < a and b < a, and cc_find only lowers), so there are at most max(a, b) rounds.  Nothing here reads a location twice to
// see it change: a round ends with the value atomicMin returned.
__device__ __forceinline__ void cc_union(int* par, int a, int b) {
    for (;;) {
        a = cc_find(par, a);
        b = cc_find(par, b);
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = atomicMin(par + a, b);
        if (old == a) return;                                                 // a was a root and now hangs below b
        a = old;                                                              // a had a parent already: unite that one with b
    }
}

template <class K>
__global__ __launch_bounds__(256) void cc_seam_kernel(const K* __restrict__ keys, long stride_n, long stride_y, int* parent, int H,
                                                      int W, int n_vseam, int n_hseam, long per_img, long total, int conn8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;                                                   // no barrier and no wave-wide call below
    const int n = (int)(i / per_img);
    long t = i - n * per_img;
    const K* __restrict__ src = keys + n * stride_n;
    int* par = parent + (long)n * H * W;
    const long v_threads = (long)n_vseam * H;
    if (t < v_threads) {                                                      // left of a vertical seam: x + 1 < W
        const int y = (int)(t / n_vseam), x = ((int)(t - (long)y * n_vseam) + 1) * C2M_CC_TW - 1;
        const K* __restrict__ row = src + (long)y * stride_y + x;
        const K k = row[0];
        const int a = y * W + x;
        if (row[1] == k) cc_union(par, a, a + 1);
        if (conn8) {
            if (y > 0 && row[1 - stride_y] == k) cc_union(par, a, a - W + 1);
            if (y + 1 < H && row[1 + stride_y] == k) cc_union(par, a, a + W + 1);
        }
    } else {                                                                  // above a horizontal seam: y + 1 < H
        t -= v_threads;
        const int s = (int)(t / W), x = (int)(t - (long)s * W), y = (s + 1) * C2M_CC_TH - 1;
        const K* __restrict__ row = src + (long)y * stride_y + x;
        const K k = row[0];
        const int a = y * W + x;
        if (row[stride_y] == k) cc_union(par, a, a + W);
        if (conn8) {
            if (x > 0 && row[stride_y - 1] == k) cc_union(par, a, a + W - 1);
            if (x + 1 < W && row[stride_y + 1] == k) cc_union(par, a, a + W + 1);
        }
    }
}

// ------------------------------------------------------------------------------------------------ flatten pass
__global__ __launch_bounds__(256) void cc_flatten_kernel(const int* __restrict__ parent, int* __restrict__ label, long HW,
                                                         long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long base = i - i % HW;
    const int* __restrict__ par = parent + base;
    int r = (int)(i - base);
    for (;;) {                                                                // bound: r strictly decreases, at most r steps
        const int q = par[r];
        if (q >= r) break;
        r = q;
    }
    label[i] = r;
}

template <class K>
static int cc_launch(const K* keys, long stride_n, long stride_y, int* parent, int* label, int N, int H, int W, int conn8,
                     hipStream_t s) {
    const long HW = (long)H * W;
    const int tiles_x = c2m_cdiv(W, C2M_CC_TW), tiles_y = c2m_cdiv(H, C2M_CC_TH);
    const long tiles = (long)tiles_x * tiles_y;
    const int n_vseam = tiles_x - 1, n_hseam = tiles_y - 1;
    const long per_img = (long)n_vseam * H + (long)n_hseam * W;               // < H * W
    hipLaunchKernelGGL(cc_tile_kernel<K>, dim3((unsigned)(tiles * N)), dim3(256), 0, s, keys, stride_n, stride_y, parent, H, W,
                       tiles_x, (int)tiles, conn8);
    C2M_LAUNCH_CHECK();
    // an image of one tile has no seam: the launch stays (one thread that returns), so that the launch count is fixed
    const long seam_total = per_img * N;
    const long seam_blocks = seam_total > 0 ? (seam_total + 255) / 256 : 1;
    hipLaunchKernelGGL(cc_seam_kernel<K>, dim3((unsigned)seam_blocks), dim3(256), 0, s, keys, stride_n, stride_y, parent, H, W,
                       n_vseam, n_hseam, per_img > 0 ? per_img : 1, seam_total, conn8);
    C2M_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)((HW * N + 255) / 256)), dim3(256), 0, s, parent, label, HW, HW * N);
    return (int)hipGetLastError();
}

C2M_API int c2m_connected_components(const void* keys, int key_bytes, long stride_n, long stride_y, int32_t* labels,
                                     void* workspace, long workspace_bytes, int N, int H, int W, int connectivity, void* stream) {
    C2M_ENTER();
    if (!cc_sizes_ok(N, H, W) || (connectivity != 4 && connectivity != 8) || (key_bytes != 1 && key_bytes != 4))
        return (int)hipErrorInvalidValue;
    if (stride_y < 0 || stride_n < 0) return (int)hipErrorInvalidValue;         // the keys are only read: rows may overlap
    if (N == 0) return 0;
    if (!keys || !labels || !workspace || workspace_bytes < (long)N * H * W * 4 || !c2m_aligned(4, workspace, labels) ||
        (key_bytes == 4 && !c2m_aligned(4, keys)))
        return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    if (key_bytes == 1) return cc_launch((const uint8_t*)keys, stride_n, stride_y, (int*)workspace, labels, N, H, W, connectivity == 8, s);
    return cc_launch((const int32_t*)keys, stride_n, stride_y, (int*)workspace, labels, N, H, W, connectivity == 8, s);
}

// ================================================================================================ instances from labels
// Workspace, in int32 words: area [N][H*W] (zeroed by every call) | parent [N][H*W] | cnt [N][T][chunks] | base [N][T][chunks]
struct SiWork { int* area; int* parent; int* cnt; int* base; long zero_words, words; int chunks; };

static inline SiWork si_work(void* ws, int N, long HW, int T) {
    SiWork w;
    w.chunks = (int)((HW + C2M_SI_CHUNK - 1) / C2M_SI_CHUNK);
    const long tc = (long)(T > 0 ? T : 1) * w.chunks;
    int* p = (int*)ws;
    w.area = p;                        p += (long)N * HW;
    w.zero_words = p - (int*)ws;
    w.parent = p;                      p += (long)N * HW;
    w.cnt = p;                         p += (long)N * tc;
    w.base = p;                        p += (long)N * tc;
    w.words = p - (int*)ws;
    return w;
}

C2M_API long c2m_semantic_instances_workspace_bytes(int N, int H, int W, int n_things) {
    if (!cc_sizes_ok(N, H, W) || n_things < 0 || n_things > C2M_SI_MAX_THINGS) return -1;
    return si_work(nullptr, N, (long)H * W, n_things).words * 4;
}

// area[root] += 1 for every thing pixel.  Whole waves reach wave_merge_add: a thread past the end contributes nothing.
__global__ __launch_bounds__(256) void si_area_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ comp,
                                                      const uint8_t* __restrict__ class_table, int* __restrict__ area, long HW,
                                                      long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < total;
    bool thing = false;
    int key = 0;
    if (live) {
        thing = class_table[labels[i]] != 0;
        key = (int)(i - i % HW) + comp[i];                                   // n * HW + root < N * H * W < 2^31
    }
    wave_merge_add(area, key, thing);
}

struct SiP {
    const uint8_t* labels; const int* comp; const uint8_t* class_table;      // [N][H*W], [N][H*W], [256]
    const int* area; int* cnt; int* base;                                     // [N][H*W], [N][T][chunks] x 2
    int* instance; int* count; int* dropped;                                  // [N][H*W], [N][T] x 2
    long HW; int T, chunks, min_area, divisor;
};

// 1 + the position of a label's class in the thing list, 0 for every other label (and for a table entry past the list).
__device__ __forceinline__ int si_ord(const SiP& p, int label) {
    const int ord = p.class_table[label];
    return ord > p.T ? 0 : ord;
}

// A thing root that takes part in the numbering: its si_ord, else 0.
__device__ __forceinline__ int si_qualifies(const SiP& p, long q, int local, int ord) {
    return (ord && p.comp[q] == local && p.area[q] >= p.min_area) ? ord : 0;
}

__global__ __launch_bounds__(256) void si_count_kernel(const SiP p) {
    __shared__ int s_cnt[C2M_SI_MAX_THINGS];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / p.chunks, chunk = blockIdx.x - n * p.chunks;
    if (tid < C2M_SI_MAX_THINGS) s_cnt[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < C2M_SI_CHUNK / 256; ++j) {
        const long local = (long)chunk * C2M_SI_CHUNK + j * 256 + tid;
        if (local < p.HW) {
            const long q = n * p.HW + local;
            const int ord = si_qualifies(p, q, (int)local, si_ord(p, p.labels[q]));
            if (ord) atomicAdd(&s_cnt[ord - 1], 1);
        }
    }
    __syncthreads();
    if (tid < p.T) p.cnt[((long)n * p.T + tid) * p.chunks + chunk] = s_cnt[tid];
}

// One workgroup per image, one wave per class at a time: exclusive prefix of cnt along the chunks, 64 chunks per round.
__global__ __launch_bounds__(256) void si_scan_kernel(const SiP p) {
    const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cap = p.divisor - 1;
    for (int t = wave; t < p.T; t += 4) {                                     // wave-uniform
        const int* __restrict__ cnt = p.cnt + ((long)n * p.T + t) * p.chunks;
        int* __restrict__ base = p.base + ((long)n * p.T + t) * p.chunks;
        int carry = 0;
        for (int c0 = 0; c0 < p.chunks; c0 += 64) {                           // wave-uniform
            const int c = c0 + lane;
            const int v = c < p.chunks ? cnt[c] : 0;
            int x = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(x, o, 64);
                if (lane >= o) x += y;
            }
            if (c < p.chunks) base[c] = carry + x - v;
            carry += __shfl(x, 63, 64);
        }
        if (lane == 0) {
            const int kept = min(carry, cap);
            p.count[n * p.T + t] = kept;
            p.dropped[n * p.T + t] = carry - kept;
        }
    }
}

__global__ __launch_bounds__(256) void si_assign_kernel(const SiP p) {
    __shared__ int s_cnt[C2M_SI_MAX_THINGS], s_base[C2M_SI_MAX_THINGS];
    __shared__ int s_rank[4];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / p.chunks, chunk = blockIdx.x - n * p.chunks;
    if (tid < C2M_SI_MAX_THINGS) {
        const bool has = tid < p.T;
        s_cnt[tid] = has ? p.cnt[((long)n * p.T + tid) * p.chunks + chunk] : 0;
        s_base[tid] = has ? p.base[((long)n * p.T + tid) * p.chunks + chunk] : 0;
    }
    int want[C2M_SI_CHUNK / 256], lab[C2M_SI_CHUNK / 256];
#pragma unroll
    for (int j = 0; j < C2M_SI_CHUNK / 256; ++j) {
        const long local = (long)chunk * C2M_SI_CHUNK + j * 256 + tid;
        want[j] = 0;
        lab[j] = 0;
        if (local < p.HW) {
            const long q = n * p.HW + local;
            lab[j] = p.labels[q];
            const int ord = si_ord(p, lab[j]);
            want[j] = si_qualifies(p, q, (int)local, ord);
            // stuff and ignore_label keep the label; so does a thing root below min_area.  The other thing pixels take their
            // root's value in the paint kernel.
            if (!ord || (!want[j] && p.comp[q] == (int)local)) p.instance[q] = lab[j];
        }
    }
    __syncthreads();
    const int cap = p.divisor - 1;
    for (int t = 0; t < p.T; ++t) {                                           // block-uniform
        if (s_cnt[t] == 0) continue;                                          // block-uniform: LDS written before the barrier
        int run = s_base[t];
#pragma unroll
        for (int j = 0; j < C2M_SI_CHUNK / 256; ++j) {                        // raster order inside the chunk: j, then tid
            int total;
            const bool mine = want[j] == t + 1;
            const int rank = block_rank_256(mine, s_rank, total);
            if (mine) {
                const int k = run + rank + 1;
                p.instance[n * p.HW + (long)chunk * C2M_SI_CHUNK + j * 256 + tid] = k <= cap ? lab[j] * p.divisor + k : lab[j];
            }
            run += total;
            __syncthreads();                                                  // s_rank is rewritten by the next call
        }
    }
}

// instance is read at the roots (written by si_assign_kernel, never here) and written elsewhere: no __restrict__ on it.
__global__ __launch_bounds__(256) void si_paint_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ comp,
                                                       const uint8_t* __restrict__ class_table, int* instance, long HW, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long base = i - i % HW;
    const int root = comp[i];
    if (class_table[labels[i]] && root != (int)(i - base)) instance[i] = instance[base + root];
}

C2M_API int c2m_semantic_instances(const uint8_t* labels, const uint8_t* class_table, int n_things, int32_t* instance,
                                   int32_t* components, int32_t* count, int32_t* dropped, void* workspace, long workspace_bytes,
                                   int N, int H, int W, int connectivity, int min_area, int label_divisor, void* stream) {
    C2M_ENTER();
    if (!cc_sizes_ok(N, H, W) || (connectivity != 4 && connectivity != 8)) return (int)hipErrorInvalidValue;
    if (n_things < 0 || n_things > C2M_SI_MAX_THINGS || min_area < 1 || label_divisor < 1 || 256L * label_divisor >= (1L << 31))
        return (int)hipErrorInvalidValue;
    if (N == 0) return 0;
    if (!labels || !class_table || !instance || !components || !count || !dropped || !workspace)
        return (int)hipErrorInvalidValue;
    const long HW = (long)H * W, total = HW * N;
    const SiWork w = si_work(workspace, N, HW, n_things);
    if (workspace_bytes < w.words * 4 || !c2m_aligned(4, workspace, instance, components, count, dropped))
        return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = c2m_zero_async(w.area, w.zero_words * 4, s);
    if (e != hipSuccess) return (int)e;
    const int rc = cc_launch(labels, HW, (long)W, w.parent, components, N, H, W, connectivity == 8, s);
    if (rc) return rc;
    const unsigned pix_blocks = (unsigned)((total + 255) / 256), chunk_blocks = (unsigned)((long)w.chunks * N);
    hipLaunchKernelGGL(si_area_kernel, dim3(pix_blocks), dim3(256), 0, s, labels, components, class_table, w.area, HW, total);
    C2M_LAUNCH_CHECK();
    const SiP p{labels, components, class_table, w.area, w.cnt, w.base, instance, count, dropped, HW, n_things, w.chunks, min_area,
                label_divisor};
    hipLaunchKernelGGL(si_count_kernel, dim3(chunk_blocks), dim3(256), 0, s, p);
    C2M_LAUNCH_CHECK();
    hipLaunchKernelGGL(si_scan_kernel, dim3(N), dim3(256), 0, s, p);
    C2M_LAUNCH_CHECK();
    hipLaunchKernelGGL(si_assign_kernel, dim3(chunk_blocks), dim3(256), 0, s, p);
    C2M_LAUNCH_CHECK();
    hipLaunchKernelGGL(si_paint_kernel, dim3(pix_blocks), dim3(256), 0, s, labels, components, class_table, instance, HW, total);
    return (int)hipGetLastError();
}
