// Scoring of label maps (gfx950): per image and class the panoptic-quality counts (tp, fp, fn, sum of matched IoUs) and the
// confusion matrix of N predicted maps against N ground-truth maps, as the reference computes them one image at a time on the
// host (cityscapesscripts/evaluation/evalPanopticSemanticLabeling.py: pq_compute_single_core; panoptic_deeplab/segmentation/
// evaluation/semantic.py: SemanticEvaluator.update) with np.unique over packed 64-bit keys and Python loops over the segments.
// Here a zero-fill and three kernels run on the caller's stream and nothing is read back (DESIGN.md 4.2j has the contract).
//
// A map value v reads as (cat, n) = (v, 0) below label_divisor, else (v / label_divisor, v % label_divisor); the pixel is void
// when v < 0, cat == ignore_label or cat >= num_classes.  key = cat * label_divisor + n < K = num_classes * label_divisor; void
// is K.  A ground-truth key of a thing class with n == 0 is that class's crowd region.
//
//   mq_count_kernel  one pass over both maps, tiles of 2048 pixels of one image per workgroup (at most 1024 workgroups in all, each
//                    walking its tiles with one LDS table).  A wave holds 64 consecutive pixels at a
//                    time and walks its DISTINCT (gt key, pred key) pairs (the walk of wave_key_step, wave.h); the leader lane
//                    of a pair adds the number of lanes that hold it to a 256-slot pair table in LDS.  After a barrier every
//                    occupied slot is committed ONCE to the image's tables in global memory: confusion[pc][gc], area_g[g],
//                    area_p[p], void_p[p] (g void), crowd_p[p] (g the crowd region of p's class) and, for a pair of equal class
//                    whose g is no crowd region, the image's open-addressing hash table of max_pairs slots: the 64-bit key is
//                    claimed with atomicCAS, the count added with an int32 atomicAdd, linear probing, at most max_pairs probes,
//                    then the image's overflow flag is set and the pair is dropped.  A pair that finds no LDS slot within
//                    C2M_MQ_LDS_PROBES probes is committed directly.  No loop here waits for another wave: every loop is
//                    bounded by a number fixed before it starts.
//   mq_pair_kernel   one thread per hash slot: inter = count, union = area_p + area_g - inter - void_p; a match iff 2 * inter >
//                    union, which writes inter / union (float64) to match_iou[g] and sets matched_p[p] -- each written at most
//                    once, because two disjoint intersections cannot both exceed half of area_g, or half of area_p - void_p.
//   mq_class_kernel  one wave per image and class walks n = 0 .. label_divisor - 1 in ascending order, 64 at a time: tp / fn
//                    (ground truth, crowd regions left out) and fp (prediction; left out when 2 * (void_p + crowd_p) > area_p)
//                    are counted by ballot, and the matched entries' match_iou are added one after the other in ascending n,
//                    in float64: the order of the reference's sorted keys, so the sum equals its sum bit for bit.
//
// The two "> 0.5" tests are made on integers: for counts below 2^31, a / b > 0.5 in float64 (a correctly rounded quotient of
// two exactly represented integers) holds iff 2 * a > b -- a quotient that is not exactly 0.5 differs from it by at least
// 1 / (2 b) > 2^-33, far above the rounding of the division.  The products are formed in 64 bits.
// The only atomics are integer adds, ORs and compare-and-swaps on keys that never change once set; every output is bit-repeatable.
#include "common.h"

#define C2M_MQ_PPT 8                            // pixels per thread of the count kernel
#define C2M_MQ_BLOCK_PIX (256 * C2M_MQ_PPT)
#define C2M_MQ_LDS_SLOTS 256                    // pair table of one workgroup (3 KB)
#define C2M_MQ_LDS_PROBES 8
#define C2M_MQ_MAX_KEYS (1 << 20)               // num_classes * label_divisor
#define C2M_MQ_MAX_PAIRS (1 << 22)
#define C2M_MQ_COUNT_BLOCKS 1024                // workgroups of the count kernel over all images (4 per CU)

typedef unsigned long long mq_u64;

// Workspace (all of it zeroed by every call): hkey [N][P] u64 | match_iou [N][K] f64 | area_g, area_p, void_p, crowd_p, matched_p
// [N][K] int32 each | conf [N][(C+1)^2] int32 | hcnt [N][P] int32 | overflow [N] int32
struct MqWork {
    mq_u64* hkey; double* match_iou;
    int *area_g, *area_p, *void_p, *crowd_p, *matched_p, *conf, *hcnt, *overflow;
    long bytes;
};

static inline MqWork mq_work(void* base, long N, long K, long C1, long P) {
    MqWork w;
    char* p = (char*)base;
    w.hkey = (mq_u64*)p;               p += N * P * 8;
    w.match_iou = (double*)p;          p += N * K * 8;
    w.area_g = (int*)p;                p += N * K * 4;
    w.area_p = (int*)p;                p += N * K * 4;
    w.void_p = (int*)p;                p += N * K * 4;
    w.crowd_p = (int*)p;               p += N * K * 4;
    w.matched_p = (int*)p;             p += N * K * 4;
    w.conf = (int*)p;                  p += N * C1 * C1 * 4;
    w.hcnt = (int*)p;                  p += N * P * 4;
    w.overflow = (int*)p;              p += N * 4;
    w.bytes = p - (char*)base;
    return w;
}

static inline bool mq_sizes_ok(long N, int C, int divisor, int max_pairs) {
    if (N < 0 || N >= (1L << 24) || C < 1 || C > 255 || divisor < 1 || (long)C * divisor > C2M_MQ_MAX_KEYS) return false;
    if (max_pairs < 1 || max_pairs > C2M_MQ_MAX_PAIRS || (max_pairs & (max_pairs - 1))) return false;
    return true;
}

C2M_API long c2m_map_quality_workspace_bytes(int N, int num_classes, int label_divisor, int max_pairs) {
    if (!mq_sizes_ok(N, num_classes, label_divisor, max_pairs)) return -1;
    return mq_work(nullptr, N, (long)num_classes * label_divisor, num_classes + 1, max_pairs).bytes;
}

struct MqP {
    const void* pred; const void* gt;                       // [N][H][W], int32 or uint8 (both the same)
    const uint8_t* thing;                                   // [256]: non-zero for a thing class
    MqWork w;
    long HW; int C, divisor, ignore, K, P, blocks_per_img, tiles_per_img;
};

__device__ __forceinline__ int mq_key(int v, int divisor, int C, int ignore, int K) {
    if (v < 0) return K;
    const int cat = v < divisor ? v : v / divisor;
    if (cat == ignore || cat >= C) return K;
    return v < divisor ? cat * divisor : v;                 // cat * divisor + n is v itself at or above the divisor
}

// `cnt` more pixels of the pair `key` (never 0: the empty slot) -> one image's open-addressing table of P slots.
__device__ __forceinline__ void mq_pair_add(mq_u64* __restrict__ hkey, int* hcnt, int* overflow, int P, mq_u64 key, int cnt) {
    const unsigned mask = (unsigned)P - 1u;
    unsigned slot = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
    for (int i = 0; i < P; ++i, slot = (slot + 1u) & mask) {               // at most max_pairs probes: no unbounded loop
        mq_u64 cur = __hip_atomic_load(hkey + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0ull) cur = atomicCAS(hkey + slot, 0ull, key);          // a key never changes once it is set
        if (cur == 0ull || cur == key) {
            atomicAdd(hcnt + slot, cnt);
            return;
        }
    }
    atomicOr(overflow, 1);                                                 // the table is full: the pair is dropped
}

// One distinct (g, p) pair of an image with its pixel count -> the image's tables.
__device__ void mq_commit(const MqP& a, int img, int g, int p, int cnt) {
    const int K = a.K, C = a.C, div = a.divisor;
    const int gc = g == K ? C : g / div, pc = p == K ? C : p / div;
    atomicAdd(a.w.conf + ((long)img * (C + 1) + pc) * (C + 1) + gc, cnt);
    const long t = (long)img * K;
    if (g != K) atomicAdd(a.w.area_g + t + g, cnt);
    if (p == K) return;
    atomicAdd(a.w.area_p + t + p, cnt);
    if (g == K) { atomicAdd(a.w.void_p + t + p, cnt); return; }
    if (gc != pc) return;
    if (a.thing[gc] && g == gc * div) { atomicAdd(a.w.crowd_p + t + p, cnt); return; }
    const mq_u64 key = (mq_u64)g * (mq_u64)(K + 1) + (mq_u64)p + 1ull;     // 0 is the empty slot
    mq_pair_add(a.w.hkey + (long)img * a.P, a.w.hcnt + (long)img * a.P, a.w.overflow + img, a.P, key, cnt);
}

template <typename T>
__global__ __launch_bounds__(256) void mq_count_kernel(const MqP a) {
    __shared__ mq_u64 s_key[C2M_MQ_LDS_SLOTS];
    __shared__ int s_cnt[C2M_MQ_LDS_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int img = blockIdx.x / a.blocks_per_img, blk = blockIdx.x - img * a.blocks_per_img;
    s_key[tid] = 0ull;
    s_cnt[tid] = 0;
    __syncthreads();
    const long HW = a.HW;
    const T* __restrict__ pm = (const T*)a.pred + (long)img * HW;          // 64-bit base offset of the image
    const T* __restrict__ gm = (const T*)a.gt + (long)img * HW;
    const int K = a.K;
    for (long tile = blk; tile < a.tiles_per_img; tile += a.blocks_per_img) {  // block-uniform: the LDS table is kept across tiles
    const long q0 = tile * C2M_MQ_BLOCK_PIX + tid;
    int gk[C2M_MQ_PPT], pk[C2M_MQ_PPT];
    bool live[C2M_MQ_PPT];
#pragma unroll
    for (int j = 0; j < C2M_MQ_PPT; ++j) {
        const long q = q0 + j * 256;
        live[j] = q < HW;
        gk[j] = pk[j] = K;
        if (live[j]) {
            gk[j] = mq_key((int)gm[q], a.divisor, a.C, a.ignore, K);
            pk[j] = mq_key((int)pm[q], a.divisor, a.C, a.ignore, K);
        }
    }
#pragma unroll
    for (int j = 0; j < C2M_MQ_PPT; ++j) {
        // wave_key_step (wave.h) for two keys, written out: on the shared step this kernel's register allocation changes
        unsigned long long todo = __ballot(live[j]);
        while (todo) {                                                     // wave-uniform; every round clears at least one bit
            const int leader = __ffsll((long long)todo) - 1;
            const int g0 = __shfl(gk[j], leader, 64), p0 = __shfl(pk[j], leader, 64);
            const unsigned long long same = __ballot(live[j] && gk[j] == g0 && pk[j] == p0) & todo;
            if (lane == leader) {
                const int cnt = __popcll(same);
                const mq_u64 key = (mq_u64)g0 * (mq_u64)(K + 1) + (mq_u64)p0 + 1ull;
                unsigned slot = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 40) & (C2M_MQ_LDS_SLOTS - 1);
                bool done = false;
                for (int i = 0; i < C2M_MQ_LDS_PROBES && !done; ++i, slot = (slot + 1u) & (C2M_MQ_LDS_SLOTS - 1)) {
                    mq_u64 cur = __hip_atomic_load(&s_key[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (cur == 0ull) cur = atomicCAS(&s_key[slot], 0ull, key);
                    if (cur == 0ull || cur == key) { atomicAdd(&s_cnt[slot], cnt); done = true; }
                }
                if (!done) mq_commit(a, img, g0, p0, cnt);
            }
            todo &= ~same;
        }
    }
    }
    __syncthreads();
    const mq_u64 key = s_key[tid];
    if (key) {
        const mq_u64 k1 = key - 1ull;
        const int g = (int)(k1 / (mq_u64)(K + 1)), p = (int)(k1 - (mq_u64)g * (mq_u64)(K + 1));
        mq_commit(a, img, g, p, s_cnt[tid]);
    }
}

// One thread per slot of the images' pair tables.
__global__ __launch_bounds__(256) void mq_pair_kernel(const MqP a, int blocks_per_img) {
    const int img = blockIdx.x / blocks_per_img, s = (blockIdx.x - img * blocks_per_img) * 256 + threadIdx.x;
    if (s >= a.P) return;
    const mq_u64 key = a.w.hkey[(long)img * a.P + s];
    if (key == 0ull) return;
    const int K = a.K;
    const long t = (long)img * K;
    const mq_u64 k1 = key - 1ull;
    const int g = (int)(k1 / (mq_u64)(K + 1)), p = (int)(k1 - (mq_u64)g * (mq_u64)(K + 1));
    const long long inter = a.w.hcnt[(long)img * a.P + s];
    const long long uni = (long long)a.w.area_p[t + p] + a.w.area_g[t + g] - inter - a.w.void_p[t + p];
    if (2 * inter > uni) {                                                 // iou > 0.5 (see the head of the file)
        a.w.match_iou[t + g] = (double)inter / (double)uni;                // written at most once per g and per p
        a.w.matched_p[t + p] = 1;
    }
}

// One wave per image and class: 64 consecutive n at a time, counts by ballot, the IoU sum over the matched entries in ascending n.
__global__ __launch_bounds__(64) void mq_class_kernel(const MqP a, int* __restrict__ tp, int* __restrict__ fp,
                                                      int* __restrict__ fn, double* __restrict__ iou,
                                                      long long* __restrict__ confusion, uint8_t* __restrict__ overflow) {
    const int C = a.C, div = a.divisor, lane = threadIdx.x;
    const int img = blockIdx.x / C, c = blockIdx.x - img * C;
    const long base = (long)img * a.K + (long)c * div;
    const bool thing = a.thing[c] != 0;
    int n_tp = 0, n_fp = 0, n_fn = 0;
    double sum = 0.0;
    for (int n0 = 0; n0 < div; n0 += 64) {                                 // wave-uniform
        const int n = n0 + lane;
        int ag = 0, ap = 0, mp = 0, vp = 0, cp = 0;
        double mi = 0.0;
        if (n < div) {
            ag = a.w.area_g[base + n]; ap = a.w.area_p[base + n]; mp = a.w.matched_p[base + n];
            vp = a.w.void_p[base + n]; cp = a.w.crowd_p[base + n]; mi = a.w.match_iou[base + n];
        }
        const bool seg = ag > 0 && !(thing && n == 0);                     // a ground-truth segment that is no crowd region
        unsigned long long m = __ballot(seg && mi != 0.0);
        n_tp += __popcll(m);
        n_fn += __popcll(__ballot(seg && mi == 0.0));
        n_fp += __popcll(__ballot(ap > 0 && !mp && !(2ll * ((long long)vp + cp) > (long long)ap)));
        while (m) {                                                        // ascending n, serial, the same in every lane
            sum += __shfl(mi, __ffsll((long long)m) - 1, 64);
            m &= m - 1ull;
        }
    }
    if (lane == 0) {
        const long o = (long)img * C + c;
        tp[o] = n_tp; fp[o] = n_fp; fn[o] = n_fn; iou[o] = sum;
        if (c == 0) overflow[img] = a.w.overflow[img] ? 1 : 0;
    }
    const long row = ((long)img * (C + 1) + c) * (C + 1);                  // the int32 counts of row c (and of the void row) as int64
    for (int i = lane; i < (c == C - 1 ? 2 : 1) * (C + 1); i += 64) confusion[row + i] = a.w.conf[row + i];
}

C2M_API int c2m_map_quality(const void* pred, const void* gt, int is_u8, const uint8_t* thing_table, int32_t* tp, int32_t* fp,
                            int32_t* fn, double* iou, int64_t* confusion, uint8_t* overflow, void* workspace,
                            long workspace_bytes, int N, int H, int W, int num_classes, int label_divisor, int ignore_label,
                            int max_pairs, void* stream) {
    C2M_ENTER();
    if (H < 1 || W < 1 || ignore_label < 0 || !mq_sizes_ok(N, num_classes, label_divisor, max_pairs))
        return (int)hipErrorInvalidValue;
    const long HW = (long)H * W;
    if (HW >= (1L << 31)) return (int)hipErrorInvalidValue;
    if (N == 0) return 0;
    if (!pred || !gt || !thing_table || !tp || !fp || !fn || !iou || !confusion || !overflow || !workspace)
        return (int)hipErrorInvalidValue;
    const int K = num_classes * label_divisor;
    const MqWork w = mq_work(workspace, N, K, num_classes + 1, max_pairs);
    if (workspace_bytes < w.bytes || !c2m_aligned(8, workspace)) return (int)hipErrorInvalidValue;
    const long bpi = (HW + C2M_MQ_BLOCK_PIX - 1) / C2M_MQ_BLOCK_PIX;
    const int pb = (max_pairs + 255) / 256;
    if ((long)pb * N >= (1L << 31) || (long)N * num_classes >= (1L << 31)) return (int)hipErrorInvalidValue;

    hipStream_t s = (hipStream_t)stream;
    hipError_t e = c2m_zero_async(workspace, w.bytes, s);
    if (e != hipSuccess) return (int)e;
    long blocks = C2M_MQ_COUNT_BLOCKS / N;                                 // workgroups per image: each walks its tiles with one
    blocks = blocks < 1 ? 1 : (blocks > bpi ? bpi : blocks);               // LDS pair table, so fewer flushes reach the hot keys
    const MqP a{pred, gt, thing_table, w, HW, num_classes, label_divisor, ignore_label, K, max_pairs, (int)blocks, (int)bpi};
    if (is_u8) hipLaunchKernelGGL(mq_count_kernel<uint8_t>, dim3((unsigned)(blocks * N)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(mq_count_kernel<int32_t>, dim3((unsigned)(blocks * N)), dim3(256), 0, s, a);
    C2M_LAUNCH_CHECK();
    hipLaunchKernelGGL(mq_pair_kernel, dim3((unsigned)((long)pb * N)), dim3(256), 0, s, a, pb);
    C2M_LAUNCH_CHECK();
    hipLaunchKernelGGL(mq_class_kernel, dim3((unsigned)(N * num_classes)), dim3(64), 0, s, a, tp, fp, fn, iou,
                       (long long*)confusion, overflow);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ tubes
// Video panoptic quality: a segment is a TUBE, the pixels of one (cat, n) in the k consecutive frames of a window, and the rules
// above apply to the window as if its frames were one image.  Every table of the count pass is additive over pixels, so the
// window's tables are the sums of its frames' tables and the pixels are read once, by mq_count_kernel over the B * T frames:
//
//   mq_merge_kernel  per window (b, t0) of k frames: area_g, area_p, void_p, crowd_p [K] are summed over the k frames by one
//                    thread per key, and every occupied slot of the k per-frame pair tables is inserted into the window's table
//                    with mq_pair_add -- the same key, the same hash, integer atomicCAS / atomicAdd, at most max_pairs probes.
//                    The window's flag is set when a frame's flag is or when the window's own table fills.
//   mq_pair_kernel, mq_class_kernel   as they are, on an MqWork of B * (T - k + 1) "images"; k = 1 runs them on the frame tables.
//   mq_id_kernel     one thread per (window, listed id): the same-id IoU of one named object, by a bounded lookup of (g, g).
//
// The window tables are not given a confusion matrix (it has no tube form); mq_class_kernel's copy of it goes to scratch.
struct MqMergeP {
    MqWork f, w;                                            // per frame [B * T], per window [B * wpc]
    int T, k, wpc, K, P, blocks_a, blocks_h;                // wpc = T - k + 1 windows per clip
};

__global__ __launch_bounds__(256) void mq_merge_kernel(const MqMergeP m) {
    const int per = m.blocks_a + m.blocks_h;
    const int win = blockIdx.x / per, blk = blockIdx.x - win * per;
    const int b = win / m.wpc, t0 = win - b * m.wpc;
    const long f0 = (long)b * m.T + t0;                                    // the window's first frame; it ends inside clip b
    if (blk < m.blocks_a) {
        if (blk == 0 && threadIdx.x == 0) {
            int any = 0;
            for (int f = 0; f < m.k; ++f) any |= m.f.overflow[f0 + f];
            if (any) atomicOr(m.w.overflow + win, 1);
        }
        const int j = blk * 256 + threadIdx.x;
        if (j >= m.K) return;
        int ag = 0, ap = 0, vp = 0, cp = 0;                                // below 2^31: k * H * W is
        for (int f = 0; f < m.k; ++f) {
            const long i = (f0 + f) * m.K + j;
            ag += m.f.area_g[i]; ap += m.f.area_p[i]; vp += m.f.void_p[i]; cp += m.f.crowd_p[i];
        }
        const long o = (long)win * m.K + j;
        m.w.area_g[o] = ag; m.w.area_p[o] = ap; m.w.void_p[o] = vp; m.w.crowd_p[o] = cp;
        return;
    }
    const int s = (blk - m.blocks_a) * 256 + threadIdx.x;
    if (s >= m.P) return;
    for (int f = 0; f < m.k; ++f) {                                        // the key of a frame's slot is the window's key as well
        const long i = (f0 + f) * m.P + s;
        const mq_u64 key = m.f.hkey[i];
        if (key) mq_pair_add(m.w.hkey + (long)win * m.P, m.w.hcnt + (long)win * m.P, m.w.overflow + win, m.P, key, m.f.hcnt[i]);
    }
}

// One thread per (window, m): the tube IoU of the object ids[b][m] with the tube of the same id.
__global__ __launch_bounds__(256) void mq_id_kernel(const MqP a, const int* __restrict__ ids, int M, int wpc, long total,
                                                    double* __restrict__ id_iou, int* __restrict__ id_gt_area,
                                                    int* __restrict__ id_pred_area) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long win = i / M;
    const int m = (int)(i - win * M), b = (int)(win / wpc);
    const int v = ids[(long)b * M + m], K = a.K;
    double r = -1.0;
    int ga = 0, pa = 0;
    const int g = v < 0 ? K : mq_key(v, a.divisor, a.C, a.ignore, K);
    if (g != K) {
        const int gc = g / a.divisor;
        if (!(a.thing[gc] && g == gc * a.divisor)) {
            const long t = win * K;
            ga = a.w.area_g[t + g];
            pa = a.w.area_p[t + g];
            if (ga > 0) {
                const mq_u64 key = (mq_u64)g * (mq_u64)(K + 1) + (mq_u64)g + 1ull;
                const unsigned mask = (unsigned)a.P - 1u;
                unsigned slot = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
                long long inter = 0;
                for (int n = 0; n < a.P; ++n, slot = (slot + 1u) & mask) { // at most max_pairs probes
                    const mq_u64 cur = a.w.hkey[win * a.P + slot];
                    if (cur == key) inter = a.w.hcnt[win * a.P + slot];
                    if (cur == key || cur == 0ull) break;
                }
                const long long uni = (long long)pa + ga - inter - a.w.void_p[t + g];    // >= ga > 0
                r = (double)inter / (double)uni;
            }
        }
    }
    id_iou[i] = r; id_gt_area[i] = ga; id_pred_area[i] = pa;
}

// Workspace: the frames' MqWork [B * T] | the windows' MqWork [B * max(T - 1, 1)] | confusion scratch int64 [B * T][(C+1)^2]
struct TqWork { long frames, windows, conf, bytes; };

static inline long mq_round8(long v) { return (v + 7) & ~7L; }

static inline bool tq_work(long B, long T, int C, int divisor, int max_pairs, TqWork* out) {
    if (B < 0 || T < 1 || B >= (1L << 24) || T >= (1L << 24) || !mq_sizes_ok(B * T, C, divisor, max_pairs)) return false;
    const long K = (long)C * divisor, nw = B * (T > 1 ? T - 1 : 1);
    out->frames = 0;
    out->windows = mq_round8(mq_work(nullptr, B * T, K, C + 1, max_pairs).bytes);
    out->conf = out->windows + mq_round8(mq_work(nullptr, nw, K, C + 1, max_pairs).bytes);
    out->bytes = out->conf + B * T * (long)(C + 1) * (C + 1) * 8;
    return true;
}

C2M_API long c2m_tube_quality_workspace_bytes(int B, int T, int num_classes, int label_divisor, int max_pairs) {
    TqWork t;
    return tq_work(B, T, num_classes, label_divisor, max_pairs, &t) ? t.bytes : -1;
}

C2M_API int c2m_tube_quality(const void* pred, const void* gt, int is_u8, const uint8_t* thing_table, const int32_t* windows,
                             int n_windows, int32_t* tp, int32_t* fp, int32_t* fn, double* iou, uint8_t* overflow,
                             const int32_t* ids, int M, double* id_iou, int32_t* id_gt_area, int32_t* id_pred_area,
                             void* workspace, long workspace_bytes, int B, int T, int H, int W, int num_classes,
                             int label_divisor, int ignore_label, int max_pairs, void* stream) {
    C2M_ENTER();
    TqWork t;
    if (H < 1 || W < 1 || ignore_label < 0 || n_windows < 0 || n_windows > T || M < 0 ||
        !tq_work(B, T, num_classes, label_divisor, max_pairs, &t))
        return (int)hipErrorInvalidValue;
    const long HW = (long)H * W, N = (long)B * T;
    if (HW * T >= (1L << 31)) return (int)hipErrorInvalidValue;           // a window's counts are int32
    if ((ids != nullptr) != (M > 0)) return (int)hipErrorInvalidValue;
    if (n_windows && !windows) return (int)hipErrorInvalidValue;
    for (int i = 0; i < n_windows; ++i) {
        if (windows[i] < 1 || windows[i] > T) return (int)hipErrorInvalidValue;
        for (int j = 0; j < i; ++j)
            if (windows[j] == windows[i]) return (int)hipErrorInvalidValue;
    }
    if (N == 0 || n_windows == 0) return 0;
    if (!pred || !gt || !thing_table || !tp || !fp || !fn || !iou || !overflow || !workspace) return (int)hipErrorInvalidValue;
    if (ids && (!id_iou || !id_gt_area || !id_pred_area)) return (int)hipErrorInvalidValue;
    if (workspace_bytes < t.bytes || !c2m_aligned(8, workspace)) return (int)hipErrorInvalidValue;
    const int K = num_classes * label_divisor;
    const long bpi = (HW + C2M_MQ_BLOCK_PIX - 1) / C2M_MQ_BLOCK_PIX;
    const int pb = (max_pairs + 255) / 256, kb = (K + 255) / 256;
    if ((long)(pb + kb) * N >= (1L << 31) || N * num_classes >= (1L << 31) || N * (M > 0 ? M : 1) >= (1L << 31) * 256)
        return (int)hipErrorInvalidValue;

    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)workspace;
    const MqWork wf = mq_work(base + t.frames, N, K, num_classes + 1, max_pairs);
    long long* conf_scratch = (long long*)(base + t.conf);
    hipError_t e = c2m_zero_async(base + t.frames, wf.bytes, s);
    if (e != hipSuccess) return (int)e;
    long blocks = C2M_MQ_COUNT_BLOCKS / N;                                 // the count pass of c2m_map_quality over the B * T frames
    blocks = blocks < 1 ? 1 : (blocks > bpi ? bpi : blocks);
    const MqP af{pred, gt, thing_table, wf, HW, num_classes, label_divisor, ignore_label, K, max_pairs, (int)blocks, (int)bpi};
    if (is_u8) hipLaunchKernelGGL(mq_count_kernel<uint8_t>, dim3((unsigned)(blocks * N)), dim3(256), 0, s, af);
    else hipLaunchKernelGGL(mq_count_kernel<int32_t>, dim3((unsigned)(blocks * N)), dim3(256), 0, s, af);
    C2M_LAUNCH_CHECK();

    long off = 0;                                                          // windows written so far
    for (int i = 0; i < n_windows; ++i) {
        const int k = windows[i], wpc = T - k + 1;
        const long nw = (long)B * wpc;
        MqP a = af;
        if (k > 1) {
            a.w = mq_work(base + t.windows, nw, K, num_classes + 1, max_pairs);
            e = c2m_zero_async(base + t.windows, a.w.bytes, s);
            if (e != hipSuccess) return (int)e;
            const MqMergeP m{wf, a.w, T, k, wpc, K, max_pairs, kb, pb};
            hipLaunchKernelGGL(mq_merge_kernel, dim3((unsigned)(nw * (kb + pb))), dim3(256), 0, s, m);
            C2M_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(mq_pair_kernel, dim3((unsigned)(pb * nw)), dim3(256), 0, s, a, pb);
        C2M_LAUNCH_CHECK();
        hipLaunchKernelGGL(mq_class_kernel, dim3((unsigned)(nw * num_classes)), dim3(64), 0, s, a, tp + off * num_classes,
                           fp + off * num_classes, fn + off * num_classes, iou + off * num_classes, conf_scratch, overflow + off);
        C2M_LAUNCH_CHECK();
        if (ids) {
            const long total = nw * M;
            hipLaunchKernelGGL(mq_id_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, ids, M, wpc, total,
                               id_iou + off * M, id_gt_area + off * M, id_pred_area + off * M);
            C2M_LAUNCH_CHECK();
        }
        off += nw;
    }
    return (int)hipGetLastError();
}
