// Panoptic-DeepLab post-processing (gfx950): semantic, instance and panoptic maps from the three heads of the network, for N
// images per call.  The reference (panoptic_deeplab/segmentation/model/post_processing/*.py, generate_segmentation.py:299-305)
// takes one image at a time, builds a [K, H*W, 2] fp32 difference tensor and loops on the host over instances and classes with
// a synchronisation each; here five kernels run on the caller's stream and nothing is read back.
//
//   pan_candidates_kernel  a pixel is a candidate centre iff score > threshold and no position of its nms x nms window (inside the
//                          image) holds a larger thresholded score.  Candidates are appended to a per-image list of pixel indices
//                          (int32 atomic counter: the ORDER of that list is arbitrary and nothing below depends on it).
//   pan_select_kernel      one workgroup per image.  Fewer than top_k candidates: all are centres.  Otherwise the exact top_k-th
//                          largest score s_k by a radix select on the float bits (scores above a threshold >= 0 are positive, so
//                          the bit order is the value order) and the centres are the candidates with score > s_k, strictly: ties at
//                          s_k all drop out, as torch.topk + `>` does in the reference.  The survivors (< 1024) are ranked by pixel
//                          index, so centres[n][k] is row-major whatever order the list had.
//   pan_group_kernel       per pixel: argmax over the C logit planes (first maximum; NaN counts as the largest, as torch.argmax),
//                          thing test from a 256-entry class table, nearest centre of (y + dy, x + dx) by d*d + e*e in fp32 with a
//                          strict <, so the first of equally near centres wins.  Writes the labels and the raw id (k + 1 on thing
//                          pixels, else 0) and accumulates votes[n][k][thing class] and area[n][class] (non-thing pixels).
//   pan_merge_kernel       one workgroup per image: k ascending, class = most frequent label of the pixels with raw id k + 1 (ties
//                          to the smaller class), number counted per class; a centre without pixels uses up no number.  Stuff
//                          classes with area >= stuff_area keep class * divisor, everything else is void.
//   pan_paint_kernel       per pixel: panoptic value from the two tables, and the instance-id image (panoptic value on things, else
//                          panoptic / divisor: stuff keeps its class, void becomes ignore_label).
//
// The distance is compared squared; the reference compares torch.norm of the same fp32 differences (a square root of the same
// sum).  Both orders agree wherever the two smallest sums differ by more than an fp32 rounding of the root.
// The only atomics are int32 adds on counters and histograms: every output is bit-repeatable.
// This file is compiled with -ffp-contract=off: d*d + e*e is two products and a sum, as written.
#include "common.h"

#define C2M_PAN_MAX_TOPK 1024                  // centres of one image: staged whole in LDS by the grouping kernel (8 KB)
#define C2M_PAN_MAX_R 7                        // nms_kernel <= 15
#define C2M_PAN_TW 64                          // candidate tile: 64 x 16 pixels, one wave per row, 4 rows per wave
#define C2M_PAN_TH 16
#define C2M_PAN_PPT 4                          // pixels per thread of the grouping and paint kernels
#define C2M_PAN_BLOCK_PIX (256 * C2M_PAN_PPT)

C2M_API int c2m_panoptic_max_top_k(void) { return C2M_PAN_MAX_TOPK; }

// Workspace, in int32 words: cand_count [N] | area [N][256] | votes [N][top_k][max(T,1)]  (zeroed by every call)
//                            | ktab [N][top_k] | stab [N][256] | cand_list [N][H*W]
struct PanWork { int* cand_count; int* area; int* votes; int* ktab; int* stab; int* cand_list; long zero_words, words; };

static inline PanWork pan_work(void* base, int N, long HW, int top_k, int T) {
    PanWork w;
    const long tv = T > 0 ? T : 1;
    int* p = (int*)base;
    w.cand_count = p;                  p += N;
    w.area = p;                        p += (long)N * 256;
    w.votes = p;                       p += (long)N * top_k * tv;
    w.zero_words = p - (int*)base;
    w.ktab = p;                        p += (long)N * top_k;
    w.stab = p;                        p += (long)N * 256;
    w.cand_list = p;                   p += (long)N * HW;
    w.words = p - (int*)base;
    return w;
}

C2M_API long c2m_panoptic_workspace_bytes(int N, int H, int W, int top_k, int n_things) {
    if (N < 0 || H < 1 || W < 1 || top_k < 1 || top_k > C2M_PAN_MAX_TOPK || n_things < 0 || n_things > 255) return -1;
    return pan_work(nullptr, N, (long)H * W, top_k, n_things).words * 4;
}

// ------------------------------------------------------------------------------------------------ candidates
__global__ __launch_bounds__(256) void pan_candidates_kernel(const float* __restrict__ center, int* __restrict__ cand_count,
                                                             int* __restrict__ cand_list, int H, int W, int tiles_x,
                                                             int tiles_per_img, float thr, int r) {
    __shared__ float tile[(C2M_PAN_TH + 2 * C2M_PAN_MAX_R) * (C2M_PAN_TW + 2 * C2M_PAN_MAX_R)];
    const int tid = threadIdx.x, lane = tid & 63;
    const int n = blockIdx.x / tiles_per_img, t = blockIdx.x - n * tiles_per_img;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const long HW = (long)H * W;
    const float* __restrict__ src = center + n * HW;
    const int x0 = tx * C2M_PAN_TW, y0 = ty * C2M_PAN_TH;
    const int LW = C2M_PAN_TW + 2 * r, LH = C2M_PAN_TH + 2 * r;
    // scores at or below the threshold (and NaN) become -1, as F.threshold does before the max pool; positions outside the image
    // hold -1 too: every candidate is > thr >= 0, so -1 never beats one ("do not take part")
    for (int i = tid; i < LW * LH; i += 256) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gy = y0 - r + ly, gx = x0 - r + lx;
        float v = -1.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const float s = src[(long)gy * W + gx];
            v = s > thr ? s : -1.f;
        }
        tile[i] = v;
    }
    __syncthreads();
    int* __restrict__ list = cand_list + n * HW;
    for (int j = 0; j < C2M_PAN_TH / 4; ++j) {                            // whole waves stay in the loop: the append is wave-wide
        const int ly = (tid >> 6) + 4 * j, lx = lane;
        const float v = tile[(ly + r) * LW + lx + r];                     // -1 outside the image
        bool cand = v > 0.f;
        if (cand) {
            for (int dy = -r; dy <= r; ++dy)
                for (int dx = -r; dx <= r; ++dx) cand = cand && !(tile[(ly + r + dy) * LW + lx + r + dx] > v);
        }
        int found;
        const int rank = wave_rank(cand, found);
        if (found) {                                                      // wave-uniform
            int base = 0;
            if (lane == 0) base = atomicAdd(cand_count + n, found);
            base = __shfl(base, 0, 64);
            if (cand) list[base + rank] = (y0 + ly) * W + x0 + lx;        // < H*W entries in all
        }
    }
}

// ------------------------------------------------------------------------------------------------ selection
__global__ __launch_bounds__(1024) void pan_select_kernel(const float* __restrict__ center, const int* __restrict__ cand_count,
                                                          const int* __restrict__ cand_list, int* __restrict__ centers,
                                                          int* __restrict__ center_count, long HW, int W, int top_k) {
    __shared__ int hist[256];
    __shared__ int sel[C2M_PAN_MAX_TOPK];
    __shared__ int s_n, s_digit, s_want;
    const int n = blockIdx.x, tid = threadIdx.x;
    const int L = cand_count[n];
    const int* __restrict__ list = cand_list + n * HW;
    const float* __restrict__ src = center + n * HW;
    const bool all = L < top_k;
    unsigned cut = 0;
    if (!all) {                                                           // block-uniform
        unsigned prefix = 0;
        int want = top_k;                                                 // rank from the top among the keys that match `prefix`
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            const unsigned hi = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
            for (int i = tid; i < L; i += 1024) {
                const unsigned key = __float_as_uint(src[list[i]]);
                if ((key & hi) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int acc = 0, d = 255;
                for (; d > 0; --d) {
                    if (acc + hist[d] >= want) break;
                    acc += hist[d];
                }
                s_digit = d;
                s_want = want - acc;
            }
            __syncthreads();
            prefix |= (unsigned)s_digit << shift;
            want = s_want;
            __syncthreads();                                              // hist and s_* are rewritten by the next digit
        }
        cut = prefix;                                                     // the bits of the top_k-th largest candidate score
    }
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int i = tid; i < L; i += 1024) {
        const int idx = list[i];
        if (all || __float_as_uint(src[idx]) > cut) {                     // at most top_k - 1 keys lie above the top_k-th largest
            const int p = atomicAdd(&s_n, 1);
            if (p < C2M_PAN_MAX_TOPK) sel[p] = idx;
        }
    }
    __syncthreads();
    const int m = min(s_n, top_k);
    int* __restrict__ out = centers + (long)n * top_k * 2;
    for (int i = tid; i < m; i += 1024) {                                 // rank by pixel index: row-major order
        const int v = sel[i];
        int rank = 0;
        for (int j = 0; j < m; ++j) rank += sel[j] < v ? 1 : 0;
        const int y = v / W;
        out[rank * 2] = y;
        out[rank * 2 + 1] = v - y * W;
    }
    for (int i = m + tid; i < top_k; i += 1024) { out[i * 2] = 0; out[i * 2 + 1] = 0; }
    if (tid == 0) center_count[n] = m;
}

// ------------------------------------------------------------------------------------------------ grouping
struct PanGroupP {
    const float* logits; const uint8_t* labels;             // [N][C][H][W] fp32, or [N][H][W] labels (exactly one is set)
    const float* offset;                                    // [N][2][H][W] (dy, dx)
    const int* centers; const int* center_count;            // [N][top_k][2] (y, x), [N]
    const uint8_t* class_table;                             // [256]: 0 = not a thing, else 1 + position in the thing list
    uint8_t* semantic; int* raw;                            // [N][H][W] each; raw is the panoptic plane before painting
    int* votes; int* area;                                  // [N][top_k][T], [N][256], zeroed
    long HW; int C, W, top_k, T, blocks_per_img;
};

__global__ __launch_bounds__(256) void pan_group_kernel(const PanGroupP p) {
    __shared__ float2 s_ctr[C2M_PAN_MAX_TOPK];
    __shared__ int s_area[256];
    __shared__ unsigned char s_tab[256];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / p.blocks_per_img, blk = blockIdx.x - n * p.blocks_per_img;
    const int m = min(max(p.center_count[n], 0), p.top_k);
    const int* __restrict__ ctr = p.centers + (long)n * p.top_k * 2;
    for (int k = tid; k < m; k += 256) s_ctr[k] = make_float2((float)ctr[k * 2], (float)ctr[k * 2 + 1]);
    s_area[tid] = 0;
    s_tab[tid] = p.class_table[tid];
    __syncthreads();

    const long HW = p.HW;
    const long q0 = (long)blk * C2M_PAN_BLOCK_PIX + tid;
    bool live[C2M_PAN_PPT];
    int sem[C2M_PAN_PPT];
#pragma unroll
    for (int j = 0; j < C2M_PAN_PPT; ++j) { live[j] = q0 + j * 256 < HW; sem[j] = 0; }
    if (p.logits) {
        const float* __restrict__ lg = p.logits + (long)n * p.C * HW;
        float best[C2M_PAN_PPT];
#pragma unroll
        for (int j = 0; j < C2M_PAN_PPT; ++j) best[j] = live[j] ? lg[q0 + j * 256] : 0.f;
        for (int c = 1; c < p.C; ++c) {
            const float* __restrict__ plane = lg + (long)c * HW;
#pragma unroll
            for (int j = 0; j < C2M_PAN_PPT; ++j) {
                if (live[j]) {
                    const float v = plane[q0 + j * 256];
                    if (v > best[j] || (v != v && best[j] == best[j])) { best[j] = v; sem[j] = c; }   // first maximum; NaN is one
                }
            }
        }
    } else {
        const uint8_t* __restrict__ lb = p.labels + n * HW;
#pragma unroll
        for (int j = 0; j < C2M_PAN_PPT; ++j) if (live[j]) sem[j] = lb[q0 + j * 256];
    }

    const float* __restrict__ off = p.offset + (long)n * 2 * HW;
    float py[C2M_PAN_PPT], px[C2M_PAN_PPT], bd[C2M_PAN_PPT];
    int bk[C2M_PAN_PPT], ord[C2M_PAN_PPT];
    bool any = false;
#pragma unroll
    for (int j = 0; j < C2M_PAN_PPT; ++j) {
        ord[j] = live[j] ? (int)s_tab[sem[j]] : 0;                        // 0: not a thing (or no pixel)
        if (ord[j] > p.T) ord[j] = 0;                                     // a table entry past the thing list votes nowhere
        py[j] = px[j] = 0.f;
        bd[j] = __builtin_inff();
        bk[j] = 0;
        if (ord[j] && m > 0) {
            const long q = q0 + j * 256;
            const int y = (int)(q / p.W), x = (int)(q - (long)y * p.W);
            py[j] = (float)y + off[q];                                    // the point the pixel votes for, rounded to fp32 as
            px[j] = (float)x + off[HW + q];                               // the reference's coord + offsets
            any = true;
        }
    }
    if (any) {
        for (int k = 0; k < m; ++k) {
            const float2 c = s_ctr[k];                                    // one LDS broadcast read for 4 pixels
#pragma unroll
            for (int j = 0; j < C2M_PAN_PPT; ++j) {
                const float d = c.x - py[j], e = c.y - px[j];
                const float dist = d * d + e * e;
                if (dist < bd[j]) { bd[j] = dist; bk[j] = k; }            // strict: the first of equally near centres wins
            }
        }
    }
    int* __restrict__ votes = p.votes + (long)n * p.top_k * p.T;
#pragma unroll
    for (int j = 0; j < C2M_PAN_PPT; ++j) {
        const bool claimed = ord[j] && m > 0;
        if (live[j]) {
            const long q = n * HW + q0 + j * 256;
            p.semantic[q] = (uint8_t)sem[j];
            p.raw[q] = claimed ? bk[j] + 1 : 0;
        }
        wave_merge_add(votes, bk[j] * p.T + ord[j] - 1, claimed);         // every thread arrives here, live or not
        wave_merge_add(s_area, sem[j], live[j] && !ord[j]);
    }
    __syncthreads();
    const int a = s_area[tid];
    if (a) atomicAdd(p.area + (long)n * 256 + tid, a);
}

// ------------------------------------------------------------------------------------------------ merge
__global__ __launch_bounds__(256) void pan_merge_kernel(const int* __restrict__ votes, const int* __restrict__ area,
                                                        const int* __restrict__ center_count,
                                                        const uint8_t* __restrict__ class_table,
                                                        const int* __restrict__ thing_classes, int* __restrict__ ktab,
                                                        int* __restrict__ stab, int top_k, int T, int divisor, int stuff_area,
                                                        int void_label) {
    __shared__ int s_val[C2M_PAN_MAX_TOPK];
    __shared__ int s_cnt[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int m = min(max(center_count[n], 0), top_k);
    for (int k = tid; k < m; k += 256) {
        const int* __restrict__ v = votes + ((long)n * top_k + k) * T;
        int best = 0, cls = -1;
        for (int t = 0; t < T; ++t)                                       // thing classes ascending: a tie keeps the smaller class
            if (v[t] > best) { best = v[t]; cls = thing_classes[t] & 255; }
        s_val[k] = cls;
    }
    s_cnt[tid] = 0;
    __syncthreads();
    if (tid == 0) {
        for (int k = 0; k < m; ++k) {                                     // serial: the numbering follows the centre order
            const int cls = s_val[k];
            s_val[k] = cls >= 0 ? cls * divisor + (++s_cnt[cls]) : void_label;
        }
    }
    __syncthreads();
    for (int k = tid; k < top_k; k += 256) ktab[(long)n * top_k + k] = k < m ? s_val[k] : void_label;
    stab[(long)n * 256 + tid] = (!class_table[tid] && area[(long)n * 256 + tid] >= stuff_area) ? tid * divisor : void_label;
}

// ------------------------------------------------------------------------------------------------ paint
__global__ __launch_bounds__(256) void pan_paint_kernel(const uint8_t* __restrict__ semantic, int* __restrict__ panoptic,
                                                        int* __restrict__ instance, const int* __restrict__ ktab,
                                                        const int* __restrict__ stab, const uint8_t* __restrict__ class_table,
                                                        long HW, int top_k, int blocks_per_img, int void_label, int void_inst) {
    __shared__ int s_k[C2M_PAN_MAX_TOPK];
    __shared__ int s_st[256];
    __shared__ unsigned char s_tab[256];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / blocks_per_img, blk = blockIdx.x - n * blocks_per_img;
    for (int k = tid; k < top_k; k += 256) s_k[k] = ktab[(long)n * top_k + k];
    s_st[tid] = stab[(long)n * 256 + tid];
    s_tab[tid] = class_table[tid];
    __syncthreads();
    const long q0 = (long)blk * C2M_PAN_BLOCK_PIX + tid;
#pragma unroll
    for (int j = 0; j < C2M_PAN_PPT; ++j) {
        const long ql = q0 + j * 256;
        if (ql < HW) {
            const long q = n * HW + ql;
            const int sem = semantic[q], raw = panoptic[q];
            int pan, ins;
            if (raw > 0) {
                pan = s_k[min(raw, top_k) - 1];
                ins = pan;
            } else {
                pan = s_tab[sem] ? void_label : s_st[sem];
                ins = pan == void_label ? void_inst : sem;
            }
            panoptic[q] = pan;
            instance[q] = ins;
        }
    }
}

// ------------------------------------------------------------------------------------------------ entry
C2M_API int c2m_panoptic_maps(const float* logits, const uint8_t* labels, int C, const float* center, const float* offset,
                              const uint8_t* class_table, const int32_t* thing_classes, int n_things, uint8_t* semantic,
                              int32_t* instance, int32_t* panoptic, int32_t* centers, int32_t* center_count, void* workspace,
                              long workspace_bytes, int N, int H, int W, float threshold, int nms_kernel, int top_k,
                              int label_divisor, int stuff_area, int ignore_label, void* stream) {
    C2M_ENTER();
    if (N < 0 || H < 1 || W < 1) return (int)hipErrorInvalidValue;
    const long HW = (long)H * W;
    if (HW >= (1L << 31)) return (int)hipErrorInvalidValue;
    if ((logits != nullptr) == (labels != nullptr)) return (int)hipErrorInvalidValue;
    if (logits && (C < 1 || C > 256)) return (int)hipErrorInvalidValue;
    if (nms_kernel < 1 || nms_kernel > 2 * C2M_PAN_MAX_R + 1 || nms_kernel % 2 == 0) return (int)hipErrorInvalidValue;
    if (top_k < 1 || top_k > C2M_PAN_MAX_TOPK || n_things < 0 || n_things > 255) return (int)hipErrorInvalidValue;
    if (!(threshold >= 0.f)) return (int)hipErrorInvalidValue;                                 // NaN included
    if (label_divisor <= top_k || ignore_label < 0 || ignore_label > 255 ||
        256L * label_divisor >= (1L << 31))
        return (int)hipErrorInvalidValue;
    if (N == 0) return 0;
    if (!center || !offset || !class_table || (n_things && !thing_classes) || !semantic || !instance || !panoptic || !centers ||
        !center_count || !workspace)
        return (int)hipErrorInvalidValue;
    const PanWork w = pan_work(workspace, N, HW, top_k, n_things);
    if (workspace_bytes < w.words * 4 || !c2m_aligned(4, workspace)) return (int)hipErrorInvalidValue;
    const int tiles_x = c2m_cdiv(W, C2M_PAN_TW), tiles_y = c2m_cdiv(H, C2M_PAN_TH);
    const long tiles = (long)tiles_x * tiles_y;
    const long bpi = (HW + C2M_PAN_BLOCK_PIX - 1) / C2M_PAN_BLOCK_PIX;
    if (tiles * N >= (1L << 31) || bpi * N >= (1L << 31)) return (int)hipErrorInvalidValue;

    hipStream_t s = (hipStream_t)stream;
    hipError_t e = c2m_zero_async(workspace, w.zero_words * 4, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pan_candidates_kernel, dim3((unsigned)(tiles * N)), dim3(256), 0, s, center, w.cand_count, w.cand_list, H,
                       W, tiles_x, (int)tiles, threshold, nms_kernel / 2);
    C2M_LAUNCH_CHECK();
    hipLaunchKernelGGL(pan_select_kernel, dim3(N), dim3(1024), 0, s, center, w.cand_count, w.cand_list, centers, center_count, HW,
                       W, top_k);
    C2M_LAUNCH_CHECK();
    const PanGroupP g{logits, labels, offset, centers, center_count, class_table, semantic, panoptic, w.votes, w.area,
                      HW, C, W, top_k, n_things, (int)bpi};
    hipLaunchKernelGGL(pan_group_kernel, dim3((unsigned)(bpi * N)), dim3(256), 0, s, g);
    C2M_LAUNCH_CHECK();
    hipLaunchKernelGGL(pan_merge_kernel, dim3(N), dim3(256), 0, s, w.votes, w.area, center_count, class_table, thing_classes,
                       w.ktab, w.stab, top_k, n_things, label_divisor, stuff_area, ignore_label * label_divisor);
    C2M_LAUNCH_CHECK();
    hipLaunchKernelGGL(pan_paint_kernel, dim3((unsigned)(bpi * N)), dim3(256), 0, s, semantic, panoptic, instance, w.ktab, w.stab,
                       class_table, HW, top_k, (int)bpi, ignore_label * label_divisor, ignore_label);
    return (int)hipGetLastError();
}
