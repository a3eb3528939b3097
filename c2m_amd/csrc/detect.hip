// detect.hip -- everything the detector metric does after the YOLOv3 heads, and the frame preprocessing in front of them.
// Reference (per object, batch 1, decode on the device then a Python loop on the host):
//   src/utils/utils_yolov3.py:69-85              nearest x s, F.pad to 416             -> c2m_detect_input
//   src/modules/networks/yolo_v3/models.py:135-178, utils/utils.py:235-248
//                                                YOLOLayer decode, conf filter, class  -> c2m_yolo_candidates
//   utils/utils.py:250-262                       the suppression-and-merge loop        -> c2m_nms_merge
//   src/utils/utils_yolov3.py:13-49,88-138       find_best_detection + the error       -> c2m_match_detections
//
// No float atomics and no atomic cursor anywhere: the compaction is counts -> prefix -> scatter, the merge sums run in
// sorted order per thread and then through a fixed shuffle / LDS tree, so every result is bit-repeatable.
// Built with -ffp-contract=off: the decode and the IoU are the reference's fp32 operations one by one.
#include "common.h"

#define C2M_DET_MAX_HEADS 4
#define C2M_DET_MAX_ANCHORS 8
#define C2M_DET_BLOCK 256
#define C2M_NMS_THREADS 256
#define C2M_NMS_LDS_ROWS 2048          // candidates staged in LDS (6 floats each, 48 KB) + 1 flag byte per candidate of any count

// ------------------------------------------------------------------------------------------------------------- input
// out[b, c, y, x] = frame[b, c, y / s, x / s] where that lies inside the frame, else 0 (S x S output).  A frame larger than
// S / s is cropped, which is what F.pad does with a negative pad.
__global__ void detect_input_kernel(const float* __restrict__ src, float* __restrict__ dst, long total, int C, int H, int W,
                                    long sb, long sc, long sh, long sw, int s, int S) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % S);
        const long r = i / S;
        const int y = (int)(r % S);
        const long q = r / S;
        const int c = (int)(q % C);
        const long b = q / C;
        const int sy = y / s, sx = x / s;
        dst[i] = (sy < H && sx < W) ? src[b * sb + c * sc + sy * sh + sx * sw] : 0.f;
    }
}

C2M_API int c2m_detect_input(const float* frame, float* out, int B, int C, int H, int W, long stride_b, long stride_c,
                             long stride_h, long stride_w, int scale, int S, void* stream) {
    C2M_ENTER();
    if (B < 0 || C < 1 || H < 1 || W < 1 || scale < 1 || S < 1 || stride_b < 0 || stride_c < 0 || stride_h < 0 || stride_w < 0)
        return (int)hipErrorInvalidValue;
    const long total = (long)B * C * S * S;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(detect_input_kernel, dim3(c2m_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, frame, out, total, C,
                       H, W, stride_b, stride_c, stride_h, stride_w, scale, S);
    return (int)hipGetLastError();
}

// -------------------------------------------------------------------------------------------------------- candidates
// Box j of an image, in the reference's order: head, anchor, row, column.  Channel k of it is head[n][a * (5 + C) + k][gy][gx].
struct DetHeads {
    const float* p[C2M_DET_MAX_HEADS];
    int g[C2M_DET_MAX_HEADS];                // grid size
    int na[C2M_DET_MAX_HEADS];               // anchors of this head
    int start[C2M_DET_MAX_HEADS + 1];        // first box of each head; start[nheads] = boxes per image
    float stride[C2M_DET_MAX_HEADS];         // image size / grid size
    float aw[C2M_DET_MAX_HEADS][C2M_DET_MAX_ANCHORS], ah[C2M_DET_MAX_HEADS][C2M_DET_MAX_ANCHORS];   // anchor / stride
    int nheads;
};

struct DetBox { const float* base; long plane; int gx, gy, h, a; };      // base: channel 0 of the box, plane: channel stride

__device__ __forceinline__ DetBox det_locate(const DetHeads& hd, int C, long n, int j) {
    int h = 0;
#pragma unroll
    for (int k = 1; k < C2M_DET_MAX_HEADS; ++k)
        if (k < hd.nheads && j >= hd.start[k]) h = k;
    const int g = hd.g[h];
    int r = j - hd.start[h];
    DetBox b;
    b.h = h;
    b.gx = r % g;
    r /= g;
    b.gy = r % g;
    b.a = r / g;
    b.plane = (long)g * g;
    b.base = hd.p[h] + ((n * hd.na[h] + b.a) * (long)(5 + C)) * b.plane + (long)b.gy * g + b.gx;
    return b;
}

__device__ __forceinline__ float det_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// pass 1: how many boxes of each 256-box block reach conf_thres
__global__ __launch_bounds__(C2M_DET_BLOCK) void yolo_count_kernel(DetHeads hd, int C, int blocks_per_image, float conf_thres,
                                                                   int* __restrict__ block_count) {
    __shared__ int wsum[C2M_DET_BLOCK / 64];
    const long n = blockIdx.x / blocks_per_image;
    const int blk = blockIdx.x % blocks_per_image;
    const int nb = hd.start[hd.nheads];
    const int j = blk * C2M_DET_BLOCK + threadIdx.x;
    bool pass = false;
    if (j < nb) {
        const DetBox b = det_locate(hd, C, n, j);
        pass = det_sigmoid(b.base[4 * b.plane]) >= conf_thres;
    }
    int passing;
    (void)block_rank_256(pass, wsum, passing);
    if (threadIdx.x == 0) block_count[blockIdx.x] = passing;
}

// pass 2: each block sums the counts of the blocks before it (at most 41 at 416 x 416), decodes its passing boxes and writes
// them at base + rank, rank = passing boxes before it in the block (ballot prefix).
__global__ __launch_bounds__(C2M_DET_BLOCK) void yolo_scatter_kernel(DetHeads hd, int C, int blocks_per_image, float conf_thres,
                                                                     const int* __restrict__ block_count, int cap,
                                                                     float* __restrict__ cand, float* __restrict__ score,
                                                                     int* __restrict__ count) {
    __shared__ int wsum[C2M_DET_BLOCK / 64];
    __shared__ int base_s;
    const long n = blockIdx.x / blocks_per_image;
    const int blk = blockIdx.x % blocks_per_image;
    const int nb = hd.start[hd.nheads];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (wave == 0) {                         // integer sums: any order gives the same value
        int s = 0, t = 0;
        for (int k = lane; k < blocks_per_image; k += 64) {
            const int v = block_count[n * blocks_per_image + k];
            t += v;
            if (k < blk) s += v;
        }
        s = wave_sum(s);
        t = wave_sum(t);
        if (lane == 0) {
            base_s = s;
            if (blk == 0) count[n] = t;
        }
    }
    const int j = blk * C2M_DET_BLOCK + tid;
    bool pass = false;
    DetBox b;
    float conf = 0.f;
    if (j < nb) {
        b = det_locate(hd, C, n, j);
        conf = det_sigmoid(b.base[4 * b.plane]);
        pass = conf >= conf_thres;
    }
    int passing;
    int rank = block_rank_256(pass, wsum, passing);      // its barrier publishes base_s as well
    if (!pass) return;
    rank += base_s;
    if (rank >= cap) return;                 // cannot happen (cap >= boxes per image is checked on the host)
    const float st = hd.stride[b.h];
    const float cx = (det_sigmoid(b.base[0]) + (float)b.gx) * st;
    const float cy = (det_sigmoid(b.base[b.plane]) + (float)b.gy) * st;
    const float w = expf(b.base[2 * b.plane]) * hd.aw[b.h][b.a] * st;
    const float h = expf(b.base[3 * b.plane]) * hd.ah[b.h][b.a] * st;
    float best = det_sigmoid(b.base[5 * b.plane]);
    int cls = 0;
    for (int k = 1; k < C; ++k) {
        const float v = det_sigmoid(b.base[(5 + k) * b.plane]);
        if (v > best) {                      // strict: the lowest index among maxima
            best = v;
            cls = k;
        }
    }
    float* __restrict__ o = cand + (n * cap + rank) * 7;
    o[0] = cx - w / 2;
    o[1] = cy - h / 2;
    o[2] = cx + w / 2;
    o[3] = cy + h / 2;
    o[4] = conf;
    o[5] = best;
    o[6] = (float)cls;
    score[n * cap + rank] = conf * best;
}

// heads: nheads device pointers [N, na * (5 + C), g, g]; anchors: nheads x max_anchors x 2 floats (w, h), ALREADY divided by the
// stride; block_count: N * ceil(boxes / 256) ints of workspace.  score rows beyond count[n] are left as the caller filled them.
C2M_API int c2m_yolo_candidates(const void* const* heads, const int* grid, const int* nanchors, const float* stride,
                                const float* anchors, int max_anchors, int nheads, int N, int C, float conf_thres, int cap,
                                int* block_count, float* cand, float* score, int* count, void* stream) {
    C2M_ENTER();
    if (nheads < 1 || nheads > C2M_DET_MAX_HEADS || N < 0 || C < 1 || cap < 1 || max_anchors < 1 ||
        max_anchors > C2M_DET_MAX_ANCHORS)
        return (int)hipErrorInvalidValue;
    DetHeads hd;
    hd.nheads = nheads;
    long nb = 0;
    for (int h = 0; h < C2M_DET_MAX_HEADS; ++h) {
        const bool on = h < nheads;
        if (on && (grid[h] < 1 || nanchors[h] < 1 || nanchors[h] > max_anchors || heads[h] == nullptr))
            return (int)hipErrorInvalidValue;
        hd.p[h] = on ? (const float*)heads[h] : nullptr;
        hd.g[h] = on ? grid[h] : 1;
        hd.na[h] = on ? nanchors[h] : 1;
        hd.stride[h] = on ? stride[h] : 1.f;
        hd.start[h] = (int)nb;
        for (int a = 0; a < C2M_DET_MAX_ANCHORS; ++a) {
            const bool ok = on && a < nanchors[h];
            hd.aw[h][a] = ok ? anchors[(h * max_anchors + a) * 2] : 0.f;
            hd.ah[h][a] = ok ? anchors[(h * max_anchors + a) * 2 + 1] : 0.f;
        }
        if (on) nb += (long)nanchors[h] * grid[h] * grid[h];
        if (nb > 0x3fffffffL) return (int)hipErrorInvalidValue;
    }
    for (int h = nheads; h <= C2M_DET_MAX_HEADS; ++h) hd.start[h] = (int)nb;
    hd.start[nheads] = (int)nb;
    if (cap < nb) return (int)hipErrorInvalidValue;      // capacity is every box: nothing is ever dropped
    if (N == 0) return 0;
    const int bpi = c2m_cdiv(nb, C2M_DET_BLOCK);
    if ((long)bpi * N > 0x7fffffffL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(yolo_count_kernel, dim3((unsigned)(bpi * N)), dim3(C2M_DET_BLOCK), 0, (hipStream_t)stream, hd, C, bpi,
                       conf_thres, block_count);
    C2M_LAUNCH_CHECK();
    hipLaunchKernelGGL(yolo_scatter_kernel, dim3((unsigned)(bpi * N)), dim3(C2M_DET_BLOCK), 0, (hipStream_t)stream, hd, C, bpi,
                       conf_thres, (const int*)block_count, cap, cand, score, count);
    return (int)hipGetLastError();
}

// --------------------------------------------------------------------------------------------------------------- NMS
// One workgroup per image.  srt: the image's candidates in descending score order.  State: one alive byte per candidate in
// LDS.  Every round: the head is the first alive candidate; every alive candidate of its class whose IoU with the head's
// ORIGINAL box exceeds nms_thres joins the invalid set; the output row is the head's row with the box replaced by the
// confidence-weighted mean of the set; the set -- and always the head -- is removed.  The next head is found in the same pass
// (minimum surviving index), so a round is one sweep over [head, n) and three barriers.
// Sums: thread t adds candidates head + t, head + t + 256, ... in that order, then a shuffle tree in the wave and the four
// wave totals in wave order -- one fixed tree for a given (head, n).
__global__ __launch_bounds__(C2M_NMS_THREADS) void nms_merge_kernel(const float* __restrict__ srt, const int* __restrict__ count,
                                                                    int cap, float nms_thres, float* __restrict__ dets,
                                                                    int* __restrict__ kept) {
    extern __shared__ unsigned char nms_lds[];
    __shared__ float red[C2M_NMS_THREADS / 64][5];
    __shared__ int red_next[C2M_NMS_THREADS / 64];
    const long img = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n = count[img];
    n = n < 0 ? 0 : n > cap ? cap : n;
    const float* __restrict__ rows = srt + img * (long)cap * 7;
    const bool staged = n <= C2M_NMS_LDS_ROWS;
    // LDS layout.  Staged (n <= C2M_NMS_LDS_ROWS): six arrays of n floats PACKED one after the other (x1, y1, x2, y2, conf, class at
    // soa + k * n, not at k * C2M_NMS_LDS_ROWS), then -- at the FIXED offset 6 * C2M_NMS_LDS_ROWS * 4, past the largest packing -- the
    // alive bytes.  Not staged: the alive bytes start at offset 0 and the rows are read from global memory with stride 7.
    float* __restrict__ soa = (float*)nms_lds;
    unsigned char* __restrict__ alive = nms_lds + (staged ? (size_t)6 * C2M_NMS_LDS_ROWS * 4 : 0);
    const float* X1 = staged ? soa : rows;
    const float* Y1 = staged ? soa + n : rows + 1;
    const float* X2 = staged ? soa + 2 * n : rows + 2;
    const float* Y2 = staged ? soa + 3 * n : rows + 3;
    const float* CF = staged ? soa + 4 * n : rows + 4;
    const float* CL = staged ? soa + 5 * n : rows + 6;
    const int es = staged ? 1 : 7;
    for (int i = tid; i < n; i += C2M_NMS_THREADS) {
        alive[i] = 1;
        if (staged) {
            const float* r = rows + (long)i * 7;
            soa[i] = r[0];
            soa[n + i] = r[1];
            soa[2 * n + i] = r[2];
            soa[3 * n + i] = r[3];
            soa[4 * n + i] = r[4];
            soa[5 * n + i] = r[6];
        }
    }
    __syncthreads();
    float* __restrict__ out = dets + img * (long)cap * 7;
    int head = 0, k = 0;
    while (head < n) {
        const float hx1 = X1[(long)head * es], hy1 = Y1[(long)head * es], hx2 = X2[(long)head * es], hy2 = Y2[(long)head * es];
        const float hcl = CL[(long)head * es];
        const float harea = (hx2 - hx1 + 1.f) * (hy2 - hy1 + 1.f);
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, sw = 0.f;
        int next = n;
        for (int i = head + tid; i < n; i += C2M_NMS_THREADS) {
            if (!alive[i]) continue;
            const long e = (long)i * es;
            const float x1 = X1[e], y1 = Y1[e], x2 = X2[e], y2 = Y2[e];
            const float iw = fminf(hx2, x2) - fmaxf(hx1, x1) + 1.f, ih = fminf(hy2, y2) - fmaxf(hy1, y1) + 1.f;
            const float inter = (iw > 0.f ? iw : 0.f) * (ih > 0.f ? ih : 0.f);
            const float area = (x2 - x1 + 1.f) * (y2 - y1 + 1.f);
            const float iou = inter / (harea + area - inter + 1e-16f);
            const bool invalid = iou > nms_thres && CL[e] == hcl;
            if (invalid) {
                const float w = CF[e];
                s0 += w * x1;
                s1 += w * y1;
                s2 += w * x2;
                s3 += w * y2;
                sw += w;
            }
            if (invalid || i == head) alive[i] = 0;          // the head always leaves, whatever its box holds
            else if (i < next) next = i;                     // ascending per thread: the first survivor it meets
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s0 += __shfl_down(s0, o, 64);
            s1 += __shfl_down(s1, o, 64);
            s2 += __shfl_down(s2, o, 64);
            s3 += __shfl_down(s3, o, 64);
            sw += __shfl_down(sw, o, 64);
            const int other = __shfl_down(next, o, 64);
            next = other < next ? other : next;
        }
        if (lane == 0) {
            red[wave][0] = s0;
            red[wave][1] = s1;
            red[wave][2] = s2;
            red[wave][3] = s3;
            red[wave][4] = sw;
            red_next[wave] = next;
        }
        __syncthreads();
        if (tid < 4) {
            float s = red[0][tid];
            float w = red[0][4];
#pragma unroll
            for (int v = 1; v < C2M_NMS_THREADS / 64; ++v) {
                s += red[v][tid];
                w += red[v][4];
            }
            out[(long)k * 7 + tid] = s / w;
        } else if (tid < 7) {
            out[(long)k * 7 + tid] = rows[(long)head * 7 + tid];
        }
        int nx = red_next[0];
#pragma unroll
        for (int v = 1; v < C2M_NMS_THREADS / 64; ++v) nx = red_next[v] < nx ? red_next[v] : nx;
        __syncthreads();                                     // red[] is rewritten by the next round
        head = nx;
        ++k;
    }
    if (tid == 0) kept[img] = k;
}

C2M_API int c2m_nms_merge(const float* sorted, const int* count, int N, int cap, float nms_thres, float* dets, int* kept,
                          void* stream) {
    C2M_ENTER();
    if (N < 0 || cap < 1) return (int)hipErrorInvalidValue;
    if (N == 0) return 0;
    const size_t lds = (size_t)6 * C2M_NMS_LDS_ROWS * 4 + (((size_t)cap + 15) & ~(size_t)15);
    if (lds > 150 * 1024) return (int)hipErrorInvalidValue;                  // ~100 000 candidates per image
    if (lds > 64 * 1024 - 64) {                                              // beyond the default limit (cap > ~16 000) only; 60 KB at 416
        hipError_t e = hipFuncSetAttribute((const void*)nms_merge_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(nms_merge_kernel, dim3((unsigned)N), dim3(C2M_NMS_THREADS), lds, (hipStream_t)stream, sorted, count, cap,
                       nms_thres, dets, kept);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------- match
// find_best_detection: the truncated detection that overlaps the truncated roi by more than half the roi, largest overlap
// first, first on ties.  Integer arithmetic decides (2 dx dy > height width); areas compare in double as Python does.
__device__ bool det_best(const float* __restrict__ d, int nd, int rymin, int rxmin, int rymax, int rxmax, double min_area,
                         int* __restrict__ box) {
    const long hw = (long)(rymax - rymin + 1) * (long)(rxmax - rxmin + 1);
    long best = -1;
    for (int i = 0; i < nd; ++i) {
        const float x1 = d[i * 7], y1 = d[i * 7 + 1], x2 = d[i * 7 + 2], y2 = d[i * 7 + 3];
        if (!(x1 > 0.f && y1 > 0.f && x2 > 0.f && y2 > 0.f)) continue;
        if (!(x1 < 2e9f && y1 < 2e9f && x2 < 2e9f && y2 < 2e9f)) continue;      // int() of it would not fit (never a real box)
        const int iy1 = (int)y1, ix1 = (int)x1, iy2 = (int)y2, ix2 = (int)x2;
        const long dx = (long)min(rxmax, ix2) - (long)max(rxmin, ix1), dy = (long)min(rymax, iy2) - (long)max(rymin, iy1);
        if (dx < 0 || dy < 0 || 2 * dx * dy <= hw) continue;
        const float bw = x2 - x1, bh = y2 - y1;
        if ((double)(bh * bw) < min_area) continue;
        if (dx * dy > best) {
            best = dx * dy;
            box[0] = iy1;
            box[1] = ix1;
            box[2] = iy2;
            box[3] = ix2;
        }
    }
    return best >= 0;
}

// flags [M][3] = skipped (or -1: an index outside the graph / batch), gt_found, pred_found; boxes [M][8] = gt, pred as
// (y1, x1, y2, x2); err [M][2] = mse, mse_normalized (double, as the reference's Python floats).
__global__ void match_detections_kernel(const float* __restrict__ dets, const int* __restrict__ kept, int cap, int B,
                                        const long* __restrict__ idx, int M, const float* __restrict__ roi, int T,
                                        const float* __restrict__ xfeat, int tin, int F, const long* __restrict__ batch,
                                        long nodes, int scale, int h, int w, double skip_area, double min_area,
                                        int* __restrict__ flags, int* __restrict__ boxes, double* __restrict__ err) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    int* fl = flags + m * 3;
    int* bx = boxes + m * 8;
    fl[0] = fl[1] = fl[2] = 0;
    for (int k = 0; k < 8; ++k) bx[k] = 0;
    err[2 * m] = err[2 * m + 1] = 0.0;
    const long id = idx[m];
    if (id < 0 || id >= nodes) {
        fl[0] = -1;
        return;
    }
    const long b = batch[id];
    if (b < 0 || b >= B) {
        fl[0] = -1;
        return;
    }
    const float* r = roi + (id * T + (T - 1)) * 4;                              // xmin, xmax, ymin, ymax
    const float fs = (float)scale;
    const float q0 = r[0] * fs, q1 = r[1] * fs, q2 = r[2] * fs, q3 = r[3] * fs;
    if (!(fabsf(q0) < 2e9f && fabsf(q1) < 2e9f && fabsf(q2) < 2e9f && fabsf(q3) < 2e9f)) {
        fl[0] = -1;
        return;
    }
    const int xmin = (int)q0, xmax = (int)q1, ymin = (int)q2, ymax = (int)q3;
    if ((double)((long)(ymax - ymin) * (long)(xmax - xmin)) < skip_area) {
        fl[0] = 1;
        return;
    }
    const int kg = min(max(kept[b], 0), cap), kp = min(max(kept[B + b], 0), cap);
    if (!det_best(dets + b * (long)cap * 7, kg, ymin, xmin, ymax, xmax, min_area, bx)) return;
    fl[1] = 1;
    if (!det_best(dets + (B + b) * (long)cap * 7, kp, ymin, xmin, ymax, xmax, min_area, bx + 4)) return;
    fl[2] = 1;
    const float* xn = xfeat + (id * tin + (tin - 1)) * (long)F;
    const float sy = (xn[0] + 1.f) / 2.f * (float)h, sx = (xn[1] + 1.f) / 2.f * (float)w;
    const double gy = (ymin + ymax) / 2.0, gx = (xmin + xmax) / 2.0;
    const double py = (bx[4] + bx[6]) / 2.0, px = (bx[5] + bx[7]) / 2.0;
    const double s_y = fabsf(sy) < 2e9f ? (double)(int)sy : 0.0, s_x = fabsf(sx) < 2e9f ? (double)(int)sx : 0.0;
    const double mse = sqrt((py - gy) * (py - gy) + (px - gx) * (px - gx));
    double nf = sqrt((s_y - gy) * (s_y - gy) + (s_x - gx) * (s_x - gx));
    nf = nf > 0.0 ? nf : 1.0;
    err[2 * m] = mse;
    err[2 * m + 1] = mse / (nf + 1e-06);
}

C2M_API int c2m_match_detections(const float* dets, const int* kept, int cap, int B, const long* index, int M, const float* roi,
                                 int T, const float* x, int tin, int F, const long* batch, long nodes, int scale, int h, int w,
                                 double skip_area, double min_area, int* flags, int* boxes, double* err, void* stream) {
    C2M_ENTER();
    if (cap < 1 || B < 1 || M < 0 || T < 1 || tin < 1 || F < 2 || nodes < 0 || scale < 1 || h < 1 || w < 1)
        return (int)hipErrorInvalidValue;
    if (M == 0) return 0;
    hipLaunchKernelGGL(match_detections_kernel, dim3(c2m_cdiv(M, 64)), dim3(64), 0, (hipStream_t)stream, dets, kept, cap, B,
                       index, M, roi, T, x, tin, F, batch, nodes, scale, h, w, skip_area, min_area, flags, boxes, err);
    return (int)hipGetLastError();
}
