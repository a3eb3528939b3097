// data_prep.hip -- the input-pipeline stage just upstream of the hot path, on the device.
// Reference (CPU, per sample, PIL arrays -> tensors): src/datasets/cityscapes.py
//   :30-33,59-61  image frames     ToTensor(): uint8 HWC -> float CHW / 255, frames stacked along dim 1  -> video [B,3,T,H,W]
//   :35-41,62-70  label-id maps    ToTensor()*255 == i for i in 0..10 (bg) / 11..19 (fg)                -> bg/fg one-hot masks
//   :212-216,255,262-265 occlusion PNGs  ToTensor()/255 -> clip_mask(> 0.5)                             -> target_bw_occ
//   :219-231,254,261     .flo flows      HWC -> CHW (no rescale at the native size), stacked over time  -> target_bw_of
// The decoded, resized arrays (PIL's job) are uploaded once as uint8 / float; everything after that runs here, so the host
// never builds the 20-channel one-hot volumes (20x the bytes of the label map).
// (v/255)*255 == v holds exactly in fp32 for every uint8 v, so the one-hot test is an integer compare.
#include "common.h"
#include "instance_compact.h"

// frames [B][T][H][W][3] uint8 -> video [B][3][T][H][W] float, x / 255 (true division, as Tensor.div(255))
__global__ void prep_video_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, long BT, int T, long HW) {
    const long total = BT * HW;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long bt = i / HW, p = i - bt * HW;
        const long b = bt / T, t = bt - b * T;
        const uint8_t* __restrict__ s = src + i * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[((b * 3 + c) * T + t) * HW + p] = (float)s[c] / 255.0f;
    }
}

// labels [B][T][H][W] uint8 -> bg [B][11][T][H][W], fg [B][9][T][H][W] one-hot floats
__global__ void prep_seg_onehot_kernel(const uint8_t* __restrict__ lab, float* __restrict__ bg, float* __restrict__ fg,
                                       long BT, int T, long HW) {
    const long total = BT * HW;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long bt = i / HW, p = i - bt * HW;
        const long b = bt / T, t = bt - b * T;
        const int v = lab[i];
#pragma unroll
        for (int c = 0; c < 11; ++c) bg[((b * 11 + c) * T + t) * HW + p] = v == c ? 1.0f : 0.0f;
#pragma unroll
        for (int c = 0; c < 9; ++c) fg[((b * 9 + c) * T + t) * HW + p] = v == 11 + c ? 1.0f : 0.0f;
    }
}

// occ [B][T][H][W] uint8 -> [B][1][T][H][W] float: (v / 255 > 0.5) ? 1 : 0;  flow [B][T][H][W][2] -> [B][2][T][H][W]
__global__ void prep_flow_occ_kernel(const uint8_t* __restrict__ occ, const float* __restrict__ flo,
                                     float* __restrict__ occ_out, float* __restrict__ flow_out, long BT, int T, long HW) {
    const long total = BT * HW;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long bt = i / HW, p = i - bt * HW;
        const long b = bt / T, t = bt - b * T;
        if (occ) occ_out[i] = ((float)occ[i] / 255.0f > 0.5f) ? 1.0f : 0.0f;
        if (flo) {
            flow_out[((b * 2 + 0) * T + t) * HW + p] = flo[i * 2 + 0];
            flow_out[((b * 2 + 1) * T + t) * HW + p] = flo[i * 2 + 1];
        }
    }
}

C2M_API int c2m_prep_video(const uint8_t* frames, float* video, int B, int T, int H, int W, void* stream) {
    C2M_ENTER();
    const long total = (long)B * T * H * W;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(prep_video_kernel, dim3(c2m_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, frames, video,
                       (long)B * T, T, (long)H * W);
    return (int)hipGetLastError();
}

C2M_API int c2m_prep_seg_onehot(const uint8_t* labels, float* bg, float* fg, int B, int T, int H, int W, void* stream) {
    C2M_ENTER();
    const long total = (long)B * T * H * W;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(prep_seg_onehot_kernel, dim3(c2m_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, labels, bg,
                       fg, (long)B * T, T, (long)H * W);
    return (int)hipGetLastError();
}

C2M_API int c2m_prep_flow_occ(const uint8_t* occ, const float* flow_hwc, float* occ_out, float* flow_out, int B, int T,
                              int H, int W, void* stream) {
    C2M_ENTER();
    const long total = (long)B * T * H * W;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(prep_flow_occ_kernel, dim3(c2m_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, occ, flow_hwc,
                       occ_out, flow_out, (long)B * T, T, (long)H * W);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------- per-instance boxes (click-to-move)
// The object graph of an interactive run is built from the instance maps of the input frames instead of tracker files:
// for every id in [id_lo, id_hi) and every (sample, input frame) plane, pixel count and x / y extent.  Integer atomics
// only (add / min / max are order-independent, so the table is bit-repeatable), and few of them: one wave owns a
// 64-column strip of `rows` rows; every lane keeps its column's current vertical run (id, count, y extent) in registers
// and the wave flushes only when some lane's id changes.  Rows are loaded C2M_INST_BATCH at a time (independent loads in
// flight), and the host shortens the strips of small frames so that enough waves run.  A flush merges the runs of neighbouring lanes that
// carry the same id (segmented reduction over shuffles) and only the first lane of each merged run touches memory.
#define C2M_INST_ROWS 32
#define C2M_INST_BATCH 8

struct InstRun { int id, cnt, ymin, ymax; };

__device__ __forceinline__ void inst_flush(InstRun r, int x, int lane, int* __restrict__ tab, int id_lo) {
    const int prev = __shfl_up(r.id, 1, 64);
    const bool head = lane == 0 || prev != r.id;
    const unsigned long long heads = __ballot(head);
    const unsigned long long later = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
    const int end = later ? __ffsll((long long)later) - 2 : 63;          // last lane of this lane's run
    int cnt = r.cnt, ymin = r.ymin, ymax = r.ymax;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {                                   // segmented suffix reduction within the run
        const int c = __shfl_down(cnt, o, 64), lo = __shfl_down(ymin, o, 64), hi = __shfl_down(ymax, o, 64);
        if (lane + o <= end) { cnt += c; ymin = min(ymin, lo); ymax = max(ymax, hi); }
    }
    const int xmax = __shfl(x, end, 64);
    if (head && r.id >= 0) {
        int* __restrict__ e = tab + (long)(r.id - id_lo) * 5;
        atomicAdd(e + 0, cnt);
        atomicMin(e + 1, x);
        atomicMax(e + 2, xmax);
        atomicMin(e + 3, ymin);
        atomicMax(e + 4, ymax);
    }
}

// instance [B][T][H][W] int32; planes p = b * t_in + t for t < t_in; table [B*t_in][nid][5] (initialised by the kernel below).
// id_lo >= 0, so -1 can stand for every ignored id.
__global__ void instance_stats_kernel(const int* __restrict__ inst, int* __restrict__ table, int T, int t_in, int H,
                                      int W, int id_lo, int id_hi, int rows, int strips, int chunks, long waves) {
    const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (wave >= waves) return;                                            // whole waves only
    const int lane = threadIdx.x & 63;
    const int strip = (int)(wave % strips);
    const long r = wave / strips;
    const int chunk = (int)(r % chunks);
    const long plane = r / chunks;
    const long b = plane / t_in, t = plane - b * t_in;
    const int x = strip * 64 + lane;
    const int y0 = chunk * rows, y1 = min(y0 + rows, H);
    const int* __restrict__ src = inst + (b * T + t) * (long)H * W;
    int* __restrict__ tab = table + plane * (long)(id_hi - id_lo) * 5;
    auto load = [&](int y) {
        if (x >= W) return -1;
        const int v = src[(long)y * W + x];
        return (v >= id_lo && v < id_hi) ? v : -1;                       // every ignored id is one class: no flush between them
    };
    InstRun run{load(y0), 1, y0, y0};
    for (int yb = y0 + 1; yb < y1; yb += C2M_INST_BATCH) {
        int v[C2M_INST_BATCH];
#pragma unroll
        for (int k = 0; k < C2M_INST_BATCH; ++k) v[k] = yb + k < y1 ? load(yb + k) : -1;
#pragma unroll
        for (int k = 0; k < C2M_INST_BATCH; ++k) {
            const int y = yb + k;
            if (y >= y1) break;                                           // wave-uniform
            if (__ballot(v[k] != run.id)) {
                inst_flush(run, x, lane, tab, id_lo);
                run = InstRun{v[k], 1, y, y};
            } else {
                run.cnt += 1;
                run.ymax = y;
            }
        }
    }
    inst_flush(run, x, lane, tab, id_lo);
}

__global__ void instance_table_init_kernel(int* __restrict__ table, long entries) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < entries; i += (long)gridDim.x * blockDim.x) {
        const int f = (int)(i % 5);
        table[i] = f == 0 ? 0 : (f == 1 || f == 3) ? 0x7fffffff : -1;    // count, x_min, x_max, y_min, y_max
    }
}

C2M_API int c2m_instance_stats(const int32_t* instance, int32_t* table, int B, int T, int t_in, int H, int W, int id_lo,
                               int id_hi, void* stream) {
    C2M_ENTER();
    if (B < 0 || t_in < 1 || t_in > T || H < 0 || W < 0 || id_lo < 0 || id_hi <= id_lo) return (int)hipErrorInvalidValue;
    const long planes = (long)B * t_in, entries = planes * (id_hi - id_lo) * 5;
    if (entries <= 0) return 0;
    hipLaunchKernelGGL(instance_table_init_kernel, dim3(c2m_grid(entries, 256)), dim3(256), 0, (hipStream_t)stream, table,
                       entries);
    C2M_LAUNCH_CHECK();
    const int strips = c2m_cdiv(W, 64);
    int rows = C2M_INST_ROWS;                                             // >= 8192 waves where the frame allows it
    while (rows > C2M_INST_BATCH && planes * strips * c2m_cdiv(H, rows) < 8192) rows /= 2;
    const int chunks = c2m_cdiv(H, rows);
    const long waves = planes * strips * chunks;
    if (waves <= 0) return 0;
    hipLaunchKernelGGL(instance_stats_kernel, dim3(c2m_cdiv(waves, 4)), dim3(256), 0, (hipStream_t)stream, instance, table,
                       T, t_in, H, W, id_lo, id_hi, rows, strips, chunks, waves);
    return (int)hipGetLastError();
}

// The objects of a sample: the ids present in EVERY input frame with count >= min_pixels, in ascending id order
// (instance_compact.h; one workgroup per sample).  ids [B][max_nodes], boxes [B][max_nodes][t_in][4], count [B], overflow [B].
// Slots past count are zero.  No cap on max_nodes.
C2M_API int c2m_instance_compact(const int32_t* table, int32_t* ids, int32_t* boxes, int32_t* count, int32_t* overflow,
                                 int B, int t_in, int nid, int id_lo, int min_pixels, int max_nodes, void* stream) {
    C2M_ENTER();
    if (B < 0 || t_in < 1 || nid < 1 || min_pixels < 1 || max_nodes < 1) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    hipLaunchKernelGGL(instance_compact_kernel<false>, dim3(B), dim3(256), 0, (hipStream_t)stream, table, ids, boxes,
                       (int*)nullptr, count, overflow, t_in, nid, id_lo, min_pixels, max_nodes, 0);
    return (int)hipGetLastError();
}
