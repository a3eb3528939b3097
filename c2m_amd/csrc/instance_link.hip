// Associating the objects of two instance maps (gfx950): which object of a frame is which object of a reference frame, when
// the two maps do not share ids.  The reference has no counterpart: it reads an id column per frame from tracker files
// (cityscapes.py:79-199); c2m_amd.tracking builds the same [T, N] id table from maps and flows with these three entries.
//
//   c2m_instance_slots    per plane of the c2m_instance_stats table, the ids with count >= min_pixels in ascending order
//                         (the one-plane form of instance_compact_kernel, instance_compact.h: its "in every input frame" rule
//                         is void), their boxes and areas.  An id's position in that list is its SLOT.
//   c2m_instance_overlap  contingency table of two maps: pairs[p][i][j] = number of frame pixels q whose id has frame slot j and
//                         whose SOURCE pixel in the reference map holds an id with reference slot i.  The source pixel is the
//                         one c2m_label_warp reads for q (warp_coord.h: warp_source, border clamp, rintf), or q itself without
//                         a flow.  Row / column max_nodes stand for "no slot".
//   c2m_instance_match    mutual best match by IoU from that table, one wave per plane.
//
// All arithmetic after the source coordinate is integer and the only atomics are int32 adds, so every output is bit-repeatable.
// This file is compiled with -ffp-contract=off (see warp_coord.h).
#include "common.h"
#include "instance_compact.h"
#include "warp_coord.h"

#define C2M_LINK_MAX_NODES 64                  // one wave holds a plane's slots: one lane per slot
#define C2M_LINK_CELLS ((C2M_LINK_MAX_NODES + 1) * (C2M_LINK_MAX_NODES + 1))
#define C2M_LINK_WG_PIXELS 16384               // pixels per workgroup of the overlap kernel (64 per thread)

C2M_API int c2m_instance_link_max_nodes(void) { return C2M_LINK_MAX_NODES; }

// ------------------------------------------------------------------------------------------------ slots
// The one-plane form of the compaction of instance_compact.h: one workgroup per plane, with areas.  table [planes][nid][5]
// (count, x_min, x_max, y_min, y_max); slot_ids [planes][max_nodes] (-1 past count: ids are >= id_lo >= 0, so a padding slot
// matches no pixel), boxes [planes][max_nodes][4] = (x_min, y_min, x_max + 1, y_max + 1), areas [planes][max_nodes] (both zero
// past count), count [planes], overflow [planes].
C2M_API int c2m_instance_slots(const int32_t* table, int32_t* slot_ids, int32_t* boxes, int32_t* areas, int32_t* count,
                               int32_t* overflow, int planes, int nid, int id_lo, int min_pixels, int max_nodes,
                               void* stream) {
    C2M_ENTER();
    if (planes < 0 || nid < 1 || id_lo < 0 || min_pixels < 1 || max_nodes < 1 || max_nodes > C2M_LINK_MAX_NODES)
        return (int)hipErrorInvalidValue;
    if (planes == 0) return 0;
    if (!table || !slot_ids || !boxes || !areas || !count || !overflow) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(instance_compact_kernel<true>, dim3(planes), dim3(256), 0, (hipStream_t)stream, table, slot_ids, boxes,
                       areas, count, overflow, 1, nid, id_lo, min_pixels, max_nodes, -1);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ overlap
// Position of v in the ascending list a[0..63] (entries past n hold INT_MAX), or `none`.  Six dependent LDS reads, no branch.
__device__ __forceinline__ int slot_of(const int* a, int n, int v, int none) {
    int pos = 0;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) pos += a[pos + s - 1] < v ? s : 0;
    return (pos < n && a[pos] == v) ? pos : none;
}

struct OverlapP {
    const int* ref; const int* frm; const float* flow;       // [P][H][W], [P][H][W], [P][2][H][W] or null
    const int* ref_slots; const int* frm_slots;             // [P][max_nodes], ascending, -1 past the count
    const int* ref_count; const int* frm_count;             // [P]
    int* pairs;                                             // [P][max_nodes + 1][max_nodes + 1], zeroed before this kernel
    int P, H, W, max_nodes, rows, strips;
};

// One workgroup per strip of `rows` rows of one plane.  The slot lists of both planes and a (nr + 1) x (nf + 1) histogram live in
// LDS (nr, nf: the plane's slot counts; the last row / column is "no slot"); at the end every non-zero cell costs one int32
// global atomic.  The frame and the flow are read coalesced (16 bytes per lane when VEC = 4), the reference map is the gather.
template <int VEC>
__global__ __launch_bounds__(256) void instance_overlap_kernel(const OverlapP p) {
    __shared__ int s_ref[C2M_LINK_MAX_NODES], s_frm[C2M_LINK_MAX_NODES];
    __shared__ int hist[C2M_LINK_CELLS];
    const int tid = threadIdx.x;
    const int plane = blockIdx.x / p.strips, strip = blockIdx.x - plane * p.strips;
    const int M = p.max_nodes;
    const int nr = min(max(p.ref_count[plane], 0), M), nf = min(max(p.frm_count[plane], 0), M);
    if (tid < C2M_LINK_MAX_NODES) {
        s_ref[tid] = tid < nr ? p.ref_slots[(long)plane * M + tid] : 0x7fffffff;
        s_frm[tid] = tid < nf ? p.frm_slots[(long)plane * M + tid] : 0x7fffffff;
    }
    const int cols = nf + 1, cells = (nr + 1) * cols;
    for (int c = tid; c < cells; c += 256) hist[c] = 0;
    __syncthreads();

    const long HW = (long)p.H * p.W;
    const int* __restrict__ ref = p.ref + plane * HW;
    const int* __restrict__ frm = p.frm + plane * HW;
    const float* __restrict__ flow = p.flow ? p.flow + plane * 2 * HW : nullptr;
    const int y0 = strip * p.rows, y1 = min(y0 + p.rows, p.H);
    const int Wv = (p.W + VEC - 1) / VEC;                                // VEC = 4 only when W % 4 == 0
    const int items = (y1 - y0) * Wv;
    const int rounds = (items + 255) / 256;                              // whole waves stay in the loop (wave_merge_add)
    for (int r = 0; r < rounds; ++r) {
        const int i = r * 256 + tid;
        const bool live = i < items;
        int key[VEC];
        if (live) {
            const int y = y0 + i / Wv, x0 = (i % Wv) * VEC;
            const long sp = (long)y * p.W + x0;
            int fv[VEC];
            float fx[VEC], fy[VEC];
            if constexpr (VEC == 4) {
                const int4 a = *reinterpret_cast<const int4*>(frm + sp);
                fv[0] = a.x; fv[1] = a.y; fv[2] = a.z; fv[3] = a.w;
                if (flow) {
                    const float4 u = *reinterpret_cast<const float4*>(flow + sp);
                    const float4 v = *reinterpret_cast<const float4*>(flow + HW + sp);
                    fx[0] = u.x; fx[1] = u.y; fx[2] = u.z; fx[3] = u.w;
                    fy[0] = v.x; fy[1] = v.y; fy[2] = v.z; fy[3] = v.w;
                }
            } else {
                fv[0] = frm[sp];
                if (flow) { fx[0] = flow[sp]; fy[0] = flow[HW + sp]; }
            }
            int rv[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                long src = sp + e;
                if (flow) {
                    float ix, iy;
                    warp_source(fx[e], fy[e], x0 + e, y, p.H, p.W, ix, iy);
                    // clamped to [0, n - 1] first (NaN -> 0), so the rounded index is in bounds for any flow
                    const int sx = (int)rintf(warp_border(ix, p.W)), sy = (int)rintf(warp_border(iy, p.H));
                    src = (long)sy * p.W + sx;
                }
                rv[e] = ref[src];
            }
            int last_f = fv[0], last_fs = slot_of(s_frm, nf, fv[0], nf);
            int last_r = rv[0], last_rs = slot_of(s_ref, nr, rv[0], nr);
            key[0] = last_rs * cols + last_fs;
#pragma unroll
            for (int e = 1; e < VEC; ++e) {                               // a thread's pixels mostly repeat the id before them
                if (fv[e] != last_f) { last_f = fv[e]; last_fs = slot_of(s_frm, nf, last_f, nf); }
                if (rv[e] != last_r) { last_r = rv[e]; last_rs = slot_of(s_ref, nr, last_r, nr); }
                key[e] = last_rs * cols + last_fs;
            }
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) key[e] = 0;
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) wave_merge_add(hist, key[e], live);
    }
    __syncthreads();
    int* __restrict__ out = p.pairs + (long)plane * (M + 1) * (M + 1);
    for (int c = tid; c < cells; c += 256) {
        const int n = hist[c];
        if (n) {
            const int i = c / cols, j = c - i * cols;
            atomicAdd(out + (i == nr ? M : i) * (M + 1) + (j == nf ? M : j), n);
        }
    }
}

C2M_API int c2m_instance_overlap(const int32_t* ref, const int32_t* frame, const float* flow, const int32_t* ref_slots,
                                 const int32_t* ref_count, const int32_t* frame_slots, const int32_t* frame_count,
                                 int32_t* pairs, int P, int H, int W, int max_nodes, void* stream) {
    C2M_ENTER();
    if (P < 0 || H < 0 || W < 0 || max_nodes < 1 || max_nodes > C2M_LINK_MAX_NODES) return (int)hipErrorInvalidValue;
    const long HW = (long)H * W;
    if (HW >= (1L << 31)) return (int)hipErrorInvalidValue;
    if (P == 0) return 0;
    if (!pairs || !ref_slots || !ref_count || !frame_slots || !frame_count) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = c2m_zero_async(pairs, (long)P * (max_nodes + 1) * (max_nodes + 1) * 4, s);
    if (e != hipSuccess) return (int)e;
    if (HW == 0) return 0;
    if (!ref || !frame) return (int)hipErrorInvalidValue;
    int rows = c2m_cdiv(C2M_LINK_WG_PIXELS, W);
    if (rows > H) rows = H;
    const int strips = c2m_cdiv(H, rows);
    if ((long)P * strips >= (1L << 31)) return (int)hipErrorInvalidValue;
    const OverlapP p{ref, frame, flow, ref_slots, frame_slots, ref_count, frame_count, pairs, P, H, W, max_nodes, rows, strips};
    // plane bases are multiples of H * W words: 16-byte aligned for every plane when W % 4 == 0
    const bool vec = W % 4 == 0 && c2m_aligned(16, frame, flow);
    const dim3 grid((unsigned)(P * strips));
    if (vec) hipLaunchKernelGGL(instance_overlap_kernel<4>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(instance_overlap_kernel<1>, grid, dim3(256), 0, s, p);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ match
// IoU(i, j) = n / (r_i + a_j - n) with r_i the row sum (the warped reference area of slot i) and a_j the column sum (the frame
// area of slot j), both including the "no slot" cell.  Fractions are compared by cross-multiplication in 64 bits: n < 2^31 and
// the union < 2^32, so no product overflows.  A cell with n = 0 is never a candidate; ties go to the lower slot = the lower id.
__device__ __forceinline__ bool iou_gt(unsigned long long n1, unsigned long long u1, unsigned long long n2,
                                       unsigned long long u2) {
    return n1 * u2 > n2 * u1;
}

// One wave per plane; lane = slot.  link[p][i] = the frame slot of reference slot i, or -1.
__global__ __launch_bounds__(64) void instance_match_kernel(const int* __restrict__ pairs, const int* __restrict__ ref_slots,
                                                            const int* __restrict__ ref_count,
                                                            const int* __restrict__ frm_slots,
                                                            const int* __restrict__ frm_count, int* __restrict__ link, int M,
                                                            int iou_num, int iou_den, int same_class) {
    __shared__ unsigned r_s[C2M_LINK_MAX_NODES], a_s[C2M_LINK_MAX_NODES];
    __shared__ int best_ref[C2M_LINK_MAX_NODES];
    const int p = blockIdx.x, lane = threadIdx.x, S = M + 1;
    const int* __restrict__ tab = pairs + (long)p * S * S;
    const int nr = min(max(ref_count[p], 0), M), nf = min(max(frm_count[p], 0), M);
    unsigned r = 0, a = 0;
    if (lane < nr) for (int j = 0; j < S; ++j) r += (unsigned)tab[lane * S + j];
    if (lane < nf) for (int i = 0; i < S; ++i) a += (unsigned)tab[i * S + lane];
    r_s[lane] = r;
    a_s[lane] = a;
    __syncthreads();
    int bi = -1;
    if (lane < nf) {                                                      // the best reference slot of frame slot `lane`
        unsigned long long bn = 0, bu = 1;
        for (int i = 0; i < nr; ++i) {
            const unsigned long long n = (unsigned)tab[i * S + lane];
            const unsigned long long u = (unsigned long long)r_s[i] + a - n;
            if (n > 0 && iou_gt(n, u, bn, bu)) { bn = n; bu = u; bi = i; }
        }
    }
    best_ref[lane] = bi;
    __syncthreads();
    int out = -1;
    if (lane < nr) {                                                      // the best frame slot of reference slot `lane`
        unsigned long long bn = 0, bu = 1;
        int bj = -1;
        for (int j = 0; j < nf; ++j) {
            const unsigned long long n = (unsigned)tab[lane * S + j];
            const unsigned long long u = (unsigned long long)r + a_s[j] - n;
            if (n > 0 && iou_gt(n, u, bn, bu)) { bn = n; bu = u; bj = j; }
        }
        if (bj >= 0 && best_ref[bj] == lane && bn * (unsigned long long)iou_den >= (unsigned long long)iou_num * bu) {
            const int rid = ref_slots[(long)p * M + lane], fid = frm_slots[(long)p * M + bj];
            if (!same_class || rid / 1000 == fid / 1000) out = bj;
        }
    }
    if (lane < M) link[(long)p * M + lane] = out;
}

C2M_API int c2m_instance_match(const int32_t* pairs, const int32_t* ref_slots, const int32_t* ref_count,
                               const int32_t* frame_slots, const int32_t* frame_count, int32_t* link, int P, int max_nodes,
                               int iou_num, int iou_den, int same_class, void* stream) {
    C2M_ENTER();
    if (P < 0 || max_nodes < 1 || max_nodes > C2M_LINK_MAX_NODES || iou_num < 0 || iou_den < 1)
        return (int)hipErrorInvalidValue;
    if (P == 0) return 0;
    if (!pairs || !ref_slots || !ref_count || !frame_slots || !frame_count || !link) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(instance_match_kernel, dim3(P), dim3(64), 0, (hipStream_t)stream, pairs, ref_slots, ref_count,
                       frame_slots, frame_count, link, max_nodes, iou_num, iou_den, same_class);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ relabel
// A plane's ids rewritten through its (from, to) list: c2m_amd.tracking.anchor_maps puts the maps of the real frames into the
// id space of the anchor with it.  The list (at most 64 pairs, from ascending) sits in LDS and a pixel's pair is found by the
// binary search of slot_of, so the mapping is simultaneous -- a pixel is looked up by its OLD value only, and two ids may swap.
// A thread reuses the result of the pixel before it when the value repeats.  Integer code only.
#define C2M_RELABEL_VEC 4
#define C2M_RELABEL_ROUNDS 8
#define C2M_RELABEL_STRIP (256 * C2M_RELABEL_VEC * C2M_RELABEL_ROUNDS)    // pixels per workgroup

struct RelabelP {
    const int* maps; int* out;                              // [P][HW]
    const int* from; const int* to; const int* count;       // [P][64], [P][64], [P]
    const uint8_t* thing;                                   // [256]
    long HW; int strips, divisor;
};

__device__ __forceinline__ int relabel_value(const int* s_from, const int* s_to, int n, int v, int divisor, const uint8_t* thing) {
    const int pos = slot_of(s_from, n, v, -1);
    if (pos >= 0) return s_to[pos];
    if (v >= divisor) {
        const int cat = v / divisor;
        if (cat < 256 && thing[cat]) return cat * divisor;                // an unlinked object: its class's crowd id
    }
    return v;
}

template <int VEC>
__global__ __launch_bounds__(256) void instance_relabel_kernel(const RelabelP p) {
    __shared__ int s_from[C2M_LINK_MAX_NODES], s_to[C2M_LINK_MAX_NODES];
    __shared__ uint8_t s_thing[256];
    const int tid = threadIdx.x;
    const int plane = blockIdx.x / p.strips, strip = blockIdx.x - plane * p.strips;
    const int n = min(max(p.count[plane], 0), C2M_LINK_MAX_NODES);
    if (tid < C2M_LINK_MAX_NODES) {
        s_from[tid] = tid < n ? p.from[(long)plane * C2M_LINK_MAX_NODES + tid] : 0x7fffffff;
        s_to[tid] = tid < n ? p.to[(long)plane * C2M_LINK_MAX_NODES + tid] : 0;
    }
    s_thing[tid] = p.thing[tid];
    __syncthreads();
    const int* __restrict__ in = p.maps + plane * p.HW;
    int* __restrict__ out = p.out + plane * p.HW;
    const long q0 = (long)strip * (256 * VEC * C2M_RELABEL_ROUNDS);
#pragma unroll 2
    for (int r = 0; r < C2M_RELABEL_ROUNDS; ++r) {
        const long q = q0 + ((long)r * 256 + tid) * VEC;
        if (q >= p.HW) break;                                             // VEC = 4 only when HW % 4 == 0: q + 3 < HW as well
        if constexpr (VEC == 4) {
            const int4 a = *reinterpret_cast<const int4*>(in + q);
            int4 o;
            o.x = relabel_value(s_from, s_to, n, a.x, p.divisor, s_thing);
            o.y = a.y == a.x ? o.x : relabel_value(s_from, s_to, n, a.y, p.divisor, s_thing);
            o.z = a.z == a.y ? o.y : relabel_value(s_from, s_to, n, a.z, p.divisor, s_thing);
            o.w = a.w == a.z ? o.z : relabel_value(s_from, s_to, n, a.w, p.divisor, s_thing);
            *reinterpret_cast<int4*>(out + q) = o;
        } else {
            out[q] = relabel_value(s_from, s_to, n, in[q], p.divisor, s_thing);
        }
    }
}

C2M_API int c2m_instance_relabel(const int32_t* maps, int32_t* out, const int32_t* from, const int32_t* to, const int32_t* count,
                                 const uint8_t* thing_table, int P, long HW, int label_divisor, void* stream) {
    C2M_ENTER();
    if (P < 0 || HW < 0 || HW >= (1L << 31) || label_divisor < 1) return (int)hipErrorInvalidValue;
    if (P == 0 || HW == 0) return 0;
    if (!maps || !out || !from || !to || !count || !thing_table || maps == out) return (int)hipErrorInvalidValue;
    const bool vec = HW % 4 == 0 && c2m_aligned(16, maps, out);           // plane bases are multiples of HW words
    const long per = vec ? C2M_RELABEL_STRIP : C2M_RELABEL_STRIP / C2M_RELABEL_VEC;
    const long strips = (HW + per - 1) / per;
    if (strips * P >= (1L << 31)) return (int)hipErrorInvalidValue;
    const RelabelP p{maps, out, from, to, count, thing_table, HW, (int)strips, label_divisor};
    const dim3 grid((unsigned)(strips * P));
    if (vec) hipLaunchKernelGGL(instance_relabel_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(instance_relabel_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}
