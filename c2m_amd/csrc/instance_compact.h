// Ordered compaction of the c2m_instance_stats table, shared by c2m_instance_compact (data_prep.hip: the objects of a sample,
// over its t_in input frames) and c2m_instance_slots (instance_link.hip: the objects of one plane, t_in = 1, with areas).
#pragma once
#include "common.h"

// One workgroup (256 threads) per group of t_in consecutive planes of the table: the ids with count >= min_pixels in EVERY one of
// the group's planes, in ascending id order.  Slots come from an ordered block-wide rank (block_rank_256), so the output does
// not depend on scheduling.  table [groups * t_in][nid][5] (count, x_min, x_max, y_min, y_max); ids [groups][max_nodes];
// boxes [groups][max_nodes][t_in][4] = (x_min, y_min, x_max + 1, y_max + 1); count [groups] (kept ids, <= max_nodes); overflow
// [groups] (1: more than max_nodes ids qualify; the rest is dropped).  Past count, ids hold pad_id and boxes are zero.
// PLANES: every group is ONE plane -- t_in is 1 at compile time (the kernel is latency-bound: one workgroup walks all ids, and
// the frame loop with a run-time bound cost the one-plane form 14 %) -- and areas [groups][max_nodes], the kept ids' counts, are
// written as well (zero past count); otherwise areas is not touched.
template <bool PLANES>
__global__ __launch_bounds__(256) void instance_compact_kernel(const int* __restrict__ table, int* __restrict__ ids,
                                                               int* __restrict__ boxes, int* __restrict__ areas,
                                                               int* __restrict__ count, int* __restrict__ overflow, int t_in,
                                                               int nid, int id_lo, int min_pixels, int max_nodes, int pad_id) {
    __shared__ int wave_tot[4];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int frames = PLANES ? 1 : t_in;
    const int* __restrict__ tab = table + (long)g * frames * nid * 5;
    int* __restrict__ my_ids = ids + (long)g * max_nodes;
    int* __restrict__ my_boxes = boxes + (long)g * max_nodes * frames * 4;
    int found = 0;
    for (int j0 = 0; j0 < nid; j0 += 256) {                                   // block-uniform: every thread ranks every chunk
        const int j = j0 + tid;
        bool keep = j < nid;
        int area = 0;                                                         // the count in the group's first plane
        for (int t = 0; t < frames && keep; ++t) {
            const int c = tab[((long)t * nid + j) * 5];
            if (t == 0) area = c;
            keep = c >= min_pixels;
        }
        int total;
        const int slot = found + block_rank_256(keep, wave_tot, total);
        if (keep && slot < max_nodes) {
            my_ids[slot] = id_lo + j;
            if constexpr (PLANES) areas[(long)g * max_nodes + slot] = area;
            for (int t = 0; t < frames; ++t) {
                const int* __restrict__ e = tab + ((long)t * nid + j) * 5;
                int* __restrict__ o = my_boxes + ((long)slot * frames + t) * 4;
                o[0] = e[1];
                o[1] = e[3];
                o[2] = e[2] + 1;
                o[3] = e[4] + 1;
            }
        }
        found += total;
        __syncthreads();                                                  // wave_tot is rewritten by the next chunk
    }
    const int kept = min(found, max_nodes);
    for (int s = kept + tid; s < max_nodes; s += 256) {
        my_ids[s] = pad_id;
        if constexpr (PLANES) areas[(long)g * max_nodes + s] = 0;
        for (int k = 0; k < frames * 4; ++k) my_boxes[(long)s * frames * 4 + k] = 0;
    }
    if (tid == 0) {
        count[g] = kept;
        overflow[g] = found > max_nodes ? 1 : 0;
    }
}
