// Wave64 primitives shared by the c2m_amd kernels (gfx950): sums, ordered ranks, the smallest key and the merge of equal keys
// before an atomic.
// Every function here is WAVE-WIDE (ballots and shuffles read all 64 lanes) or, where its name says 256, workgroup-wide: whole
// waves (whole workgroups) must reach the call.  A lane that has nothing to contribute passes pred / valid = false; it never
// leaves a loop or returns before the call.  Thread ids are 1-D (threadIdx.x).  Included by common.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ------------------------------------------------------------------------------------------------ sums (float, double, int)
// Result in lane 0.
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// The same sum, in the same shuffle order and so with the same bits, broadcast to every lane.
template <class T>
__device__ __forceinline__ T wave_sum_all(T v) { return __shfl(wave_sum(v), 0, 64); }

// Block-wide sum for blockDim.x == 256 (4 waves), smem >= 4 values.  Result valid in every thread.
template <class T>
__device__ __forceinline__ T block_sum_256(T v, T* smem) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) smem[wave] = v;
    __syncthreads();
    return smem[0] + smem[1] + smem[2] + smem[3];
}

// ------------------------------------------------------------------------------------------------ ordered ranks
// Number of lanes of the wave with pred set.
__device__ __forceinline__ int wave_count(bool pred) { return __popcll(__ballot(pred)); }

// Number of lanes BELOW this one with pred set (the lane's position in an ordered compaction); total = wave_count(pred).
__device__ __forceinline__ int wave_rank(bool pred, int& total) {
    const unsigned long long m = __ballot(pred);
    total = __popcll(m);
    return __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// The same over a 256-thread workgroup, in thread order: wave totals go through the four words of smem4.  Barrier contract: the
// barrier that publishes the totals is INSIDE (so it also publishes whatever the caller wrote to LDS before the call); the
// caller owns the barrier between its last use of the result of one call and the next call that reuses smem4.
__device__ __forceinline__ int block_rank_256(bool pred, int* smem4, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int wave_total;
    int rank = wave_rank(pred, wave_total);
    if (lane == 0) smem4[wave] = wave_total;
    __syncthreads();
    for (int w = 0; w < wave; ++w) rank += smem4[w];
    total = smem4[0] + smem4[1] + smem4[2] + smem4[3];
    return rank;
}

// ------------------------------------------------------------------------------------------------ the smallest key of a wave
// The lexicographically smallest (k, tie) over the 64 lanes and the value v of the lane that holds it, in every lane.  k must not
// be NaN.  (k, tie) is a total order: lanes with one (k, tie) must hold one v, and then the result does not depend on the order
// of the exchange.
__device__ __forceinline__ void wave_min_key_all(float& k, int& tie, float& v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float k2 = __shfl_xor(k, o, 64), v2 = __shfl_xor(v, o, 64);
        const int t2 = __shfl_xor(tie, o, 64);
        if (k2 < k || (k2 == k && t2 < tie)) { k = k2; tie = t2; v = v2; }
    }
}

// ------------------------------------------------------------------------------------------------ distinct keys of a wave
// One step of the walk over the DISTINCT keys held by the valid lanes of a wave: start with todo = __ballot(valid) and call while
// todo != 0 (wave-uniform).  Returns the leader (the lowest lane still to do), broadcasts its key to every lane in k0
// and gives the lanes of todo that hold the same key in `same`, the leader among them.  What the leader does with
// __popcll(same) stays at the call site, which ends the round with todo &= ~same: at most 64 rounds.
__device__ __forceinline__ int wave_key_step(unsigned long long todo, bool valid, int key, int& k0, unsigned long long& same) {
    const int leader = __ffsll((long long)todo) - 1;
    k0 = __shfl(key, leader, 64);
    same = __ballot(valid && key == k0) & todo;
    return leader;
}

// hist[key] += 1 for every valid lane, merged per wave: neighbouring pixels mostly share a cell, so one lane adds the number of
// lanes that hold each distinct key (a same-address atomic from 64 lanes would serialise instead).  hist: LDS or global.
__device__ __forceinline__ void wave_merge_add(int* hist, int key, bool valid) {
    unsigned long long todo = __ballot(valid);
    while (todo) {
        unsigned long long same;
        int k0;
        const int leader = wave_key_step(todo, valid, key, k0, same);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(hist + k0, __popcll(same));
        todo &= ~same;
    }
}

// ------------------------------------------------------------------------------------------------ alignment of pointers
// Are all of the pointers multiples of `bytes` (a power of two)?  A null pointer counts as aligned: an absent optional tensor
// never refuses a vector path.  For the launchers, and for the three kernels that choose their vector path themselves.
template <class... P>
__host__ __device__ static inline bool c2m_aligned(uintptr_t bytes, const P*... p) {   // at least one pointer
    return ((... | (uintptr_t)p) & (bytes - 1)) == 0;
}
