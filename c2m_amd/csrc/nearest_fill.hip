// Nearest-seed fill of label planes (gfx950): every hole pixel of an image takes all its label words from the nearest seed pixel
// of the same image.  c2m_amd.interactive.propagate_maps(fill="nearest") uses it to give a disoccluded pixel the labels of the
// nearest visible background pixel (DESIGN.md 4.2k has the contract and the cost).
//
// The rule is exact (no approximation, no jump flooding).  For a hole pixel (y, x) the source is the seed pixel (y', x') of the
// same image with the smallest key ((y - y')^2 + (x - x')^2, y', x'), compared lexicographically as integers: ties in distance go
// to the smaller row, then to the smaller column.  The kernel keeps that key as ONE 64-bit number, d^2 << 32 | (y' * W + x')
// (H, W <= 32768, so d^2 < 2^31; H * W < 2^31), and takes its minimum over every candidate it visits, so an equal distance is
// resolved by the key and never by the order of the visit.
//
//   nf_pack_kernel   a wave holds 64 consecutive x of one row: one ballot of `seed && !hole` is that row's 64-bit word of the image's
//                    seed set (bit i of word w = pixel 64 * w + i; the padding bits of a last, partly filled word are zero), and
//                    its population count goes to the image's seed counter (summed per wave and image first: a wave packs a
//                    contiguous run of words).  A pixel set in both masks is a hole, never a seed.
//   nf_fill_kernel   the same wave shape with the hole lanes active.  A hole pixel walks dy = 0, 1, 2, ... over the rows y - dy and
//                    y + dy; in each row it finds the nearest set bit at or left of x and the nearest right of x with clz / ffs
//                    on the words, going outwards no further than dy^2 + dx^2 <= best d^2 allows.  It stops as soon as dy^2 > best
//                    d^2 -- not at equality: a seed straight above at distance dy ties and wins on y' -- or when both rows are
//                    outside the image, and at once when the image has no seed (its holes are then counted in `unfilled`).  Then
//                    it copies its Cf + Ci words from the source.
//
// Filling IN PLACE has no read-after-write hazard: only hole pixels are written, only seed pixels are read as sources, and the
// packed seed set leaves out every hole, so no word is both read and written by this call, in any order of the waves.
// Every loop is bounded by H or by ceil(W / 64) before it starts, no loop waits for another wave, and the only atomics are the
// integer adds of the two counters (seeds per image, unfilled holes per image): every output is bit-repeatable.
// Planes are moved as 32-bit words, so every bit pattern survives (NaN payloads, negative ids), as in label_warp.hip.
#include "common.h"

#define C2M_NF_MAX_SIDE 32768

typedef unsigned long long nf_u64;

struct NfP {
    const uint8_t* hole; const uint8_t* seed;               // [B*T][H][W], dense
    uint32_t* pf; long fsb, fsc, fst; int Cf;                // [B][Cf][T][H][W] words, element strides, dense rows
    uint32_t* pi; long isb, isc, ist; int Ci;
    nf_u64* bits; int* nseed; int* unfilled;                 // [B*T][H][Wq] | [B*T] | [B*T]
    int T, H, W, Wq; long items;                             // items = B * T * H * Wq: one wave each
};

static inline bool nf_sizes_ok(long B, long T, long H, long W) {
    return B >= 0 && T >= 0 && H >= 0 && W >= 0 && H <= C2M_NF_MAX_SIDE && W <= C2M_NF_MAX_SIDE && H * W < (1L << 31) &&
           B * T < (1L << 31);
}

static inline long nf_words(long B, long T, long H, long W) { return B * T * H * ((W + 63) / 64); }

C2M_API long c2m_nearest_fill_workspace_bytes(int B, int T, int H, int W) {
    if (!nf_sizes_ok(B, T, H, W)) return -1;
    return nf_words(B, T, H, W) * 8 + (((long)B * T + 1) / 2) * 8;          // bit rows, then the seed counters (int32, padded to 8)
}

// (image, row, word of the row) of item i
__device__ __forceinline__ void nf_item(const NfP& p, long i, long& img, int& y, int& w) {
    w = (int)(i % p.Wq);
    const long r = i / p.Wq;
    y = (int)(r % p.H);
    img = r / p.H;
}

// A wave packs a CONTIGUOUS run of items, so that it adds its seeds to an image's counter once per image it touches: one add per
// item would put H * ceil(W / 64) adds on one address per image, and same-address atomics are served one after the other.
__global__ __launch_bounds__(256) void nf_pack_kernel(const NfP p) {
    const int lane = threadIdx.x & 63;
    const long nwaves = (long)gridDim.x * 4, per = (p.items + nwaves - 1) / nwaves;
    const long first = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * per;
    const long end = first + per < p.items ? first + per : p.items;
    long cur = -1;
    int acc = 0;
    for (long i = first; i < end; ++i) {                                        // wave-uniform, at most `per` rounds
        long img; int y, w;
        nf_item(p, i, img, y, w);
        if (img != cur) {
            if (lane == 0 && acc) atomicAdd(p.nseed + cur, acc);
            cur = img;
            acc = 0;
        }
        const int x = w * 64 + lane;
        bool s = false;
        if (x < p.W) {
            const long q = (img * p.H + y) * (long)p.W + x;
            s = p.seed[q] != 0 && p.hole[q] == 0;
        }
        const nf_u64 m = __ballot(s);
        if (lane == 0) p.bits[i] = m;
        acc += __popcll(m);
    }
    if (lane == 0 && acc) atomicAdd(p.nseed + cur, acc);
}

// The candidates of row yy (dy2 = (y - yy)^2) for pixel x: the nearest seed at or left of x and the nearest right of it.
__device__ __forceinline__ void nf_row(const nf_u64* __restrict__ row, int Wq, int W, int x, int yy, unsigned dy2, nf_u64& best) {
    const int w0 = x >> 6, bit = x & 63;
    const nf_u64 own = row[w0];
    const unsigned base = (unsigned)yy * (unsigned)W;
    nf_u64 m = own & (~0ull >> (63 - bit));
    for (int w = w0; w >= 0; --w) {                                             // at most Wq rounds
        if (w != w0) {
            const unsigned dx = (unsigned)(x - (w * 64 + 63));                   // the nearest pixel of word w
            if ((nf_u64)(dy2 + dx * dx) > (best >> 32)) break;
            m = row[w];
        }
        if (m) {
            const int xs = w * 64 + 63 - __clzll((long long)m);
            const unsigned dx = (unsigned)(x - xs);
            const nf_u64 key = ((nf_u64)(dy2 + dx * dx) << 32) | (nf_u64)(base + (unsigned)xs);
            best = key < best ? key : best;
            break;
        }
    }
    m = bit == 63 ? 0ull : own & (~0ull << (bit + 1));
    for (int w = w0; w < Wq; ++w) {
        if (w != w0) {
            const unsigned dx = (unsigned)(w * 64 - x);
            if ((nf_u64)(dy2 + dx * dx) > (best >> 32)) break;
            m = row[w];
        }
        if (m) {
            const int xs = w * 64 + __ffsll((long long)m) - 1;
            const unsigned dx = (unsigned)(xs - x);
            const nf_u64 key = ((nf_u64)(dy2 + dx * dx) << 32) | (nf_u64)(base + (unsigned)xs);
            best = key < best ? key : best;
            break;
        }
    }
}

// pl[c * stride + dst] = pl[c * stride + src] for C planes, four loads in flight at a time (the compiler cannot know that a store
// to a hole is never the next plane's source, so the loads of a group are written before its stores).
__device__ __forceinline__ void nf_copy(uint32_t* pl, long stride, int C, long src, long dst) {
    int c = 0;
    for (; c + 4 <= C; c += 4, pl += 4 * stride) {
        const uint32_t v0 = pl[src], v1 = pl[stride + src], v2 = pl[2 * stride + src], v3 = pl[3 * stride + src];
        pl[dst] = v0; pl[stride + dst] = v1; pl[2 * stride + dst] = v2; pl[3 * stride + dst] = v3;
    }
    for (; c < C; ++c, pl += stride) pl[dst] = pl[src];
}

// The search and the copy of one hole pixel (y, x) of an image that has at least one seed.
__device__ __forceinline__ void nf_fill_pixel(const NfP& p, long img, int y, int x) {
    const int H = p.H, W = p.W, Wq = p.Wq;
    const nf_u64* __restrict__ rows = p.bits + img * H * (long)Wq;
    nf_u64 best = ~0ull;
    for (int dy = 0; dy < H; ++dy) {
        const unsigned dy2 = (unsigned)dy * (unsigned)dy;
        if ((nf_u64)dy2 > (best >> 32)) break;                                  // equality goes on: a tie in a smaller row wins
        const int ya = y - dy, yb = y + dy;
        if (ya < 0 && yb >= H) break;
        if (ya >= 0) nf_row(rows + (long)ya * Wq, Wq, W, x, ya, dy2, best);
        if (dy > 0 && yb < H) nf_row(rows + (long)yb * Wq, Wq, W, x, yb, dy2, best);
    }
    if (best == ~0ull) return;                                                  // not reached with a seed in the image; writes nothing
    const long src = (long)(unsigned)(best & 0xffffffffull), dst = (long)y * W + x;
    const int b = (int)(img / p.T), t = (int)(img % p.T);
    if (p.Cf > 0) nf_copy(p.pf + (long)b * p.fsb + (long)t * p.fst, p.fsc, p.Cf, src, dst);
    if (p.Ci > 0) nf_copy(p.pi + (long)b * p.isb + (long)t * p.ist, p.isc, p.Ci, src, dst);
}

__global__ __launch_bounds__(256) void nf_fill_kernel(const NfP p) {
    const int lane = threadIdx.x & 63;
    const long nwaves = (long)gridDim.x * 4;
    for (long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6); i < p.items; i += nwaves) {      // wave-uniform
        long img; int y, w;
        nf_item(p, i, img, y, w);
        const int x = w * 64 + lane;
        const bool hole = x < p.W && p.hole[(img * p.H + y) * (long)p.W + x] != 0;
        const nf_u64 holes = __ballot(hole);
        if (!holes) continue;
        if (p.nseed[img] == 0) {                                                // wave-uniform: nothing to fill from
            if (lane == 0) atomicAdd(p.unfilled + img, __popcll(holes));
            continue;
        }
        if (hole) nf_fill_pixel(p, img, y, x);                                  // no lane leaves the wave-uniform loop early
    }
}

C2M_API int c2m_nearest_fill(const uint8_t* hole, const uint8_t* seed, float* planes_f, long fsb, long fsc, long fst, int Cf,
                             int32_t* planes_i, long isb, long isc, long ist, int Ci, int B, int T, int H, int W,
                             int32_t* unfilled, void* workspace, long workspace_bytes, void* stream) {
    C2M_ENTER();
    if (Cf < 0 || Ci < 0 || !nf_sizes_ok(B, T, H, W)) return (int)hipErrorInvalidValue;
    const long BT = (long)B * T;
    if (BT == 0) return 0;
    if (!unfilled) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = c2m_zero_async(unfilled, BT * 4, s);
    if (e != hipSuccess) return (int)e;
    if ((long)H * W == 0) return 0;
    if (Cf + Ci == 0 || !hole || !seed || !workspace || (Cf > 0 && !planes_f) || (Ci > 0 && !planes_i))
        return (int)hipErrorInvalidValue;
    const long need = c2m_nearest_fill_workspace_bytes(B, T, H, W);
    if (workspace_bytes < need || !c2m_aligned(8, workspace) || !c2m_aligned(4, planes_f, planes_i, unfilled))
        return (int)hipErrorInvalidValue;
    const int Wq = (W + 63) / 64;
    const long items = nf_words(B, T, H, W);
    nf_u64* bits = (nf_u64*)workspace;
    const NfP p{hole, seed, (uint32_t*)planes_f, fsb, fsc, fst, Cf, (uint32_t*)planes_i, isb, isc, ist, Ci,
                bits, (int*)(bits + items), unfilled, T, H, W, Wq, items};
    e = c2m_zero_async(workspace, need, s);                                     // the counters need it; the bit rows are all written
    if (e != hipSuccess) return (int)e;
    const dim3 grid(c2m_grid(items * 64, 256));
    hipLaunchKernelGGL(nf_pack_kernel, grid, dim3(256), 0, s, p);
    C2M_LAUNCH_CHECK();
    hipLaunchKernelGGL(nf_fill_kernel, grid, dim3(256), 0, s, p);
    return (int)hipGetLastError();
}
