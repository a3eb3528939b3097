// Microbenchmark: how accurate is an fp32 GEMM computed on the bf16 matrix pipe from three-piece split operands?
// C[M][N] = A[M][K] * B[K][N] (B stored transposed), one wave per 32x32 tile, against a float64 host result.
// Forms:
//   f32     v_mfma_f32_32x32x2_f32 (the exact-f32 pipe: a k-ordered fmaf chain)
//   s6      a = a0 + a1 + a2 (bf16 pieces, split by truncation); the six products a0b0 a0b1 a1b0 a0b2 a1b1 a2b0 on
//           v_mfma_f32_32x32x16_bf16 into ONE accumulator
//   s6/lo4  the same, the last four products into a second accumulator that is added at the end
//   s6/lo5  the same, every product but a0b0 into the second accumulator
//   s9      all nine products, one accumulator
// Data: standard-normal operands; and the same with column k of A scaled by 2^e_k and row k of B by 2^-e_k,
// e_k uniform in [-40, 40] (the products keep their size, the pieces of every operand move through 80 binades).
// Prints max|C - ref| / max|ref| per form and K.  Build: hipcc --offload-arch=gfx950 -O2 split_bf16_gemm.hip
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

// a == p0 + p1 + p2 bit for bit; every piece has at most 8 significant bits and the sign of a
__device__ __forceinline__ void split3(float a, __bf16& p0, __bf16& p1, __bf16& p2) {
    const unsigned u = __builtin_bit_cast(unsigned, a) & 0xFFFF0000u;
    const float r = a - __builtin_bit_cast(float, u);
    const unsigned v = __builtin_bit_cast(unsigned, r) & 0xFFFF0000u;
    const float q = r - __builtin_bit_cast(float, v);
    p0 = __builtin_bit_cast(__bf16, (unsigned short)(u >> 16));
    p1 = __builtin_bit_cast(__bf16, (unsigned short)(v >> 16));
    p2 = __builtin_bit_cast(__bf16, (unsigned short)(__builtin_bit_cast(unsigned, q) >> 16));
}

// NPROD = 6 or 9 products; the last NLOW of them (in the order above) go to the second accumulator
template <int NPROD, int NLOW>
__global__ __launch_bounds__(64) void gemm_split(const float* __restrict__ A, const float* __restrict__ Bt,
                                                 float* __restrict__ C, int K, int N) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const float* a = A + (long)(blockIdx.y * 32 + r) * K + 8 * h;
    const float* b = Bt + (long)(blockIdx.x * 32 + r) * K + 8 * h;
    f32x16 hi, lo;
    for (int i = 0; i < 16; ++i) { hi[i] = 0.f; lo[i] = 0.f; }
    // product order: descending weight
    constexpr int PA[9] = {0, 0, 1, 0, 1, 2, 1, 2, 2}, PB[9] = {0, 1, 0, 2, 1, 0, 2, 1, 2};
    for (int k = 0; k < K; k += 16) {
        bf16x8 fa[3], fb[3];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            __bf16 p0, p1, p2;
            split3(a[k + j], p0, p1, p2); fa[0][j] = p0; fa[1][j] = p1; fa[2][j] = p2;
            split3(b[k + j], p0, p1, p2); fb[0][j] = p0; fb[1][j] = p1; fb[2][j] = p2;
        }
#pragma unroll
        for (int q = 0; q < NPROD; ++q) {
            if (q >= NPROD - NLOW) lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[PA[q]], fb[PB[q]], lo, 0, 0, 0);
            else hi = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[PA[q]], fb[PB[q]], hi, 0, 0, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = blockIdx.y * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
        C[(long)row * N + blockIdx.x * 32 + r] = hi[i] + lo[i];
    }
}

__global__ __launch_bounds__(64) void gemm_f32(const float* __restrict__ A, const float* __restrict__ Bt,
                                               float* __restrict__ C, int K, int N) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const float* a = A + (long)(blockIdx.y * 32 + r) * K + h;
    const float* b = Bt + (long)(blockIdx.x * 32 + r) * K + h;
    f32x16 acc;
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int k = 0; k < K; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k], b[k], acc, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = blockIdx.y * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
        C[(long)row * N + blockIdx.x * 32 + r] = acc[i];
    }
}

int main() {
    constexpr int M = 128, N = 128, NF = 5;
    const int Ks[4] = {16, 256, 4096, 16384};
    const char* names[NF] = {"f32", "s6", "s6/lo4", "s6/lo5", "s9"};
    float *dA, *dB, *dC;
    CHECK(hipMalloc(&dA, (size_t)M * 16384 * 4));
    CHECK(hipMalloc(&dB, (size_t)N * 16384 * 4));
    CHECK(hipMalloc(&dC, (size_t)M * N * 4));
    printf("max|C - ref64| / max|ref64|, %d x %d outputs per cell\n", M, N);
    printf("%-8s %6s", "data", "K");
    for (int f = 0; f < NF; ++f) printf(" %10s", names[f]);
    printf("\n");
    for (int data = 0; data < 2; ++data) {
        for (int K : Ks) {
            std::mt19937_64 rng(1234 + K + data);
            std::normal_distribution<float> nd(0.f, 1.f);
            std::uniform_int_distribution<int> ed(-40, 40);
            std::vector<float> A((size_t)M * K), B((size_t)N * K), C((size_t)M * N);
            std::vector<int> e(K, 0);
            if (data) for (int k = 0; k < K; ++k) e[k] = ed(rng);
            for (int i = 0; i < M; ++i) for (int k = 0; k < K; ++k) A[(size_t)i * K + k] = std::ldexp(nd(rng), e[k]);
            for (int j = 0; j < N; ++j) for (int k = 0; k < K; ++k) B[(size_t)j * K + k] = std::ldexp(nd(rng), -e[k]);
            std::vector<double> ref((size_t)M * N);
            double refmax = 0;
            for (int i = 0; i < M; ++i)
                for (int j = 0; j < N; ++j) {
                    double s = 0;
                    for (int k = 0; k < K; ++k) s += (double)A[(size_t)i * K + k] * (double)B[(size_t)j * K + k];
                    ref[(size_t)i * N + j] = s;
                    refmax = std::fmax(refmax, std::fabs(s));
                }
            CHECK(hipMemcpy(dA, A.data(), A.size() * 4, hipMemcpyHostToDevice));
            CHECK(hipMemcpy(dB, B.data(), B.size() * 4, hipMemcpyHostToDevice));
            printf("%-8s %6d", data ? "spread" : "normal", K);
            for (int f = 0; f < NF; ++f) {
                CHECK(hipMemset(dC, 0xFF, C.size() * 4));
                const dim3 grid(N / 32, M / 32), block(64);
                switch (f) {
                    case 0: hipLaunchKernelGGL(gemm_f32, grid, block, 0, 0, dA, dB, dC, K, N); break;
                    case 1: hipLaunchKernelGGL((gemm_split<6, 0>), grid, block, 0, 0, dA, dB, dC, K, N); break;
                    case 2: hipLaunchKernelGGL((gemm_split<6, 4>), grid, block, 0, 0, dA, dB, dC, K, N); break;
                    case 3: hipLaunchKernelGGL((gemm_split<6, 5>), grid, block, 0, 0, dA, dB, dC, K, N); break;
                    case 4: hipLaunchKernelGGL((gemm_split<9, 0>), grid, block, 0, 0, dA, dB, dC, K, N); break;
                }
                CHECK(hipGetLastError());
                CHECK(hipMemcpy(C.data(), dC, C.size() * 4, hipMemcpyDeviceToHost));
                double err = 0;
                for (size_t i = 0; i < C.size(); ++i) {
                    const double d = std::fabs((double)C[i] - ref[i]);
                    err = std::isfinite(d) ? std::fmax(err, d) : INFINITY;
                }
                printf(" %10.3e", err / refmax);
            }
            printf("\n");
            fflush(stdout);
        }
    }
    return 0;
}
