// Toeplitz normal operator of the non-Cartesian CG stages (include/pnpadmm_toeplitz.h): the spectrum build and the pointwise kernels of
// the application around the engine's centred transform (launch_fft_rows / launch_fft_cols on the 2H x 2W grid, with its own twiddles).
//
//   setup   toeplitz_spectrum_kernel   K[j, l] = (1 / (H W)) sum_m w_m D_H(ky_m - (j - H) / 2H) D_W(kx_m - (l - W) / 2W), float64, rounded once
//   apply   toeplitz_pad_kernel        grid = p in the centred H x W window of the 2H x 2W grid, zeros elsewhere
//           | rows forward | cols forward (centred) |
//           toeplitz_mul_kernel        grid *= K
//           | rows inverse | cols inverse (centred) |
//           toeplitz_crop_kernel       q = crop(grid)  (+ mu p by one fma and the partial sums of Re<p, q>: the normal operator's last launch)
//
// The spectrum has no atomics and no partial sums.  One workgroup owns one kToeplitzTile^2 tile of K and walks ALL samples in ascending
// order, kTzChunk at a time: a chunk is staged in LDS as, per sample, the row vector a[r] = w_m D_H at the tile's rows and the column vector
// b[c] = D_W at its columns (2 x 32 Dirichlet quotients per sample for 1024 outputs), and every thread then runs acc = fma(a, b, acc) on
// its 4 x 4 register block: 16 fmas per 8 LDS reads, the sine evaluations a 16th of the fmas.  An output's value is the fma chain from 0
// over ascending m whatever the tile: the bits depend on (trajectory, weights, H, W) only.
// Every expression is written in the header's order and this unit is compiled without contraction.
#include "pnp_internal.h"
#include "block_reduce.h"

#pragma clang fp contract(off)

#include "toeplitz_dirichlet.h"

namespace pnp {

namespace {

constexpr int kTzThreads = 256;
constexpr int kTzPer = kPixelChunk / kTzThreads;          // pixels per thread of the chunked crop kernel
static_assert(kPixelChunk % kTzThreads == 0, "whole pixels per thread");
constexpr int kTzSpecThreads = 64;                         // an 8 x 8 grid of threads, a 4 x 4 register block each
constexpr int kTzReg = 4, kTzSide = 8;
static_assert(kTzReg * kTzSide == kToeplitzTile && kTzSide * kTzSide == kTzSpecThreads, "the register blocks tile the workgroup's tile");
constexpr int kTzChunk = 32;                               // samples staged per pass: 2 x 32 x 32 x 8 B = 16 KiB of LDS

__device__ __forceinline__ bool stopped(const float* tact, int n) { return tact != nullptr && tact[n] > 0.5f; }

// (dirichlet(): toeplitz_dirichlet.h)

__global__ __launch_bounds__(kTzSpecThreads) void toeplitz_spectrum_kernel(const double2* __restrict__ traj, const float* __restrict__ w, int M, int H,
                                                                           int W, float* __restrict__ K) {
    __shared__ double a_s[kTzChunk][kToeplitzTile];
    __shared__ double b_s[kTzChunk][kToeplitzTile];
    const int j0 = blockIdx.y * kToeplitzTile, l0 = blockIdx.x * kToeplitzTile;
    const int tx = threadIdx.x % kTzSide, ty = threadIdx.x / kTzSide;
    double acc[kTzReg][kTzReg];
#pragma unroll
    for (int i = 0; i < kTzReg; ++i)
#pragma unroll
        for (int k = 0; k < kTzReg; ++k) acc[i][k] = 0.0;
    for (int m0 = 0; m0 < M; m0 += kTzChunk) {
        const int cnt = min(kTzChunk, M - m0);
        for (int idx = threadIdx.x; idx < cnt * kToeplitzTile; idx += kTzSpecThreads) {
            const int sl = idx / kToeplitzTile, r = idx % kToeplitzTile;
            const double2 k = traj[m0 + sl];               // (ky, kx)
            const double ww = w != nullptr ? (double)w[m0 + sl] : 1.0;
            a_s[sl][r] = ww * dirichlet(k.x - (double)(j0 + r - H) / (double)(2 * H), H);
            b_s[sl][r] = dirichlet(k.y - (double)(l0 + r - W) / (double)(2 * W), W);
        }
        __syncthreads();
        for (int s = 0; s < cnt; ++s) {
            double a[kTzReg], b[kTzReg];
#pragma unroll
            for (int i = 0; i < kTzReg; ++i) { a[i] = a_s[s][ty + kTzSide * i]; b[i] = b_s[s][tx + kTzSide * i]; }
#pragma unroll
            for (int i = 0; i < kTzReg; ++i)
#pragma unroll
                for (int k = 0; k < kTzReg; ++k) acc[i][k] = fma(a[i], b[k], acc[i][k]);
        }
        __syncthreads();
    }
    const double hw = (double)H * (double)W;
#pragma unroll
    for (int i = 0; i < kTzReg; ++i)
#pragma unroll
        for (int k = 0; k < kTzReg; ++k)
            K[(size_t)(j0 + ty + kTzSide * i) * (2 * W) + (l0 + tx + kTzSide * k)] = (float)(acc[i][k] / hw);
}

// grid[n][gy][gx] = inside the centred H x W window ? src[n][gy - H/2][gx - W/2] : 0
__global__ __launch_bounds__(kTzThreads) void toeplitz_pad_kernel(const float2* __restrict__ src, float2* __restrict__ grid, int H, int W) {
    const int n = blockIdx.y, gw = 2 * W, G = 4 * H * W;
    const int g = blockIdx.x * kTzThreads + threadIdx.x;
    if (g >= G) return;
    const int gy = g / gw, gx = g - gy * gw;
    const int iy = gy - H / 2, ix = gx - W / 2;
    float2 v = make_float2(0.f, 0.f);
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = src[((size_t)n * H + iy) * W + ix];
    grid[(size_t)n * G + g] = v;
}

__global__ __launch_bounds__(kTzThreads) void toeplitz_mul_kernel(float2* __restrict__ grid, const float* __restrict__ K, int G) {
    const int n = blockIdx.y;
    const int g = blockIdx.x * kTzThreads + threadIdx.x;
    if (g >= G) return;
    const float k = K[g];
    float2 v = grid[(size_t)n * G + g];
    v.x *= k; v.y *= k;
    grid[(size_t)n * G + g] = v;
}

// q[n][p] = grid[n][window] (+ mu[n] pv[n][p], one fma, when pv != nullptr); partial[n, chunk, 0] = sum over the chunk of Re(conj(pv) q):
// nufft_crop_kernel's pixel ranges and fixed tree
__global__ __launch_bounds__(kTzThreads) void toeplitz_crop_kernel(const float2* __restrict__ grid, const float2* __restrict__ pv,
                                                                   const float* __restrict__ mu, const float* __restrict__ tact,
                                                                   float2* __restrict__ q, double* __restrict__ partial, int H, int W) {
    __shared__ double red[kTzThreads / 64];
    const int n = blockIdx.y, HW = H * W, gw = 2 * W;
    if (stopped(tact, n)) return;
    const int p0 = blockIdx.x * kPixelChunk + threadIdx.x;
    const size_t base = (size_t)n * HW, gbase = (size_t)n * 4 * HW;
    const int oy = H / 2, ox = W / 2;
    const float m = (pv != nullptr && mu != nullptr) ? mu[n] : 0.f;
    double dot[1] = {0.0};
#pragma unroll
    for (int j = 0; j < kTzPer; ++j) {
        const int p = p0 + j * kTzThreads;
        if (p < HW) {
            const int iy = p / W, ix = p - iy * W;
            float2 o = grid[gbase + (size_t)(iy + oy) * gw + (ix + ox)];
            if (pv != nullptr) {
                const float2 pp = pv[base + p];
                o.x = fmaf(m, pp.x, o.x); o.y = fmaf(m, pp.y, o.y);
                dot[0] += (double)pp.x * (double)o.x + (double)pp.y * (double)o.y;
            }
            q[base + p] = o;
        }
    }
    if (partial == nullptr) return;                        // (uniform)
    block_sums_fixed<kTzThreads, 1>(dot, red);
    if (threadIdx.x == 0) partial[((size_t)n * gridDim.x + blockIdx.x) * 2] = dot[0];
}

}  // namespace

hipError_t launch_toeplitz_spectrum(const double* traj, const float* w, int64_t m, int H, int W, float* K, hipStream_t s) {
    const dim3 g((unsigned)(2 * W / kToeplitzTile), (unsigned)(2 * H / kToeplitzTile));
    hipLaunchKernelGGL(toeplitz_spectrum_kernel, g, dim3(kTzSpecThreads), 0, s, reinterpret_cast<const double2*>(traj), w, (int)m, H, W, K);
    return hipGetLastError();
}

hipError_t launch_toeplitz_pad(const float2* src, float2* grid, int H, int W, int planes, hipStream_t s) {
    const dim3 g((unsigned)((4 * H * W + kTzThreads - 1) / kTzThreads), (unsigned)planes);
    hipLaunchKernelGGL(toeplitz_pad_kernel, g, dim3(kTzThreads), 0, s, src, grid, H, W);
    return hipGetLastError();
}

hipError_t launch_toeplitz_mul(float2* grid, const float* K, int H, int W, int planes, hipStream_t s) {
    const dim3 g((unsigned)((4 * H * W + kTzThreads - 1) / kTzThreads), (unsigned)planes);
    hipLaunchKernelGGL(toeplitz_mul_kernel, g, dim3(kTzThreads), 0, s, grid, K, 4 * H * W);
    return hipGetLastError();
}

hipError_t launch_toeplitz_crop(const float2* grid, const float2* pv, const float* mu, const float* tact, float2* q, double* partial, int H, int W,
                                int planes, hipStream_t s) {
    hipLaunchKernelGGL(toeplitz_crop_kernel, dim3((unsigned)pixel_chunks(H, W), (unsigned)planes), dim3(kTzThreads), 0, s, grid, pv, mu, tact, q,
                       partial, H, W);
    return hipGetLastError();
}

}  // namespace pnp
