// ADMM residuals on the device (pnp_residuals): per slice, with (x_p, z_p, u_p) the iterate before the step,
//   primal = ||x - z||,  dx = ||x - x_p||,  dz = ||z - z_p||,  du = ||u - u_p||,  delta = (dx + dz + du) / sqrt(H W)
// (the fixed-point stopping quantity of Chan, Wang, Elgendy 2017), and the k-space data misfit  dc = ||where(mask, fft_c(x) - y0, 0)||.
//
// residual_tile_kernel<DELTA>: one workgroup (256 threads) per kPixelChunk contiguous pixels of ONE slice - the range a workgroup owns
// depends on the slice's size only, never on the batch, so a slice gives the same bits wherever it sits in a handle.  A thread reads
// four pixels at a time with 16-byte loads (x: one float4; z, u: two each; the same again from the previous planes when DELTA), forms every
// difference in float32 (one rounding), squares and accumulates it in float64, and the workgroup reduces by wave shuffles, then through
// LDS, to ONE float64 partial per quantity.
// misfit_tile_kernel: the same shape over k-space.  It reads the plain (unshifted) orthonormal transform of x, which the engine's own row
// and column passes left in its scratch plane, and the episode constants in the layout reset_kernel writes: y0s = sgn * S y0 and S mask
// (shared or one per slice).  |fft_c(x) - y0| at S k equals |FFT(x) - y0s| at k (the sign has modulus 1), so no index is shifted here.
// residual_reduce_kernel: one workgroup per slice sums the slice's partials in a fixed order, takes the square roots, forms delta and
// writes the six float32 columns; columns that were not asked for are written as 0.
// No atomics anywhere: the result is bitwise reproducible.  40 B per pixel for the delta pass (12 without `prev`), 17 for the misfit pass.
#include "pnp_internal.h"
#include "block_reduce.h"

namespace pnp {

namespace {

constexpr int kResThreads = 256;
constexpr int kResIters = kPixelChunk / (4 * kResThreads);   // four-pixel groups per thread
static_assert(kPixelChunk % (4 * kResThreads) == 0, "whole batches of four-pixel groups");

__device__ __forceinline__ double sq(float d) { return (double)d * (double)d; }
// |a - b|^2 of two complex pairs held in one float4 (re0, im0, re1, im1): four float32 differences, squared and summed in float64
__device__ __forceinline__ double diff2(const float4& a, const float4& b) {
    return sq(a.x - b.x) + sq(a.y - b.y) + sq(a.z - b.z) + sq(a.w - b.w);
}

template <bool DELTA>
__global__ __launch_bounds__(kResThreads) void residual_tile_kernel(const float* __restrict__ x, const float2* __restrict__ z,
                                                                    const float2* __restrict__ u, const float* __restrict__ xp,
                                                                    const float2* __restrict__ zp, const float2* __restrict__ up,
                                                                    double* __restrict__ partial, int HW) {
    __shared__ double red[4 * (kResThreads / 64)];
    const int n = blockIdx.y;
    const size_t base = (size_t)n * HW;
    const int p0 = blockIdx.x * kPixelChunk;
    float4 vx[kResIters], vz[kResIters][2], vu[kResIters][2], wx[kResIters], wz[kResIters][2], wu[kResIters][2];
    bool on[kResIters];
    // every load of the workgroup's range is issued before the first use (HW is a multiple of 4: a group of four pixels is in or out whole)
#pragma unroll
    for (int it = 0; it < kResIters; ++it) {
        const int p = p0 + (it * kResThreads + (int)threadIdx.x) * 4;
        on[it] = p < HW;
        if (on[it]) {
            const size_t g = base + p;
            vx[it] = *reinterpret_cast<const float4*>(x + g);
            vz[it][0] = *reinterpret_cast<const float4*>(z + g);
            vz[it][1] = *reinterpret_cast<const float4*>(z + g + 2);
            if (DELTA) {
                vu[it][0] = *reinterpret_cast<const float4*>(u + g);
                vu[it][1] = *reinterpret_cast<const float4*>(u + g + 2);
                wx[it] = *reinterpret_cast<const float4*>(xp + g);
                wz[it][0] = *reinterpret_cast<const float4*>(zp + g);
                wz[it][1] = *reinterpret_cast<const float4*>(zp + g + 2);
                wu[it][0] = *reinterpret_cast<const float4*>(up + g);
                wu[it][1] = *reinterpret_cast<const float4*>(up + g + 2);
            }
        }
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int it = 0; it < kResIters; ++it) {
        if (!on[it]) continue;
        // primal: x - z with x taken as complex with zero imaginary part (the imaginary difference is -Im z: exact)
        acc[0] += sq(vx[it].x - vz[it][0].x) + sq(vz[it][0].y) + sq(vx[it].y - vz[it][0].z) + sq(vz[it][0].w) +
                  sq(vx[it].z - vz[it][1].x) + sq(vz[it][1].y) + sq(vx[it].w - vz[it][1].z) + sq(vz[it][1].w);
        if (DELTA) {
            acc[1] += sq(vx[it].x - wx[it].x) + sq(vx[it].y - wx[it].y) + sq(vx[it].z - wx[it].z) + sq(vx[it].w - wx[it].w);
            acc[2] += diff2(vz[it][0], wz[it][0]) + diff2(vz[it][1], wz[it][1]);
            acc[3] += diff2(vu[it][0], wu[it][0]) + diff2(vu[it][1], wu[it][1]);
        }
    }
    block_sums_fixed<kResThreads, 4>(acc, red);
    if (threadIdx.x == 0) {
        double* o = partial + ((size_t)n * gridDim.x + blockIdx.x) * 4;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2]; o[3] = acc[3];
    }
}

__global__ __launch_bounds__(kResThreads) void misfit_tile_kernel(const float2* __restrict__ fx, const float2* __restrict__ y0s,
                                                                  const uint8_t* __restrict__ masks, int mask_n,
                                                                  double* __restrict__ partial, int HW) {
    __shared__ double red[kResThreads / 64];
    const int n = blockIdx.y;
    const size_t base = (size_t)n * HW, mbase = mask_n > 1 ? base : 0;
    const int p0 = blockIdx.x * kPixelChunk;
    float4 a[kResIters][2], b[kResIters][2];
    unsigned m[kResIters];
    bool on[kResIters];
#pragma unroll
    for (int it = 0; it < kResIters; ++it) {
        const int p = p0 + (it * kResThreads + (int)threadIdx.x) * 4;
        on[it] = p < HW;
        if (on[it]) {
            const size_t g = base + p;
            a[it][0] = *reinterpret_cast<const float4*>(fx + g);
            a[it][1] = *reinterpret_cast<const float4*>(fx + g + 2);
            b[it][0] = *reinterpret_cast<const float4*>(y0s + g);
            b[it][1] = *reinterpret_cast<const float4*>(y0s + g + 2);
            m[it] = *reinterpret_cast<const unsigned*>(masks + mbase + p);      // four mask bytes (0 / 1 each)
        }
    }
    double acc[1] = {0.0};
#pragma unroll
    for (int it = 0; it < kResIters; ++it) {
        if (!on[it]) continue;
        if (m[it] & 0x000000ffu) acc[0] += sq(a[it][0].x - b[it][0].x) + sq(a[it][0].y - b[it][0].y);
        if (m[it] & 0x0000ff00u) acc[0] += sq(a[it][0].z - b[it][0].z) + sq(a[it][0].w - b[it][0].w);
        if (m[it] & 0x00ff0000u) acc[0] += sq(a[it][1].x - b[it][1].x) + sq(a[it][1].y - b[it][1].y);
        if (m[it] & 0xff000000u) acc[0] += sq(a[it][1].z - b[it][1].z) + sq(a[it][1].w - b[it][1].w);
    }
    block_sums_fixed<kResThreads, 1>(acc, red);
    if (threadIdx.x == 0) partial[(size_t)n * gridDim.x + blockIdx.x] = acc[0];
}

__global__ __launch_bounds__(kResThreads) void residual_reduce_kernel(const double* __restrict__ partial, const double* __restrict__ dcpartial,
                                                                      int chunks, int has_delta, int has_dc, double inv_sqrt_hw,
                                                                      float* __restrict__ out) {
    __shared__ double red[5 * (kResThreads / 64)];
    const int n = blockIdx.x;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < chunks; i += kResThreads) {
        const double* p = partial + ((size_t)n * chunks + i) * 4;
        acc[0] += p[0];
        if (has_delta) { acc[1] += p[1]; acc[2] += p[2]; acc[3] += p[3]; }
        if (has_dc) acc[4] += dcpartial[(size_t)n * chunks + i];
    }
    block_sums_fixed<kResThreads, 5>(acc, red);
    if (threadIdx.x == 0) {
        const double dx = sqrt(acc[1]), dz = sqrt(acc[2]), du = sqrt(acc[3]);
        float* o = out + (size_t)n * 6;
        o[0] = (float)sqrt(acc[0]);
        o[1] = (float)dx; o[2] = (float)dz; o[3] = (float)du;
        o[4] = (float)((dx + dz + du) * inv_sqrt_hw);
        o[5] = (float)sqrt(acc[4]);
    }
}

}  // namespace

hipError_t launch_residual_tiles(const float* x, const float2* z, const float2* u, const float* xp, const float2* zp, const float2* up,
                                 double* partial, int N, int H, int W, hipStream_t s) {
    const dim3 grid(pixel_chunks(H, W), N);
    if (xp != nullptr) hipLaunchKernelGGL(residual_tile_kernel<true>, grid, dim3(kResThreads), 0, s, x, z, u, xp, zp, up, partial, H * W);
    else hipLaunchKernelGGL(residual_tile_kernel<false>, grid, dim3(kResThreads), 0, s, x, z, u, xp, zp, up, partial, H * W);
    return hipGetLastError();
}

hipError_t launch_misfit_tiles(const float2* fx, const float2* y0s, const uint8_t* masks, int mask_n, double* dcpartial, int N, int H, int W,
                               hipStream_t s) {
    hipLaunchKernelGGL(misfit_tile_kernel, dim3(pixel_chunks(H, W), N), dim3(kResThreads), 0, s, fx, y0s, masks, mask_n, dcpartial, H * W);
    return hipGetLastError();
}

hipError_t launch_residual_reduce(const double* partial, const double* dcpartial, int has_delta, int has_dc, float* out, int N, int H, int W,
                                  hipStream_t s) {
    hipLaunchKernelGGL(residual_reduce_kernel, dim3(N), dim3(kResThreads), 0, s, partial, dcpartial, pixel_chunks(H, W), has_delta, has_dc,
                       1.0 / sqrt((double)H * (double)W), out);
    return hipGetLastError();
}

}  // namespace pnp
