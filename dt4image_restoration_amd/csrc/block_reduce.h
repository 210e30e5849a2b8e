// Bit-reproducible per-slice reductions shared by the pointwise kernels (residuals, SENSE, coil maps, acquisition, SSIM, PSNR): the pixel
// range a workgroup owns and the fixed-order workgroup sum / maximum.  No atomics: the same bits on every call.
#pragma once
#include <hip/hip_runtime.h>

namespace pnp {

// One workgroup owns kPixelChunk consecutive pixels of ONE slice (plane).  The range depends on the slice's size only, never on the
// batch, so a slice gives the same bits wherever it sits in a handle.
static constexpr int kPixelChunk = 2048;
inline int pixel_chunks(int H, int W) { return (H * W + kPixelChunk - 1) / kPixelChunk; }   // workgroups (= partials per quantity) per slice

// Fixed tree of a THREADS-wide workgroup: a 64-lane shuffle ladder, the wave leaders through LDS, then thread 0 over the wave values in
// index order, starting from 0.0.  Any other order changes result bits.  THREADS = 0: the width is the launch's blockDim.x (psnr_kernel).
template <int THREADS>
__device__ __forceinline__ int block_waves() { return THREADS ? THREADS / 64 : (int)(blockDim.x >> 6); }

// Sums of Q quantities at once.  v[]: the thread's terms (left holding ladder partials); `red` holds Q * waves doubles; thread 0 gets the
// totals in total[], no other thread writes it.  The two forms below differ only in what a thread other than 0 holds afterwards, which
// nothing reads; each kernel keeps the form it was written with, so that its instruction stream stays as it was.
template <int THREADS, int Q>
__device__ __forceinline__ void block_sums_fixed(double (&v)[Q], double* red, double (&total)[Q]) {
#pragma unroll
    for (int q = 0; q < Q; ++q)
        for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_down(v[q], o);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < Q; ++q) red[q * block_waves<THREADS>() + (threadIdx.x >> 6)] = v[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            double t = 0.0;
            for (int i = 0; i < block_waves<THREADS>(); ++i) t += red[q * block_waves<THREADS>() + i];
            total[q] = t;
        }
    }
}
// in place: thread 0 returns the totals in v[]
template <int THREADS, int Q>
__device__ __forceinline__ void block_sums_fixed(double (&v)[Q], double* red) { block_sums_fixed<THREADS, Q>(v, red, v); }
// one quantity by value: thread 0 returns the total, every other thread 0.0
template <int THREADS>
__device__ __forceinline__ double block_sum_fixed(double v, double* red) {
    double a[1] = {v}, t[1] = {0.0};
    block_sums_fixed<THREADS, 1>(a, red, t);
    return t[0];
}

// Maximum by the same tree, thread 0 starting from red[0]: `red` holds THREADS / 64 floats; thread 0 returns it.
template <int THREADS>
__device__ __forceinline__ float block_max_fixed(float v, float* red) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = red[0];
        for (int i = 1; i < THREADS / 64; ++i) t = fmaxf(t, red[i]);
        v = t;
    }
    return v;
}

}  // namespace pnp
