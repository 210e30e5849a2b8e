// Simulated CS-MRI acquisition on the device (pnp_acquire): per slice n, in the reference's centred layout,
//     y0   = mask ? fft_c(gt) + sigma_n * (g_re + i g_im) : 0
//     aty0 = ifft_c(y0)
//     x0   = max(aty0, 0) on both planes
// what synthetic.make_problem computes in numpy float64, with the same noise number for number: g = synthetic._gauss over the counter hash
// of weights.hash_uniform (splitmix64 of (seed + n, stream, centred pixel index)).
//
// Shift folding (H/2 and W/2 even, so the centred pixel p = S k has the parity of the plain bin k; sgn[k] = (-1)^(k1 + k2)):
//     fft_c(gt)[S k] = sgn[k] * FFT(gt)[k]                     (plain orthonormal transform)
//     ifft_c(y0)     = IFFT(Z'),  Z'[k] = sgn[k] * y0[S k]     (no shift left on the image side: the convention of reset_kernel's y0s)
// so the engine's own plain passes run on both sides of ONE pointwise kernel:
//   rows-forward (real input)  gt -> work         existing kernels, gt read once, no complex copy of it
//   cols-forward               work, in place     existing kernels
//   acquire_epilogue_kernel    y0[p] = mask[p] ? sgn * work[k] + noise(p) : +0;  work[k] = sgn * y0[p]
//   cols-inverse, rows-inverse work -> aty0       existing kernels
//   acquire_clamp_kernel       x0 = max(aty0, 0)
// The epilogue is indexed by the centred pixel (mask, y0 and the noise counter are contiguous; the scratch is read and written in runs of
// W/2).  The integer hash is exact; Box-Muller, the product with sigma_n and the sum with the transform are formed in float64 and rounded to
// float32 once.  Only sampled bins pay for the float64 log / sqrt / cos (compacted per workgroup).  A workgroup owns a fixed range of one slice's pixels, and the
// counter is (seed + n, p): a slice's bits do not depend on the batch or on its place in it.
#include "pnp_internal.h"
#include "block_reduce.h"
#include "noise_hash.h"

namespace pnp {

namespace {

constexpr int kAcqThreads = 256;
constexpr unsigned kStreamRe = kNoiseStreamRe, kStreamIm = kNoiseStreamIm;

// One workgroup per kPixelChunk consecutive centred pixels of one slice.  Pass 1 reads the mask, zeroes the unsampled bins and compacts the
// sampled pixels into an LDS list; pass 2 walks the list, so that the float64 Box-Muller (some 700 instructions a pixel, 4 cycles each on a
// wave of 64) is issued by full waves over the sampled fraction instead of by every wave of a scattered radial mask.  The order of the list
// (LDS atomics) varies from run to run; a pixel's value does not depend on it.
__global__ __launch_bounds__(kAcqThreads) void acquire_epilogue_kernel(float2* __restrict__ work, const uint8_t* __restrict__ mask, int mask_n,
                                                                       float2* __restrict__ y0, double sigma, unsigned long long seed,
                                                                       int H, int W, int coils) {
    __shared__ int list[kPixelChunk];
    __shared__ int count;
    constexpr int PER = kPixelChunk / kAcqThreads;
    // plane blockIdx.y = coil c of slice n (pnp_acquire: one plane per slice, c = 0)
    const int n = blockIdx.y / coils, c = blockIdx.y - n * coils, hw = H * W, hh = H >> 1, hwd = W >> 1;
    const int p0 = blockIdx.x * kPixelChunk + threadIdx.x;
    const size_t base = (size_t)blockIdx.y * hw;
    const uint8_t* const mk = mask + (mask_n > 1 ? (size_t)n * hw : 0);
    // plain bin k = S^-1 p of the centred pixel p (H/2, W/2 even: the parities of p's and k's coordinates agree)
    auto plain = [&](int p, int& par) {
        const int r = p / W, c = p - r * W;
        par = (r + c) & 1;
        return base + (size_t)(r < hh ? r + hh : r - hh) * W + (c < hwd ? c + hwd : c - hwd);
    };
    if (threadIdx.x == 0) count = 0;
    __syncthreads();
    uint8_t mm[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int p = p0 + j * kAcqThreads;
        mm[j] = p < hw ? mk[p] : (uint8_t)0;
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int p = p0 + j * kAcqThreads;
        if (p >= hw) continue;
        if (mm[j]) {
            list[atomicAdd(&count, 1)] = p;
        } else {
            int par;
            const size_t k = plain(p, par);
            y0[base + p] = make_float2(0.f, 0.f);
            work[k] = make_float2(0.f, 0.f);
        }
    }
    __syncthreads();
    const int cnt = count;
    const unsigned long long sn = (seed + (unsigned long long)n) * 0x100000001B3ull;
    const unsigned tre = kStreamRe + 4u * (unsigned)c, tim = kStreamIm + 4u * (unsigned)c;     // coil c draws the streams 9001 + 4 c, 9003 + 4 c
    const unsigned long long bre1 = splitmix64(sn + tre), bre2 = splitmix64(sn + tre + 1u);
    const unsigned long long bim1 = splitmix64(sn + tim), bim2 = splitmix64(sn + tim + 1u);
    for (int i = threadIdx.x; i < cnt; i += kAcqThreads) {
        const int p = list[i];
        int par;
        const size_t k = plain(p, par);
        const float sg = par ? -1.f : 1.f;
        const float2 f = work[k];
        float2 v = make_float2(sg * f.x, sg * f.y);
        if (sigma != 0.0) {                                 // uniform: a noiseless acquisition draws nothing and keeps the transform's own bits
            v.x = (float)((double)v.x + gauss64(bre1, bre2, (unsigned long long)p) * sigma);
            v.y = (float)((double)v.y + gauss64(bim1, bim2, (unsigned long long)p) * sigma);
        }
        y0[base + p] = v;
        work[k] = make_float2(sg * v.x, sg * v.y);
    }
}

// x0 = max(aty0, 0) on both planes
__global__ __launch_bounds__(kAcqThreads) void acquire_clamp_kernel(const float2* __restrict__ a, float2* __restrict__ x0, size_t total) {
    for (size_t i = (size_t)blockIdx.x * kAcqThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kAcqThreads) {
        const float2 v = a[i];
        x0[i] = make_float2(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f));
    }
}

}  // namespace

hipError_t launch_acquire_epilogue(float2* work, const uint8_t* mask, int mask_n, float2* y0, double sigma, uint64_t seed, int N, int H, int W,
                                   hipStream_t s, int coils) {
    hipLaunchKernelGGL(acquire_epilogue_kernel, dim3(pixel_chunks(H, W), N * coils), dim3(kAcqThreads), 0, s, work, mask, mask_n, y0,
                       sigma, (unsigned long long)seed, H, W, coils);
    return hipGetLastError();
}

hipError_t launch_acquire_clamp(const float2* aty0, float2* x0, int N, int H, int W, hipStream_t s) {
    const size_t total = (size_t)N * H * W;
    size_t blocks = (total + kAcqThreads - 1) / kAcqThreads;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(acquire_clamp_kernel, dim3((unsigned)blocks), dim3(kAcqThreads), 0, s, aty0, x0, total);
    return hipGetLastError();
}

}  // namespace pnp
