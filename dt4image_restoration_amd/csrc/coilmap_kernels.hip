// Coil sensitivity maps from the calibration block (pnp_estimate_sens): the low-resolution estimate, per slice n and coil c,
//     k_c = in block ? float32(win) * y[n, c] : 0        l_c = ifft_c(k_c)        rss = sqrt(sum_c |l_c|^2)        smax = max over the slice of rss
//     S_c = (rss > 0 and rss > float32(thresh) * smax) ? l_c / rss : 0
// with the block -acs_h/2 <= dy < acs_h/2, -acs_w/2 <= dx < acs_w/2 around the centre bin (dy = ky - H/2, dx = kx - W/2) and the window 1 (box) or
// (0.5 + 0.5 cos(2 pi dy / acs_h)) (0.5 + 0.5 cos(2 pi dx / acs_w)) (Hann), its factors and their product formed in float64, rounded to float32 once.
//
// Shift folding (H/2, W/2 even; sgn[k] = (-1)^(k1 + k2), S = the half-size roll): ifft_c(q) = IFFT(sgn[k] q[S k]), reset_kernel's y0s convention, so
// the engine's plain inverse passes run in place in the caller's map buffer between pointwise kernels:
//   coilmap_window_kernel     indexed by the plain bin k: sens[n, c][k] = in block(S k) ? sgn[k] * win * y[n, c][S k] : 0   (y is read inside the block only)
//   cols inverse, rows inverse (existing kernels, in place, batch N * C)                                                   sens = l_c
//   coilmap_rss_kernel        rss (float64 sum over the coils in coil order, one rounding), the workgroup's maximum -> partial[n, chunk]
//   coilmap_max_kernel        smax[n] = max of the slice's partials
//   coilmap_normalise_kernel  S_c in place (the float32 division is an IEEE divide)
// The centred bin S k of the plain bin k has dy = k1 (k1 < H/2) or k1 - H: the block is the four corners of the plain plane.
// Every workgroup owns kPixelChunk consecutive pixels of one plane (slice), no atomics: a slice's bits depend on (y[n], acs, window, thresh) only.
#include "pnp_internal.h"
#include "block_reduce.h"

namespace pnp {

namespace {

constexpr int kCoilmapThreads = 256;
constexpr int kCoilmapPer = kPixelChunk / kCoilmapThreads;     // pixels per thread
static_assert(kPixelChunk % kCoilmapThreads == 0, "whole pixels per thread");

// one Hann factor at offset d of a block side L, float64
__device__ __forceinline__ double hann64(int d, int L) { return 0.5 + 0.5 * cos((2.0 * 3.14159265358979323846) * (double)d / (double)L); }

// grid (chunks, N * C); sens[nc][k] = in block(S k) ? sgn[k] * win * y[nc][S k] : 0
__global__ __launch_bounds__(kCoilmapThreads) void coilmap_window_kernel(const float2* __restrict__ y, float2* __restrict__ sens, int acs_h, int acs_w,
                                                                         int hann, int H, int W) {
    const int HW = H * W, hh = H >> 1, hw = W >> 1, ah = acs_h >> 1, aw = acs_w >> 1;
    const size_t base = (size_t)blockIdx.y * HW;
    const int p0 = blockIdx.x * kPixelChunk + threadIdx.x;
    int src[kCoilmapPer];                                   // centred index S k of an in-block bin, -1 outside the block (or the plane)
    float2 v[kCoilmapPer];
#pragma unroll
    for (int j = 0; j < kCoilmapPer; ++j) {
        const int p = p0 + j * kCoilmapThreads;
        const int k1 = p / W, k2 = p - k1 * W;
        const int dy = k1 < hh ? k1 : k1 - H, dx = k2 < hw ? k2 : k2 - W;
        const bool in = p < HW && dy >= -ah && dy < ah && dx >= -aw && dx < aw;
        src[j] = in ? (dy + hh) * W + (dx + hw) : -1;
    }
#pragma unroll
    for (int j = 0; j < kCoilmapPer; ++j)
        if (src[j] >= 0) v[j] = y[base + src[j]];
#pragma unroll
    for (int j = 0; j < kCoilmapPer; ++j) {
        const int p = p0 + j * kCoilmapThreads;
        if (p >= HW) continue;
        float2 o = make_float2(0.f, 0.f);
        if (src[j] >= 0) {
            const int ky = src[j] / W, kx = src[j] - ky * W;
            const int k1 = p / W, k2 = p - k1 * W;
            float wv = ((k1 + k2) & 1) ? -1.f : 1.f;
            if (hann) wv *= (float)(hann64(ky - hh, acs_h) * hann64(kx - hw, acs_w));
            o = make_float2(wv * v[j].x, wv * v[j].y);
        }
        sens[base + p] = o;
    }
}

// grid (chunks, N); rss[n, p] = float32(sqrt(sum_c |l[n, c, p]|^2)), the sum in float64 in coil order; partial[n, chunk] = the chunk's maximum
__global__ __launch_bounds__(kCoilmapThreads) void coilmap_rss_kernel(const float2* __restrict__ l, int C, float* __restrict__ rss,
                                                                      float* __restrict__ partial, int HW) {
    __shared__ float red[kCoilmapThreads / 64];
    const int n = blockIdx.y;
    const int p0 = blockIdx.x * kPixelChunk + threadIdx.x;
    double acc[kCoilmapPer];
#pragma unroll
    for (int j = 0; j < kCoilmapPer; ++j) acc[j] = 0.0;
    for (int c = 0; c < C; ++c) {
        const float2* lc = l + ((size_t)n * C + c) * HW;
        float2 v[kCoilmapPer];
#pragma unroll
        for (int j = 0; j < kCoilmapPer; ++j) {
            const int p = p0 + j * kCoilmapThreads;
            v[j] = p < HW ? lc[p] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int j = 0; j < kCoilmapPer; ++j) acc[j] += (double)v[j].x * (double)v[j].x + (double)v[j].y * (double)v[j].y;
    }
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < kCoilmapPer; ++j) {
        const int p = p0 + j * kCoilmapThreads;
        if (p < HW) {
            const float r = (float)sqrt(acc[j]);
            rss[(size_t)n * HW + p] = r;
            m = fmaxf(m, r);
        }
    }
    m = block_max_fixed<kCoilmapThreads>(m, red);
    if (threadIdx.x == 0) partial[(size_t)n * gridDim.x + blockIdx.x] = m;
}

// grid (N); smax[n] = max of partial[n, 0 .. chunks)
__global__ __launch_bounds__(kCoilmapThreads) void coilmap_max_kernel(const float* __restrict__ partial, int chunks, float* __restrict__ smax) {
    __shared__ float red[kCoilmapThreads / 64];
    const int n = blockIdx.x;
    float m = 0.f;
    for (int i = threadIdx.x; i < chunks; i += kCoilmapThreads) m = fmaxf(m, partial[(size_t)n * chunks + i]);
    m = block_max_fixed<kCoilmapThreads>(m, red);
    if (threadIdx.x == 0) smax[n] = m;
}

// grid (chunks, N); l[n, c, p] <- (rss > 0 and rss > thresh * smax[n]) ? l / rss : 0
__global__ __launch_bounds__(kCoilmapThreads) void coilmap_normalise_kernel(float2* __restrict__ l, int C, const float* __restrict__ rss,
                                                                            const float* __restrict__ smax, float thresh, int HW) {
    const int n = blockIdx.y;
    const int p0 = blockIdx.x * kPixelChunk + threadIdx.x;
    const float cut = thresh * smax[n];
    float r[kCoilmapPer];
#pragma unroll
    for (int j = 0; j < kCoilmapPer; ++j) {
        const int p = p0 + j * kCoilmapThreads;
        r[j] = p < HW ? rss[(size_t)n * HW + p] : 0.f;
    }
    for (int c = 0; c < C; ++c) {
        float2* lc = l + ((size_t)n * C + c) * HW;
        float2 v[kCoilmapPer];
#pragma unroll
        for (int j = 0; j < kCoilmapPer; ++j) {
            const int p = p0 + j * kCoilmapThreads;
            if (p < HW) v[j] = lc[p];
        }
#pragma unroll
        for (int j = 0; j < kCoilmapPer; ++j) {
            const int p = p0 + j * kCoilmapThreads;
            if (p < HW) {
                const bool keep = r[j] > 0.f && r[j] > cut;
                lc[p] = keep ? make_float2(v[j].x / r[j], v[j].y / r[j]) : make_float2(0.f, 0.f);
            }
        }
    }
}

inline dim3 plane_grid(int H, int W, int batch) { return dim3((unsigned)pixel_chunks(H, W), (unsigned)batch); }

}  // namespace

hipError_t launch_coilmap_window(const float2* y, float2* sens, int acs_h, int acs_w, int hann, int N, int C, int H, int W, hipStream_t s) {
    hipLaunchKernelGGL(coilmap_window_kernel, plane_grid(H, W, N * C), dim3(kCoilmapThreads), 0, s, y, sens, acs_h, acs_w, hann, H, W);
    return hipGetLastError();
}

hipError_t launch_coilmap_rss(const float2* l, int C, float* rss, float* partial, int N, int H, int W, hipStream_t s) {
    hipLaunchKernelGGL(coilmap_rss_kernel, plane_grid(H, W, N), dim3(kCoilmapThreads), 0, s, l, C, rss, partial, H * W);
    return hipGetLastError();
}

hipError_t launch_coilmap_max(const float* partial, float* smax, int N, int H, int W, hipStream_t s) {
    hipLaunchKernelGGL(coilmap_max_kernel, dim3(N), dim3(kCoilmapThreads), 0, s, partial, pixel_chunks(H, W), smax);
    return hipGetLastError();
}

hipError_t launch_coilmap_normalise(float2* l, int C, const float* rss, const float* smax, float thresh, int N, int H, int W, hipStream_t s) {
    hipLaunchKernelGGL(coilmap_normalise_kernel, plane_grid(H, W, N), dim3(kCoilmapThreads), 0, s, l, C, rss, smax, thresh, H * W);
    return hipGetLastError();
}

}  // namespace pnp
