// Image-quality metrics on the device: SSIM with scipy's Gaussian window (pnp_ssim).
//
// SSIM exactly as evaluation/utils/transformations.py:61-95 defines it: G = gaussian_filter(sigma = 1.5, truncate = win // 2),
// separable, radius R, taps exp(-x^2 / (2 sigma^2)) / sum, boundary 'reflect' (d c b a | a b c d | d c b a);
//   mu = G*x,  sigma_x^2 = G*(x^2) - mu_x^2,  sigma_xy = G*(x y) - mu_x mu_y,
//   map = (2 mu_x mu_y + c1)(2 sigma_xy + c2) / ((mu_x^2 + mu_y^2 + c1)(sigma_x^2 + sigma_y^2 + c2)),  score = mean(map) over H x W.
//
// ssim_tile_kernel<R>: one workgroup (256 threads) per 32 x 32 output tile of one slice.  It stages the (32 + 2R)^2 patch of x and gt in
// LDS with the reflection folded into the load address (H, W >= 16 >= R: one reflection always suffices; positions of a tile past the
// image edge are clamped and never stored), runs the horizontal pass of the five products (x, y, x^2, y^2, xy) into LDS, then the
// vertical pass and the SSIM formula per output pixel, optionally stores the map, and writes the tile's sum as ONE f64 partial.
// ssim_reduce_kernel sums a slice's partials in a fixed order.  No atomics anywhere: the score is bitwise reproducible.
// The filter arithmetic is plain fmaf on tap weights the compiler holds in scalar registers (kernel arguments, unrolled R); the built
// code objects carry no packed-FP32 op whose low result reads the high register of a pair (tools/isa_audit.py, tests/test_ssim_host.py).
#include "pnp_internal.h"
#include "block_reduce.h"

namespace pnp {

namespace {

constexpr int kSsimTW = 32, kSsimTH = 32, kSsimThreads = 256;

template <int R> struct SsimShape {
    static constexpr int KS = 2 * R + 1;                 // taps
    static constexpr int PH = kSsimTH + 2 * R;           // patch rows (= rows of the horizontal pass)
    static constexpr int PW = kSsimTW + 2 * R;           // patch columns
    static constexpr int PWP = PW + 1;                   // odd row stride: a half-wave's 4 rows x 8 segments hit 32 distinct banks (R = 8)
    static constexpr int HZP = kSsimTW + 4;              // horizontal-pass row stride: 16-byte aligned rows for the float4 stores
    static constexpr int HZ_OFF = (2 * PH * PWP + 3) & ~3;
    static constexpr int LDS_FLOATS = HZ_OFF + 5 * PH * HZP;
};

// scipy 'reflect' (half-sample symmetric), then a clamp that only matters for positions of a tile past the image edge (never stored)
__device__ __forceinline__ int reflect_index(int i, int n) {
    i = i < 0 ? -i - 1 : i;
    i = i >= n ? 2 * n - 1 - i : i;
    return min(max(i, 0), n - 1);
}

template <int R>
__global__ __launch_bounds__(kSsimThreads) void ssim_tile_kernel(SsimArgs a) {
    using S = SsimShape<R>;
    extern __shared__ float4 ssim_lds4[];
    __shared__ double red[kSsimThreads / 64];
    float* sx = reinterpret_cast<float*>(ssim_lds4);
    float* sy = sx + S::PH * S::PWP;
    float* hz = sx + S::HZ_OFF;                          // [5][PH][HZP]
    const int tid = threadIdx.x;
    const int n = blockIdx.z;
    const int tx0 = blockIdx.x * kSsimTW, ty0 = blockIdx.y * kSsimTH;
    const int H = a.H, W = a.W;
    const size_t plane = (size_t)H * W;
    const float* xp = a.x + (size_t)n * plane;
    const float* gp = a.gt + (size_t)n * plane;

    // 1. patch of x (clamped to [0, 1] on request) and gt, reflected at the image border
    for (int i = tid; i < S::PH * S::PW; i += kSsimThreads) {
        const int r = i / S::PW, c = i - r * S::PW;
        const size_t g = (size_t)reflect_index(ty0 + r - R, H) * W + reflect_index(tx0 + c - R, W);
        float xv = xp[g];
        if (a.clamp_x) xv = fminf(fmaxf(xv, 0.f), 1.f);
        sx[r * S::PWP + c] = xv;
        sy[r * S::PWP + c] = gp[g];
    }
    __syncthreads();

    // 2. horizontal pass: every patch row, 4 consecutive output columns per thread; each input value is read once and feeds the
    //    (up to 4) outputs whose window covers it
    for (int s = tid; s < S::PH * (kSsimTW / 4); s += kSsimThreads) {
        const int r = s / (kSsimTW / 4), c0 = (s % (kSsimTW / 4)) * 4;
        const float* rx = sx + r * S::PWP + c0;
        const float* ry = sy + r * S::PWP + c0;
        float acc[5][4];
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[q][j] = 0.f;
#pragma unroll
        for (int t = 0; t < S::KS + 3; ++t) {
            const float xv = rx[t], yv = ry[t];
            const float p[5] = {xv, yv, xv * xv, yv * yv, xv * yv};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = t - j;
                if (k < 0 || k >= S::KS) continue;
#pragma unroll
                for (int q = 0; q < 5; ++q) acc[q][j] = fmaf(a.w[k], p[q], acc[q][j]);
            }
        }
#pragma unroll
        for (int q = 0; q < 5; ++q)
            *reinterpret_cast<float4*>(hz + (q * S::PH + r) * S::HZP + c0) = make_float4(acc[q][0], acc[q][1], acc[q][2], acc[q][3]);
    }
    __syncthreads();

    // 3. vertical pass: one column, 4 consecutive output rows per thread (a half-wave reads one contiguous LDS row), then the formula
    const int c = tid & (kSsimTW - 1), r0 = (tid / kSsimTW) * 4;
    float acc[5][4];
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[q][j] = 0.f;
#pragma unroll
    for (int t = 0; t < S::KS + 3; ++t) {
        float v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = hz[(q * S::PH + r0 + t) * S::HZP + c];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = t - j;
            if (k < 0 || k >= S::KS) continue;
#pragma unroll
            for (int q = 0; q < 5; ++q) acc[q][j] = fmaf(a.w[k], v[q], acc[q][j]);
        }
    }
    const int gx = tx0 + c;
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float mx = acc[0][j], my = acc[1][j];
        const float vx = acc[2][j] - mx * mx, vy = acc[3][j] - my * my, cxy = acc[4][j] - mx * my;
        const float num = (2.f * mx * my + a.c1) * (2.f * cxy + a.c2);
        const float den = (mx * mx + my * my + a.c1) * (vx + vy + a.c2);
        const float m = num / den;
        const int gy = ty0 + r0 + j;
        if (gx < W && gy < H) {
            if (a.map) a.map[(size_t)n * plane + (size_t)gy * W + gx] = m;
            sum += (double)m;
        }
    }
    const double t = block_sum_fixed<kSsimThreads>(sum, red);
    if (tid == 0) a.partial[((size_t)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = t;
}

__global__ __launch_bounds__(kSsimThreads) void ssim_reduce_kernel(const double* __restrict__ partial, int tiles, double inv_hw,
                                                                   float* __restrict__ out) {
    __shared__ double red[kSsimThreads / 64];
    const int n = blockIdx.x;
    double acc = 0.0;
    for (int i = threadIdx.x; i < tiles; i += kSsimThreads) acc += partial[(size_t)n * tiles + i];
    const double t = block_sum_fixed<kSsimThreads>(acc, red);
    if (threadIdx.x == 0) out[n] = (float)(t * inv_hw);
}

template <int R>
hipError_t launch_tile(const SsimArgs& a, int N, int tiles_x, int tiles_y, hipStream_t s) {
    static DeviceOnce once;
    const int bytes = SsimShape<R>::LDS_FLOATS * (int)sizeof(float);
    if (bytes > 64 * 1024) {
        hipError_t e = raise_lds_cap(reinterpret_cast<const void*>(&ssim_tile_kernel<R>), bytes, once);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(ssim_tile_kernel<R>, dim3(tiles_x, tiles_y, N), dim3(kSsimThreads), bytes, s, a);
    return hipGetLastError();
}

}  // namespace

int ssim_tiles(int H, int W) { return ((W + kSsimTW - 1) / kSsimTW) * ((H + kSsimTH - 1) / kSsimTH); }

hipError_t launch_ssim(const SsimArgs& args, int N, hipStream_t s) {
    const int tx = (args.W + kSsimTW - 1) / kSsimTW, ty = (args.H + kSsimTH - 1) / kSsimTH;
    hipError_t e;
    switch (args.radius) {
        case 1: e = launch_tile<1>(args, N, tx, ty, s); break;
        case 2: e = launch_tile<2>(args, N, tx, ty, s); break;
        case 3: e = launch_tile<3>(args, N, tx, ty, s); break;
        case 4: e = launch_tile<4>(args, N, tx, ty, s); break;
        case 5: e = launch_tile<5>(args, N, tx, ty, s); break;
        case 6: e = launch_tile<6>(args, N, tx, ty, s); break;
        case 7: e = launch_tile<7>(args, N, tx, ty, s); break;
        case 8: e = launch_tile<8>(args, N, tx, ty, s); break;
        case 9: e = launch_tile<9>(args, N, tx, ty, s); break;
        case 10: e = launch_tile<10>(args, N, tx, ty, s); break;
        case 11: e = launch_tile<11>(args, N, tx, ty, s); break;
        case 12: e = launch_tile<12>(args, N, tx, ty, s); break;
        case 13: e = launch_tile<13>(args, N, tx, ty, s); break;
        case 14: e = launch_tile<14>(args, N, tx, ty, s); break;
        case 15: e = launch_tile<15>(args, N, tx, ty, s); break;
        case 16: e = launch_tile<16>(args, N, tx, ty, s); break;
        default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ssim_reduce_kernel, dim3(N), dim3(kSsimThreads), 0, s, args.partial, tx * ty,
                       1.0 / ((double)args.H * (double)args.W), args.out);
    return hipGetLastError();
}

}  // namespace pnp
