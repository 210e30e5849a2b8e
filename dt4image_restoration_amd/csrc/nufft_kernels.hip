// Non-Cartesian sampling: the kernels of the NUFFT pair (include/pnpadmm.h, "non-Cartesian data fidelity") around the engine's centred
// grid transform (launch_fft_rows / launch_fft_cols on the oversampled gh x gw grid, with the plan's own twiddles).
//
//   forward   nufft_pad_kernel     grid = zero-padded (cy cx) . image            | rows forward | cols forward (centred) |
//             nufft_interp_kernel  y_m = sum_iy wy[iy] (sum_ix wx[ix] grid[i0y + iy][i0x + ix])     a gather, a thread per (slice, sample)
//   adjoint   nufft_grid_kernel    grid[g] = sum over the samples of the tile's bin, ascending, of (w_m y_m wy) wx
//             | rows inverse | cols inverse (centred) |
//             nufft_crop_kernel    image = (cy cx) . crop(grid)  (+ mu p and the partial sums of Re<p, q>: the normal operator's last launch)
//
// Gridding has no atomics.  One workgroup owns one kNufftTile^2 tile of one slice's grid and walks the tile's bin (nufft_plan.h: the
// ascending list of the samples whose periodic footprint meets the tile) in chunks of kGridChunk samples.  A chunk is staged in LDS as, per
// sample, the row vector a[ty] = (w_m y_m) wy restricted to the tile's rows and the column vector wx restricted to its columns, both zero
// outside the footprint; every thread then runs acc = fma(a[ty], wx[tx], acc) over the chunk: a dense rank-1 update with no divergence.
// fma(a, +-0, acc) and fma(+-0, wx, acc) leave a finite chain's value unchanged, so a grid point's value is the fma chain from +0 over the
// samples whose footprint contains it, in ascending sample index, whatever the tile size: the bits depend on (plan, data) only.
#include "pnp_internal.h"
#include "block_reduce.h"
#include "noise_hash.h"
#include "nufft_plan.h"

namespace pnp {

namespace {

constexpr int kNcThreads = 256;
constexpr int kNcPer = kPixelChunk / kNcThreads;          // pixels (or samples) per thread of the chunked pointwise kernels
static_assert(kPixelChunk % kNcThreads == 0, "whole pixels per thread");
constexpr int kGridChunk = 128;                            // samples staged per pass: 128 x 16 x (8 + 4) B = 24 KiB of LDS
static_assert(kNufftTile * kNufftTile == kNcThreads, "a thread per grid point of the tile");

__device__ __forceinline__ bool stopped(const float* tact, int n) { return tact != nullptr && tact[n] > 0.5f; }

// grid[n][gy][gx] = inside the centred h x w window ? (cy[iy] cx[ix]) src[n][iy][ix] : 0; src complex, or a real image (REAL)
template <bool REAL>
__global__ __launch_bounds__(kNcThreads) void nufft_pad_kernel(const void* __restrict__ src, const float* __restrict__ cy,
                                                               const float* __restrict__ cx, float2* __restrict__ grid, int H, int W, int gh,
                                                               int gw) {
    const int n = blockIdx.y, G = gh * gw;
    const int g = blockIdx.x * kNcThreads + threadIdx.x;
    if (g >= G) return;
    const int gy = g / gw, gx = g - gy * gw;
    const int iy = gy - (gh / 2 - H / 2), ix = gx - (gw / 2 - W / 2);
    float2 v = make_float2(0.f, 0.f);
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
        const size_t p = ((size_t)n * H + iy) * W + ix;
        const float f = cy[iy] * cx[ix];
        if (REAL) v = make_float2(static_cast<const float*>(src)[p] * f, 0.f);
        else { const float2 s = static_cast<const float2*>(src)[p]; v = make_float2(s.x * f, s.y * f); }
    }
    grid[(size_t)n * G + g] = v;
}

// q[n][p] = (cy cx) grid[n][window] (+ mu[n] pv[n][p] when pv != nullptr); partial[n, chunk, 0] = sum over the chunk of Re(conj(pv) q):
// sense_combine_kernel's epilogue, with the same pixel ranges and the same fixed tree
__global__ __launch_bounds__(kNcThreads) void nufft_crop_kernel(const float2* __restrict__ grid, const float* __restrict__ cy,
                                                                const float* __restrict__ cx, const float2* __restrict__ pv,
                                                                const float* __restrict__ mu, const float* __restrict__ tact,
                                                                float2* __restrict__ q, double* __restrict__ partial, int H, int W, int gh, int gw) {
    __shared__ double red[kNcThreads / 64];
    const int n = blockIdx.y, HW = H * W;
    if (stopped(tact, n)) return;
    const int p0 = blockIdx.x * kPixelChunk + threadIdx.x;
    const size_t base = (size_t)n * HW, gbase = (size_t)n * gh * gw;
    const int oy = gh / 2 - H / 2, ox = gw / 2 - W / 2;
    const float m = (pv != nullptr && mu != nullptr) ? mu[n] : 0.f;
    double dot[1] = {0.0};
#pragma unroll
    for (int j = 0; j < kNcPer; ++j) {
        const int p = p0 + j * kNcThreads;
        if (p < HW) {
            const int iy = p / W, ix = p - iy * W;
            const float2 g = grid[gbase + (size_t)(iy + oy) * gw + (ix + ox)];
            const float f = cy[iy] * cx[ix];
            float2 o = make_float2(g.x * f, g.y * f);
            if (pv != nullptr) {
                const float2 pp = pv[base + p];
                o.x += m * pp.x; o.y += m * pp.y;
                dot[0] += (double)pp.x * (double)o.x + (double)pp.y * (double)o.y;
            }
            q[base + p] = o;
        }
    }
    if (partial == nullptr) return;                        // (uniform)
    block_sums_fixed<kNcThreads, 1>(dot, red);
    if (threadIdx.x == 0) partial[((size_t)n * gridDim.x + blockIdx.x) * 2] = dot[0];
}

__device__ __forceinline__ int wrap(int i, int g) { return i < 0 ? i + g : (i >= g ? i - g : i); }   // i in (-g, 2 g)

// out[n][m] = sum_iy wy[iy] (sum_ix wx[ix] grid[n][(i0y + iy) mod gh][(i0x + ix) mod gw]), both sums ascending fma chains from +0.
// A wave's 64 samples are consecutive in m: neighbours along a readout, whose footprints overlap on the grid.
template <int J>
__global__ __launch_bounds__(kNcThreads) void nufft_interp_kernel(const float2* __restrict__ grid, const int* __restrict__ i0,
                                                                  const float* __restrict__ wts, float2* __restrict__ out, int M, int gh, int gw) {
    const int n = blockIdx.y;
    const int m = blockIdx.x * kNcThreads + threadIdx.x;
    if (m >= M) return;
    const float2* gp = grid + (size_t)n * gh * gw;
    const int y0 = i0[m], x0 = i0[(size_t)M + m];
    float wx[J];
    int col[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        wx[j] = wts[(size_t)(J + j) * M + m];
        col[j] = wrap(x0 + j, gw);
    }
    float2 acc = make_float2(0.f, 0.f);
#pragma unroll
    for (int iy = 0; iy < J; ++iy) {
        const float2* row = gp + (size_t)wrap(y0 + iy, gh) * gw;
        float2 t = make_float2(0.f, 0.f);
#pragma unroll
        for (int ix = 0; ix < J; ++ix) {
            const float2 v = row[col[ix]];
            t.x = fmaf(wx[ix], v.x, t.x);
            t.y = fmaf(wx[ix], v.y, t.y);
        }
        const float wy = wts[(size_t)iy * M + m];
        acc.x = fmaf(wy, t.x, acc.x);
        acc.y = fmaf(wy, t.y, acc.y);
    }
    out[(size_t)n * M + m] = acc;
}

// One workgroup per (tile, slice): the header's gridding.  y: [N, M] samples, w: [M] weights or nullptr (1)
template <int J>
__global__ __launch_bounds__(kNcThreads) void nufft_grid_kernel(const float2* __restrict__ y, const float* __restrict__ w, const int* __restrict__ i0,
                                                                const float* __restrict__ wts, const int* __restrict__ bin_off,
                                                                const int* __restrict__ bin_idx, float2* __restrict__ grid, int M, int gh, int gw,
                                                                int tiles_x) {
    __shared__ float2 a_s[kGridChunk][kNufftTile];
    __shared__ float wx_s[kGridChunk][kNufftTile];
    const int tile = blockIdx.x, n = blockIdx.y;
    const int ty0 = (tile / tiles_x) * kNufftTile, tx0 = (tile % tiles_x) * kNufftTile;
    const int tx = threadIdx.x % kNufftTile, ty = threadIdx.x / kNufftTile;
    const int b0 = bin_off[tile], b1 = bin_off[tile + 1];
    const float2* yn = y + (size_t)n * M;
    float2 acc = make_float2(0.f, 0.f);
    for (int c0 = b0; c0 < b1; c0 += kGridChunk) {
        const int cnt = min(kGridChunk, b1 - c0);
        for (int idx = threadIdx.x; idx < cnt * kNufftTile; idx += kNcThreads) {
            const int sl = idx / kNufftTile, j = idx % kNufftTile;
            const int m = bin_idx[c0 + sl];
            const int d = wrap(ty0 + j - i0[m], gh), e = wrap(tx0 + j - i0[(size_t)M + m], gw);
            float2 v = make_float2(0.f, 0.f);
            if (d < J) {
                const float wy = wts[(size_t)d * M + m];
                v = yn[m];
                if (w != nullptr) { const float ww = w[m]; v.x *= ww; v.y *= ww; }
                v.x *= wy; v.y *= wy;
            }
            a_s[sl][j] = v;
            wx_s[sl][j] = e < J ? wts[(size_t)(J + e) * M + m] : 0.f;
        }
        __syncthreads();
        for (int s = 0; s < cnt; ++s) {
            const float2 a = a_s[s][ty];
            const float wx = wx_s[s][tx];
            acc.x = fmaf(a.x, wx, acc.x);
            acc.y = fmaf(a.y, wx, acc.y);
        }
        __syncthreads();
    }
    grid[(size_t)n * gh * gw + (size_t)(ty0 + ty) * gw + (tx0 + tx)] = acc;
}

// partial[n, chunk] = sum over the chunk's samples of w_m |a[n][m] - y[n][m]|^2: float32 differences, squared, weighted and summed in float64
__global__ __launch_bounds__(kNcThreads) void nufft_misfit_kernel(const float2* __restrict__ a, const float2* __restrict__ y,
                                                                  const float* __restrict__ w, double* __restrict__ partial, int M) {
    __shared__ double red[kNcThreads / 64];
    const int n = blockIdx.y;
    const int m0 = blockIdx.x * kPixelChunk + threadIdx.x;
    double acc[1] = {0.0};
#pragma unroll
    for (int j = 0; j < kNcPer; ++j) {
        const int m = m0 + j * kNcThreads;
        if (m < M) {
            const float2 p = a[(size_t)n * M + m], q = y[(size_t)n * M + m];
            const float dx = p.x - q.x, dy = p.y - q.y;
            const double t = (double)dx * (double)dx + (double)dy * (double)dy;
            acc[0] += w != nullptr ? (double)w[m] * t : t;
        }
    }
    block_sums_fixed<kNcThreads, 1>(acc, red);
    if (threadIdx.x == 0) partial[(size_t)n * gridDim.x + blockIdx.x] = acc[0];
}

// dc[n][0] = the slice's partials summed in a fixed order, dc[n][1 .. dc_chunks) = 0: the layout residual_reduce_kernel sums (adding exact
// zeros changes no bit)
__global__ __launch_bounds__(kNcThreads) void nufft_misfit_sum_kernel(const double* __restrict__ partial, int chunks, double* __restrict__ dc,
                                                                      int dc_chunks) {
    __shared__ double red[kNcThreads / 64];
    const int n = blockIdx.x;
    double acc[1] = {0.0};
    for (int i = threadIdx.x; i < chunks; i += kNcThreads) acc[0] += partial[(size_t)n * chunks + i];
    block_sums_fixed<kNcThreads, 1>(acc, red);
    for (int i = threadIdx.x; i < dc_chunks; i += kNcThreads)
        if (i > 0) dc[(size_t)n * dc_chunks + i] = 0.0;
    if (threadIdx.x == 0) dc[(size_t)n * dc_chunks] = acc[0];
}

// y[n][m] += sigma (g_re + i g_im): pnp_acquire's counter hash with p = m, streams 9001 / 9003, seed + n; float64, rounded once
__global__ __launch_bounds__(kNcThreads) void nufft_noise_kernel(float2* __restrict__ y, double sigma, unsigned long long seed, int M) {
    const int n = blockIdx.y;
    const int m = blockIdx.x * kNcThreads + threadIdx.x;
    if (m >= M) return;
    const unsigned long long sn = (seed + (unsigned long long)n) * 0x100000001B3ull;
    const unsigned long long bre1 = splitmix64(sn + kNoiseStreamRe), bre2 = splitmix64(sn + kNoiseStreamRe + 1u);
    const unsigned long long bim1 = splitmix64(sn + kNoiseStreamIm), bim2 = splitmix64(sn + kNoiseStreamIm + 1u);
    float2 v = y[(size_t)n * M + m];
    v.x = (float)((double)v.x + gauss64(bre1, bre2, (unsigned long long)m) * sigma);
    v.y = (float)((double)v.y + gauss64(bim1, bim2, (unsigned long long)m) * sigma);
    y[(size_t)n * M + m] = v;
}

}  // namespace

hipError_t launch_nufft_pad(const float2* src, const float* src_real, const NufftDev& P, float2* grid, int batch, hipStream_t s) {
    const dim3 g((unsigned)((P.gh * P.gw + kNcThreads - 1) / kNcThreads), (unsigned)batch);
    if (src_real != nullptr)
        hipLaunchKernelGGL(nufft_pad_kernel<true>, g, dim3(kNcThreads), 0, s, (const void*)src_real, P.cy, P.cx, grid, P.h, P.w, P.gh, P.gw);
    else
        hipLaunchKernelGGL(nufft_pad_kernel<false>, g, dim3(kNcThreads), 0, s, (const void*)src, P.cy, P.cx, grid, P.h, P.w, P.gh, P.gw);
    return hipGetLastError();
}

hipError_t launch_nufft_crop(const float2* grid, const NufftDev& P, const float2* pv, const float* mu, const float* tact, float2* q, double* partial,
                             int batch, hipStream_t s) {
    hipLaunchKernelGGL(nufft_crop_kernel, dim3((unsigned)pixel_chunks(P.h, P.w), (unsigned)batch), dim3(kNcThreads), 0, s, grid, P.cy, P.cx, pv, mu,
                       tact, q, partial, P.h, P.w, P.gh, P.gw);
    return hipGetLastError();
}

hipError_t launch_nufft_interp(const float2* grid, const NufftDev& P, float2* out, int batch, hipStream_t s) {
    const dim3 g((unsigned)((P.m + kNcThreads - 1) / kNcThreads), (unsigned)batch);
#define PNP_NC_INTERP(J_) hipLaunchKernelGGL(nufft_interp_kernel<J_>, g, dim3(kNcThreads), 0, s, grid, P.i0, P.wts, out, (int)P.m, P.gh, P.gw)
    if (P.width == 4) PNP_NC_INTERP(4);
    else if (P.width == 6) PNP_NC_INTERP(6);
    else PNP_NC_INTERP(8);
#undef PNP_NC_INTERP
    return hipGetLastError();
}

hipError_t launch_nufft_grid(const float2* y, const float* w, const NufftDev& P, float2* grid, int batch, hipStream_t s) {
    const dim3 g((unsigned)(P.tiles_y * P.tiles_x), (unsigned)batch);
#define PNP_NC_GRID(J_) \
    hipLaunchKernelGGL(nufft_grid_kernel<J_>, g, dim3(kNcThreads), 0, s, y, w, P.i0, P.wts, P.bin_off, P.bin_idx, grid, (int)P.m, P.gh, P.gw, P.tiles_x)
    if (P.width == 4) PNP_NC_GRID(4);
    else if (P.width == 6) PNP_NC_GRID(6);
    else PNP_NC_GRID(8);
#undef PNP_NC_GRID
    return hipGetLastError();
}

int nufft_sample_chunks(int64_t m) { return (int)((m + kPixelChunk - 1) / kPixelChunk); }

hipError_t launch_nufft_misfit(const float2* a, const float2* y, const float* w, const NufftDev& P, double* partial, double* dcpartial, int N,
                               hipStream_t s) {
    const int chunks = nufft_sample_chunks(P.m);
    hipLaunchKernelGGL(nufft_misfit_kernel, dim3((unsigned)chunks, (unsigned)N), dim3(kNcThreads), 0, s, a, y, w, partial, (int)P.m);
    hipLaunchKernelGGL(nufft_misfit_sum_kernel, dim3((unsigned)N), dim3(kNcThreads), 0, s, (const double*)partial, chunks, dcpartial,
                       pixel_chunks(P.h, P.w));
    return hipGetLastError();
}

hipError_t launch_nufft_noise(float2* y, double sigma, uint64_t seed, const NufftDev& P, int N, hipStream_t s) {
    const dim3 g((unsigned)((P.m + kNcThreads - 1) / kNcThreads), (unsigned)N);
    hipLaunchKernelGGL(nufft_noise_kernel, g, dim3(kNcThreads), 0, s, y, sigma, (unsigned long long)seed, (int)P.m);
    return hipGetLastError();
}

}  // namespace pnp
