// Density compensation for any trajectory (include/pnpadmm_dcf.h): Pipe and Menon's iteration w <- w / (Psi w), Psi = G G^T with G the
// gridding kernel of the handle's NUFFT plan.  One real float64 plane, no transform, no deconvolution.
//
//   per iteration   dcf_spread_kernel   g[r][c] = sum over the samples of the tile's bin, ascending, of (w_m wy) wx          (float64 grid)
//                   dcf_gather_kernel   d_m = sum_iy wy[iy] (sum_ix wx[ix] g[..][..]);  w_m <- w_m / d_m;  max |d - 1| per workgroup
//   finish          dcf_sum_kernel      per-chunk sums of w in the fixed tree
//                   dcf_finish_kernel   out_m = float32(w_m (H W / sum w));  info[k] = the maximum of iteration k's workgroup maxima
//
// The spread is nufft_grid_kernel in float64 on one real plane: a workgroup owns one kNufftTile^2 tile, walks the tile's bin in chunks and
// every thread runs ONE fma chain from +0 in ascending sample index; fma(a, +0, acc) and fma(+0, wx, acc) change nothing, so a grid point's
// value is the chain over the samples whose footprint contains it whatever the tile.  Every grid point is stored on every call.  The gather
// is nufft_interp_kernel's chain order in float64.  No atomics, no launch waits on another workgroup: an iteration is two launches.
// Every expression is written in the header's order and this unit is compiled without contraction.
#include "pnp_internal.h"
#include "block_reduce.h"
#include "nufft_plan.h"

#pragma clang fp contract(off)

namespace pnp {

namespace {

constexpr int kDcfThreads = 256;
constexpr int kDcfChunk = 128;                             // samples staged per pass: 128 x 16 x (8 + 8) B = 32 KiB of LDS
constexpr int kDcfPer = kPixelChunk / kDcfThreads;         // samples per thread of the chunked sum / finish kernels
static_assert(kNufftTile * kNufftTile == kDcfThreads, "a thread per grid point of the tile");
static_assert(kPixelChunk % kDcfThreads == 0, "whole samples per thread");

__device__ __forceinline__ int wrap(int i, int g) { return i < 0 ? i + g : (i >= g ? i - g : i); }   // i in (-g, 2 g)

// The weight of sample m: the float64 iterate, else the caller's float32 start promoted exactly (an entry that is not positive and finite
// reads as 1: the header's rule), else 1
__device__ __forceinline__ double weight_of(const double* __restrict__ w64, const float* __restrict__ w32, int m) {
    if (w64 != nullptr) return w64[m];
    if (w32 == nullptr) return 1.0;
    const float v = w32[m];
    return (v > 0.f && v <= 3.402823466e38f) ? (double)v : 1.0;
}

template <int J>
__global__ __launch_bounds__(kDcfThreads) void dcf_spread_kernel(const double* __restrict__ w64, const float* __restrict__ w32,
                                                                 const int* __restrict__ i0, const float* __restrict__ wts,
                                                                 const int* __restrict__ bin_off, const int* __restrict__ bin_idx,
                                                                 double* __restrict__ grid, int M, int gh, int gw, int tiles_x) {
    __shared__ double a_s[kDcfChunk][kNufftTile];
    __shared__ double wx_s[kDcfChunk][kNufftTile];
    const int tile = blockIdx.x;
    const int ty0 = (tile / tiles_x) * kNufftTile, tx0 = (tile % tiles_x) * kNufftTile;
    const int tx = threadIdx.x % kNufftTile, ty = threadIdx.x / kNufftTile;
    const int b0 = bin_off[tile], b1 = bin_off[tile + 1];
    double acc = 0.0;
    for (int c0 = b0; c0 < b1; c0 += kDcfChunk) {
        const int cnt = min(kDcfChunk, b1 - c0);
        for (int idx = threadIdx.x; idx < cnt * kNufftTile; idx += kDcfThreads) {
            const int sl = idx / kNufftTile, j = idx % kNufftTile;
            const int m = bin_idx[c0 + sl];
            const int d = wrap(ty0 + j - i0[m], gh), e = wrap(tx0 + j - i0[(size_t)M + m], gw);
            a_s[sl][j] = d < J ? weight_of(w64, w32, m) * (double)wts[(size_t)d * M + m] : 0.0;
            wx_s[sl][j] = e < J ? (double)wts[(size_t)(J + e) * M + m] : 0.0;
        }
        __syncthreads();
        for (int s = 0; s < cnt; ++s) acc = fma(a_s[s][ty], wx_s[s][tx], acc);
        __syncthreads();
    }
    grid[(size_t)(ty0 + ty) * gw + (tx0 + tx)] = acc;
}

// d_m = (Psi w)_m.  psi != nullptr: psi[m] = float32(d).  wout != nullptr: wout[m] = w_m / d.  wmax != nullptr: wmax[workgroup] = the
// maximum of |d - 1| over the workgroup's samples (float32 of the float64 value: rounding is monotone, so the maximum of the rounded
// values is the rounded maximum)
template <int J>
__global__ __launch_bounds__(kDcfThreads) void dcf_gather_kernel(const double* __restrict__ grid, const int* __restrict__ i0,
                                                                 const float* __restrict__ wts, const double* __restrict__ w64,
                                                                 const float* __restrict__ w32, double* __restrict__ wout,
                                                                 float* __restrict__ psi, float* __restrict__ wmax, int M, int gh, int gw) {
    __shared__ float red[kDcfThreads / 64];
    const int m = blockIdx.x * kDcfThreads + threadIdx.x;
    float dev = 0.f;
    if (m < M) {
        const int y0 = i0[m], x0 = i0[(size_t)M + m];
        double wx[J];
        int col[J];
#pragma unroll
        for (int j = 0; j < J; ++j) {
            wx[j] = (double)wts[(size_t)(J + j) * M + m];
            col[j] = wrap(x0 + j, gw);
        }
        double acc = 0.0;
#pragma unroll
        for (int iy = 0; iy < J; ++iy) {
            const double* row = grid + (size_t)wrap(y0 + iy, gh) * gw;
            double t = 0.0;
#pragma unroll
            for (int ix = 0; ix < J; ++ix) t = fma(wx[ix], row[col[ix]], t);
            acc = fma((double)wts[(size_t)iy * M + m], t, acc);
        }
        if (psi != nullptr) psi[m] = (float)acc;
        if (wout != nullptr) wout[m] = weight_of(w64, w32, m) / acc;
        dev = (float)fabs(acc - 1.0);
    }
    if (wmax == nullptr) return;                           // (uniform)
    const float v = block_max_fixed<kDcfThreads>(dev, red);
    if (threadIdx.x == 0) wmax[blockIdx.x] = v;
}

// partial[chunk] = the sum of the chunk's w in the fixed tree
__global__ __launch_bounds__(kDcfThreads) void dcf_sum_kernel(const double* __restrict__ w, double* __restrict__ partial, int M) {
    __shared__ double red[kDcfThreads / 64];
    const int m0 = blockIdx.x * kPixelChunk + threadIdx.x;
    double acc[1] = {0.0};
#pragma unroll
    for (int j = 0; j < kDcfPer; ++j) {
        const int m = m0 + j * kDcfThreads;
        if (m < M) acc[0] += w[m];
    }
    block_sums_fixed<kDcfThreads, 1>(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc[0];
}

// Every workgroup sums the partials in the same fixed order (the same bits in each), then scales its own chunk: out = float32(w (hw / sum)).
// Workgroup 0 also reduces the maxima: info[k] = max over the nb workgroup maxima of pass k, k < passes
__global__ __launch_bounds__(kDcfThreads) void dcf_finish_kernel(const double* __restrict__ w, const double* __restrict__ partial, int chunks,
                                                                 double hw, float* __restrict__ out, const float* __restrict__ wmax, int nb,
                                                                 int passes, float* __restrict__ info, int M) {
    __shared__ double red[kDcfThreads / 64];
    __shared__ float fred[kDcfThreads / 64];
    __shared__ double scale_s;
    double acc[1] = {0.0};
    for (int i = threadIdx.x; i < chunks; i += kDcfThreads) acc[0] += partial[i];
    block_sums_fixed<kDcfThreads, 1>(acc, red);
    if (threadIdx.x == 0) scale_s = hw / acc[0];
    __syncthreads();
    const double scale = scale_s;
    const int m0 = blockIdx.x * kPixelChunk + threadIdx.x;
#pragma unroll
    for (int j = 0; j < kDcfPer; ++j) {
        const int m = m0 + j * kDcfThreads;
        if (m < M) out[m] = (float)(w[m] * scale);
    }
    if (blockIdx.x != 0 || info == nullptr) return;        // (uniform)
    for (int k = 0; k < passes; ++k) {
        float v = 0.f;
        for (int i = threadIdx.x; i < nb; i += kDcfThreads) v = fmaxf(v, wmax[(size_t)k * nb + i]);
        __syncthreads();                                   // fred of the pass before has been read
        v = block_max_fixed<kDcfThreads>(v, fred);
        if (threadIdx.x == 0) info[k] = v;
    }
}

}  // namespace

int dcf_gather_blocks(int64_t m) { return (int)((m + kDcfThreads - 1) / kDcfThreads); }
int dcf_sum_chunks(int64_t m) { return (int)((m + kPixelChunk - 1) / kPixelChunk); }

hipError_t launch_dcf_spread(const double* w64, const float* w32, const NufftDev& P, double* grid, hipStream_t s) {
    const dim3 g((unsigned)(P.tiles_y * P.tiles_x));
#define PNP_DCF_SPREAD(J_) \
    hipLaunchKernelGGL(dcf_spread_kernel<J_>, g, dim3(kDcfThreads), 0, s, w64, w32, P.i0, P.wts, P.bin_off, P.bin_idx, grid, (int)P.m, P.gh, P.gw, P.tiles_x)
    if (P.width == 4) PNP_DCF_SPREAD(4);
    else if (P.width == 6) PNP_DCF_SPREAD(6);
    else PNP_DCF_SPREAD(8);
#undef PNP_DCF_SPREAD
    return hipGetLastError();
}

hipError_t launch_dcf_gather(const double* grid, const NufftDev& P, const double* w64, const float* w32, double* wout, float* psi, float* wmax,
                             hipStream_t s) {
    const dim3 g((unsigned)dcf_gather_blocks(P.m));
#define PNP_DCF_GATHER(J_) \
    hipLaunchKernelGGL(dcf_gather_kernel<J_>, g, dim3(kDcfThreads), 0, s, grid, P.i0, P.wts, w64, w32, wout, psi, wmax, (int)P.m, P.gh, P.gw)
    if (P.width == 4) PNP_DCF_GATHER(4);
    else if (P.width == 6) PNP_DCF_GATHER(6);
    else PNP_DCF_GATHER(8);
#undef PNP_DCF_GATHER
    return hipGetLastError();
}

hipError_t launch_dcf_finish(const double* w, double* partial, const NufftDev& P, float* out, const float* wmax, int passes, float* info,
                             hipStream_t s) {
    const int chunks = dcf_sum_chunks(P.m);
    hipLaunchKernelGGL(dcf_sum_kernel, dim3((unsigned)chunks), dim3(kDcfThreads), 0, s, w, partial, (int)P.m);
    hipLaunchKernelGGL(dcf_finish_kernel, dim3((unsigned)chunks), dim3(kDcfThreads), 0, s, w, (const double*)partial, chunks,
                       (double)P.h * (double)P.w, out, wmax, dcf_gather_blocks(P.m), passes, info, (int)P.m);
    return hipGetLastError();
}

}  // namespace pnp
