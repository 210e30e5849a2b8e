// The B0 field map from two echo images by the regularised fit of include/pnpadmm_fieldmap.h (pnp_fieldmap_estimate, pnp_fieldmap_cost).
//
// THE FLOAT32 EXPRESSION ORDER is the header's, word for word (tests/fieldmap_ref.py restates it): every kernel of this unit evaluates it
// through the one set of device functions below, so the bits depend neither on the tile plan nor on which kernel ran.  The unit is compiled
// with floating-point contraction OFF (the pragma below): a product and a sum are fused only where fmaf is written.
//
//   fm_prepare_kernel   grid (pixel_chunks, N): phi, m (into the w plane) and theta^0 = phi of kPixelChunk pixels; the workgroup's maximum of m
//   fm_weights_kernel   grid (pixel_chunks, N): the slice's maximum from the workgroup maxima (any order gives the same maximum), then w and rd
//   fm_fused_kernel     a.iters <= kFmT sweeps on a register-resident kFmRegion^2 region, of which the kFmTile^2 tile is stored (the header's
//                       THE FUSED KERNEL; the structure of tv_fused_kernel)
//   fm_sweep_kernel     the naive form: ONE sweep, one thread per pixel
//   fm_finish_kernel    omega = float32((double)theta / dte)
//   fm_cost_kernel      grid (pixel_chunks, N): the float64 terms of Psi of kPixelChunk pixels, summed by block_reduce.h's fixed tree
//   fm_cost_sum_kernel  grid (N): the slice's chunk sums, ascending
// No atomics, no cross-workgroup waits: a launch ends, the next starts.
#include "pnp_internal.h"
#include "block_reduce.h"

#pragma clang fp contract(off)

namespace pnp {

namespace {

constexpr int kFmThreads = 256;
constexpr int kFmPer = kPixelChunk / kFmThreads;   // pixels per thread of the chunked kernels

// one pixel of a sweep; an absent neighbour is passed as t itself
__device__ __forceinline__ float fm_update(float t, float up, float dn, float lf, float rt, float phi, float w, float rd, float beta) {
    const float sn = sinf(t - phi);
    const float lap = ((t - up) + (t - dn)) + ((t - lf) + (t - rt));
    const float g = fmaf(beta, lap, w * sn);
    return fmaf(-g, rd, t);
}

__global__ __launch_bounds__(kFmThreads) void fm_prepare_kernel(FmArgs a) {
    __shared__ float red[kFmThreads / 64];
    const int n = blockIdx.y, HW = a.H * a.W;
    const size_t plane = (size_t)n * HW;
    float mx = 0.0f;
    for (int k = 0; k < kFmPer; ++k) {
        const int q = blockIdx.x * kPixelChunk + k * kFmThreads + threadIdx.x;
        if (q >= HW) break;
        float sx = 0.0f, sy = 0.0f;
        for (int c = 0; c < a.C; ++c) {
            const size_t idx = ((size_t)n * a.C + c) * HW + q;
            const float2 u = a.x1[idx], v = a.x2[idx];
            sx = fmaf(u.x, v.x, sx);
            sx = fmaf(u.y, v.y, sx);
            sy = fmaf(u.y, v.x, sy);
            sy = fmaf(-u.x, v.y, sy);
        }
        const float m = sqrtf(fmaf(sx, sx, sy * sy));
        const float phi = (float)atan2((double)sy, (double)sx);
        a.phi[plane + q] = phi;
        a.w[plane + q] = m;
        a.th_out[plane + q] = phi;
        mx = fmaxf(mx, m);
    }
    mx = block_max_fixed<kFmThreads>(mx, red);
    if (threadIdx.x == 0) a.maxpart[(size_t)n * gridDim.x + blockIdx.x] = mx;
}

__global__ __launch_bounds__(kFmThreads) void fm_weights_kernel(FmArgs a) {
    __shared__ float red[kFmThreads / 64];
    __shared__ float s_ri;
    const int n = blockIdx.y, HW = a.H * a.W, chunks = gridDim.x;
    const size_t plane = (size_t)n * HW;
    float mx = 0.0f;
    for (int i = threadIdx.x; i < chunks; i += kFmThreads) mx = fmaxf(mx, a.maxpart[(size_t)n * chunks + i]);
    mx = block_max_fixed<kFmThreads>(mx, red);
    if (threadIdx.x == 0) s_ri = mx > 0.0f ? 1.0f / mx : 0.0f;
    __syncthreads();
    const float ri = s_ri, b2 = 2.0f * a.beta;
    for (int k = 0; k < kFmPer; ++k) {
        const int q = blockIdx.x * kPixelChunk + k * kFmThreads + threadIdx.x;
        if (q >= HW) break;
        const int i = q / a.W, j = q - i * a.W;
        const float nn = (float)((i > 0) + (i < a.H - 1) + (j > 0) + (j < a.W - 1));
        const float w = a.w[plane + q] * ri;
        a.w[plane + q] = w;
        a.rd[plane + q] = 1.0f / fmaf(b2, nn, w);
        if (a.weight) a.weight[plane + q] = w;
    }
}

// ---- the fused kernel -------------------------------------------------------------------------------------------------------------------
constexpr int kP = 4;                            // patch side per thread
constexpr int kB = kFmRegion / kP;               // threads per side of the workgroup: 32
static_assert(kB * kP == kFmRegion && kFmTile == kFmRegion - 2 * kFmT && kFmTile > 0, "tile plan");

__global__ __launch_bounds__(kB * kB) void fm_fused_kernel(FmArgs a) {
    __shared__ float4 s_bot[kB][kB];   // theta of the patch's bottom row, by column
    __shared__ float4 s_top[kB][kB];   // ... its top row
    __shared__ float4 s_rgt[kB][kB];   // ... its right column, by row
    __shared__ float4 s_lft[kB][kB];   // ... its left column
    const int tiles = a.tiles_x * a.tiles_y;
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    const int tby = tile / a.tiles_x, tbx = tile - tby * a.tiles_x;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int H = a.H, W = a.W;
    const int gi0 = tby * kFmTile - kFmT + ty * kP, gj0 = tbx * kFmTile - kFmT + tx * kP;   // the patch's first pixel in the image
    const size_t base = (size_t)n * H * W;
    const float beta = a.beta;

    float t[kP][kP], phi[kP][kP], w[kP][kP], rd[kP][kP];
    bool rin[kP], cin[kP], rtile[kP], ctile[kP];
#pragma unroll
    for (int r = 0; r < kP; ++r) {
        const int lr = ty * kP + r, lc = tx * kP + r;
        rin[r] = gi0 + r >= 0 && gi0 + r < H;
        cin[r] = gj0 + r >= 0 && gj0 + r < W;
        rtile[r] = rin[r] && lr >= kFmT && lr < kFmRegion - kFmT;
        ctile[r] = cin[r] && lc >= kFmT && lc < kFmRegion - kFmT;
    }
#pragma unroll
    for (int r = 0; r < kP; ++r)
#pragma unroll
        for (int c = 0; c < kP; ++c) {
            const bool in = rin[r] && cin[c];
            const size_t idx = base + (size_t)(in ? gi0 + r : 0) * W + (in ? gj0 + c : 0);
            t[r][c] = in ? a.th_in[idx] : 0.0f;
            phi[r][c] = in ? a.phi[idx] : 0.0f;
            w[r][c] = in ? a.w[idx] : 0.0f;
            rd[r][c] = in ? a.rd[idx] : 0.0f;
        }
    // patch row / column of the image's first and last one (outside 0..3: not in this patch): their outer neighbour is absent
    const int rfirst = -gi0, rlast = H - 1 - gi0, cfirst = -gj0, clast = W - 1 - gj0;

    for (int it = 0; it < a.iters; ++it) {
        s_bot[ty][tx] = make_float4(t[kP - 1][0], t[kP - 1][1], t[kP - 1][2], t[kP - 1][3]);
        s_top[ty][tx] = make_float4(t[0][0], t[0][1], t[0][2], t[0][3]);
        s_rgt[ty][tx] = make_float4(t[0][kP - 1], t[1][kP - 1], t[2][kP - 1], t[3][kP - 1]);
        s_lft[ty][tx] = make_float4(t[0][0], t[1][0], t[2][0], t[3][0]);
        __syncthreads();
        // the region's own edge reads itself: it lies in the band that is dropped
        const float4 up4 = s_bot[ty > 0 ? ty - 1 : ty][tx], dn4 = s_top[ty < kB - 1 ? ty + 1 : ty][tx];
        const float4 lf4 = s_rgt[ty][tx > 0 ? tx - 1 : tx], rt4 = s_lft[ty][tx < kB - 1 ? tx + 1 : tx];
        __syncthreads();
        const float up[kP] = {up4.x, up4.y, up4.z, up4.w}, dn[kP] = {dn4.x, dn4.y, dn4.z, dn4.w};
        const float lf[kP] = {lf4.x, lf4.y, lf4.z, lf4.w}, rt[kP] = {rt4.x, rt4.y, rt4.z, rt4.w};
        float nt[kP][kP];
#pragma unroll
        for (int r = 0; r < kP; ++r)
#pragma unroll
            for (int c = 0; c < kP; ++c) {
                const float tc = t[r][c];
                const float u = r == rfirst ? tc : (r > 0 ? t[r - 1][c] : up[c]);
                const float d = r == rlast ? tc : (r < kP - 1 ? t[r + 1][c] : dn[c]);
                const float l = c == cfirst ? tc : (c > 0 ? t[r][c - 1] : lf[r]);
                const float g = c == clast ? tc : (c < kP - 1 ? t[r][c + 1] : rt[r]);
                nt[r][c] = rin[r] && cin[c] ? fm_update(tc, u, d, l, g, phi[r][c], w[r][c], rd[r][c], beta) : 0.0f;
            }
#pragma unroll
        for (int r = 0; r < kP; ++r)
#pragma unroll
            for (int c = 0; c < kP; ++c) t[r][c] = nt[r][c];
    }
#pragma unroll
    for (int r = 0; r < kP; ++r)
#pragma unroll
        for (int c = 0; c < kP; ++c)
            if (rtile[r] && ctile[c]) a.th_out[base + (size_t)(gi0 + r) * W + gj0 + c] = t[r][c];
}

// ---- the naive form: one sweep per launch, one thread per pixel ---------------------------------------------------------------------------
__global__ __launch_bounds__(kFmThreads) void fm_sweep_kernel(FmArgs a) {
    const int chunks = a.tiles_x;                                 // workgroups per slice
    const int n = blockIdx.x / chunks;
    const int q = (blockIdx.x - n * chunks) * kFmThreads + threadIdx.x;
    const int H = a.H, W = a.W;
    if (q >= H * W) return;
    const int i = q / W, j = q - i * W;
    const size_t idx = (size_t)n * H * W + q;
    const float t = a.th_in[idx];
    const float up = i > 0 ? a.th_in[idx - W] : t, dn = i < H - 1 ? a.th_in[idx + W] : t;
    const float lf = j > 0 ? a.th_in[idx - 1] : t, rt = j < W - 1 ? a.th_in[idx + 1] : t;
    a.th_out[idx] = fm_update(t, up, dn, lf, rt, a.phi[idx], a.w[idx], a.rd[idx], a.beta);
}

__global__ __launch_bounds__(kFmThreads) void fm_finish_kernel(FmArgs a) {
    const int chunks = a.tiles_x;
    const int n = blockIdx.x / chunks;
    const int q = (blockIdx.x - n * chunks) * kFmThreads + threadIdx.x;
    if (q >= a.H * a.W) return;
    const size_t idx = (size_t)n * a.H * a.W + q;
    a.omega_out[idx] = (float)((double)a.th_in[idx] / a.dte);
}

// ---- the cost -------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float fm_theta_of(const FmArgs& a, size_t idx) { return (float)((double)a.omega_in[idx] * a.dte); }

__global__ __launch_bounds__(kFmThreads) void fm_cost_kernel(FmArgs a) {
    __shared__ double red[kFmThreads / 64];
    const int n = blockIdx.y, H = a.H, W = a.W, HW = H * W;
    const size_t plane = (size_t)n * HW;
    const double hb = 0.5 * (double)a.beta;
    double acc = 0.0;
    for (int k = 0; k < kFmPer; ++k) {
        const int q = blockIdx.x * kPixelChunk + k * kFmThreads + threadIdx.x;
        if (q >= HW) break;
        const int i = q / W, j = q - i * W;
        const double t = (double)fm_theta_of(a, plane + q);
        const double dr = j < W - 1 ? t - (double)fm_theta_of(a, plane + q + 1) : 0.0;
        const double dd = i < H - 1 ? t - (double)fm_theta_of(a, plane + q + W) : 0.0;
        const double data = (double)a.w[plane + q] * (1.0 - cos(t - (double)a.phi[plane + q]));
        acc += data + hb * (dr * dr + dd * dd);
    }
    const double total = block_sum_fixed<kFmThreads>(acc, red);
    if (threadIdx.x == 0) a.part[(size_t)n * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(64) void fm_cost_sum_kernel(FmArgs a, int chunks) {
    if (threadIdx.x != 0) return;
    const int n = blockIdx.x;
    double t = 0.0;
    for (int i = 0; i < chunks; ++i) t += a.part[(size_t)n * chunks + i];
    a.cost[n] = t;
}

inline dim3 chunk_grid(const FmArgs& a, int N) { return dim3((unsigned)pixel_chunks(a.H, a.W), (unsigned)N); }

}  // namespace

hipError_t launch_fm_prepare(FmArgs a, int N, hipStream_t s) {
    hipLaunchKernelGGL(fm_prepare_kernel, chunk_grid(a, N), dim3(kFmThreads), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fm_weights_kernel, chunk_grid(a, N), dim3(kFmThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fm_fused(FmArgs a, int N, hipStream_t s) {
    a.tiles_x = (a.W + kFmTile - 1) / kFmTile;
    a.tiles_y = (a.H + kFmTile - 1) / kFmTile;
    const dim3 grid((unsigned)((size_t)N * a.tiles_x * a.tiles_y)), block(kB, kB);
    hipLaunchKernelGGL(fm_fused_kernel, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fm_sweep(FmArgs a, int N, hipStream_t s) {
    a.tiles_x = (a.H * a.W + kFmThreads - 1) / kFmThreads;
    hipLaunchKernelGGL(fm_sweep_kernel, dim3((unsigned)((size_t)N * a.tiles_x)), dim3(kFmThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fm_finish(FmArgs a, int N, hipStream_t s) {
    a.tiles_x = (a.H * a.W + kFmThreads - 1) / kFmThreads;
    hipLaunchKernelGGL(fm_finish_kernel, dim3((unsigned)((size_t)N * a.tiles_x)), dim3(kFmThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fm_cost(FmArgs a, int N, hipStream_t s) {
    hipLaunchKernelGGL(fm_cost_kernel, chunk_grid(a, N), dim3(kFmThreads), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fm_cost_sum_kernel, dim3((unsigned)N), dim3(64), 0, s, a, pixel_chunks(a.H, a.W));
    return hipGetLastError();
}

}  // namespace pnp
