// Isotropic total-variation denoiser by Chambolle's dual projection (pnp_tv_denoise, and the x-update of pnp_step under PNP_PRIOR_TV).
//
// THE FLOAT32 EXPRESSION ORDER (tests/tv_ref.py restates it; every kernel of this unit evaluates exactly this, through the one set of
// device functions below, so the bits depend neither on the tile plan nor on which kernel ran).  Every operation is one IEEE float32
// operation; the unit is compiled with floating-point contraction OFF (the pragma below), so a product and a sum are fused only where fmaf
// is written (fma = ONE rounding); the divisions and the square root are the correctly rounded ones.  Per slice:
//     lam = scale * lam_in[n]                      (a product; scale = 1 for pnp_tv_denoise, float32(tv_scale) for pnp_step)
//     not (lam > 0):  out = min(max(v, 0), 1)      (lam = 0, and a negative or NaN weight too)
//     rl  = 1 / lam                                (one IEEE reciprocal per slice)
//     py = px = 0 on every pixel; p outside the image reads as 0
//     K times, every pixel from the p of the iteration before (Jacobi):
//         d(i,j)  = ((py[i,j] - py[i-1,j]) + (px[i,j] - px[i,j-1])) - v[i,j] * rl          (the product rounded, then the difference)
//         gy      = i < H-1 ? d(i+1,j) - d(i,j) : 0 ;    gx = j < W-1 ? d(i,j+1) - d(i,j) : 0
//         s       = fma(gx, gx, gy * gy)            (gy * gy rounded, gx * gx contracted)
//         den     = fma(tau, sqrt(s), 1)            (tau = 1/8; IEEE square root)
//         r       = 1 / den                         (IEEE reciprocal)
//         py[i,j] = fma(tau, gy, py[i,j]) * r ;     px[i,j] = fma(tau, gx, px[i,j]) * r
//     out = min(max(fma(-lam, (py[i,j] - py[i-1,j]) + (px[i,j] - px[i,j-1]), v[i,j]), 0), 1)
// py of the last row and px of the last column stay 0 (their gradient is 0), so the differences above ARE the negative adjoint with its end
// cases.  On a constant image d is constant, gy = gx = 0 exactly, p stays 0 and out = clamp(v) bit for bit.  No atomics, no reductions.
// v = the float32 plane of pnp_tv_denoise, or Re z - Re u (one float32 subtraction) read from the two complex planes of pnp_step.
//
// THE FUSED KERNEL.  One workgroup of 32 x 32 threads owns a 128 x 128 REGION of a slice; every thread keeps a 4 x 4 patch of v, py, px in
// registers.  An iteration has dependency radius 1, so after t iterations the p of the region is right everywhere but in a band of t pixels
// along the region's edge; the closing divergence reads one pixel up and left.  With kTvT = 10 iterations per launch the workgroup's TILE
// (what it stores) is the region minus 11 pixels on the top / left and 10 on the bottom / right: 107 x 107, redundant-compute factor
// (128 / 107)^2 = 1.43.  Only a patch's rim crosses threads: py of its bottom row, px of its right column (read by the patches below / right
// for d), d of its top row and left column (read by the patches above / left for the gradient) - four float4 per thread, 64 KiB of LDS
// per workgroup, two barriers per iteration.  Pixels of the region outside the image hold v = 0 and p = 0, and the gradient is forced to 0 on
// the image's last row / column: the Neumann ends exactly, not zero padding.  K > kTvT runs ceil(K / kTvT) launches that hand p over
// through a (py, px) plane in device memory, ping-pong between two planes (a launch reads the halo of its neighbours' tiles).
// THE NAIVE FORM (PNP_TV_NAIVE=1): one launch per iteration, one thread per pixel, p read from one plane and written to the other, then
// tv_close_kernel; it is the bit-for-bit check of the fused kernel and its timing baseline.  tv_close_kernel also ends the fused path when
// out aliases the input plane (the last fused launch then stores p instead of out, as no launch may write what a neighbour still reads).
#include "pnp_internal.h"

#pragma clang fp contract(off)

namespace pnp {

namespace {

constexpr float kTau = 0.125f;

__device__ __forceinline__ float tv_d(float py, float pyu, float px, float pxl, float v, float rl) {
    return ((py - pyu) + (px - pxl)) - v * rl;
}

// one pixel's dual update from the gradient of d; gy / gx already forced to 0 on the last row / column
__device__ __forceinline__ void tv_update(float gy, float gx, float& py, float& px) {
    const float s = fmaf(gx, gx, gy * gy);
    const float den = fmaf(kTau, sqrtf(s), 1.0f);
    const float r = 1.0f / den;
    py = fmaf(kTau, gy, py) * r;
    px = fmaf(kTau, gx, px) * r;
}

__device__ __forceinline__ float tv_out(float py, float pyu, float px, float pxl, float v, float lam) {
    const float dv = (py - pyu) + (px - pxl);
    return fminf(fmaxf(fmaf(-lam, dv, v), 0.0f), 1.0f);
}

__device__ __forceinline__ float tv_clamp(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

template <bool ZU>
__device__ __forceinline__ float tv_load(const TvArgs& a, size_t idx) {
    if (ZU) return a.z[idx].x - a.u[idx].x;
    return a.v[idx];
}

constexpr int kP = 4;                            // patch side per thread
constexpr int kB = kTvRegion / kP;               // threads per side of the workgroup: 32
static_assert(kB * kP == kTvRegion && kTvTile == kTvRegion - 2 * kTvT - 1 && kTvTile > 0, "tile plan");

template <bool ZU>
__global__ __launch_bounds__(kB * kB) void tv_fused_kernel(TvArgs a) {
    __shared__ float4 s_pyb[kB][kB];   // py of the patch's bottom row, by column
    __shared__ float4 s_pxr[kB][kB];   // px of the patch's right column, by row
    __shared__ float4 s_dt[kB][kB];    // d of the patch's top row
    __shared__ float4 s_dl[kB][kB];    // d of the patch's left column
    const int tiles = a.tiles_x * a.tiles_y;
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    if (a.tact && a.tact[n] > 0.5f) return;                       // a stopped slice keeps x
    const int tby = tile / a.tiles_x, tbx = tile - tby * a.tiles_x;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int H = a.H, W = a.W;
    const int gi0 = tby * kTvTile - (kTvT + 1) + ty * kP, gj0 = tbx * kTvTile - (kTvT + 1) + tx * kP;   // the patch's first pixel in the image
    const float lam = a.scale * a.lam[n];
    const size_t base = (size_t)n * H * W;

    float v[kP][kP], py[kP][kP], px[kP][kP];
    bool rin[kP], cin[kP], rtile[kP], ctile[kP];
#pragma unroll
    for (int r = 0; r < kP; ++r) {
        const int lr = ty * kP + r, lc = tx * kP + r;
        rin[r] = gi0 + r >= 0 && gi0 + r < H;
        cin[r] = gj0 + r >= 0 && gj0 + r < W;
        rtile[r] = rin[r] && lr >= kTvT + 1 && lr < kTvRegion - kTvT;
        ctile[r] = cin[r] && lc >= kTvT + 1 && lc < kTvRegion - kTvT;
    }
    const bool plain = !(lam > 0.0f);
#pragma unroll
    for (int r = 0; r < kP; ++r)
#pragma unroll
        for (int c = 0; c < kP; ++c) {
            const bool in = rin[r] && cin[c];
            const size_t idx = base + (size_t)(in ? gi0 + r : 0) * W + (in ? gj0 + c : 0);
            v[r][c] = in ? tv_load<ZU>(a, idx) : 0.0f;
            float2 p = make_float2(0.0f, 0.0f);
            if (in && a.p_in && !plain) p = a.p_in[idx];
            py[r][c] = p.x; px[r][c] = p.y;
        }
    if (plain) {                                                 // lam = 0: the clamp alone (uniform over the workgroup)
        if (a.out)
#pragma unroll
            for (int r = 0; r < kP; ++r)
#pragma unroll
                for (int c = 0; c < kP; ++c)
                    if (rtile[r] && ctile[c]) a.out[base + (size_t)(gi0 + r) * W + gj0 + c] = tv_clamp(v[r][c]);
        return;
    }
    const float rl = 1.0f / lam;
    const int rlast = H - 1 - gi0, clast = W - 1 - gj0;          // patch row / column of the image's last one (outside 0..3: not in this patch)

    s_pyb[ty][tx] = make_float4(py[kP - 1][0], py[kP - 1][1], py[kP - 1][2], py[kP - 1][3]);
    s_pxr[ty][tx] = make_float4(px[0][kP - 1], px[1][kP - 1], px[2][kP - 1], px[3][kP - 1]);
    __syncthreads();
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int it = 0; it < a.iters; ++it) {
        float d[kP][kP];
        {
            const float4 up4 = ty > 0 ? s_pyb[ty - 1][tx] : zero4;
            const float4 lf4 = tx > 0 ? s_pxr[ty][tx - 1] : zero4;
            const float up[kP] = {up4.x, up4.y, up4.z, up4.w}, lf[kP] = {lf4.x, lf4.y, lf4.z, lf4.w};
#pragma unroll
            for (int r = 0; r < kP; ++r)
#pragma unroll
                for (int c = 0; c < kP; ++c)
                    d[r][c] = tv_d(py[r][c], r > 0 ? py[r - 1][c] : up[c], px[r][c], c > 0 ? px[r][c - 1] : lf[r], v[r][c], rl);
        }
        s_dt[ty][tx] = make_float4(d[0][0], d[0][1], d[0][2], d[0][3]);
        s_dl[ty][tx] = make_float4(d[0][0], d[1][0], d[2][0], d[3][0]);
        __syncthreads();
        {
            const float4 dn4 = ty < kB - 1 ? s_dt[ty + 1][tx] : zero4;     // (the region's last row / column is inside the band that is dropped)
            const float4 rt4 = tx < kB - 1 ? s_dl[ty][tx + 1] : zero4;
            const float dn[kP] = {dn4.x, dn4.y, dn4.z, dn4.w}, rt[kP] = {rt4.x, rt4.y, rt4.z, rt4.w};
#pragma unroll
            for (int r = 0; r < kP; ++r)
#pragma unroll
                for (int c = 0; c < kP; ++c) {
                    const float gy = r == rlast ? 0.0f : (r < kP - 1 ? d[r + 1][c] : dn[c]) - d[r][c];
                    const float gx = c == clast ? 0.0f : (c < kP - 1 ? d[r][c + 1] : rt[r]) - d[r][c];
                    tv_update(gy, gx, py[r][c], px[r][c]);
                    if (!(rin[r] && cin[c])) { py[r][c] = 0.0f; px[r][c] = 0.0f; }
                }
        }
        s_pyb[ty][tx] = make_float4(py[kP - 1][0], py[kP - 1][1], py[kP - 1][2], py[kP - 1][3]);
        s_pxr[ty][tx] = make_float4(px[0][kP - 1], px[1][kP - 1], px[2][kP - 1], px[3][kP - 1]);
        __syncthreads();
    }
    if (a.p_out) {
#pragma unroll
        for (int r = 0; r < kP; ++r)
#pragma unroll
            for (int c = 0; c < kP; ++c)
                if (rtile[r] && ctile[c]) a.p_out[base + (size_t)(gi0 + r) * W + gj0 + c] = make_float2(py[r][c], px[r][c]);
    }
    if (a.out) {
        const float4 up4 = ty > 0 ? s_pyb[ty - 1][tx] : zero4;
        const float4 lf4 = tx > 0 ? s_pxr[ty][tx - 1] : zero4;
        const float up[kP] = {up4.x, up4.y, up4.z, up4.w}, lf[kP] = {lf4.x, lf4.y, lf4.z, lf4.w};
#pragma unroll
        for (int r = 0; r < kP; ++r)
#pragma unroll
            for (int c = 0; c < kP; ++c)
                if (rtile[r] && ctile[c])
                    a.out[base + (size_t)(gi0 + r) * W + gj0 + c] =
                        tv_out(py[r][c], r > 0 ? py[r - 1][c] : up[c], px[r][c], c > 0 ? px[r][c - 1] : lf[r], v[r][c], lam);
    }
}

// ---- the naive form: one iteration per launch, one thread per pixel ------------------------------------------------------------------
constexpr int kPix = 256;

template <bool ZU>
__device__ __forceinline__ float tv_d_at(const TvArgs& a, size_t base, int i, int j, float rl) {
    const int W = a.W;
    const size_t idx = base + (size_t)i * W + j;
    float2 p = make_float2(0.0f, 0.0f), pu = p, pl = p;
    if (a.p_in) {
        p = a.p_in[idx];
        if (i > 0) pu = a.p_in[idx - W];
        if (j > 0) pl = a.p_in[idx - 1];
    }
    return tv_d(p.x, pu.x, p.y, pl.y, tv_load<ZU>(a, idx), rl);
}

template <bool ZU>
__global__ __launch_bounds__(kPix) void tv_iter_kernel(TvArgs a) {
    const int chunks = a.tiles_x;                                 // workgroups per slice
    const int n = blockIdx.x / chunks;
    if (a.tact && a.tact[n] > 0.5f) return;
    const int q = (blockIdx.x - n * chunks) * kPix + threadIdx.x;
    const int H = a.H, W = a.W;
    if (q >= H * W) return;
    const float lam = a.scale * a.lam[n];
    if (!(lam > 0.0f)) return;
    const float rl = 1.0f / lam;
    const int i = q / W, j = q - i * W;
    const size_t base = (size_t)n * H * W;
    const float d = tv_d_at<ZU>(a, base, i, j, rl);
    const float gy = i < H - 1 ? tv_d_at<ZU>(a, base, i + 1, j, rl) - d : 0.0f;
    const float gx = j < W - 1 ? tv_d_at<ZU>(a, base, i, j + 1, rl) - d : 0.0f;
    float2 p = a.p_in ? a.p_in[base + q] : make_float2(0.0f, 0.0f);
    tv_update(gy, gx, p.x, p.y);
    a.p_out[base + q] = p;
}

template <bool ZU>
__global__ __launch_bounds__(kPix) void tv_close_kernel(TvArgs a) {
    const int chunks = a.tiles_x;
    const int n = blockIdx.x / chunks;
    if (a.tact && a.tact[n] > 0.5f) return;
    const int q = (blockIdx.x - n * chunks) * kPix + threadIdx.x;
    const int H = a.H, W = a.W;
    if (q >= H * W) return;
    const float lam = a.scale * a.lam[n];
    const size_t idx = (size_t)n * H * W + q;
    const float v = tv_load<ZU>(a, idx);                          // (out may alias v: this thread's own pixel only)
    if (!(lam > 0.0f)) { a.out[idx] = tv_clamp(v); return; }
    const int i = q / W, j = q - i * W;
    const float2 p = a.p_in[idx];
    const float pyu = i > 0 ? a.p_in[idx - W].x : 0.0f, pxl = j > 0 ? a.p_in[idx - 1].y : 0.0f;
    a.out[idx] = tv_out(p.x, pyu, p.y, pxl, v, lam);
}

}  // namespace

hipError_t launch_tv_fused(TvArgs a, int N, hipStream_t s) {
    a.tiles_x = (a.W + kTvTile - 1) / kTvTile;
    a.tiles_y = (a.H + kTvTile - 1) / kTvTile;
    const dim3 grid((unsigned)((size_t)N * a.tiles_x * a.tiles_y)), block(kB, kB);
    if (a.z) hipLaunchKernelGGL(tv_fused_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(tv_fused_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tv_iter(TvArgs a, int N, hipStream_t s) {
    a.tiles_x = (a.H * a.W + kPix - 1) / kPix;
    a.tiles_y = 1;
    const dim3 grid((unsigned)((size_t)N * a.tiles_x)), block(kPix);
    if (a.z) hipLaunchKernelGGL(tv_iter_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(tv_iter_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tv_close(TvArgs a, int N, hipStream_t s) {
    a.tiles_x = (a.H * a.W + kPix - 1) / kPix;
    a.tiles_y = 1;
    const dim3 grid((unsigned)((size_t)N * a.tiles_x)), block(kPix);
    if (a.z) hipLaunchKernelGGL(tv_close_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(tv_close_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace pnp
