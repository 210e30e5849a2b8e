// Non-Cartesian SENSE: the coil-batched kernels of the operator A p = [F_nu(S_c . p)]_c and its adjoint (include/pnpadmm_ncsense.h) around the
// engine's centred grid transform.  A BLOCK of cb coils of every slice is in flight at a time: the grids are [N, cb, gh, gw] (plane n cb + j),
// the samples [N, *, M] with the coil stride and offset the caller names.  What one coil costs in nufft_kernels.hip and is the same for every
// coil of a sample - the footprint starts, the 2 J weights, the bin walk - is loaded once per block here.
//
//   forward   ncsense_pad_kernel     grid[n, j] = zero-padded (cy cx) . (S_(c0+j) . p): p read once, cb planes written
//             | rows forward | cols forward (centred), batch N cb |
//             ncsense_interp_kernel  a thread per (slice, sample): starts and weights once, then the J x J double fma chain per coil
//   adjoint   ncsense_grid_kernel    a workgroup per (tile, slice): wy / wx of a chunk of the tile's bin staged once, (w y) per coil beside
//                                    them; every thread forms ((w y) wy) and runs acc_j = fma(., wx, acc_j) for the block's coils
//             | rows inverse | cols inverse (centred), batch N cb |
//             ncsense_crop_kernel    acc += conj(S_(c0+j)) . ((cy cx) . crop(grid[n, j])), the chain carried from block to block through q;
//                                    the last block adds mu p and leaves the partial sums of Re<p, q>
//   naive     (PNP_NCSENSE_NAIVE=1: the bit-for-bit check and the timing baseline)  ncsense_expand_kernel writes the coil images, the
//             single-coil launches of nufft_kernels.hip run at batch N cb, and ncsense_crop_kernel<false> combines the cropped coil images
//
// Every expression is written in the header's order and this unit is compiled without contraction: a product that the header rounds is
// rounded, an fma is one where the header writes one.  Per coil plane the gather and the gridding are nufft_kernels.hip's chains, so a coil's
// bits are those of the single-coil launches on that coil's image or samples; the block size changes no bit (a float32 partial stored and
// reloaded is the same float32).
#include "pnp_internal.h"
#include "block_reduce.h"
#include "noise_hash.h"
#include "nufft_plan.h"

#pragma clang fp contract(off)

namespace pnp {

namespace {

constexpr int kNsThreads = 256;
constexpr int kNsPer = kPixelChunk / kNsThreads;          // pixels (or samples) per thread of the chunked pointwise kernels
static_assert(kPixelChunk % kNsThreads == 0, "whole pixels per thread");
static_assert(kNufftTile * kNufftTile == kNsThreads, "a thread per grid point of the tile");
constexpr int kNsChunk = 128;                              // samples staged per pass: 128 x (2 x 16 x 4 + kNcsenseSub x 8) B = 24 KiB of LDS
static_assert(kNcsenseSub == 8, "the gridding kernel's accumulators and its LDS figure are written for 8 coils");

__device__ __forceinline__ bool stopped(const float* tact, int n) { return tact != nullptr && tact[n] > 0.5f; }
__device__ __forceinline__ int wrap(int i, int g) { return i < 0 ? i + g : (i >= g ? i - g : i); }   // i in (-g, 2 g)
// the maps of slice n: [C, HW] shared (sens_n == 1) or [N, C, HW]
__device__ __forceinline__ const float2* maps_of(const float2* sens, int sens_n, int n, int C, int HW) {
    return sens + (size_t)(sens_n == 1 ? 0 : n) * C * HW;
}

// grid[n cb + j][gy][gx] = inside the centred h x w window ? (cy[iy] cx[ix]) (S_(c0+j) . src[n])[iy][ix] : 0; src complex, or a real image (REAL)
template <bool REAL>
__global__ __launch_bounds__(kNsThreads) void ncsense_pad_kernel(const void* __restrict__ src, const float2* __restrict__ sens, int sens_n, int C,
                                                                 int c0, int cb, const float* __restrict__ cy, const float* __restrict__ cx,
                                                                 float2* __restrict__ grid, int H, int W, int gh, int gw) {
    const int n = blockIdx.y, G = gh * gw, HW = H * W;
    const int g = blockIdx.x * kNsThreads + threadIdx.x;
    if (g >= G) return;
    const int gy = g / gw, gx = g - gy * gw;
    const int iy = gy - (gh / 2 - H / 2), ix = gx - (gw / 2 - W / 2);
    float2* out = grid + (size_t)n * cb * G + g;
    if (!(iy >= 0 && iy < H && ix >= 0 && ix < W)) {
        for (int j = 0; j < cb; ++j) out[(size_t)j * G] = make_float2(0.f, 0.f);
        return;
    }
    const int p = iy * W + ix;
    const float f = cy[iy] * cx[ix];
    const float2* sp = maps_of(sens, sens_n, n, C, HW) + (size_t)c0 * HW + p;
    float2 pv = make_float2(0.f, 0.f);
    if (REAL) pv.x = static_cast<const float*>(src)[(size_t)n * HW + p];
    else pv = static_cast<const float2*>(src)[(size_t)n * HW + p];
    for (int j = 0; j < cb; ++j) {
        const float2 sv = sp[(size_t)j * HW];
        float2 t;
        if (REAL) {
            t = make_float2(sv.x * pv.x, sv.y * pv.x);
        } else {
            const float a = sv.x * pv.x, b = sv.y * pv.y, c = sv.x * pv.y, d = sv.y * pv.x;
            t = make_float2(a - b, c + d);
        }
        out[(size_t)j * G] = make_float2(t.x * f, t.y * f);
    }
}

// The naive form's expand: img[n cb + j][p] = S_(c0+j) . src[n] in the pad kernel's order, as a complex plane [N, cb, h, w] for launch_nufft_pad
template <bool REAL>
__global__ __launch_bounds__(kNsThreads) void ncsense_expand_kernel(const void* __restrict__ src, const float2* __restrict__ sens, int sens_n, int C,
                                                                    int c0, int cb, float2* __restrict__ img, int HW) {
    const int n = blockIdx.y;
    const int p = blockIdx.x * kNsThreads + threadIdx.x;
    if (p >= HW) return;
    const float2* sp = maps_of(sens, sens_n, n, C, HW) + (size_t)c0 * HW + p;
    float2 pv = make_float2(0.f, 0.f);
    if (REAL) pv.x = static_cast<const float*>(src)[(size_t)n * HW + p];
    else pv = static_cast<const float2*>(src)[(size_t)n * HW + p];
    for (int j = 0; j < cb; ++j) {
        const float2 sv = sp[(size_t)j * HW];
        float2 t;
        if (REAL) {
            t = make_float2(sv.x * pv.x, sv.y * pv.x);
        } else {
            const float a = sv.x * pv.x, b = sv.y * pv.y, c = sv.x * pv.y, d = sv.y * pv.x;
            t = make_float2(a - b, c + d);
        }
        img[((size_t)n * cb + j) * HW + p] = t;
    }
}

// out[n][oc0 + j][m] = nufft_interp_kernel's double chain on plane n cb + j, for j < cb; out: [N, ocs, M]
template <int J>
__global__ __launch_bounds__(kNsThreads) void ncsense_interp_kernel(const float2* __restrict__ grid, const int* __restrict__ i0,
                                                                    const float* __restrict__ wts, float2* __restrict__ out, int ocs, int oc0, int cb,
                                                                    int M, int gh, int gw) {
    const int n = blockIdx.y;
    const int m = blockIdx.x * kNsThreads + threadIdx.x;
    if (m >= M) return;
    const size_t G = (size_t)gh * gw;
    const int y0 = i0[m], x0 = i0[(size_t)M + m];
    float wx[J], wy[J];
    int col[J], row[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        wy[j] = wts[(size_t)j * M + m];
        wx[j] = wts[(size_t)(J + j) * M + m];
        row[j] = wrap(y0 + j, gh) * gw;
        col[j] = wrap(x0 + j, gw);
    }
    for (int c = 0; c < cb; ++c) {
        const float2* gp = grid + ((size_t)n * cb + c) * G;
        float2 acc = make_float2(0.f, 0.f);
#pragma unroll
        for (int iy = 0; iy < J; ++iy) {
            const float2* rp = gp + row[iy];
            float2 t = make_float2(0.f, 0.f);
#pragma unroll
            for (int ix = 0; ix < J; ++ix) {
                const float2 v = rp[col[ix]];
                t.x = fmaf(wx[ix], v.x, t.x);
                t.y = fmaf(wx[ix], v.y, t.y);
            }
            acc.x = fmaf(wy[iy], t.x, acc.x);
            acc.y = fmaf(wy[iy], t.y, acc.y);
        }
        out[((size_t)n * ocs + oc0 + c) * M + m] = acc;
    }
}

// One workgroup per (tile, slice, sub-block of kNcsenseSub coils): the header's gridding on the planes n cb + j.  y: [N, ycs, M] samples read
// at the coils yc0 + j, w: [M] weights or nullptr (1).  A coil past the block (j >= cb) is neither staged nor stored; its accumulator idles.
template <int J>
__global__ __launch_bounds__(kNsThreads) void ncsense_grid_kernel(const float2* __restrict__ y, int ycs, int yc0, int cb, const float* __restrict__ w,
                                                                  const int* __restrict__ i0, const float* __restrict__ wts,
                                                                  const int* __restrict__ bin_off, const int* __restrict__ bin_idx,
                                                                  float2* __restrict__ grid, int M, int gh, int gw, int tiles_x) {
    __shared__ float wy_s[kNsChunk][kNufftTile];
    __shared__ float wx_s[kNsChunk][kNufftTile];
    __shared__ float2 v_s[kNsChunk][kNcsenseSub];
    const int tile = blockIdx.x, n = blockIdx.y, j0 = blockIdx.z * kNcsenseSub;
    const int nc = min(kNcsenseSub, cb - j0);              // coils of this sub-block (uniform)
    const int ty0 = (tile / tiles_x) * kNufftTile, tx0 = (tile % tiles_x) * kNufftTile;
    const int tx = threadIdx.x % kNufftTile, ty = threadIdx.x / kNufftTile;
    const int b0 = bin_off[tile], b1 = bin_off[tile + 1];
    const float2* yn = y + ((size_t)n * ycs + yc0 + j0) * M;
    float2 acc[kNcsenseSub];
#pragma unroll
    for (int j = 0; j < kNcsenseSub; ++j) acc[j] = make_float2(0.f, 0.f);
    for (int c0 = b0; c0 < b1; c0 += kNsChunk) {
        const int cnt = min(kNsChunk, b1 - c0);
        for (int idx = threadIdx.x; idx < cnt * kNufftTile; idx += kNsThreads) {
            const int sl = idx / kNufftTile, j = idx % kNufftTile;
            const int m = bin_idx[c0 + sl];
            const int d = wrap(ty0 + j - i0[m], gh), e = wrap(tx0 + j - i0[(size_t)M + m], gw);
            wy_s[sl][j] = d < J ? wts[(size_t)d * M + m] : 0.f;
            wx_s[sl][j] = e < J ? wts[(size_t)(J + e) * M + m] : 0.f;
        }
        for (int idx = threadIdx.x; idx < cnt * nc; idx += kNsThreads) {
            const int sl = idx / nc, j = idx - sl * nc;
            const int m = bin_idx[c0 + sl];
            float2 v = yn[(size_t)j * M + m];
            if (w != nullptr) { const float ww = w[m]; v.x *= ww; v.y *= ww; }
            v_s[sl][j] = v;
        }
        __syncthreads();
        for (int s = 0; s < cnt; ++s) {
            const float wy = wy_s[s][ty];
            const float wx = wx_s[s][tx];
#pragma unroll
            for (int j = 0; j < kNcsenseSub; ++j) {
                if (j < nc) {                              // (uniform)
                    const float2 v = v_s[s][j];
                    const float ax = v.x * wy, ay = v.y * wy;          // rounded before the fma: the header's ((y w) wy) * wx
                    acc[j].x = fmaf(ax, wx, acc[j].x);
                    acc[j].y = fmaf(ay, wx, acc[j].y);
                }
            }
        }
        __syncthreads();
    }
    const size_t G = (size_t)gh * gw;
    float2* gp = grid + ((size_t)n * cb + j0) * G + (size_t)(ty0 + ty) * gw + (tx0 + tx);
#pragma unroll
    for (int j = 0; j < kNcsenseSub; ++j)
        if (j < nc) gp[(size_t)j * G] = acc[j];
}

// acc = (first ? +0 : q[n][p]);  per coil j < cb:  a = (cy cx) grid[n cb + j][window],  acc += conj(S_(c0+j)) a  (four fmas, the header's order);
// last: q = acc (+ mu[n] pv when pv != nullptr), partial[n, chunk, 0] = sum over the chunk of Re(conj(pv) q): nufft_crop_kernel's ranges and tree.
// CROP false (the naive form's combine): `grid` holds the coil images [N, cb, h, w] nufft_crop_kernel left, a = grid[n cb + j][p] as it is
template <bool CROP>
__global__ __launch_bounds__(kNsThreads) void ncsense_crop_kernel(const float2* __restrict__ grid, const float2* __restrict__ sens, int sens_n, int C,
                                                                  int c0, int cb, int first, int last, const float* __restrict__ cy,
                                                                  const float* __restrict__ cx, const float2* __restrict__ pv,
                                                                  const float* __restrict__ mu, const float* __restrict__ tact, float2* q,
                                                                  double* __restrict__ partial, int H, int W, int gh, int gw) {
    __shared__ double red[kNsThreads / 64];
    const int n = blockIdx.y, HW = H * W;
    if (stopped(tact, n)) return;
    const int p0 = blockIdx.x * kPixelChunk + threadIdx.x;
    const size_t base = (size_t)n * HW, G = CROP ? (size_t)gh * gw : (size_t)HW;
    const float2* gn = grid + (size_t)n * cb * G;
    const float2* sn = maps_of(sens, sens_n, n, C, HW) + (size_t)c0 * HW;
    const int oy = gh / 2 - H / 2, ox = gw / 2 - W / 2;
    const bool epi = last && pv != nullptr && mu != nullptr;
    const float m = epi ? mu[n] : 0.f;
    double dot[1] = {0.0};
#pragma unroll
    for (int k = 0; k < kNsPer; ++k) {
        const int p = p0 + k * kNsThreads;
        if (p < HW) {
            const int iy = p / W, ix = p - iy * W;
            const float f = CROP ? cy[iy] * cx[ix] : 1.f;
            const size_t go = CROP ? (size_t)(iy + oy) * gw + (ix + ox) : (size_t)p;
            float2 acc = first ? make_float2(0.f, 0.f) : q[base + p];
            for (int j = 0; j < cb; ++j) {
                const float2 g = gn[(size_t)j * G + go];
                const float2 sv = sn[(size_t)j * HW + p];
                const float ax = CROP ? g.x * f : g.x, ay = CROP ? g.y * f : g.y;
                acc.x = fmaf(sv.x, ax, acc.x);
                acc.x = fmaf(sv.y, ay, acc.x);
                acc.y = fmaf(sv.x, ay, acc.y);
                acc.y = fmaf(-sv.y, ax, acc.y);
            }
            if (epi) {
                const float2 pp = pv[base + p];
                acc.x = fmaf(m, pp.x, acc.x);
                acc.y = fmaf(m, pp.y, acc.y);
                dot[0] += (double)pp.x * (double)acc.x + (double)pp.y * (double)acc.y;
            }
            q[base + p] = acc;
        }
    }
    if (!epi || partial == nullptr) return;                // (uniform)
    block_sums_fixed<kNsThreads, 1>(dot, red);
    if (threadIdx.x == 0) partial[((size_t)n * gridDim.x + blockIdx.x) * 2] = dot[0];
}

// partial[n, c0 + j, chunk] = sum over the chunk's samples of w_m |a[n, j][m] - y[n, c0 + j][m]|^2: float32 differences, squared, weighted and
// summed in float64.  a: [N, cb, M], y: [N, C, M], partial: [N, C, chunks]
__global__ __launch_bounds__(kNsThreads) void ncsense_misfit_kernel(const float2* __restrict__ a, const float2* __restrict__ y,
                                                                    const float* __restrict__ w, double* __restrict__ partial, int C, int c0, int cb,
                                                                    int M) {
    __shared__ double red[kNsThreads / 64];
    const int n = blockIdx.y / cb, j = blockIdx.y - n * cb;
    const int m0 = blockIdx.x * kPixelChunk + threadIdx.x;
    const float2* an = a + ((size_t)n * cb + j) * M;
    const float2* yn = y + ((size_t)n * C + c0 + j) * M;
    double acc[1] = {0.0};
#pragma unroll
    for (int k = 0; k < kNsPer; ++k) {
        const int m = m0 + k * kNsThreads;
        if (m < M) {
            const float2 p = an[m], q = yn[m];
            const float dx = p.x - q.x, dy = p.y - q.y;
            const double t = (double)dx * (double)dx + (double)dy * (double)dy;
            acc[0] += w != nullptr ? (double)w[m] * t : t;
        }
    }
    block_sums_fixed<kNsThreads, 1>(acc, red);
    if (threadIdx.x == 0) partial[((size_t)n * C + c0 + j) * gridDim.x + blockIdx.x] = acc[0];
}

// dc[n][0] = the slice's `count` partials (coil-major, then chunk) summed in a fixed order, dc[n][1 .. dc_chunks) = 0: the layout
// residual_reduce_kernel sums (adding exact zeros changes no bit)
__global__ __launch_bounds__(kNsThreads) void ncsense_misfit_sum_kernel(const double* __restrict__ partial, int count, double* __restrict__ dc,
                                                                        int dc_chunks) {
    __shared__ double red[kNsThreads / 64];
    const int n = blockIdx.x;
    double acc[1] = {0.0};
    for (int i = threadIdx.x; i < count; i += kNsThreads) acc[0] += partial[(size_t)n * count + i];
    block_sums_fixed<kNsThreads, 1>(acc, red);
    for (int i = threadIdx.x; i < dc_chunks; i += kNsThreads)
        if (i > 0) dc[(size_t)n * dc_chunks + i] = 0.0;
    if (threadIdx.x == 0) dc[(size_t)n * dc_chunks] = acc[0];
}

// y[n][c][m] += sigma (g_re + i g_im): pnp_acquire's counter hash with p = m, the streams 9001 + 4 c / 9003 + 4 c, seed + n; float64, rounded once.
// The float64 sum keeps the contraction nufft_noise_kernel is compiled with, so that C = 1, S = 1 gives pnp_acquire_nc's numbers.
__global__ __launch_bounds__(kNsThreads) void ncsense_noise_kernel(float2* __restrict__ y, double sigma, unsigned long long seed, int C, int M) {
#pragma clang fp contract(fast)
    const int n = blockIdx.y, c = blockIdx.z;
    const int m = blockIdx.x * kNsThreads + threadIdx.x;
    if (m >= M) return;
    const size_t o = ((size_t)n * C + c) * M + m;
    const unsigned tre = kNoiseStreamRe + 4u * (unsigned)c, tim = kNoiseStreamIm + 4u * (unsigned)c;
    const unsigned long long sn = (seed + (unsigned long long)n) * 0x100000001B3ull;
    const unsigned long long bre1 = splitmix64(sn + tre), bre2 = splitmix64(sn + tre + 1u);
    const unsigned long long bim1 = splitmix64(sn + tim), bim2 = splitmix64(sn + tim + 1u);
    float2 v = y[o];
    v.x = (float)((double)v.x + gauss64(bre1, bre2, (unsigned long long)m) * sigma);
    v.y = (float)((double)v.y + gauss64(bim1, bim2, (unsigned long long)m) * sigma);
    y[o] = v;
}

}  // namespace

hipError_t launch_ncsense_pad(const float2* src, const float* src_real, const float2* sens, int sens_n, int C, int c0, int cb, const NufftDev& P,
                              float2* grid, int batch, hipStream_t s) {
    const dim3 g((unsigned)((P.gh * P.gw + kNsThreads - 1) / kNsThreads), (unsigned)batch);
    if (src_real != nullptr)
        hipLaunchKernelGGL(ncsense_pad_kernel<true>, g, dim3(kNsThreads), 0, s, (const void*)src_real, sens, sens_n, C, c0, cb, P.cy, P.cx, grid, P.h,
                           P.w, P.gh, P.gw);
    else
        hipLaunchKernelGGL(ncsense_pad_kernel<false>, g, dim3(kNsThreads), 0, s, (const void*)src, sens, sens_n, C, c0, cb, P.cy, P.cx, grid, P.h, P.w,
                           P.gh, P.gw);
    return hipGetLastError();
}

hipError_t launch_ncsense_interp(const float2* grid, const NufftDev& P, float2* out, int ocs, int oc0, int cb, int batch, hipStream_t s) {
    const dim3 g((unsigned)((P.m + kNsThreads - 1) / kNsThreads), (unsigned)batch);
#define PNP_NS_INTERP(J_) \
    hipLaunchKernelGGL(ncsense_interp_kernel<J_>, g, dim3(kNsThreads), 0, s, grid, P.i0, P.wts, out, ocs, oc0, cb, (int)P.m, P.gh, P.gw)
    if (P.width == 4) PNP_NS_INTERP(4);
    else if (P.width == 6) PNP_NS_INTERP(6);
    else PNP_NS_INTERP(8);
#undef PNP_NS_INTERP
    return hipGetLastError();
}

hipError_t launch_ncsense_grid(const float2* y, int ycs, int yc0, int cb, const float* w, const NufftDev& P, float2* grid, int batch, hipStream_t s) {
    const dim3 g((unsigned)(P.tiles_y * P.tiles_x), (unsigned)batch, (unsigned)((cb + kNcsenseSub - 1) / kNcsenseSub));
#define PNP_NS_GRID(J_)                                                                                                                      \
    hipLaunchKernelGGL(ncsense_grid_kernel<J_>, g, dim3(kNsThreads), 0, s, y, ycs, yc0, cb, w, P.i0, P.wts, P.bin_off, P.bin_idx, grid, (int)P.m, \
                       P.gh, P.gw, P.tiles_x)
    if (P.width == 4) PNP_NS_GRID(4);
    else if (P.width == 6) PNP_NS_GRID(6);
    else PNP_NS_GRID(8);
#undef PNP_NS_GRID
    return hipGetLastError();
}

hipError_t launch_ncsense_crop(const float2* grid, const float2* sens, int sens_n, int C, int c0, int cb, const NufftDev& P, const float2* pv,
                               const float* mu, const float* tact, float2* q, double* partial, int batch, hipStream_t s) {
    hipLaunchKernelGGL(ncsense_crop_kernel<true>, dim3((unsigned)pixel_chunks(P.h, P.w), (unsigned)batch), dim3(kNsThreads), 0, s, grid, sens, sens_n,
                       C, c0, cb, c0 == 0 ? 1 : 0, c0 + cb == C ? 1 : 0, P.cy, P.cx, pv, mu, tact, q, partial, P.h, P.w, P.gh, P.gw);
    return hipGetLastError();
}

hipError_t launch_ncsense_expand(const float2* src, const float* src_real, const float2* sens, int sens_n, int C, int c0, int cb, const NufftDev& P,
                                 float2* img, int batch, hipStream_t s) {
    const int HW = P.h * P.w;
    const dim3 g((unsigned)((HW + kNsThreads - 1) / kNsThreads), (unsigned)batch);
    if (src_real != nullptr)
        hipLaunchKernelGGL(ncsense_expand_kernel<true>, g, dim3(kNsThreads), 0, s, (const void*)src_real, sens, sens_n, C, c0, cb, img, HW);
    else
        hipLaunchKernelGGL(ncsense_expand_kernel<false>, g, dim3(kNsThreads), 0, s, (const void*)src, sens, sens_n, C, c0, cb, img, HW);
    return hipGetLastError();
}

hipError_t launch_ncsense_combine(const float2* img, const float2* sens, int sens_n, int C, int c0, int cb, const NufftDev& P, const float2* pv,
                                  const float* mu, const float* tact, float2* q, double* partial, int batch, hipStream_t s) {
    hipLaunchKernelGGL(ncsense_crop_kernel<false>, dim3((unsigned)pixel_chunks(P.h, P.w), (unsigned)batch), dim3(kNsThreads), 0, s, img, sens, sens_n,
                       C, c0, cb, c0 == 0 ? 1 : 0, c0 + cb == C ? 1 : 0, P.cy, P.cx, pv, mu, tact, q, partial, P.h, P.w, P.gh, P.gw);
    return hipGetLastError();
}

hipError_t launch_ncsense_misfit(const float2* a, const float2* y, const float* w, int C, int c0, int cb, const NufftDev& P, double* partial, int N,
                                 hipStream_t s) {
    hipLaunchKernelGGL(ncsense_misfit_kernel, dim3((unsigned)nufft_sample_chunks(P.m), (unsigned)(N * cb)), dim3(kNsThreads), 0, s, a, y, w, partial,
                       C, c0, cb, (int)P.m);
    return hipGetLastError();
}

hipError_t launch_ncsense_misfit_sum(const double* partial, int C, const NufftDev& P, double* dcpartial, int N, hipStream_t s) {
    hipLaunchKernelGGL(ncsense_misfit_sum_kernel, dim3((unsigned)N), dim3(kNsThreads), 0, s, partial, C * nufft_sample_chunks(P.m), dcpartial,
                       pixel_chunks(P.h, P.w));
    return hipGetLastError();
}

hipError_t launch_ncsense_noise(float2* y, double sigma, uint64_t seed, int C, const NufftDev& P, int N, hipStream_t s) {
    const dim3 g((unsigned)((P.m + kNsThreads - 1) / kNsThreads), (unsigned)N, (unsigned)C);
    hipLaunchKernelGGL(ncsense_noise_kernel, g, dim3(kNsThreads), 0, s, y, sigma, (unsigned long long)seed, C, (int)P.m);
    return hipGetLastError();
}

}  // namespace pnp
