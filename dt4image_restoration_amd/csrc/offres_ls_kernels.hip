// Off-resonance correction with the least-squares temporal interpolator (include/pnpadmm_offres_ls.h): every sample carries a coefficient
// b_l(m) for EVERY segment, coef [L][M].  The kernels of A p = [sum_l b_l F_nu(E_l . p)]_m and its adjoint around the coil-blocked pad,
// transform and crop-and-combine of the non-Cartesian SENSE stage, as offres_kernels.hip's are for the linear interpolator.  A BLOCK of cb
// segments l0 .. l0 + cb - 1 of every slice is in flight at a time, grids [N, cb, gh, gw].
//
//   forward   offres_ls_interp_kernel   a thread per (slice, sample): i0, the 2 J weights and the wrapped rows and columns loaded once, the
//                                       block's cb grids walked with the blend kept in registers; no [N, cb, M] intermediate
//   adjoint   offres_ls_grid_kernel     a workgroup per (tile, slice, sub-block of <= kLsSub segments): a chunk of the tile's bin is staged
//                                       once - wx, the row mask and the index arithmetic shared by the segments, ((b_l q) w) wy per segment -
//                                       and every thread keeps accumulators for 4 segments at 2 grid points of one row (the waves split
//                                       the segments): 4 staged values and 2 staged wx per 16 FMAs.  A wave owns 8 of the tile's 16 rows
//                                       and skips, wave-uniformly, a sample whose footprint touches none of them
//   naive     (PNP_OFFRES_LS_NAIVE=1: the bit-for-bit check and the timing baseline)  offres_ls_blend_kernel blends the block's samples that
//             the non-Cartesian SENSE forward left, offres_ls_expand_kernel writes (b_l q) for every segment of the block for the
//             non-Cartesian SENSE adjoint
//
// Every expression is written in the header's order and this unit is compiled without contraction.  Per segment plane the gather and the
// gridding are nufft_kernels.hip's chains; a skipped sample and a sample that adds (0 . wx) leave the same number in the accumulator, so both
// forms agree as numbers, and the block size changes no bit (a float32 partial stored and reloaded is the same float32).  No atomics.
#include "pnp_internal.h"
#include "nufft_plan.h"

#pragma clang fp contract(off)

namespace pnp {

namespace {

constexpr int kLsThreads = 256;
constexpr int kLsChunk = 32;                               // samples staged per pass
constexpr int kLsSub = kOffresLsSub;                       // segments per gridding workgroup: 8 x 32 x 16 x 8 B = 32 KiB (+ 2 KiB wx) of LDS
static_assert(kNufftTile * kNufftTile == kLsThreads, "a thread per grid point of the tile");
constexpr int kLsHalf = kLsSub / 2;                        // segments per thread of the gridding: the workgroup's waves split the sub-block
constexpr int kLsCols = kNufftTile / 2;                    // a gridding thread owns the columns cx and cx + kLsCols of its row
static_assert(kNufftTile == 16 && kLsThreads == 256 && kLsThreads / 2 == kNufftTile * kLsCols,
              "half the workgroup covers the tile at two columns per thread; a wave of 64 threads owns 8 rows: the row mask's bytes");

__device__ __forceinline__ int wrap(int i, int g) { return i < 0 ? i + g : (i >= g ? i - g : i); }   // i in (-g, 2 g)

// One step of the header's forward chain: segment l = 0 starts it with the rounded products, every later one is an fma
__device__ __forceinline__ void blend_step(int l, float b, float2 v, float2* r) {
    if (l == 0) *r = make_float2(b * v.x, b * v.y);
    else { r->x = fmaf(b, v.x, r->x); r->y = fmaf(b, v.y, r->y); }
}

// out[n][m] = the chain over the block's segments of nufft_interp_kernel's double chain on each plane; grid: [N, cb, gh, gw].  l0 > 0: the
// chain continues from the partial an earlier block left in out
template <int J>
__global__ __launch_bounds__(kLsThreads) void offres_ls_interp_kernel(const float2* __restrict__ grid, const int* __restrict__ i0,
                                                                      const float* __restrict__ wts, const float* __restrict__ coef, float2* out,
                                                                      int l0, int cb, int M, int gh, int gw) {
    const int n = blockIdx.y;
    const int m = blockIdx.x * kLsThreads + threadIdx.x;
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
    float2* o = out + (size_t)n * M + m;
    float2 r = make_float2(0.f, 0.f);
    if (l0 > 0) r = *o;
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
        blend_step(l0 + c, coef[(size_t)(l0 + c) * M + m], acc, &r);
    }
    *o = r;
}

// the naive form's blend: samp [N, cb, M] are the block's samples as the non-Cartesian SENSE forward left them
__global__ __launch_bounds__(kLsThreads) void offres_ls_blend_kernel(const float2* __restrict__ samp, const float* __restrict__ coef, float2* out,
                                                                     int l0, int cb, int M) {
    const int n = blockIdx.y;
    const int m = blockIdx.x * kLsThreads + threadIdx.x;
    if (m >= M) return;
    float2* o = out + (size_t)n * M + m;
    float2 r = make_float2(0.f, 0.f);
    if (l0 > 0) r = *o;
    for (int c = 0; c < cb; ++c) blend_step(l0 + c, coef[(size_t)(l0 + c) * M + m], samp[((size_t)n * cb + c) * M + m], &r);
    *o = r;
}

// the naive form's expansion: ye[n][j][m] = b_(l0+j)(m) . y[n][m], the two products rounded
__global__ __launch_bounds__(kLsThreads) void offres_ls_expand_kernel(const float2* __restrict__ y, const float* __restrict__ coef,
                                                                      float2* __restrict__ ye, int l0, int cb, int M) {
    const int n = blockIdx.y;
    const int m = blockIdx.x * kLsThreads + threadIdx.x;
    if (m >= M) return;
    const float2 v = y[(size_t)n * M + m];
    for (int j = 0; j < cb; ++j) {
        const float b = coef[(size_t)(l0 + j) * M + m];
        ye[((size_t)n * cb + j) * M + m] = make_float2(b * v.x, b * v.y);
    }
}

// One workgroup per (tile, slice, sub-block): the segments l0 + jb kLsSub .. of the block, nc = min(kLsSub, cb - jb kLsSub) of them, each
// with nufft_grid_kernel's chain over ALL samples of the tile's bin on the sample value (b_l y).  y: [N, M], w: [M] weights or nullptr (1);
// grid: [N, cb, gh, gw].  rows_s[s] holds bit j where the sample's footprint contains row j of the tile; a wave reads its byte.  skip == 0:
// the same kernel without the test (timing).
template <int J>
__global__ __launch_bounds__(kLsThreads) void offres_ls_grid_kernel(const float2* __restrict__ y, const float* __restrict__ w,
                                                                    const int* __restrict__ i0, const float* __restrict__ wts,
                                                                    const float* __restrict__ coef, const int* __restrict__ bin_off,
                                                                    const int* __restrict__ bin_idx, float2* __restrict__ grid, int l0, int cb,
                                                                    int M, int gh, int gw, int tiles_x, int skip) {
    __shared__ float2 a_s[kLsSub][kLsChunk][kNufftTile];
    __shared__ float wx_s[kLsChunk][kNufftTile];
    __shared__ unsigned rows_s[kLsChunk];
    const int tile = blockIdx.x, n = blockIdx.y, j0 = blockIdx.z * kLsSub;
    const int nc = min(kLsSub, cb - j0);
    const int ty0 = (tile / tiles_x) * kNufftTile, tx0 = (tile % tiles_x) * kNufftTile;
    // waves 0, 1 take the sub-block's segments 0 .. 3, waves 2, 3 the segments 4 .. 7; a wave owns 8 rows, a thread the columns cx and cx + 8
    // of one row for its 4 segments: 4 staged values and 2 staged wx per 16 FMAs
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
    const int cbase = (wave / 2) * kLsHalf, mync = min(kLsHalf, nc - cbase);
    const int r = threadIdx.x % (kLsThreads / 2), ty = r / kLsCols, cx = r % kLsCols;
    const unsigned mine = skip ? 0xFFu << (8 * (wave % 2)) : 0xFFFFu;
    const int s0 = bin_off[tile], s1 = bin_off[tile + 1];
    const float2* yn = y + (size_t)n * M;
    const float* cf = coef + (size_t)(l0 + j0) * M;
    float2 acc[kLsHalf][2];
#pragma unroll
    for (int c = 0; c < kLsHalf; ++c) acc[c][0] = acc[c][1] = make_float2(0.f, 0.f);
    for (int c0 = s0; c0 < s1; c0 += kLsChunk) {
        const int cnt = min(kLsChunk, s1 - c0);
        for (int idx = threadIdx.x; idx < cnt * kNufftTile; idx += kLsThreads) {
            const int sl = idx / kNufftTile, j = idx % kNufftTile;
            const int m = bin_idx[c0 + sl];
            const int d = wrap(ty0 + j - i0[m], gh), e = wrap(tx0 + j - i0[(size_t)M + m], gw);
            const bool in = d < J;
            float2 v = make_float2(0.f, 0.f);
            float wy = 0.f, ww = 1.f;
            if (in) {
                wy = wts[(size_t)d * M + m];
                v = yn[m];
                if (w != nullptr) ww = w[m];
            }
#pragma unroll
            for (int c = 0; c < kLsSub; ++c) {
                if (c < nc) {
                    float2 t = make_float2(0.f, 0.f);
                    if (in) {
                        const float b = cf[(size_t)c * M + m];
                        t = make_float2(b * v.x, b * v.y);
                        if (w != nullptr) { t.x *= ww; t.y *= ww; }
                        t.x *= wy; t.y *= wy;
                    }
                    a_s[c][sl][j] = t;
                }
            }
            wx_s[sl][j] = e < J ? wts[(size_t)(J + e) * M + m] : 0.f;
            // the 16 lanes of a sample are neighbours in one wave: their `in` bits are the sample's row mask
            const unsigned long long bal = __ballot(in);
            if (j == 0) rows_s[sl] = (unsigned)(bal >> (16 * ((threadIdx.x % 64) / kNufftTile))) & 0xFFFFu;
        }
        __syncthreads();
        for (int s = 0; s < cnt; ++s) {
            if ((rows_s[s] & mine) == 0u) continue;         // wave-uniform: every a_s[.][s][ty] of this wave is +0
            const float wx0 = wx_s[s][cx], wx1 = wx_s[s][cx + kLsCols];
#pragma unroll
            for (int c = 0; c < kLsHalf; ++c) {
                if (c < mync) {
                    const float2 a = a_s[cbase + c][s][ty];
                    acc[c][0].x = fmaf(a.x, wx0, acc[c][0].x);
                    acc[c][0].y = fmaf(a.y, wx0, acc[c][0].y);
                    acc[c][1].x = fmaf(a.x, wx1, acc[c][1].x);
                    acc[c][1].y = fmaf(a.y, wx1, acc[c][1].y);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < kLsHalf; ++c)
        if (c < mync) {
            float2* gp = grid + ((size_t)n * cb + j0 + cbase + c) * gh * gw + (size_t)(ty0 + ty) * gw + (tx0 + cx);
            gp[0] = acc[c][0];
            gp[kLsCols] = acc[c][1];
        }
}

}  // namespace

hipError_t launch_offres_ls_interp(const float2* grid, const OffresDev& R, const NufftDev& P, float2* out, int l0, int cb, int batch, hipStream_t s) {
    const dim3 g((unsigned)((P.m + kLsThreads - 1) / kLsThreads), (unsigned)batch);
#define PNP_LS_INTERP(J_) \
    hipLaunchKernelGGL(offres_ls_interp_kernel<J_>, g, dim3(kLsThreads), 0, s, grid, P.i0, P.wts, R.coef, out, l0, cb, (int)P.m, P.gh, P.gw)
    if (P.width == 4) PNP_LS_INTERP(4);
    else if (P.width == 6) PNP_LS_INTERP(6);
    else PNP_LS_INTERP(8);
#undef PNP_LS_INTERP
    return hipGetLastError();
}

hipError_t launch_offres_ls_blend(const float2* samp, const OffresDev& R, const NufftDev& P, float2* out, int l0, int cb, int batch, hipStream_t s) {
    const dim3 g((unsigned)((P.m + kLsThreads - 1) / kLsThreads), (unsigned)batch);
    hipLaunchKernelGGL(offres_ls_blend_kernel, g, dim3(kLsThreads), 0, s, samp, R.coef, out, l0, cb, (int)P.m);
    return hipGetLastError();
}

hipError_t launch_offres_ls_expand(const float2* y, const OffresDev& R, const NufftDev& P, float2* ye, int l0, int cb, int batch, hipStream_t s) {
    const dim3 g((unsigned)((P.m + kLsThreads - 1) / kLsThreads), (unsigned)batch);
    hipLaunchKernelGGL(offres_ls_expand_kernel, g, dim3(kLsThreads), 0, s, y, R.coef, ye, l0, cb, (int)P.m);
    return hipGetLastError();
}

hipError_t launch_offres_ls_grid(const float2* y, const float* w, const OffresDev& R, const NufftDev& P, float2* grid, int l0, int cb, int batch,
                                 hipStream_t s, bool skip) {
    const int tiles = P.tiles_y * P.tiles_x;
    const dim3 g((unsigned)tiles, (unsigned)batch, (unsigned)((cb + kLsSub - 1) / kLsSub));
#define PNP_LS_GRID(J_)                                                                                                                      \
    hipLaunchKernelGGL(offres_ls_grid_kernel<J_>, g, dim3(kLsThreads), 0, s, y, w, P.i0, P.wts, R.coef, P.bin_off, P.bin_idx, grid, l0, cb, \
                       (int)P.m, P.gh, P.gw, P.tiles_x, skip ? 1 : 0)
    if (P.width == 4) PNP_LS_GRID(4);
    else if (P.width == 6) PNP_LS_GRID(6);
    else PNP_LS_GRID(8);
#undef PNP_LS_GRID
    return hipGetLastError();
}

}  // namespace pnp
