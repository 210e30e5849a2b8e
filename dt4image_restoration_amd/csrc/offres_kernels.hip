// Off-resonance correction by time segmentation (include/pnpadmm_offres.h): the kernels of A p = [b0 F_nu(E_seg . p) + b1 F_nu(E_seg+1 . p)]_m
// and its adjoint around the coil-blocked pad, transform and crop-and-combine of the non-Cartesian SENSE stage, with the L segment maps E_l
// in the place of the coil maps.  A BLOCK of cb segments l0 .. l0 + cb - 1 of every slice is in flight at a time, grids [N, cb, gh, gw].
//
//   maps      offres_maps_kernel     E_l(r) = exp(-i omega(r) tau_l): phase, sine and cosine in float64, rounded once
//   forward   offres_interp_kernel   a thread per (slice, sample): the gather of the sample's TWO segment grids (those of them in the block),
//                                    blended in registers; a sample whose first segment lay in an earlier block continues from `out`
//   adjoint   offres_grid_kernel     a workgroup per (tile, slice, segment of the block): the plan's list of the tile's samples that carry
//                                    weight in that segment, (b q) formed at staging, then nufft_grid_kernel's chain
//   naive     (PNP_OFFRES_NAIVE=1: the bit-for-bit check and the timing baseline)  offres_blend_kernel blends the block's samples that the
//             non-Cartesian SENSE forward left, offres_expand_kernel writes (b_l q) for every segment of the block - zeros where a sample
//             carries no weight - for the non-Cartesian SENSE adjoint
//
// Every expression is written in the header's order and this unit is compiled without contraction.  Per segment plane the gather and the
// gridding are nufft_kernels.hip's chains; a skipped sample and a sample that adds (0 . q) leave the same number in the accumulator, so both
// forms agree as numbers, and the block size changes no bit (a float32 partial stored and reloaded is the same float32).  No atomics.
#include "pnp_internal.h"
#include "nufft_plan.h"

#pragma clang fp contract(off)

namespace pnp {

namespace {

constexpr int kOrThreads = 256;
constexpr int kOrChunk = 128;                              // samples staged per pass: 128 x 16 x (8 + 4) B = 24 KiB of LDS
static_assert(kNufftTile * kNufftTile == kOrThreads, "a thread per grid point of the tile");

__device__ __forceinline__ int wrap(int i, int g) { return i < 0 ? i + g : (i >= g ? i - g : i); }   // i in (-g, 2 g)

// maps[n][l][p] = (cos(ph), -sin(ph)), ph = (double)omega[n][p] * tau[l]
__global__ __launch_bounds__(kOrThreads) void offres_maps_kernel(const float* __restrict__ omega, const double* __restrict__ tau,
                                                                 float2* __restrict__ maps, int L, int HW) {
    const int n = blockIdx.z, l = blockIdx.y;
    const int p = blockIdx.x * kOrThreads + threadIdx.x;
    if (p >= HW) return;
    const double ph = (double)omega[(size_t)n * HW + p] * tau[l];
    maps[((size_t)n * L + l) * HW + p] = make_float2((float)cos(ph), (float)(-sin(ph)));
}

// The blend of one sample over the block l0 .. l0 + cb - 1: v(j) is the sample's value of the block's plane j.
//   o = seg in the block ? (b0 v0.x, b0 v0.y) : out (the partial an earlier block left);  seg + 1 in the block: o = fma(b1, v1, o)
template <class V>
__device__ __forceinline__ void blend_sample(int sg, float w0, float w1, int l0, int cb, int L, float2* o, V v) {
    const int j0 = sg - l0, j1 = j0 + 1;
    const bool in0 = j0 >= 0 && j0 < cb, in1 = L > 1 && j1 >= 0 && j1 < cb;
    if (!in0 && !in1) return;
    float2 r = *o;
    if (in0) {
        const float2 a = v(j0);
        r = make_float2(w0 * a.x, w0 * a.y);
    }
    if (in1) {
        const float2 a = v(j1);
        r.x = fmaf(w1, a.x, r.x);
        r.y = fmaf(w1, a.y, r.y);
    }
    *o = r;
}

// out[n][m] = the blend of nufft_interp_kernel's double chain on the sample's segment planes of the block; grid: [N, cb, gh, gw]
template <int J>
__global__ __launch_bounds__(kOrThreads) void offres_interp_kernel(const float2* __restrict__ grid, const int* __restrict__ i0,
                                                                   const float* __restrict__ wts, const int* __restrict__ seg,
                                                                   const float* __restrict__ b0, const float* __restrict__ b1, float2* out, int l0,
                                                                   int cb, int L, int M, int gh, int gw) {
    const int n = blockIdx.y;
    const int m = blockIdx.x * kOrThreads + threadIdx.x;
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
    const auto gather = [&](int c) {
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
        return acc;
    };
    float2* o = out + (size_t)n * M + m;
    float2 r = *o;
    blend_sample(seg[m], b0[m], b1[m], l0, cb, L, &r, gather);
    *o = r;
}

// the naive form's blend: samp [N, cb, M] are the block's samples as the non-Cartesian SENSE forward left them
__global__ __launch_bounds__(kOrThreads) void offres_blend_kernel(const float2* __restrict__ samp, const int* __restrict__ seg,
                                                                  const float* __restrict__ b0, const float* __restrict__ b1, float2* out, int l0,
                                                                  int cb, int L, int M) {
    const int n = blockIdx.y;
    const int m = blockIdx.x * kOrThreads + threadIdx.x;
    if (m >= M) return;
    const auto value = [&](int c) { return samp[((size_t)n * cb + c) * M + m]; };
    float2* o = out + (size_t)n * M + m;
    float2 r = *o;
    blend_sample(seg[m], b0[m], b1[m], l0, cb, L, &r, value);
    *o = r;
}

// the naive form's expansion: ye[n][j][m] = b_(l0+j)(m) . y[n][m], the two products rounded; +0 where the sample carries no weight
__global__ __launch_bounds__(kOrThreads) void offres_expand_kernel(const float2* __restrict__ y, const int* __restrict__ seg,
                                                                   const float* __restrict__ b0, const float* __restrict__ b1,
                                                                   float2* __restrict__ ye, int l0, int cb, int L, int M) {
    const int n = blockIdx.y;
    const int m = blockIdx.x * kOrThreads + threadIdx.x;
    if (m >= M) return;
    const float2 v = y[(size_t)n * M + m];
    const int sg = seg[m];
    const float w0 = b0[m], w1 = b1[m];
    for (int j = 0; j < cb; ++j) {
        const int l = l0 + j;
        float2 t = make_float2(0.f, 0.f);
        if (l == sg) t = make_float2(w0 * v.x, w0 * v.y);
        else if (L > 1 && l == sg + 1) t = make_float2(w1 * v.x, w1 * v.y);
        ye[((size_t)n * cb + j) * M + m] = t;
    }
}

// One workgroup per (tile, slice, segment j of the block): nufft_grid_kernel on the list of (segment l0 + j, tile) with the sample value
// (b y): b = b0 where seg_m is the segment, b1 where it is the one before.  y: [N, M], w: [M] weights or nullptr (1); grid: [N, cb, gh, gw].
// filter != 0 (PNP_OFFRES_GRID_FILTER=1, the other layout, kept for the timing): list_off / list_idx are the NUFFT plan's tile bins, walked
// whole by every segment's workgroup; a sample that carries no weight in the segment is staged as +0 and adds nothing - the same numbers
template <int J>
__global__ __launch_bounds__(kOrThreads) void offres_grid_kernel(const float2* __restrict__ y, const float* __restrict__ w, const int* __restrict__ i0,
                                                                 const float* __restrict__ wts, const int* __restrict__ seg,
                                                                 const float* __restrict__ b0, const float* __restrict__ b1,
                                                                 const int* __restrict__ list_off, const int* __restrict__ list_idx,
                                                                 float2* __restrict__ grid, int l0, int cb, int M, int gh, int gw, int tiles_x,
                                                                 int tiles, int filter) {
    __shared__ float2 a_s[kOrChunk][kNufftTile];
    __shared__ float wx_s[kOrChunk][kNufftTile];
    const int tile = blockIdx.x, n = blockIdx.y, jb = blockIdx.z, l = l0 + jb;
    const int ty0 = (tile / tiles_x) * kNufftTile, tx0 = (tile % tiles_x) * kNufftTile;
    const int tx = threadIdx.x % kNufftTile, ty = threadIdx.x / kNufftTile;
    const size_t row = filter ? (size_t)tile : (size_t)l * tiles + tile;
    const int s0 = list_off[row], s1 = list_off[row + 1];
    const float2* yn = y + (size_t)n * M;
    float2 acc = make_float2(0.f, 0.f);
    for (int c0 = s0; c0 < s1; c0 += kOrChunk) {
        const int cnt = min(kOrChunk, s1 - c0);
        for (int idx = threadIdx.x; idx < cnt * kNufftTile; idx += kOrThreads) {
            const int sl = idx / kNufftTile, j = idx % kNufftTile;
            const int m = list_idx[c0 + sl];
            const int d = wrap(ty0 + j - i0[m], gh), e = wrap(tx0 + j - i0[(size_t)M + m], gw);
            float2 v = make_float2(0.f, 0.f);
            const int sg = seg[m];
            if (d < J && (sg == l || sg == l - 1)) {         // (the lists hold no other sample; the whole bin does)
                const float wy = wts[(size_t)d * M + m];
                const float b = sg == l ? b0[m] : b1[m];
                v = yn[m];
                v.x *= b; v.y *= b;
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
    grid[((size_t)n * cb + jb) * gh * gw + (size_t)(ty0 + ty) * gw + (tx0 + tx)] = acc;
}

}  // namespace

hipError_t launch_offres_maps(const float* omega, int map_n, const OffresDev& R, const NufftDev& P, float2* maps, hipStream_t s) {
    const int HW = P.h * P.w;
    const dim3 g((unsigned)((HW + kOrThreads - 1) / kOrThreads), (unsigned)R.segments, (unsigned)map_n);
    hipLaunchKernelGGL(offres_maps_kernel, g, dim3(kOrThreads), 0, s, omega, R.tau, maps, R.segments, HW);
    return hipGetLastError();
}

hipError_t launch_offres_interp(const float2* grid, const OffresDev& R, const NufftDev& P, float2* out, int l0, int cb, int batch, hipStream_t s) {
    const dim3 g((unsigned)((P.m + kOrThreads - 1) / kOrThreads), (unsigned)batch);
#define PNP_OR_INTERP(J_)                                                                                                                   \
    hipLaunchKernelGGL(offres_interp_kernel<J_>, g, dim3(kOrThreads), 0, s, grid, P.i0, P.wts, R.seg, R.b0, R.b1, out, l0, cb, R.segments, (int)P.m, \
                       P.gh, P.gw)
    if (P.width == 4) PNP_OR_INTERP(4);
    else if (P.width == 6) PNP_OR_INTERP(6);
    else PNP_OR_INTERP(8);
#undef PNP_OR_INTERP
    return hipGetLastError();
}

hipError_t launch_offres_blend(const float2* samp, const OffresDev& R, const NufftDev& P, float2* out, int l0, int cb, int batch, hipStream_t s) {
    const dim3 g((unsigned)((P.m + kOrThreads - 1) / kOrThreads), (unsigned)batch);
    hipLaunchKernelGGL(offres_blend_kernel, g, dim3(kOrThreads), 0, s, samp, R.seg, R.b0, R.b1, out, l0, cb, R.segments, (int)P.m);
    return hipGetLastError();
}

hipError_t launch_offres_expand(const float2* y, const OffresDev& R, const NufftDev& P, float2* ye, int l0, int cb, int batch, hipStream_t s) {
    const dim3 g((unsigned)((P.m + kOrThreads - 1) / kOrThreads), (unsigned)batch);
    hipLaunchKernelGGL(offres_expand_kernel, g, dim3(kOrThreads), 0, s, y, R.seg, R.b0, R.b1, ye, l0, cb, R.segments, (int)P.m);
    return hipGetLastError();
}

hipError_t launch_offres_grid(const float2* y, const float* w, const OffresDev& R, const NufftDev& P, float2* grid, int l0, int cb, int batch,
                              hipStream_t s, bool filter) {
    const int tiles = P.tiles_y * P.tiles_x;
    const dim3 g((unsigned)tiles, (unsigned)batch, (unsigned)cb);
#define PNP_OR_GRID(J_)                                                                                                                       \
    hipLaunchKernelGGL(offres_grid_kernel<J_>, g, dim3(kOrThreads), 0, s, y, w, P.i0, P.wts, R.seg, R.b0, R.b1, filter ? P.bin_off : R.list_off, \
                       filter ? P.bin_idx : R.list_idx, grid, l0, cb, (int)P.m, P.gh, P.gw, P.tiles_x, tiles, filter ? 1 : 0)
    if (P.width == 4) PNP_OR_GRID(4);
    else if (P.width == 6) PNP_OR_GRID(6);
    else PNP_OR_GRID(8);
#undef PNP_OR_GRID
    return hipGetLastError();
}

}  // namespace pnp
