// Toeplitz form of the off-resonance normal operator (include/pnpadmm_offres_tz.h): the multi-spectrum build and the spectral mix.  The
// pointwise kernels around them are those of the non-Cartesian SENSE stage (expand, combine: E_l in the place of coil maps) and of the plain
// Toeplitz operator (pad, crop), the transforms the engine's row and column passes.
//
//   setup   offres_tz_spectra_kernel   K_ll'[j, k] = (1 / (H W)) sum_m u_ll'(m) D_H(ky_m - (j - H) / 2H) D_W(kx_m - (k - W) / 2W), float64, rounded once
//   apply   offres_tz_mix_kernel       Y_l = scale . sum over ascending l' of K_ll' X_l' per bin of the 2H x 2W grid, for a block of slices
//
// The build is toeplitz_spectrum_kernel for PB weight vectors at once.  One workgroup owns one kToeplitzTile^2 tile of PB consecutive pairs
// and walks the block's samples in ascending order, kOtzChunk at a time: a chunk is staged in LDS as, per sample, the row vector D_H at the
// tile's rows, the column vector D_W at its columns (2 x 32 Dirichlet quotients per sample, shared by the PB pairs) and the PB weights
// u = ((double)w_m * (double)b_l) * (double)b_l'; every thread then forms u D_H at its 4 rows and runs acc = fma(u D_H, D_W, acc) on its PB
// 4 x 4 register blocks.  No atomics and no partial sums: an output's value is the fma chain from 0 over ascending m whatever the tile or
// the block, and a sample outside a pair's support adds 0 . D_W, which leaves the chain's number as skipping it does - so the bits depend
// on (trajectory, times plan, weights, H, W) only.  Under a linear plan the block's list (offres_tz_plan.h) holds the samples of two
// segments; under a least-squares plan every block walks every sample.
// Every expression is written in the header's order and this unit is compiled without contraction.
#include "pnp_internal.h"

#pragma clang fp contract(off)

#include "toeplitz_dirichlet.h"

namespace pnp {

namespace {

constexpr int kOtzSpecThreads = 64;                        // an 8 x 8 grid of threads, a 4 x 4 register block per pair each
constexpr int kOtzReg = 4, kOtzSide = 8;
static_assert(kOtzReg * kOtzSide == kToeplitzTile && kOtzSide * kOtzSide == kOtzSpecThreads, "the register blocks tile the workgroup's tile");
constexpr int kOtzChunk = 32;                              // samples staged per pass: 2 x 32 x 32 x 8 B + 32 x PB x 8 B = 17 KiB of LDS at PB = 4
constexpr int kOtzMixThreads = 256;

// b_l(m) of the live plan: the stored float32 coefficient, or 0 where the linear interpolator has none
__device__ __forceinline__ float offres_coef(const OffresDev& R, int l, int m, int M) {
    if (R.kind == 2) return R.coef[(size_t)l * M + m];
    const int sg = R.seg[m];
    return l == sg ? R.b0[m] : (l == sg + 1 ? R.b1[m] : 0.f);
}
// pair p of the header's order -> (l, l')
__device__ __forceinline__ void offres_pair(int kind, int L, int p, int* l, int* r) {
    if (kind == 1) { *l = p >> 1; *r = (p >> 1) + (p & 1); return; }
    int row = 0, left = p;
    while (left >= L - row) { left -= L - row; ++row; }     // the upper triangle row by row
    *l = row; *r = row + left;
}

template <int PB>
__global__ __launch_bounds__(kOtzSpecThreads) void offres_tz_spectra_kernel(const double2* __restrict__ traj, const float* __restrict__ w, OffresDev R,
                                                                            const int* __restrict__ blk_off, const int* __restrict__ blk_idx,
                                                                            int pairs, int M, int H, int W, float* __restrict__ K) {
    __shared__ double a_s[kOtzChunk][kToeplitzTile];
    __shared__ double b_s[kOtzChunk][kToeplitzTile];
    __shared__ double u_s[kOtzChunk][PB];
    const int j0 = blockIdx.y * kToeplitzTile, k0 = blockIdx.x * kToeplitzTile, p0 = blockIdx.z * PB;
    const int tx = threadIdx.x % kOtzSide, ty = threadIdx.x / kOtzSide;
    const int first = blk_off != nullptr ? blk_off[blockIdx.z] : 0;
    const int count = blk_off != nullptr ? blk_off[blockIdx.z + 1] - first : M;
    double acc[PB][kOtzReg][kOtzReg];
#pragma unroll
    for (int p = 0; p < PB; ++p)
#pragma unroll
        for (int i = 0; i < kOtzReg; ++i)
#pragma unroll
            for (int k = 0; k < kOtzReg; ++k) acc[p][i][k] = 0.0;
    for (int c0 = 0; c0 < count; c0 += kOtzChunk) {
        const int cnt = min(kOtzChunk, count - c0);
        for (int idx = threadIdx.x; idx < cnt * kToeplitzTile; idx += kOtzSpecThreads) {
            const int sl = idx / kToeplitzTile, r = idx % kToeplitzTile;
            const int m = blk_idx != nullptr ? blk_idx[first + c0 + sl] : c0 + sl;
            const double2 k = traj[m];                     // (ky, kx)
            a_s[sl][r] = dirichlet(k.x - (double)(j0 + r - H) / (double)(2 * H), H);
            b_s[sl][r] = dirichlet(k.y - (double)(k0 + r - W) / (double)(2 * W), W);
        }
        for (int idx = threadIdx.x; idx < cnt * PB; idx += kOtzSpecThreads) {
            const int sl = idx / PB, p = idx % PB;
            const int m = blk_idx != nullptr ? blk_idx[first + c0 + sl] : c0 + sl;
            double u = 0.0;
            if (p0 + p < pairs) {
                int l, r;
                offres_pair(R.kind, R.segments, p0 + p, &l, &r);
                const double ww = w != nullptr ? (double)w[m] : 1.0;
                u = (ww * (double)offres_coef(R, l, m, M)) * (double)offres_coef(R, r, m, M);
            }
            u_s[sl][p] = u;
        }
        __syncthreads();
        for (int s = 0; s < cnt; ++s) {
            double a[kOtzReg], b[kOtzReg];
#pragma unroll
            for (int i = 0; i < kOtzReg; ++i) { a[i] = a_s[s][ty + kOtzSide * i]; b[i] = b_s[s][tx + kOtzSide * i]; }
#pragma unroll
            for (int p = 0; p < PB; ++p) {
                const double u = u_s[s][p];
#pragma unroll
                for (int i = 0; i < kOtzReg; ++i) {
                    const double ua = u * a[i];
#pragma unroll
                    for (int k = 0; k < kOtzReg; ++k) acc[p][i][k] = fma(ua, b[k], acc[p][i][k]);
                }
            }
        }
        __syncthreads();
    }
    const double hw = (double)H * (double)W;
    const size_t G = (size_t)4 * H * W;
#pragma unroll
    for (int p = 0; p < PB; ++p) {
        if (p0 + p >= pairs) break;
#pragma unroll
        for (int i = 0; i < kOtzReg; ++i)
#pragma unroll
            for (int k = 0; k < kOtzReg; ++k)
                K[(size_t)(p0 + p) * G + (size_t)(j0 + ty + kOtzSide * i) * (2 * W) + (k0 + tx + kOtzSide * k)] = (float)(acc[p][i][k] / hw);
    }
}

// One thread per bin g of the grid; it keeps its bin's spectra in registers over the slices n0 .. of its slice group and, per slice, loads the
// L inputs, then stores the L outputs: out of place.  LMAX >= L bounds the register arrays; every index into them is a compile-time constant.
// BAND: the linear plan's pair order (l, l) at 2 l, (l, l + 1) at 2 l + 1; else the upper triangle of the L x L matrix row by row.
template <int LMAX, bool BAND>
__global__ __launch_bounds__(kOtzMixThreads) void offres_tz_mix_kernel(const float2* __restrict__ x, float2* __restrict__ y, const float* __restrict__ K,
                                                                       int L, int G, int slices, int per, float scale) {
    const int g = blockIdx.x * kOtzMixThreads + threadIdx.x;
    if (g >= G) return;
    const int n0 = blockIdx.y * per, n1 = min(slices, n0 + per);
    constexpr int NK = BAND ? 2 * LMAX - 1 : LMAX * (LMAX + 1) / 2;
    float k[NK];
    if (BAND) {
#pragma unroll
        for (int i = 0; i < NK; ++i) k[i] = i < 2 * L - 1 ? K[(size_t)i * G + g] : 0.f;
    } else {
#pragma unroll
        for (int l = 0; l < LMAX; ++l)
#pragma unroll
            for (int r = l; r < LMAX; ++r)
                k[l * LMAX - l * (l - 1) / 2 + (r - l)] = r < L ? K[(size_t)(l * L - l * (l - 1) / 2 + (r - l)) * G + g] : 0.f;
    }
    for (int n = n0; n < n1; ++n) {
        const float2* xn = x + (size_t)n * L * G + g;
        float2* yn = y + (size_t)n * L * G + g;
        float2 v[LMAX];
#pragma unroll
        for (int l = 0; l < LMAX; ++l)
            if (l < L) v[l] = xn[(size_t)l * G];
#pragma unroll
        for (int l = 0; l < LMAX; ++l) {
            if (l < L) {
                float2 acc = make_float2(0.f, 0.f);
                if (BAND) {
                    const int lm = l > 0 ? l - 1 : 0, lp = l + 1 < LMAX ? l + 1 : l;   // (constants once unrolled; clamped where the branch is dead)
                    if (l > 0) {
                        acc.x = fmaf(k[2 * lm + 1], v[lm].x, acc.x);
                        acc.y = fmaf(k[2 * lm + 1], v[lm].y, acc.y);
                    }
                    acc.x = fmaf(k[2 * l], v[l].x, acc.x);
                    acc.y = fmaf(k[2 * l], v[l].y, acc.y);
                    if (l + 1 < LMAX && l + 1 < L) {
                        acc.x = fmaf(k[2 * lp - 1], v[lp].x, acc.x);
                        acc.y = fmaf(k[2 * lp - 1], v[lp].y, acc.y);
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < LMAX; ++r) {
                        if (r < L) {
                            const int lo = l < r ? l : r, hi = l < r ? r : l;
                            const float kk = k[lo * LMAX - lo * (lo - 1) / 2 + (hi - lo)];
                            acc.x = fmaf(kk, v[r].x, acc.x);
                            acc.y = fmaf(kk, v[r].y, acc.y);
                        }
                    }
                }
                yn[(size_t)l * G] = make_float2(acc.x * scale, acc.y * scale);
            }
        }
    }
}

template <int LMAX, bool BAND>
hipError_t launch_mix(const float2* x, float2* y, const float* K, int L, int G, int slices, float scale, hipStream_t s) {
    const int gx = (G + kOtzMixThreads - 1) / kOtzMixThreads;
    // enough workgroups to fill the chip on small grids; on large ones a workgroup walks every slice and reads its spectra once
    int groups = gx >= 1024 ? 1 : (1024 + gx - 1) / gx;
    if (groups > slices) groups = slices;
    const int per = (slices + groups - 1) / groups;
    groups = (slices + per - 1) / per;
    hipLaunchKernelGGL((offres_tz_mix_kernel<LMAX, BAND>), dim3((unsigned)gx, (unsigned)groups), dim3(kOtzMixThreads), 0, s, x, y, K, L, G, slices, per,
                       scale);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_offres_tz_spectra(const double* traj, const float* w, const OffresDev& R, const OffresTzDev& T, int64_t m, int H, int W, float* K,
                                    hipStream_t s) {
    const dim3 g((unsigned)(2 * W / kToeplitzTile), (unsigned)(2 * H / kToeplitzTile), (unsigned)T.blocks);
    const double2* t2 = reinterpret_cast<const double2*>(traj);
    if (T.pair_block == 2)
        hipLaunchKernelGGL(offres_tz_spectra_kernel<2>, g, dim3(kOtzSpecThreads), 0, s, t2, w, R, T.blk_off, T.blk_idx, T.pairs, (int)m, H, W, K);
    else if (T.pair_block == 4)
        hipLaunchKernelGGL(offres_tz_spectra_kernel<4>, g, dim3(kOtzSpecThreads), 0, s, t2, w, R, T.blk_off, T.blk_idx, T.pairs, (int)m, H, W, K);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_offres_tz_mix(const float2* x, float2* y, const float* K, int kind, int L, int H, int W, int slices, float scale, hipStream_t s) {
    const int G = 4 * H * W;
    if (slices < 1 || L < 1) return hipErrorInvalidValue;
    if (kind == 1) {
        if (L <= 4) return launch_mix<4, true>(x, y, K, L, G, slices, scale, s);
        if (L <= 16) return launch_mix<16, true>(x, y, K, L, G, slices, scale, s);
        if (L <= 32) return launch_mix<32, true>(x, y, K, L, G, slices, scale, s);
    } else if (kind == 2) {
        if (L <= 4) return launch_mix<4, false>(x, y, K, L, G, slices, scale, s);
        if (L <= 8) return launch_mix<8, false>(x, y, K, L, G, slices, scale, s);
        if (L <= 16) return launch_mix<16, false>(x, y, K, L, G, slices, scale, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace pnp
