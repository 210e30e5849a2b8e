// Off-resonance correction for multi-coil data (include/pnpadmm_offres_mc.h): the two pointwise kernels that join the coil maps S_c of the
// non-Cartesian SENSE stage and the segment maps E_l of the time-segmented operator around the engine's centred grid transform.  A BLOCK of
// cbc coils x sb segments of every slice is in flight at a time: grids [N, cbc, sb, gh, gw], plane ((n cbc + j) sb + k).  Between the two
// kernels run the existing launches of offres_kernels.hip / offres_ls_kernels.hip at batch N cbc, whose indexing is exactly this layout.
//
//   forward   offres_mc_pad_kernel    grid[n, j, k] = zero-padded (cy cx) . (E_(l0+k) . (S_(c0+j) . p)): p, the cbc coil values and the sb
//                                     segment values read once per pixel, cbc sb planes written; no coil image [N, C, h, w] exists
//   adjoint   offres_mc_crop_kernel   a_j (+)= sum_k conj(E_(l0+k)) . ((cy cx) . crop(grid[n, j, k])), the chain of the single-coil adjoint,
//                                     carried from segment block to segment block through a small scratch [N, cbc, h, w]; on the last
//                                     segment block q (+)= sum_j conj(S_(c0+j)) . a_j, the SENSE combine chain carried from coil block to
//                                     coil block through q; the last coil block adds mu p and leaves the partial sums of Re<p, q>
//
// Every expression is written in the header's order and this unit is compiled without contraction.  Both kernels are memory-bound: what they
// are for is the bytes they do not move.  No atomics, no cross-workgroup waits; the block sizes change no bit (a float32 partial stored and
// reloaded is the same float32).
#include "pnp_internal.h"
#include "block_reduce.h"
#include "nufft_plan.h"

#pragma clang fp contract(off)

namespace pnp {

namespace {

constexpr int kOmThreads = 256;
constexpr int kOmPer = kPixelChunk / kOmThreads;          // pixels per thread of the chunked crop kernel: ncsense_crop_kernel's ranges
static_assert(kPixelChunk % kOmThreads == 0, "whole pixels per thread");
constexpr int kOmSub = 4;                                  // coils held in registers at a time (the default coil block).  A block of more
                                                           // coils (PNP_OFFRES_MC_COIL_BLOCK > 4) re-reads E_l once per sub-block of 4: "each
                                                           // value once per pixel per block" holds for blocks of up to 4 coils

__device__ __forceinline__ bool stopped(const float* tact, int n) { return tact != nullptr && tact[n] > 0.5f; }
// the maps of slice n: [C, HW] shared (maps_n == 1) or [N, C, HW]
__device__ __forceinline__ const float2* maps_of(const float2* maps, int maps_n, int n, int C, int HW) {
    return maps + (size_t)(maps_n == 1 ? 0 : n) * C * HW;
}
// a . b as ncsense_pad_kernel writes a complex product: four products rounded, then the difference and the sum
__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
    const float p = a.x * b.x, q = a.y * b.y, r = a.x * b.y, t = a.y * b.x;
    return make_float2(p - q, r + t);
}
// acc += conj(m) . a: ncsense_crop_kernel's four fmas
__device__ __forceinline__ void conj_fma(float2& acc, float2 m, float ax, float ay) {
    acc.x = fmaf(m.x, ax, acc.x);
    acc.x = fmaf(m.y, ay, acc.x);
    acc.y = fmaf(m.x, ay, acc.y);
    acc.y = fmaf(-m.y, ax, acc.y);
}

// grid[(n cbc + j) sb + k][gy][gx] = inside the centred h x w window ? (cy[iy] cx[ix]) (E_(l0+k) . (S_(c0+j) . src[n]))[iy][ix] : 0;
// src complex, or a real image (REAL)
template <bool REAL>
__global__ __launch_bounds__(kOmThreads) void offres_mc_pad_kernel(const void* __restrict__ src, const float2* __restrict__ sens, int sens_n, int C,
                                                                   int c0, int cbc, const float2* __restrict__ maps, int map_n, int L, int l0,
                                                                   int sb, const float* __restrict__ cy, const float* __restrict__ cx,
                                                                   float2* __restrict__ grid, int H, int W, int gh, int gw) {
    const int n = blockIdx.y, HW = H * W;
    const size_t G = (size_t)gh * gw;
    const int g = blockIdx.x * kOmThreads + threadIdx.x;
    if ((size_t)g >= G) return;
    const int gy = g / gw, gx = g - gy * gw;
    const int iy = gy - (gh / 2 - H / 2), ix = gx - (gw / 2 - W / 2);
    float2* out = grid + (size_t)n * cbc * sb * G + g;
    if (!(iy >= 0 && iy < H && ix >= 0 && ix < W)) {
        for (int j = 0; j < cbc * sb; ++j) out[(size_t)j * G] = make_float2(0.f, 0.f);
        return;
    }
    const int p = iy * W + ix;
    const float f = cy[iy] * cx[ix];
    const float2* sp = maps_of(sens, sens_n, n, C, HW) + (size_t)c0 * HW + p;
    const float2* ep = maps_of(maps, map_n, n, L, HW) + (size_t)l0 * HW + p;
    float2 pv = make_float2(0.f, 0.f);
    if (REAL) pv.x = static_cast<const float*>(src)[(size_t)n * HW + p];
    else pv = static_cast<const float2*>(src)[(size_t)n * HW + p];
    for (int j0 = 0; j0 < cbc; j0 += kOmSub) {
        float2 u[kOmSub];
#pragma unroll
        for (int jj = 0; jj < kOmSub; ++jj) {
            u[jj] = make_float2(0.f, 0.f);
            if (j0 + jj < cbc) {
                const float2 sv = sp[(size_t)(j0 + jj) * HW];
                u[jj] = REAL ? make_float2(sv.x * pv.x, sv.y * pv.x) : cmul(sv, pv);
            }
        }
        for (int k = 0; k < sb; ++k) {
            const float2 ev = ep[(size_t)k * HW];
#pragma unroll
            for (int jj = 0; jj < kOmSub; ++jj) {
                if (j0 + jj < cbc) {
                    const float2 v = cmul(ev, u[jj]);
                    out[((size_t)(j0 + jj) * sb + k) * G] = make_float2(v.x * f, v.y * f);
                }
            }
        }
    }
}

// Per pixel and coil j < cbc:  a_j = (first_seg ? +0 : part[n cbc + j][p]);  per segment k < sb:  a_j += conj(E_(l0+k)) . ((cy cx) grid[..][window]);
// not last_seg: part[n cbc + j][p] = a_j.  last_seg: acc = (first_coil ? +0 : q[n][p]);  acc += conj(S_(c0+j)) . a_j over ascending j;
// last_coil: q = acc (+ mu[n] pv when pv != nullptr), partial[n, chunk, 0] = sum over the chunk of Re(conj(pv) q): ncsense_crop_kernel's
// ranges and tree.
__global__ __launch_bounds__(kOmThreads) void offres_mc_crop_kernel(const float2* __restrict__ grid, const float2* __restrict__ sens, int sens_n,
                                                                    int C, int c0, int cbc, const float2* __restrict__ maps, int map_n, int L,
                                                                    int l0, int sb, int first_coil, int last_coil, int first_seg, int last_seg,
                                                                    const float* __restrict__ cy, const float* __restrict__ cx, float2* part,
                                                                    const float2* __restrict__ pv, const float* __restrict__ mu,
                                                                    const float* __restrict__ tact, float2* q, double* __restrict__ partial, int H,
                                                                    int W, int gh, int gw) {
    __shared__ double red[kOmThreads / 64];
    const int n = blockIdx.y, HW = H * W;
    if (stopped(tact, n)) return;
    const int p0 = blockIdx.x * kPixelChunk + threadIdx.x;
    const size_t base = (size_t)n * HW, G = (size_t)gh * gw;
    const float2* gn = grid + (size_t)n * cbc * sb * G;
    const float2* sn = maps_of(sens, sens_n, n, C, HW) + (size_t)c0 * HW;
    const float2* en = maps_of(maps, map_n, n, L, HW) + (size_t)l0 * HW;
    float2* pn = part + (size_t)n * cbc * HW;
    const int oy = gh / 2 - H / 2, ox = gw / 2 - W / 2;
    const bool epi = last_seg && last_coil && pv != nullptr && mu != nullptr;
    const float m = epi ? mu[n] : 0.f;
    double dot[1] = {0.0};
#pragma unroll
    for (int t = 0; t < kOmPer; ++t) {
        const int p = p0 + t * kOmThreads;
        if (p < HW) {
            const int iy = p / W, ix = p - iy * W;
            const float f = cy[iy] * cx[ix];
            const size_t go = (size_t)(iy + oy) * gw + (ix + ox);
            float2 acc = make_float2(0.f, 0.f);
            if (last_seg && !first_coil) acc = q[base + p];
            for (int j0 = 0; j0 < cbc; j0 += kOmSub) {
                float2 a[kOmSub];
#pragma unroll
                for (int jj = 0; jj < kOmSub; ++jj) {
                    a[jj] = make_float2(0.f, 0.f);
                    if (!first_seg && j0 + jj < cbc) a[jj] = pn[(size_t)(j0 + jj) * HW + p];
                }
                for (int k = 0; k < sb; ++k) {
                    const float2 ev = en[(size_t)k * HW + p];
#pragma unroll
                    for (int jj = 0; jj < kOmSub; ++jj) {
                        if (j0 + jj < cbc) {
                            const float2 g = gn[((size_t)(j0 + jj) * sb + k) * G + go];
                            conj_fma(a[jj], ev, g.x * f, g.y * f);
                        }
                    }
                }
#pragma unroll
                for (int jj = 0; jj < kOmSub; ++jj) {
                    if (j0 + jj < cbc) {
                        if (last_seg) conj_fma(acc, sn[(size_t)(j0 + jj) * HW + p], a[jj].x, a[jj].y);
                        else pn[(size_t)(j0 + jj) * HW + p] = a[jj];
                    }
                }
            }
            if (last_seg) {
                if (epi) {
                    const float2 pp = pv[base + p];
                    acc.x = fmaf(m, pp.x, acc.x);
                    acc.y = fmaf(m, pp.y, acc.y);
                    dot[0] += (double)pp.x * (double)acc.x + (double)pp.y * (double)acc.y;
                }
                q[base + p] = acc;
            }
        }
    }
    if (!epi || partial == nullptr) return;                // (uniform)
    block_sums_fixed<kOmThreads, 1>(dot, red);
    if (threadIdx.x == 0) partial[((size_t)n * gridDim.x + blockIdx.x) * 2] = dot[0];
}

}  // namespace

hipError_t launch_offres_mc_pad(const float2* src, const float* src_real, const float2* sens, int sens_n, int C, int c0, int cbc, const float2* maps,
                                int map_n, int L, int l0, int sb, const NufftDev& P, float2* grid, int batch, hipStream_t s) {
    const dim3 g((unsigned)((P.gh * P.gw + kOmThreads - 1) / kOmThreads), (unsigned)batch);
    if (src_real != nullptr)
        hipLaunchKernelGGL(offres_mc_pad_kernel<true>, g, dim3(kOmThreads), 0, s, (const void*)src_real, sens, sens_n, C, c0, cbc, maps, map_n, L, l0,
                           sb, P.cy, P.cx, grid, P.h, P.w, P.gh, P.gw);
    else
        hipLaunchKernelGGL(offres_mc_pad_kernel<false>, g, dim3(kOmThreads), 0, s, (const void*)src, sens, sens_n, C, c0, cbc, maps, map_n, L, l0, sb,
                           P.cy, P.cx, grid, P.h, P.w, P.gh, P.gw);
    return hipGetLastError();
}

hipError_t launch_offres_mc_crop(const float2* grid, const float2* sens, int sens_n, int C, int c0, int cbc, const float2* maps, int map_n, int L,
                                 int l0, int sb, const NufftDev& P, float2* part, const float2* pv, const float* mu, const float* tact, float2* q,
                                 double* partial, int batch, hipStream_t s) {
    hipLaunchKernelGGL(offres_mc_crop_kernel, dim3((unsigned)pixel_chunks(P.h, P.w), (unsigned)batch), dim3(kOmThreads), 0, s, grid, sens, sens_n, C,
                       c0, cbc, maps, map_n, L, l0, sb, c0 == 0 ? 1 : 0, c0 + cbc == C ? 1 : 0, l0 == 0 ? 1 : 0, l0 + sb == L ? 1 : 0, P.cy, P.cx,
                       part, pv, mu, tact, q, partial, P.h, P.w, P.gh, P.gw);
    return hipGetLastError();
}

}  // namespace pnp
