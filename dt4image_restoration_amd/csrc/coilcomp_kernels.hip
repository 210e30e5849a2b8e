// Coil compression (pnp_coil_compress_matrix / pnp_coil_compress_apply): SVD virtual coils from the calibration block, per slice n
//     G[a][b] = sum over the block's bins of y_a conj(y_b)        G = U diag(lambda) U^H        cmat[v][c] = conj(U[c][v]), lambda descending
//     out[v]  = sum_c cmat[v][c] in[c]
// with the block of coilmap_kernels.hip: -acs_h/2 <= dy < acs_h/2, -acs_w/2 <= dx < acs_w/2 around the centre bin of the centred layout.
//
//   coilcomp_gram_kernel     grid (gram_chunks, N): bins [g * per, (g + 1) * per) of the block in row-major block order (i = by * acs_w + bx),
//                            per = gram_chunk_len(acs_h * acs_w), walked IN ORDER by gram_partial (hermitian.h)
//   coilcomp_gram_sum_kernel G = the chunks' partials summed in chunk order, mirrored (gram_chunk_sum, hermitian.h, no division)
//   coilcomp_eig_kernel      grid (N), one workgroup per slice, G and the vectors U[row][col] in LDS (2 * 16 Cp^2 bytes, Cp = C rounded up to
//                            even): the cyclic Jacobi method of hermitian.h (jacobi_sweeps), at most kEigSweeps sweeps.
//                            Then the stable descending sort of the diagonal, the phase convention and the one rounding to float32.
//   coilcomp_apply_kernel    grid (pixel_chunks, N): a workgroup owns kPixelChunk pixels of one slice, stages the matrix in LDS ([c][v], the rows
//                            past V zero) and walks its pixels in passes of 256 * PPT; all VB accumulators of a pixel stay in registers
//                            (VB = 8, 16, 32 with PPT = 4, 2, 1 pixels per thread).  Per pixel and v, from re = im = +0, c ascending:
//                                re = fma(a.x, x.x, re); re = fma(-a.y, x.y, re); im = fma(a.x, x.y, im); im = fma(a.y, x.x, im)
// No atomics anywhere: a slice's bits depend on (y[n], acs) only.
#include "pnp_internal.h"
#include "block_reduce.h"
#include "hermitian.h"
#include "../../include/pnpadmm.h"

namespace pnp {

namespace {

constexpr int kCcThreads = 256;
constexpr int kCcMax = PNP_CC_MAX_COILS;
constexpr int kGramTile = 32;                                   // bins staged at a time
constexpr int kEigSweeps = 24;          // cap; the stop test ends the cases of the test suite (C = 2 .. 64) after 1 to 8 sweeps

// grid (chunks, N); partial[n][g][a * C + b], b <= a
__global__ __launch_bounds__(kCcThreads) void coilcomp_gram_kernel(const float2* __restrict__ y, int C, int acs_h, int acs_w, int per,
                                                                   double2* __restrict__ partial, int H, int W) {
    const int n = blockIdx.y, g = blockIdx.x, HW = H * W, bins = acs_h * acs_w;
    const int y0 = (H >> 1) - (acs_h >> 1), x0 = (W >> 1) - (acs_w >> 1);
    const int first = g * per, last = min(bins, first + per);
    const auto load = [&](int c, int i) {                        // bin i of the block in row-major block order, coil c
        const int by = i / acs_w, bx = i - by * acs_w;
        return y[((size_t)n * C + c) * HW + (size_t)(y0 + by) * W + (x0 + bx)];
    };
    gram_partial<kCcThreads, kCcMax, kGramTile>(C, first, last, load, partial + ((size_t)n * gridDim.x + g) * C * C);
}

// grid (ceil(C * C / threads), N); gram[n][a][b] = sum of the chunks' partials in chunk order
__global__ __launch_bounds__(kCcThreads) void coilcomp_gram_sum_kernel(const double2* __restrict__ partial, int chunks, int C,
                                                                       double2* __restrict__ gram) {
    const int n = blockIdx.y;
    gram_chunk_sum<kCcThreads, false>(partial + (size_t)n * chunks * C * C, chunks, C, 1.0, gram + (size_t)n * C * C);
}

// grid (N); LDS: G [Cp * Cp] double2, U [Cp * Cp] double2, rot [Cp / 2], then the small arrays
__global__ __launch_bounds__(kCcThreads) void coilcomp_eig_kernel(const double2* __restrict__ gram, int C, float2* __restrict__ cmat,
                                                                  float* __restrict__ eig) {
    extern __shared__ double2 cc_lds[];
    __shared__ double diag[kCcMax];
    __shared__ double2 phase[kCcMax];
    __shared__ int order[kCcMax];
    const int Cp = (C + 1) & ~1, n = blockIdx.x, tid = threadIdx.x;
    double2* G = cc_lds;
    double2* U = cc_lds + Cp * Cp;
    Rot* rot = (Rot*)(cc_lds + 2 * Cp * Cp);
    for (int idx = tid; idx < Cp * Cp; idx += kCcThreads) {
        const int r = idx / Cp, c = idx - r * Cp;
        G[idx] = r < C && c < C ? gram[(size_t)n * C * C + r * C + c] : make_double2(0.0, 0.0);
        U[idx] = make_double2(r == c ? 1.0 : 0.0, 0.0);
    }
    __syncthreads();
    jacobi_sweeps<kCcThreads, kEigSweeps, false>(G, U, Cp, rot);
    // stable descending sort of the diagonal: order[rank] = index
    if (tid < C) diag[tid] = G[tid * Cp + tid].x;
    __syncthreads();
    if (tid < C) {
        const double d = diag[tid];
        int rank = 0;
        for (int j = 0; j < C; ++j) rank += diag[j] > d || (diag[j] == d && j < tid);
        order[rank] = tid;
    }
    __syncthreads();
    // the unit factor that makes a vector's entry of largest modulus (lowest index on a tie) real and positive
    if (tid < C) {
        const int col = order[tid];
        double best = -1.0;
        double2 at = make_double2(1.0, 0.0);
        for (int c = 0; c < C; ++c) {
            const double2 u = U[c * Cp + col];
            const double m2 = u.x * u.x + u.y * u.y;
            if (m2 > best) { best = m2; at = u; }
        }
        const double mod = hypot(at.x, at.y);
        phase[tid] = mod > 0.0 ? make_double2(at.x / mod, -at.y / mod) : make_double2(1.0, 0.0);
        eig[(size_t)n * C + tid] = (float)diag[col];
    }
    __syncthreads();
    for (int idx = tid; idx < C * C; idx += kCcThreads) {
        const int v = idx / C, c = idx - v * C;
        const double2 u = cmul(U[c * Cp + order[v]], phase[v]);
        cmat[(size_t)n * C * C + idx] = make_float2((float)u.x, (float)(0.0 - u.y));      // conj; 0.0 - y: a zero comes out as +0
    }
}

// grid (pixel_chunks, N); out[n, v, p] = sum_c cmat[n or 0][v][c] in[n, c, p]
template <int VB>
__global__ __launch_bounds__(kCcThreads) void coilcomp_apply_kernel(const float2* __restrict__ in, const float2* __restrict__ cmat, int cmat_n,
                                                                    int C, int V, float2* __restrict__ out, int HW) {
    constexpr int PPT = 32 / VB;
    static_assert(kPixelChunk % (kCcThreads * PPT) == 0, "whole passes per chunk");
    __shared__ float2 A[kCcMax * VB];                            // [c][v]
    const int n = blockIdx.y;
    const float2* M = cmat + (cmat_n > 1 ? (size_t)n * C * C : 0);
    for (int idx = threadIdx.x; idx < C * VB; idx += kCcThreads) {
        const int c = idx / VB, v = idx - c * VB;
        A[idx] = v < V ? M[v * C + c] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    const float2* src = in + (size_t)n * C * HW;
    float2* dst = out + (size_t)n * V * HW;
    for (int pass = 0; pass < kPixelChunk / (kCcThreads * PPT); ++pass) {
        const int p0 = blockIdx.x * kPixelChunk + pass * (kCcThreads * PPT) + threadIdx.x;
        if (p0 >= HW) break;
        float re[PPT][VB], im[PPT][VB];
#pragma unroll
        for (int i = 0; i < PPT; ++i)
#pragma unroll
            for (int v = 0; v < VB; ++v) re[i][v] = im[i][v] = 0.f;
        float2 x[PPT], nx[PPT];
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const int p = p0 + i * kCcThreads;
            nx[i] = p < HW ? src[p] : make_float2(0.f, 0.f);
        }
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int i = 0; i < PPT; ++i) x[i] = nx[i];
            if (c + 1 < C) {
#pragma unroll
                for (int i = 0; i < PPT; ++i) {
                    const int p = p0 + i * kCcThreads;
                    if (p < HW) nx[i] = src[(size_t)(c + 1) * HW + p];
                }
            }
#pragma unroll
            for (int v = 0; v < VB; ++v) {
                const float2 a = A[c * VB + v];
#pragma unroll
                for (int i = 0; i < PPT; ++i) {
                    re[i][v] = fmaf(a.x, x[i].x, re[i][v]);
                    re[i][v] = fmaf(-a.y, x[i].y, re[i][v]);
                    im[i][v] = fmaf(a.x, x[i].y, im[i][v]);
                    im[i][v] = fmaf(a.y, x[i].x, im[i][v]);
                }
            }
        }
        float2* d = dst + p0;                                    // plane v of the output, walked by pointer: no per-plane offsets kept live
#pragma unroll
        for (int v = 0; v < VB; ++v) {
            if (v >= V) break;
#pragma unroll
            for (int i = 0; i < PPT; ++i)
                if (p0 + i * kCcThreads < HW) d[i * kCcThreads] = make_float2(re[i][v], im[i][v]);
            d += HW;
        }
    }
}

}  // namespace

hipError_t launch_coilcomp_gram(const float2* y, int C, int acs_h, int acs_w, double2* partial, double2* gram, int N, int H, int W, hipStream_t s) {
    const int bins = acs_h * acs_w, chunks = gram_chunks(bins);
    hipLaunchKernelGGL(coilcomp_gram_kernel, dim3(chunks, N), dim3(kCcThreads), 0, s, y, C, acs_h, acs_w, gram_chunk_len(bins), partial, H, W);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(coilcomp_gram_sum_kernel, dim3((C * C + kCcThreads - 1) / kCcThreads, N), dim3(kCcThreads), 0, s, partial, chunks, C, gram);
    return hipGetLastError();
}

hipError_t launch_coilcomp_eig(const double2* gram, int C, float2* cmat, float* eig, int N, hipStream_t s) {
    const int Cp = (C + 1) & ~1;
    const int lds = 2 * Cp * Cp * (int)sizeof(double2) + (Cp / 2) * (int)sizeof(Rot);
    static DeviceOnce once;                                       // 129 KB of dynamic LDS at C = 64: raise the kernel's cap once per device
    constexpr int cap = 2 * kCcMax * kCcMax * (int)sizeof(double2) + (kCcMax / 2) * (int)sizeof(Rot);
    if (hipError_t e = raise_lds_cap((const void*)coilcomp_eig_kernel, cap, once); e != hipSuccess) return e;
    hipLaunchKernelGGL(coilcomp_eig_kernel, dim3(N), dim3(kCcThreads), lds, s, gram, C, cmat, eig);
    return hipGetLastError();
}

hipError_t launch_coilcomp_apply(const float2* in, const float2* cmat, int cmat_n, int C, int V, float2* out, int N, int H, int W, hipStream_t s) {
    const dim3 grid((unsigned)pixel_chunks(H, W), (unsigned)N);
    if (V <= 8)
        hipLaunchKernelGGL(coilcomp_apply_kernel<8>, grid, dim3(kCcThreads), 0, s, in, cmat, cmat_n, C, V, out, H * W);
    else if (V <= 16)
        hipLaunchKernelGGL(coilcomp_apply_kernel<16>, grid, dim3(kCcThreads), 0, s, in, cmat, cmat_n, C, V, out, H * W);
    else
        hipLaunchKernelGGL(coilcomp_apply_kernel<32>, grid, dim3(kCcThreads), 0, s, in, cmat, cmat_n, C, V, out, H * W);
    return hipGetLastError();
}

}  // namespace pnp
