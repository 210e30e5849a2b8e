// Coil noise pre-whitening (pnp_noise_cov / pnp_whiten_matrix / pnp_whiten_apply): the channel noise covariance of a noise-only scan, its
// Cholesky factor and the inverse of that factor, and the triangular channel mix that makes the noise white and equal across channels
//     Psi[a][b] = (1 / S) sum_s n_a[s] conj(n_b[s])        Psi = L L^H        W = L^-1        out[v] = sum_{c <= v} W[v][c] in[c]
//
//   prewhiten_cov_kernel     grid (chunks, noise_n): samples [g * per, (g + 1) * per) of one scan, per = gram_chunk_len(S), walked IN ORDER by
//                            gram_partial (hermitian.h)
//   prewhiten_cov_sum_kernel Psi = (the chunks' partials summed in chunk order) / S, one division, mirrored (gram_chunk_sum, hermitian.h)
//   prewhiten_chol_kernel    grid (psi_n), one workgroup per matrix, L and W in LDS (2 * 16 C (C | 1) bytes: the row stride is odd, so a column
//                            walk does not stay on one bank), float64.  Column j of L, left-looking: thread i >= j sums
//                            s = sum_{k < j} L[i][k] conj(L[j][k]), k ascending from 0.0; thread j tests the pivot d = Re Psi[j][j] - Re s and stores
//                            sqrt(d); after the barrier thread i > j stores (Psi[i][j] - s) / L[j][j].  A pivot that is not finite or not
//                            above kPivotEps * max_i Re Psi[i][i] ends the factorisation: info = j + 1, W = L = identity.  Then thread j owns
//                            column j of W: W[j][j] = 1 / L[j][j], W[i][j] = -(sum_{k = j}^{i - 1} L[i][k] W[k][j]) / L[i][i], i and k ascending.
//                            One rounding to float32, the strict upper triangle +0.
//   prewhiten_apply_kernel   grid (pixel_chunks, N): a workgroup owns kPixelChunk pixels of one slice, stages the lower triangle of the matrix
//                            in LDS ([c][v]) and walks its pixels in passes of 256 * PPT; all CB accumulators of a pixel stay in registers
//                            (CB = C rounded up to a multiple of 8, with PPT = 4, 2, 1 pixels per thread at CB = 8, 16, above).  A thread reads the C inputs of its pixels, coil
//                            after coil, and stores its rows only after the last read: out may be in.  Per pixel and v, from re = im = +0,
//                            c ascending over c <= v only (the guard is uniform: a scalar branch, no lane diverges):
//                                re = fma(a.x, x.x, re); re = fma(-a.y, x.y, re); im = fma(a.x, x.y, im); im = fma(a.y, x.x, im)
// No atomics anywhere: a matrix's or slice's bits depend on its own input only.
#include "pnp_internal.h"
#include "block_reduce.h"
#include "hermitian.h"
#include "../../include/pnpadmm.h"

namespace pnp {

namespace {

constexpr int kPwThreads = 256;
constexpr int kPwMax = PNP_PW_MAX_COILS;
constexpr int kCovTile = 32;                                    // samples staged at a time
static_assert(kPwMax <= kPwThreads, "a thread per row of the factorisation");
constexpr double kPivotEps = 1e-12;

// grid (chunks, noise_n); partial[n][g][a * C + b], b <= a
__global__ __launch_bounds__(kPwThreads) void prewhiten_cov_kernel(const float2* __restrict__ noise, int C, int S, int per,
                                                                   double2* __restrict__ partial) {
    const int n = blockIdx.y, g = blockIdx.x;
    const long long first = (long long)g * per;
    const int last = (int)min((long long)S, first + per);
    const auto load = [&](int c, int i) { return noise[((size_t)n * C + c) * (size_t)S + (size_t)i]; };
    gram_partial<kPwThreads, kPwMax, kCovTile>(C, (int)first, last, load, partial + ((size_t)n * gridDim.x + g) * C * C);
}

// grid (ceil(C * C / threads), noise_n); psi[n][a][b] = (sum of the chunks' partials in chunk order) / S
__global__ __launch_bounds__(kPwThreads) void prewhiten_cov_sum_kernel(const double2* __restrict__ partial, int chunks, int C, int S,
                                                                       double2* __restrict__ psi) {
    const int n = blockIdx.y;
    gram_chunk_sum<kPwThreads, true>(partial + (size_t)n * chunks * C * C, chunks, C, (double)S, psi + (size_t)n * C * C);
}

// grid (psi_n); LDS: L [C][ld] double2, W [C][ld] double2, ld = C | 1
__global__ __launch_bounds__(kPwThreads) void prewhiten_chol_kernel(const double2* __restrict__ psi, int C, float2* __restrict__ wmat,
                                                                    float2* __restrict__ lmat, int* __restrict__ info) {
    extern __shared__ double2 pw_lds[];
    __shared__ double diag[kPwMax];
    __shared__ int bad;                                           // 0, or j + 1 of the first refused pivot
    const int ld = C | 1, n = blockIdx.x, tid = threadIdx.x;
    double2* L = pw_lds;
    double2* Wm = pw_lds + C * ld;
    const double2* P = psi + (size_t)n * C * C;
    // the lower triangle and the real part of the diagonal only; everything else of L and W starts as zero
    for (int idx = tid; idx < C * C; idx += kPwThreads) {
        const int r = idx / C, c = idx - r * C;
        double2 v = make_double2(0.0, 0.0);
        if (c < r) v = P[idx];
        else if (c == r) v.x = P[idx].x;
        L[r * ld + c] = v;
        Wm[r * ld + c] = make_double2(0.0, 0.0);
    }
    if (tid == 0) bad = 0;
    __syncthreads();
    if (tid == 0) {
        double m = L[0].x;
        for (int i = 1; i < C; ++i) m = fmax(m, L[i * ld + i].x);   // fmax drops a NaN; a NaN diagonal is caught as its own pivot
        diag[0] = kPivotEps * m;
    }
    __syncthreads();
    const double floor_ = diag[0];
    __syncthreads();
    for (int j = 0; j < C; ++j) {
        double2 s = make_double2(0.0, 0.0);
        const int i = tid;
        if (i >= j && i < C) {
            for (int k = 0; k < j; ++k) {
                const double2 a = L[i * ld + k], b = L[j * ld + k];
                s.x += a.x * b.x;
                s.x += a.y * b.y;
                s.y += a.y * b.x;
                s.y -= a.x * b.y;
            }
        }
        if (i == j) {
            const double d = L[j * ld + j].x - s.x;
            if (!(d > floor_) || !(d > 0.0) || !(d <= 1.7976931348623157e308)) {    // NaN fails the first test, +inf the last
                bad = j + 1;
            } else {
                const double r = sqrt(d);
                L[j * ld + j] = make_double2(r, 0.0);
                diag[j] = r;
            }
        }
        __syncthreads();
        if (bad) break;
        if (i > j && i < C) {
            const double2 p = L[i * ld + j];
            const double r = diag[j];
            L[i * ld + j] = make_double2((p.x - s.x) / r, (p.y - s.y) / r);
        }
        __syncthreads();
    }
    const int failed = bad;
    if (!failed && tid < C) {
        const int j = tid;
        Wm[j * ld + j] = make_double2(1.0 / diag[j], 0.0);
        for (int i = j + 1; i < C; ++i) {
            double2 s = make_double2(0.0, 0.0);
            for (int k = j; k < i; ++k) {
                const double2 a = L[i * ld + k], b = Wm[k * ld + j];
                s.x += a.x * b.x;
                s.x -= a.y * b.y;
                s.y += a.x * b.y;
                s.y += a.y * b.x;
            }
            const double r = diag[i];
            Wm[i * ld + j] = make_double2(-s.x / r, -s.y / r);
        }
    }
    __syncthreads();
    if (tid == 0) info[n] = failed;
    // one rounding; x + 0.0: a zero comes out as +0
    for (int idx = tid; idx < C * C; idx += kPwThreads) {
        const int r = idx / C, c = idx - r * C;
        float2 w = make_float2(r == c ? 1.f : 0.f, 0.f), l = w;
        if (!failed && c <= r) {
            const double2 a = Wm[r * ld + c], b = L[r * ld + c];
            w = make_float2((float)(a.x + 0.0), (float)(a.y + 0.0));
            l = make_float2((float)(b.x + 0.0), (float)(b.y + 0.0));
        }
        wmat[(size_t)n * C * C + idx] = w;
        if (lmat) lmat[(size_t)n * C * C + idx] = l;
    }
}

// grid (pixel_chunks, N); out[n, v, p] = sum_{c <= v} wmat[n or 0][v][c] in[n, c, p]; in and out are not __restrict__: they may be one buffer
template <int CB>
__global__ __launch_bounds__(kPwThreads) void prewhiten_apply_kernel(const float2* in, const float2* __restrict__ wmat, int wmat_n, int C,
                                                                     float2* out, int HW) {
    constexpr int PPT = CB > 16 ? 1 : CB > 8 ? 2 : 4;
    static_assert(kPixelChunk % (kPwThreads * PPT) == 0, "whole passes per chunk");
    __shared__ float2 A[CB * CB];                                // [c][v], read for c <= v < C only
    const int n = blockIdx.y;
    const float2* M = wmat + (wmat_n > 1 ? (size_t)n * C * C : 0);
    for (int idx = threadIdx.x; idx < C * CB; idx += kPwThreads) {
        const int c = idx / CB, v = idx - c * CB;
        if (v >= c) A[idx] = v < C ? M[v * C + c] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    const float2* src = in + (size_t)n * C * HW;
    float2* dst = out + (size_t)n * C * HW;
    for (int pass = 0; pass < kPixelChunk / (kPwThreads * PPT); ++pass) {
        const int p0 = blockIdx.x * kPixelChunk + pass * (kPwThreads * PPT) + threadIdx.x;
        if (p0 >= HW) break;
        float re[PPT][CB], im[PPT][CB];
#pragma unroll
        for (int i = 0; i < PPT; ++i)
#pragma unroll
            for (int v = 0; v < CB; ++v) re[i][v] = im[i][v] = 0.f;
        float2 x[PPT], nx[PPT];
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const int p = p0 + i * kPwThreads;
            nx[i] = p < HW ? src[p] : make_float2(0.f, 0.f);
        }
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int i = 0; i < PPT; ++i) x[i] = nx[i];
            if (c + 1 < C) {
#pragma unroll
                for (int i = 0; i < PPT; ++i) {
                    const int p = p0 + i * kPwThreads;
                    if (p < HW) nx[i] = src[(size_t)(c + 1) * HW + p];
                }
            }
            // rows c .. CB - 1 take coil c; the guard is uniform, a scalar branch (the rows from C to CB - 1, fewer than 8, see staged zeros
            // and are never stored)
#pragma unroll
            for (int v = 0; v < CB; ++v) {
                if (v < c) continue;
                const float2 a = A[c * CB + v];
#pragma unroll
                for (int i = 0; i < PPT; ++i) {
                    re[i][v] = fmaf(a.x, x[i].x, re[i][v]);
                    re[i][v] = fmaf(-a.y, x[i].y, re[i][v]);
                    im[i][v] = fmaf(a.x, x[i].y, im[i][v]);
                    im[i][v] = fmaf(a.y, x[i].x, im[i][v]);
                }
            }
        }
        // every read of this thread's pixels is behind it: the stores may land on the input planes
        float2* d = dst + p0;
#pragma unroll
        for (int v = 0; v < CB; ++v) {
            if (v >= CB - 7 && v >= C) break;                    // CB - 8 < C <= CB
#pragma unroll
            for (int i = 0; i < PPT; ++i)
                if (p0 + i * kPwThreads < HW) d[i * kPwThreads] = make_float2(re[i][v], im[i][v]);
            d += HW;
        }
    }
}

}  // namespace

hipError_t launch_prewhiten_cov(const float2* noise, int noise_n, int C, int S, double2* partial, double2* psi, hipStream_t s) {
    const int chunks = gram_chunks(S);
    hipLaunchKernelGGL(prewhiten_cov_kernel, dim3(chunks, noise_n), dim3(kPwThreads), 0, s, noise, C, S, gram_chunk_len(S), partial);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(prewhiten_cov_sum_kernel, dim3((C * C + kPwThreads - 1) / kPwThreads, noise_n), dim3(kPwThreads), 0, s, partial, chunks, C,
                       S, psi);
    return hipGetLastError();
}

hipError_t launch_prewhiten_chol(const double2* psi, int psi_n, int C, float2* wmat, float2* lmat, int* info, hipStream_t s) {
    const int lds = 2 * C * (C | 1) * (int)sizeof(double2);
    static DeviceOnce once;                                       // 130 KB of dynamic LDS at C = 64: raise the kernel's cap once per device
    constexpr int cap = 2 * kPwMax * (kPwMax | 1) * (int)sizeof(double2);
    if (hipError_t e = raise_lds_cap((const void*)prewhiten_chol_kernel, cap, once); e != hipSuccess) return e;
    hipLaunchKernelGGL(prewhiten_chol_kernel, dim3(psi_n), dim3(kPwThreads), lds, s, psi, C, wmat, lmat, info);
    return hipGetLastError();
}

hipError_t launch_prewhiten_apply(const float2* in, const float2* wmat, int wmat_n, int C, float2* out, int N, int H, int W, hipStream_t s) {
    const dim3 grid((unsigned)pixel_chunks(H, W), (unsigned)N);
#define PW_LAUNCH(CB) \
    case CB / 8: hipLaunchKernelGGL(prewhiten_apply_kernel<CB>, grid, dim3(kPwThreads), 0, s, in, wmat, wmat_n, C, out, H * W); break;
    switch ((C + 7) / 8) {                                        // the bucket: C rounded up to a multiple of 8
        PW_LAUNCH(8) PW_LAUNCH(16) PW_LAUNCH(24) PW_LAUNCH(32) PW_LAUNCH(40) PW_LAUNCH(48) PW_LAUNCH(56) PW_LAUNCH(64)
        default: return hipErrorInvalidValue;
    }
#undef PW_LAUNCH
    return hipGetLastError();
}

}  // namespace pnp
