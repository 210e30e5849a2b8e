// Coil compression (pnp_coil_compress_matrix / pnp_coil_compress_apply): SVD virtual coils from the calibration block, per slice n
//     G[a][b] = sum over the block's bins of y_a conj(y_b)        G = U diag(lambda) U^H        cmat[v][c] = conj(U[c][v]), lambda descending
//     out[v]  = sum_c cmat[v][c] in[c]
// with the block of coilmap_kernels.hip: -acs_h/2 <= dy < acs_h/2, -acs_w/2 <= dx < acs_w/2 around the centre bin of the centred layout.
//
//   coilcomp_gram_kernel     grid (gram_chunks, N): bins [g * per, (g + 1) * per) of the block in row-major block order (i = by * acs_w + bx),
//                            per = gram_chunk_bins(acs_h * acs_w); every thread owns entries (a, b), b <= a, and walks the bins IN ORDER:
//                            re += ar br; re += ai bi; im += ai br; im -= ar bi, float64 (the products of float32 values are exact in float64)
//   coilcomp_gram_sum_kernel G[a][b] = partial[0] + partial[1] + ... in chunk order from 0.0; G[b][a] = conj, the diagonal's imaginary part 0
//   coilcomp_eig_kernel      grid (N), one workgroup per slice, G and the vectors in LDS (2 * 16 Cp^2 bytes, Cp = C rounded up to even): cyclic
//                            Jacobi in float64, Cp - 1 rounds per sweep of Cp / 2 disjoint rotations each (round-robin: round r pairs (r, Cp - 1)
//                            and ((r + k) mod (Cp - 1), (r - k) mod (Cp - 1)), k = 1 .. Cp / 2 - 1).  Before each sweep the whole workgroup
//                            evaluates off(G)_F^2 <= (kEigEps * trace)^2 by the fixed tree and stops on it; at most kEigSweeps sweeps.
//                            Then the stable descending sort of the diagonal, the phase convention and the one rounding to float32.
//   coilcomp_apply_kernel    grid (pixel_chunks, N): a workgroup owns kPixelChunk pixels of one slice, stages the matrix in LDS ([c][v], the rows
//                            past V zero) and walks its pixels in passes of 256 * PPT; all VB accumulators of a pixel stay in registers
//                            (VB = 8, 16, 32 with PPT = 4, 2, 1 pixels per thread).  Per pixel and v, from re = im = +0, c ascending:
//                                re = fma(a.x, x.x, re); re = fma(-a.y, x.y, re); im = fma(a.x, x.y, im); im = fma(a.y, x.x, im)
// The rotation of a pair (p, q), p < q, with beta = G[p][q] != 0 (an exactly zero beta is skipped):
//     tau = (G[q][q] - G[p][p]) / (2 |beta|)     t = sgn(tau) / (|tau| + hypot(1, tau))     c = 1 / sqrt(1 + t^2)     sigma = t c beta / |beta|
//     J = [[c, sigma], [-conj(sigma), c]] on (p, q);  G <- J^H G J, vectors <- vectors J;  G[p][p] -= t |beta|, G[q][q] += t |beta|, G[p][q] = 0
// |beta| and hypot(1, tau) are overflow-safe: a vanishing beta gives tau = inf, t = 0, the identity.  Blocks (pair k, pair l) of G are
// updated for k > l only and mirrored, so G stays exactly Hermitian.  No atomics anywhere: a slice's bits depend on (y[n], acs) only.
#include "pnp_internal.h"
#include "block_reduce.h"
#include "../../include/pnpadmm.h"

namespace pnp {

int gram_chunk_bins(int bins) {
    int per = (bins + kGramMaxChunks - 1) / kGramMaxChunks;
    per = (per + 31) / 32 * 32;
    return per < kGramMinBins ? kGramMinBins : per;
}
int gram_chunks(int acs_h, int acs_w) {
    const int bins = acs_h * acs_w;
    return (bins + gram_chunk_bins(bins) - 1) / gram_chunk_bins(bins);
}

namespace {

constexpr int kCcThreads = 256;
constexpr int kCcMax = PNP_CC_MAX_COILS;
constexpr int kGramTile = 32;                                   // bins staged at a time
constexpr int kGramEnt = kCcMax * kCcMax / kCcThreads;          // Gram entries per thread at the most
static_assert(kCcMax * kCcMax % kCcThreads == 0, "whole entries per thread");

constexpr int kEigSweeps = 24;          // cap; the stop test ends the cases of the test suite (C = 2 .. 64) after 1 to 8 sweeps
constexpr double kEigEps = 1e-14;       // off(G)_F <= kEigEps * trace

// grid (chunks, N); partial[n][g][a * C + b], b <= a
__global__ __launch_bounds__(kCcThreads) void coilcomp_gram_kernel(const float2* __restrict__ y, int C, int acs_h, int acs_w, int per,
                                                                   double2* __restrict__ partial, int H, int W) {
    __shared__ float2 tile[kGramTile * kCcMax];                  // [bin][coil]
    const int n = blockIdx.y, g = blockIdx.x, HW = H * W, bins = acs_h * acs_w;
    const int y0 = (H >> 1) - (acs_h >> 1), x0 = (W >> 1) - (acs_w >> 1);
    const int first = g * per, last = min(bins, first + per);
    int ea[kGramEnt], eb[kGramEnt];
    bool on[kGramEnt];
    double re[kGramEnt], im[kGramEnt];
#pragma unroll
    for (int e = 0; e < kGramEnt; ++e) {
        const int idx = e * kCcThreads + threadIdx.x;
        ea[e] = idx / C;
        eb[e] = idx - ea[e] * C;
        on[e] = idx < C * C && eb[e] <= ea[e];
        re[e] = 0.0;
        im[e] = 0.0;
    }
    for (int t0 = first; t0 < last; t0 += kGramTile) {
        const int nb = min(kGramTile, last - t0);
        __syncthreads();
        for (int idx = threadIdx.x; idx < kGramTile * C; idx += kCcThreads) {
            const int c = idx / kGramTile, b = idx - c * kGramTile;
            if (b < nb) {
                const int i = t0 + b, by = i / acs_w, bx = i - by * acs_w;
                tile[b * C + c] = y[((size_t)n * C + c) * HW + (size_t)(y0 + by) * W + (x0 + bx)];
            }
        }
        __syncthreads();
        for (int b = 0; b < nb; ++b) {
#pragma unroll
            for (int e = 0; e < kGramEnt; ++e) {
                if (!on[e]) continue;
                const float2 p = tile[b * C + ea[e]], q = tile[b * C + eb[e]];
                re[e] += (double)p.x * (double)q.x;
                re[e] += (double)p.y * (double)q.y;
                im[e] += (double)p.y * (double)q.x;
                im[e] -= (double)p.x * (double)q.y;
            }
        }
    }
    double2* out = partial + ((size_t)n * gridDim.x + g) * C * C;
#pragma unroll
    for (int e = 0; e < kGramEnt; ++e)
        if (on[e]) out[e * kCcThreads + threadIdx.x] = make_double2(re[e], im[e]);
}

// grid (ceil(C * C / threads), N); gram[n][a][b] = sum of the chunks' partials in chunk order
__global__ __launch_bounds__(kCcThreads) void coilcomp_gram_sum_kernel(const double2* __restrict__ partial, int chunks, int C,
                                                                       double2* __restrict__ gram) {
    const int n = blockIdx.y, idx = blockIdx.x * kCcThreads + threadIdx.x;
    const int a = idx / C, b = idx - a * C;
    if (idx >= C * C || b > a) return;
    double re = 0.0, im = 0.0;
    for (int g = 0; g < chunks; ++g) {
        const double2 v = partial[((size_t)n * chunks + g) * C * C + idx];
        re += v.x;
        im += v.y;
    }
    double2* G = gram + (size_t)n * C * C;
    if (a == b) {
        G[idx] = make_double2(re, 0.0);
    } else {
        G[idx] = make_double2(re, im);
        G[b * C + a] = make_double2(re, -im);
    }
}

__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 cmulc(double2 a, double2 b) { return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }   // a conj(b)
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cscale(double s, double2 a) { return make_double2(s * a.x, s * a.y); }
__device__ __forceinline__ double2 cconj(double2 a) { return make_double2(a.x, -a.y); }

// pair k of round r among m + 1 = Cp indices, p < q
__device__ __forceinline__ void rr_pair(int k, int r, int m, int& p, int& q) {
    int a = r, b = m;
    if (k) {
        a = (r + k) % m;
        b = (r - k + m) % m;
    }
    p = min(a, b);
    q = max(a, b);
}

struct Rot { double c; double2 s; };       // J = [[c, s], [-conj(s), c]]

// grid (N); LDS: G [Cp * Cp] double2, U [Cp * Cp] double2, rot [Cp / 2], then the small arrays
__global__ __launch_bounds__(kCcThreads) void coilcomp_eig_kernel(const double2* __restrict__ gram, int C, float2* __restrict__ cmat,
                                                                  float* __restrict__ eig) {
    extern __shared__ double2 cc_lds[];
    __shared__ double red[kCcThreads / 64];
    __shared__ double diag[kCcMax];
    __shared__ double2 phase[kCcMax];
    __shared__ int order[kCcMax];
    __shared__ double trace;
    __shared__ int stop;
    const int Cp = (C + 1) & ~1, m = Cp - 1, half = Cp >> 1, n = blockIdx.x, tid = threadIdx.x;
    double2* G = cc_lds;
    double2* U = cc_lds + Cp * Cp;
    Rot* rot = (Rot*)(cc_lds + 2 * Cp * Cp);
    for (int idx = tid; idx < Cp * Cp; idx += kCcThreads) {
        const int r = idx / Cp, c = idx - r * Cp;
        G[idx] = r < C && c < C ? gram[(size_t)n * C * C + r * C + c] : make_double2(0.0, 0.0);
        U[idx] = make_double2(r == c ? 1.0 : 0.0, 0.0);
    }
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int i = 0; i < C; ++i) t += G[i * Cp + i].x;
        trace = t;
    }
    for (int sweep = 0; sweep < kEigSweeps; ++sweep) {
        double off = 0.0;
        for (int idx = tid; idx < Cp * Cp; idx += kCcThreads) {
            const int r = idx / Cp, c = idx - r * Cp;
            const double2 v = G[idx];
            if (r != c) off += v.x * v.x + v.y * v.y;
        }
        off = block_sum_fixed<kCcThreads>(off, red);
        if (tid == 0) stop = off <= (kEigEps * trace) * (kEigEps * trace);
        __syncthreads();
        if (stop) break;
        for (int r = 0; r < m; ++r) {
            if (tid < half) {
                int p, q;
                rr_pair(tid, r, m, p, q);
                const double2 beta = G[p * Cp + q];
                Rot j{1.0, make_double2(0.0, 0.0)};
                if (beta.x != 0.0 || beta.y != 0.0) {
                    const double ab = hypot(beta.x, beta.y), alpha = G[p * Cp + p].x, gamma = G[q * Cp + q].x;
                    const double tau = (gamma - alpha) / (2.0 * ab);
                    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + hypot(1.0, tau));
                    j.c = 1.0 / sqrt(1.0 + t * t);
                    const double s = t * j.c;
                    j.s = make_double2(s * (beta.x / ab), s * (beta.y / ab));
                    G[p * Cp + p] = make_double2(alpha - t * ab, 0.0);
                    G[q * Cp + q] = make_double2(gamma + t * ab, 0.0);
                    G[p * Cp + q] = make_double2(0.0, 0.0);
                    G[q * Cp + p] = make_double2(0.0, 0.0);
                }
                rot[tid] = j;
            }
            __syncthreads();
            // blocks (pair k, pair l), k > l: B <- Jk^H B Jl, mirrored; then the vectors' columns
            for (int task = tid; task < half * half; task += kCcThreads) {
                const int k = task / half, l = task - k * half;
                if (l >= k) continue;
                int p, q, pl, ql;
                rr_pair(k, r, m, p, q);
                rr_pair(l, r, m, pl, ql);
                const Rot jk = rot[k], jl = rot[l];
                const double2 b00 = G[p * Cp + pl], b01 = G[p * Cp + ql], b10 = G[q * Cp + pl], b11 = G[q * Cp + ql];
                // T = B Jl
                const double2 t00 = csub(cscale(jl.c, b00), cmulc(b01, jl.s)), t01 = cadd(cmul(b00, jl.s), cscale(jl.c, b01));
                const double2 t10 = csub(cscale(jl.c, b10), cmulc(b11, jl.s)), t11 = cadd(cmul(b10, jl.s), cscale(jl.c, b11));
                // N = Jk^H T,  Jk^H = [[c, -s], [conj(s), c]]
                const double2 n00 = csub(cscale(jk.c, t00), cmul(jk.s, t10)), n01 = csub(cscale(jk.c, t01), cmul(jk.s, t11));
                const double2 n10 = cadd(cmulc(t00, jk.s), cscale(jk.c, t10)), n11 = cadd(cmulc(t01, jk.s), cscale(jk.c, t11));
                G[p * Cp + pl] = n00; G[p * Cp + ql] = n01; G[q * Cp + pl] = n10; G[q * Cp + ql] = n11;
                G[pl * Cp + p] = cconj(n00); G[ql * Cp + p] = cconj(n01); G[pl * Cp + q] = cconj(n10); G[ql * Cp + q] = cconj(n11);
            }
            for (int task = tid; task < Cp * half; task += kCcThreads) {
                const int row = task / half, k = task - row * half;
                int p, q;
                rr_pair(k, r, m, p, q);
                const Rot j = rot[k];
                const double2 up = U[row * Cp + p], uq = U[row * Cp + q];
                U[row * Cp + p] = csub(cscale(j.c, up), cmulc(uq, j.s));
                U[row * Cp + q] = cadd(cmul(up, j.s), cscale(j.c, uq));
            }
            __syncthreads();
        }
    }
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
    const int chunks = gram_chunks(acs_h, acs_w);
    hipLaunchKernelGGL(coilcomp_gram_kernel, dim3(chunks, N), dim3(kCcThreads), 0, s, y, C, acs_h, acs_w, gram_chunk_bins(acs_h * acs_w), partial,
                       H, W);
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
