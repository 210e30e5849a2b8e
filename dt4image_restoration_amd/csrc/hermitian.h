// The Hermitian pieces shared by the coil calibration chain (coilcomp_kernels.hip, prewhiten_kernels.hip, espirit_kernels.hip), float64, no
// atomics anywhere: the bits of a result depend on its own input only.  Each piece is stated here once; the units describe what they compute.
//
//   gram_partial             the Gram partial of one chunk: G[a][b] = sum over samples i in [first, last) of x_a[i] conj(x_b[i]), where
//                            load(c, i) returns sample i of channel c (float32).  The samples are staged TILE at a time through LDS
//                            ([sample][channel]); every thread owns up to MAXC^2 / THREADS entries (a, b), b <= a, and walks the samples IN ORDER:
//                                re += ar br; re += ai bi; im += ai br; im -= ar bi
//                            with the float32 values widened to float64 (their products are exact in float64).  The chunk rule that deals a
//                            count of samples to workgroups is gram_chunk_len / gram_chunks (pnp_internal.h).
//   gram_chunk_sum           G[a][b] = partial[0] + partial[1] + ... in chunk order from 0.0, then (DIVIDE) ONE float64 division per component
//                            by `divisor`; G[b][a] = conj, the diagonal's imaginary part 0.  Without DIVIDE the sum is stored as it stands.
//   jacobi_sweeps            the cyclic Jacobi method for a Hermitian G of even order n (leading dimension n): n - 1 rounds per sweep of n / 2
//                            disjoint rotations each (round-robin, rr_pair: round r pairs (r, n - 1) and ((r + k) mod (n - 1),
//                            (r - k) mod (n - 1)), k = 1 .. n / 2 - 1).  A round has two phases with a barrier after each: the n / 2 rotations from
//                            the diagonal blocks; then the blocks (pair k, pair l), k > l, B <- Jk^H B Jl, mirrored, so that G stays exactly
//                            Hermitian, and the vectors <- vectors J.  Before each sweep the whole workgroup evaluates
//                            off(G)_F^2 <= (kJacobiEps * trace)^2 by the fixed tree (block_reduce.h) and stops on it; at most SWEEPS sweeps.
//                            The eigenvalues end on G's diagonal.
// The rotation of a pair (p, q), p < q, with beta = G[p][q] != 0 (an exactly zero beta is skipped):
//     tau = (G[q][q] - G[p][p]) / (2 |beta|)     t = sgn(tau) / (|tau| + hypot(1, tau))     c = 1 / sqrt(1 + t^2)     sigma = t c beta / |beta|
//     J = [[c, sigma], [-conj(sigma), c]] on (p, q);  G <- J^H G J, vectors <- vectors J;  G[p][p] -= t |beta|, G[q][q] += t |beta|, G[p][q] = 0
// |beta| and hypot(1, tau) are overflow-safe: a vanishing beta gives tau = inf, t = 0, the identity.
#pragma once
#include <hip/hip_runtime.h>
#include "block_reduce.h"

namespace pnp {

__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 cmulc(double2 a, double2 b) { return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }   // a conj(b)
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cscale(double s, double2 a) { return make_double2(s * a.x, s * a.y); }
__device__ __forceinline__ double2 cconj(double2 a) { return make_double2(a.x, -a.y); }

// grid (chunks, ...): the calling workgroup's partial, out[a * C + b], b <= a, of samples [first, last)
template <int THREADS, int MAXC, int TILE, class Load>
__device__ __forceinline__ void gram_partial(int C, int first, int last, Load load, double2* __restrict__ out) {
    constexpr int ENT = MAXC * MAXC / THREADS;                   // entries per thread at the most
    static_assert(MAXC * MAXC % THREADS == 0, "whole entries per thread");
    __shared__ float2 tile[TILE * MAXC];                         // [sample][channel]
    int ea[ENT], eb[ENT];
    bool on[ENT];
    double re[ENT], im[ENT];
#pragma unroll
    for (int e = 0; e < ENT; ++e) {
        const int idx = e * THREADS + threadIdx.x;
        ea[e] = idx / C;
        eb[e] = idx - ea[e] * C;
        on[e] = idx < C * C && eb[e] <= ea[e];
        re[e] = 0.0;
        im[e] = 0.0;
    }
    for (int t0 = first; t0 < last; t0 += TILE) {
        const int nb = min(TILE, last - t0);
        __syncthreads();
        for (int idx = threadIdx.x; idx < TILE * C; idx += THREADS) {
            const int c = idx / TILE, b = idx - c * TILE;
            if (b < nb) tile[b * C + c] = load(c, t0 + b);
        }
        __syncthreads();
        for (int b = 0; b < nb; ++b) {
#pragma unroll
            for (int e = 0; e < ENT; ++e) {
                if (!on[e]) continue;
                const float2 p = tile[b * C + ea[e]], q = tile[b * C + eb[e]];
                re[e] += (double)p.x * (double)q.x;
                re[e] += (double)p.y * (double)q.y;
                im[e] += (double)p.y * (double)q.x;
                im[e] -= (double)p.x * (double)q.y;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < ENT; ++e)
        if (on[e]) out[e * THREADS + threadIdx.x] = make_double2(re[e], im[e]);
}

// grid (ceil(C * C / THREADS), ...): the calling thread's entry of G from partial [chunks][C * C]
template <int THREADS, bool DIVIDE>
__device__ __forceinline__ void gram_chunk_sum(const double2* __restrict__ partial, int chunks, int C, double divisor, double2* __restrict__ G) {
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    const int a = idx / C, b = idx - a * C;
    if (idx >= C * C || b > a) return;
    double re = 0.0, im = 0.0;
    for (int g = 0; g < chunks; ++g) {
        const double2 v = partial[(size_t)g * C * C + idx];
        re += v.x;
        im += v.y;
    }
    if (DIVIDE) {
        re /= divisor;
        im /= divisor;
    }
    if (a == b) {
        G[idx] = make_double2(re, 0.0);
    } else {
        G[idx] = make_double2(re, im);
        G[b * C + a] = make_double2(re, -im);
    }
}

// pair k of round r among m + 1 = n indices, p < q
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

constexpr double kJacobiEps = 1e-14;       // off(G)_F <= kJacobiEps * trace

// One workgroup of THREADS threads; G [n][n] and the vectors V (the caller sets them to the identity) in LDS or global memory, ordered by the
// workgroup's barriers; rot: n / 2 rotations in LDS.  VT: V holds the TRANSPOSED vectors, V[col * n + row] (a rotation's two columns are two
// contiguous runs), else V[row * n + col].  Rows and columns of G past the matrix proper must be zero: they stay zero and rotate nothing.
template <int THREADS, int SWEEPS, bool VT>
__device__ __forceinline__ void jacobi_sweeps(double2* G, double2* V, int n, Rot* rot) {
    __shared__ double red[THREADS / 64];
    __shared__ double trace;
    __shared__ int stop;
    const int m = n - 1, half = n >> 1, tid = threadIdx.x;
    if (tid == 0) {
        double t = 0.0;
        for (int i = 0; i < n; ++i) t += G[i * n + i].x;
        trace = t;
    }
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        double off = 0.0;
        for (int idx = tid; idx < n * n; idx += THREADS) {
            const int r = idx / n, c = idx - r * n;
            const double2 v = G[idx];
            if (r != c) off += v.x * v.x + v.y * v.y;
        }
        off = block_sum_fixed<THREADS>(off, red);
        if (tid == 0) stop = off <= (kJacobiEps * trace) * (kJacobiEps * trace);
        __syncthreads();
        if (stop) break;
        for (int r = 0; r < m; ++r) {
            if (tid < half) {
                int p, q;
                rr_pair(tid, r, m, p, q);
                const double2 beta = G[p * n + q];
                Rot j{1.0, make_double2(0.0, 0.0)};
                if (beta.x != 0.0 || beta.y != 0.0) {
                    const double ab = hypot(beta.x, beta.y), alpha = G[p * n + p].x, gamma = G[q * n + q].x;
                    const double tau = (gamma - alpha) / (2.0 * ab);
                    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + hypot(1.0, tau));
                    j.c = 1.0 / sqrt(1.0 + t * t);
                    const double s = t * j.c;
                    j.s = make_double2(s * (beta.x / ab), s * (beta.y / ab));
                    G[p * n + p] = make_double2(alpha - t * ab, 0.0);
                    G[q * n + q] = make_double2(gamma + t * ab, 0.0);
                    G[p * n + q] = make_double2(0.0, 0.0);
                    G[q * n + p] = make_double2(0.0, 0.0);
                }
                rot[tid] = j;
            }
            __syncthreads();
            // blocks (pair k, pair l), k > l: B <- Jk^H B Jl, mirrored; then the vectors' columns
            for (int task = tid; task < half * half; task += THREADS) {
                const int k = task / half, l = task - k * half;
                if (l >= k) continue;
                int p, q, pl, ql;
                rr_pair(k, r, m, p, q);
                rr_pair(l, r, m, pl, ql);
                const Rot jk = rot[k], jl = rot[l];
                const double2 b00 = G[p * n + pl], b01 = G[p * n + ql], b10 = G[q * n + pl], b11 = G[q * n + ql];
                // T = B Jl
                const double2 t00 = csub(cscale(jl.c, b00), cmulc(b01, jl.s)), t01 = cadd(cmul(b00, jl.s), cscale(jl.c, b01));
                const double2 t10 = csub(cscale(jl.c, b10), cmulc(b11, jl.s)), t11 = cadd(cmul(b10, jl.s), cscale(jl.c, b11));
                // N = Jk^H T,  Jk^H = [[c, -s], [conj(s), c]]
                const double2 n00 = csub(cscale(jk.c, t00), cmul(jk.s, t10)), n01 = csub(cscale(jk.c, t01), cmul(jk.s, t11));
                const double2 n10 = cadd(cmulc(t00, jk.s), cscale(jk.c, t10)), n11 = cadd(cmulc(t01, jk.s), cscale(jk.c, t11));
                G[p * n + pl] = n00; G[p * n + ql] = n01; G[q * n + pl] = n10; G[q * n + ql] = n11;
                G[pl * n + p] = cconj(n00); G[ql * n + p] = cconj(n01); G[pl * n + q] = cconj(n10); G[ql * n + q] = cconj(n11);
            }
            // a task is one (row, pair): with VT neighbouring threads take neighbouring rows of one pair, else neighbouring pairs of one row
            for (int task = tid; task < n * half; task += THREADS) {
                const int hi = task / (VT ? n : half), lo = task - hi * (VT ? n : half);
                const int k = VT ? hi : lo, row = VT ? lo : hi;
                int p, q;
                rr_pair(k, r, m, p, q);
                const Rot j = rot[k];
                const int ip = VT ? p * n + row : row * n + p, iq = VT ? q * n + row : row * n + q;
                const double2 up = V[ip], uq = V[iq];
                V[ip] = csub(cscale(j.c, up), cmulc(uq, j.s));
                V[iq] = cadd(cmul(up, j.s), cscale(j.c, uq));
            }
            __syncthreads();
        }
    }
}

}  // namespace pnp
