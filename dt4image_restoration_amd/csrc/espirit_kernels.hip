// ESPIRiT coil sensitivity maps (pnp_espirit_sens), per slice, with the centred acs_h x acs_w block of coilmap_kernels.hip, kernel side k, C coils,
// n = C k^2 (np = n rounded up to even), D = 2 k - 1:
//     A[(wy, wx)][(a, iy, ix)] = y[a][y0 + wy + iy][x0 + wx + ix]        G = A^H A = V diag(lambda) V^H        P = V_kept V_kept^H
//     R[a][b][d] = (1 / k^2) sum over {i - j = d} of conj(P[(a, i), (b, j)])        G_q[a][b] = sum_d R[a][b][d] exp(+2 pi i (dy qy / H + dx qx / W))
//     v <- G_q v / ||G_q v|| from l / rss, lambda = Re(v^H G_q v), S_c = v_c p / |p| with p = sum_c conj(v_c) l_c, kept where lambda > crop and rss
//     passes the threshold of pnp_estimate_sens.
//
//   espirit_gram_kernel      grid (ceil(np^2 / 256), N): one thread per entry (r, c), c <= r, of the lower triangle; it walks the windows in row-major
//                            window order: re += xr yr; re += xi yi; im += xr yi; im -= xi yr (x = A[w][r], y = A[w][c]), float64 (the products of
//                            float32 values are exact), and stores the entry and its mirror; the diagonal's imaginary part is 0, the padding 0.
//   espirit_eig_kernel       grid (N), one workgroup of 1024 threads per slice; G and the TRANSPOSED vectors (Vt[col][row]: a rotation's two
//                            columns are two contiguous runs) live in the slice's global workspace, 2 x 16 np^2 bytes, and the workgroup's
//                            barriers order its accesses.  The cyclic Jacobi method of hermitian.h (jacobi_sweeps), at most kEsSweeps sweeps.
//                            The eigenvalues stay on G's diagonal.  No sort and no phase step: only the projector on the kept vectors is used.
//   espirit_kern_kernel      grid (ceil(C^2 D^2 / 256), N): every workgroup finds lambda_0 = max lambda and the kept flags lambda_j >
//                            sv_thresh^2 lambda_0 (the first one of a slice writes nkept); one thread per R[a][b][dy][dx]: the kept vectors j in index
//                            order, inside them the pairs (i, j) in (iy, ix) order: re += xr yr; re += xi yi; im += xr yi; im -= xi yr with
//                            x = V[(a, i)][j], y = V[(b, j)][j]; float64, divided by k^2, rounded to complex64 once.
//   espirit_pixel_kernel     grid (ceil(W / 256), H, N): a workgroup owns (a chunk of) one image row.  It builds exp(2 pi i dy qy / H) (D values) and
//                            the table exp(2 pi i m / W), m < W, in float64 from exactly reduced integer arguments, rounded to float32 once, contracts
//                            d_y into T[dx][a][b] (b <= a; float32, dy ascending) in LDS, and then every thread owns a pixel: G_q (its lower triangle
//                            in registers, dx ascending), `iters` power steps, the quotient, the phase and the kept rule, all float32 with every
//                            complex product-sum written as  re = fma(g.x, v.x, re); re = fma(-g.y, v.y, re); im = fma(g.x, v.y, im);
//                            im = fma(g.y, v.x, im).  The pixel's l_c is read from, and S_c written to, the caller's map buffer in place.
// No atomics anywhere: a slice's bits depend on its own inputs and the arguments only.
#include "pnp_internal.h"
#include "block_reduce.h"
#include "hermitian.h"
#include "../../include/pnpadmm.h"

namespace pnp {

namespace {

constexpr int kEsThreads = 256;
constexpr int kEsEigThreads = 1024;
constexpr int kEsSweeps = 40;           // cap; the stop test ends the cases of the test suite (n = 64 .. 288) after 11 to 13 sweeps
constexpr int kEsMaxD = 2 * PNP_ESPIRIT_MAX_KSIZE - 1;
constexpr int kEsMaxW = 1024;           // pnp_create's largest side

// grid (ceil(np^2 / 256), N); ws: per slice G [np][np] then Vt [np][np]
__global__ __launch_bounds__(kEsThreads) void espirit_gram_kernel(const float2* __restrict__ y, int C, int acs_h, int acs_w, int k, int np,
                                                                  double2* __restrict__ ws, int H, int W) {
    const int n = blockIdx.y, idx = blockIdx.x * kEsThreads + threadIdx.x;
    if (idx >= np * np) return;
    const int r = idx / np, c = idx - r * np;
    if (c > r) return;
    double2* G = ws + (size_t)n * 2 * np * np;
    const int kk = k * k, nn = C * kk;
    if (r >= nn) {
        G[r * np + c] = make_double2(0.0, 0.0);
        G[c * np + r] = make_double2(0.0, 0.0);
        return;
    }
    const int a = r / kk, iy = (r - a * kk) / k, ix = r - a * kk - iy * k;
    const int b = c / kk, jy = (c - b * kk) / k, jx = c - b * kk - jy * k;
    const int y0 = (H >> 1) - (acs_h >> 1), x0 = (W >> 1) - (acs_w >> 1);
    const size_t HW = (size_t)H * W;
    const float2* pa = y + ((size_t)n * C + a) * HW + (size_t)(y0 + iy) * W + (x0 + ix);
    const float2* pb = y + ((size_t)n * C + b) * HW + (size_t)(y0 + jy) * W + (x0 + jx);
    double re = 0.0, im = 0.0;
    for (int wy = 0; wy <= acs_h - k; ++wy)
        for (int wx = 0; wx <= acs_w - k; ++wx) {
            const float2 p = pa[wy * W + wx], q = pb[wy * W + wx];
            re += (double)p.x * (double)q.x;
            re += (double)p.y * (double)q.y;
            im += (double)p.x * (double)q.y;
            im -= (double)p.y * (double)q.x;
        }
    if (r == c) {
        G[idx] = make_double2(re, 0.0);
    } else {
        G[idx] = make_double2(re, im);
        G[c * np + r] = make_double2(re, -im);
    }
}

// grid (N); ws: per slice G [np][np] (in: the Gram matrix; out: the eigenvalues on its diagonal) then Vt [np][np] (out: Vt[j][row] = V[row][j])
__global__ __launch_bounds__(kEsEigThreads) void espirit_eig_kernel(double2* __restrict__ ws, int np) {
    __shared__ Rot rot[PNP_ESPIRIT_MAX_N / 2];
    double2* G = ws + (size_t)blockIdx.x * 2 * np * np;
    double2* Vt = G + (size_t)np * np;
    for (int idx = threadIdx.x; idx < np * np; idx += kEsEigThreads) {
        const int r = idx / np, c = idx - r * np;
        Vt[idx] = make_double2(r == c ? 1.0 : 0.0, 0.0);
    }
    jacobi_sweeps<kEsEigThreads, kEsSweeps, true>(G, Vt, np, rot);
}

// grid (ceil(C^2 D^2 / 256), N); kern[n][a][b][dy][dx], nkept[n]
__global__ __launch_bounds__(kEsThreads) void espirit_kern_kernel(const double2* __restrict__ ws, int C, int k, int np, double sv2,
                                                                  float2* __restrict__ kern, int* __restrict__ nkept) {
    __shared__ double lam[PNP_ESPIRIT_MAX_N];
    __shared__ unsigned char keep[PNP_ESPIRIT_MAX_N];
    __shared__ double cut;
    const int n = blockIdx.y, tid = threadIdx.x, D = 2 * k - 1, kk = k * k, nn = C * kk;
    const double2* G = ws + (size_t)n * 2 * np * np;
    const double2* Vt = G + (size_t)np * np;
    for (int j = tid; j < nn; j += kEsThreads) lam[j] = G[j * np + j].x;
    __syncthreads();
    if (tid == 0) {
        double top = lam[0];
        for (int j = 1; j < nn; ++j) top = fmax(top, lam[j]);
        cut = sv2 * top;
    }
    __syncthreads();
    for (int j = tid; j < nn; j += kEsThreads) keep[j] = lam[j] > cut;
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) {
        int count = 0;
        for (int j = 0; j < nn; ++j) count += keep[j];
        nkept[n] = count;
    }
    const int idx = blockIdx.x * kEsThreads + tid;
    if (idx >= C * C * D * D) return;
    const int dxi = idx % D, dyi = (idx / D) % D, b = (idx / (D * D)) % C, a = idx / (D * D * C);
    const int dy = dyi - (k - 1), dx = dxi - (k - 1);
    const int iy0 = max(0, dy), iy1 = min(k - 1, k - 1 + dy), ix0 = max(0, dx), ix1 = min(k - 1, k - 1 + dx);
    double re = 0.0, im = 0.0;
    for (int j = 0; j < nn; ++j) {
        if (!keep[j]) continue;
        const double2* col = Vt + (size_t)j * np;
        for (int iy = iy0; iy <= iy1; ++iy)
            for (int ix = ix0; ix <= ix1; ++ix) {
                const double2 x = col[a * kk + iy * k + ix], y = col[b * kk + (iy - dy) * k + (ix - dx)];
                re += x.x * y.x;
                re += x.y * y.y;
                im += x.x * y.y;
                im -= x.y * y.x;
            }
    }
    const double s = (double)kk;
    kern[(size_t)n * C * C * D * D + idx] = make_float2((float)(re / s), (float)(im / s));
}

// exp(+2 pi i m / L), 0 <= m < L, float64 rounded to float32 once
__device__ __forceinline__ float2 unit_root(int m, int L) {
    double s, c;
    sincospi(2.0 * (double)m / (double)L, &s, &c);
    return make_float2((float)c, (float)s);
}

__device__ __forceinline__ void cmac(float2& acc, float2 g, float2 v) {
    acc.x = fmaf(g.x, v.x, acc.x);
    acc.x = fmaf(-g.y, v.y, acc.x);
    acc.y = fmaf(g.x, v.y, acc.y);
    acc.y = fmaf(g.y, v.x, acc.y);
}

// w = G_q v from the lower triangle g(a (a + 1) / 2 + b), b <= a (the diagonal's real part only), b ascending
template <int CB>
__device__ __forceinline__ void gq_times(const float2 (&g)[CB * (CB + 1) / 2], const float2 (&v)[CB], float2 (&w)[CB]) {
#pragma unroll
    for (int a = 0; a < CB; ++a) {
        float2 acc = make_float2(0.f, 0.f);
#pragma unroll
        for (int b = 0; b < CB; ++b) {
            const float2 e = b <= a ? g[a * (a + 1) / 2 + b] : g[b * (b + 1) / 2 + a];
            if (b < a) cmac(acc, e, v[b]);
            else if (b == a) cmac(acc, make_float2(e.x, 0.f), v[b]);
            else cmac(acc, make_float2(e.x, -e.y), v[b]);
        }
        w[a] = acc;
    }
}

// grid (ceil(W / 256), H, N); sens: in l_c, out S_c; CB: the coil count rounded up to 8 or 16 (the coils past C are zero throughout).  The lower
// triangle of the pixel's G_q stays in registers: 36 complex entries at CB = 8 (123 VGPRs), 136 at CB = 16 (425 VGPRs, one wave per SIMD, no
// scratch; keeping them in LDS, [entry][thread], took 306 VGPRs and 94 KB of LDS: one 64-thread workgroup per CU, a quarter of the waves).
template <int CB>
__global__ __launch_bounds__(kEsThreads) void espirit_pixel_kernel(float2* __restrict__ sens, const float2* __restrict__ kern,
                                                                   const float* __restrict__ rss, const float* __restrict__ smax, int C, int k,
                                                                   int iters, float crop, float thresh, float* __restrict__ eval, int H, int W) {
    constexpr int NE = CB * (CB + 1) / 2, TPB = kEsThreads;
    __shared__ float2 T[kEsMaxD * NE];                          // [dx][entry]
    __shared__ float2 tw[kEsMaxW];
    __shared__ float2 ey[kEsMaxD];
    const int n = blockIdx.z, py = blockIdx.y, tid = threadIdx.x, D = 2 * k - 1, qy = py - (H >> 1);
    if (tid < D) ey[tid] = unit_root((((tid - (k - 1)) * qy) % H + H) % H, H);
    for (int m = tid; m < W; m += TPB) tw[m] = unit_root(m, W);
    __syncthreads();
    const float2* R = kern + (size_t)n * C * C * D * D;
    for (int idx = tid; idx < D * NE; idx += TPB) {
        const int dxi = idx / NE, e = idx - dxi * NE;
        int a = 0;
        while ((a + 1) * (a + 2) / 2 <= e) ++a;
        const int b = e - a * (a + 1) / 2;
        float2 acc = make_float2(0.f, 0.f);
        if (a < C)
            for (int dyi = 0; dyi < D; ++dyi) cmac(acc, R[((a * C + b) * D + dyi) * D + dxi], ey[dyi]);
        T[idx] = acc;
    }
    __syncthreads();
    const int px = blockIdx.x * TPB + tid;
    if (px >= W) return;
    const int qx = px - (W >> 1), m1 = (qx % W + W) % W, m0 = ((-(k - 1) * qx) % W + W) % W;
    float2 g[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) g[e] = make_float2(0.f, 0.f);
    int m = m0;
    for (int dxi = 0; dxi < D; ++dxi) {
        const float2 ex = tw[m];
        const float2* t = T + dxi * NE;
#pragma unroll
        for (int e = 0; e < NE; ++e) cmac(g[e], t[e], ex);
        m += m1;
        m -= m >= W ? W : 0;
    }
    const size_t HW = (size_t)H * W, pix = (size_t)py * W + px;
    float2* lc = sens + (size_t)n * C * HW + pix;
    const float r = rss[(size_t)n * HW + pix];
    float2 v[CB], w[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) {
        v[c] = make_float2(0.f, 0.f);
        if (c < C && r > 0.f) {
            const float2 l = lc[c * HW];
            v[c] = make_float2(l.x / r, l.y / r);
        }
    }
    for (int it = 0; it < iters; ++it) {
        gq_times<CB>(g, v, w);
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < CB; ++c) {
            ss = fmaf(w[c].x, w[c].x, ss);
            ss = fmaf(w[c].y, w[c].y, ss);
        }
        const float nrm = sqrtf(ss), inv = nrm > 0.f ? 1.f / nrm : 0.f;
#pragma unroll
        for (int c = 0; c < CB; ++c) v[c] = make_float2(w[c].x * inv, w[c].y * inv);
    }
    gq_times<CB>(g, v, w);
    float lam = 0.f;
    float2 p = make_float2(0.f, 0.f);
#pragma unroll
    for (int c = 0; c < CB; ++c) {
        lam = fmaf(v[c].x, w[c].x, lam);
        lam = fmaf(v[c].y, w[c].y, lam);
        if (c < C) cmac(p, lc[c * HW], make_float2(v[c].x, -v[c].y));
    }
    const float pa = hypotf(p.x, p.y);
    const float2 phi = pa > 0.f ? make_float2(p.x / pa, p.y / pa) : make_float2(1.f, 0.f);
    const bool keep = lam > crop && r > 0.f && r > thresh * smax[n];
#pragma unroll
    for (int c = 0; c < CB; ++c) {
        float2 o = make_float2(0.f, 0.f);
        if (keep) cmac(o, v[c], phi);
        if (c < C) lc[c * HW] = o;
    }
    if (eval) eval[(size_t)n * HW + pix] = lam;
}

}  // namespace

hipError_t launch_espirit_gram(const float2* y, int C, int acs_h, int acs_w, int k, double2* ws, int N, int H, int W, hipStream_t s) {
    const int np = espirit_padded(C, k);
    hipLaunchKernelGGL(espirit_gram_kernel, dim3((np * np + kEsThreads - 1) / kEsThreads, N), dim3(kEsThreads), 0, s, y, C, acs_h, acs_w, k, np, ws,
                       H, W);
    return hipGetLastError();
}

hipError_t launch_espirit_eig(double2* ws, int C, int k, int N, hipStream_t s) {
    hipLaunchKernelGGL(espirit_eig_kernel, dim3(N), dim3(kEsEigThreads), 0, s, ws, espirit_padded(C, k));
    return hipGetLastError();
}

hipError_t launch_espirit_kern(const double2* ws, int C, int k, double sv_thresh, float2* kern, int* nkept, int N, hipStream_t s) {
    const int D = 2 * k - 1;
    hipLaunchKernelGGL(espirit_kern_kernel, dim3((C * C * D * D + kEsThreads - 1) / kEsThreads, N), dim3(kEsThreads), 0, s, ws, C, k,
                       espirit_padded(C, k), sv_thresh * sv_thresh, kern, nkept);
    return hipGetLastError();
}

hipError_t launch_espirit_pixels(float2* sens, const float2* kern, const float* rss, const float* smax, int C, int k, int iters, float crop,
                                 float thresh, float* eval, int N, int H, int W, hipStream_t s) {
    const dim3 grid((unsigned)((W + kEsThreads - 1) / kEsThreads), (unsigned)H, (unsigned)N);
    if (C <= 8)
        hipLaunchKernelGGL(espirit_pixel_kernel<8>, grid, dim3(kEsThreads), 0, s, sens, kern, rss, smax, C, k, iters, crop, thresh, eval, H, W);
    else
        hipLaunchKernelGGL(espirit_pixel_kernel<16>, grid, dim3(kEsThreads), 0, s, sens, kern, rss, smax, C, k, iters, crop, thresh, eval, H, W);
    return hipGetLastError();
}

}  // namespace pnp
