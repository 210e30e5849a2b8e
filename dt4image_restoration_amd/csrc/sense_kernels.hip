// Multi-coil (SENSE) data fidelity: the pointwise kernels around the engine's plain (unshifted) FFT passes, run at batch N * C.
//
// With coil maps S_c, the sampling mask M and the centred orthonormal pair fft_c / ifft_c:
//     A p   = [ M . fft_c(S_c . p) ]_c          A^H q = sum_c conj(S_c) . ifft_c(M . q_c)          Nop(p) = A^H A p + mu p
// Shift folding (H/2, W/2 even; sgn[k] = (-1)^(k1 + k2), S = the half-size roll): fft_c(v)[S k] = sgn[k] FFT(v)[k] and
// ifft_c(q) = IFFT(sgn[k] q[S k]).  The two signs cancel inside A^H A, so the normal operator needs the PLAIN transforms and the rolled mask
// (S mask, the layout reset_kernel stores) only; y is kept as ys = sgn . S y, reset_kernel's y0s convention, one plane per coil.
//
// One Nop in this (unfused) form:  sense_expand_kernel  p -> work[n, c] = S_c . p      | rows forward | cols forward |
//                                  sense_mask_kernel    work = mask ? work : 0         | cols inverse | rows inverse |
//                                  sense_combine_kernel q = sum_c conj(S_c) . work[n, c] + mu p,  partial sums of Re<p, q>
// CG scalars: every inner product is per slice; its terms are float32 values multiplied and summed in float64 by ONE workgroup per kPixelChunk
// pixels of one slice (fixed tree: block_sums_fixed), then by sense_scalar_kernel over the slice's partials in a fixed order.  No atomics:
// bitwise reproducible, and a slice's bits do not depend on N or on its place in the batch.  alpha / beta are float64 in device memory and
// applied as float32.  Slices with t_action > 0.5 are skipped by every kernel that writes z, u, a CG vector or a scalar.
#include "pnp_internal.h"
#include "block_reduce.h"

namespace pnp {

namespace {

constexpr int kSenseThreads = 256;
constexpr int kSensePer = kPixelChunk / kSenseThreads;     // pixels per thread
static_assert(kPixelChunk % kSenseThreads == 0, "whole pixels per thread");

__device__ __forceinline__ bool stopped(const float* tact, int n) { return tact != nullptr && tact[n] > 0.5f; }
__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cmulc(float2 s, float2 w) { return make_float2(s.x * w.x + s.y * w.y, s.x * w.y - s.y * w.x); }   // conj(s) w

// work[n, c, p] = S_c[p] * src[n, p]; src complex [N, HW], or a real image (REAL)
template <bool REAL>
__global__ __launch_bounds__(kSenseThreads) void sense_expand_kernel(const void* __restrict__ src, const float2* __restrict__ sens, int sens_n,
                                                                     int C, const float* __restrict__ tact, float2* __restrict__ work, int HW) {
    const int n = blockIdx.y;
    if (stopped(tact, n)) return;
    const int p0 = blockIdx.x * kPixelChunk + threadIdx.x;
    const size_t base = (size_t)n * HW;
    float2 v[kSensePer];
#pragma unroll
    for (int j = 0; j < kSensePer; ++j) {
        const int p = p0 + j * kSenseThreads;
        if (p < HW) v[j] = REAL ? make_float2(static_cast<const float*>(src)[base + p], 0.f) : static_cast<const float2*>(src)[base + p];
    }
    for (int c = 0; c < C; ++c) {
        const float2* sc = sens + ((size_t)(sens_n > 1 ? n : 0) * C + c) * HW;
        float2* wc = work + ((size_t)n * C + c) * HW;
        float2 s[kSensePer];
#pragma unroll
        for (int j = 0; j < kSensePer; ++j) {
            const int p = p0 + j * kSenseThreads;
            if (p < HW) s[j] = sc[p];
        }
#pragma unroll
        for (int j = 0; j < kSensePer; ++j) {
            const int p = p0 + j * kSenseThreads;
            if (p < HW) wc[p] = REAL ? make_float2(s[j].x * v[j].x, s[j].y * v[j].x) : cmul(s[j], v[j]);
        }
    }
}

// work[n, c, k] = masks[k] ? work : 0 (masks: the rolled layout); grid (chunks, N * C)
__global__ __launch_bounds__(kSenseThreads) void sense_mask_kernel(float2* __restrict__ work, const uint8_t* __restrict__ masks, int mask_n, int C,
                                                                   int HW) {
    const int nc = blockIdx.y, n = nc / C;
    const int p0 = blockIdx.x * kPixelChunk + threadIdx.x;
    const uint8_t* mk = masks + (mask_n > 1 ? (size_t)n * HW : 0);
    float2* w = work + (size_t)nc * HW;
#pragma unroll
    for (int j = 0; j < kSensePer; ++j) {
        const int p = p0 + j * kSenseThreads;
        if (p < HW && !mk[p]) w[p] = make_float2(0.f, 0.f);
    }
}

// q[n, p] = sum_c conj(S_c[p]) work[n, c, p] (+ mu[n] pv[n, p] when pv != nullptr); partial[n, chunk] = sum over the chunk of Re(conj(pv) q)
__global__ __launch_bounds__(kSenseThreads) void sense_combine_kernel(const float2* __restrict__ work, const float2* __restrict__ sens, int sens_n,
                                                                      int C, const float2* __restrict__ pv, const float* __restrict__ mu,
                                                                      const float* __restrict__ tact, float2* __restrict__ q,
                                                                      double* __restrict__ partial, int HW) {
    __shared__ double red[kSenseThreads / 64];
    const int n = blockIdx.y;
    if (stopped(tact, n)) return;
    const int p0 = blockIdx.x * kPixelChunk + threadIdx.x;
    const size_t base = (size_t)n * HW;
    float2 acc[kSensePer];
    for (int c = 0; c < C; ++c) {
        const float2* sc = sens + ((size_t)(sens_n > 1 ? n : 0) * C + c) * HW;
        const float2* wc = work + ((size_t)n * C + c) * HW;
        float2 s[kSensePer], w[kSensePer];
#pragma unroll
        for (int j = 0; j < kSensePer; ++j) {
            const int p = p0 + j * kSenseThreads;
            if (p < HW) { s[j] = sc[p]; w[j] = wc[p]; }
        }
#pragma unroll
        for (int j = 0; j < kSensePer; ++j) {
            const int p = p0 + j * kSenseThreads;
            if (p < HW) {
                const float2 t = cmulc(s[j], w[j]);
                acc[j] = c == 0 ? t : make_float2(acc[j].x + t.x, acc[j].y + t.y);
            }
        }
    }
    double dot[1] = {0.0};
    const float m = (pv != nullptr && mu != nullptr) ? mu[n] : 0.f;
#pragma unroll
    for (int j = 0; j < kSensePer; ++j) {
        const int p = p0 + j * kSenseThreads;
        if (p < HW) {
            float2 o = acc[j];
            if (pv != nullptr) {
                const float2 pp = pv[base + p];
                o.x += m * pp.x; o.y += m * pp.y;
                dot[0] += (double)pp.x * (double)o.x + (double)pp.y * (double)o.y;
            }
            q[base + p] = o;
        }
    }
    if (partial == nullptr) return;                        // (uniform)
    block_sums_fixed<kSenseThreads, 1>(dot, red);
    if (threadIdx.x == 0) partial[((size_t)n * gridDim.x + blockIdx.x) * 2] = dot[0];
}

// b = aty + mu (x + u);  r = b - q;  p = r;  partial[n, chunk] = (<r, r>, <b, b>)
__global__ __launch_bounds__(kSenseThreads) void sense_cg_init_kernel(const float2* __restrict__ aty, const float* __restrict__ x,
                                                                      const float2* __restrict__ u, const float2* __restrict__ q,
                                                                      const float* __restrict__ mu, const float* __restrict__ tact,
                                                                      float2* __restrict__ r, float2* __restrict__ pv,
                                                                      double* __restrict__ partial, int HW) {
    __shared__ double red[2 * (kSenseThreads / 64)];
    const int n = blockIdx.y;
    if (stopped(tact, n)) return;
    const int p0 = blockIdx.x * kPixelChunk + threadIdx.x;
    const size_t base = (size_t)n * HW;
    const float m = mu[n];
    double acc[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < kSensePer; ++j) {
        const int p = p0 + j * kSenseThreads;
        if (p < HW) {
            const size_t g = base + p;
            const float2 a = aty[g], uu = u[g], qq = q[g];
            const float xx = x[g];
            const float2 b = make_float2(a.x + m * (xx + uu.x), a.y + m * uu.y);
            const float2 rr = make_float2(b.x - qq.x, b.y - qq.y);
            r[g] = rr;
            pv[g] = rr;
            acc[0] += (double)rr.x * (double)rr.x + (double)rr.y * (double)rr.y;
            acc[1] += (double)b.x * (double)b.x + (double)b.y * (double)b.y;
        }
    }
    block_sums_fixed<kSenseThreads, 2>(acc, red);
    if (threadIdx.x == 0) {
        double* o = partial + ((size_t)n * gridDim.x + blockIdx.x) * 2;
        o[0] = acc[0]; o[1] = acc[1];
    }
}

// The per-slice scalars sc[n, 8] = (rs, bb, alpha, beta, frozen, -, -, -), from the slice's partials summed in a fixed order.
//   mode 0: rs = sum part[., 0], bb = sum part[., 1]
//   mode 1: pq = sum part[., 0];  rs <= 0 or pq <= 0: alpha = 0, frozen;  else alpha = rs / pq
//   mode 2: rs' = sum part[., 0];  beta = frozen ? 0 : rs' / rs;  rs = rs'
__global__ __launch_bounds__(kSenseThreads) void sense_scalar_kernel(const double* __restrict__ partial, int chunks, int mode,
                                                                     const float* __restrict__ tact, double* __restrict__ sc) {
    __shared__ double red[2 * (kSenseThreads / 64)];
    const int n = blockIdx.x;
    if (stopped(tact, n)) return;
    double acc[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < chunks; i += kSenseThreads) {
        const double* p = partial + ((size_t)n * chunks + i) * 2;
        acc[0] += p[0];
        if (mode == 0) acc[1] += p[1];
    }
    block_sums_fixed<kSenseThreads, 2>(acc, red);
    if (threadIdx.x != 0) return;
    double* s = sc + (size_t)n * 8;
    if (mode == 0) {
        s[0] = acc[0]; s[1] = acc[1]; s[2] = 0.0; s[3] = 0.0; s[4] = 0.0;
    } else if (mode == 1) {
        const double rs = s[0], pq = acc[0];
        const bool ok = rs > 0.0 && pq > 0.0;
        s[2] = ok ? rs / pq : 0.0;
        s[4] = ok ? 0.0 : 1.0;
    } else {
        const double rs = s[0];
        s[3] = s[4] != 0.0 ? 0.0 : acc[0] / rs;
        s[0] = acc[0];
    }
}

// z += alpha p;  r -= alpha q;  partial[n, chunk] = <r, r>
__global__ __launch_bounds__(kSenseThreads) void sense_cg_update_kernel(float2* __restrict__ z, float2* __restrict__ r, const float2* __restrict__ pv,
                                                                        const float2* __restrict__ q, const double* __restrict__ sc,
                                                                        const float* __restrict__ tact, double* __restrict__ partial, int HW) {
    __shared__ double red[kSenseThreads / 64];
    const int n = blockIdx.y;
    if (stopped(tact, n)) return;
    const int p0 = blockIdx.x * kPixelChunk + threadIdx.x;
    const size_t base = (size_t)n * HW;
    const float alpha = (float)sc[(size_t)n * 8 + 2];
    double acc[1] = {0.0};
#pragma unroll
    for (int j = 0; j < kSensePer; ++j) {
        const int p = p0 + j * kSenseThreads;
        if (p < HW) {
            const size_t g = base + p;
            const float2 pp = pv[g], qq = q[g];
            float2 zz = z[g], rr = r[g];
            zz.x += alpha * pp.x; zz.y += alpha * pp.y;
            rr.x -= alpha * qq.x; rr.y -= alpha * qq.y;
            z[g] = zz;
            r[g] = rr;
            acc[0] += (double)rr.x * (double)rr.x + (double)rr.y * (double)rr.y;
        }
    }
    block_sums_fixed<kSenseThreads, 1>(acc, red);
    if (threadIdx.x == 0) partial[((size_t)n * gridDim.x + blockIdx.x) * 2] = acc[0];
}

// p = r + beta p
__global__ __launch_bounds__(kSenseThreads) void sense_cg_dir_kernel(const float2* __restrict__ r, float2* __restrict__ pv, const double* __restrict__ sc,
                                                                     const float* __restrict__ tact, int HW) {
    const int n = blockIdx.y;
    if (stopped(tact, n)) return;
    const int p0 = blockIdx.x * kPixelChunk + threadIdx.x;
    const size_t base = (size_t)n * HW;
    const float beta = (float)sc[(size_t)n * 8 + 3];
#pragma unroll
    for (int j = 0; j < kSensePer; ++j) {
        const int p = p0 + j * kSenseThreads;
        if (p < HW) {
            const size_t g = base + p;
            const float2 rr = r[g], pp = pv[g];
            pv[g] = make_float2(rr.x + beta * pp.x, rr.y + beta * pp.y);
        }
    }
}

// u <- u + x - z
__global__ __launch_bounds__(kSenseThreads) void sense_dual_kernel(const float* __restrict__ x, const float2* __restrict__ z, float2* __restrict__ u,
                                                                   const float* __restrict__ tact, int HW) {
    const int n = blockIdx.y;
    if (stopped(tact, n)) return;
    const int p0 = blockIdx.x * kPixelChunk + threadIdx.x;
    const size_t base = (size_t)n * HW;
#pragma unroll
    for (int j = 0; j < kSensePer; ++j) {
        const int p = p0 + j * kSenseThreads;
        if (p < HW) {
            const size_t g = base + p;
            const float2 uu = u[g], zz = z[g];
            u[g] = make_float2(uu.x + x[g] - zz.x, uu.y - zz.y);
        }
    }
}

__global__ void sense_cgres_kernel(const double* __restrict__ sc, float* __restrict__ out, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const double rs = sc[(size_t)n * 8], bb = sc[(size_t)n * 8 + 1];
    out[n] = bb > 0.0 ? (float)sqrt(rs / bb) : 0.f;
}

// partial[n, chunk] = sum_c sum over the chunk of masks[k] ? |fx[n, c, k] - ys[n, c, k]|^2 : 0   (fx: the plain transform of S_c x)
__global__ __launch_bounds__(kSenseThreads) void sense_misfit_kernel(const float2* __restrict__ fx, const float2* __restrict__ ys,
                                                                     const uint8_t* __restrict__ masks, int mask_n, int C,
                                                                     double* __restrict__ partial, int HW) {
    __shared__ double red[kSenseThreads / 64];
    const int n = blockIdx.y;
    const int p0 = blockIdx.x * kPixelChunk + threadIdx.x;
    const uint8_t* mk = masks + (mask_n > 1 ? (size_t)n * HW : 0);
    uint8_t mm[kSensePer];
#pragma unroll
    for (int j = 0; j < kSensePer; ++j) {
        const int p = p0 + j * kSenseThreads;
        mm[j] = p < HW ? mk[p] : (uint8_t)0;
    }
    double acc[1] = {0.0};
    for (int c = 0; c < C; ++c) {
        const size_t cb = ((size_t)n * C + c) * HW;
#pragma unroll
        for (int j = 0; j < kSensePer; ++j) {
            const int p = p0 + j * kSenseThreads;
            if (mm[j]) {
                const float2 a = fx[cb + p], b = ys[cb + p];
                const float dx = a.x - b.x, dy = a.y - b.y;
                acc[0] += (double)dx * (double)dx + (double)dy * (double)dy;
            }
        }
    }
    block_sums_fixed<kSenseThreads, 1>(acc, red);
    if (threadIdx.x == 0) partial[(size_t)n * gridDim.x + blockIdx.x] = acc[0];
}

// Episode constants: ys[n, c, k] = sgn[k] y[n, c, S k] (reset_kernel's y0s convention, per coil) and, masked, the same into work (the plain
// inverse transform of which is ifft_c(M y_c)); masks[k] = mask[S k].  grid (chunks, N * C)
__global__ __launch_bounds__(kSenseThreads) void sense_install_kernel(const float2* __restrict__ y, const uint8_t* __restrict__ mask, int mask_n, int C,
                                                                      float2* __restrict__ ys, float2* __restrict__ work,
                                                                      uint8_t* __restrict__ masks, int H, int W) {
    const int nc = blockIdx.y, n = nc / C, c = nc - n * C;
    const int HW = H * W, hh = H >> 1, hw = W >> 1;
    const int p0 = blockIdx.x * kPixelChunk + threadIdx.x;
    const size_t mb = mask_n > 1 ? (size_t)n * HW : 0;
    const bool store_mask = c == 0 && (mask_n > 1 || n == 0);
#pragma unroll
    for (int j = 0; j < kSensePer; ++j) {
        const int p = p0 + j * kSenseThreads;
        if (p >= HW) continue;
        const int k1 = p / W, k2 = p - k1 * W;
        const int ps = (k1 < hh ? k1 + hh : k1 - hh) * W + (k2 < hw ? k2 + hw : k2 - hw);
        const float sg = ((k1 + k2) & 1) ? -1.f : 1.f;
        const float2 yy = y[(size_t)nc * HW + ps];
        const float2 v = make_float2(sg * yy.x, sg * yy.y);
        const uint8_t m = mask[mb + ps] ? 1 : 0;
        ys[(size_t)nc * HW + p] = v;
        work[(size_t)nc * HW + p] = m ? v : make_float2(0.f, 0.f);
        if (store_mask) masks[mb + p] = m;
    }
}

// x = Re(x0), z = x0, u = 0 (pnp_reset's iterate)
__global__ __launch_bounds__(kSenseThreads) void sense_iterate_kernel(const float2* __restrict__ x0, float* __restrict__ x, float2* __restrict__ z,
                                                                      float2* __restrict__ u, size_t total) {
    for (size_t i = (size_t)blockIdx.x * kSenseThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kSenseThreads) {
        const float2 v = x0[i];
        x[i] = v.x;
        z[i] = v;
        u[i] = make_float2(0.f, 0.f);
    }
}

inline dim3 tile_grid(int H, int W, int batch) { return dim3((unsigned)pixel_chunks(H, W), (unsigned)batch); }

}  // namespace

hipError_t launch_sense_expand(const float2* src, const float* src_real, const float2* sens, int sens_n, int C, const float* tact, float2* work,
                               int N, int H, int W, hipStream_t s) {
    if (src_real != nullptr)
        hipLaunchKernelGGL(sense_expand_kernel<true>, tile_grid(H, W, N), dim3(kSenseThreads), 0, s, (const void*)src_real, sens, sens_n, C, tact, work, H * W);
    else
        hipLaunchKernelGGL(sense_expand_kernel<false>, tile_grid(H, W, N), dim3(kSenseThreads), 0, s, (const void*)src, sens, sens_n, C, tact, work, H * W);
    return hipGetLastError();
}

hipError_t launch_sense_mask(float2* work, const uint8_t* masks, int mask_n, int C, int N, int H, int W, hipStream_t s) {
    hipLaunchKernelGGL(sense_mask_kernel, tile_grid(H, W, N * C), dim3(kSenseThreads), 0, s, work, masks, mask_n, C, H * W);
    return hipGetLastError();
}

hipError_t launch_sense_combine(const float2* work, const float2* sens, int sens_n, int C, const float2* pv, const float* mu, const float* tact,
                                float2* q, double* partial, int N, int H, int W, hipStream_t s) {
    hipLaunchKernelGGL(sense_combine_kernel, tile_grid(H, W, N), dim3(kSenseThreads), 0, s, work, sens, sens_n, C, pv, mu, tact, q, partial, H * W);
    return hipGetLastError();
}

hipError_t launch_sense_cg_init(const float2* aty, const float* x, const float2* u, const float2* q, const float* mu, const float* tact, float2* r,
                                float2* pv, double* partial, int N, int H, int W, hipStream_t s) {
    hipLaunchKernelGGL(sense_cg_init_kernel, tile_grid(H, W, N), dim3(kSenseThreads), 0, s, aty, x, u, q, mu, tact, r, pv, partial, H * W);
    return hipGetLastError();
}

hipError_t launch_sense_scalar(const double* partial, int mode, const float* tact, double* sc, int N, int H, int W, hipStream_t s) {
    hipLaunchKernelGGL(sense_scalar_kernel, dim3(N), dim3(kSenseThreads), 0, s, partial, pixel_chunks(H, W), mode, tact, sc);
    return hipGetLastError();
}

hipError_t launch_sense_cg_update(float2* z, float2* r, const float2* pv, const float2* q, const double* sc, const float* tact, double* partial,
                                  int N, int H, int W, hipStream_t s) {
    hipLaunchKernelGGL(sense_cg_update_kernel, tile_grid(H, W, N), dim3(kSenseThreads), 0, s, z, r, pv, q, sc, tact, partial, H * W);
    return hipGetLastError();
}

hipError_t launch_sense_cg_dir(const float2* r, float2* pv, const double* sc, const float* tact, int N, int H, int W, hipStream_t s) {
    hipLaunchKernelGGL(sense_cg_dir_kernel, tile_grid(H, W, N), dim3(kSenseThreads), 0, s, r, pv, sc, tact, H * W);
    return hipGetLastError();
}

hipError_t launch_sense_dual(const float* x, const float2* z, float2* u, const float* tact, int N, int H, int W, hipStream_t s) {
    hipLaunchKernelGGL(sense_dual_kernel, tile_grid(H, W, N), dim3(kSenseThreads), 0, s, x, z, u, tact, H * W);
    return hipGetLastError();
}

hipError_t launch_sense_cgres(const double* sc, float* out, int N, hipStream_t s) {
    hipLaunchKernelGGL(sense_cgres_kernel, dim3((N + 63) / 64), dim3(64), 0, s, sc, out, N);
    return hipGetLastError();
}

hipError_t launch_sense_misfit(const float2* fx, const float2* ys, const uint8_t* masks, int mask_n, int C, double* dcpartial, int N, int H, int W,
                               hipStream_t s) {
    hipLaunchKernelGGL(sense_misfit_kernel, tile_grid(H, W, N), dim3(kSenseThreads), 0, s, fx, ys, masks, mask_n, C, dcpartial, H * W);
    return hipGetLastError();
}

hipError_t launch_sense_install(const float2* y, const uint8_t* mask, int mask_n, int C, float2* ys, float2* work, uint8_t* masks, int N, int H,
                                int W, hipStream_t s) {
    hipLaunchKernelGGL(sense_install_kernel, tile_grid(H, W, N * C), dim3(kSenseThreads), 0, s, y, mask, mask_n, C, ys, work, masks, H, W);
    return hipGetLastError();
}

hipError_t launch_sense_iterate(const float2* x0, float* x, float2* z, float2* u, int N, int H, int W, hipStream_t s) {
    const size_t total = (size_t)N * H * W;
    size_t blocks = (total + kSenseThreads - 1) / kSenseThreads;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(sense_iterate_kernel, dim3((unsigned)blocks), dim3(kSenseThreads), 0, s, x0, x, z, u, total);
    return hipGetLastError();
}

}  // namespace pnp
