// k-space stage for sides L = 2^a * 5^b: 80, 160, 320, 400, 640, 800 (with 16 | L <= 1024 these are all of them), mixed freely with
// power-of-two sides (640 x 320, 320 x 256).  A handle selects these kernels when one of its sides is not a power of two; a handle
// whose sides are both powers of two never reaches this file (fft_kernels.hip).
//
// Same three launches and fusions as the power-of-two path (fft_kernels.hip, header comment), same shift folding by pnp_reset:
//   rows-forward (MODE 1) : v = x + u in the load -> row FFT -> work
//   cols + prox  (MODE 1) : column FFT -> masked closed-form solve with y0s / masks / mu -> inverse column FFT, in place in `work`
//   rows-inverse (MODE 2) : row IFFT -> z;  u += x - z
// plus the centred plain passes of pnp_fft2c (MODE 0), whose fftshift / ifftshift are folded into the load and store indices as an
// add-mod by L/2 (the XOR of the power-of-two kernels is only right for powers of two).
//
// Each line is a Stockham autosort FFT in LDS with a run-time length: the radix-5 passes first (Ns = 1, 5), then radix-4 passes, then one
// radix-2 pass when log2 of the power-of-two part is odd (320 = 5 * 4^3, 640 = 5 * 4^3 * 2, 800 = 5^2 * 4^2 * 2).  Radix 5 first also keeps
// the first pass's stores (lanes 5 elements = 10 dwords apart) on distinct banks of ds_write_b64's 16-lane groups.
// Twiddles are the handle's tables exp(-2 pi i m / L) (make_twiddles), conjugated for the inverse.
//
// This file is compiled without SLP vectorisation (Makefile): its complex arithmetic stays scalar v_fma_f32 / v_add_f32, so no packed-FP32
// op whose low result reads the high register of a pair (op_sel = 1) appears in these kernels - they run in PNP_FLAG_BF16_CONVS handles
// next to bf16 MFMA kernels (profiles/r05_race.md; tools/isa_audit.py, tests/test_kspace_radix5_host.py).
#include "pnp_internal.h"
#include "fft_common.h"

namespace pnp {

namespace {

constexpr int kMixedRowElems = 2048;   // complex elements per row workgroup at most (as ROW_ELEMS of the power-of-two passes)

// v[0..4] -> its 5-point DFT in natural order.  c1 = cos(2 pi / 5), c2 = cos(4 pi / 5), s1 = sin(2 pi / 5), s2 = sin(4 pi / 5):
//   X0 = x0 + a1 + a2,  X1,4 = t1 -/+ i p,  X2,3 = t2 -/+ i q   (forward; the inverse swaps the signs of i)
// with a1 = x1 + x4, b1 = x1 - x4, a2 = x2 + x3, b2 = x2 - x3, t1 = x0 + c1 a1 + c2 a2, t2 = x0 + c2 a1 + c1 a2, p = s1 b1 + s2 b2,
// q = s2 b1 - s1 b2.
template <bool INV>
__device__ __forceinline__ void dft5_inplace(float2* v) {
    constexpr float C1 = 0.30901699437494742f, C2 = -0.80901699437494742f, S1 = 0.95105651629515357f, S2 = 0.58778525229247313f;
    const float2 x0 = v[0];
    const float2 a1 = cadd(v[1], v[4]), b1 = csub(v[1], v[4]), a2 = cadd(v[2], v[3]), b2 = csub(v[2], v[3]);
    const float2 t1 = make_float2(fmaf(C2, a2.x, fmaf(C1, a1.x, x0.x)), fmaf(C2, a2.y, fmaf(C1, a1.y, x0.y)));
    const float2 t2 = make_float2(fmaf(C1, a2.x, fmaf(C2, a1.x, x0.x)), fmaf(C1, a2.y, fmaf(C2, a1.y, x0.y)));
    const float2 p = make_float2(fmaf(S2, b2.x, S1 * b1.x), fmaf(S2, b2.y, S1 * b1.y));
    const float2 q = make_float2(fmaf(-S1, b2.x, S2 * b1.x), fmaf(-S1, b2.y, S2 * b1.y));
    // -i p = (p.y, -p.x)
    const float2 tm1 = make_float2(t1.x + p.y, t1.y - p.x), tp1 = make_float2(t1.x - p.y, t1.y + p.x);
    const float2 tm2 = make_float2(t2.x + q.y, t2.y - q.x), tp2 = make_float2(t2.x - q.y, t2.y + q.x);
    v[0] = cadd(x0, cadd(a1, a2));
    v[1] = INV ? tp1 : tm1;
    v[4] = INV ? tm1 : tp1;
    v[2] = INV ? tp2 : tm2;
    v[3] = INV ? tm2 : tp2;
}

template <int R, bool INV>
__device__ __forceinline__ void dft_small(float2* v) {
    if constexpr (R == 5) dft5_inplace<INV>(v);
    else if constexpr (R == 4) dft4_inplace<INV>(v[0], v[1], v[2], v[3]);
    else { static_assert(R == 2, "radix 2, 4 or 5"); const float2 t = v[0]; v[0] = cadd(t, v[1]); v[1] = csub(t, v[1]); }
}

// One radix-R Stockham pass over `lines` lines of length L (line i at [i lstr, i lstr + L)), Ns = the product of the radices before it:
// butterfly j (k = j mod Ns) reads j + m L/R (m < R), twiddles input m by w_{Ns R}^{m k} = tw[m k L / (Ns R)], and writes output q to
// (j - k) R + k + q Ns.  Indices stay inside [0, L): j - k is a multiple of Ns and at most L/R - Ns.
template <int R, bool INV>
__device__ __forceinline__ void mixed_pass(const float2* src, float2* dst, const float2* tw, int L, int Ns, int lines, int lstr) {
    const int per = L / R, total = lines * per, tstep = L / (Ns * R);
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const int line = idx / per, j = idx - line * per;
        const int k = j % Ns;
        const float2* sp = src + line * lstr + j;
        float2 v[R];
#pragma unroll
        for (int m = 0; m < R; ++m) v[m] = sp[m * per];
        if (Ns > 1) {
#pragma unroll
            for (int m = 1; m < R; ++m) {
                float2 w = tw[m * k * tstep];
                if (INV) w.y = -w.y;
                v[m] = cmul(v[m], w);
            }
        }
        dft_small<R, INV>(v);
        float2* dp = dst + line * lstr + (j - k) * R + k;
#pragma unroll
        for (int q = 0; q < R; ++q) dp[q * Ns] = v[q];
    }
}

// `lines` transforms of length L = 2^a * 5^b, ping-ponging src <-> dst.  Caller has synchronised the loads; returns the buffer holding
// the (synchronised) result.
template <bool INV>
__device__ float2* fft_lines_mixed(float2* src, float2* dst, const float2* tw, int L, int lines, int lstr) {
    int Ns = 1;
    auto flip = [&]() { __syncthreads(); float2* t = src; src = dst; dst = t; };
    while ((L / Ns) % 5 == 0) { mixed_pass<5, INV>(src, dst, tw, L, Ns, lines, lstr); flip(); Ns *= 5; }
    while ((L / Ns) % 4 == 0) { mixed_pass<4, INV>(src, dst, tw, L, Ns, lines, lstr); flip(); Ns *= 4; }
    if (Ns < L) { mixed_pass<2, INV>(src, dst, tw, L, Ns, lines, lstr); flip(); }   // L / Ns == 2
    return src;
}

__device__ __forceinline__ int add_mod(int i, int s, int n) { return i + s < n ? i + s : i + s - n; }   // i < n, s <= n

// Rows [y0, y0 + rpb) of slice n per workgroup; rpb divides H.  LDS: two rpb x W buffers (lines W apart) + W twiddles.
// MODE 0: in -> out with both indices rolled by `shift` (0 or W/2); 1: x + u -> work; 2: work -> z, u += x - z.
template <int MODE>
__global__ __launch_bounds__(256) void fft_rows_mixed_kernel(const float2* in, float2* out, const float* __restrict__ x, float2* __restrict__ u,
                                                             const float2* __restrict__ twg, const float* __restrict__ tact,
                                                             int H, int W, int rpb, int inverse, int shift) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int blocks_per_img = H / rpb;
    // ADMM passes: the slice -> XCD map of the power-of-two row and column kernels (workgroups b, b + 8, ... share an XCD), so the scratch
    // a slice's row pass writes is in the L2 of the XCD whose column pass reads it
    int vb = blockIdx.x;
    if (MODE != 0 && (gridDim.x & 7) == 0) vb = (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
    const int n = vb / blocks_per_img;
    const int y0 = (vb % blocks_per_img) * rpb;
    if (MODE != 0 && tact != nullptr && tact[n] > 0.5f) return;
    float2* const buf0 = smem;
    float2* const buf1 = smem + rpb * W;
    float2* const tw = smem + 2 * rpb * W;
    const size_t base = ((size_t)n * H + y0) * W;
    const int tot = rpb * W;
    for (int i = threadIdx.x; i < W; i += blockDim.x) tw[i] = twg[i];
    constexpr int NB = 8;                                  // independent global requests per thread and batch
    for (int e0 = threadIdx.x; e0 < tot; e0 += NB * 256) {
        float2 v[NB];
        float xv[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int e = e0 + k * 256;
            if (e < tot) {
                if (MODE == 1) { v[k] = u[base + e]; xv[k] = x[base + e]; }
                else if (MODE == 2) v[k] = in[base + e];
                else { const int r = e / W, c = e - r * W; v[k] = in[base + (size_t)r * W + add_mod(c, shift, W)]; }
            }
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int e = e0 + k * 256;
            if (e < tot) buf0[e] = MODE == 1 ? make_float2(xv[k] + v[k].x, v[k].y) : v[k];
        }
    }
    __syncthreads();
    const bool inv = (MODE == 2) || (MODE == 0 && inverse);
    float2* const res = inv ? fft_lines_mixed<true>(buf0, buf1, tw, W, rpb, W) : fft_lines_mixed<false>(buf0, buf1, tw, W, rpb, W);
    const float sc = rsqrtf((float)W);
    for (int e0 = threadIdx.x; e0 < tot; e0 += NB * 256) {
        float2 uu[NB];
        float xv[NB];
        if (MODE == 2) {
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                const int e = e0 + k * 256;
                if (e < tot) { uu[k] = u[base + e]; xv[k] = x[base + e]; }
            }
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int e = e0 + k * 256;
            if (e < tot) {
                float2 v = res[e];
                v.x *= sc; v.y *= sc;
                if (MODE == 2) {
                    out[base + e] = v;                                                   // z
                    u[base + e] = make_float2(uu[k].x + xv[k] - v.x, uu[k].y - v.y);     // u + x - z
                } else if (MODE == 1) {
                    out[base + e] = v;
                } else {
                    const int r = e / W, c = e - r * W;
                    out[base + (size_t)r * W + add_mod(c, shift, W)] = v;
                }
            }
        }
    }
}

// Row pass of a REAL image into complex scratch, forward, no index shift (pnp_residuals' data misfit reads the plain transform of x):
// rows [y0, y0 + rpb) of slice n per workgroup, LDS and line transform as fft_rows_mixed_kernel.  A kernel of its own, so the three shipped
// instantiations above keep their instruction streams.
__global__ __launch_bounds__(256) void fft_rows_real_m5_kernel(const float* __restrict__ x, float2* __restrict__ out,
                                                               const float2* __restrict__ twg, int H, int W, int rpb) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int blocks_per_img = H / rpb;
    const int n = blockIdx.x / blocks_per_img;
    const int y0 = (blockIdx.x % blocks_per_img) * rpb;
    float2* const buf0 = smem;
    float2* const buf1 = smem + rpb * W;
    float2* const tw = smem + 2 * rpb * W;
    const size_t base = ((size_t)n * H + y0) * W;
    const int tot = rpb * W;
    for (int i = threadIdx.x; i < W; i += blockDim.x) tw[i] = twg[i];
    constexpr int NB = 8;                                  // independent global requests per thread and batch
    for (int e0 = threadIdx.x; e0 < tot; e0 += NB * 256) {
        float xv[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int e = e0 + k * 256;
            if (e < tot) xv[k] = x[base + e];
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int e = e0 + k * 256;
            if (e < tot) buf0[e] = make_float2(xv[k], 0.f);
        }
    }
    __syncthreads();
    float2* const res = fft_lines_mixed<false>(buf0, buf1, tw, W, rpb, W);
    const float sc = rsqrtf((float)W);
    for (int e = threadIdx.x; e < tot; e += 256) {
        float2 v = res[e];
        v.x *= sc; v.y *= sc;
        out[base + e] = v;
    }
}

// Columns [x0, x0 + cw) of slice n per workgroup; cw (16, 8 or 4: a power of two) divides W.  LDS: two cw x H buffers whose lines (columns)
// are H + 1 elements apart - odd, so the cw lanes that stage or solve one row across the columns sit on distinct banks - + H twiddles.
// MODE 0: in-place centred pass with the row index rolled by `shift` (0 or H/2) in and out; 1: forward -> masked solve -> inverse.
template <int MODE>
__global__ __launch_bounds__(256) void fft_cols_mixed_kernel(float2* __restrict__ data, const float2* __restrict__ twg,
                                                             const float2* __restrict__ y0s, const uint8_t* __restrict__ masks,
                                                             int mask_n, const float* __restrict__ mu, const float* __restrict__ tact,
                                                             int H, int W, int cw, int inverse, int shift) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int strips = W / cw;
    int vb = blockIdx.x;                                   // (slice, strip) -> XCD map of fft_cols_kernel
    if ((gridDim.x & 7) == 0) vb = (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
    const int n = vb / strips;
    const int x0 = (vb % strips) * cw;
    if (MODE == 1 && tact != nullptr && tact[n] > 0.5f) return;
    const int lstr = H + 1;
    float2* const buf0 = smem;
    float2* const buf1 = smem + cw * lstr;
    float2* const tw = smem + 2 * cw * lstr;
    float2* const img = data + (size_t)n * H * W;
    const int tot = cw * H;
    const int lcw = 31 - __builtin_clz(cw);                // cw is a power of two (cols_per_block)
    for (int i = threadIdx.x; i < H; i += blockDim.x) tw[i] = twg[i];
    constexpr int NB = 8;
    for (int e0 = threadIdx.x; e0 < tot; e0 += NB * 256) {
        float2 v[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int e = e0 + k * 256;
            if (e < tot) v[k] = img[(size_t)(e >> lcw) * W + x0 + (e & (cw - 1))];
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int e = e0 + k * 256;
            if (e < tot) buf0[(e & (cw - 1)) * lstr + (MODE == 0 ? add_mod(e >> lcw, shift, H) : (e >> lcw))] = v[k];
        }
    }
    __syncthreads();
    const float sc = rsqrtf((float)H);
    if (MODE == 0) {
        float2* const res = inverse ? fft_lines_mixed<true>(buf0, buf1, tw, H, cw, lstr) : fft_lines_mixed<false>(buf0, buf1, tw, H, cw, lstr);
        for (int e = threadIdx.x; e < tot; e += 256) {
            const int r = e >> lcw, c = e & (cw - 1);
            float2 v = res[c * lstr + add_mod(r, shift, H)];
            v.x *= sc; v.y *= sc;
            img[(size_t)r * W + x0 + c] = v;
        }
        return;
    }
    float2* const res = fft_lines_mixed<false>(buf0, buf1, tw, H, cw, lstr);
    float2* const oth = (res == buf0) ? buf1 : buf0;
    const float m = mu[n];
    const float inv1m = 1.f + m;
    const float2* y0n = y0s + (size_t)n * H * W;
    const uint8_t* mk = masks + (mask_n > 1 ? (size_t)n * H * W : 0);
    for (int e0 = threadIdx.x; e0 < tot; e0 += NB * 256) {
        float2 yy[NB];
        uint8_t mm[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) {                     // mask and y0 of the batch in flight together
            const int e = e0 + k * 256;
            if (e < tot) {
                const size_t g = (size_t)(e >> lcw) * W + x0 + (e & (cw - 1));
                mm[k] = mk[g];
                yy[k] = y0n[g];
            }
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int e = e0 + k * 256;
            if (e < tot) {
                const int r = e >> lcw, c = e & (cw - 1);
                float2 v = res[c * lstr + r];
                v.x *= sc; v.y *= sc;                       // now the orthonormal FFT2 of x + u
                if (mm[k]) {                                // sampled k-space bin: closed-form solve
                    v.x = (m * v.x + yy[k].x) / inv1m;
                    v.y = (m * v.y + yy[k].y) / inv1m;
                }
                res[c * lstr + r] = v;
            }
        }
    }
    __syncthreads();
    float2* const r2 = fft_lines_mixed<true>(res, oth, tw, H, cw, lstr);
    for (int e = threadIdx.x; e < tot; e += 256) {
        const int r = e >> lcw, c = e & (cw - 1);
        float2 v = r2[c * lstr + r];
        v.x *= sc; v.y *= sc;
        img[(size_t)r * W + x0 + c] = v;
    }
}

// Rows per workgroup: the largest power of two <= min(16, kMixedRowElems / W).  H is a multiple of 16, so it always divides H (the
// power-of-two path's kMixedRowElems / W gives 6 at W = 320, which does not divide 320).
int mixed_rows_per_block(int W) {
    int r = 1;
    while (r < 16 && 2 * r * W <= kMixedRowElems) r *= 2;
    return r;
}
int mixed_cols_per_block(int H) { return H <= 256 ? 16 : (H <= 512 ? 8 : 4); }
size_t mixed_rows_lds(int W) { return (size_t)(2 * mixed_rows_per_block(W) * W + W) * sizeof(float2); }
size_t mixed_cols_lds(int H) { return (size_t)(2 * mixed_cols_per_block(H) * (H + 1) + H) * sizeof(float2); }   // <= 73.8 KiB (H = 1024)

hipError_t raise_mixed_cols_lds_cap() {
    static DeviceOnce once[2];
    const void* fns[2] = {(const void*)fft_cols_mixed_kernel<0>, (const void*)fft_cols_mixed_kernel<1>};
    for (int i = 0; i < 2; ++i)
        if (hipError_t e = pnp::raise_lds_cap(fns[i], 80 * 1024, once[i]); e != hipSuccess) return e;
    return hipSuccess;
}

}  // namespace

bool kspace_len_ok(int L) {
    if (L < 16 || L > 1024 || L % 16) return false;
    while (L % 5 == 0) L /= 5;
    return (L & (L - 1)) == 0;
}

// the mixed-radix family of the six k-space passes: reached through the dispatch in fft_kernels.hip only
namespace mixed {

hipError_t launch_fft_rows(const float2* in, float2* out, const float2* tw, int batch, int H, int W, int inverse, int shift, hipStream_t s) {
    const int rpb = mixed_rows_per_block(W);
    hipLaunchKernelGGL((fft_rows_mixed_kernel<0>), dim3(batch * (H / rpb)), dim3(256), mixed_rows_lds(W), s, in, out, nullptr, nullptr, tw,
                       nullptr, H, W, rpb, inverse, shift);
    return hipGetLastError();
}
hipError_t launch_fft_cols(float2* data, const float2* tw, int batch, int H, int W, int inverse, int shift, hipStream_t s) {
    const int cw = mixed_cols_per_block(H);
    if (hipError_t e = raise_mixed_cols_lds_cap()) return e;
    hipLaunchKernelGGL((fft_cols_mixed_kernel<0>), dim3(batch * (W / cw)), dim3(256), mixed_cols_lds(H), s, data, tw, nullptr, nullptr, 1,
                       nullptr, nullptr, H, W, cw, inverse, shift);
    return hipGetLastError();
}
hipError_t launch_fft_rows_fwd_admm(const float* x, const float2* u, float2* work, const float2* tw, const float* tact, int N, int H, int W,
                                    hipStream_t s) {
    const int rpb = mixed_rows_per_block(W);
    hipLaunchKernelGGL((fft_rows_mixed_kernel<1>), dim3(N * (H / rpb)), dim3(256), mixed_rows_lds(W), s, nullptr, work, x,
                       const_cast<float2*>(u), tw, tact, H, W, rpb, 0, 0);
    return hipGetLastError();
}
hipError_t launch_fft_rows_real(const float* x, float2* work, const float2* tw, int N, int H, int W, hipStream_t s) {
    const int rpb = mixed_rows_per_block(W);
    hipLaunchKernelGGL(fft_rows_real_m5_kernel, dim3(N * (H / rpb)), dim3(256), mixed_rows_lds(W), s, x, work, tw, H, W, rpb);
    return hipGetLastError();
}
hipError_t launch_fft_cols_prox(float2* work, const float2* tw, const float2* y0s, const uint8_t* masks, int mask_n, const float* mu,
                                const float* tact, int N, int H, int W, hipStream_t s) {
    const int cw = mixed_cols_per_block(H);
    if (hipError_t e = raise_mixed_cols_lds_cap()) return e;
    hipLaunchKernelGGL((fft_cols_mixed_kernel<1>), dim3(N * (W / cw)), dim3(256), mixed_cols_lds(H), s, work, tw, y0s, masks, mask_n, mu,
                       tact, H, W, cw, 0, 0);
    return hipGetLastError();
}
hipError_t launch_fft_rows_inv_admm(const float2* work, const float* x, float2* z, float2* u, const float2* tw, const float* tact, int N,
                                    int H, int W, hipStream_t s) {
    const int rpb = mixed_rows_per_block(W);
    hipLaunchKernelGGL((fft_rows_mixed_kernel<2>), dim3(N * (H / rpb)), dim3(256), mixed_rows_lds(W), s, work, z, x, u, tw, tact, H, W, rpb,
                       1, 0);
    return hipGetLastError();
}

}  // namespace mixed

}  // namespace pnp
