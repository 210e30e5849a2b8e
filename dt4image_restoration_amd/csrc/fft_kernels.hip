// k-space data-fidelity stage of the PnP-ADMM iteration for gfx950 (MI355X).
//
// Replaces, per iteration (/root/reference/evaluation/env.py:87-93):
//     z = fft(x + u);  z[mask] = ((mu*z + y0)/(1+mu))[mask];  z = ifft(z);  u = u + x - z
// where fft/ifft are the centred orthonormal transforms of evaluation/utils/transformations.py:6-19
// (ifftshift -> fftn/ifftn(norm='ortho') -> fftshift, i.e. 4 roll copies per iteration).
//
// Shift folding (H, W even): with S = fftshift and sgn[k1,k2] = (-1)^(k1+k2),
//     ifft_c(where(m, (mu*fft_c(v) + y0)/(1+mu), fft_c(v)))
//   = IFFT(where(S m, (mu*FFT(v) + sgn*S y0)/(1+mu), FFT(v)))          (plain, unshifted transforms)
// so pnp_reset pre-shifts the mask and y0 once and the iteration moves no roll traffic at all.
//
// Three launches, each a Stockham autosort FFT (radix-4 passes + one radix-2 pass when log2 L is odd)
// held entirely in LDS, HBM traffic coalesced in >= 128-B runs:
//   rows-forward : v = x + u -> row FFT -> work                       (reads 12 B/px, writes 8)
//   cols + prox  : column FFT -> masked closed-form solve -> inverse column FFT, in place in `work`
//                  (16 adjacent columns per workgroup so every global access is a 128-B line)
//   rows-inverse : row IFFT -> z;  u += x - z                         (reads 20 B/px, writes 16)
// Twiddles come from a host-computed (double precision) table.
// Every kernel here serves handles whose H and W are both powers of two; a side of 2^a * 5^b (80 .. 800) runs the
// mixed-radix kernels of fft_mixed_kernels.hip instead.
#include "pnp_internal.h"
#include "fft_common.h"
#include "block_reduce.h"

namespace pnp {

// `lines` independent length-L transforms, line i at [i*lstr, i*lstr+L) of src; ping-pongs src <-> dst.
// tw[m] = exp(-2 pi i m / L) in LDS.  Caller has synchronised the loads; returns the buffer holding the
// result (synchronised).
template <bool INV>
__device__ float2* fft_lines(float2* src, float2* dst, const float2* tw, int L, int lines, int lstr) {
    const int tid = threadIdx.x, nth = blockDim.x;
    int Ns = 1;
    const int per4 = L >> 2;
    while (Ns * 4 <= L) {
        const int total = lines * per4;
        const int tstep = L / (4 * Ns);
        for (int idx = tid; idx < total; idx += nth) {
            const int line = idx / per4, j = idx - line * per4;
            const int k = j & (Ns - 1);
            const float2* sp = src + line * lstr + j;
            float2 v0 = sp[0], v1 = sp[per4], v2 = sp[2 * per4], v3 = sp[3 * per4];
            if (Ns > 1) {
                float2 w1 = tw[k * tstep], w2 = tw[2 * k * tstep], w3 = tw[3 * k * tstep];
                if (INV) { w1.y = -w1.y; w2.y = -w2.y; w3.y = -w3.y; }
                v1 = cmul(v1, w1); v2 = cmul(v2, w2); v3 = cmul(v3, w3);
            }
            const float2 t0 = cadd(v0, v2), t1 = csub(v0, v2), t2 = cadd(v1, v3);
            const float2 d = csub(v1, v3);
            const float2 t3 = INV ? make_float2(-d.y, d.x) : make_float2(d.y, -d.x);   // (+/- i) * d
            float2* dp = dst + line * lstr + ((j - k) << 2) + k;
            dp[0] = cadd(t0, t2);
            dp[Ns] = cadd(t1, t3);
            dp[2 * Ns] = csub(t0, t2);
            dp[3 * Ns] = csub(t1, t3);
        }
        __syncthreads();
        float2* t = src; src = dst; dst = t;
        Ns <<= 2;
    }
    if (Ns < L) {   // one radix-2 pass (Ns == L/2)
        const int per2 = L >> 1;
        const int total = lines * per2;
        for (int idx = tid; idx < total; idx += nth) {
            const int line = idx / per2, j = idx - line * per2;
            const int k = j & (Ns - 1);
            const float2* sp = src + line * lstr + j;
            float2 v0 = sp[0], v1 = sp[per2];
            float2 w = tw[k * (L / (2 * Ns))];
            if (INV) w.y = -w.y;
            v1 = cmul(v1, w);
            float2* dp = dst + line * lstr + ((j - k) << 1) + k;
            dp[0] = cadd(v0, v1);
            dp[Ns] = csub(v0, v1);
        }
        __syncthreads();
        float2* t = src; src = dst; dst = t;
    }
    return src;
}

// Compile-time sizes (L = 128 / 256 / 512, the sizes of BASELINE's configs): every pass is fully unrolled and reads all of a
// thread's butterflies (IT x 4 points + twiddles) before it computes, so LDS latency is paid once per pass instead of once
// per butterfly.  256 threads; LINES * L / 4 must be a multiple of 256.
template <bool INV, int L, int LINES, int LSTR, int NS, bool INPLACE = false>
__device__ __forceinline__ void fft_pass4(const float2* src, float2* dst, const float2* __restrict__ tw) {
    constexpr int per4 = L / 4, IT = LINES * per4 / 256, tstep = L / (4 * NS);
    static_assert((LINES * per4) % 256 == 0, "whole batches of 256 butterflies");
    const int tid = threadIdx.x;
    float2 v[IT][4], w[IT][3];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = tid + it * 256;
        const int line = idx / per4, j = idx % per4;
        const float2* sp = src + line * LSTR + j;
        v[it][0] = sp[0]; v[it][1] = sp[per4]; v[it][2] = sp[2 * per4]; v[it][3] = sp[3 * per4];
        if (NS > 1) {
            const int k = j & (NS - 1);
            w[it][0] = tw[k * tstep]; w[it][1] = tw[2 * k * tstep]; w[it][2] = tw[3 * k * tstep];
        }
    }
    if (INPLACE) __syncthreads();                          // src == dst: every read of the pass before any write
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = tid + it * 256;
        const int line = idx / per4, j = idx % per4;
        const int k = j & (NS - 1);
        float2 v0 = v[it][0], v1 = v[it][1], v2 = v[it][2], v3 = v[it][3];
        if (NS > 1) {
            float2 w1 = w[it][0], w2 = w[it][1], w3 = w[it][2];
            if (INV) { w1.y = -w1.y; w2.y = -w2.y; w3.y = -w3.y; }
            v1 = cmul(v1, w1); v2 = cmul(v2, w2); v3 = cmul(v3, w3);
        }
        const float2 t0 = cadd(v0, v2), t1 = csub(v0, v2), t2 = cadd(v1, v3);
        const float2 d = csub(v1, v3);
        const float2 t3 = INV ? make_float2(-d.y, d.x) : make_float2(d.y, -d.x);   // (+/- i) * d
        float2* dp = dst + line * LSTR + ((j - k) << 2) + k;
        dp[0] = cadd(t0, t2);
        dp[NS] = cadd(t1, t3);
        dp[2 * NS] = csub(t0, t2);
        dp[3 * NS] = csub(t1, t3);
    }
}

template <bool INV, int L, int LINES, int LSTR, int NS, bool INPLACE = false>
__device__ __forceinline__ void fft_pass2(const float2* src, float2* dst, const float2* __restrict__ tw) {
    constexpr int per2 = L / 2, IT = LINES * per2 / 256;
    static_assert((LINES * per2) % 256 == 0 && NS * 2 == L, "radix-2 tail");
    const int tid = threadIdx.x;
    float2 v[IT][2], w[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = tid + it * 256;
        const int line = idx / per2, j = idx % per2;
        const float2* sp = src + line * LSTR + j;
        v[it][0] = sp[0]; v[it][1] = sp[per2];
        w[it] = tw[j & (NS - 1)];                              // k * (L / (2 NS)) = k
    }
    if (INPLACE) __syncthreads();
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = tid + it * 256;
        const int line = idx / per2, j = idx % per2;
        const int k = j & (NS - 1);
        float2 ww = w[it];
        if (INV) ww.y = -ww.y;
        const float2 v1 = cmul(v[it][1], ww);
        float2* dp = dst + line * LSTR + ((j - k) << 1) + k;
        dp[0] = cadd(v[it][0], v1);
        dp[NS] = csub(v[it][0], v1);
    }
}

// Same contract as fft_lines (caller has synchronised the loads; returns the buffer holding the synchronised result).
template <bool INV, int L, int LINES, int LSTR>
__device__ __forceinline__ float2* fft_lines_ct(float2* src, float2* dst, const float2* tw) {
#define PNP_FFT_STEP(NS_)                                                                              \
    if constexpr (NS_ * 4 <= L) {                                                                      \
        fft_pass4<INV, L, LINES, LSTR, NS_>(src, dst, tw);                                             \
        __syncthreads();                                                                               \
        float2* t_ = src; src = dst; dst = t_;                                                         \
    }
    PNP_FFT_STEP(1) PNP_FFT_STEP(4) PNP_FFT_STEP(16) PNP_FFT_STEP(64) PNP_FFT_STEP(256)
#undef PNP_FFT_STEP
    constexpr int NS4 = L >= 1024 ? 1024 : (L >= 256 ? 256 : (L >= 64 ? 64 : (L >= 16 ? 16 : (L >= 4 ? 4 : 1))));
    if constexpr (NS4 < L) {
        fft_pass2<INV, L, LINES, LSTR, NS4>(src, dst, tw);
        __syncthreads();
        float2* t_ = src; src = dst; dst = t_;
    }
    return src;
}

// In place in ONE buffer (half the LDS, twice the barriers): the register batch of a pass is the second buffer.
template <bool INV, int L, int LINES, int LSTR>
__device__ __forceinline__ void fft_lines_inplace(float2* buf, const float2* tw) {
#define PNP_FFT_STEP(NS_)                                                                              \
    if constexpr (NS_ * 4 <= L) {                                                                      \
        fft_pass4<INV, L, LINES, LSTR, NS_, true>(buf, buf, tw);                                       \
        __syncthreads();                                                                               \
    }
    PNP_FFT_STEP(1) PNP_FFT_STEP(4) PNP_FFT_STEP(16) PNP_FFT_STEP(64) PNP_FFT_STEP(256)
#undef PNP_FFT_STEP
    constexpr int NS4 = L >= 1024 ? 1024 : (L >= 256 ? 256 : (L >= 64 ? 64 : (L >= 16 ? 16 : (L >= 4 ? 4 : 1))));
    if constexpr (NS4 < L) {
        fft_pass2<INV, L, LINES, LSTR, NS4, true>(buf, buf, tw);
        __syncthreads();
    }
}

// ---- 256-point lines as TWO radix-16 passes with the 16-point transforms in registers (2 LDS round trips per transform
// instead of the 4 of the radix-4 passes) ------------------------------------------------------------------------------------
// In place in one buffer; element i of a line lives at i + (i >> 4) (one pad element per 16: the Stockham passes read
// positions j + 16 m and write 16 j + q / j + 16 q, which the skew turns into j + 17 m, 17 j + q, j + 17 q - lanes j hit
// distinct banks in all three), lines SK256_LS elements apart.
static constexpr int SK256_LS = 273;
__device__ __forceinline__ int sk256(int i) { return i + (i >> 4); }

// v[0..15] -> its 16-point DFT, result X[p + 4 s] in v[4 p + s] (two radix-4 stages, constant twiddles w16^(r p) between)
template <bool INV>
__device__ __forceinline__ void dft16_inplace(float2* v) {
    constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, R2 = 0.70710678118654752f;
#pragma unroll
    for (int r = 0; r < 4; ++r) dft4_inplace<INV>(v[r], v[r + 4], v[r + 8], v[r + 12]);   // A[r][p] now in v[r + 4 p]
    // w16^e = (cos, -sin)(2 pi e / 16) forward, conjugate inverse; e = r * p
    auto tw = [&](float2& x, float c, float sn) { x = cmul(x, make_float2(c, INV ? sn : -sn)); };
    tw(v[1 + 4], C1, S1);   tw(v[2 + 4], R2, R2);   tw(v[3 + 4], S1, C1);           // p = 1: e = 1, 2, 3
    tw(v[1 + 8], R2, R2);   tw(v[2 + 8], 0.f, 1.f); tw(v[3 + 8], -R2, R2);          // p = 2: e = 2, 4, 6
    tw(v[1 + 12], S1, C1);  tw(v[2 + 12], -R2, R2); tw(v[3 + 12], -C1, -S1);        // p = 3: e = 3, 6, 9
#pragma unroll
    for (int p = 0; p < 4; ++p) dft4_inplace<INV>(v[4 * p], v[4 * p + 1], v[4 * p + 2], v[4 * p + 3]);
}

// LINES (<= 16) lines of 256 points, 256 threads: thread (line, j) owns one radix-16 butterfly per pass.
template <bool INV, int LINES>
__device__ __forceinline__ void fft256_radix16_inplace(float2* buf, const float2* __restrict__ tw) {
    const int tid = threadIdx.x, line = tid >> 4, j = tid & 15;
    const bool on = line < LINES;
    float2* const base = buf + line * SK256_LS;
    float2 v[16];
    // pass 1 (Ns = 1): no twiddles; X[q] -> position 16 j + q
    if (on) {
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = base[j + 17 * m];
    }
    __syncthreads();                                       // in place: every read of the pass before any write
    if (on) {
        dft16_inplace<INV>(v);
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) base[17 * j + p + 4 * s2] = v[4 * p + s2];
    }
    __syncthreads();
    // pass 2 (Ns = 16, k = j): x[m] *= w256^(m j); X[q] -> position j + 16 q
    if (on) {
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            v[m] = base[j + 17 * m];
            if (m > 0) {
                float2 w = tw[m * j];
                if (INV) w.y = -w.y;
                v[m] = cmul(v[m], w);
            }
        }
    }
    __syncthreads();
    if (on) {
        dft16_inplace<INV>(v);
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) base[j + 17 * (p + 4 * s2)] = v[4 * p + s2];
    }
    __syncthreads();
}

// ---- 512-point lines as THREE radix-8 passes with the 8-point transforms in registers (round 5; BASELINE configs[4] is 512 x 512: its
// passes were the generic radix-4 x 4 + radix-2 ones, five LDS round trips per transform and 0.38-0.44 of their LDS cycles in bank
// conflicts, profiles/r04_pmc_current_16x512x512_f32.md) ------------------------------------------------------------------------------
// In place in one buffer; element i of a line lives at i + (i >> 3) (one pad element per 8).  A butterfly b (0..63) of a Stockham pass
// reads positions b + 64 m and writes 8 b + q (Ns = 1), 64 (b >> 3) + (b & 7) + 8 q (Ns = 8), b + 64 q (Ns = 64); under the skew these
// are sk(b) + 72 m, 9 b + q, 72 (b >> 3) + (b & 7) + 9 q, sk(b) + 72 q: consecutive lanes b stay on distinct banks in all of them.
// Lines SK512_LS elements apart.
static constexpr int SK512_LS = 577;   // odd: the column kernel stages and solves ACROSS lines (8 lanes = 8 lines at one row): a stride that is a multiple of the bank count puts them all on one bank (measured: bank-conflict share 0.65 with 576)
__device__ __forceinline__ int sk512(int i) { return i + (i >> 3); }

// v[0..7] -> its 8-point DFT, result X[q] in v[4 (q & 1) + (q >> 1)] (one radix-2 stage, constant twiddles w8^k, two radix-4 stages)
template <bool INV>
__device__ __forceinline__ void dft8_inplace(float2* v) {
    constexpr float R2 = 0.70710678118654752f;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const float2 t = v[k]; v[k] = cadd(t, v[k + 4]); v[k + 4] = csub(t, v[k + 4]); }
    // w8^k = (cos, -sin)(2 pi k / 8) forward, conjugate inverse
    v[5] = cmul(v[5], make_float2(R2, INV ? R2 : -R2));
    v[6] = INV ? make_float2(-v[6].y, v[6].x) : make_float2(v[6].y, -v[6].x);
    v[7] = cmul(v[7], make_float2(-R2, INV ? R2 : -R2));
    dft4_inplace<INV>(v[0], v[1], v[2], v[3]);             // X[0], X[2], X[4], X[6]
    dft4_inplace<INV>(v[4], v[5], v[6], v[7]);             // X[1], X[3], X[5], X[7]
}

// LINES lines of 512 points, 256 threads, TPL threads per line (LINES * TPL <= 256): thread (line, j) owns the radix-8 butterflies
// j, j + TPL, ... of its line in every pass (64 / TPL of them: two with 8 lines per workgroup, one with 4).
template <bool INV, int LINES, int TPL>
__device__ __forceinline__ void fft512_radix8_inplace(float2* buf, const float2* __restrict__ tw) {
    static_assert((TPL == 32 || TPL == 64) && LINES * TPL <= 256, "threads per line");
    constexpr int NB = 64 / TPL;
    const int tid = threadIdx.x, line = tid / TPL, j = tid % TPL;
    const bool on = line < LINES;
    float2* const base = buf + line * SK512_LS;
    float2 v[NB][8];
    auto xq = [](int q) { return 4 * (q & 1) + (q >> 1); };  // where dft8_inplace leaves X[q]
    // pass 1 (Ns = 1): no twiddles; X[q] -> position 8 b + q
    if (on) {
#pragma unroll
        for (int h = 0; h < NB; ++h)
#pragma unroll
            for (int m = 0; m < 8; ++m) v[h][m] = base[sk512(j + TPL * h) + 72 * m];
    }
    __syncthreads();                                       // in place: every read of the pass before any write
    if (on) {
#pragma unroll
        for (int h = 0; h < NB; ++h) {
            dft8_inplace<INV>(v[h]);
#pragma unroll
            for (int q = 0; q < 8; ++q) base[9 * (j + TPL * h) + q] = v[h][xq(q)];
        }
    }
    __syncthreads();
    // pass 2 (Ns = 8, k = b & 7): x[m] *= w64^(m k); X[q] -> position 64 (b >> 3) + k + 8 q
    if (on) {
#pragma unroll
        for (int h = 0; h < NB; ++h)
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                v[h][m] = base[sk512(j + TPL * h) + 72 * m];
                if (m > 0) {
                    float2 w = tw[8 * m * (j & 7)];
                    if (INV) w.y = -w.y;
                    v[h][m] = cmul(v[h][m], w);
                }
            }
    }
    __syncthreads();
    if (on) {
#pragma unroll
        for (int h = 0; h < NB; ++h) {
            dft8_inplace<INV>(v[h]);
            const int b = j + TPL * h;
#pragma unroll
            for (int q = 0; q < 8; ++q) base[72 * (b >> 3) + (b & 7) + 9 * q] = v[h][xq(q)];
        }
    }
    __syncthreads();
    // pass 3 (Ns = 64, k = b): x[m] *= w512^(m b); X[q] -> position b + 64 q
    if (on) {
#pragma unroll
        for (int h = 0; h < NB; ++h)
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                v[h][m] = base[sk512(j + TPL * h) + 72 * m];
                if (m > 0) {
                    float2 w = tw[m * (j + TPL * h)];
                    if (INV) w.y = -w.y;
                    v[h][m] = cmul(v[h][m], w);
                }
            }
    }
    __syncthreads();
    if (on) {
#pragma unroll
        for (int h = 0; h < NB; ++h) {
            dft8_inplace<INV>(v[h]);
#pragma unroll
            for (int q = 0; q < 8; ++q) base[sk512(j + TPL * h) + 72 * q] = v[h][xq(q)];
        }
    }
    __syncthreads();
}

static constexpr int ROW_ELEMS = 2048;   // complex elements per workgroup in the row passes

// MODE 0 generic (in -> out, index shifts), 1 ADMM forward (x + u -> work), 2 ADMM inverse (work -> z, u), 3 real image x -> out (forward,
// pnp_residuals' data misfit; stores as MODE 0 with shift_out = 0)
// R16 (256-point rows of the ADMM passes): SIXTEEN rows per workgroup, each as two radix-16 passes in place in one skewed buffer
// (fft256_radix16_inplace: every thread owns a butterfly, 2 LDS round trips per transform instead of 4, and the skew keeps the
// Stockham strides off each other's banks - the radix-4 passes over unpadded 256-element lines spent 0.40 of their LDS cycles
// in bank conflicts, profiles/r02_pmc_current.md).
// fft_rows_body: rows [y0, y0 + rpb) of slice n, by ONE workgroup whose LDS is smem
template <int MODE, int LC, bool R16>
__device__ __forceinline__ void fft_rows_body(float2* smem, const float2* in, float2* out,
                                              const float* __restrict__ x, float2* __restrict__ u,
                                              const float2* __restrict__ twg,
                                              int H, int W, int rpb, int inverse, int shift_in, int shift_out, int n, int y0) {
    static_assert(!R16 || ((LC == 256 || LC == 512) && MODE != 0), "register-resident passes: the 256- / 512-point ADMM passes");
    constexpr int RE = (R16 && LC == 256) ? 4096 : ROW_ELEMS;   // elements per workgroup (R16: 16 rows of 256 / 4 rows of 512 - every thread owns one butterfly per pass)
    constexpr int RLS = LC == 512 ? SK512_LS : SK256_LS;   // (R16) skewed line stride
    auto slot = [&](int e) { return !R16 ? e : (LC == 512 ? (e >> 9) * SK512_LS + sk512(e & 511) : (e >> 8) * SK256_LS + sk256(e & 255)); };
    float2* buf0 = smem;
    float2* buf1 = smem + (R16 ? 0 : rpb * W);
    float2* tw = smem + (R16 ? (RE / (LC > 0 ? LC : 1)) * RLS : 2 * rpb * W);
    const size_t base = ((size_t)n * H + y0) * W;
    const int tot = rpb * W;
    for (int i = threadIdx.x; i < W; i += blockDim.x) tw[i] = twg[i];
    // global accesses in batches of NB independent requests per thread (a plain loop with a run-time trip count waits for
    // every load before issuing the next: 8 serial HBM round trips per workgroup)
    constexpr int NB = 8;
    const int lw = 31 - __builtin_clz(W);                  // W is a power of two
    for (int e0 = threadIdx.x; e0 < tot; e0 += NB * 256) {
        float2 v[NB];
        float xv[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int e = e0 + k * 256;
            if (e < tot) {
                if (MODE == 1) { v[k] = u[base + e]; xv[k] = x[base + e]; }
                else if (MODE == 3) xv[k] = x[base + e];
                else { const int r = e >> lw, c = e & (W - 1); v[k] = in[base + (size_t)r * W + (c ^ shift_in)]; }
            }
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int e = e0 + k * 256;
            if (e < tot) buf0[slot(e)] = MODE == 1 ? make_float2(xv[k] + v[k].x, v[k].y) : (MODE == 3 ? make_float2(xv[k], 0.f) : v[k]);
        }
    }
    __syncthreads();
    const bool inv = (MODE == 2) || (MODE == 0 && inverse);
    float2* res;
    if constexpr (R16 && LC == 512) {                      // W == 512, 4 rows per workgroup (checked by the launcher)
        if constexpr (MODE == 2) fft512_radix8_inplace<true, 4, 64>(buf0, tw);
        else fft512_radix8_inplace<false, 4, 64>(buf0, tw);
        res = buf0;
    } else if constexpr (R16) {                            // W == 256, 16 rows per workgroup (checked by the launcher)
        if constexpr (MODE == 2) fft256_radix16_inplace<true, RE / 256>(buf0, tw);
        else fft256_radix16_inplace<false, RE / 256>(buf0, tw);
        res = buf0;
    } else if constexpr (LC > 0) {                         // W == LC, rpb == ROW_ELEMS / LC (checked by the launcher)
        if constexpr (MODE == 2) res = fft_lines_ct<true, LC, ROW_ELEMS / LC, LC>(buf0, buf1, tw);
        else if constexpr (MODE == 1) res = fft_lines_ct<false, LC, ROW_ELEMS / LC, LC>(buf0, buf1, tw);
        else res = inv ? fft_lines_ct<true, LC, ROW_ELEMS / LC, LC>(buf0, buf1, tw) : fft_lines_ct<false, LC, ROW_ELEMS / LC, LC>(buf0, buf1, tw);
    } else {
        res = inv ? fft_lines<true>(buf0, buf1, tw, W, rpb, W) : fft_lines<false>(buf0, buf1, tw, W, rpb, W);
    }
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
                float2 v = res[slot(e)];
                v.x *= sc; v.y *= sc;
                if (MODE == 2) {
                    out[base + e] = v;                                                   // z
                    u[base + e] = make_float2(uu[k].x + xv[k] - v.x, uu[k].y - v.y);     // u + x - z
                } else {
                    const int r = e >> lw, c = e & (W - 1);
                    out[base + (size_t)r * W + (c ^ shift_out)] = v;
                }
            }
        }
    }
}

template <int MODE, int LC, bool R16 = false>
__global__ __launch_bounds__(256) void fft_rows_kernel(const float2* in, float2* out,
                                                       const float* __restrict__ x, float2* __restrict__ u,
                                                       const float2* __restrict__ twg, const float* __restrict__ tact,
                                                       int H, int W, int rpb, int inverse, int shift_in, int shift_out) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int blocks_per_img = H / rpb;
    // ADMM passes: the same (slice -> XCD) map as fft_cols_kernel - workgroups b, b + 8, ... share an XCD, each XCD takes a contiguous range of
    // slices - so that the scratch a slice's row pass wrote is in the L2 of the XCD whose column pass reads it, and again for the inverse rows
    int vb = blockIdx.x;
    if (MODE != 0 && (gridDim.x & 7) == 0) vb = (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
    const int n = vb / blocks_per_img;
    const int y0 = (vb % blocks_per_img) * rpb;
    if (MODE != 0 && tact != nullptr && tact[n] > 0.5f) return;
    fft_rows_body<MODE, LC, R16>(smem, in, out, x, u, twg, H, W, rpb, inverse, shift_in, shift_out, n, y0);
}

// Column pass over CW adjacent columns of one slice.  MODE 0 generic in-place transform with row-index
// shifts; MODE 1 forward -> prox -> inverse (ADMM).
// fft_cols_body: columns [x0, x0 + cw) of slice n, by ONE workgroup whose LDS is smem
template <int MODE, int LC>
__device__ __forceinline__ void fft_cols_body(float2* smem, float2* __restrict__ data, const float2* __restrict__ twg,
                                              const float2* __restrict__ y0s, const uint8_t* __restrict__ masks,
                                              int mask_n, const float* __restrict__ mu, int H, int W, int cw,
                                              int inverse, int shift_in, int shift_out, int n, int x0) {
    constexpr bool R16 = MODE == 1 && LC == 256;           // 256-point columns of the ADMM pass: radix-16 passes, skewed lines
    constexpr bool R8 = MODE == 1 && LC == 512;            // 512-point columns: radix-8 passes, skewed lines
    const int lstr = R16 ? SK256_LS : (R8 ? SK512_LS : H + 1);
    float2* buf0 = smem;
    float2* buf1 = smem + cw * lstr;
    float2* tw = smem + ((MODE == 1 && LC > 0) ? 1 : 2) * cw * lstr;   // the unrolled ADMM variant works in place in buf0
    float2* img = data + (size_t)n * H * W;
    const int tot = cw * H;
    for (int i = threadIdx.x; i < H; i += blockDim.x) tw[i] = twg[i];
    constexpr int NB = 8;                                  // independent global requests per thread and batch
    const int lcw = 31 - __builtin_clz(cw);                // cw is a power of two
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
            if (e < tot) buf0[(e & (cw - 1)) * lstr + (R16 ? sk256(e >> lcw) : (R8 ? sk512(e >> lcw) : ((e >> lcw) ^ shift_in)))] = v[k];
        }
    }
    __syncthreads();
    const float sc = rsqrtf((float)H);
    if (MODE == 0) {
        float2* res = inverse ? fft_lines<true>(buf0, buf1, tw, H, cw, lstr) : fft_lines<false>(buf0, buf1, tw, H, cw, lstr);
        for (int e = threadIdx.x; e < tot; e += 256) {
            const int r = e >> lcw, c = e & (cw - 1);
            float2 v = res[c * lstr + (r ^ shift_out)];
            v.x *= sc; v.y *= sc;
            img[(size_t)r * W + x0 + c] = v;
        }
    } else if constexpr (LC > 0) {
        // H == LC, cw == CWC (checked by the launcher): the k-space constants of this strip are fetched BEFORE the forward
        // transform and sit in registers under it; all passes unrolled.
        constexpr int CWC = LC <= 256 ? 16 : (LC <= 512 ? 8 : 4), LS = R16 ? SK256_LS : (R8 ? SK512_LS : LC + 1), PER = CWC * LC / 256;
        auto rpos = [](int r) { return R16 ? sk256(r) : (R8 ? sk512(r) : r); };
        const float m = mu[n];
        const float inv1m = 1.f + m;
        const float2* y0n = y0s + (size_t)n * H * W;
        const uint8_t* mk = masks + (mask_n > 1 ? (size_t)n * H * W : 0);
        float2 yy[PER];
        uint8_t mm[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int e = threadIdx.x + k * 256;
            const size_t g = (size_t)(e / CWC) * W + x0 + (e % CWC);
            mm[k] = mk[g];
            yy[k] = y0n[g];
        }
        if constexpr (R16) fft256_radix16_inplace<false, CWC>(buf0, tw);
        else if constexpr (R8) fft512_radix8_inplace<false, CWC, 32>(buf0, tw);
        else fft_lines_inplace<false, LC, CWC, LS>(buf0, tw);
        float2* const res = buf0;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int e = threadIdx.x + k * 256;
            const int r = e / CWC, c = e % CWC;
            float2 v = res[c * LS + rpos(r)];
            v.x *= sc; v.y *= sc;                           // now the orthonormal FFT2 of x + u
            if (mm[k]) {                                    // sampled k-space bin: closed-form solve
                v.x = (m * v.x + yy[k].x) / inv1m;
                v.y = (m * v.y + yy[k].y) / inv1m;
            }
            res[c * LS + rpos(r)] = v;
        }
        __syncthreads();
        if constexpr (R16) fft256_radix16_inplace<true, CWC>(res, tw);
        else if constexpr (R8) fft512_radix8_inplace<true, CWC, 32>(res, tw);
        else fft_lines_inplace<true, LC, CWC, LS>(res, tw);
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int e = threadIdx.x + k * 256;
            const int r = e / CWC, c = e % CWC;
            float2 v = res[c * LS + rpos(r)];
            v.x *= sc; v.y *= sc;
            img[(size_t)r * W + x0 + c] = v;
        }
    } else {
        float2* res = fft_lines<false>(buf0, buf1, tw, H, cw, lstr);
        float2* oth = (res == buf0) ? buf1 : buf0;
        const float m = mu[n];
        const float inv1m = 1.f + m;
        const float2* y0n = y0s + (size_t)n * H * W;
        const uint8_t* mk = masks + (mask_n > 1 ? (size_t)n * H * W : 0);
        for (int e0 = threadIdx.x; e0 < tot; e0 += NB * 256) {
            float2 yy[NB];
            uint8_t mm[NB];
#pragma unroll
            for (int k = 0; k < NB; ++k) {                      // mask and y0 of the batch in flight together; y0 is read for
                const int e = e0 + k * 256;                     // unsampled bins too (a radial mask leaves < 1 % of the 128-B
                if (e < tot) {                                  // lines untouched, so predicating it saves nothing)
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
        float2* r2 = fft_lines<true>(res, oth, tw, H, cw, lstr);
        for (int e = threadIdx.x; e < tot; e += 256) {
            const int r = e >> lcw, c = e & (cw - 1);
            float2 v = r2[c * lstr + r];
            v.x *= sc; v.y *= sc;
            img[(size_t)r * W + x0 + c] = v;
        }
    }
}

template <int MODE, int LC>
__global__ __launch_bounds__(256) void fft_cols_kernel(float2* __restrict__ data, const float2* __restrict__ twg,
                                                       const float2* __restrict__ y0s, const uint8_t* __restrict__ masks,
                                                       int mask_n, const float* __restrict__ mu,
                                                       const float* __restrict__ tact, int H, int W, int cw,
                                                       int inverse, int shift_in, int shift_out) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int strips = W / cw;
    // Workgroups b, b + 8, b + 16, ... share an XCD (and its L2) and are dispatched back to back: each XCD walks a CONTIGUOUS range of
    // (slice, strip) pairs, so the two 8-column strips that share every 128-byte line of a 512-point slice (and of its y0 / mask) run
    // side by side on ONE L2 - the line comes from HBM once and its two half-line stores merge before they leave (round 5: the strips of a
    // line pair used to sit on different XCDs, 2.6 x the algorithmic bytes moved at 512 x 512, profiles/r04_pmc_current_16x512x512_f32.md)
    int vb = blockIdx.x;
    if ((gridDim.x & 7) == 0) vb = (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
    const int n = vb / strips;
    const int x0 = (vb % strips) * cw;
    if (MODE == 1 && tact != nullptr && tact[n] > 0.5f) return;
    fft_cols_body<MODE, LC>(smem, data, twg, y0s, masks, mask_n, mu, H, W, cw, inverse, shift_in, shift_out, n, x0);
}

// ---- 128 x 128: the whole data-fidelity stage of a slice in ONE workgroup ------------------------------------------------
// A 128 x 128 complex64 slice is 128 KiB, less than the 160 KiB of LDS a workgroup may own: v = x + u is read once, both
// forward transforms, the masked solve, both inverse transforms and the dual update happen in LDS, z and u are written once.
// HBM traffic = the algorithmic 37 B/px (x 4 + u 8 + y0 8 + mask 1 read, z 8 + u 8 written) instead of the 81 B/px of the
// three-launch path, and one launch instead of three on the reference's own problem size (env.py:44,64: 128 x 128).
// In-place Stockham passes with a register batch as the second buffer (every butterfly of a pass is read, barrier, written);
// 1024 threads: 4 radix-4 butterflies (8 radix-2) per thread and pass.  Lines are rows (element stride 1, line stride 129) or
// columns (element stride 129, line stride 1) of the same padded image: both access patterns are bank-conflict-free.
template <bool INV, int L, int LINES, int LS, int ES, int NS, int NT>
__device__ __forceinline__ void fft_pass4_strided(float2* buf, const float2* __restrict__ tw) {
    constexpr int per4 = L / 4, IT = LINES * per4 / NT, tstep = L / (4 * NS);
    static_assert((LINES * per4) % NT == 0, "whole batches of butterflies");
    const int tid = threadIdx.x;
    float2 v[IT][4], w[IT][3];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = tid + it * NT;
        const int line = idx / per4, j = idx % per4;
        const float2* sp = buf + line * LS + j * ES;
        v[it][0] = sp[0]; v[it][1] = sp[per4 * ES]; v[it][2] = sp[2 * per4 * ES]; v[it][3] = sp[3 * per4 * ES];
        if (NS > 1) {
            const int k = j & (NS - 1);
            w[it][0] = tw[k * tstep]; w[it][1] = tw[2 * k * tstep]; w[it][2] = tw[3 * k * tstep];
        }
    }
    __syncthreads();                                       // in place: every read of the pass before any write
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = tid + it * NT;
        const int line = idx / per4, j = idx % per4;
        const int k = j & (NS - 1);
        float2 v0 = v[it][0], v1 = v[it][1], v2 = v[it][2], v3 = v[it][3];
        if (NS > 1) {
            float2 w1 = w[it][0], w2 = w[it][1], w3 = w[it][2];
            if (INV) { w1.y = -w1.y; w2.y = -w2.y; w3.y = -w3.y; }
            v1 = cmul(v1, w1); v2 = cmul(v2, w2); v3 = cmul(v3, w3);
        }
        const float2 t0 = cadd(v0, v2), t1 = csub(v0, v2), t2 = cadd(v1, v3);
        const float2 d = csub(v1, v3);
        const float2 t3 = INV ? make_float2(-d.y, d.x) : make_float2(d.y, -d.x);   // (+/- i) * d
        float2* dp = buf + line * LS + (((j - k) << 2) + k) * ES;
        dp[0] = cadd(t0, t2);
        dp[NS * ES] = cadd(t1, t3);
        dp[2 * NS * ES] = csub(t0, t2);
        dp[3 * NS * ES] = csub(t1, t3);
    }
    __syncthreads();
}

template <bool INV, int L, int LINES, int LS, int ES, int NS, int NT>
__device__ __forceinline__ void fft_pass2_strided(float2* buf, const float2* __restrict__ tw) {
    constexpr int per2 = L / 2, IT = LINES * per2 / NT;
    static_assert((LINES * per2) % NT == 0 && NS * 2 == L, "radix-2 tail");
    const int tid = threadIdx.x;
    float2 v[IT][2], w[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = tid + it * NT;
        const int line = idx / per2, j = idx % per2;
        const float2* sp = buf + line * LS + j * ES;
        v[it][0] = sp[0]; v[it][1] = sp[per2 * ES];
        w[it] = tw[j & (NS - 1)];
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = tid + it * NT;
        const int line = idx / per2, j = idx % per2;
        const int k = j & (NS - 1);
        float2 ww = w[it];
        if (INV) ww.y = -ww.y;
        const float2 v1 = cmul(v[it][1], ww);
        float2* dp = buf + line * LS + (((j - k) << 1) + k) * ES;
        dp[0] = cadd(v[it][0], v1);
        dp[NS * ES] = csub(v[it][0], v1);
    }
    __syncthreads();
}

// 128-point transforms of all 128 lines: 4 * 4 * 4 * 2
template <bool INV, int LS, int ES, int NT>
__device__ __forceinline__ void fft128_all_lines(float2* buf, const float2* tw) {
    fft_pass4_strided<INV, 128, 128, LS, ES, 1, NT>(buf, tw);
    fft_pass4_strided<INV, 128, 128, LS, ES, 4, NT>(buf, tw);
    fft_pass4_strided<INV, 128, 128, LS, ES, 16, NT>(buf, tw);
    fft_pass2_strided<INV, 128, 128, LS, ES, 64, NT>(buf, tw);
}

__global__ __launch_bounds__(1024) void admm_slice128_kernel(const float* __restrict__ x, float2* __restrict__ z,
                                                             float2* u, const float2* __restrict__ twg,
                                                             const float2* __restrict__ y0s, const uint8_t* __restrict__ masks,
                                                             int mask_n, const float* __restrict__ mu,
                                                             const float* __restrict__ tact) {
    constexpr int L = 128, LP = L + 1, NT = 1024, PER = L * L / NT, HB = PER / 2;
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    float2* const buf = smem;                              // [128][129]
    float2* const tw = smem + L * LP;
    const int n = blockIdx.x, tid = threadIdx.x;
    if (tact != nullptr && tact[n] > 0.5f) return;
    const size_t base = (size_t)n * L * L;
    if (tid < L) tw[tid] = twg[tid];
    // global accesses in batches of 8 independent requests per thread (1024 threads leave 128 registers each: 16 requests
    // of 12 B with their addresses do not fit)
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
        float2 uu[HB];
        float xv[HB];
#pragma unroll
        for (int k = 0; k < HB; ++k) {
            const int e = tid + (h * HB + k) * NT;
            uu[k] = u[base + e];
            xv[k] = x[base + e];
        }
#pragma unroll
        for (int k = 0; k < HB; ++k) {
            const int e = tid + (h * HB + k) * NT;
            buf[(e >> 7) * LP + (e & 127)] = make_float2(xv[k] + uu[k].x, uu[k].y);   // v = x + u (env.py:87)
        }
    }
    __syncthreads();
    fft128_all_lines<false, LP, 1, NT>(buf, tw);           // rows
    fft128_all_lines<false, 1, LP, NT>(buf, tw);           // columns
    {
        // masked closed-form solve on the sampled bins (env.py:88-90), constants pre-shifted by pnp_reset; the two
        // orthonormal scalings 1/sqrt(128) * 1/sqrt(128) = 2^-7 are exact
        const float m = mu[n], inv1m = 1.f + m, sc = 1.f / 128.f;
        const float2* y0n = y0s + base;
        const uint8_t* mk = masks + (mask_n > 1 ? base : 0);
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            float2 yy[HB];
            uint8_t mm[HB];
#pragma unroll
            for (int k = 0; k < HB; ++k) {
                const int e = tid + (h * HB + k) * NT;
                mm[k] = mk[e];
                yy[k] = y0n[e];
            }
#pragma unroll
            for (int k = 0; k < HB; ++k) {
                const int e = tid + (h * HB + k) * NT;
                float2* p = &buf[(e >> 7) * LP + (e & 127)];
                float2 v = *p;
                v.x *= sc; v.y *= sc;
                if (mm[k]) {
                    v.x = (m * v.x + yy[k].x) / inv1m;
                    v.y = (m * v.y + yy[k].y) / inv1m;
                }
                *p = v;
            }
        }
    }
    __syncthreads();
    fft128_all_lines<true, 1, LP, NT>(buf, tw);            // columns back
    fft128_all_lines<true, LP, 1, NT>(buf, tw);            // rows back
    // x and u once more for the dual update (not carried in registers across eight transform passes); the second read is
    // served by this XCD's L2 - the lines were fetched a few microseconds ago
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
        float2 uu[HB];
        float xv[HB];
#pragma unroll
        for (int k = 0; k < HB; ++k) {
            const int e = tid + (h * HB + k) * NT;
            uu[k] = u[base + e];
            xv[k] = x[base + e];
        }
#pragma unroll
        for (int k = 0; k < HB; ++k) {
            const int e = tid + (h * HB + k) * NT;
            float2 v = buf[(e >> 7) * LP + (e & 127)];
            v.x *= 1.f / 128.f; v.y *= 1.f / 128.f;
            z[base + e] = v;                                                          // z (env.py:91)
            u[base + e] = make_float2(uu[k].x + xv[k] - v.x, uu[k].y - v.y);          // u + x - z (env.py:93)
        }
    }
}

hipError_t launch_admm_slice128(const float* x, float2* z, float2* u, const float2* tw, const float2* y0s,
                                const uint8_t* masks, int mask_n, const float* mu, const float* tact, int N, hipStream_t s) {
    constexpr size_t lds = (size_t)(128 * 129 + 128) * sizeof(float2);
    static DeviceOnce once;
    if (hipError_t e = pnp::raise_lds_cap((const void*)admm_slice128_kernel, (int)lds, once); e != hipSuccess) return e;
    hipLaunchKernelGGL(admm_slice128_kernel, dim3(N), dim3(1024), lds, s, x, z, u, tw, y0s, masks, mask_n, mu, tact);
    return hipGetLastError();
}

// The column pass needs up to ~74 KiB of dynamic LDS (H = 1024); raise the per-kernel cap once.
static hipError_t raise_lds_cap() {
    static DeviceOnce once[5];
    const void* fns[5] = {(const void*)fft_cols_kernel<0, 0>, (const void*)fft_cols_kernel<1, 0>, (const void*)fft_cols_kernel<1, 128>,
                          (const void*)fft_cols_kernel<1, 256>, (const void*)fft_cols_kernel<1, 512>};
    for (int i = 0; i < 5; ++i)
        if (hipError_t e = pnp::raise_lds_cap(fns[i], 80 * 1024, once[i]); e != hipSuccess) return e;
    return hipSuccess;
}

static inline int rows_per_block(int H, int W) {
    int r = ROW_ELEMS / W;
    if (r < 1) r = 1;
    if (r > H) r = H;
    return r;
}
static inline int cols_per_block(int H, int W) {
    int c = H <= 256 ? 16 : (H <= 512 ? 8 : 4);
    if (c > W) c = W;
    return c;
}

// the power-of-two family of the six k-space passes: reached through the dispatch below only
namespace pow2 {

// (the kernels take the shift on load and the shift on store apart; every caller wants the same one for both)
hipError_t launch_fft_rows(const float2* in, float2* out, const float2* tw, int batch, int H, int W, int inverse, int shift, hipStream_t s) {
    const int rpb = rows_per_block(H, W);
    const size_t lds = (size_t)(2 * rpb * W + W) * sizeof(float2);
    hipLaunchKernelGGL((fft_rows_kernel<0, 0>), dim3(batch * (H / rpb)), dim3(256), lds, s, in, out, nullptr, nullptr, tw,
                       nullptr, H, W, rpb, inverse, shift, shift);
    return hipGetLastError();
}
hipError_t launch_fft_cols(float2* data, const float2* tw, int batch, int H, int W, int inverse, int shift, hipStream_t s) {
    const int cw = cols_per_block(H, W);
    const size_t lds = (size_t)(2 * cw * (H + 1) + H) * sizeof(float2);
    if (hipError_t e = raise_lds_cap()) return e;
    hipLaunchKernelGGL((fft_cols_kernel<0, 0>), dim3(batch * (W / cw)), dim3(256), lds, s, data, tw, nullptr, nullptr, 1,
                       nullptr, nullptr, H, W, cw, inverse, shift, shift);
    return hipGetLastError();
}
hipError_t launch_fft_rows_real(const float* x, float2* work, const float2* tw, int N, int H, int W, hipStream_t s) {
    const int rpb = rows_per_block(H, W);
    const size_t lds = (size_t)(2 * rpb * W + W) * sizeof(float2);
    hipLaunchKernelGGL((fft_rows_kernel<3, 0>), dim3(N * (H / rpb)), dim3(256), lds, s, nullptr, work, x, nullptr, tw, nullptr, H, W, rpb, 0, 0, 0);
    return hipGetLastError();
}
// 256- / 512-point rows: the radix-16 / radix-8 variant (16 / 4 rows per workgroup)
static bool rows_r16(int H, int W) { return (W == 256 && H % 16 == 0) || (W == 512 && H % 4 == 0); }

hipError_t launch_fft_rows_fwd_admm(const float* x, const float2* u, float2* work, const float2* tw, const float* tact,
                                    int N, int H, int W, hipStream_t s) {
    if (rows_r16(H, W)) {
        if (W == 512)
            hipLaunchKernelGGL((fft_rows_kernel<1, 512, true>), dim3(N * (H / 4)), dim3(256), (size_t)(4 * SK512_LS + W) * sizeof(float2), s,
                               nullptr, work, x, const_cast<float2*>(u), tw, tact, H, W, 4, 0, 0, 0);
        else
            hipLaunchKernelGGL((fft_rows_kernel<1, 256, true>), dim3(N * (H / 16)), dim3(256), (size_t)(16 * SK256_LS + W) * sizeof(float2), s,
                               nullptr, work, x, const_cast<float2*>(u), tw, tact, H, W, 16, 0, 0, 0);
        return hipGetLastError();
    }
    const int rpb = rows_per_block(H, W);
    const size_t lds = (size_t)(2 * rpb * W + W) * sizeof(float2);
#define PNP_ROWS_FWD(LC_)                                                                                      \
    hipLaunchKernelGGL((fft_rows_kernel<1, LC_>), dim3(N * (H / rpb)), dim3(256), lds, s, nullptr, work, x,      \
                       const_cast<float2*>(u), tw, tact, H, W, rpb, 0, 0, 0)
    const bool ct = rpb == ROW_ELEMS / W;                  // the unrolled variants assume a full ROW_ELEMS batch
    if (ct && W == 128) PNP_ROWS_FWD(128);
    else PNP_ROWS_FWD(0);
#undef PNP_ROWS_FWD
    return hipGetLastError();
}
hipError_t launch_fft_cols_prox(float2* work, const float2* tw, const float2* y0s, const uint8_t* masks, int mask_n,
                                const float* mu, const float* tact, int N, int H, int W, hipStream_t s) {
    const int cw = cols_per_block(H, W);
    size_t lds = (size_t)(2 * cw * (H + 1) + H) * sizeof(float2);
    if (hipError_t e = raise_lds_cap()) return e;
#define PNP_COLS_PROX(LC_)                                                                                    \
    hipLaunchKernelGGL((fft_cols_kernel<1, LC_>), dim3(N * (W / cw)), dim3(256), lds, s, work, tw, y0s, masks, mask_n, mu, \
                       tact, H, W, cw, 0, 0, 0)
    const bool ct = cw == (H <= 256 ? 16 : (H <= 512 ? 8 : 4)) && (H == 128 || H == 256 || H == 512);   // W >= one full strip
    if (ct) lds = (size_t)(cw * (H == 256 ? SK256_LS : (H == 512 ? SK512_LS : H + 1)) + H) * sizeof(float2);      // in place: one strip buffer
    if (ct && H == 128) PNP_COLS_PROX(128);
    else if (ct && H == 256) PNP_COLS_PROX(256);
    else if (ct && H == 512) PNP_COLS_PROX(512);
    else PNP_COLS_PROX(0);
#undef PNP_COLS_PROX
    return hipGetLastError();
}
hipError_t launch_fft_rows_inv_admm(const float2* work, const float* x, float2* z, float2* u, const float2* tw,
                                    const float* tact, int N, int H, int W, hipStream_t s) {
    if (rows_r16(H, W)) {
        if (W == 512)
            hipLaunchKernelGGL((fft_rows_kernel<2, 512, true>), dim3(N * (H / 4)), dim3(256), (size_t)(4 * SK512_LS + W) * sizeof(float2), s,
                               work, z, x, u, tw, tact, H, W, 4, 1, 0, 0);
        else
            hipLaunchKernelGGL((fft_rows_kernel<2, 256, true>), dim3(N * (H / 16)), dim3(256), (size_t)(16 * SK256_LS + W) * sizeof(float2), s,
                               work, z, x, u, tw, tact, H, W, 16, 1, 0, 0);
        return hipGetLastError();
    }
    const int rpb = rows_per_block(H, W);
    const size_t lds = (size_t)(2 * rpb * W + W) * sizeof(float2);
#define PNP_ROWS_INV(LC_)                                                                                      \
    hipLaunchKernelGGL((fft_rows_kernel<2, LC_>), dim3(N * (H / rpb)), dim3(256), lds, s, work, z, x, u, tw, tact, H, W, rpb, \
                       1, 0, 0)
    const bool ct = rpb == ROW_ELEMS / W;
    if (ct && W == 128) PNP_ROWS_INV(128);
    else PNP_ROWS_INV(0);
#undef PNP_ROWS_INV
    return hipGetLastError();
}

}  // namespace pow2

// ---- the six k-space passes: ONE choice of family -----------------------------------------------------------------------------
// A handle with a side that is not a power of two (2^a * 5^b: 80 .. 800) runs the mixed-radix kernels (fft_mixed_kernels.hip) for
// every pass, its power-of-two side included; every other handle runs the kernels of this file.  The rule lives here and nowhere else.
static bool mixed_radix(int H, int W) {
    auto is_pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0; };
    return !is_pow2(H) || !is_pow2(W);
}

hipError_t launch_fft_rows(const float2* in, float2* out, const float2* tw, int batch, int H, int W, int inverse, int shift, hipStream_t s) {
    return mixed_radix(H, W) ? mixed::launch_fft_rows(in, out, tw, batch, H, W, inverse, shift, s)
                             : pow2::launch_fft_rows(in, out, tw, batch, H, W, inverse, shift, s);
}
hipError_t launch_fft_cols(float2* data, const float2* tw, int batch, int H, int W, int inverse, int shift, hipStream_t s) {
    return mixed_radix(H, W) ? mixed::launch_fft_cols(data, tw, batch, H, W, inverse, shift, s)
                             : pow2::launch_fft_cols(data, tw, batch, H, W, inverse, shift, s);
}
hipError_t launch_fft_rows_real(const float* x, float2* work, const float2* tw, int N, int H, int W, hipStream_t s) {
    return mixed_radix(H, W) ? mixed::launch_fft_rows_real(x, work, tw, N, H, W, s)
                             : pow2::launch_fft_rows_real(x, work, tw, N, H, W, s);
}
hipError_t launch_fft_rows_fwd_admm(const float* x, const float2* u, float2* work, const float2* tw, const float* tact, int N, int H, int W,
                                    hipStream_t s) {
    return mixed_radix(H, W) ? mixed::launch_fft_rows_fwd_admm(x, u, work, tw, tact, N, H, W, s)
                             : pow2::launch_fft_rows_fwd_admm(x, u, work, tw, tact, N, H, W, s);
}
hipError_t launch_fft_cols_prox(float2* work, const float2* tw, const float2* y0s, const uint8_t* masks, int mask_n, const float* mu,
                                const float* tact, int N, int H, int W, hipStream_t s) {
    return mixed_radix(H, W) ? mixed::launch_fft_cols_prox(work, tw, y0s, masks, mask_n, mu, tact, N, H, W, s)
                             : pow2::launch_fft_cols_prox(work, tw, y0s, masks, mask_n, mu, tact, N, H, W, s);
}
hipError_t launch_fft_rows_inv_admm(const float2* work, const float* x, float2* z, float2* u, const float2* tw, const float* tact, int N,
                                    int H, int W, hipStream_t s) {
    return mixed_radix(H, W) ? mixed::launch_fft_rows_inv_admm(work, x, z, u, tw, tact, N, H, W, s)
                             : pow2::launch_fft_rows_inv_admm(work, x, z, u, tw, tact, N, H, W, s);
}

// ---- Toeplitz normal operator: the fused application (include/pnpadmm_toeplitz.h) ------------------------------------------------
// q = crop(ifft2c(K . fft2c(pad(p)))) on the 2H x 2W grid in three launches, none of which touches the grid's zero half:
//   rows forward : p [planes, H, W] -> zero-filled to 2W in LDS -> row transforms of the H live rows -> buf [planes, H, 2W] (centred columns)
//   columns      : a strip's H live rows into lines of 2H, zeros elsewhere -> forward -> . K / (4 H W) -> inverse -> the H cropped rows, in
//                  place in buf: fft_cols_body<1, LC>'s shape with K in place of the masked solve
//   rows inverse : row transforms back, cropped to W, (+ mu p by one fma, the partial sums of Re<p, q>) -> q
// The four orthonormal scalings are one power of two, 1 / (4 H W): it rides on K, an exact scaling of the spectrum, and the transforms
// store unscaled.  Lines of 256 and 512 points run the register-resident radix-16 / radix-8 passes, every other length fft_lines.
// A workgroup of the row passes owns the rows of ONE pixel chunk of a slice (block_reduce.h: kPixelChunk pixels, min(H, 2048 / W) rows,
// at most 4096 grid elements), so the inverse pass leaves the partial sums in nufft_crop_kernel's ranges, by its tree.
// New kernels beside the six passes above, which they leave as they were; power-of-two sides only (mixed_radix below).
static_assert(kPixelChunk == ROW_ELEMS, "a row workgroup of the Toeplitz passes owns one pixel chunk");

template <int LC>
__device__ __forceinline__ int tz_slot(int r, int c, int L) {
    return LC == 256 ? r * SK256_LS + sk256(c) : (LC == 512 ? r * SK512_LS + sk512(c) : r * L + c);
}
// the workgroup's row transforms (loads synchronised by the caller); returns the buffer holding the synchronised result
template <bool INV, int LC>
__device__ __forceinline__ float2* tz_row_lines(float2* buf0, float2* buf1, const float2* tw, int L, int rows) {
    if constexpr (LC == 256) { fft256_radix16_inplace<INV, 16>(buf0, tw); return buf0; }
    else if constexpr (LC == 512) { fft512_radix8_inplace<INV, 8, 32>(buf0, tw); return buf0; }
    else return fft_lines<INV>(buf0, buf1, tw, L, rows, L);
}
static inline int tz_rows_per_block(int H, int W) { return H < kPixelChunk / W ? H : kPixelChunk / W; }
static inline size_t tz_rows_lds(int L, int rows) {
    return (size_t)(L == 256 ? 16 * SK256_LS + L : (L == 512 ? 8 * SK512_LS + L : 2 * rows * L + L)) * sizeof(float2);
}

// LC: 256 / 512 = the line length 2W, on the register-resident passes (16 / 8 rows per workgroup); 0: any other length
template <int LC>
__global__ __launch_bounds__(256) void tz_rows_fwd_kernel(const float2* __restrict__ p, float2* __restrict__ out, const float2* __restrict__ twg,
                                                          int H, int W, int rows) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int L = 2 * W, lw = 31 - __builtin_clz(L), tot = rows * L;
    const int blocks_per_img = H / rows;
    const int n = blockIdx.x / blocks_per_img, y0 = (blockIdx.x % blocks_per_img) * rows;
    float2* buf0 = smem;
    float2* buf1 = smem + (LC ? 0 : tot);
    float2* tw = smem + (LC == 256 ? 16 * SK256_LS : (LC == 512 ? 8 * SK512_LS : 2 * tot));
    for (int i = threadIdx.x; i < L; i += 256) tw[i] = twg[i];
    const float2* src = p + ((size_t)n * H + y0) * W;
    for (int e = threadIdx.x; e < tot; e += 256) {
        const int r = e >> lw, c = e & (L - 1);
        const int ix = (c ^ W) - W / 2;                    // position c of the unshifted line holds the centred padded column c ^ W
        float2 v = make_float2(0.f, 0.f);
        if (ix >= 0 && ix < W) v = src[(size_t)r * W + ix];
        buf0[tz_slot<LC>(r, c, L)] = v;
    }
    __syncthreads();
    const float2* res = tz_row_lines<false, LC>(buf0, buf1, tw, L, rows);
    float2* dst = out + ((size_t)n * H + y0) * L;
    for (int e = threadIdx.x; e < tot; e += 256) {
        const int r = e >> lw, c = e & (L - 1);
        dst[(size_t)r * L + (c ^ W)] = res[tz_slot<LC>(r, c, L)];
    }
}

template <int LC>
__global__ __launch_bounds__(256) void tz_rows_inv_kernel(const float2* __restrict__ in, const float2* __restrict__ twg,
                                                          const float2* __restrict__ pv, const float* __restrict__ mu,
                                                          const float* __restrict__ tact, float2* __restrict__ q, double* __restrict__ partial,
                                                          int H, int W, int rows) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    __shared__ double red[256 / 64];
    const int L = 2 * W, lw = 31 - __builtin_clz(L), tot = rows * L;
    const int chunks = H / rows;                           // = pixel_chunks(H, W)
    const int n = blockIdx.x / chunks, chunk = blockIdx.x % chunks, y0 = chunk * rows;
    if (tact != nullptr && tact[n] > 0.5f) return;
    float2* buf0 = smem;
    float2* buf1 = smem + (LC ? 0 : tot);
    float2* tw = smem + (LC == 256 ? 16 * SK256_LS : (LC == 512 ? 8 * SK512_LS : 2 * tot));
    for (int i = threadIdx.x; i < L; i += 256) tw[i] = twg[i];
    const float2* src = in + ((size_t)n * H + y0) * L;
    for (int e = threadIdx.x; e < tot; e += 256) {
        const int r = e >> lw, c = e & (L - 1);
        buf0[tz_slot<LC>(r, c, L)] = src[(size_t)r * L + (c ^ W)];
    }
    __syncthreads();
    const float2* res = tz_row_lines<true, LC>(buf0, buf1, tw, L, rows);
    const int px = rows * W, lpw = 31 - __builtin_clz(W);
    const size_t base = ((size_t)n * H + y0) * W;
    const float m = (pv != nullptr && mu != nullptr) ? mu[n] : 0.f;
    double dot[1] = {0.0};
#pragma unroll
    for (int j = 0; j < kPixelChunk / 256; ++j) {
        const int pl = threadIdx.x + j * 256;              // nufft_crop_kernel's pixel order within the chunk
        if (pl < px) {
            const int r = pl >> lpw, ix = pl & (W - 1);
            float2 o = res[tz_slot<LC>(r, (ix + W / 2) ^ W, L)];
            if (pv != nullptr) {
                const float2 pp = pv[base + pl];
                o.x = __fmaf_rn(m, pp.x, o.x); o.y = __fmaf_rn(m, pp.y, o.y);
                dot[0] += (double)pp.x * (double)o.x + (double)pp.y * (double)o.y;
            }
            q[base + pl] = o;
        }
    }
    if (partial == nullptr) return;                        // (uniform)
    block_sums_fixed<256, 1>(dot, red);
    if (threadIdx.x == 0) partial[((size_t)n * chunks + chunk) * 2] = dot[0];
}

// LC: 256 / 512 = the line length 2H on the register-resident passes (strips of 16 / 8 columns, in place in one skewed buffer); 0: any other
template <int LC>
__global__ __launch_bounds__(256) void tz_cols_kernel(float2* __restrict__ data, const float* __restrict__ K, const float2* __restrict__ twg, int H,
                                                      int W, int cw) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    constexpr bool R16 = LC == 256, R8 = LC == 512;
    const int L = 2 * H, GW = 2 * W, strips = GW / cw;
    int vb = blockIdx.x;                                   // fft_cols_kernel's (slice, strip) -> XCD map
    if ((gridDim.x & 7) == 0) vb = (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
    const int n = vb / strips, x0 = (vb % strips) * cw;
    const int lstr = R16 ? SK256_LS : (R8 ? SK512_LS : L + 1);
    auto rpos = [](int r) { return R16 ? sk256(r) : (R8 ? sk512(r) : r); };
    float2* buf0 = smem;
    float2* buf1 = smem + cw * lstr;
    float2* tw = smem + (LC > 0 ? 1 : 2) * cw * lstr;
    float2* img = data + (size_t)n * H * GW;
    const int lcw = 31 - __builtin_clz(cw), tot = cw * L;
    const float inv = 1.f / (4.f * (float)H * (float)W);   // a power of two
    for (int i = threadIdx.x; i < L; i += 256) tw[i] = twg[i];
    for (int e = threadIdx.x; e < tot; e += 256) {
        const int r = e >> lcw, c = e & (cw - 1);
        const int iy = (r ^ H) - H / 2;                    // position r of the unshifted line holds the centred padded row r ^ H
        float2 v = make_float2(0.f, 0.f);
        if (iy >= 0 && iy < H) v = img[(size_t)iy * GW + x0 + c];
        buf0[c * lstr + rpos(r)] = v;
    }
    const float2* res;
    if constexpr (LC > 0) {
        // 2H == LC, cw == CWC (checked by the launcher): the strip's K values are fetched BEFORE the forward transform and sit in registers under it
        constexpr int CWC = LC <= 256 ? 16 : 8, LS = R16 ? SK256_LS : SK512_LS, PER = CWC * LC / 256;
        float kk[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int e = threadIdx.x + k * 256;
            kk[k] = K[(size_t)((e / CWC) ^ H) * GW + x0 + (e % CWC)];
        }
        __syncthreads();
        if constexpr (R16) fft256_radix16_inplace<false, CWC>(buf0, tw);
        else fft512_radix8_inplace<false, CWC, 32>(buf0, tw);
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int e = threadIdx.x + k * 256;
            float2* p = &buf0[(e % CWC) * LS + rpos(e / CWC)];
            const float f = kk[k] * inv;
            float2 v = *p;
            v.x *= f; v.y *= f;
            *p = v;
        }
        __syncthreads();
        if constexpr (R16) fft256_radix16_inplace<true, CWC>(buf0, tw);
        else fft512_radix8_inplace<true, CWC, 32>(buf0, tw);
        res = buf0;
    } else {
        __syncthreads();
        float2* fw = fft_lines<false>(buf0, buf1, tw, L, cw, lstr);
        float2* oth = (fw == buf0) ? buf1 : buf0;
        for (int e = threadIdx.x; e < tot; e += 256) {
            const int r = e >> lcw, c = e & (cw - 1);
            const float f = K[(size_t)(r ^ H) * GW + x0 + c] * inv;
            float2 v = fw[c * lstr + r];
            v.x *= f; v.y *= f;
            fw[c * lstr + r] = v;
        }
        __syncthreads();
        res = fft_lines<true>(fw, oth, tw, L, cw, lstr);
    }
    for (int e = threadIdx.x; e < cw * H; e += 256) {
        const int iy = e >> lcw, c = e & (cw - 1);
        img[(size_t)iy * GW + x0 + c] = res[c * lstr + rpos((iy + H / 2) ^ H)];
    }
}

static hipError_t tz_raise_lds_cap() {
    static DeviceOnce once[3];
    const void* fns[3] = {(const void*)tz_rows_fwd_kernel<0>, (const void*)tz_rows_inv_kernel<0>, (const void*)tz_cols_kernel<0>};
    for (int i = 0; i < 3; ++i)
        if (hipError_t e = pnp::raise_lds_cap(fns[i], 80 * 1024, once[i]); e != hipSuccess) return e;
    return hipSuccess;
}

bool toeplitz_fused_ok(int H, int W) { return !mixed_radix(2 * H, 2 * W); }

hipError_t launch_toeplitz_rows_fwd(const float2* p, float2* buf, const float2* tw, int planes, int H, int W, hipStream_t s) {
    if (!toeplitz_fused_ok(H, W)) return hipErrorInvalidValue;
    if (hipError_t e = tz_raise_lds_cap()) return e;
    const int rows = tz_rows_per_block(H, W), L = 2 * W;
    const dim3 g((unsigned)(planes * (H / rows)));
    if (L == 256) hipLaunchKernelGGL((tz_rows_fwd_kernel<256>), g, dim3(256), tz_rows_lds(L, rows), s, p, buf, tw, H, W, rows);
    else if (L == 512) hipLaunchKernelGGL((tz_rows_fwd_kernel<512>), g, dim3(256), tz_rows_lds(L, rows), s, p, buf, tw, H, W, rows);
    else hipLaunchKernelGGL((tz_rows_fwd_kernel<0>), g, dim3(256), tz_rows_lds(L, rows), s, p, buf, tw, H, W, rows);
    return hipGetLastError();
}
hipError_t launch_toeplitz_cols(float2* buf, const float* K, const float2* tw, int planes, int H, int W, hipStream_t s) {
    if (!toeplitz_fused_ok(H, W)) return hipErrorInvalidValue;
    if (hipError_t e = tz_raise_lds_cap()) return e;
    const int L = 2 * H, cw = cols_per_block(L, 2 * W);
    const dim3 g((unsigned)(planes * (2 * W / cw)));
    if (L == 256) hipLaunchKernelGGL((tz_cols_kernel<256>), g, dim3(256), (size_t)(cw * SK256_LS + L) * sizeof(float2), s, buf, K, tw, H, W, cw);
    else if (L == 512) hipLaunchKernelGGL((tz_cols_kernel<512>), g, dim3(256), (size_t)(cw * SK512_LS + L) * sizeof(float2), s, buf, K, tw, H, W, cw);
    else hipLaunchKernelGGL((tz_cols_kernel<0>), g, dim3(256), (size_t)(2 * cw * (L + 1) + L) * sizeof(float2), s, buf, K, tw, H, W, cw);
    return hipGetLastError();
}
hipError_t launch_toeplitz_rows_inv(const float2* buf, const float2* tw, const float2* pv, const float* mu, const float* tact, float2* q,
                                    double* partial, int planes, int H, int W, hipStream_t s) {
    if (!toeplitz_fused_ok(H, W)) return hipErrorInvalidValue;
    if (hipError_t e = tz_raise_lds_cap()) return e;
    const int rows = tz_rows_per_block(H, W), L = 2 * W;
    const dim3 g((unsigned)(planes * (H / rows)));
    if (L == 256) hipLaunchKernelGGL((tz_rows_inv_kernel<256>), g, dim3(256), tz_rows_lds(L, rows), s, buf, tw, pv, mu, tact, q, partial, H, W, rows);
    else if (L == 512) hipLaunchKernelGGL((tz_rows_inv_kernel<512>), g, dim3(256), tz_rows_lds(L, rows), s, buf, tw, pv, mu, tact, q, partial, H, W, rows);
    else hipLaunchKernelGGL((tz_rows_inv_kernel<0>), g, dim3(256), tz_rows_lds(L, rows), s, buf, tw, pv, mu, tact, q, partial, H, W, rows);
    return hipGetLastError();
}

// ---- Toeplitz form of the off-resonance operator: the two column passes of its fused application (include/pnpadmm_offres_tz.h) ----------
// tz_cols_kernel cut in two, because the spectral mix between the transforms reads all L planes of a slice at one bin:
//   columns forward : a strip's H live rows of half [planes, H, 2W] into lines of 2H, zeros elsewhere -> forward -> the whole column spectrum
//                     into full [planes, 2H, 2W], centred rows
//   columns inverse : a strip's lines of full -> inverse -> the H cropped rows into half
// Both store unscaled, as the row passes do: the mix carries 1 / (4 H W).  The same line transforms as tz_cols_kernel, by the same rule.
// INV = false: in = half, out = full; INV = true: in = full, out = half
template <int LC, bool INV>
__global__ __launch_bounds__(256) void tz_cols_half_kernel(const float2* __restrict__ in, float2* __restrict__ out, const float2* __restrict__ twg,
                                                           int H, int W, int cw) {
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    constexpr bool R16 = LC == 256, R8 = LC == 512;
    const int L = 2 * H, GW = 2 * W, strips = GW / cw;
    int vb = blockIdx.x;                                   // fft_cols_kernel's (slice, strip) -> XCD map
    if ((gridDim.x & 7) == 0) vb = (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
    const int n = vb / strips, x0 = (vb % strips) * cw;
    const int lstr = R16 ? SK256_LS : (R8 ? SK512_LS : L + 1);
    auto rpos = [](int r) { return R16 ? sk256(r) : (R8 ? sk512(r) : r); };
    float2* buf0 = smem;
    float2* buf1 = smem + cw * lstr;
    float2* tw = smem + (LC > 0 ? 1 : 2) * cw * lstr;
    const float2* half_in = in + (size_t)n * H * GW;
    const float2* full_in = in + (size_t)n * L * GW;
    float2* half_out = out + (size_t)n * H * GW;
    float2* full_out = out + (size_t)n * L * GW;
    const int lcw = 31 - __builtin_clz(cw), tot = cw * L;
    for (int i = threadIdx.x; i < L; i += 256) tw[i] = twg[i];
    for (int e = threadIdx.x; e < tot; e += 256) {
        const int r = e >> lcw, c = e & (cw - 1);          // position r of the unshifted line holds the centred padded row r ^ H
        float2 v = make_float2(0.f, 0.f);
        if (INV) {
            v = full_in[(size_t)(r ^ H) * GW + x0 + c];
        } else {
            const int iy = (r ^ H) - H / 2;
            if (iy >= 0 && iy < H) v = half_in[(size_t)iy * GW + x0 + c];
        }
        buf0[c * lstr + rpos(r)] = v;
    }
    __syncthreads();
    const float2* res;
    if constexpr (R16) { fft256_radix16_inplace<INV, 16>(buf0, tw); res = buf0; }
    else if constexpr (R8) { fft512_radix8_inplace<INV, 8, 32>(buf0, tw); res = buf0; }
    else res = fft_lines<INV>(buf0, buf1, tw, L, cw, lstr);
    if (INV) {
        for (int e = threadIdx.x; e < cw * H; e += 256) {
            const int iy = e >> lcw, c = e & (cw - 1);
            half_out[(size_t)iy * GW + x0 + c] = res[c * lstr + rpos((iy + H / 2) ^ H)];
        }
    } else {
        for (int e = threadIdx.x; e < tot; e += 256) {
            const int r = e >> lcw, c = e & (cw - 1);
            full_out[(size_t)(r ^ H) * GW + x0 + c] = res[c * lstr + rpos(r)];
        }
    }
}

template <bool INV>
static hipError_t launch_tz_cols_half(const float2* in, float2* out, const float2* tw, int planes, int H, int W, hipStream_t s) {
    if (!toeplitz_fused_ok(H, W)) return hipErrorInvalidValue;
    static DeviceOnce once;
    if (hipError_t e = pnp::raise_lds_cap((const void*)tz_cols_half_kernel<0, INV>, 80 * 1024, once); e != hipSuccess) return e;
    const int L = 2 * H, cw = cols_per_block(L, 2 * W);
    const dim3 g((unsigned)(planes * (2 * W / cw)));
    if (L == 256) hipLaunchKernelGGL((tz_cols_half_kernel<256, INV>), g, dim3(256), (size_t)(cw * SK256_LS + L) * sizeof(float2), s, in, out, tw, H, W, cw);
    else if (L == 512) hipLaunchKernelGGL((tz_cols_half_kernel<512, INV>), g, dim3(256), (size_t)(cw * SK512_LS + L) * sizeof(float2), s, in, out, tw, H, W, cw);
    else hipLaunchKernelGGL((tz_cols_half_kernel<0, INV>), g, dim3(256), (size_t)(2 * cw * (L + 1) + L) * sizeof(float2), s, in, out, tw, H, W, cw);
    return hipGetLastError();
}
hipError_t launch_offres_tz_cols_fwd(const float2* half, float2* full, const float2* tw, int planes, int H, int W, hipStream_t s) {
    return launch_tz_cols_half<false>(half, full, tw, planes, H, W, s);
}
hipError_t launch_offres_tz_cols_inv(const float2* full, float2* half, const float2* tw, int planes, int H, int W, hipStream_t s) {
    return launch_tz_cols_half<true>(full, half, tw, planes, H, W, s);
}

// ---- reset: x = Re(x0), z = x0, u = 0; fold the fftshifts into the episode constants -------------
__global__ void reset_kernel(const float2* __restrict__ x0, const float2* __restrict__ y0,
                             const uint8_t* __restrict__ mask, int mask_n, float* __restrict__ x,
                             float2* __restrict__ z, float2* __restrict__ u, float2* __restrict__ y0s,
                             uint8_t* __restrict__ masks, int N, int H, int W) {
    const size_t hw = (size_t)H * W, total = (size_t)N * hw;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t n = i / hw, p = i - n * hw;
        const int k1 = (int)(p / W), k2 = (int)(p - (size_t)k1 * W);
        if (x0 != nullptr) {                                   // null: only the episode constants are rebuilt (pnp_set_kspace)
            const float2 v = x0[i];
            x[i] = v.x;
            z[i] = v;
            u[i] = make_float2(0.f, 0.f);
        }
        // S: index + N/2 mod N (add-mod: the XOR form is only right for powers of two; the same indices there).  The sign stays
        // (-1)^(k1 + k2) for every accepted size: N/2 is even, so rolling by N/2 multiplies bin k by (-1)^k
        const int s1 = k1 < (H >> 1) ? k1 + (H >> 1) : k1 - (H >> 1), s2 = k2 < (W >> 1) ? k2 + (W >> 1) : k2 - (W >> 1);
        const size_t ps = (size_t)s1 * W + s2;
        const float sg = ((k1 + k2) & 1) ? -1.f : 1.f;
        const float2 yy = y0[n * hw + ps];
        y0s[i] = make_float2(sg * yy.x, sg * yy.y);
        if (mask_n > 1 || n == 0) masks[(mask_n > 1 ? n * hw : 0) + p] = mask[(mask_n > 1 ? n * hw : 0) + ps] ? 1 : 0;
    }
}

hipError_t launch_reset(const float2* x0, const float2* y0, const uint8_t* mask, int mask_n, float* x, float2* z,
                        float2* u, float2* y0s, uint8_t* masks, int N, int H, int W, hipStream_t s) {
    const size_t total = (size_t)N * H * W;
    unsigned blocks = (unsigned)((total + 255) / 256);
    if (blocks > 8192u) blocks = 8192u;
    hipLaunchKernelGGL(reset_kernel, dim3(blocks), dim3(256), 0, s, x0, y0, mask, mask_n, x, z, u, y0s, masks, N, H, W);
    return hipGetLastError();
}

__global__ void finish_kernel(const float* __restrict__ tact, float* __restrict__ tstate, uint8_t* __restrict__ done,
                              int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const bool d = tact != nullptr && tact[n] > 0.5f;
    if (done != nullptr) done[n] = d ? 1 : 0;
    if (tstate != nullptr && !d) tstate[n] += 1.0f / 30.0f;     // env.py:98
}
hipError_t launch_finish(const float* tact, float* tstate, uint8_t* done, int N, hipStream_t s) {
    hipLaunchKernelGGL(finish_kernel, dim3((N + 63) / 64), dim3(64), 0, s, tact, tstate, done, N);
    return hipGetLastError();
}

// ---- PSNR (env.py:120-125): one workgroup per slice, f64 accumulation of the squared error --------
constexpr int kPsnrThreads = 1024;
__global__ __launch_bounds__(kPsnrThreads) void psnr_kernel(const float* __restrict__ x, const float* __restrict__ gt,
                                                    float* __restrict__ out, int HW) {
    __shared__ double part[kPsnrThreads / 64];
    const int n = blockIdx.x;
    const float* xp = x + (size_t)n * HW;
    const float* gp = gt + (size_t)n * HW;
    double acc = 0.0;
    for (int i = threadIdx.x; i < HW; i += blockDim.x) {
        const float d = fminf(fmaxf(xp[i], 0.f), 1.f) - gp[i];
        acc += (double)d * (double)d;
    }
    const double t = block_sum_fixed<0>(acc, part);        // (0: this kernel takes its width from the launch)
    if (threadIdx.x == 0) {
        const double mse = t / (double)HW;
        out[n] = (float)(10.0 * log10(1.0 / mse));
    }
}
hipError_t launch_psnr(const float* x, const float* gt, float* out, int N, int HW, hipStream_t s) {
    hipLaunchKernelGGL(psnr_kernel, dim3(N), dim3(kPsnrThreads), 0, s, x, gt, out, HW);
    return hipGetLastError();
}

}  // namespace pnp
