// Haar wavelet shrinkage (pnp_haar_denoise, and the x-update of pnp_step under PNP_PRIOR_HAAR): the decimated orthonormal transform
// (PNP_HAAR_ORTHO) and its translation-invariant, fully cycle-spun form (PNP_HAAR_TI) computed as the undecimated transform.
//
// THE FLOAT32 EXPRESSION ORDER (tests/haar_ref.py restates it; every kernel of this unit evaluates exactly this, through the one set of
// device functions below, so the bits depend neither on the tile plan nor on which kernel ran).  Every operation is one IEEE float32
// operation; the unit is compiled with floating-point contraction OFF (the pragma below) and holds no fma; every scale factor is an exact
// power of two.  Per slice, J = levels, boundaries periodic:
//     lam = scale * lam_in[n]                      (a product; scale = 1 for pnp_haar_denoise, float32(haar_scale) for pnp_step)
//     not (lam > 0):  out = min(max(v, 0), 1)      (lam = 0, and a negative or NaN threshold too)
//     one step on four samples p00 p01 / p10 p11 of the approximation a_(j-1)  (a_0 = v):
//         a  = ((p00 + p01) + (p10 + p11)) * 0.5      dh = ((p00 - p01) + (p10 - p11)) * 0.5
//         dv = ((p00 + p01) - (p10 + p11)) * 0.5      dd = ((p00 - p01) - (p10 - p11)) * 0.5
//     clip:   ch = min(max(dh, -lam), lam), cv and cd likewise                       (d - soft(d, lam) = clip(d, -lam, lam))
//     the transposed step on the residual approximation s = r_j of the block (r_J = 0) and its clipped details, unscaled:
//         q00 = (s + ch) + (cv + cd)      q01 = (s - ch) + (cv - cd)      q10 = (s + ch) - (cv + cd)      q11 = (s - ch) - (cv - cd)
//     ORTHO: the four samples are the aligned 2 x 2 group (2i, 2k) .. (2i+1, 2k+1) of a_(j-1), and r_(j-1)(2i+a, 2k+b) = q_ab * 0.5
//     TI   : with h = 2^(j-1) the block at (i, k) has the samples (i, k), (i, k+h), (i+h, k), (i+h, k+h) of a_(j-1), and
//            r_(j-1)(i, k) = ((q00 of block (i, k) + q01 of block (i, k-h)) + (q10 of block (i-h, k) + q11 of block (i-h, k-h))) * 0.125
//     out = min(max(v - r_0, 0), 1)
// The details of a constant image are exactly 0, so r = 0 and it comes back bit for bit (clamped); lam = 0 is the clamp alone.  No atomics,
// no reductions.  v = the float32 plane of pnp_haar_denoise, or Re z - Re u (one float32 subtraction) read from the complex planes of pnp_step.
//
// THE FUSED TI KERNEL (haar_ti_fused_kernel<J, ZU>): ONE launch for the whole operator.  A workgroup of 32 x 32 threads owns a 128 x 128
// REGION of a slice, loaded with periodic wrap (modulo indices); thread (tx, ty) keeps the 4 x 4 pixels (ty + 32 r, tx + 32 c) of the planes
// a_0 .. a_(J-1) in registers (a_J is never needed: the residual form starts from r_J = 0).  out(i, k) depends on v within 2^J - 1 pixels on
// every side, so the stored TILE is the region minus 2^J - 1 pixels all round: 126, 122, 114, 98 pixels a side for J = 1 .. 4.  Samples at
// distance h cross threads through two LDS planes: a_(j-1) (down and up) and r_j (up); with the strided ownership the 32 lanes of an LDS
// lane group read 32 consecutive dwords, conflict-free, and every read is the thread's one base address plus a compile-time offset.  On the
// way up a pixel recomputes the details of the four blocks that reach it from the 3 x 3 samples of a_(j-1) at spacing h, rather than holding
// 3 J detail planes.  The planes carry a margin of 8 zeros where a read can leave the region (a_(j-1): all round, 144 x 144; r_j: top and
// left, 136 x 136; 153.25 KiB together): what is computed from the margin lies in the band that is never stored.  Two barriers per level:
// J - 1 levels down, J up.
// THE NAIVE FORM (PNP_HAAR_NAIVE=1): one launch per level down and per level up, one thread per pixel, the planes a_1 .. a_(J-1) and r_j in
// device memory; it is the bit-for-bit check of the fused kernel and its timing baseline.
// ORTHO (haar_ortho_kernel): 2^J x 2^J blocks are independent and every side is a multiple of 16, so a workgroup of 256 threads owns a
// 16 x 16 tile and runs the pyramid in LDS: no halo.
#include "pnp_internal.h"

#pragma clang fp contract(off)

namespace pnp {

namespace {

__device__ __forceinline__ float haar_approx(float p00, float p01, float p10, float p11) { return ((p00 + p01) + (p10 + p11)) * 0.5f; }

__device__ __forceinline__ float haar_clip(float d, float lam) { return fminf(fmaxf(d, -lam), lam); }

// One block: the details of its four samples, clipped, and the unscaled transposed step on (s, ch, cv, cd).  Callers use the q they need.
__device__ __forceinline__ void haar_block(float p00, float p01, float p10, float p11, float s, float lam, float& q00, float& q01,
                                           float& q10, float& q11) {
    const float ch = haar_clip(((p00 - p01) + (p10 - p11)) * 0.5f, lam);
    const float cv = haar_clip(((p00 + p01) - (p10 + p11)) * 0.5f, lam);
    const float cd = haar_clip(((p00 - p01) - (p10 - p11)) * 0.5f, lam);
    q00 = (s + ch) + (cv + cd);
    q01 = (s - ch) + (cv - cd);
    q10 = (s + ch) - (cv + cd);
    q11 = (s - ch) - (cv - cd);
}

// The TI synthesis at one pixel from the 3 x 3 samples w of a_(j-1) at spacing h around it and r_j at the four block origins
// (s00: the pixel's own, s01: h to the left, s10: h up, s11: both).
__device__ __forceinline__ float haar_ti_up(const float (&w)[3][3], float s00, float s01, float s10, float s11, float lam) {
    float q00, q01, q10, q11, t0, t1, t2;
    haar_block(w[1][1], w[1][2], w[2][1], w[2][2], s00, lam, q00, t0, t1, t2);
    haar_block(w[1][0], w[1][1], w[2][0], w[2][1], s01, lam, t0, q01, t1, t2);
    haar_block(w[0][1], w[0][2], w[1][1], w[1][2], s10, lam, t0, t1, q10, t2);
    haar_block(w[0][0], w[0][1], w[1][0], w[1][1], s11, lam, t0, t1, t2, q11);
    return ((q00 + q01) + (q10 + q11)) * 0.125f;
}

__device__ __forceinline__ float haar_out(float v, float r) { return fminf(fmaxf(v - r, 0.0f), 1.0f); }

__device__ __forceinline__ float haar_clamp(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// v at offset `off` of the slice that starts at `base`
template <bool ZU>
__device__ __forceinline__ float haar_load(const HaarArgs& a, size_t base, unsigned off) {
    if (ZU) return (a.z + base)[off].x - (a.u + base)[off].x;
    return (a.v + base)[off];
}

// i modulo n for i in [-n, 2n): one wrap (every halo is shorter than the shortest side)
__device__ __forceinline__ int wrap1(int i, int n) { return i < 0 ? i + n : (i >= n ? i - n : i); }

// ---- the fused TI kernel -------------------------------------------------------------------------------------------------------------
constexpr int kR = kHaarRegion;                  // region side
constexpr int kB = 32;                           // threads per side of the workgroup
constexpr int kP = kR / kB;                      // pixels per thread and side, strided by kB
constexpr int kM = 1 << (kHaarMaxLevels - 1);   // the longest reach of a read: h of the last level
constexpr int kSA = kR + 2 * kM, kSR = kR + kM;  // row strides of the two LDS planes
static_assert(kB * kP == kR && (kSA * kSA + kSR * kSR) * sizeof(float) <= 160 * 1024, "region plan");

template <int J, bool ZU>
__global__ __launch_bounds__(kB * kB) void haar_ti_fused_kernel(HaarArgs a) {
    __shared__ float s_a[kSA * kSA];   // a_(j-1) of the region, a margin of kM all round
    __shared__ float s_r[kSR * kSR];   // r_j of the region, a margin of kM above and to the left
    constexpr int halo = (1 << J) - 1, tile = kR - 2 * halo;
    const int tiles = a.tiles_x * a.tiles_y;
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    if (a.tact && a.tact[n] > 0.5f) return;                       // a stopped slice keeps x
    const int tby = t / a.tiles_x, tbx = t - tby * a.tiles_x;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int H = a.H, W = a.W;
    const float lam = a.scale * a.lam[n];
    const size_t base = (size_t)n * H * W;

    float pl[J][kP][kP];                                          // a_0 .. a_(J-1)
    {
        // the wrapped image row / column of the thread's pixels, as 32-bit offsets into the slice (whose base is uniform: a scalar)
        unsigned gi[kP], gj[kP];
#pragma unroll
        for (int r = 0; r < kP; ++r) {
            const int i = tby * tile - halo + ty + kB * r, j = tbx * tile - halo + tx + kB * r;
            gi[r] = (unsigned)(((i % H) + H) % H) * (unsigned)W;  // (a region may be many images wide: a true modulo)
            gj[r] = (unsigned)(((j % W) + W) % W);
        }
#pragma unroll
        for (int r = 0; r < kP; ++r)
#pragma unroll
            for (int c = 0; c < kP; ++c) pl[0][r][c] = haar_load<ZU>(a, base, gi[r] + gj[c]);
    }
    // Stores value(r, c) to the pixels of the tile.  They lie inside the image, so their offsets need no modulo; these are formed from
    // an opaque copy of the thread index so that no register carries them through the levels.
    const auto store_tile = [&](auto value) {
        int sx = tx, sy = ty;
        asm volatile("" : "+v"(sx), "+v"(sy));
#pragma unroll
        for (int r = 0; r < kP; ++r) {
            const int lr = sy + kB * r, i = tby * tile - halo + lr;
            if (lr < halo || lr >= halo + tile || i >= H) continue;
#pragma unroll
            for (int c = 0; c < kP; ++c) {
                const int lc = sx + kB * c, j = tbx * tile - halo + lc;
                if (lc >= halo && lc < halo + tile && j < W) (a.out + base)[(unsigned)(i * W + j)] = value(r, c);
            }
        }
    };
    if (!(lam > 0.0f)) {                                          // the clamp alone (uniform over the workgroup)
        store_tile([&](int r, int c) { return haar_clamp(pl[0][r][c]); });
        return;
    }
    // the margins: zero, never written again (the first barrier below orders them before any read)
    for (int q = ty * kB + tx; q < kSA * kSA; q += kB * kB) {
        const int row = q / kSA, col = q - row * kSA;
        if (row < kM || row >= kM + kR || col < kM || col >= kM + kR) s_a[q] = 0.0f;
    }
    if (J > 1)
        for (int q = ty * kB + tx; q < kSR * kSR; q += kB * kB)
            if (q / kSR < kM || q % kSR < kM) s_r[q] = 0.0f;
    float* const my_a = s_a + (ty + kM) * kSA + tx + kM;          // the thread's pixel (0, 0) in either plane
    float* const my_r = s_r + (ty + kM) * kSR + tx + kM;
    const auto ofa = [](int r, int dy, int c, int dx) { return (kB * r + dy) * kSA + kB * c + dx; };   // pixel (r, c) moved by (dy, dx)
    const auto ofr = [](int r, int dy, int c, int dx) { return (kB * r + dy) * kSR + kB * c + dx; };

    // down: a_1 .. a_(J-1)
#pragma unroll
    for (int j = 1; j < J; ++j) {
        const int h = 1 << (j - 1);
#pragma unroll
        for (int r = 0; r < kP; ++r)
#pragma unroll
            for (int c = 0; c < kP; ++c) my_a[ofa(r, 0, c, 0)] = pl[j - 1][r][c];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kP; ++r) {
#pragma unroll
            for (int c = 0; c < kP; ++c)
                pl[j][r][c] = haar_approx(pl[j - 1][r][c], my_a[ofa(r, 0, c, h)], my_a[ofa(r, h, c, 0)], my_a[ofa(r, h, c, h)]);
            __builtin_amdgcn_sched_barrier(0);                    // a row's twelve reads in flight at a time
        }
        __syncthreads();
    }
    // up: r_(J-1) .. r_0
    float res[kP][kP];
#pragma unroll
    for (int j = J; j >= 1; --j) {
        const int h = 1 << (j - 1);
#pragma unroll
        for (int r = 0; r < kP; ++r)
#pragma unroll
            for (int c = 0; c < kP; ++c) {
                my_a[ofa(r, 0, c, 0)] = pl[j - 1][r][c];
                if (j < J) my_r[ofr(r, 0, c, 0)] = res[r][c];
            }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kP; ++r)
#pragma unroll
            for (int c = 0; c < kP; ++c) {
                float w[3][3];
#pragma unroll
                for (int y = 0; y < 3; ++y)
#pragma unroll
                    for (int x = 0; x < 3; ++x) w[y][x] = (y == 1 && x == 1) ? pl[j - 1][r][c] : my_a[ofa(r, (y - 1) * h, c, (x - 1) * h)];
                float s00 = 0.0f, s01 = 0.0f, s10 = 0.0f, s11 = 0.0f;
                if (j < J) {
                    s00 = res[r][c];
                    s01 = my_r[ofr(r, 0, c, -h)];
                    s10 = my_r[ofr(r, -h, c, 0)];
                    s11 = my_r[ofr(r, -h, c, -h)];
                }
                res[r][c] = haar_ti_up(w, s00, s01, s10, s11, lam);   // (in place: r_j of the other pixels is read from s_r)
                // One pixel's eleven LDS reads in flight at a time, and its value formed here rather than sunk into the guarded store
                // at the end: the planes fill the registers.
                asm volatile("" : "+v"(res[r][c]));
                __builtin_amdgcn_sched_barrier(0);
            }
        if (j > 1) __syncthreads();
    }
    store_tile([&](int r, int c) { return haar_out(pl[0][r][c], res[r][c]); });
}

// ---- the naive TI form: one level per launch, one thread per pixel ------------------------------------------------------------------
constexpr int kPix = 256;

// a_(j-1) at (i, k): the plane a.a_src, or v itself for j = 1
template <bool ZU>
__device__ __forceinline__ float haar_src(const HaarArgs& a, size_t base, int i, int k) {
    const size_t idx = base + (size_t)i * a.W + k;
    return a.a_src ? a.a_src[idx] : haar_load<ZU>(a, base, (unsigned)(i * a.W + k));
}

template <bool ZU>
__global__ __launch_bounds__(kPix) void haar_ti_down_kernel(HaarArgs a) {
    const int chunks = a.tiles_x;                                 // workgroups per slice
    const int n = blockIdx.x / chunks;
    if (a.tact && a.tact[n] > 0.5f) return;
    const int q = (blockIdx.x - n * chunks) * kPix + threadIdx.x;
    const int H = a.H, W = a.W;
    if (q >= H * W) return;
    if (!(a.scale * a.lam[n] > 0.0f)) return;
    const int h = 1 << (a.level - 1);
    const int i = q / W, k = q - i * W, i2 = wrap1(i + h, H), k2 = wrap1(k + h, W);
    const size_t base = (size_t)n * H * W;
    a.a_dst[base + q] = haar_approx(haar_src<ZU>(a, base, i, k), haar_src<ZU>(a, base, i, k2), haar_src<ZU>(a, base, i2, k),
                                    haar_src<ZU>(a, base, i2, k2));
}

// level a.level up: r_(j-1) into a.r_dst, or for level 1 the closing clamp into a.out (which must not be the plane read as a_0)
template <bool ZU>
__global__ __launch_bounds__(kPix) void haar_ti_up_kernel(HaarArgs a) {
    const int chunks = a.tiles_x;
    const int n = blockIdx.x / chunks;
    if (a.tact && a.tact[n] > 0.5f) return;
    const int q = (blockIdx.x - n * chunks) * kPix + threadIdx.x;
    const int H = a.H, W = a.W;
    if (q >= H * W) return;
    const float lam = a.scale * a.lam[n];
    const size_t base = (size_t)n * H * W;
    if (!(lam > 0.0f)) {
        if (a.level == 1) a.out[base + q] = haar_clamp(haar_load<ZU>(a, base, (unsigned)q));
        return;
    }
    const int h = 1 << (a.level - 1);
    const int i = q / W, k = q - i * W;
    const int ii[3] = {wrap1(i - h, H), i, wrap1(i + h, H)}, kk[3] = {wrap1(k - h, W), k, wrap1(k + h, W)};
    float w[3][3];
#pragma unroll
    for (int y = 0; y < 3; ++y)
#pragma unroll
        for (int x = 0; x < 3; ++x) w[y][x] = haar_src<ZU>(a, base, ii[y], kk[x]);
    float s00 = 0.0f, s01 = 0.0f, s10 = 0.0f, s11 = 0.0f;
    if (a.r_src) {
        s00 = a.r_src[base + (size_t)ii[1] * W + kk[1]];
        s01 = a.r_src[base + (size_t)ii[1] * W + kk[0]];
        s10 = a.r_src[base + (size_t)ii[0] * W + kk[1]];
        s11 = a.r_src[base + (size_t)ii[0] * W + kk[0]];
    }
    const float up = haar_ti_up(w, s00, s01, s10, s11, lam);
    if (a.level == 1) a.out[base + q] = haar_out(haar_load<ZU>(a, base, (unsigned)q), up);
    else a.r_dst[base + q] = up;
}

// ---- ORTHO: a 16 x 16 tile per workgroup, the pyramid in LDS ---------------------------------------------------------------------------
constexpr int kOT = 16;                          // tile side: every image side is a multiple of it, and so is every block side 2^J
static_assert(kOT == 1 << kHaarMaxLevels, "a tile holds whole blocks");

template <bool ZU>
__global__ __launch_bounds__(kOT * kOT) void haar_ortho_kernel(HaarArgs a) {
    __shared__ float s_a[kHaarMaxLevels][kOT * kOT];       // s_a[j]: a_j of the tile, side 16 >> j
    __shared__ float s_r[kHaarMaxLevels][kOT * kOT];       // s_r[j]: r_j of the tile
    const int tiles = a.tiles_x * a.tiles_y;
    const int n = blockIdx.x / tiles, tl = blockIdx.x - n * tiles;
    if (a.tact && a.tact[n] > 0.5f) return;
    const int tby = tl / a.tiles_x, tbx = tl - tby * a.tiles_x;
    const int t = threadIdx.x;
    const size_t base = (size_t)n * a.H * a.W;
    const unsigned off = (unsigned)((tby * kOT + t / kOT) * a.W + tbx * kOT + t % kOT);
    const size_t idx = base + off;
    const float v = haar_load<ZU>(a, base, off);                        // (out may alias v: this thread's own pixel only)
    const float lam = a.scale * a.lam[n];
    if (!(lam > 0.0f)) { a.out[idx] = haar_clamp(v); return; }
    const int J = a.levels;
    s_a[0][t] = v;
    __syncthreads();
    for (int j = 1; j < J; ++j) {
        const int side = kOT >> j, fine = 2 * side;
        if (t < side * side) {
            const int o = 2 * (t / side) * fine + 2 * (t % side);
            s_a[j][t] = haar_approx(s_a[j - 1][o], s_a[j - 1][o + 1], s_a[j - 1][o + fine], s_a[j - 1][o + fine + 1]);
        }
        __syncthreads();
    }
    for (int j = J; j >= 1; --j) {
        const int side = kOT >> j, fine = 2 * side;
        if (t < side * side) {
            const int o = 2 * (t / side) * fine + 2 * (t % side);
            float q00, q01, q10, q11;
            haar_block(s_a[j - 1][o], s_a[j - 1][o + 1], s_a[j - 1][o + fine], s_a[j - 1][o + fine + 1], j < J ? s_r[j][t] : 0.0f, lam, q00,
                       q01, q10, q11);
            s_r[j - 1][o] = q00 * 0.5f;
            s_r[j - 1][o + 1] = q01 * 0.5f;
            s_r[j - 1][o + fine] = q10 * 0.5f;
            s_r[j - 1][o + fine + 1] = q11 * 0.5f;
        }
        __syncthreads();
    }
    a.out[idx] = haar_out(v, s_r[0][t]);
}

template <int J>
void launch_fused(const HaarArgs& a, dim3 grid, dim3 block, hipStream_t s) {
    if (a.z) hipLaunchKernelGGL((haar_ti_fused_kernel<J, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((haar_ti_fused_kernel<J, false>), grid, block, 0, s, a);
}

}  // namespace

hipError_t launch_haar_ti_fused(HaarArgs a, int N, hipStream_t s) {
    const int tile = haar_tile(a.levels);
    a.tiles_x = (a.W + tile - 1) / tile;
    a.tiles_y = (a.H + tile - 1) / tile;
    const dim3 grid((unsigned)((size_t)N * a.tiles_x * a.tiles_y)), block(kB, kB);
    switch (a.levels) {
        case 1: launch_fused<1>(a, grid, block, s); break;
        case 2: launch_fused<2>(a, grid, block, s); break;
        case 3: launch_fused<3>(a, grid, block, s); break;
        case 4: launch_fused<4>(a, grid, block, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_haar_ti_down(HaarArgs a, int N, hipStream_t s) {
    a.tiles_x = (a.H * a.W + kPix - 1) / kPix;
    a.tiles_y = 1;
    const dim3 grid((unsigned)((size_t)N * a.tiles_x)), block(kPix);
    if (a.z) hipLaunchKernelGGL(haar_ti_down_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(haar_ti_down_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_haar_ti_up(HaarArgs a, int N, hipStream_t s) {
    a.tiles_x = (a.H * a.W + kPix - 1) / kPix;
    a.tiles_y = 1;
    const dim3 grid((unsigned)((size_t)N * a.tiles_x)), block(kPix);
    if (a.z) hipLaunchKernelGGL(haar_ti_up_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(haar_ti_up_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_haar_ortho(HaarArgs a, int N, hipStream_t s) {
    a.tiles_x = a.W / kOT;
    a.tiles_y = a.H / kOT;
    const dim3 grid((unsigned)((size_t)N * a.tiles_x * a.tiles_y)), block(kOT * kOT);
    if (a.z) hipLaunchKernelGGL(haar_ortho_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(haar_ortho_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace pnp
