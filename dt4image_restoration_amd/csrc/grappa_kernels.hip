// GRAPPA (pnp_grappa_weights / pnp_grappa_apply): autocalibrated k-space interpolation.  The undersampled axis is W; the acquired columns are the
// comb x = offset (mod R).  A kernel of `by` rows (odd) by `bx` comb columns (2 or 4) synthesises the R - 1 columns to the right of a comb column xa
// from their acquired neighbours, per slice, C coils:
//     sources (c, y + i - by/2, xa + (j - (bx/2 - 1)) R), s = (c by + i) bx + j, ns = C by bx        targets (c', y, xa + r), t = c' (R-1) + (r-1)
//     calibration, with the centred acs_h x acs_w block B of coilmap_kernels.hip and every window (wy, wx) that fits, span = (bx-1) R + 1:
//         A[w][s] = B[c][wy+i][wx+jR]      T[w][t] = B[c'][wy+by/2][wx+(bx/2-1)R+r]      M = A^H [A | T]      (G + lam tr(G)/ns I) X = Rh
//
//   grappa_gram_kernel       grid (ceil(ns (ns+nt) / 256), N): one thread per entry M[s][j]; the left block only for j <= s, mirrored.  It walks the
//                            windows in row-major order: re += xr yr; re += xi yi; im += xr yi; im -= xi yr (x = A[w][s], y = Z[w][j]), float64
//                            (the products of float32 values are exact).  The diagonal's imaginary part is 0.
//   grappa_solve_kernel      grid (N), one workgroup of 512 threads per slice, float64, the matrix M [ns][ns+nt] in the slice's global workspace; the
//                            workgroup's barriers order its accesses.  L is kept TRANSPOSED in the upper triangle of the left block
//                            (L[i][k] at M[k][i], k < i; the mirror makes M[k][i] = conj(M[i][k]) exactly), so that the threads of a column step
//                            read neighbouring addresses.  Cholesky by the column formulas of prewhiten_chol_kernel: thread i >= j sums
//                            s = sum_{k<j} L[i][k] conj(L[j][k]), k ascending from 0.0; d = G[j][j] - Re s; L[j][j] = sqrt(d);
//                            L[i][j] = (G[i][j] - s) / L[j][j].  A pivot that is not finite, not positive or not above kPivotEps * max diag ends
//                            it: info = j + 1 and the weights are +0.  Then thread t < nt owns right-hand side t: forward
//                            Y[i] = (Rh[i] - sum_{k<i} L[i][k] Y[k]) / L[i][i], i and k ascending, and backward
//                            X[i] = (Y[i] - sum_{k>i} conj(L[k][i]) X[k]) / L[i][i], i descending, k ascending, in place in the right block.
//                            wts[t][s] = X[s][t], one rounding to complex64.
//   grappa_apply_kernel      grid (ceil(W/R / 8), ceil(H / 8), N): a workgroup owns 8 rows x 8 comb columns and stages their source patch
//                            ((8 + by - 1) x (8 + bx - 1) comb bins per coil, indices periodic) in LDS once.  Lane l of EVERY wave owns position
//                            (l / 8, l % 8); wave w takes the target groups w, w + waves, ... of TT targets each, so a wave's weights are
//                            wave-uniform (scalar loads) and every source value a lane reads from LDS feeds TT complex accumulators:
//                                re = fma(a.x, x.x, re); re = fma(-a.y, x.y, re); im = fma(a.x, x.y, im); im = fma(a.y, x.x, im), s ascending from +0.
//                            A target bin whose mask byte is set stores the bits of y0 instead; the comb bins are copied from the staged patch.
// No atomics anywhere: a slice's bits depend on its own input and the arguments only.
#include "pnp_internal.h"
#include "hermitian.h"
#include "../../include/pnpadmm.h"

namespace pnp {

namespace {

constexpr int kGrThreads = 256;
constexpr int kGrSolveThreads = PNP_GRAPPA_MAX_SRC;             // a thread per row of the factorisation
constexpr int kGrMaxTargets = PNP_GRAPPA_MAX_COILS * (PNP_GRAPPA_MAX_ACCEL - 1);
static_assert(kGrMaxTargets <= kGrSolveThreads, "a thread per right-hand side");
constexpr double kGrPivotEps = 1e-12;
constexpr int kGrRows = 8, kGrCols = 8;                          // positions of a workgroup: one per lane
static_assert(kGrRows * kGrCols == 64, "one position per lane of a wave");

// grid (ceil(ns * ld / 256), N); ws: per slice M [ns][ld], ld = ns + nt; gram: the same layout or nullptr
__global__ __launch_bounds__(kGrThreads) void grappa_gram_kernel(const float2* __restrict__ y, int C, int acs_h, int acs_w, int R, int by, int bx,
                                                                 int ns, int nt, double2* __restrict__ ws, double2* __restrict__ gram, int H,
                                                                 int W) {
    const int n = blockIdx.y, idx = blockIdx.x * kGrThreads + threadIdx.x, ld = ns + nt;
    if (idx >= ns * ld) return;
    const int s = idx / ld, j = idx - s * ld;
    if (j < ns && j > s) return;
    const int y0 = (H >> 1) - (acs_h >> 1), x0 = (W >> 1) - (acs_w >> 1), span = (bx - 1) * R + 1, kk = by * bx;
    const size_t HW = (size_t)H * W;
    const int ca = s / kk, ia = (s - ca * kk) / bx, ja = s - ca * kk - ia * bx;
    const float2* pa = y + ((size_t)n * C + ca) * HW + (size_t)(y0 + ia) * W + (x0 + ja * R);
    const float2* pb;
    if (j < ns) {
        const int cb = j / kk, ib = (j - cb * kk) / bx, jb = j - cb * kk - ib * bx;
        pb = y + ((size_t)n * C + cb) * HW + (size_t)(y0 + ib) * W + (x0 + jb * R);
    } else {
        const int t = j - ns, cb = t / (R - 1), r = t - cb * (R - 1) + 1;
        pb = y + ((size_t)n * C + cb) * HW + (size_t)(y0 + (by >> 1)) * W + (x0 + ((bx >> 1) - 1) * R + r);
    }
    double re = 0.0, im = 0.0;
    for (int wy = 0; wy <= acs_h - by; ++wy)
        for (int wx = 0; wx <= acs_w - span; ++wx) {
            const float2 p = pa[wy * W + wx], q = pb[wy * W + wx];
            re += (double)p.x * (double)q.x;
            re += (double)p.y * (double)q.y;
            im += (double)p.x * (double)q.y;
            im -= (double)p.y * (double)q.x;
        }
    const size_t base = (size_t)n * ns * ld;
    if (j == s) im = 0.0;
    ws[base + idx] = make_double2(re, im);
    if (gram) gram[base + idx] = make_double2(re, im);
    if (j < s) {
        ws[base + (size_t)j * ld + s] = make_double2(re, -im);
        if (gram) gram[base + (size_t)j * ld + s] = make_double2(re, -im);
    }
}

// grid (N); ws: per slice M [ns][ld] (destroyed); wts [N][nt][ns]; info [N].  ws is read and written through this one pointer only.
__global__ __launch_bounds__(kGrSolveThreads) void grappa_solve_kernel(double2* ws, int ns, int nt, double lam, float2* __restrict__ wts,
                                                                       int* __restrict__ info) {
    __shared__ double diag[PNP_GRAPPA_MAX_SRC];                   // L[j][j]
    __shared__ double floor_s, shift_s;
    __shared__ int bad;                                           // 0, or j + 1 of the first refused pivot
    const int n = blockIdx.x, tid = threadIdx.x, ld = ns + nt;
    double2* M = ws + (size_t)n * ns * ld;
    if (tid == 0) {
        double tr = 0.0;
        for (int s = 0; s < ns; ++s) tr += M[(size_t)s * ld + s].x;
        const double shift = lam * tr / (double)ns;
        double m = M[0].x + shift;
        for (int s = 1; s < ns; ++s) m = fmax(m, M[(size_t)s * ld + s].x + shift);   // fmax drops a NaN; a NaN diagonal is caught as its own pivot
        shift_s = shift;
        floor_s = kGrPivotEps * m;
        bad = 0;
    }
    __syncthreads();
    const double floor_ = floor_s, shift = shift_s;
    const int i = tid;
    for (int j = 0; j < ns; ++j) {
        double2 s = make_double2(0.0, 0.0);
        if (i >= j && i < ns) {
            for (int k = 0; k < j; ++k) {
                const double2 a = M[(size_t)k * ld + i], b = M[(size_t)k * ld + j];      // L[i][k], L[j][k]
                s.x += a.x * b.x;
                s.x += a.y * b.y;
                s.y += a.y * b.x;
                s.y -= a.x * b.y;
            }
        }
        if (i == j) {
            const double d = (M[(size_t)j * ld + j].x + shift) - s.x;
            if (!(d > floor_) || !(d > 0.0) || !(d <= 1.7976931348623157e308)) {    // NaN fails the first test, +inf the last
                bad = j + 1;
            } else {
                diag[j] = sqrt(d);
            }
        }
        __syncthreads();
        if (bad) break;
        if (i > j && i < ns) {
            const double2 p = M[(size_t)j * ld + i];               // conj(G[i][j])
            const double r = diag[j];
            M[(size_t)j * ld + i] = make_double2((p.x - s.x) / r, (-p.y - s.y) / r);
        }
        __syncthreads();
    }
    const int failed = bad;
    if (!failed && tid < nt) {
        double2* X = M + ns + tid;                                // X[i] at X[i * ld]
        for (int r = 0; r < ns; ++r) {
            double2 s = make_double2(0.0, 0.0);
            for (int k = 0; k < r; ++k) {
                const double2 a = M[(size_t)k * ld + r], b = X[(size_t)k * ld];
                s.x += a.x * b.x;
                s.x -= a.y * b.y;
                s.y += a.x * b.y;
                s.y += a.y * b.x;
            }
            const double2 p = X[(size_t)r * ld];
            const double d = diag[r];
            X[(size_t)r * ld] = make_double2((p.x - s.x) / d, (p.y - s.y) / d);
        }
        for (int r = ns - 1; r >= 0; --r) {
            double2 s = make_double2(0.0, 0.0);
            for (int k = r + 1; k < ns; ++k) {
                const double2 a = M[(size_t)r * ld + k], b = X[(size_t)k * ld];          // conj(a) b, a = L[k][r]
                s.x += a.x * b.x;
                s.x += a.y * b.y;
                s.y += a.x * b.y;
                s.y -= a.y * b.x;
            }
            const double2 p = X[(size_t)r * ld];
            const double d = diag[r];
            X[(size_t)r * ld] = make_double2((p.x - s.x) / d, (p.y - s.y) / d);
        }
    }
    __syncthreads();
    if (tid == 0) info[n] = failed;
    // one rounding; x + 0.0: a zero comes out as +0
    float2* out = wts + (size_t)n * nt * ns;
    for (int idx = tid; idx < nt * ns; idx += kGrSolveThreads) {
        const int t = idx / ns, s = idx - t * ns;
        float2 v = make_float2(0.f, 0.f);
        if (!failed) {
            const double2 x = M[(size_t)s * ld + ns + t];
            v = make_float2((float)(x.x + 0.0), (float)(x.y + 0.0));
        }
        out[idx] = v;
    }
}

// grid (ceil(W/R / 8), ceil(H / 8), N), 64 * waves threads; dynamic LDS: the patch [C][8 + by - 1][8 + BX - 1]
template <int BX, int TT>
__global__ __launch_bounds__(kGrThreads) void grappa_apply_kernel(const float2* __restrict__ y0, const uint8_t* __restrict__ mask, int mask_n,
                                                                  const float2* __restrict__ wts, int wts_n, float2* __restrict__ out, int C,
                                                                  int H, int W, int R, int offset, int by, int ns, int nt) {
    extern __shared__ float2 gr_patch[];
    constexpr int PC = kGrCols + BX - 1;
    const int PR = kGrRows + by - 1, ncomb = W / R, n = blockIdx.z, tid = threadIdx.x, threads = blockDim.x;
    const int yb = blockIdx.y * kGrRows, qb = blockIdx.x * kGrCols;
    const size_t HW = (size_t)H * W;
    const float2* src = y0 + (size_t)n * C * HW;
    float2* dst = out + (size_t)n * C * HW;
    // every staged index is reduced mod H and mod W / R: no read leaves the slice
    for (int idx = tid; idx < C * PR * PC; idx += threads) {
        const int c = idx / (PR * PC), rem = idx - c * (PR * PC), pr = rem / PC, pc = rem - pr * PC;
        const int yy = (yb + pr - (by >> 1) + H) % H;
        const int qq = ((qb + pc - (BX / 2 - 1)) % ncomb + ncomb) % ncomb;
        gr_patch[idx] = src[(size_t)c * HW + (size_t)yy * W + (offset + qq * R)];
    }
    __syncthreads();
    // the comb bins of the tile, every coil
    for (int idx = tid; idx < C * 64; idx += threads) {
        const int c = idx >> 6, l = idx & 63, py = l >> 3, pq = l & 7;
        if (yb + py < H && qb + pq < ncomb)
            dst[(size_t)c * HW + (size_t)(yb + py) * W + (offset + (qb + pq) * R)] = gr_patch[(c * PR + py + (by >> 1)) * PC + pq + (BX / 2 - 1)];
    }
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), waves = threads >> 6, lane = tid & 63;
    const int ly = lane >> 3, lq = lane & 7, yy = yb + ly, q = qb + lq;
    const bool live = yy < H && q < ncomb;
    const int xa = offset + q * R;
    const float2* wbase = wts + (wts_n > 1 ? (size_t)n * nt * ns : 0);
    const uint8_t* mrow = mask + (mask_n > 1 ? (size_t)n * HW : 0) + (size_t)(live ? yy : 0) * W;
    const float2* p0 = gr_patch + ly * PC + lq;
    for (int t0 = wave * TT; t0 < nt; t0 += waves * TT) {
        const float2* wt[TT];
        float re[TT], im[TT];
#pragma unroll
        for (int k = 0; k < TT; ++k) {
            wt[k] = wbase + (size_t)min(t0 + k, nt - 1) * ns;     // a group's tail repeats the last target and is not stored
            re[k] = im[k] = 0.f;
        }
        int s = 0;
        for (int c = 0; c < C; ++c)
            for (int i = 0; i < by; ++i) {
                const float2* row = p0 + (c * PR + i) * PC;
#pragma unroll
                for (int j = 0; j < BX; ++j) {
                    const float2 x = row[j];
#pragma unroll
                    for (int k = 0; k < TT; ++k) {
                        const float2 a = wt[k][s + j];
                        re[k] = fmaf(a.x, x.x, re[k]);
                        re[k] = fmaf(-a.y, x.y, re[k]);
                        im[k] = fmaf(a.x, x.y, im[k]);
                        im[k] = fmaf(a.y, x.x, im[k]);
                    }
                }
                s += BX;
            }
        if (!live) continue;
#pragma unroll
        for (int k = 0; k < TT; ++k) {
            const int t = t0 + k;
            if (t >= nt) break;
            const int ct = t / (R - 1), r = t - ct * (R - 1) + 1;
            int x = xa + r;
            if (x >= W) x -= W;
            const size_t o = (size_t)ct * HW + (size_t)yy * W + x;
            dst[o] = mrow[x] ? src[o] : make_float2(re[k], im[k]);
        }
    }
}

}  // namespace

hipError_t launch_grappa_gram(const float2* y, int C, int acs_h, int acs_w, int R, int by, int bx, double2* ws, double2* gram, int N, int H, int W,
                              hipStream_t s) {
    const int ns = C * by * bx, nt = C * (R - 1);
    const unsigned blocks = (unsigned)(((size_t)ns * (ns + nt) + kGrThreads - 1) / kGrThreads);
    hipLaunchKernelGGL(grappa_gram_kernel, dim3(blocks, N), dim3(kGrThreads), 0, s, y, C, acs_h, acs_w, R, by, bx, ns, nt, ws, gram, H, W);
    return hipGetLastError();
}

hipError_t launch_grappa_solve(double2* ws, int ns, int nt, double lam, float2* wts, int* info, int N, hipStream_t s) {
    hipLaunchKernelGGL(grappa_solve_kernel, dim3(N), dim3(kGrSolveThreads), 0, s, ws, ns, nt, lam, wts, info);
    return hipGetLastError();
}

hipError_t launch_grappa_apply(const float2* y0, const uint8_t* mask, int mask_n, const float2* wts, int wts_n, float2* out, int C, int R,
                               int offset, int by, int bx, int N, int H, int W, hipStream_t s) {
    const int ns = C * by * bx, nt = C * (R - 1), ncomb = W / R;
    // targets per wave group: 4 (8 accumulators per lane) once that leaves every wave of a pair a group, else 2
    const int tt = nt >= 8 ? 4 : 2;
    const int groups = (nt + tt - 1) / tt;
    // the most waves (at most 4) that deal the groups out evenly; else 4
    int waves = groups < 4 ? groups : 4;
    if (groups > 4 && groups % 4) {
        const int rounds4 = (groups + 3) / 4;
        for (int w = 3; w >= 2; --w)
            if (groups % w == 0 && groups / w <= rounds4) { waves = w; break; }
    }
    const dim3 grid((unsigned)((ncomb + kGrCols - 1) / kGrCols), (unsigned)((H + kGrRows - 1) / kGrRows), (unsigned)N);
    const size_t lds = (size_t)C * (kGrRows + by - 1) * (kGrCols + bx - 1) * sizeof(float2);   // at most 32 * 14 * 11 * 8 = 39424 bytes
#define GR_LAUNCH(BX, TT)                                                                                                                       \
    hipLaunchKernelGGL((grappa_apply_kernel<BX, TT>), grid, dim3(64 * waves), lds, s, y0, mask, mask_n, wts, wts_n, out, C, H, W, R, offset, by, \
                       ns, nt)
    if (bx == 2 && tt == 2) GR_LAUNCH(2, 2);
    else if (bx == 2) GR_LAUNCH(2, 4);
    else if (bx == 4 && tt == 2) GR_LAUNCH(4, 2);
    else if (bx == 4) GR_LAUNCH(4, 4);
    else return hipErrorInvalidValue;
#undef GR_LAUNCH
    return hipGetLastError();
}

}  // namespace pnp
