/*
 * pnpadmm_dcf.h - extension of the C ABI of libpnpadmm.so (pnpadmm.h, pnpadmm_ncsense.h, pnpadmm_toeplitz.h): sample density weights for
 * ANY trajectory, by Pipe and Menon's iteration (MRM 41:179, 1999) on the handle's NUFFT plan.  Everything pnpadmm.h says about pointers,
 * streams, status codes and sizes holds here; the entry points live in the same library and take the same handle.
 *
 * Every non-Cartesian stage takes sample weights W (A^H W A + mu I, aty = A^H W y, the PNP_RES_DC column, the spectrum of
 * pnp_toeplitz_plan).  An analytic ramp exists for radial spokes only.  For a trajectory (ky_m, kx_m), m < M, with G the plan's own gridding
 * matrix - per sample the footprint start (i0y_m, i0x_m) and the float32 kernel weights wy_m[0..J), wx_m[0..J) of pnp_nufft_plan -
 *     Psi = G G^T,      w <- w / (Psi w)      (elementwise)
 * drives Psi w to 1: the weighted samples then grid to a flat density.  Psi is a real spread and a real gather; no transform and no
 * deconvolution take part.
 *
 * THE EXPRESSIONS.  All arithmetic is float64; wy, wx are the plan's float32 numbers promoted exactly; every product-sum is one fma.
 *     g[r][c]    = the fma chain from +0, over the samples m' whose periodic footprint holds (r, c), in ascending m', of
 *                      fma(a, wx_m'[e], .),  a = w_m' * wy_m'[d] (rounded once),  d = (r - i0y_m') mod gh < J,  e = (c - i0x_m') mod gw < J
 *                  (the order of the NUFFT adjoint's gridding; one workgroup per 16 x 16 tile walks the tile's bin; every grid point is
 *                  written on every call, zeros included)
 *     (Psi w)_m  = the chain from +0 over iy = 0 .. J-1 of fma(wy_m[iy], t_iy, .),
 *                  t_iy = the chain from +0 over ix = 0 .. J-1 of fma(wx_m[ix], g[(i0y_m + iy) mod gh][(i0x_m + ix) mod gw], .)
 *                  (the order of the NUFFT forward's interpolation)
 *     w_m       <- w_m / (Psi w)_m        one division.  Psi w > 0 always: the kernel is positive on its support and w > 0, so there is no guard
 *                  value, and coincident samples (the k = 0 of every radial spoke) are no special case: they see each other through g.
 * No atomics and no partial sums in the chains: the bits depend on (plan, w0, iters) only - not on N, the stream or the call.
 * THE FINISH.  s = sum_m w_m in float64 by the library's fixed tree (chunks of 2048 samples, then the chunk sums in ascending order through
 * the same tree); w_m <- float32(w_m * (H W / s)): one division, one multiplication, one rounding to float32.  sum w = H W is the convention of
 * the radial ramp, so that a penalty mu means the same with either.
 * info[k], k < iters, = float32(max_m |(Psi w)_m - 1|) for the w that ENTERS iteration k (k = 0: the start); info[iters] the same for the
 * result of the last iteration, BEFORE the finish scales it (the fixed point of the iteration is Psi w = 1; the scale is a convention).
 * A maximum does not depend on order, so info is bitwise reproducible too.  With info the call runs one more spread and gather.
 *
 * pnp_nufft_psi: out[m] = float32((Psi w)_m) for the caller's w, DEVICE float32 [M]; out DEVICE float32 [M]; out may alias w.
 * pnp_nufft_dcf: `iters` iterations (1..PNP_DCF_MAX_ITERS) from w0, DEVICE float32 [M], or NULL = all ones, then the finish; w DEVICE
 * float32 [M], may alias w0; info DEVICE float32 [iters + 1] or NULL.  flags: reserved, must be 0.
 * w0 MUST BE POSITIVE AND FINITE.  Both calls read an entry of their input that is not (> 0 and finite) - zero, negative, NaN, infinity -
 * as 1.0, the uniform start, so that Psi w > 0 holds whatever the caller passes: no division by zero, and no NaN that spreads through g to
 * the neighbours' weights.  The Python layer refuses such an input instead (ValueError).
 *
 * LAUNCHES.  An iteration is two launches, the finish two more; all are queued on the caller's stream and the calls return without
 * waiting.  No launch waits on another workgroup.
 * WORKSPACE.  Allocated inside the call, all-or-nothing through the handle's workspace and counted by pnp_workspace_bytes: the grid,
 * 8 gh gw bytes; w in float64, 8 M; the chunk sums, 8 ceil(M / 2048); the workgroup maxima, 4 (iters + 1) ceil(M / 256) (only with info).
 * The workspace is this feature's own: it shares nothing with the NUFFT pair's grid or any stage's scratch, so either call between two
 * steps of a live episode changes no bit of that episode.  Calls on one handle are stream-ordered.
 *
 * Both read the handle's current NUFFT plan (pnp_nufft_plan); without one they return PNP_ERR_INVALID and the message names
 * pnp_nufft_plan.  The argument errors that need no handle - iters out of range, flags != 0, a NULL w / out - are reported before the
 * handle is looked at; every error is reported before any HIP call and leaves the outputs untouched.
 *
 * (The entry points are declared here so that the tables that mirror the three older headers stay as they are.)
 */
#ifndef PNPADMM_DCF_H
#define PNPADMM_DCF_H

#include "pnpadmm.h"

#define PNP_DCF_MAX_ITERS 256

#ifdef __cplusplus
extern "C" {
#endif

int pnp_nufft_psi(pnp_handle h, const float* w, float* out, void* stream);
int pnp_nufft_dcf(pnp_handle h, const float* w0, int iters, int flags, float* w, float* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PNPADMM_DCF_H */
