/*
 * pnpadmm_fieldmap.h - extension of the C ABI of libpnpadmm.so (pnpadmm.h): the B0 field map of pnpadmm_offres.h estimated from two echo
 * images by the regularised fit of Funai, Fessler et al., "Regularized field map estimation in MRI", IEEE TMI 2008 (first-order roughness,
 * unit curvatures).  Everything pnpadmm.h says about pointers, streams, status codes and sizes holds here; the entry points live in the same
 * library and take the same handle, of any kind and any size pnp_create accepts.
 *
 * THE MODEL.  The sign is pnpadmm_offres.h's: a sample taken at t sees the object times exp(-i omega t).  x1 and x2 are the images at the
 * echo times TE and TE + dte, so x1 conj(x2) has the phase +omega dte.  The fit works in phase units, theta = omega dte.  Per slice and pixel j:
 *     s_j   = sum_c x1_c conj(x2_c)
 *     m_j   = |s_j|,   phi_j = arg s_j,   w_j = m_j / max_j m_j
 *     Psi(theta) = sum_j w_j (1 - cos(theta_j - phi_j)) + (beta / 2) sum over 4-neighbour pairs {j,k} (theta_j - theta_k)^2
 * The ends are Neumann: a neighbour outside the image is absent.  The cosine's curvature is at most 1 and De Pierro's split of a pair term,
 * (a - b)^2 <= (2 a - a' - b')^2 / 2 + (2 b - a' - b')^2 / 2 with equality at (a', b'), majorise Psi at the iterate by a quadratic that is
 * SEPARABLE over the pixels with curvature w_j + 2 beta nn_j (nn_j = the number of neighbours, 2..4).  Minimising it moves every pixel at once
 * (Jacobi: every pixel reads the iterate of the sweep before), and because the surrogate is separable the simultaneous update DESCENDS: Psi
 * never increases along the iteration in exact arithmetic (tests/test_fieldmap_host.py holds the float64 restatement to that on three seeds;
 * the step needed no change and has no constant beyond the 2 of the split).
 * NO PHASE UNWRAPPING: phi lies in (-pi, pi], and the estimate is valid for |omega| dte < pi (acquisition.field_map_dte chooses dte from the
 * largest frequency expected).  Unwrapping, second-order roughness, more than two echoes and Huber curvatures are OUT OF SCOPE.
 *
 * EXPRESSION ORDER.  float32 throughout except where written; every operation named below is ONE IEEE operation, in this order, an fma only
 * where one is written (the unit is compiled with floating-point contraction off).  tests/fieldmap_ref.py restates it in numpy float32.
 *   prepare   s = (+0, +0); for c ascending, with x1_c = (a, b) and x2_c = (p, q):
 *                 s.x = fma(a, p, s.x);  s.x = fma(b, q, s.x);  s.y = fma(b, p, s.y);  s.y = fma(-a, q, s.y)
 *             m_j   = sqrt(fma(s.x, s.x, s.y * s.y))                        IEEE square root
 *             phi_j = float32(atan2((double)s.y, (double)s.x))              rounded once, as the maps of pnpadmm_offres.h
 *   weights   mx = max_j m_j (a maximum does not depend on the order);  ri = mx > 0 ? 1 / mx : 0   one IEEE reciprocal per slice
 *             w_j = m_j * ri;   rd_j = 1 / fma(2 beta, nn_j, w_j)           (2 beta and nn_j are exact); a slice with mx = 0: w = 0, omega = +0
 *   sweep     theta^0 = phi; `iters` times, with t = theta_j and up / down / left / right its neighbours in the iterate of the sweep before
 *             (an absent neighbour reads t itself, so its term is exactly +0):
 *                 sn  = sinf(t - phi_j)                                     the device's sinf, the same function in every kernel
 *                 lap = ((t - up) + (t - down)) + ((t - left) + (t - right))
 *                 g   = fma(beta, lap, w_j * sn)                            the product rounded first
 *                 theta_j <- fma(-g, rd_j, t)
 *   finish    omega_j = float32((double)theta_j / dte)
 * A pixel-constant phase difference (phi the same float32 on every pixel of a slice) comes back bit for bit for any iters: lap and sn are
 * exactly 0.  iters = 0 gives the raw phase difference phi / dte.
 *
 * THE FUSED KERNEL.  One workgroup of 32 x 32 threads owns a 128 x 128 REGION of a slice; every thread keeps a 4 x 4 patch of theta, phi, w
 * and rd in registers.  A sweep has dependency radius 1, so after t sweeps the region is right everywhere but in a band of t pixels along
 * its edge.  With T = PNP_FIELDMAP_T = 10 sweeps per launch the workgroup stores its TILE, the region minus 10 pixels all round: 108 x 108,
 * redundant-compute factor (128 / 108)^2 = 1.40.  Only a patch's rim crosses threads, through LDS (four float4 per thread, 64 KiB per
 * workgroup, two barriers per sweep).  iters > T runs ceil(iters / T) launches - whole launches of T and one shorter one - that hand theta
 * over through two planes of the workspace in turn (a launch reads the halo of its neighbours' tiles from the plane it does not write);
 * launches are queued without host synchronisation.  THE NAIVE FORM (PNP_FIELDMAP_NAIVE=1, read at pnp_create): one launch per sweep, one
 * thread per pixel, the same ping-pong; the bit-for-bit check of the fused kernel and its timing baseline, as PNP_TV_NAIVE is.  Both forms
 * evaluate the one device function of the sweep and give the same bits.  Which form ships was decided by measurement.
 *
 * pnp_fieldmap_cost evaluates Psi at the caller's omega with theta_j = float32((double)omega_j * dte) and phi, w of the prepare and weights
 * steps above.  Its terms are float64: w_j (1 - cos((double)theta_j - phi_j)) and, per pixel, the pairs with its right and its lower
 * neighbour, (beta / 2) (dr^2 + dd^2) with beta / 2 formed in float64 from the float32 beta.  They are summed in a fixed order: per workgroup
 * of 2048 consecutive pixels by the tree of block_reduce.h, then over the workgroups ascending.  It is the reference-free convergence figure
 * of this estimator, as pnp_residuals is of ADMM.
 *
 *   x1, x2 : DEVICE complex64 [N,C,H,W], C = coils, 1..PNP_MC_MAX_COILS, N the handle's n
 *   dte    : seconds, finite and > 0;   beta : finite and > 0;   iters : 0..PNP_FIELDMAP_MAX_ITERS;   flags : reserved, must be 0
 *   omega  : DEVICE float32 [N,H,W] rad/s - the layout pnp_offres_maps takes at map_n == N
 *   weight : DEVICE float32 [N,H,W] or NULL: receives w, which callers use as a confidence mask
 *   cost   : DEVICE float64 [N]
 *
 * PROPERTIES.  A slice's output is a pure function of its own x1, x2, C, dte, beta and iters: not of N, the slice's place in the batch, the
 * stream, or the tile plan.  No atomics, no cross-workgroup waits; bitwise reproducible.  The calls change neither the handle's mode nor any
 * installed constants, and work in a workspace of their own (the phi, w and rd planes, the two planes of theta: 20 N H W bytes, and the
 * partial maxima and sums), so a call between two steps of a live episode disturbs nothing.  The workspace follows the setup-time semantics
 * of pnp_tv_denoise: allocated inside the first call, all-or-nothing, counted by pnp_workspace_bytes, never replaced.  Calls on one handle
 * are stream-ordered.  Every argument error (NULLs, coils, iters, a dte or beta that is out of range or not finite, flags != 0) is reported
 * before any HIP call and leaves the outputs untouched.
 */
#ifndef PNPADMM_FIELDMAP_H
#define PNPADMM_FIELDMAP_H

#include "pnpadmm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PNP_FIELDMAP_MAX_ITERS 4096
/* sweeps per launch of the fused kernel */
#define PNP_FIELDMAP_T 10

int pnp_fieldmap_estimate(pnp_handle h, const float* x1, const float* x2, int coils, double dte, float beta, int iters, int flags, float* omega,
                          float* weight, void* stream);
int pnp_fieldmap_cost(pnp_handle h, const float* x1, const float* x2, int coils, double dte, float beta, const float* omega, double* cost,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PNPADMM_FIELDMAP_H */
