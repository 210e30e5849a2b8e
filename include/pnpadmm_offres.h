/*
 * pnpadmm_offres.h - extension of the C ABI of libpnpadmm.so (pnpadmm.h): off-resonance correction of non-Cartesian data by time
 * segmentation (Noll 1991), as a NUFFT-like operator pair and a CG data-fidelity stage.  Everything pnpadmm.h says about pointers, streams,
 * status codes and sizes holds here; the entry points live in the same library and take the same handle.
 *
 * THE MODEL.  omega is the field map in rad/s per pixel, t_m the time of sample m in seconds, one per sample of the trajectory of
 * pnp_nufft_plan and shared by the handle's slices like the trajectory itself.  A sample taken at t sees the object times exp(-i omega t):
 *     exact      (A p)_m = sum_r p(r) exp(-i omega(r) t_m) exp(-i 2 pi k_m . r)
 * pnp_offres_plan places L segment centres tau_l = t_min + l D, D = (t_max - t_min) / (L - 1), and interpolates linearly between the two
 * centres around t_m:  seg_m = min(floor((t_m - t_min) / D), L - 2),  b = (t_m - tau_seg) / D clamped to [0, 1],  b1_m = float32(b),
 * b0_m = float32(1 - b); seg, tau and b are float64 on the host, b0 and b1 stored as float32.  Exactly two segments carry a sample.
 *     E_l(r)   = exp(-i omega(r) tau_l)                                       complex64 maps [map_n, L, H, W]
 *     A p      = [ b0_m F_nu(E_seg . p)_m + b1_m F_nu(E_seg+1 . p)_m ]_m
 *     A^H q    = sum_l conj(E_l) . F_nu^H( w . b_l . q )
 *     Nop(p)   = A^H W A p + mu_n p
 * L = 1: tau_0 = (t_min + t_max) / 2, b0 = 1, no second segment.  L > 1 with t_max == t_min is refused.
 * ERROR OF THE MODEL.  Between two centres the chord deviates from the arc by at most 1 - cos(omega D / 2), so
 *     |A p - A_exact p|_m  <=  (1 - cos(omega_max D / 2)) ||p||_1   for every m
 * (on top of the NUFFT's own error).  Min-max interpolators, coils times segments, and a Toeplitz form of this operator are OUT OF SCOPE:
 * the stage is single-coil and its CG runs on the gridding form; the _tz installers of pnpadmm_toeplitz.h are untouched.  (Coils times
 * segments have since been added as an operator pair and a stage of their own: pnpadmm_offres_mc.h.  This header is as it was.)
 *
 * EXPRESSION ORDER.  float32 throughout; every operation named below is ONE IEEE operation, an fma only where one is written.  F_nu / F_nu^H
 * are pnp_nufft_forward_mc / pnp_nufft_adjoint_mc of pnpadmm_ncsense.h with the L maps E_l in the place of the coil maps: the segment image
 * (each product rounded, then the sum), the factor cy cx, the transform, the gather's two ascending fma chains, the gridding's one fma chain
 * from +0 over ascending sample index, the crop and the combine chain over ascending l are that header's, word for word.
 *   maps      ph = (double)omega * tau_l, E_l = (float32(cos ph), float32(-sin ph)): phase, sine and cosine in float64, rounded once
 *   forward   with v0, v1 the gathers of the segment grids seg_m and seg_m + 1:  o = (b0 v0.x, b0 v0.y), the products rounded; then
 *             o = (fma(b1, v1.x, o.x), fma(b1, v1.y, o.y)).  L = 1: o = (b0 v0.x, b0 v0.y) = v0
 *   adjoint   the sample value of segment l is t = (b q.x, b q.y) with b = b0_m for l = seg_m and b1_m for l = seg_m + 1, rounded FIRST;
 *             then pnp_nufft_adjoint's ((t w) wy) * wx chain over the samples that carry weight in l, ascending, from +0
 * So with L = 1 pnp_offres_forward / pnp_offres_adjoint have the bits of pnp_nufft_forward_mc / pnp_nufft_adjoint_mc at C = 1 on
 * pnp_offres_maps' output, and with every t_m on a centre (b in {0, 1}) they equal, as numbers, the multi-coil pair on the samples of
 * their segment (the sign of a zero aside: 0 . q may be -0).
 * SEGMENT BLOCKS.  The segment planes are processed in blocks of SB = min(L, 8) segments through the coil-block scratch of pnpadmm_ncsense.h
 * (8 N SB gh gw + 8 N SB M bytes).  A sample whose two segments fall into two blocks takes o = (b0 v0) from the first and the fma from the
 * second, through the output - a float32 partial stored and reloaded is the same float32 - so THE BITS DO NOT DEPEND ON SB.  The
 * environment variable PNP_OFFRES_SEG_BLOCK=k (1..32), read at pnp_create, overrides the 8: a check and a timing knob, not a mode.
 * THE NAIVE FORM.  The gather and the gridding exist twice.  Naive: the non-Cartesian SENSE launches on all L planes of the block - L J^2
 * grid reads per sample and L fma chains over every sample of a tile - between two small sample kernels, a blend after the gather and an
 * expansion (zeros where a sample carries no weight) before the gridding.  Two-segment: a gather that reads only the sample's two segment
 * grids and blends in registers, and a gridding whose workgroup of (segment, tile) walks a list the plan holds for it: the tile's bin
 * filtered to seg_m in {l - 1, l}, ascending (2 entries per bin entry instead of L).  A skipped sample and a sample that adds 0 . q leave
 * the same number, so both forms agree as numbers (torch.equal).  Which one a step runs is decided by measurement, not by the caller
 * (DESIGN.md 4a).  PNP_OFFRES_NAIVE=1 / 0, read at pnp_create, selects the naive / the two-segment form of both steps: the check and the
 * timing baseline, as PNP_NCSENSE_NAIVE is of the coil-batched kernels.  No atomics, no cross-workgroup waits.
 * A slice's outputs depend on (the plans, its inputs, its map) only: not on N, its place in the batch, the stream, or whether the map is
 * shared (map_n == 1) or given per slice with the same values; bitwise reproducible.
 *
 *   t        : HOST float64 [M], M = pnp_nufft_samples; finite;   segments : 1..PNP_MC_MAX_COILS;   flags : reserved, must be 0
 *   omega    : DEVICE float32 [H,W] (map_n == 1, shared by all slices) or [N,H,W] (map_n == N, N the handle's n)
 *   maps     : DEVICE complex64 [L,H,W] (map_n == 1) or [N,L,H,W]: pnp_offres_maps' output, or any maps of that shape
 *   n * min(L, SB) <= 65535
 *
 * pnp_offres_plan needs the plan of pnp_nufft_plan (PNP_ERR_STATE without one), builds tau, seg, b0, b1 and the per-(segment, tile) lists on
 * the host and uploads them (synchronous, like pnp_nufft_plan).  It replaces an earlier off-resonance plan and drops a live off-resonance
 * stage with it; pnp_nufft_plan drops the off-resonance plan together with any live off-resonance stage, as it drops the Toeplitz spectrum.
 * pnp_offres_segments: L of the plan, 0 without one (and on NULL).
 * pnp_offres_forward / pnp_offres_adjoint: img DEVICE complex64 [batch,H,W], samples DEVICE complex64 [batch,M], weights DEVICE float32 [M]
 * or NULL; 1 <= batch <= n; no input may alias an output.  They read the caller's maps directly.
 *
 * DATA FIDELITY.  pnp_set_kspace_offres / pnp_reset_offres copy y (complex64 [N,M]) and w (float32 [M] or NULL), build the maps of omega
 * into the handle's workspace, form aty = A^H W y once, and put the handle in off-resonance mode by the rule of pnpadmm.h: the stage that
 * runs is the one whose constants were installed LAST.  pnp_step and pnp_prox_dual then run the multi-coil section's CG on Nop and
 * b = aty + mu (x + u), exactly as in non-Cartesian SENSE mode (cg_iters : 1..PNP_MC_MAX_CG; stopped slices keep z, u and the CG residual
 * bit for bit).  pnp_reset_offres also sets the iterate: x = Re(x0), z = x0, u = 0.  In this mode
 *   - pnp_offres_live is 1; pnp_{mc,nc,ncsense}_cg_residual and pnp_{mc,nc,ncsense}_normal give PNP_ERR_STATE;
 *   - pnp_residuals' PNP_RES_DC column is sqrt(sum_m w_m |(A x)_m - y_m|^2) under the segmented A, summed as the non-Cartesian stage's;
 *   - snapshots, priors and drivers work unchanged; the installers of the other modes leave this mode.
 * The installers allocate or grow the handle's workspace inside the call (the segment-block scratch, y: 8 N M, w: 4 M, the maps:
 * 8 map_n L H W, the misfit's partial sums, and the CG's vectors), all-or-nothing and counted by pnp_workspace_bytes.  The handle changes
 * mode only after every launch of the install was accepted: a call that fails leaves the mode and the iterate as they were.
 * pnp_offres_normal (q = Nop(p); p, q DEVICE complex64 [N,1,H,W], must not alias; mu DEVICE float32 [N]) and pnp_offres_cg_residual (out
 * DEVICE float32 [N]) give PNP_ERR_STATE on a handle that is not in this mode.
 *
 * pnp_acquire_offres: pnp_acquire_nc with the segmented operator,  y = A gt + sigma_n (g_re + i g_im),  aty0 = A^H (dcf . y),
 * x0 = max(aty0, 0) on both planes; the same noise streams; gt DEVICE float32 [N,1,H,W], dcf DEVICE float32 [M] or NULL, y DEVICE complex64
 * [N,M], aty0, x0 complex64 [N,1,H,W] or NULL.  Its maps live in a workspace buffer of its own (8 map_n L H W bytes).
 *
 * pnp_offres_forward, pnp_offres_adjoint, pnp_offres_maps and pnp_acquire_offres change neither the handle's mode nor any installed
 * constants; they use, and may grow, the block scratch: calls on one handle are stream-ordered.  Every entry point reports every argument
 * error (NULLs, a count out of range, map_n not 1 or N, flags != 0, a time that is not finite, a zero span with L > 1, forbidden aliasing, no
 * plan, sigma_n negative or not finite) before any HIP call, leaving the outputs untouched.
 */
#ifndef PNPADMM_OFFRES_H
#define PNPADMM_OFFRES_H

#include "pnpadmm.h"

#ifdef __cplusplus
extern "C" {
#endif

int pnp_offres_plan(pnp_handle h, const double* t, int segments, int flags);
/* Segments of the off-resonance plan; 0 without one (and on NULL). */
int pnp_offres_segments(pnp_handle h);
int pnp_offres_maps(pnp_handle h, const float* omega, int map_n, float* maps, void* stream);
int pnp_offres_forward(pnp_handle h, const float* img, const float* maps, int map_n, int batch, float* samples, void* stream);
int pnp_offres_adjoint(pnp_handle h, const float* samples, const float* weights, const float* maps, int map_n, int batch, float* img, void* stream);
int pnp_set_kspace_offres(pnp_handle h, const float* y, const float* omega, int map_n, const float* w, int cg_iters, void* stream);
int pnp_reset_offres(pnp_handle h, const float* x0, const float* y, const float* omega, int map_n, const float* w, int cg_iters, float* x, float* z,
                     float* u, void* stream);
/* 1 while the off-resonance stage is the live one; 0 otherwise (and on NULL). */
int pnp_offres_live(pnp_handle h);
int pnp_offres_cg_residual(pnp_handle h, float* out, void* stream);
int pnp_offres_normal(pnp_handle h, const float* p, const float* mu, float* q, void* stream);
int pnp_acquire_offres(pnp_handle h, const float* gt, const float* omega, int map_n, const float* dcf, double sigma_n, uint64_t seed, int flags,
                       float* y, float* aty0, float* x0, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PNPADMM_OFFRES_H */
