/*
 * pnpadmm_offres_mc.h - extension of the C ABI of libpnpadmm.so (pnpadmm.h): off-resonance correction for MULTI-COIL non-Cartesian data.
 * It joins the non-Cartesian SENSE operator of pnpadmm_ncsense.h (coil maps S_c) and the time-segmented operator of pnpadmm_offres.h /
 * pnpadmm_offres_ls.h (segment maps E_l, temporal interpolator b_l) into one operator pair and one CG data-fidelity stage: coils times
 * segments.  Everything pnpadmm.h says about pointers, streams, status codes and sizes holds here; the entry points live in the same
 * library and take the same handle.
 *
 * THE MODEL.  With the plan of pnp_nufft_plan and WHICHEVER off-resonance plan is live - linear (pnp_offres_plan: b_l(m) is b0_m at
 * l = seg_m, b1_m at l = seg_m + 1, 0 elsewhere) or least squares (pnp_offres_plan_ls: b_l(m) = coef[l][m]) -
 *     (A p)_{c,m} = sum_l b_l(m) F_nu(E_l . S_c . p)_m
 *     A^H q       = sum_c conj(S_c) . sum_l conj(E_l) . F_nu^H(w . b_l . q_c)
 *     Nop(p)      = A^H W A p + mu_n p
 * A coil plane of A p is the single-coil operator of pnpadmm_offres.h on the image S_c . p, and the inner sum of A^H is its adjoint on coil
 * c's samples; the error of the model is that header's, per coil.  PNP_ERR_STATE without an off-resonance plan.
 *
 * EXPRESSION ORDER.  float32 throughout; every operation named below is ONE IEEE operation, an fma only where one is written.
 *   forward   u = S_c . p, then v = E_l . u, each as pnpadmm_ncsense.h writes a complex product (four products rounded, then the difference
 *             and the sum; for the real x of pnp_step u = (S.x x, S.y x)); then (cy cx) . v with the factor formed first; zeros outside
 *             the window; the transform, the gather and the blend over l are pnp_offres_forward's, word for word
 *   adjoint   per coil the gridding, the transform and the combine chain a_c = sum over ascending l of conj(E_l) . ((cy cx) . crop(grid)),
 *             four fmas per segment from +0, are pnp_offres_adjoint's; then q = sum over ascending c of conj(S_c) . a_c, the four fmas of
 *             pnp_nufft_adjoint_mc's combine chain from +0; the normal operator then adds fma(mu, p, q) per plane
 * So coil plane c of pnp_offres_forward_mc has the bits of pnp_offres_forward on the image S_c . p (rounded as above), a_c has the bits of
 * pnp_offres_adjoint on coil c's samples, and with C = 1, S = 1 both entry points have the bits of the single-coil pair.
 * BLOCKS.  A block of CBc coils x SB segments of every slice is in flight at a time: grids [N, CBc, SB, gh, gw] in the coil-block scratch
 * of pnpadmm_ncsense.h, grown to 8 N CBc SB gh gw bytes of grids and 8 N CBc SB M bytes of samples, plus 8 N CBc M bytes for a coil
 * block's samples and, only when L > SB, 8 N CBc H W bytes for the segment chain's partials.  SB is the segment block of pnpadmm_offres.h (min(L, 8),
 * PNP_OFFRES_SEG_BLOCK); CBc = min(C, 4) under a least-squares plan and min(C, 2) under a linear one (the blocks that measured fastest,
 * DESIGN.md 4a), and the environment variable PNP_OFFRES_MC_COIL_BLOCK=k (1..32), read at pnp_create, overrides both: a check and a
 * timing knob, not a mode.  Coil blocks are the outer loop, segment blocks the inner one: a sample's blend continues
 * through the output across segment blocks, the segment chain through the partials, the coil chain through q - a float32 partial stored
 * and reloaded is the same float32 - so NO BIT DEPENDS ON SB OR CBc.   n * CBc * SB <= 65535.
 * THE COMPOSED FORM.  PNP_OFFRES_MC_NAIVE=1, read at pnp_create, runs what a caller of the other headers would write: per coil the image
 * S_c . p, the single-coil forward at batch N and a strided copy; in the other direction the single-coil adjoint per coil and the SENSE
 * combine.  PNP_OFFRES_MC_NAIVE=0 runs the fused pad and crop kernels, which never form a coil image [N, C, H, W]; both forms agree bit
 * for bit.  Which one a step runs by default is decided by measurement.  No atomics, no cross-workgroup waits.
 * A slice's outputs depend on (the plans, its inputs, its maps) only: not on N, its place in the batch, the stream, or whether the maps
 * are shared or given per slice with the same values; bitwise reproducible.
 *
 *   coils    : 1..PNP_MC_MAX_COILS;   sens_n, map_n : 1 (shared by all slices) or N (the handle's n), independently
 *   sens     : DEVICE complex64 [sens_n,C,H,W]
 *   maps     : DEVICE complex64 [map_n,L,H,W]: pnp_offres_maps' output, or any maps of that shape
 *   omega    : DEVICE float32 [map_n,H,W] rad/s
 *   y, samples : DEVICE complex64 [batch,C,M] (batch = N for the installers);   w, weights, dcf : DEVICE float32 [M] or NULL
 *   img      : DEVICE complex64 [batch,H,W];   1 <= batch <= n;   no input may alias an output
 *
 * DATA FIDELITY.  pnp_set_kspace_offres_mc / pnp_reset_offres_mc copy y, w and the coil maps, build the segment maps of omega into the
 * handle's workspace, form aty = A^H W y once, and make this stage the live one by the rule of pnpadmm.h: the stage that runs is the one
 * whose constants were installed LAST.  pnp_step and pnp_prox_dual then run the multi-coil section's CG on Nop and b = aty + mu (x + u)
 * (cg_iters : 1..PNP_MC_MAX_CG; stopped slices keep z, u and the CG residual bit for bit).  pnp_reset_offres_mc also sets the iterate:
 * x = Re(x0), z = x0, u = 0.  While this stage is live
 *   - pnp_offres_mc_coils is C; pnp_offres_live, pnp_ncsense_coils and pnp_mc_coils are 0;
 *   - pnp_{mc,nc,ncsense,offres}_cg_residual and pnp_{mc,nc,ncsense,offres}_normal give PNP_ERR_STATE;
 *   - pnp_residuals' PNP_RES_DC column is sqrt(sum_c sum_m w_m |(A x)_{c,m} - y_{c,m}|^2), summed as the non-Cartesian SENSE stage sums it;
 *   - snapshots, priors and drivers work unchanged; the installers of the other modes leave this mode; pnp_nufft_plan, pnp_offres_plan and
 *     pnp_offres_plan_ls drop it with the plan it was built on.
 * The installers allocate or grow the handle's workspace inside the call (the block scratch above, y: 8 N C M, w: 4 M, the coil maps:
 * 8 sens_n C H W, the segment maps: 8 map_n L H W, the misfit's partial sums, and the CG's vectors), all-or-nothing and counted by
 * pnp_workspace_bytes.  The handle changes mode only after every launch of the install was accepted: a call that fails leaves the mode and
 * the iterate as they were.
 * pnp_offres_mc_normal (q = Nop(p); p, q DEVICE complex64 [N,1,H,W], must not alias; mu DEVICE float32 [N]) and pnp_offres_mc_cg_residual
 * (out DEVICE float32 [N]) give PNP_ERR_STATE on a handle that is not in this mode.
 *
 * pnp_acquire_offres_mc: pnp_acquire_ncsense under the segmented operator,  y = A gt + sigma_n (g_re + i g_im) with that header's per-coil
 * noise streams,  aty0 = A^H (dcf . y),  x0 = max(aty0, 0) on both planes; gt DEVICE float32 [N,1,H,W], y DEVICE complex64 [N,C,M], aty0, x0
 * complex64 [N,1,H,W] or NULL; flags reserved, must be 0.  Its segment maps live in a workspace buffer of its own (8 map_n L H W bytes), so
 * it disturbs no live episode.
 *
 * pnp_offres_forward_mc, pnp_offres_adjoint_mc and pnp_acquire_offres_mc change neither the handle's mode nor any installed constants; they
 * use, and may grow, the block scratch: calls on one handle are stream-ordered.  Every entry point reports every argument error (NULLs, a
 * count out of range, sens_n or map_n not 1 or N, flags != 0, forbidden aliasing, no plan, sigma_n negative or not finite) before any HIP
 * call, leaving the outputs untouched.
 */
#ifndef PNPADMM_OFFRES_MC_H
#define PNPADMM_OFFRES_MC_H

#include "pnpadmm.h"

#ifdef __cplusplus
extern "C" {
#endif

int pnp_offres_forward_mc(pnp_handle h, const float* img, const float* maps, int map_n, const float* sens, int sens_n, int coils, int batch,
                          float* samples, void* stream);
int pnp_offres_adjoint_mc(pnp_handle h, const float* samples, const float* weights, const float* maps, int map_n, const float* sens, int sens_n,
                          int coils, int batch, float* img, void* stream);
int pnp_set_kspace_offres_mc(pnp_handle h, const float* y, const float* sens, int coils, int sens_n, const float* omega, int map_n, const float* w,
                             int cg_iters, void* stream);
int pnp_reset_offres_mc(pnp_handle h, const float* x0, const float* y, const float* sens, int coils, int sens_n, const float* omega, int map_n,
                        const float* w, int cg_iters, float* x, float* z, float* u, void* stream);
/* Coils of the installed constants while this stage is the live one; 0 otherwise (and on NULL). */
int pnp_offres_mc_coils(pnp_handle h);
int pnp_offres_mc_cg_residual(pnp_handle h, float* out, void* stream);
int pnp_offres_mc_normal(pnp_handle h, const float* p, const float* mu, float* q, void* stream);
int pnp_acquire_offres_mc(pnp_handle h, const float* gt, const float* sens, int coils, int sens_n, const float* omega, int map_n, const float* dcf,
                          double sigma_n, uint64_t seed, int flags, float* y, float* aty0, float* x0, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PNPADMM_OFFRES_MC_H */
