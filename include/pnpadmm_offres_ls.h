/*
 * pnpadmm_offres_ls.h - extension of the C ABI of libpnpadmm.so (pnpadmm.h): a least-squares temporal interpolator for the off-resonance
 * operator of pnpadmm_offres.h (Sutton, Noll, Fessler, IEEE TMI 2003).  Everything pnpadmm.h says about pointers, streams, status codes and
 * sizes holds here, and everything pnpadmm_offres.h says about omega, t, the maps, the segment blocks and the data-fidelity stage; the
 * entry points live in the same library and take the same handle.
 *
 * WHY.  The linear interpolator of pnp_offres_plan gives exactly two segments per sample, and its error 1 - cos(omega_max D / 2) falls only
 * with the square of the segment count: 32 segments leave 5.1e-3 at omega_max span = 2 pi and 1.2e-2 at 3 pi.  Here the uniform centres
 * tau_l stay where pnp_offres_plan places them, but every sample has a coefficient for EVERY segment, chosen by least squares so that
 *     sum_l b_l(t) exp(-i omega tau_l)   fits   exp(-i omega t)   over the whole band |omega| <= omega_max.
 * For a band that is symmetric about 0 the coefficients are real:
 *     G[l][l'] = sinc(omega_max (tau_l - tau_l')) + ridge [l == l'],   r_l(t) = sinc(omega_max (t - tau_l)),   sinc(x) = sin(x) / x, sinc(0) = 1
 *     b(t) = G^-1 r(t),   ridge = kOffresLsRidge = 1e-10 (a constant of the library, not an argument)
 * G, its Cholesky factor and the two triangular solves per sample are float64 on the host; b is stored as float32, coef [L][M] segment-major.
 * L = 1 is the linear plan's: one centre (t_min + t_max) / 2, coefficient 1, omega_max unused.  Eight segments at omega_max span = 2 pi leave
 * 1.2e-4, ten at 3 pi leave 1.0e-4 (DESIGN.md 4a has the table).
 *
 * THE MODEL.
 *     A p   = [ sum_l b_l(m) F_nu(E_l . p)_m ]_m         E_l as pnp_offres_maps builds them (unchanged)
 *     A^H q = sum_l conj(E_l) . F_nu^H( w . b_l . q )
 * ERROR OF THE MODEL.  |A p - A_exact p|_m <= eps(m, omega) ||p||_1 with eps = |exp(-i omega t_m) - sum_l b_l(m) exp(-i omega tau_l)| at the
 * pixel's omega (on top of the NUFFT's own error).  There is no closed form: eps is evaluated numerically (acquisition.offres_ls_error).
 * The coefficients are not a partition of unity and are not confined to [0, 1]: sum_l |b_l| reaches 14, so float32 rounding enters with
 * that factor.  An omega OUTSIDE THE BAND is not detected by the library: the fit says nothing there and the error grows quickly.  A band
 * that is not centred on 0 (complex coefficients) is OUT OF SCOPE - the caller demodulates - and so are map-specific (histogram-weighted)
 * fits, non-uniform centres, coils times segments, a Toeplitz form, and more than PNP_MC_MAX_COILS segments.
 *
 * EXPRESSION ORDER.  float32 throughout; every operation named below is ONE IEEE operation, an fma only where one is written.
 *   forward   o = (b_0 v_0.x, b_0 v_0.y), products rounded; then o = fma(b_l, v_l, o) for l = 1 .. L-1 ascending.
 *             v_l is the gather of grid l by pnp_nufft_forward_mc's two fma chains.
 *             A partial carried from one segment block to the next goes through the output (a float32 stored and reloaded), so THE BITS DO
 *             NOT DEPEND ON THE BLOCK SIZE (PNP_OFFRES_SEG_BLOCK).
 *   adjoint   per segment t = (b_l q.x, b_l q.y) rounded first, then pnp_nufft_adjoint's ((t w) wy) * wx chain
 *             over ALL samples of the tile's bin, ascending, from +0; the crop and the combine chain over ascending l are unchanged.
 * So with L = 1 the operator pair has the bits of the linear plan's pair.
 * THE NAIVE FORM.  The gather and the gridding exist twice, as in pnpadmm_offres.h.  Naive: the non-Cartesian SENSE launches on all planes
 * of the block between a dense blend and a dense expansion.  Dense: a gather that walks the block's grids with the sample's footprint
 * loaded once and the blend in registers, and a gridding whose workgroup of (tile, slice) stages a chunk of the tile's bin once for up to 8
 * segments, keeps 8 accumulators per thread, and lets a wave pass over a sample that touches none of its rows.  A skipped sample and one
 * that adds 0 . wx leave the same number, so both forms agree as numbers (torch.equal).  Which one a step runs is decided by measurement
 * (the naive gather; the dense gridding on blocks of a multiple of 8 segments, the naive one elsewhere);
 * PNP_OFFRES_LS_NAIVE=1 / 0, read at pnp_create, selects the naive / the dense form of both steps everywhere: the check and the timing
 * baseline.  PNP_OFFRES_LS_NOSKIP=1 runs the dense gridding without the row test (timing).  No atomics, no cross-workgroup waits; a slice's
 * outputs depend on (the plans, its inputs, its map) only and are bitwise reproducible.
 *
 *   t         : HOST float64 [M], M = pnp_nufft_samples; finite;   segments : 1..PNP_MC_MAX_COILS;   flags : reserved, must be 0
 *   omega_max : rad/s, finite and > 0 when segments > 1
 *   coef_host : HOST float32 [L][M]
 *
 * pnp_offres_plan_ls follows the rules of pnp_offres_plan: it needs the plan of pnp_nufft_plan (PNP_ERR_STATE without one), builds tau and
 * the coefficients on the host and uploads them (synchronous), replaces any earlier off-resonance plan of either kind and drops a live
 * off-resonance stage with it.  pnp_nufft_plan drops it as it drops the linear plan; pnp_offres_plan replaces it.  It refuses (PNP_ERR_INVALID,
 * before any HIP call, the handle as it was): a time that is not finite, a zero span with L > 1, omega_max not finite or <= 0 with L > 1,
 * and a Cholesky pivot that is not positive - the failure is reported, never a NaN coefficient.
 * Every entry point of pnpadmm_offres.h then runs on whichever plan is live, with unchanged signatures: pnp_offres_maps, _forward, _adjoint,
 * pnp_set_kspace_offres, pnp_reset_offres, pnp_offres_normal, _cg_residual, pnp_acquire_offres, pnp_offres_segments, pnp_offres_live.
 * pnp_offres_interpolator: 0 without an off-resonance plan (and on NULL), 1 linear, 2 least squares.
 * pnp_offres_ls_coeffs copies the plan's table back (synchronous): the model a caller checks against is built from the device's own
 * coefficients.  PNP_ERR_STATE without a least-squares plan.
 */
#ifndef PNPADMM_OFFRES_LS_H
#define PNPADMM_OFFRES_LS_H

#include "pnpadmm.h"

#ifdef __cplusplus
extern "C" {
#endif

int pnp_offres_plan_ls(pnp_handle h, const double* t, int segments, double omega_max, int flags);
/* 0: no off-resonance plan (and on NULL); 1: the linear interpolator of pnp_offres_plan; 2: least squares. */
int pnp_offres_interpolator(pnp_handle h);
int pnp_offres_ls_coeffs(pnp_handle h, float* coef_host);

#ifdef __cplusplus
}
#endif
#endif /* PNPADMM_OFFRES_LS_H */
