/*
 * pnpadmm_offres_tz.h - extension of the C ABI of libpnpadmm.so (pnpadmm.h): the Toeplitz form of the normal operator A^H W A of the two
 * off-resonance CG stages, single-coil (pnpadmm_offres.h, pnpadmm_offres_ls.h) and multi-coil (pnpadmm_offres_mc.h).  Everything pnpadmm.h
 * says about pointers, streams, status codes and sizes holds here; the entry points live in the same library and take the same handle.
 *
 * THE MODEL.  Let F be the exact non-uniform DFT of the planned trajectory, as in pnpadmm_toeplitz.h, and b_l(m) the float32 coefficients the
 * live off-resonance plan stores - linear (pnp_offres_plan: b0_m at l = seg_m, b1_m at l = seg_m + 1, 0 elsewhere) or least squares
 * (pnp_offres_plan_ls: coef[l][m]).  The segmented model
 *     A = sum_l diag(b_l) F diag(E_l),   E_l = exp(-i omega tau_l)
 * has a normal operator that is a sum of Toeplitz blocks between phase maps:
 *     A^H W A p = sum_l conj(E_l) . sum_l' Toep[u_ll'] (E_l' . p),     u_ll'(m) = w_m b_l(m) b_l'(m)
 *     K_ll'[j, k] = (1 / (H W)) sum_m u_ll'(m) D_H(ky_m - (j - H) / 2H) D_W(kx_m - (k - W) / 2W)
 * with the Dirichlet kernel D_n of pnpadmm_toeplitz.h.  Every K_ll' is real and K_ll' = K_l'l, so P spectra are stored: the upper triangle,
 * P = L (L + 1) / 2, under a least-squares plan; the band |l - l'| <= 1, P = 2 L - 1, under a linear plan, where every other u_ll' vanishes.
 * On the 2H x 2W grid
 *     X_l' = fft2c(pad(E_l' . p)),    Y_l = sum_l' K_ll' . X_l',    q = sum_l conj(E_l) . crop(ifft2c(Y_l)) (+ mu p)
 * which is 2 L transforms and one spectral mix per slice, whatever M and the NUFFT's width J, and exact for the model that the plan's
 * stored coefficients define (the gridding pair of pnpadmm_offres.h is a 1e-5 .. 9e-4 model of the same operator).
 *
 * EXPRESSION ORDER.
 *   spectra   per pair and sample u = ((double)w_m * (double)b_l) * (double)b_l', each product rounded (w == NULL: the double 1.0); then
 *             u * D_H; then one fma per output with D_W, over ascending m from 0 - no partial sums, no atomics; then the division by H W and
 *             ONE rounding to float32.  Under a linear plan a pair's chain runs over the samples of its two segments only; a sample that is
 *             skipped and a sample that adds 0 . D leave the same number.  The bits depend on (trajectory, times plan, weights, H, W) only,
 *             and with L = 1 pnp_offres_tz_spectrum has the bits of pnp_toeplitz_spectrum for the same weights.
 *   apply     E_l . p is pnpadmm_ncsense.h's complex product (four products rounded, then the difference and the sum) with E_l in the place
 *             of a coil map; pad and the transforms are pnpadmm_toeplitz.h's; the mix is, per bin and output segment l, two fma chains from
 *             +0 (real and imaginary) over ascending l' - inside the band under a linear plan -, then one multiplication by the form's scale
 *             (1 composed, the power of two 1 / (4 H W) fused); the combine chain over ascending l is pnpadmm_ncsense.h's four fmas per
 *             segment from +0 with E_l in the place of S_c, and the epilogue q = (fma(mu, p.x, acc.x), fma(mu, p.y, acc.y)) with the partial
 *             sums of Re<p, q> is that header's, so the CG of pnpadmm.h runs on it unchanged.
 * TWO FORMS.  Composed: expand, pad, rows, columns, mix, columns, rows, crop, combine on full [planes, 2H, 2W] pass buffers.  Fused
 * (power-of-two padded sides: H, W in {16, 32, 64, 128, 256, 512}): pnpadmm_toeplitz.h's fused forward row pass writes the H live rows into
 * [planes, H, 2W]; a forward column pass zero-fills to 2H in LDS and stores the whole column spectrum; the mix; an inverse column pass
 * stores only the H cropped rows; the fused inverse row pass; the combine.  The grid's zero half is written by nobody before the column
 * pass and read by nobody after it.  A handle with a side of 80, 160, 320 or 400 runs the composed form, and PNP_OFFRES_TZ_NAIVE=1, read
 * at pnp_create, selects it everywhere: the timing baseline and a cross-check.  The two forms need NOT agree bit for bit; each is held to
 * float64, and within a form a slice's bits depend on (the spectra, its input, its maps) only: not on the batch, the slice block, the
 * stream, the coil block or whether the maps are shared.
 * SLICE BLOCKS.  All L planes of a slice are in flight for the mix.  Slices go through the pass buffers in blocks of
 * max(1, PNP_OFFRES_TZ_PLANES / L) slices; PNP_OFFRES_TZ_SLICE_BLOCK=k, read at pnp_create, overrides the block as a check.
 * MULTI-COIL.   Nop(p) = sum_c conj(S_c) . [the above](S_c . p) + mu p: per coil block the expand kernel of pnpadmm_ncsense.h, the
 * single-coil application at batch N CB without epilogue, and the SENSE combine with the epilogue.  CB is the coil block of
 * pnpadmm_offres_mc.h (PNP_OFFRES_MC_COIL_BLOCK) while the segment maps are shared (map_n == 1); with per-slice maps the coils go one at
 * a time.  THE BITS DO NOT DEPEND ON CB.
 * SIZES AND LIMITS.  Sides as in pnpadmm_toeplitz.h: H, W in {16, 32, 64, 80, 128, 160, 256, 320, 400, 512}; a larger side is refused
 * with that header's words.  P <= PNP_OFFRES_TZ_MAX_PAIRS = 136: up to 16 segments under a least-squares plan, up to 32 under a linear
 * one; more is PNP_ERR_INVALID with a message that names the limit, before any HIP call.
 *
 * pnp_offres_tz_plan builds the P spectra for the handle's NUFFT plan and whichever off-resonance plan is live (PNP_ERR_STATE without
 * either) and these weights (DEVICE float32 [M], or NULL = 1), and keeps a copy of the weights.  flags : reserved, must be 0.  SETUP-TIME
 * SEMANTICS of pnp_set_kspace_mc: it allocates inside the call - the spectra: 16 P H W bytes, the weights copy: 4 M (none for NULL), a
 * device copy of the trajectory: 16 M, under a linear plan the per-pair sample lists (at most 8 M), the twiddles of the two sides, and
 * the pass buffers of a slice block (two of 32 H W bytes per plane, one of 8 H W) - all-or-nothing through the handle's workspace and
 * counted by pnp_workspace_bytes, and it returns after the spectra are built.  It replaces earlier spectra; if a Toeplitz off-resonance
 * stage is live, that stage's constants are dropped with them.  pnp_nufft_plan, pnp_offres_plan and pnp_offres_plan_ls drop the spectra.
 * pnp_toeplitz_plan, pnp_toeplitz_planned and pnp_toeplitz_live know nothing of this header: pnp_toeplitz_live stays 0 here, and
 * pnp_toeplitz_plan does not drop a stage installed from here.
 * pnp_offres_tz_planned: 1 if spectra exist, else 0.  pnp_offres_tz_live: 1 if the live stage's CG runs this operator, else 0.
 * pnp_offres_tz_spectra: P, or 0 without a plan.  (All three: 0 on NULL.)
 * pnp_offres_tz_spectrum copies the spectra to out, DEVICE float32 [P, 2H, 2W], each centred like pnp_fft2c's output.  THE PAIR ORDER:
 * least squares - the upper triangle row by row, (0,0) (0,1) .. (0,L-1) (1,1) ..; linear - (l, l) and (l, l+1) interleaved,
 * (0,0) (0,1) (1,1) (1,2) .. (L-1,L-1).
 *
 * pnp_offres_tz_apply / pnp_offres_tz_apply_mc: out = A^H W A img, without mu, on the caller's segment maps (maps: DEVICE complex64
 * [map_n, L, H, W], pnp_offres_maps' output or any maps of that shape; map_n 1 or N) and, _mc, coil maps (sens: DEVICE complex64
 * [sens_n, C, H, W], sens_n 1 or N, coils 1..PNP_MC_MAX_COILS).  img, out DEVICE complex64 [batch, H, W], 1 <= batch <= n; out must not
 * alias an input.  Neither changes the mode or any installed constants; they use, and _mc may grow, the handle's scratch: calls on one
 * handle are stream-ordered.
 *
 * THE INSTALLERS.  pnp_set_kspace_offres_tz, pnp_reset_offres_tz, pnp_set_kspace_offres_mc_tz and pnp_reset_offres_mc_tz take no weights:
 * the weights of the spectra are the weights of aty and of the DC column, so the operator and the right-hand side cannot disagree.  They
 * need spectra (PNP_ERR_STATE without); otherwise they do what pnp_set_kspace_offres, pnp_reset_offres, pnp_set_kspace_offres_mc and
 * pnp_reset_offres_mc do, through the same install code, and then mark the stage.  "The stage installed last runs" extends: every other
 * installer leaves this mode.  While such a stage is live pnp_step and pnp_prox_dual run the unchanged CG on this operator, and
 * pnp_offres_normal and pnp_offres_cg_residual, or pnp_offres_mc_normal and pnp_offres_mc_cg_residual, report the live stage's operator;
 * pnp_offres_live, or pnp_offres_mc_coils, stay what they are for the gridding stage.  aty, the PNP_RES_DC column and the acquisitions
 * stay on the gridding pair; snapshots, priors, residuals and drivers are unchanged.  A failed install leaves the mode and the iterate as
 * they were.
 *
 * Every entry point takes any handle kind, and reports every argument error (NULLs, a count out of range, sens_n or map_n not 1 or N,
 * flags != 0, forbidden aliasing, no plan, no spectra, a side above 512, P above the limit) before any HIP call,
 * leaving the outputs untouched.
 */
#ifndef PNPADMM_OFFRES_TZ_H
#define PNPADMM_OFFRES_TZ_H

#include "pnpadmm.h"

#define PNP_OFFRES_TZ_MAX_PAIRS 136
#define PNP_OFFRES_TZ_PLANES 512

#ifdef __cplusplus
extern "C" {
#endif

int pnp_offres_tz_plan(pnp_handle h, const float* weights, int flags, void* stream);
int pnp_offres_tz_planned(pnp_handle h);
int pnp_offres_tz_live(pnp_handle h);
int pnp_offres_tz_spectra(pnp_handle h);
int pnp_offres_tz_spectrum(pnp_handle h, float* out, void* stream);
int pnp_offres_tz_apply(pnp_handle h, const float* img, const float* maps, int map_n, int batch, float* out, void* stream);
int pnp_offres_tz_apply_mc(pnp_handle h, const float* img, const float* maps, int map_n, const float* sens, int sens_n, int coils, int batch,
                           float* out, void* stream);
int pnp_set_kspace_offres_tz(pnp_handle h, const float* y, const float* omega, int map_n, int cg_iters, void* stream);
int pnp_reset_offres_tz(pnp_handle h, const float* x0, const float* y, const float* omega, int map_n, int cg_iters, float* x, float* z, float* u,
                        void* stream);
int pnp_set_kspace_offres_mc_tz(pnp_handle h, const float* y, const float* sens, int coils, int sens_n, const float* omega, int map_n, int cg_iters,
                                void* stream);
int pnp_reset_offres_mc_tz(pnp_handle h, const float* x0, const float* y, const float* sens, int coils, int sens_n, const float* omega, int map_n,
                           int cg_iters, float* x, float* z, float* u, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PNPADMM_OFFRES_TZ_H */
