/*
 * pnpadmm_toeplitz.h - extension of the C ABI of libpnpadmm.so (pnpadmm.h, pnpadmm_ncsense.h): the Toeplitz form of the normal operator
 * A^H W A of the two non-Cartesian CG stages.  Everything pnpadmm.h says about pointers, streams, status codes and sizes holds here; the
 * entry points live in the same library and take the same handle.
 *
 * Every CG iteration of the non-Cartesian stages applies A^H W A, and with the exact operator A of a trajectory (ky_m, kx_m), m < M,
 *     (A p)_m = (1 / sqrt(H W)) sum_q p[q] exp(-2 pi i (ky_m qy + kx_m qx)),   qy = iy - H/2, qx = ix - W/2,
 * that operator is a convolution:
 *     (A^H W A p)[q] = sum_q' T[q - q'] p[q'],    T[d] = (1 / (H W)) sum_m w_m exp(2 pi i (ky_m dy + kx_m dx)),  |dy| < H, |dx| < W
 * On a 2H x 2W grid it is two transforms and one pointwise multiply by a real spectrum K that is computed once per (trajectory, weights):
 * the cost of an application depends neither on M nor on the NUFFT's width J, and the Toeplitz form is the EXACT operator where the NUFFT
 * pair is a 1e-5 .. 9e-4 model of it.
 *
 * THE SPECTRUM.  K is float32, real, [2H, 2W], centred like pnp_fft2c's output:
 *     K[j, l] = sum over |dy| < H, |dx| < W of T[d] exp(-2 pi i ((j - H) dy / 2H + (l - W) dx / 2W))
 *             = (1 / (H W)) sum_m w_m D_H(ky_m - (j - H) / 2H) D_W(kx_m - (l - W) / 2W),
 *     D_n(t)  = sum_{d = -(n-1)}^{n-1} exp(2 pi i d t) = sin((2n - 1) pi t) / sin(pi t)    (2n - 1 where t is an integer)
 * The lags dy = -H and dx = -W are never reached by q - q' and are left out; w real makes T Hermitian and K real, so only real values are
 * stored.  K is NOT non-negative (min K / max K is around -0.05 .. -0.3).  The library evaluates the real rank-1 Dirichlet sum in float64:
 * t = k_m - (j - n) / (2n) is reduced to t - rint(t) (a sample at k = +-0.5 against the bin -0.5 gives the integer 1, where the quotient
 * would be garbage) and t == 0 takes the limit 2n - 1; one thread owns a 4 x 4 block of outputs and adds the samples' terms
 * (w_m D_H) D_W in ascending m, from 0, one fma each - no partial sums, no atomics - then divides by H W and rounds to float32 once.
 * Its bits depend on (trajectory, weights, H, W) only: not on N, the stream or the call.  weights == NULL multiplies by the double 1.0,
 * which changes no bit against all-ones weights.
 *
 * THE APPLICATION.   q = crop(ifft2c_{2H,2W}(K . fft2c_{2H,2W}(pad(p))))
 * pad places p in rows H/2 .. 3H/2 - 1 and columns W/2 .. 3W/2 - 1 of the 2H x 2W grid and writes zeros elsewhere; crop takes the same
 * window.  The transforms are the engine's centred orthonormal row and column passes (pnp_fft2c's, rows then columns in both directions)
 * with twiddles for 2W and 2H; the orthonormal pair cancels the scale, so K is the unnormalised spectrum.
 * TWO FORMS.  The composed form is seven launches - pad, rows, columns, multiply by K (two rounded multiplications per grid point), rows,
 * columns, crop - on a [planes, 2H, 2W] pass buffer.  The fused form is three: a row pass that zero-fills to 2W in LDS and transforms the H
 * live rows only; a column pass that loads a strip's H live rows into lines of 2H, transforms, multiplies by K / (4 H W) - the four
 * orthonormal scalings, one exact power of two, ride on K and the transforms store unscaled - transforms back and stores the H cropped
 * rows; and the inverse row pass, which crops to W and carries the epilogue.  Its pass buffer is [planes, H, 2W]: the grid's zero half is
 * never stored.  A handle whose padded sides are both powers of two (H, W in {16, 32, 64, 128, 256, 512}) runs the fused form; a handle
 * with a side of 80, 160, 320 or 400 (the mixed-radix family) runs the composed form.  PNP_TOEPLITZ_NAIVE=1, read at pnp_create, selects
 * the composed form everywhere: the timing baseline and a cross-check.  The two forms reach different line transforms and need NOT agree
 * bit for bit; each is held to the float64 operator, and within one form the promise of bits below holds.
 * SIZES.  2H and 2W must be sides the k-space stage accepts, so H, W in {16, 32, 64, 80, 128, 160, 256, 320, 400, 512}.  A handle with
 * a side of 640, 800 or 1024 is refused with PNP_ERR_INVALID and a message that names the limit, before any HIP call.
 * MULTI-COIL.   Nop(p) = sum_c conj(S_c) . Toep(S_c . p) + mu p.  The coil image t = (sx px - sy py, sx py + sy px), the combine chain -
 * four fmas per coil from +0 in ascending c, continued across coil blocks through q -, the epilogue q = (fma(mu, p.x, acc.x),
 * fma(mu, p.y, acc.y)) and the partial sums are word for word those of pnpadmm_ncsense.h; its expand and combine kernels run them.  Each
 * block of CB = min(C, 8) coils (PNP_NCSENSE_COIL_BLOCK overrides the 8) goes through the expand kernel, the application at batch N CB
 * without epilogue, and the combine kernel: THE BITS DO NOT DEPEND ON CB.
 * SINGLE-COIL EPILOGUE.  q = (fma(mu, p.x, acc.x), fma(mu, p.y, acc.y)) with the partial sums of Re<p, q> over the non-Cartesian stage's
 * pixel ranges and fixed tree, so the CG of pnpadmm.h runs on it unchanged.  Stopped slices (t_action > 0.5) keep z, u and the CG
 * residual bit for bit: only the operator's last launch skips them, the others rewrite scratch alone.
 * A slice's output depends on (the spectrum, its input, its maps) only: not on the batch, its place in it, the stream, the coil block or
 * whether the maps are shared; bitwise reproducible.
 * WHAT STAYS ON THE NUFFT PAIR.  aty = A^H W y, the PNP_RES_DC column of pnp_residuals and the pnp_acquire_* calls.  Only the operator
 * inside the CG changes.
 *
 * pnp_toeplitz_plan builds the spectrum for the handle's NUFFT plan (pnp_nufft_plan; PNP_ERR_STATE without one) and these weights
 * (DEVICE float32 [M], or NULL = 1) and keeps a copy of the weights.  flags : reserved, must be 0.  SETUP-TIME SEMANTICS of
 * pnp_set_kspace_mc: it allocates inside the call - K: 16 H W bytes, the weights copy: 4 M (none for NULL), a device copy of the
 * trajectory: 16 M, the twiddles of the two sides: 16 (H + W), and the pass buffer of the application: 16 N H W (fused) or 32 N H W
 * (composed) - all-or-nothing through the handle's workspace and counted by pnp_workspace_bytes, and it returns after the spectrum is built.
 * A multi-coil application or installer grows the pass buffer to N CB planes and adds the block's coil images, 8 N CB H W, inside the
 * call.  It replaces an earlier spectrum.  pnp_nufft_plan drops the spectrum.  If a Toeplitz stage is live when pnp_toeplitz_plan is called, that stage's constants are
 * dropped: the handle then has no episode constants, exactly as after pnp_nufft_plan.
 * pnp_toeplitz_planned: 1 if a spectrum exists, else 0 (and 0 on NULL).  pnp_toeplitz_live: 1 if the live stage's CG runs the Toeplitz
 * operator, else 0 (and 0 on NULL).  pnp_toeplitz_spectrum copies K to out, DEVICE float32 [2H, 2W].
 *
 * pnp_toeplitz_apply / pnp_toeplitz_apply_mc: out = A^H W A img, without mu.  img, out DEVICE complex64 [batch, H, W], 1 <= batch <= n,
 * must not alias.  _mc reads the caller's maps: sens DEVICE complex64 [C, H, W] (sens_n == 1) or [N, C, H, W] (sens_n == N), coils
 * 1..PNP_MC_MAX_COILS, n * min(coils, CB) <= 65535.  Neither changes the mode or any installed constants; they use, and _mc may grow,
 * the handle's scratch: calls on one handle are stream-ordered.
 *
 * THE INSTALLERS.  pnp_set_kspace_nc_tz, pnp_reset_nc_tz, pnp_set_kspace_ncsense_tz and pnp_reset_ncsense_tz take no weights: the weights
 * of the spectrum are the weights of aty and of the DC column, so the operator and the right-hand side cannot disagree.  They need a
 * spectrum (PNP_ERR_STATE without one); otherwise they do what pnp_set_kspace_nc, pnp_reset_nc, pnp_set_kspace_ncsense and
 * pnp_reset_ncsense do, through the same install code, and then mark the stage Toeplitz.  "The stage installed last runs" extends: every
 * other installer leaves Toeplitz.  With a live Toeplitz stage pnp_step and pnp_prox_dual run the same CG on the Toeplitz Nop;
 * pnp_nc_normal and pnp_nc_cg_residual, or pnp_ncsense_normal and pnp_ncsense_cg_residual, report the live stage's operator; snapshots,
 * priors, residuals and drivers are unchanged.  A failed install leaves the mode and the iterate as they were.
 *
 * Every entry point takes any handle kind, and reports every argument error (NULLs, a count out of range, sens_n not 1 or N, flags != 0,
 * forbidden aliasing, no plan, no spectrum, a side above 512) before any HIP call, leaving the outputs untouched.
 *
 * (The entry points are declared here so that the tables that mirror the two older headers stay as they are.)
 */
#ifndef PNPADMM_TOEPLITZ_H
#define PNPADMM_TOEPLITZ_H

#include "pnpadmm_ncsense.h"

#define PNP_TOEPLITZ_MAX_SIDE 512

#ifdef __cplusplus
extern "C" {
#endif

int pnp_toeplitz_plan(pnp_handle h, const float* weights, int flags, void* stream);
int pnp_toeplitz_planned(pnp_handle h);
int pnp_toeplitz_live(pnp_handle h);
int pnp_toeplitz_spectrum(pnp_handle h, float* out, void* stream);
int pnp_toeplitz_apply(pnp_handle h, const float* img, int batch, float* out, void* stream);
int pnp_toeplitz_apply_mc(pnp_handle h, const float* img, const float* sens, int coils, int sens_n, int batch, float* out, void* stream);
int pnp_set_kspace_nc_tz(pnp_handle h, const float* y, int cg_iters, void* stream);
int pnp_reset_nc_tz(pnp_handle h, const float* x0, const float* y, int cg_iters, float* x, float* z, float* u, void* stream);
int pnp_set_kspace_ncsense_tz(pnp_handle h, const float* y, const float* sens, int coils, int sens_n, int cg_iters, void* stream);
int pnp_reset_ncsense_tz(pnp_handle h, const float* x0, const float* y, const float* sens, int coils, int sens_n, int cg_iters,
                         float* x, float* z, float* u, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PNPADMM_TOEPLITZ_H */
