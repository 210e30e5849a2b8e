/*
 * pnpadmm_ncsense.h - extension of the C ABI of libpnpadmm.so (pnpadmm.h): non-Cartesian SENSE, the multi-coil data-fidelity stage on an
 * arbitrary trajectory (iterative SENSE, Pruessmann 2001).  Everything pnpadmm.h says about pointers, streams, status codes and sizes holds
 * here; the entry points live in the same library and take the same handle.
 *
 * pnpadmm.h has two data-fidelity stages beside the reference's single-coil one: the multi-coil stage, on Cartesian masks only, and the
 * non-Cartesian stage, single-coil only.  This header joins them.  One trajectory is shared by all slices of a handle: the plan of
 * pnp_nufft_plan, which every entry point here needs (PNP_ERR_STATE without one).
 *
 * THE OPERATOR.  S_c are C coil sensitivity maps, w optional sample weights (NULL = 1; e.g. density compensation), F_nu / F_nu^H the NUFFT
 * pair exactly as pnp_nufft_forward / pnp_nufft_adjoint implement it - the same plan, float32 weights, factors cy cx and grid transform:
 *     A p    = [ F_nu(S_c . p) ]_c
 *     A^H q  = sum_c conj(S_c) . F_nu^H(w . q_c)
 *     Nop(p) = A^H W A p + mu_n p
 * EXPRESSION ORDER.  float32 throughout; every operation named below is ONE IEEE operation, an fma only where one is written.
 *   coil image   t = (sx px - sy py, sx py + sy px): each product rounded, then the sum; for a real image g, t = (sx g, sy g).  Then
 *                (t.x f, t.y f) with f = cy[iy] * cx[ix] (the rounded product), zero-padded and centred into the grid: pnp_nufft_forward's
 *                first step applied to t.
 *   transform, gather, gridding   pnpadmm.h's text, per coil plane: the gather is the two ascending fma chains, a grid point's value is one
 *                fma chain from +0 over ascending sample index of ((y w) wy) * wx with the inner products rounded first.  No atomics.
 *   crop and combine   a_c = (g.x f, g.y f) of coil c's cropped grid g; then from +0 over ascending c
 *                acc.x = fma(sx, a.x, acc.x);  acc.x = fma(sy, a.y, acc.x);  acc.y = fma(sx, a.y, acc.y);  acc.y = fma(-sy, a.x, acc.y)
 *   Nop's epilogue   q = (fma(mu, p.x, acc.x), fma(mu, p.y, acc.y)); the partial sums of Re<p, q> are float64 sums over the pixel ranges
 *                and the fixed tree of the non-Cartesian stage.
 * So pnp_nufft_forward_mc(img, S)[n, c] has the bits of pnp_nufft_forward on the coil image formed as above, and with maps that have one
 * non-zero coil per pixel, of a value v that is a power of two, pnp_nufft_adjoint_mc gives v times pnp_nufft_adjoint of that coil's samples
 * (the sign of a zero aside).  There is NO promise of bit equality with pnp_nc_normal, not even for C = 1 and S = 1: the single-coil
 * stage leaves its "+ mu p" to the compiler's contraction, this one writes the fma.
 * COIL BLOCKS.  The coil planes are processed in blocks of CB = min(C, 8) coils: workspace 8 N CB gh gw (grids) + 8 N CB M (samples) bytes on
 * top of the plan's and the CG's.  The combine chain continues from block to block through q - a float32 partial stored and reloaded is the
 * same float32 - so THE BITS DO NOT DEPEND ON CB.  The environment variable PNP_NCSENSE_COIL_BLOCK=k (1..32), read at pnp_create, overrides
 * the 8: a check and a timing knob, not a mode.
 * THE NAIVE FORM.  Each of the four steps - pad, gather, gridding, crop and combine - exists twice: as a coil-batched kernel that loads what
 * the block's coils share once, and as the single-coil launch of pnp_nufft_forward / pnp_nufft_adjoint at batch N CB (with an expand kernel
 * before the pad and a combine kernel after the crop, and 8 N CB H W more bytes for the coil images).  Both give the same bits.  Which one
 * a step runs is decided by measurement, not by the caller: a coil-batched kernel ships only where it is not slower (the pad
 * and the crop-and-combine are coil-batched, the gather and the gridding are the single-coil launches).  PNP_NCSENSE_NAIVE=1 / 0, read at
 * pnp_create, selects the naive / the coil-batched form of EVERY step: the bit-for-bit check and the timing baseline, as PNP_TV_NAIVE is of
 * the fused TV kernel.
 * A slice's outputs depend on (the plan, its inputs, its maps) only: not on N, its place in the batch, the stream, or whether the maps are
 * shared (sens_n == 1) or given per slice with the same values; bitwise reproducible.
 *
 *   sens : DEVICE complex64 [C,H,W] (sens_n == 1, shared by all slices) or [N,C,H,W] (sens_n == N, N the handle's n; slice n of a shorter
 *          batch reads maps n);   coils : 1..PNP_MC_MAX_COILS;   cg_iters : 1..PNP_MC_MAX_CG;   n * min(coils, CB) <= 65535
 *
 * pnp_nufft_forward_mc / pnp_nufft_adjoint_mc: img DEVICE complex64 [batch,H,W], samples DEVICE complex64 [batch,C,M], weights DEVICE float32
 * [M] or NULL; 1 <= batch <= n; no input may alias an output.  They read the caller's sens directly.
 *
 * DATA FIDELITY.  pnp_set_kspace_ncsense / pnp_reset_ncsense copy y (complex64 [N,C,M]), w (float32 [M] or NULL) and the maps, form
 * aty = A^H W y once, and put the handle in non-Cartesian SENSE mode by the rule of pnpadmm.h: the stage that runs is the one whose constants
 * were installed LAST.  pnp_step and pnp_prox_dual then run the multi-coil section's CG, word for word, on Nop and b = aty + mu (x + u):
 * K = cg_iters fixed iterations warm-started from z, float64 scalars on the device, a frozen slice never NaN, stopped slices (t_action > 0.5)
 * keep z, u and the CG residual bit for bit (only Nop's last launch skips them; the others rewrite scratch alone), u <- u + x - z.
 * pnp_reset_ncsense also sets the iterate: x = Re(x0), z = x0, u = 0.  In this mode
 *   - pnp_ncsense_coils is C; pnp_mc_coils is 0; pnp_mc_cg_residual, pnp_mc_normal, pnp_nc_cg_residual and pnp_nc_normal give PNP_ERR_STATE;
 *   - pnp_residuals' PNP_RES_DC column is sqrt(sum_c sum_m w_m |(A x)_{c,m} - y_{c,m}|^2): float32 differences, squared, weighted and summed
 *     in float64, the partial sums added in a fixed (coil, chunk) order;
 *   - snapshots, priors and drivers work unchanged;
 *   - pnp_nufft_plan drops these constants exactly as it drops single-coil non-Cartesian ones, and pnp_set_kspace* / pnp_reset* of the other
 *     modes leave this mode.
 * SETUP-TIME SEMANTICS of pnp_set_kspace_mc: the installers allocate or grow the handle's workspace inside the call (the blocks above, y:
 * 8 N C M, w: 4 M, the maps: 8 sens_n C H W, the misfit's partial sums 8 N C ceil(M / 2048), and the coil workspace's coil-independent part:
 * four vectors 8 N H W each, partial sums and scalars), all-or-nothing through the handle's workspace and counted by pnp_workspace_bytes; a
 * call that does not need to grow it is asynchronous.  The handle changes mode only after every launch of the install was accepted: a call
 * that fails leaves the mode and the iterate as they were.
 * pnp_ncsense_normal (q = Nop(p); p, q DEVICE complex64 [N,1,H,W], must not alias; mu DEVICE float32 [N]) and pnp_ncsense_cg_residual (out
 * DEVICE float32 [N]) are the counterparts of pnp_mc_normal and pnp_mc_cg_residual: PNP_ERR_STATE on a handle that is not in this mode.
 *
 * pnp_acquire_ncsense: pnp_acquire_mc for the planned trajectory,  y_c = F_nu(S_c gt) + sigma_n (g_re + i g_im),  aty0 = A^H (dcf . y),
 * x0 = max(aty0, 0) on both planes;  gt DEVICE float32 [N,1,H,W], dcf DEVICE float32 [M] or NULL, y DEVICE complex64 [N,C,M], aty0, x0
 * complex64 [N,1,H,W] or NULL.  Noise: pnp_acquire's counter hash with p = m, the streams 9001 + 4 c (real) and 9003 + 4 c (imaginary) for
 * coil c and seed + n for slice n - pnp_acquire_mc's and pnp_acquire_nc's conventions combined.  With sigma_n == 0 nothing is drawn and y
 * equals pnp_nufft_forward_mc of the real image as numbers (a complex image's zero imaginary part can flip the sign of a zero product, never a
 * value); with C = 1 and S = 1 the outputs equal pnp_acquire_nc's as numbers.  flags : reserved,
 * must be 0.
 *
 * pnp_nufft_forward_mc, pnp_nufft_adjoint_mc and pnp_acquire_ncsense change neither the handle's mode nor any installed constants (a live
 * Cartesian multi-coil episode's maps included); they use, and may grow, the coil-block scratch: calls on one handle are stream-ordered.
 * Every entry point takes any handle kind, and reports every argument error (NULLs, a count out of range, sens_n not 1 or N, flags != 0,
 * forbidden aliasing, no plan, sigma_n negative or not finite) before any HIP call, leaving the outputs untouched.
 *
 * (The entry points are declared here and not in pnpadmm.h so that the tables that mirror that header stay as they are; the two headers
 * may be folded together later.)
 */
#ifndef PNPADMM_NCSENSE_H
#define PNPADMM_NCSENSE_H

#include "pnpadmm.h"

#ifdef __cplusplus
extern "C" {
#endif

int pnp_nufft_forward_mc(pnp_handle h, const float* img, const float* sens, int coils, int sens_n, int batch, float* samples, void* stream);
int pnp_nufft_adjoint_mc(pnp_handle h, const float* samples, const float* weights, const float* sens, int coils, int sens_n, int batch,
                         float* img, void* stream);
int pnp_set_kspace_ncsense(pnp_handle h, const float* y, const float* sens, int coils, int sens_n, const float* w, int cg_iters, void* stream);
int pnp_reset_ncsense(pnp_handle h, const float* x0, const float* y, const float* sens, int coils, int sens_n, const float* w, int cg_iters,
                      float* x, float* z, float* u, void* stream);
/* Coils of the installed non-Cartesian SENSE constants; 0 unless this mode is live (and on NULL). */
int pnp_ncsense_coils(pnp_handle h);
int pnp_ncsense_cg_residual(pnp_handle h, float* out, void* stream);
int pnp_ncsense_normal(pnp_handle h, const float* p, const float* mu, float* q, void* stream);
int pnp_acquire_ncsense(pnp_handle h, const float* gt, const float* sens, int coils, int sens_n, const float* dcf, double sigma_n, uint64_t seed,
                        int flags, float* y, float* aty0, float* x0, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PNPADMM_NCSENSE_H */
