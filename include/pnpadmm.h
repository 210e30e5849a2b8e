/*
 * pnpadmm.h - C ABI of libpnpadmm.so: the MI355X (gfx950) PnP-ADMM CS-MRI hot path.
 *
 * This is the drop-in boundary for ONE path of joesharratt1229/DT4Image_Restoration:
 * the per-iteration loop of `PnPEnv.step` (evaluation/env.py:74-100) with its plug-in
 * operators `UNetDenoiser2D.forward` (evaluation/noise.py:155-164) and the centred FFT pair
 * (evaluation/utils/transformations.py:6-19).  The reference is pure Python, so "what its FFI
 * would bind" is a flat function per reference method; each entry point below names the
 * reference interface it replaces.  INTEGRATION.md shows the ctypes stub a maintainer adds.
 *
 * Conventions
 *   - every pointer marked DEVICE is HIP device memory owned by the caller (e.g. a torch-ROCm
 *     tensor's data_ptr()); HOST pointers are ordinary memory.  No torch types cross this ABI.
 *     DEVICE pointers are expected 16-byte aligned, as any hipMalloc or torch allocation and any whole-plane
 *     view of one is.
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream) of the
 *     handle's device; no entry point synchronises the device except pnp_create /
 *     pnp_load_unet_weights / pnp_destroy (setup-time).  Entry points switch to the handle's device
 *     for the call and restore the caller's current device before returning.
 *   - no C++ exception crosses this boundary (PNP_ERR_NOMEM / PNP_ERR_INTERNAL instead), and a failed
 *     pnp_load_unet_weights leaves the handle exactly as it was (all-or-nothing).
 *   - tile plans and experiment overrides (PNP_WINO_* environment variables) are fixed per handle at
 *     pnp_create.
 *   - real data is float32; complex data is complex64 = interleaved (re, im) float32, passed as
 *     float*; images are [N,1,H,W] contiguous exactly like the reference's tensors.
 *   - returns PNP_OK (0) or a negative pnp_status; pnp_last_error() gives the message of the last
 *     failure on the calling thread.  A handle is not thread-safe; use one per GPU/process.
 *   - H and W must each be one of 16, 32, 64, 80, 128, 160, 256, 320, 400, 512, 640, 800, 1024 (the
 *     multiples of 16 up to 1024 of the form 2^a * 5^b, mixed freely, e.g. 640 x 320) for the ADMM step /
 *     FFT (the reference is hard-wired to 128, env.py:64); any other size is refused with PNP_ERR_INVALID.
 *     The denoiser alone takes multiples of 16 up to 1024 (noise.py:49-53 pad is then a no-op).
 */
#ifndef PNPADMM_H
#define PNPADMM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pnp_engine* pnp_handle;

typedef enum {
    PNP_OK = 0,
    PNP_ERR_INVALID = -1,      /* bad argument (NULL, shape, size not supported) */
    PNP_ERR_HIP = -2,          /* a HIP runtime call failed; message has hipGetErrorString */
    PNP_ERR_STATE = -3,        /* call order: weights not loaded / reset not done */
    PNP_ERR_NOMEM = -4,        /* host or device allocation failed */
    PNP_ERR_INTERNAL = -5      /* a C++ exception was caught at the ABI boundary (never propagates to the caller) */
} pnp_status;

typedef struct {
    int32_t n;        /* slices resident on this GPU (batch); reference: 1 */
    int32_t h, w;     /* slice size; reference: 128 x 128 */
    int32_t device;   /* HIP device ordinal */
    int32_t flags;    /* PNP_FLAG_* */
} pnp_config;

#define PNP_FLAG_PROFILE 1       /* kernel-class timing with HIP events on the launch stream (pnp_profile_collect): one pair
                                    around the run of conv3x3 launches of a denoiser forward, one per other kernel */
#define PNP_FLAG_PROFILE_LAYERS 16  /* an event pair around EVERY launch (adds pnp_profile_layers; ~0.2 ms per step) */
#define PNP_FLAG_NO_DENOISER 2   /* k-space-only handle (pnp_fft2c / pnp_psnr): no activation planes */
#define PNP_FLAG_KEEP_STAGES 4   /* keep every U-Net stage output in memory for pnp_unet_read_stage (disables the
                                    fusion of the last 1x1 layer into the preceding conv's epilogue) */
#define PNP_FLAG_BF16_CONVS 8    /* BASELINE configs[4]: the 26 conv3x3 layers with Cin >= 32 round their input patch to
                                    bfloat16 (nearest even), carry every weight as TWO bfloat16 terms hi = bf16(w),
                                    lo = bf16(w - hi), and run on v_mfma_f32_32x32x16_bf16 with f32 accumulation - one MFMA
                                    per term, i.e. the convolution of the rounded activations with the 16-bit-mantissa weight
                                    hi + lo; bias, pooling, upsampling, the first and last layer and the k-space stage stay
                                    f32 (activation tensors between two such layers may be HELD as bf16 - rounded once by
                                    their producer exactly as the consumer's staging would, so the output does not change;
                                    such a stage is not readable through pnp_unet_read_stage unless the handle has
                                    PNP_FLAG_KEEP_STAGES).  NOT the reference's arithmetic: parity is against the oracle's
                                    bf16-operand mode, and the PSNR offset to the f32 reference is bounded by north_star's
                                    0.01 dB over configs[4]'s 50 iterations (tests/golden/g8_config4.npz; measured 0.002-0.003).
                                    PNP_BF16_W1=1 in the environment at pnp_create selects ONE term per weight (half the
                                    MFMAs; the offset then reaches 0.015 dB at iteration 50): an ablation, not a mode */

/* ---- lifetime ------------------------------------------------------------------------------ */

/* Replaces: PnPEnv(max_episode_step, denoiser, device_type) construction (evaluation/env.py:31-33)
 * minus the ARNIQA fetch (:34-40, out of scope).  Allocates the engine's private workspace
 * (activation planes, FFT scratch, pre-shifted k-space constants). */
int pnp_create(const pnp_config* cfg, pnp_handle* out);
int pnp_destroy(pnp_handle h);
const char* pnp_last_error(void);
const char* pnp_version(void);

/* Replaces: UNetDenoiser2D.__init__ -> net.load_state_dict (evaluation/noise.py:146-148).
 * `blob` (HOST) = the 56 state_dict tensors concatenated in state_dict order
 * (inc.conv.conv-0.conv2d.weight, .bias, ... outc.conv.weight, outc.conv.bias), weights OIHW
 * float32 exactly as nn.Conv2d stores them; n_floats must be 11,773,857. */
int pnp_load_unet_weights(pnp_handle h, const float* blob, size_t n_floats);

/* ---- the hot path --------------------------------------------------------------------------- */

/* Replaces: PnPEnv.reset (evaluation/env.py:57-71).
 *   x0, y0 : DEVICE complex64 [N,1,H,W]  (view_as_complex of the .mat arrays)
 *   mask   : DEVICE uint8 [H,W] (mask_n == 1, shared by all slices - the reference's case) or
 *            [N,H,W] (mask_n == N)
 * Writes   x (DEVICE float32 [N,1,H,W]) = Re(x0);  z = x0;  u = 0   (complex64 [N,1,H,W]),
 * and stores the k-space constants of the episode inside the engine (fftshift-folded mask and
 * y0), so `y0`/`mask` need not outlive the call. */
int pnp_reset(pnp_handle h, const float* x0, const float* y0, const uint8_t* mask, int mask_n,
              float* x, float* z, float* u, void* stream);

/* Replaces: the reference's `states['y0']` / `states['mask']` travelling WITH the state dict
 * (evaluation/env.py:71: every `step` reads them from the dict it is handed, :88-90).  The engine keeps ONE set of
 * episode constants; a caller that interleaves episodes on one handle (two environments, a tree search next to a
 * greedy rollout) re-installs the constants of the episode it is about to step.  Same arguments and pre-shift as
 * pnp_reset, the iterate (x, z, u) is not touched.  The Python shim calls it automatically when the `states` it is
 * handed belong to another episode than the engine's live one. */
int pnp_set_kspace(pnp_handle h, const float* y0, const uint8_t* mask, int mask_n, void* stream);

/* Replaces: PnPEnv.step (evaluation/env.py:74-100), batched over the N resident slices.
 *   mu, sigma_d : DEVICE float32 [N]  per-slice penalty and denoiser noise level (action_dict)
 *   t_action    : DEVICE float32 [N] or NULL; slice n with t_action[n] > 0.5 is `done`: its
 *                 x/z/u/t_state are left untouched (env.py:79-81)
 *   x           : DEVICE float32 [N,1,H,W]  out: denoiser output (states['x'])
 *   z, u        : DEVICE complex64 [N,1,H,W] in/out (states['z'], states['u'])
 *   t_state     : DEVICE float32 [N] or NULL; += 1/30 for slices that stepped (env.py:98)
 *   done        : DEVICE uint8 [N] or NULL; out: 1 where the slice was done */
int pnp_step(pnp_handle h, const float* mu, const float* sigma_d, const float* t_action,
             float* x, float* z, float* u, float* t_state, uint8_t* done, void* stream);

/* ---- stage entry points (the reference's plug-in operators; also used by tests/profiling) ---- */

/* Replaces: denoiser(x, sigma) = UNetDenoiser2D.forward (evaluation/noise.py:155-164):
 * out = clamp(x + UNet(cat[x, sigma plane])[:, :1], 0, 1).  x_in/out DEVICE float32 [N,1,H,W]
 * (may alias), sigma DEVICE float32 [N]. */
int pnp_denoise(pnp_handle h, const float* x_in, const float* sigma, float* out, void* stream);

/* A second plug-in regulariser beside the U-Net: isotropic total variation by Chambolle's dual projection (the reference has one prior only,
 * its U-Net; this is the classical baseline a PnP result is reported against).  Per slice, with v the input image [H, W], lam its weight,
 * K = iters, tau = 1/8, forward differences with Neumann ends ((Dy a)[i,j] = a[i+1,j] - a[i,j] for i < H-1 and 0 on the last row, Dx likewise)
 * and div = -D^T:
 *     not (lam > 0):  out = min(max(v, 0), 1)                                (lam = 0; a negative or NaN weight is treated alike)
 *     else:  w = v * (1 / lam);  py = px = 0;
 *            K times (Jacobi: every pixel reads the p of the iteration before):
 *                d = div(py, px) - w;   gy = Dy d;   gx = Dx d;   r = 1 / (1 + tau sqrt(gy^2 + gx^2));
 *                py = (py + tau gy) r;  px = (px + tau gx) r
 *            out = min(max(v - lam div(py, px), 0), 1)
 * float32 throughout, every operation one IEEE operation in this order (fma = one rounding; p outside the image reads as 0):
 *     rl  = 1 / lam                                                          (one IEEE reciprocal per slice)
 *     d(i,j) = ((py[i,j] - py[i-1,j]) + (px[i,j] - px[i,j-1])) - v[i,j] * rl (the product is rounded, then subtracted)
 *     gy  = i < H-1 ? d(i+1,j) - d(i,j) : 0;     gx = j < W-1 ? d(i,j+1) - d(i,j) : 0
 *     s   = fma(gx, gx, gy * gy);    den = fma(tau, sqrt(s), 1);    r = 1 / den              (IEEE square root and reciprocal)
 *     py  = fma(tau, gy, py) * r;    px = fma(tau, gx, px) * r
 *     out = min(max(fma(-lam, (py[i,j] - py[i-1,j]) + (px[i,j] - px[i,j-1]), v[i,j]), 0), 1)
 * The result at a pixel is a pure function of its slice's v, lam and K: it depends neither on N, the slice's place in the batch, the stream,
 * the handle kind, nor on how the kernels cut the image into tiles; no atomics, no reductions.  A constant image comes back bit for bit
 * (clamped).  The clamp mirrors pnp_denoise.
 *   x_in, out : DEVICE float32 [N,1,H,W]; they may alias (exactly, not partly), as in pnp_denoise
 *   lam       : DEVICE float32 [N];   iters : 1..PNP_TV_MAX_ITERS
 * Any handle kind (PNP_FLAG_NO_DENOISER, bf16 convs, single- or multi-coil mode) and any size pnp_create accepts; the call changes neither the
 * handle's mode nor its installed constants.
 * SETUP-TIME SEMANTICS, as pnp_estimate_sens: the first call that runs the operator on a handle (this one, or pnp_step under PNP_PRIOR_TV)
 * allocates 8 n H W bytes (one plane of (py, px) pairs through which launches hand the dual over; the second plane of the ping-pong is the
 * data-fidelity stage's scratch) inside the call, all-or-nothing (on PNP_ERR_NOMEM the handle keeps the workspace it had), counted by
 * pnp_workspace_bytes; later calls allocate nothing and are asynchronous.  Calls on one handle are stream-ordered (they share that workspace).
 * PNP_TV_NAIVE=1 in the environment at pnp_create selects one launch per iteration instead of the fused kernel (same bits; a check and a
 * timing baseline, not a mode).
 * Every argument error (null handle or pointer, iters outside 1..64) is reported before any HIP call and leaves the outputs untouched. */
#define PNP_TV_MAX_ITERS 64
int pnp_tv_denoise(pnp_handle h, const float* x_in, const float* lam, int iters, float* out, void* stream);

/* The prior of pnp_step's x-update, per handle.  PNP_PRIOR_UNET (the default: a handle that never calls the setter is what it always was) runs
 * the U-Net of pnp_denoise.  PNP_PRIOR_TV computes, in place of the U-Net forward,
 *     x = TV(float32(Re z - Re u), lam_n = float32(tv_scale) * sigma_d[n], tv_iters)           (the operator of pnp_tv_denoise)
 * read directly from the two complex planes (no real copy is made first); the k-space stage then runs as before, closed form or CG, whichever
 * constants are installed.  Slices with t_action > 0.5 keep x, z, u, t_state bit for bit; done and t_state behave as before.  Under
 * PNP_PRIOR_TV pnp_step needs no weights and runs on a PNP_FLAG_NO_DENOISER handle (which otherwise cannot step: PNP_ERR_STATE);
 * PNP_PRIOR_UNET on such a handle is refused with PNP_ERR_STATE.  Setting the prior back to PNP_PRIOR_UNET gives steps bit-identical to a
 * handle that never left it.  The prior is stateless - the dual starts from 0 in every call - so snapshots, residuals and every driver work
 * unchanged.
 *   prior : PNP_PRIOR_UNET or PNP_PRIOR_TV;   tv_scale : finite, >= 0;   tv_iters : 1..PNP_TV_MAX_ITERS
 * (tv_scale and tv_iters are checked and stored for PNP_PRIOR_TV only; PNP_PRIOR_UNET leaves the stored pair as it was).  No HIP call is made.
 * pnp_get_prior returns the current prior and the stored pair (1.0 and 20 on a fresh handle); all three pointers are required.
 * Every argument error (null handle or pointer, an unknown prior, tv_scale negative or not finite, tv_iters outside 1..64) leaves the handle
 * and the outputs untouched. */
#define PNP_PRIOR_UNET 0
#define PNP_PRIOR_TV   1
int pnp_set_prior(pnp_handle h, int prior, double tv_scale, int tv_iters);
int pnp_get_prior(pnp_handle h, int* prior, double* tv_scale, int* tv_iters);

/* A third plug-in regulariser: Haar wavelet shrinkage, the l1-wavelet term of Sparse MRI and, in its translation-invariant (cycle-spun) form,
 * the classical denoiser reported beside total variation.  Per slice, with v the input image [H, W] (H, W multiples of 16), lam >= 0 the
 * threshold, J = levels, periodic boundaries.  One 2-D Haar step on four samples p00 p01 / p10 p11 of the approximation a_(j-1) (a_0 = v):
 *     a  = ((p00 + p01) + (p10 + p11)) / 2        dh = ((p00 - p01) + (p10 - p11)) / 2
 *     dv = ((p00 + p01) - (p10 + p11)) / 2        dd = ((p00 - p01) - (p10 - p11)) / 2
 * and the synthesis is its transpose.
 *   PNP_HAAR_ORTHO : the decimated orthonormal transform: J levels on aligned 2 x 2 groups, the three detail bands of every level
 *                    soft-thresholded by lam, the coarsest approximation untouched, the transform inverted.  Unclamped this is exactly
 *                    prox_{lam ||detail coefficients||_1}(v).
 *   PNP_HAAR_TI    : the mean over all 4^J circular shifts (sy, sx), 0 <= sy, sx < 2^J, of shift^-1 . ORTHO . shift (full cycle spinning),
 *                    computed as the undecimated transform: at level j, with h = 2^(j-1), the block at (i, k) has the samples (i, k), (i, k+h),
 *                    (i+h, k), (i+h, k+h) of a_(j-1), and the synthesis averages the four reconstructions that reach a pixel.
 * Both are evaluated in the residual form  out = min(max(v - r, 0), 1),  r the synthesis, with zero approximation, of the clipped details
 * clip(d, -lam, lam) = d - soft(d, lam): the same function in exact arithmetic; lam = 0 gives the clamp bit for bit and a constant image
 * comes back bit for bit (its details are exactly 0).  float32 throughout, every operation one IEEE operation in this order (no fma; every
 * scale factor an exact power of two):
 *     not (lam > 0):  out = min(max(v, 0), 1)                                (lam = 0; a negative or NaN threshold is treated alike)
 *     a, dh, dv, dd as written above, "/ 2" a product with 0.5;   ch = min(max(dh, -lam), lam), cv, cd likewise
 *     with s = r_j of the block (r_J = 0):
 *         q00 = (s + ch) + (cv + cd)    q01 = (s - ch) + (cv - cd)    q10 = (s + ch) - (cv + cd)    q11 = (s - ch) - (cv - cd)
 *     ORTHO:  r_(j-1)(2i+a, 2k+b) = q_ab * 0.5                                          (block (i, k) of level j, a, b in {0, 1})
 *     TI:     r_(j-1)(i, k) = ((q00 of block (i, k) + q01 of block (i, k-h)) + (q10 of block (i-h, k) + q11 of block (i-h, k-h))) * 0.125
 *     out = min(max(v - r_0, 0), 1)
 * The result at a pixel is a pure function of its slice's v, lam, J and mode: it depends neither on N, the slice's place in the batch, the
 * stream, the handle kind, nor on how the kernels cut the image into tiles; no atomics, no reductions.  The clamp mirrors pnp_denoise.
 *   x_in, out : DEVICE float32 [N,1,H,W]; they may alias (exactly, not partly), as in pnp_tv_denoise
 *   lam       : DEVICE float32 [N];   levels : 1..PNP_HAAR_MAX_LEVELS;   mode : PNP_HAAR_TI or PNP_HAAR_ORTHO
 * Any handle kind (PNP_FLAG_NO_DENOISER, bf16 convs, single- or multi-coil mode) and any size pnp_create accepts; the call changes neither the
 * handle's mode nor its installed constants.  PNP_HAAR_TI is ONE launch (a workgroup keeps a 128 x 128 region on chip and stores the tile
 * inside it, the region minus 2^J - 1 pixels all round); when out aliases x_in the launch writes the data-fidelity stage's scratch plane and a
 * device-to-device copy on the stream ends the call (a launch reads its neighbours' halos).  Calls on one handle are stream-ordered.
 * The shipped forms need no workspace.  PNP_HAAR_NAIVE=1 in the environment at pnp_create selects, for PNP_HAAR_TI, one launch per level
 * down and per level up with the planes in device memory (same bits; a check and a timing baseline, not a mode); its planes, 20 n H W bytes
 * (a_1 .. a_3 and two residual planes), follow the SETUP-TIME SEMANTICS of pnp_tv_denoise: allocated inside the first TI call on such a
 * handle, all-or-nothing (on PNP_ERR_NOMEM the handle keeps the workspace it had), counted by pnp_workspace_bytes; later calls allocate
 * nothing and are asynchronous.
 * Every argument error (null handle or pointer, levels outside 1..4, an unknown mode) is reported before any HIP call and leaves the outputs
 * untouched. */
#define PNP_HAAR_TI         0
#define PNP_HAAR_ORTHO      1
#define PNP_HAAR_MAX_LEVELS 4
int pnp_haar_denoise(pnp_handle h, const float* x_in, const float* lam, int levels, int mode, float* out, void* stream);

/* Makes the Haar operator the x-update of pnp_step (pnp_get_prior then reports PNP_PRIOR_HAAR; pnp_set_prior itself takes PNP_PRIOR_UNET and
 * PNP_PRIOR_TV only and switches away from it as from any prior):
 *     x = Haar(float32(Re z - Re u), lam_n = float32(haar_scale) * sigma_d[n], levels, mode)      (the operator of pnp_haar_denoise)
 * read directly from the two complex planes (no real copy is made first).  The semantics are those of PNP_PRIOR_TV: pnp_step needs no weights
 * and runs on a PNP_FLAG_NO_DENOISER handle; slices with t_action > 0.5 keep x, z, u, t_state bit for bit; the prior is stateless, so
 * snapshots, residuals and every driver work unchanged; pnp_set_prior(h, PNP_PRIOR_UNET, ...) afterwards gives steps bit-identical to a handle
 * that never left the U-Net, pnp_set_prior(h, PNP_PRIOR_TV, ...) switches to total variation as before.  The TV pair of pnp_get_prior is
 * untouched.  No HIP call is made.
 *   haar_scale : finite, >= 0;   levels : 1..PNP_HAAR_MAX_LEVELS;   mode : PNP_HAAR_TI or PNP_HAAR_ORTHO
 * pnp_get_prior_haar returns the stored triple (1.0, 3, PNP_HAAR_TI on a fresh handle) whatever the current prior; all three pointers are
 * required.  Every argument error (null handle or pointer, levels outside 1..4, an unknown mode, haar_scale negative or not finite) leaves the
 * handle and the outputs untouched. */
#define PNP_PRIOR_HAAR      2
int pnp_set_prior_haar(pnp_handle h, double haar_scale, int levels, int mode);
int pnp_get_prior_haar(pnp_handle h, double* haar_scale, int* levels, int* mode);

/* Replaces: fft(img) / ifft(img) (evaluation/utils/transformations.py:6-12 / :14-19): centred
 * (ifftshift -> fftn/ifftn norm='ortho' -> fftshift) 2-D transform over the last two dims.
 * in/out DEVICE complex64 [batch,H,W] (may alias); hh, ww are the engine's h, w and batch <= n.
 * Sides of 2^a * 5^b (80 .. 800) run mixed-radix passes (radix 5, then radix 4 / 2); other sizes are refused. */
int pnp_fft2c(pnp_handle h, const float* in, float* out, int batch, int hh, int ww, int inverse, void* stream);

/* Replaces: the data-fidelity half of PnPEnv.step (evaluation/env.py:87-93) on its own:
 * z <- ifft_c(where(mask, (mu*fft_c(x+u) + y0)/(1+mu), fft_c(x+u)));  u <- u + x - z.
 * Uses the k-space constants stored by pnp_reset. */
int pnp_prox_dual(pnp_handle h, const float* mu, const float* t_action, const float* x, float* z, float* u,
                  void* stream);

/* Replaces: PnPEnv.compute_reward -> torch_psnr (evaluation/env.py:112-125): per-slice
 * 10*log10(1/mean((clamp(x,0,1)-gt)^2)).  x, gt DEVICE float32 [N,1,H,W]; out DEVICE float32 [N]. */
int pnp_psnr(pnp_handle h, const float* x, const float* gt, float* out, void* stream);

/* Replaces: calculate_ssim (evaluation/utils/transformations.py:61-95), per slice, on the device:
 *   G = gaussian_filter(sigma = 1.5) with `radius` taps each side (scipy's radius int(1.5 * truncate + 0.5), truncate =
 *   win_size // 2: 8 for the default win_size 11), boundary 'reflect';  c1 = (k1 data_range)^2, c2 = (k2 data_range)^2;
 *   map = ((2 mu_x mu_y + c1)(2 sigma_xy + c2)) / ((mu_x^2 + mu_y^2 + c1)(sigma_x^2 + sigma_y^2 + c2)), out[n] = mean of
 *   slice n's map over all H x W pixels (no border crop).
 *   x, gt : DEVICE float32 [N,1,H,W] of the handle's shape;  out : DEVICE float32 [N];  map : DEVICE float32 [N,H,W] or NULL
 *   (no map store).  flags: PNP_SSIM_CLAMP_X or 0.  radius 1..16, data_range > 0; any handle (PNP_FLAG_NO_DENOISER too).
 * Filters in float32 with the taps computed in double; the per-slice mean is summed in double in a fixed order (bitwise
 * reproducible, no atomics).  Uses a partial-sum buffer of the handle's workspace: calls on one handle are stream-ordered. */
#define PNP_SSIM_CLAMP_X 1   /* clamp x to [0,1] before filtering (what pnp_psnr does); 0 = the reference's calculate_ssim */
int pnp_ssim(pnp_handle h, const float* x, const float* gt, float data_range, float k1, float k2, int radius, int flags,
             float* out, float* map, void* stream);

/* ADMM residuals of the iterate (x, z, u), per slice, on the device - what a convergence test needs and the reference never computes
 * (its drivers stop on the policy's T only).  With (x_p, z_p, u_p) the iterate stored in `prev` and ||.|| the Euclidean norm over the
 * slice's H x W pixels (complex modulus for z, u), out[n] holds PNP_RES_COLS float32 columns:
 *   0 primal = ||x - z||   (x taken as complex with zero imaginary part)
 *   1 dx = ||x - x_p||     2 dz = ||z - z_p||     3 du = ||u - u_p||
 *   4 delta = (dx + dz + du) / sqrt(H W)   - the fixed-point stopping quantity of Chan, Wang, Elgendy (2017)
 *   5 dc = ||where(mask, fft_c(x) - y0, 0)||, fft_c = the centred orthonormal transform of pnp_fft2c, mask / y0 = the episode constants
 *   x : DEVICE float32 [N,1,H,W];  z, u : DEVICE complex64 [N,1,H,W];  out : DEVICE float32 [N, PNP_RES_COLS]
 *   prev : DEVICE buffer written by pnp_snapshot (only its x, z, u planes are read) or NULL without PNP_RES_DELTA
 *   flags : PNP_RES_DELTA (columns 1-4) | PNP_RES_DC (column 5).  Column 0 is always written; columns not asked for are written as 0.
 * x, z, u and prev must be 16-byte aligned (any hipMalloc / torch allocation is).  PNP_RES_DC needs pnp_reset / pnp_set_kspace
 * (PNP_ERR_STATE otherwise), sides the k-space stage accepts, and uses the data-fidelity stage's scratch plane.  Every argument error
 * is reported before any HIP call and leaves `out` untouched.  Any handle kind (PNP_FLAG_NO_DENOISER, bf16 convs).
 * Differences are formed in float32 (one rounding), squared and summed in float64 in a fixed order: no atomics, bitwise reproducible,
 * and a slice gives the same bits in columns 0-4 wherever it sits in the batch.  Uses a partial-sum buffer of the handle's workspace:
 * calls on one handle are stream-ordered. */
#define PNP_RES_COLS   6
#define PNP_RES_DELTA  1   /* columns 1-4; needs prev */
#define PNP_RES_DC     2   /* column 5; needs pnp_reset / pnp_set_kspace */
int pnp_residuals(pnp_handle h, const float* x, const float* z, const float* u, const void* prev, int flags, float* out,
                  void* stream);

/* Replaces: the preparation of the evaluation `.mat` files the reference loads (dataset/datasets.py:153-160,191-199: keys x0, y0, ATy0,
 * mask, gt), which it leaves to an external download - the simulated CS-MRI acquisition of N ground-truth slices, on the device:
 *   y0   = mask ? fft_c(gt) + sigma_n (g_re + i g_im) : 0        (off-mask bins are stored as +0.0)
 *   aty0 = ifft_c(y0)
 *   x0   = max(aty0, 0) on the real AND the imaginary plane      (the np.clip of datasets.py:160 on the stacked array)
 * fft_c / ifft_c = the centred orthonormal transforms of pnp_fft2c.
 *   gt   : DEVICE float32 [N,1,H,W]
 *   mask : DEVICE uint8 [H,W] (mask_n == 1) or [N,H,W] (mask_n == N), the reference's centred layout, as pnp_reset takes it
 *   y0   : DEVICE complex64 [N,1,H,W];  aty0, x0 : the same or NULL (not stored).  No output may alias gt.
 *   sigma_n : standard deviation of the noise per component, finite and >= 0;  flags : reserved, must be 0
 * Noise: g_re[p] = gauss(seed + n, 9001, p), g_im[p] = gauss(seed + n, 9003, p), p = y W + x the row-major index of the centred bin and
 * gauss(s, t, p) = sqrt(-2 ln u1) cos(2 pi u2) with u = (24 top bits of splitmix64(p ^ splitmix64(s * 0x100000001B3 + t'))) / 2^24 for
 * t' = t (u1, clamped below at 2^-25) and t + 1 (u2) - the counter hash of the Python package's weights.hash_uniform and its
 * synthetic.make_problem, so that a problem built there in float64 and one acquired here agree to rounding.  The integer hash is exact;
 * Box-Muller, the product with sigma_n and the sum with the transform are formed in float64 and rounded to float32 once.
 * With sigma_n == 0 nothing is drawn: a sampled bin holds the transform's own float32 value (its sign of zero included).
 * A slice's outputs depend on (its gt, its mask, sigma_n, seed + n) only: not on N, not on its place in the batch; bitwise reproducible.
 * Sides the k-space stage accepts (any other is refused); any handle kind (PNP_FLAG_NO_DENOISER, bf16 convs).  Uses the data-fidelity
 * stage's scratch plane and allocates nothing: calls on one handle are stream-ordered.  Every argument error (NULL gt, mask or y0, mask_n
 * not 1 or N, sigma_n negative or not finite, flags != 0) is reported before any HIP call and leaves the outputs untouched. */
int pnp_acquire(pnp_handle h, const float* gt, const uint8_t* mask, int mask_n, double sigma_n, uint64_t seed, int flags,
                float* y0, float* aty0, float* x0, void* stream);

/* ---- multi-coil (SENSE) data fidelity ----------------------------------------------------------
 * The reference restores single-coil acquisitions only: its k-space subproblem has the closed form of pnp_prox_dual because the forward
 * operator is M F.  With C coil sensitivity maps S_c the operator of slice n is
 *     A p = [ M . fft_c(S_c . p) ]_c ,   A^H q = sum_c conj(S_c) . ifft_c(M . q_c) ,   Nop(p) = A^H A p + mu_n p
 * (fft_c / ifft_c = the centred orthonormal pair of pnp_fft2c) and the subproblem (A^H A + mu I) z = A^H y + mu (x + u) is solved by a FIXED
 * number K = cg_iters of conjugate-gradient iterations, warm-started from the incoming z.  Per slice that is not stopped:
 *     v = x + u;  b = aty + mu v  (aty = A^H y, formed once when the constants are installed);  r = b - Nop(z);  p = r;  rs = <r,r>;  bb = <b,b>
 *     K times:  q = Nop(p);  pq = Re<p,q>;  rs <= 0 or pq <= 0 ? (alpha = 0, beta = 0 : a frozen slice, never NaN) : alpha = rs / pq;
 *               z += alpha p;  r -= alpha q;  rs' = <r,r>;  beta = rs' / rs (0 when frozen);  p = r + beta p;  rs = rs'
 *     cg_res[n] = sqrt(rs / bb) (0 when bb == 0);   u <- u + x - z
 * Inner products are per slice; their terms are float32 values, multiplied and summed in float64 in a fixed order (no atomics): bitwise
 * reproducible, and a slice's bits depend neither on N nor on its place in the batch.  alpha and beta are computed in float64, live in
 * device memory and are applied as float32; no entry point synchronises with the host during a step.  Stopped slices (t_action > 0.5)
 * keep z and u bit for bit.  With C = 1 and S = 1 the operator has the two eigenvalues mu and 1 + mu, CG is exact after two iterations
 * and the stage is the reference's closed form.
 *
 * WHICH stage pnp_step / pnp_prox_dual run is decided by the constants installed LAST: pnp_set_kspace_mc / pnp_reset_mc put the handle in
 * multi-coil mode, pnp_set_kspace / pnp_reset return it to the single-coil stage (and it then gives the bits of a handle that never was in
 * multi-coil mode).  In multi-coil mode pnp_residuals' PNP_RES_DC column is sqrt(sum_c ||M (fft_c(S_c x) - y_c)||^2).
 * SETUP-TIME SEMANTICS: pnp_set_kspace_mc / pnp_reset_mc / pnp_acquire_mc allocate or grow the handle's coil workspace inside the call
 * (y: N C H W complex, scratch: N C H W complex, the maps: sens_n C H W complex, A^H y and three CG vectors: N H W complex each, partial
 * sums and scalars), which may synchronise the device; a call that does not need to grow it is asynchronous like pnp_reset.  The growth is
 * all-or-nothing (on PNP_ERR_NOMEM the handle keeps the workspace and the mode it had) and is counted by pnp_workspace_bytes.
 *   y0   : DEVICE complex64 [N,C,H,W], centred layout
 *   sens : DEVICE complex64 [C,H,W] (sens_n == 1, shared by all slices) or [N,C,H,W] (sens_n == N); copied, need not outlive the call
 *   mask : as in pnp_reset;   coils : 1..PNP_MC_MAX_COILS;   cg_iters : 1..PNP_MC_MAX_CG
 * Sizes the k-space stage accepts (any other is refused); any handle kind (PNP_FLAG_NO_DENOISER, bf16 convs).  Every argument error (NULLs,
 * coils outside 1..32, sens_n / mask_n not 1 or N, cg_iters outside 1..64, sigma_n negative or not finite) is reported before any HIP call
 * and leaves the outputs untouched. */
#define PNP_MC_MAX_COILS 32
#define PNP_MC_MAX_CG 64
int pnp_set_kspace_mc(pnp_handle h, const float* y0, const float* sens, int coils, int sens_n, const uint8_t* mask, int mask_n, int cg_iters,
                      void* stream);
/* pnp_set_kspace_mc plus pnp_reset's iterate: x = Re(x0), z = x0, u = 0 (x0 complex64 [N,1,H,W], e.g. pnp_acquire_mc's x0). */
int pnp_reset_mc(pnp_handle h, const float* x0, const float* y0, const float* sens, int coils, int sens_n, const uint8_t* mask, int mask_n,
                 int cg_iters, float* x, float* z, float* u, void* stream);
/* Coils of the installed multi-coil constants; 0 on a handle in single-coil mode (and on NULL). */
int pnp_mc_coils(pnp_handle h);
/* out : DEVICE float32 [N], the relative residual sqrt(rs / bb) the CG solve of the last pnp_step / pnp_prox_dual ended with (a slice that
 * was stopped in that call keeps its earlier value; 0 before the first solve).  PNP_ERR_STATE on a handle in single-coil mode. */
int pnp_mc_cg_residual(pnp_handle h, float* out, void* stream);
/* q = Nop(p) = A^H A p + mu p with the installed constants: p, q DEVICE complex64 [N,1,H,W] (must not alias), mu DEVICE float32 [N].  The
 * operator on its own, for tests and timing.  PNP_ERR_STATE on a handle in single-coil mode. */
int pnp_mc_normal(pnp_handle h, const float* p, const float* mu, float* q, void* stream);
/* pnp_acquire for C coils:  y_c = mask ? fft_c(S_c gt) + sigma_n (g_re + i g_im) : +0.0;  aty0 = A^H y;  x0 = max(aty0, 0) on both planes.
 *   gt : DEVICE float32 [N,1,H,W];  sens, mask : as above;  y0 : DEVICE complex64 [N,C,H,W];  aty0, x0 : complex64 [N,1,H,W] or NULL
 * Noise: pnp_acquire's counter hash with the streams 9001 + 4 c (real) and 9003 + 4 c (imaginary) for coil c, seed + n for slice n; with
 * C = 1 and S = 1 every output equals pnp_acquire's bit for bit.  flags : reserved, must be 0.  Does not change the handle's mode or
 * installed constants; uses (and may grow) the coil scratch. */
int pnp_acquire_mc(pnp_handle h, const float* gt, const float* sens, int coils, int sens_n, const uint8_t* mask, int mask_n, double sigma_n,
                   uint64_t seed, int flags, float* y0, float* aty0, float* x0, void* stream);

/* ---- non-Cartesian sampling: NUFFT pair and CG data fidelity ------------------------------------
 * The reference's "radial" acquisition is a radial MASK rasterised on the Cartesian grid.  A real radial, spiral or rosette acquisition has
 * its samples off the grid; this section is the single-coil stage for such data.  One trajectory is shared by all slices of a handle.
 *
 * COORDINATES AND THE EXACT OPERATOR.  Sample m has the frequency (ky, kx) in cycles per pixel, each in [-0.5, 0.5]; with the centred pixel
 * coordinates qy = iy - H/2, qx = ix - W/2
 *     (A x)_m = (1 / sqrt(H W)) sum_q x[q] exp(-2 pi i (ky qy + kx qx))
 * so that the sample at ky = (j - H/2) / H, kx = (l - W/2) / W is bin (j, l) of pnp_fft2c.
 * GRID.  The operator is evaluated on an oversampled gh x gw grid: each side is a side the k-space stage accepts with 4 gh >= 5 H and
 * 4 gw >= 5 W; 0 selects the smallest such side (64 -> 80, 128 -> 160, 256 -> 320, 320 -> 400, 512 -> 640, 640 -> 800, 800 -> 1024; 16 -> 32,
 * 32 -> 64, 80 -> 128, 160 -> 256, 400 -> 512).  H and W are therefore at most 800: a 1024 side is refused with a message.  The oversampling
 * ratio is per axis, sigma = g / side.
 * KERNEL.  The "exponential of semicircle" kernel of width J in {4, 6, 8} grid points,
 *     phi(t) = exp(beta (sqrt(1 - (2 t / J)^2) - 1)) for |2 t / J| < 1, 0 elsewhere;   beta = 2.30 J when sigma == 2, else 0.97 pi J (1 - 1 / (2 sigma)).
 * FOOTPRINT AND WEIGHTS of one sample, per axis: the grid coordinate is u = k g + g/2; the footprint starts at i0 = ceil(u - J/2) and covers
 * the points i0 .. i0 + J - 1 taken mod g (the grid is periodic); the weights phi(u - i) are formed in float64 on the host and rounded to
 * float32 once.
 * DECONVOLUTION.  c[q] = 1 / phihat(q), phihat(q) = 2 int_0^{J/2} phi(t) cos(2 pi q t / g) dt by a 128-node Gauss-Legendre quadrature in
 * float64, rounded to float32 once; the scale sqrt(gh gw / (H W)) between the grid's orthonormal transform and 1 / sqrt(H W) is folded in
 * (per axis: cy[qy] = sqrt(gh / H) / phihat_y(qy)).
 * FORWARD (pnp_nufft_forward): the image times cy[qy] cx[qx] (the float32 product of the two factors), zero-padded, centred, into the grid;
 * the centred forward transform of pnp_fft2c on the grid (the engine's row and column passes with the plan's own twiddles); then per sample
 * t_iy = sum over ix ascending of wx[ix] X[iy][ix] and acc = sum over iy ascending of wy[iy] t_iy, real and imaginary part each an fma chain
 * from +0.
 * ADJOINT (pnp_nufft_adjoint): the conjugate transpose of the forward as implemented - the same float32 weights and factors.  v_m = w_m y_m
 * (w optional, NULL = 1) is spread onto the grid, the centred inverse transform runs, the grid is cropped and multiplied by cy cx.
 * SPREADING ORDER.  The value of a grid point is ONE fma chain from +0 over the samples whose footprint contains it, in ascending sample
 * index, of the terms (v_m wy) * wx (v_m wy rounded first).  A sample cannot reach a point twice through the wrap (J <= 8 < 32 <= g).  There
 * are no atomics: the bits depend on (plan, input) only - not on N, the slice's place in the batch, the stream, or the workgroup that owns
 * the point.  (Samples are assumed finite: a non-finite sample spoils the whole gridding tiles its footprint meets.)
 *
 * pnp_nufft_plan: SETUP-TIME SEMANTICS, as pnp_load_unet_weights - it builds the plan on the host, uploads it and allocates inside the call,
 * all-or-nothing through the handle's workspace (on PNP_ERR_NOMEM the handle keeps the plan and the workspace it had), counted by
 * pnp_workspace_bytes: the grid buffer 8 n gh gw, the sample buffer 8 n M, and the plan itself: 8 M (footprint starts) + 8 J M (weights) +
 * 4 (H + W) (factors) + 8 (gh + gw) (twiddles) + 4 (gh gw / 256 + 1) + 4 B (the gridding bins: B <= 4 M entries).  A later plan allocates
 * only what it needs beyond the plan before it, and waits for the device.  One plan per handle: a new plan replaces the old one.  If
 * non-Cartesian constants were installed they are dropped - the handle then has NO episode constants, and pnp_step / pnp_prox_dual give
 * PNP_ERR_STATE until some are installed; Cartesian and multi-coil constants are not touched.
 *   traj : HOST float64 [M][2] = (ky, kx), every coordinate finite and in [-0.5, 0.5];   m : 1..PNP_NUFFT_MAX_SAMPLES
 *   gh, gw : grid sides or 0;   width : J in {4, 6, 8};   flags : reserved, must be 0
 * pnp_nufft_samples: M of the handle's plan, 0 without one (and on NULL).  pnp_nufft_grid: the plan's grid sides (PNP_ERR_STATE without one).
 * pnp_nufft_forward / pnp_nufft_adjoint: img DEVICE complex64 [batch,H,W], samples DEVICE complex64 [batch,M], weights DEVICE float32 [M] or
 * NULL; 1 <= batch <= n; no input may alias an output.  Without a plan: PNP_ERR_STATE.  They use the plan's grid buffer: calls on one handle
 * are stream-ordered.
 *
 * DATA FIDELITY.  pnp_set_kspace_nc / pnp_reset_nc install y (complex64 [N,M]), w (float32 [M] or NULL = 1; e.g. density compensation) and
 * aty = A^H W y, and put the handle in non-Cartesian mode by the rule of the multi-coil section: the stage that runs is the one whose
 * constants were installed LAST (pnp_mc_coils stays 0 in this mode; pnp_set_kspace / pnp_reset / the _mc calls leave it).  pnp_step and
 * pnp_prox_dual then run the multi-coil section's CG, word for word, on Nop(p) = A^H W A p + mu p and b = aty + mu (x + u): K = cg_iters
 * fixed iterations warm-started from z, float64 scalars on the device, a frozen slice never NaN, stopped slices keep their bits,
 * u <- u + x - z.  pnp_reset_nc also sets the iterate: x = Re(x0), z = x0, u = 0.  They copy y and w (8 n M + 4 M bytes, 8 n ceil(M / 2048)
 * for the misfit's partial sums, and the coil workspace's coil-independent part: four vectors 8 n H W each, partial sums and scalars), with
 * the setup-time semantics of pnp_set_kspace_mc.  The handle changes mode only after every launch of the install was accepted: a call
 * that fails (argument error, PNP_ERR_NOMEM, a refused launch) leaves the mode and the iterate as they were.  In this mode pnp_residuals'
 * PNP_RES_DC column is sqrt(sum_m w_m |(A x)_m - y_m|^2).
 * pnp_nc_normal (q = Nop(p)) and pnp_nc_cg_residual are the counterparts of pnp_mc_normal and pnp_mc_cg_residual: PNP_ERR_STATE on a handle
 * that is not in non-Cartesian mode.
 *
 * pnp_acquire_nc: pnp_acquire for the planned trajectory,  y = A gt + sigma_n (g_re + i g_im),  aty0 = A^H (dcf . y),  x0 = max(aty0, 0) on
 * both planes;  gt DEVICE float32 [N,1,H,W], dcf DEVICE float32 [M] or NULL, y DEVICE complex64 [N,M], aty0, x0 complex64 [N,1,H,W] or NULL.
 * Noise: pnp_acquire's counter hash with p = m, the streams 9001 / 9003 and seed + n; with sigma_n == 0 nothing is drawn and y equals
 * pnp_nufft_forward's bits.  A slice's outputs depend neither on N nor on its place in the batch.  It does not change the handle's mode.
 *
 * Every entry point here takes any handle kind with sides the k-space stage accepts, and reports every argument error (NULLs, a count or
 * size out of range, flags != 0, forbidden aliasing, a refused trajectory or grid) before any HIP call, leaving the outputs untouched. */
#define PNP_NUFFT_MAX_SAMPLES (1 << 22)
int pnp_nufft_plan(pnp_handle h, const double* traj, int64_t m, int gh, int gw, int width, int flags);
int64_t pnp_nufft_samples(pnp_handle h);
int pnp_nufft_grid(pnp_handle h, int* gh, int* gw);
int pnp_nufft_forward(pnp_handle h, const float* img, int batch, float* samples, void* stream);
int pnp_nufft_adjoint(pnp_handle h, const float* samples, const float* weights, int batch, float* img, void* stream);
int pnp_set_kspace_nc(pnp_handle h, const float* y, const float* w, int cg_iters, void* stream);
int pnp_reset_nc(pnp_handle h, const float* x0, const float* y, const float* w, int cg_iters, float* x, float* z, float* u, void* stream);
int pnp_nc_cg_residual(pnp_handle h, float* out, void* stream);
int pnp_nc_normal(pnp_handle h, const float* p, const float* mu, float* q, void* stream);
int pnp_acquire_nc(pnp_handle h, const float* gt, const float* dcf, double sigma_n, uint64_t seed, int flags, float* y, float* aty0, float* x0,
                   void* stream);

/* Coil sensitivity maps from the fully sampled calibration (ACS) block of multi-coil k-space: the low-resolution estimate, the first stage of
 * the multi-coil path when the acquisition brings no maps (the reference restores single-coil data and has no counterpart).  Per slice n, with
 * the centred bin p = (ky, kx), dy = ky - H/2, dx = kx - W/2:
 *     in block:  -acs_h/2 <= dy < acs_h/2  and  -acs_w/2 <= dx < acs_w/2
 *     win(p)   = 1                                                                      (PNP_SENS_BOX)
 *              = (0.5 + 0.5 cos(2 pi dy / acs_h)) (0.5 + 0.5 cos(2 pi dx / acs_w))      (PNP_SENS_HANN)
 *     k_c      = in block ? float32(win) * y0[n,c] : 0
 *     l_c      = ifft_c(k_c)                        (the centred orthonormal inverse of pnp_fft2c(..., inverse = 1))
 *     rss      = sqrt(sum_c |l_c|^2)
 *     smax_n   = max over the slice of rss
 *     sens_c   = (rss > 0 and rss > float32(thresh) * smax_n) ? l_c / rss : 0
 * The window factors and their product are formed in float64 and rounded to float32 once.  The terms of rss are the float32 components of l_c,
 * squared and summed in float64 in coil order; the square root is taken in float64 and rounded to float32 once.  The threshold product and the
 * division are float32 (an IEEE divide).  On the kept set the maps have unit root-sum-of-squares, so they absorb the object's slowly varying
 * phase and the image left to restore is close to real - the iterate this engine keeps.  ESPIRiT (calibration-matrix SVD, per-pixel
 * eigen-decomposition) is pnp_espirit_sens below; it starts from these low-resolution coil images.
 *   y0     : DEVICE complex64 [N,C,H,W], centred layout (what pnp_reset_mc takes); read inside the block only: the block must be fully sampled
 *   coils  : 1..PNP_MC_MAX_COILS;   acs_h, acs_w : even, 2 <= acs_h <= H, 2 <= acs_w <= W;   window : PNP_SENS_BOX or PNP_SENS_HANN
 *   thresh : in [0, 1);   flags : reserved, must be 0
 *   sens   : DEVICE complex64 [N,C,H,W] out: per-slice maps (sens_n = N for pnp_set_kspace_mc / pnp_reset_mc); must not alias y0.  The transforms
 *            run in place in this buffer: there is no [N,C,H,W] workspace
 *   rss    : DEVICE float32 [N,H,W] out, or NULL (then a plane of the handle's workspace holds it)
 * Any handle kind (single- or multi-coil mode, PNP_FLAG_NO_DENOISER, bf16 convs); the call changes neither the handle's mode nor its installed
 * constants.  Sizes the k-space stage accepts (any other is refused), n * coils <= 65535.  A slice's bits depend on (y0[n], acs_h, acs_w, window,
 * thresh) only: not on N, its place in the batch, the stream or the handle kind; no atomics, bitwise reproducible.
 * SETUP-TIME SEMANTICS, as pnp_acquire_mc: the first call allocates 4 n ceil(H W / 2048) + 4 n bytes (per-workgroup maxima and smax) and, the first
 * time rss is NULL, 4 n H W bytes more, inside the call, all-or-nothing (on PNP_ERR_NOMEM the handle keeps the workspace it had), counted by
 * pnp_workspace_bytes; later calls allocate nothing and are asynchronous.  Calls on one handle are stream-ordered (they share that workspace).
 * Every argument error (null handle, y0 or sens, sens == y0, coils outside 1..32, acs_h / acs_w odd, below 2 or above the handle's H / W, an
 * unknown window, thresh negative, >= 1 or not finite, flags != 0) is reported before any HIP call and leaves the outputs untouched. */
#define PNP_SENS_BOX  0
#define PNP_SENS_HANN 1
int pnp_estimate_sens(pnp_handle h, const float* y0, int coils, int acs_h, int acs_w, int window, double thresh, int flags,
                      float* sens, float* rss /* may be NULL */, void* stream);

/* Coil compression: SVD virtual coils.  Every cost of the multi-coil stage is linear in the coil count, so an acquisition with C channels is
 * first mixed down to V <= PNP_MC_MAX_COILS virtual coils by the leading eigenvectors of the calibration block's channel covariance; a unitary
 * mix keeps white noise white, so the SENSE model is unchanged with the maps mixed by the same matrix (the reference has no counterpart).
 *
 * pnp_coil_compress_matrix, per slice n, with the centred block of pnp_estimate_sens (-acs_h/2 <= ky - H/2 < acs_h/2, likewise in x):
 *     G[a][b]    = sum over the block's bins of y0[n,a] conj(y0[n,b])                                   (C x C Hermitian)
 *     G          = U diag(lambda) U^H,  lambda descending
 *     cmat[v][c] = conj(U[c][v]),  eig[v] = lambda_v        row v = virtual coil v:  y'_v = sum_c cmat[v][c] y_c
 *   Gram: the terms are the float32 components of y0, multiplied and summed in float64 (the products are exact).  The block's bins, in row-major
 *     block order, are dealt to ceil(B / per) workgroups of `per` consecutive bins, B = acs_h acs_w, per = max(1024, ceil(B / 64) rounded up
 *     to a multiple of 32); each sums its bins in order (re += ar br; re += ai bi; im += ai br; im -= ar bi) and a second launch adds the
 *     workgroups' partials in index order.  No atomics: the order depends on (H, W, acs_h, acs_w) only.  G is stored exactly Hermitian, its
 *     diagonal real.
 *   Eigen-decomposition: one workgroup per slice, float64, G and the vectors on chip: cyclic Jacobi in round-robin order (C padded to even, C - 1
 *     rounds of C / 2 disjoint rotations per sweep).  Before every sweep the workgroup tests off(G)_F <= 1e-14 * trace(G) and stops on it; at most
 *     24 sweeps (noisy 8- to 64-coil blocks stop after 5 to 8; an input that runs into the cap still has eigenvalues good to the off-diagonal that is left).  No
 *     host read.  A pair whose off-diagonal entry beta is exactly zero is skipped; otherwise tau = (G[q][q] - G[p][p]) / (2 |beta|),
 *     t = sgn(tau) / (|tau| + hypot(1, tau)) - no square of tau is formed, a vanishing beta gives t = 0.
 *   Order and phase: a stable descending sort of the diagonal; each eigenvector is multiplied by the unit complex number that makes its entry of
 *     largest modulus (squared moduli compared in float64, the lowest index wins a tie) real and positive, in float64; cmat is rounded to
 *     complex64 once and eig to float32 once.  An all-zero block gives cmat = identity and eig = 0; no finite input gives NaN.
 *   y0    : DEVICE complex64 [N,C,H,W], centred layout; read inside the block only
 *   coils : 1..PNP_CC_MAX_COILS;   acs_h, acs_w : even, 2 <= acs_h <= H, 2 <= acs_w <= W;   flags : reserved, must be 0
 *   cmat  : DEVICE complex64 [N,C,C] out;   eig : DEVICE float32 [N,C] out, descending;   gram : DEVICE complex128 [N,C,C] out, or NULL
 * A slice's bits depend on (y0[n], acs_h, acs_w) only: not on N, its place in the batch, the stream or the handle kind.
 * SETUP-TIME SEMANTICS, as pnp_estimate_sens: the first call allocates 16 n C^2 ceil(B / per) bytes (the Gram partials) and, when gram is NULL,
 * 16 n C^2 bytes more (the Gram), inside the call, all-or-nothing (on PNP_ERR_NOMEM the handle keeps the workspace it had), counted by
 * pnp_workspace_bytes.  A later call allocates only if it needs more than any call before it (more coils, a block of more workgroups), and then
 * waits for the device; every other call allocates nothing and is asynchronous.  Calls on one handle are stream-ordered.
 *
 * pnp_coil_compress_apply:  out[n,v,p] = sum_{c = 0 .. C-1} cmat[n or 0][v][c] * in[n,c,p],  v < out_coils, over all H W bins - k-space or coil
 * maps: the kernel is pointwise, and no map enters it specially.  float32, from re = im = +0, c ascending, every product contracted:
 *     re = fma(a.re, x.re, re);  re = fma(-a.im, x.im, re);  im = fma(a.re, x.im, im);  im = fma(a.im, x.re, im)        (a = cmat[v][c], x = in[c])
 * so an identity or permutation matrix copies the planes exactly (a -0 component comes out as +0), and a bin that is zero in every coil stays zero.
 *   in        : DEVICE complex64 [N,C,H,W];   coils : 1..PNP_CC_MAX_COILS
 *   cmat      : DEVICE complex64 [cmat_n,C,C];   cmat_n : 1 (one matrix for all slices) or N
 *   out_coils : 1..min(coils, PNP_MC_MAX_COILS);   out : DEVICE complex64 [N,out_coils,H,W], must not alias in or cmat
 * It moves 8 C + 8 V bytes per pixel (each input value is read once), allocates nothing and is asynchronous.
 *
 * Both calls take any handle kind and change neither the handle's mode nor its installed constants; n <= 65535.  Every argument error (null
 * handle or pointer, aliased buffers, coils outside 1..64, out_coils outside 1..min(coils, 32), cmat_n not 1 or n, acs_h / acs_w odd, below 2
 * or above the handle's H / W, flags != 0) is reported before any HIP call and leaves the outputs untouched. */
#define PNP_CC_MAX_COILS 64
int pnp_coil_compress_matrix(pnp_handle h, const float* y0, int coils, int acs_h, int acs_w, int flags, float* cmat, float* eig,
                             double* gram /* may be NULL */, void* stream);
int pnp_coil_compress_apply(pnp_handle h, const float* in, int coils, const float* cmat, int cmat_n, int out_coils, float* out, void* stream);

/* Coil noise pre-whitening: the head of the chain whiten -> compress -> maps -> SENSE.  Every later stage takes the receiver noise as white and
 * equal across channels; a real array has unequal gains and correlated channels, so the channel noise covariance Psi is measured from a
 * noise-only scan and the channels are mixed by W = L^-1, Psi = L L^H, after which W Psi W^H = I (the reference has no counterpart).  The maps of
 * a whitened acquisition are mixed by the same W (S' = W S), or estimated from the whitened k-space.
 *
 * pnp_noise_cov, per scan n:   Psi[a][b] = (1 / S) sum_{s < S} noise[n,a,s] conj(noise[n,b,s])        (C x C Hermitian, the Gram convention of
 *   pnp_coil_compress_matrix).  The terms are the float32 components of the samples, multiplied and summed in float64 (the products are exact).
 *   The samples are dealt to ceil(S / per) workgroups of `per` consecutive samples, per = max(1024, ceil(S / 64) rounded up to a multiple of 32)
 *   (the Gram's rule); each sums its samples in order (re += ar br; re += ai bi; im += ai br; im -= ar bi) and a second launch adds the
 *   workgroups' partials in index order from 0.0, then divides once by S in float64.  No atomics: the order depends on (C, S) only.  Psi is
 *   stored exactly Hermitian, its diagonal real.
 *   noise : DEVICE complex64 [noise_n,C,S];   noise_n : 1..65535 (independent of the handle's n);   coils : 1..PNP_PW_MAX_COILS;   samples >= 1
 *   flags : reserved, must be 0;   psi : DEVICE complex128 [noise_n,C,C] out, must not alias noise
 *   SETUP-TIME SEMANTICS, as pnp_coil_compress_matrix: the first call allocates 16 noise_n C^2 ceil(S / per) bytes (the partials) inside the call,
 *   all-or-nothing (on PNP_ERR_NOMEM the handle keeps the workspace it had), counted by pnp_workspace_bytes.  A later call allocates only if it
 *   needs more than any call before it, and then waits for the device; every other call allocates nothing and is asynchronous.  Calls on one
 *   handle are stream-ordered.
 *
 * pnp_whiten_matrix, per matrix n, one workgroup, float64, the matrix on chip.  Only the lower triangle of Psi and the real part of its diagonal
 * are read.  Cholesky, column j = 0 .. C-1, every sum from 0.0 with k ascending and a conj(b) accumulated as
 * (re += ar br; re += ai bi; im += ai br; im -= ar bi):
 *     d       = Re Psi[j][j] - sum_{k<j} |L[j][k]|^2                      L[j][j] = sqrt(d)
 *     L[i][j] = (Psi[i][j] - sum_{k<j} L[i][k] conj(L[j][k])) / L[j][j]   (i > j; real and imaginary part each divided by the real L[j][j])
 *   W = L^-1 by forward substitution, column by column, i and k ascending, a b accumulated as (re += ar br; re -= ai bi; im += ar bi; im += ai br):
 *     W[j][j] = 1 / L[j][j]            W[i][j] = -(sum_{k=j}^{i-1} L[i][k] W[k][j]) / L[i][i]
 *   wmat and lmat are rounded to complex64 once, lower-triangular with exact +0 above the diagonal (and a zero below it stored as +0).
 *   info[n] = 0, or j + 1 for the first column whose pivot d is not finite, not positive or not greater than 1e-12 * max_i Re Psi[i][i]; that
 *   matrix's wmat and lmat are then the identity: a matrix that is not positive definite never produces NaN and needs no host read to be
 *   survived.  Psi = I gives W = L = I bit for bit.
 *   psi   : DEVICE complex128 [psi_n,C,C];   psi_n : 1..65535;   coils : 1..PNP_PW_MAX_COILS;   flags : reserved, must be 0
 *   wmat  : DEVICE complex64 [psi_n,C,C] out;   lmat : the same layout, L, or NULL;   info : DEVICE int32 [psi_n] out; none may alias another
 *   It allocates nothing and is asynchronous.
 *
 * pnp_whiten_apply:  out[n,v,p] = sum_{c = 0 .. v} wmat[n or 0][v][c] * in[n,c,p]  over all H W bins.  Only the lower triangle of wmat is read
 * (whatever lies above the diagonal is ignored, and coil c > v never enters row v).  The float32 arithmetic is that of pnp_coil_compress_apply:
 * from re = im = +0, c ascending, every product contracted:
 *     re = fma(a.re, x.re, re);  re = fma(-a.im, x.im, re);  im = fma(a.re, x.im, im);  im = fma(a.im, x.re, im)        (a = wmat[v][c], x = in[c])
 * so for coils <= 32 the result equals pnp_coil_compress_apply(in, wmat, out_coils = coils) bit for bit when wmat is zero above the diagonal,
 * the identity copies the planes, and a bin that is zero in every coil stays zero.  The bits do not depend on which kernel variant runs.
 *   in     : DEVICE complex64 [N,C,H,W];   coils : 1..PNP_PW_MAX_COILS
 *   wmat   : DEVICE complex64 [wmat_n,C,C];   wmat_n : 1 (one matrix for all slices) or N;   must not overlap in or out
 *   out    : DEVICE complex64 [N,C,H,W]; out == in (exactly) runs IN PLACE: row v needs coils 0..v only, and a thread reads all coils of its
 *            pixels before it stores any row.  Any other overlap of in and out is refused.
 * Each input value comes from memory once: 16 coils bytes per pixel (8 read, 8 written), in place or not, no workspace, asynchronous.
 *
 * All three take any handle kind and change neither the handle's mode nor its installed constants; pnp_whiten_apply needs n <= 65535.  Every
 * argument error (null handle or pointer, a count out of range, flags != 0, forbidden aliasing) is reported with PNP_ERR_INVALID and a message
 * naming the argument, before any HIP call, and leaves the outputs untouched. */
#define PNP_PW_MAX_COILS 64
int pnp_noise_cov(pnp_handle h, const float* noise, int noise_n, int coils, int samples, int flags, double* psi, void* stream);
int pnp_whiten_matrix(pnp_handle h, const double* psi, int psi_n, int coils, int flags, float* wmat, float* lmat /* may be NULL */,
                      int32_t* info, void* stream);
int pnp_whiten_apply(pnp_handle h, const float* in, int coils, const float* wmat, int wmat_n, float* out, void* stream);

/* ESPIRiT coil sensitivity maps: the maps as the dominant eigenvector, per pixel, of an operator built from the null space of the calibration
 * matrix, instead of the band-limited low-resolution estimate of pnp_estimate_sens (the reference has no counterpart).  Per slice, with the
 * centred acs_h x acs_w block B of pnp_estimate_sens, kernel side k = ksize, C = coils, n = C k^2, D = 2 k - 1:
 *   Calibration Gram matrix.  The rows of A are all (acs_h - k + 1)(acs_w - k + 1) sliding k x k x C windows of the block,
 *     A[(wy, wx)][(a, iy, ix)] = B[a][wy + iy][wx + ix], column index a k^2 + iy k + ix;  G = A^H A (n x n Hermitian).  The terms are the float32
 *     components of y0, their products are exact in float64, and every entry of the lower triangle is summed in float64 over the windows in
 *     row-major window order (re += xr yr; re += xi yi; im += xr yi; im -= xi yr for conj(x) y), one thread per entry, then mirrored; the diagonal
 *     is real.  No atomics.
 *   Eigen-decomposition.  G = V diag(lambda) V^H by the cyclic Jacobi method of pnp_coil_compress_matrix in float64: the same rotation formula,
 *     round-robin order and two-phase round, the same stop rule off(G)_F <= 1e-14 trace(G) before every sweep, at most 40 sweeps (the 64- to
 *     288-column matrices of the tests stop after 11 to 13).  One workgroup per slice; G and the vectors live in the slice's workspace in device
 *     memory (n is padded to even).  The signal space is {j : lambda_j > sv_thresh^2 lambda_0}, lambda_0 the largest eigenvalue; its size nkept is
 *     found on the device, no host read.  Only the projector P = V_kept V_kept^H enters what follows, so neither the order nor the phase of the
 *     vectors matters (no sort or phase step is run) and clustered eigenvalues leave the result well defined.
 *   Kernel auto-correlation.  R[a][b][d] = (1 / k^2) sum over {i - j = d} of conj(P[(a, i), (b, j)]), d over the D x D offsets: summed in float64
 *     (kept vectors in index order, inside them the pairs in (iy, ix) order), divided by k^2 and rounded to complex64 ONCE: kern.
 *   Per-pixel matrix.  With the centred pixel q = (py - H/2, px - W/2):  G_q[a][b] = sum_d R[a][b][d] exp(+2 pi i (dy qy / H + dx qx / W)), C x C
 *     Hermitian; with this sign and normalisation the true map vector S(q) is an eigenvector of G_q with eigenvalue 1.  float32 from here on: the
 *     twiddles are the float64 values of exactly reduced arguments (dy qy mod H, dx qx mod W in integers) rounded to float32 once; d_y is contracted
 *     first (dy ascending), then d_x (dx ascending), every complex product-sum as four fused multiply-adds from +0; only b <= a is formed, the
 *     upper triangle is its conjugate and the diagonal's imaginary part is dropped.
 *   Dominant eigenpair.  iters power steps v <- G_q v / ||G_q v|| (the squared norm by fused multiply-adds in coil order, one square root, one
 *     IEEE reciprocal, a product per component; a zero G_q v gives v = 0) from v = l / rss, where l_c = ifft_c(win * block) and rss are the
 *     low-resolution coil images and their root-sum-of-squares exactly as in pnp_estimate_sens (same window argument; rss = 0 gives v = 0 and
 *     zero maps).  eval = lambda(q) = Re(v^H G_q v) after the last step.  A fixed count: no data-dependent branch.
 *   Phase.  This engine keeps a real iterate, so the maps absorb the object's phase as the low-resolution maps do:  p = sum_c conj(v_c) l_c,
 *     phi = p / |p| (1 when p is exactly 0), S_c = v_c phi.  (Not the usual "coil 0 real" convention, which would leave a complex image.)
 *   Kept set.  sens_c = S_c where lambda(q) > float32(crop) and rss > 0 and rss > float32(thresh) * smax_n (rss, smax_n of pnp_estimate_sens), else
 *     0; thresh = 0 leaves only the crop rule.  On the kept set sum_c |S_c|^2 = 1 to float32 rounding.
 *   y0     : DEVICE complex64 [N,C,H,W], centred layout; read inside the block only: the block must be fully sampled
 *   coils  : 1..PNP_ESPIRIT_MAX_COILS (acquisitions with more channels compress first: pnp_coil_compress_*);   ksize : 2..PNP_ESPIRIT_MAX_KSIZE;
 *            coils * ksize^2 <= PNP_ESPIRIT_MAX_N;   acs_h, acs_w : even, ksize <= acs_h <= H, ksize <= acs_w <= W.  A block with fewer windows
 *            than n calibrates badly (the Gram matrix is rank deficient and the signal space is not separated)
 *   sv_thresh : in (0, 1);   crop : in [0, 1);   iters : 1..64;   window, thresh : as pnp_estimate_sens;   flags : reserved, must be 0
 *   sens   : DEVICE complex64 [N,C,H,W] out, must not alias y0.  The window and inverse-transform launches of pnp_estimate_sens run in it first and
 *            the pixel kernel reads l_c from it and writes S_c to it in place: there is no [N,C,H,W] workspace
 *   eval   : DEVICE float32 [N,H,W] out, or NULL;   kern : DEVICE complex64 [N,C,C,D,D] out, or NULL;   nkept : DEVICE int32 [N] out, or NULL
 * Any handle kind; the call changes neither the handle's mode nor its installed constants.  Sizes the k-space stage accepts, n * coils <= 65535.
 * A slice's bits depend on its own y0 and the arguments only: not on N, its place in the batch, the stream or the handle kind; no atomics.
 * SETUP-TIME SEMANTICS, as pnp_coil_compress_matrix: the first call allocates the workspace of pnp_estimate_sens with a NULL rss
 * (4 n ceil(H W / 2048) + 4 n + 4 n H W bytes, unless an earlier call did) and n (32 np^2 + 8 C^2 D^2 + 8) bytes (np = C k^2 rounded up to even: G
 * and the vectors, R, nkept), inside the call, all-or-nothing (on PNP_ERR_NOMEM the handle keeps the workspace it had), counted by
 * pnp_workspace_bytes.  A later call allocates only if it needs more than any call before it, and then waits for the device; every other call
 * allocates nothing and is asynchronous.  Calls on one handle are stream-ordered.
 * Every argument error (null handle, y0 or sens, sens == y0, coils outside 1..16, ksize outside 2..8, coils * ksize^2 > 512, acs_h / acs_w odd,
 * below ksize or above the handle's H / W, sv_thresh outside (0, 1), crop or thresh outside [0, 1), iters outside 1..64, an unknown window,
 * flags != 0, n * coils > 65535) is reported before any HIP call and leaves the outputs untouched. */
#define PNP_ESPIRIT_MAX_COILS 16
#define PNP_ESPIRIT_MAX_KSIZE 8
#define PNP_ESPIRIT_MAX_N     512
int pnp_espirit_sens(pnp_handle h, const float* y0, int coils, int acs_h, int acs_w, int ksize, double sv_thresh, double crop, int iters,
                     int window, double thresh, int flags, float* sens, float* eval /* [N,H,W], may be NULL */,
                     float* kern /* complex64 [N,C,C,2k-1,2k-1], may be NULL */, int32_t* nkept /* [N], may be NULL */, void* stream);

/* GRAPPA: autocalibrated k-space interpolation, the k-space counterpart of the map-based stages above (the reference has no counterpart).  The
 * undersampled axis is W (whole columns, as cartesian_mask); the acquired columns are the integer comb x = offset (mod R), R = accel, W % R == 0,
 * plus a fully sampled centre.  A kernel of `by` rows (odd) by `bx` comb columns (2 or 4) synthesises the R - 1 missing columns to the right of a
 * comb column xa from their acquired neighbours in every coil.  Per slice, centred layout, C = coils:
 *     sources of (y, xa):  (c, y + i - by/2, xa + (j - (bx/2 - 1)) R),  i < by, j < bx;    index s = (c by + i) bx + j,    ns = C by bx
 *     targets of (y, xa):  (c', y, xa + r),  r = 1 .. R-1;                                 index t = c' (R-1) + (r-1),     nt = C (R-1)
 *   All targets of a comb column share its sources.
 *
 * pnp_grappa_weights, per slice n, with the centred acs_h x acs_w block B of pnp_estimate_sens (it must be fully sampled; y0 is read inside it only):
 *   Windows.  All (acs_h - by + 1)(acs_w - span + 1) window positions (wy, wx) of the block, span = (bx-1) R + 1, in row-major order; windows do
 *     not wrap.  A[w][s] = B[c][wy+i][wx+jR],  T[w][t] = B[c'][wy+by/2][wx+(bx/2-1)R+r],  Z = [A | T].
 *   Gram.  M[s][j] = sum_w conj(A[w][s]) Z[w][j], j < ns + nt: the float32 components multiplied and summed in float64 (the products are exact), one
 *     thread per entry walking the windows in order (re += xr yr; re += xi yi; im += xr yi; im -= xi yr for conj(x) y, the convention of
 *     pnp_espirit_sens).  For j < ns only j <= s is formed and mirrored: the left block G is exactly Hermitian, its diagonal real.  No atomics.
 *     gram, when not NULL, receives M before regularisation.
 *   Regularisation.  lam * trace(G) / ns is added to G's diagonal; the trace is summed in float64 with s ascending.
 *   Solve.  G X = Rh (Rh = the right block of M) by Cholesky and forward and back substitution, one workgroup per slice, float64, the matrix in the
 *     slice's workspace in device memory.  The factor by the column formulas of pnp_whiten_matrix (every sum from 0.0, k ascending); then per
 *     right-hand side  Y[i] = (Rh[i] - sum_{k<i} L[i][k] Y[k]) / L[i][i], i ascending, and  X[i] = (Y[i] - sum_{k>i} conj(L[k][i]) X[k]) / L[i][i],
 *     i descending, k ascending.
 *   info[n] = 0, or j + 1 for the first column whose pivot is not finite, not positive or not greater than 1e-12 * max_i (regularised) G[i][i] -
 *     the rule of pnp_whiten_matrix; that slice's wts are then all +0 (pnp_grappa_apply leaves its missing bins zero): no finite input gives
 *     NaN and no host read is needed.  An all-zero block gives info = 1.
 *   wts[n][t][s] = X[s][t], rounded to complex64 once.
 *   y0    : DEVICE complex64 [N,C,H,W];   coils : 1..PNP_GRAPPA_MAX_COILS;   accel : 2..PNP_GRAPPA_MAX_ACCEL, W % accel == 0
 *   by    : 1, 3, 5 or 7;   bx : 2 or 4;   coils * by * bx <= PNP_GRAPPA_MAX_SRC
 *   acs_h : even, by <= acs_h <= H;   acs_w : even, span <= acs_w <= W.  A block with fewer windows than ns is rank deficient before lam is added
 *   lam   : finite, in [0, 1];   flags : reserved, must be 0;   n * coils <= 65535
 *   wts   : DEVICE complex64 [N,nt,ns] out;   info : DEVICE int32 [N] out;   gram : DEVICE complex128 [N,ns,ns+nt] out, or NULL; none may alias another
 *   SETUP-TIME SEMANTICS, as pnp_coil_compress_matrix: the first call allocates 16 n ns (ns + nt) bytes (M) inside the call, all-or-nothing (on
 *   PNP_ERR_NOMEM the handle keeps the workspace it had), counted by pnp_workspace_bytes.  A later call allocates only if it needs more than any
 *   call before it, and then waits for the device; every other call allocates nothing and is asynchronous.  Calls on one handle are stream-ordered.
 *
 * pnp_grappa_apply, for every bin (y, x) of every coil c':
 *     out = y0 (the bits)                                   where mask[n or 0][y][x] != 0
 *         = y0 (the bits)                                   where x mod R == offset: the caller promises that the comb is sampled
 *         = sum over s ascending of wts[n or 0][t][s] * src_s   otherwise, with xa the comb column at or below x (periodically), r = x - xa
 *   Source indices are periodic, mod H in y and mod W in x: the comb of a width divisible by R is periodic, so every missing bin has full support.
 *   float32 from re = im = +0 with the fused multiply-add chain of pnp_coil_compress_apply:
 *     re = fma(a.re, x.re, re);  re = fma(-a.im, x.im, re);  im = fma(a.re, x.im, im);  im = fma(a.im, x.re, im)        (a = wts[t][s], x = src_s)
 *   so a one-hot weight copies its source plane, shifted.  The bits do not depend on which kernel variant runs.
 *   mask  : DEVICE u8 [mask_n,H,W], centred;   mask_n : 1 or N;   wts : DEVICE complex64 [wts_n,nt,ns];   wts_n : 1 or N;   0 <= offset < accel
 *   out   : DEVICE complex64 [N,C,H,W]; must not overlap y0, wts or mask (neighbouring bins read y0)
 *   It does 8 ns real operations per synthesised value, allocates nothing and is asynchronous; n * coils <= 65535.
 *
 * Both calls take any handle kind and change neither the handle's mode nor its installed constants.  A slice's bits depend on its own input and
 * the arguments only: not on N, its place in the batch, the stream or the handle kind; no atomics.  Every argument error (null handle or pointer,
 * a count or size out of range, flags != 0, forbidden aliasing) is reported with PNP_ERR_INVALID and a message naming the argument, before any
 * HIP call, and leaves the outputs untouched. */
#define PNP_GRAPPA_MAX_COILS 32
#define PNP_GRAPPA_MAX_ACCEL 8
#define PNP_GRAPPA_MAX_SRC   512
int pnp_grappa_weights(pnp_handle h, const float* y0, int coils, int acs_h, int acs_w, int accel, int by, int bx, double lam, int flags,
                       float* wts /* complex64 [N,nt,ns] */, int32_t* info /* [N] */,
                       double* gram /* complex128 [N,ns,ns+nt], may be NULL */, void* stream);
int pnp_grappa_apply(pnp_handle h, const float* y0, int coils, const uint8_t* mask, int mask_n, int accel, int offset, int by, int bx,
                     const float* wts, int wts_n, float* out /* complex64 [N,C,H,W] */, void* stream);

/* ---- tree search support --------------------------------------------------------------------- */

/* Replaces: the per-child copy of `states` in expand_tree (evaluation/mcts.py:118-128), which the reference gets for
 * free because every op in PnPEnv.step allocates fresh tensors (evaluation/env.py:85-93); here x/z/u are updated in
 * place, so a node keeps its iterate as ONE packed device buffer: [x f32 N*H*W | z c64 N*H*W | u c64 N*H*W | t f32 N].
 * The episode's k-space constants (pnp_reset) are shared by all nodes and not part of a snapshot.
 * t_state may be NULL (zeros are stored / nothing restored).  Copies are asynchronous on `stream`. */
size_t pnp_snapshot_bytes(pnp_handle h);
int pnp_snapshot(pnp_handle h, const float* x, const float* z, const float* u, const float* t_state, void* dst,
                 void* stream);
int pnp_restore(pnp_handle h, const void* src, float* x, float* z, float* u, float* t_state, void* stream);

/* ---- introspection --------------------------------------------------------------------------- */

/* Copy one internal activation of the LAST denoiser forward to `dst` (DEVICE float32, NCHW
 * [N,C,h,w]) for per-stage parity tests.  which: 0..8 = stage outputs inc, down1..4, up1..4
 * (the tensors x1..x5, y1..y4 of evaluation/noise.py:120-128).  Returns C,h,w via out params.  Stage 8 (y4) is only
 * materialised on handles created with PNP_FLAG_KEEP_STAGES. */
int pnp_unet_read_stage(pnp_handle h, int which, float* dst, int* c, int* hh, int* ww, void* stream);

/* Kernel-level timing (PNP_FLAG_PROFILE).  After the stream has been synchronised by the caller,
 * pnp_profile_collect() folds the recorded event pairs into per-kernel-class totals.
 * classes: 0 conv3x3_mfma, 1 conv_first (2->32, VALU), 2 conv_last (1x1 + residual + clamp),
 *          3 fft_rows, 4 fft_cols_prox, 5 other.  Arrays of length PNP_PROFILE_CLASSES. */
#define PNP_PROFILE_CLASSES 6
int pnp_profile_reset(pnp_handle h);
int pnp_profile_collect(pnp_handle h, double* total_ms, int64_t* launches);
/* per-conv-layer totals (28 entries, execution order); handles created with PNP_FLAG_PROFILE_LAYERS only */
int pnp_profile_layers(pnp_handle h, double* layer_ms, int64_t* layer_launches);

/* Which kernel each of the 28 conv layers runs on for this handle's problem size (fixed at pnp_create):
 * 0 direct MFMA conv, 1 Winograd F(2x2,3x3) MFMA conv (executes 16/36 of the direct multiplies), 4 Winograd F(4x4,3x3)
 * MFMA conv (36/144), 2 VALU first layer, 3 last layer (fused into layer 26's epilogue or its own kernel), 5 direct bf16
 * MFMA conv in producer / consumer form (PNP_FLAG_BF16_CONVS handles on chip-filling problems). */
int pnp_conv_algorithms(pnp_handle h, int32_t* algo28);

/* Which schedule of the F(4x4,3x3) arithmetic each of the 28 conv layers runs (fixed at pnp_create; dt4image_restoration_amd/csrc/
 * winograd4_kernels.hip): 0 the layer is not on F(4x4), 1 all waves in step (32 tiles; the 32-channel variant too), 2 the two tile
 * halves half a chunk apart, 3 16-tile M-blocks in two independent workgroups per CU, 4 cout-split (16 tiles x 128 channels). */
int pnp_conv_schedules(pnp_handle h, int32_t* sched28);

/* bf16 terms per conv weight on this handle: 0 (f32 handle), 2 (PNP_FLAG_BF16_CONVS), 1 (... with PNP_BF16_W1). */
int pnp_bf16_weight_terms(pnp_handle h);

/* Engine workspace size in bytes (device memory owned by the handle). */
size_t pnp_workspace_bytes(pnp_handle h);

#ifdef __cplusplus
}
#endif
#endif /* PNPADMM_H */
