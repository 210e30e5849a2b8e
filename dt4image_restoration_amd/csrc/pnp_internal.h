// Internal declarations shared by the HIP translation units of libpnpadmm.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <atomic>
#include <vector>

namespace pnp {

// Experiment / test overrides, read from the environment ONCE per handle (pnp_create) and stored with it, so the plan a
// layer's weights were packed for is the plan every later launch uses.
struct Tuning {
    int wino_min_cin = 32;        // PNP_WINO_MIN_CIN
    long wino_min_blocks = 192;   // PNP_WINO_MIN_BLOCKS (tests force 1: Winograd on small problems too)
    bool wino_big = false;        // PNP_WINO_BIG_GROUPS: the 8-wave plans everywhere
    bool wino_small = false;      // PNP_WINO_SMALL_GROUPS
    bool no_wino = false;         // PNP_NO_WINOGRAD
    int f4_min_cin = 32;          // PNP_WINO_F4_MIN_CIN: F(4x4,3x3) for layers with at least this many input channels
    bool no_f4 = false;           // PNP_NO_WINO_F4
    bool no_f4_fused_first = false;// PNP_NO_F4_FUSED_FIRST: the first layer as its own kernel (conv_first_kernel)
    bool no_f4_fused_last = false;// PNP_NO_F4_FUSED_LAST: up4.conv-2 (+ fused last layer) on the F(2x2) kernel
    bool no_f4_phased = false;    // PNP_NO_WINO_F4_PHASED: every F(4x4) layer on the all-waves-in-step schedule
    int f4_mt16 = 0;              // PNP_WINO_F4_MT16 (experiments): 0 = default rule, 1 = never, 2 = upsample+concat layers only, 3 = every
                                  // 64-channel-block layer on 16-tile M-blocks
    bool bf16_no_ws = false;      // PNP_BF16_NO_WS (ablation): bf16 mode without the producer / consumer kernel (the round-2 kernel everywhere)
    bool bf16_f32_acts = false;   // PNP_BF16_F32_ACTS (ablation): bf16 mode keeps every activation in f32, as rounds 1-2 did
    bool bf16_no_holdhi = false;  // PNP_BF16_NO_HOLDHI (ablation): the 32 -> 32 layers of the bf16 mode stream their weights instead of holding them
    bool bf16_w1 = false;         // PNP_BF16_W1 (ablation): bf16 mode with ONE bf16 term per weight (the round-3 arithmetic: 0.015 dB of
                                  // PSNR drift against the f32 reference over configs[4]'s 50 iterations) instead of hi + lo
    int f4_cs = 1;                // PNP_WINO_F4_CS: the cout-split F(4x4) schedule (16 tiles x 128 channels per workgroup, conv3x3_wino4c_kernel):
                                  // 0 = never, 1 = the default rule (winograd_plan), 2 = every layer the schedule can take
    int f4_order = 1;             // PNP_WINO_F4_ORDER (experiments): 0 = spatial tiles dealt round-robin over the XCDs (rounds 1-2)
    int slice128_min_n = 192;     // PNP_SLICE128_MIN_N: 128 x 128 slices take the one-workgroup-per-slice data-fidelity kernel from
                                  // this batch size on (measured: one workgroup per slice is LDS-bound on its CU - 46 us a slice - so it
                                  // needs a chip-filling batch to beat the three-launch path: 64.1 vs 78.8 us at 256 slices, 48.9 vs 34.9 at 64)
    bool tv_naive = false;        // PNP_TV_NAIVE (tests): the TV prior as one launch per iteration instead of the fused kernel
    bool haar_naive = false;      // PNP_HAAR_NAIVE (tests): the Haar TI prior as one launch per level instead of the fused kernel
    int ncsense_block = 0;        // PNP_NCSENSE_COIL_BLOCK (tests, timing): coils per block of the non-Cartesian SENSE stage, 1..32 (else: kNcsenseBlock)
    int ncsense_naive = -1;       // PNP_NCSENSE_NAIVE (tests, timing): 1 = every step of that stage as the single-coil launches between an expand and a
                                  // combine kernel, 0 = every step coil-batched; unset: kNcsenseNaiveSteps, the choice per step by measurement
    bool toeplitz_naive = false;  // PNP_TOEPLITZ_NAIVE (tests, timing): the Toeplitz normal operator as its seven composed launches instead of the fused three
    int offres_block = 0;         // PNP_OFFRES_SEG_BLOCK (tests, timing): segments per block of the off-resonance operator, 1..32 (else: kOffresBlock)
    bool offres_grid_filter = false;   // PNP_OFFRES_GRID_FILTER (timing): the two-segment gridding filters the tile's whole bin per segment
                                  // instead of walking the plan's per-(segment, tile) list; the same numbers
    bool fieldmap_naive = false;  // PNP_FIELDMAP_NAIVE (tests, timing): the field map fit as one launch per sweep instead of the fused kernel
    int offres_naive = -1;        // PNP_OFFRES_NAIVE (tests, timing): 1 = the operator composed from the non-Cartesian SENSE launches and two sample
                                  // kernels, 0 = the two-segment gather and gridding; unset: kOffresNaiveSteps, the choice per step by measurement
    int offres_ls_naive = -1;     // PNP_OFFRES_LS_NAIVE (tests, timing): the same choice under a least-squares plan; unset: kOffresLsNaiveSteps
    bool offres_ls_noskip = false;   // PNP_OFFRES_LS_NOSKIP (timing): the dense gridding without its wave-uniform row skip; the same numbers
    int offres_mc_block = 0;      // PNP_OFFRES_MC_COIL_BLOCK (tests, timing): coils per block of the multi-coil off-resonance operator, 1..32
                                  // (else: kOffresMcBlock)
    int offres_mc_naive = -1;     // PNP_OFFRES_MC_NAIVE (tests, timing): 1 = that operator composed per coil from the single-coil operator between
                                  // an expand and a combine kernel, 0 = the fused pad and crop; unset: kOffresMcNaiveSteps
    bool offres_tz_naive = false; // PNP_OFFRES_TZ_NAIVE (tests, timing): the Toeplitz form of the off-resonance operator composed on full 2H x 2W
                                  // planes instead of the fused passes
    int offres_tz_slices = 0;     // PNP_OFFRES_TZ_SLICE_BLOCK (tests): slices per block of that application (else: kOffresTzPlanes / L); no bit
                                  // depends on it
};
Tuning tuning_from_env();

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) must be applied once per DEVICE (the attribute lives with the device's
// code object), not once per process: one bit per device ordinal.
struct DeviceOnce { std::atomic<uint64_t> mask{0}; };
hipError_t raise_lds_cap(const void* fn, int bytes, DeviceOnce& once);

// ---- denoiser conv layer description (mirrors dt4image_restoration_amd/unet_spec.py) ----------
enum SrcMode : int { SRC_PLAIN = 0, SRC_SIGMA = 1, SRC_POOL = 2, SRC_UPCAT = 3, SRC_FIRST = 4 };   // FIRST: F(4x4) 32-channel variant only

struct LayerSpec {
    int cin, cout, ksize, level, src, cskip;
};
static constexpr int N_LAYERS = 28;
extern const LayerSpec kLayers[N_LAYERS];

// Arguments of one conv3x3 MFMA launch.  Activations are NHWC float32.
struct ConvArgs {
    const float* src0;   // PLAIN: [N,H,W,Cin]; POOL: [N,2H,2W,Cin]; UPCAT: skip [N,H,W,Cskip]
    const float* src1;   // UPCAT: low-res [N,H/2,W/2,Cin-Cskip]; else unused
    const float* wpack;  // packed weights, see pack_conv3x3_weights()
    const float* bias;   // [Cout]
    float* dst;          // [N,H,W,Cout]
    float* pooled;       // optional: also write MaxPool2d(2) of the output, [N,H/2,W/2,Cout] (H, W even)
    // optional fused last layer (1x1 conv 32 -> 1 + image residual + clamp), Cout = 32 LDS-epilogue plan only:
    const float* last_w; const float* last_b; const float* last_ximg; const float2* last_z; const float2* last_u; float* last_out;
    // optional fused FIRST layer (SRC_FIRST: sigma-plane cat + conv 2 -> 32 + LeakyReLU computed into the patch; the image channel comes
    // from last_ximg or Re(last_z - last_u)): raw [32][18] weights, [32] bias, [N] sigma
    const float* first_w; const float* first_b; const float* first_sigma;
    float* partial;      // split-K workspace, conv3x3_partial_floats() floats (small problems only)
    const float* tact;   // [N] stop actions or nullptr; slice skipped when tact[n] > 0.5
    int N, H, W;         // OUTPUT spatial size
    int Cin, Cskip, Cout;
    int tilesX, tilesY;  // filled by launch_conv3x3 from the plan
    float rh, rw;        // UPCAT: (H/2-1)/(H-1), (W/2-1)/(W-1)  (bilinear align_corners=True scale)
    int bf16;            // bf16 MFMA operands (wpack = pack_conv3x3_weights_bf16), f32 accumulate: 0 = off, 2 = weights as two bf16 terms
                         // hi + lo (the mode's default), 1 = one term (PNP_BF16_W1)
    int act16;           // bf16 mode, 32-channel plan: bit 0 = src0 (PLAIN source / UPCAT skip) holds bf16, 2 B per channel; bit 1 = dst too;
                         // bit 2 = the pooled copy is written as bf16 (producer / consumer kernel's OFFLOAD store only)
    int order;           // F(4x4): blockIdx -> tile order (wino4_decode), from the plan
#ifdef PNP_STAMPS
    int stamp_slot;      // diagnostic build: launch index into the stamp buffer (winograd_kernels.hip)
#endif
#ifdef PNP_DIAG
    int diag;            // diagnostic build (`make diag`, timing only, results wrong): bit 0 = the F(4x4) epilogue's global stores are dropped
                         // (descriptor of zero records: same instruction stream), bit 1 = every workgroup stages the patch of tile 0 of
                         // slice 0 (L2 hits instead of HBM reads).  Set per launch from PNP_DIAG_L0 for the level-0 layers: the compute-only
                         // time of a layer = what a fused conv-1 -> conv-2 pair could at best pay per layer (profiles/r04_level0_bound.md)
#endif
};

// Launch the conv3x3 (+bias +LeakyReLU 0.2) implicit-GEMM kernel matching `a` (picks the tile shape
// from W and Cout).  Returns hipSuccess or the launch error.
// Tile plan of a conv3x3 launch (picked from the problem size and Cout).
struct ConvPlan {
    int tw, th;        // pixel tile
    int bm, bn;        // pixels / output channels per workgroup tile
    int mt, nt, wm, wn; // M-/N-blocks (32x32) per wave; wave grid
    int ck;            // input channels per staged chunk (16 or 32)
    int splitk;        // K ranges (of whole chunks), one workgroup each; > 1 only on small problems
    int ws;            // bf16 mode: the producer / consumer kernel (conv_bf16_kernels.hip) runs this layer; ck = 32
    int holdhi = 1;    // ws, 32 -> 32 layers under two-term weights: both weight fragments of every k-step held in registers (Tuning.bf16_no_holdhi)
    int tiles_x, tiles_y;
};
ConvPlan conv3x3_plan(int N, int H, int W, int Cin, int Cout, bool bf16 = false, int src_mode = SRC_PLAIN, bool allow_ws = true);
hipError_t launch_conv3x3_bf16ws(const ConvArgs& a, const ConvPlan& p, int src_mode, hipStream_t s);
size_t conv3x3_partial_floats(const ConvPlan& p, int N, int H, int W, int Cout);
bool conv3x3_pooled_output_ok(const ConvPlan& p);
bool conv3x3_tensor_fits(int N, int H, int W, int Cin, int Cout);   // whole-tensor buffer descriptors: < 2 GiB per activation tensor
hipError_t launch_conv3x3(const ConvArgs& a, const ConvPlan& p, int src_mode, hipStream_t s);

// Host-side repack of OIHW conv3x3 weights into the per-lane MFMA B-fragment stream (chunk size ck from the
// layer's plan).  dst must hold conv3x3_pack_floats(cin, cout) floats.
size_t conv3x3_pack_floats(int cin, int cout);
void pack_conv3x3_weights(const float* oihw, int cin, int cout, int ck, float* dst);
size_t conv3x3_pack_floats_bf16(int cin, int cout, int terms);
void pack_conv3x3_weights_bf16(const float* oihw, int cin, int cout, int ck, int terms, float* dst);

// Winograd F(2x2,3x3) path for the K-heavy layers (winograd_kernels.hip).
struct WinoPlan {
    bool use;          // layer is eligible (long K, enough workgroups)
    int algo;          // 1: F(2x2,3x3) (winograd_kernels.hip), 4: F(4x4,3x3) (winograd4_kernels.hip)
    int tw, th, bn, wm, wn, ck, tiles_x, tiles_y;
    int stack;         // F(4x4) on 16 x 16 images: two slices stacked into one 32-tile workgroup
    int mt;            // F(4x4): tiles per workgroup (32, or 16 = two independent 4-wave workgroups per CU)
    int phased;        // F(4x4), 64-channel blocks, plain source: the two tile halves run half a chunk apart (conv3x3_wino4p_kernel)
    int cs;            // F(4x4), Cout % 128 == 0: one 16-tile M-block x 128 channels per workgroup (conv3x3_wino4c_kernel); bn = 128, mt = 16
    int order;         // F(4x4): 1 = every XCD walks a contiguous range of spatial tiles (halo pixels shared through its L2), 0 = tiles dealt round-robin
};
// `src_mode` = the source mode the layer will be LAUNCHED with (a POOL layer whose producer writes the pooled copy runs PLAIN)
// `Cskip`: channels an upsample + concat layer takes from its skip tensor (0: unknown - such a layer is then not planned on the cout-split schedule)
WinoPlan winograd_plan(int N, int H, int W, int Cin, int Cout, int src_mode, const Tuning& t, int Cskip = 0);
bool upsample_lines_regular(int H);   // winograd4_kernels.hip: the x2 upsample to H rows reads lines floor((g - 1) / 2), + 1 in float32 too
size_t winograd4_pack_floats(int cin, int cout);
void pack_winograd4_weights(const float* oihw, int cin, int cout, int ck, float* dst);
hipError_t launch_conv3x3_winograd4(const ConvArgs& a, const WinoPlan& p, int src_mode, hipStream_t s);
size_t winograd_pack_floats(int cin, int cout);
void pack_winograd_weights(const float* oihw, int cin, int cout, int ck, float* dst);
hipError_t launch_conv3x3_winograd(const ConvArgs& a, const WinoPlan& p, int src_mode, hipStream_t s);

// First layer (2 -> 32, K = 18: too thin for MFMA, direct VALU) and last layer (1x1 32 -> 1 fused
// with the residual add and clamp).  `ximg` (f32 [N,H,W]) or, when null, Re(z-u) of complex64 z,u
// is the image channel.
hipError_t launch_conv_first(const float* ximg, const float2* z, const float2* u, const float* sigma,
                             const float* tact, const float* w, const float* bias, float* dst,
                             int N, int H, int W, hipStream_t s, bool dst_bf16 = false);
hipError_t launch_conv_last(const float* act, const float* ximg, const float2* z, const float2* u,
                            const float* tact, const float* w, const float* bias, float* out,
                            int N, int H, int W, hipStream_t s);
hipError_t launch_nhwc_to_nchw(const float* src, float* dst, int N, int C, int H, int W, hipStream_t s);

// ---- FFT / data-fidelity stage -----------------------------------------------------------------
struct FftPlan {
    int h, w;
    float2* tw_h;   // device: exp(-2 pi i m / h), m < h
    float2* tw_w;
};

bool kspace_len_ok(int L);   // 16 <= L <= 1024, 16 | L, L = 2^a * 5^b
// The six k-space passes.  Each picks its kernel family itself: the power-of-two kernels (fft_kernels.hip), or the mixed-radix ones
// (fft_mixed_kernels.hip) for a handle with a side that is not a power of two - one rule, stated in fft_kernels.hip (mixed_radix).
// generic passes, in place or not; shift: the index shift on load and on store (0: the plain transform, L / 2: the centred one of pnp_fft2c)
hipError_t launch_fft_rows(const float2* in, float2* out, const float2* tw, int batch, int H, int W, int inverse, int shift, hipStream_t s);
hipError_t launch_fft_cols(float2* data, const float2* tw, int batch, int H, int W, int inverse, int shift, hipStream_t s);
// row pass of a REAL image into complex scratch, no index shift (the first half of the plain transform of an image)
hipError_t launch_fft_rows_real(const float* x, float2* work, const float2* tw, int N, int H, int W, hipStream_t s);
// ADMM passes
hipError_t launch_fft_rows_fwd_admm(const float* x, const float2* u, float2* work, const float2* tw, const float* tact, int N, int H, int W,
                                    hipStream_t s);
hipError_t launch_fft_cols_prox(float2* work, const float2* tw, const float2* y0s, const uint8_t* masks, int mask_n, const float* mu,
                                const float* tact, int N, int H, int W, hipStream_t s);
hipError_t launch_fft_rows_inv_admm(const float2* work, const float* x, float2* z, float2* u, const float2* tw, const float* tact, int N,
                                    int H, int W, hipStream_t s);
// the mixed-radix family behind them (fft_mixed_kernels.hip), same arguments: for the dispatch only
namespace mixed {
hipError_t launch_fft_rows(const float2* in, float2* out, const float2* tw, int batch, int H, int W, int inverse, int shift, hipStream_t s);
hipError_t launch_fft_cols(float2* data, const float2* tw, int batch, int H, int W, int inverse, int shift, hipStream_t s);
hipError_t launch_fft_rows_real(const float* x, float2* work, const float2* tw, int N, int H, int W, hipStream_t s);
hipError_t launch_fft_rows_fwd_admm(const float* x, const float2* u, float2* work, const float2* tw, const float* tact, int N, int H, int W,
                                    hipStream_t s);
hipError_t launch_fft_cols_prox(float2* work, const float2* tw, const float2* y0s, const uint8_t* masks, int mask_n, const float* mu,
                                const float* tact, int N, int H, int W, hipStream_t s);
hipError_t launch_fft_rows_inv_admm(const float2* work, const float* x, float2* z, float2* u, const float2* tw, const float* tact, int N,
                                    int H, int W, hipStream_t s);
}  // namespace mixed

// x0 / x / z / u may all be null: only the episode constants (y0s, masks) are rebuilt
// 128 x 128 only: the whole stage (both transforms each way, the solve, the dual update) in one workgroup per slice
hipError_t launch_admm_slice128(const float* x, float2* z, float2* u, const float2* tw, const float2* y0s,
                                const uint8_t* masks, int mask_n, const float* mu, const float* tact, int N, hipStream_t s);

// x0 / x / z / u may all be null: only the episode constants (y0s, masks) are rebuilt
hipError_t launch_reset(const float2* x0, const float2* y0, const uint8_t* mask, int mask_n, float* x, float2* z,
                        float2* u, float2* y0s, uint8_t* masks, int N, int H, int W, hipStream_t s);
hipError_t launch_finish(const float* tact, float* tstate, uint8_t* done, int N, hipStream_t s);
hipError_t launch_psnr(const float* x, const float* gt, float* out, int N, int HW, hipStream_t s);

// ---- metrics (metrics_kernels.hip) ---------------------------------------------------------------
static constexpr int kSsimMaxRadius = 16;
struct SsimArgs {
    const float* x;      // [N,H,W]
    const float* gt;     // [N,H,W]
    float* map;          // [N,H,W] or nullptr (no map store)
    double* partial;     // [N, ssim_tiles(H, W)] per-tile sums
    float* out;          // [N] mean of the map
    int H, W;
    int radius;          // 1..kSsimMaxRadius
    int clamp_x;         // clamp x to [0, 1] on load
    float c1, c2;
    float w[2 * kSsimMaxRadius + 1];   // normalised Gaussian taps (computed in double on the host), w[0 .. 2 radius]
};
int ssim_tiles(int H, int W);
hipError_t launch_ssim(const SsimArgs& a, int N, hipStream_t s);

// ---- ADMM residuals (residual_kernels.hip) ---------------------------------------------------------
// every partial buffer holds one entry per workgroup of pixel_chunks(H, W) (block_reduce.h) per slice
// partial: [N, pixel_chunks, 4] sums of |x - z|^2, |x - xp|^2, |z - zp|^2, |u - up|^2; xp == nullptr: only the first is formed (u, zp, up unread)
hipError_t launch_residual_tiles(const float* x, const float2* z, const float2* u, const float* xp, const float2* zp, const float2* up,
                                 double* partial, int N, int H, int W, hipStream_t s);
// fx: the plain orthonormal transform of x (unshifted), y0s / masks: the episode constants as reset_kernel stores them; dcpartial: [N, pixel_chunks]
hipError_t launch_misfit_tiles(const float2* fx, const float2* y0s, const uint8_t* masks, int mask_n, double* dcpartial, int N, int H, int W,
                               hipStream_t s);
hipError_t launch_residual_reduce(const double* partial, const double* dcpartial, int has_delta, int has_dc, float* out, int N, int H, int W,
                                  hipStream_t s);

// ---- simulated acquisition (acquire_kernels.hip) ---------------------------------------------------
// work: the plain orthonormal transform of gt (unshifted); mask, y0: centred layout.  Stores y0 and leaves sgn * S y0 in work (reset_kernel's y0s
// convention), whose plain inverse transform is ifft_c(y0).  Noise: synthetic._gauss of (seed + n, 9001 / 9003, centred pixel), float64.
// coils > 1 (pnp_acquire_mc): work / y0 hold N * coils planes, plane n * coils + c takes slice n's mask and the streams 9001 + 4 c / 9003 + 4 c
hipError_t launch_acquire_epilogue(float2* work, const uint8_t* mask, int mask_n, float2* y0, double sigma, uint64_t seed, int N, int H, int W,
                                   hipStream_t s, int coils = 1);
hipError_t launch_acquire_clamp(const float2* aty0, float2* x0, int N, int H, int W, hipStream_t s);

// ---- multi-coil (SENSE) data fidelity (sense_kernels.hip) -------------------------------------------
// Pointwise kernels around the plain FFT passes at batch N * C; work / ys: [N, C, H, W] complex, sens: [sens_n, C, H, W], masks: the rolled
// layout reset_kernel stores.  tact (or nullptr): slices with tact[n] > 0.5 are skipped.
hipError_t launch_sense_expand(const float2* src, const float* src_real, const float2* sens, int sens_n, int C, const float* tact, float2* work,
                               int N, int H, int W, hipStream_t s);                    // work = S_c . src (src_real != nullptr: a real image)
hipError_t launch_sense_mask(float2* work, const uint8_t* masks, int mask_n, int C, int N, int H, int W, hipStream_t s);
// q = sum_c conj(S_c) work (+ mu pv); partial ([N, chunks, 2], column 0) = Re<pv, q> per chunk; pv / partial may be nullptr
hipError_t launch_sense_combine(const float2* work, const float2* sens, int sens_n, int C, const float2* pv, const float* mu, const float* tact,
                                float2* q, double* partial, int N, int H, int W, hipStream_t s);
hipError_t launch_sense_cg_init(const float2* aty, const float* x, const float2* u, const float2* q, const float* mu, const float* tact, float2* r,
                                float2* pv, double* partial, int N, int H, int W, hipStream_t s);
// sc: [N, 8] float64 (rs, bb, alpha, beta, frozen); mode 0: rs, bb from the init partials, 1: alpha from Re<p, q>, 2: beta and rs from <r, r>
hipError_t launch_sense_scalar(const double* partial, int mode, const float* tact, double* sc, int N, int H, int W, hipStream_t s);
hipError_t launch_sense_cg_update(float2* z, float2* r, const float2* pv, const float2* q, const double* sc, const float* tact, double* partial,
                                  int N, int H, int W, hipStream_t s);
hipError_t launch_sense_cg_dir(const float2* r, float2* pv, const double* sc, const float* tact, int N, int H, int W, hipStream_t s);
hipError_t launch_sense_dual(const float* x, const float2* z, float2* u, const float* tact, int N, int H, int W, hipStream_t s);
hipError_t launch_sense_cgres(const double* sc, float* out, int N, hipStream_t s);
hipError_t launch_sense_misfit(const float2* fx, const float2* ys, const uint8_t* masks, int mask_n, int C, double* dcpartial, int N, int H, int W,
                               hipStream_t s);
hipError_t launch_sense_install(const float2* y, const uint8_t* mask, int mask_n, int C, float2* ys, float2* work, uint8_t* masks, int N, int H,
                                int W, hipStream_t s);
hipError_t launch_sense_iterate(const float2* x0, float* x, float2* z, float2* u, int N, int H, int W, hipStream_t s);

// ---- coil sensitivity maps from the calibration block (coilmap_kernels.hip) -------------------------
// Pointwise kernels around the plain inverse FFT passes at batch N * C, in place in the caller's map buffer sens: [N, C, H, W] complex.
// sens[n, c][k] = in block(S k) ? sgn[k] * win * y[n, c][S k] : 0 (plain bin k; y: centred layout, read inside the acs_h x acs_w block only)
hipError_t launch_coilmap_window(const float2* y, float2* sens, int acs_h, int acs_w, int hann, int N, int C, int H, int W, hipStream_t s);
// rss: [N, H, W] = sqrt(sum_c |l_c|^2) (float64 sum in coil order, one rounding); partial: [N, chunks] maxima of rss
hipError_t launch_coilmap_rss(const float2* l, int C, float* rss, float* partial, int N, int H, int W, hipStream_t s);
hipError_t launch_coilmap_max(const float* partial, float* smax, int N, int H, int W, hipStream_t s);   // smax: [N]
// l <- (rss > 0 and rss > thresh * smax[n]) ? l / rss : 0
hipError_t launch_coilmap_normalise(float2* l, int C, const float* rss, const float* smax, float thresh, int N, int H, int W, hipStream_t s);

// ---- coil compression (coilcomp_kernels.hip) --------------------------------------------------------
// The chunk rule of a Gram accumulation (hermitian.h), shared with the noise covariance: `count` samples (the block's bins, a scan's samples)
// are dealt to gram_chunks(count) workgroups, gram_chunk_len(count) consecutive samples each: kGramMinBins, or for counts above
// kGramMinBins * kGramMaxChunks the 32-multiple that gives at most kGramMaxChunks workgroups.
static constexpr int kGramMinBins = 1024, kGramMaxChunks = 64;
inline int gram_chunk_len(long long count) {
    const long long per = ((count + kGramMaxChunks - 1) / kGramMaxChunks + 31) / 32 * 32;
    return per < kGramMinBins ? kGramMinBins : (int)per;
}
inline int gram_chunks(long long count) { return (int)((count + gram_chunk_len(count) - 1) / gram_chunk_len(count)); }
// gram: [N, C, C] complex128 = sum over the centred acs_h x acs_w block of y_a conj(y_b); partial: [N, gram_chunks, C, C] complex128.  Two launches.
hipError_t launch_coilcomp_gram(const float2* y, int C, int acs_h, int acs_w, double2* partial, double2* gram, int N, int H, int W, hipStream_t s);
// cmat: [N, C, C] complex64, eig: [N, C] float32 from gram: one workgroup per slice
hipError_t launch_coilcomp_eig(const double2* gram, int C, float2* cmat, float* eig, int N, hipStream_t s);
// out[n, v] = sum_c cmat[n or 0][v][c] in[n, c], v < V; in: [N, C, H, W], out: [N, V, H, W]
hipError_t launch_coilcomp_apply(const float2* in, const float2* cmat, int cmat_n, int C, int V, float2* out, int N, int H, int W, hipStream_t s);

// ---- coil noise pre-whitening (prewhiten_kernels.hip) -----------------------------------------------
// psi: [noise_n, C, C] complex128 = (1 / S) sum_s n_a conj(n_b); noise: [noise_n, C, S]; partial: [noise_n, gram_chunks(S), C, C] complex128.  Two launches.
hipError_t launch_prewhiten_cov(const float2* noise, int noise_n, int C, int S, double2* partial, double2* psi, hipStream_t s);
// wmat, lmat (or nullptr): [psi_n, C, C] complex64 lower-triangular, info: [psi_n]; one workgroup per matrix
hipError_t launch_prewhiten_chol(const double2* psi, int psi_n, int C, float2* wmat, float2* lmat, int* info, hipStream_t s);
// out[n, v] = sum_{c <= v} wmat[n or 0][v][c] in[n, c]; in, out: [N, C, H, W]; out may be in
hipError_t launch_prewhiten_apply(const float2* in, const float2* wmat, int wmat_n, int C, float2* out, int N, int H, int W, hipStream_t s);

// ---- GRAPPA (grappa_kernels.hip) ---------------------------------------------------------------------
// ns = C by bx sources, nt = C (R - 1) targets.  ws: per slice M [ns][ns + nt] complex128 (the solve destroys it); gram: the same layout or nullptr
hipError_t launch_grappa_gram(const float2* y, int C, int acs_h, int acs_w, int R, int by, int bx, double2* ws, double2* gram, int N, int H, int W,
                              hipStream_t s);
// wts: [N, nt, ns] complex64, info: [N]; one workgroup per slice
hipError_t launch_grappa_solve(double2* ws, int ns, int nt, double lam, float2* wts, int* info, int N, hipStream_t s);
// out: [N, C, H, W]; the comb x = offset (mod R) and the bins of mask are copies of y0, the others are synthesised; out overlaps nothing
hipError_t launch_grappa_apply(const float2* y0, const uint8_t* mask, int mask_n, const float2* wts, int wts_n, float2* out, int C, int R,
                               int offset, int by, int bx, int N, int H, int W, hipStream_t s);

// ---- ESPIRiT coil maps (espirit_kernels.hip) --------------------------------------------------------
// np: the side of the calibration Gram matrix, n = C k^2 rounded up to even.  ws: per slice G [np][np] then the transposed vectors [np][np], complex128
inline int espirit_padded(int C, int k) { return (C * k * k + 1) & ~1; }
hipError_t launch_espirit_gram(const float2* y, int C, int acs_h, int acs_w, int k, double2* ws, int N, int H, int W, hipStream_t s);
hipError_t launch_espirit_eig(double2* ws, int C, int k, int N, hipStream_t s);              // one workgroup per slice; eigenvalues on G's diagonal
// kern: [N, C, C, 2k-1, 2k-1] complex64, nkept: [N]
hipError_t launch_espirit_kern(const double2* ws, int C, int k, double sv_thresh, float2* kern, int* nkept, int N, hipStream_t s);
// sens: [N, C, H, W], in the low-resolution coil images, out the maps; rss [N, H, W], smax [N] of the coil map kernels; eval [N, H, W] or nullptr
hipError_t launch_espirit_pixels(float2* sens, const float2* kern, const float* rss, const float* smax, int C, int k, int iters, float crop,
                                 float thresh, float* eval, int N, int H, int W, hipStream_t s);

// ---- total-variation prior (tv_kernels.hip) ---------------------------------------------------------
// The fused kernel's plan: kTvT iterations per launch over a kTvRegion^2 region, of which the kTvTile^2 tile is stored
static constexpr int kTvT = 10, kTvRegion = 128, kTvTile = kTvRegion - 2 * kTvT - 1;
struct TvArgs {
    const float* v;        // [N,H,W] input plane, or nullptr: Re z - Re u
    const float2* z;       // [N,H,W] complex planes of pnp_step, or nullptr
    const float2* u;
    const float* lam;      // [N]; the slice's weight is scale * lam[n]
    float scale;
    const float* tact;     // [N] stop actions or nullptr; slice skipped when tact[n] > 0.5
    const float2* p_in;    // [N,H,W] (py, px) of the iteration before, or nullptr: p = 0
    float2* p_out;         // [N,H,W] or nullptr (fused kernel: p is not stored)
    float* out;            // [N,H,W] or nullptr (fused kernel: no closing divergence)
    int H, W;
    int iters;             // fused kernel: iterations of this launch, 1..kTvT
    int tiles_x, tiles_y;  // filled by the launchers
};
hipError_t launch_tv_fused(TvArgs a, int N, hipStream_t s);   // a.iters iterations from p_in, then p_out and / or out
hipError_t launch_tv_iter(TvArgs a, int N, hipStream_t s);    // ONE iteration p_in -> p_out, a thread per pixel (p_in must not be p_out)
hipError_t launch_tv_close(TvArgs a, int N, hipStream_t s);   // out = clamp(v - lam div p_in); out may alias v

// ---- Haar wavelet prior (haar_kernels.hip) ----------------------------------------------------------
// The fused TI kernel's plan: a kHaarRegion^2 region per workgroup, of which the tile - the region minus the halo 2^J - 1 all round - is stored
static constexpr int kHaarRegion = 128, kHaarMaxLevels = 4;   // (PNP_HAAR_MAX_LEVELS: asserted equal in pnp_capi.hip)
inline int haar_tile(int levels) { return kHaarRegion - 2 * ((1 << levels) - 1); }
struct HaarArgs {
    const float* v;        // [N,H,W] input plane, or nullptr: Re z - Re u
    const float2* z;       // [N,H,W] complex planes of pnp_step, or nullptr
    const float2* u;
    const float* lam;      // [N]; the slice's threshold is scale * lam[n]
    float scale;
    const float* tact;     // [N] stop actions or nullptr; slice skipped when tact[n] > 0.5
    float* out;            // [N,H,W]; only the ORTHO kernel may be handed out == v
    int H, W;
    int levels;            // J: 1..kHaarMaxLevels
    int level;             // naive kernels: the level j of this launch
    const float* a_src;    // naive kernels: a_(j-1) [N,H,W], or nullptr: v (j = 1)
    float* a_dst;          // naive down: a_j
    const float* r_src;    // naive up: r_j, or nullptr: 0 (j = J)
    float* r_dst;          // naive up: r_(j-1) (j > 1; level 1 stores out)
    int tiles_x, tiles_y;  // filled by the launchers
};
hipError_t launch_haar_ti_fused(HaarArgs a, int N, hipStream_t s);   // the whole TI operator in one launch; out must not be v
hipError_t launch_haar_ti_down(HaarArgs a, int N, hipStream_t s);    // ONE level down, a thread per pixel: a_src -> a_dst
hipError_t launch_haar_ti_up(HaarArgs a, int N, hipStream_t s);      // ONE level up: (a_src, r_src) -> r_dst, or out at level 1 (out must not be v)
hipError_t launch_haar_ortho(HaarArgs a, int N, hipStream_t s);      // the whole ORTHO operator; out may alias v

// ---- non-Cartesian sampling (nufft_kernels.hip; the plan: nufft_plan.h) -------------------------------
// The uploaded plan: every pointer is device memory, laid out as NufftPlan's vectors
struct NufftDev {
    int h = 0, w = 0, gh = 0, gw = 0, width = 0, tiles_y = 0, tiles_x = 0;
    int64_t m = 0;           // 0: no plan
    int* i0 = nullptr;       // [2][M]
    float* wts = nullptr;    // [2 J][M]
    float* cy = nullptr;     // [h]
    float* cx = nullptr;     // [w]
    int* bin_off = nullptr;  // [tiles + 1]
    int* bin_idx = nullptr;
    float2* tw_gh = nullptr; // twiddles of the grid's sides
    float2* tw_gw = nullptr;
};
// grid [batch, gh, gw] = the zero-padded (cy cx) . image; src complex [batch, h, w], or src_real != nullptr: a real image, no complex copy
hipError_t launch_nufft_pad(const float2* src, const float* src_real, const NufftDev& P, float2* grid, int batch, hipStream_t s);
// q = (cy cx) . crop(grid) (+ mu pv); partial ([batch, pixel_chunks, 2], column 0) = Re<pv, q> per chunk, as launch_sense_combine; pv, mu, tact,
// partial may be nullptr
hipError_t launch_nufft_crop(const float2* grid, const NufftDev& P, const float2* pv, const float* mu, const float* tact, float2* q, double* partial,
                             int batch, hipStream_t s);
hipError_t launch_nufft_interp(const float2* grid, const NufftDev& P, float2* out, int batch, hipStream_t s);   // out: [batch, M]
// grid = the spread of w . y (w: [M] or nullptr), every grid point written; one workgroup per (tile, slice), no atomics
hipError_t launch_nufft_grid(const float2* y, const float* w, const NufftDev& P, float2* grid, int batch, hipStream_t s);
int nufft_sample_chunks(int64_t m);   // workgroups (= partials) per slice of the misfit pass
// partial: [N, nufft_sample_chunks(M)]; dcpartial: [N, pixel_chunks(h, w)] = (sum_m w_m |a - y|^2, 0, ..): launch_residual_reduce's DC input
hipError_t launch_nufft_misfit(const float2* a, const float2* y, const float* w, const NufftDev& P, double* partial, double* dcpartial, int N,
                               hipStream_t s);
// y [N, M] += sigma (g_re + i g_im): pnp_acquire's counter hash of (seed + n, 9001 / 9003, m)
hipError_t launch_nufft_noise(float2* y, double sigma, uint64_t seed, const NufftDev& P, int N, hipStream_t s);

// ---- non-Cartesian SENSE (ncsense_kernels.hip; the operator: include/pnpadmm_ncsense.h) ---------------
// A block of cb coils c0 .. c0 + cb - 1 of every slice per launch.  grid: [batch, cb, gh, gw]; sens: [sens_n, C, h, w], sens_n 1 or batch's n
static constexpr int kNcsenseBlock = 8;    // default coils per block (PNP_NCSENSE_COIL_BLOCK overrides it)
static constexpr int kNcsenseSub = 8;      // coils per workgroup of the gridding: its register sub-block
// the steps of the stage, as bits: which of them run as the naive launches.  Both forms give the same bits (include/pnpadmm_ncsense.h)
enum NcsenseStep : int { NS_PAD = 1, NS_GATHER = 2, NS_GRID = 4, NS_CROP = 8, NS_ALL = 15 };
// the shipped choice (profiles/ncsense_bench.json): a coil-batched kernel ships only where it is not slower than the launch it replaces
static constexpr int kNcsenseNaiveSteps = NS_GATHER | NS_GRID;
// grid[n, j] = the zero-padded (cy cx) . (S_(c0+j) . src[n]); src complex [batch, h, w], or src_real != nullptr: a real image
hipError_t launch_ncsense_pad(const float2* src, const float* src_real, const float2* sens, int sens_n, int C, int c0, int cb, const NufftDev& P,
                              float2* grid, int batch, hipStream_t s);
// out[n, oc0 + j] = the gather of grid[n, j]; out: [batch, ocs, M]
hipError_t launch_ncsense_interp(const float2* grid, const NufftDev& P, float2* out, int ocs, int oc0, int cb, int batch, hipStream_t s);
// grid[n, j] = the spread of w . y[n, yc0 + j] (y: [batch, ycs, M]; w: [M] or nullptr), every grid point written, no atomics
hipError_t launch_ncsense_grid(const float2* y, int ycs, int yc0, int cb, const float* w, const NufftDev& P, float2* grid, int batch, hipStream_t s);
// q (+)= sum_j conj(S_(c0+j)) . (cy cx) . crop(grid[n, j]): the first block (c0 == 0) starts from +0, a later one from q; the last block
// (c0 + cb == C) adds mu pv and leaves the partial sums of Re<pv, q> as launch_nufft_crop does (pv, mu, tact, partial may be nullptr)
hipError_t launch_ncsense_crop(const float2* grid, const float2* sens, int sens_n, int C, int c0, int cb, const NufftDev& P, const float2* pv,
                               const float* mu, const float* tact, float2* q, double* partial, int batch, hipStream_t s);
// the naive form (PNP_NCSENSE_NAIVE): img [batch, cb, h, w] = S_(c0+j) . src, for launch_nufft_pad at batch * cb planes; and launch_ncsense_crop's
// combine on the coil images [batch, cb, h, w] that launch_nufft_crop left
hipError_t launch_ncsense_expand(const float2* src, const float* src_real, const float2* sens, int sens_n, int C, int c0, int cb, const NufftDev& P,
                                 float2* img, int batch, hipStream_t s);
hipError_t launch_ncsense_combine(const float2* img, const float2* sens, int sens_n, int C, int c0, int cb, const NufftDev& P, const float2* pv,
                                  const float* mu, const float* tact, float2* q, double* partial, int batch, hipStream_t s);
// partial [N, C, nufft_sample_chunks(M)] at the block's coils = sum_m w_m |a[n, j] - y[n, c0 + j]|^2 per chunk; a: [N, cb, M], y: [N, C, M]
hipError_t launch_ncsense_misfit(const float2* a, const float2* y, const float* w, int C, int c0, int cb, const NufftDev& P, double* partial, int N,
                                 hipStream_t s);
// dcpartial: [N, pixel_chunks(h, w)] = (the slice's partials summed in (coil, chunk) order, 0, ..): launch_residual_reduce's DC input
hipError_t launch_ncsense_misfit_sum(const double* partial, int C, const NufftDev& P, double* dcpartial, int N, hipStream_t s);
// y [N, C, M] += sigma (g_re + i g_im): pnp_acquire's counter hash of (seed + n, 9001 + 4 c / 9003 + 4 c, m)
hipError_t launch_ncsense_noise(float2* y, double sigma, uint64_t seed, int C, const NufftDev& P, int N, hipStream_t s);

// ---- Toeplitz normal operator (toeplitz_kernels.hip; the operator: include/pnpadmm_toeplitz.h) ---------
static constexpr int kToeplitzTile = 32;   // outputs per side of a spectrum workgroup's tile: divides 2 L for every k-space side L
// K [2H, 2W] float32 from traj [M][2] float64 (ky, kx) and w [M] float32 or nullptr (1): the header's float64 Dirichlet sum, no atomics
hipError_t launch_toeplitz_spectrum(const double* traj, const float* w, int64_t m, int H, int W, float* K, hipStream_t s);
// grid [planes, 2H, 2W] = src [planes, H, W] in the centred window, zeros elsewhere
hipError_t launch_toeplitz_pad(const float2* src, float2* grid, int H, int W, int planes, hipStream_t s);
hipError_t launch_toeplitz_mul(float2* grid, const float* K, int H, int W, int planes, hipStream_t s);   // grid *= K per plane
// q = crop(grid) (+ mu pv by one fma, with partial ([planes, pixel_chunks, 2], column 0) = Re<pv, q> per chunk, as launch_nufft_crop); pv, mu,
// tact, partial may be nullptr
hipError_t launch_toeplitz_crop(const float2* grid, const float2* pv, const float* mu, const float* tact, float2* q, double* partial, int H, int W,
                                int planes, hipStream_t s);
// the fused application (fft_kernels.hip), three launches through buf [planes, H, 2W]: the grid's live rows only.  Sides whose padded
// grid runs the power-of-two k-space kernels (toeplitz_fused_ok, by the one rule of fft_kernels.hip); other handles run the composed form
bool toeplitz_fused_ok(int H, int W);
hipError_t launch_toeplitz_rows_fwd(const float2* p, float2* buf, const float2* tw, int planes, int H, int W, hipStream_t s);
hipError_t launch_toeplitz_cols(float2* buf, const float* K, const float2* tw, int planes, int H, int W, hipStream_t s);   // tw: of 2H
// q = the cropped inverse rows (+ mu pv by one fma; partial as launch_toeplitz_crop; stopped slices skipped)
hipError_t launch_toeplitz_rows_inv(const float2* buf, const float2* tw, const float2* pv, const float* mu, const float* tact, float2* q,
                                    double* partial, int planes, int H, int W, hipStream_t s);

// ---- density compensation (dcf_kernels.hip; the iteration: include/pnpadmm_dcf.h) ----------------------
// The weights of a pass: w64 [M] (the float64 iterate), else w32 [M] (the caller's float32 start; an entry that is not positive and finite
// reads as 1), else 1.
int dcf_gather_blocks(int64_t m);                          // workgroups (= maxima per pass) of the gather
int dcf_sum_chunks(int64_t m);                             // partial sums of the finish
// grid [gh, gw] float64 = G^T w: every grid point is written
hipError_t launch_dcf_spread(const double* w64, const float* w32, const NufftDev& P, double* grid, hipStream_t s);
// d = G grid; psi [M] = float32(d), wout [M] = w / d, wmax [dcf_gather_blocks] = max |d - 1| per workgroup; each may be nullptr
hipError_t launch_dcf_gather(const double* grid, const NufftDev& P, const double* w64, const float* w32, double* wout, float* psi, float* wmax,
                             hipStream_t s);
// out [M] = float32(w (h w / sum w)); info [passes] = the maximum of each pass's wmax row (info may be nullptr); partial [dcf_sum_chunks]
hipError_t launch_dcf_finish(const double* w, double* partial, const NufftDev& P, float* out, const float* wmax, int passes, float* info,
                             hipStream_t s);

// ---- off-resonance correction (offres_kernels.hip; the operator: include/pnpadmm_offres.h; the plan: offres_plan.h) ---
// The uploaded plan: every pointer is device memory, laid out as OffresPlan's vectors
struct OffresDev {
    int segments = 0;        // L; 0: no plan
    double* tau = nullptr;   // [L]
    int* seg = nullptr;      // [M]
    float* b0 = nullptr;     // [M]
    float* b1 = nullptr;     // [M]
    int* list_off = nullptr; // [L tiles + 1]
    int* list_idx = nullptr;
    int kind = 0;            // 0: no plan, 1: the linear interpolator (seg, b0, b1, lists), 2: least squares (coef; include/pnpadmm_offres_ls.h)
    float* coef = nullptr;   // [L][M] segment-major, kind == 2
};
static constexpr int kOffresBlock = 8;     // default segments per block (PNP_OFFRES_SEG_BLOCK overrides it)
// the steps of the operator, as bits: which of them run as the naive launches.  Both forms give the same numbers (include/pnpadmm_offres.h)
enum OffresStep : int { OR_GATHER = 1, OR_GRID = 2, OR_ALL = 3 };
// the shipped choice (profiles/offres_bench.json): a two-segment kernel ships only where it is not slower than the naive form
static constexpr int kOffresNaiveSteps = 0;
// maps [map_n, L, h, w] = exp(-i omega tau_l); omega: [map_n, h, w]
hipError_t launch_offres_maps(const float* omega, int map_n, const OffresDev& R, const NufftDev& P, float2* maps, hipStream_t s);
// out [batch, M] (+)= the blended gather of the block's grids [batch, cb, gh, gw] (segments l0 .. l0 + cb - 1); a sample whose first segment
// lies before the block continues from out
hipError_t launch_offres_interp(const float2* grid, const OffresDev& R, const NufftDev& P, float2* out, int l0, int cb, int batch, hipStream_t s);
// the naive form's blend of the block's samples samp [batch, cb, M]
hipError_t launch_offres_blend(const float2* samp, const OffresDev& R, const NufftDev& P, float2* out, int l0, int cb, int batch, hipStream_t s);
// the naive form's expansion ye [batch, cb, M] = b_l . y of y [batch, M]
hipError_t launch_offres_expand(const float2* y, const OffresDev& R, const NufftDev& P, float2* ye, int l0, int cb, int batch, hipStream_t s);
// grid [batch, cb, gh, gw] = per segment of the block the spread of w . b_l . y, every grid point written, no atomics
// filter: walk the NUFFT plan's whole tile bin per segment instead of the plan's per-(segment, tile) list (PNP_OFFRES_GRID_FILTER: timing)
hipError_t launch_offres_grid(const float2* y, const float* w, const OffresDev& R, const NufftDev& P, float2* grid, int l0, int cb, int batch,
                              hipStream_t s, bool filter = false);

// ---- off-resonance correction, least-squares interpolator (offres_ls_kernels.hip; include/pnpadmm_offres_ls.h; the plan: offres_ls_plan.h) ---
// the steps, as OffresStep bits, that run as the naive launches under a least-squares plan.  The shipped choice (profiles/offres_ls_bench.json,
// DESIGN.md 4a): a dense kernel ships only where it is not slower than the naive launches.  At the benchmark shape the dense gridding takes
// 0.92x of the naive launches' adjoint and ships; the dense gather takes 1.46x of their forward, so the gather ships naive and the dense
// one stays behind PNP_OFFRES_LS_NAIVE=0
static constexpr int kOffresLsNaiveSteps = OR_GATHER;
static constexpr int kOffresLsSub = 8;     // segments per workgroup of the dense gridding (its register and LDS sub-block)
// out [batch, M] = the chain over the block's segments of coef_l . gather(grid l); l0 > 0 continues from out
hipError_t launch_offres_ls_interp(const float2* grid, const OffresDev& R, const NufftDev& P, float2* out, int l0, int cb, int batch, hipStream_t s);
// the naive form's blend of the block's samples samp [batch, cb, M], and its expansion ye [batch, cb, M] = coef_l . y of y [batch, M]
hipError_t launch_offres_ls_blend(const float2* samp, const OffresDev& R, const NufftDev& P, float2* out, int l0, int cb, int batch, hipStream_t s);
hipError_t launch_offres_ls_expand(const float2* y, const OffresDev& R, const NufftDev& P, float2* ye, int l0, int cb, int batch, hipStream_t s);
// grid [batch, cb, gh, gw] = per segment of the block the spread of w . coef_l . y over the tile's whole bin, every grid point written, no
// atomics; skip: a wave passes over a sample that touches none of its rows (false: PNP_OFFRES_LS_NOSKIP, timing)
hipError_t launch_offres_ls_grid(const float2* y, const float* w, const OffresDev& R, const NufftDev& P, float2* grid, int l0, int cb, int batch,
                                 hipStream_t s, bool skip = true);

// ---- off-resonance correction for multi-coil data (offres_mc_kernels.hip; include/pnpadmm_offres_mc.h) ---------
// default coils per block (PNP_OFFRES_MC_COIL_BLOCK overrides both): the fastest of 1 / 2 / 4 as measured (profiles/offres_mc_bench.json,
// DESIGN.md 4a) - 4 under a least-squares plan (step 0.72x of the composed form at L = 8; 2: 0.79x), 2 under a linear plan (0.92x at
// L = 32; 4: 0.99x)
static constexpr int kOffresMcBlock = 4;
static constexpr int kOffresMcBlockLinear = 2;
// the two steps that exist in a fused and a composed form, as bits: which of them run composed.  Both give the same bits
enum OffresMcStep : int { ORM_PAD = 1, ORM_CROP = 2, ORM_ALL = 3 };
// the shipped choice (profiles/offres_mc_bench.json): both fused steps measured no slower than the composed form
static constexpr int kOffresMcNaiveSteps = 0;
// grid [batch, cbc, sb, gh, gw] = zero-padded (cy cx) . (E_(l0+k) . (S_(c0+j) . src)); src complex, or src_real
hipError_t launch_offres_mc_pad(const float2* src, const float* src_real, const float2* sens, int sens_n, int C, int c0, int cbc, const float2* maps,
                                int map_n, int L, int l0, int sb, const NufftDev& P, float2* grid, int batch, hipStream_t s);
// the segment chain per coil through part [batch, cbc, h, w] (read unless l0 == 0, written unless l0 + sb == L), then on the last segment
// block the coil chain through q (read unless c0 == 0); the last coil block adds mu pv and leaves the partial sums of Re<pv, q> (pv, mu,
// tact, partial may be nullptr)
hipError_t launch_offres_mc_crop(const float2* grid, const float2* sens, int sens_n, int C, int c0, int cbc, const float2* maps, int map_n, int L,
                                 int l0, int sb, const NufftDev& P, float2* part, const float2* pv, const float* mu, const float* tact, float2* q,
                                 double* partial, int batch, hipStream_t s);

// ---- Toeplitz form of the off-resonance operator (offres_tz_kernels.hip; include/pnpadmm_offres_tz.h; the plan: offres_tz_plan.h) -----
static constexpr int kOffresTzPlanes = 512;   // planes (slices x segments) in flight in the pass buffers: a slice block is kOffresTzPlanes / L slices
// the uploaded pair plan: which samples the workgroups of pair block b walk (nullptr: all of them, in order)
struct OffresTzDev {
    int pairs = 0;           // P; 0: no plan
    int pair_block = 0;      // pairs per workgroup of the build
    int blocks = 0;
    int* blk_off = nullptr;  // [blocks + 1], or nullptr: every block walks samples 0 .. M - 1
    int* blk_idx = nullptr;  // ascending sample indices per block
};
// K [P, 2H, 2W] float32 from traj [M][2] float64 (ky, kx), w [M] float32 or nullptr (1) and the coefficients of R: the header's float64
// Dirichlet sums, no atomics
hipError_t launch_offres_tz_spectra(const double* traj, const float* w, const OffresDev& R, const OffresTzDev& T, int64_t m, int H, int W, float* K,
                                    hipStream_t s);
// y [slices, L, 2H, 2W] = scale . (sum over ascending l' of K_ll' x_l'), restricted to the band |l - l'| <= 1 under a linear plan (kind == 1)
hipError_t launch_offres_tz_mix(const float2* x, float2* y, const float* K, int kind, int L, int H, int W, int slices, float scale, hipStream_t s);
// the column passes of the fused application (fft_kernels.hip): half [planes, H, 2W] -> full [planes, 2H, 2W] and back, unscaled
hipError_t launch_offres_tz_cols_fwd(const float2* half, float2* full, const float2* tw, int planes, int H, int W, hipStream_t s);
hipError_t launch_offres_tz_cols_inv(const float2* full, float2* half, const float2* tw, int planes, int H, int W, hipStream_t s);

// ---- field map estimation (fieldmap_kernels.hip; the fit: include/pnpadmm_fieldmap.h) ----------------------------
// The fused kernel's plan: kFmT sweeps per launch over a kFmRegion^2 region, of which the kFmTile^2 tile is stored
static constexpr int kFmT = 10, kFmRegion = 128, kFmTile = kFmRegion - 2 * kFmT;
struct FmArgs {
    const float2* x1;      // [N,C,H,W] the echo images (prepare)
    const float2* x2;
    int C;
    float* phi;            // [N,H,W] planes of the workspace: prepare writes phi, w (m, then normalised by the weights kernel) and rd
    float* w;
    float* rd;
    const float* th_in;    // [N,H,W] the iterate a sweep / the finish reads
    float* th_out;         // [N,H,W] the iterate a sweep writes (never th_in); prepare: theta^0 = phi
    float* maxpart;        // [N, pixel_chunks] workgroup maxima of m
    float* weight;         // [N,H,W] the caller's copy of w, or nullptr
    float* omega_out;      // [N,H,W] (finish)
    const float* omega_in; // [N,H,W] (cost)
    double* part;          // [N, pixel_chunks] chunk sums of the cost
    double* cost;          // [N]
    double dte;
    float beta;
    int H, W;
    int iters;             // fused kernel: sweeps of this launch, 1..kFmT
    int tiles_x, tiles_y;  // set by the launchers
};
hipError_t launch_fm_prepare(FmArgs a, int N, hipStream_t s);  // phi, w, rd, theta^0 (th_out), weight: two launches
hipError_t launch_fm_fused(FmArgs a, int N, hipStream_t s);    // a.iters sweeps th_in -> th_out
hipError_t launch_fm_sweep(FmArgs a, int N, hipStream_t s);    // ONE sweep th_in -> th_out, a thread per pixel
hipError_t launch_fm_finish(FmArgs a, int N, hipStream_t s);   // omega_out = th_in / dte
hipError_t launch_fm_cost(FmArgs a, int N, hipStream_t s);     // cost [N] = Psi at omega_in with the planes of launch_fm_prepare: two launches

}  // namespace pnp
