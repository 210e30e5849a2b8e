// C ABI of libpnpadmm.so (declared in include/pnpadmm.h): engine object, weight ingest, launch
// sequencing of one PnP-ADMM iteration, kernel-level event timing.
#include "../../include/pnpadmm.h"
#include "../../include/pnpadmm_ncsense.h"
#include "../../include/pnpadmm_toeplitz.h"
#include "../../include/pnpadmm_dcf.h"
#include "../../include/pnpadmm_offres.h"
#include "../../include/pnpadmm_offres_ls.h"
#include "../../include/pnpadmm_offres_mc.h"
#include "../../include/pnpadmm_fieldmap.h"
#include "../../include/pnpadmm_offres_tz.h"
#include "pnp_internal.h"
#include "denoiser_plan.h"
#include "nufft_plan.h"
#include "offres_plan.h"
#include "offres_ls_plan.h"
#include "offres_tz_plan.h"
#include "block_reduce.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

using namespace pnp;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(PNP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// No C++ exception may cross the C ABI: every entry point body runs inside this guard.
#define PNP_API_BEGIN try {
#define PNP_API_END(name)                                                                          \
    } catch (const std::bad_alloc&) { return fail(PNP_ERR_NOMEM, name ": out of host memory");     \
    } catch (const std::exception& ex_) { return fail(PNP_ERR_INTERNAL, name ": %s", ex_.what());  \
    } catch (...) { return fail(PNP_ERR_INTERNAL, name ": unknown C++ exception"); }

// Entry points run on the handle's device whatever the caller's current device is, and leave the caller's current
// device as they found it.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) { err = hipSetDevice(dev); switched = err == hipSuccess; }
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};
#define PNP_ON_DEVICE(e)                                                                                  \
    DeviceGuard dev_guard_((e)->cfg.device);                                                              \
    if (dev_guard_.err != hipSuccess) return fail(PNP_ERR_HIP, "hipSetDevice(%d): %s", (e)->cfg.device, hipGetErrorString(dev_guard_.err))

constexpr size_t kNParams = 11773857;

// the profile classes of pnp_profile_collect, in the order of _lib.PROFILE_CLASS_NAMES
enum ProfClass : int { PROF_CONV3X3 = 0, PROF_CONV_FIRST = 1, PROF_CONV_LAST = 2, PROF_FFT_ROWS = 3, PROF_FFT_COLS = 4, PROF_OTHER = 5 };
static_assert(PROF_OTHER + 1 == PNP_PROFILE_CLASSES, "one enumerator per profile class");

struct EventPair {
    hipEvent_t a, b;
    int cls, layer;
    int count;      // kernel launches between the two events (a run of same-class kernels shares one pair)
};

// The handle's live data-fidelity stage: the constants installed LAST, which pnp_step / pnp_prox_dual solve with and PNP_RES_DC measures
// against.  STAGE_NONE: nothing installed yet, or dropped with the plan it was built on; STAGE_CART: the closed form (pnp_reset /
// pnp_set_kspace); STAGE_MC: SENSE; the four non-Cartesian kinds are one operator (NcOp below) with or without coil maps and with or without
// the segment maps of a field map - STAGE_NC: neither; STAGE_NS: coils (include/pnpadmm_ncsense.h); STAGE_OR: segments
// (include/pnpadmm_offres.h); STAGE_ORS: both (include/pnpadmm_offres_mc.h).  Their constants live in the handle's one set of slots
// (pnp_engine::st_*).  Every kind but the closed form runs a CG on stage_normal().
// `form`: the normal operator a non-Cartesian stage's CG runs - the gridding pair, the Toeplitz spectrum of include/pnpadmm_toeplitz.h
// (a _tz installer of STAGE_NC / STAGE_NS) or the spectra of include/pnpadmm_offres_tz.h (a _tz installer of STAGE_OR / STAGE_ORS).
// aty, the misfit and the acquisitions run on the gridding pair whatever the form.
// Written by commit_stage and drop_stage only.
enum StageKind { STAGE_NONE, STAGE_CART, STAGE_MC, STAGE_NC, STAGE_NS, STAGE_OR, STAGE_ORS };
enum StageForm { FORM_GRID, FORM_TZ, FORM_OTZ };
struct LiveStage {
    StageKind kind = STAGE_NONE;
    StageForm form = FORM_GRID;
    int coils = 0;               // STAGE_MC, STAGE_NS, STAGE_ORS: coils of the installed constants (else 0)
    int sens_n = 1;              // ... and the sens_n of the installed coil maps
    int cg = 0;                  // CG iterations per step
    bool has_w = false;          // the non-Cartesian kinds: weights were installed (st_w; else they are 1)
    int map_n = 1;               // STAGE_OR, STAGE_ORS: map_n of the installed field map
};
inline bool stage_noncart(StageKind k) { return k == STAGE_NC || k == STAGE_NS || k == STAGE_OR || k == STAGE_ORS; }
inline bool stage_segmented(StageKind k) { return k == STAGE_OR || k == STAGE_ORS; }

}  // namespace

struct pnp_engine {
    pnp_config cfg;
    bool weights_loaded = false;
    LiveStage stage;
    // denoiser
    float* d_wpack[N_LAYERS] = {};   // packed conv3x3 weights, raw for the first and the last layer
    float* d_bias[N_LAYERS] = {};
    float* plane[N_LEVELS][N_SLOTS] = {};   // activation planes by (level, slot); sized by the plan, [.][SLOT_NONE] stays null
    float* d_partial = nullptr;      // split-K workspace (small problems)
    Tuning tune;                      // environment overrides, read once in pnp_create
    DenoiserPlan dplan;               // fixed at pnp_create (plan_denoiser): the allocations, the weight pack and every launch read it
    ConvArgs largs[N_LAYERS] = {};    // per launch of the plan: the ConvArgs fields that never change (planes, sizes, format bits)
    // data-fidelity stage
    FftPlan plan = {};
    float2* d_work = nullptr;   // [N,H,W] complex scratch
    float2* d_y0s = nullptr;    // [N,H,W] sgn * S y0
    uint8_t* d_masks = nullptr; // [mask_n,H,W] S mask
    double* d_ssim_part = nullptr; // [N, ssim_tiles(H, W)] per-tile SSIM sums (pnp_ssim)
    double* d_res_part = nullptr;  // [N, pixel_chunks(H, W), 4] + [N, pixel_chunks(H, W)] per-workgroup sums of squares (pnp_residuals)
    int mask_n = 1;
    size_t ws_bytes = 0;
    // multi-coil (SENSE) data-fidelity stage: allocated / grown by pnp_set_kspace_mc, pnp_reset_mc, pnp_acquire_mc
    float2* mc_y = nullptr;      // [N,C,H,W] sgn * S y per coil (reset_kernel's y0s convention)
    float2* mc_work = nullptr;   // [N,C,H,W] coil-image scratch
    float2* mc_sens = nullptr;   // [sens_n,C,H,W]
    size_t mc_y_cap = 0, mc_work_cap = 0, mc_sens_cap = 0;   // capacities in bytes, as every *_cap below
    float2* mc_vec = nullptr;    // [4,N,H,W]: A^H y and the CG vectors r, p, q
    double* mc_part = nullptr;   // [N, pixel_chunks, 2] per-workgroup sums
    double* mc_sc = nullptr;     // [N, 8] CG scalars (rs, bb, alpha, beta, frozen)
    // coil map estimate (pnp_estimate_sens): allocated inside its first call
    float* cm_max = nullptr;     // [N, pixel_chunks] per-workgroup maxima of rss, then smax [N]
    float* cm_rss = nullptr;     // [N,H,W] rss for callers that pass none
    // coil compression (pnp_coil_compress_matrix): allocated inside its first call, grown by a call that needs more
    double2* cc_part = nullptr;  // [N, gram_chunks, C, C] per-workgroup Gram partials
    double2* cc_gram = nullptr;  // [N, C, C] Gram for callers that pass none
    size_t cc_part_cap = 0, cc_gram_cap = 0;
    // noise pre-whitening (pnp_noise_cov): allocated inside its first call, grown by a call that needs more
    double2* pw_part = nullptr;  // [noise_n, gram_chunks, C, C] per-workgroup covariance partials
    size_t pw_part_cap = 0;
    // ESPIRiT maps (pnp_espirit_sens): allocated inside its first call, grown by a call that needs more
    void* es_ws = nullptr;       // per slice G and the vectors [2, np, np] complex128, then R [N, C, C, D, D] complex64, then nkept [N]
    size_t es_cap = 0;
    // GRAPPA weights (pnp_grappa_weights): allocated inside its first call, grown by a call that needs more
    double2* gr_ws = nullptr;    // per slice M = A^H [A | T], [ns, ns + nt] complex128; the solve factors it in place
    size_t gr_cap = 0;
    // non-Cartesian stage: the plan and its two buffers by pnp_nufft_plan, the episode constants by pnp_set_kspace_nc / pnp_reset_nc
    NufftDev nc;                 // the uploaded plan; nc.m == 0: none
    size_t nc_i0_cap = 0, nc_wts_cap = 0, nc_cy_cap = 0, nc_cx_cap = 0, nc_off_cap = 0, nc_idx_cap = 0, nc_twh_cap = 0, nc_tww_cap = 0;
    float2* nc_grid = nullptr;   // [N, gh, gw] the oversampled grid
    float2* nc_samp = nullptr;   // [N, M] sample scratch (A p inside the normal operator, A x of the misfit)
    size_t nc_grid_cap = 0, nc_samp_cap = 0;
    // the constants of the live non-Cartesian stage, whichever kind it is (the installers' last ws_grow): one set of slots, each as large as
    // the largest install so far needed it
    float2* st_y = nullptr;      // [N, M] or [N, C, M] the installed samples
    float* st_w = nullptr;       // [M] the installed weights (read only through stage_w)
    float2* st_sens = nullptr;   // [sens_n, C, H, W] the installed coil maps
    float2* st_maps = nullptr;   // [map_n, L, H, W] the installed segment maps
    double* st_mpart = nullptr;  // [N, nufft_sample_chunks(M)] or [N, C, nufft_sample_chunks(M)] partial sums of the misfit
    float2* acq_maps = nullptr;  // [map_n, L, H, W] the off-resonance acquisitions' own segment maps: the installed ones stay as they are
    size_t st_y_cap = 0, st_w_cap = 0, st_sens_cap = 0, st_maps_cap = 0, st_mpart_cap = 0, acq_maps_cap = 0;
    // non-Cartesian SENSE (include/pnpadmm_ncsense.h): the coil-block scratch by every entry point of that header
    int ns_block = kNcsenseBlock; // coils per block: kNcsenseBlock, or PNP_NCSENSE_COIL_BLOCK (read at pnp_create)
    int ns_naive = kNcsenseNaiveSteps;   // NcsenseStep bits: the steps that run as the single-coil launches at batch N cb (PNP_NCSENSE_NAIVE: all or none)
    float2* ns_img = nullptr;    // naive pad or crop only: [N, cb, H, W] the block's coil images
    size_t ns_img_cap = 0;
    float2* ns_grid = nullptr;   // [N, cb, gh, gw] the block's oversampled grids
    float2* ns_samp = nullptr;   // [N, cb, M] the block's samples (A p inside the normal operator, A x of the misfit)
    size_t ns_grid_cap = 0, ns_samp_cap = 0;
    // off-resonance correction (include/pnpadmm_offres.h): the plan by pnp_offres_plan; the segment-block scratch is the coil-block
    // scratch above
    std::vector<int32_t> nc_bin_off_h, nc_bin_idx_h;   // host copy of the NUFFT plan's tile bins: what the per-segment lists are built from
    OffresDev orp;               // the uploaded plan; orp.segments == 0: none
    size_t or_tau_cap = 0, or_seg_cap = 0, or_b0_cap = 0, or_b1_cap = 0, or_loff_cap = 0, or_lidx_cap = 0, or_coef_cap = 0;
    int or_block = kOffresBlock; // segments per block: kOffresBlock, or PNP_OFFRES_SEG_BLOCK (read at pnp_create)
    int or_naive = kOffresNaiveSteps;   // OffresStep bits: the steps that run as the naive launches (PNP_OFFRES_NAIVE: all or none)
    int orls_naive = kOffresLsNaiveSteps;   // ... under a least-squares plan (PNP_OFFRES_LS_NAIVE: all or none)
    // off-resonance correction for multi-coil data (include/pnpadmm_offres_mc.h): blocks of coils x segments go through the coil-block scratch
    // above (ns_grid, ns_samp, ns_img), sized for them by op_ensure; the rest is this section's own
    int om_block = 0;                    // coils per block: PNP_OFFRES_MC_COIL_BLOCK (read at pnp_create), or 0: the measured default of the live
                                         // plan's interpolator (om_block_of)
    int om_naive = kOffresMcNaiveSteps;  // OffresMcStep bits: the steps that run composed per coil (PNP_OFFRES_MC_NAIVE: all or none)
    float2* om_samp = nullptr;   // [N, cbc, M] a coil block's samples (A p inside the normal operator, A x of the misfit)
    float2* om_part = nullptr;   // [N, cbc, H, W] the segment chain's partials (allocated only when L > SB); composed adjoint: the coil images a_c
    float2* om_img = nullptr;    // composed form only: [N, H, W] one coil's image
    float2* om_line = nullptr;   // composed form only: [N, M] one coil's samples
    size_t om_samp_cap = 0, om_part_cap = 0, om_img_cap = 0, om_line_cap = 0;
    // Toeplitz normal operator (include/pnpadmm_toeplitz.h): the spectrum and its buffers by pnp_toeplitz_plan
    std::vector<double> nc_traj; // host copy of the planned trajectory [M][2] (ky, kx): what the spectrum is built from
    double* tz_traj = nullptr;   // [M][2] its device copy
    float* tz_k = nullptr;       // [2H, 2W] the spectrum, centred
    float* tz_w = nullptr;       // [M] the weights the spectrum was built with (read only while tz_has_w): the installers' weights
    float2* tz_tw_h = nullptr;   // twiddles of 2H and 2W
    float2* tz_tw_w = nullptr;
    bool tz_fused = false;       // the application runs its three fused launches (set at pnp_create: a power-of-two padded grid and no
                                 // PNP_TOEPLITZ_NAIVE); else the seven composed ones
    float2* tz_grid = nullptr;   // the pass buffer, N planes (N cb for a multi-coil application): [planes, H, 2W] fused, [planes, 2H, 2W] composed
    size_t tz_traj_cap = 0, tz_k_cap = 0, tz_w_cap = 0, tz_twh_cap = 0, tz_tww_cap = 0, tz_grid_cap = 0;
    bool tz_planned = false;     // a spectrum exists for the handle's NUFFT plan
    bool tz_has_w = false;
    // Toeplitz form of the off-resonance operator (include/pnpadmm_offres_tz.h): the spectra and the pass buffers by pnp_offres_tz_plan
    std::vector<int32_t> or_seg_h;   // host copy of the linear plan's segment per sample: what the per-pair sample lists are built from
    OffresTzDev otz;             // the uploaded pair plan; otz.pairs == 0: none
    double* otz_traj = nullptr;  // [M][2] device copy of the trajectory
    float* otz_k = nullptr;      // [P, 2H, 2W] the spectra, centred
    float* otz_w = nullptr;      // [M] the weights the spectra were built with (read only while otz_has_w): the installers' weights
    float2* otz_tw_h = nullptr;  // twiddles of 2H and 2W
    float2* otz_tw_w = nullptr;
    float2* otz_img = nullptr;   // [planes, H, W] the slice block's segment images E_l . p, then the cropped results
    float2* otz_x = nullptr;     // [planes, 2H, 2W] the two pass buffers: transforms in x, mix x -> y, transforms back in y (composed);
    float2* otz_y = nullptr;     // fused: rows into y's first half, columns y -> x, mix x -> y, columns y -> x's first half, rows out of x
    float2* otz_cimg = nullptr;  // multi-coil: [N, CB, H, W] the coil block's images S_c . p, then their results
    size_t otz_off_cap = 0, otz_idx_cap = 0, otz_traj_cap = 0, otz_k_cap = 0, otz_w_cap = 0, otz_twh_cap = 0, otz_tww_cap = 0, otz_img_cap = 0,
           otz_x_cap = 0, otz_y_cap = 0, otz_cimg_cap = 0;
    bool otz_planned = false;    // spectra exist for the handle's NUFFT plan and off-resonance plan
    bool otz_has_w = false;
    bool otz_fused = false;      // the application runs the fused passes (set at pnp_create: a power-of-two padded grid and no PNP_OFFRES_TZ_NAIVE)
    int otz_slices = 0;          // PNP_OFFRES_TZ_SLICE_BLOCK (read at pnp_create), or 0: kOffresTzPlanes / L
    // density compensation (include/pnpadmm_dcf.h): its own workspace, grown inside pnp_nufft_psi / pnp_nufft_dcf
    double* dcf_grid = nullptr;  // [gh, gw] G^T w
    double* dcf_w = nullptr;     // [M] the float64 iterate
    double* dcf_part = nullptr;  // [dcf_sum_chunks(M)] chunk sums of the finish
    float* dcf_max = nullptr;    // [iters + 1, dcf_gather_blocks(M)] workgroup maxima of |Psi w - 1| (only with info)
    size_t dcf_grid_cap = 0, dcf_w_cap = 0, dcf_part_cap = 0, dcf_max_cap = 0;
    // the prior of pnp_step (pnp_set_prior) and the total-variation denoiser's workspace (allocated inside the first call that runs it)
    int prior = PNP_PRIOR_UNET;
    double tv_scale = 1.0;       // as given; applied as float32
    int tv_iters = 20;
    float2* tv_p = nullptr;      // [N,H,W] (py, px): the hand-over plane between launches; the other plane of the ping-pong is d_work
    // the Haar wavelet prior (pnp_set_prior_haar): prior == PNP_PRIOR_HAAR while it is the x-update
    double haar_scale = 1.0;     // as given; applied as float32
    int haar_levels = 3;
    int haar_mode = PNP_HAAR_TI;
    float* haar_ws = nullptr;    // naive form only, allocated inside its first TI call: kHaarNaivePlanes planes [N,H,W] (a_1 .. a_3, two of r_j)
    // field map estimation (include/pnpadmm_fieldmap.h): its own workspace, allocated inside the first call that runs it
    float* fm_ws = nullptr;      // five planes [N,H,W]: phi, w, rd and the two of theta; then [N, pixel_chunks] workgroup maxima
    double* fm_part = nullptr;   // [N, pixel_chunks] chunk sums of the cost
    // profiling
    std::vector<EventPair> events;
    size_t ev_used = 0;
    double cls_ms[PNP_PROFILE_CLASSES] = {};
    int64_t cls_n[PNP_PROFILE_CLASSES] = {};
    double layer_ms[N_LAYERS] = {};
    int64_t layer_n[N_LAYERS] = {};
};

namespace {

#define PNP_KSPACE_SIZES "16, 32, 64, 80, 128, 160, 256, 320, 400, 512, 640, 800, 1024"   // every L with kspace_len_ok(L)
// the rejection of a handle whose sides the k-space stage does not take; `what`: the words between the entry point's name and the size list
int check_kspace_sizes(const char* fn, const pnp_engine* e, const char* what = "the k-space stage takes h, w in") {
    if (kspace_len_ok(e->cfg.h) && kspace_len_ok(e->cfg.w)) return PNP_OK;
    return fail(PNP_ERR_INVALID, "%s: %s {" PNP_KSPACE_SIZES "} (got %dx%d)", fn, what, e->cfg.h, e->cfg.w);
}

// One HIP event pair around a kernel launch - or, with `defer_end`, around a RUN of same-class launches that follow each
// other on the stream (the conv3x3 launches of a denoiser forward): `count` launches, closed by end().  Event records
// cost ~3 us of stream time each, so the default profile mode brackets the conv run once; PNP_FLAG_PROFILE_LAYERS keeps
// a pair per launch for the per-layer table.
struct Prof {
    pnp_engine* e;
    hipStream_t s;
    EventPair* ep = nullptr;
    bool deferred = false;
    Prof(pnp_engine* e_, hipStream_t s_, int cls, int layer, bool active = true, bool defer_end = false) : e(e_), s(s_), deferred(defer_end) {
        if (!active || !(e->cfg.flags & (PNP_FLAG_PROFILE | PNP_FLAG_PROFILE_LAYERS))) return;
        if (e->ev_used == e->events.size()) {
            EventPair p{};
            if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) return;
            e->events.push_back(p);
        }
        ep = &e->events[e->ev_used++];
        ep->cls = cls;
        ep->layer = layer;
        ep->count = 1;
        (void)hipEventRecord(ep->a, s);
    }
    void end(int count) {
        if (ep) { ep->count = count; (void)hipEventRecord(ep->b, s); ep = nullptr; }
    }
    ~Prof() {
        if (ep && !deferred) (void)hipEventRecord(ep->b, s);
        else if (ep) { ep->count = 0; (void)hipEventRecord(ep->b, s); }     // a run left early (error path)
    }
};

// Layout of a pnp_snapshot buffer: [x float32 | z complex64 | u complex64] over the handle's n h w pixels, then t_state float32 [n]
struct SnapLayout {
    size_t px, n;
    explicit SnapLayout(const pnp_engine* e) : px((size_t)e->cfg.n * e->cfg.h * e->cfg.w), n((size_t)e->cfg.n) {}
    size_t x_bytes() const { return px * 4; }
    size_t zu_bytes() const { return px * 8; }             // z and u each
    size_t t_bytes() const { return n * 4; }
    size_t z_off() const { return x_bytes(); }
    size_t u_off() const { return z_off() + zu_bytes(); }
    size_t t_off() const { return u_off() + zu_bytes(); }
    size_t bytes() const { return t_off() + t_bytes(); }
};

std::vector<float2> twiddle_table(int L) {
    std::vector<float2> t(L);
    for (int m = 0; m < L; ++m) {
        const double a = -2.0 * M_PI * (double)m / (double)L;
        t[m] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    return t;
}
int make_twiddles(int L, float2** out) {
    const std::vector<float2> t = twiddle_table(L);
    HIP_TRY(hipMalloc((void**)out, sizeof(float2) * L));
    HIP_TRY(hipMemcpy(*out, t.data(), sizeof(float2) * L, hipMemcpyHostToDevice));
    return PNP_OK;
}

// a conv3x3 launch on the kernel family of its plan record - the family its weights were packed for
hipError_t launch_conv_layer(const ConvLaunch& l, const ConvArgs& a, hipStream_t s) {
    switch (l.family) {
    case FAM_WINO4: return launch_conv3x3_winograd4(a, l.wino, l.src_mode, s);
    case FAM_WINO2: return launch_conv3x3_winograd(a, l.wino, l.src_mode, s);
    case FAM_DIRECT: case FAM_WS: return launch_conv3x3(a, l.conv, l.src_mode, s);
    default: return hipErrorInvalidValue;
    }
}

// The part of every launch's ConvArgs that is fixed with the plan: plane names resolved to the handle's buffers, sizes, format bits.
void resolve_launches(pnp_engine* e) {
    const DenoiserPlan& P = e->dplan;
    auto at = [&](PlaneRef r) { return e->plane[r.level][r.slot]; };
    for (int i = 0; i < P.n_launches; ++i) {
        const ConvLaunch& l = P.launch[i];
        const LayerSpec& L = kLayers[l.layer];
        ConvArgs a{};
        a.src0 = at(l.src0); a.src1 = at(l.src1); a.dst = at(l.dst); a.pooled = at(l.pooled);
        a.partial = e->d_partial;
        a.bf16 = P.bf16_terms;
        a.act16 = l.act16;
        a.N = e->cfg.n; a.H = e->cfg.h >> L.level; a.W = e->cfg.w >> L.level; a.Cin = L.cin; a.Cskip = L.cskip; a.Cout = L.cout;
        if (L.src == SRC_UPCAT) {
            const int hs = a.H / 2, ws = a.W / 2;
            a.rh = a.H > 1 ? (float)(hs - 1) / (float)(a.H - 1) : 0.f;
            a.rw = a.W > 1 ? (float)(ws - 1) / (float)(a.W - 1) : 0.f;
        }
        e->largs[i] = a;
    }
}

// ConvArgs of launch `i` of the plan for one forward: the resolved part plus the weights and the caller's pointers
ConvArgs conv_args(const pnp_engine* e, int i, const float* ximg, const float2* z, const float2* u, const float* sigma, const float* tact, float* out) {
    const ConvLaunch& l = e->dplan.launch[i];
    ConvArgs a = e->largs[i];
    a.wpack = e->d_wpack[l.layer]; a.bias = e->d_bias[l.layer]; a.tact = tact;
    if (l.fused_first) {                               // inc.conv-1 evaluates the first layer while staging its patch
        a.first_w = e->d_wpack[0]; a.first_b = e->d_bias[0]; a.first_sigma = sigma;
        a.last_ximg = ximg; a.last_z = z; a.last_u = u;
    }
    if (l.fused_last) {                                // up4.conv-2 with the last layer (1x1 + residual + clamp) in its epilogue: writes `out` directly
        a.last_w = e->d_wpack[N_LAYERS - 1]; a.last_b = e->d_bias[N_LAYERS - 1]; a.last_ximg = ximg; a.last_z = z; a.last_u = u; a.last_out = out;
    }
#ifdef PNP_DIAG
    if (const char* dv = getenv("PNP_DIAG_L0")) a.diag = kLayers[l.layer].level == 0 ? atoi(dv) : 0;
    if (const char* dv = getenv("PNP_DIAG_ALL")) a.diag = atoi(dv);
#endif
    return a;
}

// One denoiser forward: the launches of the handle's plan in order - the first layer (unless fused), the run of conv3x3 MFMA launches,
// the last layer (unless fused).  Image channel = ximg, or Re(z-u).
int run_unet(pnp_engine* e, const float* ximg, const float2* z, const float2* u, const float* sigma,
             const float* tact, float* out, hipStream_t s) {
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w;
    if (e->cfg.flags & PNP_FLAG_NO_DENOISER)
        return fail(PNP_ERR_STATE, "this handle was created with PNP_FLAG_NO_DENOISER");
    const DenoiserPlan& P = e->dplan;
    int i = 0;
    if (P.launch[i].family == FAM_FIRST) {
        Prof p(e, s, PROF_CONV_FIRST, P.launch[i].layer);
        HIP_TRY(launch_conv_first(ximg, z, u, sigma, tact, e->d_wpack[0], e->d_bias[0], e->largs[i].dst, N, H, W, s, (P.launch[i].act16 & 2) != 0));
        ++i;
    }
    const bool per_layer = (e->cfg.flags & PNP_FLAG_PROFILE_LAYERS) != 0;
#ifdef PNP_DIAG
    static hipStream_t diag_pool[8];
    static hipEvent_t diag_fork, diag_join[8];
    static int diag_made = 0;
    const int diag_k = getenv("PNP_DIAG_STREAMS") ? std::min(8, std::max(1, atoi(getenv("PNP_DIAG_STREAMS")))) : 1;
    if (diag_k > 1) {
        if (!diag_made) {
            for (int i = 0; i < 8; ++i) { HIP_TRY(hipStreamCreateWithFlags(&diag_pool[i], hipStreamNonBlocking)); HIP_TRY(hipEventCreateWithFlags(&diag_join[i], hipEventDisableTiming)); }
            HIP_TRY(hipEventCreateWithFlags(&diag_fork, hipEventDisableTiming));
            diag_made = 1;
        }
        HIP_TRY(hipEventRecord(diag_fork, s));
        for (int i = 0; i < diag_k; ++i) HIP_TRY(hipStreamWaitEvent(diag_pool[i], diag_fork, 0));
    }
    struct DiagJoin {
        hipStream_t s; int k; hipStream_t* pool; hipEvent_t* ev;
        ~DiagJoin() { if (k > 1) for (int i = 0; i < k; ++i) { (void)hipEventRecord(ev[i], pool[i]); (void)hipStreamWaitEvent(s, ev[i], 0); } }
    } diag_joiner{s, diag_k, diag_pool, diag_join};
#endif
    Prof run(e, s, PROF_CONV3X3, -1, !per_layer, true);   // one event pair around the whole conv3x3 run
    int run_launches = 0;
    for (; i < P.n_launches && P.launch[i].family != FAM_LAST; ++i) {
        const ConvLaunch& l = P.launch[i];
        const ConvArgs a = conv_args(e, i, ximg, z, u, sigma, tact, out);
        Prof p(e, s, PROF_CONV3X3, l.layer, per_layer);
        ++run_launches;
        hipStream_t ls = s;
#ifdef PNP_DIAG
        // PNP_DIAG_STREAMS=K (timing only, results wrong): conv launch i goes to side stream i % K, so consecutive layers do NOT wait for
        // each other - the ceiling of any scheme that overlaps a layer's tail with its successor's head (profiles/r05_ablation.md)
        if (diag_k > 1) ls = diag_pool[l.layer % diag_k];
#endif
        HIP_TRY(launch_conv_layer(l, a, ls));
    }
    run.end(run_launches);
    if (i < P.n_launches) {
        Prof p(e, s, PROF_CONV_LAST, P.launch[i].layer);
        HIP_TRY(launch_conv_last(e->largs[i].src0, ximg, z, u, tact, e->d_wpack[N_LAYERS - 1], e->d_bias[N_LAYERS - 1], out, N, H, W, s));
    }
    return PNP_OK;
}

// ---- the plain transform ----------------------------------------------------------------------------
// Plain (unshifted) orthonormal 2-D transform of `batch` planes, src -> dst; the shifts of fft_c live in the constants and indices of the
// pointwise kernels around it.  Forward: rows src -> dst (or from `real_src`, a real image read once with no complex copy of it; src unused),
// then columns in place in dst.  Inverse: columns in place in SRC, then rows src -> dst - the other order, which rounds differently.
// src == dst is the in-place transform: a row workgroup reads and writes its own rows only.
int plain_fft2(pnp_engine* e, float2* src, float2* dst, int batch, int inverse, hipStream_t s, const float* real_src = nullptr) {
    const int H = e->cfg.h, W = e->cfg.w;
    auto rows = [&]() -> int {
        Prof p(e, s, PROF_FFT_ROWS, -1);
        if (real_src) HIP_TRY(launch_fft_rows_real(real_src, dst, e->plan.tw_w, batch, H, W, s));
        else HIP_TRY(launch_fft_rows(src, dst, e->plan.tw_w, batch, H, W, inverse, 0, s));
        return PNP_OK;
    };
    auto cols = [&]() -> int {
        Prof p(e, s, PROF_FFT_COLS, -1);
        HIP_TRY(launch_fft_cols(inverse ? src : dst, e->plan.tw_h, batch, H, W, inverse, 0, s));
        return PNP_OK;
    };
    int rc;
    if (inverse) { if ((rc = cols()) || (rc = rows())) return rc; }
    else { if ((rc = rows()) || (rc = cols())) return rc; }
    return PNP_OK;
}

// ---- multi-coil stage -------------------------------------------------------------------------------
float2* mc_aty(pnp_engine* e) { return e->mc_vec; }
float2* mc_r(pnp_engine* e) { return e->mc_vec + (size_t)e->cfg.n * e->cfg.h * e->cfg.w; }
float2* mc_p(pnp_engine* e) { return e->mc_vec + 2 * (size_t)e->cfg.n * e->cfg.h * e->cfg.w; }
float2* mc_q(pnp_engine* e) { return e->mc_vec + 3 * (size_t)e->cfg.n * e->cfg.h * e->cfg.w; }

// q = A^H A pv + mu pv; the partial sums of Re<pv, q> go to mc_part.  Unfused: seven launches.
int mc_normal(pnp_engine* e, const float2* pv, const float* mu, const float* tact, float2* q, hipStream_t s) {
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w, C = e->stage.coils;
    int rc;
    {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_sense_expand(pv, nullptr, e->mc_sens, e->stage.sens_n, C, tact, e->mc_work, N, H, W, s));
    }
    if ((rc = plain_fft2(e, e->mc_work, e->mc_work, N * C, 0, s))) return rc;
    {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_sense_mask(e->mc_work, e->d_masks, e->mask_n, C, N, H, W, s));
    }
    if ((rc = plain_fft2(e, e->mc_work, e->mc_work, N * C, 1, s))) return rc;
    Prof p(e, s, PROF_OTHER, -1);
    HIP_TRY(launch_sense_combine(e->mc_work, e->mc_sens, e->stage.sens_n, C, pv, mu, tact, q, e->mc_part, N, H, W, s));
    return PNP_OK;
}

// ---- non-Cartesian stage ----------------------------------------------------------------------------
// the live non-Cartesian stage's weights (nullptr: 1)
const float* stage_w(const pnp_engine* e) { return e->stage.has_w ? e->st_w : nullptr; }
// the centred transform of pnp_fft2c of `planes` planes of gh x gw, in place in `grid`: rows then columns in both directions
int grid_fft(pnp_engine* e, float2* grid, const float2* tw_h, const float2* tw_w, int planes, int gh, int gw, int inverse, hipStream_t s) {
    {
        Prof p(e, s, PROF_FFT_ROWS, -1);
        HIP_TRY(launch_fft_rows(grid, grid, tw_w, planes, gh, gw, inverse, gw / 2, s));
    }
    Prof p(e, s, PROF_FFT_COLS, -1);
    HIP_TRY(launch_fft_cols(grid, tw_h, planes, gh, gw, inverse, gh / 2, s));
    return PNP_OK;
}
// ... on the NUFFT plan's oversampled grid: nc_grid, or the block's grids in ns_grid
int nc_fft(pnp_engine* e, float2* grid, int planes, int inverse, hipStream_t s) {
    return grid_fft(e, grid, e->nc.tw_gh, e->nc.tw_gw, planes, e->nc.gh, e->nc.gw, inverse, s);
}
// out [batch, M] = A src (src complex, or src_real: a real image)
int nc_forward(pnp_engine* e, const float2* src, const float* src_real, int batch, float2* out, hipStream_t s) {
    {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_nufft_pad(src, src_real, e->nc, e->nc_grid, batch, s));
    }
    if (int rc = nc_fft(e, e->nc_grid, batch, 0, s)) return rc;
    Prof p(e, s, PROF_OTHER, -1);
    HIP_TRY(launch_nufft_interp(e->nc_grid, e->nc, out, batch, s));
    return PNP_OK;
}
// q [batch, h, w] = A^H (w . y) (+ mu pv, with the partial sums of Re<pv, q>: the crop kernel's epilogue)
int nc_adjoint(pnp_engine* e, const float2* y, const float* w, int batch, const float2* pv, const float* mu, const float* tact, float2* q,
               double* partial, hipStream_t s) {
    {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_nufft_grid(y, w, e->nc, e->nc_grid, batch, s));
    }
    if (int rc = nc_fft(e, e->nc_grid, batch, 1, s)) return rc;
    Prof p(e, s, PROF_OTHER, -1);
    HIP_TRY(launch_nufft_crop(e->nc_grid, e->nc, pv, mu, tact, q, partial, batch, s));
    return PNP_OK;
}

// ---- non-Cartesian SENSE stage (include/pnpadmm_ncsense.h) --------------------------------------------
int ns_block_of(const pnp_engine* e, int coils) { return coils < e->ns_block ? coils : e->ns_block; }
// F_nu(S_c . src) for the block's coils c0 .. c0 + cb - 1 into out [batch, ocs, M] at the coils oc0 ..
int ns_forward_block(pnp_engine* e, const float2* src, const float* src_real, const float2* sens, int sens_n, int C, int c0, int cb, int batch,
                     float2* out, int ocs, int oc0, hipStream_t s) {
    const size_t row = (size_t)cb * e->nc.m * sizeof(float2);          // one slice's samples of the block
    const bool direct = ocs == cb;                                     // (then oc0 == 0) the block's samples are contiguous in out
    {
        Prof p(e, s, PROF_OTHER, -1);
        if (e->ns_naive & NS_PAD) {
            HIP_TRY(launch_ncsense_expand(src, src_real, sens, sens_n, C, c0, cb, e->nc, e->ns_img, batch, s));
            HIP_TRY(launch_nufft_pad(e->ns_img, nullptr, e->nc, e->ns_grid, batch * cb, s));
            p.end(2);
        } else {
            HIP_TRY(launch_ncsense_pad(src, src_real, sens, sens_n, C, c0, cb, e->nc, e->ns_grid, batch, s));
        }
    }
    if (int rc = nc_fft(e, e->ns_grid, batch * cb, 0, s)) return rc;
    Prof p(e, s, PROF_OTHER, -1);
    if (!(e->ns_naive & NS_GATHER)) {
        HIP_TRY(launch_ncsense_interp(e->ns_grid, e->nc, out, ocs, oc0, cb, batch, s));
        return PNP_OK;
    }
    HIP_TRY(launch_nufft_interp(e->ns_grid, e->nc, direct ? out : e->ns_samp, batch * cb, s));
    if (!direct)
        HIP_TRY(hipMemcpy2DAsync(out + (size_t)oc0 * e->nc.m, (size_t)ocs * e->nc.m * sizeof(float2), e->ns_samp, row, row, (size_t)batch,
                                 hipMemcpyDeviceToDevice, s));
    return PNP_OK;
}
// q (+)= sum over the block's coils of conj(S_c) . F_nu^H(w . y[., yc0 + j]); the last block adds mu pv and leaves the partial sums of Re<pv, q>
int ns_adjoint_block(pnp_engine* e, const float2* y, int ycs, int yc0, const float* w, const float2* sens, int sens_n, int C, int c0, int cb,
                     int batch, const float2* pv, const float* mu, const float* tact, float2* q, double* partial, hipStream_t s) {
    {
        Prof p(e, s, PROF_OTHER, -1);
        if (e->ns_naive & NS_GRID) {
            const size_t row = (size_t)cb * e->nc.m * sizeof(float2);
            if (ycs != cb)                                             // the block's samples gathered into the contiguous scratch
                HIP_TRY(hipMemcpy2DAsync(e->ns_samp, row, y + (size_t)yc0 * e->nc.m, (size_t)ycs * e->nc.m * sizeof(float2), row, (size_t)batch,
                                         hipMemcpyDeviceToDevice, s));
            HIP_TRY(launch_nufft_grid(ycs != cb ? e->ns_samp : y, w, e->nc, e->ns_grid, batch * cb, s));
        } else {
            HIP_TRY(launch_ncsense_grid(y, ycs, yc0, cb, w, e->nc, e->ns_grid, batch, s));
        }
    }
    if (int rc = nc_fft(e, e->ns_grid, batch * cb, 1, s)) return rc;
    Prof p(e, s, PROF_OTHER, -1);
    if (e->ns_naive & NS_CROP) {
        HIP_TRY(launch_nufft_crop(e->ns_grid, e->nc, nullptr, nullptr, nullptr, e->ns_img, nullptr, batch * cb, s));
        HIP_TRY(launch_ncsense_combine(e->ns_img, sens, sens_n, C, c0, cb, e->nc, pv, mu, tact, q, partial, batch, s));
        p.end(2);
    } else {
        HIP_TRY(launch_ncsense_crop(e->ns_grid, sens, sens_n, C, c0, cb, e->nc, pv, mu, tact, q, partial, batch, s));
    }
    return PNP_OK;
}
// out [batch, C, M] = A src, block by block
int ns_forward(pnp_engine* e, const float2* src, const float* src_real, const float2* sens, int sens_n, int C, int batch, float2* out, hipStream_t s) {
    const int B = ns_block_of(e, C);
    for (int c0 = 0; c0 < C; c0 += B)
        if (int rc = ns_forward_block(e, src, src_real, sens, sens_n, C, c0, std::min(B, C - c0), batch, out, C, c0, s)) return rc;
    return PNP_OK;
}
// q [batch, h, w] = A^H (w . y), y: [batch, C, M]
int ns_adjoint(pnp_engine* e, const float2* y, const float* w, const float2* sens, int sens_n, int C, int batch, float2* q, hipStream_t s) {
    const int B = ns_block_of(e, C);
    for (int c0 = 0; c0 < C; c0 += B)
        if (int rc = ns_adjoint_block(e, y, C, c0, w, sens, sens_n, C, c0, std::min(B, C - c0), batch, nullptr, nullptr, nullptr, q, nullptr, s))
            return rc;
    return PNP_OK;
}

// ---- off-resonance correction (include/pnpadmm_offres.h) ------------------------------------------------
int or_block_of(const pnp_engine* e) { return e->orp.segments < e->or_block ? e->orp.segments : e->or_block; }
// the steps that run as the naive launches under the live plan's interpolator
int or_naive_of(const pnp_engine* e) { return e->orp.kind == 2 ? e->orls_naive : e->or_naive; }
// out [batch, M] = A src with the segment maps `maps` [map_n, L, h, w], block by block: a block's samples are blended into out before the
// next block's grids replace them
int or_forward(pnp_engine* e, const float2* src, const float* src_real, const float2* maps, int map_n, int batch, float2* out, hipStream_t s) {
    const int L = e->orp.segments, B = or_block_of(e);
    const bool ls = e->orp.kind == 2;
    for (int l0 = 0; l0 < L; l0 += B) {
        const int cb = std::min(B, L - l0);
        if (or_naive_of(e) & OR_GATHER) {
            if (int rc = ns_forward_block(e, src, src_real, maps, map_n, L, l0, cb, batch, e->ns_samp, cb, 0, s)) return rc;
            Prof p(e, s, PROF_OTHER, -1);
            if (ls) HIP_TRY(launch_offres_ls_blend(e->ns_samp, e->orp, e->nc, out, l0, cb, batch, s));
            else HIP_TRY(launch_offres_blend(e->ns_samp, e->orp, e->nc, out, l0, cb, batch, s));
            continue;
        }
        {
            Prof p(e, s, PROF_OTHER, -1);
            if (e->ns_naive & NS_PAD) {
                HIP_TRY(launch_ncsense_expand(src, src_real, maps, map_n, L, l0, cb, e->nc, e->ns_img, batch, s));
                HIP_TRY(launch_nufft_pad(e->ns_img, nullptr, e->nc, e->ns_grid, batch * cb, s));
                p.end(2);
            } else {
                HIP_TRY(launch_ncsense_pad(src, src_real, maps, map_n, L, l0, cb, e->nc, e->ns_grid, batch, s));
            }
        }
        if (int rc = nc_fft(e, e->ns_grid, batch * cb, 0, s)) return rc;
        Prof p(e, s, PROF_OTHER, -1);
        if (ls) HIP_TRY(launch_offres_ls_interp(e->ns_grid, e->orp, e->nc, out, l0, cb, batch, s));
        else HIP_TRY(launch_offres_interp(e->ns_grid, e->orp, e->nc, out, l0, cb, batch, s));
    }
    return PNP_OK;
}
// q [batch, h, w] = A^H (w . y), y: [batch, M] (+ mu pv with the partial sums of Re<pv, q>: the last block's epilogue; pv, mu, tact, partial
// may be nullptr)
int or_adjoint(pnp_engine* e, const float2* y, const float* w, const float2* maps, int map_n, int batch, const float2* pv, const float* mu,
               const float* tact, float2* q, double* partial, hipStream_t s) {
    const int L = e->orp.segments, B = or_block_of(e);
    const bool ls = e->orp.kind == 2;
    for (int l0 = 0; l0 < L; l0 += B) {
        const int cb = std::min(B, L - l0);
        // the dense least-squares gridding costs what a full sub-block of 8 segments costs: by default it runs on full sub-blocks only
        // (measured: 0.92x of the naive launches at 8 segments, 1.09x at 6); PNP_OFFRES_LS_NAIVE=0 runs it on every block
        const bool ragged = ls && e->tune.offres_ls_naive < 0 && cb % kOffresLsSub != 0;
        if ((or_naive_of(e) & OR_GRID) || ragged) {
            {
                Prof p(e, s, PROF_OTHER, -1);
                if (ls) HIP_TRY(launch_offres_ls_expand(y, e->orp, e->nc, e->ns_samp, l0, cb, batch, s));
                else HIP_TRY(launch_offres_expand(y, e->orp, e->nc, e->ns_samp, l0, cb, batch, s));
            }
            if (int rc = ns_adjoint_block(e, e->ns_samp, cb, 0, w, maps, map_n, L, l0, cb, batch, pv, mu, tact, q, partial, s)) return rc;
            continue;
        }
        {
            Prof p(e, s, PROF_OTHER, -1);
            if (ls) HIP_TRY(launch_offres_ls_grid(y, w, e->orp, e->nc, e->ns_grid, l0, cb, batch, s, !e->tune.offres_ls_noskip));
            else HIP_TRY(launch_offres_grid(y, w, e->orp, e->nc, e->ns_grid, l0, cb, batch, s, e->tune.offres_grid_filter));
        }
        if (int rc = nc_fft(e, e->ns_grid, batch * cb, 1, s)) return rc;
        Prof p(e, s, PROF_OTHER, -1);
        if (e->ns_naive & NS_CROP) {
            HIP_TRY(launch_nufft_crop(e->ns_grid, e->nc, nullptr, nullptr, nullptr, e->ns_img, nullptr, batch * cb, s));
            HIP_TRY(launch_ncsense_combine(e->ns_img, maps, map_n, L, l0, cb, e->nc, pv, mu, tact, q, partial, batch, s));
            p.end(2);
        } else {
            HIP_TRY(launch_ncsense_crop(e->ns_grid, maps, map_n, L, l0, cb, e->nc, pv, mu, tact, q, partial, batch, s));
        }
    }
    return PNP_OK;
}

// ---- off-resonance correction for multi-coil data (include/pnpadmm_offres_mc.h) ----------------------------
// coils per block: the knob, else the block that measured fastest under the live plan's interpolator (profiles/offres_mc_bench.json)
int om_block_of(const pnp_engine* e, int coils) {
    const int b = e->om_block > 0 ? e->om_block : e->orp.kind == 2 ? kOffresMcBlock : kOffresMcBlockLinear;
    return coils < b ? coils : b;
}
// one coil's plane of a block buffer [batch, cb, len] <-> a contiguous [batch, len]
int om_copy_out(float2* blk, int cb, int j, const float2* line, size_t len, int batch, hipStream_t s) {
    HIP_TRY(hipMemcpy2DAsync(blk + (size_t)j * len, (size_t)cb * len * sizeof(float2), line, len * sizeof(float2), len * sizeof(float2), (size_t)batch,
                             hipMemcpyDeviceToDevice, s));
    return PNP_OK;
}
int om_copy_in(float2* line, const float2* blk, int cb, int j, size_t len, int batch, hipStream_t s) {
    HIP_TRY(hipMemcpy2DAsync(line, len * sizeof(float2), blk + (size_t)j * len, (size_t)cb * len * sizeof(float2), len * sizeof(float2), (size_t)batch,
                             hipMemcpyDeviceToDevice, s));
    return PNP_OK;
}
// blk [batch, cb, M] = the samples of the coils c0 .. c0 + cb - 1 of A src, segment block by segment block: a sample's blend continues
// through blk.  Composed: per coil the image S_c . src, the single-coil forward at batch `batch`, a strided copy
int om_forward_block(pnp_engine* e, const float2* src, const float* src_real, const float2* maps, int map_n, const float2* sens, int sens_n, int C,
                     int c0, int cb, int batch, float2* blk, hipStream_t s) {
    const int L = e->orp.segments, B = or_block_of(e);
    const size_t M = (size_t)e->nc.m;
    const bool ls = e->orp.kind == 2;
    if (e->om_naive & ORM_PAD) {
        for (int j = 0; j < cb; ++j) {
            {
                Prof p(e, s, PROF_OTHER, -1);
                HIP_TRY(launch_ncsense_expand(src, src_real, sens, sens_n, C, c0 + j, 1, e->nc, e->om_img, batch, s));
            }
            if (int rc = or_forward(e, e->om_img, nullptr, maps, map_n, batch, cb == 1 ? blk : e->om_line, s)) return rc;
            if (cb != 1)
                if (int rc = om_copy_out(blk, cb, j, e->om_line, M, batch, s)) return rc;
        }
        return PNP_OK;
    }
    for (int l0 = 0; l0 < L; l0 += B) {
        const int sb = std::min(B, L - l0);
        {
            Prof p(e, s, PROF_OTHER, -1);
            HIP_TRY(launch_offres_mc_pad(src, src_real, sens, sens_n, C, c0, cb, maps, map_n, L, l0, sb, e->nc, e->ns_grid, batch, s));
        }
        if (int rc = nc_fft(e, e->ns_grid, batch * cb * sb, 0, s)) return rc;
        Prof p(e, s, PROF_OTHER, -1);
        if (or_naive_of(e) & OR_GATHER) {                  // the plan's gather ships composed: every plane's samples, then the blend
            if (e->ns_naive & NS_GATHER) HIP_TRY(launch_nufft_interp(e->ns_grid, e->nc, e->ns_samp, batch * cb * sb, s));
            else HIP_TRY(launch_ncsense_interp(e->ns_grid, e->nc, e->ns_samp, sb, 0, sb, batch * cb, s));
            if (ls) HIP_TRY(launch_offres_ls_blend(e->ns_samp, e->orp, e->nc, blk, l0, sb, batch * cb, s));
            else HIP_TRY(launch_offres_blend(e->ns_samp, e->orp, e->nc, blk, l0, sb, batch * cb, s));
            p.end(2);
        } else if (ls) {
            HIP_TRY(launch_offres_ls_interp(e->ns_grid, e->orp, e->nc, blk, l0, sb, batch * cb, s));
        } else {
            HIP_TRY(launch_offres_interp(e->ns_grid, e->orp, e->nc, blk, l0, sb, batch * cb, s));
        }
    }
    return PNP_OK;
}
// q (+)= sum over the block's coils of conj(S_c) . A_1^H(w . blk[., j]), A_1 the single-coil operator; blk: [batch, cb, M].  The coil chain
// is carried from block to block through q; the last block adds mu pv and leaves the partial sums of Re<pv, q> (pv, mu, tact, partial may
// be nullptr).  Composed: the single-coil adjoint per coil into om_part, then the SENSE combine
int om_adjoint_block(pnp_engine* e, const float2* blk, const float* w, const float2* maps, int map_n, const float2* sens, int sens_n, int C, int c0,
                     int cb, int batch, const float2* pv, const float* mu, const float* tact, float2* q, double* partial, hipStream_t s) {
    const int L = e->orp.segments, B = or_block_of(e), H = e->cfg.h, W = e->cfg.w;
    const size_t M = (size_t)e->nc.m;
    const bool ls = e->orp.kind == 2;
    if (e->om_naive & ORM_CROP) {
        for (int j = 0; j < cb; ++j) {
            const float2* yj = blk;
            if (cb != 1) {
                if (int rc = om_copy_in(e->om_line, blk, cb, j, M, batch, s)) return rc;
                yj = e->om_line;
            }
            if (int rc = or_adjoint(e, yj, w, maps, map_n, batch, nullptr, nullptr, nullptr, cb == 1 ? e->om_part : e->om_img, nullptr, s)) return rc;
            if (cb != 1)
                if (int rc = om_copy_out(e->om_part, cb, j, e->om_img, (size_t)H * W, batch, s)) return rc;
        }
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_ncsense_combine(e->om_part, sens, sens_n, C, c0, cb, e->nc, pv, mu, tact, q, partial, batch, s));
        return PNP_OK;
    }
    for (int l0 = 0; l0 < L; l0 += B) {
        const int sb = std::min(B, L - l0);
        // the per-plan choices of or_adjoint, at batch `batch` cb
        const bool ragged = ls && e->tune.offres_ls_naive < 0 && sb % kOffresLsSub != 0;
        {
            Prof p(e, s, PROF_OTHER, -1);
            if ((or_naive_of(e) & OR_GRID) || ragged) {
                if (ls) HIP_TRY(launch_offres_ls_expand(blk, e->orp, e->nc, e->ns_samp, l0, sb, batch * cb, s));
                else HIP_TRY(launch_offres_expand(blk, e->orp, e->nc, e->ns_samp, l0, sb, batch * cb, s));
                if (e->ns_naive & NS_GRID) HIP_TRY(launch_nufft_grid(e->ns_samp, w, e->nc, e->ns_grid, batch * cb * sb, s));
                else HIP_TRY(launch_ncsense_grid(e->ns_samp, sb, 0, sb, w, e->nc, e->ns_grid, batch * cb, s));
                p.end(2);
            } else if (ls) {
                HIP_TRY(launch_offres_ls_grid(blk, w, e->orp, e->nc, e->ns_grid, l0, sb, batch * cb, s, !e->tune.offres_ls_noskip));
            } else {
                HIP_TRY(launch_offres_grid(blk, w, e->orp, e->nc, e->ns_grid, l0, sb, batch * cb, s, e->tune.offres_grid_filter));
            }
        }
        if (int rc = nc_fft(e, e->ns_grid, batch * cb * sb, 1, s)) return rc;
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_offres_mc_crop(e->ns_grid, sens, sens_n, C, c0, cb, maps, map_n, L, l0, sb, e->nc, e->om_part, pv, mu, tact, q, partial, batch,
                                      s));
    }
    return PNP_OK;
}
// out [batch, C, M] = A src, coil block by coil block (a block that is not all of C goes through om_samp and a 2-D copy)
int om_forward(pnp_engine* e, const float2* src, const float* src_real, const float2* maps, int map_n, const float2* sens, int sens_n, int C,
               int batch, float2* out, hipStream_t s) {
    const int B = om_block_of(e, C);
    const size_t M = (size_t)e->nc.m;
    for (int c0 = 0; c0 < C; c0 += B) {
        const int cb = std::min(B, C - c0);
        if (int rc = om_forward_block(e, src, src_real, maps, map_n, sens, sens_n, C, c0, cb, batch, cb == C ? out : e->om_samp, s)) return rc;
        if (cb != C)
            HIP_TRY(hipMemcpy2DAsync(out + (size_t)c0 * M, (size_t)C * M * sizeof(float2), e->om_samp, (size_t)cb * M * sizeof(float2),
                                     (size_t)cb * M * sizeof(float2), (size_t)batch, hipMemcpyDeviceToDevice, s));
    }
    return PNP_OK;
}
// q [batch, h, w] = A^H (w . y), y: [batch, C, M]
int om_adjoint(pnp_engine* e, const float2* y, const float* w, const float2* maps, int map_n, const float2* sens, int sens_n, int C, int batch,
               float2* q, hipStream_t s) {
    const int B = om_block_of(e, C);
    const size_t M = (size_t)e->nc.m;
    for (int c0 = 0; c0 < C; c0 += B) {
        const int cb = std::min(B, C - c0);
        if (cb != C)
            HIP_TRY(hipMemcpy2DAsync(e->om_samp, (size_t)cb * M * sizeof(float2), y + (size_t)c0 * M, (size_t)C * M * sizeof(float2),
                                     (size_t)cb * M * sizeof(float2), (size_t)batch, hipMemcpyDeviceToDevice, s));
        if (int rc = om_adjoint_block(e, cb == C ? y : e->om_samp, w, maps, map_n, sens, sens_n, C, c0, cb, batch, nullptr, nullptr, nullptr, q,
                                      nullptr, s))
            return rc;
    }
    return PNP_OK;
}

// ---- the one non-Cartesian operator ----------------------------------------------------------------------
// What a non-Cartesian operator is made of beyond the NUFFT plan: coil maps (coils == 0: single-coil) and the segment maps of a field map
// (maps == nullptr: unsegmented).  The four combinations are the four families above; every caller that serves them all goes through the
// op_* dispatchers below and never asks which family it has.
struct NcOp {
    int coils;
    const float2* sens;
    int sens_n;
    const float2* maps;
    int map_n;
};
// the live stage's operator: the installed constants
NcOp live_op(const pnp_engine* e) {
    const LiveStage& st = e->stage;
    return {st.coils, st.coils ? e->st_sens : nullptr, st.sens_n, stage_segmented(st.kind) ? e->st_maps : nullptr, st.map_n};
}
// out [batch, M] or [batch, C, M] = A src (src complex, or src_real: a real image)
int op_forward(pnp_engine* e, const NcOp& o, const float2* src, const float* src_real, int batch, float2* out, hipStream_t s) {
    if (o.coils) return o.maps ? om_forward(e, src, src_real, o.maps, o.map_n, o.sens, o.sens_n, o.coils, batch, out, s)
                               : ns_forward(e, src, src_real, o.sens, o.sens_n, o.coils, batch, out, s);
    return o.maps ? or_forward(e, src, src_real, o.maps, o.map_n, batch, out, s) : nc_forward(e, src, src_real, batch, out, s);
}
// q [batch, h, w] = A^H (w . y)
int op_adjoint(pnp_engine* e, const NcOp& o, const float2* y, const float* w, int batch, float2* q, hipStream_t s) {
    if (o.coils) return o.maps ? om_adjoint(e, y, w, o.maps, o.map_n, o.sens, o.sens_n, o.coils, batch, q, s)
                               : ns_adjoint(e, y, w, o.sens, o.sens_n, o.coils, batch, q, s);
    return o.maps ? or_adjoint(e, y, w, o.maps, o.map_n, batch, nullptr, nullptr, nullptr, q, nullptr, s)
                  : nc_adjoint(e, y, w, batch, nullptr, nullptr, nullptr, q, nullptr, s);
}
// a multi-coil operator's coils per block, and the scratch [N, cb, M] a block's samples go through
int op_block_of(const pnp_engine* e, const NcOp& o) { return o.maps ? om_block_of(e, o.coils) : ns_block_of(e, o.coils); }
float2* op_block_samp(const pnp_engine* e, const NcOp& o) { return o.maps ? e->om_samp : e->ns_samp; }
// blk [batch, cb, M] = the samples of the coils c0 .. c0 + cb - 1 of A src
int op_forward_block(pnp_engine* e, const NcOp& o, const float2* src, const float* src_real, int c0, int cb, int batch, float2* blk, hipStream_t s) {
    return o.maps ? om_forward_block(e, src, src_real, o.maps, o.map_n, o.sens, o.sens_n, o.coils, c0, cb, batch, blk, s)
                  : ns_forward_block(e, src, src_real, o.sens, o.sens_n, o.coils, c0, cb, batch, blk, cb, 0, s);
}
// q (+)= the block's part of A^H (w . blk); the last block adds mu pv and leaves the partial sums of Re<pv, q>
int op_adjoint_block(pnp_engine* e, const NcOp& o, const float2* blk, const float* w, int c0, int cb, int batch, const float2* pv, const float* mu,
                     const float* tact, float2* q, double* partial, hipStream_t s) {
    return o.maps ? om_adjoint_block(e, blk, w, o.maps, o.map_n, o.sens, o.sens_n, o.coils, c0, cb, batch, pv, mu, tact, q, partial, s)
                  : ns_adjoint_block(e, blk, cb, 0, w, o.sens, o.sens_n, o.coils, c0, cb, batch, pv, mu, tact, q, partial, s);
}
// q = A^H W A pv + mu pv by the gridding pair; the partial sums of Re<pv, q> go to mc_part.  Single-coil: A pv goes through nc_samp whole (a
// segmented blend joins neighbouring segments) before the adjoint starts.  Multi-coil: coil block by coil block, a block's samples go through
// the block scratch and are gridded before the next block's replace them.  Stopped slices: only the launches that write q skip them
int op_normal(pnp_engine* e, const NcOp& o, const float* w, const float2* pv, const float* mu, const float* tact, float2* q, hipStream_t s) {
    const int N = e->cfg.n;
    if (!o.coils) {
        if (int rc = op_forward(e, o, pv, nullptr, N, e->nc_samp, s)) return rc;
        return o.maps ? or_adjoint(e, e->nc_samp, w, o.maps, o.map_n, N, pv, mu, tact, q, e->mc_part, s)
                      : nc_adjoint(e, e->nc_samp, w, N, pv, mu, tact, q, e->mc_part, s);
    }
    const int C = o.coils, B = op_block_of(e, o);
    float2* const blk = op_block_samp(e, o);
    for (int c0 = 0; c0 < C; c0 += B) {
        const int cb = std::min(B, C - c0);
        if (int rc = op_forward_block(e, o, pv, nullptr, c0, cb, N, blk, s)) return rc;
        if (int rc = op_adjoint_block(e, o, blk, w, c0, cb, N, pv, mu, tact, q, e->mc_part, s)) return rc;
    }
    return PNP_OK;
}
// the partial sums of sum_m w_m |(A x)_m - y_m|^2 (summed over the coils) into dcpart: A x into the sample scratch - whole, or coil block by
// coil block with the coil-major sums in between
int op_misfit(pnp_engine* e, const NcOp& o, const float* x, const float2* y, const float* w, double* mpart, double* dcpart, hipStream_t s) {
    const int N = e->cfg.n;
    if (!o.coils) {
        if (int rc = op_forward(e, o, nullptr, x, N, e->nc_samp, s)) return rc;
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_nufft_misfit(e->nc_samp, y, w, e->nc, mpart, dcpart, N, s));
        return PNP_OK;
    }
    const int C = o.coils, B = op_block_of(e, o);
    float2* const blk = op_block_samp(e, o);
    for (int c0 = 0; c0 < C; c0 += B) {
        const int cb = std::min(B, C - c0);
        if (int rc = op_forward_block(e, o, nullptr, x, c0, cb, N, blk, s)) return rc;
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_ncsense_misfit(blk, y, w, C, c0, cb, e->nc, mpart, N, s));
    }
    Prof p(e, s, PROF_OTHER, -1);
    HIP_TRY(launch_ncsense_misfit_sum(mpart, C, e->nc, dcpart, N, s));
    return PNP_OK;
}
// ---- Toeplitz normal operator (include/pnpadmm_toeplitz.h) ----------------------------------------------
// q [planes, h, w] = crop(ifft2c(K . fft2c(pad(src)))) (+ mu pv with the partial sums of Re<pv, q>: the last launch's epilogue), through
// tz_grid.  Three fused launches, or the seven composed ones; src may be q (the grid lies between them).  Stopped slices: only the last
// launch skips them
int tz_apply(pnp_engine* e, const float2* src, int planes, const float2* pv, const float* mu, const float* tact, float2* q, double* partial,
             hipStream_t s) {
    const int H = e->cfg.h, W = e->cfg.w;
    if (e->tz_fused) {
        {
            Prof p(e, s, PROF_FFT_ROWS, -1);
            HIP_TRY(launch_toeplitz_rows_fwd(src, e->tz_grid, e->tz_tw_w, planes, H, W, s));
        }
        {
            Prof p(e, s, PROF_FFT_COLS, -1);
            HIP_TRY(launch_toeplitz_cols(e->tz_grid, e->tz_k, e->tz_tw_h, planes, H, W, s));
        }
        Prof p(e, s, PROF_FFT_ROWS, -1);
        HIP_TRY(launch_toeplitz_rows_inv(e->tz_grid, e->tz_tw_w, pv, mu, tact, q, partial, planes, H, W, s));
        return PNP_OK;
    }
    const auto fft = [&](int inverse) { return grid_fft(e, e->tz_grid, e->tz_tw_h, e->tz_tw_w, planes, 2 * H, 2 * W, inverse, s); };
    {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_toeplitz_pad(src, e->tz_grid, H, W, planes, s));
    }
    if (int rc = fft(0)) return rc;
    {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_toeplitz_mul(e->tz_grid, e->tz_k, H, W, planes, s));
    }
    if (int rc = fft(1)) return rc;
    Prof p(e, s, PROF_OTHER, -1);
    HIP_TRY(launch_toeplitz_crop(e->tz_grid, pv, mu, tact, q, partial, H, W, planes, s));
    return PNP_OK;
}
// out [batch, h, w] (+)= sum over the coils of conj(S_c) . Toep(S_c . src), block by block through ns_img; the last block adds mu pv and leaves
// the partial sums of Re<pv, out> (pv, mu, tact, partial may be nullptr)
int tz_apply_mc(pnp_engine* e, const float2* src, const float2* sens, int sens_n, int C, int batch, const float2* pv, const float* mu,
                const float* tact, float2* out, double* partial, hipStream_t s) {
    const int B = ns_block_of(e, C);
    for (int c0 = 0; c0 < C; c0 += B) {
        const int cb = std::min(B, C - c0);
        {
            Prof p(e, s, PROF_OTHER, -1);
            HIP_TRY(launch_ncsense_expand(src, nullptr, sens, sens_n, C, c0, cb, e->nc, e->ns_img, batch, s));
        }
        if (int rc = tz_apply(e, e->ns_img, batch * cb, nullptr, nullptr, nullptr, e->ns_img, nullptr, s)) return rc;
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_ncsense_combine(e->ns_img, sens, sens_n, C, c0, cb, e->nc, pv, mu, tact, out, partial, batch, s));
    }
    return PNP_OK;
}

// ---- Toeplitz form of the off-resonance operator (include/pnpadmm_offres_tz.h) ------------------------------
// slices per block of an application over `batch` slices: all L planes of a slice are in flight for the mix
int otz_slice_block(const pnp_engine* e, int batch) {
    const int L = e->orp.segments;
    int nb = e->otz_slices > 0 ? e->otz_slices : std::max(1, kOffresTzPlanes / L);
    nb = std::min(nb, std::max(1, 16384 / L));              // (planes index a launch grid's y)
    return std::min(nb, batch);
}
// q [batch, h, w] = sum_l conj(E_l) . crop(ifft2c(sum_l' K_ll' . fft2c(pad(E_l' . src)))) (+ mu pv with the partial sums of Re<pv, q>: the
// combine's epilogue; pv, mu, tact, partial may be nullptr), slice block by slice block through otz_img, otz_x and otz_y.  src may be q: a
// block's slices are read by its first launch and written by its last.  Stopped slices: only the combine skips them
int otz_apply(pnp_engine* e, const float2* src, const float2* maps, int map_n, int batch, const float2* pv, const float* mu, const float* tact,
              float2* q, double* partial, hipStream_t s) {
    const int H = e->cfg.h, W = e->cfg.w, L = e->orp.segments, kind = e->orp.kind;
    const size_t hw = (size_t)H * W;
    const int NB = otz_slice_block(e, batch), chunks = pixel_chunks(H, W);
    for (int n0 = 0; n0 < batch; n0 += NB) {
        const int nb = std::min(NB, batch - n0), planes = nb * L;
        const float2* mb = map_n == 1 ? maps : maps + (size_t)n0 * L * hw;
        {
            Prof p(e, s, PROF_OTHER, -1);
            HIP_TRY(launch_ncsense_expand(src + (size_t)n0 * hw, nullptr, mb, map_n, L, 0, L, e->nc, e->otz_img, nb, s));
        }
        if (e->otz_fused) {
            {
                Prof p(e, s, PROF_FFT_ROWS, -1);
                HIP_TRY(launch_toeplitz_rows_fwd(e->otz_img, e->otz_y, e->otz_tw_w, planes, H, W, s));
            }
            {
                Prof p(e, s, PROF_FFT_COLS, -1);
                HIP_TRY(launch_offres_tz_cols_fwd(e->otz_y, e->otz_x, e->otz_tw_h, planes, H, W, s));
            }
            {
                Prof p(e, s, PROF_OTHER, -1);
                HIP_TRY(launch_offres_tz_mix(e->otz_x, e->otz_y, e->otz_k, kind, L, H, W, nb, 1.f / (4.f * (float)H * (float)W), s));
            }
            {
                Prof p(e, s, PROF_FFT_COLS, -1);
                HIP_TRY(launch_offres_tz_cols_inv(e->otz_y, e->otz_x, e->otz_tw_h, planes, H, W, s));
            }
            Prof p(e, s, PROF_FFT_ROWS, -1);
            HIP_TRY(launch_toeplitz_rows_inv(e->otz_x, e->otz_tw_w, nullptr, nullptr, nullptr, e->otz_img, nullptr, planes, H, W, s));
        } else {
            const auto fft = [&](float2* grid, int inverse) { return grid_fft(e, grid, e->otz_tw_h, e->otz_tw_w, planes, 2 * H, 2 * W, inverse, s); };
            {
                Prof p(e, s, PROF_OTHER, -1);
                HIP_TRY(launch_toeplitz_pad(e->otz_img, e->otz_x, H, W, planes, s));
            }
            if (int rc = fft(e->otz_x, 0)) return rc;
            {
                Prof p(e, s, PROF_OTHER, -1);
                HIP_TRY(launch_offres_tz_mix(e->otz_x, e->otz_y, e->otz_k, kind, L, H, W, nb, 1.f, s));
            }
            if (int rc = fft(e->otz_y, 1)) return rc;
            Prof p(e, s, PROF_OTHER, -1);
            HIP_TRY(launch_toeplitz_crop(e->otz_y, nullptr, nullptr, nullptr, e->otz_img, nullptr, H, W, planes, s));
        }
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_ncsense_combine(e->otz_img, mb, map_n, L, 0, L, e->nc, pv ? pv + (size_t)n0 * hw : nullptr, mu ? mu + n0 : nullptr,
                                       tact ? tact + n0 : nullptr, q + (size_t)n0 * hw, partial ? partial + (size_t)n0 * chunks * 2 : nullptr, nb, s));
    }
    return PNP_OK;
}
// coils per block of the multi-coil application: the coil block of the multi-coil off-resonance stage while the segment maps are shared; with
// per-slice maps a coil image's slice must stay the slice of its maps, so the coils go one at a time
int otz_coil_block(const pnp_engine* e, int coils, int map_n) { return map_n == 1 ? om_block_of(e, coils) : 1; }
// out [batch, h, w] = sum over the coils of conj(S_c) . [otz_apply](S_c . src), block by block in place in otz_cimg; the coil chain is
// carried through out, the last block adds mu pv and leaves the partial sums of Re<pv, out>
int otz_apply_mc(pnp_engine* e, const float2* src, const float2* maps, int map_n, const float2* sens, int sens_n, int C, int batch, const float2* pv,
                 const float* mu, const float* tact, float2* out, double* partial, hipStream_t s) {
    const int B = otz_coil_block(e, C, map_n);
    for (int c0 = 0; c0 < C; c0 += B) {
        const int cb = std::min(B, C - c0);
        {
            Prof p(e, s, PROF_OTHER, -1);
            HIP_TRY(launch_ncsense_expand(src, nullptr, sens, sens_n, C, c0, cb, e->nc, e->otz_cimg, batch, s));
        }
        if (int rc = otz_apply(e, e->otz_cimg, maps, map_n, batch * cb, nullptr, nullptr, nullptr, e->otz_cimg, nullptr, s)) return rc;
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_ncsense_combine(e->otz_cimg, sens, sens_n, C, c0, cb, e->nc, pv, mu, tact, out, partial, batch, s));
    }
    return PNP_OK;
}
// the live non-Cartesian stage's normal operator in its three forms: q = A^H W A pv + mu pv, the partial sums of Re<pv, q> in mc_part
int grid_normal(pnp_engine* e, const float2* pv, const float* mu, const float* tact, float2* q, hipStream_t s) {
    return op_normal(e, live_op(e), stage_w(e), pv, mu, tact, q, s);
}
int tz_normal(pnp_engine* e, const float2* pv, const float* mu, const float* tact, float2* q, hipStream_t s) {
    const NcOp o = live_op(e);
    return o.coils ? tz_apply_mc(e, pv, o.sens, o.sens_n, o.coils, e->cfg.n, pv, mu, tact, q, e->mc_part, s)
                   : tz_apply(e, pv, e->cfg.n, pv, mu, tact, q, e->mc_part, s);
}
int otz_normal(pnp_engine* e, const float2* pv, const float* mu, const float* tact, float2* q, hipStream_t s) {
    const NcOp o = live_op(e);
    return o.coils ? otz_apply_mc(e, pv, o.maps, o.map_n, o.sens, o.sens_n, o.coils, e->cfg.n, pv, mu, tact, q, e->mc_part, s)
                   : otz_apply(e, pv, o.maps, o.map_n, e->cfg.n, pv, mu, tact, q, e->mc_part, s);
}
// the K-step CG solve of (A^H A + mu I) z = A^H y + mu (x + u), warm-started from z, then u <- u + x - z; `normal`: the stage's normal
// operator (mc_normal: the coil operator; grid_normal, tz_normal, otz_normal: the non-Cartesian stage's three forms), which also leaves the partial sums of Re<p, q> in mc_part
using NormalOp = int (*)(pnp_engine*, const float2*, const float*, const float*, float2*, hipStream_t);
// the live stage's normal operator, run stage.cg times per step (nullptr: the stage has none - the closed form, or nothing installed)
NormalOp stage_normal(const pnp_engine* e) {
    if (e->stage.kind == STAGE_MC) return mc_normal;
    if (!stage_noncart(e->stage.kind)) return nullptr;
    return e->stage.form == FORM_TZ ? tz_normal : e->stage.form == FORM_OTZ ? otz_normal : grid_normal;
}
int run_prox_dual_cg(pnp_engine* e, NormalOp normal, int iters, const float* mu, const float* tact, const float* x, float2* z, float2* u,
                     hipStream_t s) {
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w;
    int rc;
    if ((rc = normal(e, z, mu, tact, mc_q(e), s))) return rc;
    {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_sense_cg_init(mc_aty(e), x, u, mc_q(e), mu, tact, mc_r(e), mc_p(e), e->mc_part, N, H, W, s));
        HIP_TRY(launch_sense_scalar(e->mc_part, 0, tact, e->mc_sc, N, H, W, s));
        p.end(2);
    }
    for (int k = 0; k < iters; ++k) {
        if ((rc = normal(e, mc_p(e), mu, tact, mc_q(e), s))) return rc;
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_sense_scalar(e->mc_part, 1, tact, e->mc_sc, N, H, W, s));
        HIP_TRY(launch_sense_cg_update(z, mc_r(e), mc_p(e), mc_q(e), e->mc_sc, tact, e->mc_part, N, H, W, s));
        HIP_TRY(launch_sense_scalar(e->mc_part, 2, tact, e->mc_sc, N, H, W, s));
        HIP_TRY(launch_sense_cg_dir(mc_r(e), mc_p(e), e->mc_sc, tact, N, H, W, s));
        p.end(4);
    }
    Prof p(e, s, PROF_OTHER, -1);
    HIP_TRY(launch_sense_dual(x, z, u, tact, N, H, W, s));
    return PNP_OK;
}

// Grow buffers of the handle's workspace: the one contract of every entry point that allocates inside the call (include/pnpadmm.h).  A slot
// grows when it needs more bytes than it holds (cap == nullptr: a buffer that is never replaced; its caller asks for its fixed size while the
// slot is null and for 0 afterwards).  Nothing to grow: PNP_OK without a HIP call.  All-or-nothing: every new buffer is allocated, and
// zero-filled where asked, before any old one is released, and on failure the new ones are freed and the handle keeps the workspace it had.
// Buffers that grow lose their contents (their callers rewrite them).
struct WsSlot { void** ptr; size_t* cap; size_t need; bool zero; };
int ws_grow(pnp_engine* e, const char* label, std::initializer_list<WsSlot> slots) {
    void* fresh[10] = {};                                  // pnp_nufft_plan's ten slots are the most
    const auto held = [](const WsSlot& q) { return q.cap ? *q.cap : 0; };
    const auto undo = [&] { for (void* f : fresh) (void)hipFree(f); };   // hipFree(nullptr) is a no-op
    bool any = false, replaces = false;
    size_t i = 0;
    for (const WsSlot& q : slots) {
        void*& f = fresh[i++];
        if (q.need <= held(q)) continue;
        any = true;
        replaces |= *q.ptr != nullptr;
        if (hipMalloc(&f, q.need) != hipSuccess) {
            f = nullptr;
            undo();
            return fail(PNP_ERR_NOMEM, "%s: %zu bytes (the handle keeps the workspace it had)", label, q.need);
        }
    }
    if (!any) return PNP_OK;
    i = 0;
    for (const WsSlot& q : slots) {
        void* f = fresh[i++];
        if (f && q.zero && hipMemset(f, 0, q.need) != hipSuccess) {
            undo();
            return fail(PNP_ERR_HIP, "%s: hipMemset failed", label);
        }
    }
    if (replaces) (void)hipDeviceSynchronize();            // no launch still reads a buffer being replaced
    i = 0;
    for (const WsSlot& q : slots) {
        void* f = fresh[i++];
        if (!f) continue;
        (void)hipFree(*q.ptr);
        *q.ptr = f;
        e->ws_bytes += q.need - held(q);
        if (q.cap) *q.cap = q.need;
    }
    return PNP_OK;
}

// The coil workspace: `y_need`, `work_need`, `sens_need` complex elements (0: leave that buffer alone) and the per-slice vectors
int mc_ensure(pnp_engine* e, size_t y_need, size_t work_need, size_t sens_need) {
    const size_t px = (size_t)e->cfg.n * e->cfg.h * e->cfg.w;
    const size_t part_bytes = (size_t)e->cfg.n * pixel_chunks(e->cfg.h, e->cfg.w) * 2 * sizeof(double), sc_bytes = (size_t)e->cfg.n * 8 * sizeof(double);
    return ws_grow(e, "coil workspace", {{(void**)&e->mc_y, &e->mc_y_cap, y_need * sizeof(float2), false},
                                        {(void**)&e->mc_work, &e->mc_work_cap, work_need * sizeof(float2), false},
                                        {(void**)&e->mc_sens, &e->mc_sens_cap, sens_need * sizeof(float2), false},
                                        {(void**)&e->mc_vec, nullptr, e->mc_vec ? 0 : 4 * px * sizeof(float2), false},
                                        {(void**)&e->mc_part, nullptr, e->mc_part ? 0 : part_bytes, false},
                                        {(void**)&e->mc_sc, nullptr, e->mc_sc ? 0 : sc_bytes, true}});
}

// argument errors shared by the three multi-coil entry points that take maps and a mask: before any HIP call
// (the scalar ranges come first and need no handle: they are reported whatever else is wrong)
int mc_check_scalars(const char* fn, int coils, int sens_n, int mask_n) {
    if (coils < 1 || coils > PNP_MC_MAX_COILS) return fail(PNP_ERR_INVALID, "%s: coils must be 1..%d (got %d)", fn, PNP_MC_MAX_COILS, coils);
    if (sens_n < 1) return fail(PNP_ERR_INVALID, "%s: sens_n must be 1 or n (got %d)", fn, sens_n);
    if (mask_n < 1) return fail(PNP_ERR_INVALID, "%s: mask_n must be 1 or n (got %d)", fn, mask_n);
    return PNP_OK;
}
int mc_check(const char* fn, pnp_engine* e, int coils, int sens_n, int mask_n) {
    const int N = e->cfg.n;
    if (sens_n != 1 && sens_n != N) return fail(PNP_ERR_INVALID, "%s: sens_n must be 1 or n=%d", fn, N);
    if (mask_n != 1 && mask_n != N) return fail(PNP_ERR_INVALID, "%s: mask_n must be 1 or n=%d", fn, N);
    if (int rc = check_kspace_sizes(fn, e)) return rc;
    if ((long long)N * coils > 65535) return fail(PNP_ERR_INVALID, "%s: n * coils must be <= 65535 (got %d * %d)", fn, N, coils);
    return PNP_OK;
}

// The one way a stage becomes live: an installer's last statement, after its last launch was accepted.  A failed HIP call inside an
// installer therefore leaves the handle in the stage it had (its CG vectors and, for the Cartesian stages, its mask are rewritten by the
// next install); nothing between an installer's first launch and this line reads the record - the launches take the new constants as arguments.
void commit_stage(pnp_engine* e, const LiveStage& st) { e->stage = st; }
// The four plan calls that replace what a live stage was built on: the stage loses its constants with it.  pnp_nufft_plan: every
// non-Cartesian stage (DROP_NONCART); pnp_offres_plan / pnp_offres_plan_ls: the segmented ones (DROP_SEGMENTED); pnp_toeplitz_plan and
// pnp_offres_tz_plan: the stages whose CG runs on that spectrum (DROP_FORM with the form).  The closed-form and SENSE stages use none of
// these and stay.
enum StageDrop { DROP_NONCART, DROP_SEGMENTED, DROP_FORM };
void drop_stage(pnp_engine* e, StageDrop what, StageForm form = FORM_GRID) {
    const LiveStage& st = e->stage;
    if (!stage_noncart(st.kind)) return;
    if (what == DROP_NONCART || (what == DROP_SEGMENTED && stage_segmented(st.kind)) || (what == DROP_FORM && st.form == form)) e->stage = LiveStage{};
}

// pnp_set_kspace (no iterate) / pnp_reset: the closed-form stage's constants
int cart_install(const char* fn, pnp_engine* e, bool with_iterate, const float2* x0, const float2* y0, const uint8_t* mask, int mask_n, float* x,
                 float2* z, float2* u, hipStream_t s) {
    if (!e || !y0 || !mask || (with_iterate && (!x0 || !x || !z || !u))) return fail(PNP_ERR_INVALID, "%s: null argument", fn);
    if (mask_n != 1 && mask_n != e->cfg.n) return fail(PNP_ERR_INVALID, "%s: mask_n must be 1 or n=%d", fn, e->cfg.n);
    if (int rc = check_kspace_sizes(fn, e)) return rc;
    PNP_ON_DEVICE(e);
    e->mask_n = mask_n;
    HIP_TRY(launch_reset(x0, y0, mask, mask_n, x, z, u, e->d_y0s, e->d_masks, e->cfg.n, e->cfg.h, e->cfg.w, s));
    commit_stage(e, {STAGE_CART});
    return PNP_OK;
}

// pnp_set_kspace_mc (no iterate) / pnp_reset_mc: the SENSE stage's constants.  Every rejection happens before any HIP call; scalar ranges first
int mc_install(const char* fn, pnp_engine* e, bool with_iterate, const float2* x0, const float2* y0, const float2* sens, int coils, int sens_n,
               const uint8_t* mask, int mask_n, int cg_iters, float* x, float2* z, float2* u, hipStream_t s) {
    if (cg_iters < 1 || cg_iters > PNP_MC_MAX_CG) return fail(PNP_ERR_INVALID, "%s: cg_iters must be 1..%d (got %d)", fn, PNP_MC_MAX_CG, cg_iters);
    int rc;
    if ((rc = mc_check_scalars(fn, coils, sens_n, mask_n))) return rc;
    if (with_iterate && !x0) return fail(PNP_ERR_INVALID, "%s: null x0", fn);
    if (!y0) return fail(PNP_ERR_INVALID, "%s: null y0", fn);
    if (!sens) return fail(PNP_ERR_INVALID, "%s: null sens", fn);
    if (!mask) return fail(PNP_ERR_INVALID, "%s: null mask", fn);
    if (with_iterate && (!x || !z || !u)) return fail(PNP_ERR_INVALID, "%s: null x, z or u", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if ((rc = mc_check(fn, e, coils, sens_n, mask_n))) return rc;
    PNP_ON_DEVICE(e);
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w;
    const size_t hw = (size_t)H * W, img = (size_t)N * coils * hw, sn = (size_t)sens_n * coils * hw;
    if ((rc = mc_ensure(e, img, img, sn))) return rc;
    HIP_TRY(hipMemcpyAsync(e->mc_sens, sens, sn * sizeof(float2), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemsetAsync(e->mc_sc, 0, (size_t)N * 8 * sizeof(double), s));
    e->mask_n = mask_n;
    {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_sense_install(y0, mask, mask_n, coils, e->mc_y, e->mc_work, e->d_masks, N, H, W, s));
    }
    // aty = A^H y = sum_c conj(S_c) IFFT(masked ys_c)
    if ((rc = plain_fft2(e, e->mc_work, e->mc_work, N * coils, 1, s))) return rc;
    {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_sense_combine(e->mc_work, e->mc_sens, sens_n, coils, nullptr, nullptr, nullptr, mc_aty(e), nullptr, N, H, W, s));
    }
    if (with_iterate) {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_sense_iterate(x0, x, z, u, N, H, W, s));
    }
    commit_stage(e, {STAGE_MC, FORM_GRID, coils, sens_n, cg_iters});
    return PNP_OK;
}

// The workspace of pnp_estimate_sens: the maxima / smax buffer and, with `own_rss`, the rss plane
int cm_ensure(pnp_engine* e, bool own_rss) {
    const size_t max_bytes = (size_t)e->cfg.n * (pixel_chunks(e->cfg.h, e->cfg.w) + 1) * sizeof(float);
    const size_t rss_bytes = (size_t)e->cfg.n * e->cfg.h * e->cfg.w * sizeof(float);
    return ws_grow(e, "coil map workspace", {{(void**)&e->cm_max, nullptr, e->cm_max ? 0 : max_bytes, false},
                                            {(void**)&e->cm_rss, nullptr, own_rss && !e->cm_rss ? rss_bytes : 0, false}});
}

// The workspace of pnp_coil_compress_matrix: `part_need` complex128 Gram partials and, for callers that pass no Gram, `gram_need` more
int cc_ensure(pnp_engine* e, size_t part_need, size_t gram_need) {
    return ws_grow(e, "coil compression workspace", {{(void**)&e->cc_part, &e->cc_part_cap, part_need * sizeof(double2), false},
                                                    {(void**)&e->cc_gram, &e->cc_gram_cap, gram_need * sizeof(double2), false}});
}

// The workspace of pnp_noise_cov: `need` complex128 covariance partials
int pw_ensure(pnp_engine* e, size_t need) {
    return ws_grow(e, "noise covariance workspace", {{(void**)&e->pw_part, &e->pw_part_cap, need * sizeof(double2), false}});
}

// The workspace of pnp_espirit_sens beyond cm_ensure's: one buffer of `need` bytes
int es_ensure(pnp_engine* e, size_t need) { return ws_grow(e, "ESPIRiT workspace", {{&e->es_ws, &e->es_cap, need, false}}); }

// The workspace of pnp_grappa_weights: `need` complex128 entries
int gr_ensure(pnp_engine* e, size_t need) {
    return ws_grow(e, "GRAPPA workspace", {{(void**)&e->gr_ws, &e->gr_cap, need * sizeof(double2), false}});
}

// The workspace of the total-variation denoiser: one (py, px) plane
int tv_ensure(pnp_engine* e) {
    const size_t bytes = (size_t)e->cfg.n * e->cfg.h * e->cfg.w * sizeof(float2);
    return ws_grow(e, "total-variation workspace", {{(void**)&e->tv_p, nullptr, e->tv_p ? 0 : bytes, false}});
}

// out = TV(v, scale * lam, iters), v = the plane `v` or Re z - Re u.  p travels between launches through two planes in turn: the
// data-fidelity stage's scratch plane (free while the x-update runs; calls on one handle are stream-ordered) and tv_p.  No launch writes
// a plane that another workgroup of it reads: when out aliases v the last fused launch stores p and tv_close_kernel ends the call.
int run_tv(pnp_engine* e, const float* v, const float2* z, const float2* u, const float* lam, float scale, const float* tact, int iters,
           float* out, hipStream_t s) {
    const int N = e->cfg.n;
    if (int rc = tv_ensure(e)) return rc;
    float2* const buf[2] = {e->d_work, e->tv_p};
    TvArgs a{};
    a.v = v; a.z = z; a.u = u; a.lam = lam; a.scale = scale; a.tact = tact; a.H = e->cfg.h; a.W = e->cfg.w;
    Prof p(e, s, PROF_OTHER, -1, true, true);
    int launches = 0;
    const bool alias = v != nullptr && v == out;
    const int L = e->tune.tv_naive ? iters : (iters + kTvT - 1) / kTvT;
    for (int l = 0; l < L; ++l) {
        a.p_in = l == 0 ? nullptr : buf[l & 1];
        a.p_out = buf[(l + 1) & 1];
        a.out = nullptr;
        ++launches;
        if (e->tune.tv_naive) { HIP_TRY(launch_tv_iter(a, N, s)); continue; }
        a.iters = iters - l * kTvT < kTvT ? iters - l * kTvT : kTvT;
        if (l == L - 1 && !alias) { a.p_out = nullptr; a.out = out; }
        HIP_TRY(launch_tv_fused(a, N, s));
    }
    if (e->tune.tv_naive || alias) {
        a.p_in = buf[L & 1]; a.p_out = nullptr; a.out = out;
        ++launches;
        HIP_TRY(launch_tv_close(a, N, s));
    }
    p.end(launches);
    return PNP_OK;
}

// The planes of the naive Haar form: a_1 .. a_(J-1) and the residual's ping-pong pair, never replaced
constexpr int kHaarNaivePlanes = PNP_HAAR_MAX_LEVELS - 1 + 2;
static_assert(PNP_HAAR_MAX_LEVELS == kHaarMaxLevels, "the header's limit is the kernels'");
int haar_ensure(pnp_engine* e) {
    const size_t bytes = (size_t)e->cfg.n * e->cfg.h * e->cfg.w * sizeof(float) * kHaarNaivePlanes;
    return ws_grow(e, "Haar workspace", {{(void**)&e->haar_ws, nullptr, e->haar_ws ? 0 : bytes, false}});
}

// out = Haar(v, scale * lam, levels, mode), v = the plane `v` or Re z - Re u.  ORTHO is one launch whose threads read and write their own
// pixel.  A TI launch reads the halo of its neighbours' tiles, so it never writes the plane it reads: when out aliases v it writes the
// data-fidelity stage's scratch plane (free while the x-update runs; calls on one handle are stream-ordered) and a copy ends the call.
int run_haar(pnp_engine* e, const float* v, const float2* z, const float2* u, const float* lam, float scale, const float* tact, int levels,
             int mode, float* out, hipStream_t s) {
    const int N = e->cfg.n;
    const size_t px = (size_t)N * e->cfg.h * e->cfg.w;
    const bool ti = mode == PNP_HAAR_TI, naive = ti && e->tune.haar_naive;
    if (naive)
        if (int rc = haar_ensure(e)) return rc;
    HaarArgs a{};
    a.v = v; a.z = z; a.u = u; a.lam = lam; a.scale = scale; a.tact = tact; a.H = e->cfg.h; a.W = e->cfg.w; a.levels = levels;
    const bool alias = ti && v != nullptr && v == out;
    a.out = alias ? (float*)e->d_work : out;
    Prof p(e, s, PROF_OTHER, -1, true, true);
    int launches = 1;
    if (!ti) {
        HIP_TRY(launch_haar_ortho(a, N, s));
    } else if (!naive) {
        HIP_TRY(launch_haar_ti_fused(a, N, s));
    } else {
        const auto plane = [&](int i) { return e->haar_ws + (size_t)i * px; };
        launches = 0;
        for (int j = 1; j < levels; ++j, ++launches) {             // a_j into plane j - 1
            a.level = j; a.a_src = j > 1 ? plane(j - 2) : nullptr; a.a_dst = plane(j - 1);
            HIP_TRY(launch_haar_ti_down(a, N, s));
        }
        for (int j = levels; j >= 1; --j, ++launches) {            // r_(j-1) from r_j, through the last two planes in turn
            a.level = j; a.a_src = j > 1 ? plane(j - 2) : nullptr; a.a_dst = nullptr;
            a.r_src = j < levels ? plane(kHaarNaivePlanes - 2 + (j & 1)) : nullptr;
            a.r_dst = plane(kHaarNaivePlanes - 2 + ((j - 1) & 1));
            HIP_TRY(launch_haar_ti_up(a, N, s));
        }
    }
    if (alias) {
        HIP_TRY(hipMemcpyAsync(out, e->d_work, px * sizeof(float), hipMemcpyDeviceToDevice, s));
        ++launches;
    }
    p.end(launches);
    return PNP_OK;
}

int run_prox_dual(pnp_engine* e, const float* mu, const float* tact, const float* x, float2* z, float2* u,
                  hipStream_t s) {
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w;
    if (NormalOp normal = stage_normal(e)) return run_prox_dual_cg(e, normal, e->stage.cg, mu, tact, x, z, u, s);   // a CG stage
    if (H == 128 && W == 128 && N >= e->tune.slice128_min_n) {   // chip-filling batches of the reference's slice size: 37 B/px
        Prof p(e, s, PROF_FFT_COLS, -1);
        HIP_TRY(launch_admm_slice128(x, z, u, e->plan.tw_w, e->d_y0s, e->d_masks, e->mask_n, mu, tact, N, s));
        return PNP_OK;
    }
    {                                                     // three launches; each picks the kernel family for the handle's sides
        Prof p(e, s, PROF_FFT_ROWS, -1);
        HIP_TRY(launch_fft_rows_fwd_admm(x, u, e->d_work, e->plan.tw_w, tact, N, H, W, s));
    }
    {
        Prof p(e, s, PROF_FFT_COLS, -1);
        HIP_TRY(launch_fft_cols_prox(e->d_work, e->plan.tw_h, e->d_y0s, e->d_masks, e->mask_n, mu, tact, N, H, W, s));
    }
    {
        Prof p(e, s, PROF_FFT_ROWS, -1);
        HIP_TRY(launch_fft_rows_inv_admm(e->d_work, x, z, u, e->plan.tw_w, tact, N, H, W, s));
    }
    return PNP_OK;
}

// pnp_residuals' PNP_RES_DC: the partial sums of the live stage's data misfit of x into dcpart
int stage_misfit(pnp_engine* e, const float* x, double* dcpart, hipStream_t s) {
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w, C = e->stage.coils;
    switch (e->stage.kind) {
    case STAGE_NC: case STAGE_NS: case STAGE_OR: case STAGE_ORS:
        return op_misfit(e, live_op(e), x, e->st_y, stage_w(e), e->st_mpart, dcpart, s);
    case STAGE_MC: {
        // the plain transforms of S_c x into the coil scratch, then sum_c ||M (FFT(S_c x) - ys_c)||^2
        {
            Prof p(e, s, PROF_OTHER, -1);
            HIP_TRY(launch_sense_expand(nullptr, x, e->mc_sens, e->stage.sens_n, C, nullptr, e->mc_work, N, H, W, s));
        }
        if (int rc = plain_fft2(e, e->mc_work, e->mc_work, N * C, 0, s)) return rc;
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_sense_misfit(e->mc_work, e->mc_y, e->d_masks, e->mask_n, C, dcpart, N, H, W, s));
        return PNP_OK;
    }
    case STAGE_CART: {
        // the plain transform of x into the data-fidelity stage's scratch; the shifts of fft_c live in the stored constants (reset_kernel)
        if (int rc = plain_fft2(e, nullptr, e->d_work, N, 0, s, x)) return rc;
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_misfit_tiles(e->d_work, e->d_y0s, e->d_masks, e->mask_n, dcpart, N, H, W, s));
        return PNP_OK;
    }
    case STAGE_NONE: break;                                // pnp_residuals has refused it
    }
    return PNP_OK;
}

// the refusal of an entry point that serves one CG stage while another stage is live: each stage's own sentence
int need_stage(const char* fn, const pnp_engine* e, StageKind kind) {
    if (e->stage.kind == kind) return PNP_OK;
    switch (kind) {
    case STAGE_MC: return fail(PNP_ERR_STATE, "%s: the handle is in single-coil mode (pnp_set_kspace_mc / pnp_reset_mc)", fn);
    case STAGE_NC: return fail(PNP_ERR_STATE, "%s: the handle is not in non-Cartesian mode (pnp_set_kspace_nc / pnp_reset_nc)", fn);
    case STAGE_OR: return fail(PNP_ERR_STATE, "%s: the handle is not in off-resonance mode (pnp_set_kspace_offres / pnp_reset_offres)", fn);
    case STAGE_ORS:
        return fail(PNP_ERR_STATE, "%s: the handle is not in multi-coil off-resonance mode (pnp_set_kspace_offres_mc / pnp_reset_offres_mc)", fn);
    default: return fail(PNP_ERR_STATE, "%s: the handle is not in non-Cartesian SENSE mode (pnp_set_kspace_ncsense / pnp_reset_ncsense)", fn);
    }
}
// pnp_{mc,nc,ncsense}_cg_residual
int stage_cg_residual(const char* fn, pnp_engine* e, StageKind kind, float* out, hipStream_t s) {
    if (!e || !out) return fail(PNP_ERR_INVALID, "%s: null argument", fn);
    if (int rc = need_stage(fn, e, kind)) return rc;
    PNP_ON_DEVICE(e);
    Prof p(e, s, PROF_OTHER, -1);
    HIP_TRY(launch_sense_cgres(e->mc_sc, out, e->cfg.n, s));
    return PNP_OK;
}
// pnp_{mc,nc,ncsense}_normal
int stage_normal_op(const char* fn, pnp_engine* e, StageKind kind, const float* pv, const float* mu, float* q, hipStream_t s) {
    if (!e || !pv || !mu || !q) return fail(PNP_ERR_INVALID, "%s: null argument", fn);
    if (pv == q) return fail(PNP_ERR_INVALID, "%s: p and q must not alias", fn);
    if (int rc = need_stage(fn, e, kind)) return rc;
    PNP_ON_DEVICE(e);
    return stage_normal(e)(e, (const float2*)pv, mu, nullptr, (float2*)q, s);
}

}  // namespace

extern "C" {

const char* pnp_last_error(void) { return g_err.c_str(); }
const char* pnp_version(void) { return "pnpadmm 0.4 (gfx950, f32 MFMA; optional bf16-operand convs with two-term weights)"; }

// Allocates what the handle's plan (e->dplan, e->tune: set by pnp_create) asks for, and the k-space side
static int create_impl(const pnp_config* cfg, pnp_engine* e) {
    const size_t N = cfg->n, H = cfg->h, W = cfg->w;
    const DenoiserPlan& P = e->dplan;
    for (int k = 0; k < N_LEVELS; ++k)
        for (int slot = 0; slot < N_SLOTS; ++slot) {
            const size_t bytes = P.plane_bytes[k][slot];
            if (bytes == 0) continue;
            hipError_t er = hipMalloc((void**)&e->plane[k][slot], bytes);
            if (er != hipSuccess) return fail(PNP_ERR_NOMEM, "activation planes: %s", hipGetErrorString(er));
            e->ws_bytes += bytes;
        }
    if (P.partial_floats > 0) {
        if (hipMalloc((void**)&e->d_partial, P.partial_floats * sizeof(float)) != hipSuccess) return fail(PNP_ERR_NOMEM, "split-K workspace");
        e->ws_bytes += P.partial_floats * sizeof(float);
    }
    resolve_launches(e);
    const size_t cbytes = N * H * W * sizeof(float2);
    if (hipMalloc((void**)&e->d_work, cbytes) != hipSuccess || hipMalloc((void**)&e->d_y0s, cbytes) != hipSuccess ||
        hipMalloc((void**)&e->d_masks, N * H * W) != hipSuccess)
        return fail(PNP_ERR_NOMEM, "k-space scratch");
    e->ws_bytes += 2 * cbytes + N * H * W;
    const size_t sbytes = N * (size_t)ssim_tiles(cfg->h, cfg->w) * sizeof(double);
    if (hipMalloc((void**)&e->d_ssim_part, sbytes) != hipSuccess) return fail(PNP_ERR_NOMEM, "SSIM partial sums");
    e->ws_bytes += sbytes;
    // pnp_residuals: its own partial sums (the SSIM buffer holds one double per 32 x 32 tile - fewer than five per 2048 pixels on small slices)
    const size_t rbytes = N * (size_t)pixel_chunks(cfg->h, cfg->w) * 5 * sizeof(double);
    if (hipMalloc((void**)&e->d_res_part, rbytes) != hipSuccess) return fail(PNP_ERR_NOMEM, "residual partial sums");
    e->ws_bytes += rbytes;
    e->plan.h = cfg->h; e->plan.w = cfg->w;
    int rc;
    if ((rc = make_twiddles(cfg->h, &e->plan.tw_h)) || (rc = make_twiddles(cfg->w, &e->plan.tw_w))) return rc;
    return PNP_OK;
}

int pnp_create(const pnp_config* cfg, pnp_handle* out) {
    PNP_API_BEGIN
    if (!cfg || !out) return fail(PNP_ERR_INVALID, "pnp_create: null argument");
    *out = nullptr;
    if (cfg->n < 1 || cfg->h < 16 || cfg->w < 16 || cfg->h % 16 || cfg->w % 16)
        return fail(PNP_ERR_INVALID, "pnp_create: need n >= 1 and h, w multiples of 16 (got n=%d h=%d w=%d)", cfg->n,
                    cfg->h, cfg->w);
    if (cfg->h > 1024 || cfg->w > 1024) return fail(PNP_ERR_INVALID, "pnp_create: h, w <= 1024");
    // the conv kernels' x2 upsample reads two compile-time source lines per output row (commit_lo / interpolate): holds in float32
    // for every even height up to 1024 - checked, not assumed
    for (int k = 0; k < 4; ++k)
        if (!(cfg->flags & PNP_FLAG_NO_DENOISER) && !upsample_lines_regular(cfg->h >> k))
            return fail(PNP_ERR_INVALID, "pnp_create: upsample to %d rows is not line-regular in float32", cfg->h >> k);
    // the whole denoiser plan before any device call or allocation: a handle it refuses costs nothing
    const Tuning tune = tuning_from_env();
    DenoiserPlan plan;
    std::string why;
    if (!plan_denoiser(*cfg, tune, &plan, &why)) return fail(PNP_ERR_INVALID, "%s", why.c_str());
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(PNP_ERR_INVALID, "pnp_create: device %d of %d", cfg->device, ndev);
    pnp_engine* e = new (std::nothrow) pnp_engine();
    if (!e) return fail(PNP_ERR_NOMEM, "pnp_create: out of host memory");
    e->cfg = *cfg;
    e->tune = tune;
    if (tune.ncsense_block >= 1 && tune.ncsense_block <= PNP_MC_MAX_COILS) e->ns_block = tune.ncsense_block;   // a check and a timing knob
    if (tune.ncsense_naive >= 0) e->ns_naive = tune.ncsense_naive ? NS_ALL : 0;
    if (tune.offres_block >= 1 && tune.offres_block <= PNP_MC_MAX_COILS) e->or_block = tune.offres_block;     // a check and a timing knob
    if (tune.offres_naive >= 0) e->or_naive = tune.offres_naive ? OR_ALL : 0;
    if (tune.offres_ls_naive >= 0) e->orls_naive = tune.offres_ls_naive ? OR_ALL : 0;
    if (tune.offres_mc_block >= 1 && tune.offres_mc_block <= PNP_MC_MAX_COILS) e->om_block = tune.offres_mc_block;   // a check and a timing knob
    if (tune.offres_mc_naive >= 0) e->om_naive = tune.offres_mc_naive ? ORM_ALL : 0;
    e->tz_fused = !tune.toeplitz_naive && kspace_len_ok(2 * cfg->h) && kspace_len_ok(2 * cfg->w) && toeplitz_fused_ok(cfg->h, cfg->w);
    e->otz_fused = !tune.offres_tz_naive && kspace_len_ok(2 * cfg->h) && kspace_len_ok(2 * cfg->w) && toeplitz_fused_ok(cfg->h, cfg->w);
    if (tune.offres_tz_slices >= 1) e->otz_slices = tune.offres_tz_slices;   // a check, not a mode
    e->dplan = plan;
    int rc;
    {
        DeviceGuard g(cfg->device);
        if (g.err != hipSuccess) { delete e; return fail(PNP_ERR_HIP, "hipSetDevice(%d): %s", cfg->device, hipGetErrorString(g.err)); }
        try { rc = create_impl(cfg, e); }
        catch (...) { const std::string keep = g_err; pnp_destroy(e); g_err = keep; throw; }
        if (rc != PNP_OK) { const std::string keep = g_err; pnp_destroy(e); g_err = keep; return rc; }
    }
    *out = e;
    return PNP_OK;
    PNP_API_END("pnp_create")
}

int pnp_destroy(pnp_handle e) {
    PNP_API_BEGIN
    if (!e) return PNP_OK;
    DeviceGuard g(e->cfg.device);
    (void)hipDeviceSynchronize();
    for (int i = 0; i < N_LAYERS; ++i) { (void)hipFree(e->d_wpack[i]); (void)hipFree(e->d_bias[i]); }
    for (auto& level : e->plane) for (float* b : level) (void)hipFree(b);
    (void)hipFree(e->d_work); (void)hipFree(e->d_y0s); (void)hipFree(e->d_masks); (void)hipFree(e->d_ssim_part); (void)hipFree(e->d_res_part); (void)hipFree(e->d_partial);
    (void)hipFree(e->mc_y); (void)hipFree(e->mc_work); (void)hipFree(e->mc_sens); (void)hipFree(e->mc_vec); (void)hipFree(e->mc_part); (void)hipFree(e->mc_sc);
    (void)hipFree(e->cm_max); (void)hipFree(e->cm_rss);
    (void)hipFree(e->cc_part); (void)hipFree(e->cc_gram);
    (void)hipFree(e->pw_part);
    (void)hipFree(e->es_ws);
    (void)hipFree(e->gr_ws);
    (void)hipFree(e->tv_p);
    (void)hipFree(e->haar_ws);
    (void)hipFree(e->fm_ws); (void)hipFree(e->fm_part);
    (void)hipFree(e->nc.i0); (void)hipFree(e->nc.wts); (void)hipFree(e->nc.cy); (void)hipFree(e->nc.cx); (void)hipFree(e->nc.bin_off); (void)hipFree(e->nc.bin_idx);
    (void)hipFree(e->nc.tw_gh); (void)hipFree(e->nc.tw_gw);
    (void)hipFree(e->ns_img);
    (void)hipFree(e->tz_traj); (void)hipFree(e->tz_k); (void)hipFree(e->tz_w); (void)hipFree(e->tz_tw_h); (void)hipFree(e->tz_tw_w); (void)hipFree(e->tz_grid);
    (void)hipFree(e->orp.tau); (void)hipFree(e->orp.seg); (void)hipFree(e->orp.b0); (void)hipFree(e->orp.b1); (void)hipFree(e->orp.list_off);
    (void)hipFree(e->orp.coef);
    (void)hipFree(e->orp.list_idx);
    (void)hipFree(e->om_samp); (void)hipFree(e->om_part); (void)hipFree(e->om_img); (void)hipFree(e->om_line);
    (void)hipFree(e->otz.blk_off); (void)hipFree(e->otz.blk_idx); (void)hipFree(e->otz_traj); (void)hipFree(e->otz_k); (void)hipFree(e->otz_w);
    (void)hipFree(e->otz_tw_h); (void)hipFree(e->otz_tw_w); (void)hipFree(e->otz_img); (void)hipFree(e->otz_x); (void)hipFree(e->otz_y); (void)hipFree(e->otz_cimg);
    (void)hipFree(e->dcf_grid); (void)hipFree(e->dcf_w); (void)hipFree(e->dcf_part); (void)hipFree(e->dcf_max);
    (void)hipFree(e->ns_grid); (void)hipFree(e->ns_samp);
    (void)hipFree(e->nc_grid); (void)hipFree(e->nc_samp);
    (void)hipFree(e->st_y); (void)hipFree(e->st_w); (void)hipFree(e->st_sens); (void)hipFree(e->st_maps); (void)hipFree(e->st_mpart); (void)hipFree(e->acq_maps);
    (void)hipFree(e->plan.tw_h); (void)hipFree(e->plan.tw_w);
    for (auto& p : e->events) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    delete e;
    return PNP_OK;
    PNP_API_END("pnp_destroy")
}

size_t pnp_workspace_bytes(pnp_handle e) { return e ? e->ws_bytes : 0; }
int pnp_bf16_weight_terms(pnp_handle e) { return e ? e->dplan.bf16_terms : 0; }

// All-or-nothing: every layer is packed on the host and uploaded into NEW device buffers first; the handle's buffers are
// replaced only when all 56 uploads succeeded, so a failure leaves the handle exactly as it was (an earlier successful
// load stays usable, a never-loaded handle stays "weights not loaded").
int pnp_load_unet_weights(pnp_handle e, const float* blob, size_t n_floats) {
    PNP_API_BEGIN
    if (!e || !blob) return fail(PNP_ERR_INVALID, "pnp_load_unet_weights: null argument");
    if (n_floats != kNParams)
        return fail(PNP_ERR_INVALID, "pnp_load_unet_weights: expected %zu floats (56 tensors of UNet(2,1)), got %zu",
                    kNParams, n_floats);
    if (e->cfg.flags & PNP_FLAG_NO_DENOISER) return fail(PNP_ERR_STATE, "pnp_load_unet_weights: handle created with PNP_FLAG_NO_DENOISER");
    PNP_ON_DEVICE(e);
    float* nw_pack[N_LAYERS] = {};
    float* nw_bias[N_LAYERS] = {};
    auto drop_new = [&]() { for (int i = 0; i < N_LAYERS; ++i) { (void)hipFree(nw_pack[i]); (void)hipFree(nw_bias[i]); } };
    const bool bf16 = (e->cfg.flags & PNP_FLAG_BF16_CONVS) != 0;
    size_t off = 0;
    std::vector<float> tmp;
    hipError_t er = hipSuccess;
    try {
        for (int li = 0; li < N_LAYERS && er == hipSuccess; ++li) {
            const LayerSpec& L = kLayers[li];
            const size_t nw = (size_t)L.cout * L.cin * L.ksize * L.ksize;
            const float* w = blob + off;
            const float* b = blob + off + nw;
            off += nw + L.cout;
            size_t pf;
            const float* src;
            const int at = e->dplan.launch_of[li];           // (-1: a layer fused into its neighbour; only the two raw ones can be)
            switch (e->dplan.family[li]) {
            case FAM_FIRST: case FAM_LAST:                   // first (2->32, OIHW as is) and last (1x1) layers
                pf = nw; src = w;
                break;
            case FAM_WINO4:
                pf = winograd4_pack_floats(L.cin, L.cout);
                tmp.assign(pf, 0.f);
                pack_winograd4_weights(w, L.cin, L.cout, e->dplan.launch[at].wino.ck, tmp.data());
                src = tmp.data();
                break;
            case FAM_WINO2:
                pf = winograd_pack_floats(L.cin, L.cout);
                tmp.assign(pf, 0.f);
                pack_winograd_weights(w, L.cin, L.cout, e->dplan.launch[at].wino.ck, tmp.data());
                src = tmp.data();
                break;
            default:                                         // FAM_DIRECT, FAM_WS
                pf = bf16 ? conv3x3_pack_floats_bf16(L.cin, L.cout, e->dplan.bf16_terms) : conv3x3_pack_floats(L.cin, L.cout);
                tmp.assign(pf, 0.f);
                if (bf16) pack_conv3x3_weights_bf16(w, L.cin, L.cout, e->dplan.launch[at].conv.ck, e->dplan.bf16_terms, tmp.data());
                else pack_conv3x3_weights(w, L.cin, L.cout, e->dplan.launch[at].conv.ck, tmp.data());
                src = tmp.data();
            }
            if ((er = hipMalloc((void**)&nw_pack[li], pf * sizeof(float))) != hipSuccess) break;
            if ((er = hipMemcpy(nw_pack[li], src, pf * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) break;
            if ((er = hipMalloc((void**)&nw_bias[li], L.cout * sizeof(float))) != hipSuccess) break;
            er = hipMemcpy(nw_bias[li], b, L.cout * sizeof(float), hipMemcpyHostToDevice);
        }
    } catch (...) { drop_new(); throw; }
    if (er != hipSuccess) { drop_new(); return fail(PNP_ERR_HIP, "pnp_load_unet_weights: upload failed: %s (handle unchanged)", hipGetErrorString(er)); }
    (void)hipDeviceSynchronize();                        // no launch still reads the buffers being replaced
    for (int li = 0; li < N_LAYERS; ++li) {
        (void)hipFree(e->d_wpack[li]); (void)hipFree(e->d_bias[li]);
        e->d_wpack[li] = nw_pack[li]; e->d_bias[li] = nw_bias[li];
    }
    e->weights_loaded = true;
    return PNP_OK;
    PNP_API_END("pnp_load_unet_weights")
}

int pnp_reset(pnp_handle e, const float* x0, const float* y0, const uint8_t* mask, int mask_n, float* x, float* z,
              float* u, void* stream) {
    PNP_API_BEGIN
    return cart_install("pnp_reset", e, true, (const float2*)x0, (const float2*)y0, mask, mask_n, x, (float2*)z, (float2*)u, (hipStream_t)stream);
    PNP_API_END("pnp_reset")
}

int pnp_set_kspace(pnp_handle e, const float* y0, const uint8_t* mask, int mask_n, void* stream) {
    PNP_API_BEGIN
    return cart_install("pnp_set_kspace", e, false, nullptr, (const float2*)y0, mask, mask_n, nullptr, nullptr, nullptr, (hipStream_t)stream);
    PNP_API_END("pnp_set_kspace")
}

int pnp_step(pnp_handle e, const float* mu, const float* sigma_d, const float* t_action, float* x, float* z, float* u,
             float* t_state, uint8_t* done, void* stream) {
    PNP_API_BEGIN
    if (!e || !mu || !sigma_d || !x || !z || !u) return fail(PNP_ERR_INVALID, "pnp_step: null argument");
    const bool tv = e->prior == PNP_PRIOR_TV, haar = e->prior == PNP_PRIOR_HAAR;
    if (!tv && !haar && !e->weights_loaded) return fail(PNP_ERR_STATE, "pnp_step: denoiser weights not loaded (pnp_load_unet_weights)");
    if (e->stage.kind == STAGE_NONE) return fail(PNP_ERR_STATE, "pnp_step: pnp_reset has not been called");
    PNP_ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (tv) {
        if ((rc = run_tv(e, nullptr, (const float2*)z, (const float2*)u, sigma_d, (float)e->tv_scale, t_action, e->tv_iters, x, s))) return rc;
    } else if (haar) {
        if ((rc = run_haar(e, nullptr, (const float2*)z, (const float2*)u, sigma_d, (float)e->haar_scale, t_action, e->haar_levels, e->haar_mode, x, s)))
            return rc;
    } else if ((rc = run_unet(e, nullptr, (const float2*)z, (const float2*)u, sigma_d, t_action, x, s))) return rc;
    if ((rc = run_prox_dual(e, mu, t_action, x, (float2*)z, (float2*)u, s))) return rc;
    if (t_state || done) {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_finish(t_action, t_state, done, e->cfg.n, s));
    }
    return PNP_OK;
    PNP_API_END("pnp_step")
}

int pnp_denoise(pnp_handle e, const float* x_in, const float* sigma, float* out, void* stream) {
    PNP_API_BEGIN
    if (!e || !x_in || !sigma || !out) return fail(PNP_ERR_INVALID, "pnp_denoise: null argument");
    if (!e->weights_loaded) return fail(PNP_ERR_STATE, "pnp_denoise: denoiser weights not loaded");
    PNP_ON_DEVICE(e);
    return run_unet(e, x_in, nullptr, nullptr, sigma, nullptr, out, (hipStream_t)stream);
    PNP_API_END("pnp_denoise")
}

int pnp_tv_denoise(pnp_handle e, const float* x_in, const float* lam, int iters, float* out, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_tv_denoise";
    if (iters < 1 || iters > PNP_TV_MAX_ITERS) return fail(PNP_ERR_INVALID, "%s: iters must be 1..%d (got %d)", fn, PNP_TV_MAX_ITERS, iters);
    if (!x_in) return fail(PNP_ERR_INVALID, "%s: null x_in", fn);
    if (!lam) return fail(PNP_ERR_INVALID, "%s: null lam", fn);
    if (!out) return fail(PNP_ERR_INVALID, "%s: null out", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    PNP_ON_DEVICE(e);
    return run_tv(e, x_in, nullptr, nullptr, lam, 1.0f, nullptr, iters, out, (hipStream_t)stream);
    PNP_API_END("pnp_tv_denoise")
}

int pnp_set_prior(pnp_handle e, int prior, double tv_scale, int tv_iters) {
    PNP_API_BEGIN
    const char* fn = "pnp_set_prior";
    if (prior != PNP_PRIOR_UNET && prior != PNP_PRIOR_TV)
        return fail(PNP_ERR_INVALID, "%s: prior must be PNP_PRIOR_UNET or PNP_PRIOR_TV (got %d)", fn, prior);
    if (prior == PNP_PRIOR_TV) {
        if (!(tv_scale >= 0.0) || !std::isfinite(tv_scale)) return fail(PNP_ERR_INVALID, "%s: tv_scale must be finite and >= 0 (got %g)", fn, tv_scale);
        if (tv_iters < 1 || tv_iters > PNP_TV_MAX_ITERS)
            return fail(PNP_ERR_INVALID, "%s: tv_iters must be 1..%d (got %d)", fn, PNP_TV_MAX_ITERS, tv_iters);
    }
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (prior == PNP_PRIOR_UNET) {
        if (e->cfg.flags & PNP_FLAG_NO_DENOISER)
            return fail(PNP_ERR_STATE, "%s: PNP_PRIOR_UNET on a handle created with PNP_FLAG_NO_DENOISER", fn);
        e->prior = PNP_PRIOR_UNET;                             // (the TV parameters stay as they were: they are not read under this prior)
        return PNP_OK;
    }
    e->prior = PNP_PRIOR_TV;
    e->tv_scale = tv_scale;
    e->tv_iters = tv_iters;
    return PNP_OK;
    PNP_API_END("pnp_set_prior")
}

int pnp_get_prior(pnp_handle e, int* prior, double* tv_scale, int* tv_iters) {
    PNP_API_BEGIN
    const char* fn = "pnp_get_prior";
    if (!prior || !tv_scale || !tv_iters) return fail(PNP_ERR_INVALID, "%s: null pointer", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    *prior = e->prior;
    *tv_scale = e->tv_scale;
    *tv_iters = e->tv_iters;
    return PNP_OK;
    PNP_API_END("pnp_get_prior")
}

int pnp_haar_denoise(pnp_handle e, const float* x_in, const float* lam, int levels, int mode, float* out, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_haar_denoise";
    if (levels < 1 || levels > PNP_HAAR_MAX_LEVELS)
        return fail(PNP_ERR_INVALID, "%s: levels must be 1..%d (got %d)", fn, PNP_HAAR_MAX_LEVELS, levels);
    if (mode != PNP_HAAR_TI && mode != PNP_HAAR_ORTHO) return fail(PNP_ERR_INVALID, "%s: mode must be PNP_HAAR_TI or PNP_HAAR_ORTHO (got %d)", fn, mode);
    if (!x_in) return fail(PNP_ERR_INVALID, "%s: null x_in", fn);
    if (!lam) return fail(PNP_ERR_INVALID, "%s: null lam", fn);
    if (!out) return fail(PNP_ERR_INVALID, "%s: null out", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    PNP_ON_DEVICE(e);
    return run_haar(e, x_in, nullptr, nullptr, lam, 1.0f, nullptr, levels, mode, out, (hipStream_t)stream);
    PNP_API_END("pnp_haar_denoise")
}

int pnp_set_prior_haar(pnp_handle e, double haar_scale, int levels, int mode) {
    PNP_API_BEGIN
    const char* fn = "pnp_set_prior_haar";
    if (!(haar_scale >= 0.0) || !std::isfinite(haar_scale))
        return fail(PNP_ERR_INVALID, "%s: haar_scale must be finite and >= 0 (got %g)", fn, haar_scale);
    if (levels < 1 || levels > PNP_HAAR_MAX_LEVELS)
        return fail(PNP_ERR_INVALID, "%s: levels must be 1..%d (got %d)", fn, PNP_HAAR_MAX_LEVELS, levels);
    if (mode != PNP_HAAR_TI && mode != PNP_HAAR_ORTHO) return fail(PNP_ERR_INVALID, "%s: mode must be PNP_HAAR_TI or PNP_HAAR_ORTHO (got %d)", fn, mode);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    e->prior = PNP_PRIOR_HAAR;
    e->haar_scale = haar_scale;
    e->haar_levels = levels;
    e->haar_mode = mode;
    return PNP_OK;
    PNP_API_END("pnp_set_prior_haar")
}

int pnp_get_prior_haar(pnp_handle e, double* haar_scale, int* levels, int* mode) {
    PNP_API_BEGIN
    const char* fn = "pnp_get_prior_haar";
    if (!haar_scale || !levels || !mode) return fail(PNP_ERR_INVALID, "%s: null pointer", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    *haar_scale = e->haar_scale;
    *levels = e->haar_levels;
    *mode = e->haar_mode;
    return PNP_OK;
    PNP_API_END("pnp_get_prior_haar")
}

int pnp_fft2c(pnp_handle e, const float* in, float* out, int batch, int hh, int ww, int inverse, void* stream) {
    PNP_API_BEGIN
    if (!e || !in || !out) return fail(PNP_ERR_INVALID, "pnp_fft2c: null argument");
    if (hh != e->cfg.h || ww != e->cfg.w || batch < 1 || batch > e->cfg.n)
        return fail(PNP_ERR_INVALID, "pnp_fft2c: shape [%d,%d,%d] does not fit the engine [%d,%d,%d]", batch, hh, ww,
                    e->cfg.n, e->cfg.h, e->cfg.w);
    if (int rc = check_kspace_sizes("pnp_fft2c", e, "h, w must be in")) return rc;   // (hh, ww are the handle's)
    PNP_ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    // fft_c = S . FFT . S : fold both shifts into the load/store indices of the two passes (add-mod by L/2); rows then columns in BOTH
    // directions, unlike the plain transform
    {
        Prof p(e, s, PROF_FFT_ROWS, -1);
        HIP_TRY(launch_fft_rows((const float2*)in, (float2*)out, e->plan.tw_w, batch, hh, ww, inverse, ww / 2, s));
    }
    {
        Prof p(e, s, PROF_FFT_COLS, -1);
        HIP_TRY(launch_fft_cols((float2*)out, e->plan.tw_h, batch, hh, ww, inverse, hh / 2, s));
    }
    return PNP_OK;
    PNP_API_END("pnp_fft2c")
}

int pnp_prox_dual(pnp_handle e, const float* mu, const float* t_action, const float* x, float* z, float* u,
                  void* stream) {
    PNP_API_BEGIN
    if (!e || !mu || !x || !z || !u) return fail(PNP_ERR_INVALID, "pnp_prox_dual: null argument");
    if (e->stage.kind == STAGE_NONE) return fail(PNP_ERR_STATE, "pnp_prox_dual: pnp_reset has not been called");
    PNP_ON_DEVICE(e);
    return run_prox_dual(e, mu, t_action, x, (float2*)z, (float2*)u, (hipStream_t)stream);
    PNP_API_END("pnp_prox_dual")
}

int pnp_psnr(pnp_handle e, const float* x, const float* gt, float* out, void* stream) {
    PNP_API_BEGIN
    if (!e || !x || !gt || !out) return fail(PNP_ERR_INVALID, "pnp_psnr: null argument");
    PNP_ON_DEVICE(e);
    Prof p(e, (hipStream_t)stream, PROF_OTHER, -1);
    HIP_TRY(launch_psnr(x, gt, out, e->cfg.n, e->cfg.h * e->cfg.w, (hipStream_t)stream));
    return PNP_OK;
    PNP_API_END("pnp_psnr")
}

int pnp_ssim(pnp_handle e, const float* x, const float* gt, float data_range, float k1, float k2, int radius, int flags, float* out,
             float* map, void* stream) {
    PNP_API_BEGIN
    // scalar arguments first, so that every rejection happens before any HIP call
    if (radius < 1 || radius > kSsimMaxRadius) return fail(PNP_ERR_INVALID, "pnp_ssim: radius must be 1..%d (got %d)", kSsimMaxRadius, radius);
    if (!(data_range > 0.f) || !std::isfinite(data_range)) return fail(PNP_ERR_INVALID, "pnp_ssim: data_range must be > 0 (got %g)", (double)data_range);
    if (!std::isfinite(k1) || !std::isfinite(k2)) return fail(PNP_ERR_INVALID, "pnp_ssim: k1, k2 must be finite");
    if (flags & ~PNP_SSIM_CLAMP_X) return fail(PNP_ERR_INVALID, "pnp_ssim: unknown flag bits 0x%x", (unsigned)(flags & ~PNP_SSIM_CLAMP_X));
    if (!e || !x || !gt || !out) return fail(PNP_ERR_INVALID, "pnp_ssim: null argument");
    PNP_ON_DEVICE(e);
    SsimArgs a{};
    a.x = x; a.gt = gt; a.map = map; a.partial = e->d_ssim_part; a.out = out;
    a.H = e->cfg.h; a.W = e->cfg.w; a.radius = radius; a.clamp_x = (flags & PNP_SSIM_CLAMP_X) ? 1 : 0;
    const double c1 = (double)k1 * data_range, c2 = (double)k2 * data_range;
    a.c1 = (float)(c1 * c1); a.c2 = (float)(c2 * c2);
    // scipy.ndimage._gaussian_kernel1d(sigma = 1.5, order 0, radius): exp(-x^2 / (2 sigma^2)) normalised to sum 1, in double
    double tap[2 * kSsimMaxRadius + 1], sum = 0.0;
    for (int i = -radius; i <= radius; ++i) sum += (tap[i + radius] = std::exp(-0.5 / (1.5 * 1.5) * (double)i * (double)i));
    for (int i = 0; i <= 2 * radius; ++i) a.w[i] = (float)(tap[i] / sum);
    Prof p(e, (hipStream_t)stream, PROF_OTHER, -1);
    HIP_TRY(launch_ssim(a, e->cfg.n, (hipStream_t)stream));
    return PNP_OK;
    PNP_API_END("pnp_ssim")
}

int pnp_residuals(pnp_handle e, const float* x, const float* z, const float* u, const void* prev, int flags, float* out, void* stream) {
    PNP_API_BEGIN
    // every rejection happens before any HIP call, and leaves `out` untouched
    if (flags & ~(PNP_RES_DELTA | PNP_RES_DC))
        return fail(PNP_ERR_INVALID, "pnp_residuals: unknown flag bits 0x%x", (unsigned)(flags & ~(PNP_RES_DELTA | PNP_RES_DC)));
    if (!x) return fail(PNP_ERR_INVALID, "pnp_residuals: null x");
    if (!z) return fail(PNP_ERR_INVALID, "pnp_residuals: null z");
    if (!u) return fail(PNP_ERR_INVALID, "pnp_residuals: null u");
    if (!out) return fail(PNP_ERR_INVALID, "pnp_residuals: null out");
    if ((flags & PNP_RES_DELTA) && !prev) return fail(PNP_ERR_INVALID, "pnp_residuals: PNP_RES_DELTA needs prev (a pnp_snapshot buffer), got null");
    if (!e) return fail(PNP_ERR_INVALID, "pnp_residuals: null handle");
    // the tile kernels read with 16-byte loads
    const struct { const void* p; const char* name; } al[] = {{x, "x"}, {z, "z"}, {u, "u"}, {prev, "prev"}};
    for (const auto& a : al)
        if ((reinterpret_cast<uintptr_t>(a.p) & 15u) != 0) return fail(PNP_ERR_INVALID, "pnp_residuals: %s must be 16-byte aligned", a.name);
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w;
    if (flags & PNP_RES_DC) {
        if (int rc = check_kspace_sizes("pnp_residuals", e, "PNP_RES_DC takes h, w in")) return rc;
        if (e->stage.kind == STAGE_NONE) return fail(PNP_ERR_STATE, "pnp_residuals: PNP_RES_DC needs the episode's k-space constants (pnp_reset / pnp_set_kspace)");
    }
    PNP_ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    const SnapLayout snap(e);
    double* const part = e->d_res_part;
    double* const dcpart = part + (size_t)N * pixel_chunks(H, W) * 4;
    {
        const char* pv = static_cast<const char*>((flags & PNP_RES_DELTA) ? prev : nullptr);   // [x | z | u | t] as pnp_snapshot packs them
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_residual_tiles(x, (const float2*)z, (const float2*)u, (const float*)pv, pv ? (const float2*)(pv + snap.z_off()) : nullptr,
                                      pv ? (const float2*)(pv + snap.u_off()) : nullptr, part, N, H, W, s));
    }
    if (flags & PNP_RES_DC)
        if (int rc = stage_misfit(e, x, dcpart, s)) return rc;
    Prof p(e, s, PROF_OTHER, -1);
    HIP_TRY(launch_residual_reduce(part, dcpart, (flags & PNP_RES_DELTA) ? 1 : 0, (flags & PNP_RES_DC) ? 1 : 0, out, N, H, W, s));
    return PNP_OK;
    PNP_API_END("pnp_residuals")
}

int pnp_acquire(pnp_handle e, const float* gt, const uint8_t* mask, int mask_n, double sigma_n, uint64_t seed, int flags, float* y0,
                float* aty0, float* x0, void* stream) {
    PNP_API_BEGIN
    // every rejection happens before any HIP call, and leaves the outputs untouched
    if (flags != 0) return fail(PNP_ERR_INVALID, "pnp_acquire: flags must be 0 (got 0x%x)", (unsigned)flags);
    if (!(sigma_n >= 0.0) || !std::isfinite(sigma_n)) return fail(PNP_ERR_INVALID, "pnp_acquire: sigma_n must be finite and >= 0 (got %g)", sigma_n);
    if (!gt) return fail(PNP_ERR_INVALID, "pnp_acquire: null gt");
    if (!mask) return fail(PNP_ERR_INVALID, "pnp_acquire: null mask");
    if (!y0) return fail(PNP_ERR_INVALID, "pnp_acquire: null y0");
    if (!e) return fail(PNP_ERR_INVALID, "pnp_acquire: null handle");
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w;
    if (mask_n != 1 && mask_n != N) return fail(PNP_ERR_INVALID, "pnp_acquire: mask_n must be 1 or n=%d", N);
    if (int rc = check_kspace_sizes("pnp_acquire", e)) return rc;
    PNP_ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    // the plain transform of gt into the data-fidelity stage's scratch, by the passes pnp_residuals' misfit uses; the shifts of fft_c live in
    // the epilogue's indices and sign
    if ((rc = plain_fft2(e, nullptr, e->d_work, N, 0, s, gt))) return rc;
    {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_acquire_epilogue(e->d_work, mask, mask_n, (float2*)y0, sigma_n, seed, N, H, W, s));
    }
    if (!aty0 && !x0) return PNP_OK;
    float2* const a = aty0 ? (float2*)aty0 : e->d_work;     // without aty0 the row pass runs in place: a workgroup reads and writes its own rows only
    if ((rc = plain_fft2(e, e->d_work, a, N, 1, s))) return rc;
    if (x0) {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_acquire_clamp(a, (float2*)x0, N, H, W, s));
    }
    return PNP_OK;
    PNP_API_END("pnp_acquire")
}

int pnp_set_kspace_mc(pnp_handle e, const float* y0, const float* sens, int coils, int sens_n, const uint8_t* mask, int mask_n, int cg_iters,
                      void* stream) {
    PNP_API_BEGIN
    return mc_install("pnp_set_kspace_mc", e, false, nullptr, (const float2*)y0, (const float2*)sens, coils, sens_n, mask, mask_n, cg_iters, nullptr,
                      nullptr, nullptr, (hipStream_t)stream);
    PNP_API_END("pnp_set_kspace_mc")
}

int pnp_reset_mc(pnp_handle e, const float* x0, const float* y0, const float* sens, int coils, int sens_n, const uint8_t* mask, int mask_n,
                 int cg_iters, float* x, float* z, float* u, void* stream) {
    PNP_API_BEGIN
    return mc_install("pnp_reset_mc", e, true, (const float2*)x0, (const float2*)y0, (const float2*)sens, coils, sens_n, mask, mask_n, cg_iters, x,
                      (float2*)z, (float2*)u, (hipStream_t)stream);
    PNP_API_END("pnp_reset_mc")
}

int pnp_mc_coils(pnp_handle e) { return e && e->stage.kind == STAGE_MC ? e->stage.coils : 0; }

int pnp_mc_cg_residual(pnp_handle e, float* out, void* stream) {
    PNP_API_BEGIN
    return stage_cg_residual("pnp_mc_cg_residual", e, STAGE_MC, out, (hipStream_t)stream);
    PNP_API_END("pnp_mc_cg_residual")
}

int pnp_mc_normal(pnp_handle e, const float* pv, const float* mu, float* q, void* stream) {
    PNP_API_BEGIN
    return stage_normal_op("pnp_mc_normal", e, STAGE_MC, pv, mu, q, (hipStream_t)stream);
    PNP_API_END("pnp_mc_normal")
}

int pnp_acquire_mc(pnp_handle e, const float* gt, const float* sens, int coils, int sens_n, const uint8_t* mask, int mask_n, double sigma_n,
                   uint64_t seed, int flags, float* y0, float* aty0, float* x0, void* stream) {
    PNP_API_BEGIN
    // every rejection happens before any HIP call, and leaves the outputs untouched
    if (flags != 0) return fail(PNP_ERR_INVALID, "pnp_acquire_mc: flags must be 0 (got 0x%x)", (unsigned)flags);
    if (!(sigma_n >= 0.0) || !std::isfinite(sigma_n)) return fail(PNP_ERR_INVALID, "pnp_acquire_mc: sigma_n must be finite and >= 0 (got %g)", sigma_n);
    if (int rc = mc_check_scalars("pnp_acquire_mc", coils, sens_n, mask_n)) return rc;
    if (!gt) return fail(PNP_ERR_INVALID, "pnp_acquire_mc: null gt");
    if (!sens) return fail(PNP_ERR_INVALID, "pnp_acquire_mc: null sens");
    if (!mask) return fail(PNP_ERR_INVALID, "pnp_acquire_mc: null mask");
    if (!y0) return fail(PNP_ERR_INVALID, "pnp_acquire_mc: null y0");
    if (!e) return fail(PNP_ERR_INVALID, "pnp_acquire_mc: null handle");
    if (int rc = mc_check("pnp_acquire_mc", e, coils, sens_n, mask_n)) return rc;
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w;
    PNP_ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = mc_ensure(e, 0, (size_t)N * coils * H * W, 0))) return rc;
    // the plain transforms of S_c gt in the coil scratch, by pnp_acquire's passes; the shifts of fft_c live in the epilogue's indices and sign
    {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_sense_expand(nullptr, gt, (const float2*)sens, sens_n, coils, nullptr, e->mc_work, N, H, W, s));
    }
    if ((rc = plain_fft2(e, e->mc_work, e->mc_work, N * coils, 0, s))) return rc;
    {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_acquire_epilogue(e->mc_work, mask, mask_n, (float2*)y0, sigma_n, seed, N, H, W, s, coils));
    }
    if (!aty0 && !x0) return PNP_OK;
    if ((rc = plain_fft2(e, e->mc_work, e->mc_work, N * coils, 1, s))) return rc;
    float2* const a = aty0 ? (float2*)aty0 : mc_q(e);       // without aty0 the coil sum goes to a CG vector (dead between steps)
    {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_sense_combine(e->mc_work, (const float2*)sens, sens_n, coils, nullptr, nullptr, nullptr, a, nullptr, N, H, W, s));
    }
    if (x0) {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_acquire_clamp(a, (float2*)x0, N, H, W, s));
    }
    return PNP_OK;
    PNP_API_END("pnp_acquire_mc")
}

// ---- non-Cartesian sampling ---------------------------------------------------------------------------
static_assert(PNP_NUFFT_MAX_SAMPLES == kNufftMaxSamples, "the header's limit is the plan's");

namespace {

hipError_t nc_upload(void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }

int nc_need_plan(const char* fn, const pnp_engine* e) {
    return e->nc.m > 0 ? PNP_OK : fail(PNP_ERR_STATE, "%s: the handle has no NUFFT plan (pnp_nufft_plan)", fn);
}
int tz_need_spectrum(const char* fn, const pnp_engine* e) {
    if (int rc = nc_need_plan(fn, e)) return rc;
    return e->tz_planned ? PNP_OK : fail(PNP_ERR_STATE, "%s: the handle has no Toeplitz spectrum (pnp_toeplitz_plan)", fn);
}
// the Toeplitz pass buffer for `planes` planes and, with `coil_images`, the block's coil images
int tz_ensure(pnp_engine* e, size_t planes, bool coil_images) {
    const size_t hw = (size_t)e->cfg.h * e->cfg.w;
    return ws_grow(e, "Toeplitz scratch", {{(void**)&e->tz_grid, &e->tz_grid_cap, planes * (e->tz_fused ? 2 : 4) * hw * sizeof(float2), false},
                                          {(void**)&e->ns_img, &e->ns_img_cap, coil_images ? planes * hw * sizeof(float2) : 0, false}});
}
int or_need_plan(const char* fn, const pnp_engine* e) {
    if (int rc = nc_need_plan(fn, e)) return rc;
    return e->orp.segments > 0 ? PNP_OK : fail(PNP_ERR_STATE, "%s: the handle has no off-resonance plan (pnp_offres_plan)", fn);
}
// the Toeplitz spectra of include/pnpadmm_offres_tz.h, which its installers and applications need
int otz_need_spectra(const char* fn, const pnp_engine* e) {
    if (int rc = or_need_plan(fn, e)) return rc;
    return e->otz_planned ? PNP_OK : fail(PNP_ERR_STATE, "%s: the handle has no Toeplitz off-resonance spectra (pnp_offres_tz_plan)", fn);
}
// the pass buffers of that form for applications over `slices` slices and, multi-coil, `cimg_planes` coil images
int otz_ensure(pnp_engine* e, int slices, size_t cimg_planes) {
    const size_t hw = (size_t)e->cfg.h * e->cfg.w, planes = (size_t)otz_slice_block(e, slices) * e->orp.segments;
    return ws_grow(e, "Toeplitz off-resonance scratch", {{(void**)&e->otz_img, &e->otz_img_cap, planes * hw * sizeof(float2), false},
                                                        {(void**)&e->otz_x, &e->otz_x_cap, planes * 4 * hw * sizeof(float2), false},
                                                        {(void**)&e->otz_y, &e->otz_y_cap, planes * 4 * hw * sizeof(float2), false},
                                                        {(void**)&e->otz_cimg, &e->otz_cimg_cap, cimg_planes * hw * sizeof(float2), false}});
}

// What an entry point's operator takes beyond the NUFFT plan (the arguments' side of NcOp): coil maps, a field map or its segment maps
enum OpTakes { TAKES_COILS = 1, TAKES_MAPS = 2, TAKES_BOTH = 3 };
StageKind stage_kind_of(int takes) {
    static const StageKind kinds[4] = {STAGE_NC, STAGE_NS, STAGE_OR, STAGE_ORS};
    return kinds[takes & 3];
}
// this call's operator: the arguments it was given
NcOp arg_op(int takes, const float2* sens, int coils, int sens_n, const float2* maps, int map_n) {
    return {(takes & TAKES_COILS) ? coils : 0, (takes & TAKES_COILS) ? sens : nullptr, sens_n, (takes & TAKES_MAPS) ? maps : nullptr, map_n};
}

// argument errors shared by the entry points of the non-Cartesian headers, before any HIP call: the scalar ranges need no handle and come
// first (they are reported whatever else is wrong), then what depends on the handle - the counts, the plan, the launch grids' block limit
int op_check_scalars(const char* fn, int takes, int coils, int sens_n, int map_n) {
    if (takes & TAKES_COILS) {
        if (coils < 1 || coils > PNP_MC_MAX_COILS) return fail(PNP_ERR_INVALID, "%s: coils must be 1..%d (got %d)", fn, PNP_MC_MAX_COILS, coils);
        if (sens_n < 1) return fail(PNP_ERR_INVALID, "%s: sens_n must be 1 or n (got %d)", fn, sens_n);
    }
    if ((takes & TAKES_MAPS) && map_n < 1) return fail(PNP_ERR_INVALID, "%s: map_n must be 1 or n (got %d)", fn, map_n);
    return PNP_OK;
}
int op_check(const char* fn, const pnp_engine* e, int takes, int coils, int sens_n, int map_n) {
    const int N = e->cfg.n;
    if ((takes & TAKES_COILS) && sens_n != 1 && sens_n != N) return fail(PNP_ERR_INVALID, "%s: sens_n must be 1 or n=%d", fn, N);
    if ((takes & TAKES_MAPS) && map_n != 1 && map_n != N) return fail(PNP_ERR_INVALID, "%s: map_n must be 1 or n=%d", fn, N);
    if (int rc = (takes & TAKES_MAPS) ? or_need_plan(fn, e) : nc_need_plan(fn, e)) return rc;
    if (takes == TAKES_BOTH) {
        if ((long long)N * om_block_of(e, coils) * or_block_of(e) > 65535)
            return fail(PNP_ERR_INVALID, "%s: n * min(coils, coil block) * min(segments, block) must be <= 65535 (got %d * %d * %d)", fn, N,
                        om_block_of(e, coils), or_block_of(e));
    } else if (takes == TAKES_COILS) {
        if ((long long)N * ns_block_of(e, coils) > 65535)
            return fail(PNP_ERR_INVALID, "%s: n * min(coils, block) must be <= 65535 (got %d * %d)", fn, N, ns_block_of(e, coils));
    } else if (takes == TAKES_MAPS) {
        if ((long long)N * or_block_of(e) > 65535)
            return fail(PNP_ERR_INVALID, "%s: n * min(segments, block) must be <= 65535 (got %d * %d)", fn, N, or_block_of(e));
    }
    return PNP_OK;
}

// The block scratch of an operator that takes coils, maps or both (the plain NUFFT pair's is the plan's own) and `amaps_need` bytes of an
// acquisition's own segment maps.  The coil-block scratch of the non-Cartesian SENSE stage (ns_grid, ns_samp, ns_img) serves a block of coils,
// of segments or of coils x segments; the multi-coil off-resonance operator adds its block's samples and the segment chain's partials
int op_ensure(pnp_engine* e, int takes, int coils, size_t amaps_need = 0) {
    if (!takes) return PNP_OK;
    const size_t N = (size_t)e->cfg.n, HW = (size_t)e->cfg.h * e->cfg.w, M = (size_t)e->nc.m;
    const bool both = takes == TAKES_BOTH;
    const size_t cbc = both ? (size_t)om_block_of(e, coils) : 0;
    const size_t planes = both ? N * cbc * or_block_of(e) : takes == TAKES_COILS ? N * ns_block_of(e, coils) : N * or_block_of(e);
    return ws_grow(e, both ? "multi-coil off-resonance scratch" : takes == TAKES_COILS ? "non-Cartesian SENSE scratch" : "off-resonance scratch",
                   {{(void**)&e->ns_grid, &e->ns_grid_cap, planes * e->nc.gh * e->nc.gw * sizeof(float2), false},
                    {(void**)&e->ns_samp, &e->ns_samp_cap, planes * M * sizeof(float2), false},
                    {(void**)&e->ns_img, &e->ns_img_cap, (e->ns_naive & (NS_PAD | NS_CROP)) ? planes * HW * sizeof(float2) : 0, false},
                    {(void**)&e->om_samp, &e->om_samp_cap, N * cbc * M * sizeof(float2), false},
                    // the partials: the fused crop touches them only when the segments do not fit one block; the composed adjoint's coil images
                    {(void**)&e->om_part, &e->om_part_cap,
                     both && ((e->om_naive & ORM_CROP) || e->orp.segments > or_block_of(e)) ? N * cbc * HW * sizeof(float2) : 0, false},
                    {(void**)&e->om_img, &e->om_img_cap, both && e->om_naive ? N * HW * sizeof(float2) : 0, false},
                    {(void**)&e->om_line, &e->om_line_cap, both && e->om_naive ? N * M * sizeof(float2) : 0, false},
                    {(void**)&e->acq_maps, &e->acq_maps_cap, amaps_need, false}});
}

// The twelve pnp_set_kspace_* (no iterate) / pnp_reset_* members of the non-Cartesian headers: the episode constants of the stage `takes`
// names - y, w, the coil maps, the segment maps of omega, A^H W y - and optionally the iterate.  `toeplitz`: a _tz installer, whose CG runs
// on the spectrum of the stage's kind (w: the spectrum's weights, whatever is passed).  Every rejection happens before any HIP call.  The
// constants grow last, after every scratch grow has succeeded: an allocation failure leaves the live stage's constants as they were
int nc_install(const char* fn, pnp_engine* e, int takes, bool with_iterate, bool toeplitz, const float2* x0, const float2* y, const float2* sens,
               int coils, int sens_n, const float* omega, int map_n, const float* w, int cg_iters, float* x, float2* z, float2* u, hipStream_t s) {
    const bool has_coils = takes & TAKES_COILS, segmented = takes & TAKES_MAPS;
    int rc;
    if ((rc = op_check_scalars(fn, takes, coils, sens_n, map_n))) return rc;
    if (cg_iters < 1 || cg_iters > PNP_MC_MAX_CG) return fail(PNP_ERR_INVALID, "%s: cg_iters must be 1..%d (got %d)", fn, PNP_MC_MAX_CG, cg_iters);
    if (with_iterate && !x0) return fail(PNP_ERR_INVALID, "%s: null x0", fn);
    if (!y) return fail(PNP_ERR_INVALID, "%s: null y", fn);
    if (has_coils && !sens) return fail(PNP_ERR_INVALID, "%s: null sens", fn);
    if (segmented && !omega) return fail(PNP_ERR_INVALID, "%s: null omega", fn);
    if (with_iterate && (!x || !z || !u)) return fail(PNP_ERR_INVALID, "%s: null x, z or u", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if ((rc = op_check(fn, e, takes, coils, sens_n, map_n))) return rc;
    if (toeplitz && (rc = segmented ? otz_need_spectra(fn, e) : tz_need_spectrum(fn, e))) return rc;
    PNP_ON_DEVICE(e);
    if (toeplitz) w = segmented ? (e->otz_has_w ? e->otz_w : nullptr) : (e->tz_has_w ? e->tz_w : nullptr);
    if (!has_coils) { coils = 0; sens_n = 1; }
    if (!segmented) map_n = 1;
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w, L = e->orp.segments;
    const size_t M = (size_t)e->nc.m, lines = (size_t)N * (has_coils ? coils : 1), sn = (size_t)sens_n * coils * H * W;
    if ((rc = mc_ensure(e, 0, 0, 0))) return rc;            // the CG vectors, partial sums and scalars: the coil workspace's, coil-independent
    if ((rc = op_ensure(e, takes, coils))) return rc;
    if (toeplitz && segmented) {
        const int cb = has_coils ? otz_coil_block(e, coils, map_n) : 1;
        if ((rc = otz_ensure(e, N * cb, has_coils ? (size_t)N * cb : 0))) return rc;
    } else if (toeplitz && has_coils) {
        if ((rc = tz_ensure(e, (size_t)N * ns_block_of(e, coils), true))) return rc;
    }
    static const char* const labels[4] = {"non-Cartesian constants", "non-Cartesian SENSE constants", "off-resonance constants",
                                          "multi-coil off-resonance constants"};
    if ((rc = ws_grow(e, labels[takes & 3],
                      {{(void**)&e->st_y, &e->st_y_cap, lines * M * sizeof(float2), false},
                       {(void**)&e->st_sens, &e->st_sens_cap, sn * sizeof(float2), false},
                       {(void**)&e->st_maps, &e->st_maps_cap, segmented ? (size_t)map_n * L * H * W * sizeof(float2) : 0, false},
                       {(void**)&e->st_w, &e->st_w_cap, w ? M * sizeof(float) : 0, false},
                       {(void**)&e->st_mpart, &e->st_mpart_cap, lines * nufft_sample_chunks((int64_t)M) * sizeof(double), false}})))
        return rc;
    HIP_TRY(hipMemcpyAsync(e->st_y, y, lines * M * sizeof(float2), hipMemcpyDeviceToDevice, s));
    if (has_coils) HIP_TRY(hipMemcpyAsync(e->st_sens, sens, sn * sizeof(float2), hipMemcpyDeviceToDevice, s));
    if (w) HIP_TRY(hipMemcpyAsync(e->st_w, w, M * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemsetAsync(e->mc_sc, 0, (size_t)N * 8 * sizeof(double), s));
    if (segmented) {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_offres_maps(omega, map_n, e->orp, e->nc, e->st_maps, s));
    }
    const NcOp o = arg_op(takes, e->st_sens, coils, sens_n, e->st_maps, map_n);
    if ((rc = op_adjoint(e, o, e->st_y, w ? e->st_w : nullptr, N, mc_aty(e), s))) return rc;
    if (with_iterate) {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_sense_iterate(x0, x, z, u, N, H, W, s));
    }
    commit_stage(e, {stage_kind_of(takes), !toeplitz ? FORM_GRID : segmented ? FORM_OTZ : FORM_TZ, coils, sens_n, cg_iters, w != nullptr, map_n});
    return PNP_OK;
}

// The four pnp_acquire_* members of the non-Cartesian headers: y = A gt + noise on the operator `takes` names and, where asked, aty0 = A^H
// (dcf . y) and x0 = max(aty0, 0).  A segmented acquisition's maps go to a buffer of its own: it disturbs no live episode.  Every rejection
// happens before any HIP call, and leaves the outputs untouched
int nc_acquire(const char* fn, pnp_engine* e, int takes, const float* gt, const float* sens, int coils, int sens_n, const float* omega, int map_n,
               const float* dcf, double sigma_n, uint64_t seed, int flags, float* y, float* aty0, float* x0, hipStream_t s) {
    const bool has_coils = takes & TAKES_COILS, segmented = takes & TAKES_MAPS;
    if (flags != 0) return fail(PNP_ERR_INVALID, "%s: flags must be 0 (got 0x%x)", fn, (unsigned)flags);
    if (!(sigma_n >= 0.0) || !std::isfinite(sigma_n)) return fail(PNP_ERR_INVALID, "%s: sigma_n must be finite and >= 0 (got %g)", fn, sigma_n);
    if (int rc = op_check_scalars(fn, takes, coils, sens_n, map_n)) return rc;
    if (!gt) return fail(PNP_ERR_INVALID, "%s: null gt", fn);
    if (has_coils && !sens) return fail(PNP_ERR_INVALID, "%s: null sens", fn);
    if (segmented && !omega) return fail(PNP_ERR_INVALID, "%s: null omega", fn);
    if (!y) return fail(PNP_ERR_INVALID, "%s: null y", fn);
    if (takes) {                                            // (the plain pair's acquisition names no aliasing rule)
        const auto input = [&](const float* p) { return p == gt || (has_coils && p == sens) || (segmented && p == omega); };
        if (input(y) || (aty0 && (input(aty0) || aty0 == y)) || (x0 && (input(x0) || x0 == y)))
            return fail(PNP_ERR_INVALID, "%s: no output may alias gt, %s or another output", fn,
                        !segmented ? "sens" : has_coils ? "sens, omega" : "omega");
    }
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (int rc = op_check(fn, e, takes, coils, sens_n, map_n)) return rc;
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w;
    PNP_ON_DEVICE(e);
    int rc;
    if ((rc = op_ensure(e, takes, coils, segmented ? (size_t)map_n * e->orp.segments * H * W * sizeof(float2) : 0))) return rc;
    if (segmented) {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_offres_maps(omega, map_n, e->orp, e->nc, e->acq_maps, s));
    }
    const NcOp o = arg_op(takes, (const float2*)sens, coils, sens_n, e->acq_maps, map_n);
    if ((rc = op_forward(e, o, nullptr, gt, N, (float2*)y, s))) return rc;
    if (sigma_n != 0.0) {                                   // a noiseless acquisition draws nothing and keeps the forward's own bits
        Prof p(e, s, PROF_OTHER, -1);
        if (has_coils) HIP_TRY(launch_ncsense_noise((float2*)y, sigma_n, seed, coils, e->nc, N, s));
        else HIP_TRY(launch_nufft_noise((float2*)y, sigma_n, seed, e->nc, N, s));
    }
    if (!aty0 && !x0) return PNP_OK;
    float2* const a = aty0 ? (float2*)aty0 : e->d_work;     // without aty0 the image goes to the data-fidelity stage's scratch plane
    if ((rc = op_adjoint(e, o, (const float2*)y, dcf, N, a, s))) return rc;
    if (x0) {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_acquire_clamp(a, (float2*)x0, N, H, W, s));
    }
    return PNP_OK;
}

}  // namespace

int pnp_nufft_plan(pnp_handle e, const double* traj, int64_t m, int gh, int gw, int width, int flags) {
    PNP_API_BEGIN
    // every rejection happens before any HIP call and leaves the handle as it was; scalar ranges first
    if (flags != 0) return fail(PNP_ERR_INVALID, "pnp_nufft_plan: flags must be 0 (got 0x%x)", (unsigned)flags);
    if (m < 1 || m > PNP_NUFFT_MAX_SAMPLES) return fail(PNP_ERR_INVALID, "pnp_nufft_plan: m must be 1..%lld (got %lld)", (long long)PNP_NUFFT_MAX_SAMPLES, (long long)m);
    if (width != 4 && width != 6 && width != 8) return fail(PNP_ERR_INVALID, "pnp_nufft_plan: width must be 4, 6 or 8 (got %d)", width);
    if (gh < 0 || gw < 0) return fail(PNP_ERR_INVALID, "pnp_nufft_plan: gh, gw must be 0 or a grid side (got %dx%d)", gh, gw);
    if (!traj) return fail(PNP_ERR_INVALID, "pnp_nufft_plan: null traj");
    if (!e) return fail(PNP_ERR_INVALID, "pnp_nufft_plan: null handle");
    NufftPlan P;
    std::string why;
    if (!plan_nufft(e->cfg.h, e->cfg.w, gh, gw, width, traj, m, &P, &why)) return fail(PNP_ERR_INVALID, "pnp_nufft_plan: %s", why.c_str());
    const std::vector<float2> twh = twiddle_table(P.gh), tww = twiddle_table(P.gw);
    PNP_ON_DEVICE(e);
    NufftDev& D = e->nc;
    const size_t N = (size_t)e->cfg.n, G = (size_t)P.gh * P.gw, M = (size_t)P.m;
    if (int rc = ws_grow(e, "NUFFT plan", {{(void**)&D.i0, &e->nc_i0_cap, P.i0.size() * sizeof(int32_t), false},
                                           {(void**)&D.wts, &e->nc_wts_cap, P.wts.size() * sizeof(float), false},
                                           {(void**)&D.cy, &e->nc_cy_cap, P.cy.size() * sizeof(float), false},
                                           {(void**)&D.cx, &e->nc_cx_cap, P.cx.size() * sizeof(float), false},
                                           {(void**)&D.bin_off, &e->nc_off_cap, P.bin_off.size() * sizeof(int32_t), false},
                                           {(void**)&D.bin_idx, &e->nc_idx_cap, P.bin_idx.size() * sizeof(int32_t), false},
                                           {(void**)&D.tw_gh, &e->nc_twh_cap, twh.size() * sizeof(float2), false},
                                           {(void**)&D.tw_gw, &e->nc_tww_cap, tww.size() * sizeof(float2), false},
                                           {(void**)&e->nc_grid, &e->nc_grid_cap, N * G * sizeof(float2), false},
                                           {(void**)&e->nc_samp, &e->nc_samp_cap, N * M * sizeof(float2), false}}))
        return rc;
    if (D.m > 0) (void)hipDeviceSynchronize();              // no launch still reads the plan being replaced
    // from here on the old plan is gone: its non-Cartesian constants are dropped with it
    D.m = 0;
    drop_stage(e, DROP_NONCART);
    e->tz_planned = false;                                  // the spectrum belongs to the plan it was built for
    e->orp.segments = 0;                                    // ... and so does the off-resonance plan
    e->orp.kind = 0;
    e->otz_planned = false;                                 // ... and the spectra built on the two
    e->nc_traj.assign(traj, traj + 2 * (size_t)m);
    e->nc_bin_off_h = P.bin_off;
    e->nc_bin_idx_h = P.bin_idx;
    HIP_TRY(nc_upload(D.i0, P.i0.data(), P.i0.size() * sizeof(int32_t)));
    HIP_TRY(nc_upload(D.wts, P.wts.data(), P.wts.size() * sizeof(float)));
    HIP_TRY(nc_upload(D.cy, P.cy.data(), P.cy.size() * sizeof(float)));
    HIP_TRY(nc_upload(D.cx, P.cx.data(), P.cx.size() * sizeof(float)));
    HIP_TRY(nc_upload(D.bin_off, P.bin_off.data(), P.bin_off.size() * sizeof(int32_t)));
    HIP_TRY(nc_upload(D.bin_idx, P.bin_idx.data(), P.bin_idx.size() * sizeof(int32_t)));
    HIP_TRY(nc_upload(D.tw_gh, twh.data(), twh.size() * sizeof(float2)));
    HIP_TRY(nc_upload(D.tw_gw, tww.data(), tww.size() * sizeof(float2)));
    D.h = P.h; D.w = P.w; D.gh = P.gh; D.gw = P.gw; D.width = P.width; D.tiles_y = P.tiles_y; D.tiles_x = P.tiles_x;
    D.m = P.m;
    return PNP_OK;
    PNP_API_END("pnp_nufft_plan")
}

int64_t pnp_nufft_samples(pnp_handle e) { return e ? e->nc.m : 0; }

int pnp_nufft_grid(pnp_handle e, int* gh, int* gw) {
    PNP_API_BEGIN
    if (!e || !gh || !gw) return fail(PNP_ERR_INVALID, "pnp_nufft_grid: null argument");
    if (int rc = nc_need_plan("pnp_nufft_grid", e)) return rc;
    *gh = e->nc.gh; *gw = e->nc.gw;
    return PNP_OK;
    PNP_API_END("pnp_nufft_grid")
}

int pnp_nufft_forward(pnp_handle e, const float* img, int batch, float* samples, void* stream) {
    PNP_API_BEGIN
    if (batch < 1) return fail(PNP_ERR_INVALID, "pnp_nufft_forward: batch must be 1..n (got %d)", batch);
    if (!img) return fail(PNP_ERR_INVALID, "pnp_nufft_forward: null img");
    if (!samples) return fail(PNP_ERR_INVALID, "pnp_nufft_forward: null samples");
    if (img == samples) return fail(PNP_ERR_INVALID, "pnp_nufft_forward: samples must not alias img");
    if (!e) return fail(PNP_ERR_INVALID, "pnp_nufft_forward: null handle");
    if (batch > e->cfg.n) return fail(PNP_ERR_INVALID, "pnp_nufft_forward: batch must be 1..n=%d (got %d)", e->cfg.n, batch);
    if (int rc = nc_need_plan("pnp_nufft_forward", e)) return rc;
    PNP_ON_DEVICE(e);
    return nc_forward(e, (const float2*)img, nullptr, batch, (float2*)samples, (hipStream_t)stream);
    PNP_API_END("pnp_nufft_forward")
}

int pnp_nufft_adjoint(pnp_handle e, const float* samples, const float* weights, int batch, float* img, void* stream) {
    PNP_API_BEGIN
    if (batch < 1) return fail(PNP_ERR_INVALID, "pnp_nufft_adjoint: batch must be 1..n (got %d)", batch);
    if (!samples) return fail(PNP_ERR_INVALID, "pnp_nufft_adjoint: null samples");
    if (!img) return fail(PNP_ERR_INVALID, "pnp_nufft_adjoint: null img");
    if (img == samples || (const float*)img == weights) return fail(PNP_ERR_INVALID, "pnp_nufft_adjoint: img must not alias samples or weights");
    if (!e) return fail(PNP_ERR_INVALID, "pnp_nufft_adjoint: null handle");
    if (batch > e->cfg.n) return fail(PNP_ERR_INVALID, "pnp_nufft_adjoint: batch must be 1..n=%d (got %d)", e->cfg.n, batch);
    if (int rc = nc_need_plan("pnp_nufft_adjoint", e)) return rc;
    PNP_ON_DEVICE(e);
    return nc_adjoint(e, (const float2*)samples, weights, batch, nullptr, nullptr, nullptr, (float2*)img, nullptr, (hipStream_t)stream);
    PNP_API_END("pnp_nufft_adjoint")
}

int pnp_set_kspace_nc(pnp_handle e, const float* y, const float* w, int cg_iters, void* stream) {
    PNP_API_BEGIN
    return nc_install("pnp_set_kspace_nc", e, 0, false, false, nullptr, (const float2*)y, nullptr, 0, 1, nullptr, 1, w, cg_iters, nullptr, nullptr,
                      nullptr, (hipStream_t)stream);
    PNP_API_END("pnp_set_kspace_nc")
}

int pnp_reset_nc(pnp_handle e, const float* x0, const float* y, const float* w, int cg_iters, float* x, float* z, float* u, void* stream) {
    PNP_API_BEGIN
    return nc_install("pnp_reset_nc", e, 0, true, false, (const float2*)x0, (const float2*)y, nullptr, 0, 1, nullptr, 1, w, cg_iters, x, (float2*)z,
                      (float2*)u, (hipStream_t)stream);
    PNP_API_END("pnp_reset_nc")
}

int pnp_nc_cg_residual(pnp_handle e, float* out, void* stream) {
    PNP_API_BEGIN
    return stage_cg_residual("pnp_nc_cg_residual", e, STAGE_NC, out, (hipStream_t)stream);
    PNP_API_END("pnp_nc_cg_residual")
}

int pnp_nc_normal(pnp_handle e, const float* pv, const float* mu, float* q, void* stream) {
    PNP_API_BEGIN
    return stage_normal_op("pnp_nc_normal", e, STAGE_NC, pv, mu, q, (hipStream_t)stream);
    PNP_API_END("pnp_nc_normal")
}

int pnp_acquire_nc(pnp_handle e, const float* gt, const float* dcf, double sigma_n, uint64_t seed, int flags, float* y, float* aty0, float* x0,
                   void* stream) {
    PNP_API_BEGIN
    return nc_acquire("pnp_acquire_nc", e, 0, gt, nullptr, 0, 1, nullptr, 1, dcf, sigma_n, seed, flags, y, aty0, x0, (hipStream_t)stream);
    PNP_API_END("pnp_acquire_nc")
}

// ---- non-Cartesian SENSE (include/pnpadmm_ncsense.h) ---------------------------------------------------
int pnp_nufft_forward_mc(pnp_handle e, const float* img, const float* sens, int coils, int sens_n, int batch, float* samples, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_nufft_forward_mc";
    if (int rc = op_check_scalars(fn, TAKES_COILS, coils, sens_n, 0)) return rc;
    if (batch < 1) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n (got %d)", fn, batch);
    if (!img) return fail(PNP_ERR_INVALID, "%s: null img", fn);
    if (!sens) return fail(PNP_ERR_INVALID, "%s: null sens", fn);
    if (!samples) return fail(PNP_ERR_INVALID, "%s: null samples", fn);
    if (samples == img || samples == sens) return fail(PNP_ERR_INVALID, "%s: samples must not alias img or sens", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (batch > e->cfg.n) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n=%d (got %d)", fn, e->cfg.n, batch);
    if (int rc = op_check(fn, e, TAKES_COILS, coils, sens_n, 0)) return rc;
    PNP_ON_DEVICE(e);
    if (int rc = op_ensure(e, TAKES_COILS, coils)) return rc;
    return ns_forward(e, (const float2*)img, nullptr, (const float2*)sens, sens_n, coils, batch, (float2*)samples, (hipStream_t)stream);
    PNP_API_END("pnp_nufft_forward_mc")
}

int pnp_nufft_adjoint_mc(pnp_handle e, const float* samples, const float* weights, const float* sens, int coils, int sens_n, int batch, float* img,
                         void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_nufft_adjoint_mc";
    if (int rc = op_check_scalars(fn, TAKES_COILS, coils, sens_n, 0)) return rc;
    if (batch < 1) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n (got %d)", fn, batch);
    if (!samples) return fail(PNP_ERR_INVALID, "%s: null samples", fn);
    if (!sens) return fail(PNP_ERR_INVALID, "%s: null sens", fn);
    if (!img) return fail(PNP_ERR_INVALID, "%s: null img", fn);
    if (img == samples || img == sens || (const float*)img == weights) return fail(PNP_ERR_INVALID, "%s: img must not alias samples, weights or sens", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (batch > e->cfg.n) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n=%d (got %d)", fn, e->cfg.n, batch);
    if (int rc = op_check(fn, e, TAKES_COILS, coils, sens_n, 0)) return rc;
    PNP_ON_DEVICE(e);
    if (int rc = op_ensure(e, TAKES_COILS, coils)) return rc;
    return ns_adjoint(e, (const float2*)samples, weights, (const float2*)sens, sens_n, coils, batch, (float2*)img, (hipStream_t)stream);
    PNP_API_END("pnp_nufft_adjoint_mc")
}

int pnp_set_kspace_ncsense(pnp_handle e, const float* y, const float* sens, int coils, int sens_n, const float* w, int cg_iters, void* stream) {
    PNP_API_BEGIN
    return nc_install("pnp_set_kspace_ncsense", e, TAKES_COILS, false, false, nullptr, (const float2*)y, (const float2*)sens, coils, sens_n, nullptr,
                      1, w, cg_iters, nullptr, nullptr, nullptr, (hipStream_t)stream);
    PNP_API_END("pnp_set_kspace_ncsense")
}

int pnp_reset_ncsense(pnp_handle e, const float* x0, const float* y, const float* sens, int coils, int sens_n, const float* w, int cg_iters, float* x,
                      float* z, float* u, void* stream) {
    PNP_API_BEGIN
    return nc_install("pnp_reset_ncsense", e, TAKES_COILS, true, false, (const float2*)x0, (const float2*)y, (const float2*)sens, coils, sens_n,
                      nullptr, 1, w, cg_iters, x, (float2*)z, (float2*)u, (hipStream_t)stream);
    PNP_API_END("pnp_reset_ncsense")
}

int pnp_ncsense_coils(pnp_handle e) { return e && e->stage.kind == STAGE_NS ? e->stage.coils : 0; }

int pnp_ncsense_cg_residual(pnp_handle e, float* out, void* stream) {
    PNP_API_BEGIN
    return stage_cg_residual("pnp_ncsense_cg_residual", e, STAGE_NS, out, (hipStream_t)stream);
    PNP_API_END("pnp_ncsense_cg_residual")
}

int pnp_ncsense_normal(pnp_handle e, const float* pv, const float* mu, float* q, void* stream) {
    PNP_API_BEGIN
    return stage_normal_op("pnp_ncsense_normal", e, STAGE_NS, pv, mu, q, (hipStream_t)stream);
    PNP_API_END("pnp_ncsense_normal")
}

int pnp_acquire_ncsense(pnp_handle e, const float* gt, const float* sens, int coils, int sens_n, const float* dcf, double sigma_n, uint64_t seed,
                        int flags, float* y, float* aty0, float* x0, void* stream) {
    PNP_API_BEGIN
    return nc_acquire("pnp_acquire_ncsense", e, TAKES_COILS, gt, sens, coils, sens_n, nullptr, 1, dcf, sigma_n, seed, flags, y, aty0, x0,
                      (hipStream_t)stream);
    PNP_API_END("pnp_acquire_ncsense")
}

// ---- off-resonance correction (include/pnpadmm_offres.h) -------------------------------------------------
static_assert(PNP_MC_MAX_COILS == kOffresMaxSegments, "the header's limit is the plan's");

int pnp_offres_plan(pnp_handle e, const double* t, int segments, int flags) {
    PNP_API_BEGIN
    const char* fn = "pnp_offres_plan";
    // every rejection happens before any HIP call and leaves the handle as it was; scalar ranges first
    if (flags != 0) return fail(PNP_ERR_INVALID, "%s: flags must be 0 (got 0x%x)", fn, (unsigned)flags);
    if (segments < 1 || segments > PNP_MC_MAX_COILS) return fail(PNP_ERR_INVALID, "%s: segments must be 1..%d (got %d)", fn, PNP_MC_MAX_COILS, segments);
    if (!t) return fail(PNP_ERR_INVALID, "%s: null t", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (int rc = nc_need_plan(fn, e)) return rc;
    OffresPlan P;
    std::string why;
    const int tiles = e->nc.tiles_y * e->nc.tiles_x;
    if (!plan_offres(t, e->nc.m, segments, tiles, e->nc_bin_off_h.data(), e->nc_bin_idx_h.data(), &P, &why)) return fail(PNP_ERR_INVALID, "%s: %s", fn, why.c_str());
    PNP_ON_DEVICE(e);
    OffresDev& D = e->orp;
    const size_t M = (size_t)P.m;
    if (int rc = ws_grow(e, "off-resonance plan", {{(void**)&D.tau, &e->or_tau_cap, P.tau.size() * sizeof(double), false},
                                                   {(void**)&D.seg, &e->or_seg_cap, M * sizeof(int32_t), false},
                                                   {(void**)&D.b0, &e->or_b0_cap, M * sizeof(float), false},
                                                   {(void**)&D.b1, &e->or_b1_cap, M * sizeof(float), false},
                                                   {(void**)&D.list_off, &e->or_loff_cap, P.list_off.size() * sizeof(int32_t), false},
                                                   {(void**)&D.list_idx, &e->or_lidx_cap, std::max<size_t>(P.list_idx.size(), 1) * sizeof(int32_t), false}}))
        return rc;
    if (D.segments > 0) (void)hipDeviceSynchronize();       // no launch still reads the plan being replaced
    // from here on the old plan is gone: a live off-resonance stage's maps belong to its centres and are dropped with it
    D.segments = 0;
    D.kind = 0;
    e->otz_planned = false;                                 // the Toeplitz spectra belong to the plan's coefficients
    drop_stage(e, DROP_SEGMENTED);
    e->or_seg_h = P.seg;
    HIP_TRY(nc_upload(D.tau, P.tau.data(), P.tau.size() * sizeof(double)));
    HIP_TRY(nc_upload(D.seg, P.seg.data(), M * sizeof(int32_t)));
    HIP_TRY(nc_upload(D.b0, P.b0.data(), M * sizeof(float)));
    HIP_TRY(nc_upload(D.b1, P.b1.data(), M * sizeof(float)));
    HIP_TRY(nc_upload(D.list_off, P.list_off.data(), P.list_off.size() * sizeof(int32_t)));
    if (!P.list_idx.empty()) HIP_TRY(nc_upload(D.list_idx, P.list_idx.data(), P.list_idx.size() * sizeof(int32_t)));
    D.segments = P.segments;
    D.kind = 1;
    return PNP_OK;
    PNP_API_END("pnp_offres_plan")
}

// ---- the least-squares interpolator (include/pnpadmm_offres_ls.h) ----
int pnp_offres_plan_ls(pnp_handle e, const double* t, int segments, double omega_max, int flags) {
    PNP_API_BEGIN
    const char* fn = "pnp_offres_plan_ls";
    // every rejection happens before any HIP call and leaves the handle as it was; scalar ranges first
    if (flags != 0) return fail(PNP_ERR_INVALID, "%s: flags must be 0 (got 0x%x)", fn, (unsigned)flags);
    if (segments < 1 || segments > PNP_MC_MAX_COILS) return fail(PNP_ERR_INVALID, "%s: segments must be 1..%d (got %d)", fn, PNP_MC_MAX_COILS, segments);
    if (segments > 1 && (!std::isfinite(omega_max) || !(omega_max > 0.0)))
        return fail(PNP_ERR_INVALID, "%s: omega_max must be finite and > 0 (got %g)", fn, omega_max);
    if (!t) return fail(PNP_ERR_INVALID, "%s: null t", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (int rc = nc_need_plan(fn, e)) return rc;
    OffresLsPlan P;
    std::string why;
    if (!plan_offres_ls(t, e->nc.m, segments, omega_max, &P, &why)) return fail(PNP_ERR_INVALID, "%s: %s", fn, why.c_str());
    PNP_ON_DEVICE(e);
    OffresDev& D = e->orp;
    if (int rc = ws_grow(e, "off-resonance plan", {{(void**)&D.tau, &e->or_tau_cap, P.tau.size() * sizeof(double), false},
                                                   {(void**)&D.coef, &e->or_coef_cap, P.coef.size() * sizeof(float), false}}))
        return rc;
    if (D.segments > 0) (void)hipDeviceSynchronize();       // no launch still reads the plan being replaced
    // from here on the old plan is gone: a live off-resonance stage's maps belong to its plan and are dropped with it
    D.segments = 0;
    D.kind = 0;
    e->otz_planned = false;                                 // the Toeplitz spectra belong to the plan's coefficients
    drop_stage(e, DROP_SEGMENTED);
    HIP_TRY(nc_upload(D.tau, P.tau.data(), P.tau.size() * sizeof(double)));
    HIP_TRY(nc_upload(D.coef, P.coef.data(), P.coef.size() * sizeof(float)));
    D.segments = P.segments;
    D.kind = 2;
    return PNP_OK;
    PNP_API_END("pnp_offres_plan_ls")
}

int pnp_offres_interpolator(pnp_handle e) { return e && e->nc.m > 0 && e->orp.segments > 0 ? e->orp.kind : 0; }

int pnp_offres_ls_coeffs(pnp_handle e, float* coef_host) {
    PNP_API_BEGIN
    const char* fn = "pnp_offres_ls_coeffs";
    if (!coef_host) return fail(PNP_ERR_INVALID, "%s: null coef_host", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (int rc = nc_need_plan(fn, e)) return rc;
    if (e->orp.segments < 1 || e->orp.kind != 2)
        return fail(PNP_ERR_STATE, "%s: the handle has no least-squares off-resonance plan (pnp_offres_plan_ls)", fn);
    PNP_ON_DEVICE(e);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(coef_host, e->orp.coef, (size_t)e->orp.segments * (size_t)e->nc.m * sizeof(float), hipMemcpyDeviceToHost));
    return PNP_OK;
    PNP_API_END("pnp_offres_ls_coeffs")
}

int pnp_offres_segments(pnp_handle e) { return e && e->nc.m > 0 ? e->orp.segments : 0; }

int pnp_offres_maps(pnp_handle e, const float* omega, int map_n, float* maps, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_offres_maps";
    if (int rc = op_check_scalars(fn, TAKES_MAPS, 0, 0, map_n)) return rc;
    if (!omega) return fail(PNP_ERR_INVALID, "%s: null omega", fn);
    if (!maps) return fail(PNP_ERR_INVALID, "%s: null maps", fn);
    if (maps == omega) return fail(PNP_ERR_INVALID, "%s: maps must not alias omega", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (int rc = op_check(fn, e, TAKES_MAPS, 0, 0, map_n)) return rc;
    PNP_ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    Prof p(e, s, PROF_OTHER, -1);
    HIP_TRY(launch_offres_maps(omega, map_n, e->orp, e->nc, (float2*)maps, s));
    return PNP_OK;
    PNP_API_END("pnp_offres_maps")
}

int pnp_offres_forward(pnp_handle e, const float* img, const float* maps, int map_n, int batch, float* samples, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_offres_forward";
    if (int rc = op_check_scalars(fn, TAKES_MAPS, 0, 0, map_n)) return rc;
    if (batch < 1) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n (got %d)", fn, batch);
    if (!img) return fail(PNP_ERR_INVALID, "%s: null img", fn);
    if (!maps) return fail(PNP_ERR_INVALID, "%s: null maps", fn);
    if (!samples) return fail(PNP_ERR_INVALID, "%s: null samples", fn);
    if (samples == img || samples == maps) return fail(PNP_ERR_INVALID, "%s: samples must not alias img or maps", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (batch > e->cfg.n) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n=%d (got %d)", fn, e->cfg.n, batch);
    if (int rc = op_check(fn, e, TAKES_MAPS, 0, 0, map_n)) return rc;
    PNP_ON_DEVICE(e);
    if (int rc = op_ensure(e, TAKES_MAPS, 0)) return rc;
    return or_forward(e, (const float2*)img, nullptr, (const float2*)maps, map_n, batch, (float2*)samples, (hipStream_t)stream);
    PNP_API_END("pnp_offres_forward")
}

int pnp_offres_adjoint(pnp_handle e, const float* samples, const float* weights, const float* maps, int map_n, int batch, float* img, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_offres_adjoint";
    if (int rc = op_check_scalars(fn, TAKES_MAPS, 0, 0, map_n)) return rc;
    if (batch < 1) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n (got %d)", fn, batch);
    if (!samples) return fail(PNP_ERR_INVALID, "%s: null samples", fn);
    if (!maps) return fail(PNP_ERR_INVALID, "%s: null maps", fn);
    if (!img) return fail(PNP_ERR_INVALID, "%s: null img", fn);
    if (img == samples || img == maps || (const float*)img == weights) return fail(PNP_ERR_INVALID, "%s: img must not alias samples, weights or maps", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (batch > e->cfg.n) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n=%d (got %d)", fn, e->cfg.n, batch);
    if (int rc = op_check(fn, e, TAKES_MAPS, 0, 0, map_n)) return rc;
    PNP_ON_DEVICE(e);
    if (int rc = op_ensure(e, TAKES_MAPS, 0)) return rc;
    return or_adjoint(e, (const float2*)samples, weights, (const float2*)maps, map_n, batch, nullptr, nullptr, nullptr, (float2*)img, nullptr,
                      (hipStream_t)stream);
    PNP_API_END("pnp_offres_adjoint")
}

int pnp_set_kspace_offres(pnp_handle e, const float* y, const float* omega, int map_n, const float* w, int cg_iters, void* stream) {
    PNP_API_BEGIN
    return nc_install("pnp_set_kspace_offres", e, TAKES_MAPS, false, false, nullptr, (const float2*)y, nullptr, 0, 1, omega, map_n, w, cg_iters,
                      nullptr, nullptr, nullptr, (hipStream_t)stream);
    PNP_API_END("pnp_set_kspace_offres")
}

int pnp_reset_offres(pnp_handle e, const float* x0, const float* y, const float* omega, int map_n, const float* w, int cg_iters, float* x, float* z,
                     float* u, void* stream) {
    PNP_API_BEGIN
    return nc_install("pnp_reset_offres", e, TAKES_MAPS, true, false, (const float2*)x0, (const float2*)y, nullptr, 0, 1, omega, map_n, w, cg_iters,
                      x, (float2*)z, (float2*)u, (hipStream_t)stream);
    PNP_API_END("pnp_reset_offres")
}

int pnp_offres_live(pnp_handle e) { return e && e->stage.kind == STAGE_OR ? 1 : 0; }

int pnp_offres_cg_residual(pnp_handle e, float* out, void* stream) {
    PNP_API_BEGIN
    return stage_cg_residual("pnp_offres_cg_residual", e, STAGE_OR, out, (hipStream_t)stream);
    PNP_API_END("pnp_offres_cg_residual")
}

int pnp_offres_normal(pnp_handle e, const float* pv, const float* mu, float* q, void* stream) {
    PNP_API_BEGIN
    return stage_normal_op("pnp_offres_normal", e, STAGE_OR, pv, mu, q, (hipStream_t)stream);
    PNP_API_END("pnp_offres_normal")
}

int pnp_acquire_offres(pnp_handle e, const float* gt, const float* omega, int map_n, const float* dcf, double sigma_n, uint64_t seed, int flags,
                       float* y, float* aty0, float* x0, void* stream) {
    PNP_API_BEGIN
    return nc_acquire("pnp_acquire_offres", e, TAKES_MAPS, gt, nullptr, 0, 1, omega, map_n, dcf, sigma_n, seed, flags, y, aty0, x0,
                      (hipStream_t)stream);
    PNP_API_END("pnp_acquire_offres")
}

// ---- off-resonance correction for multi-coil data (include/pnpadmm_offres_mc.h) ----------------------------
int pnp_offres_forward_mc(pnp_handle e, const float* img, const float* maps, int map_n, const float* sens, int sens_n, int coils, int batch,
                          float* samples, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_offres_forward_mc";
    if (int rc = op_check_scalars(fn, TAKES_BOTH, coils, sens_n, map_n)) return rc;
    if (batch < 1) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n (got %d)", fn, batch);
    if (!img) return fail(PNP_ERR_INVALID, "%s: null img", fn);
    if (!maps) return fail(PNP_ERR_INVALID, "%s: null maps", fn);
    if (!sens) return fail(PNP_ERR_INVALID, "%s: null sens", fn);
    if (!samples) return fail(PNP_ERR_INVALID, "%s: null samples", fn);
    if (samples == img || samples == maps || samples == sens) return fail(PNP_ERR_INVALID, "%s: samples must not alias img, maps or sens", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (batch > e->cfg.n) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n=%d (got %d)", fn, e->cfg.n, batch);
    if (int rc = op_check(fn, e, TAKES_BOTH, coils, sens_n, map_n)) return rc;
    PNP_ON_DEVICE(e);
    if (int rc = op_ensure(e, TAKES_BOTH, coils)) return rc;
    return om_forward(e, (const float2*)img, nullptr, (const float2*)maps, map_n, (const float2*)sens, sens_n, coils, batch, (float2*)samples,
                      (hipStream_t)stream);
    PNP_API_END("pnp_offres_forward_mc")
}

int pnp_offres_adjoint_mc(pnp_handle e, const float* samples, const float* weights, const float* maps, int map_n, const float* sens, int sens_n,
                          int coils, int batch, float* img, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_offres_adjoint_mc";
    if (int rc = op_check_scalars(fn, TAKES_BOTH, coils, sens_n, map_n)) return rc;
    if (batch < 1) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n (got %d)", fn, batch);
    if (!samples) return fail(PNP_ERR_INVALID, "%s: null samples", fn);
    if (!maps) return fail(PNP_ERR_INVALID, "%s: null maps", fn);
    if (!sens) return fail(PNP_ERR_INVALID, "%s: null sens", fn);
    if (!img) return fail(PNP_ERR_INVALID, "%s: null img", fn);
    if (img == samples || img == maps || img == sens || (const float*)img == weights)
        return fail(PNP_ERR_INVALID, "%s: img must not alias samples, weights, maps or sens", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (batch > e->cfg.n) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n=%d (got %d)", fn, e->cfg.n, batch);
    if (int rc = op_check(fn, e, TAKES_BOTH, coils, sens_n, map_n)) return rc;
    PNP_ON_DEVICE(e);
    if (int rc = op_ensure(e, TAKES_BOTH, coils)) return rc;
    return om_adjoint(e, (const float2*)samples, weights, (const float2*)maps, map_n, (const float2*)sens, sens_n, coils, batch, (float2*)img,
                      (hipStream_t)stream);
    PNP_API_END("pnp_offres_adjoint_mc")
}

int pnp_set_kspace_offres_mc(pnp_handle e, const float* y, const float* sens, int coils, int sens_n, const float* omega, int map_n, const float* w,
                             int cg_iters, void* stream) {
    PNP_API_BEGIN
    return nc_install("pnp_set_kspace_offres_mc", e, TAKES_BOTH, false, false, nullptr, (const float2*)y, (const float2*)sens, coils, sens_n, omega,
                      map_n, w, cg_iters, nullptr, nullptr, nullptr, (hipStream_t)stream);
    PNP_API_END("pnp_set_kspace_offres_mc")
}

int pnp_reset_offres_mc(pnp_handle e, const float* x0, const float* y, const float* sens, int coils, int sens_n, const float* omega, int map_n,
                        const float* w, int cg_iters, float* x, float* z, float* u, void* stream) {
    PNP_API_BEGIN
    return nc_install("pnp_reset_offres_mc", e, TAKES_BOTH, true, false, (const float2*)x0, (const float2*)y, (const float2*)sens, coils, sens_n,
                      omega, map_n, w, cg_iters, x, (float2*)z, (float2*)u, (hipStream_t)stream);
    PNP_API_END("pnp_reset_offres_mc")
}

int pnp_offres_mc_coils(pnp_handle e) { return e && e->stage.kind == STAGE_ORS ? e->stage.coils : 0; }

int pnp_offres_mc_cg_residual(pnp_handle e, float* out, void* stream) {
    PNP_API_BEGIN
    return stage_cg_residual("pnp_offres_mc_cg_residual", e, STAGE_ORS, out, (hipStream_t)stream);
    PNP_API_END("pnp_offres_mc_cg_residual")
}

int pnp_offres_mc_normal(pnp_handle e, const float* pv, const float* mu, float* q, void* stream) {
    PNP_API_BEGIN
    return stage_normal_op("pnp_offres_mc_normal", e, STAGE_ORS, pv, mu, q, (hipStream_t)stream);
    PNP_API_END("pnp_offres_mc_normal")
}

int pnp_acquire_offres_mc(pnp_handle e, const float* gt, const float* sens, int coils, int sens_n, const float* omega, int map_n, const float* dcf,
                          double sigma_n, uint64_t seed, int flags, float* y, float* aty0, float* x0, void* stream) {
    PNP_API_BEGIN
    return nc_acquire("pnp_acquire_offres_mc", e, TAKES_BOTH, gt, sens, coils, sens_n, omega, map_n, dcf, sigma_n, seed, flags, y, aty0, x0,
                      (hipStream_t)stream);
    PNP_API_END("pnp_acquire_offres_mc")
}

// ---- Toeplitz normal operator (include/pnpadmm_toeplitz.h) ----------------------------------------------
static_assert(2 * PNP_TOEPLITZ_MAX_SIDE == 1024, "the padded grid's sides are sides of the k-space stage");

namespace {

int tz_check_sizes(const char* fn, const pnp_engine* e) {
    if (e->cfg.h <= PNP_TOEPLITZ_MAX_SIDE && e->cfg.w <= PNP_TOEPLITZ_MAX_SIDE)
        return kspace_len_ok(2 * e->cfg.h) && kspace_len_ok(2 * e->cfg.w)
                   ? PNP_OK
                   : fail(PNP_ERR_INVALID, "%s: 2h and 2w must be sides of the k-space stage {" PNP_KSPACE_SIZES "} (got %dx%d)", fn, e->cfg.h, e->cfg.w);
    return fail(PNP_ERR_INVALID, "%s: the Toeplitz operator transforms a 2h x 2w grid, so it takes h, w up to %d (got %dx%d)", fn,
                PNP_TOEPLITZ_MAX_SIDE, e->cfg.h, e->cfg.w);
}

}  // namespace

int pnp_toeplitz_plan(pnp_handle e, const float* weights, int flags, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_toeplitz_plan";
    if (flags != 0) return fail(PNP_ERR_INVALID, "%s: flags must be 0 (got 0x%x)", fn, (unsigned)flags);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (int rc = nc_need_plan(fn, e)) return rc;
    if (int rc = tz_check_sizes(fn, e)) return rc;
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w;
    const size_t M = (size_t)e->nc.m;
    const std::vector<float2> twh = twiddle_table(2 * H), tww = twiddle_table(2 * W);
    PNP_ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ws_grow(e, "Toeplitz spectrum", {{(void**)&e->tz_k, &e->tz_k_cap, (size_t)4 * H * W * sizeof(float), false},
                                                  {(void**)&e->tz_w, &e->tz_w_cap, weights ? M * sizeof(float) : 0, false},
                                                  {(void**)&e->tz_traj, &e->tz_traj_cap, M * 2 * sizeof(double), false},
                                                  {(void**)&e->tz_tw_h, &e->tz_twh_cap, twh.size() * sizeof(float2), false},
                                                  {(void**)&e->tz_tw_w, &e->tz_tww_cap, tww.size() * sizeof(float2), false},
                                                  {(void**)&e->tz_grid, &e->tz_grid_cap, (size_t)N * (e->tz_fused ? 2 : 4) * H * W * sizeof(float2), false}}))
        return rc;
    if (e->tz_planned) (void)hipDeviceSynchronize();        // no launch still reads the spectrum being replaced
    // from here on the old spectrum is gone: a live Toeplitz stage's constants are dropped with it, as pnp_nufft_plan drops them
    e->tz_planned = false;
    drop_stage(e, DROP_FORM, FORM_TZ);
    HIP_TRY(nc_upload(e->tz_traj, e->nc_traj.data(), M * 2 * sizeof(double)));
    HIP_TRY(nc_upload(e->tz_tw_h, twh.data(), twh.size() * sizeof(float2)));
    HIP_TRY(nc_upload(e->tz_tw_w, tww.data(), tww.size() * sizeof(float2)));
    if (weights) HIP_TRY(hipMemcpyAsync(e->tz_w, weights, M * sizeof(float), hipMemcpyDeviceToDevice, s));
    {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_toeplitz_spectrum(e->tz_traj, weights ? e->tz_w : nullptr, e->nc.m, H, W, e->tz_k, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    e->tz_has_w = weights != nullptr;
    e->tz_planned = true;
    return PNP_OK;
    PNP_API_END("pnp_toeplitz_plan")
}

int pnp_toeplitz_planned(pnp_handle e) { return e && e->tz_planned ? 1 : 0; }
int pnp_toeplitz_live(pnp_handle e) { return e && e->stage.form == FORM_TZ ? 1 : 0; }

int pnp_toeplitz_spectrum(pnp_handle e, float* out, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_toeplitz_spectrum";
    if (!out) return fail(PNP_ERR_INVALID, "%s: null out", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (int rc = tz_need_spectrum(fn, e)) return rc;
    PNP_ON_DEVICE(e);
    HIP_TRY(hipMemcpyAsync(out, e->tz_k, (size_t)4 * e->cfg.h * e->cfg.w * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PNP_OK;
    PNP_API_END("pnp_toeplitz_spectrum")
}

int pnp_toeplitz_apply(pnp_handle e, const float* img, int batch, float* out, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_toeplitz_apply";
    if (batch < 1) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n (got %d)", fn, batch);
    if (!img) return fail(PNP_ERR_INVALID, "%s: null img", fn);
    if (!out) return fail(PNP_ERR_INVALID, "%s: null out", fn);
    if (img == out) return fail(PNP_ERR_INVALID, "%s: out must not alias img", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (batch > e->cfg.n) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n=%d (got %d)", fn, e->cfg.n, batch);
    if (int rc = tz_need_spectrum(fn, e)) return rc;
    PNP_ON_DEVICE(e);
    return tz_apply(e, (const float2*)img, batch, nullptr, nullptr, nullptr, (float2*)out, nullptr, (hipStream_t)stream);
    PNP_API_END("pnp_toeplitz_apply")
}

int pnp_toeplitz_apply_mc(pnp_handle e, const float* img, const float* sens, int coils, int sens_n, int batch, float* out, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_toeplitz_apply_mc";
    if (int rc = op_check_scalars(fn, TAKES_COILS, coils, sens_n, 0)) return rc;
    if (batch < 1) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n (got %d)", fn, batch);
    if (!img) return fail(PNP_ERR_INVALID, "%s: null img", fn);
    if (!sens) return fail(PNP_ERR_INVALID, "%s: null sens", fn);
    if (!out) return fail(PNP_ERR_INVALID, "%s: null out", fn);
    if (out == img || out == sens) return fail(PNP_ERR_INVALID, "%s: out must not alias img or sens", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (batch > e->cfg.n) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n=%d (got %d)", fn, e->cfg.n, batch);
    if (int rc = op_check(fn, e, TAKES_COILS, coils, sens_n, 0)) return rc;
    if (int rc = tz_need_spectrum(fn, e)) return rc;
    PNP_ON_DEVICE(e);
    if (int rc = tz_ensure(e, (size_t)e->cfg.n * ns_block_of(e, coils), true)) return rc;
    return tz_apply_mc(e, (const float2*)img, (const float2*)sens, sens_n, coils, batch, nullptr, nullptr, nullptr, (float2*)out, nullptr,
                       (hipStream_t)stream);
    PNP_API_END("pnp_toeplitz_apply_mc")
}

int pnp_set_kspace_nc_tz(pnp_handle e, const float* y, int cg_iters, void* stream) {
    PNP_API_BEGIN
    return nc_install("pnp_set_kspace_nc_tz", e, 0, false, true, nullptr, (const float2*)y, nullptr, 0, 1, nullptr, 1, nullptr, cg_iters, nullptr,
                      nullptr, nullptr, (hipStream_t)stream);
    PNP_API_END("pnp_set_kspace_nc_tz")
}

int pnp_reset_nc_tz(pnp_handle e, const float* x0, const float* y, int cg_iters, float* x, float* z, float* u, void* stream) {
    PNP_API_BEGIN
    return nc_install("pnp_reset_nc_tz", e, 0, true, true, (const float2*)x0, (const float2*)y, nullptr, 0, 1, nullptr, 1, nullptr, cg_iters, x,
                      (float2*)z, (float2*)u, (hipStream_t)stream);
    PNP_API_END("pnp_reset_nc_tz")
}

int pnp_set_kspace_ncsense_tz(pnp_handle e, const float* y, const float* sens, int coils, int sens_n, int cg_iters, void* stream) {
    PNP_API_BEGIN
    return nc_install("pnp_set_kspace_ncsense_tz", e, TAKES_COILS, false, true, nullptr, (const float2*)y, (const float2*)sens, coils, sens_n,
                      nullptr, 1, nullptr, cg_iters, nullptr, nullptr, nullptr, (hipStream_t)stream);
    PNP_API_END("pnp_set_kspace_ncsense_tz")
}

int pnp_reset_ncsense_tz(pnp_handle e, const float* x0, const float* y, const float* sens, int coils, int sens_n, int cg_iters, float* x, float* z,
                         float* u, void* stream) {
    PNP_API_BEGIN
    return nc_install("pnp_reset_ncsense_tz", e, TAKES_COILS, true, true, (const float2*)x0, (const float2*)y, (const float2*)sens, coils, sens_n,
                      nullptr, 1, nullptr, cg_iters, x, (float2*)z, (float2*)u, (hipStream_t)stream);
    PNP_API_END("pnp_reset_ncsense_tz")
}

// ---- Toeplitz form of the off-resonance operator (include/pnpadmm_offres_tz.h) ------------------------------
static_assert(PNP_OFFRES_TZ_MAX_PAIRS == kOffresTzMaxPairs && PNP_OFFRES_TZ_PLANES == kOffresTzPlanes, "the header's limits are the plan's");

int pnp_offres_tz_plan(pnp_handle e, const float* weights, int flags, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_offres_tz_plan";
    // every rejection happens before any HIP call and leaves the handle as it was
    if (flags != 0) return fail(PNP_ERR_INVALID, "%s: flags must be 0 (got 0x%x)", fn, (unsigned)flags);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (int rc = or_need_plan(fn, e)) return rc;
    if (int rc = tz_check_sizes(fn, e)) return rc;
    OffresTzPlan P;
    std::string why;
    if (!plan_offres_tz(e->orp.kind, e->orp.segments, e->nc.m, e->orp.kind == 1 ? e->or_seg_h.data() : nullptr, &P, &why))
        return fail(PNP_ERR_INVALID, "%s: %s", fn, why.c_str());
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w;
    const size_t M = (size_t)e->nc.m, hw = (size_t)H * W, planes = (size_t)otz_slice_block(e, N) * e->orp.segments;
    const std::vector<float2> twh = twiddle_table(2 * H), tww = twiddle_table(2 * W);
    PNP_ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ws_grow(e, "Toeplitz off-resonance spectra",
                         {{(void**)&e->otz_k, &e->otz_k_cap, (size_t)P.pairs * 4 * hw * sizeof(float), false},
                          {(void**)&e->otz_w, &e->otz_w_cap, weights ? M * sizeof(float) : 0, false},
                          {(void**)&e->otz_traj, &e->otz_traj_cap, M * 2 * sizeof(double), false},
                          {(void**)&e->otz_tw_h, &e->otz_twh_cap, twh.size() * sizeof(float2), false},
                          {(void**)&e->otz_tw_w, &e->otz_tww_cap, tww.size() * sizeof(float2), false},
                          {(void**)&e->otz.blk_off, &e->otz_off_cap, P.blk_off.size() * sizeof(int32_t), false},
                          {(void**)&e->otz.blk_idx, &e->otz_idx_cap, P.blk_idx.size() * sizeof(int32_t), false},
                          {(void**)&e->otz_img, &e->otz_img_cap, planes * hw * sizeof(float2), false},
                          {(void**)&e->otz_x, &e->otz_x_cap, planes * 4 * hw * sizeof(float2), false},
                          {(void**)&e->otz_y, &e->otz_y_cap, planes * 4 * hw * sizeof(float2), false}}))
        return rc;
    if (e->otz_planned) (void)hipDeviceSynchronize();       // no launch still reads the spectra being replaced
    // from here on the old spectra are gone: a live stage that runs on them loses its constants, as pnp_offres_plan drops them
    e->otz_planned = false;
    e->otz.pairs = 0;
    drop_stage(e, DROP_FORM, FORM_OTZ);
    HIP_TRY(nc_upload(e->otz_traj, e->nc_traj.data(), M * 2 * sizeof(double)));
    HIP_TRY(nc_upload(e->otz_tw_h, twh.data(), twh.size() * sizeof(float2)));
    HIP_TRY(nc_upload(e->otz_tw_w, tww.data(), tww.size() * sizeof(float2)));
    if (!P.blk_off.empty()) HIP_TRY(nc_upload(e->otz.blk_off, P.blk_off.data(), P.blk_off.size() * sizeof(int32_t)));
    if (!P.blk_idx.empty()) HIP_TRY(nc_upload(e->otz.blk_idx, P.blk_idx.data(), P.blk_idx.size() * sizeof(int32_t)));
    if (weights) HIP_TRY(hipMemcpyAsync(e->otz_w, weights, M * sizeof(float), hipMemcpyDeviceToDevice, s));
    OffresTzDev T = e->otz;                                 // a least-squares plan has no lists: its workgroups walk every sample
    T.pairs = P.pairs; T.pair_block = P.pair_block; T.blocks = P.blocks;
    if (P.blk_off.empty()) { T.blk_off = nullptr; T.blk_idx = nullptr; }
    {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_offres_tz_spectra(e->otz_traj, weights ? e->otz_w : nullptr, e->orp, T, e->nc.m, H, W, e->otz_k, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    e->otz.pairs = P.pairs; e->otz.pair_block = P.pair_block; e->otz.blocks = P.blocks;
    e->otz_has_w = weights != nullptr;
    e->otz_planned = true;
    return PNP_OK;
    PNP_API_END("pnp_offres_tz_plan")
}

int pnp_offres_tz_planned(pnp_handle e) { return e && e->otz_planned ? 1 : 0; }
int pnp_offres_tz_live(pnp_handle e) { return e && e->stage.form == FORM_OTZ ? 1 : 0; }
int pnp_offres_tz_spectra(pnp_handle e) { return e && e->otz_planned ? e->otz.pairs : 0; }

int pnp_offres_tz_spectrum(pnp_handle e, float* out, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_offres_tz_spectrum";
    if (!out) return fail(PNP_ERR_INVALID, "%s: null out", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (int rc = otz_need_spectra(fn, e)) return rc;
    PNP_ON_DEVICE(e);
    HIP_TRY(hipMemcpyAsync(out, e->otz_k, (size_t)e->otz.pairs * 4 * e->cfg.h * e->cfg.w * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PNP_OK;
    PNP_API_END("pnp_offres_tz_spectrum")
}

int pnp_offres_tz_apply(pnp_handle e, const float* img, const float* maps, int map_n, int batch, float* out, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_offres_tz_apply";
    if (int rc = op_check_scalars(fn, TAKES_MAPS, 0, 0, map_n)) return rc;
    if (batch < 1) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n (got %d)", fn, batch);
    if (!img) return fail(PNP_ERR_INVALID, "%s: null img", fn);
    if (!maps) return fail(PNP_ERR_INVALID, "%s: null maps", fn);
    if (!out) return fail(PNP_ERR_INVALID, "%s: null out", fn);
    if (out == img || out == maps) return fail(PNP_ERR_INVALID, "%s: out must not alias img or maps", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (batch > e->cfg.n) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n=%d (got %d)", fn, e->cfg.n, batch);
    if (int rc = op_check(fn, e, TAKES_MAPS, 0, 0, map_n)) return rc;
    if (int rc = otz_need_spectra(fn, e)) return rc;
    PNP_ON_DEVICE(e);
    if (int rc = otz_ensure(e, e->cfg.n, 0)) return rc;
    return otz_apply(e, (const float2*)img, (const float2*)maps, map_n, batch, nullptr, nullptr, nullptr, (float2*)out, nullptr, (hipStream_t)stream);
    PNP_API_END("pnp_offres_tz_apply")
}

int pnp_offres_tz_apply_mc(pnp_handle e, const float* img, const float* maps, int map_n, const float* sens, int sens_n, int coils, int batch,
                           float* out, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_offres_tz_apply_mc";
    if (int rc = op_check_scalars(fn, TAKES_BOTH, coils, sens_n, map_n)) return rc;
    if (batch < 1) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n (got %d)", fn, batch);
    if (!img) return fail(PNP_ERR_INVALID, "%s: null img", fn);
    if (!maps) return fail(PNP_ERR_INVALID, "%s: null maps", fn);
    if (!sens) return fail(PNP_ERR_INVALID, "%s: null sens", fn);
    if (!out) return fail(PNP_ERR_INVALID, "%s: null out", fn);
    if (out == img || out == maps || out == sens) return fail(PNP_ERR_INVALID, "%s: out must not alias img, maps or sens", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (batch > e->cfg.n) return fail(PNP_ERR_INVALID, "%s: batch must be 1..n=%d (got %d)", fn, e->cfg.n, batch);
    if (int rc = op_check(fn, e, TAKES_BOTH, coils, sens_n, map_n)) return rc;
    if (int rc = otz_need_spectra(fn, e)) return rc;
    PNP_ON_DEVICE(e);
    const int cb = otz_coil_block(e, coils, map_n);
    if (int rc = otz_ensure(e, e->cfg.n * cb, (size_t)e->cfg.n * cb)) return rc;
    return otz_apply_mc(e, (const float2*)img, (const float2*)maps, map_n, (const float2*)sens, sens_n, coils, batch, nullptr, nullptr, nullptr,
                        (float2*)out, nullptr, (hipStream_t)stream);
    PNP_API_END("pnp_offres_tz_apply_mc")
}

int pnp_set_kspace_offres_tz(pnp_handle e, const float* y, const float* omega, int map_n, int cg_iters, void* stream) {
    PNP_API_BEGIN
    return nc_install("pnp_set_kspace_offres_tz", e, TAKES_MAPS, false, true, nullptr, (const float2*)y, nullptr, 0, 1, omega, map_n, nullptr,
                      cg_iters, nullptr, nullptr, nullptr, (hipStream_t)stream);
    PNP_API_END("pnp_set_kspace_offres_tz")
}

int pnp_reset_offres_tz(pnp_handle e, const float* x0, const float* y, const float* omega, int map_n, int cg_iters, float* x, float* z, float* u,
                        void* stream) {
    PNP_API_BEGIN
    return nc_install("pnp_reset_offres_tz", e, TAKES_MAPS, true, true, (const float2*)x0, (const float2*)y, nullptr, 0, 1, omega, map_n, nullptr,
                      cg_iters, x, (float2*)z, (float2*)u, (hipStream_t)stream);
    PNP_API_END("pnp_reset_offres_tz")
}

int pnp_set_kspace_offres_mc_tz(pnp_handle e, const float* y, const float* sens, int coils, int sens_n, const float* omega, int map_n, int cg_iters,
                                void* stream) {
    PNP_API_BEGIN
    return nc_install("pnp_set_kspace_offres_mc_tz", e, TAKES_BOTH, false, true, nullptr, (const float2*)y, (const float2*)sens, coils, sens_n,
                      omega, map_n, nullptr, cg_iters, nullptr, nullptr, nullptr, (hipStream_t)stream);
    PNP_API_END("pnp_set_kspace_offres_mc_tz")
}

int pnp_reset_offres_mc_tz(pnp_handle e, const float* x0, const float* y, const float* sens, int coils, int sens_n, const float* omega, int map_n,
                           int cg_iters, float* x, float* z, float* u, void* stream) {
    PNP_API_BEGIN
    return nc_install("pnp_reset_offres_mc_tz", e, TAKES_BOTH, true, true, (const float2*)x0, (const float2*)y, (const float2*)sens, coils, sens_n,
                      omega, map_n, nullptr, cg_iters, x, (float2*)z, (float2*)u, (hipStream_t)stream);
    PNP_API_END("pnp_reset_offres_mc_tz")
}

// ---- density compensation (include/pnpadmm_dcf.h) -------------------------------------------------------
namespace {

int dcf_need_plan(const char* fn, const pnp_engine* e) {
    return e->nc.m > 0 ? PNP_OK : fail(PNP_ERR_INVALID, "%s: the handle has no NUFFT plan (pnp_nufft_plan)", fn);
}
// the feature's own workspace: the grid, the float64 weights, the chunk sums and, for `passes` > 0, that many rows of workgroup maxima
int dcf_ensure(pnp_engine* e, int passes) {
    const size_t M = (size_t)e->nc.m;
    return ws_grow(e, "density compensation workspace",
                   {{(void**)&e->dcf_grid, &e->dcf_grid_cap, (size_t)e->nc.gh * e->nc.gw * sizeof(double), false},
                    {(void**)&e->dcf_w, &e->dcf_w_cap, M * sizeof(double), false},
                    {(void**)&e->dcf_part, &e->dcf_part_cap, (size_t)dcf_sum_chunks(e->nc.m) * sizeof(double), false},
                    {(void**)&e->dcf_max, &e->dcf_max_cap, (size_t)passes * dcf_gather_blocks(e->nc.m) * sizeof(float), false}});
}

}  // namespace

int pnp_nufft_psi(pnp_handle e, const float* w, float* out, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_nufft_psi";
    if (!w) return fail(PNP_ERR_INVALID, "%s: null w", fn);
    if (!out) return fail(PNP_ERR_INVALID, "%s: null out", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (int rc = dcf_need_plan(fn, e)) return rc;
    PNP_ON_DEVICE(e);
    if (int rc = dcf_ensure(e, 0)) return rc;
    hipStream_t s = (hipStream_t)stream;
    Prof p(e, s, PROF_OTHER, -1);
    HIP_TRY(launch_dcf_spread(nullptr, w, e->nc, e->dcf_grid, s));
    HIP_TRY(launch_dcf_gather(e->dcf_grid, e->nc, nullptr, nullptr, nullptr, out, nullptr, s));
    p.end(2);
    return PNP_OK;
    PNP_API_END("pnp_nufft_psi")
}

int pnp_nufft_dcf(pnp_handle e, const float* w0, int iters, int flags, float* w, float* info, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_nufft_dcf";
    if (iters < 1 || iters > PNP_DCF_MAX_ITERS) return fail(PNP_ERR_INVALID, "%s: iters must be 1..%d (got %d)", fn, PNP_DCF_MAX_ITERS, iters);
    if (flags != 0) return fail(PNP_ERR_INVALID, "%s: flags must be 0 (got 0x%x)", fn, (unsigned)flags);
    if (!w) return fail(PNP_ERR_INVALID, "%s: null w", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if (int rc = dcf_need_plan(fn, e)) return rc;
    PNP_ON_DEVICE(e);
    if (int rc = dcf_ensure(e, info ? iters + 1 : 0)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t nb = (size_t)dcf_gather_blocks(e->nc.m);
    Prof p(e, s, PROF_OTHER, -1);
    for (int k = 0; k < iters; ++k) {
        const double* w64 = k ? e->dcf_w : nullptr;         // the first pass reads the caller's start (or ones)
        const float* w32 = k ? nullptr : w0;
        HIP_TRY(launch_dcf_spread(w64, w32, e->nc, e->dcf_grid, s));
        HIP_TRY(launch_dcf_gather(e->dcf_grid, e->nc, w64, w32, e->dcf_w, nullptr, info ? e->dcf_max + k * nb : nullptr, s));
    }
    if (info) {                                             // max |Psi w - 1| of the result: one more spread and gather
        HIP_TRY(launch_dcf_spread(e->dcf_w, nullptr, e->nc, e->dcf_grid, s));
        HIP_TRY(launch_dcf_gather(e->dcf_grid, e->nc, nullptr, nullptr, nullptr, nullptr, e->dcf_max + (size_t)iters * nb, s));
    }
    HIP_TRY(launch_dcf_finish(e->dcf_w, e->dcf_part, e->nc, w, e->dcf_max, iters + 1, info, s));
    p.end(2 * iters + (info ? 2 : 0) + 2);
    return PNP_OK;
    PNP_API_END("pnp_nufft_dcf")
}

// ---- field map estimation (include/pnpadmm_fieldmap.h) --------------------------------------------------
namespace {

static_assert(PNP_FIELDMAP_T == kFmT, "the header's sweeps per launch are the kernels'");

// the feature's own workspace, never replaced: the five planes and the workgroup maxima in one buffer, the cost's chunk sums in another
int fm_ensure(pnp_engine* e) {
    const size_t px = (size_t)e->cfg.n * e->cfg.h * e->cfg.w, chunks = (size_t)e->cfg.n * pixel_chunks(e->cfg.h, e->cfg.w);
    return ws_grow(e, "field map workspace", {{(void**)&e->fm_ws, nullptr, e->fm_ws ? 0 : (5 * px + chunks) * sizeof(float), false},
                                              {(void**)&e->fm_part, nullptr, e->fm_part ? 0 : chunks * sizeof(double), false}});
}

// every argument error of the two entry points, before any HIP call
int fm_check(const char* fn, const pnp_engine* e, const float* x1, const float* x2, int coils, double dte, float beta, bool omega_in,
             const float* omega, const void* out, const char* out_name) {
    if (coils < 1 || coils > PNP_MC_MAX_COILS) return fail(PNP_ERR_INVALID, "%s: coils must be 1..%d (got %d)", fn, PNP_MC_MAX_COILS, coils);
    if (!(dte > 0.0) || !std::isfinite(dte)) return fail(PNP_ERR_INVALID, "%s: dte must be finite and > 0 (got %g)", fn, dte);
    if (!(beta > 0.0f) || !std::isfinite(beta)) return fail(PNP_ERR_INVALID, "%s: beta must be finite and > 0 (got %g)", fn, (double)beta);
    if (!x1) return fail(PNP_ERR_INVALID, "%s: null x1", fn);
    if (!x2) return fail(PNP_ERR_INVALID, "%s: null x2", fn);
    if (omega_in && !omega) return fail(PNP_ERR_INVALID, "%s: null omega", fn);
    if (!out) return fail(PNP_ERR_INVALID, "%s: null %s", fn, out_name);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    if ((long long)e->cfg.n > 65535) return fail(PNP_ERR_INVALID, "%s: n must be <= 65535 (got %d)", fn, e->cfg.n);
    return PNP_OK;
}

// the planes of the workspace, and phi, w, rd, theta^0 of (x1, x2) in them: two launches
int fm_prepare(pnp_engine* e, FmArgs& a, float* (&th)[2], const float* x1, const float* x2, int coils, double dte, float beta, float* weight,
               hipStream_t s) {
    const size_t px = (size_t)e->cfg.n * e->cfg.h * e->cfg.w;
    a.x1 = (const float2*)x1; a.x2 = (const float2*)x2; a.C = coils; a.dte = dte; a.beta = beta; a.H = e->cfg.h; a.W = e->cfg.w;
    a.phi = e->fm_ws; a.w = e->fm_ws + px; a.rd = e->fm_ws + 2 * px;
    th[0] = e->fm_ws + 3 * px; th[1] = e->fm_ws + 4 * px;
    a.maxpart = e->fm_ws + 5 * px;
    a.part = e->fm_part;
    a.weight = weight;
    a.th_out = th[0];
    HIP_TRY(launch_fm_prepare(a, e->cfg.n, s));
    return PNP_OK;
}

}  // namespace

int pnp_fieldmap_estimate(pnp_handle e, const float* x1, const float* x2, int coils, double dte, float beta, int iters, int flags, float* omega,
                          float* weight, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_fieldmap_estimate";
    if (iters < 0 || iters > PNP_FIELDMAP_MAX_ITERS) return fail(PNP_ERR_INVALID, "%s: iters must be 0..%d (got %d)", fn, PNP_FIELDMAP_MAX_ITERS, iters);
    if (flags != 0) return fail(PNP_ERR_INVALID, "%s: flags must be 0 (got 0x%x)", fn, (unsigned)flags);
    if (int rc = fm_check(fn, e, x1, x2, coils, dte, beta, false, nullptr, omega, "omega")) return rc;
    PNP_ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    const int N = e->cfg.n;
    FmArgs a{};
    float* th[2];
    if (int rc = fm_ensure(e)) return rc;
    Prof p(e, s, PROF_OTHER, -1);
    if (int rc = fm_prepare(e, a, th, x1, x2, coils, dte, beta, weight, s)) return rc;
    const bool naive = e->tune.fieldmap_naive;
    const int L = naive ? iters : (iters + kFmT - 1) / kFmT;
    for (int l = 0; l < L; ++l) {                            // theta ping-pongs through the two planes; no launch writes the plane it reads
        a.th_in = th[l & 1];
        a.th_out = th[(l + 1) & 1];
        if (naive) { HIP_TRY(launch_fm_sweep(a, N, s)); continue; }
        a.iters = iters - l * kFmT < kFmT ? iters - l * kFmT : kFmT;
        HIP_TRY(launch_fm_fused(a, N, s));
    }
    a.th_in = th[L & 1];
    a.omega_out = omega;
    HIP_TRY(launch_fm_finish(a, N, s));
    p.end(L + 3);
    return PNP_OK;
    PNP_API_END("pnp_fieldmap_estimate")
}

int pnp_fieldmap_cost(pnp_handle e, const float* x1, const float* x2, int coils, double dte, float beta, const float* omega, double* cost,
                      void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_fieldmap_cost";
    if (int rc = fm_check(fn, e, x1, x2, coils, dte, beta, true, omega, cost, "cost")) return rc;
    PNP_ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    FmArgs a{};
    float* th[2];
    if (int rc = fm_ensure(e)) return rc;
    Prof p(e, s, PROF_OTHER, -1);
    if (int rc = fm_prepare(e, a, th, x1, x2, coils, dte, beta, nullptr, s)) return rc;
    a.omega_in = omega;
    a.cost = cost;
    HIP_TRY(launch_fm_cost(a, e->cfg.n, s));
    p.end(4);
    return PNP_OK;
    PNP_API_END("pnp_fieldmap_cost")
}

int pnp_estimate_sens(pnp_handle e, const float* y0, int coils, int acs_h, int acs_w, int window, double thresh, int flags, float* sens,
                      float* rss, void* stream) {
    PNP_API_BEGIN
    // every rejection happens before any HIP call, and leaves the outputs untouched; scalar ranges first
    if (flags != 0) return fail(PNP_ERR_INVALID, "pnp_estimate_sens: flags must be 0 (got 0x%x)", (unsigned)flags);
    if (!(thresh >= 0.0) || !(thresh < 1.0)) return fail(PNP_ERR_INVALID, "pnp_estimate_sens: thresh must be finite and in [0, 1) (got %g)", thresh);
    if (window != PNP_SENS_BOX && window != PNP_SENS_HANN)
        return fail(PNP_ERR_INVALID, "pnp_estimate_sens: window must be PNP_SENS_BOX or PNP_SENS_HANN (got %d)", window);
    if (coils < 1 || coils > PNP_MC_MAX_COILS) return fail(PNP_ERR_INVALID, "pnp_estimate_sens: coils must be 1..%d (got %d)", PNP_MC_MAX_COILS, coils);
    if (acs_h < 2 || (acs_h & 1)) return fail(PNP_ERR_INVALID, "pnp_estimate_sens: acs_h must be even and >= 2 (got %d)", acs_h);
    if (acs_w < 2 || (acs_w & 1)) return fail(PNP_ERR_INVALID, "pnp_estimate_sens: acs_w must be even and >= 2 (got %d)", acs_w);
    if (!y0) return fail(PNP_ERR_INVALID, "pnp_estimate_sens: null y0");
    if (!sens) return fail(PNP_ERR_INVALID, "pnp_estimate_sens: null sens");
    if (sens == y0) return fail(PNP_ERR_INVALID, "pnp_estimate_sens: sens must not alias y0");
    if (!e) return fail(PNP_ERR_INVALID, "pnp_estimate_sens: null handle");
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w;
    if (acs_h > H) return fail(PNP_ERR_INVALID, "pnp_estimate_sens: acs_h must be <= h=%d (got %d)", H, acs_h);
    if (acs_w > W) return fail(PNP_ERR_INVALID, "pnp_estimate_sens: acs_w must be <= w=%d (got %d)", W, acs_w);
    if (int rc = check_kspace_sizes("pnp_estimate_sens", e)) return rc;
    if ((long long)N * coils > 65535) return fail(PNP_ERR_INVALID, "pnp_estimate_sens: n * coils must be <= 65535 (got %d * %d)", N, coils);
    PNP_ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = cm_ensure(e, rss == nullptr))) return rc;
    float* const r = rss ? rss : e->cm_rss;
    float* const smax = e->cm_max + (size_t)N * pixel_chunks(H, W);
    {
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_coilmap_window((const float2*)y0, (float2*)sens, acs_h, acs_w, window == PNP_SENS_HANN, N, coils, H, W, s));
    }
    // l_c = the plain inverse transform of the windowed, sign-folded block, in place in the caller's buffer
    if ((rc = plain_fft2(e, (float2*)sens, (float2*)sens, N * coils, 1, s))) return rc;
    Prof p(e, s, PROF_OTHER, -1);
    HIP_TRY(launch_coilmap_rss((const float2*)sens, coils, r, e->cm_max, N, H, W, s));
    HIP_TRY(launch_coilmap_max(e->cm_max, smax, N, H, W, s));
    HIP_TRY(launch_coilmap_normalise((float2*)sens, coils, r, smax, (float)thresh, N, H, W, s));
    p.end(3);
    return PNP_OK;
    PNP_API_END("pnp_estimate_sens")
}

int pnp_coil_compress_matrix(pnp_handle e, const float* y0, int coils, int acs_h, int acs_w, int flags, float* cmat, float* eig, double* gram,
                             void* stream) {
    PNP_API_BEGIN
    // every rejection happens before any HIP call, and leaves the outputs untouched; scalar ranges first
    const char* fn = "pnp_coil_compress_matrix";
    if (flags != 0) return fail(PNP_ERR_INVALID, "%s: flags must be 0 (got 0x%x)", fn, (unsigned)flags);
    if (coils < 1 || coils > PNP_CC_MAX_COILS) return fail(PNP_ERR_INVALID, "%s: coils must be 1..%d (got %d)", fn, PNP_CC_MAX_COILS, coils);
    if (acs_h < 2 || (acs_h & 1)) return fail(PNP_ERR_INVALID, "%s: acs_h must be even and >= 2 (got %d)", fn, acs_h);
    if (acs_w < 2 || (acs_w & 1)) return fail(PNP_ERR_INVALID, "%s: acs_w must be even and >= 2 (got %d)", fn, acs_w);
    if (!y0) return fail(PNP_ERR_INVALID, "%s: null y0", fn);
    if (!cmat) return fail(PNP_ERR_INVALID, "%s: null cmat", fn);
    if (!eig) return fail(PNP_ERR_INVALID, "%s: null eig", fn);
    if ((const void*)cmat == (const void*)y0 || (const void*)eig == (const void*)y0 || (const void*)gram == (const void*)y0 ||
        (const void*)cmat == (const void*)eig || (const void*)gram == (const void*)cmat || (const void*)gram == (const void*)eig)
        return fail(PNP_ERR_INVALID, "%s: y0, cmat, eig and gram must not alias", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w;
    if (acs_h > H) return fail(PNP_ERR_INVALID, "%s: acs_h must be <= h=%d (got %d)", fn, H, acs_h);
    if (acs_w > W) return fail(PNP_ERR_INVALID, "%s: acs_w must be <= w=%d (got %d)", fn, W, acs_w);
    if (N > 65535) return fail(PNP_ERR_INVALID, "%s: n must be <= 65535 (got %d)", fn, N);
    PNP_ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t cc = (size_t)coils * coils;
    if (int rc = cc_ensure(e, (size_t)N * gram_chunks(acs_h * acs_w) * cc, gram ? 0 : (size_t)N * cc)) return rc;
    double2* const g = gram ? (double2*)gram : e->cc_gram;
    Prof p(e, s, PROF_OTHER, -1);
    HIP_TRY(launch_coilcomp_gram((const float2*)y0, coils, acs_h, acs_w, e->cc_part, g, N, H, W, s));
    HIP_TRY(launch_coilcomp_eig(g, coils, (float2*)cmat, eig, N, s));
    p.end(3);
    return PNP_OK;
    PNP_API_END("pnp_coil_compress_matrix")
}

int pnp_coil_compress_apply(pnp_handle e, const float* in, int coils, const float* cmat, int cmat_n, int out_coils, float* out, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_coil_compress_apply";
    if (coils < 1 || coils > PNP_CC_MAX_COILS) return fail(PNP_ERR_INVALID, "%s: coils must be 1..%d (got %d)", fn, PNP_CC_MAX_COILS, coils);
    const int vmax = coils < PNP_MC_MAX_COILS ? coils : PNP_MC_MAX_COILS;
    if (out_coils < 1 || out_coils > vmax) return fail(PNP_ERR_INVALID, "%s: out_coils must be 1..min(coils, %d) = %d (got %d)", fn, PNP_MC_MAX_COILS, vmax, out_coils);
    if (cmat_n < 1) return fail(PNP_ERR_INVALID, "%s: cmat_n must be 1 or the handle's n (got %d)", fn, cmat_n);
    if (!in) return fail(PNP_ERR_INVALID, "%s: null in", fn);
    if (!cmat) return fail(PNP_ERR_INVALID, "%s: null cmat", fn);
    if (!out) return fail(PNP_ERR_INVALID, "%s: null out", fn);
    if (out == in || out == cmat) return fail(PNP_ERR_INVALID, "%s: out must not alias in or cmat", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w;
    if (cmat_n != 1 && cmat_n != N) return fail(PNP_ERR_INVALID, "%s: cmat_n must be 1 or the handle's n=%d (got %d)", fn, N, cmat_n);
    if (N > 65535) return fail(PNP_ERR_INVALID, "%s: n must be <= 65535 (got %d)", fn, N);
    PNP_ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    Prof p(e, s, PROF_OTHER, -1);
    HIP_TRY(launch_coilcomp_apply((const float2*)in, (const float2*)cmat, cmat_n, coils, out_coils, (float2*)out, N, H, W, s));
    return PNP_OK;
    PNP_API_END("pnp_coil_compress_apply")
}

int pnp_noise_cov(pnp_handle e, const float* noise, int noise_n, int coils, int samples, int flags, double* psi, void* stream) {
    PNP_API_BEGIN
    // every rejection happens before any HIP call, and leaves the outputs untouched; scalar ranges first
    const char* fn = "pnp_noise_cov";
    if (flags != 0) return fail(PNP_ERR_INVALID, "%s: flags must be 0 (got 0x%x)", fn, (unsigned)flags);
    if (coils < 1 || coils > PNP_PW_MAX_COILS) return fail(PNP_ERR_INVALID, "%s: coils must be 1..%d (got %d)", fn, PNP_PW_MAX_COILS, coils);
    if (samples < 1) return fail(PNP_ERR_INVALID, "%s: samples must be >= 1 (got %d)", fn, samples);
    if (noise_n < 1 || noise_n > 65535) return fail(PNP_ERR_INVALID, "%s: noise_n must be 1..65535 (got %d)", fn, noise_n);
    if (!noise) return fail(PNP_ERR_INVALID, "%s: null noise", fn);
    if (!psi) return fail(PNP_ERR_INVALID, "%s: null psi", fn);
    if ((const void*)psi == (const void*)noise) return fail(PNP_ERR_INVALID, "%s: psi must not alias noise", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    PNP_ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = pw_ensure(e, (size_t)noise_n * gram_chunks(samples) * coils * coils)) return rc;
    Prof p(e, s, PROF_OTHER, -1);
    HIP_TRY(launch_prewhiten_cov((const float2*)noise, noise_n, coils, samples, e->pw_part, (double2*)psi, s));
    p.end(2);
    return PNP_OK;
    PNP_API_END("pnp_noise_cov")
}

int pnp_whiten_matrix(pnp_handle e, const double* psi, int psi_n, int coils, int flags, float* wmat, float* lmat, int32_t* info, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_whiten_matrix";
    if (flags != 0) return fail(PNP_ERR_INVALID, "%s: flags must be 0 (got 0x%x)", fn, (unsigned)flags);
    if (coils < 1 || coils > PNP_PW_MAX_COILS) return fail(PNP_ERR_INVALID, "%s: coils must be 1..%d (got %d)", fn, PNP_PW_MAX_COILS, coils);
    if (psi_n < 1 || psi_n > 65535) return fail(PNP_ERR_INVALID, "%s: psi_n must be 1..65535 (got %d)", fn, psi_n);
    if (!psi) return fail(PNP_ERR_INVALID, "%s: null psi", fn);
    if (!wmat) return fail(PNP_ERR_INVALID, "%s: null wmat", fn);
    if (!info) return fail(PNP_ERR_INVALID, "%s: null info", fn);
    {
        const void* q[4] = {psi, wmat, info, lmat};
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j)
                if (q[j] && q[i] == q[j]) return fail(PNP_ERR_INVALID, "%s: psi, wmat, lmat and info must not alias", fn);
    }
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    PNP_ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    Prof p(e, s, PROF_OTHER, -1);
    HIP_TRY(launch_prewhiten_chol((const double2*)psi, psi_n, coils, (float2*)wmat, (float2*)lmat, (int*)info, s));
    return PNP_OK;
    PNP_API_END("pnp_whiten_matrix")
}

int pnp_whiten_apply(pnp_handle e, const float* in, int coils, const float* wmat, int wmat_n, float* out, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_whiten_apply";
    if (coils < 1 || coils > PNP_PW_MAX_COILS) return fail(PNP_ERR_INVALID, "%s: coils must be 1..%d (got %d)", fn, PNP_PW_MAX_COILS, coils);
    if (wmat_n < 1) return fail(PNP_ERR_INVALID, "%s: wmat_n must be 1 or the handle's n (got %d)", fn, wmat_n);
    if (!in) return fail(PNP_ERR_INVALID, "%s: null in", fn);
    if (!wmat) return fail(PNP_ERR_INVALID, "%s: null wmat", fn);
    if (!out) return fail(PNP_ERR_INVALID, "%s: null out", fn);
    if (out == wmat || in == wmat) return fail(PNP_ERR_INVALID, "%s: wmat must not alias in or out", fn);
    // out == in is the in-place call; any other overlap is refused.  The planes of the smallest handle (16 x 16) already span 2048 coils bytes,
    // so an offset below that overlaps whatever the handle is: refused before the handle is looked at
    const uintptr_t pi = (uintptr_t)in, po = (uintptr_t)out;
    const uintptr_t gap = pi < po ? po - pi : pi - po;
    if (gap != 0 && gap < (uintptr_t)2048 * (uintptr_t)coils)
        return fail(PNP_ERR_INVALID, "%s: out must be in exactly (in place) or must not overlap it (the buffers lie %zu bytes apart)", fn, (size_t)gap);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w;
    if (wmat_n != 1 && wmat_n != N) return fail(PNP_ERR_INVALID, "%s: wmat_n must be 1 or the handle's n=%d (got %d)", fn, N, wmat_n);
    if (N > 65535) return fail(PNP_ERR_INVALID, "%s: n must be <= 65535 (got %d)", fn, N);
    const uintptr_t bytes = (uintptr_t)N * coils * H * W * sizeof(float2), wbytes = (uintptr_t)wmat_n * coils * coils * sizeof(float2);
    if (gap != 0 && gap < bytes)
        return fail(PNP_ERR_INVALID, "%s: out must be in exactly (in place) or must not overlap it (the buffers lie %zu bytes apart)", fn, (size_t)gap);
    const uintptr_t pw = (uintptr_t)wmat;
    if ((pw < po + bytes && po < pw + wbytes) || (pw < pi + bytes && pi < pw + wbytes))
        return fail(PNP_ERR_INVALID, "%s: wmat must not alias in or out", fn);
    PNP_ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    Prof p(e, s, PROF_OTHER, -1);
    HIP_TRY(launch_prewhiten_apply((const float2*)in, (const float2*)wmat, wmat_n, coils, (float2*)out, N, H, W, s));
    return PNP_OK;
    PNP_API_END("pnp_whiten_apply")
}

int pnp_espirit_sens(pnp_handle e, const float* y0, int coils, int acs_h, int acs_w, int ksize, double sv_thresh, double crop, int iters,
                     int window, double thresh, int flags, float* sens, float* eval, float* kern, int32_t* nkept, void* stream) {
    PNP_API_BEGIN
    // every rejection happens before any HIP call, and leaves the outputs untouched; scalar ranges first
    const char* fn = "pnp_espirit_sens";
    if (flags != 0) return fail(PNP_ERR_INVALID, "%s: flags must be 0 (got 0x%x)", fn, (unsigned)flags);
    if (!(thresh >= 0.0) || !(thresh < 1.0)) return fail(PNP_ERR_INVALID, "%s: thresh must be finite and in [0, 1) (got %g)", fn, thresh);
    if (!(crop >= 0.0) || !(crop < 1.0)) return fail(PNP_ERR_INVALID, "%s: crop must be finite and in [0, 1) (got %g)", fn, crop);
    if (!(sv_thresh > 0.0) || !(sv_thresh < 1.0)) return fail(PNP_ERR_INVALID, "%s: sv_thresh must be in (0, 1) (got %g)", fn, sv_thresh);
    if (iters < 1 || iters > 64) return fail(PNP_ERR_INVALID, "%s: iters must be 1..64 (got %d)", fn, iters);
    if (window != PNP_SENS_BOX && window != PNP_SENS_HANN)
        return fail(PNP_ERR_INVALID, "%s: window must be PNP_SENS_BOX or PNP_SENS_HANN (got %d)", fn, window);
    if (coils < 1 || coils > PNP_ESPIRIT_MAX_COILS)
        return fail(PNP_ERR_INVALID, "%s: coils must be 1..%d (got %d); compress more channels first", fn, PNP_ESPIRIT_MAX_COILS, coils);
    if (ksize < 2 || ksize > PNP_ESPIRIT_MAX_KSIZE) return fail(PNP_ERR_INVALID, "%s: ksize must be 2..%d (got %d)", fn, PNP_ESPIRIT_MAX_KSIZE, ksize);
    if (coils * ksize * ksize > PNP_ESPIRIT_MAX_N)
        return fail(PNP_ERR_INVALID, "%s: coils * ksize^2 must be <= %d (got %d * %d^2)", fn, PNP_ESPIRIT_MAX_N, coils, ksize);
    if (acs_h < ksize || (acs_h & 1)) return fail(PNP_ERR_INVALID, "%s: acs_h must be even and >= ksize=%d (got %d)", fn, ksize, acs_h);
    if (acs_w < ksize || (acs_w & 1)) return fail(PNP_ERR_INVALID, "%s: acs_w must be even and >= ksize=%d (got %d)", fn, ksize, acs_w);
    if (!y0) return fail(PNP_ERR_INVALID, "%s: null y0", fn);
    if (!sens) return fail(PNP_ERR_INVALID, "%s: null sens", fn);
    if (sens == y0) return fail(PNP_ERR_INVALID, "%s: sens must not alias y0", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w;
    if (acs_h > H) return fail(PNP_ERR_INVALID, "%s: acs_h must be <= h=%d (got %d)", fn, H, acs_h);
    if (acs_w > W) return fail(PNP_ERR_INVALID, "%s: acs_w must be <= w=%d (got %d)", fn, W, acs_w);
    if (int rc = check_kspace_sizes(fn, e)) return rc;
    if ((long long)N * coils > 65535) return fail(PNP_ERR_INVALID, "%s: n * coils must be <= 65535 (got %d * %d)", fn, N, coils);
    PNP_ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    const size_t np = (size_t)espirit_padded(coils, ksize), D = (size_t)(2 * ksize - 1);
    const size_t mat_bytes = (size_t)N * 2 * np * np * sizeof(double2), kern_bytes = (size_t)N * coils * coils * D * D * sizeof(float2);
    if ((rc = cm_ensure(e, true))) return rc;
    if ((rc = es_ensure(e, mat_bytes + kern_bytes + (size_t)N * 8))) return rc;
    double2* const ws = (double2*)e->es_ws;
    float2* const R = kern ? (float2*)kern : (float2*)((char*)e->es_ws + mat_bytes);
    int* const nk = nkept ? (int*)nkept : (int*)((char*)e->es_ws + mat_bytes + kern_bytes);
    float* const smax = e->cm_max + (size_t)N * pixel_chunks(H, W);
    {   // the calibration part: Gram matrix, eigen-decomposition, kernel auto-correlation
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_espirit_gram((const float2*)y0, coils, acs_h, acs_w, ksize, ws, N, H, W, s));
        HIP_TRY(launch_espirit_eig(ws, coils, ksize, N, s));
        HIP_TRY(launch_espirit_kern(ws, coils, ksize, sv_thresh, R, nk, N, s));
        p.end(3);
    }
    {   // l_c, rss and smax exactly as pnp_estimate_sens forms them
        Prof p(e, s, PROF_OTHER, -1);
        HIP_TRY(launch_coilmap_window((const float2*)y0, (float2*)sens, acs_h, acs_w, window == PNP_SENS_HANN, N, coils, H, W, s));
    }
    if ((rc = plain_fft2(e, (float2*)sens, (float2*)sens, N * coils, 1, s))) return rc;
    Prof p(e, s, PROF_OTHER, -1);
    HIP_TRY(launch_coilmap_rss((const float2*)sens, coils, e->cm_rss, e->cm_max, N, H, W, s));
    HIP_TRY(launch_coilmap_max(e->cm_max, smax, N, H, W, s));
    HIP_TRY(launch_espirit_pixels((float2*)sens, R, e->cm_rss, smax, coils, ksize, iters, (float)crop, (float)thresh, eval, N, H, W, s));
    p.end(3);
    return PNP_OK;
    PNP_API_END("pnp_espirit_sens")
}

namespace {
// the kernel geometry shared by the two GRAPPA entry points; scalar ranges only, no handle
int grappa_check_kernel(const char* fn, int coils, int accel, int by, int bx) {
    if (coils < 1 || coils > PNP_GRAPPA_MAX_COILS) return fail(PNP_ERR_INVALID, "%s: coils must be 1..%d (got %d)", fn, PNP_GRAPPA_MAX_COILS, coils);
    if (accel < 2 || accel > PNP_GRAPPA_MAX_ACCEL) return fail(PNP_ERR_INVALID, "%s: accel must be 2..%d (got %d)", fn, PNP_GRAPPA_MAX_ACCEL, accel);
    if (by != 1 && by != 3 && by != 5 && by != 7) return fail(PNP_ERR_INVALID, "%s: by must be 1, 3, 5 or 7 (got %d)", fn, by);
    if (bx != 2 && bx != 4) return fail(PNP_ERR_INVALID, "%s: bx must be 2 or 4 (got %d)", fn, bx);
    if (coils * by * bx > PNP_GRAPPA_MAX_SRC)
        return fail(PNP_ERR_INVALID, "%s: coils * by * bx must be <= %d (got %d * %d * %d)", fn, PNP_GRAPPA_MAX_SRC, coils, by, bx);
    return PNP_OK;
}
// [a, a + an) and [b, b + bn) share a byte
bool ranges_overlap(const void* a, size_t an, const void* b, size_t bn) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + bn && pb < pa + an;
}
}  // namespace

int pnp_grappa_weights(pnp_handle e, const float* y0, int coils, int acs_h, int acs_w, int accel, int by, int bx, double lam, int flags,
                       float* wts, int32_t* info, double* gram, void* stream) {
    PNP_API_BEGIN
    // every rejection happens before any HIP call, and leaves the outputs untouched; scalar ranges first
    const char* fn = "pnp_grappa_weights";
    if (flags != 0) return fail(PNP_ERR_INVALID, "%s: flags must be 0 (got 0x%x)", fn, (unsigned)flags);
    if (!(lam >= 0.0) || !(lam <= 1.0)) return fail(PNP_ERR_INVALID, "%s: lam must be finite and in [0, 1] (got %g)", fn, lam);
    if (int rc = grappa_check_kernel(fn, coils, accel, by, bx)) return rc;
    const int span = (bx - 1) * accel + 1;
    if (acs_h < by || (acs_h & 1)) return fail(PNP_ERR_INVALID, "%s: acs_h must be even and >= by=%d (got %d)", fn, by, acs_h);
    if (acs_w < span || (acs_w & 1)) return fail(PNP_ERR_INVALID, "%s: acs_w must be even and >= (bx - 1) accel + 1 = %d (got %d)", fn, span, acs_w);
    if (!y0) return fail(PNP_ERR_INVALID, "%s: null y0", fn);
    if (!wts) return fail(PNP_ERR_INVALID, "%s: null wts", fn);
    if (!info) return fail(PNP_ERR_INVALID, "%s: null info", fn);
    {
        const void* q[4] = {y0, wts, info, gram};
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j)
                if (q[j] && q[i] == q[j]) return fail(PNP_ERR_INVALID, "%s: y0, wts, info and gram must not alias", fn);
    }
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w;
    if (W % accel) return fail(PNP_ERR_INVALID, "%s: accel must divide w=%d (got %d)", fn, W, accel);
    if (acs_h > H) return fail(PNP_ERR_INVALID, "%s: acs_h must be <= h=%d (got %d)", fn, H, acs_h);
    if (acs_w > W) return fail(PNP_ERR_INVALID, "%s: acs_w must be <= w=%d (got %d)", fn, W, acs_w);
    if ((long long)N * coils > 65535) return fail(PNP_ERR_INVALID, "%s: n * coils must be <= 65535 (got %d * %d)", fn, N, coils);
    const int ns = coils * by * bx, nt = coils * (accel - 1);
    {   // with the sizes known: no two of the four buffers may share a byte
        const void* q[4] = {y0, wts, info, gram};
        const size_t len[4] = {(size_t)N * coils * H * W * sizeof(float2), (size_t)N * nt * ns * sizeof(float2), (size_t)N * sizeof(int32_t),
                               (size_t)N * ns * (ns + nt) * sizeof(double2)};
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j)
                if (q[j] && ranges_overlap(q[i], len[i], q[j], len[j])) return fail(PNP_ERR_INVALID, "%s: y0, wts, info and gram must not alias", fn);
    }
    PNP_ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = gr_ensure(e, (size_t)N * ns * (ns + nt))) return rc;
    Prof p(e, s, PROF_OTHER, -1);
    HIP_TRY(launch_grappa_gram((const float2*)y0, coils, acs_h, acs_w, accel, by, bx, e->gr_ws, (double2*)gram, N, H, W, s));
    HIP_TRY(launch_grappa_solve(e->gr_ws, ns, nt, lam, (float2*)wts, (int*)info, N, s));
    p.end(2);
    return PNP_OK;
    PNP_API_END("pnp_grappa_weights")
}

int pnp_grappa_apply(pnp_handle e, const float* y0, int coils, const uint8_t* mask, int mask_n, int accel, int offset, int by, int bx,
                     const float* wts, int wts_n, float* out, void* stream) {
    PNP_API_BEGIN
    const char* fn = "pnp_grappa_apply";
    if (int rc = grappa_check_kernel(fn, coils, accel, by, bx)) return rc;
    if (offset < 0 || offset >= accel) return fail(PNP_ERR_INVALID, "%s: offset must be 0..accel-1 = %d (got %d)", fn, accel - 1, offset);
    if (mask_n < 1) return fail(PNP_ERR_INVALID, "%s: mask_n must be 1 or the handle's n (got %d)", fn, mask_n);
    if (wts_n < 1) return fail(PNP_ERR_INVALID, "%s: wts_n must be 1 or the handle's n (got %d)", fn, wts_n);
    if (!y0) return fail(PNP_ERR_INVALID, "%s: null y0", fn);
    if (!mask) return fail(PNP_ERR_INVALID, "%s: null mask", fn);
    if (!wts) return fail(PNP_ERR_INVALID, "%s: null wts", fn);
    if (!out) return fail(PNP_ERR_INVALID, "%s: null out", fn);
    // the planes of the smallest handle (16 x 16) already span 2048 coils bytes: a y0 and an out closer than that overlap whatever the handle is
    if (out == wts || (const void*)out == (const void*)mask || ranges_overlap(out, (size_t)2048 * coils, y0, (size_t)2048 * coils))
        return fail(PNP_ERR_INVALID, "%s: out must not overlap y0, wts or mask", fn);
    if (!e) return fail(PNP_ERR_INVALID, "%s: null handle", fn);
    const int N = e->cfg.n, H = e->cfg.h, W = e->cfg.w;
    if (W % accel) return fail(PNP_ERR_INVALID, "%s: accel must divide w=%d (got %d)", fn, W, accel);
    if (mask_n != 1 && mask_n != N) return fail(PNP_ERR_INVALID, "%s: mask_n must be 1 or the handle's n=%d (got %d)", fn, N, mask_n);
    if (wts_n != 1 && wts_n != N) return fail(PNP_ERR_INVALID, "%s: wts_n must be 1 or the handle's n=%d (got %d)", fn, N, wts_n);
    if ((long long)N * coils > 65535) return fail(PNP_ERR_INVALID, "%s: n * coils must be <= 65535 (got %d * %d)", fn, N, coils);
    const size_t ns = (size_t)coils * by * bx, nt = (size_t)coils * (accel - 1);
    const size_t bytes = (size_t)N * coils * H * W * sizeof(float2), wbytes = (size_t)wts_n * nt * ns * sizeof(float2), mbytes = (size_t)mask_n * H * W;
    if (ranges_overlap(out, bytes, y0, bytes) || ranges_overlap(out, bytes, wts, wbytes) || ranges_overlap(out, bytes, mask, mbytes))
        return fail(PNP_ERR_INVALID, "%s: out must not overlap y0, wts or mask", fn);
    PNP_ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    Prof p(e, s, PROF_OTHER, -1);
    HIP_TRY(launch_grappa_apply((const float2*)y0, mask, mask_n, (const float2*)wts, wts_n, (float2*)out, coils, accel, offset, by, bx, N, H, W, s));
    return PNP_OK;
    PNP_API_END("pnp_grappa_apply")
}

size_t pnp_snapshot_bytes(pnp_handle e) {
    return e ? SnapLayout(e).bytes() : 0;
}

int pnp_snapshot(pnp_handle e, const float* x, const float* z, const float* u, const float* t_state, void* dst,
                 void* stream) {
    PNP_API_BEGIN
    if (!e || !x || !z || !u || !dst) return fail(PNP_ERR_INVALID, "pnp_snapshot: null argument");
    PNP_ON_DEVICE(e);
    const SnapLayout snap(e);
    char* d = static_cast<char*>(dst);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(d, x, snap.x_bytes(), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + snap.z_off(), z, snap.zu_bytes(), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + snap.u_off(), u, snap.zu_bytes(), hipMemcpyDeviceToDevice, s));
    if (t_state) HIP_TRY(hipMemcpyAsync(d + snap.t_off(), t_state, snap.t_bytes(), hipMemcpyDeviceToDevice, s));
    else HIP_TRY(hipMemsetAsync(d + snap.t_off(), 0, snap.t_bytes(), s));
    return PNP_OK;
    PNP_API_END("pnp_snapshot")
}

int pnp_restore(pnp_handle e, const void* src, float* x, float* z, float* u, float* t_state, void* stream) {
    PNP_API_BEGIN
    if (!e || !x || !z || !u || !src) return fail(PNP_ERR_INVALID, "pnp_restore: null argument");
    PNP_ON_DEVICE(e);
    const SnapLayout snap(e);
    const char* d = static_cast<const char*>(src);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(x, d, snap.x_bytes(), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(z, d + snap.z_off(), snap.zu_bytes(), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(u, d + snap.u_off(), snap.zu_bytes(), hipMemcpyDeviceToDevice, s));
    if (t_state) HIP_TRY(hipMemcpyAsync(t_state, d + snap.t_off(), snap.t_bytes(), hipMemcpyDeviceToDevice, s));
    return PNP_OK;
    PNP_API_END("pnp_restore")
}

int pnp_unet_read_stage(pnp_handle e, int which, float* dst, int* c, int* hh, int* ww, void* stream) {
    PNP_API_BEGIN
    if (!e || which < 0 || which > 8) return fail(PNP_ERR_INVALID, "pnp_unet_read_stage: which must be 0..8");
    if (e->cfg.flags & PNP_FLAG_NO_DENOISER) return fail(PNP_ERR_STATE, "pnp_unet_read_stage: handle has no denoiser");
    const StagePlan& st = e->dplan.stage[which];
    if (st.fused_away) return fail(PNP_ERR_STATE, "pnp_unet_read_stage: stage 8 is fused away; create the handle with PNP_FLAG_KEEP_STAGES");
    if (st.bf16) return fail(PNP_ERR_STATE, "pnp_unet_read_stage: this stage is held as bf16 on this handle; create it with PNP_FLAG_KEEP_STAGES");
    PNP_ON_DEVICE(e);
    const float* src = e->plane[st.plane.level][st.plane.slot];
    if (c) *c = st.c;
    if (hh) *hh = st.h;
    if (ww) *ww = st.w;
    if (dst) HIP_TRY(launch_nhwc_to_nchw(src, dst, e->cfg.n, st.c, st.h, st.w, (hipStream_t)stream));
    return PNP_OK;
    PNP_API_END("pnp_unet_read_stage")
}

int pnp_conv_algorithms(pnp_handle e, int32_t* algo28) {
    PNP_API_BEGIN
    if (!e || !algo28) return fail(PNP_ERR_INVALID, "pnp_conv_algorithms: null argument");
    if (e->cfg.flags & PNP_FLAG_NO_DENOISER) return fail(PNP_ERR_STATE, "pnp_conv_algorithms: handle has no denoiser");
    for (int i = 0; i < N_LAYERS; ++i) algo28[i] = e->dplan.family[i];
    return PNP_OK;
    PNP_API_END("pnp_conv_algorithms")
}

int pnp_conv_schedules(pnp_handle e, int32_t* sched28) {
    PNP_API_BEGIN
    if (!e || !sched28) return fail(PNP_ERR_INVALID, "pnp_conv_schedules: null argument");
    if (e->cfg.flags & PNP_FLAG_NO_DENOISER) return fail(PNP_ERR_STATE, "pnp_conv_schedules: handle has no denoiser");
    for (int i = 0; i < N_LAYERS; ++i) {
        const int at = e->dplan.launch_of[i];
        sched28[i] = 0;
        if (at < 0 || e->dplan.family[i] != FAM_WINO4) continue;
        const WinoPlan& w = e->dplan.launch[at].wino;
        sched28[i] = w.cs ? 4 : (w.mt == 16 ? 3 : (w.phased ? 2 : 1));
    }
    return PNP_OK;
    PNP_API_END("pnp_conv_schedules")
}

int pnp_profile_reset(pnp_handle e) {
    PNP_API_BEGIN
    if (!e) return fail(PNP_ERR_INVALID, "null handle");
    e->ev_used = 0;
    memset(e->cls_ms, 0, sizeof e->cls_ms); memset(e->cls_n, 0, sizeof e->cls_n);
    memset(e->layer_ms, 0, sizeof e->layer_ms); memset(e->layer_n, 0, sizeof e->layer_n);
    return PNP_OK;
    PNP_API_END("pnp_profile_reset")
}

int pnp_profile_collect(pnp_handle e, double* total_ms, int64_t* launches) {
    PNP_API_BEGIN
    if (!e) return fail(PNP_ERR_INVALID, "null handle");
    PNP_ON_DEVICE(e);
    for (size_t i = 0; i < e->ev_used; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e->events[i].a, e->events[i].b));
        const EventPair& p = e->events[i];
        e->cls_ms[p.cls] += ms; e->cls_n[p.cls] += p.count;
        if (p.layer >= 0) { e->layer_ms[p.layer] += ms; e->layer_n[p.layer] += 1; }
    }
    e->ev_used = 0;
    for (int i = 0; i < PNP_PROFILE_CLASSES; ++i) {
        if (total_ms) total_ms[i] = e->cls_ms[i];
        if (launches) launches[i] = e->cls_n[i];
    }
    return PNP_OK;
    PNP_API_END("pnp_profile_collect")
}

int pnp_profile_layers(pnp_handle e, double* layer_ms, int64_t* layer_launches) {
    PNP_API_BEGIN
    if (!e) return fail(PNP_ERR_INVALID, "null handle");
    for (int i = 0; i < N_LAYERS; ++i) {
        if (layer_ms) layer_ms[i] = e->layer_ms[i];
        if (layer_launches) layer_launches[i] = e->layer_n[i];
    }
    return PNP_OK;
    PNP_API_END("pnp_profile_layers")
}

}  // extern "C"
