// The denoiser's launch plan: which kernel family runs each conv layer, with which tile plan and source mode, which activation plane
// every launch reads and writes, and what the handle has to allocate for it.  plan_denoiser() is pure host code (no HIP call), so the
// plan a handle uses is the plan the CPU suite checks (tests/asan_host.cpp); pnp_capi.hip allocates, packs weights and launches from it.
#pragma once
#include "../../include/pnpadmm.h"
#include "pnp_internal.h"
#include <string>

namespace pnp {

// the codes pnp_conv_algorithms reports
enum ConvFamily : int {
    FAM_DIRECT = 0,   // conv_kernels.hip
    FAM_WINO2 = 1,    // F(2x2,3x3), winograd_kernels.hip
    FAM_FIRST = 2,    // the 2 -> 32 first layer (conv_first_kernel)
    FAM_LAST = 3,     // the 1x1 last layer + residual + clamp (conv_last_kernel)
    FAM_WINO4 = 4,    // F(4x4,3x3), winograd4_kernels.hip
    FAM_WS = 5,       // bf16 mode's producer / consumer kernel (conv_bf16_kernels.hip), launched through the direct launcher
};

// An activation plane by name: levels 0..4 (h >> level rows), each with a ping, a pong and a skip plane (the stage output kept for the
// up path) and, above the bottom level, the MaxPool2d(2) copy of the skip plane at a quarter of its size.
enum PlaneSlot : int { SLOT_NONE = 0, SLOT_PING, SLOT_PONG, SLOT_SKIP, SLOT_POOL, N_SLOTS };
static constexpr int N_LEVELS = 5;
struct PlaneRef {
    int level = 0, slot = SLOT_NONE;
    bool operator==(const PlaneRef& o) const { return level == o.level && slot == o.slot; }
};

struct ConvLaunch {
    int layer;                // index into kLayers
    int family;               // ConvFamily
    int src_mode;             // the source mode of the launch: a POOL layer whose producer writes the pooled copy runs PLAIN
    PlaneRef src0, src1, dst, pooled;   // src0: none for the first layer (it reads the caller's image); src1: the UPCAT low-res input
    bool fused_first;         // evaluates the first layer while staging its patch (SRC_FIRST)
    bool fused_last;          // carries the last layer (1x1 conv + residual + clamp) in its epilogue and writes the caller's output
    int act16;                // ConvArgs.act16: bit 0 = src0 holds bf16, bit 1 = dst holds bf16, bit 2 = the pooled copy is written as bf16
    WinoPlan wino;            // FAM_WINO2 / FAM_WINO4
    ConvPlan conv;            // FAM_DIRECT / FAM_WS, ws and holdhi final
};

static constexpr int N_STAGES = 9;   // inc, down1..4, up1..4: the outputs pnp_unet_read_stage serves
struct StagePlan {
    PlaneRef plane;
    int c, h, w;
    bool bf16;                // held as bf16 on this handle: not readable
    bool fused_away;          // never written: the launch that would write it carries the fused last layer instead
};

struct DenoiserPlan {
    int n_launches = 0;                   // 0: a handle without a denoiser (PNP_FLAG_NO_DENOISER)
    ConvLaunch launch[N_LAYERS] = {};     // in launch order; a layer fused into its neighbour has no record of its own
    int launch_of[N_LAYERS] = {};         // layer -> index into launch[], -1: fused away
    int family[N_LAYERS] = {};            // per layer, fused ones included
    bool fuse_first = false;              // first layer (2 -> 32) is computed in the staging of inc.conv-1 (F(4x4) 32-channel variant)
    bool fuse_last = false;               // last 1x1 layer rides in the epilogue of up4.conv-2
    bool act16 = false;                   // bf16 mode: the 32-channel level-0 activations are stored as bf16
    int bf16_terms = 0;                   // bf16 mode: bf16 terms per conv weight (2: hi + lo, the default; 1: PNP_BF16_W1); 0 = f32 mode
    bool pool_ok[N_LEVELS] = {};          // the level's stage output also gets a pooled copy (its producing kernel supports it)
    size_t partial_floats = 0;            // split-K workspace
    size_t plane_bytes[N_LEVELS][N_SLOTS] = {};
    StagePlan stage[N_STAGES] = {};
};

// false: the handle is refused, `err` says why (the pnp_create message)
bool plan_denoiser(const pnp_config& cfg, const Tuning& t, DenoiserPlan* out, std::string* err);

}  // namespace pnp
