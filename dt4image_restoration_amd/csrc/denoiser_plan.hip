// plan_denoiser(): the launch plan of one denoiser forward, from the handle's configuration and tuning alone (host code, no HIP call).
// The schedule - which plane every layer reads and writes - is derived from kLayers[]: a stage is three consecutive layers; a stage's
// last layer writes the level's skip plane on the way down; an upsample + concat layer reads the skip plane of its own level and the
// previous stage's output.
#include "denoiser_plan.h"

#include <cstdio>

namespace pnp {

namespace {

constexpr int kStageLayers = 3;
constexpr int kFirstLayer = 0, kLastLayer = N_LAYERS - 1;   // the 2 -> 32 and 1x1 layers around the 26 conv3x3 MFMA layers
constexpr int kHead = kFirstLayer + 1;                      // inc.conv-1: can evaluate the first layer while staging
constexpr int kTail = kLastLayer - 1;                       // up4.conv-2: can carry the last layer in its epilogue

bool is_wino(const ConvLaunch& l) { return l.family == FAM_WINO2 || l.family == FAM_WINO4; }

// Does layer `l` (a stage's last conv, planned already) also write the 2x2 max-pooled copy of its output?  Its output must have
// even sides and its kernel must support it (a Winograd kernel, or the direct kernel's LDS-epilogue plan).  ONE predicate for the
// consumer's planned source mode and for the pooled plane of the launch record.
bool pooled_copy_ok(const pnp_config& cfg, const ConvLaunch& l) {
    const int lh = cfg.h >> kLayers[l.layer].level, lw = cfg.w >> kLayers[l.layer].level;
    return lh % 2 == 0 && lw % 2 == 0 && (is_wino(l) || conv3x3_pooled_output_ok(l.conv));
}

}  // namespace

bool plan_denoiser(const pnp_config& cfg, const Tuning& tune, DenoiserPlan* out, std::string* err) {
    DenoiserPlan& P = *out;
    P = DenoiserPlan{};
    const bool bf16 = (cfg.flags & PNP_FLAG_BF16_CONVS) != 0;
    const bool keep_stages = (cfg.flags & PNP_FLAG_KEEP_STAGES) != 0;
    P.bf16_terms = bf16 ? (tune.bf16_w1 ? 1 : 2) : 0;
    if (cfg.flags & PNP_FLAG_NO_DENOISER) return true;      // k-space-only handle: no launches, no activation planes

    // ---- the schedule: one record per layer, planes by name --------------------------------------------------------------------------
    ConvLaunch rec[N_LAYERS] = {};
    int first_up = N_LAYERS;
    for (int li = N_LAYERS - 1; li >= 0; --li) if (kLayers[li].src == SRC_UPCAT) first_up = li;
    for (int li = 0; li < N_LAYERS; ++li) {
        const LayerSpec& L = kLayers[li];
        ConvLaunch& r = rec[li];
        r.layer = li;
        r.src_mode = L.src;
        const int pos = li % kStageLayers;
        if (li != kLastLayer) r.dst = {L.level, pos == 0 ? SLOT_PING : (pos == 1 ? SLOT_PONG : (li < first_up ? SLOT_SKIP : SLOT_PING))};
        if (li == kFirstLayer) continue;                    // reads the caller's image
        if (L.src == SRC_UPCAT) { r.src0 = {L.level, SLOT_SKIP}; r.src1 = rec[li - 1].dst; }
        else r.src0 = rec[li - 1].dst;                      // (a pooled stage input moves to the producer's pooled copy below)
    }
    rec[kFirstLayer].family = FAM_FIRST;
    rec[kLastLayer].family = FAM_LAST;

    // ---- launch plans of the 26 conv3x3 layers: fixed here, used by the weight pack and by every launch --------------------------------
    for (int li = kHead; li <= kTail; ++li) {
        const LayerSpec& L = kLayers[li];
        ConvLaunch& r = rec[li];
        const int lh = cfg.h >> L.level, lw = cfg.w >> L.level;
        // the source mode the launch will use: a pooled stage input is read PLAIN from the producer's pooled copy, which
        // exists iff the producing layer (li - 1, planned just before) runs a Winograd kernel or the direct LDS-epilogue plan
        // (the producer's output size - twice this layer's - must be even, which it always is, and its kernel must be one that
        // writes the pooled copy).  Which stage outputs get one: the producing conv must run a kernel whose epilogue goes through
        // LDS - the Winograd kernel, or the direct kernel's Cout = 32 configuration on a large problem
        if (L.src == SRC_POOL && pooled_copy_ok(cfg, rec[li - 1])) {
            r.src_mode = SRC_PLAIN;
            rec[li - 1].pooled = r.src0 = {kLayers[li - 1].level, SLOT_POOL};
            P.pool_ok[kLayers[li - 1].level] = true;
        }
        r.wino = winograd_plan(cfg.n, lh, lw, L.cin, L.cout, r.src_mode, tune, L.cskip);
        if (li == kTail && r.wino.algo == 4 && !keep_stages && (tune.no_f4_fused_last || r.wino.bn != 32 || r.wino.mt != 32)) {
            // up4.conv-2 carries the fused last layer (1x1 conv + residual + clamp) in its epilogue: the F(4x4) kernel's
            // 32-channel variant has it (DPP reduce-scatter over a pixel's channels); PNP_NO_F4_FUSED_LAST puts the layer
            // back on the F(2x2) kernel, which walks whole pixels there
            Tuning t2 = tune;
            t2.no_f4 = true;
            r.wino = winograd_plan(cfg.n, lh, lw, L.cin, L.cout, r.src_mode, t2, L.cskip);
        }
        // (the producer / consumer kernel's upsample is the separable form: only on heights with the regular line structure)
        const bool ws_ok = !tune.bf16_no_ws && (r.src_mode != SRC_UPCAT || upsample_lines_regular(lh));
        r.conv = conv3x3_plan(cfg.n, lh, lw, L.cin, L.cout, bf16, r.src_mode, ws_ok);
        // up4.conv-2 (fused last layer): on the producer / consumer kernel only in the two-term mode, where its producers evaluate the last
        // layer (OFFLOAD); the one-term form of that tile measured slower than conv_kernels.hip (conv3x3_plan)
        r.conv.holdhi = tune.bf16_no_holdhi ? 0 : 1;
        if (li == kTail && r.conv.nt == 1 && (P.bf16_terms != 2 || tune.bf16_no_holdhi)) r.conv.ws = 0;
        r.family = (r.wino.use && !bf16) ? (r.wino.algo == 4 ? FAM_WINO4 : FAM_WINO2) : (r.conv.ws ? FAM_WS : FAM_DIRECT);
        if (r.family == FAM_WINO4) continue;                      // (per-slice descriptors)
        if (!conv3x3_tensor_fits(cfg.n, lh, lw, L.cin, L.cout)) {
            char buf[512];
            snprintf(buf, sizeof buf, "pnp_create: layer %d's output tensor (%d x %d x %d x %d floats) reaches 2 GiB, past this "
                     "kernel's buffer descriptor: use a smaller batch per handle", li, cfg.n, lh, lw, L.cout);
            *err = buf;
            return false;
        }
        if (is_wino(r)) continue;
        const size_t f = conv3x3_partial_floats(r.conv, cfg.n, lh, lw, L.cout);
        if (f > P.partial_floats) P.partial_floats = f;
    }

    P.fuse_last = !keep_stages && (is_wino(rec[kTail]) || conv3x3_pooled_output_ok(rec[kTail].conv));
    P.fuse_first = rec[kHead].family == FAM_WINO4 && rec[kHead].wino.bn == 32 && rec[kHead].wino.mt == 32 && !tune.no_f4_fused_first;
    if (P.fuse_first) { rec[kHead].fused_first = true; rec[kHead].src_mode = SRC_FIRST; }
    rec[kTail].fused_last = P.fuse_last;

    // writer of every launch's src0 plane, and the decoder layer that reads a stage output as its skip tensor (0: none)
    int src0_from[N_LAYERS] = {}, skip_reader[N_LAYERS] = {};
    for (int li = kHead; li <= kLastLayer; ++li) {
        int w = li - 1;
        while (w > 0 && !(rec[w].dst == rec[li].src0) && !(rec[w].pooled == rec[li].src0)) --w;
        src0_from[li] = w;
        if (kLayers[li].src == SRC_UPCAT) skip_reader[w] = li;
    }

    // bf16 mode: the five 32-channel level-0 layers exchange bf16 tensors (same bits the staging would round to; half the
    // bytes of the HBM-bound level).  Needs the plan that has the variant on all five and the pooled copy for down1
    // (always so today); a KEEP_STAGES handle keeps f32 stages for pnp_unet_read_stage.
    P.act16 = bf16 && !keep_stages && !tune.bf16_f32_acts && P.pool_ok[0];
    for (int li = kHead; li <= kTail; ++li)
        if (kLayers[li].level == 0) P.act16 = P.act16 && conv3x3_pooled_output_ok(rec[li].conv);
    if (P.act16) {
        // ... and so do the layers of the producer / consumer kernel among themselves: a tensor is bf16 when the launch that
        // writes it and every launch that reads it as src0 (next layer, PLAIN or POOL; the decoder layer taking it as its
        // skip tensor) can; the low-res input of an upsample (the src1 of an UPCAT layer) stays f32 - its consumer
        // rounds after interpolating - and so do the pooled copy of level 0 and the input of the unfused 1x1 conv
        auto can = [&](int li) { return li >= kHead && li <= kTail && (kLayers[li].level == 0 || rec[li].conv.ws != 0); };
        bool out16[N_LAYERS] = {};
        out16[kFirstLayer] = true;                             // conv_first -> inc.conv-1
        for (int li = kHead; li < kTail; ++li) {
            if (kLayers[li + 1].src == SRC_UPCAT) continue;
            // (a stage's last layer: the next stage reads the f32 pooled copy instead when there is one)
            const bool next_reads = rec[li + 1].src0 == rec[li].dst;
            out16[li] = can(li) && (!next_reads || can(li + 1)) && (skip_reader[li] == 0 || can(skip_reader[li]));
        }
        for (int li = kHead; li <= kTail; ++li) {
            // (a pooled source: the producer's f32 pooled copy)
            const bool in16 = rec[li].src0.slot == SLOT_POOL ? false : out16[src0_from[li]];
            // the level-0 kernel writes bf16 only from its bf16-source variant
            if (kLayers[li].level == 0 && !in16) out16[li] = false;
            rec[li].act16 = (in16 ? 1 : 0) | (out16[li] ? 2 : 0);
        }
        rec[kFirstLayer].act16 = 2;
        // round 5: level 0's pooled copy (inc.conv-2 -> down1.conv-0) as bf16 too when both layers run the producer / consumer kernel:
        // rounding to nearest even is monotonic, so bf16(max(a, b, c, d)) == max(bf16(a), ...) - the bits down1.conv-0 stages are the
        // ones it rounded the f32 copy to, at half the bytes written and read (bit 2 of the writer's act16, bit 0 of the reader's)
        for (int li = kHead; li < kTail; ++li) {
            ConvLaunch &w = rec[li], &r = rec[li + 1];
            if (kLayers[li].level == 0 && w.pooled.slot == SLOT_POOL && (w.act16 & 2) && w.conv.ws && r.conv.ws && w.conv.holdhi && P.bf16_terms == 2) {
                w.act16 |= 4;
                r.act16 |= 1;
            }
        }
    }

    // ---- what the handle allocates and serves ----------------------------------------------------------------------------------------
    for (int li = kFirstLayer; li <= kTail; ++li) {
        const LayerSpec& L = kLayers[li];
        const size_t bytes = (size_t)cfg.n * (cfg.h >> L.level) * (cfg.w >> L.level) * L.cout * sizeof(float);
        P.plane_bytes[L.level][rec[li].dst.slot] = bytes;
        // (the pooled plane of a level is allocated whether or not this handle's kernels write it)
        if (kLayers[li + 1].src == SRC_POOL) P.plane_bytes[L.level][SLOT_POOL] = bytes / 4;
    }
    for (int s = 0; s < N_STAGES; ++s) {
        const ConvLaunch& r = rec[kStageLayers * s + kStageLayers - 1];
        const LayerSpec& L = kLayers[r.layer];
        P.stage[s] = {r.dst, L.cout, cfg.h >> L.level, cfg.w >> L.level, (r.act16 & 2) != 0, r.fused_last};
    }
    for (int li = 0; li < N_LAYERS; ++li) {
        P.family[li] = rec[li].family;
        const bool fused = (li == kFirstLayer && P.fuse_first) || (li == kLastLayer && P.fuse_last);
        P.launch_of[li] = fused ? -1 : P.n_launches;
        if (!fused) P.launch[P.n_launches++] = rec[li];
    }
    return true;
}

}  // namespace pnp
