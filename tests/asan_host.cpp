// Host-side sanitizer check of libpnpadmm (tests/test_host_logic.py::test_host_side_under_asan_ubsan builds and runs it;
// `make -C dt4image_restoration_amd/csrc asan` builds the instrumented library, host code only).
// AddressSanitizer + UBSan see: the denoiser plan of every handle kind (plan_denoiser, the planner pnp_create runs) with its buffer liveness and
// format checks, every weight repack into buffers of exactly the size the library asks for (heap redzones catch an overrun by one float), and
// the argument validation of every C-ABI entry point.
// No GPU is needed: nothing here launches a kernel.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/pnpadmm.h"
#include "../dt4image_restoration_amd/csrc/pnp_internal.h"
#include "../dt4image_restoration_amd/csrc/denoiser_plan.h"

using namespace pnp;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d %s [%s]\n", __FILE__, __LINE__, #cond, g_case); ++fails; } } while (0)
static char g_case[128] = "";

// what an activation plane holds while the launches of a plan are walked in order
struct Held { int layer = -1; int c = 0, h = 0, w = 0; bool bf16 = false, pooled = false; };

// The U-Net's own wiring, from kLayers alone: layer li reads the output of li - 1; an upsample + concat layer reads it as the low-res input and, as its
// skip tensor, the output of the last encoder layer (before the first UPCAT layer) at its own level.
static int skip_producer(int li) {
    int first_up = N_LAYERS, at = -1;
    for (int i = N_LAYERS - 1; i >= 0; --i) if (kLayers[i].src == SRC_UPCAT) first_up = i;
    for (int i = 0; i < first_up; ++i) if (kLayers[i].level == kLayers[li].level) at = i;
    return at;
}

static void check_tiles(const ConvLaunch& l, int n, int h, int wd, bool bf16) {
    const LayerSpec& L = kLayers[l.layer];
    if (l.family == FAM_WINO2 || l.family == FAM_WINO4) {
        const WinoPlan& wp = l.wino;
        CHECK(wp.use && wp.algo == l.family && !bf16);
        CHECK(wp.tiles_x * wp.tw >= wd && wp.tiles_y * wp.th >= h && L.cin % wp.ck == 0);
        return;
    }
    const ConvPlan& cp = l.conv;
    CHECK(cp.tiles_x * cp.tw >= wd && cp.tiles_y * cp.th >= h && cp.splitk >= 1);
    CHECK(L.cin % cp.ck == 0);
    CHECK((l.family == FAM_WS) == (cp.ws != 0));
    if (!cp.ws) return;
    // bf16 mode, the producer / consumer plan: only with bf16 operands, always 32-channel chunks and whole tiles, one of its
    // five tile shapes, never split-K
    CHECK(bf16);
    CHECK(cp.ck == 32 && cp.splitk == 1 && cp.tw >= 16 && cp.bm == cp.th * cp.tw && L.cout % cp.bn == 0);
    CHECK((cp.mt == 4 && cp.nt == 2 && cp.wm * cp.wn == 4) || (cp.mt == 2 && cp.nt == 1 && cp.wm == 4 && cp.tw == 32 && l.src_mode == SRC_PLAIN));
    CHECK((long)cp.tiles_x * cp.tiles_y * n * (L.cout / cp.bn) >= 192);
    CHECK(l.src_mode != SRC_POOL || cp.wn == 2);
}

// every property of one handle's plan that needs no device
static void check_plan(const DenoiserPlan& P, const pnp_config& cfg, const Tuning& t) {
    const bool bf16 = (cfg.flags & PNP_FLAG_BF16_CONVS) != 0, keep = (cfg.flags & PNP_FLAG_KEEP_STAGES) != 0;
    const int n = cfg.n;
    CHECK(P.bf16_terms == (bf16 ? (t.bf16_w1 ? 1 : 2) : 0));
    CHECK(P.family[0] == FAM_FIRST && P.family[N_LAYERS - 1] == FAM_LAST);
    CHECK((P.launch_of[0] < 0) == P.fuse_first && (P.launch_of[N_LAYERS - 1] < 0) == P.fuse_last);
    CHECK(P.n_launches == N_LAYERS - (P.fuse_first ? 1 : 0) - (P.fuse_last ? 1 : 0));
    CHECK(!(keep && (P.fuse_last || P.act16)) && !(P.act16 && (!bf16 || t.bf16_f32_acts)));
    Held held[N_LEVELS][N_SLOTS];
    auto at = [&](PlaneRef r) -> Held& { return held[r.level][r.slot]; };
    size_t partial = 0;
    int prev_layer = -1;
    for (int i = 0; i < P.n_launches; ++i) {
        const ConvLaunch& l = P.launch[i];
        const LayerSpec& L = kLayers[l.layer];
        const int h = cfg.h >> L.level, wd = cfg.w >> L.level;
        CHECK(l.layer > prev_layer && P.launch_of[l.layer] == i && P.family[l.layer] == l.family);
        prev_layer = l.layer;
        CHECK((l.family == FAM_FIRST) == (l.layer == 0) && (l.family == FAM_LAST) == (l.layer == N_LAYERS - 1));
        const bool mfma = l.family != FAM_FIRST && l.family != FAM_LAST;
        if (mfma) {
            CHECK(l.family == FAM_DIRECT || l.family == FAM_WINO2 || l.family == FAM_WINO4 || l.family == FAM_WS);
            CHECK(!(t.bf16_no_ws && l.family == FAM_WS) && !(t.no_f4 && l.family == FAM_WINO4));
            check_tiles(l, n, h, wd, bf16);
            if (l.family == FAM_DIRECT) { const size_t f = conv3x3_partial_floats(l.conv, n, h, wd, L.cout); if (f > partial) partial = f; }
            CHECK(l.family == FAM_WINO4 || conv3x3_tensor_fits(n, h, wd, L.cin, L.cout));
            CHECK(l.conv.holdhi == (t.bf16_no_holdhi ? 0 : 1));
        }
        CHECK(P.act16 || l.act16 == 0);
        // (e) fusion only where the kernel has it
        CHECK(!l.fused_first || (l.layer == 1 && P.fuse_first && l.src_mode == SRC_FIRST && l.family == FAM_WINO4 && l.wino.bn == 32 && l.wino.mt == 32 &&
                                 !t.no_f4_fused_first));
        CHECK((l.src_mode == SRC_FIRST) == l.fused_first);
        CHECK(!l.fused_last || (l.layer == N_LAYERS - 2 && P.fuse_last && !keep &&
                                (l.family == FAM_WINO2 || (l.family == FAM_WINO4 && l.wino.bn == 32 && l.wino.mt == 32 && !t.no_f4_fused_last) ||
                                 ((l.family == FAM_DIRECT || l.family == FAM_WS) && conv3x3_pooled_output_ok(l.conv)))));
        CHECK(l.layer != 1 || l.fused_first == P.fuse_first);
        CHECK(l.layer != N_LAYERS - 2 || l.fused_last == P.fuse_last);
        // (b) no launch reads a plane it writes
        const bool reads0 = l.family != FAM_FIRST && !l.fused_first, reads1 = L.src == SRC_UPCAT;
        CHECK((l.src1.slot != SLOT_NONE) == reads1);
        for (PlaneRef wr : {l.dst, l.pooled}) {
            if (wr.slot == SLOT_NONE) continue;
            CHECK(!(reads0 && wr == l.src0) && !(reads1 && wr == l.src1));
        }
        CHECK(l.pooled.slot == SLOT_NONE || !(l.pooled == l.dst));
        // (a) every plane read holds the tensor the network wires to this input, at the size and channel count the launch expects, (c) in the format
        // the launch expects, (d) a pooled stage input read PLAIN from the producer's pooled copy exactly when there is one
        if (reads0) {
            const Held& s0 = at(l.src0);
            const int want = L.src == SRC_UPCAT ? skip_producer(l.layer) : l.layer - 1;
            CHECK(l.src0.slot != SLOT_NONE && s0.layer == want);
            CHECK(s0.c == (L.src == SRC_UPCAT ? L.cskip : L.cin));
            if (L.src == SRC_POOL) {
                const ConvLaunch& prod = P.launch[P.launch_of[l.layer - 1]];
                const bool copy = prod.pooled.slot != SLOT_NONE;
                CHECK(copy == P.pool_ok[L.level - 1]);
                CHECK(l.src_mode == (copy ? (int)SRC_PLAIN : (int)SRC_POOL));
                CHECK(l.src0 == (copy ? prod.pooled : prod.dst) && s0.pooled == copy);
                CHECK(copy ? (s0.h == h && s0.w == wd) : (s0.h == 2 * h && s0.w == 2 * wd));
            } else {
                CHECK(l.src_mode == (l.fused_first ? (int)SRC_FIRST : L.src) && !s0.pooled && s0.h == h && s0.w == wd);
            }
            CHECK(((l.act16 & 1) != 0) == s0.bf16);
        }
        if (reads1) {
            const Held& s1 = at(l.src1);
            CHECK(s1.layer == l.layer - 1 && s1.c == L.cin - L.cskip && s1.h == h / 2 && s1.w == wd / 2 && !s1.pooled && !s1.bf16);
        }
        // what it leaves behind (the fused last layer writes the caller's image instead of the stage output)
        if (l.family == FAM_LAST) { CHECK(l.dst.slot == SLOT_NONE && l.pooled.slot == SLOT_NONE); continue; }
        CHECK(l.dst.slot != SLOT_NONE && l.dst.slot != SLOT_POOL && l.dst.level == L.level);
        CHECK(P.plane_bytes[l.dst.level][l.dst.slot] == (size_t)n * h * wd * L.cout * sizeof(float));
        if (!l.fused_last) at(l.dst) = {l.layer, L.cout, h, wd, (l.act16 & 2) != 0, false};
        if (l.pooled.slot != SLOT_NONE) {
            CHECK(l.pooled.slot == SLOT_POOL && l.pooled.level == L.level && h % 2 == 0 && wd % 2 == 0 && P.pool_ok[L.level]);
            CHECK(l.family == FAM_WINO2 || l.family == FAM_WINO4 || conv3x3_pooled_output_ok(l.conv));
            CHECK(P.plane_bytes[L.level][SLOT_POOL] == (size_t)n * (h / 2) * (wd / 2) * L.cout * sizeof(float));
            at(l.pooled) = {l.layer, L.cout, h / 2, wd / 2, (l.act16 & 4) != 0, true};
        } else {
            CHECK(!(l.act16 & 4));
        }
    }
    // (g) the split-K workspace is the largest any direct launch asks for
    CHECK(P.partial_floats == partial);
    // the stage table: after the forward, every stage's plane still holds that stage's output - stage s is layers 3 s .. 3 s + 2
    for (int s = 0; s < N_STAGES; ++s) {
        const StagePlan& st = P.stage[s];
        const LayerSpec& L = kLayers[3 * s + 2];
        CHECK(st.c == L.cout && st.h == (cfg.h >> L.level) && st.w == (cfg.w >> L.level) && st.plane.level == L.level);
        CHECK(st.fused_away == (s == N_STAGES - 1 && P.fuse_last));                       // (e)
        if (st.fused_away) continue;
        const Held& hd = at(st.plane);
        CHECK(hd.layer == 3 * s + 2 && hd.c == st.c && hd.h == st.h && hd.w == st.w && hd.bf16 == st.bf16);
        if (keep) CHECK(!st.bf16);
        for (int s2 = 0; s2 < s; ++s2) CHECK(!(P.stage[s2].plane == st.plane));
    }
}

// (f) the weight repack of every conv3x3 launch with the family and chunk size of ITS plan, into a buffer of exactly the size the library asks for
static size_t repack(const DenoiserPlan& P) {
    std::vector<float> w;
    size_t packed = 0;
    for (int i = 0; i < P.n_launches; ++i) {
        const ConvLaunch& l = P.launch[i];
        const LayerSpec& L = kLayers[l.layer];
        if (l.family == FAM_FIRST || l.family == FAM_LAST) continue;
        w.assign((size_t)L.cout * L.cin * 9, 0.f);
        for (size_t k = 0; k < w.size(); ++k) w[k] = (float)((k * 2654435761u) % 1000) * 1e-3f - 0.5f;
        size_t pf;
        switch (l.family) {
        case FAM_WINO4: pf = winograd4_pack_floats(L.cin, L.cout); break;
        case FAM_WINO2: pf = winograd_pack_floats(L.cin, L.cout); break;
        default: pf = P.bf16_terms ? conv3x3_pack_floats_bf16(L.cin, L.cout, P.bf16_terms) : conv3x3_pack_floats(L.cin, L.cout);
        }
        float* dst = (float*)std::malloc(pf * sizeof(float));          // exact size: redzones right behind it
        if (l.family == FAM_WINO4) pack_winograd4_weights(w.data(), L.cin, L.cout, l.wino.ck, dst);
        else if (l.family == FAM_WINO2) pack_winograd_weights(w.data(), L.cin, L.cout, l.wino.ck, dst);
        else if (P.bf16_terms) pack_conv3x3_weights_bf16(w.data(), L.cin, L.cout, l.conv.ck, P.bf16_terms, dst);
        else pack_conv3x3_weights(w.data(), L.cin, L.cout, l.conv.ck, dst);
        std::free(dst);
        ++packed;
    }
    return packed;
}

int main() {
    // ---- the plan of every handle kind over the sizes the tests and the bench use, and the packs of two of them ------------------------
    const int shapes[][3] = {{1, 128, 128}, {64, 256, 256}, {4, 256, 256}, {2, 48, 64}, {16, 512, 512}, {1, 16, 16}, {3, 64, 16},
                             {8, 272, 272}, {2, 256, 144}, {1, 320, 320}, {256, 128, 128}, {1, 1024, 1024}};
    const int flagsv[] = {0, PNP_FLAG_KEEP_STAGES, PNP_FLAG_BF16_CONVS, PNP_FLAG_BF16_CONVS | PNP_FLAG_KEEP_STAGES};
    const char* names[9] = {"default", "wino_min_blocks=1", "no_f4", "no_f4_fused_last", "no_f4_fused_first", "bf16_no_ws", "bf16_f32_acts", "bf16_w1",
                            "bf16_no_holdhi"};
    Tuning variants[9];
    for (auto& t : variants) t = tuning_from_env();
    variants[1].wino_min_blocks = 1;
    variants[2].no_f4 = true;
    variants[3].no_f4_fused_last = true;
    variants[4].no_f4_fused_first = true;
    variants[5].bf16_no_ws = true;
    variants[6].bf16_f32_acts = true;
    variants[7].bf16_w1 = true;
    variants[8].bf16_no_holdhi = true;
    size_t packed_layers = 0, plans = 0, pooled_sources = 0, fused_first = 0, fused_last = 0, act16 = 0;
    for (int v = 0; v < 9; ++v)
        for (const auto& sh : shapes)
            for (int fl : flagsv) {
                std::snprintf(g_case, sizeof g_case, "%s %dx%dx%d flags=%d", names[v], sh[0], sh[1], sh[2], fl);
                const pnp_config cfg = {sh[0], sh[1], sh[2], 0, fl};
                DenoiserPlan P;
                std::string err;
                const bool ok = plan_denoiser(cfg, variants[v], &P, &err);
                CHECK(ok && err.empty());
                if (!ok) continue;
                check_plan(P, cfg, variants[v]);
                ++plans;
                for (int i = 0; i < P.n_launches; ++i) pooled_sources += kLayers[P.launch[i].layer].src == SRC_POOL && P.launch[i].src_mode == SRC_POOL;
                fused_first += P.fuse_first; fused_last += P.fuse_last; act16 += P.act16;
                // repack (slow under ASan) for two shapes only, f32 and bf16 handles, the default and the forced-Winograd plans and one-term weights
                if ((&sh == &shapes[0] || &sh == &shapes[3]) && !(fl & PNP_FLAG_KEEP_STAGES) && (v <= 1 || (v == 7 && fl))) packed_layers += repack(P);
            }
    g_case[0] = 0;
    CHECK(plans == 9 * 12 * 4 && packed_layers > 100);
    CHECK(pooled_sources > 0 && fused_first > 0 && fused_last > 0 && act16 > 0);       // the sweep reaches every plan feature
    {   // a handle the planner refuses: layer 1's output is exactly 2^31 bytes and bf16 mode plans no F(4x4); a k-space-only handle plans nothing
        DenoiserPlan P;
        std::string err;
        pnp_config big = {256, 256, 256, 0, PNP_FLAG_BF16_CONVS};
        CHECK(!plan_denoiser(big, variants[0], &P, &err) && err.find("2 GiB") != std::string::npos);
        big.flags = PNP_FLAG_NO_DENOISER;
        err.clear();
        CHECK(plan_denoiser(big, variants[0], &P, &err) && P.n_launches == 0 && P.partial_floats == 0);
        for (auto& lv : P.plane_bytes) for (size_t b : lv) CHECK(b == 0);
    }

    // ---- C ABI argument validation (every entry point, no GPU behind it) ------------------------------------------------
    pnp_handle h = nullptr;
    pnp_config bad = {0, 128, 128, 0, 0};
    CHECK(pnp_create(&bad, &h) == PNP_ERR_INVALID && h == nullptr && std::strlen(pnp_last_error()) > 0);
    bad = {1, 100, 128, 0, 0};
    CHECK(pnp_create(&bad, &h) == PNP_ERR_INVALID);
    bad = {1, 2048, 128, 0, 0};
    CHECK(pnp_create(&bad, &h) == PNP_ERR_INVALID);
    CHECK(pnp_create(nullptr, &h) == PNP_ERR_INVALID && pnp_create(&bad, nullptr) == PNP_ERR_INVALID);
    bad = {256, 256, 256, 0, PNP_FLAG_BF16_CONVS};      // refused by the planner, before any device call
    CHECK(pnp_create(&bad, &h) == PNP_ERR_INVALID && h == nullptr && std::strstr(pnp_last_error(), "2 GiB") != nullptr);
    pnp_config ok = {1, 128, 128, 0, 0};
    const int rc = pnp_create(&ok, &h);                 // no GPU here: must fail cleanly, with a message, leaking nothing
    if (rc != PNP_OK) CHECK(h == nullptr && std::strlen(pnp_last_error()) > 0);
    else CHECK(pnp_destroy(h) == PNP_OK);
    float f = 0.f; uint8_t b = 0; int c;
    CHECK(pnp_destroy(nullptr) == PNP_OK);
    CHECK(pnp_load_unet_weights(nullptr, &f, 1) == PNP_ERR_INVALID);
    CHECK(pnp_reset(nullptr, &f, &f, &b, 1, &f, &f, &f, nullptr) == PNP_ERR_INVALID);
    CHECK(pnp_set_kspace(nullptr, &f, &b, 1, nullptr) == PNP_ERR_INVALID);
    CHECK(pnp_step(nullptr, &f, &f, &f, &f, &f, &f, &f, &b, nullptr) == PNP_ERR_INVALID);
    CHECK(pnp_denoise(nullptr, &f, &f, &f, nullptr) == PNP_ERR_INVALID);
    CHECK(pnp_fft2c(nullptr, &f, &f, 1, 128, 128, 0, nullptr) == PNP_ERR_INVALID);
    CHECK(pnp_prox_dual(nullptr, &f, &f, &f, &f, &f, nullptr) == PNP_ERR_INVALID);
    CHECK(pnp_psnr(nullptr, &f, &f, &f, nullptr) == PNP_ERR_INVALID);
    CHECK(pnp_snapshot(nullptr, &f, &f, &f, &f, &f, nullptr) == PNP_ERR_INVALID);
    CHECK(pnp_restore(nullptr, &f, &f, &f, &f, &f, nullptr) == PNP_ERR_INVALID);
    CHECK(pnp_unet_read_stage(nullptr, 0, &f, &c, &c, &c, nullptr) == PNP_ERR_INVALID);
    CHECK(pnp_conv_algorithms(nullptr, nullptr) == PNP_ERR_INVALID);
    CHECK(pnp_profile_reset(nullptr) == PNP_ERR_INVALID && pnp_profile_collect(nullptr, nullptr, nullptr) == PNP_ERR_INVALID);
    CHECK(pnp_profile_layers(nullptr, nullptr, nullptr) == PNP_ERR_INVALID);
    CHECK(pnp_snapshot_bytes(nullptr) == 0 && pnp_workspace_bytes(nullptr) == 0);
    CHECK(std::strstr(pnp_version(), "gfx950") != nullptr);
    std::printf("asan_host: %zu layer repacks, %d failures\n", packed_layers, fails);
    return fails ? 1 : 0;
}
