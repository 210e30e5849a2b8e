// Host-only check of the cout-split rule of winograd_plan (run by tests/test_wino4_coutsplit_plan_host.py against the built library):
// the schedule is an alternative INSIDE F(4x4) - at no batch size may a layer that is on F(4x4) without it (PNP_WINO_F4_CS=0) leave
// F(4x4) with it, under the default rule or under PNP_WINO_F4_CS=2, and a layer that takes it passes the workgroup-count gate with
// its own (halved) workgroup count.  Prints one line per checked handle shape and "plan_coutsplit_host: N failures".
#include <cstdio>
#include <string>

#include "../dt4image_restoration_amd/csrc/denoiser_plan.h"

using namespace pnp;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static long cs_blocks(const WinoPlan& w, int n, int cout) { return (long)w.tiles_x * w.tiles_y * n * (cout / 128); }

int main() {
    const int sizes[][2] = {{256, 256}, {128, 128}, {512, 512}, {320, 320}, {144, 64}, {96, 112}, {64, 64}};
    for (const auto& hw : sizes)
        for (int n = 1; n <= 96; ++n) {
            pnp_config cfg{n, hw[0], hw[1], 0, 0};
            Tuning off{}, dflt{}, all{};
            off.f4_cs = 0;
            all.f4_cs = 2;
            DenoiserPlan P0, P1, P2;
            std::string err;
            if (!plan_denoiser(cfg, off, &P0, &err)) continue;
            CHECK(plan_denoiser(cfg, dflt, &P1, &err) && plan_denoiser(cfg, all, &P2, &err), "n %d %d x %d: %s", n, hw[0], hw[1], err.c_str());
            int taken1 = 0, taken2 = 0;
            for (int li = 0; li < N_LAYERS; ++li) {
                CHECK(P1.family[li] == P0.family[li] && P2.family[li] == P0.family[li], "n %d %d x %d layer %d: family %d without the schedule, %d default, %d forced",
                      n, hw[0], hw[1], li, P0.family[li], P1.family[li], P2.family[li]);
                for (const DenoiserPlan* P : {&P1, &P2}) {
                    const int at = P->launch_of[li];
                    if (at < 0 || P->family[li] != FAM_WINO4 || !P->launch[at].wino.cs) continue;
                    const WinoPlan& w = P->launch[at].wino;
                    (P == &P1 ? taken1 : taken2) += 1;
                    CHECK(kLayers[li].cout % 128 == 0 && w.bn == 128 && w.mt == 16 && !w.stack && !w.phased, "layer %d", li);
                    CHECK(cs_blocks(w, n, kLayers[li].cout) >= dflt.wino_min_blocks, "n %d %d x %d layer %d: %ld workgroups", n, hw[0], hw[1], li,
                          cs_blocks(w, n, kLayers[li].cout));
                    CHECK(P == &P2 || kLayers[li].src == SRC_UPCAT, "default rule: upsample + concat layers only (layer %d)", li);
                }
            }
            CHECK(taken1 <= taken2, "default rule takes no layer the forced rule does not");
            if (hw[0] == 256 && hw[1] == 256 && (n == 8 || n == 16 || n == 64))
                std::printf("256x256 n %d: up1.conv-0 family %d (schedule off: %d) cs %d, up2.conv-0 family %d (schedule off: %d) cs %d; layers on the schedule: default %d, forced %d\n", n,
                            P1.family[15], P0.family[15], P1.launch[P1.launch_of[15]].wino.cs, P1.family[18], P0.family[18], P1.launch[P1.launch_of[18]].wino.cs, taken1, taken2);
        }
    // an upsample + concat layer with an unknown or short skip half is not planned on the schedule (the kernel's prologue wants three skip chunks)
    Tuning all{};
    all.f4_cs = 2;
    CHECK(winograd_plan(64, 32, 32, 768, 256, SRC_UPCAT, all, 256).cs == 1, "up1.conv-0 takes it when forced");
    CHECK(winograd_plan(64, 32, 32, 768, 256, SRC_UPCAT, all).cs == 0 && winograd_plan(64, 32, 32, 768, 256, SRC_UPCAT, all).algo == 4, "unknown Cskip");
    CHECK(winograd_plan(64, 32, 32, 288, 256, SRC_UPCAT, all, 32).cs == 0 && winograd_plan(64, 32, 32, 288, 256, SRC_UPCAT, all, 32).use, "two skip chunks");
    std::printf("plan_coutsplit_host: %d failures\n", fails);
    return fails ? 1 : 0;
}
