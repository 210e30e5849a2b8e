// Stand-alone check of the NUFFT plan builder (csrc/nufft_plan.hip: pure host code, compiled into this program; no GPU, no HIP call).
//   nufft_plan_host            one plan description on stdin: `h w gh gw J M` and M lines `ky kx` (hex floats).  Checks the bins of the
//                              plan - every sample is listed in every tile its periodic footprint meets and in no other, every list is
//                              ascending - and prints, for tests/test_nufft_host.py to compare with the float64 restatement's bits:
//                                  grid gh gw
//                                  s <i0y> <i0x> <2 J weight words, hex>         one line per sample
//                                  cy <H words>      cx <W words>
//   nufft_plan_host --invalid  every invalid argument is refused, with a message, and a valid plan is accepted
// Built plain and with -fsanitize=address,undefined (host) by the test.
#include "../dt4image_restoration_amd/csrc/nufft_plan.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <set>
#include <utility>

using namespace pnp;

static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }

static int check_bins(const NufftPlan& P) {
    const int ntiles = P.tiles_y * P.tiles_x;
    if ((int)P.bin_off.size() != ntiles + 1 || P.bin_off[0] != 0 || (size_t)P.bin_off[ntiles] != P.bin_idx.size()) {
        std::printf("bins: offsets malformed\n");
        return 1;
    }
    std::vector<std::set<int>> want(ntiles);
    for (int64_t s = 0; s < P.m; ++s)
        for (int a = 0; a < P.width; ++a)
            for (int b = 0; b < P.width; ++b) {
                const int gy = ((P.i0[s] + a) % P.gh + P.gh) % P.gh, gx = ((P.i0[P.m + s] + b) % P.gw + P.gw) % P.gw;
                want[(gy / kNufftTile) * P.tiles_x + gx / kNufftTile].insert((int)s);
            }
    for (int t = 0; t < ntiles; ++t) {
        const int b0 = P.bin_off[t], b1 = P.bin_off[t + 1];
        if (b1 < b0) { std::printf("bins: tile %d has a negative length\n", t); return 1; }
        for (int i = b0 + 1; i < b1; ++i)
            if (P.bin_idx[i] <= P.bin_idx[i - 1]) { std::printf("bins: tile %d is not strictly ascending at %d\n", t, i - b0); return 1; }
        const std::set<int> got(P.bin_idx.begin() + b0, P.bin_idx.begin() + b1);
        if (got != want[t]) { std::printf("bins: tile %d lists %zu samples, its footprints give %zu\n", t, got.size(), want[t].size()); return 1; }
    }
    return 0;
}

static int refuse(const char* what, int h, int w, int gh, int gw, int J, const double* traj, int64_t m, NufftPlan* out) {
    std::string why;
    if (plan_nufft(h, w, gh, gw, J, traj, m, out, &why)) { std::printf("NOT refused: %s\n", what); return 1; }
    if (why.empty()) { std::printf("refused without a message: %s\n", what); return 1; }
    std::printf("refused %-28s %s\n", what, why.c_str());
    return 0;
}

static int invalid() {
    NufftPlan P;
    std::vector<double> t = {0.0, 0.0, 0.25, -0.25, -0.5, 0.5};
    int bad = 0;
    bad += refuse("null traj", 64, 64, 80, 80, 6, nullptr, 3, &P);
    bad += refuse("null plan", 64, 64, 80, 80, 6, t.data(), 3, nullptr);
    bad += refuse("m = 0", 64, 64, 80, 80, 6, t.data(), 0, &P);
    bad += refuse("m < 0", 64, 64, 80, 80, 6, t.data(), -1, &P);
    bad += refuse("m > max", 64, 64, 80, 80, 6, t.data(), kNufftMaxSamples + 1, &P);
    for (int J : {0, 2, 3, 5, 7, 10, -6}) bad += refuse("width", 64, 64, 80, 80, J, t.data(), 3, &P);
    bad += refuse("h not a k-space side", 48, 64, 80, 80, 6, t.data(), 3, &P);
    bad += refuse("w not a k-space side", 64, 96, 80, 128, 6, t.data(), 3, &P);
    bad += refuse("gh not a k-space side", 64, 64, 96, 80, 6, t.data(), 3, &P);
    bad += refuse("gw not a k-space side", 64, 64, 80, 100, 6, t.data(), 3, &P);
    bad += refuse("gh negative", 64, 64, -80, 80, 6, t.data(), 3, &P);
    bad += refuse("gh below 1.25 h", 64, 64, 64, 80, 6, t.data(), 3, &P);
    bad += refuse("gw below 1.25 w", 128, 128, 160, 128, 6, t.data(), 3, &P);
    bad += refuse("h = 1024, default grid", 1024, 64, 0, 0, 6, t.data(), 3, &P);
    bad += refuse("w = 1024, default grid", 64, 1024, 0, 0, 6, t.data(), 3, &P);
    bad += refuse("w = 1024, grid 1024", 64, 1024, 80, 1024, 6, t.data(), 3, &P);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (double v : {0.5000001, -0.5000001, 1.0, inf, -inf, nan})
        for (int at = 0; at < 6; ++at) {
            std::vector<double> u = t;
            u[at] = v;
            bad += refuse("coordinate", 64, 64, 80, 80, 6, u.data(), 3, &P);
        }
    std::string why;
    if (!plan_nufft(64, 64, 0, 0, 6, t.data(), 3, &P, &why) || P.gh != 80 || P.gw != 80) { std::printf("valid plan refused: %s\n", why.c_str()); ++bad; }
    if (!plan_nufft(800, 16, 0, 0, 8, t.data(), 3, &P, &why) || P.gh != 1024 || P.gw != 32 || check_bins(P)) { std::printf("800 x 16 refused: %s\n", why.c_str()); ++bad; }
    const int sides[] = {16, 32, 64, 80, 128, 160, 256, 320, 400, 512, 640, 800}, grids[] = {32, 64, 80, 128, 160, 256, 320, 400, 512, 640, 800, 1024};
    for (int i = 0; i < 12; ++i)
        if (nufft_default_grid(sides[i]) != grids[i]) { std::printf("default grid of %d is %d\n", sides[i], nufft_default_grid(sides[i])); ++bad; }
    if (bad) return 1;
    std::printf("nufft_plan_host: invalid ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--invalid") == 0) return invalid();
    int h, w, gh, gw, J;
    long long m;
    if (std::scanf("%d %d %d %d %d %lld", &h, &w, &gh, &gw, &J, &m) != 6 || m < 1 || m > kNufftMaxSamples) { std::fprintf(stderr, "nufft_plan_host: bad header\n"); return 2; }
    std::vector<double> traj(2 * (size_t)m);
    for (double& v : traj)
        if (std::scanf("%la", &v) != 1) { std::fprintf(stderr, "nufft_plan_host: bad coordinate\n"); return 2; }
    NufftPlan P;
    std::string why;
    if (!plan_nufft(h, w, gh, gw, J, traj.data(), m, &P, &why)) { std::printf("refused: %s\n", why.c_str()); return 1; }
    if (check_bins(P)) return 1;
    std::printf("grid %d %d\n", P.gh, P.gw);
    for (int64_t s = 0; s < P.m; ++s) {
        std::printf("s %d %d", P.i0[s], P.i0[P.m + s]);
        for (int j = 0; j < J; ++j) std::printf(" %08x", bits(P.wy(s, j)));
        for (int j = 0; j < J; ++j) std::printf(" %08x", bits(P.wx(s, j)));
        std::printf("\n");
    }
    std::printf("cy");
    for (float c : P.cy) std::printf(" %08x", bits(c));
    std::printf("\ncx");
    for (float c : P.cx) std::printf(" %08x", bits(c));
    std::printf("\nnufft_plan_host: bins ok\n");
    return 0;
}
