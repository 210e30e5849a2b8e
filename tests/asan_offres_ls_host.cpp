// Stand-alone host program over the pure-host plan code of the least-squares temporal interpolator (csrc/offres_ls_plan.hip,
// include/pnpadmm_offres_ls.h): tests/test_offres_ls_host.py compiles it together with that unit, plain and with
// -fsanitize=address,undefined, and runs it directly.  It has its own main, loads nothing into another process and makes no HIP call, so it
// needs no GPU.
//   --invalid                     every refusal of plan_offres_ls, and that a refused call leaves the output plan untouched
//   --dump IN L OMEGA_MAX OUT     IN:  int64 m, double t[m]      OUT: double tau[L], float coef[L][m]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../dt4image_restoration_amd/csrc/offres_ls_plan.h"

using namespace pnp;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d %s [%s]\n", __FILE__, __LINE__, #cond, why.c_str()); ++fails; } } while (0)

static int invalid() {
    std::string why;
    OffresLsPlan P;
    P.segments = 77;                                        // a refused call leaves the plan as it was
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    double t[5] = {0.0, 1e-3, 2e-3, 3e-3, 4e-3};
    const double om = 2.0 * 3.14159265358979323846 * 100.0;
    const auto says = [&](const char* what) { return why.find(what) != std::string::npos; };
    const int bad_segments[] = {0, -1, 33, std::numeric_limits<int>::min(), std::numeric_limits<int>::max()};
    for (int L : bad_segments) CHECK(!plan_offres_ls(t, 5, L, om, &P, &why) && says("segments must be 1..32"));
    CHECK(!plan_offres_ls(t, 0, 2, om, &P, &why) && says("m must be"));
    CHECK(!plan_offres_ls(nullptr, 5, 2, om, &P, &why) && says("null"));
    CHECK(!plan_offres_ls(t, 5, 2, om, nullptr, &why) && says("null"));
    for (double v : {nan, inf, -inf, 0.0, -1.0}) {
        for (int L : {2, 8, 32}) CHECK(!plan_offres_ls(t, 5, L, v, &P, &why) && says("omega_max"));
        CHECK(plan_offres_ls(t, 5, 1, v, &P, nullptr));      // one centre does not read the band
        P = OffresLsPlan();
        P.segments = 77;
    }
    for (double v : {nan, inf, -inf}) {
        double u[5] = {0.0, 1e-3, v, 3e-3, 4e-3};
        for (int L : {1, 2, 32}) CHECK(!plan_offres_ls(u, 5, L, om, &P, &why) && says("sample 2") && says("not finite"));
    }
    double big[2] = {-std::numeric_limits<double>::max(), std::numeric_limits<double>::max()};
    CHECK(!plan_offres_ls(big, 2, 2, om, &P, &why) && says("span"));
    double same[3] = {2e-3, 2e-3, 2e-3};
    for (int L : {2, 3, 32}) CHECK(!plan_offres_ls(same, 3, L, om, &P, &why) && says("positive span"));
    CHECK(P.segments == 77 && P.tau.empty() && P.coef.empty());
    // accepted: L = 1 on a zero span, one sample, and without an error string
    CHECK(plan_offres_ls(same, 3, 1, om, &P, &why) && P.segments == 1 && P.tau.size() == 1 && P.tau[0] == 2e-3 && P.coef.size() == 3 &&
          P.coef[0] == 1.f && P.coef[2] == 1.f && P.omega_max == 0.0);
    CHECK(plan_offres_ls(t, 1, 1, om, &P, nullptr) && P.m == 1);
    CHECK(!plan_offres_ls(t, 1, 2, om, &P, nullptr));
    // a sample on a centre: the fit interpolates it to within the ridge; every coefficient finite
    CHECK(plan_offres_ls(t, 5, 3, om, &P, &why) && P.coef.size() == 15 && P.tau[1] == 2e-3 && P.step == 2e-3 && P.omega_max == om);
    CHECK(std::fabs(P.coef[1 * 5 + 2] - 1.f) < 1e-6f && std::fabs(P.coef[0 * 5 + 2]) < 1e-6f && std::fabs(P.coef[2 * 5 + 2]) < 1e-6f);
    bool finite = true;
    for (float c : P.coef) finite = finite && std::isfinite(c);
    CHECK(finite);
    // the widest plan on a tiny band: the pivots stay positive thanks to the ridge, or the failure is reported - never a NaN
    {
        std::vector<double> u(257);
        for (size_t i = 0; i < u.size(); ++i) u[i] = 1e-2 * (double)i / 256.0;
        for (double band : {1e-3, 1.0, 2.0 * 3.14159265358979323846 * 100.0, 6.0 * 3.14159265358979323846 * 100.0}) {
            OffresLsPlan Q;
            const bool ok = plan_offres_ls(u.data(), (int64_t)u.size(), 32, band, &Q, &why);
            bool fin = true;
            for (float c : Q.coef) fin = fin && std::isfinite(c);
            CHECK((ok && fin && Q.coef.size() == 32 * u.size()) || (!ok && says("pivot") && Q.coef.empty()));
        }
    }
    if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
    std::printf("asan_offres_ls_host: invalid ok\n");
    return 0;
}

static int dump(const char* in, int L, double omega_max, const char* out) {
    std::FILE* f = std::fopen(in, "rb");
    if (!f) { std::printf("cannot open %s\n", in); return 2; }
    int64_t m = 0;
    std::vector<double> t;
    bool ok = std::fread(&m, sizeof m, 1, f) == 1 && m >= 1 && m <= (1 << 22);
    if (ok) {
        t.resize((size_t)m);
        ok = std::fread(t.data(), sizeof(double), (size_t)m, f) == (size_t)m;
    }
    std::fclose(f);
    if (!ok) { std::printf("bad input file\n"); return 2; }
    OffresLsPlan P;
    std::string why;
    if (!plan_offres_ls(t.data(), m, L, omega_max, &P, &why)) { std::printf("refused: %s\n", why.c_str()); return 3; }
    std::FILE* g = std::fopen(out, "wb");
    if (!g) { std::printf("cannot open %s\n", out); return 2; }
    ok = std::fwrite(P.tau.data(), sizeof(double), P.tau.size(), g) == P.tau.size() &&
         std::fwrite(P.coef.data(), sizeof(float), P.coef.size(), g) == P.coef.size();
    std::fclose(g);
    if (!ok) { std::printf("short write\n"); return 2; }
    std::printf("asan_offres_ls_host: dump ok L=%d m=%lld step=%.17g omega_max=%.17g ridge=%g\n", P.segments, (long long)P.m, P.step, P.omega_max,
                kOffresLsRidge);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--invalid")) return invalid();
    if (argc == 6 && !std::strcmp(argv[1], "--dump")) return dump(argv[2], std::atoi(argv[3]), std::atof(argv[4]), argv[5]);
    std::printf("usage: asan_offres_ls_host --invalid | --dump IN L OMEGA_MAX OUT\n");
    return 2;
}
