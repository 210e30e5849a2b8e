// Stand-alone host program over the pure-host plan code of the off-resonance operator (csrc/offres_plan.hip, include/pnpadmm_offres.h):
// tests/test_offres_host.py compiles it together with that unit, plain and with -fsanitize=address,undefined, and runs it directly.  It has
// its own main, loads nothing into another process and makes no HIP call, so it needs no GPU.
//   --invalid                 every refusal of plan_offres, and that a refused call leaves the output plan untouched
//   --dump IN L OUT           IN:  int64 m, int32 tiles, double t[m], int32 bin_off[tiles + 1], int32 bin_idx[bin_off[tiles]]
//                             OUT: double tau[L], int32 seg[m], float b0[m], float b1[m], int32 list_off[L tiles + 1], int32 list_idx[..]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../dt4image_restoration_amd/csrc/offres_plan.h"

using namespace pnp;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d %s [%s]\n", __FILE__, __LINE__, #cond, why.c_str()); ++fails; } } while (0)

static int invalid() {
    std::string why;
    OffresPlan P;
    P.segments = 77;                                        // a refused call leaves the plan as it was
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    double t[5] = {0.0, 1e-3, 2e-3, 3e-3, 4e-3};
    const int32_t off[3] = {0, 3, 5}, idx[5] = {0, 1, 2, 3, 4};
    const auto says = [&](const char* what) { return why.find(what) != std::string::npos; };
    const int bad_segments[] = {0, -1, 33, std::numeric_limits<int>::min(), std::numeric_limits<int>::max()};
    for (int L : bad_segments) CHECK(!plan_offres(t, 5, L, 0, nullptr, nullptr, &P, &why) && says("segments must be 1..32"));
    CHECK(!plan_offres(t, 0, 2, 0, nullptr, nullptr, &P, &why) && says("m must be"));
    CHECK(!plan_offres(nullptr, 5, 2, 0, nullptr, nullptr, &P, &why) && says("null"));
    CHECK(!plan_offres(t, 5, 2, 0, nullptr, nullptr, nullptr, &why) && says("null"));
    CHECK(!plan_offres(t, 5, 2, 2, nullptr, idx, &P, &why) && says("tiles without bins"));
    CHECK(!plan_offres(t, 5, 2, 2, off, nullptr, &P, &why) && says("tiles without bins"));
    for (double v : {nan, inf, -inf}) {
        double u[5] = {0.0, 1e-3, v, 3e-3, 4e-3};
        for (int L : {1, 2, 32}) CHECK(!plan_offres(u, 5, L, 0, nullptr, nullptr, &P, &why) && says("sample 2") && says("not finite"));
    }
    double big[2] = {-std::numeric_limits<double>::max(), std::numeric_limits<double>::max()};
    CHECK(!plan_offres(big, 2, 2, 0, nullptr, nullptr, &P, &why) && says("span"));
    double same[3] = {2e-3, 2e-3, 2e-3};
    for (int L : {2, 3, 32}) CHECK(!plan_offres(same, 3, L, 0, nullptr, nullptr, &P, &why) && says("positive span"));
    const int32_t bad_idx[5] = {0, 1, 7, 3, 4};
    CHECK(!plan_offres(t, 5, 2, 2, off, bad_idx, &P, &why) && says("names sample"));
    CHECK(P.segments == 77 && P.tau.empty());
    // accepted: L = 1 on a zero span, one sample, and without an error string
    CHECK(plan_offres(same, 3, 1, 0, nullptr, nullptr, &P, &why) && P.segments == 1 && P.tau.size() == 1 && P.tau[0] == 2e-3 && P.b0[2] == 1.f &&
          P.b1[2] == 0.f && P.seg[2] == 0 && P.list_off.empty());
    CHECK(plan_offres(t, 1, 1, 0, nullptr, nullptr, &P, nullptr) && P.m == 1);
    CHECK(!plan_offres(t, 1, 2, 0, nullptr, nullptr, &P, nullptr));
    CHECK(plan_offres(t, 5, 3, 2, off, idx, &P, &why) && P.list_off.size() == 7 && P.list_off[6] == (int32_t)P.list_idx.size());
    CHECK(P.seg[4] == 1 && P.b1[4] == 1.f && P.b0[4] == 0.f && P.seg[2] == 1 && P.b1[2] == 0.f && P.b0[2] == 1.f);   // t_max; a centre
    if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
    std::printf("asan_offres_host: invalid ok\n");
    return 0;
}

template <class T>
static bool read_n(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
template <class T>
static bool write_v(std::FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

static int dump(const char* in, int L, const char* out) {
    std::FILE* f = std::fopen(in, "rb");
    if (!f) { std::printf("cannot open %s\n", in); return 2; }
    int64_t m = 0;
    int32_t tiles = 0;
    std::vector<double> t;
    std::vector<int32_t> off, idx;
    bool ok = std::fread(&m, sizeof m, 1, f) == 1 && std::fread(&tiles, sizeof tiles, 1, f) == 1 && m >= 1 && m <= (1 << 22) && tiles >= 0 &&
              tiles <= (1 << 16) && read_n(f, t, (size_t)m) && read_n(f, off, (size_t)tiles + 1) && off[(size_t)tiles] >= 0 &&
              read_n(f, idx, (size_t)off[(size_t)tiles]);
    std::fclose(f);
    if (!ok) { std::printf("bad input file\n"); return 2; }
    OffresPlan P;
    std::string why;
    if (!plan_offres(t.data(), m, L, tiles, off.data(), idx.data(), &P, &why)) { std::printf("refused: %s\n", why.c_str()); return 3; }
    std::FILE* g = std::fopen(out, "wb");
    if (!g) { std::printf("cannot open %s\n", out); return 2; }
    ok = write_v(g, P.tau) && write_v(g, P.seg) && write_v(g, P.b0) && write_v(g, P.b1) && write_v(g, P.list_off) && write_v(g, P.list_idx);
    std::fclose(g);
    if (!ok) { std::printf("short write\n"); return 2; }
    std::printf("asan_offres_host: dump ok L=%d m=%lld lists=%zu step=%.17g\n", P.segments, (long long)P.m, P.list_idx.size(), P.step);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--invalid")) return invalid();
    if (argc == 5 && !std::strcmp(argv[1], "--dump")) return dump(argv[2], std::atoi(argv[3]), argv[4]);
    std::printf("usage: asan_offres_host --invalid | --dump IN L OUT\n");
    return 2;
}
