// Stand-alone host program over the pure-host pair plan of the off-resonance operator's Toeplitz form (csrc/offres_tz_plan.hip,
// include/pnpadmm_offres_tz.h): tests/test_offres_tz_host.py compiles it together with that unit, plain and with
// -fsanitize=address,undefined, and runs it directly.  It has its own main, loads nothing into another process and makes no HIP call, so it
// needs no GPU.
//   --invalid                 every refusal of plan_offres_tz, and that a refused call leaves the output plan untouched
//   --dump IN KIND L OUT      IN:  int64 m, int32 seg[m]
//                             OUT: int32 pairs, pair_block, blocks, n_off, left[pairs], right[pairs], blk_off[n_off], blk_idx[..]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../dt4image_restoration_amd/csrc/offres_tz_plan.h"

using namespace pnp;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d %s [%s]\n", __FILE__, __LINE__, #cond, why.c_str()); ++fails; } } while (0)

static int invalid() {
    std::string why;
    OffresTzPlan P;
    P.segments = 77;                                        // a refused call leaves the plan as it was
    const int32_t seg[5] = {0, 1, 0, 1, 1};
    const auto says = [&](const char* what) { return why.find(what) != std::string::npos; };
    CHECK(!plan_offres_tz(0, 3, 5, seg, &P, &why) && says("no off-resonance plan"));
    CHECK(!plan_offres_tz(3, 3, 5, seg, &P, &why) && says("no off-resonance plan"));
    const int bad_segments[] = {0, -1, std::numeric_limits<int>::min()};
    for (int L : bad_segments) CHECK(!plan_offres_tz(1, L, 5, seg, &P, &why) && says("segments must be"));
    for (int L : {17, 18, 32}) CHECK(!plan_offres_tz(2, L, 5, nullptr, &P, &why) && says("more than the limit of 136") && says("least-squares"));
    CHECK(!plan_offres_tz(1, 69, 5, seg, &P, &why) && says("more than the limit of 136") && says("linear"));
    CHECK(!plan_offres_tz(1, 3, 0, seg, &P, &why) && says("m must be"));
    CHECK(!plan_offres_tz(1, 3, 5, nullptr, &P, &why) && says("null"));
    CHECK(!plan_offres_tz(1, 3, 5, seg, nullptr, &why) && says("null"));
    const int32_t bad_seg[5] = {0, 1, 2, 1, 0};             // segment L - 1 holds no sample of a linear plan
    CHECK(!plan_offres_tz(1, 3, 5, bad_seg, &P, &why) && says("sample 2"));
    const int32_t neg_seg[5] = {0, -1, 0, 1, 0};
    CHECK(!plan_offres_tz(1, 3, 5, neg_seg, &P, &why) && says("sample 1"));
    CHECK(P.segments == 77 && P.left.empty());
    // accepted: the limits themselves, one segment, and without an error string
    CHECK(plan_offres_tz(2, 16, 5, nullptr, &P, &why) && P.pairs == 136 && P.blocks == 34 && P.blk_off.empty() && P.left[16] == 1 && P.right[16] == 1);
    const int32_t zeros[5] = {0, 0, 0, 0, 0};
    CHECK(plan_offres_tz(1, 1, 5, zeros, &P, nullptr) && P.pairs == 1 && P.blocks == 1 && P.blk_off.size() == 2 && P.blk_off[1] == 5);
    CHECK(plan_offres_tz(1, 3, 5, seg, &P, &why) && P.pairs == 5 && P.blocks == 3 && P.blk_off[3] == (int32_t)P.blk_idx.size() && P.blk_idx.size() == 10);
    CHECK(P.blk_off[1] == 2 && P.blk_off[2] == 7 && P.blk_idx[0] == 0 && P.blk_idx[1] == 2 && P.blk_idx[2] == 0 && P.blk_idx[6] == 4);
    if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
    std::printf("asan_offres_tz_host: invalid ok\n");
    return 0;
}

template <class T>
static bool write_v(std::FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

static int dump(const char* in, int kind, int L, const char* out) {
    std::FILE* f = std::fopen(in, "rb");
    if (!f) { std::printf("cannot open %s\n", in); return 2; }
    int64_t m = 0;
    std::vector<int32_t> seg;
    bool ok = std::fread(&m, sizeof m, 1, f) == 1 && m >= 1 && m <= (1 << 22);
    if (ok) {
        seg.resize((size_t)m);
        ok = std::fread(seg.data(), sizeof(int32_t), (size_t)m, f) == (size_t)m;
    }
    std::fclose(f);
    if (!ok) { std::printf("bad input file\n"); return 2; }
    OffresTzPlan P;
    std::string why;
    if (!plan_offres_tz(kind, L, m, seg.data(), &P, &why)) { std::printf("refused: %s\n", why.c_str()); return 3; }
    std::FILE* g = std::fopen(out, "wb");
    if (!g) { std::printf("cannot open %s\n", out); return 2; }
    const std::vector<int32_t> head = {P.pairs, P.pair_block, P.blocks, (int32_t)P.blk_off.size()};
    ok = write_v(g, head) && write_v(g, P.left) && write_v(g, P.right) && write_v(g, P.blk_off) && write_v(g, P.blk_idx);
    std::fclose(g);
    if (!ok) { std::printf("short write\n"); return 2; }
    std::printf("asan_offres_tz_host: dump ok kind=%d L=%d pairs=%d lists=%zu\n", P.kind, P.segments, P.pairs, P.blk_idx.size());
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--invalid")) return invalid();
    if (argc == 6 && !std::strcmp(argv[1], "--dump")) return dump(argv[2], std::atoi(argv[3]), std::atoi(argv[4]), argv[5]);
    std::printf("usage: asan_offres_tz_host --invalid | --dump IN KIND L OUT\n");
    return 2;
}
