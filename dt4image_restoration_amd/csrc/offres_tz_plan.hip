// plan_offres_tz(): see offres_tz_plan.h.  Pure host code.
#include "offres_tz_plan.h"

#include <cstdarg>
#include <cstdio>
#include <utility>

namespace pnp {

namespace {

void set_err(std::string* err, const char* fmt, ...) {
    if (!err) return;
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    *err = buf;
}

}  // namespace

int offres_tz_pairs(int kind, int segments) {
    if (segments < 1) return 0;
    return kind == 1 ? 2 * segments - 1 : (kind == 2 ? segments * (segments + 1) / 2 : 0);
}

bool plan_offres_tz(int kind, int segments, int64_t m, const int32_t* seg, OffresTzPlan* out, std::string* err) {
    if (kind != 1 && kind != 2) { set_err(err, "no off-resonance plan (kind %d)", kind); return false; }
    if (segments < 1) { set_err(err, "segments must be >= 1 (got %d)", segments); return false; }
    const int L = segments, pairs = offres_tz_pairs(kind, L);
    if (pairs > kOffresTzMaxPairs) {
        set_err(err, "%d segments under a %s plan need %d spectra, more than the limit of %d (16 segments least squares, 32 linear)", L,
                kind == 1 ? "linear" : "least-squares", pairs, kOffresTzMaxPairs);
        return false;
    }
    if (m < 1) { set_err(err, "m must be >= 1 (got %.0f)", (double)m); return false; }
    if (!out || (kind == 1 && !seg)) { set_err(err, "null argument"); return false; }

    OffresTzPlan P;                                         // built aside: a refusal leaves *out as it was
    P.kind = kind; P.segments = L; P.pairs = pairs;
    P.pair_block = kind == 1 ? kOffresTzBlockLinear : kOffresTzBlockDense;
    P.blocks = (pairs + P.pair_block - 1) / P.pair_block;
    P.left.reserve((size_t)pairs); P.right.reserve((size_t)pairs);
    if (kind == 2) {
        for (int l = 0; l < L; ++l)
            for (int r = l; r < L; ++r) { P.left.push_back(l); P.right.push_back(r); }
        *out = std::move(P);
        return true;
    }
    for (int l = 0; l < L; ++l) {
        P.left.push_back(l); P.right.push_back(l);
        if (l + 1 < L) { P.left.push_back(l); P.right.push_back(l + 1); }
    }
    // block l = the pairs (l, l) and (l, l + 1): its samples are those of segments l - 1 (b1 b1 into (l, l)) and l, in ascending order
    std::vector<int64_t> count((size_t)L + 1, 0);
    for (int64_t s = 0; s < m; ++s) {
        const int sg = seg[s];
        if (sg < 0 || sg >= L || (L > 1 && sg > L - 2)) { set_err(err, "sample %.0f lies in segment %d of %d", (double)s, sg, L); return false; }
        ++count[(size_t)sg];
    }
    int64_t total = 0;
    for (int l = 0; l < L; ++l) total += count[(size_t)l] + (l > 0 ? count[(size_t)l - 1] : 0);
    if (total > (int64_t)INT32_MAX) { set_err(err, "the per-pair sample lists need %.0f entries, more than 2^31 - 1", (double)total); return false; }
    P.blk_off.assign((size_t)L + 1, 0);
    for (int l = 0; l < L; ++l) P.blk_off[(size_t)l + 1] = P.blk_off[(size_t)l] + (int32_t)(count[(size_t)l] + (l > 0 ? count[(size_t)l - 1] : 0));
    P.blk_idx.resize((size_t)total);
    std::vector<int32_t> fill(P.blk_off.begin(), P.blk_off.end() - 1);
    for (int64_t s = 0; s < m; ++s) {                       // ascending s: every list comes out ascending
        const int sg = seg[s];
        P.blk_idx[(size_t)fill[(size_t)sg]++] = (int32_t)s;
        if (sg + 1 < L) P.blk_idx[(size_t)fill[(size_t)sg + 1]++] = (int32_t)s;
    }
    *out = std::move(P);
    return true;
}

}  // namespace pnp
