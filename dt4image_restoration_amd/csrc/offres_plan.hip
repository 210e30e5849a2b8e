// plan_offres(): see offres_plan.h.  Pure host code; every expression below is float64 and restated operation by operation in
// tests/offres_ref.py, which the CPU suite compares bit for bit.
#include "offres_plan.h"

#include <cmath>
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

bool plan_offres(const double* t, int64_t m, int segments, int tiles, const int32_t* bin_off, const int32_t* bin_idx, OffresPlan* out,
                 std::string* err) {
    if (segments < 1 || segments > kOffresMaxSegments) {
        set_err(err, "segments must be 1..%d (got %d)", kOffresMaxSegments, segments);
        return false;
    }
    if (m < 1) { set_err(err, "m must be >= 1 (got %.0f)", (double)m); return false; }
    if (!t || !out) { set_err(err, "null argument"); return false; }
    if (tiles < 0 || (tiles > 0 && (!bin_off || !bin_idx))) { set_err(err, "tiles without bins"); return false; }
    double lo = t[0], hi = t[0];
    for (int64_t s = 0; s < m; ++s) {
        if (!std::isfinite(t[s])) { set_err(err, "sample %.0f: time %g is not finite", (double)s, t[s]); return false; }
        if (t[s] < lo) lo = t[s];
        if (t[s] > hi) hi = t[s];
    }
    const int L = segments;
    if (!std::isfinite(hi - lo)) { set_err(err, "the span of the times %g .. %g is not finite", lo, hi); return false; }
    if (L > 1 && !(hi > lo)) { set_err(err, "segments = %d needs times of a positive span (all %.0f samples are at %g)", L, (double)m, lo); return false; }

    OffresPlan P;                                           // built aside: a refusal leaves *out as it was
    P.segments = L; P.m = m; P.t_min = lo; P.t_max = hi;
    P.tau.resize((size_t)L);
    P.seg.assign((size_t)m, 0);
    P.b0.assign((size_t)m, 1.f);
    P.b1.assign((size_t)m, 0.f);
    if (L == 1) {
        P.tau[0] = 0.5 * (lo + hi);
    } else {
        const double D = (hi - lo) / (double)(L - 1);
        P.step = D;
        for (int l = 0; l < L; ++l) P.tau[(size_t)l] = lo + (double)l * D;
        for (int64_t s = 0; s < m; ++s) {
            double f = std::floor((t[s] - lo) / D);
            if (f > (double)(L - 2)) f = (double)(L - 2);
            if (f < 0.0) f = 0.0;
            const int sg = (int)f;
            double b = (t[s] - P.tau[(size_t)sg]) / D;
            if (b < 0.0) b = 0.0;
            if (b > 1.0) b = 1.0;
            P.seg[(size_t)s] = sg;
            P.b1[(size_t)s] = (float)b;
            P.b0[(size_t)s] = (float)(1.0 - b);
        }
    }
    if (tiles == 0) { *out = std::move(P); return true; }
    // lists: the tile's bin in its own (ascending) order, kept where the sample carries weight in segment l
    const int64_t total = (int64_t)bin_off[tiles] * (L > 1 ? 2 : 1);
    if (total > (int64_t)INT32_MAX) { set_err(err, "the per-segment sample lists need %.0f entries, more than 2^31 - 1", (double)total); return false; }
    P.list_off.assign((size_t)L * tiles + 1, 0);
    P.list_idx.resize((size_t)total);
    int32_t fill = 0;
    for (int l = 0; l < L; ++l)
        for (int tile = 0; tile < tiles; ++tile) {
            for (int32_t k = bin_off[tile]; k < bin_off[tile + 1]; ++k) {
                const int32_t s = bin_idx[k];
                if (s < 0 || s >= m) { set_err(err, "bin entry %d names sample %d of %.0f", k, s, (double)m); return false; }
                const int sg = P.seg[(size_t)s];
                if (sg == l || (L > 1 && sg == l - 1)) P.list_idx[(size_t)fill++] = s;
            }
            P.list_off[(size_t)l * tiles + tile + 1] = fill;
        }
    P.list_idx.resize((size_t)fill);
    *out = std::move(P);
    return true;
}

}  // namespace pnp
