// plan_offres_ls(): see offres_ls_plan.h.  Pure host code; every expression below is float64 and restated in tests/offres_ls_ref.py.
#include "offres_ls_plan.h"

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

double sinc(double x) { return x == 0.0 ? 1.0 : std::sin(x) / x; }

}  // namespace

bool plan_offres_ls(const double* t, int64_t m, int segments, double omega_max, OffresLsPlan* out, std::string* err) {
    if (segments < 1 || segments > kOffresMaxSegments) {
        set_err(err, "segments must be 1..%d (got %d)", kOffresMaxSegments, segments);
        return false;
    }
    if (m < 1) { set_err(err, "m must be >= 1 (got %.0f)", (double)m); return false; }
    if (!t || !out) { set_err(err, "null argument"); return false; }
    const int L = segments;
    if (L > 1 && (!std::isfinite(omega_max) || !(omega_max > 0.0))) {
        set_err(err, "segments = %d needs a finite omega_max > 0 (got %g)", L, omega_max);
        return false;
    }
    double lo = t[0], hi = t[0];
    for (int64_t s = 0; s < m; ++s) {
        if (!std::isfinite(t[s])) { set_err(err, "sample %.0f: time %g is not finite", (double)s, t[s]); return false; }
        if (t[s] < lo) lo = t[s];
        if (t[s] > hi) hi = t[s];
    }
    if (!std::isfinite(hi - lo)) { set_err(err, "the span of the times %g .. %g is not finite", lo, hi); return false; }
    if (L > 1 && !(hi > lo)) { set_err(err, "segments = %d needs times of a positive span (all %.0f samples are at %g)", L, (double)m, lo); return false; }

    OffresLsPlan P;                                         // built aside: a refusal leaves *out as it was
    P.segments = L; P.m = m; P.t_min = lo; P.t_max = hi;
    P.tau.resize((size_t)L);
    P.coef.assign((size_t)L * (size_t)m, 1.f);
    if (L == 1) {
        P.tau[0] = 0.5 * (lo + hi);
        *out = std::move(P);
        return true;
    }
    const double D = (hi - lo) / (double)(L - 1);
    P.step = D;
    P.omega_max = omega_max;
    for (int l = 0; l < L; ++l) P.tau[(size_t)l] = lo + (double)l * D;
    // C C^T = G, C lower triangular, row by row
    double C[kOffresMaxSegments][kOffresMaxSegments];
    for (int i = 0; i < L; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = sinc(omega_max * (P.tau[(size_t)i] - P.tau[(size_t)j])) + (i == j ? kOffresLsRidge : 0.0);
            for (int k = 0; k < j; ++k) s -= C[i][k] * C[j][k];
            if (i == j) {
                if (!(s > 0.0) || !std::isfinite(s)) {
                    set_err(err, "pivot %d of the Cholesky factor of G is %g: omega_max span = %g is too small for %d segments", i, s,
                            omega_max * (hi - lo), L);
                    return false;
                }
                C[i][i] = std::sqrt(s);
            } else {
                C[i][j] = s / C[j][j];
            }
        }
    double r[kOffresMaxSegments];
    for (int64_t s = 0; s < m; ++s) {
        for (int l = 0; l < L; ++l) r[l] = sinc(omega_max * (t[s] - P.tau[(size_t)l]));
        for (int i = 0; i < L; ++i) {                       // C z = r
            double v = r[i];
            for (int k = 0; k < i; ++k) v -= C[i][k] * r[k];
            r[i] = v / C[i][i];
        }
        for (int i = L - 1; i >= 0; --i) {                  // C^T b = z
            double v = r[i];
            for (int k = i + 1; k < L; ++k) v -= C[k][i] * r[k];
            r[i] = v / C[i][i];
        }
        for (int l = 0; l < L; ++l) {
            if (!std::isfinite(r[l])) { set_err(err, "sample %.0f: coefficient %d is not finite", (double)s, l); return false; }
            P.coef[(size_t)l * (size_t)m + (size_t)s] = (float)r[l];
        }
    }
    *out = std::move(P);
    return true;
}

}  // namespace pnp
