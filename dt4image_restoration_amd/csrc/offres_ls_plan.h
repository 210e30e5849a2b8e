// The plan of the least-squares temporal interpolator of include/pnpadmm_offres_ls.h (Sutton, Noll, Fessler 2003): the segment centres of
// plan_offres() and, per sample, one float32 coefficient for EVERY segment, chosen so that sum_l b_l(t) exp(-i omega tau_l) fits
// exp(-i omega t) in the least-squares sense over the band |omega| <= omega_max.  For a symmetric band the normal equations are real:
//     G[l][l'] = sinc(omega_max (tau_l - tau_l')) + kOffresLsRidge [l == l'],   r_l(t) = sinc(omega_max (t - tau_l)),   b(t) = G^-1 r(t)
// with sinc(x) = sin(x) / x and sinc(0) = 1 exactly.  G, its Cholesky factor and the two triangular solves per sample are float64; the
// coefficients are rounded once, to float32.  plan_offres_ls() is pure host code (no HIP call, no HIP header), so the plan a handle uploads
// is the plan the CPU suite checks (tests/asan_offres_ls_host.cpp); pnp_capi.hip uploads it and offres_ls_kernels.hip reads it.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

#include "offres_plan.h"

namespace pnp {

// The ridge added to the diagonal of G.  G is ill-conditioned by design (the centres oversample the band); 1e-10 keeps its float64 Cholesky
// factor positive for every L <= kOffresMaxSegments at the cost of a fit error far below float32's rounding.  Not an argument.
static constexpr double kOffresLsRidge = 1e-10;

struct OffresLsPlan {
    int segments = 0;                                  // L
    int64_t m = 0;                                     // samples
    double t_min = 0.0, t_max = 0.0, step = 0.0;       // as OffresPlan's
    double omega_max = 0.0;                            // the band's edge in rad/s; 0 for L == 1 (unused)
    std::vector<double> tau;                           // [L]: exactly plan_offres' centres
    std::vector<float> coef;                           // [L][M] segment-major: coef[l M + m] = float32(b_l(t_m)); L == 1: all 1
};

// t: [M] seconds.  false: refused, `err` says why and *out is as it was.  Refused: segments outside 1..kOffresMaxSegments, a time that is not
// finite, a zero span with L > 1, omega_max not finite or <= 0 with L > 1, a pivot of the Cholesky factor that is not positive and finite.
bool plan_offres_ls(const double* t, int64_t m, int segments, double omega_max, OffresLsPlan* out, std::string* err);

}  // namespace pnp
