// plan_nufft(): the host half of the non-Cartesian operator pair (nufft_plan.h).  Pure host code: no HIP call, no HIP header.
// Every float32 the kernels read is formed here in float64 and rounded once; the expressions are written out operation by operation, with
// contraction off, so that a float64 restatement of them (tests/nufft_ref.py) rounds the same values.
#include "nufft_plan.h"

#include <cmath>
#include <cstdio>

#pragma clang fp contract(off)

namespace pnp {

namespace {

void set_err(std::string* err, const char* fmt, double a = 0, double b = 0, double c = 0, double d = 0) {
    if (!err) return;
    char buf[256];
    std::snprintf(buf, sizeof buf, fmt, a, b, c, d);
    *err = buf;
}

// Gauss-Legendre nodes and weights on [-1, 1] (Newton on P_n from the Chebyshev guess; symmetric pairs)
void gauss_legendre(int n, double* x, double* w) {
    for (int i = 0; i < (n + 1) / 2; ++i) {
        double z = std::cos(M_PI * (i + 0.75) / (n + 0.5)), pp = 1.0;
        for (int it = 0; it < 100; ++it) {
            double p1 = 1.0, p2 = 0.0;
            for (int j = 1; j <= n; ++j) {
                const double p3 = p2;
                p2 = p1;
                p1 = ((2.0 * j - 1.0) * z * p2 - (j - 1.0) * p3) / j;
            }
            pp = n * (z * p1 - p2) / (z * z - 1.0);
            const double dz = p1 / pp;
            z -= dz;
            if (std::fabs(dz) < 1e-16) break;
        }
        x[i] = -z; x[n - 1 - i] = z;
        w[i] = w[n - 1 - i] = 2.0 / ((1.0 - z * z) * pp * pp);
    }
}

inline int floor_mod(int a, int g) { const int r = a % g; return r < 0 ? r + g : r; }

}  // namespace

bool nufft_side_ok(int L) {
    if (L < 16 || L > 1024 || L % 16) return false;
    while (L % 2 == 0) L /= 2;
    while (L % 5 == 0) L /= 5;
    return L == 1;
}

int nufft_default_grid(int side) {
    for (int g = 16; g <= 1024; g += 16)
        if (nufft_side_ok(g) && 4 * g >= 5 * side) return g;
    return 0;
}

double nufft_beta(int width, int g, int side) {
    if (g == 2 * side) return 2.30 * width;
    return 0.97 * M_PI * width * (1.0 - (double)side / (2.0 * g));
}

double nufft_phi(double t, int width, double beta) {
    const double z = 2.0 * t / width;
    if (!(std::fabs(z) < 1.0)) return 0.0;
    const double a = 1.0 - z * z;
    return std::exp(beta * (std::sqrt(a) - 1.0));
}

double nufft_phihat(int q, int width, int g, double beta) {
    static double gx[kNufftQuadNodes], gwt[kNufftQuadNodes];
    static const bool ready = (gauss_legendre(kNufftQuadNodes, gx, gwt), true);
    (void)ready;
    const double half = 0.25 * width;                      // [0, J/2] = half (x + 1)
    double sum = 0.0;
    for (int i = 0; i < kNufftQuadNodes; ++i) {
        const double t = half * (gx[i] + 1.0);
        sum += gwt[i] * nufft_phi(t, width, beta) * std::cos(2.0 * M_PI * q * t / g);
    }
    return 2.0 * half * sum;
}

bool plan_nufft(int h, int w, int gh, int gw, int width, const double* traj, int64_t m, NufftPlan* out, std::string* err) {
    if (!traj || !out) { set_err(err, "null trajectory or plan"); return false; }
    if (m < 1 || m > kNufftMaxSamples) { set_err(err, "m must be 1..%.0f (got %.0f)", (double)kNufftMaxSamples, (double)m); return false; }
    if (width != 4 && width != 6 && width != 8) { set_err(err, "width must be 4, 6 or 8 (got %.0f)", width); return false; }
    if (!nufft_side_ok(h) || !nufft_side_ok(w)) { set_err(err, "h, w must be sides the k-space stage accepts (got %.0fx%.0f)", h, w); return false; }
    if (gh < 0 || gw < 0) { set_err(err, "gh, gw must be 0 or a grid side (got %.0fx%.0f)", gh, gw); return false; }
    if (gh == 0) gh = nufft_default_grid(h);
    if (gw == 0) gw = nufft_default_grid(w);
    if (gh == 0 || gw == 0) {
        set_err(err, "a %.0fx%.0f image has no 1.25x grid: the largest side the k-space stage accepts is 1024, so h, w <= 800", h, w);
        return false;
    }
    if (!nufft_side_ok(gh) || !nufft_side_ok(gw)) {
        set_err(err, "gh, gw must be sides the k-space stage accepts (got %.0fx%.0f)", gh, gw);
        return false;
    }
    if (4 * gh < 5 * h || 4 * gw < 5 * w) {
        set_err(err, "the grid must be oversampled by 1.25 or more: 4 gh >= 5 h and 4 gw >= 5 w (got %.0fx%.0f for %.0fx%.0f)", gh, gw, h, w);
        return false;
    }
    for (int64_t s = 0; s < m; ++s)
        for (int a = 0; a < 2; ++a) {
            const double k = traj[2 * s + a];
            if (!std::isfinite(k) || k < -0.5 || k > 0.5) {
                set_err(err, "sample %.0f: coordinate %.0f = %g is not in [-0.5, 0.5]", (double)s, a, k);
                return false;
            }
        }

    NufftPlan& P = *out;
    P = NufftPlan();
    P.h = h; P.w = w; P.gh = gh; P.gw = gw; P.width = width; P.m = m;
    P.tiles_y = gh / kNufftTile; P.tiles_x = gw / kNufftTile;
    const int J = width;
    P.i0.resize(2 * (size_t)m);
    P.wts.resize(2 * (size_t)J * m);
    const double beta[2] = {nufft_beta(J, gh, h), nufft_beta(J, gw, w)};
    const int g2[2] = {gh, gw};
    for (int64_t s = 0; s < m; ++s)
        for (int a = 0; a < 2; ++a) {
            const double kg = traj[2 * s + a] * g2[a];
            const double u = kg + 0.5 * g2[a];
            const int i0 = (int)std::ceil(u - 0.5 * J);
            P.i0[(size_t)a * m + s] = i0;
            for (int j = 0; j < J; ++j) {
                const double t = u - (double)(i0 + j);
                P.wts[(size_t)(a * J + j) * m + s] = (float)nufft_phi(t, J, beta[a]);
            }
        }
    // deconvolution: 1 / phihat with the scale between the grid's orthonormal transform and 1 / sqrt(h w) folded in, per axis
    const int side[2] = {h, w};
    for (int a = 0; a < 2; ++a) {
        std::vector<float>& c = a ? P.cx : P.cy;
        c.resize(side[a]);
        const double scale = std::sqrt((double)g2[a] / (double)side[a]);
        for (int i = 0; i < side[a]; ++i) c[i] = (float)(scale / nufft_phihat(i - side[a] / 2, J, g2[a], beta[a]));
    }
    // bins: a footprint of J <= kNufftTile points meets one or two tiles per axis (the second through the periodic wrap at the grid's edge too)
    const int ntiles = P.tiles_y * P.tiles_x;
    P.bin_off.assign((size_t)ntiles + 1, 0);
    auto tiles_of = [&](int64_t s, int a, int t[2]) {
        const int i0 = P.i0[(size_t)a * m + s];
        t[0] = floor_mod(i0, g2[a]) / kNufftTile;
        t[1] = floor_mod(i0 + J - 1, g2[a]) / kNufftTile;
        return t[0] == t[1] ? 1 : 2;
    };
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<int32_t> fill;
        if (pass == 1) {
            for (int t = 0; t < ntiles; ++t) P.bin_off[t + 1] += P.bin_off[t];
            P.bin_idx.resize((size_t)P.bin_off[ntiles]);
            fill.assign(P.bin_off.begin(), P.bin_off.end() - 1);
        }
        for (int64_t s = 0; s < m; ++s) {
            int ty[2], tx[2];
            const int ny = tiles_of(s, 0, ty), nx = tiles_of(s, 1, tx);
            for (int a = 0; a < ny; ++a)
                for (int b = 0; b < nx; ++b) {
                    const int t = ty[a] * P.tiles_x + tx[b];
                    if (pass == 0) ++P.bin_off[t + 1];
                    else P.bin_idx[(size_t)fill[t]++] = (int32_t)s;
                }
        }
    }
    return true;
}

}  // namespace pnp
