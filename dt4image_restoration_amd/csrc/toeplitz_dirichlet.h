// The Dirichlet kernel of the Toeplitz spectra (include/pnpadmm_toeplitz.h, include/pnpadmm_offres_tz.h): one definition for the two units that
// sum spectra, toeplitz_kernels.hip and offres_tz_kernels.hip, which include it after switching contraction off.
#pragma once
#include <hip/hip_runtime.h>

namespace pnp {

// D_n(t) = sin((2n - 1) pi t) / sin(pi t), t reduced to [-0.5, 0.5] first; 2n - 1 at t == 0.  The rounding error of the product (2n - 1) t,
// up to 2^-44 of a period at n = 512, is put back to first order
__device__ __forceinline__ double dirichlet(double t, int n) {
    t = t - rint(t);
    if (t == 0.0) return (double)(2 * n - 1);
    const double a = (double)(2 * n - 1);
    const double hi = a * t, lo = fma(a, t, -hi);
    double sn, cs;
    sincospi(hi, &sn, &cs);
    return fma(3.14159265358979323846 * lo, cs, sn) / sinpi(t);
}

}  // namespace pnp
