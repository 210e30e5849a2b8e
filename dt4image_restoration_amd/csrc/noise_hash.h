// The counter-hash Gaussian of the simulated acquisitions (pnp_acquire, pnp_acquire_mc, pnp_acquire_nc): synthetic._gauss over
// weights.hash_uniform, number for number.  The integer hash is exact; Box-Muller is float64.
#pragma once
#include <hip/hip_runtime.h>

namespace pnp {

constexpr unsigned kNoiseStreamRe = 9001u, kNoiseStreamIm = 9003u;   // synthetic.make_problem: _gauss(s, 9001, .), _gauss(s, 9003, .)

// weights._splitmix64
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// (hash_uniform(seed, stream, .)[i] + 1) / 2 in float64: the 24 top bits of the hash, exactly
__device__ __forceinline__ double hash_u01(unsigned long long base, unsigned long long i) {
    return (double)(splitmix64(i ^ base) >> 40) * (1.0 / 16777216.0);
}
// synthetic._gauss(seed, stream, .)[i]; b1 / b2 = the stream bases of `stream` and `stream + 1`
__device__ __forceinline__ double gauss64(unsigned long long b1, unsigned long long b2, unsigned long long i) {
    double u1 = hash_u01(b1, i);
    const double u2 = hash_u01(b2, i);
    u1 = u1 > 0x1p-25 ? u1 : 0x1p-25;
    return sqrt(-2.0 * log(u1)) * cos((2.0 * 3.14159265358979323846) * u2);
}

}  // namespace pnp
