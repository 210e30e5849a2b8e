// Complex helpers shared by the k-space kernels (fft_kernels.hip: power-of-two lengths; fft_mixed_kernels.hip: 2^a * 5^b).
#pragma once
#include <hip/hip_runtime.h>

namespace pnp {

// (explicit fused form: `a.x * b.x - a.y * b.y` has two legal contractions with different roundings, and hipcc has picked different ones for the
// same pass body inlined into two kernels - every kernel that runs a pass must round it the same way, so the form is fixed here)
__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
    return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

template <bool INV>
__device__ __forceinline__ void dft4_inplace(float2& a, float2& b, float2& c, float2& d) {
    const float2 t0 = cadd(a, c), t1 = csub(a, c), t2 = cadd(b, d), e = csub(b, d);
    const float2 t3 = INV ? make_float2(-e.y, e.x) : make_float2(e.y, -e.x);        // (+/- i) * (b - d)
    a = cadd(t0, t2); b = cadd(t1, t3); c = csub(t0, t2); d = csub(t1, t3);
}

}  // namespace pnp
