// The plan of the time-segmented off-resonance operator of include/pnpadmm_offres.h: the segment centres, per sample its segment and the two
// float32 weights of the linear temporal interpolator, and for the gridding kernel the CSR list, per (segment, tile), of the samples of the
// tile's bin that carry weight in that segment.  plan_offres() is pure host code (no HIP call, no HIP header), so the plan a handle uploads
// is the plan the CPU suite checks (tests/asan_offres_host.cpp); pnp_capi.hip uploads it and offres_kernels.hip reads it.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

namespace pnp {

static constexpr int kOffresMaxSegments = 32;          // (PNP_MC_MAX_COILS: asserted equal in pnp_capi.hip)

struct OffresPlan {
    int segments = 0;                                  // L
    int64_t m = 0;                                     // samples
    double t_min = 0.0, t_max = 0.0, step = 0.0;       // D = (t_max - t_min) / (L - 1); 0 for L == 1
    std::vector<double> tau;                           // [L]: t_min + l D; L == 1: (t_min + t_max) / 2
    std::vector<int32_t> seg;                          // [M]: min(floor((t - t_min) / D), L - 2); L == 1: 0
    std::vector<float> b0, b1;                         // [M]: b1 = float32(b), b0 = float32(1 - b), b = clamp((t - tau_seg) / D, 0, 1) in float64
    std::vector<int32_t> list_off;                     // [L tiles + 1], row l tiles + tile; empty when no bins were given
    std::vector<int32_t> list_idx;                     // ascending sample indices: the tile's bin filtered to seg_m in {l - 1, l}
};

// t: [M] seconds.  bin_off [tiles + 1] / bin_idx: the NUFFT plan's tile bins, or tiles == 0: no lists are built.  false: refused, `err` says why.
bool plan_offres(const double* t, int64_t m, int segments, int tiles, const int32_t* bin_off, const int32_t* bin_idx, OffresPlan* out,
                 std::string* err);

}  // namespace pnp
