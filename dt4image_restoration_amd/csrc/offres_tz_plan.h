// The pair plan of the Toeplitz form of the off-resonance operator (include/pnpadmm_offres_tz.h): the P segment pairs (l, l'), l <= l', whose
// spectra K_ll' the build sums, dealt to the build's workgroups in blocks of consecutive pairs, and under a linear plan the ascending list,
// per block, of the samples that carry weight in one of the block's pairs.  plan_offres_tz() is pure host code (no HIP call, no HIP header),
// so the lists a handle uploads are the lists the CPU suite checks (tests/asan_offres_tz_host.cpp); pnp_capi.hip uploads them and
// offres_tz_kernels.hip reads them.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

namespace pnp {

static constexpr int kOffresTzMaxPairs = 136;          // (PNP_OFFRES_TZ_MAX_PAIRS: asserted equal in pnp_capi.hip) 16 segments least squares, 32 linear
static constexpr int kOffresTzBlockLinear = 2;         // pairs per workgroup of the build: (l, l) and (l, l + 1) share the samples of segment l
static constexpr int kOffresTzBlockDense = 4;          // ... under a least-squares plan: every pair walks every sample

struct OffresTzPlan {
    int kind = 0;                                      // 1: linear (the band), 2: least squares (the upper triangle)
    int segments = 0;                                  // L
    int pairs = 0;                                     // P: 2 L - 1 linear, L (L + 1) / 2 least squares
    int pair_block = 0;                                // pairs per block
    int blocks = 0;                                    // ceil(P / pair_block)
    std::vector<int32_t> left, right;                  // [P]: the pair order - linear (0,0) (0,1) (1,1) (1,2) .., least squares the upper triangle row by row
    std::vector<int32_t> blk_off;                      // [blocks + 1]; empty under a least-squares plan (every block walks 0 .. M - 1)
    std::vector<int32_t> blk_idx;                      // ascending sample indices: seg_m in {l - 1, l} for the block of (l, l) and (l, l + 1)
};

// P of a plan of `kind` with L segments (0: no such plan)
int offres_tz_pairs(int kind, int segments);
// seg: [M] the linear plan's segment per sample (read only for kind == 1).  false: refused, `err` says why.
bool plan_offres_tz(int kind, int segments, int64_t m, const int32_t* seg, OffresTzPlan* out, std::string* err);

}  // namespace pnp
