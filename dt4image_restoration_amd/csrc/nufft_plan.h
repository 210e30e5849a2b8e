// The plan of the non-Cartesian (NUFFT) operator pair of include/pnpadmm.h: per sample the footprint start and the 2 J float32 kernel
// weights, per axis the deconvolution factors, and for the gridding kernel the CSR list of the samples whose periodic footprint meets each
// grid tile.  plan_nufft() is pure host code (no HIP call, no HIP header), so the plan a handle uploads is the plan the CPU suite checks
// (tests/nufft_plan_host.cpp); pnp_capi.hip uploads it and nufft_kernels.hip reads it.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

namespace pnp {

static constexpr int kNufftTile = 16;                  // side of a gridding tile in grid points; every accepted grid side is a multiple of it
static constexpr int64_t kNufftMaxSamples = (int64_t)1 << 22;   // (PNP_NUFFT_MAX_SAMPLES: asserted equal in pnp_capi.hip)

struct NufftPlan {
    int h = 0, w = 0, gh = 0, gw = 0, width = 0;       // image, grid, kernel width J
    int64_t m = 0;                                     // samples
    int tiles_y = 0, tiles_x = 0;                      // gh / kNufftTile, gw / kNufftTile
    std::vector<int32_t> i0;                           // [2][M]: i0y then i0x = ceil(u - J/2), NOT reduced mod g: -J/2 .. g - J/2
    std::vector<float> wts;                            // [2 J][M]: rows 0 .. J-1 = phi(uy - (i0y + j)), rows J .. 2J-1 = phi(ux - (i0x + j))
    std::vector<float> cy, cx;                         // [H], [W]: sqrt(g / side) / phihat(q), q = i - side / 2
    std::vector<int32_t> bin_off;                      // [tiles_y tiles_x + 1]
    std::vector<int32_t> bin_idx;                      // ascending sample indices per tile (row-major tiles)
    float wy(int64_t s, int j) const { return wts[(size_t)j * m + s]; }
    float wx(int64_t s, int j) const { return wts[(size_t)(width + j) * m + s]; }
};

bool nufft_side_ok(int L);                             // a side the k-space stage accepts (kspace_len_ok's rule)
int nufft_default_grid(int side);                      // the smallest accepted g with 4 g >= 5 side; 0: none (side > 800)
double nufft_beta(int width, int g, int side);         // 2.30 J when g == 2 side, else 0.97 pi J (1 - side / (2 g))
double nufft_phi(double t, int width, double beta);    // the kernel
// phihat(q) = 2 int_0^{J/2} phi(t) cos(2 pi q t / g) dt by Gauss-Legendre quadrature (kNufftQuadNodes nodes), float64
static constexpr int kNufftQuadNodes = 128;
double nufft_phihat(int q, int width, int g, double beta);

// gh / gw == 0: the default grid of that axis.  traj: [M][2] (ky, kx) in cycles per pixel.  false: refused, `err` says why.
bool plan_nufft(int h, int w, int gh, int gw, int width, const double* traj, int64_t m, NufftPlan* out, std::string* err);

}  // namespace pnp
