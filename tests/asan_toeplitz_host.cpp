// Host-side sanitizer check of the Toeplitz entry points of libpnpadmm (`make -C dt4image_restoration_amd/csrc asan_toeplitz` builds it
// against the instrumented library of `make asan`, host code only, and tests/asan_host.cpp's conventions apply).
// AddressSanitizer + UBSan see the argument validation of every entry point of include/pnpadmm_toeplitz.h: every rejection that needs no
// handle comes back before the handle is looked at, with the outputs untouched.  (The rejections that read the handle - batch > n, sens_n
// that is neither 1 nor n, a side above 512, a call without a plan or without a spectrum - are checked on the GPU by
// tests/test_gpu_toeplitz.py.)
// No GPU is needed: nothing here launches a kernel or makes a HIP call.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../include/pnpadmm_toeplitz.h"

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d %s [%s]\n", __FILE__, __LINE__, #cond, pnp_last_error()); ++fails; } } while (0)

static bool says(const char* what) { return std::strstr(pnp_last_error(), what) != nullptr; }

static float img[512], sens[512], smp[64], wgt[8], x[256], z[512], u[512], out[512];

int main() {
    const int imin = std::numeric_limits<int>::min(), imax = std::numeric_limits<int>::max();
    float* const bufs[] = {img, sens, smp, x, z, u, out};
    const size_t lens[] = {512, 512, 64, 256, 512, 512, 512};
    for (int b = 0; b < 7; ++b)
        for (size_t i = 0; i < lens[b]; ++i) bufs[b][i] = 7.f;

    // the plan, the getters, the spectrum
    CHECK(pnp_toeplitz_plan(nullptr, wgt, 0, nullptr) == PNP_ERR_INVALID && says("null handle") && says("pnp_toeplitz_plan"));
    CHECK(pnp_toeplitz_plan(nullptr, nullptr, 0, nullptr) == PNP_ERR_INVALID && says("null handle"));                     // weights may be NULL
    const int bad_flags[] = {1, -1, imin, imax};
    for (int f : bad_flags) CHECK(pnp_toeplitz_plan(nullptr, wgt, f, nullptr) == PNP_ERR_INVALID && says("flags"));
    CHECK(pnp_toeplitz_planned(nullptr) == 0 && pnp_toeplitz_live(nullptr) == 0);
    CHECK(pnp_toeplitz_spectrum(nullptr, out, nullptr) == PNP_ERR_INVALID && says("null handle") && says("pnp_toeplitz_spectrum"));
    CHECK(pnp_toeplitz_spectrum(nullptr, nullptr, nullptr) == PNP_ERR_INVALID && says("null out"));

    // the applications
    CHECK(pnp_toeplitz_apply(nullptr, img, 1, out, nullptr) == PNP_ERR_INVALID && says("null handle") && says("pnp_toeplitz_apply"));
    CHECK(pnp_toeplitz_apply_mc(nullptr, img, sens, 4, 1, 1, out, nullptr) == PNP_ERR_INVALID && says("null handle") && says("pnp_toeplitz_apply_mc"));
    CHECK(pnp_toeplitz_apply_mc(nullptr, img, sens, PNP_MC_MAX_COILS, 3, imax, out, nullptr) == PNP_ERR_INVALID && says("null handle"));
    const int bad_batch[] = {0, -1, imin};
    for (int b : bad_batch) {
        CHECK(pnp_toeplitz_apply(nullptr, img, b, out, nullptr) == PNP_ERR_INVALID && says("batch"));
        CHECK(pnp_toeplitz_apply_mc(nullptr, img, sens, 4, 1, b, out, nullptr) == PNP_ERR_INVALID && says("batch"));
    }
    const int bad_coils[] = {0, -1, PNP_MC_MAX_COILS + 1, imin, imax};
    for (int c : bad_coils) {
        CHECK(pnp_toeplitz_apply_mc(nullptr, img, sens, c, 1, 1, out, nullptr) == PNP_ERR_INVALID && says("coils"));
        CHECK(pnp_set_kspace_ncsense_tz(nullptr, smp, sens, c, 1, 8, nullptr) == PNP_ERR_INVALID && says("coils"));
        CHECK(pnp_reset_ncsense_tz(nullptr, img, smp, sens, c, 1, 8, x, z, u, nullptr) == PNP_ERR_INVALID && says("coils"));
    }
    const int bad_sens_n[] = {0, -1, imin};
    for (int n : bad_sens_n) {
        CHECK(pnp_toeplitz_apply_mc(nullptr, img, sens, 4, n, 1, out, nullptr) == PNP_ERR_INVALID && says("sens_n"));
        CHECK(pnp_set_kspace_ncsense_tz(nullptr, smp, sens, 4, n, 8, nullptr) == PNP_ERR_INVALID && says("sens_n"));
        CHECK(pnp_reset_ncsense_tz(nullptr, img, smp, sens, 4, n, 8, x, z, u, nullptr) == PNP_ERR_INVALID && says("sens_n"));
    }
    CHECK(pnp_toeplitz_apply(nullptr, nullptr, 1, out, nullptr) == PNP_ERR_INVALID && says("null img"));
    CHECK(pnp_toeplitz_apply(nullptr, img, 1, nullptr, nullptr) == PNP_ERR_INVALID && says("null out"));
    CHECK(pnp_toeplitz_apply(nullptr, img, 1, img, nullptr) == PNP_ERR_INVALID && says("alias"));
    CHECK(pnp_toeplitz_apply_mc(nullptr, nullptr, sens, 4, 1, 1, out, nullptr) == PNP_ERR_INVALID && says("null img"));
    CHECK(pnp_toeplitz_apply_mc(nullptr, img, nullptr, 4, 1, 1, out, nullptr) == PNP_ERR_INVALID && says("null sens"));
    CHECK(pnp_toeplitz_apply_mc(nullptr, img, sens, 4, 1, 1, nullptr, nullptr) == PNP_ERR_INVALID && says("null out"));
    CHECK(pnp_toeplitz_apply_mc(nullptr, img, sens, 4, 1, 1, img, nullptr) == PNP_ERR_INVALID && says("alias"));
    CHECK(pnp_toeplitz_apply_mc(nullptr, img, sens, 4, 1, 1, sens, nullptr) == PNP_ERR_INVALID && says("alias"));

    // the installers: a valid set reaches the handle check
    CHECK(pnp_set_kspace_nc_tz(nullptr, smp, 8, nullptr) == PNP_ERR_INVALID && says("null handle") && says("pnp_set_kspace_nc_tz"));
    CHECK(pnp_reset_nc_tz(nullptr, img, smp, PNP_MC_MAX_CG, x, z, u, nullptr) == PNP_ERR_INVALID && says("null handle") && says("pnp_reset_nc_tz"));
    CHECK(pnp_set_kspace_ncsense_tz(nullptr, smp, sens, 4, 1, 1, nullptr) == PNP_ERR_INVALID && says("null handle") && says("pnp_set_kspace_ncsense_tz"));
    CHECK(pnp_reset_ncsense_tz(nullptr, img, smp, sens, 4, 2, 8, x, z, u, nullptr) == PNP_ERR_INVALID && says("null handle") && says("pnp_reset_ncsense_tz"));
    const int bad_cg[] = {0, -1, PNP_MC_MAX_CG + 1, imin, imax};
    for (int k : bad_cg) {
        CHECK(pnp_set_kspace_nc_tz(nullptr, smp, k, nullptr) == PNP_ERR_INVALID && says("cg_iters"));
        CHECK(pnp_reset_nc_tz(nullptr, img, smp, k, x, z, u, nullptr) == PNP_ERR_INVALID && says("cg_iters"));
        CHECK(pnp_set_kspace_ncsense_tz(nullptr, smp, sens, 4, 1, k, nullptr) == PNP_ERR_INVALID && says("cg_iters"));
        CHECK(pnp_reset_ncsense_tz(nullptr, img, smp, sens, 4, 1, k, x, z, u, nullptr) == PNP_ERR_INVALID && says("cg_iters"));
    }
    CHECK(pnp_set_kspace_nc_tz(nullptr, nullptr, 8, nullptr) == PNP_ERR_INVALID && says("null y"));
    CHECK(pnp_reset_nc_tz(nullptr, nullptr, smp, 8, x, z, u, nullptr) == PNP_ERR_INVALID && says("null x0"));
    CHECK(pnp_reset_nc_tz(nullptr, img, nullptr, 8, x, z, u, nullptr) == PNP_ERR_INVALID && says("null y"));
    CHECK(pnp_reset_nc_tz(nullptr, img, smp, 8, nullptr, z, u, nullptr) == PNP_ERR_INVALID && says("null x, z or u"));
    CHECK(pnp_reset_nc_tz(nullptr, img, smp, 8, x, nullptr, u, nullptr) == PNP_ERR_INVALID && says("null x, z or u"));
    CHECK(pnp_reset_nc_tz(nullptr, img, smp, 8, x, z, nullptr, nullptr) == PNP_ERR_INVALID && says("null x, z or u"));
    CHECK(pnp_set_kspace_ncsense_tz(nullptr, nullptr, sens, 4, 1, 8, nullptr) == PNP_ERR_INVALID && says("null y"));
    CHECK(pnp_set_kspace_ncsense_tz(nullptr, smp, nullptr, 4, 1, 8, nullptr) == PNP_ERR_INVALID && says("null sens"));
    CHECK(pnp_reset_ncsense_tz(nullptr, nullptr, smp, sens, 4, 1, 8, x, z, u, nullptr) == PNP_ERR_INVALID && says("null x0"));
    CHECK(pnp_reset_ncsense_tz(nullptr, img, nullptr, sens, 4, 1, 8, x, z, u, nullptr) == PNP_ERR_INVALID && says("null y"));
    CHECK(pnp_reset_ncsense_tz(nullptr, img, smp, nullptr, 4, 1, 8, x, z, u, nullptr) == PNP_ERR_INVALID && says("null sens"));
    CHECK(pnp_reset_ncsense_tz(nullptr, img, smp, sens, 4, 1, 8, nullptr, z, u, nullptr) == PNP_ERR_INVALID && says("null x, z or u"));
    CHECK(pnp_reset_ncsense_tz(nullptr, img, smp, sens, 4, 1, 8, x, nullptr, u, nullptr) == PNP_ERR_INVALID && says("null x, z or u"));
    CHECK(pnp_reset_ncsense_tz(nullptr, img, smp, sens, 4, 1, 8, x, z, nullptr, nullptr) == PNP_ERR_INVALID && says("null x, z or u"));

    for (int b = 0; b < 7; ++b)
        for (size_t i = 0; i < lens[b]; ++i) CHECK(bufs[b][i] == 7.f);

    if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
    std::printf("asan_toeplitz_host: ok\n");
    return 0;
}
