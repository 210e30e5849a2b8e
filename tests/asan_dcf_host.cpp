// Host-side sanitizer check of the density compensation entry points of libpnpadmm (`make -C dt4image_restoration_amd/csrc asan_dcf` builds
// it against the instrumented library of `make asan`, host code only, and tests/asan_host.cpp's conventions apply).
// AddressSanitizer + UBSan see the argument validation of both entry points of include/pnpadmm_dcf.h: every rejection that needs no handle
// comes back before the handle is looked at, with the outputs untouched.  (The rejection that reads the handle - a call without a plan -
// is checked on the GPU by tests/test_gpu_dcf.py.)
// No GPU is needed: nothing here launches a kernel or makes a HIP call.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../include/pnpadmm_dcf.h"

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d %s [%s]\n", __FILE__, __LINE__, #cond, pnp_last_error()); ++fails; } } while (0)

static bool says(const char* what) { return std::strstr(pnp_last_error(), what) != nullptr; }

static float w0[64], w[64], out[64], info[PNP_DCF_MAX_ITERS + 1];

int main() {
    const int imin = std::numeric_limits<int>::min(), imax = std::numeric_limits<int>::max();
    float* const bufs[] = {w0, w, out, info};
    const size_t lens[] = {64, 64, 64, PNP_DCF_MAX_ITERS + 1};
    for (int b = 0; b < 4; ++b)
        for (size_t i = 0; i < lens[b]; ++i) bufs[b][i] = 7.f;

    // pnp_nufft_psi
    CHECK(pnp_nufft_psi(nullptr, w0, out, nullptr) == PNP_ERR_INVALID && says("null handle") && says("pnp_nufft_psi"));
    CHECK(pnp_nufft_psi(nullptr, w0, w0, nullptr) == PNP_ERR_INVALID && says("null handle"));                               // out may alias w
    CHECK(pnp_nufft_psi(nullptr, nullptr, out, nullptr) == PNP_ERR_INVALID && says("null w"));
    CHECK(pnp_nufft_psi(nullptr, w0, nullptr, nullptr) == PNP_ERR_INVALID && says("null out"));

    // pnp_nufft_dcf: a valid set reaches the handle check; w0 and info may be NULL, w may alias w0
    CHECK(pnp_nufft_dcf(nullptr, w0, 30, 0, w, info, nullptr) == PNP_ERR_INVALID && says("null handle") && says("pnp_nufft_dcf"));
    CHECK(pnp_nufft_dcf(nullptr, nullptr, 1, 0, w, nullptr, nullptr) == PNP_ERR_INVALID && says("null handle"));
    CHECK(pnp_nufft_dcf(nullptr, w, PNP_DCF_MAX_ITERS, 0, w, info, nullptr) == PNP_ERR_INVALID && says("null handle"));
    const int bad_iters[] = {0, -1, PNP_DCF_MAX_ITERS + 1, imin, imax};
    for (int k : bad_iters) {
        CHECK(pnp_nufft_dcf(nullptr, w0, k, 0, w, info, nullptr) == PNP_ERR_INVALID && says("iters"));
        CHECK(pnp_nufft_dcf(nullptr, w0, k, 1, nullptr, info, nullptr) == PNP_ERR_INVALID && says("iters"));                // scalar ranges first
    }
    const int bad_flags[] = {1, -1, imin, imax};
    for (int f : bad_flags) CHECK(pnp_nufft_dcf(nullptr, w0, 30, f, w, info, nullptr) == PNP_ERR_INVALID && says("flags"));
    CHECK(pnp_nufft_dcf(nullptr, w0, 30, 0, nullptr, info, nullptr) == PNP_ERR_INVALID && says("null w"));

    for (int b = 0; b < 4; ++b)
        for (size_t i = 0; i < lens[b]; ++i) CHECK(bufs[b][i] == 7.f);

    if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
    std::printf("asan_dcf_host: ok\n");
    return 0;
}
