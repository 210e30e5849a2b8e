"""Launch counts per profile class of every k-space entry point, on the MI355X through the C ABI (PnPEngine is the ctypes binding).

The results of these entry points are checked elsewhere; what is pinned here is how each one is sequenced: how many launches it books
under `fft_rows`, `fft_cols_prox` and `other` (pnp_profile_collect).  bench.py reads the first two, and an entry point that dropped,
doubled or re-classed a pass would still compute the right numbers.  Sizes: 16 x 16 (the smallest accepted; power-of-two passes) and
80 x 16, 16 x 80 (the smallest mixed-radix side on each axis); N = 2, C = 2 coils, K = 2 CG iterations.

Expected (rows, cols, other), read off the launch sequences in csrc/pnp_capi.hip:
  fft2c                       rows, cols                                                              (1, 1, 0)
  prox_dual, single-coil      rows forward, cols + solve, rows inverse                                (2, 1, 0)
  residuals(prev, dc)         tiles | rows, cols | misfit | reduce                                    (1, 1, 3)
  acquire -> y0, aty0, x0     rows, cols | epilogue | cols, rows | clamp                              (2, 2, 2)
  estimate_sens               window | cols, rows | rss, max, normalise                               (1, 1, 4)
  prox_dual, multi-coil       K + 1 normal operators (expand | rows, cols | mask | cols, rows | combine), the CG start (2), four
                              launches per CG iteration, the dual update                   (2 (K+1), 2 (K+1), 3 (K+1) + 2 + 4 K + 1)
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, C, K = 2, 2, 2
SIZES = [(16, 16), (80, 16), (16, 80)]
DEV = "cuda"


class _Case:
    def __init__(self, h, w):
        from dt4image_restoration_amd.engine import PnPEngine
        self.h, self.w = h, w
        self.e = PnPEngine(N, h, w, device=0, profile=True, denoiser=False)
        g = torch.Generator().manual_seed(1000 * h + w)
        rnd = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
        cpx = lambda *s: torch.complex(rnd(*s) - 0.5, rnd(*s) - 0.5).to(DEV)   # noqa: E731
        self.gt = rnd(N, 1, h, w).to(DEV)
        self.x0, self.y0 = cpx(N, 1, h, w), cpx(N, 1, h, w)
        self.y0c, self.sens = cpx(N, C, h, w), cpx(C, h, w)
        self.mask = (rnd(h, w) < 0.4).to(torch.uint8).to(DEV)
        self.mu = torch.tensor([0.1, 0.3], device=DEV)

    def counts(self, call):
        """(fft_rows, fft_cols_prox, other) launches booked by `call` alone."""
        torch.cuda.synchronize()
        self.e.profile_reset()
        call()
        torch.cuda.synchronize()
        p = self.e.profile_collect()
        return tuple(p[k]["launches"] for k in ("fft_rows", "fft_cols_prox", "other"))


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def case(request):
    c = _Case(*request.param)
    yield c
    c.e.close()


def test_fft2c(case):
    for inverse in (False, True):
        assert case.counts(lambda: case.e.fft2c(case.y0, inverse=inverse)) == (1, 1, 0)


def test_prox_dual_single_coil(case):
    x, z, u = case.e.reset(case.x0, case.y0, case.mask)
    assert case.counts(lambda: case.e.prox_dual(x, z, u, case.mu)) == (2, 1, 0)


def test_residuals_single_coil(case):
    x, z, u = case.e.reset(case.x0, case.y0, case.mask)
    prev = case.e.snapshot(x, z, u)
    case.e.prox_dual(x, z, u, case.mu)
    assert case.counts(lambda: case.e.residuals(x, z, u, prev=prev, dc=True)) == (1, 1, 3)


def test_acquire(case):
    assert case.counts(lambda: case.e.acquire(case.gt, case.mask, 0.01, 7)) == (2, 2, 2)


def test_estimate_sens(case):
    assert case.counts(lambda: case.e.estimate_sens(case.y0c, (8, 8))) == (1, 1, 4)


def test_prox_dual_multi_coil(case):
    x, z, u = case.e.reset(case.x0, case.y0c, case.mask, sens=case.sens, cg_iters=K)
    assert case.counts(lambda: case.e.prox_dual(x, z, u, case.mu)) == (2 * (K + 1), 2 * (K + 1), 3 * (K + 1) + 2 + 4 * K + 1)
