"""Every slice size the engine accepts, 16 through 1024, against a plain float64 restatement of the same operation.

The k-space stage (pnp_reset, pnp_set_kspace, pnp_prox_dual, pnp_fft2c, pnp_step) takes H and W from the 13 sides of the form 2^a * 5^b
(kspace_len_ok), mixed freely: all 169 (H, W) pairs run here, which reaches every kernel variant of both paths:
  * both sides powers of two (fft_kernels.hip): rows by fft_rows_kernel<1|2, 0> at W = 16, 32, 64, 1024 (2 rows per workgroup at 1024),
    the unrolled <1|2, 128> at W = 128, the radix-16 / radix-8 forms at W = 256 / 512; columns by fft_cols_kernel<1, 0> at H = 16, 32, 64,
    1024 (4 columns and 73.8 KB of LDS per workgroup at 1024: the raised cap), the unrolled <1, 128 | 256 | 512> at the other three;
    pnp_fft2c by fft_rows_kernel<0, 0> / fft_cols_kernel<0, 0> at every power-of-two pair;
  * a side of 80, 160, 320, 400, 640 or 800 (fft_mixed_kernels.hip) beside each of the 13 sides, on either axis: 2 to 16 rows per
    workgroup, 16 / 8 / 4 columns (57.7 KB of LDS at H = 800, 73.8 KB at H = 1024).
The 51 other multiples of 16 are refused without touching their outputs.  The denoiser (any multiple of 16 up to 1024) and the full step
run at the corners of that range.  Expected values are computed here, in float64 from the exact float32 / complex64 inputs the GPU sees;
no fixture is read."""
import os

import numpy as np
import pytest
import torch

from dt4image_restoration_amd import _lib, synthetic, weights
from oracle import pnp_oracle as O

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCUMENTED = "16, 32, 64, 80, 128, 160, 256, 320, 400, 512, 640, 800, 1024"   # include/pnpadmm.h, README.md, the refusal message


def kspace_len_ok(L: int) -> bool:
    """The engine's size rule (kspace_len_ok): 16 <= L <= 1024, 16 | L, and L = 2^a * 5^b."""
    if L < 16 or L > 1024 or L % 16:
        return False
    while L % 5 == 0:
        L //= 5
    return L & (L - 1) == 0


MULTIPLES = list(range(16, 1025, 16))
SIDES = [L for L in MULTIPLES if kspace_len_ok(L)]
REFUSED = [L for L in MULTIPLES if not kspace_len_ok(L)]
PAIRS = [(h, w) for h in SIDES for w in SIDES]
# each refused side once, beside an accepted side, on alternating axes
REFUSED_PAIRS = [(L, SIDES[i % len(SIDES)]) if i % 2 == 0 else (SIDES[i % len(SIDES)], L) for i, L in enumerate(REFUSED)]


def _ids(shapes):
    return ["x".join(str(v) for v in s) for s in shapes]


# ---- float64 reference ---------------------------------------------------------------------------------------------------------------

def fft2c64(a) -> np.ndarray:
    """Centred orthonormal 2-D DFT over the last two axes in complex128: ifftshift, fft2(norm='ortho'), fftshift."""
    a = np.asarray(a, dtype=np.complex128)
    return np.fft.fftshift(np.fft.fft2(np.fft.ifftshift(a, axes=(-2, -1)), norm="ortho"), axes=(-2, -1))


def ifft2c64(a) -> np.ndarray:
    a = np.asarray(a, dtype=np.complex128)
    return np.fft.fftshift(np.fft.ifft2(np.fft.ifftshift(a, axes=(-2, -1)), norm="ortho"), axes=(-2, -1))


def prox64(x, u, y0, mask, mu):
    """The data-fidelity half of PnPEnv.step (env.py:87-93) in float64: zf = fft2c(x + u); on the mask zf = (mu zf + y0) / (1 + mu);
    z = ifft2c(zf); u' = u + x - z.  x [n,1,H,W] real, u / y0 [n,1,H,W] complex, mask bool [H,W] or [n,H,W], mu [n].  Returns (z, u')."""
    x = np.asarray(x, dtype=np.float64)
    u = np.asarray(u, dtype=np.complex128)
    n, _, h, w = x.shape
    m = np.asarray(mask, dtype=bool).reshape(-1, 1, h, w)
    mu = np.asarray(mu, dtype=np.float64).reshape(n, 1, 1, 1)
    zf = fft2c64(x + u)
    zf = np.where(m, (mu * zf + np.asarray(y0, dtype=np.complex128)) / (1 + mu), zf)
    z = ifft2c64(zf)
    return z, u + x - z


def psnr64(x, gt) -> np.ndarray:
    """torch_psnr (env.py:120-125) in float64: 10 log10(1 / mean((clamp(x, 0, 1) - gt)^2)) per slice."""
    x = np.clip(np.asarray(x, dtype=np.float64), 0.0, 1.0)
    n = x.shape[0]
    mse = ((x.reshape(n, -1) - np.asarray(gt, dtype=np.float64).reshape(n, -1)) ** 2).mean(axis=1)
    return 10 * np.log10(1.0 / mse)


def _errs(got: torch.Tensor, ref: np.ndarray):
    """(max abs error of any real / imaginary part, rms(err) / rms(ref)) of a device result against its float64 reference."""
    d = got.cpu().numpy().astype(ref.dtype) - ref
    mx = float(max(np.abs(d.real).max(), np.abs(d.imag).max()))
    return mx, float(np.sqrt((np.abs(d) ** 2).mean() / (np.abs(ref) ** 2).mean()))


def _cplx(rng, shape, scale=1.0) -> torch.Tensor:
    """complex64 with real and imaginary parts uniform in [-scale, scale)."""
    v = (rng.random(tuple(shape) + (2,), dtype=np.float32) * 2 - 1) * np.float32(scale)
    return torch.view_as_complex(torch.from_numpy(v))


def _mirror(m: torch.Tensor) -> torch.Tensor:
    """Point reflection about the centred origin (H/2, W/2): index k -> -k mod L."""
    return torch.roll(torch.flip(m, dims=(-2, -1)), shifts=(1, 1), dims=(-2, -1))


# ---- CPU: the size list and the reference itself -------------------------------------------------------------------------------------

def test_size_list_is_the_documented_one():
    assert SIDES == [int(s) for s in DOCUMENTED.split(", ")]
    assert len(PAIRS) == 169 and len(set(PAIRS)) == 169
    assert len(REFUSED) == 51 and not set(REFUSED) & set(SIDES)
    assert sorted(L for p in REFUSED_PAIRS for L in p if L in REFUSED) == REFUSED
    assert all(kspace_len_ok(a) != kspace_len_ok(b) for a, b in REFUSED_PAIRS)
    assert {p[0] in REFUSED for p in REFUSED_PAIRS} == {True, False}        # refused on both axes
    for path in ("include/pnpadmm.h", "README.md", "dt4image_restoration_amd/csrc/pnp_capi.hip"):
        assert DOCUMENTED in open(os.path.join(ROOT, path)).read(), path


@pytest.mark.parametrize("h,w", [(16, 16), (80, 80), (800, 800), (1024, 80)], ids=_ids([(16, 16), (80, 80), (800, 800), (1024, 80)]))
def test_float64_reference_matches_the_oracle_in_complex128(h, w):
    rng = np.random.default_rng(h * 7 + w)
    a = rng.standard_normal((2, 1, h, w)) + 1j * rng.standard_normal((2, 1, h, w))
    at = torch.from_numpy(a)
    assert np.abs(fft2c64(a) - O.fft2c(at).numpy()).max() <= 1e-12
    assert np.abs(ifft2c64(a) - O.ifft2c(at).numpy()).max() <= 1e-12
    # prox64 against the same step written with the oracle's transforms (env.py:87-93 as pnp_oracle.admm_step has it)
    x = rng.random((2, 1, h, w))
    mask = rng.random((2, 1, h, w)) < 0.3
    mu = np.array([0.0, 0.6])
    z, u = prox64(x, a, 0.5 * a[::-1], mask, mu)
    mut = torch.from_numpy(mu).view(2, 1, 1, 1)
    zf = O.fft2c(torch.from_numpy(x) + at)
    zo = O.ifft2c(torch.where(torch.from_numpy(mask), (mut * zf + torch.from_numpy(0.5 * a[::-1].copy())) / (1 + mut), zf))
    assert np.abs(z - zo.numpy()).max() <= 1e-12
    assert np.abs(u - (at + torch.from_numpy(x) - zo).numpy()).max() <= 1e-12


# ---- GPU: the k-space stage on all 169 pairs ------------------------------------------------------------------------------------------

FFT_ATOL = 3e-6        # FLOAT TOLERANCE: f32 FFT of O(1) data against float64 (the suite's bound since the first fft2c test)
PROX_ATOL = 5e-6       # FLOAT TOLERANCE: two f32 FFTs + the pointwise solve, O(1) data (the suite's prox_dual bound)
REL_RMS = 1e-6         # rms(err) / rms(ref): a few f32 ulps of accumulated rounding at every size
MUS = (0.0, 0.05, 0.6, 4.0)   # 0 = hard data consistency
SENTINEL = -7.25


def _kspace_engine(n, h, w):
    from dt4image_restoration_amd.engine import PnPEngine
    return PnPEngine(n, h, w, denoiser=False)


@gpu
@pytest.mark.parametrize("h,w", PAIRS, ids=_ids(PAIRS))
def test_fft2c_and_psnr_at_every_pair(h, w, record_property):
    """pnp_fft2c both ways against float64 on a batch below n, round trip, Parseval, known answers, in == out; batch > n refused;
    pnp_psnr with the clamp at work."""
    n, b = 3, 2
    rng = np.random.default_rng(10_000 + 1031 * h + w)
    e = _kspace_engine(n, h, w)
    try:
        c = _cplx(rng, (b, 1, h, w))
        cg = c.cuda()
        fwd = None
        for inverse, ref in ((False, fft2c64(c.numpy())), (True, ifft2c64(c.numpy()))):
            got = e.fft2c(cg, inverse=inverse)
            mx, rel = _errs(got, ref)
            record_property("ifft2c" if inverse else "fft2c", f"{mx:.3e} {rel:.3e}")
            assert mx <= FFT_ATOL and rel <= REL_RMS, (inverse, mx, rel)
            # in == out (the header allows it): the same bits as out-of-place
            buf = cg.clone()
            _lib.check(e.lib.pnp_fft2c(e._h, buf.data_ptr(), buf.data_ptr(), b, h, w, int(inverse), e._stream()), "pnp_fft2c")
            assert torch.equal(buf, got), inverse
            if not inverse:
                fwd = got
        back = e.fft2c(fwd, inverse=True)
        assert float(torch.view_as_real(back.cpu() - c).abs().max()) <= FFT_ATOL
        f64, c64 = fwd.cpu().numpy().astype(np.complex128), c.numpy().astype(np.complex128)
        assert abs((np.abs(f64) ** 2).sum() / (np.abs(c64) ** 2).sum() - 1) < 1e-5      # Parseval (ortho)

        # known answers: the centred bin (p, q) (p in [-H/2, H/2)) sits at index ((p + H/2) mod H, (q + W/2) mod W)
        yy, xx = np.meshgrid(np.arange(h) - h // 2, np.arange(w) - w // 2, indexing="ij")
        bins = ((0, 0), (-h // 2, -w // 2), (3, -(w // 4) - 1))   # origin, Nyquist on both axes, an asymmetric bin
        waves = np.stack([np.exp(2j * np.pi * (p * yy / h + q * xx / w)) / np.sqrt(h * w) for p, q in bins])[:, None]
        peaks = np.zeros((3, 1, h, w), dtype=np.complex128)
        for s, (p, q) in enumerate(bins):
            peaks[s, 0, (p + h // 2) % h, (q + w // 2) % w] = 1.0
        assert peaks[1, 0, 0, 0] == 1 and peaks[2, 0, h // 2 + 3, w // 4 - 1] == 1
        # the wave of bin (0, 0) is the constant 1/sqrt(HW); a delta at the centred origin maps to it both ways
        for inverse, src, dst in ((False, waves, peaks), (True, peaks, waves)):
            got = e.fft2c(torch.from_numpy(src.astype(np.complex64)).cuda(), inverse=inverse).cpu().numpy()
            assert np.abs(got - dst).max() <= FFT_ATOL, inverse
        got = e.fft2c(torch.from_numpy(peaks[:1].astype(np.complex64)).cuda()).cpu().numpy()
        assert np.abs(got - 1 / np.sqrt(h * w)).max() <= FFT_ATOL

        # a batch above n is refused and the output is not touched
        big = torch.zeros((n + 1, 1, h, w), dtype=torch.complex64, device="cuda")
        out = torch.full_like(big, complex(SENTINEL, SENTINEL))
        assert e.lib.pnp_fft2c(e._h, big.data_ptr(), out.data_ptr(), n + 1, h, w, 0, e._stream()) == -1   # PNP_ERR_INVALID
        assert "does not fit the engine" in e.lib.pnp_last_error().decode()
        torch.cuda.synchronize()
        assert bool((out == complex(SENTINEL, SENTINEL)).all())

        x = torch.from_numpy(rng.random((n, 1, h, w), dtype=np.float32) * np.float32(1.6) - np.float32(0.3))   # ~ 35 % clamped
        gt = torch.from_numpy(rng.random((n, 1, h, w), dtype=np.float32))
        got = e.psnr(x.cuda(), gt.cuda()).cpu().numpy()
        np.testing.assert_allclose(got, psnr64(x.numpy(), gt.numpy()), rtol=1e-6, atol=0)
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("h,w", PAIRS, ids=_ids(PAIRS))
def test_reset_and_prox_dual_at_every_pair(h, w, record_property):
    """pnp_reset exactly; pnp_prox_dual against prox64 with random asymmetric masks (per slice on half of the pairs), y0 random on every
    bin and per-slice mu in {0, 0.05, 0.6, 4}; a slice stopped by t_action kept bit for bit; set_kspace after a reset with other
    constants = a reset with them, bit for bit; the same slices at positions 5-7 of n = 8 give the same bits."""
    n = 3
    i, j = SIDES.index(h), SIDES.index(w)
    k = i * len(SIDES) + j
    per_slice = (i + j) % 2 == 0
    rng = np.random.default_rng(20_000 + 1031 * h + w)
    x0, y0 = _cplx(rng, (n, 1, h, w)), _cplx(rng, (n, 1, h, w))
    dens = np.array([0.15, 0.35, 0.6])[:, None, None]
    mask = torch.from_numpy(rng.random((n, h, w)) < dens) if per_slice else torch.from_numpy(rng.random((h, w)) < 0.3)
    ya = _cplx(rng, (n, 1, h, w))                          # the other episode's constants, with the other mask layout
    mask_a = torch.from_numpy(rng.random((h, w)) < 0.5) if per_slice else torch.from_numpy(rng.random((n, h, w)) < 0.5)
    assert not torch.equal(mask, _mirror(mask))            # not point-symmetric: a wrong mirror fold cannot hide
    xin = torch.from_numpy(rng.random((n, 1, h, w), dtype=np.float32))
    uin = _cplx(rng, (n, 1, h, w), 0.5)
    mu = torch.tensor([MUS[(k + s) % len(MUS)] for s in range(n)], dtype=torch.float32)
    g = {name: t.cuda() for name, t in (("x0", x0), ("y0", y0), ("mask", mask), ("ya", ya), ("mask_a", mask_a), ("x", xin),
                                         ("u", uin), ("mu", mu))}
    sent = complex(SENTINEL, SENTINEL)
    e = _kspace_engine(n, h, w)
    try:
        # episode A, then B's constants through set_kspace
        x, z, u = e.reset(g["x0"], g["ya"], g["mask_a"])
        assert torch.equal(x.cpu(), x0.real.reshape(n, 1, h, w)) and torch.equal(z.cpu(), x0) and not bool(u.cpu().abs().any())
        e.set_kspace(g["y0"], g["mask"])
        xs, zs, us = g["x"].clone(), torch.full_like(g["u"], sent), g["u"].clone()
        e.prox_dual(xs, zs, us, g["mu"])
        # a reset with B
        x, z, u = e.reset(g["x0"], g["y0"], g["mask"])
        assert torch.equal(x.cpu(), x0.real.reshape(n, 1, h, w)) and torch.equal(z.cpu(), x0) and not bool(u.cpu().abs().any())
        xb, zb, ub = g["x"].clone(), torch.full_like(g["u"], sent), g["u"].clone()
        e.prox_dual(xb, zb, ub, g["mu"])
        zr, ur = prox64(xin.numpy(), uin.numpy(), y0.numpy(), mask.numpy(), mu.numpy())
        for name, got, ref in (("z", zb, zr), ("u", ub, ur)):
            mx, rel = _errs(got, ref)
            record_property(f"prox_{name}", f"{mx:.3e} {rel:.3e}")
            assert mx <= PROX_ATOL and rel <= REL_RMS, (name, mx, rel)
        assert torch.equal(zs, zb) and torch.equal(us, ub)    # set_kspace(B) == reset(B)
        assert torch.equal(xb, g["x"])                         # x is read only

        # one slice stopped: its z and u keep their bits, x is not written, the others move
        stop = k % n
        tact = torch.zeros(n)
        tact[stop] = 0.9
        z1, u1 = zb.clone(), ub.clone()
        e.prox_dual(xb, zb, ub, g["mu"], t_action=tact.cuda())
        assert torch.equal(zb[stop], z1[stop]) and torch.equal(ub[stop], u1[stop]) and torch.equal(xb, g["x"])
        for s in range(n):
            if s != stop:
                assert not torch.equal(ub[s], u1[s]) and not torch.equal(zb[s], z1[s]), s

        # the same three slices at positions 5-7 of an 8-slice handle (grids that are multiples of 8: the XCD remap is active)
        def pad8(t):
            return torch.cat([t[:1].expand(5, *t.shape[1:]), t]).contiguous()
        e8 = _kspace_engine(8, h, w)
        try:
            e8.reset(pad8(g["x0"]), pad8(g["y0"]), pad8(g["mask"]) if per_slice else g["mask"])
            x8, z8, u8 = pad8(g["x"]), torch.full((8, 1, h, w), sent, dtype=torch.complex64, device="cuda"), pad8(g["u"])
            e8.prox_dual(x8, z8, u8, pad8(g["mu"]))
            assert torch.equal(z8[5:], z1) and torch.equal(u8[5:], u1)
        finally:
            e8.close()
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("h,w", REFUSED_PAIRS, ids=_ids(REFUSED_PAIRS))
def test_refused_sizes_name_the_shape_and_touch_nothing(h, w):
    from dt4image_restoration_amd._lib import PnPError
    rng = np.random.default_rng(h * 1031 + w)
    e = _kspace_engine(1, h, w)
    try:
        x0, y0 = _cplx(rng, (1, 1, h, w)).cuda(), _cplx(rng, (1, 1, h, w)).cuda()
        mask = torch.from_numpy(rng.random((h, w)) < 0.3).to(torch.uint8).cuda()
        x = torch.full((1, 1, h, w), SENTINEL, device="cuda")
        z, u, out = (torch.full((1, 1, h, w), complex(SENTINEL, SENTINEL), dtype=torch.complex64, device="cuda") for _ in range(3))

        def refused(rc, what):
            with pytest.raises(PnPError) as ei:
                _lib.check(rc, what)
            msg = str(ei.value)
            assert f"{h}x{w}" in msg and DOCUMENTED in msg, msg

        refused(e.lib.pnp_reset(e._h, x0.data_ptr(), y0.data_ptr(), mask.data_ptr(), 1, x.data_ptr(), z.data_ptr(), u.data_ptr(),
                                e._stream()), "pnp_reset")
        refused(e.lib.pnp_set_kspace(e._h, y0.data_ptr(), mask.data_ptr(), 1, e._stream()), "pnp_set_kspace")
        for inverse in (0, 1):
            refused(e.lib.pnp_fft2c(e._h, x0.data_ptr(), out.data_ptr(), 1, h, w, inverse, e._stream()), "pnp_fft2c")
        with pytest.raises(PnPError, match="pnp_reset has not been called"):
            e.prox_dual(x, z, u, torch.zeros(1, device="cuda"))
        torch.cuda.synchronize()
        assert bool((x == SENTINEL).all())
        for t in (z, u, out):
            assert bool((t == complex(SENTINEL, SENTINEL)).all())
    finally:
        e.close()


# ---- GPU: the denoiser at the sides no other test runs -------------------------------------------------------------------------------

DENOISER_SHAPES = [(1, 1024, 1024), (1, 16, 1024), (1, 1024, 16), (2, 800, 640), (1, 1008, 112)]
DENOISER_MODE_ENV = {"default": {}, "winograd": {"PNP_WINO_MIN_BLOCKS": "1"}, "direct": {"PNP_NO_WINOGRAD": "1"}, "bf16": {}}
STAGES_SHAPE = (1, 1024, 1024)          # test_denoiser_stages_at_1024x1024
_DENOISER_REF = {}


@pytest.fixture(scope="module")
def sd_np():
    return weights.generate_unet_weights(0, "unit_gain")


def _denoiser_inputs(n, h, w):
    x = (torch.from_numpy(synthetic.hash_uniform(23, h * 1031 + w, n * h * w).reshape(n, 1, h, w)) + 1) * 0.5
    return x, torch.linspace(5, 50, n) / 255.0


def _denoiser_ref(sd_np, n, h, w, bf16):
    """O.denoise on the f32 or bf16-operand oracle, once per shape and arithmetic (~2 s at 1024 x 1024 on 8 cores)."""
    key = (n, h, w, bf16)
    if key not in _DENOISER_REF:
        x, sigma = _denoiser_inputs(n, h, w)
        _DENOISER_REF[key] = O.denoise(O.torch_weights(sd_np), x, sigma, bf16_operands=bf16)
    return _DENOISER_REF[key]


@gpu
@pytest.mark.parametrize("mode", list(DENOISER_MODE_ENV))
@pytest.mark.parametrize("n,h,w", DENOISER_SHAPES, ids=_ids(DENOISER_SHAPES))
def test_denoiser_at_large_and_extreme_sides(sd_np, n, h, w, mode, monkeypatch):
    """16 x 1024 has a 1 x 64 bottom level, 1024 x 16 a 64 x 1 one, 1008 x 112 a 63 x 7 one (1008 is refused by the k-space stage
    only); each under the modes of test_denoiser_shape_sweep, with its bounds.  In default mode, out == x gives the same bits."""
    from dt4image_restoration_amd.engine import PnPEngine
    for k, v in DENOISER_MODE_ENV[mode].items():
        monkeypatch.setenv(k, v)
    e = PnPEngine(n, h, w, bf16_convs=(mode == "bf16"))
    try:
        e.load_weights(sd_np)
        algos = e.conv_algorithms()[1:27]
        if mode == "winograd":
            assert any(v in (1, 4) for v in algos)
        if mode == "direct":
            assert all(v == 0 for v in algos)
        if mode == "bf16":
            assert all(v in (0, 5) for v in algos)
        x, sigma = _denoiser_inputs(n, h, w)
        xg, sg = x.cuda(), sigma.cuda()
        got = e.denoise(xg, sg)
        ref = _denoiser_ref(sd_np, n, h, w, mode == "bf16")
        # FLOAT TOLERANCE: f32 summation order (1e-5); bf16 operands: rounding flips reach the output at ~1e-3 (test_gpu_kernels.py)
        np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), rtol=0, atol=2e-3 if mode == "bf16" else 1e-5)
        assert float((got - xg).abs().max()) > 1e-3                # the network did something
        if mode == "default":
            xa = xg.clone()
            assert e.denoise(xa, sg, out=xa) is xa
            assert torch.equal(xa, got)
    finally:
        e.close()


@gpu
def test_denoiser_stages_at_1024x1024(sd_np):
    from dt4image_restoration_amd.engine import PnPEngine
    n, h, w = STAGES_SHAPE
    e = PnPEngine(n, h, w, keep_stages=True)
    try:
        e.load_weights(sd_np)
        x, sigma = _denoiser_inputs(n, h, w)
        got = e.denoise(x.cuda(), sigma.cuda())
        ref_raw, stages = O.unet_forward(O.torch_weights(sd_np), torch.cat([x, torch.ones(n, 1, h, w) * sigma.view(n, 1, 1, 1)], 1),
                                         return_stages=True)
        for which, (name, ref) in enumerate(stages.items()):
            a = e.read_stage(which).cpu()
            assert a.shape == ref.shape, name
            # FLOAT TOLERANCE: the per-stage bound of test_denoiser_matches_oracle_per_stage
            err = float((a - ref).abs().max())
            assert err < 5e-5 * max(1.0, float(ref.abs().max())), f"stage {name}: max err {err}"
        np.testing.assert_allclose(got.cpu().numpy(), torch.clamp(ref_raw, 0, 1).numpy(), rtol=0, atol=1e-5)
    finally:
        e.close()


# ---- GPU: the full step at the corners of the size range ----------------------------------------------------------------------------

STEP_SHAPES = [(2, 16, 16), (1, 16, 1024), (1, 1024, 16), (1, 1024, 1024), (2, 800, 160)]


@gpu
@pytest.mark.parametrize("n,h,w", STEP_SHAPES, ids=_ids(STEP_SHAPES))
def test_step_at_the_corners_of_the_size_range(sd_np, n, h, w):
    """Three pnp_step iterations against O.admm_step after each one: x, z, u, PSNR, t_state and done; with two slices, slice 1 is
    stopped from the second iteration on and keeps its bits."""
    from dt4image_restoration_amd.engine import PnPEngine
    iters = 3
    data = synthetic.make_problem(n, h, w, accel=4.0, seed=600 + h + w)
    mu_tab, sig_tab = synthetic.param_table(n, iters, seed=77)
    sd = O.torch_weights(sd_np)
    st = O.reset(data)
    e = PnPEngine(n, h, w)
    try:
        e.load_weights(sd_np)
        x, z, u = e.reset(st["z"].cuda(), st["y0"].cuda(), st["mask"].reshape(h, w).cuda())
        gt = st["gt"].cuda()
        ts = torch.zeros(n, device="cuda")
        done = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        t_exp = np.zeros(n, dtype=np.float32)
        frozen = None
        for t in range(iters):
            tact = torch.zeros(n)
            if n == 2 and t >= 1:
                tact[1] = 1.0
            mu, sg = torch.from_numpy(mu_tab[:, t]), torch.from_numpy(sig_tab[:, t])
            st, done_o = O.admm_step(sd, st, mu, sg, tact)
            e.step(x, z, u, mu.cuda(), sg.cuda(), t_action=tact.cuda(), t_state=ts, done=done)
            # FLOAT TOLERANCE: f32 U-Net + FFTs against the f32 oracle, the bound of the trajectory tests
            for name, got, ref in (("x", x, st["x"]), ("z", z, st["z"]), ("u", u, st["u"])):
                d = got.cpu() - ref
                err = float((torch.view_as_real(d) if d.is_complex() else d).abs().max())
                assert err < 1e-4, (t, name, err)
            dp = (e.psnr(x, gt).cpu() - O.psnr(st["x"], st["gt"])[:, 0]).abs().max()
            assert float(dp) < 0.01, (t, float(dp))
            # finish_kernel: done = t_action > 0.5; t_state += 1/30 (f32) where not done
            d_exp = (tact > 0.5).numpy()
            assert np.array_equal(done.cpu().numpy(), d_exp.astype(np.uint8)) and np.array_equal(done_o.numpy(), d_exp)
            t_exp[~d_exp] += np.float32(1.0) / np.float32(30.0)
            assert np.array_equal(ts.cpu().numpy(), t_exp), (t, ts.cpu().numpy(), t_exp)
            if n == 2:
                if t == 0:
                    frozen = [v[1].clone() for v in (x, z, u)]
                else:
                    assert all(torch.equal(a[1], b) for a, b in zip((x, z, u), frozen)), t
    finally:
        e.close()
