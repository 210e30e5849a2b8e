"""Every caller-owned buffer of the C ABI (include/pnpadmm.h) inside guard bands (tests/guard_bands.py), on the GPU.

The value tests hand the library tensors that sit alone in a 512-byte-aligned torch allocation, so a store a few elements past the end
or before the start of a buffer lands in slack and every comparison still passes.  Here every tensor of every call - outputs and inputs
alike - is a view into the middle of a larger allocation with a band of a NaN-payload pattern on both sides, 16 bytes off 32-byte
alignment.  Each case asserts
  1. the call returns PNP_OK;
  2. both bands of every tensor hold the pattern and every input has the bits it had (compared as integers);
  3. every output is bit-identical to the same call made on ordinary torch tensors by a second handle of the same kind - which ties the
     guarded run to the values the rest of the suite verifies and catches a result that depends on 512-byte alignment.
No tolerance anywhere, no float64 reference: the other GPU tests own accuracy.  The one exception to (3) are the milliseconds of
pnp_profile_collect / pnp_profile_layers: two runs do not take the same time, so those arrays are checked for their bands, for finite
non-negative values, and the launch COUNTS are compared exactly.

Table 1: entry point -> guarded tensors (in = frozen input, out = output, io = both; "|NULL" = also run with the pointer NULL)
  pnp_reset                 in x0, y0, mask (mask_n 1 and N); out x, z, u                                     test_reset_and_set_kspace
  pnp_set_kspace            in y0, mask (mask_n 1 and N); (its effect: a pnp_prox_dual after it, bit for bit)  test_reset_and_set_kspace
  pnp_prox_dual             in mu, t_action|NULL, x; io z, u (single-coil: every stage variant of table 2)     test_prox_dual, test_multicoil
  pnp_step                  in mu, sigma_d, t_action|NULL; io x, z, u, t_state|NULL; out done|NULL             test_step, test_multicoil_step
  pnp_denoise               in x_in, sigma; out out - and io x with out == x_in                                test_denoise
  pnp_fft2c                 in in; out out - and io buf with out == in; batch n and n - 1                      test_fft2c, test_positive_control
  pnp_psnr                  in x, gt; out out[N]                                                               test_psnr_and_ssim
  pnp_ssim                  in x, gt; out out[N], map|NULL (radius 1, 8, 16)                                   test_psnr_and_ssim
  pnp_residuals             in x, z, u, prev|NULL; out out[N,6] (flags 0, DELTA, DC, both; multi-coil DC too)  test_residuals, test_multicoil
  pnp_acquire               in gt, mask (1, N); out y0, aty0|NULL, x0|NULL                                     test_acquire
  pnp_acquire_mc            in gt, sens (1, N), mask (1, N); out y0, aty0|NULL, x0|NULL                        test_acquire_mc
  pnp_set_kspace_mc         in y0, sens (1, N), mask (1, N)                                                    test_multicoil
  pnp_reset_mc              in x0, y0, sens, mask; out x, z, u                                                 test_multicoil
  pnp_mc_normal             in p, mu; out q                                                                    test_multicoil
  pnp_mc_cg_residual        out out[N]                                                                         test_multicoil
  pnp_estimate_sens         in y0; out sens (the transforms run in place in it), rss|NULL                      test_estimate_sens
  pnp_coil_compress_matrix  in y0; out cmat, eig, gram|NULL (complex128)                                       test_coil_compression
  pnp_coil_compress_apply   in in, cmat (cmat_n 1, N); out out                                                 test_coil_compression
  pnp_snapshot              in x, z, u, t_state|NULL; out dst (pnp_snapshot_bytes, uint8)                      test_snapshot_and_restore
  pnp_restore               in src; out x, z, u, t_state|NULL                                                  test_snapshot_and_restore
  pnp_unet_read_stage       out dst (NCHW), every stage 0..8 of a KEEP_STAGES handle; HOST out c, hh, ww       test_read_stage
  pnp_conv_algorithms       HOST out algo28 (int32[28])                                                        test_host_arrays
  pnp_profile_collect       HOST out total_ms (float64[6]), launches (int64[6])                                test_host_arrays
  pnp_profile_layers        HOST out layer_ms (float64[28]), layer_launches (int64[28])                        test_host_arrays
  (pnp_load_unet_weights reads a HOST blob only; pnp_create / pnp_destroy / pnp_last_error / pnp_version / pnp_mc_coils /
   pnp_snapshot_bytes / pnp_bf16_weight_terms / pnp_workspace_bytes / pnp_profile_reset take no caller buffer.)

Table 2: shape (N, H, W) -> launch function and variant.  rows/wg and cols/wg are the rows / columns one workgroup owns; with N >= 2 the
last workgroup of the grid owns the last rows / columns of the last plane.  "plain" = pnp_fft2c (and, through plain_fft2 with shift 0, the
same launches under pnp_acquire, pnp_residuals DC, pnp_estimate_sens and the multi-coil operator); "stage" = the three launches of the
single-coil pnp_prox_dual / pnp_step, which write z and u.
  power-of-two sides (fft_kernels.hip, namespace pow2)
    (2,16,16)     launch_fft_rows <0,0> 16 rows/wg (clipped to H); launch_fft_cols <0,0> 16 cols/wg; stage rows <1,0> / <2,0>, cols_prox <1,0>;
                  launch_fft_rows_real <3,0> (pnp_acquire, pnp_residuals DC)
    (2,16,1024)   rows <0,0> / <1,0> / <2,0> 2 rows/wg; cols <0,0> / <1,0> 16 cols/wg
    (2,1024,16)   rows <0,0> / <1,0> / <2,0> 128 rows/wg (ROW_ELEMS / W); cols <0,0> / <1,0> 4 cols/wg (73.8 KB of LDS)
    (2,64,32)     rows <0,0> / <1,0> / <2,0> 64 rows/wg (ROW_ELEMS / W); cols <0,0> / <1,0> 16 cols/wg
    (2,32,64)     rows <0,0> / <1,0> / <2,0> 32 rows/wg (all of H: one workgroup per plane); cols 16 cols/wg
    (2,64,64)     rows <0,0> / <1,0> / <2,0> 32 rows/wg (two workgroups per plane); cols 16 cols/wg; with (5,64,64) also <3,0> at 32 rows/wg
    (2,128,128)   rows <0,0> 16 rows/wg, stage rows <1,128> / <2,128>; cols <0,0>, stage cols_prox <1,128> 16 cols/wg
    (2,256,512)   rows <0,0> 4 rows/wg, stage rows <1,512,true> / <2,512,true> (radix-8 form, 4 rows/wg); cols <0,0>, cols_prox <1,256> 16 cols/wg
    (2,512,256)   rows <0,0> 8 rows/wg, stage rows <1,256,true> / <2,256,true> (radix-16 form, 16 rows/wg); cols <0,0>, cols_prox <1,512> 8 cols/wg
    (3,128,128) with PNP_SLICE128_MIN_N=1   launch_admm_slice128 (one workgroup per slice, writes z and u)
    (rows_per_block = min(H, 2048 / W) takes the values 2, 4, 8, 16, 32, 64, 128: W = 1024, 512, 256, 128 / 16 with H = 16, 64, 32, 16 with
    H >= 128; cols_per_block 16, 8, 4: H <= 256, 512, 1024.  The one-launch case asserts (0, 1, 0) booked launches, i.e. that the form ran.)
  a side that is not a power of two (fft_mixed_kernels.hip, namespace mixed): fft_rows_mixed_kernel<0|1|2>, fft_rows_real_m5_kernel,
  fft_cols_mixed_kernel<0|1>; rows/wg = mixed_rows_per_block(W), cols/wg = mixed_cols_per_block(H)
    (2,80,160)    8 rows/wg, 16 cols/wg            (2,160,80)   16 rows/wg, 16 cols/wg
    (2,16,800)    2 rows/wg, 16 cols/wg            (2,800,16)   16 rows/wg, 4 cols/wg
    (2,320,64)    16 rows/wg, 8 cols/wg            (2,64,400)   4 rows/wg, 16 cols/wg
    (2,16,80), (2,80,80), (2,80,32), (1,64,80) of the pointwise lists: 16 rows/wg, 16 cols/wg
  pointwise k-space kernels and reductions (grid pixel_chunks(H, W) x planes, 2048 pixels per workgroup, stores guarded by p < HW)
    (3,16,16) an eighth of a chunk; (2,16,80) 1280 pixels; (2,80,80) 3.125 chunks; (5,64,64) exactly two chunks;
    (65,16,16) one slice past a 64-thread workgroup of finish_kernel / sense_cgres_kernel ([N] outputs)
  denoiser: (1,16,48), (3,96,112), (2,80,48), (1,208,32) under default / PNP_NO_WINOGRAD / F(2x2) only / F(4x4) from 32 channels (also
    (2,256,144)) / bf16: conv_first_kernel and conv_last_kernel (or the last layer in layer 26's epilogue) read x and write out;
    (3,256,256) default: the fused first and last layer inside the F(4x4) kernel (algos[1] == algos[26] == 4);
    (16,256,256) bf16: the producer / consumer kernel (5 in algos) with its offloaded last layer
  multi-coil, coil maps, compression: (2,C,16,16), (2,C,80,32), (1,C,64,80), C in {1, 3, 32} (compression also 5 and 64:
    coilcomp_apply_kernel<8> for V <= 8, <16> for V <= 16, <32> above)"""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_bands as gb  # noqa: E402

from dt4image_restoration_amd import _lib, weights  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, C64, U8, F64, C128 = torch.float32, torch.complex64, torch.uint8, torch.float64, torch.complex128
SECOND_PATTERN = 0x7FA11CE5          # what a plane the call must not touch is pre-filled with (another NaN with a payload)

KS = [(3, 16, 16), (2, 16, 80), (2, 80, 80), (5, 64, 64)]      # pointwise k-space kernels and reductions
KS_N = KS + [(65, 16, 16)]                                      # ... and the [N] outputs
FFT = [(2, 16, 16), (2, 16, 1024), (2, 1024, 16), (2, 128, 128), (2, 256, 512), (2, 512, 256), (2, 80, 160), (2, 160, 80), (2, 16, 800),
       (2, 800, 16), (2, 320, 64), (2, 64, 400), (2, 64, 32), (2, 32, 64), (2, 64, 64)]
MC = [(2, 16, 16), (2, 80, 32), (1, 64, 80)]


def _ids(shapes):
    return ["x".join(str(v) for v in s) for s in shapes]


def _kind_shapes(shapes):
    """Every shape on a k-space-only handle; the first one also on an f32 and on a bf16 denoiser handle."""
    return [("kspace", s) for s in shapes] + [("f32", shapes[0]), ("bf16", shapes[0])]


def _ks_ids(cases):
    return [f"{k}-{'x'.join(str(v) for v in s)}" for k, s in cases]


# ---- engines and data ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sd_np():
    return weights.generate_unet_weights(0, "unit_gain")


class _Pair:
    """Two handles of one kind: `g` gets the guarded tensors, `p` the plain ones."""

    def __init__(self, kind, n, h, w, sd=None, **kw):
        from dt4image_restoration_amd.engine import PnPEngine
        self.engines = []
        for _ in range(2):
            e = PnPEngine(n, h, w, denoiser=(kind != "kspace"), bf16_convs=(kind == "bf16"), **kw)
            self.engines.append(e)
            if sd is not None:
                e.load_weights(sd)
        self.g, self.p = self.engines
        self.n, self.h, self.w = n, h, w

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        for e in self.engines:
            e.close()

    def both(self, fn):
        for e in self.engines:
            fn(e)


def _gen(*key):
    seed = 12345
    for v in key:
        seed = (seed * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _real(g, *shape, lo=0.0, hi=1.0):
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def _cplx(g, *shape, scale=1.0):
    return torch.view_as_complex((torch.rand(tuple(shape) + (2,), generator=g) * 2 - 1) * scale)


def _mask(g, *shape, p=0.35):
    return (torch.rand(shape, generator=g) < p).to(U8)


def _tact(n, stop):
    t = torch.zeros(n)
    t[stop] = 0.9
    return t


# ---- the guarded call --------------------------------------------------------------------------------------------------------------------

class A:
    """One pointer argument.  role: "in" (frozen), "io", "out", or None (passed as NULL)."""

    def __init__(self, name, role, init=None, shape=None, dtype=None, device=DEV):
        self.name, self.role, self.init, self.device = name, role, init, device
        self.shape = tuple(init.shape) if init is not None else (tuple(shape) if shape is not None else None)
        self.dtype = init.dtype if init is not None else dtype


def a_in(name, t):
    return A(name, "in", init=t)


def a_io(name, t):
    return A(name, "io", init=t)


def a_out(name, shape, dtype, device=DEV):
    return A(name, "out", shape=shape, dtype=dtype, device=device)


def a_null(name):
    return A(name, None)


def _ptrs(tensors):
    return {k: (None if v is None else v.data_ptr()) for k, v in tensors.items()}


def run_pair(pair, fn, args, what):
    """fn(engine, {name: pointer or None}) -> status, once on guarded tensors by pair.g and once on plain ones by pair.p: PNP_OK, bands and
    inputs intact, outputs bit-identical.  Returns (guarded, plain) tensors by name."""
    G, P = {}, {}
    for a in args:
        if a.role is None:
            G[a.name] = P[a.name] = None
        elif a.role == "out":
            G[a.name] = gb.guarded(a.shape, a.dtype, a.device, name=a.name)          # holds the pattern: an element left unwritten shows
            P[a.name] = torch.empty(a.shape, dtype=a.dtype, device=a.device)
        else:
            G[a.name] = gb.guarded(a.shape, a.dtype, a.device, fill=a.init, name=a.name)
            P[a.name] = a.init.detach().clone().to(a.device)
    outs = {a.name: G[a.name] for a in args if a.role in ("out", "io")}
    ins = {a.name: G[a.name] for a in args if a.role == "in"}
    for t in G.values():
        assert t is None or t.data_ptr() % 32 == 16
    with gb.watch(outputs=outs, inputs=ins):
        rc = fn(pair.g, _ptrs(G))
        assert rc == 0, (what, rc, pair.g.lib.pnp_last_error().decode())
    rc = fn(pair.p, _ptrs(P))
    assert rc == 0, (what, rc, pair.p.lib.pnp_last_error().decode())
    torch.cuda.synchronize()
    for name in outs:
        assert torch.equal(gb.as_bytes(G[name]), gb.as_bytes(P[name])), f"{what}: {name} differs between the guarded and the plain call"
    return G, P


def _optional(present, arg):
    return arg if present else a_null(arg.name)


# ---- single coil: reset, set_kspace, prox_dual, step -------------------------------------------------------------------------------------

def _reset_fn(mask_n):
    return lambda e, p: e.lib.pnp_reset(e._h, p["x0"], p["y0"], p["mask"], mask_n, p["x"], p["z"], p["u"], e._stream())


def _prox_fn(e, p):
    return e.lib.pnp_prox_dual(e._h, p["mu"], p["t_action"], p["x"], p["z"], p["u"], e._stream())


def _prox_args(g, n, h, w, stop=None):
    return [a_in("mu", _real(g, n, lo=0.0, hi=1.0)), a_null("t_action") if stop is None else a_in("t_action", _tact(n, stop)),
            a_in("x", _real(g, n, 1, h, w)), a_io("z", _cplx(g, n, 1, h, w)), a_io("u", _cplx(g, n, 1, h, w, scale=0.5))]


@pytest.mark.parametrize("kind,shape", _kind_shapes(KS), ids=_ks_ids(_kind_shapes(KS)))
def test_reset_and_set_kspace(kind, shape):
    n, h, w = shape
    g = _gen(1, n, h, w)
    with _Pair(kind, n, h, w) as pair:
        for mask_n in (1, n):
            mshape = (h, w) if mask_n == 1 else (n, h, w)
            run_pair(pair, _reset_fn(mask_n),
                     [a_in("x0", _cplx(g, n, 1, h, w)), a_in("y0", _cplx(g, n, 1, h, w)), a_in("mask", _mask(g, *mshape)),
                      a_out("x", (n, 1, h, w), F32), a_out("z", (n, 1, h, w), C64), a_out("u", (n, 1, h, w), C64)], f"pnp_reset mask_n={mask_n}")
            # the constants it stored: a data-fidelity step on both handles
            run_pair(pair, _prox_fn, _prox_args(g, n, h, w), "pnp_prox_dual after pnp_reset")
            # other constants through pnp_set_kspace, the caller's y0 and mask unchanged, then the same step
            other_n = n if mask_n == 1 else 1
            run_pair(pair, lambda e, p: e.lib.pnp_set_kspace(e._h, p["y0"], p["mask"], other_n, e._stream()),
                     [a_in("y0", _cplx(g, n, 1, h, w)), a_in("mask", _mask(g, *((h, w) if other_n == 1 else (n, h, w)), p=0.6))],
                     f"pnp_set_kspace mask_n={other_n}")
            run_pair(pair, _prox_fn, _prox_args(g, n, h, w, stop=n - 1), "pnp_prox_dual after pnp_set_kspace")


def _install(pair, g, n, h, w, per_slice=False):
    x0, y0 = _cplx(g, n, 1, h, w).to(DEV), _cplx(g, n, 1, h, w).to(DEV)
    mask = _mask(g, *((n, h, w) if per_slice else (h, w))).to(DEV)
    pair.both(lambda e: e.reset(x0, y0, mask))


PROX_CASES = [("kspace", s, {}) for s in KS_N + FFT] + [("f32", KS[0], {}), ("bf16", KS[0], {}),
                                                        ("kspace", (3, 128, 128), {"PNP_SLICE128_MIN_N": "1"}),
                                                        ("f32", (3, 128, 128), {"PNP_SLICE128_MIN_N": "1"})]


@pytest.mark.parametrize("kind,shape,env", PROX_CASES, ids=[f"{k}-{'x'.join(map(str, s))}{'-' + '-'.join(e) if e else ''}" for k, s, e in PROX_CASES])
def test_prox_dual(kind, shape, env, monkeypatch):
    """The data-fidelity stage writes z and u from its row kernels (or the one-launch form): every stage variant of table 2.  Both handles
    profile, and every call is asserted to be the form the case is about: the one-launch form (launch_admm_slice128) books
    (fft_rows, fft_cols_prox, other) = (0, 1, 0) launches, the three-launch path (2, 1, 0)."""
    n, h, w = shape
    g = _gen(2, n, h, w)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with _Pair(kind, n, h, w, profile=True) as pair:
        for k in env:
            monkeypatch.delenv(k)
        for per_slice, stop in ((False, None), (True, n - 1), (False, 0)):
            _install(pair, g, n, h, w, per_slice)
            torch.cuda.synchronize()
            pair.both(lambda e: e.profile_reset())
            G, _ = run_pair(pair, _prox_fn, _prox_args(g, n, h, w, stop=stop), f"pnp_prox_dual stop={stop}")
            assert not bool(torch.isnan(torch.view_as_real(G["z"])).any())
            for e in pair.engines:
                prof = e.profile_collect()
                booked = tuple(prof[k]["launches"] for k in ("fft_rows", "fft_cols_prox", "other"))
                assert booked == ((0, 1, 0) if env else (2, 1, 0)), (booked, env)


@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("shape", KS_N, ids=_ids(KS_N))
def test_step(sd_np, kind, shape):
    """pnp_step: t_state and done present and NULL (finish_kernel: (N + 63) / 64 workgroups of 64), one slice stopped."""
    n, h, w = shape
    g = _gen(3, n, h, w)
    with _Pair(kind, n, h, w, sd=sd_np) as pair:
        _install(pair, g, n, h, w)

        def step(e, p):
            return e.lib.pnp_step(e._h, p["mu"], p["sigma_d"], p["t_action"], p["x"], p["z"], p["u"], p["t_state"], p["done"], e._stream())

        for has_ts, has_done, stop in ((True, True, n - 1), (False, False, n - 1), (True, False, 0), (False, True, None)):
            z0 = _cplx(g, n, 1, h, w) * 0.5 + 0.5
            args = [a_in("mu", _real(g, n)), a_in("sigma_d", _real(g, n, lo=5 / 255, hi=50 / 255)),
                    a_null("t_action") if stop is None else a_in("t_action", _tact(n, stop)),
                    a_io("x", _real(g, n, 1, h, w)), a_io("z", z0), a_io("u", _cplx(g, n, 1, h, w, scale=0.1)),
                    _optional(has_ts, a_io("t_state", _real(g, n))), _optional(has_done, a_out("done", (n,), U8))]
            G, _ = run_pair(pair, step, args, f"pnp_step t_state={has_ts} done={has_done} stop={stop}")
            if has_done:
                want = torch.zeros(n, dtype=U8) if stop is None else (_tact(n, stop) > 0.5).to(U8)
                assert torch.equal(G["done"].cpu(), want)
            if stop is not None:                            # the stopped slice keeps x, z, u (and t_state) bit for bit
                for a in args:
                    if a.role == "io":
                        assert torch.equal(gb.as_bytes(G[a.name][stop]), gb.as_bytes(a.init[stop].to(DEV))), a.name


# ---- the denoiser ------------------------------------------------------------------------------------------------------------------------

DENOISE_MODES = {
    "default": ("f32", {}),
    "direct": ("f32", {"PNP_NO_WINOGRAD": "1"}),
    "wino2": ("f32", {"PNP_WINO_MIN_BLOCKS": "1", "PNP_NO_WINO_F4": "1"}),
    "wino4": ("f32", {"PNP_WINO_MIN_BLOCKS": "1", "PNP_WINO_F4_MIN_CIN": "32"}),
    "bf16": ("bf16", {}),
}
DENOISE_SHAPES = [(1, 16, 48), (3, 96, 112), (2, 80, 48), (1, 208, 32)]
DENOISE_CASES = [(m, s) for m in DENOISE_MODES for s in DENOISE_SHAPES] + [("wino4", (2, 256, 144)), ("default", (3, 256, 256)),
                                                                          ("bf16", (16, 256, 256))]


@pytest.mark.parametrize("mode,shape", DENOISE_CASES, ids=[f"{m}-{'x'.join(map(str, s))}" for m, s in DENOISE_CASES])
def test_denoise(sd_np, mode, shape, monkeypatch):
    """pnp_denoise out of place and with out == x_in: the first layer reads x and the last writes out from whatever kernel the plan gives them."""
    n, h, w = shape
    kind, env = DENOISE_MODES[mode]
    g = _gen(4, n, h, w)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with _Pair(kind, n, h, w, sd=sd_np) as pair:
        for k in env:
            monkeypatch.delenv(k)
        algos = pair.g.conv_algorithms()
        assert algos == pair.p.conv_algorithms()
        if mode == "direct":
            assert all(v == 0 for v in algos[1:27])
        if mode == "wino2":
            assert 1 in algos and 4 not in algos
        if mode == "wino4":
            assert 4 in algos
        if (mode, shape) == ("default", (3, 256, 256)):
            assert algos[1] == 4 and algos[26] == 4          # the fused first and last layer read x and write out themselves
        if (mode, shape) == ("bf16", (16, 256, 256)):
            assert 5 in algos                                # the producer / consumer kernel with its offloaded last layer
        x, sigma = _real(g, n, 1, h, w), _real(g, n, lo=5 / 255, hi=50 / 255)
        G, _ = run_pair(pair, lambda e, p: e.lib.pnp_denoise(e._h, p["x_in"], p["sigma"], p["out"], e._stream()),
                        [a_in("x_in", x), a_in("sigma", sigma), a_out("out", (n, 1, h, w), F32)], "pnp_denoise")
        out = G["out"]
        assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0       # every pixel written (the band pattern is NaN) and clamped
        G2, _ = run_pair(pair, lambda e, p: e.lib.pnp_denoise(e._h, p["x"], p["sigma"], p["x"], e._stream()),
                         [a_io("x", x), a_in("sigma", sigma)], "pnp_denoise out == x_in")
        assert torch.equal(gb.as_bytes(G2["x"]), gb.as_bytes(out))


# ---- pnp_fft2c ---------------------------------------------------------------------------------------------------------------------------

def _fft_fn(batch, h, w, inverse, in_place):
    if in_place:
        return lambda e, p: e.lib.pnp_fft2c(e._h, p["buf"], p["buf"], batch, h, w, inverse, e._stream())
    return lambda e, p: e.lib.pnp_fft2c(e._h, p["in"], p["out"], batch, h, w, inverse, e._stream())


@pytest.mark.parametrize("kind,shape", _kind_shapes(FFT), ids=_ks_ids(_kind_shapes(FFT)))
def test_fft2c(kind, shape):
    """Both directions, in place and out of place, at batch n; then batch n - 1 on guarded views of n planes whose last plane holds a second
    pattern and must keep it."""
    n, h, w = shape
    g = _gen(5, n, h, w)
    with _Pair(kind, n, h, w) as pair:
        src = _cplx(g, n, h, w)
        for inverse in (0, 1):
            G, _ = run_pair(pair, _fft_fn(n, h, w, inverse, False), [a_in("in", src), a_out("out", (n, h, w), C64)], f"pnp_fft2c inverse={inverse}")
            G2, _ = run_pair(pair, _fft_fn(n, h, w, inverse, True), [a_io("buf", src)], f"pnp_fft2c in place inverse={inverse}")
            assert torch.equal(gb.as_bytes(G2["buf"]), gb.as_bytes(G["out"]))
            # batch n - 1: the last plane of the caller's n-plane views is not the call's
            b = n - 1
            second = torch.full((h, w, 2), SECOND_PATTERN, dtype=torch.int32).view(F32)
            tail = torch.view_as_complex(second)
            full_in = torch.cat([src[:b], tail[None]])
            gin = gb.guarded((n, h, w), C64, DEV, fill=full_in, name="in")
            gout = gb.guarded((n, h, w), C64, DEV, name="out")
            gout[b].copy_(tail)
            gbuf = gb.guarded((n, h, w), C64, DEV, fill=full_in, name="buf")
            e = pair.g
            with gb.watch(outputs={"out": gout, "buf": gbuf}, inputs={"in": gin}):
                assert e.lib.pnp_fft2c(e._h, gin.data_ptr(), gout.data_ptr(), b, h, w, inverse, e._stream()) == 0
                assert e.lib.pnp_fft2c(e._h, gbuf.data_ptr(), gbuf.data_ptr(), b, h, w, inverse, e._stream()) == 0
            want_tail = gb.as_bytes(tail.to(DEV))
            assert torch.equal(gb.as_bytes(gout[b]), want_tail) and torch.equal(gb.as_bytes(gbuf[b]), want_tail), "the plane past the batch was written"
            assert torch.equal(gb.as_bytes(gout[:b]), gb.as_bytes(G["out"][:b])) and torch.equal(gb.as_bytes(gbuf[:b]), gb.as_bytes(G["out"][:b]))


# one test, two shapes: the power-of-two and the mixed-radix family store through different kernels (fft_cols_kernel<0,0>,
# fft_cols_mixed_kernel<0>), and the control shows the harness seeing each of them; both stay inside the band the test owns
@pytest.mark.parametrize("shape", [(2, 16, 16), (2, 80, 160)], ids=_ids([(2, 16, 16), (2, 80, 160)]))
def test_positive_control(shape):
    """The harness sees a real device store outside a view: pnp_fft2c with batch = 2 and an output that is a guarded view of ONE plane.  The
    second plane of the result lands in the trailing band, which is at least one plane wide (max(4096, H W) elements), so every store
    stays inside the test's own allocation; the report names the side, the offset H W and the count H W."""
    n, h, w = shape
    g = _gen(6, n, h, w)
    with _Pair("kspace", n, h, w) as pair:
        e = pair.g
        gin = gb.guarded((n, h, w), C64, DEV, fill=_cplx(g, n, h, w), name="in")
        gout = gb.guarded((1, h, w), C64, DEV, name="out")
        g_info = gout._guard
        assert g_info.raw.numel() - g_info.start - g_info.nbytes >= h * w * 8        # the band holds the whole second plane
        with pytest.raises(gb.GuardBandError) as ei:
            with gb.watch(outputs={"out": gout}, inputs={"in": gin}):
                assert e.lib.pnp_fft2c(e._h, gin.data_ptr(), gout.data_ptr(), n, h, w, 0, e._stream()) == 0
        assert str(ei.value) == f"out: trailing band touched: first at offset {h * w} (elements, relative to the view), {h * w} elements touched"
        # and what landed there is the second plane of the transform
        want = pair.p.fft2c(gin.clone())
        end = g_info.start + g_info.nbytes
        assert torch.equal(g_info.raw[end:end + h * w * 8], gb.as_bytes(want[1]))
        assert torch.equal(gb.as_bytes(gout[0]), gb.as_bytes(want[0]))


# ---- metrics -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,shape", _kind_shapes(KS_N), ids=_ks_ids(_kind_shapes(KS_N)))
def test_psnr_and_ssim(kind, shape):
    n, h, w = shape
    g = _gen(7, n, h, w)
    with _Pair(kind, n, h, w) as pair:
        x, gt = _real(g, n, 1, h, w, lo=-0.3, hi=1.3), _real(g, n, 1, h, w)
        run_pair(pair, lambda e, p: e.lib.pnp_psnr(e._h, p["x"], p["gt"], p["out"], e._stream()),
                 [a_in("x", x), a_in("gt", gt), a_out("out", (n,), F32)], "pnp_psnr")
        for radius in (1, 8, 16):
            for has_map in (True, False):
                G, _ = run_pair(pair, lambda e, p: e.lib.pnp_ssim(e._h, p["x"], p["gt"], 1.0, 0.01, 0.03, radius, _lib.PNP_SSIM_CLAMP_X, p["out"],
                                                                   p["map"], e._stream()),
                                [a_in("x", x), a_in("gt", gt), a_out("out", (n,), F32), _optional(has_map, a_out("map", (n, h, w), F32))],
                                f"pnp_ssim radius={radius} map={has_map}")
                assert not bool(torch.isnan(G["out"]).any()) and (not has_map or not bool(torch.isnan(G["map"]).any()))


def _snap_bytes(x, z, u, t):
    return torch.cat([gb.as_bytes(v.contiguous()) for v in (x, z, u, t)])


@pytest.mark.parametrize("kind,shape", _kind_shapes(KS_N), ids=_ks_ids(_kind_shapes(KS_N)))
def test_residuals(kind, shape):
    n, h, w = shape
    g = _gen(8, n, h, w)
    with _Pair(kind, n, h, w) as pair:
        _install(pair, g, n, h, w, per_slice=True)
        assert pair.g.lib.pnp_snapshot_bytes(pair.g._h) == 4 * n * h * w * 5 + 4 * n
        x, z, u = _real(g, n, 1, h, w), _cplx(g, n, 1, h, w), _cplx(g, n, 1, h, w)
        prev = _snap_bytes(_real(g, n, 1, h, w), _cplx(g, n, 1, h, w), _cplx(g, n, 1, h, w), _real(g, n))
        for flags in (0, _lib.PNP_RES_DELTA, _lib.PNP_RES_DC, _lib.PNP_RES_DELTA | _lib.PNP_RES_DC):
            G, _ = run_pair(pair, lambda e, p: e.lib.pnp_residuals(e._h, p["x"], p["z"], p["u"], p["prev"], flags, p["out"], e._stream()),
                            [a_in("x", x), a_in("z", z), a_in("u", u), _optional(flags & _lib.PNP_RES_DELTA, a_in("prev", prev)),
                             a_out("out", (n, _lib.PNP_RES_COLS), F32)], f"pnp_residuals flags={flags}")
            out = G["out"].cpu()
            assert not bool(torch.isnan(out).any())                             # all six columns written
            assert bool((out[:, 0] > 0).all())
            for cols, flag in ((out[:, 1:5], _lib.PNP_RES_DELTA), (out[:, 5], _lib.PNP_RES_DC)):     # asked for: positive; not asked for: written as 0
                assert bool((cols > 0).all()) if flags & flag else not bool(cols.any())


@pytest.mark.parametrize("kind,shape", _kind_shapes(KS_N), ids=_ks_ids(_kind_shapes(KS_N)))
def test_snapshot_and_restore(kind, shape):
    n, h, w = shape
    g = _gen(9, n, h, w)
    with _Pair(kind, n, h, w) as pair:
        nbytes = pair.g.lib.pnp_snapshot_bytes(pair.g._h)
        x, z, u, t = _real(g, n, 1, h, w), _cplx(g, n, 1, h, w), _cplx(g, n, 1, h, w), _real(g, n)
        for has_t in (True, False):
            G, _ = run_pair(pair, lambda e, p: e.lib.pnp_snapshot(e._h, p["x"], p["z"], p["u"], p["t_state"], p["dst"], e._stream()),
                            [a_in("x", x), a_in("z", z), a_in("u", u), _optional(has_t, a_in("t_state", t)), a_out("dst", (nbytes,), U8)],
                            f"pnp_snapshot t_state={has_t}")
            packed = _snap_bytes(x, z, u, t if has_t else torch.zeros(n))
            assert torch.equal(G["dst"].cpu(), packed)
            t_before = _real(g, n)
            R, _ = run_pair(pair, lambda e, p: e.lib.pnp_restore(e._h, p["src"], p["x"], p["z"], p["u"], p["t_state"], e._stream()),
                            [a_in("src", packed), a_out("x", (n, 1, h, w), F32), a_out("z", (n, 1, h, w), C64), a_out("u", (n, 1, h, w), C64),
                             _optional(has_t, a_io("t_state", t_before))], f"pnp_restore t_state={has_t}")
            for name, want in (("x", x), ("z", z), ("u", u)) + ((("t_state", t),) if has_t else ()):
                assert torch.equal(gb.as_bytes(R[name].cpu()), gb.as_bytes(want)), name


# ---- acquisition ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,shape", _kind_shapes(KS), ids=_ks_ids(_kind_shapes(KS)))
def test_acquire(kind, shape):
    n, h, w = shape
    g = _gen(10, n, h, w)
    with _Pair(kind, n, h, w) as pair:
        gt = _real(g, n, 1, h, w)
        for mask_n, has_aty, has_x0 in ((1, True, True), (n, False, False), (n, True, False), (1, False, True)):
            mask = _mask(g, *((h, w) if mask_n == 1 else (n, h, w)))
            G, _ = run_pair(pair, lambda e, p: e.lib.pnp_acquire(e._h, p["gt"], p["mask"], mask_n, 0.02, 7, 0, p["y0"], p["aty0"], p["x0"], e._stream()),
                            [a_in("gt", gt), a_in("mask", mask), a_out("y0", (n, 1, h, w), C64), _optional(has_aty, a_out("aty0", (n, 1, h, w), C64)),
                             _optional(has_x0, a_out("x0", (n, 1, h, w), C64))], f"pnp_acquire mask_n={mask_n} aty0={has_aty} x0={has_x0}")
            y0 = G["y0"].cpu().reshape(n, h, w)
            assert bool((y0[(mask == 0).expand(n, h, w)] == 0).all()) and not bool(torch.isnan(torch.view_as_real(y0)).any())


def _sens(g, sens_n, c, h, w):
    return _cplx(g, *((c, h, w) if sens_n == 1 else (sens_n, c, h, w)), scale=0.7)


MC_CASES = [(s, c) for s in MC for c in (1, 3, 32)]
MC_IDS = [f"{'x'.join(map(str, s))}-C{c}" for s, c in MC_CASES]


@pytest.mark.parametrize("shape,c", MC_CASES, ids=MC_IDS)
def test_acquire_mc(shape, c):
    n, h, w = shape
    g = _gen(11, n, h, w, c)
    with _Pair("kspace", n, h, w) as pair:
        gt = _real(g, n, 1, h, w)
        for mask_n, sens_n, has_aty, has_x0 in ((1, 1, True, True), (n, n, False, False), (n, 1, True, False), (1, n, False, True)):
            mask = _mask(g, *((h, w) if mask_n == 1 else (n, h, w)))
            run_pair(pair, lambda e, p: e.lib.pnp_acquire_mc(e._h, p["gt"], p["sens"], c, sens_n, p["mask"], mask_n, 0.02, 11, 0, p["y0"], p["aty0"],
                                                             p["x0"], e._stream()),
                     [a_in("gt", gt), a_in("sens", _sens(g, sens_n, c, h, w)), a_in("mask", mask), a_out("y0", (n, c, h, w), C64),
                      _optional(has_aty, a_out("aty0", (n, 1, h, w), C64)), _optional(has_x0, a_out("x0", (n, 1, h, w), C64))],
                     f"pnp_acquire_mc mask_n={mask_n} sens_n={sens_n} aty0={has_aty} x0={has_x0}")


# ---- the multi-coil stage ---------------------------------------------------------------------------------------------------------------------

def _mc_prox_args(g, n, h, w, stop):
    return [a_in("mu", _real(g, n, lo=0.05, hi=1.0)), a_null("t_action") if stop is None else a_in("t_action", _tact(n, stop)),
            a_in("x", _real(g, n, 1, h, w)), a_io("z", _cplx(g, n, 1, h, w)), a_io("u", _cplx(g, n, 1, h, w, scale=0.5))]


MC_STAGE_CASES = [("kspace", s, c) for s, c in MC_CASES] + [("kspace", (65, 16, 16), 3), ("f32", MC[0], 3), ("bf16", MC[0], 3)]


@pytest.mark.parametrize("kind,shape,c", MC_STAGE_CASES, ids=[f"{k}-{'x'.join(map(str, s))}-C{c}" for k, s, c in MC_STAGE_CASES])
def test_multicoil(kind, shape, c):
    """pnp_set_kspace_mc, pnp_reset_mc, pnp_mc_normal, pnp_prox_dual (the CG solve), pnp_mc_cg_residual and pnp_residuals' multi-coil DC column."""
    n, h, w = shape
    g = _gen(12, n, h, w, c)
    cg = 3
    with _Pair(kind, n, h, w) as pair:
        for sens_n, mask_n in ((1, n), (n, 1)):
            sens, mask = _sens(g, sens_n, c, h, w), _mask(g, *((h, w) if mask_n == 1 else (n, h, w)))
            y0 = _cplx(g, n, c, h, w)
            run_pair(pair, lambda e, p: e.lib.pnp_reset_mc(e._h, p["x0"], p["y0"], p["sens"], c, sens_n, p["mask"], mask_n, cg, p["x"], p["z"], p["u"],
                                                           e._stream()),
                     [a_in("x0", _cplx(g, n, 1, h, w)), a_in("y0", y0), a_in("sens", sens), a_in("mask", mask), a_out("x", (n, 1, h, w), F32),
                      a_out("z", (n, 1, h, w), C64), a_out("u", (n, 1, h, w), C64)], f"pnp_reset_mc sens_n={sens_n} mask_n={mask_n}")
            assert pair.g.coils == c
            run_pair(pair, lambda e, p: e.lib.pnp_mc_normal(e._h, p["p"], p["mu"], p["q"], e._stream()),
                     [a_in("p", _cplx(g, n, 1, h, w)), a_in("mu", _real(g, n)), a_out("q", (n, 1, h, w), C64)], "pnp_mc_normal")
            run_pair(pair, _prox_fn, _mc_prox_args(g, n, h, w, None), "pnp_prox_dual (multi-coil)")
            R, _ = run_pair(pair, lambda e, p: e.lib.pnp_mc_cg_residual(e._h, p["out"], e._stream()), [a_out("out", (n,), F32)], "pnp_mc_cg_residual")
            assert not bool(torch.isnan(R["out"]).any())
            # other constants through pnp_set_kspace_mc, then a solve with one slice stopped
            run_pair(pair, lambda e, p: e.lib.pnp_set_kspace_mc(e._h, p["y0"], p["sens"], c, sens_n, p["mask"], mask_n, cg, e._stream()),
                     [a_in("y0", _cplx(g, n, c, h, w)), a_in("sens", _sens(g, sens_n, c, h, w)), a_in("mask", mask)],
                     f"pnp_set_kspace_mc sens_n={sens_n} mask_n={mask_n}")
            run_pair(pair, _prox_fn, _mc_prox_args(g, n, h, w, n - 1), "pnp_prox_dual (multi-coil, one slice stopped)")
            run_pair(pair, lambda e, p: e.lib.pnp_mc_cg_residual(e._h, p["out"], e._stream()), [a_out("out", (n,), F32)], "pnp_mc_cg_residual")
            run_pair(pair, lambda e, p: e.lib.pnp_residuals(e._h, p["x"], p["z"], p["u"], None, _lib.PNP_RES_DC, p["out"], e._stream()),
                     [a_in("x", _real(g, n, 1, h, w)), a_in("z", _cplx(g, n, 1, h, w)), a_in("u", _cplx(g, n, 1, h, w)),
                      a_out("out", (n, _lib.PNP_RES_COLS), F32)], "pnp_residuals DC (multi-coil)")


@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("c", [3, 32])
def test_multicoil_step(sd_np, kind, c):
    """pnp_step on a multi-coil handle, C = 3 and C = 32 (the solve at the header's PNP_MC_MAX_COILS)."""
    n, h, w = 2, 16, 16
    g = _gen(13, c)
    with _Pair(kind, n, h, w, sd=sd_np) as pair:
        x0, y0, sens, mask = _cplx(g, n, 1, h, w).to(DEV), _cplx(g, n, c, h, w).to(DEV), _sens(g, n, c, h, w).to(DEV), _mask(g, h, w).to(DEV)
        pair.both(lambda e: e.reset(x0, y0, mask, sens=sens, cg_iters=4))
        for has_opt, stop in ((True, 1), (False, None)):
            args = [a_in("mu", _real(g, n, lo=0.05)), a_in("sigma_d", _real(g, n, lo=5 / 255, hi=50 / 255)),
                    a_null("t_action") if stop is None else a_in("t_action", _tact(n, stop)),
                    a_io("x", _real(g, n, 1, h, w)), a_io("z", _cplx(g, n, 1, h, w) * 0.5 + 0.5), a_io("u", _cplx(g, n, 1, h, w, scale=0.1)),
                    _optional(has_opt, a_io("t_state", _real(g, n))), _optional(has_opt, a_out("done", (n,), U8))]
            run_pair(pair, lambda e, p: e.lib.pnp_step(e._h, p["mu"], p["sigma_d"], p["t_action"], p["x"], p["z"], p["u"], p["t_state"], p["done"],
                                                       e._stream()), args, f"pnp_step (multi-coil C={c})")
            run_pair(pair, lambda e, p: e.lib.pnp_mc_cg_residual(e._h, p["out"], e._stream()), [a_out("out", (n,), F32)], "pnp_mc_cg_residual")


# ---- coil maps and coil compression ----------------------------------------------------------------------------------------------------------

SENS_CASES = [("kspace", s, c) for s, c in MC_CASES] + [("f32", MC[0], 3), ("bf16", MC[0], 3)]


@pytest.mark.parametrize("kind,shape,c", SENS_CASES, ids=[f"{k}-{'x'.join(map(str, s))}-C{c}" for k, s, c in SENS_CASES])
def test_estimate_sens(kind, shape, c):
    """The inverse transform runs IN PLACE in the caller's sens buffer at batch N * C: column pass, then row pass, each workgroup owning
    whole rows / columns of it."""
    n, h, w = shape
    g = _gen(14, n, h, w, c)
    with _Pair(kind, n, h, w) as pair:
        y0 = _cplx(g, n, c, h, w)
        for acs, window, has_rss in (((h, w), _lib.PNP_SENS_HANN, True), ((2, 2), _lib.PNP_SENS_BOX, False), ((8, 6), _lib.PNP_SENS_BOX, True),
                                     ((h, 2), _lib.PNP_SENS_HANN, False)):
            G, _ = run_pair(pair, lambda e, p: e.lib.pnp_estimate_sens(e._h, p["y0"], c, acs[0], acs[1], window, 0.05, 0, p["sens"], p["rss"],
                                                                       e._stream()),
                            [a_in("y0", y0), a_out("sens", (n, c, h, w), C64), _optional(has_rss, a_out("rss", (n, h, w), F32))],
                            f"pnp_estimate_sens acs={acs} window={window} rss={has_rss}")
            assert not bool(torch.isnan(torch.view_as_real(G["sens"])).any())


CC_CASES = [(s, c) for s in MC for c in (1, 3, 5, 32, 64)]


@pytest.mark.parametrize("shape,c", CC_CASES, ids=[f"{'x'.join(map(str, s))}-C{c}" for s, c in CC_CASES])
def test_coil_compression(shape, c):
    n, h, w = shape
    g = _gen(15, n, h, w, c)
    with _Pair("kspace", n, h, w) as pair:
        y0 = _cplx(g, n, c, h, w)
        cmat = None
        for acs, has_gram in (((h, w), True), ((8, 6), False)):
            G, _ = run_pair(pair, lambda e, p: e.lib.pnp_coil_compress_matrix(e._h, p["y0"], c, acs[0], acs[1], 0, p["cmat"], p["eig"], p["gram"],
                                                                              e._stream()),
                            [a_in("y0", y0), a_out("cmat", (n, c, c), C64), a_out("eig", (n, c), F32), _optional(has_gram, a_out("gram", (n, c, c), C128))],
                            f"pnp_coil_compress_matrix acs={acs} gram={has_gram}")
            cmat = G["cmat"].cpu()
            assert not bool(torch.isnan(G["eig"]).any()) and not bool(torch.isnan(torch.view_as_real(cmat)).any())
        vmax = min(c, _lib.PNP_MC_MAX_COILS)
        for v in sorted({1, vmax, min(vmax, 12), (vmax + 1) // 2}):       # <8>, the largest, and one in between (<16> from C = 32 on)
            for cmat_n in (1, n):
                m = cmat if cmat_n == n else cmat[0]
                run_pair(pair, lambda e, p: e.lib.pnp_coil_compress_apply(e._h, p["in"], c, p["cmat"], cmat_n, v, p["out"], e._stream()),
                         [a_in("in", y0), a_in("cmat", m.contiguous()), a_out("out", (n, v, h, w), C64)], f"pnp_coil_compress_apply V={v} cmat_n={cmat_n}")


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_coil_compression_on_denoiser_handles(kind):
    n, h, w, c = 2, 16, 16, 5
    g = _gen(16)
    with _Pair(kind, n, h, w) as pair:
        y0 = _cplx(g, n, c, h, w)
        G, _ = run_pair(pair, lambda e, p: e.lib.pnp_coil_compress_matrix(e._h, p["y0"], c, 8, 8, 0, p["cmat"], p["eig"], p["gram"], e._stream()),
                        [a_in("y0", y0), a_out("cmat", (n, c, c), C64), a_out("eig", (n, c), F32), a_out("gram", (n, c, c), C128)],
                        "pnp_coil_compress_matrix")
        run_pair(pair, lambda e, p: e.lib.pnp_coil_compress_apply(e._h, p["in"], c, p["cmat"], n, 3, p["out"], e._stream()),
                 [a_in("in", y0), a_in("cmat", G["cmat"].cpu()), a_out("out", (n, 3, h, w), C64)], "pnp_coil_compress_apply")
        run_pair(pair, lambda e, p: e.lib.pnp_acquire_mc(e._h, p["gt"], p["sens"], c, 1, p["mask"], 1, 0.01, 3, 0, p["y0"], p["aty0"], p["x0"], e._stream()),
                 [a_in("gt", _real(g, n, 1, h, w)), a_in("sens", _sens(g, 1, c, h, w)), a_in("mask", _mask(g, h, w)), a_out("y0", (n, c, h, w), C64),
                  a_out("aty0", (n, 1, h, w), C64), a_out("x0", (n, 1, h, w), C64)], "pnp_acquire_mc")


# ---- introspection ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 16, 48), (1, 80, 32)], ids=_ids([(2, 16, 48), (1, 80, 32)]))
def test_read_stage(sd_np, kind, shape):
    """pnp_unet_read_stage writes NCHW from the engine's NHWC planes: every stage a KEEP_STAGES handle holds, the three HOST ints guarded too."""
    n, h, w = shape
    g = _gen(17, n, h, w)
    with _Pair(kind, n, h, w, sd=sd_np, keep_stages=True) as pair:
        x, sigma = _real(g, n, 1, h, w).to(DEV), _real(g, n, lo=5 / 255, hi=50 / 255).to(DEV)
        pair.both(lambda e: e.denoise(x, sigma))
        for which in range(9):
            dims = {k: gb.guarded((1,), torch.int32, "cpu", name=k) for k in ("c", "hh", "ww")}
            ip = {k: C.cast(v.data_ptr(), C.POINTER(C.c_int)) for k, v in dims.items()}
            e = pair.g
            with gb.watch(outputs=dims):
                assert e.lib.pnp_unet_read_stage(e._h, which, None, ip["c"], ip["hh"], ip["ww"], e._stream()) == 0
            c, hh, ww = (int(dims[k]) for k in ("c", "hh", "ww"))
            lvl = which if which <= 4 else 8 - which
            assert (hh, ww) == (h >> lvl, w >> lvl) and c == 32 << lvl
            G, _ = run_pair(pair, lambda e, p: e.lib.pnp_unet_read_stage(e._h, which, p["dst"], None, None, None, e._stream()),
                            [a_out("dst", (n, c, hh, ww), F32)], f"pnp_unet_read_stage {which}")
            assert not bool(torch.isnan(G["dst"]).any())


def test_host_arrays(sd_np):
    """The HOST arrays of pnp_conv_algorithms, pnp_profile_collect and pnp_profile_layers, guarded like the device buffers."""
    n, h, w = 2, 16, 80
    g = _gen(18)
    with _Pair("f32", n, h, w, sd=sd_np, profile=True, profile_layers=True) as pair:
        def cast(ptr, ctype):
            return C.cast(ptr, C.POINTER(ctype))

        G, _ = run_pair(pair, lambda e, p: e.lib.pnp_conv_algorithms(e._h, cast(p["algo28"], C.c_int32)),
                        [a_out("algo28", (_lib.N_LAYERS,), torch.int32, device="cpu")], "pnp_conv_algorithms")
        assert G["algo28"].tolist() == pair.g.conv_algorithms() and G["algo28"][0] == 2 and G["algo28"][27] == 3
        x, sigma = _real(g, n, 1, h, w).to(DEV), _real(g, n, lo=5 / 255, hi=50 / 255).to(DEV)
        c = _cplx(g, n, h, w).to(DEV)
        pair.both(lambda e: (e.profile_reset(), e.denoise(x, sigma), e.fft2c(c)))
        torch.cuda.synchronize()
        tensors = {}
        for e, store in ((pair.g, True), (pair.p, False)):
            if store:
                t = {"total_ms": gb.guarded((_lib.PROFILE_CLASSES,), F64, "cpu"), "launches": gb.guarded((_lib.PROFILE_CLASSES,), torch.int64, "cpu"),
                     "layer_ms": gb.guarded((_lib.N_LAYERS,), F64, "cpu"), "layer_launches": gb.guarded((_lib.N_LAYERS,), torch.int64, "cpu")}
            else:
                t = {"total_ms": torch.empty(_lib.PROFILE_CLASSES, dtype=F64), "launches": torch.empty(_lib.PROFILE_CLASSES, dtype=torch.int64),
                     "layer_ms": torch.empty(_lib.N_LAYERS, dtype=F64), "layer_launches": torch.empty(_lib.N_LAYERS, dtype=torch.int64)}
            assert e.lib.pnp_profile_collect(e._h, cast(t["total_ms"].data_ptr(), C.c_double), cast(t["launches"].data_ptr(), C.c_int64)) == 0
            assert e.lib.pnp_profile_layers(e._h, cast(t["layer_ms"].data_ptr(), C.c_double), cast(t["layer_launches"].data_ptr(), C.c_int64)) == 0
            if store:
                gb.check(t)
            tensors[store] = t
        gt, pt = tensors[True], tensors[False]
        # the times of two runs differ; the counts do not
        assert torch.equal(gt["launches"], pt["launches"]) and torch.equal(gt["layer_launches"], pt["layer_launches"])
        assert int(gt["launches"].sum()) > 0 and int(gt["layer_launches"].sum()) > 0
        for name in ("total_ms", "layer_ms"):
            assert bool(torch.isfinite(gt[name]).all()) and bool((gt[name] >= 0).all()), name
