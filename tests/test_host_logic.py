"""CPU-only checks: the C-ABI library loads and exports every symbol include/pnpadmm.h declares, the
generators are deterministic, the shift-folding identity the kernels rely on, shard arithmetic,
and that the product path refuses to run without a GPU (no CPU fallback)."""
import os
import re

import numpy as np
import pytest
import torch

from dt4image_restoration_amd import _lib, sharding, synthetic, unet_spec, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions():
    src = open(os.path.join(ROOT, "include", "pnpadmm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pnp_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()                                   # no compute calls: works without a GPU
    names = _header_functions()
    assert len(names) >= 14
    for name in names:
        assert hasattr(lib, name), f"{name} declared in include/pnpadmm.h but not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert sorted(_lib.SIGNATURES) == names
    assert b"gfx950" in lib.pnp_version()


def test_header_is_plain_c_and_links_from_c(tmp_path):
    """The boundary is a C ABI: include/pnpadmm.h compiles as strict C99 and a C program links against the library and
    calls it (argument validation only - no GPU needed)."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "abi.c"
    src.write_text(
        '#include <stdio.h>\n#include <string.h>\n#include "pnpadmm.h"\n'
        "int main(void) {\n"
        "    pnp_handle h = 0;\n"
        "    pnp_config bad = {0, 128, 128, 0, 0};\n"
        "    if (pnp_create(&bad, &h) == PNP_OK) return 1;          /* n = 0 must be rejected before any HIP call */\n"
        "    if (strlen(pnp_last_error()) == 0) return 2;\n"
        "    if (pnp_step(0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == PNP_OK) return 3;   /* null handle */\n"
        "    if (pnp_snapshot_bytes(0) != 0) return 4;\n"
        '    printf("%s\\n", pnp_version());\n'
        "    return 0;\n}\n")
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe), "-L", libdir, "-lpnpadmm", f"-Wl,-rpath,{libdir}"], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in out


def test_create_rejects_bad_config_without_touching_a_gpu():
    import ctypes as C
    lib = _lib.load()
    h = C.c_void_p()
    cfg = _lib.pnp_config(1, 100, 128, 0, 0)            # h not a multiple of 16
    assert lib.pnp_create(C.byref(cfg), C.byref(h)) == -1
    assert b"multiples of 16" in lib.pnp_last_error()
    assert lib.pnp_create(None, C.byref(h)) == -1


def test_create_rejects_a_plan_past_2gib_before_any_device_call():
    """The denoiser's plan is made before the first device call: in bf16 mode (no F(4x4) layers) layer 1's output of a 256 x 256 x 256 handle
    is exactly 2^31 bytes, which the planner refuses - with or without a GPU, and without allocating anything."""
    import ctypes as C
    lib = _lib.load()
    h = C.c_void_p()
    cfg = _lib.pnp_config(256, 256, 256, 0, _lib.PNP_FLAG_BF16_CONVS)
    assert lib.pnp_create(C.byref(cfg), C.byref(h)) == -1            # PNP_ERR_INVALID
    assert b"2 GiB" in lib.pnp_last_error() and not h.value


def test_product_path_never_touches_the_oracle():
    """Nothing under the package (sub-packages and the C sources included) imports, names or links the oracle; only tests/,
    __graft_entry__.smoke() and bench.py's cpu_baseline leg may."""
    pkg = os.path.join(ROOT, "dt4image_restoration_amd")
    seen = 0
    for dirpath, _dirs, files in os.walk(pkg):
        if "__pycache__" in dirpath or os.path.basename(dirpath) in ("_asan", "_stamps"):
            continue
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".cpp", ".c")) or fn == "Makefile":
                seen += 1
                text = open(os.path.join(dirpath, fn)).read()
                assert "oracle" not in text and "pnp_ref" not in text, os.path.join(dirpath, fn)
    assert seen >= 18                                    # top-level modules + drivers/ + csrc/
    bench = open(os.path.join(ROOT, "bench.py")).read()
    assert bench.count("from oracle") == 1 and "def cpu_baseline" in bench      # one import, inside the baseline leg


def test_one_place_reads_the_environment():
    """Every getenv of the library sits in tuning_from_env, read once per handle at pnp_create - a plan, a launch or an entry point never reads
    the process environment on its own - except the timing switches of the diagnostic build (`#ifdef PNP_DIAG` regions of pnp_capi.hip).  The four
    retired experiment switches are named nowhere in the package."""
    csrc = os.path.join(ROOT, "dt4image_restoration_amd", "csrc")
    reads = 0
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith((".hip", ".h", ".cpp", ".c")):
            continue
        text = open(os.path.join(csrc, fn)).read()
        allowed = []                                     # [start, end) character ranges that may read the environment
        m = re.search(r"^Tuning tuning_from_env\(\) \{$.*?^\}$", text, re.S | re.M)
        if m:
            allowed.append(m.span())
        if fn == "pnp_capi.hip":                         # #ifdef PNP_DIAG ... its #endif (conditionals inside it nest)
            depth, start = 0, None
            for d in re.finditer(r"^[ \t]*#[ \t]*(ifdef|ifndef|if|endif)\b(.*)$", text, re.M):
                if d.group(1) != "endif":
                    if start is None and d.group(1) == "ifdef" and d.group(2).strip() == "PNP_DIAG":
                        start, depth = d.end(), 0
                    elif start is not None:
                        depth += 1
                elif start is not None:
                    if depth == 0:
                        allowed.append((start, d.start()))
                        start = None
                    else:
                        depth -= 1
            assert start is None, "unterminated #ifdef PNP_DIAG"
        for g in re.finditer(r"getenv\s*\(", text):
            reads += 1
            line = text.count("\n", 0, g.start()) + 1
            assert any(a <= g.start() < b for a, b in allowed), f"{fn}:{line}: getenv outside tuning_from_env"
    assert reads >= 20                                   # the scan found tuning_from_env's own reads
    retired = ("PNP_FFT_XCD", "PNP_SPLITK_INLAUNCH", "PNP_SPLITK_COARSE", "PNP_FFT_ROWS_R4")
    seen = 0
    for dirpath, _dirs, files in os.walk(os.path.join(ROOT, "dt4image_restoration_amd")):
        if "__pycache__" in dirpath or os.path.basename(dirpath) in ("_asan", "_stamps", "_diag", "_isa"):
            continue
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".cpp", ".c")) or fn in ("Makefile", "libpnpadmm.so"):   # the sources and what they built
                seen += 1
                blob = open(os.path.join(dirpath, fn), "rb").read()
                for name in retired:
                    assert name.encode() not in blob, f"{os.path.join(dirpath, fn)} names {name}"
    assert seen >= 18


def test_product_path_fails_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from dt4image_restoration_amd.engine import PnPEngine
    from dt4image_restoration_amd.denoiser import UNetDenoiser2D
    from dt4image_restoration_amd.env import PnPEnv
    with pytest.raises(_lib.PnPError):
        PnPEngine(1, 64, 64)
    den = UNetDenoiser2D.seeded(0)
    with pytest.raises(RuntimeError):
        den(torch.zeros(1, 1, 32, 32), torch.zeros(1))
    with pytest.raises(RuntimeError):
        PnPEnv(30, den, "cuda").reset({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.make_problem(1, 32, 32).items()}, "cpu")


def test_host_side_under_asan_ubsan():
    """host-side AddressSanitizer + UBSan build of the C ABI (`make asan`: host code instrumented, device code as
    usual) running tests/asan_host.cpp - every tile plan, every weight repack into exactly-sized heap buffers, and the
    argument validation of every entry point.  CPU box only (GPU sanitizer runs are not available on the pool)."""
    import shutil
    import subprocess
    if torch.cuda.is_available():
        pytest.skip("sanitizer build is for the CPU box")
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc / make")
    csrc = os.path.join(ROOT, "dt4image_restoration_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j", "4", "asan"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "_asan", "asan_host")], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr


def test_no_low_reads_high_packed_ops_next_to_bf16_mfma():
    """Round 5 (profiles/r05_race.md): on MI355X a v_pk_{mul,fma,add}_f32 operand whose LOW result reads the HIGH register of the pair
    (op_sel = 1) reads zero in lanes 48-63 now and then while the SIMD's other wave runs bf16 MFMAs fed by loads; hipcc forms such operands from
    plain scalar source.  The code objects inside the BUILT library must hold none in a kernel with non-f32 MFMAs (tools/isa_audit.py
    disassembles them); the f32-MFMA and MFMA-free kernels may (measured safe: exp/pk_opsel_probe.hip)."""
    import subprocess
    import sys
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump") or not os.path.exists(_lib.LIB_PATH):
        pytest.skip("no llvm-objdump / library")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_audit.py"), "--lib", _lib.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "0 kernels flagged" in r.stdout and "conv3x3_bf16ws" not in r.stdout.replace("  ok", "")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_patch
    # the detector itself: the forms the probe found faulty and the ones it found clean
    assert isa_patch.parse_pk("\tv_pk_mul_f32 v[42:43], v[84:85], v[94:95] op_sel:[0,1]")["sel"] == [0, 1]
    assert isa_patch.parse_pk("\tv_pk_fma_f32 v[80:81], v[116:117], v[80:81], v[118:119] op_sel:[0,1,0] op_sel_hi:[1,0,1]")["crossed_overlap"]
    assert isa_patch.parse_pk("\tv_pk_fma_f32 v[96:97], v[72:73], v[78:79], v[42:43] op_sel_hi:[0,1,1]")["sel"] == [0, 0, 0]


def test_unet_spec_counts():
    assert len(unet_spec.UNET_LAYERS) == 28 and len(unet_spec.STATE_DICT_KEYS) == 56
    assert unet_spec.N_PARAMS == 11_773_857
    assert unet_spec.FLOPS_PER_PIXEL == 591_040
    assert unet_spec.conv_flops(256, 256, 64) == 591_040 * 65536 * 64


def test_weight_generator_is_deterministic_and_keyed():
    a = weights.generate_unet_weights(0)
    b = weights.generate_unet_weights(0)
    c = weights.generate_unet_weights(1)
    assert list(a) == unet_spec.STATE_DICT_KEYS
    for k in a:
        assert np.array_equal(a[k], b[k])
    assert not np.array_equal(a["inc.conv.conv-1.conv2d.weight"], c["inc.conv.conv-1.conv2d.weight"])
    assert a["up1.conv.conv-0.conv2d.weight"].shape == (256, 768, 3, 3)
    blob = weights.flatten_state_dict(a)
    assert blob.size == unet_spec.N_PARAMS and blob.dtype == np.float32
    bad = dict(a); bad.pop("outc.conv.bias")
    with pytest.raises(KeyError):
        weights.check_state_dict(bad)
    bad = dict(a); bad["outc.conv.bias"] = np.zeros(2, np.float32)
    with pytest.raises(ValueError):
        weights.check_state_dict(bad)


def test_synthetic_problem_is_shard_consistent():
    full = synthetic.make_problem(4, 32, 32, seed=9)
    part = synthetic.make_problem(2, 32, 32, seed=9, first_slice=2)
    for k in ("x0", "y0", "gt"):
        assert np.array_equal(full[k][2:], part[k])
    assert full["mask"].mean() >= 0.25 and full["mask"].mean() < 0.30
    assert full["x0"].min() >= 0.0                       # datasets.py:160 clip


def test_shift_folding_identity():
    """ifft_c(where(m,(mu fft_c(v)+y0)/(1+mu),fft_c(v))) == IFFT(where(S m,(mu FFT(v)+sgn S y0)/(1+mu),FFT(v)))
    - the identity fft_kernels.hip / pnp_reset rely on (plain unshifted ortho transforms, even sizes)."""
    rng = np.random.default_rng(0)
    for h, w in ((16, 16), (32, 64)):
        v = rng.standard_normal((h, w)) + 1j * rng.standard_normal((h, w))
        y0 = rng.standard_normal((h, w)) + 1j * rng.standard_normal((h, w))
        m = rng.random((h, w)) < 0.3
        mu = 0.37
        f = synthetic.fft2c_np(v)
        ref = synthetic.ifft2c_np(np.where(m, (mu * f + y0) / (1 + mu), f))
        k1, k2 = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        sgn = (-1.0) ** (k1 + k2)
        Sm, Sy = np.fft.fftshift(m), np.fft.fftshift(y0)
        # S as the kernels index it: k ^ (n/2)
        assert np.array_equal(Sm, m[np.ix_(np.arange(h) ^ (h // 2), np.arange(w) ^ (w // 2))])
        F = np.fft.fft2(v, norm="ortho")
        got = np.fft.ifft2(np.where(Sm, (mu * F + sgn * Sy) / (1 + mu), F), norm="ortho")
        assert np.abs(got - ref).max() < 1e-12


def test_shard_range_partitions():
    for total, world in ((512, 8), (10, 4), (3, 8), (64, 1)):
        seen = []
        for r in range(world):
            a, b = sharding.shard_range(total, r, world)
            seen += list(range(a, b))
        assert seen == list(range(total))
    with pytest.raises(ValueError):
        sharding.shard_range(4, 4, 4)


def test_checkpoint_file_ingest_on_the_cpu(tmp_path):
    """The reference's weight ingest (noise.py:146-148: `net.load_state_dict(torch.load(ckpt_path))`): a torch.save'd
    OrderedDict of the 56 tensors loads through `UNetDenoiser2D(ckpt_path=...)` into exactly the arrays it was written from
    (no GPU needed up to here: the engine is created on first use), a file with a missing / misshapen tensor is rejected, and
    the policy's 85-key checkpoint round-trips through `torch.load` + `load_state_dict` like eval.py:20,27 does."""
    import collections
    import torch
    from dt4image_restoration_amd.denoiser import UNetDenoiser2D
    from dt4image_restoration_amd.policy import DecisionTransformer, DecisionTransformerConfig
    sd = weights.generate_unet_weights(3, "torch_default")
    ck = tmp_path / "unet-nm.pt"
    torch.save(collections.OrderedDict((k, torch.from_numpy(v.copy())) for k, v in sd.items()), ck)
    den = UNetDenoiser2D(ckpt_path=str(ck))
    assert list(den.weights) == unet_spec.STATE_DICT_KEYS
    for k in sd:
        assert den.weights[k].dtype == np.float32 and np.array_equal(den.weights[k], sd[k]), k
    bad = collections.OrderedDict((k, torch.from_numpy(v.copy())) for k, v in sd.items())
    bad.pop("down2.mpconv.1.conv-1.conv2d.bias")
    torch.save(bad, tmp_path / "bad.pt")
    with pytest.raises(KeyError):
        UNetDenoiser2D(ckpt_path=str(tmp_path / "bad.pt"))
    with pytest.raises(ValueError):
        UNetDenoiser2D()                                  # neither a path nor a mapping (noise.py:143-145)
    m = DecisionTransformer(DecisionTransformerConfig(block_size=18, n_embeds=9, mode="norm"))
    psd = weights.generate_policy_weights(m, 5, t_bias=-1.0, head_gain=8.0)
    assert len(psd) == 85
    torch.save(psd, tmp_path / "model_experiment_1.pt")
    m2 = DecisionTransformer(DecisionTransformerConfig(block_size=18, n_embeds=9, mode="norm"))
    m2.load_state_dict(torch.load(tmp_path / "model_experiment_1.pt", map_location="cpu"))
    for k, v in m2.state_dict().items():
        assert torch.equal(v, torch.as_tensor(psd[k])), k
