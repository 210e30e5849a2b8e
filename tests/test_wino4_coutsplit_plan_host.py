"""The cout-split rule of winograd_plan on the host (no GPU): tests/plan_coutsplit_host.cpp, linked against the built library, plans every
batch size 1..96 at seven slice sizes with the schedule off, under the default rule and forced, and requires that no layer ever leaves
F(4x4) because of it (its workgroups are half as many, so its count must pass the workgroup gate itself; otherwise the older plan stands)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dt4image_restoration_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def plan_output(tmp_path_factory):
    if not os.path.exists(HIPCC) or shutil.which("make") is None:
        pytest.skip("no hipcc / make")
    if not os.path.exists(os.path.join(CSRC, "libpnpadmm.so")):
        subprocess.run(["make", "-C", CSRC, "-j", "4"], check=True, capture_output=True)
    exe = str(tmp_path_factory.mktemp("plan") / "plan_coutsplit_host")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", os.path.join(ROOT, "tests", "plan_coutsplit_host.cpp"), "-o", exe,
                    "-L" + CSRC, "-lpnpadmm", "-Wl,-rpath," + CSRC], check=True, capture_output=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PNP_")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_no_layer_leaves_f4_because_of_the_schedule(plan_output):
    assert "plan_coutsplit_host: 0 failures" in plan_output and "FAIL" not in plan_output


@pytest.mark.parametrize("n", [8, 16, 64])
def test_the_deep_upsample_layers_stay_on_f4_at_mid_size_batches(plan_output, n):
    """256 x 256, workgroup gate 192: up1.conv-0 has 16 n workgroups of 64 channels (128 / 256 / 1024 at n = 8 / 16 / 64: F(4x4) from 12
    slices on), up2.conv-0 32 n (F(4x4) from 6 on), and half as many of 128 channels.  With the schedule they run what they ran without
    it or the schedule itself - F(4x4) at 16 slices for both, at 8 for up2.conv-0 - and at 64, the measured case, the schedule."""
    m = re.search(rf"256x256 n {n}: up1.conv-0 family (\d) \(schedule off: (\d)\) cs (\d), up2.conv-0 family (\d) \(schedule off: (\d)\) cs (\d)", plan_output)
    assert m, plan_output
    up1, up1_off, up1_cs, up2, up2_off, up2_cs = m.groups()
    assert up1 == up1_off and up2 == up2_off, m.group(0)
    assert up2 == "4" and (up1 == "4") == (n >= 12), m.group(0)
    if n == 64:
        assert up1_cs == "1" and up2_cs == "1", m.group(0)
