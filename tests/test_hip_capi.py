"""GPU checks of the C generator entry (nb_generator_*, include/neube_hip.h): device weight packers, the kernel plan, bitwise
equality with the Python pass (also at every batch threshold of the nets in tests/_gen_configs.py), the float64 oracle, the reference's
golden vectors, graph capture and a C host program.  Every check runs in a child
process (tests/_capi_worker.py) under a time limit."""
import os
import subprocess
import sys

import pytest

from _gen_configs import CONFIGS

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "_capi_worker.py")


def run_worker(*args, timeout=600):
    r = subprocess.run([sys.executable, WORKER] + [str(a) for a in args], cwd=REPO, capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-6000:] + r.stderr[-3000:])
    assert r.returncode == 0, f"worker {args} exited with {r.returncode}"
    assert "[capi] done" in r.stdout


def test_device_packers_match_torch():
    run_worker("packers")


@pytest.mark.parametrize("res", [128, 256])
@pytest.mark.parametrize("mode", ["f32", "h3", "f8"])
def test_native_equals_python_and_describe(mode, res):
    run_worker("python", mode, res, timeout=900)


@pytest.mark.parametrize("mode", ["f32", "h3", "f8"])
@pytest.mark.parametrize("cid", list(CONFIGS))
def test_native_equals_python_at_batch_thresholds(cid, mode):
    """Ragged channels, no conv_clamp, w_dim % 16 != 0, other geometry layouts: describe == layer_kernels and bitwise equal outputs
    at n = 1, 3, 8, 9, 15, 16, 32, and the decision rows the net exists for are reached."""
    run_worker("matrix", cid, mode)


@pytest.mark.parametrize("cid", list(CONFIGS))
def test_native_against_float64_oracle(cid):
    run_worker("oracle", cid)


@pytest.mark.parametrize("mode", ["f32", "h3", "f8"])
def test_native_against_reference_golden(mode):
    run_worker("golden", mode)


@pytest.mark.parametrize("res", [128, 256])
@pytest.mark.parametrize("mode", ["f8", "f32"])
def test_native_graph_capture(mode, res):
    run_worker("graph", mode, res)


def test_c_host_example(tmp_path):
    exe = str(tmp_path / "generate")
    cmd = ["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
           os.path.join(REPO, "examples", "capi", "generate.c"), "-o", exe, "-L/opt/rocm/lib", "-lamdhip64",
           "-L" + os.path.join(REPO, "brushstroke_engine_amd", "csrc"), "-lneube_hip"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    run_worker("chost", exe, str(tmp_path))
