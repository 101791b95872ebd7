"""GPU checks of the staged C generator entry (nb_generator_forward_staged: the head and tail of the painting engine's split around
the feature-canvas blend) and the canvas helpers of a C host: bitwise equality with the Python `_stop_after` / `_resume` passes,
argument errors on a real handle, graph capture, the blending template, and a C program that paints the engine's blended canvases.
Every check runs in a child process (tests/_capi_staged_worker.py) under a time limit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "_capi_staged_worker.py")


def run_worker(*args, timeout=600):
    r = subprocess.run([sys.executable, WORKER] + [str(a) for a in args], cwd=REPO, capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-6000:] + r.stderr[-3000:])
    assert r.returncode == 0, f"worker {args} exited with {r.returncode}"
    assert "[capi staged] done" in r.stdout


@pytest.mark.parametrize("mode,res", [("f32", 128), ("h3", 128), ("f8", 128), ("f8", 256)])
def test_head_and_tail_equal_python(mode, res):
    """R = 128: stages R, R/2 and R/4 (where a geometry feature enters at the resumed block), batches 1, 5 and 8, with and without
    positions, geometry as fp32 features and as stroke masks.  R = 256 (f8): R/2 at batches 1 and 32 -- the large kernels, the operand
    hand-off and in-kernel noise."""
    run_worker("python", mode, res)


def test_staged_errors_leave_outputs_untouched():
    run_worker("errors")


def test_staged_graph_capture():
    run_worker("graph")


def test_dirty_area_alpha_bitwise():
    run_worker("alpha")


@pytest.mark.parametrize("level", [1, 2, 3])
@pytest.mark.parametrize("mode", ["h3", "f8"])
def test_paint_blended_example_equals_painting_helper(tmp_path, mode, level):
    """examples/capi/paint_blended.c on engine_r128.npz, batch 4: canvas, feature canvas and mask equal PaintingHelper's at the same
    level bit for bit; at level 2 also the reference engine's canvas and feature canvas within the bounds of tests/test_hip_painting.py."""
    exe = str(tmp_path / "paint_blended")
    cmd = ["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
           os.path.join(REPO, "examples", "capi", "paint_blended.c"), "-o", exe, "-L/opt/rocm/lib", "-lamdhip64",
           "-L" + os.path.join(REPO, "brushstroke_engine_amd", "csrc"), "-lneube_hip"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    run_worker("paint", exe, str(tmp_path), mode, level)
