"""GPU checks of the geometry encoder behind the C generator entry (nb_generator_attach_encoder, nb_generator_forward_geom): bitwise
equality with the Python pass on the lazy encoder, argument errors on a real handle, graph capture, and a C program that paints the
reference's level-0 canvas from the stroke image.  Every check runs in a child process (tests/_capi_geom_worker.py) under a time limit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "_capi_geom_worker.py")


def run_worker(*args, timeout=600):
    r = subprocess.run([sys.executable, WORKER] + [str(a) for a in args], cwd=REPO, capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-6000:] + r.stderr[-3000:])
    assert r.returncode == 0, f"worker {args} exited with {r.returncode}"
    assert "[capi geom] done" in r.stdout


@pytest.mark.parametrize("mode,res", [(m, r) for m in ("f32", "h3", "f8") for r in (128, 256)] + [("h3", 64), ("f8", 64)])
def test_forward_geom_equals_python_lazy_encoder(mode, res):
    run_worker("python", mode, res, timeout=900)


def test_forward_geom_errors():
    run_worker("errors")


@pytest.mark.parametrize("mode,res", [("f8", 256), ("h3", 128)])
def test_forward_geom_graph_capture(mode, res):
    run_worker("graph", mode, res)


@pytest.mark.parametrize("mode", ["h3", "f8"])
def test_paint_example_reproduces_level0_canvas(tmp_path, mode):
    exe = str(tmp_path / "paint")
    cmd = ["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
           os.path.join(REPO, "examples", "capi", "paint.c"), "-o", exe, "-L/opt/rocm/lib", "-lamdhip64",
           "-L" + os.path.join(REPO, "brushstroke_engine_amd", "csrc"), "-lneube_hip"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    run_worker("paint", exe, str(tmp_path), mode)
