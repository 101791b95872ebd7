"""GPU checks of brush noise sets through the C generator (nb_brush_noise_create / _load / _destroy, nb_generator_bind_brush_noise):
bitwise equality with the Python pass on the same set for whole, stroke-mask and staged passes, and the binding rules on real
handles.  Every check runs in a child process (tests/_capi_brush_noise_worker.py) under a time limit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "_capi_brush_noise_worker.py")


def run_worker(*args, timeout=300):
    r = subprocess.run([sys.executable, WORKER] + [str(a) for a in args], cwd=REPO, capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-6000:] + r.stderr[-3000:])
    assert r.returncode == 0, f"worker {args} exited with {r.returncode}"
    assert "[capi brush noise] done" in r.stdout


@pytest.mark.parametrize("mode", ["h3", "f8"])
def test_forward_with_a_bound_set_equals_python(mode):
    """style1 R=64, batch 4 (large kernels with in-kernel noise, fused styles + noise launch): a plain load, a lerp load and a
    partial dict; whole passes with and without positions, from stroke masks, and the head / tail at R/2."""
    run_worker("python", mode)


def test_binding_rules():
    """A bound but unloaded set, bind(NULL), describe, a set of another handle (NB_EINVAL), destroying a bound set."""
    run_worker("binding")
