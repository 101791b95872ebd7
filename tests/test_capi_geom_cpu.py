"""CPU checks of the geometry encoder behind the C generator entry (nb_encoder_*, nb_generator_encoder_check, nb_generator_attach_encoder,
nb_generator_forward_geom): the parameter table, argument validation before any HIP call, and the C painting example building against
the library."""
import ctypes
import os
import subprocess

import pytest

from brushstroke_engine_amd import _lib, build, config as cfgmod, encoder as encmod
from brushstroke_engine_amd.native import encoder_param_table, native_config
from _gen_configs import CONFIGS as GEN_CONFIGS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def library():
    build.build()
    return _lib.lib()


def test_encoder_param_table(library):
    want = [(k, tuple(s)) for k, s in encmod.ENCODER_STATE_SHAPES
            if not k.endswith("num_batches_tracked") and (k.startswith("encoder.") or k.startswith("decoder.model.0."))]
    assert len(want) == 42
    assert encoder_param_table() == want
    sd = encmod.random_encoder_state_dict(5)
    assert all(tuple(sd[k].shape) == s for k, s in want)
    assert library.nb_encoder_param_info(42, None, 0, None, None) == _lib.NB_EINVAL
    assert b"out of range" in library.nb_last_error()
    assert library.nb_encoder_param_info(0, ctypes.create_string_buffer(4), 4, None, None) == _lib.NB_EINVAL


@pytest.mark.parametrize("res", [32, 64, 128, 256, 512])
def test_encoder_layouts_accepted(library, res):
    c = native_config(cfgmod.style1_config(res))
    for pre in (None, "none", "-11inverse", "inverse"):
        assert library.nb_generator_encoder_check(ctypes.byref(c), _lib.NB_GEOM_PREPROC[pre]) == _lib.NB_OK, library.nb_last_error()


@pytest.mark.parametrize("cid", list(GEN_CONFIGS))
def test_non_encoder_layouts_refused(library, cid):
    cfg = GEN_CONFIGS[cid][0]
    c = native_config(cfg)
    r = cfg.img_resolution
    default = tuple(cfg.geom_feature_channels) == (16, 256) and tuple(cfg.geom_feature_resolutions) == (r // 8, r // 4)
    rc = library.nb_generator_encoder_check(ctypes.byref(c), 0)
    if default:                       # (every R >= 32 with the default layout is a size the encoder tiles)
        assert rc == _lib.NB_OK
    else:
        assert rc == _lib.NB_EINVAL
        assert b"geometry layout is not the encoder's" in library.nb_last_error()


def test_bad_arguments_fail_without_gpu(library):
    c = native_config(cfgmod.style1_config(128))
    for pre in (-1, 3, 17):
        assert library.nb_generator_encoder_check(ctypes.byref(c), pre) == _lib.NB_EINVAL
        assert b"unknown preproc" in library.nb_last_error()
    c.img_resolution = 16                  # a generator the encoder cannot take (R/8 = 2: the generator refuses it first)
    assert library.nb_generator_encoder_check(ctypes.byref(c), 0) == _lib.NB_EINVAL
    assert library.nb_generator_attach_encoder(None, None, 0, None) == _lib.NB_EINVAL
    assert b"null generator" in library.nb_last_error()
    ins, outs = _lib.NbGeneratorInputs(), _lib.NbGeneratorOutputs()
    assert library.nb_generator_forward_geom(None, ctypes.byref(ins), None, ctypes.byref(outs), 1, None) == _lib.NB_EINVAL
    assert b"null pointer" in library.nb_last_error()


def test_error_texts_of_the_encoder_table_and_forward_entries(library):
    """The whole nb_last_error text of one failing call per entry."""
    assert library.nb_encoder_param_info(42, None, 0, None, None) == _lib.NB_EINVAL
    assert library.nb_last_error() == b"encoder: parameter index 42 out of range [0, 42)"
    assert library.nb_encoder_param_info(0, ctypes.create_string_buffer(4), 4, None, None) == _lib.NB_EINVAL
    assert library.nb_last_error() == b"generator: name buffer too short (4 bytes for \"encoder.model.0.conv.0.weight\")"
    ins, outs = _lib.NbGeneratorInputs(), _lib.NbGeneratorOutputs()
    assert library.nb_generator_forward_geom(None, ctypes.byref(ins), None, ctypes.byref(outs), 1, None) == _lib.NB_EINVAL
    assert library.nb_last_error() == b"generator_forward_geom: null pointer"


def test_paint_example_builds(library, tmp_path):
    cmd = ["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
           os.path.join(REPO, "examples", "capi", "paint.c"), "-o", str(tmp_path / "paint"), "-L/opt/rocm/lib", "-lamdhip64",
           "-L" + os.path.dirname(_lib.LIB_PATH), "-lneube_hip"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert os.path.exists(tmp_path / "paint")
