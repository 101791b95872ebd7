"""CPU checks of the C generator entry (nb_generator_*): the parameter and layer tables the library derives from a configuration,
argument validation before any HIP call, and the C example building against the library."""
import ctypes
import os
import subprocess

import pytest

from brushstroke_engine_amd import _lib, build, config as cfgmod, weights as wmod
from brushstroke_engine_amd.native import layer_table, native_config, param_table
from brushstroke_engine_amd.networks import Generator
from _gen_configs import ALL, CONFIGS as GEN_CONFIGS, ROWS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = [cfgmod.style1_config(128), cfgmod.style1_config(256), cfgmod.tiny_config(32)] + [
    cfgmod.GeneratorConfig(z_dim=64, w_dim=64, img_resolution=res, channel_base=cbase, channel_max=cmax, geom_feature_channels=geom)
    for res, cmax, cbase, geom in [(64, 96, 4096, (8, 24)), (128, 72, 8192, (16, 40)), (64, 160, 16384, (16, 256)), (64, 100, 6400, (5, 21))]]


@pytest.fixture(scope="module")
def library():
    build.build()
    return _lib.lib()


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"R{c.img_resolution}_c{c.channel_max}_g{'-'.join(map(str, c.geom_feature_channels))}")
def test_param_and_layer_tables(library, cfg):
    sd = wmod.random_state_dict(cfg, 0)
    table = param_table(cfg)
    assert [k for k, _ in table] == list(sd.keys())                   # names and order
    assert [s for _, s in table] == [tuple(v.shape) for v in sd.values()]    # shapes (0-dim noise_strength included)
    layers, num_ws = layer_table(cfg)
    assert layers == cfg.layers and num_ws == cfg.num_ws


@pytest.mark.parametrize("cid", list(GEN_CONFIGS))
def test_gen_config_tables_and_python_generator(library, cid):
    """The nets the GPU tests run through both paths (tests/_gen_configs.py: ragged channels, no conv_clamp, w_dim 40, zero, one and
    three geometry features at explicit resolutions): the C entry derives the Python tables, and the Python Generator takes each
    configuration the C entry takes."""
    cfg, rows = GEN_CONFIGS[cid]
    assert rows and set(rows) <= set(ROWS) and all(set(m) <= set(ALL) for m in rows.values())
    sd = wmod.random_state_dict(cfg, 0)
    table = param_table(cfg)
    assert [k for k, _ in table] == list(sd.keys())
    assert [s for _, s in table] == [tuple(v.shape) for v in sd.values()]
    layers, num_ws = layer_table(cfg)
    assert layers == cfg.layers and num_ws == cfg.num_ws
    c = native_config(cfg)
    assert c.num_geom == len(cfg.geom_feature_channels) and list(c.geom_resolutions[:c.num_geom]) == list(cfg.geom_feature_resolutions)
    G = Generator(cfg, sd)
    assert sorted(G.state_dict().keys()) == sorted(sd.keys())
    assert G.synthesis.geom_feature_resolutions == list(cfg.geom_feature_resolutions)


def _cfg(**kw):
    c = native_config(cfgmod.style1_config(128))
    for k, v in kw.items():
        if k in ("geom_channels", "geom_resolutions"):
            for i, x in enumerate(v):
                getattr(c, k)[i] = x
        else:
            setattr(c, k, v)
    return c


@pytest.mark.parametrize("kw,msg", [
    (dict(c_dim=1), b"c_dim must be 0"),
    (dict(img_resolution=48), b"power of two"),
    (dict(z_dim=0), b"z_dim and w_dim"),
    (dict(w_dim=1024), b"z_dim and w_dim"),
    (dict(mapping_layers=0), b"mapping_layers"),
    (dict(channel_base=64), b"channel_base"),
    (dict(num_geom=5), b"num_geom"),
    (dict(num_geom=3, geom_channels=[16, 256, 8], geom_resolutions=[0, 0, 0]), b"default geometry resolutions"),
    (dict(geom_resolutions=[16, 128]), b"geometry resolution 128"),
    (dict(geom_resolutions=[16, 16]), b"given twice"),
    (dict(geom_channels=[0, 256]), b"geom_channels[0]"),
])
def test_bad_configs_fail_without_gpu(library, kw, msg):
    c = _cfg(**kw)
    assert library.nb_generator_param_count(ctypes.byref(c)) == _lib.NB_EINVAL
    assert msg in library.nb_last_error()
    assert library.nb_generator_layer_count(ctypes.byref(c), None) == _lib.NB_EINVAL
    h = ctypes.c_void_p()
    assert library.nb_generator_create(ctypes.byref(c), None, _lib.NB_CONV_MODES["f8"], 4, None, ctypes.byref(h)) == _lib.NB_EINVAL
    assert h.value is None


def test_unsupported_modes_and_bad_arguments_fail_without_gpu(library):
    c = _cfg()
    h = ctypes.c_void_p()
    for mode in ("f6", "f16"):
        assert library.nb_generator_create(ctypes.byref(c), None, _lib.NB_CONV_MODES[mode], 4, None, ctypes.byref(h)) == _lib.NB_EUNSUPPORTED
        assert b"not supported" in library.nb_last_error()
    assert library.nb_generator_create(ctypes.byref(c), None, 17, 4, None, ctypes.byref(h)) == _lib.NB_EUNSUPPORTED
    assert b"unknown conv_mode" in library.nb_last_error()
    assert library.nb_generator_create(ctypes.byref(c), None, _lib.NB_CONV_MODES["f8"], 0, None, ctypes.byref(h)) == _lib.NB_EINVAL
    assert b"n_max" in library.nb_last_error()
    assert library.nb_generator_create(ctypes.byref(c), None, _lib.NB_CONV_MODES["f8"], 4, None, ctypes.byref(h)) == _lib.NB_EINVAL
    assert b"null parameter array" in library.nb_last_error()
    ptrs = (ctypes.c_void_p * library.nb_generator_param_count(ctypes.byref(c)))()
    assert library.nb_generator_create(ctypes.byref(c), ptrs, _lib.NB_CONV_MODES["f32"], 4, None, ctypes.byref(h)) == _lib.NB_EINVAL
    assert b"parameter 0 (mapping.fc0.weight) is NULL" in library.nb_last_error()
    assert h.value is None
    ins, outs = _lib.NbGeneratorInputs(), _lib.NbGeneratorOutputs()
    assert library.nb_generator_forward(None, ctypes.byref(ins), ctypes.byref(outs), 1, None) == _lib.NB_EINVAL
    assert library.nb_generator_describe(None, 1, ctypes.create_string_buffer(16), 16) == _lib.NB_EINVAL
    name = ctypes.create_string_buffer(4)
    assert library.nb_generator_param_info(ctypes.byref(c), 0, name, 4, None, None) == _lib.NB_EINVAL      # buffer too short
    assert library.nb_generator_param_info(ctypes.byref(c), 10 ** 6, None, 0, None, None) == _lib.NB_EINVAL


def test_error_texts_of_the_table_describe_and_forward_entries(library):
    """The whole nb_last_error text of one failing call per entry (the entries share their helpers: the texts are each entry's own)."""
    c = _cfg()
    count = library.nb_generator_param_count(ctypes.byref(c))
    assert library.nb_generator_param_info(ctypes.byref(c), count, None, 0, None, None) == _lib.NB_EINVAL
    assert library.nb_last_error() == b"generator: parameter index %d out of range [0, %d)" % (count, count)
    assert library.nb_generator_param_info(ctypes.byref(c), 0, ctypes.create_string_buffer(4), 4, None, None) == _lib.NB_EINVAL
    assert library.nb_last_error() == b"generator: name buffer too short (4 bytes for \"mapping.fc0.weight\")"
    assert library.nb_generator_describe(None, 1, ctypes.create_string_buffer(16), 16) == _lib.NB_EINVAL
    assert library.nb_last_error() == b"generator_describe: bad arguments"
    ins, outs = _lib.NbGeneratorInputs(), _lib.NbGeneratorOutputs()
    assert library.nb_generator_forward(None, ctypes.byref(ins), ctypes.byref(outs), 1, None) == _lib.NB_EINVAL
    assert library.nb_last_error() == b"generator_forward: null pointer"


def test_c_example_builds(library, tmp_path):
    cmd = ["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
           os.path.join(REPO, "examples", "capi", "generate.c"), "-o", str(tmp_path / "generate"), "-L/opt/rocm/lib", "-lamdhip64",
           "-L" + os.path.dirname(_lib.LIB_PATH), "-lneube_hip"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert os.path.exists(tmp_path / "generate")
