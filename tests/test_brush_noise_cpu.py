"""CPU-side checks of brush noise sets (a projected brush's noise buffers as a device object): the C entries are exported, bound and
reject bad arguments on the host; the struct layout matches the header; the planner rows the GPU tests are meant to reach are
reached at their shapes; and the reference-generated fixture tests/golden/engine_brush_noise_r128.npz is what it claims to be."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from brushstroke_engine_amd import _lib, build, config as cfgmod, encoder as encmod, weights as wmod
from brushstroke_engine_amd.networks import SynthesisNetwork
from brush_noise_refs import fixture_buffers, fixture_patches
from conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nb_brush_noise_build_f32", "nb_brush_noise_create", "nb_brush_noise_load", "nb_generator_bind_brush_noise",
           "nb_brush_noise_destroy")


@pytest.fixture(scope="module")
def library():
    build.build()
    return _lib.lib()


def test_entries_are_exported_and_bound(library):
    text = open(os.path.join(REPO, "include", "neube_hip.h")).read()
    for name in ENTRIES:
        assert name in _lib.PROTOTYPES and hasattr(library, name), name
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in include/neube_hip.h"
    assert "nb_brush_noise.hip" in build.SOURCES and build.FILE_FLAGS["nb_brush_noise.hip"] == ["-fno-slp-vectorize"]
    assert library.nb_abi_version() == _lib.ABI_VERSION >= 18


def test_layer_struct_matches_header():
    text = open(os.path.join(REPO, "include", "neube_hip.h")).read()
    m = re.search(r"typedef struct NbBrushNoiseLayer \{(.*?)\} NbBrushNoiseLayer;", text, flags=re.S)
    assert m, "struct NbBrushNoiseLayer is not in the header"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields, size = [], 0
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        if "*" in decl:                                       # "const float* a"
            names, width = [decl.split("*")[-1].strip()], 8
        else:                                                 # "int32_t res, pad"
            ctype, rest = decl.split(" ", 1)
            names, width = [n.strip() for n in rest.split(",")], {"int32_t": 4}[ctype]
        fields += names
        size += width * len(names)
    assert fields == [f for f, _ in _lib.NbBrushNoiseLayer._fields_]
    assert size == ctypes.sizeof(_lib.NbBrushNoiseLayer) == 40        # four pointers, two int32: no padding


def _layer(a=8, dst=16, dst_t=24, res=32, b=0):
    return _lib.NbBrushNoiseLayer(a or None, b or None, dst or None, dst_t or None, res, 0)


def test_build_rejects_bad_arguments_on_the_host(library):
    """Validation happens before the launch: no GPU is touched (the pointers below are never dereferenced)."""
    def rc_of(layers, n=None):
        arr = (_lib.NbBrushNoiseLayer * max(len(layers), 1))(*layers)
        rc = library.nb_brush_noise_build_f32(arr, len(layers) if n is None else n, 1.0, 0.0, None)
        return rc, library.nb_last_error().decode()
    rc = library.nb_brush_noise_build_f32(None, 1, 1.0, 0.0, None)
    assert rc == _lib.NB_EINVAL and "null layer array" in library.nb_last_error().decode()
    for n in (0, -1, _lib.NB_PLAN_MAX_LAYERS + 1):
        rc, msg = rc_of([_layer()], n)
        assert rc == _lib.NB_EINVAL and "layers outside" in msg, (n, msg)
    for bad in (dict(a=0), dict(dst=0), dict(dst_t=0)):
        rc, msg = rc_of([_layer(), _layer(**bad)])
        assert rc == _lib.NB_EINVAL and "layer 1 has a null" in msg, (bad, msg)
    for res in (0, 2, 3, 6, 48, -4):
        rc, msg = rc_of([_layer(res=res)])
        assert rc == _lib.NB_EINVAL and "not a power of two" in msg, (res, msg)
    for bad in (dict(dst_t=8), dict(b=24), dict(dst=24)):            # dst_t may alias nothing (dst == a is fine, but needs a launch)
        rc, msg = rc_of([_layer(**bad)])
        assert rc == _lib.NB_EINVAL and "aliases" in msg, (bad, msg)


def test_set_entries_reject_null_handles(library):
    out = ctypes.c_void_p(7)
    assert library.nb_brush_noise_create(None, None, ctypes.byref(out)) == _lib.NB_EINVAL
    assert "null generator" in library.nb_last_error().decode() and out.value is None
    assert library.nb_brush_noise_create(None, None, None) == _lib.NB_EINVAL and "null output" in library.nb_last_error().decode()
    assert library.nb_brush_noise_load(None, None, None, 1.0, None) == _lib.NB_EINVAL and "null set" in library.nb_last_error().decode()
    assert library.nb_generator_bind_brush_noise(None, None) == _lib.NB_EINVAL and "null generator" in library.nb_last_error().decode()
    assert library.nb_brush_noise_destroy(None) == _lib.NB_OK
    # the whole text of one failing call per set entry
    assert library.nb_brush_noise_create(None, None, ctypes.byref(out)) == _lib.NB_EINVAL
    assert library.nb_last_error() == b"brush_noise_create: null generator"
    assert library.nb_brush_noise_load(None, None, None, 1.0, None) == _lib.NB_EINVAL
    assert library.nb_last_error() == b"brush_noise_load: null set"
    assert library.nb_generator_bind_brush_noise(None, None) == _lib.NB_EINVAL
    assert library.nb_last_error() == b"generator_bind_brush_noise: null generator"


def test_gpu_shapes_reach_the_rows_the_feature_exists_for():
    """style1 R=64 with integer positions: batch 4 runs large kernels with in-kernel noise behind the fused styles + noise launch,
    batch 9 normalises the positions once -- unless the pass carries per-call noise overrides (the noise_buffers= route), which
    switch all of it off.  A noise set asks for the ordinary plan."""
    syn = SynthesisNetwork(cfgmod.style1_config(64))
    p4, p9 = syn.pass_plan(4, noise_overrides=False), syn.pass_plan(9, noise_overrides=False)
    assert p4.inkernel_from is not None and p4.styles_noise and not p4.positions_once
    assert p9.inkernel_from is not None and p9.positions_once
    assert any(lp.noise_in_kernel for lp in p4.layers)
    o4, o9 = syn.pass_plan(4, noise_overrides=True), syn.pass_plan(9, noise_overrides=True)
    assert o4.inkernel_from is None and not o4.styles_noise and not any(lp.noise_in_kernel for lp in o4.layers)
    assert o9.inkernel_from is None and not o9.styles_noise
    assert [lp.kernel for lp in o4.layers] == [lp.kernel for lp in p4.layers]


# ---- the reference-generated fixture ----
def test_fixture_is_smaller_than_engine_r128():
    size = lambda n: os.path.getsize(os.path.join(REPO, "tests", "golden", n))      # noqa: E731
    assert size("engine_brush_noise_r128.npz") < size("engine_r128.npz")


def test_fixture_noise_shows_in_the_picture():
    g = load_golden("engine_brush_noise_r128.npz")
    assert g["tiles_noise"].shape == g["tiles_plain"].shape == (2, 108, 108, 4) and int(g["level"]) == 2 and int(g["crop_margin"]) == 10
    d = np.abs(g["tiles_noise"].astype(np.int32) - g["tiles_plain"].astype(np.int32))
    assert (d > 1).mean() > 0.05, (d > 1).mean()
    (x0, y0), (x1, y1) = g["xy"].tolist()
    assert abs(x0 - x1) < 128 and abs(y0 - y1) < 128          # the two tiles overlap


def test_oracle_reproduces_the_first_tile():
    """The CPU oracle with ``noise_buffers=`` against the reference engine's triad data of the first tile (an empty feature canvas:
    nothing is blended yet), to the figures tests/test_oracle_golden.py holds the oracle to."""
    from oracle import neube_oracle as orc, painting_oracle as po
    g = load_golden("engine_brush_noise_r128.npz")
    R = int(g["resolution"])
    cfg = cfgmod.style1_config(R)
    G = orc.OracleGenerator(cfg, wmod.random_state_dict(cfg, seed=int(g["weights_seed"])))
    esd = encmod.random_encoder_state_dict(int(g["encoder_seed"]))
    geom = 1 - torch.from_numpy(fixture_patches(g)[:1, :, :, 0]).to(torch.float32).unsqueeze(1) / 255.0      # brush.py:679
    feats = po.encoder_encode(esd, geom, None)
    x, y = g["xy"][0].tolist()
    _, dbg = G.forward_pre_mapped(g["ws"], feats, positions=np.array([[y, x]], np.int64), return_debug_data=True,
                                  noise_buffers=fixture_buffers(g, cfg))
    e_uvs = float(np.abs(np.asarray(dbg["uvs"], np.float64) - g["uvs0"]).max())
    e_col = float(np.abs(np.asarray(dbg["colors"], np.float64) - g["colors0"]).max())
    print(f"[brush noise fixture] oracle vs reference, first tile: uvs {e_uvs:.2e} colors {e_col:.2e}")
    assert e_uvs <= 2e-5 and e_col <= 1e-5
    _, plain = G.forward_pre_mapped(g["ws"], feats, positions=np.array([[y, x]], np.int64), return_debug_data=True)
    assert float(np.abs(np.asarray(plain["uvs"], np.float64) - g["uvs0"]).max()) > 1e-2      # (the buffers matter to it)
