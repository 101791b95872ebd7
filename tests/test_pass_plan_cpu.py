"""CPU checks of the per-batch layer plan (nb_synthesis_plan, include/neube_hip.h) that SynthesisNetwork and the C generator both
follow: it reproduces the decisions the Python pass made before the planner existed (tests/golden/pass_plans.json), and every net of
tests/_gen_configs.py reaches the decision rows it exists for."""
import ctypes
import json
import os

import pytest

from brushstroke_engine_amd import _lib, build, config as cfgmod
from brushstroke_engine_amd.native import native_config
from brushstroke_engine_amd.networks import SynthesisNetwork
from _gen_configs import ALL, BATCHES, CONFIGS, expected_rows, rows_reached

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pass_plans.json")
NETS = {"style1_128": cfgmod.style1_config(128), "style1_256": cfgmod.style1_config(256), "tiny_32": cfgmod.tiny_config(32)}
NETS.update({cid: c for cid, (c, _) in CONFIGS.items()})
KIND = {_lib.NB_KERNEL_F32: "F", _lib.NB_KERNEL_SMALL_H3: "S", _lib.NB_KERNEL_LARGE_H3: "L"}


@pytest.fixture(scope="module")
def library():
    build.build()
    return _lib.lib()


def shape_kwargs(shape, R):
    """The pass shapes of the snapshot: positional constant noise, constant noise without positions, a pass that stops after
    block R/2, a pass resumed after it.  (The bit of block res in a mask, 1 << log2(res), is res itself.)"""
    return {"pos": {}, "const": dict(noise_positions=_lib.NB_PLAN_POS_NONE), "split": dict(tap_mask=R // 2),
            "resume": dict(resume_res=R // 2)}[shape]


def encode(kp, labels):
    """One snapshot line (the golden file's "format")."""
    head = f"{int(kp.styles_fast)}{int(kp.styles_noise)}{int(kp.positions_once)}:{'-' if kp.inkernel_from is None else kp.inkernel_from}"
    layers = ",".join(f"{KIND[lp.kind]}{lp.in_fmt}{lp.kernel_fmt}{lp.out_fmt}{lp.handoff}{lp.fused_torgb}{lp.noise_in_kernel}"
                      f"{lp.packs:x}@{labels.index(lp.kernel)}" for lp in kp.layers)
    geom = ",".join(f"{gp.early_pack}{gp.fmt}{gp.encoder_handoff}" for gp in kp.geom) or "-"
    return f"{head} {layers} {geom}"


@pytest.mark.parametrize("net", list(NETS))
def test_planner_reproduces_the_snapshot(library, net):
    golden = json.load(open(GOLDEN))
    cfg = NETS[net]
    syn = SynthesisNetwork(cfg)
    R = cfg.img_resolution
    for mode in ("f32", "h3", "f8", "f6", "f16"):
        syn.conv_mode = mode
        for n in BATCHES:
            for shape in ("pos", "const", "split", "resume"):
                key = f"{net} {mode} {n} {shape}"
                assert encode(syn.pass_plan(n, **shape_kwargs(shape, R)), golden["labels"]) == golden["cases"][key], key


@pytest.mark.parametrize("cid", list(CONFIGS))
def test_planner_reaches_the_declared_rows(library, cid):
    """rows_reached on the planner's labels (the ToRGB's entry included, as describe and layer_kernels give it) at every batch of
    BATCHES: each net reaches the rows it declares for each mode."""
    cfg = CONFIGS[cid][0]
    syn = SynthesisNetwork(cfg)
    for mode in ALL:
        syn.conv_mode = mode
        reached = set()
        for n in BATCHES:
            kp = syn.pass_plan(n)
            kernels = {s.name: lp.kernel for s, lp in zip(cfg.layers, kp.layers)}
            last = kp.layers[-1]
            kernels[cfg.torgb_name] = last.kernel if last.fused_torgb else "torgb_triad_kernel"
            formats = {s.name: lp.in_fmt for s, lp in zip(cfg.layers, kp.layers) if lp.kind == _lib.NB_KERNEL_LARGE_H3}
            reached |= rows_reached(cfg, mode, kernels, formats)
        missing = expected_rows(cid, mode) - reached
        assert not missing, f"{cid} {mode}: missing rows {sorted(missing)}"


def test_plan_cache_follows_the_knobs(library):
    """The per-instance plan cache is keyed on the knobs: toggling one between passes changes the plan."""
    syn = SynthesisNetwork(cfgmod.style1_config(256))
    on = syn.pass_plan(32)
    assert any(lp.handoff for lp in on.layers)
    syn.h2_handoff = False
    assert not any(lp.handoff for lp in syn.pass_plan(32).layers)
    syn.h2_handoff = True
    assert syn.pass_plan(32) is on
    syn.h3_min_batch = 99
    assert all(lp.kind != _lib.NB_KERNEL_LARGE_H3 for lp in syn.pass_plan(32).layers)


def test_plan_arguments_are_checked(library):
    c = native_config(cfgmod.style1_config(128))
    o, p = _lib.NbPlanOptions(), _lib.NbPassPlan()
    assert library.nb_plan_options_default(ctypes.byref(o)) == 0
    assert library.nb_synthesis_plan(ctypes.byref(c), ctypes.byref(o), 0, ctypes.byref(p)) == _lib.NB_EINVAL
    assert b"batch 0" in library.nb_last_error()
    o.conv_mode = 9
    assert library.nb_synthesis_plan(ctypes.byref(c), ctypes.byref(o), 1, ctypes.byref(p)) == _lib.NB_EINVAL
    assert b"conv_mode" in library.nb_last_error()


def test_styles_fast_only_within_its_lds_array(library):
    """nb_styles_fast_f32 keeps a layer's squared styles in a 1024-entry LDS array: a table with a c_aff past it (a conv0 with a
    wide geometry feature, or a ToRGB of 1016+ channels: c + 9) is planned on nb_styles_f32, at every batch and mode."""
    wide = [cfgmod.GeneratorConfig(z_dim=64, w_dim=64, img_resolution=16, channel_base=512, channel_max=32,
                                   geom_feature_channels=(1100,), geom_feature_resolutions=(8,)),
            cfgmod.GeneratorConfig(z_dim=64, w_dim=64, img_resolution=8, channel_base=8192, channel_max=1016,
                                   geom_feature_channels=(8,), geom_feature_resolutions=(4,))]
    edge = cfgmod.GeneratorConfig(z_dim=64, w_dim=64, img_resolution=16, channel_base=512, channel_max=32,
                                  geom_feature_channels=(992,), geom_feature_resolutions=(8,))        # c_aff = 1024 exactly
    for cfg, fast in [(c, False) for c in wide] + [(edge, True)]:
        syn = SynthesisNetwork(cfg)
        for mode in ALL:
            syn.conv_mode = mode
            for n in BATCHES:
                kp = syn.pass_plan(n)
                assert kp.styles_fast == fast and (fast or not kp.styles_noise), (cfg, mode, n)
