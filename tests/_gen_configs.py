"""Generator configurations that reach the per-batch kernel decisions the shipped style1 shapes never take, shared by the CPU and GPU
tests.  The decisions live once, in the library's planner (nb_synthesis_plan, csrc/nb_gen_plan.hip), which SynthesisNetwork
(networks.py) and the C entry's gen_walk both follow.  These nets have ragged channel counts (c_in not a multiple of 8 or 16, partial
64-channel c_out slices), no conv_clamp, a w_dim that is not a multiple of 16 and geometry layouts other than the default two features.

Each entry names the decision branches ("rows") it exists for and the conv modes that must reach them at some batch of BATCHES.
``rows_reached`` derives the rows from the kernels a pass ran (NativeGenerator.describe or SynthesisNetwork.layer_kernels, the ToRGB's
entry included) and the layer shapes, so that the tests fail when a later change to a threshold turns one of these cases into a no-op."""
import dataclasses

from brushstroke_engine_amd import config as cfgmod

# every eligibility threshold of the split-f16 kernels lies between two of these: 8 / 9 switches the fused styles + noise launch and
# positions_once, 15 / 16 the w8 / w16 up=2 paths; h3_min_pixels (128 x 128) falls at n = 4 for R = 64 layers and n = 1 for R = 128
BATCHES = (1, 3, 8, 9, 15, 16, 32)
SPLIT = ("h3", "f8")
ALL = ("f32", "h3", "f8")

ROWS = {
    "h2_operands_large": "f8 mode: a large split-f16 kernel reads H2 operands (operand format 0: c_in % 16 != 0)",
    "large_cin_not8": "a large split-f16 kernel with c_in % 8 != 0",
    "large_partial_cout": "a large split-f16 kernel with a partial 64-channel c_out slice",
    "w8_up2_ragged": "the large up=2 kernel on an 8x8 input (batch >= 16) with c_in % 16 != 0 or c_out % 64 != 0",
    "handoff_refused": "two consecutive large layers, the operand hand-off refused (c_out % 8, or an f8 consumer and c_out % 16)",
    "early_pack": "a geometry feature packed into its consumer's operands at the start of the pass",
    "early_pack_refused": "producer and consumer of a geometry feature both large, the early pack refused for the channel counts",
    "large_last_fused_torgb": "the last layer on a large kernel with the ToRGB fused into it (c_last <= 128)",
    "large_last_standalone_torgb": "the last layer on a large kernel, then the standalone ToRGB (c_last > 128)",
    "split_f32_fallback": "split mode, a small layer on the fp32 kernel because c_in % 16 != 0",
    "no_clamp": "no conv_clamp: no split-f16 kernel in any layer",
    "styles_slow": "nb_styles_f32 and a separate noise launch (w_dim % 16 != 0)",
    "geom_layout": "a geometry layout other than two features at (R/8, R/4)",
}


def _net(res, cmax, cbase, geom, geom_res=()):
    return cfgmod.GeneratorConfig(z_dim=64, w_dim=64, img_resolution=res, channel_base=cbase, channel_max=cmax,
                                  geom_feature_channels=geom, geom_feature_resolutions=geom_res)


# id -> (config, {row: conv modes that must reach it})
CONFIGS = {
    "C1": (cfgmod.tiny_config(32),
           {"split_f32_fallback": SPLIT, "h2_operands_large": ("f8",), "w8_up2_ragged": SPLIT, "large_partial_cout": SPLIT}),
    "C2": (_net(64, 96, 4096, (8, 24)),
           {"split_f32_fallback": SPLIT, "h2_operands_large": ("f8",), "w8_up2_ragged": SPLIT, "large_partial_cout": SPLIT}),
    "C3": (_net(128, 72, 8192, (16, 40)),
           {"h2_operands_large": ("f8",), "handoff_refused": ("f8",), "early_pack_refused": ("f8",), "early_pack": ("h3",),
            "split_f32_fallback": SPLIT, "large_partial_cout": SPLIT, "w8_up2_ragged": SPLIT}),
    "C4": (_net(64, 160, 16384, (16, 256)),
           {"large_last_standalone_torgb": SPLIT, "large_partial_cout": SPLIT, "w8_up2_ragged": SPLIT}),
    "C5": (_net(128, 100, 12800, (5, 21)),
           {"h2_operands_large": ("f8",), "handoff_refused": SPLIT, "early_pack_refused": SPLIT, "large_cin_not8": SPLIT,
            "large_partial_cout": SPLIT, "split_f32_fallback": SPLIT, "w8_up2_ragged": SPLIT}),
    "C6": (dataclasses.replace(cfgmod.style1_config(128), conv_clamp=None), {"no_clamp": SPLIT}),
    "C7": (dataclasses.replace(cfgmod.style1_config(128), z_dim=40, w_dim=40, mapping_layers=2),
           {"styles_slow": ALL, "early_pack": SPLIT, "large_last_fused_torgb": SPLIT}),
    "C8_nogeom": (_net(64, 96, 4096, ()), {"geom_layout": ALL, "w8_up2_ragged": SPLIT}),
    "C8_one": (_net(64, 96, 4096, (12,), (16,)),
               {"geom_layout": ALL, "large_cin_not8": SPLIT, "h2_operands_large": ("f8",), "split_f32_fallback": SPLIT}),
    "C8_three": (_net(64, 96, 4096, (12, 20, 36), (8, 16, 32)),
                 {"geom_layout": ALL, "large_cin_not8": SPLIT, "early_pack": SPLIT, "h2_operands_large": ("f8",),
                  "split_f32_fallback": SPLIT}),
}


def kernel_kind(name: str) -> str:
    """'large' (split-f16 large-tile kernels), 'small' (split-f16 small-image kernel) or 'f32' (exact-fp32 kernels)."""
    if name.startswith("modconv3x3_up1_h3_kernel") or name in ("modconv3x3_up2_h3_kernel", "modconv3x3_up2v_kernel"):
        return "large"
    if name == "modconv3x3_up1_small_h3_kernel":
        return "small"
    if name.startswith(("modconv3x3_up1_kernel<", "modconv3x3_up2_kernel<")):
        return "f32"
    raise ValueError(f"unknown kernel {name!r}")


def rows_reached(cfg, mode, kernels, formats=None):
    """The ROWS one pass took, from {layer name: kernel} and the layer shapes.  ``formats`` (SynthesisNetwork.layer_formats) is
    checked where given: every large layer on H2 operands must have recorded format 0."""
    layers = cfg.layers
    kind = {s.name: kernel_kind(kernels[s.name]) for s in layers}
    large = lambda s: kind[s.name] == "large"                                   # noqa: E731
    fmt = lambda s: 1 if mode == "f8" and s.in_channels % 16 == 0 else 0        # noqa: E731  (the operand format a large layer reads)
    rows = set()
    for i, s in enumerate(layers):
        nxt = layers[i + 1] if i + 1 < len(layers) else None
        last = nxt is None
        if large(s):
            if fmt(s) == 0 and mode == "f8":
                rows.add("h2_operands_large")
                if formats is not None and formats.get(s.name) != 0:
                    raise AssertionError(f"{s.name}: c_in {s.in_channels} on operand format {formats.get(s.name)}, expected 0")
            if s.in_channels % 8:
                rows.add("large_cin_not8")
            if s.out_channels % 64:
                rows.add("large_partial_cout")
            if s.up == 2 and s.in_res == 8 and (s.in_channels % 16 or s.out_channels % 64):
                rows.add("w8_up2_ragged")
            if last:
                if kernels.get(cfg.torgb_name) == kernels[s.name]:
                    rows.add("large_last_fused_torgb")
                elif kernels.get(cfg.torgb_name) == "torgb_triad_kernel":
                    rows.add("large_last_standalone_torgb")
            elif large(nxt):
                geo = cfg.geom_channels_at(s.block_res) if s.up == 1 else 0
                if not (s.out_channels % 8 == 0 and (fmt(nxt) == 0 or (s.out_channels % 16 == 0 and geo % 16 == 0))):
                    rows.add("handoff_refused")
        elif kind[s.name] == "f32" and mode in SPLIT and cfg.conv_clamp is not None and s.in_channels % 16:
            if (s.up == 1 and s.block_res <= 64) or (s.up == 2 and s.in_res <= 32):
                rows.add("split_f32_fallback")
    for gch, gres in zip(cfg.geom_feature_channels, cfg.geom_feature_resolutions):
        sp = next(s for s in layers if s.name == f"synthesis.b{gres}.conv1")
        sc = next(s for s in layers if s.name == f"synthesis.b{2 * gres}.conv0")
        if large(sp) and large(sc):
            ok = sp.out_channels % 8 == 0 and (fmt(sc) == 0 or (sp.out_channels % 16 == 0 and gch % 16 == 0))
            rows.add("early_pack" if ok else "early_pack_refused")
    if mode in SPLIT and cfg.conv_clamp is None and all(k == "f32" for k in kind.values()):
        rows.add("no_clamp")
    if not (cfg.w_dim % 16 == 0 and all(s.out_channels % 4 == 0 for s in layers)):
        rows.add("styles_slow")
    r = cfg.img_resolution
    if cfg.geom_feature_resolutions != (r // 8, r // 4):
        rows.add("geom_layout")
    return rows


def expected_rows(cid, mode):
    return {row for row, modes in CONFIGS[cid][1].items() if mode in modes}
