"""Paint a drawing layer by layer, every layer with its own brush, on a canvas that stays on the device
(``painting.PaintSession``): the command-line counterpart of what a paint program does with the engine.

    python -m brushstroke_engine_amd.paint_session_main --gan_checkpoint engine.npz --script session.json \\
        --output_file_prefix out/session [--on_white] [--conv_mode h3] [--uvs_calibration cal.npz]

The script is JSON::

    {"size": [H, W], "crop_margin": 10, "feature_blending_level": 0,
     "layers": [{"strokes": <what painting.StrokeList.from_json reads>, "library": "rand100", "style_id": "...",
                 "colors": [[r, g, b] | null, ...], "mode": "paint" | "erase", "opacity": 255, "uvs_mapping": true}, ...]}

``crop_margin`` (10), ``feature_blending_level`` (0), and per layer ``library`` ("rand100"), ``colors`` (none; up to three of 0..255
values: primary, secondary, canvas colour; null keeps the style's), ``mode`` ("paint") and ``opacity`` (255) are optional.  The layers are
added in order; one PNG is written: ``<prefix>.png``.  Single process.

``--uvs_calibration`` takes the ``.npz`` of ``paint_image_main`` ('medium' and 'thick' calibration drawings) and turns the clear-background
mapping on for every layer that does not say ``"uvs_mapping": false``; the brushes of the script are calibrated together
(``StyleUVSMapper.calibrate``) before the first layer is added.  Without the flag a layer must not ask for ``"uvs_mapping": true``.
"""
from __future__ import annotations

import argparse
import json
import logging
import os

import torch

from . import encoder, formats, painting
from . import launch
from .networks import DEFAULT_CONV_MODE, Generator

logger = logging.getLogger(__name__)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Layered painting session on MI355X.")
    ap.add_argument("--gan_checkpoint", required=True, help=".npz engine container (generator + encoder)")
    ap.add_argument("--script", required=True, help="JSON session script: size, layers of strokes with their brushes")
    ap.add_argument("--output_file_prefix", required=True)
    ap.add_argument("--on_white", action="store_true")
    ap.add_argument("--uvs_calibration", default=None,
                    help=".npz with 'medium' and 'thick' [5,R,R] uint8 calibration drawings (StyleUVSMapper): clear-background mapping "
                         "for every layer that does not set \"uvs_mapping\": false")
    ap.add_argument("--conv_mode", default=None, choices=["f8", "h3", "f32"],
                    help="arithmetic of the conv layers (default: networks.DEFAULT_CONV_MODE)")
    return ap


def _int(value, what: str) -> int:
    if isinstance(value, bool) or not isinstance(value, int):
        raise ValueError(f"session script: {what} must be an integer, got {value!r}")
    return value


def parse_script(data) -> dict:
    """The decoded script, checked and with its defaults filled in: {"size": (H, W), "crop_margin", "feature_blending_level",
    "layers": [{"strokes": StrokeList, "library", "style_id", "colors", "mode", "opacity", "uvs_mapping": True | False | None (not
    said)}]}.  ValueError for anything else."""
    if isinstance(data, (str, bytes)):
        data = json.loads(data)
    if not isinstance(data, dict):
        raise ValueError("session script: an object with 'size' and 'layers' expected")
    size = data.get("size")
    if not isinstance(size, (list, tuple)) or len(size) != 2:
        raise ValueError(f"session script: 'size' must be [H, W], got {size!r}")
    h, w = _int(size[0], "size"), _int(size[1], "size")
    if h < 1 or w < 1:
        raise ValueError(f"session script: 'size' must be positive, got {size!r}")
    margin = _int(data.get("crop_margin", 10), "crop_margin")
    level = _int(data.get("feature_blending_level", 0), "feature_blending_level")
    if margin < 0 or level < 0:
        raise ValueError("session script: crop_margin and feature_blending_level must not be negative")
    layers = data.get("layers")
    if not isinstance(layers, list) or not layers:
        raise ValueError("session script: 'layers' must be a non-empty list")
    out = []
    for i, layer in enumerate(layers):
        if not isinstance(layer, dict) or "strokes" not in layer or "style_id" not in layer:
            raise ValueError(f"session script: layer {i} needs 'strokes' and 'style_id'")
        mode = layer.get("mode", "paint")
        if mode not in painting.COMPOSE_MODES:
            raise ValueError(f"session script: layer {i}: mode {mode!r} is neither 'paint' nor 'erase'")
        opacity = _int(layer.get("opacity", 255), f"layer {i}: opacity")
        if not 0 <= opacity <= 255:
            raise ValueError(f"session script: layer {i}: opacity {opacity} outside 0..255")
        colors = layer.get("colors") or []
        if not isinstance(colors, list) or len(colors) > 3:
            raise ValueError(f"session script: layer {i}: 'colors' takes up to three entries")
        for c in colors:
            if c is not None and not (isinstance(c, list) and len(c) == 3 and all(0 <= _int(v, "a colour value") <= 255 for v in c)):
                raise ValueError(f"session script: layer {i}: a colour is [r, g, b] in 0..255 or null, got {c!r}")
        mapping = layer.get("uvs_mapping")
        if mapping is not None and not isinstance(mapping, bool):
            raise ValueError(f"session script: layer {i}: 'uvs_mapping' must be true or false, got {mapping!r}")
        out.append({"strokes": painting.StrokeList.from_json(layer["strokes"]), "library": str(layer.get("library", "rand100")),
                    "style_id": str(layer["style_id"]), "colors": colors, "mode": mode, "opacity": opacity, "uvs_mapping": mapping})
    return {"size": (h, w), "crop_margin": margin, "feature_blending_level": level, "layers": out}


def layer_options(layer: dict, libraries: dict, z_dim: int) -> painting.GanBrushOptions:
    """The brush of one layer.  ``libraries`` keeps one library per ``library`` string for the whole script (``rand<N>`` draws its
    styles from one generator, in order)."""
    lib = libraries.get(layer["library"])
    if lib is None:
        lib = libraries[layer["library"]] = formats.BrushLibrary.from_arg(layer["library"], z_dim=z_dim)
    opts = painting.GanBrushOptions()
    for i, c in enumerate(layer["colors"]):
        if c is not None:
            opts.set_color(i, torch.tensor(c, dtype=torch.float32) / 255.0)
    lib.set_style(layer["style_id"], opts)
    return opts


def run_script(helper: painting.PaintingHelper, script: dict, z_dim: int) -> painting.PaintSession:
    """A session on ``helper`` with every layer of the parsed ``script`` added.  With a ``helper.uvs_mapper`` the layers paint with the
    clear-background mapping unless they say ``"uvs_mapping": false``, and the distinct brushes among them are calibrated by ONE
    ``calibrate`` call before the first layer is added (a brush without a ``style_id`` -- ``rand<N>`` -- cannot be looked up again and
    is calibrated when its layer is added)."""
    helper.set_feature_blending(script["feature_blending_level"])
    session = painting.PaintSession(helper, script["size"], crop_margin=script["crop_margin"])
    libraries: dict = {}
    mapper = helper.uvs_mapper
    brushes = [layer_options(layer, libraries, z_dim) for layer in script["layers"]]
    for i, (layer, opts) in enumerate(zip(script["layers"], brushes)):
        if mapper is None and layer.get("uvs_mapping"):
            raise RuntimeError(f"session script: layer {i} asks for uvs_mapping: that needs --uvs_calibration")
        opts.enable_uvs_mapping = mapper is not None and layer.get("uvs_mapping") is not False
    with torch.no_grad():
        if mapper is not None:
            todo = {}
            for opts in brushes:
                if opts.enable_uvs_mapping and opts.style_id is not None and opts.style_id not in mapper.sfactors:
                    todo.setdefault(opts.style_id, opts)
            if todo:
                mapper.calibrate(list(todo.values()), batch=helper.batch)
        for layer, opts in zip(script["layers"], brushes):
            session.add(layer["strokes"], opts, mode=layer["mode"], opacity=layer["opacity"])
    return session


def main(argv=None) -> str:
    args = build_parser().parse_args(argv)
    with open(args.script) as f:
        script = parse_script(f.read())
    _, _, device, _ = launch.init()                  # kernel library first, then the device
    cfg, gen_sd, enc_sd, preproc, _ = formats.load_engine_snapshot(args.gan_checkpoint)
    G = Generator(cfg, gen_sd, conv_mode=args.conv_mode or DEFAULT_CONV_MODE).to(device)
    if not encoder.HipGeometryEncoder.supports(cfg.img_resolution):
        raise RuntimeError(f"the geometry-encoder kernels tile patches of 32, 64 or 128 k pixels; this checkpoint paints {cfg.img_resolution}")
    ops = painting.TileOps(G, encoder.HipGeometryEncoder(enc_sd, preproc_type=preproc, device=device))
    mapper = None
    if args.uvs_calibration:
        from .drawings import load_calibration
        mapper = painting.StyleUVSMapper(ops, *load_calibration(args.uvs_calibration, cfg.img_resolution, device))
    session = run_script(painting.PaintingHelper(ops, uvs_mapper=mapper), script, G.z_dim)
    from PIL import Image
    output_file = args.output_file_prefix + ".png"
    os.makedirs(os.path.dirname(os.path.abspath(output_file)), exist_ok=True)
    Image.fromarray(session.image(on_white=args.on_white)).save(output_file)
    logger.info(f"Saved result to: {output_file}")
    print(output_file)
    return output_file


if __name__ == "__main__":
    main()
