"""GPU: a PROJECTED brush (W+ code plus noise buffers in ``opts.custom_args``, what formats.WBrushLibrary hands to ``set_style_w``)
through the painting engine.  The reference renders such a brush with ``**opts.custom_args`` (forger/ui/brush.py:746-754);
tests/golden/engine_brush_noise_r128.npz holds two overlapping tiles it painted with the buffers, and the same two without."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from brushstroke_engine_amd import config as cfgmod, weights as wmod, encoder as encmod, painting
from brushstroke_engine_amd.networks import Generator
from brush_noise_refs import fixture_buffers, fixture_patches

pytestmark = pytest.mark.gpu
# the caps tests/test_hip_painting.py applies to its stroke sequence: <= 1 LSB, on at most this share of the bytes
MAX_FRAC = {"f32": 1e-3, "h3": 1e-3, "f8": 5e-3}


@pytest.fixture(scope="module")
def fx():
    g = load_golden("engine_brush_noise_r128.npz")
    cfg = cfgmod.style1_config(int(g["resolution"]))
    return dict(g=g, cfg=cfg, sd=wmod.random_state_dict(cfg, seed=int(g["weights_seed"])),
                esd=encmod.random_encoder_state_dict(int(g["encoder_seed"])), bufs=fixture_buffers(g, cfg), patches=fixture_patches(g))


def tile_ops(fx, mode, noise=None):
    """TileOps on the fixture's generator; ``noise``: a buffer dict written into the CHECKPOINT's noise_const instead."""
    sd = dict(fx["sd"])
    for k, v in (noise or {}).items():
        sd["synthesis." + k] = v
    G = Generator(fx["cfg"], sd, conv_mode=mode).to("cuda")
    return painting.TileOps(G, encmod.HipGeometryEncoder(fx["esd"]))


def w_brush(fx, bufs):
    opts = painting.GanBrushOptions()
    opts.set_style_w(torch.from_numpy(fx["g"]["ws"]), 594, custom_args=None if bufs is None else {"noise_buffers": bufs})
    return opts


def strokes(fx, helper, opts_of, level=None):
    g = fx["g"]
    helper.make_new_canvas(int(g["size"]), int(g["size"]), feature_blending=int(g["level"]) if level is None else level)
    tiles = []
    for i, (x, y) in enumerate(g["xy"].tolist()):
        opts = opts_of(i)
        opts.set_position(x, y)
        res, _, _ = helper.render_stroke(fx["patches"][i], None, opts, meta={"x": x, "y": y, "crop_margin": int(g["crop_margin"])})
        tiles.append(res)
    return np.stack(tiles)


def close_to_reference(got, want, mode, what):
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"[brush noise painting {mode}] {what}: max {d.max()} LSB, share of differing bytes {(d > 0).mean():.2e} (cap {MAX_FRAC[mode]:.0e})")
    assert d.max() <= 1, (what, d.max())
    assert (d > 0).mean() <= MAX_FRAC[mode], (what, (d > 0).mean())


@pytest.mark.parametrize("mode", ["f32", "h3", "f8"])
def test_render_stroke_matches_the_reference(fx, mode):
    ops = tile_ops(fx, mode)
    bufs = {k: torch.from_numpy(v) for k, v in fx["bufs"].items()}
    brush, plain = w_brush(fx, bufs), painting.GanBrushOptions()
    plain.set_style_w(torch.from_numpy(fx["g"]["ws"]), 594, custom_args={})
    # without buffers (custom_args == {}): the checkpoint's noise, as before
    close_to_reference(strokes(fx, painting.PaintingHelper(ops), lambda i: plain), fx["g"]["tiles_plain"], mode, "without buffers")
    # with the brush's buffers
    close_to_reference(strokes(fx, painting.PaintingHelper(ops), lambda i: brush), fx["g"]["tiles_noise"], mode, "with buffers")


def test_paint_image_equals_a_checkpoint_that_holds_the_buffers(fx):
    """2 x 2 tiles, feature blending level 2, batch 2: two batches on the two stream slots, staged head / tail passes."""
    geom = load_golden("engine_r128.npz")["geom"][:150, :150, None]
    runs = []
    for ops, opts in ((tile_ops(fx, "f8"), w_brush(fx, fx["bufs"])), (tile_ops(fx, "f8", noise=fx["bufs"]), w_brush(fx, None))):
        helper = painting.PaintingHelper(ops, batch=2)
        helper.set_feature_blending(2)
        out, full, crops, _ = helper.paint_image(geom, opts, crop_margin=10, return_full=True)
        assert len(crops) == 4 and ops.n_streams == 2
        runs.append((out, full, helper.features.clone()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2].cpu(), runs[1][2].cpu())
    # ... and without feature blending (whole passes)
    outs = []
    for ops, opts in ((tile_ops(fx, "f8"), w_brush(fx, fx["bufs"])), (tile_ops(fx, "f8", noise=fx["bufs"]), w_brush(fx, None))):
        outs.append(painting.PaintingHelper(ops, batch=2).paint_image(geom, opts, crop_margin=10))
    assert np.array_equal(outs[0], outs[1])
    plain = painting.PaintingHelper(tile_ops(fx, "f8"), batch=2).paint_image(geom, w_brush(fx, None), crop_margin=10)
    d = np.abs(plain.astype(np.int32) - outs[0].astype(np.int32))
    assert (d > 1).mean() > 0.05                      # (the brush's noise is in the picture)


@pytest.mark.parametrize("level", [0, 2])
def test_single_tile_graphs_follow_the_brush(fx, level):
    """render_stroke replays captured passes (TileOps.graph_single).  The captured graphs read the helper's ONE set, so a second
    brush -- another buffer dict handed to set_style_w -- is one reload and no new graph."""
    g = fx["g"]
    second = {k: np.ascontiguousarray(v[::-1] * np.float32(0.5)) for k, v in fx["bufs"].items()}
    ops = tile_ops(fx, "h3")
    helper = painting.PaintingHelper(ops)
    assert helper.graph_strokes
    brushes = [w_brush(fx, fx["bufs"]), w_brush(fx, second)]
    got = {}
    for name, order in (("first", (0, 0)), ("second", (1, 1)), ("mixed", (0, 1))):
        got[name] = strokes(fx, helper, lambda i: brushes[order[i]], level)
        n_graphs = len(ops._graphs)
    assert n_graphs == (2 if level else 1) and helper._noise_set is not None
    ref = {}
    for name, noise in (("first", fx["bufs"]), ("second", second)):
        h2 = painting.PaintingHelper(tile_ops(fx, "h3", noise=noise))
        ref[name] = strokes(fx, h2, lambda i: w_brush(fx, None), level)
    assert np.array_equal(got["first"], ref["first"])
    assert np.array_equal(got["second"], ref["second"])
    assert not np.array_equal(got["first"], got["second"])
    assert np.array_equal(got["mixed"][0], ref["first"][0])            # the first stroke of "mixed" is the first brush's ...
    assert not np.array_equal(got["mixed"][1], ref["first"][1])        # ... the second one followed the new brush
