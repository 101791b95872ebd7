"""The brush catalogue without a GPU: ``StyleUVSMapper``'s colours, icons and batched calibration on the oracle-backed ops against
what the REFERENCE mapper produced (tests/golden/brush_catalogue_r128.npz), the torch route of ``masked_kth_largest``, the C entry's
argument checks and the command lines."""
import ctypes
import json

import numpy as np
import pytest
import torch

import brush_catalogue_cases as bc
from conftest import load_golden
from brushstroke_engine_amd import _lib, config as cfgmod, weights as wmod, encoder as encmod, formats, paint_image_main, painting
from oracle_tile_ops import OracleTileOps


@pytest.fixture(scope="module")
def cat():
    """The mapper on the R=128 engine of tests/test_painting_cpu.py, the four fixture brushes one by one, and their catalogue at batch 10
    (two brushes per pass, two passes)."""
    e, g = load_golden("engine_r128.npz"), load_golden("brush_catalogue_r128.npz")
    cfg = cfgmod.style1_config(int(g["resolution"]))
    ops = OracleTileOps(cfg, wmod.random_state_dict(cfg, seed=int(g["weights_seed"])), encmod.random_encoder_state_dict(int(g["encoder_seed"])))
    mapper = painting.StyleUVSMapper(ops, e["uvs_cal_medium"], e["uvs_cal_thick"])
    lib = bc.FixtureLibrary(g, cfg.z_dim)
    single = []
    for sid in lib.get_style_ids():
        o = painting.GanBrushOptions()
        lib.set_style(sid, o)
        single.append(dict(colors=mapper.get_colors_raw(o).numpy(), spec=mapper.get_colors(o), white=mapper.get_brush_icon(o),
                           plain=mapper.get_brush_icon(o, on_white=False), sf=float(mapper.get_sfactor(o))))
    mapper.sfactors = {}
    batched = mapper.catalogue(lib, batch=10)
    return dict(e=e, g=g, cfg=cfg, ops=ops, mapper=mapper, lib=lib, single=single, batched=batched)


def test_mapper_matches_reference(cat):
    g = cat["g"]
    for i, s in enumerate(cat["single"]):
        assert s["colors"].shape == (1, 3, 3)
        assert np.abs(s["colors"][0] - g["colors_raw"][i]).max() <= 1e-5            # the oracle's stated distance from the reference
        bc.canvas_close(s["white"], g["icons_on_white"][i])
        bc.canvas_close(s["plain"], g["icons_plain"][i])
        assert s["white"].shape == (128, 128, 3) and s["white"].dtype == np.uint8
        assert np.abs(bc.spec_ints(s["spec"]) - bc.spec_ints(str(g["color_specs"][i]))).max() <= 1
        assert len(bc.spec_ints(s["spec"])) == 9 and s["spec"].count("rgb(") == 3
        np.testing.assert_allclose(s["sf"], float(g["sfactors"][i]), rtol=1e-5)


def test_catalogue_equals_single_calls(cat):
    b, single = cat["batched"], cat["single"]
    assert b.ids == cat["lib"].get_style_ids() and len(b.opts) == 4
    assert b.colors_raw.shape == (4, 3, 3) and b.icons.shape == (4, 128, 128, 3) and b.sfactors.shape == (4,)
    for i, s in enumerate(single):
        assert np.array_equal(b.colors_raw[i], s["colors"][0])
        assert b.color_specs[i] == s["spec"]
        assert np.array_equal(b.icons[i], s["white"])
        assert float(b.sfactors[i]) == s["sf"]
    # the catalogue filled the factor cache like calibrate
    assert sorted(cat["mapper"].sfactors) == sorted(b.ids)
    assert float(cat["mapper"].get_sfactor(b.opts[2])) == single[2]["sf"]


def test_calibrate_caches_only_brushes_with_an_id(cat):
    e, ops, lib = cat["e"], cat["ops"], cat["lib"]
    mapper = painting.StyleUVSMapper(ops, e["uvs_cal_medium"], e["uvs_cal_thick"])
    named, anon = painting.GanBrushOptions(), painting.GanBrushOptions()
    lib.set_style("0", named)
    lib.set_style("1", anon)
    anon.style_id = None
    sf = mapper.calibrate([named, anon], batch=10)
    assert sf.shape == (2,) and list(mapper.sfactors) == ["0"]
    assert float(sf[0]) == cat["single"][1]["sf"] and float(sf[1]) == cat["single"][2]["sf"]
    assert mapper.calibrate([]).shape == (0,)
    with pytest.raises(RuntimeError, match="no calibration"):
        painting.StyleUVSMapper(ops).get_sfactor(named)
    with pytest.raises(RuntimeError, match="no calibration"):
        painting.StyleUVSMapper(ops).get_colors_raw(named)


def test_random_library_entry_reproduces_its_icon(cat):
    """``rand<N>`` draws a fresh latent at every ``set_style``: the catalogue keeps the options it rendered, and they paint that brush."""
    mapper = cat["mapper"]
    b = mapper.catalogue(formats.RandomBrushLibrary(2, cat["cfg"].z_dim), batch=10, icon_k=4)
    full = mapper.catalogue(formats.RandomBrushLibrary(2, cat["cfg"].z_dim), batch=10)
    assert b.ids == ["rand0", "rand1"] and b.icons.shape == (2, 32, 32, 3)
    for i in range(2):
        assert b.opts[i].style_id is None
        icon = mapper.get_brush_icon(b.opts[i])
        assert np.array_equal(icon, full.icons[i])
        rgba = np.concatenate([icon, np.full((128, 128, 1), 255, np.uint8)], axis=2)
        assert np.array_equal(b.icons[i], painting.canvas_view_numpy(rgba, 0, 0, 128, 128, 4)[..., :3])
    assert not np.array_equal(full.icons[0], full.icons[1])
    for bad in (0, 17, 3):
        with pytest.raises(ValueError):
            mapper.catalogue(cat["lib"], icon_k=bad)


@pytest.mark.parametrize("name,x,masks,ks", bc.cases(), ids=[c[0] for c in bc.cases()])
def test_masked_kth_largest_torch_route(name, x, masks, ks):
    ops = painting.TileOpsBase()
    n, count = x.shape
    h = 33 if count == 1089 else 1
    strided = torch.full([n, 3, h, count // h], 1e30)                  # the uvs[:, 2] view
    strided[:, 2] = torch.from_numpy(x).view(n, h, count // h)
    for k in ks:
        want, cnt = bc.kth_largest_numpy(x, masks, k)
        for xt, mt in ((torch.from_numpy(x).view(n, 1, h, count // h), torch.from_numpy(masks).view(-1, 1, h, count // h) != 0),
                       (strided[:, 2], torch.from_numpy(masks).view(-1, h, count // h))):
            kth, n_masked = ops.masked_kth_largest(xt, mt, k)
            assert kth.dtype == torch.float32 and n_masked.dtype == torch.int32
            assert np.array_equal(kth.numpy(), want, equal_nan=True), (name, k)
            assert np.array_equal(n_masked.numpy(), cnt), (name, k)
    with pytest.raises(ValueError):
        ops.masked_kth_largest(torch.from_numpy(x).view(n, 1, h, count // h), torch.from_numpy(masks).view(-1, count)[:, :-1], 1)
    with pytest.raises(ValueError):
        ops.masked_kth_largest(torch.from_numpy(x).view(n, 1, h, count // h), torch.from_numpy(masks), 0)


def test_too_few_background_pixels(cat):
    e = cat["e"]
    thick = e["uvs_cal_thick"].copy()
    thick[3] = 0
    thick[3].reshape(-1)[:14] = 255
    with pytest.raises(RuntimeError, match="drawing 3"):
        painting.StyleUVSMapper(cat["ops"], e["uvs_cal_medium"], thick)
    thick[3].reshape(-1)[14] = 255                                    # 15 are enough
    painting.StyleUVSMapper(cat["ops"], e["uvs_cal_medium"], thick)


def test_c_entry_argument_checks():
    """Validation happens on the host before any HIP call: usable without a GPU."""
    library = _lib.lib()
    x = np.zeros(64, np.float32)
    mask = np.ones(64, np.uint8)
    kth, cnt = np.zeros(4, np.float32), np.zeros(4, np.int32)
    X, M, K, N = x.ctypes.data, mask.ctypes.data, kth.ctypes.data, cnt.ctypes.data

    def call(x=X, stride=16, mask=M, n_masks=1, count=16, k=1, n=4, kth=K, n_masked=N):
        return library.nb_masked_kth_largest_f32(x, stride, mask, n_masks, count, k, n, kth, n_masked, None)
    for bad, word in ((dict(x=None), "null"), (dict(mask=None), "null"), (dict(kth=None), "null"), (dict(n_masked=None), "null"),
                      (dict(k=0), "k = 0"), (dict(k=-3), "k = -3"), (dict(count=0, stride=0), "count 0"), (dict(n_masks=0), "n_masks 0"),
                      (dict(n=-1), "n -1"), (dict(stride=15), "stride_n 15"), (dict(x=X + 2), "aligned")):
        rc = call(**bad)
        assert rc == _lib.NB_EINVAL, bad
        assert word.encode() in library.nb_last_error(), (bad, library.nb_last_error())
        with pytest.raises(_lib.NeubeHipError):
            _lib.check(rc, "masked_kth_largest")
    assert call(n=0) == 0
    assert _lib.PROTOTYPES["nb_masked_kth_largest_f32"][1][1] is ctypes.c_longlong


def test_set_colors_from_another_style():
    class StubMapper:
        def get_colors_raw(self, opts):
            self.asked = opts.style_id
            return torch.tensor([[[0.5, -1.0, 0.1], [0.0, 1.0, 0.2], [-0.5, 0.25, 0.3]]])
    lib, mapper = formats.SeedBrushLibrary([594, 12], 64), StubMapper()
    opts = painting.GanBrushOptions()
    paint_image_main.set_colors("2", opts, lib, mapper, "594", "12")
    assert mapper.asked == "12"
    assert torch.equal(opts.color0, torch.tensor([[0.75, 0.5, 0.25]])) and torch.equal(opts.color1, torch.tensor([[0.0, 1.0, 0.625]]))
    assert opts.canvas_color is None
    paint_image_main.set_colors("1", opts, lib, mapper, "594", "12")
    assert mapper.asked == "594"
    for mode in ("1", "2"):
        with pytest.raises(RuntimeError, match="--uvs_calibration"):
            paint_image_main.set_colors(mode, painting.GanBrushOptions(), lib, None, "594", "12")
    with pytest.raises(RuntimeError, match="style_id2"):
        paint_image_main.set_colors("2", painting.GanBrushOptions(), lib, mapper, "594", None)
    paint_image_main.set_colors("255,0,0;;", opts)                     # explicit colours as before
    assert torch.equal(opts.color0, torch.tensor([[1.0, 0.0, 0.0]]))


def test_catalogue_json_and_sheet(cat, tmp_path):
    b = cat["batched"]
    back = json.loads(b.to_json())
    assert back["ids"] == b.ids and back["color_specs"] == b.color_specs
    assert np.array_equal(np.array(back["sfactors"], np.float32), b.sfactors)
    sheet = b.sheet(cols=3)
    assert sheet.shape == (256, 384, 3)
    assert np.array_equal(sheet[128:, :128], b.icons[3]) and (sheet[128:, 128:] == 255).all()
    from PIL import Image
    from brushstroke_engine_amd import brush_catalogue_main
    png, info = brush_catalogue_main.write_catalogue(b, str(tmp_path / "o" / "lib"), 3)
    assert np.array_equal(np.array(Image.open(png)), sheet) and json.load(open(info)) == back
    args = brush_catalogue_main.build_parser().parse_args(["--gan_checkpoint", "e.npz", "--uvs_calibration", "c.npz", "--output_file_prefix", "o"])
    assert (args.library, args.icon_k, args.cols, args.batch) == ("rand100", 1, 10, 32)


def test_session_script_uvs_mapping_key():
    from brushstroke_engine_amd import paint_session_main
    s = paint_session_main.parse_script({"size": [5, 7], "layers": [{"strokes": [], "style_id": 3},
                                                                     {"strokes": [], "style_id": 4, "uvs_mapping": False}]})
    assert [l["uvs_mapping"] for l in s["layers"]] == [None, False]
    with pytest.raises(ValueError):
        paint_session_main.parse_script({"size": [5, 7], "layers": [{"strokes": [], "style_id": 3, "uvs_mapping": 1}]})
    assert paint_session_main.build_parser().parse_args(["--gan_checkpoint", "e", "--script", "s", "--output_file_prefix", "o",
                                                         "--uvs_calibration", "c.npz"]).uvs_calibration == "c.npz"
