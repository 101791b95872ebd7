"""The brush catalogue on the GPU: the selection kernel (csrc/nb_select.hip) against a numpy statement bit for bit, ``get_sfactor``
through the kernel against the parent's ``torch.topk`` formula, ``StyleUVSMapper`` on the HIP engine against what the REFERENCE mapper
produced (tests/golden/brush_catalogue_r128.npz), and ``paint_session_main --uvs_calibration``."""
import json

import numpy as np
import pytest
import torch

import brush_catalogue_cases as bc
import compose_refs as cr
from conftest import load_golden
from brushstroke_engine_amd import config as cfgmod, encoder as encmod, painting, weights as wmod

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    """The HIP engine of tests/test_hip_painting.py::eng (R=128, conv_mode h3) with the mapper on the stored calibration drawings."""
    e, g = load_golden("engine_r128.npz"), load_golden("brush_catalogue_r128.npz")
    cfg = cfgmod.style1_config(128)
    sd = wmod.random_state_dict(cfg, seed=0)
    esd = encmod.random_encoder_state_dict(5)
    from brushstroke_engine_amd.networks import Generator
    ops = painting.TileOps(Generator(cfg, sd, conv_mode="h3").to("cuda"), encmod.HipGeometryEncoder(esd))
    mapper = painting.StyleUVSMapper(ops, e["uvs_cal_medium"], e["uvs_cal_thick"])
    return dict(e=e, g=g, cfg=cfg, sd=sd, esd=esd, ops=ops, mapper=mapper, lib=bc.FixtureLibrary(g, cfg.z_dim))


@pytest.fixture(scope="module")
def single(eng):
    """The four fixture brushes through the one-brush calls, computed once."""
    out = []
    with torch.no_grad():
        for sid in eng["lib"].get_style_ids():
            o = painting.GanBrushOptions()
            eng["lib"].set_style(sid, o)
            m = eng["mapper"]
            out.append(dict(opts=o, colors=m.get_colors_raw(o).cpu().numpy(), spec=m.get_colors(o), white=m.get_brush_icon(o),
                            plain=m.get_brush_icon(o, on_white=False), sf=float(m.get_sfactor(o))))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------
def _layouts(x):
    """x [n,count] on the device as the views the kernel must read: dense rows starting 0, 1 and 3 floats behind a 16-byte boundary,
    and channel 2 of an [n,3,count] tensor (stride 3 * count, first row at 2 * count).  Everything around the rows is 1e30: a read
    outside a row would win every selection."""
    n, count = x.shape
    xd = torch.from_numpy(x).cuda()
    for off in (0, 1, 3):
        buf = torch.full([n * count + 8], 1e30, dtype=torch.float32, device="cuda")
        assert buf.data_ptr() % 16 == 0
        view = buf[off:off + n * count].view(n, 1, 1, count)
        view.copy_(xd.view(n, 1, 1, count))
        yield f"offset{off}", view
    uvs = torch.full([n, 3, 1, count], 1e30, dtype=torch.float32, device="cuda")
    uvs[:, 2] = xd.view(n, 1, count)
    yield "uvs_channel", uvs[:, 2]


@pytest.mark.parametrize("name,x,masks,ks", bc.cases(), ids=[c[0] for c in bc.cases()])
def test_masked_kth_largest_kernel_bitwise(eng, name, x, masks, ks):
    ops = eng["ops"]
    md = torch.from_numpy(masks).cuda()
    want = {k: bc.kth_largest_numpy(x, masks, k) for k in ks}
    for lname, view in _layouts(x):
        assert view.data_ptr() % 4 == 0
        for k in ks:
            runs = []
            for _ in range(2):
                kth, n_masked = ops.masked_kth_largest(view, md, k)
                runs.append((kth.cpu().numpy(), n_masked.cpu().numpy()))
            (kth, cnt), (kth2, cnt2) = runs
            assert np.array_equal(cnt, want[k][1]), (name, lname, k)
            assert np.array_equal(kth, want[k][0], equal_nan=True), (name, lname, k)
            assert kth.tobytes() == kth2.tobytes() and cnt.tobytes() == cnt2.tobytes(), (name, lname, k)
    # bool masks, and a mask per image
    if masks.shape[0] == 1:
        kth, _ = ops.masked_kth_largest(torch.from_numpy(x).cuda().view(x.shape[0], 1, -1), (md != 0).expand(x.shape[0], -1).contiguous(), ks[0])
        assert np.array_equal(kth.cpu().numpy(), want[ks[0]][0], equal_nan=True)


def test_get_sfactor_equals_the_parent_formula(eng):
    """The batched path keeps the parent's operations: on the SAME S, the kernel route gives the bits of the ``torch.topk`` loop."""
    ops, mapper = eng["ops"], eng["mapper"]
    opts = painting.GanBrushOptions()
    eng["lib"].set_style("594", opts)
    with torch.no_grad():
        n = mapper.bmask.shape[0]
        ws = ops.map_style(z=opts.style_z, ws=opts.style_ws).expand(n, -1, -1).contiguous()
        uvs = ops.triad_debug(ws, mapper.geom_feature)[1]["uvs"]
        S = uvs[:, 2:3]
        val = torch.stack([torch.topk(S[i][mapper.bmask[i]], k=15)[0].min() for i in range(n)]).min()      # the parent, verbatim
        parent = 1 / val
        kth, n_masked = ops.masked_kth_largest(uvs[:, 2], mapper.bmask, 15)
        mine = 1 / kth.view(1, n).min(dim=1)[0]
        assert np.array_equal(n_masked.cpu().numpy(), mapper.bmask.reshape(n, -1).sum(dim=1).cpu().numpy())
        assert mine[0].cpu().numpy().tobytes() == parent.cpu().numpy().tobytes()
        mapper.sfactors.pop("594", None)
        assert mapper.get_sfactor(opts).cpu().numpy().tobytes() == parent.cpu().numpy().tobytes()
        assert "594" in mapper.sfactors and ops.background_weight(ws, mapper.geom_feature).shape == S.shape


def test_indexed_geometry_provider_still_hands_off():
    """R=256, five samples: the layer that consumes the 256-channel geometry feature takes its operands from the encoder.  A provider
    whose plain features exist already -- the per-brush ``get_sfactor`` of before indexed ``geom_feature[0]`` -- must still fill that
    operand tensor: the generator skips its own packing for it.  Both routes are split-f16 arithmetic, 5e-6 from fp32 on (0, 1) weights
    each, so they lie within 1e-5 of each other; the indexed provider takes the fresh one's route, bit for bit."""
    from brushstroke_engine_amd.networks import Generator
    cfg = cfgmod.style1_config(256)
    ops = painting.TileOps(Generator(cfg, wmod.random_state_dict(cfg, seed=0), conv_mode="h3").to("cuda"),
                           encmod.HipGeometryEncoder(encmod.random_encoder_state_dict(5)))
    geo = torch.ones([5, 1, 256, 256], device="cuda")
    for i in range(5):
        geo[i, 0, 40 + 30 * i:52 + 30 * i, 30:220] = 0
        geo[i, 0, 60:200, 100 + 10 * i:106 + 10 * i] = 0
    with torch.no_grad():
        ws = ops.map_style(z=torch.from_numpy(np.random.RandomState(0).randn(1, cfg.z_dim))).expand(5, -1, -1).contiguous()
        fresh = ops.triad_debug(ws, ops.encoder.lazy(geo))[1]["uvs"]
        used = ops.encoder.lazy(geo)
        assert used[0].shape[0] == 5                                        # computes and keeps the plain features
        indexed = ops.triad_debug(ws, used)[1]["uvs"]
        plain = ops.triad_debug(ws, ops.encoder.encode(geo))[1]["uvs"]
    assert torch.equal(indexed, fresh)
    assert float((plain - fresh).abs().max()) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# the mapper on the HIP engine
# ---------------------------------------------------------------------------------------------------------------------
def test_mapper_matches_reference(eng, single):
    g = eng["g"]
    for i, s in enumerate(single):
        np.testing.assert_allclose(s["sf"], float(g["sfactors"][i]), rtol=1e-4)
        assert s["colors"].shape == (1, 3, 3) and np.abs(s["colors"][0].astype(np.float64) - g["colors_raw"][i]).max() <= 1e-5
        bc.canvas_close(s["white"], g["icons_on_white"][i])
        bc.canvas_close(s["plain"], g["icons_plain"][i])
        assert np.abs(bc.spec_ints(s["spec"]) - bc.spec_ints(str(g["color_specs"][i]))).max() <= 1


def test_catalogue_against_single_calls(eng, single):
    mapper = eng["mapper"]
    with torch.no_grad():
        mapper.sfactors = {}
        full = mapper.catalogue(eng["lib"], batch=10)                      # two brushes per pass, two passes
        assert sorted(mapper.sfactors) == sorted(full.ids)
        small = mapper.catalogue(eng["lib"], batch=10, icon_k=4)
    assert full.icons.shape == (4, 128, 128, 3) and small.icons.shape == (4, 32, 32, 3)
    for i, s in enumerate(single):
        np.testing.assert_allclose(float(full.sfactors[i]), s["sf"], rtol=1e-4)
        np.testing.assert_allclose(float(full.sfactors[i]), float(eng["g"]["sfactors"][i]), rtol=1e-4)
        assert np.abs(full.colors_raw[i].astype(np.float64) - eng["g"]["colors_raw"][i]).max() <= 1e-5
        bc.canvas_close(full.icons[i], s["white"])
        bc.canvas_close(full.icons[i], eng["g"]["icons_on_white"][i])
        rgba = np.concatenate([full.icons[i], np.full((128, 128, 1), 255, np.uint8)], axis=2)
        assert np.array_equal(small.icons[i], painting.canvas_view_numpy(rgba, 0, 0, 128, 128, 4)[..., :3])
        assert full.color_specs[i] == mapper.color_spec(full.colors_raw[i:i + 1])


def test_session_main_with_uvs_calibration(eng, tmp_path):
    """Two brushes calibrated together before the first layer give the file of the same script painted with factors obtained one by one."""
    from PIL import Image
    from brushstroke_engine_amd import formats, paint_session_main
    snap, cal = str(tmp_path / "engine.npz"), str(tmp_path / "cal.npz")
    formats.save_engine_snapshot(snap, eng["cfg"], eng["sd"], eng["esd"], preproc_type=None)
    np.savez(cal, medium=eng["e"]["uvs_cal_medium"], thick=eng["e"]["uvs_cal_thick"])
    data = cr.good_script()
    data["layers"][1].update(mode="paint", opacity=255)
    script = tmp_path / "session.json"
    script.write_text(json.dumps(data))
    args = ["--gan_checkpoint", snap, "--script", str(script), "--conv_mode", "h3"]
    written = paint_session_main.main(args + ["--output_file_prefix", str(tmp_path / "cli" / "mapped"), "--uvs_calibration", cal])
    plain = paint_session_main.main(args + ["--output_file_prefix", str(tmp_path / "cli" / "plain")])
    parsed = paint_session_main.parse_script(json.dumps(data))
    mapper = painting.StyleUVSMapper(eng["ops"], eng["e"]["uvs_cal_medium"], eng["e"]["uvs_cal_thick"])
    libs = {}
    with torch.no_grad():
        for layer in parsed["layers"]:                                      # one by one; run_script then finds them in the cache
            mapper.get_sfactor(paint_session_main.layer_options(layer, libs, eng["cfg"].z_dim))
    assert sorted(mapper.sfactors) == ["12", "594"]
    calls = []
    mapper.calibrate = lambda *a, **k: calls.append(a)                      # (nothing left to calibrate)
    session = paint_session_main.run_script(painting.PaintingHelper(eng["ops"], uvs_mapper=mapper), parsed, eng["cfg"].z_dim)
    assert not calls
    mine = session.image(on_white=False)
    assert np.array_equal(np.array(Image.open(written)), mine)
    assert not np.array_equal(np.array(Image.open(plain)), mine)
    # a layer can opt out; without the flag it cannot opt in
    data["layers"][0]["uvs_mapping"] = True
    with pytest.raises(RuntimeError, match="--uvs_calibration"):
        paint_session_main.run_script(painting.PaintingHelper(eng["ops"]), paint_session_main.parse_script(data), eng["cfg"].z_dim)
