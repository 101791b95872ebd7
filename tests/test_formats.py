"""Formats row: websocket binary protocol, brush libraries, engine snapshot container.  The cross-checks
against the reference read what its own functions and generator produced (tests/golden/formats_ref.npz, made by
tests/golden/make_golden_formats.py); no test here needs the reference tree."""
import argparse
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden
from brushstroke_engine_amd import config as cfgmod, encoder as encmod, formats, painting, weights as wmod


def _request(w, h, x, y, m, rs):
    stroke = rs.randint(0, 256, (h, w, 4)).astype(np.uint8)
    return np.array([w, h, x, y, m], np.int32).tobytes() + stroke.tobytes() + stroke[::-1].tobytes(), stroke


def test_protocol_roundtrip():
    rs = np.random.RandomState(0)
    msg, stroke = _request(8, 6, 120, -4, 10, rs)
    head = bytes([1, 2, 7]) + bytes([0, 255, 0, 0]) + bytes([1, 0, 128, 255])
    meta, off = formats.decode_render_request_metadata(head + msg)
    assert meta["debug"] is True and meta["extra_data"] == 7 and off == 11
    assert [list(c) for c in meta["colors"]] == [[0, 255, 0, 0], [1, 0, 128, 255]]
    m, img, canvas = formats.binary_to_image_patches(head + msg, offset=off)
    assert m == {"width": 8, "height": 6, "x": 120, "y": -4, "crop_margin": 10} and canvas is None
    assert np.array_equal(img, stroke)
    out = formats.image_patch_to_binary(stroke, 5, 9)
    assert list(np.frombuffer(out, np.int32, 4)) == [8, 6, 5, 9] and out[16:] == stroke.tobytes()
    assert formats.int32_to_binary(-3) == np.array([-3], np.int32).tobytes()
    with pytest.raises(RuntimeError):
        formats.image_patch_to_binary(stroke.astype(np.float32), 0, 0)
    with pytest.raises(ValueError):
        formats.binary_to_image_patches(msg[:40])


def test_protocol_matches_reference():
    """The three protocol functions against the reference's (forger/ui/util.py) on the same messages."""
    g = load_golden("formats_ref.npz")
    msg, stroke = _request(16, 16, 3, 4, 2, np.random.RandomState(1))
    assert msg == g["proto_msg"].tobytes()                    # the message the reference decoded
    meta, img = formats.binary_to_image_patches(msg)[:2]
    assert meta == dict(zip(g["proto_meta_keys"].tolist(), g["proto_meta_values"].tolist())) and np.array_equal(img, g["proto_img"])
    assert formats.image_patch_to_binary(stroke, 7, 8) == g["proto_patch_binary"].tobytes()
    meta, off = formats.decode_render_request_metadata(g["proto_head"].tobytes())
    assert off == int(g["proto_head_offset"]) and list(meta["colors"][0]) == g["proto_head_color0"].tolist()


def test_seed_and_w_libraries(tmp_path):
    f = tmp_path / "seeds.txt"
    f.write_text("# my brushes\n594 0.1 0.2\n\n12\nbroken line\n7 1 2 3\n")
    zs, zdim = formats.read_zs(str(f))
    assert zs == [594, 12, 7] and zdim == 3
    lib = formats.BrushLibrary.from_arg(str(f), z_dim=64)
    assert isinstance(lib, formats.SeedBrushLibrary) and lib.get_style_ids() == ["12", "594", "7"]
    opts = painting.GanBrushOptions()
    lib.set_style("594", opts)
    assert opts.style_id == "594" and opts.style_ws is None
    assert np.array_equal(opts.style_z.numpy(), np.random.RandomState(594).randn(1, 64))
    rl = formats.BrushLibrary.from_arg("rand5", 64)
    assert rl.get_style_ids() == ["rand0", "rand1", "rand2", "rand3", "rand4"]
    rl.set_style("rand3", opts)
    g = torch.Generator(); g.manual_seed(1)
    assert torch.equal(opts.style_z, torch.rand((1, 64), generator=g)) and opts.style_id is None
    assert formats.BrushLibrary.from_arg("3,1,2").get_style_ids() == ["1", "2", "3"]
    assert len(formats.BrushLibrary.from_arg("4").zs) == 4
    lib.set_interpolated_style("594", "7", 0.25, opts)
    assert opts.style_id == "594_0.25__7"
    # W library: bare ws, {'w', 'noise'}, and the legacy flat dict
    ws = lambda s: torch.from_numpy(np.random.RandomState(s).randn(1, 14, 64).astype(np.float32))
    noise = lambda s: {"b8.conv0.noise_const": np.random.RandomState(s).randn(8, 8).astype(np.float32)}
    styles = {"a": ws(1), "b": {"w": ws(2), "noise": noise(2)}, "c": dict(w=ws(3), **noise(3))}
    wf = tmp_path / "proj.pkl"
    wf.write_bytes(pickle.dumps(styles))
    wl = formats.BrushLibrary.from_file(str(wf))
    assert isinstance(wl, formats.WBrushLibrary) and wl.get_style_ids() == ["a", "b", "c"]
    wl.set_style("a", opts)
    assert opts.style_z is None and torch.equal(opts.style_ws, styles["a"]) and opts.custom_args == {"noise_buffers": None}
    wl.set_style("c", opts)
    assert torch.is_tensor(opts.custom_args["noise_buffers"]["b8.conv0.noise_const"])
    wl.set_interpolated_style("b", "c", 0.5, opts)
    want = 0.5 * noise(2)["b8.conv0.noise_const"] + 0.5 * noise(3)["b8.conv0.noise_const"]
    np.testing.assert_allclose(opts.custom_args["noise_buffers"]["b8.conv0.noise_const"].numpy(), want, rtol=1e-6)
    np.testing.assert_allclose(opts.style_ws.numpy(), (0.5 * ws(2) + 0.5 * ws(3)).numpy(), rtol=1e-6)


def test_engine_snapshot_roundtrip(tmp_path):
    cfg = cfgmod.tiny_config(32)
    sd = wmod.random_state_dict(cfg, seed=3)
    esd = encmod.random_encoder_state_dict(4)
    p = str(tmp_path / "engine.npz")
    formats.save_engine_snapshot(p, cfg, sd, esd, preproc_type="-11inverse", extra={"color_format": "triad"})
    cfg2, sd2, esd2, pre, extra = formats.load_engine_snapshot(p)
    assert cfg2 == cfg and pre == "-11inverse" and extra == {"color_format": "triad"}
    assert sd.keys() == sd2.keys() and all(np.array_equal(sd[k], sd2[k]) for k in sd)
    assert esd.keys() == esd2.keys() and all(np.array_equal(esd[k], esd2[k]) for k in esd)
    wmod.validate_state_dict(cfg2, sd2)


# A stand-in for the two reference modules tools/convert_snapshot.py opens a snapshot with: the network pickle becomes the object
# graph the converter reads (generator attributes, blocks' conv1, state_dict(), encoder, args), built from plain data.
STUB_FILES = {
    "thirdparty/__init__.py": "",
    "thirdparty/stylegan2_ada_pytorch/__init__.py": "",
    "thirdparty/stylegan2_ada_pytorch/dnnlib/__init__.py": "from . import util\n",
    "thirdparty/stylegan2_ada_pytorch/dnnlib/util.py": "def open_url(url):\n    return open(url, 'rb')\n",
    "thirdparty/stylegan2_ada_pytorch/legacy.py": '''
import pickle
from types import SimpleNamespace as NS


def load_network_pkl(f):
    d = pickle.load(f)
    g, sd = d["G_ema"], d["G_ema"]["state_dict"]
    blocks = {f"b{r}": NS(conv1=NS(weight=sd[f"synthesis.b{r}.conv1.weight"], conv_clamp=g["conv_clamp"])) for r in g["block_resolutions"]}
    syn = NS(block_resolutions=g["block_resolutions"], geom_feature_channels=g["geom_feature_channels"],
             geom_feature_resolutions=g["geom_feature_resolutions"], **blocks)
    return dict(d, G_ema=NS(z_dim=g["z_dim"], w_dim=g["w_dim"], img_resolution=g["img_resolution"], synthesis=syn, state_dict=lambda: dict(sd)))
''',
}


def test_convert_reference_snapshot(tmp_path):
    """tools/convert_snapshot.py on a snapshot of a reference generator: its key names, shapes and attributes are those of the
    reference's Generator (style1 shapes, R=128) that loaded this build's state dict strictly (tests/golden/formats_ref.npz)."""
    g = load_golden("formats_ref.npz")
    cfg = cfgmod.style1_config(128)
    sd = wmod.random_state_dict(cfg, seed=0)
    keys = g["snap_keys"].tolist()
    assert sorted(keys) == sorted(sd.keys())
    for k, shape in zip(keys, g["snap_shapes"].tolist()):
        assert list(np.shape(sd[k])) == [d for d in shape if d >= 0], k
    ref = tmp_path / "reference"
    for name, text in STUB_FILES.items():
        (ref / name).parent.mkdir(parents=True, exist_ok=True)
        (ref / name).write_text(text)
    z_dim, w_dim, res = g["snap_dims"].tolist()
    snap = {"G_ema": dict(z_dim=z_dim, w_dim=w_dim, img_resolution=res, block_resolutions=g["snap_block_resolutions"].tolist(),
                          conv_clamp=int(g["snap_conv_clamp"]), geom_feature_channels=g["snap_geom_feature_channels"].tolist(),
                          geom_feature_resolutions=g["snap_geom_feature_resolutions"].tolist(),
                          state_dict={k: torch.from_numpy(np.asarray(sd[k])) for k in keys}),
            "args": argparse.Namespace(color_format="triad", geom_inject_resolutions=[0, 1]),
            "encoder": {"args": argparse.Namespace(preproc_type="inverse"),
                        "model_state": {k: torch.from_numpy(v) for k, v in encmod.random_encoder_state_dict(5).items()}}}
    with open(tmp_path / "snap.pkl", "wb") as f:
        pickle.dump(snap, f)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    out = str(tmp_path / "engine.npz")
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "convert_snapshot.py"), "--reference", str(ref),
                           "--pkl", str(tmp_path / "snap.pkl"), "--out", out], env=env, stdout=subprocess.DEVNULL)
    cfg, sd, esd, pre, extra = formats.load_engine_snapshot(out)
    assert cfg == cfgmod.style1_config(128) and pre == "inverse" and extra["geom_inject_resolutions"] == [0, 1]
    want = wmod.random_state_dict(cfg, seed=0)
    assert want.keys() == sd.keys() and all(np.array_equal(np.asarray(want[k]), sd[k]) for k in want)
    assert all(np.array_equal(encmod.random_encoder_state_dict(5)[k], esd[k]) for k in esd)
