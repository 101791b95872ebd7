"""Golden vectors for tests/test_formats.py: the REFERENCE's websocket protocol functions (forger/ui/util.py) on seeded
messages, and the snapshot interface that tools/convert_snapshot.py reads from a reference generator (its attributes and its
state-dict key names and shapes, style1 shapes at R=128).  Needs the reference source tree; the fixture is data only and the
tests that read it never touch the reference.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_formats.py --reference /path/to/brushstroke_engine
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def request(w, h, x, y, m, rs):
    """The render request of tests/test_formats.py::_request."""
    stroke = rs.randint(0, 256, (h, w, 4)).astype(np.uint8)
    return np.array([w, h, x, y, m], np.int32).tobytes() + stroke.tobytes() + stroke[::-1].tobytes(), stroke


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference source tree")
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    # import stubs for packages the build environment lacks (nothing of them is exercised by the functions used here)
    for name in ("tornado", "tornado.websocket", "tornado.web", "tornado.gen", "skimage", "skimage.io", "skimage.filters",
                 "torchvision"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
    sys.modules["tornado.websocket"].WebSocketHandler = object
    sys.modules["tornado"].gen = sys.modules["tornado.gen"]
    sys.modules["tornado.gen"].coroutine = lambda f: f
    sys.modules["skimage.io"].imread = sys.modules["skimage.io"].imsave = None
    sys.modules["skimage.filters"].threshold_otsu = sys.modules["skimage.filters"].threshold_local = None
    import matplotlib
    matplotlib.use("Agg")
    import thirdparty.stylegan2_ada_pytorch  # noqa: F401
    import thirdparty.stylegan2_ada_pytorch.dnnlib as dnnlib
    from thirdparty.stylegan2_ada_pytorch.training.networks_modified import Generator
    import forger.ui.util as ref
    from brushstroke_engine_amd import config as cfgmod, weights as wmod

    out = {}
    # protocol: a 16x16 request, a patch reply, render-request metadata
    msg, stroke = request(16, 16, 3, 4, 2, np.random.RandomState(1))
    meta, img = ref.binary_to_image_patches(msg)[:2]
    out["proto_msg"] = np.frombuffer(msg, np.uint8)
    out["proto_meta_keys"] = np.array(list(meta.keys()))
    out["proto_meta_values"] = np.array([int(v) for v in meta.values()], np.int64)
    out["proto_img"] = np.asarray(img)
    out["proto_patch_binary"] = np.frombuffer(ref.image_patch_to_binary(stroke, 7, 8), np.uint8)
    head = bytes([0, 1, 3, 2, 9, 8, 7])
    dmeta, off = ref.decode_render_request_metadata(head)
    out["proto_head"] = np.frombuffer(head, np.uint8)
    out["proto_head_offset"] = np.int64(off)
    out["proto_head_color0"] = np.array(list(dmeta["colors"][0]), np.int64)

    # snapshot interface: the reference generator the converter test pickles, built with this build's style1 shapes at R=128
    cfg = cfgmod.style1_config(128)
    sd = wmod.random_state_dict(cfg, seed=0)
    G = Generator(z_dim=64, c_dim=0, w_dim=64, img_resolution=128, img_channels=3, mapping_kwargs=dnnlib.EasyDict(num_layers=4),
                  synthesis_kwargs=dnnlib.EasyDict(channel_base=16384, channel_max=128, num_fp16_res=0, conv_clamp=256, architecture="orig",
                                                   color_format="triad", color_w_channels=0, enable_geom_linear=False,
                                                   geom_feature_channels=[16, 256], geom_feature_resolutions=[16, 32])).eval()
    G.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    gsd = G.state_dict()
    syn = G.synthesis
    out["snap_keys"] = np.array(list(gsd.keys()))
    out["snap_shapes"] = np.array([list(v.shape) + [-1] * (4 - v.dim()) for v in gsd.values()], np.int64)
    out["snap_dims"] = np.array([G.z_dim, G.w_dim, G.img_resolution], np.int64)
    out["snap_block_resolutions"] = np.array(syn.block_resolutions, np.int64)
    out["snap_conv_clamp"] = np.float64(getattr(syn, f"b{G.img_resolution}").conv1.conv_clamp)
    out["snap_geom_feature_channels"] = np.array(syn.geom_feature_channels, np.int64)
    out["snap_geom_feature_resolutions"] = np.array(syn.geom_feature_resolutions, np.int64)
    np.savez_compressed(os.path.join(HERE, "formats_ref.npz"), **out)
    print("wrote", os.path.join(HERE, "formats_ref.npz"), {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
