"""The generator through its C entry (``nb_generator_*`` of include/neube_hip.h): the path a C or C++ host takes, from Python.

``NativeGenerator`` owns one library-side generator handle: packed weights and workspaces for batches up to ``n_max`` on one
device.  ``render_triad`` is a thin ctypes call on the current torch stream that enqueues the whole step (mapping, styles, noise,
every layer, the fused ToRGB + compositing) as one chain of launches; its results equal ``Generator.render_triad``'s bit for bit
when the Python path runs as one chain too.  The Python ``Generator`` is not involved.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .config import GeneratorConfig, LayerSpec

_p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
_U64 = (1 << 64) - 1


def native_config(cfg: GeneratorConfig) -> "_lib.NbGeneratorConfig":
    """config.GeneratorConfig -> struct NbGeneratorConfig."""
    if cfg.c_dim != 0:
        raise ValueError("c_dim must be 0")
    if len(cfg.geom_feature_channels) > 4:
        raise ValueError("at most 4 geometry features")
    c = _lib.NbGeneratorConfig()
    c.z_dim, c.c_dim, c.w_dim, c.img_resolution = cfg.z_dim, cfg.c_dim, cfg.w_dim, cfg.img_resolution
    c.mapping_layers, c.mapping_lr_multiplier = cfg.mapping_layers, cfg.mapping_lr_multiplier
    c.channel_base, c.channel_max = cfg.channel_base, cfg.channel_max
    c.conv_clamp = -1.0 if cfg.conv_clamp is None else float(cfg.conv_clamp)
    c.num_geom = len(cfg.geom_feature_channels)
    for k, (ch, res) in enumerate(zip(cfg.geom_feature_channels, cfg.geom_feature_resolutions)):
        c.geom_channels[k], c.geom_resolutions[k] = ch, res
    return c


def param_table(cfg: GeneratorConfig) -> List[tuple]:
    """[(state-dict key, shape)] in the order nb_generator_create takes the parameters (weights.random_state_dict's)."""
    lib, c = _lib.lib(), native_config(cfg)
    count = lib.nb_generator_param_count(ctypes.byref(c))
    _lib.check(min(count, 0), "generator_param_count")
    out, name = [], ctypes.create_string_buffer(256)
    shape, ndim = (ctypes.c_int64 * 4)(), ctypes.c_int()
    for i in range(count):
        _lib.check(lib.nb_generator_param_info(ctypes.byref(c), i, name, 256, shape, ctypes.byref(ndim)), "generator_param_info")
        out.append((name.value.decode(), tuple(int(shape[k]) for k in range(ndim.value))))
    return out


def layer_table(cfg: GeneratorConfig):
    """([LayerSpec] in execution order, num_ws) as the library derives them from the configuration."""
    lib, c = _lib.lib(), native_config(cfg)
    num_ws = ctypes.c_int()
    count = lib.nb_generator_layer_count(ctypes.byref(c), ctypes.byref(num_ws))
    _lib.check(min(count, 0), "generator_layer_count")
    out, name, info = [], ctypes.create_string_buffer(256), _lib.NbGeneratorLayerInfo()
    for i in range(count):
        _lib.check(lib.nb_generator_layer_info(ctypes.byref(c), i, name, 256, ctypes.byref(info)), "generator_layer_info")
        out.append(LayerSpec(name.value.decode(), info.block_res, info.up, info.in_channels, info.out_channels, info.geom_channels,
                             info.w_index))
    return out, num_ws.value


def encoder_param_table() -> List[tuple]:
    """[(state-dict key, shape)] in the order nb_generator_attach_encoder takes the encoder parameters (encoder.ENCODER_STATE_SHAPES
    without num_batches_tracked)."""
    lib = _lib.lib()
    count = lib.nb_encoder_param_count()
    _lib.check(min(count, 0), "encoder_param_count")
    out, name = [], ctypes.create_string_buffer(256)
    shape, ndim = (ctypes.c_int64 * 4)(), ctypes.c_int()
    for i in range(count):
        _lib.check(lib.nb_encoder_param_info(i, name, 256, shape, ctypes.byref(ndim)), "encoder_param_info")
        out.append((name.value.decode(), tuple(int(shape[k]) for k in range(ndim.value))))
    return out


class NativeGenerator:
    """One ``NbGenerator`` handle.  Build it with :meth:`from_state_dict` or :meth:`from_generator`."""

    def __init__(self, cfg: GeneratorConfig, handle: int, conv_mode: str, n_max: int, device: torch.device):
        self.cfg, self._h, self.conv_mode, self.n_max, self.device = cfg, handle, conv_mode, n_max, device
        self.img_resolution, self.num_ws = cfg.img_resolution, cfg.num_ws

    @staticmethod
    def from_state_dict(cfg: GeneratorConfig, sd, conv_mode: str = "f8", n_max: int = 32, device="cuda") -> "NativeGenerator":
        """sd: state dict (numpy arrays or tensors, the reference's key names).  The parameters are uploaded, handed to
        nb_generator_create (which copies and packs them) and released."""
        if conv_mode not in _lib.NB_CONV_MODES:
            raise ValueError(f"unknown conv_mode {conv_mode!r}")
        if tuple(cfg.resample_filter) != (1, 3, 3, 1):
            raise ValueError("the C entry takes the [1, 3, 3, 1] resample filter of the shipped configuration")
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        table = param_table(cfg)
        tensors = []
        for name, shape in table:
            v = sd[name]
            t = v if torch.is_tensor(v) else torch.from_numpy(np.array(v, dtype=np.float32))     # (0-dim stays 0-dim)
            t = t.detach().to(device=device, dtype=torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
            tensors.append(t)
        ptrs = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        c = native_config(cfg)
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            _lib.check(_lib.lib().nb_generator_create(ctypes.byref(c), ptrs, _lib.NB_CONV_MODES[conv_mode], n_max, stream,
                                                      ctypes.byref(h)), "generator_create")
        return NativeGenerator(cfg, h.value, conv_mode, n_max, device)

    @staticmethod
    def from_generator(G, n_max: int = 32) -> "NativeGenerator":
        """The weights and arithmetic mode of a networks.Generator."""
        dev = G.synthesis.get_last_block().conv1.weight.device
        return NativeGenerator.from_state_dict(G.cfg, G.state_dict(), G.synthesis.conv_mode, n_max, dev)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().nb_generator_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:                    # noqa: BLE001  (interpreter shutdown)
            pass

    def describe(self, n: int, stop_res: int = 0, resume_res: int = 0) -> dict:
        """{layer name: kernel} the forward at batch n launches (the strings SynthesisNetwork.layer_kernels records; the ToRGB's
        entry is the last conv's kernel when fused into it).  ``stop_res`` / ``resume_res``: the layers of that staged pass
        (:meth:`head` / :meth:`tail`) instead of the whole pass."""
        buf = ctypes.create_string_buffer(8192)
        if stop_res or resume_res:
            _lib.check(_lib.lib().nb_generator_describe_staged(self._h, n, stop_res, resume_res, buf, len(buf)), "generator_describe_staged")
        else:
            _lib.check(_lib.lib().nb_generator_describe(self._h, n, buf, len(buf)), "generator_describe")
        return dict(line.split("=", 1) for line in buf.value.decode().splitlines())

    def attach_encoder(self, encoder_state_dict, preproc_type=None):
        """Attach the geometry encoder (encoder.HipGeometryEncoder's weights and preproc_type strings): the forward then also takes
        stroke patches (``geom=``).  The parameters are uploaded, folded and packed by the library and released."""
        if preproc_type not in _lib.NB_GEOM_PREPROC:
            raise RuntimeError(f'Unknown preprocessing type "{preproc_type}"')
        tensors = []
        for name, shape in encoder_param_table():
            v = encoder_state_dict[name]
            t = v if torch.is_tensor(v) else torch.from_numpy(np.array(v, dtype=np.float32))
            t = t.detach().to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
            tensors.append(t)
        ptrs = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(_lib.lib().nb_generator_attach_encoder(self._h, ptrs, _lib.NB_GEOM_PREPROC[preproc_type], stream),
                       "generator_attach_encoder")

    # ---- brush noise sets (a projected brush's noise buffers; include/neube_hip.h) ----
    def brush_noise(self) -> "NativeBrushNoise":
        """A new set of this handle (nb_brush_noise_create), holding the checkpoint's noise until its ``load``."""
        return NativeBrushNoise(self)

    def bind_brush_noise(self, bn: Optional["NativeBrushNoise"]) -> None:
        """Every later constant-noise forward of the handle reads ``bn`` (None: the checkpoint's noise again).  Host state only."""
        _lib.check(_lib.lib().nb_generator_bind_brush_noise(self._h, None if bn is None else bn._h), "generator_bind_brush_noise")

    # ---- forward ----
    def _f32(self, t, shape, name):
        t = torch.as_tensor(t, device=self.device).to(torch.float32).contiguous()
        if list(t.shape) != list(shape):
            raise ValueError(f"{name}: expected shape {list(shape)}, got {list(t.shape)}")
        return t

    def forward_into(self, outputs: dict, n: int, z=None, ws=None, geom_feature: Sequence = (), positions=None, noise_mode="const",
                     render_mode="clear", user_colors=None, sfactor=None, truncation_psi=1.0, truncation_cutoff=None, geom=None,
                     stage=None, noise_seed=0, noise_offset=0, noise_state=None):
        """Enqueue one forward on the current stream into caller-allocated ``outputs`` (keys rgba_u8 / rgba / img / uvs / colors;
        missing = not wanted).  Inputs must already be device tensors of the right dtype and shape (nothing is converted here):
        the form for graph capture.  ``geom``: stroke patches [n, 1, R, R] fp32 for the attached encoder, instead of
        ``geom_feature``.  ``stage``: an ``_lib.NbGeneratorStage`` for one half of a split pass
        (nb_generator_forward_staged; :meth:`head` / :meth:`tail` build it).  ``noise_mode="seeded"``: sample k draws the noise of
        (``noise_seed``, ``noise_offset`` + k), or of the two values in ``noise_state`` (int64[2] device tensor) when given."""
        if geom is not None and len(geom_feature):
            raise ValueError("pass either geom (stroke patches) or geom_feature, not both")
        ins = _lib.NbGeneratorInputs()
        ins.z, ins.ws = _p(z), _p(ws)
        ins.truncation_psi = float(truncation_psi)
        ins.truncation_cutoff = -1 if truncation_cutoff is None else int(truncation_cutoff)
        for k, g in enumerate(geom_feature):
            ins.geom[k] = _p(g)
        ins.positions = _p(positions)
        ins.noise_mode = _lib.NB_NOISE_MODES[noise_mode] if isinstance(noise_mode, str) else int(noise_mode)
        if render_mode not in _lib.NB_RENDER_MODES:
            raise RuntimeError(f"Unknown render mode for TriadGanPaintEngine: {render_mode}")
        ins.render_mode = _lib.NB_RENDER_MODES[render_mode]
        ins.user_colors, ins.sfactor = _p(user_colors), _p(sfactor)
        ins.noise_seed, ins.noise_offset = int(noise_seed) & _U64, int(noise_offset) & _U64
        ins.noise_state = _p(noise_state)
        outs = _lib.NbGeneratorOutputs()
        for k in ("rgba_u8", "rgba", "img", "uvs", "colors"):
            setattr(outs, k, _p(outputs.get(k)))
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            if stage is not None:
                _lib.check(_lib.lib().nb_generator_forward_staged(self._h, ctypes.byref(ins), _p(geom), ctypes.byref(stage), ctypes.byref(outs),
                                                                  n, stream), "generator_forward_staged")
            elif geom is None:
                _lib.check(_lib.lib().nb_generator_forward(self._h, ctypes.byref(ins), ctypes.byref(outs), n, stream), "generator_forward")
            else:
                _lib.check(_lib.lib().nb_generator_forward_geom(self._h, ctypes.byref(ins), _p(geom), ctypes.byref(outs), n, stream),
                           "generator_forward_geom")

    def render_triad(self, z=None, ws=None, geom_feature=None, positions=None, render_mode="clear", user_colors=None, want_u8=True,
                     want_f32=False, sfactor=None, noise_mode="const", truncation_psi=1.0, truncation_cutoff=None, geom=None,
                     noise_seed=0, noise_offset=0, noise_state=None):
        """Generator.render_triad through the C entry: (rgba_u8 [N,R,R,4] | None, rgba [N,4,R,R] | None, {uvs, colors, img}).
        ``geom``: stroke patches [N, 1, R, R] (1 = background) for the attached encoder (:meth:`attach_encoder`), instead of the
        encoded ``geom_feature``."""
        cfg, dev = self.cfg, self.device
        if (z is None) == (ws is None):
            raise ValueError("pass exactly one of z / ws")
        n = (z if z is not None else ws).shape[0]
        z = None if z is None else self._f32(z, [n, cfg.z_dim], "z")
        ws = None if ws is None else self._f32(ws, [n, cfg.num_ws, cfg.w_dim], "ws")
        patches = None
        if geom is not None:
            if geom_feature is not None:
                raise ValueError("pass either geom (stroke patches) or geom_feature, not both")
            patches = self._f32(geom, [n, 1, cfg.img_resolution, cfg.img_resolution], "geom")
            geom = []
        else:
            geom_feature = list(geom_feature) if isinstance(geom_feature, (list, tuple)) else [geom_feature]
            if len(geom_feature) != len(cfg.geom_feature_channels):
                raise ValueError(f"expected {len(cfg.geom_feature_channels)} geometry features, got {len(geom_feature)}")
            geom = [self._f32(g, [n, c, r, r], f"geom_feature[{k}]")
                    for k, (g, c, r) in enumerate(zip(geom_feature, cfg.geom_feature_channels, cfg.geom_feature_resolutions))]
        pos = None
        if positions is not None:
            pos = torch.as_tensor(positions, device=dev).to(torch.int64).contiguous()
            if list(pos.shape) != [n, 2]:
                raise ValueError(f"positions: expected shape [{n}, 2], got {list(pos.shape)}")
        user = None if user_colors is None else self._f32(user_colors, [n, 3, 3], "user_colors")
        sfac = None
        if sfactor is not None:
            sfac = torch.as_tensor(sfactor, dtype=torch.float32, device=dev).reshape(-1)
            sfac = self._f32(sfac.expand(n) if sfac.numel() == 1 else sfac, [n], "sfactor")
        r = cfg.img_resolution
        outs = {"uvs": torch.empty([n, 3, r, r], dtype=torch.float32, device=dev),
                "img": torch.empty([n, 3, r, r], dtype=torch.float32, device=dev),
                "colors": torch.empty([n, 3, 3], dtype=torch.float32, device=dev)}
        if want_u8:
            outs["rgba_u8"] = torch.empty([n, r, r, 4], dtype=torch.uint8, device=dev)
        if want_f32:
            outs["rgba"] = torch.empty([n, 4, r, r], dtype=torch.float32, device=dev)
        self.forward_into(outs, n, z=z, ws=ws, geom_feature=geom, positions=pos, noise_mode=noise_mode, render_mode=render_mode,
                          user_colors=user, sfactor=sfac, truncation_psi=truncation_psi, truncation_cutoff=truncation_cutoff, geom=patches,
                          noise_seed=noise_seed, noise_offset=noise_offset, noise_state=noise_state)
        # the inputs converted here are read by work enqueued on the current stream: keep them alive for it
        cur = torch.cuda.current_stream(dev)
        for t in [z, ws, pos, user, sfac, patches] + geom:
            if t is not None:
                t.record_stream(cur)
        return outs.get("rgba_u8"), outs.get("rgba"), {"uvs": outs["uvs"], "colors": outs["colors"], "img": outs["img"]}

    # ---- staged passes: the generator split around the feature-canvas blend (painting.PaintingHelper._schedule) ----
    def head(self, n: int, stop_res: int, features_out, z=None, ws=None, geom_feature: Sequence = (), geom=None, positions=None,
             noise_mode="const", truncation_psi=1.0, truncation_cutoff=None, noise_seed=0, noise_offset=0, noise_state=None):
        """Enqueue the pass up to block ``stop_res`` (``forward_pre_mapped(_stop_after=stop_res)``): the block's fp32 output, before
        blending, goes into ``features_out`` [n, channels(stop_res), stop_res, stop_res].  Device tensors of the right dtype and
        shape, as :meth:`forward_into` takes them."""
        stage = _lib.NbGeneratorStage(int(stop_res), 0, _p(features_out), None)
        self.forward_into({}, n, z=z, ws=ws, geom_feature=geom_feature, positions=positions, noise_mode=noise_mode,
                          truncation_psi=truncation_psi, truncation_cutoff=truncation_cutoff, geom=geom, stage=stage,
                          noise_seed=noise_seed, noise_offset=noise_offset, noise_state=noise_state)
        return features_out

    def tail(self, n: int, resume_res: int, features_in, outputs: dict, z=None, ws=None, geom_feature: Sequence = (), geom=None,
             positions=None, noise_mode="const", render_mode="clear", user_colors=None, sfactor=None, truncation_psi=1.0,
             truncation_cutoff=None, noise_seed=0, noise_offset=0, noise_state=None):
        """Enqueue the pass behind block ``resume_res`` (``render_triad(_resume=(resume_res, features_in))``) into the caller's
        ``outputs`` (keys as :meth:`forward_into`).  Only the geometry features at resolutions >= ``resume_res`` are read
        (``geom_feature`` entries below may be None)."""
        stage = _lib.NbGeneratorStage(0, int(resume_res), None, _p(features_in))
        self.forward_into(outputs, n, z=z, ws=ws, geom_feature=geom_feature, positions=positions, noise_mode=noise_mode,
                          render_mode=render_mode, user_colors=user_colors, sfactor=sfactor, truncation_psi=truncation_psi,
                          truncation_cutoff=truncation_cutoff, geom=geom, stage=stage, noise_seed=noise_seed,
                          noise_offset=noise_offset, noise_state=noise_state)
        return outputs


def pack_weights_dev(weight: torch.Tensor, kind: str, resample_filter: Optional[torch.Tensor] = None):
    """The device packers on their own (tests, tools): kind 'wpk' -> (wpk, wsq), 'f8' -> the f8 format, 'h3_up2' -> the four phase
    kernels, 'h3' -> nb_pack_conv_weight_h3_dev with co_align 64."""
    lib = _lib.lib()
    o, i = weight.shape[:2]
    w = weight.detach().to(torch.float32).contiguous()
    dev = w.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    nch, op64 = (i + 15) // 16, (o + 63) // 64 * 64
    with torch.cuda.device(dev):
        if kind == "wpk":
            wpk = torch.empty([(i + 7) // 8 * 8, 9, (o + 31) // 32 * 32], dtype=torch.float32, device=dev)
            wsq = torch.empty([i, o], dtype=torch.float32, device=dev)
            _lib.check(lib.nb_pack_conv_weight_dev(_p(w), o, i, _p(wpk), _p(wsq), stream), "pack_conv_weight_dev")
            return wpk, wsq
        if kind == "h3":
            out = torch.empty([nch, 3, 3, 2, 2, op64, 8], dtype=torch.float16, device=dev)
            _lib.check(lib.nb_pack_conv_weight_h3_dev(_p(w), o, i, 64, 0, _p(out), stream), "pack_conv_weight_h3_dev")
            return out
        if kind == "f8":
            out = torch.empty([nch, 3, 3, 2, 2, op64, 8], dtype=torch.float16, device=dev)
            _lib.check(lib.nb_pack_conv_weight_h3f8_dev(_p(w), o, i, _p(out), stream), "pack_conv_weight_h3f8_dev")
            return out
        if kind == "h3_up2":
            f = resample_filter.detach().to(device=dev, dtype=torch.float32).contiguous()
            out = torch.empty([4, nch, 3, 3, 2, 2, op64, 8], dtype=torch.float16, device=dev)
            _lib.check(lib.nb_pack_conv_weight_h3_up2_dev(_p(w), _p(f), o, i, _p(out), stream), "pack_conv_weight_h3_up2_dev")
            return out
    raise ValueError(f"unknown kind {kind!r}")


class NativeBrushNoise:
    """One ``NbBrushNoise`` handle (``NativeGenerator.brush_noise()``): a projected brush's noise buffers on the device, for the C
    generator.  ``load`` takes the reference's ``noise_buffers`` dicts like ``networks.BrushNoise.load``; close it before its
    generator."""

    def __init__(self, gen: NativeGenerator):
        self.gen = gen
        h = ctypes.c_void_p()
        with torch.cuda.device(gen.device):
            _lib.check(_lib.lib().nb_brush_noise_create(gen._h, torch.cuda.current_stream(gen.device).cuda_stream, ctypes.byref(h)),
                       "brush_noise_create")
        self._h = h.value

    def _pointers(self, buffers, keep):
        ptrs = (ctypes.c_void_p * len(self.gen.cfg.layers))()
        for i, s in enumerate(self.gen.cfg.layers):
            buf = None if not buffers else buffers.get(f"b{s.block_res}.conv{0 if s.up == 2 else 1}.noise_const")
            if buf is not None:
                buf = self.gen._f32(buf if torch.is_tensor(buf) else np.asarray(buf), [s.block_res, s.block_res], s.name + ".noise_const")
                keep.append(buf)
                ptrs[i] = buf.data_ptr()
        return ptrs

    def load(self, noise_buffers, other=None, alpha: float = 1.0) -> "NativeBrushNoise":
        """nb_brush_noise_load on the current stream: missing keys / None values = the checkpoint's buffer; with ``other`` the set
        becomes ``noise_buffers * alpha + other * (1 - alpha)`` (alpha as a C float)."""
        keep = []
        a = self._pointers(noise_buffers, keep)
        b = None if other is None else self._pointers(other, keep)
        with torch.cuda.device(self.gen.device):
            _lib.check(_lib.lib().nb_brush_noise_load(self._h, a, b, alpha, torch.cuda.current_stream(self.gen.device).cuda_stream),
                       "brush_noise_load")
        return self

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().nb_brush_noise_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:                    # noqa: BLE001  (interpreter shutdown)
            pass
