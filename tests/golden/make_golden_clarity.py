"""Golden vectors for brushstroke_engine_amd.clarity: the REFERENCE's ``run_one_clarity_opt`` (scripts/opt_clarity_main.py) driven on
the CPU for 8 steps, ``w_plus=True``, with the default loss without its perceptual item.  Build container only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_clarity.py

The engine handed to the reference is a stand-in: ``G.synthesis`` is a small torch module around ``oracle.OracleGenerator``
(``tiny_config(32)``, float32) whose ``noise_const`` buffers are registered under the reference's names, ``encoder.encode`` is
``clarity_refs.StandInEncoder``, the geometry iterator deals fixed batches of line drawings.  Modules the reference imports for its
visualisations and data sets, and which this container does not have, are stubbed; ``make_viz`` and ``imsave`` are no-ops.

Recorded: the inputs, the random draws (initial noise planes, the W noise of each step: the global generator is seeded and its draws
are replayed here in the reference's order), per step lr / loss items / regulariser, the final w and noise planes, ``get_w_stats`` of
the stand-in's mapping and the schedule, and eps_ref = the largest deviation of those float32 results from the float64 statement
(tests/clarity_refs.py) driven with the same draws.
"""
import importlib.abc
import importlib.machinery
import importlib.util
import logging
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = "/root/reference"
sys.dont_write_bytecode = True
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), REFERENCE]

STUB_ROOTS = ("imageio", "torchvision", "skimage", "lpips", "pyspng")
NUM_STEPS, BATCH, SEED, Z_SEED = 8, 4, 77, 42
LOSSES = "0.5*iou_inv(uvs)+0.5*iou(u)+50*l1(fake_orig)"


class _Anything:
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return None

    def __getattr__(self, n):
        return _Anything()


class _StubModule(types.ModuleType):
    def __getattr__(self, n):
        if n.startswith("__"):
            raise AttributeError(n)
        return _Anything


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """Behind the real finders: only modules that are missing here are replaced."""

    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] in STUB_ROOTS:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        m = _StubModule(spec.name)
        m.__path__ = []
        return m

    def exec_module(self, module):
        pass


def load_reference_script():
    sys.meta_path.append(_StubFinder())
    spec = importlib.util.spec_from_file_location("opt_clarity_main", os.path.join(REFERENCE, "scripts", "opt_clarity_main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.make_viz = lambda *a, **k: None
    mod.imsave = lambda *a, **k: None
    return mod


def main():
    import clarity_refs as cr
    from brushstroke_engine_amd import clarity, config as cfgmod, weights as wmod
    ref = load_reference_script()
    import forger.train.losses as ref_losses
    import thirdparty.stylegan2_ada_pytorch.experiment.util.latent as ref_latent
    logging.disable(logging.CRITICAL)

    cfg = cfgmod.tiny_config(32)
    sd = wmod.random_state_dict(cfg, seed=3)
    lo = clarity.ArenaLayout.from_config(cfg)
    gen32 = cr.OracleGen(cfg, sd, torch.float32)
    enc = cr.StandInEncoder(cfg)
    drawings = cr.line_drawings(cfg.img_resolution, 12, seed=5)
    idx = np.stack([(np.arange(BATCH) + BATCH * s) % len(drawings) for s in range(NUM_STEPS)])

    class Synthesis(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for name in lo.names:                                         # 'b4.conv1.noise_const' -> attribute 'b4' . 'conv1' . 'noise_const'
                blk, conv, leaf = name.split(".")
                if not hasattr(self, blk):
                    setattr(self, blk, torch.nn.Module())
                if not hasattr(getattr(self, blk), conv):
                    setattr(getattr(self, blk), conv, torch.nn.Module())
                getattr(getattr(self, blk), conv).register_buffer(leaf, torch.from_numpy(np.asarray(sd["synthesis." + name], np.float32)).clone())

        def forward(self, ws, geom_feature=None, noise_mode="const", return_debug_data=False):
            bufs = dict(self.named_buffers())
            return gen32.synthesis(ws, geom_feature, noise_mode=noise_mode, noise_buffers={n: bufs[n] for n in lo.names},
                                   return_debug_data=return_debug_data)

    class Mapping:
        num_ws = cfg.num_ws

        def __call__(self, z, c=None):
            return gen32.mapping(z, c)

    G = types.SimpleNamespace(synthesis=Synthesis(), mapping=Mapping(), z_dim=cfg.z_dim, img_resolution=cfg.img_resolution)
    Engine = types.SimpleNamespace(G=G, encoder=enc, device=torch.device("cpu"))

    assert [n for n, _ in G.synthesis.named_buffers()] == lo.names

    def geom_iterator():
        for s in range(NUM_STEPS):
            g = torch.from_numpy(drawings[idx[s]])[:, None].expand(-1, 3, -1, -1).contiguous()
            yield g, None

    w_avg, w_std = ref_latent.get_w_stats(num_samples=500, z_dim=cfg.z_dim, mapping_network=G.mapping, device="cpu")
    w_std = float(w_std)
    z = np.random.RandomState(Z_SEED).randn(1, cfg.z_dim)
    w_start = G.mapping(torch.from_numpy(z), None).detach()

    # the reference's draws, in its order: randn_like of every noise buffer, then randn_like(w_opt) once per step
    torch.manual_seed(SEED)
    init_noise = torch.cat([torch.randn(r, r).reshape(-1) for r in lo.res]).numpy()[None]
    w_noise = np.stack([torch.randn(1, cfg.num_ws, cfg.w_dim).numpy() for _ in range(NUM_STEPS)])

    records, states = [], []

    class Recorder:
        """ForgerLosses of the reference, recording what every step's compute returns and the noise planes the step runs on (the
        reference returns neither its regulariser nor its learning rate: the regulariser is restated on these planes below)."""

        def __init__(self):
            self.inner = ref_losses.ForgerLosses.create_from_string(LOSSES)

        def compute(self, raw, truth):
            total, details = self.inner.compute(raw, truth)
            records.append({k: float(v.detach()) for k, v in details.items()})
            states.append(torch.cat([b.detach().reshape(-1) for _, b in G.synthesis.named_buffers()]).numpy().copy())
            return total, details

    torch.manual_seed(SEED)
    w_opt = ref.run_one_clarity_opt(Engine, geom_iterator(), 1, 1, torch.device("cpu"), True, w_start, w_std, Recorder(), num_steps=NUM_STEPS,
                                    output_prefix="unused")
    bufs = dict(G.synthesis.named_buffers())
    final_noise = torch.cat([bufs[n].detach().reshape(-1) for n in lo.names]).numpy()
    assert np.array_equal(states[0], init_noise[0]), "the replayed draws are not the reference's"
    planes_only = clarity.ArenaLayout(0, lo.res)
    reg_ref_states = np.array([float(cr.noise_reg_f64(s[None], planes_only)[0]) for s in states])
    names = sorted(records[0].keys())
    items = np.array([[r[k] for k in names] for r in records], np.float64)

    # the float64 statement with the same draws
    draws = cr.ReplayDraws(init_noise, w_noise, idx)
    steps64, row64 = cr.run_statement_loop(cr.OracleGen(cfg, sd, torch.float64), enc, drawings, w_start, draws, NUM_STEPS, BATCH, w_std)
    order = [["iou_inv_uvs", "iou_u", "l1_fake_orig"].index(n) for n in names]
    items64 = np.array([[s[1][j] for j in order] for s in steps64])
    lr64 = np.array([s[0] for s in steps64])
    final32 = np.concatenate([w_opt.numpy().reshape(-1), final_noise]).astype(np.float64)
    eps_items = float(np.abs(items - items64).max())
    eps_final = float(np.abs(final32 - row64).max())
    reg64 = np.array([s[2] for s in steps64])
    denom_min = np.array([s[3] for s in steps64])
    eps_reg = float(np.abs(reg_ref_states - reg64).max())
    sched = np.array([clarity.lr_and_noise_schedule(s, NUM_STEPS, w_std) for s in range(NUM_STEPS)])
    out = dict(drawings=drawings, drawing_idx=idx, z=z, w_start=w_start.numpy(), w_avg=w_avg, w_std=np.float64(w_std), w_stats_samples=np.int64(500),
               init_noise=init_noise, w_noise=w_noise, item_names=np.array(names), items=items, lr=lr64, w_noise_scale=sched[:, 1],
               reg_f64=reg64, adam_denom_min=denom_min, reg_ref_states=reg_ref_states, final_w=w_opt.numpy(), final_noise=final_noise, final_row_f64=row64, items_f64=items64,
               eps_items=np.float64(eps_items), eps_final=np.float64(eps_final), eps_reg=np.float64(eps_reg),
               eps_ref=np.float64(max(eps_items, eps_final, eps_reg)),
               state_seed=np.int64(3), num_steps=np.int64(NUM_STEPS), batch=np.int64(BATCH), losses=np.array(LOSSES))
    np.savez_compressed(os.path.join(HERE, "clarity_opt.npz"), **out)
    print("clarity_opt.npz:", {k: float(v) for k, v in out.items() if k.startswith("eps")}, "items first/last", items[0], items[-1],
          "reg first/last", reg64[0], reg64[-1], "w_std", w_std)


if __name__ == "__main__":
    main()
