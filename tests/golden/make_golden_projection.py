"""Golden vectors for brushstroke_engine_amd.projection: the REFERENCE's ``project()`` (scripts/project_main.py) driven on the CPU for
8 steps, twice: W+ with the composite over the mean background colour, and W without the composite; ``l1_fg_weight`` and ``bg_weight``
positive in both.  Build container only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_projection.py

The generator handed to the reference is a stand-in: ``G.synthesis`` is a small torch module around ``oracle.OracleGenerator``
(``tiny_config(32)``, float32) whose ``noise_const`` buffers are registered under the reference's names (a fresh one per run:
``project()`` leaves its buffers requiring grad), the geometry features come from ``clarity_refs.StandInEncoder``, and
``geom_metric.lpips_batched_vgg`` is replaced by ``projection_refs.stand_in_perceptual``.  Modules the reference imports for its
visualisations and data sets, and which this container does not have, are stubbed with the finder of make_golden_clarity.py.

On the CPU the reference's ``w_best`` / ``noise_best`` (``.detach().cpu()``) share memory with the tensors Adam updates in place, so
what ``project()`` returns there is the state after the LAST step; that is what is recorded as final_w / final_noise.

Recorded: the exemplar's seed (it is ``projection_refs.exemplar``) and, per run, the random draws (initial noise planes, the W noise of each step, replayed in the reference's order),
the perceptual value of each step, the final w and noise planes, ``bg``, and eps_ref = the deviation of those float32 results from
the float64 statement (tests/projection_refs.py) driven with the same draws, with that run's lr and smallest Adam denominators.
"""
import logging
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_clarity as mgc                                          # the stub finder, the paths

NUM_STEPS, B, SEED, EXEMPLAR_SEED = 8, 3, 91, 11
WEIGHTS = (0.5, 0.25)
RUNS = {"wplus_comp": dict(w_plus=True, with_composite=True), "w_nocomp": dict(w_plus=False, with_composite=False)}


def load_reference_script():
    import importlib.util
    sys.meta_path.append(mgc._StubFinder())
    spec = importlib.util.spec_from_file_location("project_main", os.path.join(mgc.REFERENCE, "scripts", "project_main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import clarity_refs as cr
    import projection_refs as pr
    from brushstroke_engine_amd import clarity, config as cfgmod, weights as wmod
    ref = load_reference_script()
    import forger.metrics.geom_metric as ref_gm
    import thirdparty.stylegan2_ada_pytorch.experiment.util.latent as ref_latent
    logging.disable(logging.CRITICAL)

    cfg = cfgmod.tiny_config(32)
    sd = wmod.random_state_dict(cfg, seed=3)
    full = clarity.ArenaLayout.from_config(cfg)
    gen32 = pr.OracleGen(cfg, sd, torch.float32)
    enc = cr.StandInEncoder(cfg)
    ex = pr.exemplar(cfg.img_resolution, B, seed=EXEMPLAR_SEED)

    class Synthesis(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for name in full.names:
                blk, conv, leaf = name.split(".")
                if not hasattr(self, blk):
                    setattr(self, blk, torch.nn.Module())
                if not hasattr(getattr(self, blk), conv):
                    setattr(getattr(self, blk), conv, torch.nn.Module())
                getattr(getattr(self, blk), conv).register_buffer(leaf, torch.from_numpy(np.asarray(sd["synthesis." + name], np.float32)).clone())

        def forward(self, ws, geom_feature=None, noise_mode="const", norm_noise_positions=None, noise_buffers=None, return_debug_data=False):
            return gen32.synthesis(ws, geom_feature, norm_noise_positions=norm_noise_positions, noise_mode=noise_mode, noise_buffers=noise_buffers,
                                   return_debug_data=return_debug_data)

    class Mapping:
        num_ws = cfg.num_ws

        def __call__(self, z, c=None):
            return gen32.mapping(z, c)

    w_avg, w_std = ref_latent.get_w_stats(num_samples=500, z_dim=cfg.z_dim, mapping_network=Mapping(), device="cpu")
    w_std = float(w_std)
    perc_values = []

    def perceptual(target, synth):
        v = pr.stand_in_perceptual(target, synth)
        perc_values.append(float(v.mean().detach()))
        return v

    ref_gm.lpips_batched_vgg = perceptual
    target, geom = ex[0] * 2 - 1, ex[1]
    feats = enc(geom)
    # (the exemplar is projection_refs.exemplar(32, B, EXEMPLAR_SEED), numpy's legacy generator: its seed and two sums are recorded, not
    # its 36 KB; the initial noise planes are the same draws in both runs and are recorded once)
    out = dict(exemplar_seed=np.int64(EXEMPLAR_SEED), patches=np.int64(B), target_sum=np.float64(ex[0].double().sum()),
               geom_sum=np.float64(ex[1].double().sum()), w_avg=w_avg, w_std=np.float64(w_std), w_stats_samples=np.int64(500), state_seed=np.int64(3),
               num_steps=np.int64(NUM_STEPS), weights=np.array(WEIGHTS), run_names=np.array(sorted(RUNS)))
    eps_all = []
    for name, opt in sorted(RUNS.items()):
        rows = cfg.num_ws if opt["w_plus"] else 1
        torch.manual_seed(SEED)
        init_noise = torch.cat([torch.randn(r, r).reshape(-1) for r in full.res]).numpy()[None]
        w_noise = np.stack([torch.randn(1, rows, cfg.w_dim).numpy() for _ in range(NUM_STEPS)])
        G = types.SimpleNamespace(synthesis=Synthesis(), mapping=Mapping(), z_dim=cfg.z_dim, img_resolution=cfg.img_resolution, img_channels=3)
        assert [n for n, _ in G.synthesis.named_buffers()] == full.names
        del perc_values[:]
        torch.manual_seed(SEED)
        res = ref.project(G, target=target, geom=geom, geom_feature=feats, device=torch.device("cpu"), w_plus=opt["w_plus"], num_steps=NUM_STEPS,
                          with_composite=opt["with_composite"], l1_fg_weight=WEIGHTS[0], bg_weight=WEIGHTS[1], w_std=w_std, w_avg=w_avg)
        assert res["step"] == NUM_STEPS - 1 and len(perc_values) == NUM_STEPS
        final_w = res["w"].detach().numpy().copy()
        final_noise = torch.cat([res["noise"][n].detach().reshape(-1) for n in full.names]).numpy().copy()
        bufs = dict(G.synthesis.named_buffers())
        assert np.array_equal(final_noise, torch.cat([bufs[n].detach().reshape(-1) for n in full.names]).numpy()), "the result is not the live state"

        w_start = np.concatenate([w_avg] * rows, axis=1)
        draws = cr.ReplayDraws(init_noise, w_noise[:, None], np.zeros([NUM_STEPS, 1], np.int64))
        steps64, row64, _, bg64 = pr.run_statement_loop(pr.OracleGen(cfg, sd, torch.float64), enc, ex, torch.from_numpy(w_start), draws, NUM_STEPS, w_std,
                                                        opt["w_plus"], opt["with_composite"], WEIGHTS, perceptual=pr.stand_in_perceptual)
        final32 = np.concatenate([final_w.reshape(-1), final_noise]).astype(np.float64)
        perc64 = np.array([s[1][2] for s in steps64])
        eps = dict(final=float(np.abs(final32 - row64).max()), perc=float(np.abs(np.array(perc_values) - perc64).max()),
                   bg=float(np.abs(res["bg"].numpy().astype(np.float64) - bg64).max()))
        eps_all.append(max(eps.values()))
        assert "init_noise" not in out or np.array_equal(out["init_noise"], init_noise)
        out["init_noise"] = init_noise
        out.update({f"{name}/w_noise": w_noise, f"{name}/perceptual": np.array(perc_values), f"{name}/final_w": final_w,
                    f"{name}/final_noise": final_noise, f"{name}/bg": res["bg"].numpy(),
                    f"{name}/lr": np.array([s[0] for s in steps64]), f"{name}/adam_denom_min": np.array([s[3] for s in steps64]),
                    f"{name}/eps_ref": np.float64(max(eps.values()))})
        print(name, eps, "perceptual first/last", perc_values[0], perc_values[-1])
    out["eps_ref"] = np.float64(max(eps_all))
    np.savez_compressed(os.path.join(HERE, "projection.npz"), **out)
    print("projection.npz: eps_ref", float(out["eps_ref"]), os.path.getsize(os.path.join(HERE, "projection.npz")), "bytes")


if __name__ == "__main__":
    main()
