"""ms per Generator.render_triad step under noise_mode const / random / seeded, same box, same process.

style1_config(R) at each batch of --batches (default 32 and 1), the library's default arithmetic; inputs without positions for all
three modes (random and seeded ignore them; const then shares one noise image per layer).  The modes alternate: --pairs rounds
(default 3) of [const, random, seeded], each a window of --steps (default 200) steps between two device events after a warm-up of
every mode; the figure per mode is the median of its windows, the spread their min / max.  Seeded steps advance noise_offset by the
batch, as a run that numbers its samples would.

    python tools/bench_noise_modes.py [--res 256] [--batches 32,1] [--steps 200] [--pairs 3] [--out profiles/noise_modes.json]
    python tools/bench_noise_modes.py --only seeded --steps 50 --pairs 1        # a short run to put under a kernel trace

--brush-noise: what a projected brush's noise buffers cost per step, in the same window scheme.  The legs alternate const (the
checkpoint's noise), noise_buffers (the per-call dict: the plan with noise overrides, a layer table built and uploaded per step) and
noise_set (networks.BrushNoise: the ordinary plan on the set's tables), all WITH integer positions -- without them the three run the
same launches.  --legs picks a subset (a tree without noise sets times const,noise_buffers).

    python tools/bench_noise_modes.py --brush-noise [--legs const,noise_buffers,noise_set] [--out profiles/brush_noise.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brushstroke_engine_amd import build, config as cfgmod, synthetic, weights as wmod  # noqa: E402
from brushstroke_engine_amd.networks import Generator  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--batches", default="32,1")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--brush-noise", action="store_true")
    ap.add_argument("--legs", default="const,noise_buffers,noise_set")
    a = ap.parse_args()
    build.build(verbose=False)
    if not torch.cuda.is_available():
        sys.exit("bench_noise_modes: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    cfg = cfgmod.style1_config(a.res)
    G = Generator(cfg, wmod.random_state_dict(cfg, seed=0)).to(dev)
    modes = [a.only] if a.only else ["const", "random", "seeded"]
    if a.brush_noise:
        modes = a.legs.split(",")
        rs = np.random.RandomState(7)
        bufs = {f"b{s.block_res}.conv{0 if s.up == 2 else 1}.noise_const": torch.from_numpy(rs.randn(s.block_res, s.block_res).astype(np.float32)).to(dev)
                for s in cfg.layers}
        noise_set = G.synthesis.brush_noise().load(bufs) if "noise_set" in modes else None
    noise_pixels = sum(s.block_res ** 2 for s in cfg.layers)
    result = {"res": a.res, "conv_mode": G.synthesis.conv_mode, "steps": a.steps, "pairs": a.pairs, "device": torch.cuda.get_device_name(0),
              "noise_bytes_per_sample": 4 * noise_pixels, "batches": {}}
    if a.brush_noise:
        result["legs"], result["positions"] = modes, True
    for n in (int(b) for b in a.batches.split(",")):
        z = torch.from_numpy(synthetic.batch_z(cfg, n, 0).astype(np.float32)).to(dev)
        geom = [torch.from_numpy(g).to(dev) for g in synthetic.geom_features(cfg, n, seed=1)]
        offset = [0]

        pos = torch.from_numpy(synthetic.positions(cfg, n, seed=2)).to(dev)

        def step(mode):
            if a.brush_noise:
                kw = {"noise_buffers": bufs} if mode == "noise_buffers" else {"noise_set": noise_set} if mode == "noise_set" else {}
                return G.render_triad(z=z, geom_feature=geom, positions=pos, noise_mode="const", **kw)
            kw = {}
            if mode == "seeded":
                kw = dict(noise_seed=1234, noise_offset=offset[0])
                offset[0] += n
            return G.render_triad(z=z, geom_feature=geom, noise_mode=mode, **kw)

        for mode in modes:                                   # warm every mode: code objects, workspaces, packed weights
            for _ in range(10):
                step(mode)
        torch.cuda.synchronize()
        windows = {m: [] for m in modes}
        for _ in range(a.pairs):
            for mode in modes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    step(mode)
                e1.record()
                torch.cuda.synchronize()
                windows[mode].append(e0.elapsed_time(e1) / a.steps)
        row = {m: {"ms_per_step": float(np.median(w)), "min": float(min(w)), "max": float(max(w))} for m, w in windows.items()}
        if a.brush_noise:
            row["kernels"] = sorted(set(G.synthesis.layer_kernels.values()))
        else:
            row["noise_mb_written_per_step"] = 4e-6 * noise_pixels * n
        result["batches"][str(n)] = row
        print(f"R={a.res} batch {n}: " + "  ".join(f"{m} {row[m]['ms_per_step']:.4f} ms [{row[m]['min']:.4f}, {row[m]['max']:.4f}]" for m in modes),
              flush=True)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
