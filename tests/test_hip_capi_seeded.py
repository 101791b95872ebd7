"""GPU: NB_NOISE_SEEDED through the C generator (nb_generator_forward, _forward_geom, _forward_staged via native.NativeGenerator)
against the Python seeded pass, bit for bit, with the seed by value and through the noise_state pointer; and
examples/capi/variations.c (one graph, K replays, 16 bytes of state written before each) against NativeGenerator."""
import os
import subprocess

import numpy as np
import pytest
import torch

from brushstroke_engine_amd import config as cfgmod, encoder as encmod, synthetic, weights as wmod
from brushstroke_engine_amd.native import NativeGenerator, param_table
from brushstroke_engine_amd.networks import Generator

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, OFFSET = 0xFEEDFACE0BADF00D, 2 ** 32 - 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def D(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def stroke_masks(n, r, seed):
    """Stroke patches [n, 1, r, r] fp32, 1 = background."""
    rs = np.random.RandomState(seed)
    g = np.ones((n, 1, r, r), np.float32)
    yy, xx = np.mgrid[0:r, 0:r]
    for i in range(n):
        for _ in range(3):
            cy, cx, rad = rs.uniform(0, r), rs.uniform(0, r), rs.uniform(r / 10, r / 3)
            g[i, 0][(yy - cy) ** 2 + (xx - cx) ** 2 < rad ** 2] = np.float32(rs.randint(0, 200)) / np.float32(255.0)
    return g


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[2]["uvs"], b[2]["uvs"]) and torch.equal(a[2]["colors"], b[2]["colors"])


@pytest.mark.parametrize("mode", ["f8", "h3"])
def test_native_generator_equals_python_seeded_pass(dev, mode):
    R, n = 128, 3
    cfg = cfgmod.style1_config(R)
    G = Generator(cfg, wmod.random_state_dict(cfg, seed=5), conv_mode=mode).to(dev)
    G.sub_stream_min_batch = 10 ** 9                          # the Python pass as one chain too
    ng = NativeGenerator.from_generator(G, n_max=n)
    try:
        esd = encmod.random_encoder_state_dict(5)
        enc = encmod.HipGeometryEncoder(esd, "-11inverse")
        enc.arith = "f8" if mode == "f8" else "h3"             # TileOps' rule
        ng.attach_encoder(esd, "-11inverse")
        z = D(synthetic.batch_z(cfg, n, 31).astype(np.float32), dev)
        geom = [D(g, dev) for g in synthetic.geom_features(cfg, n, seed=31)]
        mask = D(stroke_masks(n, R, 31), dev)
        as_i64 = lambda v: v - 2 ** 64 if v >= 2 ** 63 else v
        state = torch.tensor([as_i64(SEED), as_i64(OFFSET)], dtype=torch.int64, device=dev)
        by_value = dict(noise_mode="seeded", noise_seed=SEED, noise_offset=OFFSET)
        by_state = dict(noise_mode="seeded", noise_state=state, noise_seed=1, noise_offset=2)       # (by-value fields are ignored)
        # ---- whole passes: features, and stroke patches through the attached encoder ----
        want = G.render_triad(z=z, geom_feature=geom, **by_value)
        want_geom = G.render_triad(z=z, geom_feature=enc.lazy(mask), **by_value)
        const = G.render_triad(z=z, geom_feature=geom)
        assert not torch.equal(want[0], const[0])
        for kw in (by_value, by_state):
            assert same(ng.render_triad(z=z, geom_feature=geom, **kw), want)
            assert same(ng.render_triad(z=z, geom=mask, **kw), want_geom)
        # ---- head / tail at the blending block ----
        res = R // 2
        head = G(z, None, geom, _stop_after=res, **by_value).clone()
        x = (head * 0.75 - 0.02).contiguous()
        tail = G.render_triad(z=z, geom_feature=geom, _resume=(res, x), **by_value)
        for kw in (by_value, by_state):
            got = torch.full_like(head, 7.0)
            ng.head(n, res, got, z=z, geom_feature=geom, **kw)
            outs = {"rgba_u8": torch.zeros([n, R, R, 4], dtype=torch.uint8, device=dev), "uvs": torch.zeros([n, 3, R, R], device=dev),
                    "colors": torch.zeros([n, 3, 3], device=dev)}
            ng.tail(n, res, x, outs, z=z, geom_feature=geom, **kw)
            torch.cuda.synchronize()
            assert torch.equal(got, head)
            assert torch.equal(outs["rgba_u8"], tail[0]) and torch.equal(outs["uvs"], tail[2]["uvs"]) and torch.equal(outs["colors"], tail[2]["colors"])
    finally:
        ng.close()


def test_variations_example(dev, tmp_path):
    exe = str(tmp_path / "variations")
    cmd = ["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
           os.path.join(REPO, "examples", "capi", "variations.c"), "-o", exe, "-L/opt/rocm/lib", "-lamdhip64",
           "-L" + os.path.join(REPO, "brushstroke_engine_amd", "csrc"), "-lneube_hip"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    R, K, mode = 64, 3, "f8"
    cfg = cfgmod.style1_config(R)
    sd = wmod.random_state_dict(cfg, seed=13)
    with open(tmp_path / "weights.bin", "wb") as f:
        for name, _ in param_table(cfg):
            f.write(np.ascontiguousarray(np.asarray(sd[name], np.float32)).tobytes())
    z = synthetic.batch_z(cfg, 1, 21).astype(np.float32)
    geom = synthetic.geom_features(cfg, 1, seed=21)
    with open(tmp_path / "inputs.bin", "wb") as f:
        for a in [z] + geom:
            f.write(np.ascontiguousarray(a).tobytes())
    out = str(tmp_path / "out.bin")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(REPO, "brushstroke_engine_amd", "csrc"), "/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    r = subprocess.run([exe, str(R), mode, str(K), hex(SEED), str(OFFSET), str(tmp_path / "weights.bin"), str(tmp_path / "inputs.bin"), out],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(out, dtype=np.uint8).reshape(K, R, R, 4)
    ng = NativeGenerator.from_state_dict(cfg, sd, mode, 1, dev)
    try:
        for i in range(K):
            u8, _, _ = ng.render_triad(z=D(z, dev), geom_feature=[D(g, dev) for g in geom], noise_mode="seeded", noise_seed=SEED,
                                       noise_offset=OFFSET + i)
            assert np.array_equal(got[i], u8[0].cpu().numpy()), i
    finally:
        ng.close()
    assert not np.array_equal(got[0], got[1])
