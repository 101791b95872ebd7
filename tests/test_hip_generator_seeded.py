"""GPU: noise_mode="seeded" of the Python pass (networks.SynthesisNetwork, graphed.GraphedTriad) -- one nb_noise_seeded_f32 launch in
place of the random path's torch.randn per layer.  The seeded pass is pinned from two sides: against the random path fed the same
normals (same launches, bit for bit), and against a constant-noise pass whose noise_buffers are those normals (another path through
the noise plumbing); then batch splits, staged passes against the C generator, and graph replays."""
import ctypes

import numpy as np
import pytest
import torch

from brushstroke_engine_amd import _lib, config as cfgmod, synthetic, weights as wmod
from test_hip_generator import PIX          # pixels / uvs across arithmetic modes and kernel variants (that file's header)

pytestmark = pytest.mark.gpu
SEED = 0xC0FFEE1234567


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def D(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def build(cfg, seed, dev, mode):
    from brushstroke_engine_amd.networks import Generator
    G = Generator(cfg, wmod.random_state_dict(cfg, seed=seed), conv_mode=mode).to(dev)
    G.sub_stream_min_batch = 10 ** 9                       # one chain of launches
    return G


def inputs(cfg, n, seed, dev):
    z = D(synthetic.batch_z(cfg, n, seed), dev).to(torch.float32)
    return z, [D(x, dev) for x in synthetic.geom_features(cfg, n, seed=seed)]


def raw_normals(cfg, seed, offset, n, dev):
    """Every layer's [n, res, res] normals of (seed, offset) before the strength multiply, from the stand-alone entry (a table with
    noise_strength = NULL; tests/test_hip_noise_seeded.py checks that entry against float64)."""
    out = [torch.empty([n, s.block_res, s.block_res], dtype=torch.float32, device=dev) for s in cfg.layers]
    descs = (_lib.NbLayerDesc * len(out))()
    for d, s, t in zip(descs, cfg.layers, out):
        d.res, d.noise_out = s.block_res, t.data_ptr()
    table = torch.from_numpy(np.frombuffer(bytes(descs), dtype=np.uint8).copy()).to(dev)
    _lib.check(_lib.lib().nb_noise_seeded_f32(table.data_ptr(), 0, len(out), cfg.img_resolution, seed, offset, None, n,
                                              torch.cuda.current_stream().cuda_stream), "noise_seeded")
    torch.cuda.synchronize()
    return out


def large_kernel_plan(G, n):
    """(an up=1 layer, an up=2 layer on the large split-f16 kernels, ToRGB fused) in the plan of a seeded / random pass at batch n."""
    kp = G.synthesis.pass_plan(n, noise_positions=_lib.NB_PLAN_POS_NONE)
    large = [s.up for s, lp in zip(G.cfg.layers, kp.layers) if lp.kind == _lib.NB_KERNEL_LARGE_H3]
    return 1 in large, 2 in large, any(lp.fused_torgb for lp in kp.layers)


# tiny_config(32) in every arithmetic mode, and the smallest style1 shape whose plan holds the large kernels: by the planner's
# thresholds (output pixels per batch) R=32 needs batch 16, R=64 batch 4, R=128 batch 1 -- the same 16384 pixels; (64, 4) is the one
# with both a batch to index and the fewest layers.  test_large_shape_plan asserts it.
LARGE_R, LARGE_N = 64, 4
CASES = [("tiny", 32, 3, m) for m in ("f32", "h3", "f8")] + [("style1", LARGE_R, LARGE_N, m) for m in ("f8", "h3")]


def make(kind, res, mode, dev):
    return build(cfgmod.tiny_config(res) if kind == "tiny" else cfgmod.style1_config(res), 3, dev, mode)


@pytest.mark.parametrize("mode", ["f8", "h3"])
def test_large_shape_plan(dev, mode):
    G = make("style1", LARGE_R, mode, dev)
    assert large_kernel_plan(G, LARGE_N) == (True, True, True)
    assert large_kernel_plan(G, LARGE_N - 1) != (True, True, True)            # ... and no smaller batch at this resolution does


def render_all(G, z, geom, **kw):
    """(img, uvs, colors, rgba_u8) of one mode: the plain forward's image and the fused compositing's outputs."""
    img = G(z, None, geom, **kw).clone()
    u8, _, dbg = G.render_triad(z=z, geom_feature=geom, **kw)
    return img, dbg["uvs"].clone(), dbg["colors"].clone(), u8.clone()


@pytest.mark.parametrize("kind, res, n, mode", CASES)
def test_seeded_equals_random_path_fed_the_same_normals(dev, monkeypatch, kind, res, n, mode):
    G = make(kind, res, mode, dev)
    cfg = G.cfg
    if kind == "style1":
        assert large_kernel_plan(G, n) == (True, True, True)
    z, geom = inputs(cfg, n, 11, dev)
    offset = 2 ** 32 - 2
    normals = raw_normals(cfg, SEED, offset, n, dev)
    calls = []

    def fake_randn(shape, **kw):
        t = normals[len(calls) % len(normals)]
        assert list(shape) == list(t.shape) and kw["device"] == t.device
        calls.append(tuple(shape))
        return t.clone()

    monkeypatch.setattr(torch, "randn", fake_randn)
    want = render_all(G, z, geom, noise_mode="random")
    monkeypatch.undo()
    assert len(calls) == 2 * len(cfg.layers)                                   # one draw per layer and pass
    monkeypatch.setattr(torch, "randn", lambda *a, **k: pytest.fail("the seeded pass called torch.randn"))
    got = render_all(G, z, geom, noise_mode="seeded", noise_seed=SEED, noise_offset=offset)
    monkeypatch.undo()
    torch.cuda.synchronize()
    for name, g, w in zip(("img", "uvs", "colors", "rgba_u8"), got, want):
        assert torch.equal(g, w), name
    # the noise reaches the image: another offset, another image
    other = G(z, None, geom, noise_mode="seeded", noise_seed=SEED, noise_offset=offset + n)
    assert not torch.equal(other, got[0])
    # ... and the state tensor is the same source as the by-value pair
    as_i64 = lambda v: v - 2 ** 64 if v >= 2 ** 63 else v
    state = torch.tensor([as_i64(SEED), as_i64(offset)], dtype=torch.int64, device=dev)
    assert torch.equal(G(z, None, geom, noise_mode="seeded", noise_state=state), got[0])


def const_pass_with_normals(G, z1, geom1, normals, k):
    """A batch-1 constant-noise pass without positions whose noise_buffers are sample k's raw normals."""
    bufs = {f"b{s.block_res}.conv{0 if s.up == 2 else 1}.noise_const": t[k] for s, t in zip(G.cfg.layers, normals)}
    img, dbg = G(z1, None, geom1, noise_mode="const", noise_buffers=bufs, return_debug_data=True)
    return img, dbg["uvs"]


def test_seeded_equals_const_pass_with_noise_buffers_f32(dev):
    """conv_mode f32: the batch-1 seeded pass at offset o + k IS the const pass on sample k's normals (same plan, same launches but
    for the noise kernel: bit for bit); sample k of the seeded batch runs kernel variants chosen for its batch size, and equals it
    within tests/test_hip_generator.py's figure for a sample against its sub-batch in f32 (2e-5)."""
    G = make("tiny", 32, "f32", dev)
    n, offset = 3, 40
    z, geom = inputs(G.cfg, n, 12, dev)
    normals = raw_normals(G.cfg, SEED, offset, n, dev)
    batch, dbg = G(z, None, geom, noise_mode="seeded", noise_seed=SEED, noise_offset=offset, return_debug_data=True)
    for k in range(n):
        z1, geom1 = z[k:k + 1], [g[k:k + 1] for g in geom]
        want, want_uvs = const_pass_with_normals(G, z1, geom1, normals, k)
        one, dbg1 = G(z1, None, geom1, noise_mode="seeded", noise_seed=SEED, noise_offset=offset + k, return_debug_data=True)
        assert torch.equal(one, want) and torch.equal(dbg1["uvs"], want_uvs), k
        assert float((batch[k:k + 1] - want).abs().max()) <= 2e-5 and float((dbg["uvs"][k:k + 1] - want_uvs).abs().max()) <= 2e-5, k


@pytest.mark.parametrize("mode", ["f8", "h3"])
def test_seeded_equals_const_pass_with_noise_buffers_large_kernels(dev, mode):
    """The large-kernel shape against batch-1 const passes (which run the small kernels): within PIX[mode], the tolerance
    tests/test_hip_generator.py holds pixels and uvs to across arithmetic modes."""
    G = make("style1", LARGE_R, mode, dev)
    n, offset = LARGE_N, 2 ** 64 - 2
    assert large_kernel_plan(G, n) == (True, True, True)
    z, geom = inputs(G.cfg, n, 13, dev)
    normals = raw_normals(G.cfg, SEED, offset, n, dev)
    batch, dbg = G(z, None, geom, noise_mode="seeded", noise_seed=SEED, noise_offset=offset, return_debug_data=True)
    for k in range(n):
        want, want_uvs = const_pass_with_normals(G, z[k:k + 1], [g[k:k + 1] for g in geom], normals, k)
        e_img, e_uvs = float((batch[k:k + 1] - want).abs().max()), float((dbg["uvs"][k:k + 1] - want_uvs).abs().max())
        print(f"{mode} sample {k}: img {e_img:.3g} uvs {e_uvs:.3g}")
        assert e_img <= PIX[mode] and e_uvs <= PIX[mode], (k, e_img, e_uvs)
    # (the comparison sees the noise: the same pass without it is far outside the tolerance)
    none = G(z, None, geom, noise_mode="none")
    assert float((none - batch).abs().max()) > 10 * PIX[mode]


@pytest.mark.parametrize("mode", ["f32", "h3", "f8"])
def test_batch_split(dev, mode):
    """Samples 2..3 of an n = 4, offset 10 pass are the n = 2, offset 12 pass: bit for bit, since both batches get the same plan."""
    G = make("tiny", 32, mode, dev)
    plan = lambda n: [tuple(sorted(vars(lp).items())) for lp in G.synthesis.pass_plan(n, noise_positions=_lib.NB_PLAN_POS_NONE).layers]
    assert plan(4) == plan(2)
    z, geom = inputs(G.cfg, 4, 14, dev)
    whole, dw = G(z, None, geom, noise_mode="seeded", noise_seed=SEED, noise_offset=10, return_debug_data=True)
    whole, uvs = whole.clone(), dw["uvs"].clone()
    part, dp = G(z[2:], None, [g[2:] for g in geom], noise_mode="seeded", noise_seed=SEED, noise_offset=12, return_debug_data=True)
    assert torch.equal(part, whole[2:]) and torch.equal(dp["uvs"], uvs[2:])
    shifted = G(z[2:], None, [g[2:] for g in geom], noise_mode="seeded", noise_seed=SEED, noise_offset=10)
    assert not torch.equal(shifted, whole[2:])


@pytest.mark.parametrize("mode", ["f8", "h3"])
def test_staged_passes_equal_the_c_generator(dev, mode):
    """_stop_after=64, then _resume from its (perturbed) features, with one seed: the C head / tail with that seed, bit for bit.  The
    tail's noise launch starts at layer 9 of 11: the layer index is absolute on both sides."""
    from brushstroke_engine_amd.native import NativeGenerator
    G = build(cfgmod.style1_config(128), 5, dev, mode)
    cfg, n, offset = G.cfg, 2, 77
    ng = NativeGenerator.from_generator(G, n_max=n)
    try:
        z, geom = inputs(cfg, n, 15, dev)
        kw = dict(noise_mode="seeded", noise_seed=SEED, noise_offset=offset)
        head = G(z, None, geom, _stop_after=64, **kw).clone()
        got = torch.full_like(head, 7.0)
        ng.head(n, 64, got, z=z, geom_feature=geom, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got, head)
        x = (head * 1.25 + 0.01).contiguous()                                  # what a blend hands the tail is not the head's own value
        u8, _, dbg = G.render_triad(z=z, geom_feature=geom, _resume=(64, x), **kw)
        outs = {"rgba_u8": torch.zeros([n, 128, 128, 4], dtype=torch.uint8, device=dev), "uvs": torch.zeros([n, 3, 128, 128], device=dev),
                "colors": torch.zeros([n, 3, 3], device=dev)}
        ng.tail(n, 64, x, outs, z=z, geom_feature=geom, **kw)
        torch.cuda.synchronize()
        assert torch.equal(outs["rgba_u8"], u8) and torch.equal(outs["uvs"], dbg["uvs"]) and torch.equal(outs["colors"], dbg["colors"])
        # the tail's layers drew the noise of layers 9 and 10, not of 0 and 1: the batch-1 tail is the constant-noise tail whose
        # noise_buffers are those layers' normals
        z1, geom1, x1 = z[:1], [g[:1] for g in geom], x[:1].contiguous()
        normals = raw_normals(cfg, SEED, offset, 1, dev)
        bufs = {f"b{s.block_res}.conv{0 if s.up == 2 else 1}.noise_const": t[0] for s, t in zip(cfg.layers, normals)}
        want_u8, _, _ = G.render_triad(z=z1, geom_feature=geom1, _resume=(64, x1), noise_mode="const", noise_buffers=bufs)
        got_u8, _, _ = G.render_triad(z=z1, geom_feature=geom1, _resume=(64, x1), **kw)
        assert [s.block_res for s in cfg.layers[9:]] == [128, 128] and torch.equal(got_u8, want_u8)
    finally:
        ng.close()


def test_graph_replays_draw_fresh_noise(dev):
    from brushstroke_engine_amd.graphed import GraphedTriad
    G = build(cfgmod.style1_config(64), 5, dev, "f8")
    cfg = G.cfg
    z, geom = inputs(cfg, 1, 16, dev)
    gr = GraphedTriad(G, batch=1, noise_mode="seeded")
    outs = []
    for offset in (0, 1, 0):
        u8, _, dbg = gr(z=z, geom_feature=geom, noise_seed=SEED, noise_offset=offset)
        torch.cuda.synchronize()
        outs.append((u8.clone(), dbg["uvs"].clone()))
        e8, _, edbg = G.render_triad(z=z, geom_feature=geom, noise_mode="seeded", noise_seed=SEED, noise_offset=offset)
        assert torch.equal(outs[-1][0], e8) and torch.equal(outs[-1][1], edbg["uvs"]), offset
    assert not torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[0][1], outs[2][1])
    # default construction is unchanged: constant noise, no state tensor
    assert GraphedTriad(G, batch=1).noise_state is None
