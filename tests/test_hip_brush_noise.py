"""Generator passes on a brush noise set (``noise_set=``, networks.BrushNoise): the brush's noise buffers at fixed device addresses, read
by the ORDINARY planned pass -- in-kernel noise of the large kernels, the fused styles + noise launch of small batches and
positions_once included (tests/test_brush_noise_cpu.py shows the shapes below reach those rows).

The yardstick is a second generator built from the same state dict with every noise_const replaced by the buffers: its pass runs
the same launches on the same values, so everything must agree bit for bit.  The older ``noise_buffers=dict`` route (another plan:
per-call overrides) is compared within the parity tolerance of tests/test_hip_generator.py."""
import numpy as np
import pytest
import torch

from brushstroke_engine_amd import config as cfgmod, synthetic, weights as wmod
from brushstroke_engine_amd.networks import BrushNoise, Generator
from conftest import load_golden
from test_hip_generator import PIX

pytestmark = pytest.mark.gpu
MODES = ("f32", "h3", "f8")
# tiny n=3; style1 R=64 at n=4 (large kernels with in-kernel noise, fused styles + noise launch) and n=9 (positions_once)
SHAPES = {"tiny3": ("tiny", 3), "s64n4": ("s64", 4), "s64n9": ("s64", 9)}
CFGS = {"tiny": cfgmod.tiny_config(32), "s64": cfgmod.style1_config(64)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def D(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def key_of(s):
    return f"b{s.block_res}.conv{0 if s.up == 2 else 1}.noise_const"


def buffers(cfg, seed):
    """Seeded standard normals for every layer, under the reference's noise_buffers key names (host float32)."""
    rs = np.random.RandomState(seed)
    return {key_of(s): rs.randn(s.block_res, s.block_res).astype(np.float32) for s in cfg.layers}


def with_noise(sd, bufs):
    sd = dict(sd)
    for k, v in bufs.items():
        assert "synthesis." + k in sd
        sd["synthesis." + k] = v
    return sd


_NETS = {}


def nets(name, mode, dev):
    """(cfg, G, G2, B, set of G loaded with B): G2's checkpoint holds B.  Built once per (config, mode)."""
    if (name, mode) not in _NETS:
        cfg = CFGS[name]
        sd = wmod.random_state_dict(cfg, seed=3)
        B = buffers(cfg, 77)
        G = Generator(cfg, sd, conv_mode=mode).to(dev)
        G2 = Generator(cfg, with_noise(sd, B), conv_mode=mode).to(dev)
        _NETS[(name, mode)] = (cfg, G, G2, B, G.synthesis.brush_noise().load(B))
    return _NETS[(name, mode)]


def inputs(cfg, n, dev):
    ws = D(np.random.RandomState(5).randn(n, cfg.num_ws, cfg.w_dim).astype(np.float32), dev)
    geom = [D(g, dev) for g in synthetic.geom_features(cfg, n, seed=2)]
    return ws, geom, D(synthetic.positions(cfg, n, seed=4), dev)


def run(G, ws, geom, pos, **kw):
    """One pass -> (img, uvs, colors, rgba_u8) on the host, and the kernels it ran."""
    extra = {"rgba_u8": True, "render_mode": "clear"}
    img, dbg = G.forward_pre_mapped(ws, geom, positions=pos, return_debug_data=True, noise_mode="const", _extra_outputs=extra, **kw)
    torch.cuda.synchronize()
    out = dict(img=img.cpu().numpy(), uvs=dbg["uvs"].cpu().numpy(), colors=dbg["colors"].cpu().numpy(),
               rgba_u8=extra["out"]["rgba_u8"].cpu().numpy())
    return out, dict(G.synthesis.layer_kernels)


def same(a, b, what):
    for k in ("img", "uvs", "colors", "rgba_u8"):
        assert np.array_equal(a[k], b[k]), (what, k, float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max()))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_set_equals_checkpoint_with_the_buffers_bit_for_bit(dev, shape, mode):
    name, n = SHAPES[shape]
    cfg, G, G2, B, bn = nets(name, mode, dev)
    ws, geom, pos = inputs(cfg, n, dev)
    got, k1 = run(G, ws, geom, pos, noise_set=bn)
    want, k2 = run(G2, ws, geom, pos)
    same(got, want, shape)
    assert k1 == k2 and len(k1) == len(cfg.layers) + 1
    # ... and it is the brush's noise that was rendered, not the checkpoint's
    plain, _ = run(G, ws, geom, pos)
    assert np.abs(plain["uvs"] - got["uvs"]).max() > 10 * PIX[mode]
    # a second pass at the batch size uploads nothing: the set's tables of this workspace are all there
    tables = {k: dict(v[1]) for k, v in bn._tables.items()}
    again, _ = run(G, ws, geom, pos, noise_set=bn)
    same(again, want, shape + " again")
    assert {k: dict(v[1]) for k, v in bn._tables.items()}.keys() == tables.keys()
    assert all(t is tables[k][f] for k, v in bn._tables.items() for f, t in v[1].items())


@pytest.mark.parametrize("mode", MODES)
def test_no_positions_and_staged_passes(dev, mode):
    cfg, G, G2, B, bn = nets("s64", mode, dev)
    ws, geom, pos = inputs(cfg, 4, dev)
    same(run(G, ws, geom, None, noise_set=bn)[0], run(G2, ws, geom, None)[0], "no positions")
    # a head that stops after block 32, and the tail that resumes behind it
    x1 = G.forward_pre_mapped(ws, geom, positions=pos, noise_mode="const", _stop_after=32, noise_set=bn)
    x2 = G2.forward_pre_mapped(ws, geom, positions=pos, noise_mode="const", _stop_after=32)
    assert torch.equal(x1, x2)
    got, k1t = run(G, ws, geom, pos, _resume=(32, x1), noise_set=bn)
    want, k2t = run(G2, ws, geom, pos, _resume=(32, x2))
    same(got, want, "staged")
    assert k1t == k2t
    same(got, run(G2, ws, geom, pos)[0], "staged == whole")


@pytest.mark.parametrize("mode", MODES)
def test_partial_dict_keeps_the_checkpoint_elsewhere(dev, mode):
    cfg, G, _, B, _ = nets("tiny", mode, dev)
    part = {k: v for k, v in B.items() if k.startswith("b8.")}
    assert 0 < len(part) < len(B)
    part["b16.conv1.noise_const"] = None                      # a None value = the checkpoint's buffer, like a missing key
    sd = wmod.random_state_dict(cfg, seed=3)
    G3 = Generator(cfg, with_noise(sd, {k: v for k, v in part.items() if v is not None}), conv_mode=mode).to(dev)
    ws, geom, pos = inputs(cfg, 3, dev)
    same(run(G, ws, geom, pos, noise_set=G.synthesis.brush_noise().load(part))[0], run(G3, ws, geom, pos)[0], "partial")
    # an unloaded set renders like no set
    same(run(G, ws, geom, pos, noise_set=G.synthesis.brush_noise())[0], run(G, ws, geom, pos)[0], "unloaded")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", ["tiny3", "s64n4"])
def test_against_the_dict_route(dev, shape, mode):
    name, n = SHAPES[shape]
    cfg, G, _, B, bn = nets(name, mode, dev)
    ws, geom, pos = inputs(cfg, n, dev)
    got, _ = run(G, ws, geom, pos, noise_set=bn)
    ref, _ = run(G, ws, geom, pos, noise_buffers={k: D(v, dev) for k, v in B.items()})
    plain, _ = run(G, ws, geom, pos)
    for k in ("img", "uvs"):
        e = float(np.abs(got[k] - ref[k]).max())
        far = float(np.abs(plain[k] - ref[k]).max())
        print(f"[brush noise {shape} {mode}] {k}: set vs dict {e:.2e} (tolerance {PIX[mode]:.0e}); dict vs no buffers {far:.2e}")
        assert e <= PIX[mode], k
        assert far > 10 * PIX[mode], k
    assert float(np.abs(got["colors"] - ref["colors"]).max()) <= 1e-5


@pytest.mark.parametrize("mode", MODES)
def test_reference_vectors_case_c(dev, mode):
    g = load_golden("gen_tiny.npz")
    cfg = cfgmod.tiny_config(32)
    G = Generator(cfg, wmod.random_state_dict(cfg, seed=int(g["weights_seed"])), conv_mode=mode).to(dev)
    geom = [D(x, dev) for x in synthetic.geom_features(cfg, 3, seed=int(g["geom_seed"]))]
    bn = G.synthesis.brush_noise().load({k[len("C_nb_"):]: g[k] for k in g if k.startswith("C_nb_")})
    img, dbg = G.forward_pre_mapped(D(g["C_ws"], dev), geom, positions=D(g["positions"][::-1].copy(), dev), return_debug_data=True,
                                    noise_mode="const", noise_set=bn)
    e = {k: float(np.abs(v.cpu().numpy().astype(np.float64) - g["C_" + k]).max()) for k, v in (("img", img), ("uvs", dbg["uvs"]), ("colors", dbg["colors"]))}
    print(f"[brush noise case C {mode}] {e}")
    assert e["img"] <= PIX[mode] and e["uvs"] <= PIX[mode] and e["colors"] <= 1e-5


@pytest.mark.parametrize("mode", MODES)
def test_lerp_load_equals_the_host_lerp(dev, mode):
    cfg, G, _, A, _ = nets("s64", mode, dev)
    Bb = buffers(cfg, 78)
    ws, geom, pos = inputs(cfg, 4, dev)
    bn = G.synthesis.brush_noise()
    got, _ = run(G, ws, geom, pos, noise_set=bn.load(A, other={k: torch.from_numpy(v) for k, v in Bb.items()}, alpha=0.3))
    host = {k: A[k] * 0.3 + Bb[k] * (1 - 0.3) for k in A}      # formats.WBrushLibrary.set_interpolated_style's expression
    assert all(v.dtype == np.float32 for v in host.values())
    want, _ = run(G, ws, geom, pos, noise_set=bn.load(host))
    same(got, want, "lerp")
    bn.load(A, other=Bb, alpha=0.3)
    for i, s in enumerate(cfg.layers):
        assert np.array_equal(bn.noise_const[i].cpu().numpy(), host[key_of(s)])
        assert np.array_equal(bn.noise_const_t[i].cpu().numpy(), host[key_of(s)].T)


def test_graph_replays_what_load_wrote_last(dev):
    cfg, G, _, B1, _ = nets("s64", "f8", dev)
    B2 = buffers(cfg, 79)
    ws, geom, pos = inputs(cfg, 4, dev)
    bn = G.synthesis.brush_noise().load(B1)
    call = lambda: G.render_triad(ws=ws, geom_feature=geom, positions=pos, noise_set=bn)      # noqa: E731
    cur = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(cur)
    with torch.cuda.stream(side):                  # workspaces, the set's tables, per-kernel attributes: before the capture
        for _ in range(2):
            first = call()[0].clone()
    cur.wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        u8, _, dbg = call()
    bn.load(B2)                                    # another brush: one launch, no recapture
    graph.replay()
    torch.cuda.synchronize(dev)
    got_u8, got_uvs = u8.clone(), dbg["uvs"].clone()
    want_u8, _, want = call()
    torch.cuda.synchronize(dev)
    assert torch.equal(got_u8, want_u8) and torch.equal(got_uvs, want["uvs"])
    assert not torch.equal(got_u8, first)


def test_errors(dev):
    cfg, G, G2, B, bn = nets("tiny", "f32", dev)
    ws, geom, pos = inputs(cfg, 3, dev)
    with pytest.raises(RuntimeError, match="not a brush noise set of this network"):
        G2.forward_pre_mapped(ws, geom, positions=pos, noise_mode="const", noise_set=bn)
    with pytest.raises(RuntimeError, match="noise_set and noise_buffers"):
        G.forward_pre_mapped(ws, geom, positions=pos, noise_mode="const", noise_set=bn, noise_buffers={k: D(v, dev) for k, v in B.items()})
    with pytest.raises(AssertionError):
        G.synthesis.brush_noise().load({"b8.conv0.noise_const": np.zeros((4, 4), np.float32)})
    # the other noise modes ignore a set, as they ignore noise_buffers
    a = G.forward_pre_mapped(ws, geom, positions=pos, noise_mode="none", noise_set=bn)
    assert torch.equal(a, G.forward_pre_mapped(ws, geom, positions=pos, noise_mode="none"))
    G3 = Generator(cfg, wmod.random_state_dict(cfg, seed=3), conv_mode="f32").to(dev)
    stale = G3.synthesis.brush_noise()
    assert isinstance(stale, BrushNoise)
    G3.load_state_dict(G3.state_dict())
    with pytest.raises(RuntimeError, match="weights were reloaded or moved"):
        G3.forward_pre_mapped(ws, geom, positions=pos, noise_mode="const", noise_set=stale)
    with pytest.raises(RuntimeError, match="weights were reloaded or moved"):
        stale.load(B)
