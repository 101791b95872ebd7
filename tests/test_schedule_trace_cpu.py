"""The painting schedule as a TRACE (CPU, no generator): which device operations ``PaintingHelper`` asks for, in which order, on which
stream, with which workspace slot -- and what comes out -- against ``tests/golden/schedule_trace.json``, which was recorded with the
``_schedule`` that was ONE 190-line method (the commit before it became a list of phases).  The fixture is data of this project's own
code; it is never regenerated from the code under test: a difference here means that the schedule changed.

The stand-in records every call and computes tiles that are a fixed function of each tile's position and geometry, so a batch routed
to the wrong tiles, a strip cut from the wrong place or pieces replayed in another order change the hashes as well as the call list.
It runs with ``n_streams = 2`` and ``stream_policy = 2``: the multi-stream branch of the schedule is the one exercised.

Shapes: patch width 32, batch 4, crop margin 5, 3 x 3 tiles at stride 22 (neighbours overlap by 10 px = 5 cells of the level-2 feature
canvas) on a 76 x 76 canvas.  ``feature_blending_margin`` is 4 here (the product's 16 leaves no interior in a 16-cell tile)."""
import contextlib
import hashlib
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLDEN, REPO
from brushstroke_engine_amd import painting
from oracle_tile_ops import sequential_replay, sequential_replay_pieces

R, BATCH, CROP, STRIDE, CANVAS, CHANNELS = 32, 4, 5, 22, 76, 4
CROPS = [(r * STRIDE, c * STRIDE) for r in range(3) for c in range(3)]


class _Cfg:
    @staticmethod
    def channels(res):
        return CHANNELS


class RecordingOps(painting.TileOpsBase):
    """Every scheduling hook and device operation of ``TileOps``, recorded: [method, stream tag, slot, batch size, first tile position]
    (+ what else the call was given).  The stream tag is ``caller``, the ``k`` of the ``stream(k)`` in force, or ``comm``."""
    n_streams = 2
    stream_policy = 2
    cfg = _Cfg()
    patch_width = R
    device = torch.device("cpu")

    def __init__(self):
        self.calls, self.pieces, self._tag = [], [], "caller"

    def _rec(self, method, slot=None, n=None, pos=None, **extra):
        first = None if pos is None or len(pos) == 0 else [int(v) for v in pos[0].tolist()]
        self.calls.append([method, self._tag, slot, n, first] + ([extra] if extra else []))

    @contextlib.contextmanager
    def _tagged(self, name, tag):
        self._rec(name + ".enter", k=tag)
        prev, self._tag = self._tag, tag
        try:
            yield
        finally:
            self._tag = prev
            self._rec(name + ".exit", k=tag)

    # -- scheduling hooks --
    def stream(self, k):
        return self._tagged("stream", k)

    def comm_stream(self):
        return self._tagged("comm_stream", "comm")

    def join_streams(self, tensors=()):
        self._rec("join_streams", n=len(tensors))

    def join_comm(self, tensors=()):
        self._rec("join_comm", n=len(tensors))

    def prepare(self, n, slots):
        self._rec("prepare", n=n, slots=list(slots))

    def choose_streams(self, n, render_mode="clear"):
        self._rec("choose_streams", n=n, render_mode=render_mode)

    # -- inputs --
    def to_device(self, a):
        return torch.from_numpy(np.ascontiguousarray(a))

    def map_style(self, z=None, ws=None):
        return ws.to(torch.float32)

    def geom_tiles(self, geom, tile_yx):
        self._rec("geom_tiles", n=tile_yx.shape[0], pos=tile_yx)
        return torch.stack([geom[y:y + R, x:x + R].to(torch.float32)[None] / 255 for y, x in tile_yx.tolist()])

    def encode(self, geom):
        self._rec("encode", n=geom.shape[0])
        return [geom]

    # -- generator stubs: exact small integers and quarters, a fixed function of the tile's position, the channel and its geometry --
    @staticmethod
    def _features(ws, geom_feats, positions, res):
        n, g = ws.shape[0], geom_feats[0]
        assert g.shape[0] == n and positions.shape == (n, 2)
        pooled = torch.nn.functional.avg_pool2d(g, R // res) if res < R else g
        yy, xx = torch.meshgrid(torch.arange(res), torch.arange(res), indexing="ij")
        out = torch.empty([n, CHANNELS, res, res], dtype=torch.float32)
        for i, (py, px) in enumerate(positions.tolist()):
            for c in range(CHANNELS):
                out[i, c] = ((py * 7 + px * 3 + c * 11 + yy * 5 + xx) % 61).to(torch.float32) + pooled[i, 0] + ws[i, 0, 0]
        return out

    @staticmethod
    def _rgba(feats, positions, user_colors):
        up = feats.repeat_interleave(R // feats.shape[-1], 2).repeat_interleave(R // feats.shape[-1], 3)
        shift = torch.tensor([py + 2 * px for py, px in positions.tolist()], dtype=torch.float32).view(-1, 1, 1, 1)
        if user_colors is not None:
            shift = shift + torch.round(torch.nan_to_num(user_colors, nan=0.0).sum(dim=(1, 2)) * 255).view(-1, 1, 1, 1)
        return (torch.floor(up * 4 + shift).to(torch.int64) % 256).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    def head(self, ws, geom_feats, positions, stop_res, slot=0):
        self._rec("head", slot=slot, n=ws.shape[0], pos=positions, res=stop_res)
        return self._features(ws, geom_feats, positions, stop_res)

    def tail(self, ws, feats, geom_feats, positions, resume_res, render_mode, user_colors, sfactor=None, slot=0):
        self._rec("tail", slot=slot, n=ws.shape[0], pos=positions, res=resume_res, render_mode=render_mode)
        assert feats.shape[0] == ws.shape[0] == geom_feats[0].shape[0] and sfactor is None
        return self._rgba(feats + geom_feats[0][:, :, :resume_res, :resume_res], positions, user_colors)

    def full(self, ws, geom_feats, positions, render_mode, user_colors, sfactor=None, slot=0):
        self._rec("full", slot=slot, n=ws.shape[0], pos=positions, render_mode=render_mode)
        return self._rgba(self._features(ws, geom_feats, positions, R), positions, user_colors)

    # -- canvas --
    def new_feature_canvas(self, c, hc, wc):
        self._rec("new_feature_canvas", shape=[c, hc, wc])
        return torch.zeros([1, c, hc, wc]), torch.zeros([hc, wc], dtype=torch.uint8)

    def replay(self, tiles, tile_yx, alpha0, crop, canvas, mask, cell_off, cell_tiles, box=None):
        self._rec("replay", n=tiles.shape[0], pos=tile_yx, crop=crop, box=None if box is None else [int(v) for v in box])
        return sequential_replay(tiles, tile_yx, alpha0, crop, canvas, mask)

    def replay_pieces(self, pieces, hw, alpha0, crop, canvas, mask, cell_off, cell_pieces, box):
        self._rec("replay_pieces", n=len(pieces), crop=crop, box=[int(v) for v in box])
        # (tile origin on the feature canvas -> tile index: origins are distinct on the 3 x 3 grid)
        origin = {(y // 2, x // 2): i for i, (y, x) in enumerate(CROPS)}
        self.pieces.append([[origin.get((cy - ly0, cx - lx0)), [cy, cx, cy + v.shape[1], cx + v.shape[2]], [ly0, lx0]]
                            for v, cy, cx, ly0, lx0 in ((p[0], *(int(a) for a in p[1:])) for p in pieces)])
        return sequential_replay_pieces(pieces, hw, alpha0, crop, canvas, mask)

    def paste(self, canvas_u8, tiles_u8, dst_yx, crop, cell_off, cell_tiles):
        self._rec("paste", n=tiles_u8.shape[0], pos=dst_yx, crop=crop)
        r = tiles_u8.shape[1]
        for t, (y, x) in enumerate(dst_yx.tolist()):
            canvas_u8[y + crop:y + r - crop, x + crop:x + r - crop] = tiles_u8[t, crop:r - crop, crop:r - crop]


def _sha(t):
    return None if t is None else hashlib.sha256(np.ascontiguousarray(t.numpy() if torch.is_tensor(t) else t).tobytes()).hexdigest()


def _geometry(size=CANVAS, seed=3):
    return ((np.random.RandomState(seed).rand(size, size) > 0.3) * 255).astype(np.uint8)


def _opts(seed=0):
    opts = painting.GanBrushOptions(primary_color=np.array([10, 20, 30], np.uint8))
    opts.set_style_w(torch.full([1, 1, 2], float(seed)), style_id=seed)
    return opts


def _helper(ops, level, size=CANVAS):
    helper = painting.PaintingHelper(ops, batch=BATCH)
    helper.feature_blending_margin = 4
    helper.make_new_canvas(size, size, feature_blending=level)
    return helper


def _trace(ops, helper, rgba):
    """The trace of the calls since the last one: the stand-in's records, emptied."""
    tr = {"calls": ops.calls, "rgba": _sha(rgba), "features": _sha(helper.features), "mask": _sha(helper.mask),
          "halo_bytes": helper.halo_bytes, "pieces": ops.pieces}
    ops.calls, ops.pieces = [], []
    return tr


def _render_tiles_case(ops, helper, crops, seed=0):
    ops_canvas = helper.render_tiles(_geometry(), crops, _opts(seed), crop_margin=CROP)
    return _trace(ops, helper, ops_canvas)


def _single_process_cases():
    out = {}
    ops = RecordingOps()
    for level in (0, 2):                              # 9 tiles in batches of 4, 4 and 1
        out[f"level{level}"] = _render_tiles_case(ops, _helper(ops, level), CROPS)
    # one tile through render_stroke on a 128 x 128 canvas: the single-batch rule and the replay box
    helper = _helper(ops, 2, size=128)
    stroke = np.zeros((R, R, 1), np.uint8)
    stroke[8:20, 4:28] = 255
    opts = _opts(1)
    opts.set_position(37, 53)
    img, _, where = helper.render_stroke(stroke, None, opts, meta={"x": 37, "y": 53, "crop_margin": CROP})
    out["render_stroke"] = dict(_trace(ops, helper, img), where=where)
    return out


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo_worker(rank, world, port, tmp):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    torch.set_num_threads(2)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out = {}
        ops = RecordingOps()
        helper = _helper(ops, 2)
        if world == 2:
            # rank 0 owns 5 tiles in two batches, rank 1 owns 4 (the single-batch rule); then a second sharded call on the same canvas
            # (the lazy sync_canvas); then one tile over two ranks (rank 1 owns nothing and still joins the exchange and the gather)
            out["world2"] = _render_tiles_case(ops, helper, CROPS)
            out["world2_second_call"] = _render_tiles_case(ops, helper, CROPS[2:7], seed=2)
            out["world2_one_tile"] = _render_tiles_case(ops, _helper(ops, 2), CROPS[4:5])
        else:                                         # NB_FORCE_PG=1 at world size 1: the strip sent to myself
            out["force_pg_world1"] = _render_tiles_case(ops, helper, CROPS)
        with open(os.path.join(tmp, f"trace_w{world}_r{rank}.json"), "w") as f:
            json.dump(out, f)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _gloo_cases(tmp, world):
    mp.spawn(_gloo_worker, args=(world, _free_port(), str(tmp)), nprocs=world, join=True)
    per_rank = [json.load(open(os.path.join(tmp, f"trace_w{world}_r{r}.json"))) for r in range(world)]
    return {name: {f"rank{r}": per_rank[r][name] for r in range(world)} for name in per_rank[0]}


def collect_traces(tmp):
    """Every case's trace, as the fixture holds them (through JSON, so that tuples and lists compare alike)."""
    out = _single_process_cases()
    out.update(_gloo_cases(tmp, 2))
    prev = os.environ.get("NB_FORCE_PG")
    os.environ["NB_FORCE_PG"] = "1"                   # (the spawned rank inherits it)
    try:
        out.update(_gloo_cases(tmp, 1))
    finally:
        if prev is None:
            del os.environ["NB_FORCE_PG"]
        else:
            os.environ["NB_FORCE_PG"] = prev
    return json.loads(json.dumps(out))


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    return collect_traces(tmp_path_factory.mktemp("schedule_trace"))


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "schedule_trace.json")) as f:
        return json.load(f)


def _assert_same(got, want, where):
    if isinstance(want, dict) and "calls" in want:
        assert sorted(got) == sorted(want), where
        for field in want:
            if field != "calls":
                assert got[field] == want[field], f"{where}: {field}"
        for i, (a, b) in enumerate(zip(got["calls"], want["calls"])):
            assert a == b, f"{where}: call {i} is {a}, recorded {b}"
        assert len(got["calls"]) == len(want["calls"]), f"{where}: {len(got['calls'])} calls, recorded {len(want['calls'])}"
    else:
        assert sorted(got) == sorted(want), where
        for k in want:
            _assert_same(got[k], want[k], f"{where}/{k}")


CASES = ["level0", "level2", "render_stroke", "world2", "world2_second_call", "world2_one_tile", "force_pg_world1"]


def test_the_fixture_holds_these_cases(recorded):
    assert sorted(recorded) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_schedule_trace_is_the_recorded_one(traces, recorded, case):
    _assert_same(traces[case], recorded[case], case)


def test_the_cases_reach_the_branches_they_are_there_for(recorded):
    """What each case is in the fixture for, read from the RECORDED traces (so the fixture cannot quietly stop covering it)."""
    methods = lambda tr: [c[0] for c in tr["calls"]]
    lvl2 = recorded["level2"]
    heads = [c for c in lvl2["calls"] if c[0] == "head"]
    assert [c[3] for c in heads] == [1, 4, 4] and [c[1] for c in heads] == [2, 1, 0]          # phase 1 last-to-first, ragged batch
    assert [c[2] for c in heads] == [painting.PAINT_SLOT0 + k % 2 for k in (2, 1, 0)]
    assert "prepare" in methods(lvl2) and "choose_streams" in methods(lvl2)
    assert [c[3] for c in recorded["level0"]["calls"] if c[0] == "full"] == [4, 4, 1]
    stroke = recorded["render_stroke"]
    assert "prepare" not in methods(stroke) and "stream.enter" not in methods(stroke)          # the single-batch rule
    assert [c[2] for c in stroke["calls"] if c[0] in ("head", "tail")] == [0, 0]
    assert [c[5]["box"] for c in stroke["calls"] if c[0] == "replay"][0] is not None            # the replay box
    w2 = recorded["world2"]
    assert "prepare" in methods(w2["rank0"]) and "prepare" not in methods(w2["rank1"])
    assert w2["rank0"]["halo_bytes"]["sent"] == w2["rank1"]["halo_bytes"]["received"] > 0
    assert any(p[0] is not None and p[0] < 5 for p in w2["rank1"]["pieces"][0])                 # strips of rank 0's tiles
    one = recorded["world2_one_tile"]["rank1"]
    assert "comm_stream.enter" in methods(one) and "head" not in methods(one) and one["rgba"] is None
    assert recorded["force_pg_world1"]["rank0"]["halo_bytes"] == {"sent": 4 * CHANNELS * 16 * 16, "received": 4 * CHANNELS * 16 * 16}
