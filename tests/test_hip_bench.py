"""bench.py's N>1 control flow on a one-GPU box: `python bench.py --gpus 2` must launch its two ranks itself (child
torchrun, one process per rank), gather the RGBA tiles inside the step and print ONE JSON line with n_gpus = 2.
Both ranks share device 0 and the collective backend is gloo (RCCL refuses two ranks on one device); the numbers of
such a run mean nothing -- the test is about the launch path the driver's `--gpus N` run takes.
A plain run measures the headline figure alone; the tests that read what else the benchmark measures run it with --full."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


COMPACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline", "box_calibration", "modes", "detail_file")
ROOFLINE_KEYS = ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "launch_ms", "launches_per_step", "flops_per_launch")
# what only a --full run measures: never in the line or the record of a plain run
FULL_ONLY_KEYS = ("roofline", "box_calibration", "telemetry", "modes", "value_single_stream", "single_stream", "value_fp32_parity",
                  "latency_batch1", "cpu_baseline", "parity")


def _last_line(stdout, full=True):
    """The driver keeps the last 8 KB of stdout and parses its last line: that line must be small and complete."""
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout[-2000:]
    assert stdout.rstrip().splitlines()[-1] == lines[0]
    assert len(lines[0]) < 4096, len(lines[0])
    out = json.loads(lines[0])
    for k in COMPACT_KEYS:
        if full or k not in FULL_ONLY_KEYS:
            assert k in out, k
    if full:
        for k in ROOFLINE_KEYS:
            assert k in out["roofline"], k
    else:
        assert not set(out) & set(FULL_ONLY_KEYS), sorted(set(out) & set(FULL_ONLY_KEYS))
    assert set(out["config"]) >= {"workload", "batch_per_gpu", "resolution"} and "model" not in out["config"]
    return out


def _detail(out):
    with open(os.path.join(REPO, out["detail_file"])) as f:
        return json.load(f)


def _run(args, extra_env=None, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra_env or {})
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, env=env, cwd=REPO, capture_output=True,
                          text=True, timeout=timeout)


def test_bench_self_spawns_two_ranks():
    r = _run(["--gpus", "2", "--steps", "3", "--warmup", "1", "--res", "128", "--batch", "16", "--full", "--no-cpu", "--no-latency"],
             {"NB_BENCH_SHARE_GPU": "1", "NB_BENCH_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-3000:]
    out = _last_line(r.stdout)
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1 and out["scaling"] == "weak"
    assert "gather of RGBA tiles to rank 0" in out["config"]["parallelism"]
    assert out["value"] > 0 and out["roofline"]["frac"] > 0
    # the N > 1 line says who took part and what the gather cost: both ranks seen (one device here: the share-GPU hook), every
    # rank's own step time, and how long rank 0 waited for the tiles
    assert out["rccl"]["world"] == 2 and out["rccl"]["backend"] == "gloo" and out["rccl"]["ranks_seen"] == [0, 1]
    assert [r_["rank"] for r_ in _detail(out)["rccl"]["ranks_seen"]] == [0, 1]
    assert out["rccl"]["distinct_devices"] == 1
    assert len(out["ms_per_step_per_rank"]) == 2 and all(v > 0 for v in out["ms_per_step_per_rank"])
    assert out["gather_wait_ms"]["waits"] >= 3 and out["gather_wait_ms"]["host_ms_per_step"] >= 0
    assert out["box_calibration"]["mfma_f16_sustained_tflops"] > 100
    assert out["streams"] in (1, 3) and out["value_single_stream"] > 0


def test_bench_single_schedule_and_f6_on_request():
    """`--schedule single` is the one-stream loop alone (what the A/B tools and the profiler passes run); `--modes f6` still
    measures the round-5 experiment when asked."""
    r = _run(["--steps", "2", "--warmup", "1", "--res", "128", "--batch", "8", "--full", "--no-latency", "--no-cpu", "--schedule", "single",
              "--modes", "f8,f6"])
    assert r.returncode == 0, r.stderr[-3000:]
    out = _last_line(r.stdout)
    assert set(out["modes"]) == {"f8", "f6"} and "value_single_stream" not in out and "streams" not in out
    assert "one stream" in _detail(out)["schedule"]


def test_bench_line_carries_every_arithmetic_mode():
    """`--full` (N=1) reports all three arithmetic modes in ONE line: each with its own value, dominant-kernel
    roofline against the peak of the type it multiplies in, and a live parity figure against the fp32 CPU oracle; the label of
    a split mode never claims "f32"."""
    r = _run(["--steps", "2", "--warmup", "1", "--res", "128", "--batch", "8", "--full", "--no-latency", "--cpu-seconds", "1"])
    assert r.returncode == 0, r.stderr[-3000:]
    out = _last_line(r.stdout)
    # (f6, the round-5 experiment: only with --modes f6 / all; f16 = the reference's shipped precision, a timing data point)
    assert set(out["modes"]) == {"f8", "h3", "f32", "f16"} and out["conv_mode"] == "f8"
    assert "NOT a parity mode" in out["modes"]["f16"]["note"]
    # the headline is the library's concurrent schedule; the single-stream figure the roofline comes from rides along
    assert out["streams"] in (1, 3) and out["value_single_stream"] > 0 and out["modes"]["h3"]["value_single_stream"] > 0
    assert out["value"] == out["modes"]["f8"]["value"] and out["value_fp32_parity"] == out["modes"]["h3"]["value"]
    assert not out["dtype"].startswith("f32")
    # (f16 is NOT a parity mode: hi x hi products only in the large launches -- which at this test's R=128 / batch 8 are few, hence
    #  the loose bound: the figure that matters is the R=256 one in the driver's line)
    tol = {"f8": 3e-4, "h3": 2e-5, "f32": 2e-5, "f16": 3e-2}
    for m, rec in out["modes"].items():
        assert rec["value"] > 0 and rec["roofline"]["frac"] > 0
        assert rec["roofline"]["peak"] == (157.3 if m == "f32" else 2500.0)
        assert rec["parity"] <= tol[m], (m, rec["parity"])
    assert out["modes"]["f16"]["parity"] >= out["modes"]["f8"]["parity"]
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["kind"] == "port" and out["cpu_baseline"]["cores"] >= 1
    assert out["parity"]["max_abs_rgba_vs_oracle"] <= tol["f8"] and out["parity"]["tolerance"] == 1e-3
    # the full record (tables, per-layer times, explanatory strings) is in the detail file, same numbers
    out_c, out = out, _detail(out)
    assert out["value"] == out_c["value"] and out["roofline"]["frac"] == out_c["roofline"]["frac"]
    assert not out["modes"]["h3"]["dtype"].startswith("f32") and "calibration" in out["roofline"]
    # the box is in the line: what it sustains on a registers-only f16 MFMA loop, and (where the hwmon files are readable) power
    # and shader clock during each mode's timed region
    assert 500 < out["box_calibration"]["mfma_f16_sustained_tflops"] < 2600 and out["box_calibration"]["loop_clock_mhz"] > 500
    for m, rec in out["modes"].items():
        # (means only over >= 20 sampler ticks: the window runs from the mode's burn-in to the end of its last timed region)
        assert "telemetry" in rec and ("power_w_mean" in rec["telemetry"] or rec["telemetry"]["samples"] < 20)
        assert "single-stream" in rec["schedule"] or "in flight" in rec["schedule"]
        assert rec["single_stream"]["ms_per_step"] > 0 and "SINGLE-STREAM" in rec["roofline"]["note"]
        if m != "f32":
            assert 0 < rec["roofline"]["frac_of_sustained"] < 1


def test_bench_fails_nonzero_when_a_rank_dies():
    """A failing child must surface as a non-zero exit code of `python bench.py --gpus N`, with no JSON line."""
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--res", "128", "--batch", "16", "--no-cpu", "--no-latency"],
             {"NB_BENCH_SHARE_GPU": "1", "NB_BENCH_BACKEND": "gloo", "NB_BENCH_FAIL_RANK": "1"}, timeout=600)
    assert r.returncode != 0
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_train_bench_two_ranks_gradient_all_reduce():
    """BASELINE config 5's data-parallel step with its N>1 launch path on a one-GPU box: `tools/bench_train.py --gpus 2`
    launches two ranks itself; every optimiser step is preceded by the all-reduce of the flattened gradients (gloo here,
    RCCL on a multi-GPU node), incl. the path-length, R1 and forger geometry phases."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update({"NB_BENCH_SHARE_GPU": "1", "NB_BENCH_BACKEND": "gloo"})
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "bench_train.py"), "--gpus", "2", "--res", "128", "--batch", "2",
                        "--iters", "4", "--warmup", "1", "--geom-interval", "2"], env=env, cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["value"] > 0 and "all-reduce" in out["config"]["parallelism"]


def test_bench_dumps_the_last_timed_step(tmp_path):
    """`--dump-outputs DIR` writes what the headline leg's last timed step returned -- the primary mode's uint8 RGBA tiles, in float32 --
    and `--steps` sets the timed steps.  The tiles are the ones Generator.render_triad gives for the seeded weights and inputs of
    bench.py (rank 0), bit for bit."""
    import numpy as np
    r = _run(["--steps", "3", "--warmup", "1", "--res", "128", "--batch", "8", "--full", "--no-latency", "--no-cpu", "--modes", "primary",
              "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-3000:]
    out = _last_line(r.stdout)
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    got = np.load(tmp_path / "rgba_u8.npy")
    assert got.dtype == np.float32 and got.shape == (8, 128, 128, 4) and os.listdir(tmp_path) == ["rgba_u8.npy"]
    assert np.array_equal(got, _rendered_tiles(out["conv_mode"], 128, 8))


def test_plain_run_measures_the_headline_alone(tmp_path):
    """Without --full the run sets up, warms up, times the K steps on the library's throughput schedule and prints the line: the
    contract's keys, none of the figures of a --full run (in the line or in the detail record), and --dump-outputs writes the
    same tiles as Generator.render_triad gives for bench.py's seeded weights and inputs (rank 0), bit for bit."""
    import numpy as np
    r = _run(["--steps", "3", "--warmup", "1", "--res", "128", "--batch", "8", "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-3000:]
    out = _last_line(r.stdout, full=False)
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["higher_is_better"] is True and out["conv_mode"] == "f8" and not out["dtype"].startswith("f32")
    assert abs(out["value"] - 8 / (out["ms_per_step"] * 1e-3)) <= 1e-3 * out["value"]
    assert out["streams"] in (1, 3)
    detail = _detail(out)
    assert not set(detail) & set(FULL_ONLY_KEYS), sorted(set(detail) & set(FULL_ONLY_KEYS))
    assert "in flight" in detail["schedule"] and detail["value"] == out["value"]
    got = np.load(tmp_path / "rgba_u8.npy")
    assert got.dtype == np.float32 and got.shape == (8, 128, 128, 4) and os.listdir(tmp_path) == ["rgba_u8.npy"]
    assert np.array_equal(got, _rendered_tiles(out["conv_mode"], 128, 8))


def _rendered_tiles(conv_mode, res, batch):
    """The uint8 RGBA tiles of bench.py's rank-0 batch (seeded weights and inputs) through Generator.render_triad, as float32."""
    import torch
    from brushstroke_engine_amd import config as cfgmod, synthetic, weights as wmod
    from brushstroke_engine_amd.networks import Generator
    cfg, dev = cfgmod.style1_config(res), torch.device("cuda:0")
    G = Generator(cfg, wmod.random_state_dict(cfg, seed=0), conv_mode=conv_mode).to(dev)
    u8 = G.render_triad(z=torch.from_numpy(synthetic.batch_z(cfg, batch, first_seed=0)).to(dev).to(torch.float32),
                        geom_feature=[torch.from_numpy(g).to(dev) for g in synthetic.geom_features(cfg, batch, seed=0)],
                        positions=torch.from_numpy(synthetic.positions(cfg, batch, seed=0)).to(dev), render_mode="clear")[0]
    return u8.cpu().numpy().astype("float32")
