"""bench.py's final stdout line (CPU-side check of the reduction): the driver keeps the last 8 KB of stdout, and round 4's 20 KB line
left its record unparseable.  The compact form of a real full record must stay under 4 KB -- also with eight ranks in it -- and carry
the contract's keys."""
import copy
import importlib.util
import json
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_compact_line_of_a_full_record_is_small_and_complete():
    b = _bench()
    full = json.load(open(os.path.join(REPO, "profiles", "r04_bench.json")))       # a full one-GPU record (20 KB)
    assert len(json.dumps(full)) > 15000
    c = b.compact_line(full)
    line = json.dumps(c, separators=(",", ":"))
    assert len(line) < b.MAX_LINE_BYTES
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "parity", "box_calibration", "telemetry", "latency_batch1", "modes"):
        assert k in c, k
    assert c["value"] == full["value"] and c["ms_per_step"] == full["ms_per_step"]
    r = c["roofline"]
    for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "launch_ms", "launches_per_step", "flops_per_launch"):
        assert k in r, k
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert set(c["cpu_baseline"]) >= {"value", "unit", "cores", "kind", "sample"}
    assert set(c["modes"]) == {"f8", "h3", "f32"}                     # (the round-4 record; round 5 adds "f6")
    assert not any(isinstance(v, str) and len(v) > 200 for v in c.values())


def test_compact_line_with_eight_ranks():
    b = _bench()
    full = copy.deepcopy(json.load(open(os.path.join(REPO, "profiles", "r04_bench.json"))))
    full["n_gpus"] = 8
    full["rccl"] = {"world": 8, "backend": "nccl", "nccl_version": "2.22.3", "distinct_devices": 8,
                    "ranks_seen": [{"rank": i, "host": "node-with-a-long-name-0123456789", "pid": 100000 + i, "device": i,
                                    "pci_bus_id": f"0000:{i:02x}:00.0", "uuid": "GPU-" + "ab" * 16} for i in range(8)]}
    full["ms_per_step_per_rank"] = [1.8321] * 8
    full["gather_wait_ms"] = {"host_ms_per_step": 0.0123, "stream_ms_per_step": 0.0456, "waits": 160, "what": "x" * 400}
    full["modes"] = {"f8": full["modes"]["f8"]}
    c = b.compact_line(full)
    line = json.dumps(c, separators=(",", ":"))
    assert len(line) < b.MAX_LINE_BYTES
    assert c["rccl"]["ranks_seen"] == list(range(8)) and c["rccl"]["distinct_devices"] == 8
    assert len(c["ms_per_step_per_rank"]) == 8 and c["gather_wait_ms"]["waits"] == 160


def test_fit_line_degrades_instead_of_failing():
    """A record whose compact form would not fit the 4 KB the driver's tail keeps is reduced key by key -- least important first -- and
    ALWAYS printed (round 5 asserted instead: a finished measurement without its line, and at N > 1 the other ranks left in the
    closing barrier)."""
    b = _bench()
    full = copy.deepcopy(json.load(open(os.path.join(REPO, "profiles", "r04_bench.json"))))
    c = b.compact_line(full)
    line = b.fit_line(copy.deepcopy(c))
    assert len(line) < b.MAX_LINE_BYTES and "dropped" not in json.loads(line)          # fits: nothing dropped
    # sixty-four ranks with long kernel names in every mode: far too long
    c["ms_per_step_per_rank"] = [1.83217] * 64
    c["rccl"] = {"world": 64, "backend": "RCCL (torch backend nccl)", "nccl_version": "2.26.6", "distinct_devices": 64, "ranks_seen": list(range(64))}
    for m in c["modes"].values():
        m["roofline"]["kernel"] = "modconv3x3_up2v_kernel<true, 2, false, false>" * 12
    c["roofline"]["kernel"] = "k" * 300
    line = b.fit_line(copy.deepcopy(c))
    out = json.loads(line)
    assert len(line) < b.MAX_LINE_BYTES and out["dropped"]
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in out, k
    assert out["value"] == c["value"]
    # even a pathological record ends as one parseable line with the contract's scalar keys
    c["config"]["workload"] = "w" * 5000
    out = json.loads(b.fit_line(copy.deepcopy(c)))
    assert out["value"] == c["value"] and out["metric"] == c["metric"] and "dropped" in out


def test_debug_env_names_map_onto_declared_setters():
    """tools/nb_debug_env.py (the developer switches of the A/B scripts; the library itself reads no environment variable since round 6)
    only names setters that include/neube_hip_debug.h declares, and no csrc source calls getenv."""
    import importlib.util
    import re
    spec = importlib.util.spec_from_file_location("nb_debug_env", os.path.join(REPO, "tools", "nb_debug_env.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    hdr = open(os.path.join(REPO, "include", "neube_hip_debug.h")).read()
    declared = set(re.findall(r"\bvoid (nb_debug_[a-z0-9_]+)\s*\(int ", hdr))
    assert len(m.SWITCHES) >= 12
    for var, (setter, _) in m.SWITCHES.items():
        assert var.startswith("NB_") and setter in declared, (var, setter)
    csrc = os.path.join(REPO, "brushstroke_engine_amd", "csrc")
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h")):
            assert "getenv" not in open(os.path.join(csrc, f)).read(), f


def test_dump_outputs_writes_float32_within_the_limit(tmp_path):
    """--dump-outputs: the whole output in float32 while it fits, else the same seeded sample of patches on every run, with the indices
    taken; all files together within the limit."""
    import numpy as np
    b = _bench()
    tiles = np.random.RandomState(3).randint(0, 256, (6, 16, 16, 4)).astype(np.uint8)
    assert b.dump_outputs(str(tmp_path / "all"), {"rgba_u8": tiles}) == {"rgba_u8.npy": [6, 16, 16, 4]}
    got = np.load(tmp_path / "all" / "rgba_u8.npy")
    assert got.dtype == np.float32 and np.array_equal(got, tiles)
    limit = 2 * b.NPY_HEADER_BYTES + 3 * (16 * 16 * 4 * 4 + 8)              # room for three of the six patches
    for run in ("a", "b"):
        files = b.dump_outputs(str(tmp_path / run), {"rgba_u8": tiles}, limit=limit)
        assert files == {"rgba_u8.npy": [3, 16, 16, 4], "rgba_u8_index.npy": [3]}
        assert sum(os.path.getsize(tmp_path / run / f) for f in files) <= limit
    idx = np.load(tmp_path / "a" / "rgba_u8_index.npy")
    assert idx.dtype == np.float64 and list(idx) == sorted(set(idx)) and np.array_equal(idx, np.load(tmp_path / "b" / "rgba_u8_index.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "rgba_u8.npy"), tiles[idx.astype(int)])


def test_full_is_off_by_default_and_other_modes_need_it():
    """A plain run measures the headline figure alone; what else the benchmark measures -- other arithmetic modes among it -- is behind
    --full, and a plain run asked for other modes fails at once instead of ignoring the request."""
    import pytest
    b = _bench()
    assert b.parse_args([]).full is False
    assert b.parse_args(["--full"]).full is True
    assert b.parse_args(["--modes", "primary"]).modes == "primary"
    assert b.parse_args(["--full", "--modes", "f8,h3"]).modes == "f8,h3"
    with pytest.raises(SystemExit) as e:
        b.parse_args(["--modes", "f8,h3"])
    assert e.value.code == 2


def test_compact_line_of_a_plain_record():
    """The record of a plain run has none of the --full figures: its compact line carries the contract's keys and nothing made up for
    the figures it lacks."""
    b = _bench()
    full = json.load(open(os.path.join(REPO, "profiles", "r04_bench.json")))
    only_full = ("roofline", "box_calibration", "telemetry", "modes", "value_single_stream", "single_stream", "value_fp32_parity",
                 "value_fp32_parity_what", "latency_batch1", "cpu_baseline")
    plain = {k: v for k, v in full.items() if k not in only_full}
    c = b.compact_line(copy.deepcopy(plain))
    out = json.loads(b.fit_line(c))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config"):
        assert k in out, k
    assert out["value"] == full["value"] and out["ms_per_step"] == full["ms_per_step"] and "dropped" not in out
    assert not set(out) & set(only_full + ("parity",)), sorted(set(out) & set(only_full))
