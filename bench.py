"""Headline benchmark: stylized 256x256 stroke patches / second at batch 32 on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--res 256] [--batch 32] [--dump-outputs DIR] [--full [--no-cpu] ...]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Started without a torchrun environment and --gpus N > 1, it launches the N ranks itself (one process per GPU through
``python -m torch.distributed.run`` as a CHILD process, before anything in this process touches the GPU -- the
reference's counterpart is ``torch.multiprocessing.spawn`` per GPU + ``init_process_group('nccl')`` in
thirdparty/stylegan2_ada_pytorch/train.py:811-816, 523-530) and exits with the child's exit code.

A step = one pass of the hot path (mapping -> styles/noise -> 15 fused modulated-conv launches ->
fused ToRGB/softmax/triad + paint-engine compositing to uint8 RGBA) over one batch of 32 synthetic
patches per GPU (BASELINE.json configs[1]: random z, random stroke-geometry features, random patch
positions, style1 checkpoint shapes at R=256, fp32).  Inputs are resident in HBM before the timed
region.  With N > 1 every rank renders its own batch (weak scaling, replicated weights) and the
uint8 RGBA tiles are gathered to rank 0 over RCCL inside the step, overlapped with the next batch.

Prints ONE JSON line on rank 0.  Top level = the PRIMARY arithmetic mode (the library default, `f8`): `value`,
`ms_per_step`, `dtype` (what multiplies; never "f32" for a split mode).  A plain run does only what that figure needs:
it sets up, probes the stream count of the concurrent schedule, burns in and warms up, times the K steps and prints the
line.

--full adds everything else the benchmark measures or checks, in the same process: the registers-only MFMA calibration
of the board and its power / clock telemetry; per mode, the same K steps back to back on ONE stream (`value_single_stream`)
with `roofline` (dominant kernel: algorithmic FLOPs / HIP-event time on the launch stream, against the dense MFMA peak of
the type that kernel MULTIPLIES in -- MI355X_MICROARCH.md).  At N=1 it then measures the other modes the same way (own
Generator, same W warm-up + K timed steps) and reports them under `modes` = {"f8": .., "h3": .., "f32": .., "f16": ..},
each with value / ms_per_step / roofline / live parity against the fp32 CPU oracle; `value_fp32_parity` = the `h3`
number (SURVEY 8d's "fp32 parity mode": products to ~2^-22); `latency_batch1` = one patch through the hipGraph-captured
step; `cpu_baseline` = the CPU oracle (port of the reference path) timed on this box's host cores on a bounded sample.

--dump-outputs DIR writes what the headline leg's last timed step returned to its caller -- the uint8 RGBA tiles of the
primary mode, rank 0's batch -- as DIR/rgba_u8.npy in float32 (see dump_outputs), with or without --full.  Weights and
inputs are seeded, so two builds run with the same arguments can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np
import torch
import torch.distributed as dist

PEAK_F32_MATRIX_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2/16x16x4, 64 FLOP/clk/SIMD (spec)
PEAK_F16_MATRIX_TFLOPS = 2500.0     # MI355X_MICROARCH.md: dense f16/bf16 MFMA (spec, no sparsity); the split-f16 kernels
                                    # execute 3 (h3) or the time-equivalent of 2 (f8) MFMA FLOPs per algorithmic FLOP
PEAK_FP8_MATRIX_TFLOPS = 5000.0     # dense fp8 MFMA (same guide)
PEAK_HBM_GBPS = 8000.0              # HBM3E (same guide)


def layer_flops(spec, batch):
    """Algorithmic FLOPs of one modulated-conv launch (2 x MACs; up-layers at their
    non-zero transposed-conv MACs + the 4x4 FIR)."""
    if spec.up == 2:
        macs = spec.in_res ** 2 * spec.out_channels * spec.in_channels * 9 + spec.block_res ** 2 * spec.out_channels * 16
    else:
        macs = spec.block_res ** 2 * spec.out_channels * spec.in_channels * 9
    return 2.0 * macs * batch


def is_split_kernel(kname):
    """Kernels that multiply in f16 (+ fp8 corrections): the split-f16 family, incl. the two re-tiled up=2 kernels of round 4."""
    return "_h3_" in kname or "up2v_kernel" in kname


def kernel_label(spec):
    return f"modconv3x3_up{spec.up}[{spec.in_channels}->{spec.out_channels}@{spec.block_res}]"


def cpu_baseline(cfg, sd, seconds_budget=12.0, n_sample=8, threads=16, gens=None, dev=None):
    """The CPU oracle (oracle/neube_oracle.py, a port of the reference path onto plain torch CPU ops, fused
    modulated conv = the reference's eval-mode fp32 default) timed on this box's host cores.  Bounded
    sample: `n_sample` patches per pass, repeated until ~seconds_budget of CPU time is spent.  16 threads:
    measured on the MI355X host (256 logical CPUs) the oracle peaks at 16 torch threads (8: 5.7, 16: 6.1,
    32: 4.9, 64: 2.5, 128: 1.6 patches/s; tools/cpu_threads_scan.py).  A reported baseline, not the target."""
    from oracle import neube_oracle as orc
    from brushstroke_engine_amd import synthetic
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    torch.set_num_threads(max(1, min(threads, avail)))
    O = orc.OracleGenerator(cfg, sd)
    z = synthetic.batch_z(cfg, n_sample, 0)
    geom = synthetic.geom_features(cfg, n_sample, seed=0)
    pos = synthetic.positions(cfg, n_sample, seed=0)

    last = {}

    def one():
        img, dbg = O(z, None, geom, positions=pos, return_debug_data=True)
        last["rgba"] = orc.triad_composite(dbg["uvs"], dbg["colors"], "clear")
        last["uvs"] = dbg["uvs"]
        return orc.rgba_to_uint8(last["rgba"])

    u8_ref = one()                          # warm-up (thread pool, allocator)
    t0 = time.perf_counter()
    reps = 0
    while True:
        one()
        reps += 1
        el = time.perf_counter() - t0
        if el >= seconds_budget or reps >= 50:
            break
    out = {"value": round(reps * n_sample / el, 3), "unit": "patches/s", "cores": torch.get_num_threads(), "kind": "port",
           "sample": f"{reps} passes of batch {n_sample} at {cfg.img_resolution}x{cfg.img_resolution} "
                     f"(oracle = torch-CPU port of the reference generator + compositing, fp32, {el:.1f} s, "
                     f"{torch.get_num_threads()} of {avail} host CPUs)"}
    # the oracle as the checker: the same sample through every benchmarked HIP generator (one per arithmetic mode), compared
    # with the oracle's fp32 result at the full 256x256 size
    to_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    out["parity_by_mode"] = {}
    for mode, G in (gens or {}).items():
        u8, rgba, dbg = G.render_triad(z=torch.from_numpy(z).to(dev), geom_feature=[torch.from_numpy(g).to(dev) for g in geom],
                                       positions=torch.from_numpy(pos).to(dev), render_mode="clear", want_f32=True)
        torch.cuda.synchronize()
        out["parity_by_mode"][mode] = {
            "max_abs_rgba_vs_oracle": float(np.abs(to_np(rgba) - to_np(last["rgba"])).max()),
            "max_abs_uvs_vs_oracle": float(np.abs(to_np(dbg["uvs"]) - to_np(last["uvs"])).max()),
            "max_u8_diff": int(np.abs(to_np(u8).astype(np.int32) - to_np(u8_ref).transpose(0, 2, 3, 1).astype(np.int32)).max()),
            "tolerance": 1e-3, "patches": n_sample,
            "what": f"HIP generator in mode {mode} vs the fp32 CPU oracle on the cpu_baseline sample"}
    return out


def latency_batch1(G, cfg, dev, geom, pos, iters=300):
    """BASELINE.json config 4 / second half of the metric: per-stroke latency of ONE patch through the
    hipGraph-captured generator step (inputs on device -> uint8 RGBA on device), wall-clock per replay
    including the launch and a stream sync, plus the D2H copy of the tile measured separately."""
    from brushstroke_engine_amd.graphed import GraphedTriadRender
    gr = GraphedTriadRender(G, batch=1)
    gr.set_inputs(z=torch.randn(1, cfg.z_dim, device=dev), geom_feature=[g[:1] for g in geom], positions=pos[:1])
    for _ in range(20):
        gr.replay()
    torch.cuda.synchronize()
    ts, ts_d2h = [], []
    host = torch.empty_like(gr.out_u8, device="cpu").pin_memory()
    for i in range(iters):
        t0 = time.perf_counter()
        gr.replay()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        host.copy_(gr.out_u8, non_blocking=True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ts.append((t1 - t0) * 1e3)
        ts_d2h.append((t2 - t0) * 1e3)
    q = lambda a, p: round(float(np.percentile(a, p)), 4)
    return {"unit": "ms", "p50": q(ts, 50), "p99": q(ts, 99), "mean": round(float(np.mean(ts)), 4),
            "p50_incl_d2h": q(ts_d2h, 50), "p99_incl_d2h": q(ts_d2h, 99), "iters": iters,
            "what": "batch=1 256x256 patch, hipGraph replay of the whole generator step (mapping ... fused ToRGB) + stream sync"}


MODE_DTYPE = {
    # what MULTIPLIES in the conv layers of each arithmetic mode (accumulation is fp32 in all three); never a precision claim
    "f32": "f32 x f32 MFMA (v_mfma_f32_32x32x2_f32 / 16x16x4_f32), fp32 accumulate: exact fp32 products",
    "h3": "f16 x f16 MFMA, three per fp32 product on hi/lo-split operands (xh*wh + xl*wh + xh*wl), fp32 accumulate: ~2^-22 "
          "relative per product, ~5e-6 from an all-fp32 evaluation on pixels",
    "f8": "f16 hi x f16 hi MFMA + 2 block-scaled fp8 (e4m3) correction products per fp32 product, fp32 accumulate: ~2^-15 relative "
          "per product, ~1e-4 from an all-fp32 evaluation on pixels (north_star budget 1e-3)",
    "f16": "f16 hi x f16 hi MFMA only in the four large launches (the f8 mode with its correction products skipped): plain single-f16 products, "
           "1.5e-3 ... 3e-3 from an all-fp32 evaluation on pixels -- OUTSIDE the 1e-3 budget: the reference's own shipped arithmetic for blocks >= 32^2 "
           "(training/networks.py:634-638), a timing data point, NOT a parity mode",
    "f6": "f8 with fp6 (e2m3) correction products (per-pixel 16-channel block scales) in the two large up=2 launches: the round-5 experiment, "
          "not faster than f8 (profiles/r05_f6_ab.txt); everything else as f8",
}


def scheme_ceiling(mode):
    """Matrix work a mode executes per algorithmic FLOP, at the nominal dense peaks."""
    return {"f32": PEAK_F32_MATRIX_TFLOPS, "h3": PEAK_F16_MATRIX_TFLOPS / 3,
            "f8": 1 / (1 / PEAK_F16_MATRIX_TFLOPS + 2 / PEAK_FP8_MATRIX_TFLOPS),
            "f6": 1 / (1 / PEAK_F16_MATRIX_TFLOPS + 2 / PEAK_FP8_MATRIX_TFLOPS),         # (priced as f8: most of its launches are)
            "f16": PEAK_F16_MATRIX_TFLOPS}[mode]                                        # (priced at its four large launches: one f16 MFMA FLOP per algorithmic FLOP)


def load_traffic(mode, res, batch):
    """HBM bytes per launch by kernel: PMC counters cannot be read inside this process, so the figures come from
    profiles/hbm_traffic.json (tools/collect_profiles.sh: separate rocprofv3 --pmc passes of this very command per mode), and
    only if that file was measured on the kernel sources that are running now (content digest) -- otherwise null."""
    tpath = os.path.join(REPO, "profiles", "hbm_traffic.json")
    if not os.path.exists(tpath):
        return {}, "profiles/hbm_traffic.json missing"
    try:
        from brushstroke_engine_amd import build as _b
        tj = json.load(open(tpath))
        stamp = tj.get("_stamp", {})
        if not (res == 256 and batch == 32):
            return {}, "profiles/hbm_traffic.json holds the default workload (R=256, batch 32): not used for this one"
        if stamp.get("source_digest") != _b.source_digest():
            return {}, "profiles/hbm_traffic.json was measured on other kernel sources (stale): not used"
        table = tj.get("modes", {}).get(mode)
        if table is None and mode in ("f6", "f16"):
            table = tj.get("modes", {}).get("f8")                      # (the same kernels; the f6 / hi-only template forms read the same bytes)
        if table is None and mode == "f8" and "modes" not in tj:
            table = {k: v for k, v in tj.items() if not k.startswith("_")}
        if table is None:
            return {}, f"profiles/hbm_traffic.json has no PMC pass for mode {mode}"
        return table, f"rocprofv3 PMC passes at commit {stamp.get('git_head') or '(unrecorded)'}, same kernel sources"
    except Exception as e:                                  # noqa: BLE001
        return {}, f"profiles/hbm_traffic.json unreadable: {e}"


def traffic_lookup(table, kname):
    """Bytes per launch of kernel `kname`; the fp32 kernels are named by their leading template parameters only
    (nb_modconv3x3_variant), the profiler prints all of them."""
    if kname in table:
        return table[kname]
    if kname.endswith(">"):
        hits = [v for k, v in table.items() if k.startswith(kname[:-1] + ",") or k.startswith(kname[:-1] + ">")]
        if len(hits) == 1:
            return hits[0]
    return None


def measure_mode(G, mode, args, cfg, inputs, world, rank, dev, backend, gather, sampler=None, calib=None, outputs=None):
    """W warm-up steps, then exactly K timed steps of the hot path in one arithmetic mode, bracketed by barrier +
    synchronize; returns this mode's figures (value, ms_per_step; with --full also the single-stream leg and the roofline of
    its dominant kernel).  ``outputs`` (a dict): receives the uint8 RGBA tiles of the last timed step of the leg `value` is
    measured on, as a host array."""
    from brushstroke_engine_amd.sharding import TileGatherer
    z, geom, pos = inputs
    B = args.batch
    # the generator runs a batch as `sub` sub-batches on separate HIP streams; with N>1 each part's RGBA tiles are
    # gathered from the part's own stream, so steps keep overlapping across the streams at any N
    sub = G.sub_streams if (B >= G.sub_stream_min_batch and args.schedule in ("concurrent", "single")) else 1
    use_pg = args.use_pg                 # a process group exists: N > 1, or NB_FORCE_PG=1 at N = 1 (the collectives of the N > 1 path through RCCL on one GPU)
    gatherer = TileGatherer([B, args.res, args.res, 4], torch.uint8, dev, timing=True) if gather else None
    part_gatherers = []
    if gatherer is not None and sub > 1:
        bounds = [(i * B // sub, (i + 1) * B // sub) for i in range(sub)]
        part_gatherers = [TileGatherer([b - a, args.res, args.res, 4], torch.uint8, dev, timing=True) for a, b in bounds]

    def finish_gathers():
        if gatherer is not None:
            gatherer.finish()
            for g_ in part_gatherers:
                g_.finish()

    pipe = None
    if args.schedule == "pipeline":
        from brushstroke_engine_amd.pipeline import TriadStepPipeline
        pipe = TriadStepPipeline(G)
        if not pipe._eligible(B):
            pipe = None
    schedule_single = ("steps software-pipelined over two HIP streams (pipeline.TriadStepPipeline): the head of step k+1 -- mapping, styles, "
                       "the <= 16x16 layers: 2 % of the FLOPs in latency-bound launches -- runs under the big convolutions of step k"
                       if pipe is not None else "steps enqueued back to back on one stream")
    if args.schedule == "prefetch" and pipe is None:
        from brushstroke_engine_amd.pipeline import TriadPrefetchPipeline
        pipe = TriadPrefetchPipeline(G, mark_layer=os.environ.get("NB_PREFETCH_MARK") or None)
        schedule_single = ("steps on one stream; what step k+1 needs before its first layer (mapping, styles, small layers' noise, geometry "
                           "packs: no matrix work) is enqueued on a side stream under the LAST layer of step k (pipeline.TriadPrefetchPipeline)")

    def step():
        if pipe is not None:
            u8 = pipe.submit(z, geom, pos)
            if gatherer is not None:
                with torch.cuda.stream(getattr(pipe, "tail_stream", None) or pipe.main_stream):
                    gatherer.finish()
                    gatherer.start(u8)
            return u8
        # without a gather the step is enqueued without joining the generator's sub-batch streams, so consecutive
        # steps overlap across them (the timed region ends with a device-wide synchronize)
        res = G.render_triad(z=z, geom_feature=geom, positions=pos, render_mode="clear", join=False)
        if gatherer is not None:
            if callable(res):           # sub-batches: one gather per part, enqueued from the part's stream
                for g_, st_, u8_ in zip(part_gatherers, res.streams, res.parts_u8):
                    with torch.cuda.stream(st_):
                        g_.finish()     # previous step's gather must be done before its buffer is reused
                        g_.start(u8_)
            else:
                gatherer.finish()
                gatherer.start(res[0])
        return res

    # The library's throughput schedule (pipeline.ConcurrentTriadSteps; the headline since round 6): independent steps dealt round-robin
    # to k HIP streams with a workspace slot each -- the other chains' kernels fill the CUs one chain leaves idle in its kernel tails
    # and in its small launches.  k = --streams, 0 = the library's own probe (1 or 3).  With N > 1 every stream has its own gatherer:
    # the tiles of step i are gathered from the stream that rendered them, the gather of step i - k is waited for first.
    conc, conc_gatherers = None, []
    if args.schedule == "concurrent":
        from brushstroke_engine_amd.pipeline import ConcurrentTriadSteps
        conc = ConcurrentTriadSteps(G, streams=args.streams)
        if args.streams == 0:
            conc.choose(z, geom, pos)
        if gather:
            conc_gatherers = [TileGatherer([B, args.res, args.res, 4], torch.uint8, dev, timing=True) for _ in range(conc.streams)]

    def step_conc():
        u8 = conc.submit(z, geom, pos)
        if conc_gatherers:
            g_ = conc_gatherers[(conc._i - 1) % conc.streams]
            with torch.cuda.stream(conc.last_stream):
                g_.finish()
                g_.start(u8)
        return u8

    def finish_conc():
        for g_ in conc_gatherers:
            g_.finish()
        conc.wait()

    # Burn-in (untimed, before the W warmup steps): a fresh process on a fresh box runs its first steps well below
    # steady state (host-side first-touch costs: lazily loaded code objects, allocator growth, cold Python paths, clock
    # ramp), and one step is only ~2 ms.  Run chunks of 5 steps until two consecutive chunks agree within 3 %
    # (at least 0.5 s, at most 8 s); the chunk times are reported as "burn_in_ms_per_step".
    burn_in = []
    if sampler is not None:
        # board power / shader clock of this mode: sampled from here to the end of its last timed region (burn-in + warm-up + rehearsals
        # + timed legs: the same steps throughout) -- the timed K steps alone are ~40 ms, four ticks of the 10 ms sampler
        sampler.mark(mode)
    t_burn = time.perf_counter()
    while True:
        tb = time.perf_counter()
        for _ in range(5):
            step()
        finish_gathers()
        torch.cuda.synchronize()
        burn_in.append((time.perf_counter() - tb) / 5 * 1e3)
        spent = time.perf_counter() - t_burn
        stable = len(burn_in) >= 2 and abs(burn_in[-1] - burn_in[-2]) <= 0.03 * burn_in[-2]
        if use_pg:                          # all ranks must leave the loop together
            flag = torch.tensor([1.0 if (stable and spent >= 0.5) or spent >= 8.0 else 0.0], device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if flag.item() > 0:
                break
        elif (stable and spent >= 0.5) or spent >= 8.0:
            break
    def reduce_times(el, el_local):
        """MAX over ranks of the timed region, and every rank's own time for its K steps (before the closing barrier)."""
        if not use_pg:
            return el, None
        t = torch.tensor([el], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        mine = torch.zeros([world], dtype=torch.float64, device=dev)
        mine[rank] = el_local / args.steps * 1e3
        dist.all_reduce(mine, op=dist.ReduceOp.SUM)
        return float(t.item()), [round(float(v), 4) for v in mine.tolist()]

    def gather_wait_of(gs):
        """How long rank 0 waited for the tile gathers inside the timed steps."""
        gs = [g_ for g_ in gs if g_ is not None]
        if not gs:
            return None
        w_ = [g_.wait_ms() for g_ in gs]
        return {"host_ms_per_step": round(sum(x["host_ms"] for x in w_) / args.steps, 4),
                "stream_ms_per_step": (round(sum(x["stream_ms"] or 0.0 for x in w_) / args.steps, 4)
                                       if any(x["stream_ms"] is not None for x in w_) else None),
                "waits": sum(x["waits"] for x in w_),
                "what": "time TileGatherer.finish() kept THIS rank (0) waiting inside the timed steps: host wall clock, and "
                        "HIP events on the issuing stream around the wait (an RCCL wait stalls the stream, not the host); the "
                        "gather of a step is waited for when its stream's next step has been enqueued, after a whole step of compute"}

    # The single-stream leg: W warm-up steps, then K timed steps on the schedule of step().  It is the headline when the schedule
    # is not the concurrent one; with --full it always runs, and the roofline comes from it.  Only --full brackets launches
    # with HIP events (calibration pass, dominant kernel in the timed steps): a plain run times the bare steps.
    single, schedule, cal, events, rehearsal_ms = None, schedule_single, {}, [], None
    if args.full or conc is None:
        for _ in range(args.warmup):
            step()
        finish_gathers()
        torch.cuda.synchronize()

        none_ = frozenset()
        dom_layers = none_
        if args.full:
            # Calibration (untimed): 3 steps with a HIP-event pair around EVERY launch give the per-layer table and name the
            # dominant kernel.  Event pairs cost ~10 us of stream time each (45 launches -> ~0.9 ms per step), so the timed
            # region below only brackets the launches of that dominant kernel.
            G.synthesis.layer_events, G.synthesis.event_filter = [], None
            for _ in range(3):
                step()
            finish_gathers()
            torch.cuda.synchronize()
            cal_events = G.synthesis.layer_events
            layer_kernels = dict(G.synthesis.layer_kernels)
            for name, e0, e1 in cal_events:
                cal.setdefault(name, []).append(e0.elapsed_time(e1))
            ksum = {}
            for name, ts in cal.items():
                if name in layer_kernels:
                    ksum[layer_kernels[name]] = ksum.get(layer_kernels[name], 0.0) + float(np.mean(ts))
            dom_name = max(ksum, key=ksum.get)
            dom_layers = {name for name, k in layer_kernels.items() if k == dom_name}

        # events for the timed region are created and recorded once beforehand (event creation is slow in a fresh process),
        # and the timed loop is rehearsed once, untimed, in exactly its final configuration (same event filter, pooled
        # events) so that nothing happens for the first time inside the timed region
        def make_pool():
            pool = [torch.cuda.Event(enable_timing=True) for _ in range(2 * len(dom_layers) * args.steps + 2)]
            for e in pool:
                e.record()
            torch.cuda.synchronize()
            return pool
        if args.full:
            G.synthesis.event_pool = make_pool()
            G.synthesis.layer_events = []
        t_reh = time.perf_counter()
        for i_ in range(args.steps):
            G.synthesis.event_filter = dom_layers if i_ % args.event_every == 0 else none_
            step()
        finish_gathers()
        torch.cuda.synchronize()
        rehearsal_ms = (time.perf_counter() - t_reh) / args.steps * 1e3
        if args.full:
            G.synthesis.event_pool = make_pool()
        if use_pg:
            dist.barrier()
        torch.cuda.synchronize()
        if args.full:
            G.synthesis.layer_events = []
        for g_ in [gatherer] + part_gatherers:
            if g_ is not None:
                g_.wait_ms()                                 # (reset: count the waits of the timed region only)
        t0 = time.perf_counter()
        for i_ in range(args.steps):
            G.synthesis.event_filter = dom_layers if i_ % args.event_every == 0 else none_
            last = step()
        finish_gathers()
        torch.cuda.synchronize()
        elapsed_local = time.perf_counter() - t0
        if use_pg:
            dist.barrier()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        if sampler is not None:
            sampler.unmark(mode)                    # (moved on below when the concurrent leg follows)
        if outputs is not None and conc is None:    # (a pipeline returns the tiles; render_triad a tuple, or a joining callable)
            last = last() if callable(last) else last
            outputs["rgba_u8"] = (last if torch.is_tensor(last) else last[0]).cpu().numpy()
        last = None
        events = G.synthesis.layer_events or []
        G.synthesis.layer_events, G.synthesis.event_filter, G.synthesis.event_pool = None, None, None

        elapsed, per_rank_ms = reduce_times(elapsed, elapsed_local)
        gather_wait = gather_wait_of([gatherer] + part_gatherers)
        single = {"value": round(world * B * args.steps / elapsed, 2), "ms_per_step": round(elapsed / args.steps * 1e3, 4), "schedule": schedule_single}
    if conc is not None:
        # the headline leg: the same K steps on the concurrent schedule -- W warm-up steps, one untimed rehearsal of the timed loop,
        # then exactly K steps between barrier + synchronize on both sides; no events inside (launches overlap: their durations say
        # nothing about a kernel, which is why the roofline comes from the single-stream leg above)
        for _ in range(args.warmup):
            step_conc()
        finish_conc()
        torch.cuda.synchronize()
        t_reh = time.perf_counter()
        for _ in range(args.steps):
            step_conc()
        finish_conc()
        torch.cuda.synchronize()
        rehearsal_ms = (time.perf_counter() - t_reh) / args.steps * 1e3
        for g_ in conc_gatherers:
            g_.wait_ms()
        if use_pg:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            last = step_conc()
        finish_conc()
        torch.cuda.synchronize()
        elapsed_local = time.perf_counter() - t0
        if use_pg:
            dist.barrier()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        if sampler is not None:
            sampler.unmark(mode)
        if outputs is not None:
            outputs["rgba_u8"] = last.cpu().numpy()
        last = None
        elapsed, per_rank_ms = reduce_times(elapsed, elapsed_local)
        gather_wait = gather_wait_of(conc_gatherers)
        schedule = (f"{conc.streams} independent steps in flight, dealt round-robin to {conc.streams} HIP streams with a workspace slot each "
                    f"(pipeline.ConcurrentTriadSteps, the library's throughput schedule"
                    + (f"; stream count chosen by its probe: {conc.probe}" if conc.probe else "") + "); every step is the plain "
                    "Generator.render_triad pass: bit-identical to the serial loop (tests/test_hip_generator.py)")

    ms_per_step = elapsed / args.steps * 1e3
    whole = B * 2 * cfg.macs_per_patch() / (ms_per_step * 1e-3) / 1e12
    headline = {
        "value": round(world * B * args.steps / elapsed, 2), "unit": "patches/s", "ms_per_step": round(ms_per_step, 4),
        "steps": args.steps, "warmup": args.warmup, "dtype": MODE_DTYPE[mode], "schedule": schedule,
        "roofline_whole_step": {
            "what": "the whole step (all launches of one GPU) against the ceilings of SURVEY 8d: algorithmic FLOPs of the batch / ms_per_step",
            "achieved": round(whole, 1), "unit": "TFLOP/s", "fp32_matrix_peak": PEAK_F32_MATRIX_TFLOPS,
            "scheme_ceiling": round(scheme_ceiling(mode), 1), "frac_of_scheme_ceiling": round(whole / scheme_ceiling(mode), 4),
            "note": "scheme ceiling = the matrix work the arithmetic mode executes per algorithmic FLOP at nominal dense peaks (f8: one f16 "
                    "+ two fp8 MFMA FLOPs; h3: three f16); the K loops run at ~1.6-1.8 GHz under load (in-kernel s_memtime clock), not 2.4"},
        "rehearsal_ms_per_step": round(rehearsal_ms, 4),
        "burn_in_ms_per_step": [round(b, 3) for b in burn_in[:6]] + (["..."] if len(burn_in) > 7 else []) + [round(b, 3) for b in burn_in[6:][-1:]],
    }
    if conc is not None:
        headline["streams"] = conc.streams
        headline["stream_probe"] = conc.probe
    if per_rank_ms is not None:
        headline["ms_per_step_per_rank"] = per_rank_ms
    if gather_wait is not None:
        headline["gather_wait_ms"] = gather_wait
    if not args.full:
        return headline

    # after the timed region: the dominant kernel once more with the whole batch on ONE stream (3 steps), so that its
    # launch duration is also known without another stream's kernels sharing the chip
    iso = {}
    if sub > 1:
        keep = G.sub_streams
        G.sub_streams = 1
        for _ in range(2):                           # (first single-stream steps build that workspace: not measured)
            step()
        finish_gathers()
        torch.cuda.synchronize()
        G.synthesis.layer_events, G.synthesis.event_filter = [], dom_layers
        for _ in range(3):
            step()
        finish_gathers()
        torch.cuda.synchronize()
        for name, e0, e1 in G.synthesis.layer_events:
            iso.setdefault(name, []).append(e0.elapsed_time(e1))
        G.synthesis.layer_events, G.synthesis.event_filter = None, None
        G.sub_streams = keep

    # dominant kernel: algorithmic FLOPs / HIP-event time of its launches inside the timed region (launch stream)
    specs = {sp.name: sp for sp in cfg.layers}
    timed = {}
    for name, e0, e1 in events:
        timed.setdefault(name, []).append(e0.elapsed_time(e1))
    # a layer is launched once per sub-batch (the generator runs the batch as `sub` sub-batches on separate streams):
    # every launch is bracketed on its own stream and carries batch/sub patches
    sampled_steps = len(range(0, args.steps, args.event_every))
    sub = max(1, round(len(next(iter(timed.values()))) / sampled_steps))
    dom_ms = sum(float(np.mean(ts)) for ts in timed.values())            # mean launch duration, summed over the kernel's layers
    dom_fl = sum(layer_flops(specs[name], B / sub) for name in timed)
    dom_launches = len(timed)
    peak_of = lambda kname: PEAK_F16_MATRIX_TFLOPS if is_split_kernel(kname) else PEAK_F32_MATRIX_TFLOPS
    dom_peak = peak_of(dom_name)
    achieved = dom_fl / (dom_ms * 1e-3) / 1e12
    # calibration table (all launches bracketed, untimed pass)
    rows, kernels = [], {}
    for name, ts in cal.items():
        if name not in specs:
            continue
        ms = float(np.mean(ts))
        fl = layer_flops(specs[name], B / max(1, round(len(ts) / 3)))
        kname = layer_kernels[name]
        rows.append((ms, kernel_label(specs[name]), fl, kname))
        k = kernels.setdefault(kname, {"ms": 0.0, "flops": 0.0, "launches": 0, "peak": peak_of(kname)})
        k["ms"] += ms; k["flops"] += fl; k["launches"] += 1
    rows.sort(reverse=True)
    conv_ms = sum(r[0] for r in rows)
    conv_fl = sum(r[2] for r in rows)
    ttable, traffic_note = load_traffic(mode, args.res, B)
    traffic = traffic_lookup(ttable, dom_name)
    split = is_split_kernel(dom_name)
    roofline = {"bound": "mfma", "kernel": dom_name, "achieved": round(achieved, 2), "peak": dom_peak,
                "unit": "TFLOP/s", "frac": round(achieved / dom_peak, 4), "traffic": traffic, "traffic_source": traffic_note,
                "peak_what": ("dense f16 MFMA (MI355X_MICROARCH.md ~2.5 PFLOP/s): the type this kernel multiplies in" if split else
                              "fp32 MFMA (MI355X_MICROARCH.md 157.3 TFLOP/s): the type this kernel multiplies in"),
                "executed_mfma": (({"tflops": round(3 * achieved, 1), "frac": round(3 * achieved / dom_peak, 4),
                                    "what": "f16 MFMA FLOPs actually executed for the algorithmic ones (3 products per fp32 "
                                            "product; halo / block-rounding overhead of the up=2 kernel not included)"}
                                   if mode == "h3" else
                                   {"tflops": round(achieved, 1), "frac": round(achieved / dom_peak, 4),
                                    "what": "hi-only f16 products: one f16 MFMA FLOP per algorithmic FLOP"}
                                   if mode == "f16" else
                                   {"f16_tflops": round(achieved, 1), "fp8_tflops": round(2 * achieved, 1),
                                    "frac": round(achieved / PEAK_F16_MATRIX_TFLOPS + 2 * achieved / PEAK_FP8_MATRIX_TFLOPS, 4),
                                    "what": "matrix work actually executed per algorithmic FLOP: 1 f16 MFMA FLOP (main product) + "
                                            "2 fp8 MFMA FLOPs (both correction products in one K=64 block-scaled instruction per "
                                            "tap pair); frac = share of the matrix pipes' time (f16 peak 2500, fp8 peak 5000 TFLOP/s)"})
                                  if split else None),
                "hbm": ({"what": "the same launches against the HBM roofline (MI355X_MICROARCH.md: ~8 TB/s): measured HBM bytes per "
                                 "launch (traffic) / launch duration; the path is matrix-pipe bound, not HBM bound",
                         "achieved": round(traffic / (dom_ms / dom_launches * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                         "frac": round(traffic / (dom_ms / dom_launches * 1e-3) / 1e9 / PEAK_HBM_GBPS, 4)} if traffic else None),
                "launch_ms": round(dom_ms / dom_launches, 4), "launches_per_step": dom_launches * sub,
                "sampling": f"HIP events around the kernel's launches in every {args.event_every}-th of the {args.steps} timed steps "
                            f"({sampled_steps} steps sampled)",
                "patches_per_launch": B // sub,
                "concurrency": ((f"{sub} sub-batches in flight on {sub} HIP streams: launch durations are measured while "
                                 f"the other stream's kernels share the chip") if sub > 1 else
                                ("tails back to back on one stream; only the next step's small head launches (mapping, styles, <= 16x16 "
                                 "layers) share the chip with this kernel") if pipe is not None else "single stream"),
                "isolated": ({"what": f"same kernel, whole batch of {B} on one stream (3 untimed steps after the timed region)",
                              "launch_ms": round(sum(float(np.mean(t)) for t in iso.values()) / len(iso), 4),
                              "achieved": round(sum(layer_flops(specs[nm], B) for nm in iso)
                                                / (sum(float(np.mean(t)) for t in iso.values()) * 1e-3) / 1e12, 2),
                              "frac": round(sum(layer_flops(specs[nm], B) for nm in iso)
                                            / (sum(float(np.mean(t)) for t in iso.values()) * 1e-3) / 1e12 / dom_peak, 4)}
                             if iso else None),
                "flops_per_launch": dom_fl / dom_launches,
                "note": (("fp32 MFMA" if not split else
                          "split-f16 kernels execute 3 f16 MFMA FLOPs per algorithmic fp32 FLOP: frac <= 1/3 by construction"
                          if mode == "h3" else
                          "hi-only f16 products: one f16 MFMA FLOP per algorithmic FLOP (NOT a parity mode: 1.5e-3 ... 3e-3 from fp32)"
                          if mode == "f16" else
                          "split-f16 + fp8-correction kernels spend 2 f16-MFMA-equivalents of matrix time per algorithmic fp32 FLOP: "
                          "frac (against the f16 peak) <= 1/2 by construction")
                         + ("; launch durations are from this mode's SINGLE-STREAM timed leg (value_single_stream: the same K steps "
                            "back to back on one stream, HIP events on that stream), not from the headline leg, where the steps of "
                            "several streams share the chip and a launch's duration says nothing about the kernel" if conc is not None else "")),
                "calibration": {"what": "untimed pass with every launch bracketed by HIP events",
                                "all_conv_launches": {"tflops": round(conv_fl / (conv_ms * 1e-3) / 1e12, 2), "ms_per_step": round(conv_ms, 4)},
                                "kernels": {k: {"ms_per_step": round(v["ms"], 4), "launches": v["launches"],
                                                "achieved": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2), "peak": v["peak"],
                                                "traffic": traffic_lookup(ttable, k)}
                                            for k, v in kernels.items()},
                                "layers_ms": {r[1]: round(r[0], 4) for r in rows},
                                "other_ms": {k: round(float(np.sum(v)) / 3, 4) for k, v in cal.items() if k not in specs}}}
    if calib and calib.get("mfma_f16_sustained_tflops") and split:
        roofline["frac_of_sustained"] = round(achieved / calib["mfma_f16_sustained_tflops"], 4)
        roofline["frac_of_sustained_what"] = ("achieved / box_calibration.mfma_f16_sustained_tflops: against what THIS board holds on a "
                                              "registers-only f16 MFMA loop at its own clock under load, instead of the nominal 2.5 PFLOP/s")
    extra = {}
    if sampler is not None:
        extra["telemetry"] = sampler.summary(mode)
    if conc is not None:
        extra["value_single_stream"] = single["value"]
        extra["single_stream"] = single
    return {**headline, **extra, "roofline": roofline}


MAX_LINE_BYTES = 4096               # the final stdout line: the driver keeps the last 8 KB of stdout
DUMP_LIMIT_BYTES = 64 * 2**20       # --dump-outputs: all files together
NPY_HEADER_BYTES = 4096             # (an upper bound of one .npy file's header)


def dump_outputs(dirname, arrays, limit=DUMP_LIMIT_BYTES):
    """Writes every array of ``arrays`` ({name: array}) as ``dirname/<name>.npy`` in float32.  If they do not fit ``limit`` bytes,
    each keeps the same fixed, seeded sample of its leading axis (patches), in ascending order, and the indices taken go to
    ``dirname/<name>_index.npy`` (float64).  Returns {file name: shape}."""
    os.makedirs(dirname, exist_ok=True)
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    full = sum(a.size * 4 + NPY_HEADER_BYTES for a in arrays.values())
    idx = None
    if full > limit:
        n = min(a.shape[0] for a in arrays.values())
        per_item = sum(a[0].size * 4 + 8 for a in arrays.values())
        k = (limit - 2 * NPY_HEADER_BYTES * len(arrays)) // per_item
        if k < 1:
            raise ValueError(f"--dump-outputs: one patch of the outputs is larger than {limit} bytes")
        idx = np.sort(np.random.RandomState(0).choice(n, min(k, n), replace=False))
    written = {}
    for name, a in arrays.items():
        parts = {name: a.astype(np.float32)} if idx is None else {name: a[idx].astype(np.float32), f"{name}_index": idx.astype(np.float64)}
        for fn, arr in parts.items():
            np.save(os.path.join(dirname, f"{fn}.npy"), arr)
            written[f"{fn}.npy"] = list(arr.shape)
    return written


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d and d[k] is not None} if isinstance(d, dict) else None


def compact_roofline(r):
    """The roofline object without its tables and prose (those are in bench_detail.json)."""
    c = _pick(r, ("bound", "kernel", "achieved", "peak", "unit", "frac", "frac_of_sustained", "traffic", "launch_ms", "launches_per_step",
                  "flops_per_launch", "patches_per_launch"))
    c.setdefault("traffic", None)
    if r.get("hbm"):
        c["hbm"] = _pick(r["hbm"], ("achieved", "peak", "unit", "frac"))
    return c


def fit_line(c):
    """The compact record as ONE JSON line below MAX_LINE_BYTES: optional keys are dropped, least important first, until it fits --
    a line is ALWAYS printed (an assertion here once stood between a finished measurement and its record, and at N > 1 would have
    left the other ranks waiting in the closing barrier)."""
    dumps = lambda d: json.dumps(d, separators=(",", ":"))
    line = dumps(c)
    droppable = ["stream_probe", "telemetry", "box_calibration", "ms_per_step_per_rank", "gather_wait_ms", "latency_batch1",
                 "roofline_whole_step", "parity", "modes", "rccl", "value_fp32_parity", "detail_file"]
    dropped = []
    for k in droppable:
        if len(line) < MAX_LINE_BYTES:
            break
        if k == "modes" and isinstance(c.get("modes"), dict):          # first without the per-mode rooflines, then without the modes
            c["modes"] = {m: _pick(r, ("value", "ms_per_step", "parity")) for m, r in c["modes"].items()}
            dropped.append("modes.*.roofline")
            line = dumps({**c, "dropped": dropped})
            if len(line) < MAX_LINE_BYTES:
                break
        if k in c:
            del c[k]
            dropped.append(k)
            line = dumps({**c, "dropped": dropped})
    if len(line) >= MAX_LINE_BYTES:                                     # (cannot happen with the contract's keys alone: < 1.5 KB)
        c = _pick(c, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                      "data"))
        line = dumps({**c, "dropped": "everything but the contract's scalar keys"})
    return line


def compact_line(out):
    """What goes to stdout: the contract's keys, numbers only (no calibration tables, no per-layer times, no explanatory strings).
    The figures of a --full run (roofline, box calibration, the other modes ...) only where the record has them."""
    c = _pick(out, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "conv_mode", "data"))
    c["vs_baseline"] = None
    c["dtype"] = out["dtype"].split(",")[0].split(":")[0][:90]
    cfg_ = out["config"]
    c["config"] = {"workload": cfg_["workload"].split(";")[0], "batch_per_gpu": cfg_["batch_per_gpu"], "resolution": cfg_["resolution"],
                   "gflop_per_patch": cfg_["gflop_per_patch"], "parallelism": cfg_["parallelism"].split(" inside every step")[0]}
    if out.get("roofline"):
        c["roofline"] = compact_roofline(out["roofline"])
    ws = out.get("roofline_whole_step") or {}
    c["roofline_whole_step"] = _pick(ws, ("achieved", "unit", "scheme_ceiling", "frac_of_scheme_ceiling"))
    if out.get("cpu_baseline"):
        c["cpu_baseline"] = _pick(out["cpu_baseline"], ("value", "unit", "cores", "kind"))
        c["cpu_baseline"]["sample"] = out["cpu_baseline"].get("sample", "").split(" (")[0]
        par = out["cpu_baseline"].get("parity")
        if par:
            c["parity"] = _pick(par, ("max_abs_rgba_vs_oracle", "max_u8_diff", "tolerance", "patches"))
    if "box_calibration" in out:
        c["box_calibration"] = _pick(out["box_calibration"] or {}, ("mfma_f16_sustained_tflops", "loop_clock_mhz"))
    tele = _pick(out.get("telemetry") or {}, ("power_w_mean", "sclk_mhz_mean", "power_cap_w", "samples"))
    if tele and tele.get("power_w_mean") is not None:          # (absent when the window held too few samples to mean anything)
        c["telemetry"] = tele
    if out.get("latency_batch1"):
        c["latency_batch1"] = _pick(out["latency_batch1"], ("unit", "p50", "p99", "p50_incl_d2h", "p99_incl_d2h"))
    for k_ in ("value_single_stream", "streams"):
        if out.get(k_) is not None:
            c[k_] = out[k_]
    if out.get("stream_probe"):
        c["stream_probe"] = out["stream_probe"].get("ms_per_step")
    if "value_fp32_parity" in out:
        c["value_fp32_parity"] = out["value_fp32_parity"]
    modes = {}
    for m, r in (out.get("modes") or {}).items():
        modes[m] = {"value": r["value"], "ms_per_step": r["ms_per_step"], **_pick(r, ("value_single_stream", "streams")),
                    "roofline": _pick(r["roofline"], ("kernel", "achieved", "peak", "frac", "frac_of_sustained", "launch_ms")),
                    "parity": (r.get("parity") or {}).get("max_abs_rgba_vs_oracle")}
        if m == "f16":
            modes[m]["note"] = "reference's shipped arithmetic (plain f16 products); NOT a parity mode: outside the 1e-3 budget"
    if modes:
        c["modes"] = modes
    if out.get("rccl"):
        f = out["rccl"]
        c["rccl"] = _pick(f, ("world", "backend", "nccl_version", "distinct_devices"))
        c["rccl"]["ranks_seen"] = [r_.get("rank") for r_ in f.get("ranks_seen", [])]
        c["ms_per_step_per_rank"] = out.get("ms_per_step_per_rank")
        c["gather_wait_ms"] = _pick(out.get("gather_wait_ms") or {}, ("host_ms_per_step", "stream_ms_per_step", "waits"))
    c["detail_file"] = out.get("detail_file")
    return c


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32, help="patches per GPU per step")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything else, in the same process: board calibration and telemetry, the "
                         "single-stream leg and the roofline of its dominant kernel, the other arithmetic modes (N=1), batch-1 latency, "
                         "the CPU baseline and every mode's parity against it.  Without it a run does only what `value` needs")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the cpu_baseline leg (and with it the live parity of every mode)")
    ap.add_argument("--no-latency", action="store_true", help="--full: skip the batch-1 hipGraph latency leg")
    ap.add_argument("--conv-mode", default=None, choices=["h3", "f8", "f6", "f32", "f16"],
                    help="the PRIMARY arithmetic mode = top-level value; default: the library default (networks.DEFAULT_CONV_MODE = f8). "
                         "f8: f16 main product + two block-scaled fp8 correction products (pixels within 1e-4 of fp32; budget 1e-3); "
                         "h3: three f16 products on hi/lo-split operands (5e-6); f32: all layers on the fp32 MFMA kernels")
    ap.add_argument("--modes", default=None,
                    help="--full: comma list of arithmetic modes measured one after the other in this process (each its own Generator, W "
                         "warm-up + K timed steps) and reported under `modes`; default: f8, h3, f32, f16 at N=1, the primary one only at N>1; "
                         "'primary' = only it (what a run without --full measures)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="--full: CPU time budget of the cpu_baseline leg")
    ap.add_argument("--no-gather", action="store_true", help="N>1: skip the RGBA gather to rank 0")
    ap.add_argument("--schedule", default="concurrent", choices=["concurrent", "single", "pipeline", "prefetch"],
                    help="how the K steps are enqueued.  concurrent (default; the library's throughput schedule, pipeline.ConcurrentTriadSteps): "
                         "independent steps dealt round-robin to --streams HIP streams with a workspace slot each -- `value` is measured on it; "
                         "with --full, `roofline` and `value_single_stream` on the same K steps back to back on ONE stream (measured in the same "
                         "run, where every launch has the chip to itself and its HIP-event duration is the kernel's own time).  single: only "
                         "that leg.  pipeline / prefetch: the two-stream software pipelines of pipeline.py (+2 %% / -0.3 %%; kept for A/Bs)")
    ap.add_argument("--streams", type=int, default=0, help="streams of the concurrent schedule; 0 = the library's probe picks 1 or 3")
    ap.add_argument("--prefetch", action="store_true", help="= --schedule prefetch")
    ap.add_argument("--pipeline", action="store_true", help="= --schedule pipeline")
    ap.add_argument("--full-line", action="store_true", help="print the FULL record on stdout instead of the compact line (the A/B scripts under "
                                                             "tools/ read the calibration tables of a --full run from it)")
    ap.add_argument("--detail", default=None, help="where the full record goes (default: bench_detail.json next to this file)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the headline leg's last timed step returned (the primary mode's uint8 RGBA "
                         "tiles of rank 0's batch) as DIR/rgba_u8.npy in float32; a fixed, seeded sample of the patches if the whole "
                         f"would exceed {DUMP_LIMIT_BYTES >> 20} MB")
    ap.add_argument("--event-every", type=int, default=4,
                    help="--full: bracket the dominant kernel's launches with HIP events in every K-th step of the single-stream leg (an "
                         "event pair costs ~10 us of stream time, which a single chain of launches cannot hide)")
    args = ap.parse_args(argv)
    if args.event_every < 1:
        ap.error("--event-every must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.pipeline or args.prefetch:
        args.schedule = "pipeline" if args.pipeline else "prefetch"
    if args.streams < 0 or args.streams > 8:
        ap.error("--streams must lie in 0..8")
    if args.dump_outputs and args.res * args.res * 4 * 4 + 8 > DUMP_LIMIT_BYTES - 2 * NPY_HEADER_BYTES:
        ap.error(f"--dump-outputs: one {args.res}x{args.res} patch exceeds {DUMP_LIMIT_BYTES >> 20} MB")
    if args.modes not in (None, "primary") and not args.full:
        ap.error("--modes measures other arithmetic modes: that needs --full (a plain run measures the primary mode, --conv-mode)")
    return args


def main():
    args = parse_args()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # self-launch: N ranks as a child torchrun.  Nothing in this process has touched the GPU (importing torch does
        # not), and it only waits for the child -- no exec of a GPU-initialised process.  The kernel library is built
        # here, once, so that no rank compiles while the others wait in a collective.  --standalone lets torchrun's own
        # rendezvous pick the port (no bind-and-close race with other jobs on the node).
        import subprocess
        from brushstroke_engine_amd import build as _build
        _build.build(verbose=False)
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env.setdefault("OMP_NUM_THREADS", "8")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
               f"--nproc-per-node={args.gpus}", os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd, env=env))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    args.gpus = world
    assert torch.cuda.is_available(), "bench.py needs a GPU (there is no CPU product path)"
    # test hooks for a 1-GPU box: NB_BENCH_SHARE_GPU=1 puts every rank on device 0, NB_BENCH_BACKEND=gloo swaps RCCL out
    # (exercises the N>1 control flow; numbers from such a run mean nothing)
    if os.environ.get("NB_BENCH_SHARE_GPU") == "1":
        local_rank = 0
    backend = os.environ.get("NB_BENCH_BACKEND", "nccl")
    if os.environ.get("NB_BENCH_FAIL_RANK") == str(rank) and world > 1:        # test hook: a rank that dies at start-up
        raise SystemExit(7)
    # the kernel library exists (and is current) BEFORE the process group does: a rank that compiles for minutes while
    # the others sit in init / a collective would run into their timeouts (build() is a no-op when up to date and
    # serialises concurrent callers on a file lock)
    from brushstroke_engine_amd import build as _build, _lib as _nblib
    _build.build(verbose=False)
    _nblib.lib()
    try:                                                  # developer A/B switches (NB_UP1_PP=0 ...): the library itself reads no environment
        sys.path.insert(0, os.path.join(REPO, "tools"))
        import nb_debug_env
        dbg_env = nb_debug_env.apply(_nblib.lib())
    except ImportError:
        dbg_env = {}
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # NB_FORCE_PG=1: create the process group (RCCL) at ANY world size and take every `N > 1` branch below -- pre-flight, fabric report,
    # the gather of RGBA tiles inside the step, barriers and reductions around the timed regions -- so that the collectives of the
    # multi-GPU path run through RCCL on a one-GPU box (`torchrun --nproc-per-node=1`, or plain `python bench.py`: the rendezvous
    # variables are filled in here)
    force_pg = os.environ.get("NB_FORCE_PG") == "1"
    use_pg = world > 1 or force_pg
    args.use_pg = use_pg
    if use_pg:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:
            import socket
            with socket.socket() as sk_:
                sk_.bind(("127.0.0.1", 0))
                os.environ.setdefault("MASTER_PORT", str(sk_.getsockname()[1]))
            os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import datetime
        tmo = datetime.timedelta(seconds=300)            # a wedged collective should fail the run, not hang it
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, timeout=tmo)
        else:
            dist.init_process_group(backend, timeout=tmo)
        # RCCL prints its version banner to stdout through C stdio when the communicator comes up: bring that about NOW and flush, or
        # the banner leaves the process at exit -- behind the JSON line, which must be the last line of stdout (launch.flush_c_stdio)
        from brushstroke_engine_amd import launch as _launch0
        _launch0.warm_up_communicator(dev)

    from brushstroke_engine_amd import config as cfgmod, weights as wmod, synthetic
    from brushstroke_engine_amd.networks import Generator, DEFAULT_CONV_MODE
    from brushstroke_engine_amd.sharding import TileGatherer
    if args.conv_mode is None:
        args.conv_mode = DEFAULT_CONV_MODE
    if not args.full:
        modes = [args.conv_mode]                        # (parse_args refuses --modes naming other modes without --full)
    elif args.modes in (None, "all"):
        # (f6 -- the round-5 experiment, not faster and less accurate than f8 -- only on request: --modes f6 or all)
        # (f16: the reference's shipped precision, OUTSIDE the parity budget -- a timing data point, labelled so in `modes.f16.note`)
        modes = (["f8", "h3", "f32", "f16", "f6"] if args.modes == "all" else ["f8", "h3", "f32", "f16"]) if (world == 1 or args.modes == "all") else [args.conv_mode]
    elif args.modes == "primary":
        modes = [args.conv_mode]
    else:
        modes = [m.strip() for m in args.modes.split(",") if m.strip()]
        if any(m not in MODE_DTYPE for m in modes):
            raise SystemExit(f"--modes: unknown mode in {modes}")
    modes = [args.conv_mode] + [m for m in modes if m != args.conv_mode]        # the primary mode is measured first

    cfg = cfgmod.style1_config(args.res)
    sd = wmod.random_state_dict(cfg, seed=0)
    B = args.batch
    # synthetic inputs, resident in HBM before anything is timed (different per rank)
    # (z in the dtype the mapping network computes in: the fp32 cast of networks.py:261 is then a no-op instead of a launch)
    z = torch.from_numpy(synthetic.batch_z(cfg, B, first_seed=rank * B)).to(dev).to(torch.float32)
    geom = [torch.from_numpy(g).to(dev) for g in synthetic.geom_features(cfg, B, seed=rank)]
    pos = torch.from_numpy(synthetic.positions(cfg, B, seed=rank)).to(dev)
    gather = use_pg and not args.no_gather
    if gather:
        # pre-flight: one small RCCL gather, checked on rank 0.  The gather IS part of the measured job (north_star: "RCCL
        # gather over xGMI to assemble the stylized canvas"): if the fabric refuses it the run fails, non-zero.
        try:
            probe = TileGatherer([4, 8, 8, 4], torch.uint8, dev)
            probe.start(torch.full([4, 8, 8, 4], rank, dtype=torch.uint8, device=dev))
            got = probe.finish()
            torch.cuda.synchronize()
            ok = torch.tensor([1.0 if (rank != 0 or all(int(g.flatten()[0]) == r for r, g in enumerate(got))) else 0.0], device=dev)
        except Exception as e:                                     # noqa: BLE001
            print(f"[bench] rank {rank}: RCCL gather pre-flight failed: {e}", file=sys.stderr, flush=True)
            ok = torch.tensor([0.0], device=dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if ok.item() < 1:
            if rank == 0:
                print("[bench] FAILED: the RCCL gather of RGBA tiles did not pass its pre-flight; no number is reported "
                      "(--no-gather measures the sharded compute alone, and says so in config.parallelism)", file=sys.stderr, flush=True)
            dist.destroy_process_group()
            raise SystemExit(3)

    # who is here (N > 1: all-gather of every rank's device; fails unless the ranks sit on N distinct devices)
    from brushstroke_engine_amd import launch as _launch, telemetry as _tele
    fabric = _launch.fabric_report(dev, rank, world, backend, collective=use_pg)
    # --full: what this board sustains on the instruction the conv kernels are built on (50 ms registers-only f16 MFMA loop),
    # before anything is timed; then a side thread samples board power and shader clock for the rest of the run
    calib, sampler = None, None
    if args.full:
        try:
            import ctypes as _C
            tf, ms_, clk = _C.c_double(), _C.c_double(), _C.c_double()
            _nblib.check(_nblib.lib().nb_calibrate_mfma_f16(50.0, _C.byref(tf), _C.byref(ms_), _C.byref(clk), None), "calibrate")
            calib = {"mfma_f16_sustained_tflops": round(tf.value, 1), "loop_ms": round(ms_.value, 2), "loop_clock_mhz": round(clk.value, 1),
                     "frac_of_nominal_peak": round(tf.value / PEAK_F16_MATRIX_TFLOPS, 4),
                     "what": "registers-only loop of back-to-back v_mfma_f32_32x32x16_f16 on random operands, one wave per SIMD on every CU "
                             "(nb_calibrate_mfma_f16), ~50 ms, run before the first mode; loop_clock_mhz = median in-kernel clock "
                             "(s_memtime / s_memrealtime)"}
        except Exception as e:                                       # noqa: BLE001
            calib = {"mfma_f16_sustained_tflops": None, "what": f"calibration failed: {e}"}
        # (NB_TELEMETRY=0: no sampler thread at all -- the switch of the sampler-on/off A/B, tools/ab_env.sh NB_TELEMETRY=0)
        sampler = _tele.PowerClockSampler(_tele.find_hwmon(_tele.pci_bus_id_of(local_rank)) if os.environ.get("NB_TELEMETRY", "1") != "0" else None)
        sampler.__enter__()
    gens, results = {}, {}
    dumped = {} if (args.dump_outputs and rank == 0) else None
    for m in modes:
        gens[m] = Generator(cfg, sd, conv_mode=m).to(dev)
        results[m] = measure_mode(gens[m], m, args, cfg, (z, geom, pos), world, rank, dev, backend, gather, sampler=sampler, calib=calib,
                                  outputs=dumped if m == args.conv_mode else None)
    G = gens[args.conv_mode]
    prim = results[args.conv_mode]
    if rank == 0:
        out = {
            "metric": "stylized 256x256 stroke patches/sec at batch=32" if args.res == 256 and B == 32
                      else f"stylized {args.res}x{args.res} stroke patches/sec at batch={B}",
            "value": prim["value"], "unit": "patches/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": prim["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": MODE_DTYPE[args.conv_mode],
            "conv_mode": args.conv_mode,
            "data": "synthetic",
            "config": {"workload": f"batch={B} random-z {args.res}x{args.res} patches through the HIP SynthesisNetwork, "
                                   f"style1 checkpoint shapes (BASELINE.json configs[1]); generator + triad compositing "
                                   f"to uint8 RGBA; geometry features precomputed",
                       "batch_per_gpu": B, "resolution": args.res, "gflop_per_patch": round(2 * cfg.macs_per_patch() / 1e9, 3),
                       "parallelism": f"patch-parallel x{world}" + ("" if not use_pg else
                                                                   (f" + {'RCCL' if backend == 'nccl' else backend} gather of RGBA tiles to rank 0 "
                                                                    f"inside every step (rank 0 receives {world - 1} x {B * args.res * args.res * 4 / 1e6:.1f} MB "
                                                                    f"per step; see gather_wait_ms / ms_per_step_per_rank / rccl)") if gather else " (NO gather: --no-gather)")},
            "schedule": prim["schedule"],
            **({"debug_switches": dbg_env} if dbg_env else {}),
            **({"box_calibration": calib, "telemetry": prim.get("telemetry"), "roofline": prim["roofline"]} if args.full else {}),
            "roofline_whole_step": prim["roofline_whole_step"],
            "rehearsal_ms_per_step": prim["rehearsal_ms_per_step"],
            "burn_in_ms_per_step": prim["burn_in_ms_per_step"],
        }
        for k_ in ("value_single_stream", "single_stream", "streams", "stream_probe"):
            if k_ in prim:
                out[k_] = prim[k_]
        if use_pg:
            out["rccl"] = fabric
            out["ms_per_step_per_rank"] = prim.get("ms_per_step_per_rank")
            out["gather_wait_ms"] = prim.get("gather_wait_ms")
        if args.full:
            if "h3" in results:
                # SURVEY 8(d)'s "fp32 parity mode": every fp32 product to ~2^-22 (5e-6 on pixels), the same grade as an fp32 evaluation
                out["value_fp32_parity"] = results["h3"]["value"]
                out["value_fp32_parity_what"] = "patches/s of mode h3 (fp32-grade products: 5e-6 from an all-fp32 evaluation); f32 = exact fp32 MFMA"
            out["modes"] = {m: {k: v for k, v in r.items()} for m, r in results.items()}
            if world == 1 and not args.no_latency:
                out["latency_batch1"] = latency_batch1(G, cfg, dev, geom, pos)
            if world == 1 and not args.no_cpu:
                out["cpu_baseline"] = cpu_baseline(cfg, sd, seconds_budget=args.cpu_seconds, gens=gens, dev=dev)
                for m, pr in out["cpu_baseline"].pop("parity_by_mode", {}).items():
                    out["modes"][m]["parity"] = pr
                out["cpu_baseline"]["parity"] = out["modes"][args.conv_mode].get("parity")
        # The full record (calibration tables, per-layer times, every explanatory string: ~20 KB) goes to a FILE; stdout gets ONE
        # compact line (< 4 KB) with the contract's keys -- the driver keeps only the last 8 KB of stdout, and a 20 KB line
        # left its round-4 record unparseable.
        detail_path = args.detail or os.path.join(REPO, "bench_detail.json")
        try:
            with open(detail_path, "w") as f:
                json.dump(out, f)
            out["detail_file"] = os.path.relpath(detail_path, REPO)
        except OSError as e:
            out["detail_file"] = f"(not written: {e})"
        final_line = json.dumps(out) if args.full_line else fit_line(compact_line(out))
        if dumped is not None:
            files = dump_outputs(args.dump_outputs, dumped)
            print(f"[bench] outputs of the last timed step ({args.conv_mode}) written to {args.dump_outputs}: {files}", file=sys.stderr, flush=True)
    if sampler is not None:
        sampler.__exit__(None, None, None)
    if use_pg:
        dist.barrier()
        dist.destroy_process_group()
        _launch.flush_c_stdio()
    if rank == 0:
        # the LAST thing this job writes to stdout: after the process group is gone and every C-side buffer is out
        print(final_line, flush=True)


if __name__ == "__main__":
    main()
