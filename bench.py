#!/usr/bin/env python3
"""Headline benchmark: GCN max-cut training epochs/sec + SpMM achieved HBM GB/s on
n=1000 d=7 regular graphs (BASELINE.json), one process per GPU.

    python bench.py --gpus N --steps K --warmup W [--full]   (N > 1: spawns the N ranks itself)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times the K steps, writes --dump-outputs and prints the headline line.  --full adds
every region below that is not the headline; the headline's timed steps compute and time the same in both.

A *step* is one pass of the hot path (forward, cut loss, backward, RCCL gradient all-reduce
when N > 1, fused Adam) over this rank's batch of graphs; inputs are resident in HBM before
the timed region.  Workload at N=1: config[3] of BASELINE.json on one GPU - 160 synthetic
n=1000 d=7 graphs (R = 160,000 rows, 646 MB algorithmic bytes per F=500 SpMM, beyond the
256 MiB Infinity Cache).  `value` counts epochs of 160 graphs per second.  --scaling weak
(default): every rank holds its own 160 graphs (N*160 graphs per step); --scaling strong: the 160
graphs are split over the ranks (160/N each - BASELINE config[3] literally at N=8).  With --full and N > 1 the
line of a weak run also carries `strong_scaling`, the same job re-timed on the strong split, and
`allreduce_ms_per_step`.

With --full the JSON line also carries
  roofline      - the DOMINANT KERNEL OF THE TIMED STEP (the fused backward or forward of layer 1): the bytes it must
                  move per launch (compulsory = algorithmic: H once + tables + partials) / its mean launch duration,
                  HIP events recorded by the library on the launch stream over K eager steps; `traffic` = PMC bytes
                  from profiles/traffic_fused.json when that file was measured on these very kernel sources (else
                  null); `lds` = the same launch priced on LDS bytes (gathers + tile writes) against the LDS peak -
                  the resource the fused kernels' time actually goes into (`limited_by`); the other fused kernel
                  under `also`;
  roofline_spmm - the SpMM the metric names (LDS-tiled CSR SpMM of the layer-1 aggregation, forward + backward
                  launches of a region of K steps run as one kernel per operation, gmc_set_fuse(0)) on SURVEY 8(d)'s
                  algorithmic bytes, plus `by_batch`: the same kernel at B = 1 / 20 / 160 / 1024 graphs;
  other_workloads - the same step on 160 x n=1000 graphs of degree 8, degree 12 and G(n, p=0.01) graphs (the
                  reference's generator, GraphCreator.py:70-78): ms per step, per-kernel us, parity gate;
  dp_shard_profile - the data-parallel step sequence on ONE rank over RCCL at the strong split's shard sizes
                  (20 / 40 / 80 / 160 graphs), eager launches vs hipGraphs: ms per step, per-kernel us, host
                  enqueue time, single-rank all-reduce us (N = 1 runs only; a model input, not a scaling claim);
  sequential    - the reference's own schedule (one Adam step per graph, TrainingNeural.py:371-386)
                  on the same 160 graphs, one hipGraph per epoch: the like-for-like partner of
  cpu_baseline  - the CPU oracle timed on this box's host cores on a bounded sample, rank 0, N=1 only:
                  variant A = oracle/ref_dense.py (reference-structured torch-CPU port: dense [n,1000]
                  GEMM, per-row Python one-hot, dense loss, one Adam step per graph) at torch's default
                  thread count, at 16 and at 1 thread (`value` = the best of them, `cores` says which);
                  variant B = oracle/gcn_oracle.c (scalar C: CSR SpMM, fused
                  argmax / loss), 1 thread.  Both GPU/CPU ratios are printed (neither is a quality claim).

Order of the regions inside a --full run: graph generation (worker processes, before the GPU is touched), `sequential`,
the per-kernel probe (150 untimed + K eager steps with HIP events around every kernel), the one-kernel-per-operation
leg (10 untimed + K probed steps) + SpMM batch sweep, the other workloads, the data-parallel shard profile, and LAST
the headline: W untimed warmup steps, then exactly K timed steps between barrier + synchronize pairs.  A plain run
generates the headline's graphs only and takes the probe's and the one-kernel-per-operation leg's steps without HIP
events: they train the model the timed steps start from.  In place of the profile it pauses as long as a --full run
idles before its timed steps (PAUSE_BEFORE_HEADLINE_S): after such a pause the chip runs ~100 steps slower than
sustained, so a short run's figure depends on it.  After the timed steps, --full adds the strong split, the
all-reduce time, the CPU baselines and the parity gate.

--dump-outputs DIR: after the timed steps, rank 0 writes what the last of them computed as DIR/<name>.npy (float32, the
loss float64; see `step_outputs`).  Inputs and initial weights are seeded and the kernels sum in a fixed order, so runs
with the same arguments give the same arrays: two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.distributed as dist

EPOCH_GRAPHS = 160  # BASELINE.json configs[3]
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s HBM3E
LDS_PEAK_GBS = 256 * 256 * 2.4  # MI355X_MICROARCH.md, LDS: 256 B/clk/CU x 256 CUs x 2.4 GHz max clock = 157,286 GB/s
DUMP_LIMIT_BYTES = 64 << 20  # --dump-outputs: at most this much in all
PAUSE_BEFORE_HEADLINE_S = 0.2  # plain run: the idle time a --full run has before its timed steps


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--graphs-per-gpu", type=int, default=None,
                    help="default: 160 (weak scaling) or 160 / N (strong scaling)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak: 160 graphs per GPU; strong: 160 graphs in total (BASELINE configs[3] at N=8)")
    ap.add_argument("--nodes", type=int, default=1000, help="nodes per graph")
    ap.add_argument("--degree", type=int, default=7)
    ap.add_argument("--hidden", type=int, default=500)
    ap.add_argument("--mode", choices=["batched", "sequential"], default="batched",
                    help="batched: one Adam step per rank-batch (DP schedule); sequential: the "
                         "reference's one Adam step per graph (N=1 only)")
    ap.add_argument("--full", action="store_true",
                    help="also run every region beyond the headline: reference schedule, per-kernel HIP events and "
                         "rooflines, SpMM batch sweep, other workloads, data-parallel profile, strong scaling, "
                         "all-reduce time, CPU baselines and parity gate")
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="budget of EACH CPU baseline sample (three are timed)")
    ap.add_argument("--no-sequential", action="store_true", help="skip the reference-schedule region (--full)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the CPU baselines (--full)")
    ap.add_argument("--no-probe", action="store_true",
                    help="skip the probe and one-kernel-per-operation regions, their steps included")
    ap.add_argument("--no-other-workloads", action="store_true", help="skip the d=8 / d=12 / G(n,p) steps (--full)")
    ap.add_argument("--no-dp-profile", action="store_true", help="skip the single-rank data-parallel shard profile (--full)")
    ap.add_argument("--no-spmm-sweep", action="store_true", help="skip the SpMM batch-size sweep (--full)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last of them computed (loss, per-graph losses, "
                         "probabilities, partition, parameters and gradient) as DIR/<name>.npy (rank 0)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def regular_graph(n, d, seed):
    """Synthetic input of SURVEY section 8d: nx.random_regular_graph + unit weights, the
    reference's generator (DataGenerator/GraphCreator.py:70-90) restated."""
    import networkx as nx
    tmp = nx.convert_node_labels_to_integers(nx.random_regular_graph(d=d, n=n, seed=seed))
    g = nx.Graph()
    g.add_nodes_from(sorted(tmp.nodes()))
    g.add_edges_from(tmp.edges)
    nx.set_edge_attributes(g, 1, "weight")
    nx.set_edge_attributes(g, 1, "capacity")
    return g


def gnp_graph(n, p, seed):
    """G(n,p) as the reference's generator builds it (GraphCreator.py:76: graph_type 'prob' = fast_gnp_random_graph),
    re-drawn with another seed while a node is isolated (DGL's GraphConv refuses zero in-degree nodes)."""
    import networkx as nx
    while True:
        tmp = nx.convert_node_labels_to_integers(nx.fast_gnp_random_graph(n, p, seed=seed))
        if min(d for _, d in tmp.degree()) > 0:
            break
        seed += 100000
    g = nx.Graph()
    g.add_nodes_from(sorted(tmp.nodes()))
    g.add_edges_from(tmp.edges)
    nx.set_edge_attributes(g, 1, "weight")
    nx.set_edge_attributes(g, 1, "capacity")
    return g


def _make_graph(spec):
    kind, n, par, seed = spec
    return regular_graph(n, par, seed) if kind == "reg" else gnp_graph(n, par, seed)


def generate(specs):
    """networkx graphs of [(kind, n, degree-or-p, seed), ...] on a few worker processes.  Called BEFORE this process
    touches the GPU (forked workers and an initialised HIP runtime do not mix)."""
    import multiprocessing as mp
    workers = max(1, min(8, (os.cpu_count() or 2) // 2, len(specs)))
    # Under a counter-collecting profiler (rocprofv3 --pmc) the profiler's preloaded library has initialised the GPU
    # before this program's first line: forked workers then hang now and then (two of two passes of this round, on
    # exit).  Generate in this process there - a profiled run is not timed from the outside.
    if os.environ.get("GCN_MAXCUT_BENCH_SERIAL_GEN") == "1" or "rocprof" in os.environ.get("LD_PRELOAD", "").lower() \
            or any(k.startswith("ROCPROFILER_") or k.startswith("ROCPROF_") for k in os.environ):
        workers = 1
    if workers == 1:
        return [_make_graph(sp) for sp in specs]
    with mp.get_context("fork").Pool(workers) as pool:
        return pool.map(_make_graph, specs, chunksize=max(1, len(specs) // (4 * workers)))


def terminals_of(n, seed):
    """Three seeded terminals (the reference draws them unseeded, GraphCreator.py:109); a draw holding two or more
    of the nodes 0, 1, 2 is drawn again - process_graphs_from_folder SKIPS such a graph (graphExtender.py:72-97)."""
    import random
    while True:
        t = random.Random(seed).sample(range(n), 3)
        if len(set(t) & {0, 1, 2}) < 2:
            return t
        seed += 100000


def csrc_fingerprint():
    """sha256 over the kernel sources' CODE (comments and blank lines dropped): profiles/traffic_*.json carry the
    fingerprint they were measured on, and a PMC figure is quoted only for the code it belongs to."""
    import glob
    import hashlib
    import re
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "gcn-max-cut_amd", "csrc", "*.hip")) +
                    glob.glob(os.path.join(ROOT, "gcn-max-cut_amd", "csrc", "*.h"))):
        text = open(f, "r", encoding="utf-8").read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)                       # block comments
        text = re.sub(r"//[^\n]*", "", text)                                    # line comments (no '//' inside the kernels' strings)
        code = "\n".join(ln.rstrip() for ln in text.splitlines() if ln.strip())
        h.update(os.path.basename(f).encode())
        h.update(code.encode())
    return h.hexdigest()[:16]


def free_port():
    import socket
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        return sock.getsockname()[1]


def self_launch(args) -> int:
    """`bench.py --gpus N` without a rendezvous environment: start the N ranks as CHILD processes
    (torch.distributed.run) before this process has touched a GPU, hand their output through and return
    their exit status.  Nothing here initialises HIP (device_count() does not)."""
    import subprocess
    rehearse = os.environ.get("GCN_MAXCUT_BENCH_REHEARSE") == "1"
    have = torch.cuda.device_count()
    if have < (1 if rehearse else args.gpus):
        print(f"bench.py: --gpus {args.gpus} but {have} HIP device(s) visible; refusing to launch "
              f"(set GCN_MAXCUT_BENCH_REHEARSE=1 to rehearse N ranks on one device over gloo)", file=sys.stderr)
        return 2
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    # --standalone: torch.distributed.run brings up its own rendezvous store on a port IT finds free (nothing is probed
    # here and handed over later, which another process could grab in between); --local-addr: the container's hostname
    # may not resolve
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
           f"--nproc-per-node={args.gpus}", os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # rehearsal aid (one-GPU boxes): GCN_MAXCUT_BENCH_REHEARSE=1 puts every rank on device 0 and uses
    # gloo, to exercise the N > 1 control flow; never set by the driver
    rehearse = os.environ.get("GCN_MAXCUT_BENCH_REHEARSE") == "1"
    if rehearse:
        local = 0
    # GCN_MAXCUT_DP_SINGLE_RANK=1 (one-GPU boxes): ONE rank over RCCL runs the data-parallel step sequence -
    # communicator set-up, the collective on the launch stream and graph capture beside RCCL's threads
    single_dp = world == 1 and os.environ.get("GCN_MAXCUT_DP_SINGLE_RANK") == "1"
    dp = world > 1 or single_dp
    if args.mode == "sequential" and world > 1:
        raise SystemExit("sequential mode is the single-GPU reference schedule")
    if args.graphs_per_gpu is None:
        args.graphs_per_gpu = EPOCH_GRAPHS if args.scaling == "weak" else max(1, EPOCH_GRAPHS // world)
    gpg, n, d = args.graphs_per_gpu, args.nodes, args.degree

    # ---- synthetic inputs, generated on worker processes BEFORE this process touches the GPU
    extras_on = (args.full and not dp and args.mode == "batched" and not args.no_other_workloads and not args.no_probe)
    seeds = [3000 + rank * gpg + i for i in range(gpg)]
    specs = [("reg", n, d, sd) for sd in seeds]
    extra_defs = []
    n_other = EPOCH_GRAPHS if gpg >= EPOCH_GRAPHS else gpg   # (reduced runs, e.g. the contract test: as many as the headline)
    if extras_on:   # GraphCreator.py:70-78,151-152: regular graphs of degree min..max and G(n,p) graphs
        extra_defs = [("d8", "reg", 8, 8000, f"{n_other} x n={n} d=8 regular graphs (8-slot table, every slot live)"),
                      ("d12", "reg", 12, 12000, f"{n_other} x n={n} d=12 regular graphs (16-slot table, 12 live)"),
                      ("gnp", "gnp", 10.0 / n, 20000, f"{n_other} x G(n={n}, p={10.0 / n:g}) graphs, mean degree 10 "
                       "(GraphCreator 'prob'; 16-slot table + overflow lists for the rows beyond 16)")]
        for _name, kind, par, base, _what in extra_defs:
            specs += [(kind, n, par, base + i) for i in range(n_other)]
        # BASELINE configs[1]: a batch of 20 x n = 500 graphs of degree 6..8 (the reference pipeline's own mix,
        # GraphCreator.py:151-152) - half-size graphs run the 32-column tiles
        c1_n, c1_count = max(50, n // 2), min(20, n_other)
        specs += [("reg", c1_n, 6 + i % 3, 30000 + i) for i in range(c1_count)]
    t_gen = time.perf_counter()
    if rank == 0:
        print(f"[bench] generating {len(specs)} graphs", file=sys.stderr, flush=True)
    made = generate(specs)
    t_gen = time.perf_counter() - t_gen
    if rank == 0:
        print(f"[bench] graphs generated in {t_gen:.1f} s", file=sys.stderr, flush=True)
    graphs = dict(enumerate(made[:gpg]))
    terms = {i: terminals_of(n, s) for i, s in enumerate(seeds)}

    torch.cuda.set_device(local)
    backend = None
    if dp:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if single_dp:
            os.environ.setdefault("MASTER_PORT", str(free_port()))
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if rehearse:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        backend = dist.get_backend()
        world = dist.get_world_size()      # what the collective library saw, not what the flag said

    import gcn_max_cut_amd as pkg
    from gcn_max_cut_amd.DataGenerator import graphExtender as GE
    from gcn_max_cut_amd.Training import TrainingNeural as T

    def extend(gs, ts):
        with contextlib.redirect_stdout(io.StringIO()):
            ds = GE.process_graphs_from_folder(gs, ts, 1000)
        assert len(ds) == len(gs), "a synthetic graph was skipped by the terminal normalisation"
        return ds

    dataset = extend(graphs, terms)
    cfg = T.TrainingConfig(n_nodes=1000, hidden_dim=args.hidden, number_epochs=10 ** 9, patience=10 ** 9)

    def fresh_model():
        torch.manual_seed(0)  # CPU RNG: identical Xavier init on every rank
        net_, embed_, opt_ = T.setup_model_and_optimizer(cfg)
        net_.train()
        return net_, embed_, opt_

    net, embed, opt = fresh_model()
    gps = gpg if args.mode == "batched" else 1
    trainer = T.FusedTrainer(net, opt, cfg, graphs_per_step=gps, local_shard=True)
    trainer.prepare(dataset)
    eng = trainer.eng
    spmm_bytes = trainer._batches[0].spmm_bytes(eng.Fp)

    def sync():
        if dist.is_initialized():
            dist.barrier()
        torch.cuda.synchronize()

    t_start = time.perf_counter()

    def note(what):   # region timings on stderr (the JSON line is the only thing on stdout)
        if rank == 0:
            print(f"[bench +{time.perf_counter() - t_start:6.1f}s] {what}", file=sys.stderr, flush=True)

    def timed(tr, data, warmup, steps):
        """W untimed steps, then EXACTLY K steps between barrier + synchronize pairs; max over ranks."""
        loss = None
        for _ in range(warmup):
            tr.epoch(data)
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = tr.epoch(data)
        sync()
        dt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device="cuda")
        if dist.is_initialized():
            dist.all_reduce(dt, op=dist.ReduceOp.MAX)
        return float(dt.item()), loss

    def probed(tr, data, untimed, steps, record=True):
        """Per-kernel mean milliseconds over `steps` eager steps (HIP events recorded by the library on the launch
        stream around every kernel; a graph replay cannot carry them), after `untimed` eager steps.  `record=False`
        takes the same steps without the events and returns nothing."""
        was = tr.allow_graph
        tr.allow_graph = False
        for _ in range(untimed):
            tr.epoch(data)
        sync()
        if not record:
            for _ in range(steps):
                tr.epoch(data)
            sync()
            tr.allow_graph = was
            return None
        te = time.perf_counter()
        with pkg.hip.Probe(16 * max(1, len(tr._batches)) * steps) as probe:
            for _ in range(steps):
                tr.epoch(data)
            sync()
        wall_ms = 1e3 * (time.perf_counter() - te) / steps
        tr.allow_graph = was
        by = {}
        for tag, ms in probe.records:
            by.setdefault(tag, []).append(ms)
        return {k: float(np.mean(v)) for k, v in by.items()}, by, wall_ms

    # Order of the regions: the reference-schedule run, the per-kernel probe and the one-kernel-per-operation leg
    # come FIRST, the headline's W warmup + K timed steps LAST: a freshly started process needs ~30 steps (7 ms)
    # to reach the clocks the chip sustains, and training throughput is a sustained quantity.
    # the reference's own schedule on the same graphs: one Adam step per graph (TrainingNeural.py:371-386),
    # one hipGraph per epoch - what `cpu_baseline` (same schedule, host cores) is to be compared with
    sequential = None
    if args.full and not dp and args.mode == "batched" and not args.no_sequential:
        net_s, embed_s, opt_s = fresh_model()
        tr_q = T.FusedTrainer(net_s, opt_s, cfg, graphs_per_step=1, local_shard=True)
        k_seq = max(3, args.steps // 10)
        dt, _ = timed(tr_q, dataset, 2, k_seq)
        sequential = {"value": k_seq * gpg / EPOCH_GRAPHS / dt, "unit": f"epochs/s (1 epoch = {EPOCH_GRAPHS} graphs)",
                      "ms_per_epoch": 1e3 * dt / k_seq, "us_per_graph_step": 1e6 * dt / (k_seq * gpg),
                      "optimizer_steps_per_epoch": gpg, "epochs_timed": k_seq,
                      "schedule": "one Adam step per graph, dataset order (reference schedule), hipGraph per epoch"}
        del tr_q, net_s, embed_s, opt_s
        note("reference-schedule region done")

    # per-kernel means of the default (fused) step: 150 untimed eager steps (kernel set-up; ~40 ms of full load bring
    # the chip to its sustained clocks after the light reference-schedule region), then K probed ones -> `roofline`.
    # These steps and those of the next region train the model the timed steps start from: a run without --full takes
    # them too, without the HIP events, so that its timed steps compute what those of a --full run compute.
    kmean, eager_ms = {}, None
    if not args.no_probe:
        if args.full:
            kmean, _by, eager_ms = probed(trainer, dataset, 150, args.steps)
        else:
            probed(trainer, dataset, 150, args.steps, record=False)

    # third region (EVERY rank runs it: each step holds a collective when N > 1): the same step as
    # one kernel per operation -> timings of the stand-alone SpMM kernel
    spmm, k2 = [], {}
    lib = pkg.hip.load()
    if args.mode == "batched" and not args.no_probe:
        prev = lib.gmc_set_fuse(0)
        if args.full:
            _m, k2, _w = probed(trainer, dataset, 10, args.steps)
        else:
            probed(trainer, dataset, 10, args.steps, record=False)
        lib.gmc_set_fuse(prev)
        spmm = [ms for tag in ("agg_fwd", "agg_bwd") for ms in k2.get(tag, [])]
        note("probe + one-kernel-per-operation regions done")

    # SpMM at several batch sizes ("config 3 must be reported at several batch sizes"):
    # B = 1024 is the 160 graphs repeated (R = 1,024,000 rows, 4.1 GB per [R, F] operand: nothing can be cache-served)
    by_batch = None
    if args.full and not dp and args.mode == "batched" and not args.no_probe and not args.no_spmm_sweep and gpg >= 20:
        by_batch = {}
        keys = list(dataset)
        prev = lib.gmc_set_fuse(0)
        for B in (1, 20, min(160, gpg), 1024):
            try:   # (an extra: e.g. an allocation failure at B = 1024 must not cost the run its headline)
                sub = {i: dataset[keys[i % len(keys)]] for i in range(B)}
                net_b, embed_b, opt_b = fresh_model()
                tr_b = T.FusedTrainer(net_b, opt_b, cfg, graphs_per_step=B, local_shard=True)
                steps_b = 10 if B >= 1024 else 40
                _m, kb, _w = probed(tr_b, sub, 5, steps_b)
                durs = [ms for tag in ("agg_fwd", "agg_bwd") for ms in kb.get(tag, [])]
                alg = tr_b._batches[0].spmm_bytes(tr_b.eng.Fp)
                dur = float(np.mean(durs)) * 1e-3
                by_batch[str(B)] = {"rows": tr_b._batches[0].R, "algorithmic_bytes_per_launch": alg, "mean_launch_us": dur * 1e6,
                                    "achieved_GBps": alg / dur / 1e9, "frac": alg / dur / 1e9 / HBM_PEAK_GBS,
                                    "workgroups": tr_b._batches[0].B * lib_groups(pkg, tr_b._batches[0], tr_b.eng.Fp),
                                    "launches": len(durs)}
                del tr_b, net_b, embed_b, opt_b, sub
            except Exception as e:   # noqa: BLE001
                by_batch[str(B)] = {"error": f"{type(e).__name__}: {e}"[:300]}
            torch.cuda.empty_cache()
        lib.gmc_set_fuse(prev)
        note("SpMM batch sweep done")

    # the same step on other degrees / graph families (N = 1): a 7-slot specialisation must not be the only evidence
    other = None
    if extras_on:
        other = {}
        off = gpg
        runs = [(name, what, n, n_other, base) for name, _kind, _par, base, what in extra_defs]
        runs.append(("c1_20x500_d6to8", f"{c1_count} x n={c1_n} regular graphs of degree 6, 7, 8 (BASELINE configs[1]; one batched "
                     "step per epoch of 20 graphs)", c1_n, c1_count, 30000))
        for name, what, n_o, count_o, base in runs:
            gl = dict(enumerate(made[off:off + count_o]))
            off += count_o
            try:   # (an extra: must not cost the run its headline)
                ds_o = extend(gl, {i: terminals_of(n_o, base + i) for i in gl})
                net_o, embed_o, opt_o = fresh_model()
                tr_o = T.FusedTrainer(net_o, opt_o, cfg, graphs_per_step=len(ds_o), local_shard=True)
                k_o = max(20, args.steps // 2)
                km_o, _by, _w = probed(tr_o, ds_o, 40, k_o)
                dt_o, loss_o = timed(tr_o, ds_o, 20, k_o)
                b0 = tr_o._batches[0]
                other[name] = {
                    "workload": what, "ms_per_step": 1e3 * dt_o / k_o, "value": k_o * len(ds_o) / EPOCH_GRAPHS / dt_o,
                    "unit": f"epochs/s (1 epoch = {EPOCH_GRAPHS} graphs)", "steps": k_o,
                    "kernels_us": {k: round(1e3 * v, 2) for k, v in sorted(km_o.items())},
                    "directed_edges": b0.nnz, "max_degree": b0.host.max_degree, "table_slots": b0.host.ell_width,
                    "live_slots": b0.host.ell_slots,
                    "overflow_blocks": int(b0.host.ovf_ptr[-1]) if b0.host.ovf_ptr is not None else 0,
                    "overflow_blocks_of_the_fullest_graph": b0.host.ovf_max_blocks,
                    "last_loss": loss_o, "parity": parity_gate(pkg, T, net_o, ds_o, n_graphs=1)}
                del tr_o, net_o, embed_o, opt_o, ds_o
            except Exception as e:   # noqa: BLE001
                other[name] = {"workload": what, "error": f"{type(e).__name__}: {e}"[:300]}
            note(f"other workload {name} done")
            del gl
            torch.cuda.empty_cache()
    del made

    # data-parallel step sequence at the strong split's shard sizes, ONE rank over RCCL (N = 1 runs only)
    dp_profile = None
    profile_on = not dp and args.mode == "batched" and not args.no_dp_profile and not args.no_probe
    if profile_on and args.full:
        try:   # (an extra: whatever goes wrong in it must not cost the run its headline)
            dp_profile = dp_shard_profile(args, pkg, T, cfg, dataset, fresh_model, timed, probed)
        except Exception as e:   # noqa: BLE001
            dp_profile = {"error": f"{type(e).__name__}: {e}"[:400]}
            if dist.is_initialized():
                dist.destroy_process_group()
        note("data-parallel shard profile done")
    elif profile_on:
        # A --full run's timed steps start ~0.2 s after the profile's last launch (its RCCL group is torn down in
        # between), and after such a pause the chip runs the next ~100 steps slower than sustained (DESIGN.md section
        # 6).  A plain run pauses as long in its place: --steps and --warmup time the steps they always have.
        sync()
        time.sleep(PAUSE_BEFORE_HEADLINE_S)

    trainer.allow_graph = True

    # timed region: eager launches queued behind the previous step's backward on one GPU (losses stored into pinned
    # host memory); forward/backward and Adam around the eager all-reduce on N GPUs
    elapsed, last_loss = timed(trainer, dataset, args.warmup, args.steps)
    note("headline timed region done")
    # read back before anything else steps the model (the strong-scaling region below trains it further)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, step_outputs(trainer, last_loss))
        note(f"outputs of the last timed step written to {args.dump_outputs}")

    # N > 1, weak run: the same job on the strong split (160 graphs in total, 160 / N per rank)
    strong = None
    if args.full and dp and args.scaling == "weak" and args.mode == "batched":
        per = min(len(dataset), max(1, EPOCH_GRAPHS // world))
        sub = {k: dataset[k] for k in list(dataset)[:per]}
        tr_s = T.FusedTrainer(net, opt, cfg, graphs_per_step=per, local_shard=True)
        dt, _ = timed(tr_s, sub, max(3, args.warmup // 2), args.steps)
        strong = {"graphs_per_gpu": per, "graphs_per_step": per * world, "ms_per_step": 1e3 * dt / args.steps,
                  "value": args.steps * per * world / EPOCH_GRAPHS / dt, "scaling": "strong"}

    # per-step collective time (events on the launch stream around the eager all-reduce), N > 1
    allreduce_ms = None
    if args.full and dp:
        allreduce_ms = allreduce_time_ms(eng, sync)

    if rank != 0:
        if dp:
            dist.destroy_process_group()
        return

    epochs = args.steps * world * gpg / EPOCH_GRAPHS
    out = {
        "metric": "training epochs/sec (n=1000 d=7 graphs)",
        "value": epochs / elapsed,
        "unit": f"epochs/s (1 epoch = {EPOCH_GRAPHS} graphs)",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {
            "workload": f"{gpg} x n={n} d={d} regular graphs per GPU (BASELINE configs[3]"
                        f"{' on one GPU' if world == 1 else ''}; {world * gpg} graphs per step), "
                        f"GCN 1000->{args.hidden}->3, {args.mode} steps, Adam lr 1e-3",
            "graphs_per_gpu": gpg, "rows_per_gpu": gpg * n, "nnz_per_gpu": gpg * n * d,
            "hidden_dim": args.hidden, "mode": args.mode, "epoch_graphs": EPOCH_GRAPHS,
            "optimizer_steps_per_step": len(trainer._batches),
            "parallelism": f"dp{world}" if dp else "single",
        },
        "backend": backend,
        "last_loss": last_loss,
        "launch": ("hipGraph replay" if trainer._graph is not None else
                   "hipGraphs around the eager all-reduce" if trainer._dp_graph is not None else
                   "eager launches queued behind the previous step's backward (losses stored into pinned host memory)"
                   if getattr(trainer, "_loss_host_dev", None) and not dp else
                   "eager launches around the all-reduce (loss published to pinned host memory ahead of Adam)"
                   if dp and getattr(trainer, "_step_host_dev", None) else "eager"),
        "ms_per_step_eager_probed": eager_ms,
        "host_enqueue_us_per_step": 1e6 * trainer.last_enqueue_s,
        "kernels_ms": {k: round(v, 5) for k, v in sorted(kmean.items())},
        "graph_generation_s": round(t_gen, 2),
        "steady_state_note": "the first ~30 steps of a fresh process run ~9 % slower (clock ramp), and ~100 steps after "
                             "an idle pause up to ~45 % slower; the timed steps follow the probe and "
                             "one-kernel-per-operation steps and a 0.2 s pause (--full: the reference-schedule, sweep, "
                             "other-workload and profile regions, whose RCCL teardown is the pause), so short runs "
                             "time clocks below the sustained ones; DESIGN.md quotes the defaults --steps 200 --warmup 30",
    }
    if allreduce_ms is not None:
        out["allreduce_ms_per_step"] = allreduce_ms
    if strong is not None:
        out["strong_scaling"] = strong
    if sequential is not None:
        out["sequential"] = sequential

    out["roofline"] = step_roofline(kmean, trainer._batches[0], eng, pkg) if kmean else None

    if k2:
        out["kernels_ms_unfused"] = {k: round(float(np.mean(v)), 5) for k, v in sorted(k2.items())}
    if spmm and args.mode == "batched":
        dur = float(np.mean(spmm)) * 1e-3
        achieved = spmm_bytes / dur / 1e9
        out["roofline_spmm"] = {
            "kernel": "spmm_lds_kernel (layer-1 aggregation SpMM, fwd + bwd launches; one-kernel-per-op leg)",
            "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS, "traffic": recorded_traffic("traffic_spmm.json", "hbm_bytes_per_launch", gpg * n, eng.Fp),
            "algorithmic_bytes_per_launch": spmm_bytes, "mean_launch_us": dur * 1e6,
            "launches": len(spmm), "by_batch": by_batch,
        }
    else:
        out["roofline_spmm"] = None
    if other is not None:
        out["other_workloads"] = other
    if dp_profile is not None:
        out["dp_shard_profile"] = dp_profile

    if args.full and not dp and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args, graphs, terms, net)
        if sequential is not None:   # same schedule on both sides: GPU reference-schedule rate / CPU rate (both variants)
            cb = out["cpu_baseline"]
            cb["gpu_sequential_over_cpu"] = sequential["value"] / cb["value"]
            cb["gpu_sequential_over_cpu_variant_B"] = sequential["value"] / cb["variants"]["B_sparse_c_1_thread"]["value"]
            cb["ratio_note"] = ("reported baselines, not quality claims: the first ratio is against the reference-structured "
                                "torch-CPU port at its best thread count, the second against the fastest CPU code in this "
                                "line (scalar C, CSR, 1 thread)")
        out["parity"] = parity_gate(pkg, T, net, dataset)
    print(json.dumps(out), flush=True)
    if dp:
        dist.destroy_process_group()


def step_outputs(trainer, loss):
    """What the last timed step computed, as host arrays: the loss `epoch()` returned, every graph's loss of that
    epoch, the probabilities and partition of its last optimizer step's batch, and the parameters and gradient that
    step left in the model (logical shapes)."""
    eng, last = trainer.eng, trainer._batches[-1]
    if trainer.dp or trainer._dropout() > 0.0:   # these steps keep the per-graph losses in the device slots
        slots = trainer._loss_slots.cpu().numpy()
    else:                                        # single-GPU steps land them in the pinned host buffer
        slots = trainer._loss_host_np
    out = {
        "loss": np.array([loss], np.float64),
        "graph_losses": np.concatenate([slots[i, :b.B] for i, b in enumerate(trainer._batches)]).astype(np.float32),
        "probabilities": trainer._out[0][:last.R].cpu().numpy(),
        "partition": trainer._out[1][:last.R].cpu().numpy().astype(np.float32),
    }
    for prefix, buf in (("param", eng.flat), ("grad", eng.grad)):
        for k, v in eng.views(buf).items():
            out[f"{prefix}.{k}"] = v.contiguous().cpu().numpy()
    return out


def dump_outputs(path, arrays):
    """Write every array as `path/<name>.npy`.  While all of them fit DUMP_LIMIT_BYTES they are written whole; past
    that, an array larger than an equal share of the limit is replaced by a fixed, seeded sample of its rows, whose
    indices go to `<name>.rows.npy`."""
    os.makedirs(path, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    for v in arrays.values():
        assert v.dtype in (np.float32, np.float64), v.dtype
    share = (DUMP_LIMIT_BYTES - 4096 * len(arrays)) // len(arrays)   # (npy headers)
    fits = sum(v.nbytes for v in arrays.values()) <= DUMP_LIMIT_BYTES - 256 * len(arrays)
    for name, v in arrays.items():
        if not fits and v.nbytes > share:
            row_bytes = v.nbytes // v.shape[0]
            k = max(1, share // (row_bytes + 8))
            rows = np.sort(np.random.default_rng(0).choice(v.shape[0], size=k, replace=False))
            np.save(os.path.join(path, f"{name}.rows.npy"), rows.astype(np.float64))
            v = v[rows]
        np.save(os.path.join(path, f"{name}.npy"), v)


def lib_groups(pkg, batch, F):
    """Workgroups per graph of the LDS-tiled SpMM for this batch (what decides how much of the chip a small batch uses)."""
    slices = -(-F // 16)
    per = 4
    while per > 1 and batch.B * (-(-slices // per)) < 128:
        per >>= 1
    return -(-slices // per)


def allreduce_time_ms(eng, sync, reps=20):
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    sync()
    for a, b in evs:
        a.record()
        eng.allreduce_grad()
        b.record()
    sync()
    return float(np.mean([a.elapsed_time(b) for a, b in evs[2:]]))


def recorded_traffic(fname, key, rows, F):
    """PMC traffic of a kernel from profiles/<fname> - only when that record was measured on THESE kernel sources
    (its `csrc_sha` equals the fingerprint of gcn-max-cut_amd/csrc now) and on this shape; else None."""
    path = os.path.join(ROOT, "profiles", fname)
    if not os.path.exists(path):
        return None
    rec = json.load(open(path))
    if rec.get("rows") != rows or rec.get("F") != F or rec.get("csrc_sha") != csrc_fingerprint():
        return None
    return rec.get(key)


def step_roofline(kmean, batch, eng, pkg):
    """`roofline` of the line: the dominant kernel of the TIMED (default, fused) step - the fused layer-1 backward or
    forward - on the bytes it must move, with the LDS line beside the HBM one."""
    R_, F_, N_, nnz = batch.R, eng.Fp, eng.N, batch.nnz
    B, W = batch.B, batch.host.ell_width
    slices = -(-F_ // 16)
    chunks = max(1, min(B, min(16, -(-256 // slices))))
    zparts = lib_groups(pkg, batch, F_)
    Fs = slices * 16
    table = R_ * W * 2
    fused = {}
    defs = (
        ("fwd1_fused", "fwd1_lds_kernel",
         R_ * Fs * 4 + N_ * F_ * 4 + table + R_ * 4 + R_ * 12 * zparts,
         f"H write + W1 + neighbour table + dinv + {zparts} Zpart partials",
         # LDS: gather #1 + gather #2 reads, W1 tile landing + T0 tile writes
         2 * nnz * Fs * 4 + 2 * R_ * Fs * 4),
        ("bwd1_fused", "bwd1_reg_kernel" if W == 8 else "bwd1_lds_kernel",
         R_ * Fs * 4 + R_ * 16 + table + chunks * batch.n_max * F_ * 4 + chunks * F_ * 16,
         f"H read + (GY2, dinv) rows + neighbour table + {chunks} dW1 / column chunk partials",
         # LDS: two gathers' reads, H tile landing + Gs in place (read + write) + U tile write
         2 * nnz * Fs * 4 + 4 * R_ * Fs * 4))
    for tag, kname, compulsory, what, lds_bytes in defs:
        if tag not in kmean:
            continue
        dur = kmean[tag] * 1e-3
        fused[tag] = {
            "kernel": kname, "bound": "hbm", "achieved": compulsory / dur / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": compulsory / dur / 1e9 / HBM_PEAK_GBS,
            "traffic": recorded_traffic("traffic_fused.json", tag, R_, F_),
            "algorithmic_bytes_per_launch": compulsory, "algorithmic_bytes_are": what, "mean_launch_us": dur * 1e6,
            "limited_by": "lds",
            "lds": {"achieved": lds_bytes / dur / 1e9, "peak": LDS_PEAK_GBS, "unit": "GB/s",
                    "frac": lds_bytes / dur / 1e9 / LDS_PEAK_GBS, "bytes_per_launch": lds_bytes,
                    "bytes_are": "ds_read_b128 of the two neighbour gathers (2 x directed edges x padded row of "
                                 "F floats) + tile writes (DMA landing, in-place transform, gather #1 output)",
                    "peak_is": "256 B/clk/CU x 256 CUs x 2.4 GHz (MI355X_MICROARCH.md, LDS); PMC: the array is busy "
                               "59-72 % of wave time, a quarter of it bank conflicts (profiles/)"},
            "in_timed_region": True}
    if not fused:
        return None
    dom = max(fused, key=lambda k: fused[k]["mean_launch_us"])
    return dict(fused[dom], also={k: v for k, v in fused.items() if k != dom})


def dp_shard_profile(args, pkg, T, cfg, dataset, fresh_model, timed, probed):
    """The data-parallel step (shard forward/backward -> all-reduce of [gradient | loss] -> publish -> Adam) on ONE
    rank over RCCL at the shard sizes of the strong split of BASELINE configs[3] (160 graphs over 8 / 4 / 2 / 1 GPUs),
    eager launches against GCN_MAXCUT_DP_GRAPHS=1.  Per-rank times are MEASURED; what N > 1 adds is the collective
    between N ranks, which one GPU cannot measure (DESIGN section 7 carries the model)."""
    import tempfile
    keys = list(dataset)
    saved = {k: os.environ.get(k) for k in ("GCN_MAXCUT_DP_SINGLE_RANK", "GCN_MAXCUT_DP_GRAPHS")}
    store = tempfile.NamedTemporaryFile(prefix="gmc_dp_store_", delete=False)
    store.close()
    os.unlink(store.name)   # (FileStore wants to create it)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    out = {"backend": None, "by_shard": {}}
    try:
        dist.init_process_group("nccl", init_method=f"file://{store.name}", rank=0, world_size=1,
                                device_id=torch.device("cuda", torch.cuda.current_device()))
        out["backend"] = dist.get_backend()
        os.environ["GCN_MAXCUT_DP_SINGLE_RANK"] = "1"
        steps = max(20, min(args.steps, 100))
        shards = [B for B in (20, 40, 80, 160) if B <= len(keys)] or [len(keys)]
        for B in shards:
            sub = {k: dataset[k] for k in keys[:B]}
            rec = {}
            for mode in ("eager", "graphs"):
                os.environ["GCN_MAXCUT_DP_GRAPHS"] = "1" if mode == "graphs" else "0"
                net_d, embed_d, opt_d = fresh_model()
                tr = T.FusedTrainer(net_d, opt_d, cfg, graphs_per_step=B, local_shard=True)
                assert tr.dp
                dt, _ = timed(tr, sub, 20, steps)
                host = []
                for _ in range(20):
                    tr.epoch(sub)
                    host.append(tr.last_enqueue_s)
                rec[mode] = {"ms_per_step": 1e3 * dt / steps, "host_enqueue_us": 1e6 * float(np.median(host))}
                if mode == "eager":
                    km, _by, _w = probed(tr, sub, 10, steps)
                    rec["kernels_us"] = {k: round(1e3 * v, 2) for k, v in sorted(km.items())}
                    rec["kernels_sum_us"] = round(1e3 * sum(km.values()), 2)
                    torch.cuda.synchronize()
                    rec["allreduce_single_rank_us"] = 1e3 * allreduce_time_ms(tr.eng, torch.cuda.synchronize)
                del tr, net_d, embed_d, opt_d
            rec["faster"] = min(("eager", "graphs"), key=lambda m: rec[m]["ms_per_step"])
            out["by_shard"][str(B)] = rec
        out["note"] = ("one rank over RCCL on one GPU: per-rank step time, kernel time, host enqueue time and the "
                       "single-rank collective are measured; the N-rank all-reduce is not (see DESIGN section 7)")
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        with contextlib.suppress(OSError):
            os.unlink(store.name)
    return out


def cpu_model_name() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.lower().startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(args, graphs, terms, net):
    """The oracle as the CPU path on the first graphs of the same workload, reference schedule (one Adam
    step per graph, TrainingNeural.py:371-386).  Variant A: oracle/ref_dense.py, reference-structured
    torch-CPU (dense [n,1000] GEMM, per-row Python one-hot, dense loss, autograd, torch Adam) at all
    threads and at one thread.  Variant B: oracle/gcn_oracle.c, scalar C with CSR SpMM and fused
    argmax / loss (so the comparison is not inflated by the reference's dense waste), one thread."""
    from oracle import c_oracle as CO
    from oracle import ref_dense as R
    import copy
    all_threads = torch.get_num_threads()
    params = R.init_params(1000, args.hidden, 3, seed=0)

    def run_a(threads):
        torch.set_num_threads(threads)
        tr = R.Trainer(params, lr=1e-3)
        t_total, k = 0.0, 0
        for i in sorted(graphs):
            if t_total > args.cpu_seconds or k >= 64:
                break
            g = copy.deepcopy(graphs[i])  # bench graphs were already relabelled in place
            item = [R.graph_from_networkx(g), R.dense_adjacency(g, 1000), g, [0, 1, 2]]
            t0 = time.perf_counter()
            tr.step([item])
            t_total += time.perf_counter() - t0
            k += 1
        torch.set_num_threads(all_threads)
        return t_total, k

    def run_b():
        ct = CO.CTrainer({k: v.numpy() for k, v in params.items()}, lr=1e-3)
        t_total, k = 0.0, 0
        for i in sorted(graphs):
            if t_total > args.cpu_seconds or k >= 160:
                break
            csr = CO.csr_of(graphs[i])
            t0 = time.perf_counter()
            ct.step([csr])
            t_total += time.perf_counter() - t0
            k += 1
        return t_total, k

    def rec(t_total, k, cores, what):
        per = t_total / max(k, 1)
        return {"value": 1.0 / (per * EPOCH_GRAPHS), "cores": cores, "ms_per_graph_step": per * 1e3,
                "sample": f"{k} sequential graph-steps (n={args.nodes} d={args.degree}, hidden {args.hidden}) of {what}, {t_total:.1f} s"}

    what_a = "the reference-structured torch-CPU oracle (variant A)"
    a_all = rec(*run_a(all_threads), all_threads, what_a)
    mid = min(16, all_threads)   # a GPU box hands one GPU's job a share of the host: many more threads than that oversubscribe
    a_mid = rec(*run_a(mid), mid, what_a) if mid not in (1, all_threads) else None
    a_one = rec(*run_a(1), 1, what_a)
    b_one = rec(*run_b(), 1, "the scalar C oracle: CSR SpMM, fused argmax/loss (variant B)")
    variants = {"A_all_threads": a_all, "A_1_thread": a_one, "B_sparse_c_1_thread": b_one}
    if a_mid is not None:
        variants[f"A_{mid}_threads"] = a_mid
    best = max((v for k, v in variants.items() if k.startswith("A_")), key=lambda v: v["value"])
    return {
        # the reference-structured variant at the thread count that serves it best (all of them are listed)
        "value": best["value"], "unit": f"epochs/s (1 epoch = {EPOCH_GRAPHS} graphs)",
        "cores": best["cores"], "kind": "port", "sample": best["sample"],
        "schedule": "one Adam step per graph (reference schedule; compare with `sequential`, not with `value`)",
        "variants": variants,
        "host_cpus": os.cpu_count(), "torch_default_threads": all_threads, "cpu_model": cpu_model_name(),
        "torch": torch.__version__,
    }


def parity_gate(pkg, T, net, dataset, n_graphs=2):
    """Parity numbers reported with every perf number: probabilities
    vs the C oracle on the first graphs of the workload with the current weights."""
    from oracle import c_oracle as CO
    params = {k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()}
    worst, worst_unfused, arg_ok, loss_ok = 0.0, 0.0, True, True
    net.eval()
    for key in list(dataset)[:n_graphs]:
        g, a_pad, nx_g, _t = dataset[key]
        with torch.no_grad():
            P = net(g, a_pad).cpu().numpy()
        rp, cl, vl = CO.csr_of(nx_g)
        ref = CO.forward(rp, cl, vl, params["conv1.weight"], params["conv1.bias"], params["conv2.weight"],
                         params["conv2.bias"])["P"]
        S, loss, _ = CO.loss_grad(rp, cl, vl, ref)
        worst = max(worst, float(np.abs(P - ref).max()))
        # the one-kernel-per-operation sequence (whose SpMM the `roofline` object times) on the same graph
        lib = pkg.hip.load()
        prev = lib.gmc_set_fuse(0)
        try:
            with torch.no_grad():
                P0 = net(g, a_pad).cpu().numpy()
        finally:
            lib.gmc_set_fuse(prev)
        worst_unfused = max(worst_unfused, float(np.abs(P0 - ref).max()))
        arg_ok &= bool(np.array_equal(P.argmax(1)[3:], ref.argmax(1)[3:]))
        res = T.evaluate_model(net, {0: dataset[key]}, T.TrainingConfig())
        loss_ok &= res["total_loss"] == loss
    net.train()
    return {"max_abs_prob_diff": worst, "max_abs_prob_diff_one_kernel_per_op": worst_unfused, "argmax_equal": arg_ok,
            "loss_equals_minus_cut": loss_ok, "tolerance": 1e-4}


if __name__ == "__main__":
    main()
