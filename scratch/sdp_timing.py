"""The semidefinite relaxation (gmc_sdp_relax_f32 / gmc_sdp_round_f32, maxcut.solve_sdp): what it costs and what it finds.

    python scratch/sdp_timing.py OUT.json [--skip-quality]

1. Relaxation.  160 graphs n = 1000 d = 7 (unit weights) and the first of them alone, ranks 16, 32, 64: one call of 10
   and one of 60 sweeps (init and value included in both), device events around loops of CALLS calls, ROUNDS loops,
   median; time per sweep = the difference over 50, per launch = that over max_classes.  Bytes of a sweep, from the
   shapes: per node its neighbours' rows (deg * rank * 4), its own row written (rank * 4), its CSR entries (deg * 4, no
   values: unit weights), two rowptr words and its order word - against the HBM peak of 8 TB/s, though V (41 MB at rank
   64) stays in the caches.
2. Rounding.  200 planes on the same batches.
3. Against the trained solver.  The held-out 7-regular graphs of scratch/tabu_timing.py (10 of n = 1000),
   maxcut.solve_batch at K = 2 without terminals (hidden 64, 200 epochs, lr 1e-2, 34 candidates) against
   maxcut.solve_sdp_batch (rank 64, 50 sweeps, 200 planes), three seeds, alternating: at equal anneal_sweeps (100), and
   at equal wall time - the SDP route is given the annealing sweeps that fill solve_batch's measured wall time (host clock
   around a call that ends in a synchronise).  Also the relaxed value of one graph after 50, 200 and 1000 sweeps and its
   best of 64 planes."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gcn_max_cut_amd import hip, maxcut  # noqa: E402
from gcn_max_cut_amd.graph import GraphBatch, from_networkx  # noqa: E402
from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN  # noqa: E402
from oracle import ref_dense as R  # noqa: E402

CALLS, ROUNDS, SEEDS = 3, 5, 3
HBM_PEAK = 8.0e12


def timed(fn, calls=CALLS, rounds=ROUNDS):
    fn()
    out = []
    for _ in range(rounds):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_time(stop) / calls)
    return dict(ms_median=float(np.median(out)), ms_min=float(min(out)), ms_max=float(max(out)))


def wall(fn, rounds=3):
    fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out))


def relaxation(batch, label):
    rows = []
    classes = batch.refine_classes(2, False)
    keys = maxcut._sdp_keys(batch, 0)
    deg = batch.nnz / batch.R
    for rank in hip.SDP_RANKS:
        t10 = timed(lambda: maxcut._sdp_relax_keys(batch, keys, rank, 10, False, None, None))
        t60 = timed(lambda: maxcut._sdp_relax_keys(batch, keys, rank, 60, False, None, None))
        V, _ = maxcut._sdp_relax_keys(batch, keys, rank, 50, False, None, None)
        t_round = timed(lambda: maxcut._sdp_round_keys(batch, V, keys, 0, 200, False))
        per_sweep = (t60["ms_median"] - t10["ms_median"]) / 50
        sweep_bytes = batch.R * (deg * rank * 4 + rank * 4 + deg * 4 + 12)
        rows.append(dict(batch=label, B=batch.B, R=batch.R, rank=rank, max_classes=classes, launches_per_sweep=classes,
                         call_10_sweeps=t10, call_60_sweeps=t60, ms_per_sweep=per_sweep,
                         us_per_launch=per_sweep * 1e3 / classes, bytes_per_sweep=sweep_bytes,
                         bytes_per_second=sweep_bytes / (per_sweep * 1e-3),
                         share_of_hbm_peak=sweep_bytes / (per_sweep * 1e-3) / HBM_PEAK,
                         round_200_planes=t_round))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def spread(values):
    return dict(mean=float(np.mean(values)), min=float(min(values)), max=float(max(values)))


def quality(dev):
    n = 1000
    batch = GraphBatch([from_networkx(R.regular_graph(n, 7, 5000 + 10 * n + i)) for i in range(10)], None, dev)
    kw = dict(number_classes=2, hidden_dim=64, epochs=200, learning_rate=1e-2)
    rec = dict(graphs=10, n=n, edges=n * 7 // 2, solve_batch=kw, sdp=dict(rank=64, sweeps=50, planes=200))
    t_solve = wall(lambda: maxcut.solve_batch(batch, seed=0, **kw))
    t_sdp = wall(lambda: maxcut.solve_sdp_batch(batch, seed=0))
    t_sdp300 = wall(lambda: maxcut.solve_sdp_batch(batch, seed=0, anneal_sweeps=300))
    ms_per_sweep = (t_sdp300 - t_sdp) / 200
    equal = int(min(max(100 + (t_solve - t_sdp) / ms_per_sweep, 100), 20000))
    t_equal = wall(lambda: maxcut.solve_sdp_batch(batch, seed=0, anneal_sweeps=equal))
    rec.update(solve_batch_wall_ms=t_solve, solve_sdp_wall_ms=t_sdp, sdp_anneal_ms_per_sweep_200_candidates=ms_per_sweep,
               equal_time_anneal_sweeps=equal, solve_sdp_equal_time_wall_ms=t_equal)
    runs = dict(trained=[], sdp=[], sdp_equal_time=[], sdp_rounded=[], sdp_relaxed=[], trained_rounded=[], trained_trained=[])
    for seed in range(SEEDS):                                   # alternating in one run
        t = maxcut.solve_batch(batch, seed=seed, **kw)
        s = maxcut.solve_sdp_batch(batch, seed=seed)
        e = maxcut.solve_sdp_batch(batch, seed=seed, anneal_sweeps=equal)
        runs["trained"].append(float(t.cut.mean()))
        runs["trained_rounded"].append(float(t.rounded_cut.mean()))
        runs["trained_trained"].append(float(t.trained_cut.mean()))
        runs["sdp"].append(float(s.cut.mean()))
        runs["sdp_equal_time"].append(float(e.cut.mean()))
        runs["sdp_rounded"].append(float(s.rounded_cut.mean()))
        runs["sdp_relaxed"].append(float(s.relaxed_value.mean()))
        print("seed", seed, {k: v[-1] for k, v in runs.items()}, flush=True)
    rec["mean_over_graphs_then_seeds"] = {k: spread(v) for k, v in runs.items()}
    rec["per_seed"] = runs
    one = GraphBatch([from_networkx(R.regular_graph(n, 7, 5000 + 10 * n))], None, dev)
    keys = maxcut._sdp_keys(one, 0)
    values = {}
    for sweeps in (50, 200, 1000):
        V, value = maxcut._sdp_relax_keys(one, keys, 64, sweeps, False, None, None)
        planes = maxcut._sdp_round_keys(one, V, keys, 0, 64, False)
        cut = TN._kway_anneal_on_gpu(one, 2, planes.clone(), np.zeros(0, np.float32), 0, 0, False)[1]
        values[str(sweeps)] = dict(value=float(value[0]), best_of_64_planes=float(cut[0]))
    rec["one_graph_rank_64"] = values
    print(json.dumps(rec), flush=True)
    return rec


def main():
    out_path = sys.argv[1]
    hip.require_gpu()
    dev = torch.device("cuda")
    rec = {"device": torch.cuda.get_device_name(0)}

    def save():
        with open(out_path, "w") as f:
            json.dump(rec, f, indent=1)

    handles = [from_networkx(R.regular_graph(1000, 7, 9000 + i)) for i in range(160)]
    rec["relaxation_160_graphs_n1000_d7"] = relaxation(GraphBatch(handles, None, dev), "160 x (n = 1000, d = 7)")
    save()
    rec["relaxation_one_graph_n1000_d7"] = relaxation(GraphBatch(handles[:1], None, dev), "1 x (n = 1000, d = 7)")
    save()
    if "--skip-quality" not in sys.argv:
        rec["against_solve_batch_K2_plain"] = quality(dev)
        save()
    rec["method"] = (f"device events around loops of {CALLS} calls, {ROUNDS} loops, median; per sweep: (60 sweeps - 10 sweeps) / "
                     f"50; wall: host clock around a call ending in a synchronise, median of 3 after a warm-up; {SEEDS} seeds, "
                     f"the two solvers alternating; no default changed")
    save()


if __name__ == "__main__":
    main()
