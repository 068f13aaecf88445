"""The evolution stage (gmc_kway_evolve_f32): what a generation costs next to an annealing call of the same sweeps, and
the cut of search_dataset with generations against plain annealing at equal sweeps per candidate.

    python scratch/evolve_timing.py OUT.json

1. Time on 160 graphs n = 1000 d = 7 (unit weights), K = 3 and 4, 201 candidates that 100 annealing sweeps have already
   brought to local optima: ONE generation (10 sweeps cooling from 0.6, descent 100 at most, elite 50) against ONE
   gmc_kway_refine_anneal_f32 call with the same schedule on the same candidates, from the library's event probe (device
   events around the launch), after a warm-up of both, alternating in one run, 3 windows of 6 calls.  The difference is
   the price of ranking, alignment and crossover (and of whatever the children's descents run longer).  The scoring
   launch of the evolve call is reported beside them.
2. Quality at equal work: the 3-class and 4-class models of scratch/rounding_timing.py (same dataset, same training),
   10 held-out d = 7 regular graphs per size n = 500, 1000, 200 samples (202 candidates).  For a grid of (generations
   G, generation_sweeps s, elite, t_start): mean evolved_cut of search_dataset(anneal_sweeps=100, generations=G,
   generation_sweeps=s) against mean searched_cut of search_dataset(anneal_sweeps=100 + G * s) - both spend the same
   number of annealing sweeps per candidate.  t_start is TN.EVOLVE_T_START, set here per grid point.
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gcn_max_cut_amd import hip  # noqa: E402
from gcn_max_cut_amd.graph import GraphBatch, from_networkx  # noqa: E402
from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN  # noqa: E402
from oracle import ref_dense as R  # noqa: E402
import rounding_timing as RT  # noqa: E402

CANDS, SAMPLES, SWEEPS, GEN_SWEEPS, ELITE, WINDOWS, PER_WINDOW = 201, 200, 100, 10, 50, 3, 6
# (generations, generation_sweeps, elite or None = max(2, cands // 4), t_start)
GRID = [(10, 10, None, 0.6), (5, 10, None, 0.6), (5, 20, None, 0.6), (20, 5, None, 0.6), (10, 10, 10, 0.6),
        (10, 10, 2, 0.6), (10, 10, None, 0.3), (10, 10, None, 1.0), (20, 10, None, 0.6)]


def probed(launch):
    with hip.Probe(8) as pr:
        launch()
    return pr.records


def generation_times(K):
    dev = torch.device("cuda")
    batch = GraphBatch([from_networkx(R.regular_graph(1000, 7, 9000 + i)) for i in range(160)], None, dev)
    p, lib = hip.ptr, hip.load()
    order, cgoff, cptr = batch.refine_order(K)
    levels = torch.from_numpy(TN.anneal_levels()).to(dev)
    starts = np.asarray(batch.goff_host[:-1], np.int64)
    A = np.random.RandomState(K).randint(0, K, (CANDS, batch.R)).astype(np.int8)
    for j in range(K):
        A[:, starts + j] = j
    optima = torch.from_numpy(A).to(dev)
    TN._kway_anneal_on_gpu(batch, K, optima, TN.anneal_schedule(SWEEPS), 1, 100)      # in place: the local optima
    inv_t = torch.from_numpy(TN.anneal_schedule(GEN_SWEEPS, t_start=TN.EVOLVE_T_START)).to(dev)
    work = torch.empty_like(optima)
    pop = torch.empty((2, CANDS, batch.R), dtype=torch.int8, device=dev)
    cut = torch.empty((2, batch.B, CANDS), device=dev)
    cut_all = torch.empty((batch.B, CANDS), device=dev)
    best_assign = torch.empty(batch.R, dtype=torch.int32, device=dev)
    best_cut = torch.empty(batch.B, device=dev)
    best_idx = torch.empty(batch.B, dtype=torch.int32, device=dev)
    history = torch.empty((2, batch.B), device=dev)

    def anneal():
        work.copy_(optima)
        return probed(lambda: hip.check(lib.gmc_kway_refine_anneal_f32(
            batch.ref(), K, p(order), p(cgoff), p(cptr), CANDS, p(work), p(inv_t), GEN_SWEEPS, p(levels), 1, 100,
            p(cut_all), p(best_assign), p(best_cut), p(best_idx), None, None, hip.stream()), "kway anneal"))

    def generation():
        pop[0].copy_(optima)
        return probed(lambda: hip.check(lib.gmc_kway_evolve_f32(
            batch.ref(), K, p(order), p(cgoff), p(cptr), CANDS, p(pop), p(cut), 1, ELITE, p(inv_t), GEN_SWEEPS, p(levels), 1,
            100, p(best_assign), p(best_cut), p(best_idx), p(history), hip.stream()), "kway evolve"))
    anneal(), generation()
    torch.cuda.synchronize()
    gained = dict(mean_best_before=float(history[0].mean()), mean_best_after_one_generation=float(history[1].mean()),
                  mean_best_after_the_annealing_call=float(best_cut.mean()))
    ms = dict(anneal_call=[], generation=[], scoring=[])
    for _ in range(WINDOWS * PER_WINDOW):
        ms["anneal_call"].append([t for name, t in anneal() if name == "anneal"][0])
        rec = generation()
        ms["generation"].append([t for name, t in rec if name == "anneal"][0])
        ms["scoring"].append([t for name, t in rec if name == "sample"][0])
    torch.cuda.synchronize()
    out = {name: RT.summary(v) for name, v in ms.items()}
    out.update(K=K, B=batch.B, R=batch.R, candidates=CANDS, sweeps=GEN_SWEEPS, elite=ELITE, **gained,
               staged=int(lib.gmc_refine_anneal_staged(batch.ref())),
               generation_over_anneal_call=out["generation"]["kernel_ms_median"] / out["anneal_call"]["kernel_ms_median"])
    return out


def quality(net, K):
    rec = {}
    mean = lambda res, key: float(np.mean([r[key] for r in res]))   # noqa: E731
    for n in (500, 1000):
        ds = RT.dataset([(n, 7, 5000 + 10 * n + i) for i in range(10)], K)
        plain = {}
        for total in sorted({SWEEPS} | {SWEEPS + G * s for G, s, _e, _t in GRID}):
            plain[total] = mean(TN.search_dataset(net, ds, SAMPLES, anneal_sweeps=total), "searched_cut")
        points = []
        for G, s, elite, t_start in GRID:
            TN.EVOLVE_T_START = t_start
            res = TN.search_dataset(net, ds, SAMPLES, anneal_sweeps=SWEEPS, generations=G, generation_sweeps=s, elite=elite)
            points.append(dict(generations=G, generation_sweeps=s, elite=elite, t_start=t_start,
                               evolved=mean(res, "evolved_cut"), searched_before=mean(res, "searched_cut"),
                               plain_annealing_at_equal_sweeps=plain[SWEEPS + G * s],
                               graphs_better=sum(r["evolved_cut"] > r["searched_cut"] for r in res)))
            points[-1]["evolved_minus_plain"] = points[-1]["evolved"] - points[-1]["plain_annealing_at_equal_sweeps"]
            print(K, n, points[-1], flush=True)
        rec[str(n)] = dict(plain_annealing_by_sweeps={str(k): v for k, v in plain.items()}, grid=points, graphs=10,
                           edges=int(n * 7 // 2))
    return rec


def main():
    out_path = sys.argv[1]
    hip.require_gpu()
    default_t = TN.EVOLVE_T_START
    rec = {"one_generation_on_160_graphs_n1000_d7": {f"K{K}": generation_times(K) for K in (3, 4)}}
    print(rec, flush=True)
    rec["quality_d7_mean_cut_per_size"] = {}
    for K in (3, 4):
        with tempfile.TemporaryDirectory() as workdir:      # (the dataset pickles hold dense [n, 1000] adjacencies)
            net, info = RT.train(workdir, K, "cut")
            rec[f"model_K{K}"] = info
            rec["quality_d7_mean_cut_per_size"][f"K{K}"] = quality(net, K)
    TN.EVOLVE_T_START = default_t
    rec["method"] = (f"times: hip.Probe (device events around the launch), both calls warmed up, alternating in one run, "
                     f"{WINDOWS} windows of {PER_WINDOW} calls; quality: search_dataset with {SAMPLES} samples (sample_seed 0, "
                     f"anneal_seed 0), 202 candidates, {SWEEPS} annealing sweeps before the generations")
    rec["device"] = torch.cuda.get_device_name(0)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
