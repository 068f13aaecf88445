"""The tempering stage (gmc_kway_temper_f32): what a round costs next to an annealing call of the same sweeps, and what
the stage buys at equal time against more annealing sweeps.

    python scratch/temper_timing.py OUT.json [quick]

1. Time on 160 graphs n = 1000 d = 7 (unit weights), K = 2 and 3, with and without a cost array, 200 candidates (25
   ladders of 8) that 100 annealing sweeps have brought to local optima: ONE round of 10 sweeps against ONE
   gmc_kway_refine_anneal_c_f32 call of 10 sweeps (no descent) on the same candidates, from the library's event probe
   (device events around the launch), after a warm-up of both, alternating in one run, 3 windows of 6 calls.
2. Quality at equal time, at the decoders (no model: 200 random starts per graph, so the comparison is the search's
   alone), 10 graphs per family, three seeds: the default annealing (100 sweeps) followed by the stage and the descent,
   against ONE annealing call that is given the stage's milliseconds as extra sweeps (the price of a sweep is measured
   on the same batch from calls of 100 and 300 sweeps; every time is device events around the whole call).  Families:
   7-regular n = 1000 at K = 2 without terminals and at K = 3 with them; the +-1 spin glass on 7-regular graphs
   (n = 1000, K = 2, the ladder and the schedule in units of the mean absolute weight); the G(800, 0.06) QUBO family
   (w = q / 2, q in -2..2 without 0, linear terms -3..3 in the cost array) from a starved (10 sweeps) and from the
   default annealing.  A grid over (rungs, round_sweeps, t_hot) on the spin glass.  The exchange acceptance is the
   accepted exchanges over the tested ones, from `swaps`.
"""
import json
import os
import sys

import networkx as nx
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gcn_max_cut_amd import hip, maxcut  # noqa: E402
from gcn_max_cut_amd.graph import GraphBatch, from_networkx  # noqa: E402
from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN  # noqa: E402
from oracle import ref_dense as R  # noqa: E402

CANDS, RUNGS, SWEEPS, ROUND_SWEEPS, WINDOWS, PER_WINDOW = 200, 8, 100, 10, 3, 6
SEEDS = (0, 1, 2)
GRID = [(8, 4, 1.5), (4, 4, 1.5), (8, 2, 1.5), (8, 8, 1.5), (8, 4, 1.0), (8, 4, 2.5), (20, 4, 1.5)]


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


def probed(launch):
    with hip.Probe(8) as pr:
        launch()
    return [t for name, t in pr.records if name == "anneal"]


def starts(batch, K, terminals, cands, seed):
    A = np.random.RandomState(seed).randint(0, K, (cands, batch.R)).astype(np.int8)
    if terminals:
        first = np.asarray(batch.goff_host[:-1], np.int64)
        for j in range(K):
            A[:, first + j] = j
    return torch.from_numpy(A).to(batch.device)


HANDLES = []


def round_times(K, costly):
    dev = torch.device("cuda")
    if not HANDLES:
        HANDLES.extend(from_networkx(R.regular_graph(1000, 7, 9000 + i)) for i in range(160))
    batch = GraphBatch(HANDLES, None, dev)
    p, lib = hip.ptr, hip.load()
    order, cgoff, cptr = batch.refine_order(K, True)
    levels = torch.from_numpy(TN.anneal_levels()).to(dev)
    cost = None
    if costly:
        cost = torch.from_numpy(np.random.RandomState(3).uniform(-1, 1, (batch.R, K)).astype(np.float32)).to(dev)
    optima = starts(batch, K, True, CANDS, K)
    TN._kway_anneal_on_gpu(batch, K, optima, TN.anneal_schedule(SWEEPS), 1, 100, True, cost)
    ladder = torch.from_numpy(TN.temper_ladder(RUNGS)).to(dev)
    inv_t = torch.from_numpy(np.repeat(TN.temper_ladder(RUNGS)[RUNGS // 2], ROUND_SWEEPS)).to(dev)
    work, best = torch.empty_like(optima), torch.empty_like(optima)
    cut_all, best_assign, best_cut, best_idx = TN._search_outputs(batch, CANDS)
    score = torch.empty((batch.B, CANDS), device=dev)
    ints = [torch.empty((batch.B, CANDS), dtype=torch.int32, device=dev) for _ in range(3)]
    need = int(lib.gmc_kway_temper_workspace_bytes(batch.ref(), CANDS))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def anneal():
        work.copy_(optima)
        return probed(lambda: hip.check(lib.gmc_kway_refine_anneal_c_f32(
            batch.ref(), K, 1, p(cost), p(order), p(cgoff), p(cptr), CANDS, p(work), p(inv_t), ROUND_SWEEPS, p(levels), 1, 0,
            p(cut_all), p(best_assign), p(best_cut), p(best_idx), None, None, hip.stream()), "anneal"))[0]

    def one_round():
        work.copy_(optima)
        return probed(lambda: hip.check(lib.gmc_kway_temper_f32(
            batch.ref(), K, 1, p(cost), p(order), p(cgoff), p(cptr), CANDS, RUNGS, p(ladder), 1, ROUND_SWEEPS, p(levels), 1,
            p(work), p(best), p(score), p(ints[0]), p(ints[1]), p(ints[2]), p(ws), need, hip.stream()), "temper"))[0]

    def second_round():   # the launch of t = 1: the prologue with its exchange, loads of the best state
        work.copy_(optima)
        return probed(lambda: hip.check(lib.gmc_kway_temper_f32(
            batch.ref(), K, 1, p(cost), p(order), p(cgoff), p(cptr), CANDS, RUNGS, p(ladder), 2, ROUND_SWEEPS, p(levels), 1,
            p(work), p(best), p(score), p(ints[0]), p(ints[1]), p(ints[2]), p(ws), need, hip.stream()), "temper"))[1]
    anneal(), one_round(), second_round()
    ms = dict(anneal_call=[], round=[], second_round=[])
    for _ in range(WINDOWS * PER_WINDOW):
        ms["anneal_call"].append(anneal())
        ms["round"].append(one_round())
        ms["second_round"].append(second_round())
    torch.cuda.synchronize()
    out = {k: dict(kernel_ms_median=median(v), kernel_ms_min=float(min(v)), kernel_ms_max=float(max(v)), calls=len(v))
           for k, v in ms.items()}
    out.update(K=K, cost=bool(costly), B=batch.B, candidates=CANDS, rungs=RUNGS, sweeps=ROUND_SWEEPS,
               staged=int(lib.gmc_refine_anneal_staged(batch.ref())),
               round_over_anneal_call=out["round"]["kernel_ms_median"] / out["anneal_call"]["kernel_ms_median"],
               second_round_over_anneal_call=out["second_round"]["kernel_ms_median"] / out["anneal_call"]["kernel_ms_median"])
    return out


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def family(name, graphs_count):
    """(graphs, K, terminals, per-node cost or None, signed)"""
    if name in ("regular_K2", "regular_K3"):
        return [R.regular_graph(1000, 7, 7000 + i) for i in range(graphs_count)], int(name[-1]), name[-1] == "3", None
    if name == "spin_glass":
        gs = []
        for i in range(graphs_count):
            g = nx.random_regular_graph(7, 1000, seed=7100 + i)
            rng = np.random.RandomState(7200 + i)
            for u, v in g.edges():
                g[u][v]["weight"] = float(rng.choice([-2.0, 2.0]))      # w = 2 J, J = +-1
            gs.append(g)
        return gs, 2, False, None
    assert name == "qubo"
    gs, rows = [], []
    for i in range(graphs_count):
        while True:
            g = nx.gnp_random_graph(800, 0.06, seed=7300 + i)
            if min(d for _v, d in g.degree()) > 0:
                break
        rng = np.random.RandomState(7400 + i)
        half = np.zeros(800)
        for u, v in g.edges():
            q = float(rng.choice([-2, -1, 1, 2]))
            g[u][v]["weight"] = 0.5 * q
            half[u] += 0.5 * q
            half[v] += 0.5 * q
        c = np.zeros((800, 2), np.float32)
        c[:, 1] = rng.randint(-3, 4, 800) + half
        gs.append(g)
        rows.append(c)
    return gs, 2, False, np.concatenate(rows)


def equal_time(name, graphs_count, rounds, round_sweeps=4, rungs=RUNGS, t_hot=TN.TEMPER_T_HOT, first_sweeps=SWEEPS):
    dev = torch.device("cuda")
    graphs, K, terminals, cost = family(name, graphs_count)
    batch = GraphBatch([from_networkx(g) for g in graphs], None, dev)
    cost = None if cost is None else torch.from_numpy(cost).to(dev)
    scale = maxcut._mean_abs_edge_weight(batch)
    ladder = TN.temper_ladder(rungs, t_hot, TN.TEMPER_T_COLD, scale)
    none = np.zeros(0, np.float32)
    rec = dict(family=name, graphs=batch.B, K=K, terminals=terminals, cost=cost is not None, candidates=CANDS, rungs=rungs,
               rounds=rounds, round_sweeps=round_sweeps, t_hot=t_hot, annealing_sweeps_before=first_sweeps, seeds=[])

    def anneal(sweeps, seed):
        cands = starts(batch, K, terminals, CANDS, 100 + seed)
        (_, cut, _), ms = timed(lambda: TN._kway_anneal_on_gpu(batch, K, cands, TN.anneal_schedule(sweeps, scale=scale), seed,
                                                               100, terminals, cost))
        return cands, cut, ms
    anneal(first_sweeps, 0)                                                     # warm-up
    per_sweep = median([(anneal(300, s)[2] - anneal(100, s)[2]) / 200 for s in SEEDS])
    for seed in SEEDS:
        cands, annealed, ms_anneal = anneal(first_sweeps, seed)

        def stage():
            out = TN._kway_temper_on_gpu(batch, K, cands.clone(), ladder, rounds, round_sweeps, seed, terminals, cost)
            return out, TN._kway_anneal_on_gpu(batch, K, out[0], none, 0, 100, terminals, cost)[1]
        stage()
        (out, tempered), ms_stage = timed(stage)
        tempered = torch.maximum(tempered, annealed)
        extra = int(round(ms_stage / per_sweep))
        _, longer, ms_longer = anneal(first_sweeps + extra, seed)
        pairs = sum(len(range(t & 1, rungs - 1, 2)) for t in range(1, rounds))
        proposals = pairs * (CANDS // rungs) * batch.B
        rec["seeds"].append(dict(
            seed=seed, annealed=float(annealed.mean()), tempered=float(tempered.mean()), ms_annealing=ms_anneal,
            ms_stage=ms_stage, extra_sweeps_at_equal_time=extra, annealing_at_equal_time=float(longer.mean()),
            ms_annealing_at_equal_time=ms_longer, graphs_tempered_better=int((tempered > longer).sum()),
            graphs_annealing_better=int((longer > tempered).sum()),
            exchange_acceptance=float(out[4].sum()) / 2 / proposals if proposals else None,
            slots_whose_best_came_after_round_0=float((out[2] > 0).float().mean())))
    for key in ("annealed", "tempered", "annealing_at_equal_time"):
        v = [s[key] for s in rec["seeds"]]
        rec[key] = dict(mean=float(np.mean(v)), min=float(min(v)), max=float(max(v)))
    rec["tempered_minus_annealing_at_equal_time"] = rec["tempered"]["mean"] - rec["annealing_at_equal_time"]["mean"]
    rec["ms_per_annealing_sweep"] = per_sweep
    print(json.dumps({k: v for k, v in rec.items() if k != "seeds"}), flush=True)
    return rec


def main():
    out_path = sys.argv[1]
    quick = len(sys.argv) > 2 and sys.argv[2] == "quick"
    hip.require_gpu()
    rec = {"one_round_on_160_graphs_n1000_d7": [round_times(K, c) for K in (2, 3) for c in (False, True)]}
    print(json.dumps(rec), flush=True)
    count = 4 if quick else 10
    rec["equal_time"] = [equal_time(name, count, 50) for name in ("regular_K2", "regular_K3", "spin_glass", "qubo")]
    rec["equal_time"].append(equal_time("qubo", count, 50, first_sweeps=10))
    rec["grid_on_the_spin_glass"] = [equal_time("spin_glass", count, 200 // s, s, r, t) for r, s, t in GRID]
    rec["method"] = ("times of a round: hip.Probe (device events around the launch), alternating in one run; equal time: "
                     "device events around whole calls, 200 random starts per graph, seeds 0..2, mean cut (objective) over "
                     "the graphs; the tempered result is the better of the annealed and the tempered partition per graph, "
                     "as the solver doors take it")
    rec["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
