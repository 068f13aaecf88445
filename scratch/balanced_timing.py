"""The balanced stage (gmc_kway_balance_f32): what the size bookkeeping costs next to gmc_kway_tabu_f32, what exact
bounds cost in time, and what the constraint costs in cut.

    python scratch/balanced_timing.py OUT.json [--skip-quality]

1. Cost.  160 graphs n = 1000 d = 7 (unit weights, terminals), 201 candidates that 100 annealing sweeps have brought to
   local optima, K = 2, 3, 8.  One gmc_kway_tabu_f32 call, one gmc_kway_balance_f32 call with the loose bounds (0, n) -
   the same outputs, checked here - and one with the exact bounds floor / ceil of n / K (every iteration of an
   n = 1000 graph at K = 2 and 8 is then a move and a counter-move: two scans), ITERATIONS iterations each, alternating
   in one process (t, l, e, e, l, t): device events around loops of CALLS calls, ROUNDS loops each, median with min and
   max.  Every call starts from a fresh copy of its candidates (the copy is inside the timed loop of all three).  The
   exact call's repair moves are counted and reported: they are part of its time.
2. What the constraint costs.  maxcut.solve_batch at K = 2 and 3 without terminals (hidden 64, 200 epochs, lr 1e-2, the
   defaults otherwise: 34 candidates) on the held-out 7-regular graphs (10 per size, n = 500 and 1000), with
   class_sizes="balanced" (balance_iterations = None: 20 n): mean `cut` against mean `unconstrained_cut`, and the
   largest class-size spread (largest class minus smallest) of the unconstrained partitions.  ONE seed."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gcn_max_cut_amd import hip, maxcut  # noqa: E402
from gcn_max_cut_amd.graph import GraphBatch, from_networkx  # noqa: E402
from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN  # noqa: E402
from oracle import ref_dense as R  # noqa: E402
from tabu_timing import random_candidates, timed  # noqa: E402

ITERATIONS, CALLS, ROUNDS, CANDS, SWEEPS = 1000, 2, 4, 201, 100


def cost(batch, K, cands=CANDS, terminals=True, iterations=ITERATIONS):
    optima = random_candidates(batch, K, cands, terminals, K)
    TN._kway_anneal_on_gpu(batch, K, optima, TN.anneal_schedule(SWEEPS), 1, 100, terminals)
    n = np.asarray(batch.sizes, np.int64)
    loose = (np.zeros((batch.B, K), np.int32), np.repeat(n[:, None], K, axis=1).astype(np.int32))
    exact = TN.class_size_bounds("timing", "balanced", n, K, terminals)
    tabu = lambda: TN._kway_tabu_on_gpu(batch, K, optima.clone(), iterations, TN.TABU_TENURE, 1, terminals)  # noqa: E731
    bal = lambda b: TN._kway_balance_on_gpu(batch, K, optima.clone(), b[0], b[1], iterations, TN.TABU_TENURE, 1, terminals)  # noqa: E731
    t_out, l_out, e_out = tabu(), bal(loose), bal(exact)
    same = all(torch.equal(t_out[i], l_out[j]) for i, j in ((0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 6)))
    trio = [("tabu", tabu), ("balance_loose", lambda: bal(loose)), ("balance_exact", lambda: bal(exact))]
    rec = {}
    for name, fn in trio + trio[::-1]:
        rec.setdefault(name, []).append(timed(fn, CALLS, ROUNDS))
    med = {k: float(np.median([r["ms_median"] for r in v])) for k, v in rec.items()}
    chains = batch.B * cands
    out = dict(K=K, B=batch.B, n_max=batch.n_max, candidates=cands, iterations=iterations, chains=chains,
               loose_outputs_equal_tabu=bool(same), runs=rec, ms_per_call=med,
               ns_per_iteration_per_chain={k: v * 1e6 / iterations / chains for k, v in med.items()},
               loose_over_tabu=med["balance_loose"] / med["tabu"], exact_over_tabu=med["balance_exact"] / med["tabu"],
               exact_mean_repairs=float(e_out[5].float().mean()), exact_mean_moves=float(e_out[4].float().mean()),
               exact_mean_cut=float(e_out[1].mean()), tabu_mean_cut=float(t_out[1].mean()))
    print(json.dumps(out), flush=True)
    return out


def spread_of(partition, goff, K):
    out = []
    for g in range(len(goff) - 1):
        s = np.bincount(partition[goff[g]:goff[g + 1]], minlength=K)
        out.append(int(s.max() - s.min()))
    return out


def quality():
    rec = {}
    for K in (2, 3):
        kw = dict(number_classes=K, hidden_dim=64, epochs=200, learning_rate=1e-2, seed=0)
        for n in (500, 1000):
            batch = GraphBatch([from_networkx(R.regular_graph(n, 7, 5000 + 10 * n + i)) for i in range(10)], None,
                               torch.device("cuda"))
            plain = maxcut.solve_batch(batch, **kw)
            res = maxcut.solve_batch(batch, class_sizes="balanced", **kw)
            assert torch.equal(res.unconstrained_cut, plain.cut)
            goff = np.asarray(batch.goff_host, np.int64)
            spreads = spread_of(plain.partition.cpu().numpy(), goff, K)
            within = spread_of(res.partition.cpu().numpy(), goff, K)
            rec[f"K{K}_n{n}"] = dict(graphs=10, edges=n * 7 // 2, balance_iterations=20 * n,
                                     mean_cut_balanced=float(res.cut.mean()),
                                     mean_unconstrained_cut=float(res.unconstrained_cut.mean()),
                                     cut_balanced=res.cut.cpu().tolist(), unconstrained_cut=plain.cut.cpu().tolist(),
                                     unconstrained_class_size_spread=spreads, largest_unconstrained_spread=max(spreads),
                                     largest_balanced_spread=max(within))
            print(json.dumps({f"K{K}_n{n}": rec[f"K{K}_n{n}"]}), flush=True)
    return rec


def main():
    out_path = sys.argv[1]
    hip.require_gpu()
    rec = {"device": torch.cuda.get_device_name(0)}

    def save():
        with open(out_path, "w") as f:
            json.dump(rec, f, indent=1)

    batch = GraphBatch([from_networkx(R.regular_graph(1000, 7, 9000 + i)) for i in range(160)], None, torch.device("cuda"))
    rec["cost_160_graphs_n1000_d7_201_candidates"] = []
    for K in (2, 3, 8):
        rec["cost_160_graphs_n1000_d7_201_candidates"].append(cost(batch, K))
        save()
    if "--skip-quality" not in sys.argv:
        rec["solve_batch_balanced_against_unconstrained"] = quality()
        save()
    rec["method"] = (f"cost: device events around loops of {CALLS} calls, {ROUNDS} loops, the three calls alternating "
                     f"(t, l, e, e, l, t), {ITERATIONS} iterations; quality: one seed (0), no default changed")
    save()


if __name__ == "__main__":
    main()
