"""The chain searches with per-node class costs (gmc_kway_tabu_c_f32, gmc_kway_balance_c_f32): what the cost variants
cost next to their NULL twins, whether the tabu stage pays on a dense QUBO at equal time, and what a cardinality bound
costs in energy.  An extension of scratch/balanced_timing.py's method.

    python scratch/chain_cost_timing.py OUT.json [--skip-cost] [--skip-dense]

1. Cost.  balanced_timing.py's workload: 160 graphs n = 1000 d = 7 (unit weights, terminals), 201 candidates that 100
   annealing sweeps have brought to local optima, ITERATIONS iterations, K = 2, 3, 8.  Six calls alternating in one
   process (forwards, then backwards): tabu and tabu with an integer cost in -3..3, the balanced search under loose
   and under exact bounds, each without and with the cost.  Device events around loops of CALLS calls, ROUNDS loops,
   median with min and max.  The candidates are optima of the PLAIN cut, so with the cost the chains have more to do
   early on: the figure is the call's time on this input, not an instruction count.
2. Dense QUBO at equal time.  GRAPHS instances G(n = 800, p = 0.06) (about 19,000 couplings each, integers in +-1, +-2;
   linear terms integers in -3..3), solve_qubo's mapping.  Per solver seed 0, 1, 2: solve_qubo(anneal_sweeps = base,
   tabu_iterations = T) against solve_qubo(anneal_sweeps = base + extra), `extra` the tabu call's measured time (34
   candidates: solve_qubo's default) at the measured time per annealing sweep; base = 100 (the default) and base = 10
   (a starved annealing, which leaves something to find).  Mean energy over the instances.
3. A cardinality bound on the same family: solve_qubo(cardinality = n // 4) next to the unconstrained energy, and the
   time of one balanced call of 20 n iterations on the 34 annealed candidates."""
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

ITERATIONS, CALLS, ROUNDS, CANDS, SWEEPS = 1000, 2, 3, 201, 100
GRAPHS, N, P = 4, 800, 0.06
TRAIN = dict(hidden_dim=32, epochs=100, learning_rate=1e-2)


def cost_of_the_cost(batch, K, cands=CANDS, terminals=True, iterations=ITERATIONS):
    optima = random_candidates(batch, K, cands, terminals, K)
    TN._kway_anneal_on_gpu(batch, K, optima, TN.anneal_schedule(SWEEPS), 1, 100, terminals)
    n = np.asarray(batch.sizes, np.int64)
    loose = (np.zeros((batch.B, K), np.int32), np.repeat(n[:, None], K, axis=1).astype(np.int32))
    exact = TN.class_size_bounds("timing", "balanced", n, K, terminals)
    nc = torch.from_numpy(np.random.RandomState(K).randint(-3, 4, (batch.R, K)).astype(np.float32)).to(batch.device)
    tabu = lambda c: TN._kway_tabu_on_gpu(batch, K, optima.clone(), iterations, TN.TABU_TENURE, 1, terminals, c)  # noqa: E731
    bal = lambda b, c: TN._kway_balance_on_gpu(batch, K, optima.clone(), b[0], b[1], iterations, TN.TABU_TENURE, 1,  # noqa: E731
                                               terminals, c)
    six = [("tabu", lambda: tabu(None)), ("tabu_cost", lambda: tabu(nc)),
           ("balance_loose", lambda: bal(loose, None)), ("balance_loose_cost", lambda: bal(loose, nc)),
           ("balance_exact", lambda: bal(exact, None)), ("balance_exact_cost", lambda: bal(exact, nc))]
    zero = torch.zeros_like(nc)
    twin_equal = all(torch.equal(a, b) for a, b in zip(tabu(None), tabu(zero))) and \
        all(torch.equal(a, b) for a, b in zip(bal(exact, None), bal(exact, zero)))
    rec = {}
    for name, fn in six + six[::-1]:
        rec.setdefault(name, []).append(timed(fn, CALLS, ROUNDS))
    med = {k: float(np.median([r["ms_median"] for r in v])) for k, v in rec.items()}
    out = dict(K=K, B=batch.B, n_max=batch.n_max, candidates=cands, iterations=iterations, chains=batch.B * cands,
               zero_cost_outputs_equal_twin=bool(twin_equal), runs=rec, ms_per_call=med,
               cost_over_null={k: med[k + "_cost"] / med[k] for k in ("tabu", "balance_loose", "balance_exact")},
               mean_moves_tabu=float(tabu(None)[4].float().mean()), mean_moves_tabu_cost=float(tabu(nc)[4].float().mean()))
    print(json.dumps(out), flush=True)
    return out


def dense_family():
    """(edge_index [2, E] both directions, ptr, quadratic [E], linear [R]) of GRAPHS instances."""
    import networkx as nx
    src, dst, q, ptr = [], [], [], [0]
    rng = np.random.RandomState(7)
    for i in range(GRAPHS):
        g = nx.gnp_random_graph(N, P, seed=100 + i)
        e = np.asarray(list(g.edges()), np.int64)
        qq = rng.choice([-2.0, -1.0, 1.0, 2.0], size=len(e))
        src += [e[:, 0] + ptr[-1], e[:, 1] + ptr[-1]]
        dst += [e[:, 1] + ptr[-1], e[:, 0] + ptr[-1]]
        q += [qq, qq]
        ptr.append(ptr[-1] + N)
    ei = np.stack([np.concatenate(src), np.concatenate(dst)])
    return ei, np.asarray(ptr, np.int64), np.concatenate(q), rng.randint(-3, 4, ptr[-1]).astype(np.float64)


def dense(rec, save):
    ei, ptr, q, lin = dense_family()
    rec["family"] = dict(graphs=GRAPHS, n=N, p=P, couplings_per_graph=int(ei.shape[1] // 2 // GRAPHS),
                         density=float(ei.shape[1] / GRAPHS / (N * (N - 1))), train=TRAIN)
    # ---- the two budgets, on the arrays solve_qubo builds
    batch = GraphBatch.from_edge_index(ei, ptr, edge_weight=(0.5 * q).astype(np.float32))
    half = np.zeros(batch.R)
    np.add.at(half, ei[0], 0.5 * q)
    nc = np.zeros((batch.R, 2), np.float32)
    nc[:, 1] = lin + half
    nc = torch.from_numpy(nc).to(batch.device)
    scale = maxcut._mean_abs_edge_weight(batch)
    start = random_candidates(batch, 2, 34, False, 3)
    optima = start.clone()
    TN._kway_anneal_on_gpu(batch, 2, optima, TN.anneal_schedule(100, scale=scale), 1, 100, False, nc)
    anneal = lambda s: timed(lambda: TN._kway_anneal_on_gpu(batch, 2, start.clone(), TN.anneal_schedule(s, scale=scale), 1, 100,  # noqa: E731
                                                            False, nc), 2, 3)["ms_median"]
    a100, a300 = anneal(100), anneal(300)
    ms_per_sweep = (a300 - a100) / 200
    rec["anneal_ms"] = dict(sweeps_100=a100, sweeps_300=a300, per_sweep=ms_per_sweep)
    shape = int(hip.load().gmc_kway_tabu_shape(batch.ref(), 2))
    rec["tabu_shape"] = dict(chains_per_workgroup=shape & 15, csr_staged_in_lds=shape >> 4)
    rows = []
    for base, T in ((100, 2000), (100, 10000), (100, 40000), (10, 500), (10, 2000)):
        tabu_ms = timed(lambda: TN._kway_tabu_on_gpu(batch, 2, optima.clone(), T, TN.TABU_TENURE, 1, False, nc), 2, 3)["ms_median"]
        extra = max(1, int(round(tabu_ms / ms_per_sweep)))
        row = dict(base_sweeps=base, iterations=T, tabu_ms=tabu_ms, extra_sweeps=extra, annealed=[], with_tabu=[], longer=[])
        for seed in (0, 1, 2):
            kw = dict(quadratic=q, linear=lin, seed=seed, **TRAIN)
            t = maxcut.solve_qubo(ei, ptr, anneal_sweeps=base, tabu_iterations=T, **kw)
            longer = maxcut.solve_qubo(ei, ptr, anneal_sweeps=base + extra, **kw)
            row["annealed"].append(float(-t.result.annealed_cut.mean()))
            row["with_tabu"].append(float(t.energy.mean()))
            row["longer"].append(float(longer.energy.mean()))
        rows.append(row)
        print(json.dumps(row), flush=True)
        rec["equal_time"] = rows
        save()
    # ---- a cardinality bound
    k = N // 4
    lo, hi = maxcut._cardinality_sizes(k, ptr)
    lo, hi = lo.astype(np.int32), hi.astype(np.int32)
    bal_ms = timed(lambda: TN._kway_balance_on_gpu(batch, 2, optima.clone(), lo, hi, 20 * N, TN.TABU_TENURE, 1, False, nc), 1, 3)
    card = dict(cardinality=k, balance_iterations=20 * N, balanced_stage_ms=bal_ms, constrained=[], unconstrained=[], ones=[])
    for seed in (0, 1, 2):
        res = maxcut.solve_qubo(ei, ptr, quadratic=q, linear=lin, seed=seed, cardinality=k, **TRAIN)
        card["constrained"].append(float(res.energy.mean()))
        card["unconstrained"].append(float(-res.result.unconstrained_cut.mean()))
        x = res.x.cpu().numpy()
        card["ones"].append([int(x[a:b].sum()) for a, b in zip(ptr[:-1], ptr[1:])])
    rec["cardinality"] = card
    print(json.dumps(card), flush=True)
    save()


def main():
    out_path = sys.argv[1]
    hip.require_gpu()
    rec = {"device": torch.cuda.get_device_name(0)}

    def save():
        with open(out_path, "w") as f:
            json.dump(rec, f, indent=1)

    if "--skip-dense" not in sys.argv:
        rec["dense_qubo"] = {}
        dense(rec["dense_qubo"], save)
    if "--skip-cost" not in sys.argv:
        batch = GraphBatch([from_networkx(R.regular_graph(1000, 7, 9000 + i)) for i in range(160)], None, torch.device("cuda"))
        rec["cost_160_graphs_n1000_d7_201_candidates"] = []
        for K in (2, 3, 8):
            rec["cost_160_graphs_n1000_d7_201_candidates"].append(cost_of_the_cost(batch, K))
            save()
    rec["method"] = (f"cost: device events around loops of {CALLS} calls, {ROUNDS} loops, six calls alternating forwards then "
                     f"backwards, {ITERATIONS} iterations; dense: three solver seeds, no default changed")
    save()


if __name__ == "__main__":
    main()
