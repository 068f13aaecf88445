"""The tabu stage (gmc_kway_tabu_f32): what it costs next to the annealing, and whether it pays at equal time.

    python scratch/tabu_timing.py OUT.json [--skip-quality] [--skip-solve]

1. Cost.  160 graphs n = 1000 d = 7 (unit weights), K = 2, 3, 8, with 4, 34 and 201 candidates that 100 annealing sweeps
   have already brought to local optima (4 candidates: one workgroup per graph, every workgroup resident, so the call's
   time over its iterations is what ONE iteration of a chain takes), and one Gset-like dense graph (n = 800, 19,176
   edges, K = 2).  One gmc_kway_tabu_f32 call of ITERATIONS iterations against one gmc_kway_refine_anneal_t_f32 call of
   100 sweeps on the same batch, alternating in one process: device events around loops of CALLS calls, ROUNDS loops
   each, median with min and max.  Both calls start from a fresh copy of their candidates (the copy is inside the
   timed loop of both).
2. Does it pay?  The 3-class and 4-class models of scratch/rounding_timing.py on the held-out 7-regular graphs (10 per
   size, n = 500 and 1000, 200 samples: 202 candidates), no change of any default.  For a grid of (iterations, tenure)
   and SEEDS seeds: best cut per graph of [100 annealing sweeps, then the tabu stage, the better of the two] against
   [100 + extra annealing sweeps], where `extra` is the tabu call's measured time in annealing sweeps (from the time of
   100 and 200 sweeps on the same candidates).  The time of the longer annealing call is measured too, so the table
   shows how equal the two budgets were.  Mean over the graphs, then mean / min / max over the seeds.
3. The same comparison through maxcut.solve_batch at K = 2 without terminals (hidden 64, 200 epochs, lr 1e-2, 34
   candidates: the plain max-cut batch of scratch/plain_maxcut_timing.py), the sweeps-per-millisecond taken from random
   candidates on the same batch."""
import json
import os
import sys
import tempfile

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

ITERATIONS, CALLS, ROUNDS, SEEDS, SAMPLES, SWEEPS = 1000, 3, 5, 3, 200, 100
# (iterations as a multiple of n, (tenure_base, tenure_span, tenure_div))
GRID = [(5, (3, 0, 10)), (20, (3, 0, 10)), (20, (10, 0, 0)), (20, (3, 10, 0)), (20, (3, 0, 4)), (50, (3, 0, 10))]


def timed(fn, calls=CALLS, rounds=ROUNDS):
    """ms per call: loops of `calls` calls between two device events; (median, min, max) over `rounds` loops."""
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


def random_candidates(batch, K, cands, terminals, seed):
    A = np.random.RandomState(seed).randint(0, K, (cands, batch.R)).astype(np.int8)
    if terminals:
        starts = np.asarray(batch.goff_host[:-1], np.int64)
        for j in range(K):
            A[:, starts + j] = j
    return torch.from_numpy(A).to(batch.device)


def cost(batch, K, cands, terminals=True, iterations=ITERATIONS):
    lib = hip.load()
    start = random_candidates(batch, K, cands, terminals, K)
    inv_temp = TN.anneal_schedule(SWEEPS)
    optima = start.clone()
    TN._kway_anneal_on_gpu(batch, K, optima, inv_temp, 1, 100, terminals)
    rec = {}
    pair = [("anneal_100_sweeps", lambda: TN._kway_anneal_on_gpu(batch, K, start.clone(), inv_temp, 1, 100, terminals)),
            ("tabu", lambda: TN._kway_tabu_on_gpu(batch, K, optima.clone(), iterations, TN.TABU_TENURE, 1, terminals))]
    for name, fn in pair + pair[::-1]:                     # alternating: a, t, t, a
        rec.setdefault(name, []).append(timed(fn))
    shape = int(lib.gmc_kway_tabu_shape(batch.ref(), K))
    t = float(np.median([r["ms_median"] for r in rec["tabu"]]))
    chains = batch.B * cands
    out = dict(K=K, B=batch.B, n_max=batch.n_max, candidates=cands, iterations=iterations, chains=chains,
               chains_per_workgroup=shape & 15, csr_staged_in_lds=shape >> 4,
               anneal_csr_staged_in_lds=int(lib.gmc_refine_anneal_staged(batch.ref())), runs=rec, tabu_ms_per_call=t,
               anneal_ms_per_call=float(np.median([r["ms_median"] for r in rec["anneal_100_sweeps"]])),
               us_per_iteration_of_the_call=t * 1e3 / iterations,
               ns_per_iteration_per_chain=t * 1e6 / iterations / chains)
    print(json.dumps(out), flush=True)
    return out


def model_candidates(net, ds):
    """The batch and the candidates search_dataset builds: the argmax decode, the rounded partition, SAMPLES samples."""
    items = list(ds.values())
    eng = net.engine()
    handles = [it[0] for it in items]
    batch = GraphBatch(handles, [h.edge_values(it[1]) for h, it in zip(handles, items)], eng.device)
    P, S, _ = eng.forward(batch, 1.0, want_loss=True)
    rnd = TN._round_on_gpu(batch, P, 0)[0]
    samples = TN._kway_sample_on_gpu(batch, P, SAMPLES, 0, range(batch.B), True)[3]
    return batch, torch.cat([S.to(torch.int8).reshape(1, -1), rnd.reshape(1, -1), samples]).contiguous()


def spread(values):
    return dict(mean=float(np.mean(values)), min=float(min(values)), max=float(max(values)))


def equal_time(batch, K, cands, terminals, n):
    """The grid on one batch and one set of candidates."""
    anneal = lambda sweeps, seed, a: TN._kway_anneal_on_gpu(batch, K, a, TN.anneal_schedule(sweeps), seed, 100, terminals)  # noqa: E731
    t100 = timed(lambda: anneal(SWEEPS, 0, cands.clone()))["ms_median"]
    t200 = timed(lambda: anneal(2 * SWEEPS, 0, cands.clone()))["ms_median"]
    ms_per_sweep = (t200 - t100) / SWEEPS
    points = []
    for mult, tenure in GRID:
        iterations = mult * n
        annealed = cands.clone()
        anneal(SWEEPS, 0, annealed)
        t_tabu = timed(lambda: TN._kway_tabu_on_gpu(batch, K, annealed.clone(), iterations, tenure, 0, terminals))["ms_median"]
        extra = max(1, int(round(t_tabu / ms_per_sweep)))
        t_long = timed(lambda: anneal(SWEEPS + extra, 0, cands.clone()))["ms_median"]
        with_tabu, longer, base, better = [], [], [], []
        for seed in range(SEEDS):
            a = cands.clone()
            cut_a = anneal(SWEEPS, seed, a)[1]
            cut_t = TN._kway_tabu_on_gpu(batch, K, a.clone(), iterations, tenure, seed, terminals)[1]
            cut_l = anneal(SWEEPS + extra, seed, cands.clone())[1]
            both = torch.maximum(cut_a, cut_t)
            base.append(float(cut_a.mean()))
            with_tabu.append(float(both.mean()))
            longer.append(float(cut_l.mean()))
            better.append(int((cut_t > cut_a).sum()))
        points.append(dict(iterations=iterations, tenure=list(tenure), tabu_ms=t_tabu, extra_sweeps=extra,
                           anneal_100_ms=t100, anneal_100_plus_extra_ms=t_long, annealed_100=spread(base),
                           annealed_100_then_tabu=spread(with_tabu), annealed_100_plus_extra=spread(longer),
                           tabu_minus_longer_annealing=float(np.mean(with_tabu) - np.mean(longer)),
                           graphs_where_tabu_beat_its_input=better))
        print(K, n, json.dumps(points[-1]), flush=True)
    return dict(graphs=batch.B, candidates=int(cands.shape[0]), anneal_ms_per_sweep=ms_per_sweep, grid=points)


def quality():
    import rounding_timing as RT
    rec = {}
    for K in (3, 4):
        with tempfile.TemporaryDirectory() as workdir:      # (the dataset pickles hold dense [n, 1000] adjacencies)
            net, info = RT.train(workdir, K, "cut")
        rec[f"model_K{K}"] = info
        for n in (500, 1000):
            ds = RT.dataset([(n, 7, 5000 + 10 * n + i) for i in range(10)], K)
            batch, cands = model_candidates(net, ds)
            rec[f"K{K}_n{n}"] = dict(edges=n * 7 // 2, **equal_time(batch, K, cands, True, n))
    return rec


def solve_quality():
    """maxcut.solve_batch at K = 2 without terminals on the held-out graphs: tabu_iterations against extra sweeps."""
    rec = {}
    kw = dict(number_classes=2, hidden_dim=64, epochs=200, learning_rate=1e-2)
    for n in (500, 1000):
        batch = GraphBatch([from_networkx(R.regular_graph(n, 7, 5000 + 10 * n + i)) for i in range(10)], None,
                           torch.device("cuda"))
        start = random_candidates(batch, 2, 34, False, n)
        anneal = lambda sweeps: TN._kway_anneal_on_gpu(batch, 2, start.clone(), TN.anneal_schedule(sweeps), 0, 100, False)  # noqa: E731
        t100, t200 = timed(lambda: anneal(SWEEPS))["ms_median"], timed(lambda: anneal(2 * SWEEPS))["ms_median"]
        ms_per_sweep = (t200 - t100) / SWEEPS
        optima = start.clone()
        TN._kway_anneal_on_gpu(batch, 2, optima, TN.anneal_schedule(SWEEPS), 0, 100, False)
        points = []
        for mult in (5, 20, 50):
            iterations = mult * n
            t_tabu = timed(lambda: TN._kway_tabu_on_gpu(batch, 2, optima.clone(), iterations, TN.TABU_TENURE, 0, False))["ms_median"]
            extra = max(1, int(round(t_tabu / ms_per_sweep)))
            with_tabu, longer, base = [], [], []
            for seed in range(SEEDS):
                r = maxcut.solve_batch(batch, seed=seed, tabu_iterations=iterations, **kw)
                l = maxcut.solve_batch(batch, seed=seed, anneal_sweeps=SWEEPS + extra, **kw)
                with_tabu.append(float(r.cut.mean()))
                base.append(float(r.annealed_cut.mean()))
                longer.append(float(l.cut.mean()))
            points.append(dict(tabu_iterations=iterations, tabu_ms=t_tabu, extra_sweeps=extra, annealed_100=spread(base),
                               annealed_100_then_tabu=spread(with_tabu), annealed_100_plus_extra=spread(longer),
                               tabu_minus_longer_annealing=float(np.mean(with_tabu) - np.mean(longer))))
            print("solve", n, json.dumps(points[-1]), flush=True)
        rec[f"n{n}"] = dict(edges=n * 7 // 2, graphs=10, candidates=34, anneal_ms_per_sweep=ms_per_sweep, grid=points)
    return rec


def main():
    out_path = sys.argv[1]
    hip.require_gpu()
    dev = torch.device("cuda")
    rec = {"device": torch.cuda.get_device_name(0)}

    def save():
        with open(out_path, "w") as f:
            json.dump(rec, f, indent=1)

    batch = GraphBatch([from_networkx(R.regular_graph(1000, 7, 9000 + i)) for i in range(160)], None, dev)
    rec["cost_160_graphs_n1000_d7"] = [cost(batch, K, cands) for K in (2, 3, 8) for cands in (4, 34, 201)]
    save()
    dense = GraphBatch([from_networkx(nx.gnm_random_graph(800, 19176, seed=1))], None, dev)
    rec["cost_one_dense_graph_n800_m19176"] = [cost(dense, 2, cands, terminals=False) for cands in (4, 34, 201)]
    save()
    if "--skip-quality" not in sys.argv:
        rec["equal_time_models_d7"] = quality()
        save()
    if "--skip-solve" not in sys.argv:
        rec["equal_time_maxcut_solve_K2_plain"] = solve_quality()
        save()
    rec["method"] = (f"cost: device events around loops of {CALLS} calls, {ROUNDS} loops, the two calls alternating (a, t, t, a); "
                     f"equal time: the tabu call's measured time turned into annealing sweeps by the measured time per sweep; "
                     f"{SEEDS} seeds (anneal seed = tabu seed = 0..{SEEDS - 1}); no default changed")
    save()


if __name__ == "__main__":
    main()
