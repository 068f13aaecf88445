"""Per-graph early stopping of solve_dataset on the MI355X: profiles/r20_instance_early_stop.json.

    python scratch/instance_early_stop_timing.py OUT.json [--skip-kernels] [--skip-solve] [--skip-large]

(a) gmc_inst_adam_f32 against gmc_adam_f32 on the buffers of 160 x (n = 1000, d = 7), hidden 500, K = 3, in ONE process,
    alternating: ROUNDS rounds of REPS calls each, per-call time of every round (host clock around work that ends in a
    device synchronise); nothing stopped, half of the graphs stopped (every other one), 90 % stopped.
(b) the two-launch stop call (gmc_inst_early_stop_f32) against gmc_inst_keep_best_f32 on the same batch, the same way.
(c) solve_dataset at the reference's defaults (tolerance 1e-4, patience 20, number_epochs 1000) on the held-out 7-regular
    graphs of scratch/instance_timing.py (10 per size, n = 500 and 1000), both losses at the learning rates used there,
    one torch seed: wall time with and without early_stopping, the stop epochs, the number of compactions and the time
    spent in InstanceEngine.subset, wall time at check_every 1 / 16 / 64, and the mean cut of `partition` either way.
(d) the same solve with the hard loss on the 160 x (n = 1000) batch of (a), whose step is bound by bandwidth: without
    early stopping, and with it over check_every 1 / 16 / 64 x compact_fraction 0.1 / 0.25 / 0.5."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gcn_max_cut_amd as pkg  # noqa: E402
from gcn_max_cut_amd import hip  # noqa: E402
from gcn_max_cut_amd.DataGenerator import graphExtender as GE  # noqa: E402
from gcn_max_cut_amd.Training import TrainingNeural as T  # noqa: E402
from oracle import ref_dense as R  # noqa: E402

HIDDEN, K = 500, 3
ROUNDS, REPS = 7, 40


def dataset(specs):
    graphs = {i: R.regular_graph(n, d, s) for i, (n, d, s) in enumerate(specs)}
    terms = {i: R.seeded_terminals(n, s) for i, (n, d, s) in enumerate(specs)}
    return GE.process_graphs_from_folder(graphs, terms, 1000)


def alternating(fns):
    """{name: [ms per call of each round]} of the callables, one round of each after the other, ROUNDS times."""
    for fn in fns.values():
        for _ in range(5):
            fn()
    out = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(REPS):
                fn()
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) / REPS * 1e3)
    return {name: dict(median_ms=float(np.median(v)), min_ms=min(v), max_ms=max(v), rounds_ms=v) for name, v in out.items()}


def kernel_times(ds):
    handles = [it[0] for it in ds.values()]
    eng = pkg.engine.InstanceEngine(handles, HIDDEN, K)
    torch.manual_seed(0)
    eng.reset_parameters()
    eng.grad.normal_(0, 1e-3)
    lib = hip.load()
    B = eng.B
    masks = {"none": torch.full((B,), -1, dtype=torch.int32, device=eng.device)}
    half = masks["none"].clone()
    half[::2] = 0
    most = torch.zeros(B, dtype=torch.int32, device=eng.device)
    most[::10] = -1
    masks.update(half=half, ninety_percent=most)
    step = [0]

    def flat():
        step[0] += 1
        lib.gmc_adam_f32(hip.ptr(eng.flat), hip.ptr(eng.grad), hip.ptr(eng.m), hip.ptr(eng.v), eng.count, 1e-3, 0.9, 0.999,
                         1e-8, step[0], hip.stream())

    def segmented(mask):
        def call():
            step[0] += 1
            lib.gmc_inst_adam_f32(eng.batch.ref(), eng.Fp, eng.K, hip.ptr(eng.flat), hip.ptr(eng.grad), hip.ptr(eng.m),
                                  hip.ptr(eng.v), 1e-3, 0.9, 0.999, 1e-8, step[0], hip.ptr(mask), hip.stream())
        return call

    rec = {"graphs": B, "n": 1000, "hidden": HIDDEN, "K": K, "parameters": eng.count, "bytes_per_call": 28 * eng.count,
           "rounds": ROUNDS, "reps_per_round": REPS}
    rec["adam"] = alternating({"gmc_adam_f32": flat, "gmc_inst_adam_f32_none_stopped": segmented(masks["none"]),
                               "gmc_inst_adam_f32_half_stopped": segmented(masks["half"]),
                               "gmc_inst_adam_f32_90pct_stopped": segmented(masks["ninety_percent"])})
    for name, r in rec["adam"].items():
        print(name, {k: round(v, 4) for k, v in r.items() if k != "rounds_ms"}, flush=True)
    _P, S, losses = eng.train_fwd_bwd(1.0)
    epoch = [0]

    def keep():
        eng.keep_best(S, losses, epoch[0])
        epoch[0] += 1

    def stop():
        eng.early_stop(S, losses, epoch[0], 1e-4, 1 << 30)
        epoch[0] += 1

    rec["finish"] = alternating({"gmc_inst_keep_best_f32": keep, "gmc_inst_early_stop_f32": stop})
    for name, r in rec["finish"].items():
        print(name, {k: round(v, 4) for k, v in r.items() if k != "rounds_ms"}, flush=True)
    return rec


REAL_SUBSET = pkg.engine.InstanceEngine.subset
SPENT = []


def timed_subset(self, keep):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sub = REAL_SUBSET(self, keep)
    torch.cuda.synchronize()
    SPENT.append(dict(ms=(time.perf_counter() - t0) * 1e3, graphs_from=self.B, graphs_to=sub.B))
    return sub


def solve_large(ds):
    cfg = T.TrainingConfig(n_nodes=1000, hidden_dim=HIDDEN, number_epochs=1000, learning_rate=1e-3, tolerance=1e-4,
                           patience=20)
    rec = {"graphs": len(ds), "n": 1000, "loss": "cut", "lr": 1e-3}

    def run(**kw):
        torch.manual_seed(0)
        del SPENT[:]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = T.solve_dataset(ds, cfg, loss="cut", **kw)
        torch.cuda.synchronize()
        out = dict(wall_s=time.perf_counter() - t0, mean_cut=float(np.mean([r["cut"] for r in res])))
        if kw:
            stops = [r["stopped_epoch"] for r in res]
            ran = [1000 if s is None else s + 1 for s in stops]
            out.update(stop_epoch_min=min(ran) - 1, stop_epoch_median=float(np.median(ran)) - 1, stop_epoch_max=max(ran) - 1,
                       ran_to_the_end=sum(s is None for s in stops), compactions=len(SPENT),
                       rebuild_ms_total=sum(x["ms"] for x in SPENT), rebuilds=list(SPENT))
        return out

    pkg.engine.InstanceEngine.subset = timed_subset
    run(early_stopping=True)                                # warm-up
    rec["no_early_stopping"] = run()
    print("large no_early_stopping", rec["no_early_stopping"], flush=True)
    for every in (16, 1, 64):
        for fraction in (0.25, 0.1, 0.5):
            key = f"check_every_{every}_compact_{fraction}"
            rec[key] = run(early_stopping=True, check_every=every, compact_fraction=fraction)
            print("large", key, {k: v for k, v in rec[key].items() if k != "rebuilds"}, flush=True)
    rec["no_early_stopping_again"] = run()
    print("large no_early_stopping_again", rec["no_early_stopping_again"], flush=True)
    pkg.engine.InstanceEngine.subset = REAL_SUBSET
    return rec


def solves():
    rec = {}
    spent = SPENT
    pkg.engine.InstanceEngine.subset = timed_subset
    for n in (500, 1000):
        ds = dataset([(n, 7, 5000 + 10 * n + i) for i in range(10)])
        row = {"graphs": len(ds), "edges": n * 7 // 2}
        for name, loss, lr in (("hard_lr1e-3", "cut", 1e-3), ("expected_cut_lr1e-2", "expected_cut", 1e-2)):
            cfg = T.TrainingConfig(n_nodes=1000, hidden_dim=HIDDEN, number_epochs=1000, learning_rate=lr, tolerance=1e-4,
                                   patience=20)

            def run(**kw):
                torch.manual_seed(0)
                del spent[:]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = T.solve_dataset(ds, cfg, loss=loss, **kw)
                torch.cuda.synchronize()
                return res, time.perf_counter() - t0

            run()                                               # warm-up
            case = {}
            for label, kw in (("no_early_stopping", {}), ("check_every_16", dict(early_stopping=True, check_every=16)),
                              ("check_every_1", dict(early_stopping=True, check_every=1)),
                              ("check_every_64", dict(early_stopping=True, check_every=64)),
                              ("no_early_stopping_again", {}), ("check_every_16_again", dict(early_stopping=True, check_every=16))):
                res, wall = run(**kw)
                case[label] = dict(wall_s=wall, mean_cut=float(np.mean([r["cut"] for r in res])),
                                   cuts=[int(r["cut"]) for r in res], best_epochs=[int(r["best_epoch"]) for r in res])
                if kw:
                    case[label].update(stop_epochs=[r["stopped_epoch"] for r in res], compactions=len(spent),
                                       rebuilds=list(spent))
                print(n, name, label, case[label], flush=True)
            row[name] = case
        rec[str(n)] = row
    pkg.engine.InstanceEngine.subset = REAL_SUBSET
    return rec


def main():
    out_path = sys.argv[1]
    hip.require_gpu()
    rec = {"device": torch.cuda.get_device_name(0)}
    big = dataset([(1000, 7, 100 + i) for i in range(160)])
    if "--skip-kernels" not in sys.argv:
        rec["kernels"] = kernel_times(big)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    if "--skip-solve" not in sys.argv:
        rec["solve_dataset_d7"] = solves()
    if "--skip-large" not in sys.argv:
        rec["solve_dataset_160x1000"] = solve_large(big)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
