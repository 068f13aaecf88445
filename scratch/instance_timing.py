"""One model per graph (gmc_inst_*, InstanceEngine, solve_dataset) on the MI355X: profiles/r19_instance_models.json.

    python scratch/instance_timing.py OUT.json [--skip-quality]

(a) Step time at 160 x (n = 1000, d = 7), hidden 500, in ONE run:
    - the instance step (train_fwd_bwd + Adam + keep_best) at K = 3 and K = 4, with the per-launch times of the probe;
    - a K-class shared-model step (gmc_kway_train_fwd_bwd + Adam) over the same batch at K = 3 (kway=True) and K = 4;
    - 160 sequential one-graph steps of the fused 3-class trainer (train_single_epoch, one optimizer step per graph) with
      a model of n_nodes = 1000.
    Steps are timed with a host clock around work that ends in a device synchronise, after warm-up.
(b) Quality on the held-out 7-regular graphs of the local-search paragraph (10 per size, n = 500 and 1000, the seeds of
    scratch/refine_timing.py), one torch seed: mean cut of solve_dataset's `partition` after 500 epochs at lr 1e-3 with
    the hard loss and at lr 1e-2 with expected_cut; search_dataset(module(g)) on the solved instances of n = 500."""
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
from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN  # noqa: E402
from gcn_max_cut_amd.Training import TrainingNeural as T  # noqa: E402
from oracle import ref_dense as R  # noqa: E402

HIDDEN = 500


def dataset(specs):
    graphs = {i: R.regular_graph(n, d, s) for i, (n, d, s) in enumerate(specs)}
    terms = {i: R.seeded_terminals(n, s) for i, (n, d, s) in enumerate(specs)}
    return GE.process_graphs_from_folder(graphs, terms, 1000)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3      # ms per call


def probe_of(fn):
    with hip.Probe(64) as probe:
        fn()
    return [[tag, round(ms * 1e3, 1)] for tag, ms in probe.records]      # microseconds per launch


def step_times(ds):
    items = list(ds.values())
    handles = [it[0] for it in items]
    rec = {"graphs": len(items), "n": 1000, "d": 7, "hidden": HIDDEN}
    for K in (3, 4):
        eng = pkg.engine.InstanceEngine(handles, HIDDEN, K)
        torch.manual_seed(0)
        eng.reset_parameters()
        epoch = [0]

        def inst_step():
            _P, S, losses = eng.train_fwd_bwd(1.0)
            eng.adam_step(1e-3)
            eng.keep_best(S, losses, epoch[0])
            epoch[0] += 1

        ms = timed(inst_step, 5, 50)
        rec[f"instance_K{K}"] = dict(step_ms=ms, per_graph_step_us=ms * 1e3 / len(items), launches_us=probe_of(inst_step),
                                     parameters=eng.count)
        print(f"instance K={K}", rec[f"instance_K{K}"], flush=True)
        del eng
        shared = pkg.engine.FusedEngine(1000, HIDDEN, K, kway=True)
        torch.manual_seed(0)
        for k, v in shared.views().items():
            if k.endswith("weight"):
                torch.nn.init.xavier_uniform_(v)
        batch = pkg.GraphBatch(handles, None, shared.device)

        def shared_step():
            shared.train_fwd_bwd(batch, 1.0)
            shared.adam_step(1e-3)

        ms = timed(shared_step, 5, 50)
        rec[f"shared_kway_K{K}"] = dict(step_ms=ms, per_graph_step_us=ms * 1e3 / len(items), launches_us=probe_of(shared_step))
        print(f"shared K={K}", rec[f"shared_kway_K{K}"], flush=True)
        del shared, batch
    # the reference's schedule: one optimizer step per graph, 160 of them per epoch, the fused 3-class trainer
    cfg = T.TrainingConfig(n_nodes=1000, hidden_dim=HIDDEN)
    torch.manual_seed(0)
    net, embed, opt = T.setup_model_and_optimizer(cfg)
    ms = timed(lambda: T.train_single_epoch(ds, net, opt, embed, cfg), 3, 10)
    rec["sequential_fused_K3"] = dict(epoch_ms=ms, per_graph_step_us=ms * 1e3 / len(items),
                                      schedule="train_single_epoch, graphs_per_step = 1: 160 optimizer steps per epoch")
    print("sequential", rec["sequential_fused_K3"], flush=True)
    return rec


def quality():
    rec = {}
    for n in (500, 1000):
        ds = dataset([(n, 7, 5000 + 10 * n + i) for i in range(10)])
        row = {"graphs": len(ds), "edges": n * 7 // 2}
        for name, loss, lr in (("hard_lr1e-3", "cut", 1e-3), ("expected_cut_lr1e-2", "expected_cut", 1e-2)):
            cfg = T.TrainingConfig(n_nodes=1000, hidden_dim=HIDDEN, number_epochs=500, learning_rate=lr)
            torch.manual_seed(0)
            t0 = time.time()
            res = T.solve_dataset(ds, cfg, loss=loss)
            row[name] = dict(mean_cut=float(np.mean([r["cut"] for r in res])), cuts=[int(r["cut"]) for r in res],
                             mean_best_epoch=float(np.mean([r["best_epoch"] for r in res])), wall_s=time.time() - t0)
            print(n, name, row[name], flush=True)
            if n == 500:
                found = []
                for r, (key, item) in zip(res, ds.items()):
                    found.append(TN.search_dataset(r["model"](), {0: item})[0])
                row[name]["search_dataset_of_module"] = {
                    k: float(np.mean([f[k] for f in found])) for k in ("simple_cut", "rounded_cut", "post_cut", "searched_cut")}
                print(n, name, "search", row[name]["search_dataset_of_module"], flush=True)
        rec[str(n)] = row
    return rec


def main():
    out_path = sys.argv[1]
    hip.require_gpu()
    rec = {"device": torch.cuda.get_device_name(0)}
    if "--skip-quality" not in sys.argv:
        rec["quality_d7"] = quality()
    rec["step_time"] = step_times(dataset([(1000, 7, 100 + i) for i in range(160)]))
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
