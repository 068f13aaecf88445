"""Rounding by conditional expectations (gmc_round_conditional_f32): kernel time next to the seeded sampler and the
local search, and cut quality next to argmax, best of 200 samples and the refinement.

    python scratch/rounding_timing.py OUT.json

1. Trains three models with train_from_pickle on the n200_300_d8_12-style dataset of scratch/refine_timing.py (seeded):
   the 3-class model of DESIGN section 10 (loss "cut"), one 3-class model with loss="expected_cut", one 4-class model.
2. Kernel time (K = 3, section 10's model), from the library's event probe (device events around the launch), after a
   warm-up call of every variant, the variants alternating in one run, 3 windows of 6 calls, median and window medians:
   rounding with descent 0, rounding with descent 100, the seeded sampler at 200 samples, the local search (100 sweeps
   at most) over the argmax decode + 200 samples; (a) 50 graphs n in {50, 100, 200, 300, 500} d = 7 (BASELINE
   configs[4]), (b) 160 graphs n = 1000 d = 7.
3. Mean cut over 10 held-out d = 7 regular graphs per size n = 100 .. 1000: argmax, best of 200 samples (numpy seed 0),
   rounded, rounded + descent (100 sweeps at most), refined (local search over argmax + 200 samples), next to the mean
   expected cut; for the two 3-class models.  For the 4-class model: argmax, rounded, rounded + descent.
"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gcn_max_cut_amd import hip  # noqa: E402
from gcn_max_cut_amd.commons import save_object  # noqa: E402
from gcn_max_cut_amd.DataGenerator import graphExtender as GE  # noqa: E402
from gcn_max_cut_amd.graph import GraphBatch  # noqa: E402
from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN  # noqa: E402
from gcn_max_cut_amd.Training import TrainingNeural as T  # noqa: E402
from oracle import ref_dense as R  # noqa: E402

ITERS, WINDOWS, PER_WINDOW = 200, 3, 6


def dataset(specs, K=3):
    graphs = {i: R.regular_graph(n, d, s) for i, (n, d, s) in enumerate(specs)}
    if K == 3:
        terms = {i: R.seeded_terminals(n, s) for i, (n, d, s) in enumerate(specs)}
        return GE.process_graphs_from_folder(graphs, terms, 1000)
    terms = {i: [int(t) for t in np.random.RandomState(s).permutation(n)[:K]] for i, (n, d, s) in enumerate(specs)}
    return GE.process_graphs_from_folder(graphs, terms, 1000, number_classes=K)


def train(workdir, K=3, loss="cut"):
    rng = np.random.RandomState(0)
    specs = []
    while len(specs) < 200:
        n, d = int(rng.randint(200, 301)), int(rng.randint(8, 13))
        if n * d % 2 == 0:
            specs.append((n, d, 1000 + len(specs)))
    path = os.path.join(workdir, f"nx_generated_graph_n200_300_d8_12_t200_k{K}.pkl")
    if not os.path.exists(path):
        save_object(dataset(specs, K), path)
    torch.manual_seed(0)
    t0 = time.time()
    net, best_loss, epoch, _emb, _hist = T.train_from_pickle(path, os.path.join(workdir, "rounding_model"), n_nodes=1000,
                                                            number_epochs=100, save_directory=None, number_classes=K,
                                                            loss=loss)
    net.eval()
    return net, dict(graphs=len(specs), number_classes=K, loss=loss, epochs_run=epoch + 1, best_loss=best_loss,
                     train_s=time.time() - t0,
                     schedule="train_from_pickle: one optimizer step per graph (the reference's), hidden_dim 500")


def probed(tag, launch):
    with hip.Probe(4) as pr:
        launch()
    ms = [t for name, t in pr.records if name == tag]
    return ms[0]                                              # (the pick launch of the searches is not tagged)


def summary(ms):
    windows = [float(np.median(ms[w * PER_WINDOW:(w + 1) * PER_WINDOW])) for w in range(WINDOWS)]
    return dict(kernel_ms_median=float(np.median(ms)), kernel_ms_min=float(min(ms)), calls=len(ms),
                window_medians_ms=windows)


def kernel_times(net, ds):
    eng = net.engine()
    items = list(ds.values())
    batch = GraphBatch([it[0] for it in items], [it[0].edge_values(it[1]) for it in items], eng.device)
    P, S, _loss = eng.forward(batch, 1.0, want_loss=True)
    dev, p, lib = batch.device, hip.ptr, hip.load()
    order, cgoff, cptr = batch.refine_order(3)
    gkey = torch.from_numpy(TN.sample_keys(0, range(batch.B)).view(np.int64)).to(dev)
    assign_all = torch.empty((ITERS, batch.R), dtype=torch.int8, device=dev)
    cut_all = torch.empty((batch.B, ITERS + 1), device=dev)
    best_assign = torch.empty(batch.R, dtype=torch.int32, device=dev)
    best_cut = torch.empty(batch.B, device=dev)
    best_idx = torch.empty(batch.B, dtype=torch.int32, device=dev)
    r_assign = torch.empty(batch.R, dtype=torch.int8, device=dev)
    r_cut = torch.empty(batch.B, device=dev)
    r_expected = torch.empty(batch.B, device=dev)
    r_sweeps = torch.empty(batch.B, dtype=torch.int32, device=dev)
    ls_sweeps = torch.empty((batch.B, ITERS + 1), dtype=torch.int32, device=dev)

    def sample():
        hip.check(lib.gmc_decode_sample_seeded_f32(batch.ref(), p(P), p(gkey), ITERS, p(assign_all), p(cut_all),
                                                   p(best_assign), p(best_cut), p(best_idx), hip.stream()), "sample")

    def rounding(descent):
        hip.check(lib.gmc_round_conditional_f32(batch.ref(), p(P), 3, p(order), p(cgoff), p(cptr), descent, p(r_assign),
                                                p(r_cut), p(r_expected), p(r_sweeps), hip.stream()), "round")

    sample()
    pristine = torch.cat([S.to(torch.int8).reshape(1, -1), assign_all]).contiguous()
    work = pristine.clone()

    def search():
        hip.check(lib.gmc_refine_local_f32(batch.ref(), p(order), p(cgoff), p(cptr), ITERS + 1, p(work), 100, p(cut_all),
                                           p(best_assign), p(best_cut), p(best_idx), p(ls_sweeps), hip.stream()), "refine")

    rounding(0), rounding(100), search()                       # warm-up (code object load)
    torch.cuda.synchronize()
    ms = {"rounding_descent_0": [], "rounding_descent_100": [], "seeded_sampler_200": [], "local_search_201_candidates": []}
    for _ in range(WINDOWS * PER_WINDOW):
        ms["rounding_descent_0"].append(probed("refine", lambda: rounding(0)))
        ms["rounding_descent_100"].append(probed("refine", lambda: rounding(100)))
        ms["seeded_sampler_200"].append(probed("sample", sample))
        work.copy_(pristine)
        ms["local_search_201_candidates"].append(probed("refine", search))
    rounding(100)
    torch.cuda.synchronize()
    out = {k: summary(v) for k, v in ms.items()}
    out.update(B=batch.B, R=batch.R, rounding_descent_sweeps_mean=float(r_sweeps.float().mean()),
               rounding_descent_sweeps_max=int(r_sweeps.max()), local_search_sweeps_mean=float(ls_sweeps.float().mean()))
    return out


def quality(net, K):
    rec = {}
    for n in (100, 200, 300, 500, 1000):
        ds = dataset([(n, 7, 5000 + 10 * n + i) for i in range(10)], K)
        mean = lambda res, key: float(np.mean([r[key] for r in res]))
        if K == 3:
            np.random.seed(0)
            res = TN.decode_dataset(net, ds, ITERS, local_search_sweeps=100, rounding_descent_sweeps=0)
            row = dict(argmax=mean(res, "simple_cut"), best_of_200=mean(res, "post_cut"), rounded=mean(res, "rounded_cut"),
                       refined=mean(res, "refined_cut"), expected_cut=mean(res, "expected_cut"))
        else:
            res = TN.round_dataset(net, ds, 0)
            row = dict(argmax=mean(res, "simple_cut"), rounded=mean(res, "rounded_cut"), expected_cut=mean(res, "expected_cut"))
        down = TN.round_dataset(net, ds, 100)
        row.update(rounded_plus_descent=mean(down, "rounded_cut"), descent_sweeps_mean=mean(down, "descent_sweeps"),
                   graphs=len(res), edges=int(n * 7 // 2),
                   rounded_below_expected=int(sum(r["rounded_cut"] < r["expected_cut"] - 5e-5 * (n * 7 // 2) for r in res)))
        rec[str(n)] = row
        print(K, n, row, flush=True)
    return rec


CONFIG_A = [(n, 7, 7000 + 10 * n + i) for n in (50, 100, 200, 300, 500) for i in range(10)]
CONFIG_B = [(1000, 7, 9000 + i) for i in range(160)]


def main():
    out_path = sys.argv[1]
    hip.require_gpu()
    rec = {"models": {}, "quality_d7_mean_cut_per_size": {}}
    with tempfile.TemporaryDirectory() as workdir:      # (the dataset pickles hold dense [n, 1000] adjacencies)
        for name, K, loss in (("section10_model", 3, "cut"), ("expected_cut_model", 3, "expected_cut"),
                              ("four_class_model", 4, "cut")):
            net, info = train(workdir, K, loss)
            rec["models"][name] = info
            rec["quality_d7_mean_cut_per_size"][name] = quality(net, K)
            if name == "section10_model":
                for cfg_name, specs in (("a_configs4_50_graphs", CONFIG_A), ("b_160_graphs_n1000_d7", CONFIG_B)):
                    rec[cfg_name] = kernel_times(net, dataset(specs))
                    print(cfg_name, rec[cfg_name], flush=True)
    rec["method"] = (f"kernel times: hip.Probe (device events around the launch), every variant warmed up, variants "
                     f"alternating in one run, {WINDOWS} windows of {PER_WINDOW} calls")
    rec["device"] = torch.cuda.get_device_name(0)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
