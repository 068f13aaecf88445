"""The K-class sampler and annealing (gmc_kway_decode_sample_seeded_f32, gmc_kway_refine_anneal_f32): kernel time per
class count, and the cut quality of search_dataset for a 4-class model.

    python scratch/kway_search_timing.py OUT.json

profiles/r12_kway_search.json was recorded by an earlier form of this script, when gmc_refine_anneal_f32 and
gmc_decode_sample_seeded_f32 had 3-class kernels of their own: it also timed those ("anneal_3class", "sampler_3class")
next to K = 3 and compared their outputs.  The 3-class entry points now launch the K = 3 instantiations, so those
variants would time one kernel twice and are gone; scratch/decoder_merge_timing.py compares the two libraries.

1. Kernel time on 160 graphs n = 1000 d = 7 (unit weights), from the library's event probe (device events around the
   launch), after a warm-up call of every variant, the variants alternating in one run, 3 windows of 6 calls, median and
   window medians:
   - annealing, 201 uniform random candidates (terminals fixed), 100 sweeps, descent 100 at most:
     gmc_kway_refine_anneal_f32 at K = 3, 2, 4, 8;
   - the seeded sampler, 200 samples of softmax rows, assign_all written: the K-class kernel at K = 3, 2, 4, 8.
2. Quality: the 4-class model of scratch/rounding_timing.py (same dataset, same training), 10 held-out d = 7 regular
   graphs per size n = 500, 1000: mean cut of argmax, rounded, rounded + descent, best of 200 seeded samples,
   search_dataset with anneal_sweeps = 0 (the local search over 202 candidates) and with 100 annealing sweeps.
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

CANDS, SAMPLES, SWEEPS, WINDOWS, PER_WINDOW = 201, 200, 100, 3, 6


def probed(tag, launch):
    with hip.Probe(4) as pr:
        launch()
    return [t for name, t in pr.records if name == tag][0]      # (the pick launches are not tagged)


def softmax_rows(R_, K, seed):
    logits = np.random.RandomState(seed).standard_normal((R_, K)) * 2.0
    e = np.exp(logits - logits.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


def kernel_times():
    dev = torch.device("cuda")
    batch = GraphBatch([from_networkx(R.regular_graph(1000, 7, 9000 + i)) for i in range(160)], None, dev)
    p, lib = hip.ptr, hip.load()
    inv_t = torch.from_numpy(TN.anneal_schedule(SWEEPS)).to(dev)
    levels = torch.from_numpy(TN.anneal_levels()).to(dev)
    gkey = torch.from_numpy(TN.sample_keys(0, range(batch.B)).view(np.int64)).to(dev)
    cut_all = torch.empty((batch.B, CANDS), device=dev)
    best_assign = torch.empty(batch.R, dtype=torch.int32, device=dev)
    best_cut = torch.empty(batch.B, device=dev)
    best_idx = torch.empty(batch.B, dtype=torch.int32, device=dev)
    assign_all = torch.empty((SAMPLES, batch.R), dtype=torch.int8, device=dev)
    work = torch.empty((CANDS, batch.R), dtype=torch.int8, device=dev)
    starts = np.asarray(batch.goff_host[:-1], np.int64)
    variants = {}
    for K in (3, 2, 4, 8):
        A = np.random.RandomState(K).randint(0, K, (CANDS, batch.R)).astype(np.int8)
        for j in range(K):
            A[:, starts + j] = j
        pristine = torch.from_numpy(A).to(dev)
        P = torch.from_numpy(softmax_rows(batch.R, K, 100 + K)).to(dev)
        order, cgoff, cptr = batch.refine_order(K)

        def anneal_k(K=K, order=order, cgoff=cgoff, cptr=cptr):
            hip.check(lib.gmc_kway_refine_anneal_f32(batch.ref(), K, p(order), p(cgoff), p(cptr), CANDS, p(work), p(inv_t),
                                                     SWEEPS, p(levels), 1, 100, p(cut_all), p(best_assign), p(best_cut),
                                                     p(best_idx), None, None, hip.stream()), "kway anneal")

        def sample_k(K=K, P=P):
            hip.check(lib.gmc_kway_decode_sample_seeded_f32(batch.ref(), p(P), K, p(gkey), SAMPLES, p(assign_all),
                                                            p(cut_all), p(best_assign), p(best_cut), p(best_idx),
                                                            hip.stream()), "kway sample")
        variants[f"anneal_kway_K{K}"] = ("anneal", anneal_k, pristine)
        variants[f"sampler_kway_K{K}"] = ("sample", sample_k, None)
    for name, (_tag, launch, pristine) in variants.items():       # warm-up (code object load)
        if pristine is not None:
            work.copy_(pristine)
        launch()
        torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(WINDOWS * PER_WINDOW):
        for name, (tag, launch, pristine) in variants.items():
            if pristine is not None:
                work.copy_(pristine)
            ms[name].append(probed(tag, launch))
    torch.cuda.synchronize()
    out = {name: RT.summary(v) for name, v in ms.items()}
    out.update(B=batch.B, R=batch.R, candidates=CANDS, samples=SAMPLES, anneal_sweeps=SWEEPS,
               staged=int(lib.gmc_refine_anneal_staged(batch.ref())))
    return out


def quality(net, K):
    rec = {}
    mean = lambda res, key: float(np.mean([r[key] for r in res]))   # noqa: E731
    for n in (500, 1000):
        ds = RT.dataset([(n, 7, 5000 + 10 * n + i) for i in range(10)], K)
        local = TN.search_dataset(net, ds, SAMPLES, anneal_sweeps=0)
        full = TN.search_dataset(net, ds, SAMPLES, anneal_sweeps=SWEEPS)
        down = TN.round_dataset(net, ds, 100)
        rec[str(n)] = dict(argmax=mean(full, "simple_cut"), rounded=mean(full, "rounded_cut"),
                           rounded_plus_descent=mean(down, "rounded_cut"), best_of_200_samples=mean(full, "post_cut"),
                           searched_local_search_only=mean(local, "searched_cut"), searched=mean(full, "searched_cut"),
                           searched_from=[r["searched_from"] for r in full], graphs=len(full), edges=int(n * 7 // 2))
        print(K, n, rec[str(n)], flush=True)
    return rec


def main():
    out_path = sys.argv[1]
    hip.require_gpu()
    rec = {"b_160_graphs_n1000_d7": kernel_times()}
    print(rec, flush=True)
    with tempfile.TemporaryDirectory() as workdir:      # (the dataset pickles hold dense [n, 1000] adjacencies)
        net, info = RT.train(workdir, 4, "cut")
        rec["four_class_model"] = info
        rec["quality_d7_mean_cut_per_size"] = quality(net, 4)
    rec["method"] = (f"kernel times: hip.Probe (device events around the launch), every variant warmed up, variants "
                     f"alternating in one run, {WINDOWS} windows of {PER_WINDOW} calls; quality: search_dataset with "
                     f"{SAMPLES} samples (sample_seed 0, anneal_seed 0), 202 candidates")
    rec["device"] = torch.cuda.get_device_name(0)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
