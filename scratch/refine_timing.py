"""Local search over decoded partitions (gmc_refine_local_f32): kernel time, CPU restatement time and cut quality.

    python scratch/refine_timing.py OUT.json            everything below, one JSON record
    python scratch/refine_timing.py --profile           only the two timed refinements, 5 times each
                                                        (for `rocprofv3 --kernel-trace --stats -- python ...`)

1. Trains a model with train_from_pickle on an n200_300_d8_12-style dataset (random regular graphs, n in 200..300,
   d in 8..12, terminals normalised to 0,1,2 by process_graphs_from_folder; seeded).
2. Quality: decode_dataset(..., 200, local_search_sweeps=100) on held-out d = 7 regular graphs of n = 100 .. 1000:
   mean cut per size of the argmax decode, the reference's post-processing (best of 200 samples) and the refinement.
3. Timing, candidates = argmax decode + 200 samples of the trained model, max_sweeps = 100:
   (a) 50 graphs, n in {50, 100, 200, 300, 500} (BASELINE configs[4]), d = 7;  (b) 160 graphs n = 1000 d = 7.
   Kernel time of the refine launch from the library's event probe (median of 20), sweeps per candidate, and the CPU
   restatement (tests/refine_ref.py) on the same candidates: all of (a), 16 of the 160 graphs of (b).
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

import gcn_max_cut_amd as pkg  # noqa: E402
from gcn_max_cut_amd import hip  # noqa: E402
from gcn_max_cut_amd.commons import save_object  # noqa: E402
from gcn_max_cut_amd.DataGenerator import graphExtender as GE  # noqa: E402
from gcn_max_cut_amd.graph import GraphBatch  # noqa: E402
from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN  # noqa: E402
from gcn_max_cut_amd.Training import TrainingNeural as T  # noqa: E402
from oracle import ref_dense as R  # noqa: E402
from tests import refine_ref as RR  # noqa: E402


def dataset(specs):
    graphs = {i: R.regular_graph(n, d, s) for i, (n, d, s) in enumerate(specs)}
    terms = {i: R.seeded_terminals(n, s) for i, (n, d, s) in enumerate(specs)}
    return GE.process_graphs_from_folder(graphs, terms, 1000)


def train(workdir):
    rng = np.random.RandomState(0)
    specs = []
    while len(specs) < 200:
        n, d = int(rng.randint(200, 301)), int(rng.randint(8, 13))
        if n * d % 2 == 0:
            specs.append((n, d, 1000 + len(specs)))
    path = os.path.join(workdir, "nx_generated_graph_n200_300_d8_12_t200.pkl")
    save_object(dataset(specs), path)
    torch.manual_seed(0)
    t0 = time.time()
    net, best_loss, epoch, _emb, _hist = T.train_from_pickle(path, os.path.join(workdir, "refine_model"),
                                                            n_nodes=1000, number_epochs=100, save_directory=None)
    return net, dict(graphs=len(specs), epochs_run=epoch + 1, best_loss=best_loss, train_s=time.time() - t0,
                     schedule="train_from_pickle: one optimizer step per graph (the reference's), hidden_dim 500")


def candidates(net, ds, iters=200, seed=0):
    """GraphBatch, pristine candidates [1 + iters, R] int8: argmax decode, then the samples in draw order."""
    eng = net.engine()
    net.eval()
    items = list(ds.values())
    batch = GraphBatch([it[0] for it in items], [it[0].edge_values(it[1]) for it in items], eng.device)
    P, S, _loss = eng.forward(batch, 1.0, want_loss=True)
    np.random.seed(seed)
    _b, _c, _all, assign_all = TN._sample_on_gpu(batch, P, iters)
    return batch, torch.cat([S.to(torch.int8).reshape(1, -1), assign_all]).contiguous()


def refine_once(batch, work, max_sweeps, with_sweeps=False):
    cands = work.shape[0]
    order, cgoff, cptr = batch.refine_order()
    dev = batch.device
    cut_all = torch.empty((batch.B, cands), device=dev)
    best_assign = torch.empty(batch.R, dtype=torch.int32, device=dev)
    best_cut = torch.empty(batch.B, device=dev)
    best_idx = torch.empty(batch.B, dtype=torch.int32, device=dev)
    sweeps = torch.empty((batch.B, cands), dtype=torch.int32, device=dev) if with_sweeps else None
    p = hip.ptr
    hip.check(hip.load().gmc_refine_local_f32(batch.ref(), p(order), p(cgoff), p(cptr), cands, p(work), max_sweeps,
                                              p(cut_all), p(best_assign), p(best_cut), p(best_idx), p(sweeps),
                                              hip.stream()), "gmc_refine_local_f32")
    return cut_all, sweeps


def time_refine(batch, pristine, max_sweeps=100, reps=20):
    work = pristine.clone()
    refine_once(batch, work, max_sweeps)                      # warm-up (code object load)
    ms = []
    for _ in range(reps):
        work.copy_(pristine)
        with hip.Probe(8) as pr:
            refine_once(batch, work, max_sweeps)
        ms += [t for tag, t in pr.records if tag == "refine"]
    work.copy_(pristine)
    _cut, sweeps = refine_once(batch, work, max_sweeps, with_sweeps=True)
    torch.cuda.synchronize()
    sw = sweeps.cpu().numpy()
    return work.cpu().numpy(), dict(refine_kernel_ms_median=float(np.median(ms)), refine_kernel_ms_min=float(min(ms)),
                                    reps=reps, B=batch.B, R=batch.R, candidates=int(pristine.shape[0]),
                                    max_sweeps=max_sweeps, sweeps_mean=float(sw.mean()), sweeps_max=int(sw.max()))


def cpu_restatement(ds, batch, pristine, refined_gpu, graphs, max_sweeps=100):
    A = pristine.cpu().numpy()
    items = list(ds.values())
    t0 = time.time()
    same = True
    for g in graphs:
        h = items[g][0]
        lo, hi = int(batch.goff_host[g]), int(batch.goff_host[g + 1])
        out, _sw = RR.refine(h.n, h.rowptr, h.col, h.weight, A[:, lo:hi], max_sweeps)
        same &= bool((out == refined_gpu[:, lo:hi]).all())
    return dict(cpu_restatement_s=time.time() - t0, graphs_timed=len(graphs), equal_to_gpu=same,
                how="tests/refine_ref.py (numpy, one host thread, vectorised over candidates and class nodes)")


CONFIG_A = [(n, 7, 7000 + 10 * n + i) for n in (50, 100, 200, 300, 500) for i in range(10)]
CONFIG_B = [(1000, 7, 9000 + i) for i in range(160)]


def main():
    profile = "--profile" in sys.argv
    out_path = None if profile else sys.argv[1]
    hip.require_gpu()
    with tempfile.TemporaryDirectory() as workdir:      # (the dataset pickle holds dense [n, 1000] adjacencies)
        net, train_info = train(workdir)
    rec = {"train": train_info}
    if not profile:
        quality = {}
        for n in (100, 200, 300, 500, 1000):
            ds = dataset([(n, 7, 5000 + 10 * n + i) for i in range(10)])
            np.random.seed(0)
            t0 = time.time()
            res = TN.decode_dataset(net, ds, 200, local_search_sweeps=100)
            quality[str(n)] = dict(
                graphs=len(res), edges=int(n * 7 // 2), wall_s=time.time() - t0,
                argmax=float(np.mean([r["simple_cut"] for r in res])),
                post_processing_200=float(np.mean([r["post_cut"] for r in res])),
                refined=float(np.mean([r["refined_cut"] for r in res])),
                refined_from_argmax=int(sum(r["refined_from"] == 0 for r in res)))
            print(n, quality[str(n)], flush=True)
        rec["quality_d7"] = quality
    for name, specs, cpu_graphs in (("a_configs4_50_graphs", CONFIG_A, range(50)),
                                    ("b_160_graphs_n1000_d7", CONFIG_B, range(16))):
        ds = dataset(specs)
        batch, pristine = candidates(net, ds)
        refined, t = time_refine(batch, pristine, reps=5 if profile else 20)
        if not profile:
            t.update(cpu_restatement(ds, batch, pristine, refined, list(cpu_graphs)))
        rec[name] = t
        print(name, t, flush=True)
    rec["device"] = torch.cuda.get_device_name(0)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
