"""Annealing over decoded partitions (gmc_refine_anneal_f32): kernel time per candidate-sweep against the local
search's, and cut quality.  Model, datasets and candidates are those of scratch/refine_timing.py.

    python scratch/anneal_timing.py OUT.json            everything below, one JSON record
    python scratch/anneal_timing.py --profile           only the timed launches, 3 times each
                                                        (for `rocprofv3 --kernel-trace --stats -- python ...`)

1. Quality: decode_dataset(..., 200, local_search_sweeps=100, anneal_sweeps=100) on the held-out d = 7 regular graphs
   of n = 100 .. 1000 of refine_timing.py: mean cut per size of argmax, post-processing, local search and annealing
   (all 201 candidates, and the first 32).
2. Timing, 100 annealing sweeps + descent, on (a) 50 graphs n in 50..500 and (b) 160 graphs n = 1000, d = 7, at 201 and
   32 candidates: kernel time of the anneal launch and of the local-search launch on the same candidates from the
   library's event probe (median of 10), the local search's mean sweeps, and the two times per candidate-sweep.
   (b) is also run on the global-memory path of the kernel: the same batch given explicit unit edge weights, which
   pushes its copy past the LDS budget (that run also reads the weights; its local-search figure does too).
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_timing as RT  # noqa: E402  (puts the repository root on sys.path)

from gcn_max_cut_amd import hip  # noqa: E402
from gcn_max_cut_amd.graph import GraphBatch  # noqa: E402
from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN  # noqa: E402

SWEEPS = 100


def anneal_once(batch, work, inv_t, levels, seed=0, max_descent=100, outputs=False):
    cands = work.shape[0]
    order, cgoff, cptr = batch.refine_order()
    dev = batch.device
    cut_all = torch.empty((batch.B, cands), device=dev)
    best_assign = torch.empty(batch.R, dtype=torch.int32, device=dev)
    best_cut = torch.empty(batch.B, device=dev)
    best_idx = torch.empty(batch.B, dtype=torch.int32, device=dev)
    snap = torch.empty((batch.B, cands), dtype=torch.int32, device=dev) if outputs else None
    sweeps = torch.empty((batch.B, cands), dtype=torch.int32, device=dev) if outputs else None
    p = hip.ptr
    hip.check(hip.load().gmc_refine_anneal_f32(batch.ref(), p(order), p(cgoff), p(cptr), cands, p(work), p(inv_t),
                                               int(inv_t.numel()), p(levels), seed, max_descent, p(cut_all),
                                               p(best_assign), p(best_cut), p(best_idx), p(snap), p(sweeps),
                                               hip.stream()), "gmc_refine_anneal_f32")
    return cut_all, snap, sweeps


def probe_ms(tag, launch, pristine, work, reps):
    launch()                                                   # warm-up (code object load)
    ms = []
    for _ in range(reps):
        work.copy_(pristine)
        with hip.Probe(8) as pr:
            launch()
        ms += [t for name, t in pr.records if name == tag]
    work.copy_(pristine)
    return float(np.median(ms)), float(min(ms))


def time_pair(batch, pristine, reps):
    """Anneal and local-search kernel times on the same candidates, and what they come to per candidate-sweep."""
    dev = batch.device
    inv_t = torch.from_numpy(TN.anneal_schedule(SWEEPS)).to(dev)
    levels = torch.from_numpy(TN.anneal_levels()).to(dev)
    work = pristine.clone()
    a_med, a_min = probe_ms("anneal", lambda: anneal_once(batch, work, inv_t, levels), pristine, work, reps)
    cut_a, snap, sw_a = anneal_once(batch, work, inv_t, levels, outputs=True)
    work.copy_(pristine)
    r_med, r_min = probe_ms("refine", lambda: RT.refine_once(batch, work, 100), pristine, work, reps)
    cut_r, sw_r = RT.refine_once(batch, work, 100, with_sweeps=True)
    torch.cuda.synchronize()
    sw_r, sw_a = sw_r.cpu().numpy(), sw_a.cpu().numpy()
    local_per_sweep = r_med / float(sw_r.mean())
    rec = dict(staged_in_lds=int(hip.load().gmc_refine_anneal_staged(batch.ref())), B=batch.B, R=batch.R,
               candidates=int(pristine.shape[0]), anneal_sweeps=SWEEPS, reps=reps,
               anneal_kernel_ms_median=a_med, anneal_kernel_ms_min=a_min, descent_sweeps_mean=float(sw_a.mean()),
               snapshot_sweep_mean=float(snap.cpu().numpy().mean()),
               local_search_kernel_ms_median=r_med, local_search_kernel_ms_min=r_min,
               local_search_sweeps_mean=float(sw_r.mean()),
               local_search_ms_per_sweep=local_per_sweep,
               anneal_ms_per_sweep_all_time_on_the_anneal_sweeps=a_med / SWEEPS,
               anneal_ms_per_sweep_descent_counted=a_med / (SWEEPS + float(sw_a.mean())),
               ratio_anneal_sweep_to_local_search_sweep=(a_med / SWEEPS) / local_per_sweep,
               mean_cut_annealed=float(cut_a.mean().item()), mean_cut_local_search=float(cut_r.mean().item()),
               mean_best_cut_annealed=float(cut_a.max(dim=1).values.mean().item()),
               mean_best_cut_local_search=float(cut_r.max(dim=1).values.mean().item()))
    return rec


def main():
    profile = "--profile" in sys.argv
    out_path = None if profile else sys.argv[1]
    hip.require_gpu()
    with tempfile.TemporaryDirectory() as workdir:
        net, train_info = RT.train(workdir)
    rec = {"train": train_info}
    if not profile:
        quality = {}
        for n in (100, 200, 300, 500, 1000):
            ds = RT.dataset([(n, 7, 5000 + 10 * n + i) for i in range(10)])
            np.random.seed(0)
            res = TN.decode_dataset(net, ds, 200, local_search_sweeps=100, anneal_sweeps=SWEEPS)
            np.random.seed(0)
            res32 = TN.decode_dataset(net, ds, 200, anneal_sweeps=SWEEPS, anneal_candidates=32)
            mean = lambda rows, key: float(np.mean([r[key] for r in rows]))
            quality[str(n)] = dict(graphs=len(res), argmax=mean(res, "simple_cut"),
                                   post_processing_200=mean(res, "post_cut"), refined=mean(res, "refined_cut"),
                                   annealed=mean(res, "annealed_cut"), annealed_32_candidates=mean(res32, "annealed_cut"),
                                   annealed_below_refined_graphs=int(sum(r["annealed_cut"] < r["refined_cut"] for r in res)))
            print(n, quality[str(n)], flush=True)
        rec["quality_d7"] = quality
        worse = [n for n, q in quality.items() if q["annealed"] < q["refined"]]
        if worse:
            raise SystemExit(f"annealed mean cut below the refined mean at n = {worse}: {quality}")
    reps = 3 if profile else 10
    for name, specs in (("a_configs4_50_graphs", RT.CONFIG_A), ("b_160_graphs_n1000_d7", RT.CONFIG_B)):
        ds = RT.dataset(specs)
        batch, pristine = RT.candidates(net, ds)
        for cands in (201, 32):
            key = f"{name}_{cands}_candidates"
            rec[key] = time_pair(batch, pristine[:cands].contiguous(), reps)
            print(key, rec[key], flush=True)
        if name.startswith("b_"):
            items = list(ds.values())
            ones = [np.ones(it[0].col.size, np.float32) for it in items]
            weighted = GraphBatch([it[0] for it in items], ones, batch.device)
            for cands in (201, 32):
                key = f"{name}_{cands}_candidates_global_memory_path"
                rec[key] = time_pair(weighted, pristine[:cands].contiguous(), reps)
                print(key, rec[key], flush=True)
    rec["device"] = torch.cuda.get_device_name(0)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
