"""The dense annealing (gmc_dense_anneal_f32) against the sparse annealing (gmc_kway_refine_anneal_c_f32, K = 2, no
terminals) on the same integer-weight graphs, and what a visit costs.

    python scratch/dense_timing.py OUT.json [quick]

1. G(n, density) with integer weights in -3..4 without 0, n in 512 / 1024 / 2048, density 0.06 / 0.5 / 1.0, 200 candidates
   from random starts, the colour order of the graph for both calls, no descent.  Both calls run the same sweeps and their
   outputs are compared byte for byte, so the comparison is pure time: device events around the whole call, a warm-up of
   each, then PAIRS alternating pairs in one run.  100 sweeps; the sparse call walks n entries per visit with one thread
   at work on these graphs, so above SPARSE_BUDGET entry visits per call both calls run fewer sweeps (recorded) and the
   figure to compare is the time per sweep.  Recorded: ms per sweep of either call (median, min, max), accepted moves per
   sweep and chain, the ratio of the medians and the sparse call's own spread (max - min) / median.
2. A visit's cost, n = 1024 complete: every visit rejected (inv_temp = 1e30 from states the descent has brought to local
   optima) and every visit accepted (inv_temp = 0: delta * 0 <= level always), 20 sweeps, 200 chains; ns per visit of a
   chain and, for the accepted case, the bytes of W rows read per second over the whole device.
3. Sherrington-Kirkpatrick instances J ~ N(0, 1 / n), n = 1024, three seeds, maxcut.solve_ising_dense with 200 chains:
   the energy per spin after 100 and after 1000 sweeps (the Parisi value is -0.7632; the figure depends on the provisional
   temperature unit).
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gcn_max_cut_amd import hip, maxcut  # noqa: E402
from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN  # noqa: E402
from tests import dense_ref as DR  # noqa: E402
from tests import plain_ref as PR  # noqa: E402

CANDS, SWEEPS, PAIRS, SEED = 200, 100, 3, 11
SPARSE_BUDGET = 4.0e8      # entry visits (nnz * sweeps) of one sparse call before the sweeps are cut


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


def timed(launch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    launch()
    b.record()
    torch.cuda.synchronize()
    return float(a.elapsed_time(b))


def stats(ms, sweeps):
    per = [t / sweeps for t in ms]
    return dict(ms_per_sweep_median=median(per), ms_per_sweep_min=min(per), ms_per_sweep_max=max(per), calls=len(ms))


class Sparse:
    """The graph of W as a one-graph gmc_batch with its (colour, id) order, on the device."""

    def __init__(self, W):
        n = W.shape[0]
        rp, cl, w = DR.csr_of_dense(W)
        complete = len(cl) == n * (n - 1)
        classes = [np.asarray([v]) for v in range(n)] if complete else PR.colouring(n, rp, cl, 0)
        self.order_local = np.concatenate(classes).astype(np.int32)
        cptr = np.concatenate([[0], np.cumsum([len(c) for c in classes])]).astype(np.int32)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.keep = [dev(np.asarray([0, n], np.int32)), dev(rp.astype(np.int32)), dev(cl.astype(np.int32)), dev(w),
                     dev(self.order_local), dev(np.asarray([0, len(cptr)], np.int32)), dev(cptr)]
        p = hip.ptr
        self.nnz, self.colours = len(cl), len(classes)
        self.c = hip.GmcBatch(B=1, R=n, nnz=len(cl), n_max=n, nnz_max=len(cl), goff=p(self.keep[0]), rowptr=p(self.keep[1]),
                              lcol=p(self.keep[2]), gcol=p(self.keep[2]), vals=p(self.keep[3]))
        self.order, self.cgoff, self.cptr = self.keep[4:]


def compare(n, density, quick):
    W = DR.weights_of("int", n, 1000 + n, density)
    sp = Sparse(W)
    sweeps = SWEEPS if not quick else 10
    while sp.nnz * sweeps > SPARSE_BUDGET and sweeps > 5:
        sweeps //= 2
    lib, p = hip.load(), hip.ptr
    Wd = torch.from_numpy(W[None]).cuda()
    starts = torch.from_numpy(np.random.RandomState(n).randint(0, 2, (CANDS, n)).astype(np.int8)).cuda()
    inv_temp = TN.anneal_schedule(sweeps, scale=TN.dense_scale(Wd))
    inv_t, levels, _ = TN._schedule_tensors(inv_temp, Wd.device)
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
    out_s = dict(a=torch.empty_like(starts), score=f32(1, CANDS), best=i32(n), bs=f32(1), bi=i32(1), snap=i32(1, CANDS))
    out_d = dict(a=torch.empty_like(starts), score=f32(1, CANDS), best=i32(n), bs=f32(1), bi=i32(1), snap=i32(1, CANDS),
                 moves=torch.empty((1, CANDS), dtype=torch.int64, device="cuda"))
    ws = torch.empty(16, dtype=torch.uint8, device="cuda")

    def sparse():
        o = out_s
        o["a"].copy_(starts)
        return timed(lambda: hip.check(lib.gmc_kway_refine_anneal_c_f32(
            C.byref(sp.c), 2, 0, None, p(sp.order), p(sp.cgoff), p(sp.cptr), CANDS, p(o["a"]), p(inv_t), sweeps, p(levels),
            SEED, 0, p(o["score"]), p(o["best"]), p(o["bs"]), p(o["bi"]), p(o["snap"]), None, hip.stream()), "sparse"))

    def dense():
        o = out_d
        o["a"].copy_(starts)
        return timed(lambda: hip.check(lib.gmc_dense_anneal_f32(
            1, n, p(Wd), n, None, p(sp.order), CANDS, p(o["a"]), p(inv_t), sweeps, p(levels), SEED, 0, p(ws), 16,
            p(o["score"]), p(o["best"]), p(o["bs"]), p(o["bi"]), p(o["snap"]), None, p(o["moves"]), hip.stream()), "dense"))

    first = dict(dense=dense(), sparse=sparse())                      # warm-up of each (and the outputs to compare)
    same = all(bool((out_s[k] == out_d[k]).all()) for k in ("a", "best", "bi", "snap")) and \
        out_s["score"].cpu().numpy().tobytes() == out_d["score"].cpu().numpy().tobytes()
    ms = dict(sparse=[], dense=[])
    for _ in range(PAIRS):
        ms["sparse"].append(sparse())
        ms["dense"].append(dense())
    s, d = stats(ms["sparse"], sweeps), stats(ms["dense"], sweeps)
    rec = dict(n=n, density=density, nnz=sp.nnz, colours=sp.colours, candidates=CANDS, sweeps=sweeps, outputs_identical=same,
               warm_up_ms=first, sparse=s, dense=d,
               moves_per_sweep_per_chain=float(out_d["moves"].sum().item()) / (sweeps * CANDS),
               sparse_over_dense=s["ms_per_sweep_median"] / d["ms_per_sweep_median"],
               sparse_spread=(s["ms_per_sweep_max"] - s["ms_per_sweep_min"]) / s["ms_per_sweep_median"])
    print(json.dumps(rec), flush=True)
    return rec


def visit_cost(n=1024, sweeps=20):
    W = DR.weights_of("real", n, 77)                               # real weights: no visit of delta = 0
    lib, p = hip.load(), hip.ptr
    Wd = torch.from_numpy(W[None]).cuda()
    optima = torch.from_numpy(np.random.RandomState(5).randint(0, 2, (CANDS, n)).astype(np.int8)).cuda()
    TN._dense_anneal_on_gpu(Wd, optima, np.zeros(0, np.float32), 0, 1000)          # the descent: local optima
    levels = torch.from_numpy(TN.anneal_levels()).cuda()
    ws = torch.empty(16, dtype=torch.uint8, device="cuda")
    out = dict(score=torch.empty((1, CANDS), device="cuda"), best=torch.empty(n, dtype=torch.int32, device="cuda"),
               bs=torch.empty(1, device="cuda"), bi=torch.empty(1, dtype=torch.int32, device="cuda"),
               moves=torch.empty((1, CANDS), dtype=torch.int64, device="cuda"))
    rec = {}
    for name, beta in (("rejected", 1e30), ("accepted", 0.0)):
        inv_t = torch.full((sweeps,), beta, dtype=torch.float32, device="cuda")
        work = torch.empty_like(optima)

        def call(k):
            work.copy_(optima)
            return timed(lambda: hip.check(lib.gmc_dense_anneal_f32(
                1, n, p(Wd), n, None, None, CANDS, p(work), p(inv_t), k, p(levels), SEED, 0, p(ws), 16, p(out["score"]),
                p(out["best"]), p(out["bs"]), p(out["bi"]), None, None, p(out["moves"]), hip.stream()), "dense"))
        call(sweeps), call(0)
        full = [call(sweeps) for _ in range(PAIRS)]
        base = [call(0) for _ in range(PAIRS)]                        # the passes and the pick without any sweep
        call(sweeps)
        moves = float(out["moves"].sum().item())
        ms = median(full) - median(base)
        rec[name] = dict(sweeps=sweeps, call_ms=full, call_ms_without_sweeps=base, accepted_moves=moves,
                         ns_per_visit_of_a_chain=ms * 1e6 / (sweeps * n))
        if name == "accepted":
            rec[name]["row_bytes_per_second"] = moves * n * 4 / (ms * 1e-3)
            rec[name]["fraction_of_8_TB_per_s"] = rec[name]["row_bytes_per_second"] / 8e12
    print(json.dumps(rec), flush=True)
    return rec


def sk(n=1024, seeds=(0, 1, 2), sweep_counts=(100, 1000)):
    rows = []
    for seed in seeds:
        g = np.random.RandomState(seed).normal(0.0, 1.0 / np.sqrt(n), (n, n))
        J = np.triu(g, 1)
        J = (J + J.T).astype(np.float32)
        for sweeps in sweep_counts:
            t = time.time()
            res = maxcut.solve_ising_dense(J, candidates=CANDS, anneal_sweeps=sweeps, seed=seed)
            torch.cuda.synchronize()
            rows.append(dict(seed=seed, sweeps=sweeps, energy_per_spin=float(res.energy[0]) / n, wall_s=time.time() - t,
                             moves_per_sweep_per_chain=float(res.result.moves.sum().item()) / (sweeps * CANDS)))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    out_path = sys.argv[1]
    quick = len(sys.argv) > 2 and sys.argv[2] == "quick"
    hip.require_gpu()
    result = dict(device=torch.cuda.get_device_name(0), candidates=CANDS, pairs=PAIRS, comparison=[], parisi=-0.7632)
    sizes = ((512, 1024) if quick else (512, 1024, 2048))
    for n in sizes:
        for density in (0.06, 0.5, 1.0):
            result["comparison"].append(compare(n, density, quick))
            json.dump(result, open(out_path, "w"), indent=1)
    result["visit"] = visit_cost()
    json.dump(result, open(out_path, "w"), indent=1)
    result["sk"] = sk(sweep_counts=(100,) if quick else (100, 1000))
    json.dump(result, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
