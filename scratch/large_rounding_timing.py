"""The multi-workgroup rounding (gmc_large_round_conditional_f32) against the one-workgroup kernel, and on large graphs.

    python scratch/large_rounding_timing.py profiles/r15_large_rounding.json

(a) 160 x (n = 1000, d = 7) and one n = 4096 graph (d = 7), K = 3: gmc_large_round_conditional_f32 against
    gmc_round_conditional_f32 on the same batch, P and order arrays, at max_descent_sweeps 0 and 100, and the large call
    once more with max_descent_sweeps = the sweeps the slowest graph ran: the difference to 100 is the time of the
    launches issued after convergence.  The outputs of the two kernels are compared byte for byte before timing.
(b) one 7-regular graph of 20,000 nodes and one of 2^20 nodes, K = 3: time, launches and sweeps of the same call.
(c) a 20,000-node graph through train_model (adjacency="none", expected-cut loss, a few epochs) and round_large_dataset:
    the argmax cut, the expected cut, the rounded cut, the rounded + descent cut.  One seed, nothing claimed beyond it.
ms per call: device events around `calls` calls after a warm-up, `windows` windows per variant, the variants of a
workload alternating, median.  P: softmax of normal logits (scale 2), terminals' rows included (never read).
"""
import json
import os
import sys
import tempfile
import time

import networkx as nx
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gcn_max_cut_amd as pkg  # noqa: E402
from gcn_max_cut_amd import hip  # noqa: E402
from tests import large_ref as LR  # noqa: E402
from tests import large_round_ref as LRR  # noqa: E402


class Call:
    """One of the two entry points on a batch, with caller-owned buffers."""

    def __init__(self, name, batch, P, K, descent, large):
        self.name, self.batch, self.large, self.descent = name, batch, large, descent
        lib, p = hip.load(), hip.ptr
        order, cgoff, cptr = batch.refine_order(K)
        self.classes = batch.refine_classes(K)
        self.assign = torch.empty(batch.R, dtype=torch.int8, device="cuda")
        self.cut = torch.empty(batch.B, device="cuda")
        self.expected = torch.empty(batch.B, device="cuda")
        self.sweeps = torch.empty(batch.B, dtype=torch.int32, device="cuda")
        self.keep = (order, cgoff, cptr, P)
        if large:
            need = int(lib.gmc_large_round_workspace_bytes(batch.ref(), K))
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            self.keep += (ws,)
            self.workspace_bytes = need
            self.launches = 1 + 2 + self.classes + descent * (self.classes + 1) + 2

            def call():
                hip.check(lib.gmc_large_round_conditional_f32(
                    batch.ref(), p(P), K, p(order), p(cgoff), p(cptr), self.classes, descent, p(ws), need, p(self.assign),
                    p(self.cut), p(self.expected), p(self.sweeps), hip.stream()), "gmc_large_round_conditional_f32")
        else:
            self.workspace_bytes, self.launches = 0, 1

            def call():
                hip.check(lib.gmc_round_conditional_f32(
                    batch.ref(), p(P), K, p(order), p(cgoff), p(cptr), descent, p(self.assign), p(self.cut),
                    p(self.expected), p(self.sweeps), hip.stream()), "gmc_round_conditional_f32")
        self.call = call

    def run(self, n):
        for _ in range(n):
            self.call()


def measure(variants, calls, warmup, windows):
    ms = {v.name: [] for v in variants}
    for w in range(windows):
        for v in variants:
            v.run(warmup if w == 0 else 2)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            v.run(calls)
            b.record()
            b.synchronize()
            ms[v.name].append(a.elapsed_time(b) / calls)
    out = {}
    for v in variants:
        sw = v.sweeps.cpu().numpy()
        out[v.name] = {"ms_per_call_median": float(np.median(ms[v.name])), "ms_per_call_windows": ms[v.name],
                       "launches": v.launches, "colour_classes": v.classes, "max_descent_sweeps": v.descent,
                       "sweeps_run_max": int(sw.max()), "sweeps_run_mean": float(sw.mean()),
                       "cut_mean": float(v.cut.mean().item()), "expected_mean": float(v.expected.mean().item()),
                       "workspace_bytes": v.workspace_bytes}
        print(v.name, json.dumps(out[v.name]), flush=True)
    return out


def handles(count, n, d, seed):
    return [pkg.GraphHandle(*LR.circulant(n, d, seed + i if d % 2 else None)) for i in range(count)]


def probabilities(batch, K, seed):
    P = np.concatenate([LRR.softmax_rows(int(n), K, seed + i, scale=2.0) for i, n in enumerate(batch.sizes)])
    return torch.from_numpy(P).cuda()


def against_the_one_workgroup_kernel(batch, K, calls, warmup, windows):
    P = probabilities(batch, K, 500)
    old0, new0 = Call("one workgroup, descent 0", batch, P, K, 0, False), Call("large, descent 0", batch, P, K, 0, True)
    old100, new100 = Call("one workgroup, descent 100", batch, P, K, 100, False), Call("large, descent 100", batch, P, K, 100, True)
    for a, b in ((old0, new0), (old100, new100)):
        a.run(1), b.run(1)
        torch.cuda.synchronize()
        assert torch.equal(a.assign, b.assign) and torch.equal(a.sweeps, b.sweeps) and torch.equal(a.cut, b.cut)
    needed = int(new100.sweeps.max().item())
    exact = Call(f"large, descent {needed} (the sweeps the slowest graph ran)", batch, P, K, needed, True)
    out = measure([old0, new0, old100, new100, exact], calls, warmup, windows)
    t = lambda v: out[v.name]["ms_per_call_median"]
    out["ratio large / one workgroup, descent 0"] = t(new0) / t(old0)
    out["ratio large / one workgroup, descent 100"] = t(new100) / t(old100)
    out["ms of the descent-100 call spent on launches after convergence"] = t(new100) - t(exact)
    out["share of the descent-100 call spent on launches after convergence"] = (t(new100) - t(exact)) / t(new100)
    return out


def quality_20000():
    from gcn_max_cut_amd.DataGenerator import graphExtender as GE
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    from gcn_max_cut_amd.Training import TrainingNeural as T
    n = 20000
    _n, rp, col = LR.circulant(n, 7, 77)
    rows = np.repeat(np.arange(n), np.diff(rp))
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(zip(rows[rows < col].tolist(), col[rows < col].tolist()), weight=1)
    ds = GE.process_graphs_from_folder({0: g}, {0: [10, 20, 30]}, n, adjacency="none")
    cfg = T.TrainingConfig(n_nodes=n, hidden_dim=512, number_epochs=20, learning_rate=1e-3)
    torch.manual_seed(0)
    t0 = time.time()
    net, _best, _epoch, _w, history = T.train_model(ds, cfg, loss="expected_cut")
    torch.cuda.synchronize()
    t1 = time.time()
    plain = TN.round_large_dataset(net, ds, 0)[0]
    refined = TN.round_large_dataset(net, ds, 100)[0]
    return {"nodes": n, "edges": int(col.size // 2), "hidden": 512, "epochs": cfg.number_epochs, "loss": "expected_cut",
            "seed": 0, "train_model_host_seconds": round(t1 - t0, 3), "loss_history_first_last": [history[0], history[-1]],
            "argmax_cut": plain["simple_cut"], "expected_cut": plain["expected_cut"], "rounded_cut": plain["rounded_cut"],
            "rounded_and_descent_cut": refined["rounded_cut"], "descent_sweeps": refined["descent_sweeps"]}


def main():
    out_path = os.path.abspath(sys.argv[1])
    os.chdir(tempfile.mkdtemp())   # train_model writes its checkpoints into the working directory
    calls, warmup, windows = 20, 3, 5
    hip.require_gpu()
    rec = {"device": torch.cuda.get_device_name(0),
           "method": f"ms per call: device events around {calls} calls after {warmup} warm-up calls, {windows} windows per "
                     "variant, the variants of a workload alternating, median; K = 3, expected and sweeps requested; the "
                     "two kernels' assign, sweeps and cut compared for equality before timing",
           "workloads": {}}
    w = rec["workloads"]
    batch = pkg.GraphBatch(handles(160, 1000, 7, 3000), None)
    w["(a) 160 x (n = 1000, d = 7)"] = against_the_one_workgroup_kernel(batch, 3, calls, warmup, windows)
    batch = pkg.GraphBatch(handles(1, 4096, 7, 4000), None)
    w["(a) one n = 4096 graph (d = 7)"] = against_the_one_workgroup_kernel(batch, 3, calls, warmup, windows)
    for name, n in (("(b) one n = 20000 graph (d = 7)", 20000), ("(b) one n = 2^20 graph (d = 7)", 1 << 20)):
        batch = pkg.GraphBatch(handles(1, n, 7, 100), None)
        P = probabilities(batch, 3, 700)
        w[name] = measure([Call(f"large, descent {d}", batch, P, 3, d, True) for d in (0, 100)], calls, warmup, windows)
        del batch, P
        torch.cuda.empty_cache()
    rec["(c) quality, one n = 20000 graph through train_model"] = quality_20000()
    print(json.dumps(rec["(c) quality, one n = 20000 graph through train_model"]), flush=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
