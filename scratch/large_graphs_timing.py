"""One training step of the large-graph path (gmc_large_train_fwd_bwd + Adam), and the split head against head_k_kernel.

    python scratch/large_graphs_timing.py profiles/r14_large_graphs.json

Workloads (circulant graphs of tests/large_ref.py: node i next to i +- 1.., odd degree: a seeded matching on top):
  1 x and 8 x (n = 20,000, d = 7), hidden 512, K = 3 and K = 8      the engine's own routing (FusedEngine.train_fwd_bwd)
  n = 2^20, d = 4, hidden 64, K = 3                                with the workspace bytes
  160 x (n = 1000, d = 7), hidden 500, K = 3                       gmc_large_* against gmc_kway_* on the same batch
  one n = 4096 graph (d = 7), hidden 512, K = 3                    the same two: head_k_kernel is one workgroup there
One step = train_fwd_bwd + the generic device-stepped Adam, eager launches.  ms per step: device events around `steps` steps
after a warm-up, `windows` windows per variant, the variants of a workload alternating, median.  Per-launch times: the
library's event probe, median of `reps` probed steps, in launch order (the large head is records 3..6: probabilities, loss
and softmax backward, fold, GY2).  Last: a 20,000-node graph through train_model and evaluate_model from an
adjacency="none" dataset (two epochs; says that it ran, and how long the calls took on the host clock).
"""
import ctypes as C
import json
import os
import sys
import time

import networkx as nx
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gcn_max_cut_amd as pkg  # noqa: E402
from gcn_max_cut_amd import hip  # noqa: E402
from tests import large_ref as LR  # noqa: E402

LRATE = 1e-3


def engine(N, hidden, K, seed=0):
    eng = pkg.engine.FusedEngine(N, hidden, K, kway=K != 3)
    rng = np.random.RandomState(seed)
    v = eng.views()
    v["conv1.weight"].copy_(torch.from_numpy(rng.uniform(-0.06, 0.06, (N, hidden)).astype(np.float32)))
    v["conv2.weight"].copy_(torch.from_numpy(rng.uniform(-0.1, 0.1, (hidden, K)).astype(np.float32)))
    return eng


class Variant:
    """name, engine, and one step as a closure over caller-owned buffers.  entry: "engine" (its own routing), or the
    prefix of the library's entry points called directly ("gmc_large", "gmc_kway")."""

    def __init__(self, name, batch, N, hidden, K, entry="engine"):
        self.name = name
        self.eng = eng = engine(N, hidden, K)
        lib = hip.load()
        P = torch.empty((batch.R, K), device="cuda")
        S = torch.empty(batch.R, dtype=torch.int32, device="cuda")
        loss = torch.empty(batch.B, device="cuda")
        if entry == "engine":
            self.ws_bytes = eng.workspace_bytes(batch, True)
            ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device="cuda")
            self.large = eng.needs_large(batch)

            def fwd_bwd():
                eng.train_fwd_bwd(batch, 1.0, out=(P, S, loss), ws=ws)
        else:
            model = eng._call_model()
            self.ws_bytes = need = int(getattr(lib, entry + "_workspace_bytes")(batch.ref(), C.byref(model), 1))
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            call = getattr(lib, entry + "_train_fwd_bwd")
            self.large = entry == "gmc_large"

            def fwd_bwd():
                rc = call(batch.ref(), C.byref(model), 1.0, hip.ptr(ws), need, hip.ptr(P), hip.ptr(S), hip.ptr(loss),
                          hip.ptr(eng.grad), hip.stream())
                hip.check(rc, entry)

        def step():
            fwd_bwd()
            eng.adam_step_dev(LRATE)
        self.step = step
        self.keep = (ws, P, S, loss, batch)

    def run(self, steps):
        self.eng.sync_step_dev()
        for _ in range(steps):
            self.step()


def measure(variants, steps, warmup, windows, reps):
    ms = {v.name: [] for v in variants}
    for w in range(windows):
        for v in variants:
            v.run(warmup if w == 0 else 5)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            v.run(steps)
            b.record()
            b.synchronize()
            ms[v.name].append(a.elapsed_time(b) / steps)
    out = {}
    for v in variants:
        runs = []
        for _ in range(reps):
            with hip.Probe(32) as pr:
                v.run(1)
            runs.append(pr.records)
        tags = [t for t, _ in runs[0]]
        assert all([t for t, _ in r] == tags for r in runs)
        launches = [[tag, round(1e3 * float(np.median([r[i][1] for r in runs])), 2)] for i, tag in enumerate(tags)]
        head = [us for tag, us in launches if tag == "head"]
        out[v.name] = {"ms_per_step_median": float(np.median(ms[v.name])), "ms_per_step_windows": ms[v.name],
                       "launch_us_median": launches, "head_us": head, "head_us_total": round(sum(head), 2),
                       "large_sequence": bool(v.large), "workspace_bytes": int(v.ws_bytes)}
        print(v.name, json.dumps(out[v.name]), flush=True)
    return out


def handles(count, n, d, seed):
    return [pkg.GraphHandle(*LR.circulant(n, d, seed + i if d % 2 else None)) for i in range(count)]


def train_and_evaluate_20000():
    from gcn_max_cut_amd.DataGenerator import graphExtender as GE
    from gcn_max_cut_amd.Training import TrainingNeural as T
    n = 20000
    _n, rp, col = LR.circulant(n, 7, 77)
    rows = np.repeat(np.arange(n), np.diff(rp))
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(zip(rows[rows < col].tolist(), col[rows < col].tolist()), weight=1)
    ds = GE.process_graphs_from_folder({0: g}, {0: [10, 20, 30]}, n, adjacency="none")
    assert len(ds) == 1 and ds[0][1] is None
    cfg = T.TrainingConfig(n_nodes=n, hidden_dim=512, number_epochs=2, learning_rate=1e-3)
    torch.manual_seed(0)
    t0 = time.time()
    net, best, epoch, _w, history = T.train_model(ds, cfg)
    torch.cuda.synchronize()
    t1 = time.time()
    ev = T.evaluate_model(net, ds, cfg)
    torch.cuda.synchronize()
    t2 = time.time()
    with torch.no_grad():
        P = net(ds[0][0], None)
    S = P.argmax(1).cpu().numpy()
    S[:3] = [0, 1, 2]
    h = ds[0][0]                                   # (the terminals were moved onto 0, 1, 2: the handle's own CSR)
    rows, col = np.repeat(np.arange(n), np.diff(h.rowptr)), h.col
    cut = int((S[rows] != S[col]).sum()) // 2
    assert ev["total_loss"] == -float(cut), (ev, cut)
    return {"nodes": n, "edges": int(col.size // 2), "hidden": 512, "epochs": 2, "loss_history": history,
            "evaluate_model_total_loss": ev["total_loss"], "numpy_cut_of_the_argmax_partition": cut,
            "train_model_host_seconds": round(t1 - t0, 3), "evaluate_model_host_seconds": round(t2 - t1, 3),
            "large_sequence": bool(net._fused_trainer._large)}


def main():
    out_path = sys.argv[1]
    steps, warmup, windows, reps = 200, 20, 3, 9
    hip.require_gpu()
    rec = {"device": torch.cuda.get_device_name(0),
           "method": f"one step = train_fwd_bwd + device-stepped Adam, eager; device events around {steps} steps after "
                     f"{warmup} warm-up steps, {windows} windows per variant, the variants of a workload alternating, median; "
                     f"launch times: event probe, median of {reps} probed steps, in launch order (dense_mfma = hw2_k; the "
                     "large head = the four head records: probabilities, loss + softmax backward, fold, GY2)",
           "workloads": {}}
    w = rec["workloads"]
    for count in (1, 8):
        batch = pkg.GraphBatch(handles(count, 20000, 7, 100), None)
        w[f"{count} x (n = 20000, d = 7), hidden 512"] = measure(
            [Variant(f"K={K}", batch, 20000, 512, K) for K in (3, 8)], steps, warmup, windows, reps)
        del batch
    batch = pkg.GraphBatch(handles(1, 1 << 20, 4, 0), None)
    w["n = 2^20, d = 4, hidden 64"] = measure([Variant("K=3", batch, 1 << 20, 64, 3)], steps, warmup, windows, reps)
    del batch
    torch.cuda.empty_cache()
    batch = pkg.GraphBatch(handles(160, 1000, 7, 3000), None)
    w["160 x (n = 1000, d = 7), hidden 500, K = 3"] = measure(
        [Variant("large (four head launches)", batch, 1000, 500, 3, "gmc_large"),
         Variant("kway (head_k_kernel)", batch, 1000, 500, 3, "gmc_kway")], steps, warmup, windows, reps)
    batch = pkg.GraphBatch(handles(1, 4096, 7, 4000), None)
    w["one n = 4096 graph (d = 7), hidden 512, K = 3"] = measure(
        [Variant("large (four head launches)", batch, 4096, 512, 3, "gmc_large"),
         Variant("kway (head_k_kernel)", batch, 4096, 512, 3, "gmc_kway")], steps, warmup, windows, reps)
    del batch
    torch.cuda.empty_cache()
    rec["train_model and evaluate_model, one n = 20000 graph, adjacency='none'"] = train_and_evaluate_20000()
    print(json.dumps(rec["train_model and evaluate_model, one n = 20000 graph, adjacency='none'"]), flush=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
