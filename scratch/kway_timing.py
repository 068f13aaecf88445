"""One training step of the K-class path (gmc_kway_train_fwd_bwd + Adam) against the 3-way sequences, for scale.

    python scratch/kway_timing.py profiles/r09_kway.json

Workload: 160 x (n = 1000, d = 7) regular graphs, hidden 500, unit weights, hard loss.  Timed, in ONE run and alternating:
  kway K=2, 3, 4, 8   train_fwd_bwd (gmc_kway_train_fwd_bwd: the row-kernel sequence with the K-wide kernels) + the generic
                      device-stepped Adam - K = 3 through the engine's own model struct and buffers
  3-way per-op        gmc_train_fwd_bwd under gmc_set_fuse(0) + the same Adam
  3-way fused         gmc_train_fwd_bwd, fused default, + the same Adam (the shipped step, gmc_train_step_f32, also fuses the
                      gradient fold with Adam; it is timed as well)
ms per step: device events around `steps` eager steps after a warm-up, `windows` windows per variant, median.  Per-kernel
times of one step of each variant: the library's event probe, median of `reps` probed steps.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gcn_max_cut_amd as pkg  # noqa: E402
from gcn_max_cut_amd import hip  # noqa: E402
from oracle import ref_dense as R  # noqa: E402

N, HIDDEN, LR = 1000, 500, 1e-3


def engine(K, seed=0):
    eng = pkg.engine.FusedEngine(N, HIDDEN, K, kway=K != 3)
    rng = np.random.RandomState(seed)
    v = eng.views()
    v["conv1.weight"].copy_(torch.from_numpy(rng.uniform(-0.06, 0.06, (N, HIDDEN)).astype(np.float32)))
    v["conv2.weight"].copy_(torch.from_numpy(rng.uniform(-0.1, 0.1, (HIDDEN, K)).astype(np.float32)))
    return eng


class Variant:
    """name, engine, and one step as a closure over caller-owned buffers."""

    def __init__(self, name, K, batch, fuse=None, kway3=False, fused_step=False):
        self.name, self.K, self.fuse = name, K, fuse
        self.eng = eng = engine(K)
        lib = hip.load()
        self.out = (torch.empty((batch.R, K), device="cuda"), torch.empty(batch.R, dtype=torch.int32, device="cuda"),
                    torch.empty(batch.B, device="cuda"))
        if kway3:   # K = 3 through the new entry point: the engine would take the 3-way one
            model = eng._call_model()
            need = int(lib.gmc_kway_workspace_bytes(batch.ref(), C.byref(model), 1))
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            P, S, loss = self.out

            def fwd_bwd():
                rc = lib.gmc_kway_train_fwd_bwd(batch.ref(), C.byref(model), 1.0, hip.ptr(ws), need, hip.ptr(P), hip.ptr(S),
                                                hip.ptr(loss), hip.ptr(eng.grad), hip.stream())
                hip.check(rc, "gmc_kway_train_fwd_bwd")
        else:
            ws = torch.empty(eng.workspace_bytes(batch, True), dtype=torch.uint8, device="cuda")

            def fwd_bwd():
                eng.train_fwd_bwd(batch, 1.0, out=self.out, ws=ws)
        if fused_step:
            self.step = lambda: eng.train_step(batch, LR, 1.0, out=self.out, ws=ws, slab=True)
        else:
            def step():
                fwd_bwd()
                eng.adam_step_dev(LR)
            self.step = step
        self.keep = ws

    def run(self, steps):
        lib = hip.load()
        prev = lib.gmc_set_fuse(self.fuse) if self.fuse is not None else None
        try:
            self.eng.sync_step_dev()
            for _ in range(steps):
                self.step()
        finally:
            if prev is not None:
                lib.gmc_set_fuse(prev)


def main():
    out_path = sys.argv[1]
    steps, warmup, windows, reps = 200, 30, 4, 15
    hip.require_gpu()
    hs = [pkg.from_networkx(R.regular_graph(1000, 7, 3000 + i)) for i in range(160)]
    batch = pkg.GraphBatch(hs, None)
    variants = [Variant(f"kway K={K}", K, batch, kway3=K == 3) for K in (2, 3, 4, 8)]
    variants += [Variant("3-way per-op (gmc_set_fuse(0))", 3, batch, fuse=0),
                 Variant("3-way fused, train_fwd_bwd + Adam", 3, batch, fuse=1),
                 Variant("3-way fused train_step (shipped)", 3, batch, fuse=1, fused_step=True)]
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
    kernels = {}
    for v in variants:
        per = {}
        for _ in range(reps):
            with hip.Probe(32) as pr:
                v.run(1)
            seen = {}
            for tag, t in pr.records:
                seen[tag] = seen.get(tag, 0.0) + t
            for tag, t in seen.items():
                per.setdefault(tag, []).append(t)
        kernels[v.name] = {tag: float(np.median(ts)) for tag, ts in per.items()}
    med = {k: float(np.median(x)) for k, x in ms.items()}
    rec = {"device": torch.cuda.get_device_name(0),
           "workload": "160 x (n = 1000, d = 7) regular graphs, hidden 500, unit weights, hard loss; one step = "
                       "train_fwd_bwd + device-stepped Adam, eager launches",
           "method": f"device events around {steps} steps after {warmup} warm-up steps, {windows} windows per variant, "
                     f"variants alternating; kernel times: event probe, median of {reps} probed steps (dense_mfma = "
                     "the K-class sequence's stand-alone H @ W2 launch, hw2_k)",
           "ms_per_step_median": med, "ms_per_step_windows": ms, "kernel_ms_median": kernels,
           "ratios": {"kway K=3 / 3-way per-op": med["kway K=3"] / med["3-way per-op (gmc_set_fuse(0))"],
                      "kway K=3 / 3-way fused, train_fwd_bwd + Adam": med["kway K=3"] / med["3-way fused, train_fwd_bwd + Adam"],
                      "kway K=3 / shipped train_step": med["kway K=3"] / med["3-way fused train_step (shipped)"],
                      "kway K=2 / kway K=3": med["kway K=2"] / med["kway K=3"],
                      "kway K=4 / kway K=3": med["kway K=4"] / med["kway K=3"],
                      "kway K=8 / kway K=3": med["kway K=8"] / med["kway K=3"]}}
    print(json.dumps({"ms_per_step_median": med, "ratios": rec["ratios"], "kernel_ms_median": kernels}, indent=1), flush=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
