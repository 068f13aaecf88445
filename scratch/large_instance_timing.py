"""One model per graph beyond 4096 nodes (gmc_inst_large_*, LargeInstanceEngine, maxcut.solve_large): what the large
sequence costs where both run, and what it does where only it runs.

    python scratch/large_instance_timing.py profiles/out.json [a] [b] [c]

(a) 160 x (n = 1000, d = 7), hidden 500, K = 3, hard loss: one train_fwd_bwd step of LargeInstanceEngine against
    InstanceEngine on the same batch and parameters, the two alternating in this process; and the per-launch times of one
    step of each by the library's probe events.
(b) the step on one 7-regular graph of 20,000 nodes (hidden 64 and 512) and on one of 2^20 nodes (hidden 64), K = 3.
(c) maxcut.solve_large end to end on the 20,000-node graph of DESIGN section 21 (large_ref.circulant(20000, 7, 77)),
    K = 3, hidden 64, 200 epochs, lr 1e-2, expected-cut loss, 32 samples, 100 annealing and at most 20 descent sweeps,
    with and without terminals: cut, trained_cut, rounded_cut, host seconds, peak device memory.  One seed.
ms per call: device events around `calls` calls after a warm-up, `loops` loops per variant, median (min - max).
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gcn_max_cut_amd as pkg  # noqa: E402
from gcn_max_cut_amd import hip, maxcut  # noqa: E402
from tests import large_ref as LR  # noqa: E402

K = 3


def handles(n, d, count, seed):
    return [pkg.GraphHandle(*LR.circulant(n, d, seed + i if d % 2 else None)) for i in range(count)]


def timed(fn, calls, loops=5, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(loops):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return out


def spread(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def engine(cls, hs, F, seed=0):
    eng = getattr(pkg.engine, cls)(hs, F, K)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        eng.reset_parameters()
    return eng


def probe_step(eng):
    out = eng._outputs()
    eng.train_fwd_bwd(1.0, out=out)
    torch.cuda.synchronize()
    with hip.Probe(64) as probe:
        eng.train_fwd_bwd(1.0, out=out)
    return [[t, ms] for t, ms in probe.records]


def part_a():
    hs = handles(1000, 7, 160, 1)
    small, large = engine("InstanceEngine", hs, 500), engine("LargeInstanceEngine", hs, 500)
    so, lo = small._outputs(), large._outputs()
    rec = {"small": [], "large": []}
    for _ in range(3):   # the two alternating
        rec["small"] += timed(lambda: small.train_fwd_bwd(1.0, out=so), 100, loops=3)
        rec["large"] += timed(lambda: large.train_fwd_bwd(1.0, out=lo), 100, loops=3)
    return dict(gmc_inst_train_fwd_bwd=spread(rec["small"]), gmc_inst_large_train_fwd_bwd=spread(rec["large"]),
                launches_small=probe_step(small), launches_large=probe_step(large),
                same_S=bool(torch.equal(so[1], lo[1])))


def part_b():
    rec = {}
    for n, F, calls in ((20000, 64, 100), (20000, 512, 50), (1 << 20, 64, 10)):
        torch.cuda.reset_peak_memory_stats()
        eng = engine("LargeInstanceEngine", handles(n, 7, 1, 77), F)
        out = eng._outputs()
        rec[f"n={n} hidden={F}"] = dict(step=spread(timed(lambda: eng.train_fwd_bwd(1.0, out=out), calls)),
                                        adam=spread(timed(lambda: eng.adam_step(1e-2), calls)),
                                        launches=probe_step(eng), peak_bytes=int(torch.cuda.max_memory_allocated()),
                                        workspace_bytes=eng.workspace_bytes(True), flat_floats=eng.count)
        del eng, out
    return rec


def part_c():
    n, rp, col = LR.circulant(20000, 7, 77)
    rows = np.repeat(np.arange(n), np.diff(rp))
    ei = np.stack([rows, col])
    rec = {"edges": int(col.size // 2)}
    for terminals in (True, False):
        kw = dict(num_nodes=n, number_classes=K, terminals=terminals, hidden_dim=64, epochs=200, learning_rate=1e-2,
                  samples=32, anneal_sweeps=100, max_descent_sweeps=20, seed=0)
        maxcut.solve_large(ei, **{**kw, "epochs": 2})          # warm-up
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        res = maxcut.solve_large(ei, **kw)
        torch.cuda.synchronize()
        rec[f"terminals={terminals}"] = dict(seconds=time.perf_counter() - t0, cut=float(res.cut[0]),
                                             trained_cut=float(res.trained_cut[0]), rounded_cut=float(res.rounded_cut[0]),
                                             peak_bytes=int(torch.cuda.max_memory_allocated()))
    return rec


if __name__ == "__main__":
    path, parts = sys.argv[1], sys.argv[2:] or ["a", "b", "c"]
    rec = json.load(open(path)) if os.path.exists(path) else {}
    for part in parts:
        rec[part] = {"a": part_a, "b": part_b, "c": part_c}[part]()
        print(part, json.dumps(rec[part])[:2000], flush=True)
        json.dump(rec, open(path, "w"), indent=1)
