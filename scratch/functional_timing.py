"""Timing of the functional form of the model (profiles/r21_functional.json).

    python scratch/functional_timing.py OUT.json

One forward + backward at 160 x (n = 1000, d = 7), hidden 500, K = 3, in one process, the variants alternating round by
round on one MI355X:

  fn_autograd     P = functional.gcn_softmax(batch, W1, b1, W2, b2); P.backward(GP)     (with its parameter copy and buffers)
  fn_library      gmc_fn_forward + gmc_fn_backward on buffers allocated once
  kway_step       gmc_kway_train_fwd_bwd: the same row kernels with the one-workgroup head and the built-in loss
  net_autograd    the existing 3-class autograd path of net(g, a_pad) on the same batch (gmc_forward + gmc_backward_from_gp)

Times are device events around `REPS` calls; per-launch times come from the library's probe, one call per variant."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gcn_max_cut_amd as pkg  # noqa: E402
from gcn_max_cut_amd import functional as Fn  # noqa: E402
from gcn_max_cut_amd.Training import TrainingNeural as T  # noqa: E402

GRAPHS, N, D, HIDDEN, K = 160, 1000, 7, 500, 3
ROUNDS, REPS, WARMUP = 7, 10, 3


def regular_graph(n, d, seed):
    """A d-regular graph on n nodes (d odd, n even): the ring offsets 1..d//2 plus a seeded perfect matching that avoids
    them; sorted CSR rows."""
    i = np.arange(n)
    cols = [(i + s * o) % n for o in range(1, d // 2 + 1) for s in (1, -1)]
    rng = np.random.RandomState(seed)
    while True:
        perm = rng.permutation(n)
        mate = i.copy()
        mate[perm[:n // 2]], mate[perm[n // 2:]] = perm[n // 2:], perm[:n // 2]
        gap = np.minimum((mate - i) % n, (i - mate) % n)
        if gap.min() > d // 2:
            break
    nb = np.sort(np.stack(cols + [mate], 1), axis=1)
    return n, np.arange(n + 1) * d, nb.ravel()


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(REPS):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / REPS


def main(out_path):
    pkg.hip.require_gpu()
    dev = torch.device("cuda", 0)
    lib, p = pkg.hip.load(), pkg.hip.ptr
    batch = pkg.GraphBatch([pkg.GraphHandle(*regular_graph(N, D, s)) for s in range(GRAPHS)], None, dev)
    rng = np.random.RandomState(0)
    params = {"conv1.weight": rng.uniform(-0.06, 0.06, (N, HIDDEN)).astype(np.float32), "conv1.bias": np.zeros(HIDDEN, np.float32),
              "conv2.weight": rng.uniform(-0.1, 0.1, (HIDDEN, K)).astype(np.float32), "conv2.bias": np.zeros(K, np.float32)}
    net = pkg.engine.module_of({k: torch.from_numpy(v) for k, v in params.items()})
    eng = net.engine()
    named = [dict(net.named_parameters())[k] for k in pkg.engine.PARAM_ORDER]
    GP = torch.from_numpy(rng.standard_normal((batch.R, K)).astype(np.float32)).to(dev)

    def clear():
        for q in named:
            q.grad = None

    def fn_autograd():
        clear()
        Fn.gcn_softmax(batch, *named).backward(GP)

    def net_autograd():
        clear()
        T._GCNForward.apply(net, batch, None, *named).backward(GP)

    keng = pkg.engine.FusedEngine(N, HIDDEN, K, kway=True)
    for k, v in keng.views().items():
        v.copy_(torch.from_numpy(params[k]))
    kout = keng._outputs(batch)

    def kway_step():
        keng.train_fwd_bwd(batch, 1.0, out=kout)

    model = pkg.hip.GmcModel.from_buffer_copy(keng._model)
    model.flags = 0
    need = int(lib.gmc_fn_workspace_bytes(batch.ref(), C.byref(model), 0))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    P = torch.empty((batch.R, K), device=dev)
    grad = torch.empty(keng.count, device=dev)

    def fn_library():
        st = pkg.hip.stream()
        pkg.hip.check(lib.gmc_fn_forward(batch.ref(), C.byref(model), None, 0, p(ws), need, p(P), st), "gmc_fn_forward")
        pkg.hip.check(lib.gmc_fn_backward(batch.ref(), C.byref(model), None, 0, p(ws), need, p(P), p(GP), p(grad), None, 0, st),
                      "gmc_fn_backward")

    variants = {"fn_autograd": fn_autograd, "fn_library": fn_library, "kway_step": kway_step, "net_autograd": net_autograd}
    for fn in variants.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    rounds = {name: [] for name in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            rounds[name].append(timed(fn))
    launches = {}
    for name, fn in variants.items():
        with pkg.hip.Probe(64) as probe:
            fn()
            torch.cuda.synchronize()
        launches[name] = [[tag, round(ms, 5)] for tag, ms in probe.records]
    out = {
        "device": torch.cuda.get_device_name(0),
        "shape": {"graphs": GRAPHS, "n": N, "d": D, "hidden": HIDDEN, "K": K, "rows": batch.R},
        "rounds": ROUNDS, "reps_per_round": REPS, "order": "the variants alternate round by round in one process",
        "forward_backward_ms": {name: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds_ms": v}
                                for name, v in rounds.items()},
        "launches_ms": {name: {"records": rec, "sum_ms": round(sum(ms for _t, ms in rec), 5)} for name, rec in launches.items()},
        "script": "python scratch/functional_timing.py OUT.json",
    }
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    for name, v in out["forward_backward_ms"].items():
        print(f"{name}: median {v['median_ms']:.4f} ms (min {v['min_ms']:.4f}, max {v['max_ms']:.4f}); launches "
              f"{out['launches_ms'][name]['sum_ms']:.4f} ms in {len(launches[name])}")


if __name__ == "__main__":
    main(sys.argv[1])
