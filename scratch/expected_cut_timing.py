"""The relaxed loss (GMC_LOSS_EXPECTED_CUT, loss="expected_cut") against the hard one: kernel and step times, and what
each trains to.

    python scratch/expected_cut_timing.py OUT.json [--bench-branch LINE.json ...] [--bench-parent LINE.json ...]

1. Head kernel time, hard and relaxed, at 160 x (n = 1000, d = 7), hidden 500: the library's event probe around
   gmc_train_fwd_bwd, median of 30, the two losses alternating.
2. ms per batched step (gmc_train_step_loss_f32, 160 graphs per step): device events around 200 eager steps after 30
   warm-up steps, four windows per loss, alternating.
3. us per graph-step on the reference schedule (one optimizer step per graph; FusedTrainer replays the epoch's hipGraph):
   wall clock around 30 epochs of 160 graph-steps after 5 warm-up epochs (an epoch ends with its losses on the host),
   three windows per loss, alternating.
4. Training: 20 graphs (n = 1000, d = 7), hidden 500, one Adam step per epoch over all 20, 500 epochs, lr 1e-3 and 1e-2,
   each loss from the same seeded initial model: argmax cut as a fraction of the edges on the TRAINING graphs after 200
   and 500 epochs (evaluate_model with the hard loss: -total_loss / edges), and the epoch losses at both points.
--bench-*: result lines of `python bench.py` on this tree and on the parent commit's (same box, alternating), copied
into the record with the ratio of the medians of ms_per_step.
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
from gcn_max_cut_amd import hip  # noqa: E402
from gcn_max_cut_amd.Training import TrainingNeural as T  # noqa: E402
from oracle import ref_dense as R  # noqa: E402

LOSSES = ("cut", "expected_cut")


def handles(count, n=1000, d=7, base=3000):
    return [pkg.from_networkx(R.regular_graph(n, d, base + i)) for i in range(count)]


def dataset(hs):
    """A dataset dict of handles alone: the trainer takes the edge values from the handle (unit weights here)."""
    return {i: (h, None) for i, h in enumerate(hs)}


def model(lr=1e-3, seed=0):
    cfg = T.TrainingConfig(n_nodes=1000, hidden_dim=500, learning_rate=lr)
    torch.manual_seed(seed)
    net, embed, opt = T.setup_model_and_optimizer(cfg)
    return cfg, net, opt


def head_kernel_ms(batch, reps=30):
    _cfg, net, _opt = model()
    eng = net.engine()
    ms = {k: [] for k in LOSSES}
    for k in LOSSES:
        eng.train_fwd_bwd(batch, loss=k)                        # warm-up (code object load)
    for _ in range(reps):
        for k in LOSSES:
            with hip.Probe(16) as pr:
                eng.train_fwd_bwd(batch, loss=k)
            ms[k] += [t for tag, t in pr.records if tag == "head"]
    return {k: dict(head_kernel_ms_median=float(np.median(v)), head_kernel_ms_min=float(min(v)), reps=len(v))
            for k, v in ms.items()}


def batched_step_ms(batch, steps=200, warmup=30, windows=4):
    engines = {}
    for k in LOSSES:
        _cfg, net, _opt = model()
        engines[k] = (net, net.engine())
    out = {k: [] for k in LOSSES}
    bufs = {k: (torch.empty((batch.R, 3), device="cuda"), torch.empty(batch.R, dtype=torch.int32, device="cuda"),
                torch.empty(batch.B, device="cuda")) for k in LOSSES}
    for w in range(windows):
        for k in LOSSES:
            eng = engines[k][1]
            ws = torch.empty(eng.workspace_bytes(batch, True), dtype=torch.uint8, device="cuda")
            eng.sync_step_dev()
            for _ in range(warmup if w == 0 else 5):
                eng.train_step(batch, 1e-3, out=bufs[k], ws=ws, slab=True, loss=k)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                eng.train_step(batch, 1e-3, out=bufs[k], ws=ws, slab=True, loss=k)
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / steps)
    return {k: dict(ms_per_step_median=float(np.median(v)), ms_per_step_windows=[float(x) for x in v], steps=steps)
            for k, v in out.items()}


def reference_schedule_us(ds, epochs=30, warmup=5, windows=3):
    trainers = {}
    for k in LOSSES:
        cfg, net, opt = model()
        net.train()
        trainers[k] = (net, T.FusedTrainer(net, opt, cfg, graphs_per_step=1, loss=k))
    out = {k: [] for k in LOSSES}
    for w in range(windows):
        for k in LOSSES:
            tr = trainers[k][1]
            for _ in range(warmup if w == 0 else 1):
                tr.epoch(ds)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(epochs):
                tr.epoch(ds)
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) / (epochs * len(ds)) * 1e6)
    return {k: dict(us_per_graph_step_median=float(np.median(v)), us_per_graph_step_windows=[float(x) for x in v],
                    graph_steps_per_window=epochs * len(ds), replayed_graph=trainers[k][1]._graph is not None)
            for k, v in out.items()}


def train_run(ds, edges, lr, loss, epochs=500, marks=(200, 500)):
    cfg, net, opt = model(lr)
    tr = T.FusedTrainer(net, opt, cfg, graphs_per_step=len(ds), loss=loss)
    rec = {}
    for e in range(1, epochs + 1):
        net.train()
        epoch_loss = tr.epoch(ds)
        if e in marks:
            hard = T.evaluate_model(net, ds, cfg)["total_loss"]
            relaxed = T.evaluate_model(net, ds, cfg, loss="expected_cut")["total_loss"]
            rec[str(e)] = dict(argmax_cut_fraction=-hard / edges, expected_cut_fraction=-relaxed / edges,
                               last_epoch_training_loss=epoch_loss)
    return rec


def bench_lines(paths):
    lines = []
    for p in paths:
        with open(p) as f:
            text = [ln for ln in f.read().splitlines() if ln.strip().startswith("{")]
        lines.append(json.loads(text[-1]))
    return lines


def main():
    argv = sys.argv[1:]
    out_path = argv[0]
    groups = {"--bench-branch": [], "--bench-parent": []}
    cur = None
    for a in argv[1:]:
        if a in groups:
            cur = a
        else:
            groups[cur].append(a)
    hip.require_gpu()
    rec = {"device": torch.cuda.get_device_name(0),
           "workload": "160 x (n = 1000, d = 7) regular graphs, hidden 500, unit weights"}
    hs = handles(160)
    _cfg, net0, _opt = model()
    batch = net0.engine().make_batch(hs)
    rec["head_kernel"] = head_kernel_ms(batch)
    print("head_kernel", rec["head_kernel"], flush=True)
    rec["batched_step"] = batched_step_ms(batch)
    print("batched_step", rec["batched_step"], flush=True)
    rec["reference_schedule"] = reference_schedule_us(dataset(hs))
    print("reference_schedule", rec["reference_schedule"], flush=True)
    train_hs = handles(20, base=7000)
    edges = sum(h.number_of_edges() for h in train_hs) // 2
    rec["training"] = {"setup": "20 graphs n = 1000 d = 7, hidden 500, one Adam step per epoch over all 20, 500 epochs, "
                                "seed 0; fractions of the 70,000 edges of the TRAINING graphs",
                       "runs": {}}
    for lr in (1e-3, 1e-2):
        for k in LOSSES:
            r = train_run(dataset(train_hs), edges, lr, k)
            rec["training"]["runs"][f"lr={lr:g} loss={k}"] = r
            print("training", lr, k, r, flush=True)
    for key, name in (("--bench-branch", "bench_branch"), ("--bench-parent", "bench_parent")):
        if groups[key]:
            rec[name] = bench_lines(groups[key])
    if groups["--bench-branch"] and groups["--bench-parent"]:
        med = {n: float(np.median([ln["ms_per_step"] for ln in rec[n]])) for n in ("bench_branch", "bench_parent")}
        rec["bench_ms_per_step_median"] = dict(med, branch_over_parent=med["bench_branch"] / med["bench_parent"])
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
