"""One training step of the attention path (gmc_att_train_fwd_bwd + Adam) against the K-class path at K = 3, and the
training quality of both first layers on the 20-graph training set of DESIGN section 13.

    python scratch/attention_timing.py profiles/r13_attention.json

Timing workload: 160 x (n = 1000, d = 7) regular graphs, hidden 500, unit weights, hard loss.  Timed, in ONE run and
alternating:
  attention     FusedEngine(N, F, 3, attention=True): train_fwd_bwd (the row-kernel sequence with the kernels of
                csrc/attention.hip) + the generic device-stepped Adam
  kway K=3      FusedEngine(N, F, 3, kway=True): the same row-kernel plan with GraphConv as layer 1 + the same Adam
ms per step: device events around `steps` eager steps after a warm-up, `windows` windows per variant, median.  Per-launch
times of one step of each variant: the library's event probe, median of `reps` probed steps, in launch order (the attention
launches reuse tags: scores and H @ W2 are both "dense_mfma", the edge backward and the transposed aggregation both
"agg_bwd", ...; LAUNCHES names them by position).

Quality: 20 graphs (n = 1000, d = 7, seeds 7000..7019), hidden 500, one Adam step per epoch over all 20, lr 1e-2, one seed,
each loss and each first layer from its seeded initial model: the argmax cut as a fraction of the edges on the TRAINING
graphs after the same number of epochs.  Reported as it comes: nothing is claimed about held-out graphs or about which
layer is better.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gcn_max_cut_amd as pkg  # noqa: E402
from gcn_max_cut_amd import hip  # noqa: E402
from gcn_max_cut_amd.Training import TrainingNeural as T  # noqa: E402
from oracle import ref_dense as R  # noqa: E402

N, HIDDEN, LR = 1000, 500, 1e-3
LAUNCHES = {
    "attention": ["gather_w1", "scores", "att_fwd", "hw2", "head", "gy2_scale", "hidden_bwd", "colsum", "edge_bwd", "bwd_t",
                  "avec_part", "avec_fold", "dw1", "adam"],
    "kway K=3": ["gather_w1", "agg_fwd", "hw2", "head", "hidden_bwd", "colsum", "agg_bwd", "dw1", "adam"],
}


def engine(seed=0, **mode):
    eng = pkg.engine.FusedEngine(N, HIDDEN, 3, **mode)
    rng = np.random.RandomState(seed)
    v = eng.views()
    v["conv1.weight"].copy_(torch.from_numpy(rng.uniform(-0.06, 0.06, (N, HIDDEN)).astype(np.float32)))
    v["conv2.weight"].copy_(torch.from_numpy(rng.uniform(-0.1, 0.1, (HIDDEN, 3)).astype(np.float32)))
    if eng.attention:
        bound = float(np.sqrt(6.0 / (HIDDEN + 1)))
        for k in ("conv1.attn_src", "conv1.attn_dst"):
            v[k].copy_(torch.from_numpy(rng.uniform(-bound, bound, HIDDEN).astype(np.float32)))
    return eng


class Variant:
    def __init__(self, name, batch, **mode):
        self.name = name
        self.eng = eng = engine(**mode)
        self.out = (torch.empty((batch.R, 3), device="cuda"), torch.empty(batch.R, dtype=torch.int32, device="cuda"),
                    torch.empty(batch.B, device="cuda"))
        self.ws = ws = torch.empty(eng.workspace_bytes(batch, True), dtype=torch.uint8, device="cuda")

        def step():
            eng.train_fwd_bwd(batch, 1.0, out=self.out, ws=ws)
            eng.adam_step_dev(LR)
        self.step = step

    def run(self, steps):
        self.eng.sync_step_dev()
        for _ in range(steps):
            self.step()


def step_times(batch, steps=200, warmup=30, windows=4, reps=15):
    variants = [Variant("attention", batch, attention=True), Variant("kway K=3", batch, kway=True)]
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
    launches = {}
    for v in variants:
        per = None
        for _ in range(reps):
            with hip.Probe(32) as pr:
                v.run(1)
            per = per or [[] for _ in pr.records]
            assert len(pr.records) == len(per) >= len(LAUNCHES[v.name]), (v.name, [t for t, _ in pr.records])
            for i, (_tag, t) in enumerate(pr.records):
                per[i].append(t)
        tags = [t for t, _ in pr.records]
        # the launches up to dW1 by position; what follows (a fold of dW1 chunks, Adam and its counter) by its own tag
        names = LAUNCHES[v.name][:-1] + tags[len(LAUNCHES[v.name]) - 1:]
        launches[v.name] = [dict(launch=name, tag=tag, ms=float(np.median(ts))) for name, tag, ts in zip(names, tags, per)]
    med = {k: float(np.median(x)) for k, x in ms.items()}
    by = {}
    for name, rows in launches.items():
        by[name] = {}
        for r in rows:
            by[name][r["launch"]] = by[name].get(r["launch"], 0.0) + r["ms"]
    a, k = by["attention"], by["kway K=3"]
    compare = {"att_fwd / agg_fwd": a["att_fwd"] / k["agg_fwd"],
               "(edge_bwd + bwd_t) / agg_bwd": (a["edge_bwd"] + a["bwd_t"]) / k["agg_bwd"],
               "att_fwd_ms": a["att_fwd"], "agg_fwd_ms": k["agg_fwd"], "edge_bwd_ms": a["edge_bwd"], "bwd_t_ms": a["bwd_t"],
               "agg_bwd_ms": k["agg_bwd"],
               "other attention-only launches (scores, gy2_scale, avec_part, avec_fold) ms":
                   a["scores"] + a["gy2_scale"] + a["avec_part"] + a["avec_fold"]}
    return dict(method=f"device events around {steps} steps after {warmup} warm-up steps, {windows} windows per variant, "
                       f"variants alternating; launch times: event probe, median of {reps} probed steps",
                ms_per_step_median=med, ms_per_step_windows=ms, ratio_attention_over_kway3=med["attention"] / med["kway K=3"],
                launches_ms_median=launches, layer1_kernels=compare)


def quality(epochs=200, lr=1e-2, seed=0):
    hs = [pkg.from_networkx(R.regular_graph(1000, 7, 7000 + i)) for i in range(20)]
    ds = {i: (h, None) for i, h in enumerate(hs)}
    edges = sum(h.number_of_edges() for h in hs) / 2
    out = {}
    for layer1 in ("graphconv", "attention"):
        for loss in ("cut", "expected_cut"):
            cfg = T.TrainingConfig(n_nodes=N, hidden_dim=HIDDEN, learning_rate=lr)
            torch.manual_seed(seed)
            net, _embed, opt = T.setup_model_and_optimizer(cfg, layer1=layer1)
            tr = T.FusedTrainer(net, opt, cfg, graphs_per_step=len(ds), loss=loss)
            last = None
            for _ in range(epochs):
                net.train()
                last = tr.epoch(ds)
            hard = T.evaluate_model(net, ds, cfg)["total_loss"]
            out[f"{layer1}, loss={loss}"] = dict(argmax_cut_fraction=-hard / edges, last_epoch_training_loss=last)
    return dict(setup=f"20 graphs n = 1000 d = 7 (seeds 7000..7019), hidden 500, one Adam step per epoch over all 20, "
                      f"{epochs} epochs, lr {lr}, torch seed {seed}; argmax cut / edges on the TRAINING graphs",
                runs=out)


def main():
    out_path = sys.argv[1]
    hip.require_gpu()
    hs = [pkg.from_networkx(R.regular_graph(1000, 7, 3000 + i)) for i in range(160)]
    batch = pkg.GraphBatch(hs, None)
    rec = {"device": torch.cuda.get_device_name(0),
           "workload": "160 x (n = 1000, d = 7) regular graphs, hidden 500, unit weights, hard loss; one step = "
                       "train_fwd_bwd + device-stepped Adam, eager launches",
           "step": step_times(batch)}
    print(json.dumps(rec["step"], indent=1), flush=True)
    rec["quality"] = quality()
    print(json.dumps(rec["quality"], indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
