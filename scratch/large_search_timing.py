"""The multi-workgroup sampler and annealing (gmc_large_sample_seeded_f32, gmc_large_anneal_f32) against the
one-workgroup kernels, and on large graphs.

    python scratch/large_search_timing.py profiles/r16_large_search.json [a] [b] [c] [d]

(a) 160 x (n = 1000, d = 7) and one n = 4096 graph (d = 7), K = 3, 201 candidates (random classes), 100 annealing
    sweeps, max_descent_sweeps 100: gmc_large_anneal_f32 against gmc_kway_refine_anneal_f32 on the same batch, candidates
    and order arrays, and the large call once more with max_descent_sweeps = the sweeps the slowest candidate ran: the
    difference to 100 is the time of the launches issued after convergence.  Every output of the two kernels is compared
    for equality before timing.
(b) the same two batches: gmc_large_sample_seeded_f32 against gmc_kway_decode_sample_seeded_f32 at 200 samples, with
    assign_all.
(c) one 7-regular graph of 20,000 nodes and one of 2^20 nodes, K = 3: the three calls search_large_dataset makes after
    its forward (rounding at descent 0, sampler, annealing with 100 sweeps and max_descent_sweeps 20) on softmax rows of
    normal logits, at 202 candidates (200 samples) and at 10 (8 samples): ms per stage, launches, peak device memory.
(d) a 20,000-node graph through train_model (adjacency="none", expected-cut loss, 20 epochs) and search_large_dataset:
    the argmax cut, the rounded cut, the rounded + descent cut, the searched cut at 202 and at 10 candidates, host
    seconds and peak device memory of the call.  One seed, nothing claimed beyond it.
ms per call: device events around `calls` calls after a warm-up, `windows` windows per variant, the variants of a
workload alternating, median.
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
from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN  # noqa: E402
from tests import large_ref as LR  # noqa: E402
from tests import large_round_ref as LRR  # noqa: E402

K = 3


class Anneal:
    """One of the two annealing entry points on a batch, with caller-owned buffers; every call starts from `start`."""

    def __init__(self, name, batch, start, sweeps, descent, large):
        self.name, self.large = name, large
        lib, p = hip.load(), hip.ptr
        order, cgoff, cptr = batch.refine_order(K)
        classes = batch.refine_classes(K)
        cands = int(start.shape[0])
        self.assign = start.clone()
        self.out = dict(cut_all=torch.empty((batch.B, cands), device="cuda"),
                        best_assign=torch.empty(batch.R, dtype=torch.int32, device="cuda"),
                        best_cut=torch.empty(batch.B, device="cuda"),
                        best_idx=torch.empty(batch.B, dtype=torch.int32, device="cuda"),
                        snap=torch.empty((batch.B, cands), dtype=torch.int32, device="cuda"),
                        sweeps=torch.empty((batch.B, cands), dtype=torch.int32, device="cuda"))
        o = self.out
        inv_t = torch.from_numpy(TN.anneal_schedule(sweeps)).cuda() if sweeps else None
        lv = torch.from_numpy(TN.anneal_levels()).cuda() if sweeps else None
        self.keep = (order, cgoff, cptr, inv_t, lv, start)
        self.info = {"colour_classes": classes, "candidates": cands, "anneal_sweeps": sweeps, "max_descent_sweeps": descent}
        if large:
            need = int(lib.gmc_large_search_workspace_bytes(batch.ref(), K, cands))
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            self.keep += (ws,)
            self.info["workspace_bytes"] = need
            self.info["launches"] = 5 + (2 + sweeps * (classes + 3) if sweeps else 0) + descent * (classes + 1)

            def call():
                self.assign.copy_(start)
                hip.check(lib.gmc_large_anneal_f32(
                    batch.ref(), K, p(order), p(cgoff), p(cptr), classes, cands, p(self.assign), p(inv_t), sweeps, p(lv), 7,
                    descent, p(ws), need, p(o["cut_all"]), p(o["best_assign"]), p(o["best_cut"]), p(o["best_idx"]),
                    p(o["snap"]), p(o["sweeps"]), hip.stream()), "gmc_large_anneal_f32")
        else:
            self.info["launches"] = 2

            def call():
                self.assign.copy_(start)
                hip.check(lib.gmc_kway_refine_anneal_f32(
                    batch.ref(), K, p(order), p(cgoff), p(cptr), cands, p(self.assign), p(inv_t), sweeps, p(lv), 7,
                    descent, p(o["cut_all"]), p(o["best_assign"]), p(o["best_cut"]), p(o["best_idx"]), p(o["snap"]),
                    p(o["sweeps"]), hip.stream()), "gmc_kway_refine_anneal_f32")
        self.call = call

    def results(self):
        return dict(self.out, assign=self.assign)

    def describe(self):
        sw = self.out["sweeps"].cpu().numpy()
        return dict(self.info, descent_sweeps_run_max=int(sw.max()), descent_sweeps_run_mean=float(sw.mean()),
                    best_cut_mean=float(self.out["best_cut"].mean().item()))


class Sample:
    def __init__(self, name, batch, P, iters, large):
        self.name = name
        lib, p = hip.load(), hip.ptr
        gkey = torch.from_numpy(TN.sample_keys(5, range(batch.B)).view(np.int64)).cuda()
        self.out = dict(assign_all=torch.empty((iters, batch.R), dtype=torch.int8, device="cuda"),
                        cut_all=torch.empty((batch.B, iters), device="cuda"),
                        best_assign=torch.empty(batch.R, dtype=torch.int32, device="cuda"),
                        best_cut=torch.empty(batch.B, device="cuda"),
                        best_iter=torch.empty(batch.B, dtype=torch.int32, device="cuda"))
        o = self.out
        self.keep = (gkey, P)
        self.info = {"samples": iters}
        if large:
            need = int(lib.gmc_large_search_workspace_bytes(batch.ref(), K, iters))
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            self.keep += (ws,)
            self.info.update(workspace_bytes=need, launches=5)

            def call():
                hip.check(lib.gmc_large_sample_seeded_f32(
                    batch.ref(), p(P), K, p(gkey), iters, p(o["assign_all"]), p(ws), need, p(o["cut_all"]),
                    p(o["best_assign"]), p(o["best_cut"]), p(o["best_iter"]), hip.stream()), "gmc_large_sample_seeded_f32")
        else:
            self.info["launches"] = 2

            def call():
                hip.check(lib.gmc_kway_decode_sample_seeded_f32(
                    batch.ref(), p(P), K, p(gkey), iters, p(o["assign_all"]), p(o["cut_all"]), p(o["best_assign"]),
                    p(o["best_cut"]), p(o["best_iter"]), hip.stream()), "gmc_kway_decode_sample_seeded_f32")
        self.call = call

    def results(self):
        return self.out

    def describe(self):
        return dict(self.info, best_cut_mean=float(self.out["best_cut"].mean().item()))


def measure(variants, calls, warmup, windows):
    ms = {v.name: [] for v in variants}
    for w in range(windows):
        for v in variants:
            for _ in range(warmup if w == 0 else 1):
                v.call()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                v.call()
            b.record()
            b.synchronize()
            ms[v.name].append(a.elapsed_time(b) / calls)
    out = {}
    for v in variants:
        out[v.name] = dict(ms_per_call_median=float(np.median(ms[v.name])), ms_per_call_windows=ms[v.name], **v.describe())
        print(v.name, json.dumps(out[v.name]), flush=True)
    return out


def equal_outputs(a, b):
    a.call(), b.call()
    torch.cuda.synchronize()
    ra, rb = a.results(), b.results()
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k


def handles(count, n, d, seed):
    return [pkg.GraphHandle(*LR.circulant(n, d, seed + i if d % 2 else None)) for i in range(count)]


def probabilities(batch, seed):
    P = np.concatenate([LRR.softmax_rows(int(n), K, seed + i, scale=2.0) for i, n in enumerate(batch.sizes)])
    return torch.from_numpy(P).cuda()


def random_candidates(batch, cands, seed):
    A = np.random.RandomState(seed).randint(0, K, (cands, batch.R)).astype(np.int8)
    for lo in batch.goff_host[:-1]:
        A[:, int(lo):int(lo) + K] = np.arange(K, dtype=np.int8)
    return torch.from_numpy(A).cuda()


def against_the_one_workgroup_kernels(batch, parts, calls, warmup, windows):
    out = {}
    if "a" in parts:
        start = random_candidates(batch, 201, 11)
        old, new = Anneal("one workgroup", batch, start, 100, 100, False), Anneal("large", batch, start, 100, 100, True)
        equal_outputs(old, new)
        needed = int(new.out["sweeps"].max().item())
        exact = Anneal(f"large, max_descent_sweeps {needed} (the sweeps the slowest candidate ran)", batch, start, 100,
                       needed, True)
        r = measure([old, new, exact], calls, warmup, windows)
        t = lambda v: r[v.name]["ms_per_call_median"]
        r["ratio large / one workgroup"] = t(new) / t(old)
        r["ms of the large call spent on descent launches after convergence"] = t(new) - t(exact)
        r["share of the large call spent on descent launches after convergence"] = (t(new) - t(exact)) / t(new)
        out["annealing, 201 candidates, 100 sweeps, max_descent_sweeps 100"] = r
    if "b" in parts:
        P = probabilities(batch, 500)
        old, new = Sample("one workgroup", batch, P, 200, False), Sample("large", batch, P, 200, True)
        equal_outputs(old, new)
        r = measure([old, new], calls, warmup, windows)
        r["ratio large / one workgroup"] = r["large"]["ms_per_call_median"] / r["one workgroup"]["ms_per_call_median"]
        out["sampler, 200 samples"] = r
    return out


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    b.synchronize()
    return res, a.elapsed_time(b)


def stages_of_the_search(n, samples, sweeps, descent):
    """The calls search_large_dataset makes after its forward, on one graph of n nodes."""
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    batch = pkg.GraphBatch(handles(1, n, 7, 100), None)
    P = probabilities(batch, 700)
    S = P.argmax(1).to(torch.int8)
    S[:K] = torch.arange(K, dtype=torch.int8, device="cuda")
    batch.refine_order(K)
    rec = {"nodes": n, "samples": samples, "candidates": samples + 2, "anneal_sweeps": sweeps,
           "max_descent_sweeps": descent, "colour_classes": batch.refine_classes(K)}
    for attempt in ("first call ms", "second call ms"):
        ws = TN._large_search_workspace(batch, K, samples + 2)
        (rnd, _cut, _e, _s), t_round = timed(lambda: TN._round_on_gpu(batch, P, 0, large=True))
        (_ba, best_cut, _ca, assign_all), t_sample = timed(
            lambda: TN._kway_sample_on_gpu(batch, P, samples, 5, [0], True, large=True, workspace=ws))
        cands = torch.cat([S.reshape(1, -1), rnd.reshape(1, -1), assign_all]).contiguous()
        (_fa, found_cut, found_idx), t_anneal = timed(
            lambda: TN._kway_anneal_on_gpu(batch, K, cands, TN.anneal_schedule(sweeps), 3, descent, large=True,
                                           workspace=ws))
        rec[attempt] = {"rounding at descent 0": t_round, "sampler": t_sample, "annealing": t_anneal}
        rec["workspace_bytes"] = int(ws.numel())
        rec["rounded_cut"], rec["best_sample_cut"] = float(_cut.item()), float(best_cut.item())
        rec["searched_cut"], rec["searched_from"] = float(found_cut.item()), int(found_idx.item())
        del ws, cands, assign_all
    classes = rec["colour_classes"]
    rec["launches of the annealing"] = 5 + 2 + sweeps * (classes + 3) + descent * (classes + 1)
    rec["peak_device_bytes_above_start"] = int(torch.cuda.max_memory_allocated() - base)
    print(json.dumps(rec), flush=True)
    return rec


def quality_20000():
    from gcn_max_cut_amd.DataGenerator import graphExtender as GE
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
    net, _best, _epoch, _w, history = T.train_model(ds, cfg, loss="expected_cut")
    torch.cuda.synchronize()
    refined = TN.round_large_dataset(net, ds, 100)[0]
    rec = {"nodes": n, "edges": int(col.size // 2), "hidden": 512, "epochs": cfg.number_epochs, "loss": "expected_cut",
           "seed": 0, "loss_history_first_last": [history[0], history[-1]],
           "rounded_and_descent_cut": refined["rounded_cut"], "descent_sweeps": refined["descent_sweeps"]}
    for samples in (200, 8):
        TN.search_large_dataset(net, ds, samples=samples, max_descent_sweeps=20)   # warm-up (order arrays, allocator)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.time()
        res = TN.search_large_dataset(net, ds, samples=samples, max_descent_sweeps=20)[0]
        torch.cuda.synchronize()
        rec[f"search_large_dataset, {samples + 2} candidates, 100 sweeps, max_descent_sweeps 20"] = {
            "host_seconds": round(time.time() - t0, 3), "peak_device_bytes_above_start": int(torch.cuda.max_memory_allocated() - base),
            "argmax_cut": res["simple_cut"], "expected_cut": res["expected_cut"], "rounded_cut": res["rounded_cut"],
            "best_sample_cut": res["post_cut"], "searched_cut": res["searched_cut"], "searched_from": res["searched_from"]}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    out_path = os.path.abspath(sys.argv[1])
    parts = set(sys.argv[2:]) or set("abcd")
    os.chdir(tempfile.mkdtemp())   # train_model writes its checkpoints into the working directory
    calls, warmup, windows = 2, 1, 3
    hip.require_gpu()
    rec = json.load(open(out_path)) if os.path.exists(out_path) else {}
    rec["device"] = torch.cuda.get_device_name(0)
    rec["method"] = (f"ms per call: device events around {calls} calls after {warmup} warm-up call, {windows} windows per "
                     "variant, the variants of a workload alternating, median; K = 3, unit weights; every output of the "
                     "two kernels compared for equality before timing; each annealing call copies the candidates in first")
    w = rec.setdefault("workloads", {})
    if parts & set("ab"):
        for name, batch in (("160 x (n = 1000, d = 7)", pkg.GraphBatch(handles(160, 1000, 7, 3000), None)),
                            ("one n = 4096 graph (d = 7)", pkg.GraphBatch(handles(1, 4096, 7, 4000), None))):
            w.setdefault(name, {}).update(against_the_one_workgroup_kernels(batch, parts, calls, warmup, windows))
    if "c" in parts:
        for n in (20000, 1 << 20):
            for samples in (200, 8):
                w[f"(c) one n = {n} graph (d = 7), {samples + 2} candidates"] = stages_of_the_search(n, samples, 100, 20)
    if "d" in parts:
        rec["(d) quality, one n = 20000 graph through train_model"] = quality_20000()
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
