"""What the run-time `first` costs, and what plain max-cut gives, on the MI355X: profiles/r23_plain_maxcut.json.

    python scratch/plain_maxcut_timing.py OUT.json --parent DIR [--windows 4] [--skip-bench] [--skip-solve]
    python scratch/plain_maxcut_timing.py --window          (one window of this tree: a JSON line on stdout)
    python scratch/plain_maxcut_timing.py OUT.json --parent DIR --round-only [--windows 4]

(a) Four existing entry points on 160 x (n = 1000, d = 7), K = 3 - gmc_kway_refine_anneal_f32 (201 candidates, 100
    sweeps), gmc_kway_decode_sample_seeded_f32 (200 samples), gmc_round_conditional_f32 and one gmc_inst_train_fwd_bwd
    step (hidden 500) - timed in WINDOWS of one fresh process each, this tree and the parent commit's tree (DIR: a
    checkout of it with its library built) alternating: per entry point and window the median over ROUNDS loops of the
    time per call of a loop of many calls (5 of the annealing, 300 of the sampler and of the rounding, 200 of the step)
    between two device events.  The parent's own min-max range over its windows is the noise estimate; `within` says
    whether this tree's median of window medians lies inside it.
(b) `python bench.py` on both trees, two runs each, in the order this, parent, parent, this: the result lines.
(c) For information, ONE seed: maxcut.solve wall time on the same 160 graphs at K = 2 and 3 (hidden 64, 200 epochs,
    lr 1e-2) split into batch build, training and search, and the mean cut / trained_cut / rounded_cut on the held-out
    7-regular graphs of DESIGN.md section 10 (10 per size, n = 500 and 1000) with and without terminals.
(d) --round-only: where the rounding call's time goes, both trees alternating: per window the median over 200 calls of
    the kernel's own time (the library's probe: HIP events around the launch) and of the host's time to enqueue the call
    (host clock around the Python call, no synchronise); added to OUT.json under "round_split"."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIDDEN, K, ROUNDS = 500, 3, 5


def timed(fn, calls):
    """ms per call: the median over ROUNDS loops of `calls` calls, each loop between two device events."""
    import torch
    for _ in range(min(calls, 10)):
        fn()
    out = []
    for _ in range(ROUNDS):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_time(stop) / calls)
    return float(np.median(out))


def window():
    """Medians (ms) of the four calls in the tree this file's process runs in (the current directory)."""
    sys.path.insert(0, os.getcwd())
    import torch
    import gcn_max_cut_amd as pkg
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    from oracle import ref_dense as R
    pkg.hip.require_gpu()
    handles = [pkg.from_networkx(R.regular_graph(1000, 7, 100 + i)) for i in range(160)]
    eng = pkg.engine.InstanceEngine(handles, HIDDEN, K)
    torch.manual_seed(0)
    eng.reset_parameters()
    batch = eng.batch
    P, S, _ = eng.forward(1.0)
    rnd = TN._round_on_gpu(batch, P, 0)[0]
    samples = TN._kway_sample_on_gpu(batch, P, 199, 1, range(batch.B), True)[3]
    cands = torch.cat([S.to(torch.int8).reshape(1, -1), rnd.reshape(1, -1), samples]).contiguous()
    assert cands.shape[0] == 201
    inv_temp = TN.anneal_schedule(100)
    rec = {
        "anneal_201x100": timed(lambda: TN._kway_anneal_on_gpu(batch, K, cands.clone(), inv_temp, 0, 100), 5),
        "sample_200": timed(lambda: TN._kway_sample_on_gpu(batch, P, 200, 1, range(batch.B), False), 300),
        "round_descent100": timed(lambda: TN._round_on_gpu(batch, P, 100), 300),
        "inst_train_fwd_bwd": timed(lambda: eng.train_fwd_bwd(1.0), 200),
    }
    print("WINDOW " + json.dumps(rec), flush=True)


def round_window():
    """Kernel time (probe) and host enqueue time of _round_on_gpu(descent 100) in the current directory's tree."""
    sys.path.insert(0, os.getcwd())
    import torch
    import gcn_max_cut_amd as pkg
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    from oracle import ref_dense as R
    pkg.hip.require_gpu()
    handles = [pkg.from_networkx(R.regular_graph(1000, 7, 100 + i)) for i in range(160)]
    eng = pkg.engine.InstanceEngine(handles, HIDDEN, K)
    torch.manual_seed(0)
    eng.reset_parameters()
    batch = eng.batch
    P = eng.forward(1.0)[0]
    for _ in range(20):
        TN._round_on_gpu(batch, P, 100)
    torch.cuda.synchronize()
    host = []
    for _ in range(200):
        t0 = time.perf_counter()
        TN._round_on_gpu(batch, P, 100)
        host.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
    with pkg.hip.Probe(256) as probe:
        for _ in range(200):
            TN._round_on_gpu(batch, P, 100)
        torch.cuda.synchronize()
    kernel = [ms for tag, ms in probe.records if tag == "refine"]
    assert len(kernel) == 200, len(kernel)
    print("WINDOW " + json.dumps({"kernel_ms": float(np.median(kernel)), "host_enqueue_ms": float(np.median(host))}), flush=True)


def run_window(tree, mode="--window"):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), mode], cwd=tree, capture_output=True, text=True,
                         timeout=600, env={**os.environ, "PYTHONPATH": tree})
    if out.returncode != 0:
        raise SystemExit(f"window in {tree} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    line = [l for l in out.stdout.splitlines() if l.startswith("WINDOW ")][-1]
    return json.loads(line[len("WINDOW "):])


def run_bench(tree):
    out = subprocess.run([sys.executable, "bench.py"], cwd=tree, capture_output=True, text=True, timeout=900,
                         env={**os.environ, "PYTHONPATH": tree})
    if out.returncode != 0:
        raise SystemExit(f"bench.py in {tree} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def solve_info():
    sys.path.insert(0, ROOT)
    import torch
    import gcn_max_cut_amd as pkg
    from gcn_max_cut_amd import maxcut
    from oracle import ref_dense as R

    def tensors(specs):
        handles = [pkg.from_networkx(R.regular_graph(n, d, s)) for n, d, s in specs]
        rows, cols, off, ptr = [], [], 0, [0]
        for h in handles:
            rows.append(np.repeat(np.arange(h.n), np.diff(h.rowptr)) + off)
            cols.append(h.col.astype(np.int64) + off)
            off += h.n
            ptr.append(off)
        return torch.from_numpy(np.stack([np.concatenate(rows), np.concatenate(cols)])).cuda(), np.asarray(ptr, np.int64)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    rec = {"note": "one seed (0); for information only", "hidden_dim": 64, "epochs": 200, "learning_rate": 1e-2}
    kw = dict(hidden_dim=64, epochs=200, learning_rate=1e-2, seed=0)
    ei, ptr = tensors([(1000, 7, 100 + i) for i in range(160)])
    maxcut.solve(ei, ptr, number_classes=2, **{**kw, "epochs": 2})          # warm-up: code objects, allocator
    for Kc in (2, 3):
        _, whole = clock(lambda: maxcut.solve(ei, ptr, number_classes=Kc, **kw))
        batch, build = clock(lambda: pkg.GraphBatch.from_edge_index(ei, ptr))
        _, trained = clock(lambda: maxcut.solve_batch(batch, number_classes=Kc, samples=0, anneal_sweeps=0,
                                                      max_descent_sweeps=0, **kw))
        res, full = clock(lambda: maxcut.solve_batch(batch, number_classes=Kc, **kw))
        rec[f"solve_160x1000_K{Kc}"] = dict(
            wall_s=whole, build_s=build, training_and_scoring_s=trained, search_s=full - trained,
            mean_cut=float(res.cut.mean()), mean_trained_cut=float(res.trained_cut.mean()),
            mean_rounded_cut=float(res.rounded_cut.mean()))
        print(Kc, rec[f"solve_160x1000_K{Kc}"], flush=True)
    for n in (500, 1000):
        ei, ptr = tensors([(n, 7, 5000 + 10 * n + i) for i in range(10)])
        for Kc in (2, 3):
            for terminals in (False, True):
                r = maxcut.solve(ei, ptr, number_classes=Kc, terminals=terminals, **kw)
                key = f"held_out_n{n}_K{Kc}_{'terminals' if terminals else 'plain'}"
                rec[key] = dict(edges=n * 7 // 2, mean_cut=float(r.cut.mean()), mean_trained_cut=float(r.trained_cut.mean()),
                                mean_rounded_cut=float(r.rounded_cut.mean()))
                print(key, rec[key], flush=True)
    return rec


def main():
    if "--window" in sys.argv:
        return window()
    if "--round-window" in sys.argv:
        return round_window()
    out_path = sys.argv[1]
    parent = os.path.abspath(sys.argv[sys.argv.index("--parent") + 1])
    windows = int(sys.argv[sys.argv.index("--windows") + 1]) if "--windows" in sys.argv else 4
    if "--round-only" in sys.argv:
        rec = json.load(open(out_path)) if os.path.exists(out_path) else {}
        split = rec["round_split"] = {"this": [], "parent": []}
        for i in range(windows):
            for name, tree in (("parent", parent), ("this", ROOT)) if i % 2 == 0 else (("this", ROOT), ("parent", parent)):
                split[name].append(run_window(tree, "--round-window"))
                print(name, split[name][-1], flush=True)
        with open(out_path, "w") as f:
            json.dump(rec, f, indent=1)
        return
    rec = {"workload": "160 x (n = 1000, d = 7), K = 3, hidden 500", "loops_per_window": ROUNDS, "windows": {"this": [], "parent": []}}

    def save():
        with open(out_path, "w") as f:
            json.dump(rec, f, indent=1)

    for i in range(windows):
        for name, tree in (("parent", parent), ("this", ROOT)) if i % 2 == 0 else (("this", ROOT), ("parent", parent)):
            rec["windows"][name].append(run_window(tree))
            print(name, rec["windows"][name][-1], flush=True)
            save()
    rec["summary"] = {}
    for key in rec["windows"]["this"][0]:
        mine = [w[key] for w in rec["windows"]["this"]]
        theirs = [w[key] for w in rec["windows"]["parent"]]
        rec["summary"][key] = dict(this_median_ms=float(np.median(mine)), this_range_ms=[min(mine), max(mine)],
                                   parent_median_ms=float(np.median(theirs)), parent_range_ms=[min(theirs), max(theirs)],
                                   within=bool(min(theirs) <= float(np.median(mine)) <= max(theirs)))
        print(key, rec["summary"][key], flush=True)
    save()
    if "--skip-bench" not in sys.argv:
        rec["bench"] = {"this": [], "parent": []}
        rec["bench_order"] = ["this", "parent", "parent", "this"]
        for pair in ((("this", ROOT), ("parent", parent)), (("parent", parent), ("this", ROOT))):
            for name, tree in pair:
                rec["bench"][name].append(run_bench(tree))
                print("bench", name, rec["bench"][name][-1], flush=True)
                save()
    if "--skip-solve" not in sys.argv:
        rec["solve"] = solve_info()
    save()


if __name__ == "__main__":
    main()
