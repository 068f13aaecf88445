"""Dense-feature path (net(g, embed.weight)): the three forms of the fp32 MFMA GEMM (gmc_gemm_f32) next to torch.matmul
- rocBLAS, what the layer-1 product ran on before - on the same operands in the same process, and one forward + backward.

    python scratch/dense_features_timing.py OUT.json              wall time of net(g, embed.weight) forward + backward at
                                                                  n = 1000, hidden 500, split by kernel tag (event probe),
                                                                  and event-probe times of the GEMM forms (cross-check)
    python scratch/dense_features_timing.py --profile PHASES.json only the timed GEMM launches, REPS of each, for
                                                                  `rocprofv3 --kernel-trace --stats --output-format csv -- python ...`
    python scratch/dense_features_timing.py --summarize TRACE.csv PHASES.json OUT.json
                                                                  kernel time and TF/s per phase from the kernel trace

--profile runs, per shape and form, REPS launches of the library's GEMM and then REPS torch.matmul calls; a 1 x 1 x 1
library GEMM (one workgroup) separates the phases in the trace, so whatever kernels rocBLAS launches for a product are
all counted for it.  Shapes (R, N, F): the workload's (1000, 1000, 500) and (4096, 1000, 4096).
    NN  T0  = X @ W1     [R,N] . [N,F]      TN  dW1 = X^T @ U   [N,R] . [R,F]      NT  dX = U @ W1^T   [R,F] . [F,N]
"""
import csv
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((1000, 1000, 500), (4096, 1000, 4096))
REPS = 10
PEAK_TF = 157.0   # fp32 matrix peak of an MI355X


def operands(R, N, F):
    g = torch.Generator(device="cuda").manual_seed(0)
    mk = lambda *s: torch.rand(s, device="cuda", generator=g) * 2 - 1
    return mk(R, N), mk(N, F), mk(R, F)   # X, W1, U


def forms(R, N, F, X, W1, U):
    """name -> (ta, tb, M, Nc, K, A, B, the torch product, its output)"""
    return {
        "NN": (0, 0, R, F, N, X, W1, lambda out: torch.matmul(X, W1, out=out), torch.empty(R, F, device="cuda")),
        "TN": (1, 0, N, F, R, X, U, lambda out: torch.matmul(X.t(), U, out=out), torch.empty(N, F, device="cuda")),
        "NT": (0, 1, R, N, F, U, W1, lambda out: torch.matmul(U, W1.t(), out=out), torch.empty(R, N, device="cuda")),
    }


def ours(hip, ta, tb, M, Nc, K, A, B, C):
    hip.check(hip.load().gmc_gemm_f32(ta, tb, M, Nc, K, hip.ptr(A), A.shape[1], hip.ptr(B), B.shape[1], None,
                                      hip.ptr(C), C.shape[1], hip.stream()), "gmc_gemm_f32")


def profile(phases_path):
    from gcn_max_cut_amd import hip
    hip.require_gpu()
    one = torch.zeros(4, device="cuda")
    sink = torch.zeros(1, 4, device="cuda")
    mark = lambda: ours(hip, 0, 0, 1, 1, 1, one.view(1, 4), one.view(1, 4), sink)
    phases, work = [], []
    for R, N, F in SHAPES:
        X, W1, U = operands(R, N, F)
        for name, (ta, tb, M, Nc, K, A, B, product, out) in forms(R, N, F, X, W1, U).items():
            C = torch.empty_like(out)
            ours(hip, ta, tb, M, Nc, K, A, B, C)       # warm-up of both, and they agree
            product(out)
            err = float((C - out).abs().max())
            flops = 2.0 * M * Nc * K
            work.append((dict(shape=[R, N, F], form=name, impl="gmc_gemm_f32", flops=flops, reps=REPS, max_abs_diff=err),
                         lambda a=(ta, tb, M, Nc, K, A, B, C): ours(hip, *a)))
            work.append((dict(shape=[R, N, F], form=name, impl="torch.matmul", flops=flops, reps=REPS),
                         lambda p=product, o=out: p(o)))
    torch.cuda.synchronize()
    for rec, launch in work:
        mark()
        for _ in range(REPS):
            launch()
        phases.append(rec)
    mark()
    torch.cuda.synchronize()
    with open(phases_path, "w") as f:
        json.dump(phases, f, indent=1)


def summarize(trace_path, phases_path, out_path):
    rows = sorted(csv.DictReader(open(trace_path)), key=lambda r: int(r["Start_Timestamp"]))
    num = lambda r, *keys: next((int(r[k]) for k in keys if r.get(k)), 1)
    wgs = lambda r: (num(r, "Grid_Size_X", "Grid_Size") // max(1, num(r, "Workgroup_Size_X", "Workgroup_Size"))) * \
                    (num(r, "Grid_Size_Y") // max(1, num(r, "Workgroup_Size_Y")))
    is_mark = lambda r: "gemm_mfma_kernel" in r["Kernel_Name"] and wgs(r) == 1
    marks = [i for i, r in enumerate(rows) if is_mark(r)]
    phases = json.load(open(phases_path))
    assert len(marks) == len(phases) + 1, (len(marks), len(phases))
    out = []
    for rec, lo, hi in zip(phases, marks[:-1], marks[1:]):
        mine = rows[lo + 1:hi]
        us = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in mine) / 1e3 / rec["reps"]
        per = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in mine]
        tf = rec["flops"] / (us * 1e-6) / 1e12
        out.append(dict(rec, kernel_us_per_product=us, kernels_per_product=len(mine) / rec["reps"],
                        single_kernel_us_min=min(per), single_kernel_us_max=max(per), tflops=tf,
                        share_of_157_tf_fp32_peak=tf / PEAK_TF,
                        kernel_names=sorted({r["Kernel_Name"][:80] for r in mine})))
    for a, b in zip(out[0::2], out[1::2]):
        a["time_ratio_to_torch_matmul"] = a["kernel_us_per_product"] / b["kernel_us_per_product"]
    json.dump(dict(source="rocprofv3 --kernel-trace --stats", gemm=out), open(out_path, "w"), indent=1)
    for r in out:
        print(r["shape"], r["form"], r["impl"], f"{r['kernel_us_per_product']:.1f} us", f"{r['tflops']:.1f} TF",
              r.get("time_ratio_to_torch_matmul", ""))


def step(out_path):
    """net(g, embed.weight) forward + backward at n = 1000, hidden 500: wall time and the kernels by tag."""
    from gcn_max_cut_amd import hip
    from gcn_max_cut_amd.DataGenerator import graphExtender as GE
    from gcn_max_cut_amd.Training import TrainingNeural as T
    import networkx as nx
    hip.require_gpu()
    g_nx = nx.random_regular_graph(7, 1000, seed=1)
    nx.set_edge_attributes(g_nx, 1, "weight")
    (g, _a_pad, _nx, _t), = GE.process_graphs_from_folder({0: g_nx}, {0: [10, 20, 30]}, 1000).values()
    torch.manual_seed(0)
    net, embed, _opt = T.setup_model_and_optimizer(T.TrainingConfig(n_nodes=1000, hidden_dim=500))
    G = torch.randn(1000, 3, device="cuda")

    def one():
        net.zero_grad(); embed.zero_grad()
        (net(g, embed.weight) * G).sum().backward()

    for _ in range(5):
        one()
    torch.cuda.synchronize()
    walls = []
    for _ in range(20):
        t0 = time.perf_counter()
        one()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    by_tag, runs = {}, 10
    for _ in range(runs):
        with hip.Probe(64) as p:
            one()
        for tag, ms in p.records:
            by_tag.setdefault(tag, []).append(ms)
    launches = {t: len(v) // runs for t, v in by_tag.items()}
    kernel_ms = {t: float(np.sum(v)) / runs for t, v in by_tag.items()}
    rec = dict(n=1000, hidden=500, N=1000, wall_ms_median=float(np.median(walls)), wall_ms_min=float(min(walls)),
               launches_by_tag=launches, event_probe_ms_by_tag=kernel_ms, event_probe_ms_total=float(sum(kernel_ms.values())))
    # cross-check of the trace figures with the library's event probe (hipEvents around each launch: includes launch gaps)
    probe = []
    for R, N, F in SHAPES:
        X, W1, U = operands(R, N, F)
        for name, (ta, tb, M, Nc, K, A, B, _product, out) in forms(R, N, F, X, W1, U).items():
            ours(hip, ta, tb, M, Nc, K, A, B, out)
            ms = []
            for _ in range(REPS):
                with hip.Probe(4) as p:
                    ours(hip, ta, tb, M, Nc, K, A, B, out)
                ms += [t for tag, t in p.records if tag == "gemm"]
            probe.append(dict(shape=[R, N, F], form=name, event_probe_us_median=float(np.median(ms)) * 1e3))
    rec = dict(forward_backward=rec, gemm_event_probe=probe, device=torch.cuda.get_device_name(0))
    print(json.dumps(rec, indent=1))
    json.dump(rec, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "--profile":
        profile(sys.argv[2])
    elif sys.argv[1] == "--summarize":
        summarize(*sys.argv[2:5])
    else:
        step(sys.argv[1])
