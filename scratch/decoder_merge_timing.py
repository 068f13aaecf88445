"""The one-workgroup decoders of this tree against another build of the library (the parent commit's), after the
3-class sampler and annealing became the K = 3 instantiations of the K-class kernels and the descent one loop.

    python scratch/decoder_merge_timing.py run OTHER_LIB.so OUT.json      the whole measurement
    python scratch/decoder_merge_timing.py window OUT.json                one window of the library GCN_MAXCUT_LIB names

Workload: 160 graphs n = 1000 d = 7 (unit weights), the one of profiles/r12_kway_search.json.  Calls, each timed by the
library's event probe (device events around the tagged launch; the pick launches are not tagged):
  sample_seeded      gmc_decode_sample_seeded_f32, 200 samples of softmax rows, assign_all written
  anneal             gmc_refine_anneal_f32, 201 uniform random candidates (terminals fixed), 100 sweeps + descent 100
  refine_local       gmc_refine_local_f32 on the same candidates, 100 sweeps at most
  round_K3, round_K8 gmc_round_conditional_f32 on softmax rows, descent 100
  kway_anneal_K4     gmc_kway_refine_anneal_f32 at K = 4, 201 candidates, 100 sweeps + descent 100
A window is one process: it warms every call up once, then times six rounds of all calls.  `run` starts three windows per
library, the two libraries alternating window by window, the other library first, every window under its own time limit;
the first failure ends the run.  A window also records a digest of every call's outputs, and `run` checks that the two
libraries agree on them.  Per call: medians, window medians, the other library's window-to-window spread
(max - min of its window medians) / median, the ratio of the medians, and whether this tree's median stays within
twice that spread of the other's."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CANDS, SAMPLES, SWEEPS, DESCENT, WINDOWS, PER_WINDOW, WINDOW_LIMIT_S = 201, 200, 100, 100, 3, 6, 240


def softmax_rows(R_, K, seed):
    logits = np.random.RandomState(seed).standard_normal((R_, K)) * 2.0
    e = np.exp(logits - logits.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


def window(out_path):
    import torch
    from gcn_max_cut_amd import hip
    from gcn_max_cut_amd.graph import GraphBatch, from_networkx
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    from oracle import ref_dense as R
    hip.require_gpu()
    dev = torch.device("cuda")
    batch = GraphBatch([from_networkx(R.regular_graph(1000, 7, 9000 + i)) for i in range(160)], None, dev)
    p, lib = hip.ptr, hip.load()
    inv_t = torch.from_numpy(TN.anneal_schedule(SWEEPS)).to(dev)
    levels = torch.from_numpy(TN.anneal_levels()).to(dev)
    gkey = torch.from_numpy(TN.sample_keys(0, range(batch.B)).view(np.int64)).to(dev)
    cut_all = torch.empty((batch.B, CANDS), device=dev)
    cut_samples = torch.empty((batch.B, SAMPLES), device=dev)
    cut = torch.empty(batch.B, device=dev)
    best_assign = torch.empty(batch.R, dtype=torch.int32, device=dev)
    best_cut = torch.empty(batch.B, device=dev)
    best_idx = torch.empty(batch.B, dtype=torch.int32, device=dev)
    assign_all = torch.empty((SAMPLES, batch.R), dtype=torch.int8, device=dev)
    rounded = torch.empty(batch.R, dtype=torch.int8, device=dev)
    work = torch.empty((CANDS, batch.R), dtype=torch.int8, device=dev)
    starts = np.asarray(batch.goff_host[:-1], np.int64)
    picks = (best_assign, best_cut, best_idx)

    def candidates(K):
        A = np.random.RandomState(K).randint(0, K, (CANDS, batch.R)).astype(np.int8)
        for j in range(K):
            A[:, starts + j] = j
        return torch.from_numpy(A).to(dev)

    P = {K: torch.from_numpy(softmax_rows(batch.R, K, 100 + K)).to(dev) for K in (3, 8)}
    A = {K: candidates(K) for K in (3, 4)}
    o = {K: batch.refine_order(K) for K in (3, 4, 8)}
    st = hip.stream

    def round_call(K):
        return lambda: lib.gmc_round_conditional_f32(batch.ref(), p(P[K]), K, p(o[K][0]), p(o[K][1]), p(o[K][2]), DESCENT,
                                                     p(rounded), p(cut), None, None, st())

    # name: (probe tag, launch, candidates copied into `work` before the call, outputs)
    calls = {
        "sample_seeded": ("sample", lambda: lib.gmc_decode_sample_seeded_f32(
            batch.ref(), p(P[3]), p(gkey), SAMPLES, p(assign_all), p(cut_samples), p(best_assign), p(best_cut),
            p(best_idx), st()), None, (assign_all, cut_samples) + picks),
        "anneal": ("anneal", lambda: lib.gmc_refine_anneal_f32(
            batch.ref(), p(o[3][0]), p(o[3][1]), p(o[3][2]), CANDS, p(work), p(inv_t), SWEEPS, p(levels), 1, DESCENT,
            p(cut_all), p(best_assign), p(best_cut), p(best_idx), None, None, st()), A[3], (work, cut_all) + picks),
        "refine_local": ("refine", lambda: lib.gmc_refine_local_f32(
            batch.ref(), p(o[3][0]), p(o[3][1]), p(o[3][2]), CANDS, p(work), DESCENT, p(cut_all), p(best_assign),
            p(best_cut), p(best_idx), None, st()), A[3], (work, cut_all) + picks),
        "round_K3": ("refine", round_call(3), None, (rounded, cut)),
        "round_K8": ("refine", round_call(8), None, (rounded, cut)),
        "kway_anneal_K4": ("anneal", lambda: lib.gmc_kway_refine_anneal_f32(
            batch.ref(), 4, p(o[4][0]), p(o[4][1]), p(o[4][2]), CANDS, p(work), p(inv_t), SWEEPS, p(levels), 1, DESCENT,
            p(cut_all), p(best_assign), p(best_cut), p(best_idx), None, None, st()), A[4], (work, cut_all) + picks),
    }

    def timed(name):
        tag, launch, pristine, _outs = calls[name]
        if pristine is not None:
            work.copy_(pristine)
        with hip.Probe(4) as pr:
            hip.check(launch(), name)
        return [t for kernel, t in pr.records if kernel == tag][0]

    digest = {}
    for name in calls:                                   # warm-up (code object load) and the outputs
        timed(name)
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in calls[name][3]:
            h.update(t.cpu().numpy().tobytes())
        digest[name] = h.hexdigest()
    ms = {name: [] for name in calls}
    for _ in range(PER_WINDOW):
        for name in calls:
            ms[name].append(timed(name))
    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump(dict(ms=ms, digest=digest, lib=hip.LIB_PATH, device=torch.cuda.get_device_name(0),
                       staged=int(lib.gmc_refine_anneal_staged(batch.ref()))), f)


def run(other_lib, out_path):
    tmp = out_path + ".windows"
    os.makedirs(tmp, exist_ok=True)
    recs = {"other": [], "this": []}
    for w in range(WINDOWS):
        for which in ("other", "this"):
            env = dict(os.environ)
            env.pop("GCN_MAXCUT_LIB", None)
            if which == "other":
                env["GCN_MAXCUT_LIB"] = os.path.abspath(other_lib)
            path = os.path.join(tmp, f"{which}_{w}.json")
            print(f"window {w} of {which}", flush=True)
            subprocess.run([sys.executable, os.path.abspath(__file__), "window", path], env=env, check=True,
                           timeout=WINDOW_LIMIT_S)   # a failure or an overrun raises: nothing more is started
            recs[which].append(json.load(open(path)))
    out = {"calls": {}}
    for name in recs["this"][0]["ms"]:
        row = {}
        for which in recs:
            all_ms = [t for r in recs[which] for t in r["ms"][name]]
            wm = [float(np.median(r["ms"][name])) for r in recs[which]]
            row[which] = dict(kernel_ms_median=float(np.median(all_ms)), kernel_ms_min=float(min(all_ms)),
                              calls=len(all_ms), window_medians_ms=wm)
        other, this = row["other"], row["this"]
        spread = (max(other["window_medians_ms"]) - min(other["window_medians_ms"])) / other["kernel_ms_median"]
        ratio = this["kernel_ms_median"] / other["kernel_ms_median"]
        digests = {r["digest"][name] for which in recs for r in recs[which]}
        row.update(other_window_spread=spread, this_over_other=ratio, within_twice_the_spread=bool(ratio <= 1 + 2 * spread),
                   outputs_equal_in_every_window=len(digests) == 1)
        out["calls"][name] = row
        print(name, json.dumps(row), flush=True)
    out.update(workload="160 graphs n = 1000 d = 7, unit weights", candidates=CANDS, samples=SAMPLES, anneal_sweeps=SWEEPS,
               max_descent_sweeps=DESCENT, staged=recs["this"][0]["staged"], device=recs["this"][0]["device"],
               other="the parent commit's library (3-class kernels in sample_seeded.hip and anneal.hip)",
               method=(f"hip.Probe (device events around the tagged launch); a window is one process that warms every call "
                       f"up and times {PER_WINDOW} rounds of all calls; {WINDOWS} windows per library, the libraries "
                       f"alternating window by window, the other library first; spread = (max - min of the other "
                       f"library's window medians) / its median; acceptance: this_over_other <= 1 + 2 * spread"))
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "window":
        window(sys.argv[2])
    else:
        run(sys.argv[2], sys.argv[3])
