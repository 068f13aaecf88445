"""Seeded post-processing sampler (gmc_decode_sample_seeded_f32) against the numpy-stream one (gmc_decode_sample_f32):
kernel time, wall time of decode_dataset, cut quality, and one 20,000-sample call without the sample array.  Model and
datasets are those of scratch/refine_timing.py; 200 samples.

    python scratch/seeded_sampler_timing.py OUT.json        (profiles/r10_seeded_sampler.json; one MI355X)

Workloads: (a) 50 graphs, n in {50, 100, 200, 300, 500} (BASELINE configs[4]), d = 7;  (b) 160 graphs n = 1000 d = 7.
1. Kernel time of both samplers in this process from the library's event probe: 18 probed calls each after a warm-up,
   the two variants alternating, in 3 windows of 6; medians, minima, and the spread of the window medians.
2. Wall time of decode_dataset(model, ds, 200) from call to returned list (torch.cuda.synchronize() inside the timed
   region) with and without sample_seed, 11 calls each, alternating; and the numpy path's host work before its kernel
   launch (draws, concatenate, copy to the device), 10 times.
3. Quality on (a): mean best-of-200 cut with the numpy sampler under 5 np.random.seed values and with the seeded
   sampler under 5 seeds, the same model.
4. One seeded call with iters = 20000 and assign_all = NULL on (a): kernel time, wall time of the call (both launches)
   and the bytes of its outputs against the [iters][R] array it does without.
"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_timing as RT  # noqa: E402  (puts the repository root on sys.path)

from gcn_max_cut_amd import hip  # noqa: E402
from gcn_max_cut_amd.graph import GraphBatch  # noqa: E402
from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN  # noqa: E402

ITERS = 200
WINDOWS, PER_WINDOW = 3, 6


def outputs(batch, iters, keep=True):
    dev = batch.device
    return dict(assign_all=torch.empty((iters, batch.R), dtype=torch.int8, device=dev) if keep else None,
                cut_all=torch.empty((batch.B, iters), device=dev),
                best_assign=torch.empty(batch.R, dtype=torch.int32, device=dev),
                best_cut=torch.empty(batch.B, device=dev),
                best_iter=torch.empty(batch.B, dtype=torch.int32, device=dev))


def host_uniforms(batch, iters):
    """The host work of the numpy path before its launch, as TestingNeuralNetwork._sample_on_gpu does it."""
    draws = [np.random.rand(iters, int(n) - 3) for n in batch.sizes]
    uoff = np.zeros(batch.B + 1, np.int64)
    np.cumsum([d.size for d in draws], out=uoff[1:])
    u = torch.from_numpy(np.concatenate([d.ravel() for d in draws])).to(batch.device)
    uo = torch.from_numpy(uoff).to(batch.device)
    return u, uo


def launch_numpy(batch, P, u, uo, o, iters):
    p = hip.ptr
    hip.check(hip.load().gmc_decode_sample_f32(batch.ref(), p(P), p(u), p(uo), iters, p(o["assign_all"]), p(o["cut_all"]),
                                               p(o["best_assign"]), p(o["best_cut"]), p(o["best_iter"]), hip.stream()),
              "gmc_decode_sample_f32")


def launch_seeded(batch, P, gkey, o, iters):
    p = hip.ptr
    hip.check(hip.load().gmc_decode_sample_seeded_f32(batch.ref(), p(P), p(gkey), iters, p(o["assign_all"]),
                                                      p(o["cut_all"]), p(o["best_assign"]), p(o["best_cut"]),
                                                      p(o["best_iter"]), hip.stream()), "gmc_decode_sample_seeded_f32")


def device_keys(batch, seed):
    return torch.from_numpy(TN.sample_keys(seed, range(batch.B)).view(np.int64)).to(batch.device)


def probed(tag, launch):
    with hip.Probe(4) as pr:
        launch()
    (ms,) = [t for name, t in pr.records if name == tag]
    return ms


def summary(ms):
    windows = [float(np.median(ms[w * PER_WINDOW:(w + 1) * PER_WINDOW])) for w in range(WINDOWS)]
    return dict(kernel_ms_median=float(np.median(ms)), kernel_ms_min=float(min(ms)), calls=len(ms),
                window_medians_ms=windows, window_spread_ms=max(windows) - min(windows))


def kernel_times(batch, P):
    np.random.seed(0)
    u, uo = host_uniforms(batch, ITERS)
    gkey = device_keys(batch, 0)
    o = outputs(batch, ITERS)
    launch_numpy(batch, P, u, uo, o, ITERS)                    # warm-up (code object load)
    launch_seeded(batch, P, gkey, o, ITERS)
    torch.cuda.synchronize()
    ms_numpy, ms_seeded, ms_lean = [], [], []
    lean = dict(o, assign_all=None)
    for _ in range(WINDOWS * PER_WINDOW):
        ms_numpy.append(probed("decode", lambda: launch_numpy(batch, P, u, uo, o, ITERS)))
        ms_seeded.append(probed("sample", lambda: launch_seeded(batch, P, gkey, o, ITERS)))
        ms_lean.append(probed("sample", lambda: launch_seeded(batch, P, gkey, lean, ITERS)))
    a, b, c = summary(ms_numpy), summary(ms_seeded), summary(ms_lean)
    return dict(B=batch.B, R=batch.R, iters=ITERS, uniform_bytes=int(u.numel() * 8),
                numpy_stream_sampler=a, seeded_sampler=b, seeded_sampler_without_sample_array=c,
                seeded_minus_numpy_ms=b["kernel_ms_median"] - a["kernel_ms_median"],
                seeded_not_slower_within_numpy_window_spread=bool(
                    b["kernel_ms_median"] <= a["kernel_ms_median"] + a["window_spread_ms"]))


def wall_times(net, ds, batch):
    def timed(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = TN.decode_dataset(net, ds, ITERS, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res
    np.random.seed(0)
    timed()
    timed(sample_seed=0)                                       # warm-up of both paths
    t_numpy, t_seeded = [], []
    for _ in range(11):
        t_numpy.append(timed()[0])
        t_seeded.append(timed(sample_seed=0)[0])
    t_host = []
    for _ in range(10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        u, uo = host_uniforms(batch, ITERS)
        torch.cuda.synchronize()
        t_host.append(time.perf_counter() - t0)
        del u, uo
    med = lambda t: float(np.median(t))
    return dict(calls_each=11, decode_dataset_numpy_stream_s_median=med(t_numpy), decode_dataset_numpy_stream_s_min=min(t_numpy),
                decode_dataset_seeded_s_median=med(t_seeded), decode_dataset_seeded_s_min=min(t_seeded),
                ratio_numpy_stream_to_seeded=med(t_numpy) / med(t_seeded),
                numpy_path_draws_concatenate_copy_s_median=med(t_host), numpy_path_draws_concatenate_copy_s_min=min(t_host))


def quality(net, ds):
    mean_cut = lambda res: float(np.mean([r["post_cut"] for r in res]))
    by_numpy, by_seeded = [], []
    for s in range(5):
        np.random.seed(s)
        by_numpy.append(mean_cut(TN.decode_dataset(net, ds, ITERS)))
        by_seeded.append(mean_cut(TN.decode_dataset(net, ds, ITERS, sample_seed=s)))
    spread = lambda v: float(max(v) - min(v))
    diff = float(np.mean(by_seeded) - np.mean(by_numpy))
    return dict(graphs=len(ds), seeds=list(range(5)), mean_best_of_200_numpy_stream=by_numpy, mean_best_of_200_seeded=by_seeded,
                mean_numpy_stream=float(np.mean(by_numpy)), mean_seeded=float(np.mean(by_seeded)),
                spread_numpy_stream_max_minus_min=spread(by_numpy), spread_seeded_max_minus_min=spread(by_seeded),
                std_numpy_stream=float(np.std(by_numpy, ddof=1)), std_seeded=float(np.std(by_seeded, ddof=1)),
                seeded_minus_numpy_stream=diff,
                difference_inside_the_larger_spread=bool(abs(diff) <= max(spread(by_numpy), spread(by_seeded))))


def many_samples(batch, P, iters=20000):
    gkey = device_keys(batch, 0)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    o = outputs(batch, iters, keep=False)
    allocated = torch.cuda.memory_allocated() - before
    launch_seeded(batch, P, gkey, o, iters)                    # warm-up
    torch.cuda.synchronize()
    ms, wall = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        ms.append(probed("sample", lambda: launch_seeded(batch, P, gkey, o, iters)))
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    return dict(iters=iters, B=batch.B, R=batch.R, kernel_ms_median=float(np.median(ms)), kernel_ms_min=float(min(ms)),
                call_wall_ms_median_both_launches=float(np.median(wall)) * 1e3,
                output_bytes=int(sum(t.numel() * t.element_size() for t in o.values() if t is not None)),
                torch_allocated_bytes=int(allocated), sample_array_bytes_not_allocated=int(iters) * int(batch.R),
                mean_best_cut=float(o["best_cut"].mean().item()))


def main():
    out_path = sys.argv[1]
    hip.require_gpu()
    with tempfile.TemporaryDirectory() as workdir:
        net, train_info = RT.train(workdir)
    net.eval()
    eng = net.engine()
    rec = {"train": train_info}
    for name, specs in (("a_configs4_50_graphs", RT.CONFIG_A), ("b_160_graphs_n1000_d7", RT.CONFIG_B)):
        ds = RT.dataset(specs)
        items = list(ds.values())
        batch = GraphBatch([it[0] for it in items], [it[0].edge_values(it[1]) for it in items], eng.device)
        P, _S, _loss = eng.forward(batch, 1.0, want_loss=True)
        P = P.contiguous().clone()
        rec[name] = dict(kernel=kernel_times(batch, P), wall=wall_times(net, ds, batch))
        print(name, rec[name], flush=True)
        if name.startswith("a_"):
            rec["quality_a"] = quality(net, ds)
            print("quality_a", rec["quality_a"], flush=True)
            rec["a_20000_samples_without_sample_array"] = many_samples(batch, P)
            print("many", rec["a_20000_samples_without_sample_array"], flush=True)
    rec["device"] = torch.cuda.get_device_name(0)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
