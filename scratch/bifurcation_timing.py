"""What a step of the discrete simulated bifurcation (gmc_dense_sb_f32) costs, and whether the stage pays at equal time.

    python scratch/bifurcation_timing.py OUT.json [steps|equal]

1. `steps`.  n = 256 / 1024 / 2048 / 4096, cands = 16 / 64 / 200, B = 1 / 16, +-1 weights drawn on the device: the time
   per step of a call of STEPS steps (device events around the whole call, a warm-up, then ROUNDS rounds alternating the
   tile the call chooses and the three forced tiles 64 x 64, 32 x 64, 64 x 16), the achieved TFLOP/s at 2 B n^2 cands flops
   per step, set against the 157 TF fp32 matrix peak and the launch floor.
2. `equal`.  Instances: Sherrington-Kirkpatrick J ~ N(0, 1 / n) at n = 1024; G(1024, 0.5) with +-1 weights; the complete
   +-1 graph at n = 2048; the QUBO family G(800, 0.06) (couplings +-1, +-2, linear terms in -3..3, as
   scratch/chain_cost_timing.py draws them, here as a matrix).  Per instance seed 0, 1, 2 and three arms, alternating in one
   process: (A) the door's default call, 100 sweeps; (B) bifurcation_steps = S plus a shortened annealing, S and the sweeps
   chosen from a measured step and a measured sweep so that each half takes half of (A)'s time; (C) the annealing alone
   with the sweeps that fill (B)'s measured time.  Wall time of the whole door call (host work included, the same in every
   arm), and the objective: energy per spin, cut or energy.
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gcn_max_cut_amd import hip, maxcut  # noqa: E402
from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN  # noqa: E402
from tests import dense_ref as DR  # noqa: E402

ROUNDS, PEAK_TF = 3, 157.0
TILES = {0: "chosen", 1: "64x64", 2: "32x64", 3: "64x16"}


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


def timed(launch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    launch()
    b.record()
    torch.cuda.synchronize()
    return float(a.elapsed_time(b))


def step_cost(B, n, cands, steps):
    lib, p = hip.load(), hip.ptr
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n + cands)
    half = torch.randint(0, 2, (B, n, n), generator=gen, device="cuda", dtype=torch.int8).to(torch.float32) * 2 - 1
    W = torch.triu(half, 1)
    W = (W + W.transpose(1, 2)).contiguous()
    del half
    x = torch.empty((B * n, cands), device="cuda")
    y = torch.empty((B * n, cands), device="cuda")
    pump = torch.from_numpy(TN.bifurcation_pump(steps)).cuda()
    assign = torch.empty((cands, B * n), dtype=torch.int8, device="cuda")
    need = int(lib.gmc_dense_sb_workspace_bytes(B, n, cands))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    c0 = 0.5 / TN.dense_scale(W[:1])

    def call(k):
        hip.check(lib.gmc_dense_sb_init_f32(B, n, cands, 1, 0.1, p(x), p(y), hip.stream()), "init")
        return timed(lambda: hip.check(lib.gmc_dense_sb_f32(B, n, p(W), n, None, cands, p(x), p(y), p(pump), k, c0, 1.25,
                                                            p(ws), need, p(assign), hip.stream()), "sb"))
    rec = dict(B=B, n=n, cands=cands, steps=steps, flops_per_step=2.0 * B * n * n * cands, tiles={})
    ms = {t: [] for t in TILES}
    for t in TILES:
        lib.gmc_debug_set_sb_tile(t)
        call(steps)
    for _ in range(ROUNDS):
        for t in TILES:
            lib.gmc_debug_set_sb_tile(t)
            ms[t].append(call(steps))
    lib.gmc_debug_set_sb_tile(0)
    rec["empty_call_ms"] = median([call(0) for _ in range(ROUNDS)])
    for t, name in TILES.items():
        per = [m / steps * 1e3 for m in ms[t]]
        us = median(per)
        rec["tiles"][name] = dict(us_per_step_median=us, us_per_step_min=min(per), us_per_step_max=max(per),
                                  tflops=rec["flops_per_step"] / (us * 1e-6) / 1e12,
                                  fraction_of_peak=rec["flops_per_step"] / (us * 1e-6) / 1e12 / PEAK_TF)
    best = min((v["us_per_step_median"], k) for k, v in rec["tiles"].items() if k != "chosen")
    rec["fastest_forced_tile"] = best[1]
    print(json.dumps(rec), flush=True)
    return rec


def steps_part(result, save):
    result["step_cost"] = []
    for B in (1, 16):
        for n in (256, 1024, 2048, 4096):
            for cands in (16, 64, 200):
                flops = 2.0 * B * n * n * cands
                steps = 200 if flops < 2e9 else (50 if flops < 3e10 else 20)
                result["step_cost"].append(step_cost(B, n, cands, steps))
                save()


# ---- equal time ----------------------------------------------------------------------------------------------------------
def instance(kind, seed):
    if kind == "sk1024":
        n = 1024
        g = np.random.RandomState(seed).normal(0.0, 1.0 / np.sqrt(n), (n, n))
        J = np.triu(g, 1)
        return "ising", (J + J.T).astype(np.float32), None
    if kind == "g1024_half_pm1":
        return "maxcut", DR.weights_of("pm1", 1024, 50 + seed, 0.5), None
    if kind == "k2048_pm1":
        return "maxcut", DR.weights_of("pm1", 2048, 60 + seed), None
    assert kind == "qubo800"
    Q = DR.symmetric(800, lambda r, m: r.choice([-2.0, -1.0, 1.0, 2.0], size=m), 0.06, 70 + seed)
    return "qubo", Q, np.random.RandomState(80 + seed).randint(-3, 4, 800).astype(np.float64)


def door(kind, M, lin, seed, **kw):
    """(objective to report, wall seconds) of one call of the instance's door."""
    torch.cuda.synchronize()
    t = time.perf_counter()
    if kind == "ising":
        res = maxcut.solve_ising_dense(M, lin, seed=seed, **kw)
        value = float(res.energy[0]) / M.shape[-1]          # energy per spin
    elif kind == "qubo":
        res = maxcut.solve_qubo_dense(M, lin, seed=seed, **kw)
        value = float(res.energy[0])
    else:
        res = maxcut.solve_dense(M, seed=seed, **kw)
        value = float(res.cut[0])
    torch.cuda.synchronize()
    return value, time.perf_counter() - t


def equal_part(result, save):
    result["equal_time"] = []
    for name in ("sk1024", "g1024_half_pm1", "k2048_pm1", "qubo800"):
        rows = []
        for seed in (0, 1, 2):
            kind, M, lin = instance(name, seed)
            Md = torch.from_numpy(M).cuda()
            door(kind, Md, lin, seed, anneal_sweeps=2, bifurcation_steps=2)          # warm-up of every kernel
            _, t0 = door(kind, Md, lin, seed, anneal_sweeps=0)
            _, t100 = door(kind, Md, lin, seed)
            _, tsb = door(kind, Md, lin, seed, anneal_sweeps=0, bifurcation_steps=1000)
            per_sweep, per_step = (t100 - t0) / 100, (tsb - t0) / 1000
            S = max(int(0.5 * (t100 - t0) / per_step), 1)
            sweeps_b = max(int(0.5 * (t100 - t0) / per_sweep), 1)
            row = dict(seed=seed, seconds_without_sweeps=t0, seconds_per_sweep=per_sweep, seconds_per_step=per_step,
                       bifurcation_steps=S, sweeps_b=sweeps_b, A=[], B=[], C=[], B_only=[])
            _, tb = door(kind, Md, lin, seed, anneal_sweeps=sweeps_b, bifurcation_steps=S)
            sweeps_c = max(int(round((tb - t0) / per_sweep)), 1)
            row["sweeps_c"] = sweeps_c
            for _ in range(2):                                                         # the arms alternate
                row["A"].append(door(kind, Md, lin, seed))
                row["B"].append(door(kind, Md, lin, seed, anneal_sweeps=sweeps_b, bifurcation_steps=S))
                row["C"].append(door(kind, Md, lin, seed, anneal_sweeps=sweeps_c))
            row["B_only"].append(door(kind, Md, lin, seed, anneal_sweeps=0, bifurcation_steps=2 * S))
            rows.append(row)
            print(name, json.dumps(row), flush=True)
        rec = dict(instance=name, rows=rows)
        for arm in ("A", "B", "C", "B_only"):
            vals = [r[arm][0][0] for r in rows]                                        # reproducible: the first repeat
            secs = [s for r in rows for _, s in r[arm]]
            rec[arm] = dict(mean=float(np.mean(vals)), min=min(vals), max=max(vals), seconds_mean=float(np.mean(secs)),
                            seconds_min=min(secs), seconds_max=max(secs))
        result["equal_time"].append(rec)
        print(json.dumps({k: rec[k] for k in ("instance", "A", "B", "C", "B_only")}), flush=True)
        save()


def main():
    out_path = sys.argv[1]
    part = sys.argv[2] if len(sys.argv) > 2 else "all"
    hip.require_gpu()
    result = dict(device=torch.cuda.get_device_name(0), rounds=ROUNDS, peak_tflops=PEAK_TF, parisi=-0.7632)
    if os.path.exists(out_path):
        result.update(json.load(open(out_path)))
    save = lambda: json.dump(result, open(out_path, "w"), indent=1)  # noqa: E731
    if part in ("steps", "all"):
        steps_part(result, save)
    if part in ("equal", "all"):
        equal_part(result, save)
    save()


if __name__ == "__main__":
    main()
