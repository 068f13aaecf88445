"""Timing of the batch build from edge-index tensors (profiles/r22_batch_build.json).

    python scratch/batch_build_timing.py OUT.json

One MI355X, one process, the variants alternating round by round, wall-clock time of the whole call with a device
synchronisation after it (every variant ends with the batch usable on the device):

  device      GraphBatch.from_edge_index(edge_index, ptr) from tensors already on the device
  handles     GraphBatch(handles) from ready GraphHandles (BatchArrays in numpy, gmc_ell_arrange_host, the copies)
  networkx    [from_networkx(g) for g in graphs] + GraphBatch(handles) - only up to the size at which it stays under a minute

Workloads: 50 graphs of 50..500 nodes, 160 x (n = 1000, d = 7), one graph of 20,000 nodes, one of 2^20 nodes, all 7-regular
circulants (offsets 1, 2, 3 and n / 2) generated as edge tensors.  For the device variant the two stages are also timed
with device events around the library calls on buffers allocated once (gmc_batch_build_csr, gmc_batch_build_table - without
overflow lists the table stage is the arrange kernel alone), and the one read of the report by the wall clock."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gcn_max_cut_amd as pkg  # noqa: E402

ROUNDS = 5
NETWORKX_MAX_NODES = 200_000   # beyond this the networkx route is not attempted (building the networkx object alone is Python loops over millions of edges)


def circulant(n):
    """(src, dst) of the 7-regular circulant on n nodes (n even, n >= 8), both directions of every edge."""
    i = np.arange(n, dtype=np.int64)
    nbrs = [(i + o) % n for o in (1, 2, 3, n - 1, n - 2, n - 3, n // 2)]
    return np.tile(i, 7), np.concatenate(nbrs)


def workload(sizes):
    src, dst, ptr = [], [], [0]
    for n in sizes:
        s, d = circulant(n)
        src.append(s + ptr[-1]); dst.append(d + ptr[-1]); ptr.append(ptr[-1] + n)
    return np.stack([np.concatenate(src), np.concatenate(dst)]), np.asarray(ptr, np.int64)


def handles_of(sizes):
    out = []
    for n in sizes:
        s, d = circulant(n)
        out.append(pkg.from_edge_index(np.stack([s, d]), n))
    return out


def networkx_of(sizes):
    import networkx as nx
    out = []
    for n in sizes:
        s, d = circulant(n)
        g = nx.Graph()
        g.add_nodes_from(range(n))
        g.add_edges_from(zip(s.tolist(), d.tolist()))
        out.append(g)
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stages(ei, ptr, built):
    """Device-event times of the two library calls and the wall time of the report's read, on buffers allocated once."""
    hip, lib = pkg.hip, pkg.hip.load()
    dev, p = ei.device, pkg.hip.ptr
    B, R, E = len(ptr) - 1, int(ptr[-1]), ei.shape[1]
    src, dst = ei[0].to(torch.int32).contiguous(), ei[1].to(torch.int32).contiguous()
    goff = torch.from_numpy(ptr.astype(np.int32)).to(dev)
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    rowptr, lcol, gcol, dinv = new(R + 1, torch.int32), new(E, torch.int32), new(E, torch.int32), new(R, torch.float32)
    report = new(hip.BB_REPORT_WORDS, torch.int32)
    ws = new(int(lib.gmc_batch_build_workspace_bytes(B, R, E)), torch.uint8)
    W, NS = built.c.ell_width, built.c.ell_slots
    ell = new((R, W), torch.int16) if W else None
    out = {"csr_ms": [], "report_read_ms": [], "table_ms": []}
    for _ in range(ROUNDS + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        hip.check(lib.gmc_batch_build_csr(B, R, E, p(goff), p(src), p(dst), None, p(rowptr), p(lcol), p(gcol), None, p(dinv),
                                          p(report), p(ws), ws.numel(), hip.stream()), "csr")
        ev[1].record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        report.cpu()
        out["report_read_ms"].append((time.perf_counter() - t0) * 1e3)
        if W:
            ev[2].record()
            hip.check(lib.gmc_batch_build_table(B, R, built.n_max, p(goff), p(rowptr), p(lcol), None, W, NS, p(ell), None, None,
                                                None, None, 0, p(ws), ws.numel(), hip.stream()), "table")
            ev[3].record()
        torch.cuda.synchronize()
        out["csr_ms"].append(ev[0].elapsed_time(ev[1]))
        if W:
            out["table_ms"].append(ev[2].elapsed_time(ev[3]))
    return {k: (statistics.median(v[1:]) if v else None) for k, v in out.items()}   # (the first round warms up)


def main(out_path):
    pkg.hip.require_gpu()
    dev = torch.device("cuda", 0)
    loads = {"50 graphs, n = 50..500": [int(n) // 2 * 2 for n in np.linspace(50, 500, 50)],
             "160 x (n = 1000, d = 7)": [1000] * 160,
             "one graph, n = 20,000": [20000],
             "one graph, n = 2^20": [1 << 20]}
    result = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "networkx_not_timed_beyond_nodes": NETWORKX_MAX_NODES,
              "workloads": {}}
    for name, sizes in loads.items():
        ei_host, ptr = workload(sizes)
        ei = torch.from_numpy(ei_host).to(dev)
        handles = handles_of(sizes)
        graphs = networkx_of(sizes) if sum(sizes) <= NETWORKX_MAX_NODES else None
        variants = {"device": lambda: pkg.GraphBatch.from_edge_index(ei, ptr),
                    "handles": lambda: pkg.GraphBatch(handles, None, dev)}
        if graphs is not None:
            variants["networkx"] = lambda: pkg.GraphBatch([pkg.from_networkx(g) for g in graphs], None, dev)
        built = variants["device"]()   # warm-up, and the facts of the batch
        variants["handles"]()
        times = {k: [] for k in variants}
        for _ in range(ROUNDS):
            for k, fn in variants.items():
                times[k].append(wall(fn))
        row = {"graphs": len(sizes), "rows": int(ptr[-1]), "entries": int(ei.shape[1]), "ell_width": built.c.ell_width,
               "ell_slots": built.c.ell_slots,
               "wall_ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()},
               "device_stages": stages(ei, ptr, built)}
        st = row["device_stages"]
        if st["table_ms"] is not None:
            row["arrange_share_of_device_time"] = st["table_ms"] / (st["csr_ms"] + st["table_ms"])
        result["workloads"][name] = row
        print(name, json.dumps(row), flush=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
