"""Shared builders for the parity tests: the same seeded graphs go through the product's
GraphExtender (-> GraphHandle + padded adjacency) and through the oracle's."""
import contextlib
import re
import struct
import subprocess

import networkx as nx
import numpy as np
import torch

from oracle import c_oracle as CO
from oracle import ref_dense as R


def make_graphs(specs):
    graphs = {i: R.regular_graph(n, d, s) for i, (n, d, s) in enumerate(specs)}
    terms = {i: R.seeded_terminals(n, s) for i, (n, d, s) in enumerate(specs)}
    return graphs, terms


def product_dataset(specs, max_nodes=1000):
    from gcn_max_cut_amd.DataGenerator import graphExtender as GE
    graphs, terms = make_graphs(specs)
    return GE.process_graphs_from_folder(graphs, terms, max_nodes)


def oracle_dataset(specs, max_nodes=1000):
    graphs, terms = make_graphs(specs)
    return R.make_dataset(graphs, terms, max_nodes)


def csrs_of(dataset):
    return [CO.csr_of(item[2]) for item in dataset.values()]


def np_params(state):
    return {k: v.detach().cpu().numpy().astype(np.float32).copy() for k, v in state.items()}


def weighted_copy(dataset_specs, seed=0):
    """Graphs with non-unit integer weights (exercises the `vals` path)."""
    graphs, terms = make_graphs(dataset_specs)
    rng = np.random.RandomState(seed)
    for g in graphs.values():
        for u, v in g.edges():
            g[u][v]["weight"] = int(rng.randint(1, 4))
    return graphs, terms


def dataset_of(graphs, terms, max_nodes=1000):
    """Product dataset of arbitrary networkx graphs (dict index -> graph / terminal list)."""
    from gcn_max_cut_amd.DataGenerator import graphExtender as GE
    return GE.process_graphs_from_folder(graphs, terms, max_nodes)


def near_regular(n, d, seed, attrs=True):
    """d-regular on n nodes; when n * d is odd, a d-regular graph on n + 1 nodes without its last node.
    `attrs`: unit weight / capacity on every edge, as the reference's generator sets them."""
    d = min(d, n - 1)
    m = n if n * d % 2 == 0 else n + 1
    g = nx.random_regular_graph(d, m, seed=seed)
    if m > n:
        g.remove_node(n)
    out = nx.Graph()
    out.add_nodes_from(range(n))
    out.add_edges_from(g.edges)
    if attrs:
        nx.set_edge_attributes(out, 1, "weight")
        nx.set_edge_attributes(out, 1, "capacity")
    return out


def add_hub(g, hub_degree, seed, hub=5, attrs=True):
    """Raises node `hub` to hub_degree: new neighbours in the order of a seeded permutation of the nodes."""
    rng = np.random.RandomState(seed)
    for v in rng.permutation(g.number_of_nodes()):
        if g.degree(hub) >= hub_degree:
            break
        if int(v) != hub and not g.has_edge(hub, int(v)):
            g.add_edge(hub, int(v), **(dict(weight=1, capacity=1) if attrs else {}))
    assert g.degree(hub) == hub_degree
    return g


def with_hub(n, d, seed, hub_degree, hub=5):
    return add_hub(R.regular_graph(n, d, seed), hub_degree, seed, hub)


def model(hidden, n_nodes=1000, seed=0):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    cfg = T.TrainingConfig(n_nodes=n_nodes, hidden_dim=hidden)
    torch.manual_seed(seed)
    net, embed, opt = T.setup_model_and_optimizer(cfg)
    return T, cfg, net, embed, opt, np_params(net.state_dict())


def batch_of(pkg, eng, ds, weighted=True):
    """The GraphBatch of a dataset (or a list of its items) on the engine's device; `weighted`: with each graph's
    edge_values (None for a graph of unit weights), else no values at all."""
    items = list(ds.values()) if isinstance(ds, dict) else list(ds)
    vals = [it[0].edge_values(it[1]) for it in items] if weighted else None
    return pkg.GraphBatch([it[0] for it in items], vals, eng.device)


@contextlib.contextmanager
def fused(pkg, on):
    """gmc_set_fuse(on) for the block (None: as it is), restored after it."""
    if on is None:
        yield
        return
    lib = pkg.hip.load()
    prev = lib.gmc_set_fuse(on)
    try:
        yield
    finally:
        lib.gmc_set_fuse(prev)


def poison(eng, batch, grad=True):
    """Sizes the engine's training workspace for the batch, then fills it and (`grad`) the gradient with NaN."""
    eng._workspace(batch, True)
    eng._ws.fill_(255)                 # all-ones bytes = NaN
    if grad:
        eng.grad.fill_(float("nan"))


def _slab_of(W1: np.ndarray) -> np.ndarray:
    """gmc_model.W1_slab: [ceil(F/16)][N][16], pad columns zero."""
    N, F = W1.shape
    pad = np.zeros((N, (F + 15) // 16 * 16), np.float32)
    pad[:, :F] = W1
    return pad.reshape(N, -1, 16).transpose(1, 0, 2).copy()


# ---- the dropout mask of csrc/dropout.hip restated: splitmix64 of (seed, batch row, column), 24-bit uniform in float32
_U64 = np.uint64


def mix64(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
    return z ^ (z >> _U64(31))


def dropout_uniform(seed, rows, cols):
    """uniform_of(seed, row, col) for every (row, col) of the two index vectors: [len(rows), len(cols)] float32."""
    idx = np.asarray(rows, np.uint64)[:, None] * _U64(4096) + np.asarray(cols, np.uint64)[None, :] + _U64(1)
    with np.errstate(over="ignore"):
        h = mix64(_U64(seed) + _U64(0x9E3779B97F4A7C15) * idx)
    return (h >> _U64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def dropout_keep(seed, rows, cols, p):
    """The kept units of the batch rows x columns (the kernel keeps iff u >= p, both in float32)."""
    return dropout_uniform(seed, rows, cols) >= np.float32(p)


# ---- the gfx950 code objects of the built library (census tests; CPU only)
ROCM_LLVM = "/opt/rocm/llvm/bin"


def gfx950_code_objects(lib_path):
    """The gfx950 ELF code objects inside the library's offload bundles (the __CLANG_OFFLOAD_BUNDLE__ header)."""
    data = open(lib_path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out = []
    for m in re.finditer(re.escape(magic), data):
        p = m.start()
        (n,) = struct.unpack_from("<Q", data, p + len(magic))
        q = p + len(magic) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, q)
            triple = data[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if not triple.endswith("gfx950"):
                continue
            co = data[p + off:p + off + size]
            assert co[:4] == b"\x7fELF", triple
            out.append(co)
    assert out, "no gfx950 code object found in the library"
    return out


def kernel_symbols(lib_path):
    """Demangled names of every function in the library's gfx950 code objects (symbols read with llvm-readelf,
    demangled with c++filt)."""
    syms = set()
    for co in gfx950_code_objects(lib_path):
        out = subprocess.run([f"{ROCM_LLVM}/llvm-readelf", "-s", "--wide", "-"], input=co, capture_output=True,
                             check=True).stdout.decode()
        for line in out.splitlines():
            f = line.split()
            if len(f) >= 8 and f[3] == "FUNC" and f[7].startswith("_Z"):
                syms.add(f[7])
    dem = subprocess.run(["c++filt"], input="\n".join(sorted(syms)), capture_output=True, text=True, check=True).stdout
    return set(dem.splitlines())
