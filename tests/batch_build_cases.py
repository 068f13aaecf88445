"""The graphs the device batch build is checked on (tests/test_batch_build_host.py, tests/test_gpu_batch_build.py): the
smallest shapes at which each of its kernels can go wrong, as networkx graphs - the yardstick is what ``from_networkx`` and
``GraphBatch(handles)`` make of them - and as the ``edge_index`` / ``ptr`` / ``edge_weight`` arrays of the same graphs."""
import functools

import networkx as nx
import numpy as np

from tests import util

MIXED = (5, 300, 65, 257)      # the batch the other suites use
WG_SORT = 4096                 # entries a workgroup sorts in LDS (csrc/batch_build.hip: kWgMax)


def regular(n, d, seed=0):
    return util.near_regular(n, d, seed, attrs=False)


def weighted(g, seed):
    """Real-valued float32 weights on every edge."""
    rng = np.random.RandomState(seed)
    for u, v in g.edges():
        g[u][v]["weight"] = float(np.float32(rng.uniform(0.25, 2.0)))
    return g


def ones(g):
    nx.set_edge_attributes(g, 1.0, "weight")
    return g


def with_loop(g, node):
    g.add_edge(node, node)
    return g


def hub(degree):
    return util.add_hub(regular(1000, 7, 3), degree, seed=degree, attrs=False)


# name -> the graphs of the batch
CASES = {
    "path3": lambda: [nx.path_graph(3)],
    "mixed": lambda: [regular(n, 4, i) for i, n in enumerate(MIXED)],
    "reg7_n64": lambda: [regular(64, 7)],                    # W = 8, NS = 7
    "reg7_n65": lambda: [regular(65, 7)],                    # the last quad partly absent
    "reg8": lambda: [regular(64, 8)],                        # NS = 8
    "reg12": lambda: [regular(64, 12)],                      # W = 16
    "reg16": lambda: [regular(66, 16), regular(35, 16, 1)],
    "star64": lambda: [nx.star_graph(64)],                   # the wave sort's last size
    "star65": lambda: [nx.star_graph(65)],                   # the workgroup sort's first
    "star70": lambda: [nx.star_graph(70), regular(20, 3)],
    "star_wg": lambda: [nx.star_graph(WG_SORT)],             # the workgroup sort's last size (no table: n > 4096)
    "star_wg1": lambda: [nx.star_graph(WG_SORT + 1)],        # the sort on global memory
    "hub40": lambda: [hub(40)],                              # overflow blocks
    "hub128": lambda: [hub(128)],                            # 15 blocks at W = 8: the most a row descriptor says
    "hub140": lambda: [hub(140)],                            # too many: no table
    "gnp300": lambda: [nx.gnp_random_graph(300, 0.1, seed=2)],
    "n4200": lambda: [regular(4200, 7, 5)],
    "loop": lambda: [with_loop(regular(20, 3, 1), 4), regular(9, 4)],
    "real": lambda: [weighted(regular(60, 7, 2), 1), weighted(hub(40), 2)],
    "mixed_weights": lambda: [regular(30, 5), weighted(regular(64, 7, 4), 3), regular(17, 4)],
    "all_ones": lambda: [ones(regular(40, 7)), ones(regular(33, 6))],
}


@functools.lru_cache(maxsize=None)
def graphs(name):
    return tuple(CASES[name]())


def edge_arrays(gs, pairs="both", dtype=np.int64, weights=None):
    """(edge_index [2, E], ptr [B+1], edge_weight [E] or None) of a list of networkx graphs on nodes 0..n-1.
    ``weights``: None gives them exactly when an edge carries one."""
    src, dst, w, ptr = [], [], [], [0]
    has_w = any("weight" in d for g in gs for _u, _v, d in g.edges(data=True)) if weights is None else weights
    for g in gs:
        off = ptr[-1]
        for u, v, wt in g.edges(data="weight", default=1.0):
            src.append(u + off); dst.append(v + off); w.append(wt)
            if pairs == "both" and u != v:
                src.append(v + off); dst.append(u + off); w.append(wt)
        ptr.append(off + g.number_of_nodes())
    ei = np.asarray([src, dst], dtype).reshape(2, -1)
    return ei, np.asarray(ptr, np.int64), (np.asarray(w, np.float32) if has_w else None)
