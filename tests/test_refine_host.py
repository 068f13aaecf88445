"""CPU checks of the local search over decoded partitions (include/gcnmaxcut.h, gmc_refine_order_host /
gmc_refine_local_f32): the host colouring against a plain-Python first-fit, the CPU restatement's own properties,
the kernel entry point's argument checks (no GPU needed) and the kernel's presence in the gfx950 code object."""
import ctypes as C
import subprocess

import networkx as nx
import numpy as np
import pytest

from oracle import ref_dense as R
from tests import refine_ref as RR
from tests import util


def handles_of(graphs):
    from gcn_max_cut_amd.graph import from_networkx
    return [from_networkx(g) for g in graphs]


def gnp_graph(n, p, seed):
    g = nx.gnp_random_graph(n, p, seed=seed)
    for v in range(n):                       # no isolated node (GraphBatch refuses zero in-degree)
        if g.degree(v) == 0:
            g.add_edge(v, (v + 1) % n)
    return g


def hub_graph(n, d, seed, hub=5, hub_degree=100):
    g = R.regular_graph(n, d, seed)
    rng = np.random.RandomState(seed)
    for u in rng.choice([v for v in range(n) if v != hub], hub_degree, replace=False):
        g.add_edge(hub, int(u))
    return g


def loop_graph(n, d, seed):
    g = R.regular_graph(n, d, seed)
    for v in range(0, n, 3):
        g.add_edge(v, v)
    return g


def host_order(batch_arrays, cap=None):
    from gcn_max_cut_amd import hip
    ba = batch_arrays
    order = np.full(max(ba.R, 1), -7, np.int32)
    cgoff = np.full(ba.B + 1, -7, np.int32)
    cptr = np.full(ba.R + ba.B if cap is None else cap, -7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    go = ba.goff.astype(np.int32)
    rc = hip.load().gmc_refine_order_host(ba.B, p(go), p(ba.rowptr), p(ba.lcol), p(order), p(cgoff), p(cptr),
                                          cptr.size)
    return rc, order, cgoff, cptr


COLOURING_CASES = {
    "regular_d3": [R.regular_graph(300, 3, 1)],
    "regular_d7": [R.regular_graph(1000, 7, 2)],
    "regular_d12": [R.regular_graph(500, 12, 3)],
    "gnp_hubs": [gnp_graph(800, 0.01, 4), hub_graph(400, 7, 5)],
    "self_loops": [loop_graph(200, 6, 6)],
    "mixed": [nx.complete_graph(3), R.regular_graph(50, 6, 7), nx.complete_graph(4), R.regular_graph(4096, 7, 8),
              R.regular_graph(100, 3, 9)],
}


@pytest.mark.parametrize("case", sorted(COLOURING_CASES))
def test_host_colouring_is_first_fit(built, case):
    from gcn_max_cut_amd.graph import BatchArrays
    hs = handles_of(COLOURING_CASES[case])
    ba = BatchArrays(hs)
    rc, order, cgoff, cptr = host_order(ba)
    assert rc == 0
    ref_order, ref_cgoff, ref_cptr = RR.order_of_batch(hs)
    moving = ba.R - 3 * ba.B
    assert (order[:moving] == ref_order).all() and (order[moving:] == -7).all()
    assert (cgoff == ref_cgoff).all()
    assert (cptr[:cgoff[-1]] == ref_cptr).all() and (cptr[cgoff[-1]:] == -7).all()
    for g, h in enumerate(hs):
        r0 = int(ba.goff[g])
        lo, hi = cptr[cgoff[g]], cptr[cgoff[g + 1] - 1]
        assert sorted(order[lo:hi] - r0) == list(range(3, h.n))       # a permutation of the movable rows
        if h.n == 3:
            assert cgoff[g + 1] - cgoff[g] == 1                        # no class at all
        for k in range(cgoff[g], cgoff[g + 1] - 1):
            cls = set((order[cptr[k]:cptr[k + 1]] - r0).tolist())
            assert cls and list(order[cptr[k]:cptr[k + 1]]) == sorted(order[cptr[k]:cptr[k + 1]])
            for v in cls:                                              # independent among movable nodes
                nb = set(h.col[h.rowptr[v]:h.rowptr[v + 1]].tolist()) - {v}
                assert not (nb & cls), (case, g, k, v)


def test_host_colouring_refuses_bad_sizes(built):
    from gcn_max_cut_amd import hip
    from gcn_max_cut_amd.graph import BatchArrays
    ba = BatchArrays(handles_of([R.regular_graph(60, 5, 1), nx.complete_graph(3)]))
    rc, *_ = host_order(ba, cap=ba.R + ba.B - 1)
    assert rc == -2                                                    # GMC_ERR_SHAPE
    rc, order, cgoff, cptr = host_order(ba, cap=ba.R + ba.B)
    assert rc == 0
    lib = hip.load()
    null = C.c_void_p(None)
    some = (C.c_int32 * 8)()
    assert lib.gmc_refine_order_host(1, null, some, some, some, some, some, 8) == -1
    assert lib.gmc_refine_order_host(-1, some, some, some, some, some, some, 8) == -2
    goff = (C.c_int32 * 2)(0, 2)                                       # a two-node graph
    assert lib.gmc_refine_order_host(1, goff, some, some, some, some, some, 8) == -6


def edge_graph(n, edges):
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(edges)
    return g


# A graph whose first-fit classes are {3} {4, 5} {6} (5 and 6 adjacent), and one ({3, 5} {4}) whose colouring stamps
# colour 1 with node id 5: coloured after it in the same batch, the second graph must come out as on its own.
STAMP_GRAPH = lambda: edge_graph(6, [(0, 1), (1, 2), (2, 0), (0, 3), (3, 4), (4, 5)])
VICTIM_GRAPH = lambda: edge_graph(7, [(0, 1), (1, 2), (2, 0), (0, 3), (3, 4), (3, 5), (3, 6), (5, 6)])


def product_classes(batch_arrays):
    """Per graph of the batch, the classes gmc_refine_order_host made, as lists of local ids."""
    rc, order, cgoff, cptr = host_order(batch_arrays)
    assert rc == 0
    out = []
    for g in range(batch_arrays.B):
        r0 = int(batch_arrays.goff[g])
        out.append([(order[cptr[k]:cptr[k + 1]] - r0).tolist() for k in range(cgoff[g], cgoff[g + 1] - 1)])
    return out


def test_host_colouring_of_a_graph_does_not_depend_on_the_graphs_before_it(built):
    from gcn_max_cut_amd.graph import BatchArrays
    alone = product_classes(BatchArrays(handles_of([VICTIM_GRAPH()])))[0]
    assert alone == [[3], [4, 5], [6]]
    after = product_classes(BatchArrays(handles_of([STAMP_GRAPH(), VICTIM_GRAPH()])))
    assert after[0] == [[3, 5], [4]] and after[1] == alone
    # the same over random small graphs in several batch orders
    rng = np.random.RandomState(3)
    graphs = [gnp_graph(int(rng.randint(4, 40)), float(rng.uniform(0.1, 0.5)), 100 + i) for i in range(40)]
    solo = [product_classes(BatchArrays(handles_of([g])))[0] for g in graphs]
    for _ in range(4):
        perm = rng.permutation(len(graphs))
        batched = product_classes(BatchArrays(handles_of([graphs[i] for i in perm])))
        for i, cls in zip(perm, batched):
            assert cls == solo[i], i
    hs = handles_of(graphs)
    for h, cls in zip(hs, solo):
        assert cls == [c.tolist() for c in RR.colouring(h.n, h.rowptr, h.col)[1]]


def random_case(seed, n=120, d=6, weights=None, cands=12, loops=False):
    g = loop_graph(n, d, seed) if loops else R.regular_graph(n, d, seed)
    h = handles_of([g])[0]
    rng = np.random.RandomState(seed)
    w = None
    if weights == "int":
        w = rng.randint(1, 5, h.col.size).astype(np.float32)
    elif weights == "float":
        w = rng.uniform(0.1, 2.0, h.col.size).astype(np.float32)
    if w is not None:                                                  # symmetric: one value per undirected edge
        rows = np.repeat(np.arange(h.n), np.diff(h.rowptr))
        key = {}
        for e, (a, b) in enumerate(zip(rows, h.col)):
            w[e] = key.setdefault((min(a, b), max(a, b)), w[e])
    A = rng.randint(0, 3, (cands, h.n)).astype(np.int8)
    A[:, :3] = rng.randint(0, 3, (cands, 3))                           # terminals hold anything; they never move
    return h, w, A


@pytest.mark.parametrize("seed,weights,loops", [(1, None, False), (2, "int", False), (3, None, True), (4, "float", False)])
def test_restatement_converges_to_a_local_optimum(built, seed, weights, loops):
    """The sweeps run over the classes gmc_refine_order_host made (equal to the restatement's own first-fit)."""
    from gcn_max_cut_amd.graph import BatchArrays
    h, w, A = random_case(seed, weights=weights, loops=loops)
    classes = [np.asarray(c) for c in product_classes(BatchArrays([h]))[0]]
    assert [c.tolist() for c in classes] == [c.tolist() for c in RR.colouring(h.n, h.rowptr, h.col)[1]]
    out, sweeps = RR.refine(h.n, h.rowptr, h.col, w, A, 100, classes=classes)
    assert (sweeps < 100).all() and (sweeps >= 1).all()
    assert (out[:, :3] == A[:, :3]).all()
    for a0, a1 in zip(A, out):
        before, after = RR.cut(h.rowptr, h.col, w, a0), RR.cut(h.rowptr, h.col, w, a1)
        assert after >= before - 1e-9 * max(1.0, before)
        assert RR.best_single_move_gain(h.n, h.rowptr, h.col, w, a1) <= 1e-5 * max(1.0, after)
    again, sweeps2 = RR.refine(h.n, h.rowptr, h.col, w, out, 100)
    assert (again == out).all() and (sweeps2 == 1).all()              # a converged candidate: one sweep, no move
    none, sweeps0 = RR.refine(h.n, h.rowptr, h.col, w, A, 0)
    assert (none == A).all() and (sweeps0 == 0).all()


@pytest.mark.parametrize("seed,weights,loops", [(5, None, False), (6, "int", True), (7, "float", False)])
def test_one_parallel_sweep_is_one_sequential_sweep(built, seed, weights, loops):
    """One parallel sweep over the classes gmc_refine_order_host made is one sequential sweep in (colour, id) order:
    every class the product makes is an independent set."""
    from gcn_max_cut_amd.graph import BatchArrays
    h, w, A = random_case(seed, n=80, weights=weights, loops=loops, cands=4)
    A[0, 7] = -1                                                       # a byte of no class: counts for nothing, moves
    classes = [np.asarray(c) for c in product_classes(BatchArrays([h]))[0]]
    out, sweeps = RR.refine(h.n, h.rowptr, h.col, w, A, 1, classes=classes)
    assert (sweeps == 1).all()
    for a0, a1 in zip(A, out):
        assert RR.sequential_sweep(h.n, h.rowptr, h.col, w, a0.tolist()) == a1.tolist()
    assert 0 <= out[0, 7] <= 2


def test_refine_entry_point_checks_arguments_without_a_gpu(built):
    hip = built.hip
    lib = hip.load()
    null, some = C.c_void_p(None), C.c_void_p(4096)                    # (never dereferenced: the calls fail first)
    b = hip.GmcBatch(B=2, R=100, n_max=60, goff=4096, rowptr=4096, lcol=4096)
    f = lambda batch, *rest, cands=4, sweeps=10, out=some: lib.gmc_refine_local_f32(
        batch, some, some, some, cands, some, sweeps, some, some, some, out, null, None)
    assert f(C.byref(b), out=null) == -1                               # GMC_ERR_NULL (best_idx)
    assert lib.gmc_refine_local_f32(C.byref(b), null, some, some, 4, some, 10, some, some, some, some, null, None) == -1
    assert f(None) == -1
    assert f(C.byref(hip.GmcBatch(abi=100, B=2, R=100, n_max=60, goff=4096, rowptr=4096, lcol=4096))) == -8
    assert f(C.byref(hip.GmcBatch(B=2, R=100, n_max=60, goff=4096, rowptr=4096))) == -1       # lcol
    assert f(C.byref(b), cands=0) == -2
    assert f(C.byref(b), sweeps=-1) == -2
    assert f(C.byref(hip.GmcBatch(B=2, R=100, n_max=4097, goff=4096, rowptr=4096, lcol=4096))) == -6
    assert f(C.byref(hip.GmcBatch(B=2, R=100, n_max=2, goff=4096, rowptr=4096, lcol=4096))) == -6
    assert f(C.byref(hip.GmcBatch(B=0, goff=4096, rowptr=4096, lcol=4096))) == 0               # nothing launched
    assert "refine" in hip.KERNEL_TAGS and hip.KERNEL_TAGS.index("refine") == 15


def test_refine_kernel_is_in_the_code_object_without_scratch(built):
    lib_path = built.hip.LIB_PATH
    names = util.kernel_symbols(lib_path)
    assert any("refine_local_kernel" in s for s in names), sorted(names)
    seen = 0
    for co in util.gfx950_code_objects(lib_path):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            if "refine_local_kernel" in entry and ".name:" in entry:
                fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith("."))
                if "refine_local_kernel" not in fields.get(".name", ""):
                    continue
                seen += 1
                assert int(fields[".private_segment_fixed_size"]) == 0
                assert int(fields[".vgpr_spill_count"]) == 0
    assert seen == 1
