"""Contracting pinned nodes, without a GPU: the rule of include/gcnmaxcut.h as tests/contract_ref.py restates it keeps
every cut (checked on every assignment of small graphs), ``graph.contract`` is that restatement array for array, the
Python argument errors come before the library is touched, and the new entry points answer bad arguments with the
documented codes (fake non-NULL addresses: no call reaches a launch)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import contract_ref as CR

SOME, BIG = 4096, 1 << 40
GMC_OK, NULL, SHAPE, CLASSES, WORKSPACE, GRAPH_SIZE, ABI = 0, -1, -2, -3, -5, -6, -8

SMALL = [(n, K, weights, seed) for seed, (n, K) in enumerate([(5, 2), (6, 3), (7, 2), (8, 3), (9, 2), (10, 3), (10, 2)])
         for weights in ("unit", "integer")]


def pin_patterns(graph, K, seed):
    n = graph[0]
    counts = sorted({K, min(K + 1, n - 1), max(K, n // 2), n - 1})
    return [CR.drawn_pins(graph, K, count, seed * 10 + i) for i, count in enumerate(counts)]


@pytest.mark.parametrize("n,K,weights,seed", SMALL)
def test_every_honouring_assignment_keeps_its_cut(n, K, weights, seed):
    import gcn_max_cut_amd as pkg
    graph = CR.drawn_graph(n, n // 2 + 2, seed, weights)
    for pins in pin_patterns(graph, K, seed):
        ct = CR.contract(graph, pins, K)
        # the shipped host twin contracts to the same arrays, so what follows holds for it too
        same_contraction(pkg.graph.contract(handle_of(pkg, graph), *pin_arrays(pins, seed), K), ct, (n, K, weights, pins))
        full = CR.assignments(n, pins, K)
        image = np.zeros((full.shape[0], ct["graph"][0]), np.int64)
        image[:, ct["node_map"]] = full            # pinned nodes of class c all write c into column c
        assert (image[:, :K] == np.arange(K)).all()
        assert (image[:, ct["node_map"]] == full).all()
        original, contracted = CR.cut_of(graph, full), CR.cut_of(ct["graph"], image)
        assert np.array_equal(original, contracted + float(ct["fixed_cut"])), (pins, ct["fixed_cut"])
        assert original.max() == contracted.max() + float(ct["fixed_cut"])
        # every assignment of the contracted graph with p'[c] = c is the image of exactly one honouring assignment
        assert len({tuple(row) for row in image.tolist()}) == K ** (n - len(pins))


def handle_of(pkg, graph):
    n, rowptr, col, w = graph
    return pkg.GraphHandle(n, rowptr, col, w)


def pin_arrays(pins, seed=0, repeat=True):
    items = list(pins.items())
    if repeat:
        items.append(items[0])                       # one harmless repeat
    order = np.random.RandomState(seed).permutation(len(items))
    return (np.asarray([items[i][0] for i in order], np.int64), np.asarray([items[i][1] for i in order], np.int64))


def same_contraction(got, want, what):
    n, rowptr, col, w = want["graph"]
    h = got.handle
    assert h.n == n and h.rowptr.dtype == np.int32 and h.col.dtype == np.int32, what
    assert h.rowptr.tobytes() == rowptr.tobytes() and h.col.tobytes() == col.tobytes(), what
    assert (h.weight is None) == (w is None), what
    assert w is None or (h.weight.dtype == np.float32 and h.weight.tobytes() == w.tobytes()), what
    assert got.node_map.dtype == np.int32 and got.node_map.tobytes() == want["node_map"].tobytes(), what
    assert np.float32(got.fixed_cut).tobytes() == np.float32(want["fixed_cut"]).tobytes(), what
    assert got.pinned.dtype == np.bool_ and np.array_equal(got.pinned, want["pinned"]), what


HOST_CASES = [(7, 2, "unit", 1), (10, 3, "integer", 2), (40, 3, "signed", 3), (65, 8, "real", 4), (300, 2, "real", 5),
              (600, 4, "real", 6)]


@pytest.mark.parametrize("n,K,weights,seed", HOST_CASES)
def test_graph_contract_is_the_restatement(n, K, weights, seed):
    import gcn_max_cut_amd as pkg
    graph = CR.drawn_graph(n, 2 * n, seed, weights)
    for i, count in enumerate(sorted({K, max(K, (3 * n) // 10), n - 1})):
        pins = CR.drawn_pins(graph, K, count, seed * 7 + i)
        want = CR.contract(graph, pins, K)
        nodes, classes = pin_arrays(pins, seed)
        got = pkg.graph.contract(handle_of(pkg, graph), nodes, classes, K)
        same_contraction(got, want, (n, K, weights, count))
        again = pkg.graph.contract(handle_of(pkg, graph), torch.from_numpy(nodes[::-1].copy()).to(torch.int32),
                                   classes[::-1].astype(np.int16), K)
        same_contraction(again, want, (n, K, weights, count, "reversed, other dtypes"))
        part = np.random.RandomState(seed).randint(0, K, want["graph"][0])
        assert got.lift(part).dtype == np.int32 and np.array_equal(got.lift(part), part[want["node_map"]])


def test_a_self_loop_on_a_free_node_is_kept_and_one_on_a_pinned_node_is_dropped():
    import gcn_max_cut_amd as pkg
    edges = [(0, 1), (1, 2), (2, 3), (3, 4), (0, 4), (1, 1), (2, 2), (1, 3)]
    graph = CR.from_edges(5, sorted(edges), 3, "integer")
    pins = {1: 0, 4: 1}
    want = CR.contract(graph, pins, 2)
    n, rowptr, col, _w = want["graph"]
    loops = [(r, c) for r in range(n) for c in col[rowptr[r]:rowptr[r + 1]] if r == c]
    assert loops == [(int(want["node_map"][2]),) * 2]
    same_contraction(pkg.graph.contract(handle_of(pkg, graph), *pin_arrays(pins), 2), want, "loops")


def test_merged_weights_that_cancel_keep_their_entry():
    import gcn_max_cut_amd as pkg
    n, rowptr, col, _w = CR.from_edges(4, [(0, 1), (0, 2), (0, 3), (1, 3), (2, 3)], 0, "unit")
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    value = {(0, 1): 2.0, (0, 2): -2.0, (0, 3): 1.0, (1, 3): 1.0, (2, 3): 3.0}
    w = np.asarray([value[(min(r, c), max(r, c))] for r, c in zip(rows.tolist(), col.tolist())], np.float32)
    graph = (n, rowptr, col, w)
    pins = {1: 0, 2: 0, 3: 1}                       # node 0 sees class 0 through weights 2 and -2
    want = CR.contract(graph, pins, 2)
    n2, rp, cl, ww = want["graph"]
    assert n2 == 3 and cl.tolist() == [2, 2, 0, 1] and ww.tolist() == [0.0, 1.0, 0.0, 1.0]
    assert float(want["fixed_cut"]) == 4.0
    same_contraction(pkg.graph.contract(handle_of(pkg, graph), *pin_arrays(pins), 2), want, "cancelling")


def test_host_contract_names_what_is_wrong_with_the_pins():
    import gcn_max_cut_amd as pkg
    graph = CR.drawn_graph(12, 6, 9)
    h = handle_of(pkg, graph)
    i64 = lambda *a: np.asarray(a, np.int64)
    with pytest.raises(ValueError, match="2 pins with a node id out of range"):
        pkg.graph.contract(h, i64(0, 5, 12, -1), i64(0, 1, 0, 1), 2)
    with pytest.raises(ValueError, match=r"1 pins with a class outside 0\.\.1"):
        pkg.graph.contract(h, i64(0, 5, 7), i64(0, 1, 2), 2)
    with pytest.raises(ValueError, match="1 nodes pinned to two different classes"):
        pkg.graph.contract(h, i64(0, 5, 5, 5), i64(0, 1, 0, 1), 2)
    with pytest.raises(ValueError, match="1 graphs in which some class has no pinned node.*pin every class"):
        pkg.graph.contract(h, i64(0, 5), i64(0, 0), 2)
    with pytest.raises(ValueError, match="1 graphs without a free node"):
        pkg.graph.contract(h, np.arange(12), np.arange(12) % 2, 2)
    ring = CR.drawn_graph(12, 0, 1)
    with pytest.raises(ValueError, match="1 .graph, class. pairs whose pinned nodes have no free neighbour.*pin a node"):
        pkg.graph.contract(handle_of(pkg, ring), i64(3, 4, 5, 9), i64(0, 1, 0, 0), 2)   # node 4 sits between 3 and 5


def test_pin_lists_of_any_integer_dtype_keep_their_values():
    """Narrow dtypes hold neither -1 nor the upper bound of the clamp: they are widened first (CPU tensors here; the
    device takes the same path)."""
    from gcn_max_cut_amd.graph import _pin_ids
    cpu = torch.device("cpu")
    for dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, np.uint8, np.int8, np.uint16, np.int16,
                  np.uint32, np.int32, np.uint64, np.int64):
        values = [0, 1, 2, 7, 100]
        a = torch.tensor(values, dtype=dtype) if isinstance(dtype, torch.dtype) else np.asarray(values, dtype)
        for top in (3, 8, 1 << 20):
            got = _pin_ids(a, top, cpu)                                # (int32 goes as it is: the device checks the range)
            want = values if dtype in (torch.int32, np.int32) else [min(v, top) for v in values]
            assert got.dtype == torch.int32 and got.is_contiguous() and got.tolist() == want, (dtype, top)
    assert _pin_ids(torch.tensor([-5, 200], dtype=torch.int16), 8, cpu).tolist() == [-1, 8]
    assert _pin_ids(torch.tensor([250], dtype=torch.uint8), 8, cpu).tolist() == [8]
    for big in (torch.tensor([1 << 40, -(1 << 40), (1 << 32) + 1]), np.asarray([1 << 40, -(1 << 40), (1 << 32) + 1])):
        assert _pin_ids(big, 10, cpu).tolist() == [10, -1, 10]         # no id wraps into range
    assert _pin_ids(np.asarray([(1 << 64) - 1, 1 << 63, 5], np.uint64), 10, cpu).tolist() == [-1, -1, 5]   # refused either way


# ---- the Python argument errors come before the library is touched
@pytest.fixture
def no_library(monkeypatch):
    import gcn_max_cut_amd as pkg

    def refuse(*_a, **_k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(pkg.hip, "load", refuse)
    monkeypatch.setattr(pkg.hip, "require_gpu", refuse)
    return pkg


def test_argument_errors_come_before_the_library(no_library):
    pkg = no_library
    batch = pkg.GraphBatch.__new__(pkg.GraphBatch)
    batch.B, batch.R, batch.nnz, batch.device = 1, 10, 20, torch.device("cpu")
    good = np.arange(3)
    for nodes, classes, K, text in ((good, good, 1, "number_classes must be in 2..8"),
                                    (good, good, 9, "number_classes must be in 2..8"),
                                    (good.reshape(1, 3), good, 3, "nodes must be a one-dimensional array"),
                                    (good, np.arange(4), 4, "one length"),
                                    (good.astype(np.float32), good, 3, "nodes must hold integers"),
                                    (good, torch.zeros(3), 3, "classes must hold integers"),
                                    ([0, 1, 2], good, 3, "nodes must be a one-dimensional array")):
        with pytest.raises(ValueError, match=text):
            batch.contract(nodes, classes, K)
        with pytest.raises(ValueError, match=text):
            pkg.graph.contract(None, nodes, classes, K)
    ei = np.asarray([[0, 1, 1, 2, 2, 0], [1, 0, 2, 1, 0, 2]])
    kw = dict(num_nodes=3, hidden_dim=8, epochs=1, learning_rate=0.1)
    for solve in (pkg.maxcut.solve, pkg.maxcut.solve_large):
        with pytest.raises(ValueError, match="fixed .* terminals=True .* pass one of the two"):
            solve(ei, fixed=(good[:2], good[:2]), terminals=True, **kw)
        with pytest.raises(ValueError, match="fixed must be a pair"):
            solve(ei, fixed=good, **kw)
        with pytest.raises(ValueError, match="one length"):
            solve(ei, fixed=(good, good[:2]), **kw)
    for solve in (pkg.maxcut.solve_batch, pkg.maxcut.solve_large_batch):
        with pytest.raises(ValueError, match="pass one of the two"):
            solve(batch, fixed=(good[:2], good[:2]), terminals=True, hidden_dim=8, epochs=1, learning_rate=0.1)
        with pytest.raises(ValueError, match="classes must hold integers"):
            solve(batch, fixed=(good, good * 0.5), hidden_dim=8, epochs=1, learning_rate=0.1)


# ---- status codes of the entry points
def fields(**kw):
    return {**dict(B=2, R=120, nnz=840, n_max=60, nnz_max=420, goff=SOME, rowptr=SOME, gcol=SOME, lcol=SOME, dinv=SOME), **kw}


def call_map(hip, batch=None, K=3, P=4, nbytes=BIG, **a):
    g = {**dict(pin_node=SOME, pin_class=SOME, node_map=SOME, goff_out=SOME, report=SOME, ws=SOME), **a}
    b = None if batch is None else C.byref(hip.GmcBatch(**batch))
    return hip.load().gmc_contract_map(b, K, P, g["pin_node"], g["pin_class"], g["node_map"], g["goff_out"], g["report"],
                                       g["ws"], nbytes, None)


def call_entries(hip, batch=None, K=3, E=10, nbytes=BIG, **a):
    g = {**dict(node_map=SOME, goff_out=SOME, src=SOME, dst=SOME, w=SOME, fixed_cut=SOME, ws=SOME), **a}
    b = None if batch is None else C.byref(hip.GmcBatch(**batch))
    return hip.load().gmc_contract_entries(b, K, g["node_map"], g["goff_out"], E, g["src"], g["dst"], g["w"],
                                           g["fixed_cut"], g["ws"], nbytes, None)


def test_entry_points_check_their_arguments(built):
    hip = built.hip
    lib = hip.load()
    need = lib.gmc_contract_workspace_bytes(2, 120, 840, 3)
    none = lib.gmc_contract_workspace_bytes(0, 0, 0, 3)   # of an empty batch
    assert need >= 120 * 20 and need % 16 == 0
    assert lib.gmc_contract_workspace_bytes(2, 1 << 20, 7 << 20, 8) < 32 << 20
    for args in ((-1, 120, 840, 3), (2, -1, 840, 3), (2, 120, -1, 3), (2, 120, 1 << 31, 3), (2, 120, 840, 1),
                 (2, 120, 840, 9)):
        assert lib.gmc_contract_workspace_bytes(*args) == 0, args
    for call, outs, count in ((call_map, ("node_map", "goff_out", "report", "ws", "pin_node", "pin_class"), "P"),
                              (call_entries, ("node_map", "goff_out", "fixed_cut", "ws", "src", "dst", "w"), "E")):
        assert call(hip, None) == NULL
        for name in outs:
            assert call(hip, fields(), **{name: None}) == NULL, name
        assert call(hip, fields(abi=100)) == ABI
        assert call(hip, fields(abi=100), K=1) == ABI              # the abi word before any other field or argument
        assert call(hip, fields(abi=100, goff=None)) == ABI
        for name in ("goff", "rowptr", "gcol"):
            assert call(hip, fields(**{name: None})) == NULL, name
        for K in (1, 9, 0, -3):
            assert call(hip, fields(), K=K) == CLASSES, K
        assert call(hip, fields(B=-1), K=9) == CLASSES             # the class count before the sizes
        for name in ("B", "R", "nnz", "n_max"):
            assert call(hip, fields(**{name: -1})) == SHAPE, name
        assert call(hip, fields(), **{count: -1}) == SHAPE
        assert call(hip, fields(n_max=(1 << 20) + 1)) == GRAPH_SIZE
        assert call(hip, fields(B=-1), nbytes=0) == SHAPE          # the sizes before the workspace
        assert call(hip, fields(), nbytes=need - 1) == WORKSPACE
        assert call(hip, fields(B=0, R=0, nnz=0, n_max=0), nbytes=none) == GMC_OK   # nothing to launch
    assert call_map(hip, fields(B=0, R=0, nnz=0, n_max=0), P=0, pin_node=None, pin_class=None, nbytes=none) == GMC_OK
    assert call_entries(hip, fields(B=0, R=0, nnz=0, n_max=0), E=0, src=None, dst=None, w=None, nbytes=none) == GMC_OK
    assert set(("gmc_contract_workspace_bytes", "gmc_contract_map", "gmc_contract_entries")) <= set(hip.SYMBOLS)
    assert hip.CT_REPORT_WORDS == 8 and len(hip.CT_REPORT) == 8 and hip.CT_BAD_WORDS == 6
