"""GPU checks of ``GraphBatch.contract`` (gmc_contract_map / gmc_contract_entries, csrc/contract.hip) and of
``maxcut.solve*(..., fixed=...)``.

The contraction is compared byte for byte: every array and scalar of ``Contraction.batch`` against ``GraphBatch`` built
from the contracted graphs of tests/contract_ref.py (the numpy restatement of the rule in include/gcnmaxcut.h, in its sum
orders), plus ``node_map``, ``fixed_cut`` and ``pinned``.  The kernel has one row regime (a thread per row), so the row
lengths 1, 8, 9, 64 and 65 are there for the issue's sake and the tiles of 256 rows (graphs of 256, 257 and 300 nodes, more
than one workgroup per graph) for the fold's.  The solver checks use integer weights, for which every cut is exact."""
import functools

import numpy as np
import pytest
import torch

from tests import contract_ref as CR
from tests import util
from tests.test_gpu_batch_build import same_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


# ---- the cases: (graphs, pins per graph, K)
def row_lengths_graph(weights):
    """70 pool nodes on a ring, and free nodes 70..74 joined to the first 1, 8, 9, 64 and 65 pool nodes."""
    edges = [(i, (i + 1) % 70) if i < 69 else (0, 69) for i in range(70)]
    for node, degree in zip(range(70, 75), (1, 8, 9, 64, 65)):
        edges += [(p, node) for p in range(degree)]
    return CR.from_edges(75, sorted(edges), 5, weights)


def row_lengths_pins(K):
    """Every third pool node, classes in turn - so the long free rows have several neighbours in every class - plus two
    adjacent pairs: 10, 11 in one class and 22, 23 in two."""
    pins = {i: (i // 3) % K for i in range(0, 70, 3)}
    pins[10] = pins[11] = 1
    pins[22], pins[23] = 0, 1
    return pins


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "one_per_class_b1":
        gs, K = [CR.drawn_graph(40, 60, 1)], 2
        return gs, [CR.drawn_pins(gs[0], K, K, 1)], K
    if name == "third_pinned_b5":
        sizes, K = (6, 65, 257, 300, 33), 3
        gs = [CR.drawn_graph(n, 2 * n, 10 + i, "integer") for i, n in enumerate(sizes)]
        return gs, [CR.drawn_pins(g, K, max(K, (3 * g[0]) // 10), 20 + i) for i, g in enumerate(gs)], K
    if name == "eight_classes_real_b5":
        sizes, K = (20, 256, 100, 300, 65), 8
        gs = [CR.drawn_graph(n, 3 * n, 30 + i, "real") for i, n in enumerate(sizes)]
        return gs, [CR.drawn_pins(g, K, max(K, (3 * g[0]) // 10), 40 + i) for i, g in enumerate(gs)], K
    if name == "all_but_one_signed":
        sizes, K = (9, 70, 300), 2
        gs = [CR.drawn_graph(n, 2 * n, 50 + i, "signed") for i, n in enumerate(sizes)]
        return gs, [CR.drawn_pins(g, K, g[0] - 1, 60 + i) for i, g in enumerate(gs)], K
    if name == "row_lengths_unit":
        return [row_lengths_graph("unit")], [row_lengths_pins(3)], 3
    if name == "row_lengths_real":
        return [CR.drawn_graph(12, 6, 3, "real"), row_lengths_graph("real")], \
            [CR.drawn_pins(CR.drawn_graph(12, 6, 3, "real"), 8, 8, 2), row_lengths_pins(8)], 8
    raise KeyError(name)


CASES = ("one_per_class_b1", "third_pinned_b5", "eight_classes_real_b5", "all_but_one_signed", "row_lengths_unit",
         "row_lengths_real")


def edge_arrays(gs):
    src, dst, w, ptr = [], [], [], [0]
    for n, rowptr, col, weight in gs:
        src.append(np.repeat(np.arange(n), np.diff(rowptr)) + ptr[-1])
        dst.append(col.astype(np.int64) + ptr[-1])
        w.append(np.ones(col.size, np.float32) if weight is None else weight)
        ptr.append(ptr[-1] + n)
    weighted = any(g[3] is not None for g in gs)
    return np.stack([np.concatenate(src), np.concatenate(dst)]), np.asarray(ptr, np.int64), \
        (np.concatenate(w) if weighted else None)


def pin_arrays(pins_per_graph, ptr, seed=0, repeat=True):
    """Global (nodes, classes) int64 in a drawn order, with one harmless repeat."""
    items = [(u + int(ptr[g]), c) for g, pins in enumerate(pins_per_graph) for u, c in pins.items()]
    if repeat:
        items.append(items[len(items) // 2])
    order = np.random.RandomState(seed).permutation(len(items))
    return np.asarray([items[i][0] for i in order], np.int64), np.asarray([items[i][1] for i in order], np.int64)


_built = {}


def original(pkg, name):
    if name not in _built:
        gs, pins, K = case(name)
        ei, ptr, w = edge_arrays(gs)
        _built[name] = (pkg.GraphBatch.from_edge_index(ei, ptr, edge_weight=w), ei, ptr, w)
    return _built[name]


_wanted = {}


def wanted(pkg, name):
    """The restatement's contraction of every graph of the case and the ``GraphBatch`` of the contracted graphs: built
    once, shared, never written."""
    if name not in _wanted:
        gs, pins, K = case(name)
        cts = [CR.contract(g, p, K) for g, p in zip(gs, pins)]
        batch = pkg.GraphBatch([pkg.GraphHandle(*ct["graph"]) for ct in cts])
        goff = np.concatenate([[0], np.cumsum([ct["graph"][0] for ct in cts])])
        node_map = np.concatenate([ct["node_map"] + goff[g] for g, ct in enumerate(cts)]).astype(np.int32)
        fixed = np.asarray([ct["fixed_cut"] for ct in cts], np.float32)
        _wanted[name] = (batch, node_map, fixed, np.concatenate([ct["pinned"] for ct in cts]))
    return _wanted[name]


def same_contraction(got, want, what):
    batch, node_map, fixed, pinned = want
    same_batch(got.batch, batch, what)
    for name, a, b in (("node_map", got.node_map, node_map), ("fixed_cut", got.fixed_cut, fixed), ("pinned", got.pinned, pinned)):
        assert a.is_cuda and a.cpu().numpy().dtype == b.dtype and a.cpu().numpy().tobytes() == b.tobytes(), (what, name)


@pytest.mark.parametrize("name", CASES)
def test_contraction_equals_the_restatement(pkg, name):
    gs, pins, K = case(name)
    batch, _ei, ptr, _w = original(pkg, name)
    got = batch.contract(*pin_arrays(pins, ptr), K)
    same_contraction(got, wanted(pkg, name), name)
    print(f"{name}: B {batch.B} R {batch.R} nnz {batch.nnz} -> R' {got.batch.R} nnz' {got.batch.nnz} weights "
          f"{got.batch.vals is not None} fixed_cut {got.fixed_cut.cpu().tolist()}")
    part = torch.from_numpy(np.random.RandomState(1).randint(0, K, got.batch.R).astype(np.int32)).cuda()
    lifted = got.lift(part)
    assert lifted.dtype == torch.int32 and torch.equal(lifted, part[got.node_map.long()])


def test_cases_hold_what_they_are_there_for(pkg):
    gs, pins, K = case("row_lengths_real")
    n, rowptr, col, _w = gs[1]
    free_lengths = {int(rowptr[u + 1] - rowptr[u]) for u in range(n) if u not in pins[1]}
    assert {1, 8, 9, 64, 65} <= free_lengths
    classes_of = lambda u: [pins[1][int(x)] for x in col[rowptr[u]:rowptr[u + 1]] if int(x) in pins[1]]
    assert set(classes_of(74)) == set(range(8)) and max(np.bincount(classes_of(74))) >= 2
    adjacent = [(u, int(x)) for u in pins[1] for x in col[rowptr[u]:rowptr[u + 1]] if int(x) in pins[1] and x > u]
    assert any(pins[1][a] == pins[1][b] for a, b in adjacent) and any(pins[1][a] != pins[1][b] for a, b in adjacent)
    assert wanted(pkg, "row_lengths_real")[2][1] > 0 and wanted(pkg, "one_per_class_b1")[0].vals is None
    assert wanted(pkg, "third_pinned_b5")[0].vals is not None          # merged unit... integer sums are weights
    assert all(len(p) == g[0] - 1 for g, p in zip(*case("all_but_one_signed")[:2]))
    assert wanted(pkg, "row_lengths_unit")[0].vals is not None         # counts above 1 on a unit-weight graph


@pytest.mark.parametrize("name", ["third_pinned_b5", "row_lengths_real"])
def test_pin_list_forms_and_orders_give_the_same_bytes(pkg, name):
    gs, pins, K = case(name)
    batch, _ei, ptr, _w = original(pkg, name)
    want = wanted(pkg, name)
    for seed in (1, 2, 2):                                             # two orders, the last one twice
        nodes, classes = pin_arrays(pins, ptr, seed)
        same_contraction(batch.contract(nodes, classes, K), want, f"{name} int64 on the host, order {seed}")
    nodes, classes = pin_arrays(pins, ptr, 3)
    dev = lambda a, dtype: torch.from_numpy(a).to(dtype).cuda()
    same_contraction(batch.contract(dev(nodes, torch.int32), dev(classes, torch.int32), K), want, f"{name} int32 on the device")
    same_contraction(batch.contract(torch.from_numpy(nodes), classes.astype(np.uint8), K), want, f"{name} mixed forms")
    nodes, classes = pin_arrays(pins, ptr, 4, repeat=False)
    same_contraction(batch.contract(np.sort(nodes), classes[np.argsort(nodes)], K), want, f"{name} sorted, no repeat")


def test_a_batch_built_from_handles_contracts_to_the_same_bytes(pkg):
    name = "eight_classes_real_b5"
    gs, pins, K = case(name)
    batch = pkg.GraphBatch([pkg.GraphHandle(*g) for g in gs])
    same_contraction(batch.contract(*pin_arrays(pins, batch.goff_host), K), wanted(pkg, name), "from handles")


def test_an_empty_batch_contracts_to_an_empty_batch(pkg):
    from gcn_max_cut_amd import maxcut
    none = np.zeros(0, np.int64)
    batch = pkg.GraphBatch.from_edge_index(np.zeros((2, 0), np.int64), np.zeros(1, np.int64))
    ct = batch.contract(none, none, 3)
    assert ct.batch.B == 0 and ct.batch.R == 0 and ct.batch.nnz == 0
    assert [tuple(t.shape) for t in (ct.node_map, ct.fixed_cut, ct.pinned)] == [(0,)] * 3
    res = maxcut.solve_batch(batch, fixed=(none, none), number_classes=3, hidden_dim=8, epochs=1, learning_rate=0.1)
    assert tuple(res.partition.shape) == (0,) and tuple(res.cut.shape) == (0,) and tuple(res.fixed_cut.shape) == (0,)


# ---- bad input: counted on the device, refused before the entries stage
@pytest.fixture
def entries_calls(pkg, monkeypatch):
    lib, calls = pkg.hip.load(), []
    real = lib.gmc_contract_entries
    monkeypatch.setattr(lib, "gmc_contract_entries", lambda *a: calls.append(1) or real(*a))
    return calls


def test_bad_pins_are_refused(pkg, entries_calls):
    gs = [CR.drawn_graph(12, 0, 1), CR.drawn_graph(20, 10, 2)]
    ei, ptr, w = edge_arrays(gs)
    batch = pkg.GraphBatch.from_edge_index(ei, ptr)
    i64 = lambda *a: np.asarray(a, np.int64)
    good_n, good_c = i64(0, 6, 12, 20), i64(0, 1, 0, 1)
    add = lambda nodes, classes: (np.concatenate([good_n, i64(*nodes)]), np.concatenate([good_c, i64(*classes)]))
    for nodes, dtype in (((32, -1, 1 << 20), np.int64), ((32, -7, 1 << 40), np.int64), ((32, -1, -(1 << 31)), np.int32)):
        n, c = add(nodes, (0, 1, 0))
        with pytest.raises(ValueError, match="3 pins with a node id out of range"):
            batch.contract(n.astype(dtype), c, 2)
        with pytest.raises(ValueError, match="3 pins with a node id out of range"):
            batch.contract(torch.from_numpy(n.astype(dtype)).cuda(), torch.from_numpy(c).cuda(), 2)
    with pytest.raises(ValueError, match=r"2 pins with a class outside 0\.\.1"):
        batch.contract(*add((3, 4), (2, -1)), 2)
    with pytest.raises(ValueError, match=r"1 pins with a class outside 0\.\.2"):
        batch.contract(*add((3, 4), (2, 1 << 33)), 3)
    with pytest.raises(ValueError, match="2 nodes pinned to two different classes"):
        batch.contract(*add((3, 3, 3, 25, 25), (0, 1, 0, 1, 0)), 2)
    with pytest.raises(ValueError, match="1 graphs in which some class has no pinned node.*pin every class"):
        batch.contract(i64(0, 6, 12), i64(0, 1, 0), 2)
    with pytest.raises(ValueError, match="2 graphs in which some class has no pinned node"):
        batch.contract(i64(), i64(), 2)                                # no pins at all
    with pytest.raises(ValueError, match="1 graphs without a free node"):
        batch.contract(np.concatenate([np.arange(12), i64(12, 20)]), np.concatenate([np.arange(12) % 2, i64(0, 1)]), 2)
    with pytest.raises(ValueError, match="1 .graph, class. pairs whose pinned nodes have no free neighbour.*pin a node"):
        batch.contract(i64(3, 4, 5, 12, 20), i64(0, 1, 0, 0, 1), 2)    # node 4 of the ring sits between 3 and 5
    assert entries_calls == []
    assert batch.contract(good_n, good_c, 2).batch.R == 32 - 4 + 2 * 2   # and the good pins alone are taken
    assert entries_calls == [1]


# ---- one pin per class is a relabelling
@pytest.mark.parametrize("n,K", [(50, 2), (50, 3), (200, 2), (200, 3)])
def test_one_pin_per_class_is_a_relabelling(pkg, n, K):
    from gcn_max_cut_amd import maxcut
    g = util.near_regular(n, 7, 3, attrs=False)
    rng = np.random.RandomState(n + K)
    while True:                                                        # K nodes no two of which are adjacent
        pins = [int(u) for u in rng.permutation(n)[:K]]
        if not any(g.has_edge(a, b) for a in pins for b in pins):
            break
    rest = [u for u in range(n) if u not in pins]
    new_id = np.empty(n, np.int64)
    new_id[pins + rest] = np.arange(n)                                 # terminals first, the rest ascending
    edges = np.asarray([(a, b) for a, b in g.edges()] + [(b, a) for a, b in g.edges()], np.int64).T
    kw = dict(num_nodes=n, number_classes=K, hidden_dim=8, epochs=5, learning_rate=2e-2, samples=4, anneal_sweeps=5, seed=2)
    by_hand = maxcut.solve(new_id[edges], terminals=True, **kw)
    pinned = maxcut.solve(edges, fixed=(np.asarray(pins), np.arange(K)), **kw)
    assert pinned.partition.cpu().numpy().tobytes() == by_hand.partition.cpu().numpy()[new_id].tobytes()
    assert pinned.partition.cpu().numpy()[pins].tolist() == list(range(K))
    for name in ("cut", "trained_cut", "rounded_cut", "ptr"):
        assert getattr(pinned, name).cpu().numpy().tobytes() == getattr(by_hand, name).cpu().numpy().tobytes(), name
    assert pinned.fixed_cut.cpu().tolist() == [0.0] and by_hand.fixed_cut is None


# ---- the solvers with many pins per class
def recount(gs, ptr, partition):
    return np.asarray([CR.cut_of(g, partition[ptr[i]:ptr[i + 1]])[0] for i, g in enumerate(gs)], np.float32)


@functools.lru_cache(maxsize=None)
def solver_case(K):
    sizes = (8, 10, 60, 130)
    gs = [CR.drawn_graph(n, n, 70 + K + i, "integer") for i, n in enumerate(sizes)]
    return gs, [CR.drawn_pins(g, K, max(K, g[0] // 3), 80 + K + i) for i, g in enumerate(gs)]


@pytest.mark.parametrize("K", [2, 3, 4])
def test_solve_with_many_pins_per_class(pkg, K):
    from gcn_max_cut_amd import maxcut
    gs, pins = solver_case(K)
    ei, ptr, w = edge_arrays(gs)
    nodes, classes = pin_arrays(pins, ptr, K)
    kw = dict(number_classes=K, hidden_dim=8, epochs=5, learning_rate=2e-2, samples=4, anneal_sweeps=5, seed=3)
    res = maxcut.solve(ei, ptr, edge_weight=w, fixed=(nodes, classes), **kw)
    part = res.partition.cpu().numpy()
    assert res.partition.dtype == torch.int32 and part.shape == (int(ptr[-1]),) and res.ptr.cpu().tolist() == ptr.tolist()
    assert np.array_equal(part[nodes], classes)                        # every pin is honoured
    cut, trained, rounded = (t.cpu().numpy() for t in (res.cut, res.trained_cut, res.rounded_cut))
    print("K", K, "cut", cut, "trained", trained, "rounded", rounded, "fixed", res.fixed_cut.cpu().numpy())
    assert np.array_equal(cut, recount(gs, ptr, part))
    assert (cut >= trained).all() and (cut >= rounded).all()
    # the contracted run on its own: its cut plus the constant is the cut on the original graph
    batch = pkg.GraphBatch.from_edge_index(ei, ptr, edge_weight=w)
    ct = batch.contract(nodes, classes, K)
    inner = maxcut.solve_batch(ct.batch, terminals=True, **kw)
    assert torch.equal(ct.lift(inner.partition), res.partition)
    for name in ("cut", "trained_cut", "rounded_cut"):
        assert torch.equal(getattr(inner, name) + ct.fixed_cut, getattr(res, name)), name
    assert torch.equal(res.fixed_cut, ct.fixed_cut)
    for i, g in enumerate(gs):                                         # against every honouring assignment
        if g[0] <= 10:
            assert cut[i] <= CR.cut_of(g, CR.assignments(g[0], pins[i], K)).max()
    again = maxcut.solve_batch(pkg.GraphBatch([pkg.GraphHandle(*g) for g in gs]), fixed=(torch.from_numpy(nodes).cuda(),
                               torch.from_numpy(classes).to(torch.int32).cuda()), **kw)
    for name in ("partition", "cut", "trained_cut", "rounded_cut", "ptr", "fixed_cut"):
        assert getattr(again, name).cpu().numpy().tobytes() == getattr(res, name).cpu().numpy().tobytes(), name


def test_solve_with_pins_and_the_tabu_stage(pkg):
    from gcn_max_cut_amd import maxcut
    gs, pins = solver_case(3)
    ei, ptr, w = edge_arrays(gs)
    nodes, classes = pin_arrays(pins, ptr, 1)
    res = maxcut.solve(ei, ptr, edge_weight=w, fixed=(nodes, classes), number_classes=3, hidden_dim=8, epochs=3,
                       learning_rate=2e-2, samples=4, anneal_sweeps=5, seed=3, tabu_iterations=20)
    part = res.partition.cpu().numpy()
    assert np.array_equal(part[nodes], classes) and np.array_equal(res.cut.cpu().numpy(), recount(gs, ptr, part))
    assert (res.cut >= res.annealed_cut).all() and (res.annealed_cut >= res.rounded_cut).all()


def test_solve_large_with_pins(pkg):
    from gcn_max_cut_amd import maxcut
    n, K = 5000, 2
    g = util.near_regular(n, 7, 9, attrs=False)
    edges = np.asarray([(a, b) for a, b in g.edges()] + [(b, a) for a, b in g.edges()], np.int64).T
    rng = np.random.RandomState(5)
    nodes = rng.permutation(n)[:n // 10]
    classes = rng.randint(0, K, nodes.size)
    res = maxcut.solve_large(edges, num_nodes=n, fixed=(nodes, classes), number_classes=K, hidden_dim=8, epochs=3,
                             learning_rate=2e-2, samples=2, anneal_sweeps=5, max_descent_sweeps=5, seed=1)
    part = res.partition.cpu().numpy()
    assert part.shape == (n,) and np.array_equal(part[nodes], classes)
    want = float((part[edges[0]] != part[edges[1]]).sum()) / 2
    fixed = float(((classes[:, None] != classes[None, :]) & np.asarray(
        [[g.has_edge(int(a), int(b)) for b in nodes] for a in nodes])).sum()) / 2
    print("solve_large with pins: cut", res.cut.cpu().tolist(), "fixed_cut", res.fixed_cut.cpu().tolist())
    assert res.cut.cpu().tolist() == [want] and res.fixed_cut.cpu().tolist() == [fixed]
    assert (res.cut >= res.trained_cut).all() and (res.cut >= res.rounded_cut).all()


# ---- solve judges the size on the contracted graph: an original graph beyond the small decoders, a contraction within
@functools.lru_cache(maxsize=None)
def oversized_case(weights):
    n, K = 4500, 3
    g = CR.drawn_graph(n, 2 * n, 91, weights)
    rng = np.random.RandomState(92)
    nodes = rng.permutation(n)[:(2 * n) // 5]                          # 40 % pinned: 2,703 nodes are left
    return g, nodes.astype(np.int64), rng.randint(0, K, nodes.size).astype(np.int64), K


@pytest.mark.parametrize("weights", ["unit", "real"])
def test_solve_takes_a_large_graph_whose_contraction_is_small(pkg, weights):
    """The original graph (4,500 nodes) is beyond ``hip.MAX_GRAPH_NODES``, the contracted one is not: ``solve`` runs its
    own route on the contraction and recounts on the original with the large decoders' scoring call.  Unit weights: every
    cut is exact, so it is the numpy count and the contracted run's cut plus ``fixed_cut``.  Real weights: the bits of
    another large decoder for the same bytes (``large_local_search`` without sweeps), and a float64 recount within the
    fp32 sum's bound - at most 64 roundings on the way from an entry to the graph's cut (a row of <= 30 entries, 6 + 3
    steps of the tile's fold, 18 tiles): 64 * 2^-24 * sum |w|."""
    from gcn_max_cut_amd import maxcut
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as T
    g, nodes, classes, K = oversized_case(weights)
    n = g[0]
    assert n > pkg.hip.MAX_GRAPH_NODES and K + n - nodes.size <= pkg.hip.MAX_GRAPH_NODES and np.diff(g[1]).max() <= 30
    ei, ptr, w = edge_arrays([g])
    kw = dict(number_classes=K, hidden_dim=8, epochs=3, learning_rate=2e-2, samples=2, anneal_sweeps=3,
              max_descent_sweeps=5, seed=4)
    res = maxcut.solve(ei, ptr, edge_weight=w, fixed=(nodes, classes), **kw)
    part = res.partition.cpu().numpy()
    assert part.shape == (n,) and np.array_equal(part[nodes], classes) and res.ptr.cpu().tolist() == [0, n]
    batch = pkg.GraphBatch.from_edge_index(ei, ptr, edge_weight=w)
    ct = batch.contract(nodes, classes, K)
    assert ct.batch.n_max == K + n - nodes.size
    inner = maxcut.solve_batch(ct.batch, terminals=True, **kw)
    assert torch.equal(ct.lift(inner.partition), res.partition) and torch.equal(res.fixed_cut, ct.fixed_cut)
    cut, trained, rounded = (float(t.cpu()[0]) for t in (res.cut, res.trained_cut, res.rounded_cut))
    exact = float(CR.cut_of(g, part)[0])
    print(f"{weights}: cut {cut!r} trained {trained!r} rounded {rounded!r} float64 recount {exact!r} fixed_cut "
          f"{res.fixed_cut.cpu().tolist()} contracted cut {inner.cut.cpu().tolist()}")
    if weights == "unit":
        assert cut == exact and cut >= trained and cut >= rounded
        for name in ("cut", "trained_cut", "rounded_cut"):
            assert torch.equal(getattr(inner, name) + ct.fixed_cut, getattr(res, name)), name
    else:
        total = float(np.abs(g[3].astype(np.float64)).sum()) / 2
        assert abs(cut - exact) <= 64 * 2.0 ** -24 * total
        handle = pkg.GraphHandle(*g)
        assert cut == float(T.large_local_search(part.tolist(), handle, K, max_sweeps=0, terminals=False)[1])


def test_solve_refuses_a_contraction_that_is_still_too_large(pkg):
    from gcn_max_cut_amd import maxcut
    g, nodes, classes, K = oversized_case("unit")
    ei, ptr, w = edge_arrays([g])
    few = np.concatenate([nodes[classes == c][:1] for c in range(K)])  # one pin per class: 4,500 nodes stay
    with pytest.raises(ValueError, match="a graph of 4500 nodes is beyond the one-workgroup head"):
        maxcut.solve(ei, ptr, fixed=(few, np.arange(K)), number_classes=K, hidden_dim=8, epochs=1, learning_rate=0.1)


def test_narrow_torch_dtypes_are_taken(pkg):
    name = "third_pinned_b5"
    gs, pins, K = case(name)
    batch, _ei, ptr, _w = original(pkg, name)
    nodes, classes = pin_arrays(pins, ptr, 5)
    assert nodes.max() < 1 << 15
    for node_type, class_type in ((torch.int16, torch.uint8), (torch.int64, torch.int8), (torch.int16, torch.int16)):
        got = batch.contract(torch.from_numpy(nodes).to(node_type), torch.from_numpy(classes).to(class_type).cuda(), K)
        same_contraction(got, wanted(pkg, name), f"{name} {node_type} {class_type}")
    with pytest.raises(ValueError, match=r"1 pins with a class outside 0\.\.2"):
        batch.contract(torch.from_numpy(nodes), torch.from_numpy(np.where(np.arange(nodes.size) == 0, 200, classes)).to(torch.uint8), K)
