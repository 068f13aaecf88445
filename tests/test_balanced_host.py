"""CPU checks of the tabu search under class-size bounds (include/gcnmaxcut.h, gmc_kway_balance_f32): the restatement
tests/balanced_ref.py against brute force on tiny graphs and against tests/tabu_ref.py under loose bounds, the repair,
the bridge graph, the host-side errors of the Python API (no GPU needed), the status codes of the three entry points
and gmc_kway_balance_fits / gmc_kway_balance_shape against the layout formula."""
import ctypes as C
import functools
import itertools
import os

import networkx as nx
import numpy as np
import pytest

from oracle import ref_dense as R
from tests import balanced_ref as BR
from tests import tabu_ref as TR
from tests import util
from tests.test_refine_host import gnp_graph, handles_of, loop_graph
from tests.test_tabu_host import NULL, SOME, int_weighted, lds_shape, mk, start


def feasible(a, K, lo, hi):
    s = np.array([(np.asarray(a) == c).sum() for c in range(K)])
    return bool(((s >= lo) & (s <= hi)).all())


# ---- optimality on tiny graphs -------------------------------------------------------------------------------------
# 42 drawn cases: G(n, 0.5), K = 2, 3, 4 in turn, n = 8..11 (8, 9 at K = 4 without terminals: 4^9 states), terminals on
# and off, unit / integer 1..5 / all-negative weights, the exact bounds floor and ceil of n / K; 4 chains of 20 n
# iterations, chain 0 from every node in class 0 (the terminals in their own), the others from random classes.
DRAWN = 42
AT_LEAST = 38   # 90 % of 42, rounded up


def drawn_case(index):
    K = (2, 3, 4)[index % 3]
    t = (index // 3) % 2 == 1
    n = 8 + index % 4 if (K < 4 or t) else 8 + index % 2
    kind = ("unit", "int", "negative")[(index // 6) % 3]
    g = gnp_graph(n, 0.5, 300 + index)
    rng = np.random.RandomState(index)
    for u, v in g.edges():
        g[u][v]["weight"] = {"unit": 1, "int": int(rng.randint(1, 6)), "negative": -int(rng.randint(1, 4))}[kind]
    return g, n, K, t


def constrained_optimum(h, K, first, lo, hi):
    rows = np.repeat(np.arange(h.n), np.diff(h.rowptr))
    tail = np.array(list(itertools.product(range(K), repeat=h.n - first)), np.int8)
    full = np.concatenate([np.tile(np.arange(first, dtype=np.int8), (tail.shape[0], 1)), tail], axis=1)
    ok = np.ones(full.shape[0], bool)
    for c in range(K):
        s = (full == c).sum(axis=1)
        ok &= (s >= lo[c]) & (s <= hi[c])
    full = full[ok]
    w = np.ones(h.col.size) if h.weight is None else np.asarray(h.weight, np.float64)
    return float((((full[:, rows] != full[:, h.col]) * w[None, :]).sum(axis=1) / 2).max())


@functools.lru_cache(maxsize=None)
def tiny_outcomes():
    out = []
    for index in range(DRAWN):
        g, n, K, t = drawn_case(index)
        h = handles_of([g])[0]
        first = K if t else 0
        lo, hi = BR.balanced_bounds(n, K)
        assert BR.admits(lo, hi, n, t)
        cuts = []
        for chain in range(4):
            a0 = np.zeros(n, np.int8) if chain == 0 else np.random.RandomState(10 * index + chain).randint(0, K, n).astype(np.int8)
            a0[:first] = np.arange(first)
            res = BR.balanced(n, h.rowptr, h.col, h.weight, a0, K, t, chain, lo, hi, 20 * n, seed=300 + index)
            assert feasible(res.assign, K, lo, hi), (index, chain)
            assert (res.assign[:first] == np.arange(first)).all(), (index, chain)
            assert ((res.assign >= 0) & (res.assign < K)).all()
            cuts.append(TR.cut_f64(h.rowptr, h.col, h.weight, res.assign))
        out.append((max(cuts), constrained_optimum(h, K, first, lo, hi)))
    return out


def test_the_restatement_reaches_the_constrained_optimum_of_tiny_graphs():
    outcomes = tiny_outcomes()
    assert len(outcomes) == DRAWN >= 40 and AT_LEAST >= 0.9 * DRAWN
    assert all(got <= best for got, best in outcomes)                   # (brute force is an upper bound)
    reached = sum(got == best for got, best in outcomes)
    print("reached the constrained optimum on", reached, "of", DRAWN)
    assert reached >= AT_LEAST, [(i, o) for i, o in enumerate(outcomes) if o[0] != o[1]]


# ---- loose bounds: the tabu search ------------------------------------------------------------------------------------
LOOSE = {   # graph, K, terminals, iterations, tenure (base, span, div)
    "regular_k2": (lambda: R.regular_graph(60, 5, 1), 2, False, 200, (3, 0, 10)),
    "regular_k3_t": (lambda: R.regular_graph(60, 5, 2), 3, True, 200, (3, 0, 10)),
    "gnp_k8_t": (lambda: gnp_graph(40, 0.3, 3), 8, True, 150, (0, 0, 0)),
    "int_k4": (lambda: int_weighted(R.regular_graph(50, 6, 4), 4), 4, False, 200, (2, 5, 0)),
    "signed_k2": (lambda: int_weighted(R.regular_graph(50, 6, 5), 5, signed=True), 2, False, 200, (3, 0, 10)),
    "hub_loops_k3": (lambda: loop_graph(45, 4, 6), 3, True, 120, (1, 3, 7)),
    "long_tenure": (lambda: R.regular_graph(20, 3, 7), 2, False, 100, (50, 0, 0)),
}


@pytest.mark.parametrize("name", sorted(LOOSE))
def test_loose_bounds_give_the_tabu_search_byte_for_byte(name):
    make, K, t, iters, tenure = LOOSE[name]
    h = handles_of([make()])[0]
    a0 = start(h.n, K, t, 11)
    lo, hi = np.zeros(K, np.int64), np.full(K, h.n, np.int64)
    got = BR.balanced(h.n, h.rowptr, h.col, h.weight, a0, K, t, 2, lo, hi, iters, *tenure, seed=77, trace=True)
    ref = TR.tabu(h.n, h.rowptr, h.col, h.weight, a0, K, t, 2, iters, *tenure, seed=77)
    assert got.assign.tobytes() == ref.assign.tobytes()
    assert (got.best_it, got.moves, got.repairs) == (ref.best_it, ref.moves, 0)
    assert np.float32(got.best).tobytes() == np.float32(ref.best).tobytes()
    assert all(kind == "free" for *_x, kind in got.trace)


# ---- the repair -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terminals", (True, False))
@pytest.mark.parametrize("K", range(2, 9))
def test_repair_from_one_class(K, terminals):
    """Every movable node in class 0 under the exact bounds.  A repair move lowers V by 1 or by 2 and the repair ends at
    V = 0, so it takes between V / 2 and V moves and never fewer than the nodes class 0 has to lose; at K = 2 every move
    lowers both terms, V / 2 moves.  (The count is NOT V in general: the 2048 moves of 4096 nodes at K = 2 repair
    V = 4096.)  With iterations = 0 the output is the repaired state: the input with the traced moves applied."""
    n = 37 + K
    h = handles_of([R.regular_graph(n if n % 2 == 0 else n + 1, 5, K)])[0]
    n = h.n
    first = K if terminals else 0
    a0 = np.zeros(n, np.int8)
    a0[:first] = np.arange(first)
    lo, hi = BR.balanced_bounds(n, K)
    s, _m = BR.sizes(a0, K, first)
    V = BR.violation(s, lo, hi)
    res = BR.balanced(n, h.rowptr, h.col, h.weight, a0, K, terminals, 0, lo, hi, 0, trace=True)
    assert V > 0 and (V + 1) // 2 <= res.repairs <= V and res.repairs >= s[0] - hi[0]
    if K == 2:
        assert 2 * res.repairs == V
    assert res.moves == 0 and res.best_it == 0 and res.best == 0
    assert feasible(res.assign, K, lo, hi) and (res.assign[:first] == np.arange(first)).all()
    replay = a0.copy()
    for it, v, b, _gain, kind in res.trace:
        assert (it, kind) == (-1, "repair") and v >= first and replay[v] != b
        replay[v] = b
    assert (replay == res.assign).all() and len(res.trace) == res.repairs
    # the search that follows starts from that state: its first trace entries are the same repair moves
    longer = BR.balanced(n, h.rowptr, h.col, h.weight, a0, K, terminals, 0, lo, hi, 50, trace=True)
    assert longer.repairs == res.repairs and longer.trace[:res.repairs] == res.trace
    assert feasible(longer.assign, K, lo, hi)
    assert TR.cut_f64(h.rowptr, h.col, None, longer.assign) == TR.cut_f64(h.rowptr, h.col, None, res.assign) + float(longer.best)


def test_repair_leaves_a_feasible_input_alone():
    h = handles_of([R.regular_graph(40, 5, 2)])[0]
    for K, t in ((2, False), (4, True), (5, False)):
        a0 = (np.arange(40) % K).astype(np.int8)                        # classes of 40 / K or one more: feasible
        lo, hi = BR.balanced_bounds(40, K)
        assert feasible(a0, K, lo, hi)
        res = BR.balanced(40, h.rowptr, h.col, h.weight, a0, K, t, 0, lo, hi, 0)
        assert res.repairs == 0 and (res.assign == a0).all()
        res = BR.balanced(40, h.rowptr, h.col, h.weight, a0, K, t, 0, lo, hi, 100, trace=True)
        assert res.repairs == 0 and feasible(res.assign, K, lo, hi) and all(k != "repair" for *_x, k in res.trace)
        if 40 % K == 0:                                                 # lo = hi: no move is free
            assert {k for *_x, k in res.trace} == {"paired", "counter"}


# ---- the bridge graph -------------------------------------------------------------------------------------------------
def bridge_graph(weight=-1):
    g = nx.disjoint_union(nx.complete_graph(8), nx.complete_graph(8))
    g.add_edge(7, 8)
    for u, v in g.edges():
        g[u][v]["weight"] = weight
    return g


def bridge_starts():
    A = np.random.RandomState(5).randint(0, 2, (4, 16)).astype(np.int8)
    A[0] = 0
    return A


def test_the_bridge_of_two_cliques_is_found_from_every_start():
    """Weights -1 and an exact bisection: the balanced minimum cut.  Without the bound the answer is one class and cut 0."""
    h = handles_of([bridge_graph()])[0]
    lo, hi = BR.balanced_bounds(16, 2)
    for chain, a0 in enumerate(bridge_starts()):
        res = BR.balanced(16, h.rowptr, h.col, h.weight, a0, 2, False, chain, lo, hi, 20 * 16, seed=1)
        assert TR.cut_f64(h.rowptr, h.col, h.weight, res.assign) == -1.0, chain
        assert len(set(res.assign[:8])) == 1 and len(set(res.assign[8:])) == 1 and res.assign[0] != res.assign[8]
    free = TR.tabu(16, h.rowptr, h.col, h.weight, bridge_starts()[1], 2, False, 1, 320, seed=1)
    assert TR.cut_f64(h.rowptr, h.col, h.weight, free.assign) == 0.0


# ---- host errors ------------------------------------------------------------------------------------------------------
def test_bounds_that_admit_no_partition_raise_on_the_host():
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    g = R.regular_graph(12, 3, 1)
    part = [i % 3 for i in range(12)]
    bad = {"lo > hi": ([5, 2, 2], [4, 6, 6]), "lower sum": ([5, 5, 5], [6, 6, 6]), "upper sum": ([0, 0, 0], [4, 4, 3]),
           "terminal": ([0, 0, 0], [12, 0, 12])}
    for name, sizes in bad.items():
        with pytest.raises(ValueError, match="graph 0"):
            TN.kway_balanced_search(part, g, 3, class_sizes=sizes, terminals=True)
        assert not BR.admits(sizes[0], sizes[1], 12, True), name
    assert BR.admits([0, 0, 0], [12, 0, 12], 12, False)                 # hi = 0 is an empty class without terminals
    lo, hi = TN.class_size_bounds("t", ([0, 0, 0], [12, 0, 12]), [12], 3, False)
    assert lo.tolist() == [[0, 0, 0]] and hi.tolist() == [[12, 0, 12]] and lo.dtype == np.int32
    with pytest.raises(ValueError, match="admit no partition"):         # max(lo, t): the terminals need a node each
        TN.class_size_bounds("t", ([0, 0, 10], [12, 12, 12]), [11], 3, True)
    TN.class_size_bounds("t", ([0, 0, 10], [12, 12, 12]), [12], 3, True)
    with pytest.raises(ValueError, match="graph 1"):                    # per graph, and the graph is named
        TN.class_size_bounds("t", ([[4, 4], [4, 4]], [[5, 5], [5, 5]]), [9, 11], 2, False)
    for shape_bad in (([1, 2], [3, 4]), "even", ([4, 4, 4],), ([[4, 4, 4]] * 2, [[4, 4, 4]] * 2), ([4.0] * 3, [4.0] * 3), 4):
        with pytest.raises(ValueError, match="class_sizes"):
            TN.kway_balanced_search(part, g, 3, class_sizes=shape_bad)
    with pytest.raises(ValueError):
        TN.kway_balanced_search(part, g, 3, iterations=-1)
    with pytest.raises(ValueError):
        TN.kway_balanced_search(part + [0], g, 3)
    lo, hi = TN.class_size_bounds("t", "balanced", [12, 13, 7], 3, True)
    assert lo.tolist() == [[4] * 3, [4] * 3, [2] * 3] and hi.tolist() == [[4] * 3, [5] * 3, [3] * 3]


def test_solve_refuses_on_the_host():
    from gcn_max_cut_amd import maxcut
    ei = np.asarray([[0, 1, 1, 2, 2, 3], [1, 0, 2, 1, 3, 2]], np.int64)
    kw = dict(hidden_dim=8, epochs=1, learning_rate=0.01)
    with pytest.raises(ValueError, match="class_sizes with fixed"):
        maxcut.solve(ei, num_nodes=4, class_sizes="balanced", fixed=(np.asarray([0, 1]), np.asarray([0, 1])), **kw)
    with pytest.raises(ValueError, match="class_sizes with fixed"):
        maxcut.solve_batch(None, class_sizes="balanced", fixed=(np.asarray([0, 1]), np.asarray([0, 1])), **kw)
    with pytest.raises(ValueError, match="graph 0"):
        maxcut.solve(ei, num_nodes=4, class_sizes=([3, 3], [4, 4]), **kw)
    with pytest.raises(ValueError, match="graph 1"):
        maxcut.solve(ei, np.asarray([0, 2, 4]), class_sizes=([[1, 1], [2, 2]], [[1, 1], [2, 2]]), **kw)
    with pytest.raises(ValueError, match="class_sizes"):
        maxcut.solve(ei, num_nodes=4, class_sizes=([1, 1, 1], [2, 2, 2]), **kw)
    with pytest.raises(ValueError, match="balance_iterations"):
        maxcut.solve(ei, num_nodes=4, class_sizes="balanced", balance_iterations=-1, **kw)
    for route in (maxcut.solve_large, ):
        with pytest.raises(NotImplementedError, match="balanced"):
            route(ei, num_nodes=4, class_sizes="balanced", **kw)
    with pytest.raises(NotImplementedError, match="balanced"):
        maxcut.solve_large_batch(None, class_sizes="balanced", **kw)


def test_balanced_sizes():
    from gcn_max_cut_amd import maxcut
    lo, hi = maxcut.balanced_sizes([0, 10, 21, 1021], 2)
    assert lo.tolist() == [[5, 5], [5, 5], [500, 500]] and hi.tolist() == [[5, 5], [6, 6], [500, 500]]
    lo, hi = maxcut.balanced_sizes(np.asarray([0, 1000, 1100]), 2, 0.03)
    assert lo.tolist() == [[485, 485], [48, 48]] and hi.tolist() == [[515, 515], [52, 52]]
    lo, hi = maxcut.balanced_sizes([0, 10], 3, 0.5)
    assert lo.tolist() == [[1, 1, 1]] and hi.tolist() == [[5, 5, 5]] and lo.dtype == np.int32 and lo.shape == (1, 3)
    for n in range(2, 40):
        for K in range(2, 9):
            lo, hi = maxcut.balanced_sizes([0, n], K)
            blo, bhi = BR.balanced_bounds(n, K)
            assert lo[0].tolist() == blo.tolist() and hi[0].tolist() == bhi.tolist()
    with pytest.raises(ValueError):
        maxcut.balanced_sizes([0, 10], 9)
    with pytest.raises(ValueError):
        maxcut.balanced_sizes([0, 10], 2, -0.1)


# ---- the entry points without a GPU --------------------------------------------------------------------------------
def test_status_codes_of_the_balanced_search(built):
    hip = built.hip
    lib = hip.load()
    assert {"gmc_kway_balance_f32", "gmc_kway_balance_fits", "gmc_kway_balance_shape"} <= set(hip.SYMBOLS)

    def f(batch, K=4, t=1, cands=4, assign=SOME, size_lo=SOME, size_hi=SOME, iterations=10, base=3, span=0, div=10,
          cut_all=SOME, best_assign=SOME, best_cut=SOME, best_idx=SOME, best_iter=SOME, moves=SOME, repairs=SOME,
          feasible=SOME):
        b = None if batch is None else C.byref(batch)
        return lib.gmc_kway_balance_f32(b, K, t, cands, assign, size_lo, size_hi, iterations, base, span, div, 7, cut_all,
                                        best_assign, best_cut, best_idx, best_iter, moves, repairs, feasible, None)
    b = mk(hip)
    assert f(None) == -1
    for name in ("assign", "size_lo", "size_hi", "cut_all", "best_assign", "best_cut", "best_idx"):
        assert f(b, **{name: NULL}) == -1, name
    assert f(mk(hip, abi=100)) == -8 and f(mk(hip, abi=100), size_lo=NULL) == -1   # the order: NULL, then the abi word
    for field in ("goff", "rowptr", "lcol"):
        assert f(mk(hip, **{field: None})) == -1, field
        assert f(mk(hip, abi=100, **{field: None})) == -8              # ... then the batch's arrays
    for K in (1, 9, 0, -3):
        assert f(b, K=K) == -3, K
        assert f(b, K=K, cands=0) == -3 and f(b, K=K, iterations=-1) == -3   # ... then the class count
        assert f(mk(hip, lcol=None), K=K) == -1
    for kw in (dict(cands=0), dict(cands=-1), dict(iterations=-1), dict(iterations=-(1 << 31)), dict(base=-1),
               dict(span=-1), dict(div=-1), dict(t=2), dict(t=-1)):
        assert f(b, **kw) == -2, kw                                     # ... then the shape
        assert f(mk(hip, n_max=3), **kw) == -2                          # ... before the graph size
    assert f(mk(hip, B=-1)) == -2
    assert f(mk(hip, n_max=3)) == -6 and f(mk(hip, n_max=4097)) == -6 and f(mk(hip, n_max=0), t=0) == -6
    assert f(mk(hip, n_max=2), K=3) == -6
    empty = hip.GmcBatch(B=0, goff=4096, rowptr=4096, lcol=4096)
    for K in range(2, 9):
        for t in (0, 1):
            assert f(empty, K=K, t=t) == 0
            assert f(empty, K=K, t=t, iterations=0, best_iter=NULL, moves=NULL, repairs=NULL, feasible=NULL) == 0
        assert f(mk(hip, n_max=K - 1), K=K) == -6
    assert f(empty, iterations=(1 << 31) - 1, base=(1 << 31) - 1, span=(1 << 31) - 1, div=(1 << 31) - 1) == 0
    assert f(empty, cands=0) == -2 and f(empty, K=9) == -3 and f(empty, size_hi=NULL) == -1


def test_fits_and_shape_are_the_tabu_searchs(built):
    hip = built.hip
    lib = hip.load()
    for K in (2, 8):
        q = lambda **kw: lib.gmc_kway_balance_fits(C.byref(hip.GmcBatch(**kw)), K)
        assert q(n_max=1) == 1 and q(n_max=4096, nnz_max=1 << 24) == 1 and q(n_max=4097) == 0 and q(n_max=0) == 0
        assert q(n_max=4096, vals=4096) == 1
        assert lib.gmc_kway_balance_fits(None, K) == -1 and q(n_max=10, abi=100) == -8
        assert lib.gmc_kway_balance_shape(C.byref(hip.GmcBatch(n_max=4097)), K) == -6
        assert lib.gmc_kway_balance_shape(None, K) == -1
    assert lib.gmc_kway_balance_fits(C.byref(hip.GmcBatch(n_max=10)), 9) == -3
    assert lib.gmc_kway_balance_shape(C.byref(hip.GmcBatch(n_max=10)), 1) == -3
    seen = set()
    for K in range(2, 9):
        for n_max, nnz_max in ((1, 0), (100, 700), (1000, 7000), (600, 180000), (2000, 14000), (4096, 12288), (4096, 28672),
                               (1100, 7700), (2100, 14700), (800, 38352)):
            for vals in (None, 4096):
                batch = hip.GmcBatch(n_max=n_max, nnz_max=nnz_max, vals=vals)
                got = lib.gmc_kway_balance_shape(C.byref(batch), K)
                slots, staged = lds_shape(K, n_max, nnz_max, vals is not None)   # n_pad * (4 K + 6) per chain: tabu's
                assert got == (slots | staged << 4) == lib.gmc_kway_tabu_shape(C.byref(batch), K), (K, n_max, nnz_max, vals)
                seen.add((slots, staged))
    assert seen == {(s, g) for s in (4, 2, 1) for g in (0, 1)}


def test_header_states_the_rule():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gcnmaxcut.h")).read()
    for text in ("int gmc_kway_balance_f32(", "int gmc_kway_balance_fits(", "int gmc_kway_balance_shape(",
                 "s[a] > lo[a] and s[b] < hi[b]", "m[b] >= 1", "da + db < 0", "sum of max(lo[c], t) <= n <= sum of hi[c]"):
        assert text in header, text


def test_every_instantiation_is_in_the_code_object(built):
    names = util.kernel_symbols(built.hip.LIB_PATH)
    for K in range(2, 9):
        assert sum(f"balance_kernel<{K}>" in s for s in names) == 1, K
        assert sum(f"balance_pick_kernel<{K}>" in s for s in names) == 1, K
        assert sum(f"tabu_kernel<{K}>" in s for s in names) == 1, K     # the shared header took nothing from it


def test_no_instantiation_uses_scratch(built):
    """The sizes and bounds are wave-uniform registers and the tables are LDS: the code object's own notes say that no
    instantiation has a private segment or spills a register to memory."""
    import subprocess
    seen = 0
    for co in util.gfx950_code_objects(built.hip.LIB_PATH):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            if "balance_" not in entry or ".name:" not in entry:
                continue
            fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith(".") and ":" in l)
            if "balance_kernel" not in fields.get(".name", "") and "balance_pick_kernel" not in fields.get(".name", ""):
                continue
            seen += 1
            assert int(fields[".private_segment_fixed_size"]) == 0, fields[".name"]
            assert int(fields[".vgpr_spill_count"]) == 0 and int(fields[".sgpr_spill_count"]) >= 0, fields[".name"]
    assert seen == 14                                                   # K = 2..8, the chains and the pick
