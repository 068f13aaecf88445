"""CPU restatement of the sampler and the annealing for graphs of up to 2^20 nodes (include/gcnmaxcut.h:
gmc_large_sample_seeded_f32, gmc_large_anneal_f32), and the cases their tests share.

The rule is that of tests/kway_search_ref.py (``anneal``, ``refine``, ``assignments``); what is new is the counter of
the move test, chosen by the graph's node count (``wide``): ``cand << 32 | s << 12 | v`` up to 4096 nodes - the
one-workgroup kernel's, whose 12-bit node field would make node v of sweep s share its hash with node v - 4096 of sweep
s + 1 beyond them - and ``cand << 40 | s << 20 | v`` for larger graphs.

``anneal`` takes all nodes of a colour class and all candidates at once through the padded neighbour tables of
tests/large_round_ref.py (a class split by degree, a loop over the edge POSITION so that every row's float32 sums are
taken in CSR order): a million nodes in seconds.  No two nodes of a class are adjacent, so the class-parallel form
equals ``sequential``, the plain one-node-at-a-time form that serves as the definition.  Cuts are counted in float64
and rounded to fp32 once: for unit, integer and dyadic weights that is the value any fp32 summation order gives, so
snapshot decisions are bit for bit the device's there (and only there)."""
import functools

import numpy as np

from tests import anneal_ref as AR
from tests import kway_search_ref as KS
from tests import large_ref as LR
from tests import large_round_ref as LRR
from tests import refine_ref as RR

F32 = np.float32
INF = F32(np.inf)
U = np.uint64
SMALL_NODES = 4096      # GMC_MAX_GRAPH_NODES


# ---- the counter ------------------------------------------------------------------------------------------------------
def wide(n):
    """Does a graph of n nodes take the 20-bit node and sweep fields?"""
    return n > SMALL_NODES


def counter(cand, s, v, wide_layout):
    """ctr of candidate cand, sweep s, local node v (Python integers)."""
    return (cand << 40) | (s << 20) | v if wide_layout else (cand << 32) | (s << 12) | v


def level_index(seed, cand, s, v, wide_layout):
    return AR.mix64_int(seed + AR.GOLD * (counter(cand, s, v, wide_layout) + 1)) >> 54


def level_indices(seed, cand_ids, s, nodes, wide_layout):
    """level_index for every (candidate, node): [cands, m] int64."""
    c = np.asarray(cand_ids, U)[:, None]
    v = np.asarray(nodes, U)[None, :]
    ctr = (c << U(40)) | U(s << 20) | v if wide_layout else (c << U(32)) | U(s << 12) | v
    with np.errstate(over="ignore"):
        h = AR._mix64(U(seed & AR.M64) + U(AR.GOLD) * (ctr + U(1)))
    return (h >> U(54)).astype(np.int64)


# ---- the search -------------------------------------------------------------------------------------------------------
def groups_of(n, rowptr, col, w, K, classes=None):
    """The (nodes, neighbour ids, weights) tables of the graph in colour order (large_round_ref.class_tables, flat:
    the nodes of a class are independent, so the groups of a class may be visited one after the other)."""
    if classes is None:
        classes = LRR.colouring(n, rowptr, col, K)
    return [grp for groups in LRR.class_tables(n, rowptr, col, w, classes) for grp in groups]


def descent(A, groups, K, max_sweeps):
    """kway_search_ref.refine over the padded state A [cands, n + 1] (in place): the sweeps run per candidate."""
    cands = A.shape[0]
    sweeps = np.zeros(cands, np.int64)
    active = np.ones(cands, bool)
    for _ in range(max_sweeps):
        if not active.any():
            break
        sweeps[active] += 1
        moved = np.zeros(cands, bool)
        for nodes, nb, wt in groups:
            W = KS._sums(A[active], nb, wt, K)
            c = A[np.ix_(active, nodes)]
            _own, wc = KS._own(W, c, K)
            kk = W.argmin(axis=0)                              # the first smallest: lowest index on ties
            move = np.take_along_axis(W, kk[None], 0)[0] < wc
            A[np.ix_(active, nodes)] = np.where(move, kk.astype(np.int8), c)
            moved[active] |= move.any(axis=1)
        active &= moved
    return sweeps


def anneal(n, rowptr, col, w, assign, K, inv_temp, table, seed, max_descent_sweeps, cand_ids=None, groups=None,
           wide_layout=None):
    """assign [cands, n] int8 -> (annealed [cands, n] int8, snap_sweep [cands], descent sweeps [cands]).
    wide_layout: the counter layout (default: the one a graph of n nodes takes)."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    if wide_layout is None:
        wide_layout = wide(n)
    if groups is None:
        groups = groups_of(n, rowptr, col, w, K)
    cands = assign.shape[0]
    cand_ids = np.arange(cands) if cand_ids is None else np.asarray(cand_ids)
    A = KS._padded(np.asarray(assign, np.int8), n)
    best = A.copy()
    snap = np.zeros(cands, np.int64)
    if len(inv_temp):
        best_cut = AR.cuts_f32(rowptr, col, w, A[:, :n])
    for s, inv_t in enumerate(np.asarray(inv_temp, F32)):
        for nodes, nb, wt in groups:
            W = KS._sums(A, nb, wt, K)
            c = A[:, nodes]
            own, wc = KS._own(W, c, K)
            others = np.where(own, INF, W)                     # a byte of no class masks nothing: the smallest of all
            kk = others.argmin(axis=0)
            wk = np.take_along_axis(others, kk[None], 0)[0]
            delta = wk - wc
            lvl = table[level_indices(seed, cand_ids, s, nodes, wide_layout)]
            move = (delta < 0) | (delta * inv_t <= lvl)
            A[:, nodes] = np.where(move, kk.astype(np.int8), c)
        cs = AR.cuts_f32(rowptr, col, w, A[:, :n])
        better = cs > best_cut
        best[better] = A[better]
        best_cut[better] = cs[better]
        snap[better] = s + 1
    sweeps = descent(best, groups, K, max_descent_sweeps)
    return best[:, :n].copy(), snap, sweeps


def sequential(n, rowptr, col, w, assign, K, inv_temp, table, seed, max_descent_sweeps, cand=0, wide_layout=None):
    """The definition, for a single assignment (list): one node at a time in (colour, id) order.
    Returns (assignment list, snap_sweep, descent sweeps)."""
    if wide_layout is None:
        wide_layout = wide(n)
    a = [int(x) for x in assign]
    classes = [c.tolist() for c in LRR.colouring(n, rowptr, col, K)]
    best, snap = list(a), 0
    if len(inv_temp):
        best_cut = F32(RR.cut(rowptr, col, w, a))
    for s, inv_t in enumerate(inv_temp):
        for cls in classes:
            for v in cls:
                W = KS._node_sums(rowptr, col, w, a, v, K)
                c = a[v]
                if 0 <= c < K:
                    k = min((i for i in range(K) if i != c), key=lambda i: (W[i], i))
                    delta = F32(W[k] - W[c])
                    if delta < 0 or F32(delta * F32(inv_t)) <= table[level_index(seed, cand, s, v, wide_layout)]:
                        a[v] = k
                else:
                    a[v] = min(range(K), key=lambda i: (W[i], i))
        cs = F32(RR.cut(rowptr, col, w, a))
        if cs > best_cut:
            best, best_cut, snap = list(a), cs, s + 1
    a, sweeps = best, 0
    while sweeps < max_descent_sweeps:
        sweeps += 1
        nxt = KS.sequential_sweep(n, rowptr, col, w, a, K, classes)
        if nxt == a:
            break
        a = nxt
    return a, snap, sweeps


def search(n, rowptr, col, w, assign, K, inv_temp, table, seed, max_descent_sweeps, groups=None):
    """What gmc_large_anneal_f32 reports for one graph: assign [cands, n] int8, cut_all [cands] float32, snap, sweeps,
    best_assign [n] int32, best_cut, best_idx (the strictly best, the first on ties)."""
    out, snap, sweeps = anneal(n, rowptr, col, w, assign, K, inv_temp, table, seed, max_descent_sweeps, groups=groups)
    cut_all = AR.cuts_f32(np.asarray(rowptr, np.int64), np.asarray(col, np.int64), w, out)
    bi = int(np.argmax(cut_all))
    return dict(assign=out, cut_all=cut_all, snap=snap.astype(np.int32), sweeps=sweeps.astype(np.int32),
                best_assign=out[bi].astype(np.int32), best_cut=cut_all[bi], best_idx=bi)


# ---- the sampler ------------------------------------------------------------------------------------------------------
def sample(n, rowptr, col, w, P, key, iters):
    """kway_search_ref.sample for a numpy CSR of any size (the cut count vectorised)."""
    a = KS.assignments(np.asarray(P, F32)[:n], key, iters)
    cut_all = AR.cuts_f32(np.asarray(rowptr, np.int64), np.asarray(col, np.int64), w, a)
    bi = int(np.argmax(cut_all))
    return dict(assign_all=a, cut_all=cut_all, best_assign=a[bi].astype(np.int32), best_cut=cut_all[bi], best_iter=bi)


# ---- cases beyond 4096 nodes ------------------------------------------------------------------------------------------
def integer_edge_weights(n, rowptr, col, seed):
    """float32 weights in {1, 2, 3, -1}, one per undirected edge (both directions the same value): every fp32 sum of
    them is exact in any order."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    key = np.minimum(rows, col) * n + np.maximum(rows, col)
    uniq, inv = np.unique(key, return_inverse=True)
    return np.random.RandomState(500 + seed).choice(np.asarray([1, 2, 3, -1], F32), uniq.size)[inv].astype(F32)


SEED = 11               # the annealing seed of every case below
# name -> (K, graph spec of large_round_ref.build_graph, weights, candidates, annealing sweeps, descent sweeps)
BIG_CASES = {
    "n4097_K2": (2, ("circ", 4097, 7, 6), "integer", 5, 6, 20),
    "n4097_K8": (8, ("circ", 4097, 7, 6), "unit", 3, 6, 20),
    "n5000_K3": (3, ("circ", 5000, 7, 7), "integer", 9, 5, 20),
    "star4200": (3, ("star", 4200, 5), "unit", 3, 4, 10),
    "hubring4200": (4, ("hubring", 4201, 9), "integer", 3, 4, 10),
    "n70000": (4, ("circ", 70000, 7, None), "unit", 3, 3, 5),
    "n2^20": (3, ("circ", 1 << 20, 4, None), "unit", 2, 2, 3),
}
SCHEDULE = dict(t_start=0.8, t_end=0.3)   # warm enough to accept uphill moves, cool enough to find better cuts


def schedule(sweeps):
    return AR.schedule(sweeps, **SCHEDULE)


def candidates(n, K, cands, seed):
    """[cands, n] int8: random classes, the terminals in place, two bytes of no class on movable nodes of candidate 0."""
    A = np.random.RandomState(seed).randint(0, K, (cands, n)).astype(np.int8)
    A[:, :K] = np.arange(K, dtype=np.int8)
    if n > K + 2:
        A[0, n - 1], A[0, K + 1] = K, -1
    return A


@functools.lru_cache(maxsize=None)
def big_case(name):
    """(K, n, rowptr, col, w, A [cands, n], inv_temp, descent sweeps, groups) of a case beyond 4096 nodes."""
    K, spec, weights, cands, sweeps, max_descent = BIG_CASES[name]
    n, rowptr, col = LRR.build_graph(spec)
    seed = sum(map(ord, name))
    w = integer_edge_weights(n, rowptr, col, seed) if weights == "integer" else None
    A = candidates(n, K, cands, seed + 2)
    A.setflags(write=False)
    return K, n, rowptr, col, w, A, schedule(sweeps), max_descent, groups_of(n, rowptr, col, w, K)


@functools.lru_cache(maxsize=None)
def big_reference(name):
    """The restatement of a big case, computed once and shared."""
    K, n, rowptr, col, w, A, inv_t, max_descent, groups = big_case(name)
    ref = search(n, rowptr, col, w, A, K, inv_t, AR.levels(), SEED, max_descent, groups=groups)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def mixed_batch():
    """Graphs of 300 / 4097 / 5000 nodes: both counter layouts in one call."""
    return [LR.circulant(300, 5, 3), LR.circulant(4097, 7, 6), LR.circulant(5000, 6, 2)]


@functools.lru_cache(maxsize=None)
def condition_case(K):
    """(handle, A [6, n], inv_temp) of a 200-node graph whose candidates 0..2 are random and 3..5 local optima (the
    descent of random ones), annealed hot: the random ones find better cuts on the way (snap_sweep > 0), a local optimum
    only loses (snap_sweep == 0)."""
    from oracle import ref_dense as R
    from tests.test_refine_host import handles_of
    h = handles_of([R.regular_graph(200, 5, 77 + K)])[0]
    A = candidates(h.n, K, 6, 31 + K)
    A[0, h.n - 1], A[0, K + 1] = 0, K - 1
    A[3:], _sweeps = KS.refine(h.n, h.rowptr, h.col, h.weight, A[3:], K, 100)
    A.setflags(write=False)
    return h, A, AR.schedule(6, t_start=2.0, t_end=1.0)
