"""CPU restatement of parallel tempering over decoded partitions (include/gcnmaxcut_temper.h, gmc_kway_temper_f32),
written from the header's text in numpy float32: the rungs and the exchange test, the sweeps at each slot's own inverse
temperature, the best-state rule, and the scores in the device's own summation order (so they hold bit for bit for
real-valued weights and costs).

The sweep is tests/kway_search_ref.py's class-parallel form over all candidates of a graph at once (its ``_own`` and
``_padded``, the level indices of tests/anneal_ref.py, the class tables of tests/refine_ref.py, the colouring of
tests/plain_ref.py) with the class sums started from the cost rows as tests/node_cost_ref.py starts them; the score is
node_cost_ref's ``score`` - rows per thread, the wave's butterfly, the four wave sums - taken for every candidate at
once (tests/test_temper_host.py holds the two forms against each other).

Also here: the graphs, states and costs the CPU and GPU tests of the stage share."""
import functools

import numpy as np

from tests import anneal_ref as AR
from tests import kway_search_ref as KS
from tests import node_cost_ref as NC
from tests import plain_ref as PR
from tests import refine_ref as RR

F32 = np.float32
INF = F32(np.inf)
TAG = 0x54454D5045523031        # GMC_TEMPER_TAG
GOLD = AR.GOLD
M64 = AR.M64
THREADS = NC.THREADS


# ---- the scores of all candidates, in the kernel's fp32 order ------------------------------------------------------------
def _reduce(acc):
    """[cands, 256] per-thread sums -> [cands]: the butterfly per wave of 64, then ((q0 + q1) + q2) + q3."""
    v = acc.reshape(acc.shape[0], 4, 64).astype(F32, copy=True)
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lanes ^ d]
    q = v[:, :, 0]
    return ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]


def scores(n, rowptr, col, w, cost, A, K):
    """node_cost_ref.score of every row of A [cands, n] int8: float32 [cands]."""
    A = np.asarray(A, np.int8)
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    cands = A.shape[0]
    acc = np.zeros((cands, THREADS), F32)
    cst = np.zeros((cands, THREADS), F32)
    for lo in range(0, n, THREADS):
        rows = np.arange(lo, min(lo + THREADS, n))
        t = rows - lo
        deg = rowptr[rows + 1] - rowptr[rows]
        me = A[:, rows]
        for j in range(int(deg.max()) if rows.size else 0):
            live = deg > j
            e = np.where(live, rowptr[rows] + j, 0)
            we = np.ones(rows.size, F32) if w is None else np.asarray(w, F32)[e]
            add = np.where((A[:, col[e]] != me) & live[None, :], we[None, :], F32(0))
            acc[:, t] = acc[:, t] + add
        if cost is not None:
            ok = (me >= 0) & (me < K)
            c = np.asarray(cost, F32)[rows[None, :], np.where(ok, me, 0)]
            cst[:, t] = cst[:, t] + np.where(ok, c, F32(0))
    cut = _reduce(acc) * F32(0.5)
    return cut if cost is None else (cut - _reduce(cst)).astype(F32)


# ---- the sweep ---------------------------------------------------------------------------------------------------------
def _sums(A, nb, wt, K, cost_rows):
    """kway_search_ref._sums with the sums started from the nodes' cost rows (cost_rows [m, K] or None)."""
    W = np.zeros((K, A.shape[0], nb.shape[0]), F32)
    if cost_rows is not None:
        W += np.asarray(cost_rows, F32).T[:, None, :]
    for j in range(nb.shape[1]):
        cls = A[:, nb[:, j]]
        for k in range(K):
            W[k] += np.where(cls == k, wt[:, j], F32(0))
    return W


def tables_of(n, rowptr, col, w, first):
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    return [(cls, *RR._class_tables(n, rowptr, col, w, cls)) for cls in PR.colouring(n, rowptr, col, first)]


def sweep(A, tables, cost, K, inv_t, table, seed, s, cand_ids):
    """One sweep of the annealing's step 2 on A [cands, n + 1] (kway_search_ref._padded), in place; inv_t [cands]."""
    inv_t = np.asarray(inv_t, F32)[:, None]
    for nodes, nb, wt in tables:
        W = _sums(A, nb, wt, K, None if cost is None else cost[nodes])
        c = A[:, nodes]
        own, wc = KS._own(W, c, K)
        others = np.where(own, INF, W)
        kk = others.argmin(axis=0)
        wk = np.take_along_axis(others, kk[None], 0)[0]
        wk = np.where(own.any(axis=0), wk, F32(0))          # a byte of no class: delta = 0 - inf, the move is taken
        with np.errstate(invalid="ignore"):
            delta = (wk - wc).astype(F32)
            lvl = table[AR.level_indices(seed, cand_ids, s, nodes)]
            move = (delta < 0) | ((delta * inv_t).astype(F32) <= lvl)
        A[:, nodes] = np.where(move, kk.astype(np.int8), c)


# ---- the exchange --------------------------------------------------------------------------------------------------------
def exchange_hash(seed, t, copy, p):
    E = AR.mix64_int((seed & M64) ^ TAG)
    return AR.mix64_int(E + GOLD * ((((t << 40) | (copy << 8) | p) + 1) & M64))


def exchange(rung, x, rungs, ladder, table, seed, t):
    """Step 1 of round t > 0 for one graph: rung [cands] and x [cands] float32 after round t - 1 -> (new rung, swapped
    [cands] bool, proposals made)."""
    ladder = np.asarray(ladder, F32)
    new, swapped, proposals = rung.copy(), np.zeros(rung.size, bool), 0
    for copy in range(rung.size // rungs):
        base = copy * rungs
        slot_of = {int(r): base + j for j, r in enumerate(rung[base:base + rungs])}
        for p in range(t & 1, rungs - 1, 2):
            lo, hi = slot_of[p], slot_of[p + 1]
            d = F32(F32(ladder[p + 1] - ladder[p]) * F32(x[hi] - x[lo]))
            h = exchange_hash(seed, t, copy, p)
            proposals += 1
            if d < 0 or d <= table[h >> 54]:
                new[lo], new[hi] = p + 1, p
                swapped[lo] = swapped[hi] = True
    return new, swapped, proposals


# ---- the call, one graph ---------------------------------------------------------------------------------------------------
def temper(n, rowptr, col, w, cost, state, K, first, rungs, ladder, rounds, round_sweeps, table, seed, trace=None):
    """state [cands, n] int8 -> dict of what gmc_kway_temper_f32 leaves for one graph: state, best [cands, n] int8,
    best_score float32, best_round, rung, swaps int32 [cands]; and `proposals`, the exchanges tested.  trace: a list
    that receives the rungs after every round."""
    state = np.asarray(state, np.int8)
    cands = state.shape[0]
    assert cands % rungs == 0
    cost = None if cost is None else np.asarray(cost, F32)
    ladder = np.asarray(ladder, F32)
    tables = tables_of(n, rowptr, col, w, first)
    ids = np.arange(cands)
    A = KS._padded(state, n)
    rung = (ids % rungs).astype(np.int32)
    swaps = np.zeros(cands, np.int32)
    x = scores(n, rowptr, col, w, cost, A[:, :n], K)
    best, best_score, best_round = A.copy(), x.copy(), np.zeros(cands, np.int32)
    proposals = 0
    for t in range(rounds):
        if t > 0:
            rung, swapped, made = exchange(rung, x, rungs, ladder, table, seed, t)
            swaps += swapped
            proposals += made
        if trace is not None:
            trace.append(rung.copy())
        for j in range(round_sweeps):
            sweep(A, tables, cost, K, ladder[rung], table, seed, t * round_sweeps + j, ids)
            x = scores(n, rowptr, col, w, cost, A[:, :n], K)
            better = x > best_score
            best[better] = A[better]
            best_score[better] = x[better]
            best_round[better] = t
    return dict(state=A[:, :n].copy(), best=best[:, :n].copy(), best_score=best_score.astype(F32), best_round=best_round,
                rung=rung.astype(np.int32), swaps=swaps, proposals=proposals)


# ---- what the CPU and the GPU tests share ----------------------------------------------------------------------------------
def big_colour_graph(leaves=300):
    """Two centres joined to each other and to every leaf: the leaves are one colour class of more than 256 nodes, and
    both centre rows have more than 64 entries."""
    n = leaves + 2
    rowptr, col = [0], []
    for v in range(n):
        col.extend([u for u in range(n) if u != v] if v < 2 else [0, 1])
        rowptr.append(len(col))
    return n, np.asarray(rowptr, np.int64), np.asarray(col, np.int64)


def symmetric(n, rowptr, col, draw):
    """Weights on the entries of a CSR, one draw per undirected edge."""
    w, at = np.zeros(len(col), F32), {}
    for v in range(n):
        for e in range(int(rowptr[v]), int(rowptr[v + 1])):
            key = (min(int(col[e]), v), max(int(col[e]), v))
            if key not in at:
                at[key] = draw()
            w[e] = at[key]
    return w


def weights_of(kind, n, rowptr, col, seed):
    rng = np.random.RandomState(seed)
    if kind == "unit":
        return None
    if kind == "signed":
        return symmetric(n, rowptr, col, lambda: float(rng.choice([-2, -1, 1, 2, 3])))
    assert kind == "real"
    return symmetric(n, rowptr, col, lambda: float(F32(rng.uniform(0.1, 2.0) * (1.0 + 2.0 ** -20))))


@functools.lru_cache(maxsize=None)
def mixed_graphs(kind, K, terminals):
    """The mixed batch as (rowptr, col, w) per graph: n = 5 (below `first` at K = 8 with terminals: skipped), 37 and 130
    (rings with chords), a star whose centre row has 70 entries, the graph with a colour class of 300 nodes, and a graph
    of 1 node with terminals (below `first`, skipped) or 3 nodes without."""
    out = []
    for i, (n, rp, cl) in enumerate((PR.ring_with_chords(5, 1), PR.ring_with_chords(37, 2), PR.ring_with_chords(130, 3),
                                     PR.star_centre2(70), big_colour_graph(300))):
        out.append((rp, cl, weights_of(kind, n, rp, cl, 50 + i)))
    if terminals:
        out.insert(2, (np.array([0, 0], np.int64), np.zeros(0, np.int64), None if kind == "unit" else np.zeros(0, F32)))
    else:
        _n, rp, cl = PR.path_021()
        out.insert(2, (rp, cl, weights_of(kind, 3, rp, cl, 59)))
    return tuple(out)


def skipped(n, K, terminals):
    return n < PR.first_of(K, terminals)


def start_states(sizes, K, first, cands, seed):
    """[cands, R] int8: random classes, the terminals' own on the first `first` rows of every graph."""
    R = int(np.sum(sizes))
    A = np.random.RandomState(seed).randint(0, K, (cands, R)).astype(np.int8)
    lo = 0
    for n in sizes:
        m = min(first, int(n))
        A[:, lo:lo + m] = np.arange(m)
        lo += int(n)
    return A


def cost_of(kind, R, K, seed):
    if kind is None:
        return None
    if kind == "zero":
        return np.zeros((R, K), F32)
    return (np.random.RandomState(seed).uniform(-2.0, 2.0, (R, K)) * (1.0 + 2.0 ** -20)).astype(F32)


def mean_abs(graphs):
    vals = [np.abs(w) for _rp, cl, w in graphs if w is not None and len(w)]
    if not vals:
        return 1.0
    ones = sum(len(cl) for _rp, cl, w in graphs if w is None)
    return float((np.concatenate(vals).sum(dtype=np.float64) + ones) / (sum(v.size for v in vals) + ones))


def ladder(rungs, t_hot=1.5, t_cold=0.15, scale=1.0):
    """Testing.temper_ladder: geometric, float64 rounded once, hottest first."""
    r = np.arange(rungs, dtype=np.float64)
    return (1.0 / (scale * t_hot * (t_cold / t_hot) ** (r / max(rungs - 1, 1)))).astype(F32)


# ---- the cases of tests/test_gpu_temper.py (tests/test_temper_host.py counts the exchanges they make) ------------------------
def cands_of(spec, rungs):
    return {"r": rungs, "2r": 2 * rungs}.get(spec, spec)


#        K  terminals cost    weights   rungs cands rounds round_sweeps
CASES = [(2, False, None, "unit", 1, "r", 1, 1),
         (2, True, "zero", "signed", 2, "2r", 2, 3),
         (3, True, "real", "real", 3, 24, 5, 3),
         (3, False, None, "signed", 8, "r", 5, 1),
         (8, True, "real", "unit", 3, "2r", 2, 1),
         (8, False, "zero", "real", 8, 24, 5, 3),
         (2, True, "real", "signed", 8, "2r", 0, 1),
         (3, False, "real", "unit", 2, 24, 1, 3),
         (8, True, None, "real", 1, "2r", 5, 1),
         (2, False, "real", "real", 3, "r", 2, 3)]
