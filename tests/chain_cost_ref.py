"""CPU restatement of the two chain searches with per-node class costs (include/gcnmaxcut.h, gmc_kway_tabu_c_f32 and
gmc_kway_balance_c_f32), written from the header's text in numpy float32 and independent of the library.  It builds on
tests/tabu_ref.py and tests/balanced_ref.py by import (the hash draws, the move, the tie order, the sizes): the rules
are the twins' with the table started from the node's cost row, and the score is tests/node_cost_ref.py's - block_cut
minus block_cost in the device's own summation order.

``cost`` is [n, K] float32 by local id, or None.  With None, and with an all-zero array, `tabu` and `balanced` here equal
tabu_ref.tabu and balanced_ref.balanced output for output (tests/test_chain_cost_host.py)."""
import itertools

import numpy as np

from tests import balanced_ref as BR
from tests import node_cost_ref as NR
from tests import tabu_ref as TR
from tests.balanced_ref import _apply, _best, sizes, violation
from tests.tabu_ref import M64, draws

F = np.float32


def class_sums(n, rowptr, col, w, state, K, cost=None):
    """W [n, K] float32: tabu_ref.class_sums started from the node's cost row instead of +0.0, the row's weights added
    in CSR order; then the header's canonicalisation, one addition of +0.0 (a sum of -0.0 becomes +0.0)."""
    if cost is None:
        return TR.class_sums(n, rowptr, col, w, state, K)
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    ww = np.ones(col.size, F) if w is None else np.asarray(w, F)
    W = np.array(cost, F, copy=True).reshape(n, K)
    deg = np.diff(rowptr)
    for j in range(int(deg.max()) if n else 0):
        v = np.nonzero(deg > j)[0]
        e = rowptr[v] + j
        u = col[e]
        cu = np.asarray(state)[u].astype(np.int64)
        ok = (u != v) & (cu >= 0) & (cu < K)
        W[v[ok], cu[ok]] = W[v[ok], cu[ok]] + ww[e[ok]]    # one node once per j: a plain fp32 add each
    return W + F(0.0)


def tabu(n, rowptr, col, w, cost, state0, K, terminals, cand, iterations, tenure_base=3, tenure_span=0, tenure_div=10,
         seed=0):
    """One chain of gmc_kway_tabu_c_f32 -> tabu_ref.Result (trace None).  Steps 1-5 are tabu_ref.tabu's, word for word;
    only the table's start differs."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    ww = np.ones(col.size, F) if w is None else np.asarray(w, F)
    state = np.array(state0, np.int8).copy()
    snap = state.copy()
    first = K if terminals else 0
    n_mov = n - first
    best_it = moves = 0
    rel = best = F(0.0)
    if iterations > 0 and n_mov > 0:
        W = class_sums(n, rowptr, col, w, state, K, cost)
        until = np.zeros(n, np.int64)
        mov = np.arange(first, n)
        ks = np.arange(K)
        for it in range(iterations):
            r, tenure = draws(seed & M64, cand, it, n_mov, tenure_base, tenure_span, tenure_div)
            c = state[mov].astype(np.int64)
            in_class = (c >= 0) & (c < K)
            cc = np.where(in_class, c, 0)
            gain = W[mov, cc][:, None] - W[mov]           # [n_mov, K] float32, one subtraction each
            assert gain.dtype == F
            free = until[mov] <= it
            adm = in_class[:, None] & (ks[None, :] != cc[:, None]) & (free[:, None] | ((rel + gain) > best))
            pick = _best(gain, adm, (mov - first - r) % n_mov, K)
            if pick is None:
                continue
            i, k = pick
            v, c_v, g = int(mov[i]), int(cc[i]), gain[i, k]
            _apply(W, state, rowptr, col, ww, v, c_v, k)
            rel = F(rel + g)
            until[v] = it + 1 + tenure
            moves += 1
            if rel > best:
                best, best_it = rel, it + 1
                snap = state.copy()
    return TR.Result(snap, best_it, moves, best, None)


def balanced(n, rowptr, col, w, cost, state0, K, terminals, cand, lo, hi, iterations, tenure_base=3, tenure_span=0,
             tenure_div=10, seed=0):
    """One chain of gmc_kway_balance_c_f32 under lo, hi [K] -> balanced_ref.Result (trace None): balanced_ref.balanced's
    repair and iterations, word for word, on the table started from the cost rows.  The caller checks admits() first."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    ww = np.ones(col.size, F) if w is None else np.asarray(w, F)
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    state = np.array(state0, np.int8).copy()
    first = K if terminals else 0
    n_mov = n - first
    best_it = moves = repairs = 0
    rel = best = F(0.0)
    s, m = sizes(state, K, first)
    snap = state.copy()
    if n_mov > 0 and (iterations > 0 or violation(s, lo, hi) > 0):
        W = class_sums(n, rowptr, col, w, state, K, cost)
        mov = np.arange(first, n)
        ks = np.arange(K)
        off_diag = ks[:, None] != ks[None, :]

        def view():
            c = state[mov].astype(np.int64)
            in_class = (c >= 0) & (c < K)
            cc = np.where(in_class, c, 0)
            gain = W[mov, cc][:, None] - W[mov]               # [n_mov, K] float32, one subtraction each
            assert gain.dtype == F
            return in_class, cc, gain

        while violation(s, lo, hi) > 0:                       # ---- the repair
            da = np.where(s > hi, -1, np.where(s <= lo, 1, 0))
            db = np.where(s < lo, -1, np.where(s >= hi, 1, 0))
            lowers = (da[:, None] + db[None, :] < 0) & off_diag
            in_class, cc, gain = view()
            pick = _best(gain, in_class[:, None] & lowers[cc], mov - first, K)
            if pick is None:
                break
            i, b = pick
            v, a = int(mov[i]), int(cc[i])
            _apply(W, state, rowptr, col, ww, v, a, b)
            s[a] -= 1; m[a] -= 1; s[b] += 1; m[b] += 1
            repairs += 1
        snap = state.copy()
        until = np.zeros(n, np.int64)
        for it in range(iterations):                          # ---- the iterations
            r, tenure = draws(seed & M64, cand, it, n_mov, tenure_base, tenure_span, tenure_div)
            free_ab = (s > lo)[:, None] & (s < hi)[None, :] & off_diag
            paired_ab = ~free_ab & (m >= 1)[None, :] & off_diag
            in_class, cc, gain = view()
            unbanned = until[mov] <= it
            free_mv = in_class[:, None] & free_ab[cc]
            adm = (free_mv & (unbanned[:, None] | ((rel + gain) > best))) | \
                  (in_class[:, None] & paired_ab[cc] & unbanned[:, None])
            rank = (mov - first - r) % n_mov
            pick = _best(gain, adm, rank, K)
            if pick is None:
                continue
            i, b = pick
            v, a, g = int(mov[i]), int(cc[i]), gain[i, b]
            is_free = bool(free_ab[a, b])
            _apply(W, state, rowptr, col, ww, v, a, b)
            rel = F(rel + g)
            until[v] = it + 1 + tenure
            moves += 1
            if is_free:
                s[a] -= 1; m[a] -= 1; s[b] += 1; m[b] += 1
            else:
                in_class, cc, gain = view()                   # from the updated table
                ok = np.zeros((n_mov, K), bool)
                ok[:, a] = in_class & (cc == b) & (mov != v)
                i2, _a2 = _best(gain, ok, rank, K)            # m[b] >= 1: it exists
                u, g2 = int(mov[i2]), gain[i2, a]
                _apply(W, state, rowptr, col, ww, u, b, a)
                rel = F(rel + g2)
                until[u] = it + 1 + tenure
            if rel > best:
                best, best_it = rel, it + 1
                snap = state.copy()
    return BR.Result(snap, best_it, moves, repairs, best, None)


def score(n, rowptr, col, w, cost, a, K):
    """The score of a snapshot in the device's order: node_cost_ref.score."""
    return NR.score(n, rowptr, col, w, cost, a, K)


def run(n, rowptr, col, w, cost, A, K, terminals, iterations, bounds=None, tenure=(3, 0, 10), seed=0):
    """Every candidate of A [cands, n] int8 for one graph, as the entry points report it: a dict of assign [cands, n]
    int8, best_iter, moves (and repairs with bounds) [cands] int32, cut_all [cands] float32 in the device's order and
    the pick (best_idx, best_cut, best_assign int32: strictly best, first on ties).  bounds: (lo, hi) [K], or None for
    gmc_kway_tabu_c_f32."""
    A = np.asarray(A, np.int8)
    if bounds is None:
        res = [tabu(n, rowptr, col, w, cost, A[i], K, terminals, i, iterations, *tenure, seed) for i in range(len(A))]
    else:
        res = [balanced(n, rowptr, col, w, cost, A[i], K, terminals, i, bounds[0], bounds[1], iterations, *tenure, seed)
               for i in range(len(A))]
    out = dict(assign=np.stack([x.assign for x in res]), best_iter=np.asarray([x.best_it for x in res], np.int32),
               moves=np.asarray([x.moves for x in res], np.int32))
    if bounds is not None:
        out["repairs"] = np.asarray([x.repairs for x in res], np.int32)
    out["cut_all"] = np.asarray([score(n, rowptr, col, w, cost, a, K) for a in out["assign"]], F)
    bi = 0
    for i in range(1, len(A)):                                # strict '>' keeps the first best
        if out["cut_all"][i] > out["cut_all"][bi]:
            bi = i
    out.update(best_idx=bi, best_cut=out["cut_all"][bi], best_assign=out["assign"][bi].astype(np.int32))
    return out


# ---- small instances and their optima -----------------------------------------------------------------------------------
def drawn_instance(seed, n, K):
    """node_cost_ref.drawn_instance's graph (the ring plus chords, integer weights in -2..2 without 0) with integer costs
    in -3..3 for K classes: (rowptr, col, w float32, cost [n, K] float32, edges, quad, lin).  The last three are the QUBO
    reading at K = 2 (node_cost_ref.qubo_to_maxcut gives its own w and cost)."""
    _n, edges, quad, lin = NR.drawn_instance(seed, n)
    rowptr, col, w = NR.csr_of_edges(n, edges, quad)
    cost = np.random.RandomState(5000 + seed).randint(-3, 4, size=(n, K)).astype(F)
    return rowptr, col, w, cost, edges, quad, lin


def brute_force_max(n, K, rowptr, col, w, cost, lo, hi):
    """The largest cut - cost (float64; exact for integer data) over the partitions whose class sizes are within lo, hi."""
    best = -float("inf")
    for a in itertools.product(range(K), repeat=n):
        a = np.asarray(a)
        s = np.bincount(a, minlength=K)
        if (s >= lo).all() and (s <= hi).all():
            best = max(best, NR.objective64(rowptr, col, w, cost, a, K))
    return best


# (seed, n, K) of drawn_instance on which tests/test_chain_cost_host.py asserts the brute-force optimum: seeds 0..11,
# n cycling through 6..10 at K = 2 and 6..8 at K = 3 (3^8 = 6561 partitions to enumerate), none left out.
BRUTE_INSTANCES = tuple((s, 6 + s % 5, 2) for s in range(6)) + tuple((s, 6 + s % 3, 3) for s in range(6, 12))
